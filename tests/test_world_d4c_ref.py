"""The numpy restatement of D4C (tests/world_d4c_ref.py) over the inputs of the analysis tests (tests/world_analysis_cases.py), on the CPU: every
frame an emulator or GPU test of D4C runs keeps its integer decisions and its Love-Train ratio clear of the points where they flip, both branches
(on / off) are live, and the restatement is what it says (off rows, the ends of a row, code_aperiodicity, float64 against longdouble)."""
import numpy
import pytest

import world_analysis_cases as C
import world_d4c_cases as D
import world_d4c_ref as R

LENGTHS = sorted(set(C.LENGTHS_GPU) | set(C.LENGTHS_EMU))
BAR_A0, BAR_COARSE, BAR_AP = D.bars()


@pytest.mark.parametrize('fs', C.RATES)
@pytest.mark.parametrize('kind', C.TRACKS)
def test_every_voiced_frame_is_clear_of_its_rounding_flips(fs, kind):
    """A condition on the inputs: 1.5 fs / f, 2 fs / f, the three origins (t -+ 0.25 / f) fs + 0.001, f N / fs and (f / 2) N / fs are at least 1e-6 away from
    where their rounding flips, in every voiced frame, none excluded."""
    worst = [numpy.inf] * 7
    for n in LENGTHS:
        for a, b in zip(C.f0_track(kind, n), C.times(n)):
            if a != 0:
                worst = [min(p, q) for p, q in zip(worst, R.rounding_margins(a, b, fs))]
    print(fs, kind, worst)
    assert min(worst) >= D.MARGIN, worst


@pytest.mark.parametrize('fs', C.RATES)
@pytest.mark.parametrize('wk', C.WAVES)
def test_every_voiced_frame_is_clear_of_the_threshold(fs, wk):
    """|a0 - 0.85| >= 1e-6 with the float64 restatement and the seed the D4C tests use, in every voiced frame, none excluded."""
    worst = numpy.inf
    for tk in C.TRACKS:
        for n in LENGTHS:
            x, f0, t = C.case(wk, tk, n, fs)
            for a, b in zip(f0, t):
                if a != 0:
                    worst = min(worst, abs(float(R.love_train(x, a, b, fs, seed=D.SEED)) - R.THRESHOLD))
    print(fs, wk, 'closest |a0 - threshold|', worst)
    assert worst >= D.MARGIN, worst


@pytest.mark.parametrize('fs', C.RATES)
def test_both_branches_are_live(fs):
    x, f0, t = C.case('glide', 'glide', 201, fs)
    on = R.d4c(x, f0, t, fs, seed=D.SEED, details=True)[2]
    assert on.sum() >= 150, on.sum()
    x, f0, t = C.case('noise', 'glide', 201, fs)
    assert not R.d4c(x, f0, t, fs, seed=D.SEED, details=True)[2].any()


@pytest.mark.parametrize('fs', C.RATES)
def test_the_restatement_is_what_it_says(fs):
    assert R.fft_size_d4c(fs) == R.fft_size_love_train(fs) == 2048 and R.bands(fs) == {16000: 1, 24000: 3}[fs]
    x, f0, t = C.case('glide', 'alternating', 40, fs)
    ap, a0, on, coarse = R.d4c(x, f0, t, fs, seed=D.SEED, details=True)
    assert on.any() and not on[1::2].any() and (a0[1::2] == 0).all()
    assert ap.shape == (40, 513) and numpy.isfinite(ap).all()
    assert (ap[~on] == 1.0 - 1e-12).all()                                         # off rows, exactly
    assert numpy.abs(ap[on][:, 0] - 1e-3).max() <= 1e-18 and (ap[on] > 0).all() and (ap[on] < 1).all()
    assert (coarse[on] <= 0).all() and (coarse[on] > -60).all()
    coded = R.code_aperiodicity(ap, fs)
    assert coded.shape == (40, R.bands(fs)) and numpy.abs(coded[on] - coarse[on]).max() <= 1e-9
    assert numpy.array_equal(R.d4c(x, f0[[7, 2]], t[[7, 2]], fs, seed=D.SEED), ap[[2 + 5, 2]])        # a row depends on its own frame only
    hi = R.d4c(x, f0, t, fs, seed=D.SEED, dtype=numpy.longdouble, details=True)
    assert numpy.array_equal(hi[2], on)
    e = (float(numpy.abs(a0 - hi[1]).max()), float(numpy.abs(coarse[on] - hi[3][on]).max()),
         float(numpy.abs(20 * numpy.log10(ap.astype(numpy.longdouble)) - 20 * numpy.log10(hi[0])).max()))
    print(fs, 'float64 against longdouble: a0 %.3g (bar %.3g) coarse %.3g (bar %.3g) ap %.3g (bar %.3g)' % (e[0], BAR_A0, e[1], BAR_COARSE, e[2], BAR_AP))
    assert e[0] <= BAR_A0 and e[1] <= BAR_COARSE and e[2] <= BAR_AP


def test_rounding_and_noise_keys():
    assert [R.mround(v) for v in (2.5, -2.5, 0.49, -0.49, -0.5, 0.0, -127.6)] == [3, -3, 0, 0, -1, 0, -128]
    assert R.frame_integers(80.0, 0.0, 16000)[2] < 0                              # the window at t - 0.25 / f starts before the wave
    # the keys of the four windows of one frame are disjoint, and disjoint from CheapTrick's (centre x 2048 + 0 .. 1536) of any frame
    h3, h4, om, oc, op = R.frame_integers(47.5, 0.0, 24000)[:5]
    spans = [(R.KEY_BASE + (o + R.KEY_BIAS) * R.KEY_ORIGIN + w * R.KEY_WINDOW, 2 * h + 1) for o, w, h in ((oc, 0, h3), (om, 1, h4), (op, 2, h4), (oc, 3, h4))]
    assert all(n <= R.KEY_WINDOW for _, n in spans) and len({s for s, _ in spans}) == 4
    assert min(s for s, _ in spans) >= 1 << 62 and max(s + n for s, n in spans) < 1 << 63
    x, f0, t = C.case('zeros', 'alternating', 12, 16000)
    a, b = R.d4c(x, f0, t, 16000, seed=1, details=True), R.d4c(x, f0, t, 16000, seed=2, details=True)
    assert numpy.isfinite(a[0]).all() and not numpy.array_equal(a[1], b[1])     # the noise term is live


# ---- the inputs at the edges of the domain (tests/world_domain_cases.py, run by tests/test_world_domain_*.py) ----
import world_domain_cases as DC

DOMAIN_FRAMES = sorted(set(DC.FRAMES_GPU) | set(DC.FRAMES_EMU))


@pytest.mark.parametrize('fs', DC.D4C_RATES)
@pytest.mark.parametrize('kind', DC.D4C_TRACKS)
def test_every_domain_frame_is_clear_of_its_rounding_flips(fs, kind):
    worst = [numpy.inf] * 7
    for n in DOMAIN_FRAMES:
        for a, b in zip(DC.f0_track(kind, n, fs), DC.times(kind, n)):
            worst = [min(p, q) for p, q in zip(worst, R.rounding_margins(a, b, fs))]
    print(fs, kind, worst)
    assert min(worst) >= D.MARGIN, worst


@pytest.mark.parametrize('fs', DC.D4C_RATES)
@pytest.mark.parametrize('wk', DC.WAVES)
def test_every_domain_frame_is_clear_of_the_threshold(fs, wk):
    worst = numpy.inf
    for tk in DC.D4C_TRACKS:
        for n in DOMAIN_FRAMES:
            x, f0, t = DC.case(wk, tk, n, fs)
            for a, b in zip(f0, t):
                worst = min(worst, abs(float(R.love_train(x, a, b, fs, seed=DC.SEED)) - DC.threshold(tk)))
    print(fs, wk, 'closest |a0 - threshold|', worst)
    assert worst >= D.MARGIN, worst


@pytest.mark.parametrize('fs', DC.D4C_RATES)
def test_the_domain_tracks_reach_the_bounds_they_are_there_for(fs):
    h3, h4, om, oc, op, L, b1, b2 = R.frame_integers(DC.f0_track('high', 1, fs)[0], 0.0, fs)
    assert (L, b1, b2) == (1023, 1024, 512) and 1025 + 2 * b1 == 3073
    low = DC.f0_track('lowest47', 13, fs)
    assert (low[0::2] > 47.0).all() and (low[0::2] < 47.1).all() and (low[1::2] > 40.0).all() and (low[1::2] < 47.0).all()
    assert 2 * R.frame_integers(low[1], 0.0, 24000)[1] + 1 == 2043                              # of 2048
    on = [R.d4c(*DC.case('glide', tk, 13, fs), fs, threshold=DC.threshold(tk), seed=DC.SEED, details=True)[2] for tk in DC.D4C_TRACKS]
    print(fs, 'frames on:', [int(o.sum()) for o in on])
    assert sum(int(o.sum()) for o in on) >= 13 and on[1][0] and not on[1].all()                                  # the general body is live, at the top of `high` too
