"""The numpy restatement of WORLD synthesis (tests/world_synth_ref.py) against known answers, its streaming form against its one-shot form,
and the vetting of the f0 tracks the GPU test runs (CPU, no kernel)."""
import numpy
import pytest

import world_synth_cases as C
import world_synth_ref as R

FS = 16000


def flat(n, c=1e-4, a=0.001):
    return numpy.full((n, 513), c), numpy.full((n, 513), a)


def test_noise_is_a_pure_function_of_seed_and_position():
    k = numpy.arange(100000)
    g = R.noise(7, k)
    assert numpy.array_equal(g[1234:1300], R.noise(7, k[1234:1300])) and not numpy.array_equal(g, R.noise(8, k))
    assert numpy.array_equal(g * 2 ** 24, numpy.round(g * 2 ** 24)) and g.min() >= -6 and g.max() < 6
    assert abs(g.mean()) < 0.02 and abs(g.var() - 1) < 0.02
    big = R.noise(7, numpy.array([2 ** 33 + 5, 5]))               # positions beyond 32 bits are their own samples
    assert big[0] != big[1]


def test_flat_spectrum_periodic_f0_gives_impulses():
    """sp = c, ap at its floor, f0 = fs / 100: pulses exactly every 100 samples, every periodic response a DC-corrected impulse of height
    sqrt(c (1 - ap^2) period) at the pulse."""
    n, period, c = 60, 100, 1e-4
    sp, ap = flat(n, c)
    y, P, _ = R.synthesize(numpy.full(n, FS / period), sp, ap, FS, return_pulses=True)
    idx = numpy.array([p[0] for p in P])
    assert len(y) == R.y_length(n, FS, 5.0) == 4721
    assert numpy.array_equal(numpy.diff(idx), numpy.full(len(idx) - 1, period)) and idx[0] == period - 1
    assert all(p[2] for p in P) and max(abs(p[1]) for p in P) < 1e-9
    per, aper = R.pulse_response(int(idx[3]), P[3][1], True, period, sp, ap, 0, n - 1, FS, 5.0, 1024, 0, parts=True)
    amp = numpy.sqrt((c * (1 - 0.001 ** 2) + 1e-12) * period)
    rem = R.dc_remover(1024)
    want = numpy.zeros(1024)
    want[512] = numpy.sqrt(c * (1 - 0.001 ** 2) + 1e-12)          # flat log spectrum: the minimum phase is an impulse at time 0
    want = (want - want[512] * rem) * numpy.sqrt(period)
    assert numpy.abs(per - want).max() < 1e-12 * amp + 1e-18
    assert abs(per[512] - amp * (1 - rem[512])) < 1e-12 * amp
    assert numpy.abs(aper).max() < 0.02 * amp                     # ap at its floor: the noise part is 1e-3 of the spectrum


def test_all_unvoiced_is_a_500_hz_grid_with_the_power_of_sp():
    n = 200
    for fs, step in ((16000, 32), (24000, 48)):
        sp, ap = flat(n, 4e-4, 0.5)
        y, P, _ = R.synthesize(numpy.zeros(n), sp, ap, fs, seed=5, return_pulses=True)
        idx = numpy.array([p[0] for p in P])
        assert numpy.array_equal(numpy.diff(idx), numpy.full(len(idx) - 1, step)) and not any(p[2] for p in P)
        core = y[2000:-2000]
        assert abs(core.var() / 4e-4 - 1) < 0.1                   # white noise of variance sp (unvoiced: sp alone shapes it)
        y4 = R.synthesize(numpy.zeros(n), 4 * sp, ap, fs, seed=5)
        assert numpy.abs(y4 - 2 * y).max() <= 1e-12 * numpy.abs(y).max()


def test_ap_near_one_has_no_periodic_part_and_seeds_matter_only_through_noise():
    n = 40
    f0 = numpy.full(n, 200.0)
    sp, _ = flat(n)
    ones = numpy.ones((n, 513))
    P = R.synthesize(f0, sp, ones, FS, return_pulses=True)[1]
    per, aper = R.pulse_response(P[5][0], P[5][1], True, 80, sp, ones, 0, n - 1, FS, 5.0, 1024, 0, parts=True)
    assert not per.any() and aper.any()
    lo = numpy.full((n, 513), 0.001)
    a, b = R.synthesize(f0, sp, lo, FS, seed=1), R.synthesize(f0, sp, lo, FS, seed=2)
    assert numpy.abs(a - b).max() < 0.01 * numpy.abs(a).max() and not numpy.array_equal(a, b)


def test_one_frame_silence_and_scaling():
    sp, ap = flat(1)
    y = R.synthesize([150.0], sp, ap, FS)
    assert y.shape == (1,) and y[0] == 0.0
    n = 50
    rng = numpy.random.default_rng(0)
    f0 = C.f0_track('glide', n, FS)
    ap = C.aperiodicity(n).astype(numpy.float64)
    quiet = R.synthesize(f0, numpy.full((n, 513), 1e-16), ap, FS)
    assert numpy.isfinite(quiet).all() and numpy.abs(quiet).max() < 1e-5
    sp = numpy.exp(rng.normal(-6, 1.5, (n, 513)))
    y1, y2 = R.synthesize(f0, sp, ap, FS, seed=3), R.synthesize(f0, 2 * sp, ap, FS, seed=3)
    assert numpy.abs(y2 - numpy.sqrt(2) * y1).max() < 1e-6 * numpy.abs(y1).max()       # the 1e-12 safeguard is not scaled


def test_length_formula():
    for fs in C.RATES:
        for n in C.LENGTHS:
            assert len(R.synthesize(numpy.zeros(n), *flat(n), fs)) == int((n - 1) * 5.0 / 1000 * fs) + 1


@pytest.mark.parametrize('cuts', [[1] * 60, [100], [7, 13, 40, 1, 39], [59, 41], [2, 98]])
def test_stream_equals_one_shot_bit_for_bit(cuts):
    n = sum(cuts)
    f0, sp, ap = C.case('glide', n, 24000)
    want = R.synthesize(f0, sp, ap, 24000, seed=9)
    s = R.Stream(24000, 5.0, seed=9)
    out, i, lag = [], 0, 0
    for c in cuts:
        out.append(s.push(f0[i:i + c], sp[i:i + c], ap[i:i + c]))
        i += c
        lag = max(lag, R.y_length(i, 24000, 5.0) - s.done)
    out.append(s.flush())
    assert numpy.array_equal(numpy.concatenate(out), want)
    assert lag <= R.lag_samples(24000, f0=24000 / 1024 + 1) + 1           # half a transform + a frame + the longest pulse period


@pytest.mark.parametrize('fs', C.RATES)
@pytest.mark.parametrize('kind', C.TRACKS)
def test_gpu_tracks_keep_clear_of_the_wrap_threshold(kind, fs):
    """The tracks of tests/test_world_synth_gpu.py, before a GPU sees them: no wrap decision of the restatement within 1e-9 rad of 2 pi --
    except the prescribed constant-f0 tracks (unvoiced 500 Hz, 71 Hz, 800 Hz), whose phase returns to a whole number of turns and which
    therefore sit ON the threshold by construction: for them equality of the indices rests on identical IEEE-754 operations, and this
    test pins that they do sit there."""
    n = 2000
    f0 = C.f0_track(kind, n, fs)
    cf0 = R.coarse_f0(f0, fs, 1024)
    f, v = R.sample_f0(cf0, 0, R.y_length(n, fs, 5.0), fs, 5.0, n - 1)
    scan = R.PulseScan(fs)
    pulses = scan.feed(f, v)
    assert len(pulses) > 100
    if kind in C.CONSTANT:
        assert scan.min_margin < 1e-9
        if kind in C.ON_GRID:
            assert len(set(numpy.diff([p[0] for p in pulses]))) == 1      # and the grid is exactly periodic all the same
    else:
        assert scan.min_margin > 1e-9, scan.min_margin
    if kind == 'below':
        assert not all(p[2] for p in pulses) and (cf0 == 0).any()
    if kind == 'above':
        assert (cf0 > 0).all()


# ---- the inputs at the edges of the domain (tests/world_domain_cases.py, run by tests/test_world_domain_*.py) ----
import world_domain_cases as DC


@pytest.mark.parametrize('fs,fp', DC.CONFIGS)
@pytest.mark.parametrize('kind', DC.SYNTH_TRACKS)
def test_domain_tracks_keep_clear_of_the_wrap_threshold(kind, fs, fp):
    """Every (track, rate, frame period, frame count) tests/test_world_domain_*.py runs: no wrap decision within 1e-9 rad of 2 pi, none excluded."""
    spf = fs * fp / 1000
    for n in sorted(set(DC.SYNTH_FRAMES_GPU) | set(DC.SYNTH_FRAMES_EMU)):
        n = DC.synth_frames(n, fs, fp)
        f0 = DC.synth_f0(kind, n, fs)
        assert (f0 < 0.5 * fs).all()
        cf0 = R.coarse_f0(f0, fs, 1024)
        f, v = R.sample_f0(cf0, 0, R.y_length(n, fs, fp), fs, fp, n - 1)
        scan = R.PulseScan(fs)
        pulses = scan.feed(f, v)
        assert scan.min_margin > 1e-9, (n, scan.min_margin)
        if n >= 40:
            assert len(pulses) >= 2
            if kind == 'high':
                assert {2, 3} <= set(numpy.diff([p[0] for p in pulses]).tolist())
            if kind == 'below':
                assert (cf0 == 0).any() and (cf0 != 0).any()
            if kind == 'above':
                assert (cf0 > 0).all()
    assert DC.synth_frames(12, 16000, 0.0625) == 881 == R.y_length(12, 16000, 5.0) and spf >= 1.0


@pytest.mark.parametrize('fs,fp', DC.CONFIGS)
def test_the_restated_stream_equals_one_shot_at_inexact_frame_lengths(fs, fp):
    n = DC.synth_frames(12, fs, fp)
    f0, sp, ap = DC.synth_case('glide', n, fs)
    want = R.synthesize(f0, sp, ap, fs, fp, seed=9, fft_size=1024)
    for cuts in ([1] * n, [5, n - 5]):
        s = R.Stream(fs, fp, seed=9, fft_size=1024)
        out, i = [], 0
        for c in cuts:
            out.append(s.push(f0[i:i + c], sp[i:i + c], ap[i:i + c]))
            i += c
        out.append(s.flush())
        assert numpy.array_equal(numpy.concatenate(out), want)


def test_a_frame_count_whose_last_sample_wraps_exists():
    n = DC.frames_ending_on_a_wrap()
    assert 200 <= n < 232 and R.y_length(n, 16000, 0.0625) == n
