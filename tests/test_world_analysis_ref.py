"""The numpy restatement of CheapTrick / sp2mc (tests/world_analysis_ref.py) and the inputs of the analysis tests (tests/world_analysis_cases.py), on
the CPU: every frame a CPU or GPU test runs keeps its integer decisions clear of the point where they flip, the restatement is finite on silence,
`sp2mc` inverts the independent checker oracle/mc2sp.py, and `freqt` cannot tell 513 cepstral values from 1024."""
from fractions import Fraction

import numpy
import pytest

import world_analysis_cases as C
import world_analysis_ref as R
from oracle import mc2sp as O

LENGTHS = sorted(set(C.LENGTHS_GPU) | set(C.LENGTHS_EMU) | {2000})          # 2000: the frames of the poison test's large call


def exact(num, den):
    """True when num / den (integers) is a whole number: the float64 quotient is then exact, nothing is rounded and no decision can flip."""
    return Fraction(num, den).denominator == 1


@pytest.mark.parametrize('fs', C.RATES)
@pytest.mark.parametrize('kind', C.TRACKS)
def test_every_case_frame_is_clear_of_its_rounding_flips(fs, kind):
    """A condition on the inputs, not a measurement: 1.5 fs / f0, t fs + 0.001, f0 fft_size / fs (and the smoothing width in bins, the fourth integer
    the kernel decides) are at least 1e-6 away from where their rounding flips.  The one exception is arithmetic that does not round at all: the
    prescribed 500 Hz of an unvoiced frame at 16 kHz gives f0 fft_size / fs = 32 exactly (512000 / 16000 in integers)."""
    floor = C.f0_floor(kind)
    worst = [numpy.inf] * 4
    for n in LENGTHS:
        f0, t = C.f0_track(kind, n), C.times(n)
        for a, b in zip(f0, t):
            m = list(R.rounding_margins(a, b, fs, 1024, floor))
            used = R.frame_integers(a, b, fs, 1024, floor)[0]
            if m[2] < 1e-6 and used == int(used) and exact(int(used) * 1024, fs):
                m[2] = numpy.inf
            worst = [min(p, q) for p, q in zip(worst, m)]
    print(fs, kind, worst)
    assert min(worst) >= 1e-6, worst


def test_the_prescribed_tracks_are_what_they_say():
    for fs in C.RATES:
        assert all(R.frame_integers(f, 0.0, fs, 1024, 71.0)[0] == 500.0 for f in C.f0_track('below', 50))
        assert R.frame_integers(71.0, 0.0, fs, 1024, 71.0)[0] == 500.0              # 71 Hz is not above a floor of 71 Hz
        assert R.frame_integers(71.0, 0.0, fs, 1024, C.f0_floor('f71'))[0] == 71.0
        assert 2 * R.frame_integers(71.0, 0.0, fs, 1024, 60.0)[1] + 1 <= 1021
    g = C.f0_track('glide', 400)
    assert g[0] == 80.0 and 390 < g[-1] < 400 and (numpy.diff(g) > 0).all()
    assert C.wave_length('short', 40, 16000) < 2 * R.frame_integers(800.0, 0.0, 16000, 1024, 71.0)[1] + 1
    assert C.times(400)[-1] * 16000 > C.wave_length('glide', 400, 16000)            # frames behind the end of the wave


@pytest.mark.parametrize('fs', C.RATES)
def test_silence_is_finite(fs):
    x, f0, t = C.case('zeros', 'alternating', 12, fs)
    sp = R.cheaptrick(x, f0, t, fs, seed=1)
    assert numpy.isfinite(sp).all() and (sp > 0).all()
    assert numpy.isfinite(R.sp2mc(sp, 8, 0.41)).all()
    assert not numpy.array_equal(sp, R.cheaptrick(x, f0, t, fs, seed=2))            # the noise terms are live


def test_a_row_depends_on_its_own_frame_only():
    x, f0, t = C.case('glide', 'glide', 12, 16000)
    full = R.cheaptrick(x, f0, t, 16000, seed=3)
    assert numpy.array_equal(R.cheaptrick(x, f0[[7, 2]], t[[7, 2]], 16000, seed=3), full[[7, 2]])


@pytest.mark.parametrize('fs,alpha', [(16000, 0.41), (24000, 0.466)])
def test_sp2mc_inverts_the_independent_mc2sp(fs, alpha):
    """The round trip through oracle/mc2sp.py (the closed form; shares nothing with the restatement).  Bar: 513 cepstral values of size <= 1 pass a
    1024-point float64 transform (relative error of a few eps log2(1024)) and a recursion that sums them with weights below 1 / (1 - alpha): 1e-12
    relative is a hundred times that and a million times below anything a wrong step would leave."""
    mc0 = numpy.random.default_rng(9).normal(0.0, 0.3, (6, 9))
    mc0[:, 0] -= 4.0
    back = R.sp2mc(O.mc2sp(mc0, alpha, 1024), 8, alpha)
    e = numpy.abs(back - mc0).max() / numpy.abs(mc0).max()
    print('round trip', e)
    assert e <= 1e-12


def test_freqt_cannot_tell_513_values_from_1024():
    x, f0, t = C.case('glide', 'glide', 5, 24000)
    sp = R.cheaptrick(x, f0, t, 24000)
    for alpha in (0.41, 0.466):
        assert numpy.array_equal(R.sp2mc(sp, 8, alpha), R.sp2mc(sp, 8, alpha, all_values=True))


def test_the_longdouble_transform_is_a_transform():
    a = numpy.random.default_rng(1).normal(size=1024)
    got = R.fft_any(a.astype(numpy.longdouble), numpy.longdouble)
    assert numpy.abs(got - numpy.fft.fft(a)).max() <= 1e-11


# ---- the inputs at the edges of the domain (tests/world_domain_cases.py, run by tests/test_world_domain_*.py) ----
import world_domain_cases as DC

DEFAULT_F0 = 500.0
DOMAIN_FRAMES = sorted(set(DC.FRAMES_GPU) | set(DC.FRAMES_EMU))


def _margins(f0_k, t_k, fs, floor):
    """`rounding_margins`, with the exception of the first test of this file: a 500 Hz frame whose f0 fft_size / fs is a whole number in integers."""
    m = list(R.rounding_margins(f0_k, t_k, fs, 1024, floor))
    used = R.frame_integers(f0_k, t_k, fs, 1024, floor)[0]
    if m[2] < 1e-6 and used == DEFAULT_F0 and exact(500 * 1024, fs):
        m[2] = numpy.inf
    return m


@pytest.mark.parametrize('fs', DC.RATES)
@pytest.mark.parametrize('kind', DC.TRACKS)
def test_every_domain_frame_is_clear_of_its_rounding_flips(fs, kind):
    """The same condition, the same 1e-6, on the `lowest` / `high` / `offgrid` frames at every rate, none excluded."""
    worst = [numpy.inf] * 4
    for n in DOMAIN_FRAMES:
        for a, b in zip(DC.f0_track(kind, n, fs), DC.times(kind, n)):
            worst = [min(p, q) for p, q in zip(worst, _margins(a, b, fs, DC.FLOOR))]
    print(fs, kind, worst)
    assert min(worst) >= 1e-6, worst


@pytest.mark.parametrize('floor', DC.FLOORS + (DC.FLOOR,))
def test_the_glide_frames_are_clear_of_their_flips_at_the_other_floors(floor):
    for n in DOMAIN_FRAMES:
        for a, b in zip(C.f0_track('glide', n), C.times(n)):
            assert min(_margins(a, b, 16000, floor)) >= 1e-6


@pytest.mark.parametrize('fs', DC.RATES)
def test_the_domain_tracks_reach_the_bounds_they_are_there_for(fs):
    floor = R.effective_floor(fs, 1024, DC.FLOOR)
    for n in DOMAIN_FRAMES:
        low = [R.frame_integers(f, 0.0, fs, 1024, DC.FLOOR) for f in DC.f0_track('lowest', n, fs)]
        assert all(v[0] != 500.0 and v[0] < floor * 1.002 for v in low)                         # voiced, within 0.2 % of the floor in force
        if fs >= 16000:
            assert all(2 * v[1] + 1 == 1021 for v in low)                                       # the longest window there is
        f0, h, centre, L, b, u = R.frame_integers(DC.f0_track('high', n, fs)[0], 0.0, fs, 1024, DC.FLOOR)
        assert f0 < 0.5 * fs and f0 * 1024 / fs > 511.5 and L == 511 and b == 342 and 513 + 2 * b <= 1280
        t = DC.times('offgrid', n)
        assert t[0] == -1.0 and t.min() >= -1.0 and t.max() <= 1e6 and (n < 2 or t[-1] == 1e6)
    t = DC.times('offgrid', 13)
    assert (t[1:3] < 0).all() and t[1:].min() > -0.013 and (t[-3:] > 3.0).all()
    assert numpy.abs((t[1:-3] / C.FRAME_PERIOD) % 1 - 0.5).max() < 0.5                          # off the 5 ms grid
    assert max(abs(a) for a in DC.ALPHAS) == 0.9 and min(DC.Q1) == -0.4 and max(DC.Q1) == 0.0 and set(DC.ORDERS) >= {0, 63}


def test_sp2mc_rows_is_sp2mc_bit_for_bit():
    for order, alpha in ((0, 0.0), (1, -0.9), (8, 0.41), (63, 0.9)):
        sp = DC.sp2mc_rows(order, alpha)[:3]
        assert numpy.array_equal(R.sp2mc_rows(sp, order, alpha), R.sp2mc(sp, order, alpha))
