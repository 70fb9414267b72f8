"""Seeded inputs of the WORLD analysis tests (tests/test_world_analysis_*.py) and of the tolerance measurement
(scripts/analysis_tolerance.py): one place, so that the CPU test can vet the frames a GPU test will run."""
import numpy

RATES = (16000, 24000)
WAVES = ('glide', 'noise', 'zeros', 'click', 'short')
TRACKS = ('glide', 'unvoiced', 'below', 'f71', 'f800', 'alternating')
LENGTHS_GPU = (1, 2, 201, 400)
LENGTHS_EMU = (1, 2, 23, 40)
FRAME_PERIOD = 0.005
ORDER = 8
SEED = 5


def f0_track(kind, n):
    k = numpy.arange(n)
    glide = 80.0 * 5.0 ** (k / max(n - 1, 1) * 0.9973)             # 80 -> just under 400 Hz, no round numbers on the way
    if kind == 'glide':
        return glide
    if kind == 'unvoiced':
        return numpy.zeros(n)
    if kind == 'below':                                            # below every floor (71 Hz; 3 fs / 1021 = 47.0 / 70.5 Hz): analysed at 500 Hz
        return numpy.full(n, 40.0 + 0.0137 * k)
    if kind == 'f71':                                              # run with a floor of 60 Hz (`f0_floor` below): voiced, the longest windows there are
        return numpy.full(n, 71.0)
    if kind == 'f800':
        return numpy.full(n, 800.0)
    if kind == 'alternating':
        return numpy.where(k % 2 == 0, glide, 0.0)
    raise ValueError(kind)


def f0_floor(track_kind):
    """The floor the tests hand over with a track: 60 Hz for 'f71' (so that 71 Hz frames are voiced -- the longest windows -- at 16 kHz;
    at 24 kHz the floor in force is 3 fs / 1021 = 70.52 Hz), WORLD's default 71 Hz otherwise.  fft_size is always given as 1024."""
    return 60.0 if track_kind == 'f71' else 71.0


def times(n):
    """Frame k at k x 5 ms: the first frame sits at t = 0, the last ones behind the end of the wave (`wave_length`)."""
    return numpy.arange(n) * FRAME_PERIOD


def wave_length(kind, n, fs):
    if kind == 'short':
        return 37                                                  # shorter than any window (2 h + 1 >= 61): clamped on both sides
    return max(int(0.9 * (n - 1) * FRAME_PERIOD * fs), 200)        # the last tenth of the frames lies behind the end


def wave(kind, n, fs, seed=77):
    m = wave_length(kind, n, fs)
    rng = numpy.random.default_rng(seed)
    if kind == 'zeros':
        return numpy.zeros(m)
    if kind in ('noise', 'short'):
        return rng.normal(0.0, 0.1, m)
    if kind == 'click':
        x = numpy.zeros(m)
        x[m // 3] = 1.0
        return x
    if kind == 'glide':                                            # harmonics of an 80 -> 400 Hz glide under a formant-like envelope, a breath of noise
        f = 80.0 * 5.0 ** (numpy.arange(m) / max(m - 1, 1))
        phase = 2.0 * numpy.pi * numpy.cumsum(f) / fs
        x = numpy.zeros(m)
        for k in range(1, int(0.47 * fs / 80.0) + 1):
            fk = k * f
            amp = 0.02 + sum(g / (1.0 + ((fk - F) / B) ** 2) for F, B, g in ((700.0, 90.0, 1.0), (1250.0, 110.0, 0.6), (2600.0, 160.0, 0.35), (3600.0, 220.0, 0.2)))
            x += numpy.where(fk < 0.47 * fs, amp, 0.0) * numpy.sin(k * phase)
        return 0.05 * x + rng.normal(0.0, 1e-3, m)
    raise ValueError(kind)


def case(wave_kind, track_kind, n, fs):
    """-> x, f0, t"""
    return wave(wave_kind, n, fs), f0_track(track_kind, n), times(n)
