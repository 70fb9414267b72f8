"""Seeded inputs at the edges of what the WORLD units of the C ABI accept (tests/test_world_domain_*.py, scripts/world_domain_tolerance.py):
one place, so that the CPU tests (tests/test_world_*_ref.py) can vet every frame and track before an emulator or GPU test runs it.
The waves, the `glide` / `below` / `above` tracks and the spectrogram / aperiodicity rows are those of tests/world_analysis_cases.py and
tests/world_synth_cases.py; what is new is where the f0, the frame times, the rates and the frame periods sit.

The domain (INTEGRATION.md sections 10 and 11): synthesis 8000 <= fs <= 48000, fs * frame_period / 1000 >= 1, f0 < fs / 2; analysis
8000 <= fs <= 48000, f0 < fs / 2, order 0 .. 63, |alpha| <= 0.9, -0.4 <= q1 <= 0, 1 <= f0_floor <= 1000, -1 <= t <= 1e6."""
import numpy

import world_analysis_cases as A
import world_analysis_ref as RA
import world_synth_cases as S

SEED = 5
BINS = 513

# ---- analysis ------------------------------------------------------------------------------------------------------------------------
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)           # CheapTrick and sp2mc (fft_size is always given as 1024)
D4C_RATES = (16000, 24000)
WAVES = ('glide', 'noise')
TRACKS = ('lowest', 'high', 'offgrid')
D4C_TRACKS = TRACKS + ('lowest47',)
FRAMES_GPU = (1, 2, 61)
FRAMES_EMU = (1, 2, 13)
FLOOR = 40.0                                                       # handed over as f0_floor: below 3 fs / 1021 from 13.7 kHz on
TOP = 0.49985                                                      # x fs: f 1024 / fs = 511.85 (L clamps to 511), the smoothing width 341.23 bins (b = 342),
                                                                   # D4C: f 2048 / fs = 1023.69 (L = 1023, b1 = 1024), b2 = 512
T_FIRST, T_LAST = -1.0, 1e6                                        # the bounds of t
Q1 = (0.0, -0.15, -0.4)
FLOORS = (1.0, 1000.0)                                             # the bounds of f0_floor
ORDERS = (0, 1, 2, 3, 4, 7, 24, 59, 63)
ALPHAS = (-0.9, -0.5, 0.0, 0.41, 0.466, 0.9)
SP2MC_ROWS = 30


def f0_track(kind, n, fs):
    k = numpy.arange(n)
    if kind == 'lowest':                                           # just above the floor in force: the longest CheapTrick window (h = 510 from 13.7 kHz on)
        return RA.effective_floor(fs, 1024, FLOOR) * (1.001 + 4e-4 * k / 64.0)
    if kind == 'lowest47':                                         # D4C's floor: even frames just above 47 Hz, odd ones between its two floors (analysed at 47 Hz:
        return numpy.where(k % 2 == 0, 47.0 * (1.001 + 4e-4 * k / 64.0), 46.5 + 1e-3 * k)      # h4 = round(2 fs / 47), 2043 samples at 24 kHz)
    if kind == 'high':                                             # frame 0 at TOP x fs, gliding down to 800 Hz: one frame shows the bound
        return TOP * fs * (800.0 / (TOP * fs)) ** (k / max(n - 1, 1.0))
    if kind == 'offgrid':
        return A.f0_track('glide', n)
    raise ValueError(kind)


def times(kind, n):
    if kind != 'offgrid':
        return A.times(n)
    rng = numpy.random.default_rng(41)
    t = (numpy.arange(n) - 2.2) * A.FRAME_PERIOD + rng.uniform(-0.002, 0.002, n)              # the first frames are negative, down to -0.013 s
    if n >= 4:
        t[-3:] += 3.0                                              # seconds behind the end of the wave
    t[0] = T_FIRST
    if n >= 2:
        t[-1] = T_LAST
    return t


def threshold(kind):
    """D4C's Love-Train threshold for a track.  `high`: 0.3 instead of WORLD's 0.85 -- a window of seven samples at f0 near fs / 2 has a ratio of
    0.37 .. 0.68 on the `glide` wave and below 0.15 on `noise`, so at 0.3 the top frame runs the general body (L = 1023, the mirror of 3073 values)
    on one wave and is off on the other."""
    return 0.3 if kind == 'high' else 0.85


def case(wave_kind, track_kind, n, fs):
    """-> x, f0, t"""
    return A.wave(wave_kind, n, fs), f0_track(track_kind, n, fs), times(track_kind, n)


def sp2mc_rows(order, alpha):
    """30 spectra with a known mel-cepstrum, as tests/test_world_analysis_cpu.py makes its six."""
    from oracle import mc2sp as O
    mc0 = numpy.random.default_rng(9).normal(0.0, 0.3, (SP2MC_ROWS, order + 1))
    mc0[:, 0] -= 4.0
    return O.mc2sp(mc0, alpha, 1024)


# ---- synthesis -----------------------------------------------------------------------------------------------------------------------
CONFIGS = ((22050, 5.0),                                           # 110.25 samples per frame, exact in binary
           (16000, 5.8),                                           # 92.8: inexact
           (24000, 1.0),
           (16000, 0.0625),                                        # 1: the lowest admitted
           (48000, 10.0),
           (8000, 5.0))
SYNTH_TRACKS = ('glide', 'below', 'above', 'high')
SYNTH_FRAMES_GPU = (1, 2, 40)
SYNTH_FRAMES_EMU = (1, 2, 12)
SYNTH_TOP = 0.45                                                   # x fs: a pulse every 2 to 3 samples


def synth_frames(n, fs, frame_period):
    """The frame count of a case: at one sample per frame, the count that gives the samples n frames of 5 ms at 16 kHz give."""
    return n if fs * frame_period / 1000 > 1 or n <= 2 else (n - 1) * 80 + 1


def synth_f0(kind, n, fs):
    if kind == 'high':
        k = numpy.arange(n)
        return 800.0 * (SYNTH_TOP * fs / 800.0) ** (k / max(n - 1, 1.0))
    return S.f0_track(kind, n, fs)


def synth_case(kind, n, fs):
    return synth_f0(kind, n, fs), S.spectrogram(n), S.aperiodicity(n)


def frames_ending_on_a_wrap(fs=16000, frame_period=0.0625, start=200):
    """A frame count of the `high` track at a whole number of samples per frame whose LAST sample is a wrap of the phase.  Only there does a sample sit
    exactly on the last frame (position n - 1, weight 0): the one place where `positions at or behind the last frame take that frame` decides
    whether the frame behind the last -- which does not exist -- is read.  Found with the restatement's scan."""
    import world_synth_ref as R
    for n in range(start, start + 32):
        f0 = synth_f0('high', n, fs)
        length = R.y_length(n, fs, frame_period)
        f, v = R.sample_f0(R.coarse_f0(f0, fs, 1024), 0, length, fs, frame_period, n - 1)
        scan = R.PulseScan(fs)
        pulses = scan.feed(f, v)
        if pulses and pulses[-1][0] == length - 2 and scan.min_margin > 1e-9:
            return n
    raise ValueError('no such frame count')
