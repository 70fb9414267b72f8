"""Seeded inputs of the WORLD synthesis tests (tests/test_world_synth_*.py) and of the tolerance measurement
(scripts/synth_tolerance.py): one place, so that the CPU test can vet the tracks a GPU test will run."""
import numpy

BINS = 513
RATES = (16000, 24000)
LENGTHS = (1, 2, 100, 300, 2000)
# Constant-f0 tracks: with f0 / fs rational the phase comes back to a whole number of turns (every 32 samples on the 500 Hz unvoiced grid, every
# 20 / 30 at 800 Hz, every second at 71 Hz), so some of their wraps are near-ties BY CONSTRUCTION.  The issue prescribes these tracks; their
# pulse indices are equal because both sides do the same IEEE-754 operations in the same order, not because the decisions are far from the
# threshold.  Every track whose shape is ours to choose must keep clear of it (test_world_synth_ref.py).
CONSTANT = ('unvoiced', 'voiced71', 'voiced800')
ON_GRID = ('unvoiced', 'voiced800')          # ... of these, the ones whose period is a whole number of samples
TRACKS = ('glide', 'unvoiced', 'voiced71', 'voiced800', 'below', 'above')


def threshold(fs):
    return fs / 1024 + 1.0


def f0_track(kind, n, fs):
    t = numpy.arange(n)
    if kind == 'glide':                      # gliding voiced f0 with unvoiced gaps (starts voiced: the phase is off the 500 Hz grid)
        f = 180.0 + 70.0 * numpy.sin(t / 23.0) + 0.37 * t % 11
        f[(t % 97 >= 60) & (t % 97 < 75)] = 0.0
        return f
    if kind == 'unvoiced':
        return numpy.zeros(n)
    if kind == 'voiced71':
        return numpy.full(n, 71.0)
    if kind == 'voiced800':
        return numpy.full(n, 800.0)
    if kind == 'below':                      # just below fs / fft_size + 1: unvoiced, with voiced stretches so that the flag interpolates
        f = numpy.full(n, threshold(fs) - 1e-3)
        v = (t % 50) < 20
        f[v] = 123.4 + 0.0137 * t[v]         # a slow drift: no two voiced stretches repeat the same phase advance
        return f
    if kind == 'above':                      # just above: voiced at the lowest f0 there is
        f = numpy.full(n, threshold(fs) + 1e-3)
        v = (t % 50) < 20
        f[v] = 123.4 + 0.0137 * t[v]
        return f
    raise ValueError(kind)


def spectrogram(n, seed=356):
    """`synth.stage2_input` (exp(N(-6, 1.5)) + 1e-16, float32), one window."""
    from realtime_yukarin_amd import synth
    return synth.stage2_input(n, seed=seed)[0]


def aperiodicity(n, seed=11, mode='mixed'):
    rng = numpy.random.default_rng(seed)
    if mode == 'floor':
        return numpy.full((n, BINS), 0.001, numpy.float32)
    if mode == 'ceil':
        return numpy.ones((n, BINS), numpy.float32)
    if mode == 'clamps':                     # below the lower clamp / above the upper one, mixed per bin
        return numpy.where(rng.random((n, BINS)) < 0.5, 0.0, 1.5).astype(numpy.float32)
    return rng.uniform(0.001, 0.999, (n, BINS)).astype(numpy.float32)


def case(kind, n, fs, ap_mode='mixed'):
    return f0_track(kind, n, fs), spectrogram(n), aperiodicity(n, mode=ap_mode)
