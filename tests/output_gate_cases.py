"""Inputs of the output-gate tests, seeded: the chunk sizes (both reflections in one frame, a multiple of the hop, lengths around n_fft, the
shipped 24000) and the signals at 24 kHz.  The float64 reference is computed once per (signal, size) and shared."""
import functools

import numpy

import output_gate_ref as R

FS = 24000
CHUNKS = (1025, 1536, 2047, 2048, 2049, 4096, 24000)
SIGNALS = ('zeros', 'sine', 'noise1e-6', 'noise3e-6', 'noise1e-4', 'voiced', 'click')
THRESHOLD = 80.0


@functools.lru_cache(maxsize=None)
def _signal(name, n):
    rng = numpy.random.default_rng(1000 + SIGNALS.index(name) * 100003 + n)
    t = numpy.arange(n) / FS
    if name == 'zeros':
        x = numpy.zeros(n)
    elif name == 'sine':
        x = 0.1 * numpy.sin(2 * numpy.pi * 220 * t)
    elif name.startswith('noise'):
        x = rng.normal(0.0, float(name[5:]), n)
    elif name == 'voiced':
        x = 0.2 * (1 + 0.5 * numpy.sin(2 * numpy.pi * 3 * t)) * numpy.sin(2 * numpy.pi * 150 * t) + rng.normal(0.0, 1e-3, n)
    else:
        x = numpy.zeros(n)
        x[-1] = 0.5
    x.setflags(write=False)
    return x


def signal(name, n):
    """n samples of the named signal (read-only, shared)."""
    return _signal(name, int(n))


@functools.lru_cache(maxsize=None)
def ref_mean(name, n):
    return R.mean_db(signal(name, n))


CASES = [(s, n) for n in CHUNKS for s in SIGNALS]


def verdict_cases(threshold=THRESHOLD, margin=1.0):
    """The cases whose reference mean lies at least `margin` dB from -threshold: a condition on the inputs (all of CASES meet it at 80)."""
    return [(s, n) for s, n in CASES if abs(ref_mean(s, n) + threshold) >= margin]


def splits(total, count, seed):
    """`count` seeded cut positions of a signal of `total` samples -> piece lengths; cuts may coincide (a piece of 0 samples) and lie one apart."""
    rng = numpy.random.default_rng(seed)
    cuts = sorted(int(c) for c in rng.integers(0, total + 1, count))
    if count >= 3:
        cuts[1] = cuts[0]                                          # a piece of 0 samples
        cuts[2] = min(cuts[0] + 1, total)                          # a piece of 1 sample
        cuts.sort()
    edges = [0] + cuts + [total]
    return [b - a for a, b in zip(edges, edges[1:])]
