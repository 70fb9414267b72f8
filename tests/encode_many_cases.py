"""Cases the emulator and the GPU tests of the many-waves encode share (test_encode_many_cpu.py, test_encode_many_gpu.py).  The yardstick of every
comparison is the shipped single-wave call -- `CrepeModel.track` -> `Analyzer.run_device` -- on a SEPARATE handle of the same weights, and every
comparison is bit equality through `encode_cases.same`: the seven outputs (voiced, the masked float64 f0, the time axis, sp, mc, ap, coded_ap) and
the float32 rows left on the card."""
import numpy

import encode_cases as E
from crepe_cases import tie_activations
from realtime_yukarin_amd import crepe, world_analysis

KEYS = ('sp64', 'mc', 'ap64', 'coded_ap')
NAMES = ('voiced', 'f0', 't') + KEYS + ('sp32', 'ap32')
STEP = 5
TRACK_FRAMES = (1, 2, 3, E.VOICING_CHUNK - 1, E.VOICING_CHUNK + 1, 2 * E.VOICING_CHUNK + 1)
CONFIDENCE_SETS = ('crossing', 'crossing ramp', 'threshold', 'zeros', 'const 0.0795', 'square 7')      # the tie-laden and the crossing sets


class Rig(object):
    """Two CREPE handles of the same weights and two analyzers of the same settings on one context: `many` takes the batched calls, `one` the
    single-wave calls they are held to."""

    def __init__(self, ctx, capacity, fs: int, dtype: str = 'f32'):
        self.ctx, self.fs = ctx, fs
        self.many = crepe.CrepeModel(capacity, seed=21, ctx=ctx, dtype=dtype)
        self.one = crepe.CrepeModel(capacity, seed=21, ctx=ctx, dtype=dtype)
        self.a_many = world_analysis.Analyzer(fs, order=8, seed=5, ctx=ctx)
        self.a_one = world_analysis.Analyzer(fs, order=8, seed=5, ctx=ctx)

    def fresh(self):
        return Rig(self.ctx, self.many.m, self.fs, self.many.dtype)

    def close(self):
        for h in (self.many, self.one, self.a_many, self.a_one):
            h.close()

    def poison(self):
        for h in (self.many, self.one, self.a_many, self.a_one):
            h.poison()

    def _rows(self, rows, n):
        h = numpy.empty((n, 513), numpy.float32)
        self.ctx.dev_download(rows.address, h)
        return h

    def single(self, x):
        """The shipped chain on one wave -> {name: array} of NAMES."""
        trk = self.one.track(x, self.fs, crepe.hop_length(STEP), STEP, device=True)
        args = (trk.wave, trk.samples, trk.f0, trk.t, trk.frames)
        out = dict(zip(KEYS, self.a_one.run_device(*args, want=KEYS)))
        rows = self.a_one.run_device(*args, want=('sp', 'ap'), device_rows=True)
        out['sp32'], out['ap32'] = self._rows(rows[0], trk.frames), self._rows(rows[1], trk.frames)
        out['voiced'], out['f0'] = trk.download()
        t = numpy.empty(trk.frames, numpy.float64)
        self.ctx.dev_download(trk.t, t.view(numpy.float32))
        out['t'] = t
        return out

    def batch(self, xs):
        """The batched chain on the list -> [{name: array}] per wave."""
        trk = self.many.track_many(xs, self.fs, crepe.hop_length(STEP), STEP, device=True)
        assert trk.waves == len(xs) and list(numpy.diff(trk.sample_offsets)) == [numpy.asarray(x).size for x in xs]
        args = (trk.wave, trk.sample_offsets, trk.f0, trk.t, trk.frame_offsets)
        got = dict(zip(KEYS, self.a_many.run_device_many(*args, want=KEYS)))
        rows = self.a_many.run_device_many(*args, want=('sp', 'ap'), device_rows=True)
        got['sp32'], got['ap32'] = self._rows(rows[0], trk.frames), self._rows(rows[1], trk.frames)
        t = numpy.empty(trk.frames, numpy.float64)
        self.ctx.dev_download(trk.t, t.view(numpy.float32))
        tracks = trk.download()
        out, o = [], trk.frame_offsets
        for i in range(trk.waves):
            d = {k: v[o[i]:o[i + 1]] for k, v in got.items()}
            d['voiced'], d['f0'], d['t'] = tracks[i][0], tracks[i][1], t[o[i]:o[i + 1]]
            out.append(d)
        return out


def assert_same(got, want, what=''):
    for k in NAMES:
        assert E.same(got[k], want[k]), (what, k, numpy.asarray(got[k]).shape, numpy.asarray(want[k]).shape)


def check_batch(rig, xs, order=None, singles=None, frames=None):
    """The batch of xs (in `order`, a permutation) against the single call on every wave; -> the singles, for the next permutation."""
    singles = singles if singles is not None else [rig.single(x) for x in xs]
    order = list(range(len(xs))) if order is None else list(order)
    got = rig.batch([xs[i] for i in order])
    if frames is not None:
        assert [g['voiced'].size for g in got] == [frames[i] for i in order]
    for g, i in zip(got, order):
        assert_same(g, singles[i], 'wave %d of %s' % (i, order))
    return singles


def loud(n: int) -> numpy.ndarray:
    return numpy.full(n, 1e30, numpy.float32)


def check_voicing_many(many, one, frames=TRACK_FRAMES, device=True):
    """Tracks of `frames` frames side by side, every set of CONFIDENCE_SETS, both steps: each equals `voicing` on it alone."""
    f0s = [numpy.random.default_rng([7, n]).uniform(40.0, 900.0, n).astype(numpy.float32) for n in frames]
    sets = [E.confidence_sets(n) for n in frames]
    for name in CONFIDENCE_SETS:
        cs = [s[name] for s in sets]
        for step in E.STEPS:
            got = many.voicing_many(cs, f0s, threshold=0.1, step_size=step, device=device)
            for n, c, f, g in zip(frames, cs, f0s, got):
                want = one.voicing(c, f, threshold=0.1, step_size=step)
                assert numpy.array_equal(g[0], want[0]) and E.same(g[1], want[1]) and E.same(g[2], want[2]), (name, step, n)


def check_decode_many(many, one, frames, viterbi=True):
    """Tie-laden activations of `frames` frames side by side: each track's f0, confidence and path equal `decode` on it alone."""
    acts = [tie_activations(n, 100 + n) for n in frames]
    got = many.decode_many(acts, viterbi=viterbi)
    for n, a, g in zip(frames, acts, got):
        want = one.decode(a, viterbi=viterbi)
        assert all(E.same(x, y) for x, y in zip(g, want)), (n, viterbi)
