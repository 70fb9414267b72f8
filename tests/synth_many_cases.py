"""What the batched-synthesis tests share (tests/test_synth_many_cpu.py on the emulator, tests/test_synth_many_gpu.py on the MI355X): a rig of two
handles -- `many` takes the batched calls, `one` the yardstick, `synthesize` of every item alone on a SEPARATE handle with the same rate, frame
period and seed -- and the comparison: `numpy.array_equal` on the samples and on the pulse index / shift / voiced lists.  No tolerance anywhere: a
batched wave has the bits of its single call, which is the code held to the float64 restatement by tests/test_world_synth_*.py.  Inputs:
tests/world_synth_cases.py."""
import numpy

import world_synth_cases as C
from realtime_yukarin_amd import world_synth

SEED = 5
ROW = C.BINS * 4


class Rig(object):
    def __init__(self, ctx, fs, seed=SEED):
        self.ctx, self.fs, self.seed = ctx, fs, seed
        self.many = world_synth.Synthesizer(fs, 5.0, seed=seed, ctx=ctx)
        self.one = world_synth.Synthesizer(fs, 5.0, seed=seed, ctx=ctx)
        self._singles = {}

    def fresh(self):
        return world_synth.Synthesizer(self.fs, 5.0, seed=self.seed, ctx=self.ctx)

    def single(self, key, it):
        """(wave, pulse index, shift, voiced) of `synthesize` on the item alone; computed once per key and kept unchanged."""
        if key not in self._singles:
            y = self.one.synthesize(*it)
            got = (y.copy(),) + tuple(a.copy() for a in self.one.pulses())
            for a in got:
                a.setflags(write=False)
            self._singles[key] = got
        return self._singles[key]

    def close(self):
        self.many.close()
        self.one.close()


def item(kind, n, fs):
    return C.case(kind, n, fs)


def loud(n):
    """A neighbour that would show in anything that read across a wave boundary: sp constant 1e30, ap beyond both clamps."""
    return numpy.zeros(n) + 150.0, numpy.full((n, C.BINS), 1e30, numpy.float32), C.aperiodicity(n, mode='clamps')


def assert_wave(rig, b, y, want, pulses=True):
    assert y.dtype == numpy.float64 and numpy.array_equal(y, want[0]), 'wave %d: samples differ' % b
    if pulses:
        idx, shift, voiced = rig.many.pulses_many(b)
        assert numpy.array_equal(idx, want[1]) and numpy.array_equal(shift, want[2]) and numpy.array_equal(voiced, want[3]), 'wave %d: pulses differ' % b


def check_batch(rig, keyed, order=None):
    """`keyed`: [(key, (f0, sp, ap))].  The batched call on the list (in `order`) against the single call of every item; -> the batch's waves."""
    order = list(range(len(keyed))) if order is None else list(order)
    sel = [keyed[i] for i in order]
    before = dict(world_synth.calls)
    out = rig.many.synthesize_many([it for _, it in sel])
    assert world_synth.calls['packed'] == before['packed'] + 1 and world_synth.calls['fallback'] == before['fallback']
    assert len(out) == len(sel)
    for b, ((key, it), y) in enumerate(zip(sel, out)):
        assert len(y) == rig.many.length(len(it[0]))
        assert_wave(rig, b, y, rig.single(key, it))
    assert rig.many.pulses()[0].size == 0                              # ry_synth_debug_pulses after a batched call: none
    return out


def glides(rig, frames):
    return [(('glide', n), item('glide', n, rig.fs)) for n in frames]


def device_slices(ctx, items):
    """The items' sp / ap as consecutive slices of ONE device buffer each (what a batched stage-2 output is) -> [(f0, DeviceRows, DeviceRows)]."""
    sp = world_synth.to_device(ctx, numpy.concatenate([it[1] for it in items]))
    ap = world_synth.to_device(ctx, numpy.concatenate([it[2] for it in items]))
    out, r = [], 0
    for f0, _, _ in items:
        n = len(f0)
        out.append((f0, world_synth.DeviceRows(sp.address + r * ROW, n, keep=sp), world_synth.DeviceRows(ap.address + r * ROW, n, keep=ap)))
        r += n
    return out


# ---- the cases both suites run ---------------------------------------------------------------------------------------------------------
EDGES = {16000: [((13, 14), (961, 1041)), ((4, 5), (241, 321))], 24000: [((9, 10), (961, 1081))]}


def check_block_edges(rig):
    """Waves that end either side of a scan block (1024 samples) and of an overlap workgroup (256 samples): a wave boundary falls inside an
    overlap workgroup, and a workgroup boundary inside a wave."""
    for frames, samples in EDGES[rig.fs]:
        out = check_batch(rig, glides(rig, frames))
        assert tuple(len(y) for y in out) == samples
        check_batch(rig, glides(rig, frames), order=[1, 0])


def check_kinds(rig, n):
    """Every track kind in one call: pulse counts that differ tenfold between neighbours, a wave with very few pulses next to dense ones."""
    keyed = [((k, n), item(k, n, rig.fs)) for k in ('unvoiced', 'voiced71', 'voiced800', 'below', 'above', 'glide')]
    check_batch(rig, keyed)
    counts = [rig.single(k, it)[1].size for k, it in keyed]
    assert max(counts) >= 8 * max(min(counts), 1), counts
    check_batch(rig, keyed, order=[2, 1, 5, 0, 4, 3])


def check_no_leak(rig):
    mid = ('glide', 5), item('glide', 5, rig.fs)
    out = check_batch(rig, [(('loud', 7), loud(7)), mid, (('loud', 3), loud(3))])
    assert all(numpy.isfinite(y).all() for y in out)
    assert numpy.array_equal(out[1], rig.single(*mid)[0])


def check_noise_position(rig, n=12):
    """Two identical items: a noise position counted over the whole call would change the second one."""
    it = (('glide', n), item('glide', n, rig.fs))
    a, b = check_batch(rig, [it, it])
    assert numpy.array_equal(a, b) and numpy.abs(a).max() > 0


def check_device_rows(rig, frames=(5, 1, 9)):
    keyed = glides(rig, frames)
    items = [it for _, it in keyed]
    host = check_batch(rig, keyed)
    before = dict(world_synth.calls)
    dev = rig.many.synthesize_many(device_slices(rig.ctx, items))
    assert world_synth.calls == dict(before, in_place=before['in_place'] + 1)          # one call, nothing packed, no fallback
    for b, (y, h) in enumerate(zip(dev, host)):
        assert_wave(rig, b, y, rig.single(*keyed[b]))
        assert numpy.array_equal(y, h)
    # device rows that do not follow one another, and host and device items in one list: item by item, the same waves
    sl = device_slices(rig.ctx, items)
    for mixed in ([sl[1], sl[0], sl[2]], [sl[0], items[1], sl[2]], [(items[0][0], sl[0][1], items[0][2]), items[1]]):
        before = dict(world_synth.calls)
        got = rig.many.synthesize_many(mixed)
        assert world_synth.calls == dict(before, fallback=before['fallback'] + 1)
        for y, it in zip(got, mixed):
            key = ('glide', len(it[0]))
            assert numpy.array_equal(y, rig.single(key, None)[0])


def check_poison(rig):
    keyed = glides(rig, (6, 2))
    clean = check_batch(rig, keyed)
    rig.many.poison()
    again = check_batch(rig, keyed)
    assert all(numpy.array_equal(a, b) for a, b in zip(clean, again))


def check_aba(rig, a=(3, 2), b=(7, 1, 9)):
    """Batch A, batch B (longer: every buffer grows, more waves), batch A on one handle equal A on a fresh handle."""
    A, B = glides(rig, a), glides(rig, b)
    f = rig.fresh()
    want = f.synthesize_many([it for _, it in A])
    f.close()
    for keyed in (A, B, A):
        got = check_batch(rig, keyed)
        if keyed is A:
            assert all(numpy.array_equal(x, y) for x, y in zip(got, want))


def check_stream(rig, n=24):
    f0, sp, ap = item('glide', n, rig.fs)
    f = rig.fresh()
    want = numpy.concatenate([f.push(f0[:9], sp[:9], ap[:9]), f.push(f0[9:], sp[9:], ap[9:]), f.flush()])
    f.close()
    s = rig.many
    keyed = glides(rig, (4, 5))
    check_batch(rig, keyed)
    got = numpy.concatenate([s.push(f0[:9], sp[:9], ap[:9]), s.push(f0[9:], sp[9:], ap[9:]), s.flush()])
    assert numpy.array_equal(got, want)
    # a batched call in the middle of an open stream leaves the stream reset, exactly as `synthesize` does: nothing pushed, nothing to flush,
    # and the next stream starts at sample 0
    lib, h = s._get()
    s.push(f0[:9], sp[:9], ap[:9])
    assert lib.dll.ry_synth_bound(h, 0, 1) > 0
    check_batch(rig, keyed)
    assert lib.dll.ry_synth_bound(h, 0, 1) == 0 and lib.dll.ry_synth_bound(h, 1, 1) == 1
    import ctypes
    y, k = numpy.zeros(8), ctypes.c_int()
    assert lib.dll.ry_synth_flush(h, y.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 8, ctypes.byref(k)) == -4          # flush of an empty stream
    got = numpy.concatenate([s.push(f0[:9], sp[:9], ap[:9]), s.push(f0[9:], sp[9:], ap[9:]), s.flush()])
    assert numpy.array_equal(got, want)
