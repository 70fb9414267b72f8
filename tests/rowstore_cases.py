"""Cases the emulator and the GPU tests of the row store share (test_rowstore_cpu.py, test_rowstore_gpu.py): `ry_rowstore_append` / `_fetch` /
`_retire` against a numpy model of the three rings, bit for bit, on a ring of 64 rows and 700 samples with mc rows of 9 floats and ap rows of 1
or 2 -- widths at which rows start at every 4-byte alignment.  The store is poisoned first, so a word the model does not expect to be written
shows; every destination lies at an odd 4-byte offset inside a block of sentinel words and the WHOLE block is compared."""
import ctypes

import numpy

from realtime_yukarin_amd import _lib, streams

CAP_ROWS, CAP_SAMPLES, MC_COLS = 64, 700, 9
SENTINEL = numpy.uint32(0x7fc12345)                      # a NaN with a payload: no copy and no pad produces it
POISON = numpy.uint32(0xffffffff)
EINVAL, ESTATE = -1, -4
IP = ctypes.POINTER(ctypes.c_int)


def u32(a):
    return numpy.ascontiguousarray(a).view(numpy.uint32)


class Model(object):
    """The rings in numpy: what the card must hold, word for word."""

    def __init__(self, ap_cols):
        self.cols = (MC_COLS, ap_cols)
        self.mc = numpy.full((CAP_ROWS, MC_COLS), POISON, numpy.uint32)
        self.ap = numpy.full((CAP_ROWS, ap_cols), POISON, numpy.uint32)
        self.wave = numpy.full(CAP_SAMPLES, POISON, numpy.uint32)
        self.row_tail = self.row_live = self.sample_tail = self.sample_live = 0

    def append(self, mc, ap, wave):
        rp, sp = (self.row_tail + self.row_live) % CAP_ROWS, (self.sample_tail + self.sample_live) % CAP_SAMPLES
        for k in range(len(mc)):
            self.mc[(rp + k) % CAP_ROWS], self.ap[(rp + k) % CAP_ROWS] = u32(mc[k]), u32(ap[k])
        self.wave[(sp + numpy.arange(len(wave))) % CAP_SAMPLES] = u32(wave)
        self.row_live += len(mc)
        self.sample_live += len(wave)
        return rp, sp

    def retire(self, rows, samples):
        self.row_tail, self.row_live = (self.row_tail + rows) % CAP_ROWS, self.row_live - rows
        self.sample_tail, self.sample_live = (self.sample_tail + samples) % CAP_SAMPLES, self.sample_live - samples

    def fetch(self, spans, ring, cap, out):
        for src, dst, n in spans:
            for k in range(n):
                out[dst + k] = 0 if src < 0 else ring[(src + k) % cap]


class Blocks(object):
    """Device blocks of 4-byte words, freed together."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, words) -> int:
        words = numpy.ascontiguousarray(words).view(numpy.float32).ravel()
        p = self.ctx.dev_alloc(max(words.size, 1))
        self.ctx.dev_upload(p, words)
        self.ptrs.append(p)
        return p

    def down(self, p, n) -> numpy.ndarray:
        out = numpy.empty(n, numpy.float32)
        self.ctx.dev_download(p, out)
        return out.view(numpy.uint32)

    def close(self):
        for p in self.ptrs:
            self.ctx.dev_free(p)


def rings_of(store, blocks, ap_cols):
    mc, ap, wave = store.buffers()
    return (blocks.down(mc, CAP_ROWS * MC_COLS).reshape(CAP_ROWS, MC_COLS), blocks.down(ap, CAP_ROWS * ap_cols).reshape(CAP_ROWS, ap_cols),
            blocks.down(wave, CAP_SAMPLES))


def assert_rings(store, blocks, model):
    mc, ap, wave = rings_of(store, blocks, model.cols[1])
    assert numpy.array_equal(mc, model.mc) and numpy.array_equal(ap, model.ap) and numpy.array_equal(wave, model.wave)
    assert store.held() == (model.row_live, model.sample_live)


def table(spans):
    return numpy.ascontiguousarray(numpy.asarray(spans, numpy.int32).reshape(-1, 3))


def raw_fetch(store, row_spans, sample_spans, mc_ptr, ap_ptr, wave_ptr, dst_rows, dst_samples):
    lib, h = store._get()
    rt, st = table(row_spans), table(sample_spans)
    return lib.dll.ry_rowstore_fetch(h, rt.ctypes.data_as(IP), len(rt), st.ctypes.data_as(IP), len(st), _lib._fptr(mc_ptr), _lib._fptr(ap_ptr),
                                     _lib._fptr(wave_ptr), dst_rows, dst_samples)


def check_fetch(store, blocks, model, row_spans, sample_spans, dst_rows, dst_samples, lead=1):
    """One fetch into destinations `lead` words into blocks of sentinels; the whole blocks against the model."""
    ap_cols = model.cols[1]
    sizes = [dst_rows * MC_COLS, dst_rows * ap_cols, dst_samples]
    guard = 7
    ptrs = [blocks.up(numpy.full(lead + n + guard, SENTINEL, numpy.uint32)) for n in sizes]
    rc = raw_fetch(store, row_spans, sample_spans, ptrs[0] + 4 * lead, ptrs[1] + 4 * lead, ptrs[2] + 4 * lead, dst_rows, dst_samples)
    assert rc == 0, store._ctx.lib.dll.ry_last_error()
    want = [numpy.full(lead + n + guard, SENTINEL, numpy.uint32) for n in sizes]
    model.fetch(row_spans, model.mc, CAP_ROWS, want[0][lead:lead + sizes[0]].reshape(dst_rows, MC_COLS))
    model.fetch(row_spans, model.ap, CAP_ROWS, want[1][lead:lead + sizes[1]].reshape(dst_rows, ap_cols))
    model.fetch(sample_spans, model.wave, CAP_SAMPLES, want[2][lead:lead + sizes[2]])
    for p, w in zip(ptrs, want):
        assert numpy.array_equal(blocks.down(p, w.size), w), (row_spans, sample_spans)
    c = store.counts()
    busy = any(n > 0 for _, _, n in list(row_spans) + list(sample_spans))
    assert (c['launches'], c['uploads'], c['waits']) == ((1, 1, 1) if busy else (0, 0, 0))


def source(rng, rows, ap_cols, samples):
    """Source blocks with ordinary values, NaNs, infinities, negative zeros and denormals: the store copies words."""
    out = []
    for shape in ((rows, MC_COLS), (rows, ap_cols), (samples,)):
        a = rng.normal(size=shape).astype(numpy.float32)
        flat = a.reshape(-1)
        flat[rng.permutation(flat.size)[:6]] = numpy.array([numpy.nan, numpy.inf, -numpy.inf, -0.0, 1e-42, 0.0], numpy.float32)[:min(6, flat.size)]
        out.append(a)
    return out


def check_store(ctx, ap_cols):
    """Grow, wrap, retire: four segments of 21 rows / 230 samples through a ring of 64 / 700, every fetch shape on the way."""
    rng = numpy.random.default_rng([ap_cols, 3])
    blocks = Blocks(ctx)
    store = streams.RowStore(MC_COLS, ap_cols, CAP_ROWS, CAP_SAMPLES, ctx=ctx)
    store.poison()
    model = Model(ap_cols)
    assert_rings(store, blocks, model)
    mc, ap, wave = source(rng, 40, ap_cols, 520)
    src = [blocks.up(a) for a in (mc, ap, wave)]

    def append(clock, row0, n_rows, sample0, n_samples):
        seg = store.append(clock, src[0], src[1], row0, n_rows, src[2], sample0, n_samples)
        want = model.append(mc[row0:row0 + n_rows], ap[row0:row0 + n_rows], wave[sample0:sample0 + n_samples])
        assert (seg.row_pos, seg.sample_pos) == want
        c = store.counts()
        assert (c['launches'], c['uploads'], c['waits']) == (1 if n_rows or n_samples else 0, 0, 0)      # enqueue only
        assert_rings(store, blocks, model)
        return seg

    append(0.0, 3, 21, 5, 230)
    append(0.1, 17, 21, 251, 230)
    # leading, interior and trailing pads, an empty span, a gap the call must not touch, spans inside one segment and across two
    check_fetch(store, blocks, model, [(-1, 0, 4), (0, 4, 21), (21, 25, 0), (-1, 25, 3), (21, 28, 21), (-1, 51, 2)],
                [(-1, 0, 7), (3, 7, 227), (-1, 234, 1), (230, 235, 230), (-1, 470, 9)], 55, 481)
    check_fetch(store, blocks, model, [(10, 2, 25)], [(100, 1, 300)], 30, 310, lead=3)                  # a gap in front of and behind the span
    check_fetch(store, blocks, model, [(5, 0, 0)], [(9, 0, 0)], 1, 1)                                   # nothing but empty spans: no launch
    check_fetch(store, blocks, model, [(-1, 0, 5)], [(-1, 0, 12)], 5, 12, lead=2)                       # nothing but pads
    check_fetch(store, blocks, model, [(42, 0, 0), (0, 0, 42)], [(460, 0, 0), (0, 0, 460)], 42, 460)    # an empty span at the write position
    store.retire(1)
    model.retire(21, 230)
    assert_rings(store, blocks, model)
    append(0.2, 0, 21, 0, 230)                            # rows 42 .. 62, samples 460 .. 689
    seg = append(0.3, 19, 21, 290, 230)                   # rows 63, 0 .. 19 and samples 690 .. 699, 0 .. 219: both wrap
    assert (seg.row_pos, seg.sample_pos) == (63, 690)
    # spans that cross the ring end, alone and between pads; the oldest live segment still whole
    check_fetch(store, blocks, model, [(21, 0, 21), (42, 21, 21), (63, 42, 21)], [(230, 0, 230), (460, 230, 460)], 63, 690)
    check_fetch(store, blocks, model, [(-1, 0, 1), (60, 1, 10), (-1, 11, 1)], [(-1, 0, 3), (695, 3, 100), (-1, 103, 2)], 12, 105, lead=3)
    for lead in (1, 2, 3, 4):                             # every residue of the destination against the ring's
        check_fetch(store, blocks, model, [(62, 0, 5)], [(697 - lead, 0, 37 + lead)], 5, 37 + lead, lead=lead)
    # through the plan: the store's own tables, rows and samples of segments 1 .. 3 by clock
    plan = streams.fetch_plan(store.clocks(), 0.1, 0.2, 0.05, 200)
    rows = streams.row_spans(plan, [s.rows for s in store.segments])
    n_rows, n_samples = streams.span_count(rows), streams.span_count(streams.wave_spans(plan, 5, 16000, [s.samples for s in store.segments]))
    dst = [blocks.up(numpy.full(n, SENTINEL, numpy.uint32)) for n in (n_rows * MC_COLS + 1, n_rows * ap_cols + 1, n_samples + 1)]
    assert store.fetch(plan, 5, 16000, dst[0] + 4, dst[1] + 4, dst[2] + 4, n_rows, n_samples) == (n_rows, n_samples) and n_rows >= 40
    got = blocks.down(dst[0], n_rows * MC_COLS + 1)
    assert got[0] == SENTINEL and not (got[1:] == SENTINEL).any()
    store.retire(3)
    model.retire(63, 690)
    assert store.held() == (0, 0) and store.segments == []
    store.reset()
    store.close()
    blocks.close()


def check_refusals(ctx, ap_cols):
    """Every refusal by return code, each leaving the rings, the live counts and the destinations as they were."""
    rng = numpy.random.default_rng([ap_cols, 4])
    blocks = Blocks(ctx)
    store = streams.RowStore(MC_COLS, ap_cols, CAP_ROWS, CAP_SAMPLES, ctx=ctx)
    store.poison()
    model = Model(ap_cols)
    mc, ap, wave = source(rng, 64, ap_cols, 700)
    src = [blocks.up(a) for a in (mc, ap, wave)]
    for k in range(2):
        store.append(0.1 * k, src[0], src[1], 0, 21, src[2], 0, 230)
        model.append(mc[:21], ap[:21], wave[:230])
    store.retire(1)
    model.retire(21, 230)                                 # live: rows 21 .. 41, samples 230 .. 459
    lib, h = store._get()
    dll = lib.dll
    f = _lib._fptr
    rp, sp = ctypes.c_int(-7), ctypes.c_int(-7)
    out = (ctypes.byref(rp), ctypes.byref(sp))
    appends = [(EINVAL, (h, f(0), f(src[1]), 0, 1, f(src[2]), 0, 1) + out), (EINVAL, (h, f(src[0]), f(0), 0, 1, f(src[2]), 0, 1) + out),
               (EINVAL, (h, f(src[0]), f(src[1]), 0, 1, f(0), 0, 1) + out), (EINVAL, (h, f(src[0]), f(src[1]), 0, -1, f(src[2]), 0, 1) + out),
               (EINVAL, (h, f(src[0]), f(src[1]), 0, 1, f(src[2]), 0, -1) + out), (EINVAL, (h, f(src[0]), f(src[1]), -1, 1, f(src[2]), 0, 1) + out),
               (EINVAL, (h, f(src[0]), f(src[1]), 0, 1, f(src[2]), -1, 1) + out), (EINVAL, (h, f(src[0]), f(src[1]), 0, 44, f(src[2]), 0, 1) + out),
               (EINVAL, (h, f(src[0]), f(src[1]), 0, 1, f(src[2]), 0, 471) + out), (EINVAL, (h, f(src[0]), f(src[1]), 0, 1, f(src[2]), 0, 1, None, out[1])),
               (EINVAL, (h, f(src[0]), f(src[1]), 0, 1, f(src[2]), 0, 1, out[0], None)), (ESTATE, (None, f(src[0]), f(src[1]), 0, 1, f(src[2]), 0, 1) + out)]
    for want, args in appends:
        assert dll.ry_rowstore_append(*args) == want, args[3:8]
    assert (rp.value, sp.value) == (-7, -7)
    for want, args in ((EINVAL, (h, 22, 0)), (EINVAL, (h, 0, 231)), (EINVAL, (h, -1, 0)), (EINVAL, (h, 0, -1)), (ESTATE, (None, 0, 0))):
        assert dll.ry_rowstore_retire(*args) == want, args[1:]
    dst_rows, dst_samples = 30, 300
    sizes = [dst_rows * MC_COLS, dst_rows * ap_cols, dst_samples]
    dst = [blocks.up(numpy.full(n, SENTINEL, numpy.uint32)) for n in sizes]
    good_r, good_s = [(21, 0, 21)], [(230, 0, 230)]
    bad_rows = [[(21, 0, -1)], [(21, -1, 2)], [(21, 10, 21)], [(64, 0, 1)], [(-2, 0, 1)], [(20, 0, 2)], [(41, 0, 2)], [(42, 0, 1)], [(0, 0, 1)],
                [(21, 0, 21), (21, 29, 2)]]
    bad_samples = [[(230, 0, -1)], [(230, -1, 2)], [(230, 71, 230)], [(700, 0, 1)], [(-2, 0, 1)], [(229, 0, 2)], [(459, 0, 2)], [(460, 0, 1)],
                   [(699, 0, 2)]]
    for spans in bad_rows:
        assert raw_fetch(store, spans, good_s, dst[0], dst[1], dst[2], dst_rows, dst_samples) == EINVAL, spans
    for spans in bad_samples:
        assert raw_fetch(store, good_r, spans, dst[0], dst[1], dst[2], dst_rows, dst_samples) == EINVAL, spans
    for ptrs in ((0, dst[1], dst[2]), (dst[0], 0, dst[2]), (dst[0], dst[1], 0)):
        assert raw_fetch(store, good_r, good_s, ptrs[0], ptrs[1], ptrs[2], dst_rows, dst_samples) == EINVAL, ptrs
    assert raw_fetch(store, good_r, good_s, dst[0], dst[1], dst[2], -1, dst_samples) == EINVAL
    assert raw_fetch(store, good_r, good_s, dst[0], dst[1], dst[2], dst_rows, -1) == EINVAL
    rt = table(good_r)
    null_i = ctypes.cast(ctypes.c_void_p(0), IP)
    tail = (f(dst[0]), f(dst[1]), f(dst[2]), dst_rows, dst_samples)
    assert dll.ry_rowstore_fetch(h, null_i, 1, rt.ctypes.data_as(IP), 0, *tail) == EINVAL
    assert dll.ry_rowstore_fetch(h, rt.ctypes.data_as(IP), 0, null_i, 1, *tail) == EINVAL
    assert dll.ry_rowstore_fetch(h, rt.ctypes.data_as(IP), -1, null_i, 0, *tail) == EINVAL
    assert dll.ry_rowstore_fetch(h, rt.ctypes.data_as(IP), 0, null_i, -1, *tail) == EINVAL
    assert dll.ry_rowstore_fetch(None, rt.ctypes.data_as(IP), 1, null_i, 0, *tail) == ESTATE
    assert b'retired' in (raw_fetch(store, [(20, 0, 2)], [], dst[0], dst[1], dst[2], dst_rows, dst_samples), dll.ry_last_error())[1]
    # nothing changed: the rings, the counts, the destinations
    assert_rings(store, blocks, model)
    for p, n in zip(dst, sizes):
        assert (blocks.down(p, n) == SENTINEL).all()
    # and the store still works: the good spans, then an append into the room that is left
    assert raw_fetch(store, good_r, good_s, dst[0], dst[1], dst[2], dst_rows, dst_samples) == 0
    assert numpy.array_equal(blocks.down(dst[0], 21 * MC_COLS), model.mc[21:42].ravel())
    hc = ctypes.c_void_p()
    for args in ((0, ap_cols, 4, 4), (MC_COLS, 0, 4, 4), (MC_COLS, ap_cols, 0, 4), (MC_COLS, ap_cols, 4, 0), (65537, 1, 4, 4), (MC_COLS, ap_cols, (1 << 22) + 1, 4),
                 (65536, 1, 1 << 15, 4)):
        assert dll.ry_rowstore_create(ctx.handle, *args, ctypes.byref(hc)) == EINVAL and not hc.value, args
    assert dll.ry_rowstore_create(None, MC_COLS, ap_cols, 4, 4, ctypes.byref(hc)) == EINVAL
    assert dll.ry_rowstore_create(ctx.handle, MC_COLS, ap_cols, 4, 4, None) == EINVAL
    store.close()
    blocks.close()
