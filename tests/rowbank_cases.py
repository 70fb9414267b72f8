"""Cases the emulator and the GPU tests of the row bank share (test_rowbank_cpu.py, test_rowbank_gpu.py): `ry_rowbank_append` / `_fetch` /
`_pick_ap` / `_retire` for B = 3 streams against one numpy model of the rings per stream (`rowstore_cases.Model`), bit for bit, at the widths of
tests/rowstore_cases.py -- rings of 64 rows and 700 samples, mc rows of 9 floats, ap rows of 1 or 2 -- where rows start at every 4-byte alignment.
The bank is poisoned first; every destination lies 1 to 4 words into a block of sentinel words and the WHOLE block is compared.  The picked ap
rows are also held to a `RowStore` per stream driven through `fetch`, `ry_mask_rows` and the slice [k0, k1) on the same data."""
import ctypes

import numpy

import rowstore_cases as R
from realtime_yukarin_amd import _lib, streams

B = 3
CAP_ROWS, CAP_SAMPLES, MC_COLS = R.CAP_ROWS, R.CAP_SAMPLES, R.MC_COLS
SENTINEL, EINVAL, ESTATE = R.SENTINEL, R.EINVAL, R.ESTATE
IP, LLP, UBP = R.IP, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ubyte)
SPECIALS = numpy.array([numpy.nan, numpy.inf, -numpy.inf, -0.0, 1e-42, -1e-44], numpy.float32)


def ints(a, dtype=numpy.int32):
    a = numpy.ascontiguousarray(a, dtype=dtype).ravel()
    return a, a.ctypes.data_as(LLP if dtype == numpy.int64 else IP)


def offsets(counts):
    return [0] + [int(v) for v in numpy.cumsum(counts)]


def source(rng, rows, ap_cols, samples):
    """The shared encode blocks: ordinary values with a NaN, an infinity, a negative zero or a denormal at every third word."""
    out = []
    for shape in ((rows, MC_COLS), (rows, ap_cols), (samples,)):
        a = rng.normal(size=shape).astype(numpy.float32)
        flat = a.reshape(-1)
        flat[::3] = SPECIALS[numpy.arange(flat[::3].size) % SPECIALS.size]
        out.append(a)
    return out


def arrays_of(bank, blocks, ap_cols):
    mc, ap, wave = bank.buffers()
    return (blocks.down(mc, B * CAP_ROWS * MC_COLS).reshape(B, CAP_ROWS, MC_COLS), blocks.down(ap, B * CAP_ROWS * ap_cols).reshape(B, CAP_ROWS, ap_cols),
            blocks.down(wave, B * CAP_SAMPLES).reshape(B, CAP_SAMPLES))


def assert_bank(bank, blocks, models):
    mc, ap, wave = arrays_of(bank, blocks, models[0].cols[1])
    for b, m in enumerate(models):
        assert numpy.array_equal(mc[b], m.mc) and numpy.array_equal(ap[b], m.ap) and numpy.array_equal(wave[b], m.wave), b
        assert bank.held(b) == (m.row_live, m.sample_live), b


def launch_counts(bank):
    c = bank.counts()
    return c['launches'], c['uploads'], c['waits']


def span_tables(per_stream):
    """[[(src, dst, n)]] per stream -> (the table of all spans, its offsets per stream)."""
    flat = [s for spans in per_stream for s in spans]
    return R.table(flat if flat else numpy.empty((0, 3), numpy.int32)), offsets([len(spans) for spans in per_stream])


def raw_append(bank, part, src, row0, n_rows, sample0, n_samples, null_out=False):
    lib, h = bank._get()
    n = len(part)
    rp, sp = numpy.full(max(n, 1), -7, numpy.int32), numpy.full(max(n, 1), -7, numpy.int32)
    null_i = ctypes.cast(ctypes.c_void_p(0), IP)
    rc = lib.dll.ry_rowbank_append(h, n, ints(part)[1], _lib._fptr(src[0]), _lib._fptr(src[1]), ints(row0)[1], ints(n_rows)[1], _lib._fptr(src[2]),
                                   ints(sample0, numpy.int64)[1], ints(n_samples)[1], null_i if null_out else rp.ctypes.data_as(IP), sp.ctypes.data_as(IP))
    return rc, rp, sp


def raw_fetch(bank, part, row_spans, sample_spans, mc_ptr, wave_ptr, fo, so, ro=None, wo=None):
    lib, h = bank._get()
    rt, r_off = span_tables(row_spans)
    st, s_off = span_tables(sample_spans)
    return lib.dll.ry_rowbank_fetch(h, len(part), ints(part)[1], rt.ctypes.data_as(IP), ints(r_off if ro is None else ro)[1], st.ctypes.data_as(IP),
                                    ints(s_off if wo is None else wo)[1], _lib._fptr(mc_ptr), _lib._fptr(wave_ptr), ints(fo)[1], ints(so, numpy.int64)[1])


def raw_pick(bank, part, row_spans, fo, keep, mask_ptr, pack_ptr, pack_rows):
    lib, h = bank._get()
    rt, r_off = span_tables(row_spans)
    return lib.dll.ry_rowbank_pick_ap(h, len(part), ints(part)[1], rt.ctypes.data_as(IP), ints(r_off)[1], ints(fo)[1], ints([k for pair in keep for k in pair])[1],
                                      ctypes.cast(ctypes.c_void_p(mask_ptr), UBP), _lib._fptr(pack_ptr), pack_rows)


def up_mask(blocks, mask) -> int:
    """A byte mask on the card (padded to whole words)."""
    m = numpy.zeros((len(mask) + 4) // 4 * 4, numpy.uint8)
    m[:len(mask)] = mask
    return blocks.up(m.view(numpy.uint32))


def busy(per_stream):
    return any(n > 0 for spans in per_stream for _, _, n in spans)


def check_fetch(bank, blocks, models, part, row_spans, sample_spans, sizes, lead):
    """One fetch of the streams `part` into blocks `lead` words in; the whole blocks against the models.  sizes: (rows, samples) per stream."""
    fo, so = offsets([r for r, _ in sizes]), offsets([s for _, s in sizes])
    want = [numpy.full(lead + n + 7, SENTINEL, numpy.uint32) for n in (fo[-1] * MC_COLS, so[-1])]
    ptrs = [blocks.up(w) for w in want]
    rc = raw_fetch(bank, part, row_spans, sample_spans, ptrs[0] + 4 * lead, ptrs[1] + 4 * lead, fo, so)
    assert rc == 0, bank._ctx.lib.dll.ry_last_error()
    for i, b in enumerate(part):
        m = models[b]
        m.fetch(row_spans[i], m.mc, CAP_ROWS, want[0][lead + fo[i] * MC_COLS:lead + fo[i + 1] * MC_COLS].reshape(-1, MC_COLS))
        m.fetch(sample_spans[i], m.wave, CAP_SAMPLES, want[1][lead + so[i]:lead + so[i + 1]])
    for p, w in zip(ptrs, want):
        assert numpy.array_equal(blocks.down(p, w.size), w), (part, row_spans, sample_spans)
    assert launch_counts(bank) == ((1, 1, 1) if busy(row_spans) or busy(sample_spans) else (0, 0, 0))


def picked(model, spans, rows, mask, keep, ap_cols):
    """What `pick_ap` must pack for one stream: the window by the model, the mask applied, the slice; None where no span covers a row."""
    window = numpy.full((rows, ap_cols), -1, numpy.int64)
    words = numpy.zeros((rows, ap_cols), numpy.uint32)
    model.fetch(spans, model.ap, CAP_ROWS, words)
    for _, dst, n in spans:
        window[dst:dst + n] = words[dst:dst + n]
    window[(numpy.asarray(mask) == 0) & (window[:, 0] >= 0)] = 0
    return window[keep[0]:keep[1]]


def check_pick(ctx, bank, stores, blocks, models, part, row_spans, rows, keep, masks, lead):
    """One pick of the streams `part` into a block `lead` words in: the whole block against the models, the counts, and every stream's rows
    against its lone `RowStore` through fetch, `ry_mask_rows` and the slice."""
    ap_cols = models[0].cols[1]
    fo = offsets(rows)
    total = sum(k1 - k0 for k0, k1 in keep)
    want = numpy.full(lead + total * ap_cols + 7, SENTINEL, numpy.uint32)
    at = lead
    for i, b in enumerate(part):
        w = picked(models[b], row_spans[i], rows[i], masks[i], keep[i], ap_cols).ravel()
        seen = w >= 0
        want[at:at + w.size][seen] = w[seen].astype(numpy.uint32)
        at += w.size
    pack = blocks.up(want * 0 + SENTINEL)
    mask_ptr = up_mask(blocks, numpy.concatenate([numpy.asarray(m, numpy.uint8) for m in masks] + [numpy.zeros(0, numpy.uint8)]))
    rc = raw_pick(bank, part, row_spans, fo, keep, mask_ptr, pack + 4 * lead, total)
    assert rc == 0, bank._ctx.lib.dll.ry_last_error()
    got = blocks.down(pack, want.size)
    assert numpy.array_equal(got, want), (part, keep)
    kept_rows = any(n > 0 and max(dst, k0) < min(dst + n, k1) for spans, (k0, k1) in zip(row_spans, keep) for _, dst, n in spans)
    assert launch_counts(bank) == ((1, 1, 1) if kept_rows else (0, 0, 0))
    at = lead
    for i, b in enumerate(part):                          # the lone store: fetch, mask, slice
        k0, k1 = keep[i]
        dst = [blocks.up(numpy.full(max(rows[i], 1) * c + 1, SENTINEL, numpy.uint32)) for c in (MC_COLS, ap_cols)]
        assert R.raw_fetch(stores[b], row_spans[i], [], dst[0] + 4, dst[1] + 4, 0, rows[i], 0) == 0
        if rows[i] > 0:
            ctx.mask_rows(dst[1] + 4, up_mask(blocks, masks[i]), rows[i], ap_cols, k0, k1)
        alone = blocks.down(dst[1], rows[i] * ap_cols + 1)[1:].reshape(rows[i], ap_cols)[k0:k1].ravel()
        assert numpy.array_equal(got[at:at + alone.size], alone), (b, keep[i])
        at += alone.size


def check_bank(ctx, ap_cols):
    """Three streams with segments of 21, 13 and 30 rows through rings of 64 rows: they wrap at different pushes; one sits calls out, one
    is retired alone; every fetch and pick shape on the way."""
    rng = numpy.random.default_rng([ap_cols, 33])
    blocks = R.Blocks(ctx)
    bank = streams.RowBank(B, MC_COLS, ap_cols, CAP_ROWS, CAP_SAMPLES, ctx=ctx)
    bank.poison()
    stores = [streams.RowStore(MC_COLS, ap_cols, CAP_ROWS, CAP_SAMPLES, ctx=ctx) for _ in range(B)]
    models = [R.Model(ap_cols) for _ in range(B)]
    assert_bank(bank, blocks, models)
    mc, ap, wave = source(rng, 70, ap_cols, 800)
    src = [blocks.up(a) for a in (mc, ap, wave)]
    seg_rows, seg_samples = (21, 13, 30), (230, 150, 330)

    def append(part, row0, sample0):
        """The segments of `part` from rows row0[i] / samples sample0[i] of the shared blocks, in the bank, the models and the lone stores."""
        rows, samples = [(r, seg_rows[b]) for b, r in zip(part, row0)], [(s, seg_samples[b]) for b, s in zip(part, sample0)]
        pieces = 0
        for b in part:                                    # what the table must hold: a run per array, two where it crosses the ring end
            m = models[b]
            rp, sp = (m.row_tail + m.row_live) % CAP_ROWS, (m.sample_tail + m.sample_live) % CAP_SAMPLES
            pieces += 2 * (2 if rp + seg_rows[b] > CAP_ROWS else 1) + (2 if sp + seg_samples[b] > CAP_SAMPLES else 1)
        segs = bank.append_many(part, [0.1 * b for b in part], src, rows, samples)
        assert launch_counts(bank) == ((1, 0, 0) if pieces <= 6 else (1, 1, 1)), (part, pieces, bank.counts())
        for seg, b, (r, n), (s, k) in zip(segs, part, rows, samples):
            want = models[b].append(mc[r:r + n], ap[r:r + n], wave[s:s + k])
            assert (seg.row_pos, seg.sample_pos) == want
            stores[b].append(0.0, src[0], src[1], r, n, src[2], s, k)
        assert_bank(bank, blocks, models)
        return segs

    append([0, 2], [3, 24], [5, 235])                     # two streams in one call, the third sits out: six pieces, by value
    append([0, 1, 2], [1, 22, 35], [0, 230, 380])         # n = 3: nine pieces, the table goes up
    append([1], [40], [7])                                # n = 1
    # stream 0: rows 0 .. 41; stream 1: 0 .. 25; stream 2: 0 .. 59.  n = 3: leading, interior and trailing pads, empty spans, a gap in stream 1
    spans3 = [[(-1, 0, 4), (0, 4, 21), (21, 25, 0), (-1, 25, 3), (21, 28, 21), (-1, 49, 2)], [(2, 1, 20)], [(-1, 0, 1), (30, 1, 30)]]
    samples3 = [[(-1, 0, 7), (3, 7, 227), (-1, 234, 1), (230, 235, 230), (-1, 465, 9)], [(10, 2, 280)], [(330, 0, 330), (-1, 330, 5)]]
    for lead in (1, 2, 3, 4):
        check_fetch(bank, blocks, models, [0, 1, 2], spans3, samples3, [(51, 474), (22, 285), (31, 335)], lead)
    check_fetch(bank, blocks, models, [1], [[(13, 0, 13)]], [[(150, 0, 150)]], [(13, 150)], 1)                        # n = 1
    check_fetch(bank, blocks, models, [0, 2], [[(5, 0, 0)], [(-1, 0, 3)]], [[(9, 0, 0)], [(-1, 0, 0)]], [(1, 1), (3, 0)], 2)
    check_fetch(bank, blocks, models, [0, 1], [[(5, 0, 0)], []], [[], [(9, 0, 0)]], [(0, 0), (0, 0)], 3)             # nothing but empty spans: no launch
    # pick: masks with zeros at the first and the last kept row and beside the pads; a keep range that starts inside a pad; no kept row for stream 1
    rows3 = [51, 22, 31]
    cover1 = [[(-1, 0, 4), (0, 4, 21), (-1, 25, 3), (21, 28, 21), (-1, 49, 2)], [(0, 0, 22)], [(-1, 0, 1), (30, 1, 30)]]
    masks = [numpy.ones(n, numpy.uint8) for n in rows3]
    masks[0][[2, 4, 24, 28, 30, 47, 48]] = 0              # first kept row, rows beside the pads, the last kept row and the one before
    masks[2][[1, 7, 8, 30]] = 0
    for lead in (1, 2, 3, 4):
        check_pick(ctx, bank, stores, blocks, models, [0, 1, 2], cover1, rows3, [(2, 49), (7, 7), (0, 31)], masks, lead)
    check_pick(ctx, bank, stores, blocks, models, [2], [cover1[2]], [31], [(1, 31)], [masks[2]], 1)                   # n = 1
    check_pick(ctx, bank, stores, blocks, models, [0, 1], cover1[:2], rows3[:2], [(25, 27), (0, 0)], masks[:2], 2)    # pads alone
    check_pick(ctx, bank, stores, blocks, models, [0, 1], cover1[:2], rows3[:2], [(0, 0), (22, 22)], masks[:2], 3)    # nothing kept: no launch
    # retire of one stream only, then appends: stream 2 wraps (rows 60 .. 63, 0 .. 25), the others do not yet
    bank.retire(2, 1)
    stores[2].retire(1)
    models[2].retire(30, 330)
    assert_bank(bank, blocks, models)
    segs = append([1, 2], [0, 9], [100, 300])
    assert (segs[1].row_pos, segs[1].sample_pos) == (60, 660)
    check_fetch(bank, blocks, models, [1, 2], [[(26, 0, 13), (0, 13, 26)], [(-1, 0, 2), (30, 2, 60), (-1, 62, 1)]],
                [[(300, 0, 150)], [(-1, 0, 3), (330, 3, 660)]], [(39, 150), (63, 663)], 3)                            # across the ring end, between pads
    m2 = numpy.ones(63, numpy.uint8)
    m2[[2, 31, 32, 35, 36, 61]] = 0                      # beside the pads and on both sides of the ring end (window rows 31 / 32 -> ring rows 59 / 60 .. 63 / 0)
    for lead in (1, 4):
        check_pick(ctx, bank, stores, blocks, models, [2], [[(-1, 0, 2), (30, 2, 60), (-1, 62, 1)]], [63], [(1, 63)], [m2], lead)
    # stream 0 wraps two pushes later than stream 2 did; stream 1 much later
    bank.retire(0, 1)
    stores[0].retire(1)
    models[0].retire(21, 230)
    segs = append([0], [30], [400])                       # rows 42 .. 62
    bank.retire(0, 1)
    stores[0].retire(1)
    models[0].retire(21, 230)
    segs = append([0, 1], [0, 50], [0, 600])              # stream 0: rows 63, 0 .. 19 and samples 690 .. 699, 0 .. 219: both wrap
    assert (segs[0].row_pos, segs[0].sample_pos) == (63, 690) and (segs[1].row_pos, segs[1].sample_pos) == (39, 450)
    check_fetch(bank, blocks, models, [0, 1, 2], [[(42, 0, 42)], [(13, 1, 39)], [(62, 0, 20)]], [[(460, 0, 460)], [(150, 0, 450)], [(697, 0, 40)]],
                [(42, 460), (40, 450), (20, 40)], 1)
    # through the plans: `fetch_many` and `pick_ap` over the bank's own tables
    plans = [streams.fetch_plan(bank.clocks(b), 0.1 * b, 0.2, 0.05, 200) for b in range(B)]
    sizes = [(streams.span_count(streams.row_spans(p, [s.rows for s in bank.segments[b]])),
              streams.span_count(streams.wave_spans(p, 5, 16000, [s.samples for s in bank.segments[b]]))) for b, p in enumerate(plans)]
    n_rows, n_samples = sum(r for r, _ in sizes), sum(s for _, s in sizes)
    dst = [blocks.up(numpy.full(n + 1, SENTINEL, numpy.uint32)) for n in (n_rows * MC_COLS, n_samples, n_rows * ap_cols)]
    assert bank.fetch_many([0, 1, 2], plans, 5, 16000, dst[0] + 4, dst[1] + 4) == sizes and n_rows >= 60
    got = blocks.down(dst[0], n_rows * MC_COLS + 1)
    assert got[0] == SENTINEL and not (got[1:] == SENTINEL).any()
    keep = [(1, r - 1) for r, _ in sizes]
    assert bank.pick_ap([0, 1, 2], plans, keep, up_mask(blocks, numpy.ones(n_rows, numpy.uint8)), dst[2] + 4) == n_rows - 6
    got = blocks.down(dst[2], n_rows * ap_cols + 1)
    assert got[0] == SENTINEL and not (got[1:(n_rows - 6) * ap_cols + 1] == SENTINEL).any() and (got[(n_rows - 6) * ap_cols + 1:] == SENTINEL).all()
    mc1, ap1, wave1 = bank.download(0, bank.segments[0][-1])             # a segment that wraps, brought down whole
    assert numpy.array_equal(R.u32(mc1), numpy.concatenate([models[0].mc[63:], models[0].mc[:20]])) and ap1.shape == (21, ap_cols) and wave1.size == 230
    bank.poison()                                         # poison covers only what is not live, per stream
    assert_bank(bank, blocks, [poisoned(m) for m in models])
    bank.reset(1)
    assert bank.held(1) == (0, 0) and bank.segments[1] == [] and bank.held(0) == (models[0].row_live, models[0].sample_live)
    bank.reset()
    assert all(bank.held(b) == (0, 0) and bank.segments[b] == [] for b in range(B))
    bank.close()
    for s in stores:
        s.close()
    blocks.close()


def poisoned(model):
    """The model after `ry_rowbank_debug_poison`: every position that is not live holds the poison word."""
    out = R.Model(model.cols[1])
    out.row_tail, out.row_live, out.sample_tail, out.sample_live = model.row_tail, model.row_live, model.sample_tail, model.sample_live
    rows = (model.row_tail + numpy.arange(model.row_live)) % CAP_ROWS
    samples = (model.sample_tail + numpy.arange(model.sample_live)) % CAP_SAMPLES
    out.mc[rows], out.ap[rows], out.wave[samples] = model.mc[rows], model.ap[rows], model.wave[samples]
    return out


def check_refusals(ctx, ap_cols):
    """Every refusal by return code, each leaving the rings, the live counts and the destinations as they were; then a good call."""
    rng = numpy.random.default_rng([ap_cols, 34])
    blocks = R.Blocks(ctx)
    bank = streams.RowBank(B, MC_COLS, ap_cols, CAP_ROWS, CAP_SAMPLES, ctx=ctx)
    bank.poison()
    models = [R.Model(ap_cols) for _ in range(B)]
    mc, ap, wave = source(rng, 64, ap_cols, 700)
    src = [blocks.up(a) for a in (mc, ap, wave)]
    for k in range(2):
        bank.append_many([0, 2], [0.1 * k] * 2, src, [(0, 21), (0, 21)], [(0, 230), (0, 230)])
        for b in (0, 2):
            models[b].append(mc[:21], ap[:21], wave[:230])
    bank.retire(2, 1)
    models[2].retire(21, 230)                             # stream 0: rows 0 .. 41 live; stream 1: nothing; stream 2: rows 21 .. 41, samples 230 .. 459
    lib, h = bank._get()
    dll = lib.dll
    ok = ([0, 2], src, [0, 0], [1, 1], [0, 0], [1, 1])
    bad_appends = [([2, 0],) + ok[1:], ([0, 0],) + ok[1:], ([0, 3],) + ok[1:], ([-1, 2],) + ok[1:],                 # descending, repeated, outside the bank
                   (ok[0], [0, src[1], src[2]]) + ok[2:], (ok[0], [src[0], 0, src[2]]) + ok[2:], (ok[0], [src[0], src[1], 0]) + ok[2:],
                   ok[:2] + ([0, -1],) + ok[3:], ok[:3] + ([1, -1],) + ok[4:], ok[:4] + ([-1, 0],) + ok[5:], ok[:5] + ([1, -1],),
                   ok[:3] + ([23, 1],) + ok[4:], ok[:3] + ([1, 44],) + ok[4:], ok[:5] + ([1, 471],), ok[:5] + ([241, 1],)]   # the second stream of the call does not fit
    for args in bad_appends:
        rc, rp, sp = raw_append(bank, *args)
        assert rc == EINVAL and (rp == -7).all() and (sp == -7).all(), args
    assert raw_append(bank, *ok, null_out=True)[0] == EINVAL
    assert raw_append(bank, [0, 1, 2, 0], src, [0] * 4, [1] * 4, [0] * 4, [1] * 4)[0] == EINVAL           # more entries than streams
    assert dll.ry_rowbank_append(None, 0, None, None, None, None, None, None, None, None, None, None) == ESTATE
    for want, args in ((EINVAL, (h, 0, 43, 0)), (EINVAL, (h, 2, 22, 0)), (EINVAL, (h, 2, 0, 231)), (EINVAL, (h, 1, 1, 0)), (EINVAL, (h, 0, -1, 0)),
                       (EINVAL, (h, 3, 0, 0)), (EINVAL, (h, -1, 0, 0)), (ESTATE, (None, 0, 0, 0))):
        assert dll.ry_rowbank_retire(*args) == want, args[1:]
    assert dll.ry_rowbank_reset(h, 3) == EINVAL and dll.ry_rowbank_reset(h, -2) == EINVAL and dll.ry_rowbank_reset(None, 0) == ESTATE
    r, s = ctypes.c_int(), ctypes.c_int()
    assert dll.ry_rowbank_held(h, 3, ctypes.byref(r), ctypes.byref(s)) == EINVAL and dll.ry_rowbank_held(h, 0, None, ctypes.byref(s)) == EINVAL
    # fetch and pick: two streams, windows of 30 / 25 rows and 300 / 240 samples
    part, fo, so = [0, 2], [0, 30, 55], [0, 300, 540]
    sizes = [55 * MC_COLS, 540, 55 * ap_cols]
    dst = [blocks.up(numpy.full(n, SENTINEL, numpy.uint32)) for n in sizes]
    good_r, good_s = [[(0, 0, 30)], [(21, 2, 21)]], [[(0, 0, 300)], [(230, 5, 230)]]
    bad_rows = [[(21, 0, -1)], [(21, -1, 2)], [(21, 5, 21)], [(64, 0, 1)], [(-2, 0, 1)], [(20, 0, 2)], [(41, 0, 2)], [(42, 0, 1)], [(0, 0, 1)], [(21, 24, 2)]]
    bad_samples = [[(230, 0, -1)], [(230, -1, 2)], [(230, 11, 230)], [(700, 0, 1)], [(-2, 0, 1)], [(229, 0, 2)], [(459, 0, 2)], [(460, 0, 1)], [(699, 0, 2)]]
    fetch = lambda *a, **k: raw_fetch(bank, *a, **k)
    for spans in bad_rows:                                # the second stream's spans against ITS ring and ITS slice (rows live in stream 0 are not in 2)
        assert fetch(part, [good_r[0], spans], good_s, dst[0], dst[1], fo, so) == EINVAL, spans
    for spans in bad_samples:
        assert fetch(part, good_r, [good_s[0], spans], dst[0], dst[1], fo, so) == EINVAL, spans
    assert fetch(part, [[(0, 0, 31)], good_r[1]], good_s, dst[0], dst[1], fo, so) == EINVAL              # into the next stream's slice
    assert fetch([0, 1], [good_r[0], [(0, 0, 1)]], good_s, dst[0], dst[1], fo, so) == EINVAL             # stream 1 holds nothing
    for bad_part in ([2, 0], [2, 2], [0, 3], [-1, 2]):
        assert fetch(bad_part, good_r, good_s, dst[0], dst[1], fo, so) == EINVAL, bad_part
    for bad_fo, bad_so in (([1, 30, 55], so), ([0, 30, 29], so), (fo, [1, 300, 540]), (fo, [0, 300, 299])):
        assert fetch(part, good_r, good_s, dst[0], dst[1], bad_fo, bad_so) == EINVAL, (bad_fo, bad_so)
    assert fetch(part, good_r, good_s, dst[0], dst[1], fo, so, ro=[1, 1, 2]) == EINVAL and fetch(part, good_r, good_s, dst[0], dst[1], fo, so, ro=[0, 2, 1]) == EINVAL
    assert fetch(part, good_r, good_s, dst[0], dst[1], fo, so, wo=[1, 1, 2]) == EINVAL and fetch(part, good_r, good_s, dst[0], dst[1], fo, so, wo=[0, 2, 1]) == EINVAL
    assert fetch(part, good_r, good_s, 0, dst[1], fo, so) == EINVAL and fetch(part, good_r, good_s, dst[0], 0, fo, so) == EINVAL
    assert dll.ry_rowbank_fetch(None, 0, None, None, None, None, None, None, None, None, None) == ESTATE
    assert b'retired' in (fetch(part, [good_r[0], [(20, 0, 2)]], good_s, dst[0], dst[1], fo, so), dll.ry_last_error())[1]
    mask = up_mask(blocks, numpy.ones(55, numpy.uint8))
    keep = [(1, 29), (2, 23)]
    pick = lambda *a: raw_pick(bank, *a)
    for spans in bad_rows:
        assert pick(part, [good_r[0], spans], fo, keep, mask, dst[2], 49) == EINVAL, spans
    for bad_keep, rows in (([(-1, 29), keep[1]], 51), ([(1, 31), keep[1]], 51), ([(5, 4), keep[1]], 20), ([keep[0], (2, 26)], 52)):
        assert pick(part, good_r, fo, bad_keep, mask, dst[2], rows) == EINVAL, bad_keep
    assert pick(part, good_r, fo, keep, mask, dst[2], 48) == EINVAL and pick(part, good_r, fo, keep, mask, dst[2], 50) == EINVAL
    assert pick(part, good_r, fo, keep, 0, dst[2], 49) == EINVAL and pick(part, good_r, fo, keep, mask, 0, 49) == EINVAL
    assert pick([2, 0], good_r, fo, keep, mask, dst[2], 49) == EINVAL and pick(part, good_r, [0, 30, 29], keep, mask, dst[2], 49) == EINVAL
    assert dll.ry_rowbank_pick_ap(None, 0, None, None, None, None, None, None, None, 0) == ESTATE
    # nothing changed: the rings, the counts, the destinations
    assert_bank(bank, blocks, models)
    for p, n in zip(dst, sizes):
        assert (blocks.down(p, n) == SENTINEL).all()
    # and the bank still works: the good tables, then an append into the room that is left
    assert fetch(part, good_r, good_s, dst[0], dst[1], fo, so) == 0
    got = blocks.down(dst[0], sizes[0])
    assert numpy.array_equal(got[:30 * MC_COLS], models[0].mc[:30].ravel()) and numpy.array_equal(got[32 * MC_COLS:53 * MC_COLS], models[2].mc[21:42].ravel())
    assert pick(part, good_r, fo, keep, mask, dst[2], 49) == 0
    got = blocks.down(dst[2], sizes[2])
    assert numpy.array_equal(got[:28 * ap_cols], models[0].ap[1:29].ravel()) and numpy.array_equal(got[28 * ap_cols:49 * ap_cols], models[2].ap[21:42].ravel())
    assert (got[49 * ap_cols:] == SENTINEL).all()
    rc, rp, sp = raw_append(bank, [0, 1, 2], src, [0, 1, 2], [22, 64, 43], [0, 0, 0], [240, 700, 470])   # exactly the room each stream has
    assert rc == 0 and list(rp) == [42, 0, 42] and list(sp) == [460, 0, 460]
    hc = ctypes.c_void_p()
    for args in ((0, MC_COLS, ap_cols, 4, 4), (-1, MC_COLS, ap_cols, 4, 4), (65537, MC_COLS, ap_cols, 4, 4), (B, 0, ap_cols, 4, 4), (B, MC_COLS, 0, 4, 4),
                 (B, MC_COLS, ap_cols, 0, 4), (B, MC_COLS, ap_cols, 4, 0), (B, 65537, 1, 4, 4), (B, MC_COLS, ap_cols, (1 << 22) + 1, 4), (B, 65536, 1, 1 << 15, 4),
                 (1 << 16, 256, 1, 1 << 22, 4), (1 << 16, 1, 1, 4, 1 << 30)):                             # the last two: more than 2^40 floats in an array
        assert dll.ry_rowbank_create(ctx.handle, *args, ctypes.byref(hc)) == EINVAL and not hc.value, args
    assert dll.ry_rowbank_create(None, B, MC_COLS, ap_cols, 4, 4, ctypes.byref(hc)) == EINVAL
    assert dll.ry_rowbank_create(ctx.handle, B, MC_COLS, ap_cols, 4, 4, None) == EINVAL
    bank.close()
    blocks.close()
