"""Cases the emulator and the GPU tests of the many-waves wave-to-wave chain share (test_pipeline_many_cpu.py, test_pipeline_many_gpu.py).  The yardstick
of every comparison is the shipped single-wave call in the same process -- `ry_vc_gate`, `Analyzer.extract_resident`, `ry_vc_enqueue_wave_device`,
numpy for `ry_gather_rows`, a lone `Pipeline` for `PipelineBank` -- and every comparison is bit equality (`pipeline_cases.same`)."""
import ctypes
import itertools

import numpy

import pipeline_cases as P
from realtime_yukarin_amd import _lib, crepe, gate, world_analysis

GUARD = 0xA5A5A5A5                      # the word every guard and every unwritten part of an output block holds
UB, IP, LLP = ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)


class Blocks(object):
    """Device blocks of 4-byte words, freed with the object."""

    def __init__(self, ctx):
        self.ctx, self.all = ctx, []

    def filled(self, words: int, value=GUARD) -> int:
        p = self.ctx.dev_alloc(max(words, 1))
        self.all.append(p)
        self.ctx.dev_upload(p, numpy.full(max(words, 1), value, numpy.uint32))
        return p

    def of(self, a) -> int:
        raw = numpy.ascontiguousarray(a).tobytes()
        raw += b'\0' * (-len(raw) % 4)
        words = numpy.frombuffer(raw or b'\0\0\0\0', numpy.uint32)
        p = self.ctx.dev_alloc(words.size)
        self.all.append(p)
        self.ctx.dev_upload(p, words)
        return p

    def read(self, p: int, words: int) -> numpy.ndarray:
        out = numpy.empty(words, numpy.uint32)
        self.ctx.dev_download(p, out)
        return out

    def close(self):
        for p in self.all:
            self.ctx.dev_free(p)
        self.all = []


# ---- ry_gather_rows -------------------------------------------------------------------------------------------------------------------
def gather_reference(rows, src, mask):
    out = rows[src].copy()
    if mask is not None:
        out[~mask[src].astype(bool)] = 0.0
    return out


def gather_cases():
    """(cols, n_rows, index table, mask or None, word offset of the source block, of the destination): 1 .. 22 output rows; 513 columns (consecutive
    rows start at every residue, on both sides), 6, 4 and 1; identity, reversed and repeated indices; no mask, all-0, all-1 and alternating masks;
    every pair of base residues at 513 columns."""
    out = []
    kinds = ('identity', 'reversed', 'repeated')
    masks = ('none', 'zeros', 'ones', 'alt')
    combos = list(itertools.product(kinds, masks))
    k = 0
    for cols in (513, 6, 4, 1):
        for n_out in (range(1, 23) if cols == 513 else (1, 9, 22)):
            for kind, mk in (combos if n_out in (1, 5, 22) else [combos[k % len(combos)]]):
                out.append((cols, n_out, kind, mk, k % 4, (k // 4) % 4))
                k += 1
    for so, do in itertools.product(range(4), range(4)):
        out.append((513, 5, 'reversed', 'alt', so, do))
    return out


def check_gather_rows(ctx):
    rng = numpy.random.default_rng(11)
    for cols, n_out, kind, mk, s_off, d_off in gather_cases():
        n_rows = n_out + 3 if kind != 'repeated' else max(n_out // 2, 1)
        rows = rng.normal(size=(n_rows, cols)).astype(numpy.float32)
        rows[rng.uniform(size=rows.shape) < 0.05] = numpy.nan
        src = numpy.arange(n_out)
        src = (src[::-1] + 3 if kind == 'reversed' else src % n_rows if kind == 'repeated' else src).astype(numpy.int32)
        alt = (numpy.arange(n_rows) % 2).astype(numpy.uint8)
        mask = {'none': None, 'zeros': numpy.zeros(n_rows, numpy.uint8), 'ones': numpy.ones(n_rows, numpy.uint8), 'alt': alt}[mk]
        B = Blocks(ctx)
        src_block = B.of(numpy.concatenate([numpy.zeros(s_off, numpy.float32), rows.ravel()]))
        table = B.of(src)
        mask_block = B.of(mask) if mask is not None else None
        total = d_off + (n_out + 2) * cols + 4                           # a guard row in front and behind, and the base offset
        dst = B.filled(total)
        ctx.gather_rows(src_block + 4 * s_off, n_rows, cols, table, dst + 4 * (d_off + cols), n_out, mask_ptr=mask_block)
        ctx.sync()
        got = B.read(dst, total)
        want = numpy.full(total, GUARD, numpy.uint32)
        want[d_off + cols:d_off + (n_out + 1) * cols] = P.bits(gather_reference(rows, src, mask)).ravel()
        assert numpy.array_equal(got, want), (cols, n_out, kind, mk, s_off, d_off)
        B.close()
    # n_out = 0: nothing is launched, nothing is written
    B = Blocks(ctx)
    dst, table, src_block = B.filled(16), B.of(numpy.zeros(4, numpy.int32)), B.of(numpy.ones(16, numpy.float32))
    ctx.gather_rows(src_block, 4, 4, table, dst, 0)
    ctx.sync()
    assert (B.read(dst, 16) == GUARD).all()
    B.close()


def check_gather_rows_refusals(ctx):
    dll, h = ctx.lib.dll, ctx.handle
    B = Blocks(ctx)
    rows, table, mask, dst = B.of(numpy.ones(64, numpy.float32)), B.of(numpy.arange(4, dtype=numpy.int32)), B.of(numpy.ones(4, numpy.uint8)), B.filled(64)
    f, ip, ub = _lib._fptr, lambda a: ctypes.cast(ctypes.c_void_p(a), IP), lambda a: ctypes.cast(ctypes.c_void_p(a), UB)
    good = [h, f(rows), 4, 16, ip(table), ub(mask), f(dst), 4, None]
    assert dll.ry_gather_rows(*good) == 0
    B.ctx.sync()
    ctx.dev_upload(dst, numpy.full(64, GUARD, numpy.uint32))
    for i, bad in ((0, None), (1, f(None)), (4, ip(0)), (6, f(None)), (2, 0), (3, 0), (7, -1)):
        args = list(good)
        args[i] = bad
        assert dll.ry_gather_rows(*args) == -1, i
    args = list(good)
    args[5] = ub(0)                                                        # a null mask keeps every row
    assert dll.ry_gather_rows(*args) == 0
    ctx.sync()
    assert numpy.array_equal(B.read(dst, 64), P.bits(numpy.ones(64, numpy.float32)))
    B.close()


# ---- the gate over many waves ---------------------------------------------------------------------------------------------------------
def gate_single(core, waves, frames, hop, fft, thr):
    rng = numpy.random.default_rng(17)
    cin = core.stage1.desc.in_ch
    feats = [rng.normal(size=(n, cin)).astype(numpy.float32) for n in frames]
    return feats, [core.gate(x, hop, fft, thr[0], thr[1], f) for x, f in zip(waves, feats)]


def check_gate_waves(ctx, core, waves, frames, hop, fft=1024, thr=None, order=None, singles=None):
    """One `ry_vc_gate_waves_device` over `waves` (in `order`) against `ry_vc_gate` per wave: mask, count, x_eff and row_of; the rows behind a wave's
    count and the guard words around every block keep their bits."""
    thr = gate.thresholds(P.THRESHOLD) if thr is None else thr
    feats, want = singles if singles is not None else gate_single(core, waves, frames, hop, fft, thr)
    order = list(range(len(waves))) if order is None else list(order)
    cin = core.stage1.desc.in_ch
    so = numpy.concatenate([[0], numpy.cumsum([waves[i].size for i in order])]).astype(numpy.int64)
    fo = numpy.concatenate([[0], numpy.cumsum([frames[i] for i in order])]).astype(numpy.int32)
    n, g = int(fo[-1]), 8
    B = Blocks(ctx)
    wave_block, feat_block = B.of(numpy.concatenate([waves[i] for i in order])), B.of(numpy.concatenate([feats[i] for i in order]))
    mask_words = (n + 3) // 4
    mask_block, x_block, row_block = B.filled(mask_words + 2 * g), B.filled(n * cin + 2 * g), B.filled(n + 2 * g)
    eff, n_eff = core.gate_waves_device(wave_block, so, fo, hop, fft, thr[0], thr[1], feat_block, mask_block + 4 * g, x_block + 4 * g, row_block + 4 * g)
    ctx.sync()
    mask_got, x_got, row_got = B.read(mask_block, mask_words + 2 * g), B.read(x_block, n * cin + 2 * g), B.read(row_block, n + 2 * g)
    for words in (mask_got, x_got, row_got):
        assert (words[:g] == GUARD).all() and (words[-g:] == GUARD).all()
    mask_bytes = mask_got[g:g + mask_words].view(numpy.uint8)
    tail = numpy.full(mask_words * 4, 0xA5, numpy.uint8)[n:]
    assert numpy.array_equal(mask_bytes[n:], tail)                         # the bytes behind the last frame
    x_got, row_got = x_got[g:g + n * cin].reshape(n, cin), row_got[g:g + n]
    for j, i in enumerate(order):
        m, x, rows = want[i]
        a, b, k = int(fo[j]), int(fo[j + 1]), len(rows)
        what = (i, order)
        assert n_eff[j] == k and numpy.array_equal(eff[a:b], m) and numpy.array_equal(mask_bytes[a:b], m.astype(numpy.uint8)), what
        assert numpy.array_equal(x_got[a:a + k], P.bits(x)) and numpy.array_equal(row_got[a:a + k].view(numpy.int32), rows), what
        assert (x_got[a + k:b] == GUARD).all() and (row_got[a + k:b] == GUARD).all(), what
    B.close()
    return feats, want


def gate_lengths(fs):
    """Three waves of different lengths: one hop, a length that is no multiple of the hop, 0.25 s -> (waves, frames)."""
    hop = fs * P.FRAME_PERIOD // 1000
    sizes = (hop, 7 * hop + 37, int(0.25 * fs))
    waves = [P.wave_of('gap' if n > 2000 else 'loud', fs, n / fs, seed=s)[:n] for s, n in enumerate(sizes)]
    assert [w.size for w in waves] == list(sizes)
    return waves, [1, 8, sizes[2] // hop + 1], hop


def loud_and_quiet(fs):
    """A wave whose maximum reaches the top_db clamp at a 90 dB threshold (every frame effective, its silent middle included) beside one whose own
    maximum stays below it (its silent middle is cut)."""
    from yukarin import Wave
    n = int(0.3 * fs)
    tone = numpy.sin(2 * numpy.pi * 220.0 * numpy.arange(n) / fs)
    loud, quiet = (0.9 * tone).astype(numpy.float32), (0.01 * tone).astype(numpy.float32)
    for x in (loud, quiet):
        x[n // 3:2 * n // 3] = 0
    masks = [Wave(x, fs).get_effective_frame(threshold_db=90.0, fft_length=1024, frame_period=P.FRAME_PERIOD) for x in (loud, quiet)]
    assert masks[0].all() and masks[1].any() and not masks[1].all()       # the host gate: two modes
    return [loud, quiet], [len(m) for m in masks], gate.thresholds(90.0)


def check_gate_waves_refusals(ctx, core):
    """Every refusal by return code, on guard-filled outputs that stay as they were."""
    fs = 16000
    hop = 80
    waves, frames = [P.wave_of('loud', fs, 0.02, seed=s) for s in (0, 1)], [5, 5]
    cin = core.stage1.desc.in_ch
    B = Blocks(ctx)
    wave_block, feat_block = B.of(numpy.concatenate(waves)), B.of(numpy.ones((10, cin), numpy.float32))
    outs = [B.filled(16), B.filled(10 * cin), B.filled(10)]
    so, fo = numpy.array([0, 320, 640], numpy.int64), numpy.array([0, 5, 10], numpy.int32)
    host_mask, counts = numpy.zeros(10, numpy.uint8), numpy.zeros(2, numpy.int32)
    f, ub, ip = _lib._fptr, lambda a: ctypes.cast(ctypes.c_void_p(a), UB), lambda a: ctypes.cast(ctypes.c_void_p(a), IP)
    dll = ctx.lib.dll

    def call(so=so, fo=fo, n_waves=2, hop=hop, fft=1024, **null):
        args = dict(vc=core.handle, wave=f(wave_block), feat=f(feat_block), mask=ub(outs[0]), host=host_mask.ctypes.data_as(UB), count=counts.ctypes.data_as(IP),
                    x=f(outs[1]), rows=ip(outs[2]), so=so.ctypes.data_as(LLP) if so is not None else None, fo=fo.ctypes.data_as(IP) if fo is not None else None)
        args.update(null)
        return dll.ry_vc_gate_waves_device(args['vc'], args['wave'], args['so'], args['fo'], n_waves, hop, fft, 1e-6, 3e38, args['feat'], args['mask'],
                                           args['host'], args['count'], args['x'], args['rows'])
    assert call(vc=None) == -1 and call(wave=f(None)) == -1 and call(feat=f(None)) == -1 and call(mask=ub(0)) == -1 and call(host=None) == -1
    assert call(count=None) == -1 and call(so=None) == -1 and call(fo=None) == -1 and call(x=f(None)) == -1 and call(rows=ip(0)) == -1
    assert call(n_waves=0) == -1 and call(hop=0) == -1 and call(fft=100) == -1 and call(fft=2048) == -1
    assert call(so=numpy.array([1, 320, 640], numpy.int64)) == -1 and call(fo=numpy.array([1, 5, 10], numpy.int32)) == -1
    assert call(so=numpy.array([0, 320, 320], numpy.int64)) == -1 and call(fo=numpy.array([0, 5, 4], numpy.int32)) == -1
    assert b'wave 1' in dll.ry_last_error()
    assert call(n_waves=65537) == -1                                        # the size limits, refused from the offsets alone
    assert call(n_waves=1, so=numpy.array([0, 2 ** 31], numpy.int64), fo=numpy.array([0, 5], numpy.int32)) == -1
    assert call(n_waves=1, so=numpy.array([0, 320], numpy.int64), fo=numpy.array([0, 2 ** 22 + 1], numpy.int32)) == -1
    ctx.sync()
    for p, words in zip(outs, (16, 10 * cin, 10)):
        assert (B.read(p, words) == GUARD).all()
    assert call() == 0 and counts.tolist() == [5, 5]
    B.close()


# ---- Analyzer.extract_many_resident -----------------------------------------------------------------------------------------------------
def check_extract_many_resident(ctx, fs):
    """Three waves (one of a single frame) against `extract_resident` per wave; a refused track and the other refusals leave poisoned blocks poisoned."""
    import encode_cases as E
    cases = [E.analysis_case(fs, n, seed) for seed, n in enumerate((12, 1, 7))]
    a, one = world_analysis.Analyzer(fs, order=P.ORDER, seed=5, ctx=ctx), world_analysis.Analyzer(fs, order=P.ORDER, seed=5, ctx=ctx)
    widths = (P.ORDER + 1, P.BINS, P.BINS)
    want = []
    for x, f0, t in cases:
        dev = E.DeviceArrays(ctx, x, f0, t)
        out = E.DeviceArrays(ctx, *[numpy.full((f0.size, w), numpy.nan, numpy.float32) for w in widths])
        one.extract_resident(dev.address[0], x.size, dev.address[1], dev.address[2], f0.size, *out.address)
        rows = [numpy.empty((f0.size, w), numpy.float32) for w in widths]
        for r, p in zip(rows, out.address):
            ctx.dev_download(p, r)
        want.append(rows)
        dev.close()
        out.close()
    so = numpy.concatenate([[0], numpy.cumsum([c[0].size for c in cases])]).astype(numpy.int64)
    fo = numpy.concatenate([[0], numpy.cumsum([c[1].size for c in cases])]).astype(numpy.int32)
    n = int(fo[-1])
    f0_all = numpy.concatenate([c[1] for c in cases])
    dev = E.DeviceArrays(ctx, numpy.concatenate([c[0] for c in cases]), f0_all, numpy.concatenate([c[2] for c in cases]))
    poison = [numpy.full((n, w), numpy.nan, numpy.float32) for w in widths]
    out = E.DeviceArrays(ctx, *poison)
    a.poison()
    a.extract_many_resident(dev.address[0], so, dev.address[1], dev.address[2], fo, *out.address)
    for k, (p, w) in enumerate(zip(out.address, widths)):
        got = numpy.empty((n, w), numpy.float32)
        ctx.dev_download(p, got)
        for i in range(len(cases)):
            assert P.same(got[fo[i]:fo[i + 1]], want[i][k]), (fs, i, k)
    # refusals: a track the device check refuses, null pointers, offsets
    lib, h = a._get()
    f0b = f0_all.copy()
    f0b[13] = fs / 2
    devb = E.DeviceArrays(ctx, f0b)
    refused = E.DeviceArrays(ctx, *poison)
    outs = [_lib._fptr(p) for p in refused.address]
    null = _lib._fptr(None)

    def call(handle=h, wave=_lib._fptr(dev.address[0]), so=so, f0=dev.address[1], t=dev.address[2], fo=fo, n_waves=3, outs=outs):
        return lib.dll.ry_analysis_extract_many_resident(handle, wave, so.ctypes.data_as(LLP) if so is not None else None, E._DP(f0), E._DP(t),
                                                         fo.ctypes.data_as(IP) if fo is not None else None, n_waves, 0.85, *outs)
    assert call(f0=devb.address[0]) == -1 and b'f0[13]' in lib.dll.ry_last_error(), lib.dll.ry_last_error()
    for i in range(3):
        assert call(outs=[null if j == i else o for j, o in enumerate(outs)]) == -1
    assert call(wave=null) == -1 and call(f0=0) == -1 and call(t=0) == -1 and call(so=None) == -1 and call(fo=None) == -1 and call(n_waves=0) == -1
    assert call(handle=None) == -4
    assert call(so=so + 1) == -1 and call(fo=numpy.array([0, 12, 12, 20], numpy.int32)) == -1
    for p, w in zip(refused.address, widths):
        got = numpy.zeros((n, w), numpy.float32)
        ctx.dev_download(p, got)
        assert numpy.isnan(got).all()
    for d in (dev, out, devb, refused):
        d.close()
    a.close()
    one.close()


# ---- ry_vc_enqueue_waves_device ---------------------------------------------------------------------------------------------------------
class Windows(object):
    """Waves and feature rows on the card, and what `enqueue_wave_device` gives for each wave alone under every discard hint asked for."""

    def __init__(self, ctx, core, waves, frames, hop, fft=1024, thr=None):
        self.ctx, self.core, self.waves, self.frames, self.hop, self.fft = ctx, core, waves, frames, hop, fft
        self.thr = gate.thresholds(P.THRESHOLD) if thr is None else thr
        rng = numpy.random.default_rng(23)
        cin = core.stage1.desc.in_ch
        self.feats = [(rng.normal(size=(n, cin)) * numpy.linspace(4, 0.2, cin)).astype(numpy.float32) for n in frames]
        self.want = {}

    def single(self, discard):
        """[(mc, sp, mask, count)] per wave under `discard`, computed once."""
        if discard not in self.want:
            ctx, core, out = self.ctx, self.core, []
            core.set_discard(*discard)
            for x, f, n in zip(self.waves, self.feats, self.frames):
                B = Blocks(ctx)
                blocks = [B.of(x), B.of(f), B.filled(n * core.M), B.filled(n * core.F), B.filled(n // 4 + 2)]
                eff, n_eff = core.enqueue_wave_device(blocks[0], x.size, self.hop, self.fft, self.thr[0], self.thr[1], blocks[1], n, *blocks[2:])
                ctx.sync()
                out.append((B.read(blocks[2], n * core.M), B.read(blocks[3], n * core.F), eff, n_eff))
                B.close()
            self.want[discard] = out
        return self.want[discard]

    def check(self, discard=(0, 0), order=None):
        ctx, core = self.ctx, self.core
        want = self.single(discard)
        order = list(range(len(self.waves))) if order is None else list(order)
        so = numpy.concatenate([[0], numpy.cumsum([self.waves[i].size for i in order])]).astype(numpy.int64)
        fo = numpy.concatenate([[0], numpy.cumsum([self.frames[i] for i in order])]).astype(numpy.int32)
        n, g = int(fo[-1]), 8
        B = Blocks(ctx)
        wave_block, feat_block = B.of(numpy.concatenate([self.waves[i] for i in order])), B.of(numpy.concatenate([self.feats[i] for i in order]))
        mc_block, sp_block, mask_block = B.filled(n * core.M + 2 * g), B.filled(n * core.F + 2 * g), B.filled((n + 3) // 4 + 2 * g)
        core.set_discard(*discard)
        eff, n_eff = core.enqueue_waves_device(wave_block, so, fo, self.hop, self.fft, self.thr[0], self.thr[1], feat_block, mc_block + 4 * g,
                                               sp_block + 4 * g, mask_block + 4 * g)
        ctx.sync()
        mc, sp, mask = B.read(mc_block, n * core.M + 2 * g), B.read(sp_block, n * core.F + 2 * g), B.read(mask_block, (n + 3) // 4 + 2 * g)
        for words in (mc, sp, mask):
            assert (words[:g] == GUARD).all() and (words[-g:] == GUARD).all()
        mc, sp, mask = mc[g:-g].reshape(n, core.M), sp[g:-g].reshape(n, core.F), mask[g:-g].view(numpy.uint8)
        for j, i in enumerate(order):
            a, b = int(fo[j]), int(fo[j + 1])
            w_mc, w_sp, w_eff, w_n = want[i]
            what = (i, order, discard)
            assert n_eff[j] == w_n and numpy.array_equal(eff[a:b], w_eff) and numpy.array_equal(mask[a:b], w_eff.astype(numpy.uint8)), what
            assert numpy.array_equal(mc[a:b].ravel(), w_mc), what
            assert numpy.array_equal(sp[a:b].ravel(), w_sp), what         # the discarded rows: the guard word on both sides
        B.close()
        core.set_discard(0, 0)


def check_enqueue_waves_refusals(ctx, core):
    fs, hop = 16000, 80
    waves, frames = [P.wave_of('loud', fs, 0.02, seed=s) for s in (0, 1)], [5, 5]
    cin = core.stage1.desc.in_ch
    B = Blocks(ctx)
    wave_block, feat_block = B.of(numpy.concatenate(waves)), B.of(numpy.ones((10, cin), numpy.float32))
    outs = [B.filled(10 * core.M), B.filled(10 * core.F), B.filled(16)]
    so, fo = numpy.array([0, 320, 640], numpy.int64), numpy.array([0, 5, 10], numpy.int32)
    host_mask, counts = numpy.zeros(10, numpy.uint8), numpy.zeros(8, numpy.int32)
    assert core.ring <= 8                                                  # the last call below has one wave of 80 samples and one frame per ring slot
    f, ub = _lib._fptr, lambda a: ctypes.cast(ctypes.c_void_p(a), UB)
    dll = ctx.lib.dll

    def call(so=so, fo=fo, n_waves=2, hop=hop, fft=1024, **null):
        args = dict(vc=core.handle, wave=f(wave_block), feat=f(feat_block), mc=f(outs[0]), sp=f(outs[1]), mask=ub(outs[2]), host=host_mask.ctypes.data_as(UB),
                    count=counts.ctypes.data_as(IP), so=so.ctypes.data_as(LLP) if so is not None else None, fo=fo.ctypes.data_as(IP) if fo is not None else None)
        args.update(null)
        return dll.ry_vc_enqueue_waves_device(args['vc'], args['wave'], args['so'], args['fo'], n_waves, hop, fft, 1e-6, 3e38, args['feat'], 1e-16,
                                              args['mc'], args['sp'], args['mask'], args['host'], args['count'])
    for key, bad in (('vc', None), ('wave', f(None)), ('feat', f(None)), ('mc', f(None)), ('sp', f(None)), ('mask', ub(0)), ('host', None), ('count', None),
                     ):
        assert call(**{key: bad}) == -1, key
    assert call(so=None) == -1 and call(fo=None) == -1
    assert call(n_waves=0) == -1 and call(hop=0) == -1 and call(fft=100) == -1 and call(fft=2048) == -1
    assert call(so=numpy.array([1, 320, 640], numpy.int64)) == -1 and call(fo=numpy.array([2, 5, 10], numpy.int32)) == -1
    assert call(so=numpy.array([0, 640, 320], numpy.int64)) == -1 and call(fo=numpy.array([0, 5, 5], numpy.int32)) == -1
    assert b'wave 1' in dll.ry_last_error()
    # the size limits: more than 65536 waves, 2^31 - 1 samples, 2^22 frames in one call (refused from the offsets alone)
    assert call(n_waves=65537) == -1
    assert call(n_waves=1, so=numpy.array([0, 2 ** 31], numpy.int64), fo=numpy.array([0, 5], numpy.int32)) == -1 and b'sample' in dll.ry_last_error()
    assert call(n_waves=1, so=numpy.array([0, 320], numpy.int64), fo=numpy.array([0, 2 ** 22 + 1], numpy.int32)) == -1 and b'frame' in dll.ry_last_error()
    # a ring slot of the call held by a ticket: RY_ESTATE (-4) until the ticket has been waited for; as many waves as slots, so the held one is met
    ring = core.ring
    eff = numpy.ones(5, bool)
    ticket = core.submit(numpy.ones((5, cin), numpy.float32), eff)
    so6, fo6 = (numpy.arange(ring + 1) * 80).astype(numpy.int64), numpy.arange(ring + 1, dtype=numpy.int32)
    assert call(n_waves=ring, so=so6, fo=fo6) == -4 and b'ticket' in dll.ry_last_error()
    core.wait(ticket)
    ctx.sync()
    for p, words in zip(outs, (10 * core.M, 10 * core.F, 16)):
        assert (B.read(p, words) == GUARD).all()
    assert call(n_waves=ring, so=so6, fo=fo6) == 0 and counts[0] in (0, 1)   # the same call once the slot is free
    ctx.sync()
    B.close()


# ---- PipelineBank -------------------------------------------------------------------------------------------------------------------------
def bank_rounds(fs, seconds, kinds_of_stream):
    """Three rounds over three streams: stream 0 sits the second round out, stream 1 ends (`final`) in the second round and restarts in the third,
    stream 2 is all silent -> [(waves per stream or None, final)]."""
    from yukarin import Wave
    w = lambda kind, seed: Wave(P.wave_of(kind, fs, seconds, seed=seed), fs)
    k0, k1, k2 = kinds_of_stream
    return [([w(k0, 1), w(k1, 2), w(k2, 3)], ()), ([None, w(k1, 4), w(k2, 5)], (1,)), ([w(k0, 6), w(k1, 7), w(k2, 8)], ())]


def check_bank_against_lone_pipelines(bank, lone, rounds, discard):
    """Every return value of `bank.push` / `flush` against the lone pipelines' for the same waves, discards and flushes."""
    live = [False] * len(lone)
    for waves, final in rounds:
        got = bank.push(waves, discard=discard, final=final)
        for s, wave in enumerate(waves):
            if wave is None:
                assert got[s].wave.size == 0
                continue
            want = lone[s].push(wave, discard=discard, final=s in final)
            live[s] = s not in final
            assert got[s].sampling_rate == want.sampling_rate and P.same(got[s].wave, want.wave), (s, final)
    got = bank.flush()
    for s, p in enumerate(lone):
        if live[s]:
            assert P.same(got[s].wave, p.flush().wave), s
        else:
            assert got[s].wave.size == 0, s                               # a stream that ended holds nothing
    return got
