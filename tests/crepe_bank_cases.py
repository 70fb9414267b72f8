"""Cases the emulator and the GPU tests of the bank of streaming trackers share (test_crepe_bank_cpu.py, test_crepe_bank_gpu.py).  The rule that
says which rows a window may keep, the signals and the reference are those of crepe_stream_cases (`Rule`, `portable_frames`, `SEQUENCES`,
`Reference`): one `Rule` per stream of the bank, fed that stream's windows alone, says how many frames each wave may compute -- no more and no
fewer -- and `CrepeModel.track` / `predict` of each window on a separate handle of the same weights say what every wave must hold, bit for bit."""
import ctypes

import numpy

import crepe_stream_cases as S
from realtime_yukarin_amd import _lib, crepe

BINS = S.BINS
_IP = ctypes.POINTER(ctypes.c_int)


def plan(n_streams, per_stream, sit_out=(), orders=None):
    """per_stream[s]: [(window, advance)] of stream s, one per call it takes part in; sit_out: {(call, stream)}; -> [call] with
    call = dict(windows=[array or None per stream], advances=[int or None per stream], order=None or the streams in the call's order)."""
    left = [list(w) for w in per_stream]
    n_calls = max(len(w) + sum(1 for c, s in sit_out if s == i) for i, w in enumerate(left))
    calls = []
    for c in range(n_calls):
        windows, advances = [None] * n_streams, [None] * n_streams
        for s in range(n_streams):
            if (c, s) in sit_out or not left[s]:
                continue
            windows[s], advances[s] = left[s].pop(0)
        calls.append(dict(windows=windows, advances=advances, order=None if orders is None else orders[c]))
    return calls


def three_streams(sr, small=False):
    """Case 1 at 16 or 24 kHz, hop 80: stream 0 has 3200 samples at 16 kHz advancing 800 (41 frames; 24 computed at 16 kHz), stream 1 a shorter
    window with another advance, stream 2 the same window three times (advance 0).  small: the shorter windows of the emulator (21 frames)."""
    k = sr // 8000                                                     # 2 or 3: samples at sr per sample at 8 kHz
    n1, a1, n2 = (800, 80, 800) if small else (1200, 240, 800)
    return [S.slices(sr, (0, 400 * k, 800 * k), (1600 * k,) * 3, (None, 400 * k, 400 * k), seed=0),
            S.slices(sr, (0, a1 * k, 2 * a1 * k), (n1 * k,) * 3, (None, a1 * k, a1 * k), seed=1),
            S.slices(sr, (0, 0, 0), (n2 * k,) * 3, (None, 0, 0), seed=2)]


def sit_out_streams():
    """Case 2 at 16 kHz, hop 160, windows of 16 frames: stream 1 sits call 1 out and returns with an advance that spans both buffers (960 of
    2400 samples)."""
    w = [S.SEQUENCES['small_16k']['windows'](), None, S.SEQUENCES['other_signal']['windows']()]
    w[1] = S.slices(16000, (0, 960), (2400,) * 2, (None, 960), seed=5)
    return w


class Bank(object):
    """A `CrepeStreamBank` over its own model, the restated rule per stream and the checks of one call."""

    def __init__(self, ctx, ref, n_streams, dtype='f32', lone=False):
        self.ctx, self.ref, self.n, self.dtype = ctx, ref, n_streams, dtype
        self.model = S.new_model(ctx, ref.capacity, dtype)
        self.bank = crepe.CrepeStreamBank(self.model, n_streams)
        self.rules = [S.Rule() for _ in range(n_streams)]
        self.lone = [crepe.CrepeStream(self.model) for _ in range(n_streams)] if lone else None      # on the same model: they must not disturb each other
        self.log = []                                                  # per call {stream: (computed, frames)}

    def close(self):
        for s in self.lone or ():
            s.close()
        self.bank.close()
        self.model.close()

    def portable_kept(self):
        return [r.portable_kept() for r in self.rules]

    def call(self, sr, hop, step, windows, advances, order=None, poison=False, dtype=None, device=False):
        """One call: every wave has the bits of the reference on its window, computes what the rule counts, and -- with lone streams -- equals the
        lone `CrepeStream.track` of that stream."""
        dtype = dtype or self.dtype
        if poison:
            assert self.bank.poison() == self.portable_kept()
            self.model.poison()
        got, computed = self.bank.track_many(windows, sr, hop, step, advances=advances, device=device, order=order)
        part = [s for s in range(self.n) if windows[s] is not None] if order is None else list(order)
        if device:
            o = got.frame_offsets
            assert got.waves == len(part) and list(got.sample_offsets) == list(numpy.concatenate([[0], numpy.cumsum([windows[s].size for s in part])]))
            tracks = got.download()
        out = {}
        for i, s in enumerate(part):
            x = windows[s]
            src, want = self.rules[s].push(x, sr, hop, advances[s], dtype)
            voiced, f0, t, act, conf = self.ref.of(x, sr, hop, step, dtype)
            assert (computed[i], self.bank.computed[s], self.bank.frames[s]) == (want, want, src.size), (s, computed[i], want, src.size)
            if device:
                assert int(o[i + 1] - o[i]) == src.size and S.same(tracks[i][0], voiced) and S.same(tracks[i][1], f0), s
            else:
                assert S.same(got[i][0], voiced) and S.same(got[i][1], f0) and S.same(got[i][2], t), s
            a = self.bank.activation(s)
            assert S.same(a, act) and S.same(a.max(axis=1), conf), s
            out[s] = (want, src.size)
        if self.lone:
            for s in part:
                one = self.lone[s].track(windows[s], sr, hop, step, advance=advances[s])
                voiced, f0, t, act, conf = self.ref.of(windows[s], sr, hop, step, dtype)
                assert S.same(one[0], voiced) and S.same(one[1], f0) and S.same(one[2], t), s
                assert (self.lone[s].computed, self.lone[s].frames) == out[s], s
                assert S.same(self.lone[s].activation(), self.bank.activation(s)), s
        self.log.append(out)
        return out

    def run(self, sr, hop, step, calls, poison=False):
        for k, c in enumerate(calls):
            self.call(sr, hop, step, c['windows'], c['advances'], c['order'], poison=poison and k > 0)
        return self.log


def run_plan(ctx, ref, sr, hop, step, per_stream, dtype='f32', poison=False, lone=False, sit_out=(), orders=None):
    """The calls of `plan` through a fresh bank -> [{stream: (computed, frames)}] per call."""
    b = Bank(ctx, ref, len(per_stream), dtype, lone)
    try:
        return b.run(sr, hop, step, plan(len(per_stream), per_stream, sit_out, orders), poison)
    finally:
        b.close()


def run_named(ctx, ref, names, dtype='f32', poison=False, lone=False):
    """One stream per sequence of `crepe_stream_cases.SEQUENCES` (all of one rate, hop and step)."""
    cases = [S.SEQUENCES[n] for n in names]
    sr, hop, step = cases[0]['sr'], cases[0]['hop'], cases[0]['step']
    assert all((c['sr'], c['hop'], c['step']) == (sr, hop, step) for c in cases)
    return run_plan(ctx, ref, sr, hop, step, [c['windows']() for c in cases], dtype, poison, lone)


def all_computed(log, stream):
    return all(c[stream][0] == c[stream][1] for c in log if stream in c)


def keeps_after_the_first(log, stream):
    mine = [c[stream] for c in log if stream in c]
    return mine[0][0] == mine[0][1] and all(c < n for c, n in mine[1:])


# ---- the assembling kernel alone ------------------------------------------------------------------------------------------------------------
def check_assemble_many(ctx):
    """`ry_crepe_bank_debug_assemble`: blocks of row-and-column-coded values; kept rows, fresh rows, indices outside their block on both sides, a
    wave of one frame, a wave that keeps nothing, a wave that keeps everything; several workgroups of rows.  Every row of the call's block and of
    every write slot against a numpy gather; rows with a source outside its block, the guard rows behind every block and the sources keep their
    bits."""
    model = S.new_model(ctx, 1)
    bank = crepe.CrepeStreamBank(model, 2)
    lib, h = bank._get()
    rng = numpy.random.default_rng(13)
    guard = 2
    coded = lambda tag, rows: (tag * 1000000.0 + numpy.arange(rows)[:, None] * 1000.0 + numpy.arange(BINS)[None, :]).astype(numpy.float32)
    n_frames = [7, 1, 5, 6, 9]
    n_keep = [9, 3, 0, 6, 4]
    n_fresh = 11
    src = [[2, -1, 8, -2, 0, -11, 3],                                  # kept and fresh rows, the last row of either block
           [-3],                                                       # a wave of one frame
           [-4, -5, -6, -7, -8],                                       # keeps nothing (and has no kept slot: a null pointer)
           [5, 4, 3, 2, 1, 0],                                         # keeps everything
           [4, -12, 9, -2 ** 31, 2 ** 31 - 1, 3, -1, 0, -11]]          # outside on both sides: 4 of 4 kept rows, -12 of 11 fresh rows, the ends of int
    fresh = coded(9, n_fresh)
    fresh[3, 17] = numpy.nan
    keeps = [coded(1 + i, k) for i, k in enumerate(n_keep)]
    total = sum(n_frames)
    before_out = -coded(7, total + guard)
    before_slots = [-coded(10 + i, n + guard) for i, n in enumerate(n_frames)]

    def up(a):
        p = ctx.dev_alloc(max(a.size, 4))
        if a.size:
            ctx.dev_upload(p, a)
        return p
    d_fresh, d_out = up(fresh), up(before_out)
    d_keeps, d_slots = [up(k) for k in keeps], [up(s) for s in before_slots]
    addr = int                                                         # `dev_alloc` returns the address
    keep_arr = (ctypes.c_void_p * 5)(*[addr(p) if k else None for p, k in zip(d_keeps, n_keep)])
    slot_arr = (ctypes.c_void_p * 5)(*[addr(p) for p in d_slots])
    as_i = lambda v: numpy.ascontiguousarray(v, dtype=numpy.int64).astype(numpy.int32)
    nf, nk, flat = as_i(n_frames), as_i(n_keep), as_i(numpy.concatenate([numpy.asarray(s, numpy.int64) for s in src]))
    ip = lambda a: a.ctypes.data_as(_IP)
    args = [h, ip(nf), 5, keep_arr, ip(nk), slot_arr, _lib._fptr(d_fresh), n_fresh, ip(flat), _lib._fptr(d_out)]
    lib.check(lib.dll.ry_crepe_bank_debug_assemble(*args))
    want_out, want_slots = before_out.copy(), [s.copy() for s in before_slots]
    j = 0
    for i, rows in enumerate(src):
        for local, s in enumerate(rows):
            row = keeps[i][s] if 0 <= s < n_keep[i] else fresh[-1 - s] if s < 0 and -1 - s < n_fresh else None
            if row is not None:
                want_out[j], want_slots[i][local] = row, row
            j += 1
    got = numpy.empty_like(before_out)
    ctx.dev_download(d_out, got)
    assert S.same(got, want_out)
    for i in range(5):
        got = numpy.empty_like(before_slots[i])
        ctx.dev_download(d_slots[i], got)
        assert S.same(got, want_slots[i]), i
        if n_keep[i]:
            got = numpy.empty_like(keeps[i])
            ctx.dev_download(d_keeps[i], got)
            assert S.same(got, keeps[i]), i
    got = numpy.empty_like(fresh)
    ctx.dev_download(d_fresh, got)
    assert S.same(got, fresh)
    # refusals: a null handle, null arrays, no wave, a wave without a frame, a negative count, a kept count without a block, a wave without a slot
    zero = as_i([7, 0, 5, 6, 9])
    neg = as_i([9, -1, 0, 6, 4])
    no_keep = (ctypes.c_void_p * 5)(*[None] * 5)
    no_slot = (ctypes.c_void_p * 5)(*[addr(p) if i != 2 else None for i, p in enumerate(d_slots)])
    for i, bad in ((0, None), (1, None), (2, 0), (3, None), (4, None), (5, None), (6, _lib._fptr(None)), (7, -1), (8, None), (9, _lib._fptr(None)),
                   (1, ip(zero)), (4, ip(neg)), (3, no_keep), (5, no_slot)):
        a = list(args)
        a[i] = bad
        assert lib.dll.ry_crepe_bank_debug_assemble(*a) != 0, i
    for p in [d_fresh, d_out] + d_keeps + d_slots:
        ctx.dev_free(p)
    bank.close()
    model.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def check_refusals(b, sr, hop, step, x, y):
    """Every refusal of `ry_crepe_bank_track` on the bank `b` (two streams or more): its error code, guard-filled outputs untouched, no track
    reported.  x, y: two good windows at sr."""
    lib, h = b.bank._get()
    mh = b.bank._model_handle
    audio = numpy.concatenate([x, y])
    counts, streams = numpy.asarray([x.size, y.size], numpy.int32), numpy.asarray([0, 1], numpy.int32)
    adv, ok = numpy.asarray([0, 0], numpy.int32), numpy.asarray([1, 1], numpy.int32)
    nf, nc = numpy.full(2, -3, numpy.int32), numpy.full(2, -3, numpy.int32)
    voiced, f0, t = numpy.full(4096, 0xA5, numpy.uint8), numpy.full(4096, -7.0), numpy.full(4096, -7.0)
    UB, DP = ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_double)
    ip = lambda a: a.ctypes.data_as(_IP)
    good = [h, _lib._fptr(audio), ip(counts), ip(streams), 2, sr, hop, float(step), 0.1, ip(adv), ip(ok), ip(nf), ip(nc),
            voiced.ctypes.data_as(UB), f0.ctypes.data_as(DP), t.ctypes.data_as(DP), 0]
    uploads = b.bank.uploads()
    b.model.track_many([x, y], sr, hop, step)                          # a track on the card: every refusal with a bank handle forgets it
    f = lib.dll.ry_crepe_bank_track
    arr = lambda *v: ip(numpy.asarray(v, numpy.int32))
    keep_alive = []

    def refused(code, **kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
            keep_alive.append(v)
        assert f(*a) == code, kw
        assert lib.dll.ry_crepe_track_many_buffers(mh, None, None, None, None, None, None, None) == -4      # no track reported
    assert f(None, *good[1:]) == -4
    refused(-1, a1=_lib._fptr(None))
    refused(-1, a2=None)
    refused(-1, a4=0)                                                  # what ry_crepe_track_many refuses: no wave, a wave without a sample,
    refused(-1, a2=arr(x.size, 0))                                     # a hop of 0, a step of 0, a NaN threshold, a rate without tables, null outputs
    refused(-1, a6=0)
    refused(-1, a7=0.0)
    refused(-1, a8=float('nan'))
    refused(-4, a5=22050)
    refused(-1, a11=None)
    refused(-1, a13=None)
    refused(-1, a3=None)                                               # the bank's own: a null stream list, a stream outside the bank on either side,
    refused(-1, a3=arr(0, b.n))                                        # a stream named twice, null advances, null verdicts, a null count
    refused(-1, a3=arr(-1, 1))
    refused(-1, a3=arr(1, 1))
    refused(-1, a9=None)
    refused(-1, a10=None)
    refused(-1, a12=None)
    assert (nf == -3).all() and (nc == -3).all() and (voiced == 0xA5).all() and (f0 == -7.0).all() and (t == -7.0).all()
    assert b.bank.uploads() == uploads                                 # nothing went up
    return len(keep_alive)
