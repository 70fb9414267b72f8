"""Cases the emulator and the GPU tests of the streaming tracker share (test_crepe_stream_cpu.py, test_crepe_stream_gpu.py), and the rule that says
which activation rows a window may take from the previous one -- restated here from DESIGN.md section 18 in numpy, independently of the C++.

The rule.  Window k - 1 had n_old samples at rate sr, window k has n_new; the caller declares an advance a: x_new[i] is x_old[i + a].  Rows are kept
only when all four hold, otherwise every frame is computed:
 1. overlap: 0 <= a < n_old and the 32-bit patterns of x_new[:m] and x_old[a:a + m] are equal, m = min(n_new, n_old - a);
 2. alignment: a16 = a * 16000 / sr is a whole number and a multiple of hop; the frame shift is d = a16 / hop;
 3. phase: at sr != 16000 the time register repeats exactly, tr[t + a16] == tr[t] + a as doubles for every output t of the overlap (and with it
    the first tap int(tr) and the fraction tr - int(tr), the two numbers the resampler takes from it);
 4. network: rate, hop and the arithmetic of the GEMMs are those of the previous call.
An output t of a window read as n_in samples long is clean when neither tap loop of the resampler is cut by an end of the signal (room >= lim on
both sides; at 16 kHz every sample is clean).  Frame f is portable in it when [f * hop - 512, f * hop + 512) lies inside the 16 kHz signal and
holds clean outputs only.  Frame j of the new window takes the row of old frame j + d iff old frame j + d was portable in the old window (n_old)
and frame j is portable in the new window read as m samples long.  Every other frame is computed."""
import ctypes

import numpy

from realtime_yukarin_amd import _lib, crepe

FRAME, HALF, BINS = 1024, 512, 360


def bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view({8: numpy.uint64, 4: numpy.uint32, 1: numpy.uint8}[a.dtype.itemsize])


def same(a, b) -> bool:
    a, b = numpy.asarray(a), numpy.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(numpy.array_equal(bits(a), bits(b)))


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------------
def length16(n_in: int, sr: int) -> int:
    return int(n_in) if sr == 16000 else int(int(n_in) * (16000.0 / sr))


def clean_outputs(sr: int, n_in: int) -> numpy.ndarray:
    """bool per 16 kHz output of a window of n_in samples at sr: neither tap loop of `crepe.resample` is cut by an end of the signal."""
    n16 = length16(n_in, sr)
    if sr == 16000 or n16 < 1:
        return numpy.ones(max(n16, 0), bool)
    ratio = 16000.0 / sr
    scale = min(1.0, ratio)
    win, num_table, step = crepe.resampler_tables(sr)
    tr = crepe.time_register(sr, n16)
    n = tr.astype(numpy.int64)
    frac0 = scale * (tr - n)
    ok = numpy.ones(n16, bool)
    for side in (0, 1):
        frac = scale - frac0 if side else frac0
        offset = (frac * num_table).astype(numpy.int64)
        lim = (win.size - offset) // step
        room = n_in - n - 1 if side else n + 1
        ok &= room >= lim
    return ok


def portable_frames(sr: int, n_in: int, hop: int) -> numpy.ndarray:
    """bool per frame of a window of n_in samples at sr: its 1024 samples lie inside the 16 kHz signal and are all clean."""
    n16 = length16(n_in, sr)
    if n16 < 1:
        return numpy.zeros(0, bool)
    clean = clean_outputs(sr, n_in)
    out = numpy.zeros(1 + n16 // hop, bool)
    for f in range(out.size):
        lo, hi = f * hop - HALF, f * hop + HALF
        out[f] = lo >= 0 and hi <= n16 and bool(clean[lo:hi].all())
    return out


def register_repeats(sr: int, a: int, a16: int, n_check: int) -> bool:
    if sr == 16000 or n_check < 1:
        return True
    tr = crepe.time_register(sr, n_check + a16)
    new, old = tr[:n_check], tr[a16:a16 + n_check]
    return bool(numpy.all(old == new + float(a)) and numpy.all(old.astype(numpy.int64) == new.astype(numpy.int64) + a) and
                numpy.all(old - numpy.floor(old) == new - numpy.floor(new)))


class Rule(object):
    """The host-side account of a stream: what the rule lets each push keep, from the windows alone."""

    def __init__(self):
        self.prev = None

    def reset(self):
        self.prev = None

    def push(self, x, sr: int, hop: int, advance, dtype: str = 'f32'):
        """-> (src [frames]: the old frame a row comes from or -1, computed frames); the window becomes the previous one."""
        x = numpy.ascontiguousarray(x, numpy.float32)
        nf = 1 + length16(x.size, sr) // hop
        src = numpy.full(nf, -1, numpy.int64)
        p = self.prev
        if p is not None and advance is not None and 0 <= advance < p['x'].size and (sr, hop, dtype) == (p['sr'], p['hop'], p['dtype']):
            m = min(x.size, p['x'].size - advance)
            overlap = numpy.array_equal(bits(x[:m]), bits(p['x'][advance:advance + m]))
            aligned = (advance * 16000) % sr == 0 and (advance * 16000 // sr) % hop == 0
            if overlap and aligned:
                a16 = advance * 16000 // sr
                d = a16 // hop
                if register_repeats(sr, advance, a16, min(length16(m, sr), length16(p['x'].size, sr) - a16)):
                    new = portable_frames(sr, m, hop)
                    for j in range(min(nf, new.size)):
                        if new[j] and j + d < p['portable'].size and p['portable'][j + d]:
                            src[j] = j + d
        self.prev = dict(x=x.copy(), sr=sr, hop=hop, dtype=dtype, portable=portable_frames(sr, x.size, hop))
        return src, int((src < 0).sum())

    def portable_kept(self) -> int:
        return 0 if self.prev is None else int(self.prev['portable'].sum())


# ---- signals and sequences ---------------------------------------------------------------------------------------------------------------
def signal(sr: int, n: int, seed: int = 0) -> numpy.ndarray:
    """float32: a gliding tone with noise, so that frames differ and some are voiced."""
    rng = numpy.random.default_rng([seed, sr])
    t = numpy.arange(n) / sr
    x = 0.4 * numpy.sin(2 * numpy.pi * (180.0 + 60.0 * t) * t) + 0.05 * rng.normal(0, 1, n)
    return x.astype(numpy.float32)


def slices(sr, starts, lengths, advances, seed=0):
    """[(window, declared advance)]: slices of one signal."""
    x = signal(sr, max(s + n for s, n in zip(starts, lengths)), seed)
    return [(x[s:s + n].copy(), a) for s, n, a in zip(starts, lengths, advances)]


def _flipped():
    w = slices(16000, (0, 480, 960), (2400,) * 3, (None, 480, 480))
    x = w[1][0]
    bits(x)[700] ^= 1                                                  # one bit of a sample inside the overlap with the first window
    w[2] = (w[2][0], 480)
    w[2][0][:1920] = x[480:]                                           # the third window overlaps the second as it now is
    return w


def _signed_zero():
    w = slices(16000, (0, 480, 960), (2400,) * 3, (None, 480, 480))
    w[0][0][480 + 900] = 0.0
    w[1][0][900] = -0.0                                                # equal as numbers, different as words
    w[2][0][420] = -0.0                                                # the third window overlaps the second as it now is
    w[1][0][480 + 1000] = 0.0
    w[2][0][1000] = 0.0
    return w


# name -> dict(sr, hop, step (ms), windows = [(samples, declared advance)], reuse: a push after the first keeps rows)
SEQUENCES = {
    # 41 frames, 7 edge frames each side
    '16k_3200_800': dict(sr=16000, hop=80, step=5, reuse=True, windows=lambda: slices(16000, (0, 800, 1600), (3200,) * 3, (None, 800, 800))),
    '24k_4800_1200': dict(sr=24000, hop=80, step=5, reuse=True, windows=lambda: slices(24000, (0, 1200, 2400), (4800,) * 3, (None, 1200, 1200))),
    # the small geometry: 2400 samples at 16 kHz, hop 160 -> 16 frames, frames 4 .. 11 portable
    '48k': dict(sr=48000, hop=160, step=10, reuse=True, windows=lambda: slices(48000, (0, 1440, 2880), (7200,) * 3, (None, 1440, 1440))),
    'advance_0': dict(sr=16000, hop=160, step=10, reuse=True, windows=lambda: slices(16000, (0, 0, 0), (2400,) * 3, (None, 0, 0))),
    'fractional_advance': dict(sr=24000, hop=160, step=10, reuse=False, windows=lambda: slices(24000, (0, 721, 1442), (3600,) * 3, (None, 721, 721))),
    'advance_off_the_hop': dict(sr=16000, hop=160, step=10, reuse=False, windows=lambda: slices(16000, (0, 400, 800), (2400,) * 3, (None, 400, 400))),
    'advance_past_the_window': dict(sr=16000, hop=160, step=10, reuse=False,
                                    windows=lambda: slices(16000, (0, 2400, 5000), (2400,) * 3, (None, 2400, 2600))),
    '44k1': dict(sr=44100, hop=160, step=10, reuse=False, windows=lambda: slices(44100, (0, 1323, 2646), (6615,) * 3, (None, 1323, 1323))),
    'grow_and_shrink': dict(sr=16000, hop=160, step=10, reuse=True,
                            windows=lambda: slices(16000, (0, 480, 960, 1440), (2400, 3200, 1760, 2400), (None, 480, 480, 480))),
    'grow_and_shrink_24k': dict(sr=24000, hop=160, step=10, reuse=True,
                                windows=lambda: slices(24000, (0, 720, 1440, 2160), (3600, 4800, 2640, 3600), (None, 720, 720, 720))),
    'shorter_than_a_frame': dict(sr=16000, hop=160, step=10, reuse=False, windows=lambda: slices(16000, (0, 160, 320), (800,) * 3, (None, 160, 160))),
    'flipped_bit': dict(sr=16000, hop=160, step=10, reuse=None, windows=_flipped),
    'signed_zero': dict(sr=16000, hop=160, step=10, reuse=None, windows=_signed_zero),
    'small_16k': dict(sr=16000, hop=160, step=10, reuse=True, windows=lambda: slices(16000, (0, 480, 960), (2400,) * 3, (None, 480, 480))),
    'small_24k': dict(sr=24000, hop=160, step=10, reuse=True, windows=lambda: slices(24000, (0, 720, 1440), (3600,) * 3, (None, 720, 720))),
    'other_signal': dict(sr=16000, hop=160, step=10, reuse=True, windows=lambda: slices(16000, (0, 480, 960), (2400,) * 3, (None, 480, 480), seed=7)),
    # 601 frames advancing 280: the first push runs three passes, the packed list of the later ones (294 frames) crosses a pass of 256
    '601_frames': dict(sr=16000, hop=80, step=5, reuse=True, windows=lambda: slices(16000, (0, 22400, 44800), (48000,) * 3, (None, 22400, 22400))),
    'pair': dict(sr=24000, hop=80, step=5, reuse=True, windows=lambda: slices(24000, (0, 1200), (4800,) * 2, (None, 1200))),
}


# ---- the reference: `track` and `predict` of every window on a separate handle of the same weights, computed once ---------------------------
class Reference(object):
    def __init__(self, ctx, capacity, seed=3):
        self.ctx, self.capacity, self.seed = ctx, capacity, seed
        self.models, self.results = {}, {}

    def model(self, dtype):
        if dtype not in self.models:
            self.models[dtype] = crepe.CrepeModel(self.capacity, seed=self.seed, ctx=self.ctx, dtype=dtype)
        return self.models[dtype]

    def of(self, x, sr, hop, step, dtype='f32'):
        """-> (voiced, f0, t, activation, confidence), read-only."""
        key = (dtype, sr, hop, step, x.tobytes())
        if key not in self.results:
            m = self.model(dtype)
            voiced, f0, t = m.track(x, sr, hop, step)
            _, conf, act = m.predict(x, sr, hop, activation=True)
            out = (voiced, f0, t, act, conf)
            for a in out:
                a.setflags(write=False)
            self.results[key] = out
        return self.results[key]

    def close(self):
        for m in self.models.values():
            m.close()
        self.models, self.results = {}, {}


def new_model(ctx, capacity, dtype='f32', seed=3):
    return crepe.CrepeModel(capacity, seed=seed, ctx=ctx, dtype=dtype)


def check_push(stream, rule, ref, x, sr, hop, step, advance, dtype='f32', poison=False):
    """One push: the bits of the reference, and as many frames through the network as the restated rule counts.  -> (computed, frames)."""
    if poison:
        assert stream.poison() == rule.portable_kept()
    got = stream.track(x, sr, hop, step, advance=advance)
    src, computed = rule.push(x, sr, hop, advance, dtype)
    voiced, f0, t, act, conf = ref.of(x, sr, hop, step, dtype)
    assert (stream.computed, stream.frames) == (computed, src.size), (stream.computed, stream.frames, computed, src.size)
    assert same(got[0], voiced) and same(got[1], f0) and same(got[2], t)
    a = stream.activation()
    assert same(a, act) and same(a.max(axis=1), conf)
    return computed, src.size


def run_sequence(ctx, ref, name, dtype='f32', poison=False, model=None):
    """The pushes of SEQUENCES[name] through a fresh stream.  -> [(computed, frames)] per push."""
    case = SEQUENCES[name]
    own = model is None
    model = new_model(ctx, ref.capacity, dtype) if own else model
    stream, rule, out = crepe.CrepeStream(model), Rule(), []
    try:
        for x, advance in case['windows']():
            out.append(check_push(stream, rule, ref, x, case['sr'], case['hop'], case['step'], advance, dtype, poison))
    finally:
        stream.close()
        if own:
            model.close()
    if case['reuse'] is True:
        assert all(c < n for c, n in out[1:]), out
    elif case['reuse'] is False:
        assert all(c == n for c, n in out), out
    assert out[0][0] == out[0][1]
    return out


# ---- the assembling kernel alone ------------------------------------------------------------------------------------------------------------
def check_assemble(ctx):
    """`ry_crepe_stream_debug_assemble`: one row; sources at the first and the last row of either block; several workgroups of rows; an index outside
    its block writes nothing; the guard rows behind the destination keep their bits."""
    model = new_model(ctx, 1)
    stream = crepe.CrepeStream(model)
    lib, h = stream._get()
    rng = numpy.random.default_rng(11)
    n_keep, n_fresh, guard = 5, 3, 2
    keep = rng.normal(size=(n_keep, BINS)).astype(numpy.float32)
    fresh = rng.normal(size=(n_fresh, BINS)).astype(numpy.float32)
    keep[2, 7] = numpy.nan
    blocks = [ctx.dev_alloc(keep.size), ctx.dev_alloc(fresh.size)]
    ctx.dev_upload(blocks[0], keep)
    ctx.dev_upload(blocks[1], fresh)
    cases = ([0], [-1], [n_keep - 1], [-n_fresh], [0, n_keep - 1, -1, -n_fresh], [n_keep, -n_fresh - 1, 1, -2 ** 31, 2 ** 31 - 1],
             list(rng.integers(-n_fresh, n_keep, 23)))
    for src in cases:
        src = numpy.asarray(src, numpy.int32)
        n = src.size
        before = rng.normal(size=(n + guard, BINS)).astype(numpy.float32)
        out = ctx.dev_alloc(before.size)
        ctx.dev_upload(out, before)
        lib.check(lib.dll.ry_crepe_stream_debug_assemble(h, _lib._fptr(blocks[0]), n_keep, _lib._fptr(blocks[1]), n_fresh,
                                                         src.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n, _lib._fptr(out)))
        got = numpy.empty_like(before)
        ctx.dev_download(out, got)
        want = before.copy()
        for j, s in enumerate(src.tolist()):
            if 0 <= s < n_keep:
                want[j] = keep[s]
            elif s < 0 and -1 - s < n_fresh:
                want[j] = fresh[-1 - s]
        assert same(got, want), src.tolist()
        ctx.dev_free(out)
    null = _lib._fptr(None)
    one = numpy.zeros(1, numpy.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    good = [h, _lib._fptr(blocks[0]), n_keep, _lib._fptr(blocks[1]), n_fresh, one, 1, _lib._fptr(blocks[0])]
    for i, bad in ((0, None), (1, null), (3, null), (5, None), (7, null), (2, -1), (4, -1), (6, 0)):
        args = list(good)
        args[i] = bad
        assert lib.dll.ry_crepe_stream_debug_assemble(*args) != 0, i
    for b in blocks:
        ctx.dev_free(b)
    stream.close()
    model.close()
