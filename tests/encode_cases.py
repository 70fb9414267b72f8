"""Cases the emulator and the GPU tests of the fused CREPE-mode encode share (test_encode_cpu.py, test_encode_gpu.py): the confidence sets of the
voicing kernel with their host reference, the waves of the track tests, the tracks of the analysis tests.  Every comparison is bit equality: floats
are compared as the unsigned integers of their bytes, so a NaN or a signed zero cannot hide a difference."""
import numpy

from realtime_yukarin_amd import crepe

VOICING_CHUNK = 1024             # CREPE_VOICING_CHUNK of csrc/crepe_kernels.h: frames per pass of the voicing kernel through the LDS
LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, VOICING_CHUNK - 1, VOICING_CHUNK, 2 * VOICING_CHUNK - 1, 2 * VOICING_CHUNK, 2 * VOICING_CHUNK + 1)
STEPS = (5, 10)


def bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view({8: numpy.uint64, 4: numpy.uint32, 1: numpy.uint8}[a.dtype.itemsize])


def same(a, b) -> bool:
    a, b = numpy.asarray(a), numpy.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(numpy.array_equal(bits(a), bits(b)))


def crossing() -> numpy.float32:
    """The confidence between the two means where the two states' log densities cross, from numpy alone: the root of
    c0 + (x - mu0)^2 / v0 = c1 + (x - mu1)^2 / v1 in (mu0, mu1).  An fma or a reordered sum flips a state within a few ulps of it."""
    (m0, m1), (v0, v1) = crepe.VOICING_MEANS, crepe.VOICING_VARS
    c = numpy.log(2 * numpy.pi * numpy.asarray([v0, v1]))
    roots = numpy.roots([1 / v0 - 1 / v1, -2 * m0 / v0 + 2 * m1 / v1, m0 * m0 / v0 - m1 * m1 / v1 + c[0] - c[1]])
    inside = [r.real for r in roots if abs(r.imag) < 1e-12 and m0 < r.real < m1]
    assert len(inside) == 1, roots
    return numpy.float32(inside[0])


def neighbours(x, k: int) -> numpy.ndarray:
    """x and the k float32 values on either side of it, ascending."""
    x = numpy.float32(x)
    lo, hi = [x], [x]
    for _ in range(k):
        lo.append(numpy.nextafter(lo[-1], numpy.float32(-1)))
        hi.append(numpy.nextafter(hi[-1], numpy.float32(2)))
    return numpy.asarray(lo[:0:-1] + hi, numpy.float32)


def confidence_sets(n: int, seed: int = 0):
    """name -> float32 [n]."""
    rng = numpy.random.default_rng([seed, n])
    k = numpy.arange(n)
    out = {'uniform': rng.uniform(0, 1, n), 'zeros': numpy.zeros(n), 'ones': numpy.ones(n)}
    for v in (0.05, 0.0795, 0.3, 0.6278):
        out['const %g' % v] = numpy.full(n, v)
    for period in (1, 2, 7, 400):                                  # switches the 0.9991 / 0.9975 self-transitions do and do not follow
        out['square %d' % period] = numpy.where((k // period) % 2, 0.9, 0.02)
    near = neighbours(crossing(), 3)
    out['crossing'] = near[rng.integers(0, near.size, n)]
    out['crossing ramp'] = near[k % near.size]
    out['threshold'] = neighbours(numpy.float32(0.1), 1)[k % 3]     # float32(0.1) and its two neighbours: the strict `>`
    return {name: numpy.asarray(c, numpy.float32) for name, c in out.items()}


def voicing_reference(c, f0, step):
    """What the chain the kernel replaces computes on the host: the reference wrapper's mask, the f0 it masks, the shim's time axis."""
    c = numpy.asarray(c, numpy.float32)
    voiced = (crepe.predict_voicing(c) == 1) | (c > 0.1)
    f64 = f0.astype(numpy.float64)
    f64[~voiced] = 0
    return voiced, f64, numpy.arange(c.size) * step / 1000.0


def check_voicing(model, n: int, device: bool = False, poison: bool = False):
    """Every confidence set at n frames and both steps against the host; returns how many frames differed anywhere (0)."""
    f0 = numpy.random.default_rng([7, n]).uniform(40.0, 900.0, n).astype(numpy.float32)
    for name, c in confidence_sets(n).items():
        for step in STEPS:
            if poison:
                model.poison()
            voiced, f64, t = model.voicing(c, f0, threshold=0.1, step_size=step, device=device)
            want = voicing_reference(c, f0, step)
            assert voiced.dtype == numpy.bool_ and numpy.array_equal(voiced, want[0]), (name, n, step, numpy.flatnonzero(voiced != want[0])[:8])
            assert same(f64, want[1]), (name, n, step)
            assert same(t, want[2]), (name, n, step)


def mixed_wave(seconds: float, sr: int, seed: int = 0) -> numpy.ndarray:
    """A 220 Hz tone, noise, and a digitally silent stretch in the middle third, float32."""
    n = int(round(seconds * sr))
    rng = numpy.random.default_rng([seed, n, sr])
    x = 0.4 * numpy.sin(2 * numpy.pi * 220.0 * numpy.arange(n) / sr) + 0.05 * rng.normal(0, 1, n)
    x[n // 3:2 * n // 3] = 0
    x[2 * n // 3:] += 0.2 * rng.normal(0, 1, n - 2 * n // 3)
    return x.astype(numpy.float32)



def chain(model, x, sr, hop, step):
    """The chain `track` replaces: predict -> predict_voicing -> the mask on the host."""
    f0, conf, _ = model.predict(x, sr, hop)
    return voicing_reference(conf, f0, step)


def check_track(model, seconds, sr, step=5):
    x = mixed_wave(seconds, sr)
    hop = crepe.hop_length(step)
    want = chain(model, x, sr, hop, step)
    got = model.track(x, sr, hop, step)
    assert got[0].shape == want[0].shape, (got[0].shape, want[0].shape)
    assert numpy.array_equal(got[0], want[0]) and same(got[1], want[1]) and same(got[2], want[2])
    return x, hop, got


def analysis_case(fs: int, n: int = 40, seed: int = 0):
    """(wave float32, f0 [n] float64 with zeros and 80 .. 600 Hz, t [n] float64 at 5 ms)."""
    rng = numpy.random.default_rng([seed, fs, n])
    t = numpy.arange(n) * 5 / 1000.0
    x = mixed_wave(t[-1] + 0.02, fs, seed + 1)
    f0 = rng.uniform(80.0, 600.0, n)
    f0[rng.uniform(0, 1, n) < 0.3] = 0.0
    f0[0], f0[-1] = 0.0, 600.0
    return x, f0, t


class DeviceArrays(object):
    """Host arrays on the card of `ctx` (freed with the object): `address[i]` of array i."""

    def __init__(self, ctx, *arrays):
        self.ctx, self.address = ctx, []
        for a in arrays:
            words = numpy.ascontiguousarray(a).view(numpy.float32)
            self.address.append(ctx.dev_alloc(max(words.size, 1)))
            ctx.dev_upload(self.address[-1], words)

    def close(self):
        for p in self.address:
            self.ctx.dev_free(p)
        self.address = []


KEYS = ('sp64', 'mc', 'ap64', 'coded_ap')


def check_run_device(ctx, fs: int):
    """`Analyzer.run_device` against `Analyzer.run`, then the three refusals on NaN-prefilled outputs and a valid call after them."""
    from realtime_yukarin_amd import _lib, world_analysis
    x, f0, t = analysis_case(fs)
    a = world_analysis.Analyzer(fs, order=8, seed=5, ctx=ctx)
    want = a.run(x.astype(numpy.float64), f0, t, want=KEYS)
    dev = DeviceArrays(ctx, x, f0, t)
    got = a.run_device(dev.address[0], x.size, dev.address[1], dev.address[2], f0.size, want=KEYS)
    for k, g, w in zip(KEYS, got, want):
        assert same(g, w), k
    # the float32 rows left on the card
    rows_w = a.run(x.astype(numpy.float64), f0, t, want=('sp', 'ap'), device_rows=True)
    rows_g = a.run_device(dev.address[0], x.size, dev.address[1], dev.address[2], f0.size, want=('sp', 'ap'), device_rows=True)
    for g, w in zip(rows_g, rows_w):
        hg, hw = numpy.empty((f0.size, 513), numpy.float32), numpy.empty((f0.size, 513), numpy.float32)
        ctx.dev_download(g.address, hg)
        ctx.dev_download(w.address, hw)
        assert same(hg, hw)
    assert same(hg, want[2].astype(numpy.float32))
    # refusals: nothing is written, on the host or on the card
    lib, h = a._get()
    for bad_f0, bad_t, word in ((numpy.nan, None, b'f0['), (fs / 2, None, b'f0['), (None, -2.0, b't[')):
        f0b, tb = f0.copy(), t.copy()
        if bad_f0 is not None:
            f0b[17] = bad_f0
        if bad_t is not None:
            tb[17] = bad_t
        devb = DeviceArrays(ctx, f0b, tb, numpy.full((f0.size, 513), numpy.nan, numpy.float32))
        outs = [numpy.full(s, numpy.nan) for s in ((f0.size, 513), (f0.size, 9), (f0.size, 513), (f0.size, a.bands()))]
        rc = lib.dll.ry_analysis_extract_dev(h, _lib._fptr(dev.address[0]), x.size, _DP(devb.address[0]), _DP(devb.address[1]), f0.size, 0.85,
                                             _dp(outs[0]), _lib._fptr(devb.address[2]), _dp(outs[1]), _dp(outs[2]), None, _dp(outs[3]))
        assert rc == -1 and word in lib.dll.ry_last_error(), (rc, lib.dll.ry_last_error())          # RY_EINVAL
        rows = numpy.zeros((f0.size, 513), numpy.float32)
        ctx.dev_download(devb.address[2], rows)
        assert all(numpy.isnan(o).all() for o in outs) and numpy.isnan(rows).all()
        devb.close()
    again = a.run_device(dev.address[0], x.size, dev.address[1], dev.address[2], f0.size, want=KEYS)
    for k, g, w in zip(KEYS, again, want):
        assert same(g, w), k
    dev.close()
    a.close()


def _DP(address):
    import ctypes
    return ctypes.cast(ctypes.c_void_p(address), ctypes.POINTER(ctypes.c_double))


def _dp(a):
    import ctypes
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
