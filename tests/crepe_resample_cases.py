"""Shared by tests/test_crepe_resample_cpu.py (emulator) and tests/test_crepe_resample_gpu.py (MI355X): the case lists of the device resampler
(`ry_crepe_set_resampler` / `ry_crepe_resample` / `ry_crepe_predict_sr`), its inputs with the host function's result computed once, and the
checks both files run.  The bar is `array_equal` with `crepe.resample`: one device thread per output adds the host function's terms in
its order in float64, each operation rounded on its own, from the tables the host function itself uses."""
import ctypes
import functools

import numpy

import crepe_ref
from realtime_yukarin_amd import _lib, crepe

HOP = 80
# 8000: up-sampling (table step 512); 22050 / 44100: the time register rounds at almost every output; 24000 / 48000: it is exact
RATES = (8000, 22050, 24000, 44100, 48000)
# input lengths at 24 kHz -> 1, 2, 3, 26, 63, 64, 65, 255, 256, 257, 466 outputs: a single output, signals shorter than the filter's half width (both
# sides cut by the signal's ends), one output either side of a wave and of the 256-thread block, a ragged last block
LENGTHS_24K = (2, 3, 5, 40, 95, 96, 98, 383, 384, 386, 700)
OUTPUTS_24K = (1, 2, 3, 26, 63, 64, 65, 255, 256, 257, 466)
# every rate: the shortest input that gives an output, and a few short ones
SHORT = {8000: (1, 2, 129), 22050: (2, 3, 354), 24000: (2, 3, 386), 44100: (3, 6, 709), 48000: (3, 6, 772)}
DP = ctypes.POINTER(ctypes.c_double)


@functools.lru_cache(maxsize=None)
def case(sr, n):
    """(x float32 [n] seeded normal noise, crepe.resample(x, sr)), computed once and read-only"""
    x = numpy.random.default_rng(sr + n).normal(0, 1, n).astype(numpy.float32)
    y = crepe.resample(x, sr)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def new_model(ctx, m=1, seed=3):
    P = crepe.synthetic_params(m, seed)
    return crepe.CrepeModel(m, P, ctx=ctx), P


def same(a, b):
    return all(numpy.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def check_exact(model, sr, n):
    x, want = case(sr, n)
    got = model.resample(x, sr)
    assert got.dtype == numpy.float32 and got.shape == want.shape == (crepe.resampled_length(n, sr),), (sr, n, got.shape, want.shape)
    assert numpy.array_equal(got, want), (sr, n, int((got != want).sum()), float(numpy.abs(got - want).max()))


def check_restatement(model, sr):
    """the first, middle and last 40 outputs of the 1 s call against the per-sample restatement (the bar of
    test_crepe_cpu.py::test_resampler_matches_sinc_sum for the host function)"""
    x, _ = case(sr, sr)
    y = model.resample(x, sr)
    at = list(range(0, 40)) + list(range(len(y) // 2 - 20, len(y) // 2 + 20)) + list(range(len(y) - 40, len(y)))
    ref = crepe_ref.sinc_resample(x, sr, 16000, at=at)
    err = float(numpy.abs(y[at] - ref).max() / numpy.abs(ref).max())
    print('resample %d Hz: max |y - sinc sum| / max |ref| = %.3g' % (sr, err))
    assert err < 1e-5, (sr, err)


def check_growth_and_mixing(ctx):
    """44.1 kHz: 40 samples, 1 s (the time register grows), 40 samples again; then 24 kHz, 44.1 kHz, 24 kHz on one handle"""
    model, _ = new_model(ctx)
    fresh, _ = new_model(ctx)
    try:
        short, long_ = case(44100, 40)[0], case(44100, 44100)[0]
        a = model.resample(short, 44100)
        held = model._rs[44100]
        b = model.resample(long_, 44100)
        assert model._rs[44100] > held and model._rs[44100] >= len(b)
        c = model.resample(short, 44100)
        assert numpy.array_equal(a, c) and numpy.array_equal(a, fresh.resample(short, 44100)) and numpy.array_equal(a, case(44100, 40)[1])
        assert numpy.array_equal(b, case(44100, 44100)[1])
        x24 = case(24000, 700)[0]
        first = model.resample(x24, 24000)
        mid = model.resample(case(44100, 709)[0], 44100)
        again = model.resample(x24, 24000)
        assert numpy.array_equal(first, again) and numpy.array_equal(first, fresh.resample(x24, 24000)) and numpy.array_equal(first, case(24000, 700)[1])
        assert numpy.array_equal(mid, case(44100, 709)[1])
        assert set(model._rs) == {44100, 24000}
    finally:
        model.close(); fresh.close()


def check_poison(ctx):
    model, _ = new_model(ctx)
    try:
        x = case(24000, 1776)[0]                                     # 1184 samples at 16 kHz: three uncentred frames
        clean_y = model.resample(x, 24000)
        clean = model.predict(x, 24000, HOP, center=False)
        model.poison()
        y = model.resample(x, 24000)
        assert numpy.isfinite(y).all() and numpy.array_equal(y, clean_y)
        model.poison()
        out = model.predict(x, 24000, HOP, center=False)
        assert all(numpy.isfinite(o).all() for o in out) and same(out, clean)
        model.poison()
        part = model.resample(x[:300], 24000)                       # a shorter call on the poisoned buffers
        assert numpy.array_equal(part, crepe.resample(x[:300], 24000))
    finally:
        model.close()


PREDICT_CASES = [(False, 1536, 1), (False, 1776, 3), (True, 60, 1), (True, 300, 3)]       # center, samples at 24 kHz, frames


def check_predict(model, center, n, frames):
    x, x16 = case(24000, n)
    want = model.predict16k(x16, HOP, center=center)
    got = model.predict(x, 24000, HOP, center=center)
    assert got[0].shape == (frames,) and got[2].shape == (frames, crepe.BINS)
    assert same(got, want), (center, n)
    assert same(model.predict(x, 24000, HOP, center=center, viterbi=False), model.predict16k(x16, HOP, center=center, viterbi=False))
    f0, conf, act = model.predict(x, 24000, HOP, center=center, activation=False)
    assert act is None and numpy.array_equal(f0, want[0]) and numpy.array_equal(conf, want[1])


def check_predict_16k_is_predict16k(model):
    x = case(16000, 1184)[0]
    assert same(model.predict(x, 16000, HOP, center=False), model.predict16k(x, HOP, center=False))
    assert numpy.array_equal(model.resample(x, 16000), x)


def check_on_device(model, ctx):
    """on_device = 1: audio at 24 kHz and every output in device buffers, the host calls' bits"""
    x, x16 = case(24000, 1776)
    frames = 3
    f0, conf, act = model.predict(x, 24000, HOP, center=False)
    lib, h = model._get()
    bufs = [ctx.dev_alloc(n) for n in (x.size, x16.size, frames, frames, frames * crepe.BINS)]
    try:
        ctx.dev_upload(bufs[0], numpy.ascontiguousarray(x))
        lib.check(lib.dll.ry_crepe_resample(h, _lib._fptr(bufs[0]), x.size, 24000, _lib._fptr(bufs[1]), 1))
        lib.check(lib.dll.ry_crepe_predict_sr(h, _lib._fptr(bufs[0]), x.size, 24000, HOP, 0, 1, _lib._fptr(bufs[2]), _lib._fptr(bufs[3]),
                                              _lib._fptr(bufs[4]), 1))
        ctx.sync()
        got = [numpy.empty(s, numpy.float32) for s in (x16.size, frames, frames, (frames, crepe.BINS))]
        for p, a in zip(bufs[1:], got):
            ctx.dev_download(p, a)
        ctx.sync()
    finally:
        for p in bufs:
            ctx.dev_free(p)
    assert numpy.array_equal(got[0], x16)
    assert numpy.array_equal(got[1], f0) and numpy.array_equal(got[2], conf) and numpy.array_equal(got[3], act)


def check_shim(monkeypatch, tmp_path, P, m, model=None):
    """shim.predict at 24 kHz: the device resampler by default, `crepe.resample` under RY_CREPE_RESAMPLE=host, the same bits.  `model`: a
    CrepeModel over another build of the library (the emulator) to seat in the shim; None: the shim builds its own from RY_CREPE_MODEL."""
    from realtime_yukarin_amd.compat import crepe as shim
    path = tmp_path / ('crepe_m%d.npz' % m)
    crepe.save_weights(path, P)
    monkeypatch.setenv('RY_CREPE_MODEL', str(path))
    monkeypatch.setattr(shim, '_weights', {})
    monkeypatch.setattr(shim, '_models', {} if model is None else {m: model})
    calls = []
    host = crepe.resample

    def spy(*a, **k):
        calls.append(a[1])
        return host(*a, **k)
    monkeypatch.setattr(crepe, 'resample', spy)
    x = case(24000, 300)[0]                                       # 200 samples at 16 kHz: three centred frames at 5 ms
    stereo = numpy.stack([x, 0.5 * x], axis=1).astype(numpy.float64)
    try:
        monkeypatch.delenv('RY_CREPE_RESAMPLE', raising=False)
        dev = shim.predict(x, 24000, viterbi=True, model_capacity=m, step_size=5, verbose=0)
        dev_st = shim.predict(stereo, 24000, viterbi=True, model_capacity=m, step_size=5, verbose=0)
        assert calls == [], 'the default path resampled on the host'
        monkeypatch.setenv('RY_CREPE_RESAMPLE', 'host')
        ref = shim.predict(x, 24000, viterbi=True, model_capacity=m, step_size=5, verbose=0)
        ref_st = shim.predict(stereo, 24000, viterbi=True, model_capacity=m, step_size=5, verbose=0)
        assert calls == [24000, 24000]
        assert dev[1].dtype == numpy.float64 and len(dev[0]) == 3
        assert same(dev, ref) and same(dev_st, ref_st)
        monkeypatch.setenv('RY_CREPE_RESAMPLE', 'cpu')
        try:
            shim.predict(x, 24000, viterbi=True, model_capacity=m, step_size=5, verbose=0)
            raise AssertionError('an unknown RY_CREPE_RESAMPLE value was accepted')
        except RuntimeError as e:
            assert 'RY_CREPE_RESAMPLE' in str(e)
    finally:
        if model is None and m in shim._models:
            shim._models[m].close()


def check_refusals(ctx):
    """each refusal returns an error code and a message and launches nothing: the output buffers keep their sentinel"""
    model, _ = new_model(ctx)
    lib, h = model._get()
    dll = lib.dll
    try:
        x = numpy.ascontiguousarray(case(24000, 1776)[0])
        y = numpy.full(2000, 7.0, numpy.float32)
        f0, conf = numpy.full(8, 7.0, numpy.float32), numpy.full(8, 7.0, numpy.float32)

        def refused(rc, word):
            msg = dll.ry_last_error()
            assert rc < 0 and word in msg, (rc, msg)
            assert (y == 7.0).all() and (f0 == 7.0).all() and (conf == 7.0).all(), 'a refused call wrote its output'

        def resample(n, sr, handle=h):
            return dll.ry_crepe_resample(handle, _lib._fptr(x), n, sr, _lib._fptr(y), 0)

        def predict(n, sr, center, handle=h):
            return dll.ry_crepe_predict_sr(handle, _lib._fptr(x), n, sr, HOP, center, 1, _lib._fptr(f0), _lib._fptr(conf), None, 0)
        # a rate without tables
        refused(resample(1776, 24000), b'no resampler tables')
        refused(predict(1776, 24000, 1), b'no resampler tables')
        refused(resample(1776, 0), b'sample rate')
        refused(predict(1776, -5, 1), b'sample rate')
        # tables whose time register holds 100 outputs: 150 inputs fill it, 153 need 102
        win, num_table, step = crepe.resampler_tables(24000)
        tr = crepe.time_register(24000, 100)
        assert dll.ry_crepe_set_resampler(h, 24000, win.ctypes.data_as(DP), win.size, num_table, step, tr.ctypes.data_as(DP), tr.size) == 0
        refused(resample(153, 24000), b'time table')
        refused(predict(153, 24000, 1), b'time table')
        assert resample(150, 24000) == 0 and numpy.array_equal(y[:100], crepe.resample(x[:150], 24000)) and (y[100:] == 7.0).all()
        y[:] = 7.0
        # an empty output: 1 sample at 24 kHz, 2 samples at 48 kHz
        refused(resample(1, 24000), b'no sample at 16 kHz')
        refused(predict(1, 24000, 1), b'no sample at 16 kHz')
        refused(resample(0, 24000), b'samples')
        win48, nt48, step48 = crepe.resampler_tables(48000)
        tr48 = crepe.time_register(48000, 10)
        assert dll.ry_crepe_set_resampler(h, 48000, win48.ctypes.data_as(DP), win48.size, nt48, step48, tr48.ctypes.data_as(DP), tr48.size) == 0
        refused(resample(2, 48000), b'no sample at 16 kHz')
        refused(predict(2, 48000, 1), b'no sample at 16 kHz')
        # center = 0 with fewer than 1024 resampled samples (1535 samples at 24 kHz give 1023)
        tr = crepe.time_register(24000, 2000)
        assert dll.ry_crepe_set_resampler(h, 24000, None, 0, 0, 0, tr.ctypes.data_as(DP), tr.size) == 0
        refused(predict(1535, 24000, 0), b'1024')
        assert predict(1536, 24000, 0) == 0 and (f0[0] != 7.0 and conf[0] != 7.0) and (f0[1:] == 7.0).all()
        f0[:] = 7.0; conf[:] = 7.0
        # a null handle, null tables, tables that are no time register
        refused(resample(1776, 24000, None), b'null crepe handle')
        refused(predict(1776, 24000, 1, None), b'null crepe handle')
        refused(dll.ry_crepe_set_resampler(None, 24000, win.ctypes.data_as(DP), win.size, num_table, step, tr.ctypes.data_as(DP), tr.size), b'null crepe handle')
        refused(dll.ry_crepe_set_resampler(h, 44100, None, 0, 0, 0, tr.ctypes.data_as(DP), tr.size), b'filter table')
        refused(dll.ry_crepe_set_resampler(h, 44100, win.ctypes.data_as(DP), win.size, num_table, 0, tr.ctypes.data_as(DP), tr.size), b'step')
        bad = tr.copy(); bad[50] = bad[49] - 1.0
        refused(dll.ry_crepe_set_resampler(h, 24000, None, 0, 0, 0, bad.ctypes.data_as(DP), bad.size), b'time register')
        # a register that runs past the signal: int(tr[n_out - 1]) must be an input sample
        fast = numpy.ascontiguousarray(tr * 2.0)
        assert dll.ry_crepe_set_resampler(h, 24000, None, 0, 0, 0, fast.ctypes.data_as(DP), fast.size) == 0
        refused(resample(1776, 24000), b'input sample')
        # the Python layer
        for bad_sr in (0, -1, 22050.5):
            try:
                model.resample(x, bad_sr)
                raise AssertionError('sample rate %r accepted' % (bad_sr,))
            except ValueError:
                pass
        for call in (lambda: model.resample(x[:1], 24000), lambda: model.predict(x[:1], 24000, HOP), lambda: model.predict(x[:1535], 24000, HOP, center=False)):
            try:
                call()
                raise AssertionError('accepted')
            except ValueError:
                pass
    finally:
        model.close()
