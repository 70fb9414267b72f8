"""The D4C kernel (realtime_yukarin_amd/csrc/d4c_kernels.h) on the host-side SIMT emulator against the numpy restatement (tests/world_d4c_ref.py):
short inputs (<= 40 frames), the refusals of the C ABI, the Python surface and the opt-in `extract` binding on a restated `AcousticFeature`.

Bars (profiles/r10/d4c_tolerance.txt, written by scripts/d4c_tolerance.py): the integers of a frame and on / off exact; a0, the coarse dB values and
20 log10 ap: <= 4 x the same figure of the float64 restatement against the longdouble one, worst over the case set; coded_ap against
code_aperiodicity(ref ap): the coarse bar; off rows, float32 rows and every bit identity: exact.  The frames are vetted by tests/test_world_d4c_ref.py."""
import ctypes

import numpy
import pytest

import world_analysis_cases as C
import world_d4c_cases as D
import world_d4c_ref as R
from realtime_yukarin_amd import _lib, world_analysis, world_synth

BAR_A0, BAR_COARSE, BAR_AP = D.bars()
_DP = ctypes.POINTER(ctypes.c_double)


def download(ctx, rows):
    out = numpy.empty((rows.frames, 513), numpy.float32)
    if rows.frames:
        ctx.dev_download(rows.address, out)
    return out


def check(ctx, wk, tk, n, fs, seed=D.SEED):
    """One case against the restatement: integers and on / off exact, a0 / coarse / ap / coded_ap inside their bars, off rows exact, float32 rows =
    float32(float64 rows), two runs the same bits, recording off the same bits."""
    x, f0, t = C.case(wk, tk, n, fs)
    a = world_analysis.Analyzer(fs, fft_size=1024, seed=seed, ctx=ctx)
    a.record_integers()
    rows, ap, coded = a.run(x, f0, t, want=('ap', 'ap64', 'coded_ap'), device_rows=True)
    ints, on, a0, coarse = a.d4c_record()
    want, want_a0, want_on, want_coarse = R.d4c(x, f0, t, fs, seed=seed, details=True)
    assert numpy.array_equal(ints, R.integers(f0, t, fs))
    assert numpy.array_equal(on, want_on)
    assert ap.shape == want.shape and coded.shape == (n, R.bands(fs)) and ap.dtype == coded.dtype == numpy.float64
    assert numpy.isfinite(ap).all() and numpy.isfinite(coded).all() and (ap > 0).all() and (ap <= 1).all()
    e_a0 = float(numpy.abs(a0 - want_a0).max())
    e_co = float(numpy.abs(coarse[on] - want_coarse[on]).max()) if on.any() else 0.0
    e_ap = float(numpy.abs(20 * numpy.log10(ap) - 20 * numpy.log10(want)).max())
    e_cd = float(numpy.abs(coded - R.code_aperiodicity(want, fs)).max())
    print('%-6s %-12s fs=%d frames=%3d on=%3d: a0 %.3g (bar %.3g)  coarse %.3g (bar %.3g)  ap %.3g (bar %.3g)  coded_ap %.3g (bar %.3g)'
          % (wk, tk, fs, n, on.sum(), e_a0, BAR_A0, e_co, BAR_COARSE, e_ap, BAR_AP, e_cd, BAR_COARSE))
    assert e_a0 <= BAR_A0, e_a0
    assert e_co <= BAR_COARSE, e_co
    assert e_ap <= BAR_AP, e_ap
    assert e_cd <= BAR_COARSE, e_cd
    assert numpy.array_equal(ap[~on], want[~on])                                   # off rows: 1 - 1e-12, bit for bit
    assert numpy.array_equal(download(ctx, rows), ap.astype(numpy.float32))
    again = a.run(x, f0, t, want=('ap', 'coded_ap'))
    assert numpy.array_equal(again[0], ap) and numpy.array_equal(again[1], coded)
    a.record_integers(False)                                       # the product path: nothing recorded, the same bits
    plain = a.run(x, f0, t, want=('ap', 'coded_ap'))
    assert a.d4c_record()[0].shape == (0, 8)
    assert numpy.array_equal(plain[0], ap) and numpy.array_equal(plain[1], coded)
    a.close()


@pytest.mark.parametrize('n', C.LENGTHS_EMU)
@pytest.mark.parametrize('tk', C.TRACKS)
@pytest.mark.parametrize('wk', C.WAVES)
@pytest.mark.parametrize('fs', C.RATES)
def test_kernel_matches_the_restatement(emu_ctx, fs, wk, tk, n):
    check(emu_ctx, wk, tk, n, fs)


def test_rows_do_not_depend_on_the_batch(emu_ctx):
    fs, n = 24000, 40
    x, f0, t = C.case('glide', 'alternating', n, fs)
    a = world_analysis.Analyzer(fs, seed=2, ctx=emu_ctx)
    ap, coded = a.run(x, f0, t, want=('ap', 'coded_ap'))
    rng = numpy.random.default_rng(3)
    for pick in (rng.permutation(n), rng.permutation(n)[:17], numpy.array([n - 2])):
        ap2, coded2 = a.run(x, f0[pick], t[pick], want=('ap', 'coded_ap'))
        assert numpy.array_equal(ap2, ap[pick]) and numpy.array_equal(coded2, coded[pick])
    a.close()


def test_seeds_and_silence(emu_ctx):
    fs = 16000
    x, f0, t = C.case('zeros', 'glide', 23, fs)
    a, b = world_analysis.Analyzer(fs, seed=1, ctx=emu_ctx), world_analysis.Analyzer(fs, seed=2, ctx=emu_ctx)
    a.record_integers(); b.record_integers()
    za, zb = a.run(x, f0, t, want=('ap', 'coded_ap')), b.run(x, f0, t, want=('ap', 'coded_ap'))
    assert all(numpy.isfinite(v).all() for v in za + zb)
    a0a, a0b = a.d4c_record()[2], b.d4c_record()[2]
    assert numpy.isfinite(a0a).all() and numpy.isfinite(a0b).all() and not numpy.array_equal(a0a, a0b)        # the noise is live
    a.close(); b.close()


def test_poisoned_buffers(emu_ctx):
    fs = 24000
    x, f0, t = C.case('glide', 'glide', 23, fs)
    a = world_analysis.Analyzer(fs, seed=4, ctx=emu_ctx)
    want = ('sp', 'mc', 'ap', 'coded_ap')
    clean = a.run(x, f0, t, want=want)
    a.record_integers()
    a.run(*C.case('noise', 'alternating', 40, fs), want=want)      # grows every buffer beyond the 23 frames of the next call
    a.record_integers(False)
    a.poison()
    got = a.run(x, f0, t, want=want)
    assert all(numpy.isfinite(g).all() and numpy.array_equal(g, c) for g, c in zip(got, clean))
    a.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_one_call_for_everything_equals_the_separate_calls(emu_ctx, fs):
    x, f0, t = C.case('glide', 'alternating', 23, fs)
    a = world_analysis.Analyzer(fs, seed=7, ctx=emu_ctx)
    sp, mc, ap, coded = a.run(x, f0, t, want=('sp', 'mc', 'ap', 'coded_ap'))
    sp1, mc1 = a.run(x, f0, t)
    ap1, coded1 = a.run(x, f0, t, want=('ap', 'coded_ap'))
    assert numpy.array_equal(sp, sp1) and numpy.array_equal(mc, mc1) and numpy.array_equal(ap, ap1) and numpy.array_equal(coded, coded1)
    assert numpy.array_equal(a.d4c(x, f0, t), ap)
    rows_sp, rows_ap = a.run(x, f0, t, want=('sp', 'ap'), device_rows=True)
    assert numpy.array_equal(download(emu_ctx, rows_sp), sp.astype(numpy.float32)) and numpy.array_equal(download(emu_ctx, rows_ap), ap.astype(numpy.float32))
    a.close()


def test_chain_into_the_synthesizer_on_the_device(emu_ctx):
    fs, n = 16000, 23
    x, f0, t = C.case('glide', 'alternating', n, fs)
    a = world_analysis.Analyzer(fs, seed=6, ctx=emu_ctx)
    rows_sp, rows_ap = a.run(x, f0, t, want=('sp', 'ap'), device_rows=True)
    assert isinstance(rows_ap, world_synth.DeviceRows) and rows_ap.frames == n
    s = world_synth.Synthesizer(fs, 5.0, seed=6, ctx=emu_ctx)
    dev = s.synthesize(f0, rows_sp, rows_ap)
    host = s.synthesize(f0, download(emu_ctx, rows_sp), download(emu_ctx, rows_ap))
    assert len(dev) == s.length(n) and numpy.isfinite(dev).all() and dev.any() and numpy.array_equal(dev, host)
    s.close(); a.close()


def test_threshold(emu_ctx):
    fs = 16000
    x, f0, t = C.case('glide', 'glide', 23, fs)
    a = world_analysis.Analyzer(fs, seed=D.SEED, ctx=emu_ctx)
    a.record_integers()
    a.d4c(x, f0, t)
    a0 = a.d4c_record()[2]
    th = float(numpy.sort(a0)[len(a0) // 2]) + 1e-4                # between two frames' ratios: about half of the frames are off
    assert numpy.abs(a0 - th).min() >= D.MARGIN
    ap = a.d4c(x, f0, t, threshold=th)
    assert numpy.array_equal(a.d4c_record()[1], a0 > th) and numpy.array_equal((ap == 1.0 - 1e-12).all(axis=1), ~(a0 > th))
    assert numpy.abs(20 * numpy.log10(ap) - 20 * numpy.log10(R.d4c(x, f0, t, fs, threshold=th, seed=D.SEED))).max() <= BAR_AP
    a.close()


def test_abi_refusals(emu_ctx):
    lib, d = emu_ctx.lib, emu_ctx.lib.dll
    h = ctypes.c_void_p()
    lib.check(d.ry_analysis_create(emu_ctx.handle, 16000, 1024, 8, 0.41, -0.15, 71.0, 0, ctypes.byref(h)))
    assert d.ry_analysis_d4c_bands(h) == 1
    x, f0, t = C.case('glide', 'glide', 4, 16000)
    ap, coded = numpy.full((4, 513), numpy.nan), numpy.full((4, 1), numpy.nan)
    null = ctypes.cast(ctypes.c_void_p(0), _DP)
    px, pf, pt = x.ctypes.data_as(_DP), f0.ctypes.data_as(_DP), t.ctypes.data_as(_DP)

    def run(x_, xl, f0_, t_, n, th=0.85):
        return d.ry_analysis_d4c(h, x_, xl, f0_, t_, n, th, ap.ctypes.data_as(_DP), _lib._fptr(None), coded.ctypes.data_as(_DP))
    assert run(px, x.size, pf, pt, -1) == -1 and b'frames' in d.ry_last_error()
    assert run(null, x.size, pf, pt, 4) == -1 and b'null wave' in d.ry_last_error()
    assert run(px, x.size, null, pt, 4) == -1 and run(px, x.size, pf, null, 4) == -1 and run(px, -1, pf, pt, 4) == -1
    assert run(px, x.size, pf, pt, 4, numpy.nan) == -1 and b'threshold' in d.ry_last_error()
    for bad in (numpy.nan, numpy.inf, 8000.0):
        g = f0.copy(); g[2] = bad
        assert run(px, x.size, g.ctypes.data_as(_DP), pt, 4) == -1 and b'f0[2]' in d.ry_last_error()
    g = t.copy(); g[1] = -1.5
    assert run(px, x.size, pf, g.ctypes.data_as(_DP), 4) == -1 and b't[1]' in d.ry_last_error()
    assert run(px, x.size, pf, pt, 0) == 0 and run(null, 0, pf, pt, 4) == 0                       # succeed, write nothing
    assert numpy.isnan(ap).all() and numpy.isnan(coded).all()
    assert d.ry_analysis_d4c(h, px, x.size, pf, pt, 4, 0.85, null, _lib._fptr(None), null) == 0    # every output may be null
    assert run(px, x.size, pf, pt, 4) == 0 and numpy.isfinite(ap).all() and numpy.isfinite(coded).all()
    assert d.ry_analysis_d4c(None, px, x.size, pf, pt, 4, 0.85, null, _lib._fptr(None), null) == -4 and d.ry_analysis_d4c_bands(None) == -4
    n = ctypes.c_int(-1)
    assert d.ry_analysis_debug_d4c(h, None, None, 0, ctypes.byref(n)) == 0 and n.value == 0       # nothing was recorded
    d.ry_analysis_destroy(h)
    # a rate whose D4C sizes are not the built ones: CheapTrick runs, D4C is refused with the reason
    lib.check(d.ry_analysis_create(emu_ctx.handle, 12000, 1024, 8, 0.41, -0.15, 71.0, 0, ctypes.byref(h)))
    sp = numpy.empty((4, 513))
    assert d.ry_analysis_run(h, px, x.size, pf, pt, 4, sp.ctypes.data_as(_DP), _lib._fptr(None), null) == 0
    assert d.ry_analysis_d4c_bands(h) == -1 and b'12000 Hz' in d.ry_last_error()
    assert run(px, x.size, pf, pt, 4) == -1 and b'12000 Hz' in d.ry_last_error()
    assert d.ry_analysis_extract(h, px, x.size, pf, pt, 4, 0.85, null, _lib._fptr(None), null, null, _lib._fptr(None), null) == -1
    d.ry_analysis_destroy(h)


def test_python_surface(emu_ctx, monkeypatch):
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    fs = 24000
    x, f0, t = C.case('glide', 'glide', 5, fs)
    a = world_analysis.Analyzer(fs, ctx=emu_ctx)
    assert a.bands() == 3
    ap, coded = a.run(x, f0, t, want=('ap', 'coded_ap'))
    assert numpy.array_equal(world_analysis.d4c(x, f0, t, fs), ap)                              # pyworld's argument order, seed 0
    assert numpy.array_equal(world_analysis.d4c(x, f0, t, fs, 0.85, 1024), ap)
    # the host's 20 log10 of the same ap values against the device's: two log10 implementations, each within a few ulp of values <= 60 (ulp 7e-15)
    assert numpy.abs(world_analysis.code_aperiodicity(ap, fs) - coded).max() <= 1e-13
    got = world_analysis.device_aperiodicity(x, f0, t, fs, 1024)
    assert numpy.array_equal(got[0], ap) and numpy.array_equal(got[1], coded)
    e, c = a.run(x, f0[:0], t[:0], want=('ap', 'coded_ap'))
    assert e.shape == (0, 513) and c.shape == (0, 3)
    with pytest.raises(ValueError, match='empty wave'):
        a.run(x[:0], f0, t, want=('ap',))
    with pytest.raises(ValueError, match='want'):
        a.run(x, f0, t, want=('ap', 'bap'))
    with pytest.raises(_lib.Ry355Error, match='fft_size'):
        world_analysis.d4c(x, f0, t, fs, fft_size=2048)
    with pytest.raises(_lib.Ry355Error):
        world_analysis.d4c(x, f0, t, 48000)                                                     # fft_size 2048 rows: not built
    with pytest.raises(_lib.Ry355Error, match='12000 Hz'):
        world_analysis.Analyzer(12000, fft_size=1024, ctx=emu_ctx).d4c(x, f0, t)
    with pytest.raises(ValueError):
        world_analysis.code_aperiodicity(ap, 22050)
    with pytest.raises(ValueError):
        world_analysis.code_aperiodicity(ap[:, :100], fs)
    a.close()


# ---- the reference's class, restated as in tests/test_world_analysis_cpu.py ----
class _Wave(object):
    def __init__(self, wave, sampling_rate):
        self.wave, self.sampling_rate = wave, sampling_rate


def _feature_class():
    from realtime_yukarin_amd.compat.yukarin.acoustic_feature import AcousticFeature as Base

    class AcousticFeature(Base):
        @classmethod
        def extract_f0(cls, x, fs, frame_period, f0_floor, f0_ceil):              # a fake tracker (the CREPE wrapper binds here)
            n = int(len(x) / fs * 1000 / frame_period) + 1
            return C.f0_track('alternating', n), numpy.arange(n) * frame_period / 1000
    return AcousticFeature


@pytest.mark.parametrize('fs', C.RATES)
def test_opt_in_extract_needs_no_pyworld(emu_ctx, monkeypatch, fs):
    import sys
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setitem(sys.modules, 'pyworld', None)                              # importing it fails
    monkeypatch.setattr(world_analysis, 'aperiodicity', world_analysis.device_aperiodicity)      # the opt-in line of INTEGRATION.md section 11
    AF = _feature_class()
    monkeypatch.setattr(AF, 'extract', classmethod(world_analysis.extract))
    x = C.wave('glide', 30, fs).astype(numpy.float32)
    bands = R.bands(fs)
    for dtype in (numpy.float32, numpy.float64):
        f = AF.extract(_Wave(x, fs), frame_period=5, f0_floor=71.0, f0_ceil=800.0, fft_length=1024, order=8, alpha=0.41, dtype=dtype)
        n = len(f.f0)
        for k, s in dict(f0=(n, 1), sp=(n, 513), ap=(n, 513), coded_ap=(n, bands), mc=(n, 9), voiced=(n, 1)).items():
            v = getattr(f, k)
            assert v.shape == s and v.dtype == (numpy.bool_ if k == 'voiced' else dtype), k
    f0, t = AF.extract_f0(x, fs, 5, 71.0, 800.0)
    want = R.d4c(x.astype(numpy.float64), f0, t, fs, seed=0)
    assert numpy.abs(20 * numpy.log10(f.ap) - 20 * numpy.log10(want)).max() <= BAR_AP
    assert (f.ap[1::2] == 1.0 - 1e-12).all() and (f.ap[0:20:2] < 1.0 - 1e-12).any()
