"""D4C on the MI355X (realtime_yukarin_amd/world_analysis.py, kernel: csrc/d4c_kernels.h) against the numpy float64 restatement (tests/world_d4c_ref.py).

Bars.  The integers of a frame, on / off, off rows, the float32 rows against float32(float64 rows) and every bit identity: exact.  a0 (the Love-Train
ratio), the coarse dB values and 20 log10 ap: <= 4 x the same figure of the float64 restatement against the restatement in longdouble with its own
transform, worst over the case set -- measured by scripts/d4c_tolerance.py, read from profiles/r10/d4c_tolerance.txt (lines 1 to 3); coded_ap against
code_aperiodicity(ref ap): the coarse bar.  The frames are vetted by tests/test_world_d4c_ref.py (integer decisions and a0 clear of their flips).
The output of a run of this file, with every printed figure against its bar, is kept as profiles/r10/d4c_pytest_gpu.txt."""
import numpy
import pytest

import world_analysis_cases as C
import world_d4c_cases as D
import world_d4c_ref as R
from realtime_yukarin_amd import _lib, world_analysis, world_synth

pytestmark = pytest.mark.gpu
BAR_A0, BAR_COARSE, BAR_AP = D.bars()


def download(ctx, rows):
    out = numpy.empty((rows.frames, 513), numpy.float32)
    ctx.dev_download(rows.address, out)
    return out


def check(ctx, wk, tk, n, fs, seed=D.SEED):
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
    assert numpy.array_equal(download(ctx, rows), ap.astype(numpy.float32))        # float32(float64 row), bit for bit
    again = a.run(x, f0, t, want=('ap', 'coded_ap'))
    assert numpy.array_equal(again[0], ap) and numpy.array_equal(again[1], coded)  # two runs: the same bits
    a.record_integers(False)                                       # the product path: nothing recorded, the same bits
    plain = a.run(x, f0, t, want=('ap', 'coded_ap'))
    assert a.d4c_record()[0].shape == (0, 8)
    assert numpy.array_equal(plain[0], ap) and numpy.array_equal(plain[1], coded)
    a.close()


@pytest.mark.parametrize('n', C.LENGTHS_GPU)
@pytest.mark.parametrize('tk', C.TRACKS)
@pytest.mark.parametrize('wk', C.WAVES)
@pytest.mark.parametrize('fs', C.RATES)
def test_cases(gpu_ctx, fs, wk, tk, n):
    check(gpu_ctx, wk, tk, n, fs)


@pytest.mark.parametrize('fs', C.RATES)
def test_rows_do_not_depend_on_the_batch(gpu_ctx, fs):
    n = 400
    x, f0, t = C.case('glide', 'alternating', n, fs)
    a = world_analysis.Analyzer(fs, seed=2, ctx=gpu_ctx)
    ap, coded = a.run(x, f0, t, want=('ap', 'coded_ap'))
    rng = numpy.random.default_rng(3)
    for pick in (rng.permutation(n), rng.permutation(n)[:57], numpy.array([n - 2]), numpy.arange(0, n, 3)):
        ap2, coded2 = a.run(x, f0[pick], t[pick], want=('ap', 'coded_ap'))
        assert numpy.array_equal(ap2, ap[pick]) and numpy.array_equal(coded2, coded[pick])
    a.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_seeds_and_silence(gpu_ctx, fs):
    """All-zero wave: everything finite, and two seeds give different Love-Train ratios (the noise is live); one seed twice: the same bits."""
    n = 201
    x, f0, t = C.case('zeros', 'glide', n, fs)
    a, b = world_analysis.Analyzer(fs, seed=1, ctx=gpu_ctx), world_analysis.Analyzer(fs, seed=2, ctx=gpu_ctx)
    a.record_integers(); b.record_integers()
    za, zb = a.run(x, f0, t, want=('ap', 'coded_ap')), b.run(x, f0, t, want=('ap', 'coded_ap'))
    assert all(numpy.isfinite(v).all() for v in za + zb)
    a0a, a0b = a.d4c_record()[2], b.d4c_record()[2]
    assert numpy.isfinite(a0a).all() and numpy.isfinite(a0b).all() and not numpy.array_equal(a0a, a0b)
    c = world_analysis.Analyzer(fs, seed=1, ctx=gpu_ctx)
    c.record_integers()
    assert numpy.array_equal(c.run(x, f0, t, want=('ap',))[0], za[0]) and numpy.array_equal(c.d4c_record()[2], a0a)
    a.close(); b.close(); c.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_poisoned_buffers(gpu_ctx, fs):
    """After a 2000-frame call has grown every buffer they are filled with NaN bit patterns: a 201-frame call gives the bits of the clean run."""
    x, f0, t = C.case('glide', 'glide', 201, fs)
    a = world_analysis.Analyzer(fs, seed=4, ctx=gpu_ctx)
    want = ('sp', 'mc', 'ap', 'ap64', 'coded_ap')
    clean = a.run(x, f0, t, want=want, device_rows=True)
    clean32 = download(gpu_ctx, clean[0]), download(gpu_ctx, clean[2])
    a.record_integers()
    a.run(*C.case('noise', 'alternating', 2000, fs), want=('sp64', 'mc', 'ap64', 'coded_ap'))
    a.record_integers(False)
    a.poison()
    got = a.run(x, f0, t, want=want, device_rows=True)
    for i in (1, 3, 4):
        assert numpy.isfinite(got[i]).all() and numpy.array_equal(got[i], clean[i])
    assert numpy.array_equal(download(gpu_ctx, got[0]), clean32[0]) and numpy.array_equal(download(gpu_ctx, got[2]), clean32[1])
    a.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_one_call_for_everything_equals_the_separate_calls(gpu_ctx, fs):
    x, f0, t = C.case('glide', 'alternating', 201, fs)
    a = world_analysis.Analyzer(fs, seed=7, ctx=gpu_ctx)
    sp, mc, ap, coded = a.run(x, f0, t, want=('sp', 'mc', 'ap', 'coded_ap'))
    sp1, mc1 = a.run(x, f0, t)
    ap1, coded1 = a.run(x, f0, t, want=('ap', 'coded_ap'))
    assert numpy.array_equal(sp, sp1) and numpy.array_equal(mc, mc1) and numpy.array_equal(ap, ap1) and numpy.array_equal(coded, coded1)
    assert numpy.array_equal(a.d4c(x, f0, t), ap)
    # the host's 20 log10 of the same ap values against the device's: two log10 implementations, each within a few ulp of values <= 60 (ulp 7e-15)
    assert numpy.abs(world_analysis.code_aperiodicity(ap, fs) - coded).max() <= 1e-13
    a.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_chain_into_the_synthesizer_on_the_device(gpu_ctx, fs):
    """Analyzer.run(device_rows=True) sp + ap -> Synthesizer.synthesize(f0, DeviceRows, DeviceRows): the rows never leave the card, and the wave equals
    the one from the downloaded float32 rows bit for bit."""
    n = 201
    x, f0, t = C.case('glide', 'alternating', n, fs)
    a = world_analysis.Analyzer(fs, seed=6, ctx=gpu_ctx)
    rows_sp, rows_ap = a.run(x, f0, t, want=('sp', 'ap'), device_rows=True)
    assert isinstance(rows_ap, world_synth.DeviceRows) and rows_ap.frames == n
    s = world_synth.Synthesizer(fs, 5.0, seed=6, ctx=gpu_ctx)
    dev = s.synthesize(f0, rows_sp, rows_ap)
    host = s.synthesize(f0, download(gpu_ctx, rows_sp), download(gpu_ctx, rows_ap))
    assert len(dev) == s.length(n) and numpy.isfinite(dev).all() and dev.any() and numpy.array_equal(dev, host)
    s.close(); a.close()


def test_module_functions_and_refusals(gpu_ctx):
    fs = 24000
    x, f0, t = C.case('glide', 'glide', 12, fs)
    a = world_analysis.Analyzer(fs, ctx=gpu_ctx)
    ap, coded = a.run(x, f0, t, want=('ap', 'coded_ap'))
    assert a.bands() == 3 and numpy.array_equal(world_analysis.d4c(x, f0, t, fs), ap)
    got = world_analysis.device_aperiodicity(x, f0, t, fs, 1024)
    assert numpy.array_equal(got[0], ap) and numpy.array_equal(got[1], coded)
    e, c = a.run(x, f0[:0], t[:0], want=('ap', 'coded_ap'))
    assert e.shape == (0, 513) and c.shape == (0, 3)
    with pytest.raises(ValueError, match='empty wave'):
        a.run(x[:0], f0, t, want=('ap',))
    with pytest.raises(_lib.Ry355Error, match='fft_size'):
        world_analysis.d4c(x, f0, t, fs, fft_size=2048)
    with pytest.raises(_lib.Ry355Error, match='12000 Hz'):
        world_analysis.Analyzer(12000, fft_size=1024, ctx=gpu_ctx).d4c(x, f0, t)
    a.close()
