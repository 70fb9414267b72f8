"""WORLD analysis on the MI355X (realtime_yukarin_amd/world_analysis.py) against the numpy float64 restatement (tests/world_analysis_ref.py).

Bars.  The integers of a frame (window half length, centre sample, DC-correction bin limit, smoothing boundary), the float32 rows against
float32(float64 rows) and every bit identity: exact.  sp: max |log sp - log ref| <= 4 x the same figure of the float64 restatement against the
restatement in longdouble with its own transform, worst over the case set; mc: max |mc - ref| / max |ref|, made the same way -- both measured by
scripts/analysis_tolerance.py and read from profiles/r09/analysis_tolerance.txt (lines 1 and 2).  The frames are vetted by
tests/test_world_analysis_ref.py (integer decisions clear of their flips).  The output of a run of this file, with every printed figure against its
bar, is kept as profiles/r09/analysis_pytest_gpu.txt."""
from pathlib import Path

import numpy
import pytest

import world_analysis_cases as C
import world_analysis_ref as R
from oracle import mc2sp as O
from realtime_yukarin_amd import sptk, world_analysis, world_synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
_TOL = (ROOT / 'profiles' / 'r09' / 'analysis_tolerance.txt').read_text().splitlines()
assert _TOL[0].startswith('worst sp') and _TOL[1].startswith('worst mc')
BAR_SP, BAR_MC = 4 * float(_TOL[0].split()[-1]), 4 * float(_TOL[1].split()[-1])


def download(ctx, rows):
    out = numpy.empty((rows.frames, 513), numpy.float32)
    ctx.dev_download(rows.address, out)
    return out


def check(ctx, wk, tk, n, fs, seed=C.SEED):
    x, f0, t = C.case(wk, tk, n, fs)
    floor = C.f0_floor(tk)
    a = world_analysis.Analyzer(fs, fft_size=1024, order=C.ORDER, f0_floor=floor, seed=seed, ctx=ctx)
    a.record_integers()
    rows, sp, mc = a.run(x, f0, t, want=('sp', 'sp64', 'mc'), device_rows=True)
    assert numpy.array_equal(a.integers(), R.integers(f0, t, fs, 1024, floor))
    want = R.cheaptrick(x, f0, t, fs, f0_floor=floor, fft_size=1024, seed=seed)
    want_mc = R.sp2mc(want, C.ORDER, a.alpha)
    assert sp.shape == want.shape and mc.shape == want_mc.shape and sp.dtype == mc.dtype == numpy.float64
    assert numpy.isfinite(sp).all() and numpy.isfinite(mc).all() and (sp > 0).all()
    e_sp = float(numpy.abs(numpy.log(sp) - numpy.log(want)).max())
    e_mc = float(numpy.abs(mc - want_mc).max() / numpy.abs(want_mc).max())
    print('%-6s %-12s fs=%d frames=%3d: sp %.3g (bar %.3g)  mc %.3g (bar %.3g)' % (wk, tk, fs, n, e_sp, BAR_SP, e_mc, BAR_MC))
    assert e_sp <= BAR_SP, e_sp
    assert e_mc <= BAR_MC, e_mc
    assert numpy.array_equal(download(ctx, rows), sp.astype(numpy.float32))              # float32(float64 row), bit for bit
    a.record_integers(False)                                       # the product path: nothing recorded, the same bits
    again = a.run(x, f0, t)
    assert a.integers().shape == (0, 4)
    assert numpy.array_equal(again[0], sp) and numpy.array_equal(again[1], mc)           # two runs: the same bits
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
    sp, mc = a.run(x, f0, t)
    rng = numpy.random.default_rng(3)
    for pick in (rng.permutation(n), rng.permutation(n)[:57], numpy.array([n - 1]), numpy.arange(0, n, 3)):
        sp2, mc2 = a.run(x, f0[pick], t[pick])
        assert numpy.array_equal(sp2, sp[pick]) and numpy.array_equal(mc2, mc[pick])
    a.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_seeds_and_silence(gpu_ctx, fs):
    """All-zero wave: finite sp and mc, and two seeds give different bits (the noise is live).  How far two seeds move log sp of the glide wave is
    printed, not gated: the 1e-12 term is far above float64 rounding at a spectral null."""
    n = 201
    x, f0, t = C.case('zeros', 'alternating', n, fs)
    a, b = world_analysis.Analyzer(fs, seed=1, ctx=gpu_ctx), world_analysis.Analyzer(fs, seed=2, ctx=gpu_ctx)
    za, zb = a.run(x, f0, t), b.run(x, f0, t)
    assert all(numpy.isfinite(v).all() for v in za + zb) and (za[0] > 0).all()
    assert not numpy.array_equal(za[0], zb[0]) and not numpy.array_equal(za[1], zb[1])
    assert numpy.array_equal(world_analysis.Analyzer(fs, seed=1, ctx=gpu_ctx).run(x, f0, t)[0], za[0])
    x, f0, t = C.case('glide', 'glide', n, fs)
    ga, gb = a.run(x, f0, t)[0], b.run(x, f0, t)[0]
    print('fs=%d glide wave, seeds 1 / 2: max |log sp_1 - log sp_2| = %.3g (recorded, not gated; sp bar %.3g)' % (fs, numpy.abs(numpy.log(ga) - numpy.log(gb)).max(), BAR_SP))
    a.close(); b.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_poisoned_buffers(gpu_ctx, fs):
    """After a 2000-frame call has grown every buffer they are filled with NaN bit patterns: a 201-frame call gives the bits of the clean run."""
    x, f0, t = C.case('glide', 'glide', 201, fs)
    a = world_analysis.Analyzer(fs, seed=4, ctx=gpu_ctx)
    clean = a.run(x, f0, t, want=('sp', 'sp64', 'mc'), device_rows=True)
    clean32 = download(gpu_ctx, clean[0])
    a.run(*C.case('noise', 'alternating', 2000, fs), want=('sp64', 'mc'))
    a.poison()
    got = a.run(x, f0, t, want=('sp', 'sp64', 'mc'), device_rows=True)
    assert numpy.isfinite(got[1]).all() and numpy.isfinite(got[2]).all()
    assert numpy.array_equal(got[1], clean[1]) and numpy.array_equal(got[2], clean[2]) and numpy.array_equal(download(gpu_ctx, got[0]), clean32)
    a.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_chain_into_the_synthesizer_on_the_device(gpu_ctx, fs):
    """Analyzer.run(device_rows=True) -> Synthesizer.synthesize(f0, DeviceRows, ap): the rows never leave the card, and the wave equals the one from
    the downloaded float32 rows bit for bit."""
    n = 201
    x, f0, t = C.case('glide', 'alternating', n, fs)
    a = world_analysis.Analyzer(fs, seed=6, ctx=gpu_ctx)
    rows, = a.run(x, f0, t, want=('sp',), device_rows=True)
    assert isinstance(rows, world_synth.DeviceRows) and rows.frames == n
    ap = numpy.random.default_rng(11).uniform(0.001, 0.999, (n, 513)).astype(numpy.float32)
    s = world_synth.Synthesizer(fs, 5.0, seed=6, ctx=gpu_ctx)
    dev = s.synthesize(f0, rows, ap)
    host = s.synthesize(f0, download(gpu_ctx, rows), ap)
    assert len(dev) == s.length(n) and numpy.isfinite(dev).all() and dev.any() and numpy.array_equal(dev, host)
    s.close(); a.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_sp2mc_round_trip_and_device_rows(gpu_ctx, fs):
    """Analyzer.sp2mc(oracle mc2sp(mc0)) against mc0; bar: 4 x what the numpy restatement's round trip leaves."""
    alpha = sptk.mcepalpha(fs)
    mc0 = numpy.random.default_rng(9).normal(0.0, 0.3, (60, C.ORDER + 1))
    mc0[:, 0] -= 4.0
    sp = O.mc2sp(mc0, alpha, 1024)
    bar = 4 * float(numpy.abs(R.sp2mc(sp, C.ORDER, alpha) - mc0).max() / numpy.abs(mc0).max())
    a = world_analysis.Analyzer(fs, order=C.ORDER, ctx=gpu_ctx)
    got = a.sp2mc(sp)
    e = float(numpy.abs(got - mc0).max() / numpy.abs(mc0).max())
    print('fs=%d sp2mc round trip: %.3g (bar %.3g)' % (fs, e, bar))
    assert e <= bar
    rows = world_synth.to_device(gpu_ctx, sp)
    assert numpy.array_equal(a.sp2mc(rows), a.sp2mc(sp.astype(numpy.float32)))
    assert numpy.array_equal(a.sp2mc(sp[[5, 3]]), got[[5, 3]])
    a.close()


def test_module_functions_and_empty_calls(gpu_ctx):
    fs = 24000
    x, f0, t = C.case('noise', 'glide', 12, fs)
    a = world_analysis.Analyzer(fs, ctx=gpu_ctx)
    sp, mc = a.run(x, f0, t)
    assert numpy.array_equal(world_analysis.cheaptrick(x, f0, t, fs), sp)
    assert numpy.array_equal(world_analysis.sp2mc(sp, 8, a.alpha), a.sp2mc(sp))
    e, m = a.run(x, f0[:0], t[:0])
    assert e.shape == (0, 513) and m.shape == (0, 9)
    with pytest.raises(ValueError, match='empty wave'):
        a.run(x[:0], f0, t)
    a.close()
