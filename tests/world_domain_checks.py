"""The bodies tests/test_world_domain_cpu.py (emulator) and tests/test_world_domain_gpu.py (MI355X) share: each takes the context it runs on.
What they assert is what tests/test_world_analysis_*.py, test_world_d4c_*.py and test_world_synth_*.py assert, on the inputs of
tests/world_domain_cases.py.  Bars: 4 x the figure the float64 restatement has against the longdouble one on the same inputs, per group, read from
profiles/r13/world_domain_tolerance.txt (scripts/world_domain_tolerance.py); integers, flags, lengths and every bit identity are exact."""
import ctypes
from pathlib import Path

import numpy

import world_analysis_cases as A
import world_analysis_ref as RA
import world_d4c_ref as RD
import world_domain_cases as C
import world_synth_cases as S
import world_synth_ref as RS
from realtime_yukarin_amd import _lib, world_analysis, world_synth

ROOT = Path(__file__).resolve().parent.parent
_DP = ctypes.POINTER(ctypes.c_double)


def _bars():
    out = {}
    for line in (ROOT / 'profiles' / 'r13' / 'world_domain_tolerance.txt').read_text().splitlines():
        if line and not line.startswith('#'):
            label, value = line.rsplit(None, 1)
            out[label] = 4 * float(value)
    return out


BARS = _bars()
BINS = C.BINS


def mc_bar(path, order, alpha):
    return BARS['mc %s order=%d alpha=%g' % (path, order, alpha)]


def download(ctx, rows):
    out = numpy.empty((rows.frames, BINS), numpy.float32)
    if rows.frames:
        ctx.dev_download(rows.address, out)
    return out



# ---- CheapTrick ----------------------------------------------------------------------------------------------------------------------
def cheaptrick(ctx, wk, tk, n, fs, q1=-0.15, floor=C.FLOOR, inputs=None, order=A.ORDER):
    x, f0, t = inputs if inputs is not None else C.case(wk, tk, n, fs)
    a = world_analysis.Analyzer(fs, fft_size=1024, order=order, q1=q1, f0_floor=floor, seed=C.SEED, ctx=ctx)
    a.record_integers()
    rows, sp, mc = a.run(x, f0, t, want=('sp', 'sp64', 'mc'), device_rows=True)
    ints = a.integers()
    assert numpy.array_equal(ints, RA.integers(f0, t, fs, 1024, floor))
    want = RA.cheaptrick(x, f0, t, fs, q1=q1, f0_floor=floor, fft_size=1024, seed=C.SEED)
    want_mc = RA.sp2mc_rows(want, order, a.alpha)
    assert sp.shape == want.shape and mc.shape == want_mc.shape and sp.dtype == mc.dtype == numpy.float64
    assert numpy.isfinite(sp).all() and numpy.isfinite(mc).all() and (sp > 0).all()
    e_sp = float(numpy.abs(numpy.log(sp) - numpy.log(want)).max())
    e_mc = float(numpy.abs(mc - want_mc).max() / numpy.abs(want_mc).max())
    bar_mc = BARS['mc cases']                                      # order 8, alpha = mcepalpha(fs)
    print('%-6s %-8s fs=%5d frames=%2d q1=%g floor=%g h<=%d L<=%d b<=%d: sp %.3g (bar %.3g)  mc %.3g (bar %.3g)'
          % (wk, tk, fs, n, q1, floor, ints[:, 0].max(), ints[:, 2].max(), ints[:, 3].max(), e_sp, BARS['sp'], e_mc, bar_mc))
    assert e_sp <= BARS['sp'], e_sp
    assert e_mc <= bar_mc, e_mc
    assert numpy.array_equal(download(ctx, rows), sp.astype(numpy.float32))
    a.record_integers(False)
    again = a.run(x, f0, t)
    assert numpy.array_equal(again[0], sp) and numpy.array_equal(again[1], mc)                # two runs: the same bits
    a.close()
    return ints


def cheaptrick_case(ctx, wk, tk, n, fs):
    x, f0, t = C.case(wk, tk, n, fs)
    ints = cheaptrick(ctx, wk, tk, n, fs, inputs=(x, f0, t))
    if tk == 'lowest' and fs >= 16000:
        assert (ints[:, 0] == 510).all()                           # 1021 samples: the whole window loop is live
    if tk == 'high':
        assert ints[0, 2] == 511 and ints[0, 3] == 342             # the clamp of L and the widest mirror
    if tk == 'offgrid' and n >= 13:
        assert (ints[:, 1] < 0).sum() >= 3 and ints[0, 1] == -fs and ints[-1, 1] == int(C.T_LAST) * fs


def permutation(ctx, tk, fs, n, d4c):
    x, f0, t = C.case('glide', tk, n, fs)
    want = ('sp', 'mc', 'ap', 'coded_ap') if d4c else ('sp', 'mc')
    a = world_analysis.Analyzer(fs, fft_size=1024, f0_floor=C.FLOOR, seed=2, ctx=ctx)
    kw = dict(threshold=C.threshold(tk)) if d4c else {}
    full = a.run(x, f0, t, want=want, **kw)
    pick = numpy.random.default_rng(3).permutation(n)[:max(n // 2, 1)]
    part = a.run(x, f0[pick], t[pick], want=want, **kw)
    assert all(numpy.array_equal(p, f[pick]) for p, f in zip(part, full))
    a.close()


# ---- sp2mc ---------------------------------------------------------------------------------------------------------------------------
def sp2mc(ctx, order, alpha, fs=16000):
    sp = C.sp2mc_rows(order, alpha)
    want = RA.sp2mc_rows(sp, order, alpha)
    a = world_analysis.Analyzer(fs, fft_size=1024, order=order, alpha=alpha, f0_floor=C.FLOOR, seed=C.SEED, ctx=ctx)
    mc = a.sp2mc(sp)
    bar = mc_bar('sp2mc', order, alpha)
    e = float(numpy.abs(mc - want).max() / numpy.abs(want).max())
    assert mc.shape == (C.SP2MC_ROWS, order + 1) and numpy.isfinite(mc).all()
    # the other way in: CheapTrick's own rows (Analyzer.run), the mel-cepstrum of the restatement's spectrogram
    x, f0, t = A.case('glide', 'glide', 13, fs)
    sp_run, mc_run = a.run(x, f0, t, want=('sp', 'mc'))
    assert numpy.array_equal(a.run(x, f0, t, want=('mc',))[0], mc_run)
    want_run = RA.sp2mc_rows(RA.cheaptrick(x, f0, t, fs, f0_floor=C.FLOOR, fft_size=1024, seed=C.SEED), order, alpha)
    bar_run = mc_bar('run', order, alpha)
    e_run = float(numpy.abs(mc_run - want_run).max() / numpy.abs(want_run).max())
    print('order=%2d alpha=%6g: sp2mc %.3g (bar %.3g)  run %.3g (bar %.3g)' % (order, alpha, e, bar, e_run, bar_run))
    assert e <= bar, e
    assert e_run <= bar_run, e_run
    if alpha == 0.0:                                               # S is a selection: mc = the first order + 1 cepstral values, c0 halved
        cep = numpy.array([RA.cepstrum(r)[:order + 1] for r in sp])
        cep[:, 0] /= 2
        assert float(numpy.abs(mc - cep).max() / numpy.abs(cep).max()) <= bar
    assert numpy.array_equal(a.sp2mc(sp), mc)
    rows = world_synth.to_device(ctx, sp)
    assert numpy.array_equal(a.sp2mc(rows), a.sp2mc(sp.astype(numpy.float32)))
    a.close()


# ---- D4C -----------------------------------------------------------------------------------------------------------------------------
def d4c_case(ctx, wk, tk, n, fs):
    x, f0, t = C.case(wk, tk, n, fs)
    a = world_analysis.Analyzer(fs, fft_size=1024, f0_floor=C.FLOOR, seed=C.SEED, ctx=ctx)
    a.record_integers()
    th = C.threshold(tk)
    rows, ap, coded = a.run(x, f0, t, want=('ap', 'ap64', 'coded_ap'), device_rows=True, threshold=th)
    ints, on, a0, coarse = a.d4c_record()
    want, want_a0, want_on, want_coarse = RD.d4c(x, f0, t, fs, threshold=th, seed=C.SEED, details=True)
    assert numpy.array_equal(ints, RD.integers(f0, t, fs))
    assert numpy.array_equal(on, want_on)
    assert ap.shape == want.shape and coded.shape == (n, RD.bands(fs))
    assert numpy.isfinite(ap).all() and numpy.isfinite(coded).all() and (ap > 0).all() and (ap <= 1).all()
    e_a0 = float(numpy.abs(a0 - want_a0).max())
    e_co = float(numpy.abs(coarse[on] - want_coarse[on]).max()) if on.any() else 0.0
    e_ap = float(numpy.abs(20 * numpy.log10(ap) - 20 * numpy.log10(want)).max())
    e_cd = float(numpy.abs(coded - RD.code_aperiodicity(want, fs)).max())
    print('%-6s %-8s fs=%5d frames=%2d on=%2d h4<=%d L<=%d b1<=%d b2<=%d: a0 %.3g (bar %.3g)  coarse %.3g (bar %.3g)  ap %.3g (bar %.3g)  coded_ap %.3g (bar %.3g)'
          % (wk, tk, fs, n, on.sum(), ints[:, 1].max(), ints[:, 5].max(), ints[:, 6].max(), ints[:, 7].max(),
             e_a0, BARS['a0'], e_co, BARS['coarse'], e_ap, BARS['ap'], e_cd, BARS['coarse']))
    assert e_a0 <= BARS['a0'], e_a0
    assert e_co <= BARS['coarse'], e_co
    assert e_ap <= BARS['ap'], e_ap
    assert e_cd <= BARS['coarse'], e_cd
    assert numpy.array_equal(ap[~on], want[~on])
    assert numpy.array_equal(download(ctx, rows), ap.astype(numpy.float32))
    again = a.run(x, f0, t, want=('ap', 'coded_ap'), threshold=th)
    assert numpy.array_equal(again[0], ap) and numpy.array_equal(again[1], coded)
    a.close()
    if tk == 'lowest47' and fs == 24000 and n >= 2:
        assert ints[1, 1] == 1021                                  # 2043 of 2048 samples
    if tk == 'high':
        assert tuple(ints[0, 5:8]) == (1023, 1024, 512) and bool(on[0]) == (wk == 'glide')   # the general body at its limits, and the off branch
    if tk == 'offgrid':
        assert ints[0, 3] == -fs


def poisoned_analysis(ctx, fs, grow):
    """CheapTrick, sp2mc and D4C on `lowest` after a larger call has grown every buffer and all of them were filled with NaN patterns."""
    x, f0, t = C.case('glide', 'lowest', 13, fs)
    want = ('sp', 'mc', 'ap', 'coded_ap')
    a = world_analysis.Analyzer(fs, fft_size=1024, f0_floor=C.FLOOR, seed=4, ctx=ctx)
    clean = a.run(x, f0, t, want=want)
    a.record_integers()
    a.run(*A.case('noise', 'alternating', grow, fs), want=want)
    a.record_integers(False)
    a.poison()
    got = a.run(x, f0, t, want=want)
    assert all(numpy.isfinite(g).all() and numpy.array_equal(g, c) for g, c in zip(got, clean))
    a.close()


# ---- synthesis -----------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(numpy.abs(a - b).max() / max(numpy.abs(b).max(), 1e-300))


def synth_check(s, f0, sp, ap, seed, label=''):
    fs, fp = s.fs, s.frame_period
    want, P, _ = RS.synthesize(f0, sp, ap, fs, fp, seed=seed, fft_size=1024, return_pulses=True)
    y = s.synthesize(f0, sp, ap)
    idx, shift, voiced = s.pulses()
    assert len(y) == len(want) == int((len(f0) - 1) * fp / 1000 * fs) + 1
    assert numpy.array_equal(idx, numpy.array([p[0] for p in P], numpy.int64)) and list(voiced) == [p[2] for p in P]
    assert numpy.isfinite(y).all()
    if P:
        assert numpy.abs(shift - numpy.array([p[1] for p in P])).max() <= 1e-9
        e = rel(y, want)
        print('%s fs=%5d period=%g frames=%4d: %4d pulses, rel err %.3g (bar %.3g)' % (label, fs, fp, len(f0), len(P), e, BARS['synthesis waveform']))
        assert e <= BARS['synthesis waveform'], e
    else:
        assert not y.any()
    return y, idx


def synth_case(ctx, fs, fp, kind, n):
    n = C.synth_frames(n, fs, fp)
    f0, sp, ap = C.synth_case(kind, n, fs)
    s = world_synth.Synthesizer(fs, fp, seed=1, ctx=ctx, fft_size=1024)
    y, idx = synth_check(s, f0, sp, ap, 1, kind)
    assert numpy.array_equal(s.synthesize(f0, sp, ap), y)
    if kind == 'high' and len(idx) > 100:
        assert {2, 3} <= set(numpy.diff(idx).tolist())             # noise sizes of 2 and 3
    s.close()


def synth_stream(ctx, fs, fp, n, seed=3):
    n = C.synth_frames(n, fs, fp)
    f0, sp, ap = C.synth_case('glide', n, fs)
    s = world_synth.Synthesizer(fs, fp, seed=seed, ctx=ctx, fft_size=1024)
    want = s.synthesize(f0, sp, ap)
    rng = numpy.random.default_rng(5)
    ragged = []
    while sum(ragged) < n:
        ragged.append(min(int(rng.integers(1, max(n // 3, 2))), n - sum(ragged)))
    k = min(5, n - 1)
    for cuts in ([1] * k + [n - k], ragged, [1] * n):
        out, i, lag = [], 0, 0
        for c in cuts:
            out.append(s.push(f0[i:i + c], sp[i:i + c], ap[i:i + c]))
            i += c
            lag = max(lag, s.length(i) - sum(map(len, out)))
        out.append(s.flush())
        assert numpy.array_equal(numpy.concatenate(out), want), cuts[:8]
        assert lag <= s.lag_samples(f0=fs / 1024 + 1) + 1, lag
    s.close()


def poisoned_synth(ctx, n, grow):
    fs, fp = 16000, 5.8
    f0, sp, ap = C.synth_case('high', n, fs)
    s = world_synth.Synthesizer(fs, fp, seed=8, ctx=ctx, fft_size=1024)
    clean, _ = synth_check(s, f0, sp, ap, 8, 'high')
    s.synthesize(*S.case('unvoiced', grow, fs))
    s.poison()
    y = s.synthesize(f0, sp, ap)
    assert numpy.isfinite(y).all() and numpy.array_equal(y, clean)
    s.poison()
    out = []
    for a, b in ((0, n // 3), (n // 3, n // 3 + 1), (n // 3 + 1, n)):
        out.append(s.push(f0[a:b], sp[a:b], ap[a:b]))
        s.poison()
    out.append(s.flush())
    y = numpy.concatenate(out)
    assert numpy.isfinite(y).all() and numpy.array_equal(y, clean)
    s.close()
    # one sample per frame, the last sample a wrap: it sits exactly on the last frame, and the f0 slot behind that frame holds a NaN pattern
    fs, fp = 16000, 0.0625
    m = C.frames_ending_on_a_wrap(fs, fp)
    f0, sp, ap = C.synth_case('high', m, fs)
    s = world_synth.Synthesizer(fs, fp, seed=8, ctx=ctx, fft_size=1024)
    s.synthesize(*S.case('unvoiced', max(grow, 3 * m), fs))      # the f0 buffer now reaches well behind frame m - 1
    s.poison()
    y, idx = synth_check(s, f0, sp, ap, 8, 'high')
    assert idx[-1] == len(y) - 2
    s.close()


# ---- refusals: every one returns before a launch ----------------------------------------------------------------------------------------
def refusals(ctx):
    lib, d = ctx.lib, ctx.lib.dll
    h = ctypes.c_void_p()
    # synthesis: the rate, and f0 at or above fs / 2 (a first phase step of 2 pi or more would put a pulse at sample -1, in front of the frame window)
    for fs in (7999, 48001, 1000, 384000):
        assert d.ry_synth_create(ctx.handle, fs, 5.0, 1024, 0, ctypes.byref(h)) == -1 and not h.value and b'sampling rate' in d.ry_last_error()
    for fs in (8000, 48000):
        lib.check(d.ry_synth_create(ctx.handle, fs, 5.0, 1024, 0, ctypes.byref(h)))
        d.ry_synth_destroy(h)
    assert d.ry_synth_create(ctx.handle, 16000, 0.0624, 1024, 0, ctypes.byref(h)) == -1 and b'shorter than a sample' in d.ry_last_error()
    lib.check(d.ry_synth_create(ctx.handle, 16000, 5.0, 1024, 0, ctypes.byref(h)))
    n = 4
    f0, sp, ap = S.case('glide', n, 16000)
    y, got = numpy.full(400, numpy.nan), ctypes.c_int(-5)
    for fn in (d.ry_synth_run, d.ry_synth_push):
        for i, bad in ((0, 16000.0), (0, 8000.0), (3, 8000.0), (2, 1e300)):
            g = f0.copy(); g[i] = bad
            rc = fn(h, g.ctypes.data_as(_DP), _lib._fptr(sp), _lib._fptr(ap), n, 513, 0, y.ctypes.data_as(_DP), 400, ctypes.byref(got))
            assert rc == -1 and b'f0[%d]' % i in d.ry_last_error() and b'below fs / 2' in d.ry_last_error()
            assert got.value == 0 and numpy.isnan(y).all()
        g = f0.copy(); g[0] = numpy.nextafter(8000.0, 0.0)         # the largest f0 below fs / 2 passes the check (y too small: refused later)
        rc = fn(h, g.ctypes.data_as(_DP), _lib._fptr(sp), _lib._fptr(ap), n, 513, 0, y.ctypes.data_as(_DP), 10, ctypes.byref(got))
        assert rc == -1 and b'y holds' in d.ry_last_error()
    assert d.ry_synth_flush(h, y.ctypes.data_as(_DP), 400, ctypes.byref(got)) == -4              # no refused push left frames behind
    d.ry_synth_destroy(h)
    # analysis: alpha, q1, f0_floor at the handle; t at the call (CheapTrick and D4C alike)

    def create(fs=16000, alpha=0.41, q1=-0.15, floor=71.0):
        return d.ry_analysis_create(ctx.handle, fs, 1024, 8, alpha, q1, floor, 0, ctypes.byref(h))
    for kw, word in ((dict(alpha=0.9000001), b'alpha'), (dict(alpha=-0.95), b'alpha'), (dict(alpha=numpy.nan), b'alpha'),
                     (dict(q1=0.01), b'q1'), (dict(q1=-0.41), b'q1'), (dict(q1=numpy.nan), b'q1'),
                     (dict(floor=0.5), b'f0_floor'), (dict(floor=1000.5), b'f0_floor'), (dict(floor=-71.0), b'f0_floor'), (dict(floor=numpy.inf), b'f0_floor'),
                     (dict(fs=7999), b'sampling rate'), (dict(fs=48001), b'sampling rate')):
        assert create(**kw) == -1 and not h.value and word in d.ry_last_error(), kw
    for kw in (dict(alpha=0.9), dict(alpha=-0.9), dict(q1=0.0), dict(q1=-0.4), dict(floor=1.0), dict(floor=1000.0), dict(fs=8000), dict(fs=48000)):
        lib.check(create(**kw))
        d.ry_analysis_destroy(h)
    lib.check(create())
    x, f0, t = A.case('noise', 'glide', 4, 16000)
    sp64 = numpy.full((4, 513), numpy.nan)
    null = ctypes.cast(ctypes.c_void_p(0), _DP)
    for bad in (-1.0000001, 1000000.5, 1e9, -numpy.inf, numpy.nan):
        g = t.copy(); g[1] = bad
        args = (h, x.ctypes.data_as(_DP), x.size, f0.ctypes.data_as(_DP), g.ctypes.data_as(_DP), 4)
        assert d.ry_analysis_run(*args, sp64.ctypes.data_as(_DP), _lib._fptr(None), null) == -1 and b't[1]' in d.ry_last_error()
        assert d.ry_analysis_d4c(*args, 0.85, sp64.ctypes.data_as(_DP), _lib._fptr(None), null) == -1 and b't[1]' in d.ry_last_error()
    assert numpy.isnan(sp64).all()
    d.ry_analysis_destroy(h)
