"""Every node of the stage-2 convert graph against float64, layer by layer, on poisoned buffers (RY_POISON=1, a fresh plan per run).

`engine.Net.debug_activation` (`ry_net_debug_activation`, test-only) hands back the padded input and every layer's fp32 / 16-bit buffer after a real
`convert`; `cases.s2_walk` restates each layer in float64 ON THE INPUT THE DEVICE ITSELF READ with the filters of the parameter dict, so errors do not
chain: the bar is one layer's summation error (cases.F32_TOL / BF16_TOL / X3_TOL times the element's own bound), and an element a node should have
written is NaN at that node.  Which rows a window needs is restated from the operators' stencils (cases.s2_needed_rows), never asked of the library:
every needed row is finite and within the bar, every NaN row is not needed.  The fused exp of the end layer and the log of the pad node are held to
E / E_log, the measured accuracy of the device's expf / logf (profiles/r12/stage2_graph_tolerance.txt, scripts/stage2_graph_tolerance.py).

`-s` prints, per layer and mode, the worst |y - r| / bound, the NaN-row counts, the kernel names and the worst expf / logf errors met.

Measured on MI355X (profiles/r12/stage2_graph_pytest_gpu.txt) and on the emulator (stage2_graph_pytest_emu.txt)."""
import ctypes

import numpy
import pytest

import cases
from realtime_yukarin_amd import _lib, engine, sptk, synth
from realtime_yukarin_amd.netspec import NetDesc, pad_frames
from realtime_yukarin_amd.weights import flatten_params, synthetic_params

F32_TOL = cases.F32_TOL
E, E_LOG = cases.s2_tolerances()


def _sp(n_frames, bins, windows=1, seed=91):
    return synth.stage2_input(n_frames, windows, seed=seed, bins=bins)


def _print_walk(what, w, end=None, elog=None):
    for q in w['layers']:
        f = lambda v: '   -    ' if v is None else '%8.3g' % v
        print('%-46s %-11s %-5s need %4d..%-4d worst %s  worst16 %s  NaN rows fp32 %s 16-bit %s%s'
              % (what, q['layer'], q['fmt'], q['need'][0], q['need'][1], f(q['worst']), f(q['worst16']), q['nan32'], q['nan16'], '  (reference of the whole run)' if q['reused'] else ''))
    if end is not None:
        print('%-46s end        |log y - r| / (F32_TOL bound + E) = %.3g   logf rel err %.3g (E_log %.3g)' % (what, end, elog, E_LOG))


def _names(net, n_frames):
    return {q['name'].split('<')[0] if not q['name'].startswith('ry_sr_last<') else q['name'] for q in net.profile(1, n_frames, 1, window=True)}


def _run(ctx, monkeypatch, net, desc, P, sp, mode, discard=(0, 0), prof=(), refs=True, cache=None, what=''):
    """One convert on a fresh poisoned plan + the walk, the pad check and the end check.  -> (y, walk)"""
    n = sp.shape[1]
    net.set_dtype(mode)                                   # drops the plans: the next convert builds poisoned buffers
    y = net.convert(sp, discard=discard)
    w = cases.s2_walk(net, desc, P, n, y, discard, prof, refs, cache, what=what)
    elog = cases.s2_check_pad(w['x_in'], sp, n, True, E_LOG, what)
    pad = w['x_in'][:, n:]
    assert pad.shape[1] == pad_frames(n)
    end = cases.s2_check_end(w, P, y, n, E, what)
    k0, k1 = w['k']
    assert not y[:, :k0].any() and not y[:, k1:].any(), (what, 'discarded rows come back as zeros (host call)')
    _print_walk(what, w, end, elog)
    return y, w


def _hole_stretches(w, n_frames):
    """Down the encoder the rows behind the real frames are copies of ONE row, so every layer has a stretch of output rows that are equal bit for bit:
    identical input rows [a, b] give identical output rows [ceil((a + p) / s), floor((b - (k - 1) + p) / s)].  -> [(layer, first, last)] checked"""
    a, b = n_frames, w['x_in'].shape[1] - 1
    out = []
    for i in range(8):
        spec = w['specs'][i]
        a, b = -(-(a + spec['p']) // spec['s']), (b - (spec['k'] - 1) + spec['p']) // spec['s']
        for kind, o in enumerate(w['raw'][i]):
            if o is None:
                continue
            b = min(b, o.shape[1] - 1)
            if b - a < 1:
                return out
            bits = o.view(numpy.uint32) if o.dtype == numpy.float32 else o
            assert (bits[:, a:b + 1] == bits[:, a:a + 1]).all(), (spec['name'], kind, 'rows %d .. %d behind the real frames are not bit-identical' % (a, b))
            out.append((spec['name'], a, b))
    return out


def _untouched_rows(ctx, net, sp, discard):
    """The device-pointer call: rows outside [k0, k1) of the caller's block stay as they were."""
    B, n, C = sp.shape
    d_in, d_out = ctx.dev_alloc(sp.size), ctx.dev_alloc(sp.size)
    try:
        mark = numpy.full(sp.shape, -7.25, 'f4')
        ctx.dev_upload(d_in, sp); ctx.dev_upload(d_out, mark)
        ctx.lib.check(ctx.lib.dll.ry_sr_convert_rows(net.handle, _lib._fptr(d_in), _lib._fptr(d_out), B, n, discard[0], discard[1], 1))
        ctx.sync()
        y = numpy.empty(sp.shape, 'f4')
        ctx.dev_download(d_out, y)
    finally:
        ctx.dev_free(d_in); ctx.dev_free(d_out)
    return y


# ---- SYN-64, width 512, one window of 100 frames (T = 128): the smallest window with the fused end layer, Winograd, the dead-row crop and the copied rows ----

SYN64_MODES = [('f32', '1'), ('f32', '0'), ('bf16', '1'), ('bf16x3', '1')]


@pytest.fixture(scope='module')
def syn64_params():
    return synth.model_params('SYN-64')[1]


@pytest.mark.gpu
@pytest.mark.parametrize('mode,wino', SYN64_MODES, ids=['f32-winograd', 'f32-direct', 'bf16', 'bf16x3'])
def test_syn64_layer_walk_gpu(gpu_ctx, monkeypatch, syn64_params, mode, wino):
    """The whole window and the same window with discard = (20, 20): every layer against float64 on the device's sources, needed rows finite, NaN rows
    not needed, at least one decoder layer with uncomputed rows in both runs (the default RY_S2_CROP=2 is seen), 16-bit copies the roundings of their
    fp32 twins, copied encoder rows bit-identical, the end layer under exp, discarded rows zero (host) / untouched (device)."""
    d2, P2 = syn64_params
    n = 100
    sp = _sp(n, synth.FFT_BINS)
    monkeypatch.setenv('RY_WINOGRAD', wino)
    tag = 'SYN-64 n=100 %s%s' % (mode, '' if wino == '1' else ' RY_WINOGRAD=0')
    try:
        with cases.poisoned(gpu_ctx, monkeypatch):
            net = engine.Net(gpu_ctx, d2, flatten_params(d2, P2), width=synth.FFT_BINS - 1)
            net.set_dtype(mode)
            net.convert(sp)
            prof = net.profile(1, n, 1, window=True)
            print('%-46s kernels %s' % (tag, sorted(_names(net, n))))
            rep = bool([q for q in prof if q['name'] == 'ry_rep_rows'])
            if mode == 'f32' and wino == '1':
                assert [q for q in prof if q['name'].startswith('ry_wino_ldsdma<')]
            cache = {}
            y, w = _run(gpu_ctx, monkeypatch, net, d2, P2, sp, mode, prof=prof, cache=cache, what=tag + ' whole')
            assert w['fused']
            holes = _hole_stretches(w, n)
            assert holes
            print('%-46s bit-identical stretches %s' % (tag, holes))
            yd, wd = _run(gpu_ctx, monkeypatch, net, d2, P2, sp, mode, discard=(20, 20), prof=prof, cache=cache, what=tag + ' discard (20, 20)')
            assert numpy.array_equal(yd[:, 20:80], y[:, 20:80])
            for ww in (w, wd):
                assert any((q['nan32'] or 0) + (q['nan16'] or 0) > 0 for q in ww['layers'][8:15]), 'the dead-row crop left no decoder row out'
            if mode == 'f32' and not rep:       # 8-row Winograd tiles: no whole tile row inside the 12 identical rows of encoder c1 at 100 frames; 130 (T = 256) has six
                sp2 = _sp(130, synth.FFT_BINS)
                net.set_dtype(mode); net.convert(sp2)
                assert [q for q in net.profile(1, 130, 1, window=True) if q['name'] == 'ry_rep_rows'], 'no copied rows at 100 nor at 130 frames'
                _, w2 = _run(gpu_ctx, monkeypatch, net, d2, P2, sp2, mode, what=tag.replace('n=100', 'n=130') + ' whole')
                holes = _hole_stretches(w2, 130)
                print('%-46s bit-identical stretches at 130 frames %s' % (tag, holes))
                rep = True
            assert rep or mode != 'f32', 'no ry_rep_rows node in fp32 mode'
            yu = _untouched_rows(gpu_ctx, net, sp, (20, 20))
            assert numpy.array_equal(yu[:, 20:80], y[:, 20:80]) and (yu[:, :20] == -7.25).all() and (yu[:, 80:] == -7.25).all()
            net.close()
    finally:
        monkeypatch.delenv('RY_WINOGRAD', raising=False); gpu_ctx.reload_env()


@pytest.mark.gpu
@pytest.mark.parametrize('B,n', [(1, 1), (1, 101), (2, 100)], ids=['1-frame', '101-frames', '2-windows-of-100'])
def test_syn64_end_layer_strip_counts_gpu(gpu_ctx, monkeypatch, syn64_params, B, n):
    """ry_sr_last<false> with other strip counts modulo 64 (B rows_valid 32 strips: 32, 3232, 6400), so that its XCD bands end on another workgroup and
    the `lb >= nb` return is taken: the end layer against float64, every needed row of every other layer finite."""
    d2, P2 = syn64_params
    sp = _sp(n, synth.FFT_BINS, B)
    with cases.poisoned(gpu_ctx, monkeypatch):
        net = engine.Net(gpu_ctx, d2, flatten_params(d2, P2), width=synth.FFT_BINS - 1)
        y, w = _run(gpu_ctx, monkeypatch, net, d2, P2, sp, 'f32', refs=False, what='SYN-64 B=%d n=%d f32' % (B, n))
        assert w['fused']
        net.close()


# ---- the padded input (ry_pad_min_rows<16 / 64>) ----

def _stage2_pad(ctx, monkeypatch, n, width, base=8):
    d = NetDesc(2, 1, 1, base, 8)
    P = synthetic_params(d, 431, bias_std=0.05)
    sp = _sp(n, width + 1)
    with cases.poisoned(ctx, monkeypatch):
        net = engine.Net(ctx, d, flatten_params(d, P), width=width)
        y = net.convert(sp)
        x_in = net.debug_activation(-1)
        net.close()
    assert x_in.shape == (1, n + pad_frames(n), width) and numpy.isfinite(y).all()
    e = cases.s2_check_pad(x_in, sp, n, True, E_LOG, 'stage 2 n=%d width=%d' % (n, width))
    print('stage-2 padded input n=%4d width=%3d: worst logf rel err %.3g (E_log %.3g)' % (n, width, e, E_LOG))


@pytest.mark.gpu
@pytest.mark.parametrize('n,width', [(1, 512), (100, 512), (128, 512), (513, 128)])
def test_stage2_padded_input_gpu(gpu_ctx, monkeypatch, n, width):
    """513 columns: the last workgroup has one live column; 1 / 100 frames: rows_in below / off a multiple of the 16 row groups; 128: a whole extra
    block of pad rows; 513 frames (<64>): the second round of loads."""
    _stage2_pad(gpu_ctx, monkeypatch, n, width)


@pytest.mark.parametrize('n,width', [(1, 128), (100, 128), (128, 128), (513, 128)])
def test_stage2_padded_input_emu(emu_ctx, monkeypatch, n, width):
    _stage2_pad(emu_ctx, monkeypatch, n, width)


def _stage1_pad(ctx, monkeypatch, in_ch, n):
    d = NetDesc(1, in_ch, 9, 16, 8)
    P = synthetic_params(d, 432, bias_std=0.05)
    x = synth.stage1_input(n, stress=in_ch == 523)
    assert x.shape == (1, n, in_ch)
    with cases.poisoned(ctx, monkeypatch):
        net = engine.Net(ctx, d, flatten_params(d, P))
        y = net.convert(x)
        x_in = net.debug_activation(-1)
        if in_ch <= 64:                                   # a short window of a narrow input: the first layer pads for itself and the call says so
            net.convert(x[:, :100])
            with pytest.raises(_lib.Ry355Error, match='was not written'):
                net.debug_activation(-1)
        with pytest.raises(_lib.Ry355Error, match='stage-2'):
            net.debug_activation(0)
        net.close()
    assert numpy.isfinite(y).all()
    cases.s2_check_pad(x_in, x, n, False, 0.0, 'stage 1 in_ch=%d n=%d' % (in_ch, n))


@pytest.mark.gpu
@pytest.mark.parametrize('in_ch,n', [(9, 2049), (523, 300)])
def test_stage1_padded_input_gpu(gpu_ctx, monkeypatch, in_ch, n):
    """No log: the whole block is bit-equal to numpy.pad(mode='minimum').  2049 frames: five rounds of loads of <64>, rows_in off a multiple of 64;
    523 columns: off a multiple of 16."""
    _stage1_pad(gpu_ctx, monkeypatch, in_ch, n)


@pytest.mark.parametrize('in_ch,n', [(9, 2049), (523, 300)])
def test_stage1_padded_input_emu(emu_ctx, monkeypatch, in_ch, n):
    _stage1_pad(emu_ctx, monkeypatch, in_ch, n)


# ---- small predictors in convert mode: the end-layer forms SYN-64 never takes ----

# (base, extensive_layers, width, windows)
SMALL_NETS = [
    (12, 3, 24, 1),       # N / 4 = 3 quads: the division path of ry_sr_first (qshift = -1); no implicit-GEMM layout: ry_conv_direct everywhere + ry_sr_post
    (16, 0, 10, 2),       # 1x1 layers only (k1 end layers: ry_conv_direct + ry_sr_post), two windows
    (12, 1, 10, 2),       # k3 end layers without a down layer: ry_sr_first on W % 4 = 2 (the ragged last pixel group; extensive_layers = 0 has no 3x3 first layer)
    (64, 3, 24, 1),       # 2 base = 128 channels into the end layer, W % 16 != 0: ry_sr_last_gather under exp with the edge bin
    (32, 3, 40, 1),       # 2 base = 64: ry_conv_direct + ry_sr_post behind implicit-GEMM layers
    (8, 8, 128, 1),       # seven down layers to one pixel row
]
SMALL_FRAMES = [1, 7, 127, 128, 129]     # one below / at / above the pad multiple


def _small(ctx, monkeypatch, cfg, n):
    base, e, width, B = cfg
    d = NetDesc(2, 1, 1, base, e)
    P = synthetic_params(d, 440 + base + e, bias_std=0.05)
    sp = _sp(n, width + 1, B, seed=92 + n)
    what = 'base %d e %d width %d B %d n=%d' % (base, e, width, B, n)
    with cases.poisoned(ctx, monkeypatch):
        net = engine.Net(ctx, d, flatten_params(d, P), width=width)
        y, w = _run(ctx, monkeypatch, net, d, P, sp, 'f32', what=what)
        names = _names(net, n)
        net.close()
    print('%-46s kernels %s' % (what, sorted(names)))
    assert w['fused'] == (base == 64)
    return names


@pytest.mark.gpu
@pytest.mark.parametrize('n', SMALL_FRAMES)
@pytest.mark.parametrize('cfg', SMALL_NETS, ids=lambda c: 'x'.join(str(v) for v in c))
def test_small_predictor_walk_gpu(gpu_ctx, monkeypatch, cfg, n):
    _small(gpu_ctx, monkeypatch, cfg, n)


@pytest.mark.parametrize('n', SMALL_FRAMES)
@pytest.mark.parametrize('cfg', SMALL_NETS, ids=lambda c: 'x'.join(str(v) for v in c))
def test_small_predictor_walk_emu(emu_ctx, monkeypatch, cfg, n):
    _small(emu_ctx, monkeypatch, cfg, n)


def _small_16bit(ctx, monkeypatch, mode, n):
    """The base-64, extensive_layers = 3 predictor on the bf16 pipes: encoder c0 (ry_sr_first) and decoder c6 write both copies (the end layer reads
    fp32, the implicit GEMM the 16-bit one), the layers between them the 16-bit copy alone."""
    d = NetDesc(2, 1, 1, 64, 3)
    P = synthetic_params(d, 440 + 64 + 3, bias_std=0.05)
    sp = _sp(n, 25, 1, seed=92 + n)
    what = 'base 64 e 3 width 24 n=%d %s' % (n, mode)
    monkeypatch.setenv('RY_X3_MINM', '1')                   # every implicit-GEMM layer on the split path, whatever its row count
    try:
        with cases.poisoned(ctx, monkeypatch):
            net = engine.Net(ctx, d, flatten_params(d, P), width=24)
            net.set_dtype(mode)
            net.convert(sp)
            prof = net.profile(1, n, 1, window=True)
            assert cases.s2_reads_16bit(prof), prof
            y, w = _run(ctx, monkeypatch, net, d, P, sp, mode, prof=prof, what=what)
            net.close()
    finally:
        monkeypatch.delenv('RY_X3_MINM', raising=False)
    both = [q['layer'] for i, q in enumerate(w['layers']) if w['raw'][i][0] is not None and w['raw'][i][1] is not None]
    only16 = [q['layer'] for i, q in enumerate(w['layers']) if w['raw'][i][0] is None and w['raw'][i][1] is not None]
    print('%-46s both copies %s, 16-bit alone %s' % (what, both, only16))
    assert 'encoder/c0' in both and only16


@pytest.mark.gpu
@pytest.mark.parametrize('n', [7, 129])
@pytest.mark.parametrize('mode', ['bf16', 'bf16x3'])
def test_small_predictor_16bit_walk_gpu(gpu_ctx, monkeypatch, mode, n):
    _small_16bit(gpu_ctx, monkeypatch, mode, n)


@pytest.mark.parametrize('mode,n', [('bf16', 7), ('bf16', 129), ('bf16x3', 7)])      # (split-bf16 at 129 frames takes the emulator 14 s: on the card only)
def test_small_predictor_16bit_walk_emu(emu_ctx, monkeypatch, mode, n):
    _small_16bit(emu_ctx, monkeypatch, mode, n)


def _copied_rows(ctx, monkeypatch):
    """Copied rows at a size the emulator can run: base 64, extensive_layers = 3, width 64, 70 frames, encoder c1 / c2 without split-K (as at full size) on
    64- and 32-row tiles (RY_PLAN), so that both leave whole tile rows of their identical stretch to ry_rep_rows.  Every row against float64 -- a copy
    from the wrong row is a wrong or an unwritten row -- and the stretches bit-identical."""
    d = NetDesc(2, 1, 1, 64, 3)
    P = synthetic_params(d, 451, bias_std=0.05)
    sp = _sp(70, 65, 1, seed=72)
    monkeypatch.setenv('RY_PLAN', '1:3:1:1,2:4:1:1')
    try:
        with cases.poisoned(ctx, monkeypatch):
            net = engine.Net(ctx, d, flatten_params(d, P), width=64)
            y, w = _run(ctx, monkeypatch, net, d, P, sp, 'f32', what='base 64 e 3 width 64 n=70 RY_PLAN')
            yd, wd = _run(ctx, monkeypatch, net, d, P, sp, 'f32', discard=(20, 30), what='base 64 e 3 width 64 n=70 RY_PLAN discard (20, 30)')
            reps = {q['layer'] for q in net.profile(1, 70, 1, window=True) if q['name'] == 'ry_rep_rows'}
            net.close()
    finally:
        monkeypatch.delenv('RY_PLAN', raising=False); ctx.reload_env()
    assert reps == {'encoder/c1', 'encoder/c2'}, reps
    assert numpy.array_equal(yd[:, 20:40], y[:, 20:40])
    holes = _hole_stretches(w, 70)
    print('base 64 e 3 width 64 n=70: ry_rep_rows on %s, bit-identical stretches %s' % (sorted(reps), holes))
    assert {h[0] for h in holes} >= reps


@pytest.mark.gpu
def test_copied_rows_walk_gpu(gpu_ctx, monkeypatch):
    _copied_rows(gpu_ctx, monkeypatch)


def test_copied_rows_walk_emu(emu_ctx, monkeypatch):
    _copied_rows(emu_ctx, monkeypatch)


KERNELS_WANTED = {'ry_sr_first', 'ry_sr_last<false>', 'ry_sr_last_gather', 'ry_conv_direct', 'ry_sr_post', 'ry_pad_min_rows', 'ry_rep_rows',
                  'ry_splitk_reduce', 'ry_splitk_reduce_wide'}


@pytest.mark.gpu
def test_cases_of_this_file_meet_every_kernel_gpu(gpu_ctx, monkeypatch, syn64_params):
    """The kernel names (Net.profile of the convert window) over the predictors and modes of this file: no label of KERNELS_WANTED may be missing."""
    d2, P2 = syn64_params
    got = set()
    for base, e, width, B in SMALL_NETS:
        d = NetDesc(2, 1, 1, base, e)
        net = engine.Net(gpu_ctx, d, flatten_params(d, synthetic_params(d, 440 + base + e, bias_std=0.05)), width=width)
        net.convert(_sp(7, width + 1))
        got |= _names(net, 7)
        net.close()
    net = engine.Net(gpu_ctx, d2, flatten_params(d2, P2), width=synth.FFT_BINS - 1)
    try:
        for mode, wino in SYN64_MODES:
            monkeypatch.setenv('RY_WINOGRAD', wino); gpu_ctx.reload_env()
            net.set_dtype(mode)
            net.convert(_sp(100, synth.FFT_BINS))
            got |= _names(net, 100)
    finally:
        monkeypatch.delenv('RY_WINOGRAD', raising=False); gpu_ctx.reload_env()
        net.close()
    print('kernel names met: %s' % sorted(got))
    assert not KERNELS_WANTED - got, sorted(KERNELS_WANTED - got)


# ---- the end layer as an operator (path='last'): float64 element by element ----

# B, H, W, C: the rolling form (C = 128 as 64 + 64, W % 16 == 0) and the gather form
LAST_CASES = [(1, 1, 16, 128), (1, 3, 16, 128), (2, 5, 32, 128), (1, 9, 512, 128), (1, 4, 6, 256)]


def _last_op(ctx, monkeypatch, case):
    B, H, W_, C = case
    x, Wt, b, _ = cases.trained_like_operands(numpy.random.default_rng(71), B, H, W_, C, 1, 3, False)
    with cases.poisoned(ctx, monkeypatch):
        y = ctx.conv2d(x, Wt, b, None, stride=1, pad=1, act=None, path='last')
    r, bound = cases.ref_conv2d_f64(x, Wt, b, None, 1, 1, False, None)
    worst = cases.assert_close_elementwise(y, r, bound, F32_TOL, 'last %s' % (case,))
    print('path=last %-20s worst %.3g' % (case, worst))


@pytest.mark.gpu
@pytest.mark.parametrize('case', LAST_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_end_layer_operator_gpu(gpu_ctx, monkeypatch, case):
    _last_op(gpu_ctx, monkeypatch, case)


@pytest.mark.parametrize('case', LAST_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_end_layer_operator_emu(emu_ctx, monkeypatch, case):
    _last_op(emu_ctx, monkeypatch, case)


# ---- ry_mc2sp ----

MC2SP_CASES = [(1, 9, 513), (3, 9, 513), (300, 9, 513), (7, 60, 513)]


def _mc2sp(ctx, monkeypatch, case, floor):
    n, m, f = case
    rng = numpy.random.default_rng(73)
    scale = numpy.concatenate([synth.MC_SCALE, numpy.full(max(m - 9, 0), 0.1)])[:m]
    mc = (rng.normal(size=(n, m)) * scale).astype('f4')
    mc[n // 2] = 0.0                                            # one row of zeros: exp(0) + floor exactly
    M = sptk.mc2sp_matrix(m - 1, 0.41, 2 * (f - 1)).astype('f4')
    assert M.shape == (m, f) and (n * f) % 256 != 0
    with cases.poisoned(ctx, monkeypatch):
        sp = ctx.mc2sp(mc, M, floor)
    assert numpy.isfinite(sp).all()
    assert (sp[n // 2] == numpy.float32(1.0) + numpy.float32(floor)).all()
    z = mc.astype('f8') @ M.astype('f8')
    bound = numpy.abs(mc).astype('f8') @ numpy.abs(M).astype('f8')
    assert float(numpy.abs(z).max()) <= cases.EXP_ARG_MAX
    # (+ floor is one more float32 rounding of the sum; taking it off again in float64 is exact)
    bar = F32_TOL * bound + E + (2.0 ** -24 if floor else 0.0) * (1 + numpy.float32(floor) / numpy.exp(z))
    err = numpy.abs(numpy.log(sp.astype('f8') - numpy.float64(numpy.float32(floor))) - z) / bar
    print('ry_mc2sp %-16s floor %-6g worst |log(sp - floor) - mc M| / bar = %.3g' % (case, floor, float(err.max())))
    assert float(err.max()) <= 1.0, (case, floor, float(err.max()))


@pytest.mark.gpu
@pytest.mark.parametrize('floor', [0.0, 1e-16])
@pytest.mark.parametrize('case', MC2SP_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_mc2sp_gpu(gpu_ctx, monkeypatch, case, floor):
    _mc2sp(gpu_ctx, monkeypatch, case, floor)


@pytest.mark.parametrize('floor', [0.0, 1e-16])
@pytest.mark.parametrize('case', MC2SP_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_mc2sp_emu(emu_ctx, monkeypatch, case, floor):
    _mc2sp(emu_ctx, monkeypatch, case, floor)


def test_debug_activation_refuses_what_the_plan_does_not_have_emu(emu_ctx):
    """`ry_net_debug_activation`: nothing before the first run, no 16-bit copies in fp32 mode, no padded input of a raw forward, the end layer's
    block when it stored into the caller's; the sizes it reports are the ones it copies."""
    d = NetDesc(2, 1, 1, 64, 3)
    net = engine.Net(emu_ctx, d, flatten_params(d, synthetic_params(d, 7)), width=16)
    with pytest.raises(_lib.Ry355Error, match='no forward or convert has run'):
        net.debug_activation(0)
    net.forward(numpy.zeros((1, 16, 16), 'f4'))
    assert net.debug_activation(0).shape == (1, 16, 16, 64) and net.debug_activation(14).shape == (1, 16, 16, 64)
    for layer, kind, msg in ((-1, 0, 'no padded input'), (15, 0, "caller's block"), (3, 1, 'writes no 16-bit copy'), (16, 0, 'layer must be'), (2, 2, 'layer must be')):
        with pytest.raises(_lib.Ry355Error, match=msg):
            net.debug_activation(layer, kind)
    dims = (ctypes.c_int * 5)()
    buf = numpy.empty(10, 'f4')
    assert emu_ctx.lib.dll.ry_net_debug_activation(net.handle, 0, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes, dims) != 0
    assert b'bytes' in emu_ctx.lib.dll.ry_last_error()
    net.set_dtype('bf16x3')
    with pytest.raises(_lib.Ry355Error, match='no forward or convert has run'):
        net.debug_activation(0)
    net.close()
