"""The stage-1 kernels against float64, element by element, with every output buffer poisoned (RY_POISON=1): ry_c1d_os, the output-stationary
kernel of the predictors, through its single operator (Context.conv1d_os) on every instantiation and forced slice, and the whole stage-1 convert.

ry_c1d_os has exact properties the suite asserts bit for bit: for one mode and input-channel count every output goes through the same arithmetic
whatever the slice, the source form or the pad form (each lane runs the same FMA chain over its channel sets, RyReduceScatter64 uses the same
butterfly order for every sum count, the ci waves are summed in a fixed order), and the windows of a batch do not interact.

The emulator part (no GPU) runs case lists that reach all 18 instantiations and every loop of the kernel (cases.os1_branches); the GPU part runs
every SYN-64 stage-1 layer at its 300-, 1000- and 2048-frame shapes, shapes derived from netspec.  `-s` prints the worst element-wise ratio
|y - r| / bound and rel_max of every case."""
import numpy
import pytest

from conftest import rel_max
import cases

F32_TOL = cases.F32_TOL  # fp32: any summation order of the same products
SLICES = ((4, 8), (4, 4), (2, 8), (2, 4))


def _ids(c):
    return 'x'.join(str(v) for v in c).replace(' ', '')


def _check(what, y, r, bound):
    worst = cases.assert_close_elementwise(y, r, bound, F32_TOL, what)
    rm = rel_max(y, r)
    print('%-100s worst %.3g  rel_max %.3g' % (what, worst, rm))
    assert rm < cases.TOL, (what, rm)
    return worst


def _operands(case, seed, trained=False):
    B, L, Ca, Cb, Cout, k, s, p, tr, act, tile, n_real, keep = case
    return cases.stage1_operands(numpy.random.default_rng(seed), B, L, Ca, Cb, Cout, k, tr, trained=trained)


def _run(ctx, case, xa, xb, W, b, bn, tile='case'):
    """the case on ry_conv1d_os; a fused-pad case hands over its real rows only"""
    B, L, Ca, Cb, Cout, k, s, p, tr, act, t, n_real, keep = case
    return ctx.conv1d_os(xa[:, :n_real] if n_real else xa, W, b, bn, stride=s, pad=p, transposed=tr, act=act, xb=xb,
                         tile=t if tile == 'case' else tile, pad_to=L if n_real else 0, keep=keep)


def _ref(case, xa, xb, W, b, bn):
    B, L, Ca, Cb, Cout, k, s, p, tr, act, tile, n_real, keep = case
    return cases.ref_conv1d_f64(xa, xb, W, b, bn, s, p, 1, tr, act, n_real=n_real, keep=keep)


def _slices(tr, Ca, Cb):
    """every slice that has an instantiation for this layer"""
    if Cb and Ca % 64:
        return [(2, 4)]
    return [t for t in SLICES if not (tr and t == (4, 8))]


# ---- emulator: every instantiation and loop of ry_c1d_os ----

def test_os1_cases_cover_every_branch():
    """The forced-slice lists reach all 18 instantiations <MODE,CB,TP,PADMIN,USRC>, kt 1 / 2 / 4, the quad / pair / single channel-set loops and a
    ci wave without a channel set, ragged Cout / Ctot / last position tile, batch 2, keep < Lout, the U-Net's edge lengths, every stride-1 k / pad, and
    both two-source forms (labels: cases.os1_branches, a restatement of the kernel's loops)."""
    got = set()
    for c in cases.OS1_CASES + cases.OS1_PAD_CASES:
        got |= cases.os1_branches(c)
    assert len(cases.OS1_INSTANTIATIONS) == 18
    missing = cases.OS1_BRANCHES - got
    assert not missing, sorted(missing)
    print('\n'.join(sorted(cases.OS1_INSTANTIATIONS)))
    pads = {(c[11], c[2]) for c in cases.OS1_PAD_CASES}
    assert {n for n, _ in pads} >= {1, 2, 3, 63, 64, 65, 300} and {ca for _, ca in pads} >= {1, 9, 64}


@pytest.mark.parametrize('case', cases.OS1_CASES + cases.OS1_PAD_CASES, ids=_ids)
def test_os1_case_against_f64_emu(emu_ctx, monkeypatch, case):
    ops = _operands(case, 71)
    with cases.poisoned(emu_ctx, monkeypatch):
        y = _run(emu_ctx, case, *ops)
    r, bound = _ref(case, *ops)
    _check('%s %s' % (_ids(case), cases.os1_of(case)['inst']), y, r, bound)


# B, L, Ca, Cb, Cout, k, stride, pad, transposed, act, n_real, keep: one shape on the planner's slice and on every other one
OS1_SLICE_SHAPES = [
    (2, 40, 65, 0, 10, 4, 2, 1, False, 'lrelu', 0, 0),
    (1, 11, 523, 0, 9, 3, 1, 1, False, 'lrelu', 0, 0),
    (1, 24, 64, 64, 9, 3, 1, 1, False, None, 0, 21),
    (1, 9, 128, 64, 12, 4, 2, 1, True, 'relu', 0, 0),
    (1, 5, 512, 512, 6, 4, 2, 1, True, 'relu', 0, 0),
    (2, 128, 9, 0, 16, 3, 1, 1, False, 'lrelu', 37, 0),
]


def _case(shape, tile):
    B, L, Ca, Cb, Cout, k, s, p, tr, act, n_real, keep = shape
    return (B, L, Ca, Cb, Cout, k, s, p, tr, act, tile, n_real, keep)


def _every_slice(ctx, shape, ops):
    """{slice: output} over the planner's pick (None) and every slice with an instantiation"""
    tr, Ca, Cb = shape[8], shape[2], shape[3]
    return {t: _run(ctx, _case(shape, t), *ops) for t in [None] + _slices(tr, Ca, Cb)}


@pytest.mark.parametrize('shape', OS1_SLICE_SHAPES, ids=_ids)
def test_os1_every_slice_is_bit_identical_emu(emu_ctx, monkeypatch, shape):
    ops = _operands(_case(shape, None), 72)
    with cases.poisoned(emu_ctx, monkeypatch):
        ys = _every_slice(emu_ctx, shape, ops)
    r, bound = _ref(_case(shape, None), *ops)
    _check('%s planner slice' % _ids(shape), ys[None], r, bound)
    for t, y in ys.items():
        assert numpy.array_equal(y, ys[None]), (shape, t, 'differs from the planner slice')


# B, L, Ca, Cb, Cout, k, stride, pad, transposed, act: two sources against their concatenation handed over as one
OS1_SPLIT_SHAPES = [
    (1, 30, 40, 25, 9, 3, 1, 1, False, None),        # split inside a wave: the per-lane form against the single-source 2x4 launch
    (2, 20, 40, 30, 12, 4, 2, 1, False, 'lrelu'),
    (1, 9, 30, 35, 7, 4, 2, 1, True, 'relu'),
    (1, 24, 64, 64, 9, 3, 1, 1, False, None),         # on a wave boundary (every slice)
    (1, 7, 128, 64, 13, 4, 2, 1, True, 'relu'),
]


@pytest.mark.parametrize('shape', OS1_SPLIT_SHAPES, ids=_ids)
def test_os1_split_sources_equal_one_source_emu(emu_ctx, monkeypatch, shape):
    B, L, Ca, Cb, Cout, k, s, p, tr, act = shape
    xa, xb, W, b, bn = cases.stage1_operands(numpy.random.default_rng(73), B, L, Ca, Cb, Cout, k, tr, trained=False)
    xc = numpy.ascontiguousarray(numpy.concatenate([xa, xb], axis=2))
    kw = dict(stride=s, pad=p, transposed=tr, act=act)
    with cases.poisoned(emu_ctx, monkeypatch):
        for t in _slices(tr, Ca, Cb):
            y2 = emu_ctx.conv1d_os(xa, W, b, bn, xb=xb, tile=t, **kw)
            y1 = emu_ctx.conv1d_os(xc, W, b, bn, tile=t, **kw)
            assert numpy.array_equal(y2, y1), (shape, t)
    r, bound = cases.ref_conv1d_f64(xa, xb, W, b, bn, s, p, 1, tr, act)
    _check('%s two sources' % _ids(shape), y2, r, bound)


@pytest.mark.parametrize('case', cases.OS1_PAD_CASES, ids=_ids)
def test_os1_fused_pad_equals_host_padded_input_emu(emu_ctx, monkeypatch, case):
    """The PADMIN instantiation on n_real rows against the plain one on the same rows padded on the host with their float32 column minimum"""
    B, L, Ca, Cb, Cout, k, s, p, tr, act, tile, n_real, keep = case
    xa, xb, W, b, bn = _operands(case, 74)
    xp = xa.copy()
    xp[:, n_real:] = xa[:, :n_real].min(axis=1, keepdims=True)
    with cases.poisoned(emu_ctx, monkeypatch):
        yf = _run(emu_ctx, case, xa, xb, W, b, bn)
        yh = emu_ctx.conv1d_os(xp, W, b, bn, stride=s, pad=p, act=act, tile=tile)
    assert numpy.array_equal(yf, yh), case


@pytest.mark.parametrize('case', [c for c in cases.OS1_CASES + cases.OS1_PAD_CASES if c[0] == 2], ids=_ids)
def test_os1_batch_element_equals_lone_window_emu(emu_ctx, monkeypatch, case):
    xa, xb, W, b, bn = _operands(case, 75)
    with cases.poisoned(emu_ctx, monkeypatch):
        y = _run(emu_ctx, case, xa, xb, W, b, bn)
        for i in range(case[0]):
            one = (1,) + case[1:]
            yi = _run(emu_ctx, one, xa[i:i + 1], None if xb is None else xb[i:i + 1], W, b, bn)
            assert numpy.array_equal(yi[0], y[i]), (case, i)


def test_os1_refuses_what_it_cannot_run_emu(emu_ctx):
    """Shapes without an instantiation are errors, not crashes: GLU, the generic mode, k > 4, a 4x8 deconvolution, a non-2x4 slice on sources
    that split inside a wave, a fused pad on a layer that is not stride 1 or reads more than 64 channels or two sources, an unknown slice"""
    from realtime_yukarin_amd._lib import Ry355Error
    rng = numpy.random.default_rng(76)
    x = rng.normal(size=(1, 16, 40)).astype('f4'); x2 = rng.normal(size=(1, 16, 25)).astype('f4')
    W = lambda co, ci, k: rng.normal(0, 0.1, size=(co, ci, k)).astype('f4')
    bad = [
        (dict(xa=x, W=W(8, 40, 3), pad=1, act='glu'), 'without GLU'),
        (dict(xa=x, W=W(8, 40, 4), stride=3, pad=1), 'k4 s2 p1'),
        (dict(xa=x, W=W(8, 40, 4), stride=2, pad=2), 'k4 s2 p1'),
        (dict(xa=x, W=W(8, 40, 5), pad=2), 'k <= 4'),
        (dict(xa=x, W=rng.normal(0, 0.1, size=(40, 8, 4)).astype('f4'), stride=2, pad=1, transposed=True, tile=(4, 8)), 'no ry_c1d_os instantiation'),
        (dict(xa=x, xb=x2, W=W(8, 65, 3), pad=1, tile=(4, 4)), '2x4 slice only'),
        (dict(xa=x, W=W(8, 40, 3), pad=1, tile=(3, 8)), 'no ry_c1d_os instantiation'),
        (dict(xa=x[:, :10], W=W(8, 40, 4), stride=2, pad=1, pad_to=16), 'fused pad'),
        (dict(xa=rng.normal(size=(1, 10, 65)).astype('f4'), W=W(8, 65, 3), pad=1, pad_to=16), 'fused pad'),
        (dict(xa=x[:, :10], xb=x2, W=W(8, 65, 3), pad=1, pad_to=16), 'fused pad'),
        (dict(xa=x, W=W(8, 40, 3), pad=1, keep=17), 'keep'),
    ]
    for kw, msg in bad:
        with pytest.raises(Ry355Error) as e:
            emu_ctx.conv1d_os(**kw)
        assert msg in str(e.value), (sorted(kw), str(e.value))
    emu_ctx.conv1d_os(x, W(8, 40, 3), pad=1)                          # and the context is still usable


def test_stage1_convert_poisoned_emu(emu_ctx, monkeypatch):
    """A small stage-1 predictor (base 8, 523-channel input: four ci waves in encoder c0, the separate pad node) and the SYN-64 shape of the fused
    pad (base 8, 9 channels) with every plan buffer poisoned: no NaN, the same bits as without poison"""
    from realtime_yukarin_amd import engine
    from realtime_yukarin_amd.netspec import NetDesc
    from realtime_yukarin_amd.weights import flatten_params, synthetic_params
    from oracle import unet
    for cin, frames in ((9, (1, 127, 128, 130)), (523, (37,))):
        d = NetDesc(1, cin, 9, 8, 8)
        P = synthetic_params(d, 411, bias_std=0.05)
        flat = flatten_params(d, P)
        xs = {n: numpy.random.default_rng(15 + n).normal(size=(n, cin)).astype('f4') for n in frames}
        net = engine.Net(emu_ctx, d, flat)
        clean = {n: net.convert(x) for n, x in xs.items()}
        net.close()
        with cases.poisoned(emu_ctx, monkeypatch):
            net = engine.Net(emu_ctx, d, flat)
            for n, x in xs.items():
                y = net.convert(x)
                assert not numpy.isnan(y).any() and numpy.array_equal(y, clean[n]), (cin, n)
                assert rel_max(y, unet.stage1_convert_core(x, P)) < cases.TOL
            net.close()


# ---- GPU: every SYN-64 stage-1 layer at full size ----

STAGE1_FRAMES = (300, 1000, 2048)


@pytest.mark.gpu
@pytest.mark.parametrize('frames', STAGE1_FRAMES)
@pytest.mark.parametrize('layer', range(16))
def test_syn64_stage1_layer_against_f64_gpu(gpu_ctx, monkeypatch, frames, layer):
    """One SYN-64 stage-1 layer at the window of `frames` on trained-like operands (encoder c0: the fused pad on signed features; decoder c1 .. c7:
    two sources; c7: keep = frames), on the planner's slice and on every other slice: each against float64 under poison, two runs of one slice
    with identical bits, every slice with the planner's bits"""
    case, name = cases.syn64_stage1_layers(frames)[layer]
    B, L, Ca, Cb, Cout, k, s, p, tr, act, tile, n_real, keep = case
    xa, xb, W, b, bn = _operands(case, 80 + layer, trained=layer != 0)
    r, bound = _ref(case, xa, xb, W, b, bn)
    ys = {}
    with cases.poisoned(gpu_ctx, monkeypatch):
        for t in [None] + _slices(tr, Ca, Cb):
            y = _run(gpu_ctx, case, xa, xb, W, b, bn, tile=t)
            assert numpy.array_equal(y, _run(gpu_ctx, case, xa, xb, W, b, bn, tile=t)), (name, frames, t, 'two runs differ')
            _check('%s %d frames slice %s' % (name, frames, t or 'planner'), y, r, bound)
            ys[t] = y
    for t, y in ys.items():
        assert numpy.array_equal(y, ys[None]), (name, frames, t, 'differs from the planner slice')


@pytest.mark.gpu
@pytest.mark.parametrize('cin,n_frames', [(9, 1), (9, 127), (9, 128), (9, 300), (9, 2048), (9, 2049), (523, 300)])
def test_syn64_stage1_convert_poisoned_gpu(gpu_ctx, monkeypatch, cin, n_frames):
    """The whole stage-1 convert with every plan buffer poisoned (2048 frames: the last fused pad; 2049: the separate ry_pad_min_rows node; 523
    channels: the separate node at 300): no NaN, the unpoisoned bits, and the rel_max bar against the torch oracle"""
    from realtime_yukarin_amd import engine, synth
    from realtime_yukarin_amd.weights import flatten_params
    from oracle import torch_ref
    (d1, P1), _ = synth.model_params('SYN-64', stage1_in=cin)
    flat = flatten_params(d1, P1)
    x = synth.stage1_input(n_frames, stress=cin != synth.MC_DIMS)[0]
    net = engine.Net(gpu_ctx, d1, flat)
    clean = net.convert(x)
    net.close()
    with cases.poisoned(gpu_ctx, monkeypatch):
        net = engine.Net(gpu_ctx, d1, flat)
        y = net.convert(x)
        net.close()
    assert not numpy.isnan(y).any() and numpy.array_equal(y, clean), (cin, n_frames)
    assert rel_max(y, torch_ref.stage1_convert_core(torch_ref.TorchUNet(P1), x)) < cases.TOL
