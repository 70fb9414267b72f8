"""The stage-2 GEMM kernels (ry_igemm_ldsdma, ry_wino_ldsdma, ry_c2d_os) against float64, element by element, with every output and slab
buffer poisoned (RY_POISON=1): an element the launch does not write in this call is NaN, and a wrong K range or a skipped tile in a
low-magnitude region cannot hide below the largest output (the bound of cases.ref_conv2d_f64 is per element).

The emulator part (no GPU) runs case lists that take every branch of the schedule the two LDS-DMA kernels share (fill_sched, ry_tile_decode,
ry_tile_pos, ry_split_range, ry_tile_epilogue); the GPU part runs the layers of SYN-64 at the 300-frame window.  `-s` prints the worst
element-wise ratio |y - r| / bound and rel_max of every case."""
import numpy
import pytest

from conftest import rel_max
import cases

F32_TOL = cases.F32_TOL  # fp32 paths: any summation order of the same products
X3_TOL = cases.X3_TOL   # split-bf16 against the fp32-operand reference (the dropped lo * lo term and the 16-bit split)
BF16_TOL = cases.BF16_TOL  # plain bf16 against the reference on bf16-rounded operands
BF16_F32_TOL = 1e-2     # ... and against the fp32-operand reference (two operands rounded to 8 bits)


def _ids(c):
    return 'x'.join(str(v) for v in c).replace(' ', '')


def _report(what, worst, rm):
    print('%-72s worst %.3g  rel_max %.3g' % (what, worst, rm))


def _check(what, y, r, bound, tol, rel_bar):
    worst = cases.assert_close_elementwise(y, r, bound, tol, what)
    rm = rel_max(y, r)
    _report(what, worst, rm)
    assert rm < rel_bar, (what, rm)
    return worst


# ---- emulator: the schedule branches ----

def test_sched_cases_cover_every_branch():
    """Each kernel's case list takes every branch of the shared schedule: XCD grouping 0 / 1 / 2 / 4 / 8, krem 0 and not, one K unit per split,
    batch 2 on 2-D tiles, and (implicit GEMM) a ragged raster tile.  The labels come from cases.sched_of, a restatement of fill_sched."""
    for lst, extra in ((cases.SCHED_WINO_CASES, set()), (cases.SCHED_IGEMM_CASES, {'ragged raster tile'})):
        got = set()
        for c in lst:
            got |= cases.sched_branches(c)
        missing = (cases.SCHED_BRANCHES | extra) - got
        assert not missing, (lst[0][10], sorted(missing))
    assert any(cases.sched_of(c)['splits'] > 1 and cases.sched_of(c)['splits'] == cases.sched_of(c)['units'] for c in cases.SCHED_WINO_CASES)
    assert any(cases.sched_of(c)['splits'] > 1 and cases.sched_of(c)['splits'] == cases.sched_of(c)['units'] for c in cases.SCHED_IGEMM_CASES)


@pytest.mark.parametrize('case', cases.SCHED_WINO_CASES + cases.SCHED_IGEMM_CASES, ids=_ids)
def test_sched_case_against_f64_emu(emu_ctx, monkeypatch, case):
    B, H, W_, Cin, Cout, k, s, p, tr, act, path, tile, splits = case
    x, Wt, b, bn = cases.trained_like_operands(numpy.random.default_rng(43), B, H, W_, Cin, Cout, k, tr)
    with cases.poisoned(emu_ctx, monkeypatch):
        y = emu_ctx.conv2d(x, Wt, b, bn, stride=s, pad=p, transposed=tr, act=act, path=path, tile=tile, splits=splits)
    r, bound = cases.ref_conv2d_f64(x, Wt, b, bn, s, p, tr, act)
    _check('%s %s' % (_ids(case), sorted(cases.sched_branches(case))), y, r, bound, F32_TOL, 1e-5 if path == 'wino' else cases.TOL)


@pytest.mark.parametrize('case', cases.CONV1D_CASES, ids=_ids)
def test_conv1d_poisoned_emu(emu_ctx, monkeypatch, case):
    """ry_conv1d (ry_conv1d_ws + ry_materialize: GLU, the generic mode) with its split-K slabs and output poisoned: every slab element the
    materialize step sums was written by the launch, and every output element is within F32_TOL of float64 (tests/test_stage1_oracle.py: ry_c1d_os)"""
    from conftest import bn_params
    ops = cases.conv1d_operands(numpy.random.default_rng(11), case, bn_params)
    with cases.poisoned(emu_ctx, monkeypatch):
        y, r = cases.run_conv1d(emu_ctx, None, case, bn_params, operands=ops)
    assert numpy.isfinite(y).all() and rel_max(y, r) < cases.TOL
    B, L, Cin, Cout, k, s, p, d, tr, act, splits = case
    x, W, b, bn = ops
    r64, bound = cases.ref_conv1d_f64(x, None, W, b, bn, s, p, d, tr, act)
    _check('%s ry_conv1d' % _ids(case), y, r64, bound, F32_TOL, cases.TOL)


# ---- GPU: the SYN-64 layers at full size ----

def _run_twice(ctx, what, x, Wt, b, bn, **kw):
    y = ctx.conv2d(x, Wt, b, bn, **kw)
    y2 = ctx.conv2d(x, Wt, b, bn, **kw)
    assert numpy.array_equal(y, y2), (what, 'two runs differ')
    return y


IGEMM_ONLY_FULL_SIZE = [                                      # B, H, W, Cin, Cout, transposed: split-K implicit GEMM + reduce in the planner's plan
    (1, 24, 32, 512, 512, False),                             # encoder c5
    (1, 12, 16, 1024, 512, True),                             # decoder c2
]


@pytest.mark.gpu
@pytest.mark.parametrize('case', cases.WINO_FULL_SIZE + IGEMM_ONLY_FULL_SIZE, ids=_ids)
def test_stage2_gemm_full_size_against_f64_gpu(gpu_ctx, monkeypatch, case):
    """One layer of SYN-64 at the 300-frame window on trained-like operands: the Winograd form on every workgroup shape and with a forced external
    split that leaves a remainder (krem != 0), the implicit GEMM on the planner's tile and split and on one forced tile, each against float64."""
    B, H, W_, Cin, Cout, tr = case
    x, Wt, b, bn = cases.trained_like_operands(numpy.random.default_rng(61), B, H, W_, Cin, Cout, 4, tr)
    act = 'relu' if tr else 'lrelu'
    r, bound = cases.ref_conv2d_f64(x, Wt, b, bn, 2, 1, tr, act)
    kw = dict(stride=2, pad=1, transposed=tr, act=act)
    runs = []
    if case in cases.WINO_FULL_SIZE:
        npatches = (1 if tr else 4) * (Cin // 16)
        ksplit = next(q for q in (3, 5, 7) if npatches % q)
        for tile in (None, (1, 0), (2, 0)):
            runs.append(('wino', tile, 0))
        runs.append(('wino', None, ksplit))
    runs.append(('igemm', None, 0))
    runs.append(('igemm', '128x64' if tr or Cout % 128 else '96x128k2', 0))
    with cases.poisoned(gpu_ctx, monkeypatch):
        for path, tile, splits in runs:
            what = '%s %s %s split %s' % (_ids(case), path, tile, splits)
            try:
                y = _run_twice(gpu_ctx, what, x, Wt, b, bn, path=path, tile=tile, splits=splits, **kw)
            except RuntimeError as e:          # (as in test_conv2d_wino_full_size_gpu: 24 x 32 has no 16-row tile of the eight-wave shape)
                assert 'no Winograd plan' in str(e) and tile == (2, 0) and (H if tr else H // 2) % 16, (what, e)
                continue
            _check(what, y, r, bound, F32_TOL, 1e-5 if path == 'wino' else cases.TOL)


@pytest.mark.gpu
@pytest.mark.parametrize('case', cases.X3_FULL_SIZE + [(1, 24, 32, 1024, 512, 4, 2, 1, True, 'relu', None, 0),       # decoder c3
                                                       (1, 192, 256, 128, 256, 4, 2, 1, False, 'lrelu', None, 0)],   # encoder c2
                         ids=_ids)
def test_stage2_bf16_full_size_against_f64_gpu(gpu_ctx, monkeypatch, case):
    """The bf16-operand implicit GEMM at full size: split-bf16 against the fp32-operand reference; plain bf16 against the reference on bf16-rounded
    operands (exact products, fp32 accumulation) and against the fp32-operand one."""
    B, H, W_, Cin, Cout, k, s, p, tr, act, tile, splits = case
    x, Wt, b, bn = cases.trained_like_operands(numpy.random.default_rng(62), B, H, W_, Cin, Cout, k, tr)
    kw = dict(stride=s, pad=p, transposed=tr, act=act, tile=tile, splits=splits)
    r, bound = cases.ref_conv2d_f64(x, Wt, b, bn, s, p, tr, act)
    with cases.poisoned(gpu_ctx, monkeypatch):
        y3 = _run_twice(gpu_ctx, 'x3', x, Wt, b, bn, path='igemm_x3', **kw)
        y16 = _run_twice(gpu_ctx, 'bf16', x, Wt, b, bn, path='igemm_bf16', **kw)
    _check('%s igemm_x3' % _ids(case), y3, r, bound, X3_TOL, 2e-5)
    _check('%s igemm_bf16 vs fp32 operands' % _ids(case), y16, r, bound, BF16_F32_TOL, 2e-2)
    del r, bound
    r16, bound16 = cases.ref_conv2d_f64(cases.bf16_round(x), cases.bf16_round(Wt), b, bn, s, p, tr, act)
    _check('%s igemm_bf16 vs bf16 operands' % _ids(case), y16, r16, bound16, BF16_TOL, 1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize('case', cases.OS_FULL_SIZE, ids=_ids)
def test_stage2_os_full_size_against_f64_gpu(gpu_ctx, monkeypatch, case):
    """The weight-streaming layers at the bottom of SYN-64 (ry_c2d_os, planner's slice) against float64."""
    B, H, W_, Cin, Cout, k, s, p, tr, act, path, tile, splits = case
    x, Wt, b, bn = cases.trained_like_operands(numpy.random.default_rng(63), B, H, W_, Cin, Cout, k, tr)
    r, bound = cases.ref_conv2d_f64(x, Wt, b, bn, s, p, tr, act)
    with cases.poisoned(gpu_ctx, monkeypatch):
        y = _run_twice(gpu_ctx, _ids(case), x, Wt, b, bn, stride=s, pad=p, transposed=tr, act=act, path='os', tile=tile)
    _check('%s os' % _ids(case), y, r, bound, F32_TOL, cases.TOL)
