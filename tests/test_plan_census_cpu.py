"""The plan census on what the emulator can hold (tests/plan_census_cases.py; the sweep itself: tests/test_plan_census_gpu.py): the records of
`ry_net_debug_plan` are legal and the same every time, the cover selection is deterministic and complete, `cases.s2_walk(layers=, bands=)` gives the
numbers of the full walk on the layers it holds."""
import ctypes

import numpy
import pytest

import cases
import plan_census_cases as pc
from realtime_yukarin_amd import _lib, engine, synth
from realtime_yukarin_amd.netspec import NetDesc
from realtime_yukarin_amd.weights import flatten_params, synthetic_params
from test_stage2_graph_oracle import SMALL_FRAMES, SMALL_NETS, SYN64_MODES

E, E_LOG = cases.s2_tolerances()


def test_modes_are_the_walk_tests_modes():
    assert pc.MODES == SYN64_MODES and len(pc.MODE_IDS) == len(pc.MODES)


def test_sweep_domain_is_the_issues():
    pts = pc.sweep_domain()
    conv = [p for p in pts if p[2]]
    assert sorted({pc.padded(p) for p in conv}) == list(range(128, 2049, 128)) and all(p[0] == 1 and pc.padded(p) - p[1] == 28 for p in conv)
    assert {p[3] for p in conv} == {(0, 0), (20, 20)} and len(conv) == 32 and conv[0][1] == 100
    assert sorted((p[0], p[1]) for p in pts if not p[2]) == sorted((B, T) for B in (2, 3, 4, 8) for T in (128, 256, 384, 512))
    assert all(p in pts for p in [(1, 100, True, (0, 0)), (1, 100, True, (20, 20))])


def _legal(net, desc, P, mode, points, what):
    specs = cases.s2_layers(desc)
    ch = pc.layer_channels(P, specs)
    table, records = pc.census(net, mode, points)
    for p, recs in records.items():
        for r, spec, (cin, cout) in zip(recs, specs, ch):
            pc.check_legal(r, spec, cin, cout, (what, p))
    return table, records


@pytest.mark.parametrize('mode', range(4), ids=pc.MODE_IDS)
def test_syn64_census_is_legal_and_deterministic_emu(emu_ctx, monkeypatch, mode):
    """SYN-64 at T <= 256, B <= 2: every record legal; the census, the walked set and the cover the same from a second handle; the cover leaves no
    signature out."""
    d2, P2 = synth.model_params('SYN-64')[1]
    pts = pc.emu_domain() + [(1, 130, True, (0, 0))]
    monkeypatch.setenv('RY_WINOGRAD', pc.MODES[mode][1]); emu_ctx.reload_env()
    try:
        got = []
        for _ in range(2):
            net = engine.Net(emu_ctx, d2, flatten_params(d2, P2), width=synth.FFT_BINS - 1)
            net.set_dtype(pc.MODES[mode][0])
            table, records = _legal(net, d2, P2, mode, pts if not got else list(reversed(pts)), 'SYN-64 ' + pc.MODE_IDS[mode])
            net.close()
            walked = pc.walked_points(table)
            got.append((table, records, walked, pc.greedy_cover(table, walked)))
    finally:
        monkeypatch.delenv('RY_WINOGRAD', raising=False); emu_ctx.reload_env()
    assert got[0] == got[1]
    table, _, walked, cover = got[0]
    every = {s for sigs in table.values() for s in sigs}
    met = {s for p in walked for s in table[p]} | {table[p][i] for p, new in cover for i in new}
    assert met == every
    assert all(s[1] == mode for s in every)
    if pc.MODES[mode] == ('f32', '1'):
        assert any(s[3] == 'wino' for s in every)
    if pc.MODES[mode][0] != 'f32':
        assert any(s[3] == 'igemm16' for s in every)
    assert any(s[-2] != 'none' for s in every) and any(s[-1] != 'none' for s in every), 'no crop or no hole in the census'


@pytest.mark.parametrize('cfg', SMALL_NETS, ids=lambda c: 'x'.join(str(v) for v in c))
def test_small_predictor_census_is_legal_emu(emu_ctx, cfg):
    base, e, width, B = cfg
    d = NetDesc(2, 1, 1, base, e)
    P = synthetic_params(d, 440 + base + e, bias_std=0.05)
    net = engine.Net(emu_ctx, d, flatten_params(d, P), width=width)
    pts = [(B, n, True, disc) for n in SMALL_FRAMES for disc in ((0, 0), (2, 3))] + [(B, 128, False, (0, 0))]
    t1, r1 = _legal(net, d, P, 0, pts, str(cfg))
    net.set_dtype('f32')
    t2, r2 = _legal(net, d, P, 0, pts, str(cfg))
    net.close()
    assert (t1, r1) == (t2, r2)


def test_greedy_cover_on_a_synthetic_table():
    """Smallest B x T first; a point with nothing new is not chosen; walked signatures are not covered again; every other signature belongs to exactly
    one chosen point, as new there."""
    P = lambda B, n, w=True, d=(0, 0): (B, n, w, d)
    sig = lambda *names: [(i, 0, False, nm) for i, nm in enumerate(names)]
    table = {P(1, 100): sig('a', 'b', 'c'), P(1, 228): sig('a', 'b', 'd'), P(1, 356): sig('a', 'e', 'd'), P(1, 484): sig('a', 'b', 'c'),
             P(2, 128, False): sig('a', 'f', 'd'), P(1, 100, True, (20, 20)): sig('a', 'b', 'g')}
    cover = pc.greedy_cover(table, [P(1, 100)])
    # 2 x 128 and 1 x 256 rows tie: the shorter window goes first and takes 'd' as well
    assert cover == [(P(1, 100, True, (20, 20)), [2]), (P(2, 128, False), [1, 2]), (P(1, 356), [1])]
    assert pc.greedy_cover(dict(reversed(list(table.items()))), [P(1, 100)]) == cover
    assert pc.greedy_cover(table, list(table)) == []
    everything = pc.greedy_cover(table, [])
    assert [p for p, _ in everything][0] == P(1, 100) and sorted(table[p][i][3] for p, new in everything for i in new) == list('abcdefg')


def test_signature_keeps_row_ranges_relative():
    rec = dict(layer=12, path=8, tile=0, splits=1, kgroups=0, wino_cfg=1, wino_mbw=2, os2=(0, 0, 0, 0), reads16=0, writes32=1, writes16=0, patch=0, reduce=0, last_exp=0,
               rows_out=256, grid_rows=128, grid_cols=64, tile_rows=8, tile_cols=32, out_lo=16, out_n=208, crop_lo=8, crop_n=104, hole_lo=0, hole_n=0)
    big = dict(rec, rows_out=512, grid_rows=256, out_n=464, crop_n=232)
    assert pc.signature(rec, 0, False) == pc.signature(big, 0, False) and pc.signature(rec, 0, False)[-2] == (1, 2)
    assert pc.signature(dict(rec, crop_n=96, out_n=192), 0, False) != pc.signature(rec, 0, False)          # one tile row fewer
    assert pc.signature(dict(rec, splits=2, reduce=1), 0, False) != pc.signature(rec, 0, False)
    assert pc.signature(dict(rec, crop_lo=9), 0, False)[-2][0] == '1.1'
    with pytest.raises(AssertionError):
        pc.check_legal(dict(rec, crop_lo=9, out_lo=18), cases.s2_layers(NetDesc(2, 1, 1, 64, 8))[12], 1024, 256)


def test_band_rows_hold_the_edges():
    rec = dict(layer=12, rows_out=512, grid_rows=256, tile_rows=8, out_lo=32, out_n=400, hole_lo=0, hole_n=0)
    bands = pc.band_rows(rec, (40, 425), 3)
    rows = {r for a, b in bands for r in range(a, b)}
    assert bands == pc.band_rows(rec, (40, 425), 3) and all(a % 16 == 0 and (b % 16 == 0) for a, b in bands)
    for e in (0, 31, 511, 480, 32, 31, 431, 432, 39, 40, 424, 425):
        assert e in rows, e
    assert 32 * 16 / 3 <= len(rows) < 512
    rec = dict(layer=1, rows_out=128, grid_rows=128, tile_rows=8, out_lo=0, out_n=128, hole_lo=56, hole_n=64)
    rows = {r for a, b in pc.band_rows(rec, (0, 128), 4) for r in range(a, b)}
    assert {55, 56, 119, 120} <= rows


@pytest.mark.parametrize('tr,k,s,p', [(False, 4, 2, 1), (True, 4, 2, 1), (False, 3, 1, 1), (False, 1, 1, 0)])
def test_band_reference_is_the_rows_of_the_whole_reference(tr, k, s, p):
    rng = numpy.random.default_rng(17)
    B, H, W_, Ca, Cb, Cout = 2, 12, 6, 3, 2, 5
    xa, xb = rng.normal(size=(B, H, W_, Ca)), rng.normal(size=(B, H, W_, Cb))
    Wt = rng.normal(size=(Ca + Cb, Cout, k, k) if tr else (Cout, Ca + Cb, k, k))
    b = rng.normal(size=Cout)
    spec = dict(name='t', tr=tr, k=k, s=s, p=p, act='lrelu')
    r, bound = cases.ref_conv2d_f64(numpy.concatenate([xa, xb], axis=3), Wt, b, None, s, p, tr, 'lrelu')
    Ho = r.shape[1]
    reads = []
    def rows(lo, hi):
        reads.append((lo, hi))
        return [xa[:, lo:hi], xb[:, lo:hi]]
    for a_, b_ in [(0, 1), (0, Ho), (Ho - 1, Ho), (1, 3), (Ho // 2, Ho // 2 + 3)]:
        rr, bd = cases.s2_band_reference(spec, rows, Wt, b, None, a_, b_, H)
        assert rr.shape == r[:, a_:b_].shape
        assert numpy.allclose(rr, r[:, a_:b_], rtol=0, atol=1e-13 * bound.max()) and numpy.allclose(bd, bound[:, a_:b_], rtol=1e-13)
        assert reads[-1] == cases.s2_rows_read(spec, a_, b_, H)           # only the source rows the stencil reads


def test_layers_walk_gives_the_full_walks_numbers_emu(emu_ctx, monkeypatch):
    """base 64, extensive_layers 3, 129 frames: the walk restricted to two layers holds exactly those, with the worst ratios of the full walk, and gives
    every other layer the finiteness / NaN-row rule; on bands, the worst ratio is the full walk's over those rows."""
    base, e, width, B = SMALL_NETS[3]
    d = NetDesc(2, 1, 1, base, e)
    P = synthetic_params(d, 440 + base + e, bias_std=0.05)
    n = 129
    with cases.poisoned(emu_ctx, monkeypatch):
        net = engine.Net(emu_ctx, d, flatten_params(d, P), width=width)
        full = pc.run_point(net, d, P, 0, (B, n, True, (3, 5)), range(16), E, E_LOG)
        part = pc.run_point(net, d, P, 0, (B, n, True, (3, 5)), [2, 13], E, E_LOG)
        band = pc.run_point(net, d, P, 0, (B, n, True, (3, 5)), [2, 13], E, E_LOG, band_from=0)
        net.close()
    assert full['met'] == set(range(16)) and part['met'] == {2, 13, 15} and band['met'] == {2, 13, 15}
    assert numpy.array_equal(full['y'], part['y']) and full['signatures'] == part['signatures']
    for i, (qf, qp, qb) in enumerate(zip(full['walk']['layers'], part['walk']['layers'], band['walk']['layers'])):
        assert (qp['nan32'], qp['nan16'], qp['need']) == (qf['nan32'], qf['nan16'], qf['need'])
        if i in (2, 13):
            assert qp['held'] and qp['worst'] == qf['worst'] and qp['worst'] is not None and qp['banded'] is None
            assert qb['banded'] and 0 < qb['worst'] <= qf['worst'] * (1 + 1e-9)
        else:
            assert not qp['held'] and qp['worst'] is None and qp['worst16'] is None
    # a wrong element in a layer that is held fails the restricted walk; one in a layer that is not held does not reach a float64 comparison
    w = part['walk']
    bad = {i: (None if o32 is None else o32.copy(), o16) for i, (o32, o16) in w['raw'].items()}
    a, b = w['need'][13]
    bad[13][0][0, a, 0, 0] += 1.0

    class Fake(object):
        def debug_activation(self, layer, kind=0):
            o = w['x_in'] if layer < 0 else bad[layer][kind]
            if o is None:
                raise _lib.Ry355Error('writes no such copy')
            return o
    with pytest.raises(AssertionError, match='decoder/c5'):
        cases.s2_walk(Fake(), d, P, n, part['y'], (3, 5), layers={2, 13})
    with pytest.raises(AssertionError, match='decoder/c5'):
        cases.s2_walk(Fake(), d, P, n, part['y'], (3, 5), layers={13}, bands={13: [(a, a + 1)]})
    cases.s2_walk(Fake(), d, P, n, part['y'], (3, 5), layers={2})


def test_debug_plan_builds_the_plan_and_refuses_bad_arguments_emu(emu_ctx):
    d = NetDesc(2, 1, 1, 64, 3)
    net = engine.Net(emu_ctx, d, flatten_params(d, synthetic_params(d, 7)), width=16)
    recs = net.debug_plan(1, 100, window=True, discard=(20, 20))
    assert len(recs) == 16 and recs[15]['rows_out'] == 128 and (recs[15]['out_lo'], recs[15]['out_n']) in ((20, 60), (0, 128))
    with pytest.raises(_lib.Ry355Error, match='no forward or convert has run'):       # nothing ran: the entry enqueues nothing and remembers no plan
        net.debug_activation(0)
    assert net.debug_plan(1, 100, window=True) != recs or recs[15]['out_n'] == 128
    assert net.debug_plan(1, 100, window=True, discard=(20, 20)) == recs
    y = net.convert(numpy.ones((1, 100, 17), 'f4'))                       # a convert after it is not disturbed by the discards it was asked about
    assert numpy.isfinite(y).all() and y[:, :20].all()
    for args, msg in (((1, 100, 2, 0, 0), 'window must be'), ((0, 100, 1, 0, 0), 'positive'), ((1, 128, 0, 1, 0), 'raw forward has none'), ((1, 100, 1, -1, 0), 'negative')):
        buf = (_lib.RyPlanRecord * 16)()
        k = ctypes.c_int()
        assert emu_ctx.lib.dll.ry_net_debug_plan(net.handle, *args, buf, 16, ctypes.byref(k)) != 0 and msg.encode() in emu_ctx.lib.dll.ry_last_error()
    buf = (_lib.RyPlanRecord * 16)()
    k = ctypes.c_int()
    assert emu_ctx.lib.dll.ry_net_debug_plan(net.handle, 1, 100, 1, 0, 0, buf, 15, ctypes.byref(k)) != 0 and k.value == 0
    net.close()
    d1 = NetDesc(1, 9, 9, 8, 8)
    net1 = engine.Net(emu_ctx, d1, flatten_params(d1, synthetic_params(d1, 7)))
    with pytest.raises(_lib.Ry355Error, match='stage-2'):
        net1.debug_plan(1, 100, window=True)
    net1.close()
