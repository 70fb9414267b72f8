"""Every launch plan the stage-2 planner emits over the sweep domain (tests/plan_census_cases.py: one window of T - 28 frames for T = 128 .. 2048, whole
and with discard (20, 20); the raw forward of 2, 3, 4, 8 windows at T = 128 .. 512) is held to float64 on the card, per mode of SYN64_MODES.

The census (`engine.Net.debug_plan`, no launch) gives every point's per-layer signatures.  Those of the windows test_syn64_layer_walk_gpu walks are taken
off; the rest is covered greedily, smallest B x T first, and at each cover point the convert / forward runs on a fresh poisoned plan and `cases.s2_walk`
holds the layers whose signature is new there to float64 on the device's own sources (cases.F32_TOL / BF16_TOL / X3_TOL times the element's bound, E /
E_log at the fused end and the pad node, needed rows finite, NaN rows not needed, 16-bit copies the roundings of their fp32 twins, copied rows
bit-identical), every other layer to the finiteness / NaN-row rule.  From 640 padded rows up a new layer is held on row bands (plan_census_cases.band_rows:
the first and last two tile rows, both sides of every boundary of its record, a seeded third of the rest).  A batch's windows are bit-equal to the
windows run alone on every layer whose signature is the B = 1 plan's.  The closing assertion: walked + covered signatures = the census.

`-s` prints the census size, the cover and, per point, the wall time and the worst ratio to the bar of every layer held (profiles/r27/plan_census_pytest_gpu.txt; the census itself:
profiles/r27/plan_census.txt)."""
import numpy
import pytest

import cases
import plan_census_cases as pc
from realtime_yukarin_amd import engine, synth
from realtime_yukarin_amd.weights import flatten_params
from test_stage2_graph_oracle import SYN64_MODES

E, E_LOG = cases.s2_tolerances()

# Points that failed once stay here by name, next to the computed cover: (mode index, (B, frames, window, discard), layers)
NAMED_POINTS = []


@pytest.fixture(scope='module')
def syn64_params():
    return synth.model_params('SYN-64')[1]


@pytest.mark.gpu
@pytest.mark.parametrize('mode', range(4), ids=pc.MODE_IDS)
def test_every_plan_signature_is_held_to_float64_gpu(gpu_ctx, monkeypatch, syn64_params, mode):
    assert pc.MODES == SYN64_MODES
    d2, P2 = syn64_params
    dtype, wino = pc.MODES[mode]
    specs = cases.s2_layers(d2)
    ch = pc.layer_channels(P2, specs)
    monkeypatch.setenv('RY_WINOGRAD', wino)
    try:
        with cases.poisoned(gpu_ctx, monkeypatch):
            net = engine.Net(gpu_ctx, d2, flatten_params(d2, P2), width=synth.FFT_BINS - 1)
            net.set_dtype(dtype)
            domain = pc.sweep_domain() + [(1, 130, True, (0, 0))]
            table, records = pc.census(net, mode, domain)
            for p, recs in records.items():
                for r, spec, (cin, cout) in zip(recs, specs, ch):
                    pc.check_legal(r, spec, cin, cout, (pc.MODE_IDS[mode], p))
            walked = pc.walked_points(table)
            table = {p: s for p, s in table.items() if p in walked or p in pc.sweep_domain()}     # (130 frames count only where the walk test runs them)
            every = {s for sigs in table.values() for s in sigs}
            met = {s for p in walked for s in table[p]}
            cover = pc.greedy_cover(table, walked)
            print('%-12s census: %d points, %d signatures, %d met by the walked windows %s; cover: %d points'
                  % (pc.MODE_IDS[mode], len(table), len(every), len(met), walked, len(cover)))
            points = cover + [(p, layers) for m, p, layers in NAMED_POINTS if m == mode]
            for p, new in points:
                res = pc.run_point(net, d2, P2, mode, p, new, E, E_LOG)
                assert res['signatures'] == table.get(p, res['signatures']), (res['what'], 'the plan changed between the census and the run')
                same = pc.batch_equals_alone(net, mode, p, res) if p[0] > 1 else None
                pc.print_point(res, new)
                if same is not None:
                    print('%-46s         bit-equal to each window alone on layers %s' % (res['what'], same))
                met |= {res['signatures'][i] for i in res['met']}
                del res
            net.close()
    finally:
        monkeypatch.delenv('RY_WINOGRAD', raising=False); gpu_ctx.reload_env()
    missing = sorted(every - met, key=repr)
    assert not missing, 'signatures no float64 comparison ran on: %s' % (missing,)
