"""The plan census of SYN-64 in the four modes (tests/plan_census_cases.py), one line per (mode, layer, signature) with the points that have it:
profiles/r27/plan_census.txt.  Builds plans only, launches nothing.   usage (GPU box): python scripts/plan_census_report.py > plan_census.txt"""
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / 'tests'), str(ROOT)]

import plan_census_cases as pc                                  # noqa: E402
from realtime_yukarin_amd import engine, synth                  # noqa: E402
from realtime_yukarin_amd.weights import flatten_params         # noqa: E402

ctx = engine.get_context(0)
d2, P2 = synth.model_params('SYN-64')[1]
for mode, (dtype, wino) in enumerate(pc.MODES):
    os.environ['RY_WINOGRAD'] = wino
    ctx.reload_env()
    net = engine.Net(ctx, d2, flatten_params(d2, P2), width=synth.FFT_BINS - 1)
    net.set_dtype(dtype)
    table, _ = pc.census(net, mode, pc.sweep_domain() + [(1, 130, True, (0, 0))])
    walked = pc.walked_points(table)
    table = {p: s for p, s in table.items() if p in walked or p in pc.sweep_domain()}
    print('\n'.join(pc.census_report(pc.MODE_IDS[mode], table)))
    net.close()
