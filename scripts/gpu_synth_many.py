#!/usr/bin/env python3
"""The WORLD synthesis of B feature sets on one MI355X, batched against sequential: the median milliseconds of device-synchronised
`Synthesizer.synthesize_many` calls on B items against B sequential `synthesize` calls on the same items -- the shipped single call, the
yardstick -- in one process on the same handle, alternated call by call.  Grid: 1 s and 0.5 s of frames (200 / 100 at 5 ms) at 16 and 24 kHz, a
voiced ('glide') and an all-unvoiced input (the most pulses), B = 1, 2, 8, 32, host rows and device rows (consecutive slices of one buffer, read
in place).  The items of a cell differ (seeded slices of one long track).  Every cell checks that wave i of the batch has the bits of its own
`synthesize`, and reports the spread of the sequential side (its 10th and 90th percentile) next to the medians.  Prints one JSON object and, with
--out, writes it.

    python scripts/gpu_synth_many.py [--reps 30] [--out FILE]       the measurement, as a child process under its own `timeout`
    python scripts/gpu_synth_many.py --child --cell 16000,glide,200,8,host --only batched      one side of one cell alone (no timing, no JSON), for
                                                                    `rocprofv3 --kernel-trace --stats -- ...` and scripts/rocprof_summary.py
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]

import numpy  # noqa: E402

LIMIT_S = 540
BATCHES = (1, 2, 8, 32)


def run(args):
    import world_synth_cases as C
    from realtime_yukarin_amd import engine, world_synth
    ctx = engine.get_context(0)
    res = {'what': 'world synthesis of B feature sets, ms per B items incl. host copies: one synthesize_many against B synthesize calls', 'reps': args.reps,
           'cells': []}
    one = args.cell.split(',') if args.cell else None
    for fs in C.RATES if not one else (int(one[0]),):
        s = world_synth.Synthesizer(fs, 5.0, seed=1, ctx=ctx)
        for kind in ('glide', 'unvoiced') if not one else (one[1],):
            for n in (200, 100) if not one else (int(one[2]),):
                f0, sp, ap = C.case(kind, n * max(BATCHES), fs)
                for B in BATCHES if not one else (int(one[3]),):
                    host = [(f0[i * n:(i + 1) * n], sp[i * n:(i + 1) * n], ap[i * n:(i + 1) * n]) for i in range(B)]
                    dsp, dap = world_synth.to_device(ctx, sp[:B * n]), world_synth.to_device(ctx, ap[:B * n])
                    row = world_synth.BINS * 4
                    dev = [(f0[i * n:(i + 1) * n], world_synth.DeviceRows(dsp.address + i * n * row, n, keep=dsp),
                            world_synth.DeviceRows(dap.address + i * n * row, n, keep=dap)) for i in range(B)]
                    for rows, items in (('host', host), ('device', dev)) if not one else ((one[4], host if one[4] == 'host' else dev),):
                        ms = {'sequential': [], 'batched': []}

                        def sequential():
                            t0 = time.perf_counter()
                            out = [s.synthesize(*it) for it in items]
                            ms['sequential'].append((time.perf_counter() - t0) * 1e3)
                            return out

                        def batched():
                            t0 = time.perf_counter()
                            out = s.synthesize_many(items)
                            ms['batched'].append((time.perf_counter() - t0) * 1e3)
                            return out

                        if args.only:                                   # one side alone, for a kernel trace
                            for _ in range(3 + args.reps):
                                sequential() if args.only == 'sequential' else batched()
                            continue
                        for _ in range(3):
                            a, b = sequential(), batched()
                        equal = len(a) == len(b) and all(p.dtype == q.dtype and numpy.array_equal(p, q) for p, q in zip(a, b))
                        for v in ms.values():
                            del v[:]
                        calls = dict(world_synth.calls)
                        for _ in range(args.reps):
                            sequential(); batched()
                        path = 'packed' if rows == 'host' else 'in_place'
                        assert world_synth.calls == dict(calls, **{path: calls[path] + args.reps}), world_synth.calls
                        seq = numpy.asarray(ms['sequential'])
                        cell = {'fs': fs, 'kind': kind, 'frames': n, 'B': B, 'rows': rows, 'bits_equal': bool(equal),
                                'ms_sequential': round(float(numpy.median(seq)), 4), 'ms_batched': round(float(numpy.median(ms['batched'])), 4),
                                'ms_sequential_p10': round(float(numpy.percentile(seq, 10)), 4), 'ms_sequential_p90': round(float(numpy.percentile(seq, 90)), 4)}
                        cell['batched_over_sequential'] = round(cell['ms_batched'] / cell['ms_sequential'], 3)
                        res['cells'].append(cell)
                        print(json.dumps(cell), file=sys.stderr, flush=True)
        s.close()
    if args.only:
        return 0
    res['bits_equal'] = all(c['bits_equal'] for c in res['cells'])
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + '\n')
    return 0 if res['bits_equal'] else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default='')
    ap.add_argument('--cell', default='', help='rate,kind,frames,B,host|device: this cell alone')
    ap.add_argument('--only', default='', choices=('', 'sequential', 'batched'), help='with --child: run this side alone')
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    a = ap.parse_args()
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps)] + (['--out', a.out] if a.out else []) + (['--cell', a.cell] if a.cell else [])
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
