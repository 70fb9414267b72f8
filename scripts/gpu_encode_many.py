#!/usr/bin/env python3
"""The CREPE-mode encode of B waves at 'full' capacity on one MI355X, batched against sequential: the median milliseconds of device-synchronised
`encode.extract_many` calls on B waves against B sequential `encode.extract` calls on the same waves -- the shipped single-wave path, the yardstick
-- both through the drop-in `AcousticFeature` in one process on the same handles, alternated call by call.  Grid: 1 s waves at 24 and 16 kHz, f32
and bf16x3, B = 1, 2, 4, 8, step 5 ms.  Every cell checks that wave i of the batch has the bits of its own `extract`, and reports the spread of the
sequential side (its 10th and 90th percentile) next to the medians.  Prints one JSON object and, with --out, writes it.  Seeded synthetic weights.

    python scripts/gpu_encode_many.py [--reps 30] [--out FILE]      the measurement, as a child process under its own `timeout`
    python scripts/gpu_encode_many.py --child --cell f32,24000,2 --only batched      one side of one cell alone (no timing, no JSON), for
                                                                    `rocprofv3 --kernel-trace --stats -- ...` and scripts/rocprof_summary.py
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy  # noqa: E402

from gpu_encode import signal  # noqa: E402

STEP_MS = 5
LIMIT_S = 540
ARGS = dict(frame_period=STEP_MS, f0_floor=71.0, f0_ceil=800.0, fft_length=1024, order=8, alpha=0.466, dtype=numpy.float32)
KEYS = ('f0', 'sp', 'ap', 'coded_ap', 'mc', 'voiced')


def same(a, b):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run(args):
    from realtime_yukarin_amd import crepe, encode, world_analysis
    from realtime_yukarin_amd.compat import crepe as shim
    from realtime_yukarin_amd.compat.yukarin import AcousticFeature, Wave

    class Feature(AcousticFeature):
        pass

    class CrepeFeature(Feature):
        pass

    world_analysis.aperiodicity = world_analysis.device_aperiodicity
    encode.install(Feature, CrepeFeature)
    P = crepe.synthetic_params('full', 0)
    res = {'capacity': 'full', 'step_ms': STEP_MS, 'seconds': 1.0, 'reps': args.reps, 'cells': []}
    one = args.cell.split(',') if args.cell else None
    for dtype in ('f32', 'bf16x3') if not one else (one[0],):
        model = crepe.CrepeModel('full', P, dtype=dtype)
        shim._models[model.m] = model
        for sr in (24000, 16000) if not one else (int(one[1]),):
            for B in (1, 2, 4, 8) if not one else (int(one[2]),):
                waves = [Wave(signal(sr, sr, seed=i), sr) for i in range(B)]
                ms = {'sequential': [], 'batched': []}

                def sequential():
                    t0 = time.perf_counter()
                    out = [encode.extract(CrepeFeature, w, **ARGS) for w in waves]
                    ms['sequential'].append((time.perf_counter() - t0) * 1e3)
                    return out

                def batched():
                    t0 = time.perf_counter()
                    out = encode.extract_many(CrepeFeature, waves, **ARGS)
                    ms['batched'].append((time.perf_counter() - t0) * 1e3)
                    return out

                if args.only:                                           # one side alone, for a kernel trace
                    for _ in range(3 + args.reps):
                        sequential() if args.only == 'sequential' else batched()
                    continue
                for _ in range(3):
                    a, b = sequential(), batched()
                equal = all(same(getattr(p, k), getattr(q, k)) for p, q in zip(a, b) for k in KEYS)
                for v in ms.values():
                    del v[:]
                calls = dict(encode.calls)
                for _ in range(args.reps):
                    sequential(); batched()
                assert encode.calls['many'] - calls['many'] == args.reps and encode.calls['fused'] - calls['fused'] == args.reps * B, encode.calls
                seq = numpy.asarray(ms['sequential'])
                cell = {'dtype': dtype, 'sr': sr, 'B': B, 'frames': int(sum(f.f0.shape[0] for f in a)), 'bits_equal': bool(equal),
                        'ms_sequential': round(float(numpy.median(seq)), 4), 'ms_batched': round(float(numpy.median(ms['batched'])), 4),
                        'ms_sequential_p10': round(float(numpy.percentile(seq, 10)), 4), 'ms_sequential_p90': round(float(numpy.percentile(seq, 90)), 4)}
                cell['batched_over_sequential'] = round(cell['ms_batched'] / cell['ms_sequential'], 3)
                res['cells'].append(cell)
                print(json.dumps(cell), file=sys.stderr, flush=True)
        model.close()
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
    ap.add_argument('--cell', default='', help='dtype,rate,B: this cell alone')
    ap.add_argument('--only', default='', choices=('', 'sequential', 'batched'), help='with --child: run this side alone')
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    a = ap.parse_args()
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps)] + (['--out', a.out] if a.out else []) + (['--cell', a.cell] if a.cell else [])
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
