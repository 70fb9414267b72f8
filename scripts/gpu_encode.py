#!/usr/bin/env python3
"""The CREPE-mode encode stage at 'full' capacity on one MI355X, fused against unfused: median milliseconds of device-synchronised calls after
warm-up, both forms in the same process on the same handles, alternated call by call.  Unfused is the chain `world_analysis.extract` runs behind
the reference's CREPE wrapper, its three parts timed separately: `CrepeModel.predict` (with the activation, as the shim asks for it), the host's
`predict_voicing` + mask + time axis, `Analyzer.run` on the float64 wave.  Fused is what `encode.extract` runs: `CrepeModel.track(device=True)`,
`Analyzer.run_device`, the download of f0 -- and the same with `device_rows=True` (sp and ap stay on the card as float32 rows).  Grid: 0.5 s and
1 s of audio, 16 and 24 kHz, f32 and bf16x3, step 5 ms.  Checks in every cell that both forms return the same bits, prints one JSON object and,
with --out, writes it.  Seeded synthetic weights (no trained ones exist here).

    python scripts/gpu_encode.py [--reps 30] [--out FILE]      the measurement, as a child process under its own `timeout`
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

STEP_MS = 5
LIMIT_S = 420
WANT = ('sp', 'mc', 'ap', 'coded_ap')


def signal(n, sr, seed=0):
    rng = numpy.random.default_rng(seed)
    t = numpy.arange(n) / sr
    f = 180 + 50 * numpy.sin(2 * numpy.pi * t)
    x = 0.3 * numpy.sin(2 * numpy.pi * numpy.cumsum(f) / sr) + rng.normal(0, 0.02, n)
    x[n // 2:n // 2 + n // 5] = rng.normal(0, 0.02, n // 5)          # an unvoiced stretch
    return x.astype(numpy.float32)


def run(args):
    from realtime_yukarin_amd import crepe, engine, world_analysis
    ctx = engine.get_context(0)
    hop = crepe.hop_length(STEP_MS)
    P = crepe.synthetic_params('full', 0)
    res = {'capacity': 'full', 'step_ms': STEP_MS, 'reps': args.reps, 'cells': []}
    for dtype in ('f32', 'bf16x3'):
        model = crepe.CrepeModel('full', P, ctx=ctx, dtype=dtype)
        for sr in (16000, 24000):
            analyzer = world_analysis.Analyzer(sr, order=8, ctx=ctx)
            for seconds in (0.5, 1.0):
                x = signal(int(sr * seconds), sr)
                parts = {'predict': [], 'host_voicing': [], 'extract': [], 'unfused': [], 'fused': [], 'fused_device_rows': []}

                def unfused():
                    t0 = time.perf_counter()
                    f0, conf, _ = model.predict(x, sr, hop)
                    t1 = time.perf_counter()
                    voiced = (crepe.predict_voicing(conf) == 1) | (conf > 0.1)
                    f64 = f0.astype(numpy.float64)
                    f64[~voiced] = 0
                    t = numpy.arange(conf.shape[0]) * STEP_MS / 1000.0
                    t2 = time.perf_counter()
                    out = analyzer.run(x.astype(numpy.float64), f64, t, want=WANT)
                    t3 = time.perf_counter()
                    for k, v in (('predict', t1 - t0), ('host_voicing', t2 - t1), ('extract', t3 - t2), ('unfused', t3 - t0)):
                        parts[k].append(v * 1e3)
                    return (f64,) + out

                def fused(device_rows=False):
                    t0 = time.perf_counter()
                    trk = model.track(x, sr, hop, STEP_MS, device=True)
                    out = analyzer.run_device(trk.wave, trk.samples, trk.f0, trk.t, trk.frames, want=WANT, device_rows=device_rows)
                    f64 = trk.download()[1]
                    parts['fused_device_rows' if device_rows else 'fused'].append((time.perf_counter() - t0) * 1e3)
                    return (f64,) + out

                for _ in range(3):
                    a, b = unfused(), fused()
                    fused(True)
                equal = all(p.dtype == q.dtype and numpy.array_equal(p.view(numpy.uint64), q.view(numpy.uint64)) for p, q in zip(a, b))
                for v in parts.values():
                    del v[:]
                for _ in range(args.reps):
                    unfused(); fused(); fused(True)
                cell = {'dtype': dtype, 'sr': sr, 'seconds': seconds, 'frames': int(a[0].size), 'voiced_frames': int((a[0] != 0).sum()), 'bits_equal': bool(equal)}
                cell.update({'ms_' + k: round(float(numpy.median(v)), 4) for k, v in parts.items()})
                cell['unfused_over_fused'] = round(cell['ms_unfused'] / cell['ms_fused'], 3)
                res['cells'].append(cell)
                print(json.dumps(cell), file=sys.stderr, flush=True)
            analyzer.close()
        model.close()
    res['bits_equal'] = all(c['bits_equal'] for c in res['cells'])
    res['fused_faster_everywhere'] = all(c['ms_fused'] < c['ms_unfused'] for c in res['cells'])
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
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    a = ap.parse_args()
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps)] + (['--out', a.out] if a.out else [])
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
