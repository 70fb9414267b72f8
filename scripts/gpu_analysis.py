#!/usr/bin/env python3
"""WORLD analysis (CheapTrick + sp2mc) on one MI355X: milliseconds per host call of `Analyzer.run` (every call returns after its rows are
written) for 1 s and 0.5 s of audio (200 / 100 frames at 5 ms) at 16 and 24 kHz, with the float64 rows copied to the host and with the float32
rows left on the device, median of --reps calls, and -- labelled as what it is -- the numpy restatement's time on the same host.  Prints one JSON
line and writes it to --out.

    python scripts/gpu_analysis.py [--reps 30] [--out profiles/r09/analysis_bench.json]   timing
    python scripts/gpu_analysis.py --profile                                               a few 1-s calls only, for `rocprofv3 --kernel-trace --stats -- ...`
    python scripts/gpu_analysis.py --summary DB_GLOB OUT                                   per-kernel table of a rocprofv3 run
    python scripts/gpu_analysis.py --all [--out-dir DIR]                                   all of the above as child processes, each under its own
                                                                                           timeout, stopping at the first failure
"""
import argparse
import glob
import json
import sqlite3
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]

import numpy  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': float(numpy.median(ts)), 'min_ms': float(numpy.min(ts)), 'p90_ms': float(numpy.percentile(ts, 90))}


def inputs(fs, n):
    import world_analysis_cases as C
    x = C.wave('glide', int(n / 0.9) + 2, fs)                      # a wave that covers every frame
    return x, C.f0_track('alternating', n), C.times(n)


def run(args):
    import world_analysis_ref as R
    from realtime_yukarin_amd import engine, world_analysis
    ctx = engine.get_context(0)
    res = {'what': 'world analysis (CheapTrick + sp2mc), float64 transforms, ms per host call incl. copies', 'reps': args.reps, 'cases': []}
    for fs in (16000, 24000):
        for n in (200, 100):
            x, f0, t = inputs(fs, n)
            a = world_analysis.Analyzer(fs, ctx=ctx)
            host = timed(lambda: a.run(x, f0, t, want=('sp', 'mc')), args.reps)
            dev = timed(lambda: a.run(x, f0, t, want=('sp', 'mc'), device_rows=True), args.reps)
            mc_only = timed(lambda: a.run(x, f0, t, want=('mc',)), args.reps)
            sp = a.run(x, f0, t, want=('sp',))[0]
            again = timed(lambda: a.sp2mc(sp), args.reps)
            t0 = time.perf_counter()
            ref = R.cheaptrick(x, f0, t, fs)
            t1 = time.perf_counter()
            R.sp2mc(ref, 8, a.alpha)
            t2 = time.perf_counter()
            res['cases'].append({'fs': fs, 'frames': n, 'audio_ms': n * 5.0, 'wave_samples': int(x.size), 'host_rows_sp64_mc': host,
                                 'device_rows_sp32_mc': dev, 'mc_only': mc_only, 'sp2mc_of_host_rows': again,
                                 'run_over_audio': host['median_ms'] / (n * 5.0),
                                 'numpy_restatement_same_host_ms': {'cheaptrick': (t1 - t0) * 1e3, 'sp2mc': (t2 - t1) * 1e3}})
            a.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + '\n')


def profile(args):
    from realtime_yukarin_amd import engine, world_analysis
    ctx = engine.get_context(0)
    for fs in (16000, 24000):
        x, f0, t = inputs(fs, 200)
        a = world_analysis.Analyzer(fs, ctx=ctx)
        for _ in range(5):
            sp = a.run(x, f0, t)[0]
            a.sp2mc(sp)
        a.close()


def summary(db_glob, out):
    """Per-kernel totals from the rocpd database of `rocprofv3 --kernel-trace --stats` (its `top_kernels` view; durations in microseconds)."""
    db = sorted(glob.glob(db_glob, recursive=True))[0]
    rows = [r for r in sqlite3.connect(db).cursor().execute('select name, total_calls, total_duration, average, percentage from top_kernels')]
    tot = sum(r[2] for r in rows if 'analysis_' in r[0]) or 1.0
    lines = ['# rocprofv3 --kernel-trace --stats -- python scripts/gpu_analysis.py --profile: 5 calls of Analyzer.run + Analyzer.sp2mc on 1 s (200 frames)',
             '# at 16 / 24 kHz; durations in microseconds; share = of the analysis kernels\' time',
             '%-40s %8s %12s %10s %7s' % ('kernel', 'calls', 'total_us', 'avg_us', 'share')]
    for name, calls, total, avg, pct in rows:
        if 'analysis_' in name:
            lines.append('%-40s %8d %12.1f %10.2f %6.1f%%' % (name.split('(')[0][:40], calls, total, avg, 100.0 * total / tot))
    Path(out).write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def everything(args):
    out = Path(args.out_dir).resolve()
    out.mkdir(parents=True, exist_ok=True)
    me = str(Path(__file__).resolve())
    steps = [(300, [sys.executable, me, '--reps', str(args.reps), '--out', str(out / 'analysis_bench.json')]),
             (300, ['rocprofv3', '--kernel-trace', '--stats', '-d', str(out / 'trace'), '--', sys.executable, me, '--profile']),
             (120, [sys.executable, me, '--summary', str(out / 'trace' / '**' / '*.db'), str(out / 'analysis_kernel_trace.txt')])]
    for limit, cmd in steps:
        rc = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, cwd=str(ROOT)).returncode
        if rc != 0:
            print('step failed (%d): %s' % (rc, ' '.join(cmd)))
            return rc
    return 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default='')
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--summary', nargs=2)
    ap.add_argument('--all', action='store_true')
    ap.add_argument('--out-dir', default=str(ROOT / 'build' / 'analysis'), help='--all: where the bench record, the trace and its summary go (scratch; build/ is not tracked)')
    a = ap.parse_args()
    if a.summary:
        summary(*a.summary)
    elif a.profile:
        profile(a)
    elif a.all:
        sys.exit(everything(a))
    else:
        run(a)
