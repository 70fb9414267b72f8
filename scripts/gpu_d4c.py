#!/usr/bin/env python3
"""D4C (band aperiodicity of the WORLD analysis) on one MI355X: milliseconds per host call of `Analyzer.run` (every call returns after its rows are
written) for 1 s and 0.5 s of the `glide` case (200 / 100 frames at 5 ms) at 16 and 24 kHz -- `ap` alone and `sp + mc + ap + coded_ap` in one call,
each with host rows and with device rows -- median of --reps calls; the 1-s call with an all-voiced and with an all-unvoiced track (off frames skip
the general body); the existing `sp + mc` call for comparison with scripts/gpu_analysis.py; and -- labelled as what it is -- the numpy
restatement's time on the same host.  Prints one JSON line and writes it to --out.

    python scripts/gpu_d4c.py [--reps 30] [--out profiles/r10/d4c_bench.json]       timing
    python scripts/gpu_d4c.py --profile                                              a few 1-s calls only, for `rocprofv3 --kernel-trace --stats -- ...`
    python scripts/gpu_d4c.py --summary DB_GLOB OUT                                  per-kernel table of a rocprofv3 run
    python scripts/gpu_d4c.py --all [--out-dir DIR]                                  the GPU tests of D4C (output kept), then all of the above, as child
                                                                                     processes, each under its own timeout, stopping at the first failure
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


def inputs(fs, n, track='glide'):
    import world_analysis_cases as C
    x = C.wave('glide', int(n / 0.9) + 2, fs)                      # a wave that covers every frame
    return x, C.f0_track(track, n), C.times(n)


def run(args):
    import world_d4c_ref as R
    from realtime_yukarin_amd import engine, world_analysis
    ctx = engine.get_context(0)
    everything = ('sp', 'mc', 'ap', 'coded_ap')
    res = {'what': 'world analysis with D4C, float64 transforms, ms per host call incl. copies', 'reps': args.reps, 'cases': []}
    for fs in (16000, 24000):
        for n in (200, 100):
            x, f0, t = inputs(fs, n)
            a = world_analysis.Analyzer(fs, ctx=ctx)
            a.record_integers()
            a.run(x, f0, t, want=('ap',))
            frames_on = int(a.d4c_record()[1].sum())
            a.record_integers(False)
            case = {'fs': fs, 'frames': n, 'frames_on': frames_on, 'audio_ms': n * 5.0, 'wave_samples': int(x.size),
                    'ap_host_rows': timed(lambda: a.run(x, f0, t, want=('ap',)), args.reps),
                    'ap_device_rows': timed(lambda: a.run(x, f0, t, want=('ap',), device_rows=True), args.reps),
                    'sp_mc_ap_coded_host_rows': timed(lambda: a.run(x, f0, t, want=everything), args.reps),
                    'sp_mc_ap_coded_device_rows': timed(lambda: a.run(x, f0, t, want=everything, device_rows=True), args.reps),
                    'sp_mc_host_rows': timed(lambda: a.run(x, f0, t, want=('sp', 'mc')), args.reps)}
            if n == 200:
                u = numpy.zeros(n)
                case['ap_host_rows_all_unvoiced'] = timed(lambda: a.run(x, u, t, want=('ap',)), args.reps)
                case['ap_host_rows_all_voiced'] = case['ap_host_rows']
            t0 = time.perf_counter()
            R.d4c(x, f0, t, fs)
            case['numpy_restatement_same_host_ms'] = {'d4c': (time.perf_counter() - t0) * 1e3}
            case['run_over_audio'] = case['sp_mc_ap_coded_host_rows']['median_ms'] / (n * 5.0)
            res['cases'].append(case)
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
            a.run(x, f0, t, want=('sp', 'mc', 'ap', 'coded_ap'))
            a.run(x, numpy.zeros(200), t, want=('ap',))
        a.close()


def summary(db_glob, out):
    """Per-kernel totals from the rocpd database of `rocprofv3 --kernel-trace --stats` (its `top_kernels` view; durations in microseconds)."""
    db = sorted(glob.glob(db_glob, recursive=True))[0]
    rows = [r for r in sqlite3.connect(db).cursor().execute('select name, total_calls, total_duration, average, percentage from top_kernels')]
    keep = [r for r in rows if 'analysis_' in r[0] or 'd4c_' in r[0]]
    tot = sum(r[2] for r in keep) or 1.0
    lines = ['# rocprofv3 --kernel-trace --stats -- python scripts/gpu_d4c.py --profile: per rate (16 / 24 kHz) 5 calls of Analyzer.run for sp + mc + ap + coded_ap',
             '# on 1 s (200 voiced frames: analysis_frame + d4c_frame) and 5 calls for ap on 200 unvoiced frames (d4c_frame, rows filled); durations in',
             '# microseconds; share = of these kernels\' time',
             '%-40s %8s %12s %10s %7s' % ('kernel', 'calls', 'total_us', 'avg_us', 'share')]
    for name, calls, total, avg, pct in keep:
        lines.append('%-40s %8d %12.1f %10.2f %6.1f%%' % (name.split('(')[0][:40], calls, total, avg, 100.0 * total / tot))
    Path(out).write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def everything(args):
    out = Path(args.out_dir).resolve()
    out.mkdir(parents=True, exist_ok=True)
    me = str(Path(__file__).resolve())
    log = out / 'd4c_pytest_gpu.txt'
    steps = [(900, ['bash', '-c', 'set -o pipefail; %s -m pytest tests/test_world_d4c_gpu.py -q -s -m gpu -p no:cacheprovider 2>&1 | tee %s | tail -5' % (sys.executable, log)]),
             (300, [sys.executable, me, '--reps', str(args.reps), '--out', str(out / 'd4c_bench.json')]),
             (300, ['rocprofv3', '--kernel-trace', '--stats', '-d', str(out / 'trace'), '--', sys.executable, me, '--profile']),
             (120, [sys.executable, me, '--summary', str(out / 'trace' / '**' / '*.db'), str(out / 'd4c_kernel_trace.txt')])]
    for limit, cmd in steps[args.skip_tests:]:
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
    ap.add_argument('--skip-tests', type=int, default=0, choices=(0, 1), help='--all: 1 leaves the GPU tests out')
    ap.add_argument('--out-dir', default=str(ROOT / 'build' / 'd4c'), help='--all: where the test output, the bench record, the trace and its summary go (scratch; build/ is not tracked)')
    a = ap.parse_args()
    if a.summary:
        summary(*a.summary)
    elif a.profile:
        profile(a)
    elif a.all:
        sys.exit(everything(a))
    else:
        run(a)
