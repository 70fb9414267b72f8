#!/usr/bin/env python3
"""WORLD synthesis on one MI355X: device-synchronised milliseconds per call (every `ry_synth_*` call returns after its samples are on the
host) for 1 s and 0.5 s of frames (200 / 100 at 5 ms) at 16 and 24 kHz, a voiced and an all-unvoiced input (the latter has the most pulses),
one-shot and as a stream of 0.5-s pushes, the streaming lag in samples, and -- labelled as what it is -- the numpy restatement's time on the
same host.  Prints one JSON line and writes it to --out.

    python scripts/gpu_synth.py [--reps 30] [--out profiles/r08/synth_bench.json]      timing
    python scripts/gpu_synth.py --profile                                               a few 1-s calls only, for `rocprofv3 --kernel-trace --stats -- ...`
    python scripts/gpu_synth.py --summary DB_GLOB OUT                                   per-kernel table of a rocprofv3 run
    python scripts/gpu_synth.py --all [--out-dir DIR]                                   all of the above as child processes, each under its own
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


def run(args):
    import world_synth_cases as C
    import world_synth_ref as R
    from realtime_yukarin_amd import engine, world_synth
    ctx = engine.get_context(0)
    res = {'what': 'world synthesis, float64 transforms, ms per call incl. host copies', 'reps': args.reps, 'cases': []}
    for fs in C.RATES:
        for kind in ('glide', 'unvoiced'):
            for n in (200, 100):
                f0, sp, ap = C.case(kind, 3 * n, fs)
                s = world_synth.Synthesizer(fs, 5.0, seed=1, ctx=ctx)
                one = timed(lambda: s.synthesize(f0[:n], sp[:n], ap[:n]), args.reps)
                dsp, dap = world_synth.to_device(ctx, sp[:n]), world_synth.to_device(ctx, ap[:n])
                dev = timed(lambda: s.synthesize(f0[:n], dsp, dap), args.reps)
                pulses = len(s.pulses()[0])
                # steady-state push of n frames: the stream keeps running over a long input, one push per timing
                state = {'i': 0}
                big = C.case(kind, n * (args.reps + 8), fs)

                def push():
                    a = state['i'] * n
                    state['i'] += 1
                    return s.push(big[0][a:a + n], big[1][a:a + n], big[2][a:a + n])
                st = timed(push, args.reps)
                emitted_bound = int(s._ctx.lib.dll.ry_synth_bound(s._handle, 0, 1))      # what a flush would still return = the lag
                s.reset()
                t0 = time.perf_counter()
                R.synthesize(f0[:n], sp[:n], ap[:n], fs, 5.0, seed=1)
                ref_ms = (time.perf_counter() - t0) * 1e3
                audio_ms = n * 5.0
                res['cases'].append({'fs': fs, 'input': kind, 'frames': n, 'audio_ms': audio_ms, 'pulses': pulses, 'one_shot_host_rows': one,
                                     'one_shot_device_rows': dev, 'stream_push': st, 'push_over_audio': st['median_ms'] / audio_ms,
                                     'lag_samples_after_push': emitted_bound, 'lag_bound_samples': s.lag_samples(f0=fs / 1024 + 1),
                                     'numpy_restatement_same_host_ms': ref_ms})
                s.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + '\n')


def profile(args):
    import world_synth_cases as C
    from realtime_yukarin_amd import engine, world_synth
    ctx = engine.get_context(0)
    for fs in C.RATES:
        for kind in ('glide', 'unvoiced'):
            f0, sp, ap = C.case(kind, 200, fs)
            s = world_synth.Synthesizer(fs, 5.0, seed=1, ctx=ctx)
            for _ in range(5):
                s.synthesize(f0, sp, ap)
            s.close()


def summary(db_glob, out):
    """Per-kernel totals from the rocpd database of `rocprofv3 --kernel-trace --stats` (its `top_kernels` view; durations in microseconds)."""
    db = sorted(glob.glob(db_glob, recursive=True))[0]
    rows = [r for r in sqlite3.connect(db).cursor().execute('select name, total_calls, total_duration, average, percentage from top_kernels')]
    tot = sum(r[2] for r in rows if 'synth_' in r[0]) or 1.0
    lines = ['# rocprofv3 --kernel-trace --stats -- python scripts/gpu_synth.py --profile: 5 one-shot calls of 1 s (200 frames) at 16 / 24 kHz x voiced /',
             '# all-unvoiced; durations in microseconds; share = of the synthesis kernels\' time',
             '%-40s %8s %12s %10s %7s' % ('kernel', 'calls', 'total_us', 'avg_us', 'share')]
    for name, calls, total, avg, pct in rows:
        if 'synth_' in name:
            lines.append('%-40s %8d %12.1f %10.2f %6.1f%%' % (name.split('(')[0][:40], calls, total, avg, 100.0 * total / tot))
    Path(out).write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def everything(args):
    out = Path(args.out_dir).resolve()
    out.mkdir(parents=True, exist_ok=True)
    me = str(Path(__file__).resolve())
    steps = [(300, [sys.executable, me, '--reps', str(args.reps), '--out', str(out / 'synth_bench.json')]),
             (300, ['rocprofv3', '--kernel-trace', '--stats', '-d', str(out / 'trace'), '--', sys.executable, me, '--profile']),
             (120, [sys.executable, me, '--summary', str(out / 'trace' / '**' / '*.db'), str(out / 'synth_kernel_trace.txt')])]
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
    ap.add_argument('--out-dir', default=str(ROOT / 'build' / 'synth'), help='--all: where the bench record, the trace and its summary go (scratch; build/ is not tracked)')
    a = ap.parse_args()
    if a.summary:
        summary(*a.summary)
    elif a.profile:
        profile(a)
    elif a.all:
        sys.exit(everything(a))
    else:
        run(a)
