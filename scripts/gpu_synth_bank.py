#!/usr/bin/env python3
"""The realtime WORLD synthesis of B sessions on one MI355X, one bank push against B lone pushes: the median milliseconds of a
`StreamBank.push` of 0.5 s of frames (100 at 5 ms) on every one of B streams against B sequential `Synthesizer.push` calls on B lone handles with
the same seeds -- the shipped stream, the yardstick -- in one process, alternated call by call, in steady state (three warm-up pushes first).
Grid: 16 and 24 kHz, a voiced ('glide') and an all-unvoiced input (the most pulses), B = 1, 2, 8, 32, host rows and device rows (consecutive
slices of one buffer, read in place).  The streams of a cell get different frames (seeded slices of one long track, walked round and round).
Every push of every cell checks that stream b of the bank has the bits of its lone handle, and a cell reports the spread of the sequential side
(its 10th and 90th percentile) next to the medians.  Prints one JSON object and, with --out, writes it.

    python scripts/gpu_synth_bank.py [--reps 30] [--out FILE]       the measurement, as a child process under its own `timeout`
    python scripts/gpu_synth_bank.py --child --cell 16000,glide,8,host --only batched      one side of one cell alone (no timing, no JSON), for
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
FRAMES = 100                                   # 0.5 s at 5 ms
WARMUP = 3
SPAN = 8                                       # pushes a stream walks through before its frames repeat


def run(args):
    import world_synth_cases as C
    from realtime_yukarin_amd import engine, world_synth
    ctx = engine.get_context(0)
    res = {'what': 'realtime world synthesis of B sessions, ms per buffer of 0.5 s incl. host copies: one StreamBank.push against B Synthesizer.push calls',
           'reps': args.reps, 'frames': FRAMES, 'cells': []}
    one = args.cell.split(',') if args.cell else None
    row = world_synth.BINS * 4
    for fs in C.RATES if not one else (int(one[0]),):
        for kind in ('glide', 'unvoiced') if not one else (one[1],):
            n_all = FRAMES * (SPAN + max(BATCHES))
            f0, sp, ap = C.case(kind, n_all, fs)
            for B in BATCHES if not one else (int(one[2]),):
                for rows in ('host', 'device') if not one else (one[3],):
                    bank = world_synth.StreamBank(fs, 5.0, n_streams=B, seeds=list(range(B)), ctx=ctx)
                    lone = [world_synth.Synthesizer(fs, 5.0, seed=b, ctx=ctx) for b in range(B)]
                    ms = {'sequential': [], 'batched': []}
                    equal = True

                    def items(step):
                        """Push `step` of every stream: stream b reads slice (b + step mod SPAN) of the track; device rows: one buffer, in stream order."""
                        at = [((b + step % SPAN) * FRAMES) for b in range(B)]
                        host = [(f0[a:a + FRAMES], sp[a:a + FRAMES], ap[a:a + FRAMES]) for a in at]
                        if rows == 'host':
                            return host
                        dsp = world_synth.to_device(ctx, numpy.concatenate([h[1] for h in host]))
                        dap = world_synth.to_device(ctx, numpy.concatenate([h[2] for h in host]))
                        return [(h[0], world_synth.DeviceRows(dsp.address + i * FRAMES * row, FRAMES, keep=dsp),
                                 world_synth.DeviceRows(dap.address + i * FRAMES * row, FRAMES, keep=dap)) for i, h in enumerate(host)]

                    calls = dict(world_synth.calls)
                    for step in range(WARMUP + args.reps):
                        its = items(step)                               # outside the timed part: both sides get the same rows
                        a = b = None
                        if args.only != 'batched':
                            t0 = time.perf_counter()
                            a = [s.push(*it) for s, it in zip(lone, its)]
                            ms['sequential'].append((time.perf_counter() - t0) * 1e3)
                        if args.only != 'sequential':
                            t0 = time.perf_counter()
                            b = bank.push(its)
                            ms['batched'].append((time.perf_counter() - t0) * 1e3)
                        if a is not None and b is not None:
                            equal = equal and all(p.dtype == q.dtype and p.size > 0 and numpy.array_equal(p, q) for p, q in zip(a, b))
                    counts = bank.counts() if not args.only or args.only == 'batched' else {}
                    bank.close()
                    for s in lone:
                        s.close()
                    if args.only:
                        continue
                    path = 'bank_packed' if rows == 'host' else 'bank_in_place'
                    assert world_synth.calls == dict(calls, **{path: calls[path] + WARMUP + args.reps}), world_synth.calls
                    seq, bat = numpy.asarray(ms['sequential'][WARMUP:]), numpy.asarray(ms['batched'][WARMUP:])
                    cell = {'fs': fs, 'kind': kind, 'B': B, 'rows': rows, 'bits_equal': bool(equal), 'counts': counts,
                            'ms_sequential': round(float(numpy.median(seq)), 4), 'ms_batched': round(float(numpy.median(bat)), 4),
                            'ms_sequential_p10': round(float(numpy.percentile(seq, 10)), 4), 'ms_sequential_p90': round(float(numpy.percentile(seq, 90)), 4),
                            'ms_batched_p10': round(float(numpy.percentile(bat, 10)), 4), 'ms_batched_p90': round(float(numpy.percentile(bat, 90)), 4)}
                    cell['batched_over_sequential'] = round(cell['ms_batched'] / cell['ms_sequential'], 3)
                    res['cells'].append(cell)
                    print(json.dumps(cell), file=sys.stderr, flush=True)
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
    ap.add_argument('--cell', default='', help='rate,kind,B,host|device: this cell alone')
    ap.add_argument('--only', default='', choices=('', 'sequential', 'batched'), help='with --child: run this side alone')
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    a = ap.parse_args()
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps)] + (['--out', a.out] if a.out else []) + (['--cell', a.cell] if a.cell else [])
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
