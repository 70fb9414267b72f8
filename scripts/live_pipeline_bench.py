#!/usr/bin/env python3
"""The reference's three-stream live loop on one MI355X at the shipped margins -- 1 s buffers, encode / convert / decode margins 0 / 0.5 / 0,
24 kHz, `full` CREPE capacity, SYN-64 predictors: ms per second of audio, medians and quartiles, of three arms that take turns buffer by buffer
(the order rotates) in one session:
  (live)      `LivePipeline.push`: every buffer encoded once, the convert window fetched from rows kept on the card;
  (composed)  `LivePipeline(resident=False).push`: the same plans applied to host arrays over the separate calls;
  (window)    `Pipeline.push(discard=(100, 100), advance=24000)` over the equivalent 2 s windows: every sample goes through the encode stage twice
              (the CREPE network passes of the shared frames are kept, the rest runs again).
live and composed are checked for equal bits call by call; the window arm computes another signal and is not
compared.  Prints one JSON object and writes it to --out; a gap is called one only when it exceeds BOTH arms' interquartile ranges.

    python scripts/live_pipeline_bench.py [--reps 12] [--out profiles/r31/live_pipeline_bench.json]
    (the measurement runs in a child process under its own `timeout`)
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'scripts')]

import pipeline_gate_first_bench as GF  # noqa: E402  (the models, the signal, the statistics)

LIMIT_S = 540
FS, T, MARGINS, PAD = GF.FS, 1.0, (0.0, 0.5, 0.0), 100
WARM = GF.WARM


def run(args):
    n = args.reps + WARM
    vc, param, _, pipeline, shim = GF.set_up(1)
    from yukarin import Wave                                              # (the shims are installed by now)
    sig = GF.signal(FS * (n + 2), 2)
    arms = {'live': pipeline.LivePipeline(vc, param, T, *MARGINS, crepe_capacity='full', seed=1),
            'composed': pipeline.LivePipeline(vc, param, T, *MARGINS, crepe_capacity='full', seed=1, resident=False),
            'window': pipeline.Pipeline(vc, param, crepe_capacity='full', seed=1)}
    names = list(arms)
    ms, bits = {name: [] for name in names}, True
    before = dict(pipeline.calls)
    for k in range(n):
        seen = {}
        for name in names[k % 3:] + names[:k % 3]:
            t0 = time.perf_counter()
            if name == 'window':
                out = arms[name].push(Wave(sig[k * FS:(k + 2) * FS], FS), discard=(PAD, PAD), advance=None if k == 0 else FS)
            else:
                out = arms[name].push(sig[(k + 1) * FS:(k + 2) * FS])
            t = 1e3 * (time.perf_counter() - t0)
            seen[name] = out.wave
            if k >= WARM:
                ms[name].append(t / T)
        bits = bits and GF.same(seen['live'], seen['composed'])
    took = {key: pipeline.calls[key] - before[key] for key in before}
    res = {'what': 'ms per second of audio, the arms taking turns buffer by buffer: LivePipeline.push (live), its composed path (composed), '
                   'Pipeline.push(advance=) over the equivalent 2 s windows (window)',
           'capacity': 'full', 'fs': FS, 'time_length': T, 'margins': list(MARGINS), 'reps': args.reps, 'warm': WARM,
           'live_equals_composed': bool(bits), 'calls': took}
    res.update({name + '_ms_per_s': GF.stats(v) for name, v in ms.items()})
    res['live_against_window'] = GF.compare(res, 'window_ms_per_s', 'live_ms_per_s')
    res['live_against_composed'] = GF.compare(res, 'composed_ms_per_s', 'live_ms_per_s')
    vc._fused_core().set_discard(0, 0)
    for a in arms.values():
        a.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + '\n')
    return 0 if bits and took['resident'] == 2 * n and took['composed'] == n else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r31' / 'live_pipeline_bench.json'))
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    a = ap.parse_args()
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps), '--out', a.out]
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
