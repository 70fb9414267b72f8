#!/usr/bin/env python3
"""The three-stream live loop for B streams on one MI355X at the shipped margins -- 1 s buffers, encode / convert / decode margins 0 / 0.5 / 0,
24 kHz, `full` CREPE capacity, SYN-64 predictors -- at B = 1, 2, 4, 8: ms per buffer of all B streams, medians and quartiles, of two arms that
take turns buffer by buffer (the order alternates) in one session:
  (lone)  B `LivePipeline.push` calls, one per stream, one after the other;
  (bank)  one `LivePipelineBank.push` with the same buffers and seeds.
Every stream's samples are checked for equal bits between the arms in every round.  Prints one JSON object and writes it to --out; a gap is
called one only when it exceeds BOTH arms' interquartile ranges.

    python scripts/live_bank_bench.py [--reps 12] [--out profiles/r33/live_bank_bench.json]
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

LIMIT_S = 840
FS, T, MARGINS = GF.FS, 1.0, (0.0, 0.5, 0.0)
BANKS = (1, 2, 4, 8)
WARM = GF.WARM


def run(args):
    n = args.reps + WARM
    vc, param, _, pipeline, shim = GF.set_up(1)
    sigs = [GF.signal(FS * (n + 1), 10 + b) for b in range(max(BANKS))]
    res = {'what': 'ms per buffer of B streams, the arms taking turns buffer by buffer: B LivePipeline.push calls (lone), one LivePipelineBank.push (bank)',
           'capacity': 'full', 'fs': FS, 'time_length': T, 'margins': list(MARGINS), 'reps': args.reps, 'warm': WARM, 'cells': {}}
    ok = True
    for B in BANKS:
        seeds = list(range(1, B + 1))
        lone = [pipeline.LivePipeline(vc, param, T, *MARGINS, crepe_capacity='full', seed=s) for s in seeds]
        bank = pipeline.LivePipelineBank(vc, param, B, T, *MARGINS, seeds=seeds, crepe_capacity='full')
        ms, bits = {'lone': [], 'bank': []}, True
        before = dict(pipeline.calls)
        for k in range(n):
            bufs = [sigs[b][k * FS:(k + 1) * FS] for b in range(B)]
            seen = {}
            for name in (('lone', 'bank') if k % 2 == 0 else ('bank', 'lone')):
                t0 = time.perf_counter()
                if name == 'lone':
                    outs = [p.push(x) for p, x in zip(lone, bufs)]
                else:
                    outs = bank.push(bufs)
                t = 1e3 * (time.perf_counter() - t0)
                seen[name] = [o.wave for o in outs]
                if k >= WARM:
                    ms[name].append(t)
            bits = bits and all(GF.same(a, b) for a, b in zip(seen['lone'], seen['bank']))
        took = {key: pipeline.calls[key] - before[key] for key in before}
        cell = {'equal_bits': bool(bits), 'calls': took, 'lone_ms': GF.stats(ms['lone']), 'bank_ms': GF.stats(ms['bank'])}
        cell['bank_against_lone'] = GF.compare(cell, 'lone_ms', 'bank_ms')
        res['cells'][str(B)] = cell
        ok = ok and bits and took['resident'] == 2 * B * n and took['composed'] == 0
        vc._fused_core().set_discard(0, 0)
        for p in lone:
            p.close()
        bank.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r33' / 'live_bank_bench.json'))
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    a = ap.parse_args()
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps), '--out', a.out]
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
