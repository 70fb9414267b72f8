#!/usr/bin/env python3
"""A bank of live streams behind a bank of output gates on one MI355X, with the synthesized samples brought to the gate through the host or left
on the card: medians and quartiles of alternated calls on the same windows -- `full` capacity, 24 kHz, 1.5 s windows advancing 0.5 s (301 frames
at 5 ms), discard = (100, 100), SYN-64 predictors, gate chunk 12000, float32 out, `f32` and `bf16x3` CREPE, B = 1, 4 and 8 streams, all audible or
all silent (digital zeros in, and a gate threshold that calls every chunk silent) -- of two arms in one process, and of a third in a process of its own:
  (host)   `PipelineBank.push(advance=a, out_gate=G)` of this checkout with the device route switched off (`pipeline._gate_on_card` answers no);
  (device) the same call on the device route;
  (parent) `PipelineBank.push(advance=a, out_gate=G)` of ANOTHER checkout -- the parent commit, built in its own tree and named with --parent --:
           a worker process started from that tree, which builds the same windows and times its own calls.
The arms take turns window by window (the order rotates), so they share the session, the card and its clocks.  Every stream's chunks of all arms
are checked for equal bits, call by call.  The PCIe bytes of a call are read from the counters, not from the timings: the gate's upload bytes and
`sample_bytes_down`, and 8 bytes per synthesized sample down on the host route.  Prints one JSON object: per cell every arm's median, quartiles and
interquartile range, and per pair of arms the gap and whether it exceeds BOTH interquartile ranges or lies within both; writes it to --out.

    python scripts/pipeline_out_gate_bench.py --parent DIR [--reps 12] [--out profiles/r30/pipeline_out_gate_bench.json]
    (a child process under its own `timeout`; without --parent the third arm is left out and the JSON says so)
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = Path(sys.argv[sys.argv.index('--root') + 1]).resolve() if '--root' in sys.argv else ROOT      # the worker imports the package of another tree
sys.path[:0] = [str(PKG), str(PKG / 'scripts')]

import numpy  # noqa: E402

import pipeline_gate_first_bench as GF  # noqa: E402  (the windows, the models, the statistics)

LIMIT_S = 1100
CHUNK, THRESHOLD, SCALE = 12000, 60.0, 0.5
WARM = GF.WARM


def gates_of(B, silent=False):
    """silent: a threshold below which every chunk lies (the synthesizer turns digital zeros into shaped noise, which a gate at 60 dB calls audible):
    the gate computes and judges every chunk and calls it silent."""
    from realtime_yukarin_amd import output_gate
    return output_gate.OutputGateBank(B, CHUNK, -1e9 if silent else THRESHOLD, SCALE, numpy.float32)


def windows_of(sigs, B, silent, k):
    return GF.windows_of(sigs, B, B if silent else 0, k)


def worker(args):
    """The third arm: this script run from another tree (--root).  One JSON line in, one out: a cell opens a bank, a push times one call."""
    vc, param, sigs, pipeline, shim = GF.set_up(args.reps + WARM)
    bank = gates = cell = None
    print(json.dumps({'ready': str(PKG)}), flush=True)
    for line in sys.stdin:
        m = json.loads(line)
        if m['cmd'] == 'cell':
            shim._model('full').set_dtype(m['dtype'])
            cell = (m['B'], m['silent'])
            bank = pipeline.PipelineBank(vc, param, m['B'], seeds=list(range(1, m['B'] + 1)), crepe_capacity='full')
            gates = gates_of(m['B'], m['silent'])
            print(json.dumps({'ok': True}), flush=True)
        elif m['cmd'] == 'push':
            waves = windows_of(sigs, cell[0], cell[1], m['k'])
            t0 = time.perf_counter()
            outs = bank.push(waves, discard=(100, 100), advance=GF.ADVANCE, out_gate=gates)
            ms = 1e3 * (time.perf_counter() - t0)
            print(json.dumps({'ms': ms, 'digest': GF.digest(outs)}), flush=True)
        elif m['cmd'] == 'close':
            vc._fused_core().set_discard(0, 0)
            bank.close()
            gates.close()
            bank = gates = None
            print(json.dumps({'ok': True}), flush=True)
        else:
            break
    return 0


class Parent(GF.Parent):
    def __init__(self, root, reps):
        cmd = [sys.executable, str(Path(__file__).resolve()), '--worker', '--root', str(root), '--reps', str(reps)]
        self.p = subprocess.Popen(cmd, cwd=str(root), stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        self.root = self.ask(None)['ready']


def run(args):
    n_windows = args.reps + WARM
    vc, param, sigs, pipeline, shim = GF.set_up(n_windows)
    parent = Parent(args.parent, args.reps) if args.parent else None
    on_card = pipeline._gate_on_card
    res = {'what': 'ms per call, the arms taking turns window by window: PipelineBank.push(advance=a, out_gate=G) with the samples through the host '
                   '(host), left on the card (device), and of the parent commit in a worker process of its own tree (parent); pcie_bytes_per_call: '
                   'from the counters -- the gate\'s one upload, the emitted chunks down, and 8 bytes per synthesized sample down on the host route '
                   '(which that route then sends up again inside the gate\'s upload)',
           'parent_arm': bool(parent), 'capacity': 'full', 'fs': GF.FS, 'window_samples': GF.WINDOW, 'advance_samples': GF.ADVANCE, 'discard': [100, 100],
           'chunk': CHUNK, 'out_dtype': 'float32', 'reps': args.reps, 'cells': {}}
    ok = True
    try:
        for dtype in ('f32', 'bf16x3'):
            shim._model('full').set_dtype(dtype)
            for B in GF.BANKS:
                for silent in (False, True):
                    seeds = list(range(1, B + 1))
                    banks = {name: pipeline.PipelineBank(vc, param, B, seeds=seeds, crepe_capacity='full') for name in ('host', 'device')}
                    gates = {name: gates_of(B, silent) for name in banks}
                    if parent:
                        parent.ask({'cmd': 'cell', 'dtype': dtype, 'B': B, 'silent': silent})
                    names = ['host', 'device'] + (['parent'] if parent else [])
                    ms, bits, routed, verdicts = {name: [] for name in names}, True, True, set()
                    pcie = {name: {'gate_up': [], 'chunks_down': [], 'synth_down': []} for name in banks}
                    held = {name: 0 for name in banks}
                    for k in range(n_windows):
                        waves = windows_of(sigs, B, silent, k)
                        turn = names[k % len(names):] + names[:k % len(names)]
                        seen = {}
                        for name in turn:
                            if name == 'parent':
                                got = parent.ask({'cmd': 'push', 'k': k})
                                t, seen[name] = got['ms'], got['digest']
                            else:
                                pipeline._gate_on_card = on_card if name == 'device' else (lambda gate, ctx: False)
                                before = dict(pipeline.routes)
                                t0 = time.perf_counter()
                                outs = banks[name].push(waves, discard=(100, 100), advance=GF.ADVANCE, out_gate=gates[name])
                                t = 1e3 * (time.perf_counter() - t0)
                                pipeline._gate_on_card = on_card
                                seen[name] = GF.digest(outs)
                                routed = routed and pipeline.routes['gate_' + name] == before['gate_' + name] + 1
                                c, g = gates[name].counts(), gates[name]
                                now = sum(g.held(s) for s in range(B))
                                samples = now + CHUNK * sum(1 for s in range(B) if g.last[s][0]) - held[name]
                                held[name] = now
                                verdicts.update(r[1] for r in g.last if r[0])
                                if k >= WARM:
                                    pcie[name]['gate_up'].append(c['upload_bytes'])
                                    pcie[name]['chunks_down'].append(c['sample_bytes_down'])
                                    pcie[name]['synth_down'].append(0 if name == 'device' else 8 * samples)
                            if k >= WARM:
                                ms[name].append(t)
                        bits = bits and len(set(seen.values())) == 1
                    cell = {name + '_ms': GF.stats(v) for name, v in ms.items()}
                    cell.update(streams=B, silent=bool(silent), chunks_judged_silent=sorted(verdicts), same_bits=bool(bits), routes_as_named=bool(routed),
                                pcie_bytes_per_call={name: {key: GF.statistics.median(v) for key, v in d.items()} for name, d in pcie.items()},
                                device_against_host=GF.compare(cell, 'host_ms', 'device_ms'))
                    if parent:
                        cell.update(host_against_parent=GF.compare(cell, 'parent_ms', 'host_ms'), device_against_parent=GF.compare(cell, 'parent_ms', 'device_ms'))
                        parent.ask({'cmd': 'close'})
                    ok = ok and bits and routed and verdicts == {bool(silent)}
                    key = '%s_B%d_%s' % (dtype, B, 'silent' if silent else 'audible')
                    res['cells'][key] = cell
                    print(json.dumps({key: cell}), file=sys.stderr, flush=True)
                    vc._fused_core().set_discard(0, 0)
                    for name in banks:
                        banks[name].close()
                        gates[name].close()
    finally:
        if parent:
            parent.close()
    res['same_bits'] = all(c['same_bits'] for c in res['cells'].values())
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r30' / 'pipeline_out_gate_bench.json'))
    ap.add_argument('--parent', default=None, help='the built tree of the parent commit: the baseline arm')
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    ap.add_argument('--worker', action='store_true', help='the baseline arm: started by the measurement from the tree named by --root')
    ap.add_argument('--root', default=None)
    a = ap.parse_args()
    if a.worker:
        sys.exit(worker(a))
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps), '--out', a.out]
    if a.parent:
        cmd += ['--parent', str(Path(a.parent).resolve())]
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
