#!/usr/bin/env python3
"""A bank of live streams with the silence gate in front of the encode stage on one MI355X: medians and quartiles of alternated, device-synchronised
calls on the same windows -- `full` capacity, 24 kHz, 1.5 s windows advancing 0.5 s (301 frames at 5 ms), discard = (100, 100), SYN-64 predictors,
`f32` and `bf16x3`, B = 1, 4 and 8 streams of which none, half (B // 2; none at B = 1 is the same cell) and all are silent -- of two arms in one
process, and of a third in a process of its own:
  (off)    `PipelineBank.push(advance=a)` of this checkout with the flag off;
  (on)     `PipelineBank.push(advance=a, gate_first=True)`;
  (parent) `PipelineBank.push(advance=a)` of ANOTHER checkout -- the parent commit, built in its own tree and named with --parent -- the baseline:
           a worker process started from that tree, which builds the same windows and times its own calls; the three arms take turns window by
           window (the order rotates), so they share the session, the card and its clocks.  Next to (off) it shows whether the flag-off path moved.
A silent stream pushes digital zeros; the others a signal each without a pause (every frame of it is effective, so `none silent` means that in every
call).  Every stream's samples of all arms are checked for equal bits, call by call.  Prints one JSON object: per cell every arm's median, quartiles
and interquartile range, the waves the gate skipped per call, and per pair of arms the gap and whether it exceeds BOTH interquartile ranges or
NEITHER; writes it to --out.

    python scripts/pipeline_gate_first_bench.py --parent DIR [--reps 12] [--out profiles/r25/pipeline_gate_first_bench.json]
    (a child process under its own `timeout`; without --parent the third arm is left out and the JSON says so)
"""
import argparse
import hashlib
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = Path(sys.argv[sys.argv.index('--root') + 1]).resolve() if '--root' in sys.argv else ROOT      # the worker imports the package of another tree
sys.path[:0] = [str(PKG), str(PKG / 'scripts')]

import numpy  # noqa: E402

LIMIT_S = 840
FS, WINDOW, ADVANCE = 24000, 36000, 12000
BANKS = (1, 4, 8)
WARM = 3                                                               # windows before the timed ones: the first is computed in full


def stats(v):
    q = statistics.quantiles(v, n=4)
    return {'median': statistics.median(v), 'q1': q[0], 'q3': q[2], 'iqr': q[2] - q[0], 'min': min(v), 'max': max(v)}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(numpy.array_equal(a.view(numpy.uint8), b.view(numpy.uint8)))


def signal(n, seed=0):
    """`pipeline_bench.signal` without its digitally silent stretch: a gliding tone with a little noise, audible throughout."""
    rng = numpy.random.default_rng(seed)
    t = numpy.arange(n) / FS
    f = 180 + 50 * numpy.sin(2 * numpy.pi * t)
    return (0.3 * numpy.sin(2 * numpy.pi * numpy.cumsum(f) / FS) + rng.normal(0, 0.02, n)).astype(numpy.float32)


def digest(outs):
    h = hashlib.sha256()
    for o in outs:
        a = numpy.ascontiguousarray(o.wave)
        h.update(str((a.dtype, a.shape)).encode() + a.tobytes())
    return h.hexdigest()


def compare(cell, base, new):
    a, b = cell[base], cell[new]
    gap = a['median'] - b['median']
    return {'gap_ms': gap, 'ratio': b['median'] / a['median'], 'beyond_both_iqr': bool(abs(gap) > max(a['iqr'], b['iqr'])),
            'within_both_iqr': bool(abs(gap) <= min(a['iqr'], b['iqr']))}


def set_up(n_windows):
    """-> (voice changer, acoustic parameters, the signals, the `pipeline` and `crepe` shim modules) of the tree this process imports."""
    import pipeline_bench as PB
    from realtime_yukarin_amd import _lib, compat
    _lib.ensure_hw_queues()
    compat.install()
    from realtime_yukarin_amd import crepe, encode, pipeline
    from become_yukarin import SuperResolution
    from become_yukarin.config.sr_config import create_from_json as create_sr_config
    from yukarin import AcousticConverter
    from yukarin.config import create_from_json as create_config
    from yukarin.f0_converter import F0Converter
    from realtime_yukarin_amd.compat import crepe as shim
    from realtime_yukarin_amd.voice_changer import VoiceChanger
    sigs = [signal(WINDOW + ADVANCE * n_windows, 2 + s) for s in range(max(BANKS))]
    with tempfile.TemporaryDirectory() as tmp:
        d = Path(tmp)
        PB.write_models(d)
        crepe.save_weights(d / 'crepe.npz', crepe.synthetic_params('full', 0))
        shim.load_model(d / 'crepe.npz', 'full')
        f0c = F0Converter(input_statistics=d / 'in_stat.npy', target_statistics=d / 'tg_stat.npy')
        acv = AcousticConverter(create_config(d / 's1.json'), d / 's1.npz', f0_converter=f0c, out_sampling_rate=FS)
        sr = SuperResolution(create_sr_config(d / 's2.json'), d / 's2.npz')
    vc = VoiceChanger(acoustic_converter=acv, super_resolution=sr, threshold=60)
    pipeline.install()
    encode.model_capacity = 'full'
    return vc, acv.config.dataset.acoustic_param, sigs, pipeline, shim


def windows_of(sigs, B, silent, k):
    from yukarin import Wave
    zeros = numpy.zeros(WINDOW, numpy.float32)
    return [Wave(zeros if s >= B - silent else sigs[s][k * ADVANCE:k * ADVANCE + WINDOW], FS) for s in range(B)]


def worker(args):
    """The third arm: this script run from another tree (--root).  One JSON line in, one out: a cell opens a bank, a push times one call."""
    vc, param, sigs, pipeline, shim = set_up(args.reps + WARM)
    bank, cell = None, None
    print(json.dumps({'ready': str(PKG)}), flush=True)
    for line in sys.stdin:
        m = json.loads(line)
        if m['cmd'] == 'cell':
            shim._model('full').set_dtype(m['dtype'])
            cell = (m['B'], m['silent'])
            bank = pipeline.PipelineBank(vc, param, m['B'], seeds=list(range(1, m['B'] + 1)), crepe_capacity='full')
            print(json.dumps({'ok': True}), flush=True)
        elif m['cmd'] == 'push':
            waves = windows_of(sigs, cell[0], cell[1], m['k'])
            t0 = time.perf_counter()
            outs = bank.push(waves, discard=(100, 100), advance=ADVANCE)
            ms = 1e3 * (time.perf_counter() - t0)
            print(json.dumps({'ms': ms, 'digest': digest(outs)}), flush=True)
        elif m['cmd'] == 'close':
            vc._fused_core().set_discard(0, 0)
            bank.close()
            bank = None
            print(json.dumps({'ok': True}), flush=True)
        else:
            break
    return 0


class Parent(object):
    """The worker process over the parent's tree."""

    def __init__(self, root, reps):
        cmd = [sys.executable, str(Path(__file__).resolve()), '--worker', '--root', str(root), '--reps', str(reps)]
        self.p = subprocess.Popen(cmd, cwd=str(root), stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        self.root = self.ask(None)['ready']

    def ask(self, message):
        if message is not None:
            self.p.stdin.write(json.dumps(message) + '\n')
            self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError('the parent worker ended (status %s)' % self.p.poll())
        return json.loads(line)

    def close(self):
        try:
            self.p.stdin.write(json.dumps({'cmd': 'quit'}) + '\n')
            self.p.stdin.close()
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


def run(args):
    n_windows = args.reps + WARM
    vc, param, sigs, pipeline, shim = set_up(n_windows)
    parent = Parent(args.parent, args.reps) if args.parent else None
    res = {'what': 'ms per call, device-synchronised, the arms taking turns window by window: (off) PipelineBank.push(advance=a), (on) the same with '
                   'gate_first=True, (parent) PipelineBank.push(advance=a) of the parent commit in a worker process of its own tree',
           'parent_arm': bool(parent), 'capacity': 'full', 'fs': FS, 'window_samples': WINDOW, 'advance_samples': ADVANCE, 'discard': [100, 100],
           'reps': args.reps, 'cells': {}}
    ok = True
    try:
        for dtype in ('f32', 'bf16x3'):
            shim._model('full').set_dtype(dtype)
            for B in BANKS:
                for silent in sorted(set((0, B // 2, B))):
                    seeds = list(range(1, B + 1))
                    off, on = (pipeline.PipelineBank(vc, param, B, seeds=seeds, crepe_capacity='full', gate_first=g) for g in (False, True))
                    if parent:
                        parent.ask({'cmd': 'cell', 'dtype': dtype, 'B': B, 'silent': silent})
                    names = ['off', 'on'] + (['parent'] if parent else [])
                    ms, bits, gated = {name: [] for name in names}, True, set()
                    for k in range(n_windows):
                        waves = windows_of(sigs, B, silent, k)
                        turn = names[k % len(names):] + names[:k % len(names)]
                        seen = {}
                        for name in turn:
                            if name == 'parent':
                                got = parent.ask({'cmd': 'push', 'k': k})
                                t, seen[name] = got['ms'], got['digest']
                            else:
                                t0 = time.perf_counter()
                                outs = (off if name == 'off' else on).push(waves, discard=(100, 100), advance=ADVANCE)
                                t = 1e3 * (time.perf_counter() - t0)
                                seen[name] = digest(outs)
                            if k >= WARM:
                                ms[name].append(t)
                        bits = bits and len(set(seen.values())) == 1
                        gated.add(len(waves) - sum(on.last_gate['tracked']))
                    cell = {name + '_ms': stats(v) for name, v in ms.items()}
                    cell.update(streams=B, silent=silent, skipped_per_call=sorted(gated), same_bits=bool(bits),
                                on_against_off=compare(cell, 'off_ms', 'on_ms'))
                    if parent:
                        cell.update(off_against_parent=compare(cell, 'parent_ms', 'off_ms'), on_against_parent=compare(cell, 'parent_ms', 'on_ms'))
                        parent.ask({'cmd': 'close'})
                    ok = ok and bits and sorted(gated) == [silent]
                    res['cells']['%s_B%d_silent%d' % (dtype, B, silent)] = cell
                    print(json.dumps({'%s_B%d_silent%d' % (dtype, B, silent): cell}), file=sys.stderr, flush=True)
                    vc._fused_core().set_discard(0, 0)
                    off.close()
                    on.close()
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
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r25' / 'pipeline_gate_first_bench.json'))
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
