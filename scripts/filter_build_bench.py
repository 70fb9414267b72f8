#!/usr/bin/env python3
"""What a live user meets before the first window: the wall time of creating the two SYN-64 predictors, of the first convert of a 300-frame window
(RY_WINOGRAD at its default: the window's plans take the Winograd layers, whose filters are built then) and of the tenth, in three arms that take turns:
  (parent) the parent commit, built in its own tree and named with --parent;
  (host)   this tree with the filter build mode 'host' (the default);
  (device) this tree with the filter build mode 'device'.
Every sample is a fresh child process under its own time limit (a start-up cost is paid once per process: nothing of it can be measured in a loop);
a child that fails ends the run.  Prints one JSON object -- per arm and figure the median, quartiles and interquartile range, and the three claims of
DESIGN.md section 23 checked against BOTH interquartile ranges -- and writes it to --out.

    python scripts/filter_build_bench.py --parent DIR [--samples 10] [--out profiles/r29/filter_build_bench.json]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
FRAMES = 300
CHILD_LIMIT_S = 180


def child(root, arm):
    """one sample, in the tree `root`: -> one JSON line"""
    sys.path.insert(0, str(root))
    import numpy
    from realtime_yukarin_amd import _lib, engine, synth
    from realtime_yukarin_amd.weights import flatten_params
    _lib.ensure_hw_queues()
    ctx = engine.get_context(0)
    if arm != 'parent':
        engine.set_filter_build(arm)
    (d1, P1), (d2, P2) = synth.model_params('SYN-64')
    b1, b2 = flatten_params(d1, P1), flatten_params(d2, P2)
    x1 = synth.stage1_input(FRAMES)
    x2 = synth.stage2_input(FRAMES)
    ctx.sync()
    t0 = time.perf_counter()
    n1 = engine.Net(ctx, d1, b1)
    n2 = engine.Net(ctx, d2, b2)
    ctx.sync()
    t_create = time.perf_counter() - t0
    times, y = [], None
    for i in range(10):
        t0 = time.perf_counter()
        n1.convert(x1)
        y = n2.convert(x2)
        times.append(time.perf_counter() - t0)
    out = dict(arm=arm, create_ms=1e3 * t_create, first_ms=1e3 * times[0], tenth_ms=1e3 * times[9], finite=bool(numpy.isfinite(y).all()),
               digest=int(numpy.ascontiguousarray(y).view(numpy.uint32).sum(dtype=numpy.uint64)))
    if arm != 'parent':
        out['stats'] = n2.build_stats()
    print('SAMPLE ' + json.dumps(out), flush=True)
    n1.close(); n2.close()


def stats(v):
    q = statistics.quantiles(v, n=4)
    return {'median': statistics.median(v), 'q1': q[0], 'q3': q[2], 'iqr': q[2] - q[0], 'min': min(v), 'max': max(v), 'n': len(v)}


def compare(a, b):
    """b against a: the gap of the medians and where it lies against both interquartile ranges"""
    gap = a['median'] - b['median']
    return {'gap_ms': gap, 'ratio': b['median'] / a['median'], 'beyond_both_iqr': bool(abs(gap) > max(a['iqr'], b['iqr'])),
            'within_both_iqr': bool(abs(gap) <= min(a['iqr'], b['iqr']))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help='tree of the parent commit, built')
    ap.add_argument('--samples', type=int, default=10)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r29' / 'filter_build_bench.json'))
    ap.add_argument('--child', help=argparse.SUPPRESS)
    ap.add_argument('--root', default=str(ROOT), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(Path(args.root).resolve(), args.child)
    arms = (['parent'] if args.parent else []) + ['host', 'device']
    samples = {a: [] for a in arms}
    for s in range(args.samples):
        for k in range(len(arms)):
            arm = arms[(s + k) % len(arms)]                               # the order rotates
            root = Path(args.parent).resolve() if arm == 'parent' else ROOT
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), '--child', arm, '--root', str(root)], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, timeout=CHILD_LIMIT_S, text=True)
            line = [q for q in r.stdout.splitlines() if q.startswith('SAMPLE ')]
            if r.returncode != 0 or not line:
                print(r.stdout[-4000:])
                raise SystemExit('the %s child of sample %d failed (exit status %s): nothing more is started' % (arm, s, r.returncode))
            samples[arm].append(json.loads(line[0][7:]))
            print('sample %d %-6s create %8.1f ms  first %8.1f ms  tenth %7.2f ms' % (s, arm, samples[arm][-1]['create_ms'], samples[arm][-1]['first_ms'],
                                                                                     samples[arm][-1]['tenth_ms']), flush=True)
    res = {'model': 'SYN-64', 'frames': FRAMES, 'samples': args.samples, 'arms': {}, 'claims': {}}
    for a in arms:
        assert all(q['finite'] for q in samples[a]) and len({q['digest'] for q in samples[a]}) == 1, a
        res['arms'][a] = {f: stats([q[f] for q in samples[a]]) for f in ('create_ms', 'first_ms', 'tenth_ms')}
        if 'stats' in samples[a][0]:
            res['arms'][a]['build_stats_stage2'] = samples[a][0]['stats']
    res['same_bits_all_arms'] = len({q['digest'] for a in arms for q in samples[a]}) == 1
    A = res['arms']
    if args.parent:
        res['claims']['host_mode_equals_parent'] = {f: compare(A['parent'][f], A['host'][f]) for f in ('create_ms', 'first_ms', 'tenth_ms')}
    res['claims']['device_below_host'] = {f: compare(A['host'][f], A['device'][f]) for f in ('create_ms', 'first_ms')}
    res['claims']['tenth_window_equal'] = compare(A['host']['tenth_ms'], A['device']['tenth_ms'])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
