"""MI355X: the output gate against the host expression, per buffer.  Chunks of 24000 samples produced by pushes of 1 s at 24 kHz, an audible and a
silent signal, B = 1, 2, 4 and 8 streams, three arms per configuration --
    host   `host_mean_db` + slicing + scale + cast to float32 per stream (what a caller without the gate does in numpy)
    lone   B lone `OutputGate`s, one push each
    bank   one `OutputGateBank.push`
-- alternated round by round in one process after a warm-up; every call is timed on the host from entry to return (each completes its chunk, so
the return is after the last wait).  Reported: median, quartiles, min and max of ROUNDS rounds, in milliseconds per buffer of B streams.  No ratio
is promised: a direction is claimed only where the gap between two medians exceeds both arms' interquartile ranges (`separated`).
Writes profiles/r24/output_gate_bench.json.

    python scripts/output_gate_bench.py [--rounds 30] [--out FILE]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]

FS, CHUNK, THRESHOLD, SCALE = 24000, 24000, 80.0, 0.5


def stats(ms):
    a = numpy.sort(numpy.asarray(ms))
    q1, med, q3 = (float(numpy.percentile(a, p)) for p in (25, 50, 75))
    return dict(median_ms=med, q1_ms=q1, q3_ms=q3, min_ms=float(a[0]), max_ms=float(a[-1]), rounds=len(a))


def separated(a, b):
    gap = abs(a['median_ms'] - b['median_ms'])
    return bool(gap > a['q3_ms'] - a['q1_ms'] and gap > b['q3_ms'] - b['q1_ms'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r24' / 'output_gate_bench.json'))
    a = ap.parse_args()
    assert a.rounds >= 10
    import output_gate_cases as C
    from realtime_yukarin_amd import engine
    from realtime_yukarin_amd.output_gate import OutputGate, OutputGateBank, host_mean_db
    ctx = engine.get_context(0)
    results = []
    for kind in ('audible', 'silent'):
        for B in (1, 2, 4, 8):
            name = 'voiced' if kind == 'audible' else 'noise1e-6'
            # every round has buffers of its own: nothing is served from a cache of the previous round
            bufs = [[numpy.array(numpy.roll(C.signal(name, CHUNK), 17 * (r * B + b))) for b in range(B)] for r in range(a.rounds + a.warmup)]
            lone = [OutputGate(CHUNK, THRESHOLD, SCALE, numpy.float32, ctx=ctx) for _ in range(B)]
            bank = OutputGateBank(B, CHUNK, THRESHOLD, SCALE, numpy.float32, ctx=ctx)

            def host(waves):
                out = []
                for w in waves:
                    w = numpy.array(w)
                    w[numpy.isnan(w)] = 0
                    chunk = w[:CHUNK]
                    out.append(None if host_mean_db(chunk) < -THRESHOLD else (chunk * SCALE).astype(numpy.float32))
                return out
            arms = dict(host=host, lone=lambda waves: [g.push(w) for g, w in zip(lone, waves)], bank=bank.push)
            times = {k: [] for k in arms}
            for r in range(a.rounds + a.warmup):
                order = list(arms)
                order = order[r % 3:] + order[:r % 3]                # the arms take turns at going first
                outs = {}
                for k in order:
                    t0 = time.perf_counter()
                    outs[k] = arms[k](bufs[r])
                    dt = (time.perf_counter() - t0) * 1e3
                    if r >= a.warmup:
                        times[k].append(dt)
                for k in ('lone', 'bank'):                          # the arms agree, every round
                    assert all((x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()) for x, y in zip(outs[k], outs['host'])), (kind, B, r, k)
                assert all((o is None) == (kind == 'silent') for o in outs['bank'])
            st = {k: stats(v) for k, v in times.items()}
            row = dict(signal=kind, streams=B, chunk=CHUNK, arms=st,
                       bank_vs_host_separated=separated(st['bank'], st['host']), bank_vs_lone_separated=separated(st['bank'], st['lone']),
                       bank_counts=bank.counts())
            results.append(row)
            print('%-7s B=%d  host %.3f [%.3f, %.3f]  lone %.3f [%.3f, %.3f]  bank %.3f [%.3f, %.3f] ms  separated: host %s lone %s' % (
                kind, B, st['host']['median_ms'], st['host']['q1_ms'], st['host']['q3_ms'], st['lone']['median_ms'], st['lone']['q1_ms'], st['lone']['q3_ms'],
                st['bank']['median_ms'], st['bank']['q1_ms'], st['bank']['q3_ms'], row['bank_vs_host_separated'], row['bank_vs_lone_separated']), flush=True)
            bank.close()
            for g in lone:
                g.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(fs=FS, chunk=CHUNK, threshold_db=THRESHOLD, scale=SCALE, dtype='float32', rounds=a.rounds, warmup=a.warmup,
                                   timing='host perf_counter around each synchronous call, arms alternated per round', numpy=numpy.__version__,
                                   results=results), indent=1) + '\n')


if __name__ == '__main__':
    main()
