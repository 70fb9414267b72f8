#!/usr/bin/env python3
"""A bank of live streams with and without kept activation rows on one MI355X: medians of alternated, device-synchronised calls on the same windows
-- `full` capacity, 24 kHz, 1.5 s windows advancing 0.5 s (301 frames at 5 ms), discard = (100, 100), SYN-64 predictors, B = 1, 2, 4, 8 streams
with a signal each, `f32` and `bf16x3` -- of three arms in one process:
  (a) `PipelineBank.push` without `advance`: the path this work leaves unchanged, the yardstick;
  (b) `PipelineBank.push(advance=a)`: one chain per buffer, the tracks through a `CrepeStreamBank`;
  (c) B lone `Pipeline.push(advance=a)`, one after the other.
and of the tracker alone, `CrepeModel.track_many` against `CrepeStreamBank.track_many` (host results, so both wait for the device).  Every stream's
samples of (a), (b) and (c) are checked for equal bits, call by call.  Prints one JSON object with every arm's median and spread (max - min), the
computed / frames of every stream in (b), and per pair of arms whether the gap exceeds the sum of both spreads; writes it to --out.

    python scripts/pipeline_bank_stream_bench.py [--reps 12] [--out profiles/r23/pipeline_bank_stream_bench.json]   a child process under its own `timeout`
"""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'scripts')]

import numpy  # noqa: E402

LIMIT_S = 540
FS, WINDOW, ADVANCE, HOP, STEP = 24000, 36000, 12000, 80, 5
BANKS = (1, 2, 4, 8)
WARM = 3                                                               # windows before the timed ones: the first is computed in full


def stats(v):
    return {'median': statistics.median(v), 'spread': max(v) - min(v), 'min': min(v), 'max': max(v)}


def verdict(cell, base, new):
    gap = cell[base]['median'] - cell[new]['median']
    return {'gap_ms': gap, 'beyond_both_spreads': bool(abs(gap) > cell[base]['spread'] + cell[new]['spread']),
            'ratio': cell[new]['median'] / cell[base]['median']}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(numpy.array_equal(a.view(numpy.uint8), b.view(numpy.uint8)))


def run(args):
    import pipeline_bench as PB
    from realtime_yukarin_amd import _lib, compat
    _lib.ensure_hw_queues()
    compat.install()
    from realtime_yukarin_amd import crepe, encode, pipeline
    from become_yukarin import SuperResolution
    from become_yukarin.config.sr_config import create_from_json as create_sr_config
    from yukarin import AcousticConverter, Wave
    from yukarin.config import create_from_json as create_config
    from yukarin.f0_converter import F0Converter
    from realtime_yukarin_amd.compat import crepe as shim
    from realtime_yukarin_amd.voice_changer import VoiceChanger
    n_windows = args.reps + WARM
    sigs = [PB.signal(WINDOW + ADVANCE * n_windows, 2 + s) for s in range(max(BANKS))]
    window = lambda s, k: sigs[s][k * ADVANCE:k * ADVANCE + WINDOW]
    res = {'what': 'ms per call, device-synchronised, alternated: (a) PipelineBank.push, (b) PipelineBank.push(advance=a), (c) B lone '
                   'Pipeline.push(advance=a); track alone: CrepeModel.track_many against CrepeStreamBank.track_many',
           'capacity': 'full', 'fs': FS, 'window_samples': WINDOW, 'advance_samples': ADVANCE, 'discard': [100, 100], 'reps': args.reps, 'cells': {}}
    P = crepe.synthetic_params('full', 0)
    with tempfile.TemporaryDirectory() as tmp:
        d = Path(tmp)
        PB.write_models(d)
        crepe.save_weights(d / 'crepe.npz', P)
        shim.load_model(d / 'crepe.npz', 'full')
        f0c = F0Converter(input_statistics=d / 'in_stat.npy', target_statistics=d / 'tg_stat.npy')
        acv = AcousticConverter(create_config(d / 's1.json'), d / 's1.npz', f0_converter=f0c, out_sampling_rate=FS)
        sr = SuperResolution(create_sr_config(d / 's2.json'), d / 's2.npz')
    vc = VoiceChanger(acoustic_converter=acv, super_resolution=sr, threshold=60)
    param = acv.config.dataset.acoustic_param
    pipeline.install()
    encode.model_capacity = 'full'
    ok = True
    for dtype in ('f32', 'bf16x3'):
        model = shim._model('full')
        model.set_dtype(dtype)
        for B in BANKS:
            seeds = list(range(1, B + 1))
            plain, kept = (pipeline.PipelineBank(vc, param, B, seeds=seeds, crepe_capacity='full') for _ in range(2))
            lone = [pipeline.Pipeline(vc, param, crepe_capacity='full', seed=s) for s in seeds]
            trackers = crepe.CrepeStreamBank(model, B)
            before = (dict(pipeline.calls_many), dict(pipeline.calls))
            ms = {k: [] for k in ('a_push', 'b_push_advance', 'c_lone_push_advance', 'a_track_many', 'b_bank_track_many')}
            bits, computed = True, set()
            for k in range(n_windows):
                xs = [window(s, k) for s in range(B)]
                waves = [Wave(x, FS) for x in xs]
                t0 = time.perf_counter()
                a = plain.push(waves, discard=(100, 100))
                t1 = time.perf_counter()
                b = kept.push(waves, discard=(100, 100), advance=ADVANCE)
                t2 = time.perf_counter()
                c = [p.push(w, discard=(100, 100), advance=ADVANCE) for p, w in zip(lone, waves)]
                t3 = time.perf_counter()
                ta = model.track_many(xs, FS, HOP, STEP, device=False)
                t4 = time.perf_counter()
                tb, _ = trackers.track_many(xs, FS, HOP, STEP, advances=ADVANCE, device=False)
                t5 = time.perf_counter()
                bits = bits and all(same(p.wave, q.wave) and same(p.wave, r.wave) for p, q, r in zip(a, b, c))
                bits = bits and all(same(u, v) for p, q in zip(ta, tb) for u, v in zip(p, q))
                if k >= WARM:
                    for key, t in zip(ms, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                        ms[key].append(1e3 * t)
                    computed.add(tuple(kept._crepe_bank.computed))
            cell = {key + '_ms': stats(v) for key, v in ms.items()}
            cell.update(computed_per_stream=sorted(list(c) for c in computed), frames_per_stream=list(kept._crepe_bank.frames), same_bits=bool(bits),
                        composed_calls=pipeline.calls_many['composed'] - before[0]['composed'] + pipeline.calls['composed'] - before[1]['composed'],
                        b_against_a=verdict(cell, 'a_push_ms', 'b_push_advance_ms'), b_against_c=verdict(cell, 'c_lone_push_advance_ms', 'b_push_advance_ms'),
                        track_b_against_a=verdict(cell, 'a_track_many_ms', 'b_bank_track_many_ms'))
            ok = ok and bits and cell['composed_calls'] == 0
            res['cells']['%s_B%d' % (dtype, B)] = cell
            print(json.dumps({'%s_B%d' % (dtype, B): cell}), file=sys.stderr, flush=True)
            vc._fused_core().set_discard(0, 0)
            trackers.close()
            for p in [plain, kept] + lone:
                p.close()
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
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r23' / 'pipeline_bank_stream_bench.json'))
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    a = ap.parse_args()
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps), '--out', a.out]
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
