#!/usr/bin/env python3
"""B live streams, wave to wave, on one MI355X: B lone `Pipeline.push` calls per buffer (existing code, unchanged) against ONE `PipelineBank.push`
for all B, in the same process, alternated round by round after a warm-up.  B = 1, 2, 4, 8; every stream pushes a 1.5 s window (0.5 s buffer + 2 x
0.5 s overlap) with discard = (100, 100) at 24 kHz in and out, 5 ms frames; CREPE at `full` capacity and the SYN-64 predictors of bench.py (seeded
synthetic weights).  Every stream has a seed and a signal of its own.  Both arms must return the same bits for every stream in EVERY round (the script
exits with an error otherwise).  Prints one JSON object with the medians, the spreads (max - min) and the ratio bank / lone per B -- whatever comes
out, B = 1 included -- and writes it to --out.

    python scripts/pipeline_many_bench.py [--alternations 10] [--warmup 3] [--out profiles/r21/pipeline_many_bench.json]
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'scripts'))

import numpy  # noqa: E402

import pipeline_bench as single  # noqa: E402

FS, FRAME_PERIOD = single.FS, single.FRAME_PERIOD
STREAMS = (1, 2, 4, 8)
DISCARD = (100, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--alternations', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r21' / 'pipeline_many_bench.json'))
    args = ap.parse_args()
    from realtime_yukarin_amd import _lib, compat
    _lib.ensure_hw_queues()
    compat.install()
    from become_yukarin import SuperResolution
    from become_yukarin.config.sr_config import create_from_json as create_sr_config
    from yukarin import AcousticConverter, Wave
    from yukarin.config import create_from_json as create_config
    from yukarin.f0_converter import F0Converter
    from realtime_yukarin_amd import crepe, encode, pipeline
    from realtime_yukarin_amd.compat import crepe as shim
    from realtime_yukarin_amd.voice_changer import VoiceChanger
    with tempfile.TemporaryDirectory() as tmp:
        d = Path(tmp)
        single.write_models(d)
        crepe.save_weights(d / 'crepe.npz', crepe.synthetic_params('full', 0))
        shim.load_model(d / 'crepe.npz', 'full')
        f0c = F0Converter(input_statistics=d / 'in_stat.npy', target_statistics=d / 'tg_stat.npy')
        acv = AcousticConverter(create_config(d / 's1.json'), d / 's1.npz', f0_converter=f0c, out_sampling_rate=FS)
        sr = SuperResolution(create_sr_config(d / 's2.json'), d / 's2.npz')
    vc = VoiceChanger(acoustic_converter=acv, super_resolution=sr, threshold=60)
    param = acv.config.dataset.acoustic_param
    pipeline.install()
    encode.model_capacity = 'full'
    res = {'capacity': 'full', 'predictors': 'SYN-64', 'fs': FS, 'frame_period_ms': FRAME_PERIOD, 'window_s': 1.5, 'discard': list(DISCARD),
           'alternations': args.alternations, 'warmup': args.warmup, 'streams': {}}
    ok = True
    for B in STREAMS:
        seeds = list(range(1, B + 1))
        waves = [Wave(single.signal(3 * FS // 2, 10 + s), FS) for s in range(B)]
        lone = [pipeline.Pipeline(vc, param, crepe_capacity='full', seed=s) for s in seeds]
        bank = pipeline.PipelineBank(vc, param, B, seeds=seeds, crepe_capacity='full')
        before = (dict(pipeline.calls), dict(pipeline.calls_many))
        final = list(range(B))                                            # every round is a whole signal: both arms start from the same state

        def run_lone():
            return [p.push(w, discard=DISCARD, final=True).wave for p, w in zip(lone, waves)]

        def run_bank():
            return [w.wave for w in bank.push(waves, discard=DISCARD, final=final)]

        ms, same = {'lone': [], 'bank': []}, True
        for r in range(args.warmup + args.alternations):
            got = {}
            for arm, fn in (('lone', run_lone), ('bank', run_bank)):
                t0 = time.perf_counter()
                got[arm] = fn()
                if r >= args.warmup:
                    ms[arm].append(1e3 * (time.perf_counter() - t0))
            same = same and all(a.size > 0 and numpy.array_equal(a.view(numpy.uint64), b.view(numpy.uint64)) for a, b in zip(got['lone'], got['bank']))
        cell = {'samples_in_per_stream': int(waves[0].wave.size), 'samples_out_per_stream': int(got['bank'][0].size), 'same_bits_in_every_round': same,
                'lone_resident_calls': pipeline.calls['resident'] - before[0]['resident'], 'lone_composed_calls': pipeline.calls['composed'] - before[0]['composed'],
                'bank_resident_calls': pipeline.calls_many['resident'] - before[1]['resident'],
                'bank_composed_calls': pipeline.calls_many['composed'] - before[1]['composed']}
        for arm, v in ms.items():
            cell[arm + '_ms'] = {'median': statistics.median(v), 'spread': max(v) - min(v), 'min': min(v), 'max': max(v), 'all': v}
        cell['ratio_bank_to_lone'] = cell['bank_ms']['median'] / cell['lone_ms']['median']
        cell['bank_ms_per_stream'] = cell['bank_ms']['median'] / B
        cell['lone_ms_per_stream'] = cell['lone_ms']['median'] / B
        res['streams'][str(B)] = cell
        ok = ok and same and cell['lone_composed_calls'] == 0 and cell['bank_composed_calls'] == 0
        bank.close()
        for p in lone:
            p.close()
    text = json.dumps(res, indent=1)
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text + '\n')
    if not ok:
        sys.exit('the two arms differ in some round, or a call took the composed path')


if __name__ == '__main__':
    main()
