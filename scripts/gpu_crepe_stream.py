#!/usr/bin/env python3
"""The streaming tracker on one MI355X against the shipped call: medians of alternated, device-synchronised `CrepeModel.track` and `CrepeStream.track`
calls on the same windows -- `full` capacity, 24 kHz, 1.5 s windows advancing 0.5 s over one fixed signal (301 frames at 5 ms), `f32` and `bf16x3` --
and the same for `Pipeline.push` without and with `advance` (SYN-64 predictors, discard = (100, 100)).  The yardstick is `model.track` /
`push(advance=None)` in the same run: the code path this work leaves unchanged.  Every pair is checked for equal bits.  Prints one JSON object with
both arms, their spreads (max - min), computed / frames of the stream arm and the same-bits flags, and writes it to --out.

    python scripts/gpu_crepe_stream.py [--reps 30] [--out profiles/r22/crepe_stream_bench.json]      as a child process under its own `timeout`
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


def stats(v):
    return {'median': statistics.median(v), 'spread': max(v) - min(v), 'min': min(v), 'max': max(v)}


def verdict(cell, base, new):
    gap = cell[base]['median'] - cell[new]['median']
    cell['gap_ms'] = gap
    cell['beyond_both_spreads'] = bool(gap > cell[base]['spread'] + cell[new]['spread'])
    cell['ratio'] = cell[new]['median'] / cell[base]['median']


def bits_equal(a, b):
    return all(p.dtype == q.dtype and p.shape == q.shape and numpy.array_equal(p.view(numpy.uint8), q.view(numpy.uint8)) for p, q in zip(a, b))


def run(args):
    import pipeline_bench as PB
    from realtime_yukarin_amd import _lib, compat
    _lib.ensure_hw_queues()
    compat.install()
    from realtime_yukarin_amd import crepe, encode, engine, pipeline
    ctx = engine.get_context(0)
    n_windows = args.reps + 3
    sig = PB.signal(WINDOW + ADVANCE * n_windows, 2)
    windows = [sig[k * ADVANCE:k * ADVANCE + WINDOW] for k in range(n_windows)]
    res = {'what': 'ms per call, device-synchronised, alternated: CrepeModel.track against CrepeStream.track, Pipeline.push without against with advance',
           'capacity': 'full', 'fs': FS, 'window_samples': WINDOW, 'advance_samples': ADVANCE, 'reps': args.reps, 'tracker': {}, 'push': {}}
    P = crepe.synthetic_params('full', 0)
    for dtype in ('f32', 'bf16x3'):
        model, other = crepe.CrepeModel('full', params=P, dtype=dtype), crepe.CrepeModel('full', params=P, dtype=dtype)
        stream = crepe.CrepeStream(other)
        ms, same, computed = {'track': [], 'stream': []}, True, []
        for k, x in enumerate(windows):
            t0 = time.perf_counter()
            want = model.track(x, FS, HOP, STEP)
            t1 = time.perf_counter()
            got = stream.track(x, FS, HOP, STEP, advance=ADVANCE if k else None)
            t2 = time.perf_counter()
            same = same and bits_equal(want, got)
            if k >= 3:                                                 # warm-up: three windows, the first of them computed in full
                ms['track'].append(1e3 * (t1 - t0))
                ms['stream'].append(1e3 * (t2 - t1))
                computed.append(stream.computed)
        cell = {'track_ms': stats(ms['track']), 'stream_ms': stats(ms['stream']), 'computed': sorted(set(computed)), 'frames': stream.frames,
                'same_bits': bool(same)}
        verdict(cell, 'track_ms', 'stream_ms')
        res['tracker'][dtype] = cell
        print(json.dumps({dtype: cell}), file=sys.stderr, flush=True)
        stream.close(); model.close(); other.close()
    # the whole push: two pipelines over one voice changer, alternated window by window
    from become_yukarin import SuperResolution
    from become_yukarin.config.sr_config import create_from_json as create_sr_config
    from yukarin import AcousticConverter, Wave
    from yukarin.config import create_from_json as create_config
    from yukarin.f0_converter import F0Converter
    from realtime_yukarin_amd.compat import crepe as shim
    from realtime_yukarin_amd.voice_changer import VoiceChanger
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
    for dtype in ('f32', 'bf16x3'):
        shim._model('full').set_dtype(dtype)
        plain, streamed = pipeline.Pipeline(vc, param, crepe_capacity='full', seed=1), pipeline.Pipeline(vc, param, crepe_capacity='full', seed=1)
        before = dict(pipeline.calls)
        ms, same, computed = {'push': [], 'push_advance': []}, True, []
        for k, x in enumerate(windows):
            w = Wave(x, FS)
            t0 = time.perf_counter()
            want = plain.push(w, discard=(100, 100)).wave
            t1 = time.perf_counter()
            got = streamed.push(w, discard=(100, 100), advance=ADVANCE).wave
            t2 = time.perf_counter()
            same = same and bits_equal([want], [got])
            if k >= 3:
                ms['push'].append(1e3 * (t1 - t0))
                ms['push_advance'].append(1e3 * (t2 - t1))
                computed.append(streamed._crepe_stream.computed)
        cell = {'push_ms': stats(ms['push']), 'push_advance_ms': stats(ms['push_advance']), 'computed': sorted(set(computed)),
                'frames': streamed._crepe_stream.frames, 'same_bits': bool(same),
                'composed_calls': pipeline.calls['composed'] - before['composed']}
        verdict(cell, 'push_ms', 'push_advance_ms')
        res['push'][dtype] = cell
        print(json.dumps({dtype: cell}), file=sys.stderr, flush=True)
        plain.close(); streamed.close()
    res['same_bits'] = all(c['same_bits'] for part in ('tracker', 'push') for c in res[part].values())
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + '\n')
    return 0 if res['same_bits'] and all(c['composed_calls'] == 0 for c in res['push'].values()) else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r22' / 'crepe_stream_bench.json'))
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    a = ap.parse_args()
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps), '--out', a.out]
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
