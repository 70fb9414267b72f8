#!/usr/bin/env python3
"""A wave in, a wave out on one MI355X: `Pipeline.convert_wave` / `push` (the feature rows stay on the card) against the chain of the separate calls
(`encode.extract` -> `VoiceChanger.convert_from_acoustic_feature` -> `world_synth.decode` / `Synthesizer.push`: unchanged code) in the same process,
alternated call by call after a warm-up.  Both arms run CREPE at `full` capacity and the SYN-64 predictors of bench.py (seeded synthetic weights: no
trained ones exist here), 24 kHz in and out, 5 ms frames.  Two configurations: `one_second` -- convert_wave on 1 s; `window` -- push of a 1.5 s
window (0.5 s buffer + 2 x 0.5 s overlap) with discard = (100, 100).  Checks that both arms return the same bits, prints one JSON object with the
medians, the spreads (max - min) and the ratio resident / chain, and writes it to --out.

    python scripts/pipeline_bench.py [--alternations 10] [--warmup 3] [--out profiles/r20/pipeline_bench.json]
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy  # noqa: E402

FS, FRAME_PERIOD, ORDER = 24000, 5, 8


def signal(n, seed=0):
    rng = numpy.random.default_rng(seed)
    t = numpy.arange(n) / FS
    f = 180 + 50 * numpy.sin(2 * numpy.pi * t)
    x = 0.3 * numpy.sin(2 * numpy.pi * numpy.cumsum(f) / FS) + rng.normal(0, 0.02, n)
    x[n // 2:n // 2 + n // 5] = 0                                     # a digitally silent stretch: the gate cuts frames
    return x.astype(numpy.float32)


def write_models(d):
    from realtime_yukarin_amd import synth
    from realtime_yukarin_amd.weights import save_npz
    (d1, P1), (d2, P2) = synth.model_params('SYN-64')
    save_npz(d / 's1.npz', P1)
    save_npz(d / 's2.npz', P2)
    (d / 's1.json').write_text(json.dumps({
        'dataset': {'acoustic_param': {'sampling_rate': FS, 'frame_period': FRAME_PERIOD, 'order': ORDER, 'alpha': 0.466},
                    'in_features': ['mc'], 'out_features': ['mc']},
        'model': {'in_channels': ORDER + 1, 'out_channels': ORDER + 1, 'generator_base_channels': d1.base, 'generator_extensive_layers': 8}}))
    (d / 's2.json').write_text(json.dumps({
        'dataset': {'param': {'voice_param': {'sample_rate': FS}, 'acoustic_feature_param': {'frame_period': FRAME_PERIOD, 'order': ORDER}}},
        'model': {'generator_base_channels': d2.base, 'generator_extensive_layers': 8}}))
    numpy.save(str(d / 'in_stat.npy'), {'mean': numpy.log(200.0), 'var': 0.04})
    numpy.save(str(d / 'tg_stat.npy'), {'mean': numpy.log(300.0), 'var': 0.09})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--alternations', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r20' / 'pipeline_bench.json'))
    args = ap.parse_args()
    from realtime_yukarin_amd import _lib, compat
    _lib.ensure_hw_queues()
    compat.install()
    from become_yukarin import SuperResolution
    from become_yukarin.config.sr_config import create_from_json as create_sr_config
    from yukarin import AcousticConverter, Wave
    from yukarin.config import create_from_json as create_config
    from yukarin.f0_converter import F0Converter
    from realtime_yukarin_amd import crepe, encode, pipeline, world_synth
    from realtime_yukarin_amd.compat import crepe as shim
    from realtime_yukarin_amd.voice_changer import VoiceChanger
    with tempfile.TemporaryDirectory() as tmp:
        d = Path(tmp)
        write_models(d)
        crepe.save_weights(d / 'crepe.npz', crepe.synthetic_params('full', 0))
        shim.load_model(d / 'crepe.npz', 'full')
        f0c = F0Converter(input_statistics=d / 'in_stat.npy', target_statistics=d / 'tg_stat.npy')
        acv = AcousticConverter(create_config(d / 's1.json'), d / 's1.npz', f0_converter=f0c, out_sampling_rate=FS)
        sr = SuperResolution(create_sr_config(d / 's2.json'), d / 's2.npz')
    vc = VoiceChanger(acoustic_converter=acv, super_resolution=sr, threshold=60)
    param = acv.config.dataset.acoustic_param
    pipeline.install()
    encode.model_capacity = 'full'
    pipe = pipeline.Pipeline(vc, param, crepe_capacity='full', seed=1)
    cls = pipe.feature_class
    chain_synth = world_synth.Synthesizer(FS, FRAME_PERIOD, seed=1)
    vocoder = types.SimpleNamespace(out_sampling_rate=FS, acoustic_param=param, _ry_synth=chain_synth)
    eargs = dict(frame_period=param.frame_period, f0_floor=param.f0_floor, f0_ceil=param.f0_ceil, fft_length=param.fft_length, order=param.order,
                 alpha=param.alpha, dtype=param.dtype)

    def chain_feature(wave, discard):
        f = encode.extract(cls, wave, **eargs)
        f.wave = wave
        return vc.convert_from_acoustic_feature(f, discard)

    def chain_convert(wave):
        return world_synth.decode(vocoder, chain_feature(wave, (0, 0))).wave

    def chain_window(wave):
        out = chain_feature(wave, (100, 100))
        k1 = len(out.f0) - 100
        got = chain_synth.push(numpy.asarray(out.f0).ravel()[100:k1], out.sp[100:k1], out.ap[100:k1])
        return numpy.concatenate([got, chain_synth.flush()])

    configs = {
        'one_second': (Wave(signal(FS), FS), chain_convert, lambda w: pipe.convert_wave(w).wave),
        'window': (Wave(signal(3 * FS // 2, 1), FS), chain_window, lambda w: pipe.push(w, discard=(100, 100), final=True).wave),
    }
    res = {'capacity': 'full', 'predictors': 'SYN-64', 'fs': FS, 'frame_period_ms': FRAME_PERIOD, 'alternations': args.alternations,
           'warmup': args.warmup, 'configs': {}}
    for name, (wave, chain, resident) in configs.items():
        before = dict(pipeline.calls)
        for _ in range(args.warmup):
            want, got = chain(wave), resident(wave)
        same = bool(numpy.array_equal(want.view(numpy.uint64), got.view(numpy.uint64)))
        ms = {'chain': [], 'resident': []}
        for _ in range(args.alternations):
            for arm, fn in (('chain', chain), ('resident', resident)):
                t0 = time.perf_counter()
                fn(wave)
                ms[arm].append(1e3 * (time.perf_counter() - t0))
        cell = {'samples_in': int(wave.wave.size), 'samples_out': int(got.size), 'same_bits': same,
                'resident_calls': pipeline.calls['resident'] - before['resident'], 'composed_calls': pipeline.calls['composed'] - before['composed']}
        for arm, v in ms.items():
            cell[arm + '_ms'] = {'median': statistics.median(v), 'spread': max(v) - min(v), 'min': min(v), 'max': max(v), 'all': v}
        cell['ratio_resident_to_chain'] = cell['resident_ms']['median'] / cell['chain_ms']['median']
        res['configs'][name] = cell
    res['resident_faster_in_both'] = all(c['resident_ms']['median'] < c['chain_ms']['median'] for c in res['configs'].values())
    text = json.dumps(res, indent=1)
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text + '\n')
    pipe.close()
    chain_synth.close()
    if not all(c['same_bits'] and c['composed_calls'] == 0 for c in res['configs'].values()):
        sys.exit('the two arms differ, or the pipeline took the composed path')


if __name__ == '__main__':
    main()
