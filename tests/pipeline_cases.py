"""Cases the emulator and the GPU tests of the resident wave-to-wave chain share (test_pipeline_cpu.py, test_pipeline_gpu.py): the waves, the model
files (SYN-8 predictors, order 8, input rate = output rate), the set-up of the process (CREPE weights behind the shim, D4C from the device, the
feature classes) and the chain of the separate calls every result is compared with, bit for bit: `encode.extract` ->
`VoiceChanger.convert_from_acoustic_feature` -> `world_synth.decode` (or a `Synthesizer.push` sequence)."""
import json
import types

import numpy

from realtime_yukarin_amd import compat, crepe, encode, pipeline, world_analysis, world_synth
from realtime_yukarin_amd.netspec import NetDesc
from realtime_yukarin_amd.weights import save_npz, synthetic_params

compat.install()
RATES = (24000, 16000)
KINDS = ('loud', 'gap', 'zeros', 'gap_silent_ends')
FRAME_PERIOD, ORDER, THRESHOLD = 5, 8, 60
BINS = 513


def bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view({8: numpy.uint64, 4: numpy.uint32, 1: numpy.uint8}[a.dtype.itemsize])


def same(a, b) -> bool:
    a, b = numpy.asarray(a), numpy.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(numpy.array_equal(bits(a), bits(b)))


def wave_of(kind: str, fs: int, seconds: float = 0.25, seed: int = 0) -> numpy.ndarray:
    """float32.  'loud': a 220 Hz tone burst with a little noise throughout; 'gap': a loud head, an exactly zero middle and a loud tail; 'zeros';
    'gap_silent_ends': 'gap' with 640 zero samples at either end (more than half a gate window: the first and the last frame are silent)."""
    n = int(round(seconds * fs))
    rng = numpy.random.default_rng([seed, n, fs])
    x = 0.4 * numpy.sin(2 * numpy.pi * 220.0 * numpy.arange(n) / fs) + 0.05 * rng.normal(0, 1, n)
    if kind == 'zeros':
        x[:] = 0
    elif kind == 'gap':
        x[n // 4:3 * n // 4] = 0
    elif kind == 'gap_silent_ends':
        x[n // 2 - 700:n // 2 + 700] = 0
        x[:640] = 0
        x[n - 640:] = 0
    else:
        assert kind == 'loud', kind
    return x.astype(numpy.float32)


def host_mask(x, fs, n_frames=None):
    """The host gate (compat/yukarin/wave.py) at the tests' threshold, cut or padded to n_frames as `separate_effective` does."""
    from yukarin import Wave
    eff = Wave(x, fs).get_effective_frame(threshold_db=THRESHOLD, fft_length=1024, frame_period=FRAME_PERIOD)
    if n_frames is not None:
        eff = numpy.concatenate([eff, numpy.zeros(max(n_frames - len(eff), 0), bool)])[:n_frames]
    return eff


def check_split(kind, x, fs, n_frames=None):
    """The case is worth its name: a wave that should split into effective and silent frames does, before anything is compared."""
    eff = host_mask(x, fs, n_frames)
    n_eff, n = int(eff.sum()), len(eff)
    if kind == 'loud':
        assert n_eff == n, (kind, n_eff, n)
    elif kind == 'zeros':
        assert n_eff == 0, (kind, n_eff, n)
    else:
        assert 0 < n_eff < n, (kind, n_eff, n)
    if kind == 'gap_silent_ends':
        assert not eff[0] and not eff[-1], eff
    return eff


def write_models(d, fs):
    """SYN-8 predictors with synthetic weights, their configs (input and output rate fs) and the f0 statistics."""
    d1, d2 = NetDesc(1, ORDER + 1, ORDER + 1, 8, 8), NetDesc(2, 1, 1, 8, 8)
    save_npz(d / 's1.npz', synthetic_params(d1, 11, bias_std=0.05))
    save_npz(d / 's2.npz', synthetic_params(d2, 12, bias_std=0.02))
    (d / 's1.json').write_text(json.dumps({
        'dataset': {'acoustic_param': {'sampling_rate': fs, 'frame_period': FRAME_PERIOD, 'order': ORDER, 'alpha': 0.466 if fs == 24000 else 0.41},
                    'in_features': ['mc'], 'out_features': ['mc']},
        'model': {'in_channels': ORDER + 1, 'out_channels': ORDER + 1, 'generator_base_channels': 8, 'generator_extensive_layers': 8}}))
    (d / 's2.json').write_text(json.dumps({
        'dataset': {'param': {'voice_param': {'sample_rate': fs}, 'acoustic_feature_param': {'frame_period': FRAME_PERIOD, 'order': ORDER}}},
        'model': {'generator_base_channels': 8, 'generator_extensive_layers': 8}}))
    numpy.save(str(d / 'in_stat.npy'), {'mean': numpy.log(200.0), 'var': 0.04})
    numpy.save(str(d / 'tg_stat.npy'), {'mean': numpy.log(300.0), 'var': 0.09})
    return d


def voice_changer(d, fs):
    from become_yukarin import SuperResolution
    from become_yukarin.config.sr_config import create_from_json as create_sr_config
    from yukarin import AcousticConverter
    from yukarin.config import create_from_json as create_config
    from yukarin.f0_converter import F0Converter
    from realtime_yukarin_amd.voice_changer import VoiceChanger
    f0c = F0Converter(input_statistics=d / 'in_stat.npy', target_statistics=d / 'tg_stat.npy')
    ac = AcousticConverter(create_config(d / 's1.json'), d / 's1.npz', f0_converter=f0c, out_sampling_rate=fs)
    sr = SuperResolution(create_sr_config(d / 's2.json'), d / 's2.npz')
    return VoiceChanger(acoustic_converter=ac, super_resolution=sr, threshold=THRESHOLD)


def close_voice_changer(vc):
    vc.close()
    vc.acoustic_converter.close()
    vc.super_resolution.close()


def set_up(monkeypatch, tmp_path, capacity, crepe_dtype=None):
    """CREPE weights of `capacity` behind the shim (its models are this test's), D4C from the device, the pipeline's class named for `encode`."""
    from realtime_yukarin_amd.compat import crepe as shim
    path = tmp_path / 'crepe.npz'
    crepe.save_weights(path, crepe.synthetic_params(capacity, 21))
    monkeypatch.setattr(shim, '_weights', {})
    monkeypatch.setattr(shim, '_models', {})
    monkeypatch.delenv('RY_CREPE_RESAMPLE', raising=False)
    monkeypatch.delenv('RY_DEVICE_GATE', raising=False)
    monkeypatch.delenv('RY_DISCARD_HINT', raising=False)
    if crepe_dtype is None:
        monkeypatch.delenv('RY_CREPE_DTYPE', raising=False)
    else:
        monkeypatch.setenv('RY_CREPE_DTYPE', crepe_dtype)
    shim.load_model(path, capacity)
    monkeypatch.setattr(world_analysis, 'aperiodicity', world_analysis.device_aperiodicity)
    monkeypatch.setattr(encode, 'crepe_classes', {pipeline.crepe_feature_class()})
    monkeypatch.setattr(encode, 'model_capacity', capacity)
    monkeypatch.setattr(pipeline, 'calls', {'resident': 0, 'composed': 0})
    return shim


def close_shim(shim):
    for m in shim._models.values():
        m.close()


def encode_args(param):
    return dict(frame_period=param.frame_period, f0_floor=param.f0_floor, f0_ceil=param.f0_ceil, fft_length=param.fft_length, order=param.order,
                alpha=param.alpha, dtype=param.dtype)


def chain_feature(vc, param, cls, wave, discard=(0, 0)):
    f = encode.extract(cls, wave, **encode_args(param))
    f.wave = wave
    return vc.convert_from_acoustic_feature(f, discard)


def chain(vc, param, cls, wave, synth):
    """The chain of the separate calls -> float64 samples (`world_synth.decode` over `synth`)."""
    vocoder = types.SimpleNamespace(out_sampling_rate=vc.output_sampling_rate, acoustic_param=param, _ry_synth=synth)
    return world_synth.decode(vocoder, chain_feature(vc, param, cls, wave)).wave


def chain_push(vc, param, cls, wave, synth, discard):
    """One buffer of the live chain: encode, convert with the discard hint, pick [front, frames - back), push."""
    out = chain_feature(vc, param, cls, wave, discard)
    k0, k1 = discard[0], len(out.f0) - discard[1]
    return synth.push(numpy.asarray(out.f0).ravel()[k0:k1], out.sp[k0:k1], out.ap[k0:k1])


def mask_rows_reference(rows, mask, k0, k1):
    want = rows.copy()
    sel = numpy.zeros(len(mask), bool)
    sel[k0:k1] = ~mask[k0:k1].astype(bool)
    want[sel] = 0.0
    return want


def mask_rows_cases():
    """(n, cols, mask bytes, k0, k1): one row and several workgroups of rows; cols 513 (every alignment of a row start), 4, 1, 6; all-0, all-1 and
    alternating masks; an empty range; ranges that leave silent rows out."""
    out = []
    for cols in (513, 4, 1, 6):
        out.append((1, cols, numpy.zeros(1, numpy.uint8), 0, 1))
        out.append((1, cols, numpy.ones(1, numpy.uint8), 0, 1))
        for n in (9, 22):
            alt = (numpy.arange(n) % 2).astype(numpy.uint8)
            for mask in (numpy.zeros(n, numpy.uint8), numpy.ones(n, numpy.uint8), alt, 1 - alt):
                out.append((n, cols, mask, 0, n))
            out.append((n, cols, numpy.zeros(n, numpy.uint8), 3, 3))          # k0 = k1: nothing
            out.append((n, cols, numpy.zeros(n, numpy.uint8), 2, n - 3))      # silent rows outside the range keep their bits
            out.append((n, cols, alt, 1, n - 1))
    return out


def check_mask_rows(ctx):
    rng = numpy.random.default_rng(5)
    for n, cols, mask, k0, k1 in mask_rows_cases():
        rows = rng.normal(size=(n + 2, cols)).astype(numpy.float32)           # a guard row behind and in front
        rows[rng.uniform(size=rows.shape) < 0.1] = numpy.nan
        block, m = ctx.dev_alloc(rows.size), ctx.dev_alloc(n // 4 + 2)
        words = numpy.zeros(n // 4 + 2, numpy.float32)
        words.view(numpy.uint8)[:n] = mask
        ctx.dev_upload(block, rows)
        ctx.dev_upload(m, words)
        ctx.mask_rows(block + 4 * cols, m, n, cols, k0, k1)
        got = numpy.empty_like(rows)
        ctx.dev_download(block, got)
        want = rows.copy()
        want[1:n + 1] = mask_rows_reference(rows[1:n + 1], mask, k0, k1)
        assert same(got, want), (n, cols, mask.tolist(), k0, k1)
        ctx.dev_free(block)
        ctx.dev_free(m)


def check_extract_resident(ctx, fs):
    """`Analyzer.extract_resident` against `Analyzer.run_device` rows cast with astype(float32); a track with one f0 >= fs / 2 is refused and leaves
    poisoned blocks untouched."""
    import encode_cases as E
    x, f0, t = E.analysis_case(fs)
    n = f0.size
    a = world_analysis.Analyzer(fs, order=ORDER, seed=5, ctx=ctx)
    dev = E.DeviceArrays(ctx, x, f0, t)
    sp, mc, ap = a.run_device(dev.address[0], x.size, dev.address[1], dev.address[2], n, want=('sp64', 'mc', 'ap64'))
    shapes = ((n, ORDER + 1), (n, BINS), (n, BINS))
    poison = [numpy.full(s, numpy.nan, numpy.float32) for s in shapes]
    out = E.DeviceArrays(ctx, *poison)
    a.poison()
    a.extract_resident(dev.address[0], x.size, dev.address[1], dev.address[2], n, *out.address)
    for want, address, shape in zip((mc, sp, ap), out.address, shapes):
        got = numpy.empty(shape, numpy.float32)
        ctx.dev_download(address, got)
        assert same(got, want.astype(numpy.float32))
    f0b = f0.copy()
    f0b[17] = fs / 2
    devb = E.DeviceArrays(ctx, f0b)
    refused = E.DeviceArrays(ctx, *poison)
    lib, h = a._get()
    from realtime_yukarin_amd import _lib
    rc = lib.dll.ry_analysis_extract_resident(h, _lib._fptr(dev.address[0]), x.size, E._DP(devb.address[0]), E._DP(dev.address[2]), n, 0.85,
                                              *[_lib._fptr(p) for p in refused.address])
    assert rc == -1 and b'f0[17]' in lib.dll.ry_last_error(), (rc, lib.dll.ry_last_error())
    for address, shape in zip(refused.address, shapes):
        got = numpy.zeros(shape, numpy.float32)
        ctx.dev_download(address, got)
        assert numpy.isnan(got).all()
    # the other refusals: a null output, null inputs, a negative count
    null = _lib._fptr(None)
    args = (h, _lib._fptr(dev.address[0]), x.size, E._DP(dev.address[1]), E._DP(dev.address[2]), n, 0.85)
    outs = [_lib._fptr(p) for p in refused.address]
    for i in range(3):
        assert lib.dll.ry_analysis_extract_resident(*args, *[null if j == i else o for j, o in enumerate(outs)]) == -1
    assert lib.dll.ry_analysis_extract_resident(h, null, x.size, *args[3:], *outs) == -1
    assert lib.dll.ry_analysis_extract_resident(*args[:5], -1, 0.85, *outs) == -1
    assert lib.dll.ry_analysis_extract_resident(None, *args[1:], *outs) == -4
    assert lib.dll.ry_analysis_extract_resident(*args[:5], 0, 0.85, *outs) == 0           # no frames: nothing to do, nothing written
    for address, shape in zip(refused.address, shapes):
        got = numpy.zeros(shape, numpy.float32)
        ctx.dev_download(address, got)
        assert numpy.isnan(got).all()
    for d in (dev, out, devb, refused):
        d.close()
    a.close()
