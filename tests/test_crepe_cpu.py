"""CREPE without a GPU: the kernels on the host-side SIMT emulator at reduced filter multipliers (m = 1, 2) and a few frames against the
torch float64 / numpy restatement in tests/crepe_ref.py, the decode on constructed activations, the resampler, the weights loader, the C
ABI's parameter count and refusals, and the drop-in `crepe` module."""
import ctypes
import inspect
import os
import subprocess
import sys
from pathlib import Path

import numpy
import pytest

import crepe_ref
from crepe_cases import tie_activations
from realtime_yukarin_amd import _lib, build, crepe

ROOT = Path(__file__).resolve().parent.parent
HOP = 80


def rel(a, b):
    a, b = numpy.asarray(a, numpy.float64), numpy.asarray(b, numpy.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(numpy.abs(a - b).max() / max(numpy.abs(b).max(), 1e-30))


@pytest.fixture(scope='module')
def models(emu_ctx):
    out = {}
    for m in (1, 2):
        P = crepe.synthetic_params(m, 10 + m)
        out[m] = (crepe.CrepeModel(m, P, ctx=emu_ctx), P)
    return out


def check_network(model, P, audio, center):
    f0, conf, act = model.predict16k(audio, HOP, center=center)
    fr = crepe_ref.frames(audio, HOP, center)
    outs, logits, act_ref = crepe_ref.network(P, fr)
    n = len(fr)
    assert act.shape == (n, 360) and f0.shape == (n,) and conf.shape == (n,)
    assert rel(model.debug_layer(0, n), fr) < 1e-6
    for i in range(6):
        assert rel(model.debug_layer(i + 1, n), outs[i]) < 1e-5, 'conv%d' % (i + 1)
    assert rel(model.debug_layer(7, n), logits) < 1e-5
    assert numpy.abs(act - act_ref).max() < 1e-6
    return f0, conf, act


@pytest.mark.parametrize('m', [1, 2])
def test_layers_match_torch_float64(models, m):
    """Every conv layer (both 'same' edges: all output positions are compared; the stride-4 conv1), the dense layer and the sigmoid, with
    three frames (the dense layer's odd row count).  The synthetic weights have negative BN gammas."""
    model, P = models[m]
    assert (P['conv1_BN.weight'] < 0).any() and (P['conv2_BN.weight'] < 0).any()
    audio = numpy.random.default_rng(m).normal(0, 0.3, 1024 + 2 * HOP).astype(numpy.float32)
    check_network(model, P, audio, center=False)


def test_bn_before_pool_with_negative_gamma(emu_ctx):
    """All gammas negative: max-pooling before BN would give the minimum of each pair after BN instead of the maximum."""
    P = crepe.synthetic_params(1, 5)
    for i in range(1, 7):
        P['conv%d_BN.weight' % i] = -numpy.abs(P['conv%d_BN.weight' % i]) - 0.1
    model = crepe.CrepeModel(1, P, ctx=emu_ctx)
    audio = numpy.random.default_rng(7).normal(0, 1, 1024 + HOP).astype(numpy.float32)
    check_network(model, P, audio, center=False)
    model.close()


def test_framing_silence_and_short_signal(models):
    """A digitally silent frame normalises to zeros (the std clamp), not NaN; a centred signal shorter than one frame gives
    1 + n // hop frames; the frames equal the numpy restatement."""
    model, P = models[1]
    audio = numpy.random.default_rng(3).normal(0, 0.5, 1024 + 2 * HOP).astype(numpy.float32)
    audio[HOP:HOP + 1024] = 0.25                                   # frame 1 is constant: std 0
    f0, conf, act = check_network(model, P, audio, center=False)
    assert numpy.all(model.debug_layer(0, 3)[1] == 0)
    assert numpy.isfinite(act).all() and numpy.isfinite(f0).all() and numpy.isfinite(conf).all()
    short = numpy.random.default_rng(4).normal(0, 0.5, 300).astype(numpy.float32)
    f0, conf, act = check_network(model, P, short, center=True)
    assert len(f0) == 1 + 300 // HOP == crepe.n_frames(300, HOP, True)


def test_split_k_path_is_used(models):
    """conv2 at m = 1 runs split over K (slabs + the reduction kernel), conv1 in one piece (fused epilogue)."""
    s = models[1][0].splits()
    assert s[0] == 1 and s[1] > 1


# ---- decode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1])
def test_viterbi_path_bit_identical_with_ties(models, seed):
    model = models[1][0]
    a = tie_activations(41, seed)
    f0, conf, path = model.decode(a, viterbi=True)
    f0_ref, conf_ref, path_ref = crepe_ref.decode(a, viterbi=True)
    assert numpy.array_equal(path, path_ref)
    assert numpy.array_equal(conf, conf_ref)
    assert numpy.allclose(f0, f0_ref, rtol=1e-6, atol=0)


def test_decode_without_viterbi(models):
    model = models[1][0]
    a = numpy.random.default_rng(9).uniform(0, 1, (17, 360)).astype(numpy.float32)
    a[3] = 0                                                        # an all-zero row: 0 / 0 -> f0 = 0
    f0, conf, path = model.decode(a, viterbi=False)
    f0_ref, conf_ref, centers = crepe_ref.decode(a, viterbi=False)
    assert numpy.array_equal(path, centers)
    assert f0[3] == 0 and f0_ref[3] == 0
    assert numpy.allclose(f0, f0_ref, rtol=1e-6, atol=0)


@pytest.mark.parametrize('b', [0, 1, 100, 359])
def test_known_answer_bump(models, b):
    """A symmetric bump around bin b decodes to the bin's own cents: f0 = 10 * 2^(cents_b / 1200)."""
    a = numpy.zeros((3, 360), numpy.float32)
    a[:, b] = 0.9
    for d in (1, 2):
        for c in (b - d, b + d):
            if 0 <= c < 360 and 0 <= 2 * b - c < 360:
                a[:, c] = 0.9 / (2 + d)
    want = 10 * 2 ** (crepe.cents_mapping()[b] / 1200)
    for vit in (True, False):
        f0, conf, path = models[1][0].decode(a, viterbi=vit)
        assert numpy.all(path == b)
        assert numpy.allclose(f0, want, rtol=1e-6, atol=0)


# ---- resampler ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', [24000, 8000, 44100])
def test_resampler_matches_sinc_sum(sr):
    x = numpy.random.default_rng(sr).normal(0, 1, sr // 20)
    y = crepe.resample(x, sr, 16000)
    assert y.dtype == numpy.float32 and len(y) == int(len(x) * 16000 / sr)
    at = list(range(0, 40)) + list(range(len(y) // 2 - 20, len(y) // 2 + 20)) + list(range(len(y) - 40, len(y)))
    ref = crepe_ref.sinc_resample(x, sr, 16000, at=at)
    assert numpy.abs(y[at] - ref).max() < 1e-5 * numpy.abs(ref).max()


@pytest.mark.parametrize('sr', [24000, 48000])
def test_resampler_band_limited_tones(sr):
    t = numpy.arange(sr // 2) / sr
    freqs = (110.0, 440.0, 3000.0)
    x = sum(numpy.sin(2 * numpy.pi * f * t + i) for i, f in enumerate(freqs))
    y = crepe.resample(x, sr, 16000)
    t16 = numpy.arange(len(y)) / 16000
    want = sum(numpy.sin(2 * numpy.pi * f * t16 + i) for i, f in enumerate(freqs))
    mid = slice(400, len(y) - 400)                                  # away from the edges the filter's support reaches
    # resampy steps through the table by int(scale * 512) entries (341 for 24 kHz, 170 for 48 kHz): a pass-band gain off by
    # up to ~0.3 %, which the per-frame normalisation of CREPE removes
    assert numpy.abs(y[mid] - want[mid]).max() < 5e-3 * numpy.abs(want).max()


# ---- weights, ABI ---------------------------------------------------------------------------------------------------------------
def test_param_count_all_capacities():
    lib = _lib.Ry355Lib(build.build_product())
    for name, m in crepe.CAPACITIES.items():
        assert int(lib.dll.ry_crepe_param_count(m)) == crepe.param_count(m), name
    assert crepe.param_count(32) == 22244328 and crepe.param_count(4) == 487096
    for bad in (0, -1, 33):
        assert int(lib.dll.ry_crepe_param_count(bad)) == 0
        assert b'capacity' in lib.dll.ry_last_error()


def test_create_refuses_bad_sizes(emu_ctx):
    lib = emu_ctx.lib
    blob = numpy.zeros(crepe.param_count(1), numpy.float32)
    h = ctypes.c_void_p()
    assert lib.dll.ry_crepe_create(emu_ctx.handle, 1, _lib._fptr(blob), blob.size - 1, 1e-3, ctypes.byref(h)) == -1
    assert b'needs' in lib.dll.ry_last_error()
    assert lib.dll.ry_crepe_create(emu_ctx.handle, 40, _lib._fptr(blob), blob.size, 1e-3, ctypes.byref(h)) == -1
    assert not h.value


def test_predict_refuses_short_uncentred_audio(models, emu_ctx):
    model = models[1][0]
    lib, h = model._get()
    x = numpy.zeros(1000, numpy.float32)
    out = numpy.zeros(4, numpy.float32)
    assert lib.dll.ry_crepe_predict(h, _lib._fptr(x), x.size, HOP, 0, 1, _lib._fptr(out), _lib._fptr(out), None, 0) == -1
    assert b'1024' in lib.dll.ry_last_error()
    assert lib.dll.ry_crepe_predict(h, _lib._fptr(x), x.size, 0, 1, 1, _lib._fptr(out), _lib._fptr(out), None, 0) == -1
    with pytest.raises(ValueError):
        model.predict16k(x, HOP, center=False)


def test_loader_round_trip_and_refusals(tmp_path):
    import torch
    P = crepe.synthetic_params(1, 2)
    crepe.save_weights(tmp_path / 'w.npz', P)
    m, Q = crepe.load_weights(tmp_path / 'w.npz')
    assert m == 1 and all(numpy.array_equal(P[k], Q[k]) for k in P)
    # the fork's state dict: (Cout, Cin, W, 1) filters and BN counters
    sd = {k: torch.from_numpy(v[..., None] if k.startswith('conv') and k.endswith('.weight') and v.ndim == 3 else v) for k, v in P.items()}
    sd['conv1_BN.num_batches_tracked'] = torch.tensor(7)
    torch.save(sd, tmp_path / 'w.pt')
    m, Q = crepe.load_weights(tmp_path / 'w.pt', 1)
    assert all(numpy.array_equal(P[k], Q[k]) for k in P)
    assert numpy.array_equal(crepe.flatten_params(1, Q), crepe.flatten_params(1, P))
    bad = dict(P); del bad['conv3.bias']
    with pytest.raises(ValueError, match='missing'):
        crepe.validate_params(1, bad)
    bad = dict(P); bad['conv7.weight'] = P['conv6.weight']
    with pytest.raises(ValueError, match='unexpected'):
        crepe.validate_params(1, bad)
    bad = dict(P); bad['conv2.weight'] = P['conv2.weight'][:, :, :63]
    with pytest.raises(ValueError, match='shape'):
        crepe.validate_params(1, bad)
    with pytest.raises(ValueError, match='shape'):
        crepe.load_weights(tmp_path / 'w.npz', 'tiny')
    with pytest.raises(ValueError):
        crepe.multiplier('huge')


def test_predict_voicing_constants():
    conf = numpy.concatenate([numpy.full(50, 0.05), numpy.full(80, 0.8), numpy.full(50, 0.02)])
    v = crepe.predict_voicing(conf)
    assert v.shape == conf.shape and set(numpy.unique(v)) <= {0, 1}
    assert (v[:50] == 0).all() and (v[60:120] == 1).all() and (v[-40:] == 0).all()


# ---- drop-in module -------------------------------------------------------------------------------------------------------------
def test_shim_signatures_and_missing_weights(monkeypatch):
    from realtime_yukarin_amd.compat import crepe as shim
    p = inspect.signature(shim.predict).parameters
    assert list(p) == ['audio', 'sr', 'viterbi', 'model_capacity', 'center', 'step_size', 'verbose']
    assert (p['viterbi'].default, p['model_capacity'].default, p['center'].default, p['step_size'].default) == (False, 'full', True, 10)
    assert list(inspect.signature(shim.get_activation).parameters) == ['audio', 'sr', 'model_capacity', 'center', 'step_size', 'verbose']
    assert list(inspect.signature(shim.predict_voicing).parameters) == ['confidence']
    monkeypatch.delenv('RY_CREPE_MODEL', raising=False)
    monkeypatch.setattr(shim, '_weights', {})
    monkeypatch.setattr(shim, '_models', {})
    with pytest.raises(RuntimeError, match='RY_CREPE_MODEL'):
        shim.predict(numpy.zeros(1600, numpy.float32), 16000, viterbi=True, step_size=5)


def test_import_crepe_resolves_to_the_shim():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT / 'realtime_yukarin_amd' / 'compat'), str(ROOT)]))
    env.pop('RY_CREPE_MODEL', None)
    code = ('import crepe, realtime_yukarin_amd.compat.crepe as s; assert crepe.__file__ == s.__file__, crepe.__file__; '
            'print(crepe.predict.__module__)')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == 'crepe'
