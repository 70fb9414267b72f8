"""CREPE on the MI355X against the torch float64 / numpy restatement (tests/crepe_ref.py), with seeded synthetic weights."""
import numpy
import pytest

import crepe_ref
from realtime_yukarin_amd import crepe

pytestmark = pytest.mark.gpu
HOP = 80


def rel(a, b):
    a, b = numpy.asarray(a, numpy.float64), numpy.asarray(b, numpy.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(numpy.abs(a - b).max() / max(numpy.abs(b).max(), 1e-30))


@pytest.fixture(scope='module')
def full(gpu_ctx):
    P = crepe.synthetic_params('full', 1)
    return crepe.CrepeModel('full', P, ctx=gpu_ctx), P


def speech_like(n, seed, sr=16000):
    """A gliding harmonic tone in noise, silence at the start."""
    rng = numpy.random.default_rng(seed)
    t = numpy.arange(n) / sr
    f = 150 + 60 * numpy.sin(2 * numpy.pi * 1.3 * t)
    x = sum(numpy.sin(2 * numpy.pi * numpy.cumsum(f * k) / sr) / k for k in (1, 2, 3)) + rng.normal(0, 0.05, n)
    x[:n // 10] = 0
    return (0.3 * x).astype(numpy.float32)


def test_full_capacity_layers_match_torch(full):
    model, P = full
    audio = speech_like(1024 + 23 * HOP, 0)
    f0, conf, act = model.predict16k(audio, HOP, center=False)
    assert act.shape == (24, 360)
    fr = crepe_ref.frames(audio, HOP, center=False)
    outs, logits, act_ref = crepe_ref.network(P, fr)
    assert rel(model.debug_layer(0, 24), fr) < 1e-5
    for i in range(6):
        assert rel(model.debug_layer(i + 1, 24), outs[i]) < 1e-4, 'conv%d' % (i + 1)
    assert rel(model.debug_layer(7, 24), logits) < 1e-4
    assert numpy.abs(act - act_ref).max() < 1e-4


def test_frames_are_independent_201(full):
    """201 frames in one call equal the same frames from three separate calls on sub-windows of the signal (center = False, windows
    cut at hop boundaries); f0 / confidence equal the numpy decode of the device's own activation, path included."""
    model, _ = full
    audio = speech_like(1024 + 200 * HOP, 1)
    f0, conf, act = model.predict16k(audio, HOP, center=False)
    assert act.shape == (201, 360)
    parts = []
    for a, b in ((0, 50), (50, 151), (151, 201)):
        parts.append(model.predict16k(audio[a * HOP:(b - 1) * HOP + 1024], HOP, center=False)[2])
    assert numpy.array_equal(numpy.concatenate(parts), act)         # exact: fixed split counts, one K order per row (test_crepe_oracle.py)
    f0_ref, conf_ref, path_ref = crepe_ref.decode(act, viterbi=True)
    assert numpy.array_equal(conf, conf_ref)
    assert numpy.allclose(f0, f0_ref, rtol=1e-6, atol=0)
    f0_d, _, path = model.decode(act, viterbi=True)
    assert numpy.array_equal(path, path_ref)
    assert numpy.array_equal(f0_d, f0)


@pytest.mark.parametrize('capacity', ['tiny', 'small', 'medium', 'large'])
def test_every_capacity(gpu_ctx, capacity):
    P = crepe.synthetic_params(capacity, 2)
    model = crepe.CrepeModel(capacity, P, ctx=gpu_ctx)
    audio = speech_like(1024 + 11 * HOP, 3)
    f0, conf, act = model.predict16k(audio, HOP, center=False)
    _, logits, act_ref = crepe_ref.network(P, crepe_ref.frames(audio, HOP, center=False))
    assert rel(model.debug_layer(7, 12), logits) < 1e-4
    assert numpy.abs(act - act_ref).max() < 1e-4
    f0_ref, _, _ = crepe_ref.decode(act)
    assert numpy.allclose(f0, f0_ref, rtol=1e-6, atol=0)
    model.close()


@pytest.mark.parametrize('n', [1, 79, 500, 1024, 16000, 32000])
def test_lengths(full, n):
    """1 sample .. 2 s (401 frames: two passes of the network).  The first frames of the 2-s call, whose windows lie inside the first
    second, equal those of the 1-s call."""
    model, _ = full
    audio = speech_like(32000, 4)[:n]
    f0, conf, act = model.predict16k(audio, HOP)
    assert len(f0) == 1 + n // HOP == len(conf) == len(act)
    assert numpy.isfinite(act).all() and numpy.isfinite(f0).all() and (f0 >= 0).all()
    if n == 32000:
        a1 = model.predict16k(audio[:16000], HOP)[2]
        k = (16000 - 512) // HOP
        assert numpy.array_equal(act[:k], a1[:k])


def test_24khz_and_silence_through_the_shim(full, tmp_path, monkeypatch):
    """24 kHz input (resampled on the host, float64) and a digitally silent stretch: no NaN anywhere; the shim equals the model on the
    resampled signal."""
    from realtime_yukarin_amd.compat import crepe as shim
    model, P = full
    path = tmp_path / 'crepe_full.npz'
    crepe.save_weights(path, P)
    monkeypatch.setenv('RY_CREPE_MODEL', str(path))
    monkeypatch.setattr(shim, '_weights', {})
    monkeypatch.setattr(shim, '_models', {})
    x = speech_like(24000, 5, sr=24000)
    x[6000:14000] = 0                                              # a third of a second of digital silence
    t, f0, conf, act = shim.predict(x, 24000, viterbi=True, step_size=5, verbose=0)
    assert numpy.isfinite(act).all() and numpy.isfinite(f0).all() and numpy.isfinite(conf).all()
    f0_m, conf_m, act_m = model.predict16k(crepe.resample(x, 24000), HOP)
    assert numpy.array_equal(act, act_m) and numpy.array_equal(conf, conf_m) and numpy.array_equal(f0, f0_m.astype(numpy.float64))
    shim._models[32].close()


def test_reference_extract_f0_through_the_shim(full, tmp_path, monkeypatch):
    """The body of the reference's CrepeAcousticFeatureWrapper.extract_f0 (yukarin_wrapper/acoustic_feature_wrapper.py:65-80), restated,
    with `import crepe` resolving to the drop-in module."""
    import importlib
    import sys
    from realtime_yukarin_amd import compat
    _, P = full
    path = tmp_path / 'crepe_full.npz'
    crepe.save_weights(path, P)
    monkeypatch.setenv('RY_CREPE_MODEL', str(path))
    monkeypatch.syspath_prepend(str(compat.COMPAT_DIR))
    sys.modules.pop('crepe', None)
    shim = importlib.import_module('crepe')
    assert shim.__file__ == str(compat.COMPAT_DIR / 'crepe' / '__init__.py')

    def extract_f0(x, fs, frame_period, f0_floor, f0_ceil):
        import crepe as c
        t, f0, confidence, _ = c.predict(x, fs, viterbi=True, model_capacity='full', step_size=frame_period, verbose=0)
        voiced = (c.predict_voicing(confidence) == 1) | (confidence > 0.1)
        f0[~voiced] = 0
        return f0, t

    x = speech_like(24000, 6, sr=24000).astype(numpy.float64)
    f0, t = extract_f0(x, 24000, 5, 71.0, 800.0)
    n = 1 + 16000 // 80
    assert f0.shape == (n,) and t.shape == (n,) and f0.dtype == numpy.float64
    assert numpy.allclose(t, numpy.arange(n) * 0.005)
    _, f0_all, conf, _ = shim.predict(x, 24000, viterbi=True, model_capacity='full', step_size=5, verbose=0)
    voiced = (shim.predict_voicing(conf) == 1) | (conf > 0.1)
    assert numpy.array_equal(f0[voiced], f0_all[voiced]) and (f0[~voiced] == 0).all()
    shim._models[32].close()
    sys.modules.pop('crepe', None)
