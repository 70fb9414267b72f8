"""The fused CREPE-mode encode on the MI355X against the chain it replaces, bit for bit: the voicing kernel against `crepe.predict_voicing` and the
reference wrapper's mask, `CrepeModel.track` against predict -> predict_voicing -> mask, `Analyzer.run_device` against `Analyzer.run`, and
`encode.extract` against `world_analysis.extract` through the drop-in `AcousticFeature`.  Cases: tests/encode_cases.py.  `tiny` capacity with
synthetic weights throughout.  The output of a run of this file is kept as profiles/r15/encode_pytest_gpu.txt."""
import numpy
import pytest

import encode_cases as E
from realtime_yukarin_amd import crepe, encode, world_analysis

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model(gpu_ctx):
    m = crepe.CrepeModel('tiny', seed=21, ctx=gpu_ctx)
    yield m
    m.close()


@pytest.mark.parametrize('n', E.LENGTHS)
def test_voicing_equals_predict_voicing_and_the_mask(model, n):
    E.check_voicing(model, n)


@pytest.mark.parametrize('n', [3, 257, E.VOICING_CHUNK + 1])
def test_voicing_on_poisoned_buffers_and_from_device_pointers(model, n):
    E.check_voicing(model, n, poison=True)
    E.check_voicing(model, n, device=True)


@pytest.mark.parametrize('sr', [16000, 24000])
def test_track_equals_the_chain_it_replaces(model, sr):
    """0.25 s (51 frames) and 0.6 s (121 frames), then 1.4 s (281 frames: a second pass through the network), then the first wave again on the
    same handle, on poisoned buffers and left on the card: the same bits every time."""
    x, hop, first = E.check_track(model, 0.25, sr)
    assert first[0].size == 51
    assert E.check_track(model, 0.6, sr)[2][0].size == 121
    long_ = E.check_track(model, 1.4, sr)[2]
    assert long_[0].size == 281
    again = model.track(x, sr, hop, 5)
    assert all(E.same(a, b) for a, b in zip(again, first))
    model.poison()
    trk = model.track(x, sr, hop, 5, device=True)
    assert (trk.frames, trk.samples) == (51, x.size)
    voiced, f64 = trk.download()
    assert numpy.array_equal(voiced, first[0]) and E.same(f64, first[1])


@pytest.mark.parametrize('fs', [16000, 24000])
def test_run_device_equals_run(gpu_ctx, fs):
    E.check_run_device(gpu_ctx, fs)


@pytest.fixture
def installed(gpu_ctx, tmp_path, monkeypatch):
    """The drop-in `AcousticFeature` with `encode.extract` installed, a local CREPE wrapper class, `tiny` weights behind the shim."""
    from realtime_yukarin_amd.compat import crepe as shim
    from realtime_yukarin_amd.compat.yukarin import AcousticFeature

    class Feature(AcousticFeature):                                 # a class of the test's own: the shared one keeps its `extract`
        pass

    class CrepeFeature(Feature):
        @classmethod
        def extract_f0(cls, x, fs, frame_period, f0_floor, f0_ceil):       # the reference wrapper's body, restated (capacity: the test's)
            t, f0, confidence, _ = shim.predict(x, fs, viterbi=True, model_capacity='tiny', step_size=frame_period, verbose=0)
            voiced = (shim.predict_voicing(confidence) == 1) | (confidence > 0.1)
            f0[~voiced] = 0
            return f0, t

    class OtherFeature(Feature):                                    # the same f0, but nobody named the class
        extract_f0 = CrepeFeature.__dict__['extract_f0']

    path = tmp_path / 'crepe_tiny.npz'
    crepe.save_weights(path, crepe.synthetic_params('tiny', 21))
    monkeypatch.setattr(shim, '_weights', {})
    monkeypatch.setattr(shim, '_models', {})
    monkeypatch.delenv('RY_CREPE_RESAMPLE', raising=False)
    monkeypatch.delenv('RY_CREPE_DTYPE', raising=False)
    shim.load_model(path, 'tiny')
    monkeypatch.setattr(world_analysis, 'aperiodicity', world_analysis.device_aperiodicity)
    monkeypatch.setattr(encode, 'crepe_classes', set())
    monkeypatch.setattr(encode, 'model_capacity', 'tiny')
    monkeypatch.setattr(encode, 'calls', {'fused': 0, 'unfused': 0})
    encode.install(Feature, CrepeFeature)
    yield CrepeFeature, OtherFeature
    for m in shim._models.values():
        m.close()


ARGS = dict(frame_period=5, f0_floor=71.0, f0_ceil=800.0, fft_length=1024, order=8, alpha=0.466)


def equal_features(a, b):
    for k in ('f0', 'sp', 'ap', 'coded_ap', 'mc', 'voiced'):
        assert E.same(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize('dtype', [numpy.float32, numpy.float64])
def test_extract_fused_equals_world_analysis_extract(installed, dtype):
    from realtime_yukarin_amd.compat.yukarin import Wave
    CrepeFeature, _ = installed
    wave = Wave(E.mixed_wave(0.5, 24000, seed=3), 24000)
    got = CrepeFeature.extract(wave, dtype=dtype, **ARGS)
    assert encode.calls == {'fused': 1, 'unfused': 0}
    want = world_analysis.extract(CrepeFeature, wave, dtype=dtype, **ARGS)
    assert got.f0.shape == (101, 1) and got.voiced.dtype == numpy.bool_
    assert got.sp.dtype == dtype and type(got) is type(want)
    equal_features(got, want)


def test_extract_falls_back_unchanged(installed):
    """A float64 wave that does not round-trip through float32, and a class nobody named: `world_analysis.extract`, its bits."""
    from realtime_yukarin_amd.compat.yukarin import Wave
    CrepeFeature, OtherFeature = installed
    x = E.mixed_wave(0.25, 24000, seed=4).astype(numpy.float64)
    x[100] += 2.0 ** -40
    assert not numpy.array_equal(x.astype(numpy.float32).astype(numpy.float64), x)
    for cls, wave in ((CrepeFeature, Wave(x, 24000)), (OtherFeature, Wave(x.astype(numpy.float32), 24000))):
        before = dict(encode.calls)
        got = cls.extract(wave, dtype=numpy.float32, **ARGS)
        assert encode.calls == {'fused': before['fused'], 'unfused': before['unfused'] + 1}
        equal_features(got, world_analysis.extract(cls, wave, dtype=numpy.float32, **ARGS))
