"""The resident wave-to-wave chain on the MI355X against the chain of the separate calls, bit for bit: `Pipeline.convert_wave` / `push` / `flush`
against `encode.extract` -> `VoiceChanger.convert_from_acoustic_feature` -> `world_synth.decode` (or a `Synthesizer.push` sequence) in the same
process, and the entry points under it (`ry_analysis_extract_resident`, `ry_mask_rows`).  `tiny` CREPE capacity, SYN-8 predictors, 0.25 s waves
(51 frames) and a wave of a single hop.  Cases: tests/pipeline_cases.py."""
import numpy
import pytest

import pipeline_cases as P
from realtime_yukarin_amd import pipeline, world_synth

pytestmark = pytest.mark.gpu
SEED = 3


@pytest.fixture(scope='module')
def changers(gpu_ctx, tmp_path_factory):
    """One voice changer per rate for the module: the predictors and their launch plans are built once."""
    out = {fs: P.voice_changer(P.write_models(tmp_path_factory.mktemp('models%d' % fs), fs), fs) for fs in P.RATES}
    yield out
    for vc in out.values():
        P.close_voice_changer(vc)


@pytest.fixture(scope='module')
def reference(changers):
    """(rate, kind, CREPE dtype) -> the samples of the chain of the separate calls, computed once and left unchanged."""
    return {}


def run_chain(reference, shim_dtype, vc, fs, kind, wave, cls):
    key = (fs, kind, shim_dtype)
    if key not in reference:
        synth = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=SEED)
        reference[key] = P.chain(vc, vc.acoustic_converter.config.dataset.acoustic_param, cls, wave, synth)
        synth.close()
        reference[key].setflags(write=False)
    return reference[key]


@pytest.fixture(params=['f32', 'bf16x3'])
def process(request, gpu_ctx, monkeypatch, tmp_path):
    shim = P.set_up(monkeypatch, tmp_path, 'tiny', request.param)
    yield request.param
    P.close_shim(shim)


def pipe_of(vc):
    return pipeline.Pipeline(vc, vc.acoustic_converter.config.dataset.acoustic_param, crepe_capacity='tiny', seed=SEED)


@pytest.mark.parametrize('fs', P.RATES)
@pytest.mark.parametrize('kind', P.KINDS)
def test_convert_wave_equals_the_chain(process, changers, reference, kind, fs):
    from yukarin import Wave
    x = P.wave_of(kind, fs)
    P.check_split(kind, x, fs, 51)
    vc = changers[fs]
    pipe = pipe_of(vc)
    want = run_chain(reference, process, vc, fs, kind, Wave(x, fs), pipe.feature_class)
    got = pipe.convert_wave(Wave(x, fs))
    assert pipeline.calls == {'resident': 1, 'composed': 0}
    assert got.sampling_rate == fs and got.wave.size == int(50 * P.FRAME_PERIOD / 1000 * fs) + 1
    assert P.same(got.wave, want)
    assert P.same(pipe.convert_wave(Wave(x, fs)).wave, want) and pipeline.calls['resident'] == 2          # the blocks are reused
    pipe.close()


@pytest.mark.parametrize('fs', P.RATES)
def test_a_wave_of_a_single_hop(process, changers, reference, fs):
    from yukarin import Wave
    x = P.wave_of('loud', fs, P.FRAME_PERIOD / 1000)
    assert x.size == fs * P.FRAME_PERIOD // 1000
    vc = changers[fs]
    pipe = pipe_of(vc)
    want = run_chain(reference, process, vc, fs, 'hop', Wave(x, fs), pipe.feature_class)
    assert P.same(pipe.convert_wave(Wave(x, fs)).wave, want) and pipeline.calls == {'resident': 1, 'composed': 0}
    pipe.close()


@pytest.mark.parametrize('fs', P.RATES)
def test_convert_wave_on_poisoned_buffers(process, changers, reference, gpu_ctx, monkeypatch, tmp_path, fs):
    """After `ry_crepe_debug_poison`, `ry_analysis_debug_poison` and `ry_synth_debug_poison`, then under RY_POISON=1 on predictors made for it
    (fresh activation buffers hold NaN patterns): what a call reads it has written."""
    from yukarin import Wave
    from realtime_yukarin_amd import world_analysis
    from realtime_yukarin_amd.compat import crepe as shim
    vc = changers[fs]
    pipe = pipe_of(vc)
    param = pipe.acoustic_param
    for kind in ('gap', 'gap_silent_ends'):
        x = P.wave_of(kind, fs)
        want = run_chain(reference, process, vc, fs, kind, Wave(x, fs), pipe.feature_class)
        pipe.convert_wave(Wave(x, fs))                                 # the handles and the blocks exist
        shim._model('tiny').poison()
        world_analysis._analyzer(fs, 1024, param.order, float(param.alpha)).poison()
        pipe.synth.poison()
        assert P.same(pipe.convert_wave(Wave(x, fs)).wave, want)
    pipe.close()
    monkeypatch.setenv('RY_POISON', '1')
    gpu_ctx.reload_env()
    try:
        fresh = P.voice_changer(P.write_models(tmp_path, fs), fs)
        pipe = pipe_of(fresh)
        x = P.wave_of('gap', fs)
        assert P.same(pipe.convert_wave(Wave(x, fs)).wave, run_chain(reference, process, vc, fs, 'gap', Wave(x, fs), pipe.feature_class))
        pipe.close()
        P.close_voice_changer(fresh)
    finally:
        monkeypatch.delenv('RY_POISON')
        gpu_ctx.reload_env()
    assert pipeline.calls['composed'] == 0


@pytest.mark.parametrize('fs', P.RATES)
def test_push_and_flush_equal_the_chain_with_the_same_picks(process, changers, fs):
    """Three buffers with discard = (10, 10), then the flush: every return value equals the chain's (`convert_from_acoustic_feature` with the same
    hint, the pick of rows [10, frames - 10), `Synthesizer.push`).  The synthesis noise is a function of the seed and the sample position."""
    from yukarin import Wave
    vc = changers[fs]
    pipe = pipe_of(vc)
    param = pipe.acoustic_param
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=SEED)
    waves = [Wave(P.wave_of(kind, fs, seed=s), fs) for s, kind in enumerate(('loud', 'gap', 'gap_silent_ends'))]
    want = [P.chain_push(vc, param, pipe.feature_class, w, ref, (10, 10)) for w in waves] + [ref.flush()]
    got = [pipe.push(w, discard=(10, 10)).wave for w in waves] + [pipe.flush().wave]
    assert pipeline.calls == {'resident': 3, 'composed': 0}
    for g, w in zip(got, want):
        assert P.same(g, w)
    assert sum(len(w) for w in want) == int((3 * 31 - 1) * P.FRAME_PERIOD / 1000 * fs) + 1
    vc._fused_core().set_discard(0, 0)
    pipe.close()
    ref.close()


@pytest.mark.parametrize('fs', P.RATES)
def test_extract_resident_equals_run_device_cast_to_float32(gpu_ctx, fs):
    P.check_extract_resident(gpu_ctx, fs)


def test_mask_rows_equals_numpy(gpu_ctx):
    P.check_mask_rows(gpu_ctx)
