"""WORLD mode on the MI355X: the track ingest of the analysis unit against its numpy statement, and `Pipeline(f0_mode='world')` /
`PipelineBank(f0_mode='world')` against the composed chain run with the same f0 callable -- `world_analysis.extract` (D4C from the device) ->
`VoiceChanger.convert_from_acoustic_feature` -> `world_synth.decode` / a `Synthesizer.push` sequence -- bit for bit, at 16 and 24 kHz.  SYN-8
predictors; no CREPE weights exist in the process.  Cases and bodies: tests/pipeline_world_cases.py."""
import numpy
import pytest

import pipeline_cases as P
import pipeline_world_cases as W
from realtime_yukarin_amd import pipeline, world_synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def changers(gpu_ctx, tmp_path_factory):
    """One voice changer per rate for the module: the predictors and their launch plans are built once."""
    out = {fs: P.voice_changer(P.write_models(tmp_path_factory.mktemp('world%d' % fs), fs), fs) for fs in P.RATES}
    yield out
    for vc in out.values():
        P.close_voice_changer(vc)


@pytest.fixture
def process(gpu_ctx, monkeypatch):
    shim = W.set_up(monkeypatch)
    yield gpu_ctx
    P.close_shim(shim)


# ---- 1. the ingest alone
@pytest.mark.parametrize('period', W.PERIODS)
def test_ingest_equals_the_numpy_statement(gpu_ctx, period):
    W.check_ingest_sizes(gpu_ctx, period)


def test_ingest_on_poisoned_buffers(gpu_ctx):
    W.check_ingest_poison(gpu_ctx)


def test_ingest_refusals_leave_the_previous_track(gpu_ctx):
    W.check_ingest_refusals(gpu_ctx)


@pytest.mark.parametrize('fs', P.RATES)
def test_the_extract_calls_take_the_ingested_track_in_place(gpu_ctx, fs):
    W.check_extract_takes_the_track_in_place(gpu_ctx, fs)


# ---- 2. the pipeline
def sizes_of(fs):
    """The shortest wave the chain accepts (one sample: one frame), 37 frames, and one sample either side of a hop multiple (37 -> 38 frames)."""
    hop = W.hop_of(fs)
    return (1, W.samples_for(37, fs), 37 * hop - 1, 37 * hop, 37 * hop + 1)


@pytest.mark.parametrize('fs', P.RATES)
def test_convert_wave_equals_the_chain(process, changers, fs):
    from yukarin import Wave
    vc = changers[fs]
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3)
    for i, n in enumerate(sizes_of(fs)):
        x = W.half_quiet_wave(n, fs, n) if i % 2 else W.voiced_wave(n, fs, n)
        W.check_convert_wave(vc, fs, x, W.f0_fn, W.chain(vc, W.param_of(vc), W.f0_fn, Wave(x, fs), ref))
    ref.close()


@pytest.mark.parametrize('fs', P.RATES)
def test_an_all_unvoiced_track(process, changers, fs):
    """D4C takes only the Love-Train path: every frame is off."""
    from yukarin import Wave
    vc = changers[fs]
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3)
    x = W.voiced_wave(W.samples_for(37, fs), fs, 5)
    W.check_convert_wave(vc, fs, x, W.unvoiced_fn, W.chain(vc, W.param_of(vc), W.unvoiced_fn, Wave(x, fs), ref))
    ref.close()


@pytest.mark.parametrize('fs', P.RATES)
def test_push_and_flush_on_300_frame_windows(process, changers, fs):
    W.check_push_flush(changers[fs], fs, None, 300, (100, 100))


@pytest.mark.parametrize('fs', P.RATES)
def test_refused_tracks_keep_the_blocks_good(process, changers, fs):
    W.check_refused_tracks(changers[fs], fs, None, 37)


@pytest.mark.parametrize('fs', P.RATES)
def test_a_track_that_does_not_fit_takes_the_composed_path(process, changers, fs):
    W.check_misfit_takes_the_composed_path(changers[fs], fs, None, 37)


def test_the_other_fallbacks_still_apply(process, changers, monkeypatch):
    W.check_other_fallbacks(changers[24000], 24000, None, monkeypatch, 37)


# ---- 3. the bank, 4. the gate in front
@pytest.mark.parametrize('fs', P.RATES)
def test_bank_streams_equal_their_lone_pipelines(process, changers, fs):
    W.check_bank(changers[fs], fs, (37, 21, 30), (3, 3))


def test_bank_out_gate_with_a_silent_stream(process, changers):
    W.check_bank_out_gate(changers[24000], 24000, None, (40, 40, 40), (3, 3), 1025, rounds=2)


@pytest.mark.parametrize('fs', P.RATES)
def test_gate_first_skips_the_host_f0_call(process, changers, fs):
    W.check_gate_first(changers[fs], fs, (37, 21, 30), (3, 3))


def test_bank_under_gate_first_equals_the_lone_pipelines(process, changers):
    W.check_bank(changers[16000], 16000, (37, 21, 30), (3, 3), gate_first=True)


# ---- 5. no CREPE, 6. the default path
def test_world_mode_builds_no_crepe_model(process, changers, monkeypatch):
    W.check_no_crepe(changers[16000], 16000, process, monkeypatch, 37)


def test_the_default_mode_keeps_its_path_and_bits(gpu_ctx, changers, monkeypatch, tmp_path):
    """`test_convert_wave_equals_the_chain[gap-24000]` of tests/test_pipeline_gpu.py, run from here with `f0_mode` left at its default."""
    from yukarin import Wave
    shim = P.set_up(monkeypatch, tmp_path, 'tiny')
    fs = 24000
    vc = changers[fs]
    x = P.wave_of('gap', fs)
    P.check_split('gap', x, fs, 51)
    pipe = pipeline.Pipeline(vc, W.param_of(vc), crepe_capacity='tiny', seed=3)
    assert pipe.f0_mode == 'crepe' and pipe.f0_fn is None
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3)
    want = P.chain(vc, W.param_of(vc), pipe.feature_class, Wave(x, fs), ref)
    got = pipe.convert_wave(Wave(x, fs))
    assert pipeline.calls == {'resident': 1, 'composed': 0} and got.wave.size == int(50 * P.FRAME_PERIOD / 1000 * fs) + 1
    assert P.same(got.wave, want)
    pipe.close()
    ref.close()
    P.close_shim(shim)
