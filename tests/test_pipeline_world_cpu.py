"""WORLD mode without a GPU, on the host-side SIMT emulator: the track ingest of the analysis unit against its numpy statement at every size, its
refusals by return code, and `Pipeline(f0_mode='world')` / `PipelineBank(f0_mode='world')` against the composed chain with the same f0 callable, bit
for bit, at the smallest sizes that take every path (the emulator analyses a few frames a second; the GPU file runs the full sizes).
Cases and bodies: tests/pipeline_world_cases.py."""
import numpy
import pytest

import pipeline_cases as P
import pipeline_world_cases as W
from realtime_yukarin_amd import engine, pipeline, world_analysis, world_synth


@pytest.fixture
def on_emulator(emu_ctx, monkeypatch):
    """Every lazily created context of the shims and the audio units is the emulator's."""
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: emu_ctx)
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    return emu_ctx


@pytest.fixture
def process(on_emulator, monkeypatch):
    shim = W.set_up(monkeypatch)
    yield on_emulator
    P.close_shim(shim)


@pytest.fixture
def changer(process, tmp_path):
    """fs -> the voice changer over SYN-8 predictors at that rate (made on first use, closed with the test)."""
    made = {}

    def make(fs):
        if fs not in made:
            d = tmp_path / str(fs)
            d.mkdir()
            made[fs] = P.voice_changer(P.write_models(d, fs), fs)
        return made[fs]
    yield make
    for vc in made.values():
        P.close_voice_changer(vc)


# ---- 1. the ingest alone
@pytest.mark.parametrize('period', W.PERIODS)
def test_ingest_equals_the_numpy_statement(emu_ctx, period):
    W.check_ingest_sizes(emu_ctx, period)


def test_ingest_on_poisoned_buffers(emu_ctx):
    W.check_ingest_poison(emu_ctx)


def test_ingest_refusals_leave_the_previous_track(emu_ctx):
    W.check_ingest_refusals(emu_ctx)


@pytest.mark.parametrize('fs', P.RATES)
def test_the_extract_calls_take_the_ingested_track_in_place(emu_ctx, fs):
    W.check_extract_takes_the_track_in_place(emu_ctx, fs)


def test_the_frame_count_rule():
    """`int(1000 * n / fs / frame_period) + 1`: one sample either side of a hop multiple changes the count."""
    for fs in P.RATES:
        hop = W.hop_of(fs)
        assert [world_analysis.harvest_frames(n, fs, P.FRAME_PERIOD) for n in (1, hop - 1, hop, hop + 1, 37 * hop - 1, 37 * hop, 37 * hop + 1)] == [1, 1, 2, 2, 37, 38, 38]
    assert W.f0_track(2960, 16000)[0].size == 38 and (W.f0_track(2960, 16000)[0] == 0).any() and (W.f0_track(2960, 16000)[0] != 0).any()


# ---- 2. the pipeline
@pytest.mark.parametrize('fs', P.RATES)
def test_convert_wave_equals_the_chain(process, changer, fs):
    """The shortest wave (one sample, one frame), one sample either side of a hop multiple (4 and 5 frames), an all-unvoiced track."""
    from yukarin import Wave
    vc, hop = changer(fs), W.hop_of(fs)
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3, ctx=process)
    for n, fn in ((1, W.f0_fn), (4 * hop - 1, W.f0_fn), (4 * hop, W.f0_fn), (4 * hop + 1, W.unvoiced_fn)):
        x = W.half_quiet_wave(n, fs, n)
        W.check_convert_wave(vc, fs, x, fn, W.chain(vc, W.param_of(vc), fn, Wave(x, fs), ref))
    ref.close()


def test_push_and_flush_equal_the_chain(process, changer):
    W.check_push_flush(changer(24000), 24000, process, 6, (2, 2))


def test_refused_tracks_and_the_composed_fallbacks(process, changer, monkeypatch):
    vc = changer(16000)
    W.check_refused_tracks(vc, 16000, process, 4)
    W.check_misfit_takes_the_composed_path(vc, 16000, process, 4)
    W.check_other_fallbacks(vc, 16000, process, monkeypatch, 3)


# ---- 3. the bank, 4. the gate in front
def test_bank_streams_equal_their_lone_pipelines(process, changer):
    W.check_bank(changer(16000), 16000, (5, 3, 4), (1, 1))


def test_bank_out_gate_with_a_silent_stream(process, changer):
    W.check_bank_out_gate(changer(16000), 16000, process, (10, 10, 10), (1, 0), 160, rounds=2)


def test_gate_first_skips_the_host_f0_call(process, changer):
    W.check_gate_first(changer(24000), 24000, (4, 3, 2), (1, 0))


# ---- 5. no CREPE, 6. the default path
def test_world_mode_builds_no_crepe_model(process, changer, monkeypatch):
    W.check_no_crepe(changer(16000), 16000, process, monkeypatch, 3)


def test_f0_mode_is_checked():
    with pytest.raises(ValueError):
        pipeline.Pipeline(None, None, f0_mode='harvest')
    with pytest.raises(ValueError):
        pipeline.Pipeline(None, None, f0_fn=W.f0_fn)


def test_the_default_mode_keeps_its_path_and_bits(on_emulator, monkeypatch, tmp_path):
    """A CREPE-mode case of tests/test_pipeline_cpu.py, run from here with `f0_mode` left at its default: the resident path, the chain's bits."""
    from yukarin import Wave
    shim = P.set_up(monkeypatch, tmp_path, 1)
    fs = 16000
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    param = W.param_of(vc)
    pipe = pipeline.Pipeline(vc, param, crepe_capacity=1, seed=3)
    assert pipe.f0_mode == 'crepe' and pipe.f0_fn is None
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3, ctx=on_emulator)
    x = P.wave_of('loud', fs, 0.02)
    x[x.size // 2:] *= numpy.float32(1e-5)
    want = P.chain(vc, param, pipe.feature_class, Wave(x, fs), ref)
    assert P.same(pipe.convert_wave(Wave(x, fs)).wave, want) and pipeline.calls == {'resident': 1, 'composed': 0}
    pipe.close()
    ref.close()
    P.close_voice_changer(vc)
    P.close_shim(shim)
