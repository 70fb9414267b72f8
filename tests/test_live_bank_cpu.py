"""`pipeline.LivePipelineBank` without a GPU, on the host-side SIMT emulator, in WORLD mode at the sizes of test_live_pipeline_cpu.py: B = 2,
buffers of 0.02 s at 16 kHz (320 samples, 5 frames), margins (0, 0.01, 0), rings of 22 rows per stream that wrap, 6 pushes with a buffer of
zeros, a stream that sits a push out and a stream that is flushed behind the third push and starts a new signal.  Every returned `Wave` is
held to the lone `LivePipeline` of its stream, bit for bit.  Bodies: tests/live_bank_cases.py."""
import pytest

import live_bank_cases as LB
import pipeline_cases as P
import pipeline_world_cases as W
from realtime_yukarin_amd import engine, pipeline, world_analysis, world_synth

FS, T = 16000, 0.02
MARGINS = (0.0, 0.01, 0.0)


@pytest.fixture
def process(emu_ctx, monkeypatch):
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: emu_ctx)
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    shim = W.set_up(monkeypatch)
    monkeypatch.setattr(pipeline, 'routes', {'gate_device': 0, 'gate_host': 0})
    yield emu_ctx
    P.close_shim(shim)


@pytest.fixture
def changer(process, tmp_path):
    vc = P.voice_changer(P.write_models(tmp_path, FS), FS)
    yield vc
    P.close_voice_changer(vc)


def test_every_stream_equals_its_lone_pipeline(process, changer):
    """Stream 0 has a buffer of zeros, stream 1 sits push 1 out, stream 0 is flushed behind push 3 and starts a new signal; 5 kept rows a push."""
    LB.check_bank_equals_lone(changer, FS, 'world', None, T, MARGINS, 6, 2, ring_rows=22, ring_samples=1400, sit_out=(1, 1), flush=(0, 2), kept_rows=5)


def test_a_decode_margin_sends_every_stream_down_the_composed_path(process, changer):
    LB.check_decode_margin_is_composed(changer, FS, 'world', None, T, (0.0, 0.01, 0.01), 3, 2)


def test_a_misfit_track_demotes_its_stream_alone(process, changer):
    LB.check_a_misfit_demotes_one_stream(changer, FS, T, MARGINS, 3)


def test_out_gate_routes(process, changer):
    assert LB.check_out_gate(changer, FS, process, 'world', None, T, MARGINS, 4, 2, 400) == 'gate_host'


def test_arguments_are_checked():
    with pytest.raises(ValueError):
        pipeline.LivePipelineBank(None, None, 0, 0.1, 0, 0, 0)
    with pytest.raises(ValueError):
        pipeline.LivePipelineBank(None, None, 2, 0.1, 0, 0, 0, seeds=[1, 2, 3])
    with pytest.raises(ValueError):
        pipeline.LivePipelineBank(None, None, 2, 0.1, 0, 0, 0, f0_mode='harvest')
