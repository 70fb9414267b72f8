"""`pipeline.LivePipeline` without a GPU, on the host-side SIMT emulator, in WORLD mode at the smallest sizes that take every path: buffers of
0.02 s at 16 kHz (320 samples, 5 frames), a store that wraps, a convert margin, an encode margin, a decode margin (the composed path) and the
gate.  The emulator analyses a few frames a second; the GPU file runs the issue's sizes and CREPE mode.  Bodies: tests/live_pipeline_cases.py."""
import pytest

import live_pipeline_cases as L
import pipeline_cases as P
import pipeline_world_cases as W
from realtime_yukarin_amd import engine, pipeline, world_analysis, world_synth

FS, T = 16000, 0.02


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


def test_resident_equals_composed_on_a_ring_that_wraps(process, changer):
    """(0, 0.01, 0): 5-row segments, four live at an append (the retire rule keeps a window of slack); a ring of 22 rows wraps at the fifth push."""
    L.check_resident_equals_composed(changer, FS, 'world', None, T, (0.0, 0.01, 0.0), 6, ring_rows=22, ring_samples=1400, zero_at=2, wraps_by=5)


def test_an_encode_margin(process, changer):
    L.check_resident_equals_composed(changer, FS, 'world', None, T, (0.01, 0.01, 0.0), 3)


def test_a_decode_margin_takes_the_composed_path(process, changer):
    L.check_decode_margin_takes_the_composed_path(changer, FS, 'world', None, T, (0.0, 0.01, 0.01), 3)


def test_out_gate_routes(process, changer):
    L.check_out_gate(changer, FS, process, 'world', None, T, (0.0, 0.01, 0.0), 4, 400)


def test_arguments_are_checked():
    with pytest.raises(ValueError):
        pipeline.LivePipeline(None, None, 0.1, 0, 0, 0, f0_mode='harvest')
