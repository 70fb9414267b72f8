"""The device route into the output gate without a GPU, on the host-side SIMT emulator: the synthesizer entries that leave their samples on the
card against the host entries on a twin, the gates fed on the card against the gates fed from the host, and `Pipeline.push(out_gate=)` /
`PipelineBank.push(out_gate=)` on the new route against the host route, bit for bit; the counters; every refusal.  The synthesizer and the gates
run at the sizes of the GPU file; the pipelines run WORLD mode on windows of six frames (the emulator analyses a few frames a second) and CREPE
mode on one lone stream of five-frame windows.  Cases and bodies: tests/out_gate_device_cases.py."""
import numpy
import pytest

import out_gate_device_cases as D
import pipeline_cases as P
import pipeline_world_cases as W
from realtime_yukarin_amd import engine, pipeline, world_analysis, world_synth


@pytest.fixture
def on_emulator(emu_ctx, monkeypatch):
    """Every lazily created context of the shims and the audio units is the emulator's."""
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: emu_ctx)
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(pipeline, 'routes', {'gate_device': 0, 'gate_host': 0})
    return emu_ctx


@pytest.fixture
def world_changer(on_emulator, monkeypatch, tmp_path):
    shim = W.set_up(monkeypatch)
    vc = P.voice_changer(P.write_models(tmp_path, 24000), 24000)
    yield vc
    P.close_voice_changer(vc)
    P.close_shim(shim)


# ---- 1. the synthesizer alone
@pytest.mark.parametrize('device_rows, poison', [(False, False), (True, True)])
def test_lone_synthesizer_leaves_its_samples_on_the_card(emu_ctx, device_rows, poison):
    D.check_lone_synth(emu_ctx, device_rows=device_rows, poison=poison)


@pytest.mark.parametrize('B, device_rows, poison', [(3, False, False), (3, True, True), (1, False, True)])
def test_bank_leaves_its_samples_on_the_card(emu_ctx, B, device_rows, poison):
    D.check_bank_synth(emu_ctx, B, device_rows=device_rows, poison=poison)


def test_bank_item_by_item_lays_the_streams_back_to_back(emu_ctx):
    D.check_bank_item_by_item(emu_ctx)


# ---- 2. the gate fed on the card
@pytest.mark.parametrize('sequence', ['none', 'exact', 'backlog'])
@pytest.mark.parametrize('signal', ['voiced', 'noise1e-6'])
@pytest.mark.parametrize('chunk, dtype', [(1025, numpy.float32), (2048, numpy.float64)])
def test_gate_fed_on_the_card(emu_ctx, chunk, dtype, signal, sequence):
    D.check_gate_fed_on_the_card(emu_ctx, chunk, dtype, signal, sequence, poison=(sequence == 'backlog'))


@pytest.mark.parametrize('chunk, dtype', [(1025, numpy.float64), (2048, numpy.float32)])
def test_gate_fed_on_the_card_other_dtype(emu_ctx, chunk, dtype):
    D.check_gate_fed_on_the_card(emu_ctx, chunk, dtype, 'voiced', 'backlog')


def test_gate_bank_fed_on_the_card(emu_ctx):
    D.check_gate_bank_fed_on_the_card(emu_ctx, 1025, numpy.float32)


def test_host_fallback_gate_has_no_device_form(emu_ctx):
    D.check_host_fallback_has_no_device_form(emu_ctx)


def test_lone_pipeline_world_mode(on_emulator, world_changer, monkeypatch):
    other = engine.Context(0, on_emulator.lib)                               # a gate of another context: the host route
    D.check_lone_pipeline(world_changer, on_emulator, 24000, 'world', None, 6, 1025, numpy.float32, monkeypatch, other_ctx=other)
    other.close()


def test_bank_pipeline_world_mode(on_emulator, world_changer):
    D.check_bank_pipeline(world_changer, on_emulator, 24000, 'world', None, 6, 1025, numpy.float32)


def test_lone_pipeline_crepe_mode(on_emulator, monkeypatch, tmp_path):
    shim = P.set_up(monkeypatch, tmp_path, 1)
    vc = P.voice_changer(P.write_models(tmp_path, 24000), 24000)
    D.check_lone_pipeline(vc, on_emulator, 24000, 'crepe', 1, 5, 1025, numpy.float64, monkeypatch)
    P.close_voice_changer(vc)
    P.close_shim(shim)


# ---- 3. the counters
def test_counters_say_device_route(on_emulator, world_changer):
    D.check_counters(world_changer, on_emulator, 24000, 8)


# ---- 4. refusals
def test_lone_refusals(emu_ctx):
    D.check_lone_refusals(emu_ctx)


def test_bank_refusals(emu_ctx):
    D.check_bank_refusals(emu_ctx)
