"""The device route into the output gate on the MI355X: the synthesizer entries that leave their samples on the card against the host entries
on a twin, the gates fed on the card against the gates fed from the host, and `Pipeline.push(out_gate=)` / `PipelineBank.push(out_gate=)` on the
new route against the host route run by hand on a twin (`push` without a gate, then the gate's `push`), bit for bit, in CREPE mode and in WORLD
mode with the fixed track of tests/pipeline_world_cases.py; the counters; every refusal.  SYN-8 predictors at 24 kHz, windows of 12 frames, gate
chunks of 1025 and 2048 samples.  Cases and bodies: tests/out_gate_device_cases.py."""
import numpy
import pytest

import out_gate_device_cases as D
import pipeline_cases as P
import pipeline_world_cases as W
from realtime_yukarin_amd import pipeline

pytestmark = pytest.mark.gpu
FS, FRAMES = 24000, 12                          # ten frames a push: 1200 samples, so that some pushes complete a chunk and some do not


@pytest.fixture(scope='module')
def changer(gpu_ctx, tmp_path_factory):
    vc = P.voice_changer(P.write_models(tmp_path_factory.mktemp('outgate_device'), FS), FS)
    yield vc
    P.close_voice_changer(vc)


@pytest.fixture
def world(gpu_ctx, monkeypatch):
    shim = W.set_up(monkeypatch)
    monkeypatch.setattr(pipeline, 'routes', {'gate_device': 0, 'gate_host': 0})
    yield gpu_ctx
    P.close_shim(shim)


@pytest.fixture
def crepe(gpu_ctx, monkeypatch, tmp_path):
    shim = P.set_up(monkeypatch, tmp_path, 'tiny')
    monkeypatch.setattr(pipeline, 'calls_many', {'resident': 0, 'composed': 0})
    monkeypatch.setattr(pipeline, 'routes', {'gate_device': 0, 'gate_host': 0})
    yield gpu_ctx
    P.close_shim(shim)


# ---- 1. the synthesizer alone
@pytest.mark.parametrize('device_rows, poison', [(False, False), (True, True)])
def test_lone_synthesizer_leaves_its_samples_on_the_card(gpu_ctx, device_rows, poison):
    D.check_lone_synth(gpu_ctx, device_rows=device_rows, poison=poison)


@pytest.mark.parametrize('B, device_rows, poison', [(3, False, False), (3, True, True), (1, False, True)])
def test_bank_leaves_its_samples_on_the_card(gpu_ctx, B, device_rows, poison):
    D.check_bank_synth(gpu_ctx, B, device_rows=device_rows, poison=poison)


def test_bank_item_by_item_lays_the_streams_back_to_back(gpu_ctx):
    D.check_bank_item_by_item(gpu_ctx)


# ---- 2. the gate fed on the card
@pytest.mark.parametrize('sequence', ['none', 'exact', 'backlog'])
@pytest.mark.parametrize('signal', ['voiced', 'noise1e-6'])
@pytest.mark.parametrize('dtype', D.GATE_DTYPES)
@pytest.mark.parametrize('chunk', D.GATE_CHUNKS)
def test_gate_fed_on_the_card(gpu_ctx, chunk, dtype, signal, sequence):
    D.check_gate_fed_on_the_card(gpu_ctx, chunk, dtype, signal, sequence, poison=(sequence == 'backlog'))


@pytest.mark.parametrize('chunk, dtype', [(1025, numpy.float32), (2048, numpy.float64)])
def test_gate_bank_fed_on_the_card(gpu_ctx, chunk, dtype):
    D.check_gate_bank_fed_on_the_card(gpu_ctx, chunk, dtype)


def test_host_fallback_gate_has_no_device_form(gpu_ctx):
    D.check_host_fallback_has_no_device_form(gpu_ctx)


@pytest.mark.parametrize('chunk, dtype', [(1025, numpy.float32), (2048, numpy.float64)])
def test_lone_pipeline_world_mode(world, changer, monkeypatch, chunk, dtype):
    D.check_lone_pipeline(changer, world, FS, 'world', None, FRAMES, chunk, dtype, monkeypatch)


@pytest.mark.parametrize('chunk, dtype', [(1025, numpy.float64), (2048, numpy.float32)])
def test_lone_pipeline_crepe_mode(crepe, changer, monkeypatch, chunk, dtype):
    D.check_lone_pipeline(changer, crepe, FS, 'crepe', 'tiny', FRAMES, chunk, dtype, monkeypatch)


def test_bank_pipeline_world_mode(world, changer):
    D.check_bank_pipeline(changer, world, FS, 'world', None, FRAMES, 2048, numpy.float64)


def test_bank_pipeline_crepe_mode(crepe, changer):
    D.check_bank_pipeline(changer, crepe, FS, 'crepe', 'tiny', FRAMES, 1025, numpy.float32)


# ---- 3. the counters
def test_counters_say_device_route(world, changer):
    D.check_counters(changer, world, FS, FRAMES)


# ---- 4. refusals
def test_lone_refusals(gpu_ctx):
    D.check_lone_refusals(gpu_ctx)


def test_bank_refusals(gpu_ctx):
    D.check_bank_refusals(gpu_ctx)
