"""`pipeline.LivePipelineBank` on the MI355X: SYN-8 predictors, `tiny` CREPE capacity, 16 kHz, as test_live_pipeline_gpu.py.  B = 3 streams with
different signals and seeds, buffers of 0.1 s (21 frames), the margins (0, 0.05, 0) and (0.1, 0.1, 0) over 8 pushes on rings of 85 / 106 rows
per stream that wrap, with a buffer of zeros, a stream that sits a push out and a stream that is flushed mid-run, in CREPE and in WORLD mode; the
shipped margins (1 s buffers, 0 / 0.5 / 0) once at B = 2; the gates on the card.  Every returned `Wave` equals the lone `LivePipeline`'s of its
stream, bit for bit.  Bodies: tests/live_bank_cases.py."""
import pytest

import live_bank_cases as LB
import pipeline_cases as P
import pipeline_world_cases as W
from realtime_yukarin_amd import pipeline

pytestmark = pytest.mark.gpu
FS = 16000
CASES = {'convert_margin': ((0.0, 0.05, 0.0), 85, 6500), 'all_but_decode': ((0.1, 0.1, 0.0), 106, 8100)}


@pytest.fixture(scope='module')
def changer(gpu_ctx, tmp_path_factory):
    vc = P.voice_changer(P.write_models(tmp_path_factory.mktemp('live_bank'), FS), FS)
    yield vc
    P.close_voice_changer(vc)


@pytest.fixture
def process(gpu_ctx, monkeypatch, tmp_path, request):
    mode = request.param
    if mode == 'world':
        shim = W.set_up(monkeypatch)
    else:
        shim = P.set_up(monkeypatch, tmp_path, 'tiny')
    monkeypatch.setattr(pipeline, 'routes', {'gate_device': 0, 'gate_host': 0})
    yield mode
    P.close_shim(shim)


@pytest.mark.parametrize('case', sorted(CASES))
@pytest.mark.parametrize('process', ['crepe', 'world'], indirect=True)
def test_eight_pushes_of_three_streams(process, changer, case):
    """Stream 0 has a buffer of zeros, stream 1 sits push 2 out, stream 2 is flushed behind push 4 and starts a new signal."""
    margins, ring_rows, ring_samples = CASES[case]
    LB.check_bank_equals_lone(changer, FS, process, 'tiny', 0.1, margins, 8, 3, ring_rows=ring_rows, ring_samples=ring_samples, sit_out=(1, 2), flush=(2, 3),
                              zero=(0, 3), kept_rows=21)


@pytest.mark.parametrize('process', ['crepe'], indirect=True)
def test_the_shipped_margins(process, changer):
    LB.check_bank_equals_lone(changer, FS, process, 'tiny', 1.0, (0.0, 0.5, 0.0), 3, 2, zero=None)


@pytest.mark.parametrize('process', ['crepe'], indirect=True)
def test_out_gates_run_on_the_card_once_per_call(process, changer, gpu_ctx):
    """`check_out_gate` holds the bank's route counter to one per call (6), not one per stream (18)."""
    assert LB.check_out_gate(changer, FS, None, process, 'tiny', 0.1, (0.0, 0.05, 0.0), 6, 3, 2048) == 'gate_device'
