"""`pipeline.LivePipeline` on the MI355X: SYN-8 predictors, `tiny` CREPE capacity, 16 kHz.  Buffers of 0.1 s (1600 samples, 21 frames) with the
margins (0, 0.05, 0) and (0.1, 0.1, 0) over 8 pushes on a ring that wraps, one buffer of zeros and a flush, in CREPE and in WORLD mode; the
shipped margins (1 s buffers, 0 / 0.5 / 0) once; a decode margin (the composed path); the gate on the card.  Every returned chunk equals the
composed path's, bit for bit.  The rings are sized by the retire rule (`worker.retire_time` keeps one window of slack): with 21-row segments,
(0, 0.05, 0) has four segments live at an append and a ring of 85 rows wraps at the fifth push; (0.1, 0.1, 0) has five (105 rows), so the
earliest a ring can wrap is the sixth push, which a ring of 106 rows does.  Bodies: tests/live_pipeline_cases.py."""
import pytest

import live_pipeline_cases as L
import pipeline_cases as P
import pipeline_world_cases as W
from realtime_yukarin_amd import pipeline

pytestmark = pytest.mark.gpu
FS = 16000
CASES = {'convert_margin': ((0.0, 0.05, 0.0), 85, 6500, 5), 'all_but_decode': ((0.1, 0.1, 0.0), 106, 8100, 6)}


@pytest.fixture(scope='module')
def changer(gpu_ctx, tmp_path_factory):
    vc = P.voice_changer(P.write_models(tmp_path_factory.mktemp('live'), FS), FS)
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
def test_eight_pushes_on_a_ring_that_wraps(process, changer, case):
    margins, ring_rows, ring_samples, wraps_by = CASES[case]
    L.check_resident_equals_composed(changer, FS, process, 'tiny', 0.1, margins, 8, ring_rows=ring_rows, ring_samples=ring_samples, zero_at=3,
                                     wraps_by=wraps_by)


@pytest.mark.parametrize('process', ['crepe'], indirect=True)
def test_the_shipped_margins(process, changer):
    L.check_resident_equals_composed(changer, FS, process, 'tiny', 1.0, (0.0, 0.5, 0.0), 4)


@pytest.mark.parametrize('process', ['crepe', 'world'], indirect=True)
def test_a_decode_margin_takes_the_composed_path(process, changer):
    L.check_decode_margin_takes_the_composed_path(changer, FS, process, 'tiny', 0.1, (0.0, 0.05, 0.05), 4)


@pytest.mark.parametrize('process', ['crepe'], indirect=True)
def test_out_gate_runs_on_the_card(process, changer, gpu_ctx):
    before = pipeline.routes['gate_device']
    L.check_out_gate(changer, FS, None, process, 'tiny', 0.1, (0.0, 0.05, 0.0), 6, 2048)
    assert pipeline.routes['gate_device'] == before + 6
