"""The gate-first form of the wave-to-wave chain on the MI355X: flag on against flag off, bit for bit, for a lone `Pipeline` and a `PipelineBank` (with
and without `advance`, output gates and a discard), the counters that show the skipped work and the kept rows, poisoned feature blocks, the
compaction kernel and the masked window call against the gate's own calls, the split tracker entries, the frame-count rule and every refusal.
`tiny` CREPE capacity, SYN-8 predictors, windows of 0.2 s at 24 kHz.  Cases: tests/pipeline_gate_first_cases.py."""
import numpy
import pytest

import pipeline_cases as P
import pipeline_gate_first_cases as G
import pipeline_many_cases as M
from realtime_yukarin_amd import pipeline
from realtime_yukarin_amd.output_gate import OutputGate, OutputGateBank

pytestmark = pytest.mark.gpu
FS, SECONDS, ADVANCE = 24000, 0.2, 480


@pytest.fixture(scope='module')
def changer(gpu_ctx, tmp_path_factory):
    vc = P.voice_changer(P.write_models(tmp_path_factory.mktemp('models'), FS), FS)
    yield vc
    P.close_voice_changer(vc)


@pytest.fixture(params=['f32', 'bf16x3'])
def process(request, gpu_ctx, monkeypatch, tmp_path, changer):
    shim = P.set_up(monkeypatch, tmp_path, 'tiny', request.param)
    monkeypatch.setattr(pipeline, 'calls_many', {'resident': 0, 'composed': 0})
    yield shim
    changer._fused_core().set_discard(0, 0)
    P.close_shim(shim)


def test_the_waves_are_what_their_names_say():
    G.check_counts(FS, SECONDS)
    G.check_counts(FS, 0.15)


@pytest.mark.parametrize('advance, discard, gated_out', [(None, (0, 0), False), (ADVANCE, (10, 10), True), (ADVANCE, (0, 0), False)])
def test_lone_pipeline_keeps_its_bits(gpu_ctx, process, changer, advance, discard, gated_out):
    gates = [OutputGate(2048, P.THRESHOLD, 0.5) for _ in range(2)] if gated_out else None
    G.check_lone(changer, 'tiny', FS, SECONDS, advance, discard, gates, kept=True)
    for g in gates or ():
        g.close()


@pytest.mark.parametrize('advance, discard', [(None, (0, 0)), (ADVANCE, (10, 10))])
def test_bank_keeps_its_bits_and_skips_the_work(process, changer, advance, discard):
    G.check_bank(changer, 'tiny', FS, SECONDS, advance, discard, process._model('tiny').frames_through_network)


def test_bank_with_an_output_gate_bank(process, changer):
    made = []

    def gate_bank():
        made.append(OutputGateBank(3, 2048, P.THRESHOLD, 0.5))
        return made[-1]
    G.check_bank(changer, 'tiny', FS, SECONDS, ADVANCE, (10, 10), process._model('tiny').frames_through_network, gate_bank)
    for g in made:
        g.close()


def test_lone_kept_rows_and_the_accumulated_advance(process, changer):
    G.check_lone_kept_rows(changer, 'tiny', FS, SECONDS, ADVANCE)


def test_nothing_of_a_skipped_wave_is_read(process, changer):
    G.check_poisoned(changer, 'tiny', FS, SECONDS, process._model('tiny'))


def test_compaction_kernel(gpu_ctx, changer):
    G.check_compaction(gpu_ctx, changer._fused_core())


def test_compaction_equals_the_gate(gpu_ctx, changer):
    G.check_compaction_equals_the_gate(gpu_ctx, changer._fused_core(), FS)


def test_masked_window_call_equals_the_single_call(gpu_ctx, changer):
    hop = FS * P.FRAME_PERIOD // 1000
    kinds = ('loud', 'gap', 'zeros', 'gap_silent_ends', 'loud', 'zeros', 'gap')       # more waves than ring slots
    waves = [P.wave_of(k, FS, 0.15 + 0.01 * s, seed=s) for s, k in enumerate(kinds)]
    core = changer._fused_core()
    w = M.Windows(gpu_ctx, core, waves, [x.size // hop + 1 for x in waves], hop)
    for lanes in (1, 2):
        core.set_lanes(lanes)
        G.check_masked_windows(gpu_ctx, core, w)
    core.set_lanes(1)


@pytest.mark.parametrize('fs', P.RATES)
def test_split_tracker_entries(process, fs):
    G.check_split_tracker(process._model('tiny'), fs)


def test_frame_count_rule(process):
    G.check_frame_rule(process._model('tiny'))


def test_refusals(gpu_ctx, process, changer):
    G.check_refusals(gpu_ctx, changer._fused_core(), process._model('tiny'))
