"""The gate-first form of the wave-to-wave chain without a GPU, on the host-side SIMT emulator: flag on against flag off, bit for bit, for a lone
`Pipeline` and a `PipelineBank`; the counters that show the skipped work; poisoned feature blocks; the compaction kernel, the verdict call and the
masked window call against the gate's own calls; the split tracker entries; the frame-count rule; the composed fallback; every refusal.  The
networks run on windows of a few frames (the emulator runs them at about ten frames a second): the windows of 0.15 - 0.3 s, the bank behind an
output gate bank, the lone pipelines beside the bank and the bank's kept rows are the GPU tests'; the accumulated advance with kept rows is shown
here on a lone pipeline with windows of 0.1 s.
Cases: tests/pipeline_gate_first_cases.py."""
import numpy
import pytest

import pipeline_cases as P
import pipeline_gate_first_cases as G
import pipeline_many_cases as M
from realtime_yukarin_amd import engine, pipeline, world_analysis, world_synth
from realtime_yukarin_amd.output_gate import OutputGate

FS, SECONDS = 16000, 0.03


@pytest.fixture
def on_emulator(emu_ctx, monkeypatch):
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: emu_ctx)
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    return emu_ctx


@pytest.fixture
def process(on_emulator, monkeypatch, tmp_path):
    shim = P.set_up(monkeypatch, tmp_path, 1)
    monkeypatch.setattr(pipeline, 'calls_many', {'resident': 0, 'composed': 0})
    yield shim
    P.close_shim(shim)


@pytest.fixture
def changer(process, tmp_path):
    vc = P.voice_changer(P.write_models(tmp_path, FS), FS)
    yield vc
    vc._fused_core().set_discard(0, 0)
    P.close_voice_changer(vc)


def test_the_waves_are_what_their_names_say():
    G.check_counts(FS, SECONDS)
    G.check_counts(24000, 0.2)
    G.check_counts(24000, 0.15)


@pytest.mark.parametrize('advance, discard, gated_out', [(None, (0, 0), False), (160, (1, 1), True)])
def test_lone_pipeline_keeps_its_bits(on_emulator, changer, advance, discard, gated_out):
    gates = [OutputGate(1100, P.THRESHOLD, 0.5, ctx=on_emulator) for _ in range(2)] if gated_out else None
    G.check_lone(changer, 1, FS, SECONDS, advance, discard, gates)
    for g in gates or ():
        g.close()


def test_bank_keeps_its_bits_and_skips_the_work(process, changer):
    """Against the flag-off bank (the lone pipelines per stream are the GPU test's: the emulator would spend another minute on them)."""
    model = process._model(1)
    G.check_bank(changer, 1, FS, SECONDS, None, (1, 1), model.frames_through_network, with_lone=False)


def test_kept_rows_and_the_accumulated_advance(process, changer):
    """Windows of 0.1 s, 10 ms apart (21 frames, of which those whose support lies inside the window may be kept): the smallest that show it."""
    G.check_lone_kept_rows(changer, 1, FS, 0.1, 160)


def test_nothing_of_a_skipped_wave_is_read(process, changer):
    G.check_poisoned(changer, 1, FS, SECONDS, process._model(1))


def test_compaction_kernel(on_emulator, changer):
    G.check_compaction(on_emulator, changer._fused_core())


def test_compaction_equals_the_gate(on_emulator, changer):
    G.check_compaction_equals_the_gate(on_emulator, changer._fused_core(), 24000)


def test_masked_window_call_equals_the_single_call(on_emulator, changer):
    fs, hop = 16000, 80
    waves, frames = [], []
    for s in range(7):                                                      # more waves than ring slots
        n = 3 + s % 3
        x = P.wave_of('loud', fs, n * hop / fs, seed=s)
        if s % 4 == 1:
            x[x.size // 2:] *= numpy.float32(1e-5)
        if s % 4 == 2:
            x[:] = 0
        waves.append(x)
        frames.append(n)
    core = changer._fused_core()
    w = M.Windows(on_emulator, core, waves, frames, hop, fft=128)
    for lanes in (1, 2):
        core.set_lanes(lanes)
        G.check_masked_windows(on_emulator, core, w)
    core.set_lanes(1)


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
@pytest.mark.parametrize('fs', P.RATES)
def test_split_tracker_entries(process, fs, dtype):
    model = process._model(1)
    model.set_dtype(dtype)
    G.check_split_tracker(model, fs)
    model.set_dtype('f32')


def test_frame_count_rule(process):
    """Without the wave of 1 s (the emulator would spend half a minute on its 201 frames): that length is the GPU test's."""
    G.check_frame_rule(process._model(1), one_second=False)


def test_fallback_ignores_the_flag(process, changer, monkeypatch):
    """RY_DEVICE_GATE=0, then a feature class that is no CREPE class: the composed way, the flag ignored, the same bits."""
    from yukarin import Wave
    from yukarin.acoustic_feature import AcousticFeature
    on, off = G.make_pair(changer, 1)
    w = G.W('loud', FS, SECONDS)
    want = off.convert_wave(w).wave
    monkeypatch.setenv('RY_DEVICE_GATE', '0')
    before = dict(pipeline.calls)
    assert P.same(on.convert_wave(w).wave, want) and P.same(on.push(w, advance=0).wave, off.push(w, advance=0).wave)
    assert pipeline.calls['composed'] - before['composed'] == 3 and pipeline.calls['resident'] == before['resident']
    assert pipeline.calls.get('gated', 0) == before.get('gated', 0)
    assert P.same(on.flush().wave, off.flush().wave)
    monkeypatch.delenv('RY_DEVICE_GATE')

    class Plain(AcousticFeature):                                           # the same f0, but not named in encode.crepe_classes
        extract_f0 = pipeline.crepe_feature_class().extract_f0
    param = changer.acoustic_converter.config.dataset.acoustic_param
    other = [pipeline.PipelineBank(changer, param, 1, seeds=[3], crepe_capacity=1, feature_class=Plain, gate_first=g) for g in (True, False)]
    z = Wave(G.wave_of('zeros', FS, SECONDS), FS)
    before = dict(pipeline.calls_many)
    got, ref = other[0].convert_waves([z]), other[1].convert_waves([z])
    assert P.same(got[0].wave, ref[0].wave) and pipeline.calls_many['composed'] - before['composed'] == 2
    assert pipeline.calls_many.get('gated', 0) == before.get('gated', 0) and other[0].last_gate is None
    for p in other + [on, off]:
        p.close()


def test_refusals(on_emulator, process, changer):
    G.check_refusals(on_emulator, changer._fused_core(), process._model(1))
