"""The many-waves wave-to-wave chain without a GPU, on the host-side SIMT emulator: `ry_gather_rows` against numpy, the gate over many waves against
`ry_vc_gate` per wave, `ry_analysis_extract_many_resident` against `extract_resident` per wave, `ry_vc_enqueue_waves_device` against
`ry_vc_enqueue_wave_device` per wave, every refusal by return code, and `PipelineBank` against lone `Pipeline`s on either route.  The networks run
on waves of a few frames (the emulator runs them at about ten frames a second).  Cases: tests/pipeline_many_cases.py."""
import itertools

import numpy
import pytest

import pipeline_cases as P
import pipeline_many_cases as M
from realtime_yukarin_amd import engine, gate, pipeline, world_analysis, world_synth


@pytest.fixture
def on_emulator(emu_ctx, monkeypatch):
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: emu_ctx)
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    return emu_ctx


@pytest.fixture
def core(on_emulator, tmp_path):
    vc = P.voice_changer(P.write_models(tmp_path, 16000), 16000)
    yield vc._fused_core()
    P.close_voice_changer(vc)


def test_gather_rows_equals_numpy(emu_ctx):
    M.check_gather_rows(emu_ctx)


def test_gather_rows_refusals(emu_ctx):
    M.check_gather_rows_refusals(emu_ctx)


@pytest.mark.parametrize('fs', P.RATES)
@pytest.mark.parametrize('fft', [1024, 128])
def test_gate_over_three_lengths_in_every_order(on_emulator, core, fs, fft):
    """One hop, a length that is no multiple of the hop and 0.25 s in one call, in every permutation: every wave keeps its bits."""
    waves, frames, hop = M.gate_lengths(fs)
    singles = None
    for order in itertools.permutations(range(3)):
        singles = M.check_gate_waves(on_emulator, core, waves, frames, hop, fft=fft, order=order, singles=singles)


def test_gate_over_the_kinds(on_emulator, core):
    """loud, exact-zero middle, all zeros, silent ends in one call; each wave is first held to the host gate, which splits it as its name says."""
    fs = 24000
    waves = [P.wave_of(kind, fs) for kind in P.KINDS]
    masks = [P.check_split(kind, x, fs) for kind, x in zip(P.KINDS, waves)]
    feats, want = M.check_gate_waves(on_emulator, core, waves, [len(m) for m in masks], fs * P.FRAME_PERIOD // 1000)
    for (m, _, _), host in zip(want, masks):
        assert numpy.array_equal(m, host)


def test_a_quiet_wave_does_not_inherit_all_frames_from_a_loud_neighbour(on_emulator, core):
    fs = 16000
    waves, frames, thr = M.loud_and_quiet(fs)
    for order in ((0, 1), (1, 0)):
        feats, want = M.check_gate_waves(on_emulator, core, waves, frames, fs * P.FRAME_PERIOD // 1000, thr=thr, order=order)
    assert want[0][0].all() and not want[1][0].all()


def test_gate_waves_refusals(on_emulator, core):
    M.check_gate_waves_refusals(on_emulator, core)


@pytest.mark.parametrize('fs', P.RATES)
def test_extract_many_resident_equals_extract_resident(emu_ctx, fs):
    M.check_extract_many_resident(emu_ctx, fs)


def short_windows(ctx, core, count):
    """`count` windows of 3 .. 5 frames at 16 kHz: a loud one, one that is half below the gate, an all-silent one, then loud ones."""
    fs, hop = 16000, 80
    waves, frames = [], []
    for s in range(count):
        n = 3 + s % 3
        x = P.wave_of('loud', fs, n * hop / fs, seed=s)
        if s % 4 == 1:
            x[x.size // 2:] *= numpy.float32(1e-5)
        if s % 4 == 2:
            x[:] = 0
        waves.append(x)
        frames.append(n)
    return M.Windows(ctx, core, waves, frames, hop, fft=128)


def test_enqueue_waves_device_equals_the_single_call(on_emulator, core):
    """Three windows -- loud, half silent, all silent -- with and without a discard hint, in two orders."""
    w = short_windows(on_emulator, core, 3)
    assert [c[3] for c in w.single((0, 0))][2] == 0 and 0 < w.single((0, 0))[1][3] < w.frames[1]
    w.check()
    w.check(order=(2, 0, 1))
    w.check(discard=(1, 1))


def test_enqueue_waves_device_with_more_waves_than_ring_slots(on_emulator, core):
    """Seven windows on a ring of six, one lane and two: a slot comes round again within the call."""
    w = short_windows(on_emulator, core, 7)
    for lanes in (1, 2):
        core.set_lanes(lanes)
        assert core.ring == 6
        w.check()
    core.set_lanes(1)


def test_enqueue_waves_device_refusals(on_emulator, core):
    M.check_enqueue_waves_refusals(on_emulator, core)


@pytest.fixture
def process(on_emulator, monkeypatch, tmp_path):
    shim = P.set_up(monkeypatch, tmp_path, 1)
    monkeypatch.setattr(pipeline, 'calls_many', {'resident': 0, 'composed': 0})
    yield on_emulator
    P.close_shim(shim)


def short_wave(fs, seed=0, silent=False):
    x = P.wave_of('loud', fs, 0.02, seed)
    x[x.size // 2:] *= numpy.float32(1e-5)
    if silent:
        x[:] = 0
    return x


def test_bank_equals_lone_pipelines(process, tmp_path):
    """`convert_waves` against `Pipeline.convert_wave` per wave, then three `push` rounds over three streams with distinct seeds and a flush against
    three lone `Pipeline`s: one stream sits a round out, one ends and restarts, one is all silent."""
    from yukarin import Wave
    fs, seeds = 16000, [3, 4, 5]
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    param = vc.acoustic_converter.config.dataset.acoustic_param
    bank = pipeline.PipelineBank(vc, param, 3, seeds=seeds, crepe_capacity=1)
    lone = [pipeline.Pipeline(vc, param, crepe_capacity=1, seed=s) for s in seeds]
    waves = [Wave(short_wave(fs, 0), fs), Wave(short_wave(fs, 1, silent=True), fs), Wave(P.wave_of('loud', fs, 0.03, 2), fs)]
    got = bank.convert_waves(waves)
    for g, w in zip(got, waves):
        assert P.same(g.wave, lone[0].convert_wave(w).wave)
    assert pipeline.calls_many == {'resident': 1, 'composed': 0}
    mk = lambda seed, silent=False: Wave(short_wave(fs, seed, silent), fs)
    rounds = [([mk(1), mk(2), mk(3, True)], ()), ([None, mk(4), mk(5, True)], (1,)), ([mk(6), mk(7), mk(8, True)], ())]
    M.check_bank_against_lone_pipelines(bank, lone, rounds, (1, 1))
    assert pipeline.calls_many == {'resident': 4, 'composed': 0}
    bank.close()
    for p in lone:
        p.close()
    P.close_voice_changer(vc)


def test_the_composed_route_runs_through_the_bank(process, tmp_path):
    """A float64 wave that does not round-trip through float32 sends the whole call down the chain of the separate calls: the same bits, counted in
    `calls_many`."""
    from yukarin import Wave
    fs, seeds = 16000, [3, 4]
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    param = vc.acoustic_converter.config.dataset.acoustic_param
    bank = pipeline.PipelineBank(vc, param, 2, seeds=seeds, crepe_capacity=1)
    lone = [pipeline.Pipeline(vc, param, crepe_capacity=1, seed=s) for s in seeds]
    x64 = short_wave(fs).astype(numpy.float64)
    x64[100] += 2.0 ** -40
    rounds = [([Wave(x64, fs), Wave(short_wave(fs, 1), fs)], (0,))]
    M.check_bank_against_lone_pipelines(bank, lone[:1] + lone[1:], rounds, (1, 1))
    assert pipeline.calls_many == {'resident': 0, 'composed': 1}
    bank.close()
    for p in lone:
        p.close()
    P.close_voice_changer(vc)


def test_mixed_rates_run_the_composed_route_through_the_bank(process, tmp_path):
    """A 16 kHz and a 24 kHz wave in one call: the bank takes the chain of the separate calls for both while the lone pipelines stay on their resident
    paths -- the same bits, in `push` with the flush and in `convert_waves` (whose composed arm also takes a float64 wave that does not round-trip)."""
    from yukarin import Wave
    fs, seeds = 16000, [3, 4]
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    param = vc.acoustic_converter.config.dataset.acoustic_param
    bank = pipeline.PipelineBank(vc, param, 2, seeds=seeds, crepe_capacity=1)
    lone = [pipeline.Pipeline(vc, param, crepe_capacity=1, seed=s) for s in seeds]
    mixed = [Wave(short_wave(16000), 16000), Wave(short_wave(24000, 1), 24000)]
    M.check_bank_against_lone_pipelines(bank, lone, [(mixed, ())], (1, 1))
    assert pipeline.calls_many == {'resident': 0, 'composed': 1} and pipeline.calls == {'resident': 2, 'composed': 0}
    x64 = short_wave(fs).astype(numpy.float64)
    x64[100] += 2.0 ** -40
    for waves in (mixed, [Wave(x64, fs)]):
        for g, w in zip(bank.convert_waves(waves), waves):
            assert P.same(g.wave, lone[0].convert_wave(w).wave)
    assert pipeline.calls_many == {'resident': 0, 'composed': 3}
    bank.close()
    for p in lone:
        p.close()
    P.close_voice_changer(vc)
