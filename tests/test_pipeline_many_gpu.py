"""The many-waves wave-to-wave chain on the MI355X, bit for bit against the shipped single-wave calls in the same process: `ry_gather_rows` against
numpy, the gate over many waves against `ry_vc_gate`, `ry_analysis_extract_many_resident` against `extract_resident`, `ry_vc_enqueue_waves_device`
against `ry_vc_enqueue_wave_device`, `PipelineBank` against lone `Pipeline`s.  `tiny` CREPE capacity, SYN-8 predictors, waves of 0.25 s and shorter.
Cases: tests/pipeline_many_cases.py."""
import itertools

import numpy
import pytest

import pipeline_cases as P
import pipeline_many_cases as M
from realtime_yukarin_amd import pipeline

pytestmark = pytest.mark.gpu
SEEDS = [3, 4, 5]


@pytest.fixture(scope='module')
def changers(gpu_ctx, tmp_path_factory):
    out = {fs: P.voice_changer(P.write_models(tmp_path_factory.mktemp('models%d' % fs), fs), fs) for fs in P.RATES}
    yield out
    for vc in out.values():
        P.close_voice_changer(vc)


@pytest.fixture
def core(changers):
    c = changers[16000]._fused_core()
    yield c
    c.set_discard(0, 0)


def test_gather_rows_equals_numpy(gpu_ctx):
    M.check_gather_rows(gpu_ctx)


def test_gather_rows_refusals(gpu_ctx):
    M.check_gather_rows_refusals(gpu_ctx)


@pytest.mark.parametrize('fs', P.RATES)
@pytest.mark.parametrize('fft', [1024, 128])
def test_gate_over_three_lengths_in_every_order(gpu_ctx, core, fs, fft):
    waves, frames, hop = M.gate_lengths(fs)
    singles = None
    for order in itertools.permutations(range(3)):
        singles = M.check_gate_waves(gpu_ctx, core, waves, frames, hop, fft=fft, order=order, singles=singles)


def test_gate_over_the_kinds(gpu_ctx, core):
    fs = 24000
    waves = [P.wave_of(kind, fs) for kind in P.KINDS]
    masks = [P.check_split(kind, x, fs) for kind, x in zip(P.KINDS, waves)]
    feats, want = M.check_gate_waves(gpu_ctx, core, waves, [len(m) for m in masks], fs * P.FRAME_PERIOD // 1000)
    for (m, _, _), host in zip(want, masks):
        assert numpy.array_equal(m, host)


def test_a_quiet_wave_does_not_inherit_all_frames_from_a_loud_neighbour(gpu_ctx, core):
    fs = 16000
    waves, frames, thr = M.loud_and_quiet(fs)
    for order in ((0, 1), (1, 0)):
        feats, want = M.check_gate_waves(gpu_ctx, core, waves, frames, fs * P.FRAME_PERIOD // 1000, thr=thr, order=order)
    assert want[0][0].all() and not want[1][0].all()


def test_gate_on_poisoned_blocks(gpu_ctx, core, monkeypatch):
    """RY_POISON=1: the blocks of the gate hold NaN patterns before every call."""
    monkeypatch.setenv('RY_POISON', '1')
    gpu_ctx.reload_env()
    try:
        waves, frames, hop = M.gate_lengths(16000)
        M.check_gate_waves(gpu_ctx, core, waves, frames, hop)
    finally:
        monkeypatch.delenv('RY_POISON')
        gpu_ctx.reload_env()


def test_gate_waves_refusals(gpu_ctx, core):
    M.check_gate_waves_refusals(gpu_ctx, core)


@pytest.mark.parametrize('fs', P.RATES)
def test_extract_many_resident_equals_extract_resident(gpu_ctx, fs):
    M.check_extract_many_resident(gpu_ctx, fs)


def windows(ctx, core, fs, count):
    """0.25 s windows of the kinds of `pipeline_cases.KINDS` (an all-silent one among them), then shorter loud ones."""
    hop = fs * P.FRAME_PERIOD // 1000
    waves = [P.wave_of(P.KINDS[s % 4], fs, 0.25 if s < 4 else 0.05 + 0.01 * s, seed=s) for s in range(count)]
    return M.Windows(ctx, core, waves, [x.size // hop + 1 for x in waves], hop)


@pytest.mark.parametrize('lanes', [1, 2])
def test_enqueue_waves_device_equals_the_single_call(gpu_ctx, changers, lanes):
    """Seven windows on a ring of six -- loud, gaps, all silent -- with and without a discard hint, in two orders, on one lane and on two."""
    core = changers[24000]._fused_core()
    before = core.lanes
    core.set_lanes(lanes)
    try:
        w = windows(gpu_ctx, core, 24000, 7)
        assert w.single((0, 0))[2][3] == 0 and core.ring == 6
        w.check()
        w.check(order=(6, 2, 0, 5, 1, 4, 3))
        w.check(discard=(10, 10))
    finally:
        core.set_discard(0, 0)
        core.set_lanes(before)


def test_enqueue_waves_device_on_poisoned_predictors(gpu_ctx, monkeypatch, tmp_path):
    monkeypatch.setenv('RY_POISON', '1')
    gpu_ctx.reload_env()
    try:
        fresh = P.voice_changer(P.write_models(tmp_path, 16000), 16000)
        w = windows(gpu_ctx, fresh._fused_core(), 16000, 4)
        w.check()
        P.close_voice_changer(fresh)
    finally:
        monkeypatch.delenv('RY_POISON')
        gpu_ctx.reload_env()


def test_enqueue_waves_device_refusals(gpu_ctx, core):
    M.check_enqueue_waves_refusals(gpu_ctx, core)


@pytest.fixture(params=['f32', 'bf16x3'])
def process(request, gpu_ctx, monkeypatch, tmp_path):
    shim = P.set_up(monkeypatch, tmp_path, 'tiny', request.param)
    monkeypatch.setattr(pipeline, 'calls_many', {'resident': 0, 'composed': 0})
    yield request.param
    P.close_shim(shim)


def make(vc, n):
    param = vc.acoustic_converter.config.dataset.acoustic_param
    bank = pipeline.PipelineBank(vc, param, n, seeds=SEEDS[:n], crepe_capacity='tiny')
    return bank, [pipeline.Pipeline(vc, param, crepe_capacity='tiny', seed=s) for s in SEEDS[:n]]


def close(bank, lone, vc):
    vc._fused_core().set_discard(0, 0)
    bank.close()
    for p in lone:
        p.close()


@pytest.mark.parametrize('fs', P.RATES)
def test_convert_waves_equals_convert_wave(process, changers, fs):
    """Mixed kinds and lengths in one call, each wave against `Pipeline.convert_wave` on it alone."""
    from yukarin import Wave
    vc = changers[fs]
    bank, lone = make(vc, 1)
    waves = [Wave(P.wave_of(kind, fs, seconds, seed=s), fs) for s, (kind, seconds) in
             enumerate((('loud', 0.25), ('gap', 0.25), ('zeros', 0.1), ('gap_silent_ends', 0.25), ('loud', P.FRAME_PERIOD / 1000)))]
    got = bank.convert_waves(waves)
    assert pipeline.calls_many == {'resident': 1, 'composed': 0}
    for g, w in zip(got, waves):
        assert P.same(g.wave, lone[0].convert_wave(w).wave)
    close(bank, lone, vc)


@pytest.mark.parametrize('fs', P.RATES)
def test_push_rounds_equal_lone_pipelines(process, changers, fs):
    """Three rounds with discard = (10, 10) and a flush over three streams with distinct seeds: one sits the second round out, one ends in the
    second round and restarts in the third, one is all silent."""
    vc = changers[fs]
    bank, lone = make(vc, 3)
    M.check_bank_against_lone_pipelines(bank, lone, M.bank_rounds(fs, 0.25, ('gap', 'loud', 'zeros')), (10, 10))
    assert pipeline.calls_many == {'resident': 3, 'composed': 0}
    close(bank, lone, vc)


def test_push_on_poisoned_blocks(process, changers):
    """Tracker, analyzer, stream bank and the bank's own blocks poisoned before a call: what a call reads it has written."""
    from realtime_yukarin_amd import world_analysis
    from realtime_yukarin_amd.compat import crepe as shim
    fs = 24000
    vc = changers[fs]
    bank, lone = make(vc, 3)
    rounds = M.bank_rounds(fs, 0.25, ('gap', 'loud', 'zeros'))
    bank.push(rounds[0][0], discard=(10, 10))                              # the handles and the blocks exist
    bank.flush()
    param = bank.acoustic_param
    shim._model('tiny').poison()
    world_analysis._analyzer(fs, 1024, param.order, float(param.alpha)).poison()
    bank.bank.poison()
    for k, p in bank._blocks.items():
        if not k.startswith('w_'):
            words = (bank._cap // 4 + 4) if k == 'mask' else bank._cap * bank._blocks['w_' + k]
            bank._ctx.dev_upload(p, numpy.full(words, 0xFFFFFFFF, numpy.uint32))
    bank._table = None                                                     # the index table is lost with its block: the next push uploads it again
    M.check_bank_against_lone_pipelines(bank, lone, rounds, (10, 10))
    close(bank, lone, vc)


def test_the_composed_route_runs_through_the_bank(process, changers):
    """A float64 wave that does not round-trip through float32, then a list of mixed rates: the chain of the separate calls per stream over the
    same bank, the same bits, counted in `calls_many`."""
    from yukarin import Wave
    fs = 24000
    vc = changers[fs]
    bank, lone = make(vc, 2)
    x64 = P.wave_of('gap', fs, 0.1).astype(numpy.float64)
    x64[100] += 2.0 ** -40
    assert not numpy.array_equal(x64.astype(numpy.float32).astype(numpy.float64), x64)
    rounds = [([Wave(x64, fs), Wave(P.wave_of('loud', fs, 0.1, seed=1), fs)], ()), ([Wave(P.wave_of('loud', fs, 0.1, seed=2), fs), None], (0,))]
    M.check_bank_against_lone_pipelines(bank, lone, rounds, (3, 3))
    assert pipeline.calls_many == {'resident': 1, 'composed': 1}
    close(bank, lone, vc)


def test_mixed_rates_run_the_composed_route_through_the_bank(process, changers):
    """A 24 kHz and a 16 kHz wave in one call: the bank takes the chain of the separate calls for both, the lone pipelines stay on their resident
    paths, each at its wave's rate -- the same bits, in `push` (two rounds and the flush) and in `convert_waves`."""
    from yukarin import Wave
    vc = changers[24000]
    bank, lone = make(vc, 2)
    mk = lambda seed: [Wave(P.wave_of('gap', 24000, 0.1, seed=seed), 24000), Wave(P.wave_of('loud', 16000, 0.1, seed=seed + 1), 16000)]
    before = dict(pipeline.calls)
    M.check_bank_against_lone_pipelines(bank, lone, [(mk(0), ()), (mk(2), (1,))], (3, 3))
    assert pipeline.calls_many == {'resident': 0, 'composed': 2}
    assert pipeline.calls['resident'] - before['resident'] == 4 and pipeline.calls['composed'] == before['composed']     # the lone calls: resident
    x64 = P.wave_of('gap', 24000, 0.1).astype(numpy.float64)
    x64[100] += 2.0 ** -40
    for waves in (mk(4), [Wave(x64, 24000), Wave(P.wave_of('loud', 24000, 0.05, seed=6), 24000)]):
        got = bank.convert_waves(waves)
        for g, w in zip(got, waves):
            want = lone[0].convert_wave(w)
            assert g.sampling_rate == want.sampling_rate and P.same(g.wave, want.wave)
    assert pipeline.calls_many == {'resident': 0, 'composed': 4}
    close(bank, lone, vc)
