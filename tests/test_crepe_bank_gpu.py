"""The bank of streaming trackers on the MI355X: `CrepeStreamBank` against `CrepeModel.track` / `predict` of every window on a separate handle
of the same weights and against a lone `CrepeStream` per stream on the bank's own model, bit for bit, with every wave's count of computed frames
held to the restated rule's; `PipelineBank.push(..., advance=a)` against the same pushes without and against lone `Pipeline.push(advance=a)`.
Multiplier 1, except one pair of calls at multiplier 32.  Cases: tests/crepe_bank_cases.py; the rule: tests/crepe_stream_cases.py."""
import pytest

import crepe_bank_cases as B
import crepe_stream_cases as S
import pipeline_cases as P
from realtime_yukarin_amd import pipeline

pytestmark = pytest.mark.gpu
DTYPES = ['f32', 'bf16x3']


@pytest.fixture(scope='module')
def ref(gpu_ctx):
    r = S.Reference(gpu_ctx, 1)
    yield r
    r.close()


# ---- 1, 5: three streams of different lengths and advances, with and without poison between the calls -----------------------------------------
@pytest.mark.parametrize('poison', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('sr', [16000, 24000])
def test_three_streams_of_different_lengths_and_advances(gpu_ctx, ref, sr, dtype, poison):
    log = B.run_plan(gpu_ctx, ref, sr, 80, 5, B.three_streams(sr), dtype=dtype, poison=poison, lone=True)
    if sr == 16000:
        assert [c[0] for c in log] == [(41, 41), (24, 41), (24, 41)]
    assert all(B.keeps_after_the_first(log, s) for s in range(3)), log


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_pair_of_calls_at_full_capacity(gpu_ctx, dtype):
    r = S.Reference(gpu_ctx, 32)
    try:
        log = B.run_plan(gpu_ctx, r, 24000, 80, 5, [s[:2] for s in B.three_streams(24000)], dtype=dtype)
    finally:
        r.close()
    assert all(B.keeps_after_the_first(log, s) for s in range(3)), log


# ---- 2: a stream that sits out ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('orders', [None, [(2, 0, 1), (0, 2), (1, 2, 0)]])
def test_a_stream_that_sits_out_keeps_its_rows(gpu_ctx, ref, orders):
    log = B.run_plan(gpu_ctx, ref, 16000, 160, 10, B.sit_out_streams(), poison=True, lone=True, sit_out={(1, 1)}, orders=orders)
    assert 1 not in log[1] and log[2][1][0] < log[2][1][1] and log[0][1] == (16, 16), log
    assert B.keeps_after_the_first(log, 0) and B.keeps_after_the_first(log, 2), log


# ---- 3: one bad overlap among good ones; banks that may keep nothing ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['flipped_bit', 'signed_zero'])
def test_one_bad_overlap_among_good_ones(gpu_ctx, ref, name):
    log = B.run_named(gpu_ctx, ref, ['small_16k', name, 'other_signal'], lone=True)
    assert log[1][1] == (16, 16) and log[2][1][0] < 16, log
    assert B.keeps_after_the_first(log, 0) and B.keeps_after_the_first(log, 2), log


@pytest.mark.parametrize('name', ['fractional_advance', 'advance_off_the_hop', '44k1'])
def test_a_bank_that_may_keep_nothing_computes_every_frame(gpu_ctx, ref, name):
    log = B.run_named(gpu_ctx, ref, [name] * 3, lone=True)
    assert all(B.all_computed(log, s) for s in range(3)), log


# ---- 4: the packed list crosses a pass of 256 with a wave boundary inside a pass ----------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_the_packed_list_crosses_a_pass(gpu_ctx, ref, dtype):
    """12 streams of 41 frames (12 x 24 = 288 computed in steady state, 492 on the first call) and one of 601 whose own list (294) crosses a pass."""
    w = [S.slices(16000, (0, 800, 1600), (3200,) * 3, (None, 800, 800), seed=20 + s) for s in range(12)]
    w.append(S.SEQUENCES['601_frames']['windows']())
    log = B.run_plan(gpu_ctx, ref, 16000, 80, 5, w, dtype=dtype, poison=True)
    for c, first in zip(log, (True, False, False)):
        assert [c[s] for s in range(12)] == [(41 if first else 24, 41)] * 12 and c[12] == (601 if first else 294, 601), c


# ---- 6: the kernel alone ------------------------------------------------------------------------------------------------------------------------
def test_assemble_many_alone(gpu_ctx):
    B.check_assemble_many(gpu_ctx)


# ---- 7: state -----------------------------------------------------------------------------------------------------------------------------------
def test_state(gpu_ctx, ref):
    """Calls on the model between two bank calls, a refused call of every kind, tables that go up only when they change, `reset` of one stream, a
    dtype switch; the lone streams beside the bank on one model throughout."""
    case = S.SEQUENCES['small_24k']
    w, v = case['windows'](), S.slices(24000, (0, 720, 1440), (3600,) * 3, (None, 720, 720), seed=7)
    args = (case['sr'], case['hop'], case['step'])
    b = B.Bank(gpu_ctx, ref, 2, lone=True)
    other = S.signal(16000, 1500, seed=9)
    b.call(*args, [w[0][0], v[0][0]], [None, None])
    b.model.predict(other, 16000, 160)
    b.model.track(other, 16000, 160, 10)
    b.model.track_many([other[:900], w[0][0][:1100]], 24000, 160, 10)
    b.model.poison()
    B.check_refusals(b, *args, w[1][0], v[1][0])
    out = b.call(*args, [w[1][0], v[1][0]], [w[1][1], v[1][1]], poison=True)
    assert out[0][0] < 16 and out[1][0] < 16, out
    n = b.bank.uploads()
    for k in range(3):
        out = b.call(*args, [w[1][0], v[1][0]], [0, 0], device=True)
        assert out[0][0] < 16, out
    assert b.bank.uploads() == n + 2                                   # the third call of the three found its tables on the card
    b.bank.reset(1)
    b.rules[1].reset()
    b.lone[1].reset()
    out = b.call(*args, [w[2][0], v[2][0]], [w[2][1], v[2][1]])
    assert out[0][0] < 16 and out[1] == (16, 16), out
    b.model.set_dtype('bf16x3')
    out = b.call(*args, [w[2][0], v[2][0]], [0, 0], dtype='bf16x3')
    assert out[0] == (16, 16) and out[1] == (16, 16), out
    out = b.call(*args, [w[2][0], v[2][0]], [0, 0], dtype='bf16x3')
    assert out[0][0] < 16 and out[1][0] < 16, out
    b.close()


# ---- 8: PipelineBank.push(..., advance=a) -------------------------------------------------------------------------------------------------------
SEEDS = [3, 4, 5]


@pytest.fixture(scope='module')
def changers(gpu_ctx, tmp_path_factory):
    out = {fs: P.voice_changer(P.write_models(tmp_path_factory.mktemp('models%d' % fs), fs), fs) for fs in P.RATES}
    yield out
    for vc in out.values():
        P.close_voice_changer(vc)


@pytest.fixture(params=DTYPES)
def process(request, gpu_ctx, monkeypatch, tmp_path):
    shim = P.set_up(monkeypatch, tmp_path, 1, request.param)
    monkeypatch.setattr(pipeline, 'calls_many', {'resident': 0, 'composed': 0})
    yield request.param
    P.close_shim(shim)


@pytest.mark.parametrize('fs', P.RATES)
def test_bank_push_with_an_advance(process, changers, fs):
    """Four pushes over three streams ('gap', 'loud', all zeros) of 0.25 s windows advancing 50 ms, discard = (10, 10): stream 0 sits the second
    push out and returns with twice the advance, stream 1 ends with the third push and starts again in the fourth; then the flush.  Every stream's
    samples equal those of `PipelineBank.push` without `advance` and of a lone `Pipeline(seed=seeds[b]).push(advance=a)`, call by call."""
    from yukarin import Wave
    vc = changers[fs]
    param = vc.acoustic_converter.config.dataset.acoustic_param
    n, a = fs // 4, fs // 20
    sigs = [P.wave_of(kind, fs, 0.5, seed=s) for s, kind in enumerate(('gap', 'loud', 'zeros'))]
    win = lambda s, k: Wave(sigs[s][k * a:k * a + n].copy(), fs)
    #         waves per stream,                 final, advance per stream
    rounds = [([win(0, 0), win(1, 0), win(2, 0)], (), [a, a, a]),                # declared, with nothing before it: computed in full
              ([None, win(1, 1), win(2, 1)], (), [None, a, a]),
              ([win(0, 2), win(1, 2), win(2, 2)], (1,), [2 * a, a, a]),
              ([win(0, 3), win(1, 3), win(2, 3)], (), [a, a, a])]
    banks = [pipeline.PipelineBank(vc, param, 3, seeds=SEEDS, crepe_capacity=1) for _ in range(2)]
    lone = [pipeline.Pipeline(vc, param, crepe_capacity=1, seed=s) for s in SEEDS]
    for k, (waves, final, adv) in enumerate(rounds):
        got = banks[0].push(waves, discard=(10, 10), final=final, advance=adv)
        plain = banks[1].push(waves, discard=(10, 10), final=final)
        t = banks[0]._crepe_bank
        for s, wave in enumerate(waves):
            if wave is None:
                assert got[s].wave.size == 0
                continue
            want = lone[s].push(wave, discard=(10, 10), final=s in final, advance=adv[s])
            assert P.same(got[s].wave, plain[s].wave) and P.same(got[s].wave, want.wave), (k, s)
            assert (t.computed[s], t.frames[s]) == (lone[s]._crepe_stream.computed, lone[s]._crepe_stream.frames), (k, s)
            fresh = k == 0 or (k == 3 and s == 1)                          # the first push; the push after `final` named the stream
            assert t.computed[s] == t.frames[s] if fresh else 0 < t.computed[s] < t.frames[s], (k, s, t.computed, t.frames)
    assert pipeline.calls_many == {'resident': 8, 'composed': 0}
    got, plain = banks[0].flush(), banks[1].flush()
    for s in range(3):
        assert P.same(got[s].wave, plain[s].wave) and P.same(got[s].wave, lone[s].flush().wave), s
    assert banks[0]._crepe_bank._prev == [None] * 3                        # the flush dropped the kept rows
    assert sum(len(g.wave) for g in got) > 0
    vc._fused_core().set_discard(0, 0)
    for p in banks + lone:
        p.close()
