"""The bank of streaming trackers without a GPU: `CrepeStreamBank` on the host-side SIMT emulator against `CrepeModel.track` / `predict` of every
window on a separate handle of the same weights, bit for bit, with every wave's count of computed frames held to the restated rule's (an
implementation that recomputes everything fails, and so does one that keeps too much).  Multiplier 1, `f32`; windows of 41 frames where the issue
names them (16 kHz and 24 kHz, hop 80), of 21 and 16 frames elsewhere.  The emulator runs the network at about twelve frames a second, so what
runs here is the reduced form of the GPU file's cases (test_crepe_bank_gpu.py): at 24 kHz two calls of two streams instead of three of three; the lone `CrepeStream`
beside every stream, `signed_zero`, the banks that may keep nothing (fractional advance, advance off the hop, 44.1 kHz), `bf16x3` and the packed list that crosses a pass of 256 are there only.
`PipelineBank.push(advance=a)` runs here as one reduced pair of pushes over two streams.
Cases: tests/crepe_bank_cases.py; the rule: tests/crepe_stream_cases.py."""
import numpy
import pytest

import crepe_bank_cases as B
import crepe_stream_cases as S
import pipeline_cases as P
from realtime_yukarin_amd import crepe, engine, pipeline, world_analysis, world_synth


@pytest.fixture(scope='module')
def ref(emu_ctx):
    r = S.Reference(emu_ctx, 1)
    yield r
    r.close()


def test_three_streams_of_different_lengths_and_advances(emu_ctx, ref):
    log = B.run_plan(emu_ctx, ref, 16000, 80, 5, B.three_streams(16000, small=True))
    assert [c[0] for c in log] == [(41, 41), (24, 41), (24, 41)]
    assert all(B.keeps_after_the_first(log, s) for s in range(3)), log


def test_two_calls_at_24_khz(emu_ctx, ref):
    w = [s[:2] for s in B.three_streams(24000, small=True)[:2]]
    log = B.run_plan(emu_ctx, ref, 24000, 80, 5, w)
    assert log[0][0] == (41, 41) and all(B.keeps_after_the_first(log, s) for s in range(2)), log


def test_a_stream_that_sits_out_keeps_its_rows_whatever_the_order_of_the_others(emu_ctx, ref):
    """Stream 1 sits the second call out and returns with an advance that spans both buffers; the order of the waves changes from call to call;
    everything of the bank and of the model is poisoned between the calls."""
    log = B.run_plan(emu_ctx, ref, 16000, 160, 10, B.sit_out_streams(), poison=True, sit_out={(1, 1)}, orders=[(2, 0, 1), (0, 2), (1, 2, 0)])
    assert 1 not in log[1] and log[2][1][0] < log[2][1][1] and log[0][1] == (16, 16), log
    assert B.keeps_after_the_first(log, 0) and B.keeps_after_the_first(log, 2), log


def test_one_bad_overlap_among_good_ones(emu_ctx, ref):
    log = B.run_named(emu_ctx, ref, ['small_16k', 'flipped_bit', 'other_signal'])
    assert log[1][1] == (16, 16) and log[2][1][0] < 16, log             # the flipped bit: every frame; the window after it keeps rows again
    assert B.keeps_after_the_first(log, 0) and B.keeps_after_the_first(log, 2), log


def test_assemble_many_alone(emu_ctx):
    B.check_assemble_many(emu_ctx)


def test_state(emu_ctx, ref):
    """Calls on the model between two bank calls, a refused call of every kind, `reset` of one stream, a dtype switch, and tables that go up only
    when they change."""
    case = S.SEQUENCES['small_16k']
    w, v = case['windows'](), S.SEQUENCES['other_signal']['windows']()
    args = (case['sr'], case['hop'], case['step'])
    b = B.Bank(emu_ctx, ref, 2)
    other = S.signal(16000, 1500, seed=9)
    b.call(*args, [w[0][0], v[0][0]], [None, None])
    b.model.predict(other, 16000, 160)
    b.model.track(other, 16000, 160, 10)
    b.model.track_many([other[:900], other[:1100]], 16000, 160, 10)
    b.model.poison()
    B.check_refusals(b, *args, w[1][0], v[1][0])
    out = b.call(*args, [w[1][0], v[1][0]], [w[1][1], v[1][1]])
    assert out[0][0] < 16 and out[1][0] < 16, out
    # steady state: the third call's tables are new (every stream has swapped its slots), the fourth's are those of the second, the fifth's of the third
    n = b.bank.uploads()
    for k in range(3):
        out = b.call(*args, [w[1][0], v[1][0]], [0, 0])
        assert out[0][0] < 16, out
    assert b.bank.uploads() == n + 2
    b.bank.reset(1)
    b.rules[1].reset()
    out = b.call(*args, [w[2][0], v[2][0]], [w[2][1], v[2][1]])
    assert out[0][0] < 16 and out[1] == (16, 16), out
    b.model.set_dtype('bf16x3')
    out = b.call(*args, [w[2][0], v[2][0]], [0, 0], dtype='bf16x3')
    assert out[0] == (16, 16) and out[1] == (16, 16), out
    b.close()


def test_the_activation_of_a_stream_without_a_window_is_refused(emu_ctx):
    from realtime_yukarin_amd import _lib
    model = S.new_model(emu_ctx, 1)
    bank = crepe.CrepeStreamBank(model, 2)
    lib, h = bank._get()
    out = numpy.zeros(S.BINS, numpy.float32)
    assert lib.dll.ry_crepe_bank_activation(h, 0, _lib._fptr(out), 0) == -4
    assert lib.dll.ry_crepe_bank_activation(h, 2, _lib._fptr(out), 0) == -1
    assert lib.dll.ry_crepe_bank_activation(h, 0, _lib._fptr(None), 0) == -1
    assert lib.dll.ry_crepe_bank_reset(h, 2) == -1 and lib.dll.ry_crepe_bank_reset(h, -2) == -1 and lib.dll.ry_crepe_bank_reset(h, -1) == 0
    assert bank.poison() == [0, 0]
    bank.close()
    bank.close()
    model.close()


# ---- PipelineBank.push(..., advance=a) --------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_emulator(emu_ctx, monkeypatch):
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: emu_ctx)
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    return emu_ctx


def test_bank_push_with_an_advance_returns_the_samples_of_push_without(on_emulator, monkeypatch, tmp_path):
    """Two streams, two pushes and the flush at 24 kHz, with and without `advance`: the same samples, fewer frames through the network in the
    second push."""
    from yukarin import Wave
    fs = 24000
    shim = P.set_up(monkeypatch, tmp_path, 1, 'f32')
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    param = vc.acoustic_converter.config.dataset.acoustic_param
    n, a = fs // 10, fs // 100                                         # 0.1 s windows (21 frames) advancing 10 ms
    sigs = [P.wave_of('loud', fs, 0.2, seed) for seed in (1, 2)]
    got = {}
    for advance in (None, a):
        bank = pipeline.PipelineBank(vc, param, 2, seeds=[3, 4], crepe_capacity=1)
        out = []
        for k in range(2):
            out.append([w.wave for w in bank.push([Wave(x[k * a:k * a + n], fs) for x in sigs], discard=(2, 2), advance=advance)])
            if advance is not None:
                t = bank._crepe_bank
                assert t.frames == [21, 21] and (t.computed == [21, 21] if k == 0 else all(0 < c < 21 for c in t.computed)), (k, t.computed)
        got[advance] = out + [[w.wave for w in bank.flush()]]
        if advance is not None:
            assert bank._crepe_bank._prev == [None, None]                  # the flush dropped the kept rows
        bank.close()
    assert all(P.same(g, w) for gs, ws in zip(got[a], got[None]) for g, w in zip(gs, ws)) and sum(len(w) for ws in got[None] for w in ws) > 0
    P.close_voice_changer(vc)
    P.close_shim(shim)
