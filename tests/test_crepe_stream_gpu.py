"""The streaming tracker on the MI355X: `CrepeStream` against `CrepeModel.track` / `predict` of every window on a separate handle of the same
weights, bit for bit, with the number of frames that went through the network held to the restated rule's count; `Pipeline.push(..., advance=a)`
against the same pushes without.  Multiplier 4 (`tiny`); the 601-frame sequence at multiplier 1 (three passes on the first push, a packed list that
crosses a pass of 256 on the later ones) and one push pair at multiplier 32.  Cases and the rule: tests/crepe_stream_cases.py."""
import ctypes

import numpy
import pytest

import crepe_stream_cases as S
import pipeline_cases as P
from realtime_yukarin_amd import _lib, crepe, pipeline

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ref(gpu_ctx):
    r = S.Reference(gpu_ctx, 4)
    yield r
    r.close()


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
@pytest.mark.parametrize('name', ['16k_3200_800', '24k_4800_1200', '48k', 'advance_0', 'fractional_advance', 'advance_off_the_hop',
                                  'advance_past_the_window', '44k1', 'grow_and_shrink', 'grow_and_shrink_24k', 'shorter_than_a_frame', 'small_16k',
                                  'small_24k'])
def test_sequence(gpu_ctx, ref, name, dtype):
    out = S.run_sequence(gpu_ctx, ref, name, dtype=dtype, poison=True)
    if name == '16k_3200_800':
        assert out == [(41, 41), (24, 41), (24, 41)]
    if name == 'advance_0':
        assert out[1] == out[2] == (8, 16)


@pytest.mark.parametrize('name', ['flipped_bit', 'signed_zero'])
def test_an_overlap_that_differs_in_one_word_is_computed_in_full(gpu_ctx, ref, name):
    out = S.run_sequence(gpu_ctx, ref, name)
    assert out[1][0] == out[1][1] and out[2][0] < out[2][1], out


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
def test_601_frames_cross_the_passes(gpu_ctx, dtype):
    r = S.Reference(gpu_ctx, 1)
    try:
        out = S.run_sequence(gpu_ctx, r, '601_frames', dtype=dtype, poison=True)
    finally:
        r.close()
    assert out == [(601, 601), (294, 601), (294, 601)]


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
def test_a_push_pair_at_full_capacity(gpu_ctx, dtype):
    r = S.Reference(gpu_ctx, 32)
    try:
        out = S.run_sequence(gpu_ctx, r, 'pair', dtype=dtype)
    finally:
        r.close()
    assert out[1][0] < out[1][1] == 41


def test_a_dtype_switch_between_pushes_computes_every_frame(gpu_ctx, ref):
    case = S.SEQUENCES['small_24k']
    w = case['windows']()
    model = S.new_model(gpu_ctx, 4)
    stream, rule = crepe.CrepeStream(model), S.Rule()
    args = (case['sr'], case['hop'], case['step'])
    S.check_push(stream, rule, ref, w[0][0], *args, None, 'f32')
    model.set_dtype('bf16x3')
    assert S.check_push(stream, rule, ref, w[1][0], *args, w[1][1], 'bf16x3') == (16, 16)
    c, n = S.check_push(stream, rule, ref, w[2][0], *args, w[2][1], 'bf16x3')
    assert c < n
    model.set_dtype('f32')
    assert S.check_push(stream, rule, ref, w[2][0], *args, 0, 'f32') == (16, 16)
    stream.close()
    model.close()


def test_calls_on_the_model_between_pushes_leave_the_kept_rows_alone(gpu_ctx, ref):
    """`predict`, `track_many` and `ry_crepe_debug_poison` on the model between two pushes, a longer call included (the model's buffers grow)."""
    case = S.SEQUENCES['24k_4800_1200']
    w = case['windows']()
    args = (case['sr'], case['hop'], case['step'])
    model = S.new_model(gpu_ctx, 4)
    stream, rule = crepe.CrepeStream(model), S.Rule()
    other = S.signal(16000, 30000, seed=9)
    S.check_push(stream, rule, ref, w[0][0], *args, None)
    model.predict(other, 16000, 80)
    model.track_many([other[:900], w[0][0][:1100]], 24000, 80, 5)
    model.poison()
    c, n = S.check_push(stream, rule, ref, w[1][0], *args, w[1][1])
    assert c < n
    model.poison()
    c, n = S.check_push(stream, rule, ref, w[2][0], *args, w[2][1], poison=True)
    assert c < n
    stream.close()
    model.close()


def test_two_streams_on_one_model_pushed_alternately(gpu_ctx, ref):
    a, b = S.SEQUENCES['small_16k'], S.SEQUENCES['other_signal']
    model = S.new_model(gpu_ctx, 4)
    streams, rules = [crepe.CrepeStream(model), crepe.CrepeStream(model)], [S.Rule(), S.Rule()]
    for (xa, aa), (xb, ab) in zip(a['windows'](), b['windows']()):
        ca = S.check_push(streams[0], rules[0], ref, xa, a['sr'], a['hop'], a['step'], aa, poison=True)
        cb = S.check_push(streams[1], rules[1], ref, xb, b['sr'], b['hop'], b['step'], ab, poison=True)
        assert ca == cb and (aa is None or ca[0] < ca[1])
    for s in streams:
        s.close()
    model.close()


def test_reset_makes_a_stream_a_fresh_one(gpu_ctx, ref):
    a, b = S.SEQUENCES['small_16k'], S.SEQUENCES['other_signal']
    model = S.new_model(gpu_ctx, 4)
    stream, rule = crepe.CrepeStream(model), S.Rule()
    for case in (a, b, a):
        w = case['windows']()
        stream.reset()
        rule.reset()
        assert S.check_push(stream, rule, ref, w[0][0], case['sr'], case['hop'], case['step'], 480) == (16, 16)
        c, n = S.check_push(stream, rule, ref, w[1][0], case['sr'], case['hop'], case['step'], w[1][1])
        assert c < n
    stream.close()
    model.close()


def test_a_refused_call_between_two_pushes(gpu_ctx, ref):
    case = S.SEQUENCES['small_16k']
    w = case['windows']()
    args = (case['sr'], case['hop'], case['step'])
    model = S.new_model(gpu_ctx, 4)
    stream, rule = crepe.CrepeStream(model), S.Rule()
    S.check_push(stream, rule, ref, w[0][0], *args, None)
    lib, h = stream._get()
    x = w[1][0]
    voiced, f0, t = numpy.full(64, 0xA5, numpy.uint8), numpy.full(64, -7.0), numpy.full(64, -7.0)
    nf, nc = ctypes.c_int(-3), ctypes.c_int(-3)
    UB, DP = ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_double)
    tail = (ctypes.byref(nf), ctypes.byref(nc), voiced.ctypes.data_as(UB), f0.ctypes.data_as(DP), t.ctypes.data_as(DP), 0)
    f = lib.dll.ry_crepe_stream_track
    assert f(h, _lib._fptr(x), 0, 16000, 160, 10.0, 0.1, 480, 1, *tail) == -1                           # no sample
    assert f(h, _lib._fptr(x), x.size, 22050, 160, 10.0, 0.1, 480, 1, *tail) == -4                      # a rate without tables
    assert (nf.value, nc.value) == (-3, -3) and (voiced == 0xA5).all() and (f0 == -7.0).all() and (t == -7.0).all()
    c, n = S.check_push(stream, rule, ref, x, *args, w[1][1], poison=True)
    assert c < n
    stream.close()
    model.close()


def test_assemble_alone(gpu_ctx):
    S.check_assemble(gpu_ctx)


# ---- Pipeline.push(..., advance=a) ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def changers(gpu_ctx, tmp_path_factory):
    out = {fs: P.voice_changer(P.write_models(tmp_path_factory.mktemp('models%d' % fs), fs), fs) for fs in P.RATES}
    yield out
    for vc in out.values():
        P.close_voice_changer(vc)


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
@pytest.mark.parametrize('fs', P.RATES)
def test_push_with_an_advance_returns_the_samples_of_push_without(gpu_ctx, changers, monkeypatch, tmp_path, fs, dtype):
    """Three pushes and the flush, with and without `advance`: the same samples, the same count of calls.  The first window starts with zero
    padding that the second holds audio for -- the shape `BaseStream.fetch` produces at a stream's start -- so the second push finds an overlap
    that does not match and computes every frame; the third keeps rows."""
    from yukarin import Wave
    shim = P.set_up(monkeypatch, tmp_path, 'tiny', dtype)
    vc = changers[fs]
    param = vc.acoustic_converter.config.dataset.acoustic_param
    n, a = fs // 4, fs // 20                                           # 0.25 s windows (51 frames) advancing 50 ms
    sig = P.wave_of('loud', fs, 0.4, 1)
    first = sig[:n].copy()
    first[:2 * a] = 0                                                  # audio that had not arrived yet
    windows = [first, sig[a:a + n], sig[2 * a:2 * a + n]]
    got = {}
    for advance in (None, a):
        pipe = pipeline.Pipeline(vc, param, crepe_capacity='tiny', seed=3)
        before = dict(pipeline.calls)
        out = []
        for k, w in enumerate(windows):
            out.append(pipe.push(Wave(w, fs), discard=(10, 10), advance=advance).wave)
            if advance is not None:
                s = pipe._crepe_stream
                assert s.frames == 51 and (s.computed == 51 if k < 2 else 0 < s.computed < 51), (k, s.computed)
        got[advance] = out + [pipe.flush().wave]
        assert pipeline.calls['resident'] - before['resident'] == 3 and pipeline.calls['composed'] == before['composed']
        if advance is not None:
            assert pipe._crepe_stream._prev is None                    # the flush dropped the kept rows
        pipe.close()
    assert all(P.same(g, w) for g, w in zip(got[a], got[None])) and sum(len(w) for w in got[None]) > 0
    vc._fused_core().set_discard(0, 0)
    P.close_shim(shim)
