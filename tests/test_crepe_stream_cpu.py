"""The streaming tracker without a GPU: the rule on the host resampler alone, then `CrepeStream` on the host-side SIMT emulator against
`CrepeModel.track` / `predict` of every window on a separate handle of the same weights, bit for bit, with the number of frames that went through the
network held to the restated rule's count (an implementation that always recomputes fails).  Multiplier 1; windows of 16 frames except where the
shape is the point (41 frames at 16 and 24 kHz).  The 601-frame sequence, whose packed list crosses a pass of 256, runs on the GPU only
(test_crepe_stream_gpu.py): the emulator runs the network at about twelve frames a second, and the sequence and its reference have 3000.
Cases and the rule: tests/crepe_stream_cases.py."""
import ctypes

import numpy
import pytest

import crepe_stream_cases as S
import pipeline_cases as P
from realtime_yukarin_amd import _lib, crepe, engine, pipeline, world_analysis, world_synth


# ---- the rule itself: no device code --------------------------------------------------------------------------------------------------------
def test_a_clean_output_has_the_bits_of_the_shifted_signal_and_a_cut_one_does_not():
    """24 kHz, y = x[1200:]: resample(y)[t] has the bits of resample(x)[t + 800] at every t the rule calls clean in both, and differs at some t
    the rule calls not clean at the head of y -- the margin is needed, not merely generous."""
    rng = numpy.random.default_rng(5)
    x = rng.normal(0, 0.3, 6000).astype(numpy.float32)
    a, a16 = 1200, 800
    y = x[a:]
    rx, ry = crepe.resample(x, 24000), crepe.resample(y, 24000)
    cx, cy = S.clean_outputs(24000, x.size), S.clean_outputs(24000, y.size)
    assert rx.size == cx.size == 4000 and ry.size == cy.size == 3200
    assert S.register_repeats(24000, a, a16, ry.size)
    both = cy & cx[a16:a16 + ry.size]
    assert 2000 < both.sum() < ry.size
    assert numpy.array_equal(S.bits(ry[both]), S.bits(rx[a16:a16 + ry.size][both]))
    head = numpy.flatnonzero(~cy)
    head = head[head < ry.size // 2]
    assert head.size and (S.bits(ry[head]) != S.bits(rx[a16 + head])).any()
    assert not cy[0] and not cx[0] and cx[a16] and cy[ry.size // 2]


def test_the_register_repeats_at_24_and_48_khz_and_drifts_at_44k1():
    assert S.register_repeats(24000, 1200, 800, 3200) and S.register_repeats(48000, 2400, 800, 3200)
    assert not S.register_repeats(44100, 1323, 480, 1920)           # the sequential sum of 2.75625 rounds: no reuse, whatever the rate is called


def test_the_edges_of_the_reference_window():
    """16 kHz, hop 80, 3200 samples: 41 frames, 7 edge frames each side; advancing 800 keeps 17 and computes 24."""
    p = S.portable_frames(16000, 3200, 80)
    assert p.size == 41 and not p[:7].any() and p[7:34].all() and not p[34:].any()
    rule = S.Rule()
    x = S.signal(16000, 4000)
    assert rule.push(x[:3200], 16000, 80, None)[1] == 41
    src, computed = rule.push(x[800:], 16000, 80, 800)
    assert computed == 24 and list(numpy.flatnonzero(src >= 0)) == list(range(7, 24)) and list(src[7:24]) == list(range(17, 34))


# ---- the stream on the emulator -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ref(emu_ctx):
    r = S.Reference(emu_ctx, 1)
    yield r
    r.close()


@pytest.mark.parametrize('name', ['16k_3200_800', '24k_4800_1200', '48k', 'advance_0', 'fractional_advance', 'advance_off_the_hop',
                                  'advance_past_the_window', '44k1', 'grow_and_shrink', 'shorter_than_a_frame'])
def test_sequence(emu_ctx, ref, name):
    out = S.run_sequence(emu_ctx, ref, name)
    if name == '16k_3200_800':
        assert out == [(41, 41), (24, 41), (24, 41)]
    if name == 'advance_0':
        assert out[1] == out[2] == (8, 16)                             # the edge frames alone


@pytest.mark.parametrize('name', ['flipped_bit', 'signed_zero'])
def test_an_overlap_that_differs_in_one_word_is_computed_in_full(emu_ctx, ref, name):
    out = S.run_sequence(emu_ctx, ref, name)
    assert out[1][0] == out[1][1] and out[2][0] < out[2][1], out


@pytest.mark.parametrize('name', ['small_16k', 'small_24k'])
def test_bf16x3_throughout(emu_ctx, ref, name):
    S.run_sequence(emu_ctx, ref, name, dtype='bf16x3')


def test_a_dtype_switch_between_pushes_computes_every_frame(emu_ctx, ref):
    case = S.SEQUENCES['small_16k']
    w = case['windows']()
    model = S.new_model(emu_ctx, 1)
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


def test_calls_on_the_model_between_pushes_leave_the_kept_rows_alone(emu_ctx, ref):
    """`predict`, `track_many` and `ry_crepe_debug_poison` on the model between two pushes."""
    case = S.SEQUENCES['small_24k']
    w = case['windows']()
    args = (case['sr'], case['hop'], case['step'])
    model = S.new_model(emu_ctx, 1)
    stream, rule = crepe.CrepeStream(model), S.Rule()
    other = S.signal(16000, 1500, seed=9)
    S.check_push(stream, rule, ref, w[0][0], *args, None)
    model.predict(other, 16000, 160)
    model.track_many([other[:900], w[0][0][:1100]], 24000, 160, 10)
    model.poison()
    c, n = S.check_push(stream, rule, ref, w[1][0], *args, w[1][1])
    assert c < n
    model.poison()
    c, n = S.check_push(stream, rule, ref, w[2][0], *args, w[2][1], poison=True)
    assert c < n
    stream.close()
    model.close()


def test_two_streams_on_one_model_pushed_alternately(emu_ctx, ref):
    a, b = S.SEQUENCES['small_16k'], S.SEQUENCES['other_signal']
    model = S.new_model(emu_ctx, 1)
    streams, rules = [crepe.CrepeStream(model), crepe.CrepeStream(model)], [S.Rule(), S.Rule()]
    for (xa, aa), (xb, ab) in zip(a['windows'](), b['windows']()):
        assert not S.same(xa, xb)
        ca = S.check_push(streams[0], rules[0], ref, xa, a['sr'], a['hop'], a['step'], aa)
        cb = S.check_push(streams[1], rules[1], ref, xb, b['sr'], b['hop'], b['step'], ab)
        assert ca == cb and (aa is None or ca[0] < ca[1])
    for s in streams:
        s.close()
    model.close()


def test_reset_makes_a_stream_a_fresh_one(emu_ctx, ref):
    """A, B, A on one stream with `reset` before each change of signal: every push equals that of a fresh stream, and computes every frame."""
    a, b = S.SEQUENCES['small_16k'], S.SEQUENCES['other_signal']
    model = S.new_model(emu_ctx, 1)
    stream, rule = crepe.CrepeStream(model), S.Rule()
    for case in (a, b, a):
        w = case['windows']()
        stream.reset()
        rule.reset()
        # the advance is declared although the stream was reset: nothing is kept
        assert S.check_push(stream, rule, ref, w[0][0], case['sr'], case['hop'], case['step'], 480) == (16, 16)
        c, n = S.check_push(stream, rule, ref, w[1][0], case['sr'], case['hop'], case['step'], w[1][1])
        assert c < n
    stream.close()
    model.close()


def test_poison_before_every_push(emu_ctx, ref):
    for name in ('small_24k', 'grow_and_shrink'):
        S.run_sequence(emu_ctx, ref, name, poison=True)


def test_a_refused_call_between_two_pushes(emu_ctx, ref):
    """No sample, a rate without tables, a null count: refused by return code, guard-filled outputs untouched, and the next push keeps its rows."""
    case = S.SEQUENCES['small_16k']
    w = case['windows']()
    args = (case['sr'], case['hop'], case['step'])
    model = S.new_model(emu_ctx, 1)
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
    assert f(h, _lib._fptr(x), x.size, 16000, 0, 10.0, 0.1, 480, 1, *tail) == -1
    assert f(h, _lib._fptr(x), x.size, 16000, 160, 0.0, 0.1, 480, 1, *tail) == -1
    assert f(h, _lib._fptr(None), x.size, 16000, 160, 10.0, 0.1, 480, 1, *tail) == -1
    assert f(h, _lib._fptr(x), x.size, 16000, 160, 10.0, 0.1, 480, 1, tail[0], None, *tail[2:]) == -1
    assert f(h, _lib._fptr(x), x.size, 16000, 160, 10.0, 0.1, 480, 1, *tail[:2], None, *tail[3:]) == -1
    assert f(None, _lib._fptr(x), x.size, 16000, 160, 10.0, 0.1, 480, 1, *tail) == -4
    assert (nf.value, nc.value) == (-3, -3) and (voiced == 0xA5).all() and (f0 == -7.0).all() and (t == -7.0).all()
    c, n = S.check_push(stream, rule, ref, x, *args, w[1][1], poison=True)
    assert c < n
    stream.close()
    model.close()


def test_the_activation_of_a_stream_without_a_window_is_refused(emu_ctx):
    model = S.new_model(emu_ctx, 1)
    stream = crepe.CrepeStream(model)
    lib, h = stream._get()
    out = numpy.zeros(S.BINS, numpy.float32)
    assert lib.dll.ry_crepe_stream_activation(h, _lib._fptr(out), 0) == -4
    assert lib.dll.ry_crepe_stream_activation(h, _lib._fptr(None), 0) == -1
    assert stream.poison() == 0
    stream.close()
    stream.close()
    model.close()



def test_assemble_alone(emu_ctx):
    S.check_assemble(emu_ctx)


# ---- Pipeline.push(..., advance=a) ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_emulator(emu_ctx, monkeypatch):
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: emu_ctx)
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    return emu_ctx


@pytest.mark.parametrize('fs, dtype', [(24000, 'f32'), (16000, 'bf16x3'), (16000, 'f32'), (24000, 'bf16x3')])
def test_push_with_an_advance_returns_the_samples_of_push_without(on_emulator, monkeypatch, tmp_path, fs, dtype):
    """Three pushes and the flush, with and without `advance`: the same samples, the same count of calls.  The first window starts with zero
    padding that the second holds audio for -- the shape `BaseStream.fetch` produces at a stream's start -- so the second push finds an overlap
    that does not match and computes every frame; the third keeps rows."""
    from yukarin import Wave
    shim = P.set_up(monkeypatch, tmp_path, 1, dtype)
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    param = vc.acoustic_converter.config.dataset.acoustic_param
    n, a = fs // 10, fs // 100                                         # 0.1 s windows (21 frames) advancing 10 ms
    sig = P.wave_of('loud', fs, 0.2, 1)
    first = sig[:n].copy()
    first[:2 * a] = 0                                                  # audio that had not arrived yet
    windows = [first, sig[a:a + n], sig[2 * a:2 * a + n]]
    got = {}
    for advance in (None, a):
        pipe = pipeline.Pipeline(vc, param, crepe_capacity=1, seed=3)
        before = dict(pipeline.calls)
        out = []
        for k, w in enumerate(windows):
            out.append(pipe.push(Wave(w, fs), discard=(2, 2), advance=advance).wave)
            if advance is not None:
                s = pipe._crepe_stream
                assert s.frames == 21 and (s.computed == 21 if k < 2 else 0 < s.computed < 21), (k, s.computed)
        got[advance] = out + [pipe.flush().wave]
        assert pipeline.calls['resident'] - before['resident'] == 3 and pipeline.calls['composed'] == before['composed']
        if advance is not None:
            assert pipe._crepe_stream._prev is None                    # the flush dropped the kept rows
        pipe.close()
    assert all(P.same(g, w) for g, w in zip(got[a], got[None])) and sum(len(w) for w in got[None]) > 0
    P.close_voice_changer(vc)
    P.close_shim(shim)
