"""The resident wave-to-wave chain without a GPU, on the host-side SIMT emulator: the three new entry points (`ry_analysis_extract_resident`,
`ry_vc_enqueue_wave_device`, `ry_mask_rows`) against the host results and their refusals by return code; the waves of the GPU tests against the host
gate (they split where their names say); which path `Pipeline` takes, and that either path returns the bits of the chain of the separate calls.
20 ms waves (5 frames: the emulator runs the network at about ten frames a second).  Cases: tests/pipeline_cases.py."""
import ctypes

import numpy
import pytest

import pipeline_cases as P
from realtime_yukarin_amd import _lib, engine, pipeline, world_analysis, world_synth


@pytest.fixture
def on_emulator(emu_ctx, monkeypatch):
    """Every lazily created context of the shims and the audio units is the emulator's."""
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: emu_ctx)
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    return emu_ctx


@pytest.mark.parametrize('fs', P.RATES)
@pytest.mark.parametrize('kind', P.KINDS)
def test_the_waves_split_where_their_names_say(kind, fs):
    """The 0.25 s waves of the GPU tests on the host gate: 'loud' keeps every frame, 'zeros' none, the two 'gap' waves some, and
    'gap_silent_ends' neither the first nor the last."""
    eff = P.check_split(kind, P.wave_of(kind, fs), fs)
    assert len(eff) == 51


def test_mask_rows_equals_numpy(emu_ctx):
    P.check_mask_rows(emu_ctx)


def test_mask_rows_refusals(emu_ctx):
    dll, h = emu_ctx.lib.dll, emu_ctx.handle
    rows, mask = emu_ctx.dev_alloc(64), emu_ctx.dev_alloc(4)
    f, ub = _lib._fptr, lambda a: ctypes.cast(ctypes.c_void_p(a), ctypes.POINTER(ctypes.c_ubyte))
    assert dll.ry_mask_rows(h, f(rows), ub(mask), 4, 16, 0, 4, None) == 0
    for args in ((None, f(rows), ub(mask), 4, 16, 0, 4), (h, f(None), ub(mask), 4, 16, 0, 4), (h, f(rows), ub(0), 4, 16, 0, 4),
                 (h, f(rows), ub(mask), 0, 16, 0, 0), (h, f(rows), ub(mask), 4, 0, 0, 4), (h, f(rows), ub(mask), 4, 16, -1, 4),
                 (h, f(rows), ub(mask), 4, 16, 3, 2), (h, f(rows), ub(mask), 4, 16, 0, 5)):
        assert dll.ry_mask_rows(*args, None) == -1, args[3:]
    emu_ctx.dev_free(rows)
    emu_ctx.dev_free(mask)


@pytest.mark.parametrize('fs', P.RATES)
def test_extract_resident_equals_run_device_cast_to_float32(emu_ctx, fs):
    P.check_extract_resident(emu_ctx, fs)


def test_enqueue_wave_device_equals_submit_wave(on_emulator, tmp_path):
    """The same window through `ry_vc_submit_wave` (host arrays) and `ry_vc_enqueue_wave_device` (everything on the card): mask, count, mc and sp, with
    a threshold that splits the frames; then under a discard hint (the kept rows equal, the others untouched) and the refusals."""
    from realtime_yukarin_amd.compat.yukarin.wave import frame_power
    ctx, fs, hop, n = on_emulator, 16000, 80, 13
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    core = vc._fused_core()
    rng = numpy.random.default_rng(3)
    wave = (P.wave_of('loud', fs, n * hop / fs) * numpy.linspace(0.01, 1.0, n * hop)).astype(numpy.float32)
    feat = (rng.normal(size=(n, 9)) * [4, 1, .5, .5, .3, .3, .2, .2, .2]).astype(numpy.float32)
    p_eff = float(numpy.sort(frame_power(wave, 1024, hop))[n // 2])
    mc, sp, eff = core.wait_wave(core.submit_wave(wave, hop, 1024, p_eff, 3e38, feat))
    assert 0 < eff.sum() < n
    blocks = [ctx.dev_alloc(k) for k in (wave.size, feat.size, n * 9, n * 513, n // 4 + 2)]
    ctx.dev_upload(blocks[0], wave)
    ctx.dev_upload(blocks[1], feat)
    for discard in ((0, 0), (2, 3)):
        core.set_discard(*discard)
        ctx.dev_upload(blocks[3], numpy.full((n, 513), numpy.nan, numpy.float32))
        eff2, n_eff = core.enqueue_wave_device(blocks[0], wave.size, hop, 1024, p_eff, 3e38, blocks[1], n, *blocks[2:])
        mc2, sp2, words = numpy.empty_like(mc), numpy.empty_like(sp), numpy.empty(n // 4 + 2, numpy.float32)
        ctx.sync()
        for host, block in ((mc2, blocks[2]), (sp2, blocks[3]), (words, blocks[4])):
            ctx.dev_download(block, host)
        k0, k1 = discard[0], n - discard[1]
        assert numpy.array_equal(eff2, eff) and n_eff == eff.sum() and numpy.array_equal(words.view(numpy.uint8)[:n], eff.astype(numpy.uint8))
        assert P.same(mc2, mc) and P.same(sp2[k0:k1], sp[k0:k1])
        assert numpy.isnan(sp2[:k0]).all() and numpy.isnan(sp2[k1:]).all()
    core.set_discard(0, 0)
    dll, ub = ctx.lib.dll, lambda a: ctypes.cast(ctypes.c_void_p(a), ctypes.POINTER(ctypes.c_ubyte))
    host_mask, count = numpy.empty(n, numpy.uint8), ctypes.c_int()
    good = [core.handle, _lib._fptr(blocks[0]), wave.size, hop, 1024, p_eff, 3e38, _lib._fptr(blocks[1]), n, 1e-16, _lib._fptr(blocks[2]),
            _lib._fptr(blocks[3]), ub(blocks[4]), host_mask.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), ctypes.byref(count)]
    assert dll.ry_vc_enqueue_wave_device(*good) == 0 and count.value == eff.sum()
    for i, bad in ((0, None), (1, _lib._fptr(None)), (7, _lib._fptr(None)), (10, _lib._fptr(None)), (11, _lib._fptr(None)), (12, ub(0)), (13, None),
                   (14, None), (2, 0), (3, 0), (4, 100), (4, 2048), (8, 0)):
        args = list(good)
        args[i] = bad
        assert dll.ry_vc_enqueue_wave_device(*args) == -1, i
    for b in blocks:
        ctx.dev_free(b)
    P.close_voice_changer(vc)


@pytest.fixture
def process(on_emulator, monkeypatch, tmp_path):
    shim = P.set_up(monkeypatch, tmp_path, 1)
    yield on_emulator
    P.close_shim(shim)


def short_wave(fs, seed=0):
    """20 ms: a loud half and a half far below the gate's threshold of 1e-6 in power."""
    x = P.wave_of('loud', fs, 0.02, seed)
    x[x.size // 2:] *= numpy.float32(1e-5)
    return x


@pytest.mark.parametrize('fs', P.RATES)
def test_resident_path_equals_the_chain(process, tmp_path, fs):
    from yukarin import Wave
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    param = vc.acoustic_converter.config.dataset.acoustic_param
    pipe = pipeline.Pipeline(vc, param, crepe_capacity=1, seed=3)
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3, ctx=process)
    for x in (short_wave(fs), numpy.zeros(int(0.02 * fs), numpy.float32)):
        wave = Wave(x, fs)
        want = P.chain(vc, param, pipe.feature_class, wave, ref)
        got = pipe.convert_wave(wave)
        assert got.sampling_rate == fs and P.same(got.wave, want)
    assert pipeline.calls == {'resident': 2, 'composed': 0}
    # the live form: two buffers with a discard hint, then the flush
    waves = [Wave(short_wave(fs, s), fs) for s in (1, 2)]
    want = [P.chain_push(vc, param, pipe.feature_class, w, ref, (1, 1)) for w in waves] + [ref.flush()]
    got = [pipe.push(w, discard=(1, 1)).wave for w in waves] + [pipe.flush().wave]
    assert all(P.same(g, w) for g, w in zip(got, want)) and sum(len(w) for w in want) > 0
    assert pipeline.calls == {'resident': 4, 'composed': 0}
    pipe.close()
    ref.close()
    P.close_voice_changer(vc)


def test_composed_path_for_what_the_resident_path_does_not_take(process, tmp_path):
    """A float64 wave with more than 24 significant bits, a class nobody named as a CREPE class, a wave of two channels: the separate calls,
    unchanged -- the chain's bits, or the chain's refusal."""
    from yukarin import Wave
    fs = 24000
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    param = vc.acoustic_converter.config.dataset.acoustic_param
    named = pipeline.crepe_feature_class()
    other = type('OtherFeature', (named.__mro__[1],), {'extract_f0': named.__dict__['extract_f0']})
    x64 = short_wave(fs).astype(numpy.float64)
    x64[100] += 2.0 ** -40
    assert not numpy.array_equal(x64.astype(numpy.float32).astype(numpy.float64), x64)
    x2 = numpy.stack([short_wave(fs), short_wave(fs, 1)], 1)
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3, ctx=process)
    for i, (cls, x) in enumerate(((named, x64), (other, short_wave(fs)), (named, x2))):
        pipe = pipeline.Pipeline(vc, param, crepe_capacity=1, seed=3, feature_class=cls)
        wave = Wave(x, fs)
        assert pipe._resident_handles(wave) is None
        try:
            want = P.chain(vc, param, cls, wave, ref)
        except Exception as e:                                      # what the separate calls refuse, the pipeline refuses in the same words
            with pytest.raises(type(e)) as ei:
                pipe.convert_wave(wave)
            assert str(ei.value) == str(e)
        else:
            assert P.same(pipe.convert_wave(wave).wave, want)
        assert pipeline.calls == {'resident': 0, 'composed': i + 1}
        pipe.close()
    ref.close()
    P.close_voice_changer(vc)
