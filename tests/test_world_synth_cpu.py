"""The WORLD synthesis kernels (realtime_yukarin_amd/csrc/synth_kernels.h) on the host-side SIMT emulator against the numpy restatement
(tests/world_synth_ref.py): short inputs -- the emulator is slow --, the stream against the one-shot call bit for bit, the refusals of the
C ABI, and the two `decode` bindings on the bodies of the reference's `Vocoder` / `RealtimeVocoder` (restated, as tests/test_vocoder_feed.py
restates them)."""
import ctypes
import sys
from pathlib import Path

import numpy
import pytest

import world_synth_cases as C
import world_synth_ref as R
from realtime_yukarin_amd import _lib, compat, world_synth

ROOT = Path(__file__).resolve().parent.parent
BAR = 4 * float([l for l in (ROOT / 'profiles' / 'r08' / 'synth_tolerance.txt').read_text().splitlines() if l.startswith('worst float64')][0].split()[-1])
_DP = ctypes.POINTER(ctypes.c_double)


def rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(numpy.abs(a - b).max() / max(numpy.abs(b).max(), 1e-300))


@pytest.mark.parametrize('fs,kind,n', [(16000, 'glide', 60), (24000, 'glide', 40), (16000, 'unvoiced', 20), (24000, 'above', 45), (16000, 'voiced800', 12),
                                      (16000, 'glide', 1), (24000, 'glide', 2)])
def test_kernels_match_the_restatement(emu_ctx, fs, kind, n):
    f0, sp, ap = C.case(kind, n, fs)
    want, P, _ = R.synthesize(f0, sp, ap, fs, 5.0, seed=4, return_pulses=True)
    s = world_synth.Synthesizer(fs, 5.0, seed=4, ctx=emu_ctx)
    y = s.synthesize(f0, sp, ap)
    idx, shift, voiced = s.pulses()
    assert len(y) == len(want) == int((n - 1) * 5.0 / 1000 * fs) + 1
    assert list(idx) == [p[0] for p in P] and list(voiced) == [p[2] for p in P]
    if P:
        assert numpy.abs(shift - numpy.array([p[1] for p in P])).max() <= 1e-9
        e = rel(y, want)
        print('%s fs=%d n=%d: %d pulses, rel err %.3g (bar %.3g)' % (kind, fs, n, len(P), e, BAR))
        assert e <= BAR
    else:
        assert not y.any()
    assert numpy.array_equal(s.synthesize(f0, sp, ap), y)                       # and again: the same bits
    s.close()


@pytest.mark.parametrize('cuts', [[1] * 30, [7, 13, 10], [29, 1], [2, 28], [30]])
def test_stream_equals_one_shot_bit_for_bit(emu_ctx, cuts):
    n, fs = sum(cuts), 16000
    f0, sp, ap = C.case('glide', n, fs)
    s = world_synth.Synthesizer(fs, 5.0, seed=2, ctx=emu_ctx)
    want = s.synthesize(f0, sp, ap)
    out, i = [], 0
    for c in cuts:
        out.append(s.push(f0[i:i + c], sp[i:i + c], ap[i:i + c]))
        i += c
        assert int((i - 1) * 5.0 / 1000 * fs) + 1 - sum(map(len, out)) <= s.lag_samples(f0=fs / 1024 + 1) + 1
    out.append(s.flush())
    assert numpy.array_equal(numpy.concatenate(out), want)
    # the stream starts again after a flush, and a poisoned scratch changes nothing
    s.poison()
    again = numpy.concatenate([s.push(f0[:11], sp[:11], ap[:11]), s.push(f0[11:], sp[11:], ap[11:]), s.flush()])
    assert numpy.array_equal(again, want)
    s.close()


def test_float64_and_device_rows_take_the_same_path(emu_ctx):
    n, fs = 12, 16000
    f0, sp, ap = C.case('glide', n, fs)
    s = world_synth.Synthesizer(fs, 5.0, seed=1, ctx=emu_ctx)
    y = s.synthesize(f0.astype(numpy.float32).astype(numpy.float64), sp, ap)
    assert numpy.array_equal(s.synthesize(f0.astype(numpy.float32), sp.astype(numpy.float64), ap.astype(numpy.float64)), y)
    dsp, dap = world_synth.to_device(emu_ctx, sp), world_synth.to_device(emu_ctx, ap)
    assert numpy.array_equal(s.synthesize(f0.astype(numpy.float32), dsp, dap), y)
    assert numpy.array_equal(s.synthesize(f0.astype(numpy.float32), dsp, ap), y)          # mixed: the host side is brought over
    s.close()


def test_abi_refusals(emu_ctx):
    lib, d = emu_ctx.lib, emu_ctx.lib.dll
    h = ctypes.c_void_p()
    for args in ((16000, 5.0, 2048, 0), (16000, 5.0, 512, 0), (10, 5.0, 1024, 0), (16000, 0.0, 1024, 0), (16000, float('nan'), 1024, 0)):
        assert d.ry_synth_create(emu_ctx.handle, *args, ctypes.byref(h)) == -1 and not h.value, args
    assert b'fft_size' in d.ry_last_error() or b'frame period' in d.ry_last_error()
    lib.check(d.ry_synth_create(emu_ctx.handle, 16000, 5.0, 1024, 0, ctypes.byref(h)))
    n = 4
    f0, sp, ap = C.case('glide', n, 16000)
    y = numpy.full(2000, numpy.nan)
    got = ctypes.c_int(-5)

    def run(fn, f0_, n_, bins, cap):
        return fn(h, f0_.ctypes.data_as(_DP), _lib._fptr(sp), _lib._fptr(ap), n_, bins, 0, y.ctypes.data_as(_DP), cap, ctypes.byref(got))
    for fn in (d.ry_synth_run, d.ry_synth_push):
        assert run(fn, f0, 0, 513, 2000) == -1 and b'at least one frame' in d.ry_last_error()
        assert run(fn, f0, n, 512, 2000) == -1 and b'bins' in d.ry_last_error()
        assert run(fn, f0, n, 1025, 2000) == -1
        bad = f0.copy(); bad[2] = numpy.inf
        assert run(fn, bad, n, 513, 2000) == -1 and b'finite' in d.ry_last_error()
        bad[2] = numpy.nan
        assert run(fn, bad, n, 513, 2000) == -1
        assert run(fn, f0, n, 513, 100) == -1 and b'y holds' in d.ry_last_error()
        assert got.value == 0 and numpy.isnan(y).all()
    assert d.ry_synth_flush(h, y.ctypes.data_as(_DP), 2000, ctypes.byref(got)) == -4                    # nothing was pushed
    assert d.ry_synth_length(h, n) == 241 and d.ry_synth_bound(h, n, 0) == 240 and d.ry_synth_bound(h, n, 1) == 241
    assert run(d.ry_synth_run, f0, n, 513, 241) == 0 and got.value == 241 and numpy.isfinite(y[:241]).all() and numpy.isnan(y[241:]).all()
    assert d.ry_synth_run(None, None, None, None, 1, 513, 0, None, 0, None) == -4
    d.ry_synth_destroy(h)
    d.ry_synth_destroy(None)


# ---- the reference's classes, restated (realtime_voice_conversion/yukarin_wrapper/vocoder.py:15-126) ---------------------------------
class _Param(object):
    frame_period = 5.0


class Vocoder(object):
    def __init__(self, acoustic_param, out_sampling_rate, extract_f0_mode=None):
        self.acoustic_param = acoustic_param
        self.out_sampling_rate = out_sampling_rate
        self.extract_f0_mode = extract_f0_mode

    def encode(self, wave):                                         # the caller's WORLD: not part of this project
        raise NotImplementedError

    def decode(self, acoustic_feature):
        import pyworld
        acoustic_feature = acoustic_feature.astype_only_float(numpy.float64)
        out = pyworld.synthesize(f0=acoustic_feature.f0.ravel(), spectrogram=acoustic_feature.spectrogram, aperiodicity=acoustic_feature.aperiodicity,
                                 fs=self.out_sampling_rate, frame_period=self.acoustic_param.frame_period)
        from yukarin import Wave
        return Wave(out, sampling_rate=self.out_sampling_rate)


class RealtimeVocoder(Vocoder):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._synthesizer = None
        self._before_buffer = []

    def create_synthesizer(self, buffer_size, number_of_pointers):
        from world4py.native import structures
        assert self._synthesizer is None
        self._synthesizer = structures.WorldSynthesizer()

    def decode(self, acoustic_feature):
        from world4py.native import apidefinitions
        raise AssertionError('world4py reached')

    def warm_up(self, time_length):
        from yukarin import Wave
        y = numpy.zeros(int(time_length * self.out_sampling_rate))
        f = self.encode(Wave(wave=y, sampling_rate=self.out_sampling_rate))
        self.decode(f)


def _feature(n, fs, dtype=numpy.float32):
    from yukarin import AcousticFeature
    f0, sp, ap = C.case('glide', n, fs)
    f0 = f0.astype(numpy.float32)                                   # the features are float32 on the convert side, float64 on the decode side
    return AcousticFeature(f0=f0.reshape(-1, 1).astype(dtype), sp=sp.astype(dtype), ap=ap.astype(dtype), voiced=f0.reshape(-1, 1) > 0)


def test_decode_bindings_on_the_reference_bodies(emu_ctx, monkeypatch):
    """`Vocoder.decode = world_synth.decode`, `RealtimeVocoder.decode = world_synth.decode_realtime` (+ create_synthesizer): `Wave`s of the right
    rate, dtype and length; neither `pyworld` nor `world4py` is imported."""
    compat.install()
    from yukarin import Wave
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(Vocoder, 'decode', world_synth.decode)
    monkeypatch.setattr(RealtimeVocoder, 'decode', world_synth.decode_realtime)
    monkeypatch.setattr(RealtimeVocoder, 'create_synthesizer', world_synth.create_synthesizer)
    for m in ('pyworld', 'world4py', 'world4py.native'):
        monkeypatch.setitem(sys.modules, m, None)                   # an import of either raises ImportError
    fs, n = 24000, 30
    f = _feature(n, fs)
    v = Vocoder(_Param(), fs)
    w = v.decode(f)
    assert isinstance(w, Wave) and w.sampling_rate == fs and w.wave.dtype == numpy.float64 and len(w.wave) == int((n - 1) * 5.0 / 1000 * fs) + 1
    want = R.synthesize(f.f0.ravel(), f.sp, f.ap, fs, 5.0, seed=0)
    assert rel(w.wave, want) <= BAR
    assert numpy.array_equal(v.decode(_feature(n, fs, numpy.float64)).wave, w.wave)     # the decode side's float64 features: the same float32 rows
    r = RealtimeVocoder(_Param(), fs)
    r.create_synthesizer(buffer_size=1024, number_of_pointers=16)
    parts = [r.decode(_feature(n, fs)) for _ in range(3)]
    assert all(isinstance(p, Wave) and p.sampling_rate == fs and p.wave.dtype == numpy.float64 for p in parts)
    total = sum(len(p.wave) for p in parts)
    assert 0 < 3 * n * 120 - total <= r._synthesizer.lag_samples(f0=fs / 1024 + 1) + 120
    three = R.synthesize(numpy.tile(f.f0.ravel(), 3), numpy.tile(f.sp, (3, 1)), numpy.tile(f.ap, (3, 1)), fs, 5.0, seed=0)
    assert rel(numpy.concatenate([p.wave for p in parts]), three[:total]) <= BAR
    # warm_up: its encode half is the caller's WORLD; the decode half runs here
    monkeypatch.setattr(RealtimeVocoder, 'encode', lambda self, wave: _feature(len(wave.wave) // 120 + 1, fs))
    r.warm_up(0.05)
    r._synthesizer.close()
    v._ry_synth.close()
