"""WORLD synthesis on the MI355X: `Synthesizer`, the handle over `ry_synth_*` (include/ry355.h), and the two `decode` bodies that bind it
over the reference's `Vocoder.decode` / `RealtimeVocoder.decode` (realtime_voice_conversion/yukarin_wrapper/vocoder.py:50-120):

    from realtime_yukarin_amd import world_synth
    Vocoder.decode = world_synth.decode
    RealtimeVocoder.decode = world_synth.decode_realtime
    RealtimeVocoder.create_synthesizer = world_synth.create_synthesizer

`pyworld` / `world4py` are never imported on this path and never shadowed.  The arithmetic is WORLD's `Synthesis` restated
(tests/world_synth_ref.py); it deviates from `pyworld` in two stated ways -- the noise is a counter-based function of (seed, sample
position) instead of a process-global xorshift sequence, and the pulse phase is wrapped at every step instead of once at the end -- and
parity at the `pyworld` boundary is unpinned: the package cannot be installed where this was built.

Spectrogram and aperiodicity travel as float32 `[frames][513]` rows (what stage 2 writes); `DeviceRows` -- rows already on the card,
e.g. a stage-2 output left there -- are read where they are, without a host round trip (a `fusion.LazySpectrogram` stands for the INPUT
of stage 2 and is materialised).  f0 goes in and the float64 wave comes out through the host."""
import ctypes
import os
from typing import Optional

import numpy

from . import _lib
from ._handle import _DP, DeviceHandle, EngineForTests

FFT_SIZE = 1024
BINS = FFT_SIZE // 2 + 1
# which path `Synthesizer.synthesize_many` took, counted per call: 'in_place' (device rows read where they are), 'packed' (host rows, one
# upload) -- both ONE `ry_synth_run_many` --, 'fallback' (one `synthesize` per item)
calls = {'in_place': 0, 'packed': 0, 'fallback': 0}


def cheaptrick_fft_size(fs, f0_floor: float = 71.0) -> int:
    return int(2 ** (1 + int(numpy.log2(3.0 * fs / f0_floor + 1))))


class DeviceRows(object):
    """`[frames][513]` float32 rows that are already on the GPU of the synthesizer's context (e.g. a stage-2 output left there)."""

    def __init__(self, address: int, frames: int, keep=None):
        self.address, self.frames, self.keep = int(address), int(frames), keep
        self.shape = (self.frames, BINS)


class Synthesizer(DeviceHandle):
    """WORLD synthesis on the device (`ry_synth_*`).  One-shot `synthesize`, or a stream: `push` returns the samples that can no longer
    change (it lags the input by about fft_size / 2 samples + one frame + one pulse period), `flush` the rest; the concatenation equals
    `synthesize` on the concatenated frames bit for bit, for any cut.  `fft_size=None` is CheapTrick's size at `fs`; the kernels are built for
    1024, so rates other than 16 to 24 kHz (8 .. 48 kHz are accepted) need `fft_size=1024` rows.  `ctx` (tests): a context over another build
    of the library."""

    def __init__(self, fs: int, frame_period: float = 5.0, seed: int = 0, ctx=None, device: Optional[int] = None, fft_size: Optional[int] = None):
        self.fs, self.frame_period, self.seed = int(fs), float(frame_period), int(seed) & 0xffffffff
        self.fft_size = int(fft_size) if fft_size else cheaptrick_fft_size(self.fs)
        DeviceHandle.__init__(self, ctx, device)

    _destroy = 'ry_synth_destroy'

    def _create(self, lib, ctx):
        h = ctypes.c_void_p()
        lib.check(lib.dll.ry_synth_create(ctx.handle, self.fs, self.frame_period, self.fft_size, self.seed, ctypes.byref(h)))
        return h

    # ---- arguments
    @staticmethod
    def _rows(a, n, name):
        """-> (pointer, on_device, keep-alive)."""
        if isinstance(a, DeviceRows):
            if a.frames != n:
                raise ValueError('%s has %d device rows, f0 has %d frames' % (name, a.frames, n))
            return _lib._fptr(a.address), True, a
        h = numpy.ascontiguousarray(a, dtype=numpy.float32)
        if h.ndim != 2 or h.shape[0] != n:
            raise ValueError('%s must be (%d, bins), got %s' % (name, n, h.shape))
        return _lib._fptr(h), False, h

    def _frames(self, f0, sp, ap):
        f0 = numpy.ascontiguousarray(numpy.asarray(f0, dtype=numpy.float64).reshape(-1))
        n = f0.size
        from . import fusion
        if isinstance(sp, fusion.LazySpectrogram):
            sp = device_spectrogram(sp)
        psp, dsp, ksp = self._rows(sp, n, 'sp')
        pap, dap, kap = self._rows(ap, n, 'ap')
        bins = int(sp.shape[1]) if not dsp else BINS
        if not dap and ap.shape[1] != bins:
            raise ValueError('sp has %d bins, ap %d' % (bins, ap.shape[1]))
        if dsp != dap:                                             # one flag in the ABI: bring the host side over
            if not dsp:
                ksp = _upload(self._ctx, ksp)
                psp = _lib._fptr(ksp.address)
            else:
                kap = _upload(self._ctx, kap)
                pap = _lib._fptr(kap.address)
            dsp = dap = True
        return f0, n, psp, pap, bins, int(dsp), (ksp, kap)

    # ---- calls
    def length(self, n_frames: int) -> int:
        return int((int(n_frames) - 1) * self.frame_period / 1000 * self.fs) + 1

    def synthesize(self, f0, sp, ap) -> numpy.ndarray:
        lib, h = self._get()
        f0, n, psp, pap, bins, dev, keep = self._frames(f0, sp, ap)
        y = numpy.empty(max(self.length(n), 1) if n > 0 else 1, numpy.float64)
        got = ctypes.c_int()
        lib.check(lib.dll.ry_synth_run(h, f0.ctypes.data_as(_DP), psp, pap, n, bins, dev, y.ctypes.data_as(_DP), y.size, ctypes.byref(got)))
        return y[:got.value]

    def synthesize_many(self, items) -> list:
        """`items`: a list of `(f0, sp, ap)` -> the list of their waves, each with the bits of `synthesize` on it alone, in ONE device call
        (`ry_synth_run_many`): host rows are packed and uploaded once, `DeviceRows` that are consecutive slices of one buffer -- a batched
        stage-2 output -- are read where they are.  Lists that mix host and device rows, or whose device rows do not follow one another, are
        synthesized item by item (`calls` says which path ran)."""
        items = [self._item(*it) for it in items]
        if not items:
            return []
        lib, h = self._get()
        kinds = set(dev for _, _, _, dev in items)
        row = BINS * 4
        in_place = kinds == {True} and all(b[k].address == a[k].address + a[k].frames * row for a, b in zip(items, items[1:]) for k in (1, 2))
        if not (in_place or kinds == {False}):
            calls['fallback'] += 1
            return [self.synthesize(f0, sp, ap) for f0, sp, ap, _ in items]
        for f0, sp, ap, dev in items:
            if not dev and (sp.shape[1] != BINS or ap.shape[1] != BINS):
                raise ValueError('%d bins per frame, %d expected' % (sp.shape[1], BINS))
        f0 = numpy.ascontiguousarray(numpy.concatenate([it[0] for it in items]))
        n = numpy.array([it[0].size for it in items], numpy.int32)
        if in_place:
            keep = items
            psp, pap = _lib._fptr(items[0][1].address), _lib._fptr(items[0][2].address)
        else:
            keep = (numpy.concatenate([it[1] for it in items]), numpy.concatenate([it[2] for it in items]))
            psp, pap = _lib._fptr(keep[0]), _lib._fptr(keep[1])
        off = numpy.zeros(len(items) + 1, numpy.int64)
        y = numpy.empty(max(sum(self.length(int(k)) for k in n if k > 0), 1), numpy.float64)
        lib.check(lib.dll.ry_synth_run_many(h, f0.ctypes.data_as(_DP), psp, pap, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(items), BINS,
                                            int(in_place), y.ctypes.data_as(_DP), y.size, off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        calls['in_place' if in_place else 'packed'] += 1
        del keep
        return [y[off[i]:off[i + 1]].copy() for i in range(len(items))]

    def _item(self, f0, sp, ap):
        """-> (f0 float64 [n], sp, ap, on_device); sp / ap float32 `[n][bins]` arrays, or both `DeviceRows`; one of each: as they came."""
        f0 = numpy.ascontiguousarray(numpy.asarray(f0, dtype=numpy.float64).reshape(-1))
        from . import fusion
        if isinstance(sp, fusion.LazySpectrogram):
            sp = device_spectrogram(sp)
        dsp, dap = isinstance(sp, DeviceRows), isinstance(ap, DeviceRows)
        if dsp != dap:
            return f0, sp, ap, None
        return f0, self._rows(sp, f0.size, 'sp')[2], self._rows(ap, f0.size, 'ap')[2], dsp

    def pulses_many(self, wave: int):
        """`pulses()` for wave `wave` of the last `synthesize_many` that ran as one call (`ry_synth_debug_pulses_many`)."""
        lib, h = self._get()
        n = ctypes.c_int()
        lib.check(lib.dll.ry_synth_debug_pulses_many(h, int(wave), None, None, None, 0, ctypes.byref(n)))
        idx, sh, vo = numpy.empty(n.value, numpy.int64), numpy.empty(n.value, numpy.float64), numpy.empty(n.value, numpy.int32)
        lib.check(lib.dll.ry_synth_debug_pulses_many(h, int(wave), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), sh.ctypes.data_as(_DP),
                                                     vo.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n.value, ctypes.byref(n)))
        return idx, sh, vo != 0

    def push(self, f0, sp, ap) -> numpy.ndarray:
        lib, h = self._get()
        f0, n, psp, pap, bins, dev, keep = self._frames(f0, sp, ap)
        y = numpy.empty(max(int(lib.dll.ry_synth_bound(h, max(n, 0), 0)), 1), numpy.float64)
        got = ctypes.c_int()
        lib.check(lib.dll.ry_synth_push(h, f0.ctypes.data_as(_DP), psp, pap, n, bins, dev, y.ctypes.data_as(_DP), y.size, ctypes.byref(got)))
        return y[:got.value].copy()

    def flush(self) -> numpy.ndarray:
        lib, h = self._get()
        y = numpy.empty(max(int(lib.dll.ry_synth_bound(h, 0, 1)), 1), numpy.float64)
        got = ctypes.c_int()
        lib.check(lib.dll.ry_synth_flush(h, y.ctypes.data_as(_DP), y.size, ctypes.byref(got)))
        return y[:got.value].copy()

    def reset(self) -> None:
        lib, h = self._get()
        lib.check(lib.dll.ry_synth_reset(h))

    def pulses(self):
        """(index int64, shift float64 in samples, voiced bool) of the pulses the last call found (`ry_synth_debug_pulses`)."""
        lib, h = self._get()
        n = ctypes.c_int()
        lib.check(lib.dll.ry_synth_debug_pulses(h, None, None, None, 0, ctypes.byref(n)))
        idx, sh, vo = numpy.empty(n.value, numpy.int64), numpy.empty(n.value, numpy.float64), numpy.empty(n.value, numpy.int32)
        lib.check(lib.dll.ry_synth_debug_pulses(h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), sh.ctypes.data_as(_DP),
                                                vo.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n.value, ctypes.byref(n)))
        return idx, sh, vo != 0

    def poison(self) -> None:
        lib, h = self._get()
        lib.check(lib.dll.ry_synth_debug_poison(h))

    def lag_samples(self, f0: float = 500.0) -> int:
        """What `push` holds back at most: half a transform, one frame, one pulse period (of `f0`; 500 Hz: unvoiced)."""
        return self.fft_size // 2 + int(numpy.ceil(self.fs * self.frame_period / 1000)) + int(numpy.ceil(self.fs / f0))


class _DeviceBuffer(object):
    """A `ry_dev_alloc` buffer that frees itself."""

    def __init__(self, ctx, n_floats):
        self.ctx = ctx
        p = _lib._FP()
        ctx.lib.check(ctx.lib.dll.ry_dev_alloc(ctx.handle, int(n_floats), ctypes.byref(p)))
        self.ptr = p
        self.address = ctypes.cast(p, ctypes.c_void_p).value

    def __del__(self):
        try:
            if self.ctx.handle is not None and self.ptr:
                self.ctx.lib.dll.ry_dev_free(self.ctx.handle, self.ptr)
        except Exception:
            pass


def _upload(ctx, host: numpy.ndarray) -> DeviceRows:
    buf = _DeviceBuffer(ctx, host.size)
    ctx.lib.check(ctx.lib.dll.ry_dev_upload(ctx.handle, buf.ptr, _lib._fptr(host), host.size))
    return DeviceRows(buf.address, host.shape[0], keep=buf)


def to_device(ctx, rows) -> DeviceRows:
    """Host `[frames][513]` rows -> `DeviceRows` on the GPU of `ctx` (tests, callers without a tensor library)."""
    h = numpy.ascontiguousarray(rows, dtype=numpy.float32)
    if h.ndim != 2 or h.shape[1] != BINS:
        raise ValueError('rows must be (frames, %d), got %s' % (BINS, h.shape))
    return _upload(ctx, h)


def device_spectrogram(sp):
    """A `fusion.LazySpectrogram` stays what it is until somebody looks at it; this asks for its float32 array (the device rows it stands
    for are the INPUT of stage 2 -- the synthesizer wants the output, which the caller hands over as an array or as `DeviceRows`)."""
    return numpy.asarray(sp, dtype=numpy.float32)


# ---- the reference's methods ---------------------------------------------------------------------------------------------------------
engine_for_tests = EngineForTests()           # for the synthesizers the bindings below create


def _new_synth(vocoder) -> Synthesizer:
    return Synthesizer(vocoder.out_sampling_rate, vocoder.acoustic_param.frame_period, seed=int(os.environ.get('RY_SYNTH_SEED', '0')),
                       ctx=engine_for_tests.ctx)


def _synth_of(self, key='_ry_synth'):
    s = getattr(self, key, None)
    if s is None:
        s = _new_synth(self)
        setattr(self, key, s)
    return s


def decode(self, acoustic_feature):
    """Drop-in body of `Vocoder.decode` (vocoder.py:50-62): `pyworld.synthesize` of the whole feature -> `Wave` (float64)."""
    from yukarin import Wave
    f = acoustic_feature
    out = _synth_of(self).synthesize(numpy.asarray(f.f0).ravel(), f.sp, f.ap)
    return Wave(out, sampling_rate=self.out_sampling_rate)


def decode_many(self, features):
    """The list form of `decode`: the waves of a list of features in one device call (`Synthesizer.synthesize_many`), each equal to `decode` of
    its feature bit for bit.  An empty list gives `[]`."""
    from yukarin import Wave
    features = list(features)
    if not features:
        return []
    outs = _synth_of(self).synthesize_many([(numpy.asarray(f.f0).ravel(), f.sp, f.ap) for f in features])
    return [Wave(o, sampling_rate=self.out_sampling_rate) for o in outs]


def create_synthesizer(self, buffer_size: int, number_of_pointers: int):
    """Drop-in body of `RealtimeVocoder.create_synthesizer` (vocoder.py:72-87): world4py's ring of `number_of_pointers` parameter sets and
    its `buffer_size` output block have no counterpart -- the device stream takes pushes of any size and returns what is final."""
    assert self._synthesizer is None
    self._synthesizer = _new_synth(self)
    self._synthesizer.buffer_size = int(buffer_size)
    self._synthesizer.number_of_pointers = int(number_of_pointers)


def decode_realtime(self, acoustic_feature):
    """Drop-in body of `RealtimeVocoder.decode` (vocoder.py:89-120): the frames go to the stream, the samples that are final come back."""
    from yukarin import Wave
    assert self._synthesizer is not None
    f = acoustic_feature
    out = self._synthesizer.push(numpy.asarray(f.f0).ravel(), f.sp, f.ap)
    return Wave(wave=out, sampling_rate=self.out_sampling_rate)
