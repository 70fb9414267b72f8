"""The tail of the reference's decode worker on the MI355X: `OutputGate` / `OutputGateBank`, the handles over `ry_outgate_*` (include/ry355.h).

    wave_fragment = numpy.concatenate([wave_fragment, wave])                     # worker/decode_worker.py:53-59
    if len(wave_fragment) >= out_audio_chunk:
        wave, wave_fragment = wave_fragment[:out_audio_chunk], wave_fragment[out_audio_chunk:]
        power = librosa.core.power_to_db(numpy.abs(librosa.stft(wave)) ** 2).mean()
        if power < - output_silent_threshold:
            wave = None
    else:
        wave = None

becomes `wave = gate.push(wave)`: the fragment is carried on the card, the 2048-point STFT of the chunk runs there, and a silent chunk -- the
common case between utterances -- brings no sample back to the host.  `scale` / `dtype=numpy.float32` fold in run.py:194-198
(`out_wave *= output_scale`, `.astype(numpy.float32)`); NaN samples are replaced by 0.0 as `DecodeStream.process` does (decode_stream.py:38).
`librosa` is never imported: the expression is restated in float64 (`host_mean_db`, tests/output_gate_ref.py), and parity at the librosa
boundary, which stores the STFT as complex64, is unpinned.  There is no CPU path for chunks the card takes; chunk sizes
below 1025 samples, which the C ABI refuses because the reflect padding would wrap twice, are judged by `host_mean_db` on the host."""
import ctypes
from typing import Optional

import numpy

from ._handle import _DP, DeviceHandle, _dptr

N_FFT = 2048
HOP = 512
MIN_DEVICE_CHUNK = N_FFT // 2 + 1


def host_mean_db(wave) -> float:
    """`librosa.core.power_to_db(numpy.abs(librosa.stft(wave)) ** 2).mean()` in float64 numpy: n_fft 2048, hop 512, periodic Hann window,
    center=True with reflect padding, amin 1e-10, ref 1.0, top_db 80."""
    wave = numpy.asarray(wave, numpy.float64).reshape(-1)
    if wave.size < 2:
        raise ValueError('reflect padding needs at least two samples')
    y = numpy.pad(wave, (N_FFT // 2, N_FFT // 2), mode='reflect')     # a short wave is reflected as often as it takes, as in librosa
    n_frames = 1 + wave.size // HOP
    window = 0.5 - 0.5 * numpy.cos(2.0 * numpy.pi * numpy.arange(N_FFT) / N_FFT)
    frames = numpy.lib.stride_tricks.as_strided(y, (n_frames, N_FFT), (HOP * y.strides[0], y.strides[0]))
    power = numpy.abs(numpy.fft.rfft(frames * window, axis=1)) ** 2
    db = 10.0 * numpy.log10(numpy.maximum(1e-10, power))
    db = numpy.maximum(db, db.max() - 80.0)
    return float(db.mean())


class _HostGate(object):
    """The same bookkeeping for a chunk size the card does not take (below 1025 samples), judged by `host_mean_db`."""

    def __init__(self, chunk, threshold_db, scale, dtype):
        self.chunk, self.threshold_db, self.scale, self.dtype = chunk, threshold_db, scale, dtype
        self.fragment = numpy.empty(0, numpy.float64)

    def push(self, wave):
        wave = numpy.array(wave, numpy.float64).reshape(-1)
        wave[numpy.isnan(wave)] = 0
        self.fragment = numpy.concatenate([self.fragment, wave])
        if len(self.fragment) < self.chunk:
            return None, (False, False, 0.0)
        wave, self.fragment = self.fragment[:self.chunk], self.fragment[self.chunk:]
        with numpy.errstate(all='ignore'):
            mean = host_mean_db(wave)
        silent = bool(mean < -self.threshold_db)
        return (None if silent else (wave * self.scale).astype(self.dtype)), (True, silent, mean)


def _check(chunk, threshold_db, scale, dtype):
    dtype = numpy.dtype(dtype)
    if dtype not in (numpy.dtype(numpy.float64), numpy.dtype(numpy.float32)):
        raise ValueError('dtype must be float64 or float32, got %s' % dtype)
    if int(chunk) < 2:
        raise ValueError('a chunk of %d samples' % int(chunk))
    if numpy.isnan(threshold_db) or numpy.isnan(scale):
        raise ValueError('the threshold and the scale must not be NaN')
    return int(chunk), float(threshold_db), float(scale), dtype


def _samples(wave):
    """-> float64 host samples (NaN is scrubbed on the card)."""
    return numpy.ascontiguousarray(numpy.asarray(wave, dtype=numpy.float64).reshape(-1))


class OutputGate(DeviceHandle):
    """`push(wave)` -> the next chunk of `chunk` samples times `scale` as `dtype`, or None when no chunk was completed or the chunk is silent --
    what `decode_worker` puts into `item.item`.  At most one chunk per push; the rest stays carried (on the card).  `last` = (emitted, silent,
    mean_db) of the last push.  `ctx` (tests): a context over another build of the library."""
    _destroy = 'ry_outgate_destroy'

    def __init__(self, chunk: int, threshold_db: float, scale: float = 1.0, dtype=numpy.float64, ctx=None, device: Optional[int] = None):
        self.chunk, self.threshold_db, self.scale, self.dtype = _check(chunk, threshold_db, scale, dtype)
        self.last = (False, False, 0.0)
        self._host = _HostGate(self.chunk, self.threshold_db, self.scale, self.dtype) if self.chunk < MIN_DEVICE_CHUNK else None
        DeviceHandle.__init__(self, ctx, device)

    def __getstate__(self):
        d = DeviceHandle.__getstate__(self)
        if self._host is not None:
            d['_host'] = _HostGate(self.chunk, self.threshold_db, self.scale, self.dtype)
        return d

    def _create(self, lib, ctx):
        h = ctypes.c_void_p()
        lib.check(lib.dll.ry_outgate_create(ctx.handle, self.chunk, self.threshold_db, self.scale, int(self.dtype == numpy.float32), ctypes.byref(h)))
        return h

    def push(self, wave) -> Optional[numpy.ndarray]:
        if self._host is not None:
            out, self.last = self._host.push(wave)
            return out
        x = _samples(wave)
        return self._push(_dptr(x), x.size, 0)

    def _push(self, samples, n, on_device):
        lib, h = self._get()
        out = numpy.empty(self.chunk, self.dtype)
        n_out, silent, mean = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        lib.check(lib.dll.ry_outgate_push(h, samples, n, on_device, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n_out), ctypes.byref(silent),
                                          ctypes.byref(mean)))
        self.last = (n_out.value > 0, bool(silent.value), float(mean.value))
        return out if n_out.value > 0 and not silent.value else None

    def on_device(self, ctx=None) -> bool:
        """Whether `push_device` exists for this gate: it judges on the card (chunk >= MIN_DEVICE_CHUNK) -- and, with `ctx`, on that context,
        whose device pointers it can then read."""
        if self._host is not None:
            return False
        self._get()
        return ctx is None or self._ctx is ctx

    def push_device(self, ptr: int, n: int) -> Optional[numpy.ndarray]:
        """`push` of `n` float64 samples that are on the card at address `ptr` (e.g. where `Synthesizer.push_device` left them), read in the
        order of the context stream: nothing goes up but the gate's table, and only an audible chunk comes down.  Returns what `push` returns
        and sets `last` the same way.  A gate on the host fallback (`chunk < MIN_DEVICE_CHUNK`) has no device form."""
        if self._host is not None:
            raise ValueError('a chunk of %d samples is judged on the host: no device form below %d' % (self.chunk, MIN_DEVICE_CHUNK))
        n = int(n)
        if n < 0 or (n > 0 and not ptr):
            raise ValueError('%d samples at address %r' % (n, ptr))
        return self._push(ctypes.cast(ctypes.c_void_p(int(ptr or 0)), _DP), n, 1)

    def held(self) -> int:
        if self._host is not None:
            return len(self._host.fragment)
        lib, h = self._get()
        n = int(lib.dll.ry_outgate_held(h))
        if n < 0:
            lib.check(n)
        return n

    def reset(self) -> None:
        if self._host is not None:
            self._host.fragment = numpy.empty(0, numpy.float64)
            return
        lib, h = self._get()
        lib.check(lib.dll.ry_outgate_reset(h))

    def counts(self) -> dict:
        """tests: what the last push cost."""
        lib, h = self._get()
        c = (ctypes.c_longlong * 5)()
        lib.check(lib.dll.ry_outgate_debug_counts(h, c))
        d = dict(zip(('waits', 'launches', 'uploads', 'downloads', 'sample_bytes_down'), (int(v) for v in c)))
        d['upload_bytes'] = int(lib.dll.ry_outgate_debug_upload_bytes(h))
        return d

    def poison(self) -> None:
        lib, h = self._get()
        lib.check(lib.dll.ry_outgate_debug_poison(h))


class OutputGateBank(DeviceHandle):
    """`n_streams` output gates with one chunk size, threshold, scale and dtype, served by ONE device call per buffer.  `push(waves)` -> a list:
    entry b is what `OutputGate.push(waves[b])` of a lone gate returns, bit for bit; a stream whose wave is None or empty sits the call out.
    `last[b]` = (emitted, silent, mean_db)."""
    _destroy = 'ry_outgate_bank_destroy'

    def __init__(self, n_streams: int, chunk: int, threshold_db: float, scale: float = 1.0, dtype=numpy.float64, ctx=None, device: Optional[int] = None):
        self.n_streams = int(n_streams)
        if self.n_streams < 1:
            raise ValueError('%d streams' % self.n_streams)
        self.chunk, self.threshold_db, self.scale, self.dtype = _check(chunk, threshold_db, scale, dtype)
        self.last = [(False, False, 0.0)] * self.n_streams
        self._host = None
        if self.chunk < MIN_DEVICE_CHUNK:
            self._host = [_HostGate(self.chunk, self.threshold_db, self.scale, self.dtype) for _ in range(self.n_streams)]
        DeviceHandle.__init__(self, ctx, device)

    def __getstate__(self):
        d = DeviceHandle.__getstate__(self)
        if self._host is not None:
            d['_host'] = [_HostGate(self.chunk, self.threshold_db, self.scale, self.dtype) for _ in range(self.n_streams)]
        return d

    def _create(self, lib, ctx):
        h = ctypes.c_void_p()
        lib.check(lib.dll.ry_outgate_bank_create(ctx.handle, self.n_streams, self.chunk, self.threshold_db, self.scale, int(self.dtype == numpy.float32),
                                                 ctypes.byref(h)))
        return h

    def push(self, waves) -> list:
        waves = list(waves)
        if len(waves) != self.n_streams:
            raise ValueError('%d waves for %d streams' % (len(waves), self.n_streams))
        xs = [_samples(w) if w is not None else numpy.empty(0, numpy.float64) for w in waves]
        if self._host is not None:
            res = [g.push(x) if x.size else (None, (False, False, 0.0)) for g, x in zip(self._host, xs)]
            self.last = [r[1] for r in res]
            return [r[0] for r in res]
        B = self.n_streams
        off = numpy.zeros(B + 1, numpy.int64)
        numpy.cumsum([x.size for x in xs], out=off[1:])
        x = numpy.ascontiguousarray(numpy.concatenate(xs))
        return self._push(x.ctypes.data_as(_DP), off, 0)

    def on_device(self, ctx=None) -> bool:
        """As `OutputGate.on_device`."""
        if self._host is not None:
            return False
        self._get()
        return ctx is None or self._ctx is ctx

    def push_device(self, ptr: int, offsets) -> list:
        """`push` of samples that are on the card: stream b's are the float64 samples [offsets[b], offsets[b + 1]) behind address `ptr`
        (`n_streams + 1` offsets on the host, starting at 0) -- where `StreamBank.push_device` left them.  Returns what `push` returns and sets
        `last` the same way; a stream without a sample sits the call out.  No device form on the host fallback."""
        if self._host is not None:
            raise ValueError('a chunk of %d samples is judged on the host: no device form below %d' % (self.chunk, MIN_DEVICE_CHUNK))
        off = numpy.ascontiguousarray(offsets, dtype=numpy.int64).reshape(-1)
        if off.size != self.n_streams + 1 or off[0] != 0 or (numpy.diff(off) < 0).any():
            raise ValueError('offsets %s for %d streams' % (off.tolist(), self.n_streams))
        if off[-1] > 0 and not ptr:
            raise ValueError('%d samples at address %r' % (int(off[-1]), ptr))
        return self._push(ctypes.cast(ctypes.c_void_p(int(ptr or 0)), _DP), off, 1)

    def _push(self, samples, off, on_device):
        B = self.n_streams
        self.last = [(False, False, 0.0)] * B
        if off[B] == 0:
            return [None] * B
        lib, h = self._get()
        out = numpy.empty(B * self.chunk, self.dtype)
        out_off = numpy.zeros(B + 1, numpy.int64)
        silent, mean = numpy.zeros(B, numpy.int32), numpy.zeros(B, numpy.float64)
        LLP = ctypes.POINTER(ctypes.c_longlong)
        lib.check(lib.dll.ry_outgate_bank_push(h, samples, off.ctypes.data_as(LLP), on_device, out.ctypes.data_as(ctypes.c_void_p), out.size,
                                               out_off.ctypes.data_as(LLP), silent.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), mean.ctypes.data_as(_DP)))
        self.last = [(int(s) >= 0, int(s) == 1, float(m)) for s, m in zip(silent, mean)]
        return [out[out_off[b]:out_off[b + 1]].copy() if silent[b] == 0 else None for b in range(B)]

    def held(self, stream: int) -> int:
        if self._host is not None:
            return len(self._host[stream].fragment)
        lib, h = self._get()
        n = int(lib.dll.ry_outgate_bank_held(h, int(stream)))
        if n < 0:
            lib.check(n)
        return n

    def reset(self, stream: int = -1) -> None:
        if self._host is not None:
            for g in (self._host if stream < 0 else [self._host[stream]]):
                g.fragment = numpy.empty(0, numpy.float64)
            return
        lib, h = self._get()
        lib.check(lib.dll.ry_outgate_bank_reset(h, int(stream)))

    def counts(self) -> dict:
        lib, h = self._get()
        c = (ctypes.c_longlong * 5)()
        lib.check(lib.dll.ry_outgate_bank_debug_counts(h, c))
        d = dict(zip(('waits', 'launches', 'uploads', 'downloads', 'sample_bytes_down'), (int(v) for v in c)))
        d['upload_bytes'] = int(lib.dll.ry_outgate_bank_debug_upload_bytes(h))
        return d

    def poison(self) -> None:
        lib, h = self._get()
        lib.check(lib.dll.ry_outgate_bank_debug_poison(h))
