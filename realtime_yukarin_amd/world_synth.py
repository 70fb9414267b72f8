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
of stage 2 and is materialised).  f0 goes in through the host; the float64 wave comes out through the host, or -- `push_device` /
`flush_device` / `StreamBank.push_device` -- stays on the card in a `SampleBlock` of the caller's, where `output_gate` reads it."""
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
# ... and `StreamBank.push`: 'bank_in_place' / 'bank_packed' -- ONE `ry_synth_bank_push` --, 'bank_fallback' (one bank push per item, the other
# streams sitting out)
calls = {'in_place': 0, 'packed': 0, 'fallback': 0, 'bank_in_place': 0, 'bank_packed': 0, 'bank_fallback': 0}


def cheaptrick_fft_size(fs, f0_floor: float = 71.0) -> int:
    return int(2 ** (1 + int(numpy.log2(3.0 * fs / f0_floor + 1))))


class DeviceRows(object):
    """`[frames][513]` float32 rows that are already on the GPU of the synthesizer's context (e.g. a stage-2 output left there)."""

    def __init__(self, address: int, frames: int, keep=None):
        self.address, self.frames, self.keep = int(address), int(frames), keep
        self.shape = (self.frames, BINS)


class SampleBlock(object):
    """Room for `samples` float64 samples on the GPU of the synthesizer's context, at `address`: where `Synthesizer.push_device` /
    `flush_device` / `StreamBank.push_device` leave their samples and `OutputGate.push_device` reads them."""

    def __init__(self, address: int, samples: int, keep=None):
        self.address, self.samples, self.keep = int(address), int(samples), keep

    def at(self, k: int) -> int:
        """The address of sample k."""
        return self.address + 8 * int(k)


def _block_room(block: SampleBlock, at: int):
    at = int(at)
    if at < 0 or at > block.samples:
        raise ValueError('sample %d of a block of %d' % (at, block.samples))
    return ctypes.cast(ctypes.c_void_p(block.at(at)), _DP), block.samples - at


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

    def push_device(self, f0, sp, ap, block: SampleBlock, at: int = 0) -> int:
        """`push` with the samples left on the card: they are written at sample `at` of `block` (room for `bound` samples behind it) by the
        overlap-add kernel itself -> how many (`ry_synth_push_dev`).  Nothing comes down and nothing is waited for beyond the scan's own
        waits; a reader on the context stream (`OutputGate.push_device`) finds them in order."""
        lib, h = self._get()
        f0, n, psp, pap, bins, dev, keep = self._frames(f0, sp, ap)
        y, room = _block_room(block, at)
        got = ctypes.c_longlong()
        lib.check(lib.dll.ry_synth_push_dev(h, f0.ctypes.data_as(_DP), psp, pap, n, bins, dev, y, room, ctypes.byref(got)))
        return int(got.value)

    def flush_device(self, block: SampleBlock, at: int = 0) -> int:
        """`flush` with the samples left on the card at sample `at` of `block` -> how many (`ry_synth_flush_dev`); `at` = what the push before
        returned puts push and flush back to back."""
        lib, h = self._get()
        y, room = _block_room(block, at)
        got = ctypes.c_longlong()
        lib.check(lib.dll.ry_synth_flush_dev(h, y, room, ctypes.byref(got)))
        return int(got.value)

    def bound(self, n: int, final: bool = False) -> int:
        """Samples a push of `n` frames (final: with the flush behind it) may return (`ry_synth_bound`)."""
        lib, h = self._get()
        return int(lib.dll.ry_synth_bound(h, max(int(n), 0), int(bool(final))))

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


class StreamBank(DeviceHandle):
    """B independent synthesis streams at one rate and one frame period, each with its own seed, advanced by ONE device call per buffer
    (`ry_synth_bank_*`): what `Synthesizer.push` / `flush` are for one session, for the sessions of a process.  Stream b returns, call by call,
    the bits a lone `Synthesizer(fs, frame_period, seed=seeds[b])` returns for the same frames in the same cuts, whatever the other streams do.
    `seeds=None`: every stream has RY_SYNTH_SEED, as the synthesizers of the drop-in bodies."""

    def __init__(self, fs: int, frame_period: float = 5.0, n_streams: int = 1, seeds=None, ctx=None, device: Optional[int] = None,
                 fft_size: Optional[int] = None):
        self.fs, self.frame_period, self.n_streams = int(fs), float(frame_period), int(n_streams)
        if seeds is None:
            seeds = [int(os.environ.get('RY_SYNTH_SEED', '0'))] * self.n_streams
        self.seeds = [int(v) & 0xffffffff for v in seeds]
        if len(self.seeds) != self.n_streams:
            raise ValueError('%d seeds for %d streams' % (len(self.seeds), self.n_streams))
        self.fft_size = int(fft_size) if fft_size else cheaptrick_fft_size(self.fs)
        DeviceHandle.__init__(self, ctx, device)

    _destroy = 'ry_synth_bank_destroy'
    _rows = staticmethod(Synthesizer._rows)
    _item = Synthesizer._item

    def _create(self, lib, ctx):
        h = ctypes.c_void_p()
        seeds = (ctypes.c_uint * max(self.n_streams, 1))(*self.seeds)
        lib.check(lib.dll.ry_synth_bank_create(ctx.handle, self.fs, self.frame_period, self.fft_size, self.n_streams, seeds, ctypes.byref(h)))
        return h

    def bound(self, stream: int, n: int, final: bool = False) -> int:
        lib, h = self._get()
        return int(lib.dll.ry_synth_bank_bound(h, int(stream), int(n), int(bool(final))))

    def _call(self, entries, final, in_place, block=None, at=0):
        """One `ry_synth_bank_push`: `entries` {stream: (f0, sp, ap)} with all rows on the host, or all on the card and consecutive.  block (a
        `SampleBlock`): one `ry_synth_bank_push_dev` that leaves the samples at sample `at` of it -> the offsets int64 [B + 1] from there."""
        lib, h = self._get()
        B = self.n_streams
        order = sorted(entries)
        n = numpy.zeros(B, numpy.int32)
        fin = numpy.zeros(B, numpy.int32)
        for b in order:
            n[b] = entries[b][0].size
        fin[list(final)] = 1
        if order:
            f0 = numpy.ascontiguousarray(numpy.concatenate([entries[b][0] for b in order]))
        else:                                                      # a plain flush: nothing is read
            f0 = numpy.zeros(1)
        if in_place:
            keep = entries
            psp, pap = _lib._fptr(entries[order[0]][1].address), _lib._fptr(entries[order[0]][2].address)
        elif order:
            keep = (numpy.concatenate([entries[b][1] for b in order]), numpy.concatenate([entries[b][2] for b in order]))
            psp, pap = _lib._fptr(keep[0]), _lib._fptr(keep[1])
        else:
            keep = (numpy.zeros((1, BINS), numpy.float32),) * 2
            psp, pap = _lib._fptr(keep[0]), _lib._fptr(keep[1])
        cap = sum(self.bound(b, int(n[b]), bool(fin[b])) for b in range(B) if n[b] > 0 or fin[b])
        off = numpy.zeros(B + 1, numpy.int64)
        ip = ctypes.POINTER(ctypes.c_int)
        if block is not None:
            y, room = _block_room(block, at)
            lib.check(lib.dll.ry_synth_bank_push_dev(h, f0.ctypes.data_as(_DP), psp, pap, n.ctypes.data_as(ip), fin.ctypes.data_as(ip), BINS,
                                                     int(in_place), y, room, off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
            del keep
            return off
        y = numpy.empty(max(cap, 1), numpy.float64)
        lib.check(lib.dll.ry_synth_bank_push(h, f0.ctypes.data_as(_DP), psp, pap, n.ctypes.data_as(ip), fin.ctypes.data_as(ip), BINS, int(in_place),
                                             y.ctypes.data_as(_DP), cap, off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        del keep
        return [y[off[b]:off[b + 1]].copy() for b in range(B)]

    def _entries(self, items, final):
        """The arguments of `push` / `push_device` -> ({stream: (f0, sp, ap, on_device)} of the streams with frames, `final` sorted, whether the
        rows are read in place, whether the list runs as ONE call)."""
        items = list(items)
        if len(items) != self.n_streams:
            raise ValueError('%d items for %d streams' % (len(items), self.n_streams))
        final = sorted(set(int(b) for b in final))
        if any(b < 0 or b >= self.n_streams for b in final):
            raise ValueError('final names stream %s of %d' % (final, self.n_streams))
        ent = {b: self._item(*it) for b, it in enumerate(items) if it is not None}
        ent = {b: it for b, it in ent.items() if it[0].size > 0}
        for f0, sp, ap, dev in ent.values():
            if dev is False and (sp.shape[1] != BINS or ap.shape[1] != BINS):
                raise ValueError('%d bins per frame, %d expected' % (sp.shape[1], BINS))
        if not ent and not final:
            raise ValueError('no stream has a frame or ends')
        order = sorted(ent)
        kinds = set(ent[b][3] for b in order)
        row = BINS * 4
        in_place = kinds == {True} and all(ent[b][k].address == ent[a][k].address + ent[a][k].frames * row for a, b in zip(order, order[1:]) for k in (1, 2))
        return ent, final, in_place, in_place or kinds <= {False}

    def push_device(self, items, final, block: SampleBlock) -> numpy.ndarray:
        """`push` with the samples left on the card: stream b's lie at samples [offsets[b], offsets[b + 1]) of `block`, back to back -- what
        `OutputGateBank.push_device` reads -> offsets int64 [B + 1].  `block` holds the sum of `bound` over the streams that take part.  A list
        that `push` runs item by item runs here as one `ry_synth_bank_push_dev` per stream, in stream order, each behind the one before."""
        ent, final, in_place, one_call = self._entries(items, final)
        self._kept_pulses = None
        if one_call:
            off = self._call(ent, final, in_place, block)
            calls['bank_in_place' if in_place else 'bank_packed'] += 1
            return off
        calls['bank_fallback'] += 1
        off, kept = numpy.zeros(self.n_streams + 1, numpy.int64), {}
        for b in range(self.n_streams):
            off[b + 1] = off[b]
            if b not in ent and b not in final:
                continue
            one, dev = {}, False
            if b in ent:
                f0, sp, ap, dev = ent[b]
                if dev is None:                                    # one of each: bring the host side over
                    sp = sp if isinstance(sp, DeviceRows) else _upload(self._get_ctx(), self._rows(sp, f0.size, 'sp')[2])
                    ap = ap if isinstance(ap, DeviceRows) else _upload(self._get_ctx(), self._rows(ap, f0.size, 'ap')[2])
                    dev = True
                one = {b: (f0, sp, ap)}
            off[b + 1] += self._call(one, [b] if b in final else [], dev, block, int(off[b]))[self.n_streams]
            kept[b] = self.pulses(b)                               # the next call reuses the pulse arrays
        self._kept_pulses = kept
        return off

    def push(self, items, final=()) -> list:
        """`items`: a list of length B of `(f0, sp, ap)` or None (the stream sits the call out); `final`: the streams whose signal ends with this
        call (everything left comes back and the slot starts a new signal with its next frames).  -> B float64 arrays, empty for a stream that
        sat out.  Host rows go up in one packed upload, `DeviceRows` that are consecutive slices of one buffer are read where they are -- one
        `ry_synth_bank_push` either way; any other list runs as one bank push per item with the other streams sitting out: the same bits."""
        ent, final, in_place, one_call = self._entries(items, final)
        order = sorted(ent)
        self._kept_pulses = None
        if one_call:
            out = self._call(ent, final, in_place)
            calls['bank_in_place' if in_place else 'bank_packed'] += 1
            return out
        calls['bank_fallback'] += 1
        out = [numpy.empty(0, numpy.float64) for _ in range(self.n_streams)]
        kept = {}
        for b in order:
            f0, sp, ap, dev = ent[b]
            if dev is None:                                        # one of each: bring the host side over
                sp = sp if isinstance(sp, DeviceRows) else _upload(self._get_ctx(), self._rows(sp, f0.size, 'sp')[2])
                ap = ap if isinstance(ap, DeviceRows) else _upload(self._get_ctx(), self._rows(ap, f0.size, 'ap')[2])
                dev = True
            out[b] = self._call({b: (f0, sp, ap)}, [b] if b in final else [], dev)[b]
            kept[b] = self.pulses(b)                               # the next call reuses the pulse arrays
        rest = [b for b in final if b not in ent]
        if rest:
            got = self._call({}, rest, False)
            for b in rest:
                out[b] = got[b]
                kept[b] = self.pulses(b)
        self._kept_pulses = kept
        return out

    def _get_ctx(self):
        self._get()
        return self._ctx

    def flush(self, streams) -> list:
        """Ends the signals of `streams`: what is left of each (a list of B arrays, empty for the others); their slots start anew."""
        return self.push([None] * self.n_streams, final=streams)

    def reset(self, stream=None) -> None:
        lib, h = self._get()
        lib.check(lib.dll.ry_synth_bank_reset(h, -1 if stream is None else int(stream)))

    def pulses(self, stream: int):
        """(index, shift, voiced) of the pulses the last push found for `stream`, as `Synthesizer.pulses` (`ry_synth_bank_debug_pulses`)."""
        lib, h = self._get()
        kept = getattr(self, '_kept_pulses', None)
        if kept is not None:                                       # the last push ran item by item
            return kept.get(int(stream), (numpy.empty(0, numpy.int64), numpy.empty(0, numpy.float64), numpy.empty(0, bool)))
        n = ctypes.c_int()
        lib.check(lib.dll.ry_synth_bank_debug_pulses(h, int(stream), None, None, None, 0, ctypes.byref(n)))
        idx, sh, vo = numpy.empty(n.value, numpy.int64), numpy.empty(n.value, numpy.float64), numpy.empty(n.value, numpy.int32)
        lib.check(lib.dll.ry_synth_bank_debug_pulses(h, int(stream), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), sh.ctypes.data_as(_DP),
                                                     vo.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n.value, ctypes.byref(n)))
        return idx, sh, vo != 0

    def poison(self) -> None:
        lib, h = self._get()
        self._kept_pulses = None
        lib.check(lib.dll.ry_synth_bank_debug_poison(h))

    def counts(self) -> dict:
        """Stream waits, kernel launches and host <-> device copies of the last push (`ry_synth_bank_debug_counts`)."""
        lib, h = self._get()
        c = (ctypes.c_int * 4)()
        lib.check(lib.dll.ry_synth_bank_debug_counts(h, c))
        return dict(zip(('waits', 'launches', 'h2d', 'd2h'), (int(v) for v in c)))

    def rows(self, stream: int) -> int:
        """Window rows kept for `stream` (`ry_synth_bank_debug_rows`)."""
        lib, h = self._get()
        return int(lib.dll.ry_synth_bank_debug_rows(h, int(stream)))


class BankSlot(object):
    """One stream of a `StreamBank`, with the `push` of a `Synthesizer`: what `create_synthesizer_many` gives a `RealtimeVocoder`."""

    def __init__(self, bank: StreamBank, slot: int):
        self.bank, self.slot = bank, int(slot)

    def _alone(self, item):
        items = [None] * self.bank.n_streams
        items[self.slot] = item
        return items

    def push(self, f0, sp, ap) -> numpy.ndarray:
        return self.bank.push(self._alone((f0, sp, ap)))[self.slot]

    def flush(self) -> numpy.ndarray:
        return self.bank.flush([self.slot])[self.slot]

    def reset(self) -> None:
        self.bank.reset(self.slot)


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
    """Drop-in body of `RealtimeVocoder.decode` (vocoder.py:89-120): the frames go to the stream, the samples that are final come back.  A
    vocoder that holds a slot of a bank (`create_synthesizer_many`) pushes that slot alone."""
    from yukarin import Wave
    assert self._synthesizer is not None
    f = acoustic_feature
    out = self._synthesizer.push(numpy.asarray(f.f0).ravel(), f.sp, f.ap)
    return Wave(wave=out, sampling_rate=self.out_sampling_rate)


def create_synthesizer_many(vocoders, buffer_size: int, number_of_pointers: int) -> StreamBank:
    """`create_synthesizer` for a list of `RealtimeVocoder` objects that one process serves: they get the slots of ONE `StreamBank`, so that
    `decode_realtime_many` advances all of them in one device call.  They share the sampling rate and the frame period."""
    vocoders = list(vocoders)
    if not vocoders:
        raise ValueError('no vocoder')
    fs, fp = vocoders[0].out_sampling_rate, vocoders[0].acoustic_param.frame_period
    if any(v.out_sampling_rate != fs or v.acoustic_param.frame_period != fp for v in vocoders):
        raise ValueError('the vocoders of one bank share the sampling rate and the frame period')
    assert all(v._synthesizer is None for v in vocoders)
    bank = StreamBank(fs, fp, n_streams=len(vocoders), ctx=engine_for_tests.ctx)
    bank.buffer_size, bank.number_of_pointers = int(buffer_size), int(number_of_pointers)
    for i, v in enumerate(vocoders):
        v._synthesizer = BankSlot(bank, i)
    return bank


def decode_realtime_many(vocoders, features):
    """The list form of `decode_realtime` for vocoders that hold the slots of one bank (`create_synthesizer_many`): one feature per vocoder, None
    for a vocoder that sits the call out (it gets an empty `Wave`) -> the `Wave`s, each equal to `decode_realtime` of its feature bit for bit."""
    from yukarin import Wave
    vocoders, features = list(vocoders), list(features)
    if len(vocoders) != len(features):
        raise ValueError('%d features for %d vocoders' % (len(features), len(vocoders)))
    if not vocoders:
        return []
    slots = [v._synthesizer for v in vocoders]
    if not all(isinstance(s, BankSlot) and s.bank is slots[0].bank for s in slots) or len(set(s.slot for s in slots)) != len(slots):
        raise ValueError('the vocoders do not hold distinct slots of one bank (create_synthesizer_many)')
    bank = slots[0].bank
    items = [None] * bank.n_streams
    for s, f in zip(slots, features):
        if f is not None:
            items[s.slot] = (numpy.asarray(f.f0).ravel(), f.sp, f.ap)
    outs = bank.push(items)
    return [Wave(wave=outs[s.slot], sampling_rate=v.out_sampling_rate) for s, v in zip(slots, vocoders)]
