"""WORLD analysis on the MI355X, the half that feeds the networks: `Analyzer`, the handle over `ry_analysis_*` (include/ry355.h) --
CheapTrick (spectral envelope) and sp2mc (the mel-cepstrum made from it) -- and `extract`, a drop-in body of the reference's
`AcousticFeature.extract` (yukarin's acoustic_feature.py, reached from `Vocoder.encode`, realtime_voice_conversion/yukarin_wrapper/vocoder.py:28-48):

    from realtime_yukarin_amd import world_analysis
    AcousticFeature.extract = classmethod(world_analysis.extract)

`pyworld` / `pysptk` are never imported for `sp` and `mc`.  The arithmetic is WORLD's CheapTrick and SPTK's sp2mc restated
(tests/world_analysis_ref.py); parity at the `pyworld` / `pysptk` boundary is unpinned: neither package can be installed
where this was built.  The one deliberate deviation from `pyworld`: WORLD's two `randn()` terms (1e-12 on the windowed wave, eps |randn| on the
power spectrum) are counter-based functions of (seed, centre sample of the frame, index) instead of draws from a process-global sequence, so a
frame's rows depend on (x, f0, t, seed) only and not on which other frames share the call.

D4C (`ap`, `coded_ap`) is on the device too (`Analyzer.d4c`, `d4c`, `code_aperiodicity`; restated in tests/world_d4c_ref.py, the same counter-based
noise with keys of its own), but `extract` takes it only when asked to: `ap` / `coded_ap` come from `aperiodicity`, a module-level callable whose
default still tries `pyworld` and otherwise raises `NotImplementedError`.  The device path is opted into with

    world_analysis.aperiodicity = world_analysis.device_aperiodicity

after which `extract` makes one `Analyzer.run` for sp, mc, ap and coded_ap (one upload of the wave).

Limits: fft_size 1024 only (16 and 24 kHz), for D4C as well."""
import ctypes
import os
from typing import Optional

import numpy

from . import _lib, sptk
from ._handle import _DP, DeviceHandle, EngineForTests, _dptr
from .world_synth import BINS, FFT_SIZE, DeviceRows, _DeviceBuffer, cheaptrick_fft_size

_LLP = ctypes.POINTER(ctypes.c_longlong)


def harvest_frames(n_samples: int, fs, frame_period) -> int:
    """The frames `pyworld.harvest` returns for n_samples at fs: `int(1000 * n / fs / frame_period) + 1`.  Restated from memory of WORLD's
    GetSamplesForHarvest and unpinned like the rest of the `pyworld` boundary: the pipeline only ever compares it with what
    the f0 callable really returned and takes the composed path when they differ."""
    return int(1000.0 * int(n_samples) / fs / frame_period) + 1


def frame_times(n: int, frame_period) -> numpy.ndarray:
    """`t` of a WORLD f0 tracker for n frames: k * frame_period / 1000, two rounded float64 operations -- what `ry_analysis_ingest_tracks` writes."""
    return numpy.arange(int(n), dtype=numpy.float64) * float(frame_period) / 1000.0


class UploadedWaves(object):
    """What `Analyzer.upload_waves` left on the card: the address of the float32 waves (back to back) and `offsets` (int64, waves + 1 entries): where
    wave i starts.  Holds until the next `upload_waves` / `poison` of the analyzer."""

    def __init__(self, analyzer, ctx, wave, offsets):
        self.analyzer, self.ctx, self.wave, self.offsets = analyzer, ctx, wave, offsets
        self.waves, self.samples = offsets.size - 1, int(offsets[-1])


class WorldTracks(object):
    """What `Analyzer.ingest_tracks` left on the card for the waves `which` of an `UploadedWaves`, with the fields `pipeline` reads of a CREPE track:
    the addresses of the uploaded block `wave` (`samples` of it) and of the concatenated `voiced` (bytes), `f0` and `t` (float64) of the tracked
    waves; `frame_offsets` (int32, tracked + 1 entries) into them; `first_sample` / `n_samples` of every tracked wave in the block, and -- when every
    uploaded wave was tracked, so that waves and tracks correspond -- `sample_offsets` (int64, waves + 1 entries; else None).  They belong to the
    analyzer's handle and hold until its next `upload_waves` / `ingest_tracks` / `poison`."""

    def __init__(self, analyzer, ctx, uploaded, which, voiced, f0, t, frame_offsets):
        self.analyzer, self.ctx, self.which = analyzer, ctx, list(which)
        self.wave, self.samples = uploaded.wave, uploaded.samples
        self.first_sample = numpy.asarray([uploaded.offsets[i] for i in which], numpy.int64)
        self.n_samples = numpy.asarray([uploaded.offsets[i + 1] - uploaded.offsets[i] for i in which], numpy.int32)
        self.sample_offsets = uploaded.offsets if self.which == list(range(uploaded.waves)) else None
        self.voiced, self.f0, self.t, self.frame_offsets = voiced, f0, t, frame_offsets
        self.waves, self.frames = len(self.which), int(frame_offsets[-1])

    def download(self, t: bool = False):
        """[(voiced [frames] bool, f0 [frames] float64)] per tracked wave, read back from the card; t=True: [(voiced, f0, t)]."""
        n, ctx = self.frames, self.ctx
        words, f64, t64 = numpy.empty((n + 3) // 4, numpy.float32), numpy.empty(n, numpy.float64), numpy.empty(n, numpy.float64)
        ctx.dev_download(self.voiced, words)
        ctx.dev_download(self.f0, f64.view(numpy.float32))
        if t:
            ctx.dev_download(self.t, t64.view(numpy.float32))
        voiced, o = words.view(numpy.uint8)[:n].astype(bool), self.frame_offsets
        return [(voiced[o[i]:o[i + 1]], f64[o[i]:o[i + 1]]) + ((t64[o[i]:o[i + 1]],) if t else ()) for i in range(self.waves)]


class Analyzer(DeviceHandle):
    """CheapTrick + sp2mc on the device (`ry_analysis_*`): one workgroup per frame, stateless.  `ctx` (tests): a context over another build of
    the library."""

    def __init__(self, fs: int, fft_size: Optional[int] = None, order: int = 8, alpha: Optional[float] = None, q1: float = -0.15,
                 f0_floor: float = 71.0, seed: int = 0, ctx=None, device: Optional[int] = None):
        self.fs = int(fs)
        self.fft_size = int(fft_size) if fft_size else cheaptrick_fft_size(self.fs, f0_floor)
        self.order = int(order)
        self.alpha = float(sptk.mcepalpha(self.fs) if alpha is None else alpha)
        self.q1, self.f0_floor, self.seed = float(q1), float(f0_floor), int(seed) & 0xffffffff
        DeviceHandle.__init__(self, ctx, device)

    _destroy = 'ry_analysis_destroy'

    def _create(self, lib, ctx):
        h = ctypes.c_void_p()
        lib.check(lib.dll.ry_analysis_create(ctx.handle, self.fs, self.fft_size, self.order, self.alpha, self.q1, self.f0_floor, self.seed, ctypes.byref(h)))
        return h

    def bands(self) -> int:
        """The number of D4C bands at this rate (columns of `coded_ap`): 1 at 16 kHz, 3 at 24 kHz."""
        lib, h = self._get()
        b = lib.dll.ry_analysis_d4c_bands(h)
        if b < 0:
            lib.check(b)
        return b

    def run(self, x, f0, t, want=('sp', 'mc'), device_rows: bool = False, threshold: float = 0.85):
        """-> tuple in the order of `want`: 'sp' [frames][513] float64 (with device_rows: `DeviceRows`, the float32 rows left on the card),
        'mc' [frames][order + 1] float64, 'sp64' the float64 rows whatever `device_rows` says; D4C (`threshold`): 'ap' [frames][513] float64 (with
        device_rows: `DeviceRows`), 'ap64', 'coded_ap' [frames][bands] float64.  CheapTrick and D4C asked for together share one upload of the wave.
        No frames: empty arrays; frames but an empty wave: ValueError (the C ABI would succeed and write nothing, and the rows would no longer
        match `f0`)."""
        lib, h = self._get()
        self._check_want(want)
        x = numpy.ascontiguousarray(numpy.asarray(x, dtype=numpy.float64).reshape(-1))
        f0 = numpy.ascontiguousarray(numpy.asarray(f0, dtype=numpy.float64).reshape(-1))
        t = numpy.ascontiguousarray(numpy.asarray(t, dtype=numpy.float64).reshape(-1))
        if f0.size != t.size:
            raise ValueError('f0 has %d frames, t %d' % (f0.size, t.size))
        n = f0.size
        if n > 0 and x.size == 0:
            raise ValueError('an empty wave cannot be analysed at %d frames' % n)
        d4c = bool(set(want) & {'ap', 'ap64', 'coded_ap'})
        cheaptrick = bool(set(want) & {'sp', 'sp64', 'mc'}) or not d4c
        got, out_sp, out_ap = self._outputs(n, want, device_rows)
        head = (h, _dptr(x), x.size, _dptr(f0), _dptr(t), n)
        if not d4c:
            lib.check(lib.dll.ry_analysis_run(*(head + out_sp)))
        elif not cheaptrick:
            lib.check(lib.dll.ry_analysis_d4c(*(head + (float(threshold),) + out_ap)))
        else:
            lib.check(lib.dll.ry_analysis_extract(*(head + (float(threshold),) + out_sp + out_ap)))
        return tuple(got[k] for k in want)

    @staticmethod
    def _check_want(want) -> None:
        unknown = set(want) - {'sp', 'mc', 'sp64', 'ap', 'ap64', 'coded_ap'}
        if unknown:
            raise ValueError('want: %s' % sorted(unknown))

    def _outputs(self, n: int, want, device_rows: bool):
        """The arrays of a call of n frames -> (what `want` names, the CheapTrick output arguments, the D4C output arguments)."""
        sp64 = numpy.empty((n, BINS), numpy.float64) if ('sp64' in want or ('sp' in want and not device_rows)) else None
        mc = numpy.empty((n, self.order + 1), numpy.float64) if 'mc' in want else None
        ap64 = numpy.empty((n, BINS), numpy.float64) if ('ap64' in want or ('ap' in want and not device_rows)) else None
        coded = numpy.empty((n, self.bands()), numpy.float64) if 'coded_ap' in want else None

        def device(key):
            if not (device_rows and key in want):
                return None
            buf = _DeviceBuffer(self._ctx, max(n, 1) * BINS)
            return DeviceRows(buf.address, n, keep=buf)
        rows, rows_ap = device('sp'), device('ap')
        got = {'sp': rows if device_rows else sp64, 'sp64': sp64, 'mc': mc, 'ap': rows_ap if device_rows else ap64, 'ap64': ap64, 'coded_ap': coded}
        out_sp = (_dptr(sp64), _lib._fptr(rows.address if rows else None), _dptr(mc))
        out_ap = (_dptr(ap64), _lib._fptr(rows_ap.address if rows_ap else None), _dptr(coded))
        return got, out_sp, out_ap

    def run_device(self, wave_dev: int, n_samples: int, f0_dev: int, t_dev: int, n: int, want=('sp', 'mc', 'ap', 'coded_ap'), device_rows: bool = False,
                   threshold: float = 0.85):
        """`run` on a wave and a track that are already on the card of this analyzer's context (`ry_analysis_extract_dev`): `wave_dev` the address
        of n_samples float32 samples (widened on the device: the bits of `run` on `wave.astype(float64)`), `f0_dev` / `t_dev` of n float64 entries --
        what `CrepeModel.track(..., device=True)` left there.  The same `want` keys and the same values as `run`; CheapTrick and D4C both run
        whatever `want` names.  A track `run` would refuse is refused here too (the device checks it; nothing is written)."""
        lib, h = self._get()
        self._check_want(want)
        n, n_samples = int(n), int(n_samples)
        if n > 0 and n_samples == 0:
            raise ValueError('an empty wave cannot be analysed at %d frames' % n)
        got, out_sp, out_ap = self._outputs(n, want, device_rows)
        as_d = lambda a: ctypes.cast(ctypes.c_void_p(a), _DP)
        lib.check(lib.dll.ry_analysis_extract_dev(h, _lib._fptr(int(wave_dev)), n_samples, as_d(f0_dev), as_d(t_dev), n, float(threshold), *(out_sp + out_ap)))
        return tuple(got[k] for k in want)

    def extract_resident(self, wave_dev: int, n_samples: int, f0_dev: int, t_dev: int, n: int, mc32_dev: int, sp32_dev: int, ap32_dev: int,
                         threshold: float = 0.85) -> None:
        """`run_device` with device outputs only (`ry_analysis_extract_resident`): float32 `mc` (n, order + 1), `sp` and `ap` (n, 513) rows written to
        the blocks at the three addresses -- the bits of `run_device(...)`'s float64 rows cast with `astype(float32)`.  Nothing but the verdict of the
        track check comes back to the host; a refused track raises and leaves the blocks untouched."""
        lib, h = self._get()
        n, n_samples = int(n), int(n_samples)
        if n > 0 and n_samples == 0:
            raise ValueError('an empty wave cannot be analysed at %d frames' % n)
        as_d = lambda a: ctypes.cast(ctypes.c_void_p(a), _DP)
        lib.check(lib.dll.ry_analysis_extract_resident(h, _lib._fptr(int(wave_dev)), n_samples, as_d(f0_dev), as_d(t_dev), n, float(threshold),
                                                       _lib._fptr(int(mc32_dev)), _lib._fptr(int(sp32_dev)), _lib._fptr(int(ap32_dev))))

    def run_device_many(self, wave_dev: int, sample_offsets, f0_dev: int, t_dev: int, frame_offsets, want=('sp', 'mc', 'ap', 'coded_ap'),
                        device_rows: bool = False, threshold: float = 0.85):
        """`run_device` on the waves and tracks `CrepeModel.track_many(..., device=True)` left on the card (`ry_analysis_extract_many_dev`): the waves
        back to back at `wave_dev`, the tracks back to back at `f0_dev` / `t_dev`, wave i at sample_offsets[i] / frame_offsets[i] (waves + 1 entries
        each, starting at 0).  One check of the whole track and one wait for its verdict; the rows of all waves come back concatenated in wave order
        -- the same `want` keys as `run`, rows of wave i with the bits of `run_device` on wave i alone."""
        lib, h = self._get()
        self._check_want(want)
        so = numpy.ascontiguousarray(sample_offsets, dtype=numpy.int64).ravel()
        fo = numpy.ascontiguousarray(frame_offsets, dtype=numpy.int32).ravel()
        if so.size != fo.size or so.size < 2:
            raise ValueError('run_device_many needs two offset arrays of waves + 1 >= 2 entries, got %d and %d' % (so.size, fo.size))
        got, out_sp, out_ap = self._outputs(max(int(fo[-1]), 0), want, device_rows)
        as_d = lambda a: ctypes.cast(ctypes.c_void_p(a), _DP)
        lib.check(lib.dll.ry_analysis_extract_many_dev(h, _lib._fptr(int(wave_dev)), so.ctypes.data_as(_LLP), as_d(f0_dev), as_d(t_dev),
                                                       fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), so.size - 1, float(threshold), *(out_sp + out_ap)))
        return tuple(got[k] for k in want)

    def extract_many_resident(self, wave_dev: int, sample_offsets, f0_dev: int, t_dev: int, frame_offsets, mc32_dev: int, sp32_dev: int, ap32_dev: int,
                              threshold: float = 0.85) -> None:
        """`run_device_many` with device outputs only (`ry_analysis_extract_many_resident`): float32 `mc` (sum n, order + 1), `sp` and `ap` (sum n, 513)
        rows in wave order at the three addresses; rows of wave i have the bits `extract_resident` writes for wave i alone.  One verdict comes back
        to the host; a refused call raises and leaves the blocks untouched."""
        lib, h = self._get()
        so = numpy.ascontiguousarray(sample_offsets, dtype=numpy.int64).ravel()
        fo = numpy.ascontiguousarray(frame_offsets, dtype=numpy.int32).ravel()
        if so.size != fo.size or so.size < 2:
            raise ValueError('extract_many_resident needs two offset arrays of waves + 1 >= 2 entries, got %d and %d' % (so.size, fo.size))
        as_d = lambda a: ctypes.cast(ctypes.c_void_p(a), _DP)
        lib.check(lib.dll.ry_analysis_extract_many_resident(h, _lib._fptr(int(wave_dev)), so.ctypes.data_as(_LLP), as_d(f0_dev), as_d(t_dev),
                                                            fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), so.size - 1, float(threshold),
                                                            _lib._fptr(int(mc32_dev)), _lib._fptr(int(sp32_dev)), _lib._fptr(int(ap32_dev))))

    def extract_spans_resident(self, wave_dev: int, samples: int, first_sample, n_samples, f0_dev: int, t_dev: int, frame_offsets, row_offsets,
                               mc32_dev: int, sp32_dev: int, ap32_dev: int, threshold: float = 0.85) -> None:
        """`extract_many_resident` for waves that lie anywhere in an uploaded block of `samples` samples (`first_sample` / `n_samples` per wave) and
        rows that go anywhere in the blocks (`row_offsets`: the first row of every wave; `frame_offsets`: waves + 1 entries, where its track starts)
        -- what `CrepeModel.track_uploaded` left, into the frame layout of a call with more waves than were tracked
        (`ry_analysis_extract_spans_resident`).  No other row of the blocks is written."""
        lib, h = self._get()
        fs = numpy.ascontiguousarray(first_sample, dtype=numpy.int64).ravel()
        ns = numpy.ascontiguousarray(n_samples, dtype=numpy.int32).ravel()
        fo = numpy.ascontiguousarray(frame_offsets, dtype=numpy.int32).ravel()
        ro = numpy.ascontiguousarray(row_offsets, dtype=numpy.int32).ravel()
        if not (fs.size == ns.size == ro.size == fo.size - 1 and fs.size >= 1):
            raise ValueError('extract_spans_resident needs one first sample, count and row offset per wave and waves + 1 frame offsets')
        as_d = lambda a: ctypes.cast(ctypes.c_void_p(a), _DP)
        ip = ctypes.POINTER(ctypes.c_int)
        lib.check(lib.dll.ry_analysis_extract_spans_resident(h, _lib._fptr(int(wave_dev)), int(samples), fs.ctypes.data_as(_LLP), ns.ctypes.data_as(ip),
                                                             as_d(f0_dev), as_d(t_dev), fo.ctypes.data_as(ip), ro.ctypes.data_as(ip), fs.size,
                                                             float(threshold), _lib._fptr(int(mc32_dev)), _lib._fptr(int(sp32_dev)),
                                                             _lib._fptr(int(ap32_dev))))

    def upload_waves(self, waves) -> UploadedWaves:
        """The one upload of a call whose f0 comes from the caller (`ry_analysis_upload_waves`): float32 waves back to back in a block of this
        analyzer's handle -- no CREPE model is involved.  What `extract_*_resident` and the gate entries of `VcCore` read."""
        xs = [numpy.ascontiguousarray(w, dtype=numpy.float32).ravel() for w in waves]
        if not xs:
            raise ValueError('upload_waves needs at least one wave')
        lib, h = self._get()
        counts = numpy.asarray([x.size for x in xs], numpy.int32)
        audio = numpy.ascontiguousarray(numpy.concatenate(xs))
        p = ctypes.c_void_p()
        lib.check(lib.dll.ry_analysis_upload_waves(h, _lib._fptr(audio), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(xs), ctypes.byref(p)))
        return UploadedWaves(self, self._ctx, p.value, numpy.concatenate([[0], numpy.cumsum(counts, dtype=numpy.int64)]).astype(numpy.int64))

    def ingest_tracks(self, f0s, frame_period, uploaded: UploadedWaves, which=None) -> WorldTracks:
        """The f0 tracks of a host tracker (one float64 array per wave of `which`, ascending indices into `uploaded`; None: every wave) onto the card
        in one upload and one launch (`ry_analysis_ingest_tracks`): `t = k * frame_period / 1000`, `voiced = f0 != 0` and f0 itself, per wave from its
        own first frame -- the bits of the call on that wave alone.  Nothing about the values is checked here; `extract_*_resident` refuses a track
        `run` would refuse."""
        which = list(range(uploaded.waves)) if which is None else [int(i) for i in which]
        tracks = [numpy.ascontiguousarray(numpy.asarray(f, dtype=numpy.float64).reshape(-1)) for f in f0s]
        if uploaded.analyzer is not self or not which or len(tracks) != len(which) or any(i < 0 or i >= uploaded.waves for i in which) \
                or any(b <= a for a, b in zip(which, which[1:])):
            raise ValueError('ingest_tracks needs one track per wave of ascending indices into an upload of this analyzer, got %d tracks for %s of %d'
                             % (len(tracks), which, uploaded.waves))
        lib, h = self._get()
        counts = numpy.asarray([f.size for f in tracks], numpy.int32)
        f0 = numpy.ascontiguousarray(numpy.concatenate(tracks))
        lib.check(lib.dll.ry_analysis_ingest_tracks(h, _dptr(f0), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(tracks), float(frame_period)))
        return self._tracks_on_card(uploaded, which)

    def _tracks_on_card(self, uploaded, which) -> WorldTracks:
        lib, h = self._get()
        p = [ctypes.c_void_p() for _ in range(4)]
        nw, nt = ctypes.c_int(), ctypes.c_int()
        so, fo = _LLP(), ctypes.POINTER(ctypes.c_int)()
        lib.check(lib.dll.ry_analysis_track_buffers(h, ctypes.byref(p[0]), ctypes.byref(nw), ctypes.byref(so), ctypes.byref(nt), ctypes.byref(fo),
                                                    *[ctypes.byref(q) for q in p[1:]]))
        assert nt.value == len(which) and p[0].value == uploaded.wave and nw.value == uploaded.waves, (nt.value, len(which), nw.value)
        frame_offsets = numpy.asarray(fo[:nt.value + 1], numpy.int32)           # a copy: the handle's array changes with its next call
        return WorldTracks(self, self._ctx, uploaded, which, p[1].value, p[2].value, p[3].value, frame_offsets)

    def d4c(self, x, f0, t, threshold: float = 0.85) -> numpy.ndarray:
        """`pyworld.d4c` of this analyzer's rate: -> aperiodicity [frames][513] float64."""
        return self.run(x, f0, t, want=('ap',), threshold=threshold)[0]

    def d4c_record(self):
        """tests: what the last D4C run after `record_integers()` decided -> (integers [frames][8] int64: half length of the Love-Train window, of the
        other windows, origins of the windows at t - 0.25 / f, t, t + 0.25 / f, DC-correction bin limit, smoothing boundaries of width f and f / 2;
        on [frames] bool; a0 [frames]; coarse dB [frames][bands])."""
        lib, h = self._get()
        n = ctypes.c_int()
        lib.check(lib.dll.ry_analysis_debug_d4c(h, None, None, 0, ctypes.byref(n)))
        ints, vals = numpy.empty((n.value, 9), numpy.int64), numpy.empty((n.value, 4), numpy.float64)
        lib.check(lib.dll.ry_analysis_debug_d4c(h, ints.ctypes.data_as(_LLP), _dptr(vals), n.value, ctypes.byref(n)))
        return ints[:, :8], ints[:, 8] != 0, vals[:, 0], vals[:, 1:1 + self.bands()]

    def sp2mc(self, sp) -> numpy.ndarray:
        """Mel-cepstrum of a spectrogram that comes from elsewhere: [frames][513] host rows (taken as float64) or `DeviceRows` (float32)."""
        lib, h = self._get()
        if isinstance(sp, DeviceRows):
            n, ptr, dev = sp.frames, ctypes.c_void_p(sp.address), 1
        else:
            sp = numpy.ascontiguousarray(numpy.atleast_2d(numpy.asarray(sp, dtype=numpy.float64)))
            if sp.shape[1] != BINS:
                raise ValueError('sp must be (frames, %d), got %s' % (BINS, sp.shape))
            n, ptr, dev = sp.shape[0], ctypes.c_void_p(sp.ctypes.data), 0
        mc = numpy.empty((n, self.order + 1), numpy.float64)
        lib.check(lib.dll.ry_analysis_sp2mc(h, ptr, n, dev, _dptr(mc)))
        return mc

    def record_integers(self, on: bool = True) -> None:
        """tests: later `run`s keep the integers they decide (`ry_analysis_debug_record`; off by default, one copy less per call)."""
        lib, h = self._get()
        lib.check(lib.dll.ry_analysis_debug_record(h, int(bool(on))))

    def integers(self) -> numpy.ndarray:
        """[frames][4] int64 of the last `run` after `record_integers()`: window half length, centre sample, DC-correction bin limit, smoothing
        boundary."""
        lib, h = self._get()
        n = ctypes.c_int()
        lib.check(lib.dll.ry_analysis_debug_ints(h, None, 0, ctypes.byref(n)))
        out = numpy.empty((n.value, 4), numpy.int64)
        lib.check(lib.dll.ry_analysis_debug_ints(h, out.ctypes.data_as(_LLP), n.value, ctypes.byref(n)))
        return out

    def poison(self) -> None:
        lib, h = self._get()
        lib.check(lib.dll.ry_analysis_debug_poison(h))


# ---- the packages' functions ---------------------------------------------------------------------------------------------------------
engine_for_tests = EngineForTests()           # for the analyzers the functions below create


_analyzers = {}


def _analyzer(fs, fft_size, order, alpha, q1=-0.15, f0_floor=71.0) -> Analyzer:
    ctx = engine_for_tests.ctx
    key = (os.getpid(), id(ctx), int(fs), fft_size, int(order), alpha, float(q1), float(f0_floor))
    a = _analyzers.get(key)
    if a is None:
        a = _analyzers[key] = Analyzer(fs, fft_size, order, alpha, q1, f0_floor, seed=int(os.environ.get('RY_ANALYSIS_SEED', '0')), ctx=ctx)
    return a


def cheaptrick(x, f0, temporal_positions, fs, q1=-0.15, f0_floor=71.0, fft_size=None):
    """`pyworld.cheaptrick`: -> spectrogram [frames][fft_size / 2 + 1] float64."""
    return _analyzer(fs, fft_size, 0, 0.0, q1, f0_floor).run(x, f0, temporal_positions, want=('sp',))[0]


def sp2mc(sp, order, alpha):
    """`pysptk.sp2mc`: power spectrogram [frames][513] (or one row) -> mel-cepstrum [frames][order + 1] float64."""
    sp = numpy.asarray(sp, dtype=numpy.float64)
    mc = _analyzer(16000, FFT_SIZE, order, float(alpha)).sp2mc(sp)               # sp2mc does not depend on the sampling rate
    return mc[0] if sp.ndim == 1 else mc


def aperiodicity(x, f0, t, fs, fft_size):
    """(ap, coded_ap) of the frames.  This default hands D4C to `pyworld` where that package exists; assign another callable of the same
    signature to `world_analysis.aperiodicity` to replace it -- `device_aperiodicity` for D4C on the device."""
    try:
        import pyworld
        ap = pyworld.d4c(x, f0, t, fs, fft_size=fft_size)
        return ap, pyworld.code_aperiodicity(ap, fs)
    except (ImportError, NotImplementedError) as e:
        raise NotImplementedError('aperiodicity: D4C (WORLD\'s band aperiodicity) is not built on the device yet and `pyworld` is not usable here; '
                                  'assign a callable (x, f0, t, fs, fft_size) -> (ap, coded_ap) to world_analysis.aperiodicity') from e


def d4c(x, f0, temporal_positions, fs, threshold=0.85, fft_size=None):
    """`pyworld.d4c`: -> aperiodicity [frames][fft_size / 2 + 1] float64 (fft_size 1024 only)."""
    return _analyzer(fs, fft_size, 0, 0.0).d4c(x, f0, temporal_positions, threshold)


def code_aperiodicity(ap, fs):
    """`pyworld.code_aperiodicity`: aperiodicity [frames][513] -> its dB values at 3000 i Hz, [frames][bands] float64.  A read of the columns
    that are those frequencies (bins 192 i at 16 kHz, 128 i at 24 kHz): host arithmetic, no kernel."""
    ap = numpy.atleast_2d(numpy.asarray(ap, dtype=numpy.float64))
    if ap.shape[1] != BINS:
        raise ValueError('ap must be (frames, %d), got %s' % (BINS, ap.shape))
    fs = int(fs)
    bands = int(min(15000.0, fs / 2.0 - 3000.0) / 3000.0)
    if bands < 1 or (3000 * FFT_SIZE) % fs:
        raise ValueError('code_aperiodicity at %d Hz: built for the rates whose band centres are bins of the row (16 and 24 kHz)' % fs)
    return 20.0 * numpy.log10(ap[:, [3000 * i * FFT_SIZE // fs for i in range(1, bands + 1)]])


def device_aperiodicity(x, f0, t, fs, fft_size):
    """(ap, coded_ap) of the frames from the device: assign it to `world_analysis.aperiodicity` to take D4C from the card."""
    ap, coded = _analyzer(fs, fft_size, 0, 0.0).run(x, f0, t, want=('ap', 'coded_ap'))
    return ap, coded


def extract(cls, wave, frame_period, f0_floor, f0_ceil, fft_length, order, alpha, dtype):
    """Drop-in body of `AcousticFeature.extract`: f0 from `cls.extract_f0` (so a bound CREPE wrapper keeps working), `sp` / `mc` from the
    device, `ap` / `coded_ap` from `world_analysis.aperiodicity` (when that is `device_aperiodicity`: all four from one `Analyzer.run`).
    Returns the plain `AcousticFeature` container whatever `cls` is, like the original."""
    x = wave.wave.astype(numpy.float64)
    fs = wave.sampling_rate
    f0, t = cls.extract_f0(x=x, fs=fs, frame_period=frame_period, f0_floor=f0_floor, f0_ceil=f0_ceil)
    f0, t = numpy.asarray(f0, numpy.float64), numpy.asarray(t, numpy.float64)
    fft_size = int(fft_length) if fft_length else cheaptrick_fft_size(fs)
    if aperiodicity is device_aperiodicity:
        sp, mc, ap, coded_ap = _analyzer(fs, fft_size, order, float(alpha)).run(x, f0, t, want=('sp', 'mc', 'ap', 'coded_ap'))
    else:
        sp, mc = _analyzer(fs, fft_size, order, float(alpha)).run(x, f0, t, want=('sp', 'mc'))
        ap, coded_ap = aperiodicity(x, f0, t, fs, fft_size)
    voiced = ~(f0 == 0)
    # the plain container, as the body this replaces builds it: `cls` may be a wrapper whose constructor takes more (the reference's
    # AcousticFeatureWrapper needs `wave` and builds itself from this result's __dict__)
    container = next(k for k in cls.__mro__ if 'astype_only_float' in vars(k))
    feature = container(f0=f0[:, None], sp=sp, ap=ap, coded_ap=coded_ap, mc=mc, voiced=voiced[:, None])
    feature = feature.astype_only_float(dtype)
    feature.validate()
    return feature
