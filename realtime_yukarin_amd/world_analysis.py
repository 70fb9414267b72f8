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

Limits: fft_size 1024 only (16 and 24 kHz); D4C is NOT built -- `ap` / `coded_ap` come from `aperiodicity`, a module-level callable whose
default tries `pyworld` and otherwise raises `NotImplementedError`."""
import ctypes
import os
from typing import Optional

import numpy

from . import _lib, sptk
from .world_synth import BINS, FFT_SIZE, DeviceRows, _DeviceBuffer, cheaptrick_fft_size

_DP = ctypes.POINTER(ctypes.c_double)
_LLP = ctypes.POINTER(ctypes.c_longlong)


def _dptr(a):
    return a.ctypes.data_as(_DP) if a is not None else ctypes.cast(ctypes.c_void_p(0), _DP)


class Analyzer(object):
    """CheapTrick + sp2mc on the device (`ry_analysis_*`): one workgroup per frame, stateless.  `ctx` (tests): a context over another build of
    the library."""

    def __init__(self, fs: int, fft_size: Optional[int] = None, order: int = 8, alpha: Optional[float] = None, q1: float = -0.15,
                 f0_floor: float = 71.0, seed: int = 0, ctx=None, device: Optional[int] = None):
        self.fs = int(fs)
        self.fft_size = int(fft_size) if fft_size else cheaptrick_fft_size(self.fs, f0_floor)
        self.order = int(order)
        self.alpha = float(sptk.mcepalpha(self.fs) if alpha is None else alpha)
        self.q1, self.f0_floor, self.seed = float(q1), float(f0_floor), int(seed) & 0xffffffff
        self.device = int(os.environ.get('RY_DEVICE', '0')) if device is None else int(device)
        self._given_ctx = ctx
        self._ctx = None
        self._handle = None
        self._pid = None

    def __getstate__(self):
        d = dict(self.__dict__)
        d.update(_handle=None, _pid=None, _ctx=None, _given_ctx=None)
        return d

    def _get(self):
        if self._handle is None or self._pid != os.getpid():
            from . import engine
            given = self._given_ctx is not None and self._given_ctx.pid == os.getpid()
            self._ctx = self._given_ctx if given else engine.get_context(self.device)
            lib = self._ctx.lib
            h = ctypes.c_void_p()
            lib.check(lib.dll.ry_analysis_create(self._ctx.handle, self.fs, self.fft_size, self.order, self.alpha, self.q1, self.f0_floor, self.seed,
                                                 ctypes.byref(h)))
            self._handle, self._pid = h, os.getpid()
        return self._ctx.lib, self._handle

    def run(self, x, f0, t, want=('sp', 'mc'), device_rows: bool = False):
        """-> tuple in the order of `want`: 'sp' [frames][513] float64 (with device_rows: `DeviceRows`, the float32 rows left on the card),
        'mc' [frames][order + 1] float64, 'sp64' the float64 rows whatever `device_rows` says.  No frames: empty arrays; frames but an empty wave:
        ValueError (the C ABI would succeed and write nothing, and the rows would no longer match `f0`)."""
        lib, h = self._get()
        unknown = set(want) - {'sp', 'mc', 'sp64'}
        if unknown:
            raise ValueError('want: %s' % sorted(unknown))
        x = numpy.ascontiguousarray(numpy.asarray(x, dtype=numpy.float64).reshape(-1))
        f0 = numpy.ascontiguousarray(numpy.asarray(f0, dtype=numpy.float64).reshape(-1))
        t = numpy.ascontiguousarray(numpy.asarray(t, dtype=numpy.float64).reshape(-1))
        if f0.size != t.size:
            raise ValueError('f0 has %d frames, t %d' % (f0.size, t.size))
        n = f0.size
        if n > 0 and x.size == 0:
            raise ValueError('an empty wave cannot be analysed at %d frames' % n)
        sp64 = numpy.empty((n, BINS), numpy.float64) if ('sp64' in want or ('sp' in want and not device_rows)) else None
        mc = numpy.empty((n, self.order + 1), numpy.float64) if 'mc' in want else None
        rows = None
        if device_rows and 'sp' in want:
            buf = _DeviceBuffer(self._ctx, max(n, 1) * BINS)
            rows = DeviceRows(buf.address, n, keep=buf)
        lib.check(lib.dll.ry_analysis_run(h, _dptr(x), x.size, _dptr(f0), _dptr(t), n, _dptr(sp64), _lib._fptr(rows.address if rows else None),
                                          _dptr(mc)))
        got = {'sp': rows if device_rows else sp64, 'sp64': sp64, 'mc': mc}
        return tuple(got[k] for k in want)

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

    def close(self):
        if self._handle is not None and self._pid == os.getpid() and self._ctx is not None and self._ctx.handle is not None:
            self._ctx.lib.dll.ry_analysis_destroy(self._handle)
        self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the packages' functions ---------------------------------------------------------------------------------------------------------
class engine_for_tests(object):
    """tests: `ctx`, a context over another build of the library (the emulator), for the analyzers the functions below create."""
    ctx = None


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
    """(ap, coded_ap) of the frames.  D4C is the stage of the analysis that is not built here: this default hands it to `pyworld` where that
    package exists; assign another callable of the same signature to `world_analysis.aperiodicity` to replace it."""
    try:
        import pyworld
        ap = pyworld.d4c(x, f0, t, fs, fft_size=fft_size)
        return ap, pyworld.code_aperiodicity(ap, fs)
    except (ImportError, NotImplementedError) as e:
        raise NotImplementedError('aperiodicity: D4C (WORLD\'s band aperiodicity) is not built on the device yet and `pyworld` is not usable here; '
                                  'assign a callable (x, f0, t, fs, fft_size) -> (ap, coded_ap) to world_analysis.aperiodicity') from e


def extract(cls, wave, frame_period, f0_floor, f0_ceil, fft_length, order, alpha, dtype):
    """Drop-in body of `AcousticFeature.extract`: f0 from `cls.extract_f0` (so a bound CREPE wrapper keeps working), `sp` / `mc` from the
    device, `ap` / `coded_ap` from `world_analysis.aperiodicity`.  Returns the plain `AcousticFeature` container whatever `cls` is, like the original."""
    x = wave.wave.astype(numpy.float64)
    fs = wave.sampling_rate
    f0, t = cls.extract_f0(x=x, fs=fs, frame_period=frame_period, f0_floor=f0_floor, f0_ceil=f0_ceil)
    f0, t = numpy.asarray(f0, numpy.float64), numpy.asarray(t, numpy.float64)
    fft_size = int(fft_length) if fft_length else cheaptrick_fft_size(fs)
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
