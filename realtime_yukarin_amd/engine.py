"""Host-side handles over the C ABI: one `Context` per (process, GPU), one `Net` per predictor.

Mirrors what the reference's dependencies do around their Chainer models ([MEM]; call sites
/root/reference/realtime_voice_conversion/converter/yukarin_converter.py:40-55): build the predictor
from the config's `model` section, load the npz, move it to the GPU, then run `model(x)` per buffer.
Contexts are created lazily per process id: the reference constructs the converter objects in the
parent and ships them to a child `Process` (/root/reference/run.py:39-46,69-79), and a HIP context
must never cross a fork.
"""
import ctypes
import os
import weakref
from typing import Dict, List, Optional

import numpy

from . import _lib
from .netspec import NetDesc, pad_frames, param_count


class Context(object):
    def __init__(self, device: int = 0, lib: Optional[_lib.Ry355Lib] = None):
        self.lib = lib if lib is not None else _lib.default_lib()
        self.device = int(device)
        self.pid = os.getpid()
        n = self.lib.device_count()
        if n < 1:
            raise _lib.Ry355Error('no HIP device is visible: realtime_yukarin_amd needs an MI355X (there is no CPU path)')
        h = ctypes.c_void_p()
        self.lib.check(self.lib.dll.ry_init(self.device, ctypes.byref(h)))
        self.handle = h

    def sync(self):
        self.lib.check(self.lib.dll.ry_sync(self.handle))

    @property
    def stream(self) -> int:
        return int(self.lib.dll.ry_stream(self.handle) or 0)

    def reload_env(self):
        """Read the process-wide RY_* switches again (`ry_debug_reload_env`; tests and A/B scripts).  Launch plans that exist keep their choices until
        `Net.set_dtype` drops them."""
        self.lib.check(self.lib.dll.ry_debug_reload_env())

    def timer_start(self):
        self.lib.check(self.lib.dll.ry_timer_start(self.handle))

    def timer_stop(self) -> float:
        ms = ctypes.c_float()
        self.lib.check(self.lib.dll.ry_timer_stop(self.handle, ctypes.byref(ms)))
        return float(ms.value)

    def close(self):
        if self.handle is not None and self.pid == os.getpid():
            self.lib.dll.ry_shutdown(self.handle)
        self.handle = None

    def dev_alloc(self, n_floats: int) -> int:
        p = ctypes.POINTER(ctypes.c_float)()
        self.lib.check(self.lib.dll.ry_dev_alloc(self.handle, int(n_floats), ctypes.byref(p)))
        return ctypes.cast(p, ctypes.c_void_p).value

    def dev_free(self, ptr: int):
        self.lib.check(self.lib.dll.ry_dev_free(self.handle, _lib._fptr(int(ptr))))

    def dev_upload(self, ptr: int, a: numpy.ndarray):
        a = numpy.ascontiguousarray(a)
        assert a.dtype.itemsize == 4, 'four-byte elements (float32 / int32)'
        self.lib.check(self.lib.dll.ry_dev_upload(self.handle, _lib._fptr(int(ptr)), ctypes.cast(a.ctypes.data, ctypes.POINTER(ctypes.c_float)), a.size))

    def dev_download(self, ptr: int, a: numpy.ndarray):
        assert a.flags['C_CONTIGUOUS'] and a.dtype.itemsize == 4
        self.lib.check(self.lib.dll.ry_dev_download(self.handle, ctypes.cast(a.ctypes.data, ctypes.POINTER(ctypes.c_float)), _lib._fptr(int(ptr)), a.size))

    def mask_rows(self, rows_ptr: int, mask_ptr: int, n: int, cols: int, k0: int = 0, k1: Optional[int] = None, stream: Optional[int] = None):
        """`combine_silent` of float32 rows that stay on the card (`ry_mask_rows`): rows [k0, k1) of the (n, cols) block at `rows_ptr` whose byte in
        the mask at `mask_ptr` is 0 become +0.0 in place.  Enqueued on `stream` (default: the context stream), nothing is waited for."""
        self.lib.check(self.lib.dll.ry_mask_rows(self.handle, _lib._fptr(int(rows_ptr)), ctypes.cast(ctypes.c_void_p(int(mask_ptr)), ctypes.POINTER(ctypes.c_ubyte)),
                                                 int(n), int(cols), int(k0), int(n if k1 is None else k1), ctypes.c_void_p(stream or 0)))

    def gather_rows(self, rows_ptr: int, n_rows: int, cols: int, src_row_ptr: int, dst_ptr: int, n_out: int, mask_ptr: Optional[int] = None,
                    stream: Optional[int] = None):
        """`ry_gather_rows`: row j < n_out of the block at `dst_ptr` = row src_row[j] of the (n_rows, cols) float32 block at `rows_ptr` (`src_row_ptr`: an
        int32 table on the card), or +0.0 where the mask byte of that source row is 0 (`mask_ptr` None: every row is kept).  Enqueued on `stream`
        (default: the context stream), nothing is waited for."""
        self.lib.check(self.lib.dll.ry_gather_rows(self.handle, _lib._fptr(int(rows_ptr)), int(n_rows), int(cols),
                                                   ctypes.cast(ctypes.c_void_p(int(src_row_ptr)), ctypes.POINTER(ctypes.c_int)),
                                                   ctypes.cast(ctypes.c_void_p(int(mask_ptr or 0)), ctypes.POINTER(ctypes.c_ubyte)),
                                                   _lib._fptr(int(dst_ptr)), int(n_out), ctypes.c_void_p(stream or 0)))

    def debug_layer_filters(self, W: numpy.ndarray, kind: str, cin_b: int = 0, stride: int = 1, pad: int = 0, transposed: bool = False,
                            want_os2: bool = False) -> numpy.ndarray:
        """Tests: layout `kind` ('w1d', 'w1os', 'wig', 'wdir', 'w2os', 'wwin') of ONE layer with the raw Chainer filter W -- (Cout, Cin, k[, k]), transposed
        (Cin, Cout, 4[, 4]); the last cin_b input channels are the second skip source -- built in the filter build mode in force
        (`ry_debug_layer_filters`), flat float32.  Raises `Ry355Error` when the layer has no such layout."""
        W = numpy.ascontiguousarray(W, dtype=numpy.float32)
        ndim = W.ndim - 2
        cin, cout = (W.shape[0], W.shape[1]) if transposed else (W.shape[1], W.shape[0])
        args = [self.handle, ndim, cin - int(cin_b), int(cin_b), cout, W.shape[2], int(stride), int(pad), int(bool(transposed)), int(bool(want_os2)),
                _lib._fptr(W), _lib.FILTER_KINDS[kind]]
        n = ctypes.c_size_t(0)
        rc = self.lib.dll.ry_debug_layer_filters(*(args + [None, 0, ctypes.byref(n)]))
        if n.value == 0:
            self.lib.check(rc)
        out = numpy.empty(n.value, dtype=numpy.float32)
        self.lib.check(self.lib.dll.ry_debug_layer_filters(*(args + [_lib._fptr(out), out.size, ctypes.byref(n)])))
        return out

    def mc2sp(self, mc, mtx, floor: float = 0.0):
        """`decode_spectrogram` on the device: exp(mc (N, M) @ mtx (M, F)) + floor."""
        mc = numpy.ascontiguousarray(mc, dtype=numpy.float32)
        mtx = numpy.ascontiguousarray(mtx, dtype=numpy.float32)
        sp = numpy.empty((mc.shape[0], mtx.shape[1]), dtype=numpy.float32)
        self.lib.check(self.lib.dll.ry_mc2sp(self.handle, _lib._fptr(mc), _lib._fptr(mtx), mc.shape[0], mc.shape[1], mtx.shape[1],
                                             float(floor), _lib._fptr(sp)))
        return sp

    # ---- single operators (Chainer layouts in, channels-last activations) ----
    def conv1d(self, x, W, b=None, bn=None, stride=1, pad=0, dilate=1, transposed=False, act=None, splits=0):
        """x (B, L, Cin) -> (B, Lout, Cout).  W (Cout,Cin,k) or transposed (Cin,Cout,k); bn = (gamma,beta,mean,var)."""
        x = numpy.ascontiguousarray(x, dtype=numpy.float32)
        W = numpy.ascontiguousarray(W, dtype=numpy.float32)
        B, L, Cin = x.shape
        Cout = W.shape[1] if transposed else W.shape[0]
        k = W.shape[2]
        Lout = 2 * L if transposed else (L + 2 * pad - dilate * (k - 1) - 1) // stride + 1
        a = _lib.ACTS[act]
        y = numpy.empty((B, max(Lout, 0), Cout // 2 if a == _lib.ACT_GLU else Cout), dtype=numpy.float32)
        bnv = None if bn is None else numpy.ascontiguousarray(numpy.concatenate([numpy.ravel(v) for v in bn]), dtype=numpy.float32)
        bv = None if b is None else numpy.ascontiguousarray(b, dtype=numpy.float32)
        self.lib.check(self.lib.dll.ry_conv1d(self.handle, _lib._fptr(x), B, L, Cin, _lib._fptr(W), _lib._fptr(bv), _lib._fptr(bnv),
                                              Cout, k, stride, pad, dilate, int(bool(transposed)), a, int(splits), _lib._fptr(y)))
        return y

    def conv1d_os(self, xa, W, b=None, bn=None, stride=1, pad=0, transposed=False, act=None, xb=None, tile=None, pad_to=0, keep=0):
        """The layer of `conv1d` on the predictors' output-stationary stage-1 kernel (ry_c1d_os), one launch.  xa (B, L, Ca) and xb (B, L, Cb) or
        None: the two sources of a skip concat, W over Ca + Cb input channels.  tile = (cb, tp) slice, None = the planner's pick.  pad_to > 0: the
        fused pad of the convert wrapper -- xa holds the n_real = xa.shape[1] real rows of each window, the kernel reads rows n_real .. pad_to - 1
        as the per-channel minimum of the real rows (L = pad_to).  keep: rows stored per window (0 = all).  -> (B, keep or Lout, Cout)."""
        xa = numpy.ascontiguousarray(xa, dtype=numpy.float32)
        W = numpy.ascontiguousarray(W, dtype=numpy.float32)
        B, rows, Ca = xa.shape
        xbv = None if xb is None else numpy.ascontiguousarray(xb, dtype=numpy.float32)
        Cb = 0 if xbv is None else xbv.shape[2]
        L = int(pad_to) if pad_to else rows
        assert xbv is None or xbv.shape[:2] == (B, L), (xa.shape, xbv.shape)
        Cout = W.shape[1] if transposed else W.shape[0]
        k = W.shape[2]
        Lout = 2 * L if transposed else (L + 2 * pad - k) // stride + 1
        y = numpy.empty((B, max(keep or Lout, 0), Cout), dtype=numpy.float32)
        bnv = None if bn is None else numpy.ascontiguousarray(numpy.concatenate([numpy.ravel(v) for v in bn]), dtype=numpy.float32)
        bv = None if b is None else numpy.ascontiguousarray(b, dtype=numpy.float32)
        cb, tp = tile or (0, 0)
        self.lib.check(self.lib.dll.ry_conv1d_os(self.handle, _lib._fptr(xa), _lib._fptr(xbv), B, L, Ca, Cb, _lib._fptr(W), _lib._fptr(bv),
                                                 _lib._fptr(bnv), Cout, k, stride, pad, int(bool(transposed)), _lib.ACTS[act], int(cb), int(tp),
                                                 rows if pad_to else 0, int(keep), _lib._fptr(y)))
        return y

    def conv2d(self, x, W, b=None, bn=None, stride=1, pad=0, transposed=False, act=None, path='auto', tile=None, splits=0, dilate=1):
        """x (B, H, W, Cin) -> (B, Ho, Wo, Cout).  W (Cout,Cin,k,k) or transposed (Cin,Cout,k,k)."""
        x = numpy.ascontiguousarray(x, dtype=numpy.float32)
        W = numpy.ascontiguousarray(W, dtype=numpy.float32)
        B, H, Wd, Cin = x.shape
        Cout = W.shape[1] if transposed else W.shape[0]
        k = W.shape[2]
        Ho = 2 * H if transposed else (H + 2 * pad - dilate * (k - 1) - 1) // stride + 1
        Wo = 2 * Wd if transposed else (Wd + 2 * pad - dilate * (k - 1) - 1) // stride + 1
        y = numpy.empty((B, max(Ho, 0), max(Wo, 0), Cout), dtype=numpy.float32)
        bnv = None if bn is None else numpy.ascontiguousarray(numpy.concatenate([numpy.ravel(v) for v in bn]), dtype=numpy.float32)
        bv = None if b is None else numpy.ascontiguousarray(b, dtype=numpy.float32)
        pth = {'auto': 0, 'igemm': 1, 'direct': 2, 'first': 3, 'last': 4, 'igemm_bf16': 5, 'igemm_x3': 6, 'os': 7, 'wino': 8}[path]
        if path == 'wino':       # Winograd F(2x2, 2x2) form of a k4 s2 p1 layer: tile = (cfg, mbw): workgroup shape (1: 2x2 waves, 2: 4x2 waves) and M-blocks per tile row; zeros / None = the planner's choice
            c = tuple(tile or ()) + (0, 0)
            tcode = int(c[0]) + 16 * int(c[1])
        elif path == 'os':         # output-stationary weight-streaming kernel: tile = (mt4, nt4, waves, depth), zeros / None = the planner's choice
            c = tuple(tile or ()) + (0, 0, 0, 0)
            tcode = int(c[0]) + 16 * int(c[1]) + 256 * int(c[2]) + 8192 * int(c[3])
        else:
            tcode = _lib.TILES[tile]
        self.lib.check(self.lib.dll.ry_conv2d_dilated(self.handle, _lib._fptr(x), B, H, Wd, Cin, _lib._fptr(W), _lib._fptr(bv), _lib._fptr(bnv),
                                                      Cout, k, stride, pad, int(dilate), int(bool(transposed)), _lib.ACTS[act], pth, tcode,
                                                      int(splits), _lib._fptr(y)))
        return y


class VcCore(object):
    """Device-resident core of `VoiceChanger.convert_from_acoustic_feature`: stage-1 on the effective frames ->
    scatter into the silent block -> mc2sp (exp(mc @ M)) -> + floor -> stage-2, one H2D and one D2H per window (`ry_vc_convert`)."""

    def __init__(self, stage1: 'Net', stage2: 'Net', mtx: numpy.ndarray, lanes: Optional[int] = None):
        self.stage1, self.stage2 = stage1, stage2
        self.lib = stage1.ctx.lib
        mtx = numpy.ascontiguousarray(mtx, dtype=numpy.float32)
        self.M, self.F = mtx.shape
        h = ctypes.c_void_p()
        self.lib.check(self.lib.dll.ry_vc_create(stage1.handle, stage2.handle, _lib._fptr(mtx), self.M, self.F, ctypes.byref(h)))
        self.handle = h
        stage1._dependents.add(self); stage2._dependents.add(self)       # `ry_vc` holds raw pointers to both predictors: they must outlive it (Net.close)
        self._pending = {}
        self.discard = (0, 0)
        # lanes: the six ring slots spread over two pairs of predictor handles (`ry_vc_set_lanes`), so that two windows really run side by side
        # (RY_VC_LANES=1: one stage-2 forward after the other; 3 measured slower than 2)
        self.lanes = int(os.environ.get('RY_VC_LANES', '2')) if lanes is None else int(lanes)
        if self.lanes != 1:
            self.set_lanes(self.lanes)

    def reserve(self, n_frames: int):
        """Size the ring for windows of up to n_frames ahead of time (`ry_vc_reserve_frames`): a stream whose windows grow while others are in
        flight is otherwise refused (the ring cannot be re-allocated under a window)."""
        self.lib.check(self.lib.dll.ry_vc_reserve_frames(self.handle, int(n_frames)))

    def warm(self, n_frames: int, rounds: int = 2):
        """Build the launch plans and capture the graphs of every ring slot for windows of n_frames before the first real window
        arrives (each slot otherwise pays them on its first window: tens of milliseconds, once).  Silence-gated windows of another
        effective length still build their stage-1 plan on first sight."""
        x = numpy.zeros((int(n_frames), self.stage1.desc.in_ch), numpy.float32)
        eff = numpy.ones(int(n_frames), bool)
        for _ in range(6 * int(rounds)):
            self.convert(x, eff)

    def set_discard(self, front: int, back: int):
        """The caller will throw away the first `front` / last `back` frames of every following window (`ry_vc_set_discard`): stage 2
        does not compute them, their spectrogram rows come back as zeros; (0, 0) = everything."""
        self.lib.check(self.lib.dll.ry_vc_set_discard(self.handle, int(front), int(back)))
        self.discard = (int(front), int(back))

    def set_lanes(self, lanes: int):
        self.lib.check(self.lib.dll.ry_vc_set_lanes(self.handle, int(lanes)))
        self.lanes = int(lanes)

    STREAM_FORMS = ('wide', 'compact-a', 'compact-b')

    def debug_streams(self):
        """(form, n): the stream topology of the lanes ('wide': two streams per lane; 'compact-a': one per lane; 'compact-b': one stage-1 stream
        beside a stage-2 stream per lane -- chosen from GPU_MAX_HW_QUEUES / RY_VC_STREAMS when the core was made, `ry_vc_set_lanes`) and the number
        of distinct streams the calls have enqueued on since (`ry_vc_debug_streams`, tests)."""
        f, n = ctypes.c_int(-1), ctypes.c_int(-1)
        self.lib.check(self.lib.dll.ry_vc_debug_streams(self.handle, ctypes.byref(f), ctypes.byref(n)))
        return self.STREAM_FORMS[f.value], int(n.value)

    @property
    def ring(self) -> int:
        """Windows that may be in flight: six ring slots up to three lanes, else two per lane."""
        return 6 if self.lanes <= 3 else 2 * self.lanes

    @staticmethod
    def _rows(effective):
        effective = numpy.asarray(effective, dtype=bool)
        return int(effective.size), numpy.ascontiguousarray(numpy.nonzero(effective)[0], dtype=numpy.int32)

    def submit(self, x_eff: numpy.ndarray, effective: numpy.ndarray, sp_floor: float = 1e-16) -> int:
        """Queue one window (pinned ring slot -> H2D -> stage-1 -> ... -> D2H) and return its ticket without waiting; up to six
        windows may be in flight (`ry_vc_submit`)."""
        n, rows = self._rows(effective)
        x_eff = numpy.ascontiguousarray(x_eff, dtype=numpy.float32)
        if len(rows):
            x_eff = x_eff.reshape(len(rows), -1)
        t = ctypes.c_int(-1)
        self.lib.check(self.lib.dll.ry_vc_submit(self.handle, _lib._fptr(x_eff) if len(rows) else _lib._fptr(None),
                                                 rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(rows), n, float(sp_floor), ctypes.byref(t)))
        self._pending[t.value] = n
        return int(t.value)

    def wait(self, ticket: int):
        """(mc (n_frames, M), sp (n_frames, F)) of a submitted window (`ry_vc_wait`)."""
        n = self._pending.pop(ticket)
        mc = numpy.empty((n, self.M), dtype=numpy.float32)
        sp = numpy.empty((n, self.F), dtype=numpy.float32)
        self.lib.check(self.lib.dll.ry_vc_wait(self.handle, int(ticket), _lib._fptr(mc), _lib._fptr(sp)))
        return mc, sp

    def convert(self, x_eff: numpy.ndarray, effective: numpy.ndarray, sp_floor: float = 1e-16):
        """x_eff (n_eff, in_ch) = features of the effective frames, effective (n_frames,) bool -> (mc (n_frames, M), sp (n_frames, F))."""
        return self.wait(self.submit(x_eff, effective, sp_floor))

    def submit_wave(self, wave: numpy.ndarray, hop: int, fft_length: int, p_effective: float, p_all: float, feat: numpy.ndarray,
                    sp_floor: float = 1e-16) -> int:
        """`ry_vc_submit_wave`: the silence gate on the device.  wave float32 (n_samples,), feat (n_frames, in_ch) = the features of ALL
        frames; the thresholds come from `gate.thresholds(threshold_db)`."""
        wave = numpy.ascontiguousarray(wave, dtype=numpy.float32)
        feat = numpy.ascontiguousarray(feat, dtype=numpy.float32)
        t = ctypes.c_int(-1)
        self.lib.check(self.lib.dll.ry_vc_submit_wave(self.handle, _lib._fptr(wave), wave.size, int(hop), int(fft_length), float(p_effective),
                                                      float(p_all), _lib._fptr(feat), feat.shape[0], float(sp_floor), ctypes.byref(t)))
        self._pending[t.value] = feat.shape[0]
        return int(t.value)

    def gate(self, wave: numpy.ndarray, hop: int, fft_length: int, p_effective: float, p_all: float, feat: numpy.ndarray):
        """`ry_vc_gate`: `separate_effective` alone on the device -> (effective (n,) bool, x_eff (n_eff, in_ch), row_of (n_eff,))."""
        wave = numpy.ascontiguousarray(wave, dtype=numpy.float32)
        feat = numpy.ascontiguousarray(feat, dtype=numpy.float32)
        n = feat.shape[0]
        mask = numpy.empty(n, dtype=numpy.uint8)
        x = numpy.empty((n, feat.shape[1]), dtype=numpy.float32)
        rows = numpy.empty(n, dtype=numpy.int32)
        n_eff = ctypes.c_int(0)
        self.lib.check(self.lib.dll.ry_vc_gate(self.handle, _lib._fptr(wave), wave.size, int(hop), int(fft_length), float(p_effective), float(p_all),
                                               _lib._fptr(feat), n, mask.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), ctypes.byref(n_eff),
                                               _lib._fptr(x), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return mask.astype(bool), x[:n_eff.value], rows[:n_eff.value]

    def wait_wave(self, ticket: int):
        """(mc, sp, effective (n_frames,) bool) of a window submitted with `submit_wave`."""
        n = self._pending.pop(ticket)
        mc = numpy.empty((n, self.M), dtype=numpy.float32)
        sp = numpy.empty((n, self.F), dtype=numpy.float32)
        mask = numpy.empty(n, dtype=numpy.uint8)
        n_eff = ctypes.c_int(0)
        self.lib.check(self.lib.dll.ry_vc_wait_wave(self.handle, int(ticket), _lib._fptr(mc), _lib._fptr(sp),
                                                    mask.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), ctypes.byref(n_eff)))
        return mc, sp, mask.astype(bool)

    def convert_stream(self, windows, sp_floor: float = 1e-16, depth: int = 2):
        """Generator over (x_eff, effective) pairs -> (mc, sp) in order, keeping `depth` windows in flight: the copies of one window
        run under the kernels of another."""
        if not 1 <= depth <= self.ring:
            raise ValueError('depth must be 1..%d (six ring slots up to three lanes, else two per lane)' % self.ring)
        tickets = []
        for x_eff, effective in windows:
            tickets.append(self.submit(x_eff, effective, sp_floor))
            if len(tickets) >= depth:
                yield self.wait(tickets.pop(0))
        while tickets:
            yield self.wait(tickets.pop(0))

    def enqueue_device(self, x_ptr: int, rows_ptr: int, n_eff: int, n_frames: int, mc_ptr: int, sp_ptr: int, sp_floor: float = 1e-16):
        """Device pointers in and out, nothing waited for (`ry_vc_enqueue_device`)."""
        self.lib.check(self.lib.dll.ry_vc_enqueue_device(
            self.handle, _lib._fptr(int(x_ptr)), ctypes.cast(ctypes.c_void_p(int(rows_ptr)), ctypes.POINTER(ctypes.c_int)),
            int(n_eff), int(n_frames), float(sp_floor), _lib._fptr(int(mc_ptr)), _lib._fptr(int(sp_ptr))))

    def enqueue_wave_device(self, wave_ptr: int, n_samples: int, hop: int, fft_length: int, p_effective: float, p_all: float, feat_ptr: int,
                            n_frames: int, mc_ptr: int, sp_ptr: int, mask_ptr: int, sp_floor: float = 1e-16):
        """`ry_vc_enqueue_wave_device`: `submit_wave` on a float32 wave and a (n_frames, in_ch) feature block that are already on the card, mc / sp /
        the mask bytes left on the card -> (effective (n_frames,) bool, n_eff).  Waits for the count only; the context stream is ordered behind the
        window, so what is enqueued on it afterwards reads complete rows."""
        mask = numpy.empty(int(n_frames), dtype=numpy.uint8)
        n_eff = ctypes.c_int(0)
        ub = ctypes.POINTER(ctypes.c_ubyte)
        self.lib.check(self.lib.dll.ry_vc_enqueue_wave_device(
            self.handle, _lib._fptr(int(wave_ptr)), int(n_samples), int(hop), int(fft_length), float(p_effective), float(p_all),
            _lib._fptr(int(feat_ptr)), int(n_frames), float(sp_floor), _lib._fptr(int(mc_ptr)), _lib._fptr(int(sp_ptr)),
            ctypes.cast(ctypes.c_void_p(int(mask_ptr)), ub), mask.ctypes.data_as(ub), ctypes.byref(n_eff)))
        return mask.astype(bool), int(n_eff.value)

    @staticmethod
    def _offsets(sample_offsets, frame_offsets):
        so = numpy.ascontiguousarray(sample_offsets, dtype=numpy.int64).ravel()
        fo = numpy.ascontiguousarray(frame_offsets, dtype=numpy.int32).ravel()
        if so.size != fo.size or so.size < 2:
            raise ValueError('two offset arrays of waves + 1 >= 2 entries are needed, got %d and %d' % (so.size, fo.size))
        return so, fo, so.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    def gate_waves_device(self, wave_ptr: int, sample_offsets, frame_offsets, hop: int, fft_length: int, p_effective: float, p_all: float,
                          feat_ptr: int, mask_ptr: int, x_eff_ptr: Optional[int] = None, row_of_ptr: Optional[int] = None):
        """`ry_vc_gate_waves_device`: `separate_effective` of the waves back to back at `wave_ptr` (wave i at sample_offsets[i] / frame_offsets[i])
        in one launch pair and one wait -> (effective (sum n,) bool, n_eff (waves,) int32); the mask bytes at `mask_ptr`, the effective rows and
        their frame indices in the blocks at `x_eff_ptr` / `row_of_ptr` (wave i from row frame_offsets[i] on), all on the card."""
        so, fo, pso, pfo = self._offsets(sample_offsets, frame_offsets)
        mask, n_eff = numpy.empty(max(int(fo[-1]), 1), numpy.uint8), numpy.zeros(so.size - 1, numpy.int32)
        ub, ip = ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)
        self.lib.check(self.lib.dll.ry_vc_gate_waves_device(
            self.handle, _lib._fptr(int(wave_ptr)), pso, pfo, so.size - 1, int(hop), int(fft_length), float(p_effective), float(p_all),
            _lib._fptr(int(feat_ptr)), ctypes.cast(ctypes.c_void_p(int(mask_ptr)), ub), mask.ctypes.data_as(ub), n_eff.ctypes.data_as(ip),
            _lib._fptr(None if x_eff_ptr is None else int(x_eff_ptr)), ctypes.cast(ctypes.c_void_p(int(row_of_ptr or 0)), ip)))
        return mask[:int(fo[-1])].astype(bool), n_eff

    def enqueue_waves_device(self, wave_ptr: int, sample_offsets, frame_offsets, hop: int, fft_length: int, p_effective: float, p_all: float,
                             feat_ptr: int, mc_ptr: int, sp_ptr: int, mask_ptr: int, sp_floor: float = 1e-16):
        """`ry_vc_enqueue_waves_device`: `enqueue_wave_device` for the waves back to back at `wave_ptr` in one call -- one gate and one wait for all
        counts, then every wave's window on its own rows of the (sum n, ...) blocks -> (effective (sum n,) bool, n_eff (waves,) int32).  Wave i gets
        the bits of the single call on it alone."""
        so, fo, pso, pfo = self._offsets(sample_offsets, frame_offsets)
        mask, n_eff = numpy.empty(max(int(fo[-1]), 1), numpy.uint8), numpy.zeros(so.size - 1, numpy.int32)
        ub = ctypes.POINTER(ctypes.c_ubyte)
        self.lib.check(self.lib.dll.ry_vc_enqueue_waves_device(
            self.handle, _lib._fptr(int(wave_ptr)), pso, pfo, so.size - 1, int(hop), int(fft_length), float(p_effective), float(p_all),
            _lib._fptr(int(feat_ptr)), float(sp_floor), _lib._fptr(int(mc_ptr)), _lib._fptr(int(sp_ptr)),
            ctypes.cast(ctypes.c_void_p(int(mask_ptr)), ub), mask.ctypes.data_as(ub), n_eff.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return mask[:int(fo[-1])].astype(bool), n_eff

    def gate_verdict_waves_device(self, wave_ptr: int, sample_offsets, frame_offsets, hop: int, fft_length: int, p_effective: float, p_all: float,
                                  mask_ptr: int):
        """`ry_vc_gate_verdict_waves_device`: the verdict of `gate_waves_device` before any feature row exists -- the same launches, the same one
        wait, no row read or written -> (effective (sum n,) bool, n_eff (waves,) int32), the mask bytes at `mask_ptr`."""
        so, fo, pso, pfo = self._offsets(sample_offsets, frame_offsets)
        mask, n_eff = numpy.empty(max(int(fo[-1]), 1), numpy.uint8), numpy.zeros(so.size - 1, numpy.int32)
        ub = ctypes.POINTER(ctypes.c_ubyte)
        self.lib.check(self.lib.dll.ry_vc_gate_verdict_waves_device(
            self.handle, _lib._fptr(int(wave_ptr)), pso, pfo, so.size - 1, int(hop), int(fft_length), float(p_effective), float(p_all),
            ctypes.cast(ctypes.c_void_p(int(mask_ptr)), ub), mask.ctypes.data_as(ub), n_eff.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return mask[:int(fo[-1])].astype(bool), n_eff

    @staticmethod
    def _verdict(frame_offsets, effective, n_eff):
        fo = numpy.ascontiguousarray(frame_offsets, dtype=numpy.int32).ravel()
        if fo.size < 2:
            raise ValueError('frame offsets of waves + 1 >= 2 entries are needed, got %d' % fo.size)
        eff = numpy.ascontiguousarray(numpy.asarray(effective).astype(numpy.uint8)).ravel()
        ne = numpy.ascontiguousarray(n_eff, dtype=numpy.int32).ravel()
        if eff.size != int(fo[-1]) or ne.size != fo.size - 1:
            raise ValueError('%d mask bytes and %d counts for %d frames of %d waves' % (eff.size, ne.size, int(fo[-1]), fo.size - 1))
        ub, ip = ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)
        return fo, eff, ne, fo.ctypes.data_as(ip), eff.ctypes.data_as(ub), ne.ctypes.data_as(ip)

    def compact_waves_device(self, frame_offsets, mask_ptr: int, effective, n_eff, feat_ptr: int, x_eff_ptr: Optional[int] = None,
                             row_of_ptr: Optional[int] = None) -> None:
        """`ry_vc_compact_waves_device`: the ordered compaction of `gate_waves_device` alone, from its verdict (the mask bytes at `mask_ptr`, their
        host copy and the counts): the effective rows and their frame indices at `x_eff_ptr` / `row_of_ptr`, wave i from row frame_offsets[i] on."""
        fo, eff, ne, pfo, peff, pne = self._verdict(frame_offsets, effective, n_eff)
        ub, ip = ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)
        self.lib.check(self.lib.dll.ry_vc_compact_waves_device(
            self.handle, pfo, fo.size - 1, ctypes.cast(ctypes.c_void_p(int(mask_ptr)), ub), peff, pne, _lib._fptr(int(feat_ptr)),
            _lib._fptr(None if x_eff_ptr is None else int(x_eff_ptr)), ctypes.cast(ctypes.c_void_p(int(row_of_ptr or 0)), ip)))

    def enqueue_waves_masked_device(self, frame_offsets, feat_ptr: int, mc_ptr: int, sp_ptr: int, mask_ptr: int, effective, n_eff,
                                    sp_floor: float = 1e-16) -> None:
        """`ry_vc_enqueue_waves_masked_device`: `enqueue_waves_device` on a verdict `gate_verdict_waves_device` made earlier -- no gate kernel, no
        wait; the feature rows of a wave without an effective frame are not read."""
        fo, eff, ne, pfo, peff, pne = self._verdict(frame_offsets, effective, n_eff)
        ub = ctypes.POINTER(ctypes.c_ubyte)
        self.lib.check(self.lib.dll.ry_vc_enqueue_waves_masked_device(
            self.handle, pfo, fo.size - 1, _lib._fptr(int(feat_ptr)), float(sp_floor), _lib._fptr(int(mc_ptr)), _lib._fptr(int(sp_ptr)),
            ctypes.cast(ctypes.c_void_p(int(mask_ptr)), ub), peff, pne))

    def enqueue_device_batch(self, x_ptr: int, rows_ptr: int, n_eff, n_frames: int, mc_ptr: int, sp_ptr: int, sp_floor: float = 1e-16):
        """`ry_vc_enqueue_device_batch`: len(n_eff) windows of n_frames each, device pointers, nothing waited for."""
        ne = numpy.ascontiguousarray(n_eff, dtype=numpy.int32)
        self.lib.check(self.lib.dll.ry_vc_enqueue_device_batch(
            self.handle, len(ne), _lib._fptr(int(x_ptr)), ctypes.cast(ctypes.c_void_p(int(rows_ptr)), ctypes.POINTER(ctypes.c_int)),
            ne.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(n_frames), float(sp_floor), _lib._fptr(int(mc_ptr)), _lib._fptr(int(sp_ptr))))

    def convert_batch(self, windows, sp_floor: float = 1e-16):
        """Host arrays in and out for a list of (x_eff, effective) windows of ONE length: [(mc, sp), ...].  Plain (blocking) copies:
        the call is for throughput on a backlog, not for latency."""
        ctx = self.stage1.ctx
        n, cin = len(windows[0][1]), self.stage1.desc.in_ch
        xs, rows, ne = [], [], []
        for x_eff, effective in windows:
            nn, r = self._rows(effective)
            if nn != n:
                raise ValueError('convert_batch needs windows of one length (got %d and %d frames)' % (n, nn))
            x_eff = numpy.ascontiguousarray(x_eff, dtype=numpy.float32)
            if x_eff.shape[0] != len(r):
                raise ValueError('%d effective rows for a mask with %d set frames' % (x_eff.shape[0], len(r)))
            xs.append(x_eff.reshape(len(r), cin)); rows.append(r); ne.append(len(r))
        W, tot = len(windows), int(sum(ne))
        d_x = ctx.dev_alloc(max(tot, 1) * cin); d_r = ctx.dev_alloc(max(tot, 1)); d_mc = ctx.dev_alloc(W * n * self.M); d_sp = ctx.dev_alloc(W * n * self.F)
        try:
            if tot:
                ctx.dev_upload(d_x, numpy.concatenate(xs))
                ctx.dev_upload(d_r, numpy.concatenate(rows).astype(numpy.int32))
            self.enqueue_device_batch(d_x, d_r, ne, n, d_mc, d_sp, sp_floor)
            ctx.sync()
            mc = numpy.empty((W, n, self.M), numpy.float32); sp = numpy.empty((W, n, self.F), numpy.float32)
            ctx.dev_download(d_mc, mc); ctx.dev_download(d_sp, sp)
            if self.discard != (0, 0):                                   # rows the caller said it throws away were not computed: zeros
                k0 = self.discard[0] if self.discard[0] < n else 0
                k1 = n - self.discard[1] if n - self.discard[1] > k0 else n
                sp[:, :k0] = 0; sp[:, k1:] = 0
        finally:
            for q in (d_x, d_r, d_mc, d_sp):
                ctx.dev_free(q)
        return [(mc[w], sp[w]) for w in range(W)]

    # ---- the chain cut where the reference's own VoiceChanger cuts it (voice_changer.py:33-41)
    def convert_stage1(self, x_eff: numpy.ndarray) -> numpy.ndarray:
        """`AcousticConverter.convert` array part; the converted rows also stay on the device for `stage2_from_mc`."""
        x_eff = numpy.ascontiguousarray(x_eff, dtype=numpy.float32)
        y = numpy.empty((x_eff.shape[0], self.M), dtype=numpy.float32)
        self.lib.check(self.lib.dll.ry_vc_stage1(self.handle, _lib._fptr(x_eff), x_eff.shape[0], _lib._fptr(y)))
        return y

    def stage2_from_mc(self, effective: numpy.ndarray, sp_floor: float) -> numpy.ndarray:
        """combine_silent + decode_spectrogram + floor + SuperResolution.convert from the rows `convert_stage1` left on the device."""
        n, rows = self._rows(effective)
        sp = numpy.empty((n, self.F), dtype=numpy.float32)
        self.lib.check(self.lib.dll.ry_vc_stage2_from_mc(self.handle, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(rows), n,
                                                         float(sp_floor), _lib._fptr(sp)))
        return sp

    def mid_sp(self, effective: numpy.ndarray, sp_floor: float) -> numpy.ndarray:
        """The intermediate spectrogram exp(mc @ M) + floor of the rows `convert_stage1` left on the device."""
        n, rows = self._rows(effective)
        sp = numpy.empty((n, self.F), dtype=numpy.float32)
        self.lib.check(self.lib.dll.ry_vc_mid_sp(self.handle, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(rows), n,
                                                 float(sp_floor), _lib._fptr(sp)))
        return sp

    def close(self):
        """`ry_vc_destroy` dereferences both predictors (their context, the lane clones): it only runs while both are alive.  `Net.close`
        closes its dependent cores first, so the order the caller closes things in does not matter."""
        if (self.handle is not None and self.stage1.handle is not None and self.stage2.handle is not None
                and self.stage1.ctx.handle is not None and self.stage1.ctx.pid == os.getpid()):
            self.lib.dll.ry_vc_destroy(self.handle)
        self.handle = None
        self.stage1._dependents.discard(self); self.stage2._dependents.discard(self)

    def alive_on(self, stage1: 'Net', stage2: 'Net') -> bool:
        """True while this core is open and still sits on exactly these two (open) predictors."""
        return (self.handle is not None and self.stage1 is stage1 and self.stage2 is stage2
                and stage1.handle is not None and stage2.handle is not None)


_contexts: Dict = {}


def get_context(device: int = 0, lib: Optional[_lib.Ry355Lib] = None) -> Context:
    """Per-(pid, device) context, created on first use in the calling process (fork-safe laziness)."""
    key = (os.getpid(), int(device), id(lib) if lib is not None else 0)
    ctx = _contexts.get(key)
    if ctx is None:
        ctx = Context(device, lib)
        _contexts[key] = ctx
    return ctx


def set_filter_build(mode: str, lib: Optional[_lib.Ry355Lib] = None):
    """Where the filter layouts of the predictors created from now on are built (`ry_set_filter_build`, process-wide): 'host' (the default: host
    loops, one upload per layout, the Winograd filters by way of a download) or 'device' (one upload of each raw filter, layout kernels on the
    card; the same bits).  The environment variable RY_FILTER_BUILD=host|device sets the same switch when a context is created
    or `Context.reload_env` runs; the compat shims follow the variable only.  lib: another build of the library (tests: the emulator)."""
    if mode not in _lib.FILTER_BUILD:
        raise ValueError("filter build mode must be 'host' or 'device', got %r" % (mode,))
    lib = lib if lib is not None else _lib.default_lib()
    lib.check(lib.dll.ry_set_filter_build(_lib.FILTER_BUILD[mode]))


class Net(object):
    """A predictor resident on one GPU.  `blob` = flat float32 weights (netspec K-list order), either a
    host ndarray or (ptr, n) of a device buffer (e.g. the tensor an RCCL broadcast filled)."""

    def __init__(self, ctx: Context, desc: NetDesc, blob, width: int = 512, bn_eps: float = 2e-5, lrelu_slope: float = 0.2):
        self.ctx = ctx
        self.desc = desc
        self.width = int(width) if desc.ndim == 2 else 1
        self.cdesc = _lib.RyNetDesc(desc.ndim, desc.in_ch, desc.out_ch, desc.base, desc.extensive_layers, self.width,
                                    bn_eps, lrelu_slope, int(bool(desc.glu)))
        lib = ctx.lib
        want = int(lib.dll.ry_net_param_count(ctypes.byref(self.cdesc)))
        if want != param_count(desc):
            raise _lib.Ry355Error('library and netspec disagree on the parameter count: %d vs %d' % (want, param_count(desc)))
        h = ctypes.c_void_p()
        if isinstance(blob, tuple):
            ptr, n = blob
            lib.check(lib.dll.ry_net_create(ctx.handle, ctypes.byref(self.cdesc), _lib._fptr(int(ptr)), int(n), 1, ctypes.byref(h)))
        else:
            blob = numpy.ascontiguousarray(blob, dtype=numpy.float32)
            lib.check(lib.dll.ry_net_create(ctx.handle, ctypes.byref(self.cdesc), _lib._fptr(blob), blob.size, 0, ctypes.byref(h)))
        self.handle = h
        self._dependents = weakref.WeakSet()                  # VcCores built on this predictor (they hold raw pointers to it)

    def set_dtype(self, dtype: str):
        """'f32' (exact fp32 MFMA, default), 'bf16' (stage-2 only: bf16 operands, fp32 accumulate -- BASELINE config #5) or
        'bf16x3' (stage-2 only: every fp32 product as three bf16 products hi*hi + lo*hi + hi*lo on the bf16 matrix pipe, fp32
        accumulate -- fp32-class results)."""
        self.ctx.lib.check(self.ctx.lib.dll.ry_net_set_dtype(self.handle, {'f32': 0, 'bf16': 1, 'bf16x3': 2}[dtype]))

    def close(self):
        for core in list(self._dependents):                    # a window core on a freed predictor is a use-after-free in `ry_vc_*`: it goes first
            core.close()
        if self.handle is not None and self.ctx.handle is not None and self.ctx.pid == os.getpid():
            self.ctx.lib.dll.ry_net_destroy(self.handle)
        self.handle = None

    # ---- host-array API ----
    def forward(self, x: numpy.ndarray) -> numpy.ndarray:
        """Raw predictor on a padded block.  stage-1: (B, T, in_ch) -> (B, T, out_ch); stage-2: (B, T, width) -> same."""
        x = numpy.ascontiguousarray(x, dtype=numpy.float32)
        B, T = x.shape[0], x.shape[1]
        cin = self.desc.in_ch if self.desc.ndim == 1 else self.width
        cout = self.desc.out_ch if self.desc.ndim == 1 else self.width
        if x.shape != (B, T, cin):
            raise ValueError('expected (B, T, %d), got %s' % (cin, x.shape))
        y = numpy.empty((B, T, cout), dtype=numpy.float32)
        self.ctx.lib.check(self.ctx.lib.dll.ry_net_forward(self.handle, _lib._fptr(x), _lib._fptr(y), B, T, 0))
        return y

    def convert(self, x: numpy.ndarray, discard=(0, 0)) -> numpy.ndarray:
        """The wrapper arithmetic + predictor: stage-1 `AcousticConverter.convert` array part
        ((B,) N, in_ch) -> ((B,) N, out_ch); stage-2 `SuperResolution.convert` ((B,) N, width+1) -> same.
        discard = (front, back), stage 2 only: the caller will throw away that many leading / trailing frames of every window
        (`ry_sr_convert_rows`): they are not computed and come back as zeros, the others are bit-identical to the full call."""
        x = numpy.ascontiguousarray(x, dtype=numpy.float32)
        squeeze = x.ndim == 2
        if squeeze:
            x = x[numpy.newaxis]
        B, N, C = x.shape
        if self.desc.ndim == 1:
            if C != self.desc.in_ch:
                raise ValueError('stage-1 input needs %d channels, got %d' % (self.desc.in_ch, C))
            y = numpy.empty((B, N, self.desc.out_ch), dtype=numpy.float32)
            fn = self.ctx.lib.dll.ry_ac_convert
        else:
            if C != self.width + 1:
                raise ValueError('stage-2 input needs %d bins, got %d' % (self.width + 1, C))
            y = numpy.empty((B, N, C), dtype=numpy.float32)
            fn = self.ctx.lib.dll.ry_sr_convert
        if self.desc.ndim == 2 and tuple(discard) != (0, 0):
            self.ctx.lib.check(self.ctx.lib.dll.ry_sr_convert_rows(self.handle, _lib._fptr(x), _lib._fptr(y), B, N, int(discard[0]), int(discard[1]), 0))
        else:
            self.ctx.lib.check(fn(self.handle, _lib._fptr(x), _lib._fptr(y), B, N, 0))
        return y[0] if squeeze else y

    # ---- device-pointer API (inputs already resident in HBM; only enqueues on the context stream) ----
    def forward_device(self, x_ptr: int, y_ptr: int, batch: int, frames: int):
        self.ctx.lib.check(self.ctx.lib.dll.ry_net_forward(self.handle, _lib._fptr(int(x_ptr)), _lib._fptr(int(y_ptr)), batch, frames, 1))

    def convert_device(self, x_ptr: int, y_ptr: int, batch: int, n_frames: int):
        fn = self.ctx.lib.dll.ry_ac_convert if self.desc.ndim == 1 else self.ctx.lib.dll.ry_sr_convert
        self.ctx.lib.check(fn(self.handle, _lib._fptr(int(x_ptr)), _lib._fptr(int(y_ptr)), batch, n_frames, 1))

    def debug_activation(self, layer: int, kind: int = 0) -> numpy.ndarray:
        """Tests: one buffer of the plan that ran last on this handle (`ry_net_debug_activation`).  layer -1: the convert wrapper's padded input
        (B, T, cols) float32; layer 0 .. 15 (stage 2): kind 0 the fp32 output (B, Ho, Wo, Cout), kind 1 its 16-bit copy as raw uint16, (B, Ho, Wo, Cout)
        plain bf16 or (B, Ho, Wo, 2, Cout) split-bf16 [hi | lo].  Raises `Ry355Error` when the plan has no such buffer."""
        lib = self.ctx.lib
        dims = (ctypes.c_int * 5)()
        lib.check(lib.dll.ry_net_debug_activation(self.handle, int(layer), int(kind), None, 0, dims))
        B, H, W, C, fmt = (int(v) for v in dims)
        out = numpy.empty((B, H, W, C), dtype=numpy.float32 if fmt == 0 else numpy.uint16)
        lib.check(lib.dll.ry_net_debug_activation(self.handle, int(layer), int(kind), out.ctypes.data_as(ctypes.c_void_p), out.nbytes, dims))
        if layer < 0:
            return out[..., 0]
        return out.reshape(B, H, W, 2, C // 2) if fmt == 2 else out

    def debug_plan(self, batch: int, frames: int, window: bool = False, discard=(0, 0)) -> List[dict]:
        """Tests: the stage-2 launch plan of (batch, frames), one dict per layer with the fields of `ry_plan_record` (`ry_net_debug_plan`): built if it
        does not exist yet, nothing is enqueued.  window=True: the convert wrapper on `frames` real frames (discard as in `convert`); False: the raw
        forward at `frames` padded rows."""
        recs = (_lib.RyPlanRecord * 16)()
        n = ctypes.c_int()
        self.ctx.lib.check(self.ctx.lib.dll.ry_net_debug_plan(self.handle, int(batch), int(frames), int(bool(window)), int(discard[0]), int(discard[1]),
                                                             recs, 16, ctypes.byref(n)))
        return [{f: (tuple(getattr(recs[i], f)) if f == 'os2' else int(getattr(recs[i], f))) for f in _lib.RyPlanRecord.FIELDS} for i in range(n.value)]

    def build_stats(self) -> dict:
        """What building this predictor's filters has taken so far (`ry_net_build_stats`): bytes_uploaded, bytes_downloaded, layout_launches,
        host_relayout_floats, arena_bytes.  The clones of a predictor share the counters; lazy Winograd builds go on counting."""
        st = _lib.RyBuildStats()
        self.ctx.lib.check(self.ctx.lib.dll.ry_net_build_stats(self.handle, ctypes.byref(st)))
        return {f: int(getattr(st, f)) for f in _lib.RyBuildStats.FIELDS}

    def debug_filters(self, layer: int, kind: str) -> numpy.ndarray:
        """Tests: one filter layout of layer 0 .. 15 as it lies on the card (`ry_net_debug_filters`), flat float32.  kind: 'w1d', 'w1os' (stage 1),
        'wig', 'wdir', 'w2os', 'wwin' (stage 2; 'wwin' is built on demand in the filter build mode in force).  Raises `Ry355Error` when the layer has
        no such layout."""
        lib = self.ctx.lib
        n = ctypes.c_size_t(0)
        rc = lib.dll.ry_net_debug_filters(self.handle, int(layer), _lib.FILTER_KINDS[kind], None, 0, ctypes.byref(n))
        if n.value == 0:                                     # (the size query itself is refused with the size set: anything else is an error)
            lib.check(rc)
        out = numpy.empty(n.value, dtype=numpy.float32)
        lib.check(lib.dll.ry_net_debug_filters(self.handle, int(layer), _lib.FILTER_KINDS[kind], _lib._fptr(out), out.size, ctypes.byref(n)))
        return out

    def profile(self, batch: int, frames: int, reps: int = 5, window: bool = False) -> List[dict]:
        """Per-launch timings of the raw forward at `frames` padded rows, or (window=True) of the convert wrapper on one window
        of `frames` real frames -- what the window call runs."""
        stats = (_lib.RyKernelStat * 96)()
        n = ctypes.c_int()
        if window:
            self.ctx.lib.check(self.ctx.lib.dll.ry_net_profile_window(self.handle, frames, reps, stats, 96, ctypes.byref(n)))
        else:
            self.ctx.lib.check(self.ctx.lib.dll.ry_net_profile(self.handle, batch, frames, reps, stats, 96, ctypes.byref(n)))
        return [dict(name=stats[i].name.decode(), layer=stats[i].layer.decode(), ms=float(stats[i].ms),
                     flops=float(stats[i].flops), bytes=float(stats[i].bytes), grid=tuple(stats[i].grid), flops_exec=float(stats[i].flops_exec))
                for i in range(n.value)]
