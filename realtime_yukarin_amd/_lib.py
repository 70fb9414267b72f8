"""ctypes binding of libry355.so (C ABI: include/ry355.h).

This is the whole host<->device boundary: plain pointers and sizes, no torch types.  The product
library is `realtime_yukarin_amd/libry355.so`, built in-tree by `__graft_entry__.build()`
(hipcc --offload-arch=gfx950).  There is NO CPU fallback: if the library is missing or no GPU is
visible, every entry point of this package raises.  (tests/ may bind a different path -- the
host-side SIMT emulator build of the same sources -- by constructing `Ry355Lib(path)` explicitly;
nothing in this package ever does.)
"""
import ctypes
import os
from pathlib import Path

import numpy

LIB_NAME = 'libry355.so'
DEFAULT_LIB_PATH = Path(__file__).resolve().parent / LIB_NAME

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_GLU = 0, 1, 2, 3
ACTS = {None: ACT_NONE, 'none': ACT_NONE, 'lrelu': ACT_LRELU, 'relu': ACT_RELU, 'glu': ACT_GLU}
PATH_AUTO, PATH_IGEMM, PATH_DIRECT = 0, 1, 2
TILES = {None: 0, 'auto': 0, '128x128': 1, '64x128': 3, '32x128': 4, '128x64': 5, '96x128': 6}
TILES.update({k + 'k2': v + 16 for k, v in list(TILES.items()) if isinstance(k, str) and k != 'auto'})   # two K groups per workgroup
TILES.update({k + 'k1': v + 32 for k, v in list(TILES.items()) if isinstance(k, str) and k[-2:] != 'k2' and k != 'auto'})           # force one

def ensure_hw_queues() -> None:
    """The window call runs up to two windows side by side on HIP streams of their own (ry_vc_set_lanes): streams only overlap when each
    has a hardware queue of its own.  ROCm hands out GPU_MAX_HW_QUEUES of them (4 by default) and folds further streams onto queues that
    are taken, in the order the streams were created.  With 16, every stream of the wide topology (a stage-1 and a stage-2 stream per lane)
    has a queue.  With 4 and two lanes (measured on MI355X, profiles/r16/queues_parent.txt) the wide topology leaves the second lane's two
    streams on one queue -- 0.878 against 0.813 ms per window -- so the core then enqueues on three streams (`ry_vc_create` reads the
    variable; one stage-1 stream for both lanes beside the two stage-2 streams; profiles/r16/queues_ab.txt), which with the context stream
    fill the four queues: nothing else of the process may hold a queue busy (the null stream of a torch process that launches on it).
    The HIP runtime reads the variable when it starts, so it is set when the product library is BOUND (`Ry355Lib.__init__`: the first
    GPU context of the process, `engine.get_context`) -- not at import: importing the package changes nothing.  The entry points
    (bench.py, the worker processes of `dispatch`) set it themselves before anything else.  A caller's own value is respected.  A runtime
    that is already up keeps the queues it started with: the variable is then left alone, and the core takes the compact topology of the
    default 4."""
    if 'GPU_MAX_HW_QUEUES' in os.environ:
        return
    import sys
    t = sys.modules.get('torch')
    try:
        late = t is not None and t.cuda.is_initialized()
    except Exception:
        late = False
    if not late:
        os.environ['GPU_MAX_HW_QUEUES'] = '16'


# every symbol include/ry355.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = (
    'ry_init', 'ry_shutdown', 'ry_sync', 'ry_stream', 'ry_device_count', 'ry_last_error',
    'ry_net_param_count', 'ry_net_create', 'ry_net_destroy', 'ry_net_clone', 'ry_net_set_dtype', 'ry_net_forward',
    'ry_ac_convert', 'ry_sr_convert', 'ry_sr_convert_rows', 'ry_conv1d', 'ry_conv1d_os', 'ry_conv2d', 'ry_conv2d_dilated',
    'ry_timer_start', 'ry_timer_stop', 'ry_net_profile', 'ry_net_profile_window', 'ry_net_debug_activation', 'ry_net_debug_plan', 'ry_debug_plan_igemm', 'ry_debug_reload_env', 'ry_debug_stream_overlap', 'ry_debug_plan_igemm_bf16', 'ry_debug_plan_os2', 'ry_debug_plan_wino',
    'ry_vc_create', 'ry_vc_destroy', 'ry_vc_convert', 'ry_mc2sp',
    'ry_vc_submit', 'ry_vc_set_lanes', 'ry_vc_set_discard', 'ry_vc_wait', 'ry_vc_enqueue_device', 'ry_vc_enqueue_device_batch', 'ry_vc_stage1', 'ry_vc_stage2_from_mc', 'ry_vc_mid_sp', 'ry_vc_reserve_frames',
    'ry_vc_submit_wave', 'ry_vc_wait_wave', 'ry_vc_gate', 'ry_vc_debug_streams',
    'ry_comm_unique_id', 'ry_comm_init', 'ry_comm_destroy', 'ry_comm_bcast_weights', 'ry_comm_allreduce_max', 'ry_comm_barrier',
    'ry_dev_alloc', 'ry_dev_free', 'ry_dev_upload', 'ry_dev_download',
    'ry_crepe_param_count', 'ry_crepe_create', 'ry_crepe_destroy', 'ry_crepe_predict', 'ry_crepe_decode', 'ry_crepe_set_viterbi_tables',
    'ry_crepe_debug_layer', 'ry_crepe_debug_splits', 'ry_crepe_debug_poison',
    'ry_crepe_set_resampler', 'ry_crepe_resample', 'ry_crepe_predict_sr', 'ry_crepe_set_dtype',
    'ry_crepe_voicing', 'ry_crepe_set_voicing_tables', 'ry_crepe_track', 'ry_crepe_track_buffers',
    'ry_crepe_track_many', 'ry_crepe_track_many_buffers', 'ry_crepe_decode_many', 'ry_crepe_voicing_many', 'ry_analysis_extract_many_dev',
    'ry_crepe_stream_create', 'ry_crepe_stream_destroy', 'ry_crepe_stream_reset', 'ry_crepe_stream_track', 'ry_crepe_stream_activation',
    'ry_crepe_stream_debug_poison', 'ry_crepe_stream_debug_assemble',
    'ry_crepe_bank_create', 'ry_crepe_bank_destroy', 'ry_crepe_bank_reset', 'ry_crepe_bank_track', 'ry_crepe_bank_activation',
    'ry_crepe_bank_debug_poison', 'ry_crepe_bank_debug_uploads', 'ry_crepe_bank_debug_assemble',
    'ry_synth_create', 'ry_synth_destroy', 'ry_synth_length', 'ry_synth_run', 'ry_synth_bound', 'ry_synth_push', 'ry_synth_flush', 'ry_synth_reset',
    'ry_synth_debug_pulses', 'ry_synth_debug_poison', 'ry_synth_run_many', 'ry_synth_debug_pulses_many',
    'ry_synth_bank_create', 'ry_synth_bank_destroy', 'ry_synth_bank_bound', 'ry_synth_bank_push', 'ry_synth_bank_reset',
    'ry_synth_bank_debug_pulses', 'ry_synth_bank_debug_poison', 'ry_synth_bank_debug_counts', 'ry_synth_bank_debug_rows',
    'ry_analysis_create', 'ry_analysis_destroy', 'ry_analysis_run', 'ry_analysis_sp2mc', 'ry_analysis_debug_record', 'ry_analysis_debug_ints', 'ry_analysis_debug_poison',
    'ry_analysis_d4c', 'ry_analysis_extract', 'ry_analysis_d4c_bands', 'ry_analysis_debug_d4c', 'ry_analysis_extract_dev',
    'ry_analysis_extract_resident', 'ry_vc_enqueue_wave_device', 'ry_mask_rows',
    'ry_analysis_extract_many_resident', 'ry_vc_gate_waves_device', 'ry_vc_enqueue_waves_device', 'ry_gather_rows',
    'ry_vc_gate_verdict_waves_device', 'ry_vc_compact_waves_device', 'ry_vc_enqueue_waves_masked_device', 'ry_analysis_extract_spans_resident',
    'ry_crepe_upload_waves', 'ry_crepe_track_uploaded', 'ry_crepe_uploaded_buffers', 'ry_crepe_bank_track_uploaded', 'ry_crepe_debug_frames',
    'ry_outgate_create', 'ry_outgate_destroy', 'ry_outgate_reset', 'ry_outgate_push', 'ry_outgate_held', 'ry_outgate_debug_counts', 'ry_outgate_debug_poison',
    'ry_outgate_bank_create', 'ry_outgate_bank_destroy', 'ry_outgate_bank_reset', 'ry_outgate_bank_push', 'ry_outgate_bank_held',
    'ry_outgate_bank_debug_counts', 'ry_outgate_bank_debug_poison',
    'ry_synth_push_dev', 'ry_synth_flush_dev', 'ry_synth_bank_push_dev', 'ry_outgate_debug_upload_bytes', 'ry_outgate_bank_debug_upload_bytes',
    'ry_analysis_upload_waves', 'ry_analysis_ingest_tracks', 'ry_analysis_track_buffers',
    'ry_set_filter_build', 'ry_net_build_stats', 'ry_net_debug_filters', 'ry_debug_layer_filters',
    'ry_rowstore_create', 'ry_rowstore_destroy', 'ry_rowstore_append', 'ry_rowstore_retire', 'ry_rowstore_held', 'ry_rowstore_fetch', 'ry_rowstore_reset',
    'ry_rowstore_debug_buffers', 'ry_rowstore_debug_counts', 'ry_rowstore_debug_poison',
    'ry_rowbank_create', 'ry_rowbank_destroy', 'ry_rowbank_append', 'ry_rowbank_fetch', 'ry_rowbank_pick_ap', 'ry_rowbank_retire', 'ry_rowbank_reset',
    'ry_rowbank_held', 'ry_rowbank_debug_buffers', 'ry_rowbank_debug_counts', 'ry_rowbank_debug_poison',
)


class RyNetDesc(ctypes.Structure):
    _fields_ = [('ndim', ctypes.c_int), ('in_ch', ctypes.c_int), ('out_ch', ctypes.c_int),
                ('base', ctypes.c_int), ('extensive_layers', ctypes.c_int), ('width', ctypes.c_int),
                ('bn_eps', ctypes.c_float), ('lrelu_slope', ctypes.c_float), ('glu', ctypes.c_int)]


class RyKernelStat(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char * 48), ('layer', ctypes.c_char * 24), ('ms', ctypes.c_float),
                ('flops', ctypes.c_double), ('bytes', ctypes.c_double), ('grid', ctypes.c_int * 3), ('flops_exec', ctypes.c_double)]


class RyPlanRecord(ctypes.Structure):
    """ry_plan_record (include/ry355.h): all ints, in the header's order"""
    FIELDS = ('layer', 'path', 'tile', 'splits', 'kgroups', 'wino_cfg', 'wino_mbw', 'os2', 'reads16', 'writes32', 'writes16', 'patch', 'reduce', 'last_exp',
              'rows_out', 'grid_rows', 'grid_cols', 'tile_rows', 'tile_cols', 'out_lo', 'out_n', 'crop_lo', 'crop_n', 'hole_lo', 'hole_n')
    _fields_ = [(f, ctypes.c_int * 4 if f == 'os2' else ctypes.c_int) for f in FIELDS]


class RyBuildStats(ctypes.Structure):
    """ry_build_stats (include/ry355.h): unsigned 64-bit counters, in the header's order"""
    FIELDS = ('bytes_uploaded', 'bytes_downloaded', 'layout_launches', 'host_relayout_floats', 'arena_bytes')
    _fields_ = [(f, ctypes.c_ulonglong) for f in FIELDS]


FILTER_BUILD = {'host': 0, 'device': 1}
FILTER_KINDS = {'w1d': 0, 'w1os': 1, 'wig': 2, 'wdir': 3, 'w2os': 4, 'wwin': 5}


class Ry355Error(RuntimeError):
    pass


_FP = ctypes.POINTER(ctypes.c_float)
_VP = ctypes.c_void_p


def _fptr(a):
    """float* of a C-contiguous float32 ndarray, or a raw device address (int)."""
    if isinstance(a, int):
        return ctypes.cast(ctypes.c_void_p(a), _FP)
    if a is None:
        return ctypes.cast(ctypes.c_void_p(0), _FP)
    assert isinstance(a, numpy.ndarray) and a.dtype == numpy.float32 and a.flags['C_CONTIGUOUS'], \
        'expected a C-contiguous float32 array'
    return a.ctypes.data_as(_FP)


class Ry355Lib(object):
    def __init__(self, path=None):
        path = Path(path) if path is not None else DEFAULT_LIB_PATH
        if not path.exists():
            raise Ry355Error(
                '%s not found: the MI355X HIP library is not built (run `python -c "import __graft_entry__ as g; '
                'g.build()"` at the repo root). This package has no CPU fallback.' % path)
        self.path = path
        ensure_hw_queues()
        self.dll = ctypes.CDLL(str(path))
        d = self.dll
        d.ry_last_error.restype = ctypes.c_char_p
        d.ry_init.argtypes = [ctypes.c_int, ctypes.POINTER(_VP)]
        d.ry_shutdown.argtypes = [_VP]
        d.ry_shutdown.restype = None
        d.ry_sync.argtypes = [_VP]
        d.ry_stream.argtypes = [_VP]
        d.ry_stream.restype = _VP
        d.ry_device_count.restype = ctypes.c_int
        d.ry_net_param_count.argtypes = [ctypes.POINTER(RyNetDesc)]
        d.ry_net_param_count.restype = ctypes.c_size_t
        d.ry_net_create.argtypes = [_VP, ctypes.POINTER(RyNetDesc), _FP, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(_VP)]
        d.ry_net_destroy.argtypes = [_VP]
        d.ry_net_set_dtype.argtypes = [_VP, ctypes.c_int]
        d.ry_net_destroy.restype = None
        d.ry_net_forward.argtypes = [_VP, _FP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        d.ry_ac_convert.argtypes = [_VP, _FP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        d.ry_sr_convert.argtypes = [_VP, _FP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        d.ry_conv1d.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _FP, _FP, _FP] + [ctypes.c_int] * 8 + [_FP]
        d.ry_conv1d_os.argtypes = [_VP, _FP, _FP] + [ctypes.c_int] * 4 + [_FP, _FP, _FP] + [ctypes.c_int] * 10 + [_FP]
        d.ry_conv2d.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _FP, _FP, _FP] + [ctypes.c_int] * 9 + [_FP]
        d.ry_conv2d_dilated.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _FP, _FP, _FP] + [ctypes.c_int] * 10 + [_FP]
        d.ry_vc_create.argtypes = [_VP, _VP, _FP, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_VP)]
        d.ry_vc_destroy.argtypes = [_VP]
        d.ry_vc_destroy.restype = None
        d.ry_vc_convert.argtypes = [_VP, _FP, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_float, _FP, _FP]
        d.ry_mc2sp.argtypes = [_VP, _FP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, _FP]
        _IP = ctypes.POINTER(ctypes.c_int)
        d.ry_vc_submit.argtypes = [_VP, _FP, _IP, ctypes.c_int, ctypes.c_int, ctypes.c_float, _IP]
        d.ry_vc_wait.argtypes = [_VP, ctypes.c_int, _FP, _FP]
        d.ry_vc_set_lanes.argtypes = [_VP, ctypes.c_int]
        d.ry_vc_debug_streams.argtypes = [_VP, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        d.ry_vc_set_discard.argtypes = [_VP, ctypes.c_int, ctypes.c_int]
        d.ry_sr_convert_rows.argtypes = [_VP, _FP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        d.ry_debug_stream_overlap.argtypes = [_VP, ctypes.c_int, ctypes.c_int, _FP]
        d.ry_net_clone.argtypes = [_VP, ctypes.POINTER(ctypes.c_void_p)]
        d.ry_vc_enqueue_device.argtypes = [_VP, _FP, _IP, ctypes.c_int, ctypes.c_int, ctypes.c_float, _FP, _FP]
        d.ry_vc_enqueue_device_batch.argtypes = [_VP, ctypes.c_int, _FP, _IP, _IP, ctypes.c_int, ctypes.c_float, _FP, _FP]
        d.ry_vc_stage1.argtypes = [_VP, _FP, ctypes.c_int, _FP]
        d.ry_vc_stage2_from_mc.argtypes = [_VP, _IP, ctypes.c_int, ctypes.c_int, ctypes.c_float, _FP]
        d.ry_vc_mid_sp.argtypes = [_VP, _IP, ctypes.c_int, ctypes.c_int, ctypes.c_float, _FP]
        d.ry_vc_reserve_frames.argtypes = [_VP, ctypes.c_int]
        d.ry_vc_submit_wave.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, _FP, ctypes.c_int,
                                        ctypes.c_float, _IP]
        d.ry_vc_wait_wave.argtypes = [_VP, ctypes.c_int, _FP, _FP, ctypes.POINTER(ctypes.c_ubyte), _IP]
        d.ry_vc_gate.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, _FP, ctypes.c_int,
                                 ctypes.POINTER(ctypes.c_ubyte), _IP, _FP, _IP]
        d.ry_comm_unique_id.argtypes = [ctypes.c_char_p]
        d.ry_comm_init.argtypes = [_VP, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_VP)]
        d.ry_comm_destroy.argtypes = [_VP]
        d.ry_comm_destroy.restype = None
        d.ry_comm_bcast_weights.argtypes = [_VP, _FP, ctypes.c_size_t, ctypes.c_int]
        d.ry_comm_allreduce_max.argtypes = [_VP, ctypes.POINTER(ctypes.c_double)]
        d.ry_comm_barrier.argtypes = [_VP]
        d.ry_dev_alloc.argtypes = [_VP, ctypes.c_size_t, ctypes.POINTER(_FP)]
        d.ry_dev_free.argtypes = [_VP, _FP]
        d.ry_dev_upload.argtypes = [_VP, _FP, _FP, ctypes.c_size_t]
        d.ry_dev_download.argtypes = [_VP, _FP, _FP, ctypes.c_size_t]
        d.ry_timer_start.argtypes = [_VP]
        d.ry_timer_stop.argtypes = [_VP, ctypes.POINTER(ctypes.c_float)]
        d.ry_net_profile.argtypes = [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RyKernelStat),
                                     ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        _DP = ctypes.POINTER(ctypes.c_double)
        d.ry_crepe_param_count.argtypes = [ctypes.c_int]
        d.ry_crepe_param_count.restype = ctypes.c_size_t
        d.ry_crepe_create.argtypes = [_VP, ctypes.c_int, _FP, ctypes.c_size_t, ctypes.c_float, ctypes.POINTER(_VP)]
        d.ry_crepe_destroy.argtypes = [_VP]
        d.ry_crepe_destroy.restype = None
        d.ry_crepe_predict.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _FP, _FP, _FP, ctypes.c_int]
        d.ry_crepe_decode.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, _FP, _FP, ctypes.POINTER(ctypes.c_int)]
        d.ry_crepe_set_viterbi_tables.argtypes = [_VP, _DP, _DP, _DP]
        d.ry_crepe_set_resampler.argtypes = [_VP, ctypes.c_int, _DP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _DP, ctypes.c_int]
        d.ry_crepe_resample.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, _FP, ctypes.c_int]
        d.ry_crepe_predict_sr.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _FP, _FP, _FP, ctypes.c_int]
        d.ry_crepe_debug_layer.argtypes = [_VP, ctypes.c_int, ctypes.c_int, _FP]
        d.ry_crepe_debug_poison.argtypes = [_VP]
        d.ry_crepe_set_dtype.argtypes = [_VP, ctypes.c_int]
        d.ry_crepe_debug_splits.argtypes = [_VP, ctypes.POINTER(ctypes.c_int)]
        _UB = ctypes.POINTER(ctypes.c_ubyte)
        d.ry_crepe_set_voicing_tables.argtypes = [_VP, _DP, _DP, _DP, _DP, _DP]
        d.ry_crepe_voicing.argtypes = [_VP, _FP, _FP, ctypes.c_int, ctypes.c_double, ctypes.c_double, _UB, _DP, _DP, ctypes.c_int]
        d.ry_crepe_track.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, _IP, _UB, _DP, _DP, ctypes.c_int]
        d.ry_crepe_track_buffers.argtypes = [_VP, ctypes.POINTER(_VP), _IP, _IP, ctypes.POINTER(_VP), ctypes.POINTER(_VP), ctypes.POINTER(_VP)]
        _LLPP, _IPP = ctypes.POINTER(ctypes.POINTER(ctypes.c_longlong)), ctypes.POINTER(_IP)
        d.ry_crepe_track_many.argtypes = [_VP, _FP, _IP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, _IP, _UB, _DP, _DP, ctypes.c_int]
        d.ry_crepe_track_many_buffers.argtypes = [_VP, ctypes.POINTER(_VP), _IP, _LLPP, _IPP, ctypes.POINTER(_VP), ctypes.POINTER(_VP), ctypes.POINTER(_VP)]
        d.ry_crepe_decode_many.argtypes = [_VP, _FP, _IP, ctypes.c_int, ctypes.c_int, _FP, _FP, _IP]
        d.ry_crepe_voicing_many.argtypes = [_VP, _FP, _FP, _IP, ctypes.c_int, ctypes.c_double, ctypes.c_double, _UB, _DP, _DP, ctypes.c_int]
        d.ry_crepe_stream_create.argtypes = [_VP, ctypes.POINTER(_VP)]
        d.ry_crepe_stream_destroy.argtypes = [_VP]
        d.ry_crepe_stream_destroy.restype = None
        d.ry_crepe_stream_reset.argtypes = [_VP]
        d.ry_crepe_stream_track.argtypes = [_VP, _FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                            _IP, _IP, _UB, _DP, _DP, ctypes.c_int]
        d.ry_crepe_stream_activation.argtypes = [_VP, _FP, ctypes.c_int]
        d.ry_crepe_stream_debug_poison.argtypes = [_VP, _IP]
        d.ry_crepe_stream_debug_assemble.argtypes = [_VP, _FP, ctypes.c_int, _FP, ctypes.c_int, _IP, ctypes.c_int, _FP]
        d.ry_crepe_bank_create.argtypes = [_VP, ctypes.c_int, ctypes.POINTER(_VP)]
        d.ry_crepe_bank_destroy.argtypes = [_VP]
        d.ry_crepe_bank_destroy.restype = None
        d.ry_crepe_bank_reset.argtypes = [_VP, ctypes.c_int]
        d.ry_crepe_bank_track.argtypes = [_VP, _FP, _IP, _IP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, _IP, _IP,
                                          _IP, _IP, _UB, _DP, _DP, ctypes.c_int]
        d.ry_crepe_bank_activation.argtypes = [_VP, ctypes.c_int, _FP, ctypes.c_int]
        d.ry_crepe_bank_debug_poison.argtypes = [_VP, _IP]
        d.ry_crepe_bank_debug_uploads.argtypes = [_VP, ctypes.POINTER(ctypes.c_longlong)]
        d.ry_crepe_bank_debug_assemble.argtypes = [_VP, _IP, ctypes.c_int, ctypes.POINTER(_VP), _IP, ctypes.POINTER(_VP), _FP, ctypes.c_int, _IP, _FP]
        _CI = ctypes.c_int
        d.ry_synth_create.argtypes = [_VP, _CI, ctypes.c_double, _CI, ctypes.c_uint, ctypes.POINTER(_VP)]
        d.ry_synth_destroy.argtypes = [_VP]
        d.ry_synth_destroy.restype = None
        d.ry_synth_length.argtypes = [_VP, _CI]
        d.ry_synth_bound.argtypes = [_VP, _CI, _CI]
        d.ry_synth_run.argtypes = [_VP, _DP, _FP, _FP, _CI, _CI, _CI, _DP, _CI, _IP]
        d.ry_synth_push.argtypes = [_VP, _DP, _FP, _FP, _CI, _CI, _CI, _DP, _CI, _IP]
        d.ry_synth_flush.argtypes = [_VP, _DP, _CI, _IP]
        d.ry_synth_reset.argtypes = [_VP]
        d.ry_synth_push_dev.argtypes = [_VP, _DP, _FP, _FP, _CI, _CI, _CI, _DP, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
        d.ry_synth_flush_dev.argtypes = [_VP, _DP, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
        d.ry_synth_debug_pulses.argtypes = [_VP, ctypes.POINTER(ctypes.c_longlong), _DP, _IP, _CI, _IP]
        d.ry_synth_debug_poison.argtypes = [_VP]
        d.ry_synth_run_many.argtypes = [_VP, _DP, _FP, _FP, _IP, _CI, _CI, _CI, _DP, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
        d.ry_synth_debug_pulses_many.argtypes = [_VP, _CI, ctypes.POINTER(ctypes.c_longlong), _DP, _IP, _CI, _IP]
        d.ry_synth_bank_create.argtypes = [_VP, _CI, ctypes.c_double, _CI, _CI, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(_VP)]
        d.ry_synth_bank_destroy.argtypes = [_VP]
        d.ry_synth_bank_destroy.restype = None
        d.ry_synth_bank_bound.argtypes = [_VP, _CI, _CI, _CI]
        d.ry_synth_bank_push.argtypes = [_VP, _DP, _FP, _FP, _IP, _IP, _CI, _CI, _DP, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
        d.ry_synth_bank_push_dev.argtypes = [_VP, _DP, _FP, _FP, _IP, _IP, _CI, _CI, _DP, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
        d.ry_synth_bank_reset.argtypes = [_VP, _CI]
        d.ry_synth_bank_debug_pulses.argtypes = [_VP, _CI, ctypes.POINTER(ctypes.c_longlong), _DP, _IP, _CI, _IP]
        d.ry_synth_bank_debug_poison.argtypes = [_VP]
        d.ry_synth_bank_debug_counts.argtypes = [_VP, _IP]
        d.ry_synth_bank_debug_rows.argtypes = [_VP, _CI]
        _LL = ctypes.c_longlong
        d.ry_analysis_create.argtypes = [_VP, _CI, _CI, _CI, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_uint, ctypes.POINTER(_VP)]
        d.ry_analysis_destroy.argtypes = [_VP]
        d.ry_analysis_destroy.restype = None
        d.ry_analysis_run.argtypes = [_VP, _DP, _LL, _DP, _DP, _CI, _DP, _FP, _DP]
        d.ry_analysis_sp2mc.argtypes = [_VP, _VP, _CI, _CI, _DP]
        d.ry_analysis_debug_record.argtypes = [_VP, _CI]
        d.ry_analysis_debug_ints.argtypes = [_VP, ctypes.POINTER(_LL), _CI, _IP]
        d.ry_analysis_debug_poison.argtypes = [_VP]
        d.ry_analysis_d4c.argtypes = [_VP, _DP, _LL, _DP, _DP, _CI, ctypes.c_double, _DP, _FP, _DP]
        d.ry_analysis_extract.argtypes = [_VP, _DP, _LL, _DP, _DP, _CI, ctypes.c_double, _DP, _FP, _DP, _DP, _FP, _DP]
        d.ry_analysis_extract_dev.argtypes = [_VP, _FP, _LL, _DP, _DP, _CI, ctypes.c_double, _DP, _FP, _DP, _DP, _FP, _DP]
        d.ry_analysis_extract_many_dev.argtypes = [_VP, _FP, ctypes.POINTER(_LL), _DP, _DP, _IP, _CI, ctypes.c_double, _DP, _FP, _DP, _DP, _FP, _DP]
        d.ry_analysis_extract_resident.argtypes = [_VP, _FP, _LL, _DP, _DP, _CI, ctypes.c_double, _FP, _FP, _FP]
        d.ry_vc_enqueue_wave_device.argtypes = [_VP, _FP, _CI, _CI, _CI, ctypes.c_float, ctypes.c_float, _FP, _CI, ctypes.c_float, _FP, _FP, _UB, _UB, _IP]
        d.ry_mask_rows.argtypes = [_VP, _FP, _UB, _CI, _CI, _CI, _CI, _VP]
        d.ry_analysis_extract_many_resident.argtypes = [_VP, _FP, ctypes.POINTER(_LL), _DP, _DP, _IP, _CI, ctypes.c_double, _FP, _FP, _FP]
        d.ry_gather_rows.argtypes = [_VP, _FP, _CI, _CI, _IP, _UB, _FP, _CI, _VP]
        d.ry_vc_gate_waves_device.argtypes = [_VP, _FP, ctypes.POINTER(_LL), _IP, _CI, _CI, _CI, ctypes.c_float, ctypes.c_float, _FP, _UB, _UB, _IP, _FP, _IP]
        d.ry_vc_enqueue_waves_device.argtypes = [_VP, _FP, ctypes.POINTER(_LL), _IP, _CI, _CI, _CI, ctypes.c_float, ctypes.c_float, _FP, ctypes.c_float,
                                                 _FP, _FP, _UB, _UB, _IP]
        d.ry_vc_gate_verdict_waves_device.argtypes = [_VP, _FP, ctypes.POINTER(_LL), _IP, _CI, _CI, _CI, ctypes.c_float, ctypes.c_float, _UB, _UB, _IP]
        d.ry_vc_compact_waves_device.argtypes = [_VP, _IP, _CI, _UB, _UB, _IP, _FP, _FP, _IP]
        d.ry_vc_enqueue_waves_masked_device.argtypes = [_VP, _IP, _CI, _FP, ctypes.c_float, _FP, _FP, _UB, _UB, _IP]
        d.ry_analysis_extract_spans_resident.argtypes = [_VP, _FP, _LL, ctypes.POINTER(_LL), _IP, _DP, _DP, _IP, _IP, _CI, ctypes.c_double, _FP, _FP, _FP]
        d.ry_crepe_upload_waves.argtypes = [_VP, _FP, _IP, _CI, _CI, ctypes.POINTER(_VP)]
        d.ry_crepe_track_uploaded.argtypes = [_VP, _IP, _IP, _CI, _CI, _CI, ctypes.c_double, ctypes.c_double, _IP, _UB, _DP, _DP, _CI]
        d.ry_crepe_uploaded_buffers.argtypes = [_VP, ctypes.POINTER(_VP), ctypes.POINTER(_LL), _IP, _IPP, ctypes.POINTER(_VP), ctypes.POINTER(_VP),
                                                ctypes.POINTER(_VP)]
        d.ry_crepe_bank_track_uploaded.argtypes = [_VP, _IP, _IP, _IP, _CI, _CI, _CI, ctypes.c_double, ctypes.c_double, _IP, _IP, _IP, _IP, _UB, _DP, _DP,
                                                   _CI]
        d.ry_crepe_debug_frames.argtypes = [_VP, ctypes.POINTER(_LL)]
        d.ry_analysis_upload_waves.argtypes = [_VP, _FP, _IP, _CI, ctypes.POINTER(_VP)]
        d.ry_analysis_ingest_tracks.argtypes = [_VP, _DP, _IP, _CI, ctypes.c_double]
        d.ry_analysis_track_buffers.argtypes = [_VP, ctypes.POINTER(_VP), _IP, _LLPP, _IP, _IPP, ctypes.POINTER(_VP), ctypes.POINTER(_VP), ctypes.POINTER(_VP)]
        d.ry_analysis_d4c_bands.argtypes = [_VP]
        _LLP = ctypes.POINTER(_LL)
        d.ry_outgate_create.argtypes = [_VP, _CI, ctypes.c_double, ctypes.c_double, _CI, ctypes.POINTER(_VP)]
        d.ry_outgate_destroy.argtypes = [_VP]
        d.ry_outgate_destroy.restype = None
        d.ry_outgate_reset.argtypes = [_VP]
        d.ry_outgate_push.argtypes = [_VP, _DP, _CI, _CI, _VP, _CI, _IP, _IP, _DP]
        d.ry_outgate_held.argtypes = [_VP]
        d.ry_outgate_debug_counts.argtypes = [_VP, _LLP]
        d.ry_outgate_debug_poison.argtypes = [_VP]
        d.ry_outgate_bank_create.argtypes = [_VP, _CI, _CI, ctypes.c_double, ctypes.c_double, _CI, ctypes.POINTER(_VP)]
        d.ry_outgate_bank_destroy.argtypes = [_VP]
        d.ry_outgate_bank_destroy.restype = None
        d.ry_outgate_bank_reset.argtypes = [_VP, _CI]
        d.ry_outgate_bank_push.argtypes = [_VP, _DP, _LLP, _CI, _VP, _LL, _LLP, _IP, _DP]
        d.ry_outgate_bank_held.argtypes = [_VP, _CI]
        d.ry_outgate_bank_debug_counts.argtypes = [_VP, _LLP]
        d.ry_outgate_bank_debug_poison.argtypes = [_VP]
        d.ry_outgate_debug_upload_bytes.argtypes = [_VP]
        d.ry_outgate_debug_upload_bytes.restype = ctypes.c_longlong
        d.ry_outgate_bank_debug_upload_bytes.argtypes = [_VP]
        d.ry_outgate_bank_debug_upload_bytes.restype = ctypes.c_longlong
        d.ry_rowstore_create.argtypes = [_VP, _CI, _CI, _CI, _CI, ctypes.POINTER(_VP)]
        d.ry_rowstore_destroy.argtypes = [_VP]
        d.ry_rowstore_destroy.restype = None
        d.ry_rowstore_append.argtypes = [_VP, _FP, _FP, _CI, _CI, _FP, _CI, _CI, _IP, _IP]
        d.ry_rowstore_retire.argtypes = [_VP, _CI, _CI]
        d.ry_rowstore_held.argtypes = [_VP, _IP, _IP]
        d.ry_rowstore_fetch.argtypes = [_VP, _IP, _CI, _IP, _CI, _FP, _FP, _FP, _CI, _CI]
        d.ry_rowstore_reset.argtypes = [_VP]
        d.ry_rowstore_debug_buffers.argtypes = [_VP, ctypes.POINTER(_VP), ctypes.POINTER(_VP), ctypes.POINTER(_VP)]
        d.ry_rowstore_debug_counts.argtypes = [_VP, _LLP]
        d.ry_rowstore_debug_poison.argtypes = [_VP]
        d.ry_rowbank_create.argtypes = [_VP, _CI, _CI, _CI, _CI, _CI, ctypes.POINTER(_VP)]
        d.ry_rowbank_destroy.argtypes = [_VP]
        d.ry_rowbank_destroy.restype = None
        d.ry_rowbank_append.argtypes = [_VP, _CI, _IP, _FP, _FP, _IP, _IP, _FP, _LLP, _IP, _IP, _IP]
        d.ry_rowbank_fetch.argtypes = [_VP, _CI, _IP, _IP, _IP, _IP, _IP, _FP, _FP, _IP, _LLP]
        d.ry_rowbank_pick_ap.argtypes = [_VP, _CI, _IP, _IP, _IP, _IP, _IP, _UB, _FP, _CI]
        d.ry_rowbank_retire.argtypes = [_VP, _CI, _CI, _CI]
        d.ry_rowbank_reset.argtypes = [_VP, _CI]
        d.ry_rowbank_held.argtypes = [_VP, _CI, _IP, _IP]
        d.ry_rowbank_debug_buffers.argtypes = [_VP, ctypes.POINTER(_VP), ctypes.POINTER(_VP), ctypes.POINTER(_VP)]
        d.ry_rowbank_debug_counts.argtypes = [_VP, _LLP]
        d.ry_rowbank_debug_poison.argtypes = [_VP]
        d.ry_analysis_debug_d4c.argtypes = [_VP, ctypes.POINTER(_LL), _DP, _CI, _IP]
        d.ry_net_profile_window.argtypes = [_VP, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RyKernelStat), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        d.ry_net_debug_activation.argtypes = [_VP, ctypes.c_int, ctypes.c_int, _VP, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        d.ry_net_debug_plan.argtypes = [_VP] + [ctypes.c_int] * 5 + [ctypes.POINTER(RyPlanRecord), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        d.ry_set_filter_build.argtypes = [ctypes.c_int]
        d.ry_net_build_stats.argtypes = [_VP, ctypes.POINTER(RyBuildStats)]
        d.ry_net_debug_filters.argtypes = [_VP, ctypes.c_int, ctypes.c_int, _FP, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        d.ry_debug_layer_filters.argtypes = [_VP] + [ctypes.c_int] * 9 + [_FP, ctypes.c_int, _FP, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]

    def check(self, rc):
        if rc != 0:
            raise Ry355Error('libry355: %s (code %d)' % ((self.dll.ry_last_error() or b'').decode('utf-8', 'replace'), rc))

    def device_count(self):
        return int(self.dll.ry_device_count())


_default_lib = None


def default_lib():
    """The product library (never the emulator)."""
    global _default_lib
    if _default_lib is None:
        _default_lib = Ry355Lib()
    return _default_lib
