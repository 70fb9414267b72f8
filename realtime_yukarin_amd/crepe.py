"""CREPE pitch tracker on the MI355X: network spec, weights (seeded synthetic, or a `.npz` / torch state-dict file), the host-side
pieces (the resampler's tables and its host statement, the HMM tables, `predict_voicing`) and `CrepeModel`, the handle over `ry_crepe_*`
(include/ry355.h), which resamples to 16 kHz, runs the network and decodes on the device; `CrepeModel.voicing` is `predict_voicing` and the
wrapper's mask on the device, `CrepeModel.track` the whole chain in one call (`encode.extract` builds on it); `CrepeStream` is `track` window by
window over a live signal, with the activation rows of the frames two windows share kept on the card (`ry_crepe_stream_*`).

The reference turns CREPE on with `extract_f0_mode: crepe` (realtime-yukarin: realtime_voice_conversion/config.py:8-10); its
CrepeAcousticFeatureWrapper.extract_f0 calls `crepe.predict(x, fs, viterbi=True, model_capacity='full', step_size=frame_period)` and
`crepe.predict_voicing(confidence)` (yukarin_wrapper/acoustic_feature_wrapper.py:65-80).  The drop-in module with those names is
`realtime_yukarin_amd/compat/crepe`.  Everything here is restated from the public crepe package and its PyTorch fork ([MEM]): no
trained weights, crepe, resampy or hmmlearn exist to pin it against.
"""
import ctypes
import os
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy

from . import _lib
from ._handle import _DP, DeviceHandle, _dptr

_UBP = ctypes.POINTER(ctypes.c_ubyte)

# ---- the network ([MEM], one place) --------------------------------------------------------------------------------------------
CAPACITIES = {'tiny': 4, 'small': 8, 'medium': 16, 'large': 24, 'full': 32}
FILTERS = (32, 4, 4, 4, 8, 16)           # x multiplier
WIDTHS = (512, 64, 64, 64, 64, 64)
STRIDES = (4, 1, 1, 1, 1, 1)
PADS = ((254, 254), (31, 32), (31, 32), (31, 32), (31, 32), (31, 32))     # Keras 'same'
MODEL_SRATE = 16000
FRAME = 1024
BINS = 360
BN_EPS = 1e-3                            # Keras BatchNormalization default
STD_FLOOR = 1e-10                        # divisor clamp of a silent frame (torchcrepe's choice; the original gives NaN)
CENTS_OFFSET = 1997.3794084376191        # cents of bin b = 7180 / 359 * b + CENTS_OFFSET (linspace(0, 7180, 360))
# resampy's 'kaiser_best' filter ([MEM]): 64 zero crossings, 2^9 table entries per crossing, Kaiser beta, roll-off
KAISER_BEST = dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)
# predict_voicing: two-state Gaussian HMM over the confidence ([MEM]: start, transition, means, variances; state 1 = voiced)
VOICING_START = (0.7472, 0.2528)
VOICING_TRANS = ((0.9991, 0.0009), (0.0025, 0.9975))
VOICING_MEANS = (0.0795, 0.6278)
VOICING_VARS = (0.0181, 0.0454)
# arithmetic of the network's GEMMs (`ry_crepe_set_dtype`, numbered as `ry_net_set_dtype`): fp32 MFMA, or three bf16 products per fp32 product
DTYPES = {'f32': 0, 'bf16x3': 2}


def multiplier(capacity) -> int:
    """'tiny' .. 'full' -> 4 .. 32; an int is taken as the multiplier itself (1 .. 32; tests use reduced ones)."""
    if isinstance(capacity, str):
        if capacity not in CAPACITIES:
            raise ValueError('unknown CREPE capacity %r (one of %s)' % (capacity, ', '.join(CAPACITIES)))
        return CAPACITIES[capacity]
    m = int(capacity)
    if not 1 <= m <= 32:
        raise ValueError('CREPE capacity multiplier %d out of range 1 .. 32' % m)
    return m


def channels(m: int) -> List[int]:
    return [f * m for f in FILTERS]


def param_list(m: int) -> List[Tuple[str, Tuple[int, ...]]]:
    """Keys and shapes in blob order (`ry_crepe_create`), named after the PyTorch fork's state dict ([MEM])."""
    out, cin = [], 1
    for i, (c, w) in enumerate(zip(channels(m), WIDTHS), 1):
        out += [('conv%d.weight' % i, (c, cin, w)), ('conv%d.bias' % i, (c,))]
        out += [('conv%d_BN.%s' % (i, k), (c,)) for k in ('weight', 'bias', 'running_mean', 'running_var')]
        cin = c
    return out + [('classifier.weight', (BINS, 4 * cin)), ('classifier.bias', (BINS,))]


def param_count(m: int) -> int:
    return sum(int(numpy.prod(s)) for _, s in param_list(m))


def synthetic_params(capacity, seed: int = 0) -> Dict[str, numpy.ndarray]:
    """Seeded stand-in weights: He-scaled filters, small biases, BatchNorm statistics whose gamma is negative for every eighth channel
    (so BN cannot be folded into the filters and the pool must compare values after BN)."""
    m = multiplier(capacity)
    rng = numpy.random.default_rng(seed)
    P = {}
    for key, shape in param_list(m):
        if key.endswith('.weight') and len(shape) > 1:
            fan_in = int(numpy.prod(shape[1:]))
            a = rng.normal(0.0, numpy.sqrt((2.0 if key.startswith('conv') else 1.0) / fan_in), shape)
        elif key.endswith('_BN.weight'):
            a = rng.normal(0.8, 0.4, shape)
            a[::8] = -numpy.abs(a[::8])
        elif key.endswith('_BN.running_mean'):
            a = rng.uniform(0.0, 0.5, shape)
        elif key.endswith('_BN.running_var'):
            a = rng.uniform(0.5, 1.5, shape)
        else:                                                    # conv / BN / classifier biases
            a = rng.normal(0.0, 0.1, shape)
        P[key] = a.astype(numpy.float32)
    return P


def validate_params(m: int, P: Dict[str, numpy.ndarray]) -> Dict[str, numpy.ndarray]:
    """Exactly the keys of `param_list(m)` (a torch state dict may also carry `num_batches_tracked`), conv filters (Cout, Cin, W) or the
    fork's (Cout, Cin, W, 1).  Returns the float32 arrays in the canonical shapes; refuses anything else."""
    want = dict(param_list(m))
    have = {k: v for k, v in P.items() if not k.endswith('num_batches_tracked')}
    missing, extra = sorted(set(want) - set(have)), sorted(set(have) - set(want))
    if missing or extra:
        raise ValueError('CREPE weight keys do not match capacity %d: missing=%s unexpected=%s' % (m, missing, extra))
    out = {}
    for k, shape in want.items():
        a = numpy.asarray(have[k])
        if a.shape != shape and not (len(shape) == 3 and a.shape == shape + (1,)):
            raise ValueError('CREPE weight %s has shape %s, capacity %d needs %s' % (k, a.shape, m, shape))
        if not numpy.issubdtype(a.dtype, numpy.floating):
            raise ValueError('CREPE weight %s has dtype %s' % (k, a.dtype))
        out[k] = numpy.ascontiguousarray(a.reshape(shape), dtype=numpy.float32)
    return out


def capacity_of(P: Dict[str, numpy.ndarray]) -> int:
    """The multiplier a weight set was built for (conv1 has 32 m filters)."""
    if 'conv1.weight' not in P:
        raise ValueError('CREPE weights without conv1.weight')
    c = int(numpy.asarray(P['conv1.weight']).shape[0])
    if c % 32:
        raise ValueError('conv1.weight has %d filters, not a multiple of 32' % c)
    return c // 32


def load_weights(path, capacity=None) -> Tuple[int, Dict[str, numpy.ndarray]]:
    """A `.npz` (keys of `param_list`) or a torch state dict (`.pt` / `.pth`, tensors under the same keys) -> (multiplier, weights)."""
    path = Path(path)
    if path.suffix == '.npz':
        with numpy.load(str(path)) as z:
            P = {k: numpy.asarray(z[k]) for k in z.files}
    else:
        import torch
        sd = torch.load(str(path), map_location='cpu', weights_only=True)
        if not isinstance(sd, dict):
            raise ValueError('%s: expected a state dict, got %s' % (path, type(sd).__name__))
        P = {k: v.detach().cpu().numpy() if hasattr(v, 'detach') else numpy.asarray(v) for k, v in sd.items()}
    m = capacity_of(P) if capacity is None else multiplier(capacity)
    return m, validate_params(m, P)


def save_weights(path, P: Dict[str, numpy.ndarray]) -> None:
    numpy.savez(str(path), **P)


def flatten_params(m: int, P: Dict[str, numpy.ndarray]) -> numpy.ndarray:
    P = validate_params(m, P)
    return numpy.concatenate([P[k].ravel() for k, _ in param_list(m)])


# ---- framing, decode tables, resampling, voicing (host, float64) ---------------------------------------------------------------
def n_frames(n_samples: int, hop: int, center: bool = True) -> int:
    return 1 + (int(n_samples) + (FRAME if center else 0) - FRAME) // int(hop)


def track_frames(n_samples: int, sr, hop: int) -> int:
    """The frames `CrepeModel.track` returns for n_samples at sr -- centred frames of the signal at 16 kHz, `n_frames(resampled_length(n), hop)`,
    the rule `ry_crepe_track` applies on its side -- computed without a model: what a caller that skips the tracker for a wave needs to know of it."""
    n16 = int(n_samples) if int(sr) == MODEL_SRATE else resampled_length(n_samples, sr)
    return n_frames(n16, hop, True) if n16 >= 1 else 0


def hop_length(step_size) -> int:
    """`int(16000 * step_size / 1000)`: 80 samples for the reference's 5 ms."""
    return int(MODEL_SRATE * step_size / 1000)


def viterbi_tables():
    """(logT [360][360], logE [360][360], logS [360]) in float64 with numpy's log: uniform start, T[i][j] ~ max(12 - |i - j|, 0) per row,
    emission 0.1 I + 0.9 / 360.  Uploaded to the device so that its Viterbi path equals the numpy restatement's bit for bit."""
    xx, yy = numpy.meshgrid(range(BINS), range(BINS))
    T = numpy.maximum(12 - abs(xx - yy), 0)
    T = T / numpy.sum(T, axis=1)[:, None]
    E = numpy.eye(BINS) * 0.1 + numpy.ones((BINS, BINS)) * (0.9 / BINS)
    with numpy.errstate(divide='ignore'):
        return numpy.log(T), numpy.log(E), numpy.log(numpy.ones(BINS) / BINS)


def cents_mapping() -> numpy.ndarray:
    return numpy.linspace(0, 7180, BINS) + CENTS_OFFSET


def _kaiser_best_window():
    k = KAISER_BEST
    n = (2 ** k['precision']) * k['num_zeros']
    sinc = k['rolloff'] * numpy.sinc(k['rolloff'] * numpy.linspace(0, k['num_zeros'], num=n + 1, endpoint=True))
    return numpy.kaiser(2 * n + 1, k['beta'])[n:] * sinc, 2 ** k['precision']


def resample(x, sr_orig: int, sr_new: int = MODEL_SRATE) -> numpy.ndarray:
    """Band-limited windowed-sinc interpolation with resampy's 'kaiser_best' parameters ([MEM]; the interpolation loop of
    resampy.resample_f, every output a sum over the taps on both sides of its time), in float64; returns float32.  Output length
    int(len * sr_new / sr_orig)."""
    x = numpy.asarray(x, dtype=numpy.float64)
    if sr_orig == sr_new:
        return x.astype(numpy.float32)
    ratio = float(sr_new) / sr_orig
    win, num_table = _kaiser_best_window()
    if ratio < 1:
        win = win * ratio
    delta = numpy.zeros_like(win)
    delta[:-1] = numpy.diff(win)
    n_out = int(x.shape[0] * ratio)
    y = numpy.zeros(n_out)
    if n_out == 0:
        return y.astype(numpy.float32)
    scale = min(1.0, ratio)
    step = int(scale * num_table)
    tr = numpy.concatenate([[0.0], numpy.cumsum(numpy.full(n_out - 1, 1.0 / ratio))])     # time_register += increment, in order
    n = tr.astype(numpy.int64)
    nwin = win.shape[0]
    for side in (0, 1):
        frac = scale * (tr - n)
        if side:
            frac = scale - frac
        index_frac = frac * num_table
        offset = index_frac.astype(numpy.int64)
        eta = index_frac - offset
        lim = (nwin - offset) // step
        cap = numpy.minimum(n + 1, lim) if side == 0 else numpy.minimum(x.shape[0] - n - 1, lim)
        for i in range(int(cap.max()) if cap.size else 0):
            live = i < cap
            idx = offset[live] + i * step
            src = n[live] - i if side == 0 else n[live] + i + 1
            y[live] += (win[idx] + eta[live] * delta[idx]) * x[src]
    return y.astype(numpy.float32)


def _rate(sr) -> int:
    if int(sr) != sr or int(sr) < 1:
        raise ValueError('the device resampler takes a whole, positive sample rate in Hz, got %r' % (sr,))
    return int(sr)


def resampled_length(n_samples: int, sr) -> int:
    """Samples at 16 kHz of n_samples at sr, in the form `resample` computes it."""
    return int(int(n_samples) * (float(MODEL_SRATE) / sr))


def resampler_tables(sr):
    """(win, num_table, step) of `resample(x, sr)`: the half filter (scaled by the ratio when down-sampling), its entries per zero
    crossing and per input sample.  `ry_crepe_set_resampler` takes them as they are."""
    ratio = float(MODEL_SRATE) / sr
    win, num_table = _kaiser_best_window()
    if ratio < 1:
        win = win * ratio
    return numpy.ascontiguousarray(win, dtype=numpy.float64), num_table, int(min(1.0, ratio) * num_table)


def time_register(sr, n_out: int) -> numpy.ndarray:
    """The input time of outputs 0 .. n_out - 1 of `resample(x, sr)`: resampy's `time_register += 1 / ratio`, summed one by one in
    float64 (the expression `resample` uses; a shorter register is a prefix of a longer one)."""
    ratio = float(MODEL_SRATE) / sr
    return numpy.concatenate([[0.0], numpy.cumsum(numpy.full(int(n_out) - 1, 1.0 / ratio))])


def predict_voicing(confidence) -> numpy.ndarray:
    """Voiced (1) / unvoiced (0) per frame: Viterbi path of a two-state Gaussian HMM over the confidence, float64, lowest state on ties
    (the fork's `predict_voicing` with fixed constants, [MEM])."""
    x = numpy.asarray(confidence, dtype=numpy.float64).ravel()
    if x.size == 0:
        return numpy.zeros(0, numpy.int64)
    mu, var = numpy.asarray(VOICING_MEANS), numpy.asarray(VOICING_VARS)
    logp = -0.5 * (numpy.log(2 * numpy.pi * var)[None, :] + (x[:, None] - mu[None, :]) ** 2 / var[None, :])
    logT = numpy.log(numpy.asarray(VOICING_TRANS))
    lat = numpy.log(numpy.asarray(VOICING_START)) + logp[0]
    bp = numpy.zeros((x.size, 2), numpy.int64)
    for t in range(1, x.size):
        s = lat[:, None] + logT
        bp[t] = numpy.argmax(s, axis=0)
        lat = s[bp[t], [0, 1]] + logp[t]
    path = numpy.zeros(x.size, numpy.int64)
    path[-1] = int(numpy.argmax(lat))
    for t in range(x.size - 1, 0, -1):
        path[t - 1] = bp[t, path[t]]
    return path


def voicing_tables():
    """(c [2], mu [2], var [2], logT [2][2], logS [2]) of `predict_voicing` in float64, the logs by the expressions it uses: what
    `ry_crepe_set_voicing_tables` takes, so that the device's mask equals the host's bit for bit."""
    mu, var = numpy.asarray(VOICING_MEANS), numpy.asarray(VOICING_VARS)
    return numpy.log(2 * numpy.pi * var), mu, var, numpy.log(numpy.asarray(VOICING_TRANS)), numpy.log(numpy.asarray(VOICING_START))


class DeviceTrack(object):
    """What `CrepeModel.track(..., device=True)` left on the card: addresses of the uploaded float32 wave (`samples` of it) and of `voiced`
    (bytes), `f0` and `t` (float64) of `frames` frames.  They belong to the model's handle and hold until its next call; `ctx` is the
    context whose stream orders the work that reads them (`Analyzer.run_device`)."""

    def __init__(self, model, ctx, wave, samples, frames, voiced, f0, t):
        self.model, self.ctx = model, ctx
        self.wave, self.samples, self.frames, self.voiced, self.f0, self.t = wave, samples, frames, voiced, f0, t

    def download(self) -> numpy.ndarray:
        """voiced [frames] bool, f0 [frames] float64 (waits for the stream)."""
        return self.model._download_track(self)


class DeviceTracks(object):
    """What `CrepeModel.track_many(..., device=True)` left on the card: the addresses of the uploaded float32 waves (back to back) and of the
    concatenated `voiced` (bytes), `f0` and `t` (float64); `sample_offsets` / `frame_offsets` (int64 / int32, waves + 1 entries): where wave i
    starts in them.  They belong to the model's handle and hold until its next call (`Analyzer.run_device_many` reads them)."""

    def __init__(self, model, ctx, wave, voiced, f0, t, sample_offsets, frame_offsets):
        self.model, self.ctx = model, ctx
        self.wave, self.voiced, self.f0, self.t = wave, voiced, f0, t
        self.sample_offsets, self.frame_offsets = sample_offsets, frame_offsets
        self.waves, self.samples, self.frames = sample_offsets.size - 1, int(sample_offsets[-1]), int(frame_offsets[-1])

    def download(self):
        """[(voiced [frames] bool, f0 [frames] float64)] per wave (waits for the stream)."""
        voiced, f0 = self.model._download_track(self)
        o = self.frame_offsets
        return [(voiced[o[i]:o[i + 1]], f0[o[i]:o[i + 1]]) for i in range(self.waves)]


class UploadedWaves(object):
    """What `CrepeModel.upload_waves` left on the card: the address of the float32 waves (back to back, at `sr`) and `offsets` (int64, waves + 1
    entries): where wave i starts.  Holds until the next call on the model that is not `track_uploaded` (of the model or of a bank over it)."""

    def __init__(self, model, ctx, wave, sr, offsets):
        self.model, self.ctx, self.wave, self.sr, self.offsets = model, ctx, wave, sr, offsets
        self.waves, self.samples = offsets.size - 1, int(offsets[-1])


class UploadedTracks(object):
    """What `track_uploaded` left on the card for the waves `which` of an `UploadedWaves`: the addresses of the concatenated `voiced` (bytes), `f0` and
    `t` (float64) of the tracked waves, `frame_offsets` (int32, tracked + 1 entries) into them, `first_sample` / `n_samples` of every tracked wave in
    the uploaded block `wave` of `samples` samples."""

    def __init__(self, model, ctx, uploaded, which, voiced, f0, t, frame_offsets):
        self.model, self.ctx, self.which = model, ctx, list(which)
        self.wave, self.samples = uploaded.wave, uploaded.samples
        self.first_sample = numpy.asarray([uploaded.offsets[i] for i in which], numpy.int64)
        self.n_samples = numpy.asarray([uploaded.offsets[i + 1] - uploaded.offsets[i] for i in which], numpy.int32)
        self.voiced, self.f0, self.t, self.frame_offsets = voiced, f0, t, frame_offsets
        self.waves, self.frames = len(self.which), int(frame_offsets[-1])

    def download(self):
        """[(voiced [frames] bool, f0 [frames] float64)] per tracked wave (waits for the stream)."""
        voiced, f0 = self.model._download_track(self)
        o = self.frame_offsets
        return [(voiced[o[i]:o[i + 1]], f0[o[i]:o[i + 1]]) for i in range(self.waves)]


# ---- the device model ---------------------------------------------------------------------------------------------------------
class CrepeModel(DeviceHandle):
    """CREPE on the MI355X (`ry_crepe_*`).  Picklable and fork-safe: the GPU context and the device weights are created lazily in the
    process that first predicts; the host copy of the weights travels with the object.  `ctx` (tests) is a context over another build
    of the library -- the emulator -- used instead of the product's context of `device`.  `dtype`: 'f32' (default) or 'bf16x3', the
    split-bf16 form of the GEMMs (`set_dtype`); it travels with the object and is applied to every handle the object creates."""

    def __init__(self, capacity='full', params: Optional[Dict[str, numpy.ndarray]] = None, device: Optional[int] = None,
                 bn_eps: float = BN_EPS, ctx=None, seed: Optional[int] = None, dtype: str = 'f32'):
        self.m = multiplier(capacity)
        self.dtype = self._dtype_name(dtype)
        if params is None:
            if seed is None:
                raise ValueError('CrepeModel needs weights: pass params (load_weights / synthetic_params) or a seed for synthetic ones')
            params = synthetic_params(self.m, seed)
        self.blob = flatten_params(self.m, params)
        self.bn_eps = float(bn_eps)
        self._rs = {}                      # input rate -> entries of the time register the handle holds
        DeviceHandle.__init__(self, ctx, device)

    _destroy = 'ry_crepe_destroy'

    def __getstate__(self):
        d = DeviceHandle.__getstate__(self)
        d['_rs'] = {}
        return d

    def _create(self, lib, ctx):
        h = ctypes.c_void_p()
        lib.check(lib.dll.ry_crepe_create(ctx.handle, self.m, _lib._fptr(self.blob), self.blob.size, self.bn_eps, ctypes.byref(h)))
        self._rs = {}
        tabs = [numpy.ascontiguousarray(t, dtype=numpy.float64) for t in viterbi_tables()]
        lib.check(lib.dll.ry_crepe_set_viterbi_tables(h, *[_dptr(t) for t in tabs]))
        tabs = [numpy.ascontiguousarray(t, dtype=numpy.float64) for t in voicing_tables()]
        lib.check(lib.dll.ry_crepe_set_voicing_tables(h, *[_dptr(t) for t in tabs]))
        if self.dtype != 'f32':
            lib.check(lib.dll.ry_crepe_set_dtype(h, DTYPES[self.dtype]))
        return h

    @staticmethod
    def _dtype_name(dtype) -> str:
        if dtype not in DTYPES:
            raise ValueError('unknown CREPE dtype %r (one of %s)' % (dtype, ', '.join(DTYPES)))
        return dtype

    def set_dtype(self, dtype: str) -> None:
        """'f32' or 'bf16x3' for the calls that follow (`ry_crepe_set_dtype`).  A handle that exists is switched now; one created later
        (first use, after unpickling, in a forked child) is created in the mode."""
        dtype = self._dtype_name(dtype)
        if self._handle is not None and self._pid == os.getpid():
            lib, h = self._get()
            lib.check(lib.dll.ry_crepe_set_dtype(h, DTYPES[dtype]))
        self.dtype = dtype

    def predict16k(self, audio, hop: int, center: bool = True, viterbi: bool = True, activation: bool = True):
        """audio: float32 samples at 16 kHz -> (f0 float32 Hz, confidence float32, activation [frames][360] float32 or None)."""
        lib, h = self._get()
        x = numpy.ascontiguousarray(audio, dtype=numpy.float32).ravel()
        n = n_frames(x.size, hop, center)
        if x.size < 1 or n < 1:
            raise ValueError('CREPE needs at least %d samples (center=False) or one sample, got %d' % (FRAME if not center else 1, x.size))
        f0 = numpy.empty(n, numpy.float32)
        conf = numpy.empty(n, numpy.float32)
        act = numpy.empty((n, BINS), numpy.float32) if activation else None
        lib.check(lib.dll.ry_crepe_predict(h, _lib._fptr(x), x.size, int(hop), int(bool(center)), int(bool(viterbi)),
                                           _lib._fptr(f0), _lib._fptr(conf), _lib._fptr(act), 0))
        return f0, conf, act

    def _resampler(self, sr: int, n_out: int) -> None:
        """The tables of rate sr on the handle, with a time register of at least n_out entries: built on first use, the register
        grown geometrically (its values depend on the rate and the index only)."""
        lib, h = self._get()
        have = self._rs.get(sr, 0)
        if n_out <= have:
            return
        n = max(n_out, 2 * have)
        tr = numpy.ascontiguousarray(time_register(sr, n), dtype=numpy.float64)
        if have:
            lib.check(lib.dll.ry_crepe_set_resampler(h, sr, None, 0, 0, 0, _dptr(tr), n))
        else:
            win, num_table, step = resampler_tables(sr)
            lib.check(lib.dll.ry_crepe_set_resampler(h, sr, _dptr(win), win.size, num_table, step, _dptr(tr), n))
        self._rs[sr] = n

    def resample(self, audio, sr) -> numpy.ndarray:
        """audio: float32 samples at sr -> float32 samples at 16 kHz, the bits of `resample(audio, sr)` (`ry_crepe_resample`)."""
        lib, h = self._get()
        sr = _rate(sr)
        x = numpy.ascontiguousarray(audio, dtype=numpy.float32).ravel()
        if sr == MODEL_SRATE:
            return x.copy()
        n_out = resampled_length(x.size, sr)
        if n_out < 1:
            raise ValueError('%d samples at %d Hz give no sample at 16 kHz' % (x.size, sr))
        self._resampler(sr, n_out)
        y = numpy.empty(n_out, numpy.float32)
        lib.check(lib.dll.ry_crepe_resample(h, _lib._fptr(x), x.size, sr, _lib._fptr(y), 0))
        return y

    def predict(self, audio, sr, hop: int, center: bool = True, viterbi: bool = True, activation: bool = True):
        """audio: float32 samples at sr, resampled to 16 kHz on the device -> what `predict16k` returns for the resampled signal
        (`ry_crepe_predict_sr`); hop is in samples at 16 kHz."""
        sr = _rate(sr)
        if sr == MODEL_SRATE:
            return self.predict16k(audio, hop, center, viterbi, activation)
        lib, h = self._get()
        x = numpy.ascontiguousarray(audio, dtype=numpy.float32).ravel()
        n_out = resampled_length(x.size, sr)
        n = n_frames(n_out, hop, center) if n_out >= 1 else 0
        if n < 1:
            raise ValueError('CREPE needs at least %d samples at 16 kHz (center=False) or one sample, %d samples at %d Hz give %d'
                             % (FRAME if not center else 1, x.size, sr, n_out))
        self._resampler(sr, n_out)
        f0 = numpy.empty(n, numpy.float32)
        conf = numpy.empty(n, numpy.float32)
        act = numpy.empty((n, BINS), numpy.float32) if activation else None
        lib.check(lib.dll.ry_crepe_predict_sr(h, _lib._fptr(x), x.size, sr, int(hop), int(bool(center)), int(bool(viterbi)),
                                              _lib._fptr(f0), _lib._fptr(conf), _lib._fptr(act), 0))
        return f0, conf, act

    def decode(self, activation, viterbi: bool = True):
        """The decode alone on a host activation (frames, 360) -> (f0, confidence, centre bin per frame) (`ry_crepe_decode`)."""
        lib, h = self._get()
        a = numpy.ascontiguousarray(activation, dtype=numpy.float32)
        if a.ndim != 2 or a.shape[1] != BINS or a.shape[0] < 1:
            raise ValueError('activation must be (frames, %d), got %s' % (BINS, a.shape))
        n = a.shape[0]
        f0, conf, path = numpy.empty(n, numpy.float32), numpy.empty(n, numpy.float32), numpy.empty(n, numpy.int32)
        lib.check(lib.dll.ry_crepe_decode(h, _lib._fptr(a), n, int(bool(viterbi)), _lib._fptr(f0), _lib._fptr(conf),
                                          path.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return f0, conf, path

    def voicing(self, confidence, f0, threshold: float = 0.1, step_size=10, device: bool = False):
        """`(predict_voicing(confidence) == 1) | (confidence > threshold)`, the f0 it masks and the time axis, on the device
        (`ry_crepe_voicing`): confidence, f0 float32 [n] -> (voiced bool [n], f0 float64 [n], 0 where unvoiced, t float64 [n] =
        arange(n) * step_size / 1000).  The threshold is compared in float32, as numpy compares a float32 array with a Python float.  device=True (tests): the five arrays pass through device buffers of the caller."""
        lib, h = self._get()
        c = numpy.ascontiguousarray(confidence, dtype=numpy.float32).ravel()
        f = numpy.ascontiguousarray(f0, dtype=numpy.float32).ravel()
        if c.size != f.size or c.size < 1:
            raise ValueError('voicing needs confidence and f0 of one length >= 1, got %d and %d' % (c.size, f.size))
        n = c.size
        voiced, f64, t64 = numpy.empty(n, numpy.uint8), numpy.empty(n, numpy.float64), numpy.empty(n, numpy.float64)
        args = (n, float(threshold), float(step_size))
        if not device:
            lib.check(lib.dll.ry_crepe_voicing(h, _lib._fptr(c), _lib._fptr(f), *args, voiced.ctypes.data_as(_UBP), _dptr(f64), _dptr(t64), 0))
            return voiced.astype(bool), f64, t64
        from .world_synth import _DeviceBuffer
        ctx, dll = self._ctx, lib.dll
        host = [c, f, numpy.zeros((n + 3) // 4, numpy.float32), f64.view(numpy.float32), t64.view(numpy.float32)]
        bufs = [_DeviceBuffer(ctx, a.size) for a in host]
        for a, b in zip(host[:2], bufs[:2]):
            lib.check(dll.ry_dev_upload(ctx.handle, b.ptr, _lib._fptr(a), a.size))
        as_ub, as_d = (lambda b: ctypes.cast(b.ptr, _UBP)), (lambda b: ctypes.cast(b.ptr, _DP))
        lib.check(dll.ry_crepe_voicing(h, bufs[0].ptr, bufs[1].ptr, *args, as_ub(bufs[2]), as_d(bufs[3]), as_d(bufs[4]), 1))
        for a, b in zip(host[2:], bufs[2:]):
            lib.check(dll.ry_dev_download(ctx.handle, _lib._fptr(a), b.ptr, a.size))
        return host[2].view(numpy.uint8)[:n].astype(bool), f64, t64

    def _frames_at(self, n_samples: int, sr: int, hop: int) -> int:
        n16 = n_samples if sr == MODEL_SRATE else resampled_length(n_samples, sr)
        n = n_frames(n16, hop, True) if n16 >= 1 else 0
        if n < 1:
            raise ValueError('CREPE needs at least one sample at 16 kHz, %d samples at %d Hz give %d' % (n_samples, sr, n16))
        if sr != MODEL_SRATE:
            self._resampler(sr, n16)
        return n

    def track(self, audio, sr, hop: int, step_size, threshold: float = 0.1, device: bool = False):
        """`predict(audio, sr, hop)` (centred, Viterbi, no activation) and `voicing` of its result in one enqueue, one upload of the wave
        (`ry_crepe_track`) -> (voiced bool, f0 float64, 0 where unvoiced, t float64).  device=True: nothing is copied back and nothing is
        waited for -> `DeviceTrack`, the addresses of the track and of the uploaded wave on the card."""
        sr = _rate(sr)
        x = numpy.ascontiguousarray(audio, dtype=numpy.float32).ravel()
        lib, h = self._get()
        n = self._frames_at(x.size, sr, hop)
        nf = ctypes.c_int()
        head = (h, _lib._fptr(x), x.size, sr, int(hop), float(step_size), float(threshold), ctypes.byref(nf))
        if not device:
            voiced, f64, t64 = numpy.empty(n, numpy.uint8), numpy.empty(n, numpy.float64), numpy.empty(n, numpy.float64)
            lib.check(lib.dll.ry_crepe_track(*head, voiced.ctypes.data_as(_UBP), _dptr(f64), _dptr(t64), 0))
            assert nf.value == n, (nf.value, n)
            return voiced.astype(bool), f64, t64
        lib.check(lib.dll.ry_crepe_track(*head, None, None, None, 1))
        p = [ctypes.c_void_p() for _ in range(4)]
        ns, nfr = ctypes.c_int(), ctypes.c_int()
        lib.check(lib.dll.ry_crepe_track_buffers(h, ctypes.byref(p[0]), ctypes.byref(ns), ctypes.byref(nfr), *[ctypes.byref(q) for q in p[1:]]))
        return DeviceTrack(self, self._ctx, p[0].value, ns.value, nfr.value, p[1].value, p[2].value, p[3].value)

    def track_many(self, waves, sr, hop: int, step_size, threshold: float = 0.1, device: bool = True):
        """`track` for a list of waves at one rate in one enqueue (`ry_crepe_track_many`): one upload of the waves back to back, the resampler
        over all of them, their frames packed into the passes of the network, the decode and the voicing one workgroup per wave.  Wave i gets
        the bits of `track(waves[i], ...)`, whatever else is in the list.  device=True -> `DeviceTracks`; False -> [(voiced, f0, t)] per wave."""
        sr = _rate(sr)
        xs = [numpy.ascontiguousarray(w, dtype=numpy.float32).ravel() for w in waves]
        if not xs:
            raise ValueError('track_many needs at least one wave')
        lib, h = self._get()
        counts = numpy.asarray([x.size for x in xs], numpy.int32)
        want = [self._frames_at(x.size, sr, hop) for x in xs]
        audio = numpy.ascontiguousarray(numpy.concatenate(xs))
        nf = numpy.zeros(len(xs), numpy.int32)
        _IP = ctypes.POINTER(ctypes.c_int)
        head = (h, _lib._fptr(audio), counts.ctypes.data_as(_IP), len(xs), sr, int(hop), float(step_size), float(threshold), nf.ctypes.data_as(_IP))
        if not device:
            n = int(sum(want))
            voiced, f64, t64 = numpy.empty(n, numpy.uint8), numpy.empty(n, numpy.float64), numpy.empty(n, numpy.float64)
            lib.check(lib.dll.ry_crepe_track_many(*head, voiced.ctypes.data_as(_UBP), _dptr(f64), _dptr(t64), 0))
            assert list(nf) == want, (list(nf), want)
            o = numpy.concatenate([[0], numpy.cumsum(nf)])
            return [(voiced[a:b].astype(bool), f64[a:b].copy(), t64[a:b].copy()) for a, b in zip(o[:-1], o[1:])]
        lib.check(lib.dll.ry_crepe_track_many(*head, None, None, None, 1))
        return self._tracks_on_card()

    def _tracks_on_card(self) -> DeviceTracks:
        lib, h = self._get()
        p = [ctypes.c_void_p() for _ in range(4)]
        nw = ctypes.c_int()
        so, fo = ctypes.POINTER(ctypes.c_longlong)(), ctypes.POINTER(ctypes.c_int)()
        lib.check(lib.dll.ry_crepe_track_many_buffers(h, ctypes.byref(p[0]), ctypes.byref(nw), ctypes.byref(so), ctypes.byref(fo),
                                                      *[ctypes.byref(q) for q in p[1:]]))
        sample_offsets = numpy.asarray(so[:nw.value + 1], numpy.int64)          # copies: the handle's arrays change with its next call
        frame_offsets = numpy.asarray(fo[:nw.value + 1], numpy.int32)
        return DeviceTracks(self, self._ctx, p[0].value, p[1].value, p[2].value, p[3].value, sample_offsets, frame_offsets)

    def upload_waves(self, waves, sr) -> UploadedWaves:
        """The one upload of `track_many`, alone (`ry_crepe_upload_waves`): the waves back to back on the card, for a caller that decides before the
        tracker runs which of them are worth tracking (`pipeline`'s gate-first form)."""
        sr = _rate(sr)
        xs = [numpy.ascontiguousarray(w, dtype=numpy.float32).ravel() for w in waves]
        if not xs:
            raise ValueError('upload_waves needs at least one wave')
        lib, h = self._get()
        for x in xs:
            self._frames_at(x.size, sr, MODEL_SRATE)                 # installs the rate's tables; refuses a wave without a sample at 16 kHz
        counts = numpy.asarray([x.size for x in xs], numpy.int32)
        audio = numpy.ascontiguousarray(numpy.concatenate(xs))
        p = ctypes.c_void_p()
        lib.check(lib.dll.ry_crepe_upload_waves(h, _lib._fptr(audio), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(xs), sr, ctypes.byref(p)))
        return UploadedWaves(self, self._ctx, p.value, sr, numpy.concatenate([[0], numpy.cumsum(counts, dtype=numpy.int64)]).astype(numpy.int64))

    def _uploaded_tracks(self, uploaded, which) -> UploadedTracks:
        lib, h = self._get()
        p = [ctypes.c_void_p() for _ in range(4)]
        ns, nt = ctypes.c_longlong(), ctypes.c_int()
        fo = ctypes.POINTER(ctypes.c_int)()
        lib.check(lib.dll.ry_crepe_uploaded_buffers(h, ctypes.byref(p[0]), ctypes.byref(ns), ctypes.byref(nt), ctypes.byref(fo),
                                                    *[ctypes.byref(q) for q in p[1:]]))
        assert nt.value == len(which) and p[0].value == uploaded.wave, (nt.value, len(which))
        frame_offsets = numpy.asarray(fo[:nt.value + 1], numpy.int32)           # a copy: the handle's array changes with its next call
        return UploadedTracks(self, self._ctx, uploaded, which, p[1].value, p[2].value, p[3].value, frame_offsets)

    def _which(self, uploaded, which):
        which = [int(i) for i in which]
        if uploaded.model is not self or not which or any(i < 0 or i >= uploaded.waves for i in which) or any(b <= a for a, b in zip(which, which[1:])):
            raise ValueError('the waves to track must be ascending indices into an upload of this model, got %s of %d' % (which, uploaded.waves))
        as_i = lambda v: numpy.ascontiguousarray(v, dtype=numpy.int32)
        return which, as_i([uploaded.offsets[i] for i in which]), as_i([uploaded.offsets[i + 1] - uploaded.offsets[i] for i in which])

    def track_uploaded(self, uploaded: UploadedWaves, which, hop: int, step_size, threshold: float = 0.1) -> UploadedTracks:
        """`track_many(..., device=True)` on the waves `which` (ascending indices) of `uploaded`, read where they lie (`ry_crepe_track_uploaded`):
        nothing is uploaded but the segment table; every tracked wave gets the bits of `track` on it alone."""
        lib, h = self._get()
        which, first, counts = self._which(uploaded, which)
        want = [self._frames_at(int(n), uploaded.sr, hop) for n in counts]
        nf = numpy.zeros(len(which), numpy.int32)
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        lib.check(lib.dll.ry_crepe_track_uploaded(h, ip(first), ip(counts), len(which), uploaded.sr, int(hop), float(step_size), float(threshold), ip(nf),
                                                  None, None, None, 1))
        assert list(nf) == want, (list(nf), want)
        return self._uploaded_tracks(uploaded, which)

    def frames_through_network(self) -> int:
        """Tests: the frames that have gone through the network on this model's handle so far (`ry_crepe_debug_frames`)."""
        lib, h = self._get()
        n = ctypes.c_longlong()
        lib.check(lib.dll.ry_crepe_debug_frames(h, ctypes.byref(n)))
        return n.value

    def decode_many(self, activations, viterbi: bool = True):
        """`decode` of several activations side by side, one workgroup each (`ry_crepe_decode_many`) -> [(f0, confidence, centre bins)]."""
        lib, h = self._get()
        acts = [numpy.ascontiguousarray(a, dtype=numpy.float32) for a in activations]
        if not acts or any(a.ndim != 2 or a.shape[1] != BINS or a.shape[0] < 1 for a in acts):
            raise ValueError('decode_many needs activations of (frames >= 1, %d)' % BINS)
        counts = numpy.asarray([a.shape[0] for a in acts], numpy.int32)
        a = numpy.ascontiguousarray(numpy.concatenate(acts))
        n = a.shape[0]
        f0, conf, path = numpy.empty(n, numpy.float32), numpy.empty(n, numpy.float32), numpy.empty(n, numpy.int32)
        _IP = ctypes.POINTER(ctypes.c_int)
        lib.check(lib.dll.ry_crepe_decode_many(h, _lib._fptr(a), counts.ctypes.data_as(_IP), len(acts), int(bool(viterbi)), _lib._fptr(f0), _lib._fptr(conf),
                                               path.ctypes.data_as(_IP)))
        o = numpy.concatenate([[0], numpy.cumsum(counts)])
        return [(f0[i:j], conf[i:j], path[i:j]) for i, j in zip(o[:-1], o[1:])]

    def voicing_many(self, confidences, f0s, threshold: float = 0.1, step_size=10, device: bool = False):
        """`voicing` of several tracks side by side, one workgroup each (`ry_crepe_voicing_many`) -> [(voiced, f0 float64, t)] per track.
        device=True (tests): the five arrays pass through device buffers of the caller."""
        lib, h = self._get()
        cs = [numpy.ascontiguousarray(c, dtype=numpy.float32).ravel() for c in confidences]
        fs = [numpy.ascontiguousarray(f, dtype=numpy.float32).ravel() for f in f0s]
        if not cs or len(cs) != len(fs) or any(c.size != f.size or c.size < 1 for c, f in zip(cs, fs)):
            raise ValueError('voicing_many needs as many confidence as f0 arrays, pairwise of one length >= 1')
        counts = numpy.asarray([c.size for c in cs], numpy.int32)
        c, f = numpy.concatenate(cs), numpy.concatenate(fs)
        n = c.size
        voiced, f64, t64 = numpy.empty(n, numpy.uint8), numpy.empty(n, numpy.float64), numpy.empty(n, numpy.float64)
        args = (counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(cs), float(threshold), float(step_size))
        o = numpy.concatenate([[0], numpy.cumsum(counts)])
        split = lambda v: [(v[i:j].astype(bool), f64[i:j], t64[i:j]) for i, j in zip(o[:-1], o[1:])]
        if not device:
            lib.check(lib.dll.ry_crepe_voicing_many(h, _lib._fptr(c), _lib._fptr(f), *args, voiced.ctypes.data_as(_UBP), _dptr(f64), _dptr(t64), 0))
            return split(voiced)
        from .world_synth import _DeviceBuffer
        ctx, dll = self._ctx, lib.dll
        host = [c, f, numpy.zeros((n + 3) // 4, numpy.float32), f64.view(numpy.float32), t64.view(numpy.float32)]
        bufs = [_DeviceBuffer(ctx, a.size) for a in host]
        for a, b in zip(host[:2], bufs[:2]):
            lib.check(dll.ry_dev_upload(ctx.handle, b.ptr, _lib._fptr(a), a.size))
        as_ub, as_d = (lambda b: ctypes.cast(b.ptr, _UBP)), (lambda b: ctypes.cast(b.ptr, _DP))
        lib.check(dll.ry_crepe_voicing_many(h, bufs[0].ptr, bufs[1].ptr, *args, as_ub(bufs[2]), as_d(bufs[3]), as_d(bufs[4]), 1))
        for a, b in zip(host[2:], bufs[2:]):
            lib.check(dll.ry_dev_download(ctx.handle, _lib._fptr(a), b.ptr, a.size))
        return split(host[2].view(numpy.uint8)[:n])

    def _download_track(self, trk):
        lib, h = self._get()
        n = trk.frames
        words, f64 = numpy.empty((n + 3) // 4, numpy.float32), numpy.empty(n, numpy.float64)
        lib.check(lib.dll.ry_dev_download(trk.ctx.handle, _lib._fptr(words), _lib._fptr(trk.voiced), (n + 3) // 4))
        lib.check(lib.dll.ry_dev_download(trk.ctx.handle, _lib._fptr(f64.view(numpy.float32)), _lib._fptr(trk.f0), 2 * n))
        return words.view(numpy.uint8)[:n].astype(bool), f64

    def debug_layer(self, layer: int, frames: int) -> numpy.ndarray:
        """The first `frames` rows of the last pass's buffer `layer` (0 frames, 1 .. 6 pooled conv outputs, 7 logits); rows behind the
        frames of that pass are what an earlier call or `poison` left (`ry_crepe_debug_layer`)."""
        lib, h = self._get()
        c = channels(self.m)
        shape = {0: (frames, FRAME), 7: (frames, BINS)}.get(layer) or (frames, (FRAME // 4) >> layer, c[layer - 1])
        out = numpy.empty(shape, numpy.float32)
        lib.check(lib.dll.ry_crepe_debug_layer(h, int(layer), int(frames), _lib._fptr(out)))
        return out

    def poison(self) -> None:
        """Tests: NaN bit patterns in everything the next `resample` / `predict` / `predict16k` / `decode` / `voicing` / `track` must
        write (`ry_crepe_debug_poison`)."""
        lib, h = self._get()
        lib.check(lib.dll.ry_crepe_debug_poison(h))

    def splits(self) -> List[int]:
        lib, h = self._get()
        s = (ctypes.c_int * 7)()
        lib.check(lib.dll.ry_crepe_debug_splits(h, s))
        return list(s)


class CrepeStream(DeviceHandle):
    """`CrepeModel.track` window by window over a live signal (`ry_crepe_stream_*`): the activation rows of the frames a window shares with the
    previous one are taken from that call instead of being run through the network again (DESIGN.md section 18 states which).  Call by call the
    result has the bits of `model.track` on the same window.  `advance`: sample i of this window is sample i + advance of the previous window of
    this stream; the object keeps the previous window and compares the overlap as 32-bit words before it says so to the device -- a window whose
    overlap differs (zero padding that has become audio, say) is computed in full.  advance=None: computed in full, and kept for the next call.
    `computed` / `frames`: the frames of the last call that went through the network / that it has.  A model serves any number of streams."""
    _destroy = 'ry_crepe_stream_destroy'

    def __init__(self, model: CrepeModel):
        self.model = model
        self.computed = self.frames = 0
        self._prev = None
        self._model_handle = None
        DeviceHandle.__init__(self, model._given_ctx, model.device)

    def __getstate__(self):
        d = DeviceHandle.__getstate__(self)
        d.update(_prev=None, _model_handle=None)
        return d

    def _get(self):
        """-> (library, stream handle) of this process, over the model's handle as it is now."""
        lib, mh = self.model._get()
        if self._handle is None or self._pid != os.getpid() or self._model_handle is not mh:
            h = ctypes.c_void_p()
            lib.check(lib.dll.ry_crepe_stream_create(mh, ctypes.byref(h)))
            self._ctx, self._handle, self._pid, self._model_handle, self._prev = self.model._ctx, h, os.getpid(), mh, None
        return lib, self._handle

    def close(self):
        DeviceHandle.close(self)                                   # the handle frees its own blocks and reads nothing of the model
        self._prev = self._model_handle = None

    def reset(self) -> None:
        """Forgets the kept rows and the previous window: the next call computes every frame."""
        self._prev = None
        if self._handle is not None and self._pid == os.getpid():
            lib, h = self._get()
            lib.check(lib.dll.ry_crepe_stream_reset(h))

    def _overlap_ok(self, x, advance) -> bool:
        old = self._prev
        if advance is None or old is None or not 0 <= advance < old.size:
            return False
        m = min(x.size, old.size - advance)
        return bool(numpy.array_equal(x[:m].view(numpy.uint32), old[advance:advance + m].view(numpy.uint32)))

    def track(self, audio, sr, hop: int, step_size, threshold: float = 0.1, advance: Optional[int] = None, device: bool = False):
        """What `CrepeModel.track` returns for the window (`ry_crepe_stream_track`)."""
        sr = _rate(sr)
        x = numpy.ascontiguousarray(audio, dtype=numpy.float32).ravel()
        lib, h = self._get()
        model = self.model
        n = model._frames_at(x.size, sr, hop)
        adv = -1 if advance is None else int(advance)
        ok = self._overlap_ok(x, None if advance is None else adv)
        nf, nc = ctypes.c_int(), ctypes.c_int()
        head = (h, _lib._fptr(x), x.size, sr, int(hop), float(step_size), float(threshold), adv, int(ok), ctypes.byref(nf), ctypes.byref(nc))
        if not device:
            voiced, f64, t64 = numpy.empty(n, numpy.uint8), numpy.empty(n, numpy.float64), numpy.empty(n, numpy.float64)
            lib.check(lib.dll.ry_crepe_stream_track(*head, voiced.ctypes.data_as(_UBP), _dptr(f64), _dptr(t64), 0))
        else:
            lib.check(lib.dll.ry_crepe_stream_track(*head, None, None, None, 1))
        assert nf.value == n, (nf.value, n)
        self._prev = x.copy()                                      # after the call: a refused window is not the previous one
        self.frames, self.computed = nf.value, nc.value
        if not device:
            return voiced.astype(bool), f64, t64
        mh = self._model_handle
        p = [ctypes.c_void_p() for _ in range(4)]
        ns, nfr = ctypes.c_int(), ctypes.c_int()
        lib.check(lib.dll.ry_crepe_track_buffers(mh, ctypes.byref(p[0]), ctypes.byref(ns), ctypes.byref(nfr), *[ctypes.byref(q) for q in p[1:]]))
        return DeviceTrack(model, model._ctx, p[0].value, ns.value, nfr.value, p[1].value, p[2].value, p[3].value)

    def activation(self) -> numpy.ndarray:
        """The assembled activation [frames][360] of the last call (`ry_crepe_stream_activation`)."""
        lib, h = self._get()
        out = numpy.empty((self.frames, BINS), numpy.float32)
        lib.check(lib.dll.ry_crepe_stream_activation(h, _lib._fptr(out), 0))
        return out

    def poison(self) -> int:
        """Tests: NaN bit patterns in everything of the stream but the rows the next call may keep -> how many those are
        (`ry_crepe_stream_debug_poison`)."""
        lib, h = self._get()
        left = ctypes.c_int()
        lib.check(lib.dll.ry_crepe_stream_debug_poison(h, ctypes.byref(left)))
        return left.value


class CrepeStreamBank(DeviceHandle):
    """`CrepeStream` for the B live streams one process serves, in ONE call per buffer (`ry_crepe_bank_*`): `CrepeModel.track_many` on the next
    window of every stream that takes part, each wave under the rule of `CrepeStream` against the kept call of its own stream (DESIGN.md section
    19).  Every stream has a pair of activation slots of its own on the card, so a stream that sits calls out finds its rows intact when it
    returns; the object keeps the previous window of every stream and compares each overlap as 32-bit words before it declares it.  Wave by wave
    the result has the bits of `model.track` on that window.  `computed` / `frames`: per stream, the frames of its last window that went through
    the network / that it has."""
    _destroy = 'ry_crepe_bank_destroy'

    def __init__(self, model: CrepeModel, n_streams: int):
        self.model = model
        self.n_streams = int(n_streams)
        if self.n_streams < 1:
            raise ValueError('a bank has at least one stream, got %d' % self.n_streams)
        self.computed, self.frames = [0] * self.n_streams, [0] * self.n_streams
        self._prev = [None] * self.n_streams
        self._model_handle = None
        DeviceHandle.__init__(self, model._given_ctx, model.device)

    def __getstate__(self):
        d = DeviceHandle.__getstate__(self)
        d.update(_prev=[None] * self.n_streams, _model_handle=None)
        return d

    def _get(self):
        """-> (library, bank handle) of this process, over the model's handle as it is now."""
        lib, mh = self.model._get()
        if self._handle is None or self._pid != os.getpid() or self._model_handle is not mh:
            h = ctypes.c_void_p()
            lib.check(lib.dll.ry_crepe_bank_create(mh, self.n_streams, ctypes.byref(h)))
            self._ctx, self._handle, self._pid, self._model_handle = self.model._ctx, h, os.getpid(), mh
            self._prev = [None] * self.n_streams
        return lib, self._handle

    def close(self):
        DeviceHandle.close(self)                                   # the handle frees its own blocks and reads nothing of the model
        self._prev, self._model_handle = [None] * self.n_streams, None

    def _streams(self, stream):
        if stream is None:
            return list(range(self.n_streams))
        if not 0 <= int(stream) < self.n_streams:
            raise ValueError('stream %s of %d' % (stream, self.n_streams))
        return [int(stream)]

    def reset(self, stream: Optional[int] = None) -> None:
        """Forgets the kept rows and the previous window of `stream` (None: of every stream): its next window is computed in full."""
        which = self._streams(stream)
        for s in which:
            self._prev[s] = None
        if self._handle is not None and self._pid == os.getpid():
            lib, h = self._get()
            lib.check(lib.dll.ry_crepe_bank_reset(h, -1 if stream is None else which[0]))

    def _overlap_ok(self, s: int, x, advance) -> bool:
        old = self._prev[s]
        if advance is None or old is None or not 0 <= advance < old.size:
            return False
        m = min(x.size, old.size - advance)
        return bool(numpy.array_equal(x[:m].view(numpy.uint32), old[advance:advance + m].view(numpy.uint32)))

    def track_many(self, windows, sr, hop: int, step_size, threshold: float = 0.1, advances=None, device: bool = True, order=None):
        """windows: one array per stream, None for a stream that sits the call out; advances: None, one int for all, or one entry per stream (an
        entry may be None: that window is computed in full and kept).  -> (what `CrepeModel.track_many` returns for the windows that are there, in
        stream order -- `DeviceTracks`, or with device=False [(voiced, f0, t)] --, [computed frames] per such window).  order (tests): the
        streams that take part, in the order their windows lie in the call, instead of stream order."""
        windows = list(windows)
        if len(windows) != self.n_streams:
            raise ValueError('%d windows for %d streams' % (len(windows), self.n_streams))
        if advances is None or isinstance(advances, (int, numpy.integer)):
            advances = [advances] * self.n_streams
        advances = list(advances)
        if len(advances) != self.n_streams:
            raise ValueError('%d advances for %d streams' % (len(advances), self.n_streams))
        part = [s for s, w in enumerate(windows) if w is not None]
        if not part:
            raise ValueError('track_many needs at least one window')
        if order is not None:
            if sorted(int(s) for s in order) != part:
                raise ValueError('order %s does not name the streams that take part, %s' % (list(order), part))
            part = [int(s) for s in order]
        sr = _rate(sr)
        xs = [numpy.ascontiguousarray(windows[s], dtype=numpy.float32).ravel() for s in part]
        lib, h = self._get()
        model = self.model
        want = [model._frames_at(x.size, sr, hop) for x in xs]
        adv = [-1 if advances[s] is None else int(advances[s]) for s in part]
        ok = [int(self._overlap_ok(s, x, None if advances[s] is None else a)) for s, x, a in zip(part, xs, adv)]
        as_i = lambda v: numpy.ascontiguousarray(v, dtype=numpy.int32)
        counts, stream_of, adv, ok = as_i([x.size for x in xs]), as_i(part), as_i(adv), as_i(ok)
        audio = numpy.ascontiguousarray(numpy.concatenate(xs))
        nf, nc = numpy.zeros(len(xs), numpy.int32), numpy.zeros(len(xs), numpy.int32)
        _IP = ctypes.POINTER(ctypes.c_int)
        ip = lambda a: a.ctypes.data_as(_IP)
        head = (h, _lib._fptr(audio), ip(counts), ip(stream_of), len(xs), sr, int(hop), float(step_size), float(threshold), ip(adv), ip(ok), ip(nf), ip(nc))
        if not device:
            n = int(sum(want))
            voiced, f64, t64 = numpy.empty(n, numpy.uint8), numpy.empty(n, numpy.float64), numpy.empty(n, numpy.float64)
            lib.check(lib.dll.ry_crepe_bank_track(*head, voiced.ctypes.data_as(_UBP), _dptr(f64), _dptr(t64), 0))
        else:
            lib.check(lib.dll.ry_crepe_bank_track(*head, None, None, None, 1))
        assert list(nf) == want, (list(nf), want)
        for i, s in enumerate(part):                               # after the call: a refused window is not the previous one
            self._prev[s] = xs[i].copy()
            self.frames[s], self.computed[s] = int(nf[i]), int(nc[i])
        computed = [int(c) for c in nc]
        if device:
            return model._tracks_on_card(), computed
        o = numpy.concatenate([[0], numpy.cumsum(nf)])
        return [(voiced[a:b].astype(bool), f64[a:b].copy(), t64[a:b].copy()) for a, b in zip(o[:-1], o[1:])], computed

    def track_uploaded(self, uploaded: UploadedWaves, which, streams, windows, hop: int, step_size, threshold: float = 0.1, advances=None):
        """`track_many(..., device=True)` on the waves `which` (ascending indices) of `uploaded` (`ry_crepe_bank_track_uploaded`): wave which[i] is
        the next window of stream streams[i] and windows[i] the host array that was uploaded for it (the overlap is compared on the host);
        advances: one entry per named wave (None: computed in full).  -> (`UploadedTracks`, [computed frames] per named wave).  A stream that is
        not named keeps its rows."""
        lib, h = self._get()
        model = self.model
        which, first, counts = model._which(uploaded, which)
        part = [int(s) for s in streams]
        xs = [numpy.ascontiguousarray(w, dtype=numpy.float32).ravel() for w in windows]
        advances = [None] * len(which) if advances is None else list(advances)
        if not (len(part) == len(xs) == len(advances) == len(which)) or any(x.size != n for x, n in zip(xs, counts)):
            raise ValueError('one stream, one window of the uploaded length and one advance per tracked wave are needed')
        if any(not 0 <= s < self.n_streams for s in part):
            raise ValueError('streams %s of %d' % (part, self.n_streams))
        want = [model._frames_at(x.size, uploaded.sr, hop) for x in xs]
        adv = [-1 if a is None else int(a) for a in advances]
        ok = [int(self._overlap_ok(s, x, None if a0 is None else a)) for s, x, a0, a in zip(part, xs, advances, adv)]
        as_i = lambda v: numpy.ascontiguousarray(v, dtype=numpy.int32)
        stream_of, adv, ok = as_i(part), as_i(adv), as_i(ok)
        nf, nc = numpy.zeros(len(xs), numpy.int32), numpy.zeros(len(xs), numpy.int32)
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        lib.check(lib.dll.ry_crepe_bank_track_uploaded(h, ip(first), ip(counts), ip(stream_of), len(xs), uploaded.sr, int(hop), float(step_size),
                                                       float(threshold), ip(adv), ip(ok), ip(nf), ip(nc), None, None, None, 1))
        assert list(nf) == want, (list(nf), want)
        for i, s in enumerate(part):                               # after the call: a refused window is not the previous one
            self._prev[s] = xs[i].copy()
            self.frames[s], self.computed[s] = int(nf[i]), int(nc[i])
        return model._uploaded_tracks(uploaded, which), [int(c) for c in nc]

    def activation(self, stream: int) -> numpy.ndarray:
        """The assembled activation [frames][360] of the last window of `stream` (`ry_crepe_bank_activation`)."""
        lib, h = self._get()
        s = self._streams(stream)[0]
        out = numpy.empty((self.frames[s], BINS), numpy.float32)
        lib.check(lib.dll.ry_crepe_bank_activation(h, s, _lib._fptr(out), 0))
        return out

    def poison(self) -> List[int]:
        """Tests: NaN bit patterns in everything of the bank but the rows the next call may keep -> how many those are, per stream
        (`ry_crepe_bank_debug_poison`)."""
        lib, h = self._get()
        left = (ctypes.c_int * self.n_streams)()
        lib.check(lib.dll.ry_crepe_bank_debug_poison(h, left))
        return list(left)

    def uploads(self) -> int:
        """Tests: how many calls have uploaded their tables so far (`ry_crepe_bank_debug_uploads`)."""
        lib, h = self._get()
        n = ctypes.c_longlong()
        lib.check(lib.dll.ry_crepe_bank_debug_uploads(h, ctypes.byref(n)))
        return n.value
