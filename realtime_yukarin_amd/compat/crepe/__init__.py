"""`crepe` on the MI355X: the functions of the crepe package (and its PyTorch fork) that the reference calls --
`predict(audio, sr, viterbi, model_capacity, center, step_size, verbose)` and `predict_voicing(confidence)`
(realtime-yukarin: realtime_voice_conversion/yukarin_wrapper/acoustic_feature_wrapper.py:65-80) -- plus `get_activation` and
`load_model`.  Resampling to 16 kHz, the network, the decode and the Viterbi pass run in libry355 (`ry_crepe_*`); the mono average,
the float32 cast and `predict_voicing` run on the host (`predict_voicing` and the wrapper's mask also exist on the device:
`CrepeModel.voicing`, used by `realtime_yukarin_amd.encode.extract`; this module's functions do not change).  RY_CREPE_RESAMPLE=host resamples with the host statement of the same
arithmetic instead (`realtime_yukarin_amd.crepe.resample`: the same bits, far slower); a rate that is not a whole number of Hz always does.
RY_CREPE_DTYPE=bf16x3 (default f32) runs the network's GEMMs in split-bf16 form (`CrepeModel.set_dtype`); it is read when a model is built.

Weights: `load_model(path, capacity)` or the file named by RY_CREPE_MODEL (`.npz` or torch state dict, keys in INTEGRATION.md
section 9).  Without either, every call raises: there are no built-in or random weights."""
import os

import numpy

from realtime_yukarin_amd import crepe as _crepe

__all__ = ['predict', 'get_activation', 'predict_voicing', 'load_model']

model_srate = _crepe.MODEL_SRATE
_weights = {}          # multiplier -> host weights (load_model / RY_CREPE_MODEL)
_models = {}           # multiplier -> CrepeModel (its device handle is created per process)


def load_model(path, capacity='full'):
    """Use the weights in `path` for `capacity` from now on (the file's filter counts must match the capacity)."""
    m, P = _crepe.load_weights(path, capacity)
    _weights[m] = P
    old = _models.pop(m, None)
    if old is not None:
        old.close()
    return path


def _model(model_capacity):
    m = _crepe.multiplier(model_capacity)
    if m in _models:
        return _models[m]
    if m not in _weights:
        path = os.environ.get('RY_CREPE_MODEL')
        if not path:
            raise RuntimeError('crepe: no weights for capacity %r -- set RY_CREPE_MODEL=<.npz or torch state dict of the model> or call '
                               'crepe.load_model(path, capacity) first (INTEGRATION.md section 9)' % (model_capacity,))
        got, P = _crepe.load_weights(path)
        if got != m:
            raise RuntimeError('crepe: RY_CREPE_MODEL=%s holds capacity multiplier %d, the call asks for %r (%d)' % (path, got, model_capacity, m))
        _weights[m] = P
    _models[m] = _crepe.CrepeModel(m, _weights[m], dtype=_dtype())
    return _models[m]


def _dtype():
    dtype = os.environ.get('RY_CREPE_DTYPE', 'f32')
    if dtype not in _crepe.DTYPES:
        raise RuntimeError('crepe: RY_CREPE_DTYPE=%s (f32 or bf16x3)' % dtype)
    return dtype


def _mono(audio):
    audio = numpy.asarray(audio)
    if audio.ndim == 2:
        audio = audio.mean(1)                                   # make mono
    return audio.astype(numpy.float32)


def _resample_on_host(sr):
    mode = os.environ.get('RY_CREPE_RESAMPLE', 'device')
    if mode not in ('device', 'host'):
        raise RuntimeError('crepe: RY_CREPE_RESAMPLE=%s (device or host)' % mode)
    return mode == 'host' or int(sr) != sr


def _run(audio, sr, model_capacity, center, step_size, viterbi):
    model = _model(model_capacity)
    audio, hop = _mono(audio), _crepe.hop_length(step_size)
    if sr != model_srate and _resample_on_host(sr):
        audio, sr = _crepe.resample(audio, sr, model_srate), model_srate
    return model.predict(audio, sr, hop, center=center, viterbi=viterbi)


def get_activation(audio, sr, model_capacity='full', center=True, step_size=10, verbose=1):
    """(frames, 360) float32 salience."""
    return _run(audio, sr, model_capacity, center, step_size, False)[2]


def predict(audio, sr, viterbi=False, model_capacity='full', center=True, step_size=10, verbose=1):
    """(time [s], frequency [Hz], confidence, activation), as the crepe package returns them."""
    f0, confidence, activation = _run(audio, sr, model_capacity, center, step_size, viterbi)
    time = numpy.arange(confidence.shape[0]) * step_size / 1000.0
    return time, f0.astype(numpy.float64), confidence, activation


def predict_voicing(confidence):
    return _crepe.predict_voicing(confidence)
