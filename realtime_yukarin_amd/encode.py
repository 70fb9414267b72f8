"""The CREPE-mode encode stage in one device call: wave -> f0 (CREPE, its 360-state Viterbi decode, the voicing HMM and the mask) -> CheapTrick,
sp2mc and D4C, with one upload of the wave, no download of the activation and no host arithmetic between the units.  `extract` is a drop-in
body of the reference's `AcousticFeature.extract` like `world_analysis.extract`, which it calls unchanged whenever the fused path does not apply:

    from realtime_yukarin_amd import encode, world_analysis
    world_analysis.aperiodicity = world_analysis.device_aperiodicity
    encode.install(AcousticFeature, CrepeAcousticFeatureWrapper)

What the fused path replaces is `cls.extract_f0` of the reference's CrepeAcousticFeatureWrapper (`crepe.predict(x, fs, viterbi=True,
model_capacity='full', step_size=frame_period)`, `crepe.predict_voicing(confidence)`, `(path == 1) | (confidence > 0.1)`, `f0[~voiced] = 0`)
followed by `Analyzer.run`: the results have that chain's bits.  It does not call `cls.extract_f0`, so it is taken only for the classes the
integrator names in `crepe_classes` (and their subclasses) -- those whose `extract_f0` is that body."""
import numpy

from . import crepe as _crepe
from . import world_analysis
from .world_synth import cheaptrick_fft_size

crepe_classes = set()              # classes whose extract_f0 is the reference's CREPE body (`install` adds one)
model_capacity = 'full'            # the capacity the wrapper asks `crepe.predict` for (tests set a smaller one)
threshold = 0.1                    # its confidence threshold
max_many_frames = 1 << 22         # frames one `Analyzer.run_device_many` takes (`ry_analysis_extract_many_dev`); a longer list is encoded wave by wave
calls = {'fused': 0, 'unfused': 0, 'many': 0}      # which path `extract` took, counted per call; 'many': batched calls of `extract_many`


def install(acoustic_feature, *crepe_wrappers) -> None:
    """`acoustic_feature.extract` becomes `extract`; every class in `crepe_wrappers` is named as one whose f0 is the CREPE chain."""
    acoustic_feature.extract = classmethod(extract)
    crepe_classes.update(crepe_wrappers)


def _fusable(cls, wave) -> bool:
    if not any(issubclass(cls, k) for k in crepe_classes):
        return False
    if world_analysis.aperiodicity is not world_analysis.device_aperiodicity:
        return False
    w, fs = numpy.asarray(wave.wave), wave.sampling_rate
    if w.ndim != 1 or w.size == 0 or not numpy.issubdtype(w.dtype, numpy.floating):
        return False                                                    # the shim averages channels on the host; an empty wave: its refusal as it is
    if int(fs) != fs:
        return False
    from .compat import crepe as shim
    if fs != shim.model_srate and shim._resample_on_host(fs):
        return False
    # the chain analyses wave.astype(float64) and tracks its float32 cast: one float32 upload serves both only when they hold the same values
    return w.dtype == numpy.float32 or bool(numpy.array_equal(w.astype(numpy.float32).astype(w.dtype), w))


def extract(cls, wave, frame_period, f0_floor, f0_ceil, fft_length, order, alpha, dtype):
    """Drop-in body of `AcousticFeature.extract`.  Fused when `cls` derives from a class in `crepe_classes`, `world_analysis.aperiodicity` is
    `device_aperiodicity`, the wave is mono, not empty and holds float32 values (float32, or a float type that round-trips through it), the rate is a
    whole number of Hz and RY_CREPE_RESAMPLE is not `host`; otherwise `world_analysis.extract(cls, ...)`, unchanged.  Returns the plain container."""
    if not _fusable(cls, wave):
        calls['unfused'] += 1
        return world_analysis.extract(cls, wave, frame_period, f0_floor, f0_ceil, fft_length, order, alpha, dtype)
    calls['fused'] += 1
    from .compat import crepe as shim
    fs = int(wave.sampling_rate)
    x = numpy.ascontiguousarray(wave.wave, dtype=numpy.float32)
    model = shim._model(model_capacity)
    fft_size = int(fft_length) if fft_length else cheaptrick_fft_size(fs)
    analyzer = world_analysis._analyzer(fs, fft_size, order, float(alpha))
    analyzer._get()
    trk = model.track(x, fs, _crepe.hop_length(frame_period), frame_period, threshold=threshold, device=True)
    if trk.ctx is not analyzer._ctx:                                    # two contexts: two streams, nothing orders them but the host
        trk.ctx.lib.check(trk.ctx.lib.dll.ry_sync(trk.ctx.handle))
    sp, mc, ap, coded_ap = analyzer.run_device(trk.wave, trk.samples, trk.f0, trk.t, trk.frames, want=('sp', 'mc', 'ap', 'coded_ap'))
    f0 = trk.download()[1]
    voiced = ~(f0 == 0)                                                 # as the unfused body derives it: from the masked f0
    container = next(k for k in cls.__mro__ if 'astype_only_float' in vars(k))
    feature = container(f0=f0[:, None], sp=sp, ap=ap, coded_ap=coded_ap, mc=mc, voiced=voiced[:, None])
    feature = feature.astype_only_float(dtype)
    feature.validate()
    return feature


def _frames(waves, frame_period) -> int:
    """The frames `CrepeModel.track_many` makes of the waves (fusable, one rate): counted as the device counts them."""
    fs, hop = int(waves[0].sampling_rate), _crepe.hop_length(frame_period)
    n16 = [numpy.asarray(w.wave).size if fs == _crepe.MODEL_SRATE else _crepe.resampled_length(numpy.asarray(w.wave).size, fs) for w in waves]
    return sum(_crepe.n_frames(n, hop, True) if n >= 1 else 0 for n in n16)


def extract_many(cls, waves, frame_period, f0_floor, f0_ceil, fft_length, order, alpha, dtype):
    """`extract` for a list of waves in one device call: -> a list of containers, one per wave, each equal to
    `extract(cls, wave, ...)` bit for bit.  Batched (`calls['many']` counts the call) when every wave passes the conditions of the fused path and
    all share one sampling rate and the list has at most `max_many_frames` frames in all (what one analysis call takes); otherwise
    `[extract(cls, w, ...) for w in waves]`, each counted as `extract` counts it.  An empty list: []."""
    waves = list(waves)
    args = (frame_period, f0_floor, f0_ceil, fft_length, order, alpha, dtype)
    if not waves or not all(_fusable(cls, w) for w in waves) or len({int(w.sampling_rate) for w in waves}) != 1 or _frames(waves, frame_period) > max_many_frames:
        return [extract(cls, w, *args) for w in waves]
    calls['many'] = calls.get('many', 0) + 1
    from .compat import crepe as shim
    fs = int(waves[0].sampling_rate)
    xs = [numpy.ascontiguousarray(w.wave, dtype=numpy.float32) for w in waves]
    model = shim._model(model_capacity)
    fft_size = int(fft_length) if fft_length else cheaptrick_fft_size(fs)
    analyzer = world_analysis._analyzer(fs, fft_size, order, float(alpha))
    analyzer._get()
    trk = model.track_many(xs, fs, _crepe.hop_length(frame_period), frame_period, threshold=threshold, device=True)
    if trk.ctx is not analyzer._ctx:                                    # two contexts: two streams, nothing orders them but the host
        trk.ctx.lib.check(trk.ctx.lib.dll.ry_sync(trk.ctx.handle))
    sp, mc, ap, coded_ap = analyzer.run_device_many(trk.wave, trk.sample_offsets, trk.f0, trk.t, trk.frame_offsets, want=('sp', 'mc', 'ap', 'coded_ap'))
    container = next(k for k in cls.__mro__ if 'astype_only_float' in vars(k))
    out, o = [], trk.frame_offsets
    for i, (_, f0) in enumerate(trk.download()):
        a, b = int(o[i]), int(o[i + 1])
        voiced = ~(f0 == 0)                                             # as the unfused body derives it: from the masked f0
        feature = container(f0=f0[:, None], sp=sp[a:b], ap=ap[a:b], coded_ap=coded_ap[a:b], mc=mc[a:b], voiced=voiced[:, None])
        feature = feature.astype_only_float(dtype)
        feature.validate()
        out.append(feature)
    return out
