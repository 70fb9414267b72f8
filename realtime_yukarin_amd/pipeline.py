"""A wave in, a wave out, with the feature rows kept on the card: the chain the reference's check.py runs per buffer -- `Vocoder.encode` (CREPE
mode) -> `VoiceChanger.convert_from_acoustic_feature` -> `Vocoder.decode` / `RealtimeVocoder.decode` -- as one object over the handles the three
stages already have:

    from realtime_yukarin_amd import pipeline
    pipeline.install()
    p = pipeline.Pipeline(voice_changer, acoustic_param)
    out = p.convert_wave(wave)                                      # yukarin.Wave at voice_changer.output_sampling_rate

The resident path is `CrepeModel.track(..., device=True)` (the one upload of the wave) -> `Analyzer.extract_resident` (float32 mc / sp / ap rows in
blocks this object owns) -> `VcCore.enqueue_wave_device` (the gate reads the wave the tracker uploaded, stage 1 reads the mc rows, mc and the
converted spectrogram stay on the card) -> `ry_mask_rows` (combine_silent of ap) -> `ry_synth_run` / `ry_synth_push` with device rows.  The host
exchanges the wave (up, once), the track, the mask and the count (down), the converted f0 (up) and the samples (down); f0 goes through the
F0Converter on the host with exactly the numpy operations of the separate calls.  Every result has the bits of the chain of the separate calls:
`encode.extract` -> `VoiceChanger.convert_from_acoustic_feature` -> `world_synth.decode` (or `decode_realtime`), which is also what runs -- unchanged
-- whenever the resident path does not apply (`calls` counts which way a call went)."""
import ctypes
import os
from typing import Optional

import numpy

from . import _lib
from . import crepe as _crepe
from . import encode, gate, world_analysis, world_synth
from .voice_changer import SP_FLOOR
from .world_synth import BINS, FFT_SIZE, cheaptrick_fft_size

calls = {'resident': 0, 'composed': 0}          # which path `convert_wave` / `push` took, counted per call


_feature_class = None


def crepe_feature_class():
    """The feature class the pipeline encodes with unless it is given another: `yukarin`'s plain container (whichever `yukarin` the process imports:
    the converters' F0Converter tells its own container from an array) with the f0 of the reference's CrepeAcousticFeatureWrapper -- `crepe.predict`
    at `encode.model_capacity`, `predict_voicing`, the 0.1 threshold."""
    global _feature_class
    if _feature_class is None:
        from yukarin.acoustic_feature import AcousticFeature

        class CrepeFeature(AcousticFeature):
            @classmethod
            def extract_f0(cls, x, fs, frame_period, f0_floor, f0_ceil):
                from .compat import crepe as shim
                t, f0, confidence, _ = shim.predict(x, fs, viterbi=True, model_capacity=encode.model_capacity, step_size=frame_period, verbose=0)
                voiced = (shim.predict_voicing(confidence) == 1) | (confidence > encode.threshold)
                f0[~voiced] = 0
                return f0, t
        _feature_class = CrepeFeature
    return _feature_class


def install(*crepe_wrappers) -> None:
    """What the resident path needs of the process: D4C from the device (`world_analysis.aperiodicity = device_aperiodicity`) and the feature
    classes named as CREPE classes for `encode` (`crepe_feature_class()`, and every class given here, e.g. the reference's
    CrepeAcousticFeatureWrapper)."""
    world_analysis.aperiodicity = world_analysis.device_aperiodicity
    encode.crepe_classes.update((crepe_feature_class(),) + tuple(crepe_wrappers))


class _Vocoder(object):
    """What `world_synth.decode` / `decode_realtime` read of a vocoder: the composed path hands them the pipeline's synthesizer."""

    def __init__(self, acoustic_param, out_sampling_rate, synthesizer):
        self.acoustic_param, self.out_sampling_rate = acoustic_param, out_sampling_rate
        self._ry_synth = self._synthesizer = synthesizer


class Pipeline(object):
    """`convert_wave(wave)`: one buffer, start to end.  `push(wave, discard)` / `flush()`: the live form -- every buffer is encoded and converted on
    its own, the rows the caller keeps go to one synthesis stream.  `voice_changer`: the mirror `voice_changer.VoiceChanger` over the two converter
    shims; `acoustic_param`: the vocoder's (`Vocoder.acoustic_param`); `feature_class`: the class `Vocoder.encode` would call `extract` on."""

    def __init__(self, voice_changer, acoustic_param, crepe_capacity='full', seed: Optional[int] = None, feature_class=None):
        self.voice_changer, self.acoustic_param = voice_changer, acoustic_param
        self.crepe_capacity = crepe_capacity
        self.feature_class = crepe_feature_class() if feature_class is None else feature_class
        self.seed = int(os.environ.get('RY_SYNTH_SEED', '0')) if seed is None else int(seed)
        self.synth = world_synth.Synthesizer(voice_changer.output_sampling_rate, acoustic_param.frame_period, seed=self.seed,
                                             ctx=world_synth.engine_for_tests.ctx)
        self._vocoder = _Vocoder(acoustic_param, voice_changer.output_sampling_rate, self.synth)
        self.calls = calls
        self._blocks, self._cap, self._ctx, self._pid = {}, 0, None, None

    # ---- the blocks this object owns: grown, never shrunk, freed by `close` in the process that made them
    def _reserve(self, ctx, n: int, m_in: int, m_out: int, f_out: int) -> dict:
        if self._pid != os.getpid() or self._ctx is not ctx:
            self._blocks, self._cap, self._ctx, self._pid = {}, 0, ctx, os.getpid()          # another process / context: its blocks are not ours to free
        widths = dict(mc32=m_in, sp32=BINS, ap32=BINS, mc_out=m_out, sp_out=f_out)
        if n > self._cap or any(self._blocks.get('w_' + k) != w for k, w in widths.items()):
            self._free()
            cap = max(n + n // 2, 64)
            for k, w in widths.items():
                self._blocks[k] = ctx.dev_alloc(cap * w)
                self._blocks['w_' + k] = w
            self._blocks['mask'] = ctx.dev_alloc(cap // 4 + 4)
            self._cap = cap
        return self._blocks

    def _free(self) -> None:
        if self._pid == os.getpid() and self._ctx is not None and self._ctx.handle is not None:
            for k, p in self._blocks.items():
                if not k.startswith('w_'):
                    self._ctx.dev_free(p)
        self._blocks, self._cap = {}, 0

    def close(self) -> None:
        """Frees the device blocks and the synthesizer in the process that created them; the voice changer and the shared handles stay."""
        self._free()
        self.synth.close()

    # ---- which way a call goes
    def _encode_args(self):
        p = self.acoustic_param
        return dict(frame_period=p.frame_period, f0_floor=p.f0_floor, f0_ceil=p.f0_ceil, fft_length=p.fft_length, order=p.order, alpha=p.alpha,
                    dtype=p.dtype)

    def _resident_handles(self, wave):
        """-> (model, analyzer, core, gate thresholds, hop, fft_length of the gate) when every condition of the resident path holds, else None."""
        vc, p = self.voice_changer, self.acoustic_param
        if not encode._fusable(self.feature_class, wave):
            return None
        ac = vc.acoustic_converter
        if not (hasattr(ac, 'fusable') and ac.fusable()):
            return None
        from yukarin.wave import default_effective_ref
        gp = ac.config.dataset.acoustic_param
        thr = vc.threshold if vc.threshold is not None else gp.threshold_db
        w = numpy.asarray(wave.wave)
        if os.environ.get('RY_DEVICE_GATE', '1') == '0' or not gate.device_gate_usable(w, gp.fft_length, thr, default_effective_ref()):
            return None
        fs = int(wave.sampling_rate)
        fft_size = int(p.fft_length) if p.fft_length else cheaptrick_fft_size(fs)
        if fft_size != FFT_SIZE or self.synth.fft_size != FFT_SIZE:
            return None                                                    # 513 bins on both sides
        core = vc._fused_core()
        if core is None or core.F != BINS or ac.desc.in_ch != p.order + 1:
            return None
        from .compat import crepe as shim
        model = shim._model(self.crepe_capacity)
        analyzer = world_analysis._analyzer(fs, fft_size, p.order, float(p.alpha))
        model._get(), analyzer._get(), self.synth._get()
        ctx = core.stage1.ctx
        if not (model._ctx is ctx and analyzer._ctx is ctx and self.synth._ctx is ctx):
            return None                                                    # the rows of one context are not addresses of another
        hop, _ = wave.get_hop_and_length(gp.frame_period)
        return model, analyzer, core, gate.thresholds(thr), hop, int(gp.fft_length)

    # ---- the resident chain up to the rows the synthesizer reads
    def _resident_rows(self, wave, handles, discard):
        """-> (context, blocks, frames, f0 float64 [frames]: the converted track, zeros on the silent frames)."""
        model, analyzer, core, (p_eff, p_all), hop, gate_fft = handles
        vc, p = self.voice_changer, self.acoustic_param
        ac = vc.acoustic_converter
        fs = int(wave.sampling_rate)
        x = numpy.ascontiguousarray(wave.wave, dtype=numpy.float32)
        trk = model.track(x, fs, _crepe.hop_length(p.frame_period), p.frame_period, threshold=encode.threshold, device=True)     # the one upload
        n, ctx = trk.frames, core.stage1.ctx
        b = self._reserve(ctx, n, p.order + 1, core.M, core.F)
        analyzer.extract_resident(trk.wave, trk.samples, trk.f0, trk.t, n, b['mc32'], b['sp32'], b['ap32'])
        track = trk.download()[1]
        discard = (int(discard[0]), int(discard[1])) if os.environ.get('RY_DISCARD_HINT', '1') != '0' else (0, 0)
        if core.discard != discard:
            core.set_discard(*discard)
        effective, n_eff = core.enqueue_wave_device(trk.wave, trk.samples, hop, gate_fft, p_eff, p_all, b['mc32'], n, b['mc_out'], b['sp_out'],
                                                    b['mask'], SP_FLOOR)
        # f0: the numpy operations of the separate calls -- astype_only_float(dtype), indexing(effective), the F0Converter, combine_silent's
        # float32 zeros, the synthesizer's float64 cast
        from yukarin.acoustic_feature import AcousticFeature
        f0_eff = track[:, None].astype(p.dtype)[effective]
        if n_eff and ac.f0_converter is not None:
            f0_eff = ac.f0_converter.convert(AcousticFeature(f0=f0_eff)).f0
        f0 = numpy.zeros((n, 1), numpy.float32)
        f0[effective] = f0_eff
        return ctx, b, n, numpy.ascontiguousarray(f0.ravel(), dtype=numpy.float64)

    @staticmethod
    def _at(block: int, row: int):
        return _lib._fptr(int(block) + int(row) * BINS * 4)

    def _composed_feature(self, wave, discard):
        saved = encode.model_capacity
        encode.model_capacity = self.crepe_capacity                        # `encode.extract` and the default class's `extract_f0` read it
        try:
            f = encode.extract(self.feature_class, wave, **self._encode_args())
        finally:
            encode.model_capacity = saved
        f.wave = wave
        return self.voice_changer.convert_from_acoustic_feature(f, discard)

    # ---- calls
    def convert_wave(self, wave):
        """`yukarin.Wave` in (mono float32 at the input rate for the resident path) -> `yukarin.Wave` (float64) at the output rate."""
        from yukarin import Wave
        handles = self._resident_handles(wave)
        if handles is None:
            calls['composed'] += 1
            return world_synth.decode(self._vocoder, self._composed_feature(wave, (0, 0)))
        calls['resident'] += 1
        ctx, b, n, f0 = self._resident_rows(wave, handles, (0, 0))
        ctx.mask_rows(b['ap32'], b['mask'], n, BINS)
        lib, h = self.synth._get()
        y = numpy.empty(max(self.synth.length(n), 1), numpy.float64)
        got = ctypes.c_int()
        lib.check(lib.dll.ry_synth_run(h, f0.ctypes.data_as(world_synth._DP), self._at(b['sp_out'], 0), self._at(b['ap32'], 0), n, BINS, 1,
                                       y.ctypes.data_as(world_synth._DP), y.size, ctypes.byref(got)))
        return Wave(y[:got.value], sampling_rate=self.voice_changer.output_sampling_rate)

    def push(self, wave, discard=(0, 0), final: bool = False):
        """One buffer of a live stream: the wave is encoded and converted on its own (as `EncodeStream` / `ConvertStream` do per buffer), the rows
        [front, frames - back) -- what `ConvertStream.process` picks -- go to the synthesis stream, and the samples that are final come back.
        final=True: the stream ends with this buffer (`flush` follows)."""
        from yukarin import Wave
        front, back = int(discard[0]), int(discard[1])
        handles = self._resident_handles(wave)
        if handles is None:
            calls['composed'] += 1
            f = self._composed_feature(wave, (front, back))
            k0, k1 = front, len(f.f0) - back
            out = numpy.empty(0, numpy.float64)
            if k1 > k0:
                picked = f.pick(k0, k1, keys=('f0', 'sp', 'ap'))
                out = world_synth.decode_realtime(self._vocoder, picked).wave
        else:
            calls['resident'] += 1
            ctx, b, n, f0 = self._resident_rows(wave, handles, (front, back))
            k0, k1 = front, n - back
            out = numpy.empty(0, numpy.float64)
            if k1 > k0:
                ctx.mask_rows(b['ap32'], b['mask'], n, BINS, k0, k1)
                lib, h = self.synth._get()
                f0 = numpy.ascontiguousarray(f0[k0:k1])
                y = numpy.empty(max(int(lib.dll.ry_synth_bound(h, k1 - k0, 0)), 1), numpy.float64)
                got = ctypes.c_int()
                lib.check(lib.dll.ry_synth_push(h, f0.ctypes.data_as(world_synth._DP), self._at(b['sp_out'], k0), self._at(b['ap32'], k0), k1 - k0, BINS, 1,
                                                y.ctypes.data_as(world_synth._DP), y.size, ctypes.byref(got)))
                out = y[:got.value].copy()
        if final:
            out = numpy.concatenate([out, self.synth.flush()])
        return Wave(wave=out, sampling_rate=self.voice_changer.output_sampling_rate)

    def flush(self):
        """Ends the live stream: the samples `push` still held back; the next `push` starts a new signal."""
        from yukarin import Wave
        return Wave(wave=self.synth.flush(), sampling_rate=self.voice_changer.output_sampling_rate)
