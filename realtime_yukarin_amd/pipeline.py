"""A wave in, a wave out, with the feature rows kept on the card: the chain the reference's check.py runs per buffer -- `Vocoder.encode` (CREPE
mode) -> `VoiceChanger.convert_from_acoustic_feature` -> `Vocoder.decode` / `RealtimeVocoder.decode` -- as one object over the handles the three
stages already have:

    from realtime_yukarin_amd import pipeline
    pipeline.install()
    p = pipeline.Pipeline(voice_changer, acoustic_param)
    out = p.convert_wave(wave)                                      # yukarin.Wave at voice_changer.output_sampling_rate

The resident path is `CrepeModel.track(..., device=True)` (the one upload of the wave) -> `Analyzer.extract_resident` (float32 mc / sp / ap rows in
blocks this object owns) -> `VcCore.enqueue_wave_device` (the gate reads the wave the tracker uploaded, stage 1 reads the mc rows, mc and the
converted spectrogram stay on the card) -> `ry_mask_rows` (combine_silent of ap) -> `Synthesizer.synthesize` / `push` on device rows.  The host
exchanges the wave (up, once), the track, the mask and the count (down), the converted f0 (up) and the samples (down); f0 goes through the
F0Converter on the host with exactly the numpy operations of the separate calls.  Every result has the bits of the chain of the separate calls:
`encode.extract` -> `VoiceChanger.convert_from_acoustic_feature` -> `world_synth.decode` (or `decode_realtime`), which is also what runs -- unchanged
-- whenever the resident path does not apply (`calls` counts which way a call went).

`gate_first=True` (at construction, or per call) is the resident path with the silence gate in front of the encode stage: the waves go up once
(`CrepeModel.upload_waves`), `VcCore.gate_verdict_waves_device` gives every wave's mask and count with one wait, and only the waves with an
effective frame go through the tracker (`track_uploaded`) and the analysis (`Analyzer.extract_spans_resident`, rows at the wave's place in the
layout of the whole call); `VcCore.enqueue_waves_masked_device` then runs every wave's window on that verdict.  A wave without an effective frame
costs no tracker, CheapTrick, sp2mc or D4C kernel, none of its feature rows is read, and every sample of every stream keeps its bits (DESIGN.md
section 21).  `calls['gated']` counts the waves skipped; `last_gate` is the record of the last such call.

`f0_mode='world'` (the reference's default `extract_f0_mode`): f0 comes from a host callable -- `pyworld.harvest` through the feature class's
`extract_f0` unless `f0_fn` is given -- and the resident path starts at `Analyzer.upload_waves` / `Analyzer.ingest_tracks` instead of the CREPE
tracker; no CREPE model is built.  The bits are those of the composed chain with the same callable (`world_analysis.extract` ->
`convert_from_acoustic_feature` -> `world_synth.decode`), which also runs whenever the callable's track is not the one the frame-count rule
expects; with `gate_first` a silent wave costs no host f0 call."""
import os
from typing import Optional

import numpy

from . import crepe as _crepe
from . import encode, gate, world_analysis, world_synth
from .voice_changer import SP_FLOOR
from .world_synth import BINS, FFT_SIZE, cheaptrick_fft_size

calls = {'resident': 0, 'composed': 0}          # which path `convert_wave` / `push` took, counted per call; 'gated' (from the first gate_first
                                                # call on): the waves whose encode stage the gate skipped
routes = {'gate_device': 0, 'gate_host': 0}     # how the samples of a `push(..., out_gate=g)` reached the gate, counted per call: read where the
                                                # synthesizer wrote them on the card, or brought down and handed over through the host


def _note_gate(owner, counter: dict, record: dict) -> None:
    """What a gate_first call leaves behind: the waves whose encode stage it skipped, counted, and its record."""
    counter['gated'] = counter.get('gated', 0) + len(record['tracked']) - sum(record['tracked'])
    owner.last_gate = record


def _gate_on_card(out_gate, ctx) -> bool:
    """The samples can stay on the card: the gate judges there and lives in the context whose stream the synthesizer writes on."""
    return out_gate is not None and hasattr(out_gate, 'on_device') and out_gate.on_device(ctx)


def _through_host_gate(out_gate, out):
    """The host route through an output gate: the samples that came down -- one array, or the list a bank of gates takes -- are handed over, and
    what the gate does not emit comes back empty, in the gate's dtype."""
    routes['gate_host'] += 1
    emitted = lambda o: o if o is not None else numpy.empty(0, out_gate.dtype)
    got = out_gate.push(out)
    return [emitted(o) for o in got] if isinstance(out, list) else emitted(got)


def _apply_discard(core, discard) -> None:
    """The discard hint of the window calls that follow (none when the environment switches it off), set only when the core has another."""
    discard = (int(discard[0]), int(discard[1])) if os.environ.get('RY_DISCARD_HINT', '1') != '0' else (0, 0)
    if core.discard != discard:
        core.set_discard(*discard)


def _device_rows(b, first: int, counts):
    """The rows the synthesizer reads where the chain left them -- sp in `sp_out`, ap in `ap32` -- from row `first` on: one (sp, ap) pair of
    `DeviceRows` per count, each behind the other."""
    starts = first + numpy.concatenate([[0], numpy.cumsum(counts)])
    return [tuple(world_synth.DeviceRows(b[k] + int(at) * BINS * 4, int(n)) for k in ('sp_out', 'ap32')) for at, n in zip(starts, counts)]


def _spanned(advance, pending):
    """The advance of a buffer against the window its stream's tracker keeps: the caller's, plus those of the buffers the gate skipped since
    (None: one of them declared nothing, so neither does this one)."""
    return None if advance is None or pending is None else int(advance) + int(pending)


def _gate_first_rows(handles, acoustic_param, voice_changer, waves, discard, reserve, tracker=None, streams=None, advances=None):
    """The resident chain with the gate in front, for the waves of one call -> (context, blocks, frame offsets int32 [waves + 1], [f0 float64
    [frames_i]], record).  tracker / streams / advances (`push(..., advance=a)`): a `CrepeStreamBank`, the stream of every wave and its advance
    against the window that stream's tracker keeps; None: `CrepeModel.track_uploaded`.  record: n_eff per wave, which waves were tracked, and the
    frames of each that went through the network where a stream bank ran (None for a wave that was skipped)."""
    model, analyzer, core, (p_eff, p_all), hop, gate_fft = handles
    p, ac = acoustic_param, voice_changer.acoustic_converter
    fs = int(waves[0].sampling_rate)
    xs = [numpy.ascontiguousarray(w.wave, dtype=numpy.float32).ravel() for w in waves]
    hop16 = _crepe.hop_length(p.frame_period)
    up = model.upload_waves(xs, fs)                                        # the one upload
    fo = numpy.concatenate([[0], numpy.cumsum([_crepe.track_frames(x.size, fs, hop16) for x in xs])]).astype(numpy.int32)
    n, ctx = int(fo[-1]), core.stage1.ctx
    b = reserve(ctx, n, p.order + 1, core.M, core.F)
    effective, n_eff = core.gate_verdict_waves_device(up.wave, up.offsets, fo, hop, gate_fft, p_eff, p_all, b['mask'])      # the one wait of the gate
    which = [i for i in range(len(xs)) if n_eff[i] > 0]
    tracks, computed = {}, [None] * len(xs)
    if which:
        if tracker is None:
            trk = model.track_uploaded(up, which, hop16, p.frame_period, threshold=encode.threshold)
        else:
            trk, comp = tracker.track_uploaded(up, which, [streams[i] for i in which], [xs[i] for i in which], hop16, p.frame_period,
                                               threshold=encode.threshold, advances=[advances[i] for i in which])
            for i, c in zip(which, comp):
                computed[i] = c
        if list(numpy.diff(trk.frame_offsets)) != [int(fo[i + 1] - fo[i]) for i in which]:
            raise RuntimeError('the tracker returned %s frames, the frame-count rule says %s' % (list(numpy.diff(trk.frame_offsets)), list(numpy.diff(fo))))
        analyzer.extract_spans_resident(trk.wave, trk.samples, trk.first_sample, trk.n_samples, trk.f0, trk.t, trk.frame_offsets,
                                        [int(fo[i]) for i in which], b['mc32'], b['sp32'], b['ap32'])
        tracks = dict(zip(which, trk.download()))
    _apply_discard(core, discard)
    core.enqueue_waves_masked_device(fo, b['mc32'], b['mc_out'], b['sp_out'], b['mask'], effective, n_eff, SP_FLOOR)
    f0s = [_converted_f0(ac, p.dtype, tracks[i][1] if i in tracks else None, effective[fo[i]:fo[i + 1]]) for i in range(len(xs))]
    record = dict(n_eff=[int(k) for k in n_eff], tracked=[i in tracks for i in range(len(xs))], n_computed=computed)
    return ctx, b, fo, f0s, record


def _track_fits(f0, t, n: int, frame_period) -> bool:
    """WORLD mode: what the f0 callable returned is a track the ingest kernel restates -- n frames, t = k * frame_period / 1000 to the bit."""
    return f0.ndim == 1 and t.ndim == 1 and f0.size == n and t.size == n and bool(numpy.array_equal(t, world_analysis.frame_times(n, frame_period)))


def _world_f0(f0_fn, wave, acoustic_param):
    """The host f0 call of WORLD mode on `wave.wave.astype(float64)`, what `AcousticFeature.extract` hands `extract_f0` -> (f0, t) float64."""
    p = acoustic_param
    f0, t = f0_fn(wave.wave.astype(numpy.float64), wave.sampling_rate, p.frame_period, p.f0_floor, p.f0_ceil)
    return numpy.asarray(f0, numpy.float64), numpy.asarray(t, numpy.float64)


def _converted_column(ac, column, eff):
    """f0 as the synthesizer reads it, from the float32 column [frames, 1] the encode stage hands on: the numpy operations of the separate calls
    -- indexing(effective), the F0Converter, combine_silent's float32 zeros, the synthesizer's float64 cast.  column None: a wave the gate skipped."""
    from yukarin.acoustic_feature import AcousticFeature
    f0 = numpy.zeros((len(eff), 1), numpy.float32)
    if column is not None:
        f0_eff = column[eff]
        # the converter sees no empty column; one guard for every caller: a wave `_gate_first_rows` tracked has n_eff > 0, so eff.any() holds there
        if eff.any() and ac.f0_converter is not None:
            f0_eff = ac.f0_converter.convert(AcousticFeature(f0=f0_eff)).f0
        f0[eff] = f0_eff
    return numpy.ascontiguousarray(f0.ravel(), dtype=numpy.float64)


def _converted_f0(ac, dtype, track, eff):
    """`_converted_column` of one wave's track (float64 [frames]; None: a wave the gate skipped), after astype_only_float(dtype)."""
    return _converted_column(ac, None if track is None else track[:, None].astype(dtype), eff)


def _world_rows(handles, acoustic_param, voice_changer, waves, discard, reserve, f0_fn, gate_first: bool):
    """The resident chain of WORLD mode for the waves of one call: one upload (`Analyzer.upload_waves`), the host f0 call per wave, one ingest
    (`Analyzer.ingest_tracks`), then the chain of CREPE mode unchanged -> (rows, tracks).  rows: (context, blocks, frame offsets int32 [waves + 1],
    [f0 float64 [frames_i]], record), or None when a track does not fit (another frame count than Harvest's rule, another t): the call then takes
    the composed path.  tracks: {wave index: (f0, t)} of every host f0 call made, so that the composed path does not make them again.
    gate_first: the verdict of the gate first (`VcCore.gate_verdict_waves_device`), the host f0 call and the analysis only for the waves with an
    effective frame; record as `_gate_first_rows` has it (None without the flag)."""
    _, analyzer, core, (p_eff, p_all), hop, gate_fft = handles
    p, ac = acoustic_param, voice_changer.acoustic_converter
    fs = int(waves[0].sampling_rate)
    xs = [numpy.ascontiguousarray(w.wave, dtype=numpy.float32).ravel() for w in waves]
    up = analyzer.upload_waves(xs)                                         # the one upload
    fo = numpy.concatenate([[0], numpy.cumsum([world_analysis.harvest_frames(x.size, fs, p.frame_period) for x in xs])]).astype(numpy.int32)
    n, ctx = int(fo[-1]), core.stage1.ctx
    b = reserve(ctx, n, p.order + 1, core.M, core.F)
    which = list(range(len(xs)))
    if gate_first:
        effective, n_eff = core.gate_verdict_waves_device(up.wave, up.offsets, fo, hop, gate_fft, p_eff, p_all, b['mask'])      # the one wait of the gate
        which = [i for i in which if n_eff[i] > 0]
    tracks = {}
    for i in which:                                                        # a wave the gate skipped costs no host f0 call
        tracks[i] = _world_f0(f0_fn, waves[i], p)
        if not _track_fits(tracks[i][0], tracks[i][1], int(fo[i + 1] - fo[i]), p.frame_period):
            return None, tracks
    if which:
        trk = analyzer.ingest_tracks([tracks[i][0] for i in which], p.frame_period, up, which)
        if gate_first:
            analyzer.extract_spans_resident(trk.wave, trk.samples, trk.first_sample, trk.n_samples, trk.f0, trk.t, trk.frame_offsets,
                                            [int(fo[i]) for i in which], b['mc32'], b['sp32'], b['ap32'])
        else:
            analyzer.extract_many_resident(trk.wave, trk.sample_offsets, trk.f0, trk.t, fo, b['mc32'], b['sp32'], b['ap32'])
    _apply_discard(core, discard)
    if gate_first:
        core.enqueue_waves_masked_device(fo, b['mc32'], b['mc_out'], b['sp_out'], b['mask'], effective, n_eff, SP_FLOOR)
    else:
        effective, n_eff = core.enqueue_waves_device(up.wave, up.offsets, fo, hop, gate_fft, p_eff, p_all, b['mc32'], b['mc_out'], b['sp_out'],
                                                     b['mask'], SP_FLOOR)
    f0s = [_converted_f0(ac, p.dtype, tracks[i][0] if i in tracks else None, effective[fo[i]:fo[i + 1]]) for i in range(len(xs))]
    record = dict(n_eff=[int(k) for k in n_eff], tracked=[i in tracks for i in range(len(xs))], n_computed=[None] * len(xs)) if gate_first else None
    return (ctx, b, fo, f0s, record), tracks


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


class _BlockOwner(object):
    """The device blocks of a `Pipeline` / `PipelineBank`: grown, never shrunk, freed by `close` in the process that made them.  `_blocks` holds
    the feature blocks by name with their widths ('w_' + name), the gate's mask and, once a gate has read samples on the card, the sample block
    'y' of 'w_y' samples."""
    _more_widths = {}                                                      # what a subclass keeps beside the rows of the chain: {name: floats per frame}

    def __init__(self):
        self._blocks, self._cap, self._ctx, self._pid = {}, 0, None, None
        self._table = None                                                 # `PipelineBank.push`: what the index table in 'rows' holds

    def _reserve(self, ctx, n: int, m_in: int, m_out: int, f_out: int) -> dict:
        if self._pid != os.getpid() or self._ctx is not ctx:
            self._blocks, self._cap, self._ctx, self._pid, self._table = {}, 0, ctx, os.getpid(), None     # another process / context: its blocks are not ours to free
        widths = dict(mc32=m_in, sp32=BINS, ap32=BINS, mc_out=m_out, sp_out=f_out, **self._more_widths)
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
        self._blocks, self._cap, self._table = {}, 0, None

    def _sample_block(self, need: int):
        """The block the synthesizer leaves its samples in: one of the blocks `_reserve` has made -- grown when a call may return more than it
        holds (`need`: the sum of `Synthesizer.bound` / `StreamBank.bound`), freed with them in `_free`."""
        b = self._blocks
        if 'y' not in b or need > b['w_y']:
            if 'y' in b:
                self._ctx.dev_free(b.pop('y'))                             # waits for the context stream: the gate's last read has ended
            cap = max(need + need // 2, 4096)
            b['y'], b['w_y'] = self._ctx.dev_alloc(2 * cap), cap           # float64 samples in units of a float
        return world_synth.SampleBlock(b['y'], b['w_y'])


class Pipeline(_BlockOwner):
    """`convert_wave(wave)`: one buffer, start to end.  `push(wave, discard)` / `flush()`: the live form -- every buffer is encoded and converted on
    its own, the rows the caller keeps go to one synthesis stream.  `voice_changer`: the mirror `voice_changer.VoiceChanger` over the two converter
    shims; `acoustic_param`: the vocoder's (`Vocoder.acoustic_param`); `feature_class`: the class `Vocoder.encode` would call `extract` on."""

    def __init__(self, voice_changer, acoustic_param, crepe_capacity='full', seed: Optional[int] = None, feature_class=None, gate_first: bool = False,
                 f0_mode: str = 'crepe', f0_fn=None):
        """f0_mode='world' (the reference's default `extract_f0_mode`): f0 comes from the host -- `f0_fn(x float64, fs, frame_period, f0_floor,
        f0_ceil) -> (f0, t)`, by default the feature class's `extract_f0` (`pyworld.harvest`) -- and enters the resident path through
        `Analyzer.upload_waves` / `ingest_tracks`; no CREPE model is built or asked for, `crepe_capacity` and `advance=` are ignored
        (INTEGRATION.md section 20)."""
        if f0_mode not in ('crepe', 'world'):
            raise ValueError("f0_mode is 'crepe' or 'world', got %r" % (f0_mode,))
        self.voice_changer, self.acoustic_param = voice_changer, acoustic_param
        self.f0_mode = f0_mode
        self.gate_first = bool(gate_first)                                 # the silence gate in front of the encode stage (resident path only)
        self.last_gate = None                                              # the record of the last gate_first call
        self._gate_bank, self._pending = None, 0                           # gate_first with `advance`: a one-stream tracker bank; the advance of the skipped buffers
        self.crepe_capacity = crepe_capacity
        if f0_mode == 'world':
            if feature_class is None:
                from yukarin.acoustic_feature import AcousticFeature as feature_class
            self.feature_class = feature_class
            self.f0_fn = f0_fn if f0_fn is not None else (
                lambda x, fs, frame_period, f0_floor, f0_ceil: feature_class.extract_f0(x=x, fs=fs, frame_period=frame_period, f0_floor=f0_floor,
                                                                                         f0_ceil=f0_ceil))
        else:
            if f0_fn is not None:
                raise ValueError("f0_fn belongs to f0_mode='world': CREPE mode tracks on the card")
            self.feature_class = crepe_feature_class() if feature_class is None else feature_class
            self.f0_fn = None
        self.seed = int(os.environ.get('RY_SYNTH_SEED', '0')) if seed is None else int(seed)
        self.synth = world_synth.Synthesizer(voice_changer.output_sampling_rate, acoustic_param.frame_period, seed=self.seed,
                                             ctx=world_synth.engine_for_tests.ctx)
        self._vocoder = _Vocoder(acoustic_param, voice_changer.output_sampling_rate, self.synth)
        self.calls = calls
        _BlockOwner.__init__(self)
        self._crepe_stream = None                                          # `push(..., advance=a)`: the tracker that keeps rows between buffers

    def close(self) -> None:
        """Frees the device blocks and the synthesizer in the process that created them; the voice changer and the shared handles stay."""
        self._free()
        self._drop_stream()
        self.synth.close()

    def _stream_of(self, model):
        """The pipeline's `CrepeStream` over `model` (made on first use; a stream over another model is closed)."""
        if self._crepe_stream is None or self._crepe_stream.model is not model:
            self._drop_stream()
            self._crepe_stream = _crepe.CrepeStream(model)
        return self._crepe_stream

    def _drop_stream(self) -> None:
        if self._crepe_stream is not None:
            self._crepe_stream.close()
            self._crepe_stream = None
        if self._gate_bank is not None:
            self._gate_bank.close()
            self._gate_bank = None

    def _reset_stream(self, which=(True, True)) -> None:
        """Forgets the kept rows: of the plain form's `CrepeStream` (which[0]) and of the gate_first form's tracker with its accumulated advance
        (which[1]).  A call in one form resets the other: they keep different windows."""
        if which[0] and self._crepe_stream is not None:
            self._crepe_stream.reset()
        if which[1]:
            self._pending = 0
            if self._gate_bank is not None:
                self._gate_bank.reset()

    def _gate_tracker(self, model):
        if self._gate_bank is None or self._gate_bank.model is not model:
            if self._gate_bank is not None:
                self._gate_bank.close()
            self._gate_bank, self._pending = _crepe.CrepeStreamBank(model, 1), 0
        return self._gate_bank

    # ---- which way a call goes
    def _encode_args(self):
        p = self.acoustic_param
        return dict(frame_period=p.frame_period, f0_floor=p.f0_floor, f0_ceil=p.f0_ceil, fft_length=p.fft_length, order=p.order, alpha=p.alpha,
                    dtype=p.dtype)

    @staticmethod
    def _world_fusable(wave) -> bool:
        """WORLD mode's part of `encode._fusable`: D4C from the device, a mono wave that is not empty and holds float32 values, a whole rate."""
        if world_analysis.aperiodicity is not world_analysis.device_aperiodicity:
            return False
        w, fs = numpy.asarray(wave.wave), wave.sampling_rate
        if w.ndim != 1 or w.size == 0 or not numpy.issubdtype(w.dtype, numpy.floating) or int(fs) != fs:
            return False
        # the chain analyses wave.astype(float64): the one float32 upload serves it only when both hold the same values
        return w.dtype == numpy.float32 or bool(numpy.array_equal(w.astype(numpy.float32).astype(w.dtype), w))

    def _resident_handles(self, wave):
        """-> (model, analyzer, core, gate thresholds, hop, fft_length of the gate) when every condition of the resident path holds, else None."""
        vc, p = self.voice_changer, self.acoustic_param
        world = self.f0_mode == 'world'
        if not (self._world_fusable(wave) if world else encode._fusable(self.feature_class, wave)):
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
        model = None                                                       # WORLD mode: no CREPE model is built or asked for
        if not world:
            from .compat import crepe as shim
            model = shim._model(self.crepe_capacity)
            model._get()
        analyzer = world_analysis._analyzer(fs, fft_size, p.order, float(p.alpha))
        analyzer._get(), self.synth._get()
        ctx = core.stage1.ctx
        if not ((model is None or model._ctx is ctx) and analyzer._ctx is ctx and self.synth._ctx is ctx):
            return None                                                    # the rows of one context are not addresses of another
        hop, _ = wave.get_hop_and_length(gp.frame_period)
        return model, analyzer, core, gate.thresholds(thr), hop, int(gp.fft_length)

    # ---- the resident chain up to the rows the synthesizer reads
    def _resident_rows(self, wave, handles, discard, advance=None):
        """-> (context, blocks, frames, f0 float64 [frames]: the converted track, zeros on the silent frames).  advance (an int): the track comes
        from the pipeline's `CrepeStream` -- the same bits, with the rows of the frames shared with the previous buffer kept."""
        model, analyzer, core, (p_eff, p_all), hop, gate_fft = handles
        p = self.acoustic_param
        fs = int(wave.sampling_rate)
        x = numpy.ascontiguousarray(wave.wave, dtype=numpy.float32)
        tracker = model if advance is None else self._stream_of(model)
        extra = {} if advance is None else dict(advance=int(advance))
        trk = tracker.track(x, fs, _crepe.hop_length(p.frame_period), p.frame_period, threshold=encode.threshold, device=True, **extra)     # the one upload
        n, ctx = trk.frames, core.stage1.ctx
        b = self._reserve(ctx, n, p.order + 1, core.M, core.F)
        analyzer.extract_resident(trk.wave, trk.samples, trk.f0, trk.t, n, b['mc32'], b['sp32'], b['ap32'])
        track = trk.download()[1]
        _apply_discard(core, discard)
        effective, _ = core.enqueue_wave_device(trk.wave, trk.samples, hop, gate_fft, p_eff, p_all, b['mc32'], n, b['mc_out'], b['sp_out'],
                                                b['mask'], SP_FLOOR)
        return ctx, b, n, _converted_f0(self.voice_changer.acoustic_converter, p.dtype, track, effective)

    def _rows(self, wave, discard, gate_first: Optional[bool], advance=None, live: bool = False):
        """Which way a call goes, and the resident chain when it goes that way -> ((context, blocks, frames, f0) or None: the composed path, the
        (f0, t) the f0 callable of WORLD mode already returned for this wave or None).  gate_first None: the constructor's.  live (`push`): the
        call belongs to a stream, and a buffer in one form of CREPE mode drops the rows the other form's tracker keeps."""
        handles = self._resident_handles(wave)
        if handles is None:
            return None, None
        gate_first = self.gate_first if gate_first is None else gate_first
        args = (handles, self.acoustic_param, self.voice_changer, [wave], discard, self._reserve)
        if self.f0_mode == 'world':                                        # `advance` is ignored: there are no kept activation rows
            rows, tracks = _world_rows(*args, self.f0_fn, gate_first)
            if rows is None:
                return None, tracks.get(0)                                 # the callable's track does not fit: the composed path, with that track
        elif not gate_first:
            if live:
                self._reset_stream((False, True))
            return self._resident_rows(wave, handles, discard, advance), None
        else:
            if live:
                self._reset_stream((True, False))
            if advance is None:
                rows = _gate_first_rows(*args)
            else:                                                          # against the window the tracker keeps: the buffers skipped since are spanned
                adv = _spanned(advance, self._pending)
                rows = _gate_first_rows(*args, self._gate_tracker(handles[0]), [0], [adv])
                self._pending = 0 if rows[4]['tracked'][0] else adv
        ctx, b, fo, f0s, record = rows
        if record is not None:
            _note_gate(self, calls, record)
        return (ctx, b, int(fo[-1]), f0s[0]), None

    def _composed_extract(self, wave, track=None):
        """The encode stage of the separate calls -> the feature with its wave.  WORLD mode: `world_analysis.extract` over a class whose
        `extract_f0` is the f0 callable -- or hands out `track`, the (f0, t) that callable already returned for this wave."""
        if self.f0_mode == 'world':
            fn = self.f0_fn if track is None else (lambda x, fs, frame_period, f0_floor, f0_ceil: track)
            cls = type('WorldFeature', (self.feature_class,), {'extract_f0': classmethod(
                lambda cls, x, fs, frame_period, f0_floor, f0_ceil: fn(x, fs, frame_period, f0_floor, f0_ceil))})
            f = world_analysis.extract(cls, wave, **self._encode_args())
            f.wave = wave
            return f
        saved = encode.model_capacity
        encode.model_capacity = self.crepe_capacity                        # `encode.extract` and the default class's `extract_f0` read it
        try:
            f = encode.extract(self.feature_class, wave, **self._encode_args())
        finally:
            encode.model_capacity = saved
        f.wave = wave
        return f

    def _composed_feature(self, wave, discard, track=None):
        """The chain of the separate calls up to the converted feature (`_composed_extract`, then the voice changer)."""
        return self.voice_changer.convert_from_acoustic_feature(self._composed_extract(wave, track), discard)

    # ---- calls
    def convert_wave(self, wave, gate_first: Optional[bool] = None):
        """`yukarin.Wave` in (mono float32 at the input rate for the resident path) -> `yukarin.Wave` (float64) at the output rate.  gate_first
        (None: the constructor's): the gate before the encode stage; the composed path ignores it."""
        from yukarin import Wave
        rows, track = self._rows(wave, (0, 0), gate_first)
        if rows is None:
            calls['composed'] += 1
            return world_synth.decode(self._vocoder, self._composed_feature(wave, (0, 0), track))
        calls['resident'] += 1
        ctx, b, n, f0 = rows
        ctx.mask_rows(b['ap32'], b['mask'], n, BINS)
        return Wave(self.synth.synthesize(f0, *_device_rows(b, 0, [n])[0]), sampling_rate=self.voice_changer.output_sampling_rate)

    def push(self, wave, discard=(0, 0), final: bool = False, advance: Optional[int] = None, out_gate=None, gate_first: Optional[bool] = None):
        """One buffer of a live stream: the wave is encoded and converted on its own (as `EncodeStream` / `ConvertStream` do per buffer), the rows
        [front, frames - back) -- what `ConvertStream.process` picks -- go to the synthesis stream, and the samples that are final come back.
        final=True: the stream ends with this buffer (`flush` follows).  advance (an int): sample i of this buffer is sample i + advance of the previous
        one -- consecutive windows of `time_length + 2 * extra_time` share `2 * extra_time` of audio -- and the resident path tracks through a
        `CrepeStream`, which keeps the activation rows of the shared frames when the overlap really holds the same samples: the same bits, fewer frames
        through the network.  The kept rows are dropped by `flush`, by final=True and by a buffer that takes the composed path.
        out_gate (an `output_gate.OutputGate`): the samples go through it -- the tail of the reference's decode worker -- and the returned `Wave` is
        the chunk it emits (scaled, in the gate's dtype), empty when no chunk was completed or the chunk is silent.  On the resident path, with a
        gate that judges on the card in the pipeline's context, the samples never leave the card: the synthesizer writes them into a block of the
        pipeline's (`push_device`, `flush_device` behind it when final), the gate reads them there (ONE `push_device`), and only an audible chunk comes
        down, in the gate's dtype.  Otherwise -- the composed path, a host-fallback gate (chunk below 1025), a gate of another context -- they take
        the host route: the same bits (`routes` counts which).
        gate_first (None: the constructor's): the silence gate runs before the encode stage and a buffer without an effective frame skips the
        tracker and the analysis: the same samples.  Its tracker's kept rows stay, and its `advance` is added to that of the next buffer that is
        tracked, which so spans the buffers skipped.  The composed path ignores the flag."""
        from yukarin import Wave
        front, back = int(discard[0]), int(discard[1])
        rate = self.voice_changer.output_sampling_rate
        rows, track = self._rows(wave, (front, back), gate_first, advance, live=True)
        out = numpy.empty(0, numpy.float64)
        if rows is None:
            calls['composed'] += 1
            self._reset_stream()
            f = self._composed_feature(wave, (front, back), track)
            k0, k1 = front, len(f.f0) - back
            if k1 > k0:
                picked = f.pick(k0, k1, keys=('f0', 'sp', 'ap'))
                out = world_synth.decode_realtime(self._vocoder, picked).wave
        else:
            calls['resident'] += 1
            ctx, b, n, f0 = rows
            k0, k1 = front, n - back
            if _gate_on_card(out_gate, ctx):
                block = self._sample_block(self.synth.bound(k1 - k0, final))
                got = 0
                if k1 > k0:
                    ctx.mask_rows(b['ap32'], b['mask'], n, BINS, k0, k1)
                    got = self.synth.push_device(f0[k0:k1], *_device_rows(b, k0, [k1 - k0])[0], block, 0)
                if final:
                    got += self.synth.flush_device(block, got)             # behind the push, in the same block
                    self._reset_stream()
                routes['gate_device'] += 1
                out = out_gate.push_device(block.address, got)             # the one wait for the samples, and only when a chunk is complete
                return Wave(wave=out if out is not None else numpy.empty(0, out_gate.dtype), sampling_rate=rate)
            if k1 > k0:
                ctx.mask_rows(b['ap32'], b['mask'], n, BINS, k0, k1)
                out = self.synth.push(f0[k0:k1], *_device_rows(b, k0, [k1 - k0])[0])
        if final:
            out = numpy.concatenate([out, self.synth.flush()])
            self._reset_stream()
        if out_gate is not None:
            out = _through_host_gate(out_gate, out)
        return Wave(wave=out, sampling_rate=rate)

    def flush(self):
        """Ends the live stream: the samples `push` still held back; the next `push` starts a new signal."""
        from yukarin import Wave
        self._reset_stream()
        return Wave(wave=self.synth.flush(), sampling_rate=self.voice_changer.output_sampling_rate)


calls_many = {'resident': 0, 'composed': 0}     # which way a `PipelineBank.convert_waves` / `push` went, counted per call


class PipelineBank(_BlockOwner):
    """`Pipeline` for the B streams one process serves, with ONE chain per buffer instead of B: `CrepeModel.track_many` (one upload of all waves) ->
    `Analyzer.extract_many_resident` (one verdict) -> `VcCore.enqueue_waves_device` (one gate, one wait for all counts, then every wave's window) ->
    `ry_mask_rows` / `ry_gather_rows` -> `Synthesizer.synthesize_many` (`convert_waves`) or one `push` of a `StreamBank` with one seed per stream
    (`push`).  What stream b returns, call by call, has the bits a lone `Pipeline(seed=seeds[b])` returns for the same waves, discards and flushes,
    whatever the other streams do.  `seeds=None`: every stream has RY_SYNTH_SEED.  `convert_waves` is a one-shot call outside the streams: its
    synthesizer has the seed of stream 0.  The resident chain runs when every wave of a call meets the conditions of `Pipeline`'s resident path and
    all share one rate; otherwise every wave runs the chain of the separate calls, one after the other, over the same bank: the same bits
    (`calls_many` counts which way a call went)."""

    def __init__(self, voice_changer, acoustic_param, n_streams: int, seeds=None, crepe_capacity='full', feature_class=None, gate_first: bool = False,
                 f0_mode: str = 'crepe', f0_fn=None):
        """f0_mode / f0_fn: as `Pipeline` has them -- WORLD mode runs ONE upload, the host f0 call per wave, ONE ingest and one chain per call."""
        self.gate_first = bool(gate_first)                                # the silence gate in front of the encode stage (resident chain only)
        self.last_gate = None                                              # the record of the last gate_first call
        self.n_streams = int(n_streams)
        if self.n_streams < 1:
            raise ValueError('a bank has at least one stream, got %d' % self.n_streams)
        if seeds is None:
            seeds = [int(os.environ.get('RY_SYNTH_SEED', '0'))] * self.n_streams
        self.seeds = [int(s) for s in seeds]
        if len(self.seeds) != self.n_streams:
            raise ValueError('%d seeds for %d streams' % (len(self.seeds), self.n_streams))
        self.voice_changer, self.acoustic_param = voice_changer, acoustic_param
        self._one = Pipeline(voice_changer, acoustic_param, crepe_capacity=crepe_capacity, seed=self.seeds[0], feature_class=feature_class,
                             f0_mode=f0_mode, f0_fn=f0_fn)
        self.feature_class, self.f0_mode, self.f0_fn = self._one.feature_class, self._one.f0_mode, self._one.f0_fn
        self.bank = world_synth.StreamBank(voice_changer.output_sampling_rate, acoustic_param.frame_period, n_streams=self.n_streams, seeds=self.seeds,
                                           ctx=world_synth.engine_for_tests.ctx)
        self.calls = calls_many
        self._live = [False] * self.n_streams                              # the stream holds frames of a signal that has not ended
        _BlockOwner.__init__(self)
        self._crepe_bank = None                                            # `push(..., advance=a)`: the trackers that keep rows between buffers
        self._pending = [0] * self.n_streams                               # gate_first: the advance of the buffers of a stream skipped since its last tracked one

    _more_widths = dict(sp_pack=BINS, ap_pack=BINS, rows=1)             # the picked rows of a `push`, packed stream by stream, and their index table

    def close(self) -> None:
        """Frees the device blocks, the stream bank and the one-shot synthesizer in the process that created them; the voice changer and the shared
        handles stay."""
        self._free()
        self._drop_trackers()
        self.bank.close()
        self._one.close()

    def _trackers_of(self, model):
        """The bank's `CrepeStreamBank` over `model` (made on first use; one over another model is closed)."""
        if self._crepe_bank is None or self._crepe_bank.model is not model:
            self._drop_trackers()
            self._crepe_bank = _crepe.CrepeStreamBank(model, self.n_streams)
        return self._crepe_bank

    def _drop_trackers(self) -> None:
        if self._crepe_bank is not None:
            self._crepe_bank.close()
            self._crepe_bank = None

    def _reset_trackers(self, streams) -> None:
        streams = list(streams)
        for s in streams:
            self._pending[s] = 0
        if self._crepe_bank is not None:
            for s in streams:
                self._crepe_bank.reset(s)

    # ---- which way a call goes
    def _handles(self, waves):
        """The handles of the resident chain when every wave meets `Pipeline._resident_handles`, all share one rate and the bank lives in their
        context; else None."""
        if len(set(int(w.sampling_rate) for w in waves)) != 1:
            return None
        handles = None
        for w in waves:
            handles = self._one._resident_handles(w)
            if handles is None:
                return None
        self.bank._get()
        return handles if self.bank._ctx is handles[2].stage1.ctx and self.bank.fft_size == FFT_SIZE else None

    # ---- the resident chain up to the rows the synthesizers read
    def _resident_rows(self, waves, handles, discard, part=None, advance=None):
        """-> (context, blocks, frame offsets int32 [waves + 1], [f0 float64 [frames_i]: the converted track of wave i, zeros on the silent frames]).
        part, advance (`push(..., advance=a)`): wave i is the next buffer of stream part[i], advance[i] samples on from the window that stream's
        tracker keeps, and the tracks come from the bank's `CrepeStreamBank` -- the same bits, with the rows of the shared frames kept."""
        model, analyzer, core, (p_eff, p_all), hop, gate_fft = handles
        p, ac = self.acoustic_param, self.voice_changer.acoustic_converter
        fs = int(waves[0].sampling_rate)
        xs = [numpy.ascontiguousarray(w.wave, dtype=numpy.float32) for w in waves]
        if advance is None:
            trk = model.track_many(xs, fs, _crepe.hop_length(p.frame_period), p.frame_period, threshold=encode.threshold, device=True)   # the one upload
        else:
            windows, advances = [None] * self.n_streams, [None] * self.n_streams
            for s, x, a in zip(part, xs, advance):
                windows[s], advances[s] = x, a
            trk, _ = self._trackers_of(model).track_many(windows, fs, _crepe.hop_length(p.frame_period), p.frame_period, threshold=encode.threshold,
                                                         advances=advances, device=True)
        n, ctx, fo = trk.frames, core.stage1.ctx, trk.frame_offsets
        b = self._reserve(ctx, n, p.order + 1, core.M, core.F)
        analyzer.extract_many_resident(trk.wave, trk.sample_offsets, trk.f0, trk.t, fo, b['mc32'], b['sp32'], b['ap32'])
        tracks = trk.download()
        _apply_discard(core, discard)
        effective, _ = core.enqueue_waves_device(trk.wave, trk.sample_offsets, fo, hop, gate_fft, p_eff, p_all, b['mc32'], b['mc_out'], b['sp_out'],
                                                 b['mask'], SP_FLOOR)
        return ctx, b, fo, [_converted_f0(ac, p.dtype, track, effective[fo[i]:fo[i + 1]]) for i, (_, track) in enumerate(tracks)]

    def _rows(self, waves, discard, gate_first: Optional[bool], part=None, advance=None):
        """Which way a call goes, and the resident chain when it goes that way -> ((context, blocks, frame offsets, f0s) or None: the composed
        path, {wave index: the (f0, t) the f0 callable of WORLD mode already returned}).  gate_first None: the constructor's.  part, advance
        (`push`): wave i is the next buffer of stream part[i], with its advance (or advance None); a stream's advance spans the buffers of it that
        gate_first calls skipped since it was last tracked (`_pending`), whichever form tracks it."""
        handles = self._handles(waves)
        if handles is None:
            return None, {}
        gate_first = self.gate_first if gate_first is None else gate_first
        args = (handles, self.acoustic_param, self.voice_changer, waves, discard, self._reserve)
        if self.f0_mode == 'world':                                        # `advance` is ignored: there are no kept activation rows
            rows, tracks = _world_rows(*args, self.f0_fn, gate_first)
            if rows is None:
                return None, tracks                                        # a track does not fit: the composed path, with the tracks made so far
        else:
            adv = None if advance is None else [_spanned(a, self._pending[s]) for s, a in zip(part, advance)]
            if gate_first:
                rows = _gate_first_rows(*args, None if adv is None else self._trackers_of(handles[0]), part, adv)
                if adv is not None:
                    for i, s in enumerate(part):
                        self._pending[s] = 0 if rows[4]['tracked'][i] else adv[i]
            else:
                for s in part or ():
                    self._pending[s] = 0
                rows = self._resident_rows(waves, handles, discard, part, adv) + (None,)
        if rows[4] is not None:
            _note_gate(self, calls_many, dict(rows[4], streams=list(part) if part is not None else None))
        return rows[:4], {}

    # ---- calls
    def convert_waves(self, waves, gate_first: Optional[bool] = None) -> list:
        """A list of `yukarin.Wave` -> the list of their converted waves, each with the bits of `Pipeline(seed=seeds[0]).convert_wave` on it alone.
        gate_first (None: the constructor's): the gate before the encode stage; the composed path ignores it."""
        from yukarin import Wave
        waves = list(waves)
        if not waves:
            return []
        rate = self.voice_changer.output_sampling_rate
        rows, tracks = self._rows(waves, (0, 0), gate_first)
        if rows is None:
            calls_many['composed'] += 1
            return [world_synth.decode(self._one._vocoder, self._one._composed_feature(w, (0, 0), tracks.get(i))) for i, w in enumerate(waves)]
        calls_many['resident'] += 1
        ctx, b, fo, f0s = rows
        ctx.mask_rows(b['ap32'], b['mask'], int(fo[-1]), BINS)
        # consecutive rows of one block: `synthesize_many` reads them in place, in one device call
        items = [(f0, sp, ap) for f0, (sp, ap) in zip(f0s, _device_rows(b, 0, numpy.diff(fo)))]
        return [Wave(y, sampling_rate=rate) for y in self._one.synth.synthesize_many(items)]

    def _final(self, final):
        final = sorted(set(int(s) for s in (final or ())))
        if any(s < 0 or s >= self.n_streams for s in final):
            raise ValueError('final names stream %s of %d' % (final, self.n_streams))
        return final

    def push(self, waves, discard=(0, 0), final=None, advance=None, out_gate=None, gate_first: Optional[bool] = None) -> list:
        """One buffer of every live stream: `waves` has one `yukarin.Wave` per stream, None for a stream that sits the call out; every wave is
        encoded and converted on its own, the rows [front, frames - back) of each go to its synthesis stream, and the samples that are final come
        back -> one `Wave` per stream (empty for a stream that sat out).  `final`: the streams whose signal ends with this call (what `Pipeline.push(
        ..., final=True)` does for one); a stream named there without a wave is flushed.  `advance` (one int, or one entry per stream, None where
        nothing is declared): sample i of a stream's buffer is sample i + advance of that stream's previous buffer, and the resident chain tracks
        through a `CrepeStreamBank`, which keeps per stream the activation rows of the shared frames when the overlap really holds the same samples:
        the same bits, fewer frames through the network.  A stream that sits calls out keeps its rows (its advance then spans the buffers it
        missed).  A stream's kept rows are dropped by `final` naming it, by `flush` of it and by a call it takes part in that takes the composed
        path.  advance=None: the call as it was, through `CrepeModel.track_many`.
        out_gate (an `output_gate.OutputGateBank` of n_streams streams): the samples of all streams go through it in ONE call and every returned
        `Wave` is the chunk its stream's gate emits, empty when no chunk was completed or the chunk is silent; a stream without a sample in this call
        sits the gate's call out.  On the resident chain, with a bank of gates that judges on the card in the pipeline's context, the samples stay
        on the card: ONE `StreamBank.push_device` leaves them back to back in a block of this object's and ONE `OutputGateBank.push_device` reads
        them there.  Otherwise they take the host route, as `Pipeline.push` says: the same bits (`routes` counts which).
        gate_first (None: the constructor's): the silence gate runs before the encode stage, and the streams whose buffer has no effective frame
        skip the tracker and the analysis -- no kernel of either runs when every buffer is silent -- while their synthesis streams, their gates
        and every sample they return go on as before.  A skipped stream keeps its tracker's rows, and the `advance` of every buffer skipped is
        added to that of its next tracked buffer.  The composed path ignores the flag."""
        from yukarin import Wave
        waves = list(waves)
        if len(waves) != self.n_streams:
            raise ValueError('%d waves for %d streams' % (len(waves), self.n_streams))
        if advance is not None and not isinstance(advance, (int, numpy.integer)):
            advance = list(advance)
            if len(advance) != self.n_streams:
                raise ValueError('%d advances for %d streams' % (len(advance), self.n_streams))
        final = self._final(final)
        front, back = int(discard[0]), int(discard[1])
        rate = self.voice_changer.output_sampling_rate
        part = [s for s, w in enumerate(waves) if w is not None]
        outs = [numpy.empty(0, numpy.float64) for _ in range(self.n_streams)]
        on_card = None                                                     # the device route: (block, sample offsets)
        if not part:
            if final:
                outs = self.bank.flush(final)
        else:
            if advance is not None:                                        # per wave of the call
                advance = [advance if isinstance(advance, (int, numpy.integer)) else advance[s] for s in part]
            rows, tracks = self._rows([waves[s] for s in part], (front, back), gate_first, part, advance)
            if rows is None:
                calls_many['composed'] += 1
                self._reset_trackers(part)
                for i, s in enumerate(part):
                    f = self._one._composed_feature(waves[s], (front, back), tracks.get(i))
                    k0, k1 = front, len(f.f0) - back
                    if k1 > k0:
                        picked = f.pick(k0, k1, keys=('f0', 'sp', 'ap'))
                        items = [None] * self.n_streams
                        items[s] = (numpy.asarray(picked.f0).ravel(), picked.sp, picked.ap)
                        outs[s] = self.bank.push(items, final=[s] if s in final else ())[s]
                    elif s in final:
                        outs[s] = self.bank.flush([s])[s]
                rest = [s for s in final if s not in part]
                if rest:
                    got = self.bank.flush(rest)
                    for s in rest:
                        outs[s] = got[s]
            else:
                calls_many['resident'] += 1
                ctx, b, fo, f0s = rows
                picks = [(int(fo[i]) + front, int(fo[i + 1]) - back) for i in range(len(part))]
                picks = [(k0, max(k1, k0)) for k0, k1 in picks]
                total = sum(k1 - k0 for k0, k1 in picks)
                items = [None] * self.n_streams
                if total > 0:
                    key = (tuple(picks), b['rows'])
                    if self._table != key:                                 # live streams repeat their shapes: the table goes up once
                        ctx.dev_upload(b['rows'], numpy.concatenate([numpy.arange(k0, k1, dtype=numpy.int32) for k0, k1 in picks]))
                        self._table = key
                    n = int(fo[-1])
                    ctx.gather_rows(b['sp_out'], n, BINS, b['rows'], b['sp_pack'], total)
                    ctx.gather_rows(b['ap32'], n, BINS, b['rows'], b['ap_pack'], total, mask_ptr=b['mask'])       # combine_silent folded in
                    at = 0
                    for i, s in enumerate(part):
                        k0, k1 = picks[i]
                        if k1 > k0:
                            rows = [world_synth.DeviceRows(b[k] + at * BINS * 4, k1 - k0) for k in ('sp_pack', 'ap_pack')]
                            items[s] = (numpy.ascontiguousarray(f0s[i][k0 - int(fo[i]):k1 - int(fo[i])]), rows[0], rows[1])
                            at += k1 - k0
                if _gate_on_card(out_gate, ctx):
                    took = [s for s in range(self.n_streams) if items[s] is not None or s in final]
                    block = self._sample_block(sum(self.bank.bound(s, 0 if items[s] is None else items[s][0].size, s in final) for s in took))
                    on_card = (block, self.bank.push_device(items, final, block) if took else numpy.zeros(self.n_streams + 1, numpy.int64))
                elif total > 0 or final:
                    outs = self.bank.push(items, final=final)              # one device call: the packed rows follow one another and are read in place
        for s in part:
            self._live[s] = True
        for s in final:
            self._live[s] = False
        self._reset_trackers(final)
        if on_card is not None:
            routes['gate_device'] += 1
            outs = [o if o is not None else numpy.empty(0, out_gate.dtype) for o in out_gate.push_device(on_card[0].address, on_card[1])]
        elif out_gate is not None:
            outs = _through_host_gate(out_gate, outs)
        return [Wave(wave=o, sampling_rate=rate) for o in outs]

    def flush(self, stream=None):
        """Ends the signal of `stream` -> its `Wave`: the samples `push` still held back.  stream=None: ends every stream that holds frames -> one
        `Wave` per stream (empty for the others).  The next `push` of an ended stream starts a new signal."""
        from yukarin import Wave
        rate = self.voice_changer.output_sampling_rate
        if stream is not None:
            out = self.bank.flush([int(stream)])[int(stream)]
            self._live[int(stream)] = False
            self._reset_trackers([int(stream)])
            return Wave(wave=out, sampling_rate=rate)
        live = [s for s in range(self.n_streams) if self._live[s]]
        outs = self.bank.flush(live) if live else [numpy.empty(0, numpy.float64)] * self.n_streams
        self._live = [False] * self.n_streams
        self._reset_trackers(range(self.n_streams))
        return [Wave(wave=o, sampling_rate=rate) for o in outs]


class _LiveState(object):
    """The host state of ONE stream of the three-stream live loop and every rule that reads it, stated once for `LivePipeline` and
    `LivePipelineBank`: the clocks of the three workers, the lists `EncodeStream` / `ConvertStream` / `DecodeStream` keep, the plans
    (`streams.fetch_plan` over them) and the composed path, which is all host arrays.  Nothing here touches the card."""

    def __init__(self, voice_changer, acoustic_param, f0_mode: str, time_length: float, extra):
        from . import streams
        self.streams = streams
        self.voice_changer, self.acoustic_param, self.f0_mode = voice_changer, acoustic_param, f0_mode
        self.time_length, self.extra = time_length, tuple(extra)
        self.start()

    def start(self) -> None:
        """A new signal: the workers' clocks at their first values, no segment anywhere."""
        self.add = list(self.extra)                                        # `start_time = extra_time` of the three workers
        self.now = [0., 0., 0.]                                            # `StreamWrapper._current_time` of the three streams
        self.inputs, self.features, self.outputs = [], [], []              # EncodeStream / ConvertStream / DecodeStream .stream
        self.mode = None                                                   # None until the first push, then 'resident' or 'composed'

    # ---- rates and pads of the three streams, as their constructors take them
    def rates(self):
        vc, p = self.voice_changer, self.acoustic_param
        gp = vc.acoustic_converter.config.dataset.acoustic_param
        sp = vc.super_resolution.config.dataset.param.acoustic_feature_param
        return 1000 // p.frame_period, 1000 // gp.frame_period, 1000 // sp.frame_period

    @staticmethod
    def inner(pad: int, n: int):
        """`pick(data, pad, -pad)` of n elements as numpy slices it (the whole when pad is 0: the streams then do not pick)."""
        return (0, n) if pad <= 0 else _LiveState.clip(pad, -pad, n)

    @staticmethod
    def clip(first, last, n):
        a, b, _ = slice(first, last).indices(n)
        return a, max(a, b)

    def frames(self, n_samples: int, fs) -> int:
        p = self.acoustic_param
        if n_samples < 1:
            return 0
        if self.f0_mode == 'world':
            return world_analysis.harvest_frames(n_samples, fs, p.frame_period)
        return _crepe.track_frames(n_samples, fs, _crepe.hop_length(p.frame_period))

    # ---- host arrays by plan: what `concat` of the picked segments and the pads holds
    @staticmethod
    def concat(spans, arrays, width, dtype):
        parts = [numpy.zeros((b - a,) + width, dtype) if i < 0 else arrays[i][a:b] for i, a, b in spans]
        return numpy.concatenate(parts)

    def take(self, buffer):
        """The encode worker's input stage for one buffer of `time_length` seconds (a float32 array at the vocoder's rate, or a `yukarin.Wave`):
        it joins the kept inputs, the encode window is assembled by the plan and what no later window reaches goes -> the window as a `Wave`."""
        from yukarin import Wave
        S, T = self.streams, self.time_length
        fs = int(buffer.sampling_rate) if hasattr(buffer, 'sampling_rate') else int(self.acoustic_param.sampling_rate)
        x = numpy.asarray(buffer.wave if hasattr(buffer, 'wave') else buffer)
        self.inputs.append((self.add[0], x))
        self.add[0] += T
        in_plan = S.row_spans(S.fetch_plan([(s, len(a)) for s, a in self.inputs], self.now[0], T, self.extra[0], fs), [len(a) for _, a in self.inputs])
        window = self.concat(in_plan, [a for _, a in self.inputs], (), numpy.float32)            # WaveSegmentMethod.pad: float32 zeros
        self.now[0] += T
        del self.inputs[:S.retire([(s, len(a)) for s, a in self.inputs], self.now[0], T, self.extra[0], fs)]
        return Wave(window, fs)

    def plans(self, n_enc: int, n_window: int, fs):
        """Everything the stream arithmetic decides for this buffer, from the clocks and the lengths alone: the rows / samples `EncodeStream` picks
        of an encode window of n_enc frames, the convert window's plan with its clipped row and sample spans and their totals, the convert pad
        and the rows `ConvertStream` picks, and the decode window's clocks and spans."""
        S, p, T = self.streams, self.acoustic_param, self.time_length
        rate_e, rate_c, rate_d = self.rates()
        gp = self.voice_changer.acoustic_converter.config.dataset.acoustic_param
        pad_e = round(self.extra[0] * rate_e)
        ra, rb = self.inner(pad_e, n_enc)
        wa, wb = (0, n_window) if pad_e <= 0 else self.clip(round(pad_e * p.frame_period / 1000 * fs), round(-pad_e * p.frame_period / 1000 * fs), n_window)
        clocks = [(f['start'], f['rows']) for f in self.features] + [(self.add[1], rb - ra)]
        sizes = [f['samples'] for f in self.features] + [wb - wa]
        c_plan = S.fetch_plan(clocks, self.now[1], T, self.extra[1], rate_c)
        c_rows = S.row_spans(c_plan, [n for _, n in clocks])
        c_samples = S.wave_spans(c_plan, gp.frame_period, fs, sizes)
        n_c, n_w = S.span_count(c_rows), S.span_count(c_samples)
        pad_c = round(self.extra[1] * rate_c)
        k0, k1 = self.inner(pad_c, n_c)
        d_clocks = [(o['start'], o['rows']) for o in self.outputs] + [(self.add[2], k1 - k0)]
        d_rows = S.row_spans(S.fetch_plan(d_clocks, self.now[2], T, self.extra[2], rate_d), [n for _, n in d_clocks])
        return (ra, rb), (wa, wb), c_plan, c_rows, c_samples, n_c, n_w, pad_c, (k0, k1), d_clocks, d_rows

    def fits_resident(self, plans) -> bool:
        """The stream's part of the resident path's conditions: the signal has not been composed, the buffer leaves rows and samples to convert,
        and the decode plan hands on exactly the rows just converted."""
        (ra, rb), _, _, _, _, _, n_w, _, (k0, k1), d_clocks, d_rows = plans
        return self.mode != 'composed' and rb > ra and k1 > k0 and n_w > 0 and self.streams.is_identity(d_rows, len(d_clocks) - 1, k1 - k0)

    def add_resident(self, f0_track, plans) -> None:
        """The segment a resident buffer leaves on the host: its clock, its sizes and its f0 column (the rows and the wave are in the store)."""
        (ra, rb), (wa, wb) = plans[0], plans[1]
        self.features.append(dict(start=self.add[1], rows=rb - ra, samples=wb - wa, f0=f0_track[:, None].astype(self.acoustic_param.dtype)[ra:rb]))

    def resident_f0(self, plans, effective):
        """The converted f0 of the rows `ConvertStream` picks, by the convert plan over the kept columns; the decode segment joins its list."""
        c_rows, (k0, k1) = plans[3], plans[8]
        ac = self.voice_changer.acoustic_converter
        f0 = _converted_column(ac, self.concat(c_rows, [f['f0'] for f in self.features], (1,), numpy.float32), effective)[k0:k1]
        self.outputs.append(dict(start=self.add[2], rows=k1 - k0))
        return f0

    def demote(self, download) -> list:
        """The signal leaves the resident path: its live segments come down once (`download(k)` -> (mc, ap, wave) of segment k), and every later
        buffer is composed -> what came down, as `transfers` entries."""
        moved = []
        if self.mode == 'resident':
            for k, f in enumerate(self.features):
                f['mc'], f['ap'], f['wave'] = download(k)
                f['voiced'] = f['f0'] != 0
                moved += [('down', 'mc', f['mc'].size), ('down', 'ap', f['ap'].size), ('down', 'wave', f['wave'].size)]
        self.mode = 'composed'
        return moved

    def push_composed(self, pipe, vocoder, wave, track):
        """One buffer over the separate calls, the plans applied to host arrays: `pipe` encodes (`Pipeline._composed_extract`), `vocoder` holds
        the stream's synthesizer -> the samples that are final."""
        from yukarin import Wave
        from yukarin.acoustic_feature import AcousticFeature
        calls['composed'] += 1
        pipe._reset_stream()
        # encode: the separate call on the window, then `pick(pad, -pad)`; the plans follow the frames it really returned
        f = pipe._composed_extract(wave, track)
        (ra, rb), (wa, wb), _, c_rows, c_samples, _, _, pad_c, (k0, k1), _, d_rows = self.plans(len(f.f0), len(wave.wave), int(wave.sampling_rate))
        self.features.append(dict(start=self.add[1], rows=rb - ra, samples=wb - wa, f0=numpy.asarray(f.f0)[ra:rb], mc=numpy.asarray(f.mc)[ra:rb],
                                  ap=numpy.asarray(f.ap)[ra:rb], voiced=numpy.asarray(f.voiced)[ra:rb], wave=numpy.asarray(wave.wave)[wa:wb]))
        # convert: the window by the plan (`FeatureWrapperSegmentMethod`: float32 pads, keys f0 / ap / mc / voiced and the wave)
        fs_ = self.features
        g = AcousticFeature(f0=self.concat(c_rows, [s['f0'] for s in fs_], (1,), numpy.float32),
                            ap=self.concat(c_rows, [s['ap'] for s in fs_], (fs_[-1]['ap'].shape[1],), numpy.float32),
                            mc=self.concat(c_rows, [s['mc'] for s in fs_], (fs_[-1]['mc'].shape[1],), numpy.float32),
                            voiced=self.concat(c_rows, [s['voiced'] for s in fs_], (1,), bool))
        g.wave = Wave(self.concat(c_samples, [s['wave'] for s in fs_], (), numpy.float32), wave.sampling_rate)
        out = self.voice_changer.convert_from_acoustic_feature(g, (pad_c, pad_c))
        self.outputs.append(dict(start=self.add[2], rows=k1 - k0, f0=numpy.asarray(out.f0)[k0:k1], sp=numpy.asarray(out.sp)[k0:k1],
                                 ap=numpy.asarray(out.ap)[k0:k1]))
        # decode: the window by the plan (`FeatureSegmentMethod`: `AcousticFeature.silent` pads), to the synthesis stream
        held = [o for o in self.outputs]
        if any(i >= 0 and b > a and 'sp' not in held[i] for i, a, b in d_rows):
            raise RuntimeError('the decode window reaches rows that were synthesized on the card and not kept')
        if self.streams.span_count(d_rows) == 0:
            return numpy.empty(0, numpy.float64)
        last = held[-1]
        h = AcousticFeature(f0=self.concat(d_rows, [o.get('f0') for o in held], (1,), numpy.float32),
                            sp=self.concat(d_rows, [o.get('sp') for o in held], (last['sp'].shape[1],), numpy.float32),
                            ap=self.concat(d_rows, [o.get('ap') for o in held], (last['ap'].shape[1],), numpy.float32))
        return world_synth.decode_realtime(vocoder, h).wave

    def move_on(self) -> int:
        """The clocks move on and what no later window can fetch goes, on both paths -> how many of the oldest feature segments went (the
        store gives their room back)."""
        S, T = self.streams, self.time_length
        _, rate_c, rate_d = self.rates()
        self.add[1] += T
        self.add[2] += T
        self.now[1] += T
        self.now[2] += T
        gone = S.retire([(f['start'], f['rows']) for f in self.features], self.now[1], T, self.extra[1], rate_c)
        del self.features[:gone]
        del self.outputs[:S.retire([(o['start'], o['rows']) for o in self.outputs], self.now[2], T, self.extra[2], rate_d)]
        return gone


class _WindowOwner(object):
    """The device blocks a fetched convert window lies in -- mc (rows, m_in), ap (rows, 513), wave (samples,), those of `_window_arrays` --
    grown, never shrunk, freed in the process that made them."""
    _window_arrays = ('mc', 'ap', 'wave')

    def __init__(self):
        self._win, self._win_cap = {}, (0, 0)

    def _window_blocks(self, ctx, rows: int, samples: int, m_in: int):
        if self._win.get('ctx') is not ctx or self._win.get('pid') != os.getpid():
            self._win, self._win_cap = {'ctx': ctx, 'pid': os.getpid()}, (0, 0)
        if rows > self._win_cap[0] or samples > self._win_cap[1] or self._win.get('m_in') != m_in:
            self._free_window()
            cap = (max(rows + rows // 2, 64), max(samples + samples // 2, 4096))
            sizes = dict(mc=cap[0] * m_in, ap=cap[0] * BINS, wave=cap[1])
            self._win.update(ctx=ctx, pid=os.getpid(), m_in=m_in, **{k: ctx.dev_alloc(sizes[k]) for k in self._window_arrays})
            self._win_cap = cap
        return self._win

    def _free_window(self) -> None:
        w = self._win
        if w.get('pid') == os.getpid() and w.get('ctx') is not None and w['ctx'].handle is not None:
            for k in self._window_arrays:
                if k in w:
                    w['ctx'].dev_free(w.pop(k))
        self._win_cap = (0, 0)


def _ring_sizes(time_length, convert_extra_time, ring_rows, ring_samples, seg_rows: int, seg_samples: int):
    """The capacity of a stream's rings: the caller's, or what the retire rule keeps live, with a segment to spare."""
    live = int((2 * convert_extra_time + 2 * time_length) / time_length) + 3
    return (ring_rows if ring_rows is not None else live * (seg_rows + 2)), (ring_samples if ring_samples is not None else live * (seg_samples + 2))


class LivePipeline(_WindowOwner):
    """The reference's three-stream live loop (run.py: `EncodeStream` -> `ConvertStream` -> `DecodeStream`, each with its own margin) as one
    object: `push(buffer)` does for item k what the three workers do -- every `add` at `extra_time + k * time_length`, every window from
    `k * time_length`, the clocks accumulated as theirs are -- and returns the samples that are final.  Each buffer goes through the encode
    stage ONCE; its rows [pad, n - pad) and their wave slice are kept as a segment, and a convert window is FETCHED from the kept segments by
    the plan `BaseStream.fetch` follows (`streams.fetch_plan`), silent pads included, instead of being re-encoded from audio.

    Resident path: the encode window (assembled on the host from the kept input buffers: it arrives from the host anyway) goes up once
    (`CrepeModel.track(..., device=True)`, or `Analyzer.upload_waves` + `ingest_tracks` in WORLD mode), `Analyzer.extract_resident` leaves its
    rows on the card, `RowStore.append` takes the segment from there, `RowStore.fetch` writes the convert window's mc / ap rows and wave into
    blocks of this object's, `VcCore.enqueue_wave_device` reads them with the discard hint (pad, pad), `ry_mask_rows` is the combine_silent of
    ap, and the rows [pad, n - pad) go to the synthesis stream as in `Pipeline.push`.  f0 stays on the host per segment, is concatenated by the
    same plan and goes through the F0Converter with the numpy operations of the separate calls.  No mc / sp / ap row crosses the bus
    (`transfers` lists what did, call by call).  The resident path asks that the decode plan hands on exactly the rows just converted -- with
    `decode_extra_time = 0` it does -- and that `Pipeline`'s conditions hold (`_resident_handles`).

    Composed path, otherwise: the same plans applied to host arrays over the separate calls -- `encode.extract` / `world_analysis.extract`,
    `convert_from_acoustic_feature`, `decode_realtime` -- with the bits of the resident path where both apply.  A signal that has taken it once
    stays on it until `flush` (its segments are then on the host; those of earlier resident buffers are brought down once).  `calls` counts
    which way a call went.  Retired segments (`streams.retire`) are dropped after every push on both paths.

    One stream (B streams in one chain: `LivePipelineBank`); `gate_first` and `advance` are `Pipeline` / `PipelineBank` matters: with
    `encode_extra_time = 0` no audio is encoded twice, so there is no overlap for them to save.  INTEGRATION.md section 23, DESIGN.md section 25."""

    def __init__(self, voice_changer, acoustic_param, time_length: float, encode_extra_time: float, convert_extra_time: float, decode_extra_time: float,
                 f0_mode: str = 'crepe', f0_fn=None, crepe_capacity='full', seed: Optional[int] = None, feature_class=None,
                 ring_rows: Optional[int] = None, ring_samples: Optional[int] = None, resident: bool = True):
        """ring_rows / ring_samples: the capacity of the store's rings (None: what the retire rule keeps live, with a segment to spare).
        resident=False: every call takes the composed path -- the yardstick of the tests and of scripts/live_pipeline_bench.py."""
        from . import streams
        self._streams = streams
        self._pipe = Pipeline(voice_changer, acoustic_param, crepe_capacity=crepe_capacity, seed=seed, feature_class=feature_class, f0_mode=f0_mode, f0_fn=f0_fn)
        self.voice_changer, self.acoustic_param, self.f0_mode, self.synth = voice_changer, acoustic_param, f0_mode, self._pipe.synth
        self.time_length = time_length
        self.extra = (encode_extra_time, convert_extra_time, decode_extra_time)
        self.calls, self.routes = calls, routes
        self.transfers = []                                                # of the last call: (direction, what, elements)
        self.ring_rows, self.ring_samples, self.resident = ring_rows, ring_samples, bool(resident)
        self._store = None
        self._state = _LiveState(voice_changer, acoustic_param, f0_mode, time_length, self.extra)
        _WindowOwner.__init__(self)

    def _start(self) -> None:
        self._state.start()
        if self._store is not None:
            self._store.reset()

    def _store_of(self, ctx, m_in: int, seg_rows: int, seg_samples: int):
        if self._store is None or self._store._given_ctx is not ctx or self._store.mc_cols != m_in:
            if self._store is not None:
                self._store.close()
            rows, samples = _ring_sizes(self.time_length, self.extra[1], self.ring_rows, self.ring_samples, seg_rows, seg_samples)
            self._store = self._streams.RowStore(m_in, BINS, rows, samples, ctx=ctx)
        return self._store

    def close(self) -> None:
        """Frees the store, the window blocks and the synthesizer in the process that created them; the voice changer and the shared handles stay."""
        if self._store is not None:
            self._store.close()
            self._store = None
        self._free_window()
        self._pipe.close()

    def _demote(self) -> None:
        """The signal leaves the resident path: its live segments come down once, and every later buffer is composed."""
        store = self._store
        self.transfers += self._state.demote(lambda k: store.download(store.segments[k]))
        if store is not None:
            store.reset()

    def push(self, buffer, out_gate=None):
        """One buffer of `time_length` seconds at the input rate (a float32 array, or a `yukarin.Wave`) -> the `Wave` of the samples that are
        final; with `out_gate` the chunk the gate emits, as `Pipeline.push` returns it."""
        from yukarin import Wave
        s, p, vc = self._state, self.acoustic_param, self.voice_changer
        self.transfers = []
        # ---- the three plans, from clocks and lengths alone: which way the call goes is known before anything runs
        wave = s.take(buffer)
        fs = int(wave.sampling_rate)
        n_enc = s.frames(wave.wave.size, fs)
        plans = s.plans(n_enc, wave.wave.size, fs)
        handles = None
        if self.resident and s.fits_resident(plans):
            handles = self._pipe._resident_handles(wave)
        track = None
        if handles is not None and self.f0_mode == 'world':
            track = _world_f0(self._pipe.f0_fn, wave, p)
            if not _track_fits(track[0], track[1], n_enc, p.frame_period):
                handles = None                                             # the callable's track does not fit: the composed path, with that track
        if handles is None:
            self._demote()
            out = s.push_composed(self._pipe, self._pipe._vocoder, wave, track)
        else:
            s.mode = 'resident'
            out = self._push_resident(handles, wave, track, n_enc, plans, out_gate)
        gone = s.move_on()
        if s.mode == 'resident':
            self._store.retire(gone)
        if isinstance(out, Wave):
            return out                                                     # the gate read the samples on the card
        if out_gate is not None:
            out = _through_host_gate(out_gate, out)
        return Wave(wave=out, sampling_rate=vc.output_sampling_rate)

    def _push_resident(self, handles, wave, track, n_enc, plans, out_gate):
        from yukarin import Wave
        model, analyzer, core, (p_eff, p_all), hop, gate_fft = handles
        p, ac, s = self.acoustic_param, self.voice_changer.acoustic_converter, self._state
        (ra, rb), (wa, wb), c_plan, _, _, n_c, n_w, pad_c, (k0, k1), _, _ = plans
        fs = int(wave.sampling_rate)
        calls['resident'] += 1
        x = numpy.ascontiguousarray(wave.wave, dtype=numpy.float32)
        # encode: the window goes up once; its rows stay on the card
        if self.f0_mode == 'world':
            trk = analyzer.ingest_tracks([track[0]], p.frame_period, analyzer.upload_waves([x]))
            self.transfers += [('up', 'wave', x.size), ('up', 'f0', track[0].size)]
            f0_track = track[0]
        else:
            trk = model.track(x, fs, _crepe.hop_length(p.frame_period), p.frame_period, threshold=encode.threshold, device=True)
            self.transfers.append(('up', 'wave', x.size))
        if trk.frames != n_enc:
            raise RuntimeError('the tracker returned %d frames, the frame-count rule says %d' % (trk.frames, n_enc))
        ctx = core.stage1.ctx
        b = self._pipe._reserve(ctx, max(n_enc, n_c), p.order + 1, core.M, core.F)
        analyzer.extract_resident(trk.wave, trk.samples, trk.f0, trk.t, n_enc, b['mc32'], b['sp32'], b['ap32'])
        if self.f0_mode != 'world':
            f0_track = trk.download()[1]
            self.transfers.append(('down', 'track', n_enc))
        store = self._store_of(ctx, p.order + 1, rb - ra, wb - wa)
        store.append(s.add[1], b['mc32'], b['ap32'], ra, rb - ra, trk.wave, wa, wb - wa)
        s.add_resident(f0_track, plans)
        # convert: the window is fetched from the rows on the card
        w = self._window_blocks(ctx, n_c, n_w, p.order + 1)
        store.fetch(c_plan, ac.config.dataset.acoustic_param.frame_period, fs, w['mc'], w['ap'], w['wave'], n_c, n_w)
        self.transfers.append(('up', 'table', store.counts()['upload_bytes'] // 4))
        _apply_discard(core, (pad_c, pad_c))
        effective, _ = core.enqueue_wave_device(w['wave'], n_w, hop, gate_fft, p_eff, p_all, w['mc'], n_c, b['mc_out'], b['sp_out'], b['mask'], SP_FLOOR)
        self.transfers.append(('down', 'mask', n_c))
        # decode: the plan hands on exactly the rows just converted
        f0 = s.resident_f0(plans, effective)
        ctx.mask_rows(w['ap'], b['mask'], n_c, BINS, k0, k1)
        dev_rows = [world_synth.DeviceRows(base + k0 * BINS * 4, k1 - k0) for base in (b['sp_out'], w['ap'])]
        self.transfers.append(('up', 'f0', k1 - k0))
        if _gate_on_card(out_gate, ctx):
            block = self._pipe._sample_block(self.synth.bound(k1 - k0, False))
            got = self.synth.push_device(f0, dev_rows[0], dev_rows[1], block, 0)
            routes['gate_device'] += 1
            out = out_gate.push_device(block.address, got)
            if out is not None:
                self.transfers.append(('down', 'samples', out.size))
            return Wave(wave=out if out is not None else numpy.empty(0, out_gate.dtype), sampling_rate=self.voice_changer.output_sampling_rate)
        out = self.synth.push(f0, dev_rows[0], dev_rows[1])
        self.transfers.append(('down', 'samples', out.size))
        return out

    def flush(self):
        """Ends the signal: the samples `push` still held back; the next `push` starts a new signal with the clocks at their first values."""
        from yukarin import Wave
        self._pipe._reset_stream()
        self._start()
        return Wave(wave=self.synth.flush(), sampling_rate=self.voice_changer.output_sampling_rate)


class LivePipelineBank(_BlockOwner, _WindowOwner):
    """`LivePipeline` for the B live streams one process serves, with ONE resident chain per call instead of B: the encode windows are assembled
    on the host per stream, then `CrepeModel.track_many` (one upload of all windows; WORLD mode: `Analyzer.upload_waves` + one `ingest_tracks`) ->
    `Analyzer.extract_many_resident` (one verdict) -> `RowBank.append_many` (one launch) -> `RowBank.fetch_many` (every stream's convert window, one
    upload and one launch) -> `VcCore.enqueue_waves_device` with the discard hint (pad, pad) (one gate, one wait) -> `ry_gather_rows` of sp ->
    `RowBank.pick_ap` with the gate's mask (the full ap window is written nowhere) -> ONE `StreamBank.push`, or `push_device` and ONE
    `OutputGateBank.push_device`.  f0 stays on the host per segment, as in `LivePipeline`.

    Every stream has its own `_LiveState` -- clocks, input, feature and output lists: a stream that sits a call out or is flushed does not
    move the others' clocks.  Which path a stream takes is decided per stream by `LivePipeline`'s rule (the decode plan is an identity,
    `Pipeline`'s resident conditions hold, in WORLD mode the track fits), and the resident streams of a call share one rate.  A stream that
    is not eligible is demoted alone: its live segments come down once and it runs the composed path through its slot of the same
    `StreamBank` until its `flush`; the others stay in the chain.  `calls` counts per stream and call.

    What stream b returns, call by call, has the bits a lone `LivePipeline(seed=seeds[b])` returns for the same buffers and flushes, whatever
    the other streams do.  `gate_first` and `advance` stay out, for `LivePipeline`'s reason.  INTEGRATION.md section 24, DESIGN.md section 26."""
    _more_widths = PipelineBank._more_widths
    _window_arrays = ('mc', 'wave')                                        # ap is read from the rings by `pick_ap`

    def __init__(self, voice_changer, acoustic_param, n_streams: int, time_length: float, encode_extra_time: float, convert_extra_time: float,
                 decode_extra_time: float, seeds=None, f0_mode: str = 'crepe', f0_fn=None, crepe_capacity='full', feature_class=None,
                 ring_rows: Optional[int] = None, ring_samples: Optional[int] = None, resident: bool = True):
        """seeds: one per stream (None: every stream has RY_SYNTH_SEED); ring_rows / ring_samples: the capacity of EACH stream's rings;
        resident=False: every stream is composed."""
        from . import streams
        self._streams = streams
        self.n_streams = int(n_streams)
        if self.n_streams < 1:
            raise ValueError('a bank has at least one stream, got %d' % self.n_streams)
        if seeds is None:
            seeds = [int(os.environ.get('RY_SYNTH_SEED', '0'))] * self.n_streams
        self.seeds = [int(s) for s in seeds]
        if len(self.seeds) != self.n_streams:
            raise ValueError('%d seeds for %d streams' % (len(self.seeds), self.n_streams))
        if f0_mode not in ('crepe', 'world'):
            raise ValueError("f0_mode is 'crepe' or 'world', got %r" % (f0_mode,))
        self._pipe = Pipeline(voice_changer, acoustic_param, crepe_capacity=crepe_capacity, seed=self.seeds[0], feature_class=feature_class, f0_mode=f0_mode,
                              f0_fn=f0_fn)                                 # the conditions and handles of the resident path, the composed encode
        self.voice_changer, self.acoustic_param, self.f0_mode = voice_changer, acoustic_param, f0_mode
        self.time_length = time_length
        self.extra = (encode_extra_time, convert_extra_time, decode_extra_time)
        rate = voice_changer.output_sampling_rate
        self.bank = world_synth.StreamBank(rate, acoustic_param.frame_period, n_streams=self.n_streams, seeds=self.seeds, ctx=world_synth.engine_for_tests.ctx)
        self._vocoders = [_Vocoder(acoustic_param, rate, world_synth.BankSlot(self.bank, b)) for b in range(self.n_streams)]
        self._states = [_LiveState(voice_changer, acoustic_param, f0_mode, time_length, self.extra) for _ in range(self.n_streams)]
        self.calls, self.routes = calls, routes
        self.transfers = []                                                # of the last call: (direction, what, elements)
        self.ring_rows, self.ring_samples, self.resident = ring_rows, ring_samples, bool(resident)
        self._store = None
        _BlockOwner.__init__(self)
        _WindowOwner.__init__(self)

    def close(self) -> None:
        """Frees the row bank, the device blocks, the stream bank and the one-shot pipeline in the process that created them; the voice changer
        and the shared handles stay."""
        if self._store is not None:
            self._store.close()
            self._store = None
        self._free_window()
        self._free()
        self.bank.close()
        self._pipe.close()

    def _store_of(self, ctx, m_in: int, seg_rows: int, seg_samples: int):
        if self._store is None or self._store._given_ctx is not ctx or self._store.mc_cols != m_in:
            if any(s.mode == 'resident' for s in self._states):
                raise RuntimeError('the context of the resident chain changed under live streams')
            if self._store is not None:
                self._store.close()
            rows, samples = _ring_sizes(self.time_length, self.extra[1], self.ring_rows, self.ring_samples, seg_rows, seg_samples)
            self._store = self._streams.RowBank(self.n_streams, m_in, BINS, rows, samples, ctx=ctx)
        return self._store

    def _demote(self, b: int) -> None:
        """Stream b leaves the resident chain: its live segments come down once, and it is composed until its flush."""
        store = self._store
        self.transfers += self._states[b].demote(lambda k: store.download(b, store.segments[b][k]))
        if store is not None:
            store.reset(b)

    def _final(self, final):
        final = sorted(set(int(s) for s in (final or ())))
        if any(s < 0 or s >= self.n_streams for s in final):
            raise ValueError('final names stream %s of %d' % (final, self.n_streams))
        return final

    def _end(self, streams) -> None:
        """New signals for `streams`: their clocks at the first values, their rings empty."""
        for b in streams:
            self._states[b].start()
            if self._store is not None:
                self._store.reset(b)

    def push(self, buffers, out_gate=None, final=None) -> list:
        """One buffer of `time_length` seconds for every live stream: `buffers` has one entry per stream (a float32 array or a `yukarin.Wave`),
        None for a stream that sits the call out -> one `Wave` per stream: the samples that are final (empty for a stream that sat out).
        out_gate (an `output_gate.OutputGateBank` of n_streams streams): the samples of all streams go through it in ONE call, on the card when
        every stream of the call is resident and the gates judge there in the pipeline's context, else through the host: the same bits (`routes`
        counts which, once per call).  final: the streams whose signal ends with this call, as `PipelineBank.push` has it; the next buffer of
        such a stream starts a new signal."""
        from yukarin import Wave
        buffers = list(buffers)
        B = self.n_streams
        if len(buffers) != B:
            raise ValueError('%d buffers for %d streams' % (len(buffers), B))
        final = self._final(final)
        p, rate = self.acoustic_param, self.voice_changer.output_sampling_rate
        self.transfers = []
        part = [b for b in range(B) if buffers[b] is not None]
        # ---- per stream: the window, the plans and which way it goes, before anything runs
        waves, plans, n_encs, handles, tracks = {}, {}, {}, {}, {}
        for b in part:
            s = self._states[b]
            waves[b] = s.take(buffers[b])
            n, fs = waves[b].wave.size, int(waves[b].sampling_rate)
            n_encs[b] = s.frames(n, fs)
            plans[b] = s.plans(n_encs[b], n, fs)
            handles[b] = self._pipe._resident_handles(waves[b]) if self.resident and s.fits_resident(plans[b]) else None
            tracks[b] = None
            if handles[b] is not None and self.f0_mode == 'world':
                tracks[b] = _world_f0(self._pipe.f0_fn, waves[b], p)
                if not _track_fits(tracks[b][0], tracks[b][1], n_encs[b], p.frame_period):
                    handles[b] = None                                      # this stream's track does not fit: it alone is composed, with that track
        res = [b for b in part if handles[b] is not None]
        if res:
            self.bank._get()
            ctx = handles[res[0]][2].stage1.ctx
            if len(set(int(waves[b].sampling_rate) for b in res)) != 1 or self.bank._ctx is not ctx or self.bank.fft_size != FFT_SIZE:
                res = []                                                   # the chain reads one rate in one context
        outs = [numpy.empty(0, numpy.float64) for _ in range(B)]
        for b in part:
            if b not in res:
                self._demote(b)
                outs[b] = self._states[b].push_composed(self._pipe, self._vocoders[b], waves[b], tracks[b])
                self.transfers.append(('down', 'samples', outs[b].size))
        on_card = None
        rest = [b for b in final if b not in res]                          # composed or absent streams that end: what their slots still hold
        if res:                                                            # the gate reads on the card when every sample of the call is there
            on_card = self._push_resident(res, handles[res[0]], waves, tracks, n_encs, plans, out_gate if len(res) == len(part) and not rest else None,
                                          final, outs)
        if rest:
            got = self.bank.flush(rest)
            for b in rest:
                outs[b] = numpy.concatenate([outs[b], got[b]])
        for b in part:
            gone = self._states[b].move_on()
            if self._states[b].mode == 'resident':
                self._store.retire(b, gone)
        self._end(final)
        if on_card is not None:
            routes['gate_device'] += 1
            outs = [o if o is not None else numpy.empty(0, out_gate.dtype) for o in out_gate.push_device(on_card[0].address, on_card[1])]
        elif out_gate is not None:
            outs = _through_host_gate(out_gate, outs)
        return [Wave(wave=o, sampling_rate=rate) for o in outs]

    def _push_resident(self, res, handles, waves, tracks, n_encs, plans, out_gate, final, outs):
        """The one chain of the streams `res` (ascending).  The samples go into `outs`, or stay on the card for `out_gate` -> (block, offsets)."""
        model, analyzer, core, (p_eff, p_all), hop, gate_fft = handles
        p, ac, S = self.acoustic_param, self.voice_changer.acoustic_converter, self._streams
        fs = int(waves[res[0]].sampling_rate)
        calls['resident'] += len(res)
        xs = [numpy.ascontiguousarray(waves[b].wave, dtype=numpy.float32) for b in res]
        fo_e = S._offsets([n_encs[b] for b in res])
        # encode: the windows go up once; their rows stay on the card
        if self.f0_mode == 'world':
            trk = analyzer.ingest_tracks([tracks[b][0] for b in res], p.frame_period, analyzer.upload_waves(xs))
            self.transfers += [('up', 'wave', sum(x.size for x in xs)), ('up', 'f0', int(fo_e[-1]))]
            f0_tracks = [tracks[b][0] for b in res]
        else:
            trk = model.track_many(xs, fs, _crepe.hop_length(p.frame_period), p.frame_period, threshold=encode.threshold, device=True)
            self.transfers.append(('up', 'wave', sum(x.size for x in xs)))
        if list(trk.frame_offsets) != list(fo_e):
            raise RuntimeError('the tracker returned %s frames, the frame-count rule says %s' % (list(numpy.diff(trk.frame_offsets)), list(numpy.diff(fo_e))))
        ctx = core.stage1.ctx
        sizes = [(plans[b][5], plans[b][6]) for b in res]                  # rows and samples of every convert window
        fo_c, so_c = S._offsets([r for r, _ in sizes]), S._offsets([n for _, n in sizes], numpy.int64)
        blk = self._reserve(ctx, max(int(fo_e[-1]), int(fo_c[-1])), p.order + 1, core.M, core.F)
        analyzer.extract_many_resident(trk.wave, trk.sample_offsets, trk.f0, trk.t, fo_e, blk['mc32'], blk['sp32'], blk['ap32'])
        if self.f0_mode != 'world':
            f0_tracks = [track for _, track in trk.download()]
            self.transfers.append(('down', 'track', int(fo_e[-1])))
        (ra, rb), (wa, wb) = plans[res[0]][0], plans[res[0]][1]
        store = self._store_of(ctx, p.order + 1, rb - ra, wb - wa)
        store.append_many(res, [self._states[b].add[1] for b in res], (blk['mc32'], blk['ap32'], trk.wave),
                          [(int(fo_e[i]) + plans[b][0][0], plans[b][0][1] - plans[b][0][0]) for i, b in enumerate(res)],
                          [(int(trk.sample_offsets[i]) + plans[b][1][0], plans[b][1][1] - plans[b][1][0]) for i, b in enumerate(res)])
        self.transfers.append(('up', 'table', store.counts()['upload_bytes'] // 4))
        for b, f0_track in zip(res, f0_tracks):
            self._states[b].mode = 'resident'
            self._states[b].add_resident(f0_track, plans[b])
        # convert: every window is fetched from its stream's rows on the card, back to back
        w = self._window_blocks(ctx, int(fo_c[-1]), int(so_c[-1]), p.order + 1)
        c_plans = [plans[b][2] for b in res]
        if store.fetch_many(res, c_plans, ac.config.dataset.acoustic_param.frame_period, fs, w['mc'], w['wave']) != sizes:
            raise RuntimeError('the row bank fetched other windows than the plans say')
        self.transfers.append(('up', 'table', store.counts()['upload_bytes'] // 4))
        pad_c = plans[res[0]][7]
        _apply_discard(core, (pad_c, pad_c))
        effective, _ = core.enqueue_waves_device(w['wave'], so_c, fo_c, hop, gate_fft, p_eff, p_all, w['mc'], blk['mc_out'], blk['sp_out'], blk['mask'], SP_FLOOR)
        self.transfers.append(('down', 'mask', int(fo_c[-1])))
        # decode: every plan hands on exactly the rows just converted; sp is gathered and ap picked into packed rows, stream after stream
        keep = [plans[b][8] for b in res]
        picks = [(int(fo_c[i]) + k0, int(fo_c[i]) + k1) for i, (k0, k1) in enumerate(keep)]
        total = sum(k1 - k0 for k0, k1 in keep)
        key = (tuple(picks), blk['rows'])
        if self._table != key:                                             # live streams repeat their shapes: the table goes up once
            ctx.dev_upload(blk['rows'], numpy.concatenate([numpy.arange(k0, k1, dtype=numpy.int32) for k0, k1 in picks]))
            self._table = key
            self.transfers.append(('up', 'table', total))
        ctx.gather_rows(blk['sp_out'], int(fo_c[-1]), BINS, blk['rows'], blk['sp_pack'], total)
        store.pick_ap(res, c_plans, keep, blk['mask'], blk['ap_pack'])
        self.transfers.append(('up', 'table', store.counts()['upload_bytes'] // 4))
        items, at = [None] * self.n_streams, 0
        for i, b in enumerate(res):
            k0, k1 = keep[i]
            f0 = self._states[b].resident_f0(plans[b], effective[fo_c[i]:fo_c[i + 1]])
            items[b] = (numpy.ascontiguousarray(f0), world_synth.DeviceRows(blk['sp_pack'] + at * BINS * 4, k1 - k0),
                        world_synth.DeviceRows(blk['ap_pack'] + at * BINS * 4, k1 - k0))
            at += k1 - k0
        self.transfers.append(('up', 'f0', total))
        ends = [b for b in final if b in res]
        if _gate_on_card(out_gate, ctx):
            block = self._sample_block(sum(self.bank.bound(b, items[b][0].size, b in ends) for b in res))
            return block, self.bank.push_device(items, ends, block)
        got = self.bank.push(items, final=ends)
        for b in res:
            outs[b] = got[b]
        self.transfers.append(('down', 'samples', sum(got[b].size for b in res)))
        return None

    def flush(self, stream=None):
        """Ends the signal of `stream` -> its `Wave`: the samples `push` still held back; its next `push` starts a new signal with the clocks at
        their first values, and no other stream's clocks move.  stream=None: ends every stream -> one `Wave` per stream."""
        from yukarin import Wave
        rate = self.voice_changer.output_sampling_rate
        which = list(range(self.n_streams)) if stream is None else [int(stream)]
        self._pipe._reset_stream()
        outs = self.bank.flush(which)
        self._end(which)
        if stream is not None:
            return Wave(wave=outs[int(stream)], sampling_rate=rate)
        return [Wave(wave=o, sampling_rate=rate) for o in outs]
