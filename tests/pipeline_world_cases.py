"""Cases and bodies the emulator and the GPU tests of WORLD mode share (test_pipeline_world_cpu.py, test_pipeline_world_gpu.py): the track ingest of
the analysis unit (`ry_analysis_upload_waves`, `ry_analysis_ingest_tracks`, `ry_analysis_track_buffers`) against its numpy statement, and
`Pipeline(f0_mode='world')` / `PipelineBank(f0_mode='world')` against the composed chain run with the SAME f0 callable: `world_analysis.extract`
(D4C from the device) -> `VoiceChanger.convert_from_acoustic_feature` -> `world_synth.decode` / a `Synthesizer.push` sequence.  Every comparison is
bit equality (`pipeline_cases.same`).  The f0 callables are deterministic functions of the sample count alone; nothing here needs `pyworld`."""
import ctypes
import types

import numpy

import pipeline_cases as P
from realtime_yukarin_amd import _lib, pipeline, world_analysis, world_synth

UB, IP, LLP, DP, VP = (ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_double),
                       ctypes.c_void_p)
ESTATE, EINVAL = -4, -1
INGEST_FRAMES = (1, 2, 63, 64, 65, 255, 256, 257)         # either side of a wave of lanes and of a workgroup of 256 threads
RAGGED = (1, 37, 300)
PERIODS = (5.0, 5.5)                                     # 5.5: k * 5.5 / 1000 is not exact, the two roundings show


# ---- the f0 callables -----------------------------------------------------------------------------------------------------------------
def f0_track(n_samples: int, fs, frame_period=P.FRAME_PERIOD):
    """A fixed-seed piecewise track for a wave of n_samples: Harvest's frame count, voiced runs (a slow glide between 110 and 380 Hz with a little
    jitter) and unvoiced runs (exact zeros) of 2 .. 9 frames, the first run voiced; computed from the sample count alone -> (f0, t)."""
    n = world_analysis.harvest_frames(n_samples, fs, frame_period)
    rng = numpy.random.default_rng([int(n_samples), 7])
    f0 = numpy.zeros(n, numpy.float64)
    k, voiced = 0, True
    while k < n:
        run = int(rng.integers(2, 10))
        if voiced:
            a, b = rng.uniform(110.0, 380.0, 2)
            f0[k:k + run] = (numpy.linspace(a, b, run) + rng.normal(0, 1.5, run))[:n - k]
        k, voiced = k + run, not voiced
    return f0, world_analysis.frame_times(n, frame_period)


def f0_fn(x, fs, frame_period, f0_floor, f0_ceil):
    assert x.dtype == numpy.float64 and x.ndim == 1                  # what `AcousticFeature.extract` hands `extract_f0`
    return f0_track(x.size, fs, frame_period)


def unvoiced_fn(x, fs, frame_period, f0_floor, f0_ceil):
    f0, t = f0_track(x.size, fs, frame_period)
    return numpy.zeros_like(f0), t


def nan_fn(x, fs, frame_period, f0_floor, f0_ceil):
    f0, t = f0_track(x.size, fs, frame_period)
    f0[f0.size // 2] = numpy.nan
    return f0, t


def nyquist_fn(x, fs, frame_period, f0_floor, f0_ceil):
    f0, t = f0_track(x.size, fs, frame_period)
    f0[f0.size // 3] = fs / 2
    return f0, t


def wrong_count_fn(x, fs, frame_period, f0_floor, f0_ceil):
    """One frame more than Harvest's rule."""
    f0, _ = f0_track(x.size, fs, frame_period)
    f0 = numpy.concatenate([f0, f0[-1:]])
    return f0, world_analysis.frame_times(f0.size, frame_period)


def shifted_t_fn(x, fs, frame_period, f0_floor, f0_ceil):
    """The right count, frame centres half a period late."""
    f0, t = f0_track(x.size, fs, frame_period)
    return f0, t + frame_period / 2000.0


class Counting(object):
    """An f0 callable that records the sample count of every call."""

    def __init__(self, fn=f0_fn):
        self.fn, self.sizes = fn, []

    def __call__(self, x, fs, frame_period, f0_floor, f0_ceil):
        self.sizes.append(int(x.size))
        return self.fn(x, fs, frame_period, f0_floor, f0_ceil)


# ---- the process and the chain --------------------------------------------------------------------------------------------------------
def set_up(monkeypatch):
    """A WORLD-mode process: no CREPE weights anywhere (RY_CREPE_MODEL unset, nothing loaded in the shim), D4C from the device, fresh counters."""
    from realtime_yukarin_amd.compat import crepe as shim
    monkeypatch.setattr(shim, '_weights', {})
    monkeypatch.setattr(shim, '_models', {})
    for name in ('RY_CREPE_MODEL', 'RY_DEVICE_GATE', 'RY_DISCARD_HINT'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(world_analysis, 'aperiodicity', world_analysis.device_aperiodicity)
    monkeypatch.setattr(pipeline, 'calls', {'resident': 0, 'composed': 0})
    monkeypatch.setattr(pipeline, 'calls_many', {'resident': 0, 'composed': 0})
    return shim


def feature_class(fn):
    """yukarin's container with `extract_f0` = fn: what the composed chain extracts with."""
    from yukarin.acoustic_feature import AcousticFeature
    return type('ChainFeature', (AcousticFeature,), {'extract_f0': classmethod(
        lambda cls, x, fs, frame_period, f0_floor, f0_ceil: fn(x, fs, frame_period, f0_floor, f0_ceil))})


def chain_feature(vc, param, fn, wave, discard=(0, 0)):
    f = world_analysis.extract(feature_class(fn), wave, **P.encode_args(param))
    f.wave = wave
    return vc.convert_from_acoustic_feature(f, discard)


def chain(vc, param, fn, wave, synth):
    """The composed chain -> float64 samples (`world_synth.decode` over `synth`)."""
    vocoder = types.SimpleNamespace(out_sampling_rate=vc.output_sampling_rate, acoustic_param=param, _ry_synth=synth)
    return world_synth.decode(vocoder, chain_feature(vc, param, fn, wave)).wave


def chain_push(vc, param, fn, wave, synth, discard):
    """One buffer of the live chain: extract, convert with the discard hint, pick [front, frames - back), push."""
    out = chain_feature(vc, param, fn, wave, discard)
    k0, k1 = discard[0], len(out.f0) - discard[1]
    if k1 <= k0:
        return numpy.empty(0, numpy.float64)
    return synth.push(numpy.asarray(out.f0).ravel()[k0:k1], out.sp[k0:k1], out.ap[k0:k1])


def param_of(vc):
    return vc.acoustic_converter.config.dataset.acoustic_param


def pipe_of(vc, fn=f0_fn, seed=3, **kw):
    return pipeline.Pipeline(vc, param_of(vc), seed=seed, f0_mode='world', f0_fn=fn, **kw)


def hop_of(fs) -> int:
    return fs * P.FRAME_PERIOD // 1000


def samples_for(frames: int, fs) -> int:
    """A sample count in the middle of the range that gives `frames` frames."""
    n = (frames - 1) * hop_of(fs) + hop_of(fs) // 2
    assert world_analysis.harvest_frames(n, fs, P.FRAME_PERIOD) == frames
    return n


def voiced_wave(n: int, fs, seed: int = 0) -> numpy.ndarray:
    """float32, n samples: `pipeline_cases.wave_of('loud')` cut to n -- every frame above the gate's threshold."""
    return P.wave_of('loud', fs, (n + 1) / fs, seed)[:n].copy()


def half_quiet_wave(n: int, fs, seed: int = 0) -> numpy.ndarray:
    """A loud half and a half far below the gate's threshold: the frames split into effective and silent ones."""
    x = voiced_wave(n, fs, seed)
    x[n // 2:] *= numpy.float32(1e-5)
    return x


# ---- 1. the ingest alone --------------------------------------------------------------------------------------------------------------
def statement(f0, period):
    """numpy's statement of what the kernel writes for one track."""
    f0 = numpy.asarray(f0, numpy.float64)
    return f0 != 0, f0.copy(), numpy.arange(f0.size, dtype=numpy.float64) * period / 1000.0


def track_of(n: int, seed: int) -> numpy.ndarray:
    """n frames with zeros, a negative zero, a denormal, a NaN and an infinity among ordinary values: the ingest copies and tests `!= 0`, no more."""
    rng = numpy.random.default_rng([n, seed])
    f0 = rng.uniform(60.0, 900.0, n)
    f0[rng.uniform(size=n) < 0.3] = 0.0
    special = [-0.0, 5e-324, numpy.nan, numpy.inf, -numpy.inf, 12000.0]
    for i, v in zip(rng.permutation(n)[:len(special)], special):
        f0[i] = v
    return f0


def _assert_tracks(trk, tracks, period):
    got = trk.download(t=True)
    assert len(got) == len(tracks)
    for (voiced, f0, t), want in zip(got, tracks):
        w_voiced, w_f0, w_t = statement(want, period)
        assert numpy.array_equal(voiced, w_voiced) and P.same(f0, w_f0) and P.same(t, w_t)
    return got


def buffers(analyzer):
    """`ry_analysis_track_buffers` -> (return code, dict of what it reported)."""
    lib, h = analyzer._get()
    p = [VP() for _ in range(4)]
    nw, nt, so, fo = ctypes.c_int(-7), ctypes.c_int(-7), LLP(), IP()
    rc = lib.dll.ry_analysis_track_buffers(h, ctypes.byref(p[0]), ctypes.byref(nw), ctypes.byref(so), ctypes.byref(nt), ctypes.byref(fo),
                                           *[ctypes.byref(q) for q in p[1:]])
    if rc != 0:
        return rc, None
    return rc, dict(wave=p[0].value, voiced=p[1].value, f0=p[2].value, t=p[3].value, n_waves=nw.value, n_tracks=nt.value,
                    sample_offsets=[so[i] for i in range(nw.value + 1)] if nw.value else None, frame_offsets=[fo[i] for i in range(nt.value + 1)])


def _waves_for(counts):
    rng = numpy.random.default_rng(len(counts))
    return [rng.normal(size=3 + 2 * i).astype(numpy.float32) for i in range(len(counts))]


def check_ingest_sizes(ctx, period):
    """Every size alone and the ragged call: t_64, voiced and f0_64 equal the numpy statement; each wave of the ragged call equals its lone call;
    the uploaded waves come back as they went up."""
    a = world_analysis.Analyzer(16000, order=P.ORDER, seed=5, ctx=ctx)
    lone = {}
    for n in INGEST_FRAMES + RAGGED:
        f0 = track_of(n, 1)
        up = a.upload_waves(_waves_for([n]))
        trk = a.ingest_tracks([f0], period, up)
        assert trk.frames == n and list(trk.frame_offsets) == [0, n] and trk.samples == 3
        lone[n] = _assert_tracks(trk, [f0], period)[0]
    waves = _waves_for(RAGGED)
    up = a.upload_waves(waves)
    got = numpy.empty(up.samples, numpy.float32)
    ctx.dev_download(up.wave, got)
    assert P.same(got, numpy.concatenate(waves)) and list(up.offsets) == [0, 3, 8, 15]
    tracks = [track_of(n, 1) for n in RAGGED]
    trk = a.ingest_tracks(tracks, period, up)
    assert list(trk.frame_offsets) == [0, 1, 38, 338] and list(trk.sample_offsets) == [0, 3, 8, 15]
    for (voiced, f0, t), n in zip(_assert_tracks(trk, tracks, period), RAGGED):
        assert numpy.array_equal(voiced, lone[n][0]) and P.same(f0, lone[n][1]) and P.same(t, lone[n][2])
    rc, rep = buffers(a)
    assert rc == 0 and rep['n_waves'] == 3 and rep['n_tracks'] == 3 and rep['sample_offsets'] == [0, 3, 8, 15] and rep['frame_offsets'] == [0, 1, 38, 338]
    assert (rep['wave'], rep['voiced'], rep['f0'], rep['t']) == (trk.wave, trk.voiced, trk.f0, trk.t)
    # a subset of the uploaded waves, as the gate-first form ingests it: the tracks back to back, the waves named by the table
    sub = a.ingest_tracks([tracks[0], tracks[2]], period, up, which=[0, 2])
    assert list(sub.frame_offsets) == [0, 1, 301] and list(sub.first_sample) == [0, 8] and list(sub.n_samples) == [3, 7] and sub.sample_offsets is None
    for (voiced, f0, t), n in zip(_assert_tracks(sub, [tracks[0], tracks[2]], period), (1, 300)):
        assert numpy.array_equal(voiced, lone[n][0]) and P.same(f0, lone[n][1]) and P.same(t, lone[n][2])
    a.close()


def check_ingest_poison(ctx):
    """After the poison hook no track is reported and the clean call's bits come back; a 3-frame call after a 300-frame call leaves the rows behind it
    poisoned; the buffers grow across calls."""
    a = world_analysis.Analyzer(24000, order=P.ORDER, seed=5, ctx=ctx)
    assert buffers(a)[0] == ESTATE                                       # before the first ingest
    big, small = track_of(300, 2), track_of(3, 3)
    up = a.upload_waves(_waves_for([300]))
    clean = _assert_tracks(a.ingest_tracks([big], 5.0, up), [big], 5.0)[0]
    a.poison()
    assert buffers(a)[0] == ESTATE
    up = a.upload_waves(_waves_for([300]))
    again = _assert_tracks(a.ingest_tracks([big], 5.0, up), [big], 5.0)[0]
    assert all(P.same(g, w) for g, w in zip(again, clean))
    a.poison()
    up = a.upload_waves(_waves_for([3]))
    trk = a.ingest_tracks([small], 5.0, up)
    _assert_tracks(trk, [small], 5.0)
    f0, t, voiced = numpy.empty(300, numpy.float64), numpy.empty(300, numpy.float64), numpy.empty(75, numpy.float32)
    ctx.dev_download(trk.f0, f0.view(numpy.float32))
    ctx.dev_download(trk.t, t.view(numpy.float32))
    ctx.dev_download(trk.voiced, voiced)
    ones = numpy.uint64(0xffffffffffffffff)
    assert (P.bits(f0)[3:] == ones).all() and (P.bits(t)[3:] == ones).all() and (voiced.view(numpy.uint8)[3:] == 0xff).all()
    # growth: a longer call than any before it on this handle
    long = track_of(1500, 4)
    _assert_tracks(a.ingest_tracks([long, small], 5.5, a.upload_waves(_waves_for([1, 2]))), [long, small], 5.5)
    a.close()


def check_ingest_refusals(ctx):
    """Every refusal is made before anything is uploaded or changed: `ry_analysis_track_buffers` keeps reporting RY_ESTATE on a handle without a
    track, and the PREVIOUS track -- its tables and its bits -- on a handle that has one."""
    a = world_analysis.Analyzer(16000, order=P.ORDER, seed=5, ctx=ctx)
    lib, h = a._get()
    dll = lib.dll
    f0 = numpy.ascontiguousarray(track_of(8, 5))
    x = numpy.arange(8, dtype=numpy.float32)
    ip = lambda *v: numpy.asarray(v, numpy.int32).ctypes.data_as(IP)
    out = VP()
    fp, dp = _lib._fptr(x), f0.ctypes.data_as(DP)
    null_f, null_d, null_i = _lib._fptr(None), ctypes.cast(VP(0), DP), ctypes.cast(VP(0), IP)
    uploads = [(EINVAL, (h, null_f, ip(8), 1, ctypes.byref(out))), (EINVAL, (h, fp, null_i, 1, ctypes.byref(out))), (EINVAL, (h, fp, ip(8), 1, None)),
               (EINVAL, (h, fp, ip(8), 0, ctypes.byref(out))), (EINVAL, (h, fp, ip(8), -1, ctypes.byref(out))), (EINVAL, (h, fp, ip(4, 0, 4), 3, ctypes.byref(out))),
               (EINVAL, (h, fp, ip(2147483647, 1), 2, ctypes.byref(out))), (ESTATE, (None, fp, ip(8), 1, ctypes.byref(out)))]
    ingests = [(EINVAL, (h, null_d, ip(8), 1, 5.0)), (EINVAL, (h, dp, null_i, 1, 5.0)), (EINVAL, (h, dp, ip(8), 0, 5.0)), (EINVAL, (h, dp, ip(8), -2, 5.0)),
               (EINVAL, (h, dp, ip(4, 0, 4), 3, 5.0)), (EINVAL, (h, dp, ip(1 << 22, 1), 2, 5.0)), (EINVAL, (h, dp, ip(8), 1, float('nan'))),
               (EINVAL, (h, dp, ip(8), 1, float('inf'))), (EINVAL, (h, dp, ip(8), 1, 0.0)), (EINVAL, (h, dp, ip(8), 1, -5.0)), (ESTATE, (None, dp, ip(8), 1, 5.0))]

    def refuse_all():
        for want, args in uploads:
            assert dll.ry_analysis_upload_waves(*args) == want, args[3:]
        for want, args in ingests:
            assert dll.ry_analysis_ingest_tracks(*args) == want, args[3:]
    assert buffers(a)[0] == ESTATE and dll.ry_analysis_track_buffers(None, *[None] * 8) == ESTATE
    refuse_all()
    assert buffers(a)[0] == ESTATE                                       # no track before, none after
    assert dll.ry_analysis_upload_waves(h, fp, ip(8), 1, ctypes.byref(out)) == 0 and buffers(a)[0] == ESTATE      # waves alone are no track
    up = a.upload_waves([x[:3], x[3:]])
    trk = a.ingest_tracks([f0[:3], f0[3:]], 5.5, up)
    before = buffers(a)
    refuse_all()
    assert buffers(a) == before and before[0] == 0 and before[1]['frame_offsets'] == [0, 3, 8] and before[1]['sample_offsets'] == [0, 3, 8]
    _assert_tracks(trk, [f0[:3], f0[3:]], 5.5)                           # the previous track, bit for bit
    got = numpy.empty(8, numpy.float32)
    ctx.dev_download(trk.wave, got)
    assert P.same(got, x)
    assert dll.ry_analysis_track_buffers(h, *[None] * 8) == 0            # every pointer may be null
    a.close()


def check_extract_takes_the_track_in_place(ctx, fs):
    """The existing device entries on what upload + ingest left: the rows of `extract_many_resident` equal `Analyzer.run` on the host arrays, cast to
    float32, wave by wave; a track with a NaN is refused by the extract's verdict, not by the ingest, and nothing is written."""
    a = world_analysis.Analyzer(fs, order=P.ORDER, seed=5, ctx=ctx)
    sizes = [samples_for(3, fs), samples_for(5, fs)]
    xs = [voiced_wave(n, fs, i) for i, n in enumerate(sizes)]
    tracks = [f0_track(n, fs)[0] for n in sizes]
    trk = a.ingest_tracks(tracks, P.FRAME_PERIOD, a.upload_waves(xs))
    n = trk.frames
    shapes = ((n, P.ORDER + 1), (n, P.BINS), (n, P.BINS))
    blocks = [ctx.dev_alloc(s[0] * s[1]) for s in shapes]
    for p, s in zip(blocks, shapes):
        ctx.dev_upload(p, numpy.full(s, numpy.nan, numpy.float32))
    a.extract_many_resident(trk.wave, trk.sample_offsets, trk.f0, trk.t, trk.frame_offsets, *blocks)
    want = [a.run(x.astype(numpy.float64), f, world_analysis.frame_times(f.size, P.FRAME_PERIOD), want=('mc', 'sp', 'ap')) for x, f in zip(xs, tracks)]
    for j, (p, s) in enumerate(zip(blocks, shapes)):
        got = numpy.empty(s, numpy.float32)
        ctx.dev_download(p, got)
        assert P.same(got, numpy.concatenate([w[j] for w in want]).astype(numpy.float32))
    bad = [tracks[0], tracks[1].copy()]
    bad[1][2] = numpy.nan
    trk = a.ingest_tracks(bad, P.FRAME_PERIOD, a.upload_waves(xs))         # the ingest takes it
    for p, s in zip(blocks, shapes):
        ctx.dev_upload(p, numpy.full(s, numpy.nan, numpy.float32))
    try:
        a.extract_many_resident(trk.wave, trk.sample_offsets, trk.f0, trk.t, trk.frame_offsets, *blocks)
    except _lib.Ry355Error as e:
        assert 'f0[5]' in str(e) and 'finite and below fs / 2' in str(e)
    else:
        raise AssertionError('a NaN in the track was not refused')
    for p, s in zip(blocks, shapes):
        got = numpy.zeros(s, numpy.float32)
        ctx.dev_download(p, got)
        assert numpy.isnan(got).all()
        ctx.dev_free(p)
    a.close()


# ---- 2. the pipeline ------------------------------------------------------------------------------------------------------------------
def check_convert_wave(vc, fs, x, fn, want, resident=True):
    """`convert_wave` twice (the blocks are reused) against the chain's samples `want`."""
    from yukarin import Wave
    pipe = pipe_of(vc, fn)
    before = dict(pipeline.calls)
    for _ in range(2):
        got = pipe.convert_wave(Wave(x, fs))
        assert got.sampling_rate == fs and P.same(got.wave, want)
    key, other = ('resident', 'composed') if resident else ('composed', 'resident')
    assert pipeline.calls[key] == before[key] + 2 and pipeline.calls[other] == before[other]
    pipe.close()


def check_push_flush(vc, fs, ctx, frames: int, discard, fn=f0_fn):
    """Three buffers of `frames` frames with a discard hint, then the flush, against the live chain with the same picks."""
    from yukarin import Wave
    pipe = pipe_of(vc, fn)
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3, ctx=ctx)
    n = samples_for(frames, fs)
    waves = [Wave(voiced_wave(n, fs, 0), fs), Wave(half_quiet_wave(n, fs, 1), fs), Wave(voiced_wave(n + 1, fs, 2), fs)]
    want = [chain_push(vc, param_of(vc), fn, w, ref, discard) for w in waves] + [ref.flush()]
    before = pipeline.calls['resident']
    got = [pipe.push(w, discard=discard, advance=None if i == 0 else 7).wave for i, w in enumerate(waves)] + [pipe.flush().wave]     # advance is ignored
    assert pipeline.calls['resident'] == before + 3
    assert all(P.same(g, w) for g, w in zip(got, want)) and sum(len(w) for w in want) > 0
    vc._fused_core().set_discard(0, 0)
    pipe.close()
    ref.close()


def check_refused_tracks(vc, fs, ctx, frames: int):
    """A NaN and an f0 at fs / 2: the pipeline refuses in the chain's words, and its blocks still return the next good call's bits."""
    import pytest
    from yukarin import Wave
    x = voiced_wave(samples_for(frames, fs), fs)
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3, ctx=ctx)
    good = chain(vc, param_of(vc), f0_fn, Wave(x, fs), ref)
    for bad in (nan_fn, nyquist_fn):
        with pytest.raises(_lib.Ry355Error) as want:
            chain(vc, param_of(vc), bad, Wave(x, fs), ref)
        switch = types.SimpleNamespace(fn=f0_fn)
        pipe = pipe_of(vc, lambda *a: switch.fn(*a))
        assert P.same(pipe.convert_wave(Wave(x, fs)).wave, good)           # the blocks exist
        switch.fn = bad
        with pytest.raises(_lib.Ry355Error) as got:
            pipe.convert_wave(Wave(x, fs))
        assert str(got.value) == str(want.value) and 'finite and below fs / 2' in str(got.value)
        with pytest.raises(_lib.Ry355Error) as got:
            pipe.push(Wave(x, fs))
        assert str(got.value) == str(want.value)
        switch.fn = f0_fn
        assert P.same(pipe.convert_wave(Wave(x, fs)).wave, good)
        pipe.close()
    ref.close()


def check_misfit_takes_the_composed_path(vc, fs, ctx, frames: int):
    """A callable with another frame count, and one with a shifted t: the call is counted as composed, the callable runs once, the bits are the
    chain's -- in `convert_wave` and in `push`."""
    from yukarin import Wave
    x = voiced_wave(samples_for(frames, fs), fs)
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3, ctx=ctx)
    for fn in (wrong_count_fn, shifted_t_fn):
        want = chain(vc, param_of(vc), fn, Wave(x, fs), ref)
        counting = Counting(fn)
        pipe = pipe_of(vc, counting)
        before = dict(pipeline.calls)
        got = pipe.convert_wave(Wave(x, fs))
        assert pipeline.calls['composed'] == before['composed'] + 1 and pipeline.calls['resident'] == before['resident']
        assert P.same(got.wave, want) and counting.sizes == [x.size]
        want_live = [chain_push(vc, param_of(vc), fn, Wave(x, fs), ref, (1, 1)), ref.flush()]
        got_live = [pipe.push(Wave(x, fs), discard=(1, 1)).wave, pipe.flush().wave]
        assert pipeline.calls['composed'] == before['composed'] + 2 and all(P.same(g, w) for g, w in zip(got_live, want_live))
        pipe.close()
    ref.close()


def check_other_fallbacks(vc, fs, ctx, monkeypatch, frames: int):
    """What section 14 sends down the composed chain still goes there in WORLD mode: a float64 wave that float32 does not hold, RY_DEVICE_GATE=0."""
    from yukarin import Wave
    x = voiced_wave(samples_for(frames, fs), fs)
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3, ctx=ctx)
    x64 = x.astype(numpy.float64)
    x64[1] += 2.0 ** -40
    pipe = pipe_of(vc)
    for wave, env in ((Wave(x64, fs), None), (Wave(x, fs), '0')):
        if env is not None:
            monkeypatch.setenv('RY_DEVICE_GATE', env)
        before = dict(pipeline.calls)
        want = chain(vc, param_of(vc), f0_fn, wave, ref)
        assert pipe._resident_handles(wave) is None
        assert P.same(pipe.convert_wave(wave).wave, want) and pipeline.calls['composed'] == before['composed'] + 1
        monkeypatch.delenv('RY_DEVICE_GATE', raising=False)
    pipe.close()
    ref.close()


# ---- 3. / 4. the bank and the gate in front -------------------------------------------------------------------------------------------
def bank_waves(fs, frames, silent=()):
    """One wave per stream at ragged lengths; the streams in `silent` get exact zeros."""
    from yukarin import Wave
    out = []
    for s, k in enumerate(frames):
        n = samples_for(k, fs) + s
        out.append(Wave(numpy.zeros(n, numpy.float32) if s in silent else half_quiet_wave(n, fs, s) if s % 2 else voiced_wave(n, fs, s), fs))
    return out


def lone_run(vc, fs, seed, calls, fn=f0_fn):
    """What a lone WORLD-mode `Pipeline(seed=seed)` returns for the calls of one stream: ('push', wave, discard, final) / ('flush',) / ('sit',)."""
    pipe = pipe_of(vc, fn, seed=seed)
    out = []
    for c in calls:
        if c[0] == 'push':
            out.append(pipe.push(c[1], discard=c[2], final=c[3]).wave)
        elif c[0] == 'flush':
            out.append(pipe.flush().wave)
        else:
            out.append(None)
    pipe.close()
    return out


def check_bank(vc, fs, frames, discard, gate_first=False, fn=None):
    """B = 3, ragged lengths and seeds: call 0 every stream; call 1 stream 1 sits out and `final` names stream 2; call 2 stream 1 silent (exact
    zeros); then the flush, then `convert_waves`.  Every stream equals its lone WORLD-mode pipeline, call by call."""
    from yukarin import Wave
    seeds = [3, 11, 29]
    counting = Counting(fn or f0_fn)
    rounds = [bank_waves(fs, frames), bank_waves(fs, [frames[2], frames[0], frames[1]]), bank_waves(fs, frames, silent=(1,))]
    rounds[1][1] = None
    finals = [(), (2,), ()]
    bank = pipeline.PipelineBank(vc, param_of(vc), 3, seeds=seeds, f0_mode='world', f0_fn=counting, gate_first=gate_first)
    before = pipeline.calls_many['resident']
    got = []
    for waves, final in zip(rounds, finals):
        got.append([w.wave for w in bank.push(waves, discard=discard, final=final, advance=5)])
    flushed = [w.wave for w in bank.flush()]
    assert pipeline.calls_many['resident'] == before + 3 and pipeline.calls_many['composed'] == 0
    for s in range(3):
        calls = [('push', r[s], discard, s in f) if r[s] is not None else ('sit',) for r, f in zip(rounds, finals)] + [('flush',)]
        want = lone_run(vc, fs, seeds[s], calls, fn or f0_fn)
        for k in range(3):
            if want[k] is None:
                assert got[k][s].size == 0
            else:
                assert P.same(got[k][s], want[k]), (s, k)
        assert P.same(flushed[s], want[3]), s
    one_shot = bank.convert_waves(rounds[0])
    lone = pipe_of(vc, fn or f0_fn, seed=seeds[0])
    assert all(P.same(g.wave, lone.convert_wave(w).wave) for g, w in zip(one_shot, rounds[0]))
    lone.close()
    vc._fused_core().set_discard(0, 0)
    bank.close()


def check_bank_out_gate(vc, fs, ctx, frames, discard, chunk: int, rounds: int = 3):
    """`out_gate=` with stream 1 silent over `rounds` calls: every stream's chunks -- scaled, float32 -- equal those of its lone pipeline
    over a lone `OutputGate`, call by call (a stream fed zeros is unvoiced throughout: the synthesizer returns shaped noise for it, and its gate
    judges that as it judges any chunk)."""
    from realtime_yukarin_amd import output_gate
    seeds = [3, 11, 29]
    waves = bank_waves(fs, frames, silent=(1,))
    gates = output_gate.OutputGateBank(3, chunk, P.THRESHOLD, 0.5, numpy.float32, ctx=ctx)
    bank = pipeline.PipelineBank(vc, param_of(vc), 3, seeds=seeds, f0_mode='world', f0_fn=f0_fn)
    got, last = [], []
    for _ in range(rounds):
        got.append([w.wave for w in bank.push(waves, discard=discard, out_gate=gates)])
        last.append(list(gates.last))
    bank.close()
    gates.close()
    assert all(any(l[s][0] for l in last) for s in range(3))           # every stream completed a chunk, the one fed zeros too
    assert all(g[s].size in (0, chunk) and g[s].dtype == numpy.float32 for g in got for s in range(3)) and sum(g[0].size + g[2].size for g in got) > 0
    for s in range(3):
        gate = output_gate.OutputGate(chunk, P.THRESHOLD, 0.5, numpy.float32, ctx=ctx)
        pipe = pipe_of(vc, seed=seeds[s])
        for k in range(rounds):
            assert P.same(pipe.push(waves[s], discard=discard, out_gate=gate).wave, got[k][s]), (s, k)
        pipe.close()
        gate.close()
    vc._fused_core().set_discard(0, 0)


def check_gate_first(vc, fs, frames, discard):
    """B = 3 with stream 1 silent and B = 1 silent, through `push` and `convert_waves`: the f0 callable runs for the audible waves only, the skipped
    ones are counted under 'gated', and the bits equal those with the flag off."""
    from yukarin import Wave
    seeds = [3, 11, 29]
    waves = bank_waves(fs, frames, silent=(1,))
    outs, seen = {}, {}
    for flag in (False, True):
        counting = Counting()
        bank = pipeline.PipelineBank(vc, param_of(vc), 3, seeds=seeds, f0_mode='world', f0_fn=counting, gate_first=flag)
        gated = pipeline.calls_many.get('gated', 0)
        outs[flag] = [w.wave for w in bank.push(waves, discard=discard)] + [w.wave for w in bank.flush()] + [w.wave for w in bank.convert_waves(waves)]
        seen[flag] = counting.sizes
        if flag:
            assert pipeline.calls_many['gated'] == gated + 2 and bank.last_gate['tracked'] == [True, False, True] and bank.last_gate['n_eff'][1] == 0
        bank.close()
    sizes = [w.wave.size for w in waves]
    assert seen[False] == sizes * 2 and seen[True] == [sizes[0], sizes[2]] * 2
    assert all(P.same(a, b) for a, b in zip(outs[True], outs[False])) and sum(o.size for o in outs[True]) > 0
    silent = Wave(numpy.zeros(sizes[1], numpy.float32), fs)
    for flag in (False, True):
        counting = Counting()
        pipe = pipe_of(vc, counting, gate_first=flag)
        gated = pipeline.calls.get('gated', 0)
        outs[flag] = [pipe.push(silent, discard=discard).wave, pipe.flush().wave, pipe.convert_wave(silent).wave]
        assert counting.sizes == ([] if flag else [sizes[1]] * 2)
        if flag:
            assert pipeline.calls['gated'] == gated + 2 and pipe.last_gate['tracked'] == [False]
        pipe.close()
    assert all(P.same(a, b) for a, b in zip(outs[True], outs[False]))
    vc._fused_core().set_discard(0, 0)


# ---- 5. no CREPE ----------------------------------------------------------------------------------------------------------------------
def check_no_crepe(vc, fs, ctx, monkeypatch, frames: int):
    """A WORLD-mode pipeline and bank are constructed and run with RY_CREPE_MODEL unset and no weights in the shim: `ry_crepe_create` is never
    called and the shim builds no model."""
    import os
    from yukarin import Wave
    from realtime_yukarin_amd.compat import crepe as shim
    assert 'RY_CREPE_MODEL' not in os.environ and not shim._weights and not shim._models
    created = []
    real = ctx.lib.dll.ry_crepe_create

    def create_spy(*a):
        created.append('ry_crepe_create')
        return real(*a)

    def model_spy(*a, **k):
        created.append('shim._model')
        raise AssertionError('a CREPE model was asked for')
    monkeypatch.setattr(ctx.lib.dll, 'ry_crepe_create', create_spy)
    monkeypatch.setattr(shim, '_model', model_spy)
    x = half_quiet_wave(samples_for(frames, fs), fs)
    ref = world_synth.Synthesizer(fs, P.FRAME_PERIOD, seed=3, ctx=ctx)
    want = chain(vc, param_of(vc), f0_fn, Wave(x, fs), ref)
    ref.close()
    pipe = pipe_of(vc, crepe_capacity='full')
    before = pipeline.calls['resident']
    assert P.same(pipe.convert_wave(Wave(x, fs)).wave, want) and P.same(pipe.convert_wave(Wave(x, fs), gate_first=True).wave, want)
    assert pipeline.calls['resident'] == before + 2
    pipe.close()
    bank = pipeline.PipelineBank(vc, param_of(vc), 2, seeds=[3, 3], f0_mode='world', f0_fn=f0_fn)
    assert all(P.same(w.wave, want) for w in bank.convert_waves([Wave(x, fs), Wave(x, fs)]))
    bank.close()
    assert created == [] and not shim._models
