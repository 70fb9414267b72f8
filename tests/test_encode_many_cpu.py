"""The many-waves encode without a GPU, on the host-side SIMT emulator: `CrepeModel.track_many` -> `Analyzer.run_device_many` against the shipped
single-wave calls (`track` -> `run_device`) on a separate handle of the same weights, bit for bit; the decode and the voicing over a segment table
alone; poison, reuse and the refusals of the new entry points; which path `encode.extract_many` takes.  Smallest capacity, at most about 12 frames
through the network per call (the emulator runs about ten frames a second).  Cases: tests/encode_many_cases.py."""
import ctypes

import numpy
import pytest

import encode_cases as E
import encode_many_cases as M
from realtime_yukarin_amd import _lib, crepe, encode, world_analysis

_IP, _UBP, _DP = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope='module')
def rigs(emu_ctx):
    r = {fs: M.Rig(emu_ctx, 1, fs) for fs in (16000, 24000)}
    yield r
    for v in r.values():
        v.close()


def wave(n, sr, seed):
    return E.mixed_wave(max(n, 8) / sr, sr, seed=seed)[:n]


# 16 kHz: 1, 80, 320 samples -> 1, 2, 5 frames at hop 80.  24 kHz: 2, 40, 480 samples -> 1, 26, 320 outputs of the resampler -> 1, 1, 5 frames
MIXED = {16000: ((1, 80, 320), [1, 2, 5]), 24000: ((2, 40, 480), [1, 1, 5])}


def test_one_wave_equals_track_and_run_device(rigs):
    M.check_batch(rigs[24000], [wave(480, 24000, 3)], frames=[5])


@pytest.mark.parametrize('fs', [16000, 24000])
def test_mixed_short_waves_and_their_permutation(rigs, fs):
    """Wave i of the batch equals its single call in every output, and the permuted list gives the permuted results."""
    lengths, frames = MIXED[fs]
    if fs == 24000:
        assert [crepe.resampled_length(n, fs) for n in lengths] == [1, 26, 320]
    xs = [wave(n, fs, i) for i, n in enumerate(lengths)]
    singles = M.check_batch(rigs[fs], xs, frames=frames)
    M.check_batch(rigs[fs], xs, order=[2, 0, 1], singles=singles, frames=frames)


@pytest.mark.parametrize('fs', [16000, 24000])
def test_a_loud_neighbour_moves_no_bit(rigs, fs):
    """A short wave between two waves of constant 1e30: a frame, a resampler tap or an analysis window that crossed a segment boundary would show."""
    n = 120 * fs // 16000                                            # 2 frames each
    x = wave(n, fs, 9)
    want = rigs[fs].single(x)
    got = rigs[fs].batch([M.loud(n), x, M.loud(n)])
    assert [g['voiced'].size for g in got] == [2, 2, 2]
    M.assert_same(got[1], want)


def test_voicing_over_segments(rigs):
    """Tracks of 1, 2, 3, CHUNK - 1, CHUNK + 1 and 2 CHUNK + 1 frames side by side through device pointers, no network: every track equals
    `voicing` on it alone, at the tie-laden and the crossing confidence sets, both steps."""
    M.check_voicing_many(rigs[16000].many, rigs[16000].one, device=True)
    M.check_voicing_many(rigs[16000].many, rigs[16000].one, frames=(3, 1), device=False)


@pytest.mark.parametrize('viterbi', [True, False])
def test_decode_over_segments(rigs, viterbi):
    M.check_decode_many(rigs[16000].many, rigs[16000].one, M.TRACK_FRAMES, viterbi)


def test_poisoned_handles_give_the_clean_bits(rigs):
    rig = rigs[24000]
    xs = [wave(n, 24000, 20 + i) for i, n in enumerate((40, 240))]            # 1 + 3 frames
    clean = rig.batch(xs)
    rig.poison()
    for g, w in zip(rig.batch(xs), clean):
        M.assert_same(g, w)
    rig.poison()
    M.assert_same(rig.single(xs[1]), clean[1])


def test_a_smaller_call_after_a_larger_one_equals_a_fresh_handle(rigs):
    rig = rigs[16000]
    rig.batch([wave(n, 16000, 30 + i) for i, n in enumerate((320, 160, 80))])          # 5 + 3 + 2 frames
    small = [wave(n, 16000, 40 + i) for i, n in enumerate((80, 1))]                    # 2 + 1
    got = rig.batch(small)
    fresh = rig.fresh()
    for g, w in zip(got, fresh.batch(small)):
        M.assert_same(g, w)
    fresh.close()


def _track_many_raw(model, xs, sr, on_device_out=0, step=5.0, outs=None):
    lib, h = model._get()
    counts = numpy.asarray([x.size for x in xs], numpy.int32)
    audio = numpy.ascontiguousarray(numpy.concatenate(xs + [numpy.zeros(1, numpy.float32)]))
    nf, v, f, t = outs
    return lib.dll.ry_crepe_track_many(h, _lib._fptr(audio), counts.ctypes.data_as(_IP), len(xs), sr, 80, step, 0.1, nf.ctypes.data_as(_IP),
                                       v.ctypes.data_as(_UBP), f.ctypes.data_as(_DP), t.ctypes.data_as(_DP), on_device_out)


def test_track_many_refusals_write_nothing(emu_ctx):
    """B < 1, a wave with no sample, a wave the single call refuses (no sample at 16 kHz), missing resampler tables, a step the voicing refuses:
    all before anything is launched -- the outputs keep their fill and `ry_crepe_track_many_buffers` reports no track."""
    model = crepe.CrepeModel(1, seed=21, ctx=emu_ctx)
    lib, h = model._get()
    good = [wave(40, 16000, 1), wave(1, 16000, 2)]                    # one frame each
    model.track_many(good, 16000, 80, 5)                              # tracks on the card, so that a refusal has something to forget
    model._resampler(24000, 64)

    def fill():
        return numpy.full(8, -7, numpy.int32), numpy.full(64, 9, numpy.uint8), numpy.full(64, numpy.nan), numpy.full(64, numpy.nan)
    empty = numpy.zeros(0, numpy.float32)
    cases = [([], 16000, 5.0, -1), ([good[0], empty], 16000, 5.0, -1), ([empty], 16000, 5.0, -1),
             ([wave(48, 24000, 3), wave(1, 24000, 4)], 24000, 5.0, -1),          # the second yields no 16 kHz sample
             ([wave(48, 24000, 3), wave(480, 24000, 4)], 24000, 5.0, -4),        # the time register holds 64 outputs: RY_ESTATE
             (good, 22050, 5.0, -4),                                            # no tables for the rate
             (good, 16000, 0.0, -1)]
    for xs, sr, step, code in cases:
        model.track_many(good, 16000, 80, 5)
        outs = fill()
        rc = _track_many_raw(model, list(xs), sr, 0, step, outs)
        assert rc == code, (rc, code, lib.dll.ry_last_error())
        assert all(E.same(o, w) for o, w in zip(outs, fill())), (sr, step)
        assert lib.dll.ry_crepe_track_many_buffers(h, None, None, None, None, None, None, None) == -4
    # totals beyond the frame limit of the single calls: 2^24 frames at hop 1 need 2^24 samples at 16 kHz -- refused from the counts alone
    big = numpy.asarray([1 << 23, 1 << 23, 8], numpy.int32)
    outs = fill()
    rc = lib.dll.ry_crepe_track_many(h, _lib._fptr(numpy.zeros(1, numpy.float32)), big.ctypes.data_as(_IP), 3, 16000, 1, 5.0, 0.1,
                                     outs[0].ctypes.data_as(_IP), outs[1].ctypes.data_as(_UBP), outs[2].ctypes.data_as(_DP), outs[3].ctypes.data_as(_DP), 0)
    assert rc == -1 and b'frames' in lib.dll.ry_last_error() and all(E.same(o, w) for o, w in zip(outs, fill()))
    assert lib.dll.ry_crepe_track_many_buffers(h, None, None, None, None, None, None, None) == -4
    # ... and beyond the 32-bit sample offsets of the card: 2^30 + 2^30 + 8 samples at hop 2^20 are 1025 + 1025 + 1 frames, so it is the sample
    # total that refuses -- again from the counts alone
    model.track_many(good, 16000, 80, 5)
    big = numpy.asarray([1 << 30, 1 << 30, 8], numpy.int32)
    outs = fill()
    rc = lib.dll.ry_crepe_track_many(h, _lib._fptr(numpy.zeros(1, numpy.float32)), big.ctypes.data_as(_IP), 3, 16000, 1 << 20, 5.0, 0.1,
                                     outs[0].ctypes.data_as(_IP), outs[1].ctypes.data_as(_UBP), outs[2].ctypes.data_as(_DP), outs[3].ctypes.data_as(_DP), 0)
    assert rc == -1 and b'samples' in lib.dll.ry_last_error() and all(E.same(o, w) for o, w in zip(outs, fill())), lib.dll.ry_last_error()
    assert lib.dll.ry_crepe_track_many_buffers(h, None, None, None, None, None, None, None) == -4
    # the single-wave track and the batched one forget each other
    model.track_many(good, 16000, 80, 5)
    assert lib.dll.ry_crepe_track_buffers(h, None, None, None, None, None, None) == -4
    model.track(good[0], 16000, 80, 5, device=True)
    assert lib.dll.ry_crepe_track_many_buffers(h, None, None, None, None, None, None, None) == -4
    model.track_many(good, 16000, 80, 5)
    model.voicing_many([numpy.zeros(3, numpy.float32)], [numpy.ones(3, numpy.float32)])
    assert lib.dll.ry_crepe_track_many_buffers(h, None, None, None, None, None, None, None) == -4
    # a good call after all of it
    got = model.track_many(good, 16000, 80, 5, device=False)
    assert [g[0].size for g in got] == [1, 1]
    model.close()


def test_extract_many_dev_refusals_write_nothing(emu_ctx):
    """B < 1, offsets that do not start at 0, a wave with no sample, a wave with no frame, and a track the single call refuses -- found by the one
    verdict of the call, in the second wave: the host arrays and the device rows keep their fill."""
    fs = 16000
    a = world_analysis.Analyzer(fs, order=8, seed=5, ctx=emu_ctx)
    lib, h = a._get()
    x, f0, t = E.analysis_case(fs, n=6)
    xx, ff, tt = numpy.concatenate([x, x]), numpy.concatenate([f0, f0]), numpy.concatenate([t, t])
    so, fo = numpy.asarray([0, x.size, 2 * x.size], numpy.int64), numpy.asarray([0, 6, 12], numpy.int32)
    bad_f0 = ff.copy()
    bad_f0[9] = numpy.nan
    dev = E.DeviceArrays(emu_ctx, xx, ff, tt, bad_f0, numpy.full((12, 513), numpy.nan, numpy.float32))
    LLP = ctypes.POINTER(ctypes.c_longlong)

    def call(so_, fo_, n_waves, f0_address):
        outs = [numpy.full(s, numpy.nan) for s in ((12, 513), (12, 9), (12, 513), (12, a.bands()))]
        rc = lib.dll.ry_analysis_extract_many_dev(h, _lib._fptr(dev.address[0]), so_.ctypes.data_as(LLP), E._DP(f0_address), E._DP(dev.address[2]),
                                                  fo_.ctypes.data_as(_IP), n_waves, 0.85, E._dp(outs[0]), _lib._fptr(dev.address[4]), E._dp(outs[1]),
                                                  E._dp(outs[2]), None, E._dp(outs[3]))
        rows = numpy.zeros((12, 513), numpy.float32)
        emu_ctx.dev_download(dev.address[4], rows)
        return rc, outs, rows
    cases = [(so, fo, 0, 1), (so + 1, fo, 2, 1), (numpy.asarray([0, x.size, x.size], numpy.int64), fo, 2, 1),
             (so, numpy.asarray([0, 12, 12], numpy.int32), 2, 1), (so, fo, 2, 3)]
    for so_, fo_, n_waves, f0_index in cases:
        rc, outs, rows = call(so_, fo_, n_waves, dev.address[f0_index])
        assert rc == -1, (rc, lib.dll.ry_last_error())
        assert all(numpy.isnan(o).all() for o in outs) and numpy.isnan(rows).all()
    assert b'f0[9]' in lib.dll.ry_last_error()
    # more than 2^22 frames in all, the single call's limit: refused from the offsets alone
    rc, outs, rows = call(so, numpy.asarray([0, 1 << 22, (1 << 22) + 1], numpy.int32), 2, dev.address[1])
    assert rc == -1 and b'frames in one call' in lib.dll.ry_last_error(), lib.dll.ry_last_error()
    assert all(numpy.isnan(o).all() for o in outs) and numpy.isnan(rows).all()
    rc, outs, rows = call(so, fo, 2, dev.address[1])                  # and a good call after them: both halves are the single call's rows
    assert rc == 0
    want = a.run(x.astype(numpy.float64), f0, t, want=M.KEYS)
    for o, w in zip(outs, want):
        assert E.same(o[:6], w) and E.same(o[6:], w)
    assert E.same(rows[6:], want[0].astype(numpy.float32))
    dev.close()
    a.close()


class Wave(object):
    def __init__(self, wave, sampling_rate):
        self.wave, self.sampling_rate = wave, sampling_rate


def test_extract_many_takes_the_batched_path_only_when_every_wave_holds(monkeypatch):
    """The path through `encode.calls`, without a device: a fusable list is one batched call; a float64 wave that does not round-trip through
    float32, or mixed rates, send every wave through `extract`; an empty list calls nothing."""
    class Crepe(object):
        pass

    seen = []
    monkeypatch.setattr(encode, 'crepe_classes', {Crepe})
    monkeypatch.setattr(world_analysis, 'aperiodicity', world_analysis.device_aperiodicity)
    monkeypatch.delenv('RY_CREPE_RESAMPLE', raising=False)
    monkeypatch.setattr(encode, 'calls', {'fused': 0, 'unfused': 0, 'many': 0})

    def one(cls, wave, *args):
        encode.calls['fused' if encode._fusable(cls, wave) else 'unfused'] += 1
        seen.append(wave)
        return wave
    monkeypatch.setattr(encode, 'extract', one)

    class Stop(Exception):
        pass

    def batched(*a, **k):
        raise Stop()
    from realtime_yukarin_amd.compat import crepe as shim
    monkeypatch.setattr(shim, '_model', batched)                      # the first thing the batched path asks for
    args = (5, 71.0, 800.0, 1024, 8, 0.466, numpy.float32)
    x32 = numpy.linspace(-1, 1, 100).astype(numpy.float32)
    x64 = numpy.linspace(-1, 1, 100)
    assert not numpy.array_equal(x64.astype(numpy.float32).astype(numpy.float64), x64)
    assert encode.extract_many(Crepe, [], *args) == [] and encode.calls == {'fused': 0, 'unfused': 0, 'many': 0}
    with pytest.raises(Stop):
        encode.extract_many(Crepe, [Wave(x32, 24000), Wave(x32[:50].astype(numpy.float64), 24000)], *args)
    assert encode.calls == {'fused': 0, 'unfused': 0, 'many': 1} and not seen
    mixed = [Wave(x32, 24000), Wave(x64, 24000)]
    assert encode.extract_many(Crepe, mixed, *args) == mixed
    assert encode.calls == {'fused': 1, 'unfused': 1, 'many': 1}
    rates = [Wave(x32, 24000), Wave(x32, 16000)]
    assert encode.extract_many(Crepe, rates, *args) == rates
    assert encode.calls == {'fused': 3, 'unfused': 1, 'many': 1}
    # more frames than one analysis call takes (100 samples at 24 kHz are 66 at 16 kHz: one frame each): wave by wave, which succeeds
    assert encode.max_many_frames == 1 << 22
    monkeypatch.setattr(encode, 'max_many_frames', 2)
    long_ = [Wave(x32, 24000)] * 3
    assert encode.extract_many(Crepe, long_, *args) == long_
    assert encode.calls == {'fused': 6, 'unfused': 1, 'many': 1}
    with pytest.raises(Stop):
        encode.extract_many(Crepe, long_[:2], *args)
    assert encode.calls == {'fused': 6, 'unfused': 1, 'many': 2}


def test_extract_many_equals_extract(emu_ctx, monkeypatch):
    """Through the drop-in `AcousticFeature` on the emulator: two short waves in one batched call equal `encode.extract` of each."""
    from realtime_yukarin_amd.compat import crepe as shim
    from realtime_yukarin_amd.compat.yukarin import AcousticFeature, Wave as YWave

    class Feature(AcousticFeature):
        pass

    class CrepeFeature(Feature):
        pass

    model = crepe.CrepeModel(1, seed=21, ctx=emu_ctx)
    monkeypatch.setattr(shim, '_models', {1: model})                  # the shim's model of capacity 1: on the emulator
    monkeypatch.delenv('RY_CREPE_RESAMPLE', raising=False)
    monkeypatch.setattr(world_analysis, 'aperiodicity', world_analysis.device_aperiodicity)
    monkeypatch.setattr(world_analysis, '_analyzers', {})
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(encode, 'crepe_classes', set())
    monkeypatch.setattr(encode, 'model_capacity', 1)
    monkeypatch.setattr(encode, 'calls', {'fused': 0, 'unfused': 0, 'many': 0})
    encode.install(Feature, CrepeFeature)
    args = dict(frame_period=5, f0_floor=71.0, f0_ceil=800.0, fft_length=1024, order=8, alpha=0.466, dtype=numpy.float32)
    waves = [YWave(wave(n, 24000, 50 + i), 24000) for i, n in enumerate((240, 40))]
    got = encode.extract_many(CrepeFeature, waves, **args)
    assert encode.calls == {'fused': 0, 'unfused': 0, 'many': 1}
    for g, w in zip(got, waves):
        want = encode.extract(CrepeFeature, w, **args)
        assert type(g) is type(want)
        for k in ('f0', 'sp', 'ap', 'coded_ap', 'mc', 'voiced'):
            assert E.same(getattr(g, k), getattr(want, k)), k
    assert encode.calls == {'fused': 2, 'unfused': 0, 'many': 1}
    for a in world_analysis._analyzers.values():
        a.close()
    model.close()
