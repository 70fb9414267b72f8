"""The fused CREPE-mode encode without a GPU: the voicing kernel, `CrepeModel.track` and `Analyzer.run_device` on the host-side SIMT emulator
against the host chain they replace (`crepe.predict_voicing`, the reference wrapper's mask, `Analyzer.run`), bit for bit; the refusals of the new
entry points; which path `encode.extract` takes.  Cases: tests/encode_cases.py."""
import ctypes

import numpy
import pytest

import encode_cases as E
from realtime_yukarin_amd import _lib, crepe, encode, world_analysis


@pytest.fixture(scope='module')
def model(emu_ctx):
    m = crepe.CrepeModel(1, seed=21, ctx=emu_ctx)
    yield m
    m.close()


@pytest.mark.parametrize('n', E.LENGTHS)
def test_voicing_equals_predict_voicing_and_the_mask(model, n):
    """Every confidence set (uniform, constants, square waves, the neighbourhood of the crossing of the two log densities, float32(0.1) and its
    neighbours) at every length: voiced, the masked float64 f0 and the time axis at steps 5 and 10 have the host's bits."""
    E.check_voicing(model, n)


@pytest.mark.parametrize('n', [3, 257, E.VOICING_CHUNK + 1])
def test_voicing_on_poisoned_buffers_and_from_device_pointers(model, n):
    E.check_voicing(model, n, poison=True)
    E.check_voicing(model, n, device=True)


def test_the_crossing_is_where_a_state_flips():
    """The case set is worth its name: the two log densities change order inside the neighbourhood `confidence_sets` draws from."""
    near = E.neighbours(E.crossing(), 3).astype(numpy.float64)
    mu, var = numpy.asarray(crepe.VOICING_MEANS), numpy.asarray(crepe.VOICING_VARS)
    logp = -0.5 * (numpy.log(2 * numpy.pi * var)[None, :] + (near[:, None] - mu[None, :]) ** 2 / var[None, :])
    d = logp[:, 1] - logp[:, 0]
    assert d[0] < 0 < d[-1]


def test_strict_threshold_is_numpys():
    """float32(0.1) is not above the Python float 0.1 for numpy (the comparison is made in float32); its upper neighbour is."""
    c = E.neighbours(numpy.float32(0.1), 1)
    assert list(c > 0.1) == [False, False, True]


def test_c_library_defaults_equal_numpys_tables(emu_ctx):
    """`ry_crepe_create` installs the HMM's constants itself; a handle that never got numpy's tables computes the same mask on a case set that
    does not sit on a rounding edge."""
    lib = emu_ctx.lib
    blob = crepe.flatten_params(1, crepe.synthetic_params(1, 1))
    h = ctypes.c_void_p()
    lib.check(lib.dll.ry_crepe_create(emu_ctx.handle, 1, _lib._fptr(blob), blob.size, 1e-3, ctypes.byref(h)))
    c = E.confidence_sets(300)['square 7']
    f0 = numpy.full(300, 100.0, numpy.float32)
    v, f64, t = numpy.empty(300, numpy.uint8), numpy.empty(300), numpy.empty(300)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    lib.check(lib.dll.ry_crepe_voicing(h, _lib._fptr(c), _lib._fptr(f0), 300, 0.1, 5.0, v.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), dp(f64), dp(t), 0))
    assert numpy.array_equal(v.astype(bool), E.voicing_reference(c, f0, 5)[0])
    # refusals
    assert lib.dll.ry_crepe_voicing(h, _lib._fptr(c), _lib._fptr(f0), 0, 0.1, 5.0, v.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), dp(f64), dp(t), 0) == -1
    assert lib.dll.ry_crepe_voicing(h, _lib._fptr(c), _lib._fptr(f0), 300, 0.1, 0.0, v.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), dp(f64), dp(t), 0) == -1
    assert lib.dll.ry_crepe_track_buffers(h, None, None, None, None, None, None) == -4           # RY_ESTATE: no track has run
    lib.dll.ry_crepe_destroy(h)


@pytest.mark.parametrize('sr', [16000, 24000])
def test_track_equals_the_chain_it_replaces(model, sr):
    """20 ms (5 frames: the emulator runs the network at about ten frames a second; the GPU tests run 0.25 s and 0.6 s) at the smallest capacity:
    `track` against predict -> predict_voicing -> mask, then on poisoned buffers and left on the card."""
    x, hop, got = E.check_track(model, 0.02, sr)
    assert got[0].size == 5
    model.poison()
    trk = model.track(x, sr, hop, 5, device=True)
    assert (trk.frames, trk.samples) == (5, x.size)
    voiced, f64 = trk.download()
    assert numpy.array_equal(voiced, got[0]) and E.same(f64, got[1])
    model.voicing(numpy.zeros(3, numpy.float32), numpy.ones(3, numpy.float32))          # reuses the buffers: the track is gone
    lib, h = model._get()
    assert lib.dll.ry_crepe_track_buffers(h, None, None, None, None, None, None) == -4


def test_track_refuses_what_predict_refuses(model):
    with pytest.raises(ValueError):
        model.track(numpy.zeros(0, numpy.float32), 16000, 80, 5)
    with pytest.raises(ValueError):
        model.track(numpy.zeros(1, numpy.float32), 24000, 80, 5)   # no sample at 16 kHz


@pytest.mark.parametrize('fs', [16000, 24000])
def test_run_device_equals_run(emu_ctx, fs):
    E.check_run_device(emu_ctx, fs)


def test_extract_takes_the_unfused_path_unless_everything_holds(monkeypatch):
    """The conditions of the fused path, without a device: a class nobody named, `pyworld` D4C, two channels, a float64 wave that does not
    round-trip through float32, a fractional rate, RY_CREPE_RESAMPLE=host."""
    class Wave(object):
        def __init__(self, wave, sampling_rate):
            self.wave, self.sampling_rate = wave, sampling_rate

    class Plain(object):
        pass

    class Crepe(Plain):
        pass

    monkeypatch.setattr(encode, 'crepe_classes', {Crepe})
    monkeypatch.setattr(world_analysis, 'aperiodicity', world_analysis.device_aperiodicity)
    monkeypatch.delenv('RY_CREPE_RESAMPLE', raising=False)
    x32 = numpy.linspace(-1, 1, 100).astype(numpy.float32)
    assert encode._fusable(Crepe, Wave(x32, 24000)) and encode._fusable(type('Sub', (Crepe,), {}), Wave(x32.astype(numpy.float64), 16000))
    assert not encode._fusable(Plain, Wave(x32, 24000))
    assert not encode._fusable(Crepe, Wave(numpy.stack([x32, x32], 1), 24000))
    assert not encode._fusable(Crepe, Wave(numpy.linspace(-1, 1, 100), 24000))
    assert not encode._fusable(Crepe, Wave(x32, 22050.5))
    assert not encode._fusable(Crepe, Wave(x32[:0], 24000))
    monkeypatch.setenv('RY_CREPE_RESAMPLE', 'host')
    assert not encode._fusable(Crepe, Wave(x32, 24000)) and encode._fusable(Crepe, Wave(x32, 16000))
    monkeypatch.delenv('RY_CREPE_RESAMPLE')
    monkeypatch.setattr(world_analysis, 'aperiodicity', lambda *a: None)
    assert not encode._fusable(Crepe, Wave(x32, 24000))
