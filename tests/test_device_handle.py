"""The life of a device handle (realtime_yukarin_amd/_handle.py) for the three classes built on it -- `Synthesizer`, `Analyzer`, `CrepeModel` -- on the
emulator, and the call buffers of one handle (csrc/ry_host.h: DevBuf) growing between calls: small, then large enough that every buffer is replaced
(80 > 3 + 3 / 2 + 64 frames and 2000 > 400 + 200 + 64 samples for the analysis, 120 frames for the synthesizer, exact sizes for CREPE), then small
again, poisoned before every step -- on the emulator and, the same body, on the GPU.  Everything is compared bit for bit."""
import os
import pickle
import types

import numpy
import pytest

import world_analysis_cases as CA
import world_synth_cases as CS
from realtime_yukarin_amd import crepe, engine, world_analysis, world_synth

FS = 16000
CREPE_HOP = 160
SIZES = {'synth': (3, 120), 'analysis': ((3, 400), (80, 2000)), 'crepe': (1, 3)}      # (small, large): frames, (frames, samples), frames


def make(unit, ctx):
    if unit == 'synth':
        return world_synth.Synthesizer(FS, 5.0, seed=3, ctx=ctx)
    if unit == 'analysis':
        a = world_analysis.Analyzer(FS, order=CA.ORDER, seed=3, ctx=ctx)
        a.record_integers()                                        # the buffers of the recorded decisions grow too
        return a
    return crepe.CrepeModel(1, seed=3, ctx=ctx)


def call(unit, obj, size):
    """One call of the unit at SIZES[unit][size] -> tuple of arrays."""
    n = SIZES[unit][size]
    if unit == 'synth':
        return (obj.synthesize(*CS.case('glide', n, FS)),)
    if unit == 'analysis':
        frames, samples = n
        x = numpy.random.default_rng(frames).normal(0.0, 0.1, samples) + numpy.sin(numpy.arange(samples) * 0.05)
        out = obj.run(x, CA.f0_track('alternating', frames), CA.times(frames), want=('sp', 'mc', 'ap', 'coded_ap'))
        return out + (obj.integers(),) + obj.d4c_record()
    x = numpy.random.default_rng(n).normal(0.0, 0.3, 1024 + (n - 1) * CREPE_HOP).astype(numpy.float32)
    return obj.predict16k(x, CREPE_HOP, center=False)


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


UNITS = ('synth', 'analysis', 'crepe')


@pytest.mark.parametrize('unit', UNITS)
def test_pickle_close_and_foreign_context(emu_ctx, monkeypatch, unit):
    asked = []
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: asked.append(device) or emu_ctx)
    obj = make(unit, emu_ctx)
    first = call(unit, obj, 0)
    assert obj._handle is not None and obj._ctx is emu_ctx and obj._pid == os.getpid() and not asked
    copy = pickle.loads(pickle.dumps(obj))
    assert copy._handle is None and copy._ctx is None and copy._given_ctx is None and copy._pid is None
    assert obj._handle is not None and obj._given_ctx is emu_ctx   # pickling leaves the original alone
    if unit == 'crepe':
        assert copy._rs == {}
    if unit == 'analysis':
        copy.record_integers()                                     # a switch of the handle, not of the object: the fresh handle starts without it
    assert same_bits(call(unit, copy, 0), first)
    assert asked == [obj.device] and copy._ctx is emu_ctx          # no context travelled: the copy asked the engine for this process's
    assert copy._handle is not None and copy._handle.value != obj._handle.value and copy._pid == os.getpid()
    for o in (obj, copy):
        o.close()
        assert o._handle is None
        o.close()
    # a context made by another process is not used: the engine's context of this process is
    foreign = types.SimpleNamespace(pid=os.getpid() + 1, lib=None, handle=None)
    other = make(unit, foreign)
    assert same_bits(call(unit, other, 0), first)
    assert other._ctx is emu_ctx and asked == [obj.device, other.device]
    other.close()


def regrowth(ctx, unit):
    obj, fresh = make(unit, ctx), make(unit, ctx)
    steps = []
    for size in (0, 1, 0):
        obj.poison()
        steps.append(call(unit, obj, size))
        assert all(numpy.isfinite(a).all() for a in steps[-1] if a.dtype.kind == 'f')
    assert same_bits(steps[0], steps[2])
    assert same_bits(steps[1], call(unit, fresh, 1))
    assert not same_bits(steps[0], steps[1])
    obj.close(); fresh.close()


@pytest.mark.parametrize('unit', UNITS)
def test_buffers_regrow_between_calls(emu_ctx, unit):
    regrowth(emu_ctx, unit)


@pytest.mark.gpu
@pytest.mark.parametrize('unit', UNITS)
def test_buffers_regrow_between_calls_gpu(gpu_ctx, unit):
    regrowth(gpu_ctx, unit)
