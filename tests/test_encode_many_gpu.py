"""The many-waves encode on the MI355X: `CrepeModel.track_many` -> `Analyzer.run_device_many` against the shipped single-wave calls (`track` ->
`run_device`) on a separate handle of the same weights, bit for bit, in `f32` and `bf16x3` -- the seven outputs and the float32 rows left on the
card.  `tiny` capacity with synthetic weights, as in test_encode_gpu.py.  Cases: tests/encode_many_cases.py."""
import ctypes

import numpy
import pytest

import encode_cases as E
import encode_many_cases as M
from realtime_yukarin_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = ('f32', 'bf16x3')


@pytest.fixture(scope='module')
def rigs(gpu_ctx):
    made = {}

    def get(fs, dtype):
        if (fs, dtype) not in made:
            made[fs, dtype] = M.Rig(gpu_ctx, 'tiny', fs, dtype)
        return made[fs, dtype]
    yield get
    for r in made.values():
        r.close()


def wave(n, sr, seed):
    return E.mixed_wave(max(n, 8) / sr, sr, seed=seed)[:n]


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_pass_boundary_inside_a_wave_and_a_wave_boundary_inside_a_pass(rigs, dtype):
    """1.0 s, 0.6 s and one sample at 24 kHz, 5 ms: 201 + 121 + 1 frames, more than the 256 of a pass -- the second wave straddles the pass
    boundary, and in the permuted list the first wave ends inside a pass."""
    rig = rigs(24000, dtype)
    xs = [E.mixed_wave(1.0, 24000, 1), E.mixed_wave(0.6, 24000, 2), wave(2, 24000, 3)]
    singles = M.check_batch(rig, xs, frames=[201, 121, 1])
    M.check_batch(rig, xs, order=[1, 2, 0], singles=singles, frames=[201, 121, 1])


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_long_track_beside_a_short_one(rigs, dtype):
    """5.2 s (1041 frames: more than one pass of the voicing kernel through the LDS) next to 0.25 s."""
    rig = rigs(24000, dtype)
    assert 1041 > E.VOICING_CHUNK
    M.check_batch(rig, [E.mixed_wave(5.2, 24000, 4), E.mixed_wave(0.25, 24000, 5)], frames=[1041, 51])


@pytest.mark.parametrize('fs', [16000, 24000])
@pytest.mark.parametrize('dtype', DTYPES)
def test_eight_waves(rigs, fs, dtype):
    """Lengths drawn from a fixed seed between one sample and 0.5 s (at 24 kHz the shortest wave that still gives a 16 kHz sample has two)."""
    lengths = numpy.random.default_rng(8).integers(2 if fs != 16000 else 1, fs // 2 + 1, 8)
    lengths[3] = 2 if fs != 16000 else 1
    M.check_batch(rigs(fs, dtype), [wave(int(n), fs, 10 + i) for i, n in enumerate(lengths)])


def test_voicing_and_decode_over_segments(rigs):
    rig = rigs(16000, 'f32')
    M.check_voicing_many(rig.many, rig.one, device=True)
    M.check_decode_many(rig.many, rig.one, M.TRACK_FRAMES)


@pytest.mark.parametrize('dtype', DTYPES)
def test_poison_then_a_b_a_on_one_handle_equals_a_fresh_handle(rigs, dtype):
    rig = rigs(24000, dtype)
    a = [E.mixed_wave(0.3, 24000, 20), E.mixed_wave(0.1, 24000, 21), wave(2, 24000, 22)]
    b = [E.mixed_wave(0.05, 24000, 23), E.mixed_wave(0.2, 24000, 24)]
    rig.poison()
    got = [rig.batch(a), rig.batch(b), rig.batch(a)]
    fresh = rig.fresh()
    want_a, want_b = fresh.batch(a), fresh.batch(b)
    fresh.close()
    for g, w in zip(got, (want_a, want_b, want_a)):
        for gi, wi in zip(g, w):
            M.assert_same(gi, wi)


def test_a_refusal_on_a_running_stream_does_not_disturb_the_next_call(rigs):
    """A batched track is enqueued and not waited for; a refused call follows at once (it writes nothing and forgets the track that is in
    flight); the next good batches, in both orders, give the single calls' bits."""
    rig = rigs(24000, 'f32')
    xs = [E.mixed_wave(0.6, 24000, 30), E.mixed_wave(0.1, 24000, 31)]
    singles = [rig.single(x) for x in xs]
    lib, h = rig.many._get()
    rig.many.track_many(xs, 24000, 80, M.STEP, device=True)          # in flight
    counts = numpy.asarray([100, 0], numpy.int32)
    nf = numpy.full(2, -7, numpy.int32)
    _IP = ctypes.POINTER(ctypes.c_int)
    rc = lib.dll.ry_crepe_track_many(h, _lib._fptr(numpy.zeros(100, numpy.float32)), counts.ctypes.data_as(_IP), 2, 24000, 80, 5.0, 0.1,
                                     nf.ctypes.data_as(_IP), None, None, None, 1)
    assert rc == -1 and list(nf) == [-7, -7]
    assert lib.dll.ry_crepe_track_many_buffers(h, None, None, None, None, None, None, None) == -4
    M.check_batch(rig, xs, singles=singles)
    M.check_batch(rig, xs, order=[1, 0], singles=singles)
