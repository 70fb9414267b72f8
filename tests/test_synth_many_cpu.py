"""The batched WORLD synthesis (`Synthesizer.synthesize_many` / `ry_synth_run_many`) without a GPU, on the host-side SIMT emulator: every wave of
every batched call against `synthesize` of its item alone on a separate handle, bit for bit in the samples and the pulse lists; the refusals of the
C ABI; `decode_many` on the restated `Vocoder` body.  Tens of frames per wave -- the emulator is slow.  Cases: tests/synth_many_cases.py."""
import ctypes
import sys

import numpy
import pytest

import synth_many_cases as M
import world_synth_cases as C
from realtime_yukarin_amd import _lib, compat, world_synth

_DP, _IP, _LP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)
RATES = (16000, 24000)


@pytest.fixture(scope='module')
def rigs(emu_ctx):
    r = {fs: M.Rig(emu_ctx, fs) for fs in RATES}
    yield r
    for v in r.values():
        v.close()


@pytest.mark.parametrize('fs', RATES)
def test_one_wave_equals_synthesize(rigs, fs):
    M.check_batch(rigs[fs], M.glides(rigs[fs], [40]))


@pytest.mark.parametrize('fs', RATES)
def test_shortest_waves_and_their_reversal(rigs, fs):
    """1, 2 and 5 frames: one frame is a single sample, and the last pulse of a wave has no successor."""
    keyed = M.glides(rigs[fs], [1, 2, 5])
    out = M.check_batch(rigs[fs], keyed)
    assert len(out[0]) == 1
    M.check_batch(rigs[fs], keyed, order=[2, 1, 0])


@pytest.mark.parametrize('fs', RATES)
def test_either_side_of_a_scan_block_and_an_overlap_workgroup(rigs, fs):
    M.check_block_edges(rigs[fs])


def test_kinds_side_by_side(rigs):
    M.check_kinds(rigs[16000], 30)


@pytest.mark.parametrize('fs', RATES)
def test_a_loud_neighbour_moves_no_bit(rigs, fs):
    M.check_no_leak(rigs[fs])


def test_noise_is_keyed_by_the_position_inside_the_wave(rigs):
    M.check_noise_position(rigs[16000])


def test_device_rows_in_place_and_mixed_lists(rigs):
    M.check_device_rows(rigs[24000])


def test_poisoned_buffers_change_nothing(rigs):
    M.check_poison(rigs[16000])


def test_a_b_a_on_one_handle(rigs):
    M.check_aba(rigs[24000])


def test_stream_after_and_around_a_batched_call(rigs):
    M.check_stream(rigs[16000])


def test_abi_refusals_leave_the_outputs_untouched(emu_ctx):
    lib, d = emu_ctx.lib, emu_ctx.lib.dll
    h = ctypes.c_void_p()
    lib.check(d.ry_synth_create(emu_ctx.handle, 16000, 5.0, 1024, 0, ctypes.byref(h)))
    frames = [3, 4]
    f0 = numpy.concatenate([C.f0_track('glide', n, 16000) for n in frames])
    sp, ap = C.spectrogram(7), C.aperiodicity(7)
    MARK = -7.25
    y = numpy.full(2000, MARK)
    off = numpy.full(3, -99, numpy.int64)
    need = 161 + 241

    def run(f0_=f0, sp_=sp, ap_=ap, n_=frames, waves=2, bins=513, cap=2000, y_=y, off_=off, handle=h):
        n_ = None if n_ is None else numpy.asarray(n_, numpy.int32)
        rc = d.ry_synth_run_many(handle, None if f0_ is None else f0_.ctypes.data_as(_DP), None if sp_ is None else _lib._fptr(sp_),
                                 None if ap_ is None else _lib._fptr(ap_), None if n_ is None else n_.ctypes.data_as(_IP), waves, bins, 0,
                                 None if y_ is None else y_.ctypes.data_as(_DP), cap, None if off_ is None else off_.ctypes.data_as(_LP))
        assert (y == MARK).all() and (off == -99).all()
        return rc, d.ry_last_error()

    for null in ('f0_', 'sp_', 'ap_', 'n_', 'y_', 'off_'):
        rc, msg = run(**{null: None})
        assert rc == -1 and b'null' in msg, null
    assert run(waves=0)[0] == -1 and run(waves=-3)[0] == -1
    rc, msg = run(n_=[3, 0])
    assert rc == -1 and b'wave 1 has 0 frames' in msg
    assert run(n_=[-1, 4])[0] == -1
    for bins in (512, 1025):
        rc, msg = run(bins=bins)
        assert rc == -1 and b'bins' in msg
    for bad_value in (numpy.inf, numpy.nan, 8000.0, -numpy.inf):
        bad = f0.copy()
        bad[3 + 2] = bad_value                                              # wave 1, frame 2
        rc, msg = run(f0_=bad)
        assert rc == -1 and b'wave 1: f0[2]' in msg, msg
    bad = f0.copy()
    bad[1] = numpy.nan
    assert b'wave 0: f0[1]' in run(f0_=bad)[1]
    rc, msg = run(cap=need - 1)
    assert rc == -1 and b'y holds' in msg
    # totals: more than 2^22 frames in all (refused from the counts: the arrays are not read) ...
    rc, msg = run(n_=[1 << 22, 1])
    assert rc == -1 and b'frames' in msg
    assert run(n_=[(1 << 22) + 1], waves=1)[0] == -1
    # ... and more samples than the pulse arrays of one call index (2^30 entries, the single call's limit): 1 s frames at 48 kHz
    g = ctypes.c_void_p()
    lib.check(d.ry_synth_create(emu_ctx.handle, 48000, 1000.0, 1024, 0, ctypes.byref(g)))
    rc, msg = run(n_=[12000, 12000], handle=g, cap=1 << 40)
    assert rc == -1 and b'samples' in msg
    rc, msg = run(n_=[30000], waves=1, handle=g, cap=1 << 40)
    assert rc == -1 and b'samples' in msg
    d.ry_synth_destroy(g)
    assert d.ry_synth_run_many(None, None, None, None, None, 1, 513, 0, None, 0, None) == -4
    n = ctypes.c_int(-5)
    assert d.ry_synth_debug_pulses_many(h, 0, None, None, None, 0, ctypes.byref(n)) == -4 and n.value == 0      # no batched call yet
    # the same arguments, accepted
    rc = d.ry_synth_run_many(h, f0.ctypes.data_as(_DP), _lib._fptr(sp), _lib._fptr(ap), numpy.asarray(frames, numpy.int32).ctypes.data_as(_IP), 2, 513, 0,
                             y.ctypes.data_as(_DP), need, off.ctypes.data_as(_LP))
    assert rc == 0 and list(off) == [0, 161, need] and numpy.isfinite(y[:need]).all() and (y[:need] != MARK).all() and (y[need:] == MARK).all()
    assert d.ry_synth_debug_pulses_many(h, 2, None, None, None, 0, ctypes.byref(n)) == -1
    assert d.ry_synth_debug_pulses_many(h, 1, None, None, None, 0, ctypes.byref(n)) == 0 and n.value > 0
    d.ry_synth_destroy(h)


def test_python_refusals(rigs):
    s = rigs[16000].many
    f0, sp, ap = M.item('glide', 4, 16000)
    assert s.synthesize_many([]) == []
    with pytest.raises(ValueError):
        s.synthesize_many([(f0, sp[:3], ap)])
    with pytest.raises(ValueError):
        s.synthesize_many([(f0, sp[:, :512], ap[:, :512])])
    with pytest.raises(RuntimeError):
        s.synthesize_many([(f0, sp, ap), (f0[:0], sp[:0], ap[:0])])


# ---- the reference's class, restated as tests/test_world_synth_cpu.py restates it (realtime_voice_conversion/yukarin_wrapper/vocoder.py:15-62) ----
class _Param(object):
    frame_period = 5.0


class Vocoder(object):
    def __init__(self, acoustic_param, out_sampling_rate, extract_f0_mode=None):
        self.acoustic_param = acoustic_param
        self.out_sampling_rate = out_sampling_rate
        self.extract_f0_mode = extract_f0_mode

    def decode(self, acoustic_feature):
        import pyworld
        raise AssertionError('pyworld reached')


def _feature(n, fs, kind='glide'):
    from yukarin import AcousticFeature
    f0, sp, ap = C.case(kind, n, fs)
    f0 = f0.astype(numpy.float32)
    return AcousticFeature(f0=f0.reshape(-1, 1), sp=sp, ap=ap, voiced=f0.reshape(-1, 1) > 0)


def test_decode_many_on_the_reference_body(emu_ctx, monkeypatch):
    compat.install()
    from yukarin import Wave
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(Vocoder, 'decode', world_synth.decode)
    monkeypatch.setattr(Vocoder, 'decode_many', world_synth.decode_many, raising=False)
    for m in ('pyworld', 'world4py', 'world4py.native'):
        monkeypatch.setitem(sys.modules, m, None)
    fs = 24000
    feats = [_feature(7, fs), _feature(1, fs), _feature(12, fs, 'above')]
    many, one = Vocoder(_Param(), fs), Vocoder(_Param(), fs)
    assert many.decode_many([]) == [] and not hasattr(many, '_ry_synth')
    before = dict(world_synth.calls)
    waves = many.decode_many(feats)
    assert world_synth.calls == dict(before, packed=before['packed'] + 1)
    assert len(waves) == 3
    for w, f in zip(waves, feats):
        want = one.decode(f)
        assert isinstance(w, Wave) and w.sampling_rate == fs and w.wave.dtype == numpy.float64
        assert numpy.array_equal(w.wave, want.wave)
    assert numpy.array_equal(many.decode_many(iter(feats[:1]))[0].wave, waves[0].wave)
    many._ry_synth.close()
    one._ry_synth.close()
