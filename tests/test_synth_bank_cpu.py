"""The bank of synthesis streams (`StreamBank` / `ry_synth_bank_*`) without a GPU, on the host-side SIMT emulator: after every call every stream
against a lone `Synthesizer` with its seed that got the same frames in the same cuts, bit for bit in the samples and the pulse lists; the refusals
of the C ABI; `create_synthesizer_many` / `decode_realtime_many` on the restated `RealtimeVocoder` body.  Tens of frames per stream -- the
emulator is slow.  Cases: tests/synth_bank_cases.py."""
import ctypes
import sys

import numpy
import pytest

import synth_bank_cases as K
import world_synth_cases as C
from realtime_yukarin_amd import _lib, compat, world_synth

_DP, _IP, _LP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)
RATES = (16000, 24000)


@pytest.mark.parametrize('fs', RATES)
def test_one_stream_in_cuts_of_1_1_2_5_31(emu_ctx, fs):
    K.check_one_stream(emu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_ragged_cuts_sit_outs_and_the_reversed_slot_order(emu_ctx, fs):
    K.check_ragged(emu_ctx, fs)


@pytest.mark.parametrize('target', K.TARGETS)
@pytest.mark.parametrize('fs', RATES)
def test_scan_starts_either_side_of_a_block_and_a_workgroup(emu_ctx, fs, target):
    K.check_scanned_edge(emu_ctx, fs, target)


@pytest.mark.parametrize('target', K.TARGETS)
@pytest.mark.parametrize('fs', RATES)
def test_emit_starts_either_side_of_a_block_and_a_workgroup(emu_ctx, fs, target):
    K.check_done_edge(emu_ctx, fs, target)


def test_kinds_side_by_side(emu_ctx):
    K.check_kinds(emu_ctx, 16000, 30)


@pytest.mark.parametrize('fs', RATES)
def test_a_stream_ends_and_its_slot_starts_again(emu_ctx, fs):
    K.check_end_and_restart(emu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_a_loud_neighbour_moves_no_bit(emu_ctx, fs):
    K.check_loud_neighbour(emu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_seeds_are_per_stream(emu_ctx, fs):
    K.check_seeds(emu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_poison_between_calls_changes_nothing(emu_ctx, fs):
    K.check_poison(emu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_device_rows_in_place_mixed_and_scattered(emu_ctx, fs):
    K.check_device_rows(emu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_cost_does_not_depend_on_the_number_of_streams(emu_ctx, fs):
    K.check_cost(emu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_the_window_does_not_grow_with_age(emu_ctx, fs):
    K.check_window_age(emu_ctx, fs)


def test_abi_refusals_change_nothing(emu_ctx):
    """Every refusal of ry_synth_bank_push: y and sample_offsets untouched, and the next valid push still has the yardstick's bits."""
    lib, d = emu_ctx.lib, emu_ctx.lib.dll
    fs, seeds = 16000, [5, 6, 7]
    rig = K.Rig(emu_ctx, fs, seeds)
    h = rig.bank._get()[1]
    tracks = [C.case(k, 40, fs) for k in ('glide', 'above', 'glide')]
    pos = [0]
    MARK = -7.25
    y = numpy.full(6000, MARK)
    off = numpy.full(4, -99, numpy.int64)

    def good():
        """A valid push of 2 more frames on every stream, through the rig."""
        a = pos[0]
        rig.push([tuple(x[a:a + 2] for x in t) for t in tracks])
        pos[0] += 2

    frames = [3, 4, 2]
    f0 = numpy.concatenate([C.f0_track('glide', n, fs) for n in frames])
    sp, ap = C.spectrogram(9), C.aperiodicity(9)

    def run(f0_=f0, sp_=sp, ap_=ap, n_=frames, fin_=None, bins=513, cap=6000, y_=y, off_=off, handle=h):
        n_ = None if n_ is None else numpy.asarray(n_, numpy.int32)
        fin_ = None if fin_ is None else numpy.asarray(fin_, numpy.int32)
        rc = d.ry_synth_bank_push(handle, None if f0_ is None else f0_.ctypes.data_as(_DP), None if sp_ is None else _lib._fptr(sp_),
                                  None if ap_ is None else _lib._fptr(ap_), None if n_ is None else n_.ctypes.data_as(_IP),
                                  None if fin_ is None else fin_.ctypes.data_as(_IP), bins, 0,
                                  None if y_ is None else y_.ctypes.data_as(_DP), cap, None if off_ is None else off_.ctypes.data_as(_LP))
        msg = d.ry_last_error()
        assert (y == MARK).all() and (off == -99).all()
        return rc, msg

    def refused(code=-1, has=None, **kw):
        rc, msg = run(**kw)
        assert rc == code and (has is None or has in msg), (rc, msg, kw)
        good()                                                              # the bank continues, bit-equal

    good()
    for null in ('f0_', 'sp_', 'ap_', 'n_', 'y_', 'off_'):
        refused(has=b'null', **{null: None})
    refused(n_=[3, -1, 2])
    refused(n_=[0, 0, 0], has=b'no stream')
    refused(n_=[0, 0, 0], fin_=[0, 0, 0], has=b'no stream')
    for bins in (512, 1025):
        refused(bins=bins, has=b'bins')
    for bad_value in (numpy.nan, numpy.inf, 8000.0):
        bad = f0.copy()
        bad[3 + 4 + 1] = bad_value                                          # stream 2 of 3, frame 1
        refused(f0_=bad, has=b'stream 2: f0[1]')
    need = sum(rig.bank.bound(b, frames[b], False) for b in range(3))
    assert need > 0
    refused(cap=need - 1, has=b'y holds')
    refused(n_=[1 << 22, 1, 0], has=b'frames')                              # totals, refused from the counts: the arrays are not read
    assert rig.ended == 0
    rig.flush_all()
    assert rig.ended == 3
    rc, msg = run(n_=[0, 0, 0], fin_=[0, 1, 0])                             # final on an empty stream
    assert rc == -4 and b'stream 1' in msg
    rig.close()
    # more pulse entries than one call indexes (2^30): 1 s frames at 48 kHz
    g = ctypes.c_void_p()
    sd = (ctypes.c_uint * 2)(1, 2)
    lib.check(d.ry_synth_bank_create(emu_ctx.handle, 48000, 1000.0, 1024, 2, sd, ctypes.byref(g)))
    rc, msg = run(n_=[12000, 12000], handle=g, cap=1 << 40)
    assert rc == -1 and b'samples' in msg
    d.ry_synth_bank_destroy(g)
    # create: the refusals of ry_synth_create, and at least one stream
    for args in ((7999, 5.0, 1024, 2), (16000, 0.0, 1024, 2), (16000, 5.0, 512, 2), (16000, 5.0, 1024, 0)):
        assert d.ry_synth_bank_create(emu_ctx.handle, args[0], args[1], args[2], args[3], sd, ctypes.byref(g)) == -1 and not g.value
    assert d.ry_synth_bank_create(emu_ctx.handle, 16000, 5.0, 1024, 2, None, ctypes.byref(g)) == -1
    assert d.ry_synth_bank_push(None, None, None, None, None, None, 513, 0, None, 0, None) == -4


def test_python_refusals(emu_ctx):
    bank = world_synth.StreamBank(16000, 5.0, n_streams=2, ctx=emu_ctx)
    f0, sp, ap = C.case('glide', 4, 16000)
    with pytest.raises(ValueError):
        bank.push([(f0, sp, ap)])
    with pytest.raises(ValueError):
        bank.push([None, None])
    with pytest.raises(ValueError):
        bank.push([(f0, sp[:3], ap), None])
    with pytest.raises(ValueError):
        bank.push([(f0, sp[:, :512], ap[:, :512]), None])
    with pytest.raises(ValueError):
        bank.push([(f0, sp, ap), None], final=[2])
    with pytest.raises(RuntimeError):
        bank.flush([1])
    with pytest.raises(ValueError):
        world_synth.StreamBank(16000, 5.0, n_streams=2, seeds=[1], ctx=emu_ctx)
    assert len(bank.push([(f0, sp, ap), None])[1]) == 0
    bank.close()


# ---- the reference's class, restated as tests/test_world_synth_cpu.py restates it (realtime_voice_conversion/yukarin_wrapper/vocoder.py:64-120) ----
class _Param(object):
    frame_period = 5.0


class RealtimeVocoder(object):
    def __init__(self, acoustic_param, out_sampling_rate, extract_f0_mode=None):
        self.acoustic_param = acoustic_param
        self.out_sampling_rate = out_sampling_rate
        self.extract_f0_mode = extract_f0_mode
        self._synthesizer = None

    def create_synthesizer(self, buffer_size, number_of_pointers):
        import world4py
        raise AssertionError('world4py reached')

    def decode(self, acoustic_feature):
        import world4py
        raise AssertionError('world4py reached')


def _feature(f0, sp, ap):
    from yukarin import AcousticFeature
    f0 = f0.astype(numpy.float32)
    return AcousticFeature(f0=f0.reshape(-1, 1), sp=sp, ap=ap, voiced=f0.reshape(-1, 1) > 0)


def test_drop_ins_on_the_reference_body(emu_ctx, monkeypatch):
    compat.install()
    from yukarin import Wave
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(RealtimeVocoder, 'create_synthesizer', world_synth.create_synthesizer)
    monkeypatch.setattr(RealtimeVocoder, 'decode', world_synth.decode_realtime)
    for m in ('pyworld', 'world4py', 'world4py.native'):
        monkeypatch.setitem(sys.modules, m, None)
    fs = 24000
    many = [RealtimeVocoder(_Param(), fs) for _ in range(3)]
    lone = [RealtimeVocoder(_Param(), fs) for _ in range(3)]
    bank = world_synth.create_synthesizer_many(many, 1024, 16)
    for v in lone:
        v.create_synthesizer(1024, 16)
    assert isinstance(bank, world_synth.StreamBank) and bank.n_streams == 3 and [v._synthesizer.slot for v in many] == [0, 1, 2]
    tracks = [K.cut(C.case(k, 30, fs), c) for k, c in (('glide', [9, 11, 10]), ('above', [12, 0, 18]), ('glide', [1, 20, 9]))]
    for call in range(3):
        feats = [None if t[call] is None else _feature(*t[call]) for t in tracks]
        before = dict(world_synth.calls)
        waves = world_synth.decode_realtime_many(many, feats)
        assert world_synth.calls == dict(before, bank_packed=before['bank_packed'] + 1)
        assert len(waves) == 3
        for w, f, v in zip(waves, feats, lone):
            assert isinstance(w, Wave) and w.sampling_rate == fs and w.wave.dtype == numpy.float64
            if f is None:                                                   # this vocoder sat the call out
                assert w.wave.size == 0
            else:
                assert numpy.array_equal(w.wave, v.decode(f).wave)
    # `decode` on a vocoder that holds a slot pushes that slot alone
    extra = _feature(*C.case('below', 6, fs))
    assert numpy.array_equal(many[1].decode(extra).wave, lone[1].decode(extra).wave)
    assert numpy.array_equal(many[1]._synthesizer.flush(), lone[1]._synthesizer.flush())
    with pytest.raises(ValueError):
        world_synth.decode_realtime_many(many + lone[:1], [None] * 4)
    with pytest.raises(ValueError):
        world_synth.create_synthesizer_many([RealtimeVocoder(_Param(), 16000), RealtimeVocoder(_Param(), 24000)], 1024, 16)
    bank.close()
    for v in lone:
        v._synthesizer.close()
