"""The split-bf16 mode of the CREPE network (`CrepeModel.set_dtype('bf16x3')`) on the host emulator: every layer against float64 on the input the
kernel itself read, within the bars of profiles/r14/crepe_x3_tolerance.txt (tests/crepe_x3_cases.py says where they come from); the kernel against
the numpy restatement bit for bit (the emulated matrix instruction adds its 16 products one by one, as the restatement does: this is what sees a
split that truncates, which the float64 bars cannot -- 2.7e-6 against a bar of 6.8e-6); the exact properties of the fp32 path in the mode; the
switch, its refusals and its way through pickling and the drop-in module.  `-s` prints every layer's worst ratio next to its bar."""
import pickle

import numpy
import pytest

import crepe_cases as cc
import crepe_ref
import crepe_x3_cases as xc
from test_crepe_oracle import Models, check_aba, check_on_device, check_poison, check_subwindows, predict, same_bits
from realtime_yukarin_amd import crepe

HOP = xc.HOP
RY_EINVAL = -1                  # include/ry355.h


class ModelsX3(Models):
    """the models of test_crepe_oracle.py, in the mode"""

    def get(self, m):
        if m not in self.models:
            P = xc.params(m)
            self.models[m] = (crepe.CrepeModel(m, P, ctx=self.ctx, dtype='bf16x3'), P)
        return self.models[m]

    def fresh(self, m):
        return crepe.CrepeModel(m, self.get(m)[1], ctx=self.ctx, dtype='bf16x3')


@pytest.fixture(scope='module')
def emu(emu_ctx):
    ms = ModelsX3(emu_ctx)
    yield ms
    ms.close()


def _id(c):
    return 'x'.join(str(v) for v in c)


def test_x3_cases_cover_every_branch():
    """the MI355X list reaches every label of crepe_cases.BRANCHES in the mode's own plan; the emulator list all but the ones it names"""
    union = lambda cs: set().union(*[xc.branches(*c) for c in cs])
    gpu_got, emu_got = union(xc.GPU_CASES), union(xc.EMU_CASES)
    assert not (gpu_got | emu_got) - cc.BRANCHES, sorted((gpu_got | emu_got) - cc.BRANCHES)
    assert not cc.BRANCHES - gpu_got, sorted(cc.BRANCHES - gpu_got)
    assert cc.BRANCHES - emu_got == xc.EMU_UNREACHED, sorted((cc.BRANCHES - emu_got) ^ xc.EMU_UNREACHED)
    assert xc.splits(32) == [1, 5, 10, 16, 16, 20, 16] and xc.splits(4) == [1, 5, 2, 2, 2, 4, 2]
    # uneven ranges in chunks of 64 at full capacity: 1024 / 5, 128 / 10, 256 / 20; at multiplier 4: 128 / 5
    assert 'uneven split' in xc.branches(32, 1) and 'uneven split' in xc.branches(4, 1)


def test_bars_file_is_what_the_script_derives():
    """the committed bars: 4 x the worst ratio of the restatement, below the one-product ceiling except where the file says otherwise; both cross-term
    mutants above the bar for conv1, a middle conv and the dense layer; the restatement of one case recomputed here gives the file's row"""
    text = xc.BARS_FILE.read_text().splitlines()
    val = lambda key: float([l for l in text if l.startswith(key + ' =')][0].split()[-1])
    B = xc.bars()
    for n in xc.NAMES:
        assert B[n] == pytest.approx(4 * val('worst ' + n), rel=1e-6) and B[n] < 2 * xc.SANITY_CEILING, n
    for label in ('without lo hi', 'without hi lo'):
        assert [l for l in text if l.startswith('condition ' + label)][0].endswith('= met')
        for layer in ('conv1', 'conv4', 'dense'):
            rows = [l.split() for l in text if l.startswith('mutant %-6s %s' % (layer, label))]
            assert rows and any(float(r[-3]) > B[layer] for r in rows), (layer, label)
    P, fr = xc.params(1), xc.frames32(1, 1)
    L = xc.network_x3(P, 1, fr)
    row = [l for l in text if l.startswith('m 1, 1 frames')][0].split()
    for i in range(7):
        r, bound = xc.conv_exact(P, i, L[i]) if i < 6 else cc.dense_ref(P, L[6])
        got = float((numpy.abs(L[i + 1].astype('f8') - r) / bound).max())
        assert got == pytest.approx(float(row[5 + 2 * i]), rel=1e-3), (i, got, row)
        if i < 6:                                                   # the numpy float64 statement is the torch one of crepe_cases
            rt, bt = cc.layer_ref(P, i, L[i])
            assert numpy.allclose(r, rt, rtol=0, atol=1e-9 * float(bt.max())) and numpy.allclose(bound, bt, rtol=1e-6)


def test_argmax_margin_of_the_sine_signals_exceeds_the_activation_bar():
    """the f0 test may ask for the same path only if no frame's two highest bins are within twice the activation bar (float64 chain, CPU)"""
    P = xc.params(xc.SINE_M)
    for f in xc.SINES:
        act = crepe_ref.network(P, crepe_ref.frames(xc.sine(f, xc.SINE_FRAMES), HOP, False))[2]
        top = numpy.sort(act, axis=1)
        margin = float((top[:, -1] - top[:, -2]).min())
        print('sine %g Hz: argmax margin %.3g, activation bar %.3g' % (f, margin, xc.bars()['act']))
        assert margin > 2 * xc.bars()['act'], (f, margin)


@pytest.mark.parametrize('case', xc.EMU_CASES, ids=_id)
def test_case_against_f64_emu(emu, case):
    xc.check_case(emu, case[0], case[1], predict)


@pytest.mark.parametrize('case', [(1, 1), (4, 1)], ids=_id)
def test_kernel_equals_the_restatement_bit_for_bit_emu(emu, case):
    """every buffer of the call is the numpy restatement's, bit for bit: the split (RNE, both parts), the three products and their order, the chunk and
    split ranges, the reduce and the epilogue"""
    m, frames = case
    model, P = emu.get(m)
    _, out = emu.run(m, frames)
    L = out['layers']
    sp = xc.splits(m)
    for i in range(6):
        assert numpy.array_equal(L[i + 1], xc.conv_x3(P, i, L[i], sp[i])), (case, cc.NAMES[i])
    assert numpy.array_equal(L[7], xc.dense_x3(P, L[6], sp[6])), (case, 'dense')


def test_poison_then_predict_emu(emu):
    check_poison(emu, 1)


def test_frames_do_not_depend_on_row_or_call_length_emu(emu):
    """frames 1 and 2 of the three-frame call alone and as a pair: other rows of the tiles, the bits of the whole call"""
    check_subwindows(emu, 1, 3, [(2, 3), (1, 3), (0, 1)])


def test_earlier_calls_leave_nothing_behind_emu(emu):
    check_aba(emu, 1, 2, (3, 1))


def test_on_device_pointers_emu(emu):
    check_on_device(emu, 1, 2)


def test_switching_back_gives_the_fp32_bits_emu(emu, emu_ctx):
    """f32 -> bf16x3 -> f32 on one handle: the bits of a handle that never switched; the mode itself differs, within the activation bar"""
    P = xc.params(1)
    audio = cc.uncentred(2, HOP, 3)
    never = crepe.CrepeModel(1, P, ctx=emu_ctx)
    model = crepe.CrepeModel(1, P, ctx=emu_ctx)
    ref = predict(never, audio, HOP, False)
    assert same_bits(predict(model, audio, HOP, False), ref)
    assert model.splits() == cc.splits(1)
    model.set_dtype('bf16x3')
    assert model.splits() == xc.splits(1)
    mode = predict(model, audio, HOP, False)
    assert not numpy.array_equal(mode['layers'][7], ref['layers'][7])
    assert float(numpy.abs(mode['act'].astype('f8') - ref['act']).max()) <= xc.bars()['act']
    model.set_dtype('f32')
    assert same_bits(predict(model, audio, HOP, False), ref)
    never.close(); model.close()


def test_mode_against_the_fp32_path_on_sines_emu(emu, emu_ctx):
    """activation within the bar; the same Viterbi path and f0 within what the bar allows the cents average"""
    model, P = emu.get(xc.SINE_M)
    f32 = crepe.CrepeModel(xc.SINE_M, P, ctx=emu_ctx)
    check_sines(model, f32, xc.SINES[:1])
    f32.close()


def check_sines(model_x3, model_f32, freqs):
    B = xc.bars()
    for f in freqs:
        audio = xc.sine(f, xc.SINE_FRAMES)
        a, b = xc.check_against_f32(model_x3, model_f32, audio, 'm %d, sine %g Hz' % (xc.SINE_M, f))
        pa = model_x3.decode(a[2])[2]
        pb = model_f32.decode(b[2])[2]
        assert numpy.array_equal(pa, pb), (f, pa, pb)
        rel = numpy.abs(a[0].astype('f8') / b[0] - 1)
        assert numpy.all(rel <= xc.f0_allowance(b[2], pb, B['act'])), (f, rel, xc.f0_allowance(b[2], pb, B['act']))


def test_predict_at_24k_equals_predict16k_of_the_resampled_signal_emu(emu):
    model, _ = emu.get(1)
    x = cc.signal(24000 * (crepe.FRAME + HOP) // 16000 + 8, 5)
    a = model.predict(x, 24000, HOP, center=False)
    b = model.predict16k(model.resample(x, 24000), HOP, center=False)
    assert len(a[0]) >= 2 and all(numpy.array_equal(u, v) for u, v in zip(a, b))


def test_pickled_model_keeps_the_mode(emu_ctx):
    """the dtype travels with the object; the handle of the copy is created in the mode (here over the emulator context it is given again)"""
    P = xc.params(1)
    model = crepe.CrepeModel(1, P, ctx=emu_ctx, dtype='bf16x3')
    audio = cc.uncentred(1, HOP, 4)
    ref = model.predict16k(audio, HOP, center=False)
    copy = pickle.loads(pickle.dumps(model))
    assert copy.dtype == 'bf16x3' and copy._handle is None
    copy._given_ctx = emu_ctx
    assert copy.splits() == xc.splits(1)
    got = copy.predict16k(audio, HOP, center=False)
    assert all(numpy.array_equal(u, v) for u, v in zip(got, ref))
    f32 = pickle.loads(pickle.dumps(crepe.CrepeModel(1, P, ctx=emu_ctx)))
    assert f32.dtype == 'f32'
    model.close(); copy.close()


def test_refusals(emu_ctx, monkeypatch):
    """dtype 1, 3 and -1 are refused and leave the handle as it was; unknown names and a bad RY_CREPE_DTYPE are refused"""
    P = xc.params(1)
    model = crepe.CrepeModel(1, P, ctx=emu_ctx, dtype='bf16x3')
    lib, h = model._get()
    audio = cc.uncentred(1, HOP, 6)
    ref = model.predict16k(audio, HOP, center=False)
    for bad in (1, 3, -1):
        assert lib.dll.ry_crepe_set_dtype(h, bad) == RY_EINVAL
        assert 'dtype %d' % bad in lib.dll.ry_last_error().decode()
        assert model.splits() == xc.splits(1)
        assert all(numpy.array_equal(u, v) for u, v in zip(model.predict16k(audio, HOP, center=False), ref))
    assert lib.dll.ry_crepe_set_dtype(None, 2) != 0
    for bad in ('bf16', 'fp32', None):
        with pytest.raises(ValueError):
            model.set_dtype(bad)
        with pytest.raises(ValueError):
            crepe.CrepeModel(1, P, ctx=emu_ctx, dtype=bad)
    assert model.dtype == 'bf16x3'
    model.close()
    from realtime_yukarin_amd.compat import crepe as shim
    monkeypatch.setitem(shim._weights, 1, P)
    monkeypatch.setattr(shim, '_models', {})
    monkeypatch.setenv('RY_CREPE_DTYPE', 'bf16')
    with pytest.raises(RuntimeError, match='RY_CREPE_DTYPE'):
        shim._model(1)
    monkeypatch.setenv('RY_CREPE_DTYPE', 'bf16x3')
    assert shim._model(1).dtype == 'bf16x3'
    shim._models.clear()
    monkeypatch.delenv('RY_CREPE_DTYPE')
    assert shim._model(1).dtype == 'f32'
