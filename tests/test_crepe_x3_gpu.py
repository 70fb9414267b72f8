"""The split-bf16 mode of the CREPE network on the MI355X: the checks of tests/test_crepe_x3_cpu.py on the case list of the device
(tests/crepe_x3_cases.py: every tile, split and pass branch, multiplier 32 included).  The matrix instruction sums a K step in an order of its own,
so nothing here is compared with the numpy restatement bit for bit; every layer is held to float64 on the input it read, within the bars of
profiles/r14/crepe_x3_tolerance.txt.  `-s` prints every layer's worst ratio next to its bar."""
import pickle

import numpy
import pytest

import crepe_cases as cc
import crepe_x3_cases as xc
from test_crepe_oracle import check_aba, check_on_device, check_poison, check_subwindows, predict, same_bits
from test_crepe_x3_cpu import ModelsX3, check_sines
from realtime_yukarin_amd import crepe

HOP = xc.HOP
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu(gpu_ctx):
    ms = ModelsX3(gpu_ctx)
    yield ms
    ms.close()


@pytest.mark.parametrize('case', xc.GPU_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_case_against_f64_gpu(gpu, case):
    xc.check_case(gpu, case[0], case[1], predict)


@pytest.mark.parametrize('m', [2, 9])
def test_poison_then_predict_gpu(gpu, m):
    check_poison(gpu, m)


def test_frames_do_not_depend_on_row_tile_or_pass_gpu(gpu):
    """frame 256 of the 257-frame call (row 0 of the second pass) alone, as row 65 of a 66-frame call; frames of the first pass in shorter calls"""
    check_subwindows(gpu, 2, 257, [(256, 257), (191, 257), (100, 257), (0, 129)])


@pytest.mark.parametrize('m', [2, 9])
def test_earlier_calls_leave_nothing_behind_gpu(gpu, m):
    check_aba(gpu, m, 17, (40, 5))


@pytest.mark.parametrize('frames', [3, 257])
def test_on_device_pointers_gpu(gpu, frames):
    check_on_device(gpu, 2, frames)


def test_switching_back_gives_the_fp32_bits_gpu(gpu, gpu_ctx):
    P = xc.params(9)
    audio = cc.uncentred(17, HOP, 3)
    never = crepe.CrepeModel(9, P, ctx=gpu_ctx)
    model = crepe.CrepeModel(9, P, ctx=gpu_ctx)
    ref = predict(never, audio, HOP, False)
    assert same_bits(predict(model, audio, HOP, False), ref) and model.splits() == cc.splits(9)
    model.set_dtype('bf16x3')
    assert model.splits() == xc.splits(9)
    mode = predict(model, audio, HOP, False)
    assert not numpy.array_equal(mode['layers'][7], ref['layers'][7])
    d = float(numpy.abs(mode['act'].astype('f8') - ref['act']).max())
    print('m 9, 17 frames: |act_x3 - act_f32| %.3g  bar %.3g' % (d, xc.bars()['act']))
    assert d <= xc.bars()['act']
    model.set_dtype('f32')
    assert same_bits(predict(model, audio, HOP, False), ref)
    never.close(); model.close()


def test_mode_against_the_fp32_path_on_sines_gpu(gpu, gpu_ctx):
    model, P = gpu.get(xc.SINE_M)
    f32 = crepe.CrepeModel(xc.SINE_M, P, ctx=gpu_ctx)
    check_sines(model, f32, xc.SINES)
    f32.close()


def test_predict_at_24k_equals_predict16k_of_the_resampled_signal_gpu(gpu):
    model, _ = gpu.get(2)
    x = cc.signal(24000 * (crepe.FRAME + 16 * HOP) // 16000 + 8, 5)
    a = model.predict(x, 24000, HOP, center=False)
    b = model.predict16k(model.resample(x, 24000), HOP, center=False)
    assert len(a[0]) >= 17 and all(numpy.array_equal(u, v) for u, v in zip(a, b))


def test_pickled_model_keeps_the_mode_gpu(gpu_ctx):
    """a pickled and restored model creates its handle in the mode (the product's context of this process)"""
    P = xc.params(2)
    model = crepe.CrepeModel(2, P, dtype='bf16x3')
    audio = cc.uncentred(3, HOP, 4)
    ref = model.predict16k(audio, HOP, center=False)
    copy = pickle.loads(pickle.dumps(model))
    assert copy.dtype == 'bf16x3' and copy._handle is None
    assert copy.splits() == xc.splits(2)
    assert all(numpy.array_equal(u, v) for u, v in zip(copy.predict16k(audio, HOP, center=False), ref))
    model.close(); copy.close()


def test_refusals_gpu(gpu):
    model, _ = gpu.get(2)
    lib, h = model._get()
    for bad in (1, 3, -1):
        assert lib.dll.ry_crepe_set_dtype(h, bad) == -1 and 'dtype %d' % bad in lib.dll.ry_last_error().decode()
    assert model.splits() == xc.splits(2)
