"""The output gate on the MI355X: the per-case mean_db / verdict / chunk-bit checks, split invariance, bank-equals-lone at B = 3, the inf and NaN rules
and the poison check -- the bodies of the emulator tests (output_gate_checks.py, where the measured tolerance is quoted) on the card.  The largest
shape is one chunk of 24000 samples."""
import numpy
import pytest

import output_gate_cases as C
import output_gate_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('dtype', [numpy.float64, numpy.float32])
@pytest.mark.parametrize('n', C.CHUNKS)
def test_cases_gpu(gpu_ctx, n, dtype):
    for name in C.SIGNALS:
        K.check_case(gpu_ctx, name, n, dtype)


@pytest.mark.parametrize('chunk', [1025, 2049])
def test_splits_gpu(gpu_ctx, chunk):
    K.check_splits(gpu_ctx, chunk, seeds=(1, 2, 3))


@pytest.mark.parametrize('poison', [False, True])
def test_bank_equals_lone_gates_gpu(gpu_ctx, poison):
    K.check_bank(gpu_ctx, 3, 1536, poison=poison)


def test_nan_and_inf_gpu(gpu_ctx):
    K.check_nonfinite(gpu_ctx, 2049)


def test_poison_gpu(gpu_ctx):
    K.check_poison(gpu_ctx, 1536)
