"""The row store on the MI355X: the emulator cases again -- append, fetch and retire against the numpy model of the rings, bit for bit, and every
refusal by return code.  Cases and bodies: tests/rowstore_cases.py."""
import pytest

import rowstore_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('ap_cols', (1, 2))
def test_append_fetch_retire_equal_the_numpy_model(gpu_ctx, ap_cols):
    C.check_store(gpu_ctx, ap_cols)


@pytest.mark.parametrize('ap_cols', (1, 2))
def test_refusals_leave_the_store_unchanged(gpu_ctx, ap_cols):
    C.check_refusals(gpu_ctx, ap_cols)
