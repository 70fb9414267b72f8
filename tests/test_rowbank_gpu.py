"""The row bank on the MI355X: the emulator cases again -- append, fetch, the masked pick of ap rows and retire for three streams against one
numpy model of the rings per stream and against a lone `RowStore` per stream, bit for bit, the counts per call and every refusal by return
code.  Cases and bodies: tests/rowbank_cases.py."""
import pytest

import rowbank_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('ap_cols', (1, 2))
def test_append_fetch_pick_retire_equal_the_numpy_models(gpu_ctx, ap_cols):
    C.check_bank(gpu_ctx, ap_cols)


@pytest.mark.parametrize('ap_cols', (1, 2))
def test_refusals_leave_the_bank_unchanged(gpu_ctx, ap_cols):
    C.check_refusals(gpu_ctx, ap_cols)
