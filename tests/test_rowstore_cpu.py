"""The row store without a GPU, on the host-side SIMT emulator: append, fetch and retire against the numpy model of the rings, bit for bit, and
every refusal by return code.  Cases and bodies: tests/rowstore_cases.py."""
import pytest

import rowstore_cases as C


@pytest.mark.parametrize('ap_cols', (1, 2))
def test_append_fetch_retire_equal_the_numpy_model(emu_ctx, ap_cols):
    C.check_store(emu_ctx, ap_cols)


@pytest.mark.parametrize('ap_cols', (1, 2))
def test_refusals_leave_the_store_unchanged(emu_ctx, ap_cols):
    C.check_refusals(emu_ctx, ap_cols)
