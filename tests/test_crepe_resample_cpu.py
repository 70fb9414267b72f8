"""The device resampler of the CREPE path without a GPU: `crepe_resample` on the host-side SIMT emulator, through the C ABI, `CrepeModel.resample`
/ `CrepeModel.predict` and the drop-in `crepe` module, bit for bit against the host function `crepe.resample` (case lists and checks:
tests/crepe_resample_cases.py)."""
import pytest

import crepe_resample_cases as rc


@pytest.fixture(scope='module')
def model(emu_ctx):
    m, P = rc.new_model(emu_ctx)
    yield m
    m.close()


@pytest.mark.parametrize('sr', rc.RATES)
def test_one_second_equals_the_host_function(model, sr):
    rc.check_exact(model, sr, sr)


@pytest.mark.parametrize('n,n_out', list(zip(rc.LENGTHS_24K, rc.OUTPUTS_24K)))
def test_lengths_at_24khz_equal_the_host_function(model, n, n_out):
    assert rc.crepe.resampled_length(n, 24000) == n_out
    rc.check_exact(model, 24000, n)


@pytest.mark.parametrize('sr', rc.RATES)
def test_short_signals_at_every_rate_equal_the_host_function(model, sr):
    assert rc.crepe.resampled_length(rc.SHORT[sr][0], sr) >= 1 and rc.crepe.resampled_length(rc.SHORT[sr][0] - 1, sr) == 0
    for n in rc.SHORT[sr]:
        rc.check_exact(model, sr, n)


@pytest.mark.parametrize('sr', rc.RATES)
def test_matches_the_per_sample_sinc_sum(model, sr):
    rc.check_restatement(model, sr)


def test_time_table_growth_and_rates_mixed_on_one_handle(emu_ctx):
    rc.check_growth_and_mixing(emu_ctx)


def test_poison_then_resample_and_predict(emu_ctx):
    rc.check_poison(emu_ctx)


@pytest.mark.parametrize('center,n,frames', rc.PREDICT_CASES)
def test_predict_at_24khz_equals_predict16k_of_the_host_resampled(model, center, n, frames):
    rc.check_predict(model, center, n, frames)


def test_predict_at_16khz_is_predict16k(model):
    rc.check_predict_16k_is_predict16k(model)


def test_on_device_pointers(model, emu_ctx):
    rc.check_on_device(model, emu_ctx)


def test_shim_resamples_on_the_device_unless_told_otherwise(emu_ctx, monkeypatch, tmp_path):
    model, P = rc.new_model(emu_ctx, 1, 4)
    try:
        rc.check_shim(monkeypatch, tmp_path, P, 1, model)
    finally:
        model.close()


def test_refusals(emu_ctx):
    rc.check_refusals(emu_ctx)
