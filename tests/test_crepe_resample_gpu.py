"""The device resampler of the CREPE path on the MI355X: `crepe_resample` through the C ABI, `CrepeModel.resample` / `CrepeModel.predict` and the
drop-in `crepe` module, bit for bit against the host function `crepe.resample` (case lists and checks: tests/crepe_resample_cases.py; the same
cases as tests/test_crepe_resample_cpu.py at multiplier 1, and one call at full capacity through the shim)."""
import numpy
import pytest

import crepe_resample_cases as rc
from realtime_yukarin_amd import crepe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model(gpu_ctx):
    m, P = rc.new_model(gpu_ctx)
    yield m
    m.close()


@pytest.mark.parametrize('sr', rc.RATES)
def test_one_second_equals_the_host_function(model, sr):
    rc.check_exact(model, sr, sr)


@pytest.mark.parametrize('n,n_out', list(zip(rc.LENGTHS_24K, rc.OUTPUTS_24K)))
def test_lengths_at_24khz_equal_the_host_function(model, n, n_out):
    assert crepe.resampled_length(n, 24000) == n_out
    rc.check_exact(model, 24000, n)


@pytest.mark.parametrize('sr', rc.RATES)
def test_short_signals_at_every_rate_equal_the_host_function(model, sr):
    for n in rc.SHORT[sr]:
        rc.check_exact(model, sr, n)


@pytest.mark.parametrize('sr', rc.RATES)
def test_matches_the_per_sample_sinc_sum(model, sr):
    rc.check_restatement(model, sr)


def test_time_table_growth_and_rates_mixed_on_one_handle(gpu_ctx):
    rc.check_growth_and_mixing(gpu_ctx)


def test_poison_then_resample_and_predict(gpu_ctx):
    rc.check_poison(gpu_ctx)


@pytest.mark.parametrize('center,n,frames', rc.PREDICT_CASES)
def test_predict_at_24khz_equals_predict16k_of_the_host_resampled(model, center, n, frames):
    rc.check_predict(model, center, n, frames)


def test_predict_at_16khz_is_predict16k(model):
    rc.check_predict_16k_is_predict16k(model)


def test_on_device_pointers(model, gpu_ctx):
    rc.check_on_device(model, gpu_ctx)


def test_shim_resamples_on_the_device_unless_told_otherwise(gpu_ctx, monkeypatch, tmp_path):
    rc.check_shim(monkeypatch, tmp_path, crepe.synthetic_params(2, 4), 2)


def test_refusals(gpu_ctx):
    rc.check_refusals(gpu_ctx)


def test_full_capacity_half_second_at_24khz_through_the_shim(gpu_ctx, monkeypatch, tmp_path):
    """0.5 s at 24 kHz, `full` capacity, the reference's call: finite, and the bits of predict16k on the host-resampled signal."""
    from realtime_yukarin_amd.compat import crepe as shim
    P = crepe.synthetic_params('full', 1)
    path = tmp_path / 'crepe_full.npz'
    crepe.save_weights(path, P)
    monkeypatch.setenv('RY_CREPE_MODEL', str(path))
    monkeypatch.delenv('RY_CREPE_RESAMPLE', raising=False)
    monkeypatch.setattr(shim, '_weights', {})
    monkeypatch.setattr(shim, '_models', {})
    x, x16 = rc.case(24000, 12000)
    try:
        t, f0, conf, act = shim.predict(x, 24000, viterbi=True, model_capacity='full', step_size=5, verbose=0)
        assert act.shape == (101, 360) and numpy.isfinite(act).all() and numpy.isfinite(f0).all() and numpy.isfinite(conf).all()
        f0_m, conf_m, act_m = shim._models[32].predict16k(x16, rc.HOP)
        assert numpy.array_equal(act, act_m) and numpy.array_equal(conf, conf_m) and numpy.array_equal(f0, f0_m.astype(numpy.float64))
    finally:
        if 32 in shim._models:
            shim._models[32].close()
