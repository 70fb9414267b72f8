"""The silence gate's frame powers on the MI355X, pinned to the host's bits (gate_power_cases.py): the threshold sweep over every length and kind at
all four frame lengths, the 1027-frame wave, the tables of waves at fft 128 and 1024, the production thresholds at their boundary and around p_all,
and the NaN / inf rules on every gate entry.  The longest wave has 1027 frames; every other at most 24."""
import pytest

import gate_power_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('fft', C.FFTS)
def test_sweep_gpu(gpu_ctx, fft):
    calls = C.check_sweep(gpu_ctx, C.sweep_cases(fft), fft)
    print('fft %d: %d gate calls' % (fft, calls))
    assert calls > 500                          # a guard against a sweep that ran next to nothing


def test_sweep_long_wave_gpu(gpu_ctx):
    assert C.check_long(gpu_ctx) > 2000


@pytest.mark.parametrize('fft', [128, 1024])
def test_sweep_many_waves_gpu(gpu_ctx, fft):
    assert C.check_powers_many(gpu_ctx, fft) > 40


def test_threshold_boundary_gpu(gpu_ctx):
    assert C.check_threshold_boundary(gpu_ctx) == 5 * 65


def test_nonfinite_gpu(gpu_ctx):
    assert C.check_nonfinite(gpu_ctx) == 5
