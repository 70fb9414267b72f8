"""The silence gate's frame powers pinned to the host's bits by threshold sweeps, the production thresholds at their boundary and the NaN / inf
rules, on the emulator (the bodies are in gate_power_cases.py); the conditions on the reference and on the inputs, which need no kernel.

The emulator runs a 1024-fiber workgroup per gate call, so it takes a subset: the full sweep for fft 128 and 1024 (one leaf, and all three levels of
the tree over the leaves) on lengths 37, fft / 2 and 700 with the kinds `wide`, `subnormal` and `overflow` and the hop-1 wave, one table of waves, the boundary check
at 60 dB, and every non-finite case.  Left to the card (test_gate_power_gpu.py): fft 256 and 512, the other five kinds and five lengths, the
1027-frame wave that ends ragged on the four-frames-per-workgroup grid, the table at fft 1024, the boundary at 20, 80 and 100 dB and around p_all --
and what only the card can show: how ITS compiler rounds the products and sums, divides, takes the square root and treats subnormals."""
import pytest

import gate_power_cases as C


def test_cases_tell_the_orders_apart():
    """The faithful restatement of the kernel's stated order equals the host on every case (subnormal and overflowing included), and each wrong order
    differs from the host in at least one frame at every frame length at which it can: the sweep over these cases would catch it."""
    differ = C.orders_told_apart()
    for variant, by_fft in differ.items():
        for fft, frames in by_fft.items():
            if variant == 'leaves_in_sequence' and fft < 512:      # one or two leaves: the sequence IS the tree
                assert frames == 0
            else:
                assert frames > 0, (variant, fft)


def test_host_powers_lie_within_24_roundings_of_float64():
    held, worst = C.check_reference_against_float64()
    print('host powers against the float64 mean of squares: %d cases, largest error %.2f x 2^-24 (bound 24)' % (held, worst))
    assert held >= 5 * 8 * len(C.FFTS)


def test_the_last_frame_case_is_what_it_says():
    C.last_frame_case()


@pytest.mark.parametrize('fft', [128, 1024])
def test_sweep_emu(emu_ctx, fft):
    assert C.check_sweep(emu_ctx, C.emulator_cases(fft), fft) > 60


def test_sweep_many_waves_emu(emu_ctx):
    assert C.check_powers_many(emu_ctx, 128) > 40


def test_threshold_boundary_emu(emu_ctx):
    assert C.check_threshold_boundary(emu_ctx, thrs=(60,), clamp=False) == 65


def test_nonfinite_emu(emu_ctx):
    assert C.check_nonfinite(emu_ctx) == 5
