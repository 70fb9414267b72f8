"""The batched WORLD synthesis (`Synthesizer.synthesize_many` / `ry_synth_run_many`) on the MI355X: every wave of every batched call against
`synthesize` of its item alone on a separate handle, bit for bit in the samples and the pulse lists.  The cases of the emulator suite at the same
smallest shapes, the kinds side by side at 300 frames, and the two that need the card: eight waves of seeded lengths, 2000 frames next to one.
Cases: tests/synth_many_cases.py."""
import numpy
import pytest

import synth_many_cases as M

pytestmark = pytest.mark.gpu

RATES = (16000, 24000)


@pytest.fixture(scope='module')
def rigs(gpu_ctx):
    r = {fs: M.Rig(gpu_ctx, fs) for fs in RATES}
    yield r
    for v in r.values():
        v.close()


@pytest.mark.parametrize('fs', RATES)
def test_one_wave_equals_synthesize(rigs, fs):
    M.check_batch(rigs[fs], M.glides(rigs[fs], [40]))


@pytest.mark.parametrize('fs', RATES)
def test_shortest_waves_and_their_reversal(rigs, fs):
    keyed = M.glides(rigs[fs], [1, 2, 5])
    out = M.check_batch(rigs[fs], keyed)
    assert len(out[0]) == 1
    M.check_batch(rigs[fs], keyed, order=[2, 1, 0])


@pytest.mark.parametrize('fs', RATES)
def test_either_side_of_a_scan_block_and_an_overlap_workgroup(rigs, fs):
    M.check_block_edges(rigs[fs])


@pytest.mark.parametrize('fs', RATES)
def test_kinds_side_by_side(rigs, fs):
    M.check_kinds(rigs[fs], 300)


@pytest.mark.parametrize('fs', RATES)
def test_a_loud_neighbour_moves_no_bit(rigs, fs):
    M.check_no_leak(rigs[fs])


@pytest.mark.parametrize('fs', RATES)
def test_noise_is_keyed_by_the_position_inside_the_wave(rigs, fs):
    M.check_noise_position(rigs[fs])


@pytest.mark.parametrize('fs', RATES)
def test_device_rows_in_place_and_mixed_lists(rigs, fs):
    M.check_device_rows(rigs[fs])


def test_poisoned_buffers_change_nothing(rigs):
    M.check_poison(rigs[16000])


def test_a_b_a_on_one_handle(rigs):
    M.check_aba(rigs[24000])


@pytest.mark.parametrize('fs', RATES)
def test_stream_after_and_around_a_batched_call(rigs, fs):
    M.check_stream(rigs[fs])


def test_eight_waves_of_seeded_lengths(rigs):
    frames = [int(n) for n in numpy.random.default_rng(18).integers(1, 401, 8)]
    assert len(frames) == 8 and min(frames) >= 1 and max(frames) <= 400
    M.check_batch(rigs[24000], M.glides(rigs[24000], frames))


@pytest.mark.parametrize('fs', RATES)
def test_a_long_wave_beside_a_single_sample(rigs, fs):
    keyed = M.glides(rigs[fs], [2000, 1])
    M.check_batch(rigs[fs], keyed)
    M.check_batch(rigs[fs], keyed, order=[1, 0])
