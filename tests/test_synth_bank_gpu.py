"""The bank of synthesis streams (`StreamBank` / `ry_synth_bank_*`) on the MI355X: after every call every stream against a lone `Synthesizer`
with its seed that got the same frames in the same cuts, bit for bit in the samples and the pulse lists.  The cases of the emulator suite at the
same smallest shapes, the kinds side by side at 300 frames per push, and the three that need the card: eight streams of seeded ragged cuts, 2000
frames beside one, A-B-A around a reset.  Cases: tests/synth_bank_cases.py."""
import numpy
import pytest

import synth_bank_cases as K
import world_synth_cases as C

pytestmark = pytest.mark.gpu

RATES = (16000, 24000)


@pytest.mark.parametrize('fs', RATES)
def test_one_stream_in_cuts_of_1_1_2_5_31(gpu_ctx, fs):
    K.check_one_stream(gpu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_ragged_cuts_sit_outs_and_the_reversed_slot_order(gpu_ctx, fs):
    K.check_ragged(gpu_ctx, fs)


@pytest.mark.parametrize('target', K.TARGETS)
@pytest.mark.parametrize('fs', RATES)
def test_scan_starts_either_side_of_a_block_and_a_workgroup(gpu_ctx, fs, target):
    K.check_scanned_edge(gpu_ctx, fs, target)


@pytest.mark.parametrize('target', K.TARGETS)
@pytest.mark.parametrize('fs', RATES)
def test_emit_starts_either_side_of_a_block_and_a_workgroup(gpu_ctx, fs, target):
    K.check_done_edge(gpu_ctx, fs, target)


@pytest.mark.parametrize('fs', RATES)
def test_kinds_side_by_side(gpu_ctx, fs):
    K.check_kinds(gpu_ctx, fs, 300)


@pytest.mark.parametrize('fs', RATES)
def test_a_stream_ends_and_its_slot_starts_again(gpu_ctx, fs):
    K.check_end_and_restart(gpu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_a_loud_neighbour_moves_no_bit(gpu_ctx, fs):
    K.check_loud_neighbour(gpu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_seeds_are_per_stream(gpu_ctx, fs):
    K.check_seeds(gpu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_poison_between_calls_changes_nothing(gpu_ctx, fs):
    K.check_poison(gpu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_device_rows_in_place_mixed_and_scattered(gpu_ctx, fs):
    K.check_device_rows(gpu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_cost_does_not_depend_on_the_number_of_streams(gpu_ctx, fs):
    K.check_cost(gpu_ctx, fs)


@pytest.mark.parametrize('fs', RATES)
def test_the_window_does_not_grow_with_age(gpu_ctx, fs):
    K.check_window_age(gpu_ctx, fs)


def test_eight_streams_of_seeded_ragged_cuts(gpu_ctx):
    rng = numpy.random.default_rng(19)
    cuts = [[int(n) for n in rng.integers(1, 121, 6)] for _ in range(8)]
    assert all(1 <= n <= 120 for c in cuts for n in c)
    rig = K.Rig(gpu_ctx, 24000, list(range(8)))
    try:
        K.run_cuts(rig, [C.TRACKS[b % len(C.TRACKS)] for b in range(8)], cuts)
        assert rig.ended == 8
    finally:
        rig.close()


@pytest.mark.parametrize('fs', RATES)
def test_2000_frames_beside_one(gpu_ctx, fs):
    rig = K.Rig(gpu_ctx, fs, [1, 2])
    try:
        K.run_cuts(rig, ['glide', 'glide'], [[2000, 7], [1, 7]])
        assert rig.ended == 2
    finally:
        rig.close()


def test_a_b_a_around_a_reset(gpu_ctx):
    rig = K.Rig(gpu_ctx, 16000, [5, 6, 7])
    try:
        pieces = [K.cut(C.case(k, 60, 16000), c) for k, c in (('glide', [25, 35]), ('above', [40, 20]), ('unvoiced', [3, 57]))]
        first = [rig.push([p[call] for p in pieces]) for call in range(2)]
        rig.bank.reset()
        for s in rig.lone:
            s.reset()
        rig.frames, rig.out = [[] for _ in range(3)], [[] for _ in range(3)]
        again = [rig.push([p[call] for p in pieces]) for call in range(2)]
        assert all(numpy.array_equal(a, b) for x, y in zip(first, again) for a, b in zip(x, y))
        rig.flush_all()
        assert rig.ended == 3
    finally:
        rig.close()
