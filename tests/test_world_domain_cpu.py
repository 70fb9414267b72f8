"""The WORLD kernels (synth_kernels.h, analysis_kernels.h, d4c_kernels.h) at the edges of the domain the C ABI accepts, on the host-side SIMT
emulator: the longest windows (1021 samples in CheapTrick, 2043 in D4C), f0 up to fs / 2 (the clamp of L, the widest mirror of the smoothing),
frame times off the grid, negative, at -1 s and at 1e6 s, every rate from 8 to 48 kHz, orders 0 .. 63 and alpha -0.9 .. 0.9 of the mel-cepstrum,
q1 and f0_floor at their bounds, and synthesis at frame periods whose samples per frame are not whole numbers, down to one sample per frame.
The bodies and the bars: tests/world_domain_checks.py; the inputs: tests/world_domain_cases.py, vetted by tests/test_world_*_ref.py.
tests/test_world_domain_gpu.py runs the same bodies on the MI355X."""
import pytest

import world_domain_cases as C
import world_domain_checks as K

FRAMES, SYNTH_FRAMES = C.FRAMES_EMU, C.SYNTH_FRAMES_EMU
GROW_ANALYSIS, GROW_SYNTH = 40, 60


@pytest.fixture
def ctx(emu_ctx):
    return emu_ctx


def test_refusals_at_the_bounds(ctx):
    K.refusals(ctx)


@pytest.mark.parametrize('n', FRAMES)
@pytest.mark.parametrize('tk', C.TRACKS)
@pytest.mark.parametrize('wk', C.WAVES)
@pytest.mark.parametrize('fs', C.RATES)
def test_cheaptrick(ctx, fs, wk, tk, n):
    K.cheaptrick_case(ctx, wk, tk, n, fs)


@pytest.mark.parametrize('q1', C.Q1)
def test_cheaptrick_q1(ctx, q1):
    import world_analysis_cases as A
    K.cheaptrick(ctx, 'glide', 'glide', FRAMES[-1], 16000, q1=q1, inputs=A.case('glide', 'glide', FRAMES[-1], 16000))


@pytest.mark.parametrize('floor', C.FLOORS)
def test_cheaptrick_f0_floor(ctx, floor):
    import world_analysis_cases as A
    K.cheaptrick(ctx, 'glide', 'glide', FRAMES[-1], 16000, floor=floor, inputs=A.case('glide', 'glide', FRAMES[-1], 16000))


@pytest.mark.parametrize('alpha', C.ALPHAS)
@pytest.mark.parametrize('order', C.ORDERS)
def test_sp2mc(ctx, order, alpha):
    K.sp2mc(ctx, order, alpha)


@pytest.mark.parametrize('n', FRAMES)
@pytest.mark.parametrize('tk', C.D4C_TRACKS)
@pytest.mark.parametrize('wk', C.WAVES)
@pytest.mark.parametrize('fs', C.D4C_RATES)
def test_d4c(ctx, fs, wk, tk, n):
    K.d4c_case(ctx, wk, tk, n, fs)


@pytest.mark.parametrize('tk,fs,d4c', [('lowest', 24000, True), ('high', 16000, True), ('lowest47', 24000, True), ('high', 48000, False), ('offgrid', 8000, False)])
def test_rows_do_not_depend_on_the_batch(ctx, tk, fs, d4c):
    K.permutation(ctx, tk, fs, FRAMES[-1], d4c)


@pytest.mark.parametrize('fs', C.D4C_RATES)
def test_poisoned_analysis(ctx, fs):
    K.poisoned_analysis(ctx, fs, GROW_ANALYSIS)


@pytest.mark.parametrize('n', SYNTH_FRAMES)
@pytest.mark.parametrize('kind', C.SYNTH_TRACKS)
@pytest.mark.parametrize('fs,fp', C.CONFIGS)
def test_synthesis(ctx, fs, fp, kind, n):
    K.synth_case(ctx, fs, fp, kind, n)


@pytest.mark.parametrize('fs,fp', C.CONFIGS)
def test_stream_equals_one_shot_bit_for_bit(ctx, fs, fp):
    K.synth_stream(ctx, fs, fp, SYNTH_FRAMES[-1])


def test_poisoned_synthesis(ctx):
    K.poisoned_synth(ctx, SYNTH_FRAMES[-1], GROW_SYNTH)
