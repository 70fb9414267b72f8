"""The CREPE kernels against float64, layer by layer and element by element, at every tile, split and pass edge (tests/crepe_cases.py).

Each conv layer and the dense layer are compared with the float64 restatement of THAT layer on the input the device itself read
(`debug_layer` of the same pass), within F32_TOL of the element's own bound, so one layer's error cannot hide behind the previous one's and a
wrong element in a low-magnitude channel cannot hide behind the largest one; the chained comparison with crepe_ref.network stays as a second,
end-to-end assertion.  `ry_crepe_debug_poison` fills everything a call must write with NaN patterns: a tile a launch skips shows as NaN instead
of the previous call's (usually right) value.  Exact properties (`numpy.array_equal`): a frame's results do not depend on its row, its tile, its
pass or the calls before it; device pointers give the host call's bits.  The decode runs on activations full of exact ties at the edges of its
prefetch and of the 384-thread cents loop.

The emulator part (no GPU) and the MI355X part run the same checks on their own case lists; `-s` prints every case's worst element-wise ratio
|y - r| / bound over all layers and the worst chained rel."""
import numpy
import pytest

import crepe_cases as cc
import crepe_ref
import cases
from conftest import rel_max
from realtime_yukarin_amd import crepe

HOP = 80
F32_TOL = cc.F32_TOL


def _params(m):
    return crepe.synthetic_params(m, 20 + m)


class Models(object):
    """one model per multiplier on one context, and the runs the tests share"""

    def __init__(self, ctx):
        self.ctx, self.models, self.runs = ctx, {}, {}

    def get(self, m):
        if m not in self.models:
            P = _params(m)
            self.models[m] = (crepe.CrepeModel(m, P, ctx=self.ctx), P)
        return self.models[m]

    def fresh(self, m):
        return crepe.CrepeModel(m, self.get(m)[1], ctx=self.ctx)

    def run(self, m, frames):
        """the (m, frames) case at hop 80, uncentred: computed once"""
        if (m, frames) not in self.runs:
            audio = cc.uncentred(frames, HOP, 100 * m + frames)
            self.runs[(m, frames)] = (audio, predict(self.get(m)[0], audio, HOP, False))
        return self.runs[(m, frames)]

    def close(self):
        for model, _ in self.models.values():
            model.close()


@pytest.fixture(scope='module')
def emu(emu_ctx):
    ms = Models(emu_ctx)
    yield ms
    ms.close()


@pytest.fixture(scope='module')
def gpu(gpu_ctx):
    ms = Models(gpu_ctx)
    yield ms
    ms.close()


def predict(model, audio, hop, center, rows=None):
    """One call and everything it left behind: f0, confidence, activation of every frame and the eight buffers of the last pass (`rows` of them;
    default the frames of that pass)."""
    f0, conf, act = model.predict16k(audio, hop, center=center)
    n = len(f0)
    last = n - (n - 1) // cc.CHUNK * cc.CHUNK
    return dict(f0=f0, conf=conf, act=act, n=n, last=last, layers=[model.debug_layer(i, rows or last) for i in range(8)])


def same_bits(a, b):
    """two runs: every output and every buffer bit for bit"""
    return (all(numpy.array_equal(a[k], b[k], equal_nan=True) for k in ('f0', 'conf', 'act')) and
            all(numpy.array_equal(x, y, equal_nan=True) for x, y in zip(a['layers'], b['layers'])))


def check_run(what, P, audio, hop, center, out):
    """Part 1 of the oracle: frames, every layer on the device's own input, the sigmoid, the chained reference, the decode."""
    fr = crepe_ref.frames(audio, hop, center)
    n, last = out['n'], out['last']
    off = n - last
    assert n == len(fr) == crepe.n_frames(len(audio), hop, center) and out['act'].shape == (n, 360), (what, n, len(fr))
    L = out['layers']
    # frames: one float32 rounding of the float64 value
    r0 = fr[off:]
    assert numpy.all(numpy.abs(L[0].astype(numpy.float64) - r0) <= 2.0 ** -24 * numpy.abs(r0) + 1e-12), (what, 'frames')
    worst = 0.0
    for i in range(6):
        r, bound = cc.layer_ref(P, i, L[i])
        worst = max(worst, cases.assert_close_elementwise(L[i + 1], r, bound, F32_TOL, '%s conv%d' % (what, i + 1)))
    r, bound = cc.dense_ref(P, L[6])
    worst = max(worst, cases.assert_close_elementwise(L[7], r, bound, F32_TOL, '%s dense' % what))
    act_err = float(numpy.abs(out['act'][off:] - cc.sigmoid64(L[7])).max())
    # the chain: the last pass's buffers against rows [off:] of the reference, the activation of every frame
    outs, logits, act_ref = crepe_ref.network(P, fr)
    rel = max([rel_max(L[i + 1], outs[i][off:]) for i in range(6)] + [rel_max(L[7], logits[off:])])
    chain_act = float(numpy.abs(out['act'] - act_ref).max())
    print('%-44s worst %.3g  rel %.3g  |act - sigmoid64| %.3g  |act - chain| %.3g' % (what, worst, rel, act_err, chain_act))
    assert act_err <= cc.ACT_TOL, (what, act_err)
    assert rel < cc.CHAIN_TOL and chain_act < cc.CHAIN_TOL, (what, rel, chain_act)
    # the decode of the device's own activation
    f0_ref, conf_ref, _ = crepe_ref.decode(out['act'], viterbi=True)
    assert numpy.array_equal(out['conf'], conf_ref), what
    assert numpy.allclose(out['f0'], f0_ref, rtol=1e-6, atol=0), what
    return worst


def check_case(ms, m, frames):
    model, P = ms.get(m)
    assert model.splits() == cc.splits(m), (m, model.splits(), cc.splits(m))
    audio, out = ms.run(m, frames)
    check_run('m %d, %d frames' % (m, frames), P, audio, HOP, False, out)


def check_poison(ms, m):
    """poison, then predict: finite, the unpoisoned bits; a shorter call leaves the rows behind it untouched"""
    model, _ = ms.get(m)
    audio, clean = ms.run(m, 17)
    model.poison()
    out = predict(model, audio, HOP, False)
    assert all(numpy.isfinite(out[k]).all() for k in ('f0', 'conf', 'act')) and all(numpy.isfinite(x).all() for x in out['layers']), m
    assert same_bits(out, clean), (m, 'a poisoned call differs from the clean one')
    model.poison()
    short = predict(model, audio[:crepe.FRAME + 2 * HOP], HOP, False, rows=17)
    assert short['n'] == 3
    assert numpy.isfinite(short['f0']).all()                          # (f0 follows the Viterbi path of the whole call: not compared)
    for k in ('conf', 'act'):
        assert numpy.array_equal(short[k], clean[k][:3]), (m, k)
    for i, (x, y) in enumerate(zip(short['layers'], clean['layers'])):
        assert numpy.array_equal(x[:3], y[:3]), (m, i, 'rows of the short call')
        assert numpy.isnan(x[3:]).all(), (m, i, 'the grid wrote rows behind M', int((~numpy.isnan(x[3:])).sum()))


def check_subwindows(ms, m, frames, windows):
    """every frame of a call on a sub-window cut at hop boundaries has the bits it has in the whole call"""
    model, _ = ms.get(m)
    audio, whole = ms.run(m, frames)
    for a, b in windows:                                              # frames [a, b)
        part = model.predict16k(audio[a * HOP:(b - 1) * HOP + crepe.FRAME], HOP, center=False)
        assert numpy.array_equal(part[2], whole['act'][a:b]) and numpy.array_equal(part[1], whole['conf'][a:b]), (m, frames, a, b)


def check_aba(ms, m, na, nbs):
    """A, calls of other lengths, A again on one handle: the bits of A on a fresh handle"""
    model = ms.fresh(m)
    fresh = ms.fresh(m)
    A = cc.uncentred(na, HOP, 7)
    first = predict(model, A, HOP, False)
    for j, nb in enumerate(nbs):
        model.predict16k(cc.uncentred(nb, HOP, 8 + j), HOP, center=False)
    again = predict(model, A, HOP, False)
    ref = predict(fresh, A, HOP, False)
    assert same_bits(first, ref) and same_bits(again, ref), (m, na, nbs)
    model.close(); fresh.close()


def check_on_device(ms, m, frames):
    """on_device = 1: audio and outputs in device buffers, the host call's bits"""
    from realtime_yukarin_amd import _lib
    model, _ = ms.get(m)
    ctx = ms.ctx
    audio = cc.uncentred(frames, HOP, 9)
    f0, conf, act = model.predict16k(audio, HOP, center=False)
    lib, h = model._get()
    bufs = [ctx.dev_alloc(n) for n in (audio.size, frames, frames, frames * 360)]
    try:
        ctx.dev_upload(bufs[0], audio)
        lib.check(lib.dll.ry_crepe_predict(h, _lib._fptr(bufs[0]), audio.size, HOP, 0, 1, _lib._fptr(bufs[1]), _lib._fptr(bufs[2]),
                                           _lib._fptr(bufs[3]), 1))
        ctx.sync()
        got = [numpy.empty(s, numpy.float32) for s in (frames, frames, (frames, 360))]
        for p, a in zip(bufs[1:], got):
            ctx.dev_download(p, a)
        ctx.sync()
    finally:
        for p in bufs:
            ctx.dev_free(p)
    assert numpy.array_equal(got[0], f0) and numpy.array_equal(got[1], conf) and numpy.array_equal(got[2], act), (m, frames)


def check_hop(ms, hop, center):
    model, P = ms.get(1)
    audio = cc.hop_case_signal(hop, center, 3 * hop + int(center))
    check_run('m 1, hop %d, center %s' % (hop, center), P, audio, hop, center, predict(model, audio, hop, center))


def check_decode(ms, n, viterbi, poison=False):
    model, _ = ms.get(1)
    a = cc.tie_activations(n, n)
    if n >= 4:
        a[n - 2] = 0                                                 # an all-zero row: argmax 0, 0 / 0 -> f0 = 0
    if poison:
        model.decode(a, viterbi=viterbi)                             # buffers of n frames exist
        model.poison()
    f0, conf, path = model.decode(a, viterbi=viterbi)
    f0_ref, conf_ref, path_ref = crepe_ref.decode(a, viterbi=viterbi)
    assert numpy.array_equal(path, path_ref), (n, viterbi)
    assert numpy.array_equal(conf, conf_ref), (n, viterbi)
    assert numpy.allclose(f0, f0_ref, rtol=1e-6, atol=0), (n, viterbi)
    if not viterbi:
        assert numpy.array_equal(path, numpy.argmax(a, axis=1))
        if n >= 4:
            assert f0[n - 2] == 0 and path[n - 2] == 0


def _id(c):
    return 'x'.join(str(v) for v in c)


# ---- the case lists ----

def test_crepe_cases_cover_every_branch():
    """The MI355X list reaches every tile / split / pass branch a multiplier and a frame count can reach (labels: crepe_cases.branches, a restatement
    of the planning code); the emulator list all but the three it names."""
    def union(cs):
        got = set()
        for c in cs:
            got |= cc.branches(*c)
        return got
    gpu_got, emu_got = union(cc.GPU_CASES), union(cc.EMU_CASES)
    assert not (gpu_got | emu_got) - cc.BRANCHES, sorted((gpu_got | emu_got) - cc.BRANCHES)
    assert not cc.BRANCHES - gpu_got, sorted(cc.BRANCHES - gpu_got)
    assert cc.BRANCHES - emu_got == cc.EMU_UNREACHED, sorted(cc.BRANCHES - emu_got)
    # the uneven split ranges of the full capacity: 2048 chunks / 5, 256 / 10, 512 / 20
    assert cc.splits(32) == [1, 5, 10, 16, 16, 20, 16]
    print('\n'.join(sorted(cc.BRANCHES)))


# ---- emulator ----

@pytest.mark.parametrize('case', cc.EMU_CASES, ids=_id)
def test_case_against_f64_emu(emu, case):
    check_case(emu, *case)


def test_poison_then_predict_emu(emu):
    check_poison(emu, 2)


def test_frames_do_not_depend_on_row_tile_or_pass_emu(emu):
    """frame 256 of the 257-frame call (row 0 of the second pass) alone (row 0 of a first pass) and as row 65 of a 66-frame call, whose other frames
    sit in the first pass of the whole call"""
    check_subwindows(emu, 1, 257, [(256, 257), (191, 257)])


def test_earlier_calls_leave_nothing_behind_emu(emu):
    check_aba(emu, 1, 5, (9, 2))


def test_on_device_pointers_emu(emu):
    check_on_device(emu, 1, 3)


@pytest.mark.parametrize('hop,center', cc.HOP_CASES)
def test_hop_and_center_emu(emu, hop, center):
    check_hop(emu, hop, center)


@pytest.mark.parametrize('viterbi', [True, False])
@pytest.mark.parametrize('n', cc.DECODE_FRAMES)
def test_decode_with_ties_emu(emu, n, viterbi):
    check_decode(emu, n, viterbi)


def test_decode_after_poison_emu(emu):
    check_decode(emu, 1000, True, poison=True)


# ---- MI355X ----

@pytest.mark.gpu
@pytest.mark.parametrize('case', cc.GPU_CASES, ids=_id)
def test_case_against_f64_gpu(gpu, case):
    check_case(gpu, *case)


@pytest.mark.gpu
@pytest.mark.parametrize('m', [2, 9])
def test_poison_then_predict_gpu(gpu, m):
    check_poison(gpu, m)


@pytest.mark.gpu
def test_frames_do_not_depend_on_row_tile_or_pass_gpu(gpu):
    """frame 512 of the 513-frame call (row 0 of the third pass) alone, as row 65 of a 66-frame call and as row 56 of the second pass of a
    313-frame call; every other frame of those calls too"""
    check_subwindows(gpu, 2, 513, [(512, 513), (447, 513), (200, 513), (0, 129)])


@pytest.mark.gpu
@pytest.mark.parametrize('m', [2, 9])
def test_earlier_calls_leave_nothing_behind_gpu(gpu, m):
    check_aba(gpu, m, 17, (40, 5))


@pytest.mark.gpu
@pytest.mark.parametrize('frames', [3, 257])
def test_on_device_pointers_gpu(gpu, frames):
    check_on_device(gpu, 2, frames)


@pytest.mark.gpu
@pytest.mark.parametrize('hop,center', cc.HOP_CASES)
def test_hop_and_center_gpu(gpu, hop, center):
    check_hop(gpu, hop, center)


@pytest.mark.gpu
@pytest.mark.parametrize('viterbi', [True, False])
@pytest.mark.parametrize('n', cc.DECODE_FRAMES)
def test_decode_with_ties_gpu(gpu, n, viterbi):
    check_decode(gpu, n, viterbi)


@pytest.mark.gpu
def test_decode_after_poison_gpu(gpu):
    check_decode(gpu, 1000, True, poison=True)
