"""What tests/test_window_call_gpu.py compares against: `plain`, the window call with no state to get wrong -- a predictor pair created
under RY_GRAPH=0 (no captured graph, so nothing is ever replayed), one lane, no discard, every window alone through submit + wait (so
nothing else is ever in flight) -- and the CPU oracle of the chain that `plain` itself is held to (torch_ref CNNs + oracle/mc2sp.py, as
`_chained_oracle` of test_gpu_parity.py), so that the code under test is never compared with itself only.  Plus the small things every
scenario needs: windows, device blocks, the no-op guard and the message of a mismatch."""
import contextlib
import os

import numpy

import cases
from conftest import rel_max
from oracle import effective_frame as oef
from oracle import mc2sp as omc
from oracle import torch_ref
from realtime_yukarin_amd import engine, gate, sptk, synth
from realtime_yukarin_amd.weights import flatten_params

FS, FP, HOP = 16000, 5, 80
FFTLEN = {'SYN-8': 256, 'SYN-64': 1024}            # spectrogram bins = fftlen / 2 + 1 (129: the small chain of test_vc_api.py / test_device_gate.py)
GATE_FFT, GATE_DB = 256, 60
SENTINEL = numpy.float32(-7777.25)                  # no spectrogram (exp) and no mc row of these nets holds it


@contextlib.contextmanager
def graph_env(on):
    """RY_GRAPH is read by `ry_net_create` (clones inherit the setting): '0' = every call runs its launches eagerly."""
    old = os.environ.get('RY_GRAPH')
    os.environ['RY_GRAPH'] = '1' if on else '0'
    try:
        yield
    finally:
        if old is None:
            del os.environ['RY_GRAPH']
        else:
            os.environ['RY_GRAPH'] = old


def bins(name):
    return FFTLEN[name] // 2 + 1


def mtx(name):
    return sptk.mc2sp_matrix(8, sptk.mcepalpha(FS), FFTLEN[name])


def make_pair(ctx, name, graph=True):
    (d1, P1), (d2, P2) = synth.model_params(name)
    with graph_env(graph):
        n1 = engine.Net(ctx, d1, flatten_params(d1, P1))
        n2 = engine.Net(ctx, d2, flatten_params(d2, P2), width=bins(name) - 1)
    return n1, n2


def window(n, seed, keep=0.7):
    """(x_eff, effective) of n frames; keep = share of effective frames, 'lone' = exactly one."""
    rng = numpy.random.default_rng(seed)
    x = synth.stage1_input(n, seed=seed)[0]
    if keep == 'lone':
        eff = numpy.zeros(n, bool); eff[int(rng.integers(n))] = True
    else:
        eff = rng.random(n) < keep
    return numpy.ascontiguousarray(x[eff]), eff


def wave_window(n, seed, quiet=0.4):
    """A window that goes in as a wave: (wave of n * HOP samples, feat (n, 9), effective (n,) by the loop-per-frame oracle of the gate).
    quiet = share of the wave scaled below the gate (1.0: the wave is all zeros)."""
    rng = numpy.random.default_rng(seed)
    w = (0.1 * rng.normal(size=n * HOP)).astype(numpy.float32)
    if quiet >= 1.0:
        w[:] = 0.0
    elif quiet > 0:
        a = int(rng.integers(0, max(1, int(n * (1 - quiet)))))
        w[a * HOP:(a + int(round(n * quiet))) * HOP] *= 1e-4
    feat = (rng.normal(size=(n, synth.MC_DIMS)) * synth.MC_SCALE).astype(numpy.float32)
    eff = oef.separate_effective_mask(w, FS, n, GATE_DB, GATE_FFT, FP, 'abs')
    return w, feat, numpy.asarray(eff, bool)


def gate_args():
    return (HOP, GATE_FFT) + tuple(gate.thresholds(GATE_DB))


def plain(ctx, name, windows):
    """[(mc, sp)] of (x_eff, effective) windows: graphs off, one lane, discard (0, 0), one window at a time."""
    n1, n2 = make_pair(ctx, name, graph=False)
    core = engine.VcCore(n1, n2, mtx(name), lanes=1)
    try:
        return [core.convert(x, e) for x, e in windows]
    finally:
        core.close(); n1.close(); n2.close()


_torch_nets = {}


def oracle_window(name, x_eff, effective):
    """voice_changer.py:33-41 on the CPU oracle for one window: stage 1 on the effective rows, zeros elsewhere, mc2sp + 1e-16, stage 2."""
    if name not in _torch_nets:
        (_, P1), (_, P2) = synth.model_params(name)
        _torch_nets[name] = (torch_ref.TorchUNet(P1), torch_ref.TorchUNet(P2))
    t1, t2 = _torch_nets[name]
    mc = numpy.zeros((len(effective), synth.MC_DIMS), numpy.float32)
    if effective.any():
        mc[effective] = torch_ref.stage1_convert_core(t1, x_eff)
    sp_mid = (omc.mc2sp(mc, omc.mcepalpha(FS), FFTLEN[name]) + 1e-16).astype(numpy.float32)
    return mc, torch_ref.stage2_convert(t2, sp_mid)


def hold_plain_to_the_oracle(name, windows, ref, picks):
    """`plain` of the picked windows against the CPU oracle at the project's bar (cases.TOL)."""
    for i in picks:
        (x, e), (mc, sp) = windows[i], ref[i]
        mc_o, sp_o = oracle_window(name, x, e)
        e_mc, e_sp = rel_max(mc, mc_o), float(numpy.abs(sp.astype(numpy.float64) / sp_o - 1).max())
        print('plain window %d (%d of %d frames effective) against the CPU oracle: mc %.2e, sp element-wise %.2e' % (i, int(e.sum()), len(e), e_mc, e_sp))
        assert e_mc < cases.TOL and e_sp < cases.TOL and not mc[~e].any(), (i, e_mc, e_sp)


def all_differ(arrays, what):
    """The no-op guard: no two of these arrays are equal (a test whose inputs or references coincide checks nothing)."""
    seen = {}
    for i, a in enumerate(arrays):
        a = numpy.ascontiguousarray(a)
        key = (a.shape, a.dtype.str, a.tobytes())
        assert key not in seen, '%s %d and %d are equal: the scenario would not see one taken for the other' % (what, seen[key], i)
        seen[key] = i


def same_bits(got, want, what):
    """array_equal with a message that says where: the call of the sequence (in `what`), how many elements, which rows and columns."""
    got, want = numpy.asarray(got), numpy.asarray(want)
    assert got.shape == want.shape, '%s: shape %s, plain has %s' % (what, got.shape, want.shape)
    if numpy.array_equal(got, want):
        return
    dd = numpy.argwhere(got.reshape(len(got), -1) != want.reshape(len(want), -1))
    rows = sorted(set(dd[:, 0].tolist()))
    with numpy.errstate(all='ignore'):
        rel = float(numpy.nanmax(numpy.abs(got.astype(numpy.float64) - want) / numpy.maximum(numpy.abs(want.astype(numpy.float64)), 1e-30)))
    raise AssertionError('%s: %d of %d elements differ, rows %s .. %s (%d rows of %d), cols %s, max rel %.3g, sentinel in %d, NaN in %d' % (
        what, len(dd), got.size, rows[:8], rows[-4:], len(rows), len(got), sorted(set(dd[:, 1].tolist()))[:8], rel,
        int((got == SENTINEL).sum()), int(numpy.isnan(got.astype(numpy.float64)).sum())))


class Blocks(object):
    """Device blocks of one scenario, freed together."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, n_floats, fill=None):
        p = self.ctx.dev_alloc(max(int(n_floats), 1))
        self.ptrs.append(p)
        if fill is not None:
            self.fill(p, n_floats, fill)
        return p

    def fill(self, p, n_floats, value=SENTINEL):
        self.ctx.dev_upload(p, numpy.full(max(int(n_floats), 1), value, numpy.float32))

    def put(self, a):
        a = numpy.ascontiguousarray(a)
        p = self.alloc(a.size)
        if a.size:
            self.ctx.dev_upload(p, a)
        return p

    def get(self, p, shape, dtype=numpy.float32):
        a = numpy.empty(shape, dtype)
        if a.size:
            self.ctx.dev_download(p, a)
        return a

    def free(self):
        for p in self.ptrs:
            self.ctx.dev_free(p)
        self.ptrs = []


def graph_cache_model(shapes):
    """What `run_plan` does with one (in, out) address pair of one plan for a sequence of shape keys, restated for the report the tests
    print (not for any assertion): the first call captures, the same shape replays, another shape runs eagerly once and is captured
    when it comes twice in a row."""
    graph, last, out = None, None, []
    for s in shapes:
        if graph is None:
            graph = s; out.append('capture')
        elif s == graph:
            out.append('replay')
        elif s == last:
            graph = s; out.append('re-capture')
        else:
            out.append('eager')
        last = s
    return out
