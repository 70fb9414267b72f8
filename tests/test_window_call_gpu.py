"""The two state machines behind every window call, on the card, where they are real: the graph / plan cache of `run_plan` and `get_plan`
(csrc/ry_exec.cpp: compiled out under the emulator) and the cross-stream order of `ry_vc_*` (csrc/ry_vc.cpp: events, stream waits and
asynchronous copies are no-ops and memcpy under the emulator).  Every scenario is one fixed sequence, run once, that walks the transitions
of its machine, and every result is compared BIT FOR BIT with `plain` (window_call_ref.py): the same windows on handles created under
RY_GRAPH=0, one lane, no discard, one window at a time -- nothing replayed, nothing in flight, no state to get wrong.  `plain` itself is
held to the CPU oracle at cases.TOL in each scenario.  Lanes, replay, ring slots and discards are documented to leave the bits alone
("same plans, same arithmetic"); the batch call alone builds another plan (B > 1) and is held to the 1e-5 of
test_window_call_lanes_discard_and_batch against `plain`, and bit for bit against the same batch call made alone on a drained handle.
Windows of a scenario all differ (content, and where the scenario allows length and effective count), so a stale or early read lands on
visibly different numbers; the guard `all_differ` asserts it.  Each test prints the transitions it reached (pytest -s)."""
import collections

import numpy
import pytest

import cases
import window_call_ref as wr
from conftest import rel_max
from oracle import torch_ref
from realtime_yukarin_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def syn8_plain(gpu_ctx):
    """The predictor pair `plain` of the predictor-level scenarios runs on: created under RY_GRAPH=0."""
    n1, n2 = wr.make_pair(gpu_ctx, 'SYN-8', graph=False)
    yield n1, n2
    n1.close(); n2.close()


def _net(ctx, stage):
    """A fresh graph-replaying SYN-8 predictor of one stage (every scenario starts from empty caches)."""
    n1, n2 = wr.make_pair(ctx, 'SYN-8', graph=True)
    (n2 if stage == 1 else n1).close()
    return n1 if stage == 1 else n2


def _cols(stage):
    return synth.MC_DIMS if stage == 1 else wr.bins('SYN-8')


def _input(stage, n, seed, batch=1):
    """(batch, n, cols), or (n, cols) for batch 1: what `Net.convert` of this stage takes."""
    x = synth.stage1_input(n, batch, seed=seed) if stage == 1 else synth.stage2_input(n, batch, seed=seed, bins=wr.bins('SYN-8'))
    return x[0] if batch == 1 else x


def _hold_convert_to_the_oracle(stage, x, y):
    """`plain` of a predictor-level scenario (`Net.convert` on a handle without graphs) against the CPU oracle, cases.TOL."""
    (_, P1), (_, P2) = synth.model_params('SYN-8')
    if stage == 1:
        err = rel_max(y, torch_ref.stage1_convert_core(torch_ref.TorchUNet(P1), x))
    else:
        err = float(numpy.abs(y.astype(numpy.float64) / torch_ref.stage2_convert(torch_ref.TorchUNet(P2), x) - 1).max())
    print('plain stage-%d convert of %d frames against the CPU oracle: %.2e' % (stage, len(x), err))
    assert err < cases.TOL, err


def _keep(n, front, back):
    k0 = front if front < n else 0
    return k0, (n - back if n - back > k0 else n)


# ---- A. graph and plan cache (predictor level) ---------------------------------------------------------------------------------------

A1_SEQ = 'aaababbbaacca'
A1_N = {'a': 37, 'b': 50, 'c': 130}              # a, b: one plan (padded 128), the smaller one captured first; c: a second plan (padded 256)


@pytest.mark.parametrize('stage', [2, 1])
def test_a1_shape_transitions_on_one_address_pair(gpu_ctx, syn8_plain, stage):
    """One (in, out) address pair, n = a a a b a b b b a a c c a: capture, replay, a new shape run eagerly, alternation that never
    captures, re-capture, a second plan, and back -- through the host call (the plan's staging pair) and through the device-pointer call
    on fixed blocks (rows behind n keep the sentinel: a replay with a longer window's row count would write them).  Then the raw forward
    on fixed blocks at two padded lengths."""
    net, pnet, cols = _net(gpu_ctx, stage), syn8_plain[stage - 1], _cols(stage)
    ns = [A1_N[c] for c in A1_SEQ]
    xs = [_input(stage, n, 1100 + i) for i, n in enumerate(ns)]
    ref = [pnet.convert(x) for x in xs]
    wr.all_differ(xs, 'A1 input'); wr.all_differ(ref, 'A1 plain output')
    _hold_convert_to_the_oracle(stage, xs[0], ref[0]); _hold_convert_to_the_oracle(stage, xs[10], ref[10])
    blk = wr.Blocks(gpu_ctx)
    try:
        for i, (n, x) in enumerate(zip(ns, xs)):
            wr.same_bits(net.convert(x), ref[i], 'A1 stage %d host call %d of %s (n = %d)' % (stage, i, A1_SEQ, n))
        nmax = max(ns)
        d_in, d_out = blk.alloc(nmax * cols), blk.alloc(nmax * cols)
        for i, (n, x) in enumerate(zip(ns, xs)):
            gpu_ctx.dev_upload(d_in, x); blk.fill(d_out, nmax * cols)
            net.convert_device(d_in, d_out, 1, n)
            gpu_ctx.sync()
            y = blk.get(d_out, (nmax, cols))
            wr.same_bits(y[:n], ref[i], 'A1 stage %d device-pointer call %d of %s (n = %d)' % (stage, i, A1_SEQ, n))
            assert (y[n:] == wr.SENTINEL).all(), 'A1 stage %d device-pointer call %d (n = %d) wrote rows %s behind the window' % (
                stage, i, n, (n + numpy.nonzero((y[n:] != wr.SENTINEL).any(axis=1))[0])[:8])
        # the raw forward (mode 0: captured on first sight) on fixed blocks, two padded lengths taking turns
        fcols = synth.MC_DIMS if stage == 1 else wr.bins('SYN-8') - 1
        rng = numpy.random.default_rng(1199)
        ts = (128, 128, 256, 128, 256, 256)
        fx = [rng.normal(size=(1, t, fcols)).astype(numpy.float32) for t in ts]
        fref = [pnet.forward(x) for x in fx]
        wr.all_differ(fref, 'A1 plain forward')
        f_in, f_out = blk.alloc(256 * fcols), blk.alloc(256 * fcols)
        for i, (t, x) in enumerate(zip(ts, fx)):
            gpu_ctx.dev_upload(f_in, x); blk.fill(f_out, 256 * fcols)
            net.forward_device(f_in, f_out, 1, t)
            gpu_ctx.sync()
            wr.same_bits(blk.get(f_out, (1, 256, fcols))[0, :t], fref[i][0], 'A1 stage %d forward_device call %d (T = %d)' % (stage, i, t))
        per_plan = {'plan 128 (a, b)': [c for c in A1_SEQ if c != 'c'], 'plan 256 (c)': [c for c in A1_SEQ if c == 'c']}
        for name, seq in per_plan.items():
            print('A1 stage %d, %s, host pair and device pair alike: %s' % (stage, name, ' '.join('%s:%s' % p for p in zip(seq, wr.graph_cache_model(seq)))))
    finally:
        gpu_ctx.sync(); blk.free(); net.close()


A2_DISCARDS = [(0, 0), (0, 0), (10, 10), (10, 10), (0, 0), (0, 5), (0, 5), (10, 10), (60, 0), (60, 0)]


def test_a2_discards_are_part_of_the_shape(gpu_ctx, syn8_plain):
    """n = 50 on one address pair under a sequence of discards (the last would keep nothing, so it keeps all rows): the kept rows equal
    `plain`; the host call returns zeros in the discarded rows, the device-pointer call leaves them untouched (the ABI says so)."""
    net, pnet, cols, n = _net(gpu_ctx, 2), syn8_plain[1], _cols(2), 50
    xs = [_input(2, n, 1200 + i) for i in range(len(A2_DISCARDS))]
    ref = [pnet.convert(x) for x in xs]
    wr.all_differ(xs, 'A2 input'); wr.all_differ(ref, 'A2 plain output')
    _hold_convert_to_the_oracle(2, xs[0], ref[0])
    blk = wr.Blocks(gpu_ctx)
    lib = gpu_ctx.lib
    try:
        for i, ((f, b), x) in enumerate(zip(A2_DISCARDS, xs)):
            k0, k1 = _keep(n, f, b)
            y = net.convert(x, discard=(f, b))
            wr.same_bits(y[k0:k1], ref[i][k0:k1], 'A2 host call %d, discard %s, rows %d .. %d' % (i, (f, b), k0, k1))
            assert not y[:k0].any() and not y[k1:].any(), 'A2 host call %d, discard %s: the discarded rows are not zeros' % (i, (f, b))
        d_in, d_out = blk.alloc(n * cols), blk.alloc(n * cols)
        for i, ((f, b), x) in enumerate(zip(A2_DISCARDS, xs)):
            k0, k1 = _keep(n, f, b)
            gpu_ctx.dev_upload(d_in, x); blk.fill(d_out, n * cols)
            lib.check(lib.dll.ry_sr_convert_rows(net.handle, _lib._fptr(d_in), _lib._fptr(d_out), 1, n, f, b, 1))
            gpu_ctx.sync()
            y = blk.get(d_out, (n, cols))
            wr.same_bits(y[k0:k1], ref[i][k0:k1], 'A2 device-pointer call %d, discard %s, rows %d .. %d' % (i, (f, b), k0, k1))
            assert (y[:k0] == wr.SENTINEL).all() and (y[k1:] == wr.SENTINEL).all(), \
                'A2 device-pointer call %d, discard %s: discarded rows were written' % (i, (f, b))
        assert _keep(n, 60, 0) == (0, n)
        print('A2 shape keys (front, back) on each pair: ' + ' '.join('%s:%s' % p for p in zip(A2_DISCARDS, wr.graph_cache_model(A2_DISCARDS))))
    finally:
        gpu_ctx.sync(); blk.free(); net.close()


@pytest.mark.parametrize('stage', [2, 1])
def test_a3_more_than_64_address_pairs(gpu_ctx, syn8_plain, stage):
    """66 output blocks on one plan, each run twice (capture, replay), then the first two again: they were evicted (64 pairs are kept,
    least recently used goes) and capture anew.  Every output has the bits of `plain`, and a host call afterwards still works."""
    net, pnet, cols, n, blocks = _net(gpu_ctx, stage), syn8_plain[stage - 1], _cols(stage), 20, 66
    xs = [_input(stage, n, 1300 + k) for k in range(blocks)]
    ref = [pnet.convert(x) for x in xs]
    wr.all_differ(xs, 'A3 input'); wr.all_differ(ref, 'A3 plain output')
    _hold_convert_to_the_oracle(stage, xs[0], ref[0])
    blk = wr.Blocks(gpu_ctx)
    try:
        d_in = blk.alloc(n * cols)
        outs = [blk.alloc(n * cols) for _ in range(blocks)]
        assert len(set(outs)) == blocks
        order = [k for k in range(blocks) for _ in range(2)] + [0, 1]
        for i, k in enumerate(order):
            gpu_ctx.dev_upload(d_in, xs[k]); blk.fill(outs[k], n * cols)
            net.convert_device(d_in, outs[k], 1, n)
            gpu_ctx.sync()
            wr.same_bits(blk.get(outs[k], (n, cols)), ref[k], 'A3 stage %d call %d (output block %d)' % (stage, i, k))
        wr.same_bits(net.convert(xs[5]), ref[5], 'A3 stage %d host call after the evictions' % stage)
        print('A3 stage %d: %d address pairs on one plan (64 are kept): %d captures and %d replays, %d evictions, '
              '2 captures of evicted pairs, 1 host call' % (stage, blocks, blocks, blocks, blocks - 64 + 2))
    finally:
        gpu_ctx.sync(); blk.free(); net.close()


@pytest.mark.parametrize('stage', [2, 1])
def test_a4_more_than_16_plans(gpu_ctx, syn8_plain, stage):
    """17 plans on one handle (stage 2: batch sizes 1 .. 17 of a 20-frame window, the plan key is (batch, padded frames); stage 1: the 17
    lengths 100 + 128 k).  The 17th drops all 16 before it; its device-pointer call is enqueued while the 16th is still unsynchronised.
    Then the first size again: rebuilt, with the bits of its first run."""
    net, pnet, cols = _net(gpu_ctx, stage), syn8_plain[stage - 1], _cols(stage)
    sizes = [(b, 20) for b in range(1, 18)] if stage == 2 else [(1, 100 + 128 * k) for k in range(17)]
    xs = [_input(stage, n, 1400 + i, batch=b) for i, (b, n) in enumerate(sizes)]
    ref = [pnet.convert(x) for x in xs]
    wr.all_differ(xs, 'A4 input'); wr.all_differ(ref, 'A4 plain output')
    _hold_convert_to_the_oracle(stage, xs[0], ref[0])
    blk = wr.Blocks(gpu_ctx)
    try:
        d_in = [blk.put(x) for x in xs]
        d_out = [blk.alloc(x.size, fill=wr.SENTINEL) for x in xs]
        first = []
        for i in range(15):
            net.convert_device(d_in[i], d_out[i], *sizes[i])
            gpu_ctx.sync()
            first.append(blk.get(d_out[i], xs[i].shape))
        net.convert_device(d_in[15], d_out[15], *sizes[15])            # the 16th plan, not waited for ...
        net.convert_device(d_in[16], d_out[16], *sizes[16])            # ... when the 17th arrives and every plan before it goes
        gpu_ctx.sync()
        first += [blk.get(d_out[15], xs[15].shape), blk.get(d_out[16], xs[16].shape)]
        for i, y in enumerate(first):
            wr.same_bits(y, ref[i], 'A4 stage %d plan %d (batch %d, %d frames)' % ((stage, i + 1) + sizes[i]))
        blk.fill(d_out[0], xs[0].size)
        net.convert_device(d_in[0], d_out[0], *sizes[0])
        gpu_ctx.sync()
        again = blk.get(d_out[0], xs[0].shape)
        wr.same_bits(again, first[0], 'A4 stage %d first size again, after its plan was dropped' % stage)
        print('A4 stage %d: 16 plans built and captured, the 17th dropped them under the 16th call in flight, the first rebuilt: 18 plans in all' % stage)
    finally:
        gpu_ctx.sync(); blk.free(); net.close()


def test_a5_dtype_round_trip_under_captured_graphs(gpu_ctx):
    """Two lanes, six windows twice in f32 (capture, replay), the same twelve in bf16x3, then f32 again, at depth 6: `set_dtype` drops the
    plans and graphs of the caller's handle and every clone follows on its next window.  f32 before and after has the bits of `plain`;
    bf16x3 stays within the 2e-5 of test_stage2_syn64_x3_variant of it; both passes of every mode are the same bits on every lane."""
    lens = (20, 33, 41, 7, 20, 50)
    wins = [wr.window(n, 1500 + i, keep=(1.0, 0.7, 0.4, 1.0, 0.6, 0.8)[i]) for i, n in enumerate(lens)]
    ref = wr.plain(gpu_ctx, 'SYN-8', wins)
    wr.all_differ([numpy.concatenate([e, x.ravel()]) for x, e in wins], 'A5 window')
    wr.all_differ([r[0] for r in ref], 'A5 plain mc'); wr.all_differ([r[1] for r in ref], 'A5 plain sp')
    wr.hold_plain_to_the_oracle('SYN-8', wins, ref, (0, 2))
    n1, n2 = wr.make_pair(gpu_ctx, 'SYN-8')
    core = engine.VcCore(n1, n2, wr.mtx('SYN-8'), lanes=2)
    res = {}
    try:
        for mode in ('f32', 'bf16x3', 'f32 again'):
            n2.set_dtype(mode.split()[0])
            res[mode] = list(core.convert_stream(wins + wins, depth=6))
    finally:
        n2.set_dtype('f32')
    core.close(); n1.close(); n2.close()
    worst = 0.0
    for mode, got in res.items():
        for t, (mc, sp) in enumerate(got):
            what = 'A5 %s, window %d of 12 (ring slot %d, lane %d, %s pass)' % (mode, t, t % 6, t % 6 % 2, 'first' if t < 6 else 'second')
            wr.same_bits(mc, ref[t % 6][0], what + ' mc')
            if mode == 'bf16x3':
                worst = max(worst, float(numpy.abs(sp.astype(numpy.float64) / ref[t % 6][1] - 1).max()))
                wr.same_bits(sp, got[t % 6][1], what + ' sp against the first pass')
            else:
                wr.same_bits(sp, ref[t % 6][1], what + ' sp')
    print('A5: f32 capture + replay on 2 lanes, set_dtype bf16x3 (plans and graphs dropped, the clone follows), capture + replay, set_dtype f32, capture + replay; '
          'bf16x3 against plain f32: sp max rel %.2e' % worst)
    assert worst < 2e-5, worst


# ---- B. stream ordering of the window call -------------------------------------------------------------------------------------------
# (B1: the emulator scenarios on the card are the `_gpu` twins of tests/test_vc_api.py)

B2_PATTERN = ('submit', 'wave', 'dev', 'submit', 'batch', 'submit', 'split', 'wave', 'dev', 'gate', 'submit')
B2_LENS = (5, 9, 30, 41, 130, 41, 9)               # slots grow under windows in flight, then stay large
B2_OPS = 33
# share of effective frames per call (wave / gate calls: share of the wave below the gate); one all-silent window per length at the most
B2_KEEP = {0: 0.7, 3: 1.0, 5: 0.0, 10: 'lone', 11: 0.4, 14: 1.0, 16: 0.85, 21: 0.6, 22: 0.6, 25: 1.0, 27: 0.3, 32: 0.9,            # submit
           2: 0.7, 8: 'lone', 13: 0.0, 19: 1.0, 24: 0.5, 30: 0.2,                                                                   # enqueue_device
           6: 0.6, 17: 1.0, 28: 0.5,                                                                                                # convert_stage1 + stage2_from_mc
           1: 0.4, 7: 1.0, 12: 0.0, 18: 0.7, 23: 0.2, 29: 0.5, 9: 0.5, 20: 0.0, 31: 0.3}                                            # submit_wave, gate
B2_BATCH_KEEP = {4: (0.7, 1.0), 15: (1.0, 1.0), 26: (0.5, 0.3)}                                                                     # enqueue_device_batch: two windows


class _Op(object):
    def __init__(self, i):
        self.i, self.kind, self.n = i, B2_PATTERN[i % len(B2_PATTERN)], B2_LENS[i % len(B2_LENS)]
        seed = 2000 + 7 * i
        self.wave = self.feat = None
        if self.kind in ('wave', 'gate'):
            self.wave, self.feat, e = wr.wave_window(self.n, seed, quiet=B2_KEEP[i])
            self.wins = [(numpy.ascontiguousarray(self.feat[e]), e)]
        elif self.kind == 'batch':
            self.wins = [wr.window(self.n, seed + j, keep=k) for j, k in enumerate(B2_BATCH_KEEP[i])]
        else:
            self.wins = [wr.window(self.n, seed, keep=B2_KEEP[i])]
        self.first = 0                       # index of its first window in the flat list `plain` ran

    @property
    def n_eff(self):
        return [int(e.sum()) for _, e in self.wins]


@pytest.fixture(scope='module')
def b2(gpu_ctx):
    ops = [_Op(i) for i in range(B2_OPS)]
    flat = []
    for op in ops:
        op.first = len(flat); flat += op.wins
    ref = wr.plain(gpu_ctx, 'SYN-8', flat)
    return ops, flat, ref


def _dev_blocks(blk, op):
    """Inputs up, outputs filled with the sentinel: (x, rows, mc, sp) device blocks of a device-pointer call."""
    x = numpy.concatenate([x for x, _ in op.wins]) if sum(op.n_eff) else numpy.zeros((0, synth.MC_DIMS), numpy.float32)
    rows = numpy.concatenate([numpy.nonzero(e)[0] for _, e in op.wins]).astype(numpy.int32)
    W, F = len(op.wins), wr.bins('SYN-8')
    return blk.put(x), blk.put(rows), blk.alloc(W * op.n * synth.MC_DIMS, fill=wr.SENTINEL), blk.alloc(W * op.n * F, fill=wr.SENTINEL)


def _b2_run(ctx, core, ops, blk):
    """The calls of `ops` in order on one core, waiting only where the API demands it: a ticket is collected when its ring slot is needed
    (by the next submit, by a device-pointer call whose turn falls on it, by a split call or the gate on slot 0), the rest at the end."""
    ring, held, res, log = core.ring, {}, {}, collections.Counter()
    caps = [[0, 0] for _ in range(ring)]
    count = {'ticket': 0, 'dev': 0}

    def collect(slot):
        t, i = held.pop(slot)
        res[i] = core.wait_wave(t) if ops[i].kind == 'wave' else core.wait(t)

    def take(slot, need_eff, need_frames, why):
        if slot in held:
            log['%s had to wait for the ticket on its slot' % why] += 1
            collect(slot)
        if need_eff > caps[slot][0] or need_frames > caps[slot][1]:
            log['slot grown under windows in flight' if held else 'slot grown with nothing in flight'] += 1
            caps[slot] = [max(need_eff, caps[slot][0]), max(need_frames, caps[slot][1])]

    dev = {op.i: _dev_blocks(blk, op) for op in ops if op.kind in ('dev', 'batch')}
    for op in ops:
        (x, e), n, ne = op.wins[0], op.n, op.n_eff[0]
        log[op.kind] += 1
        if op.kind in ('submit', 'wave'):
            slot = count['ticket'] % ring
            take(slot, ne if op.kind == 'submit' else n, n, op.kind)
            t = core.submit(x, e) if op.kind == 'submit' else core.submit_wave(op.wave, *wr.gate_args(), op.feat)
            assert t == count['ticket']
            held[slot] = (t, op.i); count['ticket'] += 1
            log['most tickets in flight'] = max(log['most tickets in flight'], len(held))
        elif op.kind == 'dev':
            slot = count['dev'] % ring
            take(slot, ne, n, 'enqueue_device')
            px, pr, pmc, psp = dev[op.i]
            core.enqueue_device(px, pr, ne, n, pmc, psp)
            op.slot = slot; count['dev'] += 1
        elif op.kind == 'batch':
            px, pr, pmc, psp = dev[op.i]
            core.enqueue_device_batch(px, pr, op.n_eff, n, pmc, psp)
        elif op.kind == 'split':
            take(0, ne, n, 'split call')
            y1 = core.convert_stage1(x)
            res[op.i] = (y1, core.stage2_from_mc(e, 1e-16))
        elif op.kind == 'gate':
            take(0, n, n, 'gate')
            res[op.i] = core.gate(op.wave, *wr.gate_args(), op.feat)
    log['tickets still in flight at the end'] = len(held)
    for slot in sorted(held, key=lambda s: held[s][0]):
        collect(slot)
    ctx.sync()
    F = wr.bins('SYN-8')
    for op in ops:
        if op.i in dev:
            W = len(op.wins)
            res[op.i] = (blk.get(dev[op.i][2], (W, op.n, synth.MC_DIMS)), blk.get(dev[op.i][3], (W, op.n, F)))
    return res, log


def _batch_against_plain(what, op, ref, mc, sp, k0=0, k1=None):
    """The batch call's own bar: mc bit for bit where stage 1 ran window by window (unequal effective counts), else 1e-5 of the largest
    value; the kept rows of sp within 1e-5 relative; mc rows of silent frames exactly zero."""
    same_counts = len(set(op.n_eff)) == 1 and len(op.wins) > 1
    for w, (_, e) in enumerate(op.wins):
        rmc, rsp = ref[op.first + w]
        if same_counts:
            assert float(numpy.abs(mc[w] - rmc).max()) <= 1e-5 * float(numpy.abs(rmc).max()), '%s window %d: mc' % (what, w)
        else:
            wr.same_bits(mc[w], rmc, '%s window %d mc' % (what, w))
        assert not mc[w][~e].any(), '%s window %d: mc rows of silent frames are not zero' % (what, w)
        err = float(numpy.abs(sp[w][k0:k1].astype(numpy.float64) / rsp[k0:k1] - 1).max())
        assert err < 1e-5, '%s window %d: sp rows %s .. %s differ from plain by %.3g' % (what, w, k0, k1, err)


@pytest.mark.parametrize('lanes', [1, 2, 3, 4])
def test_b2_mixed_entry_points_on_one_handle(gpu_ctx, b2, lanes):
    """One stream of calls on one core -- submit / wait, submit_wave / wait_wave, enqueue_device, enqueue_device_batch, convert_stage1 +
    stage2_from_mc, gate -- with the ring kept full and no wait the API does not demand; window lengths 5 .. 130 .. 9, effective shares
    0 .. 1 with all-silent and single-frame windows.  Every mc, sp, mask and row map equals `plain` / the gate's oracle."""
    ops, flat, ref = b2
    wr.all_differ([numpy.concatenate([e, x.ravel()]) for x, e in flat], 'B2 window')
    wr.all_differ([r[0] for r in ref], 'B2 plain mc'); wr.all_differ([r[1] for r in ref], 'B2 plain sp')
    if lanes == 1:
        gated = next(op.first for op in ops if op.kind == 'submit' and 0 < op.n_eff[0] < op.n and op.n > 9)
        whole = next(op.first for op in ops if op.n_eff[0] == op.n and op.n > 9)
        wr.hold_plain_to_the_oracle('SYN-8', flat, ref, (gated, whole))
    n1, n2 = wr.make_pair(gpu_ctx, 'SYN-8')
    core = engine.VcCore(n1, n2, wr.mtx('SYN-8'), lanes=lanes)
    blk = wr.Blocks(gpu_ctx)
    try:
        res, log = _b2_run(gpu_ctx, core, ops, blk)
        alone = {}
        for op in ops:                                                   # the batch calls again, each alone on the drained handle
            if op.kind == 'batch':
                px, pr, pmc, psp = _dev_blocks(blk, op)
                core.enqueue_device_batch(px, pr, op.n_eff, op.n, pmc, psp)
                gpu_ctx.sync()
                alone[op.i] = (blk.get(pmc, res[op.i][0].shape), blk.get(psp, res[op.i][1].shape))
    finally:
        gpu_ctx.sync(); blk.free(); core.close(); n1.close(); n2.close()
    for op in ops:
        (x, e), (rmc, rsp) = op.wins[0], ref[op.first]
        what = 'B2 lanes %d call %d (%s, %d frames, %d effective%s)' % (
            lanes, op.i, op.kind, op.n, op.n_eff[0], ', ring slot %d, lane %d' % (op.slot, op.slot % lanes) if op.kind == 'dev' else '')
        got = res[op.i]
        if op.kind in ('submit', 'wave'):
            wr.same_bits(got[0], rmc, what + ' mc'); wr.same_bits(got[1], rsp, what + ' sp')
            if op.kind == 'wave':
                wr.same_bits(got[2], e, what + ' mask')
        elif op.kind == 'dev':
            wr.same_bits(got[0][0], rmc, what + ' mc'); wr.same_bits(got[1][0], rsp, what + ' sp')
        elif op.kind == 'split':
            wr.same_bits(got[0], rmc[e], what + ' stage-1 rows'); wr.same_bits(got[1], rsp, what + ' sp')
        elif op.kind == 'gate':
            wr.same_bits(got[0], e, what + ' mask')
            wr.same_bits(got[2], numpy.nonzero(e)[0].astype(numpy.int32), what + ' row map'); wr.same_bits(got[1], op.feat[e], what + ' gathered rows')
        else:
            _batch_against_plain(what, op, ref, got[0], got[1])
            wr.same_bits(got[0], alone[op.i][0], what + ' mc against the same call alone'); wr.same_bits(got[1], alone[op.i][1], what + ' sp against the same call alone')
    print('B2 lanes %d (ring %d): %s' % (lanes, 6 if lanes <= 3 else 2 * lanes, ', '.join('%s: %d' % kv for kv in sorted(log.items()))))


@pytest.fixture(scope='module')
def b3(gpu_ctx):
    """13 = 2 * ring + 1 windows of 300 frames on SYN-64, and 13 more with the same masks and other content (the first pass)."""
    n, keeps = 300, (1.0, 0.7, 1.0, 0.5, 0.9, 1.0, 0.3, 1.0, 0.8, 0.6, 1.0, 0.95, 0.4)
    real = [wr.window(n, 3000 + i, keep=k) for i, k in enumerate(keeps)]
    first = [(numpy.ascontiguousarray(synth.stage1_input(n, seed=3100 + i)[0][e]), e) for i, (_, e) in enumerate(real)]
    ref = wr.plain(gpu_ctx, 'SYN-64', first + real)
    pair = wr.make_pair(gpu_ctx, 'SYN-64')
    yield first, real, ref[:13], ref[13:], pair
    pair[0].close(); pair[1].close()


@pytest.mark.parametrize('lanes', [1, 2])
def test_b3_slot_reuse_without_a_host_wait(gpu_ctx, b3, lanes):
    """2 * ring + 1 `enqueue_device` calls back to back into distinct output blocks, one sync at the end, on SYN-64 at 300 frames, where
    a stage 2 lasts long enough for a missing wait to matter: the only check that the `ev_done` wait on slot reuse and the `ev_mid` wait
    of stage 2 are really there.  Two passes over the same blocks and ring slots: the first (other content, the same masks) builds the
    plans and captures, the second replays with nothing on the host between its launches -- and what an early read finds in the slot is
    the first pass's window, other numbers."""
    first, real, ref_first, ref_real, (n1, n2) = b3
    n, F = 300, wr.bins('SYN-64')
    wr.all_differ([numpy.concatenate([e, x.ravel()]) for x, e in first + real], 'B3 window')
    wr.all_differ([r[0] for r in ref_first + ref_real], 'B3 plain mc'); wr.all_differ([r[1] for r in ref_first + ref_real], 'B3 plain sp')
    if lanes == 1:
        wr.hold_plain_to_the_oracle('SYN-64', real, ref_real, (0, 3))
    core = engine.VcCore(n1, n2, wr.mtx('SYN-64'), lanes=lanes)
    blk = wr.Blocks(gpu_ctx)
    got = []
    try:
        d_x = [blk.alloc(n * synth.MC_DIMS) for _ in real]
        d_r = [blk.put(numpy.nonzero(e)[0].astype(numpy.int32)) for _, e in real]
        d_mc = [blk.alloc(n * synth.MC_DIMS) for _ in real]
        d_sp = [blk.alloc(n * F) for _ in real]
        for wins in (first, real):
            core.set_lanes(lanes)                                        # (drains, and the device-pointer calls start at ring slot 0 again)
            for k, (x, e) in enumerate(wins):
                gpu_ctx.dev_upload(d_x[k], x); blk.fill(d_mc[k], n * synth.MC_DIMS); blk.fill(d_sp[k], n * F)
            for k, (x, e) in enumerate(wins):
                core.enqueue_device(d_x[k], d_r[k], len(x), n, d_mc[k], d_sp[k])
            gpu_ctx.sync()
            got.append([(blk.get(d_mc[k], (n, synth.MC_DIMS)), blk.get(d_sp[k], (n, F))) for k in range(len(wins))])
    finally:
        gpu_ctx.sync(); blk.free(); core.close()
    for name, res, ref, wins in (('first pass (capture)', got[0], ref_first, first), ('second pass (replay)', got[1], ref_real, real)):
        for k, ((mc, sp), (rmc, rsp)) in enumerate(zip(res, ref)):
            what = 'B3 lanes %d, %s, call %d of 13 (ring slot %d, lane %d, %d of 300 frames effective)' % (lanes, name, k, k % 6, k % 6 % lanes, len(wins[k][0]))
            wr.same_bits(mc, rmc, what + ' mc'); wr.same_bits(sp, rsp, what + ' sp')
    print('B3 lanes %d: 2 x 13 enqueue_device calls back to back, one sync per pass: every ring slot reused twice without a host wait '
          '(ev_done), 13 stage-2 starts behind ev_mid per pass; first pass captures, second replays' % lanes)


B4_COUNTS = (1, 3, 2, 8, 3)
B4_KEEPS = ((0.7,), (1.0, 1.0, 1.0), (0.5, 0.0), (1.0, 0.6, 'lone', 0.9, 0.3, 1.0, 0.75, 0.45), (1.0, 1.0, 1.0))
B4_DISCARD = {4: (10, 10)}


def test_b4_batch_sets_taking_turns(gpu_ctx):
    """Five `enqueue_device_batch` calls back to back (1, 3, 2, 8, 3 windows of 41 frames: both buffer sets regrow under queued work; equal
    effective counts run stage 1 as one batch, unequal ones window by window; one call under discard (10, 10)) into distinct blocks, one
    sync at the end: each window against `plain` at the batch call's 1e-5, and bit for bit against the same call made alone afterwards."""
    n, F = 41, wr.bins('SYN-8')

    class Call(object):
        pass
    calls, flat = [], []
    for c, keeps in enumerate(B4_KEEPS):
        op = Call()
        op.i, op.n, op.first = c, n, len(flat)
        op.wins = [wr.window(n, 4000 + 20 * c + j, keep=k) for j, k in enumerate(keeps)]
        op.n_eff = [int(e.sum()) for _, e in op.wins]
        assert len(op.wins) == B4_COUNTS[c]
        calls.append(op); flat += op.wins
    assert len(set(calls[1].n_eff)) == 1 and len(set(calls[3].n_eff)) > 1
    ref = wr.plain(gpu_ctx, 'SYN-8', flat)
    wr.all_differ([numpy.concatenate([e, x.ravel()]) for x, e in flat], 'B4 window')
    wr.all_differ([r[0] for r in ref], 'B4 plain mc'); wr.all_differ([r[1] for r in ref], 'B4 plain sp')
    wr.hold_plain_to_the_oracle('SYN-8', flat, ref, (0, 1))
    n1, n2 = wr.make_pair(gpu_ctx, 'SYN-8')
    core = engine.VcCore(n1, n2, wr.mtx('SYN-8'))
    blk = wr.Blocks(gpu_ctx)
    res = []
    try:
        for alone in (False, True):
            dev = [_dev_blocks(blk, op) for op in calls]
            for op, (px, pr, pmc, psp) in zip(calls, dev):
                core.set_discard(*B4_DISCARD.get(op.i, (0, 0)))          # (host state of the core: nothing is waited for)
                core.enqueue_device_batch(px, pr, op.n_eff, n, pmc, psp)
                if alone:
                    gpu_ctx.sync()
            gpu_ctx.sync()
            res.append([(blk.get(pmc, (len(op.wins), n, synth.MC_DIMS)), blk.get(psp, (len(op.wins), n, F))) for op, (_, _, pmc, psp) in zip(calls, dev)])
    finally:
        core.set_discard(0, 0)
        gpu_ctx.sync(); blk.free(); core.close(); n1.close(); n2.close()
    for op, (mc, sp), (amc, asp) in zip(calls, res[0], res[1]):
        k0, k1 = _keep(n, *B4_DISCARD.get(op.i, (0, 0)))
        what = 'B4 call %d (%d windows, effective counts %s, buffer set %d, rows %d .. %d kept)' % (op.i, len(op.wins), op.n_eff, op.i & 1, k0, k1)
        _batch_against_plain(what, op, ref, mc, sp, k0, k1)
        assert (sp[:, :k0] == wr.SENTINEL).all() and (sp[:, k1:] == wr.SENTINEL).all(), what + ': discarded rows of the caller\'s block were written'
        wr.same_bits(mc.reshape(-1, synth.MC_DIMS), amc.reshape(-1, synth.MC_DIMS), what + ' mc against the same call alone')
        wr.same_bits(sp.reshape(-1, F), asp.reshape(-1, F), what + ' sp against the same call alone')
    print('B4: 5 batch calls back to back, buffer sets 0 1 0 1 0; set 0 grown for 1, 2, 3 windows and set 1 for 3, 8 under queued work; '
          'stage 1 as one batch in calls 1 and 4, window by window in calls 0, 2, 3; discard (10, 10) in call 4; then each call alone')
