"""Cases the emulator and the GPU tests of the device route into the output gate share (test_out_gate_device_cpu.py, test_out_gate_device_gpu.py):
the synthesizer entries that leave their samples on the card (`ry_synth_push_dev` / `ry_synth_flush_dev` / `ry_synth_bank_push_dev`), the gates fed
there (`OutputGate.push_device` / `OutputGateBank.push_device`) and `Pipeline.push(out_gate=)` / `PipelineBank.push(out_gate=)` on that route.  The
yardstick of every comparison is the host route on a twin with the same seed in the same process -- `ry_synth_push` / `ry_synth_flush` /
`ry_synth_bank_push`, `OutputGate.push` of host samples, `push` without a gate followed by the gate's `push` (what `push(out_gate=)` ran before
there was a device route) -- and every comparison is bit equality with dtype (`pipeline_cases.same`).  Every destination block is filled with NaN
patterns (all bits set) before a call and read back whole after it: what the call did not emit still holds the pattern."""
import ctypes

import numpy

import output_gate_cases as C
import pipeline_cases as P
import pipeline_world_cases as W
import world_synth_cases as S
from realtime_yukarin_amd import _lib, output_gate, pipeline, world_synth

FS, PERIOD = 24000, 5.0
ONES = 0xFFFFFFFF
DP, LLP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int)
SCALE = 0.5


class Poisoned(object):
    """A device block of `samples` float64 samples, every bit set."""

    def __init__(self, ctx, samples: int):
        self.ctx, self.samples = ctx, int(samples)
        self.address = ctx.dev_alloc(2 * self.samples)
        self.block = world_synth.SampleBlock(self.address, self.samples)
        self.poison()

    def poison(self):
        self.ctx.dev_upload(self.address, numpy.full(2 * self.samples, ONES, numpy.uint32))

    def put(self, at: int, x):
        """Samples x at sample `at`; -> their address."""
        x = numpy.ascontiguousarray(x, numpy.float64)
        assert at + x.size <= self.samples
        if x.size:
            self.ctx.dev_upload(self.address + 8 * at, x.view(numpy.uint32))
        return self.address + 8 * at

    def words(self) -> numpy.ndarray:
        out = numpy.empty(2 * self.samples, numpy.uint32)
        self.ctx.dev_download(self.address, out)
        return out

    def holds_only(self, at: int, x) -> bool:
        """Samples [at, at + len(x)) have the bits of x and every other word is still the pattern."""
        w = self.words()
        x = numpy.ascontiguousarray(x, numpy.float64)
        inside = numpy.array_equal(w[2 * at:2 * (at + x.size)], x.view(numpy.uint32))
        return inside and bool((w[:2 * at] == ONES).all()) and bool((w[2 * (at + x.size):] == ONES).all())

    def untouched(self) -> bool:
        return bool((self.words() == ONES).all())

    def close(self):
        self.ctx.dev_free(self.address)


def pieces(item, cuts):
    out, r = [], 0
    for n in cuts:
        out.append(tuple(a[r:r + n] for a in item))
        r += n
    return out


# ---- 1: the synthesizer alone -------------------------------------------------------------------------------------------------------------------
CUTS = (1, 2, 40, 41)


def check_lone_synth(ctx, kind='glide', device_rows=False, poison=False):
    """Pushes of 1, 2, 40 and 41 frames and a flush through the `_dev` entries against a twin on `ry_synth_push` / `ry_synth_flush`: the block's
    first n_out samples from the destination on are the twin's, everything else keeps the pattern.  The push of one frame returns nothing; the
    destinations lie at sample 0, at odd offsets, and the flush lands right behind the last push in one block.  poison: `ry_synth_debug_poison`
    before every call."""
    item = S.case(kind, sum(CUTS), FS)
    dev = world_synth.Synthesizer(FS, PERIOD, seed=7, ctx=ctx)
    host = world_synth.Synthesizer(FS, PERIOD, seed=7, ctx=ctx)
    room = dev.length(sum(CUTS)) + 64
    blk = Poisoned(ctx, room)
    sizes = []
    for call, (piece, at) in enumerate(zip(pieces(item, CUTS), (0, 3, 1, 7))):
        want = host.push(*piece)
        send = piece if not device_rows else (piece[0], world_synth.to_device(ctx, piece[1]), world_synth.to_device(ctx, piece[2]))
        assert dev.bound(len(piece[0])) >= want.size
        if poison:
            dev.poison()
        blk.poison()
        got = dev.push_device(*send, blk.block, at)
        assert got == want.size, (call, got, want.size)
        assert blk.holds_only(at, want), call
        sizes.append(got)
        idx, sh, vo = dev.pulses()
        widx, wsh, wvo = host.pulses()
        assert numpy.array_equal(idx, widx) and numpy.array_equal(sh, wsh) and numpy.array_equal(vo, wvo), call
        if call == len(CUTS) - 1:                                           # the flush right behind this push, at an odd sample where the push was
            rest = host.flush()
            assert dev.bound(0, True) == rest.size
            n = dev.flush_device(blk.block, at + got)
            assert n == rest.size and n > 0 and blk.holds_only(at, numpy.concatenate([want, rest])), (n, rest.size)
    assert sizes[0] == 0 and sizes[2] > 0, sizes                            # one frame: nothing can be emitted yet
    # the stream was reset by the flush: a new signal equals the twin's again
    want = host.push(*pieces(item, (5, 30))[1])
    blk.poison()
    assert dev.push_device(*pieces(item, (5, 30))[1], blk.block, 0) == want.size and blk.holds_only(0, want)
    blk.close()
    dev.close()
    host.close()


def bank_calls(B):
    """(frames per stream, final) per call.  B = 3: all streams; stream 1 sits out; stream 2 ends with frames; stream 0 ends without frames while
    stream 2 starts anew; the rest ends.  B = 1: two pushes, a push that ends the signal, a new signal."""
    if B == 1:
        return [((1,), ()), ((40,), ()), ((9,), (0,)), ((30,), ()), ((0,), (0,))]
    return [((13, 7, 20), ()), ((11, 0, 2), ()), ((5, 6, 17), (2,)), ((0, 9, 14), (0,)), ((0, 3, 0), (1, 2))]


def check_bank_synth(ctx, B, device_rows=False, poison=False):
    """`StreamBank.push_device` against a twin bank's `push`, call by call: the offsets equal the cumulated sizes of the twin's arrays, the block
    holds the twin's samples back to back, nothing else is written, and the counters show one download fewer and the same launches."""
    import synth_bank_cases as SB
    seeds = [3, 11, 29][:B]
    dev = world_synth.StreamBank(FS, PERIOD, n_streams=B, seeds=seeds, ctx=ctx)
    host = world_synth.StreamBank(FS, PERIOD, n_streams=B, seeds=seeds, ctx=ctx)
    calls = bank_calls(B)
    totals = [sum(c[0][b] for c in calls) for b in range(B)]
    items = [S.case(('glide', 'voiced71', 'below')[b], totals[b], FS) for b in range(B)]
    cut = [SB.cut(items[b], [c[0][b] for c in calls]) for b in range(B)]
    blk = Poisoned(ctx, sum(dev.fs // 200 * t + 1 for t in totals) + 64)
    emitted = 0
    for call, (_, final) in enumerate(calls):
        its = [cut[b][call] for b in range(B)]
        send = SB.device_slices(ctx, its) if device_rows and any(it is not None for it in its) else its
        want = host.push(send, final)
        hc = host.counts()
        if poison:
            dev.poison()
        blk.poison()
        off = dev.push_device(send, final, blk.block)
        assert off.dtype == numpy.int64 and off.tolist() == [0] + numpy.cumsum([w.size for w in want]).tolist(), (call, off)
        assert blk.holds_only(0, numpy.concatenate(want)), call
        dc = dev.counts()
        assert dc['launches'] == hc['launches'] and dc['h2d'] == hc['h2d'], (call, dc, hc)
        assert dc['d2h'] == hc['d2h'] - (1 if off[-1] > 0 else 0), (call, dc, hc)
        for b in range(B):
            for p, q in zip(dev.pulses(b), host.pulses(b)):
                assert numpy.array_equal(p, q), (call, b)
        emitted += int(off[-1])
    assert emitted > 0
    blk.close()
    dev.close()
    host.close()


def check_bank_item_by_item(ctx):
    """A list `push` runs item by item (host rows beside device rows): `push_device` lays the streams back to back all the same."""
    B, seeds = 3, [3, 11, 29]
    dev = world_synth.StreamBank(FS, PERIOD, n_streams=B, seeds=seeds, ctx=ctx)
    host = world_synth.StreamBank(FS, PERIOD, n_streams=B, seeds=seeds, ctx=ctx)
    items = [S.case('glide', 30, FS), None, S.case('voiced71', 25, FS)]
    mixed = [items[0], None, (items[2][0], world_synth.to_device(ctx, items[2][1]), world_synth.to_device(ctx, items[2][2]))]
    blk = Poisoned(ctx, 30 * 120 + 25 * 120 + 64)
    before = world_synth.calls['bank_fallback']
    for its, send, final in ((items, mixed, ()), ([None] * 3, [None] * 3, (0, 2))):
        want = host.push(its, final)
        blk.poison()
        off = dev.push_device(send, final, blk.block)
        assert off.tolist() == [0] + numpy.cumsum([w.size for w in want]).tolist() and blk.holds_only(0, numpy.concatenate(want))
    assert world_synth.calls['bank_fallback'] == before + 1
    blk.close()
    dev.close()
    host.close()


# ---- 2: the gate fed on the card ------------------------------------------------------------------------------------------------------------------
GATE_CHUNKS = (1025, 2048)
GATE_DTYPES = (numpy.float32, numpy.float64)


def gate_sequences(chunk):
    """name -> sample counts per push: one that completes no chunk, one that completes exactly one (nothing carried behind it), one that leaves
    more than a chunk carried (an empty push then cuts the next chunk of the backlog)."""
    return {'none': (chunk // 3, chunk // 3), 'exact': (chunk // 2, chunk - chunk // 2, 1), 'backlog': (2 * chunk + 37, 0, 5)}


def same_out(a, b) -> bool:
    return (a is None and b is None) or (a is not None and b is not None and P.same(a, b))


def same_last(a, b) -> bool:
    return a[:2] == b[:2] and numpy.array_equal(numpy.float64(a[2]).view(numpy.uint64), numpy.float64(b[2]).view(numpy.uint64))


def check_gate_fed_on_the_card(ctx, chunk, dtype, signal, sequence, poison=False):
    """`OutputGate.push_device` of samples at an odd sample offset of a device block against `push` of the same samples on a twin: the chunk, `last`
    and `held()` after every call; nothing of the samples goes up, and only an audible chunk comes down."""
    counts = gate_sequences(chunk)[sequence]
    x = C.signal(signal, sum(counts))
    dev = output_gate.OutputGate(chunk, C.THRESHOLD, SCALE, dtype, ctx=ctx)
    host = output_gate.OutputGate(chunk, C.THRESHOLD, SCALE, dtype, ctx=ctx)
    assert dev.on_device(ctx) and dev.on_device()
    blk = Poisoned(ctx, max(counts) + 8)
    r, emitted, down = 0, [], 0
    for n in counts:
        want = host.push(x[r:r + n])
        blk.poison()
        ptr = blk.put(3, x[r:r + n])
        if poison:
            dev.poison()
        got = dev.push_device(ptr if n else 0, n)
        assert same_out(got, want) and same_last(dev.last, host.last) and dev.held() == host.held(), (sequence, n, dev.last, host.last)
        dc, hc = dev.counts(), host.counts()
        assert dc['uploads'] == 1 and dc['upload_bytes'] == hc['upload_bytes'] - 8 * n, (dc, hc)      # the table alone: no sample goes up
        audible = dev.last[0] and not dev.last[1]
        assert dc['sample_bytes_down'] == (chunk * numpy.dtype(dtype).itemsize if audible else 0), dc
        assert dc['launches'] == hc['launches'] and dc['waits'] <= hc['waits'], (dc, hc)
        assert blk.holds_only(3, x[r:r + n])                                # the gate reads the block, it writes nothing there
        emitted.append(dev.last[0])
        down += dc['sample_bytes_down']
        r += n
    assert emitted == {'none': [False, False], 'exact': [False, True, False], 'backlog': [True, True, False]}[sequence], emitted
    if sequence == 'exact':
        assert dev.held() == 1
    assert (down > 0) == (signal == 'voiced' and sequence != 'none'), (signal, sequence, down)     # a silent chunk brings no sample to the host
    blk.close()
    dev.close()
    host.close()


def check_gate_bank_fed_on_the_card(ctx, chunk, dtype):
    """`OutputGateBank.push_device` (B = 3: an audible stream, one that sits calls out, a silent one) against `push` on a twin."""
    B = 3
    dev = output_gate.OutputGateBank(B, chunk, C.THRESHOLD, SCALE, dtype, ctx=ctx)
    host = output_gate.OutputGateBank(B, chunk, C.THRESHOLD, SCALE, dtype, ctx=ctx)
    rounds = [(chunk // 2, 0, chunk + 3), (chunk - chunk // 2, 7, chunk - 3), (0, 0, 0), (2 * chunk, chunk, 1)]
    names = ('voiced', 'sine', 'noise1e-6')
    blk = Poisoned(ctx, 4 * chunk + 64)
    at = [0, 0, 0]
    for counts in rounds:
        xs = [C.signal(names[b], 4 * chunk)[at[b]:at[b] + counts[b]] for b in range(B)]
        want = host.push([x if x.size else None for x in xs])
        off = numpy.concatenate([[0], numpy.cumsum(counts)]).astype(numpy.int64)
        blk.poison()
        ptr = blk.put(1, numpy.concatenate(xs))
        got = dev.push_device(ptr, off)
        for b in range(B):
            assert same_out(got[b], want[b]) and same_last(dev.last[b], host.last[b]) and dev.held(b) == host.held(b), (counts, b)
            at[b] += counts[b]
        if off[-1] > 0:
            dc, hc = dev.counts(), host.counts()
            assert dc['upload_bytes'] == hc['upload_bytes'] - 8 * int(off[-1]) and dc['sample_bytes_down'] == hc['sample_bytes_down'], (dc, hc)
    for bad in ([0, 1, 2], [1, 2, 3, 4], [0, 5, 4, 6]):
        try:
            dev.push_device(blk.address, bad)
        except ValueError:
            continue
        raise AssertionError(bad)
    blk.close()
    dev.close()
    host.close()


def check_host_fallback_has_no_device_form(ctx):
    g = output_gate.OutputGate(160, C.THRESHOLD, ctx=ctx)
    G = output_gate.OutputGateBank(2, 160, C.THRESHOLD, ctx=ctx)
    assert not g.on_device() and not g.on_device(ctx) and not G.on_device(ctx)
    for call in (lambda: g.push_device(8, 1), lambda: G.push_device(8, [0, 1, 1])):
        try:
            call()
        except ValueError:
            continue
        raise AssertionError('a host-fallback gate took device samples')


# ---- 2, 3: the pipelines on the device route ------------------------------------------------------------------------------------------------------
class Routes(object):
    def __init__(self):
        self.was = dict(pipeline.routes)

    def taken(self):
        now, was = dict(pipeline.routes), self.was
        self.was = now
        return now['gate_device'] - was['gate_device'], now['gate_host'] - was['gate_host']


def lone_pair(vc, mode, capacity, seed=3):
    """Two pipelines with one seed: the one under test and the twin of the host route."""
    param = W.param_of(vc)
    if mode == 'world':
        return [pipeline.Pipeline(vc, param, seed=seed, f0_mode='world', f0_fn=W.f0_fn) for _ in range(2)]
    return [pipeline.Pipeline(vc, param, crepe_capacity=capacity, seed=seed) for _ in range(2)]


def by_hand(pipe, gate, wave, **kw):
    """The host route as the parent ran it: `push` without a gate, the samples through the gate's `push` -> (what `push(out_gate=)` returns, how many
    samples the synthesizer emitted)."""
    raw = pipe.push(wave, **kw).wave
    out = gate.push(raw)
    return (out if out is not None else numpy.empty(0, gate.dtype)), raw.size


def check_lone_pipeline(vc, ctx, fs, mode, capacity, frames, chunk, dtype, monkeypatch, other_ctx=None):
    """A live stream through `Pipeline.push(out_gate=g)` on the device route against the host route on a twin: audible buffers, a buffer that takes
    the composed path in the middle (RY_DEVICE_GATE=0: the host route takes over for that call and the bits carry on), a silent buffer under
    gate_first, and a last buffer with final=True (push and flush in one block); then a second signal.  `g.last` and `g.held()` agree after every
    call, the route counter says which way each call went, and the gate's counters show that no sample went up.  other_ctx: a third pipeline over a
    gate of that context takes the host route and gives the same chunks."""
    from yukarin import Wave
    dev, host = lone_pair(vc, mode, capacity)
    g_dev = output_gate.OutputGate(chunk, P.THRESHOLD, SCALE, dtype, ctx=ctx)
    g_host = output_gate.OutputGate(chunk, P.THRESHOLD, SCALE, dtype, ctx=ctx)
    third = g_third = None
    if other_ctx is not None:
        third = lone_pair(vc, mode, capacity)[0]
        g_third = output_gate.OutputGate(chunk, P.THRESHOLD, SCALE, dtype, ctx=other_ctx)
    n = W.samples_for(frames, fs)
    loud = [Wave(W.voiced_wave(n, fs, s), fs) for s in range(4)]
    plan = [(loud[0], {}, 'card'), (loud[1], {}, 'card'), (loud[2], {}, 'composed'), (Wave(numpy.zeros(n, numpy.float32), fs), dict(gate_first=True), 'card'),
            (loud[3], dict(final=True), 'card'), (loud[0], {}, 'card'), (loud[1], dict(final=True), 'card')]
    routes, emitted, sizes = Routes(), 0, []
    for i, (w, kw, way) in enumerate(plan):
        if way == 'composed':
            monkeypatch.setenv('RY_DEVICE_GATE', '0')
        before = dict(pipeline.calls)
        got = dev.push(w, discard=(1, 1), out_gate=g_dev, **kw).wave
        assert routes.taken() == ((1, 0) if way == 'card' else (0, 1)), (i, way)
        assert pipeline.calls['composed' if way == 'composed' else 'resident'] == before['composed' if way == 'composed' else 'resident'] + 1
        if way == 'card':
            c = g_dev.counts()
            audible = g_dev.last[0] and not g_dev.last[1]
            assert c['sample_bytes_down'] == (chunk * numpy.dtype(dtype).itemsize if audible else 0), (i, c)
        want, raw = by_hand(host, g_host, w, discard=(1, 1), **kw)
        assert routes.taken() == (0, 0)                                     # no gate was handed to the twin's push
        if way == 'card':                                                   # the twin's gate took `raw` samples up, this one none
            assert g_dev.counts()['upload_bytes'] == g_host.counts()['upload_bytes'] - 8 * raw, (i, raw)
        sizes.append(raw)
        if way == 'composed':
            monkeypatch.delenv('RY_DEVICE_GATE')
        assert P.same(got, want), (i, way, got.shape, want.shape)
        assert same_last(g_dev.last, g_host.last) and g_dev.held() == g_host.held(), (i, g_dev.last, g_host.last)
        if third is not None:
            alt = third.push(w, discard=(1, 1), out_gate=g_third, **kw).wave
            assert routes.taken() == (0, 1) and P.same(alt, want), i
        emitted += int(g_dev.last[0])
    assert 2 <= emitted < len(plan), (emitted, sizes)                      # calls that completed a chunk and calls that completed none
    for p in (dev, host, third):
        if p is not None:
            p.close()
    for g in (g_dev, g_host, g_third):
        if g is not None:
            g.close()
    vc._fused_core().set_discard(0, 0)


def check_bank_pipeline(vc, ctx, fs, mode, capacity, frames, chunk, dtype):
    """`PipelineBank.push(out_gate=G)` (B = 3) on the device route against the host route on a twin bank: all streams; stream 1 sits out; stream 2
    silent under gate_first and named final; all again; then stream 0 ends with the call.  Every stream's chunk, `G.last` and `G.held(s)` after
    every call."""
    from yukarin import Wave
    B, seeds = 3, [3, 11, 29]
    param = W.param_of(vc)
    kw = dict(f0_mode='world', f0_fn=W.f0_fn) if mode == 'world' else dict(crepe_capacity=capacity)
    dev, host = [pipeline.PipelineBank(vc, param, B, seeds=seeds, **kw) for _ in range(2)]
    G_dev = output_gate.OutputGateBank(B, chunk, P.THRESHOLD, SCALE, dtype, ctx=ctx)
    G_host = output_gate.OutputGateBank(B, chunk, P.THRESHOLD, SCALE, dtype, ctx=ctx)
    n = W.samples_for(frames, fs)
    loud = lambda s: Wave(W.voiced_wave(n + s, fs, s), fs)
    zeros = Wave(numpy.zeros(n, numpy.float32), fs)
    plan = [([loud(0), loud(1), loud(2)], (), {}), ([loud(3), None, loud(4)], (), {}), ([loud(5), loud(6), zeros], (2,), dict(gate_first=True)),
            ([loud(7), loud(8), loud(9)], (), {}), ([loud(10), loud(11), loud(12)], (0,), {})]
    routes, emitted = Routes(), 0
    for i, (waves, final, extra) in enumerate(plan):
        got = dev.push(waves, discard=(1, 1), final=final, out_gate=G_dev, **extra)
        assert routes.taken() == (1, 0), i
        dc = G_dev.counts()
        outs = host.push(waves, discard=(1, 1), final=final, **extra)
        want = G_host.push([o.wave for o in outs])
        hc = G_host.counts()
        assert dc['upload_bytes'] == hc['upload_bytes'] - 8 * sum(o.wave.size for o in outs), (i, dc, hc)
        assert dc['sample_bytes_down'] == hc['sample_bytes_down'], (i, dc, hc)
        for s in range(B):
            w = want[s] if want[s] is not None else numpy.empty(0, G_host.dtype)
            assert P.same(got[s].wave, w), (i, s)
            assert same_last(G_dev.last[s], G_host.last[s]) and G_dev.held(s) == G_host.held(s), (i, s)
            emitted += int(G_dev.last[s][0])
    # the synthesizer bank brought no sample down: one download fewer than the twin's last call, the same launches
    dsc, hsc = dev.bank.counts(), host.bank.counts()
    assert dsc['d2h'] == hsc['d2h'] - 1 and dsc['launches'] == hsc['launches'], (dsc, hsc)
    assert emitted >= 3, emitted
    # a flush of every stream without a wave is no resident call: the host route
    got = dev.push([None] * B, final=(1, 2), out_gate=G_dev)
    assert routes.taken() == (0, 1)
    want = G_host.push([o.wave for o in host.push([None] * B, final=(1, 2))])
    for s in range(B):
        assert P.same(got[s].wave, want[s] if want[s] is not None else numpy.empty(0, G_host.dtype)), s
    for p in (dev, host, G_dev, G_host):
        p.close()
    vc._fused_core().set_discard(0, 0)


def check_counters(vc, ctx, fs, frames, chunk=1025, dtype=numpy.float32):
    """Test 3 on one lone WORLD-mode stream: after a resident push with a device gate the route counter says 'gate_device', the gate's one upload
    holds no sample (its size does not depend on how many the synthesizer emitted), and `sample_bytes_down` is chunk x itemsize on an emitted
    audible chunk and 0 on an incomplete or a silent one."""
    from yukarin import Wave
    pipe = lone_pair(vc, 'world', None)[0]
    g = output_gate.OutputGate(chunk, P.THRESHOLD, SCALE, dtype, ctx=ctx)
    n = W.samples_for(frames, fs)
    before = dict(pipeline.routes)
    seen, table = set(), None
    for i in range(6):
        out = pipe.push(Wave(W.voiced_wave(n, fs, i), fs), discard=(1, 1), out_gate=g).wave
        c = g.counts()
        audible = g.last[0] and not g.last[1]
        assert c['uploads'] == 1 and c['sample_bytes_down'] == (chunk * numpy.dtype(dtype).itemsize if audible else 0), (i, c)
        assert out.size == (chunk if audible else 0) and out.dtype == numpy.dtype(dtype)
        table = c['upload_bytes'] if table is None else table
        assert c['upload_bytes'] == table and table < 8 * 64, (i, c)       # the first push emits a few samples, the later ones hundreds: the same bytes
        seen.add(audible)
    assert seen == {True, False}
    assert pipeline.routes['gate_device'] == before['gate_device'] + 6 and pipeline.routes['gate_host'] == before['gate_host']
    assert 'y' in pipe._blocks and pipe._blocks['w_y'] >= pipe.synth.bound(frames - 2)
    pipe.close()
    assert pipe._blocks == {}
    g.close()
    vc._fused_core().set_discard(0, 0)


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------------------------
def check_lone_refusals(ctx):
    """Every refusal of `ry_synth_push_dev` / `ry_synth_flush_dev` by return code: the block keeps the pattern, `ry_synth_bound` says what it said,
    and the stream goes on with the twin's bits."""
    dll = ctx.lib.dll
    dev = world_synth.Synthesizer(FS, PERIOD, seed=7, ctx=ctx)
    host = world_synth.Synthesizer(FS, PERIOD, seed=7, ctx=ctx)
    _, h = dev._get()
    item = S.case('glide', 60, FS)
    first, second = pieces(item, (30, 30))
    blk = Poisoned(ctx, 8192)
    y, n_out = ctypes.cast(ctypes.c_void_p(blk.address), DP), ctypes.c_longlong(-5)
    f = _lib._fptr
    null_d, null_f = ctypes.cast(ctypes.c_void_p(0), DP), f(None)

    def push(piece, h=h, y=y, cap=8192, out=ctypes.byref(n_out), bins=S.BINS, n=None, f0=None, sp=None, ap=None):
        f0 = numpy.ascontiguousarray(piece[0], numpy.float64) if f0 is None else f0
        return dll.ry_synth_push_dev(h, f0.ctypes.data_as(DP) if f0 is not False else null_d, f(piece[1]) if sp is None else sp,
                                     f(piece[2]) if ap is None else ap, len(piece[0]) if n is None else n, bins, 0, y, cap, out)

    def refused_everything(piece):
        bound = dev.bound(len(piece[0])), dev.bound(0, True)
        bad = numpy.array(piece[0], numpy.float64)
        bad[3] = numpy.nan
        half = numpy.array(piece[0], numpy.float64)
        half[5] = FS / 2
        assert push(piece, h=None) == -4
        assert push(piece, y=null_d) == -1 and push(piece, out=None) == -1 and push(piece, cap=-1) == -1
        assert push(piece, bins=512) == -1
        assert push(piece, f0=False) == -1 and push(piece, sp=null_f) == -1 and push(piece, ap=null_f) == -1
        assert push(piece, n=0) == -1 and push(piece, n=-3) == -1 and push(piece, n=(1 << 22) + 1) == -1
        assert push(piece, f0=bad) == -1 and b'f0[3]' in dll.ry_last_error()
        assert push(piece, f0=half) == -1 and b'f0[5]' in dll.ry_last_error()
        if bound[0] > 0:
            assert push(piece, cap=bound[0] - 1) == -1 and b'ry_synth_bound' in dll.ry_last_error()
        assert (dev.bound(len(piece[0])), dev.bound(0, True)) == bound and blk.untouched()
    assert dll.ry_synth_flush_dev(h, y, 8192, ctypes.byref(n_out)) == -4            # an empty stream
    refused_everything(first)
    want = host.push(*first)
    assert push(first) == 0 and n_out.value == want.size and blk.holds_only(0, want)
    blk.poison()
    refused_everything(second)
    rest = dev.bound(0, True)
    assert dll.ry_synth_flush_dev(None, y, 8192, ctypes.byref(n_out)) == -4
    assert dll.ry_synth_flush_dev(h, null_d, 8192, ctypes.byref(n_out)) == -1 and dll.ry_synth_flush_dev(h, y, 8192, None) == -1
    assert dll.ry_synth_flush_dev(h, y, -1, ctypes.byref(n_out)) == -1 and dll.ry_synth_flush_dev(h, y, rest - 1, ctypes.byref(n_out)) == -1
    assert dev.bound(0, True) == rest and blk.untouched()
    want = host.push(*second)
    assert push(second) == 0 and n_out.value == want.size and blk.holds_only(0, want)
    rest = dev.bound(0, True)
    tail = host.flush()
    blk.poison()
    assert dll.ry_synth_flush_dev(h, y, rest, ctypes.byref(n_out)) == 0 and n_out.value == tail.size and blk.holds_only(0, tail)
    blk.close()
    dev.close()
    host.close()


def check_bank_refusals(ctx):
    """Every refusal of `ry_synth_bank_push_dev`: block, offsets, window rows, bounds and the counters of the last good push stay as they were."""
    dll = ctx.lib.dll
    B, seeds = 3, [3, 11, 29]
    dev = world_synth.StreamBank(FS, PERIOD, n_streams=B, seeds=seeds, ctx=ctx)
    host = world_synth.StreamBank(FS, PERIOD, n_streams=B, seeds=seeds, ctx=ctx)
    _, h = dev._get()
    items = [S.case('glide', 20, FS), S.case('voiced71', 12, FS), None]
    blk = Poisoned(ctx, 8192)
    want = host.push(items)
    off = dev.push_device(items, (), blk.block)
    assert blk.holds_only(0, numpy.concatenate(want)) and off[-1] > 0
    blk.poison()
    f0 = numpy.ascontiguousarray(numpy.concatenate([items[0][0], items[1][0]]))
    sp, ap = numpy.concatenate([items[0][1], items[1][1]]), numpy.concatenate([items[0][2], items[1][2]])
    y = ctypes.cast(ctypes.c_void_p(blk.address), DP)
    offsets = numpy.full(B + 1, -7, numpy.int64)
    f = _lib._fptr
    null_d = ctypes.cast(ctypes.c_void_p(0), DP)

    def push(h=h, f0=f0, n=(20, 12, 0), fin=(0, 0, 0), y=y, cap=8192, bins=S.BINS, off=offsets, sp=f(sp), ap=f(ap)):
        n, fin = numpy.array(n, numpy.int32), numpy.array(fin, numpy.int32)
        return dll.ry_synth_bank_push_dev(h, f0.ctypes.data_as(DP) if f0 is not None else null_d, sp, ap, n.ctypes.data_as(IP) if n.size else None,
                                          fin.ctypes.data_as(IP), bins, 0, y, cap, off.ctypes.data_as(LLP) if off is not None else None)
    state = lambda: ([dev.rows(b) for b in range(B)], [dev.bound(b, 5, False) for b in range(B)], [dev.bound(b, 0, True) for b in range(B)], dev.counts())
    before = state()
    bad = f0.copy()
    bad[25] = numpy.inf
    need = dev.bound(0, 20) + dev.bound(1, 12)
    assert push(h=None) == -4
    assert push(y=null_d) == -1 and push(off=None) == -1 and push(f0=None) == -1 and push(sp=f(None)) == -1 and push(ap=f(None)) == -1
    assert push(n=()) == -1 and push(bins=512) == -1
    assert push(n=(20, -1, 0)) == -1 and push(n=(0, 0, 0)) == -1
    assert push(n=(20, 12, 0), fin=(0, 0, 1)) == -4                         # final on a stream without a frame
    assert push(f0=bad) == -1 and b'stream 1' in dll.ry_last_error() and b'f0[5]' in dll.ry_last_error()
    assert need > 0 and push(cap=need - 1) == -1 and b'ry_synth_bank_bound' in dll.ry_last_error()
    assert state() == before and blk.untouched() and (offsets == -7).all()
    want = host.push(items, (0,))
    off = dev.push_device(items, (0,), blk.block)
    assert off.tolist() == [0] + numpy.cumsum([w.size for w in want]).tolist() and blk.holds_only(0, numpy.concatenate(want))
    blk.close()
    dev.close()
    host.close()
