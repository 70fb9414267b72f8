"""Bodies the emulator and the GPU tests of `pipeline.LivePipelineBank` share (test_live_bank_cpu.py, test_live_bank_gpu.py).  The yardstick of
every comparison is B lone `pipeline.LivePipeline`s with the bank's seeds, fed the same buffers and flushed at the same points, and every
comparison is bit equality (`pipeline_cases.same`).  A run is a list of events: ('push', the streams that take part) -- every stream takes its
own next buffer, so a stream that sits a call out falls behind the others -- and ('flush', a stream, or None for all)."""
import numpy

import live_pipeline_cases as L
import pipeline_cases as P
import pipeline_world_cases as W
from realtime_yukarin_amd import pipeline

SEEDS = (3, 11, 29, 5)


def signals(fs, time_length, n, B, zero=(0, 2)):
    """n buffers per stream, every stream cut from its own loud wave; buffer zero[1] of stream zero[0] is exact zeros."""
    return [L.buffers_of(fs, time_length, n, zero[1] if zero is not None and b == zero[0] else None, seed=b) for b in range(B)]


def events_of(n_push, B, sit_out=None, flush=None):
    """n_push calls; sit_out = (stream, call): that stream has no buffer in that call; flush = (stream, call): flushed behind that call."""
    out = []
    for k in range(n_push):
        out.append(('push', [b for b in range(B) if (b, k) != sit_out]))
        if flush is not None and flush[1] == k:
            out.append(('flush', flush[0]))
    return out + [('flush', None)]


def make_args(mode, capacity, fn=None):
    return dict(f0_mode='world', f0_fn=fn or W.f0_fn) if mode == 'world' else dict(f0_mode='crepe', crepe_capacity=capacity)


def run_lone(vc, b, bufs, events, mode, capacity, time_length, margins, gate=None, fn=None, **kw):
    live = pipeline.LivePipeline(vc, W.param_of(vc), time_length, margins[0], margins[1], margins[2], seed=SEEDS[b], **make_args(mode, capacity, fn), **kw)
    got, taken = [], 0
    for kind, arg in events:
        if kind == 'push' and b in arg:
            got.append(live.push(bufs[taken], out_gate=gate).wave)
            taken += 1
        elif kind == 'flush' and arg in (None, b):
            got.append(live.flush().wave)
    live.close()
    return got


def run_bank(bank, bufs, events, out_gate=None):
    """-> (per stream the waves its events returned, the `transfers` of every push, the streams of every push)."""
    B = bank.n_streams
    got, taken, transfers = [[] for _ in range(B)], [0] * B, []
    for kind, arg in events:
        if kind == 'push':
            items = [None] * B
            for b in arg:
                items[b], taken[b] = bufs[b][taken[b]], taken[b] + 1
            outs = bank.push(items, out_gate=out_gate)
            assert len(outs) == B
            for b in range(B):
                if b in arg:
                    got[b].append(outs[b].wave)
                else:
                    assert outs[b].wave.size == 0
            transfers.append((list(bank.transfers), list(arg)))
        elif arg is None:
            for b, o in enumerate(bank.flush()):
                got[b].append(o.wave)
        else:
            got[arg].append(bank.flush(arg).wave)
    return got, transfers


def make_bank(vc, B, mode, capacity, time_length, margins, fn=None, **kw):
    return pipeline.LivePipelineBank(vc, W.param_of(vc), B, time_length, margins[0], margins[1], margins[2], seeds=SEEDS[:B], **make_args(mode, capacity, fn), **kw)


def assert_same(got, want):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (b, len(g), len(w))
        for k, (x, y) in enumerate(zip(g, w)):
            assert P.same(x, y), (b, k, x.shape, y.shape)
    assert all(sum(x.size for x in w) > 0 for w in want)


def check_bank_equals_lone(vc, fs, mode, capacity, time_length, margins, n_push, B, ring_rows=None, ring_samples=None, sit_out=None, flush=None,
                           zero=(0, 2), kept_rows=None):
    """Every stream of the bank against its lone pipeline; every (stream, push) is counted resident; the windows of a call go up in one
    upload and no feature row crosses the bus."""
    bufs = signals(fs, time_length, n_push, B, zero)
    events = events_of(n_push, B, sit_out, flush)
    rings = dict(ring_rows=ring_rows, ring_samples=ring_samples)
    want = [run_lone(vc, b, bufs[b], events, mode, capacity, time_length, margins, **rings) for b in range(B)]
    bank = make_bank(vc, B, mode, capacity, time_length, margins, **rings)
    before = dict(pipeline.calls)
    got, transfers = run_bank(bank, bufs, events)
    pushes = sum(len(arg) for kind, arg in events if kind == 'push')
    assert pipeline.calls['resident'] == before['resident'] + pushes and pipeline.calls['composed'] == before['composed'], (pipeline.calls, before)
    assert_same(got, want)
    for t, part in transfers:
        assert sum(1 for d, what, _ in t if (d, what) == ('up', 'wave')) == 1, t
        assert not any(what in L.FEATURE_ROWS for _, what, _ in t), t
        if kept_rows is not None:                         # per stream: the single stream's bound on its piece tables, and an index per kept row
            assert sum(n for d, what, n in t if d == 'up' and what == 'table') <= len(part) * (64 * 8 + kept_rows), t
    # a second signal after the flush of all starts from the first clocks
    again, _ = run_bank(bank, bufs, events_of(2, B))
    assert_same(again, [run_lone(vc, b, bufs[b], events_of(2, B), mode, capacity, time_length, margins, **rings) for b in range(B)])
    bank.close()
    vc._fused_core().set_discard(0, 0)


def check_decode_margin_is_composed(vc, fs, mode, capacity, time_length, margins, n_push, B):
    """A decode margin above 0 sends every stream down the composed path through its slot of the stream bank: counted so, the lone bits."""
    assert margins[2] > 0
    bufs = signals(fs, time_length, n_push, B, None)
    events = events_of(n_push, B)
    want = [run_lone(vc, b, bufs[b], events, mode, capacity, time_length, margins) for b in range(B)]
    bank = make_bank(vc, B, mode, capacity, time_length, margins)
    before = dict(pipeline.calls)
    got, _ = run_bank(bank, bufs, events)
    assert pipeline.calls['composed'] == before['composed'] + B * n_push and pipeline.calls['resident'] == before['resident']
    assert_same(got, want)
    bank.close()
    vc._fused_core().set_discard(0, 0)


def check_a_misfit_demotes_one_stream(vc, fs, time_length, margins, n_push):
    """WORLD mode, B = 2: the f0 callable returns a frame too many for the windows of stream 1 only (told by their first sample).  Stream 1 is
    composed from its first buffer on, stream 0 stays in the resident chain, and both return their lone bits."""
    bufs = signals(fs, time_length, n_push, 2, None)
    marked = set(float(x[0]) for x in bufs[1])
    assert not marked & set(float(x[0]) for x in bufs[0])
    fn = lambda x, *a: (W.wrong_count_fn if float(x[0]) in marked else W.f0_fn)(x, *a)
    events = events_of(n_push, 2)
    want = [run_lone(vc, b, bufs[b], events, 'world', None, time_length, margins, fn=fn) for b in range(2)]
    bank = make_bank(vc, 2, 'world', None, time_length, margins, fn=fn)
    before = dict(pipeline.calls)
    got, _ = run_bank(bank, bufs, events)
    assert pipeline.calls['resident'] == before['resident'] + n_push and pipeline.calls['composed'] == before['composed'] + n_push, (pipeline.calls, before)
    assert bank._states[0].mode is None and bank._store is not None           # (flushed) -- and stream 0 went through the row bank
    assert_same(got, want)
    bank.close()
    vc._fused_core().set_discard(0, 0)


def check_out_gate(vc, fs, ctx, mode, capacity, time_length, margins, n_push, B, chunk):
    """`out_gate=`: one `OutputGateBank` call per push -- on the card where the gates judge there, else through the host -- and every stream's
    chunks are those of its lone pipeline with a lone gate."""
    from realtime_yukarin_amd import output_gate
    bufs = signals(fs, time_length, n_push, B, None)
    events = events_of(n_push, B)
    want = []
    for b in range(B):
        gate = output_gate.OutputGate(chunk, P.THRESHOLD, 0.5, numpy.float32, ctx=ctx)
        want.append(run_lone(vc, b, bufs[b], events, mode, capacity, time_length, margins, gate=gate))
        gate.close()
    gates = output_gate.OutputGateBank(B, chunk, P.THRESHOLD, 0.5, numpy.float32, ctx=ctx)
    bank = make_bank(vc, B, mode, capacity, time_length, margins)
    before = dict(pipeline.routes)
    got, _ = run_bank(bank, bufs, events, out_gate=gates)
    key = 'gate_device' if gates.on_device() else 'gate_host'
    other = 'gate_host' if key == 'gate_device' else 'gate_device'
    assert pipeline.routes[key] == before[key] + n_push and pipeline.routes[other] == before[other], (pipeline.routes, before)    # per call, not per stream
    assert_same(got, want)
    assert all(o.dtype == numpy.float32 and o.size in (0, chunk) for g in got for o in g[:-1])
    bank.close()
    gates.close()
    vc._fused_core().set_discard(0, 0)
    return key
