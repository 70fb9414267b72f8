"""Bodies the emulator and the GPU tests of `pipeline.LivePipeline` share (test_live_pipeline_cpu.py, test_live_pipeline_gpu.py).  The yardstick of
every comparison is the pipeline's own composed path -- the same plans applied to host arrays over the separate calls
(`LivePipeline(resident=False)`) -- and every comparison is bit equality (`pipeline_cases.same`).  SYN-8 predictors (tests/pipeline_cases.py);
WORLD mode runs the deterministic f0 callable of tests/pipeline_world_cases.py."""
import numpy

import pipeline_cases as P
import pipeline_world_cases as W
from realtime_yukarin_amd import pipeline

FEATURE_ROWS = ('mc', 'sp', 'ap')


def buffers_of(fs, time_length, n, zero_at=None, seed=0):
    """n buffers of time_length seconds cut from one loud wave; buffer `zero_at` is exact zeros (the gate cuts all of its frames)."""
    size = round(time_length * fs)
    x = P.wave_of('loud', fs, time_length * n + 0.01, seed)
    out = [x[k * size:(k + 1) * size].copy() for k in range(n)]
    if zero_at is not None:
        out[zero_at][:] = 0
    return out


def make(vc, mode, capacity, time_length, margins, **kw):
    args = dict(f0_mode='world', f0_fn=W.f0_fn) if mode == 'world' else dict(f0_mode='crepe', crepe_capacity=capacity)
    return pipeline.LivePipeline(vc, W.param_of(vc), time_length, margins[0], margins[1], margins[2], seed=3, **args, **kw)


def run(live, buffers, out_gate=None):
    """Every push and the flush -> (waves, the `transfers` record of every push, (ring position, rows, ring rows) of every push's segment)."""
    waves, transfers, positions = [], [], []
    for b in buffers:
        waves.append(live.push(b, out_gate=out_gate).wave)
        transfers.append(list(live.transfers))
        store = live._store
        positions.append((store.segments[-1].row_pos, store.segments[-1].rows, store.cap_rows) if store is not None and store.segments else None)
    waves.append(live.flush().wave)
    return waves, transfers, positions


def check_resident_equals_composed(vc, fs, mode, capacity, time_length, margins, n_push, ring_rows=None, ring_samples=None, zero_at=None,
                                   wraps_by=None):
    bufs = buffers_of(fs, time_length, n_push, zero_at)
    ref = make(vc, mode, capacity, time_length, margins, resident=False)
    before = dict(pipeline.calls)
    want, _, _ = run(ref, bufs)
    assert pipeline.calls['composed'] == before['composed'] + n_push and pipeline.calls['resident'] == before['resident']
    ref.close()
    live = make(vc, mode, capacity, time_length, margins, ring_rows=ring_rows, ring_samples=ring_samples)
    before = dict(pipeline.calls)
    got, transfers, positions = run(live, bufs)
    assert pipeline.calls['resident'] == before['resident'] + n_push and pipeline.calls['composed'] == before['composed'], pipeline.calls
    assert len(got) == len(want) == n_push + 1
    for k, (g, w) in enumerate(zip(got, want)):
        assert P.same(g, w), (k, g.shape, w.shape)
    assert sum(w.size for w in want) > 0
    for t in transfers:                                   # the wave goes up once, no feature row crosses the bus
        assert sum(1 for d, what, _ in t if (d, what) == ('up', 'wave')) == 1, t
        assert not any(what in FEATURE_ROWS for _, what, _ in t), t
        assert sum(n for d, what, n in t if d == 'up' and what == 'table') <= 64 * 8, t
    if wraps_by is not None:                              # the ring has wrapped: one of the first `wraps_by` segments crosses or restarts at its end
        assert any(pos + rows >= cap for pos, rows, cap in positions[:wraps_by]), positions
    # a second signal after the flush starts from the first clocks and gives the first signal's bits
    again, _, _ = run(live, bufs[:2])
    ref = make(vc, mode, capacity, time_length, margins, resident=False)
    want2, _, _ = run(ref, bufs[:2])
    assert all(P.same(g, w) for g, w in zip(again, want2))
    ref.close()
    live.close()
    vc._fused_core().set_discard(0, 0)


def check_decode_margin_takes_the_composed_path(vc, fs, mode, capacity, time_length, margins, n_push):
    """A decode margin above 0: the decode window reaches rows of earlier buffers, the call is composed and counted so, and the bits are the
    yardstick's."""
    assert margins[2] > 0
    bufs = buffers_of(fs, time_length, n_push)
    ref = make(vc, mode, capacity, time_length, margins, resident=False)
    want, _, _ = run(ref, bufs)
    ref.close()
    live = make(vc, mode, capacity, time_length, margins)
    before = dict(pipeline.calls)
    got, _, _ = run(live, bufs)
    assert pipeline.calls['composed'] == before['composed'] + n_push and pipeline.calls['resident'] == before['resident']
    assert all(P.same(g, w) for g, w in zip(got, want)) and sum(w.size for w in want) > 0
    live.close()
    vc._fused_core().set_discard(0, 0)


def check_out_gate(vc, fs, ctx, mode, capacity, time_length, margins, n_push, chunk):
    """`out_gate=`: the resident path hands the samples to the gate on the card (`routes['gate_device']`), the composed path through the host; the
    chunks are the same."""
    from realtime_yukarin_amd import output_gate
    bufs = buffers_of(fs, time_length, n_push)
    outs = {}
    for resident in (False, True):
        gate = output_gate.OutputGate(chunk, P.THRESHOLD, 0.5, numpy.float32, ctx=ctx)
        live = make(vc, mode, capacity, time_length, margins, resident=resident)
        before = dict(pipeline.routes)
        outs[resident] = [live.push(b, out_gate=gate).wave for b in bufs]
        key = 'gate_device' if resident and gate.on_device() else 'gate_host'
        assert pipeline.routes[key] == before[key] + n_push, (pipeline.routes, before)
        live.flush()
        live.close()
        gate.close()
    assert all(P.same(a, b) for a, b in zip(outs[True], outs[False]))
    assert all(o.dtype == numpy.float32 and o.size in (0, chunk) for o in outs[True]) and sum(o.size for o in outs[True]) > 0
    vc._fused_core().set_discard(0, 0)
