"""One fixed sequence of window calls for tests/test_stream_forms.py (emulator) and tests/test_stream_forms_gpu.py (children on the GPU):
every entry point that follows the stream topology of the lanes (ry_vc_submit / ry_vc_wait, ry_vc_enqueue_device, ry_vc_submit_wave,
ry_vc_enqueue_device_batch), consecutive windows on the first two (thirteen each on the GPU, where every one of the six ring slots is used again
behind a window still in flight; the emulator, half a second per window, takes seven and three: every slot is used again once), one window with a
silent stretch among them.  `run` returns {name: array}: two runs that differ only in the lane count
or in RY_VC_STREAMS must return the same bits.  As a program (the GPU test starts it in a fresh process, because the HIP runtime reads
GPU_MAX_HW_QUEUES when it starts): stream_forms_scenario.py OUT_DIR MODEL FRAMES [MODEL FRAMES ...] writes one .npz per (model, frames, lanes, form)."""
import os
import sys
from pathlib import Path

import numpy

N_WINDOWS = 13          # on the GPU: two rounds of the six ring slots and one more
GATED = 4               # this window has a silent stretch in the middle


def windows(n, count=N_WINDOWS):
    from realtime_yukarin_amd import synth
    out = []
    for i in range(count):
        x = synth.stage1_input(n, seed=700 + i)[0]
        eff = numpy.ones(n, bool)
        if i == GATED:
            eff[n // 4:n // 4 + max(1, n // 3)] = False
        out.append((numpy.ascontiguousarray(x[eff]), eff))
    return out


def run(ctx, name, n, lanes, form, count=N_WINDOWS, dev_count=N_WINDOWS, waves=3, batches=2):
    """form: 'wide' / 'compact' / 'compact-a' / 'compact-b' (RY_VC_STREAMS while the core is made) or None (chosen from GPU_MAX_HW_QUEUES)."""
    import window_call_ref as wr
    from realtime_yukarin_amd import engine, synth
    old = os.environ.pop('RY_VC_STREAMS', None)
    if form is not None:
        os.environ['RY_VC_STREAMS'] = form
    n1, n2 = wr.make_pair(ctx, name)
    try:
        core = engine.VcCore(n1, n2, wr.mtx(name), lanes=lanes)
    finally:
        os.environ.pop('RY_VC_STREAMS', None)
        if old is not None:
            os.environ['RY_VC_STREAMS'] = old
    blocks = wr.Blocks(ctx)
    out = {}
    try:
        M, F = core.M, core.F
        wins = windows(n, count)
        # host windows, as many in flight as the ring holds
        for i, (mc, sp) in enumerate(core.convert_stream(wins, depth=core.ring)):
            out['host_mc_%02d' % i], out['host_sp_%02d' % i] = mc, sp
        # device pointers, nothing waited for until the end: every window has result blocks of its own
        res = []
        for x, e in wins[::-1][:dev_count]:
            rows = numpy.nonzero(e)[0].astype(numpy.int32)
            res.append((blocks.put(x), blocks.put(rows.view(numpy.float32)), len(x),
                        blocks.alloc(n * M, fill=wr.SENTINEL), blocks.alloc(n * F, fill=wr.SENTINEL)))
        ctx.sync()
        for d_x, d_r, n_eff, d_mc, d_sp in res:
            core.enqueue_device(d_x, d_r, n_eff, n, d_mc, d_sp)
        ctx.sync()
        for i, (_, _, _, d_mc, d_sp) in enumerate(res):
            out['dev_mc_%02d' % i], out['dev_sp_%02d' % i] = blocks.get(d_mc, (n, M)), blocks.get(d_sp, (n, F))
        # the gate on the device
        tickets = []
        for i in range(waves):
            w, feat, _ = wr.wave_window(n, 40 + i)
            tickets.append(core.submit_wave(w, *wr.gate_args(), feat))
        for i, t in enumerate(tickets):
            mc, sp, mask = core.wait_wave(t)
            out['wave_mc_%d' % i], out['wave_sp_%d' % i], out['wave_mask_%d' % i] = mc, sp, numpy.asarray(mask)
        # two windows in one call, twice (both buffer sets), one of them gated
        pair = [wins[GATED], wins[0]]
        d_x = blocks.put(numpy.concatenate([x for x, _ in pair]))
        d_r = blocks.put(numpy.concatenate([numpy.nonzero(e)[0] for _, e in pair]).astype(numpy.int32).view(numpy.float32))
        for rep in range(batches):
            d_mc, d_sp = blocks.alloc(2 * n * M, fill=wr.SENTINEL), blocks.alloc(2 * n * F, fill=wr.SENTINEL)
            core.enqueue_device_batch(d_x, d_r, [len(x) for x, _ in pair], n, d_mc, d_sp)
            ctx.sync()
            out['batch_mc_%d' % rep], out['batch_sp_%d' % rep] = blocks.get(d_mc, (2, n, M)), blocks.get(d_sp, (2, n, F))
        form_used, n_streams = core.debug_streams()
        out['form'] = numpy.array(engine.VcCore.STREAM_FORMS.index(form_used))
        out['n_streams'] = numpy.array(n_streams)
        assert synth.MC_DIMS == M
    finally:
        blocks.free(); core.close(); n1.close(); n2.close()
    return out


COMBOS = ((1, 'wide'), (2, 'wide'), (2, 'compact-a'), (2, 'compact-b'), (2, None))


def main(argv):
    here = Path(__file__).resolve().parent
    sys.path[:0] = [str(here), str(here.parent)]
    from realtime_yukarin_amd import engine
    out_dir = Path(argv[0]); out_dir.mkdir(parents=True, exist_ok=True)
    ctx = engine.get_context(0)
    for name, n in zip(argv[1::2], argv[2::2]):
        for lanes, form in COMBOS:
            numpy.savez(str(out_dir / ('%s_%s_l%d_%s.npz' % (name, n, lanes, form or 'auto'))), **run(ctx, name, int(n), lanes, form))
    print('done')


if __name__ == '__main__':
    main(sys.argv[1:])
