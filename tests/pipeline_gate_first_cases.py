"""Cases the emulator and the GPU tests of the gate-first form of the wave-to-wave chain share (test_pipeline_gate_first_cpu.py,
test_pipeline_gate_first_gpu.py).  The yardstick of every comparison is the same call with the flag off in the same process -- a second, fresh
`Pipeline` / `PipelineBank` with the same seeds, `ry_vc_gate_waves_device` for the compaction, `ry_crepe_track_many` for the split tracker entries --
and every comparison is bit equality (`pipeline_cases.same`).  The waves: audible ('loud'), two silent ones (digital zeros, noise of 1e-6) and a
barely audible one whose impulses give exactly ONE effective frame; every test asserts those counts against the host gate before it compares."""
import ctypes

import numpy

import pipeline_cases as P
import pipeline_many_cases as M
from realtime_yukarin_amd import _lib, crepe, gate, pipeline

UB, IP, LLP = M.UB, M.IP, M.LLP


# ---- the waves ----------------------------------------------------------------------------------------------------------------------------
def wave_of(kind: str, fs: int, seconds: float, seed: int = 0) -> numpy.ndarray:
    """'loud' (pipeline_cases); 'zeros'; 'noise': normal noise of 1e-6; 'barely': impulses (0.02, or 0.027 each where there are two) placed so that exactly one gate window holds
    enough of them -- one impulse near the start of a wave shorter than a gate window (only the last frame's reflected window counts it twice), two
    impulses 964 samples apart in a longer one (one frame's window of 1024 holds both, every other at most one)."""
    n = int(round(seconds * fs))
    if kind == 'loud':
        return P.wave_of('loud', fs, seconds, seed)
    x = numpy.zeros(n, numpy.float32)
    if kind == 'noise':
        x[:] = (1e-6 * numpy.random.default_rng([seed, n]).normal(size=n)).astype(numpy.float32)
    elif kind == 'barely':
        if n < 1600:
            x[5] = 0.02
        else:
            x[950] = x[1914] = 0.027
    else:
        assert kind == 'zeros', kind
    return x


COUNTS = {'zeros': 0, 'noise': 0, 'barely': 1}


def n_eff_of(x, fs) -> int:
    """The host gate's count (`oracle/effective_frame.py` states the same rule; `pipeline_cases.host_mask` is the form the chain itself uses) over
    the frames the tracker gives the wave."""
    return int(P.host_mask(x, fs, crepe.track_frames(x.size, fs, crepe.hop_length(P.FRAME_PERIOD))).sum())


def check_counts(fs, seconds):
    """The inputs are what their names say, so that a drifting input cannot turn a test into a no-op."""
    from oracle import effective_frame
    for kind, want in COUNTS.items():
        x = wave_of(kind, fs, seconds)
        assert n_eff_of(x, fs) == want, (kind, n_eff_of(x, fs))
        n = crepe.track_frames(x.size, fs, crepe.hop_length(P.FRAME_PERIOD))
        m = effective_frame.separate_effective_mask(x, fs, n, P.THRESHOLD, 1024, P.FRAME_PERIOD)
        assert int(numpy.asarray(m).sum()) == want, (kind, 'oracle')
    x = wave_of('loud', fs, seconds)
    assert n_eff_of(x, fs) == crepe.track_frames(x.size, fs, crepe.hop_length(P.FRAME_PERIOD))


def W(kind, fs, seconds, seed=0):
    from yukarin import Wave
    return Wave(wave_of(kind, fs, seconds, seed), fs)


def overlapping(fs, seconds, advance, count, seed=0):
    """`count` windows of one long loud signal, each `advance` samples behind the one before: their overlaps hold the same samples."""
    n = int(round(seconds * fs))
    long = P.wave_of('loud', fs, (n + advance * count) / fs + 0.01, seed)
    return [long[i * advance:i * advance + n].copy() for i in range(count)]


# ---- 1: a lone pipeline ---------------------------------------------------------------------------------------------------------------------
def make_pair(vc, capacity, seed=3):
    param = vc.acoustic_converter.config.dataset.acoustic_param
    return (pipeline.Pipeline(vc, param, crepe_capacity=capacity, seed=seed, gate_first=True),
            pipeline.Pipeline(vc, param, crepe_capacity=capacity, seed=seed))


def check_lone(vc, capacity, fs, seconds, advance, discard, out_gates=None, kept=False):
    """`convert_wave` of every kind, then the push sequence audible, silent, silent, audible, silent and a flush, flag on against flag off.  kept:
    the windows are long enough for frames a tracker may keep, so the audible buffer behind the two skipped ones must report fewer computed frames
    than it has -- its advance spans three buffers and is still shorter than the window."""
    from yukarin import Wave
    on, off = make_pair(vc, capacity)
    assert on.gate_first and not off.gate_first
    for kind in ('loud', 'zeros', 'noise', 'barely'):
        w = W(kind, fs, seconds)
        assert P.same(on.convert_wave(w).wave, off.convert_wave(w).wave), kind
        assert on.last_gate['tracked'] == [kind in ('loud', 'barely')] and on.last_gate['n_eff'] == [n_eff_of(w.wave, fs)], (kind, on.last_gate)
    assert P.same(off.convert_wave(W('loud', fs, seconds), gate_first=True).wave, on.convert_wave(W('loud', fs, seconds), gate_first=False).wave)
    a = None if advance is None else int(advance)
    windows = overlapping(fs, seconds, a or 1, 5)
    kinds = ('loud', 'zeros', 'noise', 'loud', 'zeros')
    waves = [Wave(x if k == 'loud' else wave_of(k, fs, seconds, i), fs) for i, (k, x) in enumerate(zip(kinds, windows))]
    gated = pipeline.calls.get('gated', 0)
    for i, w in enumerate(waves):
        extra = {} if a is None else dict(advance=a)
        gates = {} if out_gates is None else dict(out_gate=out_gates[0])
        gates_off = {} if out_gates is None else dict(out_gate=out_gates[1])
        got, want = on.push(w, discard=discard, **extra, **gates), off.push(w, discard=discard, **extra, **gates_off)
        assert P.same(got.wave, want.wave), (i, kinds[i])
        assert on.last_gate['tracked'] == [kinds[i] == 'loud']
        if a is not None:
            n = crepe.track_frames(w.wave.size, fs, crepe.hop_length(P.FRAME_PERIOD))
            c = on.last_gate['n_computed'][0]
            assert c == (n if i == 0 else None if kinds[i] != 'loud' else c), (i, c)
            if i == 3:
                assert 0 < c <= n, (i, c, n)
                if kept:
                    assert 3 * a < w.wave.size and c < n, (c, n)           # the rows were kept and the skipped advances accumulated
    assert pipeline.calls['gated'] - gated == 3
    assert P.same(on.flush().wave, off.flush().wave)
    if a is not None:
        n = crepe.track_frames(waves[0].wave.size, fs, crepe.hop_length(P.FRAME_PERIOD))
        assert on._gate_bank.frames[0] == n
    on.close()
    off.close()


def check_lone_kept_rows(vc, capacity, fs, seconds, advance):
    """The accumulated advance alone, at the smallest size that shows it: audible, silent, silent, audible through a lone pipeline with `advance`, flag
    on against flag off; the last buffer goes through the network with fewer frames than it has."""
    from yukarin import Wave
    on, off = make_pair(vc, capacity)
    windows = overlapping(fs, seconds, advance, 4)
    kinds = ('loud', 'zeros', 'noise', 'loud')
    n = crepe.track_frames(windows[0].size, fs, crepe.hop_length(P.FRAME_PERIOD))
    assert 3 * advance < windows[0].size
    for i, (k, x) in enumerate(zip(kinds, windows)):
        w = Wave(x if k == 'loud' else wave_of(k, fs, seconds, i), fs)
        assert n_eff_of(w.wave, fs) == (n if k == 'loud' else 0)
        got, want = on.push(w, discard=(1, 1), advance=advance), off.push(w, discard=(1, 1), advance=advance)
        assert P.same(got.wave, want.wave), i
        assert on.last_gate['tracked'] == [k == 'loud']
    assert 0 < on.last_gate['n_computed'][0] < n, (on.last_gate, n)
    assert on._pending == 0
    assert P.same(on.flush().wave, off.flush().wave)
    on.close()
    off.close()


# ---- 2, 3: a bank ----------------------------------------------------------------------------------------------------------------------------
SEEDS = [3, 4, 5]


def bank_rounds(fs, seconds, advance):
    """B = 3.  Stream 0 is always audible, stream 1 always silent (zeros, then noise), stream 2 alternates -- audible, silent, out (None), silent,
    audible -- and is named in `final` once (round 5: its signal ends there and starts anew).  Round 6: every wave is silent.  Round 7: the only
    audible wave is the barely audible one.  Streams 0 and 2 cut their audible windows from long signals, `advance` apart per round."""
    from yukarin import Wave
    s0, s2 = overlapping(fs, seconds, advance, 8, 1), overlapping(fs, seconds, advance, 8, 2)
    z = lambda kind, seed: W(kind, fs, seconds, seed)
    loud = lambda xs, i: Wave(xs[i], fs)
    return [([loud(s0, 0), z('zeros', 1), loud(s2, 0)], ()),
            ([loud(s0, 1), z('noise', 2), z('zeros', 3)], ()),
            ([loud(s0, 2), z('zeros', 4), None], ()),
            ([loud(s0, 3), z('noise', 5), z('noise', 6)], ()),
            ([loud(s0, 4), z('zeros', 7), loud(s2, 4)], (2,)),
            ([z('zeros', 8), z('noise', 9), z('zeros', 10)], ()),
            ([z('noise', 11), z('barely', 12), z('zeros', 13)], ())]


def stream2_advances(advance):
    """The advance of stream 2's buffers against its previous buffer: it sat round 3 out, so its buffer of round 4 lies two rounds behind."""
    return [advance, advance, None, 2 * advance, advance, advance, advance]


def check_bank(vc, capacity, fs, seconds, advance, discard, frames_through_network, out_gate_of=None, with_lone=True):
    """`convert_waves` and the rounds of `bank_rounds`, flag on against a flag-off bank and against lone flag-off pipelines per stream; the
    counters and `last_gate` show what was skipped (test 3)."""
    param = vc.acoustic_converter.config.dataset.acoustic_param
    on = pipeline.PipelineBank(vc, param, 3, seeds=SEEDS, crepe_capacity=capacity, gate_first=True)
    off = pipeline.PipelineBank(vc, param, 3, seeds=SEEDS, crepe_capacity=capacity)
    lone = [pipeline.Pipeline(vc, param, crepe_capacity=capacity, seed=s) for s in SEEDS]
    first = [W('loud', fs, seconds, 1), W('zeros', fs, seconds), W('barely', fs, seconds), W('noise', fs, seconds, 2)]
    before = pipeline.calls_many.get('gated', 0)
    got = on.convert_waves(first)
    assert on.last_gate['tracked'] == [True, False, True, False] and on.last_gate['n_eff'][1:] == [0, 1, 0]
    assert pipeline.calls_many['gated'] - before == 2
    for g, w, o in zip(got, off.convert_waves(first), first):
        assert P.same(g.wave, w.wave) and (not with_lone or P.same(g.wave, lone[0].convert_wave(o).wave))
    gates = [None, None] if out_gate_of is None else [out_gate_of(), out_gate_of()]
    rounds = bank_rounds(fs, seconds, advance if advance is not None else 1)
    adv2 = stream2_advances(advance) if advance is not None else None
    computed = []
    for r, (waves, final) in enumerate(rounds):
        extra = {} if advance is None else dict(advance=[advance, advance, adv2[r]])
        before, frames_before = pipeline.calls_many.get('gated', 0), frames_through_network()
        got = on.push(waves, discard=discard, final=final, out_gate=gates[0], **extra)
        ran = frames_through_network() - frames_before
        silent = [s for s, w in enumerate(waves) if w is not None and n_eff_of(w.wave, fs) == 0]
        part = [s for s, w in enumerate(waves) if w is not None]
        assert pipeline.calls_many['gated'] - before == len(silent), (r, silent)
        assert on.last_gate['streams'] == part and [part[i] for i, t in enumerate(on.last_gate['tracked']) if not t] == silent, (r, on.last_gate)
        if len(silent) == len(part):
            assert ran == 0, (r, ran)                                      # an all-silent call: not one frame through the network
        else:
            assert ran > 0
        computed.append(dict(zip(part, on.last_gate['n_computed'])))
        want = off.push(waves, discard=discard, final=final, out_gate=gates[1], **extra)
        for s, w in enumerate(waves):
            assert P.same(got[s].wave, want[s].wave), (r, s)
            if w is None or out_gate_of is not None or not with_lone:
                continue
            alone = lone[s].push(w, discard=discard, final=s in final)
            assert P.same(got[s].wave, alone.wave), (r, s, 'lone')
    assert n_eff_of(rounds[6][0][1].wave, fs) == 1 and on.last_gate['n_eff'] == [0, 1, 0]
    for g, w in zip(on.flush(), off.flush()):
        assert P.same(g.wave, w.wave)
    if advance is not None:
        n = crepe.track_frames(rounds[0][0][0].wave.size, fs, crepe.hop_length(P.FRAME_PERIOD))
        assert all(c[1] is None for c in computed[:6])                     # stream 1 never tracked while it was silent
        assert computed[0][2] == n and computed[1][2] is None and computed[3][2] is None
        # stream 2's first audible buffer after skipped ones: rounds 2 and 4 were skipped, round 3 sat out -- the advance accumulated to 4 rounds,
        # its rows were kept, and fewer frames than the window has went through the network
        assert 0 < computed[4][2] < n, computed[4]
        assert 0 < computed[1][0] < n                                      # stream 0, plain overlap
    on.close()
    off.close()
    for p in lone:
        p.close()


# ---- 4: nothing of a skipped wave is read ---------------------------------------------------------------------------------------------------
def nan_fill(ctx, blocks, cap):
    for k in ('mc32', 'sp32', 'ap32'):
        ctx.dev_upload(blocks[k], numpy.full(cap * blocks['w_' + k], 0xFFFFFFFF, numpy.uint32))


def check_poisoned(vc, capacity, fs, seconds, model):
    """The bank's feature blocks filled with NaN patterns and the tracker poisoned before a call with two skipped streams: their samples equal
    the flag-off run's and no NaN reaches any output."""
    param = vc.acoustic_converter.config.dataset.acoustic_param
    on = pipeline.PipelineBank(vc, param, 3, seeds=SEEDS, crepe_capacity=capacity, gate_first=True)
    off = pipeline.PipelineBank(vc, param, 3, seeds=SEEDS, crepe_capacity=capacity)
    rounds = [[W('loud', fs, seconds, 1), W('zeros', fs, seconds), W('noise', fs, seconds, 3)],
              [W('loud', fs, seconds, 4), W('noise', fs, seconds, 5), W('zeros', fs, seconds)],
              [W('zeros', fs, seconds), W('noise', fs, seconds, 6), W('zeros', fs, seconds)]]
    for r, waves in enumerate(rounds):
        if on._blocks:
            nan_fill(on._ctx, on._blocks, on._cap)
        model.poison()
        got = on.push(waves, discard=(1, 1), final=(0, 1, 2) if r == 2 else ())
        want = off.push(waves, discard=(1, 1), final=(0, 1, 2) if r == 2 else ())
        assert on.last_gate['tracked'] == [r < 2, False, False]
        for s in range(3):
            assert not numpy.isnan(got[s].wave).any() and P.same(got[s].wave, want[s].wave), (r, s)
    assert sum(len(g.wave) for g in got) > 0
    on.close()
    off.close()


# ---- 5: the compaction kernel alone -----------------------------------------------------------------------------------------------------------
MASK_FRAMES = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 2049)           # the last two: a second and a third round of 1024 frames in the kernel
MASK_KINDS = ('zeros', 'ones', 'first', 'last', 'alt')


def mask_of(kind, n):
    m = numpy.zeros(n, numpy.uint8)
    if kind == 'ones':
        m[:] = 1
    elif kind == 'first':
        m[0] = 1
    elif kind == 'last':
        m[-1] = 1
    elif kind == 'alt':
        m[::2] = 1
    return m


def check_compaction(ctx, core):
    """`ry_vc_compact_waves_device` on three waves per call (an empty one in the middle) for every mask length and kind: x_eff and row_of equal
    what the gate's own compaction is defined to write -- the rows of the effective frames in ascending order, their indices from the wave's first
    frame -- and everything else keeps its guard word; the empty wave lies over NaN feature rows."""
    rng = numpy.random.default_rng(29)
    cin = core.stage1.desc.in_ch
    for n in MASK_FRAMES:
        for kind in MASK_KINDS:
            masks = [mask_of(kind, n), numpy.zeros(max(n // 2, 1), numpy.uint8), mask_of('alt' if kind != 'alt' else 'ones', n + 3)]
            feats = [rng.normal(size=(len(m), cin)).astype(numpy.float32) for m in masks]
            feats[1][:] = numpy.nan                                         # no row of the empty wave may be read
            fo = numpy.concatenate([[0], numpy.cumsum([len(m) for m in masks])]).astype(numpy.int32)
            total, g = int(fo[-1]), 8
            B = M.Blocks(ctx)
            mask_block, feat_block = B.of(numpy.concatenate(masks)), B.of(numpy.concatenate(feats))
            x_block, row_block = B.filled(total * cin + 2 * g), B.filled(total + 2 * g)
            core.compact_waves_device(fo, mask_block, numpy.concatenate(masks), [int(m.sum()) for m in masks], feat_block, x_block + 4 * g,
                                      row_block + 4 * g)
            ctx.sync()
            x_got, row_got = B.read(x_block, total * cin + 2 * g), B.read(row_block, total + 2 * g)
            for words in (x_got, row_got):
                assert (words[:g] == M.GUARD).all() and (words[-g:] == M.GUARD).all()
            x_got, row_got = x_got[g:-g].reshape(total, cin), row_got[g:-g]
            for i, (m, f) in enumerate(zip(masks, feats)):
                a, b, rows = int(fo[i]), int(fo[i + 1]), numpy.flatnonzero(m)
                k = len(rows)
                assert numpy.array_equal(x_got[a:a + k], P.bits(f[rows])) and numpy.array_equal(row_got[a:a + k].view(numpy.int32), rows), (n, kind, i)
                assert (x_got[a + k:b] == M.GUARD).all() and (row_got[a + k:b] == M.GUARD).all(), (n, kind, i)
            B.close()


def check_compaction_equals_the_gate(ctx, core, fs):
    """The same waves through `ry_vc_gate_waves_device` (gate and compaction in one) and through the verdict call followed by the compaction
    alone: mask, counts, x_eff and row_of agree word for word; the middle wave is silent and lies over NaN feature rows in the second run."""
    hop = fs * P.FRAME_PERIOD // 1000
    waves = [P.wave_of('gap', fs, 0.25, 1), wave_of('noise', fs, 0.1, 2), P.wave_of('gap_silent_ends', fs, 0.25, 3), wave_of('barely', fs, 0.15)]
    frames = [x.size // hop + 1 for x in waves]
    thr = gate.thresholds(P.THRESHOLD)
    cin = core.stage1.desc.in_ch
    rng = numpy.random.default_rng(31)
    feats = [rng.normal(size=(n, cin)).astype(numpy.float32) for n in frames]
    so = numpy.concatenate([[0], numpy.cumsum([x.size for x in waves])]).astype(numpy.int64)
    fo = numpy.concatenate([[0], numpy.cumsum(frames)]).astype(numpy.int32)
    n = int(fo[-1])
    B = M.Blocks(ctx)
    wave_block, feat_block = B.of(numpy.concatenate(waves)), B.of(numpy.concatenate(feats))
    outs = [[B.filled((n + 3) // 4), B.filled(n * cin), B.filled(n)] for _ in range(2)]
    eff, n_eff = core.gate_waves_device(wave_block, so, fo, hop, 1024, thr[0], thr[1], feat_block, *outs[0])
    assert n_eff[1] == 0 and n_eff[3] == 1 and 0 < n_eff[0] < frames[0]
    poisoned = [f.copy() for f in feats]
    poisoned[1][:] = numpy.nan
    feat_block2 = B.of(numpy.concatenate(poisoned))
    eff2, n_eff2 = core.gate_verdict_waves_device(wave_block, so, fo, hop, 1024, thr[0], thr[1], outs[1][0])
    assert numpy.array_equal(eff, eff2) and numpy.array_equal(n_eff, n_eff2)
    core.compact_waves_device(fo, outs[1][0], eff2, n_eff2, feat_block2, outs[1][1], outs[1][2])
    ctx.sync()
    for p, q, words in zip(outs[0], outs[1], ((n + 3) // 4, n * cin, n)):
        assert numpy.array_equal(B.read(p, words), B.read(q, words))
    B.close()


def check_masked_windows(ctx, core, windows):
    """`ry_vc_enqueue_waves_masked_device` on the verdict of the gate against `ry_vc_enqueue_wave_device` per wave (`pipeline_many_cases.Windows`),
    the feature rows of the waves without an effective frame replaced by NaN."""
    for discard in ((0, 0), (1, 1)):
        want = windows.single(discard)
        so = numpy.concatenate([[0], numpy.cumsum([x.size for x in windows.waves])]).astype(numpy.int64)
        fo = numpy.concatenate([[0], numpy.cumsum(windows.frames)]).astype(numpy.int32)
        n, g = int(fo[-1]), 8
        B = M.Blocks(ctx)
        feats = [f if w[3] > 0 else numpy.full_like(f, numpy.nan) for f, w in zip(windows.feats, want)]
        wave_block, feat_block = B.of(numpy.concatenate(windows.waves)), B.of(numpy.concatenate(feats))
        mc_block, sp_block, mask_block = B.filled(n * core.M + 2 * g), B.filled(n * core.F + 2 * g), B.filled((n + 3) // 4)
        eff, n_eff = core.gate_verdict_waves_device(wave_block, so, fo, windows.hop, windows.fft, windows.thr[0], windows.thr[1], mask_block)
        core.set_discard(*discard)
        core.enqueue_waves_masked_device(fo, feat_block, mc_block + 4 * g, sp_block + 4 * g, mask_block, eff, n_eff)
        ctx.sync()
        mc, sp = B.read(mc_block, n * core.M + 2 * g), B.read(sp_block, n * core.F + 2 * g)
        for words in (mc, sp):
            assert (words[:g] == M.GUARD).all() and (words[-g:] == M.GUARD).all()
        mc, sp = mc[g:-g].reshape(n, core.M), sp[g:-g].reshape(n, core.F)
        for i, (w_mc, w_sp, w_eff, w_n) in enumerate(want):
            a, b = int(fo[i]), int(fo[i + 1])
            assert n_eff[i] == w_n and numpy.array_equal(eff[a:b], w_eff), (i, discard)
            assert numpy.array_equal(mc[a:b].ravel(), w_mc) and numpy.array_equal(sp[a:b].ravel(), w_sp), (i, discard)
        B.close()
        core.set_discard(0, 0)


# ---- 6, 7: the split tracker entries and the frame-count rule -----------------------------------------------------------------------------------
def check_split_tracker(model, fs):
    """Waves {0, 2} of an uploaded table of three against `track_many` on those two alone; the upload and the track of the rest stay usable."""
    hop = crepe.hop_length(P.FRAME_PERIOD)
    xs = [P.wave_of('loud', fs, s, seed) for seed, s in enumerate((0.03, 0.02, 0.04))]
    want = model.track_many([xs[0], xs[2]], fs, hop, P.FRAME_PERIOD, device=False)
    model.poison()
    before = model.frames_through_network()
    up = model.upload_waves(xs, fs)
    assert model.frames_through_network() == before                         # the upload alone runs nothing
    trk = model.track_uploaded(up, [0, 2], hop, P.FRAME_PERIOD)
    assert list(trk.first_sample) == [0, xs[0].size + xs[1].size]
    got = trk.download()
    assert model.frames_through_network() - before == sum(len(w[0]) for w in want)
    for (v, f), (wv, wf, _) in zip(got, want):
        assert numpy.array_equal(v, wv) and P.same(f, wf)
    one = model.track_uploaded(up, [1], hop, P.FRAME_PERIOD).download()      # a second subset of the same table
    alone = model.track_many([xs[1]], fs, hop, P.FRAME_PERIOD, device=False)
    assert numpy.array_equal(one[0][0], alone[0][0]) and P.same(one[0][1], alone[0][1])


def check_frame_rule(model, one_second=True):
    """`crepe.track_frames` against the tracker's own n_frames: 1 sample, one sample either side of a hop at 16 and 24 kHz, 1 s."""
    hop = crepe.hop_length(P.FRAME_PERIOD)
    for fs in (16000, 24000):
        h = fs * P.FRAME_PERIOD // 1000
        for n in (1, 2, h - 1, h, h + 1, 3 * h - 1, 3 * h, 3 * h + 1) + ((fs,) if one_second else ()):
            if fs != 16000 and n < 2:
                continue                                                     # no sample at 16 kHz: the tracker refuses the wave
            x = numpy.zeros(n, numpy.float32)
            assert len(model.track(x, fs, hop, P.FRAME_PERIOD)[0]) == crepe.track_frames(n, fs, hop), (fs, n)
    assert crepe.track_frames(1, 16000, hop) == 1 and crepe.track_frames(16000, 16000, hop) == 201


# ---- 9: refusals ----------------------------------------------------------------------------------------------------------------------------------
def check_refusals(ctx, core, model):
    """The new C entries by return code: null pointers, a mask count that disagrees with n_eff, tables that do not ascend, a subset entry outside
    the uploaded table; guard-filled outputs stay as they were."""
    dll = ctx.lib.dll
    cin = core.stage1.desc.in_ch
    f, ub, ip = _lib._fptr, lambda a: ctypes.cast(ctypes.c_void_p(a), UB), lambda a: ctypes.cast(ctypes.c_void_p(a), IP)
    B = M.Blocks(ctx)
    mask = numpy.array([1, 0, 1, 0, 0, 1, 1, 1, 0, 0], numpy.uint8)
    mask_block, feat_block = B.of(mask), B.of(numpy.ones((10, cin), numpy.float32))
    outs = [B.filled(10 * cin), B.filled(10), B.filled(10 * core.M), B.filled(10 * core.F)]
    fo, ne = numpy.array([0, 5, 10], numpy.int32), numpy.array([2, 3], numpy.int32)

    def compact(fo=fo, ne=ne, n_waves=2, **null):
        a = dict(vc=core.handle, mask=ub(mask_block), host=mask.ctypes.data_as(UB), feat=f(feat_block), x=f(outs[0]), rows=ip(outs[1]))
        a.update(null)
        return dll.ry_vc_compact_waves_device(a['vc'], fo.ctypes.data_as(IP) if fo is not None else None, n_waves, a['mask'], a['host'],
                                              ne.ctypes.data_as(IP) if ne is not None else None, a['feat'], a['x'], a['rows'])

    def masked(fo=fo, ne=ne, n_waves=2, **null):
        a = dict(vc=core.handle, mask=ub(mask_block), host=mask.ctypes.data_as(UB), feat=f(feat_block), mc=f(outs[2]), sp=f(outs[3]))
        a.update(null)
        return dll.ry_vc_enqueue_waves_masked_device(a['vc'], fo.ctypes.data_as(IP) if fo is not None else None, n_waves, a['feat'], 1e-16, a['mc'], a['sp'],
                                                     a['mask'], a['host'], ne.ctypes.data_as(IP) if ne is not None else None)
    for call in (compact, masked):
        for key, bad in (('vc', None), ('mask', ub(0)), ('host', None), ('feat', f(None))):
            assert call(**{key: bad}) == -1, key
        assert call(fo=None) == -1 and call(ne=None) == -1 and call(n_waves=0) == -1 and call(n_waves=65537) == -1
        assert call(ne=numpy.array([2, 2], numpy.int32)) == -1 and b'wave 1' in dll.ry_last_error()       # the mask holds three
        assert call(ne=numpy.array([6, 3], numpy.int32)) == -1 and call(ne=numpy.array([-1, 3], numpy.int32)) == -1
        assert call(fo=numpy.array([1, 5, 10], numpy.int32)) == -1 and call(fo=numpy.array([0, 5, 5], numpy.int32)) == -1
        assert call(fo=numpy.array([0, 6, 4], numpy.int32)) == -1
    assert compact(x=f(None)) == -1 and compact(rows=ip(0)) == -1 and masked(mc=f(None)) == -1 and masked(sp=f(None)) == -1
    so = numpy.array([0, 320, 640], numpy.int64)
    wave_block = B.of(numpy.zeros(640, numpy.float32))
    host, counts = numpy.zeros(10, numpy.uint8), numpy.zeros(2, numpy.int32)

    def verdict(so=so, fo=fo, n_waves=2, hop=80, fft=1024, **null):
        a = dict(vc=core.handle, wave=f(wave_block), mask=ub(outs[1]), host=host.ctypes.data_as(UB), count=counts.ctypes.data_as(IP))
        a.update(null)
        return dll.ry_vc_gate_verdict_waves_device(a['vc'], a['wave'], so.ctypes.data_as(LLP) if so is not None else None,
                                                   fo.ctypes.data_as(IP) if fo is not None else None, n_waves, hop, fft, 1e-6, 3e38, a['mask'], a['host'],
                                                   a['count'])
    for key, bad in (('vc', None), ('wave', f(None)), ('mask', ub(0)), ('host', None), ('count', None)):
        assert verdict(**{key: bad}) == -1, key
    assert verdict(so=None) == -1 and verdict(fo=None) == -1 and verdict(n_waves=0) == -1 and verdict(hop=0) == -1 and verdict(fft=100) == -1
    assert verdict(so=numpy.array([0, 640, 320], numpy.int64)) == -1 and verdict(fo=numpy.array([0, 5, 5], numpy.int32)) == -1
    ctx.sync()
    for p, words in zip(outs, (10 * cin, 10, 10 * core.M, 10 * core.F)):
        assert (B.read(p, words) == M.GUARD).all()
    assert compact() == 0 and masked() == 0
    ctx.sync()
    B.close()
    # the tracker: the upload, a subset outside the table, tables that do not ascend, no table at all
    lib, h = model._get()
    hop = crepe.hop_length(P.FRAME_PERIOD)
    xs = numpy.zeros(960, numpy.float32)
    n3, nf = numpy.array([320, 160, 480], numpy.int32), numpy.zeros(3, numpy.int32)
    p = ctypes.c_void_p()
    before = model.frames_through_network()
    up = lambda audio=f(xs), counts=n3, n=3, sr=16000, out=ctypes.byref(p): lib.dll.ry_crepe_upload_waves(h, audio, counts.ctypes.data_as(IP), n, sr, out)
    assert lib.dll.ry_crepe_upload_waves(None, f(xs), n3.ctypes.data_as(IP), 3, 16000, ctypes.byref(p)) == -4
    assert up(audio=f(None)) == -1 and up(out=None) == -1 and up(n=0) == -1 and up(counts=numpy.array([320, 0, 480], numpy.int32)) == -1
    assert lib.dll.ry_crepe_upload_waves(h, f(xs), None, 3, 16000, ctypes.byref(p)) == -1

    def track(first, counts, n=2, sr=16000, hop=hop):
        first, counts = numpy.asarray(first, numpy.int32), numpy.asarray(counts, numpy.int32)
        return lib.dll.ry_crepe_track_uploaded(h, first.ctypes.data_as(IP), counts.ctypes.data_as(IP), n, sr, hop, 5.0, 0.1, nf.ctypes.data_as(IP),
                                               None, None, None, 1)
    assert track([0, 480], [320, 480]) == -4                                  # no table: the refused uploads left none
    assert up() == 0 and p.value
    assert track([0, 480], [320, 480], sr=24000) in (-1, -4)                 # another rate than the upload's
    assert track([0, 480], [320, 470]) == -1 and track([0, 481], [320, 479]) == -1 and track([0, 960], [320, 1]) == -1   # not waves of the table
    assert track([480, 0], [480, 320]) == -1 and track([0, 0], [320, 320]) == -1                                         # do not ascend
    assert track([0, 480], [320, 480], n=0) == -1 and track([0, 480], [320, 480], hop=0) == -1
    assert lib.dll.ry_crepe_track_uploaded(h, None, n3.ctypes.data_as(IP), 2, 16000, hop, 5.0, 0.1, nf.ctypes.data_as(IP), None, None, None, 1) == -1
    assert model.frames_through_network() == before                         # nothing was launched
    assert lib.dll.ry_crepe_uploaded_buffers(h, None, None, None, None, None, None, None) == -4    # the refused calls forgot the table
    assert up() == 0 and track([0, 480], [320, 480]) == 0 and nf.tolist()[:2] == [5, 7]
    nt = ctypes.c_int()
    assert lib.dll.ry_crepe_uploaded_buffers(h, None, None, ctypes.byref(nt), None, None, None, None) == 0 and nt.value == 2
    ctx.sync()
