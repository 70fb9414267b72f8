"""The frame powers of the device silence gate, pinned to the host's bits without reading them back (test_gate_power_cpu.py on the emulator,
test_gate_power_gpu.py on the card).  The gate entries take both thresholds from the caller as float32 values, so for any value v the mask at
p_eff = v and the mask at p_eff = nextafter(v, +inf), the clamp threshold out of reach, say for every frame whether power >= v and whether power > v:
sweeping v over the host's own powers fixes every frame's power to its bits.  The same through p_all for the maximum the `top_db` clamp sees.

The contract is `compat.yukarin.wave.frame_power` in numpy float32 (`host_powers`); it is itself held to the float64 mean of squares
(`check_reference_against_float64`) and to a float32 restatement of the order the kernel's header states (`restated`), whose four wrong variants the
case set must tell apart (`orders_told_apart`).

`p_eff = 0` is accepted by every gate entry and is run like any other value (no skip).  On an `overflow` wave every power is +inf: +inf has no upper
neighbour and lies above any p_all, so the clamp cannot be switched off there -- the sweep pins such a wave's powers through `p_eff = p_all = +inf`
(every frame effective only if the maximum IS +inf) and frame by frame on the one-frame waves (lengths 1, 2, 37 at hops above them).

What the sweep found when it first ran on the card: products fused into the sums (v_fmac) and a native 1-ulp square root -- the HIP headers'
__fmul_rn / __fadd_rn / __fsqrt_rn are plain `*`, `+` and the native sqrt unless OCML_BASIC_ROUNDED_OPERATIONS is defined -- and, on the host
side, that numpy adds the squares in one running sum at hop 1; csrc/ry_dev.h and ry_frame_power_of were mended, subnormal and infinite powers
were equal from the start."""
import numpy

import pipeline_many_cases as M
import test_device_gate as G
from oracle import effective_frame as oef
from realtime_yukarin_amd import gate, synth
from realtime_yukarin_amd.compat.yukarin import wave as host_wave

FS, FP, HOP = 16000, 5, 80             # the production hop: what `Wave.get_effective_frame` and the oracle derive from (FS, FP)
OFF = 3e38                              # a threshold no finite power of the cases reaches (the existing gate tests switch the clamp off with it)
U = 2.0 ** -24                          # one float32 rounding, relative
FFTS = (128, 256, 512, 1024)            # 1, 2, 4, 8 leaves of 128: 0 .. 3 levels of the tree over the leaves; 8, 16, 32, 64 active lanes
HOPS = (80, 120, 53)
KINDS = ('normal', 'wide', 'ramp', 'subnormal', 'straddle', 'overflow', 'constant', 'impulse')
CONSTANT = 0.25                         # its square and every partial sum of it are exact: the power of every frame is 0.0625
TINY = float(numpy.finfo(numpy.float32).tiny)
CIN = 9


def make_core(ctx):
    return G.make_core(ctx, 'SYN-8')


def close_core(made):
    core, n1, n2 = made
    core.close(); n1.close(); n2.close()


def wave_of(kind: str, n: int, seed: int = 0) -> numpy.ndarray:
    rng = numpy.random.default_rng([seed, n, KINDS.index(kind)])
    z = rng.normal(size=n)
    sign = numpy.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    if kind == 'normal':
        x = 0.1 * z
    elif kind == 'wide':                # magnitudes log-uniform over 2^-20 .. 1: nearly every addition rounds, the order of the sum is visible
        x = numpy.exp2(rng.uniform(-20.0, 0.0, n)) * sign
    elif kind == 'ramp':
        x = numpy.geomspace(1e-6, 0.5, n) * z
    elif kind == 'subnormal':           # squares near 1e-38: every power is subnormal or just above
        x = 1e-19 * z
    elif kind == 'straddle':            # squares 9e-38 .. 9e-36 around FLT_MIN: squares and sums cross the normal / subnormal line inside a frame
        x = numpy.exp(rng.uniform(numpy.log(3e-19), numpy.log(3e-18), n)) * sign
    elif kind == 'overflow':            # squares near 9e36: the sum of a frame overflows, the power is +inf
        x = 3e18 * z
    elif kind == 'constant':
        x = numpy.full(n, CONSTANT)
    elif kind == 'impulse':
        x = numpy.zeros(n); x[-1] = 0.5
    else:
        raise ValueError(kind)
    return x.astype(numpy.float32)


def lengths(fft: int):
    return (1, 2, 37, fft // 2 - 1, fft // 2, fft // 2 + 1, 700, 1234)


def sweep_cases(fft: int):
    """(kind, samples, hop): every length with every kind, the hop rotating so that each length and each kind meets all three, and one
    wave at hop 1; at most 31 wave frames."""
    out = []
    for i, n in enumerate(lengths(fft)):
        for j, kind in enumerate(KINDS):
            out.append((kind, n, HOPS[(i + j) % 3]))
    out.append(('wide', 30, 1))                                  # hop 1: the host adds the squares in one running sum there, and so does the kernel
    return out


def emulator_cases(fft: int):
    """The part of `sweep_cases` the emulator runs (a 1024-fiber workgroup per gate call there)."""
    keep = [c for c in sweep_cases(fft) if c[2] == 1 or (c[0] in ('wide', 'subnormal', 'overflow') and c[1] in (37, fft // 2, 700))]
    assert len(keep) == 10
    return keep


LONG_CASE = ('wide', 4 * 256 + 2, 1, 128)       # 4 * 256 + 3 wave frames: the four-frames-per-workgroup grid of ry_frame_power ends ragged


# ---- the reference and its restatements -----------------------------------------------------------------------------------------------------
def host_powers(wave: numpy.ndarray, fft: int, hop: int) -> numpy.ndarray:
    assert wave.dtype == numpy.float32
    with numpy.errstate(all='ignore'):
        p = host_wave.frame_power(wave, fft, hop)
    assert p.dtype == numpy.float32 and p.shape == (len(wave) // hop + 1,)
    return p


def frames_of(wave: numpy.ndarray, fft: int, hop: int) -> numpy.ndarray:
    """(T, fft) float32: the reflect-padded frames by index arithmetic (no numpy.pad, no strided view)."""
    n, t = len(wave), len(wave) // hop + 1
    idx = numpy.arange(t)[:, None] * hop + numpy.arange(fft)[None, :] - fft // 2
    if n == 1:
        return numpy.broadcast_to(wave, (t, fft)).copy()
    period = 2 * (n - 1)
    j = idx % period
    return wave[numpy.where(j < n, j, period - j)]


def float64_powers(wave, fft, hop):
    with numpy.errstate(all='ignore'):
        return (frames_of(wave, fft, hop).astype(numpy.float64) ** 2).mean(axis=1)


def restated(wave, fft, hop, variant='faithful'):
    """The order ry_frame_power states, in numpy float32, every product and every sum rounded on its own: leaves of 128 elements, eight interleaved
    accumulators per leaf walking their 16 elements in order, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) inside a leaf, a binary tree over the
    leaves, an exact division by the frame length, sqrt, square.  The variants are the regressions the sweep has to catch:
    'sequential' one running sum over the frame; 'leaves_in_sequence' correct leaves added one after the other; 'fma' products contracted into
    the sum, r = fl(v * v + r) through float64 (v * v is exact there); 'no_sqrt' the sqrt-and-square round trip left out.
    At hop 1 the faithful order is the running sum: the two axes of the host's frame view then have equal strides, numpy lays the squares out
    row-major and adds the rows one after the other (found by this restatement; the kernel follows the host there too)."""
    f32 = numpy.float32
    with numpy.errstate(all='ignore'):
        x = frames_of(wave, fft, hop)
        t, leaves = x.shape[0], fft // 128
        if variant == 'sequential' or (variant == 'faithful' and hop == 1):
            sq = x * x
            total = sq[:, 0].copy()
            for k in range(1, fft):
                total = total + sq[:, k]
        else:
            v = x.reshape(t, leaves, 16, 8)
            if variant == 'fma':
                r = v[:, :, 0, :] * v[:, :, 0, :]
                for i in range(1, 16):
                    w = v[:, :, i, :].astype(numpy.float64)
                    r = (w * w + r.astype(numpy.float64)).astype(f32)
            else:
                sq = v * v
                r = sq[:, :, 0, :]
                for i in range(1, 16):
                    r = r + sq[:, :, i, :]
            leaf = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
            if variant == 'leaves_in_sequence':
                total = leaf[:, 0]
                for k in range(1, leaves):
                    total = total + leaf[:, k]
            else:
                while leaf.shape[1] > 1:
                    leaf = leaf[:, 0::2] + leaf[:, 1::2]
                total = leaf[:, 0]
        assert total.dtype == f32
        mean = total / f32(fft)
        if variant == 'no_sqrt':
            return mean
        rms = numpy.sqrt(mean)
        return rms * rms


def same_bits(a, b) -> bool:
    return a.dtype == b.dtype == numpy.float32 and numpy.array_equal(a.view(numpy.uint32), b.view(numpy.uint32))


def all_cases():
    """(wave, fft, hop) of every single-wave case of the GPU file."""
    for fft in FFTS:
        for kind, n, hop in sweep_cases(fft):
            yield kind, wave_of(kind, n), fft, hop
    kind, n, hop, fft = LONG_CASE
    yield kind, wave_of(kind, n), fft, hop


def orders_told_apart():
    """{variant: {fft: frames that differ from the host}} over all cases; the faithful restatement must equal the host on every case."""
    differ = {v: {fft: 0 for fft in FFTS} for v in ('sequential', 'leaves_in_sequence', 'fma', 'no_sqrt')}
    for kind, wave, fft, hop in all_cases():
        p = host_powers(wave, fft, hop)
        assert same_bits(restated(wave, fft, hop), p), (kind, len(wave), fft, hop)
        for variant in differ if hop > 1 else ():               # the hop-1 wave has its own order: it is not counted
            q = restated(wave, fft, hop, variant)
            differ[variant][fft] += int((q.view(numpy.uint32) != p.view(numpy.uint32)).sum())
    return differ


def check_reference_against_float64():
    """|P - P64| <= 24 * 2^-24 * P64 where every square is normal (or an exact zero) and finite: one rounding per product, at most 15 + 6 additions on
    the path of any element at fft 1024, an exact scaling, one sqrt, one square.  Returns (cases held, the largest error seen in units of 2^-24)."""
    held, worst = 0, 0.0
    for kind, wave, fft, hop in all_cases():
        if kind in ('subnormal', 'straddle', 'overflow') or hop == 1:      # outside the normal range; the running sum at hop 1 has fft - 1 additions
            continue
        sq = wave.astype(numpy.float64) ** 2
        assert ((sq == 0) | ((sq >= TINY) & (sq < 1e30))).all(), kind
        p, p64 = host_powers(wave, fft, hop).astype(numpy.float64), float64_powers(wave, fft, hop)
        err = numpy.abs(p - p64)
        assert (err <= 24 * U * p64).all(), (kind, len(wave), fft, hop, float((err / numpy.maximum(p64, TINY)).max() / U))
        if kind == 'constant':
            assert (p == CONSTANT ** 2).all()
        nz = p64 > 0
        if nz.any():
            worst = max(worst, float((err[nz] / p64[nz]).max() / U))
        held += 1
    return held, worst


# ---- the sweep over one wave -----------------------------------------------------------------------------------------------------------------
def next_up(v):
    return numpy.nextafter(numpy.float32(v), numpy.float32(numpy.inf))


def sweep_values(powers):
    """Every distinct power with its upper neighbour; +inf alone."""
    out = []
    for v in numpy.unique(powers):
        out.append(numpy.float32(v))
        if numpy.isfinite(v):
            out.append(next_up(v))
    return out


def check_powers(core, wave, fft, hop, rng, what=None):
    """Pins every wave frame's power, and the maximum the clamp takes, to `host_powers`; returns the number of gate calls."""
    P = host_powers(wave, fft, hop)
    T = len(wave) // hop + 1
    top = P.max()
    assert not numpy.isnan(P).any() and (top < OFF or numpy.isinf(P).all()), what      # a condition on the inputs: OFF switches the clamp off
    calls = 0
    for n_frames in (T, T - 1):
        if n_frames < 1:
            continue
        feat = (rng.normal(size=(n_frames, CIN)) * synth.MC_SCALE).astype(numpy.float32)

        def run(p_eff, p_all, want):
            eff, x_eff, rows = core.gate(wave, hop, fft, float(p_eff), float(p_all), feat)
            tag = (what, len(wave), fft, hop, n_frames, float(p_eff), float(p_all))
            assert numpy.array_equal(eff, want), (tag, numpy.flatnonzero(eff != want)[:8], P[:n_frames][eff != want][:8])
            assert numpy.array_equal(rows, numpy.flatnonzero(want)) and numpy.array_equal(x_eff, feat[want]), tag
            return 1

        for v in sweep_values(P):
            calls += run(v, OFF, P[:n_frames] >= v)
        if numpy.isinf(top):                                                 # +inf passes any threshold: pinned by being the only value that passes +inf
            calls += run(numpy.inf, numpy.inf, numpy.ones(n_frames, bool))
        else:                                                                # no frame passes on its own; the clamp decides from ALL T frames
            calls += run(OFF, top, numpy.ones(n_frames, bool))
            calls += run(OFF, next_up(top), numpy.zeros(n_frames, bool))
    return calls


def last_frame_case():
    """fft 128, hop 80, an impulse on the last of 1234 samples: the loudest wave frame is the last one alone, the one past a feature block of T - 1 rows."""
    wave, fft, hop = wave_of('impulse', 1234), 128, 80
    P = host_powers(wave, fft, hop)
    assert P.argmax() == len(P) - 1 == 1234 // hop and (P[:-1] < P[-1]).all()
    return wave, fft, hop


def check_sweep(ctx, cases, fft):
    made = make_core(ctx)
    rng = numpy.random.default_rng(41)
    calls = 0
    for kind, n, hop in cases:
        calls += check_powers(made[0], wave_of(kind, n), fft, hop, rng, kind)
    if fft == 128:
        wave, f, hop = last_frame_case()
        calls += check_powers(made[0], wave, f, hop, rng, 'impulse on the last frame')
    close_core(made)
    return calls


def check_long(ctx):
    kind, n, hop, fft = LONG_CASE
    made = make_core(ctx)
    calls = check_powers(made[0], wave_of(kind, n), fft, hop, numpy.random.default_rng(42), 'long')
    close_core(made)
    return calls


# ---- the sweep over a table of waves -----------------------------------------------------------------------------------------------------------
def table_waves(fft):
    """Five waves back to back in one block, neighbours of very different magnitude: a frame that reflected at the block's ends, or at a neighbour's,
    would read samples 10^18 times too large or too small."""
    return [(5.0 * wave_of('normal', 700, 1)).astype(numpy.float32), wave_of('normal', 1, 2), wave_of('subnormal', fft // 2, 3), wave_of('overflow', 300, 4),
            wave_of('wide', 1234, 5)]


def check_powers_many(ctx, fft, hop=HOP, waves=None):
    """`gate_verdict_waves_device`, and `gate_waves_device` with feature rows, over `table_waves`: for every threshold of the sweep each wave's mask bytes
    and count are that wave's own host comparison; each wave's maximum is pinned through p_all."""
    made = make_core(ctx)
    core = made[0]
    waves = table_waves(fft) if waves is None else waves
    powers = [host_powers(x, fft, hop) for x in waves]
    frames = [len(p) for p in powers]
    assert all(numpy.isinf(p).all() or p.max() < OFF for p in powers) and any(numpy.isinf(p).all() for p in powers)
    rng = numpy.random.default_rng(43)
    feats = [(rng.normal(size=(n, CIN)) * synth.MC_SCALE).astype(numpy.float32) for n in frames]
    so = numpy.concatenate([[0], numpy.cumsum([x.size for x in waves])]).astype(numpy.int64)
    fo = numpy.concatenate([[0], numpy.cumsum(frames)]).astype(numpy.int32)
    n = int(fo[-1])
    B = M.Blocks(ctx)
    wave_block, feat_block = B.of(numpy.concatenate(waves)), B.of(numpy.concatenate(feats))
    mask_block, x_block, row_block = B.filled((n + 3) // 4), B.filled(n * CIN), B.filled(n)
    calls = 0

    def run(p_eff, p_all):
        want = [(p >= p_eff) | (p.max() >= p_all) for p in powers]
        tag = (fft, float(p_eff), float(p_all))
        for rows_too in (False, True):
            if rows_too:
                eff, n_eff = core.gate_waves_device(wave_block, so, fo, hop, fft, float(p_eff), float(p_all), feat_block, mask_block, x_block, row_block)
            else:
                eff, n_eff = core.gate_verdict_waves_device(wave_block, so, fo, hop, fft, float(p_eff), float(p_all), mask_block)
            ctx.sync()
            mask_bytes = B.read(mask_block, (n + 3) // 4).view(numpy.uint8)
            if rows_too:
                x_got, row_got = B.read(x_block, n * CIN).view(numpy.float32).reshape(n, CIN), B.read(row_block, n).view(numpy.int32)
            for i, w in enumerate(want):
                a, b, k = int(fo[i]), int(fo[i + 1]), int(w.sum())
                assert numpy.array_equal(eff[a:b], w) and numpy.array_equal(mask_bytes[a:b], w.astype(numpy.uint8)) and n_eff[i] == k, (tag, i, rows_too)
                if rows_too:
                    assert numpy.array_equal(row_got[a:a + k], numpy.flatnonzero(w)) and same_bits(x_got[a:a + k], feats[i][w]), (tag, i)
        return 2

    for v in sweep_values(numpy.concatenate(powers)):
        calls += run(v, OFF)
    for p in powers:
        top = p.max()
        if numpy.isinf(top):
            calls += run(numpy.inf, numpy.inf)
        else:
            calls += run(OFF, top)
            calls += run(OFF, next_up(top))
    B.close()
    close_core(made)
    return calls


# ---- the production thresholds at their boundary ---------------------------------------------------------------------------------------------------
def neighbours(centre, half=32):
    """The 2 * half + 1 consecutive positive float32 values centred on `centre`."""
    bits = int(numpy.float32(centre).view(numpy.uint32))
    return (bits + numpy.arange(-half, half + 1)).astype(numpy.uint32).view(numpy.float32)


def host_masks(wave, thr, fft):
    """The host's dB-domain mask, by the shim and by the loop-per-frame oracle; they must agree."""
    with numpy.errstate(all='ignore'):
        shim = host_wave.Wave(wave, FS).get_effective_frame(threshold_db=thr, fft_length=fft, frame_period=FP, ref='abs')
        oracle = oef.separate_effective_mask(wave, FS, len(shim), thr, fft, FP, 'abs')
    assert shim.dtype == bool and numpy.array_equal(shim, oracle), (thr, fft)
    return shim


def check_threshold_boundary(ctx, thrs=(20, 60, 80, 100), clamp=True):
    """Constant waves whose amplitude steps through the 65 float32 values around sqrt(p_eff): the host mask flips from no frame to every frame inside
    the range and the device mask equals it at every step.  Then the same around sqrt(p_all) at 100 dB, on a silent wave whose last 2 * fft samples
    hold the constant: the flip is between the few frames that touch the tail and all frames."""
    made = make_core(ctx)
    core = made[0]
    fft, checked = 512, 0
    rng = numpy.random.default_rng(44)
    for thr in thrs:
        p_eff, p_all = gate.thresholds(thr)
        seen = []
        for c in neighbours(numpy.sqrt(numpy.float32(p_eff))):
            wave = numpy.full(800, c, numpy.float32)
            want = host_masks(wave, thr, fft)
            feat = (rng.normal(size=(len(want), CIN)) * synth.MC_SCALE).astype(numpy.float32)
            eff, x_eff, rows = core.gate(wave, HOP, fft, p_eff, p_all, feat)
            assert numpy.array_equal(eff, want) and numpy.array_equal(x_eff, feat[want]), (thr, float(c))
            seen.append(int(want.sum()))
            checked += 1
        assert seen[0] == 0 and seen[-1] == len(want) and sorted(seen) == seen, (thr, seen)      # a condition on the inputs: the flip is inside
    if clamp:
        thr = 100
        p_eff, p_all = gate.thresholds(thr)
        seen = []
        for c in neighbours(numpy.sqrt(numpy.float32(p_all))):
            wave = numpy.zeros(2400, numpy.float32); wave[-2 * fft:] = c
            want = host_masks(wave, thr, fft)
            feat = (rng.normal(size=(len(want), CIN)) * synth.MC_SCALE).astype(numpy.float32)
            eff, x_eff, rows = core.gate(wave, HOP, fft, p_eff, p_all, feat)
            assert numpy.array_equal(eff, want) and numpy.array_equal(x_eff, feat[want]), ('clamp', float(c))
            seen.append(int(want.sum()))
            checked += 1
        assert 0 < seen[0] < len(want) and seen[-1] == len(want) and sorted(seen) == seen, seen
    close_core(made)
    return checked


# ---- NaN and inf samples -----------------------------------------------------------------------------------------------------------------------------
NONFINITE = {                                   # name: ((index, value) ...), what the host says
    'nan': (((617, numpy.nan),), 'none'),
    '+inf': (((617, numpy.inf),), 'all'),
    '-inf': (((617, -numpy.inf),), 'all'),
    'nan and inf': (((300, numpy.nan), (900, numpy.inf)), 'none'),
    'nan at both ends': (((0, numpy.nan), (-1, numpy.nan)), 'none'),
}
NF_FFT, NF_THR = 256, 60


def nonfinite_base(seed=0):
    w = wave_of('normal', 1234, 10 + seed)
    w[:400] *= numpy.float32(1e-6)
    return w


def nonfinite_wave(name):
    w = nonfinite_base()
    for i, v in NONFINITE[name][0]:
        w[i] = v
    return w


def check_nonfinite(ctx):
    """Every gate entry on waves with NaN and inf samples against the host (shim and oracle, which must agree): one NaN sample anywhere leaves no frame
    effective, one inf sample (and no NaN) makes every frame effective; the chained entries return what `convert` returns for that mask; in a
    table the clean neighbours of a NaN wave keep their host masks and counts."""
    made = make_core(ctx)
    core = made[0]
    rng = numpy.random.default_rng(45)
    p_eff, p_all = gate.thresholds(NF_THR)
    base_mask = host_masks(nonfinite_base(), NF_THR, NF_FFT)
    assert 0 < base_mask.sum() < len(base_mask)                                # the clean wave splits: 'none' and 'all' are both news
    for name, (_, verdict) in NONFINITE.items():
        wave = nonfinite_wave(name)
        want = host_masks(wave, NF_THR, NF_FFT)
        T = len(want)
        assert T == 1234 // HOP + 1 and (want.all() if verdict == 'all' else not want.any()), name
        feat = (rng.normal(size=(T, CIN)) * synth.MC_SCALE).astype(numpy.float32)
        mc_w, sp_w = core.convert(feat[want], want)
        # ry_vc_gate, at the feature length and one frame short of it
        for n in (T, T - 1):
            eff, x_eff, rows = core.gate(wave, HOP, NF_FFT, p_eff, p_all, feat[:n])
            assert numpy.array_equal(eff, want[:n]), (name, n, int(eff.sum()), int(want[:n].sum()))
            assert numpy.array_equal(rows, numpy.flatnonzero(want[:n])) and numpy.array_equal(x_eff, feat[:n][want[:n]]), (name, n)
        # ry_vc_submit_wave + ry_vc_wait_wave
        mc, sp, eff = core.wait_wave(core.submit_wave(wave, HOP, NF_FFT, p_eff, p_all, feat))
        assert numpy.array_equal(eff, want), (name, 'submit_wave', int(eff.sum()), int(want.sum()))
        assert same_bits(mc, mc_w) and same_bits(sp, sp_w), (name, 'submit_wave')
        # ry_vc_enqueue_wave_device
        B = M.Blocks(ctx)
        blocks = [B.of(wave), B.of(feat), B.filled(T * core.M), B.filled(T * core.F), B.filled((T + 3) // 4)]
        eff, n_eff = core.enqueue_wave_device(blocks[0], wave.size, HOP, NF_FFT, p_eff, p_all, blocks[1], T, *blocks[2:])
        ctx.sync()
        assert numpy.array_equal(eff, want) and n_eff == want.sum(), (name, 'enqueue_wave_device', n_eff, int(want.sum()))
        assert numpy.array_equal(B.read(blocks[4], (T + 3) // 4).view(numpy.uint8)[:T], want.astype(numpy.uint8)), name
        assert numpy.array_equal(B.read(blocks[2], T * core.M), mc_w.view(numpy.uint32).ravel()), (name, 'enqueue_wave_device mc')
        assert numpy.array_equal(B.read(blocks[3], T * core.F), sp_w.view(numpy.uint32).ravel()), (name, 'enqueue_wave_device sp')
        B.close()
        # the table entries: the wave between two clean ones
        waves = [nonfinite_base(1), wave, nonfinite_base(2)[:700]]
        wants = [host_masks(x, NF_THR, NF_FFT) for x in waves]
        assert 0 < wants[0].sum() < len(wants[0]) and 0 < wants[2].sum() < len(wants[2])
        feats = [(rng.normal(size=(len(m), CIN)) * synth.MC_SCALE).astype(numpy.float32) for m in wants]
        so = numpy.concatenate([[0], numpy.cumsum([x.size for x in waves])]).astype(numpy.int64)
        fo = numpy.concatenate([[0], numpy.cumsum([len(m) for m in wants])]).astype(numpy.int32)
        n = int(fo[-1])
        B = M.Blocks(ctx)
        wave_block, feat_block = B.of(numpy.concatenate(waves)), B.of(numpy.concatenate(feats))
        mask_block, x_block, row_block = B.filled((n + 3) // 4), B.filled(n * CIN), B.filled(n)
        for entry in ('gate_waves_device', 'gate_verdict_waves_device'):
            if entry == 'gate_waves_device':
                eff, n_eff = core.gate_waves_device(wave_block, so, fo, HOP, NF_FFT, p_eff, p_all, feat_block, mask_block, x_block, row_block)
            else:
                eff, n_eff = core.gate_verdict_waves_device(wave_block, so, fo, HOP, NF_FFT, p_eff, p_all, mask_block)
            ctx.sync()
            mask_bytes = B.read(mask_block, (n + 3) // 4).view(numpy.uint8)
            x_got, row_got = B.read(x_block, n * CIN).view(numpy.float32).reshape(n, CIN), B.read(row_block, n).view(numpy.int32)
            for i, m in enumerate(wants):
                a, b, k = int(fo[i]), int(fo[i + 1]), int(m.sum())
                assert n_eff[i] == k and numpy.array_equal(eff[a:b], m), (name, entry, i, int(n_eff[i]), k)
                assert numpy.array_equal(mask_bytes[a:b], m.astype(numpy.uint8)), (name, entry, i)
                if entry == 'gate_waves_device':
                    assert numpy.array_equal(row_got[a:a + k], numpy.flatnonzero(m)) and same_bits(x_got[a:a + k], feats[i][m]), (name, i)
                    assert (x_got[a + k:b].view(numpy.uint32) == M.GUARD).all() and (row_got[a + k:b].view(numpy.uint32) == M.GUARD).all(), (name, i)
        B.close()
    close_core(made)
    return len(NONFINITE)
