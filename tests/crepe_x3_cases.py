"""Shared by tests/test_crepe_x3_cpu.py, tests/test_crepe_x3_gpu.py and scripts/crepe_x3_tolerance.py: the split-bf16 mode of the CREPE network
(`CrepeModel.set_dtype('bf16x3')`, crepe_igemm_x3 in csrc/crepe_kernels.h).

The restatement (numpy, no device): one layer as the kernel computes it -- the RNE split hi = bf16(v), lo = bf16(v - hi) of the fp32 input and of the
filters, per K step of 16 the three products x_lo w_hi, x_hi w_lo, x_hi w_hi in that order, every product added to a float32 accumulator one by one in
rising k, chunks of 64 in the split ranges [z nch / splits, (z + 1) nch / splits), the slabs summed from 0 in rising z, the fp32 epilogue.  The matrix
instruction's own summation order inside a step is not documented; one by one is the order with the most roundings, and the bars leave a factor 4 for
the others (scripts/crepe_x3_tolerance.py).  The yardstick of the tests is not this restatement but float64 on the device's own input
(crepe_cases.layer_ref / dense_ref), within the bars that the script derived from the restatement and wrote to profiles/r14/crepe_x3_tolerance.txt.
Also here: the case lists, the branch labels of the mode (a restatement of the planning code, for the case lists only) and the test bodies."""
from pathlib import Path

import numpy

import cases
import crepe_cases as cc
import crepe_ref
from realtime_yukarin_amd import crepe

BK3 = 64                        # K chunk of crepe_igemm_x3
HOP = 80
NAMES = cc.NAMES
BARS_FILE = Path(__file__).resolve().parent.parent / 'profiles' / 'r14' / 'crepe_x3_tolerance.txt'
SANITY_CEILING = 3 * 2.0 ** -18     # the derivable worst case of one product: two dropped terms and the split of 2^-17, in units of |x| |w|


# ---- the case lists: (multiplier, frames), hop 80, center = False ----

EMU_CASES = [(1, 1),            # M = 1 in the dense layer, which has one chunk of K; every conv layer but conv2 unsplit
             (1, 3),            # ragged last M tiles of conv3 .. conv6 (192, 96, 48, 24 rows)
             (4, 1),            # the dense layer split over K with M = 1; conv2 split 5 ways over 128 chunks (uneven); conv1 N = 128
             (4, 2)]
# what the emulator list leaves to the MI355X (the emulator list stays at multipliers 1 and 4 and a few frames)
EMU_UNREACHED = {'conv1: several N tiles', 'conv5: several N tiles', 'conv6: several N tiles', 'conv4: several M tiles', 'conv5: several M tiles',
                 'conv6: several M tiles', 'dense: several M tiles', 'several passes', 'shorter last pass',
                 'M one row past a tile edge', 'M one row short of a tile edge'}
GPU_CASES = [(1, 17), (4, 1), (4, 3),
             (9, 17),           # conv1 N = 288, conv6 N = 144 = 128 + 16
             (17, 17),          # conv5 N = 136 = 128 + 8
             (2, 127), (2, 128), (2, 129),      # the dense layer one row either side of a tile
             (2, 257),          # a second pass of one frame
             (32, 3)]           # full capacity: uneven splits 1024 / 5, 128 / 10, 256 / 20


def splits(m):
    """the split-K count of every layer in the mode (CrepeModel.splits after set_dtype('bf16x3')): the fp32 plan in chunks of 64, floors 8 / 2"""
    out = []
    for name, lout, N, K in cc.layer_shapes(m):
        tiles = -(-cc.PLAN_FRAMES * lout // cc.BM) * -(-N // cc.BN)
        out.append(max(1, min((K // BK3) // (2 if name == 'dense' else 8), -(-cc.PLAN_WORKGROUPS // tiles))))
    return out


def branches(m, frames):
    """crepe_cases.branches for the mode: the same labels, with the chunk of 64 and the mode's split counts"""
    out = set()
    passes = [min(cc.CHUNK, frames - f) for f in range(0, frames, cc.CHUNK)]
    if len(passes) > 1:
        out.add('several passes')
        if passes[-1] < cc.CHUNK:
            out.add('shorter last pass')
    for (name, lout, N, K), sp in zip(cc.layer_shapes(m), splits(m)):
        assert K % BK3 == 0, (name, K)
        nch = K // BK3
        out.add('%s: %s' % (name, 'split' if sp > 1 else 'unsplit'))
        out.add('%s: %s' % (name, 'several N tiles' if N > cc.BN else 'one N tile'))
        if sp > 1 and nch % sp:
            out.add('uneven split')
        if sp > 1 and name == 'dense':
            out.add('dense split')
        if N > cc.BN and N % cc.BN:
            out.add('ragged last N tile')
            if N % 32:
                out.add('N % 32 != 0 in a later tile')
        for nf in passes:
            M = nf * lout
            out.add('%s: %s' % (name, 'several M tiles' if M > cc.BM else 'one M tile'))
            if M % cc.BM:
                out.add('%s: ragged last M tile' % name)
            if M == 1:
                out.add('M = 1')
            if M > 1 and M % cc.BM in (1, cc.BM - 1):
                out.add('M one row %s a tile edge' % ('past' if M % cc.BM == 1 else 'short of'))
            if sp > 1 and name == 'dense' and M == 1:
                out.add('dense split with M = 1')
    return out


# ---- the restatement ----

def split_rne(a):
    """float32 -> (hi, lo), both bf16 values held in float32, both rounded to nearest even (ry_split_bf16)"""
    return cases.bf16_split(a)


def split_trunc_lo(a):
    """a mutant: lo cut off instead of rounded"""
    a = numpy.ascontiguousarray(a, dtype=numpy.float32)
    hi = cases.bf16_round(a)
    lo = ((a - hi).view(numpy.uint32) & numpy.uint32(0xffff0000)).view(numpy.float32)
    return hi, lo


PRODUCTS = ('lo hi', 'hi lo', 'hi hi')      # x first; the order inside a K step of 16


def gemm_x3(A, W, sp, drop=None, split_x=split_rne, split_w=split_rne):
    """A (M, K) float32, W (N, K) float32, sp K splits -> (M, N) float32 as crepe_igemm_x3 (+ the split-K reduce) sums it.
    drop: a product of PRODUCTS that is left out (a mutant)."""
    M, K = A.shape
    assert K % BK3 == 0 and W.shape[1] == K
    xh, xl = (numpy.ascontiguousarray(v.T) for v in split_x(A))
    wh, wl = (numpy.ascontiguousarray(v.T) for v in split_w(W))
    pairs = [pr for name, pr in zip(PRODUCTS, ((xl, wh), (xh, wl), (xh, wh))) if name != drop]
    nch = K // BK3
    total = numpy.zeros((M, W.shape[0]), numpy.float32)
    for z in range(sp):
        acc = numpy.zeros_like(total)
        for k0 in range(BK3 * (z * nch // sp), BK3 * ((z + 1) * nch // sp), 16):
            for x, w in pairs:
                for k in range(k0, k0 + 16):
                    acc += x[k][:, None] * w[k][None, :]            # a product of two bf16 values is exact in float32: one rounding, the sum's
        total = total + acc if sp > 1 else acc
    return total


def conv_matrices(P, i, x, eps=crepe.BN_EPS, dtype=numpy.float32):
    """Conv layer i + 1 on its input x ((n, 1024) frames for i = 0, else (n, positions, channels)), float32 ->
    A (n lout, K) with k = tap Cin + ci, W (N, K), bias, scale, shift (the BN affine as ry_crepe_create computes it: float64, then one rounding)"""
    k = 'conv%d' % (i + 1)
    x = numpy.asarray(x, dtype)
    x = x[:, :, None] if i == 0 else x
    xp = numpy.pad(x, ((0, 0), crepe.PADS[i], (0, 0)))
    win = numpy.lib.stride_tricks.sliding_window_view(xp, crepe.WIDTHS[i], axis=1)[:, ::crepe.STRIDES[i]]     # (n, lout, cin, width)
    A = numpy.ascontiguousarray(win.transpose(0, 1, 3, 2)).reshape(win.shape[0] * win.shape[1], -1)
    W = numpy.asarray(P[k + '.weight'], numpy.float32)
    W = numpy.ascontiguousarray(W.reshape(W.shape[:3]).transpose(0, 2, 1)).reshape(W.shape[0], -1)
    g, be, mu, var = (numpy.asarray(P['%s_BN.%s' % (k, s)], numpy.float64) for s in ('weight', 'bias', 'running_mean', 'running_var'))
    s = g / numpy.sqrt(var + numpy.float64(numpy.float32(eps)))
    return A, W, numpy.asarray(P[k + '.bias'], numpy.float32), s.astype(numpy.float32), (be - mu * s).astype(numpy.float32)


def pool_epilogue(acc, b, sc, sh, n):
    """bias -> ReLU -> BN affine -> max of the row pair, float32 -> (n, positions / 2, N)"""
    v = numpy.maximum(acc + b[None, :], numpy.float32(0)) * sc[None, :] + sh[None, :]
    v = v.reshape(n, -1, 2, v.shape[1])
    return numpy.maximum(v[:, :, 0], v[:, :, 1])


def conv_x3(P, i, x, sp, **kw):
    """conv layer i + 1 in the mode on the fp32 input x -> pooled output (n, positions / 2, N) float32"""
    A, W, b, sc, sh = conv_matrices(P, i, x)
    return pool_epilogue(gemm_x3(A, W, sp, **kw), b, sc, sh, len(x))


def conv_exact(P, i, x):
    """the same layer in float64 with its element-wise bound (numpy; crepe_cases.layer_ref is the torch statement of the same)"""
    A, W, b, _, _ = conv_matrices(P, i, x)
    k = 'conv%d' % (i + 1)
    g, be, mu, var = (numpy.asarray(P['%s_BN.%s' % (k, s)], numpy.float64) for s in ('weight', 'bias', 'running_mean', 'running_var'))
    s = g / numpy.sqrt(var + crepe.BN_EPS)
    A, W, b = A.astype(numpy.float64), W.astype(numpy.float64), b.astype(numpy.float64)
    r = numpy.maximum(A @ W.T + b, 0) * s + (be - mu * s)
    bound = (numpy.abs(A) @ numpy.abs(W).T + numpy.abs(b)) * numpy.abs(s) + numpy.abs(be - mu * s)
    pool = lambda v: v.reshape(len(x), -1, 2, v.shape[1]).max(axis=2)
    return pool(r), pool(bound)


def dense_x3(P, flat, sp, **kw):
    """the classifier's logits in the mode on the fp32 conv6 output (n, 4, C6)"""
    A = numpy.asarray(flat, numpy.float32).reshape(len(flat), -1)
    return gemm_x3(A, numpy.asarray(P['classifier.weight'], numpy.float32), sp, **kw) + numpy.asarray(P['classifier.bias'], numpy.float32)[None, :]


def network_x3(P, m, fr32, **kw):
    """the whole network in the mode on float32 frames -> [input of conv1, .. input of the dense layer, logits], float32"""
    sp = splits(m)
    L = [numpy.asarray(fr32, numpy.float32)]
    for i in range(6):
        L.append(conv_x3(P, i, L[i], sp[i], **kw))
    return L + [dense_x3(P, L[6], sp[6], **kw)]


def network_f32(P, fr32):
    """the whole network in float32 (numpy's matrix product: some order of the fp32 products) -> the same list"""
    L = [numpy.asarray(fr32, numpy.float32)]
    for i in range(6):
        A, W, b, sc, sh = conv_matrices(P, i, L[i])
        L.append(pool_epilogue(A @ W.T, b, sc, sh, len(fr32)))
    A = L[6].reshape(len(fr32), -1)
    return L + [A @ numpy.asarray(P['classifier.weight'], numpy.float32).T + numpy.asarray(P['classifier.bias'], numpy.float32)[None, :]]


def network_f64(P, fr32):
    """the chain in float64 on the same float32 frames -> logits"""
    x = numpy.asarray(fr32, numpy.float64)
    for i in range(6):
        A, W, b, _, _ = conv_matrices(P, i, x, dtype=numpy.float64)
        k = 'conv%d' % (i + 1)
        g, be, mu, var = (numpy.asarray(P['%s_BN.%s' % (k, s)], numpy.float64) for s in ('weight', 'bias', 'running_mean', 'running_var'))
        s = g / numpy.sqrt(var + crepe.BN_EPS)
        r = numpy.maximum(A @ W.astype(numpy.float64).T + b.astype(numpy.float64), 0) * s + (be - mu * s)
        x = r.reshape(len(fr32), -1, 2, r.shape[1]).max(axis=2)
    return x.reshape(len(fr32), -1) @ numpy.asarray(P['classifier.weight'], numpy.float64).T + numpy.asarray(P['classifier.bias'], numpy.float64)


def params(m):
    return crepe.synthetic_params(m, 20 + m)


def frames32(m, frames):
    """the float32 frames of the (m, frames) case: the float64 framing, rounded once"""
    return crepe_ref.frames(cc.uncentred(frames, HOP, 100 * m + frames), HOP, False).astype(numpy.float32)


def sine(f, n_frames, sr=16000):
    """n_frames frames (hop 80, uncentred) of a sine of f Hz with a weak second harmonic"""
    t = numpy.arange(crepe.FRAME + (n_frames - 1) * HOP) / float(sr)
    return (0.5 * numpy.sin(2 * numpy.pi * f * t) + 0.05 * numpy.sin(4 * numpy.pi * f * t + 0.3)).astype(numpy.float32)


SINES = (110.0, 220.0, 440.0)
SINE_M, SINE_FRAMES = 4, 3


# ---- the bars (profiles/r14/crepe_x3_tolerance.txt, written by scripts/crepe_x3_tolerance.py) ----

def bars():
    """{'conv1': bar, .., 'dense': bar, 'act': bar} -- the layer bars in units of the element's bound, the activation bar absolute"""
    out = {}
    for line in BARS_FILE.read_text().splitlines():
        if line.startswith('bar '):
            out[line.split()[1]] = float(line.split()[-1])
    assert set(out) == set(NAMES) | {'act'}, sorted(out)
    return out


def f0_allowance(act, path, d):
    """|f0' / f0 - 1| a change of at most d in every activation can cause: f0 = 10 * 2^(c / 1200), c the average of the cents of bins
    [p - 4, p + 5) weighted by the activation.  dc <= d * sum |cents_b - c| / (sum a - 9 d); the window spans 160 cents; one float32 rounding of f0."""
    out = numpy.empty(len(path))
    for t, p in enumerate(path):
        s = float(numpy.asarray(act[t, max(0, p - 4):min(360, p + 5)], numpy.float64).sum())
        n = min(360, p + 5) - max(0, p - 4)
        dc = d * n * 160.0 / (s - n * d)
        out[t] = 2.0 ** (dc / 1200.0) - 1 + 2.0 ** -23
    return out


# ---- test bodies (ms: a Models of test_crepe_oracle.py whose models run in the mode) ----

def check_case(ms, m, frames, predict, report=None):
    """every conv layer and the dense layer of the last pass, element by element, against float64 on the input the device itself read"""
    B = bars()
    model, P = ms.get(m)
    assert model.dtype == 'bf16x3' and model.splits() == splits(m), (m, model.splits(), splits(m))
    audio, out = ms.run(m, frames)
    what = 'bf16x3 m %d, %d frames' % (m, frames)
    L = out['layers']
    n, last = out['n'], out['last']
    assert n == frames and out['act'].shape == (n, 360)
    fr = crepe_ref.frames(audio, HOP, False)[n - last:]
    assert numpy.all(numpy.abs(L[0].astype(numpy.float64) - fr) <= 2.0 ** -24 * numpy.abs(fr) + 1e-12), (what, 'frames')
    worst = {}
    for i in range(6):
        r, bound = cc.layer_ref(P, i, L[i])
        print('%-28s %-6s' % (what, NAMES[i]), end=' ')
        ratio = numpy.abs(L[i + 1].astype(numpy.float64) - r) / bound
        print('worst |y - r| / bound %.3g  bar %.3g' % (float(ratio.max()), B[NAMES[i]]))
        worst[NAMES[i]] = cases.assert_close_elementwise(L[i + 1], r, bound, B[NAMES[i]], '%s %s' % (what, NAMES[i]))
    r, bound = cc.dense_ref(P, L[6])
    ratio = numpy.abs(L[7].astype(numpy.float64) - r) / bound
    print('%-28s %-6s worst |y - r| / bound %.3g  bar %.3g' % (what, 'dense', float(ratio.max()), B['dense']))
    worst['dense'] = cases.assert_close_elementwise(L[7], r, bound, B['dense'], '%s dense' % what)
    act_err = float(numpy.abs(out['act'][n - last:] - cc.sigmoid64(L[7])).max())
    assert act_err <= cc.ACT_TOL, (what, act_err)
    f0_ref, conf_ref, _ = crepe_ref.decode(out['act'], viterbi=True)
    assert numpy.array_equal(out['conf'], conf_ref), what
    assert numpy.allclose(out['f0'], f0_ref, rtol=1e-6, atol=0), what
    if report is not None:
        report.append((what, worst))
    return worst


def check_against_f32(model_x3, model_f32, audio, what, sr=16000):
    """the activation within the bar of the fp32 path's; on a signal with a clear peak also the same path and f0 within what the bar allows"""
    B = bars()
    a = model_x3.predict(audio, sr, HOP, center=False)
    b = model_f32.predict(audio, sr, HOP, center=False)
    d = float(numpy.abs(a[2].astype(numpy.float64) - b[2]).max())
    print('%-36s |act_x3 - act_f32| %.3g  bar %.3g' % (what, d, B['act']))
    assert d <= B['act'], (what, d, B['act'])
    return a, b
