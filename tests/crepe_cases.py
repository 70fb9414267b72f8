"""Shared by tests/test_crepe_oracle.py (and tests/test_crepe_cpu.py): the float64 reference of ONE CREPE layer on the device's own input with an
element-wise error scale, the case lists of the emulator and the MI355X parts, the tile / split / pass branches a case takes (a restatement of
the planning code of csrc/crepe.cpp, for the case lists only), test signals and the tie activations of the decode tests."""
import numpy
import torch

import cases
from realtime_yukarin_amd import crepe

F32_TOL = cases.F32_TOL         # fp32: any summation order of the same products (the bar of the stage-1 and stage-2 oracle files)
ACT_TOL = 1e-6                  # |act - sigmoid64(device logits)|: float32 expf and one division on values in (0, 1)
CHAIN_TOL = 1e-4                # the end-to-end bar of tests/test_crepe_gpu.py: max |y - r| / max |r| through the whole float64 chain
BM, BN, BK = 128, 128, 32       # the tile of crepe_igemm
CHUNK = 256                     # frames per pass
PLAN_FRAMES, PLAN_WORKGROUPS = 201, 1000
NAMES = ('conv1', 'conv2', 'conv3', 'conv4', 'conv5', 'conv6', 'dense')


# ---- signals ----

def signal(n, seed):
    """n samples at 16 kHz: a gliding harmonic tone in noise (no silence: every frame has its own statistics)."""
    rng = numpy.random.default_rng(seed)
    t = numpy.arange(n) / 16000.0
    f = 150 + 60 * numpy.sin(2 * numpy.pi * 1.3 * t + seed)
    x = sum(numpy.sin(2 * numpy.pi * numpy.cumsum(f * k) / 16000.0) / k for k in (1, 2, 3)) + rng.normal(0, 0.3, n)
    return (0.3 * x).astype(numpy.float32)


def uncentred(frames, hop, seed):
    """a signal of exactly `frames` frames with center = False"""
    return signal(crepe.FRAME + (frames - 1) * hop, seed)


def tie_activations(n, seed):
    """Activations with many exact ties: flat rows, rows with two equal maxima, plateaus, and quantised rows."""
    rng = numpy.random.default_rng(seed)
    a = numpy.zeros((n, 360), numpy.float32)
    for t in range(n):
        kind = t % 4
        if kind == 0:
            a[t] = 0.5
        elif kind == 1:
            i, j = rng.integers(0, 360, 2)
            a[t, i] = a[t, j] = 0.75
        elif kind == 2:
            c = int(rng.integers(20, 340))
            a[t, c - 6:c + 6] = 0.6
        else:
            a[t] = rng.integers(0, 4, 360) / 4.0
    return a


# ---- the float64 reference of one layer ----

def _t(a):
    return torch.as_tensor(numpy.ascontiguousarray(numpy.asarray(a, dtype=numpy.float64)))


def layer_ref(P, i, x, eps=crepe.BN_EPS):
    """Conv layer i + 1 (i = 0 .. 5) in torch float64 on the input x the device itself read: (n, 1024) frames for i = 0, else the pooled output
    (n, positions, channels) of the layer before.  conv ('same' padding) + bias -> ReLU -> BN affine -> max-pool 2.
    -> (r, bound), both (n, positions / 2, Cout) float64.  bound = (conv(|x|, |W|) + |b|) |scale| + |shift| per element before the pool -- the scale
    of the rounding errors of any fp32 evaluation (ReLU is 1-Lipschitz) -- pooled with the same max: the pool is 1-Lipschitz too, so an output's error
    is at most the larger of its pair's."""
    k = 'conv%d' % (i + 1)
    F = torch.nn.functional
    W = _t(P[k + '.weight'])
    W = W.reshape(W.shape[:3])
    b = _t(P[k + '.bias'])
    gamma, beta, mean, var = (_t(P['%s_BN.%s' % (k, s)]) for s in ('weight', 'bias', 'running_mean', 'running_var'))
    scale = gamma / torch.sqrt(var + eps)
    shift = beta - mean * scale
    xt = _t(x)
    xt = xt[:, None, :] if i == 0 else xt.permute(0, 2, 1)
    xt = F.pad(xt, crepe.PADS[i])
    with torch.no_grad():
        c = F.conv1d(xt, W, b, stride=crepe.STRIDES[i])
        ca = F.conv1d(xt.abs(), W.abs(), b.abs(), stride=crepe.STRIDES[i])
        r = torch.relu(c) * scale[:, None] + shift[:, None]
        bound = ca * scale.abs()[:, None] + shift.abs()[:, None]
        r, bound = F.max_pool1d(r, 2), F.max_pool1d(bound, 2)
    return r.permute(0, 2, 1).numpy().copy(), bound.permute(0, 2, 1).numpy().copy()


def dense_ref(P, flat):
    """The classifier on the device's own conv6 output (n, 4, C6) (input index = position * C6 + channel) -> (logits, bound) (n, 360) float64,
    bound = |flat| |W|^T + |bias|."""
    x = numpy.asarray(flat, numpy.float64).reshape(len(flat), -1)
    W, b = numpy.asarray(P['classifier.weight'], numpy.float64), numpy.asarray(P['classifier.bias'], numpy.float64)
    return x @ W.T + b, numpy.abs(x) @ numpy.abs(W).T + numpy.abs(b)


def sigmoid64(logits):
    return 1.0 / (1.0 + numpy.exp(-numpy.asarray(logits, numpy.float64)))


# ---- which tiles, splits and passes a case takes: labels for the case lists only, never used by a correctness assertion ----
# A restatement of ry_crepe_create / launch_layer / ry_crepe_predict (csrc/crepe.cpp): layer shapes, the split-K counts planned for 201 frames, the
# grid (N tiles, M tiles, splits) of every pass of at most 256 frames, and split z's chunks [z nch / splits, (z + 1) nch / splits).

def layer_shapes(m):
    """[(name, output rows per frame, N, K)] of conv1 .. conv6 and the dense layer at multiplier m"""
    out, cin, lin = [], 1, crepe.FRAME
    for i, (f, w, s) in enumerate(zip(crepe.FILTERS, crepe.WIDTHS, crepe.STRIDES)):
        out.append((NAMES[i], lin // s, f * m, w * cin))
        cin, lin = f * m, lin // s // 2
    return out + [('dense', 1, crepe.BINS, 4 * cin)]


def splits(m):
    """the split-K count of every layer (CrepeModel.splits)"""
    out = []
    for name, lout, N, K in layer_shapes(m):
        tiles = -(-PLAN_FRAMES * lout // BM) * -(-N // BN)
        out.append(max(1, min((K // BK) // (4 if name == 'dense' else 16), -(-PLAN_WORKGROUPS // tiles))))
    return out


def branches(m, frames):
    """-> the set of labels of a call of `frames` frames at multiplier m (see BRANCHES)"""
    out = set()
    passes = [min(CHUNK, frames - f) for f in range(0, frames, CHUNK)]
    if len(passes) > 1:
        out.add('several passes')
        if passes[-1] < CHUNK:
            out.add('shorter last pass')
    for (name, lout, N, K), sp in zip(layer_shapes(m), splits(m)):
        nch = K // BK
        out.add('%s: %s' % (name, 'split' if sp > 1 else 'unsplit'))
        out.add('%s: %s' % (name, 'several N tiles' if N > BN else 'one N tile'))
        if sp > 1 and nch % sp:
            out.add('uneven split')
        if sp > 1 and name == 'dense':
            out.add('dense split')
        if N > BN and N % BN:
            out.add('ragged last N tile')
            if N % 32:
                out.add('N % 32 != 0 in a later tile')
        for nf in passes:
            M = nf * lout
            out.add('%s: %s' % (name, 'several M tiles' if M > BM else 'one M tile'))
            if M % BM:
                out.add('%s: ragged last M tile' % name)
            if M == 1:
                out.add('M = 1')
            if M > 1 and M % BM in (1, BM - 1):
                out.add('M one row %s a tile edge' % ('past' if M % BM == 1 else 'short of'))
            if sp > 1 and name == 'dense' and M == 1:
                out.add('dense split with M = 1')
    return out


# every label a multiplier 1 .. 32 and a frame count can reach.  conv1 (16 chunks of K, two M tiles per frame) never splits and never has one M tile;
# conv1 and conv2 rows per frame are multiples of 128; conv2 .. conv4 have at most 128 channels; conv2 (>= 64 chunks) and the dense layer's 360 columns
# always split / span three tiles
BRANCHES = (
    {'conv1: unsplit', 'conv1: one N tile', 'conv1: several N tiles', 'conv1: several M tiles',
     'conv2: split', 'conv2: one N tile', 'conv2: one M tile', 'conv2: several M tiles'} |
    {'%s: %s' % (n, l) for n in ('conv3', 'conv4') for l in ('split', 'unsplit', 'one N tile', 'one M tile', 'several M tiles', 'ragged last M tile')} |
    {'%s: %s' % (n, l) for n in ('conv5', 'conv6') for l in ('split', 'unsplit', 'one N tile', 'several N tiles', 'one M tile', 'several M tiles',
                                                              'ragged last M tile')} |
    {'dense: %s' % l for l in ('split', 'unsplit', 'several N tiles', 'one M tile', 'several M tiles', 'ragged last M tile')} |
    {'several passes', 'shorter last pass', 'uneven split', 'dense split', 'dense split with M = 1', 'ragged last N tile', 'N % 32 != 0 in a later tile',
     'M = 1', 'M one row past a tile edge', 'M one row short of a tile edge'})

# (multiplier, frames), hop 80, center = False
EMU_CASES = ([(m, f) for m in (1, 2, 5) for f in (1, 2, 17)] +
             [(4, 1),          # the dense layer split over K (crepe_igemm<RAW, 7> + crepe_reduce_sig) with M = 1
              (9, 1),          # conv1 N = 288 = 2 * 128 + 32, conv6 N = 144 = 128 + 16
              (1, 257)])       # two passes, the second of one frame
# what the emulator list leaves to the MI355X: conv5 has more than 128 channels from m = 17 on; 127 / 129 rows of the dense layer cost the emulator minutes
EMU_UNREACHED = {'conv5: several N tiles', 'M one row past a tile edge', 'M one row short of a tile edge'}
GPU_CASES = ([(m, 17) for m in (1, 3, 5, 9, 17, 4, 8, 16, 24, 32)] +                          # conv6 M = 136, dense M = 17
             [(2, f) for f in (1, 2, 15, 16, 127, 128, 129, 255, 256, 257, 513)] +
             [(4, 1)])                                                                          # the dense layer split over K with M = 1

HOP_CASES = [(hop, center) for hop in (1, 16, 80, 160, 1000) for center in (False, True)]
DECODE_FRAMES = (1, 2, 3, 4, 383, 384, 385, 1000)


def hop_case_signal(hop, center, seed):
    """3 .. 40 frames for every hop: six frames, nine for the centred hop of one sample"""
    n = max(5 * hop + 3, 8) if center else crepe.FRAME + 5 * hop + min(hop - 1, 3)
    assert 3 <= crepe.n_frames(n, hop, center) <= 40
    return signal(n, seed)
