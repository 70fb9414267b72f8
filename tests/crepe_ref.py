"""Independent restatement of CREPE for the tests: the network in torch float64 on the CPU (Conv1d with explicit 'same' padding,
ReLU, BatchNorm in inference form, MaxPool1d, Permute + Flatten, Linear, sigmoid), the framing, the decode (argmax, the 360-state
Viterbi pass as hmmlearn computes it, local-average cents) and the resampler (a direct windowed-sinc sum) in numpy float64."""
import numpy
import torch

BINS = 360
FRAME = 1024
PADS = ((254, 254), (31, 32), (31, 32), (31, 32), (31, 32), (31, 32))
STRIDES = (4, 1, 1, 1, 1, 1)


def frames(audio, hop, center=True):
    """(n, 1024) float64: zero padding of 512 each side when centred, mean / population-std normalisation, std clamped at 1e-10."""
    x = numpy.asarray(audio, dtype=numpy.float32).astype(numpy.float64)
    if center:
        x = numpy.pad(x, FRAME // 2)
    n = 1 + (len(x) - FRAME) // hop
    fr = numpy.stack([x[i * hop:i * hop + FRAME] for i in range(n)])
    fr = fr - fr.mean(axis=1, keepdims=True)
    return fr / numpy.maximum(fr.std(axis=1, keepdims=True), 1e-10)


def network(P, fr, eps=1e-3):
    """fr (n, 1024) -> (per-layer pooled outputs [(n, positions, channels)], logits (n, 360), activation (n, 360)), float64."""
    t = lambda k: torch.as_tensor(numpy.asarray(P[k], dtype=numpy.float64).reshape(numpy.asarray(P[k]).shape[:3]))
    x = torch.as_tensor(numpy.asarray(fr, dtype=numpy.float64))[:, None, :]
    outs = []
    for i in range(6):
        k = 'conv%d' % (i + 1)
        x = torch.nn.functional.pad(x, PADS[i])
        x = torch.nn.functional.conv1d(x, t(k + '.weight'), t(k + '.bias'), stride=STRIDES[i])
        x = torch.relu(x)
        b = k + '_BN.'
        x = (x - t(b + 'running_mean')[:, None]) / torch.sqrt(t(b + 'running_var')[:, None] + eps) * t(b + 'weight')[:, None] + t(b + 'bias')[:, None]
        x = torch.nn.functional.max_pool1d(x, 2)
        outs.append(x.permute(0, 2, 1).numpy().copy())
    flat = x.permute(0, 2, 1).reshape(x.shape[0], -1)
    logits = flat @ t('classifier.weight').T + t('classifier.bias')
    return outs, logits.numpy(), torch.sigmoid(logits).numpy()


def tables():
    xx, yy = numpy.meshgrid(range(BINS), range(BINS))
    T = numpy.maximum(12 - abs(xx - yy), 0)
    T = T / numpy.sum(T, axis=1)[:, None]
    E = numpy.eye(BINS) * 0.1 + numpy.ones((BINS, BINS)) * (0.9 / BINS)
    with numpy.errstate(divide='ignore'):
        return numpy.log(T), numpy.log(E), numpy.log(numpy.ones(BINS) / BINS)


def viterbi_path(obs):
    """The 360-state Viterbi path over the observations: lattice[t][j] = max_i (lattice[t-1][i] + logT[i][j]) + logE[j][obs t], first
    index on ties, backtrack by recomputing the argmax (hmmlearn's order)."""
    logT, logE, logS = tables()
    obs = numpy.asarray(obs)
    lat = numpy.empty((len(obs), BINS))
    lat[0] = logS + logE[:, obs[0]]
    for t in range(1, len(obs)):
        lat[t] = (lat[t - 1][:, None] + logT).max(axis=0) + logE[:, obs[t]]
    path = numpy.empty(len(obs), numpy.int64)
    path[-1] = numpy.argmax(lat[-1])
    for t in range(len(obs) - 2, -1, -1):
        path[t] = numpy.argmax(lat[t] + logT[:, path[t + 1]])
    return path


def local_average_cents(act, centers):
    cm = numpy.linspace(0, 7180, BINS) + 1997.3794084376191
    out = numpy.empty(len(act))
    for i, c in enumerate(centers):
        s, e = max(0, c - 4), min(BINS, c + 5)
        a = numpy.asarray(act[i, s:e], dtype=numpy.float64)
        with numpy.errstate(invalid='ignore', divide='ignore'):
            out[i] = numpy.sum(a * cm[s:e]) / numpy.sum(a)
    return out


def decode(act, viterbi=True):
    """activation (n, 360) -> (f0 float64 with NaN -> 0, confidence, centre bins)."""
    act = numpy.asarray(act)
    obs = numpy.argmax(act, axis=1)
    centers = viterbi_path(obs) if viterbi else obs
    with numpy.errstate(invalid='ignore'):
        f0 = 10 * 2 ** (local_average_cents(act, centers) / 1200)
    f0[numpy.isnan(f0)] = 0
    return f0, act.max(axis=1), centers


def sinc_resample(x, sr_orig, sr_new, num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596, at=None):
    """resampy's interpolation loop written out per output sample (scalar Python, float64) for the outputs `at` (default all): the
    Kaiser-windowed sinc table of 2^precision points per zero crossing, scaled for down-sampling, linearly interpolated; taps
    n - i on the left and n + 1 + k on the right of the output's time n + frac, stepping int(scale * 2^precision) table entries."""
    x = numpy.asarray(x, dtype=numpy.float64)
    ratio = sr_new / sr_orig
    scale = min(1.0, ratio)
    num_table = 2 ** precision
    n_half = num_table * num_zeros
    win = rolloff * numpy.sinc(rolloff * numpy.linspace(0, num_zeros, n_half + 1)) * numpy.kaiser(2 * n_half + 1, beta)[n_half:]
    if ratio < 1:
        win = win * ratio
    step = int(scale * num_table)
    n_out = int(len(x) * ratio)
    times = numpy.cumsum([0.0] + [1.0 / ratio] * (n_out - 1))
    out = []
    for t in (range(n_out) if at is None else at):
        n = int(times[t])
        acc = 0.0
        for side in (0, 1):
            frac = scale * (times[t] - n)
            if side:
                frac = scale - frac
            pos = frac * num_table
            off = int(pos)
            eta = pos - off
            i = 0
            while off + i * step <= n_half:
                src = n - i if side == 0 else n + 1 + i
                if src < 0 or src >= len(x):
                    break
                j = off + i * step
                nxt = win[j + 1] if j < n_half else win[j]
                acc += (win[j] + eta * (nxt - win[j])) * x[src]
                i += 1
        out.append(acc)
    return numpy.asarray(out)
