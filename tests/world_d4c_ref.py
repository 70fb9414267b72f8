"""WORLD `D4C` (band aperiodicity) and `code_aperiodicity` restated in numpy, the yardstick of `realtime_yukarin_amd.world_analysis.d4c`.

Neither `pyworld` nor WORLD's source can be read here, so -- as for CheapTrick (tests/world_analysis_ref.py) -- this is a restatement of the
published algorithm (Morise, "D4C, a band-aperiodicity estimator for high-quality speech synthesis", 2016; WORLD's d4c.cpp / codec.cpp); what is
written from memory is marked [MEM]; parity at the `pyworld` boundary is unpinned.  Per frame k with f0_k (Hz), t_k (s):

0. Sizes [MEM: d4c.cpp]: N = 2^(1 + floor(log2(4 fs / 47 + 1))), the Love-Train size 2^(1 + floor(log2(3 fs / 40 + 1))) (both 2048 at 16 and
   24 kHz), B = floor(min(15000, fs / 2 - 3000) / 3000) bands of 3000 Hz, a Nuttall window of 2 floor(3000 N / fs) + 1 samples.
1. Windowed wave W(f, pos, kind, ratio) [MEM: GetWindowedWaveform of d4c.cpp]: h = round(ratio fs / f / 2), samples round(pos fs + 0.001) + (-h .. h)
   clamped to the wave, window over p = (2 j / ratio) / fs: Hanning 0.5 cos(pi p f) + 0.5 or Blackman 0.42 + 0.5 cos(pi p f) + 0.08 cos(2 pi p f),
   NOT energy-normalised; wave x window + 1e-12 x noise, minus window x (sum of that / sum of the window).  `round` is WORLD's matlab_round
   (half away from zero): the shifted centres of step 3 are negative at t = 0.
2. Love Train [MEM: D4CLoveTrainSub]: unvoiced (f0 == 0): a0 = 0.  Else W(max(f0, 40), t, Blackman, 3), power spectrum at 2048, bins
   0 .. ceil(100 x 2048 / fs) zeroed, cumulative sum c, a0 = c[ceil(4000 x 2048 / fs)] / c[ceil(7900 x 2048 / fs)].  A frame is OFF when f0 == 0 or
   a0 <= threshold (0.85): its row is 1 - 1e-12 in every bin.
3. General body [MEM: D4CGeneralBody] with f = max(47, f0): centroid at pos: w = W(f, pos, Blackman, 4) / sqrt(sum w^2), S1 = rfft(w, N),
   S2 = rfft(w x (i + 1), N), Re S1 Re S2 + Im S1 Im S2; static centroid = centroid(t - 0.25 / f) + centroid(t + 0.25 / f), DC correction (CheapTrick's,
   at N, with f); smoothed power = |rfft(W(f, t, Hanning, 4), N)|^2, DC correction, linear smoothing of width f; group delay g = centroid / smoothed
   power, g = smooth(g, f / 2), g -= smooth(g, f).  Per band i = 1 .. B: c = floor(3000 i N / fs), g[c - half .. c + half] x Nuttall zero-padded to N,
   power spectrum (N / 2 + 1 values) sorted ascending, cumulative sum s, coarse_i = min(0, 10 log10(s[N/2 - 26] / s[N/2]) + (f - 100) / 50).
4. Row [MEM: GetAperiodicity]: [-60, coarse_1 .. coarse_B, -1e-12] dB over [0, 3000, .., 3000 B, fs / 2] Hz interpolated linearly at k fs / fft_size,
   then 10^(dB / 20).
`code_aperiodicity(ap, fs)` [MEM: codec.cpp]: 20 log10(ap) interpolated at 3000 i Hz -> [frames][B] (at 16 / 24 kHz these are bins 192 i / 128 i).

THE ONE DELIBERATE DEVIATION FROM `pyworld`, as in CheapTrick: the 1e-12 x randn() term is COUNTER-BASED (`world_synth_ref.noise`): the sample of
index j (0 .. 2 h) of window `which` (0 Love Train, 1 centroid at t - 0.25 / f, 2 centroid at t + 0.25 / f, 3 smoothed power) whose origin sample
is o has the key 2^62 + (o + 2^20) x 8192 + which x 2048 + j.  CheapTrick's keys of the same seed lie below 2^57 or (negative centres) above
2^64 - 2^57: disjoint.  A row therefore depends on (x, f0_k, t_k, seed) only.

`dtype` selects the arithmetic (float64: the yardstick; longdouble: the tolerance measurement, with `fft_any` instead of numpy's transform); the
integers (window half lengths, origins, DC-correction limit, smoothing boundaries) are always decided in float64, one rounded operation per step."""
import numpy

from world_analysis_ref import _pi, fft_any
from world_synth_ref import noise

THRESHOLD = 0.85
FLOOR_F0 = 47.0
LOVE_TRAIN_FLOOR = 40.0
BAND = 3000.0
UPPER_LIMIT = 15000.0
SAFEGUARD = 1e-12
KEY_BASE, KEY_BIAS, KEY_ORIGIN, KEY_WINDOW = 1 << 62, 1 << 20, 8192, 2048
LOVE_TRAIN, MINUS, PLUS, POWER = 0, 1, 2, 3
HANNING, BLACKMAN = 0, 1
NUTTALL = (0.355768, -0.487396, 0.144232, -0.012604)
INT_NAMES = ('h3', 'h4', 'o_minus', 'o_centre', 'o_plus', 'L', 'b1', 'b2')


def mround(v):
    """WORLD's matlab_round: half away from zero."""
    v = float(v)
    return int(numpy.floor(v + 0.5)) if v > 0 else -int(numpy.floor(-v + 0.5))


def fft_size_d4c(fs):
    return int(2 ** (1 + int(numpy.log2(4.0 * fs / FLOOR_F0 + 1.0))))


def fft_size_love_train(fs):
    return int(2 ** (1 + int(numpy.log2(3.0 * fs / LOVE_TRAIN_FLOOR + 1.0))))


def bands(fs):
    return int(min(UPPER_LIMIT, fs / 2.0 - BAND) / BAND)


def love_train_bins(fs):
    n = fft_size_love_train(fs)
    return tuple(-((-hz * n) // int(fs)) for hz in (100, 4000, 7900))          # ceil in integers


def frame_values(f0_k, t_k, fs):
    """(f, f of the Love Train, 1.5 fs / f_lt, 2 fs / f, the three positions x fs + 0.001, f N / fs, (f / 2) N / fs) -- float64, one operation per step."""
    n = fft_size_d4c(fs)
    fs, f0_k, t_k = float(fs), float(f0_k), float(t_k)
    f = f0_k if f0_k > FLOOR_F0 else FLOOR_F0
    fl = f0_k if f0_k > LOVE_TRAIN_FLOOR else LOVE_TRAIN_FLOOR
    r3 = (1.5 * fs) / fl
    r4 = (2.0 * fs) / f
    q = 0.25 / f
    cm = (t_k - q) * fs + 0.001
    cc = t_k * fs + 0.001
    cp = (t_k + q) * fs + 0.001
    p = (f * n) / fs
    u2 = ((f * 0.5) * n) / fs
    return f, fl, r3, r4, cm, cc, cp, p, u2


def frame_integers(f0_k, t_k, fs):
    """h3, h4, o_minus, o_centre, o_plus, L, b1, b2 (INT_NAMES): the device kernel does the same operations in the same order."""
    f, fl, r3, r4, cm, cc, cp, p, u2 = frame_values(f0_k, t_k, fs)
    L = int(numpy.floor(p))
    return mround(r3), mround(r4), mround(cm), mround(cc), mround(cp), L, L + 1, int(numpy.floor(u2)) + 1


def rounding_margins(f0_k, t_k, fs):
    """Distances of 1.5 fs / f_lt, 2 fs / f, the three origins, f N / fs and (f / 2) N / fs from the point where their rounding flips."""
    f, fl, r3, r4, cm, cc, cp, p, u2 = frame_values(f0_k, t_k, fs)

    def to_half(v):
        v = abs(v)
        return abs((v - numpy.floor(v)) - 0.5)

    def to_int(v):
        return min(v - numpy.floor(v), numpy.ceil(v) - v) if v != numpy.floor(v) else 0.0
    return to_half(r3), to_half(r4), to_half(cm), to_half(cc), to_half(cp), to_int(p), to_int(u2)


def integers(f0, temporal_positions, fs):
    return numpy.array([frame_integers(a, b, fs) for a, b in zip(f0, temporal_positions)], numpy.int64).reshape(-1, 8)


def rfft_any(a, n, dtype):
    buf = numpy.zeros(n, dtype)
    buf[:len(a)] = a
    return fft_any(buf, dtype)[:n // 2 + 1]


def power(s, dtype):
    return (s.real * s.real + s.imag * s.imag).astype(dtype)


def windowed(x, f, origin, h, kind, ratio, which, fs, seed, dtype):
    ft = numpy.dtype(dtype).type
    pi = _pi(dtype)
    fd = ft(f)
    j = numpy.arange(-h, h + 1)
    idx = numpy.clip(origin + j, 0, len(x) - 1)
    pos = ((ft(2) * j.astype(dtype)) / ft(ratio)) / ft(fs)
    if kind == HANNING:
        win = ft(0.5) * numpy.cos(pi * pos * fd) + ft(0.5)
    else:
        win = ft(0.42) + ft(0.5) * numpy.cos(pi * pos * fd) + ft(0.08) * numpy.cos(ft(2) * pi * pos * fd)
    key = KEY_BASE + (int(origin) + KEY_BIAS) * KEY_ORIGIN + which * KEY_WINDOW
    nz = noise(seed, numpy.uint64(key) + numpy.arange(2 * h + 1, dtype=numpy.uint64)).astype(dtype)
    wave = numpy.asarray(x)[idx].astype(dtype) * win + nz * ft(SAFEGUARD)
    return wave - win * (wave.sum() / win.sum())


def dc_correction(a, p, L):
    """CheapTrick's DC correction at the size of `a`: bins 0 .. L get a(p - i) added, a interpolated linearly between bins."""
    half = len(a) - 1
    frac = p - numpy.floor(p)
    i = numpy.arange(L + 1)
    lo = a[L - i]
    hi = a[numpy.minimum(L - i + 1, half)]
    out = a.copy()
    out[:L + 1] = out[:L + 1] + (lo + (hi - lo) * frac)
    return out


def linear_smoothing(a, u, b, dtype):
    """CheapTrick's linear smoothing of width u bins: mirrored by b bins at both ends, cumulative sum interpolated at i + (b - 0.5) -+ u / 2."""
    ft = numpy.dtype(dtype).type
    half = len(a) - 1
    seg = numpy.cumsum(numpy.concatenate([a[b:0:-1], a, a[half - 1::-1][:b]]))
    base = numpy.arange(half + 1).astype(dtype) + ft(b - 0.5)

    def at(pos):
        k = numpy.floor(pos).astype(numpy.int64)
        return seg[k] + (seg[k + 1] - seg[k]) * (pos - k.astype(dtype))
    return (at(base + u / 2) - at(base - u / 2)) / u


def love_train(x, f0_k, t_k, fs, seed=0, dtype=numpy.float64):
    if float(f0_k) == 0.0:
        return 0.0
    fl = frame_values(f0_k, t_k, fs)[1]
    h3, _, _, oc = frame_integers(f0_k, t_k, fs)[:4]
    w = windowed(x, fl, oc, h3, BLACKMAN, 3, LOVE_TRAIN, fs, seed, dtype)
    pw = power(rfft_any(w, fft_size_love_train(fs), dtype), dtype)
    b0, b1, b2 = love_train_bins(fs)
    pw[:b0 + 1] = 0
    c = numpy.cumsum(pw)
    return c[b1] / c[b2]


def nuttall(n, dtype):
    ft = numpy.dtype(dtype).type
    pi = _pi(dtype)
    tmp = numpy.arange(n).astype(dtype) / ft(n - 1)
    return ft(NUTTALL[0]) + ft(NUTTALL[1]) * numpy.cos(ft(2) * pi * tmp) + ft(NUTTALL[2]) * numpy.cos(ft(4) * pi * tmp) + ft(NUTTALL[3]) * numpy.cos(ft(6) * pi * tmp)


def general_body(x, f0_k, t_k, fs, seed=0, dtype=numpy.float64):
    """-> the B coarse values (dB) of a frame that is on."""
    ft = numpy.dtype(dtype).type
    n = fft_size_d4c(fs)
    f = frame_values(f0_k, t_k, fs)[0]
    h3, h4, om, oc, op, L, b1, b2 = frame_integers(f0_k, t_k, fs)
    fd, fsd = ft(f), ft(fs)
    p = (fd * n) / fsd
    u2 = ((fd * ft(0.5)) * n) / fsd
    ramp = numpy.arange(1, 2 * h4 + 2).astype(dtype)

    def centroid(origin, which):
        w = windowed(x, f, origin, h4, BLACKMAN, 4, which, fs, seed, dtype)
        w = w / numpy.sqrt((w * w).sum())
        s1, s2 = rfft_any(w, n, dtype), rfft_any(w * ramp, n, dtype)
        return (s1.real * s2.real + s1.imag * s2.imag).astype(dtype)
    cen = dc_correction(centroid(om, MINUS) + centroid(op, PLUS), p, L)
    pw = power(rfft_any(windowed(x, f, oc, h4, HANNING, 4, POWER, fs, seed, dtype), n, dtype), dtype)
    pw = linear_smoothing(dc_correction(pw, p, L), p, b1, dtype)
    g = cen / pw
    g = linear_smoothing(g, u2, b2, dtype)
    g = g - linear_smoothing(g, p, b1, dtype)
    half = (3000 * n) // int(fs)
    win = nuttall(2 * half + 1, dtype)
    coarse = []
    for i in range(1, bands(fs) + 1):
        c = (3000 * i * n) // int(fs)
        s = numpy.cumsum(numpy.sort(power(rfft_any(g[c - half:c + half + 1] * win, n, dtype), dtype)))
        v = ft(10) * numpy.log10(s[n // 2 - 26] / s[n // 2]) + (fd - ft(100)) / ft(50)
        coarse.append(min(ft(0), v))
    return numpy.array(coarse, dtype)


def aperiodicity_row(coarse, fs, fft_size, dtype=numpy.float64):
    ft = numpy.dtype(dtype).type
    nb = len(coarse)
    ys = numpy.concatenate([[ft(-60)], numpy.asarray(coarse, dtype), [ft(-SAFEGUARD)]])
    xs = numpy.array([BAND * i for i in range(nb + 1)] + [fs / 2.0], dtype)
    freq = numpy.arange(fft_size // 2 + 1).astype(dtype) * ft(fs) / ft(fft_size)
    j = numpy.minimum(numpy.floor(freq / ft(BAND)).astype(numpy.int64), nb)
    w = (freq - xs[j]) / (xs[j + 1] - xs[j])
    return ft(10) ** ((ys[j] + (ys[j + 1] - ys[j]) * w) / ft(20))


def d4c_frame(x, f0_k, t_k, fs, threshold=THRESHOLD, fft_size=1024, seed=0, dtype=numpy.float64):
    """-> (a0, on, coarse [B] (NaN when off), ap row [fft_size / 2 + 1])"""
    ft = numpy.dtype(dtype).type
    nb = bands(fs)
    a0 = love_train(x, f0_k, t_k, fs, seed, dtype)
    if float(f0_k) == 0.0 or not a0 > threshold:
        return a0, False, numpy.full(nb, numpy.nan, dtype), numpy.full(fft_size // 2 + 1, ft(1) - ft(SAFEGUARD), dtype)
    coarse = general_body(x, f0_k, t_k, fs, seed, dtype)
    return a0, True, coarse, aperiodicity_row(coarse, fs, fft_size, dtype)


def d4c(x, f0, temporal_positions, fs, threshold=THRESHOLD, fft_size=None, seed=0, dtype=numpy.float64, details=False):
    """-> aperiodicity [frames][fft_size / 2 + 1], argument order of `pyworld.d4c`.  details: -> (ap, a0 [frames], on [frames], coarse [frames][B])."""
    fft_size = fft_size or 1024
    f0, t = numpy.asarray(f0, numpy.float64).ravel(), numpy.asarray(temporal_positions, numpy.float64).ravel()
    ap = numpy.empty((len(f0), fft_size // 2 + 1), dtype)
    a0, on, coarse = numpy.zeros(len(f0), dtype), numpy.zeros(len(f0), bool), numpy.empty((len(f0), bands(fs)), dtype)
    for k in range(len(f0)):
        a0[k], on[k], coarse[k], ap[k] = d4c_frame(x, f0[k], t[k], fs, threshold, fft_size, seed, dtype)
    return (ap, a0, on, coarse) if details else ap


def code_aperiodicity(ap, fs):
    """-> [frames][B]: 20 log10(ap) at 3000 i Hz (linear interpolation between bins where 3000 i Hz is not one)."""
    ap = numpy.atleast_2d(ap)
    fft_size = 2 * (ap.shape[1] - 1)
    lg = 20 * numpy.log10(ap)
    out = numpy.empty((ap.shape[0], bands(fs)), ap.dtype)
    for i in range(1, bands(fs) + 1):
        pos = BAND * i * fft_size / fs
        k = int(numpy.floor(pos))
        out[:, i - 1] = lg[:, k] if pos == k else lg[:, k] + (lg[:, k + 1] - lg[:, k]) * (pos - k)
    return out
