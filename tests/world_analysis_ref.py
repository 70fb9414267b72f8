"""WORLD `CheapTrick` and SPTK `sp2mc` restated in numpy, the yardstick of `realtime_yukarin_amd.world_analysis`.

Neither `pyworld` nor `pysptk` can be imported here and the reference tree holds no WORLD / SPTK source, so -- as for the CNNs, `mc2sp` and
the synthesis -- this is a restatement of the published algorithms; what is written from memory is marked [MEM]; parity at the
`pyworld` / `pysptk` boundary is unpinned.  Per frame k with f0_k (Hz) and t_k (s):

1. f0 = f0_k if f0_k > f0_floor else 500 Hz; f0_floor defaults to 71 Hz and is never below 3 fs / (fft_size - 3) [MEM: CheapTrick's own check].
2. Window [MEM: GetWindowedWaveform]: half length h = round(1.5 fs / f0), samples round(t_k fs + 0.001) + (-h .. h) clamped to the wave, Hanning
   0.5 cos(pi j / (1.5 fs / f0)) + 0.5 normalised to unit energy; the windowed wave gets 1e-12 x noise added, then the window times
   (sum of the windowed wave / sum of the window) is taken off.
3. Power spectrum at fft_size; DC correction [MEM: DCCorrection + interp1Q]: with p = f0 fft_size / fs, L = int(p), bins i = 0 .. L get
   P(p - i) added, P interpolated linearly between bins (the replica of the spectrum mirrored around f0); linear smoothing of width
   2 f0 / 3 [MEM: LinearSmoothing]: the spectrum mirrored by b = int(u) + 1 bins at both ends (u = the width in bins), its cumulative sum
   interpolated linearly at i + (b - 0.5) -+ u / 2, difference / u; then eps x |noise| is added (AddInfinitesimalNoise: the floor).
4. Smoothing with recovery [MEM: SmoothingWithRecovery]: log, transform of the mirrored log spectrum, times sin(pi f0 q) / (pi f0 q) and
   (1 - 2 q1) + 2 q1 cos(2 pi f0 q) at q = i / fs, / fft_size, transform back, exp.

THE ONE DELIBERATE DEVIATION FROM `pyworld`: WORLD draws the two noise terms from a process-global `randn()` sequence; here they are
COUNTER-BASED like the synthesis noise (`world_synth_ref.noise`): sample `centre * 2048 + j` (j = index in the window, 0 .. 2 h) for the
wave and `centre * 2048 + 1024 + bin` for the floor, centre = round(t_k fs + 0.001).  A frame's row therefore depends on
(x, f0_k, t_k, seed) only, not on which other frames share a call.  These terms are what keeps an all-zero wave finite.

`sp2mc(sp, order, alpha)` [MEM: pysptk.sp2mc]: c = irfft(log sp), c[0] /= 2, freqt(c, order, alpha) -- `freqt` as the plain per-frame SPTK
recursion, sharing no code with `realtime_yukarin_amd/sptk.py`.  Whether pysptk hands `freqt` all 1024 cepstral values or the first 513 is
[MEM]; the two differ by terms of order alpha^511 (below 1e-160 for alpha < 0.5), which cannot be told apart in float64: the results are
the same bits (tests/test_world_analysis_ref.py).  This file hands over the first fft_size / 2 + 1.

`dtype` selects the arithmetic (float64: the yardstick; longdouble: the tolerance measurement, with the transform below instead of
numpy's, which computes in float64); the integers (h, centre, L, b) are always decided in float64."""
import numpy

from world_synth_ref import cheaptrick_fft_size, noise

DEFAULT_F0 = 500.0
SAFEGUARD = 1e-12
EPS = 2.220446049250313e-16
KEY_STRIDE = 2048


def effective_floor(fs, fft_size, f0_floor=71.0):
    return max(float(f0_floor), 3.0 * fs / (fft_size - 3.0))


def frame_integers(f0_k, t_k, fs, fft_size, f0_floor):
    """(f0 used, h, centre, L, b, u) -- float64, one operation per step: the device kernel does the same operations in the same order."""
    f0 = float(f0_k) if float(f0_k) > effective_floor(fs, fft_size, f0_floor) else DEFAULT_F0
    fs = float(fs)
    r = (1.5 * fs) / f0
    h = int(numpy.floor(r + 0.5))
    centre = int(numpy.floor((float(t_k) * fs + 0.001) + 0.5))
    p = (f0 * fft_size) / fs
    L = min(int(numpy.floor(p)), fft_size // 2 - 1)
    u = (((f0 * 2.0) / 3.0) * fft_size) / fs
    b = int(numpy.floor(u)) + 1
    return f0, h, centre, L, b, u


def rounding_margins(f0_k, t_k, fs, fft_size, f0_floor=71.0):
    """Distance of 1.5 fs / f0, t fs + 0.001, f0 fft_size / fs and the smoothing width in bins from the point where their rounding flips."""
    f0 = frame_integers(f0_k, t_k, fs, fft_size, f0_floor)[0]
    fs = float(fs)

    def to_half(v):
        return abs((v - numpy.floor(v)) - 0.5)

    def to_int(v):
        return min(v - numpy.floor(v), numpy.ceil(v) - v) if v != numpy.floor(v) else 0.0
    return (to_half((1.5 * fs) / f0), to_half(float(t_k) * fs + 0.001), to_int((f0 * fft_size) / fs), to_int((((f0 * 2.0) / 3.0) * fft_size) / fs))


# ---- a transform that computes in the dtype it is given (numpy's computes in float64) ----------------------------------------------
def _pi(dtype):
    return numpy.dtype(dtype).type(4) * numpy.arctan(numpy.dtype(dtype).type(1))


def fft_any(a, dtype):
    """Forward DFT of the last axis (power of two), radix-2 decimation in time, in `dtype`'s complex type."""
    if numpy.dtype(dtype) == numpy.float64:
        return numpy.fft.fft(a)
    ct = numpy.result_type(dtype, numpy.complex64)
    a = numpy.asarray(a).astype(ct)
    n = a.shape[-1]
    bits = n.bit_length() - 1
    idx = numpy.arange(n)
    rev = numpy.zeros(n, numpy.int64)
    for i in range(bits):
        rev |= ((idx >> i) & 1) << (bits - 1 - i)
    a = a[..., rev]
    size = 2
    while size <= n:
        half = size // 2
        ang = -(2 * _pi(dtype)) * numpy.arange(half).astype(dtype) / numpy.dtype(dtype).type(size)
        w = (numpy.cos(ang) + 1j * numpy.sin(ang)).astype(ct)
        a = a.reshape(a.shape[:-1] + (n // size, size))
        lo, hi = a[..., :half], a[..., half:] * w
        a = numpy.concatenate([lo + hi, lo - hi], axis=-1).reshape(a.shape[:-2] + (n,))
        size *= 2
    return a


# ---- CheapTrick, one frame ------------------------------------------------------------------------------------------------------
def cheaptrick_frame(x, f0_k, t_k, fs, fft_size, q1=-0.15, f0_floor=71.0, seed=0, dtype=numpy.float64, integers=False):
    ft = numpy.dtype(dtype).type
    half = fft_size // 2
    f0, h, centre, L, b, u = frame_integers(f0_k, t_k, fs, fft_size, f0_floor)
    if integers:
        return h, centre, L, b
    pi = _pi(dtype)
    f0d, fsd = ft(f0), ft(fs)
    # 2: the window
    j = numpy.arange(-h, h + 1)
    idx = numpy.clip(centre + j, 0, len(x) - 1)
    win = ft(0.5) * numpy.cos(pi * (j.astype(dtype) / ((ft(1.5) * fsd) / f0d))) + ft(0.5)
    win = win / numpy.sqrt((win * win).sum())
    key = numpy.int64(centre) * numpy.int64(KEY_STRIDE)
    nz = noise(seed, (key + numpy.arange(2 * h + 1, dtype=numpy.int64)).astype(numpy.uint64)).astype(dtype)
    wave = numpy.asarray(x)[idx].astype(dtype) * win + nz * ft(SAFEGUARD)
    wave = wave - win * (wave.sum() / win.sum())
    # 3: power spectrum, DC correction, linear smoothing, floor
    buf = numpy.zeros(fft_size, dtype)
    buf[:2 * h + 1] = wave
    s = fft_any(buf, dtype)[:half + 1]
    pw = (s.real * s.real + s.imag * s.imag).astype(dtype)
    pd = (f0d * fft_size) / fsd
    frac = pd - numpy.floor(pd)
    i = numpy.arange(L + 1)
    lo = pw[L - i]
    hi = pw[numpy.minimum(L - i + 1, half)]
    pw = pw.copy()
    pw[:L + 1] = pw[:L + 1] + (lo + (hi - lo) * frac)
    mirror = numpy.concatenate([pw[b:0:-1], pw, pw[half - 1::-1][:b]])              # b + (half + 1) + b values
    seg = numpy.cumsum(mirror)
    ud = (((f0d * 2) / 3) * fft_size) / fsd
    base = numpy.arange(half + 1).astype(dtype) + ft(b - 0.5)

    def at(pos):
        k = numpy.floor(pos).astype(numpy.int64)
        w = pos - k.astype(dtype)
        return seg[k] + (seg[k + 1] - seg[k]) * w
    sm = (at(base + ud / 2) - at(base - ud / 2)) / ud
    nf = noise(seed, (key + numpy.int64(1024) + numpy.arange(half + 1, dtype=numpy.int64)).astype(numpy.uint64)).astype(dtype)
    sm = sm + numpy.abs(nf) * ft(EPS)
    # 4: smoothing with recovery
    lg = numpy.log(sm)
    cep = fft_any(numpy.concatenate([lg, lg[-2:0:-1]]), dtype).real[:half + 1].astype(dtype)
    q = numpy.arange(1, half + 1).astype(dtype) / fsd
    lifter = numpy.ones(half + 1, dtype)
    lifter[1:] = (numpy.sin(pi * f0d * q) / (pi * f0d * q)) * ((ft(1) - 2 * ft(q1)) + 2 * ft(q1) * numpy.cos(2 * pi * f0d * q))
    c = cep * lifter / fft_size
    out = fft_any(numpy.concatenate([c, c[-2:0:-1]]), dtype).real[:half + 1].astype(dtype)
    return numpy.exp(out)


def cheaptrick(x, f0, temporal_positions, fs, q1=-0.15, f0_floor=71.0, fft_size=None, seed=0, dtype=numpy.float64):
    """-> spectrogram [frames][fft_size / 2 + 1] (power), argument order of `pyworld.cheaptrick`."""
    fft_size = fft_size or cheaptrick_fft_size(fs, f0_floor)
    f0, t = numpy.asarray(f0, numpy.float64).ravel(), numpy.asarray(temporal_positions, numpy.float64).ravel()
    out = numpy.empty((len(f0), fft_size // 2 + 1), dtype)
    for k in range(len(f0)):
        out[k] = cheaptrick_frame(x, f0[k], t[k], fs, fft_size, q1, f0_floor, seed, dtype)
    return out


def integers(f0, temporal_positions, fs, fft_size, f0_floor=71.0):
    """[frames][4]: h, centre sample, DC-correction bin limit L, smoothing boundary b."""
    return numpy.array([frame_integers(a, b, fs, fft_size, f0_floor)[1:5] for a, b in zip(f0, temporal_positions)], numpy.int64).reshape(-1, 4)


# ---- sp2mc ----------------------------------------------------------------------------------------------------------------------------
def freqt(c, order, alpha):
    """SPTK freqt for one frame [MEM: freqt.c]: cepstrum c[0 .. m1] -> order + 1 warped coefficients (same dtype as c)."""
    c = numpy.asarray(c)
    plain = c.dtype == numpy.float64                               # Python floats are IEEE doubles: the same bits, a few times faster
    ft = float if plain else c.dtype.type
    c = [float(v) for v in c] if plain else c
    a = ft(alpha)
    beta = ft(1) - a * a
    g = [ft(0)] * (order + 1)
    for i in range(len(c) - 1, -1, -1):
        d = list(g)
        g[0] = c[i] + a * d[0]
        if order >= 1:
            g[1] = beta * d[0] + a * d[1]
        for j in range(2, order + 1):
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
    return numpy.array(g, dtype=numpy.float64 if plain else ft)


def cepstrum(sp_row, dtype=numpy.float64):
    """irfft(log sp): the fft_size real cepstral values of one frame."""
    lg = numpy.log(numpy.asarray(sp_row).astype(dtype))
    n = 2 * (len(lg) - 1)
    return (fft_any(numpy.concatenate([lg, lg[-2:0:-1]]), dtype).real / n).astype(dtype)


def sp2mc(sp, order, alpha, dtype=numpy.float64, all_values=False):
    """-> mel-cepstrum [frames][order + 1], argument order of `pysptk.sp2mc`.  all_values: hand `freqt` all fft_size values, not the first half + 1."""
    sp = numpy.atleast_2d(sp)
    out = numpy.empty((sp.shape[0], order + 1), dtype)
    for k in range(sp.shape[0]):
        c = cepstrum(sp[k], dtype)
        c[0] = c[0] / 2
        out[k] = freqt(c if all_values else c[:sp.shape[1]], order, alpha)
    return out


def sp2mc_rows(sp, order, alpha, dtype=numpy.float64):
    """`sp2mc` with the frames as the vector axis: per frame the same operations in the same order (the same bits; tests/test_world_analysis_ref.py),
    for the case sets whose recursion in plain Python would take minutes (order 63 over hundreds of rows)."""
    sp = numpy.atleast_2d(sp)
    ft = numpy.dtype(dtype).type
    lg = numpy.log(sp.astype(dtype))
    n = 2 * (sp.shape[1] - 1)
    c = (fft_any(numpy.concatenate([lg, lg[:, -2:0:-1]], axis=1), dtype).real / n).astype(dtype)[:, :sp.shape[1]]
    c[:, 0] = c[:, 0] / 2
    a = ft(alpha)
    beta = ft(1) - a * a
    g = [numpy.zeros(sp.shape[0], dtype) for _ in range(order + 1)]
    for i in range(c.shape[1] - 1, -1, -1):
        d = list(g)
        g[0] = c[:, i] + a * d[0]
        if order >= 1:
            g[1] = beta * d[0] + a * d[1]
        for j in range(2, order + 1):
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
    return numpy.stack(g, axis=1)
