"""WORLD `Synthesis` restated in numpy (the version with fractional pulse time shifts), the yardstick of `realtime_yukarin_amd.world_synth`.

Neither `pyworld` nor `world4py` can be imported here and the reference tree holds no WORLD source, so -- as for the CNNs and `mc2sp` --
this is a restatement of the published algorithm ([MEM]); parity at the `pyworld` boundary is unpinned.  What it fixes:

* `y_length = int((N - 1) * frame_period / 1000 * fs) + 1`, `fft_size = cheaptrick_fft_size(fs)`.
* Time base (float64): f0 below `fs / fft_size + 1` is unvoiced (0); f0 and the voiced flag are interpolated linearly to the sample grid
  (sample n sits at frame position n / (fs * frame_period / 1000); WORLD's extrapolated frame behind the last only ever gets weight 0, so
  positions at or behind the last frame take the last frame); flag > 0.5 = voiced; unvoiced samples get 500 Hz.
* Pulses (float64): the phase advances by 2 pi f0[n] / fs per sample and is WRAPPED AT EVERY STEP (`if phase >= 2 pi: phase -= 2 pi`); a
  pulse sits at the sample before every wrap, its fractional shift comes from the linear interpolation of the wrapped phase across the wrap.
  WORLD sums the phase first and takes `fmod` afterwards; wrapping per step is the same mathematics, keeps the phase small (so its rounding
  does not grow with the length of the signal) and is what a stream can carry from one push to the next.
* Per pulse: spectrum and squared, clamped (0.001 .. 1 - 1e-12) aperiodicity interpolated between the two neighbouring frames at the pulse
  time; periodic response = minimum phase of sp (1 - ap^2) + 1e-12, fractional shift, inverse FFT, fftshift, raised-cosine DC removal (zero
  when unvoiced or ap^2[0] > 0.999); aperiodic response = minimum phase of sp ap^2 (sp alone when unvoiced) times the spectrum of
  min(noise_size, fft_size) mean-removed noise samples, noise_size = distance to the next pulse (0 for the last pulse: no response);
  response = (periodic sqrt(noise_size) + aperiodic) / fft_size, added at index - fft_size / 2 + 1.
* Noise is COUNTER-BASED, not WORLD's sequential xorshift: sample k of the stream's noise is a pure function of (seed, k) -- the sum of twelve
  24-bit uniforms minus six, the uniforms from a 32-bit integer hash -- and pulse p uses samples index_p .. index_p + noise_size - 1.  A stated
  deviation from `pyworld` (whose output depends on process-global generator state): reproducible, parallel, independent of how a stream is cut.
* Overlap-add: every output sample is the sum of its pulses' contributions in ascending pulse order.

`dtype` selects the arithmetic of the per-pulse stage (float64: the yardstick; longdouble / float32: the tolerance measurements); the time base
and the pulses are always float64.  `Stream` is the same arithmetic fed in pushes."""
import numpy

TWO_PI = 2.0 * numpy.pi
DEFAULT_F0 = 500.0
SAFEGUARD = 1e-12
AP_LO, AP_HI = 0.001, 0.999999999999


def cheaptrick_fft_size(fs, f0_floor=71.0):
    return int(2 ** (1 + int(numpy.log2(3.0 * fs / f0_floor + 1))))


def y_length(n_frames, fs, frame_period):
    return int((n_frames - 1) * frame_period / 1000 * fs) + 1


# ---- counter-based noise ------------------------------------------------------------------------------------------------------
def hash32(x):
    """lowbias32 (public domain integer hash) on uint64 arrays holding 32-bit values."""
    m = numpy.uint64(0xffffffff)
    x = x & m
    x ^= x >> numpy.uint64(16)
    x = (x * numpy.uint64(0x7feb352d)) & m
    x ^= x >> numpy.uint64(15)
    x = (x * numpy.uint64(0x846ca68b)) & m
    x ^= x >> numpy.uint64(16)
    return x


def noise(seed, k):
    """Samples k (array of absolute sample positions) of the noise of `seed`: float64, exact multiples of 2^-24 in [-6, 6)."""
    k = numpy.asarray(k, dtype=numpy.uint64)
    m = numpy.uint64(0xffffffff)
    hs = hash32(numpy.asarray([seed], dtype=numpy.uint64) & m)
    total = numpy.zeros(k.shape, numpy.uint64)
    for j in range(12):
        key = k * numpy.uint64(12) + numpy.uint64(j)
        h = hash32((key & m) ^ hash32((key >> numpy.uint64(32)) ^ hs))
        total += h >> numpy.uint64(8)
    return total.astype(numpy.float64) * 2.0 ** -24 - 6.0


# ---- time base and pulses (float64) ----------------------------------------------------------------------------------------------
def coarse_f0(f0, fs, fft_size):
    f0 = numpy.asarray(f0, dtype=numpy.float64).ravel()
    return numpy.where(f0 < fs / fft_size + 1.0, 0.0, f0)


def sample_f0(cf0, n0, n1, fs, frame_period, last_frame):
    """(f0, voiced) of samples n0 .. n1 - 1.  cf0: thresholded f0 of frames 0 .. ; positions at or behind `last_frame` take that frame."""
    spf = fs * frame_period / 1000
    pos = numpy.arange(n0, n1, dtype=numpy.float64) / spf
    k = numpy.floor(pos).astype(numpy.int64)
    w = pos - k
    clamp = k >= last_frame
    k0 = numpy.where(clamp, last_frame, k)
    k1 = numpy.where(clamp, last_frame, k + 1)
    w = numpy.where(clamp, 0.0, w)
    v = (cf0 != 0.0).astype(numpy.float64)
    f = cf0[k0] + (cf0[k1] - cf0[k0]) * w
    vi = v[k0] + (v[k1] - v[k0]) * w
    voiced = vi > 0.5
    return numpy.where(voiced, f, DEFAULT_F0), voiced


class PulseScan(object):
    """The sequential part: carries the wrapped phase and the voiced flag of the last sample."""

    def __init__(self, fs):
        self.fs = float(fs)
        self.phase = 0.0
        self.last_voiced = False
        self.n = 0                       # samples seen
        self.min_margin = numpy.inf      # how close the phase came to the wrap threshold (tests: inputs must stay clear of it)

    def feed(self, f0, voiced):
        """-> (index, shift in samples, voiced) of the pulses found in these samples."""
        out = []
        ph, fs = self.phase, self.fs
        d = TWO_PI * numpy.asarray(f0, dtype=numpy.float64) / fs
        for i in range(len(d)):
            new = ph + d[i]
            self.min_margin = min(self.min_margin, abs(new - TWO_PI))
            if new >= TWO_PI:
                y1 = ph - TWO_PI
                y2 = new - TWO_PI
                out.append((self.n + i - 1, -y1 / (y2 - y1), bool(voiced[i - 1]) if i > 0 else self.last_voiced))
                new = y2
            ph = new
        if len(d):
            self.last_voiced = bool(voiced[-1])
        self.phase = ph
        self.n += len(d)
        return out


# ---- one pulse -------------------------------------------------------------------------------------------------------------------
def dc_remover(fft_size, dtype=numpy.float64):
    i = numpy.arange(fft_size // 2, dtype=dtype)
    half = 0.5 - 0.5 * numpy.cos(2 * numpy.pi * (i + 1) / (1 + fft_size))
    r = numpy.concatenate([half, half[::-1]])
    return (r / (2 * half.sum())).astype(dtype)


def minimum_phase(log_half, fft_size):
    """log_half: log(spectrum) / 2 on bins 0 .. fft_size / 2 -> minimum-phase spectrum on the same bins (cepstrum folded, exp)."""
    full = numpy.concatenate([log_half, log_half[-2:0:-1]])
    cep = numpy.fft.fft(full)
    cep[1:fft_size // 2 + 1] *= 2
    cep[fft_size // 2 + 1:] = 0
    s = numpy.fft.fft(cep)[:fft_size // 2 + 1]
    return numpy.exp(s.real / fft_size) * (numpy.cos(s.imag / fft_size) + 1j * numpy.sin(s.imag / fft_size))


def frame_weights(index, fs, frame_period, last_frame):
    pos = index / (fs * frame_period / 1000)
    k0 = min(last_frame, int(numpy.floor(pos)))
    k1 = min(last_frame, int(numpy.ceil(pos)))
    return k0, k1, pos - k0


def pulse_response(index, shift, voiced, noise_size, sp, ap, frame0, last_frame, fs, frame_period, fft_size, seed, dtype=numpy.float64, parts=False):
    """sp / ap: rows of frames frame0 .. (float32 or float64 as given).  -> response [fft_size] (dtype)."""
    ft = numpy.dtype(dtype).type
    if noise_size <= 0:
        z = numpy.zeros(fft_size, dtype)
        return (z, z) if parts else z
    k0, k1, w = frame_weights(index, fs, frame_period, last_frame)
    w = ft(w)
    s0, a0 = numpy.abs(sp[k0 - frame0].astype(dtype)), numpy.clip(ap[k0 - frame0].astype(dtype), ft(AP_LO), ft(AP_HI)) ** 2
    if k0 == k1:
        s, a = s0, a0
    else:
        s = (1 - w) * s0 + w * numpy.abs(sp[k1 - frame0].astype(dtype))
        a = (1 - w) * a0 + w * numpy.clip(ap[k1 - frame0].astype(dtype), ft(AP_LO), ft(AP_HI)) ** 2
    half = fft_size // 2
    if voiced and not a[0] > 0.999:
        m = minimum_phase(numpy.log(s * (1 - a) + ft(SAFEGUARD)) / 2, fft_size)
        ang = (ft(TWO_PI) * ft(shift) / fft_size) * numpy.arange(half + 1, dtype=dtype)
        m = m * (numpy.cos(ang) - 1j * numpy.sin(ang))
        p = numpy.fft.fftshift(numpy.fft.irfft(m, fft_size) * fft_size)
        dc = p[half:].sum()
        p[:half] = 0
        periodic = p - dc * dc_remover(fft_size, dtype)
    else:
        periodic = numpy.zeros(fft_size, dtype)
    ns = min(noise_size, fft_size)
    wv = numpy.zeros(fft_size, dtype)
    g = noise(seed, index + numpy.arange(ns)).astype(dtype)
    wv[:ns] = g - g.sum() / ns
    m = minimum_phase(numpy.log(s * a if voiced else s) / 2, fft_size)
    aperiodic = numpy.fft.fftshift(numpy.fft.irfft(m * numpy.fft.rfft(wv), fft_size) * fft_size)
    if parts:
        return (periodic * numpy.sqrt(ft(noise_size)) / fft_size).astype(dtype), (aperiodic / fft_size).astype(dtype)
    return ((periodic * numpy.sqrt(ft(noise_size)) + aperiodic) / fft_size).astype(dtype)


# ---- whole signal / stream -------------------------------------------------------------------------------------------------------
class Stream(object):
    """push(f0, sp, ap) -> the samples that can no longer change; flush() -> the rest.  Concatenated = `synthesize` bit for bit."""

    def __init__(self, fs, frame_period=5.0, seed=0, fft_size=None, dtype=numpy.float64):
        self.fs, self.frame_period, self.seed, self.dtype = int(fs), float(frame_period), int(seed), dtype
        self.fft_size = fft_size or cheaptrick_fft_size(fs)
        self.reset()

    def reset(self):
        self.cf0 = numpy.zeros(0)
        self.sp = self.ap = None
        self.scan = PulseScan(self.fs)
        self.pulses = []                 # every pulse so far (index, shift, voiced)
        self.first_live = 0              # pulses before this one cannot reach an unemitted sample
        self.done = 0                    # samples emitted
        self.responses = {}

    def push(self, f0, sp, ap):
        sp, ap = numpy.atleast_2d(sp), numpy.atleast_2d(ap)
        self.cf0 = numpy.concatenate([self.cf0, coarse_f0(f0, self.fs, self.fft_size)])
        self.sp = sp if self.sp is None else numpy.concatenate([self.sp, sp])
        self.ap = ap if self.ap is None else numpy.concatenate([self.ap, ap])
        return self._advance(False)

    def flush(self):
        y = self._advance(True)
        self.reset()
        return y

    def _known(self, final):
        m = len(self.cf0)
        if final:
            return y_length(m, self.fs, self.frame_period)
        spf = self.fs * self.frame_period / 1000
        n = max(int(numpy.ceil((m - 1) * spf)), 0)
        while n > 0 and not (n - 1) / spf < m - 1:
            n -= 1
        while n / spf < m - 1:
            n += 1
        return n                         # every sample n' < n has n' / spf < m - 1: both its frames are here

    def _advance(self, final):
        m, half = len(self.cf0), self.fft_size // 2
        k1 = max(self._known(final), self.scan.n)
        f, v = sample_f0(self.cf0, self.scan.n, k1, self.fs, self.frame_period, m - 1)
        self.pulses += self.scan.feed(f, v)
        P = self.pulses
        complete = len(P) if final else len(P) - 1
        fin = k1 if final else (max(self.done, P[-1][0] - half + 1) if P else self.done)
        fin = min(fin, k1)
        y = numpy.zeros(fin - self.done, self.dtype)
        while self.first_live < len(P) - 1 and P[self.first_live][0] < self.done - half:
            self.responses.pop(self.first_live, None)
            self.first_live += 1
        for j in range(self.first_live, max(complete, self.first_live)):
            idx, shift, voiced = P[j]
            if idx - half + 1 >= fin:
                break
            if j not in self.responses:
                ns = P[j + 1][0] - idx if j + 1 < len(P) else 0
                self.responses[j] = pulse_response(idx, shift, voiced, ns, self.sp, self.ap, 0, m - 1, self.fs, self.frame_period,
                                                   self.fft_size, self.seed, self.dtype)
            off = idx - half + 1
            lo, hi = max(self.done, off), min(fin, off + self.fft_size)
            if hi > lo:
                y[lo - self.done:hi - self.done] += self.responses[j][lo - off:hi - off]
        self.done = fin
        return y


def synthesize(f0, sp, ap, fs, frame_period=5.0, seed=0, fft_size=None, dtype=numpy.float64, return_pulses=False):
    s = Stream(fs, frame_period, seed, fft_size, dtype)
    s.cf0 = coarse_f0(f0, s.fs, s.fft_size)
    s.sp, s.ap = numpy.atleast_2d(sp), numpy.atleast_2d(ap)
    y = s._advance(True)
    if return_pulses:
        return y, list(s.pulses), s.scan.min_margin
    return y


def lag_samples(fs, frame_period=5.0, fft_size=None, f0=DEFAULT_F0):
    """What `push` holds back at most, in samples: half a transform, one frame, one pulse period (of `f0`)."""
    fft_size = fft_size or cheaptrick_fft_size(fs)
    return fft_size // 2 + int(numpy.ceil(fs * frame_period / 1000)) + int(numpy.ceil(fs / f0))
