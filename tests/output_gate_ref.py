"""The output gate restated in float64 numpy (the reference's worker/decode_worker.py:53-61, run.py:194-198, stream/decode_stream.py:38 and the
librosa defaults of the version it uses): explicit framing after `numpy.pad(..., mode='reflect')`, `numpy.fft.rfft`, the dB / clamp / mean lines,
and the fragment / chunk bookkeeping.  librosa is not imported; it stores the STFT as complex64, `mean_db(..., complex64=True)` restates that."""
import numpy

N_FFT = 2048
HOP = 512


def window():
    n = numpy.arange(N_FFT, dtype=numpy.float64)
    return 0.5 - 0.5 * numpy.cos(2.0 * numpy.pi * n / N_FFT)


def stft(wave, complex64=False):
    """-> [1025][1 + len // 512] like librosa.stft(wave) with its defaults."""
    wave = numpy.asarray(wave, numpy.float64)
    y = numpy.pad(wave, N_FFT // 2, mode='reflect')
    n_frames = 1 + len(wave) // HOP
    w = window()
    out = numpy.empty((N_FFT // 2 + 1, n_frames), numpy.complex64 if complex64 else numpy.complex128)
    for f in range(n_frames):
        out[:, f] = numpy.fft.rfft(y[f * HOP:f * HOP + N_FFT] * w)
    return out


def mean_db(wave, complex64=False):
    """librosa.core.power_to_db(numpy.abs(librosa.stft(wave)) ** 2).mean(): ref 1.0, amin 1e-10, top_db 80."""
    with numpy.errstate(all='ignore'):
        power = numpy.abs(stft(wave, complex64)) ** 2
        db = 10.0 * numpy.log10(numpy.maximum(1e-10, power))
        db = numpy.maximum(db, db.max() - 80.0)
        return float(db.mean())


class Gate(object):
    """decode_worker.py:53-61 with DecodeStream's NaN scrub in front and run.py's scale / cast behind.  push -> (chunk or None, record) where
    record = (emitted, silent, mean_db); the chunk of a silent record is None."""

    def __init__(self, chunk, threshold_db, scale=1.0, dtype=numpy.float64):
        self.chunk, self.threshold_db, self.scale, self.dtype = chunk, threshold_db, scale, dtype
        self.fragment = numpy.empty(0)

    def push(self, wave):
        wave = numpy.array(wave, numpy.float64)
        wave[numpy.isnan(wave)] = 0
        self.fragment = numpy.concatenate([self.fragment, wave])
        if len(self.fragment) >= self.chunk:
            wave, self.fragment = self.fragment[:self.chunk], self.fragment[self.chunk:]
            power = mean_db(wave)
            if power < -self.threshold_db:
                return None, (True, True, power)
            return (wave * self.scale).astype(self.dtype), (True, False, power)
        return None, (False, False, 0.0)
