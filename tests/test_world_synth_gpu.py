"""WORLD synthesis on the MI355X (realtime_yukarin_amd/world_synth.py) against the numpy float64 restatement (tests/world_synth_ref.py).

Bars.  Pulse indices, voiced flags, output length and every bit identity: exact.  Waveform: max |y - ref| / max |ref| <= 4 x the error of the float64
restatement against the same restatement in longdouble, measured on these inputs by scripts/synth_tolerance.py (profiles/r08/synth_tolerance.txt) --
the kernels run float64 butterflies, so that is the figure they are held to; the project-wide 1e-4 is far above it.  The f0 tracks are vetted by
tests/test_world_synth_ref.py (wrap decisions clear of the threshold, except the prescribed constant-f0 tracks that sit on it by construction)."""
from pathlib import Path

import numpy
import pytest

import world_synth_cases as C
import world_synth_ref as R
from realtime_yukarin_amd import world_synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BAR = 4 * float([l for l in (ROOT / 'profiles' / 'r08' / 'synth_tolerance.txt').read_text().splitlines() if l.startswith('worst float64')][0].split()[-1])


def rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(numpy.abs(a - b).max() / max(numpy.abs(b).max(), 1e-300))


def check(s, f0, sp, ap, fs, seed):
    want, P, _ = R.synthesize(f0, sp, ap, fs, 5.0, seed=seed, return_pulses=True)
    y = s.synthesize(f0, sp, ap)
    idx, shift, voiced = s.pulses()
    assert len(y) == len(want) == int((len(f0) - 1) * 5.0 / 1000 * fs) + 1
    assert numpy.array_equal(idx, numpy.array([p[0] for p in P], numpy.int64)) and list(voiced) == [p[2] for p in P]
    assert numpy.isfinite(y).all()
    if P:
        assert numpy.abs(shift - numpy.array([p[1] for p in P])).max() <= 1e-9
        e = rel(y, want)
        print('fs=%d frames=%d: %d pulses, rel err %.3g (bar %.3g)' % (fs, len(f0), len(P), e, BAR))
        assert e <= BAR, e
    else:
        assert not y.any()
    return y


@pytest.mark.parametrize('n', C.LENGTHS)
@pytest.mark.parametrize('kind', C.TRACKS)
@pytest.mark.parametrize('fs', C.RATES)
def test_tracks_and_lengths(gpu_ctx, fs, kind, n):
    f0, sp, ap = C.case(kind, n, fs)
    s = world_synth.Synthesizer(fs, 5.0, seed=1, ctx=gpu_ctx)
    y = check(s, f0, sp, ap, fs, 1)
    assert numpy.array_equal(s.synthesize(f0, sp, ap), y)                       # two runs: the same bits
    s.close()


@pytest.mark.parametrize('mode', ['floor', 'ceil', 'clamps'])
@pytest.mark.parametrize('fs', C.RATES)
def test_aperiodicity_at_both_clamps(gpu_ctx, fs, mode):
    f0, sp, ap = C.case('glide', 300, fs, mode)
    s = world_synth.Synthesizer(fs, 5.0, seed=1, ctx=gpu_ctx)
    check(s, f0, sp, ap, fs, 1)
    s.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_stage2_output_left_on_the_device(gpu_ctx, fs):
    """sp = an actual stage-2 output (SYN-8 predictor on `synth.stage2_input`) that never leaves the card: the device path equals the host
    path on the downloaded rows bit for bit, and both meet the restatement."""
    from realtime_yukarin_amd import engine, synth
    from realtime_yukarin_amd.weights import flatten_params
    n = 300
    (_, _), (d2, P2) = synth.model_params('SYN-8')
    net = engine.Net(gpu_ctx, d2, flatten_params(d2, P2), width=synth.FFT_BINS - 1)
    x = synth.stage2_input(n)[0]
    px, py = gpu_ctx.dev_alloc(x.size), gpu_ctx.dev_alloc(x.size)
    gpu_ctx.dev_upload(px, x)
    net.convert_device(px, py, 1, n)
    gpu_ctx.sync()
    sp = numpy.empty_like(x)
    gpu_ctx.dev_download(py, sp)
    assert numpy.array_equal(sp, net.convert(x)) and (sp > 0).all()
    f0, _, ap = C.case('glide', n, fs)
    s = world_synth.Synthesizer(fs, 5.0, seed=6, ctx=gpu_ctx)
    host = check(s, f0, sp, ap, fs, 6)
    dev = s.synthesize(f0, world_synth.DeviceRows(py, n), world_synth.to_device(gpu_ctx, ap))
    assert numpy.array_equal(dev, host)
    mixed = s.synthesize(f0, world_synth.DeviceRows(py, n), ap)
    assert numpy.array_equal(mixed, host)
    # the stream takes device rows too (row offsets into the same buffer)
    out = [s.push(f0[a:b], world_synth.DeviceRows(py + 4 * 513 * a, b - a), ap[a:b]) for a, b in ((0, 100), (100, 200), (200, 300))] + [s.flush()]
    assert numpy.array_equal(numpy.concatenate(out), host)
    s.close(); net.close()
    gpu_ctx.dev_free(px); gpu_ctx.dev_free(py)


@pytest.mark.parametrize('fs', C.RATES)
@pytest.mark.parametrize('kind', ['glide', 'unvoiced', 'below'])
def test_stream_equals_one_shot_bit_for_bit(gpu_ctx, fs, kind):
    """100-frame pushes (the reference's buffer), ragged pushes, one-frame pushes."""
    n = 700
    f0, sp, ap = C.case(kind, n, fs)
    s = world_synth.Synthesizer(fs, 5.0, seed=3, ctx=gpu_ctx)
    want = s.synthesize(f0, sp, ap)
    rng = numpy.random.default_rng(5)
    ragged = []
    while sum(ragged) < n:
        ragged.append(min(int(rng.integers(1, 160)), n - sum(ragged)))
    for cuts in ([100] * 7, ragged, [1] * 150 + [550]):
        out, i, lag = [], 0, 0
        for c in cuts:
            out.append(s.push(f0[i:i + c], sp[i:i + c], ap[i:i + c]))
            i += c
            lag = max(lag, s.length(i) - sum(map(len, out)))
        out.append(s.flush())
        assert numpy.array_equal(numpy.concatenate(out), want), cuts[:4]
        assert lag <= s.lag_samples(f0=fs / 1024 + 1) + 1
    s.close()


def test_seeds_differ_only_where_ap_is_above_its_floor(gpu_ctx):
    fs, n = 16000, 300
    f0, sp, ap = C.case('voiced71', n, fs)
    ap[:] = 0.001
    ap[150:, :] = 0.4
    a = world_synth.Synthesizer(fs, 5.0, seed=1, ctx=gpu_ctx)
    b = world_synth.Synthesizer(fs, 5.0, seed=2, ctx=gpu_ctx)
    ya, yb = a.synthesize(f0, sp, ap), b.synthesize(f0, sp, ap)
    cut = 149 * 80 - 1024                                         # samples no pulse of the noisy half reaches
    scale = numpy.abs(ya).max()
    assert numpy.abs(ya[:cut] - yb[:cut]).max() < 2e-3 * scale    # ap at its floor: the noise is 1e-3 of the spectrum's amplitude
    assert numpy.abs(ya[cut + 2048:] - yb[cut + 2048:]).max() > 2e-2 * scale
    assert numpy.array_equal(world_synth.Synthesizer(fs, 5.0, seed=1, ctx=gpu_ctx).synthesize(f0, sp, ap), ya)
    a.close(); b.close()


@pytest.mark.parametrize('fs', C.RATES)
def test_poisoned_buffers(gpu_ctx, fs):
    """Scratch and the unused parts of the frame window pre-filled with NaN bit patterns (the output array: tests/test_world_synth_cpu.py), one-shot
    and stream: nothing unwritten is read, no NaN comes out, the bits are those of the clean run."""
    n = 300
    f0, sp, ap = C.case('glide', n, fs)
    s = world_synth.Synthesizer(fs, 5.0, seed=8, ctx=gpu_ctx)
    clean = check(s, f0, sp, ap, fs, 8)
    big = C.case('unvoiced', 2000, fs)
    s.synthesize(*big)                                            # grow every buffer well beyond what the next calls use
    s.poison()
    y = s.synthesize(f0, sp, ap)
    assert numpy.isfinite(y).all() and numpy.array_equal(y, clean)
    s.poison()
    out = []
    for a, b in ((0, 100), (100, 101), (101, 300)):
        out.append(s.push(f0[a:b], sp[a:b], ap[a:b]))
        s.poison()
    out.append(s.flush())
    y = numpy.concatenate(out)
    assert numpy.isfinite(y).all() and numpy.array_equal(y, clean)
    s.close()
