"""The bodies the emulator tests (test_output_gate_cpu.py, test_output_gate_bank_cpu.py) and the GPU tests (test_output_gate_gpu.py) share: each takes
the context it runs on.

MEAN_TOL: max |device mean_db - float64 reference (output_gate_ref.py)| over all of output_gate_cases.CASES was measured with
scripts/output_gate_tolerance.py -- 5.684342e-14 dB on the emulator, 8.526513e-14 dB on the MI355X (profiles/r24/output_gate_tolerance.txt); the
device is held to 16 times the larger of the two (room for FMA contraction and the butterfly order against numpy.fft)."""
import numpy

import output_gate_cases as C
import output_gate_ref as R
from realtime_yukarin_amd.output_gate import OutputGate, OutputGateBank

MEAN_TOL = 16 * 8.526513e-14
SCALE = 0.37


def same_record(got, ref):
    """(emitted, silent, mean_db): flags equal, mean within MEAN_TOL (NaN matches NaN)."""
    if got[0] != ref[0] or got[1] != ref[1]:
        return False
    if numpy.isnan(ref[2]) or numpy.isnan(got[2]):
        return bool(numpy.isnan(ref[2]) and numpy.isnan(got[2]))
    return abs(got[2] - ref[2]) <= MEAN_TOL


def same_chunk(got, ref):
    if got is None or ref is None:
        return got is None and ref is None
    return got.dtype == ref.dtype and got.shape == ref.shape and got.tobytes() == ref.tobytes()


def check_case(ctx, name, n, dtype):
    """One chunk of n samples: mean_db, verdict and the emitted bits against the reference."""
    x = C.signal(name, n)
    gate, ref = OutputGate(n, C.THRESHOLD, SCALE, dtype, ctx=ctx), R.Gate(n, C.THRESHOLD, SCALE, dtype)
    got = gate.push(x)
    want, rec = ref.push(x)
    print('%s N=%d ref %.12f device %.12f diff %.3e' % (name, n, rec[2], gate.last[2], abs(rec[2] - gate.last[2])))
    assert abs(rec[2] + C.THRESHOLD) >= 1.0                          # a condition on the inputs: the verdict has a margin
    assert rec[2] == C.ref_mean(name, n)
    assert same_record(gate.last, rec), (gate.last, rec)
    assert same_chunk(got, want)
    assert gate.held() == 0
    gate.close()


def three_chunks(chunk, extra=137):
    """An audible, a silent and an audible chunk, and a rest."""
    x = numpy.concatenate([C.signal('voiced', chunk), C.signal('noise1e-6', chunk), C.signal('sine', chunk), C.signal('noise1e-4', extra)])
    x.setflags(write=False)
    return x


def run_pieces(gate, x, pieces, drain):
    """push x in `pieces`, then `drain` empty pushes -> the list of (chunk, record) of the pushes that completed a chunk, and held()."""
    out, at = [], 0
    for n in list(pieces) + [0] * drain:
        got = gate.push(x[at:at + n])
        at += n
        if gate.last[0]:
            out.append((got, gate.last))
    assert at == len(x)
    return out, gate.held()


def check_splits(ctx, chunk, seeds):
    """One push of a 3-chunk signal (then empty pushes) against seeded splits of it, pieces of 0 and 1 sample among them: the same chunks, the same
    records, bit for bit, and the reference's."""
    x = three_chunks(chunk)
    ref = R.Gate(chunk, C.THRESHOLD, SCALE)
    want = []
    for piece in [x] + [x[:0]] * 3:
        w, rec = ref.push(piece)
        if rec[0]:
            want.append((w, rec))
    assert [r[1] for _, r in want] == [False, True, False] and len(ref.fragment) == 137
    gate = OutputGate(chunk, C.THRESHOLD, SCALE, ctx=ctx)
    whole, held = run_pieces(gate, x, [len(x)], 3)
    assert held == 137 and len(whole) == 3
    for (g, rec), (w, wrec) in zip(whole, want):
        assert same_record(rec, wrec) and same_chunk(g, w)
    for seed in seeds:
        gate.reset()
        pieces = C.splits(len(x), 5, seed)
        assert 0 in pieces and 1 in pieces
        got, held = run_pieces(gate, x, pieces, 3)
        assert held == 137 and len(got) == 3
        for (g, rec), (w, wrec) in zip(got, whole):
            assert same_chunk(g, w)
            assert rec[:2] == wrec[:2] and numpy.float64(rec[2]).tobytes() == numpy.float64(wrec[2]).tobytes()
    gate.close()


def check_bank(ctx, B, chunk, poison=False):
    """B streams with different signals, cuts of their own, calls they sit out and a reset of stream 1 mid-way, against lone gates that receive the
    same samples: every record and every chunk bit-equal; the launches of a call do not depend on B."""
    names = ('voiced', 'noise1e-6', 'sine', 'click', 'noise1e-4')
    xs = [numpy.concatenate([C.signal(names[(b + j) % 5], chunk) for j in range(3)]) for b in range(B)]
    n_calls = 7
    plans = []
    for b in range(B):
        pieces = C.splits(len(xs[b]), n_calls - 1, 40 + b)
        if b % 2 == 1:
            pieces[2] += pieces[3]                                 # sits call 3 out
            pieces[3] = 0
        plans.append(pieces)
    bank = OutputGateBank(B, chunk, C.THRESHOLD, SCALE, ctx=ctx)
    lone = [OutputGate(chunk, C.THRESHOLD, SCALE, ctx=ctx) for _ in range(B)]
    at = [0] * B
    emitted = 0
    for call in range(n_calls):
        if call == 4 and B > 1:
            bank.reset(1)
            lone[1].reset()
        if poison:
            bank.poison()
        waves = [xs[b][at[b]:at[b] + plans[b][call]] for b in range(B)]
        got = bank.push(waves)
        counts = bank.counts()
        n_done = sum(1 for r in bank.last if r[0])
        n_audible = sum(1 for r in bank.last if r[0] and not r[1])
        if any(len(w) for w in waves):
            assert counts['launches'] == (4 if n_done else 1) and counts['uploads'] == 1, counts
            assert counts['downloads'] == (1 + n_audible if n_done else 0), counts
            assert counts['sample_bytes_down'] == n_audible * chunk * 8, counts
        for b in range(B):
            at[b] += len(waves[b])
            if len(waves[b]) == 0:
                assert got[b] is None and bank.last[b] == (False, False, 0.0)
                continue
            want = lone[b].push(waves[b])
            assert same_chunk(got[b], want), (call, b)
            assert bank.last[b][:2] == lone[b].last[:2], (call, b, bank.last[b], lone[b].last)
            assert numpy.float64(bank.last[b][2]).tobytes() == numpy.float64(lone[b].last[2]).tobytes(), (call, b)
            assert got[b] is None or numpy.isfinite(got[b]).all()
            emitted += bank.last[b][0]
        for b in range(B):
            assert bank.held(b) == lone[b].held()
    assert emitted >= B                                             # chunks were cut
    bank.close()
    for g in lone:
        g.close()


def check_nonfinite(ctx, chunk):
    """NaN samples are scrubbed at append; a chunk with +-inf is not silent, its mean is NaN and it is returned as it is."""
    x = numpy.array(C.signal('voiced', chunk))
    x[[0, 7, chunk // 2, chunk - 1]] = numpy.nan
    gate, ref = OutputGate(chunk, C.THRESHOLD, SCALE, ctx=ctx), R.Gate(chunk, C.THRESHOLD, SCALE)
    got = gate.push(x)
    want, rec = ref.push(x)
    assert want is not None and same_chunk(got, want) and same_record(gate.last, rec) and not numpy.isnan(got).any()
    quiet = numpy.array(C.signal('noise1e-6', chunk))              # silent without the infinite sample
    for pos, v in ((chunk - 1, numpy.inf), (300, -numpy.inf)):
        y = quiet.copy()
        y[pos] = v
        got = gate.push(y)
        want, rec = ref.push(y)
        # the numpy expression: a mean that is not finite and not below anything -- NaN, or +inf where the transform of a frame with one
        # infinite sample comes out all-infinite (the last sample here); the device reports NaN for both, decided from the count
        assert rec[:2] == (True, False) and not numpy.isfinite(rec[2]) and not rec[2] < 0
        assert gate.last[:2] == (True, False) and numpy.isnan(gate.last[2])
        assert same_chunk(got, want) and numpy.isinf(got[pos])
    got = gate.push(quiet)                                          # the count does not stick
    assert got is None and gate.last[:2] == (True, True)
    # an infinite sample behind the chunk counts for the next chunk only
    y = numpy.concatenate([quiet, quiet[:10]])
    y[chunk + 3] = numpy.inf
    assert gate.push(y) is None and gate.last[:2] == (True, True) and gate.held() == 10
    got = gate.push(quiet[:chunk - 10])
    assert got is not None and numpy.isinf(got[3]) and numpy.isnan(gate.last[2])
    gate.close()


def check_poison(ctx, chunk):
    """After ry_outgate_debug_poison every result is unchanged and no sentinel (NaN bit patterns) reaches an output."""
    x = three_chunks(chunk)
    pieces = [chunk // 2, chunk, 3, len(x) - chunk - chunk // 2 - 3]
    clean, dirty = OutputGate(chunk, C.THRESHOLD, SCALE, ctx=ctx), OutputGate(chunk, C.THRESHOLD, SCALE, ctx=ctx)
    at = 0
    for n in pieces + [0, 0]:
        dirty.poison()
        a, b = clean.push(x[at:at + n]), dirty.push(x[at:at + n])
        at += n
        assert same_chunk(a, b) and clean.last[:2] == dirty.last[:2]
        assert numpy.float64(clean.last[2]).tobytes() == numpy.float64(dirty.last[2]).tobytes()
        assert b is None or numpy.isfinite(b).all()
        assert numpy.isfinite(dirty.last[2]) and clean.held() == dirty.held()
    clean.close(); dirty.close()
