"""What the stream-bank tests share (tests/test_synth_bank_cpu.py on the emulator, tests/test_synth_bank_gpu.py on the MI355X): a rig of one
`StreamBank` and one lone yardstick `Synthesizer` per stream -- same rate, frame period and seed, on the same context -- and the comparison after
EVERY call: `numpy.array_equal` on the samples and on the pulse index / shift / voiced lists, per stream.  When a signal ends, the concatenation
of what its stream returned is compared with `synthesize` on the concatenated frames.  No tolerance anywhere.  Inputs: tests/world_synth_cases.py;
the edge cases are planned with the float64 restatement (tests/world_synth_ref.py), never with the code under test."""
import functools

import numpy

import world_synth_cases as C
import world_synth_ref as R
from realtime_yukarin_amd import world_synth

ROW = C.BINS * 4
EMPTY = numpy.empty(0, numpy.float64)


class Rig(object):
    def __init__(self, ctx, fs, seeds, frame_period=5.0):
        self.ctx, self.fs, self.seeds, self.B = ctx, fs, list(seeds), len(seeds)
        self.bank = world_synth.StreamBank(fs, frame_period, n_streams=self.B, seeds=self.seeds, ctx=ctx)
        self.lone = [world_synth.Synthesizer(fs, frame_period, seed=s, ctx=ctx) for s in self.seeds]
        self.frames = [[] for _ in range(self.B)]             # of the signal in progress, per stream
        self.out = [[] for _ in range(self.B)]
        self.ended = 0

    def close(self):
        self.bank.close()
        for s in self.lone:
            s.close()

    def _want(self, b, item, final):
        """What the lone handle of stream b gives for this call: (samples, index, shift, voiced)."""
        ys, ps = [], []
        if item is not None and len(item[0]):
            ys.append(self.lone[b].push(*item))
            ps.append(self.lone[b].pulses())
            self.frames[b].append(item)
        if final:
            ys.append(self.lone[b].flush())
            ps.append(self.lone[b].pulses())
        if not ys:
            return EMPTY, numpy.empty(0, numpy.int64), EMPTY, numpy.empty(0, bool)
        return (numpy.concatenate(ys),) + tuple(numpy.concatenate([p[i] for p in ps]) for i in range(3))

    def push(self, items, final=(), send=None):
        """One bank call on `items` (host rows; `send`: the same frames in the form the bank gets them, e.g. device rows) against the lone
        handles; -> the bank's arrays."""
        got = self.bank.push(items if send is None else send, final)
        assert len(got) == self.B
        for b in range(self.B):
            want = self._want(b, items[b], b in final)
            assert got[b].dtype == numpy.float64 and numpy.array_equal(got[b], want[0]), 'stream %d: samples differ' % b
            idx, shift, voiced = self.bank.pulses(b)
            assert numpy.array_equal(idx, want[1]) and numpy.array_equal(shift, want[2]) and numpy.array_equal(voiced, want[3]), 'stream %d: pulses differ' % b
            self.out[b].append(got[b])
            if b in final:
                self._end(b)
        return got

    def _end(self, b):
        """The signal of stream b is over: the concatenation equals the one-shot call on its frames."""
        f0, sp, ap = (numpy.concatenate([it[i] for it in self.frames[b]]) for i in range(3))
        whole = self.lone[b].synthesize(f0, sp, ap)
        assert numpy.array_equal(numpy.concatenate(self.out[b]), whole), 'stream %d: concatenation differs from synthesize' % b
        self.frames[b], self.out[b] = [], []
        self.ended += 1

    def flush_all(self):
        live = [b for b in range(self.B) if self.frames[b]]
        return self.push([None] * self.B, final=live)


def cut(item, cuts):
    """(f0, sp, ap) -> its pieces of cuts[0], cuts[1], ... frames (0: None)."""
    out, r = [], 0
    for n in cuts:
        out.append(None if n == 0 else tuple(a[r:r + n] for a in item))
        r += n
    assert r <= len(item[0])
    return out


def run_cuts(rig, kinds, cuts, final_at=None, order=None):
    """Stream b gets a `kinds[b]` track in pieces cuts[b][call]; every call is checked; then everything is flushed."""
    order = list(range(rig.B)) if order is None else list(order)
    pieces = [None] * rig.B
    for slot, b in enumerate(order):
        pieces[slot] = cut(C.case(kinds[b], sum(cuts[b]), rig.fs), cuts[b])
    outs = []
    for call in range(len(cuts[0])):
        outs.append(rig.push([p[call] for p in pieces]))
    outs.append(rig.flush_all())
    return outs


def loud(n):
    """A neighbour that would show in anything that read across a stream boundary: sp constant 1e30, ap beyond both clamps."""
    return numpy.zeros(n) + 150.0, numpy.full((n, C.BINS), 1e30, numpy.float32), C.aperiodicity(n, mode='clamps')


def device_slices(ctx, items):
    """The items' sp / ap (None: no rows) as consecutive slices of ONE device buffer each -> the list in device form."""
    have = [it for it in items if it is not None]
    sp = world_synth.to_device(ctx, numpy.concatenate([it[1] for it in have]))
    ap = world_synth.to_device(ctx, numpy.concatenate([it[2] for it in have]))
    out, r = [], 0
    for it in items:
        if it is None:
            out.append(None)
            continue
        n = len(it[0])
        out.append((it[0], world_synth.DeviceRows(sp.address + r * ROW, n, keep=sp), world_synth.DeviceRows(ap.address + r * ROW, n, keep=ap)))
        r += n
    return out


# ---- edges, planned with the restatement -------------------------------------------------------------------------------------------
def known_samples(m, spf):
    """Samples whose two neighbouring frames are among the first m (tests/world_synth_ref.py, Stream._known)."""
    if m < 2:
        return 0
    n = max(int(numpy.ceil((m - 1) * spf)), 0)
    while n > 0 and not (n - 1) / spf < m - 1:
        n -= 1
    while n / spf < m - 1:
        n += 1
    return n


TARGETS = tuple(k + d for k in (256, 1024) for d in (-1, 0, 1))


@functools.lru_cache(maxsize=None)
def scanned_edge(fs, target):
    """(frame period in ms, frames) after which `scanned` = known_samples is exactly `target`: whole samples per frame, the fewest frames."""
    best = None
    for spf in range(40, 261):
        for m in range(2, 40):
            fp = 1000.0 * spf / fs
            if known_samples(m, fs * fp / 1000) == target and (best is None or m < best[1]):
                best = (fp, m)
    assert best is not None and known_samples(best[1], fs * best[0] / 1000) == target, target
    return best


@functools.lru_cache(maxsize=None)
def done_edge(fs, target):
    """(constant voiced f0, frames) after whose first push `done` = last pulse - 511 is exactly `target`, at 5 ms frames: the pulse scan of the
    restatement on candidate tracks, decisions at least 1e-9 away from the wrap threshold."""
    spf = fs * 5.0 / 1000
    for period in numpy.arange(40.137, 140.0, 0.37):           # samples per pulse: off the sample grid
        f0 = fs / period
        for m in range(int((target + 512) / spf) + 2, int((target + 512) / spf) + 5):
            k1 = known_samples(m, spf)
            cf0 = R.coarse_f0(numpy.full(m, f0), fs, 1024)
            scan = R.PulseScan(fs)
            f, v = R.sample_f0(cf0, 0, k1, fs, 5.0, m - 1)
            pulses = scan.feed(f, v)
            if pulses and scan.min_margin > 1e-9 and min(max(0, pulses[-1][0] - 511), k1) == target:
                return float(f0), m
    raise AssertionError('no track puts done on %d' % target)


def check_scanned_edge(ctx, fs, target, more=7):
    fp, m = scanned_edge(fs, target)
    rig = Rig(ctx, fs, [3, 4], frame_period=fp)
    try:
        a, b = C.case('glide', m + more, fs), C.case('above', 9, fs)
        rig.push([tuple(x[:m] for x in a), tuple(x[:4] for x in b)])
        assert rig.bank.bound(0, 0, True) > 0 and known_samples(m, fs * fp / 1000) == target
        rig.push([tuple(x[m:] for x in a), tuple(x[4:] for x in b)])          # this call's scan starts on the edge
        rig.flush_all()
        assert rig.ended == 2
    finally:
        rig.close()


def check_done_edge(ctx, fs, target, more=7):
    f0, m = done_edge(fs, target)
    rig = Rig(ctx, fs, [3, 4])
    try:
        _, sp, ap = C.case('glide', m + more, fs)
        a, b = (numpy.full(m + more, f0), sp, ap), C.case('glide', 9, fs)
        got = rig.push([tuple(x[:m] for x in a), tuple(x[:4] for x in b)])
        assert len(got[0]) == target                                          # `done` sits on the edge when the next call starts
        rig.push([tuple(x[m:] for x in a), tuple(x[4:] for x in b)])
        rig.flush_all()
        assert rig.ended == 2
    finally:
        rig.close()


# ---- the cases both suites run -----------------------------------------------------------------------------------------------------
def check_one_stream(ctx, fs):
    rig = Rig(ctx, fs, [5])
    try:
        outs = run_cuts(rig, ['glide'], [[1, 1, 2, 5, 31]])
        assert len(outs[0][0]) == 0 and rig.ended == 1
    finally:
        rig.close()


RAGGED = [[13, 13, 14], [0, 40, 0], [1, 2, 37]]


def check_ragged(ctx, fs):
    for order in (None, [2, 1, 0]):
        rig = Rig(ctx, fs, [5, 6, 7])
        try:
            run_cuts(rig, ['glide', 'above', 'glide'], RAGGED, order=order)
            assert rig.ended == 3
        finally:
            rig.close()


def check_kinds(ctx, fs, n):
    rig = Rig(ctx, fs, list(range(len(C.TRACKS))))
    try:
        run_cuts(rig, list(C.TRACKS), [[n, n]] * len(C.TRACKS))
        assert rig.ended == len(C.TRACKS)
    finally:
        rig.close()


def check_end_and_restart(ctx, fs):
    rig = Rig(ctx, fs, [5, 6, 7])
    try:
        a, b, c = (cut(C.case(k, 30, fs), [9, 11, 10]) for k in ('glide', 'above', 'glide'))
        rig.push([a[0], b[0], c[0]])
        rig.push([a[1], b[1], c[1]], final=[1])                    # stream 1 ends with these frames, 0 and 2 go on
        assert rig.ended == 1 and rig.bank.bound(1, 0, True) == 0
        fresh = world_synth.Synthesizer(fs, 5.0, seed=6, ctx=ctx)  # slot 1 starts a new signal: a fresh lone handle gives the same
        new = C.case('below', 12, fs)
        got = rig.push([a[2], new, c[2]])
        want = fresh.push(*new)
        fresh.close()
        assert numpy.array_equal(got[1], want)
        rig.push([None, None, None], final=[0])                    # final with no frames: a plain flush
        assert rig.ended == 2
        rig.flush_all()
        assert rig.ended == 4
    finally:
        rig.close()


def check_loud_neighbour(ctx, fs):
    rig = Rig(ctx, fs, [5, 6, 7])
    try:
        a, c = cut(C.case('glide', 20, fs), [9, 11]), cut(C.case('above', 20, fs), [12, 8])
        l = cut(loud(20), [7, 13])
        for call in range(2):
            got = rig.push([a[call], l[call], c[call]])
            assert numpy.isfinite(got[0]).all() and numpy.isfinite(got[2]).all()
        rig.flush_all()
    finally:
        rig.close()


def check_seeds(ctx, fs):
    it = C.case('below', 30, fs)                                   # frames 20 .. 29 are unvoiced
    pieces = cut(it, [14, 16])
    for seeds, same in (([9, 9], True), ([9, 10], False)):
        rig = Rig(ctx, fs, seeds)
        try:
            outs = [rig.push([p, p]) for p in pieces] + [rig.flush_all()]
            y = [numpy.concatenate([o[b] for o in outs]) for b in range(2)]
            assert numpy.array_equal(y[0], y[1]) == same
            lo = int(22 * rig.bank.fs * 5.0 / 1000)
            assert same or (y[0][lo:lo + 400] != y[1][lo:lo + 400]).any()
        finally:
            rig.close()


def check_poison(ctx, fs):
    rig = Rig(ctx, fs, [5, 6])
    try:
        a, b = cut(C.case('glide', 30, fs), [9, 11, 10]), cut(C.case('voiced71', 30, fs), [12, 0, 18])
        for call in range(3):
            rig.push([a[call], b[call]])
            rig.bank.poison()
        rig.flush_all()
        assert rig.ended == 2
    finally:
        rig.close()


def check_device_rows(ctx, fs):
    rig = Rig(ctx, fs, [5, 6, 7])
    try:
        a, b, c = cut(C.case('glide', 20, fs), [9, 5, 6]), cut(C.case('above', 20, fs), [4, 0, 16]), cut(C.case('glide', 20, fs), [1, 12, 7])
        calls = world_synth.calls
        # consecutive slices of one buffer, a stream that sits out contributing no rows: read in place, one call
        for call in range(2):
            items = [a[call], b[call], c[call]]
            before = dict(calls)
            rig.push(items, send=device_slices(ctx, items))
            assert calls == dict(before, bank_in_place=before['bank_in_place'] + 1)
        items = [a[2], b[2], c[2]]
        sl = device_slices(ctx, items)
        before = dict(calls)
        rig.push(items, send=[sl[0], items[1], sl[2]])             # host and device rows in one list: item by item
        assert calls == dict(before, bank_fallback=before['bank_fallback'] + 1)
        more = [tuple(x[:5] for x in C.case('below', 5, fs)) for _ in range(3)]
        sl = device_slices(ctx, [more[2], more[1], more[0]])
        before = dict(calls)
        rig.push(more, send=[sl[2], sl[1], sl[0]])                 # device rows that do not follow one another
        assert calls == dict(before, bank_fallback=before['bank_fallback'] + 1)
        before = dict(calls)
        rig.push(more)                                             # host rows: one packed upload
        assert calls == dict(before, bank_packed=before['bank_packed'] + 1)
        rig.flush_all()
        assert rig.ended == 3
    finally:
        rig.close()


def steady_counts(ctx, fs, B):
    """`counts()` of the fifth of five equal pushes of 13 frames on every stream: no buffer grows any more."""
    bank = world_synth.StreamBank(fs, 5.0, n_streams=B, seeds=list(range(B)), ctx=ctx)
    try:
        pieces = cut(C.case('unvoiced', 65, fs), [13] * 5)
        for p in pieces:
            bank.push([p] * B)
        return bank.counts()
    finally:
        bank.close()


def check_cost(ctx, fs, big=8):
    one, many = steady_counts(ctx, fs, 1), steady_counts(ctx, fs, big)
    assert one == many, (one, many)
    assert one['waits'] <= 2 and one['launches'] == 5, one


def check_window_age(ctx, fs, kind='unvoiced'):
    bank = world_synth.StreamBank(fs, 5.0, n_streams=1, seeds=[1], ctx=ctx)
    try:
        rows = []
        for p in cut(C.case(kind, 260, fs), [13] * 20):
            bank.push([p])
            rows.append(bank.rows(0))
        assert max(rows[9:20]) <= max(rows[1:9]), rows
    finally:
        bank.close()
