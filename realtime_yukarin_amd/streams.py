"""The store in the middle of the reference's three-stream live loop (run.py: `EncodeStream` -> `ConvertStream` -> `DecodeStream`), in this
project's form: the stream arithmetic as TABLES, and the feature segments as device rows.

`BaseStream.fetch` (stream/base_stream.py) walks the stored segments, pads where no data exists and concatenates what `pick` returns.  Which
row is taken is decided by float clocks -- `round((t - s.start_time) * rate)`, a running `start_time_buffer` and `remaining_time` -- so
`fetch_plan` restates that arithmetic operation for operation in Python floats and returns the spans alone:

    (segment_index, first, last)        `pick(segment.data, first, last)`: the arguments as the reference passes them, not yet clipped
    (-1, 0, width)                      `pad(width)`

`row_spans` clips a plan as numpy slicing clips (`AcousticFeature.pick`), `wave_spans` turns it into the sample spans of `pick_wrapper` /
`silent_wrapper` (`round(first * frame_period / 1000 * fs)`), and `retire` says how many of the oldest segments no later window can fetch
(`worker.retire_time`).  `RowStore` is the handle over `ry_rowstore_*` (include/ry355.h): three rings on the card the plans are applied to
without a feature row crossing the bus.  INTEGRATION.md section 23, DESIGN.md section 25."""
import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy

from . import _lib
from ._handle import DeviceHandle
from .worker import retire_time

PAD = -1
_IP = ctypes.POINTER(ctypes.c_int)


def fetch_plan(segments: Sequence[Tuple[float, int]], start_time: float, time_length: float, extra_time: float, rate) -> List[Tuple[int, int, int]]:
    """The spans `BaseStream.fetch(start_time, time_length, extra_time)` concatenates over `segments`: (start_time, length) pairs in arrival
    order, `rate` the segment method's sampling rate.  Spans with first == last occur (a segment that ends where the window starts) and are
    kept: they are part of what the reference does."""
    begin = start_time - extra_time
    length = time_length + extra_time * 2
    end = begin + length
    clock, remaining = begin, length
    plan = []
    for index, (seg_start, seg_length) in enumerate(segments):
        seg_end = seg_length / rate + seg_start
        if end < seg_start or seg_end < begin:
            continue
        if seg_start > clock:
            plan.append((PAD, 0, round((seg_start - clock) * rate)))
            remaining -= seg_start - clock
            clock = seg_start
        if remaining > seg_end - clock:
            taken = seg_end - clock
        else:
            taken = remaining
        first = round((clock - seg_start) * rate)
        last = round(first + taken * rate)
        plan.append((index, first, last))
        clock += taken
        remaining -= taken
        if clock >= end:
            return plan
    plan.append((PAD, 0, round((end - clock) * rate)))
    return plan


def _clip(first: int, last: int, n: int) -> Tuple[int, int]:
    """[first:last] of n elements as numpy slicing resolves it -> (a, b), a <= b."""
    a, b, _ = slice(first, last).indices(n)
    return a, max(a, b)


def row_spans(plan, lengths: Sequence[int]) -> List[Tuple[int, int, int]]:
    """`plan` with every data span clipped to its segment's rows (`lengths[segment_index]`), as `pick` slices."""
    return [(i, a, b) if i == PAD else (i,) + _clip(a, b, lengths[i]) for i, a, b in plan]


def wave_spans(plan, frame_period, fs, wave_lengths: Sequence[int]) -> List[Tuple[int, int, int]]:
    """The sample spans that go with a row plan: `pick_wrapper` slices the segment's wave at round(first * frame_period / 1000 * fs) -- from the
    arguments of `pick`, not from the clipped rows -- and `silent_wrapper` pads round(width * frame_period / 1000 * fs) zeros."""
    out = []
    for i, a, b in plan:
        if i == PAD:
            out.append((PAD, 0, round(b * frame_period / 1000 * fs)))
        else:
            out.append((i,) + _clip(round(a * frame_period / 1000 * fs), round(b * frame_period / 1000 * fs), wave_lengths[i]))
    return out


def span_count(spans) -> int:
    return sum(b - a for _, a, b in spans)


def is_identity(spans, index: int, length: int) -> bool:
    """The plan hands on exactly segment `index`, whole: its non-empty spans are [(index, 0, length)]."""
    return [s for s in spans if s[2] > s[1]] == ([(index, 0, length)] if length > 0 else [])


def retire(segments: Sequence[Tuple[float, int]], current_time: float, time_length: float, extra_time: float, rate) -> int:
    """How many of the oldest segments `stream.remove(end_time=worker.retire_time(...))` drops once the wrapper's clock reads `current_time`:
    the leading run with `end_time <= retire_time`.  Segments arrive in time order, so that run is everything `remove` filters out; the store
    gives room back oldest first."""
    limit = retire_time(current_time, time_length, extra_time)
    n = 0
    for seg_start, seg_length in segments:
        if seg_length / rate + seg_start > limit:
            break
        n += 1
    return n


class Segment(object):
    """One stored segment: its clock, its rows and samples and where they lie in the rings."""

    def __init__(self, start_time: float, rows: int, samples: int, row_pos: int, sample_pos: int):
        self.start_time, self.rows, self.samples, self.row_pos, self.sample_pos = start_time, int(rows), int(samples), int(row_pos), int(sample_pos)


def _table(spans, positions, cap: int) -> numpy.ndarray:
    """Clipped spans -> the int32 [n][3] table of `ry_rowstore_fetch`: ring position or -1, destination offset, count."""
    out, at = numpy.empty((len(spans), 3), numpy.int32), 0
    for k, (i, a, b) in enumerate(spans):
        out[k] = (PAD if i == PAD else (positions[i] + a) % cap, at, b - a)
        at += b - a
    return out


class RowStore(DeviceHandle):
    """The rings of one live stream on the card: float32 mc [cap_rows][mc_cols], ap [cap_rows][ap_cols], wave [cap_samples].  `append` takes a
    segment from device blocks, `fetch` writes a window's rows and samples into the caller's blocks, `retire` gives the oldest segments' room
    back.  `segments` lists what is live, oldest first.  `ctx` (tests): a context over another build of the library."""
    _destroy = 'ry_rowstore_destroy'

    def __init__(self, mc_cols: int, ap_cols: int, cap_rows: int, cap_samples: int, ctx=None, device: Optional[int] = None):
        self.mc_cols, self.ap_cols, self.cap_rows, self.cap_samples = int(mc_cols), int(ap_cols), int(cap_rows), int(cap_samples)
        self.segments: List[Segment] = []
        DeviceHandle.__init__(self, ctx, device)

    def __getstate__(self):
        d = DeviceHandle.__getstate__(self)
        d['segments'] = []
        return d

    def _create(self, lib, ctx):
        h = ctypes.c_void_p()
        lib.check(lib.dll.ry_rowstore_create(ctx.handle, self.mc_cols, self.ap_cols, self.cap_rows, self.cap_samples, ctypes.byref(h)))
        return h

    def append(self, start_time: float, mc_ptr: int, ap_ptr: int, row0: int, n_rows: int, wave_ptr: int, sample0: int, n_samples: int) -> Segment:
        """Rows [row0, row0 + n_rows) of the device blocks at `mc_ptr` / `ap_ptr` and samples [sample0, sample0 + n_samples) of the wave at
        `wave_ptr` become the newest segment: one launch on the context stream, nothing is waited for."""
        lib, h = self._get()
        rp, sp = ctypes.c_int(), ctypes.c_int()
        lib.check(lib.dll.ry_rowstore_append(h, _lib._fptr(int(mc_ptr or 0)), _lib._fptr(int(ap_ptr or 0)), int(row0), int(n_rows), _lib._fptr(int(wave_ptr or 0)),
                                             int(sample0), int(n_samples), ctypes.byref(rp), ctypes.byref(sp)))
        seg = Segment(start_time, n_rows, n_samples, rp.value, sp.value)
        self.segments.append(seg)
        return seg

    def clocks(self) -> List[Tuple[float, int]]:
        """(start_time, rows) of the live segments: what `fetch_plan` / `retire` read."""
        return [(s.start_time, s.rows) for s in self.segments]

    def fetch(self, plan, frame_period, fs, mc_ptr: int, ap_ptr: int, wave_ptr: int, dst_rows: int, dst_samples: int) -> Tuple[int, int]:
        """Applies a `fetch_plan` over `clocks()`: the window's mc and ap rows and its samples, back to back from offset 0 of the three device
        blocks (room for dst_rows rows / dst_samples samples) -> (rows, samples) written.  One upload, one launch; the upload is waited for."""
        lib, h = self._get()
        rows = row_spans(plan, [s.rows for s in self.segments])
        samples = wave_spans(plan, frame_period, fs, [s.samples for s in self.segments])
        rt = _table(rows, [s.row_pos for s in self.segments], self.cap_rows)
        st = _table(samples, [s.sample_pos for s in self.segments], self.cap_samples)
        lib.check(lib.dll.ry_rowstore_fetch(h, rt.ctypes.data_as(_IP), len(rt), st.ctypes.data_as(_IP), len(st), _lib._fptr(int(mc_ptr or 0)),
                                            _lib._fptr(int(ap_ptr or 0)), _lib._fptr(int(wave_ptr or 0)), int(dst_rows), int(dst_samples)))
        return span_count(rows), span_count(samples)

    def download(self, seg: Segment):
        """The rows and samples of a live segment, brought to the host -> (mc, ap, wave) float32.  What a stream does once, when a buffer takes
        the composed path after resident ones; it waits for the context stream."""
        mc_ring, ap_ring, wave_ring = self.buffers()

        def part(ring, pos, n, cols, cap):
            out = numpy.empty((n, cols), numpy.float32)
            head = min(n, cap - pos)
            if head > 0:
                self._ctx.dev_download(ring + 4 * pos * cols, out[:head])
            if n > head:
                self._ctx.dev_download(ring, out[head:])
            return out
        return (part(mc_ring, seg.row_pos, seg.rows, self.mc_cols, self.cap_rows), part(ap_ring, seg.row_pos, seg.rows, self.ap_cols, self.cap_rows),
                part(wave_ring, seg.sample_pos, seg.samples, 1, self.cap_samples).ravel())

    def retire(self, n_segments: int) -> None:
        """The `n_segments` oldest segments may be overwritten from now on."""
        gone = self.segments[:int(n_segments)]
        if gone:
            lib, h = self._get()
            lib.check(lib.dll.ry_rowstore_retire(h, sum(s.rows for s in gone), sum(s.samples for s in gone)))
            del self.segments[:len(gone)]

    def reset(self) -> None:
        if self._handle is not None:
            lib, h = self._get()
            lib.check(lib.dll.ry_rowstore_reset(h))
        self.segments = []

    def held(self) -> Tuple[int, int]:
        lib, h = self._get()
        r, s = ctypes.c_int(), ctypes.c_int()
        lib.check(lib.dll.ry_rowstore_held(h, ctypes.byref(r), ctypes.byref(s)))
        return r.value, s.value

    def counts(self) -> dict:
        """tests: launches, uploads, waits and bytes uploaded by the last append / fetch."""
        lib, h = self._get()
        out = (ctypes.c_longlong * 4)()
        lib.check(lib.dll.ry_rowstore_debug_counts(h, out))
        return dict(zip(('launches', 'uploads', 'waits', 'upload_bytes'), (int(v) for v in out)))

    def buffers(self) -> Tuple[int, int, int]:
        """tests: the device addresses of the mc, ap and wave rings."""
        lib, h = self._get()
        p = [ctypes.c_void_p() for _ in range(3)]
        lib.check(lib.dll.ry_rowstore_debug_buffers(h, *[ctypes.byref(q) for q in p]))
        return tuple(int(q.value) for q in p)

    def poison(self) -> None:
        lib, h = self._get()
        lib.check(lib.dll.ry_rowstore_debug_poison(h))


def _ints(a, dtype=numpy.int32):
    a = numpy.ascontiguousarray(a, dtype=dtype).ravel()
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong if dtype == numpy.int64 else ctypes.c_int))


def _offsets(counts, dtype=numpy.int32) -> numpy.ndarray:
    return numpy.concatenate([[0], numpy.cumsum(counts, dtype=numpy.int64)]).astype(dtype)


class RowBank(DeviceHandle):
    """`RowStore` for the B live streams of one process (`ry_rowbank_*`): B sets of the three rings, one shape, each stream with its own
    `segments` list and live range.  Every device call names the streams it serves (`part`, ascending) and is ONE launch for all of them:
    `append_many` takes each stream's segment from the shared blocks a many-wave encode left on the card, `fetch_many` writes every stream's
    convert window back to back in the layout `VcCore.enqueue_waves_device` reads, `pick_ap` packs the ap rows the synthesizers read with the
    silence mask applied.  The plans are `fetch_plan`'s, per stream over `clocks(stream)`."""
    _destroy = 'ry_rowbank_destroy'

    def __init__(self, n_streams: int, mc_cols: int, ap_cols: int, cap_rows: int, cap_samples: int, ctx=None, device: Optional[int] = None):
        self.n_streams = int(n_streams)
        self.mc_cols, self.ap_cols, self.cap_rows, self.cap_samples = int(mc_cols), int(ap_cols), int(cap_rows), int(cap_samples)
        self.segments: List[List[Segment]] = [[] for _ in range(max(self.n_streams, 0))]
        DeviceHandle.__init__(self, ctx, device)

    def __getstate__(self):
        d = DeviceHandle.__getstate__(self)
        d['segments'] = [[] for _ in range(max(self.n_streams, 0))]
        return d

    def _create(self, lib, ctx):
        h = ctypes.c_void_p()
        lib.check(lib.dll.ry_rowbank_create(ctx.handle, self.n_streams, self.mc_cols, self.ap_cols, self.cap_rows, self.cap_samples, ctypes.byref(h)))
        return h

    def append_many(self, part, start_times, blocks, rows, samples) -> List[Segment]:
        """For every stream of `part` (ascending) its newest segment: rows [row0, row0 + n) of the device blocks `blocks = (mc, ap, wave)` --
        `rows[i] = (row0, n)` -- and samples `samples[i] = (sample0, n)` of the wave block -> the segments.  One launch; nothing is waited for up
        to two streams, a longer piece table goes up once."""
        lib, h = self._get()
        n = len(part)
        _, sp = _ints(part)
        r0, r0p = _ints([r[0] for r in rows])
        rn, rnp = _ints([r[1] for r in rows])
        s0, s0p = _ints([s[0] for s in samples], numpy.int64)
        sn, snp = _ints([s[1] for s in samples])
        rp, sq = numpy.zeros(max(n, 1), numpy.int32), numpy.zeros(max(n, 1), numpy.int32)
        lib.check(lib.dll.ry_rowbank_append(h, n, sp, _lib._fptr(int(blocks[0] or 0)), _lib._fptr(int(blocks[1] or 0)), r0p, rnp, _lib._fptr(int(blocks[2] or 0)),
                                            s0p, snp, rp.ctypes.data_as(_IP), sq.ctypes.data_as(_IP)))
        out = []
        for i, b in enumerate(part):
            out.append(Segment(start_times[i], rn[i], sn[i], rp[i], sq[i]))
            self.segments[b].append(out[-1])
        return out

    def clocks(self, stream: int) -> List[Tuple[float, int]]:
        return [(s.start_time, s.rows) for s in self.segments[stream]]

    def _row_tables(self, part, plans):
        """The clipped row spans of every stream's plan -> (spans per stream, the int32 table of all, its offsets per stream)."""
        spans = [row_spans(plan, [s.rows for s in self.segments[b]]) for b, plan in zip(part, plans)]
        tabs = [_table(sp, [s.row_pos for s in self.segments[b]], self.cap_rows) for b, sp in zip(part, spans)]
        return spans, numpy.concatenate(tabs + [numpy.empty((0, 3), numpy.int32)]), _offsets([len(t) for t in tabs])

    def fetch_many(self, part, plans, frame_period, fs, mc_ptr: int, wave_ptr: int) -> List[Tuple[int, int]]:
        """Applies one `fetch_plan` per stream of `part`: every window's mc rows back to back from row 0 of the block at `mc_ptr` and its samples
        back to back from sample 0 of the block at `wave_ptr` -> [(rows, samples)] per stream; the windows' offsets are the running sums of those.
        One upload, one launch; the upload is waited for."""
        lib, h = self._get()
        rows, rt, ro = self._row_tables(part, plans)
        samples = [wave_spans(plan, frame_period, fs, [s.samples for s in self.segments[b]]) for b, plan in zip(part, plans)]
        sts = [_table(sp, [s.sample_pos for s in self.segments[b]], self.cap_samples) for b, sp in zip(part, samples)]
        st, so = numpy.concatenate(sts + [numpy.empty((0, 3), numpy.int32)]), _offsets([len(t) for t in sts])
        sizes = [(span_count(r), span_count(s)) for r, s in zip(rows, samples)]
        fo, fop = _ints(_offsets([r for r, _ in sizes]))
        wo, wop = _ints(_offsets([s for _, s in sizes], numpy.int64), numpy.int64)
        lib.check(lib.dll.ry_rowbank_fetch(h, len(part), _ints(part)[1], rt.ctypes.data_as(_IP), ro.ctypes.data_as(_IP), st.ctypes.data_as(_IP),
                                           so.ctypes.data_as(_IP), _lib._fptr(int(mc_ptr or 0)), _lib._fptr(int(wave_ptr or 0)), fop, wop))
        return sizes

    def pick_ap(self, part, plans, keep, mask_ptr: int, ap_pack_ptr: int) -> int:
        """Behind the window call that wrote the mask at `mask_ptr` (one byte per window row, the windows in `fetch_many`'s layout): rows
        `keep[i] = (k0, k1)` of every stream's window ap go to the block at `ap_pack_ptr`, stream after stream, zeros where the mask cut the
        frame or the plan pads -> the rows packed.  One launch; the full ap window is written nowhere."""
        lib, h = self._get()
        rows, rt, ro = self._row_tables(part, plans)
        fo, fop = _ints(_offsets([span_count(r) for r in rows]))
        kp, kpp = _ints([int(k) for pair in keep for k in pair])
        total = int(sum(k1 - k0 for k0, k1 in keep))
        lib.check(lib.dll.ry_rowbank_pick_ap(h, len(part), _ints(part)[1], rt.ctypes.data_as(_IP), ro.ctypes.data_as(_IP), fop, kpp,
                                             ctypes.cast(ctypes.c_void_p(int(mask_ptr or 0)), ctypes.POINTER(ctypes.c_ubyte)), _lib._fptr(int(ap_pack_ptr or 0)),
                                             total))
        return total

    def download(self, stream: int, seg: Segment):
        """The rows and samples of a live segment of `stream`, brought to the host -> (mc, ap, wave) float32; waits for the context stream."""
        mc_ring, ap_ring, wave_ring = self.buffers()

        def part(ring, pos, n, cols, cap):
            ring += 4 * stream * cap * cols
            out = numpy.empty((n, cols), numpy.float32)
            head = min(n, cap - pos)
            if head > 0:
                self._ctx.dev_download(ring + 4 * pos * cols, out[:head])
            if n > head:
                self._ctx.dev_download(ring, out[head:])
            return out
        return (part(mc_ring, seg.row_pos, seg.rows, self.mc_cols, self.cap_rows), part(ap_ring, seg.row_pos, seg.rows, self.ap_cols, self.cap_rows),
                part(wave_ring, seg.sample_pos, seg.samples, 1, self.cap_samples).ravel())

    def retire(self, stream: int, n_segments: int) -> None:
        """The `n_segments` oldest segments of `stream` may be overwritten from now on."""
        gone = self.segments[stream][:int(n_segments)]
        if gone:
            lib, h = self._get()
            lib.check(lib.dll.ry_rowbank_retire(h, int(stream), sum(s.rows for s in gone), sum(s.samples for s in gone)))
            del self.segments[stream][:len(gone)]

    def reset(self, stream: Optional[int] = None) -> None:
        if self._handle is not None:
            lib, h = self._get()
            lib.check(lib.dll.ry_rowbank_reset(h, -1 if stream is None else int(stream)))
        for b in range(self.n_streams):
            if stream is None or b == int(stream):
                self.segments[b] = []

    def held(self, stream: int) -> Tuple[int, int]:
        lib, h = self._get()
        r, s = ctypes.c_int(), ctypes.c_int()
        lib.check(lib.dll.ry_rowbank_held(h, int(stream), ctypes.byref(r), ctypes.byref(s)))
        return r.value, s.value

    def counts(self) -> dict:
        """tests: launches, uploads, waits and bytes uploaded by the last append / fetch / pick."""
        lib, h = self._get()
        out = (ctypes.c_longlong * 4)()
        lib.check(lib.dll.ry_rowbank_debug_counts(h, out))
        return dict(zip(('launches', 'uploads', 'waits', 'upload_bytes'), (int(v) for v in out)))

    def buffers(self) -> Tuple[int, int, int]:
        """tests: the device addresses of the mc, ap and wave arrays (stream b's rings lie b rings in)."""
        lib, h = self._get()
        p = [ctypes.c_void_p() for _ in range(3)]
        lib.check(lib.dll.ry_rowbank_debug_buffers(h, *[ctypes.byref(q) for q in p]))
        return tuple(int(q.value) for q in p)

    def poison(self) -> None:
        lib, h = self._get()
        lib.check(lib.dll.ry_rowbank_debug_poison(h))
