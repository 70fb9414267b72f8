"""`streams.fetch_plan` / `row_spans` / `wave_spans` against the reference's own `BaseStream.fetch`, run unchanged over its
`FeatureWrapperSegmentMethod` and `WaveSegmentMethod`.  The data arrays carry their own indices (segment * 10^6 + index + 1; a pad is 0), so the
concatenation the reference returns IS the plan, and equality is exact -- lengths included.  The clocks are accumulated as the workers do
(`start_time += time_length` from `extra_time`, `_current_time += time_length` from 0).  Our side drops what `streams.retire` says may go
after every window, the reference's list keeps everything (its loops never call `remove`): the same windows must come out."""
import importlib
from pathlib import Path

import numpy
import pytest

import reference_checkout
from realtime_yukarin_amd import compat, streams

ROOT = Path(__file__).resolve().parent.parent
REF = reference_checkout.locate(Path('/root/reference'))
pytestmark = pytest.mark.skipif(REF is None, reason=reference_checkout.SKIP_REASON)
FS, ORDER = 24000, 8


@pytest.fixture
def ref(monkeypatch):
    compat.install()
    for p in (str(ROOT / 'tests' / 'stubs'), str(REF)):
        monkeypatch.syspath_prepend(p)
    mod = lambda name: importlib.import_module('realtime_voice_conversion.' + name)
    return dict(base=mod('stream.base_stream'), feature=mod('segment.feature_wrapper_segment'), wave=mod('segment.wave_segment'),
                wrapper=mod('yukarin_wrapper.acoustic_feature_wrapper'))


def ids(segment: int, n: int) -> numpy.ndarray:
    return segment * 1e6 + numpy.arange(n, dtype=numpy.float64) + 1


def apply_plan(spans, segment_of):
    """zeros for a pad, ids for data: what the reference's concatenation holds when the plan is right."""
    parts = [numpy.zeros(b - a) if i == streams.PAD else ids(segment_of[i], b)[a:b] for i, a, b in spans]
    return numpy.concatenate(parts) if parts else numpy.zeros(0)


def run_stream(ref, kind, frame_period, time_length, extra_time, n_buffers, seg_rows, missing=(), first_add=0, windows_only=0):
    """`n_buffers` items through add + fetch with the workers' clocks.  kind 'feature': segments of `seg_rows` frames with the wave of one buffer;
    kind 'wave': segments of one buffer's samples.  missing: buffers that never arrive (their clocks still advance); first_add: the first
    `first_add` windows are fetched before any data exists; windows_only: further windows after the last add."""
    from yukarin.wave import Wave
    rate = 1000 // frame_period
    buf_samples = round(time_length * FS)
    if kind == 'feature':
        method = ref['feature'].FeatureWrapperSegmentMethod(sampling_rate=rate, wave_sampling_rate=FS, order=ORDER, frame_period=frame_period, keys=['f0'])
    else:
        method = ref['wave'].WaveSegmentMethod(sampling_rate=FS)
        rate = FS
    stream = ref['base'].BaseStream(in_segment_method=method, out_segment_method=None)
    ours, number = [], []                                 # (start_time, length, samples) of the live segments, their arrival numbers
    add_clock, window_clock = extra_time, 0.
    n_pads = n_data = n_empty = 0
    for k in range(n_buffers + windows_only):
        arrives = k >= first_add and k < n_buffers and k not in missing
        if arrives:
            if kind == 'feature':
                data = ref['wrapper'].AcousticFeatureWrapper(wave=Wave(wave=ids(k, buf_samples), sampling_rate=FS), f0=ids(k, seg_rows)[:, None])
                ours.append((add_clock, seg_rows, buf_samples))
            else:
                data = ids(k, buf_samples)
                ours.append((add_clock, buf_samples, buf_samples))
            number.append(k)
            stream.add(start_time=add_clock, data=data)
        add_clock += time_length
        want = stream.fetch(start_time=window_clock, time_length=time_length, extra_time=extra_time)
        plan = streams.fetch_plan([(s, n) for s, n, _ in ours], window_clock, time_length, extra_time, rate)
        rows = streams.row_spans(plan, [n for _, n, _ in ours])
        assert all(b >= a >= 0 for _, a, b in rows)
        if kind == 'feature':
            assert numpy.array_equal(numpy.asarray(want.f0).ravel(), apply_plan(rows, number)), (k, plan)
            samples = streams.wave_spans(plan, frame_period, FS, [w for _, _, w in ours])
            assert numpy.array_equal(want.wave.wave, apply_plan(samples, number)), (k, plan, samples)
        else:
            assert numpy.array_equal(want, apply_plan(rows, number)), (k, plan)
        n_pads += sum(i == streams.PAD and b > a for i, a, b in rows)
        n_data += sum(i != streams.PAD and b > a for i, a, b in rows)
        n_empty += sum(b == a for _, a, b in rows)
        window_clock += time_length
        gone = streams.retire([(s, n) for s, n, _ in ours], window_clock, time_length, extra_time, rate)
        del ours[:gone], number[:gone]
    assert len(ours) <= 4 + int(2 * extra_time / time_length)            # the store stays bounded
    return dict(pads=n_pads, data=n_data, empty=n_empty)


def test_the_shipped_margins_with_the_one_frame_overlap(ref):
    """1 s buffers, (0, 0.5, 0): what EncodeStream, ConvertStream and DecodeStream fetch over 12 buffers -- 201-frame segments at rate 200 overlap
    their successors by one frame, which `fetch` resolves with its own rounding."""
    assert run_stream(ref, 'wave', 5, 1.0, 0.0, 12, 0)['data'] >= 12
    got = run_stream(ref, 'feature', 5, 1.0, 0.5, 12, 201)
    assert got['pads'] >= 1 and got['data'] >= 23
    run_stream(ref, 'feature', 5, 1.0, 0.0, 12, 200)
    run_stream(ref, 'feature', 5, 1.0, 0.0, 12, 201)


@pytest.mark.parametrize('margins', [(0.5, 0.5, 0.5), (0.1, 0.05, 0.0)])
def test_other_margins(ref, margins):
    for extra in margins:
        run_stream(ref, 'wave', 5, 1.0, extra, 8, 0)
        for seg_rows in (200, 201):
            run_stream(ref, 'feature', 5, 1.0, extra, 8, seg_rows)


def test_a_tenth_of_a_second_at_frame_period_5(ref):
    """0.1 s buffers: 21-frame segments (20 after a pick), margins of 0, 0.05 and 0.1 s."""
    for extra in (0.0, 0.05, 0.1):
        run_stream(ref, 'wave', 5, 0.1, extra, 10, 0)
        for seg_rows in (20, 21):
            run_stream(ref, 'feature', 5, 0.1, extra, 10, seg_rows)


def test_a_missing_buffer_gives_a_pad_in_the_middle(ref):
    for kind, seg_rows in (('wave', 0), ('feature', 201), ('feature', 200)):
        with_gap = run_stream(ref, kind, 5, 1.0, 0.5, 9, seg_rows, missing=(4,))
        without = run_stream(ref, kind, 5, 1.0, 0.5, 9, seg_rows)
        assert with_gap['pads'] > without['pads']
    run_stream(ref, 'feature', 5, 0.1, 0.05, 12, 21, missing=(3, 4, 8))


def test_windows_before_any_data_and_after_the_last(ref):
    for kind, seg_rows in (('wave', 0), ('feature', 21)):
        got = run_stream(ref, kind, 5, 0.1, 0.05, 8, seg_rows, first_add=3, windows_only=3)
        assert got['pads'] >= 6


def test_clocks_accumulated_over_1000_buffers(ref):
    """0.1 is not a binary fraction: after 1000 additions the two clocks have drifted from k / 10 and from each other's rounding.  The plan
    follows the reference through every window, and empty spans -- a segment that ends where the window starts -- do occur."""
    empty = 0
    for extra in (0.0, 0.05):
        empty += run_stream(ref, 'feature', 5, 0.1, extra, 1000, 21)['empty']
        empty += run_stream(ref, 'feature', 5, 0.1, extra, 1000, 20)['empty']
    run_stream(ref, 'wave', 5, 0.1, 0.0, 1000, 0)
    assert empty > 0


def test_identity_and_counts():
    plan = [(0, 20, 20), (1, 0, 20)]
    assert streams.is_identity(plan, 1, 20) and not streams.is_identity(plan, 0, 20) and not streams.is_identity([(1, 0, 19)], 1, 20)
    assert not streams.is_identity([(streams.PAD, 0, 3), (1, 0, 20)], 1, 20)
    assert streams.span_count([(streams.PAD, 0, 3), (1, 2, 20)]) == 21
    assert streams.row_spans([(0, 5, 30), (0, -3, 9)], [21]) == [(0, 5, 21), (0, 18, 18)]
