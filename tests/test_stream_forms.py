"""The stream topology of the window lanes (`ry_vc_create` / `ry_vc_set_lanes`: wide, compact-a, compact-b) on the emulator: the same
sequence of calls (tests/stream_forms_scenario.py) returns the same bits in every form and with one lane, the core enqueues on no more streams
than the form allows, and the form follows GPU_MAX_HW_QUEUES as the environment gives it when the core is made.  The emulator runs every
launch at once, so what this holds is the host side: which handle and which stream a call goes to, clones on borrowed streams, the rebuilt
clones when the lane count changes the form."""
import numpy
import pytest

import stream_forms_scenario as scenario
import window_call_ref as wr
from realtime_yukarin_amd import engine

FRAMES = (8, 16)
WINDOWS, DEV_WINDOWS = 7, 3            # host windows, then device-pointer windows (the last host windows, backwards): ten calls over the six ring slots
_runs = {}


def run(ctx, n, lanes, form):
    key = (n, lanes, form)
    if key not in _runs:
        _runs[key] = scenario.run(ctx, 'SYN-8', n, lanes, form, count=WINDOWS, dev_count=DEV_WINDOWS, waves=1, batches=1)
    return _runs[key]


@pytest.mark.parametrize('n', FRAMES)
def test_the_scenario_sees_what_it_should(emu_ctx, n):
    """No-op guards: the windows differ, a gated window really is gated, nothing the calls should write still holds the sentinel."""
    ref = run(emu_ctx, n, 1, 'wide')
    wr.all_differ([ref['host_sp_%02d' % i] for i in range(WINDOWS)], 'spectrogram of window')
    _, eff = scenario.windows(n)[scenario.GATED]
    assert 0 < eff.sum() < n and not ref['host_mc_%02d' % scenario.GATED][~eff].any() and ref['host_mc_%02d' % scenario.GATED][eff].all()
    for k, a in ref.items():
        if a.dtype == numpy.float32:
            assert numpy.isfinite(a).all() and not (a == wr.SENTINEL).any(), k
    for i in range(DEV_WINDOWS):                  # the device-pointer call and the host call agree window by window
        wr.same_bits(ref['dev_sp_%02d' % i], ref['host_sp_%02d' % (WINDOWS - 1 - i)], 'window %d, device pointers against host arrays' % (WINDOWS - 1 - i))


@pytest.mark.parametrize('form', ['wide', 'compact-a', 'compact-b'])
@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('n', FRAMES)
def test_every_form_returns_the_bits_of_one_lane(emu_ctx, n, lanes, form):
    ref, got = run(emu_ctx, n, 1, 'wide'), run(emu_ctx, n, lanes, form)
    assert engine.VcCore.STREAM_FORMS[int(got['form'])] == form
    assert set(got) == set(ref)
    for k in sorted(ref):
        if k not in ('form', 'n_streams'):
            wr.same_bits(got[k], ref[k], '%s, %d frames, %d lanes, %s' % (k, n, lanes, form))
    # the streams the calls went to: a stage-1 and a stage-2 stream per lane; one per lane; one stage-1 stream and one stage-2 stream per lane
    assert int(got['n_streams']) == {'wide': 2 * lanes, 'compact-a': lanes, 'compact-b': 1 + lanes}[form]


def test_compact_names_the_form_that_is_kept(emu_ctx):
    got = run(emu_ctx, 8, 2, 'compact')
    assert engine.VcCore.STREAM_FORMS[int(got['form'])] in ('compact-a', 'compact-b')
    assert int(got['n_streams']) <= (2 if int(got['form']) == 1 else 3)


@pytest.mark.parametrize('queues, want', [(None, 'compact'), ('4', 'compact'), ('5', 'compact'), ('6', 'wide'), ('16', 'wide')])
def test_the_form_follows_the_queues_of_the_environment(emu_ctx, monkeypatch, queues, want):
    """Two lanes of the wide form are four streams, six users of hardware queues with the context and the null stream.  An absent
    variable is HIP's default of 4.  One lane (four users) is wide under every value."""
    monkeypatch.delenv('RY_VC_STREAMS', raising=False)
    if queues is None:
        monkeypatch.delenv('GPU_MAX_HW_QUEUES', raising=False)
    else:
        monkeypatch.setenv('GPU_MAX_HW_QUEUES', queues)
    n1, n2 = wr.make_pair(emu_ctx, 'SYN-8')
    try:
        core = engine.VcCore(n1, n2, wr.mtx('SYN-8'), lanes=2)
        two = core.debug_streams()[0]
        monkeypatch.setenv('GPU_MAX_HW_QUEUES', '16')          # read when the core is made: a later value changes nothing
        core.set_lanes(1)
        one = core.debug_streams()[0]
        core.set_lanes(2)                                       # ... and the clones come back in the form of two lanes
        x, e = scenario.windows(8)[0]
        mc, sp = core.convert(x, e)
        again = core.debug_streams()
        core.close()
    finally:
        n1.close(); n2.close()
    kept = run(emu_ctx, 8, 2, 'compact')
    assert two == (engine.VcCore.STREAM_FORMS[int(kept['form'])] if want == 'compact' else 'wide')
    assert one == 'wide' and again[0] == two and again[1] == (2 if two != 'compact-a' else 1)
    wr.same_bits(sp, run(emu_ctx, 8, 1, 'wide')['host_sp_00'], 'a window after the lanes went 2 -> 1 -> 2')


def test_an_unknown_form_is_refused(emu_ctx, monkeypatch):
    from realtime_yukarin_amd import _lib
    monkeypatch.setenv('RY_VC_STREAMS', 'narrow')
    n1, n2 = wr.make_pair(emu_ctx, 'SYN-8')
    try:
        with pytest.raises(_lib.Ry355Error, match='RY_VC_STREAMS'):
            engine.VcCore(n1, n2, wr.mtx('SYN-8'), lanes=2)
    finally:
        n1.close(); n2.close()
