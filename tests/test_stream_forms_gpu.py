"""The stream topology of the window lanes on the GPU, where streams, events and hardware queues are real: the sequence of calls of
tests/stream_forms_scenario.py in two fresh child processes, one started with GPU_MAX_HW_QUEUES=4 and one with 16 (the HIP runtime reads
the variable when it starts, so a child is the only way).  Each child runs SYN-8 at 16 frames and SYN-64 at 100 frames (the smallest shape
that walks the Winograd, implicit-GEMM and output-stationary families of stage 2) with one lane, and with two lanes in every form and in
the form the core picks by itself, and dumps what the calls returned.  This process compares the dumps bit for bit: within a child against
one lane, and between the children.  Nothing here asserts a speed."""
import os
import subprocess
import sys
from pathlib import Path

import numpy
import pytest

import stream_forms_scenario as scenario
import window_call_ref as wr

SHAPES = (('SYN-8', 16), ('SYN-64', 100))
CHILD_LIMIT = 300          # seconds; a child takes some tens (imports, five cores per shape, their launch plans and graphs)
FORMS = ('wide', 'compact-a', 'compact-b')


@pytest.fixture(scope='module')
def dumps(tmp_path_factory):
    """{queues: {(model, frames, lanes, form or 'auto'): {name: array}}} of the two children, one after the other."""
    out = {}
    for queues in ('4', '16'):
        d = tmp_path_factory.mktemp('streams_q' + queues)
        env = dict(os.environ, GPU_MAX_HW_QUEUES=queues)
        env.pop('RY_VC_STREAMS', None)
        cmd = [sys.executable, str(Path(scenario.__file__).resolve()), str(d)] + [str(v) for s in SHAPES for v in s]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_LIMIT)
        assert p.returncode == 0, 'child with GPU_MAX_HW_QUEUES=%s ended with %s:\n%s' % (queues, p.returncode, p.stdout[-3000:])
        out[queues] = {}
        for name, n in SHAPES:
            for lanes, form in scenario.COMBOS:
                with numpy.load(str(d / ('%s_%d_l%d_%s.npz' % (name, n, lanes, form or 'auto')))) as z:
                    out[queues][(name, n, lanes, form or 'auto')] = {k: z[k] for k in z.files}
    return out


def arrays(run):
    return sorted(k for k in run if k not in ('form', 'n_streams'))


@pytest.mark.gpu
@pytest.mark.parametrize('name, n', SHAPES)
def test_the_children_saw_what_they_should(dumps, name, n):
    """No-op guards on the reference of each child: distinct windows, the gated window gated, no sentinel left, device-pointer calls and host calls agree."""
    for queues in ('4', '16'):
        ref = dumps[queues][(name, n, 1, 'wide')]
        wr.all_differ([ref['host_sp_%02d' % i] for i in range(scenario.N_WINDOWS)], 'spectrogram of window')
        _, eff = scenario.windows(n)[scenario.GATED]
        assert 0 < eff.sum() < n and not ref['host_mc_%02d' % scenario.GATED][~eff].any()
        for k in arrays(ref):
            if ref[k].dtype == numpy.float32:
                assert numpy.isfinite(ref[k]).all() and not (ref[k] == wr.SENTINEL).any(), k
        for i in range(scenario.N_WINDOWS):
            j = scenario.N_WINDOWS - 1 - i                       # the device-pointer calls take the windows backwards
            wr.same_bits(ref['dev_sp_%02d' % i], ref['host_sp_%02d' % j], 'window %d, device pointers against host arrays' % j)


@pytest.mark.gpu
@pytest.mark.parametrize('queues', ['4', '16'])
@pytest.mark.parametrize('name, n', SHAPES)
def test_every_form_returns_the_bits_of_one_lane_gpu(dumps, name, n, queues):
    ref = dumps[queues][(name, n, 1, 'wide')]
    for lanes, form in scenario.COMBOS[1:]:
        got = dumps[queues][(name, n, lanes, form or 'auto')]
        assert arrays(got) == arrays(ref)
        for k in arrays(ref):
            wr.same_bits(got[k], ref[k], '%s, %s at %d frames, %d lanes, %s, GPU_MAX_HW_QUEUES=%s' % (k, name, n, lanes, form or 'auto', queues))
        used = FORMS[int(got['form'])]
        if form is not None:
            assert used == form
        assert int(got['n_streams']) == {'wide': 2 * lanes, 'compact-a': lanes, 'compact-b': 1 + lanes}[used]


@pytest.mark.gpu
@pytest.mark.parametrize('name, n', SHAPES)
def test_the_queues_pick_the_form_and_change_no_bit(dumps, name, n):
    assert FORMS[int(dumps['4'][(name, n, 2, 'auto')]['form'])] == 'compact-b'          # six users of queues do not fit into four
    assert FORMS[int(dumps['16'][(name, n, 2, 'auto')]['form'])] == 'wide'
    a, b = dumps['4'][(name, n, 2, 'auto')], dumps['16'][(name, n, 2, 'auto')]
    for k in arrays(a):
        wr.same_bits(a[k], b[k], '%s, %s at %d frames: four queues against sixteen' % (k, name, n))
