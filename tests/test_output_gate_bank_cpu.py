"""A bank of output gates (ry_outgate_bank_*) on the emulator: B = 1, 3 and 5 streams with different signals, cuts of their own, calls they sit out and
one stream reset mid-way.  Every stream is bit-equal to its lone `OutputGate`, call by call; the launches, uploads and downloads of a call do not
depend on B (output_gate_checks.check_bank reads the counters after every call)."""
import numpy
import pytest

import output_gate_cases as C
import output_gate_checks as K
from realtime_yukarin_amd.output_gate import OutputGate, OutputGateBank


@pytest.mark.parametrize('B', [1, 3, 5])
def test_bank_equals_lone_gates(emu_ctx, B):
    K.check_bank(emu_ctx, B, 1536)


def test_bank_equals_lone_gates_poisoned_float32(emu_ctx):
    K.check_bank(emu_ctx, 3, 2049, poison=True)
    bank = OutputGateBank(2, 1025, C.THRESHOLD, K.SCALE, numpy.float32, ctx=emu_ctx)
    lone = OutputGate(1025, C.THRESHOLD, K.SCALE, numpy.float32, ctx=emu_ctx)
    x = C.signal('voiced', 1025)
    got = bank.push([None, x])
    want = lone.push(x)
    assert got[0] is None and got[1].dtype == numpy.float32 and K.same_chunk(got[1], want)
    assert bank.push([None, None]) == [None, None]
    bank.close(); lone.close()


def test_every_stream_completes_in_one_call(emu_ctx):
    """The cost of a call that completes a chunk in every stream: four launches, one upload, one record download, whatever B is."""
    chunk = 1025
    for B in (1, 4):
        bank = OutputGateBank(B, chunk, C.THRESHOLD, ctx=emu_ctx)
        for _ in range(3):
            out = bank.push([C.signal('noise1e-6', chunk)] * B)
        c = bank.counts()
        assert out == [None] * B and all(r[:2] == (True, True) for r in bank.last)
        assert (c['waits'], c['launches'], c['uploads'], c['downloads'], c['sample_bytes_down']) == (1, 4, 1, 1, 0), c
        out = bank.push([C.signal('sine', chunk)] * B)
        c = bank.counts()
        assert all(o is not None for o in out)
        assert (c['waits'], c['launches'], c['uploads'], c['downloads'], c['sample_bytes_down']) == (2, 4, 1, 1 + B, B * chunk * 8), c
        bank.close()
