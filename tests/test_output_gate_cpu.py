"""The output gate (csrc/outgate.cpp, outgate_kernels.h, realtime_yukarin_amd/output_gate.py) on the emulator against the float64 restatement of the
reference's decode worker tail (output_gate_ref.py): mean_db and verdict per case, emitted bits, split invariance, one chunk per push, NaN and
inf, poison, every refusal and the state after it, untouched output of a silent chunk, waits and bytes.  The bodies shared with the GPU tests
and the measured tolerance are in output_gate_checks.py."""
import ctypes
import os
import types

import numpy
import pytest

import output_gate_cases as C
import output_gate_checks as K
import output_gate_ref as R
from realtime_yukarin_amd import engine, output_gate
from realtime_yukarin_amd.output_gate import OutputGate

_DP = ctypes.POINTER(ctypes.c_double)
EINVAL, ESTATE = -1, -4


def test_every_case_has_a_verdict_margin():
    """With threshold 80 every listed case lies at least 4 dB from the threshold in the float64 reference; the click is silent in the shipped chunk
    and audible in the shortest one."""
    assert C.verdict_cases() == C.CASES
    assert min(abs(C.ref_mean(s, n) + C.THRESHOLD) for s, n in C.CASES) >= 4.0
    assert abs(C.ref_mean('click', 24000) + 87.8) < 0.05 and abs(C.ref_mean('click', 1025) + 34.7) < 0.05


def test_host_expression_is_the_reference():
    for name, n in (('voiced', 1025), ('noise3e-6', 2049), ('click', 4096)):
        assert abs(output_gate.host_mean_db(C.signal(name, n)) - C.ref_mean(name, n)) <= 1e-11
    assert abs(R.mean_db(C.signal('voiced', 4096), complex64=True) - C.ref_mean('voiced', 4096)) <= 1.6e-5      # what librosa's complex64 costs


@pytest.mark.parametrize('dtype', [numpy.float64, numpy.float32])
@pytest.mark.parametrize('name,n', C.CASES)
def test_case(emu_ctx, name, n, dtype):
    K.check_case(emu_ctx, name, n, dtype)


def test_click_verdicts(emu_ctx):
    for n, silent in ((24000, True), (1025, False)):
        g = OutputGate(n, C.THRESHOLD, ctx=emu_ctx)
        out = g.push(C.signal('click', n))
        assert g.last[:2] == (True, silent) and (out is None) == silent
        g.close()


@pytest.mark.parametrize('chunk', [1025, 2048, 2049])
def test_splits(emu_ctx, chunk):
    K.check_splits(emu_ctx, chunk, seeds=(1, 2, 3, 4))


def test_one_chunk_per_push(emu_ctx):
    """2.5 chunks at once, then empty pushes: one chunk each, the rest carried, ry_outgate_held as the reference's fragment."""
    chunk = 1536
    x = K.three_chunks(chunk)[:chunk * 5 // 2]
    gate, ref = OutputGate(chunk, C.THRESHOLD, K.SCALE, ctx=emu_ctx), R.Gate(chunk, C.THRESHOLD, K.SCALE)
    for piece in (x, x[:0], x[:0], x[:0]):
        got = gate.push(piece)
        want, rec = ref.push(piece)
        assert K.same_chunk(got, want) and K.same_record(gate.last, rec)
        assert gate.held() == len(ref.fragment)
    assert gate.held() == chunk // 2 and gate.last == (False, False, 0.0)
    gate.reset()
    assert gate.held() == 0 and gate.push(x[:chunk - 1]) is None and gate.last[0] is False
    gate.close()


def test_nan_and_inf(emu_ctx):
    K.check_nonfinite(emu_ctx, 2049)


def test_poison(emu_ctx):
    K.check_poison(emu_ctx, 1536)


def test_short_chunks_take_the_host_expression(emu_ctx):
    """Below 1025 samples the C ABI refuses; the Python layer evaluates the same expression on the host."""
    chunk = 700
    x = numpy.concatenate([C.signal('voiced', chunk), C.signal('noise1e-6', chunk)])
    gate, ref = OutputGate(chunk, C.THRESHOLD, K.SCALE, numpy.float32, ctx=emu_ctx), R.Gate(chunk, C.THRESHOLD, K.SCALE, numpy.float32)
    for piece in (x[:100], x[100:], x[:0]):
        got = gate.push(piece)
        want, rec = ref.push(piece)
        assert K.same_chunk(got, want) and gate.last[:2] == rec[:2] and abs(gate.last[2] - rec[2]) <= 1e-11
    assert gate._handle is None


def _raw(emu_ctx, chunk=2048, f32=0):
    h = ctypes.c_void_p()
    emu_ctx.lib.check(emu_ctx.lib.dll.ry_outgate_create(emu_ctx.handle, chunk, C.THRESHOLD, K.SCALE, f32, ctypes.byref(h)))
    return h


def _msg(ctx):
    return ctx.lib.dll.ry_last_error().decode()


def test_refusals_and_state_after_them(emu_ctx):
    dll = emu_ctx.lib.dll
    h = ctypes.c_void_p()
    nan = float('nan')
    assert dll.ry_outgate_create(emu_ctx.handle, 1024, 80.0, 1.0, 0, ctypes.byref(h)) == EINVAL and '1025' in _msg(emu_ctx) and not h.value
    assert dll.ry_outgate_create(emu_ctx.handle, 2048, nan, 1.0, 0, ctypes.byref(h)) == EINVAL and 'NaN' in _msg(emu_ctx) and not h.value
    assert dll.ry_outgate_create(emu_ctx.handle, 2048, 80.0, nan, 0, ctypes.byref(h)) == EINVAL and 'NaN' in _msg(emu_ctx)
    assert dll.ry_outgate_create(None, 2048, 80.0, 1.0, 0, ctypes.byref(h)) == EINVAL and 'null context' in _msg(emu_ctx)
    assert dll.ry_outgate_create(emu_ctx.handle, 2048, 80.0, 1.0, 0, None) == EINVAL and 'null out' in _msg(emu_ctx)
    k = ctypes.c_void_p()
    assert dll.ry_outgate_bank_create(emu_ctx.handle, 0, 2048, 80.0, 1.0, 0, ctypes.byref(k)) == EINVAL and 'streams' in _msg(emu_ctx)
    assert dll.ry_outgate_bank_create(emu_ctx.handle, 2, 1000, 80.0, 1.0, 0, ctypes.byref(k)) == EINVAL and '1025' in _msg(emu_ctx)
    assert dll.ry_outgate_bank_create(emu_ctx.handle, 2, 2048, nan, 1.0, 0, ctypes.byref(k)) == EINVAL and not k.value

    chunk = 2048
    h = _raw(emu_ctx, chunk)
    x = numpy.ascontiguousarray(K.three_chunks(chunk))
    ref = R.Gate(chunk, C.THRESHOLD, K.SCALE)
    out = numpy.full(chunk, -7.25)
    n_out, silent, mean = ctypes.c_int(-9), ctypes.c_int(-9), ctypes.c_double(-9.0)
    vp = out.ctypes.data_as(ctypes.c_void_p)
    args = lambda n, o=vp, cap=chunk: (h, x.ctypes.data_as(_DP), n, 0, o, cap, ctypes.byref(n_out), ctypes.byref(silent), ctypes.byref(mean))
    emu_ctx.lib.check(dll.ry_outgate_push(*args(1000)))             # a carried fragment that the refusals must leave alone
    ref.push(x[:1000])
    assert dll.ry_outgate_push(None, x.ctypes.data_as(_DP), 10, 0, vp, chunk, ctypes.byref(n_out), ctypes.byref(silent), ctypes.byref(mean)) == ESTATE
    assert 'null output gate' in _msg(emu_ctx)
    assert dll.ry_outgate_push(h, None, 10, 0, vp, chunk, ctypes.byref(n_out), ctypes.byref(silent), ctypes.byref(mean)) == EINVAL and 'null samples' in _msg(emu_ctx)
    assert dll.ry_outgate_push(*args(1048, o=None)) == EINVAL and 'null out' in _msg(emu_ctx)
    assert dll.ry_outgate_push(h, x.ctypes.data_as(_DP), 10, 0, vp, chunk, None, ctypes.byref(silent), ctypes.byref(mean)) == EINVAL
    assert dll.ry_outgate_push(*args(-1)) == EINVAL and '-1 samples' in _msg(emu_ctx)
    assert dll.ry_outgate_push(*args(1048, cap=chunk - 1)) == EINVAL and 'out holds' in _msg(emu_ctx)
    assert dll.ry_outgate_push(*args(1048, cap=-1)) == EINVAL
    assert dll.ry_outgate_reset(None) == ESTATE and dll.ry_outgate_held(None) < 0 and dll.ry_outgate_debug_poison(None) == ESTATE
    assert dll.ry_outgate_held(h) == 1000 and (out == -7.25).all()
    # the next valid push gives the reference bits
    xs = numpy.ascontiguousarray(x[1000:])
    emu_ctx.lib.check(dll.ry_outgate_push(h, xs.ctypes.data_as(_DP), chunk, 0, vp, chunk, ctypes.byref(n_out), ctypes.byref(silent), ctypes.byref(mean)))
    want, rec = ref.push(xs[:chunk])
    assert n_out.value == chunk and silent.value == 0 and out.tobytes() == want.tobytes() and abs(mean.value - rec[2]) <= K.MEAN_TOL
    dll.ry_outgate_destroy(h)
    dll.ry_outgate_destroy(None)

    # the bank's refusals: outputs untouched, streams as they were
    B = 2
    emu_ctx.lib.check(dll.ry_outgate_bank_create(emu_ctx.handle, B, chunk, C.THRESHOLD, K.SCALE, 0, ctypes.byref(k)))
    LLP = ctypes.POINTER(ctypes.c_longlong)
    off = numpy.array([0, 500, 500 + chunk], numpy.int64)
    oo, sil, mdb = numpy.full(B + 1, -99, numpy.int64), numpy.full(B, -99, numpy.int32), numpy.full(B, -9.0)
    out2 = numpy.full(B * chunk, -7.25)

    def bank_push(samples=x.ctypes.data_as(_DP), offs=off, o=out2.ctypes.data_as(ctypes.c_void_p), cap=B * chunk, kk=None):
        return dll.ry_outgate_bank_push(k if kk is None else kk, samples, offs.ctypes.data_as(LLP) if offs is not None else None, 0, o, cap,
                                        oo.ctypes.data_as(LLP), sil.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), mdb.ctypes.data_as(_DP))
    assert bank_push(samples=None) == EINVAL and bank_push(offs=None) == EINVAL and bank_push(o=None) == EINVAL
    assert bank_push(offs=numpy.array([0, 500, 400], numpy.int64)) == EINVAL and 'stream 1' in _msg(emu_ctx)
    assert bank_push(offs=numpy.array([1, 500, 600], numpy.int64)) == EINVAL
    assert bank_push(cap=chunk - 1) == EINVAL and 'out holds' in _msg(emu_ctx)
    assert bank_push(cap=-1) == EINVAL
    assert dll.ry_outgate_bank_reset(k, 2) == EINVAL and dll.ry_outgate_bank_held(k, 2) < 0 and dll.ry_outgate_bank_reset(None, 0) == ESTATE
    assert (oo == -99).all() and (sil == -99).all() and (out2 == -7.25).all()
    assert dll.ry_outgate_bank_held(k, 0) == 0 and dll.ry_outgate_bank_held(k, 1) == 0
    assert bank_push() == 0
    assert list(oo) == [0, 0, chunk] and list(sil) == [-1, 0] and dll.ry_outgate_bank_held(k, 0) == 500
    lone = R.Gate(chunk, C.THRESHOLD, K.SCALE)
    want, rec = lone.push(x[500:500 + chunk])
    assert out2[:chunk].tobytes() == want.tobytes() and (out2[chunk:] == -7.25).all()
    dll.ry_outgate_bank_destroy(k)
    dll.ry_outgate_bank_destroy(None)


def test_foreign_context_is_not_used(emu_ctx, monkeypatch):
    """A context made by another process is not passed to the C ABI: the engine's context of this process is taken."""
    asked = []
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: asked.append(device) or emu_ctx)
    foreign = types.SimpleNamespace(pid=os.getpid() + 1, lib=None, handle=None)
    g = OutputGate(1025, C.THRESHOLD, ctx=foreign)
    g.push(C.signal('sine', 1025))
    assert g._ctx is emu_ctx and asked == [g.device] and g.last[:2] == (True, False)
    g.close()


def test_silent_chunk_leaves_out_untouched_and_counts(emu_ctx):
    """Waits and bytes on a warm handle: no chunk -- no wait; a silent chunk -- one wait, no sample byte; an audible one -- two waits, the chunk."""
    dll = emu_ctx.lib.dll
    chunk = 2048
    h = _raw(emu_ctx, chunk, f32=1)
    out = numpy.full(chunk, -7.25, numpy.float32)
    n_out, silent, mean = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    counts = (ctypes.c_longlong * 5)()

    def push(x):
        x = numpy.ascontiguousarray(x)
        emu_ctx.lib.check(dll.ry_outgate_push(h, x.ctypes.data_as(_DP), x.size, 0, out.ctypes.data_as(ctypes.c_void_p), chunk, ctypes.byref(n_out),
                                              ctypes.byref(silent), ctypes.byref(mean)))
        emu_ctx.lib.check(dll.ry_outgate_debug_counts(h, counts))
        return list(counts)
    quiet, loud = C.signal('noise1e-6', chunk), C.signal('voiced', chunk)
    for _ in range(3):                                              # both fragment buffers and every scratch buffer have their size
        push(quiet)
    assert push(quiet) == [1, 4, 1, 1, 0] and n_out.value == chunk and silent.value == 1 and (out == -7.25).all()
    assert push(quiet[:100]) == [0, 1, 1, 0, 0] and n_out.value == 0
    assert push(quiet[:chunk - 100]) == [1, 4, 1, 1, 0] and silent.value == 1 and (out == -7.25).all()
    assert push(loud) == [2, 4, 1, 2, chunk * 4] and silent.value == 0 and n_out.value == chunk
    assert out.tobytes() == (loud * K.SCALE).astype(numpy.float32).tobytes()
    dll.ry_outgate_destroy(h)
