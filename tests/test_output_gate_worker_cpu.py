"""The output gate where it is used, on the emulator: `worker.decode_worker` in a thread on `queue.Queue`s over the reference's own `DecodeStream` /
`StreamWrapper` (tests/stubs for what they import) against the reference bookkeeping (output_gate_ref.Gate) over `world_synth.decode_realtime` output,
and `Pipeline.push(out_gate=...)` / `PipelineBank.push(out_gate=...)` against `push` followed by a lone gate.  The pipelines run on waves of a few
frames (the emulator runs the networks at about ten frames a second), so their gates have a chunk below 1025 samples and take the host expression:
what is checked there is the plumbing; the device gate is held to the reference in test_output_gate_cpu.py."""
import importlib
import queue
import sys
import threading
from pathlib import Path

import numpy
import pytest

import output_gate_checks as K
import output_gate_ref as R
import pipeline_cases as P
import reference_checkout
import test_world_synth_cpu as WS
from realtime_yukarin_amd import compat, engine, pipeline, world_analysis, world_synth
from realtime_yukarin_amd.output_gate import OutputGate, OutputGateBank

ROOT = Path(__file__).resolve().parent.parent
REF = reference_checkout.locate(Path('/root/reference'))


@pytest.fixture
def on_emulator(emu_ctx, monkeypatch):
    monkeypatch.setattr(engine, 'get_context', lambda device=0, lib=None: emu_ctx)
    monkeypatch.setattr(world_analysis.engine_for_tests, 'ctx', emu_ctx)
    monkeypatch.setattr(world_synth.engine_for_tests, 'ctx', emu_ctx)
    return emu_ctx


class _Param(object):
    frame_period = 5.0
    order = 8


@pytest.mark.skipif(REF is None, reason=reference_checkout.SKIP_REASON)
def test_decode_worker_equals_the_reference_bookkeeping(on_emulator, monkeypatch):
    """Items in, items out: the chunk / None sequence of decode_worker.py:53-61 over the samples `decode_realtime` returns; None ends the loop."""
    compat.install()
    for p in (str(ROOT / 'tests' / 'stubs'), str(REF)):
        monkeypatch.syspath_prepend(p)
    st_mod = importlib.import_module('realtime_voice_conversion.stream')
    util = importlib.import_module('realtime_voice_conversion.worker.utility')
    from realtime_yukarin_amd import worker
    monkeypatch.setattr(WS.RealtimeVocoder, 'decode', world_synth.decode_realtime)
    monkeypatch.setattr(WS.RealtimeVocoder, 'create_synthesizer', world_synth.create_synthesizer)
    fs, frames, n_items = 24000, 20, 7
    time_length, extra_time, chunk, threshold = 0.1, 0.02, 4096, 80.0
    feats = [WS._feature(frames, fs) for _ in range(n_items)]
    try:
        # the reference's loop body inline, its tail restated
        voc = WS.RealtimeVocoder(_Param(), fs)
        voc.create_synthesizer(buffer_size=1024, number_of_pointers=16)
        stream = st_mod.DecodeStream(vocoder=voc)
        wrapper = st_mod.StreamWrapper(stream=stream, extra_time=extra_time)
        ref, want, start_time = R.Gate(chunk, threshold), [], extra_time
        for f in feats:
            stream.add(start_time=start_time, data=f)
            start_time += time_length
            want.append(ref.push(wrapper.process_next(time_length=time_length))[0])
        voc._synthesizer.close()
        assert sum(w is not None for w in want) >= 2 and want[0] is None

        voc2 = WS.RealtimeVocoder(_Param(), fs)
        q_in, q_out = queue.Queue(), queue.Queue()
        lock = threading.Lock(); lock.acquire()
        t = threading.Thread(target=worker.decode_worker, args=(voc2, time_length, extra_time, 1024, chunk, threshold, q_in, q_out, lock), daemon=True)
        t.start()
        for i, f in enumerate(feats):
            q_in.put(util.Item(item=f, index=i))
            got = q_out.get(timeout=300)
            assert got.index == i and K.same_chunk(got.item, want[i]), i
        q_in.put(None)
        t.join(timeout=30)
        assert not t.is_alive() and not lock.locked()
        assert len(stream.stream) == n_items                        # the reference never trims; the mirror's stream is its own and is trimmed
        voc2._synthesizer.close()
    finally:
        for m in [k for k in sys.modules if k.startswith('realtime_voice_conversion')]:
            sys.modules.pop(m)


@pytest.fixture
def process(on_emulator, monkeypatch, tmp_path):
    shim = P.set_up(monkeypatch, tmp_path, 1)
    yield on_emulator
    P.close_shim(shim)


def short_wave(fs, seed=0):
    x = P.wave_of('loud', fs, 0.02, seed)
    x[x.size // 2:] *= numpy.float32(1e-5)
    return x


def test_pipeline_push_through_a_gate(process, tmp_path):
    """`push(..., out_gate=g)` returns what a lone gate makes of `push(...)`'s samples; without the argument `push` returns those samples."""
    from yukarin import Wave
    fs, chunk = 16000, 128
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    param = vc.acoustic_converter.config.dataset.acoustic_param
    plain, gated = pipeline.Pipeline(vc, param, crepe_capacity=1, seed=3), pipeline.Pipeline(vc, param, crepe_capacity=1, seed=3)
    g, lone = OutputGate(chunk, 200.0, 0.5, numpy.float32), R.Gate(chunk, 200.0, 0.5, numpy.float32)      # -200 dB: below the floor of the expression, every chunk is audible
    emitted = 0
    for r, final in enumerate((False, False, True)):
        w = Wave(short_wave(fs, r), fs)
        a = plain.push(w, (0, 0), final=final)
        b = gated.push(w, (0, 0), final=final, out_gate=g)
        assert a.wave.dtype == numpy.float64 and b.sampling_rate == a.sampling_rate
        want, rec = lone.push(a.wave)
        if want is None:
            assert b.wave.size == 0 and b.wave.dtype == numpy.float32
        else:
            assert K.same_chunk(b.wave, want)
            emitted += 1
        assert g.last[:2] == rec[:2] and g.held() == len(lone.fragment)
    assert emitted >= 1
    for p in (plain, gated):
        p.close()
    P.close_voice_changer(vc)


def test_pipeline_bank_push_through_a_gate_bank(process, tmp_path):
    from yukarin import Wave
    fs, chunk, seeds = 16000, 128, [3, 4]
    vc = P.voice_changer(P.write_models(tmp_path, fs), fs)
    param = vc.acoustic_converter.config.dataset.acoustic_param
    plain, gated = (pipeline.PipelineBank(vc, param, 2, seeds=seeds, crepe_capacity=1) for _ in range(2))
    gates, lone = OutputGateBank(2, chunk, 200.0), [R.Gate(chunk, 200.0) for _ in seeds]
    rounds = [([0, 1], ()), ([None, 2], ()), ([3, 4], (0, 1))]
    emitted = 0
    for picks, final in rounds:
        waves = [Wave(short_wave(fs, s), fs) if s is not None else None for s in picks]
        a = plain.push(waves, (0, 0), final=final)
        b = gated.push(waves, (0, 0), final=final, out_gate=gates)
        for s in range(2):
            if a[s].wave.size == 0:                                 # no sample: the stream sits the gates' call out
                assert b[s].wave.size == 0
                continue
            want, rec = lone[s].push(a[s].wave)
            assert (b[s].wave.size == 0) if want is None else K.same_chunk(b[s].wave, want)
            assert gates.last[s][:2] == rec[:2] and gates.held(s) == len(lone[s].fragment)
            emitted += want is not None
    assert emitted >= 2
    for p in (plain, gated):
        p.close()
    P.close_voice_changer(vc)
