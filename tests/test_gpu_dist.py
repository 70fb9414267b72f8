"""The N > 1 path on the ONE GPU a test box has: a one-rank process group over RCCL ("nccl" backend of torch.distributed, and the
C-ABI transport ry_comm_*), the weight broadcast, the adoption of the broadcast buffer by ry_net_create, barrier and max -- i.e. real
RCCL initialisation and the real library load order next to libry355.so; then bench.py's own --force-dist mode through both
transports.  (Multi-rank RCCL needs one GPU per rank and cannot run here; the multi-rank logic is covered with gloo on the CPU,
tests/test_dist_cpu.py.)  Ordering contract of the reference: results are re-ordered by Item.index, /root/reference/run.py:171-183."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _run(code_or_args, env_extra=None, timeout=600):
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.update(env_extra or {})
    r = subprocess.run([sys.executable] + code_or_args, cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + '\n' + r.stderr[-4000:]
    return r.stdout


ONE_RANK = r'''
import sys, numpy
sys.path.insert(0, %r)
import torch
from realtime_yukarin_amd import dist as rdist, engine, synth
from realtime_yukarin_amd.weights import synthetic_params
kind = sys.argv[1]
torch.cuda.set_device(0)
ctx = engine.get_context(0)
comm = rdist.NativeComm(ctx, 0, 1) if kind == 'native' else rdist.TorchComm('nccl', 0, 1, torch.device('cuda', 0))
d1, d2 = synth.model_descs('SYN-8')
P1 = synthetic_params(d1, 31)
net = comm.broadcast_net(ctx, d1, P1)
comm.barrier()
assert comm.max(2.5) == 2.5
x = synth.stage1_input(100)[0]
y = net.convert(x)
from oracle import torch_ref
r = torch_ref.stage1_convert_core(torch_ref.TorchUNet(P1), x)
err = float(numpy.abs(y - r).max() / numpy.abs(r).max())
print('RESULT', comm.kind, err)
assert err < 1e-4
net.close(); comm.close()
''' % str(ROOT)


@pytest.mark.parametrize('kind', ['torch', 'native'])
def test_one_rank_rccl_broadcast_and_adoption(kind):
    out = _run(['-c', ONE_RANK, kind], {'MASTER_PORT': '29611' if kind == 'torch' else '29612'})
    assert 'RESULT' in out


@pytest.mark.parametrize('comm', ['torch', 'native'])
def test_bench_force_dist(comm):
    """bench.py through its `comm is not None` branches on one GPU, at the DRIVER'S step count (--steps 20 --warmup 5): same JSON contract,
    the headline where the plain run has it (round 3's driver line was 130 k frames/s from one unrepeated bracket with a garbage collection
    inside, and this test asked for 50 k at --steps 10: it would not have noticed)."""
    out = _run(['bench.py', '--full', '--force-dist', '--comm', comm, '--steps', '20', '--warmup', '5', '--no-cpu-baseline', '--no-extras'],
               {'MASTER_PORT': '29613' if comm == 'torch' else '29614', 'RANK': '0', 'LOCAL_RANK': '0', 'WORLD_SIZE': '1'})
    d = json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1])
    assert d['n_gpus'] == 1 and d['comm'] is not None and d['value'] > 200000 and d['dtype'] == 'f32'
    assert d['roofline']['frac'] > 0.45 and d['config']['frames'] == 300               # (round 6: on EXECUTED MFMA FLOPs -- the Winograd family sits at 0.57)
    # a bracket of 20 steps is 16 ms since round 6: the first one behind the warm-up runs 4 - 12 % slower than the others (profiles/r06/driver_cmd.txt), the median does not see it
    assert d['repeats'] >= 5 and len(d['brackets']) == d['repeats'] and d['slow_brackets'] == [] and d['spread'] < 0.20


def test_bench_at_the_drivers_own_command():
    """`python3 bench.py --gpus 1 --steps 20 --warmup 5` (what the driver runs at round end) in a fresh process: the printed line is short
    enough for an 8 KB tail, carries every bracket, and the brackets agree with each other."""
    out = _run(['bench.py', '--full', '--gpus', '1', '--steps', '20', '--warmup', '5', '--no-extras', '--cpu-seconds', '2'])
    line = [ln for ln in out.splitlines() if ln.startswith('{')][-1]
    d = json.loads(line)
    assert len(line) < 6144, len(line)
    assert d['steps'] == 20 and d['warmup'] == 5 and d['value'] > 0 and d['value_from'] == 'median bracket' and len(d['brackets']) == 7
    assert d['cpu_baseline']['gpu_result_vs_this_baseline']['sp_max_rel'] < 1e-4 and 0.0 < d['roofline']['frac'] < 1.0
    if os.environ.get('RY_TEST_PERF'):            # absolute speed and timing agreement: an idle MI355X only (round-4 advisor: a co-tenant or another
        walls = sorted(b['wall_ms'] for b in d['brackets'])      # clock state must not turn the correctness suite red) -- RY_TEST_PERF=1 opts in
        assert d['value'] > 200000 and d['roofline']['frac'] > 0.5
        assert d['slow_brackets'] == [] and walls[-1] < 1.10 * walls[0], d['brackets']
        assert abs(d['device_ms_per_step_rank0'] - d['ms_per_step']) < 0.05 * d['ms_per_step']


def test_plain_bench_times_exactly_k_steps_and_dumps_its_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` is the headline alone: one bracket of exactly K steps and none of the measurements
    of --full; `--dump-outputs` writes the mc / sp blocks of the last timed step as float32 arrays."""
    out = _run(['bench.py', '--gpus', '1', '--steps', '30', '--warmup', '5', '--dump-outputs', str(tmp_path / 'dump')])
    d = json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1])
    assert d['steps'] == 30 and d['repeats'] == 1 and len(d['brackets']) == 1 and d['value'] > 0 and d['dtype'] == 'f32'
    assert abs(d['brackets'][0]['wall_ms'] / 30 - d['ms_per_step']) < 1e-3
    assert not set(d) & {'mixed_stream', 'roofline', 'cpu_baseline', 'graph_replay_ms', 'host_path', 'split_bf16'}, sorted(d)
    sp, mc = (numpy.load(str(tmp_path / 'dump' / (k + '.npy'))) for k in ('sp', 'mc'))
    assert sp.dtype == mc.dtype == numpy.float32 and sp.shape == (1, 300, 513) and mc.shape[:2] == (1, 300)
    assert numpy.isfinite(sp).all() and (sp > 0).all() and numpy.isfinite(mc).all()
