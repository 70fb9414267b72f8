"""N > 1 path on CPU: two gloo processes, weights broadcast from rank 0, windows sharded round robin, each rank
converting on the emulator build of the kernels, results gathered in window order and checked against the oracle."""
import os
import socket
import sys
from pathlib import Path

import numpy
import pytest
import torch
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent
N_WINDOWS = 5


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, str(ROOT))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from realtime_yukarin_amd import _lib, build, dist as rdist, engine, synth
    from realtime_yukarin_amd.netspec import NetDesc
    from realtime_yukarin_amd.weights import synthetic_params
    ctx = engine.Context(0, _lib.Ry355Lib(build.EMU_LIB))
    d1, d2 = NetDesc(1, 9, 9, 8, 8), NetDesc(2, 1, 1, 8, 8)
    P1 = synthetic_params(d1, 31) if rank == 0 else None          # only rank 0 owns the weights
    P2 = synthetic_params(d2, 32) if rank == 0 else None
    dev = torch.device('cpu')
    n1 = rdist.make_net(ctx, d1, rdist.broadcast_blob(d1, P1, dev))
    n2 = rdist.make_net(ctx, d2, rdist.broadcast_blob(d2, P2, dev), width=128)
    x = synth.stage1_input(40, N_WINDOWS, seed=77)                 # every rank can see all inputs; it converts only its shard
    sp = synth.stage2_input(40, N_WINDOWS, seed=78, bins=129)
    mine = rdist.shard(N_WINDOWS)
    y1 = rdist.convert_windows(n1, [x[i] for i in mine])
    y2 = rdist.convert_windows(n2, [sp[i] for i in mine])
    g1 = rdist.gather_in_order(y1, N_WINDOWS)
    g2 = rdist.gather_in_order(y2, N_WINDOWS)
    if rank == 0:
        numpy.savez(os.path.join(out_dir, 'gathered.npz'), y1=numpy.stack(g1), y2=numpy.stack(g2), shard0=numpy.array(mine))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_chunk_parallel_convert(tmp_path):
    from realtime_yukarin_amd import build
    build.build_emu()
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    z = numpy.load(tmp_path / 'gathered.npz')
    assert list(z['shard0']) == [0, 2, 4]
    from oracle import unet
    from realtime_yukarin_amd import synth
    from realtime_yukarin_amd.netspec import NetDesc
    from realtime_yukarin_amd.weights import synthetic_params
    P1, P2 = synthetic_params(NetDesc(1, 9, 9, 8, 8), 31), synthetic_params(NetDesc(2, 1, 1, 8, 8), 32)
    x = synth.stage1_input(40, N_WINDOWS, seed=77)
    sp = synth.stage2_input(40, N_WINDOWS, seed=78, bins=129)
    for i in range(N_WINDOWS):
        r1 = unet.stage1_convert_core(x[i], P1)
        assert numpy.abs(z['y1'][i] - r1).max() / numpy.abs(r1).max() < 1e-4
        assert numpy.abs(z['y2'][i] / unet.stage2_convert(sp[i], P2) - 1).max() < 1e-4


def test_shard_is_a_partition():
    from realtime_yukarin_amd import dist as rdist
    for w in (1, 2, 4, 8):
        seen = sorted(i for r in range(w) for i in rdist.shard(11, r, w))
        assert seen == list(range(11))


def _bench_worker(rank, world, port, out_dir):
    """One rank of `bench.py --gpus 2 --emulator`: bench.py's OWN main(), launched as torch.distributed.run launches it (RANK /
    LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment)."""
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    import bench
    out = bench.main(['--gpus', str(world), '--emulator', '--frames', '24', '--steps', '1', '--warmup', '0'])
    import json
    with open(os.path.join(out_dir, 'bench_rank%d.json' % rank), 'w') as f:
        json.dump(out, f)


def test_bench_main_runs_its_distributed_branches_with_two_gloo_ranks(tmp_path):
    """The N > 1 branches of bench.py (process group, one broadcast per predictor, barrier + fence, max over the ranks of the elapsed
    time, weak-scaling aggregate) executed for real: two gloo ranks on the emulator build.  The numbers mean nothing; the plumbing is
    the thing under test, so that a blind multi-GPU run cannot fail on it."""
    import json
    from realtime_yukarin_amd import build
    build.build_emu()
    port = _free_port()
    mp.spawn(_bench_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (json.load(open(tmp_path / ('bench_rank%d.json' % r))) for r in (0, 1))
    assert r0['n_gpus'] == 2 and r0['scaling'] == 'weak' and r0['comm'] == 'torch.distributed/gloo'
    assert r0['value'] > 0 and r0['steps'] == 1 and r0['warmup'] == 0 and 'EMULATOR' in r0['data']
    assert r0['ms_per_step'] == r1['ms_per_step']                       # the maximum over the ranks, seen by both
    assert abs(r0['value'] - 2 * 1 * 24 * 1 / (r0['ms_per_step'] * 1e-3)) / r0["value"] < 5e-3   # (value is rounded to 0.1) whole-job frames / max-over-ranks time
    assert r0['config']['parallelism'].startswith('chunk-dp2')


@pytest.mark.parametrize('world', [2, 4])
def test_bench_starts_its_own_ranks_when_run_plainly(tmp_path, world):
    """Round-4 verdict: `python3 bench.py --gpus N` -- the form of the driver's 1-GPU command, no launcher -- used to exit with a usage hint.
    It now starts the N ranks itself (torch.distributed.run on a free port) and rank 0 prints the one JSON line, of the same shape as under
    the launcher."""
    import json
    import subprocess
    from realtime_yukarin_amd import build
    build.build_emu()
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, str(ROOT / 'bench.py'), '--gpus', str(world), '--emulator', '--frames', '24', '--steps', '1', '--warmup', '0', '--no-cpu-baseline',
                        '--details-out', str(tmp_path / 'details.json')], capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == world and d['comm'] == 'torch.distributed/gloo' and d['comm_ranks'] == world and d['scaling'] == 'weak'
    assert d['value'] > 0 and d['config']['parallelism'].startswith('chunk-dp%d' % world) and 'metric' in d and len(d['brackets']) >= 1
    # whole-job aggregate: `world` ranks x windows per rank x frames over the max-over-ranks time (value is rounded to 0.1)
    assert abs(d['value'] - world * d['config']['windows_per_gpu'] * 24 / (d['ms_per_step'] * 1e-3)) / d['value'] < 5e-3


def test_bench_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    """`bench.py --dump-outputs DIR` writes the mc / sp blocks of the last timed step as float32 .npy files; inputs and weights are seeded,
    so two fresh runs of one build with the same arguments write the same arrays (what lets two builds be compared output for output)."""
    import subprocess
    from realtime_yukarin_amd import build
    build.build_emu()
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    got = []
    for i in range(2):
        d = tmp_path / ('run%d' % i)
        r = subprocess.run([sys.executable, str(ROOT / 'bench.py'), '--emulator', '--frames', '24', '--steps', '2', '--warmup', '1', '--dump-outputs', str(d)],
                           capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        got.append({k: numpy.load(str(d / (k + '.npy'))) for k in ('mc', 'sp')})
    assert got[0]['mc'].shape == (1, 24, 9) and got[0]['sp'].shape == (1, 24, 513) and (got[0]['sp'] > 0).all()
    for k in ('mc', 'sp'):
        assert got[0][k].dtype == numpy.float32 and numpy.array_equal(got[0][k], got[1][k]), k
