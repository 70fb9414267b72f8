#!/usr/bin/env python3
"""CREPE at 'full' capacity on one MI355X: device-synchronised milliseconds per `predict` (host call that returns the f0 / confidence /
activation arrays) for 0.5 s and 1 s of audio (101 / 201 frames at 5 ms) at 16 kHz and at 24 kHz (host float64 resampling included and
reported on its own), the torch CPU fp32 restatement of the network on the same host (16 threads), and the real-time factors.  Prints one
JSON line.  Seeded synthetic weights (no trained ones exist here).

    python scripts/gpu_crepe.py [--reps 20] [--no-cpu]        timing
    python scripts/gpu_crepe.py --profile                       a few 1-s calls only, for `rocprofv3 --kernel-trace --stats -- ...`
    python scripts/gpu_crepe.py --summary DB_GLOB OUT           per-kernel table of a rocprofv3 run + each layer's share of the fp32 MFMA peak
"""
import argparse
import glob
import json
import sqlite3
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import numpy  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
STEP_MS = 5
PLAN_FRAMES = 201


def layer_flops(m=32, frames=PLAN_FRAMES):
    """Algorithmic (= executed: the implicit GEMM computes no padding products beyond the 'same' zeros) FLOPs per layer."""
    from realtime_yukarin_amd import crepe
    out, cin, L = [], 1, 1024
    for i, (c, w, s) in enumerate(zip(crepe.channels(m), crepe.WIDTHS, crepe.STRIDES)):
        lout = L // s
        out.append(('conv%d' % (i + 1), 2.0 * frames * lout * c * cin * w))
        cin, L = c, lout // 2
    out.append(('dense', 2.0 * frames * 360 * 4 * cin))
    return out


def signal(n, sr, seed=0):
    rng = numpy.random.default_rng(seed)
    t = numpy.arange(n) / sr
    f = 180 + 50 * numpy.sin(2 * numpy.pi * t)
    return (0.3 * numpy.sin(2 * numpy.pi * numpy.cumsum(f) / sr) + rng.normal(0, 0.02, n)).astype(numpy.float32)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(numpy.median(ts)), float(numpy.min(ts))


def run(args):
    from realtime_yukarin_amd import crepe, engine
    hop = crepe.hop_length(STEP_MS)
    model = crepe.CrepeModel('full', crepe.synthetic_params('full', 0), ctx=engine.get_context(0))
    res = {'capacity': 'full', 'step_ms': STEP_MS, 'reps': args.reps}
    if args.profile:
        x = signal(16000, 16000)
        for _ in range(5):
            model.predict16k(x, hop)
        print(json.dumps({'profile_calls': 5, 'frames': crepe.n_frames(16000, hop)}))
        return
    res['splits'] = model.splits()
    for sec in (0.5, 1.0):
        x = signal(int(16000 * sec), 16000)
        n = crepe.n_frames(len(x), hop)
        for _ in range(3):
            model.predict16k(x, hop)
        med, mn = timed(lambda: model.predict16k(x, hop), args.reps)
        res['ms_16k_%gs' % sec] = round(med, 3)
        res['ms_16k_%gs_min' % sec] = round(mn, 3)
        res['frames_%gs' % sec] = n
        x24 = signal(int(24000 * sec), 24000)
        rs_med, _ = timed(lambda: crepe.resample(x24, 24000), max(3, args.reps // 4))
        x16 = crepe.resample(x24, 24000)
        dev_med, _ = timed(lambda: model.predict16k(x16, hop), args.reps)
        res['ms_24k_%gs' % sec] = round(rs_med + dev_med, 3)
        res['ms_24k_%gs_resample_host' % sec] = round(rs_med, 3)
        res['ms_24k_%gs_device_call' % sec] = round(dev_med, 3)
    res['rtf_16k_1s'] = round(res['ms_16k_1s'] / 1000.0, 5)
    res['rtf_24k_1s'] = round(res['ms_24k_1s'] / 1000.0, 5)
    fl = layer_flops()
    res['gflop_1s'] = round(sum(f for _, f in fl) / 1e9, 2)
    res['floor_ms_1s'] = round(sum(f for _, f in fl) / PEAK_FP32_MFMA * 1e3, 3)
    res['whole_call_frac_of_peak'] = round(res['floor_ms_1s'] / res['ms_16k_1s'], 3)
    if not args.no_cpu:
        import torch
        import crepe_ref
        torch.set_num_threads(16)
        P = crepe.synthetic_params('full', 0)
        x = signal(16000, 16000)
        fr = crepe_ref.frames(x, hop).astype(numpy.float32)
        Pt = {k: v for k, v in P.items()}

        def cpu():
            with torch.no_grad():
                xt = torch.from_numpy(fr)[:, None, :]
                for i in range(6):
                    k = 'conv%d' % (i + 1)
                    xt = torch.nn.functional.pad(xt, crepe.PADS[i])
                    xt = torch.nn.functional.conv1d(xt, torch.from_numpy(Pt[k + '.weight']), torch.from_numpy(Pt[k + '.bias']), stride=crepe.STRIDES[i])
                    xt = torch.relu(xt)
                    b = k + '_BN.'
                    xt = torch.nn.functional.batch_norm(xt, torch.from_numpy(Pt[b + 'running_mean']), torch.from_numpy(Pt[b + 'running_var']),
                                                        torch.from_numpy(Pt[b + 'weight']), torch.from_numpy(Pt[b + 'bias']), False, 0.0, crepe.BN_EPS)
                    xt = torch.nn.functional.max_pool1d(xt, 2)
                flat = xt.permute(0, 2, 1).reshape(xt.shape[0], -1)
                return torch.sigmoid(flat @ torch.from_numpy(Pt['classifier.weight']).T + torch.from_numpy(Pt['classifier.bias']))
        cpu()
        med, mn = timed(cpu, 3)
        res['cpu_torch_fp32_16t_ms_1s'] = round(med, 1)
        res['speedup_vs_cpu_1s'] = round(med / res['ms_16k_1s'], 1)
    print(json.dumps(res))


def summary(db_glob, out_path):
    """Per-kernel averages from the rocpd database of `rocprofv3 --kernel-trace --stats` and, for the layer GEMMs (one instantiation per
    layer: crepe_igemm<epilogue, layer>), the share of the fp32 MFMA peak on executed FLOPs at 201 frames.  A split layer's reduction
    kernel (crepe_reduce_*) is listed separately."""
    db = sorted(glob.glob(db_glob, recursive=True))[0]
    rows = list(sqlite3.connect(db).cursor().execute('select name, total_calls, total_duration, average, percentage from top_kernels'))
    fl = dict(layer_flops())
    names = ['conv1', 'conv2', 'conv3', 'conv4', 'conv5', 'conv6', 'dense']
    lines = ['# rocprofv3 --kernel-trace --stats -- python scripts/gpu_crepe.py --profile  (full capacity, 1 s at 16 kHz = 201 frames,',
             '# 5 calls, the first of which also builds the device model); durations in microseconds; share = executed FLOPs / (avg x 157.3 TFLOP/s)',
             '%-60s %6s %12s %10s %8s %8s' % ('kernel', 'calls', 'total_us', 'avg_us', 'pct', 'share')]
    for name, calls, total, avg, pct in rows:
        share = ''
        if 'crepe_igemm<' in name:
            layer = int(name.split('crepe_igemm<')[1].split(',')[1].split('>')[0])
            share = '%.3f' % (fl[names[layer - 1]] / (avg * 1e-6 * PEAK_FP32_MFMA))
        lines.append('%-60s %6d %12.1f %10.2f %8.2f %8s' % (name[:60], calls, total, avg, pct, share))
    Path(out_path).write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--summary', nargs=2, metavar=('DB_GLOB', 'OUT'))
    a = ap.parse_args()
    if a.summary:
        summary(*a.summary)
    else:
        run(a)
