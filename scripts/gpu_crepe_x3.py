#!/usr/bin/env python3
"""The split-bf16 mode of the CREPE network (`CrepeModel.set_dtype('bf16x3')`) against the fp32 path at 'full' capacity on one MI355X, in one
process: median milliseconds of 30 device-synchronised `predict` calls on 1 s and 0.5 s of audio at 16 kHz and at 24 kHz with a 5 ms step, in
'f32' and in 'bf16x3' on the same handle, the largest |activation| difference between the two, and whether the 4.8 ms of the 100x target
 is met.  Prints one JSON object and, with --out, writes it.  Seeded synthetic weights (no trained ones exist here).

    python scripts/gpu_crepe_x3.py [--reps 30] [--out FILE]      the measurement, as a child process under its own `timeout`
    python scripts/gpu_crepe_x3.py --child --trace               five 1-s calls at 24 kHz per mode, for `rocprofv3 --kernel-trace --stats -- ...`
    python scripts/gpu_crepe_x3.py --summary DB_GLOB OUT         per-kernel table of that run: each layer's time in both modes, its share of the
                                                                 fp32 MFMA peak (crepe_igemm) or of the 2.5 PFLOP/s bf16 peak on the three
                                                                 products it executes (crepe_igemm_x3)
"""
import argparse
import glob
import json
import sqlite3
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'scripts'))

import numpy  # noqa: E402

from gpu_crepe import PEAK_FP32_MFMA, layer_flops  # noqa: E402
from gpu_crepe_resample import signal, timed  # noqa: E402

PEAK_BF16_MFMA = 2.5e15
STEP_MS = 5
LIMIT_S = 300
TARGET_MS = 4.8                 # 100x real time for 1 s at 24 kHz beside the other stages


def run(args):
    from realtime_yukarin_amd import crepe, engine
    ctx = engine.get_context(0)
    hop = crepe.hop_length(STEP_MS)
    model = crepe.CrepeModel('full', crepe.synthetic_params('full', 0), ctx=ctx)
    if args.trace:
        x = signal(24000, 24000)
        for dtype in ('f32', 'bf16x3'):
            model.set_dtype(dtype)
            for _ in range(5):
                model.predict(x, 24000, hop)
        print(json.dumps({'trace_calls_per_mode': 5, 'frames': crepe.n_frames(16000, hop)}))
        return 0
    res = {'capacity': 'full', 'step_ms': STEP_MS, 'reps': args.reps, 'target_ms_1s_24k': TARGET_MS}
    acts = {}
    for dtype in ('f32', 'bf16x3', 'f32_again'):
        model.set_dtype(dtype.split('_')[0])
        res['splits_' + dtype] = model.splits()
        for sec in (1.0, 0.5):
            for sr in (16000, 24000):
                x = signal(int(sr * sec), sr)
                for _ in range(3):
                    out = model.predict(x, sr, hop)
                acts[(dtype, sec, sr)] = out[2]
                k = 'ms_%s_%dk_%gs' % (dtype, sr // 1000, sec)
                res[k], res[k + '_min'] = timed(lambda: model.predict(x, sr, hop), args.reps)
    res['f32_bits_unchanged_by_the_switch'] = bool(all(numpy.array_equal(acts[('f32', s, r)], acts[('f32_again', s, r)]) for s in (1.0, 0.5) for r in (16000, 24000)))
    res['max_abs_act_difference'] = float(max(numpy.abs(acts[('f32', s, r)].astype('f8') - acts[('bf16x3', s, r)]).max() for s in (1.0, 0.5) for r in (16000, 24000)))
    res['x3_over_f32_1s_24k'] = round(res['ms_bf16x3_24k_1s'] / res['ms_f32_24k_1s'], 3)
    res['x3_over_f32_1s_16k'] = round(res['ms_bf16x3_16k_1s'] / res['ms_f32_16k_1s'], 3)
    res['bf16x3_faster_than_f32_1s'] = bool(res['ms_bf16x3_24k_1s'] < res['ms_f32_24k_1s'] and res['ms_bf16x3_16k_1s'] < res['ms_f32_16k_1s'])
    res['target_met_f32'] = bool(res['ms_f32_24k_1s'] <= TARGET_MS)
    res['target_met_bf16x3'] = bool(res['ms_bf16x3_24k_1s'] <= TARGET_MS)
    model.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + '\n')
    return 0 if res['f32_bits_unchanged_by_the_switch'] else 1


def summary(db_glob, out_path):
    """Per-kernel averages from the rocpd database of the --trace run; for the layer GEMMs the share of the pipe's peak on executed FLOPs at 201 frames."""
    db = sorted(glob.glob(db_glob, recursive=True))[0]
    rows = list(sqlite3.connect(db).cursor().execute('select name, total_calls, total_duration, average, percentage from top_kernels'))
    fl = dict(layer_flops())
    names = ['conv1', 'conv2', 'conv3', 'conv4', 'conv5', 'conv6', 'dense']
    lines = ['# rocprofv3 --kernel-trace --stats -- python scripts/gpu_crepe_x3.py --child --trace  (full capacity, 1 s at 24 kHz = 201 frames, 5 calls in f32,',
             '# then 5 in bf16x3 on the same handle); durations in microseconds; share = executed FLOPs / (avg x peak): crepe_igemm on 157.3 TFLOP/s (fp32 MFMA),',
             '# crepe_igemm_x3 three products per FLOP pair on 2.5 PFLOP/s (bf16 MFMA)',
             '%-60s %6s %12s %10s %8s %8s' % ('kernel', 'calls', 'total_us', 'avg_us', 'pct', 'share')]
    layer_us = {}
    for name, calls, total, avg, pct in rows:
        share = ''
        for fam, peak, mult in (('crepe_igemm_x3<', PEAK_BF16_MFMA, 3.0), ('crepe_igemm<', PEAK_FP32_MFMA, 1.0)):
            if fam in name:
                layer = int(name.split(fam)[1].split(',')[1].split('>')[0])
                share = '%.3f' % (mult * fl[names[layer - 1]] / (avg * 1e-6 * peak))
                layer_us[(names[layer - 1], fam)] = avg
        lines.append('%-60s %6d %12.1f %10.2f %8.2f %8s' % (name[:60], calls, total, avg, pct, share))
    lines.append('# per layer, average microseconds of the GEMM kernel: f32 -> bf16x3')
    for n in names:
        a, b = layer_us.get((n, 'crepe_igemm<')), layer_us.get((n, 'crepe_igemm_x3<'))
        if a and b:
            lines.append('%-6s %10.2f -> %10.2f   (x %.2f)' % (n, a, b, b / a))
    Path(out_path).write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default='')
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--summary', nargs=2, metavar=('DB_GLOB', 'OUT'))
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    a = ap.parse_args()
    if a.summary:
        summary(*a.summary)
        sys.exit(0)
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps)] + (['--out', a.out] if a.out else [])
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
