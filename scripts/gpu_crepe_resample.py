#!/usr/bin/env python3
"""The device resampler of the CREPE path at 'full' capacity on one MI355X: median milliseconds of device-synchronised calls on 1 s of audio at
24 kHz and at 48 kHz -- the resampler alone (`CrepeModel.resample`: upload, kernel, download; and with device pointers, the kernel and a sync),
`CrepeModel.predict` at the rate, and in the same process the path it replaces (`crepe.resample` on the host, then `predict16k`).  Checks that
both paths return the same bits, prints one JSON object and, with --out, writes it.  Seeded synthetic weights (no trained ones exist here).

    python scripts/gpu_crepe_resample.py [--reps 30] [--out FILE]      the measurement, as a child process under its own `timeout`
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy  # noqa: E402

STEP_MS = 5
LIMIT_S = 300


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
    return round(float(numpy.median(ts)), 4), round(float(numpy.min(ts)), 4)


def run(args):
    from realtime_yukarin_amd import _lib, crepe, engine
    ctx = engine.get_context(0)
    hop = crepe.hop_length(STEP_MS)
    model = crepe.CrepeModel('full', crepe.synthetic_params('full', 0), ctx=ctx)
    lib, h = model._get()
    res = {'capacity': 'full', 'step_ms': STEP_MS, 'reps': args.reps, 'seconds': 1.0}
    for sr in (24000, 48000):
        x = signal(sr, sr)
        k = '%dk' % (sr // 1000)
        y_host = crepe.resample(x, sr)
        new, old = model.predict(x, sr, hop), model.predict16k(y_host, hop)
        res['bits_equal_' + k] = bool(numpy.array_equal(model.resample(x, sr), y_host) and all(numpy.array_equal(a, b) for a, b in zip(new, old)))
        for _ in range(3):
            model.predict(x, sr, hop)
            model.resample(x, sr)
        res['ms_resample_%s' % k], res['ms_resample_%s_min' % k] = timed(lambda: model.resample(x, sr), args.reps)
        d_in, d_out = ctx.dev_alloc(x.size), ctx.dev_alloc(y_host.size)
        try:
            ctx.dev_upload(d_in, x)
            ctx.sync()

            def on_device():
                lib.check(lib.dll.ry_crepe_resample(h, _lib._fptr(d_in), x.size, sr, _lib._fptr(d_out), 1))
                ctx.sync()
            on_device()
            res['ms_resample_%s_device_pointers' % k], res['ms_resample_%s_device_pointers_min' % k] = timed(on_device, args.reps)
        finally:
            ctx.dev_free(d_in); ctx.dev_free(d_out)
        res['ms_predict_%s' % k], res['ms_predict_%s_min' % k] = timed(lambda: model.predict(x, sr, hop), args.reps)
        res['ms_host_path_%s' % k], res['ms_host_path_%s_min' % k] = timed(lambda: model.predict16k(crepe.resample(x, sr), hop), args.reps)
        res['ms_host_resample_%s' % k], _ = timed(lambda: crepe.resample(x, sr), args.reps)
        res['ms_predict16k_%s' % k], _ = timed(lambda: model.predict16k(y_host, hop), args.reps)
        res['host_path_over_predict_%s' % k] = round(res['ms_host_path_%s' % k] / res['ms_predict_%s' % k], 2)
    res['predict_24k_faster_than_host_path'] = bool(res['ms_predict_24k'] < res['ms_host_path_24k'])
    model.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + '\n')
    return 0 if res['bits_equal_24k'] and res['bits_equal_48k'] and res['predict_24k_faster_than_host_path'] else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default='')
    ap.add_argument('--child', action='store_true', help='the measurement itself (the default starts it under `timeout`)')
    a = ap.parse_args()
    if a.child:
        sys.exit(run(a))
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), '--child', '--reps', str(a.reps)] + (['--out', a.out] if a.out else [])
    sys.exit(subprocess.run(cmd, cwd=str(ROOT)).returncode)
