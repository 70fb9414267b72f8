"""CPU: the error bar of tests/test_world_synth_gpu.py.  The synthesis kernels run float64 butterflies, so the bar is 4 x the error of the numpy float64
restatement (tests/world_synth_ref.py) against the same restatement in numpy.longdouble, max |y - ref| / max |ref|, worst over the inputs of the GPU test
(tests/world_synth_cases.py).  Writes profiles/r08/synth_tolerance.txt.  `--float32` adds the float32-against-float64 figure (what fp32 butterflies
would be held to), on the short inputs only.

    python scripts/synth_tolerance.py [--jobs 8] [--float32]"""
import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]


def one(job):
    import world_synth_cases as C
    import world_synth_ref as R
    kind, n, fs, apm, dt = job
    f0, sp, ap = C.case(kind, n, fs, apm)
    hi = numpy.longdouble if dt == 'f64' else numpy.float64
    lo = numpy.float64 if dt == 'f64' else numpy.float32
    ref = R.synthesize(f0, sp, ap, fs, 5.0, seed=1, dtype=hi)
    y = R.synthesize(f0, sp, ap, fs, 5.0, seed=1, dtype=lo)
    den = float(numpy.abs(ref).max())
    return job, (float(numpy.abs(y.astype(hi) - ref).max()) / den if den > 0 else 0.0)


def main():
    import world_synth_cases as C
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, default=8)
    ap.add_argument('--float32', action='store_true')
    a = ap.parse_args()
    jobs = [(k, n, fs, 'mixed', 'f64') for fs in C.RATES for n in C.LENGTHS for k in C.TRACKS]
    jobs += [('glide', 300, fs, m, 'f64') for fs in C.RATES for m in ('floor', 'ceil', 'clamps')]
    if a.float32:
        jobs += [(k, 300, fs, 'mixed', 'f32') for fs in C.RATES for k in C.TRACKS]
    with Pool(a.jobs) as pool:
        res = pool.map(one, jobs, chunksize=1)
    lines = ['# numpy %s; max |y - ref| / max |ref| of the restatement, float64 against longdouble (eps %.3g)' % (numpy.__version__, numpy.finfo(numpy.longdouble).eps)]
    for (k, n, fs, m, dt), e in res:
        lines.append('%s %-10s fs=%5d frames=%4d ap=%-6s %.4g' % (dt, k, fs, n, m, e))
    w64 = max(e for (k, n, fs, m, dt), e in res if dt == 'f64')
    lines.append('worst float64-vs-longdouble %.6g' % w64)
    lines.append('bar = 4 x worst = %.6g' % (4 * w64))
    if a.float32:
        lines.append('worst float32-vs-float64 (300 frames) %.6g' % max(e for (k, n, fs, m, dt), e in res if dt == 'f32'))
    out = ROOT / 'profiles' / 'r08' / 'synth_tolerance.txt'
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines[-3:]))


if __name__ == '__main__':
    main()
