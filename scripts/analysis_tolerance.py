"""CPU: the error bars of tests/test_world_analysis_cpu.py / _gpu.py.  The analysis kernels run float64 butterflies, so their bars are 4 x the error
of the numpy float64 restatement (tests/world_analysis_ref.py) against the same restatement in numpy.longdouble with its own transform, worst over
the inputs of the tests (tests/world_analysis_cases.py):  sp: max |log sp - log ref|;  mc: max |mc - ref| / max |ref|.  `log` near a spectral null is
ill-conditioned (the smoothing is a difference of cumulative sums), which is why the bars come from the same inputs and not from a constant.
Writes profiles/r09/analysis_tolerance.txt: the two worst figures first (the tests read lines 1 and 2), then every case.

    python scripts/analysis_tolerance.py [--jobs 8]"""
import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]


def one(job):
    import world_analysis_cases as C
    import world_analysis_ref as R
    from realtime_yukarin_amd import sptk
    wk, tk, n, fs = job
    x, f0, t = C.case(wk, tk, n, fs)
    floor = C.f0_floor(tk)
    alpha = sptk.mcepalpha(fs)
    lo = R.cheaptrick(x, f0, t, fs, f0_floor=floor, fft_size=1024, seed=C.SEED)
    hi = R.cheaptrick(x, f0, t, fs, f0_floor=floor, fft_size=1024, seed=C.SEED, dtype=numpy.longdouble)
    mlo, mhi = R.sp2mc(lo, C.ORDER, alpha), R.sp2mc(hi, C.ORDER, alpha, dtype=numpy.longdouble)
    e_sp = float(numpy.abs(numpy.log(lo.astype(numpy.longdouble)) - numpy.log(hi)).max())
    e_mc = float(numpy.abs(mlo - mhi).max() / numpy.abs(mhi).max())
    return job, e_sp, e_mc


def main():
    import world_analysis_cases as C
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, default=8)
    a = ap.parse_args()
    lengths = sorted(set(C.LENGTHS_GPU) | set(C.LENGTHS_EMU))
    jobs = [(wk, tk, n, fs) for fs in C.RATES for n in lengths for wk in C.WAVES for tk in C.TRACKS]
    with Pool(a.jobs) as pool:
        res = pool.map(one, jobs, chunksize=1)
    w_sp, w_mc = max(r[1] for r in res), max(r[2] for r in res)
    lines = ['worst sp float64-vs-longdouble max |log sp - log ref| %.6g' % w_sp,
             'worst mc float64-vs-longdouble max |mc - ref| / max |ref| %.6g' % w_mc,
             '# bars = 4 x these: sp %.6g, mc %.6g' % (4 * w_sp, 4 * w_mc),
             '# numpy %s; longdouble eps %.3g; %d cases: wave, f0 track, frames, fs, sp figure, mc figure' % (numpy.__version__, numpy.finfo(numpy.longdouble).eps, len(res))]
    for (wk, tk, n, fs), e_sp, e_mc in res:
        lines.append('%-6s %-12s frames=%3d fs=%5d sp %.4g mc %.4g' % (wk, tk, n, fs, e_sp, e_mc))
    out = ROOT / 'profiles' / 'r09' / 'analysis_tolerance.txt'
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines[:3]))


if __name__ == '__main__':
    main()
