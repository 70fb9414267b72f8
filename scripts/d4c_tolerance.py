"""CPU: the error bars of tests/test_world_d4c_cpu.py / _gpu.py.  The D4C kernel runs float64 butterflies, so its bars are 4 x the error of the numpy
float64 restatement (tests/world_d4c_ref.py) against the same restatement in numpy.longdouble with its own transform, worst over the inputs of the
tests (tests/world_analysis_cases.py):  a0: max |a0 - ref| over the voiced frames;  coarse: max |coarse dB - ref| over the frames that are on in both;
ap: max |20 log10 ap - ref|.  The zero-mean step of a window cancels almost everything where the wave is constant under it (frames behind the end
of the wave), and the group delay is a quotient of smoothed spectra: the bars come from the same inputs, not from a constant.
Writes profiles/r10/d4c_tolerance.txt: the three worst figures first (the tests read lines 1 to 3), then every case.

    python scripts/d4c_tolerance.py [--jobs 8]"""
import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]


def one(job):
    import world_analysis_cases as C
    import world_d4c_ref as R
    from world_d4c_cases import SEED as R_SEED                     # the D4C tests' own seed
    wk, tk, n, fs = job
    x, f0, t = C.case(wk, tk, n, fs)
    lo = R.d4c(x, f0, t, fs, seed=R_SEED, details=True)
    hi = R.d4c(x, f0, t, fs, seed=R_SEED, dtype=numpy.longdouble, details=True)
    assert numpy.array_equal(lo[2], hi[2]), 'on / off differs between float64 and longdouble: %s' % (job,)
    on = lo[2]
    e_a0 = float(numpy.abs(lo[1] - hi[1]).max())
    e_co = float(numpy.abs(lo[3][on] - hi[3][on]).max()) if on.any() else 0.0
    e_ap = float(numpy.abs(20 * numpy.log10(lo[0].astype(numpy.longdouble)) - 20 * numpy.log10(hi[0])).max())
    return job, e_a0, e_co, e_ap, int(on.sum())


def main():
    import world_analysis_cases as C
    from world_d4c_cases import SEED as R_SEED
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, default=8)
    a = ap.parse_args()
    lengths = sorted(set(C.LENGTHS_GPU) | set(C.LENGTHS_EMU))
    jobs = [(wk, tk, n, fs) for fs in C.RATES for n in lengths for wk in C.WAVES for tk in C.TRACKS]
    with Pool(a.jobs) as pool:
        res = pool.map(one, jobs, chunksize=1)
    w_a0, w_co, w_ap = max(r[1] for r in res), max(r[2] for r in res), max(r[3] for r in res)
    lines = ['worst a0 float64-vs-longdouble max |a0 - ref| %.6g' % w_a0,
             'worst coarse float64-vs-longdouble max |coarse dB - ref| over on-frames %.6g' % w_co,
             'worst ap float64-vs-longdouble max |20 log10 ap - ref| %.6g' % w_ap,
             '# bars = 4 x these: a0 %.6g, coarse %.6g dB, ap %.6g dB' % (4 * w_a0, 4 * w_co, 4 * w_ap),
             '# numpy %s; longdouble eps %.3g; seed %d; %d cases: wave, f0 track, frames, fs, frames on, a0 figure, coarse figure, ap figure'
             % (numpy.__version__, numpy.finfo(numpy.longdouble).eps, R_SEED, len(res))]
    for (wk, tk, n, fs), e_a0, e_co, e_ap, n_on in res:
        lines.append('%-6s %-12s frames=%3d fs=%5d on=%3d a0 %.4g coarse %.4g ap %.4g' % (wk, tk, n, fs, n_on, e_a0, e_co, e_ap))
    out = ROOT / 'profiles' / 'r10' / 'd4c_tolerance.txt'
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines[:4]))


if __name__ == '__main__':
    main()
