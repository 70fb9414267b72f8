"""CPU: the error bars of tests/test_world_domain_cpu.py / _gpu.py.  As for the other WORLD tests the bars are 4 x the error of the numpy float64
restatements (tests/world_synth_ref.py, world_analysis_ref.py, world_d4c_ref.py) against the same restatements in numpy.longdouble, worst over the
inputs of the tests (tests/world_domain_cases.py), one figure per group:

    synthesis waveform      max |y - ref| / max |ref|
    sp                      max |log sp - log ref|
    mc cases                max |mc - ref| / max |ref| of the CheapTrick cases (order 8, alpha = mcepalpha(fs))
    mc sp2mc order= alpha=  ... of `sp2mc` on the 30 rows with a known mel-cepstrum, per pair: alpha = 0.9 at order 63 conditions differently from order 8
    mc run order= alpha=    ... of CheapTrick + sp2mc (Analyzer.run) on glide x glide at 16 kHz, per pair
    a0, coarse, ap          as scripts/d4c_tolerance.py

Writes profiles/r13/world_domain_tolerance.txt: one labelled line per group (the tests read them), then every case as a comment.

    python scripts/world_domain_tolerance.py [--jobs 8]"""
import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]
LD = numpy.longdouble


def one(job):
    import world_analysis_cases as A
    import world_analysis_ref as RA
    import world_d4c_ref as RD
    import world_domain_cases as C
    import world_synth_ref as RS
    from realtime_yukarin_amd import sptk
    unit = job[0]
    if unit == 'synth':
        _, fs, fp, kind, n = job
        f0, sp, ap = C.synth_case(kind, C.synth_frames(n, fs, fp), fs)
        ref = RS.synthesize(f0, sp, ap, fs, fp, seed=1, fft_size=1024, dtype=LD)
        y = RS.synthesize(f0, sp, ap, fs, fp, seed=1, fft_size=1024)
        den = float(numpy.abs(ref).max())
        return job, {'synthesis waveform': float(numpy.abs(y.astype(LD) - ref).max()) / den if den > 0 else 0.0}
    if unit == 'cheaptrick':
        _, wk, tk, n, fs, q1, floor = job
        x, f0, t = C.case(wk, tk, n, fs) if tk in C.TRACKS else A.case(wk, tk, n, fs)
        lo = RA.cheaptrick(x, f0, t, fs, q1=q1, f0_floor=floor, fft_size=1024, seed=C.SEED)
        hi = RA.cheaptrick(x, f0, t, fs, q1=q1, f0_floor=floor, fft_size=1024, seed=C.SEED, dtype=LD)
        alpha = sptk.mcepalpha(fs)
        mlo, mhi = RA.sp2mc_rows(lo, A.ORDER, alpha), RA.sp2mc_rows(hi, A.ORDER, alpha, dtype=LD)
        return job, {'sp': float(numpy.abs(numpy.log(lo.astype(LD)) - numpy.log(hi)).max()),
                     'mc cases': float(numpy.abs(mlo - mhi).max() / numpy.abs(mhi).max())}
    if unit == 'sp2mc':
        _, order, alpha = job
        sp = C.sp2mc_rows(order, alpha)
        mlo, mhi = RA.sp2mc_rows(sp, order, alpha), RA.sp2mc_rows(sp, order, alpha, dtype=LD)
        x, f0, t = A.case('glide', 'glide', 13, 16000)
        lo = RA.cheaptrick(x, f0, t, 16000, f0_floor=C.FLOOR, fft_size=1024, seed=C.SEED)
        hi = RA.cheaptrick(x, f0, t, 16000, f0_floor=C.FLOOR, fft_size=1024, seed=C.SEED, dtype=LD)
        rlo, rhi = RA.sp2mc_rows(lo, order, alpha), RA.sp2mc_rows(hi, order, alpha, dtype=LD)
        return job, {'mc sp2mc order=%d alpha=%g' % (order, alpha): float(numpy.abs(mlo - mhi).max() / numpy.abs(mhi).max()),
                     'mc run order=%d alpha=%g' % (order, alpha): float(numpy.abs(rlo - rhi).max() / numpy.abs(rhi).max())}
    _, wk, tk, n, fs = job
    x, f0, t = C.case(wk, tk, n, fs)
    lo = RD.d4c(x, f0, t, fs, threshold=C.threshold(tk), seed=C.SEED, details=True)
    hi = RD.d4c(x, f0, t, fs, threshold=C.threshold(tk), seed=C.SEED, dtype=LD, details=True)
    assert numpy.array_equal(lo[2], hi[2]), 'on / off differs between float64 and longdouble: %s' % (job,)
    on = lo[2]
    return job, {'a0': float(numpy.abs(lo[1] - hi[1]).max()),
                 'coarse': float(numpy.abs(lo[3][on] - hi[3][on]).max()) if on.any() else 0.0,
                 'ap': float(numpy.abs(20 * numpy.log10(lo[0].astype(LD)) - 20 * numpy.log10(hi[0])).max())}


def main():
    import world_domain_cases as C
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, default=8)
    a = ap.parse_args()
    frames = sorted(set(C.FRAMES_GPU) | set(C.FRAMES_EMU))
    jobs = [('synth', fs, fp, kind, n) for fs, fp in C.CONFIGS for kind in C.SYNTH_TRACKS for n in sorted(set(C.SYNTH_FRAMES_GPU) | set(C.SYNTH_FRAMES_EMU))]
    jobs += [('cheaptrick', wk, tk, n, fs, -0.15, C.FLOOR) for fs in C.RATES for tk in C.TRACKS for wk in C.WAVES for n in frames]
    jobs += [('cheaptrick', 'glide', 'glide', n, 16000, q1, C.FLOOR) for q1 in C.Q1 for n in frames]
    jobs += [('cheaptrick', 'glide', 'glide', n, 16000, -0.15, floor) for floor in C.FLOORS for n in frames]
    jobs += [('sp2mc', order, alpha) for order in C.ORDERS for alpha in C.ALPHAS]
    jobs += [('d4c', wk, tk, n, fs) for fs in C.D4C_RATES for tk in C.D4C_TRACKS for wk in C.WAVES for n in frames]
    with Pool(a.jobs) as pool:
        res = pool.map(one, jobs, chunksize=1)
    # No figure below 2^-52: a float64 result cannot be asked to sit closer to the exact one than the spacing of float64 at its own scale.  (The rows of
    # order 0 are flat spectra, whose transform is exact in any arithmetic: their measured figure is the luck of one rounding of `log`.)
    worst = {}
    for _, figures in res:
        for k, v in figures.items():
            worst[k] = max(worst.get(k, float(numpy.finfo(numpy.float64).eps)), v)
    lines = ['# float64 restatement against the longdouble one (eps %.3g), numpy %s, worst over %d cases; the tests take 4 x these'
             % (numpy.finfo(LD).eps, numpy.__version__, len(res))]
    lines += ['%s %.6g' % (k, worst[k]) for k in worst]
    for job, figures in res:
        lines.append('# ' + ' '.join(str(v) for v in job) + ': ' + '  '.join('%s %.4g' % kv for kv in figures.items()))
    out = ROOT / 'profiles' / 'r13' / 'world_domain_tolerance.txt'
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join(lines) + '\n')
    print('\n'.join(lines[:8]))


if __name__ == '__main__':
    main()
