"""The bars of the split-bf16 mode of the CREPE network (tests/test_crepe_x3_cpu.py, tests/test_crepe_x3_gpu.py), derived without a device.

    python scripts/crepe_x3_tolerance.py [--out profiles/r14/crepe_x3_tolerance.txt]

The numpy restatement of the mode (tests/crepe_x3_cases.py: RNE split of x and W, the products lo hi, hi lo, hi hi per K step of 16, float32
accumulation one product at a time in chunks of 64 in the kernel's split order) runs every layer of the case list on the float32 output of the
layer before it.  Per layer, the worst |y - exact64| / bound over the list is measured, bound = (conv(|x|, |W|) + |b|) |scale| + |shift|; the bar is
4 x that: the factor covers the summation order inside the matrix instruction, which the restatement does not model (the WORLD bars take 4 x the
float64-vs-longdouble figure in the same way).  No bar is taken from a kernel's output.  3 * 2^-18 = 1.1e-5, the derivable worst case of one
product, is printed as a sanity ceiling only: a bar near it could not see a missing cross term.

Condition on the list: for conv1, a middle conv layer and the dense layer of the small-K cases (multiplier 4: K = 512, 1024, 256) the file shows
what the restatement gives with one cross term dropped and with lo cut off instead of rounded; each should exceed the layer's bar.  A dropped cross
term does, a hundredfold.  The truncated lo does NOT: it raises an operand's error from 2^-18 to at most 2^-17 of its value, the restatement's ratio
from 1.7e-6 to 2.2 .. 2.7e-6, below 4 x the worst ratio on any input the device can be given (the file says so: `condition lo truncated = NOT MET`).
What holds the split's rounding is the emulator test that compares the kernel with the restatement bit for bit (tests/test_crepe_x3_cpu.py).

The activation bar: |act_x3 - act_f32| <= (4 (E_x3 + E_f32)) / 4 + 2 ACT_TOL, E the worst |logit - logit64| of the chained restatements (the mode's,
and plain float32) over the list and the sine signals of the f0 test; the sigmoid's slope is at most 1 / 4, ACT_TOL is the float32 sigmoid's own error."""
import argparse
import sys
from pathlib import Path

import numpy

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

FACTOR = 4.0
LIST = [(1, 1), (1, 3), (4, 1), (4, 2), (4, 3), (2, 5), (9, 2)]      # the emulator list and a few more: (multiplier, frames)
CONDITION = {'conv1': 0, 'conv4': 3, 'dense': 6}                    # at multiplier 4: K = 512, 1024, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r14' / 'crepe_x3_tolerance.txt'))
    args = ap.parse_args()
    import crepe_cases as cc
    import crepe_ref
    import crepe_x3_cases as xc

    worst = {n: 0.0 for n in xc.NAMES}
    rows, mut_rows = [], []
    e_x3 = e_f32 = 0.0
    chains = [('m %d, %d frames' % c, c[0], xc.frames32(*c)) for c in LIST]
    chains += [('m %d, sine %g Hz' % (xc.SINE_M, f), xc.SINE_M, crepe_ref.frames(xc.sine(f, xc.SINE_FRAMES), xc.HOP, False).astype('f4')) for f in xc.SINES]
    mutants = {}
    for what, m, fr in chains:
        P, sp = xc.params(m), xc.splits(m)
        L = xc.network_x3(P, m, fr)
        ratios = []
        for i in range(7):
            r, bound = xc.conv_exact(P, i, L[i]) if i < 6 else cc.dense_ref(P, L[6])
            ratios.append(float((numpy.abs(L[i + 1].astype('f8') - r) / bound).max()))
            worst[xc.NAMES[i]] = max(worst[xc.NAMES[i]], ratios[-1])
        rows.append('%-24s %s' % (what, '  '.join('%s %.3e' % (n, v) for n, v in zip(xc.NAMES, ratios))))
        l64 = xc.network_f64(P, fr)
        e_x3 = max(e_x3, float(numpy.abs(L[7] - l64).max()))
        e_f32 = max(e_f32, float(numpy.abs(xc.network_f32(P, fr)[7] - l64).max()))
        if m == 4 and 'sine' not in what:
            for name, i in CONDITION.items():
                r, bound = xc.conv_exact(P, i, L[i]) if i < 6 else cc.dense_ref(P, L[6])
                run = (lambda **kw: xc.conv_x3(P, i, L[i], sp[i], **kw)) if i < 6 else (lambda **kw: xc.dense_x3(P, L[6], sp[6], **kw))
                for label, kw in (('without lo hi', dict(drop='lo hi')), ('without hi lo', dict(drop='hi lo')),
                                  ('lo truncated', dict(split_x=xc.split_trunc_lo, split_w=xc.split_trunc_lo))):
                    v = float((numpy.abs(run(**kw).astype('f8') - r) / bound).max())
                    mutants.setdefault((name, label), []).append((what, v))
    bar = {n: FACTOR * worst[n] for n in xc.NAMES}
    text = ['# the split-bf16 mode of the CREPE network: worst |y - exact64| / bound of the numpy restatement per layer (scripts/crepe_x3_tolerance.py)',
            '# sanity ceiling (one product: 3 * 2^-18) = %.3e; factor %g on the worst ratio for the matrix instruction\'s summation order' % (xc.SANITY_CEILING, FACTOR)]
    text += rows
    text += ['worst %s = %.6e' % (n, worst[n]) for n in xc.NAMES]
    text += ['bar %s = %.6e' % (n, bar[n]) for n in xc.NAMES]
    text += ['# condition: the restatement with one term dropped / lo truncated must exceed the bar in at least one case per layer kind',
             '# %-8s %-14s %-20s %-12s %-12s' % ('layer', 'mutant', 'case', 'ratio', 'bar')]
    met = {}
    for (name, label), vals in sorted(mutants.items()):
        for what, v in vals:
            text.append('mutant %-6s %-14s %-20s %.6e %.6e %s' % (name, label, what.replace(', ', ' / '), v, bar[name], 'above' if v > bar[name] else 'below'))
        met[label] = met.get(label, True) and any(v > bar[name] for _, v in vals)
    act = FACTOR * (e_x3 + e_f32) / 4 + 2 * cc.ACT_TOL
    text += ['# chained logits against float64: split-bf16 restatement %.6e, float32 %.6e' % (e_x3, e_f32),
             '# act bar = %g (%.6e + %.6e) / 4 + 2 * %g' % (FACTOR, e_x3, e_f32, cc.ACT_TOL),
             'bar act = %.6e' % act,
             ] + ['condition %s = %s' % (label, 'met' if ok else 'NOT MET') for label, ok in sorted(met.items())]
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join(text) + '\n')
    print('\n'.join(text))
    return 0 if met['without lo hi'] and met['without hi lo'] else 1


if __name__ == '__main__':
    sys.exit(main())
