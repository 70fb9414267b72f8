"""The error bar of the output-gate tests: max |device mean_db - float64 reference| over every case of tests/output_gate_cases.py, measured on the
emulator build (default) or, with --gpu, on the card, and the figure of a complex64 restatement (what librosa stores) against the float64 one.
Each run rewrites its own lines of profiles/r24/output_gate_tolerance.txt and keeps the other's; the tests hold the device to 16 times the
larger of the two measured values.

    python scripts/output_gate_tolerance.py            # CPU, emulator
    python scripts/output_gate_tolerance.py --gpu      # MI355X"""
import argparse
import sys
from pathlib import Path

import numpy

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]
OUT = ROOT / 'profiles' / 'r24' / 'output_gate_tolerance.txt'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpu', action='store_true')
    ap.add_argument('--out', default=str(OUT))
    a = ap.parse_args()
    import output_gate_cases as C
    import output_gate_ref as R
    from realtime_yukarin_amd import _lib, build, engine, output_gate
    if a.gpu:
        ctx, tag = engine.get_context(0), 'gpu'
    else:
        ctx, tag = engine.Context(0, _lib.Ry355Lib(build.build_emu())), 'emu'
    lines, worst, worst_c64, closest = [], 0.0, 0.0, None
    for name, n in C.CASES:
        x = C.signal(name, n)
        ref = C.ref_mean(name, n)
        g = output_gate.OutputGate(n, C.THRESHOLD, ctx=ctx)
        g.push(x)
        emitted, silent, mean = g.last
        g.close()
        assert emitted
        err = abs(mean - ref)
        worst = max(worst, err)
        line = '%s %-10s N=%5d ref %.9f device %.9f |diff| %.3e silent %d' % (tag, name, n, ref, mean, err, silent)
        if not a.gpu:
            c64 = abs(R.mean_db(x, complex64=True) - ref)
            worst_c64 = max(worst_c64, c64)
            line += ' complex64 |diff| %.3e' % c64
        if closest is None or abs(ref + C.THRESHOLD) < abs(closest[2] + C.THRESHOLD):
            closest = (name, n, ref)
        lines.append(line)
    lines.append('%s worst |device - float64 reference| %.6e dB' % (tag, worst))
    if not a.gpu:
        lines.append('%s worst |complex64 restatement - float64 reference| %.6e dB' % (tag, worst_c64))
        lines.append('%s closest to -%g dB: %s N=%d at %.4f dB' % (tag, C.THRESHOLD, closest[0], closest[1], closest[2]))
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    kept = [l for l in out.read_text().splitlines() if not l.startswith(tag + ' ') and not l.startswith('#')] if out.exists() else []
    head = '# numpy %s; mean_db of the output gate against tests/output_gate_ref.py (float64); the tests use 16 x the larger worst figure' % numpy.__version__
    body = kept + lines
    body.sort(key=lambda l: 0 if l.startswith('emu ') else 1)
    out.write_text('\n'.join([head] + body) + '\n')
    print('\n'.join(lines[-3:]))


if __name__ == '__main__':
    main()
