"""The accuracy of the device's expf / logf relative to the result, measured against float64: the two allowances E / E_log of
tests/test_stage2_graph_oracle.py (the ROCm installation documents no figure for them in its headers or docs).

    python scripts/stage2_graph_tolerance.py [--emu] [--out profiles/r12/stage2_graph_tolerance.txt]

expf runs through ry_mc2sp with mc = [[1]] and the arguments as the one row of mtx (1 * a + 0 is exact): 200 001 arguments over [-40, 40], plus
every float32 within 2^-12 of zero on a coarse grid.  logf runs through the pad node of a stage-2 convert (ry_pad_min_rows, read back with
ry_net_debug_activation): 391 x 512 = 200 192 arguments exp(u), u uniform over [-40, 10] (the spectrogram floor 1e-16 is exp(-36.8)).
Each bar is 2 x the worst seen over the builds measured (argument reduction error is not uniform: a sample can miss the worst case).
The file keeps one section per build (the product library on the MI355X, --emu: the host emulator with the C library's functions); a run rewrites
its own section and the bars."""
import argparse
import sys
from pathlib import Path

import numpy

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def measure(ctx):
    from realtime_yukarin_amd import engine
    from realtime_yukarin_amd.netspec import NetDesc
    from realtime_yukarin_amd.weights import flatten_params, synthetic_params
    rng = numpy.random.default_rng(12)
    a = numpy.concatenate([numpy.linspace(-40.0, 40.0, 200001), rng.uniform(-2.0 ** -12, 2.0 ** -12, 2047)]).astype('f4')
    y = ctx.mc2sp(numpy.ones((1, 1), 'f4'), a[None, :], 0.0)[0]
    e_exp = numpy.abs(y.astype('f8') / numpy.exp(a.astype('f8')) - 1)
    d = NetDesc(2, 1, 1, 8, 8)
    net = engine.Net(ctx, d, flatten_params(d, synthetic_params(d, 1)), width=512)
    sp = numpy.exp(rng.uniform(-40.0, 10.0, size=(1, 391, 513))).astype('f4')
    net.convert(sp)
    x_in = net.debug_activation(-1)[:, :391]
    net.close()
    r = numpy.log(sp[:, :, :512].astype('f8'))
    e_log = numpy.abs(x_in - r) / numpy.abs(r)
    return (float(e_exp.max()), float(a[int(e_exp.argmax())]), a.size), (float(e_log.max()), float(sp[:, :, :512].ravel()[int(e_log.argmax())]), r.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--emu', action='store_true')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r12' / 'stage2_graph_tolerance.txt'))
    args = ap.parse_args()
    from realtime_yukarin_amd import _lib, build, engine
    ctx = engine.Context(0, _lib.Ry355Lib(build.build_emu())) if args.emu else engine.get_context(0)
    (we, ae, ne), (wl, al, nl) = measure(ctx)
    tag = 'emulator' if args.emu else 'MI355X'
    out = Path(args.out)
    old = out.read_text().splitlines() if out.exists() else []
    keep = [l for l in old if l.startswith(('emulator', 'MI355X')) and not l.startswith(tag)]
    mine = ['%s expf worst |y / exp(a) - 1| = %.6e at a = %r over %d arguments in [-40, 40]' % (tag, we, ae, ne),
            '%s logf worst |y - log(x)| / |log(x)| = %.6e at x = %r over %d arguments in exp([-40, 10])' % (tag, wl, al, nl)]
    rows = sorted(keep + mine)
    worst = lambda fn: max(float(l.split(' = ')[1].split()[0]) for l in rows if ' %s ' % fn in l)
    text = ['# expf / logf of the device against float64, relative to the result (scripts/stage2_graph_tolerance.py); no documented figure under the',
            '# ROCm installation (headers, share/doc), so the bars are measured: 2 x the worst seen over the builds below.  2^-24 = 5.96e-08 is one float32 rounding.']
    text += rows
    text += ['E = %.6e' % (2 * worst('expf')), 'E_log = %.6e' % (2 * worst('logf'))]
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join(text) + '\n')
    print('\n'.join(text))


if __name__ == '__main__':
    main()
