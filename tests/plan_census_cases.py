"""The plan census: which launch plans the stage-2 planner can emit over the window sizes and batches the callers send, and the float64 walk at a
computed cover of them (tests/test_plan_census_cpu.py on the emulator, tests/test_plan_census_gpu.py on the card; DESIGN.md, "Plan census").

A RECORD is what `engine.Net.debug_plan` (`ry_net_debug_plan`, test-only) says of one layer of a (batch, frames) plan: path, tile, splits, K groups,
the Winograd and output-stationary shapes, which copies the layer reads and writes, the patch variant and the reduce kernel the launcher derives, and the
rows one enqueue computes (crop) and copies (hole).

A SIGNATURE is the per-layer tuple (layer, mode, batched, every record field), with the two row ranges expressed in tile rows relative to the grid --
"none", or (tile rows in front of the range, tile rows behind it) -- so that T itself does not make every record unique: with n = T - 28 real frames
the ranges keep their distance from both ends of the grid at every T.  Two points with the same signature on a layer launch the same kernel
instantiation with the same split, tile and row-range shape on that layer."""
import time

import numpy

import cases
from realtime_yukarin_amd import synth
from realtime_yukarin_amd.netspec import pad_frames

# (dtype mode, RY_WINOGRAD): the modes of tests/test_stage2_graph_oracle.py::SYN64_MODES (test_plan_census_gpu.py asserts they are the same)
MODES = [('f32', '1'), ('f32', '0'), ('bf16', '1'), ('bf16x3', '1')]
MODE_IDS = ['f32-winograd', 'f32-direct', 'bf16', 'bf16x3']

PATHS = {1: 'igemm', 2: 'direct', 3: 'first', 4: 'last', 5: 'igemm16', 7: 'os2d', 8: 'wino'}
TILE_DIMS = {1: (128, 128), 3: (64, 128), 4: (32, 128), 5: (128, 64), 6: (96, 128)}


# ---- points: (B, frames, window, discard).  window: the convert wrapper on `frames` real frames; else the raw forward at `frames` padded rows ----

def padded(point):
    B, n, window, _ = point
    return n + pad_frames(n) if window else n


def sweep_domain():
    """What the callers send: one window of n = T - 28 frames through the convert wrapper for T = 128 .. 2048, whole and with 20 frames discarded at
    either end; the raw forward (what the batch call runs) of 2, 3, 4 and 8 windows at T = 128 .. 512."""
    pts = [(1, T - 28, True, d) for T in range(128, 2049, 128) for d in ((0, 0), (20, 20))]
    pts += [(B, T, False, (0, 0)) for B in (2, 3, 4, 8) for T in (128, 256, 384, 512)]
    return pts


def emu_domain():
    """The part of the domain whose activation buffers the emulator can hold: T <= 256, B <= 2"""
    return [p for p in sweep_domain() if padded(p) <= 256 and p[0] <= 2]


def walked_points(table):
    """The windows tests/test_stage2_graph_oracle.py::test_syn64_layer_walk_gpu already walks in one mode, from the census of those windows: 100 frames
    whole and with discard (20, 20); 130 frames where that test walks them -- fp32 modes in which no layer of the 100-frame window has copied rows."""
    pts = [(1, 100, True, (0, 0)), (1, 100, True, (20, 20))]
    mode = next(iter(table[pts[0]]))[1]
    if MODES[mode][0] == 'f32' and not any(s[-1] != 'none' for s in table[pts[0]]):
        pts.append((1, 130, True, (0, 0)))
    return pts


# ---- signatures ----

def _rel_range(lo, n, total, th):
    """rows [lo, lo + n) of `total` in tile rows of th: 'none' (n == 0), else (tile rows in front, tile rows behind; 'x.y' where a boundary is not on a
    tile row -- the legality check refuses those)"""
    if n == 0:
        return 'none'
    f = lambda v: v // th if v % th == 0 else '%d.%d' % (v // th, v % th)
    return (f(lo), f(total - lo - n))


def signature(rec, mode, batched):
    """-> the hashable signature of one record (module docstring).  mode: index into MODES; batched: more than one window in the launch."""
    th = rec['tile_rows'] or 1
    crop = _rel_range(rec['crop_lo'], rec['crop_n'], rec['grid_rows'], th)
    # the hole is a range of OUTPUT rows of a convolution: the grid rows
    hole = _rel_range(rec['hole_lo'], rec['hole_n'], rec['rows_out'], th)
    kept = 'all' if (rec['out_lo'], rec['out_n']) == (0, rec['rows_out']) else 'part'
    return (rec['layer'], mode, bool(batched), PATHS[rec['path']], rec['tile'], rec['splits'], rec['kgroups'], rec['wino_cfg'], rec['wino_mbw'], tuple(rec['os2']),
            rec['reads16'], rec['writes32'], rec['writes16'], rec['patch'], rec['reduce'], rec['last_exp'], rec['tile_rows'], rec['tile_cols'], kept, crop, hole)


def unbatched(sig):
    return sig[:2] + sig[3:]


def census(net, mode, points):
    """-> ({point: [16 signatures]}, {point: [16 records]}).  Builds every plan (no launch)."""
    table, records = {}, {}
    for p in points:
        B, n, window, discard = p
        recs = net.debug_plan(B, n, window, discard)
        assert [r['layer'] for r in recs] == list(range(16))
        records[p] = recs
        table[p] = [signature(r, mode, B > 1) for r in recs]
    return table, records


def _points_short(points):
    """w / d: one window through the convert wrapper, whole / with discard (20, 20); fB: the raw forward of B windows; then T / 128 with runs folded"""
    groups = {}
    for p in points:
        B, n, window, discard = p
        key = ('d' if discard != (0, 0) else 'w') if window else 'f%d' % B
        if window and padded(p) - n != 28:
            key += '(n=%d)' % n                             # (the 130-frame window of the walk test)
        groups.setdefault(key, []).append(padded(p) // 128 if padded(p) % 128 == 0 else padded(p) / 128.0)
    out = []
    for key in sorted(groups):
        v, runs = sorted(groups[key]), []
        for t in v:
            if runs and t == runs[-1][1] + 1:
                runs[-1][1] = t
            else:
                runs.append([t, t])
        out.append(key + ':' + ','.join('%g' % a if a == b else '%g-%g' % (a, b) for a, b in runs))
    return ' '.join(out)


def census_report(mode_id, table):
    """The census of one mode for the committed report: one line per (layer, signature) with every field of the signature and the points that have it --
    the table of one line per (mode, B, T, layer) with equal lines folded."""
    out = []
    for layer in range(16):
        where = {}
        for p in sorted(table, key=point_order):
            where.setdefault(table[p][layer], []).append(p)
        for sig, pts in where.items():
            (_, _, batched, path, tile, splits, kg, cfg, mbw, os2, r16, w32, w16, patch, reduce, last_exp, th, tw, kept, crop, hole) = sig
            out.append('%-12s L%-2d %-7s tile %d splits %2d kg %d wino %d:%d os2 %-9s r16 %d w32 %d w16 %d patch %d reduce %d exp %d tile %2dx%-2d B>1 %d rows %-4s crop %-8s hole %-8s | %s'
                       % (mode_id, layer, path, tile, splits, kg, cfg, mbw, ':'.join(str(v) for v in os2), r16, w32, w16, patch, reduce, last_exp, th, tw, batched, kept,
                          crop if crop == 'none' else '%s+%s' % crop, hole if hole == 'none' else '%s+%s' % hole, _points_short(pts)))
    return out


# ---- the cover ----

def point_order(p):
    return (p[0] * padded(p), padded(p), p[0], not p[2], p[1], p[3])


def greedy_cover(table, walked):
    """table {point: [signatures]}; walked: the points other tests walk.  Points in order of B x T (smallest first); a point is chosen when one of its
    signatures belongs neither to a walked point nor to a point chosen before it.  -> [(point, [layers whose signature is new there])], deterministic"""
    seen = set()
    for p in walked:
        seen |= set(table[p])
    cover = []
    for p in sorted(table, key=point_order):
        new = [i for i, s in enumerate(table[p]) if s not in seen]
        if new:
            cover.append((p, new))
            seen |= set(table[p][i] for i in new)
    return cover


# ---- legality of a record: the rules tests/test_abi.py states for the planner's picks, and those of the row ranges ----

def layer_channels(P, specs):
    """-> [(Cin, Cout)] from the parameter dict"""
    out = []
    for s in specs:
        W = P[s['key'] + '/W']
        out.append((W.shape[0], W.shape[1]) if s['tr'] else (W.shape[1], W.shape[0]))
    return out


def check_legal(rec, spec, cin, cout, what=''):
    path = PATHS[rec['path']]
    w = (what, spec['name'], rec)
    up = 2 if spec['tr'] else 1
    nphases, ntaps = (4, 4) if spec['tr'] else (1, spec['k'] ** 2)
    assert rec['splits'] >= 1, w
    if path in ('igemm', 'igemm16'):
        bm, bn = TILE_DIMS[rec['tile']]
        nk = ntaps * (cin // 32 if path == 'igemm' else (3 if rec['reads16'] == 2 else 1) * cin // 64)
        assert cout % bn == 0, w                                                    # the chosen tile divides Cout
        assert rec['kgroups'] in (1, 2) and rec['splits'] * rec['kgroups'] <= nk, w   # split-K x K groups never exceeds the K chunks
        assert rec['kgroups'] == 1 or bm <= 128, w                                  # K groups only with the 4-wave tiles
        assert path == 'igemm' or (bm <= 128 and rec['reads16'] in (1, 2)), w       # 16-bit: tiles up to 128 rows only
        assert rec['patch'] == 0 or rec['tile_cols'] == 16, w
    else:
        assert rec['tile'] == 0 and rec['kgroups'] == 0 and rec['patch'] == 0 and rec['reads16'] == 0, w
    if path == 'os2d':
        mt4, nt4, waves, depth = rec['os2']
        U = ntaps * (cin // 64)
        assert U % (4 * waves) == 0 and depth in (2, 4) and cout % (4 * nt4) == 0 and mt4 in (1, 2, 3, 4, 6), w
        assert rec['splits'] == 1, w
    else:
        assert tuple(rec['os2']) == (0, 0, 0, 0), w
    if path == 'wino':
        wm = {1: 2, 2: 4}[rec['wino_cfg']]
        assert rec['wino_mbw'] in (1, 2, 4) and wm % rec['wino_mbw'] == 0, w
        assert (rec['tile_rows'], rec['tile_cols']) == (8 * (wm // rec['wino_mbw']), 16 * rec['wino_mbw']), w
        assert rec['splits'] <= (1 if spec['tr'] else 4) * (cin // 16), w          # at least one patch per split
        assert spec['k'] == 4 and spec['s'] == 2 and cout % 64 == 0 and cin % 16 == 0, w
    else:
        assert rec['wino_cfg'] == 0 and rec['wino_mbw'] == 0, w
    assert (rec['reduce'] > 0) == (rec['splits'] > 1 and path in ('igemm', 'igemm16', 'wino')), w
    assert rec['writes32'] or rec['writes16'], w
    # the rows
    rows = rec['rows_out']
    assert 0 <= rec['out_lo'] and rec['out_n'] >= 1 and rec['out_lo'] + rec['out_n'] <= rows, w
    th = rec['tile_rows']
    if th:
        assert rec['grid_rows'] % th == 0 and rec['grid_cols'] % rec['tile_cols'] == 0, w
    if rec['crop_n']:
        assert path in ('igemm', 'igemm16', 'wino') and rec['layer'] >= 8, w
        lo, n = rec['crop_lo'], rec['crop_n']
        assert lo >= 0 and lo + n <= rec['grid_rows'] and (lo, n) != (0, rec['grid_rows']), w
        assert lo % (th or 1) == 0 and n % (th or 1) == 0, w                        # whole tile rows
        assert (rec['out_lo'], rec['out_n']) == (up * lo, up * n), w
        assert rec['hole_n'] == 0, w
    elif path != 'last':
        assert (rec['out_lo'], rec['out_n']) == (0, rows), w
    if rec['hole_n']:
        lo, n = rec['hole_lo'], rec['hole_n']
        assert path in ('igemm', 'igemm16', 'wino') and not spec['tr'] and rec['layer'] < 8, w
        assert th and lo >= 1 and lo % th == 0 and n % th == 0 and lo + n <= rows, w
        assert path == 'wino' or (rec['splits'] == 1 and rec['tile_cols'] == 16), w


# ---- bands of a layer too large for a whole float64 reference ----

def band_rows(rec, need, seed):
    """Output-row ranges of one layer for cases.s2_walk(bands=): in tile rows of the launch (the rows one tile row writes: th grid rows, 2 th of a
    deconvolution), the first and the last two, both sides of every boundary of the record (computed range, copied range, needed range), and a seeded
    third of the rest; adjacent tile rows merged.  -> [(a, b)]"""
    up = rec['rows_out'] // rec['grid_rows'] if rec['grid_rows'] else 1            # 2: a deconvolution's grid is its input pixels
    to = (rec['tile_rows'] or 1) * up
    rows = rec['rows_out']
    nt = -(-rows // to)
    pick = {0, 1, nt - 2, nt - 1}
    edges = [rec['out_lo'], rec['out_lo'] + rec['out_n'], need[0], need[1]]
    if rec['hole_n']:
        edges += [rec['hole_lo'], rec['hole_lo'] + rec['hole_n']]
    for e in edges:
        pick |= {(e - 1) // to, e // to}
    pick = {t for t in pick if 0 <= t < nt}
    rest = sorted(set(range(nt)) - pick)
    rng = numpy.random.default_rng(seed)
    if rest:
        pick |= set(int(v) for v in rng.choice(rest, size=-(-len(rest) // 3), replace=False))
    out = []
    for t in sorted(pick):
        a, b = t * to, min((t + 1) * to, rows)
        if out and out[-1][1] == a:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


BAND_FROM_T = 640     # whole float64 references up to 512 padded rows (of all windows together); above, the new layers are held on bands (measured: profiles/r27/plan_census_pytest_gpu.txt)


# ---- the walk at one point ----

def _prof_of(recs, specs):
    """what cases.s2_reads_16bit wants of a profile: the layers whose kernel reads 16-bit copies, here from the records"""
    return [dict(name='ry_igemm_ldsdma<0,0,0,0,0,true,0>', layer=specs[r['layer']]['name']) for r in recs if r['reads16']]


def hole_stretches(w, n_frames):
    """tests/test_stage2_graph_oracle.py::_hole_stretches: down the encoder the rows behind the real frames are copies of one row, so every layer has a
    stretch of output rows that are equal bit for bit.  -> [(layer, first, last)] checked"""
    a, b = n_frames, w['x_in'].shape[1] - 1
    out = []
    for i in range(8):
        spec = w['specs'][i]
        a, b = -(-(a + spec['p']) // spec['s']), (b - (spec['k'] - 1) + spec['p']) // spec['s']
        for kind, o in enumerate(w['raw'][i]):
            if o is None:
                continue
            b = min(b, o.shape[1] - 1)
            if b - a < 1:
                return out
            bits = o.view(numpy.uint32) if o.dtype == numpy.float32 else o
            assert (bits[:, a:b + 1] == bits[:, a:a + 1]).all(), (spec['name'], kind, 'rows %d .. %d behind the real frames are not bit-identical' % (a, b))
            out.append((spec['name'], a, b))
    return out


def forward_input(B, T, bins):
    """a padded block as the batch call hands it to the raw forward: log spectrogram rows, the last bin dropped"""
    return numpy.log(synth.stage2_input(T, B, seed=93, bins=bins)[:, :, :bins - 1]).astype(numpy.float32)


def run_point(net, desc, P, mode, point, new_layers, E, E_LOG, band_from=BAND_FROM_T, seed=5):
    """One cover point, on a fresh plan (the caller holds RY_POISON=1): set_dtype drops the plans, debug_plan builds this one, the convert / forward runs
    it, cases.s2_walk holds the layers in new_layers to float64 (on bands from band_from padded rows up) and every other layer to the finiteness /
    NaN-row rule.  -> dict(records, signatures, met = the layers a float64 comparison ran on, walk, seconds, y)"""
    B, n, window, discard = point
    t0 = time.time()
    specs = cases.s2_layers(desc)
    what = '%s %s B=%d n=%d discard %s' % (MODE_IDS[mode], 'convert' if window else 'forward', B, n, discard)
    net.set_dtype(MODES[mode][0])
    recs = net.debug_plan(B, n, window, discard)
    sigs = [signature(r, mode, B > 1) for r in recs]
    T = padded(point)
    bins = net.width + 1
    if window:
        sp = synth.stage2_input(n, B, seed=91, bins=bins)
        y = net.convert(sp, discard=discard)
        x_in = None
    else:
        x_in = forward_input(B, T, bins)
        y = net.forward(x_in)
    assert net.debug_plan(B, n, window, discard) == recs, (what, 'the plan that ran is not the plan of the census')
    layers = set(new_layers)
    bands = None
    if B * T >= band_from:                                    # (rows of all windows: what the float64 reference costs)
        heights = [r['rows_out'] for r in recs]
        k0 = discard[0] if discard[0] < n else 0
        k1 = n - discard[1] if n - discard[1] > k0 else n
        need = cases.s2_needed_rows(specs, heights, k0, k1)
        bands = {i: band_rows(recs[i], need[i], seed + i) for i in layers if i < 15}
    w = cases.s2_walk(net, desc, P, n, y, discard if window else (0, 0), _prof_of(recs, specs), True, None, what=what, layers=layers, bands=bands, x_in=x_in)
    met = {i for i, q in enumerate(w['layers']) if q['held']}
    assert met == {i for i in layers if not (i == 15 and w['fused'])}, (what, met, layers)
    k0, k1 = w['k']
    if window:
        cases.s2_check_pad(w['x_in'], sp, n, True, E_LOG, what)
        assert w['x_in'].shape[1] - n == pad_frames(n)
        cases.s2_check_end(w, P, y, n, E, what)                   # the end layer against float64 on the device's own sources, whatever its signature
        met.add(15)
        assert not y[:, :k0].any() and not y[:, k1:].any(), (what, 'discarded rows come back as zeros (host call)')
        if any(r['hole_n'] for r in recs):
            assert hole_stretches(w, n), what
    else:
        assert w['fused'] and numpy.isfinite(y).all(), what
        if 15 in layers:                                          # the raw forward's end layer: no exp, every row, straight into the caller's block
            spec = specs[15]
            W, b, _ = cases.s2_layer_params(P, spec, False)
            srcs = [w['raw'][s][0].astype(numpy.float64) for s in spec['src']]
            r, bound = cases.ref_conv2d_f64(numpy.concatenate(srcs, axis=3), W, b, None, 1, spec['p'], False, None)
            cases.assert_close_elementwise(y, r[..., 0], bound[..., 0], cases.F32_TOL, what + ' decoder/c7')
            met.add(15)
    return dict(records=recs, signatures=sigs, met=met, walk=w, seconds=time.time() - t0, y=y, x_in=x_in, what=what)


def batch_equals_alone(net, mode, point, res):
    """A raw forward of B > 1 windows against each window run alone: every layer whose signature (but for `batched`) is the one of the B = 1 plan, and
    whose sources are such layers, holds the same bits; so does the result when that is every layer.  -> the layers compared"""
    B, T, window, _ = point
    assert B > 1 and not window
    one = [unbatched(signature(r, mode, False)) for r in net.debug_plan(1, T, False)]
    same = []
    specs = res['walk']['specs']
    for i in range(16):
        srcs = [s for s in specs[i]['src'] if s is not None and s >= 0]
        if unbatched(res['signatures'][i]) == one[i] and all(s in same for s in srcs):
            same.append(i)
    for b in range(B):
        y1 = net.forward(res['x_in'][b:b + 1])
        for i in same:
            if i == 15:
                assert numpy.array_equal(y1[0].view(numpy.uint32), res['y'][b].view(numpy.uint32)), (res['what'], 'window %d alone differs in the result' % b)
                continue
            for kind in (0, 1):
                o = res['walk']['raw'][i][kind]
                if o is None:
                    continue
                o1 = cases.s2_fetch(net, i, kind)
                assert o1 is not None and numpy.array_equal(o1[0].view(o1.dtype.str.replace('f', 'u')), o[b].view(o.dtype.str.replace('f', 'u'))), \
                    (res['what'], 'window %d alone differs at layer %d, copy %d' % (b, i, kind))
    return same


def print_point(res, new_layers):
    """one line: wall time, then per held layer its worst |y - r| / (tol bound) (`b`: held on bands)"""
    tol = dict(f32=cases.F32_TOL, bf16=cases.BF16_TOL, x3=cases.X3_TOL)
    held = ['L%d%s %.2f' % (i, 'b' if q['banded'] else '', (q['worst'] if q['worst'] is not None else q['worst16']) / tol[q['fmt']])
            for i, q in enumerate(res['walk']['layers']) if q['held']]
    print('%-46s %4.1f s  %s%s' % (res['what'], res['seconds'], '  '.join(held), '  end' if 15 in res['met'] else ''))
