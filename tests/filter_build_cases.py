"""Filter layouts built on the card (filter build mode 'device') against the host functions of csrc/ry_plan.cpp, which stay the
oracle: cases and test bodies for tests/test_filter_build_cpu.py (the emulator) and tests/test_filter_build_gpu.py (the card).

Everything is compared as uint32, every float of every allocation (padding included), with RY_POISON=1 where the test says so: the staging buffer and
the destinations then start as NaN patterns, so a float a kernel leaves out shows.

Planted values.  Every raw filter carries -0.0, a denormal, +inf, -inf and a NaN with a payload at recorded places.  In a k4 filter of two spatial
dimensions they stand, each value in turn, on each of the 16 kernel positions of a (n, c) pair of their own: every kernel position is one tap of one of the
four 2 x 2 stencils of the Winograd form, so every value visits every tap position of a stencil, and no stencil holds two of them.  One more pair holds
+inf and -inf in one stencil (their sum is the default NaN).  Two different NaNs never meet in one sum: which payload an x86 addsd keeps then depends
on the operand order the host compiler picked, which is no property of the layout.

What the Winograd transform must show on them (why a kernel that skips the zero-coefficient terms fails): with G = [[1, 0], [1, 1], [0, 1]] a tap g[a][b]
has coefficient G[i][a] G[j][b] = 1 at four of the nine positions and 0 at five.  An infinite tap gives inf at the four and 0 * inf = NaN at the five; a
NaN tap gives NaN at all nine."""
import copy
import ctypes
import weakref

import numpy
import pytest

from realtime_yukarin_amd import engine, netspec, synth
from realtime_yukarin_amd._lib import Ry355Error
from realtime_yukarin_amd.netspec import NetDesc
from realtime_yukarin_amd.weights import flatten_params, synthetic_params

KINDS = ('w1d', 'w1os', 'wig', 'wdir', 'w2os', 'wwin')
NEG_ZERO, DENORMAL, P_INF, N_INF, NAN_PAYLOAD = 0x80000000, 0x00000001, 0x7f800000, 0xff800000, 0x7fc12345
SPECIALS = (NEG_ZERO, DENORMAL, P_INF, N_INF, NAN_PAYLOAD)
RY_EINVAL, RY_ESTATE = -1, -4

# ---- one layer: (name, W shape, keyword arguments of Context.debug_layer_filters) -------------------------------------------------------------------
# 1-D: k = 1 .. 4; stride-1 convolution, k4 s2 p1 convolution, deconvolution; one source and two; cin_a % 64 != 0 (the per-lane form of plan_s1_os);
# cout = 1, 63, 64, 65 (the layouts of a stage-1 layer do not depend on stride or pad: they are carried for the record)
LAYERS_1D = [('k%d-s1-n%d' % (k, n), (n, 5 + k, k), dict(stride=1, pad=k // 2)) for k, n in ((1, 1), (2, 63), (3, 64), (4, 65))]
LAYERS_1D += [('k4-s2-n64', (64, 70, 4), dict(stride=2, pad=1)),
              ('k4-s2-two-sources', (65, 96 + 32, 4), dict(stride=2, pad=1, cin_b=32)),          # cin_a = 96: % 64 != 0
              ('k1-two-sources-n1', (1, 40 + 24, 1), dict(cin_b=24)),
              ('deconv-n63', (64, 63, 4), dict(stride=2, pad=1, transposed=True)),
              ('deconv-two-sources-n65', (80 + 48, 65, 4), dict(stride=2, pad=1, transposed=True, cin_b=48)),
              ('deconv-n1', (33, 1, 4), dict(stride=2, pad=1, transposed=True))]
# 2-D: the smallest Winograd-eligible layers (convolution and deconvolution k4 s2 p1, cin 16 and 16 + 16, cout 64 and 128); implicit GEMM without a
# Winograd form (cout 64 at k3; cin 32, cout 64 -- and cout 32: direct only, with a Winograd-shaped filter); the last layer's shape (direct only);
# the output-stationary layout (cin_a % 256 == 0) with one source and two
K4 = dict(stride=2, pad=1)
LAYERS_2D = [('conv-16-64', (64, 16, 4, 4), K4), ('conv-16+16-128', (128, 32, 4, 4), dict(K4, cin_b=16)),
             ('deconv-16-64', (16, 64, 4, 4), dict(K4, transposed=True)), ('deconv-16+16-128', (32, 128, 4, 4), dict(K4, transposed=True, cin_b=16)),
             ('conv-k3-32-64', (64, 32, 3, 3), dict(stride=1, pad=1)), ('conv-k1-64-64', (64, 64, 1, 1), dict()),
             ('conv-32-32', (32, 32, 4, 4), K4),
             ('last-128-1', (1, 128, 3, 3), dict(stride=1, pad=1)), ('first-1-6', (6, 1, 3, 3), dict(stride=1, pad=1)),
             ('os-conv-256-8', (8, 256, 4, 4), dict(K4, want_os2=True)), ('os-deconv-256+256-64', (512, 64, 4, 4), dict(K4, transposed=True, cin_b=256, want_os2=True)),
             ('os-k1-256-64', (64, 256, 1, 1), dict(want_os2=True))]
# what each 2-D layer must have (the eligibility rules of ry_plan.cpp restated: the test fails if a layout silently goes missing in both modes)
EXPECT_2D = {'conv-16-64': {'wdir', 'wwin'}, 'conv-16+16-128': {'wdir', 'wwin'}, 'deconv-16-64': {'wdir', 'wwin'}, 'deconv-16+16-128': {'wdir', 'wwin'},
             'conv-k3-32-64': {'wig', 'wdir'}, 'conv-k1-64-64': {'wig', 'wdir'}, 'conv-32-32': {'wdir'}, 'last-128-1': {'wdir'}, 'first-1-6': {'wdir'},
             'os-conv-256-8': {'wdir', 'w2os'}, 'os-deconv-256+256-64': {'wig', 'wdir', 'w2os', 'wwin'}, 'os-k1-256-64': {'wig', 'wdir', 'w2os'}}


def syn64_largest_layer():
    """The SYN-64 layer with the most filter floats, as netspec gives it -> (name, W shape, kwargs): a decoder deconvolution of 512 + 512 -> 512 channels"""
    desc = synth.model_descs('SYN-64')[1]
    key, shape = max(((k, s) for k, s in netspec.param_list(desc) if k.endswith('/W')), key=lambda q: int(numpy.prod(q[1])))
    j = int(key.split('/')[1][1:])
    assert key.startswith('decoder/') and netspec.dec_sample(desc, j) == 'up', key
    cin_b = netspec.ENC_CH[7 - j] * desc.base
    return key, shape, dict(K4, transposed=True, cin_b=cin_b)


# ---- filters with planted values ---------------------------------------------------------------------------------------------------------------------

def plant(W, seed):
    """Random normal W (any filter shape) with the special values written in place -> [(flat index, bits)]"""
    rng = numpy.random.default_rng(seed)
    bits = W.reshape(-1).view(numpy.uint32)
    placed = []
    if W.ndim == 4 and W.shape[2] == 4 and W.shape[0] * W.shape[1] >= 5 * 16 + 1:
        pairs = rng.choice(W.shape[0] * W.shape[1], size=5 * 16 + 1, replace=False)
        for i, v in enumerate(SPECIALS):
            for pos in range(16):
                placed.append((int(pairs[i * 16 + pos]) * 16 + pos, v))
        placed += [(int(pairs[-1]) * 16 + 5, P_INF), (int(pairs[-1]) * 16 + 7, N_INF)]      # (ky, kx) = (1, 1) and (1, 3): one stencil, taps of one row
    else:
        where = rng.choice(bits.size, size=min(bits.size, 2 * len(SPECIALS)), replace=False)
        placed = [(int(w), SPECIALS[i % len(SPECIALS)]) for i, w in enumerate(where)]
    for idx, v in placed:
        bits[idx] = v
    return placed


def random_filter(shape, seed):
    W = numpy.random.default_rng(seed).normal(0, 0.1, shape).astype(numpy.float32)
    return W, plant(W, seed + 1)


def u32(a):
    return numpy.ascontiguousarray(a).view(numpy.uint32)


def same_bits(a, b, what):
    a, b = u32(a), u32(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not numpy.array_equal(a, b):
        bad = numpy.flatnonzero(a != b)
        raise AssertionError('%s: %d of %d floats differ, first at %d: %08x against %08x' % (what, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]]))


class Modes(object):
    """switches the process-wide mode of one library, and puts 'host' back"""
    def __init__(self, ctx):
        self.ctx = ctx

    def set(self, mode):
        engine.set_filter_build(mode, self.ctx.lib)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.set('host')


def poison(ctx, monkeypatch, on=True):
    if on:
        monkeypatch.setenv('RY_POISON', '1')
    else:
        monkeypatch.delenv('RY_POISON', raising=False)
    ctx.reload_env()


def layer_layouts(ctx, W, kw):
    """{kind: layout} of one layer in the mode in force; a layout the layer does not have must be refused with RY_ESTATE"""
    out = {}
    for kind in KINDS:
        if (kind in ('w1d', 'w1os')) != (W.ndim == 3):
            continue
        try:
            out[kind] = ctx.debug_layer_filters(W, kind, **kw)
        except Ry355Error as e:
            assert '(code %d)' % RY_ESTATE in str(e), (kind, e)
    return out


def check_layer(ctx, name, shape, kw, seed, expect=None):
    """One layer in both modes: the same layouts exist, with the same bits; the permutation layouts hold exactly the filter's bits (the planted ones among
    them) and +0.0 padding; the Winograd filters show the planted values as the module docstring says."""
    W, placed = random_filter(shape, seed)
    with Modes(ctx) as m:
        m.set('host'); host = layer_layouts(ctx, W, kw)
        m.set('device'); dev = layer_layouts(ctx, W, kw)
    assert set(host) == set(dev), (name, sorted(host), sorted(dev))
    if expect is not None:
        assert set(host) == set(expect), (name, sorted(host))
    assert host, name
    for kind in host:
        same_bits(dev[kind], host[kind], '%s %s' % (name, kind))
        if kind != 'wwin':
            pad = host[kind].size - W.size
            assert pad >= 0 and (pad == 0 or kind in ('w1d', 'w1os')), (name, kind, pad)
            want = numpy.sort(numpy.concatenate([u32(W).reshape(-1), numpy.zeros(pad, numpy.uint32)]))
            assert numpy.array_equal(numpy.sort(u32(dev[kind])), want), (name, kind, 'not a permutation of the filter with +0.0 padding')
    if 'wwin' in host and len(placed) > 2 * len(SPECIALS):
        n_inf = sum(1 for _, v in placed if v in (P_INF, N_INF)) - 2
        n_nan = sum(1 for _, v in placed if v == NAN_PAYLOAD)
        w = dev['wwin']
        assert int(numpy.isnan(w).sum()) >= 5 * n_inf + 9 * n_nan and int(numpy.isinf(w).sum()) >= 4 * n_inf, (name, 'the zero-coefficient terms are missing')
        assert int((u32(w) == NAN_PAYLOAD).sum()) == 9 * n_nan, (name, 'the payload of a NaN tap reaches all nine positions')
    return sorted(host)


# ---- predictors ---------------------------------------------------------------------------------------------------------------------------------------

def planted_blob(desc, seed):
    """flat weights of a predictor with the special values planted in every layer's filter (BN and bias stay ordinary) -> (blob, bytes of the filters,
    bytes of the padded scale + shift arrays)"""
    P = synthetic_params(desc, seed, bias_std=0.05)
    raw = scsh = 0
    for i, (key, shape) in enumerate(netspec.param_list(desc)):
        if key.endswith('/W'):
            P[key] = numpy.ascontiguousarray(P[key], dtype=numpy.float32)
            plant(P[key], seed + 17 * i)
            raw += 4 * P[key].size
            cout = shape[1] if key.startswith('decoder/') and key != 'decoder/c7/W' and netspec.dec_sample(desc, int(key.split('/')[1][1:])) == 'up' else shape[0]
            scsh += 2 * 4 * ((cout + 3) // 4 * 4)
    return flatten_params(desc, P), raw, scsh


def net_layouts(net):
    """{(layer, kind): layout} of everything the predictor has ('wwin' built on demand)"""
    out = {}
    for layer in range(16):
        for kind in KINDS:
            try:
                out[(layer, kind)] = net.debug_filters(layer, kind)
            except Ry355Error as e:
                assert '(code %d)' % RY_ESTATE in str(e), (layer, kind, e)
    return out


def build_pair(ctx, desc, blob, width):
    with Modes(ctx) as m:
        m.set('host'); a = engine.Net(ctx, desc, blob, width=width)
        m.set('device'); b = engine.Net(ctx, desc, blob, width=width)
    return a, b


def check_predictor_layouts(ctx, desc, width, seed, monkeypatch, os2_minw=None):
    """Two predictors from one blob, one per mode: every layer, every kind, every float; the counters after create and after the Winograd builds; equal
    arena bytes.  Under RY_POISON=1."""
    try:
        if os2_minw is not None:
            monkeypatch.setenv('RY_OS2_MINW', str(os2_minw))
        poison(ctx, monkeypatch)
        blob, raw_bytes, scsh_bytes = planted_blob(desc, seed)
        host, dev = build_pair(ctx, desc, blob, width)
        sh0, sd0 = host.build_stats(), dev.build_stats()
        with Modes(ctx) as m:
            m.set('host'); lh = net_layouts(host)
            m.set('device'); ld = net_layouts(dev)
        assert set(lh) == set(ld) and len(lh) >= 32, (sorted(lh), sorted(ld))
        for key in sorted(lh):
            same_bits(ld[key], lh[key], 'layer %d %s' % key)
        built = [k for k in lh if k[1] != 'wwin']
        wino = [k for k in lh if k[1] == 'wwin']
        # after create
        assert sd0['bytes_downloaded'] == 0 and sd0['host_relayout_floats'] == 0, sd0
        assert sd0['bytes_uploaded'] == raw_bytes + scsh_bytes, (sd0, raw_bytes, scsh_bytes)
        assert sd0['layout_launches'] == len(built), (sd0, len(built))
        assert sh0['layout_launches'] == 0 and sh0['bytes_downloaded'] == 0, sh0
        assert sh0['host_relayout_floats'] == sum(lh[k].size for k in built), sh0
        assert sh0['bytes_uploaded'] == 4 * sh0['host_relayout_floats'] + scsh_bytes, sh0
        assert sh0['arena_bytes'] == sd0['arena_bytes'], (sh0, sd0)
        # after the Winograd builds
        sh1, sd1 = host.build_stats(), dev.build_stats()
        assert sd1['bytes_downloaded'] == 0 and sd1['host_relayout_floats'] == 0 and sd1['bytes_uploaded'] == sd0['bytes_uploaded'], sd1
        assert sd1['layout_launches'] == len(built) + len(wino), sd1
        assert sh1['bytes_downloaded'] == sum(4 * lh[(k[0], 'wdir')].size for k in wino), sh1
        assert sh1['host_relayout_floats'] == sh0['host_relayout_floats'] + sum(lh[k].size for k in wino), sh1
        assert sh1['arena_bytes'] == sd1['arena_bytes'], (sh1, sd1)
        kinds = sorted(set(k[1] for k in lh))
        host.close(); dev.close()
        return kinds
    finally:
        monkeypatch.delenv('RY_OS2_MINW', raising=False)
        poison(ctx, monkeypatch, False)


def clone_of(net):
    """a second handle on the predictor (ry_net_clone) as an engine.Net"""
    h = ctypes.c_void_p()
    net.ctx.lib.check(net.ctx.lib.dll.ry_net_clone(net.handle, ctypes.byref(h)))
    c = copy.copy(net)
    c.handle = h
    c._dependents = weakref.WeakSet()
    return c


S2_SMALL = NetDesc(2, 1, 1, 64, 3)
S2_WIDTH = 64                  # the narrowest spectrogram whose k4 s2 p1 layers have a Winograd tile (16 columns after two halvings)
# every eligible layer gets the output-stationary layout and the Winograd form whatever its size; decoder c1 stays on the implicit GEMM
S2_ENV = {'RY_OS2_MINW': '1', 'RY_WINO_MINM': '1', 'RY_OS2': '9:0'}
S2_WINDOWS = (70,)             # frames of the windows of check_forward_bits


def paths_of(net, n):
    return [r['path'] for r in net.debug_plan(1, n, True)]


def check_forward_bits(ctx, monkeypatch):
    """ry_sr_convert, ry_sr_convert_rows and ry_ac_convert of device-built predictors against host-built ones; the plans' paths from ry_net_debug_plan;
    clones made before and after the lazy Winograd build; a net of each mode alive across a mode switch."""
    try:
        for k, v in S2_ENV.items():
            monkeypatch.setenv(k, v)
        poison(ctx, monkeypatch)
        P = synthetic_params(S2_SMALL, 451, bias_std=0.05)
        blob = flatten_params(S2_SMALL, P)
        with Modes(ctx) as m:
            m.set('host')
            host = engine.Net(ctx, S2_SMALL, blob, width=S2_WIDTH)                # built in host mode ...
            m.set('device')
            dev = engine.Net(ctx, S2_SMALL, blob, width=S2_WIDTH)                 # ... alive while the mode switches and a second net is built
            early = clone_of(dev)                                                 # a clone from before the lazy build
            launches0 = dev.build_stats()['layout_launches']
            seen = set()
            n_wino = set()
            for n in S2_WINDOWS:
                sp = synth.stage2_input(n, 1, seed=90 + n, bins=S2_WIDTH + 1)[0]
                m.set('host'); ref = host.convert(sp); ref_part = host.convert(sp, discard=(4, 3))
                m.set('device'); y = dev.convert(sp)
                ph, pd = paths_of(host, n), paths_of(dev, n)
                assert ph == pd, (n, ph, pd)
                seen |= set(pd)
                n_wino |= {i for i, q in enumerate(pd) if q == 8}
                same_bits(y, ref, 'ry_sr_convert, %d frames' % n)
                same_bits(dev.convert(sp, discard=(4, 3)), ref_part, 'ry_sr_convert_rows, %d frames' % n)
                late = clone_of(dev)                                              # a clone from after it
                same_bits(early.convert(sp), ref, 'clone made before the Winograd build, %d frames' % n)
                same_bits(late.convert(sp), ref, 'clone made after the Winograd build, %d frames' % n)
                assert early.build_stats() == late.build_stats() == dev.build_stats()
                late.close()
            assert {1, 7, 8} <= seen, ('the windows must take the implicit-GEMM, output-stationary and Winograd paths', sorted(seen))
            st = dev.build_stats()
            assert st['layout_launches'] - launches0 == len(n_wino) and st['bytes_downloaded'] == 0, (st, launches0, sorted(n_wino))   # one build per layer, three handles
            assert host.build_stats()['bytes_downloaded'] > 0 and host.build_stats()['layout_launches'] == 0
            early.close()
            # stage 1
            d1 = NetDesc(1, 9, 9, 16, 3)
            b1 = flatten_params(d1, synthetic_params(d1, 452, bias_std=0.05))
            x = synth.stage1_input(37, 2, seed=77)
            m.set('device'); n1d = engine.Net(ctx, d1, b1)
            m.set('host'); n1h = engine.Net(ctx, d1, b1)
            same_bits(n1d.convert(x), n1h.convert(x), 'ry_ac_convert')
            for net in (n1d, n1h, host, dev):
                net.close()
        return sorted(seen)
    finally:
        for k in S2_ENV:
            monkeypatch.delenv(k, raising=False)
        poison(ctx, monkeypatch, False)


def mode_in_force(ctx):
    """'host' or 'device', read off what a tiny predictor's build took (there is no getter: the mode is a switch, not a state to poll)"""
    d = NetDesc(1, 1, 1, 1, 0)
    net = engine.Net(ctx, d, flatten_params(d, synthetic_params(d, 3)))
    st = net.build_stats()
    net.close()
    return 'device' if st['layout_launches'] else 'host'


def check_refusals(ctx, monkeypatch):
    lib = ctx.lib
    with Modes(ctx) as m:
        for mode in ('device', 'host'):
            m.set(mode)
            for bad in (-1, 2, 7):
                assert lib.dll.ry_set_filter_build(bad) == RY_EINVAL
            with pytest.raises(ValueError):
                engine.set_filter_build('gpu', lib)
            assert mode_in_force(ctx) == mode
            try:
                monkeypatch.setenv('RY_FILTER_BUILD', 'card')
                with pytest.raises(Ry355Error, match='RY_FILTER_BUILD'):
                    ctx.reload_env()
                assert mode_in_force(ctx) == mode
                other = 'host' if mode == 'device' else 'device'
                monkeypatch.setenv('RY_FILTER_BUILD', other)
                ctx.reload_env()
                assert mode_in_force(ctx) == other
                monkeypatch.delenv('RY_FILTER_BUILD')
                ctx.reload_env()
                assert mode_in_force(ctx) == other                     # an absent variable leaves the mode alone
            finally:
                monkeypatch.delenv('RY_FILTER_BUILD', raising=False)
                ctx.reload_env()
        m.set('device')
        d = NetDesc(1, 2, 2, 4, 2)
        net = engine.Net(ctx, d, flatten_params(d, synthetic_params(d, 5)))
        before = net.build_stats()
        out = numpy.full(4096, 7.25, dtype=numpy.float32)
        n = ctypes.c_size_t(12345)
        fp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        for kind in ('wig', 'wdir', 'w2os', 'wwin'):                   # a stage-1 layer has none of them
            assert lib.dll.ry_net_debug_filters(net.handle, 1, engine._lib.FILTER_KINDS[kind], fp, out.size, ctypes.byref(n)) == RY_ESTATE
            assert n.value == 12345
        assert lib.dll.ry_net_debug_filters(net.handle, 16, 0, fp, out.size, ctypes.byref(n)) == RY_EINVAL
        assert lib.dll.ry_net_debug_filters(net.handle, 1, 6, fp, out.size, ctypes.byref(n)) == RY_EINVAL and n.value == 12345
        want = 4 * 8 * 4                                               # encoder c1: 4 -> 8 channels, [C][N][4]
        assert lib.dll.ry_net_debug_filters(net.handle, 1, 0, fp, want - 1, ctypes.byref(n)) == RY_EINVAL and n.value == want
        assert (out == 7.25).all() and net.build_stats() == before
        assert lib.dll.ry_net_debug_filters(net.handle, 1, 0, fp, want, ctypes.byref(n)) == 0 and not (out[:want] == 7.25).all() and (out[want:] == 7.25).all()
        net.close()
