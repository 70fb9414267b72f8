"""Shared parity cases: the same operator / predictor cases run on the emulator (CPU) and on the MI355X."""
import numpy

from oracle import ops_numpy as ops
from oracle import unet

TOL = 1e-4   # BASELINE.json north_star: "within 1e-4 relative fp32"
F32_TOL = 1e-5   # element-wise against float64, in units of the bound of a sum: any fp32 summation order of the same products (the oracle files)
X3_TOL = 3e-5    # ... split-bf16 against the fp32-operand reference (the dropped lo * lo term and the 16-bit split)
BF16_TOL = 1e-5  # ... plain bf16 against the reference on bf16-rounded operands (exact products, fp32 accumulation)

# B, L, Cin, Cout, k, stride, pad, dilate, transposed, act, splits
CONV1D_CASES = [
    (1, 40, 9, 64, 3, 1, 1, 1, False, 'lrelu', 0),        # encoder c0 shape
    (2, 64, 64, 128, 4, 2, 1, 1, False, 'lrelu', 0),      # encoder down layer, batch 2
    (1, 8, 128, 70, 4, 2, 1, 1, False, 'relu', 4),        # ragged Cout, split over input channels
    (1, 5, 96, 64, 4, 2, 1, 1, True, 'relu', 3),          # decoder up layer, odd length
    (2, 33, 40, 128, 4, 2, 1, 1, True, None, 0),
    (1, 50, 16, 32, 3, 1, 3, 3, False, 'glu', 0),         # dilated conv + GLU (north_star operator coverage)
    (1, 37, 8, 16, 1, 1, 0, 1, False, None, 0),           # 'same' 1x1 layer (extensive_layers < 8)
    (1, 64, 12, 20, 4, 3, 2, 2, False, 'relu', 2),        # generic stride/dilation path
    (1, 1, 16, 64, 4, 2, 1, 1, True, 'relu', 0),          # deepest decoder layer: length 1 -> 2
    (1, 2, 16, 64, 4, 2, 1, 1, False, 'lrelu', 2),        # deepest encoder layer: length 2 -> 1
]

# B, H, W, Cin, Cout, k, stride, pad, transposed, act, path, tile, splits
CONV2D_CASES = [
    (1, 8, 12, 1, 16, 3, 1, 1, False, 'lrelu', 'direct', None, 0),     # SR encoder c0 (Cin = 1)
    (1, 6, 8, 24, 1, 3, 1, 1, False, None, 'direct', None, 0),         # SR decoder c7 (Cout = 1)
    (2, 6, 8, 8, 12, 4, 2, 1, False, 'lrelu', 'direct', None, 0),
    (1, 3, 4, 8, 12, 4, 2, 1, True, 'relu', 'direct', None, 0),
    (1, 12, 16, 32, 128, 4, 2, 1, False, 'lrelu', 'igemm', '32x128', 0),
    (1, 12, 16, 32, 128, 4, 2, 1, False, 'lrelu', 'igemm', '64x128', 2),
    (2, 16, 16, 64, 128, 4, 2, 1, False, 'lrelu', 'igemm', '128x128', 1),
    (1, 16, 36, 32, 64, 4, 2, 1, False, 'relu', 'igemm', '128x64', 3),
    (1, 3, 4, 64, 128, 4, 2, 1, True, 'relu', 'igemm', '32x128', 0),   # M = 12 rows: ragged tile
    (1, 6, 10, 32, 64, 4, 2, 1, True, 'relu', 'igemm', '128x64', 2),
    (1, 5, 7, 64, 128, 3, 1, 1, False, None, 'igemm', '64x128', 0),
    (1, 5, 7, 32, 128, 1, 1, 0, False, 'relu', 'igemm', '32x128', 1),
    (1, 2, 4, 64, 128, 4, 2, 1, False, 'lrelu', 'igemm', None, 0),     # deepest encoder layer, auto tile/split
    (1, 2, 4, 128, 128, 4, 2, 1, False, 'lrelu', 'igemm', '32x128', 21),  # 21 slabs: wide split-K reduce, ragged slab groups
    (2, 7, 10, 1, 64, 3, 1, 1, False, 'lrelu', 'first', None, 0),      # specialised SR encoder c0 (ragged width)
    (2, 5, 9, 128, 1, 3, 1, 1, False, None, 'last', None, 0),          # specialised SR decoder c7 (two-source concat)
    (1, 4, 6, 256, 1, 3, 1, 1, False, None, 'last', None, 0),
    (2, 5, 32, 128, 1, 3, 1, 1, False, None, 'last', None, 0),         # rolling-window form (W % 16 == 0, 128 channels)
    (1, 3, 16, 128, 1, 3, 1, 1, False, None, 'last', None, 0),
    (1, 16, 20, 32, 64, 4, 2, 1, False, 'relu', 'igemm', '128x64', 2),
    (1, 32, 64, 32, 128, 4, 2, 1, False, 'lrelu', 'igemm', '64x128', 1),   # 512 rows: 8 tiles of 64, 2-D 4x16 pixel tiles
    (1, 32, 64, 32, 128, 4, 2, 1, False, 'lrelu', 'igemm', '128x128', 1),  # 16x32 outputs: 2-D 8x16 pixel tiles
    (2, 8, 16, 32, 128, 4, 2, 1, True, 'relu', 'igemm', '64x128', 1),      # deconv, batch 2, 2-D 4x16 tiles over the input grid
    (1, 24, 32, 32, 128, 4, 2, 1, False, 'relu', 'igemm', '96x128', 2),    # 12x16 outputs: 2-D 6x16 tiles, split-K
    (1, 20, 24, 32, 128, 4, 2, 1, False, 'lrelu', 'igemm', '96x128', 1),   # 120 rows: one full 96-row tile + a ragged one
    (1, 6, 8, 64, 256, 4, 2, 1, True, 'relu', 'igemm', '96x128', 2),       # deconv, 2 N-tiles, 4 phases, split-K, XCD-ordered grid
    (1, 6, 10, 64, 64, 4, 2, 1, True, 'relu', 'igemm', '128x64', 0),
    # two K groups per workgroup (split-K summed through the LDS), alone and combined with external split-K
    (1, 24, 32, 64, 128, 4, 2, 1, False, 'relu', 'igemm', '96x128k2', 1),  # 32 chunks: 16 + 16
    (1, 20, 24, 32, 128, 4, 2, 1, False, 'lrelu', 'igemm', '96x128k2', 1), # ragged last tile, 16 chunks
    (1, 16, 16, 96, 128, 3, 1, 1, False, 'lrelu', 'igemm', '128x128k2', 1),# 27 chunks: 13 + 14 (unequal groups)
    (1, 6, 8, 64, 256, 4, 2, 1, True, 'relu', 'igemm', '96x128k2', 2),     # deconv phases, external split 2 x 2 groups (8 chunks -> 2 + 2 | 2 + 2)
    (1, 16, 20, 64, 64, 4, 2, 1, False, 'relu', 'igemm', '128x64k2', 1),
    (2, 8, 16, 32, 128, 4, 2, 1, True, 'relu', 'igemm', '64x128k2', 1),    # 4 chunks per phase: 2 + 2
    (1, 12, 16, 32, 128, 4, 2, 1, False, 'lrelu', 'igemm', '32x128k2', 3), # 16 chunks, 3 external splits of 5/5/6 -> groups of 2+3 / 2+3 / 3+3
    (1, 24, 32, 64, 128, 4, 2, 1, False, 'relu', 'igemm', '96x128k1', 2),  # forced single group
    # sub-pixel deconvolution on 16-pixel-wide 2-D tiles: the input-patch variant (one patch per channel chunk, 4 taps read from it)
    (1, 12, 16, 128, 128, 4, 2, 1, True, 'relu', 'igemm', '96x128', 1),    # 4 chunks x 4 taps, 2 tiles of 6x16 per phase, image borders on every side
    (2, 12, 32, 96, 128, 4, 2, 1, True, 'lrelu', 'igemm', '96x128k2', 1),  # 3 chunks: K groups of 1 + 2 chunks, batch 2, 2 tile columns
    (1, 16, 16, 128, 64, 4, 2, 1, True, 'relu', 'igemm', '128x64', 2),     # 8x16 tiles, external split of 2 + 2 chunks
    (1, 8, 16, 64, 128, 4, 2, 1, True, None, 'igemm', '64x128', 1),        # 4x16 tiles, 2 chunks
    (1, 16, 32, 160, 128, 4, 2, 1, True, 'relu', 'igemm', '128x128k2', 1), # 5 chunks: groups of 2 + 3 (odd counts of 8 / 12 iterations)
    # k4 s2 convolution on 16-pixel-wide 2-D tiles: one patch per (channel chunk, input parity), image borders on every side
    (1, 32, 32, 64, 64, 4, 2, 1, False, 'relu', 'igemm', '128x64', 1),     # 16x16 outputs = 2 tiles of 8x16; 2 chunks x 4 parities
    (2, 16, 32, 96, 128, 4, 2, 1, False, 'lrelu', 'igemm', '64x128k2', 1), # batch 2, 12 patches: K groups of 6 + 6
    (1, 24, 64, 32, 128, 4, 2, 1, False, None, 'igemm', '96x128', 3),      # 2 tile columns, 4 patches over 3 external splits (2 + 1 + 1)
    (1, 32, 32, 160, 128, 4, 2, 1, False, 'relu', 'igemm', '128x128k2', 1),# 20 patches: groups of 10 + 10
]


# ry_c2d_os, the output-stationary weight-streaming kernel on the K-batched v_mfma_f32_4x4x1_16B_f32 (round 5): tile = (mt4, nt4, waves, depth);
# Cin % 128 == 0 cases are handed over as two half-width sources (the un-materialised skip concat)
CONV2D_OS_CASES = [
    (1, 6, 8, 256, 16, 4, 2, 1, False, 'lrelu', 'os', (3, 1, 4, 4), 0),    # 3x4 = 12 output pixels (encoder c7 at 300 frames), image borders on every side; 4 rounds per wave, rotated start
    (1, 12, 16, 512, 32, 4, 2, 1, False, 'lrelu', 'os', (3, 2, 8, 4), 0),  # 48 pixels = four 12-pixel tiles x four 8-channel tiles, two sources of 256 channels, eight waves
    (1, 3, 4, 256, 16, 4, 2, 1, True, 'relu', 'os', (3, 1, 4, 4), 0),      # sub-pixel deconvolution: 4 phases x 12 input pixels (decoder c0), one round per wave
    (2, 3, 4, 512, 24, 4, 2, 1, True, None, 'os', (2, 2, 8, 2), 0),        # batch 2, two sources, eight waves, three 8-pixel tiles, three 8-channel tiles
    (1, 10, 8, 256, 8, 4, 2, 1, False, 'relu', 'os', (4, 2, 4, 4), 0),     # 20 pixels on 16-pixel tiles: a ragged last tile
    (1, 5, 7, 1024, 16, 1, 1, 0, False, 'relu', 'os', (6, 4, 4, 2), 0),    # 'same' 1x1 layer (extensive_layers < 8): 35 pixels on 24-pixel tiles, 96 sums per lane, two sources
    (1, 4, 8, 256, 64, 4, 2, 1, False, 'lrelu', 'os', None, 0),            # the planner's slice
    (1, 2, 4, 256, 128, 4, 2, 1, False, 'lrelu', 'os', (1, 1, 8, 4), 0),   # deepest encoder layer at 100 frames: 1x2 pixels on a 4-pixel tile
    (1, 1, 4, 256, 64, 4, 2, 1, True, 'relu', 'os', (1, 4, 4, 4), 0),      # deepest decoder layer at 100 frames: 4 pixels, 16-channel tiles
    (1, 6, 6, 256, 8, 4, 2, 1, False, None, 'os', (1, 2, 16, 2), 0),       # 9 pixels on 4-pixel tiles, sixteen waves of one round each
    (1, 6, 8, 512, 8, 4, 2, 1, False, 'relu', 'os', (3, 2, 8, 2), 0),   # two units in flight, four rounds per wave, two sources
]


# ry_wino_ldsdma, the k4 s2 p1 layers in Winograd F(2x2, 2x2) form (round 6): tile = (cfg, mbw): cfg 1 = 2 x 2 waves (M-tile of two 8 x 16-pixel blocks,
# 64 channels), cfg 2 = 4 x 2 waves (four blocks); mbw = blocks per tile row.  Cin % 32 == 0 cases are handed over as two half-width sources.
CONV2D_WINO_CASES = [
    (1, 8, 32, 16, 64, 4, 2, 1, True, 'relu', 'wino', (1, 2), 1),      # sub-pixel deconvolution, ONE 8 x 32 tile per phase, one 16-channel patch, single source: image borders on every side
    (1, 16, 16, 32, 64, 4, 2, 1, True, 'relu', 'wino', (1, 1), 1),     # 16 x 16 tile, two sources of 16 channels
    (1, 16, 32, 64, 128, 4, 2, 1, True, 'lrelu', 'wino', (1, 2), 2),   # two tile rows, two channel tiles, external split of 2 + 2 patches (slabs + reduce)
    (1, 32, 64, 32, 64, 4, 2, 1, False, 'lrelu', 'wino', (1, 2), 1),   # k4 s2 convolution: four parity planes per chunk accumulate in the transform domain, 16 x 32 outputs
    (2, 32, 32, 48, 64, 4, 2, 1, False, None, 'wino', (1, 1), 3),      # batch 2, 12 (chunk, parity) patches over 3 splits, single source of 48 channels
    (1, 8, 64, 16, 64, 4, 2, 1, True, 'relu', 'wino', (2, 4), 1),      # eight waves: 8 x 64 tile
    (1, 16, 32, 32, 64, 4, 2, 1, True, 'relu', 'wino', (2, 2), 1),     # 16 x 32 tile
    (1, 32, 16, 64, 128, 4, 2, 1, True, 'lrelu', 'wino', (2, 1), 2),   # 32 x 16 tile, split-K
    (1, 32, 64, 32, 64, 4, 2, 1, False, 'lrelu', 'wino', (2, 2), 1),   # convolution on eight waves
    (2, 64, 32, 48, 64, 4, 2, 1, False, None, 'wino', (2, 1), 3),
    (1, 32, 64, 80, 128, 4, 2, 1, True, 'relu', 'wino', (1, 2), 0),    # 5 patches (odd iteration counts per buffer), the planner's split
    (1, 48, 64, 16, 64, 4, 2, 1, False, 'relu', 'wino', None, 0),      # the planner's everything: 24 x 32 outputs
    (1, 24, 32, 64, 64, 4, 2, 1, True, None, 'wino', (1, 2), 4),       # 3 tile rows, one patch per split
]


def wino_vs_direct(ctx, transposed, seed=41):
    """The Winograd form against the direct implicit GEMM of the same operator on trained-like magnitudes (activations after a ReLU, filters ~ N(0, 0.02)):
    -> (max |y_wino - y_direct| / max |y_direct|, max |y_direct|)"""
    rng = numpy.random.default_rng(seed)
    B, H, W_, Cin, Cout = (1, 16, 32, 128, 64) if transposed else (1, 32, 64, 128, 64)      # a 16 x 32 grid of the stencil either way
    x = numpy.maximum(rng.normal(size=(B, H, W_, Cin)), 0).astype('f4')
    Wt = rng.normal(0, 0.02, size=(Cin, Cout, 4, 4) if transposed else (Cout, Cin, 4, 4)).astype('f4')
    kw = dict(stride=2, pad=1, transposed=transposed, act=None)
    yd = ctx.conv2d(x, Wt, None, None, path='igemm', **kw)
    yw = ctx.conv2d(x, Wt, None, None, path='wino', **kw)
    return float(numpy.abs(yw - yd).max() / numpy.abs(yd).max()), float(numpy.abs(yd).max())


def os_identity_rows(ctx):
    """1x1 'conv' = plain GEMM with one-hot rows on the output-stationary path: pixel i selects input channel 65 i mod 1024, so every K block,
    every K step of a unit and several units are hit.  -> (y [16][16], W rows expected)"""
    Cin, Cout = 1024, 16
    x = numpy.zeros((1, 4, 4, Cin), 'f4')
    for i in range(16):
        x[0, i // 4, i % 4, 65 * i % Cin] = 1.0
    W = (numpy.arange(Cout * Cin, dtype='f4').reshape(Cout, Cin, 1, 1) % 251) / 251.0
    y = ctx.conv2d(x, W, None, None, stride=1, pad=0, path='os', tile=(4, 4, 4, 4))
    return y.reshape(16, Cout), numpy.stack([W[:, 65 * i % Cin, 0, 0] for i in range(16)])      # y[pixel i][n] = W[n][65 i]


def os_every_slice(ctx, one_round=False):
    """Every instantiated slice of ry_c2d_os (tile rows / 4, tile channels / 4, waves, units in flight) on one layer against the implicit GEMM of the
    same operator: a decoder-c1-like sub-pixel deconvolution (48 rows per phase, 64 K units), or with one_round a 1 x 1 layer of 2048 channels whose
    waves run the prologue and the last round only (the pixel value carries its row and its 64-channel chunk: a KiB of a ring slot read before its DMA
    landed shows as a wrong chunk).  -> [(slice, relative error)] of the slices that exist for the shape"""
    rng = numpy.random.default_rng(31)
    if one_round:
        H, W_, Cin, Cout = 3, 8, 2048, 64
        x = ((numpy.arange(H * W_).reshape(H, W_, 1) + 1) + 1000.0 * (numpy.arange(Cin) // 64)[None, None, :]).astype('f4')[None]
        Wt = numpy.ones((Cout, Cin, 1, 1), 'f4')
        kw = dict(stride=1, pad=0, act=None)
    else:
        H, W_, Cin, Cout = 6, 8, 1024, 64
        x = rng.normal(size=(1, H, W_, Cin)).astype('f4')
        Wt = rng.normal(0, 0.02, size=(Cin, Cout, 4, 4)).astype('f4')
        kw = dict(stride=2, pad=1, transposed=True, act=None)
    yi = ctx.conv2d(x, Wt, None, None, path='igemm', **kw)
    out = []
    for n in (1, 2, 4):
        for m in (1, 2, 3, 4, 6):
            for (w, d) in ((4, 4), (8, 4), (8, 2), (16, 2), (4, 2)):
                try:
                    y = ctx.conv2d(x, Wt, None, None, path='os', tile=(m, n, w, d), **kw)
                except RuntimeError as e:
                    assert 'no output-stationary slice' in str(e), e
                    continue
                out.append(((m, n, w, d), float(numpy.abs(y - yi).max() / numpy.abs(yi).max())))
    return out


# 2-D dilated convolution (north_star operator coverage: "1-D/2-D dilated conv"): B, H, W, Cin, Cout, k, stride, pad, dilate, act, path, tile, splits
CONV2D_DILATED_CASES = [
    (1, 12, 16, 32, 128, 3, 1, 2, 2, 'lrelu', 'igemm', '32x128', 0),       # 'same' 3x3 with dilation 2 on the MFMA path
    (2, 10, 14, 64, 128, 3, 1, 3, 3, 'relu', 'igemm', '64x128', 2),        # dilation 3, batch 2, split-K
    (1, 16, 20, 32, 64, 4, 2, 3, 2, None, 'igemm', '128x64', 1),           # k4 s2 with dilation 2 (the gather variant: no input patches)
    (1, 9, 11, 8, 12, 3, 1, 2, 2, 'lrelu', 'direct', None, 0),             # odd channel counts: the direct path
    (1, 7, 9, 5, 6, 2, 1, 0, 4, None, 'direct', None, 0),                  # k2, dilation 4, no padding
]


def run_conv2d_dilated(ctx, rng, case, bn_params):
    B, H, W_, Cin, Cout, k, s, p, d, act, path, tile, splits = case
    x = rng.normal(size=(B, H, W_, Cin)).astype('f4')
    Wt = rng.normal(0, 0.1, size=(Cout, Cin, k, k)).astype('f4')
    b = rng.normal(0, 0.1, Cout).astype('f4')
    bn = bn_params(rng, Cout)
    y = ctx.conv2d(x, Wt, b, bn, stride=s, pad=p, dilate=d, act=act, path=path, tile=tile, splits=splits)
    r = ops.conv_nd(x.transpose(0, 3, 1, 2), Wt, b, stride=s, pad=p, dilate=d)
    r = ops.apply_act(ops.batch_norm_inference(r, *bn), act).transpose(0, 2, 3, 1)
    return y, r


def bf16_round(a):
    """float32 -> nearest-even bfloat16 -> float32 (what v_cvt_pk_bf16_f32 does to the operands of the bf16 kernel)."""
    u = numpy.ascontiguousarray(a, dtype=numpy.float32).view(numpy.uint32).astype(numpy.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(numpy.uint32).view(numpy.float32).reshape(numpy.shape(a))


# B, H, W, Cin, Cout, k, stride, pad, transposed, act, tile, splits   (bf16-operand implicit GEMM, BASELINE config #5)
CONV2D_BF16_CASES = [
    (1, 24, 32, 128, 128, 4, 2, 1, False, 'lrelu', '96x128', 1),           # k4 s2 convolution patch variant in bf16: 2 chunks x 4 parities
    (1, 12, 16, 256, 128, 4, 2, 1, True, 'relu', '96x128', 1),             # deconvolution patch variant in bf16: 4 chunks of 64 channels
    (1, 16, 16, 128, 64, 4, 2, 1, True, 'relu', '128x64k2', 1),            # 2 chunks, one per K group
    (1, 12, 16, 64, 128, 4, 2, 1, False, 'lrelu', '32x128', 0),
    (2, 16, 16, 64, 128, 4, 2, 1, False, 'lrelu', '128x128', 1),
    (1, 32, 64, 64, 128, 4, 2, 1, False, 'relu', '128x128', 2),        # 2-D tiles, split-K
    (1, 6, 10, 128, 64, 4, 2, 1, True, 'relu', '128x64', 0),           # deconv phases
    (1, 24, 32, 64, 128, 4, 2, 1, False, None, '96x128', 1),
    (1, 5, 7, 64, 128, 3, 1, 1, False, None, '64x128', 0),
]


def run_conv2d_bf16(ctx, rng, case, bn_params):
    """-> (y, oracle on bf16-rounded operands, oracle on fp32 operands)"""
    B, H, W_, Cin, Cout, k, s, p, tr, act, tile, splits = case
    x = rng.normal(size=(B, H, W_, Cin)).astype('f4')
    Wt = rng.normal(0, 0.1, size=(Cin, Cout, k, k) if tr else (Cout, Cin, k, k)).astype('f4')
    b = rng.normal(0, 0.1, Cout).astype('f4')
    bn = bn_params(rng, Cout)
    y = ctx.conv2d(x, Wt, b, bn, stride=s, pad=p, transposed=tr, act=act, path='igemm_bf16', tile=tile, splits=splits)
    outs = []
    for xx, ww in ((bf16_round(x), bf16_round(Wt)), (x, Wt)):
        xn = xx.transpose(0, 3, 1, 2)
        r = ops.deconv_nd(xn, ww, b, stride=s, pad=p) if tr else ops.conv_nd(xn, ww, b, stride=s, pad=p)
        outs.append(ops.apply_act(ops.batch_norm_inference(r, *bn), act).transpose(0, 2, 3, 1))
    return y, outs[0], outs[1]


def bf16_split(a):
    """float32 -> (hi, lo) with hi = bf16(a), lo = bf16(a - hi): the operands of the split-bf16 ('bf16x3') mode."""
    hi = bf16_round(a)
    return hi, bf16_round(numpy.asarray(a, dtype=numpy.float32) - hi)


# split-bf16 implicit GEMM (dtype 'bf16x3'): the bf16 cases (K axis three times as long) + odd chunk counts per source
CONV2D_X3_CASES = CONV2D_BF16_CASES + [
    (1, 12, 16, 192, 128, 4, 2, 1, True, 'relu', '96x128k2', 1),           # deconvolution patches: 9 chunks in K groups of 4 + 5
    (1, 16, 32, 64, 128, 4, 2, 1, False, 'lrelu', '64x128', 3),            # convolution patches: 12 (chunk, parity) units over 3 external splits
    (1, 6, 8, 128, 128, 3, 1, 1, False, 'relu', '32x128', 4),              # gather variant, 9 taps x 6 chunks over 4 splits
]


def run_conv2d_x3(ctx, rng, case, bn_params):
    """-> (y, float64 model of the kernel: x_hi w_hi + x_lo w_hi + x_hi w_lo, float64 oracle on the fp32 operands)"""
    B, H, W_, Cin, Cout, k, s, p, tr, act, tile, splits = case
    x = rng.normal(size=(B, H, W_, Cin)).astype('f4')
    Wt = rng.normal(0, 0.1, size=(Cin, Cout, k, k) if tr else (Cout, Cin, k, k)).astype('f4')
    b = rng.normal(0, 0.1, Cout).astype('f4')
    bn = bn_params(rng, Cout)
    y = ctx.conv2d(x, Wt, b, bn, stride=s, pad=p, transposed=tr, act=act, path='igemm_x3', tile=tile, splits=splits)
    f = (lambda xx, ww, bb: ops.deconv_nd(xx, ww, bb, stride=s, pad=p)) if tr else (lambda xx, ww, bb: ops.conv_nd(xx, ww, bb, stride=s, pad=p))
    (xh, xl), (wh, wl) = bf16_split(x), bf16_split(Wt)
    t = lambda a: a.transpose(0, 3, 1, 2).astype('f8')
    zero = numpy.zeros_like(b, dtype='f8')
    r3 = f(t(xh), wh.astype('f8'), b.astype('f8')) + f(t(xl), wh.astype('f8'), zero) + f(t(xh), wl.astype('f8'), zero)
    r = f(t(x), Wt.astype('f8'), b.astype('f8'))
    fin = lambda q: ops.apply_act(ops.batch_norm_inference(q, *bn), act).transpose(0, 2, 3, 1)
    return y, fin(r3), fin(r)


def x3_scaling_property(ctx, rng, case):
    """Size-independent exactness property of the split-bf16 path: scaling the input by a power of two commutes with the bf16
    hi / lo split and with every fp32 accumulation, so y(4 x) == 4 y(x) BIT FOR BIT (no bias, no BN, ReLU), and so does
    scaling the filters.  -> (y(x), y(4 x), y(x; W / 8))"""
    B, H, W_, Cin, Cout, k, s, p, tr, act, tile, splits = case
    x = rng.normal(size=(B, H, W_, Cin)).astype('f4')
    Wt = rng.normal(0, 0.1, size=(Cin, Cout, k, k) if tr else (Cout, Cin, k, k)).astype('f4')
    f = lambda xx, ww: ctx.conv2d(xx, ww, None, None, stride=s, pad=p, transposed=tr, act='relu', path='igemm_x3', tile=tile, splits=splits)
    return f(x, Wt), f(4.0 * x, Wt), f(x, Wt / 8.0)


def conv1d_operands(rng, case, bn_params):
    B, L, Cin, Cout, k, s, p, d, tr, act, splits = case
    x = rng.normal(size=(B, L, Cin)).astype('f4')
    W = rng.normal(0, 0.1, size=(Cin, Cout, k) if tr else (Cout, Cin, k)).astype('f4')
    b = rng.normal(0, 0.1, Cout).astype('f4')
    return x, W, b, bn_params(rng, Cout)


def run_conv1d(ctx, rng, case, bn_params, operands=None):
    B, L, Cin, Cout, k, s, p, d, tr, act, splits = case
    x, W, b, bn = operands or conv1d_operands(rng, case, bn_params)
    y = ctx.conv1d(x, W, b, bn, stride=s, pad=p, dilate=d, transposed=tr, act=act, splits=splits)
    xn = x.transpose(0, 2, 1)
    r = ops.deconv_nd(xn, W, b, stride=s, pad=p) if tr else ops.conv_nd(xn, W, b, stride=s, pad=p, dilate=d)
    r = ops.apply_act(ops.batch_norm_inference(r, *bn), act).transpose(0, 2, 1)
    return y, r


def run_conv2d(ctx, rng, case, bn_params):
    B, H, W_, Cin, Cout, k, s, p, tr, act, path, tile, splits = case
    x = rng.normal(size=(B, H, W_, Cin)).astype('f4')
    Wt = rng.normal(0, 0.1, size=(Cin, Cout, k, k) if tr else (Cout, Cin, k, k)).astype('f4')
    b = rng.normal(0, 0.1, Cout).astype('f4')
    bn = bn_params(rng, Cout)
    y = ctx.conv2d(x, Wt, b, bn, stride=s, pad=p, transposed=tr, act=act, path=path, tile=tile, splits=splits)
    xn = x.transpose(0, 3, 1, 2)
    r = ops.deconv_nd(xn, Wt, b, stride=s, pad=p) if tr else ops.conv_nd(xn, Wt, b, stride=s, pad=p)
    r = ops.apply_act(ops.batch_norm_inference(r, *bn), act).transpose(0, 2, 3, 1)
    return y, r


def oracle_forward(desc, P, x):
    """channels-last block -> oracle (NC...) -> channels-last."""
    if desc.ndim == 1:
        return unet.unet_forward(x.transpose(0, 2, 1), P, desc.extensive_layers).transpose(0, 2, 1)
    return unet.unet_forward(x[:, numpy.newaxis], P, desc.extensive_layers)[:, 0]


def poisoned_converts(ctx, net, sizes, monkeypatch, modes=('f32', 'bf16', 'bf16x3')):
    """RY_POISON=1 (round 5): every fresh stage-2 activation buffer -- fp32 and bf16 copies -- is filled with NaN patterns, so a kernel that reads a
    row / pixel / channel its producer did not write in THIS forward (dead-row crop, row ranges of a discard, skipped fp32 copies of the bf16
    modes) turns the result into NaN instead of depending on what the allocator handed out.  -> [(n, mode, NaNs, NaNs in the kept rows of a discard)]"""
    import ctypes
    reread = lambda: ctx.reload_env()
    out = []
    try:
        monkeypatch.setenv('RY_POISON', '1'); reread()
        for n, sp in sizes:
            for mode in modes:
                net.set_dtype(mode)                                   # drops the plans: the next convert builds poisoned buffers
                a = net.convert(sp)
                k = max(1, n // 3)
                b = net.convert(sp, discard=(k, k)) if n > 2 * k + 1 else a
                out.append((n, mode, int(numpy.isnan(a).sum()), int(numpy.isnan(b[k:n - k]).sum()) if n > 2 * k + 1 else 0))
    finally:
        monkeypatch.delenv('RY_POISON', raising=False); reread()
        net.set_dtype('f32')
    return out


def wino_properties(ctx, shape, transposed):
    """Size-independent properties of the Winograd operator (`path='wino'`, no activation: the operator is affine in its input) at any layer size:
    affinity y(x1 + x2) + y(0) = y(x1) + y(x2); equivariance -- the input shifted by two rows / columns (one for a transposed convolution) gives the
    output shifted by one (two) away from the borders: every pixel then falls on ANOTHER position of its Winograd tile or on another tile; external
    split-K sums the same products in another order.  Returns the three relative errors (the scale is max |y(x1)|)."""
    B, H, Wd, Cin, Cout = shape
    rng = numpy.random.default_rng(97)
    x1 = rng.normal(size=(B, H, Wd, Cin)).astype('f4'); x2 = rng.normal(size=(B, H, Wd, Cin)).astype('f4')
    Wt = rng.normal(0, 0.05, size=(Cin, Cout, 4, 4) if transposed else (Cout, Cin, 4, 4)).astype('f4')
    b = rng.normal(0, 0.1, Cout).astype('f4')
    kw = dict(stride=2, pad=1, transposed=transposed, act=None, path='wino')
    f = lambda x, **k: ctx.conv2d(x, Wt, b, None, **dict(kw, **k)).astype(numpy.float64)
    y1, y2, y12, y0 = f(x1), f(x2), f(x1 + x2), f(numpy.zeros_like(x1))
    scale = float(numpy.abs(y1).max())
    e_aff = float(numpy.abs(y12 + y0 - y1 - y2).max()) / scale
    si, so = (1, 2) if transposed else (2, 1)                       # input shift -> output shift
    xs = numpy.zeros_like(x1); xs[:, si:, si:] = x1[:, :-si, :-si]
    ys = f(xs)
    m = 2 * so + 2                                                  # margin: pixels whose stencil touches the border or the shifted-in zeros
    e_eq = float(numpy.abs(ys[:, so + m:-m, so + m:-m] - y1[:, m:-so - m, m:-so - m]).max()) / scale
    e_split = float(numpy.abs(f(x1, splits=3) - y1).max()) / scale
    return e_aff, e_eq, e_split


# ---- float64 reference with an element-wise error scale (tests/test_gemm_oracle.py) ----

def ref_conv2d_f64(x, W, b, bn, stride, pad, transposed, act):
    """The 2-D operator in float64 on the CPU: torch conv2d / conv_transpose2d, then the oracle's batch_norm_inference and apply_act.
    x (B, H, W, Cin) channels-last; W (Cout, Cin, k, k), or (Cin, Cout, k, k) when transposed (the layouts of ops_numpy).
    -> (r, bound), both (B, Ho, Wo, Cout) float64: bound = |s| (conv(|x|, |W|) + |b|) + |r| with s the folded BN scale (ReLU and leaky ReLU
    are 1-Lipschitz), the scale against which any fp32 summation order of the same sum is judged element by element."""
    import torch
    f = torch.nn.functional.conv_transpose2d if transposed else torch.nn.functional.conv2d
    xt = torch.from_numpy(numpy.ascontiguousarray(numpy.asarray(x, numpy.float64).transpose(0, 3, 1, 2)))
    wt = torch.from_numpy(numpy.asarray(W, numpy.float64))
    cout = W.shape[1] if transposed else W.shape[0]
    bb = numpy.zeros(cout) if b is None else numpy.asarray(b, numpy.float64)
    with torch.no_grad():
        c = f(xt, wt, torch.from_numpy(bb), stride=stride, padding=pad).numpy()
        ca = f(xt.abs(), wt.abs(), torch.from_numpy(numpy.abs(bb)), stride=stride, padding=pad).numpy()
    if bn is not None:
        bn64 = [numpy.asarray(v, numpy.float64) for v in bn]
        c = ops.batch_norm_inference(c, *bn64)
        s = numpy.abs(bn64[0] / numpy.sqrt(bn64[3] + ops.BN_EPS)).reshape(1, -1, 1, 1)
    else:
        s = 1.0
    r = ops.apply_act(c, act)
    bound = s * ca + numpy.abs(r)
    return r.transpose(0, 2, 3, 1), bound.transpose(0, 2, 3, 1)


def assert_close_elementwise(y, r, bound, tol, what=''):
    """Every element of y within tol * bound of the float64 reference r, and no NaN / Inf.  -> the worst ratio |y - r| / bound."""
    y = numpy.asarray(y, numpy.float64)
    assert y.shape == r.shape == bound.shape, (what, y.shape, r.shape, bound.shape)
    nonfinite = int((~numpy.isfinite(y)).sum())
    ratio = numpy.abs(y - r) / numpy.maximum(bound, 1e-300)
    ratio[~numpy.isfinite(y)] = numpy.inf
    i = numpy.unravel_index(int(numpy.argmax(ratio)), ratio.shape)
    worst = float(ratio[i])
    assert nonfinite == 0 and worst <= tol, ('%s: worst |y - r| / bound = %.3g > %.3g at (b, h, w, c) = %s (y %r, r %r, bound %.3g); %d NaN / Inf elements'
                                             % (what, worst, tol, tuple(int(v) for v in i), float(y[i]), float(r[i]), float(bound[i]), nonfinite))
    return worst


class poisoned(object):
    """with poisoned(ctx, monkeypatch): RY_POISON=1 for the block -- every output, slab and activation buffer the library allocates starts as NaN
    patterns, so an element the launch does not write in THIS call shows as NaN instead of a value left behind by an earlier call."""

    def __init__(self, ctx, monkeypatch):
        self.ctx, self.mp = ctx, monkeypatch

    def __enter__(self):
        self.mp.setenv('RY_POISON', '1'); self.ctx.reload_env()
        return self

    def __exit__(self, *exc):
        self.mp.delenv('RY_POISON', raising=False); self.ctx.reload_env()
        return False


def trained_like_operands(rng, B, H, W_, Cin, Cout, k, transposed):
    """Inputs behind a ReLU, filters ~ N(0, 0.02), bias ~ N(0, 0.1) and BatchNormalization statistics (conftest.bn_params)."""
    from conftest import bn_params
    x = numpy.maximum(rng.normal(size=(B, H, W_, Cin)), 0).astype('f4')
    Wt = rng.normal(0, 0.02, size=(Cin, Cout, k, k) if transposed else (Cout, Cin, k, k)).astype('f4')
    b = rng.normal(0, 0.1, Cout).astype('f4')
    return x, Wt, b, bn_params(rng, Cout)


# ---- which branches of the shared tile schedule a launch takes: labels for the case lists only, never used by a correctness assertion ----
# A restatement of fill_sched (ry_exec.cpp): the XCD grouping xcd_gs of ry_tile_decode (0 = no even split), the K units per split kq / krem of
# ry_split_range, and the M-tiles walked by ry_tile_pos (2-D tiles of th x tw pixels, or raster tiles of bm rows when tw = 0), for launches whose
# tile and external split are forced (the planner's choices are not restated).

def sched_of(case):
    """case of the CONV2D_CASES form with path 'wino' (tile (cfg, mbw)) or 'igemm' (fp32; tile name), tile and splits given."""
    B, H, W_, Cin, Cout, k, s, p, tr, act, path, tile, splits = case
    assert tile is not None and splits > 0, case
    Ho, Wo = (2 * H, 2 * W_) if tr else ((H + 2 * p - k) // s + 1, (W_ + 2 * p - k) // s + 1)
    Mh, Mw = (H, W_) if tr else (Ho, Wo)
    nphases, ntaps = (4, 4) if tr else (1, k * k)
    if path == 'wino':
        cfg, mbw = tile
        wm = 2 if cfg == 1 else 4
        th, tw = 8 * (wm // mbw), 16 * mbw
        bm, ntiles = th * tw, Cout // 64
        units = (1 if tr else 4) * (Cin // 16)
        wbytes = 2.25 * nphases * Cout * 4.0 * Cin
    else:
        bm, bn = (int(v) for v in tile.split('k')[0].split('x'))
        kg = 2 if tile.endswith('k2') else 1                     # (a forced split leaves the automatic K groups at one)
        cpt = Cin // 32
        nk = ntaps * cpt
        if splits * kg > nk:
            kg, splits = 1, min(splits, nk)
        tw = next((t for t in (16, 8, 4) if bm % t == 0 and Mw % t == 0 and Mh % (bm // t) == 0), 0)
        th = bm // tw if tw else 1
        patch = 0
        if tw == 16:
            if tr and splits * kg <= cpt:
                patch = 1
            elif not tr and k == 4 and s == 2 and p == 1 and splits * kg <= 4 * cpt:
                patch = 2
        units = cpt if patch == 1 else 4 * cpt if patch == 2 else nk
        ntiles = Cout // bn
        wbytes = float(nphases * Cout * ntaps * Cin)
    mtiles = B * (Mh // th) * (Mw // tw) if tw else -(-B * Mh * Mw // bm)
    nsl = splits * ntiles * nphases
    abytes = float(B * H * W_ * Cin)
    gs, best = 0, 1e300
    for sh in range(4):
        g, gm = 1 << sh, 8 >> sh
        if nsl % g or mtiles % gm:
            continue
        cost = gm * wbytes + g * abytes
        if cost < best:
            best, gs = cost, g
    return dict(kernel=path, xcd_gs=gs, kq=units // splits, krem=units % splits, splits=splits, units=units, tw=tw, B=B,
                ragged=(tw == 0 and (B * Mh * Mw) % bm != 0), mtiles=mtiles)


def sched_branches(case):
    """-> the set of schedule branches a case takes (see SCHED_BRANCHES)"""
    q = sched_of(case)
    out = {'xcd_gs=%d' % q['xcd_gs'], 'krem=0' if q['krem'] == 0 else 'krem>0'}
    if q['splits'] == q['units']:
        out.add('one unit per split')
    if q['B'] == 2 and q['tw'] > 0:
        out.add('batch 2 on 2-D tiles')
    if q['ragged']:
        out.add('ragged raster tile')
    return out


SCHED_BRANCHES = {'xcd_gs=0', 'xcd_gs=1', 'xcd_gs=2', 'xcd_gs=4', 'xcd_gs=8', 'krem=0', 'krem>0', 'one unit per split', 'batch 2 on 2-D tiles'}


# The case lists of the schedule branches on the emulator (tests/test_gemm_oracle.py): every branch of fill_sched / ry_tile_decode / ry_split_range
# for both LDS-DMA kernels, tile and external split forced (the labels of SCHED_BRANCHES come from sched_branches above)
SCHED_WINO_CASES = [
    (1, 8, 32, 16, 64, 4, 2, 1, True, 'relu', 'wino', (1, 2), 1),      # one patch, one split: contiguous runs per XCD (xcd_gs 0)
    (1, 24, 32, 64, 64, 4, 2, 1, True, None, 'wino', (1, 2), 4),       # four patches over four splits: one unit per split, 3 tile rows, xcd_gs 8
    (1, 16, 64, 16, 64, 4, 2, 1, False, 'lrelu', 'wino', (1, 2), 3),   # four (chunk, parity) patches over three splits: 2 + 1 + 1 (krem 1)
    (2, 64, 64, 16, 64, 4, 2, 1, False, 'lrelu', 'wino', (1, 1), 1),   # batch 2, eight M-tiles: xcd_gs 1 (eight M-tile groups)
    (1, 64, 64, 16, 64, 4, 2, 1, False, None, 'wino', (1, 1), 2),      # four M-tiles x two splits: xcd_gs 2
    (1, 8, 64, 16, 64, 4, 2, 1, True, 'lrelu', 'wino', (1, 2), 1),     # two M-tiles x four phases: xcd_gs 4
    (1, 8, 32, 16, 128, 4, 2, 1, True, 'lrelu', 'wino', (1, 2), 1),    # one M-tile, eight slices: xcd_gs 8
    (2, 32, 64, 48, 64, 4, 2, 1, False, None, 'wino', (2, 2), 5),      # eight waves, batch 2, twelve patches over five splits (krem 2)
    (2, 16, 32, 48, 128, 4, 2, 1, True, 'lrelu', 'wino', (2, 2), 2),   # eight waves, batch 2, three patches over two splits, xcd_gs 8
    (1, 32, 16, 32, 64, 4, 2, 1, True, None, 'wino', (2, 1), 2),       # eight waves, 32 x 16 tile, one patch per split
]
SCHED_IGEMM_CASES = [
    (1, 4, 8, 32, 64, 4, 2, 1, False, 'lrelu', 'igemm', '128x64', 3),  # 8 rows of one 128-row raster tile, 16 chunks over three splits (krem 1)
    (1, 4, 32, 32, 128, 4, 2, 1, False, None, 'igemm', '32x128', 4),   # 2 x 16 tile, 4 (chunk, parity) patches over four splits: one unit per split
    (2, 4, 8, 32, 128, 3, 1, 1, False, 'lrelu', 'igemm', '32x128', 1), # batch 2 on 4 x 8 tiles
    (1, 4, 64, 32, 128, 3, 1, 1, False, 'lrelu', 'igemm', '32x128', 1),# eight 2 x 16 tiles: xcd_gs 1
    (1, 4, 32, 32, 128, 3, 1, 1, False, None, 'igemm', '32x128', 2),   # four tiles x two splits of 9 taps (5 + 4): xcd_gs 2
    (1, 4, 12, 32, 128, 3, 1, 1, False, 'lrelu', 'igemm', '32x128', 4),# 48 rows on two raster tiles (ragged), 9 taps over four splits: xcd_gs 4
    (1, 4, 8, 32, 64, 4, 2, 1, False, None, 'igemm', '128x64', 8),     # one ragged raster tile x eight splits: xcd_gs 8
    (2, 8, 16, 64, 128, 4, 2, 1, True, 'lrelu', 'igemm', '64x128', 2), # sub-pixel deconvolution, batch 2 on 4 x 16 tiles, two patches over two splits
    (1, 6, 8, 64, 256, 4, 2, 1, True, None, 'igemm', '96x128k2', 3),   # two K groups x three splits, deconvolution on a ragged raster tile
    (2, 16, 32, 64, 128, 4, 2, 1, False, 'lrelu', 'igemm', '96x128', 3),  # batch 2 on raster tiles that cross the image boundary, 32 chunks / 3
]


# the full-size layers of SYN-64 at the 300-frame window (T = 384) the GPU suite runs (tests/test_gpu_parity.py, tests/test_gemm_oracle.py)
OS_FULL_SIZE = [          # the weight-streaming bottom, planner's slice (B, H, W, Cin, Cout, k, s, p, transposed, act, path, tile, splits)
    (1, 6, 8, 512, 512, 4, 2, 1, False, 'lrelu', 'os', None, 0),          # encoder c7: 12 pixels, 16.8 MB of filters
    (1, 12, 16, 512, 512, 4, 2, 1, False, 'lrelu', 'os', None, 0),        # encoder c6: 48 pixels
    (1, 3, 4, 512, 512, 4, 2, 1, True, 'relu', 'os', None, 0),            # decoder c0
    (1, 6, 8, 1024, 512, 4, 2, 1, True, 'relu', 'os', None, 0),           # decoder c1: two sources of 512 channels, 33.5 MB
]

WINO_FULL_SIZE = [        # the eight MFMA-bound layers, the planner's plan: B, H, W, Cin, Cout, transposed
    (1, 384, 512, 64, 128, False), (1, 192, 256, 128, 256, False), (1, 96, 128, 256, 512, False), (1, 48, 64, 512, 512, False),      # encoder c1 .. c4
    (1, 24, 32, 1024, 512, True), (1, 48, 64, 1024, 256, True), (1, 96, 128, 512, 128, True), (1, 192, 256, 256, 64, True),          # decoder c3 .. c6
    (2, 48, 64, 1024, 256, True),                                                                                                     # two windows per call
]

X3_FULL_SIZE = [
    (1, 48, 64, 1024, 256, 4, 2, 1, True, 'relu', None, 0),        # decoder c4 (planner's tile / splits)
    (1, 96, 128, 256, 512, 4, 2, 1, False, 'relu', None, 0),       # encoder c3
]


# ---- stage 1: the float64 reference of a 1-D layer and the branches of ry_c1d_os (tests/test_stage1_oracle.py) ----

def ref_conv1d_f64(xa, xb, W, b, bn, stride, pad, dilate, transposed, act, n_real=0, keep=0):
    """The 1-D operator in float64 on the CPU, the counterpart of ref_conv2d_f64: torch conv1d / conv_transpose1d on concat(xa, xb) over the
    channels, the oracle's batch_norm_inference and apply_act.  xa (B, L, Ca), xb (B, L, Cb) or None, channels-last; W (Cout, Cin, k), or
    (Cin, Cout, k) when transposed.  n_real > 0: the fused pad -- rows n_real .. L - 1 of xa are replaced by the column minimum of its real rows
    (what xa holds there is ignored).  keep > 0: the first keep output rows.  -> (r, bound), both (B, keep or Lout, Cout') float64, Cout' = Cout / 2
    for GLU.  bound = |s| (conv(|x|, |W|) + |b|) + |r| per element (s the folded BN scale); for GLU y = a sigmoid(g) it is B_a + |a| B_g / 4 + |y|
    with B_a, B_g the pre-activation bounds of the two halves (sigmoid is 1/4-Lipschitz and below 1)."""
    import torch
    x = numpy.asarray(xa, numpy.float64)
    if n_real > 0:
        x = x.copy()
        x[:, n_real:] = x[:, :n_real].min(axis=1, keepdims=True)
    if xb is not None:
        x = numpy.concatenate([x, numpy.asarray(xb, numpy.float64)], axis=2)
    f = torch.nn.functional.conv_transpose1d if transposed else torch.nn.functional.conv1d
    xt = torch.from_numpy(numpy.ascontiguousarray(x.transpose(0, 2, 1)))
    wt = torch.from_numpy(numpy.asarray(W, numpy.float64))
    cout = W.shape[1] if transposed else W.shape[0]
    bb = numpy.zeros(cout) if b is None else numpy.asarray(b, numpy.float64)
    kw = dict(stride=stride, padding=pad) if transposed else dict(stride=stride, padding=pad, dilation=dilate)
    with torch.no_grad():
        c = f(xt, wt, torch.from_numpy(bb), **kw).numpy()
        ca = f(xt.abs(), wt.abs(), torch.from_numpy(numpy.abs(bb)), **kw).numpy()
    if bn is not None:
        bn64 = [numpy.asarray(v, numpy.float64) for v in bn]
        c = ops.batch_norm_inference(c, *bn64)
        s = numpy.abs(bn64[0] / numpy.sqrt(bn64[3] + ops.BN_EPS)).reshape(1, -1, 1)
    else:
        s = 1.0
    pre = s * ca                                                   # bound of each pre-activation element
    r = ops.apply_act(c, act)
    if act == 'glu':
        h = cout // 2
        bound = pre[:, :h] + numpy.abs(c[:, :h]) * pre[:, h:] / 4 + numpy.abs(r)
    else:
        bound = pre + numpy.abs(r)
    r, bound = r.transpose(0, 2, 1), bound.transpose(0, 2, 1)
    if keep:
        r, bound = r[:, :keep], bound[:, :keep]
    return r, bound


def stage1_operands(rng, B, L, Ca, Cb, Cout, k, transposed, trained=True):
    """Sources, filters over Ca + Cb channels, bias and BN of one stage-1 layer.  trained: inputs behind a ReLU and filters ~ N(0, 0.02) as in
    trained_like_operands; else signed inputs (a first layer's features) and filters ~ N(0, 0.1)."""
    from conftest import bn_params
    xa = rng.normal(size=(B, L, Ca)); xb = rng.normal(size=(B, L, Cb)) if Cb else None
    if trained:
        xa = numpy.maximum(xa, 0); xb = None if xb is None else numpy.maximum(xb, 0)
    C = Ca + Cb
    W = rng.normal(0, 0.02 if trained else 0.1, size=(C, Cout, k) if transposed else (Cout, C, k)).astype('f4')
    return (xa.astype('f4'), None if xb is None else xb.astype('f4'), W, rng.normal(0, 0.1, Cout).astype('f4'), bn_params(rng, Cout))


# Which instantiation and which loops of ry_c1d_os (ry_kernels.h) a launch takes, restated from the kernel and launch_c1d_os (ry_exec.cpp): labels for
# the case lists only, never used by a correctness assertion.  Case form (B, L, Ca, Cb, Cout, k, stride, pad, transposed, act, (cb, tp), n_real, keep):
# L = rows per window of the sources (the padded length when n_real > 0), the slice forced.

def os1_of(case):
    B, L, Ca, Cb, Cout, k, s, p, tr, act, tile, n_real, keep = case
    mode = 2 if tr else 0 if (k, s, p) == (4, 2, 1) else 1
    assert mode != 1 or (s == 1 and p <= 3), case
    cb, tp = tile
    ctot = Ca + Cb
    kt = 1 if ctot <= 64 else 2 if ctot <= 128 else 4
    pg = 4 // kt
    tpo = 2 * tp if mode == 2 else tp
    np_ = 2 * tp + 2 if mode == 0 else tp + 2 if mode == 2 else tp + 3
    quad = (np_ + 4 * cb) * 4 + cb * tpo <= 200                    # the register budget of four channel sets in flight
    lout = 2 * L if tr else (L + 2 * p - k) // s + 1
    rows = L if tr else lout                                       # the axis the position tiles walk
    loops = set()
    for kw in range(kt):                                           # the channel-set loops of each ci wave
        c0, step, seen = kw * 64, kt * 64, False
        while quad and c0 + 3 * step < ctot:
            c0 += 4 * step; loops.add('quad'); seen = True
        while c0 + step < ctot:
            c0 += 2 * step; loops.add('pair'); seen = True
        if c0 < ctot:
            loops.add('single'); seen = True
        if not seen:
            loops.add('empty wave')
    usrc = Cb == 0 or Ca % 64 == 0
    return dict(inst='<%d,%d,%d,%s,%s>' % (mode, cb, tp, 'true' if n_real else 'false', 'true' if usrc else 'false'), mode=mode, kt=kt,
                loops=loops, lout=lout, ragged_tile=rows % (pg * tp) != 0, ctot=ctot)


def os1_branches(case):
    B, L, Ca, Cb, Cout, k, s, p, tr, act, tile, n_real, keep = case
    o = os1_of(case)
    out = {'inst ' + o['inst'], 'kt=%d' % o['kt']} | o['loops']
    if Cout == 9:
        out.add('Cout 9')
    if Cout % tile[0]:
        out.add('Cout %% %d != 0' % tile[0])
    if o['ctot'] in (9, 65, 129, 523):
        out.add('Ctot %d' % o['ctot'])
    if o['ragged_tile']:
        out.add('ragged last tile')
    if B == 2:
        out.add('B=2')
    if keep and keep < o['lout']:
        out.add('keep < Lout')
    if o['mode'] == 0 and L == 2:
        out.add('stride 2 from 2 rows to 1')
    if o['mode'] == 2 and L == 1:
        out.add('deconvolution from 1 row to 2')
    if o['mode'] == 1:
        out.add('S1 k=%d pad %d' % (k, p))
    if Cb:
        out.add('two sources, Ca %% 64 %s 0' % ('==' if Ca % 64 == 0 else '!='))
    return out


# what the forced-slice list must reach (tests/test_stage1_oracle.py::test_os1_cases_cover_every_branch)
OS1_INSTANTIATIONS = {'inst <0,%d,%d,false,true>' % t for t in ((4, 8), (4, 4), (2, 8), (2, 4))} | {'inst <0,2,4,false,false>'} | \
    {'inst <1,%d,%d,%s,true>' % (c, t, pm) for c, t in ((4, 8), (4, 4), (2, 8), (2, 4)) for pm in ('false', 'true')} | {'inst <1,2,4,false,false>'} | \
    {'inst <2,%d,%d,false,true>' % t for t in ((4, 4), (2, 8), (2, 4))} | {'inst <2,2,4,false,false>'}
OS1_BRANCHES = OS1_INSTANTIATIONS | {'kt=1', 'kt=2', 'kt=4', 'quad', 'pair', 'single', 'empty wave', 'Cout 9', 'Cout % 2 != 0', 'Cout % 4 != 0',
                                     'Ctot 9', 'Ctot 65', 'Ctot 129', 'Ctot 523', 'ragged last tile', 'B=2', 'keep < Lout',
                                     'stride 2 from 2 rows to 1', 'deconvolution from 1 row to 2',
                                     'two sources, Ca % 64 == 0', 'two sources, Ca % 64 != 0'} | \
    {'S1 k=%d pad %d' % (k, p) for k in (1, 3) for p in range(4)}

# B, L, Ca, Cb, Cout, k, stride, pad, transposed, act, (cb, tp), n_real, keep
OS1_CASES = [
    # k4 s2 p1 convolution (mode 0)
    (2, 66, 9, 0, 9, 4, 2, 1, False, 'lrelu', (4, 8), 0, 0),        # Ctot 9, Cout 9 on CB 4, batch 2, 33 rows on 32-row tiles
    (1, 40, 65, 0, 10, 4, 2, 1, False, 'relu', (4, 4), 0, 0),       # Ctot 65: two ci waves of one set each; 20 rows on 8-row tiles
    (1, 34, 129, 0, 7, 4, 2, 1, False, 'lrelu', (2, 8), 0, 0),      # Ctot 129: four ci waves, the last one without a channel set; Cout 7 on CB 2
    (1, 2, 64, 0, 16, 4, 2, 1, False, 'lrelu', (2, 4), 0, 0),       # the U-Net's deepest encoder layer: 2 rows -> 1
    (1, 20, 40, 30, 12, 4, 2, 1, False, 'lrelu', (2, 4), 0, 0),     # two sources split inside a wave (the per-lane form)
    (1, 24, 1100, 0, 6, 4, 2, 1, False, None, (4, 4), 0, 5),        # 1100 channels: four sets in flight, then one; keep 5 of 12
    # stride-1 convolution (mode 1): k 1 / 3, pad 0 .. 3
    (1, 37, 9, 0, 9, 3, 1, 1, False, 'lrelu', (4, 8), 0, 0),        # encoder c0 shape, 37 rows on 32-row tiles
    (2, 21, 64, 0, 64, 1, 1, 0, False, 'relu', (4, 4), 0, 0),       # a 'same' decoder layer
    (1, 19, 9, 0, 9, 3, 1, 0, False, None, (2, 8), 0, 0),
    (1, 13, 16, 0, 10, 3, 1, 2, False, 'lrelu', (2, 4), 0, 0),
    (1, 11, 523, 0, 9, 3, 1, 3, False, 'lrelu', (4, 8), 0, 0),      # the 523-channel input: four ci waves, a pair and a single set
    (1, 9, 65, 0, 11, 1, 1, 1, False, None, (4, 8), 0, 0),
    (1, 15, 129, 0, 9, 1, 1, 2, False, 'relu', (2, 8), 0, 0),
    (1, 10, 9, 0, 5, 1, 1, 3, False, 'lrelu', (2, 4), 0, 0),
    (2, 30, 64, 64, 9, 3, 1, 1, False, None, (4, 4), 0, 27),        # decoder c7 shape: two sources on a wave boundary, keep < Lout
    (1, 30, 40, 25, 9, 3, 1, 1, False, None, (2, 4), 0, 0),         # two sources split inside a wave
    # k4 s2 p1 deconvolution (mode 2)
    (1, 1, 64, 0, 16, 4, 2, 1, True, 'relu', (4, 4), 0, 0),         # the U-Net's deepest decoder layer: 1 row -> 2
    (2, 11, 128, 64, 9, 4, 2, 1, True, 'relu', (2, 8), 0, 0),       # two sources on a wave boundary, 11 rows on 8-row tiles
    (1, 7, 64, 64, 13, 4, 2, 1, True, 'relu', (2, 4), 0, 0),
    (1, 5, 512, 512, 10, 4, 2, 1, True, 'relu', (4, 4), 0, 0),      # decoder c1's channels: four sets in flight per ci wave
    (1, 9, 30, 35, 7, 4, 2, 1, True, 'relu', (2, 4), 0, 0),         # two sources split inside a wave
]

# the fused pad of the convert wrapper (mode 1, PADMIN): n_real real rows padded to L = n_real + 128 - n_real % 128 (netspec.pad_frames)
OS1_PAD_CASES = [
    (1, 128, 9, 0, 64, 3, 1, 1, False, 'lrelu', (4, 8), 1, 0),      # fewer real rows than the four row groups of the minimum
    (1, 128, 1, 0, 16, 3, 1, 1, False, 'lrelu', (4, 4), 2, 0),
    (1, 128, 64, 0, 9, 3, 1, 1, False, 'lrelu', (2, 8), 3, 0),
    (2, 128, 9, 0, 64, 3, 1, 1, False, 'lrelu', (2, 4), 63, 0),     # around the 64-row stride of the minimum loop
    (1, 128, 64, 0, 9, 1, 1, 0, False, None, (4, 8), 64, 0),
    (1, 256, 1, 0, 10, 3, 1, 1, False, 'lrelu', (4, 4), 65, 0),
    (1, 384, 9, 0, 64, 3, 1, 1, False, 'lrelu', (4, 8), 300, 0),    # encoder c0 of the 300-frame window
    (1, 384, 64, 0, 12, 3, 1, 2, False, 'relu', (2, 8), 300, 0),
]


def syn64_stage1_layers(frames, stage1_in=9):
    """[(case, name)] of the 16 layers of the SYN-64 stage-1 predictor in a convert of `frames` frames (T = frames + netspec.pad_frames(frames) rows),
    in the case form of OS1_CASES with the planner's slice (None), shapes from netspec.param_list: encoder c0 takes the fused pad (n_real = frames),
    decoder c1 .. c7 two sources (the decoder chain, the encoder skip), decoder c7 keeps the real frames."""
    from realtime_yukarin_amd import netspec, synth
    d = synth.model_descs('SYN-64', stage1_in)[0]
    assert not d.glu
    W = dict(netspec.param_list(d))
    T = frames + netspec.pad_frames(frames)
    out, enc_len, L = [], [], T
    for i in range(8):
        name = 'encoder/c%d' % i
        co, ci, k = W[name + ('/W' if i == 0 else '/c/W')]
        s, p = (1, k // 2) if i == 0 else (2, 1) if netspec.enc_sample(d, i) == 'down' else (1, 0)
        out.append(((1, L, ci, 0, co, k, s, p, False, 'lrelu', None, frames if i == 0 else 0, 0), name))
        L = (L + 2 * p - k) // s + 1
        enc_len.append(L)
    for j in range(8):
        name = 'decoder/c%d' % j
        if j == 7:
            co, ci, k = W[name + '/W']
            up, s, p = False, 1, k // 2
        else:
            up = netspec.dec_sample(d, j) == 'up'
            w = W[name + '/c/W']
            (ci, co, k), (s, p) = (w, (2, 1)) if up else ((w[1], w[0], w[2]), (1, 0))
        cb = 0 if j == 0 else (d.base if j == 7 else netspec.ENC_CH[7 - j] * d.base)
        assert cb == 0 or enc_len[7 - j if j < 7 else 0] == L, (name, L)
        act = None if j == 7 else 'relu'
        out.append(((1, L, ci - cb, cb, co, k, s, p, up, act, None, 0, frames if j == 7 else 0), name))
        L = 2 * L if up else (L + 2 * p - k) // s + 1
    assert L == T
    return out


# ---- the stage-2 convert graph, node by node (tests/test_stage2_graph_oracle.py) ----
# Every layer is restated in float64 on the sources the DEVICE read (engine.Net.debug_activation after the run), so errors do not chain and the bar of a
# layer is one layer's summation error; a poisoned element a node should have written is NaN at that node.

def s2_layers(desc):
    """The 16 layers of a stage-2 predictor restated from oracle/unet.py (never from the library): name, parameter key, stencil, activation, sources
    (-1: the padded input; None: no second source)."""
    e = int(desc.extensive_layers)
    ek = 3 if e > 0 else 1
    L = [dict(name='encoder/c0', key='encoder/c0', k=ek, s=1, p=ek // 2, tr=False, act='lrelu', bn=None, src=(-1, None))]
    for i in range(1, 8):
        dn = i < e
        L.append(dict(name='encoder/c%d' % i, key='encoder/c%d/c' % i, k=4 if dn else 1, s=2 if dn else 1, p=1 if dn else 0, tr=False, act='lrelu',
                      bn='encoder/c%d/batchnorm/' % i, src=(i - 1, None)))
    for j in range(7):
        up = (7 - j) < e
        L.append(dict(name='decoder/c%d' % j, key='decoder/c%d/c' % j, k=4 if up else 1, s=2 if up else 1, p=1 if up else 0, tr=up, act='relu',
                      bn='decoder/c%d/batchnorm/' % j, src=(7, None) if j == 0 else (7 + j, 7 - j)))
    L.append(dict(name='decoder/c7', key='decoder/c7', k=ek, s=1, p=ek // 2, tr=False, act=None, bn=None, src=(14, 0)))
    return L


def s2_rows_read(spec, a, b, Hi):
    """Input rows [lo, hi) that output rows [a, b) of a layer read, from the operator's stencil: a convolution's output row o reads input rows
    o s - p .. o s - p + k - 1; a k4 s2 p1 transposed convolution's input row i feeds output rows o = 2 i - 1 + k', k' = 0 .. 3, so output row o reads
    the input rows i with 0 <= o + 1 - 2 i <= 3."""
    if b <= a:
        return 0, 0
    if spec['tr']:
        lo, hi = -((2 - a) // 2), b // 2 + 1                       # ceil((a - 2) / 2) .. floor(b / 2)
    else:
        lo, hi = a * spec['s'] - spec['p'], (b - 1) * spec['s'] - spec['p'] + spec['k']
    return max(lo, 0), min(hi, Hi)


def s2_needed_rows(specs, heights, k0, k1):
    """Output rows [a, b) of every layer that the kept frames [k0, k1) of a window depend on: the last layer writes rows [k0, k1); walking the decoder chain
    back, a layer's needed rows are what its consumer reads of it; the encoder (it feeds the bottom of the U-Net) and with it the skip sources are needed
    whole.  heights[i] = output rows of layer i."""
    need = [(0, heights[i]) for i in range(16)]
    need[15] = (k0, k1)
    for i in range(15, 8, -1):
        Hi = heights[specs[i]['src'][0]]
        need[i - 1] = s2_rows_read(specs[i], need[i][0], need[i][1], Hi)
    return need


def bf16_bits_to_f32(u):
    return (numpy.asarray(u, numpy.uint16).astype(numpy.uint32) << 16).view(numpy.float32)


def f32_to_bf16_bits(a):
    return (numpy.ascontiguousarray(a, numpy.float32).view(numpy.uint32) >> 16).astype(numpy.uint16)


def s2_value16(u):
    """The value a consumer rebuilds from a 16-bit copy (Net.debug_activation kind 1): bf16, or hi + lo of the split form (B, H, W, 2, C) -> float64"""
    f = bf16_bits_to_f32(u).astype(numpy.float64)
    return f[..., 0, :] + f[..., 1, :] if u.ndim == 5 else f


def s2_fetch(net, layer, kind):
    """-> the buffer, or None when this plan has none (the library refuses with RY_EINVAL and says which copy is missing)"""
    from realtime_yukarin_amd import _lib
    try:
        return net.debug_activation(layer, kind)
    except _lib.Ry355Error as e:
        assert any(w in str(e) for w in ('writes no', "caller's block", 'was not written', 'no padded input')), e
        return None


def s2_layer_params(P, spec, bf16):
    W, b = P[spec['key'] + '/W'], P[spec['key'] + '/b']
    bn = None if spec['bn'] is None else tuple(P[spec['bn'] + n] for n in ('gamma', 'beta', 'avg_mean', 'avg_var'))
    return (bf16_round(W) if bf16 else W), b, bn


def nan_rows(a):
    """rows (axis 1) of a (B, H, ...) block that hold a NaN in any window"""
    a = numpy.asarray(a)
    return numpy.isnan(a.reshape(a.shape[0], a.shape[1], -1)).any(axis=(0, 2))


def s2_reads_16bit(prof):
    """{layer name: True} for the layers whose kernel reads the producers' 16-bit copies: the implicit GEMM instantiated with BF16 = true (the sixth
    template argument of its name in Net.profile).  Which of the two 16-bit formats it reads is what the producer's copy says."""
    return {q['layer'] for q in prof if q['name'].startswith('ry_igemm_ldsdma<') and q['name'][:-1].split(',')[5] == 'true'}


def s2_band_reference(spec, srcs_rows, W, bb, bn, a, b, Hi):
    """The float64 reference of output rows [a, b) of one layer alone, from the source rows their stencil reads and nothing else.
    srcs_rows(lo, hi) -> the float64 sources' rows [lo, hi) (B, hi - lo, W, C each); Hi = the sources' rows.  The row axis is laid out by hand (rows outside
    the image are zeros, as the operator's padding has them) and the operator runs with no row padding of its own.  -> (r, bound), (B, b - a, Wo, Cout)"""
    if spec['tr']:          # k4 s2 p1 transposed: input row i feeds output rows 2 i - 1 + k'; with no row padding the slice's local row j is output row j + 2 ia - 1
        ia, ib = s2_rows_read(spec, a, b, Hi)
        xs = numpy.concatenate(srcs_rows(ia, ib), axis=3)
        r, bound = ref_conv2d_f64(xs, W, bb, bn, spec['s'], (0, spec['p']), True, spec['act'])
        off = 2 * ia - 1
        return r[:, a - off:b - off], bound[:, a - off:b - off]
    lo, hi = a * spec['s'] - spec['p'], (b - 1) * spec['s'] - spec['p'] + spec['k']          # unclamped: output row a starts at source row lo
    ia, ib = max(lo, 0), min(hi, Hi)
    xs = numpy.concatenate(srcs_rows(ia, ib), axis=3)
    xs = numpy.pad(xs, [(0, 0), (ia - lo, hi - ib), (0, 0), (0, 0)])
    r, bound = ref_conv2d_f64(xs, W, bb, bn, spec['s'], (0, spec['p']), False, spec['act'])
    assert r.shape[1] == b - a, (spec['name'], r.shape, a, b)
    return r, bound


def s2_walk(net, desc, P, n_frames, y, discard=(0, 0), prof=(), refs=True, cache=None, out=None, what='', layers=None, bands=None, x_in=None):
    """After y = net.convert(sp, discard) on a fresh, poisoned plan: every layer of the graph against float64 on the device's own sources.
    refs: True = every layer; False = finiteness of the needed rows only (the caller checks the last layer).  cache: {layer: (sources, r, bound)} of an
    earlier run of the same window and mode -- its reference is taken over for a layer whose sources are bit-equal on every row the needed rows read.
    layers: the layer indices held to float64 (None: all of them); every other layer gets what refs=False gives every layer.
    bands: {layer: [(a, b), ...]} -- that layer is held to float64 on these output row ranges only (clipped to its needed rows), each against a reference
    of the band alone (s2_band_reference); the finiteness / NaN-row rule still covers every row.
    x_in: the padded block of a raw forward (net.forward(x_in) ran, n_frames = its rows): the plan has no padded input of its own.
    -> dict(layers=[per-layer report], need, bufs={layer: value array}, fused)"""
    specs = s2_layers(desc)
    B = y.shape[0]
    k0 = discard[0] if discard[0] < n_frames else 0
    k1 = n_frames - discard[1] if n_frames - discard[1] > k0 else n_frames
    reads16 = s2_reads_16bit(prof)
    if x_in is None:
        x_in = s2_fetch(net, -1, 0)
    assert x_in is not None
    T = x_in.shape[1]
    raw = {}
    for i in range(16):
        raw[i] = (s2_fetch(net, i, 0), s2_fetch(net, i, 1))
    fused = raw[15][0] is None                                    # the 3x3 end layer wrote exp / edge bin / crop into the caller's block itself
    heights = [(raw[i][0] if raw[i][0] is not None else raw[i][1]).shape[1] if i < 15 or not fused else T for i in range(16)]
    assert heights[15] == T and heights[0] == T
    need = s2_needed_rows(specs, heights, k0, k1)
    if not fused:
        need[15] = (0, n_frames)                                  # the separate end layer computes every real row (ry_sr_post then stores the kept ones)
        for i in range(15, 8, -1):
            need[i - 1] = s2_rows_read(specs[i], need[i][0], need[i][1], heights[specs[i]['src'][0]])
    rep = []
    for i, spec in enumerate(specs):
        o32, o16 = raw[i]
        a, b = need[i]
        is16 = spec['name'] in reads16
        held, fmts = [], []                                       # the sources as the device holds them: (block, is it a 16-bit copy)
        for sidx in spec['src']:
            if sidx is None:
                continue
            if sidx < 0:
                held.append((x_in[..., None], False)); fmts.append('f32'); continue
            s32, s16 = raw[sidx]
            if is16:
                assert s16 is not None, (what, spec['name'], 'reads a 16-bit copy that layer %d does not write' % sidx)
                held.append((s16, True)); fmts.append('x3' if s16.ndim == 5 else 'bf16')
            else:
                assert s32 is not None, (what, spec['name'], 'reads an fp32 copy that layer %d does not write' % sidx)
                held.append((s32, False)); fmts.append('f32')
        assert len(set(fmts)) == 1, (what, spec['name'], fmts)
        srcs_rows = lambda lo, hi, held=held: [s2_value16(u[:, lo:hi]) if h16 else u[:, lo:hi].astype(numpy.float64) for u, h16 in held]
        fmt = fmts[0]
        tol = dict(f32=F32_TOL, bf16=BF16_TOL, x3=X3_TOL)[fmt]
        q = dict(layer=spec['name'], fmt=fmt, need=(a, b), worst=None, worst16=None, nan32=None, nan16=None, reused=False, held=False, banded=None)
        if i == 15 and fused:
            rep.append(q)
            continue
        for kind, o in (('nan32', o32), ('nan16', o16)):
            if o is None:
                continue
            nr = nan_rows(o if kind == 'nan32' else s2_value16(o))
            q[kind] = int(nr.sum())
            assert not nr[a:b].any(), (what, spec['name'], kind, 'needed rows %d .. %d hold NaN: rows %s' % (a, b - 1, numpy.nonzero(nr[a:b])[0][:8] + a))
        if o32 is not None and o16 is not None:                   # the 16-bit copy is the rounding of its fp32 twin, bit for bit (NaN rows: both NaN)
            ok = ~numpy.isnan(o32)
            if o16.ndim == 5:
                hi, lo = bf16_split(numpy.where(ok, o32, 0))
                want = numpy.stack([f32_to_bf16_bits(hi), f32_to_bf16_bits(lo)], axis=3)
                okk = ok[:, :, :, None, :]
            else:
                want = f32_to_bf16_bits(bf16_round(numpy.where(ok, o32, 0))); okk = ok
            bad = (want != o16) & okk
            assert not bad.any(), (what, spec['name'], '%d elements of the 16-bit copy are not the rounding of the fp32 copy' % int(bad.sum()))
            assert numpy.isnan(s2_value16(o16))[~ok].all(), (what, spec['name'], 'the 16-bit copy holds values where the fp32 copy is NaN')
        if not refs or (layers is not None and i not in layers):
            rep.append(q)
            continue
        q['held'] = True
        Hi = held[0][0].shape[1]

        def compare(a_, b_, rr, bd):
            """rows [a_, b_) of this layer's output against their reference -> (worst, worst16)"""
            assert numpy.isfinite(rr).all(), (what, spec['name'], 'the reference of a needed row read a NaN source row')
            if o32 is not None:
                return assert_close_elementwise(o32[:, a_:b_], rr, bd, tol, '%s %s fp32 rows %d..%d' % (what, spec['name'], a_, b_ - 1)), None
            v = s2_value16(o16[:, a_:b_])
            if o16.ndim == 5:      # hi + lo rebuilds the fp32 value to 2^-17 of it (lo = bf16(v - hi), |v - hi| <= 2^-9 |v|, rounded to 8 bits again)
                return None, assert_close_elementwise(v, rr, bd + (2.0 ** -17 / tol) * numpy.abs(rr), tol, '%s %s split copy' % (what, spec['name']))
            # rounding is monotone: the stored bf16 lies between the roundings of the two ends of the fp32 value's interval
            lo_, hi_ = bf16_round((rr - tol * bd).astype(numpy.float32)), bf16_round((rr + tol * bd).astype(numpy.float32))
            lo_ = numpy.minimum(lo_, bf16_round(numpy.nextafter((rr - tol * bd).astype(numpy.float32), numpy.float32(-numpy.inf))))   # (float64 -> float32 may round inwards)
            hi_ = numpy.maximum(hi_, bf16_round(numpy.nextafter((rr + tol * bd).astype(numpy.float32), numpy.float32(numpy.inf))))
            bad = ~((v >= lo_) & (v <= hi_))
            assert not bad.any(), ('%s %s bf16 copy: %d elements outside bf16([r - tol bound, r + tol bound])' % (what, spec['name'], int(bad.sum())))
            return None, float((numpy.abs(v - rr) / numpy.maximum(bd, 1e-300)).max())

        W, bb, bn = s2_layer_params(P, spec, fmt == 'bf16')
        if bands is not None and i in bands:
            q['banded'] = []
            for a_, b_ in bands[i]:
                a_, b_ = max(a_, a), min(b_, b)
                if b_ <= a_:
                    continue
                rr, bd = s2_band_reference(spec, srcs_rows, W, bb, bn, a_, b_, Hi)
                w32, w16 = compare(a_, b_, rr, bd)
                q['worst'] = w32 if q['worst'] is None else max(q['worst'], w32) if w32 is not None else q['worst']
                q['worst16'] = w16 if q['worst16'] is None else max(q['worst16'], w16) if w16 is not None else q['worst16']
                q['banded'].append((a_, b_))
            assert q['banded'], (what, spec['name'], 'no band inside the needed rows %d .. %d' % (a, b - 1))
            rep.append(q)
            continue
        ra, rb = s2_rows_read(spec, a, b, Hi)
        srcs = srcs_rows(0, Hi)
        hit = cache.get(i) if cache is not None else None
        if hit is not None and len(hit[0]) == len(srcs) and all(numpy.array_equal(u[:, ra:rb], v[:, ra:rb]) for u, v in zip(hit[0], srcs)):
            r, bound = hit[1], hit[2]; q['reused'] = True
        else:
            xs = numpy.concatenate(srcs, axis=3) if len(srcs) > 1 else srcs[0]
            r, bound = ref_conv2d_f64(xs, W, bb, bn, spec['s'], spec['p'], spec['tr'], spec['act'])
            if cache is not None:
                cache[i] = (srcs, r, bound)
        q['worst'], q['worst16'] = compare(a, b, r[:, a:b], bound[:, a:b])
        rep.append(q)
    return dict(layers=rep, need=need, raw=raw, x_in=x_in, fused=fused, k=(k0, k1), specs=specs)


def s2_check_end(walk, P, y, n_frames, E, what=''):
    """The end of a convert against float64.  Fused end layer (ry_sr_last / ry_sr_last_gather): |log y - r| <= F32_TOL bound + E on the kept rows, r the 3x3
    layer on the device's own fp32 sources, E the allowance of expf relative to its result.  Separate end (ry_conv_direct + ry_sr_post): the layer was held
    like every other in s2_walk; here |log y - v| <= E on the device's own pre-activation v.  Both: the edge bin repeats the last one bit for bit.
    -> worst |log y - r| / (F32_TOL bound + E)"""
    k0, k1 = walk['k']
    spec = walk['specs'][15]
    Wd = y.shape[2] - 1
    assert numpy.isfinite(y[:, k0:k1]).all() and (y[:, k0:k1] > 0).all(), (what, 'kept rows')
    assert numpy.array_equal(y[:, k0:k1, -1], y[:, k0:k1, -2]), (what, "pad(mode='edge') repeats the last predicted bin")
    ly = numpy.log(y[:, k0:k1, :Wd].astype(numpy.float64))
    if walk['fused']:
        srcs = [walk['raw'][sidx][0].astype(numpy.float64) for sidx in spec['src']]
        W, b, _ = s2_layer_params(P, spec, False)
        r, bound = ref_conv2d_f64(numpy.concatenate(srcs, axis=3), W, b, None, 1, spec['p'], False, None)
        r, bound = r[:, k0:k1, :, 0], bound[:, k0:k1, :, 0]
        bar = F32_TOL * bound + E
    else:
        r = walk['raw'][15][0][:, k0:k1, :, 0].astype(numpy.float64)
        bar = numpy.full_like(r, E)
    assert numpy.isfinite(r).all(), (what, 'the reference of a kept row read a NaN source row')
    assert float(numpy.abs(r).max()) <= EXP_ARG_MAX, (what, 'outside the arguments the expf allowance was measured on')
    ratio = numpy.abs(ly - r) / bar
    i = numpy.unravel_index(int(numpy.argmax(ratio)), ratio.shape)
    assert ratio[i] <= 1.0, ('%s: |log y - r| = %.3g > %.3g at (b, row, bin) = %s' % (what, abs(ly[i] - r[i]), bar[i], i))
    return float(ratio[i])


EXP_ARG_MAX = 40.0      # scripts/stage2_graph_tolerance.py measures expf on [-40, 40] and logf on exp([-40, 10])


def s2_tolerances():
    """(E, E_log): the allowances of the device's expf / logf relative to the result, read from profiles/r12/stage2_graph_tolerance.txt"""
    from pathlib import Path
    t = (Path(__file__).resolve().parent.parent / 'profiles' / 'r12' / 'stage2_graph_tolerance.txt').read_text().splitlines()
    get = lambda key: float([l for l in t if l.startswith(key + ' =')][0].split()[-1])
    return get('E'), get('E_log')


def s2_check_pad(x_in, x, n_frames, take_log, E_log, what=''):
    """The padded input of a convert (layer -1) against numpy.pad(mode='minimum') of the caller's block x (B, n, cols >= x_in's): the minimum is numpy's
    on the float32 input; pad rows equal each other and the device's own value in the real row that holds the column's minimum, bit for bit (same
    function, same argument); stage 1 (no log): the whole block is bit-equal to numpy.pad; stage 2: |x_in - log x| <= E_log |log x| on the real rows.
    -> worst relative error of the log"""
    B, T, C = x_in.shape
    assert not numpy.isnan(x_in).any(), (what, 'NaN in the padded input')
    xs = x[:, :, :C]
    if not take_log:
        assert numpy.array_equal(x_in, numpy.pad(xs, [(0, 0), (0, T - n_frames), (0, 0)], mode='minimum')), what
        return 0.0
    pad = x_in[:, n_frames:]
    assert (pad.view(numpy.uint32) == pad[:, :1].view(numpy.uint32)).all(), (what, 'pad rows differ from each other')
    amin = xs.argmin(axis=1)                                              # (B, C): the row of each column's minimum
    at_min = numpy.take_along_axis(x_in[:, :n_frames], amin[:, None, :], axis=1)[:, 0]
    assert numpy.array_equal(pad[:, 0].view(numpy.uint32), at_min.view(numpy.uint32)), (what, 'pad rows are not the log of the column minimum')
    r = numpy.log(xs.astype(numpy.float64))
    assert float(r.min()) >= -EXP_ARG_MAX and float(r.max()) <= 10.0
    err = numpy.abs(x_in[:, :n_frames] - r) / numpy.maximum(numpy.abs(r), 1e-300)
    assert float(err.max()) <= E_log, (what, float(err.max()), E_log)
    return float(err.max())
