// crepe_kernels.h -- the kernels of the CREPE pitch tracker (crepe.cpp): framing, one implicit-GEMM 1-D convolution family on
// v_mfma_f32_32x32x2_f32 (conv1 .. conv6 and the dense classifier) and its split-bf16 form on v_mfma_f32_32x32x16_bf16, the split-K reduction with the
// same epilogues, and the decode
// (per-frame argmax / max, the 360-state Viterbi pass in float64, the local-average cents), and the voicing of the track (a two-state Viterbi
// pass over the confidence, the masked float64 f0 and the time axis), and the assembly of a streamed window's activation block from kept and fresh rows
// (one stream: crepe_act_assemble; the waves of a bank of streams in one launch: crepe_act_assemble_many).
// Semantics restated from the public crepe package and its PyTorch fork ([MEM]; INTEGRATION.md section 9 lists what is unpinned).
//
// Activations are channels-last with every frame's 'same' padding stored as zero rows, so the kernels never test an edge:
//   frames   [frame][254 + 1024 + 258]          (conv1: stride 4, 254 left; the row is 1536 floats so float4 loads stay aligned)
//   layer i  [frame][31 + L_i + 32][C_i]        (input of a width-64 layer; the pooled output of layer i - 1 fills the interior)
//   conv6    [frame][4][C6]                     (= the dense layer's input row: index position * C6 + channel, Keras Permute + Flatten)
// For an output row m = (frame, position) the K index k = tap * Cin + ci addresses input element (position * stride + tap) * Cin + ci
// of the frame's padded block, i.e. ONE contiguous window of taps * Cin floats per row: the A operand is a strided row gather.
#pragma once
#include "ry_dev.h"

#ifdef RY_HOST_EMU
#include <cmath>
#define CREPE_ISNAN(x) std::isnan(x)
#else
#define CREPE_ISNAN(x) __builtin_isnan(x)
#endif

#define CREPE_FRAME 1024          // samples per frame
#define CREPE_FRAME_ROW 1536      // padded frame row (254 zeros | 1024 samples | 258 zeros)
#define CREPE_CONV1_PAD 254
#define CREPE_BINS 360
#define CREPE_BAND 11             // transition T[i][j] > 0 only for |i - j| <= 11 (max(12 - |i - j|, 0))

// ---------------------------------------------------------------------------------------------
// Framing: frame f starts at sample f * hop - (center ? 512 : 0) of the 16 kHz signal (zeros outside it).  Each frame has its own mean
// subtracted and is divided by its population standard deviation, both taken in float64; the divisor is clamped at 1e-10 so that a
// digitally silent frame gives zeros, not NaN (the one deliberate difference from the original).
// ---------------------------------------------------------------------------------------------
// Many waves in one call (ry_crepe_track_many): the waves lie back to back in one buffer and a table says where -- per wave its samples at
// the caller's rate, its samples at 16 kHz and its frames, each as (first, count) in the concatenated buffers.  A kernel that is handed a
// table (`seg`; null: one wave, the call's own sizes) finds the wave of a frame or an output sample by bisection -- every wave has at least
// one sample and one frame, so the starts rise strictly -- and from there on works with indices local to that wave: the wave's own length,
// its own centre padding, its own time register, its own first frame.  The arithmetic is the single call's.
struct CrepeSeg { int in_off, in_len, off16, n16, frame0, n_frames; };

RY_DEV int crepe_seg_of_frame(const CrepeSeg* seg, int n_seg, int f) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid].frame0 <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

RY_DEV int crepe_seg_of_sample16(const CrepeSeg* seg, int n_seg, int t) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid].off16 <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// A frame index list (`idx`; null: workgroup b frames frame frame0 + b) packs chosen frames of a window into the passes: workgroup b of a pass
// frames window frame idx[frame0 + b] into row b (ry_crepe_stream_track: the frames whose rows the previous call cannot supply).
struct CrepeFrameParams { const float* audio; int n, hop, center, frame0, n_frames; float* out; const CrepeSeg* seg; int n_seg; const int* idx; };

RY_KERNEL(256) void crepe_frames(CrepeFrameParams p) {
    __shared__ double red[256];
    const int tid = (int)threadIdx.x;
    int f = p.frame0 + (int)blockIdx.x;
    if (p.idx) f = p.idx[f];                                       // block-uniform: row blockIdx.x of the pass holds this frame of the window
    const float* audio = p.audio;
    int n_audio = p.n;
    if (p.seg) {                                                   // block-uniform: frame f of the call is frame f - frame0 of its wave
        const CrepeSeg sg = p.seg[crepe_seg_of_frame(p.seg, p.n_seg, f)];
        audio = p.audio + sg.off16; n_audio = sg.n16; f -= sg.frame0;
    }
    const long long s0 = (long long)f * p.hop - (p.center ? CREPE_FRAME / 2 : 0) + 4 * tid;
    float v[4];
    double s = 0.0;
    for (int i = 0; i < 4; ++i) {
        const long long s_i = s0 + i;
        v[i] = (s_i >= 0 && s_i < n_audio) ? audio[s_i] : 0.f;
        s += (double)v[i];
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
    const double mean = red[0] / CREPE_FRAME;
    __syncthreads();
    double q = 0.0;
    for (int i = 0; i < 4; ++i) { const double d = (double)v[i] - mean; q += d * d; }
    red[tid] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
    double sd = sqrt(red[0] / CREPE_FRAME);
    if (!(sd > 1e-10)) sd = 1e-10;
    float* o = p.out + (size_t)blockIdx.x * CREPE_FRAME_ROW + CREPE_CONV1_PAD + 4 * tid;
    for (int i = 0; i < 4; ++i) o[i] = (float)(((double)v[i] - mean) / sd);
}

// ---------------------------------------------------------------------------------------------
// Resampling to 16 kHz: band-limited interpolation with resampy's 'kaiser_best' table ([MEM]), the statement of crepe.resample
// (realtime_yukarin_amd/crepe.py) per output sample.  Output t sits at time tr[t] of the input (the sequentially summed time register,
// a table per rate built on the host: a parallel sum would round differently), n = int(tr[t]).  Side 0 walks the taps x[n], x[n - 1], ..
// and side 1 the taps x[n + 1], x[n + 2], .., each through the half filter `win` in steps of `step` entries from its own fractional
// offset, linearly interpolated with delta[j] = win[j + 1] - win[j] (0 behind the last entry).  One thread per output adds the terms
// (win[j] + eta * delta[j]) * x[src] in that order in float64, every operation rounded on its own (no fma): the float32 result has the
// bits of the host function.  The tap counts are cut by the table's end and by both ends of the signal, so no index leaves win or x
// as long as 0 <= n < n_in, which the host checks on its copy of the table before it launches (crepe.cpp: resample_plan).
// ---------------------------------------------------------------------------------------------
struct CrepeResampleParams {
    const float* x; int n_in;          // input at the caller's rate
    const double* win; int n_win;      // half filter, scaled by the ratio when down-sampling
    const double* tr;                  // time register [n_out]
    double scale;                      // min(1, ratio)
    int num_table, step;               // table entries per zero crossing; entries per input sample = int(scale * num_table)
    float* y; int n_out;
    const CrepeSeg* seg; int n_seg;    // many waves: x and y are the concatenated buffers, n_out the outputs of all waves, n_in is not read
};

RY_KERNEL(256) void crepe_resample(CrepeResampleParams p) {
#pragma clang fp contract(off)
    const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (t >= p.n_out) return;
    const float* x = p.x;
    int n_in = p.n_in, tl = t;
    if (p.seg) {                                                   // output t of the call is output t - off16 of its wave: that wave's register entry, its samples only
        const CrepeSeg sg = p.seg[crepe_seg_of_sample16(p.seg, p.n_seg, t)];
        x = p.x + sg.in_off; n_in = sg.in_len; tl = t - sg.off16;
    }
    const double tr = p.tr[tl];
    const int n = (int)tr;                                         // 0 <= tr < 2^31 (ry_crepe_set_resampler)
    const double frac0 = p.scale * (tr - (double)n);
    double acc = 0.0;
    for (int side = 0; side < 2; ++side) {
        const double frac = side ? p.scale - frac0 : frac0;
        const double index_frac = frac * (double)p.num_table;
        const int offset = (int)index_frac;                        // 0 .. num_table
        const double eta = index_frac - (double)offset;
        const int lim = (p.n_win - offset) / p.step;
        const int room = side ? n_in - n - 1 : n + 1;
        const int cap = room < lim ? room : lim;
        const float* xs = x + (side ? n + 1 : n);
        const double* w = p.win + offset;
        const int dir = side ? 1 : -1;
        for (int i = 0; i < cap; ++i) {
            const int j = i * p.step;                              // offset + j < n_win <= 2^31 - 1 by the cut at lim
            const double w0 = w[j];
            const double d = offset + j + 1 < p.n_win ? w[j + 1] - w0 : 0.0;
            acc += (w0 + eta * d) * (double)xs[dir * i];
        }
    }
    p.y[t] = (float)acc;
}

// ---------------------------------------------------------------------------------------------
// Implicit GEMM: D[m][n] = sum_k A[m][k] W[n][k], tile 128 x 128 x 32, four waves of 64 x 64 (2 x 2 blocks of 32 x 32), one
// v_mfma_f32_32x32x2_f32 per block and K step.  Both operands sit k-contiguous in the LDS ([row][32 + 4]); K step s of a chunk gives
// lane half h the index k = 16 h + s (A and B agree, so the sum is the same), which lets every lane fetch four steps with one 16-byte
// LDS read.  The next chunk's global loads are issued before the current chunk's MFMAs (register prefetch, one LDS buffer).
// grid = (N tiles, M tiles, splits); split z covers chunks [z * nch / splits, (z + 1) * nch / splits).
// Epilogues:  CREPE_EPI_POOL  bias -> ReLU -> BN affine -> max of the row pair (2 p, 2 p + 1) -> pooled row p of the padded output
//             CREPE_EPI_SIG   bias -> logits and sigmoid(logits) (the dense classifier)
//             CREPE_EPI_RAW   the split's raw sums into its slab [z][M][N] (crepe_reduce finishes them in a fixed order)
// Rows m, m + 1 of a pair are registers r, r + 1 of the same lane (D row = (r & 3) + 8 (r >> 2) + 4 h), so the pool is in-register.
// ---------------------------------------------------------------------------------------------
enum { CREPE_EPI_RAW = 0, CREPE_EPI_POOL = 1, CREPE_EPI_SIG = 2 };

struct CrepeGemmParams {
    const float* x;            // input activations (padded frames)
    const float* w;            // [N][K], k = tap * Cin + ci
    const float *bias, *scale, *shift;   // [N] (scale / shift: the BN affine; unused by the dense layer)
    float* y;                  // POOL: padded output / SIG: activation [M][N] / RAW: slabs [splits][M][N]
    float* y2;                 // SIG: logits [M][N]
    int M, N, K;
    int lout;                  // output positions per frame (before the pool)
    int in_fstride;            // floats per input frame
    int in_rstride;            // floats between the windows of consecutive positions (stride * Cin)
    int out_fstride, out_off;  // POOL: floats per output frame, offset of position 0 (left padding rows * N)
    int splits;
};

#define CREPE_BM 128
#define CREPE_BN 128
#define CREPE_BK 32
#define CREPE_LDS_ROW (CREPE_BK + 4)

RY_DEV float crepe_act(float acc, float b, float sc, float sh) {
    const float v = fmaxf(acc + b, 0.f);
    return v * sc + sh;
}

// the epilogue of a workgroup's 128 x 128 tile, shared by the fp32 and the split-bf16 kernel: wave (wm, wn) holds 2 x 2 accumulator blocks
template <int EPI>
RY_DEV void crepe_epilogue(const CrepeGemmParams& p, const f32x16 (&acc)[2][2], int m0, int n0, int wm, int wn, int r, int h, int z) {
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + r;
        if (n >= p.N) continue;
        float b = 0.f, sc = 1.f, sh = 0.f;
        if (EPI != CREPE_EPI_RAW) b = p.bias[n];
        if (EPI == CREPE_EPI_POOL) { sc = p.scale[n]; sh = p.shift[n]; }
        for (int i = 0; i < 2; ++i) {
            const int mb = m0 + wm * 64 + i * 32 + 4 * h;
            for (int e = 0; e < 16; e += 2) {
                const int m = mb + (e & 3) + 8 * (e >> 2);
                if (m >= p.M) continue;
                if (EPI == CREPE_EPI_POOL) {                          // conv layers: M is even, the pair is in or out together
                    const float v = fmaxf(crepe_act(acc[i][j][e], b, sc, sh), crepe_act(acc[i][j][e + 1], b, sc, sh));
                    const int pr = m >> 1, half = p.lout >> 1;
                    const int fr = pr / half, pos = pr - fr * half;
                    p.y[(size_t)fr * p.out_fstride + p.out_off + (size_t)pos * p.N + n] = v;
                } else {
                    for (int u = 0; u < 2 && m + u < p.M; ++u) {      // the dense layer: M = frames may be odd
                        const float a = acc[i][j][e + u];
                        const size_t o = (size_t)(m + u) * p.N + n;
                        if (EPI == CREPE_EPI_RAW) {
                            p.y[(size_t)z * p.M * p.N + o] = a;
                        } else {
                            const float l = a + b;
                            p.y2[o] = l;
                            p.y[o] = 1.f / (1.f + expf(-l));
                        }
                    }
                }
            }
        }
    }
}

// LAYER (1 .. 6 conv, 7 dense) only names the instantiation, so that a kernel trace tells the layers apart
template <int EPI, int LAYER>
RY_KERNEL(256) void crepe_igemm(CrepeGemmParams p) {
    __shared__ float As[CREPE_BM * CREPE_LDS_ROW];
    __shared__ float Bs[CREPE_BN * CREPE_LDS_ROW];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = (int)blockIdx.y * CREPE_BM, n0 = (int)blockIdx.x * CREPE_BN;
    const int nch = p.K / CREPE_BK;
    const int z = (int)blockIdx.z;
    const int c_lo = (int)((long long)z * nch / p.splits), c_hi = (int)((long long)(z + 1) * nch / p.splits);

    // this thread's four A rows / four B rows (row = idx >> 3, 16-byte piece kq = idx & 7 of the 32-wide chunk)
    const float* ga[4];
    const float* gb[4];
    bool va[4], vb[4];
    int lrow[4], lq[4];
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i;
        lrow[i] = idx >> 3; lq[i] = idx & 7;
        const int m = m0 + lrow[i], n = n0 + lrow[i];
        va[i] = m < p.M;
        vb[i] = n < p.N;
        const int mm = va[i] ? m : 0;
        const int fr = mm / p.lout, pos = mm - fr * p.lout;
        ga[i] = p.x + (size_t)fr * p.in_fstride + (size_t)pos * p.in_rstride + 4 * lq[i];
        gb[i] = p.w + (size_t)(vb[i] ? n : 0) * p.K + 4 * lq[i];
    }
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 ra[4], rb[4];
    auto load = [&](int c) {
        const int k0 = c * CREPE_BK;
        for (int i = 0; i < 4; ++i) {
            ra[i] = va[i] ? ry_ld4(ga[i] + k0) : zero4;
            rb[i] = vb[i] ? ry_ld4(gb[i] + k0) : zero4;
        }
    };
    auto stash = [&]() {
        for (int i = 0; i < 4; ++i) {
            ry_st4(&As[lrow[i] * CREPE_LDS_ROW + 4 * lq[i]], ra[i]);
            ry_st4(&Bs[lrow[i] * CREPE_LDS_ROW + 4 * lq[i]], rb[i]);
        }
    };

    f32x16 acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    if (c_lo < c_hi) {
        load(c_lo);
        stash();
        __syncthreads();
    }
    for (int c = c_lo; c < c_hi; ++c) {
        if (c + 1 < c_hi) load(c + 1);
        const float* pa0 = &As[(wm * 64 + r) * CREPE_LDS_ROW + 16 * h];
        const float* pa1 = pa0 + 32 * CREPE_LDS_ROW;
        const float* pb0 = &Bs[(wn * 64 + r) * CREPE_LDS_ROW + 16 * h];
        const float* pb1 = pb0 + 32 * CREPE_LDS_ROW;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 a0 = ry_ld4(pa0 + 4 * q), a1 = ry_ld4(pa1 + 4 * q);
            const f32x4 b0 = ry_ld4(pb0 + 4 * q), b1 = ry_ld4(pb1 + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][0] = ry_mfma_32x32x2(a0[e], b0[e], acc[0][0]);
                acc[0][1] = ry_mfma_32x32x2(a0[e], b1[e], acc[0][1]);
                acc[1][0] = ry_mfma_32x32x2(a1[e], b0[e], acc[1][0]);
                acc[1][1] = ry_mfma_32x32x2(a1[e], b1[e], acc[1][1]);
            }
        }
        __syncthreads();
        if (c + 1 < c_hi) {
            stash();
            __syncthreads();
        }
    }

    crepe_epilogue<EPI>(p, acc, m0, n0, wm, wn, r, h, z);
}

// ---------------------------------------------------------------------------------------------
// The split-bf16 form of the same GEMM (ry_crepe_set_dtype 2): every fp32 product x w becomes x_lo w_hi + x_hi w_lo + x_hi w_hi on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation, hi = bf16(v), lo = bf16(v - hi) (ry_split_bf16).  Same tile, grid, waves and epilogues as
// crepe_igemm; K runs in chunks of 64.  Activations stay fp32 in memory and are split while they are staged (global fp32 -> registers -> two bf16
// planes in the LDS); the filters come split, w_hi / w_lo [N][K] bf16 (crepe_split_w).  An LDS row holds the 64 bf16 of a chunk and 8 of padding:
// K step s (16 wide) of lane half h is the 16 bytes at 32 s + 16 h of the row, one ds_read_b128, and the 144-byte row stride sends the 16 rows
// of a read's lane group (distinct mod 16) to the 16 different 16-byte slots of the 256-byte bank row (144 / 16 = 9 is odd): no conflict.
// Four planes of 128 x 72 bf16 = 72 KiB: two workgroups per CU.
// Order of the products, per K step of 16 and accumulator block: lo hi, hi lo, hi hi (x first); the K steps of a chunk and the chunks of a split
// follow in rising k.
// ---------------------------------------------------------------------------------------------
#define CREPE_X3_BK 64
#define CREPE_X3_ROW (CREPE_X3_BK + 8)

struct CrepeX3Params { CrepeGemmParams g; const unsigned short *w_hi, *w_lo; };   // g.w is not read

template <int EPI, int LAYER>
RY_KERNEL(256, 2) void crepe_igemm_x3(CrepeX3Params px) {      // two workgroups per CU: the LDS holds two, so the registers must too
    __shared__ __attribute__((aligned(16))) unsigned short Ah[CREPE_BM * CREPE_X3_ROW];
    __shared__ __attribute__((aligned(16))) unsigned short Al[CREPE_BM * CREPE_X3_ROW];
    __shared__ __attribute__((aligned(16))) unsigned short Bh[CREPE_BN * CREPE_X3_ROW];
    __shared__ __attribute__((aligned(16))) unsigned short Bl[CREPE_BN * CREPE_X3_ROW];
    const CrepeGemmParams& p = px.g;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = (int)blockIdx.y * CREPE_BM, n0 = (int)blockIdx.x * CREPE_BN;
    const int nch = p.K / CREPE_X3_BK;
    const int z = (int)blockIdx.z;
    const int c_lo = (int)((long long)z * nch / p.splits), c_hi = (int)((long long)(z + 1) * nch / p.splits);

    // this thread's four A rows / four B rows (row = idx >> 3, piece kq = idx & 7 of eight k of the 64-wide chunk)
    const float* ga[4];
    const unsigned short* gbh[4];
    const unsigned short* gbl[4];
    bool va[4], vb[4];
    int lofs[4];
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i;
        const int row = idx >> 3, kq = idx & 7;
        lofs[i] = row * CREPE_X3_ROW + 8 * kq;
        const int m = m0 + row, n = n0 + row;
        va[i] = m < p.M;
        vb[i] = n < p.N;
        const int mm = va[i] ? m : 0;
        const int fr = mm / p.lout, pos = mm - fr * p.lout;
        ga[i] = p.x + (size_t)fr * p.in_fstride + (size_t)pos * p.in_rstride + 8 * kq;
        const size_t wo = (size_t)(vb[i] ? n : 0) * p.K + 8 * kq;
        gbh[i] = px.w_hi + wo;
        gbl[i] = px.w_lo + wo;
    }
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    f32x4 ra[4][2];
    u16x8 rbh[4], rbl[4];
    auto load = [&](int c) {
        const int k0 = c * CREPE_X3_BK;
        for (int i = 0; i < 4; ++i) {
            ra[i][0] = va[i] ? ry_ld4(ga[i] + k0) : zero4;
            ra[i][1] = va[i] ? ry_ld4(ga[i] + k0 + 4) : zero4;
            rbh[i] = vb[i] ? ry_ld8h(gbh[i] + k0) : zero8;
            rbl[i] = vb[i] ? ry_ld8h(gbl[i] + k0) : zero8;
        }
    };
    auto stash = [&]() {
        for (int i = 0; i < 4; ++i) {
            u16x8 xh, xl;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                unsigned short hi, lo;
                ry_split_bf16(ra[i][u >> 2][u & 3], &hi, &lo);
                xh[u] = hi; xl[u] = lo;
            }
            ry_st8h(&Ah[lofs[i]], xh);
            ry_st8h(&Al[lofs[i]], xl);
            ry_st8h(&Bh[lofs[i]], rbh[i]);
            ry_st8h(&Bl[lofs[i]], rbl[i]);
        }
    };

    f32x16 acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    if (c_lo < c_hi) {
        load(c_lo);
        stash();
        __syncthreads();
    }
    const int oa = (wm * 64 + r) * CREPE_X3_ROW + 8 * h, ob = (wn * 64 + r) * CREPE_X3_ROW + 8 * h;
    for (int c = c_lo; c < c_hi; ++c) {
        if (c + 1 < c_hi) load(c + 1);
#pragma unroll
        for (int s = 0; s < CREPE_X3_BK / 16; ++s) {
            u16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = ry_ld8h(&Ah[oa + i * 32 * CREPE_X3_ROW + 16 * s]);
                al[i] = ry_ld8h(&Al[oa + i * 32 * CREPE_X3_ROW + 16 * s]);
                bh[i] = ry_ld8h(&Bh[ob + i * 32 * CREPE_X3_ROW + 16 * s]);
                bl[i] = ry_ld8h(&Bl[ob + i * 32 * CREPE_X3_ROW + 16 * s]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = ry_mfma_32x32x16_bf16(al[i], bh[j], acc[i][j]);
                    acc[i][j] = ry_mfma_32x32x16_bf16(ah[i], bl[j], acc[i][j]);
                    acc[i][j] = ry_mfma_32x32x16_bf16(ah[i], bh[j], acc[i][j]);
                }
        }
        __syncthreads();
        if (c + 1 < c_hi) {
            stash();
            __syncthreads();
        }
    }
    crepe_epilogue<EPI>(p, acc, m0, n0, wm, wn, r, h, z);
}

// the filters of a layer, split once: eight values per thread, n8 = N K / 8 (K is a multiple of 64)
struct CrepeSplitWParams { const float* w; unsigned short *hi, *lo; long long n8; };

RY_KERNEL(256) void crepe_split_w(CrepeSplitWParams p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.n8) return;
    const f32x4 v0 = ry_ld4(p.w + 8 * t), v1 = ry_ld4(p.w + 8 * t + 4);
    u16x8 xh, xl;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        unsigned short hi, lo;
        ry_split_bf16(u < 4 ? v0[u & 3] : v1[u & 3], &hi, &lo);
        xh[u] = hi; xl[u] = lo;
    }
    ry_st8h(p.hi + 8 * t, xh);
    ry_st8h(p.lo + 8 * t, xl);
}

// The split-K sums (slab 0 + slab 1 + ... in that order) and the layer's epilogue: one thread per pooled output (POOL, M / 2 x N) or
// per output (SIG, M x N).
struct CrepeReducePoolParams { const float* slabs; const float *bias, *scale, *shift; float* y; int M, N, lout, out_fstride, out_off, splits; };

RY_KERNEL(256) void crepe_reduce_pool(CrepeReducePoolParams p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)(p.M >> 1) * p.N) return;
    const int n = (int)(idx % p.N), pr = (int)(idx / p.N);
    const size_t slab = (size_t)p.M * p.N;
    const float* s = p.slabs + (size_t)(2 * pr) * p.N + n;
    float a0 = 0.f, a1 = 0.f;
    for (int z = 0; z < p.splits; ++z) { a0 += s[z * slab]; a1 += s[z * slab + p.N]; }
    const float v = fmaxf(crepe_act(a0, p.bias[n], p.scale[n], p.shift[n]), crepe_act(a1, p.bias[n], p.scale[n], p.shift[n]));
    const int half = p.lout >> 1;
    const int fr = pr / half, pos = pr - fr * half;
    p.y[(size_t)fr * p.out_fstride + p.out_off + (size_t)pos * p.N + n] = v;
}

struct CrepeReduceSigParams { const float* slabs; const float* bias; float* act; float* logits; int M, N, splits; };

RY_KERNEL(256) void crepe_reduce_sig(CrepeReduceSigParams p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.M * p.N) return;
    const int n = (int)(idx % p.N);
    const size_t slab = (size_t)p.M * p.N;
    float a = 0.f;
    for (int z = 0; z < p.splits; ++z) a += p.slabs[z * slab + idx];
    const float l = a + p.bias[n];
    p.logits[idx] = l;
    p.act[idx] = 1.f / (1.f + expf(-l));
}

// ---------------------------------------------------------------------------------------------
// Decode.  crepe_argmax: one wave per frame, observation = argmax (lowest index on ties), confidence = max.
// crepe_decode: ONE workgroup per track (one track, or the tracks of a segment table side by side).  viterbi = 1: the 360-state Viterbi pass over all frames in float64 with the host's tables
//   lat[0][j] = logS[j] + logE[j][obs 0];  lat[t][j] = max_i (lat[t - 1][i] + logT[i][j]) + logE[j][obs t]   (lowest i wins a tie)
//   -- the additions of the numpy restatement in its order; only |i - j| <= 11 is visited (logT is -inf elsewhere and the lattice is
//   finite, so the maximum and its index are the same) -- back-pointers in global memory, the backtrack by one lane.
//   Then, per frame, the local weighted average of cents over bins [c - 4, c + 5) around the path (viterbi = 0: around the observation),
//   f0 = 10 * 2^(cents / 1200), NaN -> 0.
// ---------------------------------------------------------------------------------------------
struct CrepeArgmaxParams { const float* act; int n_frames; int* obs; float* conf; };

RY_KERNEL(256) void crepe_argmax(CrepeArgmaxParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const int t = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (t >= p.n_frames) return;                                   // wave-uniform
    const float* a = p.act + (size_t)t * CREPE_BINS;
    float best = a[lane];
    float bi = (float)lane;
    for (int j = lane + 64; j < CREPE_BINS; j += 64)
        if (a[j] > best) { best = a[j]; bi = (float)j; }
    for (int mask = 32; mask > 0; mask >>= 1) {
        const float ob = ry_shfl_xor(best, mask), oi = ry_shfl_xor(bi, mask);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { p.obs[t] = (int)bi; p.conf[t] = best; }
}

struct CrepeDecodeParams {
    const float* act; const int* obs; int n_frames; int viterbi;
    const double* logT;        // [360][360]
    const double* logE;        // [360][360]
    const double* logS;        // [360]
    int* bp;                   // [n_frames][360] back-pointers
    int* path;                 // [n_frames]
    float* f0;
    const CrepeSeg* seg;       // many tracks: one workgroup each (grid = tracks), every array above the concatenated one; n_frames is not read
};

RY_KERNEL(384) void crepe_decode(CrepeDecodeParams p) {
    __shared__ double lat[2][CREPE_BINS];
    __shared__ double tb[(2 * CREPE_BAND + 1) * CREPE_BINS];      // logT[j - 11 + d][j] at [d][j]: a wave reads consecutive doubles
    const int tid = (int)threadIdx.x;
    int n = p.n_frames;
    if (p.seg) {                                                   // this workgroup's track: its own rows of every array, its own start from logS
        const CrepeSeg sg = p.seg[blockIdx.x];
        n = sg.n_frames;
        p.act += (size_t)sg.frame0 * CREPE_BINS; p.obs += sg.frame0; p.bp += (size_t)sg.frame0 * CREPE_BINS; p.path += sg.frame0; p.f0 += sg.frame0;
    }
    if (p.viterbi) {
        const int j = tid;
        const bool live = j < CREPE_BINS;
        const double* le = p.logE + (size_t)(live ? j : 0) * CREPE_BINS;
        if (live) {
            for (int d = 0; d <= 2 * CREPE_BAND; ++d) {
                const int i = j - CREPE_BAND + d;
                tb[d * CREPE_BINS + j] = (i >= 0 && i < CREPE_BINS) ? p.logT[(size_t)i * CREPE_BINS + j] : 0.0;
            }
            lat[0][j] = p.logS[j] + le[p.obs[0]];
        }
        // the emission term of frame t + 1 and the observation of frame t + 2 are requested one step ahead; the barrier of each step waits
        // for the LDS only (ry_lds_barrier), so these loads stay in flight across it
        double e_next = (live && n > 1) ? le[p.obs[1]] : 0.0;
        int o_next = n > 2 ? p.obs[2] : 0;
        ry_lds_barrier();
        for (int t = 1; t < n; ++t) {
            const double e = e_next;
            if (live && t + 1 < n) e_next = le[o_next];
            if (t + 2 < n) o_next = p.obs[t + 2];
            const double* prev = lat[(t - 1) & 1];
            if (live) {
                double best = 0.0;
                int bi = -1;
#pragma unroll
                for (int d = 0; d <= 2 * CREPE_BAND; ++d) {
                    const int i = j - CREPE_BAND + d;
                    if (i >= 0 && i < CREPE_BINS) {
                        const double v = prev[i] + tb[d * CREPE_BINS + j];
                        if (bi < 0 || v > best) { best = v; bi = i; }
                    }
                }
                lat[t & 1][j] = best + e;
                p.bp[(size_t)t * CREPE_BINS + j] = bi;
            }
            ry_lds_barrier();
        }
        __syncthreads();                                           // the back-pointers of every wave are visible to lane 0
        if (tid == 0) {
            const double* last = lat[(n - 1) & 1];
            int st = 0;
            for (int i = 1; i < CREPE_BINS; ++i)
                if (last[i] > last[st]) st = i;
            p.path[n - 1] = st;
            for (int t = n - 1; t > 0; --t) {
                st = p.bp[(size_t)t * CREPE_BINS + st];
                p.path[t - 1] = st;
            }
        }
        __syncthreads();
    }
    for (int t = tid; t < n; t += 384) {
        const int c = p.viterbi ? p.path[t] : p.obs[t];
        const int b0 = c - 4 < 0 ? 0 : c - 4, b1 = c + 5 > CREPE_BINS ? CREPE_BINS : c + 5;
        const float* a = p.act + (size_t)t * CREPE_BINS;
        double ps = 0.0, ws = 0.0;
        for (int b = b0; b < b1; ++b) {
            ps += (double)a[b] * ((double)b * 20.0 + 1997.3794084376191);
            ws += (double)a[b];
        }
        const double f = 10.0 * exp2((ps / ws) / 1200.0);
        p.f0[t] = CREPE_ISNAN(f) ? 0.f : (float)f;
    }
}

// ---------------------------------------------------------------------------------------------
// The activation block of a streamed window (ry_crepe_stream_track): row j is row src[j] of the block the previous call left (`keep`) when
// src[j] >= 0, else row -1 - src[j] of the rows this call computed (`fresh`, packed back to back).  A row is 360 floats = 90 words of 16 bytes,
// 16-byte aligned in every block; one wave per row, lane l moves words l and l + 64: consecutive lanes, consecutive 16 bytes.  A source index
// outside its block reads nothing and writes nothing.  One launch instead of one copy per kept row.
// ---------------------------------------------------------------------------------------------
struct CrepeAssembleParams { const float* keep; int n_keep; const float* fresh; int n_fresh; const int* src; float* out; int n_rows; };

RY_KERNEL(256) void crepe_act_assemble(CrepeAssembleParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const int j = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= p.n_rows) return;                                     // wave-uniform, like everything up to the copy
    const long long s = p.src[j];
    const long long f = -1 - s;
    if (s >= 0 ? s >= p.n_keep : f >= p.n_fresh) return;
    const float* from = s >= 0 ? p.keep + (size_t)s * CREPE_BINS : p.fresh + (size_t)f * CREPE_BINS;
    float* to = p.out + (size_t)j * CREPE_BINS;
    for (int q = lane; q < CREPE_BINS / 4; q += 64) ry_st4(to + 4 * q, ry_ld4(from + 4 * q));
}

// ---------------------------------------------------------------------------------------------
// The same for the waves of a bank call (ry_crepe_bank_track), all in one launch.  Every stream of a bank has a pair of slots of its own -- the
// streams that take part change from call to call, and one that sits a call out finds its rows where it left them -- so a table says per wave
// where the stream's kept slot is (`keep`, n_keep rows) and which slot this call writes (`write`, never the kept one: new row j reads old row
// j + d while another wave of lanes writes row j + d).  Row j of the call finds its wave by bisection over the segment table; src[j] >= 0 names
// a row of that wave's kept slot, else -1 - src[j] a row of `fresh`, the packed rows all waves of the call share.  The row is written twice: to
// row j of the call's contiguous block (`out`, which the decode reads with the same segment table) and to row j - frame0 of the wave's write slot,
// the kept slot of that stream's next call.  A source index outside its block reads nothing and writes nothing.
// ---------------------------------------------------------------------------------------------
struct CrepeBankWave { const float* keep; float* write; int n_keep; int pad; };

struct CrepeAssembleManyParams {
    const CrepeSeg* seg; int n_seg;            // the call's waves: frame0 / n_frames are read
    const CrepeBankWave* wave;                 // [n_seg]
    const int* src;                            // [n_rows]
    const float* fresh; int n_fresh;
    float* out; int n_rows;
};

RY_KERNEL(256) void crepe_act_assemble_many(CrepeAssembleManyParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const int j = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= p.n_rows) return;                                     // wave-uniform, like everything up to the copy
    const int w = crepe_seg_of_frame(p.seg, p.n_seg, j);
    const CrepeBankWave d = p.wave[w];
    const int local = j - p.seg[w].frame0;
    const long long s = p.src[j];
    const long long f = -1 - s;
    if (s >= 0 ? s >= d.n_keep : f >= p.n_fresh) return;
    const float* from = s >= 0 ? d.keep + (size_t)s * CREPE_BINS : p.fresh + (size_t)f * CREPE_BINS;
    float* to = p.out + (size_t)j * CREPE_BINS;
    float* slot = d.write + (size_t)local * CREPE_BINS;
    for (int q = lane; q < CREPE_BINS / 4; q += 64) {
        const f32x4 v = ry_ld4(from + 4 * q);
        ry_st4(to + 4 * q, v);
        ry_st4(slot + 4 * q, v);
    }
}

// ---------------------------------------------------------------------------------------------
// Voicing (`predict_voicing` of realtime_yukarin_amd/crepe.py and the mask the reference's wrapper makes of it): the Viterbi path of a
// two-state Gaussian HMM over the confidence, voiced = (path == 1) | (confidence > threshold) -- the comparison in float32 against the threshold
// rounded to float32, which is how numpy evaluates `confidence > 0.1` on a float32 array -- the masked f0 and the time axis in float64.
// ONE workgroup per track; the frames run in chunks of CREPE_VOICING_CHUNK through the LDS, so a call may be of any length:
//   forward, chunk by chunk: every lane computes logp[t][s] = -0.5 * (c[s] + (x - mu[s]) * (x - mu[s]) / var[s]) of its frames into the LDS; lane 0
//     walks the chunk -- s[i][j] = lat[i] + logT[i][j], bp[j] = s[1][j] > s[0][j] (the lowest state wins a tie), lat[j] = s[bp[j]][j] + logp[t][j],
//     the lattice in its registers from chunk to chunk -- and leaves the two back-pointer bits of every frame in the LDS; every lane copies them out
//     (one byte per frame in global memory).
//   backward, chunk by chunk from the end: every lane fetches the chunk's back-pointers, lane 0 follows them from the state it arrived with, then
//     every lane writes voiced, f0_64 = voiced ? (double)f0 : 0 and t_64 = k * step_ms / 1000 of its frames.
// Float64, every operation rounded on its own and in numpy's order (no fma); the constants are the host's (ry_crepe_set_voicing_tables): no
// logarithm is taken here.  What lane 0 loads inside its walks does not depend on the lattice, so the loads run ahead of the arithmetic.
// ---------------------------------------------------------------------------------------------
#define CREPE_VOICING_CHUNK 1024

struct CrepeVoicingTables { double c[2], mu[2], var[2], logT[2][2], logS[2]; };      // c[s] = log(2 pi var[s]); logT [from][to]

struct CrepeVoicingParams {
    const float* conf; const float* f0; int n;     // [n]
    float threshold;                               // compared in float32, as numpy compares a float32 array with a Python float
    double step_ms;
    CrepeVoicingTables tab;
    unsigned char* bp;                             // [n] scratch: bit j of entry t = the state before state j of frame t
    unsigned char* voiced; double* f0_64; double* t_64;
    const CrepeSeg* seg;                           // many tracks: one workgroup each (grid = tracks), every array the concatenated one; n is not read
};

RY_KERNEL(256) void crepe_voicing(CrepeVoicingParams p) {
#pragma clang fp contract(off)
    __shared__ double lp[CREPE_VOICING_CHUNK][2];
    __shared__ unsigned char bits[CREPE_VOICING_CHUNK];            // forward: back-pointer bits; backward: the same, then the path
    const int tid = (int)threadIdx.x;
    int n = p.n;
    if (p.seg) {                                                   // this workgroup's track: its own entries, its own back-pointers, k counted from its first frame
        const CrepeSeg sg = p.seg[blockIdx.x];
        n = sg.n_frames;
        p.conf += sg.frame0; p.f0 += sg.frame0; p.bp += sg.frame0; p.voiced += sg.frame0; p.f0_64 += sg.frame0; p.t_64 += sg.frame0;
    }
    const CrepeVoicingTables& T = p.tab;
    double lat0 = 0.0, lat1 = 0.0;                                 // lane 0 only
    for (int base = 0; base < n; base += CREPE_VOICING_CHUNK) {
        const int m = n - base < CREPE_VOICING_CHUNK ? n - base : CREPE_VOICING_CHUNK;
        for (int i = tid; i < m; i += 256) {
            const double x = (double)p.conf[base + i];
            const double d0 = x - T.mu[0], d1 = x - T.mu[1];
            lp[i][0] = -0.5 * (T.c[0] + d0 * d0 / T.var[0]);
            lp[i][1] = -0.5 * (T.c[1] + d1 * d1 / T.var[1]);
        }
        __syncthreads();
        if (tid == 0) {
            int i = 0;
            if (base == 0) {
                lat0 = T.logS[0] + lp[0][0];
                lat1 = T.logS[1] + lp[0][1];
                bits[0] = 0;
                i = 1;
            }
            for (; i < m; ++i) {
                const double s00 = lat0 + T.logT[0][0], s10 = lat1 + T.logT[1][0];
                const double s01 = lat0 + T.logT[0][1], s11 = lat1 + T.logT[1][1];
                const bool b0 = s10 > s00, b1 = s11 > s01;
                lat0 = (b0 ? s10 : s00) + lp[i][0];
                lat1 = (b1 ? s11 : s01) + lp[i][1];
                bits[i] = (unsigned char)((b0 ? 1 : 0) | (b1 ? 2 : 0));
            }
        }
        __syncthreads();
        for (int i = tid; i < m; i += 256) p.bp[base + i] = bits[i];
        __syncthreads();                                           // bits and lp are free for the next chunk; the stores are visible to the workgroup
    }
    int carry = lat1 > lat0 ? 1 : 0;                               // lane 0 only: the state of the last frame, then of the frame before the chunk
    const int last = n > 0 ? (n - 1) / CREPE_VOICING_CHUNK * CREPE_VOICING_CHUNK : -1;
    for (int base = last; base >= 0; base -= CREPE_VOICING_CHUNK) {
        const int m = n - base < CREPE_VOICING_CHUNK ? n - base : CREPE_VOICING_CHUNK;
        for (int i = tid; i < m; i += 256) bits[i] = p.bp[base + i];
        __syncthreads();
        if (tid == 0) {
            int st = carry;
            for (int i = m - 1; i >= 0; --i) {
                const int b = bits[i];
                bits[i] = (unsigned char)st;
                st = (b >> st) & 1;                                // frame 0 has no predecessor: its bits are 0 and nothing reads the result
            }
            carry = st;
        }
        __syncthreads();
        for (int i = tid; i < m; i += 256) {
            const int k = base + i;
            const bool v = bits[i] == 1 || p.conf[k] > p.threshold;
            p.voiced[k] = v ? 1 : 0;
            p.f0_64[k] = v ? (double)p.f0[k] : 0.0;
            p.t_64[k] = (double)k * p.step_ms / 1000.0;
        }
        __syncthreads();
    }
}
