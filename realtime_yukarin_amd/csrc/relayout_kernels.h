// relayout_kernels.h -- the filter layouts of a predictor built on the card from ONE upload of the raw Chainer filter (filter build mode `device`,
// ry_set_filter_build): the counterparts of the host functions relayout_1d / relayout_1d_os / relayout_igemm / relayout_direct / relayout_c2d_os /
// relayout_wino of ry_plan.cpp, which stay in the tree as the oracle -- every layout is held to them bit for bit (tests/filter_build_cases.py).
//
// The five permutation kernels are one template: a thread owns four consecutive floats of the DESTINATION, finds for each of them the index of its
// source in the raw filter (conv W (N, C, k[, k]), deconv W (C, N, 4[, 4]); the two skip sources are consecutive channel ranges of that one filter,
// C = cin_a + cin_b) and writes them with one 16-byte store: a wave stores one contiguous KiB.  Where the host layout has padding (the taps beyond k of
// the stage-1 layouts) it writes +0.0f, so every float of the allocation is written.  The loads are a gather (4-byte, at the strides of the
// permutation): a load-time path, measured against the upload of the same filter in DESIGN.md section 23.
//
// ry_relayout_wino: the F(2x2, 2x2) filter transform U = G g G^T in float64, one thread per (phase, output channel, slice, channel of the slice),
// from the direct layout on the card.
#pragma once
#include "ry_dev.h"

struct RyRelayoutParams {
    const float* W;             // the raw filter
    float* out;                 // the layout: `total` floats
    long long total;
    int C, N, K;                // input channels (both sources), output channels, taps per axis
    int deconv, nphases, ntaps; // make_taps(): kernel index (ky, kx) of tap tt of phase ph
    unsigned char ky[4][16], kx[4][16];
};

RY_DEV long long ry_w2d_index(const RyRelayoutParams& p, int n, int c, int ky, int kx) {
    return p.deconv ? (((long long)c * p.N + n) * p.K + ky) * p.K + kx : (((long long)n * p.C + c) * p.K + ky) * p.K + kx;
}

// index in the raw filter of float `o` of the layout; -1: padding
template <int KIND>
RY_DEV long long ry_relayout_src(const RyRelayoutParams& p, long long o) {
    if (KIND == RY_LAYOUT_W1D || KIND == RY_LAYOUT_W1OS) {
        const int k = (int)(o & 3);
        const long long q = o >> 2;
        int c, n;
        if (KIND == RY_LAYOUT_W1D) { n = (int)(q % p.N); c = (int)(q / p.N); }       // [C][N][4]
        else { c = (int)(q % p.C); n = (int)(q / p.C); }                              // [N][C][4]
        if (k >= p.K) return -1;
        return p.deconv ? ((long long)c * p.N + n) * p.K + k : ((long long)n * p.C + c) * p.K + k;
    }
    int ph, tt, c, n;
    if (KIND == RY_LAYOUT_WDIR) {                                                     // [phase][tap][C][N]
        n = (int)(o % p.N);
        long long q = o / p.N;
        c = (int)(q % p.C); q /= p.C;
        tt = (int)(q % p.ntaps); ph = (int)(q / p.ntaps);
    } else if (KIND == RY_LAYOUT_WIG) {                                               // [phase][N/64][tap][C/32] blocks of 2048 in fragment order (wig_inblock)
        const int r = (int)(o & 2047), lane = (r >> 2) & 63;
        const int nl = (r >> 10) * 32 + (lane & 31), k = ((r >> 8) & 3) * 8 + (lane >> 5) * 4 + (r & 3);
        long long q = o >> 11;
        const int cpt = p.C / 32;
        c = (int)(q % cpt) * 32 + k; q /= cpt;
        tt = (int)(q % p.ntaps); q /= p.ntaps;
        n = (int)(q % (p.N / 64)) * 64 + nl; ph = (int)(q / (p.N / 64));
    } else {                                                                          // [phase][N/4][tap][C/64] blocks of 256: lane = 4 * ((c % 64) / 4) + n % 4, c % 4
        const int r = (int)(o & 255), lane = r >> 2;
        long long q = o >> 8;
        const int cpt = p.C / 64;
        c = (int)(q % cpt) * 64 + (lane >> 2) * 4 + (r & 3); q /= cpt;
        tt = (int)(q % p.ntaps); q /= p.ntaps;
        n = (int)(q % (p.N / 4)) * 4 + (lane & 3); ph = (int)(q / (p.N / 4));
    }
    return ry_w2d_index(p, n, c, p.ky[ph][tt], p.kx[ph][tt]);
}

template <int KIND>
RY_KERNEL(256) void ry_relayout(RyRelayoutParams p) {
    const long long o = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (o >= p.total) return;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long s = o + j < p.total ? ry_relayout_src<KIND>(p, o + j) : -1;
        v[j] = s >= 0 ? p.W[s] : 0.0f;
    }
    if (o + 4 <= p.total) {
        f32x4 q; q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = v[3];
        ry_st4(p.out + o, q);
    } else {                                   // the last piece of a layout whose size is no multiple of four floats
        for (int j = 0; o + j < p.total; ++j) p.out[o + j] = v[j];
    }
}

struct RyRelayoutWinoParams {
    const float* wd;            // the direct layout [phase][tap][C][N]
    float* out;                 // [phase][N/64][slice][position 9][n/32][lane = 32 * (cc / 4) + n % 32][cc % 4]
    long long threads;          // phases x N x slices x 8
    int C, N, nsl, deconv;
    unsigned char where[4][4];  // (ky, kx) -> phase * ntaps + tap of the direct layout
};

// Thread index = [phase][n/64][slice][n/32 % 2][cc/4][n % 32][cc % 4]: consecutive threads write consecutive floats of each of the nine positions.
// Arithmetic as relayout_wino (ry_plan.cpp): u = 0.0, then the four u += G[i][a] * g[a][b] * G[j][b] in float64, the zero-coefficient terms kept (an
// infinite tap gives NaN, a -0.0 tap the sum's zero sign), no contraction, one rounding to float32.
RY_KERNEL(256) void ry_relayout_wino(RyRelayoutWinoParams p) {
#pragma clang fp contract(off)
    long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.threads) return;
    const int cc = (int)(t & 3) + 4 * (int)((t >> 7) & 1), n32 = (int)((t >> 2) & 31), nh = (int)((t >> 8) & 1);
    t >>= 9;
    const int ks = (int)(t % p.nsl); t /= p.nsl;
    const int nb = (int)(t % (p.N / 64)), ph = (int)(t / (p.N / 64));
    const int n = nb * 64 + nh * 32 + n32;
    const int DKY[2][2] = {{1, 3}, {0, 2}};                                   // DECONV_KY
    int c;
    double g[2][2];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            int ky, kx;
            if (p.deconv) { c = ks * 8 + cc; ky = DKY[ph >> 1][1 - a]; kx = DKY[ph & 1][1 - b]; }
            else { const int par = (ks >> 1) & 3; c = (ks >> 3) * 16 + (ks & 1) * 8 + cc; ky = 2 * a + (par >> 1); kx = 2 * b + (par & 1); }
            g[a][b] = (double)p.wd[((size_t)p.where[ky][kx] * p.C + c) * p.N + n];
        }
    const double G[3][2] = {{1, 0}, {1, 1}, {0, 1}};
    const size_t piece0 = (((size_t)ph * (p.N / 64) + nb) * p.nsl + ks) * 9;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double u = 0.0;
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b) u += G[i][a] * g[a][b] * G[j][b];
            p.out[((piece0 + (size_t)(i * 3 + j)) * 2 + nh) * 256 + (size_t)((32 * (cc >> 2) + n32) * 4 + (cc & 3))] = (float)u;
        }
}
