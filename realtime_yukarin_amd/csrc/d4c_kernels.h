// d4c_kernels.h -- WORLD's D4C (band aperiodicity) of the analysis (analysis.cpp): wave + f0 track -> ap rows and coded_ap, the arithmetic of
// tests/world_d4c_ref.py.  One kernel, d4c_frame: one workgroup of 256 threads per frame, everything of the frame in the LDS, float64.
//   unvoiced (f0 == 0)            the row is filled with 1 - 1e-12: no transform
//   Love Train                    one Blackman window, one 2048-point real transform, two block sums -> a0; a0 <= threshold: the row is filled
//   general body (frames that are on)   two centroids (two transforms each), the smoothed power spectrum (one), DC correction and linear smoothing
//                    (the steps of analysis_frame at 1025 bins), group delay, and per band a Nuttall-windowed transform whose 1025 power values are
//                    sorted in the LDS (bitonic over 2048, padded with +inf) and summed; the B coarse values -> the 513 bins of the row.
// The 2048-point real transform is the 1024-point complex synth_fft of lds_fft.h (untouched) on the even / odd samples as real / imaginary parts
// plus one split pass; a thread keeps its five output bins (tid + 256 q; bin 1024 in thread 0) in registers.
// LDS per workgroup: 2049 complex (32784 B: the two transform buffers; the mirrored cumulative sum of a smoothing -- up to 3073 float64 -- and the
// 2048 sort keys reuse them) + 2 x 1025 float64 (16400 B) + 2 x 256 float64 (4096 B) + a few scalars = 53.3 KB: three workgroups per CU (160 KiB).
// The integers of a frame are decided without floating-point contraction; the branch on a0 is block-uniform (a0 is one LDS value).
// A pure function of its frame: no atomics, nothing shared between workgroups.
#pragma once
#include "analysis_kernels.h"

#define D4C_FFT 2048
#define D4C_HALF 1024
#define D4C_BINS 1025
#define D4C_FLOOR_F0 47.0
#define D4C_LOVE_TRAIN_FLOOR 40.0
#define D4C_MAX_BANDS 3
#define D4C_MAX_NUTTALL 1025
#define D4C_KEY_BASE (1ull << 62)
#define D4C_KEY_BIAS (1ll << 20)
#define D4C_KEY_ORIGIN 8192ll
#define D4C_KEY_WINDOW 2048ull
#define D4C_HANNING 0
#define D4C_BLACKMAN 1

struct D4cFrameInts { long long h3, h4, om, oc, op, L, b1, b2; };
struct D4cFrameRecord { D4cFrameInts v; long long on; double a0; double coarse[D4C_MAX_BANDS]; };

struct D4cParams {
    const double* x; long long x_len;
    const double* f0; const double* t;            // [n]
    double fs, threshold;
    unsigned seed_hash;
    const sy_c* tw;                               // [1024]: (cos, sin)(2 pi k / 1024)
    const sy_c* tw2;                              // [1025]: (cos, sin)(2 pi k / 2048)
    const double* nuttall;                        // [2 band_half + 1]
    int n_bands, band_half;                       // B; floor(3000 N / fs)
    int band_centre[D4C_MAX_BANDS];               // floor(3000 i N / fs)
    int lt0, lt1, lt2;                            // the Love Train's bins: ceil(100 / 4000 / 7900 x 2048 / fs)
    double* ap64; float* ap32; double* coded;     // [n][513], [n][513], [n][n_bands]; any may be null
    D4cFrameRecord* rec;                          // [n] or null
};

RY_DEV long long d4c_round(double v) {            // WORLD's matlab_round: half away from zero
#pragma clang fp contract(off)
    return v > 0 ? (long long)floor(v + 0.5) : -(long long)floor(-v + 0.5);
}

// the decisions of a frame, one rounded operation per step (tests/world_d4c_ref.py: frame_values / frame_integers)
RY_DEV void d4c_decide(double f0_k, double t_k, double fs, double* f, double* fl, double* p, double* u2, D4cFrameInts* v) {
#pragma clang fp contract(off)
    const double ff = f0_k > D4C_FLOOR_F0 ? f0_k : D4C_FLOOR_F0;
    const double fll = f0_k > D4C_LOVE_TRAIN_FLOOR ? f0_k : D4C_LOVE_TRAIN_FLOOR;
    const double r3 = (1.5 * fs) / fll;
    const double r4 = (2.0 * fs) / ff;
    const double q = 0.25 / ff;
    const double tm = t_k - q, tp = t_k + q;
    const double cm0 = tm * fs, cc0 = t_k * fs, cp0 = tp * fs;
    const double cm = cm0 + 0.001, cc = cc0 + 0.001, cp = cp0 + 0.001;
    const double pn = ff * (double)D4C_FFT;
    const double pp = pn / fs;
    const double hn = (ff * 0.5) * (double)D4C_FFT;
    const double uu = hn / fs;
    v->h3 = d4c_round(r3); v->h4 = d4c_round(r4);
    v->om = d4c_round(cm); v->oc = d4c_round(cc); v->op = d4c_round(cp);
    v->L = (long long)floor(pp);
    v->b1 = v->L + 1;
    v->b2 = (long long)floor(uu) + 1;
    *f = ff; *fl = fll; *p = pp; *u2 = uu;
}

// W(f, origin, kind, ratio): thread tid gets samples tid + 256 q of the 2 h + 1 (<= 2048) in v[q], zero behind the window
RY_DEV void d4c_window(const D4cParams& p, double f, long long origin, int h, int kind, double ratio, unsigned which, double* red, double v[8]) {
    const int tid = (int)threadIdx.x;
    const int n_win = 2 * h + 1;
    const unsigned long long key = D4C_KEY_BASE + (unsigned long long)((origin + D4C_KEY_BIAS) * D4C_KEY_ORIGIN) + which * D4C_KEY_WINDOW;
    double w[8], s = 0.0, ws = 0.0;
    for (int q = 0; q < 8; ++q) {
        const int i = tid + 256 * q;
        w[q] = 0.0; v[q] = 0.0;
        if (i < n_win) {
            const int j = i - h;
            long long idx = origin + j;
            idx = idx < 0 ? 0 : idx > p.x_len - 1 ? p.x_len - 1 : idx;
            const double pos = ((2.0 * (double)j) / ratio) / p.fs;
            const double c1 = cos(ANALYSIS_PI * pos * f);
            w[q] = kind == D4C_HANNING ? 0.5 * c1 + 0.5 : 0.42 + 0.5 * c1 + 0.08 * cos(2.0 * ANALYSIS_PI * pos * f);
            v[q] = p.x[idx] * w[q] + synth_noise(p.seed_hash, key + (unsigned long long)i) * ANALYSIS_SAFEGUARD;
            s += v[q]; ws += w[q];
        }
    }
    const double wave_sum = analysis_block_sum(red, s);
    const double win_sum = analysis_block_sum(red, ws);
    const double coef = wave_sum / win_sum;
    for (int q = 0; q < 8; ++q) v[q] = v[q] - w[q] * coef;              // zero stays zero behind the window: w is zero there
}

// 2048-point real transform of the 2048 float64 in `fa` (as 1024 complex: even samples real, odd imaginary): bins tid + 256 q, q < 4, and
// (thread 0) bin 1024 -> out[q]; the other threads' out[4] is zero.  fa and fb are free afterwards.
RY_DEV void d4c_rfft(sy_c* fa, sy_c* fb, const sy_c* tw, const sy_c* tw2, sy_c out[5]) {
    const int tid = (int)threadIdx.x;
    __syncthreads();                                                // the samples are written
    synth_fft(fa, fb, tw, -1.0);
    for (int q = 0; q < 5; ++q) {
        const int k = q < 4 ? tid + 256 * q : D4C_HALF;
        out[q].x = 0.0; out[q].y = 0.0;
        if (q < 4 || tid == 0) {
            const sy_c z = fb[k & (SYNTH_FFT - 1)], zc = fb[(SYNTH_FFT - k) & (SYNTH_FFT - 1)];
            const sy_c e = {0.5 * (z.x + zc.x), 0.5 * (z.y - zc.y)};              // (Z[k] + conj Z[1024 - k]) / 2: the even samples' transform
            const sy_c o = {0.5 * (z.y + zc.y), -0.5 * (z.x - zc.x)};             // (Z[k] - conj Z[1024 - k]) / (2 i): the odd samples'
            const sy_c w = {tw2[k].x, -tw2[k].y};                                 // e^{-2 pi i k / 2048}
            out[q] = sy_add(e, sy_mul(w, o));
        }
    }
    __syncthreads();                                                // fb is read
}

// a[0 .. 1024] += its replica mirrored around p bins (CheapTrick's DC correction at 1025 bins)
RY_DEV void d4c_dc_correction(double* a, double p, int L) {
    const int tid = (int)threadIdx.x;
    const double frac = p - floor(p);
    double rep[5];
    for (int q = 0; q < 5; ++q) {
        const int i = tid + 256 * q;
        rep[q] = 0.0;
        if (i <= L) {                                              // L <= 1023: f < fs / 2
            const double lo = a[L - i];
            const double hi = a[L - i + 1 < D4C_HALF ? L - i + 1 : D4C_HALF];
            rep[q] = lo + (hi - lo) * frac;
        }
    }
    __syncthreads();
    for (int q = 0; q < 5; ++q) {
        const int i = tid + 256 * q;
        if (i <= L) a[i] += rep[q];
    }
    __syncthreads();
}

// linear smoothing of a[0 .. 1024], width u bins, boundary b = floor(u) + 1 <= 1024: sm[q] = the smoothed bin tid + 256 q (thread 0: q = 4 is
// bin 1024).  seg: 1025 + 2 b <= 3073 float64 (the transform buffers).  a is not written.
RY_DEV void d4c_linear_smoothing(const double* a, double u, int b, double* seg, double* part, double sm[5]) {
    const int tid = (int)threadIdx.x;
    const int n_mir = D4C_BINS + 2 * b;
    const int chunk = (n_mir + 255) / 256;                          // <= 13 consecutive values per thread
    const int i0 = tid * chunk, i1 = i0 + chunk < n_mir ? i0 + chunk : n_mir;
    double run = 0.0;
    for (int i = i0; i < i1; ++i) {
        run += i < b ? a[b - i] : i < b + D4C_BINS ? a[i - b] : a[D4C_HALF - 1 - (i - b - D4C_BINS)];
        seg[i] = run;
    }
    part[tid] = run;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                             // inclusive scan of the threads' totals
        const double add = tid >= d ? part[tid - d] : 0.0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const double before = tid > 0 ? part[tid - 1] : 0.0;
    for (int i = i0; i < i1; ++i) seg[i] = before + seg[i];
    __syncthreads();
    for (int q = 0; q < 5; ++q) {
        const int i = q < 4 ? tid + 256 * q : D4C_HALF;
        sm[q] = 0.0;
        if (q < 4 || tid == 0) {
            const double base = (double)i + ((double)b - 0.5);
            const double ph = base + u / 2, pl = base - u / 2;
            const int kh = (int)floor(ph), kl = (int)floor(pl);    // 0 <= kl, kh + 1 < n_mir: u < b, b >= 1
            const double hi = seg[kh] + (seg[kh + 1] - seg[kh]) * (ph - (double)kh);
            const double lo = seg[kl] + (seg[kl + 1] - seg[kl]) * (pl - (double)kl);
            sm[q] = (hi - lo) / u;
        }
    }
    __syncthreads();                                                // seg is read
}

// ascending bitonic sort of key[0 .. 2047]
RY_DEV void d4c_sort(double* key) {
    const int tid = (int)threadIdx.x;
    for (int k = 2; k <= D4C_FFT; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = 0; q < 8; ++q) {
                const int i = tid + 256 * q, l = i ^ j;
                if (l > i) {
                    const double a = key[i], b = key[l];
                    if ((i & k) == 0 ? a > b : a < b) { key[i] = b; key[l] = a; }
                }
            }
            __syncthreads();
        }
}

RY_DEV void d4c_store_row(const D4cParams& p, int k, int i, double o) {
    if (p.ap64) p.ap64[(size_t)k * SYNTH_BINS + i] = o;
    if (p.ap32) p.ap32[(size_t)k * SYNTH_BINS + i] = (float)o;
}

RY_KERNEL(256) void d4c_frame(D4cParams p) {
    __shared__ sy_c fab[D4C_FFT + 1];
    __shared__ double cen[D4C_BINS];                 // static centroid, then the group delay
    __shared__ double pw[D4C_BINS];                  // power spectrum, then the smoothed one
    __shared__ double red[256];
    __shared__ double part[256];
    __shared__ double sh[2 + D4C_MAX_BANDS];         // a0; then the dB values of the row: -60, coarse 1 .. B, -1e-12
    sy_c* fa = fab;
    sy_c* fb = fab + SYNTH_FFT;
    double* rs = reinterpret_cast<double*>(fab);     // the real samples of a transform / the mirrored cumulative sum / the sort keys
    const int tid = (int)threadIdx.x;
    const int k = (int)blockIdx.x;
    const double f0_k = p.f0[k];
    double f, fl, pp, u2;
    D4cFrameInts v;
    d4c_decide(f0_k, p.t[k], p.fs, &f, &fl, &pp, &u2, &v);
    const int h3 = (int)v.h3, h4 = (int)v.h4, L = (int)v.L, b1 = (int)v.b1, b2 = (int)v.b2;
    double w[8];
    sy_c s1[5], s2[5];
    // 1: Love Train (voiced frames)
    double a0 = 0.0;
    if (f0_k != 0.0) {                                                             // block-uniform
        d4c_window(p, fl, v.oc, h3, D4C_BLACKMAN, 3.0, 0u, red, w);
        for (int q = 0; q < 8; ++q) rs[tid + 256 * q] = w[q];
        d4c_rfft(fa, fb, p.tw, p.tw2, s1);
        double lo = 0.0, hi = 0.0;
        for (int q = 0; q < 5; ++q) {
            const int i = q < 4 ? tid + 256 * q : D4C_HALF;
            const double e = s1[q].x * s1[q].x + s1[q].y * s1[q].y;               // zero in the threads that do not hold bin 1024
            if (i > p.lt0 && i <= p.lt1) lo += e;
            if (i > p.lt0 && i <= p.lt2) hi += e;
        }
        const double c1 = analysis_block_sum(red, lo);
        const double c2 = analysis_block_sum(red, hi);
        if (tid == 0) sh[0] = c1 / c2;
        __syncthreads();
        a0 = sh[0];
        __syncthreads();
    }
    const bool on = f0_k != 0.0 && a0 > p.threshold;
    if (tid == 0 && p.rec) {
        D4cFrameRecord r;
        r.v = v; r.on = on ? 1 : 0; r.a0 = a0;
        for (int i = 0; i < D4C_MAX_BANDS; ++i) r.coarse[i] = 0.0;
        p.rec[k] = r;
    }
    if (!on) {
        const double off = 1.0 - ANALYSIS_SAFEGUARD;
        for (int i = tid; i < SYNTH_BINS; i += 256) d4c_store_row(p, k, i, off);
        if (p.coded && tid < p.n_bands) p.coded[(size_t)k * p.n_bands + tid] = 20.0 * log10(off);
        return;
    }
    // 2: static centroid = centroid(t - 0.25 / f) + centroid(t + 0.25 / f), DC correction
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int side = 0; side < 2; ++side) {
        d4c_window(p, f, side == 0 ? v.om : v.op, h4, D4C_BLACKMAN, 4.0, side == 0 ? 1u : 2u, red, w);
        double e = 0.0;
        for (int q = 0; q < 8; ++q) e += w[q] * w[q];
        const double norm = sqrt(analysis_block_sum(red, e));
        for (int q = 0; q < 8; ++q) { w[q] = w[q] / norm; rs[tid + 256 * q] = w[q]; }
        d4c_rfft(fa, fb, p.tw, p.tw2, s1);
        for (int q = 0; q < 8; ++q) rs[tid + 256 * q] = w[q] * (double)(tid + 256 * q + 1);
        d4c_rfft(fa, fb, p.tw, p.tw2, s2);
        for (int q = 0; q < 5; ++q) acc[q] += s1[q].x * s2[q].x + s1[q].y * s2[q].y;
    }
    for (int q = 0; q < 4; ++q) cen[tid + 256 * q] = acc[q];
    if (tid == 0) cen[D4C_HALF] = acc[4];
    __syncthreads();
    d4c_dc_correction(cen, pp, L);
    // 3: smoothed power spectrum
    d4c_window(p, f, v.oc, h4, D4C_HANNING, 4.0, 3u, red, w);
    for (int q = 0; q < 8; ++q) rs[tid + 256 * q] = w[q];
    d4c_rfft(fa, fb, p.tw, p.tw2, s1);
    for (int q = 0; q < 4; ++q) pw[tid + 256 * q] = s1[q].x * s1[q].x + s1[q].y * s1[q].y;
    if (tid == 0) pw[D4C_HALF] = s1[4].x * s1[4].x + s1[4].y * s1[4].y;
    __syncthreads();
    d4c_dc_correction(pw, pp, L);
    double sm[5];
    d4c_linear_smoothing(pw, pp, b1, rs, part, sm);
    // 4: group delay, smoothed over f / 2, minus its smoothing over f
    for (int q = 0; q < 4; ++q) cen[tid + 256 * q] = cen[tid + 256 * q] / sm[q];
    if (tid == 0) cen[D4C_HALF] = cen[D4C_HALF] / sm[4];
    __syncthreads();
    d4c_linear_smoothing(cen, u2, b2, rs, part, sm);
    for (int q = 0; q < 4; ++q) cen[tid + 256 * q] = sm[q];         // every thread has read cen: the smoothing ends with a barrier
    if (tid == 0) cen[D4C_HALF] = sm[4];
    __syncthreads();
    double sm2[5];
    d4c_linear_smoothing(cen, pp, b1, rs, part, sm2);
    for (int q = 0; q < 4; ++q) cen[tid + 256 * q] = sm[q] - sm2[q];
    if (tid == 0) cen[D4C_HALF] = sm[4] - sm2[4];
    __syncthreads();
    // 5: the bands
    if (tid == 0) { sh[0] = -60.0; sh[p.n_bands + 1] = -ANALYSIS_SAFEGUARD; }
    const int n_nut = 2 * p.band_half + 1;
    for (int band = 0; band < p.n_bands; ++band) {
        const int first = p.band_centre[band] - p.band_half;       // >= 0, first + n_nut - 1 <= 1024: the host checks the table
        for (int q = 0; q < 8; ++q) {
            const int i = tid + 256 * q;
            rs[i] = i < n_nut ? cen[first + i] * p.nuttall[i] : 0.0;
        }
        d4c_rfft(fa, fb, p.tw, p.tw2, s1);
        for (int q = 0; q < 4; ++q) {
            rs[tid + 256 * q] = s1[q].x * s1[q].x + s1[q].y * s1[q].y;
            rs[D4C_BINS + tid + 256 * q] = INFINITY;                // 1025 .. 2048; 2048 is the real part of fab[1024], nobody's key
        }
        if (tid == 0) rs[D4C_HALF] = s1[4].x * s1[4].x + s1[4].y * s1[4].y;
        __syncthreads();
        d4c_sort(rs);
        double lo = 0.0, all = 0.0;
        for (int q = 0; q < 4; ++q) {
            const int i = 4 * tid + q;
            all += rs[i];
            if (i <= D4C_HALF - 26) lo += rs[i];
        }
        if (tid == 0) all += rs[D4C_HALF];
        const double s_lo = analysis_block_sum(red, lo);
        const double s_all = analysis_block_sum(red, all);
        if (tid == 0) {
            const double c = 10.0 * log10(s_lo / s_all) + (f - 100.0) / 50.0;
            sh[band + 1] = c < 0.0 ? c : 0.0;
            if (p.rec) p.rec[k].coarse[band] = sh[band + 1];
        }
        __syncthreads();
    }
    // 6: the row
    for (int i = tid; i < SYNTH_BINS; i += 256) {
        const double freq = (double)i * p.fs / (double)SYNTH_FFT;
        int j = (int)floor(freq / 3000.0);
        j = j < p.n_bands ? j : p.n_bands;
        const double x0 = 3000.0 * (double)j, x1 = j < p.n_bands ? 3000.0 * (double)(j + 1) : p.fs / 2.0;
        const double wgt = (freq - x0) / (x1 - x0);
        d4c_store_row(p, k, i, pow(10.0, (sh[j] + (sh[j + 1] - sh[j]) * wgt) / 20.0));
    }
    if (p.coded && tid < p.n_bands) p.coded[(size_t)k * p.n_bands + tid] = 20.0 * log10(pow(10.0, sh[tid + 1] / 20.0));
}
