// analysis_kernels.h -- the kernels of the WORLD analysis (analysis.cpp): wave + f0 track -> CheapTrick spectral envelope and its mel-cepstrum,
// the arithmetic of tests/world_analysis_ref.py (WORLD's CheapTrick and SPTK's sp2mc restated; INTEGRATION.md section 11 lists what deviates).
//   analysis_frame   one workgroup per frame, everything of the frame in the LDS, float64: clamped window gathered from the wave, three block
//                    reductions, power spectrum (1024-point transform of lds_fft.h), DC correction, linear smoothing as a block prefix sum + two
//                    interpolations, floor, log, transform, lifter, transform, exp -> sp row (float64 and / or float32); the liftered cepstrum
//                    times the freqt matrix S -> mc row.  The integers of a frame (window half length, centre sample, DC-correction bin limit,
//                    smoothing boundary) are decided without floating-point contraction: they have to equal the restatement's exactly.
//   analysis_sp2mc   one workgroup per frame of a spectrogram that comes from elsewhere: log, transform, times S.
// Both are pure functions of their frame: no atomics, nothing shared between workgroups, so a row does not depend on what else is in the call.
// At the end of the file: analysis_widen / analysis_check_track (inputs already on the card) and analysis_ingest_tracks (a caller's own f0 track).
#pragma once
#include "lds_fft.h"

#define ANALYSIS_DEFAULT_F0 500.0
#define ANALYSIS_SAFEGUARD 1e-12
#define ANALYSIS_EPS 2.220446049250313e-16
#define ANALYSIS_PI 3.14159265358979323846264338327950288
#define ANALYSIS_KEY_STRIDE 2048
#define ANALYSIS_MIRROR 1280      // >= 513 + 2 * (int(2/3 * 512) + 1): the mirrored spectrum of the highest f0 the host lets through (fs / 2)
#define ANALYSIS_MAX_MC 64

struct AnalysisFrameInts { long long h, centre, L, b; };

struct AnalysisParams {
    const double* x; long long x_len;             // the wave
    const double* f0; const double* t;            // [n]
    double fs, floor_f0, q1;
    unsigned seed_hash;
    const sy_c* tw;                               // [1024]
    const double* S;                              // [513][n_mc] freqt as a matrix
    int n_mc;                                     // order + 1
    double* sp64; float* sp32; double* mc;        // [n][513], [n][513], [n][n_mc]; any may be null
    float* mc32;                                  // [n][n_mc]: (float)mc, the bits of the host's mc.astype(float32); may be null
    AnalysisFrameInts* ints;                      // [n]
};

// the decisions of a frame, one rounded operation per step (tests/world_analysis_ref.py: frame_integers)
RY_DEV void analysis_decide(double f0_k, double t_k, double fs, double floor_f0, double* f0, double* r, double* p, double* u, AnalysisFrameInts* v) {
#pragma clang fp contract(off)
    const double f = f0_k > floor_f0 ? f0_k : ANALYSIS_DEFAULT_F0;
    const double rr = (1.5 * fs) / f;
    const double c = t_k * fs;
    const double c1 = c + 0.001;
    const double pp = (f * (double)SYNTH_FFT) / fs;
    const double uu = (((f * 2.0) / 3.0) * (double)SYNTH_FFT) / fs;
    long long L = (long long)floor(pp);
    if (L > SYNTH_HALF - 1) L = SYNTH_HALF - 1;
    v->h = (long long)floor(rr + 0.5);
    v->centre = (long long)floor(c1 + 0.5);
    v->L = L;
    v->b = (long long)floor(uu) + 1;
    *f0 = f; *r = rr; *p = pp; *u = uu;
}

// sum of red[0 .. 255] in every thread (red is free afterwards)
RY_DEV double analysis_block_sum(double* red, double v) {
    const int tid = (int)threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const double r = red[0];
    __syncthreads();
    return r;
}

// mc[m] = sum over i of c[i] S[i][m]: wave w takes m = w, w + 4, ...; its lanes sum i = lane, lane + 64, ... and meet in a tree
// out32 (may be null): the same sums rounded to float32 once, from the register that holds the float64 sum -- no second pass over `out`
RY_DEV void analysis_freqt(const double* c, const double* S, int n_mc, double* red, double* out, float* out32 = nullptr) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int m0 = 0; m0 < n_mc; m0 += 4) {
        const int m = m0 + wave;
        double acc = 0.0;
        if (m < n_mc)
            for (int i = lane; i < SYNTH_BINS; i += 64) acc += c[i] * S[(size_t)i * n_mc + m];
        red[tid] = acc;
        __syncthreads();
        for (int s = 32; s > 0; s >>= 1) { if (lane < s) red[tid] += red[tid + s]; __syncthreads(); }
        if (lane == 0 && m < n_mc) {
            if (out) out[m] = red[tid];
            if (out32) out32[m] = (float)red[tid];
        }
        __syncthreads();
    }
}

RY_KERNEL(256) void analysis_frame(AnalysisParams p) {
    __shared__ sy_c fa[SYNTH_FFT];
    __shared__ sy_c fb[SYNTH_FFT];
    __shared__ double pw[SYNTH_BINS];                 // power spectrum, then the smoothed one, then its log
    __shared__ double cp[SYNTH_BINS];                 // the liftered cepstrum
    __shared__ double red[256];
    __shared__ double part[256];
    const int tid = (int)threadIdx.x;
    const int k = (int)blockIdx.x;
    double f0, r, pp, u;
    AnalysisFrameInts v;
    analysis_decide(p.f0[k], p.t[k], p.fs, p.floor_f0, &f0, &r, &pp, &u, &v);
    if (tid == 0 && p.ints) p.ints[k] = v;
    const int h = (int)v.h, L = (int)v.L, b = (int)v.b;
    const int n_win = 2 * h + 1;                                   // <= 1021: f0 > 3 fs / 1021 (the host holds floor_f0 to that)
    const unsigned long long key = (unsigned long long)(v.centre * (long long)ANALYSIS_KEY_STRIDE);
    // 2: the window and the windowed wave (thread tid holds samples tid + 256 q)
    double w[4], xs[4], e = 0.0, ws = 0.0;
    for (int q = 0; q < 4; ++q) {
        const int i = tid + 256 * q;
        w[q] = 0.0; xs[q] = 0.0;
        if (i < n_win) {
            const int j = i - h;
            long long idx = v.centre + j;
            idx = idx < 0 ? 0 : idx > p.x_len - 1 ? p.x_len - 1 : idx;
            w[q] = 0.5 * cos(ANALYSIS_PI * ((double)j / r)) + 0.5;
            xs[q] = p.x[idx];
            e += w[q] * w[q];
        }
    }
    const double norm = sqrt(analysis_block_sum(red, e));
    double s = 0.0;
    for (int q = 0; q < 4; ++q) {
        const int i = tid + 256 * q;
        if (i < n_win) {
            w[q] = w[q] / norm;
            xs[q] = xs[q] * w[q] + synth_noise(p.seed_hash, key + (unsigned long long)i) * ANALYSIS_SAFEGUARD;
            s += xs[q]; ws += w[q];
        }
    }
    const double wave_sum = analysis_block_sum(red, s);
    const double win_sum = analysis_block_sum(red, ws);
    const double coef = wave_sum / win_sum;
    for (int q = 0; q < 4; ++q) {
        const int i = tid + 256 * q;
        fa[i].x = i < n_win ? xs[q] - w[q] * coef : 0.0;
        fa[i].y = 0.0;
    }
    __syncthreads();
    // 3: power spectrum, DC correction
    synth_fft(fa, fb, p.tw, -1.0);
    for (int i = tid; i < SYNTH_BINS; i += 256) pw[i] = fb[i].x * fb[i].x + fb[i].y * fb[i].y;
    __syncthreads();
    const double frac = pp - floor(pp);
    double rep[3];
    for (int q = 0; q < 3; ++q) {
        const int i = tid + 256 * q;
        rep[q] = 0.0;
        if (i <= L) {
            const double lo = pw[L - i];
            const double hi = pw[L - i + 1 < SYNTH_HALF ? L - i + 1 : SYNTH_HALF];
            rep[q] = lo + (hi - lo) * frac;
        }
    }
    __syncthreads();
    for (int q = 0; q < 3; ++q) {
        const int i = tid + 256 * q;
        if (i <= L) pw[i] += rep[q];
    }
    __syncthreads();
    // linear smoothing: prefix sum of the mirrored spectrum (five consecutive values per thread, the threads' totals scanned), two interpolations
    double* seg = reinterpret_cast<double*>(fa);                   // [ANALYSIS_MIRROR]
    const int n_mir = SYNTH_BINS + 2 * b;                          // <= 513 + 2 * 342 = 1197 <= ANALYSIS_MIRROR: ry_analysis_run refuses f0 >= fs / 2 (u < 341.4)
    double loc[5], run = 0.0;
    for (int q = 0; q < 5; ++q) {
        const int i = 5 * tid + q;
        double m = 0.0;
        if (i < n_mir) m = i < b ? pw[b - i] : i < b + SYNTH_BINS ? pw[i - b] : pw[SYNTH_HALF - 1 - (i - b - SYNTH_BINS)];
        run += m;
        loc[q] = run;
    }
    part[tid] = run;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                            // inclusive scan of the threads' totals
        const double add = tid >= d ? part[tid - d] : 0.0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const double before = tid > 0 ? part[tid - 1] : 0.0;
    for (int q = 0; q < 5; ++q) seg[5 * tid + q] = before + loc[q];
    __syncthreads();
    double sm[3];
    for (int q = 0; q < 3; ++q) {
        const int i = tid + 256 * q;
        sm[q] = 0.0;
        if (i < SYNTH_BINS) {
            const double base = (double)i + ((double)b - 0.5);
            const double ph = base + u / 2, pl = base - u / 2;
            const int kh = (int)floor(ph), kl = (int)floor(pl);    // 0 <= kl, kh + 1 < n_mir: u < b (so i + 1.5 b < 513 + 2 b), b >= 1; rests on the same host check
            const double hi = seg[kh] + (seg[kh + 1] - seg[kh]) * (ph - (double)kh);
            const double lo = seg[kl] + (seg[kl + 1] - seg[kl]) * (pl - (double)kl);
            sm[q] = (hi - lo) / u + fabs(synth_noise(p.seed_hash, key + 1024ull + (unsigned long long)i)) * ANALYSIS_EPS;
        }
    }
    __syncthreads();                                               // seg (= fa) is read: fa may be written
    // 4: smoothing with recovery
    for (int q = 0; q < 3; ++q) {
        const int i = tid + 256 * q;
        if (i < SYNTH_BINS) {
            const double lg = log(sm[q]);
            fa[i].x = lg; fa[i].y = 0.0;
            if (i > 0 && i < SYNTH_HALF) { fa[SYNTH_FFT - i].x = lg; fa[SYNTH_FFT - i].y = 0.0; }
        }
    }
    __syncthreads();
    synth_fft(fa, fb, p.tw, -1.0);
    for (int q = 0; q < 3; ++q) {
        const int i = tid + 256 * q;
        if (i < SYNTH_BINS) {
            double lift = 1.0;
            if (i > 0) {
                const double qf = (double)i / p.fs;
                const double a = ANALYSIS_PI * f0 * qf;
                lift = (sin(a) / a) * ((1.0 - 2.0 * p.q1) + 2.0 * p.q1 * cos(2.0 * ANALYSIS_PI * f0 * qf));
            }
            cp[i] = fb[i].x * lift / SYNTH_FFT;
        }
    }
    __syncthreads();
    for (int i = tid; i < SYNTH_FFT; i += 256) { fa[i].x = cp[i <= SYNTH_HALF ? i : SYNTH_FFT - i]; fa[i].y = 0.0; }
    __syncthreads();
    synth_fft(fa, fb, p.tw, -1.0);
    for (int i = tid; i < SYNTH_BINS; i += 256) {
        const double o = exp(fb[i].x);
        if (p.sp64) p.sp64[(size_t)k * SYNTH_BINS + i] = o;
        if (p.sp32) p.sp32[(size_t)k * SYNTH_BINS + i] = (float)o;
    }
    // mc: c = irfft(log sp) is the liftered cepstrum; c[0] / 2, then freqt as a matrix
    if (p.mc || p.mc32) {                                          // block-uniform
        if (tid == 0) cp[0] = cp[0] / 2;
        __syncthreads();
        analysis_freqt(cp, p.S, p.n_mc, red, p.mc ? p.mc + (size_t)k * p.n_mc : nullptr, p.mc32 ? p.mc32 + (size_t)k * p.n_mc : nullptr);
    }
}

struct AnalysisSp2mcParams {
    const double* sp64; const float* sp32;        // [n][513]: one of the two
    const sy_c* tw; const double* S; int n_mc;
    double* mc;                                   // [n][n_mc]
};

RY_KERNEL(256) void analysis_sp2mc(AnalysisSp2mcParams p) {
    __shared__ sy_c fa[SYNTH_FFT];
    __shared__ sy_c fb[SYNTH_FFT];
    __shared__ double cp[SYNTH_BINS];
    __shared__ double red[256];
    const int tid = (int)threadIdx.x;
    const size_t row = (size_t)blockIdx.x * SYNTH_BINS;
    for (int i = tid; i < SYNTH_BINS; i += 256) {
        const double lg = log(p.sp64 ? p.sp64[row + i] : (double)p.sp32[row + i]);
        fa[i].x = lg; fa[i].y = 0.0;
        if (i > 0 && i < SYNTH_HALF) { fa[SYNTH_FFT - i].x = lg; fa[SYNTH_FFT - i].y = 0.0; }
    }
    __syncthreads();
    synth_fft(fa, fb, p.tw, -1.0);
    for (int i = tid; i < SYNTH_BINS; i += 256) cp[i] = (i == 0 ? fb[i].x / 2 : fb[i].x) / SYNTH_FFT;
    __syncthreads();
    analysis_freqt(cp, p.S, p.n_mc, red, p.mc + (size_t)blockIdx.x * p.n_mc);
}

// ---------------------------------------------------------------------------------------------
// Inputs that are already on the card (ry_analysis_extract_dev).
//   analysis_widen        the float32 wave another unit uploaded -> the analyzer's float64 wave: (double)x is exact, so the frame kernels see
//                         the bits of the host's `wave.astype(float64)`.
//   analysis_check_track  the refusals ry_analysis_run makes on the host, on a device track: ONE workgroup finds the first frame whose f0 is
//                         not finite or not below fs / 2 (kind 1) or whose t is outside -1 .. 1e6 s (kind 2) and leaves (frame, kind), or
//                         (-1, 0), in verdict[0 .. 1].  The host reads the two words before it launches a frame kernel.
// ---------------------------------------------------------------------------------------------
struct AnalysisWidenParams { const float* x32; double* x64; long long n; };

RY_KERNEL(256) void analysis_widen(AnalysisWidenParams p) {
    const long long i = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (i < p.n) p.x64[i] = (double)p.x32[i];
}

struct AnalysisCheckParams { const double* f0; const double* t; int n; double fs; int* verdict; };

RY_KERNEL(256) void analysis_check_track(AnalysisCheckParams p) {
    __shared__ int first[256];
    const int tid = (int)threadIdx.x;
    int bad = p.n;
    for (int i = tid; i < p.n; i += 256) {
        const double f = p.f0[i], t = p.t[i];
        const bool ok = f - f == 0.0 && f < 0.5 * p.fs && t >= -1.0 && t <= 1e6;      // f - f: NaN for NaN and the infinities
        if (!ok) { bad = i; break; }
    }
    first[tid] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w && first[tid + w] < first[tid]) first[tid] = first[tid + w]; __syncthreads(); }
    if (tid == 0) {
        const int k = first[0];
        int kind = 0;
        if (k < p.n) { const double f = p.f0[k]; kind = (f - f == 0.0 && f < 0.5 * p.fs) ? 2 : 1; }
        p.verdict[0] = k < p.n ? k : -1;
        p.verdict[1] = kind;
    }
}

// ---------------------------------------------------------------------------------------------
// A track that comes from the caller (ry_analysis_ingest_tracks): the f0 of a host tracker -- WORLD mode's Harvest -- for several waves, back to back.
//   analysis_ingest_tracks  one thread per frame of the call.  A thread finds its wave in the segment table (first frame and frames per wave,
//                           ascending: a binary search) and writes, for frame k of that wave, t_64 = (k * frame_period) / 1000 -- two separately
//                           rounded float64 operations, numpy's `arange(n) * frame_period / 1000.0` --, voiced = (f0 != 0) and f0_64 = f0 as it came.
// k counts from the wave's own first frame, so a wave's rows do not depend on where it stands in the call.  Nothing is validated here: the extract
// calls refuse a track by the verdict of analysis_check_track, the one place that does.
// ---------------------------------------------------------------------------------------------
struct AnalysisIngestSeg { int frame0, n_frames; };

struct AnalysisIngestParams {
    const double* f0_in;                          // [n] as uploaded
    const AnalysisIngestSeg* segs; int n_segs;    // segs[i].frame0 ascending from 0, segs[i].frame0 + segs[i].n_frames = segs[i + 1].frame0
    int n;                                        // frames in all
    double frame_period;                          // ms
    double* f0_64; double* t_64; unsigned char* voiced;       // [n]
};

RY_DEV double analysis_frame_time(int k, double frame_period) {
#pragma clang fp contract(off)
    const double ms = (double)k * frame_period;
    return ms / 1000.0;
}

RY_KERNEL(256) void analysis_ingest_tracks(AnalysisIngestParams p) {
    const long long g = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (g >= (long long)p.n) return;
    const int i = (int)g;
    int lo = 0, hi = p.n_segs - 1;                                 // the last segment that starts at or before frame i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.segs[mid].frame0 <= i) lo = mid; else hi = mid - 1;
    }
    const int k = i - p.segs[lo].frame0;
    const double f = p.f0_in[i];
    p.t_64[i] = analysis_frame_time(k, p.frame_period);
    p.voiced[i] = f != 0.0 ? 1 : 0;                                // NaN != 0: voiced, as numpy has it
    p.f0_64[i] = f;
}
