// outgate_kernels.h -- the tail of the reference's decode worker on the card (worker/decode_worker.py:53-59, run.py:194-198): samples are
// appended to a carried fragment with NaN scrubbed, a chunk of `chunk` samples is cut, and the chunk is silent iff
//     power_to_db(|stft(chunk)|^2).mean() < -threshold          n_fft 2048, hop 512, periodic Hann, center=True with reflect padding,
//                                                               amin 1e-10, ref 1.0, top_db 80
// Float64 throughout.  og_append: the fragments of all streams to the other fragment buffer, new samples behind them.  og_frame_db: one
// workgroup per STFT frame, the 2048-point real transform as ONE 1024-point complex transform (lds_fft.h, unchanged) and a split step.
// og_finish: one workgroup per chunk, the clamped mean in a fixed order.  og_emit: the audible chunks times `scale`, float64 or float32.
// No atomics: every reduction is a fixed tree over the LDS or a sequential sum, so a chunk's record does not depend on what else the call holds.
#pragma once
#include "lds_fft.h"

#define OG_FFT 2048
#define OG_HOP 512
#define OG_BINS 1025
#define OG_PAD 1024

// one stream of a call (host-built table, one upload): where its fragment goes, where it comes from, what is cut
struct OgStream {
    long long dst0;          // first sample of its fragment in the buffer the call writes
    long long src0;          // first LIVE sample of its fragment in the buffer the last call wrote
    long long new0;          // first of its new samples in the call's samples
    int keep, n_new;         // carried samples, new samples: the fragment has keep + n_new samples after the call
    int blk0, n_blk;         // its workgroups of og_append: blk0 .. blk0 + n_blk - 1, 256 samples each
    int emit;                // index of its chunk among the call's chunks, -1: none is cut
    int pad;
};

struct OgRecord { int silent, n_inf; double mean_db; };

RY_DEV bool og_is_inf(double v) { return v == __builtin_inf() || v == -__builtin_inf(); }

struct OgAppendParams {
    const OgStream* tab; int n_streams;
    const double* old_frag; const double* fresh; double* frag;
    int chunk;
    int* inf_part;           // [workgroup] +-inf samples among those of the workgroup that belong to the stream's chunk
};

// workgroup x copies 256 samples of one stream's fragment: carried ones from the other buffer, new ones from the call's samples with NaN -> 0.0
RY_KERNEL(256) void og_append(OgAppendParams p) {
    __shared__ int cnt[256];
    const int x = (int)blockIdx.x, tid = (int)threadIdx.x;
    int lo = 0, hi = p.n_streams - 1;                              // last stream with blk0 <= x (streams without a sample share the next one's blk0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.tab[mid].blk0 <= x) lo = mid; else hi = mid - 1;
    }
    const OgStream e = p.tab[lo];
    const int i = (x - e.blk0) * 256 + tid;
    int c = 0;
    if (x - e.blk0 < e.n_blk && i < e.keep + e.n_new) {
        double v;
        if (i < e.keep) v = p.old_frag[e.src0 + i];
        else {
            v = p.fresh[e.new0 + (i - e.keep)];
            if (v != v) v = 0.0;
        }
        p.frag[e.dst0 + i] = v;
        c = (e.emit >= 0 && i < p.chunk && og_is_inf(v)) ? 1 : 0;
    }
    cnt[tid] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) cnt[tid] += cnt[tid + s]; __syncthreads(); }
    if (tid == 0) p.inf_part[x] = cnt[0];
}

struct OgFrameParams {
    const OgStream* tab; const int* stream_of;       // stream_of[c]: the stream of chunk c of the call
    const double* frag;
    int chunk, n_frames;
    const sy_c* tw1024; const sy_c* tw2048;          // (cos, sin)(2 pi k / n), host-computed
    double* db;                                      // [chunk of the call][frame][1025]
    double* fmax;                                    // [chunk of the call][frame]
};

// grid: the frames of all chunks of the call.  Frame f covers samples 512 f - 1024 .. 512 f + 1023 of the chunk, reflected at both ends (chunk >=
// 1025: one reflection per side reaches every index).  z[n] = x[2n] + i x[2n + 1], Z = FFT_1024(z), and for k = 0 .. 1024
//     X[k] = (Z[k] + conj Z[1024 - k]) / 2 - (i / 2) e^{-2 pi i k / 2048} (Z[k] - conj Z[1024 - k])            (Z[1024] = Z[0])
// Thread t takes bins t, t + 256, ...: its reads of Z[k] and Z[1024 - k] are unit-stride 16-byte elements over the lanes, up and down.
RY_KERNEL(256) void og_frame_db(OgFrameParams p) {
    __shared__ sy_c fa[SYNTH_FFT];
    __shared__ sy_c fb[SYNTH_FFT];
    __shared__ double red[256];
    const int tid = (int)threadIdx.x;
    const int c = (int)blockIdx.x / p.n_frames, f = (int)blockIdx.x % p.n_frames;
    const OgStream e = p.tab[p.stream_of[c]];
    const double* x = p.frag + e.dst0;
    const int N = p.chunk;
    for (int n = tid; n < SYNTH_FFT; n += 256) {
        double v[2];
        for (int h = 0; h < 2; ++h) {
            const int j = 2 * n + h;
            int i = f * OG_HOP + j - OG_PAD;
            if (i < 0) i = -i;
            if (i >= N) i = 2 * (N - 1) - i;
            v[h] = x[i] * (0.5 - 0.5 * p.tw2048[j].x);
        }
        sy_c z = {v[0], v[1]};
        fa[n] = z;
    }
    __syncthreads();
    synth_fft(fa, fb, p.tw1024, -1.0);
    double* out = p.db + ((size_t)c * p.n_frames + f) * OG_BINS;
    double m = -__builtin_inf();
    for (int k = tid; k < OG_BINS; k += 256) {
        const sy_c a = fb[k & (SYNTH_FFT - 1)];
        const sy_c b = fb[(SYNTH_FFT - k) & (SYNTH_FFT - 1)];
        const sy_c ev = {0.5 * (a.x + b.x), 0.5 * (a.y - b.y)};          // (Z[k] + conj Z[1024 - k]) / 2
        const sy_c od = {0.5 * (a.y + b.y), -0.5 * (a.x - b.x)};         // -i (Z[k] - conj Z[1024 - k]) / 2
        const sy_c w = {p.tw2048[k].x, -p.tw2048[k].y};
        const sy_c X = sy_add(ev, sy_mul(w, od));
        const double S = X.x * X.x + X.y * X.y;
        const double d = 10.0 * log10(S > 1e-10 ? S : 1e-10);
        out[k] = d;
        m = d > m ? d : m;
    }
    red[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
        __syncthreads();
    }
    if (tid == 0) p.fmax[(size_t)c * p.n_frames + f] = red[0];
}

struct OgFinishParams {
    const OgStream* tab; const int* stream_of;
    const double* db; const double* fmax; const int* inf_part;
    int n_frames;
    double threshold_db;
    OgRecord* rec;                                   // [chunk of the call]
};

// one workgroup per chunk: the maximum over the frame maxima, then the sum of max(db, maximum - 80) -- per frame the threads' partial sums in bin
// order and a fixed tree, the frames one after the other -- and the record.  A chunk with an infinite sample is not silent and its mean is NaN
// (what the numpy expression gives), decided from the count og_append left, not from what the sums carry.
RY_KERNEL(256) void og_finish(OgFinishParams p) {
    __shared__ double red[256];
    __shared__ int cnt[256];
    const int c = (int)blockIdx.x, tid = (int)threadIdx.x;
    const OgStream e = p.tab[p.stream_of[c]];
    const double* fm = p.fmax + (size_t)c * p.n_frames;
    double m = -__builtin_inf();
    for (int f = tid; f < p.n_frames; f += 256) m = fm[f] > m ? fm[f] : m;
    int ni = 0;
    for (int b = tid; b < e.n_blk; b += 256) ni += p.inf_part[e.blk0 + b];
    red[tid] = m; cnt[tid] = ni;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid]; cnt[tid] += cnt[tid + s]; }
        __syncthreads();
    }
    const double floor_db = red[0] - 80.0;
    const int n_inf = cnt[0];
    __syncthreads();
    double total = 0.0;                                            // thread 0's
    for (int f = 0; f < p.n_frames; ++f) {
        const double* row = p.db + ((size_t)c * p.n_frames + f) * OG_BINS;
        double s = 0.0;
        for (int k = tid; k < OG_BINS; k += 256) s += row[k] > floor_db ? row[k] : floor_db;
        red[tid] = s;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) { if (tid < h) red[tid] += red[tid + h]; __syncthreads(); }
        if (tid == 0) total += red[0];
        __syncthreads();
    }
    if (tid == 0) {
        OgRecord r;
        const double mean = total / ((double)p.n_frames * OG_BINS);
        r.n_inf = n_inf;
        r.mean_db = n_inf > 0 ? __builtin_nan("") : mean;
        r.silent = (n_inf == 0 && mean < -p.threshold_db) ? 1 : 0;
        p.rec[c] = r;
    }
}

struct OgEmitParams {
    const OgStream* tab; const int* stream_of; const OgRecord* rec;
    const double* frag;
    int chunk; long long total;                      // samples of all chunks of the call
    double scale;
    double* out64; float* out32;                     // [chunk of the call][chunk samples]: one of the two
};

// grid over the samples of the call's chunks.  The record is read where og_finish left it: a silent chunk writes nothing.  The product is taken
// in float64 and rounded once: the bits of numpy's (wave * scale).astype(float32).
RY_KERNEL(256) void og_emit(OgEmitParams p) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= p.total) return;
    const int c = (int)(g / p.chunk), i = (int)(g % p.chunk);
    if (p.rec[c].silent) return;
    const double v = p.frag[p.tab[p.stream_of[c]].dst0 + i] * p.scale;
    if (p.out32) p.out32[g] = (float)v;
    else p.out64[g] = v;
}
