// synth_kernels.h -- the kernels of the WORLD synthesizer (synth.cpp): f0 / sp / ap frames -> waveform, the arithmetic of
// tests/world_synth_ref.py (WORLD's Synthesis with fractional pulse shifts, restated; INTEGRATION.md section 10 lists what deviates).
//   synth_scan      time base + pulse scan, float64, ONE workgroup: per block of 1024 samples every thread interpolates f0 / the voiced flag
//                   for four samples, thread 0 advances the wrapped phase through the block in order (the only sequential part: one add, one
//                   compare, one select per sample), every thread turns the wraps of its four samples into pulses, appended in order.
//                   The phase is carried in SynthScanState, so the sums depend on the absolute sample position only: a stream cut anywhere
//                   gives the same bits.  No floating-point contraction here: the pulse indices have to equal the restatement's exactly.
//   synth_pulse     one workgroup per pulse: interpolated spectrum / aperiodicity row, counter-based noise, seven 1024-point transforms in
//                   the LDS (float64, radix-4 Stockham, five passes, one butterfly per thread and pass) -> response row [1024] (float64).
//   synth_overlap   overlap-add as a gather: one thread per output sample finds its pulses by binary search and sums their contributions in
//                   ascending pulse order.  No atomics: run-to-run and cut-to-cut bit identity depend on it.
// Many waves in one call (ry_synth_run_many): the same three kernels over a segment table (`seg`; null: one wave, the call's own sizes).  A
// workgroup or thread finds its wave -- the scan by its block index, a pulse by bisection over the compact response starts, an output sample by
// bisection over the sample starts, which rise strictly because every wave has at least one sample -- and from there on works with that wave's
// own rows, pulse slice, state and sample positions: frame 0 is the wave's first row, sample 0 its first sample.  The arithmetic is the single
// call's, on the same numbers.
#pragma once
#include "lds_fft.h"               // the 1024-point transform (synth_fft) and the counter-based noise (synth_noise)

#define SYNTH_BLOCK 1024          // samples per block of the scan
#define SYNTH_DEFAULT_F0 500.0
#define SYNTH_SAFEGUARD 1e-12
#define SYNTH_AP_LO 0.001
#define SYNTH_AP_HI 0.999999999999

struct SynthScanState {
    double phase;                 // wrapped phase after the last sample seen
    int last_voiced;              // voiced flag of that sample
    int n_pulses;                 // entries of the pulse arrays (old ones the host put there + the ones this launch appended)
    int overflow;                 // pulses that did not fit (the host sizes the arrays by the sample count: stays 0)
    int pad;
};

// Wave b of a batched call.  Everything is counted in elements of the packed arrays: rows of f0 / sp / ap, entries of the pulse arrays (the
// slice holds n_samples + 1: a sample gives at most one pulse), samples of the output.
struct SynthSeg { int row0, n_frames, pulse0, pulse_cap, sample0, n_samples; };

// the wave whose first sample is the last one at or before s
RY_DEV int synth_seg_of_sample(const SynthSeg* seg, int n_seg, long long s) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid].sample0 <= s) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the wave of compact pulse j: the LAST b with rstart[b] <= j (a wave without pulses shares its start with the next one and is passed over)
RY_DEV int synth_seg_of_pulse(const int* rstart, int n_seg, int j) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rstart[mid] <= j) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct SynthScanParams {
    const double* f0;             // thresholded f0 of frames frame0 .. (0 = unvoiced)
    long long frame0, last_frame; // positions at or behind last_frame take that frame
    long long n0, n1;             // samples [n0, n1)
    double spf, fs;               // samples per frame, sampling rate
    SynthScanState* st;
    long long* pidx; double* pshift; int* pvoiced; int cap;
    const SynthSeg* seg;          // many waves: one workgroup each (grid = waves); f0, st and the pulse arrays are the packed ones, the wave's
                                  // st[b] zeroed by the host; frame0, last_frame, n0, n1 and cap are not read
};

RY_KERNEL(256) void synth_scan(SynthScanParams p) {
#pragma clang fp contract(off)
    __shared__ double dphi[SYNTH_BLOCK];
    __shared__ double wr[SYNTH_BLOCK + 1];            // wrapped phase BEFORE each sample's step, then after the last
    __shared__ unsigned char vo[SYNTH_BLOCK + 1];     // voiced flag of the sample before the block, then of each sample
    __shared__ unsigned char wrapped[SYNTH_BLOCK];
    __shared__ int cnt[256];
    __shared__ int base;
    const int tid = (int)threadIdx.x;
    if (p.seg) {                                                   // this workgroup's wave: its own rows, state and pulse slice, samples [0, n_samples)
        const SynthSeg sg = p.seg[blockIdx.x];
        p.f0 += sg.row0; p.frame0 = 0; p.last_frame = sg.n_frames - 1; p.n0 = 0; p.n1 = sg.n_samples;
        p.st += blockIdx.x;
        p.pidx += sg.pulse0; p.pshift += sg.pulse0; p.pvoiced += sg.pulse0; p.cap = sg.pulse_cap;
    }
    if (tid == 0) { base = p.st->n_pulses; wr[0] = p.st->phase; vo[0] = (unsigned char)p.st->last_voiced; }
    __syncthreads();
    for (long long b0 = p.n0; b0 < p.n1; b0 += SYNTH_BLOCK) {
        const int nb = (int)(p.n1 - b0 < SYNTH_BLOCK ? p.n1 - b0 : SYNTH_BLOCK);
        for (int i = tid; i < nb; i += 256) {
            const double pos = (double)(b0 + i) / p.spf;
            long long k = (long long)floor(pos);
            double w = pos - (double)k;
            long long k0 = k, k1 = k + 1;
            if (k >= p.last_frame) { k0 = k1 = p.last_frame; w = 0.0; }
            const double fa = p.f0[k0 - p.frame0], fb = p.f0[k1 - p.frame0];
            const double va = fa != 0.0 ? 1.0 : 0.0, vb = fb != 0.0 ? 1.0 : 0.0;
            const double f = fa + (fb - fa) * w;
            const double v = va + (vb - va) * w;
            const bool voiced = v > 0.5;
            dphi[i] = SYNTH_TWO_PI * (voiced ? f : SYNTH_DEFAULT_F0) / p.fs;
            vo[i + 1] = voiced ? 1 : 0;
        }
        __syncthreads();
        if (tid == 0) {
            double ph = wr[0];
            for (int i = 0; i < nb; ++i) {
                const double nw = ph + dphi[i];
                const bool wrap = nw >= SYNTH_TWO_PI;
                wrapped[i] = wrap ? 1 : 0;
                ph = wrap ? nw - SYNTH_TWO_PI : nw;
                wr[i + 1] = ph;
            }
        }
        __syncthreads();
        int c = 0;
        for (int i = 4 * tid; i < 4 * tid + 4 && i < nb; ++i) c += wrapped[i];
        cnt[tid] = c;
        __syncthreads();
        int off = base;
        for (int t = 0; t < tid; ++t) off += cnt[t];
        for (int i = 4 * tid; i < 4 * tid + 4 && i < nb; ++i) {
            if (!wrapped[i]) continue;
            if (off < p.cap) {
                const double y1 = wr[i] - SYNTH_TWO_PI;                   // the phase before the step, one turn down
                const double y2 = wr[i + 1];                              // (wr[i] + dphi[i]) - 2 pi
                p.pidx[off] = b0 + i - 1;
                p.pshift[off] = -y1 / (y2 - y1);
                p.pvoiced[off] = vo[i];                                   // the flag of sample b0 + i - 1
            }
            ++off;
        }
        __syncthreads();
        if (tid == 255) base = off;                                       // thread 255 has seen every count
        if (tid == 0) { wr[0] = wr[nb]; vo[0] = vo[nb]; }
        __syncthreads();
    }
    if (tid == 0) {
        p.st->phase = wr[0];
        p.st->last_voiced = vo[0];
        p.st->overflow = base > p.cap ? base - p.cap : 0;
        p.st->n_pulses = base > p.cap ? p.cap : base;
    }
}

struct SynthPulseParams {
    const long long* pidx; const double* pshift; const int* pvoiced;
    int n_pulses;                 // entries of the pulse arrays (a pulse's noise size = distance to the next entry)
    int n_complete;               // = grid: pulses whose response is computed; entry n_pulses - 1 may be among them only at the end of a
                                  // signal (noise size 0: no response)
    const float* sp; const float* ap;     // rows of frames frame0 .. , [row][513]
    long long frame0, last_frame;
    double spf;
    unsigned seed_hash;
    const sy_c* tw;               // [1024]
    const double* dc;             // [1024] raised-cosine DC remover, normalised
    double* resp;                 // [n_complete][1024]
    // many waves: grid = the pulses of all waves; rstart [n_seg + 1] = the first response row of every wave (the running sum of the waves' pulse
    // counts), the pulse arrays and sp / ap are the packed ones; n_pulses, n_complete, frame0 and last_frame are not read
    const SynthSeg* seg; const int* rstart; int n_seg;
};

// minimum phase of the log-amplitude in lg[0 .. 512] -> spectrum on bins 0 .. 512 in `out` (uses a, b)
RY_DEV void synth_minimum_phase(const double* lg, sy_c* a, sy_c* b, const sy_c* tw, sy_c* out) {
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < SYNTH_FFT; i += 256) { a[i].x = lg[i <= SYNTH_HALF ? i : SYNTH_FFT - i]; a[i].y = 0.0; }
    __syncthreads();
    synth_fft(a, b, tw, -1.0);                                    // cepstrum (unnormalised) in b
    for (int i = tid; i < SYNTH_FFT; i += 256) {
        const double g = i == 0 ? 1.0 : i <= SYNTH_HALF ? 2.0 : 0.0;
        a[i].x = b[i].x * g; a[i].y = b[i].y * g;
    }
    __syncthreads();
    synth_fft(a, b, tw, -1.0);
    for (int i = tid; i < SYNTH_BINS; i += 256) {
        const double m = exp(b[i].x / SYNTH_FFT), ph = b[i].y / SYNTH_FFT;
        out[i].x = m * cos(ph); out[i].y = m * sin(ph);
    }
    __syncthreads();
}

// real signal of the Hermitian spectrum whose bins 0 .. 512 are in `half` (imaginary parts of bins 0 and 512 ignored, as a
// complex-to-real transform does), unnormalised, fftshifted -> real parts in b[].x  (uses a, b)
RY_DEV void synth_inverse_real(const sy_c* half, sy_c* a, sy_c* b, const sy_c* tw) {
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < SYNTH_FFT; i += 256) {
        sy_c v;
        if (i <= SYNTH_HALF) { v = half[i]; if (i == 0 || i == SYNTH_HALF) v.y = 0.0; }
        else { v = half[SYNTH_FFT - i]; v.y = -v.y; }
        a[i] = v;
    }
    __syncthreads();
    synth_fft(a, b, tw, 1.0);
}

RY_KERNEL(256) void synth_pulse(SynthPulseParams p) {
    __shared__ sy_c fa[SYNTH_FFT];
    __shared__ sy_c fb[SYNTH_FFT];
    __shared__ sy_c mp[SYNTH_BINS];                   // minimum-phase spectrum (then the product that is transformed back)
    __shared__ double sp[SYNTH_BINS];
    __shared__ double ap[SYNTH_BINS];                 // squared aperiodicity
    __shared__ double lg[SYNTH_BINS];
    __shared__ double per[SYNTH_FFT];                 // periodic response (fftshifted, DC removed)
    __shared__ double red[256];
    const int tid = (int)threadIdx.x;
    int j = (int)blockIdx.x;
    double* out = p.resp + (size_t)j * SYNTH_FFT;
    if (p.seg) {                                                   // block-uniform: response row j is pulse j - rstart[b] of wave b, whose last pulse has no successor
        const int b = synth_seg_of_pulse(p.rstart, p.n_seg, j);
        const SynthSeg sg = p.seg[b];
        p.n_pulses = p.rstart[b + 1] - p.rstart[b];
        j -= p.rstart[b];
        p.pidx += sg.pulse0; p.pshift += sg.pulse0; p.pvoiced += sg.pulse0;
        p.sp += (size_t)sg.row0 * SYNTH_BINS; p.ap += (size_t)sg.row0 * SYNTH_BINS;
        p.frame0 = 0; p.last_frame = sg.n_frames - 1;
    }
    const long long idx = p.pidx[j];
    const long long ns_true = j + 1 < p.n_pulses ? p.pidx[j + 1] - idx : 0;
    if (ns_true <= 0) {                                            // block-uniform
        for (int i = tid; i < SYNTH_FFT; i += 256) out[i] = 0.0;
        return;
    }
    const int ns = (int)(ns_true < SYNTH_FFT ? ns_true : SYNTH_FFT);
    const bool voiced = p.pvoiced[j] != 0;
    const double pos = (double)idx / p.spf;
    long long k0 = (long long)floor(pos), k1 = (long long)ceil(pos);
    if (k0 > p.last_frame) k0 = p.last_frame;
    if (k1 > p.last_frame) k1 = p.last_frame;
    const double w = pos - (double)k0;
    const float* s0 = p.sp + (size_t)(k0 - p.frame0) * SYNTH_BINS;
    const float* s1 = p.sp + (size_t)(k1 - p.frame0) * SYNTH_BINS;
    const float* a0 = p.ap + (size_t)(k0 - p.frame0) * SYNTH_BINS;
    const float* a1 = p.ap + (size_t)(k1 - p.frame0) * SYNTH_BINS;
    for (int i = tid; i < SYNTH_BINS; i += 256) {
        double s = fabs((double)s0[i]);
        double a = fmin(fmax((double)a0[i], SYNTH_AP_LO), SYNTH_AP_HI);
        a *= a;
        if (k0 != k1) {
            double a2 = fmin(fmax((double)a1[i], SYNTH_AP_LO), SYNTH_AP_HI);
            a2 *= a2;
            s = (1.0 - w) * s + w * fabs((double)s1[i]);
            a = (1.0 - w) * a + w * a2;
        }
        sp[i] = s; ap[i] = a;
    }
    __syncthreads();
    const bool periodic = voiced && !(ap[0] > 0.999);              // block-uniform
    if (periodic) {
        for (int i = tid; i < SYNTH_BINS; i += 256) lg[i] = log(sp[i] * (1.0 - ap[i]) + SYNTH_SAFEGUARD) / 2.0;
        __syncthreads();
        synth_minimum_phase(lg, fa, fb, p.tw, mp);
        const double coef = SYNTH_TWO_PI * p.pshift[j] / SYNTH_FFT;
        for (int i = tid; i < SYNTH_BINS; i += 256) {
            const double ang = coef * (double)i;
            const sy_c r = {cos(ang), -sin(ang)};
            mp[i] = sy_mul(mp[i], r);
        }
        __syncthreads();
        synth_inverse_real(mp, fa, fb, p.tw);
        // fftshift: position i holds sample (i + 512) mod 1024; DC of the second half (the causal part), first half replaced
        double part = fb[tid].x + fb[tid + 256].x;                // positions 512 + tid, 768 + tid
        red[tid] = part;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
        const double dcv = red[0];
        for (int i = tid; i < SYNTH_FFT; i += 256)
            per[i] = (i < SYNTH_HALF ? 0.0 : fb[i - SYNTH_HALF].x) - dcv * p.dc[i];
        __syncthreads();
    }
    // noise: ns mean-removed samples (their sum is exact: every sample is a multiple of 2^-24), zeros behind them
    double g[4];
    double part = 0.0;
    for (int q = 0; q < 4; ++q) {
        const int i = tid + 256 * q;
        g[q] = i < ns ? synth_noise(p.seed_hash, (unsigned long long)(idx + i)) : 0.0;
        part += g[q];
    }
    red[tid] = part;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const double mean = red[0] / (double)ns;
    for (int q = 0; q < 4; ++q) {
        const int i = tid + 256 * q;
        fa[i].x = i < ns ? g[q] - mean : 0.0; fa[i].y = 0.0;
    }
    for (int i = tid; i < SYNTH_BINS; i += 256) lg[i] = log(voiced ? sp[i] * ap[i] : sp[i]) / 2.0;
    __syncthreads();
    synth_fft(fa, fb, p.tw, -1.0);                                 // noise spectrum in fb
    for (int i = tid; i < SYNTH_BINS; i += 256) { sp[i] = fb[i].x; ap[i] = fb[i].y; }     // sp / ap are free now: keep bins 0 .. 512
    __syncthreads();
    synth_minimum_phase(lg, fa, fb, p.tw, mp);
    for (int i = tid; i < SYNTH_BINS; i += 256) {
        const sy_c n = {sp[i], ap[i]};
        mp[i] = sy_mul(mp[i], n);
    }
    __syncthreads();
    synth_inverse_real(mp, fa, fb, p.tw);
    const double sq = sqrt((double)ns_true);
    for (int i = tid; i < SYNTH_FFT; i += 256) {
        const double apr = fb[(i + SYNTH_HALF) & (SYNTH_FFT - 1)].x;
        out[i] = ((periodic ? per[i] * sq : 0.0) + apr) / SYNTH_FFT;
    }
}

// y[s - s0] = sum over the pulses with index in [s - 512, s + 511], ascending, of resp[pulse][s - index + 511]
// many waves: s0 = 0, s1 = the samples of all waves, y the packed output; a sample of wave b sees that wave's pulses and response rows only
struct SynthOverlapParams {
    const long long* pidx; int n_complete; const double* resp; long long s0, s1; double* y;
    const SynthSeg* seg; const int* rstart; int n_seg;
};

RY_KERNEL(256) void synth_overlap(SynthOverlapParams p) {
    long long s = p.s0 + (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= p.s1) return;
    if (p.seg) {
        const int b = synth_seg_of_sample(p.seg, p.n_seg, s);
        const SynthSeg sg = p.seg[b];
        p.pidx += sg.pulse0; p.n_complete = p.rstart[b + 1] - p.rstart[b]; p.resp += (size_t)p.rstart[b] * SYNTH_FFT;
        p.y += sg.sample0; s -= sg.sample0;                        // p.s0 = 0: y[s] below is the wave's own sample s
    }
    int lo = 0, hi = p.n_complete;                                 // first pulse with index >= s - 512
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p.pidx[mid] < s - SYNTH_HALF) lo = mid + 1; else hi = mid;
    }
    double acc = 0.0;
    for (int j = lo; j < p.n_complete; ++j) {
        const long long d = s - p.pidx[j] + (SYNTH_HALF - 1);
        if (d < 0) break;
        acc += p.resp[(size_t)j * SYNTH_FFT + d];
    }
    p.y[s - p.s0] = acc;
}
