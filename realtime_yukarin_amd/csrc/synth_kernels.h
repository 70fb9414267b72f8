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
// Many streams in one call (ry_synth_bank_push): the same three kernels over a stream table (`bank`; null: the paths above).  Stream b is workgroup b
// of the scan; a pulse finds its stream by bisection over the first response rows, an output sample by bisection over the first output samples.
// An entry carries what `advance` passes per call -- window rows, frame0 / last_frame, the sample range to scan, the pulse slice, the emit range,
// the seed hash -- with positions counted from the start of the STREAM's signal, which is what the noise is keyed by.  Two kernels do what the
// host does for a single stream: synth_gather builds every stream's [kept rows | new rows] window in the other window buffer and puts its carried
// pulses at the front of its slice, synth_retire drops the pulses that can reach no unemitted sample and carries the survivors to the next call.
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
    long long last_idx;           // index of entry n_pulses - 1 (n_pulses > 0): what the host of a bank sizes the emit range by
};

// Stream b of a bank call.  Positions (n0, n1, done, fin, pulse indices) count samples from the start of the stream's signal, frames likewise;
// rows, pulse entries, response rows and output samples count elements of the call's packed arrays.  The host fills the first two groups
// before the scan and the third after it, from the scan state.
struct SynthStream {
    long long frame0, last_frame; // absolute frame of the first row of its window, last frame pushed
    long long n0, n1;             // samples [scanned, k1) to scan
    int row0, rows;               // its window in the call's f0 / sp / ap rows
    int kept, src_row0, new_row0; // gather: rows [0, kept) come from row src_row0 .. of the old window buffer, the rest from row new_row0 .. of the new rows
    int pulse0, pulse_cap;        // its slice of the pulse arrays
    int n_live;                   // carried pulses the gather puts at the front of the slice (= st[b].n_pulses)
    unsigned seed_hash;
    int active, final;            // takes part in this call (frames or final); its signal ends with this call
    int n_pulses, n_complete;     // entries after the scan; pulses whose response is computed
    int resp0;                    // first response row
    long long done, fin;          // emits samples [done, fin)
    long long out0;               // ... to y[out0 ..]
};

// what synth_retire leaves for the host: the carried pulses and the index of the first one (the oldest frame a later call reads)
struct SynthRetired { long long first_idx; int n_live; int overflow; };

// the stream of element j of a packed array whose stream b starts at start(b): the LAST b with start <= j (a stream without elements shares its
// start with the next one and is passed over)
#define SYNTH_STREAM_OF(bank, n, j, field, out)                    \
    do {                                                           \
        int lo__ = 0, hi__ = (n) - 1;                              \
        while (lo__ < hi__) {                                      \
            const int mid__ = (lo__ + hi__ + 1) >> 1;              \
            if ((bank)[mid__].field <= (j)) lo__ = mid__; else hi__ = mid__ - 1; \
        }                                                          \
        (out) = lo__;                                              \
    } while (0)

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
    const SynthStream* bank;      // many streams: one workgroup each (grid = streams); f0 and the pulse arrays are the call's packed ones, st[b] the
                                  // stream's carried state; frame0, last_frame, n0, n1 and cap are not read
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
    if (p.bank) {                                                  // this workgroup's stream: its window, carried state and pulse slice, samples [n0, n1) of its signal
        const SynthStream e = p.bank[blockIdx.x];
        if (!e.active) return;                                     // block-uniform: a stream that sits the call out keeps its state as it is
        p.f0 += e.row0; p.frame0 = e.frame0; p.last_frame = e.last_frame; p.n0 = e.n0; p.n1 = e.n1;
        p.st += blockIdx.x;
        p.pidx += e.pulse0; p.pshift += e.pulse0; p.pvoiced += e.pulse0; p.cap = e.pulse_cap;
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
        const int n = base > p.cap ? p.cap : base;
        p.st->n_pulses = n;
        if (n > 0) p.st->last_idx = p.pidx[n - 1];                 // written by this workgroup before the loop's last barrier, or carried
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
    // many streams: grid = the response rows of all streams; the pulse arrays and sp / ap are the call's packed ones; n_pulses, n_complete, frame0,
    // last_frame and seed_hash are not read
    const SynthStream* bank; int n_streams;
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
    if (p.bank) {                                                  // block-uniform: response row j is pulse j - resp0 of stream b
        int b;
        SYNTH_STREAM_OF(p.bank, p.n_streams, j, resp0, b);
        const SynthStream e = p.bank[b];
        p.n_pulses = e.n_pulses;
        j -= e.resp0;
        p.pidx += e.pulse0; p.pshift += e.pulse0; p.pvoiced += e.pulse0;
        p.sp += (size_t)e.row0 * SYNTH_BINS; p.ap += (size_t)e.row0 * SYNTH_BINS;
        p.frame0 = e.frame0; p.last_frame = e.last_frame; p.seed_hash = e.seed_hash;
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
    const SynthStream* bank; int n_streams;      // many streams: s0 = 0, s1 = the samples the call emits; sample out0 + i of y is sample done + i of stream b
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
    if (p.bank) {
        int b;
        SYNTH_STREAM_OF(p.bank, p.n_streams, s, out0, b);
        const SynthStream e = p.bank[b];
        p.pidx += e.pulse0; p.n_complete = e.n_complete; p.resp += (size_t)e.resp0 * SYNTH_FFT;
        p.y += e.out0; s += e.done - e.out0; p.s0 = e.done;        // y[s - done] below: the stream's own position s
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

// ---- the two steps a bank does on the card (a single stream does them on the host: append_frames and the end of `advance`) ----------------------
struct SynthGatherParams {
    const SynthStream* bank; int n_streams;
    int rows;                                     // rows of all windows
    const float *old_sp, *old_ap;                 // the window buffer of the last call
    const float *new_sp, *new_ap;                 // the call's new rows, streams back to back (the packed upload, or the caller's device rows)
    float *sp, *ap;                               // the other window buffer: [stream][kept rows | new rows]
    const long long* c_idx; const double* c_shift; const int* c_voiced; int carry_cap;     // carried pulses [stream][carry_cap]
    long long* pidx; double* pshift; int* pvoiced;
};

// one row of 513 floats, 16 bytes per lane where source and destination sit alike in their 16-byte lines, 4 otherwise
RY_DEV void synth_copy_row(float* d, const float* s) {
    const int tid = (int)threadIdx.x;
    if ((((size_t)d ^ (size_t)s) & 15) == 0) {
        const int head = (int)(((16 - ((size_t)d & 15)) & 15) >> 2);
        const int n4 = (SYNTH_BINS - head) >> 2;                   // <= 128
        if (tid < n4) ry_st4(d + head + 4 * tid, ry_ld4(s + head + 4 * tid));
        const int tail = head + 4 * n4;
        if (tid >= 128 && tid - 128 < head) d[tid - 128] = s[tid - 128];
        if (tid >= 192 && tail + tid - 192 < SYNTH_BINS) d[tail + tid - 192] = s[tail + tid - 192];
    } else {
        for (int i = tid; i < SYNTH_BINS; i += 256) d[i] = s[i];
    }
}

// grid (max(rows, streams), 3): y = 0 / 1 the sp / ap row blockIdx.x of the new window buffer, y = 2 the carried pulses of stream blockIdx.x
RY_KERNEL(256) void synth_gather(SynthGatherParams p) {
    const int x = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (blockIdx.y == 2) {
        if (x >= p.n_streams) return;
        const SynthStream e = p.bank[x];
        if (!e.active) return;
        const size_t c0 = (size_t)x * p.carry_cap;
        for (int i = tid; i < e.n_live; i += 256) {
            p.pidx[e.pulse0 + i] = p.c_idx[c0 + i];
            p.pshift[e.pulse0 + i] = p.c_shift[c0 + i];
            p.pvoiced[e.pulse0 + i] = p.c_voiced[c0 + i];
        }
        return;
    }
    if (x >= p.rows) return;
    int b;
    SYNTH_STREAM_OF(p.bank, p.n_streams, x, row0, b);
    const SynthStream e = p.bank[b];
    const int r = x - e.row0;
    const float* old = blockIdx.y == 0 ? p.old_sp : p.old_ap;
    const float* nw = blockIdx.y == 0 ? p.new_sp : p.new_ap;
    float* out = blockIdx.y == 0 ? p.sp : p.ap;
    const float* src = r < e.kept ? old + (size_t)(e.src_row0 + r) * SYNTH_BINS : nw + (size_t)(e.new_row0 + r - e.kept) * SYNTH_BINS;
    synth_copy_row(out + (size_t)x * SYNTH_BINS, src);
}

struct SynthRetireParams {
    const SynthStream* bank;
    SynthScanState* st;
    const long long* pidx; const double* pshift; const int* pvoiced;
    long long* c_idx; double* c_shift; int* c_voiced; int carry_cap;
    SynthRetired* out;
};

// One workgroup per stream, after the overlap: pulses that cannot reach an unemitted sample -- index below fin - 512 -- leave the list, the last
// one always stays (it has no successor yet); the survivors go to the front of the stream's carry slot.  The indices rise, so the pulses that
// leave are a prefix and counting them is finding its length.  A stream whose signal ends is left as a new one.
RY_KERNEL(256) void synth_retire(SynthRetireParams p) {
    __shared__ int cnt[256];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const SynthStream e = p.bank[b];
    if (!e.active) return;                                         // block-uniform
    if (e.final) {
        if (tid == 0) {
            SynthScanState z;
            z.phase = 0.0; z.last_voiced = 0; z.n_pulses = 0; z.overflow = 0; z.pad = 0; z.last_idx = 0;
            p.st[b] = z;
            SynthRetired r;
            r.first_idx = -1; r.n_live = 0; r.overflow = 0;
            p.out[b] = r;
        }
        return;
    }
    const long long* idx = p.pidx + e.pulse0;
    int c = 0;
    for (int j = tid; j + 1 < e.n_pulses; j += 256) c += idx[j] < e.fin - SYNTH_HALF ? 1 : 0;
    cnt[tid] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) cnt[tid] += cnt[tid + s]; __syncthreads(); }
    const int drop = cnt[0];
    const int keep = e.n_pulses - drop;
    const int n = keep < p.carry_cap ? keep : p.carry_cap;
    const size_t c0 = (size_t)b * p.carry_cap;
    for (int i = tid; i < n; i += 256) {
        p.c_idx[c0 + i] = idx[drop + i];
        p.c_shift[c0 + i] = p.pshift[e.pulse0 + drop + i];
        p.c_voiced[c0 + i] = p.pvoiced[e.pulse0 + drop + i];
    }
    if (tid == 0) {
        p.st[b].n_pulses = n;
        SynthRetired r;
        r.first_idx = keep > 0 ? idx[drop] : -1; r.n_live = n; r.overflow = keep - n;
        p.out[b] = r;
    }
}
