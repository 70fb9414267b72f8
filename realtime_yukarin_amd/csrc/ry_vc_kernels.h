// ry_vc_kernels.h -- the small kernels of the window call (ry_vc.cpp): combine_silent (row scatter; ry_mask_rows for rows that are already
// in place; ry_gather_rows for rows that are packed elsewhere), the silence gate (frame power in numpy's summation order, gate + ordered compaction;
// the same two over a table of waves) and decode_spectrogram (mc2sp = exp(mc @ M)).
// Reference: /root/reference/realtime_voice_conversion/yukarin_wrapper/voice_changer.py:27-39.
#pragma once
#include "ry_dev.h"

// ---------------------------------------------------------------------------------------------
// Between the two CNNs: `AcousticConverter.combine_silent` (scatter converted rows into an all-silent block) and
// `decode_spectrogram` = pysptk.mc2sp.  mc2sp is freqt(-alpha) -> c0 *= 2 -> symmetric extension -> Re(rfft) -> exp;
// everything before the exp is linear in the mel-cepstrum, so sp = exp(mc @ M) with an (order+1) x (fftlen/2+1)
// matrix M computed once on the host in float64 (realtime_yukarin_amd/sptk.py).  `floor` is the 1e-16 the reference
// adds before stage-2 (voice_changer.py:39).
// ---------------------------------------------------------------------------------------------
struct RyScatterParams { const float* src; const int* row_of; float* dst; int n_src, cols; };

RY_KERNEL(256) void ry_scatter_rows(RyScatterParams p) {       // dst[row_of[i]][:] = src[i][:]
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.n_src * p.cols) return;
    const int c = (int)(idx % p.cols), i = (int)(idx / p.cols);
    p.dst[(size_t)p.row_of[i] * p.cols + c] = p.src[idx];
}

// `combine_silent` for rows that never left their block (the aperiodicity of a resident chain: AcousticConverter.convert passes ap through,
// combine_silent leaves zeros on the frames the gate cut): rows k0 .. k1 - 1 of rows[n][cols] whose mask byte is 0 become +0.0f, the others
// and everything outside the range keep their bits.  One wave per row, four rows per workgroup; a silent row is written as scalars up to the
// first 16-byte boundary, 128-bit stores over the whole quads, scalars for what is left (cols = 513: rows start at every alignment).
struct RyMaskRowsParams { float* rows; const unsigned char* mask; int cols, k0, k1; };

RY_KERNEL(256) void ry_mask_rows(RyMaskRowsParams p) {
    const int lane = (int)threadIdx.x & 63;
    const long long r = (long long)p.k0 + (long long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (r >= p.k1 || p.mask[r] != 0) return;                    // wave-uniform
    float* row = p.rows + (size_t)r * p.cols;
    int head = (int)((4 - ((reinterpret_cast<unsigned long long>(row) >> 2) & 3)) & 3);     // floats in front of the first 16-byte boundary
    if (head > p.cols) head = p.cols;
    const int quads = (p.cols - head) >> 2, tail = head + 4 * quads;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (lane < head) row[lane] = 0.f;
    for (int q = lane; q < quads; q += 64) ry_st4(row + head + 4 * q, zero);
    if (tail + lane < p.cols) row[tail + lane] = 0.f;          // at most three
}

// Rows picked by an index table, packed back to back: dst[j][:] = (mask == null || mask[src_row[j]]) ? rows[src_row[j]][:] : +0.0f for j < n_out --
// the rows [front, n_b - back) of every stream of a call in the order ry_synth_bank_push reads them, with combine_silent folded in for the
// aperiodicity.  One wave per output row, four rows per workgroup.  Source and destination rows start at any 4-byte alignment, independently
// (cols = 513): the destination is written as scalars up to its first 16-byte boundary, 128-bit stores over the whole quads, scalars for the rest;
// a quad is read with one 128-bit load when the source row has the destination's residue, else as four scalars.  Nothing outside a row is
// read or written; an index outside 0 .. n_rows - 1 reads nothing and gives a row of zeros.
struct RyGatherRowsParams { const float* rows; const int* src_row; const unsigned char* mask; float* dst; int n_rows, n_out, cols; };

RY_KERNEL(256) void ry_gather_rows(RyGatherRowsParams p) {
    const int lane = (int)threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (j >= p.n_out) return;                                   // wave-uniform
    const int s = p.src_row[j];
    const bool keep = s >= 0 && s < p.n_rows && (p.mask == nullptr || p.mask[s] != 0);      // wave-uniform
    const float* src = p.rows + (size_t)(keep ? s : 0) * p.cols;
    float* row = p.dst + (size_t)j * p.cols;
    int head = (int)((4 - ((reinterpret_cast<unsigned long long>(row) >> 2) & 3)) & 3);     // floats in front of the first 16-byte boundary
    if (head > p.cols) head = p.cols;
    const int quads = (p.cols - head) >> 2, tail = head + 4 * quads;
    const bool wide = (((reinterpret_cast<unsigned long long>(src) ^ reinterpret_cast<unsigned long long>(row)) >> 2) & 3) == 0;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (lane < head) row[lane] = keep ? src[lane] : 0.f;
    for (int q = lane; q < quads; q += 64) {
        const int c = head + 4 * q;
        f32x4 v = zero;
        if (keep) {
            if (wide) v = ry_ld4(src + c);
            else { v[0] = src[c]; v[1] = src[c + 1]; v[2] = src[c + 2]; v[3] = src[c + 3]; }
        }
        ry_st4(row + c, v);
    }
    if (tail + lane < p.cols) row[tail + lane] = keep ? src[tail + lane] : 0.f;             // at most three
}

// ---------------------------------------------------------------------------------------------
// `AcousticConverter.separate_effective` on the device (voice_changer.py:27-31).
// ry_frame_power: mse[t] = librosa.feature.rms(wave, frame_length, hop, center=True, pad_mode='reflect')[t] ** 2 in float32 with
//   NUMPY'S summation order, so that the mask is the host formula's bit for bit: `mean(abs(x) ** 2, axis=0)` of librosa's frame view
//   is numpy's pairwise sum -- leaves of 128 elements, each 8 interleaved accumulators r[j] += a[8 i + j] combined as
//   ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), leaves combined in a binary tree.  One wave per frame: lane (leaf, j) walks its
//   16 elements in order, then a butterfly over the lanes IS that tree (fp addition is commutative, the tree shape is what matters).
//   fft_length = 128 .. 1024, a power of two.  Products and sums are rounded separately (no fma contraction), sqrt is correctly rounded.
//   hop = 1 is the one exception to the order: both axes of the frame view then have the same stride, numpy lays `abs(x) ** 2` out row-major
//   and `mean(axis=0)` adds the fft rows one after the other -- one running sum per frame, which is what the kernel does there
//   (tests/gate_power_cases.py holds both orders to numpy).
// ry_gate_compact: one workgroup: the gate in the POWER domain -- effective = mse >= p_eff, or every frame when max(mse) >= p_all
//   (librosa.power_to_db's top_db clamp) -- with both thresholds derived on the host, once per threshold_db, by bisection over the
//   float32 values through the host's own log10 (realtime_yukarin_amd/gate.py), then an ordered compaction: row_of, the feature rows
//   of the effective frames, the mask and the count.  A NaN power in any of the wave's frames (a NaN sample) leaves NO frame effective:
//   on the host the NaN is log_spec.max(), the clamp makes every entry NaN and every comparison false.  An infinite power is an
//   ordinary maximum (every frame effective).
// ---------------------------------------------------------------------------------------------
struct RyFramePowerParams { const float* wave; int n, hop, fft, n_wave_frames; float* power; };

RY_DEV int ry_reflect_index(int i, int n) {                     // numpy.pad(mode='reflect') source index
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int j = i % period;
    if (j < 0) j += period;
    return j < n ? j : period - j;
}

// the power of frame `frame` of a wave of n samples, by one wave of lanes: the return value is the frame's in every lane below fft / 16
RY_DEV float ry_frame_power_of(const float* wave, int n, int hop, int fft, int frame, int lane) {
    const int L = fft >> 4;                                     // active lanes: 8 per 128-element leaf
    float r = 0.f;
    if (hop == 1) {                                             // wave-uniform: one running sum, the same in every lane (see above)
        const int base = frame - (fft >> 1);
        for (int k = 0; k < fft; ++k) {
            const float v = wave[ry_reflect_index(base + k, n)];
            r = k == 0 ? ry_mul_rn(v, v) : ry_add_rn(r, ry_mul_rn(v, v));
        }
        const float rms1 = ry_sqrt_rn(r / (float)fft);
        return ry_mul_rn(rms1, rms1);
    }
    if (lane < L) {
        const int base = frame * hop - (fft >> 1) + 128 * (lane >> 3) + (lane & 7);
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = wave[ry_reflect_index(base + 8 * i, n)];
        r = ry_mul_rn(v[0], v[0]);
#pragma unroll
        for (int i = 1; i < 16; ++i) r = ry_add_rn(r, ry_mul_rn(v[i], v[i]));
    }
    for (int mask = 1; mask < L; mask <<= 1) r = ry_add_rn(r, ry_shfl_xor(r, mask));
    const float rms = ry_sqrt_rn(r / (float)fft);              // a power of two: the division is exact scaling, as numpy's
    return ry_mul_rn(rms, rms);
}

RY_KERNEL(256) void ry_frame_power(RyFramePowerParams p) {
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int frame = (int)blockIdx.x * 4 + (tid >> 6);
    if (frame >= p.n_wave_frames) return;                       // wave-uniform
    const float pw = ry_frame_power_of(p.wave, p.n, p.hop, p.fft, frame, lane);
    if (lane == 0) p.power[frame] = pw;
}

// The same over a table of waves (ry_vc_enqueue_waves_device): per wave the first sample and the sample count in the call's wave block, the first
// frame and the frame count in the call's feature / mask blocks, the number of wave frames (n_samples / hop + 1) and their first slot in the
// call's power block, and the first row of the wave's region in the call's x_eff / row_of blocks.
struct RyWaveSeg { int s0, n_samples, f0, n_frames, p0, n_wave_frames, r0, pad; };

// One wave of lanes per wave frame over all waves: the frame finds its wave by bisection over p0 and reflects at the ends of that wave only.
struct RyFramePowerManyParams { const float* wave; const RyWaveSeg* seg; int n_waves, hop, fft, total_wave_frames; float* power; };

RY_KERNEL(256) void ry_frame_power_many(RyFramePowerManyParams p) {
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int g = (int)blockIdx.x * 4 + (tid >> 6);
    if (g >= p.total_wave_frames) return;                       // wave-uniform
    int lo = 0, hi = p.n_waves - 1;
    while (lo < hi) {                                           // the last wave whose first slot is at or before g
        const int mid = (lo + hi + 1) >> 1;
        if (p.seg[mid].p0 <= g) lo = mid; else hi = mid - 1;
    }
    const RyWaveSeg s = p.seg[lo];
    const float pw = ry_frame_power_of(p.wave + s.s0, s.n_samples, p.hop, p.fft, g - s.p0, lane);
    if (lane == 0) p.power[g] = pw;
}

struct RyGateParams {
    const float* power; int n_wave_frames, n_frames; float p_eff, p_all;
    const float* feat; int cin;                                // [n_frames][cin]
    float* x_eff; int* row_of; int* count; unsigned char* mask;
};

// the maximum that keeps a NaN (fmaxf drops it): the NaN of any power reaches slot 0 through the same reduction as the maximum
RY_DEV float ry_max_nan(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

RY_DEV void ry_gate_compact_body(const RyGateParams& p) {
    __shared__ float fmx[1024];
    __shared__ int scan[1024];
    __shared__ int s_base;
    const int tid = (int)threadIdx.x;
    float m = 0.f;
    for (int t = tid; t < p.n_wave_frames; t += 1024) m = ry_max_nan(m, p.power[t]);
    fmx[tid] = m;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) { if (tid < s) fmx[tid] = ry_max_nan(fmx[tid], fmx[tid + s]); __syncthreads(); }
    const bool none = fmx[0] != fmx[0];                        // a NaN power anywhere in the wave: the host's clamp makes every entry NaN
    const bool all = !none && fmx[0] >= p.p_all;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int t0 = 0; t0 < p.n_frames; t0 += 1024) {
        const int t = t0 + tid;
        const bool eff = t < p.n_frames && t < p.n_wave_frames && !none && (all || p.power[t] >= p.p_eff);
        scan[tid] = eff ? 1 : 0;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {                    // inclusive Hillis-Steele scan
            const int add = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const int base = s_base;
        if (t < p.n_frames) p.mask[t] = eff ? 1 : 0;
        if (eff) {
            const int pos = base + scan[tid] - 1;
            p.row_of[pos] = t;
            for (int c = 0; c < p.cin; ++c) p.x_eff[(size_t)pos * p.cin + c] = p.feat[(size_t)t * p.cin + c];
        }
        __syncthreads();
        if (tid == 1023) s_base = base + scan[1023];
        __syncthreads();
    }
    if (tid == 0) *p.count = s_base;
}

RY_KERNEL(1024) void ry_gate_compact(RyGateParams p) { ry_gate_compact_body(p); }

// One workgroup per wave of the table: the maximum over the wave's own powers, the ordered compaction into the wave's own region of the call's
// x_eff / row_of blocks (row_of counts from the wave's first frame), the mask bytes in wave order and one count per wave.  `host` is the block the
// host reads with one copy: n_waves counts, then the mask bytes of all waves (each thread copies the bytes it wrote itself).
struct RyGateManyParams {
    const float* power; const RyWaveSeg* seg; float p_eff, p_all;
    const float* feat; int cin;
    float* x_eff; int* row_of; unsigned char* mask; int* host; int n_waves;
};

RY_KERNEL(1024) void ry_gate_compact_many(RyGateManyParams p) {
    const RyWaveSeg s = p.seg[blockIdx.x];
    RyGateParams g;
    g.power = p.power + s.p0; g.n_wave_frames = s.n_wave_frames; g.n_frames = s.n_frames; g.p_eff = p.p_eff; g.p_all = p.p_all;
    g.feat = p.feat + (size_t)s.f0 * p.cin; g.cin = p.cin;
    g.x_eff = p.x_eff + (size_t)s.r0 * p.cin; g.row_of = p.row_of + s.r0; g.count = p.host + blockIdx.x; g.mask = p.mask + s.f0;
    ry_gate_compact_body(g);
    unsigned char* bytes = reinterpret_cast<unsigned char*>(p.host + p.n_waves) + s.f0;
    for (int t = (int)threadIdx.x; t < s.n_frames; t += 1024) bytes[t] = g.mask[t];
}

// The compaction of ry_gate_compact_many alone, from a verdict that already exists (ry_vc_enqueue_waves_masked_device: the gate ran before the
// feature rows were made): one workgroup per wave of the table reads the wave's mask bytes, 1024 frames a round, and writes row_of and the
// effective rows into the wave's own region of the call's blocks -- ascending frames, so order and bits are the gate's.  The positions come from
// the same inclusive scan over the round in the LDS, no atomics; the rows of a round are then copied by all threads, element by element
// in destination order, so the stores of a wave of lanes are contiguous.  A frame whose mask byte is 0 has no feature row read: a wave without an
// effective frame reads and writes nothing but its mask bytes.
struct RyCompactManyParams { const unsigned char* mask; const RyWaveSeg* seg; const float* feat; int cin; float* x_eff; int* row_of; };

RY_KERNEL(1024) void ry_compact_rows_many(RyCompactManyParams p) {
    __shared__ int scan[1024];
    __shared__ int rows[1024];
    __shared__ int s_base;
    const RyWaveSeg s = p.seg[blockIdx.x];
    const int tid = (int)threadIdx.x, cin = p.cin;
    const unsigned char* mask = p.mask + s.f0;
    const float* feat = p.feat + (size_t)s.f0 * cin;
    float* x_eff = p.x_eff + (size_t)s.r0 * cin;
    int* row_of = p.row_of + s.r0;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int t0 = 0; t0 < s.n_frames; t0 += 1024) {
        const int t = t0 + tid;
        const bool eff = t < s.n_frames && mask[t] != 0;
        scan[tid] = eff ? 1 : 0;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {                    // inclusive Hillis-Steele scan
            const int add = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const int base = s_base, count = scan[1023];
        if (eff) { rows[scan[tid] - 1] = t; row_of[base + scan[tid] - 1] = t; }
        __syncthreads();
        for (int i = tid; i < count * cin; i += 1024) {         // count <= 1024: the product fits
            const int r = i / cin;
            x_eff[(size_t)base * cin + i] = feat[(size_t)rows[r] * cin + (i - r * cin)];
        }
        __syncthreads();
        if (tid == 1023) s_base = base + count;
        __syncthreads();
    }
}

struct RyMc2spParams { const float* mc; const float* mtx; float* sp; int n, m, f; float floor; };

RY_KERNEL(256) void ry_mc2sp(RyMc2spParams p) {                 // sp[n][f] = exp(sum_m mc[n][m] * mtx[m][f]) + floor
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.n * p.f) return;
    const int f = (int)(idx % p.f), n = (int)(idx / p.f);
    const float* row = p.mc + (size_t)n * p.m;
    float z = 0.f;
    for (int m = 0; m < p.m; ++m) z = fmaf(row[m], p.mtx[(size_t)m * p.f + f], z);
    p.sp[idx] = expf(z) + p.floor;
}
