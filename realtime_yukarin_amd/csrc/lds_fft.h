// lds_fft.h -- what the float64 LDS kernels of synth_kernels.h (WORLD synthesis) and analysis_kernels.h (WORLD analysis) share: the 1024-point
// radix-4 Stockham transform of one workgroup of 256 threads and the counter-based noise.  One definition, two translation units.
#pragma once
#include "ry_dev.h"

#ifdef RY_HOST_EMU
#include <cmath>
#endif

#define SYNTH_FFT 1024
#define SYNTH_HALF 512
#define SYNTH_BINS 513
#define SYNTH_TWO_PI 6.283185307179586476925286766559

// ---------------------------------------------------------------------------------------------
// 1024-point complex transform in the LDS, float64: radix-4 Stockham (autosort), passes with Ns = 1, 4, 16, 64, 256; thread j does the
// butterfly of inputs j + 256 r.  sign = -1: forward (e^{-i...}), +1: backward; both unnormalised.  The result of the five passes is in `b`.
// tw[k] = (cos, sin)(2 pi k / 1024), host-computed.  Reads of a pass are unit-stride over the threads; the writes of the first passes are
// strided (Ns < 16): a 4-way bank conflict on two of the five passes, left as it is -- the kernel is far from being the bottleneck of a push.
// ---------------------------------------------------------------------------------------------
struct sy_c { double x, y; };
RY_DEV sy_c sy_add(sy_c a, sy_c b) { sy_c r = {a.x + b.x, a.y + b.y}; return r; }
RY_DEV sy_c sy_sub(sy_c a, sy_c b) { sy_c r = {a.x - b.x, a.y - b.y}; return r; }
RY_DEV sy_c sy_mul(sy_c a, sy_c b) { sy_c r = {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; return r; }

RY_DEV void synth_fft(sy_c* a, sy_c* b, const sy_c* tw, double sign) {
    const int j = (int)threadIdx.x;
    sy_c* src = a;
    sy_c* dst = b;
    for (int ns = 1; ns < SYNTH_FFT; ns *= 4) {
        const int k = j & (ns - 1);
        const int step = 256 / ns;                               // twiddle index of e^{2 pi i k / (4 ns)} in the 1024 table
        sy_c v0 = src[j], v1 = src[j + 256], v2 = src[j + 512], v3 = src[j + 768];
        if (ns > 1) {
            sy_c w1 = tw[k * step], w2 = tw[2 * k * step], w3 = tw[3 * k * step];
            w1.y *= sign; w2.y *= sign; w3.y *= sign;
            v1 = sy_mul(v1, w1); v2 = sy_mul(v2, w2); v3 = sy_mul(v3, w3);
        }
        const sy_c t0 = sy_add(v0, v2), t1 = sy_sub(v0, v2), t2 = sy_add(v1, v3), d = sy_sub(v1, v3);
        const sy_c t3 = {-sign * d.y, sign * d.x};               // sign * i * (v1 - v3)
        const int j0 = ((j - k) << 2) + k;
        dst[j0] = sy_add(t0, t2);
        dst[j0 + ns] = sy_add(t1, t3);
        dst[j0 + 2 * ns] = sy_sub(t0, t2);
        dst[j0 + 3 * ns] = sy_sub(t1, t3);
        __syncthreads();
        sy_c* t = src; src = dst; dst = t;
    }
}

// counter-based noise: sample k of seed's noise = (sum of twelve 24-bit uniforms) 2^-24 - 6, the uniforms from lowbias32 over (seed, 12 k + j)
RY_HOST_DEV unsigned synth_hash32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
RY_DEV double synth_noise(unsigned seed_hash, unsigned long long k) {
    unsigned total = 0;
    for (int j = 0; j < 12; ++j) {
        const unsigned long long key = k * 12ull + (unsigned long long)j;
        total += synth_hash32((unsigned)(key & 0xffffffffull) ^ synth_hash32((unsigned)(key >> 32) ^ seed_hash)) >> 8;
    }
    return (double)total * (1.0 / 16777216.0) - 6.0;
}
