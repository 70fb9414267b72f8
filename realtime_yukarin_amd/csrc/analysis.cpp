// analysis.cpp -- the WORLD analysis of libry355.so that feeds the networks (`pyworld.cheaptrick` + `pysptk.sp2mc` in the reference's
// AcousticFeature.extract, reached from Vocoder.encode): wave + f0 track -> spectral envelope rows and mel-cepstrum rows.  Kernels:
// analysis_kernels.h.  Stateless per frame: a call uploads the wave, f0 and the frame times, launches one workgroup per frame and copies
// back what was asked for; the float32 rows go to a device buffer of the caller (world_synth.DeviceRows, stage 2) and never leave the card.
#include "analysis_kernels.h"
#include "ry_host.h"

#include <algorithm>

struct ry_analysis {
    ry_ctx* ctx = nullptr;
    int fs = 0, order = 0;
    double alpha = 0, q1 = 0, floor_f0 = 0;
    unsigned seed_hash = 0;
    Arena tables;
    sy_c* tw = nullptr;
    double* S = nullptr;                     // [513][order + 1]
    Arena scratch;
    double* d_x = nullptr; long long cap_x = 0;
    double* d_f0 = nullptr; long long cap_f0 = 0;
    double* d_t = nullptr; long long cap_t = 0;
    double* d_sp = nullptr; long long cap_sp = 0;
    double* d_mc = nullptr; long long cap_mc = 0;
    AnalysisFrameInts* d_ints = nullptr; long long cap_ints = 0;
    bool record = false;                              // ry_analysis_debug_record: keep the decisions of a run (tests; off the product path)
    std::vector<AnalysisFrameInts> last_ints;         // ry_analysis_debug_ints: the decisions of the last recorded run
};

namespace {
template <typename T>
int alloc_as(Arena& a, T** p, size_t n) {
    float* q = nullptr;
    RY_TRY(a.alloc(&q, (n * sizeof(T) + sizeof(float) - 1) / sizeof(float)));
    *p = (T*)q;
    return RY_OK;
}

template <typename T>
int grow(ry_analysis* s, T** p, long long* cap, long long need) {
    if (need <= *cap) return RY_OK;
    RT_TRY(rt::stream_sync(s->ctx->stream));                       // work in flight may use the old buffer
    if (*p) s->scratch.free_one(*p);
    *p = nullptr; *cap = 0;
    const long long n = need + need / 2 + 64;
    RY_TRY(alloc_as(s->scratch, p, (size_t)n));
    *cap = n;
    return RY_OK;
}

// freqt is linear in the cepstrum: S[i] = freqt(unit vector i), the SPTK recursion in long double, rounded once
void freqt_matrix(int order, double alpha, std::vector<double>* S) {
    const int M = order + 1;
    const long double a = alpha, beta = 1.0L - a * a;
    S->assign((size_t)SYNTH_BINS * M, 0.0);
    std::vector<long double> g(M), d(M);
    for (int u = 0; u < SYNTH_BINS; ++u) {
        std::fill(g.begin(), g.end(), 0.0L);
        for (int i = u; i >= 0; --i) {                              // the inputs behind u are zero and leave g at zero
            d = g;
            g[0] = (i == u ? 1.0L : 0.0L) + a * d[0];
            if (M > 1) g[1] = beta * d[0] + a * d[1];
            for (int j = 2; j < M; ++j) g[j] = d[j - 1] + a * (d[j] - g[j - 1]);
        }
        for (int j = 0; j < M; ++j) (*S)[(size_t)u * M + j] = (double)g[j];
    }
}

int check_handle(ry_analysis* s) {
    if (!s) return fail(RY_ESTATE, "null analysis handle");
    RT_TRY(rt::set_device(s->ctx->device));
    return RY_OK;
}
}  // namespace

extern "C" {

int ry_analysis_create(ry_ctx* ctx, int fs, int fft_size, int order, double alpha, double q1, double f0_floor, unsigned seed, ry_analysis** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    if (!ctx) return fail(RY_EINVAL, "null context");
    if (fs < 8000 || fs > 48000) return fail(RY_EINVAL, "sampling rate %d", fs);
    if (fft_size != SYNTH_FFT) return fail(RY_EINVAL, "fft_size %d: the transforms are built for %d (CheapTrick's size at 16 and 24 kHz)", fft_size, SYNTH_FFT);
    if (order < 0 || order + 1 > ANALYSIS_MAX_MC) return fail(RY_EINVAL, "order %d: 0 .. %d", order, ANALYSIS_MAX_MC - 1);
    if (!(std::fabs(alpha) < 1.0)) return fail(RY_EINVAL, "alpha %g", alpha);
    if (!std::isfinite(q1) || !std::isfinite(f0_floor)) return fail(RY_EINVAL, "q1 %g / f0_floor %g", q1, f0_floor);
    RT_TRY(rt::set_device(ctx->device));
    std::unique_ptr<ry_analysis> s(new ry_analysis());
    s->ctx = ctx; s->fs = fs; s->order = order; s->alpha = alpha; s->q1 = q1;
    s->floor_f0 = std::max(f0_floor, 3.0 * fs / (fft_size - 3.0));
    unsigned h = seed;                                              // synth_hash32 on the host
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    s->seed_hash = h;
    std::vector<double> tw(2 * SYNTH_FFT), S;
    for (int k = 0; k < SYNTH_FFT; ++k) {
        tw[2 * k] = std::cos(SYNTH_TWO_PI * k / SYNTH_FFT);
        tw[2 * k + 1] = std::sin(SYNTH_TWO_PI * k / SYNTH_FFT);
    }
    freqt_matrix(order, alpha, &S);
    RY_TRY(alloc_as(s->tables, &s->tw, (size_t)SYNTH_FFT));
    RY_TRY(alloc_as(s->tables, &s->S, S.size()));
    RT_TRY(rt::h2d(s->tw, tw.data(), tw.size() * sizeof(double), ctx->stream));
    RT_TRY(rt::h2d(s->S, S.data(), S.size() * sizeof(double), ctx->stream));
    RT_TRY(rt::stream_sync(ctx->stream));
    *out = s.release();
    return RY_OK;
}

void ry_analysis_destroy(ry_analysis* s) {
    if (!s) return;
    rt::set_device(s->ctx->device);
    rt::stream_sync(s->ctx->stream);
    delete s;
}

int ry_analysis_run(ry_analysis* s, const double* x, long long x_len, const double* f0, const double* t, int n,
                    double* sp64_out, float* sp32_dev_out, double* mc_out) {
    RY_TRY(check_handle(s));
    if (n < 0) return fail(RY_EINVAL, "n = %d frames", n);
    if (x_len < 0) return fail(RY_EINVAL, "x_len = %lld", x_len);
    if (n > (1 << 22)) return fail(RY_EINVAL, "%d frames in one call", n);
    if (n == 0 || x_len == 0) { s->last_ints.clear(); return RY_OK; }      // nothing to analyse: nothing is written
    if (!x) return fail(RY_EINVAL, "null wave");
    if (!f0 || !t) return fail(RY_EINVAL, "null f0 / t");
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(f0[i]) || !(f0[i] < 0.5 * s->fs)) return fail(RY_EINVAL, "f0[%d] = %g: finite and below fs / 2", i, f0[i]);
        if (!std::isfinite(t[i]) || std::fabs(t[i]) > 1e9) return fail(RY_EINVAL, "t[%d] = %g", i, t[i]);
    }
    const ry_stream_t st = s->ctx->stream;
    RY_TRY(grow(s, &s->d_x, &s->cap_x, x_len));
    RY_TRY(grow(s, &s->d_f0, &s->cap_f0, (long long)n));
    RY_TRY(grow(s, &s->d_t, &s->cap_t, (long long)n));
    if (s->record) RY_TRY(grow(s, &s->d_ints, &s->cap_ints, (long long)n));
    if (sp64_out) RY_TRY(grow(s, &s->d_sp, &s->cap_sp, (long long)n * SYNTH_BINS));
    if (mc_out) RY_TRY(grow(s, &s->d_mc, &s->cap_mc, (long long)n * (s->order + 1)));
    RT_TRY(rt::h2d(s->d_x, x, (size_t)x_len * sizeof(double), st));
    RT_TRY(rt::h2d(s->d_f0, f0, (size_t)n * sizeof(double), st));
    RT_TRY(rt::h2d(s->d_t, t, (size_t)n * sizeof(double), st));
    AnalysisParams p;
    p.x = s->d_x; p.x_len = x_len; p.f0 = s->d_f0; p.t = s->d_t;
    p.fs = (double)s->fs; p.floor_f0 = s->floor_f0; p.q1 = s->q1; p.seed_hash = s->seed_hash;
    p.tw = s->tw; p.S = s->S; p.n_mc = s->order + 1;
    p.sp64 = sp64_out ? s->d_sp : nullptr; p.sp32 = sp32_dev_out; p.mc = mc_out ? s->d_mc : nullptr; p.ints = s->record ? s->d_ints : nullptr;
    RY_LAUNCH(analysis_frame, dim3((unsigned)n), 256, st, p);
    RT_TRY(rt::last_error());
    s->last_ints.resize(s->record ? (size_t)n : 0);
    if (s->record) RT_TRY(rt::d2h(s->last_ints.data(), s->d_ints, (size_t)n * sizeof(AnalysisFrameInts), st));
    if (sp64_out) RT_TRY(rt::d2h(sp64_out, s->d_sp, (size_t)n * SYNTH_BINS * sizeof(double), st));
    if (mc_out) RT_TRY(rt::d2h(mc_out, s->d_mc, (size_t)n * (s->order + 1) * sizeof(double), st));
    RT_TRY(rt::stream_sync(st));                                   // the caller's arrays are free, the float32 rows are written
    return RY_OK;
}

int ry_analysis_sp2mc(ry_analysis* s, const void* sp, int n, int on_device, double* mc_out) {
    RY_TRY(check_handle(s));
    if (n < 0) return fail(RY_EINVAL, "n = %d frames", n);
    if (n > (1 << 22)) return fail(RY_EINVAL, "%d frames in one call", n);
    if (n == 0) return RY_OK;
    if (!sp || !mc_out) return fail(RY_EINVAL, "null sp / mc");
    const ry_stream_t st = s->ctx->stream;
    RY_TRY(grow(s, &s->d_mc, &s->cap_mc, (long long)n * (s->order + 1)));
    AnalysisSp2mcParams p;
    p.sp64 = nullptr; p.sp32 = nullptr;
    if (on_device) p.sp32 = (const float*)sp;
    else {
        RY_TRY(grow(s, &s->d_sp, &s->cap_sp, (long long)n * SYNTH_BINS));
        RT_TRY(rt::h2d(s->d_sp, sp, (size_t)n * SYNTH_BINS * sizeof(double), st));
        p.sp64 = s->d_sp;
    }
    p.tw = s->tw; p.S = s->S; p.n_mc = s->order + 1; p.mc = s->d_mc;
    RY_LAUNCH(analysis_sp2mc, dim3((unsigned)n), 256, st, p);
    RT_TRY(rt::last_error());
    RT_TRY(rt::d2h(mc_out, s->d_mc, (size_t)n * (s->order + 1) * sizeof(double), st));
    RT_TRY(rt::stream_sync(st));
    return RY_OK;
}

int ry_analysis_debug_record(ry_analysis* s, int on) {
    if (!s) return fail(RY_ESTATE, "null analysis handle");
    s->record = on != 0;
    if (!s->record) s->last_ints.clear();
    return RY_OK;
}

int ry_analysis_debug_ints(ry_analysis* s, long long* out, int capacity, int* n) {
    if (!s || !n) return fail(RY_EINVAL, "bad argument");
    *n = (int)s->last_ints.size();
    if (!out) return RY_OK;                                        // the count alone
    if (capacity < *n) return fail(RY_EINVAL, "%d frames, room for %d", *n, capacity);
    for (int i = 0; i < *n; ++i) {
        out[4 * i] = s->last_ints[i].h; out[4 * i + 1] = s->last_ints[i].centre;
        out[4 * i + 2] = s->last_ints[i].L; out[4 * i + 3] = s->last_ints[i].b;
    }
    return RY_OK;
}

int ry_analysis_debug_poison(ry_analysis* s) {
    RY_TRY(check_handle(s));
    const ry_stream_t st = s->ctx->stream;
    RT_TRY(rt::stream_sync(st));
    // every buffer a call grows: all bits set (NaN as a double, -1 as an integer)
    if (s->d_x) RT_TRY(rt::dmemset(s->d_x, 0xff, (size_t)s->cap_x * sizeof(double), st));
    if (s->d_f0) RT_TRY(rt::dmemset(s->d_f0, 0xff, (size_t)s->cap_f0 * sizeof(double), st));
    if (s->d_t) RT_TRY(rt::dmemset(s->d_t, 0xff, (size_t)s->cap_t * sizeof(double), st));
    if (s->d_sp) RT_TRY(rt::dmemset(s->d_sp, 0xff, (size_t)s->cap_sp * sizeof(double), st));
    if (s->d_mc) RT_TRY(rt::dmemset(s->d_mc, 0xff, (size_t)s->cap_mc * sizeof(double), st));
    if (s->d_ints) RT_TRY(rt::dmemset(s->d_ints, 0xff, (size_t)s->cap_ints * sizeof(AnalysisFrameInts), st));
    RT_TRY(rt::stream_sync(st));
    return RY_OK;
}

}  // extern "C"
