// analysis.cpp -- the WORLD analysis of libry355.so that feeds the networks (`pyworld.cheaptrick` + `pysptk.sp2mc` in the reference's
// AcousticFeature.extract, reached from Vocoder.encode): wave + f0 track -> spectral envelope rows and mel-cepstrum rows.  Kernels:
// analysis_kernels.h.  Stateless per frame: a call uploads the wave, f0 and the frame times, launches one workgroup per frame and copies
// back what was asked for; the float32 rows go to a device buffer of the caller (world_synth.DeviceRows, stage 2) and never leave the card.
// D4C (`pyworld.d4c` + `pyworld.code_aperiodicity`: ap and coded_ap; kernel: d4c_kernels.h) runs over the same uploaded wave.
// ry_analysis_extract_dev takes the wave (float32) and the track from device memory instead -- what ry_crepe_track left there: the wave is widened
// on the card, the track is checked by a kernel whose verdict the host reads before it launches the same frame kernels.
// ry_analysis_extract_many_dev does that for the waves and tracks of ry_crepe_track_many: one widening, one check and one verdict for the call, then
// the frame kernels once per wave on that wave's samples and rows (a frame kernel takes one wave: its clamp at both ends is that wave's).
// ry_analysis_upload_waves / ry_analysis_ingest_tracks put the waves and an f0 track of the caller's own (WORLD mode: a host tracker) into buffers
// of this handle, in the layout those device entries read; no CREPE handle is involved.
#include "analysis_kernels.h"
#include "d4c_kernels.h"
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
    DevBufList scratch;                               // every buffer a call grows
    DevBuf<double> d_x{scratch}, d_f0{scratch}, d_t{scratch}, d_sp{scratch}, d_mc{scratch};
    DevBuf<AnalysisFrameInts> d_ints{scratch};
    bool record = false;                              // ry_analysis_debug_record: keep the decisions of a run (tests; off the product path)
    std::vector<AnalysisFrameInts> last_ints;         // ry_analysis_debug_ints: the decisions of the last recorded run
    // D4C: built for the rates whose transform sizes are 2048 and whose band centres are bins of the row (16 and 24 kHz); d4c_why says why not
    bool d4c_ok = false;
    std::string d4c_why;
    int n_bands = 0, band_half = 0, band_centre[D4C_MAX_BANDS] = {0, 0, 0}, lt[3] = {0, 0, 0};
    sy_c* tw2 = nullptr;                              // [1025]
    double* nuttall = nullptr;                        // [2 band_half + 1]
    DevBuf<double> d_ap{scratch}, d_coded{scratch};
    DevBuf<D4cFrameRecord> d_rec{scratch};
    DevBuf<int> d_verdict{scratch};                   // ry_analysis_extract_dev: (first refused frame or -1, kind) of the track check
    std::vector<D4cFrameRecord> last_rec;             // ry_analysis_debug_d4c: a0, on / off, integers and coarse values of the last recorded run
    // a caller's own track (WORLD mode: f0 from a host tracker).  ry_analysis_upload_waves: the float32 waves back to back and where each starts
    // (waves + 1 entries; empty: none).  ry_analysis_ingest_tracks: its one upload (f0, then the segment table) lands in d_ingest, the kernel leaves
    // f0 / t / voiced of the tracks back to back; trk_off: where each starts (tracks + 1 entries; empty: no track).  ry_analysis_track_buffers reports
    // both; the extract calls read them in place.  No other call writes these buffers; ry_analysis_debug_poison forgets waves and track.
    DevBuf<float> d_wave32{scratch};
    DevBuf<double> d_ingest{scratch}, d_trk_f0{scratch}, d_trk_t{scratch};
    DevBuf<unsigned char> d_trk_voiced{scratch};
    std::vector<double> ingest_host;                  // the handle's copy of the upload: it outlives the call
    std::vector<long long> up_off;
    std::vector<int> trk_off;
};

namespace {
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

int pow2_above(double v) { return 1 << (1 + (int)std::floor(std::log2(v))); }

// sizes, bands and tables of D4C at this rate; rates it is not built for leave d4c_ok false and the reason in d4c_why
int d4c_setup(ry_analysis* s) {
    const int fs = s->fs;
    char why[160];
    const int n = pow2_above(4.0 * fs / D4C_FLOOR_F0 + 1.0), n_lt = pow2_above(3.0 * fs / D4C_LOVE_TRAIN_FLOOR + 1.0);
    const int bands = (int)std::floor(std::min(15000.0, fs / 2.0 - 3000.0) / 3000.0);
    if (n != D4C_FFT || n_lt != D4C_FFT || bands < 1 || bands > D4C_MAX_BANDS || (3000ll * SYNTH_FFT) % fs != 0) {
        std::snprintf(why, sizeof why, "D4C at %d Hz needs transforms of %d / %d points and %d bands: built for 2048 / 2048 points, 1 .. %d bands "
                      "whose centres are bins of the row (16 and 24 kHz)", fs, n, n_lt, bands, D4C_MAX_BANDS);
        s->d4c_why = why;
        return RY_OK;
    }
    s->n_bands = bands;
    s->band_half = (int)(3000ll * D4C_FFT / fs);
    for (int i = 0; i < bands; ++i) s->band_centre[i] = (int)(3000ll * (i + 1) * D4C_FFT / fs);
    if (s->band_centre[0] - s->band_half < 0 || s->band_centre[bands - 1] + s->band_half > D4C_HALF || 2 * s->band_half + 1 > D4C_MAX_NUTTALL)
        return fail(RY_ESTATE, "D4C band table at %d Hz", fs);
    const long long hz[3] = {100, 4000, 7900};
    for (int i = 0; i < 3; ++i) s->lt[i] = (int)((hz[i] * D4C_FFT + fs - 1) / fs);
    const std::vector<double> tw2 = twiddles(D4C_FFT, D4C_BINS);
    std::vector<double> nut((size_t)2 * s->band_half + 1);
    for (size_t i = 0; i < nut.size(); ++i) {
        const double tmp = (double)i / (double)(nut.size() - 1);
        nut[i] = 0.355768 - 0.487396 * std::cos(SYNTH_TWO_PI * tmp) + 0.144232 * std::cos(2.0 * SYNTH_TWO_PI * tmp) - 0.012604 * std::cos(3.0 * SYNTH_TWO_PI * tmp);
    }
    RY_TRY(upload_table(s->tables, s->ctx, (const sy_c*)tw2.data(), (size_t)D4C_BINS, &s->tw2));
    RY_TRY(upload_table(s->tables, s->ctx, nut.data(), nut.size(), &s->nuttall));
    s->d4c_ok = true;
    return RY_OK;
}

struct Outputs {
    double* sp64 = nullptr; float* sp32_dev = nullptr; double* mc = nullptr;
    bool d4c = false; double threshold = 0.85;
    double* ap64 = nullptr; float* ap32_dev = nullptr; double* coded = nullptr;
    float* mc32_dev = nullptr;               // ry_analysis_extract_resident: the float32 mel-cepstrum rows, left on the card
};

// what every entry refuses before it looks at the wave or the track; *empty: nothing to analyse, nothing is written
int check_call(ry_analysis* s, long long x_len, int n, bool cheaptrick, const Outputs& o, bool* empty) {
    RY_TRY(check_handle(s, "analysis"));
    if (n < 0) return fail(RY_EINVAL, "n = %d frames", n);
    if (x_len < 0) return fail(RY_EINVAL, "x_len = %lld", x_len);
    if (n > (1 << 22)) return fail(RY_EINVAL, "%d frames in one call", n);
    if (o.d4c && !s->d4c_ok) return fail(RY_EINVAL, "%s", s->d4c_why.c_str());
    if (o.d4c && !std::isfinite(o.threshold)) return fail(RY_EINVAL, "threshold %g", o.threshold);
    *empty = n == 0 || x_len == 0;
    if (*empty) {
        if (cheaptrick) s->last_ints.clear();
        if (o.d4c) s->last_rec.clear();
    }
    return RY_OK;
}

// frames [k0, k0 + n) of a call analyse the wave of x_len samples at x0 of the call's wave buffer; their float32 device rows (sp32 / mc32 / ap32) are
// rows [r0, r0 + n) of the caller's blocks (r0 = k0 unless the caller says where the rows of a wave go: ry_analysis_extract_spans_resident)
struct Span { long long x0, x_len; int k0, n, r0; };

int run_spans(ry_analysis* s, const double* d_x, const Span* spans, int n_spans, const double* d_f0, const double* d_t, int n, bool cheaptrick, const Outputs& o);

int run_kernels(ry_analysis* s, const double* d_x, long long x_len, const double* d_f0, const double* d_t, int n, bool cheaptrick, const Outputs& o) {
    const Span one = {0, x_len, 0, n, 0};
    return run_spans(s, d_x, &one, 1, d_f0, d_t, n, cheaptrick, o);
}

// one upload of the wave and the track, then CheapTrick + sp2mc (when `cheaptrick`) and / or D4C (when o.d4c) over it
int run_frames(ry_analysis* s, const double* x, long long x_len, const double* f0, const double* t, int n, bool cheaptrick, const Outputs& o) {
    bool empty = false;
    RY_TRY(check_call(s, x_len, n, cheaptrick, o, &empty));
    if (empty) return RY_OK;
    if (!x) return fail(RY_EINVAL, "null wave");
    if (!f0 || !t) return fail(RY_EINVAL, "null f0 / t");
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(f0[i]) || !(f0[i] < 0.5 * s->fs)) return fail(RY_EINVAL, "f0[%d] = %g: finite and below fs / 2", i, f0[i]);
        if (!(t[i] >= -1.0 && t[i] <= 1e6)) return fail(RY_EINVAL, "t[%d] = %g: -1 .. 1e6 s", i, t[i]);
    }
    const ry_stream_t st = s->ctx->stream;
    RY_TRY(s->d_x.grow(s->ctx, x_len));
    RY_TRY(s->d_f0.grow(s->ctx, (long long)n));
    RY_TRY(s->d_t.grow(s->ctx, (long long)n));
    RT_TRY(rt::h2d(s->d_x.ptr(), x, (size_t)x_len * sizeof(double), st));
    RT_TRY(rt::h2d(s->d_f0.ptr(), f0, (size_t)n * sizeof(double), st));
    RT_TRY(rt::h2d(s->d_t.ptr(), t, (size_t)n * sizeof(double), st));
    return run_kernels(s, s->d_x.ptr(), x_len, s->d_f0.ptr(), s->d_t.ptr(), n, cheaptrick, o);
}

// the frame kernels over the waves and the track of n frames in device memory, one launch per wave, and the copies of what was asked for
int run_spans(ry_analysis* s, const double* d_x, const Span* spans, int n_spans, const double* d_f0, const double* d_t, int n, bool cheaptrick, const Outputs& o) {
    const ry_stream_t st = s->ctx->stream;
    if (cheaptrick) {
        if (s->record) RY_TRY(s->d_ints.grow(s->ctx, (long long)n));
        if (o.sp64) RY_TRY(s->d_sp.grow(s->ctx, (long long)n * SYNTH_BINS));
        if (o.mc) RY_TRY(s->d_mc.grow(s->ctx, (long long)n * (s->order + 1)));
    }
    if (o.d4c) {
        if (s->record) RY_TRY(s->d_rec.grow(s->ctx, (long long)n));
        if (o.ap64) RY_TRY(s->d_ap.grow(s->ctx, (long long)n * SYNTH_BINS));
        if (o.coded) RY_TRY(s->d_coded.grow(s->ctx, (long long)n * s->n_bands));
    }
    const size_t n_mc = (size_t)s->order + 1;
    for (int i = 0; i < n_spans && cheaptrick; ++i) {
        const Span& sp = spans[i];
        const size_t k0 = (size_t)sp.k0, r0 = (size_t)sp.r0;
        AnalysisParams p;
        p.x = d_x + sp.x0; p.x_len = sp.x_len; p.f0 = d_f0 + k0; p.t = d_t + k0;
        p.fs = (double)s->fs; p.floor_f0 = s->floor_f0; p.q1 = s->q1; p.seed_hash = s->seed_hash;
        p.tw = s->tw; p.S = s->S; p.n_mc = s->order + 1;
        p.sp64 = o.sp64 ? s->d_sp.ptr() + k0 * SYNTH_BINS : nullptr; p.sp32 = o.sp32_dev ? o.sp32_dev + r0 * SYNTH_BINS : nullptr;
        p.mc = o.mc ? s->d_mc.ptr() + k0 * n_mc : nullptr; p.ints = s->record ? s->d_ints.ptr() + k0 : nullptr;
        p.mc32 = o.mc32_dev ? o.mc32_dev + r0 * n_mc : nullptr;
        RY_LAUNCH(analysis_frame, dim3((unsigned)sp.n), 256, st, p);
        RT_TRY(rt::last_error());
    }
    for (int i = 0; i < n_spans && o.d4c; ++i) {
        const Span& sp = spans[i];
        const size_t k0 = (size_t)sp.k0, r0 = (size_t)sp.r0;
        D4cParams p;
        p.x = d_x + sp.x0; p.x_len = sp.x_len; p.f0 = d_f0 + k0; p.t = d_t + k0;
        p.fs = (double)s->fs; p.threshold = o.threshold; p.seed_hash = s->seed_hash;
        p.tw = s->tw; p.tw2 = s->tw2; p.nuttall = s->nuttall;
        p.n_bands = s->n_bands; p.band_half = s->band_half;
        for (int i = 0; i < D4C_MAX_BANDS; ++i) p.band_centre[i] = s->band_centre[i];
        p.lt0 = s->lt[0]; p.lt1 = s->lt[1]; p.lt2 = s->lt[2];
        p.ap64 = o.ap64 ? s->d_ap.ptr() + k0 * SYNTH_BINS : nullptr; p.ap32 = o.ap32_dev ? o.ap32_dev + r0 * SYNTH_BINS : nullptr;
        p.coded = o.coded ? s->d_coded.ptr() + k0 * (size_t)s->n_bands : nullptr; p.rec = s->record ? s->d_rec.ptr() + k0 : nullptr;
        RY_LAUNCH(d4c_frame, dim3((unsigned)sp.n), 256, st, p);
        RT_TRY(rt::last_error());
    }
    if (cheaptrick) {
        s->last_ints.resize(s->record ? (size_t)n : 0);
        if (s->record) RT_TRY(rt::d2h(s->last_ints.data(), s->d_ints.ptr(), (size_t)n * sizeof(AnalysisFrameInts), st));
        if (o.sp64) RT_TRY(rt::d2h(o.sp64, s->d_sp.ptr(), (size_t)n * SYNTH_BINS * sizeof(double), st));
        if (o.mc) RT_TRY(rt::d2h(o.mc, s->d_mc.ptr(), (size_t)n * (s->order + 1) * sizeof(double), st));
    }
    if (o.d4c) {
        s->last_rec.resize(s->record ? (size_t)n : 0);
        if (s->record) RT_TRY(rt::d2h(s->last_rec.data(), s->d_rec.ptr(), (size_t)n * sizeof(D4cFrameRecord), st));
        if (o.ap64) RT_TRY(rt::d2h(o.ap64, s->d_ap.ptr(), (size_t)n * SYNTH_BINS * sizeof(double), st));
        if (o.coded) RT_TRY(rt::d2h(o.coded, s->d_coded.ptr(), (size_t)n * s->n_bands * sizeof(double), st));
    }
    RT_TRY(rt::stream_sync(st));                                   // the caller's arrays are free, the float32 rows are written
    return RY_OK;
}

// a float32 wave buffer of x_len samples and a track of n frames on the card: widened and checked once -- ONE verdict, read before any frame kernel --
// then the frame kernels per span
int extract_dev(ry_analysis* s, const float* x32_dev, long long x_len, const double* f0_dev, const double* t_dev, int n, const Span* spans, int n_spans,
                const Outputs& o) {
    const ry_stream_t st = s->ctx->stream;
    RY_TRY(s->d_x.grow(s->ctx, x_len));
    RY_TRY(s->d_verdict.reserve(s->ctx, 2));
    AnalysisCheckParams cp;
    cp.f0 = f0_dev; cp.t = t_dev; cp.n = n; cp.fs = (double)s->fs; cp.verdict = s->d_verdict.ptr();
    RY_LAUNCH(analysis_check_track, dim3(1), 256, st, cp);
    RT_TRY(rt::last_error());
    int verdict[2] = {0, 0};
    RT_TRY(rt::d2h(verdict, s->d_verdict.ptr(), sizeof verdict, st));
    AnalysisWidenParams wp;
    wp.x32 = x32_dev; wp.x64 = s->d_x.ptr(); wp.n = x_len;
    RY_LAUNCH(analysis_widen, dim3((unsigned)((x_len + 255) / 256)), 256, st, wp);       // behind the copy: it runs while the host waits for the verdict
    RT_TRY(rt::last_error());
    RT_TRY(rt::stream_sync(st));
    if (verdict[0] >= 0 && verdict[0] < n) {                            // the refusal's values, for the message
        double v[2] = {0.0, 0.0};
        RT_TRY(rt::d2h(&v[0], f0_dev + verdict[0], sizeof(double), st));
        RT_TRY(rt::d2h(&v[1], t_dev + verdict[0], sizeof(double), st));
        RT_TRY(rt::stream_sync(st));
        if (verdict[1] == 1) return fail(RY_EINVAL, "f0[%d] = %g: finite and below fs / 2", verdict[0], v[0]);
        return fail(RY_EINVAL, "t[%d] = %g: -1 .. 1e6 s", verdict[0], v[1]);
    }
    if (verdict[0] != -1) return fail(RY_ESTATE, "the track check left %d", verdict[0]);
    return run_spans(s, s->d_x.ptr(), spans, n_spans, f0_dev, t_dev, n, true, o);
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
    if (!(std::fabs(alpha) <= 0.9)) return fail(RY_EINVAL, "alpha %g: -0.9 .. 0.9", alpha);
    if (!(q1 >= -0.4 && q1 <= 0.0)) return fail(RY_EINVAL, "q1 %g: -0.4 .. 0", q1);
    if (!(f0_floor >= 1.0 && f0_floor <= 1000.0)) return fail(RY_EINVAL, "f0_floor %g: 1 .. 1000 Hz", f0_floor);
    RT_TRY(rt::set_device(ctx->device));
    std::unique_ptr<ry_analysis> s(new ry_analysis());
    s->ctx = ctx; s->fs = fs; s->order = order; s->alpha = alpha; s->q1 = q1;
    s->floor_f0 = std::max(f0_floor, 3.0 * fs / (fft_size - 3.0));
    s->seed_hash = synth_hash32(seed);
    const std::vector<double> tw = twiddles(SYNTH_FFT);
    std::vector<double> S;
    freqt_matrix(order, alpha, &S);
    RY_TRY(upload_table(s->tables, ctx, (const sy_c*)tw.data(), (size_t)SYNTH_FFT, &s->tw));
    RY_TRY(upload_table(s->tables, ctx, S.data(), S.size(), &s->S));
    RY_TRY(d4c_setup(s.get()));
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
    Outputs o;
    o.sp64 = sp64_out; o.sp32_dev = sp32_dev_out; o.mc = mc_out;
    return run_frames(s, x, x_len, f0, t, n, true, o);
}

int ry_analysis_d4c(ry_analysis* s, const double* x, long long x_len, const double* f0, const double* t, int n, double threshold,
                    double* ap64_out, float* ap32_dev_out, double* coded_out) {
    Outputs o;
    o.d4c = true; o.threshold = threshold; o.ap64 = ap64_out; o.ap32_dev = ap32_dev_out; o.coded = coded_out;
    return run_frames(s, x, x_len, f0, t, n, false, o);
}

int ry_analysis_extract(ry_analysis* s, const double* x, long long x_len, const double* f0, const double* t, int n, double threshold,
                        double* sp64_out, float* sp32_dev_out, double* mc_out, double* ap64_out, float* ap32_dev_out, double* coded_out) {
    Outputs o;
    o.sp64 = sp64_out; o.sp32_dev = sp32_dev_out; o.mc = mc_out;
    o.d4c = true; o.threshold = threshold; o.ap64 = ap64_out; o.ap32_dev = ap32_dev_out; o.coded = coded_out;
    return run_frames(s, x, x_len, f0, t, n, true, o);
}

int ry_analysis_extract_dev(ry_analysis* s, const float* x32_dev, long long x_len, const double* f0_dev, const double* t_dev, int n, double threshold,
                            double* sp64_out, float* sp32_dev_out, double* mc_out, double* ap64_out, float* ap32_dev_out, double* coded_out) {
    Outputs o;
    o.sp64 = sp64_out; o.sp32_dev = sp32_dev_out; o.mc = mc_out;
    o.d4c = true; o.threshold = threshold; o.ap64 = ap64_out; o.ap32_dev = ap32_dev_out; o.coded = coded_out;
    bool empty = false;
    RY_TRY(check_call(s, x_len, n, true, o, &empty));
    if (empty) return RY_OK;
    if (!x32_dev) return fail(RY_EINVAL, "null wave");
    if (!f0_dev || !t_dev) return fail(RY_EINVAL, "null f0 / t");
    const Span one = {0, x_len, 0, n, 0};
    return extract_dev(s, x32_dev, x_len, f0_dev, t_dev, n, &one, 1, o);
}

int ry_analysis_extract_resident(ry_analysis* s, const float* x32_dev, long long x_len, const double* f0_dev, const double* t_dev, int n, double threshold,
                                 float* mc32_dev_out, float* sp32_dev_out, float* ap32_dev_out) {
    Outputs o;
    o.mc32_dev = mc32_dev_out; o.sp32_dev = sp32_dev_out; o.ap32_dev = ap32_dev_out;
    o.d4c = true; o.threshold = threshold;
    bool empty = false;
    RY_TRY(check_call(s, x_len, n, true, o, &empty));
    if (!mc32_dev_out || !sp32_dev_out || !ap32_dev_out) return fail(RY_EINVAL, "null output rows");
    if (empty) return RY_OK;
    if (!x32_dev) return fail(RY_EINVAL, "null wave");
    if (!f0_dev || !t_dev) return fail(RY_EINVAL, "null f0 / t");
    const Span one = {0, x_len, 0, n, 0};
    return extract_dev(s, x32_dev, x_len, f0_dev, t_dev, n, &one, 1, o);       // no host row is named: the verdict is the only copy to the host
}

}  // extern "C"

namespace {
// the waves and tracks ry_crepe_track_many left on the card: the spans of the offsets, one check of the whole track, the frame kernels per wave
int extract_many(ry_analysis* s, const float* x32_dev, const long long* sample_offsets, const double* f0_dev, const double* t_dev,
                 const int* frame_offsets, int n_waves, const Outputs& o, bool device_rows_only) {
    RY_TRY(check_handle(s, "analysis"));
    if (n_waves < 1) return fail(RY_EINVAL, "%d waves", n_waves);
    if (!sample_offsets || !frame_offsets) return fail(RY_EINVAL, "null offsets");
    if (sample_offsets[0] != 0 || frame_offsets[0] != 0) return fail(RY_EINVAL, "the offsets start at %lld / %d, not at 0", sample_offsets[0], frame_offsets[0]);
    std::vector<Span> spans((size_t)n_waves);
    for (int i = 0; i < n_waves; ++i) {
        Span& sp = spans[(size_t)i];
        sp.x0 = sample_offsets[i]; sp.x_len = sample_offsets[i + 1] - sample_offsets[i];
        sp.k0 = frame_offsets[i]; sp.n = frame_offsets[i + 1] - frame_offsets[i]; sp.r0 = sp.k0;
        if (sp.x_len < 1) return fail(RY_EINVAL, "wave %d has %lld samples", i, sp.x_len);
        if (sp.n < 1) return fail(RY_EINVAL, "wave %d has %d frames", i, sp.n);
        if (frame_offsets[i + 1] > (1 << 22)) return fail(RY_EINVAL, "%d frames in one call", frame_offsets[i + 1]);
    }
    const long long x_len = sample_offsets[n_waves];
    const int n = frame_offsets[n_waves];
    bool empty = false;
    RY_TRY(check_call(s, x_len, n, true, o, &empty));                   // never empty: every wave has a sample and a frame
    if (device_rows_only && (!o.mc32_dev || !o.sp32_dev || !o.ap32_dev)) return fail(RY_EINVAL, "null output rows");
    if (!x32_dev) return fail(RY_EINVAL, "null wave");
    if (!f0_dev || !t_dev) return fail(RY_EINVAL, "null f0 / t");
    return extract_dev(s, x32_dev, x_len, f0_dev, t_dev, n, spans.data(), n_waves, o);
}
}  // namespace

extern "C" {

int ry_analysis_extract_many_dev(ry_analysis* s, const float* x32_dev, const long long* sample_offsets, const double* f0_dev, const double* t_dev,
                                 const int* frame_offsets, int n_waves, double threshold,
                                 double* sp64_out, float* sp32_dev_out, double* mc_out, double* ap64_out, float* ap32_dev_out, double* coded_out) {
    Outputs o;
    o.sp64 = sp64_out; o.sp32_dev = sp32_dev_out; o.mc = mc_out;
    o.d4c = true; o.threshold = threshold; o.ap64 = ap64_out; o.ap32_dev = ap32_dev_out; o.coded = coded_out;
    return extract_many(s, x32_dev, sample_offsets, f0_dev, t_dev, frame_offsets, n_waves, o, false);
}

int ry_analysis_extract_many_resident(ry_analysis* s, const float* x32_dev, const long long* sample_offsets, const double* f0_dev, const double* t_dev,
                                      const int* frame_offsets, int n_waves, double threshold,
                                      float* mc32_dev_out, float* sp32_dev_out, float* ap32_dev_out) {
    Outputs o;
    o.mc32_dev = mc32_dev_out; o.sp32_dev = sp32_dev_out; o.ap32_dev = ap32_dev_out;
    o.d4c = true; o.threshold = threshold;
    return extract_many(s, x32_dev, sample_offsets, f0_dev, t_dev, frame_offsets, n_waves, o, true);      // no host row is named: one verdict comes back
}

// ry_analysis_extract_many_resident for waves that lie anywhere in an uploaded block and rows that go anywhere in the caller's blocks: wave i has the
// samples [first_sample[i], first_sample[i] + n_samples[i]) of x32_dev (x_len samples in all), the frames [frame_offsets[i], frame_offsets[i + 1]) of
// f0_dev / t_dev (the tracks back to back, as a tracker left them) and writes the rows [row_offsets[i], row_offsets[i] + its frames) of the three
// blocks.  The waves ascend without overlap, and so do the row ranges: nothing outside them is written.
int ry_analysis_extract_spans_resident(ry_analysis* s, const float* x32_dev, long long x_len, const long long* first_sample, const int* n_samples,
                                       const double* f0_dev, const double* t_dev, const int* frame_offsets, const int* row_offsets, int n_waves,
                                       double threshold, float* mc32_dev_out, float* sp32_dev_out, float* ap32_dev_out) {
    Outputs o;
    o.mc32_dev = mc32_dev_out; o.sp32_dev = sp32_dev_out; o.ap32_dev = ap32_dev_out;
    o.d4c = true; o.threshold = threshold;
    RY_TRY(check_handle(s, "analysis"));
    if (n_waves < 1) return fail(RY_EINVAL, "%d waves", n_waves);
    if (!first_sample || !n_samples || !frame_offsets || !row_offsets) return fail(RY_EINVAL, "null tables");
    if (frame_offsets[0] != 0) return fail(RY_EINVAL, "the frame offsets start at %d, not at 0", frame_offsets[0]);
    std::vector<Span> spans((size_t)n_waves);
    long long x_end = 0, r_end = 0;
    for (int i = 0; i < n_waves; ++i) {
        Span& sp = spans[(size_t)i];
        sp.x0 = first_sample[i]; sp.x_len = n_samples[i];
        sp.k0 = frame_offsets[i]; sp.n = frame_offsets[i + 1] - frame_offsets[i]; sp.r0 = row_offsets[i];
        if (sp.x_len < 1) return fail(RY_EINVAL, "wave %d has %lld samples", i, sp.x_len);
        if (sp.n < 1) return fail(RY_EINVAL, "wave %d has %d frames", i, sp.n);
        if (sp.x0 < x_end || sp.x0 + sp.x_len > x_len) return fail(RY_EINVAL, "wave %d: samples %lld .. %lld of %lld: the table must ascend inside the block", i, sp.x0, sp.x0 + sp.x_len, x_len);
        if (sp.r0 < r_end || (long long)sp.r0 + sp.n > (1 << 22)) return fail(RY_EINVAL, "wave %d: rows %d .. %lld: the table must ascend, at most 2^22 rows", i, sp.r0, (long long)sp.r0 + sp.n);
        if (frame_offsets[i + 1] > (1 << 22)) return fail(RY_EINVAL, "%d frames in one call", frame_offsets[i + 1]);
        x_end = sp.x0 + sp.x_len; r_end = (long long)sp.r0 + sp.n;
    }
    const int n = frame_offsets[n_waves];
    bool empty = false;
    RY_TRY(check_call(s, x_len, n, true, o, &empty));                   // never empty: every wave has a sample and a frame
    if (!mc32_dev_out || !sp32_dev_out || !ap32_dev_out) return fail(RY_EINVAL, "null output rows");
    if (!x32_dev) return fail(RY_EINVAL, "null wave");
    if (!f0_dev || !t_dev) return fail(RY_EINVAL, "null f0 / t");
    return extract_dev(s, x32_dev, x_len, f0_dev, t_dev, n, spans.data(), n_waves, o);
}

// ---- a caller's own track: the waves and the f0 of a host tracker put on the card for the extract calls above.  Every refusal comes before anything
// is uploaded or changed, so a refused call leaves the waves and the track of the last good call in place.
int ry_analysis_upload_waves(ry_analysis* s, const float* audio, const int* n_samples, int n_waves, const float** wave_dev) {
    RY_TRY(check_handle(s, "analysis"));
    if (!audio || !n_samples || !wave_dev) return fail(RY_EINVAL, "null audio / n_samples / wave_dev");
    if (n_waves < 1) return fail(RY_EINVAL, "%d waves", n_waves);
    std::vector<long long> off((size_t)n_waves + 1, 0);
    for (int i = 0; i < n_waves; ++i) {
        if (n_samples[i] < 1) return fail(RY_EINVAL, "wave %d has %d samples", i, n_samples[i]);
        off[(size_t)i + 1] = off[(size_t)i] + n_samples[i];
        if (off[(size_t)i + 1] > 2147483647LL) return fail(RY_EINVAL, "the waves up to %d hold %lld samples: too many for one call", i, off[(size_t)i + 1]);
    }
    const ry_stream_t st = s->ctx->stream;
    s->up_off.clear();                                                  // from here on the old block may be gone
    RY_TRY(s->d_wave32.grow(s->ctx, off.back()));
    RT_TRY(rt::h2d(s->d_wave32.ptr(), audio, (size_t)off.back() * sizeof(float), st));      // the one upload
    RT_TRY(rt::stream_sync(st));                                        // the caller's array is free
    s->up_off.swap(off);
    *wave_dev = s->d_wave32.ptr();
    return RY_OK;
}

int ry_analysis_ingest_tracks(ry_analysis* s, const double* f0, const int* n_frames, int n_waves, double frame_period_ms) {
    RY_TRY(check_handle(s, "analysis"));
    if (!f0 || !n_frames) return fail(RY_EINVAL, "null f0 / n_frames");
    if (n_waves < 1) return fail(RY_EINVAL, "%d waves", n_waves);
    if (!std::isfinite(frame_period_ms) || !(frame_period_ms > 0.0)) return fail(RY_EINVAL, "frame period %g ms: finite and positive", frame_period_ms);
    std::vector<int> off((size_t)n_waves + 1, 0);
    for (int i = 0; i < n_waves; ++i) {
        if (n_frames[i] < 1) return fail(RY_EINVAL, "wave %d has %d frames", i, n_frames[i]);
        const long long end = (long long)off[(size_t)i] + n_frames[i];
        if (end > (1 << 22)) return fail(RY_EINVAL, "%lld frames in one call", end);
        off[(size_t)i + 1] = (int)end;
    }
    const int n = off.back();
    const ry_stream_t st = s->ctx->stream;
    s->trk_off.clear();                                                 // from here on the old track may be gone
    static_assert(sizeof(AnalysisIngestSeg) == sizeof(double), "a segment takes one slot of the upload");
    const size_t slots = (size_t)n + (size_t)n_waves;                   // f0 [n], then the segment table [n_waves]
    RY_TRY(s->d_ingest.grow(s->ctx, (long long)slots));
    RY_TRY(s->d_trk_f0.grow(s->ctx, (long long)n));
    RY_TRY(s->d_trk_t.grow(s->ctx, (long long)n));
    RY_TRY(s->d_trk_voiced.grow(s->ctx, ((long long)n + 3) / 4 * 4));   // whole 32-bit words: ry_dev_download copies those
    s->ingest_host.resize(slots);
    std::memcpy(s->ingest_host.data(), f0, (size_t)n * sizeof(double));
    for (int i = 0; i < n_waves; ++i) {
        const AnalysisIngestSeg seg = {off[(size_t)i], n_frames[i]};
        std::memcpy(s->ingest_host.data() + n + i, &seg, sizeof seg);
    }
    RT_TRY(rt::h2d(s->d_ingest.ptr(), s->ingest_host.data(), slots * sizeof(double), st));          // the one upload
    AnalysisIngestParams p;
    p.f0_in = s->d_ingest.ptr(); p.segs = reinterpret_cast<const AnalysisIngestSeg*>(s->d_ingest.ptr() + n); p.n_segs = n_waves; p.n = n;
    p.frame_period = frame_period_ms;
    p.f0_64 = s->d_trk_f0.ptr(); p.t_64 = s->d_trk_t.ptr(); p.voiced = s->d_trk_voiced.ptr();
    RY_LAUNCH(analysis_ingest_tracks, dim3((unsigned)((n + 255) / 256)), 256, st, p);
    RT_TRY(rt::last_error());
    RT_TRY(rt::stream_sync(st));                                        // the handle's copy of the upload is free for the next call
    s->trk_off.swap(off);
    return RY_OK;
}

int ry_analysis_track_buffers(ry_analysis* s, const float** wave_dev, int* n_waves, const long long** sample_offsets, int* n_tracks,
                              const int** frame_offsets, const unsigned char** voiced_dev, const double** f0_dev, const double** t_dev) {
    if (!s) return fail(RY_ESTATE, "null analysis handle");
    if (s->trk_off.empty()) return fail(RY_ESTATE, "no track on the card: ry_analysis_ingest_tracks has not run, or the buffers were poisoned");
    const bool up = !s->up_off.empty();
    if (wave_dev) *wave_dev = up ? s->d_wave32.ptr() : nullptr;
    if (n_waves) *n_waves = up ? (int)s->up_off.size() - 1 : 0;
    if (sample_offsets) *sample_offsets = up ? s->up_off.data() : nullptr;
    if (n_tracks) *n_tracks = (int)s->trk_off.size() - 1;
    if (frame_offsets) *frame_offsets = s->trk_off.data();
    if (voiced_dev) *voiced_dev = s->d_trk_voiced.ptr();
    if (f0_dev) *f0_dev = s->d_trk_f0.ptr();
    if (t_dev) *t_dev = s->d_trk_t.ptr();
    return RY_OK;
}

int ry_analysis_d4c_bands(ry_analysis* s) {
    if (!s) return fail(RY_ESTATE, "null analysis handle");
    if (!s->d4c_ok) return fail(RY_EINVAL, "%s", s->d4c_why.c_str());
    return s->n_bands;
}

int ry_analysis_sp2mc(ry_analysis* s, const void* sp, int n, int on_device, double* mc_out) {
    RY_TRY(check_handle(s, "analysis"));
    if (n < 0) return fail(RY_EINVAL, "n = %d frames", n);
    if (n > (1 << 22)) return fail(RY_EINVAL, "%d frames in one call", n);
    if (n == 0) return RY_OK;
    if (!sp || !mc_out) return fail(RY_EINVAL, "null sp / mc");
    const ry_stream_t st = s->ctx->stream;
    RY_TRY(s->d_mc.grow(s->ctx, (long long)n * (s->order + 1)));
    AnalysisSp2mcParams p;
    p.sp64 = nullptr; p.sp32 = nullptr;
    if (on_device) p.sp32 = (const float*)sp;
    else {
        RY_TRY(s->d_sp.grow(s->ctx, (long long)n * SYNTH_BINS));
        RT_TRY(rt::h2d(s->d_sp.ptr(), sp, (size_t)n * SYNTH_BINS * sizeof(double), st));
        p.sp64 = s->d_sp.ptr();
    }
    p.tw = s->tw; p.S = s->S; p.n_mc = s->order + 1; p.mc = s->d_mc.ptr();
    RY_LAUNCH(analysis_sp2mc, dim3((unsigned)n), 256, st, p);
    RT_TRY(rt::last_error());
    RT_TRY(rt::d2h(mc_out, s->d_mc.ptr(), (size_t)n * (s->order + 1) * sizeof(double), st));
    RT_TRY(rt::stream_sync(st));
    return RY_OK;
}

int ry_analysis_debug_record(ry_analysis* s, int on) {
    if (!s) return fail(RY_ESTATE, "null analysis handle");
    s->record = on != 0;
    if (!s->record) { s->last_ints.clear(); s->last_rec.clear(); }
    return RY_OK;
}

int ry_analysis_debug_d4c(ry_analysis* s, long long* ints_out, double* values_out, int capacity, int* n) {
    if (!s || !n) return fail(RY_EINVAL, "bad argument");
    *n = (int)s->last_rec.size();
    if (!ints_out && !values_out) return RY_OK;                    // the count alone
    if (capacity < *n) return fail(RY_EINVAL, "%d frames, room for %d", *n, capacity);
    for (int i = 0; i < *n; ++i) {
        const D4cFrameRecord& r = s->last_rec[i];
        if (ints_out) {
            const long long v[9] = {r.v.h3, r.v.h4, r.v.om, r.v.oc, r.v.op, r.v.L, r.v.b1, r.v.b2, r.on};
            for (int j = 0; j < 9; ++j) ints_out[9 * i + j] = v[j];
        }
        if (values_out) {
            values_out[4 * i] = r.a0;
            for (int j = 0; j < D4C_MAX_BANDS; ++j) values_out[4 * i + 1 + j] = r.coarse[j];
        }
    }
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
    RY_TRY(check_handle(s, "analysis"));
    const ry_stream_t st = s->ctx->stream;
    RT_TRY(rt::stream_sync(st));
    for (DevBufBase* b : s->scratch) RY_TRY(b->poison(st));            // all bits set: NaN as a double, -1 as an integer
    RT_TRY(rt::stream_sync(st));
    s->up_off.clear(); s->trk_off.clear();                              // the uploaded waves and the ingested track are gone with their buffers
    return RY_OK;
}

}  // extern "C"
