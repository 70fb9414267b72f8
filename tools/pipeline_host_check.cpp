// pipeline_host_check.cpp -- the host paths of the resident wave-to-wave chain (ry_analysis_extract_resident, ry_vc_enqueue_wave_device, ry_mask_rows)
// in a stand-alone program over the emulator build of libry355, meant to be compiled and linked with -fsanitize=address,undefined
// (scripts/asan_pipeline.sh): every argument check, the offset arithmetic of the launchers (row ranges and row starts at every alignment, the
// blocks of the caller, the gate's buffers growing from a short window to a longer one, a discard hint) and destroy after device-pointer windows.
// SYN-8 predictors, a handful of frames per call.  Exit status 0: every call returned what it should, and the device-pointer window equals the
// host-array window on the same inputs.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ry355.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, ry_last_error()); ++failures; } } while (0)

static std::vector<float> tone(int n, int seed) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 0.4f * std::sin(0.08f * (float)(i + 13 * seed)) * (float)(i + 1) / (float)n;
    return x;
}

static float* on_card(ry_ctx* ctx, const void* host, size_t n_floats) {
    float* p = nullptr;
    EXPECT(ry_dev_alloc(ctx, n_floats, &p) == 0);
    if (host) EXPECT(ry_dev_upload(ctx, p, (const float*)host, n_floats) == 0);
    return p;
}

static void check_mask_rows(ry_ctx* ctx) {
    const int colses[4] = {513, 4, 1, 6};
    for (int cols : colses) {
        const int n = 11;
        std::vector<float> rows((size_t)(n + 2) * cols, 1.5f), got(rows.size());
        unsigned char mask[16] = {0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0};
        float* d = on_card(ctx, rows.data(), rows.size());
        float* m = on_card(ctx, mask, 4);
        const int ranges[4][2] = {{0, n}, {3, 3}, {2, n - 1}, {n - 1, n}};
        for (const int* r : ranges) {
            EXPECT(ry_dev_upload(ctx, d, rows.data(), rows.size()) == 0);
            EXPECT(ry_mask_rows(ctx, d + cols, (const unsigned char*)m, n, cols, r[0], r[1], nullptr) == 0);       // a guard row on either side
            EXPECT(ry_sync(ctx) == 0);
            EXPECT(ry_dev_download(ctx, got.data(), d, got.size()) == 0);
            for (int k = -1; k <= n; ++k) {
                const bool zero = k >= r[0] && k < r[1] && mask[k] == 0;
                for (int c = 0; c < cols; ++c) EXPECT(got[(size_t)(k + 1) * cols + c] == (zero ? 0.0f : 1.5f));
            }
        }
        EXPECT(ry_mask_rows(nullptr, d, (const unsigned char*)m, n, cols, 0, n, nullptr) == -1);
        EXPECT(ry_mask_rows(ctx, nullptr, (const unsigned char*)m, n, cols, 0, n, nullptr) == -1);
        EXPECT(ry_mask_rows(ctx, d, nullptr, n, cols, 0, n, nullptr) == -1);
        EXPECT(ry_mask_rows(ctx, d, (const unsigned char*)m, 0, cols, 0, 0, nullptr) == -1);
        EXPECT(ry_mask_rows(ctx, d, (const unsigned char*)m, n, 0, 0, n, nullptr) == -1);
        EXPECT(ry_mask_rows(ctx, d, (const unsigned char*)m, n, cols, -1, n, nullptr) == -1);
        EXPECT(ry_mask_rows(ctx, d, (const unsigned char*)m, n, cols, 5, 4, nullptr) == -1);
        EXPECT(ry_mask_rows(ctx, d, (const unsigned char*)m, n, cols, 0, n + 1, nullptr) == -1);
        EXPECT(ry_dev_free(ctx, d) == 0);
        EXPECT(ry_dev_free(ctx, m) == 0);
    }
}

static void check_extract_resident(ry_ctx* ctx) {
    const int fs = 16000, n = 6, x_len = 420;
    ry_analysis* an = nullptr;
    EXPECT(ry_analysis_create(ctx, fs, 1024, 8, 0.41, -0.15, 71.0, 5, &an) == 0);
    std::vector<float> x = tone(x_len, 3);
    double f0[n] = {0.0, 120.0, 180.0, 0.0, 400.0, 95.0}, t[n], f0_bad[n];
    for (int i = 0; i < n; ++i) { t[i] = 0.005 * i; f0_bad[i] = f0[i]; }
    f0_bad[4] = fs / 2.0;
    float* dx = on_card(ctx, x.data(), (size_t)x_len);
    float* df = on_card(ctx, f0, 2 * n);
    float* dfb = on_card(ctx, f0_bad, 2 * n);
    float* dt = on_card(ctx, t, 2 * n);
    std::vector<float> nan_rows((size_t)n * 513);
    std::memset(nan_rows.data(), 0xff, nan_rows.size() * sizeof(float));
    float* mc = on_card(ctx, nan_rows.data(), (size_t)n * 9);
    float* sp = on_card(ctx, nan_rows.data(), nan_rows.size());
    float* ap = on_card(ctx, nan_rows.data(), nan_rows.size());
    const double *f = (const double*)df, *fb = (const double*)dfb, *tt = (const double*)dt;
    // refusals: nothing is written
    EXPECT(ry_analysis_extract_resident(nullptr, dx, x_len, f, tt, n, 0.85, mc, sp, ap) == -4);
    EXPECT(ry_analysis_extract_resident(an, dx, x_len, f, tt, n, 0.85, nullptr, sp, ap) == -1);
    EXPECT(ry_analysis_extract_resident(an, dx, x_len, f, tt, n, 0.85, mc, nullptr, ap) == -1);
    EXPECT(ry_analysis_extract_resident(an, dx, x_len, f, tt, n, 0.85, mc, sp, nullptr) == -1);
    EXPECT(ry_analysis_extract_resident(an, nullptr, x_len, f, tt, n, 0.85, mc, sp, ap) == -1);
    EXPECT(ry_analysis_extract_resident(an, dx, x_len, nullptr, tt, n, 0.85, mc, sp, ap) == -1);
    EXPECT(ry_analysis_extract_resident(an, dx, x_len, f, nullptr, n, 0.85, mc, sp, ap) == -1);
    EXPECT(ry_analysis_extract_resident(an, dx, -1, f, tt, n, 0.85, mc, sp, ap) == -1);
    EXPECT(ry_analysis_extract_resident(an, dx, x_len, f, tt, -1, 0.85, mc, sp, ap) == -1);
    EXPECT(ry_analysis_extract_resident(an, dx, x_len, f, tt, (1 << 22) + 1, 0.85, mc, sp, ap) == -1);
    EXPECT(ry_analysis_extract_resident(an, dx, x_len, fb, tt, n, 0.85, mc, sp, ap) == -1);
    EXPECT(ry_analysis_extract_resident(an, dx, x_len, f, tt, 0, 0.85, mc, sp, ap) == 0);            // no frames: nothing to do
    std::vector<float> got((size_t)n * 513);
    EXPECT(ry_dev_download(ctx, got.data(), sp, got.size()) == 0);
    EXPECT(std::memcmp(got.data(), nan_rows.data(), got.size() * sizeof(float)) == 0);
    EXPECT(ry_dev_download(ctx, got.data(), mc, (size_t)n * 9) == 0);
    EXPECT(std::memcmp(got.data(), nan_rows.data(), (size_t)n * 9 * sizeof(float)) == 0);
    // the call, against the float64 rows of ry_analysis_extract_dev
    EXPECT(ry_analysis_extract_resident(an, dx, x_len, f, tt, n, 0.85, mc, sp, ap) == 0);
    std::vector<double> sp64((size_t)n * 513), mc64((size_t)n * 9), ap64((size_t)n * 513), coded((size_t)n);
    EXPECT(ry_analysis_extract_dev(an, dx, x_len, f, tt, n, 0.85, sp64.data(), nullptr, mc64.data(), ap64.data(), nullptr, coded.data()) == 0);
    EXPECT(ry_dev_download(ctx, got.data(), mc, (size_t)n * 9) == 0);
    for (int i = 0; i < n * 9; ++i) EXPECT(got[(size_t)i] == (float)mc64[(size_t)i]);
    EXPECT(ry_dev_download(ctx, got.data(), sp, got.size()) == 0);
    for (int i = 0; i < n * 513; ++i) EXPECT(got[(size_t)i] == (float)sp64[(size_t)i]);
    EXPECT(ry_dev_download(ctx, got.data(), ap, got.size()) == 0);
    for (int i = 0; i < n * 513; ++i) EXPECT(got[(size_t)i] == (float)ap64[(size_t)i]);
    for (float* p : {dx, df, dfb, dt, mc, sp, ap}) EXPECT(ry_dev_free(ctx, p) == 0);
    ry_analysis_destroy(an);
}

static ry_net* make_net(ry_ctx* ctx, int ndim) {
    ry_net_desc d;
    std::memset(&d, 0, sizeof d);
    d.ndim = ndim; d.in_ch = ndim == 1 ? 9 : 1; d.out_ch = ndim == 1 ? 9 : 1; d.base = 8; d.extensive_layers = 8; d.width = ndim == 1 ? 1 : 512;
    d.bn_eps = 2e-5f; d.lrelu_slope = 0.2f; d.glu = 0;
    const size_t np = ry_net_param_count(&d);
    std::vector<float> w(np);
    for (size_t i = 0; i < np; ++i) w[i] = 0.004f + 0.02f * std::fabs(std::sin(0.37f * (float)i));     // variances stay positive
    ry_net* net = nullptr;
    EXPECT(ry_net_create(ctx, &d, w.data(), np, 0, &net) == 0);
    return net;
}

static void check_enqueue_wave_device(ry_ctx* ctx) {
    ry_net *s1 = make_net(ctx, 1), *s2 = make_net(ctx, 2);
    std::vector<float> mtx((size_t)9 * 513);
    for (size_t i = 0; i < mtx.size(); ++i) mtx[i] = 0.01f * std::cos(0.011f * (float)i);
    ry_vc* vc = nullptr;
    EXPECT(ry_vc_create(s1, s2, mtx.data(), 9, 513, &vc) == 0);
    EXPECT(ry_vc_set_lanes(vc, 2) == 0);
    const int hop = 80, n_max = 9;
    const float p_eff = 4e-3f, p_all = 3e38f;
    std::vector<float> wave = tone(n_max * hop, 1), feat((size_t)n_max * 9);
    for (size_t i = 0; i < feat.size(); ++i) feat[i] = 0.3f * std::sin(0.7f * (float)i);
    float* dw = on_card(ctx, wave.data(), wave.size());
    float* df = on_card(ctx, feat.data(), feat.size());
    float* dmc = on_card(ctx, nullptr, (size_t)n_max * 9);
    float* dsp = on_card(ctx, nullptr, (size_t)n_max * 513);
    float* dmask = on_card(ctx, nullptr, 4);
    unsigned char* dm = (unsigned char*)dmask;
    unsigned char eff[16], eff_h[16];
    int n_eff = -1, n_eff_h = -1, ticket = -1;
    // a short window, a longer one (the slot's buffers and the power buffer grow), the short one again on the next slot; against the host-array call
    const int frames[3] = {5, n_max, 5};
    for (int n : frames) {
        const int n_samples = n * hop;
        std::vector<float> mc((size_t)n * 9), sp((size_t)n * 513), mc_h(mc.size()), sp_h(sp.size());
        EXPECT(ry_vc_enqueue_wave_device(vc, dw, n_samples, hop, 1024, p_eff, p_all, df, n, 1e-16f, dmc, dsp, dm, eff, &n_eff) == 0);
        EXPECT(ry_sync(ctx) == 0);
        EXPECT(ry_dev_download(ctx, mc.data(), dmc, mc.size()) == 0);
        EXPECT(ry_dev_download(ctx, sp.data(), dsp, sp.size()) == 0);
        EXPECT(ry_vc_submit_wave(vc, wave.data(), n_samples, hop, 1024, p_eff, p_all, feat.data(), n, 1e-16f, &ticket) == 0);
        EXPECT(ry_vc_wait_wave(vc, ticket, mc_h.data(), sp_h.data(), eff_h, &n_eff_h) == 0);
        EXPECT(n_eff == n_eff_h && n_eff >= 0 && n_eff <= n);
        EXPECT(std::memcmp(eff, eff_h, (size_t)n) == 0);
        EXPECT(std::memcmp(mc.data(), mc_h.data(), mc.size() * sizeof(float)) == 0);
        EXPECT(std::memcmp(sp.data(), sp_h.data(), sp.size() * sizeof(float)) == 0);
    }
    // a discard hint: the kept rows only
    EXPECT(ry_vc_set_discard(vc, 2, 1) == 0);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, n_max * hop, hop, 1024, p_eff, p_all, df, n_max, 1e-16f, dmc, dsp, dm, eff, &n_eff) == 0);
    EXPECT(ry_mask_rows(ctx, dsp, dm, n_max, 513, 2, n_max - 1, ry_stream(ctx)) == 0);       // behind the window, on the context stream
    EXPECT(ry_sync(ctx) == 0);
    EXPECT(ry_vc_set_discard(vc, 0, 0) == 0);
    // all silent: stage 1 is skipped
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 5 * hop, hop, 1024, 3e38f, p_all, df, 5, 1e-16f, dmc, dsp, dm, eff, &n_eff) == 0);
    EXPECT(n_eff == 0 && eff[0] == 0 && eff[4] == 0);
    EXPECT(ry_sync(ctx) == 0);
    // refusals
    EXPECT(ry_vc_enqueue_wave_device(nullptr, dw, 400, hop, 1024, p_eff, p_all, df, 5, 1e-16f, dmc, dsp, dm, eff, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, nullptr, 400, hop, 1024, p_eff, p_all, df, 5, 1e-16f, dmc, dsp, dm, eff, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 400, hop, 1024, p_eff, p_all, nullptr, 5, 1e-16f, dmc, dsp, dm, eff, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 400, hop, 1024, p_eff, p_all, df, 5, 1e-16f, nullptr, dsp, dm, eff, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 400, hop, 1024, p_eff, p_all, df, 5, 1e-16f, dmc, nullptr, dm, eff, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 400, hop, 1024, p_eff, p_all, df, 5, 1e-16f, dmc, dsp, nullptr, eff, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 400, hop, 1024, p_eff, p_all, df, 5, 1e-16f, dmc, dsp, dm, nullptr, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 400, hop, 1024, p_eff, p_all, df, 5, 1e-16f, dmc, dsp, dm, eff, nullptr) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 0, hop, 1024, p_eff, p_all, df, 5, 1e-16f, dmc, dsp, dm, eff, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 400, 0, 1024, p_eff, p_all, df, 5, 1e-16f, dmc, dsp, dm, eff, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 400, hop, 1000, p_eff, p_all, df, 5, 1e-16f, dmc, dsp, dm, eff, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 400, hop, 2048, p_eff, p_all, df, 5, 1e-16f, dmc, dsp, dm, eff, &n_eff) == -1);
    EXPECT(ry_vc_enqueue_wave_device(vc, dw, 400, hop, 1024, p_eff, p_all, df, 0, 1e-16f, dmc, dsp, dm, eff, &n_eff) == -1);
    for (float* p : {dw, df, dmc, dsp, dmask}) EXPECT(ry_dev_free(ctx, p) == 0);
    ry_vc_destroy(vc);
    ry_net_destroy(s1);
    ry_net_destroy(s2);
}

int main() {
    ry_ctx* ctx = nullptr;
    EXPECT(ry_init(0, &ctx) == 0);
    check_mask_rows(ctx);
    check_extract_resident(ctx);
    check_enqueue_wave_device(ctx);
    ry_shutdown(ctx);
    std::printf(failures ? "pipeline_host_check: %d FAILED\n" : "pipeline_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
