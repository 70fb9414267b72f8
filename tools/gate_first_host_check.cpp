// gate_first_host_check.cpp -- the host paths of the gate-first form (ry_crepe_upload_waves, ry_crepe_track_uploaded, ry_crepe_bank_track_uploaded,
// ry_crepe_uploaded_buffers, ry_vc_gate_verdict_waves_device, ry_vc_compact_waves_device, ry_vc_enqueue_waves_masked_device,
// ry_analysis_extract_spans_resident) in a stand-alone program over the emulator build of libry355, meant to be compiled and linked with
// -fsanitize=address,undefined (scripts/asan_gate_first.sh): the table of uploaded waves and the search in it, the split of upload and track (a subset
// against ry_crepe_track_many on those waves alone, two subsets of one table, a small table after a larger one and back, the handle's own frame
// offsets), the masks walked under the caller's offsets, the span and row-offset arithmetic of the analysis, every refusal, the whole chain once, and
// destroy after each.  Smallest capacity, SYN-8 predictors, a handful of frames per call, 16 kHz.  Exit status 0: every call returned what it should.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ry355.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, ry_last_error()); ++failures; } } while (0)

static std::vector<float> tone(int n, int seed) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 0.4f * std::sin(0.08f * (float)(i + 13 * seed)) + 0.01f * (float)((i * 7 + seed) % 11);
    return x;
}

static float* on_card(ry_ctx* ctx, const void* host, size_t n_floats) {
    float* p = nullptr;
    EXPECT(ry_dev_alloc(ctx, n_floats, &p) == 0);
    if (host) EXPECT(ry_dev_upload(ctx, p, (const float*)host, n_floats) == 0);
    return p;
}

static ry_crepe* make_crepe(ry_ctx* ctx) {
    const size_t np = ry_crepe_param_count(1);
    std::vector<float> w(np);
    for (size_t i = 0; i < np; ++i) w[i] = 0.05f * std::sin(0.37f * (float)i) + (i % 5 == 4 ? 1.0f : 0.0f);      // variances stay positive
    ry_crepe* c = nullptr;
    EXPECT(ry_crepe_create(ctx, 1, w.data(), np, 1.0f, &c) == 0);
    return c;
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

// ---- the upload, the subset tracks and their refusals
static void check_tracker(ry_ctx* ctx) {
    ry_crepe *a = make_crepe(ctx), *b = make_crepe(ctx);
    const int large_n[3] = {320, 160, 240}, small_n[2] = {80, 1};
    std::vector<float> xl = tone(720, 2), xs = tone(81, 1);
    const float* wave = nullptr;
    long long total = 0;
    int nt = -1, nf[3] = {0, 0, 0}, nf2[2] = {0, 0};
    const int* fo = nullptr;
    const unsigned char* vd = nullptr;
    const double *fd = nullptr, *td = nullptr;
    EXPECT(ry_crepe_uploaded_buffers(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);
    EXPECT(ry_crepe_uploaded_buffers(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);
    const int first02[2] = {0, 480}, n02[2] = {320, 240}, first1[1] = {320}, n1[1] = {160};
    EXPECT(ry_crepe_track_uploaded(a, first02, n02, 2, 16000, 80, 5.0, 0.1, nf, nullptr, nullptr, nullptr, 1) == -4);      // no table yet
    // the refusals of the upload leave no table
    EXPECT(ry_crepe_upload_waves(nullptr, xl.data(), large_n, 3, 16000, &wave) == -4);
    EXPECT(ry_crepe_upload_waves(a, nullptr, large_n, 3, 16000, &wave) == -1);
    EXPECT(ry_crepe_upload_waves(a, xl.data(), nullptr, 3, 16000, &wave) == -1);
    EXPECT(ry_crepe_upload_waves(a, xl.data(), large_n, 3, 16000, nullptr) == -1);
    EXPECT(ry_crepe_upload_waves(a, xl.data(), large_n, 0, 16000, &wave) == -1);
    const int none[3] = {320, 0, 240}, huge[3] = {1 << 30, 1 << 30, 8};
    EXPECT(ry_crepe_upload_waves(a, xl.data(), none, 3, 16000, &wave) == -1);
    EXPECT(ry_crepe_upload_waves(a, xl.data(), huge, 3, 16000, &wave) == -1);              // refused from the counts: the audio is not read
    EXPECT(ry_crepe_upload_waves(a, xl.data(), large_n, 3, 24000, &wave) == -4);            // no resampler tables
    EXPECT(ry_crepe_uploaded_buffers(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);
    // a small table, a larger one (the buffers grow), the small one again; every time a subset against ry_crepe_track_many on those waves alone
    unsigned char v[64], vw[64];
    double f[64], t[64], fw[64], tw[64];
    for (int round = 0; round < 3; ++round) {
        const bool large = round == 1;
        EXPECT(ry_crepe_upload_waves(a, large ? xl.data() : xs.data(), large ? large_n : small_n, large ? 3 : 2, 16000, &wave) == 0);
        EXPECT(wave != nullptr);
        EXPECT(ry_crepe_uploaded_buffers(a, nullptr, &total, &nt, &fo, nullptr, nullptr, nullptr) == 0);
        EXPECT(total == (large ? 720 : 81) && nt == 0 && fo == nullptr);
        if (large) {
            EXPECT(ry_crepe_track_uploaded(a, first02, n02, 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == 0);
            std::vector<float> two(xl.begin(), xl.begin() + 320);
            two.insert(two.end(), xl.begin() + 480, xl.end());
            EXPECT(ry_crepe_track_many(b, two.data(), n02, 2, 16000, 80, 5.0, 0.1, nf2, vw, fw, tw, 0) == 0);
            const int n = nf[0] + nf[1];
            EXPECT(nf[0] == nf2[0] && nf[1] == nf2[1] && n == 9 && n <= 64);
            EXPECT(std::memcmp(v, vw, (size_t)n) == 0 && std::memcmp(f, fw, (size_t)n * sizeof(double)) == 0 && std::memcmp(t, tw, (size_t)n * sizeof(double)) == 0);
            EXPECT(ry_crepe_uploaded_buffers(a, &wave, &total, &nt, &fo, &vd, &fd, &td) == 0);
            EXPECT(nt == 2 && fo && fo[0] == 0 && fo[1] == nf[0] && fo[2] == n && vd && fd && td);
            EXPECT(ry_crepe_track_many_buffers(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);    // not a back-to-back track
            // a second subset of the same table, on the card
            EXPECT(ry_crepe_track_uploaded(a, first1, n1, 1, 16000, 80, 5.0, 0.1, nf, nullptr, nullptr, nullptr, 1) == 0);
            EXPECT(ry_crepe_uploaded_buffers(a, nullptr, nullptr, &nt, &fo, nullptr, nullptr, nullptr) == 0 && nt == 1 && fo[1] == nf[0] && nf[0] == 3);
        } else {
            const int first[2] = {0, 80};
            EXPECT(ry_crepe_track_uploaded(a, first + 1, small_n + 1, 1, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == 0 && nf[0] == 1);     // the last wave: one sample
            EXPECT(ry_crepe_track_uploaded(a, first, small_n, 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == 0 && nf[0] == 2 && nf[1] == 1);
        }
    }
    // refusals of the subset call over the small table (offsets 0, 80, 81): the table stays, nothing is tracked
    const int first[2] = {0, 80};
    const int past[1] = {81}, one[1] = {1}, inside[1] = {40}, forty[1] = {40}, longer[1] = {82}, zero[1] = {0}, neg[1] = {-1};
    const int back[2] = {80, 0}, back_n[2] = {1, 80}, twice[2] = {0, 0}, twice_n[2] = {80, 80};
    EXPECT(ry_crepe_track_uploaded(a, past, one, 1, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);            // behind the table
    EXPECT(ry_crepe_track_uploaded(a, neg, one, 1, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);
    EXPECT(ry_crepe_track_uploaded(a, inside, forty, 1, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);        // inside a wave
    EXPECT(ry_crepe_track_uploaded(a, zero, longer, 1, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);         // longer than the table
    EXPECT(ry_crepe_track_uploaded(a, zero, forty, 1, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);          // a wave's start, another length
    EXPECT(ry_crepe_track_uploaded(a, back, back_n, 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);         // descending
    EXPECT(ry_crepe_track_uploaded(a, twice, twice_n, 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);       // a wave twice
    EXPECT(ry_crepe_track_uploaded(a, first, small_n, 0, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);
    EXPECT(ry_crepe_track_uploaded(a, first, small_n, 2, 16000, 0, 5.0, 0.1, nf, v, f, t, 0) == -1);
    EXPECT(ry_crepe_track_uploaded(a, first, small_n, 2, 16000, 80, 0.0, 0.1, nf, v, f, t, 0) == -1);
    EXPECT(ry_crepe_track_uploaded(a, first, small_n, 2, 16000, 80, 5.0, 0.1, nullptr, v, f, t, 0) == -1);
    EXPECT(ry_crepe_track_uploaded(a, first, small_n, 2, 16000, 80, 5.0, 0.1, nf, nullptr, f, t, 0) == -1);
    EXPECT(ry_crepe_track_uploaded(a, first, nullptr, 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);
    EXPECT(ry_crepe_track_uploaded(a, first, small_n, 2, 24000, 80, 5.0, 0.1, nf, v, f, t, 0) < 0);          // another rate
    EXPECT(ry_crepe_uploaded_buffers(a, nullptr, &total, &nt, nullptr, nullptr, nullptr, nullptr) == 0 && total == 81 && nt == 0);
    EXPECT(ry_crepe_track_uploaded(a, first, small_n, 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == 0);          // the table is still good
    EXPECT(ry_crepe_track_uploaded(a, nullptr, small_n, 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);      // a null table forgets the upload
    EXPECT(ry_crepe_uploaded_buffers(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);
    // another call on the handle forgets the table
    EXPECT(ry_crepe_upload_waves(a, xs.data(), small_n, 2, 16000, &wave) == 0);
    int nf1 = 0;
    EXPECT(ry_crepe_track(a, xs.data(), 80, 16000, 80, 5.0, 0.1, &nf1, v, f, t, 0) == 0);
    EXPECT(ry_crepe_track_uploaded(a, first, small_n, 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -4);
    // the bank over the uploaded table: stream 1 sits the first call out, then takes part; a wave named for a stream outside the bank, a stream twice
    ry_crepe_bank* bank = nullptr;
    EXPECT(ry_crepe_bank_create(a, 2, &bank) == 0);
    int nc[2] = {0, 0};
    const int adv[2] = {-1, -1}, ok[2] = {0, 0}, s0[1] = {0}, s01[2] = {0, 1}, s00[2] = {0, 0}, s02[2] = {0, 2};
    EXPECT(ry_crepe_bank_track_uploaded(bank, first02, n02, s01, 2, 16000, 80, 5.0, 0.1, adv, ok, nf, nc, v, f, t, 0) == -4);       // no table
    EXPECT(ry_crepe_upload_waves(a, xl.data(), large_n, 3, 16000, &wave) == 0);
    EXPECT(ry_crepe_bank_track_uploaded(bank, first02, n02, s0, 1, 16000, 80, 5.0, 0.1, adv, ok, nf, nc, v, f, t, 0) == 0 && nf[0] == 5 && nc[0] == 5);
    EXPECT(ry_crepe_bank_track_uploaded(bank, first02, n02, s01, 2, 16000, 80, 5.0, 0.1, adv, ok, nf, nc, v, f, t, 0) == 0 && nf[1] == 4 && nc[1] == 4);
    EXPECT(ry_crepe_uploaded_buffers(a, nullptr, nullptr, &nt, &fo, nullptr, nullptr, nullptr) == 0 && nt == 2 && fo[2] == 9);
    EXPECT(ry_crepe_bank_track_uploaded(bank, first02, n02, s00, 2, 16000, 80, 5.0, 0.1, adv, ok, nf, nc, v, f, t, 0) == -1);
    EXPECT(ry_crepe_bank_track_uploaded(bank, first02, n02, s02, 2, 16000, 80, 5.0, 0.1, adv, ok, nf, nc, v, f, t, 0) == -1);
    EXPECT(ry_crepe_bank_track_uploaded(bank, back, back_n, s01, 2, 16000, 80, 5.0, 0.1, adv, ok, nf, nc, v, f, t, 0) == -1);
    EXPECT(ry_crepe_bank_track_uploaded(bank, first02, n02, nullptr, 2, 16000, 80, 5.0, 0.1, adv, ok, nf, nc, v, f, t, 0) == -1);
    EXPECT(ry_crepe_bank_track_uploaded(bank, first02, n02, s01, 2, 16000, 80, 5.0, 0.1, nullptr, ok, nf, nc, v, f, t, 0) == -1);
    EXPECT(ry_crepe_bank_track_uploaded(bank, first02, n02, s01, 2, 16000, 80, 5.0, 0.1, adv, ok, nf, nullptr, v, f, t, 0) == -1);
    EXPECT(ry_crepe_bank_track_uploaded(nullptr, first02, n02, s01, 2, 16000, 80, 5.0, 0.1, adv, ok, nf, nc, v, f, t, 0) == -4);
    EXPECT(ry_crepe_bank_track_uploaded(bank, first02, n02, s01, 2, 16000, 80, 5.0, 0.1, adv, ok, nf, nc, v, f, t, 0) == 0);       // the table outlived the refusals
    EXPECT(ry_crepe_bank_track_uploaded(bank, nullptr, n02, s01, 2, 16000, 80, 5.0, 0.1, adv, ok, nf, nc, v, f, t, 0) == -1);
    long long frames = 0;
    EXPECT(ry_crepe_debug_frames(a, &frames) == 0 && frames > 0);
    EXPECT(ry_crepe_debug_frames(a, nullptr) == -1 && ry_crepe_debug_frames(nullptr, &frames) == -1);
    ry_crepe_bank_destroy(bank);
    ry_crepe_destroy(a);                                                               // with a table on it
    ry_crepe_destroy(b);
}

// ---- the verdict, the compaction, the masked window call: their tables and refusals, then the whole chain once
static void check_window(ry_ctx* ctx) {
    ry_net *s1 = make_net(ctx, 1), *s2 = make_net(ctx, 2);
    std::vector<float> mtx((size_t)9 * 513);
    for (size_t i = 0; i < mtx.size(); ++i) mtx[i] = 0.01f * std::cos(0.011f * (float)i);
    ry_vc* vc = nullptr;
    EXPECT(ry_vc_create(s1, s2, mtx.data(), 9, 513, &vc) == 0);
    EXPECT(ry_vc_set_lanes(vc, 2) == 0);
    ry_crepe* c = make_crepe(ctx);
    ry_analysis* an = nullptr;
    EXPECT(ry_analysis_create(ctx, 16000, 1024, 8, 0.41, -0.15, 71.0, 5, &an) == 0);
    // three waves: audible, silent (zeros), audible
    const int counts[3] = {320, 160, 240}, hop = 80;
    std::vector<float> x = tone(720, 4);
    for (int i = 320; i < 480; ++i) x[(size_t)i] = 0.f;
    const long long so[4] = {0, 320, 480, 720};
    const int fo[4] = {0, 5, 8, 12}, n = 12;                                            // 1 + samples / 80 frames per wave, the tracker's rule at 16 kHz
    std::vector<float> nan_rows((size_t)n * 513);
    std::memset(nan_rows.data(), 0xff, nan_rows.size() * sizeof(float));
    float* mc32 = on_card(ctx, nan_rows.data(), (size_t)n * 9);
    float* sp32 = on_card(ctx, nan_rows.data(), nan_rows.size());
    float* ap32 = on_card(ctx, nan_rows.data(), nan_rows.size());
    float* mc_out = on_card(ctx, nullptr, (size_t)n * 9);
    float* sp_out = on_card(ctx, nullptr, (size_t)n * 513);
    float* maskw = on_card(ctx, nullptr, 8);
    unsigned char* dm = (unsigned char*)maskw;
    const float* wave = nullptr;
    EXPECT(ry_crepe_upload_waves(c, x.data(), counts, 3, 16000, &wave) == 0);
    unsigned char eff[16];
    int n_eff[3] = {-1, -1, -1};
    const float p_eff = 1e-6f, p_all = 3e38f;
    // refusals of the verdict
    EXPECT(ry_vc_gate_verdict_waves_device(nullptr, wave, so, fo, 3, hop, 1024, p_eff, p_all, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_gate_verdict_waves_device(vc, nullptr, so, fo, 3, hop, 1024, p_eff, p_all, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, nullptr, fo, 3, hop, 1024, p_eff, p_all, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, so, nullptr, 3, hop, 1024, p_eff, p_all, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, so, fo, 0, hop, 1024, p_eff, p_all, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, so, fo, 3, 0, 1024, p_eff, p_all, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, so, fo, 3, hop, 1000, p_eff, p_all, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, so, fo, 3, hop, 1024, p_eff, p_all, nullptr, eff, n_eff) == -1);
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, so, fo, 3, hop, 1024, p_eff, p_all, dm, nullptr, n_eff) == -1);
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, so, fo, 3, hop, 1024, p_eff, p_all, dm, eff, nullptr) == -1);
    const long long so_bad[4] = {0, 480, 320, 720};
    const int fo_bad[4] = {0, 5, 5, 12};
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, so_bad, fo, 3, hop, 1024, p_eff, p_all, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, so, fo_bad, 3, hop, 1024, p_eff, p_all, dm, eff, n_eff) == -1);
    EXPECT(n_eff[0] == -1);
    // the verdict
    EXPECT(ry_vc_gate_verdict_waves_device(vc, wave, so, fo, 3, hop, 1024, p_eff, p_all, dm, eff, n_eff) == 0);
    EXPECT(n_eff[0] == 5 && n_eff[1] == 0 && n_eff[2] == 4);
    // the audible subset: tracker and analysis, rows at the waves' places in the layout of the whole call
    const int first[2] = {0, 480}, ns[2] = {320, 240};
    int nf[2] = {0, 0};
    EXPECT(ry_crepe_track_uploaded(c, first, ns, 2, 16000, 80, 5.0, 0.1, nf, nullptr, nullptr, nullptr, 1) == 0 && nf[0] == 5 && nf[1] == 4);
    long long total = 0;
    int nt = 0;
    const int* tfo = nullptr;
    const double *fd = nullptr, *td = nullptr;
    EXPECT(ry_crepe_uploaded_buffers(c, &wave, &total, &nt, &tfo, nullptr, &fd, &td) == 0 && nt == 2 && total == 720);
    const long long fs64[2] = {0, 480};
    const int rows[2] = {0, 8};
    // refusals of the spans call: nothing is written
    const long long overlap[2] = {0, 300}, outside[2] = {0, 600};
    const int rows_back[2] = {8, 0}, rows_lap[2] = {0, 3}, zero_n[2] = {320, 0}, tfo_bad[3] = {1, 5, 9}, tfo_flat[3] = {0, 5, 5};
    EXPECT(ry_analysis_extract_spans_resident(nullptr, wave, total, fs64, ns, fd, td, tfo, rows, 2, 0.85, mc32, sp32, ap32) == -4);
    EXPECT(ry_analysis_extract_spans_resident(an, nullptr, total, fs64, ns, fd, td, tfo, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, nullptr, ns, fd, td, tfo, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, nullptr, fd, td, tfo, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, nullptr, td, tfo, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, nullptr, tfo, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, nullptr, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, tfo, nullptr, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, tfo, rows, 0, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, tfo, rows, 2, 0.85, nullptr, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, tfo, rows, 2, 0.85, mc32, nullptr, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, tfo, rows, 2, 0.85, mc32, sp32, nullptr) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, overlap, ns, fd, td, tfo, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, outside, ns, fd, td, tfo, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, zero_n, fd, td, tfo, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, tfo_bad, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, tfo_flat, rows, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, tfo, rows_back, 2, 0.85, mc32, sp32, ap32) == -1);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, tfo, rows_lap, 2, 0.85, mc32, sp32, ap32) == -1);
    std::vector<float> got((size_t)n * 513);
    EXPECT(ry_dev_download(ctx, got.data(), sp32, got.size()) == 0);
    EXPECT(std::memcmp(got.data(), nan_rows.data(), got.size() * sizeof(float)) == 0);
    EXPECT(ry_analysis_extract_spans_resident(an, wave, total, fs64, ns, fd, td, tfo, rows, 2, 0.85, mc32, sp32, ap32) == 0);
    EXPECT(ry_dev_download(ctx, got.data(), sp32, got.size()) == 0);
    for (int r = 0; r < n; ++r) {                                                      // the rows of the silent wave (5 .. 7) keep their NaN patterns
        const bool written = std::memcmp(&got[(size_t)r * 513], &nan_rows[0], 513 * sizeof(float)) != 0;
        EXPECT(written == (r < 5 || r >= 8));
    }
    // refusals of the compaction and of the masked window call
    const int ne_low[3] = {4, 0, 4}, ne_out[3] = {6, 0, 4}, ne_neg[3] = {5, -1, 4}, fo_one[4] = {1, 5, 8, 12};
    float* xe = on_card(ctx, nan_rows.data(), (size_t)n * 9);
    float* ro = on_card(ctx, nan_rows.data(), (size_t)n);
    EXPECT(ry_vc_compact_waves_device(nullptr, fo, 3, dm, eff, n_eff, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, nullptr, 3, dm, eff, n_eff, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 0, dm, eff, n_eff, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, nullptr, eff, n_eff, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, dm, nullptr, n_eff, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, dm, eff, nullptr, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, dm, eff, n_eff, nullptr, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, dm, eff, n_eff, mc32, nullptr, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, dm, eff, n_eff, mc32, xe, nullptr) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo_bad, 3, dm, eff, n_eff, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo_one, 3, dm, eff, n_eff, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, dm, eff, ne_low, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, dm, eff, ne_out, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, dm, eff, ne_neg, mc32, xe, (int*)ro) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(nullptr, fo, 3, mc32, 1e-16f, mc_out, sp_out, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, nullptr, 3, mc32, 1e-16f, mc_out, sp_out, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 3, nullptr, 1e-16f, mc_out, sp_out, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 3, mc32, 1e-16f, nullptr, sp_out, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 3, mc32, 1e-16f, mc_out, nullptr, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 3, mc32, 1e-16f, mc_out, sp_out, nullptr, eff, n_eff) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 3, mc32, 1e-16f, mc_out, sp_out, dm, nullptr, n_eff) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 3, mc32, 1e-16f, mc_out, sp_out, dm, eff, nullptr) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo_bad, 3, mc32, 1e-16f, mc_out, sp_out, dm, eff, n_eff) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 3, mc32, 1e-16f, mc_out, sp_out, dm, eff, ne_low) == -1);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 65537, mc32, 1e-16f, mc_out, sp_out, dm, eff, n_eff) == -1);
    EXPECT(ry_sync(ctx) == 0);
    std::vector<float> xg((size_t)n * 9);
    EXPECT(ry_dev_download(ctx, xg.data(), xe, xg.size()) == 0);
    EXPECT(std::memcmp(xg.data(), nan_rows.data(), xg.size() * sizeof(float)) == 0);
    // the compaction alone into the caller's blocks, then into the core's; the masked window call twice in a row (nothing is waited for in between),
    // with a discard hint the second time; a window call of another shape after it (the pinned table is rewritten)
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, dm, eff, n_eff, mc32, xe, (int*)ro) == 0);
    std::vector<int> rg((size_t)n);
    EXPECT(ry_dev_download(ctx, (float*)rg.data(), ro, rg.size()) == 0);
    EXPECT(rg[0] == 0 && rg[4] == 4 && rg[5] == -1 && rg[7] == -1 && rg[8] == 0 && rg[11] == 3);
    EXPECT(ry_vc_compact_waves_device(vc, fo, 3, dm, eff, n_eff, mc32, nullptr, nullptr) == 0);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 3, mc32, 1e-16f, mc_out, sp_out, dm, eff, n_eff) == 0);
    EXPECT(ry_vc_set_discard(vc, 1, 1) == 0);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 3, mc32, 1e-16f, mc_out, sp_out, dm, eff, n_eff) == 0);
    EXPECT(ry_vc_set_discard(vc, 0, 0) == 0);
    EXPECT(ry_mask_rows(ctx, ap32, dm, n, 513, 0, n, nullptr) == 0);
    EXPECT(ry_sync(ctx) == 0);
    std::vector<float> mc((size_t)n * 9);
    EXPECT(ry_dev_download(ctx, mc.data(), mc_out, mc.size()) == 0);
    for (int r = 5; r < 8; ++r) for (int k = 0; k < 9; ++k) EXPECT(mc[(size_t)r * 9 + k] == 0.0f);           // the silent wave: combine_silent's zeros
    for (size_t i = 0; i < mc.size(); ++i) EXPECT(mc[i] == mc[i]);                                          // no NaN reached mc
    EXPECT(ry_dev_download(ctx, got.data(), ap32, got.size()) == 0);
    for (size_t i = 0; i < got.size(); ++i) EXPECT(got[i] == got[i]);                                       // nor ap, once masked
    // every wave silent: no compaction is launched, the feature block is not read at all
    unsigned char none[16] = {0};
    const int ne_none[3] = {0, 0, 0};
    float* zmask = on_card(ctx, none, 4);
    float* nan_feat = on_card(ctx, nan_rows.data(), (size_t)n * 9);
    EXPECT(ry_vc_enqueue_waves_masked_device(vc, fo, 3, nan_feat, 1e-16f, mc_out, sp_out, (unsigned char*)zmask, none, ne_none) == 0);
    EXPECT(ry_sync(ctx) == 0);
    EXPECT(ry_dev_download(ctx, mc.data(), mc_out, mc.size()) == 0);
    for (size_t i = 0; i < mc.size(); ++i) EXPECT(mc[i] == 0.0f);
    // one long wave after the short ones: the blocks of the call grow
    const int fo_long[2] = {0, 1300};
    std::vector<unsigned char> long_mask(1300);
    int ones = 0;
    for (int i = 0; i < 1300; ++i) { long_mask[(size_t)i] = (unsigned char)(i % 3 == 0); ones += long_mask[(size_t)i]; }
    std::vector<float> long_feat((size_t)1300 * 9);
    for (size_t i = 0; i < long_feat.size(); ++i) long_feat[i] = (float)i;
    std::vector<unsigned char> padded(long_mask);
    padded.resize(1304);
    float* lm = on_card(ctx, padded.data(), 326);
    float* lf = on_card(ctx, long_feat.data(), long_feat.size());
    float* lx = on_card(ctx, nullptr, long_feat.size());
    float* lr = on_card(ctx, nullptr, 1300);
    EXPECT(ry_vc_compact_waves_device(vc, fo_long, 1, (unsigned char*)lm, long_mask.data(), &ones, lf, lx, (int*)lr) == 0);
    std::vector<int> lrow(1300);
    std::vector<float> lrows((size_t)1300 * 9);
    EXPECT(ry_dev_download(ctx, (float*)lrow.data(), lr, 1300) == 0);
    EXPECT(ry_dev_download(ctx, lrows.data(), lx, lrows.size()) == 0);
    for (int k = 0; k < ones; ++k) {                                                   // across the second round of 1024 frames
        EXPECT(lrow[(size_t)k] == 3 * k);
        EXPECT(lrows[(size_t)k * 9] == (float)(3 * k * 9) && lrows[(size_t)k * 9 + 8] == (float)(3 * k * 9 + 8));
    }
    for (float* p : {mc32, sp32, ap32, mc_out, sp_out, maskw, xe, ro, zmask, nan_feat, lm, lf, lx, lr}) EXPECT(ry_dev_free(ctx, p) == 0);
    ry_analysis_destroy(an);
    ry_crepe_destroy(c);
    ry_vc_destroy(vc);                                                                 // with a compaction's event recorded
    ry_net_destroy(s1);
    ry_net_destroy(s2);
}

int main() {
    ry_ctx* ctx = nullptr;
    EXPECT(ry_init(0, &ctx) == 0);
    check_tracker(ctx);
    check_window(ctx);
    ry_shutdown(ctx);
    std::printf(failures ? "gate_first_host_check: %d FAILED\n" : "gate_first_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
