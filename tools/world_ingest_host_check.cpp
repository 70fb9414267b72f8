// world_ingest_host_check.cpp -- the host paths of the caller's-own-track ingest (ry_analysis_upload_waves, ry_analysis_ingest_tracks,
// ry_analysis_track_buffers) in a stand-alone program over the emulator build of libry355, meant to be compiled and linked with
// -fsanitize=address,undefined (scripts/asan_world_ingest.sh): upload and ingest growing across calls (every buffer reallocated more than once,
// the handle's host copy of the upload with it), the refusals (before and after a good call: the previous track stays), the kernel's segment
// search at one and at many waves, the poison hook, the extract calls reading the track in place, and destroy with and without a track.
// Exit status 0: every call returned what it should and every downloaded value equals the statement t = (k * period) / 1000, voiced = f0 != 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ry355.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, ry_last_error()); ++failures; } } while (0)

static std::vector<double> track(int n, int seed) {
    std::vector<double> f((size_t)n);
    for (int i = 0; i < n; ++i) f[(size_t)i] = (i + seed) % 5 == 0 ? 0.0 : 100.0 + 3.0 * ((i * 7 + seed) % 40);
    return f;
}

// the track on the card against the statement, wave by wave
static void check_track(ry_ctx* ctx, ry_analysis* a, const std::vector<double>& f0, const std::vector<int>& counts, double period, int want_waves) {
    const float* wave = nullptr; const unsigned char* vd = nullptr; const double *fd = nullptr, *td = nullptr;
    const long long* so = nullptr; const int* fo = nullptr;
    int nw = -1, nt = -1;
    EXPECT(ry_analysis_track_buffers(a, &wave, &nw, &so, &nt, &fo, &vd, &fd, &td) == 0);
    EXPECT(nt == (int)counts.size() && nw == want_waves && (want_waves == 0) == (wave == nullptr) && (want_waves == 0) == (so == nullptr));
    if (nt != (int)counts.size()) return;
    const size_t n = f0.size();
    EXPECT(fo[0] == 0 && (size_t)fo[nt] == n);
    std::vector<double> gf(n), gt(n);
    std::vector<unsigned char> gv((n + 3) / 4 * 4);
    EXPECT(ry_dev_download(ctx, (float*)gf.data(), (const float*)fd, 2 * n) == 0);
    EXPECT(ry_dev_download(ctx, (float*)gt.data(), (const float*)td, 2 * n) == 0);
    EXPECT(ry_dev_download(ctx, (float*)gv.data(), (const float*)vd, gv.size() / 4) == 0);
    size_t at = 0;
    for (int w = 0; w < nt; ++w) {
        EXPECT(fo[w] == (int)at && fo[w + 1] - fo[w] == counts[(size_t)w]);
        for (int k = 0; k < counts[(size_t)w]; ++k, ++at) {
            const volatile double ms = (double)k * period;              // two roundings, as the kernel makes them
            const double t = ms / 1000.0;
            EXPECT(std::memcmp(&gf[at], &f0[at], sizeof(double)) == 0 && std::memcmp(&gt[at], &t, sizeof(double)) == 0);
            EXPECT(gv[at] == (f0[at] != 0.0 ? 1 : 0));
        }
    }
}

static void refusals(ry_analysis* a) {
    const float x[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    const double f[8] = {0, 100, 0, 120, 130, 0, 0, 150};
    const float* wave = nullptr;
    const int one[1] = {8}, none[3] = {4, 0, 4}, neg[1] = {-3}, huge[2] = {2147483647, 1}, many[2] = {1 << 22, 1};
    EXPECT(ry_analysis_upload_waves(nullptr, x, one, 1, &wave) == -4);
    EXPECT(ry_analysis_upload_waves(a, nullptr, one, 1, &wave) == -1);
    EXPECT(ry_analysis_upload_waves(a, x, nullptr, 1, &wave) == -1);
    EXPECT(ry_analysis_upload_waves(a, x, one, 1, nullptr) == -1);
    EXPECT(ry_analysis_upload_waves(a, x, one, 0, &wave) == -1);
    EXPECT(ry_analysis_upload_waves(a, x, none, 3, &wave) == -1);
    EXPECT(ry_analysis_upload_waves(a, x, neg, 1, &wave) == -1);
    EXPECT(ry_analysis_upload_waves(a, x, huge, 2, &wave) == -1);        // refused from the counts: the audio is not read
    EXPECT(ry_analysis_ingest_tracks(nullptr, f, one, 1, 5.0) == -4);
    EXPECT(ry_analysis_ingest_tracks(a, nullptr, one, 1, 5.0) == -1);
    EXPECT(ry_analysis_ingest_tracks(a, f, nullptr, 1, 5.0) == -1);
    EXPECT(ry_analysis_ingest_tracks(a, f, one, 0, 5.0) == -1);
    EXPECT(ry_analysis_ingest_tracks(a, f, none, 3, 5.0) == -1);
    EXPECT(ry_analysis_ingest_tracks(a, f, neg, 1, 5.0) == -1);
    EXPECT(ry_analysis_ingest_tracks(a, f, many, 2, 5.0) == -1);         // refused from the counts: f0 is not read
    EXPECT(ry_analysis_ingest_tracks(a, f, one, 1, 0.0) == -1);
    EXPECT(ry_analysis_ingest_tracks(a, f, one, 1, -5.0) == -1);
    EXPECT(ry_analysis_ingest_tracks(a, f, one, 1, std::numeric_limits<double>::quiet_NaN()) == -1);
    EXPECT(ry_analysis_ingest_tracks(a, f, one, 1, std::numeric_limits<double>::infinity()) == -1);
    EXPECT(ry_analysis_track_buffers(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);
}

int main() {
    ry_ctx* ctx = nullptr;
    EXPECT(ry_init(0, &ctx) == 0);
    if (!ctx) return 1;
    const int fs = 16000;
    // destroy without a track, and with waves alone
    ry_analysis* a = nullptr;
    EXPECT(ry_analysis_create(ctx, fs, 1024, 8, 0.41, -0.15, 71.0, 5, &a) == 0);
    ry_analysis_destroy(a);
    EXPECT(ry_analysis_create(ctx, fs, 1024, 8, 0.41, -0.15, 71.0, 5, &a) == 0);
    EXPECT(ry_analysis_track_buffers(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);
    refusals(a);
    EXPECT(ry_analysis_track_buffers(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);
    // a track without uploaded waves
    {
        const std::vector<double> f = track(5, 1);
        const int c[1] = {5};
        EXPECT(ry_analysis_ingest_tracks(a, f.data(), c, 1, 5.0) == 0);
        check_track(ctx, a, f, {5}, 5.0, 0);
    }
    // upload and ingest growing across calls: 1 wave of 1 frame ... several waves of hundreds; shrinking in between
    const int shapes[7][3] = {{1, 0, 0}, {3, 2, 0}, {64, 65, 1}, {2, 0, 0}, {257, 300, 63}, {1, 1, 1}, {700, 900, 1200}};
    int round = 0;
    for (const int* sh : shapes) {
        std::vector<int> counts, samples;
        std::vector<double> f0;
        std::vector<float> x;
        for (int w = 0; w < 3 && sh[w] > 0; ++w) {
            counts.push_back(sh[w]);
            samples.push_back(sh[w] * 3 + 1);
            const std::vector<double> t = track(sh[w], round + w);
            f0.insert(f0.end(), t.begin(), t.end());
            for (int i = 0; i < samples.back(); ++i) x.push_back(0.001f * (float)(i + w));
        }
        const float* wave = nullptr;
        const double period = round % 2 ? 5.5 : 5.0;
        EXPECT(ry_analysis_upload_waves(a, x.data(), samples.data(), (int)samples.size(), &wave) == 0 && wave != nullptr);
        EXPECT(ry_analysis_ingest_tracks(a, f0.data(), counts.data(), (int)counts.size(), period) == 0);
        check_track(ctx, a, f0, counts, period, (int)samples.size());
        std::vector<float> back(x.size());
        EXPECT(ry_dev_download(ctx, back.data(), wave, back.size()) == 0);
        EXPECT(std::memcmp(back.data(), x.data(), x.size() * sizeof(float)) == 0);
        refusals(a);                                                    // the previous track stays
        check_track(ctx, a, f0, counts, period, (int)samples.size());
        ++round;
    }
    // the poison hook covers the new buffers and forgets the track; the next call writes what it reads
    EXPECT(ry_analysis_debug_poison(a) == 0);
    EXPECT(ry_analysis_track_buffers(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);
    // the extract call reads the track in place: two short waves, rows left on the card
    {
        const int samples[2] = {200, 360}, counts[2] = {3, 5};
        std::vector<float> x(560);
        for (size_t i = 0; i < x.size(); ++i) x[i] = 0.3f * std::sin(0.09f * (float)i);
        std::vector<double> f0 = track(8, 3);
        const float* wave = nullptr; const double *fd = nullptr, *td = nullptr; const long long* so = nullptr; const int* fo = nullptr;
        EXPECT(ry_analysis_upload_waves(a, x.data(), samples, 2, &wave) == 0);
        EXPECT(ry_analysis_ingest_tracks(a, f0.data(), counts, 2, 5.0) == 0);
        EXPECT(ry_analysis_track_buffers(a, nullptr, nullptr, &so, nullptr, &fo, nullptr, &fd, &td) == 0);
        float *mc = nullptr, *sp = nullptr, *ap = nullptr;
        EXPECT(ry_dev_alloc(ctx, 8 * 9, &mc) == 0 && ry_dev_alloc(ctx, 8 * 513, &sp) == 0 && ry_dev_alloc(ctx, 8 * 513, &ap) == 0);
        EXPECT(ry_analysis_extract_many_resident(a, wave, so, fd, td, fo, 2, 0.85, mc, sp, ap) == 0);
        std::vector<float> rows(8 * 513);
        EXPECT(ry_dev_download(ctx, rows.data(), sp, rows.size()) == 0);
        for (float v : rows) EXPECT(v > 0.0f && std::isfinite(v));
        f0[6] = std::numeric_limits<double>::quiet_NaN();                  // the ingest takes it, the extract's verdict refuses it
        EXPECT(ry_analysis_ingest_tracks(a, f0.data(), counts, 2, 5.0) == 0);
        EXPECT(ry_analysis_track_buffers(a, nullptr, nullptr, &so, nullptr, &fo, nullptr, &fd, &td) == 0);
        EXPECT(ry_analysis_extract_many_resident(a, wave, so, fd, td, fo, 2, 0.85, mc, sp, ap) == -1 && std::strstr(ry_last_error(), "f0[6]") != nullptr);
        EXPECT(ry_dev_free(ctx, mc) == 0 && ry_dev_free(ctx, sp) == 0 && ry_dev_free(ctx, ap) == 0);
    }
    ry_analysis_destroy(a);                                                 // destroy with a track
    ry_shutdown(ctx);
    std::printf(failures ? "world_ingest_host_check: %d FAILED\n" : "world_ingest_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
