// encode_many_host_check.cpp -- the host paths of the many-waves encode (ry_crepe_track_many, ry_crepe_track_many_buffers, ry_crepe_decode_many,
// ry_crepe_voicing_many, ry_analysis_extract_many_dev) in a stand-alone program over the emulator build of libry355, meant to be compiled and linked
// with -fsanitize=address,undefined (scripts/asan_encode_many.sh): the table build, every refusal, buffer growth from a small call to a larger one
// and back, destroy after a batched call and without one.  Smallest capacity, a handful of frames per call.  Exit status 0: every call returned
// what it should and wave 0 of a batch equals the single call on it.
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

int main() {
    ry_ctx* ctx = nullptr;
    EXPECT(ry_init(0, &ctx) == 0);
    const size_t np = ry_crepe_param_count(1);
    std::vector<float> w(np);
    for (size_t i = 0; i < np; ++i) w[i] = 0.05f * std::sin(0.37f * (float)i) + (i % 5 == 4 ? 1.0f : 0.0f);      // variances stay positive below
    ry_crepe *a = nullptr, *b = nullptr, *idle = nullptr;
    EXPECT(ry_crepe_create(ctx, 1, w.data(), np, 1.0f, &a) == 0);
    EXPECT(ry_crepe_create(ctx, 1, w.data(), np, 1.0f, &b) == 0);
    EXPECT(ry_crepe_create(ctx, 1, w.data(), np, 1.0f, &idle) == 0);
    EXPECT(ry_crepe_track_many_buffers(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);

    // a small call, a larger one (every buffer grows), the small one again: wave 0 against the single call on another handle every time
    const int small_n[2] = {1, 80}, large_n[3] = {320, 1, 160};
    std::vector<float> xs = tone(81, 1), xl = tone(481, 2);
    int nf[3] = {0, 0, 0}, nf1 = 0;
    unsigned char v[16], v1[16];
    double f[16], t[16], f1[16], t1[16];
    for (int round = 0; round < 3; ++round) {
        const bool large = round == 1;
        const int* counts = large ? large_n : small_n;
        const std::vector<float>& x = large ? xl : xs;
        EXPECT(ry_crepe_track_many(a, x.data(), counts, large ? 3 : 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == 0);
        EXPECT(ry_crepe_track(b, x.data(), counts[0], 16000, 80, 5.0, 0.1, &nf1, v1, f1, t1, 0) == 0);
        EXPECT(nf[0] == nf1 && nf1 >= 1);
        EXPECT(std::memcmp(v, v1, (size_t)nf1) == 0 && std::memcmp(f, f1, (size_t)nf1 * sizeof(double)) == 0 && std::memcmp(t, t1, (size_t)nf1 * sizeof(double)) == 0);
    }
    // the tracks on the card and their analysis; then the refusals of both calls
    EXPECT(ry_crepe_track_many(a, xl.data(), large_n, 3, 16000, 80, 5.0, 0.1, nf, nullptr, nullptr, nullptr, 1) == 0);
    const float* wave = nullptr;
    const long long* so = nullptr;
    const int* fo = nullptr;
    const unsigned char* vd = nullptr;
    const double *fd = nullptr, *td = nullptr;
    int nw = 0;
    EXPECT(ry_crepe_track_many_buffers(a, &wave, &nw, &so, &fo, &vd, &fd, &td) == 0);
    EXPECT(nw == 3 && so[3] == 481 && fo[3] == nf[0] + nf[1] + nf[2]);
    ry_analysis* an = nullptr;
    EXPECT(ry_analysis_create(ctx, 16000, 1024, 8, 0.41, -0.15, 71.0, 5, &an) == 0);
    const int total = fo[3];
    std::vector<double> sp((size_t)total * 513), mc((size_t)total * 9), ap((size_t)total * 513), coded((size_t)total);
    EXPECT(ry_analysis_extract_many_dev(an, wave, so, fd, td, fo, 3, 0.85, sp.data(), nullptr, mc.data(), ap.data(), nullptr, coded.data()) == 0);
    EXPECT(sp[0] > 0.0 && sp[sp.size() - 1] > 0.0);
    const long long so_bad[4] = {0, 320, 320, 481};
    const int fo_bad[4] = {0, 5, 5, 8}, fo_long[4] = {0, 1 << 22, (1 << 22) + 1, (1 << 22) + 2};
    EXPECT(ry_analysis_extract_many_dev(an, wave, so, fd, td, fo, 0, 0.85, sp.data(), nullptr, mc.data(), ap.data(), nullptr, coded.data()) == -1);
    EXPECT(ry_analysis_extract_many_dev(an, wave, so_bad, fd, td, fo, 3, 0.85, sp.data(), nullptr, mc.data(), ap.data(), nullptr, coded.data()) == -1);
    EXPECT(ry_analysis_extract_many_dev(an, wave, so, fd, td, fo_bad, 3, 0.85, sp.data(), nullptr, mc.data(), ap.data(), nullptr, coded.data()) == -1);
    EXPECT(ry_analysis_extract_many_dev(an, wave, so, fd, td, fo_long, 3, 0.85, sp.data(), nullptr, mc.data(), ap.data(), nullptr, coded.data()) == -1);
    EXPECT(ry_analysis_extract_many_dev(an, wave, so + 1, fd, td, fo, 2, 0.85, sp.data(), nullptr, mc.data(), ap.data(), nullptr, coded.data()) == -1);
    const int none[2] = {80, 0}, huge[3] = {1 << 23, 1 << 23, 8}, wide[3] = {1 << 30, 1 << 30, 8};
    EXPECT(ry_crepe_track_many(a, xl.data(), large_n, 0, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);
    EXPECT(ry_crepe_track_many(a, xl.data(), none, 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == -1);
    EXPECT(ry_crepe_track_many(a, xl.data(), large_n, 3, 24000, 80, 5.0, 0.1, nf, v, f, t, 0) == -4);      // no resampler tables
    EXPECT(ry_crepe_track_many(a, xl.data(), huge, 3, 16000, 1, 5.0, 0.1, nf, v, f, t, 0) == -1);          // refused from the counts: the audio is not read
    EXPECT(ry_crepe_track_many(a, xl.data(), wide, 3, 16000, 1 << 20, 5.0, 0.1, nf, v, f, t, 0) == -1);   // few frames, 2^31 samples: the 32-bit offsets
    EXPECT(std::strstr(ry_last_error(), "samples") != nullptr);
    EXPECT(ry_crepe_track_many(a, xl.data(), large_n, 3, 16000, 80, 0.0, 0.1, nf, v, f, t, 0) == -1);
    EXPECT(ry_crepe_track_many_buffers(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);
    // decode and voicing over a table
    const int tracks[3] = {1, 3, 2};
    std::vector<float> act((size_t)6 * 360, 0.5f), conf = {0.05f, 0.9f, 0.1f, 0.6f, 0.02f, 0.3f}, f0 = {100.f, 110.f, 120.f, 130.f, 140.f, 150.f};
    float df0[6], dconf[6];
    int path[6];
    EXPECT(ry_crepe_decode_many(a, act.data(), tracks, 3, 1, df0, dconf, path) == 0);
    EXPECT(ry_crepe_voicing_many(a, conf.data(), f0.data(), tracks, 3, 0.1, 5.0, v, f, t, 0) == 0);
    EXPECT(t[0] == 0.0 && t[1] == 0.0 && t[4] == 0.0 && t[3] == 2 * 5.0 / 1000.0);
    EXPECT(ry_crepe_voicing_many(a, conf.data(), f0.data(), none, 2, 0.1, 5.0, v, f, t, 0) == -1);
    EXPECT(ry_crepe_debug_poison(a) == 0 && ry_analysis_debug_poison(an) == 0);
    EXPECT(ry_crepe_track_many(a, xs.data(), small_n, 2, 16000, 80, 5.0, 0.1, nf, v, f, t, 0) == 0);       // destroyed with a batched track on it
    ry_analysis_destroy(an);
    ry_crepe_destroy(a);
    ry_crepe_destroy(b);
    ry_crepe_destroy(idle);                                                                                 // ... and without one
    ry_shutdown(ctx);
    std::printf(failures ? "%d checks failed\n" : "encode_many_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
