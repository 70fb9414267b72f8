// synth_many_host_check.cpp -- the host paths of the batched synthesis (ry_synth_run_many, ry_synth_debug_pulses_many, ry_synth_debug_poison) in a
// stand-alone program over the emulator build of libry355, meant to be compiled and linked with -fsanitize=address,undefined
// (scripts/asan_synth_many.sh): the segment table and the packed upload, every refusal with the outputs watched, buffer growth from a small call to
// a larger one and back, a batched call around an open stream, poison, destroy after a batched call and without one.  A handful of frames per
// wave.  Exit status 0: every call returned what it should and every wave of a batch equals ry_synth_run on it alone.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ry355.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, ry_last_error()); ++failures; } } while (0)

static const int BINS = 513;
static const double MARK = -7.25;

struct Frames { std::vector<double> f0; std::vector<float> sp, ap; };

static Frames frames(int n, int seed) {
    Frames f;
    f.f0.resize((size_t)n); f.sp.resize((size_t)n * BINS); f.ap.resize((size_t)n * BINS);
    for (int i = 0; i < n; ++i) {
        f.f0[(size_t)i] = (i + seed) % 7 == 6 ? 0.0 : 140.0 + 9.0 * ((i * 5 + seed) % 11);
        for (int k = 0; k < BINS; ++k) {
            f.sp[(size_t)i * BINS + k] = 1e-3f * (1.5f + std::sin(0.05f * (float)(k + 3 * i + seed)));
            f.ap[(size_t)i * BINS + k] = 0.5f + 0.45f * std::sin(0.11f * (float)(k + i + 2 * seed));
        }
    }
    return f;
}

// the batched call on waves of n[0 .. b) frames cut from `f`, every wave against the single call on `one`
static void check(ry_synth* many, ry_synth* one, const Frames& f, const int* n, int b) {
    long long total = 0;
    for (int i = 0; i < b; ++i) total += ry_synth_length(many, n[i]);
    std::vector<double> y((size_t)total + 3, MARK), y1((size_t)total + 3);
    std::vector<long long> off((size_t)b + 1, -99);
    EXPECT(ry_synth_run_many(many, f.f0.data(), f.sp.data(), f.ap.data(), n, b, BINS, 0, y.data(), total, off.data()) == 0);
    EXPECT(off[0] == 0 && off[(size_t)b] == total && y[(size_t)total] == MARK);
    int row = 0, cnt = -1;
    EXPECT(ry_synth_debug_pulses(many, nullptr, nullptr, nullptr, 0, &cnt) == 0 && cnt == 0);
    for (int i = 0; i < b; ++i) {
        int got = 0, np = 0, np1 = 0;
        EXPECT(ry_synth_run(one, f.f0.data() + row, f.sp.data() + (size_t)row * BINS, f.ap.data() + (size_t)row * BINS, n[i], BINS, 0, y1.data(), (int)total, &got) == 0);
        EXPECT(off[(size_t)i + 1] - off[(size_t)i] == got);
        EXPECT(std::memcmp(y.data() + off[(size_t)i], y1.data(), (size_t)got * sizeof(double)) == 0);
        EXPECT(ry_synth_debug_pulses_many(many, i, nullptr, nullptr, nullptr, 0, &np) == 0);
        EXPECT(ry_synth_debug_pulses(one, nullptr, nullptr, nullptr, 0, &np1) == 0 && np == np1);
        std::vector<long long> ix((size_t)np + 1), ix1((size_t)np + 1);
        std::vector<double> sh((size_t)np + 1), sh1((size_t)np + 1);
        std::vector<int> vo((size_t)np + 1), vo1((size_t)np + 1);
        EXPECT(ry_synth_debug_pulses_many(many, i, ix.data(), sh.data(), vo.data(), np, &np) == 0);
        EXPECT(ry_synth_debug_pulses(one, ix1.data(), sh1.data(), vo1.data(), np1, &np1) == 0);
        EXPECT(std::memcmp(ix.data(), ix1.data(), (size_t)np * sizeof(long long)) == 0 && std::memcmp(sh.data(), sh1.data(), (size_t)np * sizeof(double)) == 0 &&
               std::memcmp(vo.data(), vo1.data(), (size_t)np * sizeof(int)) == 0);
        if (np > 0) EXPECT(ry_synth_debug_pulses_many(many, i, ix.data(), nullptr, nullptr, np - 1, &np) == -1);
        row += n[i];
    }
    EXPECT(ry_synth_debug_pulses_many(many, b, nullptr, nullptr, nullptr, 0, &cnt) == -1);
    EXPECT(ry_synth_debug_pulses_many(many, -1, nullptr, nullptr, nullptr, 0, &cnt) == -1);
}

int main() {
    ry_ctx* ctx = nullptr;
    EXPECT(ry_init(0, &ctx) == 0);
    ry_synth *a = nullptr, *b = nullptr, *idle = nullptr, *slow = nullptr;
    EXPECT(ry_synth_create(ctx, 16000, 5.0, 1024, 3, &a) == 0);
    EXPECT(ry_synth_create(ctx, 16000, 5.0, 1024, 3, &b) == 0);
    EXPECT(ry_synth_create(ctx, 16000, 5.0, 1024, 3, &idle) == 0);
    EXPECT(ry_synth_create(ctx, 48000, 1000.0, 1024, 3, &slow) == 0);
    int cnt = -1;
    EXPECT(ry_synth_debug_pulses_many(a, 0, nullptr, nullptr, nullptr, 0, &cnt) == -4 && cnt == 0);
    EXPECT(ry_synth_debug_pulses_many(nullptr, 0, nullptr, nullptr, nullptr, 0, &cnt) == -4);

    // a small call, a larger one (every buffer grows, more waves), the small one again, poisoned in between
    const Frames f = frames(24, 1);
    const int small_n[2] = {1, 3}, large_n[4] = {6, 1, 13, 4};
    check(a, b, f, small_n, 2);
    check(a, b, f, large_n, 4);
    EXPECT(ry_synth_debug_poison(a) == 0);
    EXPECT(ry_synth_debug_pulses_many(a, 0, nullptr, nullptr, nullptr, 0, &cnt) == -4);       // the slices are gone
    check(a, b, f, small_n, 2);

    // a batched call around an open stream: the stream is dropped and left reset
    std::vector<double> y(4000, MARK);
    int got = 0;
    EXPECT(ry_synth_push(a, f.f0.data(), f.sp.data(), f.ap.data(), 9, BINS, 0, y.data(), 4000, &got) == 0);
    EXPECT(ry_synth_bound(a, 0, 1) > 0);
    check(a, b, f, small_n, 2);
    EXPECT(ry_synth_bound(a, 0, 1) == 0);
    EXPECT(ry_synth_flush(a, y.data(), 4000, &got) == -4);
    EXPECT(ry_synth_run(a, f.f0.data(), f.sp.data(), f.ap.data(), 5, BINS, 0, y.data(), 4000, &got) == 0 && got == 321);
    EXPECT(ry_synth_debug_pulses_many(a, 0, nullptr, nullptr, nullptr, 0, &cnt) == -4);       // the last call was another one

    // the refusals: nothing is written
    std::fill(y.begin(), y.end(), MARK);
    long long off[5] = {-99, -99, -99, -99, -99};
    const double* F = f.f0.data();
    const float *S = f.sp.data(), *A = f.ap.data();
    EXPECT(ry_synth_run_many(nullptr, F, S, A, large_n, 4, BINS, 0, y.data(), 4000, off) == -4);
    EXPECT(ry_synth_run_many(a, nullptr, S, A, large_n, 4, BINS, 0, y.data(), 4000, off) == -1);
    EXPECT(ry_synth_run_many(a, F, nullptr, A, large_n, 4, BINS, 0, y.data(), 4000, off) == -1);
    EXPECT(ry_synth_run_many(a, F, S, nullptr, large_n, 4, BINS, 0, y.data(), 4000, off) == -1);
    EXPECT(ry_synth_run_many(a, F, S, A, nullptr, 4, BINS, 0, y.data(), 4000, off) == -1);
    EXPECT(ry_synth_run_many(a, F, S, A, large_n, 4, BINS, 0, nullptr, 4000, off) == -1);
    EXPECT(ry_synth_run_many(a, F, S, A, large_n, 4, BINS, 0, y.data(), 4000, nullptr) == -1);
    EXPECT(ry_synth_run_many(a, F, S, A, large_n, 0, BINS, 0, y.data(), 4000, off) == -1);
    EXPECT(ry_synth_run_many(a, F, S, A, large_n, 4, 512, 0, y.data(), 4000, off) == -1);
    const int none[3] = {2, 0, 2}, over[2] = {1 << 22, 1}, wide[2] = {12000, 12000};
    EXPECT(ry_synth_run_many(a, F, S, A, none, 3, BINS, 0, y.data(), 4000, off) == -1 && std::strstr(ry_last_error(), "wave 1") != nullptr);
    EXPECT(ry_synth_run_many(a, F, S, A, over, 2, BINS, 0, y.data(), 4000, off) == -1 && std::strstr(ry_last_error(), "frames") != nullptr);      // from the counts: nothing is read
    EXPECT(ry_synth_run_many(slow, F, S, A, wide, 2, BINS, 0, y.data(), 1LL << 40, off) == -1 && std::strstr(ry_last_error(), "samples") != nullptr);
    Frames bad = f;
    bad.f0[6 + 1 + 2] = std::numeric_limits<double>::quiet_NaN();                              // wave 2, frame 2
    EXPECT(ry_synth_run_many(a, bad.f0.data(), S, A, large_n, 4, BINS, 0, y.data(), 4000, off) == -1 && std::strstr(ry_last_error(), "wave 2: f0[2]") != nullptr);
    bad.f0[6 + 1 + 2] = 8000.0;
    EXPECT(ry_synth_run_many(a, bad.f0.data(), S, A, large_n, 4, BINS, 0, y.data(), 4000, off) == -1);
    long long need = 0;
    for (int i = 0; i < 4; ++i) need += ry_synth_length(a, large_n[i]);
    EXPECT(ry_synth_run_many(a, F, S, A, large_n, 4, BINS, 0, y.data(), need - 1, off) == -1 && std::strstr(ry_last_error(), "y holds") != nullptr);
    bool clean = true;
    for (double v : y) clean = clean && v == MARK;
    for (long long v : off) clean = clean && v == -99;
    EXPECT(clean);
    EXPECT(ry_synth_run_many(a, F, S, A, large_n, 4, BINS, 0, y.data(), need, off) == 0 && off[4] == need && y[(size_t)need] == MARK);    // exactly enough room; destroyed with a batched call on it
    ry_synth_destroy(a);
    ry_synth_destroy(b);
    ry_synth_destroy(idle);                                                                     // ... and without one
    ry_synth_destroy(slow);
    ry_shutdown(ctx);
    std::printf(failures ? "%d checks failed\n" : "synth_many_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
