// synth_bank_host_check.cpp -- the host paths of the bank of synthesis streams (ry_synth_bank_*) in a stand-alone program over the emulator build
// of libry355, meant to be compiled and linked with -fsanitize=address,undefined (scripts/asan_synth_bank.sh): create, ragged pushes with
// streams that sit out, `final` with and without frames and a slot that starts again, every refusal with the outputs watched and a valid push
// after it, buffer growth from small pushes to a large one and back, poison between calls, the debug calls, destroy.  A handful of frames per
// push.  Exit status 0: every call returned what it should and every stream of every push equals ry_synth_push / ry_synth_flush on a lone handle
// with its seed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ry355.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, ry_last_error()); ++failures; } } while (0)

static const int BINS = 513, B = 3;
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

struct Rig {
    ry_synth_bank* bank = nullptr;
    ry_synth* lone[B] = {};
    Frames track[B];
    int pos[B] = {};
};

// one bank push of n[b] frames (final[b]: the stream ends) against the lone handles, samples and pulses
static void push(Rig& r, const int* n, const int* fin) {
    Frames pack;
    long long cap = 0;
    for (int b = 0; b < B; ++b) {
        const Frames& t = r.track[b];
        pack.f0.insert(pack.f0.end(), t.f0.begin() + r.pos[b], t.f0.begin() + r.pos[b] + n[b]);
        pack.sp.insert(pack.sp.end(), t.sp.begin() + (size_t)r.pos[b] * BINS, t.sp.begin() + (size_t)(r.pos[b] + n[b]) * BINS);
        pack.ap.insert(pack.ap.end(), t.ap.begin() + (size_t)r.pos[b] * BINS, t.ap.begin() + (size_t)(r.pos[b] + n[b]) * BINS);
        if (n[b] > 0 || (fin && fin[b])) cap += ry_synth_bank_bound(r.bank, b, n[b], fin && fin[b]);
    }
    if (pack.f0.empty()) { pack.f0.resize(1); pack.sp.resize(BINS); pack.ap.resize(BINS); }      // a plain flush: nothing is read
    std::vector<double> y((size_t)cap + 3, MARK), y1((size_t)cap + 3);
    long long off[B + 1];
    EXPECT(ry_synth_bank_push(r.bank, pack.f0.data(), pack.sp.data(), pack.ap.data(), n, fin, BINS, 0, y.data(), cap, off) == 0);
    EXPECT(off[0] == 0 && off[B] <= cap && y[(size_t)cap] == MARK);
    int counts[4] = {-1, -1, -1, -1};
    EXPECT(ry_synth_bank_debug_counts(r.bank, counts) == 0 && counts[0] >= 2 && counts[1] >= 3 && counts[1] <= 5);
    for (int b = 0; b < B; ++b) {
        const Frames& t = r.track[b];
        int got = 0, total = 0;
        std::vector<long long> ix1; std::vector<double> sh1; std::vector<int> vo1;
        for (int part = 0; part < 2; ++part) {
            int k = 0, np = 0;
            if (part == 0 && n[b] > 0)
                EXPECT(ry_synth_push(r.lone[b], t.f0.data() + r.pos[b], t.sp.data() + (size_t)r.pos[b] * BINS, t.ap.data() + (size_t)r.pos[b] * BINS, n[b], BINS, 0,
                                     y1.data() + total, (int)cap - total, &k) == 0);
            else if (part == 1 && fin && fin[b])
                EXPECT(ry_synth_flush(r.lone[b], y1.data() + total, (int)cap - total, &k) == 0);
            else
                continue;
            total += k;
            EXPECT(ry_synth_debug_pulses(r.lone[b], nullptr, nullptr, nullptr, 0, &np) == 0);
            const size_t at = ix1.size();
            ix1.resize(at + (size_t)np + 1); sh1.resize(at + (size_t)np + 1); vo1.resize(at + (size_t)np + 1);
            EXPECT(ry_synth_debug_pulses(r.lone[b], ix1.data() + at, sh1.data() + at, vo1.data() + at, np, &np) == 0);
            ix1.resize(at + (size_t)np); sh1.resize(at + (size_t)np); vo1.resize(at + (size_t)np);
        }
        got = (int)(off[b + 1] - off[b]);
        EXPECT(got == total);
        EXPECT(std::memcmp(y.data() + off[b], y1.data(), (size_t)total * sizeof(double)) == 0);
        int np = -1;
        EXPECT(ry_synth_bank_debug_pulses(r.bank, b, nullptr, nullptr, nullptr, 0, &np) == 0 && np == (int)ix1.size());
        std::vector<long long> ix((size_t)np + 1); std::vector<double> sh((size_t)np + 1); std::vector<int> vo((size_t)np + 1);
        EXPECT(ry_synth_bank_debug_pulses(r.bank, b, ix.data(), sh.data(), vo.data(), np, &np) == 0);
        EXPECT(np == 0 || (size_t)np != ix1.size() ||
               (std::memcmp(ix.data(), ix1.data(), (size_t)np * sizeof(long long)) == 0 && std::memcmp(sh.data(), sh1.data(), (size_t)np * sizeof(double)) == 0 &&
               std::memcmp(vo.data(), vo1.data(), (size_t)np * sizeof(int)) == 0));
        if (np > 0) EXPECT(ry_synth_bank_debug_pulses(r.bank, b, ix.data(), nullptr, nullptr, np - 1, &np) == -1);
        r.pos[b] += n[b];
        if (fin && fin[b]) r.pos[b] = 0;                                                         // the slot starts again, from the top of its track
        EXPECT(ry_synth_bank_debug_rows(r.bank, b) >= 0);
    }
}

int main() {
    ry_ctx* ctx = nullptr;
    EXPECT(ry_init(0, &ctx) == 0);
    Rig r;
    const unsigned seeds[B] = {3, 4, 5};
    ry_synth_bank *slow = nullptr, *idle = nullptr, *none = nullptr;
    EXPECT(ry_synth_bank_create(ctx, 16000, 5.0, 1024, B, seeds, &r.bank) == 0);
    EXPECT(ry_synth_bank_create(ctx, 48000, 1000.0, 1024, 2, seeds, &slow) == 0);
    EXPECT(ry_synth_bank_create(ctx, 24000, 5.0, 1024, 1, seeds, &idle) == 0);
    EXPECT(ry_synth_bank_create(ctx, 16000, 5.0, 1024, 0, seeds, &none) == -1 && none == nullptr);
    EXPECT(ry_synth_bank_create(ctx, 16000, 5.0, 1024, 2, nullptr, &none) == -1);
    EXPECT(ry_synth_bank_create(ctx, 7000, 5.0, 1024, 2, seeds, &none) == -1);
    EXPECT(ry_synth_bank_create(ctx, 16000, 5.0, 512, 2, seeds, &none) == -1);
    EXPECT(ry_synth_bank_create(ctx, 16000, 5.0, 1024, 2, seeds, nullptr) == -1);
    for (int b = 0; b < B; ++b) {
        EXPECT(ry_synth_create(ctx, 16000, 5.0, 1024, seeds[b], &r.lone[b]) == 0);
        r.track[b] = frames(200, b + 1);
    }
    int np = -1;
    EXPECT(ry_synth_bank_debug_pulses(r.bank, 0, nullptr, nullptr, nullptr, 0, &np) == -4 && np == 0);      // no push yet

    // ragged pushes, a stream that sits out, growth (a large push after small ones, small ones again), poison between calls
    const int c1[B] = {9, 0, 1}, c2[B] = {3, 12, 2}, c3[B] = {60, 1, 40}, c4[B] = {2, 2, 0};
    push(r, c1, nullptr);
    push(r, c2, nullptr);
    EXPECT(ry_synth_bank_debug_poison(r.bank) == 0);
    EXPECT(ry_synth_bank_debug_pulses(r.bank, 0, nullptr, nullptr, nullptr, 0, &np) == -4);
    push(r, c3, nullptr);
    EXPECT(ry_synth_bank_debug_poison(r.bank) == 0);
    push(r, c4, nullptr);
    // stream 1 ends with frames while 0 and 2 go on; its slot starts again; stream 0 ends without frames
    const int f1[B] = {0, 1, 0}, c5[B] = {4, 5, 6}, f2[B] = {1, 0, 0}, c0[B] = {0, 0, 0};
    push(r, c2, f1);
    EXPECT(ry_synth_bank_bound(r.bank, 1, 0, 1) == 0);
    push(r, c5, nullptr);
    push(r, c0, f2);

    // the refusals: nothing is written, and the bank goes on
    std::vector<double> y(6000, MARK);
    long long off[B + 1] = {-99, -99, -99, -99};
    const Frames& t = r.track[0];
    const double* F = t.f0.data();
    const float *S = t.sp.data(), *A = t.ap.data();
    const int n3[B] = {3, 4, 2};
    EXPECT(ry_synth_bank_push(nullptr, F, S, A, n3, nullptr, BINS, 0, y.data(), 6000, off) == -4);
    EXPECT(ry_synth_bank_push(r.bank, nullptr, S, A, n3, nullptr, BINS, 0, y.data(), 6000, off) == -1);
    EXPECT(ry_synth_bank_push(r.bank, F, nullptr, A, n3, nullptr, BINS, 0, y.data(), 6000, off) == -1);
    EXPECT(ry_synth_bank_push(r.bank, F, S, nullptr, n3, nullptr, BINS, 0, y.data(), 6000, off) == -1);
    EXPECT(ry_synth_bank_push(r.bank, F, S, A, nullptr, nullptr, BINS, 0, y.data(), 6000, off) == -1);
    EXPECT(ry_synth_bank_push(r.bank, F, S, A, n3, nullptr, BINS, 0, nullptr, 6000, off) == -1);
    EXPECT(ry_synth_bank_push(r.bank, F, S, A, n3, nullptr, BINS, 0, y.data(), 6000, nullptr) == -1);
    EXPECT(ry_synth_bank_push(r.bank, F, S, A, n3, nullptr, 512, 0, y.data(), 6000, off) == -1);
    const int neg[B] = {3, -1, 2}, over[B] = {1 << 22, 1, 0}, wide[2] = {12000, 12000};
    EXPECT(ry_synth_bank_push(r.bank, F, S, A, neg, nullptr, BINS, 0, y.data(), 6000, off) == -1);
    EXPECT(ry_synth_bank_push(r.bank, F, S, A, c0, nullptr, BINS, 0, y.data(), 6000, off) == -1);
    EXPECT(ry_synth_bank_push(r.bank, F, S, A, over, nullptr, BINS, 0, y.data(), 6000, off) == -1 && std::strstr(ry_last_error(), "frames") != nullptr);
    EXPECT(ry_synth_bank_push(slow, F, S, A, wide, nullptr, BINS, 0, y.data(), 1LL << 40, off) == -1 && std::strstr(ry_last_error(), "samples") != nullptr);
    const int e1[1] = {1};
    EXPECT(ry_synth_bank_push(idle, F, S, A, c0, e1, BINS, 0, y.data(), 6000, off) == -4);       // final on an empty stream
    Frames bad = t;
    bad.f0[3 + 4 + 1] = std::numeric_limits<double>::quiet_NaN();                                // stream 2, frame 1
    EXPECT(ry_synth_bank_push(r.bank, bad.f0.data(), S, A, n3, nullptr, BINS, 0, y.data(), 6000, off) == -1 && std::strstr(ry_last_error(), "stream 2: f0[1]") != nullptr);
    long long need = 0;
    for (int b = 0; b < B; ++b) need += ry_synth_bank_bound(r.bank, b, n3[b], 0);
    EXPECT(need > 0 && ry_synth_bank_push(r.bank, F, S, A, n3, nullptr, BINS, 0, y.data(), need - 1, off) == -1 && std::strstr(ry_last_error(), "y holds") != nullptr);
    bool clean = true;
    for (double v : y) clean = clean && v == MARK;
    for (long long v : off) clean = clean && v == -99;
    EXPECT(clean);
    push(r, n3, nullptr);                                                                        // the same counts, accepted: still the lone handles' bits
    EXPECT(ry_synth_bank_reset(r.bank, 3) == -1 && ry_synth_bank_reset(r.bank, 1) == 0 && ry_synth_reset(r.lone[1]) == 0);
    r.pos[1] = 0;
    push(r, c5, nullptr);
    EXPECT(ry_synth_bank_reset(r.bank, -1) == 0);
    EXPECT(ry_synth_bank_bound(r.bank, 0, 0, 1) == 0 && ry_synth_bank_debug_rows(r.bank, 3) < 0);
    ry_synth_bank_destroy(r.bank);                                                               // destroyed after pushes ...
    ry_synth_bank_destroy(slow);
    ry_synth_bank_destroy(idle);                                                                 // ... and without one
    ry_synth_bank_destroy(nullptr);
    for (int b = 0; b < B; ++b) ry_synth_destroy(r.lone[b]);
    ry_shutdown(ctx);
    std::printf(failures ? "%d checks failed\n" : "synth_bank_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
