// output_gate_host_check.cpp -- the host paths of the output gate (ry_outgate_*, ry_outgate_bank_*) in a stand-alone program over the emulator build
// of libry355, meant to be compiled and linked with -fsanitize=address,undefined (scripts/asan_output_gate.sh): create, pushes that complete no
// chunk, one chunk, a backlog drained by empty pushes, buffer growth from small pushes to a large one and back, float32 output, a bank with ragged
// pushes, streams that sit out and a reset, every refusal with the outputs watched and a valid push after it, poison between calls, the debug
// calls, destroy.  Exit status 0: every call returned what it should and every stream of the bank equals a lone gate fed the same samples.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ry355.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, ry_last_error()); ++failures; } } while (0)

static const int CHUNK = 1536, B = 3;
static const double MARK = -7.25;

static std::vector<double> signal(int n, int kind) {
    std::vector<double> x((size_t)n);
    unsigned s = 12345u + (unsigned)kind;
    for (int i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        const double u = (double)(s >> 8) / 16777216.0 - 0.5;
        x[(size_t)i] = kind == 1 ? 1e-6 * u : 0.2 * std::sin(0.04 * i + kind) + 1e-3 * u;      // kind 1: silent at 80 dB
    }
    return x;
}

int main() {
    ry_ctx* ctx = nullptr;
    EXPECT(ry_init(0, &ctx) == 0);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    ry_outgate *g = nullptr, *g32 = nullptr, *none = nullptr;
    EXPECT(ry_outgate_create(ctx, 1024, 80.0, 1.0, 0, &none) == -1 && none == nullptr);
    EXPECT(ry_outgate_create(ctx, CHUNK, nan, 1.0, 0, &none) == -1);
    EXPECT(ry_outgate_create(ctx, CHUNK, 80.0, nan, 0, &none) == -1);
    EXPECT(ry_outgate_create(nullptr, CHUNK, 80.0, 1.0, 0, &none) == -1);
    EXPECT(ry_outgate_create(ctx, CHUNK, 80.0, 1.0, 0, nullptr) == -1);
    EXPECT(ry_outgate_create(ctx, CHUNK, 80.0, 0.5, 0, &g) == 0);
    EXPECT(ry_outgate_create(ctx, CHUNK, 80.0, 0.5, 1, &g32) == 0);

    std::vector<double> out((size_t)CHUNK + 1, MARK);
    std::vector<float> out32((size_t)CHUNK + 1, (float)MARK);
    int n_out = -1, silent = -1;
    double mean = 0;
    const std::vector<double> loud = signal(5 * CHUNK, 0), quiet = signal(2 * CHUNK, 1);
    // no chunk, then one; a backlog (3.5 chunks at once) drained by empty pushes; growth and back
    EXPECT(ry_outgate_push(g, loud.data(), 100, 0, out.data(), CHUNK, &n_out, &silent, &mean) == 0 && n_out == 0 && ry_outgate_held(g) == 100);
    EXPECT(out[0] == MARK);
    EXPECT(ry_outgate_push(g, loud.data() + 100, CHUNK - 100, 0, out.data(), CHUNK, &n_out, &silent, &mean) == 0 && n_out == CHUNK && silent == 0);
    EXPECT(out[0] == loud[0] * 0.5 && out[(size_t)CHUNK - 1] == loud[(size_t)CHUNK - 1] * 0.5 && out[(size_t)CHUNK] == MARK && mean > -80.0);
    EXPECT(ry_outgate_debug_poison(g) == 0);
    EXPECT(ry_outgate_push(g, loud.data(), 3 * CHUNK + CHUNK / 2, 0, out.data(), CHUNK, &n_out, &silent, &mean) == 0 && n_out == CHUNK);
    for (int i = 0; i < 2; ++i) {
        EXPECT(ry_outgate_debug_poison(g) == 0);
        EXPECT(ry_outgate_push(g, nullptr, 0, 0, out.data(), CHUNK, &n_out, &silent, &mean) == 0 && n_out == CHUNK);
        EXPECT(out[0] == loud[(size_t)(i + 1) * CHUNK] * 0.5);
    }
    EXPECT(ry_outgate_held(g) == CHUNK / 2);
    EXPECT(ry_outgate_push(g, nullptr, 0, 0, out.data(), CHUNK, &n_out, &silent, &mean) == 0 && n_out == 0);
    long long counts[5] = {-1, -1, -1, -1, -1};
    EXPECT(ry_outgate_debug_counts(g, counts) == 0 && counts[1] == 1 && counts[4] == 0);
    EXPECT(ry_outgate_reset(g) == 0 && ry_outgate_held(g) == 0);
    // a silent chunk leaves out alone; float32
    std::fill(out.begin(), out.end(), MARK);
    EXPECT(ry_outgate_push(g, quiet.data(), CHUNK, 0, out.data(), CHUNK, &n_out, &silent, &mean) == 0 && n_out == CHUNK && silent == 1 && mean < -80.0);
    EXPECT(out[0] == MARK && out[(size_t)CHUNK - 1] == MARK);
    EXPECT(ry_outgate_debug_counts(g, counts) == 0 && counts[4] == 0);
    EXPECT(ry_outgate_push(g32, loud.data(), CHUNK, 0, out32.data(), CHUNK, &n_out, &silent, &mean) == 0 && n_out == CHUNK && silent == 0);
    EXPECT(out32[1] == (float)(loud[1] * 0.5) && out32[(size_t)CHUNK] == (float)MARK);
    // NaN scrubbed, inf: audible with a NaN mean
    std::vector<double> odd(quiet.begin(), quiet.begin() + CHUNK);
    odd[5] = nan; odd[700] = std::numeric_limits<double>::infinity();
    EXPECT(ry_outgate_push(g, odd.data(), CHUNK, 0, out.data(), CHUNK, &n_out, &silent, &mean) == 0 && n_out == CHUNK && silent == 0 && mean != mean);
    EXPECT(out[5] == 0.0 && std::isinf(out[700]));
    // refusals: nothing written, state as it was
    EXPECT(ry_outgate_push(g, quiet.data(), 10, 0, out.data(), CHUNK, &n_out, &silent, &mean) == 0 && ry_outgate_held(g) == 10);
    std::fill(out.begin(), out.end(), MARK);
    EXPECT(ry_outgate_push(nullptr, quiet.data(), 10, 0, out.data(), CHUNK, &n_out, &silent, &mean) == -4);
    EXPECT(ry_outgate_push(g, nullptr, 10, 0, out.data(), CHUNK, &n_out, &silent, &mean) == -1);
    EXPECT(ry_outgate_push(g, quiet.data(), -1, 0, out.data(), CHUNK, &n_out, &silent, &mean) == -1);
    EXPECT(ry_outgate_push(g, quiet.data(), 10, 0, nullptr, CHUNK, &n_out, &silent, &mean) == -1);
    EXPECT(ry_outgate_push(g, quiet.data(), 10, 0, out.data(), CHUNK, nullptr, &silent, &mean) == -1);
    EXPECT(ry_outgate_push(g, quiet.data(), 10, 0, out.data(), CHUNK, &n_out, nullptr, &mean) == -1);
    EXPECT(ry_outgate_push(g, quiet.data(), 10, 0, out.data(), CHUNK, &n_out, &silent, nullptr) == -1);
    EXPECT(ry_outgate_push(g, loud.data(), CHUNK, 0, out.data(), CHUNK - 1, &n_out, &silent, &mean) == -1 && std::strstr(ry_last_error(), "out holds") != nullptr);
    EXPECT(ry_outgate_held(g) == 10 && out[0] == MARK);
    EXPECT(ry_outgate_held(nullptr) < 0 && ry_outgate_reset(nullptr) == -4 && ry_outgate_debug_counts(g, nullptr) == -1 && ry_outgate_debug_poison(nullptr) == -4);
    EXPECT(ry_outgate_reset(g) == 0);

    // the bank against lone gates: ragged pushes, streams that sit out, a reset, poison between calls
    ry_outgate_bank *k = nullptr, *nobank = nullptr;
    ry_outgate* lone[B] = {};
    EXPECT(ry_outgate_bank_create(ctx, 0, CHUNK, 80.0, 0.5, 0, &nobank) == -1 && nobank == nullptr);
    EXPECT(ry_outgate_bank_create(ctx, B, 1000, 80.0, 0.5, 0, &nobank) == -1);
    EXPECT(ry_outgate_bank_create(ctx, B, CHUNK, 80.0, 0.5, 0, nullptr) == -1);
    EXPECT(ry_outgate_bank_create(ctx, B, CHUNK, 80.0, 0.5, 0, &k) == 0);
    std::vector<double> track[B];
    int pos[B] = {};
    for (int b = 0; b < B; ++b) {
        EXPECT(ry_outgate_create(ctx, CHUNK, 80.0, 0.5, 0, &lone[b]) == 0);
        track[b] = signal(6 * CHUNK, b);                                                          // stream 1 is silent
    }
    const int calls[][B] = {{700, 0, 1536}, {900, 1536, 1}, {0, 0, 3000}, {5000, 100, 0}, {1, 1436, 36}, {1536, 1536, 1536}};
    for (size_t c = 0; c < sizeof calls / sizeof calls[0]; ++c) {
        if (c == 3) { EXPECT(ry_outgate_bank_reset(k, 2) == 0 && ry_outgate_reset(lone[2]) == 0); }
        EXPECT(ry_outgate_bank_debug_poison(k) == 0);
        std::vector<double> pack;
        long long off[B + 1] = {0}, oo[B + 1] = {-99, -99, -99, -99};
        for (int b = 0; b < B; ++b) {
            pack.insert(pack.end(), track[b].begin() + pos[b], track[b].begin() + pos[b] + calls[c][b]);
            off[b + 1] = off[b] + calls[c][b];
        }
        std::vector<double> y((size_t)B * CHUNK + 1, MARK), y1((size_t)CHUNK, MARK);
        int sil[B] = {-9, -9, -9};
        double m[B] = {};
        EXPECT(ry_outgate_bank_push(k, pack.data(), off, 0, y.data(), (long long)B * CHUNK, oo, sil, m) == 0);
        EXPECT(oo[0] == 0 && y[(size_t)B * CHUNK] == MARK);
        EXPECT(ry_outgate_bank_debug_counts(k, counts) == 0 && counts[1] <= 4 && counts[2] == 1);
        for (int b = 0; b < B; ++b) {
            if (calls[c][b] == 0) { EXPECT(sil[b] == -1 && oo[b + 1] == oo[b]); continue; }
            int n1 = -1, s1 = -1;
            double m1 = 0;
            EXPECT(ry_outgate_push(lone[b], track[b].data() + pos[b], calls[c][b], 0, y1.data(), CHUNK, &n1, &s1, &m1) == 0);
            pos[b] += calls[c][b];
            EXPECT(oo[b + 1] - oo[b] == n1 && (n1 == 0 ? sil[b] == -1 : sil[b] == s1));
            EXPECT(std::memcmp(&m[b], &m1, sizeof m1) == 0);
            if (n1 > 0 && s1 == 0) EXPECT(std::memcmp(y.data() + oo[b], y1.data(), (size_t)CHUNK * sizeof(double)) == 0);
            if (n1 > 0 && s1 == 1) EXPECT(y[(size_t)oo[b]] == MARK);
            EXPECT(ry_outgate_bank_held(k, b) == ry_outgate_held(lone[b]));
        }
    }
    // the bank's refusals
    {
        long long off[B + 1] = {0, 10, 20, 30}, bad[B + 1] = {0, 10, 5, 30}, bad0[B + 1] = {1, 10, 20, 30}, big[B + 1] = {0, 1536, 3072, 4608};
        long long oo[B + 1] = {-99, -99, -99, -99};
        int sil[B] = {-9, -9, -9};
        double m[B] = {};
        std::vector<double> y((size_t)B * CHUNK, MARK);
        const int held0 = ry_outgate_bank_held(k, 0);
        EXPECT(ry_outgate_bank_push(nullptr, loud.data(), off, 0, y.data(), (long long)B * CHUNK, oo, sil, m) == -4);
        EXPECT(ry_outgate_bank_push(k, nullptr, off, 0, y.data(), (long long)B * CHUNK, oo, sil, m) == -1);
        EXPECT(ry_outgate_bank_push(k, loud.data(), nullptr, 0, y.data(), (long long)B * CHUNK, oo, sil, m) == -1);
        EXPECT(ry_outgate_bank_push(k, loud.data(), off, 0, nullptr, (long long)B * CHUNK, oo, sil, m) == -1);
        EXPECT(ry_outgate_bank_push(k, loud.data(), off, 0, y.data(), (long long)B * CHUNK, nullptr, sil, m) == -1);
        EXPECT(ry_outgate_bank_push(k, loud.data(), off, 0, y.data(), (long long)B * CHUNK, oo, nullptr, m) == -1);
        EXPECT(ry_outgate_bank_push(k, loud.data(), off, 0, y.data(), (long long)B * CHUNK, oo, sil, nullptr) == -1);
        EXPECT(ry_outgate_bank_push(k, loud.data(), bad, 0, y.data(), (long long)B * CHUNK, oo, sil, m) == -1);
        EXPECT(ry_outgate_bank_push(k, loud.data(), bad0, 0, y.data(), (long long)B * CHUNK, oo, sil, m) == -1);
        EXPECT(ry_outgate_bank_push(k, loud.data(), big, 0, y.data(), (long long)B * CHUNK - 1, oo, sil, m) == -1 && std::strstr(ry_last_error(), "out holds") != nullptr);
        EXPECT(ry_outgate_bank_push(k, loud.data(), off, 0, y.data(), -1, oo, sil, m) == -1);
        EXPECT(ry_outgate_bank_reset(k, B) == -1 && ry_outgate_bank_held(k, B) < 0 && ry_outgate_bank_held(k, -1) < 0);
        EXPECT(oo[0] == -99 && sil[0] == -9 && y[0] == MARK && ry_outgate_bank_held(k, 0) == held0);
        EXPECT(ry_outgate_bank_push(k, loud.data(), big, 0, y.data(), (long long)B * CHUNK, oo, sil, m) == 0 && oo[B] == (long long)B * CHUNK);
        EXPECT(ry_outgate_bank_reset(k, -1) == 0 && ry_outgate_bank_held(k, 0) == 0);
    }
    ry_outgate_bank_destroy(k);
    ry_outgate_bank_destroy(nullptr);
    for (int b = 0; b < B; ++b) ry_outgate_destroy(lone[b]);
    ry_outgate_destroy(g);
    ry_outgate_destroy(g32);
    ry_outgate_destroy(nullptr);
    ry_shutdown(ctx);
    std::printf(failures ? "%d checks failed\n" : "output_gate_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
