// crepe_stream_host_check.cpp -- the host paths of the streaming tracker (ry_crepe_stream_*) in a stand-alone program over the emulator build of
// libry355, meant to be compiled and linked with -fsanitize=address,undefined (scripts/asan_crepe_stream.sh): every argument check, the building of
// the src / idx tables at both ends of the window (windows that keep rows, that grow, that shrink below a frame, advances at and past the window's
// end), the growth of the stream's blocks and tables, two streams on one model pushed alternately, the debug entries and destroy.
// Multiplier 1, hop 320 (a handful of frames per call).  Exit status 0: every call returned what it should, a window that kept rows has the track
// of ry_crepe_track on the same samples, and the counts of computed frames are those of the rule at 16 kHz.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ry355.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, ry_last_error()); ++failures; } } while (0)

static const int HOP = 320;

static std::vector<float> signal(int n, int seed) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 0.4f * std::sin(0.07f * (float)(i + 31 * seed)) + 0.05f * std::sin(1.3f * (float)i + (float)seed);
    return x;
}

// the rule at 16 kHz, restated: frame f is portable in n samples when [f hop - 512, f hop + 512) lies inside them
static bool portable(int f, int n) { return f * HOP - 512 >= 0 && f * HOP + 512 <= n; }

static int expect_computed(int n_old, int n_new, int advance, bool ok) {
    const int nf = 1 + n_new / HOP, nf_old = n_old > 0 ? 1 + n_old / HOP : 0;
    if (!ok || n_old < 1 || advance < 0 || advance >= n_old || advance % HOP) return nf;
    const int d = advance / HOP, m = n_new < n_old - advance ? n_new : n_old - advance;
    int kept = 0;
    for (int j = 0; j < nf; ++j)
        if (portable(j, m) && j + d < nf_old && portable(j + d, n_old)) ++kept;
    return nf - kept;
}

struct Track { std::vector<unsigned char> v; std::vector<double> f0, t; };

static bool same(const Track& a, const Track& b, int n) {
    return std::memcmp(a.v.data(), b.v.data(), (size_t)n) == 0 && std::memcmp(a.f0.data(), b.f0.data(), (size_t)n * 8) == 0 &&
           std::memcmp(a.t.data(), b.t.data(), (size_t)n * 8) == 0;
}

int main() {
    ry_ctx* ctx = nullptr;
    EXPECT(ry_init(0, &ctx) == 0);
    const size_t np = ry_crepe_param_count(1);
    std::vector<float> w(np);
    for (size_t i = 0; i < np; ++i) w[i] = 0.02f * std::sin(0.37f * (float)i) + 0.011f;
    // BatchNorm variances must be positive: the blob's running_var entries are sums of the above plus one
    ry_crepe *model = nullptr, *ref = nullptr;
    for (size_t i = 0; i < np; ++i) w[i] = std::fabs(w[i]) + 0.001f;
    EXPECT(ry_crepe_create(ctx, 1, w.data(), np, 1e-3f, &model) == 0);
    EXPECT(ry_crepe_create(ctx, 1, w.data(), np, 1e-3f, &ref) == 0);
    ry_crepe_stream *a = nullptr, *b = nullptr;
    EXPECT(ry_crepe_stream_create(nullptr, &a) == -4);
    EXPECT(ry_crepe_stream_create(model, nullptr) == -1);
    EXPECT(ry_crepe_stream_create(model, &a) == 0);
    EXPECT(ry_crepe_stream_create(model, &b) == 0);
    const int cap = 64;
    Track got, want;
    got.v.resize(cap); got.f0.resize(cap); got.t.resize(cap);
    want = got;
    int nf = -3, nc = -3, left = -3;
    std::vector<float> act((size_t)cap * 360);
    // before the first window
    EXPECT(ry_crepe_stream_activation(a, act.data(), 0) == -4);
    EXPECT(ry_crepe_stream_debug_poison(a, &left) == 0 && left == 0);
    EXPECT(ry_crepe_stream_debug_poison(a, nullptr) == -1);
    EXPECT(ry_crepe_stream_debug_poison(nullptr, &left) == -4);
    EXPECT(ry_crepe_stream_reset(nullptr) == -4);
    EXPECT(ry_crepe_stream_reset(a) == 0);
    // windows of two signals through two streams, alternately: (start, length, declared advance, overlap verified)
    const std::vector<float> sa = signal(12000, 1), sb = signal(12000, 2);
    const int plan[][4] = {{0, 2560, -1, 0},      // the first window: everything
                           {640, 2560, 640, 1},   // keeps rows
                           {1280, 3840, 640, 1},  // grows: the blocks and the tables grow with it
                           {1920, 1600, 640, 1},  // shrinks
                           {2560, 800, 640, 1},   // shorter than a frame: nothing is portable
                           {3200, 2560, 640, 1},  // ... and nothing was
                           {3840, 2560, 640, 0},  // the caller found another overlap
                           {4000, 2560, 160, 1},  // an advance off the hop
                           {6560, 2560, 2560, 1}, // an advance at the end of the window
                           {6560, 2560, 0, 1},    // no advance: the edges alone
                           {7200, 2560, 640, 1}};
    int n_old = 0;
    for (const int* p : plan) {
        const bool ok = p[3] != 0;
        const int want_c = expect_computed(n_old, p[1], p[2], ok);
        for (int which = 0; which < 2; ++which) {
            ry_crepe_stream* s = which ? b : a;
            const float* x = (which ? sb : sa).data() + p[0];
            EXPECT(ry_crepe_stream_debug_poison(s, &left) == 0);
            EXPECT(ry_crepe_stream_track(s, x, p[1], 16000, HOP, 20.0, 0.1, p[2], p[3], &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == 0);
            EXPECT(nf == 1 + p[1] / HOP && nc == want_c);
            int nf_ref = 0;
            EXPECT(ry_crepe_track(ref, x, p[1], 16000, HOP, 20.0, 0.1, &nf_ref, want.v.data(), want.f0.data(), want.t.data(), 0) == 0);
            EXPECT(nf_ref == nf && same(got, want, nf));
            EXPECT(ry_crepe_stream_activation(s, act.data(), 0) == 0);
            const float* dev = nullptr;
            int ns = 0, nfr = 0;
            EXPECT(ry_crepe_track_buffers(model, &dev, &ns, &nfr, nullptr, nullptr, nullptr) == 0 && ns == p[1] && nfr == nf);
        }
        n_old = p[1];
    }
    // refusals: nothing is written, the kept rows stay
    const float* x = sa.data() + 7840;
    std::memset(got.v.data(), 0xA5, got.v.size());
    nf = nc = -3;
    EXPECT(ry_crepe_stream_track(nullptr, x, 2560, 16000, HOP, 20.0, 0.1, 640, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == -4);
    EXPECT(ry_crepe_stream_track(a, nullptr, 2560, 16000, HOP, 20.0, 0.1, 640, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == -1);
    EXPECT(ry_crepe_stream_track(a, x, 0, 16000, HOP, 20.0, 0.1, 640, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == -1);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 22050, HOP, 20.0, 0.1, 640, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == -4);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 0, HOP, 20.0, 0.1, 640, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == -1);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, 0, 20.0, 0.1, 640, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == -1);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 0.0, 0.1, 640, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == -1);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, std::nan(""), 640, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == -1);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 640, 1, nullptr, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == -1);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 640, 1, &nf, nullptr, got.v.data(), got.f0.data(), got.t.data(), 0) == -1);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 640, 1, &nf, &nc, nullptr, got.f0.data(), got.t.data(), 0) == -1);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 640, 1, &nf, &nc, got.v.data(), nullptr, got.t.data(), 0) == -1);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 640, 1, &nf, &nc, got.v.data(), got.f0.data(), nullptr, 0) == -1);
    EXPECT(nf == -3 && nc == -3 && got.v[0] == 0xA5 && got.v[cap - 1] == 0xA5);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 640, 1, &nf, &nc, nullptr, nullptr, nullptr, 1) == 0);      // the track stays on the card
    EXPECT(nc == expect_computed(2560, 2560, 640, true) && nc < nf);
    // a switch of the arithmetic drops the rows; a reset does too
    EXPECT(ry_crepe_set_dtype(model, 2) == 0);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 0, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == 0 && nc == nf);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 0, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == 0 && nc < nf);
    EXPECT(ry_crepe_stream_reset(a) == 0);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 0, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == 0 && nc == nf);
    EXPECT(ry_crepe_set_dtype(model, 0) == 0);
    EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 0, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == 0 && nc == nf);
    // the assembling kernel alone: indices at and past both ends of either block, a guard row behind the destination
    {
        const int n_keep = 3, n_fresh = 2, n_rows = 6;
        std::vector<float> keep((size_t)n_keep * 360), fresh((size_t)n_fresh * 360), out((size_t)(n_rows + 1) * 360, -9.f), res(out.size());
        for (size_t i = 0; i < keep.size(); ++i) keep[i] = (float)i;
        for (size_t i = 0; i < fresh.size(); ++i) fresh[i] = -(float)i - 1.f;
        float *dk = nullptr, *df = nullptr, *dout = nullptr;
        EXPECT(ry_dev_alloc(ctx, keep.size(), &dk) == 0 && ry_dev_alloc(ctx, fresh.size(), &df) == 0 && ry_dev_alloc(ctx, out.size(), &dout) == 0);
        EXPECT(ry_dev_upload(ctx, dk, keep.data(), keep.size()) == 0 && ry_dev_upload(ctx, df, fresh.data(), fresh.size()) == 0);
        EXPECT(ry_dev_upload(ctx, dout, out.data(), out.size()) == 0);
        const int src[n_rows] = {0, n_keep - 1, n_keep, -1, -n_fresh, -n_fresh - 1};
        EXPECT(ry_crepe_stream_debug_assemble(a, dk, n_keep, df, n_fresh, src, n_rows, dout) == 0);
        EXPECT(ry_dev_download(ctx, res.data(), dout, res.size()) == 0);
        for (int j = 0; j <= n_rows; ++j) {
            const float* from = j == 0 ? keep.data() : j == 1 ? keep.data() + 2 * 360 : j == 3 ? fresh.data() : j == 4 ? fresh.data() + 360 : nullptr;
            for (int q = 0; q < 360; ++q) EXPECT(res[(size_t)j * 360 + q] == (from ? from[q] : -9.f));
        }
        EXPECT(ry_crepe_stream_debug_assemble(nullptr, dk, n_keep, df, n_fresh, src, n_rows, dout) == -4);
        EXPECT(ry_crepe_stream_debug_assemble(a, nullptr, n_keep, df, n_fresh, src, n_rows, dout) == -1);
        EXPECT(ry_crepe_stream_debug_assemble(a, dk, -1, df, n_fresh, src, n_rows, dout) == -1);
        EXPECT(ry_crepe_stream_debug_assemble(a, dk, n_keep, nullptr, n_fresh, src, n_rows, dout) == -1);
        EXPECT(ry_crepe_stream_debug_assemble(a, dk, n_keep, df, -1, src, n_rows, dout) == -1);
        EXPECT(ry_crepe_stream_debug_assemble(a, dk, n_keep, df, n_fresh, nullptr, n_rows, dout) == -1);
        EXPECT(ry_crepe_stream_debug_assemble(a, dk, n_keep, df, n_fresh, src, 0, dout) == -1);
        EXPECT(ry_crepe_stream_debug_assemble(a, dk, n_keep, df, n_fresh, src, n_rows, nullptr) == -1);
        // the tables on the card are no longer those of a call: the next window uploads its own
        EXPECT(ry_crepe_stream_track(a, x, 2560, 16000, HOP, 20.0, 0.1, 0, 1, &nf, &nc, got.v.data(), got.f0.data(), got.t.data(), 0) == 0 && nc < nf);
        int nf_ref = 0;
        EXPECT(ry_crepe_track(ref, x, 2560, 16000, HOP, 20.0, 0.1, &nf_ref, want.v.data(), want.f0.data(), want.t.data(), 0) == 0 && same(got, want, nf));
        EXPECT(ry_dev_free(ctx, dk) == 0 && ry_dev_free(ctx, df) == 0 && ry_dev_free(ctx, dout) == 0);
    }
    ry_crepe_stream_destroy(nullptr);
    ry_crepe_stream_destroy(b);
    ry_crepe_stream_destroy(a);
    ry_crepe_destroy(model);
    ry_crepe_destroy(ref);
    ry_shutdown(ctx);
    std::printf(failures ? "crepe_stream_host_check: %d FAILED\n" : "crepe_stream_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
