// filter_build_host_check.cpp -- the host paths of the filter build modes (ry_set_filter_build, ry_net_build_stats, ry_net_debug_filters,
// ry_debug_layer_filters) in a stand-alone program over the emulator build of libry355, meant to be compiled and linked with
// -fsanitize=address,undefined (scripts/asan_filter_build.sh): create and destroy in both modes, every layout of both predictors compared between
// the modes, the lazy Winograd build, clones made before and after it, the staging buffer growing and being reused over layers of rising and falling
// size (a U-Net's filters rise to the bottom and fall again; single layers in an order of their own), a mode switch between two live predictors,
// and every refusal.  Exit status 0: every call returned what it should and every layout has the same bits in both modes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ry355.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, ry_last_error()); ++failures; } } while (0)

static std::vector<float> blob(size_t n, unsigned seed) {
    std::vector<float> w(n);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; w[i] = ((float)(s >> 8) / 8388608.f - 1.f) * 0.1f; }
    return w;
}

static ry_net* make(ry_ctx* ctx, const ry_net_desc& d, const std::vector<float>& w) {
    ry_net* net = nullptr;
    EXPECT(ry_net_create(ctx, &d, w.data(), w.size(), 0, &net) == 0 && net);
    return net;
}

// every layout of the predictor: -> floats fetched; `all` gets them back to back
static size_t layouts(ry_net* net, std::vector<float>& all) {
    all.clear();
    for (int layer = 0; layer < 16; ++layer)
        for (int kind = 0; kind < 6; ++kind) {
            size_t n = 0;
            const int rc = ry_net_debug_filters(net, layer, kind, nullptr, 0, &n);
            if (rc == -4) { EXPECT(n == 0); continue; }
            EXPECT(rc == -1 && n > 0);
            const size_t at = all.size();
            all.resize(at + n);
            EXPECT(ry_net_debug_filters(net, layer, kind, all.data() + at, n, &n) == 0);
        }
    return all.size();
}

static void refusals(ry_ctx* ctx, ry_net* net) {
    EXPECT(ry_set_filter_build(-1) == -1 && ry_set_filter_build(2) == -1);
    ry_build_stats st;
    EXPECT(ry_net_build_stats(nullptr, &st) == -1 && ry_net_build_stats(net, nullptr) == -1);
    float out[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    size_t n = 77;
    EXPECT(ry_net_debug_filters(nullptr, 0, 0, out, 8, &n) == -1 && ry_net_debug_filters(net, 0, 0, out, 8, nullptr) == -1);
    EXPECT(ry_net_debug_filters(net, -1, 0, out, 8, &n) == -1 && ry_net_debug_filters(net, 16, 0, out, 8, &n) == -1);
    EXPECT(ry_net_debug_filters(net, 0, -1, out, 8, &n) == -1 && ry_net_debug_filters(net, 0, 6, out, 8, &n) == -1 && n == 77);
    EXPECT(ry_net_debug_filters(net, 0, 0, out, 8, &n) == -4 && n == 77);           // a stage-2 layer has no stage-1 layout
    EXPECT(ry_net_debug_filters(net, 0, 5, out, 8, &n) == -4 && n == 77);           // ... and the first layer no Winograd form
    EXPECT(ry_net_debug_filters(net, 0, 3, out, 8, &n) == -1 && n > 8);             // short buffer: the size comes back, nothing is written
    for (float v : out) EXPECT(v == 1.f);
    const float w[4 * 4 * 4] = {0};
    EXPECT(ry_debug_layer_filters(nullptr, 1, 4, 0, 4, 4, 2, 1, 0, 0, w, 0, out, 8, &n) == -1);
    EXPECT(ry_debug_layer_filters(ctx, 3, 4, 0, 4, 4, 2, 1, 0, 0, w, 0, out, 8, &n) == -1);
    EXPECT(ry_debug_layer_filters(ctx, 1, 4, 0, 4, 3, 1, 1, 1, 0, w, 0, out, 8, &n) == -1);      // transposed k3
    EXPECT(ry_debug_layer_filters(ctx, 1, 4, 0, 4, 4, 2, 1, 0, 0, w, 3, out, 8, &n) == -4);      // a 1-D layer has no direct layout
    EXPECT(ry_debug_layer_filters(ctx, 1, 4, 0, 4, 4, 2, 1, 0, 0, w, 0, out, 8, &n) == -1 && n == 64);
    for (float v : out) EXPECT(v == 1.f);
    setenv("RY_FILTER_BUILD", "card", 1);
    EXPECT(ry_debug_reload_env() == -1);
    unsetenv("RY_FILTER_BUILD");
    EXPECT(ry_debug_reload_env() == 0);
}

int main() {
    setenv("RY_POISON", "1", 1);
    setenv("RY_WINO_MINM", "1", 1);
    setenv("RY_OS2_MINW", "1", 1);
    ry_ctx* ctx = nullptr;
    EXPECT(ry_init(0, &ctx) == 0 && ctx);
    if (!ctx) return 1;
    ry_net_desc d1 = {1, 5, 3, 16, 3, 1, 0.f, 0.2f, 0}, d2 = {2, 1, 1, 64, 3, 64, 0.f, 0.2f, 0};
    const std::vector<float> w1 = blob(ry_net_param_count(&d1), 1), w2 = blob(ry_net_param_count(&d2), 2);
    EXPECT(!w1.empty() && !w2.empty());

    // create / destroy in both modes, twice over (the staging buffer is made, grown over the rising filters, reused over the falling ones, dropped)
    for (int round = 0; round < 2; ++round)
        for (int mode = 0; mode < 2; ++mode) {
            EXPECT(ry_set_filter_build(mode) == 0);
            ry_net* a = make(ctx, d1, w1); ry_net* b = make(ctx, d2, w2);
            ry_build_stats st;
            EXPECT(ry_net_build_stats(b, &st) == 0 && (st.layout_launches > 0) == (mode == 1) && (st.host_relayout_floats > 0) == (mode == 0));
            ry_net_destroy(a); ry_net_destroy(b);
        }

    // a predictor of each mode alive across the switch; all layouts equal; the lazy Winograd build in each mode; clones before and after it
    EXPECT(ry_set_filter_build(0) == 0);
    ry_net* host1 = make(ctx, d1, w1); ry_net* host2 = make(ctx, d2, w2);
    EXPECT(ry_set_filter_build(1) == 0);
    ry_net* dev1 = make(ctx, d1, w1); ry_net* dev2 = make(ctx, d2, w2);
    ry_net *early = nullptr, *late = nullptr;
    EXPECT(ry_net_clone(dev2, &early) == 0 && early);
    const int n = 70, bins = 65;
    std::vector<float> sp((size_t)n * bins), yh(sp.size()), yd(sp.size()), ye(sp.size()), yl(sp.size());
    for (size_t i = 0; i < sp.size(); ++i) sp[i] = 0.001f + 0.0001f * (float)(i % 97);
    EXPECT(ry_set_filter_build(0) == 0);
    EXPECT(ry_sr_convert(host2, sp.data(), yh.data(), 1, n, 0) == 0);
    EXPECT(ry_set_filter_build(1) == 0);
    ry_build_stats s0, s1, s2;
    EXPECT(ry_net_build_stats(dev2, &s0) == 0);
    EXPECT(ry_sr_convert(dev2, sp.data(), yd.data(), 1, n, 0) == 0);
    EXPECT(ry_net_clone(dev2, &late) == 0 && late);
    EXPECT(ry_sr_convert(early, sp.data(), ye.data(), 1, n, 0) == 0 && ry_sr_convert(late, sp.data(), yl.data(), 1, n, 0) == 0);
    EXPECT(ry_net_build_stats(early, &s1) == 0 && ry_net_build_stats(late, &s2) == 0);
    EXPECT(s1.layout_launches > s0.layout_launches && s1.bytes_downloaded == 0 && std::memcmp(&s1, &s2, sizeof s1) == 0);
    EXPECT(std::memcmp(yh.data(), yd.data(), yh.size() * 4) == 0 && std::memcmp(yh.data(), ye.data(), yh.size() * 4) == 0 &&
           std::memcmp(yh.data(), yl.data(), yh.size() * 4) == 0);
    std::vector<float> a, b;
    EXPECT(ry_set_filter_build(0) == 0);
    const size_t nh1 = layouts(host1, a), nh2 = layouts(host2, b);
    std::vector<float> c, e;
    EXPECT(ry_set_filter_build(1) == 0);
    EXPECT(layouts(dev1, c) == nh1 && nh1 > 0 && std::memcmp(a.data(), c.data(), nh1 * 4) == 0);
    EXPECT(layouts(dev2, e) == nh2 && nh2 > 0 && std::memcmp(b.data(), e.data(), nh2 * 4) == 0);
    ry_build_stats sh, sd;
    EXPECT(ry_net_build_stats(host2, &sh) == 0 && ry_net_build_stats(dev2, &sd) == 0 && sh.arena_bytes == sd.arena_bytes && sh.bytes_downloaded > 0);
    refusals(ctx, dev2);

    // single layers in an order of their own: small, large, small (the staging buffer of each call grows from nothing and goes back)
    const int shapes[3][2] = {{16, 64}, {256, 64}, {32, 128}};
    for (int mode = 0; mode < 2; ++mode)
        for (const int* s : shapes) {
            EXPECT(ry_set_filter_build(mode) == 0);
            const std::vector<float> w = blob((size_t)s[0] * s[1] * 16, 9);
            for (int kind = 2; kind < 6; ++kind) {
                size_t nf = 0;
                const int rc = ry_debug_layer_filters(ctx, 2, s[0], 0, s[1], 4, 2, 1, 0, 1, w.data(), kind, nullptr, 0, &nf);
                if (rc == -4) continue;
                std::vector<float> out(nf);
                EXPECT(rc == -1 && nf > 0 && ry_debug_layer_filters(ctx, 2, s[0], 0, s[1], 4, 2, 1, 0, 1, w.data(), kind, out.data(), nf, &nf) == 0);
            }
        }
    EXPECT(ry_set_filter_build(0) == 0);
    ry_net_destroy(late); ry_net_destroy(early);
    ry_net_destroy(host1); ry_net_destroy(host2); ry_net_destroy(dev1); ry_net_destroy(dev2);
    ry_shutdown(ctx);
    std::printf(failures ? "filter_build_host_check: %d FAILED\n" : "filter_build_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
