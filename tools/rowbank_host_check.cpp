// rowbank_host_check.cpp -- the host paths of the row bank (ry_rowbank_*) in a stand-alone program over the emulator build of libry355, meant to
// be compiled and linked with -fsanitize=address,undefined (scripts/asan_rowbank.sh): create and its refusals, appends of three streams until one
// stream's rings are full, retire of that stream alone and an append that wraps, fetch and pick with pads, empty spans and spans across the ring
// end into destinations at an odd 4-byte offset between guard words, tables that grow from one span to one per row, every refusal with a valid
// call after it, poison, reset of one stream and of all, destroy.  Exit status 0: every call returned what it should and every word fetched or
// picked is the word appended (or +0 where the plan pads or the mask cuts).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ry355.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, ry_last_error()); ++failures; } } while (0)

static const int B = 3, MC = 9, AP = 513, ROWS = 64, SAMPLES = 700;
static const int SEG_ROWS[B] = {21, 13, 30}, SEG_SAMPLES[B] = {230, 150, 330};
static const float GUARD = -7.25f;

// the value of element i of array `array` of segment `segment` of stream `stream`
static float value(int stream, int segment, int array, int i) { return (float)(stream * 4000000 + segment * 400000 + array * 100000 + i + 1); }

struct Dev {
    ry_ctx* ctx;
    float* p = nullptr;
    size_t n;
    Dev(ry_ctx* c, size_t n_) : ctx(c), n(n_) { if (ry_dev_alloc(ctx, n, &p) != 0) p = nullptr; }
    ~Dev() { if (p) ry_dev_free(ctx, p); }
    void up(const std::vector<float>& h) { EXPECT(ry_dev_upload(ctx, p, h.data(), h.size()) == 0); }
    std::vector<float> down() { std::vector<float> h(n); EXPECT(ry_dev_download(ctx, h.data(), p, n) == 0); return h; }
};

int main() {
    ry_ctx* ctx = nullptr;
    EXPECT(ry_init(0, &ctx) == 0);
    ry_rowbank *b = nullptr, *none = nullptr;
    EXPECT(ry_rowbank_create(ctx, 0, MC, AP, ROWS, SAMPLES, &none) == -1 && none == nullptr);
    EXPECT(ry_rowbank_create(ctx, 65537, MC, AP, ROWS, SAMPLES, &none) == -1);
    EXPECT(ry_rowbank_create(ctx, B, 0, AP, ROWS, SAMPLES, &none) == -1);
    EXPECT(ry_rowbank_create(ctx, B, MC, AP, 0, SAMPLES, &none) == -1);
    EXPECT(ry_rowbank_create(ctx, B, MC, AP, ROWS, 0, &none) == -1);
    EXPECT(ry_rowbank_create(ctx, 1 << 16, 256, 1, 1 << 22, 4, &none) == -1);              // 2^46 floats in the mc array
    EXPECT(ry_rowbank_create(nullptr, B, MC, AP, ROWS, SAMPLES, &none) == -1);
    EXPECT(ry_rowbank_create(ctx, B, MC, AP, ROWS, SAMPLES, nullptr) == -1);
    EXPECT(ry_rowbank_create(ctx, B, MC, AP, ROWS, SAMPLES, &b) == 0 && b != nullptr);
    EXPECT(ry_rowbank_debug_poison(b) == 0);

    // the shared source blocks: the three streams' segments behind one another, two rows / five samples of guard in front of each
    int row_at[B], sample_at[B], rows_total = 0, samples_total = 0;
    for (int s = 0; s < B; ++s) { row_at[s] = rows_total + 2; rows_total += SEG_ROWS[s] + 2; sample_at[s] = samples_total + 5; samples_total += SEG_SAMPLES[s] + 5; }
    Dev mc(ctx, (size_t)rows_total * MC), ap(ctx, (size_t)rows_total * AP), wave(ctx, (size_t)samples_total);
    int n_seg[B] = {0, 0, 0}, pos_r[B][8], pos_s[B][8];
    auto append = [&](std::vector<int> part, int want) {
        std::vector<float> h_mc(mc.n, GUARD), h_ap(ap.n, GUARD), h_w(wave.n, GUARD);
        std::vector<int> row0, n_rows, n_samples, rp(part.size(), -1), sp(part.size(), -1);
        std::vector<long long> sample0;
        for (int s : part) {
            for (int i = 0; i < SEG_ROWS[s] * MC; ++i) h_mc[(size_t)row_at[s] * MC + i] = value(s, n_seg[s], 0, i);
            for (int i = 0; i < SEG_ROWS[s] * AP; ++i) h_ap[(size_t)row_at[s] * AP + i] = value(s, n_seg[s], 1, i);
            for (int i = 0; i < SEG_SAMPLES[s]; ++i) h_w[(size_t)sample_at[s] + i] = value(s, n_seg[s], 2, i);
            row0.push_back(row_at[s]); n_rows.push_back(SEG_ROWS[s]); sample0.push_back(sample_at[s]); n_samples.push_back(SEG_SAMPLES[s]);
        }
        mc.up(h_mc); ap.up(h_ap); wave.up(h_w);
        const int rc = ry_rowbank_append(b, (int)part.size(), part.data(), mc.p, ap.p, row0.data(), n_rows.data(), wave.p, sample0.data(), n_samples.data(),
                                         rp.data(), sp.data());
        EXPECT(rc == want);
        for (size_t i = 0; i < part.size(); ++i) {
            if (rc == 0) { pos_r[part[i]][n_seg[part[i]]] = rp[i]; pos_s[part[i]][n_seg[part[i]]] = sp[i]; ++n_seg[part[i]]; }
            else EXPECT(rp[i] == -1 && sp[i] == -1);
        }
    };
    long long counts[4] = {0, 0, 0, 0};
    // grow: two calls of all three (nine pieces: the table goes up), then stream 2 is full (60 of 64 rows) and a call that names it is refused
    append({0, 1, 2}, 0);
    EXPECT(ry_rowbank_debug_counts(b, counts) == 0 && counts[0] == 1 && counts[1] == 1 && counts[2] == 1 && counts[3] > 0);
    append({0, 1, 2}, 0);
    int rows = -1, samples = -1;
    EXPECT(ry_rowbank_held(b, 2, &rows, &samples) == 0 && rows == 60 && samples == 660);
    append({0, 2}, -1);                                              // stream 0 would fit: nothing of it changes either
    EXPECT(ry_rowbank_held(b, 0, &rows, &samples) == 0 && rows == 42 && samples == 460 && n_seg[0] == 2);
    append({0, 1}, 0);                                               // six pieces, by value
    EXPECT(ry_rowbank_debug_counts(b, counts) == 0 && counts[0] == 1 && counts[1] == 0 && counts[2] == 0);
    // retire of stream 2 alone, then its append wraps in both rings
    EXPECT(ry_rowbank_retire(b, 2, SEG_ROWS[2], SEG_SAMPLES[2]) == 0 && ry_rowbank_retire(b, 2, 0, 0) == 0);
    EXPECT(ry_rowbank_retire(b, 2, 31, 0) == -1 && ry_rowbank_retire(b, 2, 0, 331) == -1 && ry_rowbank_retire(b, 2, -1, 0) == -1);
    EXPECT(ry_rowbank_retire(b, 3, 0, 0) == -1 && ry_rowbank_retire(b, -1, 0, 0) == -1 && ry_rowbank_retire(nullptr, 0, 0, 0) == -4);
    EXPECT(ry_rowbank_held(b, 0, &rows, &samples) == 0 && rows == 63 && samples == 690);
    append({2}, 0);
    EXPECT(pos_r[2][2] == 60 && pos_s[2][2] == 660);
    EXPECT(ry_rowbank_debug_poison(b) == 0);

    // fetch of streams 0 and 2: pad | segment 1 of stream 0 | empty | pad, then pad | segments 1, 2 of stream 2 (across the ring end) | pad
    const int part[] = {0, 2};
    const int w_rows[2] = {2 + 21 + 3, 1 + 30 + 30 + 2}, w_samples[2] = {4 + 230 + 1, 330 + 330 + 6};
    const int fo[] = {0, w_rows[0], w_rows[0] + w_rows[1]};
    const long long so[] = {0, w_samples[0], w_samples[0] + w_samples[1]};
    const int rs[] = {-1, 0, 2, pos_r[0][1], 2, 21, pos_r[0][2], 23, 0, -1, 23, 3,
                      -1, 0, 1, pos_r[2][1], 1, 30, pos_r[2][2], 31, 30, -1, 61, 2};
    const int ro[] = {0, 4, 8};
    const int ss[] = {-1, 0, 4, pos_s[0][1], 4, 230, -1, 234, 1,
                      pos_s[2][1], 0, 330, pos_s[2][2], 330, 330, -1, 660, 6};
    const int wo[] = {0, 3, 6};
    Dev d_mc(ctx, (size_t)fo[2] * MC + 9), d_w(ctx, (size_t)so[2] + 9), d_ap(ctx, (size_t)fo[2] * AP + 9);
    auto clear = [&]() { d_mc.up(std::vector<float>(d_mc.n, GUARD)); d_w.up(std::vector<float>(d_w.n, GUARD)); d_ap.up(std::vector<float>(d_ap.n, GUARD)); };
    clear();
    EXPECT(ry_rowbank_fetch(b, 2, part, rs, ro, ss, wo, d_mc.p + 1, d_w.p + 1, fo, so) == 0);
    EXPECT(ry_rowbank_debug_counts(b, counts) == 0 && counts[0] == 1 && counts[1] == 1 && counts[2] == 1 && counts[3] > 0);
    // row r of the window of entry e -> (stream, segment, row in it), or segment -1: a pad
    auto row_of = [&](int e, int r, int* seg, int* in) {
        *seg = -1; *in = 0;
        if (e == 0) { if (r >= 2 && r < 23) { *seg = 1; *in = r - 2; } }
        else if (r >= 1 && r < 31) { *seg = 1; *in = r - 1; }
        else if (r >= 31 && r < 61) { *seg = 2; *in = r - 31; }
    };
    {
        const std::vector<float> got = d_mc.down();
        EXPECT(got[0] == GUARD);
        for (size_t i = (size_t)fo[2] * MC + 1; i < got.size(); ++i) EXPECT(got[i] == GUARD);
        for (int e = 0; e < 2; ++e)
            for (int r = 0; r < w_rows[e]; ++r)
                for (int c = 0; c < MC; ++c) {
                    int seg, in;
                    row_of(e, r, &seg, &in);
                    const float want = seg < 0 ? 0.f : value(part[e], seg, 0, in * MC + c), v = got[(size_t)1 + (size_t)(fo[e] + r) * MC + c];
                    if (v != want) { EXPECT(v == want); e = 2; r = 1 << 20; break; }
                }
        const std::vector<float> w = d_w.down();
        EXPECT(w[0] == GUARD);
        for (size_t i = (size_t)so[2] + 1; i < w.size(); ++i) EXPECT(w[i] == GUARD);
        for (int i = 0; i < w_samples[0]; ++i) {
            const float want = i >= 4 && i < 234 ? value(0, 1, 2, i - 4) : 0.f;
            if (w[(size_t)1 + i] != want) { EXPECT(w[(size_t)1 + i] == want); break; }
        }
        for (int i = 0; i < w_samples[1]; ++i) {
            const float want = i < 330 ? value(2, 1, 2, i) : i < 660 ? value(2, 2, 2, i - 330) : 0.f;
            if (w[(size_t)1 + so[1] + i] != want) { EXPECT(w[(size_t)1 + so[1] + i] == want); break; }
        }
    }
    // pick: rows [1, 25) and [0, 62) of the two windows, the mask cut at the first and the last kept row and beside the pads and the ring end
    std::vector<unsigned char> h_mask((size_t)fo[2] + 3, 1);
    for (int r : {1, 2, 22, 24}) h_mask[(size_t)r] = 0;
    for (int r : {0, 1, 30, 31, 34, 35, 60, 61}) h_mask[(size_t)fo[1] + r] = 0;
    Dev d_mask(ctx, (h_mask.size() + 3) / 4 + 1);
    {
        std::vector<float> words(d_mask.n, 0.f);
        std::memcpy(words.data(), h_mask.data(), h_mask.size());
        d_mask.up(words);
    }
    const int keep[] = {1, 25, 0, 62};
    const int pack_rows = 24 + 62;
    EXPECT(ry_rowbank_pick_ap(b, 2, part, rs, ro, fo, keep, (const unsigned char*)d_mask.p, d_ap.p + 1, pack_rows) == 0);
    EXPECT(ry_rowbank_debug_counts(b, counts) == 0 && counts[0] == 1 && counts[1] == 1 && counts[2] == 1);
    {
        const std::vector<float> got = d_ap.down();
        EXPECT(got[0] == GUARD);
        for (size_t i = (size_t)pack_rows * AP + 1; i < got.size(); ++i) if (got[i] != GUARD) { EXPECT(got[i] == GUARD); break; }
        size_t at = 1;
        for (int e = 0; e < 2; ++e)
            for (int r = keep[2 * e]; r < keep[2 * e + 1]; ++r, at += AP)
                for (int c = 0; c < AP; ++c) {
                    int seg, in;
                    row_of(e, r, &seg, &in);
                    const bool cut = h_mask[(size_t)fo[e] + r] == 0;
                    const float want = seg < 0 || cut ? 0.f : value(part[e], seg, 1, in * AP + c), v = got[at + c];
                    if (v != want || (want == 0.f && std::signbit(v))) { EXPECT(v == want && !std::signbit(v)); e = 2; r = 1 << 20; break; }
                }
    }
    // the tables grow: one span, then one span per row
    const int one_part[] = {2}, one[] = {pos_r[2][1], 0, 1}, one_ro[] = {0, 1}, no_wo[] = {0, 0}, one_fo[] = {0, 61};
    const long long no_so[] = {0, 0};
    const int one_keep[] = {0, 1};
    EXPECT(ry_rowbank_fetch(b, 1, one_part, one, one_ro, nullptr, no_wo, d_mc.p, nullptr, one_fo, no_so) == 0);
    EXPECT(ry_rowbank_pick_ap(b, 1, one_part, one, one_ro, one_fo, one_keep, (const unsigned char*)d_mask.p, d_ap.p, 1) == 0);
    std::vector<int> many;
    for (int r = 0; r < 60; ++r) { many.push_back((pos_r[2][1] + r) % ROWS); many.push_back(r); many.push_back(1); }
    const int many_ro[] = {0, 60}, many_keep[] = {0, 60};
    EXPECT(ry_rowbank_fetch(b, 1, one_part, many.data(), many_ro, nullptr, no_wo, d_mc.p, nullptr, one_fo, no_so) == 0);
    EXPECT(d_mc.down()[(size_t)59 * MC] == value(2, 2, 0, 29 * MC));
    {
        std::vector<float> ones(d_mask.n, 0.f);
        std::memset(ones.data(), 1, ones.size() * sizeof(float));
        d_mask.up(ones);
    }
    EXPECT(ry_rowbank_pick_ap(b, 1, one_part, many.data(), many_ro, one_fo, many_keep, (const unsigned char*)d_mask.p, d_ap.p, 60) == 0);
    EXPECT(d_ap.down()[(size_t)59 * AP + 512] == value(2, 2, 1, 29 * AP + 512));
    // refusals: nothing is written, and a valid call works after each group
    clear();
    const int bad_count[] = {pos_r[2][1], 0, -1}, bad_dst[] = {pos_r[2][1], 60, 2}, bad_pos[] = {ROWS, 0, 1}, retired[] = {pos_r[2][0] + 27, 0, 1};      // (rows 0 .. 25 of the ring are live again)
    const int other[] = {(pos_r[2][2] + SEG_ROWS[2]) % ROWS, 0, 1};                          // live in stream 0, never written in stream 2
    for (const int* bad : {bad_count, bad_dst, bad_pos, retired, other}) {
        EXPECT(ry_rowbank_fetch(b, 1, one_part, bad, one_ro, nullptr, no_wo, d_mc.p, nullptr, one_fo, no_so) == -1);
        EXPECT(ry_rowbank_pick_ap(b, 1, one_part, bad, one_ro, one_fo, one_keep, (const unsigned char*)d_mask.p, d_ap.p, 1) == -1);
    }
    EXPECT(ry_rowbank_fetch(b, 1, one_part, one, one_ro, nullptr, no_wo, d_mc.p, nullptr, one_fo, no_so) == 0);
    const int twice[] = {2, 2}, down[] = {2, 0}, outside[] = {0, 3}, bad_ro[] = {1, 1}, bad_fo[] = {0, -1};
    const long long bad_so[] = {1, 1};
    for (const int* p : {twice, down, outside}) {
        EXPECT(ry_rowbank_fetch(b, 2, p, rs, ro, ss, wo, d_mc.p, d_w.p, fo, so) == -1);
        EXPECT(ry_rowbank_pick_ap(b, 2, p, rs, ro, fo, keep, (const unsigned char*)d_mask.p, d_ap.p, pack_rows) == -1);
    }
    EXPECT(ry_rowbank_fetch(b, 4, part, rs, ro, ss, wo, d_mc.p, d_w.p, fo, so) == -1);
    EXPECT(ry_rowbank_fetch(b, 1, one_part, one, bad_ro, nullptr, no_wo, d_mc.p, nullptr, one_fo, no_so) == -1);
    EXPECT(ry_rowbank_fetch(b, 1, one_part, one, one_ro, nullptr, bad_ro, d_mc.p, nullptr, one_fo, no_so) == -1);
    EXPECT(ry_rowbank_fetch(b, 1, one_part, one, one_ro, nullptr, no_wo, d_mc.p, nullptr, bad_fo, no_so) == -1);
    EXPECT(ry_rowbank_fetch(b, 1, one_part, one, one_ro, nullptr, no_wo, d_mc.p, nullptr, one_fo, bad_so) == -1);
    EXPECT(ry_rowbank_fetch(b, 1, one_part, one, one_ro, nullptr, no_wo, nullptr, nullptr, one_fo, no_so) == -1);
    EXPECT(ry_rowbank_fetch(b, 1, one_part, nullptr, one_ro, nullptr, no_wo, d_mc.p, nullptr, one_fo, no_so) == -1);
    EXPECT(ry_rowbank_fetch(b, 2, part, rs, ro, ss, wo, d_mc.p, nullptr, fo, so) == -1);
    EXPECT(ry_rowbank_fetch(nullptr, 1, one_part, one, one_ro, nullptr, no_wo, d_mc.p, nullptr, one_fo, no_so) == -4);
    EXPECT(ry_rowbank_fetch(b, 2, part, rs, ro, ss, wo, d_mc.p + 1, d_w.p + 1, fo, so) == 0);
    clear();
    const int keep_low[] = {-1, 25, 0, 62}, keep_high[] = {1, 27, 0, 62}, keep_back[] = {5, 4, 0, 62};
    for (const int* k : {keep_low, keep_high, keep_back})
        EXPECT(ry_rowbank_pick_ap(b, 2, part, rs, ro, fo, k, (const unsigned char*)d_mask.p, d_ap.p, pack_rows) == -1);
    EXPECT(ry_rowbank_pick_ap(b, 2, part, rs, ro, fo, keep, (const unsigned char*)d_mask.p, d_ap.p, pack_rows - 1) == -1);
    EXPECT(ry_rowbank_pick_ap(b, 2, part, rs, ro, fo, keep, nullptr, d_ap.p, pack_rows) == -1);
    EXPECT(ry_rowbank_pick_ap(b, 2, part, rs, ro, fo, keep, (const unsigned char*)d_mask.p, nullptr, pack_rows) == -1);
    EXPECT(ry_rowbank_pick_ap(b, 2, part, rs, ro, fo, nullptr, (const unsigned char*)d_mask.p, d_ap.p, pack_rows) == -1);
    EXPECT(ry_rowbank_pick_ap(nullptr, 2, part, rs, ro, fo, keep, (const unsigned char*)d_mask.p, d_ap.p, pack_rows) == -4);
    for (float v : d_mc.down()) if (v != GUARD) { EXPECT(v == GUARD); break; }
    for (float v : d_ap.down()) if (v != GUARD) { EXPECT(v == GUARD); break; }
    EXPECT(ry_rowbank_pick_ap(b, 2, part, rs, ro, fo, keep, (const unsigned char*)d_mask.p, d_ap.p + 1, pack_rows) == 0);
    {
        const int p1[] = {1}, r0[] = {0}, n1[] = {1}, rp[] = {-1}, neg[] = {-1}, big[] = {ROWS};
        const long long s0[] = {0}, sneg[] = {-1};
        int o1 = -1, o2 = -1;
        EXPECT(ry_rowbank_append(b, 1, p1, nullptr, ap.p, r0, n1, wave.p, s0, n1, &o1, &o2) == -1);
        EXPECT(ry_rowbank_append(b, 1, p1, mc.p, ap.p, r0, neg, wave.p, s0, n1, &o1, &o2) == -1);
        EXPECT(ry_rowbank_append(b, 1, p1, mc.p, ap.p, neg, n1, wave.p, s0, n1, &o1, &o2) == -1);
        EXPECT(ry_rowbank_append(b, 1, p1, mc.p, ap.p, r0, n1, wave.p, sneg, n1, &o1, &o2) == -1);
        EXPECT(ry_rowbank_append(b, 1, p1, mc.p, ap.p, r0, big, wave.p, s0, n1, &o1, &o2) == -1);
        EXPECT(ry_rowbank_append(b, 1, p1, mc.p, ap.p, r0, n1, wave.p, s0, n1, nullptr, &o2) == -1);
        EXPECT(ry_rowbank_append(b, 1, nullptr, mc.p, ap.p, r0, n1, wave.p, s0, n1, &o1, &o2) == -1);
        EXPECT(ry_rowbank_append(b, -1, p1, mc.p, ap.p, r0, n1, wave.p, s0, n1, &o1, &o2) == -1);
        EXPECT(ry_rowbank_append(nullptr, 1, p1, mc.p, ap.p, r0, n1, wave.p, s0, n1, &o1, &o2) == -4);
        EXPECT(o1 == -1 && o2 == -1 && rp[0] == -1);
        EXPECT(ry_rowbank_append(b, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);       // nobody: nothing
    }
    append({1}, 0);
    // reset of one stream, then of all; the rings start again at the front
    EXPECT(ry_rowbank_reset(b, 3) == -1 && ry_rowbank_reset(b, -2) == -1 && ry_rowbank_reset(nullptr, 0) == -4);
    EXPECT(ry_rowbank_reset(b, 2) == 0);
    EXPECT(ry_rowbank_held(b, 2, &rows, &samples) == 0 && rows == 0 && samples == 0);
    EXPECT(ry_rowbank_held(b, 1, &rows, &samples) == 0 && rows == 4 * SEG_ROWS[1] && samples == 4 * SEG_SAMPLES[1]);
    EXPECT(ry_rowbank_held(b, 3, &rows, &samples) == -1 && ry_rowbank_held(b, 0, nullptr, &samples) == -1);
    EXPECT(ry_rowbank_debug_poison(b) == 0);
    n_seg[2] = 0;
    append({2}, 0);
    EXPECT(pos_r[2][0] == 0 && pos_s[2][0] == 0);
    EXPECT(ry_rowbank_reset(b, -1) == 0);
    for (int s = 0; s < B; ++s) EXPECT(ry_rowbank_held(b, s, &rows, &samples) == 0 && rows == 0 && samples == 0);
    const float* ring[3] = {nullptr, nullptr, nullptr};
    EXPECT(ry_rowbank_debug_buffers(b, &ring[0], &ring[1], &ring[2]) == 0 && ring[0] && ring[1] && ring[2]);
    EXPECT(ry_rowbank_debug_counts(b, nullptr) == -1);
    EXPECT(ry_rowbank_debug_poison(b) == 0);
    ry_rowbank_destroy(b);
    ry_rowbank_destroy(nullptr);
    std::printf(failures ? "rowbank_host_check: %d FAILED\n" : "rowbank_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
