// rowstore_host_check.cpp -- the host paths of the row store (ry_rowstore_*) in a stand-alone program over the emulator build of libry355,
// meant to be compiled and linked with -fsanitize=address,undefined (scripts/asan_rowstore.sh): create and its refusals, segments appended until
// the rings are full (grow), retire and append again so that rows and samples wrap, fetches with pads, empty spans and spans across the ring end
// into destinations at an odd 4-byte offset between guard words, a fetch table that grows from one span to many, every refusal with a valid call
// after it, poison, reset, destroy.  Exit status 0: every call returned what it should and every word fetched is the word appended.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ry355.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, ry_last_error()); ++failures; } } while (0)

static const int MC = 9, AP = 513, ROWS = 64, SAMPLES = 700, SEG_ROWS = 21, SEG_SAMPLES = 230;
static const float GUARD = -7.25f;

static float value(int segment, int array, int i) { return (float)(segment * 100000 + array * 30000 + i + 1); }

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
    ry_rowstore *s = nullptr, *none = nullptr;
    EXPECT(ry_rowstore_create(ctx, 0, AP, ROWS, SAMPLES, &none) == -1 && none == nullptr);
    EXPECT(ry_rowstore_create(ctx, MC, AP, 0, SAMPLES, &none) == -1);
    EXPECT(ry_rowstore_create(ctx, MC, AP, ROWS, 0, &none) == -1);
    EXPECT(ry_rowstore_create(nullptr, MC, AP, ROWS, SAMPLES, &none) == -1);
    EXPECT(ry_rowstore_create(ctx, MC, AP, ROWS, SAMPLES, nullptr) == -1);
    EXPECT(ry_rowstore_create(ctx, MC, AP, ROWS, SAMPLES, &s) == 0 && s != nullptr);
    EXPECT(ry_rowstore_debug_poison(s) == 0);

    // source blocks of one segment, with two rows / five samples in front that an append must skip
    Dev mc(ctx, (size_t)(SEG_ROWS + 2) * MC), ap(ctx, (size_t)(SEG_ROWS + 2) * AP), wave(ctx, (size_t)SEG_SAMPLES + 5);
    int pos_r[8], pos_s[8], n_seg = 0;
    auto append = [&](int want) {
        std::vector<float> h_mc(mc.n, GUARD), h_ap(ap.n, GUARD), h_w(wave.n, GUARD);
        for (int i = 0; i < SEG_ROWS * MC; ++i) h_mc[(size_t)2 * MC + i] = value(n_seg, 0, i);
        for (int i = 0; i < SEG_ROWS * AP; ++i) h_ap[(size_t)2 * AP + i] = value(n_seg, 1, i);
        for (int i = 0; i < SEG_SAMPLES; ++i) h_w[(size_t)5 + i] = value(n_seg, 2, i);
        mc.up(h_mc); ap.up(h_ap); wave.up(h_w);
        int rp = -1, sp = -1;
        const int rc = ry_rowstore_append(s, mc.p, ap.p, 2, SEG_ROWS, wave.p, 5, SEG_SAMPLES, &rp, &sp);
        EXPECT(rc == want);
        if (rc == 0) { pos_r[n_seg] = rp; pos_s[n_seg] = sp; ++n_seg; }
    };
    // grow: three segments fit (63 of 64 rows, 690 of 700 samples), a fourth is refused and changes nothing
    append(0); append(0); append(0);
    int rows = -1, samples = -1;
    EXPECT(ry_rowstore_held(s, &rows, &samples) == 0 && rows == 63 && samples == 690);
    append(-1);
    EXPECT(ry_rowstore_held(s, &rows, &samples) == 0 && rows == 63 && samples == 690 && n_seg == 3);
    // retire the oldest, append: the new segment wraps in both rings
    EXPECT(ry_rowstore_retire(s, SEG_ROWS + 1, 0) == 0 && ry_rowstore_retire(s, 0, 0) == 0);       // (one row of segment 1 goes too)
    EXPECT(ry_rowstore_retire(s, 100, 0) == -1 && ry_rowstore_retire(s, 0, 691) == -1 && ry_rowstore_retire(s, -1, 0) == -1);
    EXPECT(ry_rowstore_retire(s, 0, SEG_SAMPLES) == 0);
    append(0);
    EXPECT(pos_r[3] == 63 && pos_s[3] == 690);
    EXPECT(ry_rowstore_debug_poison(s) == 0);

    // fetch: pad | rows 1 .. 20 of segment 1 | empty | segment 2 | segment 3 (across the ring end) | pad, into blocks with guards, one word in
    const int dst_rows = 2 + 20 + 21 + 21 + 3, dst_samples = 4 + 230 + 230 + 230 + 6;
    Dev d_mc(ctx, (size_t)dst_rows * MC + 9), d_ap(ctx, (size_t)dst_rows * AP + 9), d_w(ctx, (size_t)dst_samples + 9);
    auto clear = [&]() {
        d_mc.up(std::vector<float>(d_mc.n, GUARD)); d_ap.up(std::vector<float>(d_ap.n, GUARD)); d_w.up(std::vector<float>(d_w.n, GUARD));
    };
    clear();
    const int rs[] = {-1, 0, 2, pos_r[1] + 1, 2, 20, pos_r[2], 22, 0, pos_r[2], 22, 21, pos_r[3], 43, 21, -1, 64, 3};
    const int ss[] = {-1, 0, 4, pos_s[1], 4, 230, pos_s[2], 234, 230, pos_s[3], 464, 230, -1, 694, 6};
    EXPECT(ry_rowstore_fetch(s, rs, 6, ss, 5, d_mc.p + 1, d_ap.p + 1, d_w.p + 1, dst_rows, dst_samples) == 0);
    long long counts[4] = {0, 0, 0, 0};
    EXPECT(ry_rowstore_debug_counts(s, counts) == 0 && counts[0] == 1 && counts[1] == 1 && counts[2] == 1 && counts[3] > 0);
    auto check_rows = [&](const std::vector<float>& got, int cols, int array) {
        EXPECT(got[0] == GUARD);
        for (size_t i = (size_t)dst_rows * cols + 1; i < got.size(); ++i) EXPECT(got[i] == GUARD);
        for (int r = 0; r < dst_rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const float v = got[(size_t)1 + (size_t)r * cols + c];
                float want = 0.f;
                if (r >= 2 && r < 22) want = value(1, array, (r - 2 + 1) * cols + c);
                else if (r >= 22 && r < 43) want = value(2, array, (r - 22) * cols + c);
                else if (r >= 43 && r < 64) want = value(3, array, (r - 43) * cols + c);
                if (v != want) { EXPECT(v == want); return; }
            }
    };
    check_rows(d_mc.down(), MC, 0);
    check_rows(d_ap.down(), AP, 1);
    {
        const std::vector<float> got = d_w.down();
        EXPECT(got[0] == GUARD);
        for (size_t i = (size_t)dst_samples + 1; i < got.size(); ++i) EXPECT(got[i] == GUARD);
        for (int i = 0; i < dst_samples; ++i) {
            float want = 0.f;
            if (i >= 4 && i < 694) want = value(1 + (i - 4) / 230, 2, (i - 4) % 230);
            if (got[(size_t)1 + i] != want) { EXPECT(got[(size_t)1 + i] == want); break; }
        }
    }
    // the table grows: one span, then one span per row
    const int one[] = {pos_r[2], 0, 1};
    EXPECT(ry_rowstore_fetch(s, one, 1, nullptr, 0, d_mc.p, d_ap.p, nullptr, dst_rows, 0) == 0);
    std::vector<int> many;
    for (int r = 0; r < 41; ++r) { many.push_back((pos_r[2] + r) % ROWS); many.push_back(r); many.push_back(1); }
    EXPECT(ry_rowstore_fetch(s, many.data(), 41, nullptr, 0, d_mc.p, d_ap.p, nullptr, dst_rows, 0) == 0);
    EXPECT(d_mc.down()[(size_t)40 * MC] == value(3, 0, 19 * MC));
    // refusals: nothing is written, and a valid call works after them
    clear();
    const int bad_count[] = {pos_r[2], 0, -1}, bad_dst[] = {pos_r[2], dst_rows - 1, 2}, bad_pos[] = {ROWS, 0, 1}, retired[] = {pos_r[1], 0, 1};
    const int never[] = {(pos_r[3] + SEG_ROWS) % ROWS, 0, 1};
    for (const int* bad : {bad_count, bad_dst, bad_pos, retired, never})
        EXPECT(ry_rowstore_fetch(s, bad, 1, nullptr, 0, d_mc.p, d_ap.p, nullptr, dst_rows, 0) == -1);
    EXPECT(ry_rowstore_fetch(s, one, 1, nullptr, 0, nullptr, d_ap.p, nullptr, dst_rows, 0) == -1);
    EXPECT(ry_rowstore_fetch(s, one, 1, nullptr, 0, d_mc.p, nullptr, nullptr, dst_rows, 0) == -1);
    EXPECT(ry_rowstore_fetch(s, nullptr, 1, nullptr, 0, d_mc.p, d_ap.p, nullptr, dst_rows, 0) == -1);
    EXPECT(ry_rowstore_fetch(s, nullptr, 0, ss, 1, d_mc.p, d_ap.p, nullptr, dst_rows, dst_samples) == -1);
    EXPECT(ry_rowstore_fetch(nullptr, one, 1, nullptr, 0, d_mc.p, d_ap.p, nullptr, dst_rows, 0) == -4);
    EXPECT(ry_rowstore_append(s, nullptr, ap.p, 0, 1, wave.p, 0, 1, &rows, &samples) == -1);
    EXPECT(ry_rowstore_append(s, mc.p, ap.p, 0, -1, wave.p, 0, 1, &rows, &samples) == -1);
    EXPECT(ry_rowstore_append(s, mc.p, ap.p, 0, 1, wave.p, 0, 1, nullptr, &samples) == -1);
    for (float v : d_mc.down()) if (v != GUARD) { EXPECT(v == GUARD); break; }
    for (float v : d_ap.down()) if (v != GUARD) { EXPECT(v == GUARD); break; }
    EXPECT(ry_rowstore_fetch(s, one, 1, nullptr, 0, d_mc.p, d_ap.p, nullptr, dst_rows, 0) == 0);
    EXPECT(d_mc.down()[0] == value(2, 0, 0));
    // retire everything, reset, start again at the front of the rings
    EXPECT(ry_rowstore_held(s, &rows, &samples) == 0 && ry_rowstore_retire(s, rows, samples) == 0);
    EXPECT(ry_rowstore_held(s, &rows, &samples) == 0 && rows == 0 && samples == 0);
    EXPECT(ry_rowstore_reset(s) == 0);
    n_seg = 0;
    append(0);
    EXPECT(pos_r[0] == 0 && pos_s[0] == 0);
    const float* ring[3] = {nullptr, nullptr, nullptr};
    EXPECT(ry_rowstore_debug_buffers(s, &ring[0], &ring[1], &ring[2]) == 0 && ring[0] && ring[1] && ring[2]);
    EXPECT(ry_rowstore_debug_poison(s) == 0);
    ry_rowstore_destroy(s);
    ry_rowstore_destroy(nullptr);
    std::printf(failures ? "rowstore_host_check: %d FAILED\n" : "rowstore_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
