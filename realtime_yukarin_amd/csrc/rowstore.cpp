// rowstore.cpp -- the row store of libry355.so: the reference's `stream.stream` list of feature segments (stream/base_stream.py) kept as device
// rows.  Three float32 rings on the card -- mc [cap_rows][mc_cols], ap [cap_rows][ap_cols], wave [cap_samples] -- filled in arrival order by
// ry_rowstore_append straight from the blocks the encode stage left on the card, and read by ry_rowstore_fetch, which writes a convert window
// (the spans `BaseStream.fetch` would concatenate, pads included) back to back into the caller's blocks.  Kernel: rowstore_kernels.h.
// The host keeps the bookkeeping: the ring position of the oldest live row / sample and the live counts.  WHEN a segment may go is the
// caller's rule (streams.retire over worker.retire_time); the store only takes ry_rowstore_retire's counts, oldest first, and refuses an append
// that would run over what is still live and a fetch that names what is not.  Every refusal is made before anything is enqueued or changed.
// Waits: an append waits for nothing (its pieces travel in the kernel arguments).  A fetch uploads its piece table from a pinned block and waits
// for that copy alone -- not for the kernel -- so the block is free for the next call (the ingest pattern of analysis.cpp).
#include "rowstore_kernels.h"
#include "ry_host.h"

struct ry_rowstore {
    ry_ctx* ctx = nullptr;
    int cols[2] = {0, 0};                            // mc, ap
    int cap_rows = 0, cap_samples = 0;
    DevBufList rings;                                // never poisoned as a whole
    DevBuf<float> mc{rings}, ap{rings}, wave{rings};
    DevBufList scratch;
    DevBuf<RsPiece> d_tab{scratch};
    int row_tail = 0, row_live = 0;                  // ring position of the oldest live row, live rows
    int sample_tail = 0, sample_live = 0;
    std::vector<RsPiece> tab;
    void* pin = nullptr; size_t pin_bytes = 0;       // staging of the table
    rt::Event up_done; bool has_event = false;
    long long counts[4] = {0, 0, 0, 0};              // of the last append / fetch: kernel launches, uploads, waits, bytes uploaded
};

namespace {
enum { RS_MAX_COLS = 1 << 16, RS_MAX_ROWS = 1 << 22, RS_MAX_SAMPLES = 1 << 30, RS_MAX_SPANS = 1 << 20, RS_MAX_GRID = 2048 };

int head_of(const float* base, long long at, int n) {
    const int h = (int)((4 - ((reinterpret_cast<unsigned long long>(base + at) >> 2) & 3)) & 3);
    return h < n ? h : n;
}

// One contiguous run of `n` elements to `tab`, cut where the ring ends.  ring_is_src: the ring is read at ring_at (-1: a pad), the block
// written at block_at; else the block is read and the ring written.
void add_run(std::vector<RsPiece>& tab, int arr, bool ring_is_src, long long ring_at, long long ring_elems, long long block_at, long long n,
             const float* dst_base) {
    while (n > 0) {
        long long take = n < (1LL << 30) ? n : (1LL << 30);          // a piece counts its elements in an int
        if (ring_at >= 0 && ring_at + take > ring_elems) take = ring_elems - ring_at;
        RsPiece e;
        memset(&e, 0, sizeof e);
        e.src = ring_is_src ? ring_at : block_at;
        e.dst = ring_is_src ? block_at : ring_at;
        e.n = (int)take; e.arr = arr;
        e.head = head_of(dst_base, e.dst, e.n);
        tab.push_back(e);
        n -= take; block_at += take;
        if (ring_at >= 0) { ring_at += take; if (ring_at >= ring_elems) ring_at = 0; }
    }
}

int number_blocks(std::vector<RsPiece>& tab) {
    long long blocks = 0;
    for (RsPiece& e : tab) {
        e.blk0 = (int)blocks;
        blocks += (((e.n - e.head) >> 2) + 1 + RS_UNITS - 1) / RS_UNITS;
    }
    return (int)blocks;
}

// position `pos`, `count` elements: inside the live part [tail, tail + live) of a ring of `cap`?
bool is_live(int pos, int count, int tail, int live, int cap) {
    const int off = pos >= tail ? pos - tail : pos - tail + cap;
    return (long long)off + count <= live;
}

int stage_room(ry_rowstore* s, size_t bytes) {
    if (bytes <= s->pin_bytes) return RY_OK;
    if (s->pin) rt::hfree(s->pin);                                  // every upload has been waited for
    s->pin = nullptr; s->pin_bytes = 0;
    const size_t n = bytes + bytes / 2 + 1024;
    if (rt::hmalloc(&s->pin, n) != 0) { s->pin = nullptr; return fail(RY_ENOMEM, "host allocation of %zu staging bytes failed", n); }
    s->pin_bytes = n;
    return RY_OK;
}

int poison(ry_rowstore* s) {
    const ry_stream_t st = s->ctx->stream;
    for (DevBufBase* b : s->scratch) RY_TRY(b->poison(st));
    // the parts of the rings that hold nothing live: [tail + live, tail + cap) mod cap, in elements
    auto dead = [&](DevBuf<float>& ring, long long unit, int tail, int live, int cap) -> int {
        long long at = ((long long)tail + live) % cap, n = (long long)cap - live;
        while (n > 0) {
            const long long take = at + n > cap ? cap - at : n;
            RT_TRY(rt::dmemset(ring.ptr() + at * unit, 0xff, (size_t)(take * unit) * sizeof(float), st));
            n -= take; at = 0;
        }
        return RY_OK;
    };
    RY_TRY(dead(s->mc, s->cols[0], s->row_tail, s->row_live, s->cap_rows));
    RY_TRY(dead(s->ap, s->cols[1], s->row_tail, s->row_live, s->cap_rows));
    RY_TRY(dead(s->wave, 1, s->sample_tail, s->sample_live, s->cap_samples));
    RT_TRY(rt::stream_sync(st));
    return RY_OK;
}
}  // namespace

extern "C" {

int ry_rowstore_create(ry_ctx* ctx, int mc_cols, int ap_cols, int cap_rows, int cap_samples, ry_rowstore** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    if (!ctx) return fail(RY_EINVAL, "null context");
    if (mc_cols < 1 || mc_cols > RS_MAX_COLS || ap_cols < 1 || ap_cols > RS_MAX_COLS)
        return fail(RY_EINVAL, "rows of %d / %d floats: 1 .. %d", mc_cols, ap_cols, (int)RS_MAX_COLS);
    if (cap_rows < 1 || cap_rows > RS_MAX_ROWS) return fail(RY_EINVAL, "a ring of %d rows: 1 .. %d", cap_rows, (int)RS_MAX_ROWS);
    if ((long long)cap_rows * (mc_cols > ap_cols ? mc_cols : ap_cols) > (1LL << 30))
        return fail(RY_EINVAL, "a ring of %d rows of %d / %d floats: at most 2^30 floats", cap_rows, mc_cols, ap_cols);
    if (cap_samples < 1 || cap_samples > RS_MAX_SAMPLES) return fail(RY_EINVAL, "a ring of %d samples: 1 .. %d", cap_samples, (int)RS_MAX_SAMPLES);
    RT_TRY(rt::set_device(ctx->device));
    std::unique_ptr<ry_rowstore> s(new ry_rowstore());
    s->ctx = ctx; s->cols[0] = mc_cols; s->cols[1] = ap_cols; s->cap_rows = cap_rows; s->cap_samples = cap_samples;
    RY_TRY(s->mc.reserve(ctx, (long long)cap_rows * mc_cols));
    RY_TRY(s->ap.reserve(ctx, (long long)cap_rows * ap_cols));
    RY_TRY(s->wave.reserve(ctx, cap_samples));
    RT_TRY(rt::event_create_fast(&s->up_done));
    s->has_event = true;
    *out = s.release();
    return RY_OK;
}

void ry_rowstore_destroy(ry_rowstore* s) {
    if (!s) return;
    rt::set_device(s->ctx->device);
    rt::stream_sync(s->ctx->stream);
    if (s->has_event) rt::event_destroy(s->up_done);
    if (s->pin) rt::hfree(s->pin);
    delete s;
}

int ry_rowstore_append(ry_rowstore* s, const float* mc_dev, const float* ap_dev, int row0, int n_rows, const float* wave_dev, int sample0, int n_samples,
                       int* row_pos, int* sample_pos) {
    RY_TRY(check_handle(s, "row store"));
    if (!row_pos || !sample_pos) return fail(RY_EINVAL, "null row_pos / sample_pos");
    if (n_rows < 0 || n_samples < 0 || row0 < 0 || sample0 < 0)
        return fail(RY_EINVAL, "rows [%d, %d + %d), samples [%d, %d + %d): counts and offsets below 0", row0, row0, n_rows, sample0, sample0, n_samples);
    if (n_rows > 0 && (!mc_dev || !ap_dev)) return fail(RY_EINVAL, "null mc / ap block");
    if (n_samples > 0 && !wave_dev) return fail(RY_EINVAL, "null wave");
    if (n_rows > s->cap_rows - s->row_live)
        return fail(RY_EINVAL, "%d rows do not fit: %d of %d are live (not retired)", n_rows, s->row_live, s->cap_rows);
    if (n_samples > s->cap_samples - s->sample_live)
        return fail(RY_EINVAL, "%d samples do not fit: %d of %d are live (not retired)", n_samples, s->sample_live, s->cap_samples);
    const int rp = (int)(((long long)s->row_tail + s->row_live) % s->cap_rows), sp = (int)(((long long)s->sample_tail + s->sample_live) % s->cap_samples);
    s->counts[0] = s->counts[1] = s->counts[2] = s->counts[3] = 0;
    std::vector<RsPiece>& tab = s->tab;
    tab.clear();
    float* const ring[RS_ARRAYS] = {s->mc.ptr(), s->ap.ptr(), s->wave.ptr()};
    for (int a = 0; a < 2; ++a) {
        const long long c = s->cols[a];
        add_run(tab, a, false, rp * c, s->cap_rows * c, row0 * c, n_rows * c, ring[a]);
    }
    add_run(tab, 2, false, sp, s->cap_samples, sample0, n_samples, ring[2]);
    if (!tab.empty()) {                                            // at most two pieces per array
        RsCopyParams p;
        memset(&p, 0, sizeof p);
        p.n_blocks = number_blocks(tab);
        p.n_pieces = (int)tab.size();
        for (size_t i = 0; i < tab.size(); ++i) p.inl[i] = tab[i];
        p.src[0] = mc_dev; p.src[1] = ap_dev; p.src[2] = wave_dev;
        for (int a = 0; a < RS_ARRAYS; ++a) p.dst[a] = ring[a];
        const int grid = p.n_blocks < RS_MAX_GRID ? p.n_blocks : (int)RS_MAX_GRID;
        RY_LAUNCH(rs_copy, dim3((unsigned)grid), 256, s->ctx->stream, p); ++s->counts[0];
        RT_TRY(rt::last_error());
    }
    s->row_live += n_rows; s->sample_live += n_samples;
    *row_pos = rp; *sample_pos = sp;
    return RY_OK;
}

int ry_rowstore_retire(ry_rowstore* s, int n_rows, int n_samples) {
    RY_TRY(check_handle(s, "row store"));
    if (n_rows < 0 || n_rows > s->row_live || n_samples < 0 || n_samples > s->sample_live)
        return fail(RY_EINVAL, "retire %d rows of %d live, %d samples of %d live", n_rows, s->row_live, n_samples, s->sample_live);
    s->row_tail = (int)(((long long)s->row_tail + n_rows) % s->cap_rows); s->row_live -= n_rows;
    s->sample_tail = (int)(((long long)s->sample_tail + n_samples) % s->cap_samples); s->sample_live -= n_samples;
    return RY_OK;
}

int ry_rowstore_held(ry_rowstore* s, int* rows, int* samples) {
    if (!s || !rows || !samples) return fail(RY_EINVAL, "bad argument");
    *rows = s->row_live; *samples = s->sample_live;
    return RY_OK;
}

int ry_rowstore_fetch(ry_rowstore* s, const int* row_spans, int n_row_spans, const int* sample_spans, int n_sample_spans, float* mc_dst_dev,
                      float* ap_dst_dev, float* wave_dst_dev, int dst_rows, int dst_samples) {
    RY_TRY(check_handle(s, "row store"));
    if (n_row_spans < 0 || n_sample_spans < 0 || n_row_spans > RS_MAX_SPANS || n_sample_spans > RS_MAX_SPANS)
        return fail(RY_EINVAL, "%d row spans, %d sample spans", n_row_spans, n_sample_spans);
    if (dst_rows < 0 || dst_samples < 0) return fail(RY_EINVAL, "destinations of %d rows / %d samples", dst_rows, dst_samples);
    if (n_row_spans > 0 && (!row_spans || !mc_dst_dev || !ap_dst_dev)) return fail(RY_EINVAL, "null row_spans / mc / ap destination");
    if (n_sample_spans > 0 && (!sample_spans || !wave_dst_dev)) return fail(RY_EINVAL, "null sample_spans / wave destination");
    for (int k = 0; k < 2; ++k) {
        const int* sp = k ? sample_spans : row_spans;
        const int n = k ? n_sample_spans : n_row_spans, cap = k ? s->cap_samples : s->cap_rows, room = k ? dst_samples : dst_rows;
        const int tail = k ? s->sample_tail : s->row_tail, live = k ? s->sample_live : s->row_live;
        const char* what = k ? "sample" : "row";
        for (int i = 0; i < n; ++i) {
            const int src = sp[3 * i], dst = sp[3 * i + 1], count = sp[3 * i + 2];
            if (count < 0) return fail(RY_EINVAL, "%s span %d has %d elements", what, i, count);
            if (dst < 0 || (long long)dst + count > room) return fail(RY_EINVAL, "%s span %d: [%d, %d + %d) outside the destination of %d", what, i, dst, dst, count, room);
            if (src == -1) continue;
            if (src < 0 || src >= cap || count > cap) return fail(RY_EINVAL, "%s span %d: position %d, %d elements outside the ring of %d", what, i, src, count, cap);
            if (count > 0 && !is_live(src, count, tail, live, cap)) return fail(RY_EINVAL, "%s span %d: [%d, %d + %d) holds retired (or never written) positions", what, i, src, src, count);
        }
    }
    s->counts[0] = s->counts[1] = s->counts[2] = s->counts[3] = 0;
    std::vector<RsPiece>& tab = s->tab;
    tab.clear();
    float* const dst[RS_ARRAYS] = {mc_dst_dev, ap_dst_dev, wave_dst_dev};
    for (int a = 0; a < 2; ++a) {
        const long long c = s->cols[a];
        for (int i = 0; i < n_row_spans; ++i) {
            const long long src = row_spans[3 * i];
            add_run(tab, a, true, src < 0 ? -1 : src * c, s->cap_rows * c, row_spans[3 * i + 1] * c, row_spans[3 * i + 2] * c, dst[a]);
        }
    }
    for (int i = 0; i < n_sample_spans; ++i)
        add_run(tab, 2, true, sample_spans[3 * i], s->cap_samples, sample_spans[3 * i + 1], sample_spans[3 * i + 2], dst[2]);
    if (tab.empty()) return RY_OK;
    const ry_stream_t st = s->ctx->stream;
    const size_t bytes = tab.size() * sizeof(RsPiece);
    RY_TRY(s->d_tab.grow(s->ctx, (long long)tab.size()));
    RY_TRY(stage_room(s, bytes));
    RsCopyParams p;
    memset(&p, 0, sizeof p);
    p.n_blocks = number_blocks(tab);
    p.n_pieces = (int)tab.size();
    memcpy(s->pin, tab.data(), bytes);
    RT_TRY(rt::h2d(s->d_tab.ptr(), s->pin, bytes, st)); ++s->counts[1]; s->counts[3] = (long long)bytes;      // the one upload: both span tables
    RT_TRY(rt::event_record(s->up_done, st));
    p.tab = s->d_tab.ptr();
    p.src[0] = s->mc.ptr(); p.src[1] = s->ap.ptr(); p.src[2] = s->wave.ptr();
    for (int a = 0; a < RS_ARRAYS; ++a) p.dst[a] = dst[a];
    const int grid = p.n_blocks < RS_MAX_GRID ? p.n_blocks : (int)RS_MAX_GRID;
    RY_LAUNCH(rs_copy, dim3((unsigned)grid), 256, st, p); ++s->counts[0];
    RT_TRY(rt::last_error());
    RT_TRY(rt::event_sync(s->up_done)); ++s->counts[2];            // the staging block is free again; the kernel is not waited for
    return RY_OK;
}

int ry_rowstore_reset(ry_rowstore* s) {
    RY_TRY(check_handle(s, "row store"));
    s->row_tail = s->row_live = s->sample_tail = s->sample_live = 0;
    return RY_OK;
}

int ry_rowstore_debug_buffers(ry_rowstore* s, const float** mc_dev, const float** ap_dev, const float** wave_dev) {
    if (!s) return fail(RY_ESTATE, "null row store handle");
    if (mc_dev) *mc_dev = s->mc.ptr();
    if (ap_dev) *ap_dev = s->ap.ptr();
    if (wave_dev) *wave_dev = s->wave.ptr();
    return RY_OK;
}

int ry_rowstore_debug_counts(ry_rowstore* s, long long* out) {
    if (!s || !out) return fail(RY_EINVAL, "bad argument");
    for (int i = 0; i < 4; ++i) out[i] = s->counts[i];
    return RY_OK;
}

int ry_rowstore_debug_poison(ry_rowstore* s) {
    RY_TRY(check_handle(s, "row store"));
    return poison(s);
}

}  // extern "C"
