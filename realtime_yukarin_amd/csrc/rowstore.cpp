// rowstore.cpp -- the row store of libry355.so: the reference's `stream.stream` list of feature segments (stream/base_stream.py) kept as device
// rows.  Three float32 rings on the card -- mc [cap_rows][mc_cols], ap [cap_rows][ap_cols], wave [cap_samples] -- filled in arrival order by
// ry_rowstore_append straight from the blocks the encode stage left on the card, and read by ry_rowstore_fetch, which writes a convert window
// (the spans `BaseStream.fetch` would concatenate, pads included) back to back into the caller's blocks.  Kernel: rowstore_kernels.h.
// The host keeps the bookkeeping: the ring position of the oldest live row / sample and the live counts.  WHEN a segment may go is the
// caller's rule (streams.retire over worker.retire_time); the store only takes ry_rowstore_retire's counts, oldest first, and refuses an append
// that would run over what is still live and a fetch that names what is not.  Every refusal is made before anything is enqueued or changed.
// Waits: an append waits for nothing (its pieces travel in the kernel arguments).  A fetch uploads its piece table from a pinned block and waits
// for that copy alone -- not for the kernel -- so the block is free for the next call (the ingest pattern of analysis.cpp).
// The row bank (ry_rowbank_*, at the end) is the same store for B streams: B sets of rings behind one another in the three arrays, a live range
// per stream, every call one launch for all the streams it names; its append and fetch are rs_copy, its masked read of ap rows is rs_pick.
#include "rowstore_kernels.h"
#include "ry_host.h"

// What a store and a bank share: the rings' shape, the piece table with its staging, and the counters of the last call.
struct RsStage {
    ry_ctx* ctx = nullptr;
    int cols[2] = {0, 0};                            // mc, ap
    int cap_rows = 0, cap_samples = 0;
    DevBufList rings;                                // never poisoned as a whole
    DevBuf<float> mc{rings}, ap{rings}, wave{rings};
    DevBufList scratch;
    DevBuf<RsPiece> d_tab{scratch};
    std::vector<RsPiece> tab;
    void* pin = nullptr; size_t pin_bytes = 0;       // staging of the table
    rt::Event up_done; bool has_event = false;
    long long counts[4] = {0, 0, 0, 0};              // of the last append / fetch / pick: kernel launches, uploads, waits, bytes uploaded
};

struct RsLive {
    int row_tail = 0, row_live = 0;                  // ring position of the oldest live row, live rows
    int sample_tail = 0, sample_live = 0;
};

struct ry_rowstore : RsStage, RsLive {};

// B sets of rings behind one another in the three arrays: stream b's mc ring starts at element b * cap_rows * mc_cols, and so on.
struct ry_rowbank : RsStage {
    int n_streams = 0;
    std::vector<RsLive> live;
    DevBuf<RsPick> d_pick{scratch};
    std::vector<RsPick> picks;
    std::vector<int> pos;                            // append: the positions, handed out once the call is through
};

namespace {
enum { RS_MAX_COLS = 1 << 16, RS_MAX_ROWS = 1 << 22, RS_MAX_SAMPLES = 1 << 30, RS_MAX_SPANS = 1 << 20, RS_MAX_GRID = 2048, RS_MAX_STREAMS = 1 << 16 };
const long long RS_MAX_ARRAY = 1LL << 40;           // floats in one array of a bank: what its pieces' offsets are held to

int head_of(const float* base, long long at, int n) {
    const int h = (int)((4 - ((reinterpret_cast<unsigned long long>(base + at) >> 2) & 3)) & 3);
    return h < n ? h : n;
}

// One contiguous run of `n` elements to `tab`, cut where the ring ends.  ring_is_src: the ring is read at ring_at (-1: a pad), the block
// written at block_at; else the block is read and the ring written.  ring_base (a bank): where the ring starts in its array.
void add_run(std::vector<RsPiece>& tab, int arr, bool ring_is_src, long long ring_at, long long ring_elems, long long block_at, long long n,
             const float* dst_base, long long ring_base = 0) {
    while (n > 0) {
        long long take = n < (1LL << 30) ? n : (1LL << 30);          // a piece counts its elements in an int
        if (ring_at >= 0 && ring_at + take > ring_elems) take = ring_elems - ring_at;
        RsPiece e;
        memset(&e, 0, sizeof e);
        const long long in_array = ring_at < 0 ? -1 : ring_base + ring_at;
        e.src = ring_is_src ? in_array : block_at;
        e.dst = ring_is_src ? block_at : in_array;
        e.n = (int)take; e.arr = arr;
        e.head = head_of(dst_base, e.dst, e.n);
        tab.push_back(e);
        n -= take; block_at += take;
        if (ring_at >= 0) { ring_at += take; if (ring_at >= ring_elems) ring_at = 0; }
    }
}

template <typename Piece>
int number_blocks(std::vector<Piece>& tab) {
    long long blocks = 0;
    for (Piece& e : tab) {
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

int stage_room(RsStage* s, size_t bytes) {
    if (bytes <= s->pin_bytes) return RY_OK;
    if (s->pin) rt::hfree(s->pin);                                  // every upload has been waited for
    s->pin = nullptr; s->pin_bytes = 0;
    const size_t n = bytes + bytes / 2 + 1024;
    if (rt::hmalloc(&s->pin, n) != 0) { s->pin = nullptr; return fail(RY_ENOMEM, "host allocation of %zu staging bytes failed", n); }
    s->pin_bytes = n;
    return RY_OK;
}

// The one upload of a call: `bytes` of a table through the pinned block to `dev`, its event recorded behind it; upload_done waits for that
// copy alone -- not for the kernel -- so the block is free for the next call.
int upload(RsStage* s, void* dev, const void* host, size_t bytes) {
    RY_TRY(stage_room(s, bytes));
    memcpy(s->pin, host, bytes);
    RT_TRY(rt::h2d(dev, s->pin, bytes, s->ctx->stream)); ++s->counts[1]; s->counts[3] = (long long)bytes;
    RT_TRY(rt::event_record(s->up_done, s->ctx->stream));
    return RY_OK;
}

int upload_done(RsStage* s) {
    RT_TRY(rt::event_sync(s->up_done)); ++s->counts[2];
    return RY_OK;
}

// s->tab through rs_copy in ONE launch.  by_value: the pieces (at most RS_INLINE) travel in the kernel arguments and nothing is waited for;
// else the table goes up and the upload is waited for.
int run_copy(RsStage* s, const float* const src[RS_ARRAYS], float* const dst[RS_ARRAYS], bool by_value) {
    std::vector<RsPiece>& tab = s->tab;
    if (tab.empty()) return RY_OK;
    const ry_stream_t st = s->ctx->stream;
    if (!by_value) RY_TRY(s->d_tab.grow(s->ctx, (long long)tab.size()));
    RsCopyParams p;
    memset(&p, 0, sizeof p);
    p.n_blocks = number_blocks(tab);
    p.n_pieces = (int)tab.size();
    if (by_value) {
        for (size_t i = 0; i < tab.size(); ++i) p.inl[i] = tab[i];
    } else {
        RY_TRY(upload(s, s->d_tab.ptr(), tab.data(), tab.size() * sizeof(RsPiece)));
        p.tab = s->d_tab.ptr();
    }
    for (int a = 0; a < RS_ARRAYS; ++a) { p.src[a] = src[a]; p.dst[a] = dst[a]; }
    const int grid = p.n_blocks < RS_MAX_GRID ? p.n_blocks : (int)RS_MAX_GRID;
    RY_LAUNCH(rs_copy, dim3((unsigned)grid), 256, st, p); ++s->counts[0];
    RT_TRY(rt::last_error());
    if (!by_value) RY_TRY(upload_done(s));
    return RY_OK;
}

// NaN bit patterns in the scratch buffers and in the parts of the rings that hold nothing live: [tail + live, tail + cap) mod cap of every
// stream's rings (`live`: n_streams entries)
int poison(RsStage* s, const RsLive* live, int n_streams) {
    const ry_stream_t st = s->ctx->stream;
    for (DevBufBase* b : s->scratch) RY_TRY(b->poison(st));
    auto dead = [&](float* ring, long long unit, int tail, int n_live, int cap) -> int {
        long long at = ((long long)tail + n_live) % cap, n = (long long)cap - n_live;
        while (n > 0) {
            const long long take = at + n > cap ? cap - at : n;
            RT_TRY(rt::dmemset(ring + at * unit, 0xff, (size_t)(take * unit) * sizeof(float), st));
            n -= take; at = 0;
        }
        return RY_OK;
    };
    for (int b = 0; b < n_streams; ++b) {
        const RsLive& l = live[b];
        RY_TRY(dead(s->mc.ptr() + (long long)b * s->cap_rows * s->cols[0], s->cols[0], l.row_tail, l.row_live, s->cap_rows));
        RY_TRY(dead(s->ap.ptr() + (long long)b * s->cap_rows * s->cols[1], s->cols[1], l.row_tail, l.row_live, s->cap_rows));
        RY_TRY(dead(s->wave.ptr() + (long long)b * s->cap_samples, 1, l.sample_tail, l.sample_live, s->cap_samples));
    }
    RT_TRY(rt::stream_sync(st));
    return RY_OK;
}

// the shape of one set of rings: the limits of ry_rowstore_create
int check_shape(int mc_cols, int ap_cols, int cap_rows, int cap_samples) {
    if (mc_cols < 1 || mc_cols > RS_MAX_COLS || ap_cols < 1 || ap_cols > RS_MAX_COLS)
        return fail(RY_EINVAL, "rows of %d / %d floats: 1 .. %d", mc_cols, ap_cols, (int)RS_MAX_COLS);
    if (cap_rows < 1 || cap_rows > RS_MAX_ROWS) return fail(RY_EINVAL, "a ring of %d rows: 1 .. %d", cap_rows, (int)RS_MAX_ROWS);
    if ((long long)cap_rows * (mc_cols > ap_cols ? mc_cols : ap_cols) > (1LL << 30))
        return fail(RY_EINVAL, "a ring of %d rows of %d / %d floats: at most 2^30 floats", cap_rows, mc_cols, ap_cols);
    if (cap_samples < 1 || cap_samples > RS_MAX_SAMPLES) return fail(RY_EINVAL, "a ring of %d samples: 1 .. %d", cap_samples, (int)RS_MAX_SAMPLES);
    return RY_OK;
}

// an append of n_rows / n_samples from row0 / sample0 to the rings of `l`: the refusals of ry_rowstore_append
int check_append(const RsStage* s, const RsLive& l, long long row0, int n_rows, long long sample0, int n_samples, const float* mc_dev, const float* ap_dev,
                 const float* wave_dev) {
    if (n_rows < 0 || n_samples < 0 || row0 < 0 || sample0 < 0)
        return fail(RY_EINVAL, "rows [%lld, %lld + %d), samples [%lld, %lld + %d): counts and offsets below 0", row0, row0, n_rows, sample0, sample0, n_samples);
    if (n_rows > 0 && (!mc_dev || !ap_dev)) return fail(RY_EINVAL, "null mc / ap block");
    if (n_samples > 0 && !wave_dev) return fail(RY_EINVAL, "null wave");
    if (n_rows > s->cap_rows - l.row_live)
        return fail(RY_EINVAL, "%d rows do not fit: %d of %d are live (not retired)", n_rows, l.row_live, s->cap_rows);
    if (n_samples > s->cap_samples - l.sample_live)
        return fail(RY_EINVAL, "%d samples do not fit: %d of %d are live (not retired)", n_samples, l.sample_live, s->cap_samples);
    return RY_OK;
}

// the pieces of that append, behind what the rings of `l` (stream `b` of a bank) hold -> the positions the segment starts at
void add_append(RsStage* s, const RsLive& l, int b, long long row0, int n_rows, long long sample0, int n_samples, int* rp, int* sp) {
    *rp = (int)(((long long)l.row_tail + l.row_live) % s->cap_rows);
    *sp = (int)(((long long)l.sample_tail + l.sample_live) % s->cap_samples);
    float* const ring[RS_ARRAYS] = {s->mc.ptr(), s->ap.ptr(), s->wave.ptr()};
    for (int a = 0; a < 2; ++a) {
        const long long c = s->cols[a];
        add_run(s->tab, a, false, *rp * c, s->cap_rows * c, row0 * c, n_rows * c, ring[a], (long long)b * s->cap_rows * c);
    }
    add_run(s->tab, 2, false, *sp, s->cap_samples, sample0, n_samples, ring[2], (long long)b * s->cap_samples);
}

int check_retire(const RsLive& l, int n_rows, int n_samples) {
    if (n_rows < 0 || n_rows > l.row_live || n_samples < 0 || n_samples > l.sample_live)
        return fail(RY_EINVAL, "retire %d rows of %d live, %d samples of %d live", n_rows, l.row_live, n_samples, l.sample_live);
    return RY_OK;
}

void retire(RsLive& l, int n_rows, int n_samples, int cap_rows, int cap_samples) {
    l.row_tail = (int)(((long long)l.row_tail + n_rows) % cap_rows); l.row_live -= n_rows;
    l.sample_tail = (int)(((long long)l.sample_tail + n_samples) % cap_samples); l.sample_live -= n_samples;
}

// `n` spans (ring position or -1, destination offset, count) against a ring of `cap` with its live part and a destination of `room`
int check_spans(const int* sp, int n, int cap, long long room, int tail, int live, const char* what) {
    for (int i = 0; i < n; ++i) {
        const int src = sp[3 * i], dst = sp[3 * i + 1], count = sp[3 * i + 2];
        if (count < 0) return fail(RY_EINVAL, "%s span %d has %d elements", what, i, count);
        if (dst < 0 || (long long)dst + count > room) return fail(RY_EINVAL, "%s span %d: [%d, %d + %d) outside the destination of %lld", what, i, dst, dst, count, room);
        if (src == -1) continue;
        if (src < 0 || src >= cap || count > cap) return fail(RY_EINVAL, "%s span %d: position %d, %d elements outside the ring of %d", what, i, src, count, cap);
        if (count > 0 && !is_live(src, count, tail, live, cap)) return fail(RY_EINVAL, "%s span %d: [%d, %d + %d) holds retired (or never written) positions", what, i, src, src, count);
    }
    return RY_OK;
}

// ---- the bank's tables
int check_streams(const ry_rowbank* b, int n, const int* stream_of) {
    if (n < 0 || n > b->n_streams) return fail(RY_EINVAL, "%d streams of a bank of %d", n, b->n_streams);
    if (n > 0 && !stream_of) return fail(RY_EINVAL, "null stream_of");
    for (int i = 0; i < n; ++i) {
        if (stream_of[i] < 0 || stream_of[i] >= b->n_streams) return fail(RY_EINVAL, "entry %d names stream %d of %d", i, stream_of[i], b->n_streams);
        if (i > 0 && stream_of[i] <= stream_of[i - 1]) return fail(RY_EINVAL, "stream_of is not strictly ascending at entry %d (%d after %d)", i, stream_of[i], stream_of[i - 1]);
    }
    return RY_OK;
}

template <typename T>
int check_offsets(const T* off, int n, const char* what) {
    if (!off) return fail(RY_EINVAL, "null %s", what);
    if (off[0] != 0) return fail(RY_EINVAL, "%s starts at %lld, not at 0", what, (long long)off[0]);
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(RY_EINVAL, "%s falls at entry %d", what, i + 1);
    return RY_OK;
}

// the row spans of every stream of a call against that stream's rings and its slice [frame_offsets[i], frame_offsets[i + 1]) of the window rows
int check_row_tables(const ry_rowbank* b, int n, const int* stream_of, const int* row_spans, const int* row_span_offsets, const int* frame_offsets) {
    RY_TRY(check_offsets(row_span_offsets, n, "row_span_offsets"));
    RY_TRY(check_offsets(frame_offsets, n, "frame_offsets"));
    if (row_span_offsets[n] > RS_MAX_SPANS) return fail(RY_EINVAL, "%d row spans", row_span_offsets[n]);
    if (row_span_offsets[n] > 0 && !row_spans) return fail(RY_EINVAL, "null row_spans");
    for (int i = 0; i < n; ++i) {
        const RsLive& l = b->live[stream_of[i]];
        RY_TRY(check_spans(row_spans + 3 * (long long)row_span_offsets[i], row_span_offsets[i + 1] - row_span_offsets[i], b->cap_rows,
                           (long long)frame_offsets[i + 1] - frame_offsets[i], l.row_tail, l.row_live, "row"));
    }
    return RY_OK;
}
}  // namespace

extern "C" {

int ry_rowstore_create(ry_ctx* ctx, int mc_cols, int ap_cols, int cap_rows, int cap_samples, ry_rowstore** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    if (!ctx) return fail(RY_EINVAL, "null context");
    RY_TRY(check_shape(mc_cols, ap_cols, cap_rows, cap_samples));
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

static void destroy_stage(RsStage* s) {
    rt::set_device(s->ctx->device);
    rt::stream_sync(s->ctx->stream);
    if (s->has_event) rt::event_destroy(s->up_done);
    if (s->pin) rt::hfree(s->pin);
}

void ry_rowstore_destroy(ry_rowstore* s) {
    if (!s) return;
    destroy_stage(s);
    delete s;
}

int ry_rowstore_append(ry_rowstore* s, const float* mc_dev, const float* ap_dev, int row0, int n_rows, const float* wave_dev, int sample0, int n_samples,
                       int* row_pos, int* sample_pos) {
    RY_TRY(check_handle(s, "row store"));
    if (!row_pos || !sample_pos) return fail(RY_EINVAL, "null row_pos / sample_pos");
    RY_TRY(check_append(s, *s, row0, n_rows, sample0, n_samples, mc_dev, ap_dev, wave_dev));
    s->counts[0] = s->counts[1] = s->counts[2] = s->counts[3] = 0;
    s->tab.clear();
    int rp, sp;
    add_append(s, *s, 0, row0, n_rows, sample0, n_samples, &rp, &sp);           // at most two pieces per array
    const float* const src[RS_ARRAYS] = {mc_dev, ap_dev, wave_dev};
    float* const ring[RS_ARRAYS] = {s->mc.ptr(), s->ap.ptr(), s->wave.ptr()};
    RY_TRY(run_copy(s, src, ring, true));
    s->row_live += n_rows; s->sample_live += n_samples;
    *row_pos = rp; *sample_pos = sp;
    return RY_OK;
}

int ry_rowstore_retire(ry_rowstore* s, int n_rows, int n_samples) {
    RY_TRY(check_handle(s, "row store"));
    RY_TRY(check_retire(*s, n_rows, n_samples));
    retire(*s, n_rows, n_samples, s->cap_rows, s->cap_samples);
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
    RY_TRY(check_spans(row_spans, n_row_spans, s->cap_rows, dst_rows, s->row_tail, s->row_live, "row"));
    RY_TRY(check_spans(sample_spans, n_sample_spans, s->cap_samples, dst_samples, s->sample_tail, s->sample_live, "sample"));
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
    const float* const ring[RS_ARRAYS] = {s->mc.ptr(), s->ap.ptr(), s->wave.ptr()};
    return run_copy(s, ring, dst, false);                          // the one upload: both span tables; the kernel is not waited for
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
    return poison(s, s, 1);
}

// ---- the bank: B sets of rings, every call one launch for all the streams it names
int ry_rowbank_create(ry_ctx* ctx, int n_streams, int mc_cols, int ap_cols, int cap_rows, int cap_samples, ry_rowbank** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    if (!ctx) return fail(RY_EINVAL, "null context");
    if (n_streams < 1 || n_streams > RS_MAX_STREAMS) return fail(RY_EINVAL, "a bank of %d streams: 1 .. %d", n_streams, (int)RS_MAX_STREAMS);
    RY_TRY(check_shape(mc_cols, ap_cols, cap_rows, cap_samples));
    const long long rows = (long long)n_streams * cap_rows, widest = mc_cols > ap_cols ? mc_cols : ap_cols;
    if (rows * widest > RS_MAX_ARRAY || (long long)n_streams * cap_samples > RS_MAX_ARRAY)
        return fail(RY_EINVAL, "%d streams of %d rows of %d / %d floats and %d samples: at most 2^40 floats in an array", n_streams, cap_rows, mc_cols, ap_cols,
                    cap_samples);
    RT_TRY(rt::set_device(ctx->device));
    std::unique_ptr<ry_rowbank> b(new ry_rowbank());
    b->ctx = ctx; b->n_streams = n_streams; b->cols[0] = mc_cols; b->cols[1] = ap_cols; b->cap_rows = cap_rows; b->cap_samples = cap_samples;
    b->live.resize((size_t)n_streams);
    RY_TRY(b->mc.reserve(ctx, rows * mc_cols));
    RY_TRY(b->ap.reserve(ctx, rows * ap_cols));
    RY_TRY(b->wave.reserve(ctx, (long long)n_streams * cap_samples));
    RT_TRY(rt::event_create_fast(&b->up_done));
    b->has_event = true;
    *out = b.release();
    return RY_OK;
}

void ry_rowbank_destroy(ry_rowbank* b) {
    if (!b) return;
    destroy_stage(b);
    delete b;
}

int ry_rowbank_append(ry_rowbank* b, int n, const int* stream_of, const float* mc_dev, const float* ap_dev, const int* row0, const int* n_rows,
                      const float* wave_dev, const long long* sample0, const int* n_samples, int* row_pos, int* sample_pos) {
    RY_TRY(check_handle(b, "row bank"));
    RY_TRY(check_streams(b, n, stream_of));
    if (n > 0 && (!row0 || !n_rows || !sample0 || !n_samples)) return fail(RY_EINVAL, "null row0 / n_rows / sample0 / n_samples");
    if (n > 0 && (!row_pos || !sample_pos)) return fail(RY_EINVAL, "null row_pos / sample_pos");
    for (int i = 0; i < n; ++i) RY_TRY(check_append(b, b->live[stream_of[i]], row0[i], n_rows[i], sample0[i], n_samples[i], mc_dev, ap_dev, wave_dev));
    b->counts[0] = b->counts[1] = b->counts[2] = b->counts[3] = 0;
    b->tab.clear();
    b->pos.resize(2 * (size_t)n);
    for (int i = 0; i < n; ++i)
        add_append(b, b->live[stream_of[i]], stream_of[i], row0[i], n_rows[i], sample0[i], n_samples[i], &b->pos[2 * i], &b->pos[2 * i + 1]);
    const float* const src[RS_ARRAYS] = {mc_dev, ap_dev, wave_dev};
    float* const ring[RS_ARRAYS] = {b->mc.ptr(), b->ap.ptr(), b->wave.ptr()};
    RY_TRY(run_copy(b, src, ring, b->tab.size() <= RS_INLINE));   // a longer table goes up: still one launch
    for (int i = 0; i < n; ++i) {
        RsLive& l = b->live[stream_of[i]];
        l.row_live += n_rows[i]; l.sample_live += n_samples[i];
        row_pos[i] = b->pos[2 * i]; sample_pos[i] = b->pos[2 * i + 1];
    }
    return RY_OK;
}

int ry_rowbank_fetch(ry_rowbank* b, int n, const int* stream_of, const int* row_spans, const int* row_span_offsets, const int* sample_spans,
                     const int* sample_span_offsets, float* mc_dst_dev, float* wave_dst_dev, const int* frame_offsets, const long long* sample_offsets) {
    RY_TRY(check_handle(b, "row bank"));
    RY_TRY(check_streams(b, n, stream_of));
    RY_TRY(check_row_tables(b, n, stream_of, row_spans, row_span_offsets, frame_offsets));
    RY_TRY(check_offsets(sample_span_offsets, n, "sample_span_offsets"));
    RY_TRY(check_offsets(sample_offsets, n, "sample_offsets"));
    if (sample_span_offsets[n] > RS_MAX_SPANS) return fail(RY_EINVAL, "%d sample spans", sample_span_offsets[n]);
    if (row_span_offsets[n] > 0 && !mc_dst_dev) return fail(RY_EINVAL, "null mc destination");
    if (sample_span_offsets[n] > 0 && (!sample_spans || !wave_dst_dev)) return fail(RY_EINVAL, "null sample_spans / wave destination");
    for (int i = 0; i < n; ++i) {
        const RsLive& l = b->live[stream_of[i]];
        RY_TRY(check_spans(sample_spans + 3 * (long long)sample_span_offsets[i], sample_span_offsets[i + 1] - sample_span_offsets[i], b->cap_samples,
                           sample_offsets[i + 1] - sample_offsets[i], l.sample_tail, l.sample_live, "sample"));
    }
    b->counts[0] = b->counts[1] = b->counts[2] = b->counts[3] = 0;
    std::vector<RsPiece>& tab = b->tab;
    tab.clear();
    float* const dst[RS_ARRAYS] = {mc_dst_dev, nullptr, wave_dst_dev};
    const long long c = b->cols[0];
    for (int i = 0; i < n; ++i)
        for (int k = row_span_offsets[i]; k < row_span_offsets[i + 1]; ++k) {
            const long long src = row_spans[3 * k];
            add_run(tab, 0, true, src < 0 ? -1 : src * c, b->cap_rows * c, (frame_offsets[i] + (long long)row_spans[3 * k + 1]) * c, row_spans[3 * k + 2] * c,
                    dst[0], (long long)stream_of[i] * b->cap_rows * c);
        }
    for (int i = 0; i < n; ++i)
        for (int k = sample_span_offsets[i]; k < sample_span_offsets[i + 1]; ++k)
            add_run(tab, 2, true, sample_spans[3 * k], b->cap_samples, sample_offsets[i] + sample_spans[3 * k + 1], sample_spans[3 * k + 2], dst[2],
                    (long long)stream_of[i] * b->cap_samples);
    const float* const ring[RS_ARRAYS] = {b->mc.ptr(), b->ap.ptr(), b->wave.ptr()};
    return run_copy(b, ring, dst, false);
}

int ry_rowbank_pick_ap(ry_rowbank* b, int n, const int* stream_of, const int* row_spans, const int* row_span_offsets, const int* frame_offsets,
                       const int* keep, const unsigned char* mask_dev, float* ap_pack_dev, int pack_rows) {
    RY_TRY(check_handle(b, "row bank"));
    RY_TRY(check_streams(b, n, stream_of));
    RY_TRY(check_row_tables(b, n, stream_of, row_spans, row_span_offsets, frame_offsets));
    if (n > 0 && !keep) return fail(RY_EINVAL, "null keep");
    long long kept = 0;
    for (int i = 0; i < n; ++i) {
        const int k0 = keep[2 * i], k1 = keep[2 * i + 1], rows = frame_offsets[i + 1] - frame_offsets[i];
        if (k0 < 0 || k1 < k0 || k1 > rows) return fail(RY_EINVAL, "entry %d keeps rows [%d, %d) of a window of %d", i, k0, k1, rows);
        kept += k1 - k0;
    }
    if (pack_rows != kept) return fail(RY_EINVAL, "pack_rows is %d, the kept rows are %lld", pack_rows, kept);
    if (kept > 0 && (!mask_dev || !ap_pack_dev)) return fail(RY_EINVAL, "null mask / ap_pack");
    b->counts[0] = b->counts[1] = b->counts[2] = b->counts[3] = 0;
    std::vector<RsPick>& tab = b->picks;
    tab.clear();
    const long long c = b->cols[1], max_rows = (1LL << 30) / c;        // a piece counts its elements in an int
    long long at = 0;                                              // the first packed row of the stream
    for (int i = 0; i < n; ++i) {
        const int k0 = keep[2 * i], k1 = keep[2 * i + 1];
        for (int k = row_span_offsets[i]; k < row_span_offsets[i + 1]; ++k) {
            const long long src = row_spans[3 * k], first = row_spans[3 * k + 1], last = first + row_spans[3 * k + 2];
            long long r = first > k0 ? first : k0;                     // the window rows of the span that are kept: [r, end)
            const long long end = last < k1 ? last : k1;
            long long ring_row = src < 0 ? -1 : (src + (r - first)) % b->cap_rows;
            while (r < end) {
                long long take = end - r < max_rows ? end - r : max_rows;
                if (ring_row >= 0 && ring_row + take > b->cap_rows) take = b->cap_rows - ring_row;
                RsPick e;
                memset(&e, 0, sizeof e);
                e.src = ring_row < 0 ? -1 : ((long long)stream_of[i] * b->cap_rows + ring_row) * c;
                e.dst = (at + (r - k0)) * c;
                e.n = (int)(take * c); e.mask0 = (int)(frame_offsets[i] + r);
                e.head = head_of(ap_pack_dev, e.dst, e.n);
                tab.push_back(e);
                r += take;
                if (ring_row >= 0) { ring_row += take; if (ring_row >= b->cap_rows) ring_row = 0; }
            }
        }
        at += k1 - k0;
    }
    if (tab.empty()) return RY_OK;
    RY_TRY(b->d_pick.grow(b->ctx, (long long)tab.size()));
    RsPickParams p;
    memset(&p, 0, sizeof p);
    p.n_blocks = number_blocks(tab);
    p.n_pieces = (int)tab.size();
    p.cols = (int)c;
    RY_TRY(upload(b, b->d_pick.ptr(), tab.data(), tab.size() * sizeof(RsPick)));
    p.tab = b->d_pick.ptr();
    p.src = b->ap.ptr(); p.mask = mask_dev; p.dst = ap_pack_dev;
    const int grid = p.n_blocks < RS_MAX_GRID ? p.n_blocks : (int)RS_MAX_GRID;
    RY_LAUNCH(rs_pick, dim3((unsigned)grid), 256, b->ctx->stream, p); ++b->counts[0];
    RT_TRY(rt::last_error());
    return upload_done(b);
}

int ry_rowbank_retire(ry_rowbank* b, int stream, int n_rows, int n_samples) {
    RY_TRY(check_handle(b, "row bank"));
    if (stream < 0 || stream >= b->n_streams) return fail(RY_EINVAL, "stream %d of %d", stream, b->n_streams);
    RY_TRY(check_retire(b->live[stream], n_rows, n_samples));
    retire(b->live[stream], n_rows, n_samples, b->cap_rows, b->cap_samples);
    return RY_OK;
}

int ry_rowbank_reset(ry_rowbank* b, int stream) {
    RY_TRY(check_handle(b, "row bank"));
    if (stream < -1 || stream >= b->n_streams) return fail(RY_EINVAL, "stream %d of %d", stream, b->n_streams);
    for (int i = 0; i < b->n_streams; ++i)
        if (stream < 0 || i == stream) b->live[i] = RsLive();
    return RY_OK;
}

int ry_rowbank_held(ry_rowbank* b, int stream, int* rows, int* samples) {
    if (!b || !rows || !samples || stream < 0 || stream >= b->n_streams) return fail(RY_EINVAL, "bad argument");
    *rows = b->live[stream].row_live; *samples = b->live[stream].sample_live;
    return RY_OK;
}

int ry_rowbank_debug_buffers(ry_rowbank* b, const float** mc_dev, const float** ap_dev, const float** wave_dev) {
    if (!b) return fail(RY_ESTATE, "null row bank handle");
    if (mc_dev) *mc_dev = b->mc.ptr();
    if (ap_dev) *ap_dev = b->ap.ptr();
    if (wave_dev) *wave_dev = b->wave.ptr();
    return RY_OK;
}

int ry_rowbank_debug_counts(ry_rowbank* b, long long* out) {
    if (!b || !out) return fail(RY_EINVAL, "bad argument");
    for (int i = 0; i < 4; ++i) out[i] = b->counts[i];
    return RY_OK;
}

int ry_rowbank_debug_poison(ry_rowbank* b) {
    RY_TRY(check_handle(b, "row bank"));
    return poison(b, b->live.data(), b->n_streams);
}

}  // extern "C"
