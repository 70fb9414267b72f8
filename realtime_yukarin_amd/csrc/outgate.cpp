// outgate.cpp -- the output gate of libry355.so: the tail of the reference's decode worker (worker/decode_worker.py:53-59 and run.py:194-198) --
// append to a carried fragment, cut one chunk per call, judge it with the librosa expression, scale and cast what is audible.  Kernels:
// outgate_kernels.h.  One code path: a lone gate is a bank of one stream whose every push takes part, so stream b of a bank has the bits of a
// lone gate by construction -- a chunk's frames, its record and its samples are computed by workgroups that see that chunk alone.
// The fragments of all streams lie back to back in one of two device buffers; every call writes the other one (og_append: the live part of each
// fragment to the front of its new place, the new samples behind it), so the remainder behind a cut chunk never moves over itself.  The host
// knows the lengths, which is all the bookkeeping asks for: whether a chunk is cut is decided before anything is launched.
// Waits: the table and the host samples go through a pinned staging block (reused once its last copy has landed, normally long ago), so a push
// that completes no chunk returns without waiting for the stream.  A push that completes chunks waits once for all records and, when one of
// them is audible, once more for those chunks; a silent chunk brings no sample to the host.
#include "outgate_kernels.h"
#include "ry_host.h"

struct OgHostStream {
    long long off = 0;       // its fragment's place in the buffer in use
    long long start = 0;     // samples at the front of that place which a cut chunk left dead
    long long held = 0;      // carried samples
};

struct ry_outgate_bank {
    ry_ctx* ctx = nullptr;
    int n_streams = 0, chunk = 0, n_frames = 0, out_f32 = 0;
    double threshold_db = 0, scale = 1;
    Arena tables;
    sy_c* tw1024 = nullptr;
    sy_c* tw2048 = nullptr;
    std::vector<OgHostStream> s;
    DevBufList carried;                              // the two fragment buffers: never poisoned as a whole
    DevBuf<double> frag0{carried}, frag1{carried};
    int cur = 0;
    long long used = 0;                              // samples of the buffer in use that belong to a stream's place
    DevBufList scratch;
    DevBuf<double> d_stage{scratch}, d_db{scratch}, d_fmax{scratch}, d_out{scratch};
    DevBuf<int> d_inf{scratch};
    DevBuf<OgRecord> d_rec{scratch};
    void* pin = nullptr; size_t pin_bytes = 0;       // staging of the upload
    rt::Event up_done; bool has_event = false, up_pending = false;
    std::vector<OgStream> tab;
    std::vector<int> stream_of;
    std::vector<OgRecord> rec;
    long long counts[5] = {0, 0, 0, 0, 0};           // of the last push: stream waits, launches, uploads, downloads, sample bytes brought down
    long long up_bytes = 0;                          // of the last push: bytes of its one upload (the tables, and the samples when they came from the host)
    DevBuf<double>& frag(int i) { return i ? frag1 : frag0; }
};

struct ry_outgate { ry_outgate_bank* k = nullptr; };

namespace {
enum { OG_MAX_CHUNK = 1 << 24, OG_MAX_STREAMS = 1 << 16 };
const long long OG_MAX_SAMPLES = 1LL << 30;          // samples of all fragments after a call

int stage_room(ry_outgate_bank* k, size_t bytes) {
    if (bytes <= k->pin_bytes) return RY_OK;
    if (k->up_pending) { RT_TRY(rt::event_sync(k->up_done)); k->up_pending = false; }
    if (k->pin) rt::hfree(k->pin);
    k->pin = nullptr; k->pin_bytes = 0;
    const size_t n = bytes + bytes / 2 + 4096;
    if (rt::hmalloc(&k->pin, n) != 0) { k->pin = nullptr; return fail(RY_ENOMEM, "host allocation of %zu staging bytes failed", n); }
    k->pin_bytes = n;
    return RY_OK;
}

// One call for all streams.  counts[b]: new samples of stream b, which lie at samples + first[b]; takes_part[b]: the stream appends and may cut.
int og_push(ry_outgate_bank* k, const double* samples, const long long* first, const int* counts_in, const unsigned char* takes_part, int on_device,
            void* out, long long out_capacity, long long* out_offsets, int* silent, double* mean_db) {
    const int B = k->n_streams, chunk = k->chunk;
    // everything that can be refused is refused here: nothing has been launched, uploaded or changed
    long long total = 0, n_new_all = 0, blocks = 0;
    int n_emit = 0;
    std::vector<OgStream>& tab = k->tab;
    tab.assign((size_t)B, OgStream());
    k->stream_of.assign((size_t)B, 0);
    for (int b = 0; b < B; ++b) {
        const OgHostStream& t = k->s[(size_t)b];
        OgStream& e = tab[(size_t)b];
        memset(&e, 0, sizeof e);
        const long long n = takes_part[b] ? counts_in[b] : 0;
        const long long len = t.held + n;
        if (len > OG_MAX_SAMPLES - total) return fail(RY_EINVAL, "more than %lld samples held in one call", OG_MAX_SAMPLES);
        e.dst0 = total; e.src0 = t.off + t.start; e.new0 = first[b];
        e.keep = (int)t.held; e.n_new = (int)n;
        e.blk0 = (int)blocks; e.n_blk = (int)((len + 255) / 256);
        e.emit = -1;
        if (takes_part[b] && len >= chunk) { e.emit = n_emit; k->stream_of[(size_t)n_emit] = b; ++n_emit; }
        total += len; n_new_all += n; blocks += e.n_blk;
    }
    if ((long long)n_emit * chunk > out_capacity)
        return fail(RY_EINVAL, "out holds %lld samples, this push completes %d chunks of %d", out_capacity, n_emit, chunk);

    const ry_stream_t st = k->ctx->stream;
    long long* const cnt = k->counts;
    cnt[0] = cnt[1] = cnt[2] = cnt[3] = cnt[4] = 0;
    k->up_bytes = 0;
    out_offsets[0] = 0;
    for (int b = 0; b < B; ++b) {
        out_offsets[b + 1] = out_offsets[b] + (tab[(size_t)b].emit >= 0 ? chunk : 0);
        silent[b] = -1;
        mean_db[b] = 0.0;
    }
    if (blocks == 0 && n_emit == 0) {                              // no stream holds or brings a sample
        k->used = 0;
        for (int b = 0; b < B; ++b) k->s[(size_t)b] = OgHostStream();
        return RY_OK;
    }
    // room first: a buffer that grows waits for the stream, and a failure here leaves every stream as it was
    const int to = 1 - k->cur;
    auto grow = [&](DevBufBase& buf, long long need) { if (need > buf.cap) ++cnt[0]; return buf.grow(k->ctx, need); };
    static_assert(sizeof(OgStream) % sizeof(double) == 0 && sizeof(OgRecord) % sizeof(double) == 0, "the tables share a buffer of doubles");
    const size_t tab_d = (size_t)B * (sizeof(OgStream) / sizeof(double)), map_d = ((size_t)B + 1) / 2;
    const size_t up_d = tab_d + map_d + (on_device ? 0 : (size_t)n_new_all);
    RY_TRY(grow(k->frag(to), total));
    RY_TRY(grow(k->d_stage, (long long)up_d));
    RY_TRY(grow(k->d_inf, blocks));
    if (n_emit > 0) {
        RY_TRY(grow(k->d_db, (long long)n_emit * k->n_frames * OG_BINS));
        RY_TRY(grow(k->d_fmax, (long long)n_emit * k->n_frames));
        RY_TRY(grow(k->d_rec, n_emit));
        RY_TRY(grow(k->d_out, (long long)n_emit * chunk));             // float32 output takes the front half
    }
    RY_TRY(stage_room(k, up_d * sizeof(double)));
    if (k->up_pending) { RT_TRY(rt::event_sync(k->up_done)); k->up_pending = false; }     // the staging block's last copy (long landed)
    // ONE upload: [streams] table | [chunks] stream of each chunk | the new samples, streams back to back
    double* const stage = (double*)k->pin;
    if (!on_device) {
        long long at = 0;
        for (int b = 0; b < B; ++b) {
            OgStream& e = tab[(size_t)b];
            if (e.n_new > 0) memcpy(stage + tab_d + map_d + at, samples + first[b], (size_t)e.n_new * sizeof(double));
            e.new0 = at;
            at += e.n_new;
        }
    }
    memcpy(stage, tab.data(), (size_t)B * sizeof(OgStream));
    memcpy(stage + tab_d, k->stream_of.data(), (size_t)B * sizeof(int));
    RT_TRY(rt::h2d(k->d_stage.ptr(), stage, up_d * sizeof(double), st)); ++cnt[2];
    k->up_bytes = (long long)(up_d * sizeof(double));
    if (k->has_event) { RT_TRY(rt::event_record(k->up_done, st)); k->up_pending = true; }
    const OgStream* d_tab = (const OgStream*)k->d_stage.ptr();
    const int* d_map = (const int*)(k->d_stage.ptr() + tab_d);
    const double* d_new = on_device ? samples : k->d_stage.ptr() + tab_d + map_d;
    double* const frag = k->frag(to).ptr();
    if (blocks > 0) {
        OgAppendParams ap;
        memset(&ap, 0, sizeof ap);
        ap.tab = d_tab; ap.n_streams = B; ap.old_frag = k->frag(k->cur).ptr(); ap.fresh = d_new; ap.frag = frag; ap.chunk = chunk;
        ap.inf_part = k->d_inf.ptr();
        RY_LAUNCH(og_append, dim3((unsigned)blocks), 256, st, ap); ++cnt[1];
        RT_TRY(rt::last_error());
    }
    k->cur = to; k->used = total;
    for (int b = 0; b < B; ++b) {
        OgHostStream& t = k->s[(size_t)b];
        const OgStream& e = tab[(size_t)b];
        const long long len = (long long)e.keep + e.n_new;
        t.off = e.dst0; t.start = e.emit >= 0 ? chunk : 0; t.held = len - t.start;
    }
    if (n_emit == 0) return RY_OK;

    OgFrameParams fp;
    memset(&fp, 0, sizeof fp);
    fp.tab = d_tab; fp.stream_of = d_map; fp.frag = frag; fp.chunk = chunk; fp.n_frames = k->n_frames;
    fp.tw1024 = k->tw1024; fp.tw2048 = k->tw2048; fp.db = k->d_db.ptr(); fp.fmax = k->d_fmax.ptr();
    RY_LAUNCH(og_frame_db, dim3((unsigned)((long long)n_emit * k->n_frames)), 256, st, fp); ++cnt[1];
    RT_TRY(rt::last_error());
    OgFinishParams np;
    memset(&np, 0, sizeof np);
    np.tab = d_tab; np.stream_of = d_map; np.db = k->d_db.ptr(); np.fmax = k->d_fmax.ptr(); np.inf_part = k->d_inf.ptr();
    np.n_frames = k->n_frames; np.threshold_db = k->threshold_db; np.rec = k->d_rec.ptr();
    RY_LAUNCH(og_finish, dim3((unsigned)n_emit), 256, st, np); ++cnt[1];
    RT_TRY(rt::last_error());
    OgEmitParams ep;
    memset(&ep, 0, sizeof ep);
    ep.tab = d_tab; ep.stream_of = d_map; ep.rec = k->d_rec.ptr(); ep.frag = frag; ep.chunk = chunk; ep.total = (long long)n_emit * chunk;
    ep.scale = k->scale;
    if (k->out_f32) ep.out32 = (float*)k->d_out.ptr(); else ep.out64 = k->d_out.ptr();
    RY_LAUNCH(og_emit, dim3((unsigned)((ep.total + 255) / 256)), 256, st, ep); ++cnt[1];
    RT_TRY(rt::last_error());
    k->rec.resize((size_t)n_emit);
    RT_TRY(rt::d2h(k->rec.data(), k->d_rec.ptr(), (size_t)n_emit * sizeof(OgRecord), st)); ++cnt[3];
    RT_TRY(rt::stream_sync(st)); ++cnt[0];                          // wait 1 of 2: the records of all chunks
    k->up_pending = false;
    const size_t elem = k->out_f32 ? sizeof(float) : sizeof(double);
    bool any = false;
    for (int c = 0; c < n_emit; ++c) {
        const int b = k->stream_of[(size_t)c];
        const OgRecord& r = k->rec[(size_t)c];
        silent[b] = r.silent ? 1 : 0;
        mean_db[b] = r.mean_db;
        if (r.silent) continue;
        RT_TRY(rt::d2h((char*)out + (size_t)out_offsets[b] * elem, (const char*)k->d_out.ptr() + (size_t)c * chunk * elem, (size_t)chunk * elem, st));
        ++cnt[3]; cnt[4] += (long long)chunk * (long long)elem;
        any = true;
    }
    if (any) { RT_TRY(rt::stream_sync(st)); ++cnt[0]; }              // wait 2 of 2: the audible chunks
    return RY_OK;
}

int poison(ry_outgate_bank* k) {
    const ry_stream_t st = k->ctx->stream;
    for (DevBufBase* b : k->scratch) RY_TRY(b->poison(st));
    RY_TRY(k->frag(1 - k->cur).poison(st));
    DevBuf<double>& f = k->frag(k->cur);
    if (f.raw) {
        RT_TRY(rt::dmemset(f.ptr() + k->used, 0xff, (size_t)(f.cap - k->used) * sizeof(double), st));
        for (const OgHostStream& t : k->s)                          // what a cut chunk left in front of a remainder
            if (t.start > 0) RT_TRY(rt::dmemset(f.ptr() + t.off, 0xff, (size_t)t.start * sizeof(double), st));
    }
    RT_TRY(rt::stream_sync(st));
    k->up_pending = false;
    return RY_OK;
}

void reset_streams(ry_outgate_bank* k, int b0, int b1) {
    for (int b = b0; b < b1; ++b) { k->s[(size_t)b].held = 0; k->s[(size_t)b].start = 0; }      // the place stays: the next call moves nothing out of it
}
}  // namespace

extern "C" {

int ry_outgate_bank_create(ry_ctx* ctx, int n_streams, int chunk, double threshold_db, double scale, int out_f32, ry_outgate_bank** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    if (!ctx) return fail(RY_EINVAL, "null context");
    if (n_streams < 1 || n_streams > OG_MAX_STREAMS) return fail(RY_EINVAL, "%d streams: 1 .. %d", n_streams, (int)OG_MAX_STREAMS);
    if (chunk < OG_BINS) return fail(RY_EINVAL, "a chunk of %d samples: at least %d (reflect padding of %d samples on each side must not wrap twice)", chunk, OG_BINS, OG_PAD);
    if (chunk > OG_MAX_CHUNK) return fail(RY_EINVAL, "a chunk of %d samples: at most %d", chunk, (int)OG_MAX_CHUNK);
    if (threshold_db != threshold_db) return fail(RY_EINVAL, "the threshold is NaN");
    if (scale != scale) return fail(RY_EINVAL, "the scale is NaN");
    RT_TRY(rt::set_device(ctx->device));
    std::unique_ptr<ry_outgate_bank> k(new ry_outgate_bank());
    k->ctx = ctx; k->n_streams = n_streams; k->chunk = chunk; k->n_frames = 1 + chunk / OG_HOP; k->out_f32 = out_f32 ? 1 : 0;
    k->threshold_db = threshold_db; k->scale = scale;
    k->s.resize((size_t)n_streams);
    const std::vector<double> t1 = twiddles(SYNTH_FFT), t2 = twiddles(OG_FFT);
    RY_TRY(upload_table(k->tables, ctx, (const sy_c*)t1.data(), (size_t)SYNTH_FFT, &k->tw1024));
    RY_TRY(upload_table(k->tables, ctx, (const sy_c*)t2.data(), (size_t)OG_FFT, &k->tw2048));
    RT_TRY(rt::event_create_fast(&k->up_done));
    k->has_event = true;
    *out = k.release();
    return RY_OK;
}

void ry_outgate_bank_destroy(ry_outgate_bank* k) {
    if (!k) return;
    rt::set_device(k->ctx->device);
    rt::stream_sync(k->ctx->stream);
    if (k->has_event) rt::event_destroy(k->up_done);
    if (k->pin) rt::hfree(k->pin);
    delete k;
}

int ry_outgate_bank_reset(ry_outgate_bank* k, int stream) {
    RY_TRY(check_handle(k, "output gate bank"));
    if (stream < -1 || stream >= k->n_streams) return fail(RY_EINVAL, "stream %d of %d", stream, k->n_streams);
    reset_streams(k, stream < 0 ? 0 : stream, stream < 0 ? k->n_streams : stream + 1);
    return RY_OK;
}

int ry_outgate_bank_held(ry_outgate_bank* k, int stream) {
    if (!k || stream < 0 || stream >= k->n_streams) return fail(RY_EINVAL, "bad argument");
    return (int)k->s[(size_t)stream].held;
}

int ry_outgate_bank_push(ry_outgate_bank* k, const double* samples, const long long* sample_offsets, int on_device, void* out, long long out_capacity,
                         long long* out_offsets, int* silent, double* mean_db) {
    RY_TRY(check_handle(k, "output gate bank"));
    if (!samples || !sample_offsets || !out || !out_offsets || !silent || !mean_db)
        return fail(RY_EINVAL, "null samples / sample_offsets / out / out_offsets / silent / mean_db");
    if (out_capacity < 0) return fail(RY_EINVAL, "out_capacity %lld", out_capacity);
    const int B = k->n_streams;
    if (sample_offsets[0] != 0) return fail(RY_EINVAL, "sample_offsets starts at %lld, not 0", sample_offsets[0]);
    std::vector<int> n((size_t)B);
    std::vector<unsigned char> part((size_t)B);
    for (int b = 0; b < B; ++b) {
        const long long d = sample_offsets[b + 1] - sample_offsets[b];
        if (d < 0) return fail(RY_EINVAL, "stream %d has %lld samples", b, d);
        if (d > OG_MAX_SAMPLES) return fail(RY_EINVAL, "stream %d: more than %lld samples held in one call", b, OG_MAX_SAMPLES);
        n[(size_t)b] = (int)d; part[(size_t)b] = d > 0;             // a stream without a new sample sits the call out
    }
    return og_push(k, samples, sample_offsets, n.data(), part.data(), on_device, out, out_capacity, out_offsets, silent, mean_db);
}

int ry_outgate_bank_debug_counts(ry_outgate_bank* k, long long* out) {
    if (!k || !out) return fail(RY_EINVAL, "bad argument");
    for (int i = 0; i < 5; ++i) out[i] = k->counts[i];
    return RY_OK;
}

long long ry_outgate_bank_debug_upload_bytes(ry_outgate_bank* k) {
    if (!k) return fail(RY_EINVAL, "bad argument");
    return k->up_bytes;
}

int ry_outgate_bank_debug_poison(ry_outgate_bank* k) {
    RY_TRY(check_handle(k, "output gate bank"));
    return poison(k);
}

// ---- the lone gate: a bank of one stream whose every push takes part (an empty push cuts the next chunk of a backlog) ----------------------
int ry_outgate_create(ry_ctx* ctx, int chunk, double threshold_db, double scale, int out_f32, ry_outgate** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    ry_outgate_bank* k = nullptr;
    RY_TRY(ry_outgate_bank_create(ctx, 1, chunk, threshold_db, scale, out_f32, &k));
    *out = new ry_outgate();
    (*out)->k = k;
    return RY_OK;
}

void ry_outgate_destroy(ry_outgate* h) {
    if (!h) return;
    ry_outgate_bank_destroy(h->k);
    delete h;
}

int ry_outgate_reset(ry_outgate* h) {
    if (!h) return fail(RY_ESTATE, "null output gate handle");
    return ry_outgate_bank_reset(h->k, 0);
}

int ry_outgate_held(ry_outgate* h) {
    if (!h) return fail(RY_EINVAL, "bad argument");
    return ry_outgate_bank_held(h->k, 0);
}

int ry_outgate_push(ry_outgate* h, const double* samples, int n, int on_device, void* out, int out_capacity, int* n_out, int* silent, double* mean_db) {
    if (!h) return fail(RY_ESTATE, "null output gate handle");
    RY_TRY(check_handle(h->k, "output gate"));
    if (n_out) *n_out = 0;
    if (!out || !n_out || !silent || !mean_db) return fail(RY_EINVAL, "null out / n_out / silent / mean_db");
    if (n < 0) return fail(RY_EINVAL, "%d samples", n);
    if (n > 0 && !samples) return fail(RY_EINVAL, "null samples");
    if (out_capacity < 0) return fail(RY_EINVAL, "out_capacity %d", out_capacity);
    const long long first[2] = {0, n};
    const unsigned char part = 1;
    long long off[2] = {0, 0};
    int sil = -1;
    double mean = 0.0;
    RY_TRY(og_push(h->k, samples, first, &n, &part, on_device, out, out_capacity, off, &sil, &mean));
    *n_out = (int)(off[1] - off[0]);
    *silent = sil > 0 ? 1 : 0;
    *mean_db = mean;
    return RY_OK;
}

int ry_outgate_debug_counts(ry_outgate* h, long long* out) {
    if (!h) return fail(RY_EINVAL, "bad argument");
    return ry_outgate_bank_debug_counts(h->k, out);
}

long long ry_outgate_debug_upload_bytes(ry_outgate* h) {
    if (!h) return fail(RY_EINVAL, "bad argument");
    return ry_outgate_bank_debug_upload_bytes(h->k);
}

int ry_outgate_debug_poison(ry_outgate* h) {
    if (!h) return fail(RY_ESTATE, "null output gate handle");
    return ry_outgate_bank_debug_poison(h->k);
}

}  // extern "C"
