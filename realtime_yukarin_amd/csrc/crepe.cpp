// crepe.cpp -- the CREPE pitch tracker of libry355.so (`crepe.predict(..., viterbi=True)`, called by the reference's
// CrepeAcousticFeatureWrapper.extract_f0): framing -> conv1 .. conv6 (conv -> ReLU -> BN -> max-pool 2, one implicit-GEMM kernel each,
// split-K where the grid is short) -> dense + sigmoid -> argmax / Viterbi / local-average cents.  Kernels: crepe_kernels.h.
// The frames of a call run in passes of at most CHUNK frames; the activation of every frame is kept for the decode, which runs once.
// Audio at another rate is resampled to 16 kHz on the device first (crepe_resample; the filter and the time register of each rate are
// tables the caller installs, ry_crepe_set_resampler).
// ry_crepe_voicing turns the decode's (confidence, f0) into the voiced mask, the masked float64 f0 and the time axis (crepe_voicing: the two-state HMM
// of `predict_voicing`); ry_crepe_track is predict + voicing in one enqueue, the track left on the card for ry_analysis_extract_dev.
// ry_crepe_track_many is ry_crepe_track for a list of waves in one enqueue: the waves are uploaded back to back with a segment table (CrepeSeg), the
// resampler runs over all of them, their frames share the passes of CHUNK, and the decode and the voicing run one workgroup per track.
// ry_crepe_set_dtype(2) runs the seven GEMMs in split-bf16 form (crepe_igemm_x3) on filters split once into two bf16 planes; everything else is shared.
// ry_crepe_stream_track is ry_crepe_track window by window over a live signal: the activation rows of the frames a window shares with the previous
// one are kept on the card (two blocks used in turn), only the other frames run through the network (crepe_frames with a frame index list), and
// crepe_act_assemble builds the window's block from both (DESIGN.md section 18 states which rows may be kept).
// ry_crepe_bank_track is ry_crepe_track_many over the next windows of several such streams: every stream has a pair of slots of its own, the
// computed frames of all waves share the passes, and crepe_act_assemble_many builds every wave's block in one launch.
// The four tracking bodies are the same steps over one TrackCall -- size_call, reserve_call, bring_up, finish_track -- plus what is theirs alone; a
// stream and every stream of a bank keep their rows in a Slot.
#include "crepe_kernels.h"
#include "ry_host.h"

namespace {
const int MULT_MAX = 32;                            // capacities: tiny 4, small 8, medium 16, large 24, full 32 (any 1 .. 32 is accepted)
const int NCONV = 6;
const int FILTERS[NCONV] = {32, 4, 4, 4, 8, 16};    // x multiplier
const int WIDTHS[NCONV] = {512, 64, 64, 64, 64, 64};
const int STRIDES[NCONV] = {4, 1, 1, 1, 1, 1};
const int PAD_L = 31, PAD_R = 32;                   // Keras 'same' for width 64 (conv1: 254 / 254, stored in the frame row)
const int CHUNK = 256;                              // frames per pass through the network
const int PLAN_FRAMES = 201;                        // split-K counts are planned for one second at 5 ms and then fixed per layer:
                                                    // every frame's sums run in the same order whatever the length of the call
const int PLAN_WORKGROUPS = 1000;

struct CLayer {
    int cin = 0, cout = 0, width = 0, stride = 1;
    int lin = 0, lout = 0, K = 0;                   // lout: positions before the pool (dense: 1)
    int splits = 1;                                 // split-K count of the fp32 kernel (chunks of CREPE_BK)
    int splits_x3 = 1;                              // ... of the split-bf16 kernel (chunks of CREPE_X3_BK)
    size_t w_off = 0;                               // this layer's filters in the bf16 planes w_hi / w_lo (elements)
    int in_fstride = 0, in_rstride = 0;             // input frame stride / window step (floats)
    int out_fstride = 0, out_off = 0;               // pooled output: frame stride / offset of position 0 (floats)
    float *w = nullptr, *b = nullptr, *sc = nullptr, *sh = nullptr;
};

size_t param_count(int m) {
    size_t n = 0;
    int cin = 1;
    for (int i = 0; i < NCONV; ++i) {
        const size_t c = (size_t)FILTERS[i] * m;
        n += c * cin * WIDTHS[i] + 5 * c;
        cin = (int)c;
    }
    return n + (size_t)CREPE_BINS * 4 * cin + CREPE_BINS;
}

// the resampler tables of one input rate (ry_crepe_set_resampler)
struct Resampler {
    double* win = nullptr;                          // half filter [n_win]
    double* tr = nullptr;                           // time register [n_times]
    int n_win = 0, num_table = 0, step = 0, n_times = 0;
    std::vector<double> tr_host;                    // the same on the host: the input sample each output starts from is checked before a launch
};
}  // namespace

struct ry_crepe {
    ry_ctx* ctx = nullptr;
    int m = 0;
    CLayer L[NCONV + 1];                            // conv1 .. conv6, dense
    Arena weights;
    double *logT = nullptr, *logE = nullptr, *logS = nullptr;
    // pass buffers (CHUNK frames at most): frame rows, the padded input of each conv layer after the first, the dense input, logits, slabs
    Arena bufs;
    int cap_chunk = 0;
    float* act_in[NCONV + 1] = {};                  // act_in[0] = frames, act_in[i] = input of layer i (conv i + 1 / dense)
    float* logits = nullptr;
    float* slabs = nullptr;
    size_t slab_floats = 0;
    int last_chunk = 0;                             // frames of the last pass (ry_crepe_debug_layer)
    // call buffers, each as long as the longest call so far needed it: the audio at 16 kHz (uploaded, or the resampler's output), the uploaded
    // input at another rate, and one entry / one row per frame of a call
    DevBufList call;
    DevBuf<float> audio{call}, audio_sr{call}, act{call}, conf{call}, f0{call};
    DevBuf<int> obs{call}, bp{call}, path{call};
    // voicing: the HMM's constants (they travel as kernel arguments), its back-pointer bytes, and the masked track of the last call
    CrepeVoicingTables vt;
    DevBuf<unsigned char> v_bp{call}, voiced{call};
    DevBuf<double> f0_64{call}, t_64{call};
    // what the last ry_crepe_track left on the card (ry_crepe_track_buffers); every other call that writes one of these buffers forgets it
    const float* trk_wave = nullptr;
    int trk_samples = 0, trk_frames = 0;
    // many waves in one call: the segment table on the card and on the host, and what the last ry_crepe_track_many left (ry_crepe_track_many_buffers):
    // the first sample / first frame of every wave and one entry behind the last, n_waves + 1 each; trk_waves = 0: no such track
    DevBuf<CrepeSeg> segs{call};
    std::vector<CrepeSeg> seg_host;
    std::vector<long long> trk_sample_off;
    std::vector<int> trk_frame_off;
    int trk_waves = 0;
    // ry_crepe_upload_waves: the waves it left on the card at the caller's rate (in `audio` at 16 kHz, else in `audio_sr`), where each starts (waves + 1
    // entries; empty: no such table) and their rate; what the last ry_crepe_track_uploaded / ry_crepe_bank_track_uploaded tracked of them
    // (ry_crepe_uploaded_buffers).  Every other call that writes a call buffer forgets the table with the tracks.
    const float* up_wave = nullptr;
    std::vector<long long> up_off;
    int up_sr = 0;
    std::vector<int> sub_frame_off;
    int sub_waves = 0;
    long long net_frames = 0;                       // frames that went through the network so far (ry_crepe_debug_frames)
    // resampling: tables per input rate
    Arena rs_tables;
    std::map<int, Resampler> rs;
    int rs_epoch = 0;                               // counts the filter tables installed: rows a stream kept under another filter are not reused
    // ry_crepe_set_dtype: 0 = fp32 MFMA, 2 = split-bf16.  The filters of every layer as two bf16 planes (layer i at L[i].w_off), built at the
    // first switch to 2.  They are weights: a list of their own, which ry_crepe_debug_poison does not walk.
    int dtype = 0;
    DevBufList planes;
    DevBuf<unsigned short> w_hi{planes}, w_lo{planes};
    bool planes_built = false;
    int splits_of(int i) const { return dtype == 2 ? L[i].splits_x3 : L[i].splits; }
};

namespace {
// What the rule of DESIGN.md section 18 needs of the call a stream keeps rows of: which of its two blocks holds them, its frames, samples at the
// caller's rate and at 16 kHz, rate, hop, arithmetic, filter table, and which frames were portable.  One per single stream, one per slot of a bank.
struct KeptCall {
    bool valid = false;
    int kept = 0, nf = 0, n_in = 0, n16 = 0, sr = 0, hop = 0, dtype = 0, rs_epoch = 0;
    std::vector<char> portable;
};

// What the rule needs of a window length / an advance, remembered: the portable frames of (rate, samples, hop), the verdict of the register
// check of (rate, advance, outputs checked).  Both follow from the rate's tables alone and are dropped when the filter changes.  One per single
// stream, one per bank (its streams share it: nothing in it depends on the stream).
struct RuleCache {
    std::map<std::tuple<int, int, int>, std::vector<char>> portable_of;
    std::map<std::tuple<int, int, int>, bool> repeats_of;
    int epoch = 0;
};

// The kept rows of one stream, single or of a bank: two activation blocks used in turn by the calls the stream takes part in, and the call
// whose rows one of them holds.
struct Slot {
    DevBuf<float> act0, act1;
    KeptCall k;
    explicit Slot(DevBufList& l) : act0(l), act1(l) {}
    DevBuf<float>& act(int i) { return i ? act1 : act0; }
    int next() const { return k.valid ? 1 - k.kept : 0; }   // the block the next call writes: the other one, so the kept rows do not move
    const float* keep() { return k.valid ? act(k.kept).ptr() : nullptr; }
    int n_keep() const { return k.valid ? k.nf : 0; }
};
}  // namespace

// A streaming tracker over a model (ry_crepe_stream_track): the activation rows of the last window, kept on the card for the next one.
// Nothing here is on the model's buffer list: no call on the model, ry_crepe_debug_poison included, touches what a stream keeps.
struct ry_crepe_stream {
    ry_ctx* ctx = nullptr;
    ry_crepe* model = nullptr;
    DevBufList bufs;
    Slot rows{bufs};
    DevBuf<float> fresh{bufs};                              // the packed rows of the computed frames
    DevBuf<int> tab{bufs};                                  // src [frames] | idx [computed] of the last upload
    std::vector<int> tab_host[2];                           // the tables of the last two uploads (the host array of a copy outlives the call)
    int tab_cur = -1;                                       // which of the two the card holds; -1: none
    RuleCache cache;
};

// A bank of streaming trackers over a model (ry_crepe_bank_track): every stream has a pair of activation slots of its own, used in turn by the
// calls that stream takes part in, so a stream that sits a call out finds its rows intact; the packed rows and the tables belong to the call.
// As with a stream, nothing here is on the model's buffer list.
struct ry_crepe_bank {
    ry_ctx* ctx = nullptr;
    ry_crepe* model = nullptr;
    DevBufList bufs;
    std::vector<std::unique_ptr<Slot>> slots;
    DevBuf<float> fresh{bufs};                              // the packed rows of the computed frames of all waves of a call
    // The tables of a call: descriptors [waves] (CrepeBankWave) | src [frames] | idx [computed], one copy.  In steady state the descriptors
    // alternate between two values (every stream swaps its slots from call to call), so the card holds the tables of two calls, each beside
    // its host copy (which outlives the upload), and a call whose tables equal either uploads nothing.
    DevBuf<int> tab0{bufs}, tab1{bufs};
    DevBuf<int>& tab(int i) { return i ? tab1 : tab0; }
    std::vector<int> tab_host[2];
    bool tab_on_card[2] = {false, false};
    int tab_last = 1;                                       // the one used last: the other is replaced by a call that matches neither
    long long uploads = 0;                                  // table uploads so far (tests)
    RuleCache cache;
};

namespace {
// every call that writes a buffer of the track on the card forgets it, and with it the uploaded table -- unless the call tracks waves of that table
void forget_track(ry_crepe* c, bool keep_upload = false) {
    c->trk_frames = 0; c->trk_waves = 0; c->sub_waves = 0;
    if (!keep_upload) c->up_off.clear();
}

int ensure_chunk(ry_crepe* c, int nf) {
    if (nf <= c->cap_chunk) return RY_OK;
    const int cap = nf;
    RT_TRY(rt::stream_sync(c->ctx->stream));                   // a call still in flight may use the old buffers
    c->bufs.release();
    size_t slab = 0;
    for (int i = 0; i <= NCONV; ++i) {
        const CLayer& l = c->L[i];
        const size_t in_floats = (size_t)cap * l.in_fstride;
        RY_TRY(c->bufs.alloc(&c->act_in[i], in_floats));
        RT_TRY(rt::dmemset(c->act_in[i], 0, in_floats * sizeof(float), c->ctx->stream));       // the padding rows stay zero
        const int sp = std::max(l.splits, l.splits_x3);            // one slab buffer serves both modes
        if (sp > 1) slab = std::max(slab, (size_t)sp * cap * l.lout * l.cout);
    }
    RY_TRY(c->bufs.alloc(&c->logits, (size_t)cap * CREPE_BINS));
    c->slab_floats = std::max(slab, (size_t)1);
    RY_TRY(c->bufs.alloc(&c->slabs, c->slab_floats));
    c->cap_chunk = cap;
    return RY_OK;
}

// the buffers of a call of n_frames frames over n_samples samples at 16 kHz in `audio` (0: the caller's device pointer is read): exact sizes
int ensure_call(ry_crepe* c, int n_frames, int n_samples) {
    const long long F = n_frames;
    RY_TRY(c->audio.reserve(c->ctx, n_samples));
    RY_TRY(c->act.reserve(c->ctx, F * CREPE_BINS));
    RY_TRY(c->conf.reserve(c->ctx, F));
    RY_TRY(c->f0.reserve(c->ctx, F));
    RY_TRY(c->obs.reserve(c->ctx, F));
    RY_TRY(c->path.reserve(c->ctx, F));
    RY_TRY(c->bp.reserve(c->ctx, F * CREPE_BINS));
    return RY_OK;
}

// layer i on the nf frames of a pass; `act`: the rows of this pass in the call's activation, written by the dense layer
int launch_layer(ry_crepe* c, int i, int nf, float* act) {
    const CLayer& l = c->L[i];
    const bool dense = i == NCONV;
    const bool x3 = c->dtype == 2;
    const int splits = c->splits_of(i);
    CrepeGemmParams p;
    p.x = c->act_in[i]; p.w = l.w; p.bias = l.b; p.scale = l.sc; p.shift = l.sh;
    p.M = nf * l.lout; p.N = l.cout; p.K = l.K; p.lout = l.lout;
    p.in_fstride = l.in_fstride; p.in_rstride = l.in_rstride;
    p.out_fstride = l.out_fstride; p.out_off = l.out_off; p.splits = splits;
    float* out = dense ? nullptr : c->act_in[i + 1];
    dim3 grid((unsigned)((l.cout + CREPE_BN - 1) / CREPE_BN), (unsigned)((p.M + CREPE_BM - 1) / CREPE_BM), (unsigned)splits);
    const ry_stream_t s = c->ctx->stream;
    const int epi = splits > 1 ? CREPE_EPI_RAW : dense ? CREPE_EPI_SIG : CREPE_EPI_POOL;
    p.y = epi == CREPE_EPI_RAW ? c->slabs : dense ? act : out;
    p.y2 = epi == CREPE_EPI_SIG ? c->logits : nullptr;
    CrepeX3Params px;
    px.g = p; px.w_hi = x3 ? c->w_hi.ptr() + l.w_off : nullptr; px.w_lo = x3 ? c->w_lo.ptr() + l.w_off : nullptr;
    switch (i * 3 + epi) {
#define CREPE_CASE(L, E) case (L) * 3 + (E):                                          \
        if (x3) RY_LAUNCH((crepe_igemm_x3<E, L + 1>), grid, 256, s, px);              \
        else RY_LAUNCH((crepe_igemm<E, L + 1>), grid, 256, s, p);                     \
        break;
        CREPE_CASE(0, CREPE_EPI_POOL) CREPE_CASE(1, CREPE_EPI_POOL) CREPE_CASE(2, CREPE_EPI_POOL)
        CREPE_CASE(3, CREPE_EPI_POOL) CREPE_CASE(4, CREPE_EPI_POOL) CREPE_CASE(5, CREPE_EPI_POOL)
        CREPE_CASE(0, CREPE_EPI_RAW) CREPE_CASE(1, CREPE_EPI_RAW) CREPE_CASE(2, CREPE_EPI_RAW) CREPE_CASE(3, CREPE_EPI_RAW)
        CREPE_CASE(4, CREPE_EPI_RAW) CREPE_CASE(5, CREPE_EPI_RAW) CREPE_CASE(6, CREPE_EPI_RAW) CREPE_CASE(6, CREPE_EPI_SIG)
#undef CREPE_CASE
        default: return fail(RY_EINVAL, "crepe layer %d epilogue %d", i, epi);
    }
    RT_TRY(rt::last_error());
    if (epi != CREPE_EPI_RAW) return RY_OK;
    if (dense) {
        CrepeReduceSigParams r;
        r.slabs = c->slabs; r.bias = l.b; r.act = act; r.logits = c->logits; r.M = p.M; r.N = l.cout; r.splits = splits;
        dim3 g((unsigned)(((long long)p.M * l.cout + 255) / 256));
        RY_LAUNCH(crepe_reduce_sig, g, 256, s, r);
    } else {
        CrepeReducePoolParams r;
        r.slabs = c->slabs; r.bias = l.b; r.scale = l.sc; r.shift = l.sh; r.y = out;
        r.M = p.M; r.N = l.cout; r.lout = l.lout; r.out_fstride = l.out_fstride; r.out_off = l.out_off; r.splits = splits;
        dim3 g((unsigned)(((long long)(p.M / 2) * l.cout + 255) / 256));
        RY_LAUNCH(crepe_reduce_pool, g, 256, s, r);
    }
    RT_TRY(rt::last_error());
    return RY_OK;
}

// `seg` (device) / n_seg: the tracks of a segment table, nf frames in all; null: one track
int launch_decode(ry_crepe* c, const float* act, int nf, int viterbi, const CrepeSeg* seg = nullptr, int n_seg = 1) {
    const ry_stream_t s = c->ctx->stream;
    CrepeArgmaxParams ap;
    ap.act = act; ap.n_frames = nf; ap.obs = c->obs.ptr(); ap.conf = c->conf.ptr();
    RY_LAUNCH(crepe_argmax, dim3((unsigned)((nf + 3) / 4)), 256, s, ap);
    RT_TRY(rt::last_error());
    CrepeDecodeParams dp;
    dp.act = act; dp.obs = c->obs.ptr(); dp.n_frames = nf; dp.viterbi = viterbi ? 1 : 0;
    dp.logT = c->logT; dp.logE = c->logE; dp.logS = c->logS; dp.bp = c->bp.ptr(); dp.path = c->path.ptr(); dp.f0 = c->f0.ptr();
    dp.seg = seg;
    RY_LAUNCH(crepe_decode, dim3((unsigned)n_seg), 384, s, dp);
    RT_TRY(rt::last_error());
    return RY_OK;
}

// frames of n_samples at 16 kHz; refuses what ry_crepe_predict refuses
int frame_count(int n_samples, int hop, int center, int* nf) {
    if (!center && n_samples < CREPE_FRAME) return fail(RY_EINVAL, "center = 0 needs at least %d samples, got %d", CREPE_FRAME, n_samples);
    const long long nfl = 1 + ((long long)n_samples + (center ? CREPE_FRAME : 0) - CREPE_FRAME) / hop;
    if (nfl > (1LL << 24)) return fail(RY_EINVAL, "%lld frames", nfl);
    *nf = (int)nfl;
    return RY_OK;
}

// The network on n rows in passes of CHUNK: row b is frame b of the call, or frame idx[b] of it (`idx`: a device list of n frame indices, packed
// back to back); the dense layer writes row b of `rows`.  ensure_chunk has run.
int run_passes(ry_crepe* c, const float* d_audio, int n_samples, int hop, int center, int n, const int* idx, float* rows,
               const CrepeSeg* seg = nullptr, int n_seg = 1) {
    const ry_stream_t s = c->ctx->stream;
    for (int f = 0; f < n; f += CHUNK) {
        const int k = std::min(CHUNK, n - f);
        CrepeFrameParams fp;
        fp.audio = d_audio; fp.n = n_samples; fp.hop = hop; fp.center = center; fp.frame0 = f; fp.n_frames = k; fp.out = c->act_in[0];
        fp.seg = seg; fp.n_seg = n_seg; fp.idx = idx;
        RY_LAUNCH(crepe_frames, dim3((unsigned)k), 256, s, fp);
        RT_TRY(rt::last_error());
        for (int i = 0; i <= NCONV; ++i) RY_TRY(launch_layer(c, i, k, rows + (size_t)f * CREPE_BINS));
        c->last_chunk = k;
        c->net_frames += k;
    }
    return RY_OK;
}

// the network and the decode on n_samples at 16 kHz in device memory, results to the caller (ensure_chunk / ensure_call have run)
int run_network(ry_crepe* c, const float* d_audio, int n_samples, int hop, int center, int viterbi, int nf,
                float* f0, float* confidence, float* activation, int on_device, const CrepeSeg* seg = nullptr, int n_seg = 1) {
    const ry_stream_t s = c->ctx->stream;
    float* act_all = c->act.ptr();
    RY_TRY(run_passes(c, d_audio, n_samples, hop, center, nf, nullptr, act_all, seg, n_seg));
    RY_TRY(launch_decode(c, act_all, nf, viterbi, seg, n_seg));
    if (!f0 && !confidence && !activation) return RY_OK;                // ry_crepe_track: the results stay in the handle's buffers
    if (on_device) {
        RT_TRY(rt::d2d(f0, c->f0.ptr(), (size_t)nf * sizeof(float), s));
        RT_TRY(rt::d2d(confidence, c->conf.ptr(), (size_t)nf * sizeof(float), s));
        if (activation) RT_TRY(rt::d2d(activation, act_all, (size_t)nf * CREPE_BINS * sizeof(float), s));
        return RY_OK;
    }
    RT_TRY(rt::d2h(f0, c->f0.ptr(), (size_t)nf * sizeof(float), s));
    RT_TRY(rt::d2h(confidence, c->conf.ptr(), (size_t)nf * sizeof(float), s));
    if (activation) RT_TRY(rt::d2h(activation, act_all, (size_t)nf * CREPE_BINS * sizeof(float), s));
    RT_TRY(rt::stream_sync(s));
    return RY_OK;
}

// n_out = int(n_in * (16000.0 / sr)) and the tables of the rate; refuses before anything is launched
int resample_plan(ry_crepe* c, int n_samples, int sr, const Resampler** r, int* n_out) {
    if (sr < 1) return fail(RY_EINVAL, "sample rate %d", sr);
    if (n_samples < 1) return fail(RY_EINVAL, "%d samples", n_samples);
    const auto it = c->rs.find(sr);
    if (it == c->rs.end()) return fail(RY_ESTATE, "no resampler tables for %d Hz (ry_crepe_set_resampler)", sr);
    const double ratio = 16000.0 / sr;
    const double nd = (double)n_samples * ratio;
    if (!(nd < 2147483648.0)) return fail(RY_EINVAL, "%d samples at %d Hz are too many at 16 kHz", n_samples, sr);
    const int n = (int)nd;
    if (n < 1) return fail(RY_EINVAL, "%d samples at %d Hz give no sample at 16 kHz", n_samples, sr);
    if (n > it->second.n_times) return fail(RY_ESTATE, "the time table for %d Hz holds %d outputs, the call needs %d", sr, it->second.n_times, n);
    // the register never decreases (checked when it was installed): every output starts inside the signal when the last one does
    if ((long long)it->second.tr_host[(size_t)n - 1] >= n_samples)
        return fail(RY_EINVAL, "the time table for %d Hz puts output %d at input sample %lld of %d", sr, n - 1, (long long)it->second.tr_host[(size_t)n - 1], n_samples);
    *r = &it->second;
    *n_out = n;
    return RY_OK;
}

int launch_resample(ry_crepe* c, const Resampler& r, const float* d_in, int n_in, int sr, float* d_out, int n_out, const CrepeSeg* seg = nullptr, int n_seg = 1) {
    CrepeResampleParams p;
    p.x = d_in; p.n_in = n_in; p.win = r.win; p.n_win = r.n_win; p.tr = r.tr;
    const double ratio = 16000.0 / sr;
    p.scale = ratio < 1.0 ? ratio : 1.0;
    p.num_table = r.num_table; p.step = r.step; p.y = d_out; p.n_out = n_out;
    p.seg = seg; p.n_seg = n_seg;
    RY_LAUNCH(crepe_resample, dim3((unsigned)((n_out + 255) / 256)), 256, c->ctx->stream, p);
    RT_TRY(rt::last_error());
    return RY_OK;
}

// the voicing of n frames whose confidence / f0 are in device memory, into device buffers (the handle's own, or a device caller's)
int launch_voicing(ry_crepe* c, const float* conf, const float* f0, int n, double threshold, double step_ms,
                   unsigned char* voiced, double* f0_64, double* t_64, const CrepeSeg* seg = nullptr, int n_seg = 1) {
    RY_TRY(c->v_bp.reserve(c->ctx, n));
    CrepeVoicingParams p;
    p.conf = conf; p.f0 = f0; p.n = n; p.threshold = (float)threshold; p.step_ms = step_ms; p.tab = c->vt;
    p.bp = c->v_bp.ptr(); p.voiced = voiced; p.f0_64 = f0_64; p.t_64 = t_64;
    p.seg = seg;
    RY_LAUNCH(crepe_voicing, dim3((unsigned)n_seg), 256, c->ctx->stream, p);
    RT_TRY(rt::last_error());
    return RY_OK;
}

int ensure_track(ry_crepe* c, int n) {
    RY_TRY(c->voiced.reserve(c->ctx, ((long long)n + 3) / 4 * 4));      // whole 32-bit words: ry_dev_download copies those
    RY_TRY(c->f0_64.reserve(c->ctx, n));
    RY_TRY(c->t_64.reserve(c->ctx, n));
    return RY_OK;
}

// The segment table of n_waves tracks of n_frames[i] frames (in_len / n16: the samples of wave i at the caller's rate and at 16 kHz; null: tracks
// alone) on the host and, one upload, on the card.  Refuses a list that is empty, a track with no frame and totals beyond what one call takes;
// nothing is launched or written before it returns RY_OK.
int plan_segments(int n_waves, const int* in_len, const int* n16, const int* n_frames, std::vector<CrepeSeg>* out) {
    if (n_waves < 1) return fail(RY_EINVAL, "%d waves", n_waves);
    out->resize((size_t)n_waves);
    long long in_off = 0, off16 = 0, frame0 = 0;
    for (int i = 0; i < n_waves; ++i) {
        if (n_frames[i] < 1) return fail(RY_EINVAL, "track %d has %d frames", i, n_frames[i]);
        CrepeSeg& g = (*out)[(size_t)i];
        g.in_off = (int)in_off; g.in_len = in_len ? in_len[i] : 0; g.off16 = (int)off16; g.n16 = n16 ? n16[i] : 0;
        g.frame0 = (int)frame0; g.n_frames = n_frames[i];
        in_off += g.in_len; off16 += g.n16; frame0 += g.n_frames;
        // the offsets are 32-bit on the card: a list whose samples or frames do not fit is refused, as the single calls refuse their sizes
        if (in_off > 2147483647LL || off16 > 2147483647LL) return fail(RY_EINVAL, "the waves up to %d hold %lld samples (%lld at 16 kHz): too many for one call", i, in_off, off16);
        if (frame0 > (1LL << 24)) return fail(RY_EINVAL, "%lld frames in one call", frame0);
    }
    return RY_OK;
}

int upload_segments(ry_crepe* c, const std::vector<CrepeSeg>& plan) {
    RY_TRY(c->segs.reserve(c->ctx, (long long)plan.size()));
    c->seg_host = plan;                                                 // the handle's copy: the host array of the upload outlives the call
    RT_TRY(rt::h2d(c->segs.ptr(), c->seg_host.data(), c->seg_host.size() * sizeof(CrepeSeg), c->ctx->stream));
    return RY_OK;
}

// The one upload of a call: total_in samples at the caller's rate into `audio` (16 kHz: the network reads them there) or `audio_sr` (r: the
// resampler reads them there) -> where they lie.
int upload_audio(ry_crepe* c, const Resampler* r, const float* audio, int total_in, float** wave) {
    if (r) RY_TRY(c->audio_sr.reserve(c->ctx, total_in));
    else RY_TRY(c->audio.reserve(c->ctx, total_in));
    *wave = r ? c->audio_sr.ptr() : c->audio.ptr();
    RT_TRY(rt::h2d(*wave, audio, (size_t)total_in * sizeof(float), c->ctx->stream));
    return RY_OK;
}

// The segments of a call over waves ry_crepe_upload_waves left on the card: entry i of the table (first sample, samples) must BE one of the uploaded
// waves, the entries ascend, the rate is the upload's.  The samples are read where they lie (in_off; at 16 kHz off16 too: the network reads the
// upload itself), the 16 kHz samples and the frames of the tracked waves are packed as those of a call on these waves alone.
int place_uploaded(const ry_crepe* c, const int* first_sample, const int* n_samples, int n_waves, int sr, std::vector<CrepeSeg>* plan) {
    if (c->up_off.empty()) return fail(RY_ESTATE, "no waves on the card: ry_crepe_upload_waves has not run, or a later call reused its buffers");
    if (sr != c->up_sr) return fail(RY_EINVAL, "the waves were uploaded at %d Hz, the call says %d", c->up_sr, sr);
    long long end = 0;
    for (int i = 0; i < n_waves; ++i) {
        const long long a = first_sample[i];
        if (a < end) return fail(RY_EINVAL, "wave %d starts at sample %lld, before the end of the one in front of it: the table must ascend", i, a);
        const auto it = std::lower_bound(c->up_off.begin(), c->up_off.end() - 1, a);
        if (it == c->up_off.end() - 1 || *it != a || *(it + 1) - a != (long long)n_samples[i])
            return fail(RY_EINVAL, "wave %d (%d samples from %lld) is not a wave of the uploaded table", i, n_samples[i], a);
        CrepeSeg& g = (*plan)[(size_t)i];
        g.in_off = (int)a;
        if (sr == 16000) g.off16 = (int)a;
        end = a + n_samples[i];
    }
    return RY_OK;
}

int voicing_args(double threshold, double step_ms) {
    if (std::isnan(threshold)) return fail(RY_EINVAL, "threshold %g", threshold);
    if (!std::isfinite(step_ms) || !(step_ms > 0.0)) return fail(RY_EINVAL, "step %g ms", step_ms);
    return RY_OK;
}

// ---- the steps of a tracking call (ry_crepe_track, _track_many / _track_uploaded, _stream_track, _bank_track / _bank_track_uploaded) ----
// The sizes of a call and, once bring_up has run, where its samples and its segment table lie on the card (one wave: no table, plan is empty).
struct TrackCall {
    int sr = 0, hop = 0, total_in = 0, total16 = 0, total_nf = 0;
    const Resampler* r = nullptr;                   // null at 16 kHz
    std::vector<int> n16, nf;                       // samples at 16 kHz / frames of every wave
    std::vector<CrepeSeg> plan;
    bool uploaded = false;                          // the waves are those ry_crepe_upload_waves left on the card
    float* wave = nullptr;
    const CrepeSeg* seg = nullptr;
    int n_seg() const { return plan.empty() ? 1 : (int)plan.size(); }
};

// Every refusal of a list of waves: each wave is held to what ry_crepe_track asks of it (and to wave_ok(i), the caller's own, before the next
// wave is looked at), the list to the sizes one call takes; first_sample: the waves are entries of the uploaded table, else null.  Host work only.
int any_wave(int) { return RY_OK; }
template <typename WaveOk>
int size_call(ry_crepe* c, const int* first_sample, const int* n_samples, int n_waves, int sr, int hop, TrackCall* z, WaveOk wave_ok) {
    z->sr = sr; z->hop = hop; z->uploaded = first_sample != nullptr;
    z->n16.assign(n_samples, n_samples + n_waves); z->nf.resize((size_t)n_waves);
    for (int i = 0; i < n_waves; ++i) {
        if (n_samples[i] < 1) return fail(RY_EINVAL, "wave %d has %d samples", i, n_samples[i]);
        if (sr != 16000) RY_TRY(resample_plan(c, n_samples[i], sr, &z->r, &z->n16[(size_t)i]));
        RY_TRY(frame_count(z->n16[(size_t)i], hop, 1, &z->nf[(size_t)i]));
        RY_TRY(wave_ok(i));
    }
    RY_TRY(plan_segments(n_waves, n_samples, z->n16.data(), z->nf.data(), &z->plan));
    if (z->uploaded) RY_TRY(place_uploaded(c, first_sample, n_samples, n_waves, sr, &z->plan));
    const CrepeSeg& last = z->plan.back();
    z->total_in = last.in_off + last.in_len; z->total16 = last.off16 + last.n16; z->total_nf = last.frame0 + last.n_frames;
    return RY_OK;
}

// one wave, tracked without a table (n_samples < 1 is refused by the caller, in its own words)
int size_call(ry_crepe* c, int n_samples, int sr, int hop, TrackCall* z) {
    RY_TRY(size_call(c, nullptr, &n_samples, 1, sr, hop, z, any_wave));
    z->plan.clear();
    return RY_OK;
}

// every buffer of the model the call needs, before its first enqueue; computed: the frames that go through the network
int reserve_call(ry_crepe* c, const TrackCall& z, int computed) {
    RY_TRY(ensure_chunk(c, std::min(computed, CHUNK)));
    RY_TRY(ensure_call(c, z.total_nf, z.total16));                     // an upload at 16 kHz lies in `audio`: it is longer than total16 and stays
    RY_TRY(ensure_track(c, z.total_nf));
    return RY_OK;
}

// The one upload of the call (the waves at the caller's rate, back to back; none when they are on the card already), the segment table of a
// list, and the resampler over all of it -> the samples at 16 kHz in `audio`.  At 16 kHz the reserve inside upload_audio finds the room
// ensure_call made: total_in == total16 there.
int bring_up(ry_crepe* c, TrackCall* z, const float* audio) {
    z->wave = const_cast<float*>(c->up_wave);
    if (!z->uploaded) RY_TRY(upload_audio(c, z->r, audio, z->total_in, &z->wave));
    if (!z->plan.empty()) {
        RY_TRY(upload_segments(c, z->plan));
        z->seg = c->segs.ptr();
    }
    if (z->r) RY_TRY(launch_resample(c, *z->r, z->wave, z->total_in, z->sr, c->audio.ptr(), z->total16, z->seg, z->n_seg()));
    return RY_OK;
}

// the masked track of n frames from the handle's buffers to the caller's, and the wait for it
int download_track(ry_crepe* c, int n, unsigned char* voiced, double* f0_64, double* t_64) {
    const ry_stream_t s = c->ctx->stream;
    RT_TRY(rt::d2h(voiced, c->voiced.ptr(), (size_t)n, s));
    RT_TRY(rt::d2h(f0_64, c->f0_64.ptr(), (size_t)n * sizeof(double), s));
    RT_TRY(rt::d2h(t_64, c->t_64.ptr(), (size_t)n * sizeof(double), s));
    RT_TRY(rt::stream_sync(s));
    return RY_OK;
}

// The end of a call whose decode is enqueued: the voicing, what the call leaves on the card (ry_crepe_track_buffers for one wave,
// ry_crepe_uploaded_buffers for waves of the uploaded table -- they are not back to back --, else ry_crepe_track_many_buffers), the frames of
// every wave to the caller, and the track too unless it stays on the card.
int finish_track(ry_crepe* c, const TrackCall& z, double threshold, double step_ms, int* n_frames, unsigned char* voiced, double* f0_64, double* t_64,
                 int on_device_out) {
    RY_TRY(launch_voicing(c, c->conf.ptr(), c->f0.ptr(), z.total_nf, threshold, step_ms, c->voiced.ptr(), c->f0_64.ptr(), c->t_64.ptr(), z.seg, z.n_seg()));
    c->trk_wave = z.wave;
    const size_t n = z.plan.size();
    if (n == 0) { c->trk_samples = z.total_in; c->trk_frames = z.total_nf; }
    else {
        c->trk_sample_off.assign(n + 1, 0);
        c->trk_frame_off.assign(n + 1, 0);
        for (size_t i = 0; i < n; ++i) {
            c->trk_sample_off[i + 1] = (long long)z.plan[i].in_off + z.plan[i].in_len;
            c->trk_frame_off[i + 1] = z.plan[i].frame0 + z.plan[i].n_frames;
        }
        if (z.uploaded) { c->sub_frame_off = c->trk_frame_off; c->sub_waves = (int)n; }
        else c->trk_waves = (int)n;
    }
    std::copy(z.nf.begin(), z.nf.end(), n_frames);
    return on_device_out ? RY_OK : download_track(c, z.total_nf, voiced, f0_64, t_64);
}

// ---- which rows of the previous window a streamed call may keep ----
// The frames of a window of n_in samples at sr (r: the rate's tables, null at 16 kHz) that are portable: the whole support [f hop - 512,
// f hop + 512) lies inside the 16 kHz signal and every output in it is clean -- neither tap loop of crepe_resample is cut by an end of the signal
// (room >= lim on both sides, in the kernel's own arithmetic on the host copy of the register).
std::vector<char> portable_frames(const Resampler* r, int sr, int n_in, int hop) {
    std::vector<char> out;
    if (n_in < 1) return out;
    int n16 = n_in;
    if (r) {
        const double nd = (double)n_in * (16000.0 / sr);
        n16 = nd < (double)r->n_times ? (int)nd : r->n_times;
    }
    if (n16 < 1) return out;
    std::vector<int> cut((size_t)n16 + 1, 0);                       // cut[t]: outputs before t that are not clean
    if (r) {
        const double ratio = 16000.0 / sr, scale = ratio < 1.0 ? ratio : 1.0;
        for (int t = 0; t < n16; ++t) {
            const double tr = r->tr_host[(size_t)t];
            const int n = (int)tr;
            const double frac0 = scale * (tr - (double)n);
            bool clean = true;
            for (int side = 0; side < 2; ++side) {
                const double frac = side ? scale - frac0 : frac0;
                const int offset = (int)(frac * (double)r->num_table);
                const int lim = (r->n_win - offset) / r->step;
                const int room = side ? n_in - n - 1 : n + 1;
                if (room < lim) clean = false;
            }
            cut[(size_t)t + 1] = cut[(size_t)t] + (clean ? 0 : 1);
        }
    }
    const int nf = 1 + n16 / hop;
    out.assign((size_t)nf, 0);
    for (int f = 0; f < nf; ++f) {
        const long long lo = (long long)f * hop - CREPE_FRAME / 2, hi = lo + CREPE_FRAME;
        if (lo >= 0 && hi <= n16 && cut[(size_t)hi] == cut[(size_t)lo]) out[(size_t)f] = 1;
    }
    return out;
}

const std::vector<char>& portable_cached(RuleCache* s, const Resampler* r, int sr, int n_in, int hop) {
    const auto key = std::make_tuple(sr, n_in, hop);
    auto it = s->portable_of.find(key);
    if (it != s->portable_of.end()) return it->second;
    if (s->portable_of.size() >= 32) s->portable_of.clear();       // a live stream repeats a handful of lengths
    return s->portable_of[key] = portable_frames(r, sr, n_in, hop);
}

// the rate's time register repeats exactly under the advance: tr[t + a16] == tr[t] + advance, as doubles, for the first n_check outputs
bool register_repeats(RuleCache* s, const Resampler& r, int sr, int advance, long long a16, int n_check) {
    const auto key = std::make_tuple(sr, advance, n_check);
    const auto it = s->repeats_of.find(key);
    if (it != s->repeats_of.end()) return it->second;
    bool ok = true;
    for (int t = 0; t < n_check && ok; ++t) {
        if (t + a16 >= r.n_times) { ok = false; break; }
        const double t_new = r.tr_host[(size_t)t], t_old = r.tr_host[(size_t)(t + a16)];
        // ... and so do the two numbers the kernel takes from it, the first tap and the fraction (a sum that rounds could pass the first test alone)
        ok = t_old == t_new + (double)advance && (int)t_old == (int)t_new + advance && t_old - (double)(int)t_old == t_new - (double)(int)t_new;
    }
    if (s->repeats_of.size() >= 32) s->repeats_of.clear();
    return s->repeats_of[key] = ok;
}

// The tables of a streamed call of nf frames over n_samples at sr: src [nf] (>= 0: the kept row; else -1 - the row of the packed block) followed
// by idx [computed] (the window frames the packed rows are computed from).  -> the number of computed frames.  Host work only.
int plan_stream(const ry_crepe* c, RuleCache* cache, const KeptCall* s, const Resampler* r, int n_samples, int sr, int hop, int nf, int advance,
                int overlap_ok, std::vector<int>* tab) {
    if (cache->epoch != c->rs_epoch) { cache->portable_of.clear(); cache->repeats_of.clear(); cache->epoch = c->rs_epoch; }
    bool reuse = s->valid && overlap_ok && advance >= 0 && advance < s->n_in && sr == s->sr && hop == s->hop && c->dtype == s->dtype &&
                 c->rs_epoch == s->rs_epoch;
    long long a16 = 0;
    int d = 0, m = 0;
    if (reuse) {
        const long long num = (long long)advance * 16000;
        a16 = num / sr;
        reuse = num % sr == 0 && a16 % hop == 0;
        d = (int)(a16 / hop);
        m = std::min(n_samples, s->n_in - advance);
    }
    const std::vector<char>* pm = nullptr;                          // the new window read as m samples long
    if (reuse) {
        pm = &portable_cached(cache, r, sr, m, hop);
        if (r && !pm->empty()) {
            const double nd = (double)m * (16000.0 / sr);
            const long long left = (long long)s->n16 - a16;
            reuse = register_repeats(cache, *r, sr, advance, a16, (int)std::max(0LL, std::min((long long)nd, left)));
        }
    }
    tab->assign((size_t)nf, 0);
    int k = 0;
    for (int j = 0; j < nf; ++j) {
        const bool keep = reuse && j < (int)pm->size() && (*pm)[(size_t)j] && j + d < s->nf && s->portable[(size_t)(j + d)];
        (*tab)[(size_t)j] = keep ? j + d : -1 - k++;
    }
    tab->resize((size_t)nf + (size_t)k);
    for (int j = 0, q = 0; j < nf; ++j)
        if ((*tab)[(size_t)j] < 0) (*tab)[(size_t)nf + (size_t)q++] = j;
    return k;
}

// the call just enqueued becomes the kept one: its rows are in block `block`
void keep_call(const ry_crepe* c, RuleCache* cache, KeptCall* k, int block, const Resampler* r, int n_samples, int n16, int sr, int hop, int nf) {
    k->kept = block; k->nf = nf; k->n_in = n_samples; k->n16 = n16; k->sr = sr; k->hop = hop; k->dtype = c->dtype; k->rs_epoch = c->rs_epoch;
    k->portable = portable_cached(cache, r, sr, n_samples, hop);
    k->valid = true;
}

int launch_assemble(ry_ctx* ctx, const float* keep, int n_keep, const float* fresh, int n_fresh, const int* src, float* out, int n_rows) {
    CrepeAssembleParams p;
    p.keep = keep; p.n_keep = n_keep; p.fresh = fresh; p.n_fresh = n_fresh; p.src = src; p.out = out; p.n_rows = n_rows;
    RY_LAUNCH(crepe_act_assemble, dim3((unsigned)((n_rows + 3) / 4)), 256, ctx->stream, p);
    RT_TRY(rt::last_error());
    return RY_OK;
}

int launch_assemble_many(ry_ctx* ctx, const CrepeSeg* seg, int n_seg, const CrepeBankWave* wave, const int* src, const float* fresh, int n_fresh,
                         float* out, int n_rows) {
    CrepeAssembleManyParams p;
    p.seg = seg; p.n_seg = n_seg; p.wave = wave; p.src = src; p.fresh = fresh; p.n_fresh = n_fresh; p.out = out; p.n_rows = n_rows;
    RY_LAUNCH(crepe_act_assemble_many, dim3((unsigned)((n_rows + 3) / 4)), 256, ctx->stream, p);
    RT_TRY(rt::last_error());
    return RY_OK;
}

// all bits set in the block of a slot about to be written and in every row of the other block that is not a portable kept row (every row when
// nothing is kept): the rows the rule may hand to the next call are the only ones left alone -> their number
int poison_slot(Slot& sl, ry_stream_t s, int* left) {
    *left = 0;
    const int w = sl.next();
    RY_TRY(sl.act(w).poison(s));
    DevBuf<float>& b = sl.act(1 - w);
    const KeptCall& k = sl.k;
    if (!k.valid) return b.poison(s);
    for (long long f = 0; f * CREPE_BINS < b.cap; ++f) {
        if (f < k.nf && k.portable[(size_t)f]) { ++*left; continue; }
        const long long n = std::min((long long)CREPE_BINS, b.cap - f * CREPE_BINS);
        RT_TRY(rt::dmemset(b.ptr() + f * CREPE_BINS, 0xff, (size_t)n * sizeof(float), s));
    }
    return RY_OK;
}

// the activation of the window a slot keeps (k.valid), to the host or to a device pointer
int read_activation(ry_ctx* ctx, Slot& sl, float* out, int on_device) {
    const ry_stream_t s = ctx->stream;
    const size_t bytes = (size_t)sl.k.nf * CREPE_BINS * sizeof(float);
    if (on_device) { RT_TRY(rt::d2d(out, sl.act(sl.k.kept).ptr(), bytes, s)); return RY_OK; }
    RT_TRY(rt::d2h(out, sl.act(sl.k.kept).ptr(), bytes, s));
    RT_TRY(rt::stream_sync(s));
    return RY_OK;
}
}  // namespace

extern "C" {

size_t ry_crepe_param_count(int capacity) {
    if (capacity < 1 || capacity > MULT_MAX) {
        fail(RY_EINVAL, "crepe capacity multiplier %d out of range (1 .. %d; tiny 4, small 8, medium 16, large 24, full 32)", capacity, MULT_MAX);
        return 0;
    }
    return param_count(capacity);
}

int ry_crepe_set_viterbi_tables(ry_crepe* c, const double* logT, const double* logE, const double* logS) {
    if (!c || !logT || !logE || !logS) return fail(RY_EINVAL, "bad argument");
    RY_TRY(check_handle(c, "crepe"));
    RT_TRY(rt::stream_sync(c->ctx->stream));                   // the tables may be in use by a call still in flight
    RT_TRY(rt::h2d(c->logT, logT, sizeof(double) * CREPE_BINS * CREPE_BINS, c->ctx->stream));
    RT_TRY(rt::h2d(c->logE, logE, sizeof(double) * CREPE_BINS * CREPE_BINS, c->ctx->stream));
    RT_TRY(rt::h2d(c->logS, logS, sizeof(double) * CREPE_BINS, c->ctx->stream));
    RT_TRY(rt::stream_sync(c->ctx->stream));
    return RY_OK;
}

int ry_crepe_create(ry_ctx* ctx, int capacity, const float* weights, size_t n_floats, float bn_eps, ry_crepe** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    if (!ctx || !weights) return fail(RY_EINVAL, "bad argument");
    const size_t want = ry_crepe_param_count(capacity);
    if (want == 0) return RY_EINVAL;
    if (n_floats != want) return fail(RY_EINVAL, "crepe weight blob has %zu floats, capacity %d needs %zu", n_floats, capacity, want);
    if (!(bn_eps > 0.f)) return fail(RY_EINVAL, "bn_eps must be positive");
    RT_TRY(rt::set_device(ctx->device));
    std::unique_ptr<ry_crepe> c(new ry_crepe());
    c->ctx = ctx;
    c->m = capacity;
    const float* src = weights;
    int cin = 1, lin = CREPE_FRAME;
    for (int i = 0; i <= NCONV; ++i) {
        CLayer& l = c->L[i];
        if (i < NCONV) {
            l.cin = cin; l.cout = FILTERS[i] * capacity; l.width = WIDTHS[i]; l.stride = STRIDES[i];
            l.lin = lin; l.lout = lin / l.stride; l.K = l.width * l.cin;
            l.in_fstride = i == 0 ? CREPE_FRAME_ROW : (lin + PAD_L + PAD_R) * cin;
            l.in_rstride = l.stride * cin;
            const int pooled = l.lout / 2;
            l.out_fstride = i + 1 < NCONV ? (pooled + PAD_L + PAD_R) * l.cout : pooled * l.cout;
            l.out_off = i + 1 < NCONV ? PAD_L * l.cout : 0;
            // torch layout W (Cout, Cin, width) -> [n][tap][ci]; BN (gamma, beta, mean, var) -> scale / shift after the ReLU
            std::vector<float> w((size_t)l.cout * l.K), sc(l.cout), sh(l.cout), b(l.cout);
            for (int n = 0; n < l.cout; ++n)
                for (int ci = 0; ci < l.cin; ++ci)
                    for (int t = 0; t < l.width; ++t)
                        w[(size_t)n * l.K + (size_t)t * l.cin + ci] = src[((size_t)n * l.cin + ci) * l.width + t];
            src += (size_t)l.cout * l.K;
            const float* bias = src; const float* g = src + l.cout; const float* be = src + 2 * l.cout;
            const float* mu = src + 3 * l.cout; const float* var = src + 4 * l.cout;
            for (int n = 0; n < l.cout; ++n) {
                const double s = (double)g[n] / std::sqrt((double)var[n] + (double)bn_eps);
                sc[n] = (float)s; sh[n] = (float)((double)be[n] - (double)mu[n] * s); b[n] = bias[n];
            }
            src += 5 * (size_t)l.cout;
            RY_TRY(upload(c->weights, ctx, w, &l.w)); RY_TRY(upload(c->weights, ctx, b, &l.b));
            RY_TRY(upload(c->weights, ctx, sc, &l.sc)); RY_TRY(upload(c->weights, ctx, sh, &l.sh));
            cin = l.cout; lin = pooled;
        } else {                                                    // dense: classifier.weight (360, 4 C6) is already [n][k]
            l.cin = 4 * cin; l.cout = CREPE_BINS; l.width = 1; l.lin = 1; l.lout = 1; l.K = 4 * cin;
            l.in_fstride = 4 * cin; l.in_rstride = 0;
            std::vector<float> w(src, src + (size_t)CREPE_BINS * l.K), b(src + (size_t)CREPE_BINS * l.K, src + (size_t)CREPE_BINS * (l.K + 1));
            src += (size_t)CREPE_BINS * (l.K + 1);
            RY_TRY(upload(c->weights, ctx, w, &l.w)); RY_TRY(upload(c->weights, ctx, b, &l.b));
        }
        // split-K: enough workgroups at one second of audio; at least 16 chunks of K per split (the dense layer: 4 -- its 6 tiles
        // would otherwise leave most of the chip idle)
        const long long tiles = (long long)((PLAN_FRAMES * l.lout + CREPE_BM - 1) / CREPE_BM) * ((l.cout + CREPE_BN - 1) / CREPE_BN);
        const int nch = l.K / CREPE_BK;
        l.splits = (int)std::max(1LL, std::min((long long)(nch / (i == NCONV ? 4 : 16)), (PLAN_WORKGROUPS + tiles - 1) / tiles));
        // the split-bf16 kernel: the same plan in its chunks of 64 (the floor is 8 / 2 chunks, the same span of K)
        if (l.K % CREPE_X3_BK) return fail(RY_EINVAL, "crepe layer %d: K = %d is not a multiple of %d", i, l.K, CREPE_X3_BK);
        const int nch3 = l.K / CREPE_X3_BK;
        l.splits_x3 = (int)std::max(1LL, std::min((long long)(nch3 / (i == NCONV ? 2 : 8)), (PLAN_WORKGROUPS + tiles - 1) / tiles));
        l.w_off = i == 0 ? 0 : c->L[i - 1].w_off + (size_t)c->L[i - 1].cout * c->L[i - 1].K;
    }
    // the HMM of the decode: uniform start, T[i][j] ~ max(12 - |i - j|, 0) per row, E = 0.1 I + 0.9 / 360 (logs in float64;
    // the Python layer replaces them by numpy's own values, ry_crepe_set_viterbi_tables)
    std::vector<double> lt((size_t)CREPE_BINS * CREPE_BINS), le((size_t)CREPE_BINS * CREPE_BINS), ls(CREPE_BINS);
    for (int i = 0; i < CREPE_BINS; ++i) {
        double sum = 0;
        for (int j = 0; j < CREPE_BINS; ++j) sum += std::max(12 - std::abs(i - j), 0);
        for (int j = 0; j < CREPE_BINS; ++j) {
            lt[(size_t)i * CREPE_BINS + j] = std::log(std::max(12 - std::abs(i - j), 0) / sum);
            le[(size_t)i * CREPE_BINS + j] = std::log((i == j ? 0.1 : 0.0) + 0.9 / CREPE_BINS);
        }
        ls[i] = std::log(1.0 / CREPE_BINS);
    }
    RY_TRY(upload_table(c->weights, ctx, lt.data(), lt.size(), &c->logT));
    RY_TRY(upload_table(c->weights, ctx, le.data(), le.size(), &c->logE));
    RY_TRY(upload_table(c->weights, ctx, ls.data(), ls.size(), &c->logS));
    // the HMM of the voicing ([MEM]: start, transition, means, variances of `predict_voicing`; state 1 = voiced), logs from the C library
    // (the Python layer replaces them by numpy's own values, ry_crepe_set_voicing_tables)
    const double v_start[2] = {0.7472, 0.2528}, v_trans[2][2] = {{0.9991, 0.0009}, {0.0025, 0.9975}};
    const double v_mu[2] = {0.0795, 0.6278}, v_var[2] = {0.0181, 0.0454};
    for (int i = 0; i < 2; ++i) {
        c->vt.c[i] = std::log(2 * 3.141592653589793 * v_var[i]); c->vt.mu[i] = v_mu[i]; c->vt.var[i] = v_var[i];
        c->vt.logS[i] = std::log(v_start[i]);
        for (int j = 0; j < 2; ++j) c->vt.logT[i][j] = std::log(v_trans[i][j]);
    }
    *out = c.release();
    return RY_OK;
}

void ry_crepe_destroy(ry_crepe* c) {
    if (!c) return;
    rt::set_device(c->ctx->device);
    rt::stream_sync(c->ctx->stream);
    delete c;
}

int ry_crepe_set_dtype(ry_crepe* c, int dtype) {
    RY_TRY(check_handle(c, "crepe"));
    if (dtype != 0 && dtype != 2) return fail(RY_EINVAL, "crepe dtype %d (0 = fp32, 2 = split-bf16; there is no plain bf16 form of this network)", dtype);
    if (dtype == 2 && !c->planes_built) {
        const CLayer& last = c->L[NCONV];
        const long long total = (long long)(last.w_off + (size_t)last.cout * last.K);
        RY_TRY(c->w_hi.reserve(c->ctx, total));
        RY_TRY(c->w_lo.reserve(c->ctx, total));
        for (int i = 0; i <= NCONV; ++i) {
            const CLayer& l = c->L[i];
            CrepeSplitWParams sp;
            sp.w = l.w; sp.hi = c->w_hi.ptr() + l.w_off; sp.lo = c->w_lo.ptr() + l.w_off; sp.n8 = (long long)l.cout * l.K / 8;
            RY_LAUNCH(crepe_split_w, dim3((unsigned)((sp.n8 + 255) / 256)), 256, c->ctx->stream, sp);
            RT_TRY(rt::last_error());
        }
        c->planes_built = true;
    }
    c->dtype = dtype;                                               // the launches of later calls follow it; the stream keeps them in order
    return RY_OK;
}

int ry_crepe_predict(ry_crepe* c, const float* audio, int n_samples, int hop, int center, int viterbi,
                     float* f0, float* confidence, float* activation, int on_device) {
    RY_TRY(check_handle(c, "crepe"));
    if (!audio || !f0 || !confidence || n_samples < 1 || hop < 1) return fail(RY_EINVAL, "bad argument");
    forget_track(c);
    int nf = 0;
    RY_TRY(frame_count(n_samples, hop, center, &nf));
    ry_ctx* ctx = c->ctx;
    const ry_stream_t s = ctx->stream;
    RY_TRY(ensure_chunk(c, std::min(nf, CHUNK)));
    RY_TRY(ensure_call(c, nf, on_device ? 0 : n_samples));
    const float* d_audio = audio;
    if (!on_device) {
        RT_TRY(rt::h2d(c->audio.ptr(), audio, (size_t)n_samples * sizeof(float), s));
        d_audio = c->audio.ptr();
    }
    return run_network(c, d_audio, n_samples, hop, center, viterbi, nf, f0, confidence, activation, on_device);
}

int ry_crepe_set_resampler(ry_crepe* c, int sr, const double* win, int n_win, int num_table, int step, const double* time_register, int n_times) {
    RY_TRY(check_handle(c, "crepe"));
    if (sr < 1 || !time_register || n_times < 1) return fail(RY_EINVAL, "bad argument");
    const bool known = c->rs.count(sr) != 0;
    if (!win && !known) return fail(RY_EINVAL, "the first call for %d Hz needs the filter table", sr);
    if (win && (n_win < 2 || num_table < 1 || step < 1)) return fail(RY_EINVAL, "filter table: %d entries, %d per zero crossing, step %d", n_win, num_table, step);
    if (!(time_register[0] >= 0.0)) return fail(RY_EINVAL, "the time register starts at %g", time_register[0]);
    for (int i = 1; i < n_times; ++i)
        if (!(time_register[i] >= time_register[i - 1]) || !(time_register[i] < 2147483648.0))
            return fail(RY_EINVAL, "the time register is not a non-decreasing sequence of sample times at entry %d", i);
    RT_TRY(rt::stream_sync(c->ctx->stream));                   // the tables may be in use by a call still in flight
    Resampler r = known ? c->rs[sr] : Resampler();
    if (win) {
        double* d = nullptr;
        RY_TRY(upload_table(c->rs_tables, c->ctx, win, (size_t)n_win, &d));
        if (r.win) c->rs_tables.free_one(r.win);
        r.win = d; r.n_win = n_win; r.num_table = num_table; r.step = step;
        ++c->rs_epoch;
    }
    double* d = nullptr;
    RY_TRY(upload_table(c->rs_tables, c->ctx, time_register, (size_t)n_times, &d));
    if (r.tr) c->rs_tables.free_one(r.tr);
    r.tr = d; r.n_times = n_times;
    r.tr_host.assign(time_register, time_register + n_times);
    c->rs[sr] = std::move(r);
    return RY_OK;
}

int ry_crepe_resample(ry_crepe* c, const float* audio, int n_samples, int sr, float* out16k, int on_device) {
    RY_TRY(check_handle(c, "crepe"));
    if (!audio || !out16k) return fail(RY_EINVAL, "bad argument");
    forget_track(c);
    const Resampler* r = nullptr;
    int n_out = 0;
    RY_TRY(resample_plan(c, n_samples, sr, &r, &n_out));
    const ry_stream_t s = c->ctx->stream;
    if (on_device) return launch_resample(c, *r, audio, n_samples, sr, out16k, n_out);
    RY_TRY(c->audio.reserve(c->ctx, n_out));
    float* wave = nullptr;
    RY_TRY(upload_audio(c, r, audio, n_samples, &wave));
    RY_TRY(launch_resample(c, *r, wave, n_samples, sr, c->audio.ptr(), n_out));
    RT_TRY(rt::d2h(out16k, c->audio.ptr(), (size_t)n_out * sizeof(float), s));
    RT_TRY(rt::stream_sync(s));
    return RY_OK;
}

int ry_crepe_predict_sr(ry_crepe* c, const float* audio, int n_samples, int sr, int hop, int center, int viterbi,
                        float* f0, float* confidence, float* activation, int on_device) {
    if (sr == 16000) return ry_crepe_predict(c, audio, n_samples, hop, center, viterbi, f0, confidence, activation, on_device);
    RY_TRY(check_handle(c, "crepe"));
    if (!audio || !f0 || !confidence || hop < 1) return fail(RY_EINVAL, "bad argument");
    forget_track(c);
    const Resampler* r = nullptr;
    int n_out = 0, nf = 0;
    RY_TRY(resample_plan(c, n_samples, sr, &r, &n_out));
    RY_TRY(frame_count(n_out, hop, center, &nf));
    RY_TRY(ensure_chunk(c, std::min(nf, CHUNK)));
    RY_TRY(ensure_call(c, nf, n_out));
    float* wave = nullptr;
    if (!on_device) RY_TRY(upload_audio(c, r, audio, n_samples, &wave));
    RY_TRY(launch_resample(c, *r, on_device ? audio : wave, n_samples, sr, c->audio.ptr(), n_out));
    return run_network(c, c->audio.ptr(), n_out, hop, center, viterbi, nf, f0, confidence, activation, on_device);
}

int ry_crepe_decode(ry_crepe* c, const float* activation, int n_frames, int viterbi, float* f0, float* confidence, int* path) {
    RY_TRY(check_handle(c, "crepe"));
    if (!activation || !f0 || !confidence || n_frames < 1 || n_frames > (1 << 24)) return fail(RY_EINVAL, "bad argument");
    forget_track(c);
    const ry_stream_t s = c->ctx->stream;
    RY_TRY(ensure_call(c, n_frames, 0));
    RT_TRY(rt::h2d(c->act.ptr(), activation, (size_t)n_frames * CREPE_BINS * sizeof(float), s));
    RY_TRY(launch_decode(c, c->act.ptr(), n_frames, viterbi));
    RT_TRY(rt::d2h(f0, c->f0.ptr(), (size_t)n_frames * sizeof(float), s));
    RT_TRY(rt::d2h(confidence, c->conf.ptr(), (size_t)n_frames * sizeof(float), s));
    if (path) RT_TRY(rt::d2h(path, viterbi ? c->path.ptr() : c->obs.ptr(), (size_t)n_frames * sizeof(int), s));
    RT_TRY(rt::stream_sync(s));
    return RY_OK;
}

int ry_crepe_set_voicing_tables(ry_crepe* c, const double* cst, const double* mu, const double* var, const double* logT, const double* logS) {
    if (!c || !cst || !mu || !var || !logT || !logS) return fail(RY_EINVAL, "bad argument");
    for (int i = 0; i < 2; ++i) {
        if (!std::isfinite(cst[i]) || !std::isfinite(mu[i]) || !(var[i] > 0.0) || !std::isfinite(var[i]) || std::isnan(logS[i]) || std::isnan(logT[2 * i]) ||
            std::isnan(logT[2 * i + 1]))
            return fail(RY_EINVAL, "voicing tables: state %d", i);
    }
    for (int i = 0; i < 2; ++i) {                                     // kernel arguments of the calls that follow: nothing in flight reads them
        c->vt.c[i] = cst[i]; c->vt.mu[i] = mu[i]; c->vt.var[i] = var[i]; c->vt.logS[i] = logS[i];
        c->vt.logT[i][0] = logT[2 * i]; c->vt.logT[i][1] = logT[2 * i + 1];
    }
    return RY_OK;
}

int ry_crepe_voicing(ry_crepe* c, const float* confidence, const float* f0, int n, double threshold, double step_ms,
                     unsigned char* voiced, double* f0_64, double* t_64, int on_device) {
    RY_TRY(check_handle(c, "crepe"));
    if (!confidence || !f0 || !voiced || !f0_64 || !t_64 || n < 1 || n > (1 << 24)) return fail(RY_EINVAL, "bad argument");
    RY_TRY(voicing_args(threshold, step_ms));
    forget_track(c);
    if (on_device) return launch_voicing(c, confidence, f0, n, threshold, step_ms, voiced, f0_64, t_64);
    const ry_stream_t s = c->ctx->stream;
    RY_TRY(c->conf.reserve(c->ctx, n));
    RY_TRY(c->f0.reserve(c->ctx, n));
    RY_TRY(ensure_track(c, n));
    RT_TRY(rt::h2d(c->conf.ptr(), confidence, (size_t)n * sizeof(float), s));
    RT_TRY(rt::h2d(c->f0.ptr(), f0, (size_t)n * sizeof(float), s));
    RY_TRY(launch_voicing(c, c->conf.ptr(), c->f0.ptr(), n, threshold, step_ms, c->voiced.ptr(), c->f0_64.ptr(), c->t_64.ptr()));
    return download_track(c, n, voiced, f0_64, t_64);
}

int ry_crepe_track(ry_crepe* c, const float* audio, int n_samples, int sr, int hop, double step_ms, double threshold, int* n_frames,
                   unsigned char* voiced, double* f0_64, double* t_64, int on_device_out) {
    RY_TRY(check_handle(c, "crepe"));
    if (!audio || !n_frames || n_samples < 1 || hop < 1) return fail(RY_EINVAL, "bad argument");
    if (!on_device_out && (!voiced || !f0_64 || !t_64)) return fail(RY_EINVAL, "null output");
    RY_TRY(voicing_args(threshold, step_ms));
    forget_track(c);                                                 // after the argument refusals: such a call keeps the previous track
    TrackCall z;
    RY_TRY(size_call(c, n_samples, sr, hop, &z));
    RY_TRY(reserve_call(c, z, z.total_nf));
    RY_TRY(bring_up(c, &z, audio));
    RY_TRY(run_network(c, c->audio.ptr(), z.total16, hop, 1, 1, z.total_nf, nullptr, nullptr, nullptr, 1));
    return finish_track(c, z, threshold, step_ms, n_frames, voiced, f0_64, t_64, on_device_out);
}

int ry_crepe_track_buffers(ry_crepe* c, const float** wave_dev, int* n_samples, int* n_frames, const unsigned char** voiced_dev,
                           const double** f0_dev, const double** t_dev) {
    if (!c) return fail(RY_ESTATE, "null crepe handle");
    if (c->trk_frames < 1) return fail(RY_ESTATE, "no track on the card: ry_crepe_track has not run, or a later call reused its buffers");
    if (wave_dev) *wave_dev = c->trk_wave;
    if (n_samples) *n_samples = c->trk_samples;
    if (n_frames) *n_frames = c->trk_frames;
    if (voiced_dev) *voiced_dev = c->voiced.ptr();
    if (f0_dev) *f0_dev = c->f0_64.ptr();
    if (t_dev) *t_dev = c->t_64.ptr();
    return RY_OK;
}

// ry_crepe_track_many (audio: the waves of the call, uploaded by it) and ry_crepe_track_uploaded (audio null: first_sample names waves of the table
// ry_crepe_upload_waves left): one body, so the segment table, the passes and the decode / voicing workgroup per wave are the same
static int track_many_impl(ry_crepe* c, const float* audio, const int* first_sample, const int* n_samples, int n_waves, int sr, int hop, double step_ms,
                           double threshold, int* n_frames, unsigned char* voiced, double* f0_64, double* t_64, int on_device_out) {
    RY_TRY(check_handle(c, "crepe"));
    const bool uploaded = audio == nullptr && first_sample != nullptr;
    forget_track(c, uploaded);                                       // a refused call leaves no track either
    if ((!audio && !first_sample) || !n_samples || !n_frames || hop < 1) return fail(RY_EINVAL, "bad argument");
    if (!on_device_out && (!voiced || !f0_64 || !t_64)) return fail(RY_EINVAL, "null output");
    if (n_waves < 1) return fail(RY_EINVAL, "%d waves", n_waves);
    RY_TRY(voicing_args(threshold, step_ms));
    TrackCall z;
    RY_TRY(size_call(c, uploaded ? first_sample : nullptr, n_samples, n_waves, sr, hop, &z, any_wave));
    RY_TRY(reserve_call(c, z, z.total_nf));
    RY_TRY(bring_up(c, &z, audio));
    RY_TRY(run_network(c, c->audio.ptr(), z.total16, hop, 1, 1, z.total_nf, nullptr, nullptr, nullptr, 1, z.seg, n_waves));
    return finish_track(c, z, threshold, step_ms, n_frames, voiced, f0_64, t_64, on_device_out);
}

int ry_crepe_track_many(ry_crepe* c, const float* audio, const int* n_samples, int n_waves, int sr, int hop, double step_ms, double threshold,
                        int* n_frames, unsigned char* voiced, double* f0_64, double* t_64, int on_device_out) {
    return track_many_impl(c, audio, nullptr, n_samples, n_waves, sr, hop, step_ms, threshold, n_frames, voiced, f0_64, t_64, on_device_out);
}

int ry_crepe_upload_waves(ry_crepe* c, const float* audio, const int* n_samples, int n_waves, int sr, const float** wave_dev) {
    RY_TRY(check_handle(c, "crepe"));
    forget_track(c);                                                 // a refused call leaves no table either
    if (!audio || !n_samples || !wave_dev) return fail(RY_EINVAL, "bad argument");
    if (n_waves < 1) return fail(RY_EINVAL, "%d waves", n_waves);
    const Resampler* r = nullptr;
    std::vector<long long> off((size_t)n_waves + 1, 0);
    for (int i = 0; i < n_waves; ++i) {
        if (n_samples[i] < 1) return fail(RY_EINVAL, "wave %d has %d samples", i, n_samples[i]);
        int n16 = 0;
        if (sr != 16000) RY_TRY(resample_plan(c, n_samples[i], sr, &r, &n16));
        off[(size_t)i + 1] = off[(size_t)i] + n_samples[i];
        if (off[(size_t)i + 1] > 2147483647LL) return fail(RY_EINVAL, "the waves up to %d hold %lld samples: too many for one call", i, off[(size_t)i + 1]);
    }
    float* wave = nullptr;
    RY_TRY(upload_audio(c, r, audio, (int)off.back(), &wave));
    c->up_wave = wave; c->up_off.swap(off); c->up_sr = sr;
    *wave_dev = wave;
    return RY_OK;
}

int ry_crepe_track_uploaded(ry_crepe* c, const int* first_sample, const int* n_samples, int n_waves, int sr, int hop, double step_ms, double threshold,
                            int* n_frames, unsigned char* voiced, double* f0_64, double* t_64, int on_device_out) {
    return track_many_impl(c, nullptr, first_sample, n_samples, n_waves, sr, hop, step_ms, threshold, n_frames, voiced, f0_64, t_64, on_device_out);
}

int ry_crepe_uploaded_buffers(ry_crepe* c, const float** wave_dev, long long* n_samples, int* n_tracked, const int** frame_offsets,
                              const unsigned char** voiced_dev, const double** f0_dev, const double** t_dev) {
    if (!c) return fail(RY_ESTATE, "null crepe handle");
    if (c->up_off.empty()) return fail(RY_ESTATE, "no waves on the card: ry_crepe_upload_waves has not run, or a later call reused its buffers");
    if (wave_dev) *wave_dev = c->up_wave;
    if (n_samples) *n_samples = c->up_off.back();
    if (n_tracked) *n_tracked = c->sub_waves;
    if (frame_offsets) *frame_offsets = c->sub_waves > 0 ? c->sub_frame_off.data() : nullptr;
    if (voiced_dev) *voiced_dev = c->voiced.ptr();
    if (f0_dev) *f0_dev = c->f0_64.ptr();
    if (t_dev) *t_dev = c->t_64.ptr();
    return RY_OK;
}

int ry_crepe_debug_frames(ry_crepe* c, long long* n_frames) {
    if (!c || !n_frames) return fail(RY_EINVAL, "bad argument");
    *n_frames = c->net_frames;
    return RY_OK;
}

int ry_crepe_track_many_buffers(ry_crepe* c, const float** wave_dev, int* n_waves, const long long** sample_offsets, const int** frame_offsets,
                                const unsigned char** voiced_dev, const double** f0_dev, const double** t_dev) {
    if (!c) return fail(RY_ESTATE, "null crepe handle");
    if (c->trk_waves < 1) return fail(RY_ESTATE, "no tracks on the card: ry_crepe_track_many has not run, or a later call reused its buffers");
    if (wave_dev) *wave_dev = c->trk_wave;
    if (n_waves) *n_waves = c->trk_waves;
    if (sample_offsets) *sample_offsets = c->trk_sample_off.data();
    if (frame_offsets) *frame_offsets = c->trk_frame_off.data();
    if (voiced_dev) *voiced_dev = c->voiced.ptr();
    if (f0_dev) *f0_dev = c->f0_64.ptr();
    if (t_dev) *t_dev = c->t_64.ptr();
    return RY_OK;
}

int ry_crepe_decode_many(ry_crepe* c, const float* activation, const int* n_frames, int n_tracks, int viterbi, float* f0, float* confidence, int* path) {
    RY_TRY(check_handle(c, "crepe"));
    if (!activation || !n_frames || !f0 || !confidence) return fail(RY_EINVAL, "bad argument");
    forget_track(c);
    std::vector<CrepeSeg> plan;
    RY_TRY(plan_segments(n_tracks, nullptr, nullptr, n_frames, &plan));
    const int total = plan.back().frame0 + plan.back().n_frames;
    const ry_stream_t s = c->ctx->stream;
    RY_TRY(ensure_call(c, total, 0));
    RY_TRY(upload_segments(c, plan));
    RT_TRY(rt::h2d(c->act.ptr(), activation, (size_t)total * CREPE_BINS * sizeof(float), s));
    RY_TRY(launch_decode(c, c->act.ptr(), total, viterbi, c->segs.ptr(), n_tracks));
    RT_TRY(rt::d2h(f0, c->f0.ptr(), (size_t)total * sizeof(float), s));
    RT_TRY(rt::d2h(confidence, c->conf.ptr(), (size_t)total * sizeof(float), s));
    if (path) RT_TRY(rt::d2h(path, viterbi ? c->path.ptr() : c->obs.ptr(), (size_t)total * sizeof(int), s));
    RT_TRY(rt::stream_sync(s));
    return RY_OK;
}

int ry_crepe_voicing_many(ry_crepe* c, const float* confidence, const float* f0, const int* n_frames, int n_tracks, double threshold, double step_ms,
                          unsigned char* voiced, double* f0_64, double* t_64, int on_device) {
    RY_TRY(check_handle(c, "crepe"));
    if (!confidence || !f0 || !n_frames || !voiced || !f0_64 || !t_64) return fail(RY_EINVAL, "bad argument");
    RY_TRY(voicing_args(threshold, step_ms));
    forget_track(c);
    std::vector<CrepeSeg> plan;
    RY_TRY(plan_segments(n_tracks, nullptr, nullptr, n_frames, &plan));
    const int n = plan.back().frame0 + plan.back().n_frames;
    const ry_stream_t s = c->ctx->stream;
    if (on_device) {
        RY_TRY(upload_segments(c, plan));
        return launch_voicing(c, confidence, f0, n, threshold, step_ms, voiced, f0_64, t_64, c->segs.ptr(), n_tracks);
    }
    RY_TRY(c->conf.reserve(c->ctx, n));
    RY_TRY(c->f0.reserve(c->ctx, n));
    RY_TRY(ensure_track(c, n));
    RY_TRY(upload_segments(c, plan));
    RT_TRY(rt::h2d(c->conf.ptr(), confidence, (size_t)n * sizeof(float), s));
    RT_TRY(rt::h2d(c->f0.ptr(), f0, (size_t)n * sizeof(float), s));
    RY_TRY(launch_voicing(c, c->conf.ptr(), c->f0.ptr(), n, threshold, step_ms, c->voiced.ptr(), c->f0_64.ptr(), c->t_64.ptr(), c->segs.ptr(), n_tracks));
    return download_track(c, n, voiced, f0_64, t_64);
}

int ry_crepe_debug_layer(ry_crepe* c, int layer, int n_frames, float* out) {
    RY_TRY(check_handle(c, "crepe"));
    if (!out || layer < 0 || layer > NCONV + 1) return fail(RY_EINVAL, "bad argument (layer %d: 0 frames, 1 .. 6 conv outputs, 7 logits)", layer);
    if (c->last_chunk < 1) return fail(RY_ESTATE, "no ry_crepe_predict has run");
    if (n_frames < 1 || n_frames > c->cap_chunk) return fail(RY_EINVAL, "%d frames asked for, the pass buffers hold %d", n_frames, c->cap_chunk);
    const ry_stream_t s = c->ctx->stream;
    const int n = n_frames;
    if (layer == NCONV + 1) {
        RT_TRY(rt::d2h(out, c->logits, (size_t)n * CREPE_BINS * sizeof(float), s));
        RT_TRY(rt::stream_sync(s));
        return RY_OK;
    }
    // the interior rows of the padded buffer
    const CLayer& dst = c->L[layer];                                // the layer that reads this buffer (dense for layer 6)
    int rows, cols, off;
    if (layer == 0) { rows = CREPE_FRAME; cols = 1; off = CREPE_CONV1_PAD; }
    else if (layer == NCONV) { rows = 4; cols = c->L[NCONV - 1].cout; off = 0; }
    else { rows = dst.lin; cols = dst.cin; off = PAD_L * dst.cin; }
    std::vector<float> h((size_t)n * dst.in_fstride);
    RT_TRY(rt::d2h(h.data(), c->act_in[layer], h.size() * sizeof(float), s));
    RT_TRY(rt::stream_sync(s));
    for (int f = 0; f < n; ++f)
        memcpy(out + (size_t)f * rows * cols, h.data() + (size_t)f * dst.in_fstride + off, (size_t)rows * cols * sizeof(float));
    return RY_OK;
}

int ry_crepe_debug_poison(ry_crepe* c) {
    RY_TRY(check_handle(c, "crepe"));
    const ry_stream_t s = c->ctx->stream;
    RT_TRY(rt::stream_sync(s));
    // all bits set (NaN as a float, -1 as an index) in everything the next call must write; the padding rows keep their zeros
    for (int i = 0; i <= NCONV && c->cap_chunk > 0; ++i) {
        const CLayer& l = c->L[i];
        const size_t off = i == 0 ? CREPE_CONV1_PAD : i == NCONV ? 0 : (size_t)PAD_L * l.cin;
        const size_t n = i == 0 ? CREPE_FRAME : i == NCONV ? (size_t)l.in_fstride : (size_t)l.lin * l.cin;
        for (int f = 0; f < c->cap_chunk; ++f)
            RT_TRY(rt::dmemset(c->act_in[i] + (size_t)f * l.in_fstride + off, 0xff, n * sizeof(float), s));
    }
    if (c->cap_chunk > 0) {
        RT_TRY(rt::dmemset(c->logits, 0xff, (size_t)c->cap_chunk * CREPE_BINS * sizeof(float), s));
        RT_TRY(rt::dmemset(c->slabs, 0xff, c->slab_floats * sizeof(float), s));
    }
    for (DevBufBase* b : c->call) RY_TRY(b->poison(s));               // the voicing's back-pointers and the masked track are on this list too
    forget_track(c);
    RT_TRY(rt::stream_sync(s));
    return RY_OK;
}

int ry_crepe_debug_splits(ry_crepe* c, int* splits) {
    if (!c || !splits) return fail(RY_EINVAL, "bad argument");
    for (int i = 0; i <= NCONV; ++i) splits[i] = c->splits_of(i);
    return RY_OK;
}

int ry_crepe_stream_create(ry_crepe* c, ry_crepe_stream** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    RY_TRY(check_handle(c, "crepe"));
    ry_crepe_stream* s = new ry_crepe_stream();
    s->ctx = c->ctx;
    s->model = c;
    *out = s;
    return RY_OK;
}

void ry_crepe_stream_destroy(ry_crepe_stream* s) {
    if (!s) return;
    rt::set_device(s->ctx->device);
    rt::stream_sync(s->ctx->stream);
    delete s;
}

int ry_crepe_stream_reset(ry_crepe_stream* s) {
    if (!s) return fail(RY_ESTATE, "null crepe stream handle");
    s->rows.k.valid = false;
    return RY_OK;
}

int ry_crepe_stream_track(ry_crepe_stream* st, const float* audio, int n_samples, int sr, int hop, double step_ms, double threshold, int advance,
                          int overlap_ok, int* n_frames, int* n_computed, unsigned char* voiced, double* f0_64, double* t_64, int on_device_out) {
    RY_TRY(check_handle(st, "crepe stream"));
    ry_crepe* c = st->model;
    // the refusals of ry_crepe_track, before anything is launched or written: the kept rows stay as they were
    if (!audio || !n_frames || !n_computed || n_samples < 1 || hop < 1) return fail(RY_EINVAL, "bad argument");
    if (!on_device_out && (!voiced || !f0_64 || !t_64)) return fail(RY_EINVAL, "null output");
    RY_TRY(voicing_args(threshold, step_ms));
    forget_track(c);
    const ry_stream_t s = c->ctx->stream;
    Slot& rows = st->rows;
    TrackCall z;
    RY_TRY(size_call(c, n_samples, sr, hop, &z));
    const int nf = z.total_nf;
    std::vector<int>& tab = st->tab_host[st->tab_cur == 0 ? 1 : 0];
    const int n_comp = plan_stream(c, &st->cache, &rows.k, z.r, n_samples, sr, hop, nf, advance, overlap_ok, &tab);
    const bool all = n_comp == nf;                                    // nothing kept: the dense layer writes the window's block itself
    const int w = rows.next();
    const float* keep = rows.keep();
    const int n_keep = rows.n_keep();
    RY_TRY(reserve_call(c, z, n_comp));
    RY_TRY(rows.act(w).grow(c->ctx, (long long)nf * CREPE_BINS));
    if (!all) {
        RY_TRY(st->fresh.grow(c->ctx, (long long)n_comp * CREPE_BINS));
        RY_TRY(st->tab.grow(c->ctx, (long long)tab.size()));
        if (st->tab_cur < 0 || st->tab_host[st->tab_cur] != tab) {    // one copy for both tables, and only when they changed
            RT_TRY(rt::h2d(st->tab.ptr(), tab.data(), tab.size() * sizeof(int), s));
            st->tab_cur = st->tab_cur == 0 ? 1 : 0;
        }
    }
    rows.k.valid = false;                                             // from here on the block about to be written is in play
    RY_TRY(bring_up(c, &z, audio));
    float* act = rows.act(w).ptr();
    if (all) {
        RY_TRY(run_passes(c, c->audio.ptr(), z.total16, hop, 1, nf, nullptr, act));
    } else {
        RY_TRY(run_passes(c, c->audio.ptr(), z.total16, hop, 1, n_comp, st->tab.ptr() + nf, st->fresh.ptr()));
        RY_TRY(launch_assemble(c->ctx, keep, n_keep, st->fresh.ptr(), n_comp, st->tab.ptr(), act, nf));
    }
    RY_TRY(launch_decode(c, act, nf, 1));
    RY_TRY(finish_track(c, z, threshold, step_ms, n_frames, voiced, f0_64, t_64, on_device_out));
    keep_call(c, &st->cache, &rows.k, w, z.r, n_samples, z.total16, sr, hop, nf);
    *n_computed = n_comp;
    return RY_OK;
}

int ry_crepe_stream_activation(ry_crepe_stream* st, float* out, int on_device) {
    RY_TRY(check_handle(st, "crepe stream"));
    if (!out) return fail(RY_EINVAL, "bad argument");
    if (!st->rows.k.valid) return fail(RY_ESTATE, "the stream holds no window: ry_crepe_stream_track has not run, or ry_crepe_stream_reset came after it");
    return read_activation(st->ctx, st->rows, out, on_device);
}

int ry_crepe_stream_debug_poison(ry_crepe_stream* st, int* rows_left) {
    RY_TRY(check_handle(st, "crepe stream"));
    if (!rows_left) return fail(RY_EINVAL, "bad argument");
    const ry_stream_t s = st->ctx->stream;
    RT_TRY(rt::stream_sync(s));
    // all bits set in the packed block, the tables on the card and whatever of the slot the rule may not hand to the next call
    RY_TRY(st->fresh.poison(s));
    RY_TRY(st->tab.poison(s));
    st->tab_cur = -1;
    int left = 0;
    RY_TRY(poison_slot(st->rows, s, &left));
    RT_TRY(rt::stream_sync(s));
    *rows_left = left;
    return RY_OK;
}

int ry_crepe_stream_debug_assemble(ry_crepe_stream* st, const float* keep_dev, int n_keep, const float* fresh_dev, int n_fresh, const int* src,
                                   int n_rows, float* out_dev) {
    RY_TRY(check_handle(st, "crepe stream"));
    if (!keep_dev || !fresh_dev || !src || !out_dev || n_keep < 0 || n_fresh < 0 || n_rows < 1 || n_rows > (1 << 24)) return fail(RY_EINVAL, "bad argument");
    const ry_stream_t s = st->ctx->stream;
    RY_TRY(st->tab.grow(st->ctx, n_rows));
    st->tab_cur = -1;                                                 // the card's tables are no longer those of a call
    RT_TRY(rt::h2d(st->tab.ptr(), src, (size_t)n_rows * sizeof(int), s));
    RY_TRY(launch_assemble(st->ctx, keep_dev, n_keep, fresh_dev, n_fresh, st->tab.ptr(), out_dev, n_rows));
    RT_TRY(rt::stream_sync(s));
    return RY_OK;
}

// ---- a bank of streams ----
int ry_crepe_bank_create(ry_crepe* c, int n_streams, ry_crepe_bank** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    RY_TRY(check_handle(c, "crepe"));
    if (n_streams < 1 || n_streams > (1 << 16)) return fail(RY_EINVAL, "a bank of %d streams", n_streams);
    std::unique_ptr<ry_crepe_bank> b(new ry_crepe_bank());
    b->ctx = c->ctx;
    b->model = c;
    for (int i = 0; i < n_streams; ++i) b->slots.emplace_back(new Slot(b->bufs));
    *out = b.release();
    return RY_OK;
}

void ry_crepe_bank_destroy(ry_crepe_bank* b) {
    if (!b) return;
    rt::set_device(b->ctx->device);
    rt::stream_sync(b->ctx->stream);
    delete b;
}

int ry_crepe_bank_reset(ry_crepe_bank* b, int stream) {
    if (!b) return fail(RY_ESTATE, "null crepe bank handle");
    const int n = (int)b->slots.size();
    if (stream < -1 || stream >= n) return fail(RY_EINVAL, "stream %d of %d", stream, n);
    for (int i = 0; i < n; ++i)
        if (stream < 0 || stream == i) b->slots[(size_t)i]->k.valid = false;
    return RY_OK;
}

// ry_crepe_bank_track (audio: the waves of the call, uploaded by it) and ry_crepe_bank_track_uploaded (audio null: first_sample names waves of the
// table ry_crepe_upload_waves left on the model): one body
static int bank_track_impl(ry_crepe_bank* b, const float* audio, const int* first_sample, const int* n_samples, const int* stream_of, int n_waves, int sr,
                           int hop, double step_ms, double threshold, const int* advance, const int* overlap_ok, int* n_frames, int* n_computed,
                           unsigned char* voiced, double* f0_64, double* t_64, int on_device_out) {
    RY_TRY(check_handle(b, "crepe bank"));
    ry_crepe* c = b->model;
    const bool uploaded = audio == nullptr && first_sample != nullptr;
    forget_track(c, uploaded);                                       // a refused call leaves no track either
    // every refusal first, before anything is launched or written: those of ry_crepe_track_many, then the bank's own
    if ((!audio && !first_sample) || !n_samples || !stream_of || !advance || !overlap_ok || !n_frames || !n_computed || hop < 1) return fail(RY_EINVAL, "bad argument");
    if (!on_device_out && (!voiced || !f0_64 || !t_64)) return fail(RY_EINVAL, "null output");
    if (n_waves < 1) return fail(RY_EINVAL, "%d waves", n_waves);
    RY_TRY(voicing_args(threshold, step_ms));
    const int n_streams = (int)b->slots.size();
    std::vector<char> named((size_t)n_streams, 0);
    TrackCall z;
    RY_TRY(size_call(c, uploaded ? first_sample : nullptr, n_samples, n_waves, sr, hop, &z, [&](int i) {
        const int st = stream_of[i];
        if (st < 0 || st >= n_streams) return fail(RY_EINVAL, "wave %d names stream %d of %d", i, st, n_streams);
        if (named[(size_t)st]) return fail(RY_EINVAL, "stream %d is named twice in one call", st);
        named[(size_t)st] = 1;
        return (int)RY_OK;
    }));
    const int total_nf = z.total_nf;
    // the tables, host work only: per wave the rule against that stream's kept call, the packed rows numbered through the call, the frames call-global
    static_assert(sizeof(CrepeBankWave) == 6 * sizeof(int), "the descriptors are copied as six ints each");
    const size_t desc_ints = 6 * (size_t)n_waves;
    std::vector<int> tab(desc_ints + (size_t)total_nf), idx, one;
    std::vector<int> comp((size_t)n_waves);
    for (int i = 0; i < n_waves; ++i) {
        const CrepeSeg& g = z.plan[(size_t)i];
        const KeptCall& k = b->slots[(size_t)stream_of[i]]->k;
        const int n_comp = plan_stream(c, &b->cache, &k, z.r, n_samples[i], sr, hop, g.n_frames, advance[i], overlap_ok[i], &one);
        const int base = (int)idx.size();
        for (int j = 0; j < g.n_frames; ++j) tab[desc_ints + (size_t)(g.frame0 + j)] = one[(size_t)j] >= 0 ? one[(size_t)j] : one[(size_t)j] - base;
        for (int q = 0; q < n_comp; ++q) idx.push_back(g.frame0 + one[(size_t)g.n_frames + (size_t)q]);
        comp[(size_t)i] = n_comp;
    }
    const int total_comp = (int)idx.size();
    tab.insert(tab.end(), idx.begin(), idx.end());
    const ry_stream_t s = c->ctx->stream;
    RY_TRY(reserve_call(c, z, total_comp));
    RY_TRY(b->fresh.grow(c->ctx, (long long)total_comp * CREPE_BINS));
    for (int i = 0; i < n_waves; ++i) {                                 // the block each wave writes, and the descriptor that says so
        Slot& sl = *b->slots[(size_t)stream_of[i]];
        const int w = sl.next();
        RY_TRY(sl.act(w).grow(c->ctx, (long long)z.nf[(size_t)i] * CREPE_BINS));
        CrepeBankWave d;
        d.keep = sl.keep(); d.n_keep = sl.n_keep(); d.write = sl.act(w).ptr(); d.pad = 0;
        memcpy(&tab[6 * (size_t)i], &d, sizeof d);
    }
    // one copy for the descriptors and both tables, and only when neither of the two sets the card holds is this one
    int t = -1;
    for (int i = 0; i < 2; ++i)
        if (b->tab_on_card[i] && b->tab_host[i] == tab) t = i;
    if (t < 0) {
        t = 1 - b->tab_last;
        b->tab_on_card[t] = false;
        RY_TRY(b->tab(t).grow(c->ctx, (long long)tab.size()));
        b->tab_host[t].swap(tab);
        RT_TRY(rt::h2d(b->tab(t).ptr(), b->tab_host[t].data(), b->tab_host[t].size() * sizeof(int), s));
        b->tab_on_card[t] = true;
        ++b->uploads;
    }
    b->tab_last = t;
    const CrepeBankWave* d_wave = (const CrepeBankWave*)b->tab(t).ptr();
    const int* d_src = b->tab(t).ptr() + desc_ints;
    const int* d_idx = d_src + total_nf;
    std::vector<int> wrote((size_t)n_waves);
    for (int i = 0; i < n_waves; ++i) {                                 // from here on the blocks about to be written are in play
        Slot& sl = *b->slots[(size_t)stream_of[i]];
        wrote[(size_t)i] = sl.next();
        sl.k.valid = false;
    }
    RY_TRY(bring_up(c, &z, audio));
    RY_TRY(run_passes(c, c->audio.ptr(), z.total16, hop, 1, total_comp, d_idx, b->fresh.ptr(), z.seg, n_waves));
    RY_TRY(launch_assemble_many(c->ctx, z.seg, n_waves, d_wave, d_src, b->fresh.ptr(), total_comp, c->act.ptr(), total_nf));
    RY_TRY(launch_decode(c, c->act.ptr(), total_nf, 1, z.seg, n_waves));
    RY_TRY(finish_track(c, z, threshold, step_ms, n_frames, voiced, f0_64, t_64, on_device_out));
    for (int i = 0; i < n_waves; ++i) {
        keep_call(c, &b->cache, &b->slots[(size_t)stream_of[i]]->k, wrote[(size_t)i], z.r, n_samples[i], z.n16[(size_t)i], sr, hop, z.nf[(size_t)i]);
        n_computed[i] = comp[(size_t)i];
    }
    return RY_OK;
}

int ry_crepe_bank_track(ry_crepe_bank* b, const float* audio, const int* n_samples, const int* stream_of, int n_waves, int sr, int hop, double step_ms,
                        double threshold, const int* advance, const int* overlap_ok, int* n_frames, int* n_computed, unsigned char* voiced,
                        double* f0_64, double* t_64, int on_device_out) {
    return bank_track_impl(b, audio, nullptr, n_samples, stream_of, n_waves, sr, hop, step_ms, threshold, advance, overlap_ok, n_frames, n_computed, voiced,
                           f0_64, t_64, on_device_out);
}

int ry_crepe_bank_track_uploaded(ry_crepe_bank* b, const int* first_sample, const int* n_samples, const int* stream_of, int n_waves, int sr, int hop,
                                 double step_ms, double threshold, const int* advance, const int* overlap_ok, int* n_frames, int* n_computed,
                                 unsigned char* voiced, double* f0_64, double* t_64, int on_device_out) {
    return bank_track_impl(b, nullptr, first_sample, n_samples, stream_of, n_waves, sr, hop, step_ms, threshold, advance, overlap_ok, n_frames, n_computed,
                           voiced, f0_64, t_64, on_device_out);
}

int ry_crepe_bank_activation(ry_crepe_bank* b, int stream, float* out, int on_device) {
    RY_TRY(check_handle(b, "crepe bank"));
    if (!out || stream < 0 || stream >= (int)b->slots.size()) return fail(RY_EINVAL, "bad argument");
    Slot& sl = *b->slots[(size_t)stream];
    if (!sl.k.valid) return fail(RY_ESTATE, "stream %d holds no window: no ry_crepe_bank_track has named it, or ry_crepe_bank_reset came after it", stream);
    return read_activation(b->ctx, sl, out, on_device);
}

int ry_crepe_bank_debug_poison(ry_crepe_bank* b, int* rows_left) {
    RY_TRY(check_handle(b, "crepe bank"));
    if (!rows_left) return fail(RY_EINVAL, "bad argument");
    const ry_stream_t s = b->ctx->stream;
    RT_TRY(rt::stream_sync(s));
    // all bits set in the packed block, both sets of tables and whatever of every slot the rule may not hand to the next call
    RY_TRY(b->fresh.poison(s));
    for (int i = 0; i < 2; ++i) {
        RY_TRY(b->tab(i).poison(s));
        b->tab_on_card[i] = false;
    }
    for (size_t i = 0; i < b->slots.size(); ++i) RY_TRY(poison_slot(*b->slots[i], s, &rows_left[i]));
    RT_TRY(rt::stream_sync(s));
    return RY_OK;
}

int ry_crepe_bank_debug_uploads(ry_crepe_bank* b, long long* n_uploads) {
    if (!b || !n_uploads) return fail(RY_EINVAL, "bad argument");
    *n_uploads = b->uploads;
    return RY_OK;
}

int ry_crepe_bank_debug_assemble(ry_crepe_bank* b, const int* n_frames, int n_waves, const float* const* keep_dev, const int* n_keep,
                                 float* const* write_dev, const float* fresh_dev, int n_fresh, const int* src, float* out_dev) {
    RY_TRY(check_handle(b, "crepe bank"));
    if (!n_frames || !keep_dev || !n_keep || !write_dev || !fresh_dev || !src || !out_dev || n_fresh < 0) return fail(RY_EINVAL, "bad argument");
    std::vector<CrepeSeg> plan;
    RY_TRY(plan_segments(n_waves, nullptr, nullptr, n_frames, &plan));
    for (int i = 0; i < n_waves; ++i)
        if (n_keep[i] < 0 || !write_dev[i] || (n_keep[i] > 0 && !keep_dev[i])) return fail(RY_EINVAL, "wave %d: bad slot", i);
    const int total = plan.back().frame0 + plan.back().n_frames;
    // descriptors | segment table | src in the first table buffer; the card's tables are no longer those of a call
    const size_t desc_ints = 6 * (size_t)n_waves;
    static_assert(sizeof(CrepeSeg) == 6 * sizeof(int), "the segment table is copied as six ints per wave");
    std::vector<int>& tab = b->tab_host[0];
    b->tab_on_card[0] = false;
    tab.assign(2 * desc_ints + (size_t)total, 0);
    for (int i = 0; i < n_waves; ++i) {
        CrepeBankWave d;
        d.keep = keep_dev[i]; d.n_keep = n_keep[i]; d.write = write_dev[i]; d.pad = 0;
        memcpy(&tab[6 * (size_t)i], &d, sizeof d);
        memcpy(&tab[desc_ints + 6 * (size_t)i], &plan[(size_t)i], sizeof(CrepeSeg));
    }
    memcpy(&tab[2 * desc_ints], src, (size_t)total * sizeof(int));
    const ry_stream_t s = b->ctx->stream;
    RY_TRY(b->tab0.grow(b->ctx, (long long)tab.size()));
    RT_TRY(rt::h2d(b->tab0.ptr(), tab.data(), tab.size() * sizeof(int), s));
    const int* d = b->tab0.ptr();
    RY_TRY(launch_assemble_many(b->ctx, (const CrepeSeg*)(d + desc_ints), n_waves, (const CrepeBankWave*)d, d + 2 * desc_ints, fresh_dev, n_fresh,
                                out_dev, total));
    RT_TRY(rt::stream_sync(s));
    return RY_OK;
}

}  // extern "C"
