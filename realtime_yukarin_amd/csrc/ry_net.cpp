// ry_net.cpp -- the predictor C ABI of libry355.so (include/ry355.h): context and predictor lifetime, dtype modes, the forward / convert entry points,
// profiling and planner debug hooks.  Planner: ry_plan.cpp; kernels + launchers + single operators: ry_exec.cpp; shared declarations: ry_plan.h /
// ry_host.h; window call: ry_vc.cpp.
//
// Build (product): hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip -c <each unit>, linked into libry355.so   (realtime_yukarin_amd/build.py)
// Build (test emulator, no GPU): clang++ -x c++ -DRY_HOST_EMU ... the same units + tests/emu/ry_emu.cpp
//
// What the reference does here (all inside un-vendored dependencies, [MEM]): Chainer builds the
// predictor from config.model, load_npz fills it, to_gpu moves it, and every convert() call runs 16
// conv/deconv links + BatchNormalization + activations one cuDNN/CuPy launch at a time with a
// materialised F.concat per decoder layer (call sites: realtime_voice_conversion/yukarin_wrapper/
// voice_changer.py:33,41).  Here: filters are re-laid out once at creation (BN folded to scale/shift),
// a plan per (batch, frames) owns all activation buffers, and the whole forward -- pad/log wrapper
// kernels, 16 fused layers, exp/crop -- is captured once into a hipGraph and replayed per buffer.
#include "ry_plan.h"

thread_local std::string g_ry_err;

// A second handle on the same predictor: the filters stay where they are (one copy in HBM, freed with the last handle), the clone
// gets its own launch plans, activation buffers and captured graphs -- what a window needs to run beside another one -- and its own
// stream, unless the caller names one (`borrowed`: a stream of another handle that outlives the clone; none is created then, because a
// stream takes a place on a hardware queue when it is created, used or not).
int net_clone_on(ry_net* src, ry_stream_t borrowed, ry_net** out) {
    if (!src || !out) return fail(RY_EINVAL, "null argument");
    *out = nullptr;
    ry_ctx* ctx = src->ctx;
    RT_TRY(rt::set_device(ctx->device));
    std::unique_ptr<ry_net> net(new ry_net());
    net->ctx = ctx; net->desc = src->desc; net->dtype = src->dtype; net->use_graph = src->use_graph;
    net->layers = src->layers;                       // device pointers into the shared arena
    net->weights = src->weights;
    if (borrowed) { net->stream = borrowed; net->owns_stream = false; }
    else RT_TRY(rt::stream_create(&net->stream));
    RT_TRY(rt::event_create_fast(&net->done));
    net->has_done = true;
    ctx->nets.push_back(net.get());
    *out = net.release();
    return RY_OK;
}

extern "C" {


const char* ry_last_error(void) { return g_ry_err.c_str(); }

int ry_device_count(void) {
    int n = 0;
    if (rt::device_count(&n) != 0) return 0;
    return n;
}

int ry_init(int device, ry_ctx** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    int n = 0;
    RT_TRY(rt::device_count(&n));
    if (device < 0 || device >= n) return fail(RY_EINVAL, "device %d out of range (%d visible)", device, n);
    RT_TRY(rt::set_device(device));
    std::unique_ptr<ry_ctx> c(new ry_ctx());
    c->device = device;
    RT_TRY(rt::stream_create(&c->stream));
    RT_TRY(rt::event_create(&c->t0));
    RT_TRY(rt::event_create(&c->t1));
    c->timers = true;
    RY_TRY(read_env_switches());
    *out = c.release();
    return RY_OK;
}

void ry_shutdown(ry_ctx* ctx) {
    if (!ctx) return;
    rt::set_device(ctx->device);
    rt::stream_sync(ctx->stream);
    if (ctx->timers) { rt::event_destroy(ctx->t0); rt::event_destroy(ctx->t1); }
    rt::stream_destroy(ctx->stream);
    for (void* q : ctx->owned) rt::dfree(q);
    delete ctx;
}

int ry_sync(ry_ctx* ctx) {
    if (!ctx) return fail(RY_ESTATE, "null context");
    for (ry_net* n : ctx->nets) RT_TRY(rt::stream_sync(n->stream));
    RT_TRY(rt::stream_sync(ctx->stream));
    return RY_OK;
}

void* ry_stream(ry_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int ry_timer_start(ry_ctx* ctx) {
    if (!ctx) return fail(RY_ESTATE, "null context");
    // Everything queued so far is waited for on the HOST, then t0 is recorded and waited for: whatever is enqueued afterwards starts after
    // t0 without a cross-stream wait.  (The former form -- every predictor stream waits on t0 with hipStreamWaitEvent -- left the two
    // window lanes of ry_vc serialised for the rest of the run: 1.32 instead of 1.16 ms per window, round 2.)
    for (ry_net* n : ctx->nets) RT_TRY(rt::stream_sync(n->stream));
    RT_TRY(rt::stream_sync(ctx->stream));
    RT_TRY(rt::event_record(ctx->t0, ctx->stream));
    RT_TRY(rt::event_sync(ctx->t0));
    return RY_OK;
}

int ry_timer_stop(ry_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(RY_EINVAL, "null argument");
    // t1 after every predictor stream, joined on the HOST: an event record on each predictor stream plus hipStreamWaitEvent from the
    // context stream, issued while the two window lanes of ry_vc still had work queued, cost them their overlap for the rest of the run
    // (1.33 instead of 1.16 ms per window, BENCH_TIMER_MODE sweep of round 2)
    for (ry_net* n : ctx->nets) RT_TRY(rt::stream_sync(n->stream));
    RT_TRY(rt::event_record(ctx->t1, ctx->stream));
    RT_TRY(rt::event_sync(ctx->t1));
    RT_TRY(rt::event_elapsed(ms, ctx->t0, ctx->t1));
    return RY_OK;
}

size_t ry_net_param_count(const ry_net_desc* desc) {
    if (check_desc(desc) != RY_OK) return 0;
    size_t n = 0;
    for (const Layer& l : build_topology(*desc)) n += layer_param_count(l, desc->ndim);
    return n;
}

int ry_net_create(ry_ctx* ctx, const ry_net_desc* desc, const float* weights, size_t n_floats, int on_device, ry_net** out) {
    if (!ctx || !out || !weights) return fail(RY_EINVAL, "null argument");
    *out = nullptr;
    RY_TRY(check_desc(desc));
    const size_t want = ry_net_param_count(desc);
    if (n_floats != want) return fail(RY_EINVAL, "weight blob has %zu floats, the predictor needs %zu", n_floats, want);
    RT_TRY(rt::set_device(ctx->device));
    std::vector<float> host;
    const float* blob = weights;
    if (on_device) {
        host.resize(n_floats);
        RT_TRY(rt::d2h(host.data(), weights, n_floats * sizeof(float), ctx->stream));
        RT_TRY(rt::stream_sync(ctx->stream));
        blob = host.data();
    }
    std::unique_ptr<ry_net> net(new ry_net());
    net->ctx = ctx;
    net->desc = *desc;
    if (net->desc.bn_eps <= 0.f) net->desc.bn_eps = 2e-5f;
    net->layers = build_topology(*desc);
    if (const char* e = getenv("RY_GRAPH")) net->use_graph = atoi(e) != 0;
    RT_TRY(rt::stream_create(&net->stream));
    RT_TRY(rt::event_create_fast(&net->done));
    net->has_done = true;
    if (on_device) net->weights->stats.bytes_downloaded += (unsigned long long)(n_floats * sizeof(float));
    size_t off = 0;
    int rc = RY_OK;
    for (Layer& l : net->layers) {
        const size_t nw = (size_t)l.cin() * l.cout * ipow((size_t)l.k, desc->ndim);
        const float* W = blob + off; off += nw;
        const float* b = blob + off; off += l.cout;
        const float* bn = nullptr;
        if (l.bn) { bn = blob + off; off += 4 * (size_t)l.cout; }
        rc = prepare_layer(ctx, *net->weights, l, desc->ndim, net->desc.bn_eps, W, b, bn);
        if (rc != RY_OK) break;
    }
    // filter build mode `device`: the layout kernels and the copies of the raw filters are queued on the context stream -- one wait for all of them
    // (the blob is the caller's, or `host` above), then the staging buffer goes back; after a refusal too
    if (rc != RY_OK) { const std::string why = g_ry_err; finish_filter_build(ctx); g_ry_err = why; return rc; }
    RY_TRY(finish_filter_build(ctx));
    ctx->nets.push_back(net.get());
    *out = net.release();
    return RY_OK;
}

// A second handle on the same predictor: the filters stay where they are (one copy in HBM, freed with the last handle), the clone
// gets its own stream, launch plans, activation buffers and captured graphs -- what a window needs to run beside another one.
int ry_net_clone(ry_net* src, ry_net** out) { return net_clone_on(src, nullptr, out); }

void ry_net_destroy(ry_net* net) {
    if (!net) return;
    rt::set_device(net->ctx->device);
    rt::stream_sync(net->stream);
    rt::stream_sync(net->ctx->stream);
    auto& v = net->ctx->nets;
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i] == net) { v.erase(v.begin() + i); break; }
    net->plans.clear(); net->last_plan = nullptr;
    if (net->has_done) rt::event_destroy(net->done);
    if (net->owns_stream) rt::stream_destroy(net->stream);
    delete net;
}

int ry_net_set_dtype(ry_net* net, int dtype) {
    if (!net) return fail(RY_EINVAL, "null argument");
    if (dtype < 0 || dtype > 2) return fail(RY_EINVAL, "dtype must be 0 (fp32), 1 (bf16 operands, fp32 accumulate) or 2 (split-bf16: three bf16 products per fp32 product, fp32 accumulate)");
    if (dtype != 0 && net->desc.ndim != 2) return fail(RY_EINVAL, "the bf16 variants exist for the stage-2 predictor only");
    ry_ctx* ctx = net->ctx;
    RT_TRY(rt::set_device(ctx->device));
    RT_TRY(rt::stream_sync(net->stream));
    RY_TRY(read_plan_env());
    if (dtype == 2)
        if (const char* e = getenv("RY_X3_MINM")) g_x3_min_m = atoi(e);      // read again here so that a test / sweep can move it per call
    if (dtype != 0)
        for (Layer& l : net->layers) RY_TRY(prepare_bf16(ctx, *net->weights, l, dtype));
    net->dtype = dtype;
    net->plans.clear(); net->last_plan = nullptr;    // launch plans (and captured graphs) depend on the kernel choice
    return RY_OK;
}

int ry_net_forward(ry_net* net, const float* x, float* y, int batch, int frames, int on_device) {
    if (!net || !x || !y) return fail(RY_EINVAL, "null argument");
    Plan* P = nullptr;
    RY_TRY(get_plan(net, batch, frames, 0, 0, &P));
    return run_plan(net, *P, x, y, on_device);
}

static int convert_common(ry_net* net, int want_ndim, const float* x, float* y, int batch, int n_frames, int on_device,
                          int disc_front = 0, int disc_back = 0) {
    if (!net || !x || !y) return fail(RY_EINVAL, "null argument");
    if (net->desc.ndim != want_ndim) return fail(RY_EINVAL, "wrong predictor: this call needs a stage-%d net", want_ndim);
    if (n_frames < 1) return fail(RY_EINVAL, "n_frames must be positive (got %d)", n_frames);
    if (disc_front < 0 || disc_back < 0) return fail(RY_EINVAL, "discarded frame counts must not be negative (got %d, %d)", disc_front, disc_back);
    if (disc_front >= (1 << 20) || disc_back >= (1 << 20)) return fail(RY_EINVAL, "discarded frame counts are limited to 2^20");
    const int T = n_frames + (128 - n_frames % 128);
    Plan* P = nullptr;
    RY_TRY(get_plan(net, batch, T, 1, n_frames, &P));
    P->disc_front = disc_front; P->disc_back = disc_back;
    RY_TRY(run_plan(net, *P, x, y, on_device));
    if (!on_device && want_ndim == 2 && (disc_front > 0 || disc_back > 0)) {       // host arrays: the rows that were not computed come back as zeros
        int k0, k1;
        keep_rows(n_frames, disc_front, disc_back, &k0, &k1);
        const size_t cols = (size_t)net->desc.width + 1;
        for (int b = 0; b < batch; ++b) {
            float* yb = y + (size_t)b * n_frames * cols;
            if (k0 > 0) memset(yb, 0, (size_t)k0 * cols * sizeof(float));
            if (k1 < n_frames) memset(yb + (size_t)k1 * cols, 0, (size_t)(n_frames - k1) * cols * sizeof(float));
        }
    }
    return RY_OK;
}

int ry_ac_convert(ry_net* net, const float* x, float* y, int batch, int n_frames, int on_device) {
    return convert_common(net, 1, x, y, batch, n_frames, on_device);
}

int ry_sr_convert(ry_net* net, const float* sp, float* out, int batch, int n_frames, int on_device) {
    return convert_common(net, 2, sp, out, batch, n_frames, on_device);
}

// The same for a caller that will throw away the first `discard_front` and the last `discard_back` frames of every window (the live
// caller: ConvertStream.process picks [pad, -pad) of what it converted, realtime_voice_conversion/stream/convert_stream.py:40-42):
// rows [discard_front, n_frames - discard_back) of `out` are written, bit-identical to ry_sr_convert; the other rows are left untouched.
int ry_sr_convert_rows(ry_net* net, const float* sp, float* out, int batch, int n_frames, int discard_front, int discard_back, int on_device) {
    return convert_common(net, 2, sp, out, batch, n_frames, on_device, discard_front, discard_back);
}

int ry_net_profile(ry_net* net, int batch, int frames, int reps, ry_kernel_stat* stats, int max_stats, int* n_stats) {
    if (!net || !stats || !n_stats || reps < 1) return fail(RY_EINVAL, "bad argument");
    Plan* P = nullptr;
    RY_TRY(get_plan(net, batch, frames, 0, 0, &P));
    return profile_plan(net, P, reps, stats, max_stats, n_stats);
}

int ry_net_profile_window(ry_net* net, int n_frames, int reps, ry_kernel_stat* stats, int max_stats, int* n_stats) {
    if (!net || !stats || !n_stats || reps < 1 || n_frames < 1) return fail(RY_EINVAL, "bad argument");
    Plan* P = nullptr;
    RY_TRY(get_plan(net, 1, n_frames + (128 - n_frames % 128), 1, n_frames, &P));
    P->disc_front = P->disc_back = 0;
    return profile_plan(net, P, reps, stats, max_stats, n_stats);
}

// tests: one buffer of the plan that ran last on this handle, copied to the host after the stream has drained -- no node, no copy and no flag on
// the forward / convert path itself (run_plan only remembers the plan's address).  layer -1: the padded input x_in of the convert wrapper
// [B][T][cols]; layer 0 .. 15: kind 0 the fp32 output [B][Ho][Wo][Cout], kind 1 its 16-bit copy as raw uint16, plain bf16 [pixel][Cout] or split-bf16
// [pixel][hi (Cout) | lo (Cout)].  dims = {B, H, W, elements per pixel, format (0 fp32, 1 bf16, 2 split-bf16)}; out may be null (dims only), else
// out_bytes must be the exact size.  RY_EINVAL when this plan has no such buffer or nothing wrote it: a copy no consumer reads (w32 / w16), a last
// layer that stores into the caller's block, x_in of a raw forward or of a stage-1 window whose first layer pads for itself.
int ry_net_debug_activation(ry_net* net, int layer, int kind, void* out, size_t out_bytes, int* dims) {
    if (!net || !dims) return fail(RY_EINVAL, "null argument");
    const Plan* P = net->last_plan;
    if (!P) return fail(RY_EINVAL, "no forward or convert has run on this handle since its plans were dropped");
    const int nd = net->desc.ndim;
    const void* src = nullptr;
    size_t esize = 4;
    if (layer == -1 && kind == 0) {
        if (P->mode != 1 || !P->x_in) return fail(RY_EINVAL, "the raw forward has no padded input: it reads the caller's block");
        if (plan_padfuse_now(net, *P)) return fail(RY_EINVAL, "the first layer of this window padded the caller's block itself: x_in was not written");
        dims[0] = P->B; dims[1] = P->T; dims[2] = nd == 1 ? net->desc.in_ch : net->desc.width; dims[3] = 1; dims[4] = 0;
        src = P->x_in;
    } else if (layer >= 0 && layer < 16 && (kind == 0 || kind == 1)) {
        if (nd != 2) return fail(RY_EINVAL, "layer buffers are handed back for the stage-2 predictor only");
        const LayerPlan& lp = P->lp[layer];
        const int N = net->layers[layer].cout;
        dims[0] = P->B; dims[1] = lp.Ho; dims[2] = lp.Wo;
        if (kind == 0) {
            if (layer == 15 && (P->mode == 0 || lp.path == PATH_LAST)) return fail(RY_EINVAL, "%s stored into the caller's block", net->layers[layer].name);
            if (!lp.w32 && lp.w16) return fail(RY_EINVAL, "%s writes no fp32 copy in this plan", net->layers[layer].name);
            dims[3] = N; dims[4] = 0; src = lp.out;
        } else {
            if (!lp.w16 || !lp.out16) return fail(RY_EINVAL, "%s writes no 16-bit copy in this plan", net->layers[layer].name);
            dims[3] = lp.o16x3 ? 2 * N : N; dims[4] = lp.o16x3 ? 2 : 1; src = lp.out16; esize = 2;
        }
    } else {
        return fail(RY_EINVAL, "layer must be -1 (kind 0) or 0 .. 15 with kind 0 (fp32) or 1 (16-bit copy); got %d, %d", layer, kind);
    }
    if (!out) return RY_OK;
    const size_t want = (size_t)dims[0] * dims[1] * dims[2] * dims[3] * esize;
    if (out_bytes != want) return fail(RY_EINVAL, "the buffer holds %zu bytes, this block has %zu", out_bytes, want);
    RT_TRY(rt::set_device(net->ctx->device));
    RT_TRY(rt::stream_sync(net->stream));
    RT_TRY(rt::d2h(out, src, want, net->stream));
    RT_TRY(rt::stream_sync(net->stream));
    return RY_OK;
}

// tests: the records of a (batch, frames) plan -- LayerPlan as build_plan left it, with the rows plan_window_rows gives one enqueue and what the
// launchers derive from both (tile shape, patch variant, reduce kernel: the same functions they call).  Reads; enqueues nothing.
int ry_net_debug_plan(ry_net* net, int batch, int frames, int window, int discard_front, int discard_back, ry_plan_record* records, int max, int* n) {
    if (!net || !records || !n) return fail(RY_EINVAL, "null argument");
    *n = 0;
    if (net->desc.ndim != 2) return fail(RY_EINVAL, "plan records are handed back for the stage-2 predictor only");
    if (window != 0 && window != 1) return fail(RY_EINVAL, "window must be 0 (raw forward) or 1 (convert wrapper); got %d", window);
    if (frames < 1 || batch < 1) return fail(RY_EINVAL, "batch and frames must be positive (got %d, %d)", batch, frames);
    if (discard_front < 0 || discard_back < 0 || (!window && (discard_front || discard_back)))
        return fail(RY_EINVAL, "discarded frame counts must not be negative, and the raw forward has none (got %d, %d)", discard_front, discard_back);
    if (max < 16) return fail(RY_EINVAL, "room for %d records, a plan has 16", max);
    RT_TRY(rt::set_device(net->ctx->device));
    Plan* P = nullptr;
    if (window) RY_TRY(get_plan(net, batch, frames + (128 - frames % 128), 1, frames, &P));
    else RY_TRY(get_plan(net, batch, frames, 0, 0, &P));
    const int df = P->disc_front, db = P->disc_back;
    P->disc_front = discard_front; P->disc_back = discard_back;
    const WindowRows rows = plan_window_rows(net, *P);
    P->disc_front = df; P->disc_back = db;
    for (int i = 0; i < 16; ++i) {
        const Layer& l = net->layers[i];
        LayerPlan lq = P->lp[i];                                  // as enqueue_forward hands it to the launcher
        if (rows.hole_n[i] > 0) { lq.hole_lo = rows.hole_lo[i]; lq.hole_n = rows.hole_n[i]; }
        if (rows.crop_hi[i] > 0) { lq.crop_hi = rows.crop_hi[i]; lq.crop_lo = rows.crop_lo[i]; }
        ry_plan_record& r = records[i];
        memset(&r, 0, sizeof r);
        r.layer = i; r.path = lq.path; r.splits = lq.splits;
        const bool igemm = lq.path == PATH_IGEMM || lq.path == PATH_IGEMM_BF16, gemm = igemm || lq.path == PATH_WINO;
        if (igemm) { r.tile = lq.tile; r.kgroups = lq.kg; }
        if (lq.path == PATH_WINO) { r.wino_cfg = lq.wino_cfg; r.wino_mbw = lq.wino_mbw; }
        if (lq.path == PATH_OS2D) { r.os2[0] = lq.os2_mt4; r.os2[1] = lq.os2_nt4; r.os2[2] = lq.os2_waves; r.os2[3] = lq.os2_depth; }
        r.reads16 = lq.path == PATH_IGEMM_BF16 ? (lq.x3 ? 2 : 1) : 0;
        r.writes32 = lq.w32 ? 1 : 0; r.writes16 = lq.w16 ? (lq.o16x3 ? 2 : 1) : 0;
        r.rows_out = lq.Ho;
        r.out_n = lq.Ho;
        if (lq.path == PATH_LAST) {
            r.last_exp = lq.last_exp;
            if (P->mode == 1) { r.out_lo = rows.k0; r.out_n = rows.k1 - rows.k0; }
        }
        if (gemm || lq.path == PATH_OS2D || lq.path == PATH_DIRECT) { r.grid_rows = l.deconv ? lq.Hi : lq.Ho; r.grid_cols = l.deconv ? lq.Wi : lq.Wo; }
        if (gemm) {
            const int up = l.deconv ? 2 : 1;
            int Mh = r.grid_rows;
            if (lq.crop_hi > 0) { Mh = lq.crop_hi; r.crop_lo = lq.crop_lo; r.crop_n = lq.crop_hi; r.out_lo = up * lq.crop_lo; r.out_n = up * lq.crop_hi; }
            r.hole_lo = lq.hole_lo; r.hole_n = lq.hole_n;
            int th = 0, tw = 0;
            if (plan_tile_rows(lq, Mh, r.grid_cols, &th, &tw)) { r.tile_rows = th; r.tile_cols = tw; } else tw = 0;
            if (igemm) r.patch = plan_igemm_patch(l, lq, batch * Mh * r.grid_cols, tw, l.cin() / (lq.path == PATH_IGEMM_BF16 ? 64 : 32) * (lq.x3 ? 3 : 1));
            if (lq.splits > 1) {
                const long long total = batch == 1 ? (long long)up * Mh * lq.Wo * l.cout : (long long)batch * lq.Ho * lq.Wo * l.cout;
                r.reduce = plan_reduce_wide(lq.splits, total) ? 2 : 1;
            }
        }
    }
    *n = 16;
    return RY_OK;
}

int ry_set_filter_build(int mode) { return set_filter_build(mode); }

int ry_net_build_stats(ry_net* net, ry_build_stats* out) {
    if (!net || !out) return fail(RY_EINVAL, "null argument");
    *out = net->weights->stats;
    return RY_OK;
}

// tests: one filter layout of a layer as it lies on the card.  Every refusal comes before anything is built or written.
int ry_net_debug_filters(ry_net* net, int layer, int kind, float* out, size_t out_floats, size_t* n_floats) {
    if (!net || !n_floats) return fail(RY_EINVAL, "null argument");
    if (layer < 0 || layer >= (int)net->layers.size()) return fail(RY_EINVAL, "layer must be 0 .. 15 (got %d)", layer);
    if (kind < RY_LAYOUT_W1D || kind > RY_LAYOUT_WWIN) return fail(RY_EINVAL, "kind must be 0 (w1d), 1 (w1os), 2 (wig), 3 (wdir), 4 (w2os) or 5 (wwin); got %d", kind);
    const Layer& l = net->layers[layer];
    const float* src = kind == RY_LAYOUT_W1D ? l.w1d : kind == RY_LAYOUT_W1OS ? l.w1os : kind == RY_LAYOUT_WIG ? l.wig : kind == RY_LAYOUT_WDIR ? l.wdir
                     : kind == RY_LAYOUT_W2OS ? l.w2os : nullptr;
    if (kind == RY_LAYOUT_WWIN ? !(l.wdir && wino_eligible(l, net->desc.ndim)) : !src) return fail(RY_ESTATE, "%s has no layout of kind %d", l.name, kind);
    const size_t n = filter_layout_floats(l, kind);
    *n_floats = n;
    if (!out || out_floats < n) return fail(RY_EINVAL, "%s: the layout has %zu floats, the buffer holds %zu", l.name, n, out ? out_floats : (size_t)0);
    RT_TRY(rt::set_device(net->ctx->device));
    if (kind == RY_LAYOUT_WWIN) RY_TRY(net_wwin(net, layer, &src));
    RT_TRY(rt::stream_sync(net->stream));
    RT_TRY(rt::d2h(out, src, n * sizeof(float), net->ctx->stream));
    RT_TRY(rt::stream_sync(net->ctx->stream));
    return RY_OK;
}

// tests: the same for ONE layer of any shape prepare_layer takes, without a predictor around it -- the layer's filters are built in an arena of the
// call, in the mode in force, from the raw filter W (host), and one layout comes back.  cin_b > 0: two skip sources.  want_os2: the output-stationary
// layout whatever the filter's size (as ry_conv2d's path 7).
int ry_debug_layer_filters(ry_ctx* ctx, int ndim, int cin_a, int cin_b, int cout, int k, int stride, int pad, int transposed, int want_os2,
                           const float* W, int kind, float* out, size_t out_floats, size_t* n_floats) {
    if (!ctx || !W || !n_floats) return fail(RY_EINVAL, "null argument");
    if ((ndim != 1 && ndim != 2) || cin_a < 1 || cin_b < 0 || cout < 1 || k < 1 || k > 4 || stride < 1 || pad < 0) return fail(RY_EINVAL, "bad layer shape");
    if (transposed && !(k == 4 && stride == 2 && pad == 1)) return fail(RY_EINVAL, "transposed layers are k4 s2 p1 only");
    if (kind < RY_LAYOUT_W1D || kind > RY_LAYOUT_WWIN) return fail(RY_EINVAL, "kind must be 0 .. 5 (got %d)", kind);
    RT_TRY(rt::set_device(ctx->device));
    Layer l;
    snprintf(l.name, sizeof l.name, "layer");
    l.deconv = transposed != 0; l.k = k; l.stride = stride; l.pad = pad; l.cin_a = cin_a; l.cin_b = cin_b; l.cout = cout;
    Arena arena;
    int rc = prepare_layer(ctx, arena, l, ndim, 2e-5f, W, nullptr, nullptr, want_os2 != 0);
    if (rc != RY_OK) { const std::string why = g_ry_err; finish_filter_build(ctx); g_ry_err = why; return rc; }
    RY_TRY(finish_filter_build(ctx));
    const float* src = kind == RY_LAYOUT_W1D ? l.w1d : kind == RY_LAYOUT_W1OS ? l.w1os : kind == RY_LAYOUT_WIG ? l.wig : kind == RY_LAYOUT_WDIR ? l.wdir
                     : kind == RY_LAYOUT_W2OS ? l.w2os : nullptr;
    if (kind == RY_LAYOUT_WWIN ? !(l.wdir && wino_eligible(l, ndim)) : !src) return fail(RY_ESTATE, "this layer has no layout of kind %d", kind);
    const size_t n = filter_layout_floats(l, kind);
    *n_floats = n;
    if (!out || out_floats < n) return fail(RY_EINVAL, "the layout has %zu floats, the buffer holds %zu", n, out ? out_floats : (size_t)0);
    if (kind == RY_LAYOUT_WWIN) { float* w = nullptr; RY_TRY(upload_wwin(ctx, arena, l, &w)); src = w; }
    RT_TRY(rt::d2h(out, src, n * sizeof(float), ctx->stream));
    RT_TRY(rt::stream_sync(ctx->stream));
    return RY_OK;
}

// diagnostics / tests: read the process-wide RY_* switches again (they are otherwise read when a context is created; launch plans built before keep
// their choices until ry_net_set_dtype drops them)
int ry_debug_reload_env(void) { return read_env_switches(); }

// diagnostics: the plan (tile, external splits, K groups, estimated time) the stage-2 planner picks for one layer shape
int ry_debug_plan_igemm(int M, int Cout, int nphases, int nk, int* tile, int* splits, int* kgroups, double* est_us) {
    if (!tile || !splits || !kgroups) return fail(RY_EINVAL, "null argument");
    if (M < 1 || Cout < 64 || Cout % 64 != 0 || nphases < 1 || nk < 1) return fail(RY_EINVAL, "not an implicit-GEMM layer shape");
    Layer l; l.cout = Cout;
    *tile = 0; *splits = 0; *kgroups = 0;
    choose_igemm(l, M, nphases, nk, tile, splits, kgroups);
    if (est_us) {
        int bm, bn; tile_dims(*tile, &bm, &bn);
        *est_us = est_time((long)((M + bm - 1) / bm) * (Cout / bn) * nphases, bm, bn, *splits, tile_occ(*tile, *kgroups), *kgroups, M, Cout, nk);
    }
    return RY_OK;
}

// the same for the bf16 (mode 1) / split-bf16 (mode 2) kernels (nk counts 64-channel chunks: taps x Cin / 64, three times that in
// split-bf16 mode); non-zero *tile / *splits / *kgroups on entry are kept (the estimate of a given plan)
int ry_debug_plan_igemm_bf16(int mode, int M, int Cout, int nphases, int nk, int* tile, int* splits, int* kgroups, double* est_us) {
    if (mode != 1 && mode != 2) return fail(RY_EINVAL, "mode must be 1 (bf16) or 2 (split-bf16)");
    if (!tile || !splits || !kgroups) return fail(RY_EINVAL, "null argument");
    if (M < 1 || Cout < 64 || Cout % 64 != 0 || nphases < 1 || nk < 1) return fail(RY_EINVAL, "not an implicit-GEMM layer shape");
    Layer l; l.cout = Cout;
    choose_igemm(l, M, nphases, nk, tile, splits, kgroups, mode);
    if (est_us) {
        int bm, bn; tile_dims(*tile, &bm, &bn);
        *est_us = est_time((long)((M + bm - 1) / bm) * (Cout / bn) * nphases, bm, bn, *splits, tile_occ(*tile, *kgroups), *kgroups, M, Cout, nk)
                  * (M > 64 && Cout % 128 == 0 ? (1.0 / bm + 1.0 / bn) * 64.0 : 1.0);
    }
    return RY_OK;
}

// diagnostics: the output-stationary slice the planner picks for one layer shape (choose_os2)
int ry_debug_plan_os2(int M, int Cout, int nphases, int units, int* mt4, int* nt4, int* waves, int* depth, double* cost) {
    if (!mt4 || !nt4 || !waves || !depth) return fail(RY_EINVAL, "null argument");
    if (M < 1 || Cout < 4 || Cout % 4 != 0 || nphases < 1 || units < 1) return fail(RY_EINVAL, "not an output-stationary layer shape");
    if (!choose_os2(M, Cout, nphases, units, mt4, nt4, waves, depth, cost))
        return fail(RY_EINVAL, "no output-stationary slice for %d rows x %d channels x %d units", M, Cout, units);
    return RY_OK;
}

int ry_debug_plan_wino(int Mh, int Mw, int Cout, int nphases, int npatches, int batch, int* cfg, int* mbw, int* splits) {
    if (!cfg || !mbw || !splits) return fail(RY_EINVAL, "null argument");
    if (Mh < 1 || Mw < 1 || Cout < 64 || Cout % 64 || (nphases != 1 && nphases != 4) || npatches < 1 || batch < 1) return fail(RY_EINVAL, "not a Winograd layer shape");
    if (!choose_wino(Mh, Mw, Cout, nphases, npatches, batch, cfg, mbw, splits)) return fail(RY_EINVAL, "no Winograd tile divides a %d x %d grid", Mh, Mw);
    return RY_OK;
}

}  // extern "C"
