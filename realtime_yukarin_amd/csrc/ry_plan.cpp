// ry_plan.cpp -- the planner of libry355.so: U-Net topology, filter re-layout at predictor creation (BN folded to scale / shift), the per-layer choice of
// kernel family, tile, split-K and K groups (stage 2: implicit GEMM / Winograd / output-stationary, for predictors and the single operator ry_conv2d; stage 1:
// output-stationary slices), the launch plan of a (batch, frames) window with its activation buffers, the rows each enqueue computes, and the environment
// switches.  No device code: the launchers are ry_exec.cpp.
#include "ry_plan.h"

// ------------------------------------------------------------------------------------------------
// topology (same K-list order as realtime_yukarin_amd/netspec.py)
// ------------------------------------------------------------------------------------------------
static const int ENC_CH[8] = {1, 2, 4, 8, 8, 8, 8, 8};
static const int DEC_IN[7] = {8, 16, 16, 16, 16, 8, 4};
static const int DEC_OUT[7] = {8, 8, 8, 8, 4, 2, 1};

std::vector<Layer> build_topology(const ry_net_desc& d) {
    std::vector<Layer> L(16);
    const int B = d.base, e = d.extensive_layers;
    const int end_k = e > 0 ? 3 : 1;
    // glu_generator (stage 1, UNVERIFIED [MEM]): a conv + BN block computes 2 x co channels (value | gate), its consumers see co = value * sigmoid(gate)
    const int g = (d.glu && d.ndim == 1) ? 2 : 1;
    const int blk_act_e = g == 2 ? RY_ACT_GLU : RY_ACT_LRELU, blk_act_d = g == 2 ? RY_ACT_GLU : RY_ACT_RELU;
    auto nm = [](Layer& l, const char* p, int i) { snprintf(l.name, sizeof l.name, "%s/c%d", p, i); };
    {   // encoder c0: conv + bias, leaky_relu
        Layer& l = L[0]; nm(l, "encoder", 0);
        l.k = end_k; l.stride = 1; l.pad = end_k / 2; l.cin_a = d.in_ch; l.cout = B; l.src_a = -1; l.act = RY_ACT_LRELU;
    }
    for (int i = 1; i < 8; ++i) {
        Layer& l = L[i]; nm(l, "encoder", i);
        const bool down = i < e;
        l.k = down ? 4 : 1; l.stride = down ? 2 : 1; l.pad = down ? 1 : 0;
        l.cin_a = ENC_CH[i - 1] * B; l.cout = ENC_CH[i] * B * g; l.src_a = i - 1; l.bn = true; l.act = blk_act_e;
    }
    for (int j = 0; j < 7; ++j) {
        Layer& l = L[8 + j]; nm(l, "decoder", j);
        const bool up = (7 - j) < e;
        l.deconv = up; l.k = up ? 4 : 1; l.stride = up ? 2 : 1; l.pad = up ? 1 : 0;
        l.cout = DEC_OUT[j] * B * g; l.bn = true; l.act = blk_act_d;
        if (j == 0) { l.cin_a = DEC_IN[0] * B; l.src_a = 7; }
        else { l.cin_a = DEC_OUT[j - 1] * B; l.cin_b = ENC_CH[7 - j] * B; l.src_a = 8 + j - 1; l.src_b = 7 - j; }
    }
    {   // decoder c7: conv + bias on concat(decoder c6, encoder c0)
        Layer& l = L[15]; nm(l, "decoder", 7);
        l.k = end_k; l.stride = 1; l.pad = end_k / 2; l.cin_a = B; l.cin_b = B; l.cout = d.out_ch; l.src_a = 14; l.src_b = 0;
        l.act = RY_ACT_NONE;
    }
    return L;
}

size_t ipow(size_t b, int e) { size_t r = 1; while (e-- > 0) r *= b; return r; }

size_t layer_param_count(const Layer& l, int ndim) {
    size_t n = (size_t)l.cin() * l.cout * ipow((size_t)l.k, ndim) + l.cout;
    if (l.bn) n += 4 * (size_t)l.cout;
    return n;
}

int check_desc(const ry_net_desc* d) {
    if (!d) return fail(RY_EINVAL, "null descriptor");
    if (d->ndim != 1 && d->ndim != 2) return fail(RY_EINVAL, "ndim must be 1 or 2 (got %d)", d->ndim);
    if (d->in_ch < 1 || d->out_ch < 1 || d->base < 1) return fail(RY_EINVAL, "in_ch/out_ch/base must be positive");
    if (d->extensive_layers < 0 || d->extensive_layers > 8) return fail(RY_EINVAL, "extensive_layers must be in 0..8");
    if (d->ndim == 2 && d->width < 1) return fail(RY_EINVAL, "stage-2 needs width >= 1");
    if (d->ndim == 2 && (d->in_ch != 1 || d->out_ch != 1))
        return fail(RY_EINVAL, "stage-2 (SRPredictor) takes and returns one channel (got %d -> %d)", d->in_ch, d->out_ch);
    if (d->glu != 0 && d->glu != 1) return fail(RY_EINVAL, "glu must be 0 or 1 (got %d)", d->glu);
    if (d->glu && d->ndim != 1) return fail(RY_EINVAL, "glu_generator is a stage-1 option");
    return RY_OK;
}

static const int DECONV_DY[2][2] = {{0, -1}, {1, 0}};  // output parity p, tap t -> input offset
static const int DECONV_KY[2][2] = {{1, 3}, {0, 2}};   // output parity p, tap t -> kernel index

static void fold_scale_shift(const Layer& l, const float* b, const float* bn, float eps,
                             std::vector<float>& scale, std::vector<float>& shift) {
    scale.resize(l.cout); shift.resize(l.cout);
    for (int c = 0; c < l.cout; ++c) {
        if (bn) {
            const double g = bn[c], be = bn[l.cout + c], mu = bn[2 * l.cout + c], var = bn[3 * l.cout + c];
            const double s = g / std::sqrt(var + (double)eps);
            scale[c] = (float)s;
            shift[c] = (float)(((double)(b ? b[c] : 0.f) - mu) * s + be);
        } else {
            scale[c] = 1.f;
            shift[c] = b ? b[c] : 0.f;
        }
    }
}

// stage-1: [Ctot][N][4], taps beyond k zero.  conv W (N, C, k); deconv W (C, N, 4)
static void relayout_1d(const Layer& l, const float* W, std::vector<float>& out) {
    const int C = l.cin(), N = l.cout, K = l.k;
    out.assign((size_t)C * N * 4, 0.f);
    for (int c = 0; c < C; ++c)
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < K; ++k)
                out[((size_t)c * N + n) * 4 + k] = l.deconv ? W[((size_t)c * N + n) * K + k] : W[((size_t)n * C + c) * K + k];
}

// the same taps as [N][Ctot][4] for ry_c1d_os (a lane walks the input channels of one output channel: 16 bytes per lane, coalesced)
static void relayout_1d_os(const Layer& l, const float* W, std::vector<float>& out) {
    const int C = l.cin(), N = l.cout, K = l.k;
    out.assign((size_t)C * N * 4, 0.f);
    for (int c = 0; c < C; ++c)
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < K; ++k)
                out[((size_t)n * C + c) * 4 + k] = l.deconv ? W[((size_t)c * N + n) * K + k] : W[((size_t)n * C + c) * K + k];
}

TapTable make_taps(const Layer& l) {
    TapTable t;
    memset(&t, 0, sizeof t);
    if (l.deconv) {
        t.nphases = 4; t.ntaps = 4;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                const int ph = py * 2 + px;
                t.pdy[ph] = py; t.pdx[ph] = px;
                for (int ty = 0; ty < 2; ++ty)
                    for (int tx = 0; tx < 2; ++tx) {
                        const int tt = ty * 2 + tx;
                        t.dy[ph][tt] = DECONV_DY[py][ty]; t.dx[ph][tt] = DECONV_DY[px][tx];
                        t.ky[ph][tt] = DECONV_KY[py][ty]; t.kx[ph][tt] = DECONV_KY[px][tx];
                    }
            }
    } else {
        t.nphases = 1; t.ntaps = l.k * l.k;
        for (int ky = 0; ky < l.k; ++ky)
            for (int kx = 0; kx < l.k; ++kx) {
                const int tt = ky * l.k + kx;
                t.dy[0][tt] = ky * l.dil; t.dx[0][tt] = kx * l.dil; t.ky[0][tt] = ky; t.kx[0][tt] = kx;
            }
    }
    return t;
}

// stage-2 filters: conv W (N, C, k, k); deconv W (C, N, 4, 4)
static float w2d_at(const Layer& l, const float* W, int n, int c, int ky, int kx) {
    const int C = l.cin(), N = l.cout, K = l.k;
    return l.deconv ? W[(((size_t)c * N + n) * K + ky) * K + kx] : W[(((size_t)n * C + c) * K + ky) * K + kx];
}

// implicit-GEMM filters: [phase][N/64][tap][C/32][64 couts][32 k].  Each (64 x 32) chunk a workgroup stages per K step is
// one contiguous 8 KB block: a wave's 16-byte lane loads cover 1 KB of consecutive addresses, and the rows of a B tile are
// not spread at a power-of-two stride of 4-16 KB (which funnels every workgroup's B traffic into the same L2 channels).
// Stage-2 implicit-GEMM weights: blocks [phase][N/64][tap][Ctot/32] of 64 output channels x 32 input channels, each block
// stored in MFMA FRAGMENT ORDER [n/32 : 2][s : 4][lane : 64][t : 4] with lane = 32 * lh + (n % 32) and k = 8 s + 4 lh + t:
// the 16 bytes lane `lane` feeds to the four v_mfma_f32_32x32x2_f32 of K step s are contiguous, one (n/32, s) piece is
// 1 KiB in lane order -- a wave loads its B fragments straight into registers (or a piece into LDS) fully coalesced.
static size_t wig_inblock(int nl, int k) {
    return (size_t)(nl >> 5) * 1024 + (size_t)(k >> 3) * 256 + (size_t)((((k >> 2) & 1) * 32 + (nl & 31)) * 4) + (size_t)(k & 3);
}

// bf16 blocks of 64 output channels x 64 input channels, same idea: [n/32 : 2][s : 4][lane : 64][j : 8] with
// lane = 32 * lh + (n % 32) and k = 16 s + 8 lh + j (the 8 bf16 a lane feeds to one v_mfma_f32_32x32x16_bf16); index in bf16 units.
static size_t wig16_inblock(int nl, int k) {
    return (size_t)(nl >> 5) * 2048 + (size_t)(k >> 4) * 512 + (size_t)((((k >> 3) & 1) * 32 + (nl & 31)) * 8) + (size_t)(k & 7);
}

static void relayout_igemm(const Layer& l, const float* W, std::vector<float>& out) {
    const TapTable t = make_taps(l);
    const int C = l.cin(), N = l.cout, cpt = C / 32;
    out.resize((size_t)t.nphases * N * t.ntaps * C);
    for (int ph = 0; ph < t.nphases; ++ph)
        for (int n = 0; n < N; ++n)
            for (int tt = 0; tt < t.ntaps; ++tt)
                for (int c = 0; c < C; ++c) {
                    const size_t blk = (((size_t)ph * (N / 64) + n / 64) * t.ntaps + tt) * cpt + c / 32;
                    out[blk * 2048 + wig_inblock(n % 64, c % 32)] = w2d_at(l, W, n, c, t.ky[ph][tt], t.kx[ph][tt]);
                }
}

static void relayout_direct(const Layer& l, const float* W, std::vector<float>& out) {
    const TapTable t = make_taps(l);
    const int C = l.cin(), N = l.cout;
    out.resize((size_t)t.nphases * t.ntaps * C * N);
    for (int ph = 0; ph < t.nphases; ++ph)
        for (int tt = 0; tt < t.ntaps; ++tt)
            for (int c = 0; c < C; ++c)
                for (int n = 0; n < N; ++n)
                    out[(((size_t)ph * t.ntaps + tt) * C + c) * N + n] = w2d_at(l, W, n, c, t.ky[ph][tt], t.kx[ph][tt]);
}

static bool igemm_eligible(const Layer& l) {
    return l.cin_a % 32 == 0 && l.cin_b % 32 == 0 && l.cout % 64 == 0 && l.cin() > 0;
}

// ry_c2d_os filters: [phase][N/4][tap][C/64] blocks of 4 output channels x 64 input channels, one KiB each in the order the lanes load it:
// lane = 4 * ((c % 64) / 4) + n % 4 holds the four consecutive input channels c % 4 = 0..3 of its output channel -- K position
// 4 * (lane / 4) + t of the block for the t-th v_mfma_f32_4x4x1_16B_f32 of the unit.  Consecutive (tap, chunk) units of one channel
// group are consecutive KiB: a wave streams its run of the K axis as one contiguous range.
static bool c2d_os_eligible(const Layer& l) {
    // (rounds of four 64-channel units inside one source; a source's zero pixel is ZTAIL floats)
    return l.cin_a % 256 == 0 && l.cin_b % 256 == 0 && l.cout % 4 == 0 && l.cin() > 0 && l.cin_a <= 2048 && l.cin_b <= 2048;
}

static void relayout_c2d_os(const Layer& l, const float* W, std::vector<float>& out) {
    const TapTable t = make_taps(l);
    const int C = l.cin(), N = l.cout, cpt = C / 64;
    out.resize((size_t)t.nphases * N * t.ntaps * C);
    for (int ph = 0; ph < t.nphases; ++ph)
        for (int n = 0; n < N; ++n)
            for (int tt = 0; tt < t.ntaps; ++tt)
                for (int c = 0; c < C; ++c) {
                    const size_t blk = (((size_t)ph * (N / 4) + n / 4) * t.ntaps + tt) * cpt + c / 64;
                    out[blk * 256 + (size_t)((((c % 64) >> 2) * 4 + (n & 3)) * 4 + (c & 3))] = w2d_at(l, W, n, c, t.ky[ph][tt], t.kx[ph][tt]);
                }
}

// ry_wino_ldsdma filters: a k4 s2 p1 layer is a sum of 2 x 2-tap stride-1 stencils -- one per sub-pixel phase of a transposed convolution
// (taps g[a][b] = W[KY[pdy][1 - a]][KY[pdx][1 - b]] on input offset (pdy - 1 + a, pdx - 1 + b)), one per input parity (r, c) of a convolution
// (g[a][b] = W[2 a + r][2 b + c] on the parity plane) -- and each stencil's F(2x2, 2x2) filters are U = G g G^T, G = [[1, 0], [1, 1], [0, 1]],
// computed in float64 and rounded once.  Layout [phase][N / 64][slice][position i * 3 + j][n / 32 : 2][lane = 32 * lh + n % 32][t : 4] with channel
// 8 * slice' + 4 * lh + t: one (slice, position, 32 channels) piece is the KiB a wave-instruction of the kernel copies, the pieces of a slice and
// consecutive slices are consecutive.  Slices follow the kernel's K loop: deconvolution slice = channel / 8; convolution
// slice = ((channel / 16) * 4 + parity) * 2 + (channel / 8) % 2.  2.25 x the floats of the direct layout (9 positions for 4 taps).
bool wino_eligible(const Layer& l, int ndim) {
    return ndim == 2 && l.k == 4 && l.stride == 2 && l.pad == 1 && l.dil == 1 && l.cin_a % 16 == 0 && l.cin_b % 16 == 0 && l.cout % 64 == 0 &&
           l.cin_a > 0 && l.cin_a <= 2032 && l.cin_b <= 2032;     // (the channel offset of a patch rides on the base of its zero-tail fetches: ZTAIL floats)
}

// wd = the layer's direct layout [phase][tap][C][N] (relayout_direct), which holds every filter element once
static void relayout_wino(const Layer& l, const std::vector<float>& wd, std::vector<float>& out) {
    const TapTable t = make_taps(l);
    const int C = l.cin(), N = l.cout;
    int where[4][4];
    for (int ph = 0; ph < t.nphases; ++ph)
        for (int tt = 0; tt < t.ntaps; ++tt) where[t.ky[ph][tt]][t.kx[ph][tt]] = ph * t.ntaps + tt;
    auto w = [&](int n, int c, int ky, int kx) { return (double)wd[((size_t)where[ky][kx] * C + c) * N + n]; };
    const int nph = l.deconv ? 4 : 1, nsl = l.deconv ? C / 8 : (C / 16) * 8;
    out.assign((size_t)nph * N * nsl * 72, 0.f);
    static const double G[3][2] = {{1, 0}, {1, 1}, {0, 1}};
    for (int ph = 0; ph < nph; ++ph)
        for (int n = 0; n < N; ++n)
            for (int ks = 0; ks < nsl; ++ks)
                for (int cc = 0; cc < 8; ++cc) {
                    int c; double g[2][2];
                    if (l.deconv) {
                        c = ks * 8 + cc;
                        for (int a = 0; a < 2; ++a)
                            for (int b = 0; b < 2; ++b) g[a][b] = w(n, c, DECONV_KY[ph >> 1][1 - a], DECONV_KY[ph & 1][1 - b]);
                    } else {
                        const int par = (ks >> 1) & 3;
                        c = (ks >> 3) * 16 + (ks & 1) * 8 + cc;
                        for (int a = 0; a < 2; ++a)
                            for (int b = 0; b < 2; ++b) g[a][b] = w(n, c, 2 * a + (par >> 1), 2 * b + (par & 1));
                    }
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) {
                            double u = 0.0;
                            for (int a = 0; a < 2; ++a)
                                for (int b = 0; b < 2; ++b) u += G[i][a] * g[a][b] * G[j][b];
                            const size_t piece = ((((size_t)ph * (N / 64) + n / 64) * nsl + ks) * 9 + (i * 3 + j)) * 2 + (n % 64) / 32;
                            out[piece * 256 + (size_t)((32 * (cc >> 2) + n % 32) * 4 + (cc & 3))] = (float)u;
                        }
                }
}

// The Winograd filters of a layer, uploaded into `arena` (2.25 x the floats of its filters): read the direct layout back, transform.  Never called under
// stream capture (plans are built before their first run).
// Filter build mode `device`: one launch on the context stream from the direct layout where it lies -- no download, no host vector, no wait here (a
// predictor's plan waits once for what its layers launched, build_plan; the single operator runs on the same stream).
static int g_filter_build = 0;                         // ry_set_filter_build / RY_FILTER_BUILD: 0 host, 1 device
static int g_poison = 0;                               // RY_POISON (below)
int filter_build_mode() { return g_filter_build; }
int set_filter_build(int mode) {
    if (mode != 0 && mode != 1) return fail(RY_EINVAL, "filter build mode must be 0 (host) or 1 (device), got %d", mode);
    g_filter_build = mode;
    return RY_OK;
}

// floats of one layout of a layer (the sizes the host functions above give their vectors)
size_t filter_layout_floats(const Layer& l, int kind) {
    const TapTable t = make_taps(l);
    const size_t C = (size_t)l.cin(), N = (size_t)l.cout;
    if (kind == RY_LAYOUT_W1D || kind == RY_LAYOUT_W1OS) return C * N * 4;
    if (kind == RY_LAYOUT_WWIN) return (size_t)(l.deconv ? 4 : 1) * N * (l.deconv ? C / 8 : (C / 16) * 8) * 72;
    return (size_t)t.nphases * t.ntaps * C * N;
}

// an upload into the arena, counted (ry_net_build_stats)
static int upload_counted(Arena& arena, ry_ctx* ctx, const std::vector<float>& h, float** d) {
    arena.stats.bytes_uploaded += (unsigned long long)(h.size() * sizeof(float));
    return upload(arena, ctx, h, d);
}
// ... of a layout that a host loop wrote
static int upload_layout(Arena& arena, ry_ctx* ctx, const std::vector<float>& h, float** d) {
    arena.stats.host_relayout_floats += (unsigned long long)h.size();
    return upload_counted(arena, ctx, h, d);
}

// device mode: an allocation of the layout's size in the arena (RY_POISON: NaN patterns first, so a float the kernel leaves out shows), one launch
static int build_layout(ry_ctx* ctx, Arena& arena, const Layer& l, int kind, const float* src, float** out) {
    const size_t n = filter_layout_floats(l, kind);
    RY_TRY(arena.alloc(out, n));
    if (g_poison) RT_TRY(rt::dmemset(*out, 0xFF, n * sizeof(float), ctx->stream));
    RY_TRY(kind == RY_LAYOUT_WWIN ? launch_relayout_wino(ctx, l, src, *out) : launch_relayout(ctx, l, kind, src, *out));
    arena.stats.layout_launches += 1;
    return RY_OK;
}

int upload_wwin(ry_ctx* ctx, Arena& arena, const Layer& l, float** out) {
    if (!l.wdir || !wino_eligible(l, 2)) return fail(RY_ESTATE, "%s: no Winograd form of this layer", l.name);
    if (g_filter_build == 1) return build_layout(ctx, arena, l, RY_LAYOUT_WWIN, l.wdir, out);
    const TapTable t = make_taps(l);
    std::vector<float> wd((size_t)t.nphases * t.ntaps * l.cin() * l.cout), w;
    RT_TRY(rt::d2h(wd.data(), l.wdir, wd.size() * sizeof(float), ctx->stream));
    RT_TRY(rt::stream_sync(ctx->stream));
    arena.stats.bytes_downloaded += (unsigned long long)(wd.size() * sizeof(float));
    relayout_wino(l, wd, w);
    return upload_layout(arena, ctx, w, out);
}

// device mode: the raw filter of a layer in the context's staging buffer (grown when a layer needs more, reused otherwise; the copy is queued behind the
// kernels that read the previous layer's filter).  The caller's array must stay until finish_filter_build has waited.
static int stage_filter(ry_ctx* ctx, Arena& arena, const float* W, size_t n, const float** dev) {
    if (!ctx->stage) ctx->stage.reset(new FilterStage());
    DevBuf<float>& st = ctx->stage->buf;
    RY_TRY(st.reserve(ctx, (long long)n));
    if (g_poison) RY_TRY(st.poison(ctx->stream));
    RT_TRY(rt::h2d(st.ptr(), W, n * sizeof(float), ctx->stream));
    arena.stats.bytes_uploaded += (unsigned long long)(n * sizeof(float));
    *dev = st.ptr();
    return RY_OK;
}

int finish_filter_build(ry_ctx* ctx) {
    if (!ctx->stage) return RY_OK;
    const rt::err_t e = rt::stream_sync(ctx->stream);
    ctx->stage->buf.drop();
    if (e != 0) return fail(RY_EHIP, "waiting for the filter layout kernels failed: %s", rt::err_str(e));
    return RY_OK;
}

// ------------------------------------------------------------------------------------------------
// per-layer launch plans
// ------------------------------------------------------------------------------------------------
// Filters above this size (floats) get the ry_c2d_os layout next to the implicit-GEMM one when a predictor is created: the layers whose time
// is the stream of their filters (SYN-64: encoder c4 .. c7, decoder c0 .. c3, 16.8 - 33.5 MB each).  Whether a plan uses it depends on the
// window (build_plan: few enough output pixels).
static size_t g_os2_min_filter = (size_t)1 << 21;      // RY_OS2_MINW (floats; tests lower it so that small predictors take the path)

int prepare_layer(ry_ctx* ctx, Arena& arena, Layer& l, int ndim, float eps, const float* W, const float* b, const float* bn, bool want_os2) {
    std::vector<float> sc, sh, w;
    fold_scale_shift(l, b, bn, eps, sc, sh);
    // scale/shift padded to a multiple of 4 floats (16-byte epilogue loads)
    sc.resize((sc.size() + 3) / 4 * 4, 1.f); sh.resize((sh.size() + 3) / 4 * 4, 0.f);
    RY_TRY(upload_counted(arena, ctx, sc, &l.scale));
    RY_TRY(upload_counted(arena, ctx, sh, &l.shift));
    if (ndim == 1 && l.k > 4) return fail(RY_EINVAL, "%s: 1-D kernels wider than 4 taps are not supported", l.name);
    if (ndim != 1 && l.k * l.k > 16) return fail(RY_EINVAL, "%s: 2-D kernels larger than 4x4 are not supported", l.name);
    const bool os2 = ndim != 1 && c2d_os_eligible(l) && (want_os2 || (igemm_eligible(l) && (size_t)l.cin() * l.cout * l.k * l.k >= g_os2_min_filter));
    if (g_filter_build == 1) {
        // one upload of the raw filter, then a kernel per layout (relayout_kernels.h): the same allocations in the same order, the same bits
        const float* dW = nullptr;
        RY_TRY(stage_filter(ctx, arena, W, (size_t)l.cin() * l.cout * ipow((size_t)l.k, ndim), &dW));
        if (ndim == 1) {
            RY_TRY(build_layout(ctx, arena, l, RY_LAYOUT_W1D, dW, &l.w1d));
            RY_TRY(build_layout(ctx, arena, l, RY_LAYOUT_W1OS, dW, &l.w1os));
        } else {
            if (igemm_eligible(l)) RY_TRY(build_layout(ctx, arena, l, RY_LAYOUT_WIG, dW, &l.wig));
            if (os2) RY_TRY(build_layout(ctx, arena, l, RY_LAYOUT_W2OS, dW, &l.w2os));
            RY_TRY(build_layout(ctx, arena, l, RY_LAYOUT_WDIR, dW, &l.wdir));
        }
        return RY_OK;
    }
    if (ndim == 1) {
        relayout_1d(l, W, w);
        RY_TRY(upload_layout(arena, ctx, w, &l.w1d));
        relayout_1d_os(l, W, w);
        RY_TRY(upload_layout(arena, ctx, w, &l.w1os));
    } else {
        if (igemm_eligible(l)) { relayout_igemm(l, W, w); RY_TRY(upload_layout(arena, ctx, w, &l.wig)); }
        if (os2) { relayout_c2d_os(l, W, w); RY_TRY(upload_layout(arena, ctx, w, &l.w2os)); }
        relayout_direct(l, W, w);
        RY_TRY(upload_layout(arena, ctx, w, &l.wdir));
    }
    return RY_OK;
}

// RY_POISON=1 (diagnostics): fresh activation buffers, split-K slabs and the outputs of the single operators are filled with NaN patterns, so
// that a kernel that reads a row / pixel its producer never wrote, or a launch that leaves an output element unwritten, shows up as NaN in the
// result instead of depending on what the allocator handed out (g_poison: above, the filter layouts built on the card start the same way)
int poison_fill(ry_ctx* ctx, float* p, size_t nfloats) {
    if (!g_poison || !p || !nfloats) return RY_OK;
    RT_TRY(rt::dmemset(p, 0xFF, nfloats * sizeof(float), ctx->stream));
    RT_TRY(rt::stream_sync(ctx->stream));
    return RY_OK;
}
int alloc_ztail(ry_ctx* ctx, Arena& arena, float** p, size_t nfloats) {
    RY_TRY(arena.alloc(p, nfloats + ZTAIL));
    if (g_poison) RT_TRY(rt::dmemset(*p, 0xFF, nfloats * sizeof(float), ctx->stream));
    RT_TRY(rt::dmemset(*p + nfloats, 0, ZTAIL * sizeof(float), ctx->stream));
    RT_TRY(rt::stream_sync(ctx->stream));
    return RY_OK;
}

void tile_dims(int tile, int* bm, int* bn) {
    switch (tile) {
        case TILE_128x128: *bm = 128; *bn = 128; break;
        case TILE_64x128: *bm = 64; *bn = 128; break;
        case TILE_128x64: *bm = 128; *bn = 64; break;
        case TILE_96x128: *bm = 96; *bn = 128; break;
        default: *bm = 32; *bn = 128; break;
    }
}


// Process-wide switches (INTEGRATION.md section 6 lists every one).  Round 3 removed the A/B switches of closed experiments (register-staged
// kernel, 256-row tiles, burst loads, raster tiles, two-graph cut + stagger, stage-1 tuning aids, ...): their measurements are in DESIGN.md.
static int g_s2_hole = 1;     // RY_S2_HOLE=0: the encoder computes the identical padding rows behind the real frames instead of copying them (A/B, bit-identity tests)
// RY_S2_CROP=0: every decoder layer of the convert wrapper computes all padded rows (A/B of the dead-row crop, used by the bit-identity tests); 1:
// only grids of more than one workgroup per CU
static int g_s2_crop = 2;
// RY_PLAN="layer:tile:splits:kgroups,...", RY_WINO="layer:cfg:mbw:splits,..." and RY_OS2="layer:mt4:nt4:waves:depth,...": tuning aids that fix the
// stage-2 plan of single layers (0 = planner's choice; "layer:0" keeps that layer off the Winograd form / on the implicit GEMM)
static LayerForce g_force[16];
bool layer_plan_fixed(int i) { return g_force[i].fixed(); }
// RY_X3_MINM: split-bf16 mode runs a layer on the bf16 pipe from this many GEMM rows (per phase) up (measured at 300 frames: 1 / 32 / 64 / 128 / 512
// / 2048 -> 0.861 / 0.865 / 0.867 / 0.864 vs 0.840 / 0.928 ms per step on two boxes; 128 beat 512 by 1 % in the same-box A/B)
int g_x3_min_m = 128;
// RY_AUTOTUNE="1[:reps[:max[:pick]]]": time candidate launch plans of every stage-2 implicit-GEMM layer on the device when a plan is built
// (autotune_plan)
int g_autotune = 0;
int g_autotune_reps = 3, g_autotune_max = 0;   // ... timed rounds per candidate; cap on the candidates per layer (0 = all; tests)
int g_autotune_pick = -1;                      // ... (tests only) take candidate `pick` of every layer instead of the fastest
// Kernel names as rocprofv3 prints them (template arguments, no spaces): bench.py matches them against profiles/*.
const char* tile_name(int tile, int kg, bool bf16, int patch) {
    {
        static std::map<int, std::string> names;        // stable storage for the returned pointers
        const int key = ((tile * 4 + kg) * 2 + (bf16 ? 1 : 0)) * 4 + patch;
        auto it = names.find(key);
        if (it == names.end()) {
            int bm, bn; tile_dims(tile, &bm, &bn);
            const int wmv = (tile == TILE_128x128) ? 2 : (tile == TILE_128x64 ? 4 : 1), wnv = 4 / wmv;
            char buf[96];
            snprintf(buf, sizeof buf, "ry_igemm_ldsdma<%d,%d,%d,%d,%d,%s,%d>", bm, bn, wmv, wnv, kg == 2 ? 2 : 1, bf16 ? "true" : "false", patch);
            it = names.emplace(key, buf).first;
        }
        return it->second.c_str();
    }
}

// ---- choice of tile, split-K and K groups for one stage-2 layer ----
// Workgroups of one tile that fit a CU.  LDS-DMA kernel: two unpadded BK = 32 buffers; register-staged kernel: one padded
// buffer, limited to 3 by its VGPR budget.
static thread_local double g_plan_peak = 157.3e6;   // flop per microsecond the planner prices the main loop at (fp32 MFMA peak; bf16: see choose_igemm)
static thread_local int g_plan_ck = 32;             // input channels per K chunk of the kernel being planned
// split-bf16 kernels (measured, profiles/r01/n_x3_plansweep_n300.txt): the main-loop rate the planner prices them at (three times
// the K of the bf16 mode per tile: the fixed costs weigh less, 128x128 tiles reach 730-800 TF of bf16 products = 0.7 x 1150),
// and the price of two K groups in one 512-thread workgroup against two 256-thread workgroups on the same CU (the GEMM alone
// ran 10-17 % slower: 69 vs 59 us on decoder c3, 73 vs 66 us on encoder c1).
static const double g_x3_peak = 2.0e9, g_x3_kg2 = 1.15;
static thread_local double g_plan_kg2 = 1.0;        // factor on the main loop of a two-K-group workgroup

int tile_occ(int tile, int kg) {
    int bm, bn; tile_dims(tile, &bm, &bn);
    const int occ = (160 * 1024) / (kg * (bm + bn) * 32 * 4 * 2 + bm * 16);
    const int cap = 4 / kg;                                              // <= 128 VGPRs: four waves per SIMD
    return occ > cap ? cap : occ;
}

// Fraction of the MFMA peak a CU sustains with r co-resident four-wave groups running the main loop (measured on gfx950:
// a lone group cannot cover its own barriers and LDS latency).
static double cu_rate(int r) {
    static const double f[5] = {0.0, 0.36, 0.70, 0.72, 0.72};
    return f[r > 4 ? 4 : r];
}

// Estimated time (microseconds) of one layer: `blocks` output tiles of bm rows, each split over s workgroups of kg
// four-wave K groups, on 256 CUs that hold occ workgroups at a time.  The busiest CU sets the main-loop time (a partial
// last round runs at the rate of its fewer resident groups); external split-K adds the slab traffic and a reduce launch.
double est_time(long blocks, int bm, int bn, int s, int occ, int kg, int M, int N, int nk) {
    const long g = blocks * s;
    const long per_cu = (g + 255) / 256;
    const long full = per_cu / occ, rem = per_cu % occ;
    const double tile_us = 2.0 * bm * bn * ((double)g_plan_ck * nk) / (g_plan_peak / 256.0);   // one tile on one CU at the peak (157.3 TFLOP/s over 256 CUs)
    const double w = tile_us / (double)(s * kg);                              // work of one four-wave group
    double t = (double)full * occ * kg * w / cu_rate(occ * kg) + (rem ? (double)rem * kg * w / cu_rate((int)rem * kg) : 0.0);
    if (kg > 1) t *= g_plan_kg2;
    t += 4.0 + (double)M * N * 4.0 / 5.0e6;                                     // launch + ramp, output stores at ~5 TB/s (exposed: one round)
    if (s > 1) t += 5.0 + (2.0 * s) * M * N * 4.0 / 4.0e6;                     // s slab writes + s slab reads at ~4 TB/s, reduce launch
    if (kg > 1) t += 1.0;                                                       // in-LDS sum, half of the waves idle in the epilogue
    return t;
}

static int best_split(long blocks, int bm, int bn, int nk, bool tinyM, int occ, int kg, int M, int N, double* t_out) {
    const int smax = tinyM ? 128 : 32, min_chunks = (tinyM ? 2 : 4) * kg;
    int best = 1; double bt = 1e30;
    for (int s = 1; s <= smax && s <= (nk >= min_chunks ? nk / min_chunks : 1); ++s) {
        double t;
        // weight streaming: two workgroups per CU keep enough loads in flight (1024 measured 30 % slower: more slabs, same bandwidth)
        if (tinyM) { const long g = blocks * s; t = g >= 512 ? 1.0 + 1e-4 * s : 512.0 / (double)g; }
        else t = est_time(blocks, bm, bn, s, occ, kg, M, N, nk);
        if (t < bt - 1e-9) { bt = t; best = s; }
    }
    if (t_out) *t_out = bt;
    return best;
}


void choose_igemm(const Layer& l, int M, int nphases, int nk, int* tile, int* splits, int* kg, int bf16) {
    const bool kg_auto = *kg == 0, splits_auto = *splits == 0;
    // bf16: 64 channels per chunk; the kernel is bound by the operand movement, not the matrix pipe: price
    // the main loop at the measured rate so that the fixed costs (launch, stores, slabs) weigh as they do in the measurements
    g_plan_peak = bf16 == 2 ? g_x3_peak : bf16 ? 0.86e9 : 157.3e6; g_plan_ck = bf16 ? 64 : 32;   // 128x128 bf16 tiles measured ~620 TF = 0.72 x 860
    g_plan_kg2 = bf16 == 2 ? g_x3_kg2 : 1.0;
    // MFMA-bound layers: every CU should hold a full set of co-resident wave groups for the whole launch.  Candidate
    // M-tiles 128 / 96 / 64 (N-tile 128), with one or two K groups per workgroup and the best external split-K, are
    // compared by estimated time.
    const bool kg_ok = M > 64 && nk >= 16;
    const int N = l.cout;
    if (*tile == 0) {
        if (N % 128 != 0) *tile = TILE_128x64;                         // (128x64 measured 94 TF vs 79 TF for the old 256x64 tile)
        else if (M <= 32) *tile = TILE_32x128;
        else if (M <= 64) *tile = TILE_64x128;
        else {
            const int cand[3] = {TILE_128x128, TILE_96x128, TILE_64x128};
            const double bias[3] = {1.0, 1.02, 1.08};                     // smaller tiles re-read more B per flop
            double bt = 1e30; int btile = TILE_128x128, bk = 1;
            for (int c = 0; c < 3; ++c)
                for (int k = 1; k <= ((kg_ok && *kg == 0) ? 2 : 1); ++k) {
                    const int kk = *kg > 0 ? *kg : k;
                    int bm, bn; tile_dims(cand[c], &bm, &bn);
                    const long mt = (M + bm - 1) / bm;
                    double t = 0.0;
                    best_split(mt * (N / bn) * nphases, bm, bn, nk, false, tile_occ(cand[c], kk), kk, M, N, &t);
                    // fp32: smaller tiles re-read more B per flop; bf16: the kernel is bound by the operand movement, time
                    // scales with operand bytes per flop, (1/BM + 1/BN)
                    t *= bf16 ? (1.0 / bm + 1.0 / bn) * 64.0 : bias[c];
                    if (t < bt - 1e-9) { bt = t; btile = cand[c]; bk = kk; }
                }
            *tile = btile;
            if (*kg == 0) *kg = bk;
        }
    }
    int bm, bn; tile_dims(*tile, &bm, &bn);
    const long blocks = (long)((M + bm - 1) / bm) * (N / bn) * nphases;
    if (*kg == 0) {
        *kg = 1;
        if (kg_ok && bm <= 128 && *splits == 0) {
            double t1 = 0.0, t2 = 0.0;
            best_split(blocks, bm, bn, nk, false, tile_occ(*tile, 1), 1, M, N, &t1);
            best_split(blocks, bm, bn, nk, false, tile_occ(*tile, 2), 2, M, N, &t2);
            if (t2 < t1 - 1e-9) *kg = 2;
        }
    }
    if (*splits == 0) *splits = best_split(blocks, bm, bn, nk, M <= 64, tile_occ(*tile, *kg), *kg, M, N, nullptr);
    // Two K groups in one workgroup (8 waves, 125 KiB of LDS: nothing else fits beside it on a CU) exist to save slabs and reduce work.  Where the plan
    // needs an external split anyway and the external-split-only form (four-wave workgroups of 62 KiB: two of ANY two launches share a CU, which is what
    // the window on the other lane needs) is estimated within one per cent, take that form: a tie alone, and measured under two lanes (round 5,
    // profiles/r05/r_plan_ab_n300.txt) decoder c3 -- the one layer this selects at 300 frames -- moves the step 1.1015 -> 1.0767 ms per window and ends
    // the bimodal phase lock of the lanes; encoder c4 / c5 and decoder c2 (4 - 12 % apart by the estimate) gain nothing and stay.
    if (kg_auto && splits_auto && bf16 == 0 && *kg == 2 && *splits > 1 && M > 64) {
        double t1 = 0.0;
        const int s1 = best_split(blocks, bm, bn, nk, false, tile_occ(*tile, 1), 1, M, N, &t1);
        const double t2 = est_time(blocks, bm, bn, *splits, tile_occ(*tile, 2), 2, M, N, nk);
        if (t1 <= 1.01 * t2) { *kg = 1; *splits = s1; }
    }
    if (*splits * *kg > nk) { *kg = 1; if (*splits > nk) *splits = nk; }
}

static bool os2_has_config(int mt4, int nt4, int waves, int depth) {
#define X(A, B, C, D) if (mt4 == A && nt4 == B && waves == C && depth == D) return true;
    RY_OS2_CONFIGS(X)
#undef X
    return false;
}

// RY_OS2_MAXCOST: a layer with the ry_c2d_os filter layout runs output-stationary when slice cost x K units stays below this (0: never).
// Fitted: encoder c6 / decoder c1 at 300 frames (4096) win by 2-4 us, encoder c5 at 300 frames (10240) and
// decoder c2 at 100 frames (8192) lose by 8-11
static int g_os2_maxcost = 4608;

// Slice of one layer, by a cost fitted to the slice sweeps on the MI355X (profiles/r05/e_os_sweep_n{300,100}.txt): a workgroup pulls K x (rows +
// channels) of its tile through its CU's L1, the pixel rows at about half the rate of the filter rows (a wave-load of pixels is four
// 256-byte pieces of four different pixels, a wave-load of filters one contiguous KiB), and the launch takes as many rounds as there are
// workgroups per CU.  cost = max(1, workgroups / 256) x (2 rows + channels) of the tile (1.5 rows where the pixels travel by DMA); the sweeps rank
// the slices of every bottom layer in this
// order (encoder c7: 4 x 8 < 8 x 4 < 4 x 4 < 12 x 4; decoder c1: 24 x 16 < 12 x 16 < 8 x 16 < 16 x 16).  `cost_out` x K units is what the
// caller compares with the implicit GEMM (g_os2_maxcost).
bool choose_os2(int M, int N, int nphases, int U, int* mt4, int* nt4, int* waves, int* depth, double* cost_out) {
    static const int MTS[5] = {1, 2, 3, 4, 6}, NTS[3] = {1, 2, 4};
    double best = 1e30; int bm = 0, bn = 0, bw = 0, bd = 0;
    for (int mi = 0; mi < 5; ++mi)
        for (int ni = 0; ni < 3; ++ni) {
            const int m = MTS[mi], n = NTS[ni];
            if ((*mt4 != 0 && *mt4 != m) || (*nt4 != 0 && *nt4 != n) || N % (4 * n) != 0) continue;
            // waves x units in flight: large tiles run four waves with four units in flight, small ones eight waves with two (more waves hide more of
            // the chain request -> landing -> MFMA at one or two workgroups per CU); whatever the run of K units feeds with whole rounds of four
            int w = 0, d = 0;
            static const int WD[4][2] = {{8, 2}, {4, 4}, {16, 2}, {8, 4}}, WD_BIG[4][2] = {{4, 4}, {8, 2}, {4, 2}, {8, 4}};
            const bool big = m * n >= 12 && !os2_xl_ok(m, 8, 2);        // (a large tile whose pixels go through the LDS keeps eight waves)
            for (int k = 0; k < 4 && w == 0; ++k) {
                const int cw = (big ? WD_BIG : WD)[k][0], cd = (big ? WD_BIG : WD)[k][1];
                if ((*waves != 0 && *waves != cw) || (*depth != 0 && *depth != cd) || U % (4 * cw) != 0 || !os2_has_config(m, n, cw, cd)) continue;
                w = cw; d = cd;
            }
            // a forced pair outside the preference lists (only one of the two forced and no preferred pair fits: no plan)
            if (w == 0 && *waves != 0 && *depth != 0)
                if (U % (4 * *waves) == 0 && os2_has_config(m, n, *waves, *depth)) { w = *waves; d = *depth; }
            if (w == 0) continue;
            const double wgs = (double)((M + 4 * m - 1) / (4 * m)) * (N / (4 * n)) * nphases;
            // pixel rows by DMA through the LDS: contiguous 256-byte pieces (encoder c6: 12 x 8 ahead of 8 x 16)
            const double px = os2_xl_ok(m, w, d) ? 6.0 : 8.0;
            // padded rows are loaded too
            const double cost = (wgs > 256.0 ? wgs / 256.0 : 1.0) * (px * m + 4.0 * n) * ((double)((M + 4 * m - 1) / (4 * m)) * 4 * m / M);
            if (cost < best - 1e-9) { best = cost; bm = m; bn = n; bw = w; bd = d; }
        }
    if (bm == 0) return false;
    *mt4 = bm; *nt4 = bn; *waves = bw; *depth = bd;
    if (cost_out) *cost_out = best;
    return true;
}

// ---- stage-2 layers in Winograd F(2x2, 2x2) form (ry_wino_ldsdma) ----
// Workgroup shapes: cfg 1 = 2 x 2 waves (two M-blocks of 8 x 16 pixels x 64 channels, one 8-channel slice per iteration, 74 KiB of LDS: two per CU),
// cfg 2 = 4 x 2 waves (four M-blocks x 64 channels, two slices per iteration, 146 KiB: one per CU).  mbw = M-blocks per tile row.
static int g_wino = 1;                 // RY_WINOGRAD=0: every layer keeps the direct implicit GEMM (the bit-exact reference of the Winograd form; A/B)
// RY_WINO_MINM: rows (pixels of one phase) from which an eligible layer takes the Winograd form (512 -> 256: encoder c4 / decoder c3 of the 100-frame
// window, 231.8 -> 240.9 k frames/s)
static int g_wino_min_m = 256;

bool wino_cfg_dims(int cfg, int* wm, int* wn, int* nsl) {
    if (cfg == 1) { *wm = 2; *wn = 2; *nsl = 1; return true; }
    if (cfg == 2) { *wm = 4; *wn = 2; *nsl = 2; return true; }
    return false;
}
void wino_tile_hw(int cfg, int mbw, int* th, int* tw) {              // pixels of the stencil's output grid per M-tile
    int wm = 2, wn = 2, nsl = 1; wino_cfg_dims(cfg, &wm, &wn, &nsl);
    *th = 8 * (wm / mbw); *tw = 16 * mbw;
}
const char* wino_name(int cfg, int mode) {
    static char buf[4][40];
    char* b = buf[(cfg - 1) * 2 + (mode - 1)];
    int wm = 2, wn = 2, nsl = 1; wino_cfg_dims(cfg, &wm, &wn, &nsl);
    snprintf(b, 40, "ry_wino_ldsdma<%d,%d,%d,%d>", wm, wn, nsl, mode);      // as rocprofv3 prints it
    return b;
}

// Plan of one layer: workgroup shape, tile shape (the squarest one that divides the grid: the patch carries one extra row and column), external split-K.
// Returns false when no tile shape divides the Mh x Mw grid.
bool choose_wino(int Mh, int Mw, int N, int nphases, int npatches, int B, int* cfg, int* mbw, int* splits) {
    double best = 1e30; int bc = 0, bm = 0, bs = 0;
    for (int c = 1; c <= 2; ++c) {
        if (*cfg != 0 && *cfg != c) continue;
        int wm, wn, nsl; wino_cfg_dims(c, &wm, &wn, &nsl);
        for (int m = 1; m <= wm; m *= 2) {
            if (*mbw != 0 && *mbw != m) continue;
            int th, tw; wino_tile_hw(c, m, &th, &tw);
            if (Mh % th || Mw % tw) continue;
            const long units = (long)B * (Mh / th) * (Mw / tw) * (N / 64) * nphases;
            const int slots = c == 1 ? 512 : 256;
            // short tiles: the dead-row crop and the copied padding rows round to whole tile rows (8 x 32 against 16 x 16 tiles, two-lane step at 300
            // frames: encoder -1.1 %, decoder -2.8 %, profiles/r06/plan_ab_mbw.txt)
            const double halo = (double)(th + 1) * (tw + 1) / ((double)th * tw) + 0.006 * th;
            for (int sp = 1; sp <= 32 && sp <= npatches; ++sp) {
                if (*splits != 0 ? *splits != sp : (sp > 1 && sp > npatches / 2)) continue;      // (the planner's own splits leave two patches per workgroup)
                // rounds of workgroups x iterations of the longest split (+ prologue / epilogue of a workgroup, in iterations) x time of an iteration
                // relative to
                // cfg 1 (cfg 2 runs twice the slices on twice the rows per slot), + the slab traffic and the reduce node of an external split
                const long rounds = (units * sp + slots - 1) / slots;
                const double its = (double)((npatches + sp - 1) / sp) * 2.0;          // 8-channel slices
                double t = (double)rounds * (its + 6.0) * (c == 1 ? 1.0 : 2.0) * (0.9 + 0.1 * halo);
                if (sp > 1) t += 8.0 + 0.02 * sp * (double)B * Mh * Mw * nphases * N / 65536.0;
                if (t < best - 1e-9) { best = t; bc = c; bm = m; bs = sp; }
            }
        }
    }
    if (bc == 0) return false;
    *cfg = bc; *mbw = bm; *splits = bs;
    return true;
}

// split heuristic of the weight-streaming stage-1 kernels (128 / 16 measured 0.275 ms, 256 / 32 0.231 ms, 512 / 64 0.238 ms per forward)
static const int g_s1_wgs = 256, g_s1_maxs = 32;

int c1d_mode(const Layer& l) {
    if (l.deconv) return RY_C1D_DECONV;
    if (l.k == 4 && l.stride == 2 && l.pad == 1 && l.dil == 1) return RY_C1D_S2;
    if (l.stride == 1 && l.dil == 1 && l.pad <= 3) return RY_C1D_S1;
    return RY_C1D_GEN;
}

int c1d_tile_len(int mode) { return mode == RY_C1D_DECONV ? 8 : 16; }

int choose_splits_1d(const Layer& l, int B, int rows, int mode) {
    // weight streaming wants many workgroups, but every split is re-summed by each consumer tile: aim for
    // ~256 workgroups, at most 32 splits, at least 16 input channels per split
    const int TL = c1d_tile_len(mode);
    const int cogroups = (l.cout + 63) / 64;
    const long wgs = (long)((cogroups + 3) / 4) * ((rows + TL - 1) / TL) * B;
    int s = (int)((g_s1_wgs + wgs - 1) / wgs);
    const int maxs = l.cin() / 16 > 0 ? l.cin() / 16 : 1;
    if (s > maxs) s = maxs;
    if (s > g_s1_maxs) s = g_s1_maxs;
    if (s < 1) s = 1;
    return s;
}


// ---- stage-1, output-stationary form (ry_c1d_os) ----
// smallest workgroup count a layer should reach before it takes a larger slice per workgroup (128 / 256 / 512 / 1024 measured 0.119 / 0.116 / 0.112 /
// 0.116 ms)
static const int g_s1_units = 256;

bool c1d_os_capable(const Layer& l) {
    const int mode = c1d_mode(l);
    return mode != RY_C1D_GEN && l.act != RY_ACT_GLU && l.k <= 4;
}

static int c1d_os_ktw(int ctot) { return ctot <= 64 ? 1 : ctot <= 128 ? 2 : 4; }

// slice (cb output channels x tp rows per position group) of one layer: the largest one that still gives g_s1_units workgroups
static void choose_os(const Layer& l, int B, int rows, int* cb, int* tp) {
    const bool dec = l.deconv;
    static const int CF[4][2] = {{4, 8}, {4, 4}, {2, 8}, {2, 4}};
    const int PG = 4 / c1d_os_ktw(l.cin());
    int best = -1; long best_units = -1; double best_waste = 1e30;
    for (int c = 0; c < 4; ++c) {
        const int b_ = CF[c][0], t_ = CF[c][1];
        if (dec && b_ * t_ * 2 > 32) continue;                                    // 2 tp outputs per input row
        const long tiles = (rows + PG * t_ - 1) / (PG * t_);
        const long units = (long)((l.cout + b_ - 1) / b_) * B * tiles;
        const double waste = (double)tiles * PG * t_ / rows * ((l.cout + b_ - 1) / b_ * b_) / (double)l.cout;
        if (units >= g_s1_units && waste <= 1.34) { best = c; break; }             // candidates are ordered by decreasing slice
        if (units > best_units || (units == best_units && waste < best_waste)) { best = c; best_units = units; best_waste = waste; }
    }
    *cb = CF[best][0]; *tp = CF[best][1];
}

// the launch shape of one stage-1 layer in output-stationary form (Wi / Wo set), for predictors (build_plan) and the single operator (ry_conv1d_os)
void plan_s1_os(const Layer& l, LayerPlan& lp, int B) {
    lp.os_kt = c1d_os_ktw(l.cin());
    choose_os(l, B, l.deconv ? lp.Wi : lp.Wo, &lp.os_cb, &lp.os_tp);
    // sources split inside a wave: the per-lane form exists for this slice only
    if (l.cin_b > 0 && l.cin_a % 64 != 0) { lp.os_cb = 2; lp.os_tp = 4; }
}

// The Winograd filters of predictor layer i, built when a plan first takes the layer onto that path and kept in the arena the clones of the predictor share
static int ensure_wwin(ry_net* net, int i, const float** out) {
    auto& lazy = net->weights->lazy;
    auto it = lazy.find(i);
    if (it == lazy.end()) {
        float* d = nullptr;
        RY_TRY(upload_wwin(net->ctx, *net->weights, net->layers[i], &d));
        it = lazy.emplace(i, d).first;
        if (g_filter_build == 1) net->weights->lazy_pending = true;       // launched on the context stream, not waited for
    }
    *out = it->second;
    return RY_OK;
}

// Layouts in `lazy` that were launched and not waited for: the predictor streams (this handle's and its clones') do not follow the context stream, so
// whoever is about to hand such a layout to them waits once -- a launch plan after its layer loop, however many layers it built
static int wait_lazy(ry_net* net) {
    if (!net->weights->lazy_pending) return RY_OK;
    RT_TRY(rt::stream_sync(net->ctx->stream));
    net->weights->lazy_pending = false;
    return RY_OK;
}

int net_wwin(ry_net* net, int layer, const float** out) {
    RY_TRY(ensure_wwin(net, layer, out));
    return wait_lazy(net);
}

// The 2-D pixel tiles a stage-2 GEMM layer's launch walks over its Mh x Mw grid: th rows x tw columns (the launchers take them from here; the
// dead-row crop and the copied padding rows round to whole tile rows); false: raster tiles (the implicit GEMM) / no Winograd tile fits
bool plan_tile_rows(const LayerPlan& lp, int Mh, int Mw, int* th, int* tw_out) {
    if (lp.path == PATH_WINO) {
        int tw; wino_tile_hw(lp.wino_cfg, lp.wino_mbw, th, &tw);
        if (tw_out) *tw_out = tw;
        return Mh % *th == 0 && Mw % tw == 0;
    }
    int bm, bn; tile_dims(lp.tile, &bm, &bn);
    for (int tw = 16; tw >= 4; tw >>= 1)
        if (bm % tw == 0 && Mw % tw == 0 && Mh % (bm / tw) == 0) { *th = bm / tw; if (tw_out) *tw_out = tw; return true; }
    return false;
}

// May the launch of this layer leave output rows [lo, lo + n) out of its grid (ry_rep_rows fills them with copies of row lo - 1)?  Whole tile
// rows of a convolution launched whole (no crop), 16-byte rows for the copy; the implicit GEMM: 16-pixel-wide tiles and no external split (the
// Winograd launch runs its reduce before the copies).  The planner picks holes by this rule (enqueue_forward), the launchers assert it.
bool plan_hole_ok(const Layer& l, const LayerPlan& lp, int lo, int n) {
    const bool igemm = lp.path == PATH_IGEMM || lp.path == PATH_IGEMM_BF16;
    if ((!igemm && lp.path != PATH_WINO) || (igemm && lp.splits != 1) || l.deconv || lp.crop_hi > 0 || (lp.Wo * l.cout) % 8) return false;
    int th = 1, tw = 0;
    if (!plan_tile_rows(lp, lp.Ho, lp.Wo, &th, &tw) || (igemm && tw != 16)) return false;
    return n > 0 && lo >= 1 && lo % th == 0 && n % th == 0 && lo + n <= lp.Ho;
}

WindowRows plan_window_rows(const ry_net* net, const Plan& P) {
    const int nd = net->desc.ndim, B = P.B;
    WindowRows w;
    // Stage 2, convert wrapper: the wrapper pads every window to T rows and keeps n_frames of the result (SuperResolution.convert crops);
    // a caller that will itself throw away the first / last frames of the window (ConvertStream.process picks the middle of what it
    // converted) can say so (ry_sr_convert_rows).  The last layer then computes output rows [k0, k1) only, reads rows [k0 - 1, k1 + 1) of
    // decoder c6, and nothing ever reads the other rows.  Walking back through the decoder: correct output rows [a, b) of a k4 s2 p1
    // deconvolution need input rows [floor((a - 1) / 2), floor(b / 2) + 1) (output row 2m takes input rows m - 1 and m, row 2m + 1 rows m
    // and m + 1).  Rows are the outermost axis of the NHWC buffers, so a layer simply runs on a row RANGE of the same buffers
    // (LayerPlan::crop_lo / crop_hi; the rows next to the range read as zero padding, which only reaches rows that are not needed).
    // Every layer demands from its producer exactly the (tile-rounded) rows it reads.  The encoder feeds the bottom of the U-Net and stays whole.
    w.k1 = P.n_frames;
    if (nd == 2 && P.mode == 1 && P.lp[15].path == PATH_LAST) {
        keep_rows(P.n_frames, P.disc_front, P.disc_back, &w.k0, &w.k1);
    }
    if (nd == 2 && P.mode == 1 && g_s2_crop && P.lp[15].path == PATH_LAST && net->layers[15].src_a == 14) {
        int need0 = w.k0 > 0 ? w.k0 - 1 : 0, need1 = w.k1 + 1;         // correct rows [need0, need1) wanted from layer i's output
        for (int i = 14; i >= 8; --i) {
            const Layer& l = net->layers[i];
            const LayerPlan& lp = P.lp[i];
            if (need1 > lp.Ho) need1 = lp.Ho;
            if (need0 <= 0 && need1 >= lp.Ho) break;
            if (lp.path != PATH_IGEMM && lp.path != PATH_IGEMM_BF16 && lp.path != PATH_WINO) break;
            if (l.src_a != i - 1) break;
            int r0, r1;
            if (l.deconv) { r0 = need0 > 0 ? (need0 - 1) / 2 : 0; r1 = need1 / 2 + 1; }
            else if (l.k == 1 && l.stride == 1) { r0 = need0; r1 = need1; }
            else break;
            const int Mw = l.deconv ? lp.Wi : lp.Wo, Mh = l.deconv ? lp.Hi : lp.Ho;
            int th = 1;
            // keep the 2-D pixel tiles of the launch: whole tile rows
            if (plan_tile_rows(lp, Mh, Mw, &th)) { r0 = r0 / th * th; r1 = (r1 + th - 1) / th * th; }
            if (r1 > lp.Hi) r1 = lp.Hi;
            if (r0 <= 0 && r1 >= lp.Hi) break;
            // measured at 300 frames (round 2, interleaved A/B on one box): decoder c6 (1536 -> 1216 workgroups, six per CU -> five) 208 -> 177 us, decoder c5
            // (512 -> 416, two per CU) 198 -> 193 us, decoder c4 (256 -> 224, one per CU) 196 -> 194 us: a grid of one workgroup per CU
            // gains nothing by itself, but the CUs it leaves idle go to the window on the other lane (ry_vc_set_lanes): 1.160 -> 1.137 ms
            // per window with two lanes, so it is cropped too (RY_S2_CROP=1 keeps such grids whole)
            int bm = 256, bn = 64;
            if (lp.path == PATH_WINO) { if (lp.wino_cfg == 2) bm = 512; } else tile_dims(lp.tile, &bm, &bn);
            const long wgs = (long)(((long)B * Mh * Mw + bm - 1) / bm) * (l.cout / bn) * (l.deconv ? 4 : 1) * lp.splits;
            if (g_s2_crop >= 2 || wgs > 256) { w.crop_lo[i] = r0; w.crop_hi[i] = r1 - r0; need0 = r0; need1 = r1; }
            else { need0 = 0; need1 = lp.Hi; }                      // this layer runs whole: it reads every row of its producer
        }
    }
    // Stage 2, convert wrapper: rows n_frames .. T - 1 of the padded window are copies of ONE row (the column minima, ry_pad_min_rows), so down the
    // encoder every layer has a stretch of output rows that are equal bit for bit (same operands, same order): identical input rows [a, b] give
    // identical output rows [ceil((a + pad) / stride), floor((b - (k - 1) dil + pad) / stride)] -- at 300 of 384 frames 40 of 192 rows of encoder c1,
    // 19 of 96 of c2.  The implicit GEMM leaves the whole tile rows inside the stretch out of its grid and ry_rep_rows copies the row above them:
    // the MFMA time of those tiles goes to the window on the other lane (RY_S2_HOLE=0 computes them; results are bit-identical either way).
    if (nd == 2 && P.mode == 1 && g_s2_hole && P.n_frames < P.T - 2) {
        int a = P.n_frames, b = P.T - 1;
        for (int i = 0; i < 8; ++i) {
            const Layer& l = net->layers[i];
            const LayerPlan& lp = P.lp[i];
            if (l.deconv || l.src_b >= 0 || l.src_a != i - 1) break;
            const int top = b - (l.k - 1) * l.dil + l.pad;
            if (top < 0) break;
            a = (a + l.pad + l.stride - 1) / l.stride; b = top / l.stride;
            if (b >= lp.Ho) b = lp.Ho - 1;
            if (b - a < 1) break;
            int th = 1;
            if (!plan_tile_rows(lp, lp.Ho, lp.Wo, &th)) continue;
            const int r0 = (a + 1 + th - 1) / th * th, r1 = (b + 1) / th * th;      // rows [r0, r1) are whole tile rows and copies of row r0 - 1 >= a
            if (r1 - r0 >= th && plan_hole_ok(l, lp, r0, r1 - r0)) { w.hole_lo[i] = r0; w.hole_n[i] = r1 - r0; }
        }
    }
    return w;
}

// ------------------------------------------------------------------------------------------------
// plan construction
// ------------------------------------------------------------------------------------------------
// The launch plan of one stage-2 layer whose geometry lp holds: path, tile, split-K and K groups, the Winograd / output-stationary shape, the fused end
// of PATH_LAST (out_layer: the predictor's last layer; mode: the plan's), and the split-K slabs in `arena`.  src16: every producer writes a bf16 copy
// of its output.  f: the layer's override record; a path it names (the single operator) runs as it is -- the process-wide switches, the producer
// rule and the row minima of the Winograd / split-bf16 forms do not apply to it.
int plan_s2_layer(ry_ctx* ctx, Arena& arena, const Layer& l, LayerPlan& lp, int B, int dtype, const LayerForce& f, bool src16, bool out_layer, int mode) {
    const TapTable t = make_taps(l);
    const int M = B * (l.deconv ? lp.Hi * lp.Wi : lp.Ho * lp.Wo);
    const bool x3 = dtype == 2;
    if (f.path ? f.path == PATH_IGEMM || f.path == PATH_IGEMM_BF16 || f.path == PATH_IGEMM_X3 : l.wig != nullptr) {
        lp.path = PATH_IGEMM; lp.tile = f.tile; lp.splits = f.splits; lp.kg = f.kg;
        if (lp.tile != 0) {                                  // RY_PLAN: refuse a tile that does not divide the output channels
            int fbm, fbn; tile_dims(lp.tile, &fbm, &fbn);
            if (l.cout % fbn != 0) return fail(RY_EINVAL, "RY_PLAN: tile %dx%d does not divide the %d output channels of %s", fbm, fbn, l.cout, l.name);
            if (dtype != 0 && fbm > 128) return fail(RY_EINVAL, "RY_PLAN: no bf16 instantiation of the %dx%d tile (%s)", fbm, fbn, l.name);
        }
        // bf16 mode: a layer runs on bf16 operands when its filters were converted and every producer it reads can
        // write a bf16 copy of its output (the first layer, implicit-GEMM layers and their reduce kernels can)
        // split-bf16 mode: the same, for the layers with enough rows to be bound by the matrix pipe (the weight-streaming
        // layers at the bottom of the U-Net would read 1.5 x the filter bytes: they stay exact fp32)
        const bool want16 = f.path ? f.path != PATH_IGEMM : src16 && (x3 ? (l.wigx3 && M >= g_x3_min_m) : (dtype == 1 && l.wig16));
        if (want16) {
            lp.path = PATH_IGEMM_BF16; lp.x3 = x3;
            choose_igemm(l, M, t.nphases, t.ntaps * ((x3 ? 3 : 1) * l.cin() / 64), &lp.tile, &lp.splits, &lp.kg, x3 ? 2 : 1);
        } else {
            choose_igemm(l, M, t.nphases, t.ntaps * (l.cin() / 32), &lp.tile, &lp.splits, &lp.kg);
        }
    }
    // the weight-streaming layers with few rows: output-stationary, one node, no slabs (ry_c2d_os) -- exact fp32 layers only
    if (f.path ? f.path == PATH_OS2D : lp.path == PATH_IGEMM && l.w2os && !(f.os2_set && f.os2[0] == 0)) {
        int c[4] = {f.os2[0], f.os2[1], f.os2[2], f.os2[3]};
        const int U = t.ntaps * (l.cin() / 64);
        double cost = 0.0;
        if (choose_os2(M, l.cout, t.nphases, U, &c[0], &c[1], &c[2], &c[3], &cost) && (f.os2_set || cost * U <= (double)g_os2_maxcost)) {
            lp.path = PATH_OS2D; lp.splits = 1; lp.kg = 1;
            lp.os2_mt4 = c[0]; lp.os2_nt4 = c[1]; lp.os2_waves = c[2]; lp.os2_depth = c[3];
        } else if (f.os2_set) {
            if (f.path) return fail(RY_EINVAL, "no output-stationary slice %d:%d:%d:%d for this shape", c[0], c[1], c[2], c[3]);
            return fail(RY_EINVAL, "RY_OS2: no output-stationary slice %d:%d:%d:%d for %s", c[0], c[1], c[2], c[3], l.name);
        }
    }
    // the MFMA-bound k4 s2 p1 layers: Winograd F(2x2, 2x2), 9 / 16 of the matrix-pipe work -- exact-fp32 mode only (RY_WINOGRAD=0: the
    // direct kernels, bit-exact reference; a layer whose direct plan RY_PLAN fixes stays direct)
    if (f.path ? f.path == PATH_WINO
               : lp.path == PATH_IGEMM && dtype == 0 && g_wino && wino_eligible(l, 2) && !(f.wino_set && f.wino[0] == 0) && !f.fixed()) {
        const int Mh = l.deconv ? lp.Hi : lp.Ho, Mw = l.deconv ? lp.Wi : lp.Wo;
        int c[3] = {f.wino[0], f.wino[1], f.wino[2]};
        const int npatches = (l.deconv ? 1 : 4) * (l.cin() / 16);
        if ((f.wino_set || M >= g_wino_min_m) && choose_wino(Mh, Mw, l.cout, t.nphases, npatches, B, &c[0], &c[1], &c[2])) {
            lp.path = PATH_WINO; lp.wino_cfg = c[0]; lp.wino_mbw = c[1]; lp.splits = c[2]; lp.kg = 1; lp.tile = 0;
        } else if (f.wino_set) {
            if (f.path) return fail(RY_EINVAL, "no Winograd plan %d:%d:%d for a %d x %d grid", c[0], c[1], c[2], Mh, Mw);
            return fail(RY_EINVAL, "RY_WINO: no Winograd plan %d:%d:%d for %s", c[0], c[1], c[2], l.name);
        }
    }
    if (lp.path == 0) {                                      // no implicit-GEMM layout
        lp.path = f.path ? f.path : PATH_DIRECT; lp.splits = 1;
        if (!f.path && !l.deconv && l.k == 3 && l.stride == 1 && l.pad == 1) {
            if (l.src_a < 0 && l.cin() == 1 && l.cout % 4 == 0) lp.path = PATH_FIRST;
            if (out_layer && l.cout == 1 && l.cin() % 128 == 0 && l.cin_a % 4 == 0) lp.path = PATH_LAST;   // exp / edge-pad / crop of SuperResolution.convert fused into the last layer
        }
        if (lp.path == PATH_LAST) {
            lp.last_rows = lp.Ho;             // convert mode: overwritten with n_frames at enqueue time
            lp.last_cols = mode == 1 ? lp.Wo + 1 : lp.Wo;
            lp.last_exp = mode == 1;
        }
    }
    if (lp.splits > 1) {
        const size_t out_elems = (size_t)B * lp.Ho * lp.Wo * l.cout;
        RY_TRY(arena.alloc(&lp.slabs, out_elems * lp.splits));
        RY_TRY(poison_fill(ctx, lp.slabs, out_elems * lp.splits));
    }
    return RY_OK;
}

int build_plan(ry_net* net, Plan& P) {
    const ry_net_desc& d = net->desc;
    const int nd = d.ndim, B = P.B;
    P.lp.assign(16, LayerPlan());
    int H = nd == 2 ? P.T : 1, W = nd == 2 ? d.width : P.T;
    // spatial sizes per layer
    for (int i = 0; i < 16; ++i) {
        const Layer& l = net->layers[i];
        LayerPlan& lp = P.lp[i];
        int hi, wi;
        if (l.src_a < 0) { hi = H; wi = W; } else { hi = P.lp[l.src_a].Ho; wi = P.lp[l.src_a].Wo; }
        lp.Hi = hi; lp.Wi = wi;
        if (l.deconv) { lp.Ho = nd == 2 ? hi * 2 : 1; lp.Wo = wi * 2; }
        else {
            const int span = l.dil * (l.k - 1) + 1;
            lp.Ho = nd == 2 ? (hi + 2 * l.pad - span) / l.stride + 1 : 1;
            lp.Wo = (wi + 2 * l.pad - span) / l.stride + 1;
        }
        if (lp.Ho < 1 || lp.Wo < 1) return fail(RY_EINVAL, "%s: input %dx%d is too small for this predictor", l.name, hi, wi);
        if (l.src_b >= 0 && (P.lp[l.src_b].Ho != hi || P.lp[l.src_b].Wo != wi))
            return fail(RY_EINVAL, "%s: skip connection is %dx%d but decoder is %dx%d (frames must be a multiple of %d)", l.name,
                        P.lp[l.src_b].Ho, P.lp[l.src_b].Wo, hi, wi, 1 << (d.extensive_layers > 0 ? d.extensive_layers - 1 : 0));
        const double taps = (double)ipow((size_t)l.k, nd);
        const double in_area = (double)B * hi * wi, out_area = (double)B * lp.Ho * lp.Wo;
        lp.flops = 2.0 * l.cin() * l.cout * taps * (l.deconv ? in_area : out_area);
        lp.bytes = 4.0 * ((double)l.cin() * l.cout * taps + in_area * l.cin() + out_area * l.cout);
        if ((double)out_area * l.cout >= 2.0e9 || in_area * l.cin() >= 2.0e9)
            return fail(RY_EINVAL, "%s: activation exceeds 2^31 elements; lower the batch", l.name);
        if (nd == 2 && ((double)out_area * l.cout >= 1.0e9 || in_area * l.cin() >= 1.0e9))
            return fail(RY_EINVAL, "%s: activation exceeds 4 GB (32-bit byte offsets of the implicit GEMM); lower the batch", l.name);
    }
    // buffers
    if (nd == 1) {
        // the output-stationary kernels whenever every layer can take them (generic stride / dilation / GLU layers: the weight-streaming kernels)
        P.s1_os = true;
        for (int i = 0; i < 16; ++i) if (!c1d_os_capable(net->layers[i]) || !net->layers[i].w1os) P.s1_os = false;
        // the pad of the convert wrapper inside the first layer: a stride-1 first layer whose input channels fit one lane set
        P.s1_padfuse = P.s1_os && P.mode == 1 && c1d_mode(net->layers[0]) == RY_C1D_S1 && net->layers[0].cin() <= 64;
    }
    for (int i = 0; i < 16; ++i) {
        const Layer& l = net->layers[i];
        LayerPlan& lp = P.lp[i];
        const size_t out_elems = (size_t)B * lp.Ho * lp.Wo * l.cout;
        if (nd == 1 && P.s1_os) {
            plan_s1_os(l, lp, B);
            if (i < 15) {                                                    // the last layer stores straight into the caller's block
                RY_TRY(P.arena.alloc(&lp.out, out_elems));
                RY_TRY(poison_fill(net->ctx, lp.out, out_elems));
            }
        } else if (nd == 1) {
            const int mode = c1d_mode(l);
            lp.splits = choose_splits_1d(l, B, mode == RY_C1D_DECONV ? lp.Wi : lp.Wo, mode);
            lp.slab_stride = (long long)out_elems;
            RY_TRY(P.arena.alloc(&lp.raw, out_elems * lp.splits));
            RY_TRY(poison_fill(net->ctx, lp.raw, out_elems * lp.splits));
        } else {
            RY_TRY(alloc_ztail(net->ctx, P.arena, &lp.out, out_elems));
            bool src16 = l.src_a >= 0;                       // the network input has no bf16 copy, nor has the output of a direct layer
            for (int src : {l.src_a, l.src_b}) {
                const int sp = src >= 0 ? P.lp[src].path : 0;
                if (src >= 0 && sp != PATH_FIRST && sp != PATH_IGEMM && sp != PATH_IGEMM_BF16 && sp != PATH_OS2D) src16 = false;
            }
            RY_TRY(plan_s2_layer(net->ctx, P.arena, l, lp, B, net->dtype, g_force[i], src16, i == 15, P.mode));
            if (lp.path == PATH_WINO) RY_TRY(ensure_wwin(net, i, &lp.wwin));
        }
    }
    RY_TRY(wait_lazy(net));
    // bf16 mode: which copies of each activation are needed (fp32 for fp32 consumers and the caller, bf16 for bf16 consumers)
    if (nd == 2 && net->dtype != 0) {
        const bool x3 = net->dtype == 2;
        std::vector<char> need32(16, 0), need16(16, 0);
        need32[15] = 1;
        for (int i = 0; i < 16; ++i)
            for (int src : {net->layers[i].src_a, net->layers[i].src_b})
                if (src >= 0) (P.lp[i].path == PATH_IGEMM_BF16 ? need16 : need32)[src] = 1;
        for (int i = 0; i < 16; ++i) {
            LayerPlan& lp = P.lp[i];
            lp.w32 = need32[i] || lp.path == PATH_DIRECT || lp.path == PATH_LAST; lp.w16 = need16[i];
            lp.o16x3 = x3;
            if (lp.w16) {
                float* q = nullptr;
                RY_TRY(alloc_ztail(net->ctx, P.arena, &q, ((size_t)B * lp.Ho * lp.Wo * net->layers[i].cout * (x3 ? 2 : 1) + 1) / 2));
                lp.out16 = reinterpret_cast<unsigned short*>(q);
            }
        }
    }
    // staging
    const int cin_user = nd == 1 ? d.in_ch : (P.mode == 1 ? d.width + 1 : d.width);
    const int cout_user = nd == 1 ? d.out_ch : (P.mode == 1 ? d.width + 1 : d.width);
    const int rows_user = P.T;                 // convert mode: any n_frames < T shares this plan
    P.user_in_floats = (size_t)B * rows_user * cin_user;
    P.user_out_floats = (size_t)B * rows_user * cout_user;
    RY_TRY(P.arena.alloc(&P.user_in, P.user_in_floats));
    RY_TRY(P.arena.alloc(&P.user_out, P.user_out_floats));
    if (P.mode == 1) {
        RY_TRY(P.arena.alloc(&P.x_in, (size_t)B * P.T * (nd == 1 ? d.in_ch : d.width)));
        RY_TRY(poison_fill(net->ctx, P.x_in, (size_t)B * P.T * (nd == 1 ? d.in_ch : d.width)));
    } else {
        P.x_in = nullptr;                      // raw forward reads the caller's block directly (cur_in)
    }
    return RY_OK;
}

// RY_PLAN / RY_WINO / RY_OS2: comma-separated "layer:v1[:v2 ...]" entries, at least one value (the missing ones: 0); `take` checks the values and
// stores them in the layer's record
static int parse_force(const char* var, const char* syntax, bool (*take)(LayerForce& f, const int* v)) {
    const char* e = getenv(var);
    for (const char* q = e; q && *q; q = strchr(q, ',') ? strchr(q, ',') + 1 : nullptr) {
        int i = -1, v[4] = {0, 0, 0, 0};
        if (sscanf(q, "%d:%d:%d:%d:%d", &i, &v[0], &v[1], &v[2], &v[3]) < 2 || i < 0 || i >= 16 || !take(g_force[i], v))
            return fail(RY_EINVAL, "%s: expected %s", var, syntax);
    }
    return RY_OK;
}

// process-wide A/B and diagnostic switches, read when a context is created
// RY_PLAN / RY_WINO / RY_OS2: read when a context is created and again at every ry_net_set_dtype (which drops the launch plans), so that one process can
// sweep plans (scripts/gpu_x3_plansweep.py, scripts/gpu_lanesweep.py)
int read_plan_env() {
    for (LayerForce& f : g_force) f = LayerForce();
    g_os2_maxcost = 4608; g_os2_min_filter = (size_t)1 << 21;
    if (const char* e = getenv("RY_OS2_MAXCOST")) g_os2_maxcost = atoi(e);
    if (const char* e = getenv("RY_OS2_MINW")) g_os2_min_filter = (size_t)atoll(e);
    g_wino = 1; g_wino_min_m = 256;
    if (const char* e = getenv("RY_WINOGRAD")) g_wino = atoi(e);
    if (const char* e = getenv("RY_WINO_MINM")) g_wino_min_m = atoi(e);
    RY_TRY(parse_force("RY_WINO", "layer:cfg[:mbw[:splits]][,...]", [](LayerForce& f, const int* v) {
        if (v[0] < 0 || v[0] > 2 || v[1] < 0 || v[2] < 0) return false;
        f.wino_set = true; f.wino[0] = v[0]; f.wino[1] = v[1]; f.wino[2] = v[2];
        return true;
    }));
    g_poison = 0;
    if (const char* e = getenv("RY_POISON")) g_poison = atoi(e);
    RY_TRY(parse_force("RY_OS2", "layer:mt4[:nt4[:waves[:depth]]][,...]", [](LayerForce& f, const int* v) {
        if (v[0] < 0 || v[1] < 0 || v[2] < 0 || v[3] < 0) return false;
        f.os2_set = true; f.os2[0] = v[0]; f.os2[1] = v[1]; f.os2[2] = v[2]; f.os2[3] = v[3];
        return true;
    }));
    return parse_force("RY_PLAN", "layer:tile:splits:kgroups[,...]", [](LayerForce& f, const int* v) {
        if (v[0] < 0 || v[0] > TILE_96x128 || v[0] == 2 || v[1] < 0 || v[2] < 0 || v[2] > 2) return false;
        f.tile = v[0]; f.splits = v[1]; f.kg = v[2];
        return true;
    });
}

int read_env_switches() {
    // RY_FILTER_BUILD=host|device: the filter build mode.  Unlike the switches below it also has a setter (ry_set_filter_build), so an absent variable
    // leaves the mode alone; a value that is neither is refused before anything else is touched
    if (const char* e = getenv("RY_FILTER_BUILD")) {
        if (!strcmp(e, "host")) g_filter_build = 0;
        else if (!strcmp(e, "device")) g_filter_build = 1;
        else return fail(RY_EINVAL, "RY_FILTER_BUILD: expected host or device, got '%s'", e);
    }
    // (re-read by ry_debug_reload_env: an absent variable means the defaults)
    g_autotune = 0; g_autotune_reps = 3; g_autotune_max = 0; g_autotune_pick = -1;
    if (const char* e = getenv("RY_AUTOTUNE")) {                                        // "1[:reps[:max[:pick]]]"
        int on = 0, reps = 3, mx = 0, pick = -1;
        if (sscanf(e, "%d:%d:%d:%d", &on, &reps, &mx, &pick) < 1) return fail(RY_EINVAL, "RY_AUTOTUNE: expected 1[:reps[:max[:pick]]]");
        g_autotune = on; g_autotune_reps = reps > 0 ? reps : 1; g_autotune_max = mx; g_autotune_pick = pick;
    }
    g_x3_min_m = 128; g_s2_crop = 2;
    if (const char* e = getenv("RY_X3_MINM")) g_x3_min_m = atoi(e);
    if (const char* e = getenv("RY_S2_CROP")) g_s2_crop = atoi(e);
    g_s2_hole = 1;
    if (const char* e = getenv("RY_S2_HOLE")) g_s2_hole = atoi(e);
    return read_plan_env();
}

unsigned short host_f2bf(float f) {
    unsigned u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

float host_bf2f(unsigned short h) { const unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }

// bf16 filters of one layer from its fp32 fragment-order blocks (wig layout): blocks [..][C/32][64][32] -> [..][C/64][64][64], RNE
static void build_wig16(const Layer& l, const std::vector<float>& w32, std::vector<unsigned short>& out) {
    const TapTable t = make_taps(l);
    const int C = l.cin(), N = l.cout;
    const size_t outer = (size_t)t.nphases * (N / 64) * t.ntaps;
    out.assign(outer * (size_t)C * 64, 0);
    for (size_t o = 0; o < outer; ++o)
        for (int c = 0; c < C; ++c)
            for (int nl = 0; nl < 64; ++nl)
                out[(o * (C / 64) + c / 64) * 4096 + wig16_inblock(nl, c % 64)] = host_f2bf(w32[(o * (C / 32) + c / 32) * 2048 + wig_inblock(nl, c % 32)]);
}

// Split-bf16 filters of one layer from its fp32 fragment-order blocks (wig layout): the K axis of each source (C channels) becomes
// [W_hi | W_hi | W_lo] (3 C), matching the activations' [x_hi | x_lo | x_hi]: the kernel's plain bf16 contraction over that axis is
// x_hi W_hi + x_lo W_hi + x_hi W_lo.  hi = bf16(w), lo = bf16(w - hi), both RNE.
static void build_wigx3(const Layer& l, const std::vector<float>& w32, std::vector<unsigned short>& out) {
    const TapTable t = make_taps(l);
    const int C = l.cin(), N = l.cout, K3 = 3 * C;
    const size_t outer = (size_t)t.nphases * (N / 64) * t.ntaps;
    out.assign(outer * (size_t)K3 * 64, 0);
    for (size_t o = 0; o < outer; ++o)
        for (int kk = 0; kk < K3; ++kk) {
            int seg, c;
            if (kk < 3 * l.cin_a) { seg = kk / l.cin_a; c = kk % l.cin_a; }
            else { const int k2 = kk - 3 * l.cin_a; seg = k2 / l.cin_b; c = l.cin_a + k2 % l.cin_b; }
            for (int nl = 0; nl < 64; ++nl) {
                const float w = w32[(o * (C / 32) + c / 32) * 2048 + wig_inblock(nl, c % 32)];
                const unsigned short hi = host_f2bf(w);
                out[(o * (K3 / 64) + kk / 64) * 4096 + wig16_inblock(nl, kk % 64)] = seg == 2 ? host_f2bf(w - host_bf2f(hi)) : hi;
            }
        }
}

// The bf16 (dtype 1: Layer::wig16) or split-bf16 (dtype 2: Layer::wigx3) filters of a stage-2 implicit-GEMM layer whose sources are whole 64-channel
// chunks, built once from its fp32 blocks into `arena` (ry_net_set_dtype for predictors, ry_conv2d for the single operator)
int prepare_bf16(ry_ctx* ctx, Arena& arena, Layer& l, int dtype) {
    float*& dst = dtype == 2 ? l.wigx3 : l.wig16;
    if (!l.wig || dst || l.cin_a % 64 != 0 || l.cin_b % 64 != 0) return RY_OK;
    const TapTable t = make_taps(l);
    std::vector<float> w32((size_t)t.nphases * l.cout * t.ntaps * l.cin());
    RT_TRY(rt::d2h(w32.data(), l.wig, w32.size() * sizeof(float), ctx->stream));
    RT_TRY(rt::stream_sync(ctx->stream));
    arena.stats.bytes_downloaded += (unsigned long long)(w32.size() * sizeof(float));
    std::vector<unsigned short> w16;
    (dtype == 2 ? build_wigx3 : build_wig16)(l, w32, w16);
    float* d = nullptr;
    RY_TRY(arena.alloc(&d, (w16.size() + 1) / 2));
    arena.stats.bytes_uploaded += (unsigned long long)(w16.size() * sizeof(unsigned short));
    RT_TRY(rt::h2d(d, w16.data(), w16.size() * sizeof(unsigned short), ctx->stream));
    RT_TRY(rt::stream_sync(ctx->stream));
    dst = d;
    return RY_OK;
}
