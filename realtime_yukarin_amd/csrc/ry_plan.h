// ry_plan.h -- what the three predictor units of libry355.so share: ry_plan.cpp (topology, filter re-layout, the launch planner and its switches),
// ry_exec.cpp (the kernels' launchers, the captured forward, profiling, the single operators) and ry_net.cpp (the C ABI of include/ry355.h).
// Host-side only: nothing here needs ry_kernels.h (one unit, ry_exec.cpp, instantiates the kernels).
#pragma once
#include "ry_dev.h"
#include "ry_host.h"

// ------------------------------------------------------------------------------------------------
// host-side filter re-layout and BatchNormalization folding (once, at creation)
// ------------------------------------------------------------------------------------------------
struct TapTable {
    int nphases = 1, ntaps = 1;
    int dy[4][16], dx[4][16], ky[4][16], kx[4][16], pdy[4], pdx[4];
};

// Activation buffers that an implicit-GEMM layer may read end in ZTAIL zeroed floats: the LDS-DMA kernel fetches its padding
// from there (RyConvGeom::zoff1 / zoff2); nothing ever writes them.
// (round 5: a whole zeroed PIXEL of up to 2048 channels -- ry_c2d_os fetches out-of-image taps from it at any channel offset)
static const size_t ZTAIL = 2048;

// ---- stage-2 output-stationary layers (ry_c2d_os) ----
// (MT4, NT4, WAVES, DEPTH): tile of 4 MT4 rows x 4 NT4 output channels per workgroup, WAVES waves that deal the K units among them in rounds
// of four, DEPTH units in flight per wave.  Sixteen-wave workgroups have 128 registers per lane: small tiles only.
#define RY_OS2_CONFIGS(X)                                                                                              \
    X(1, 1, 4, 4) X(1, 1, 8, 4) X(1, 1, 8, 2) X(1, 1, 16, 2) X(2, 1, 4, 4) X(2, 1, 8, 4) X(2, 1, 8, 2) X(2, 1, 16, 2)     \
    X(3, 1, 4, 4) X(3, 1, 8, 4) X(3, 1, 8, 2) X(3, 1, 16, 2) X(4, 1, 4, 4) X(4, 1, 8, 4) X(4, 1, 8, 2) X(4, 1, 16, 2)     \
    X(6, 1, 4, 4) X(6, 1, 8, 2)                                                             \
    X(1, 2, 4, 4) X(1, 2, 8, 4) X(1, 2, 8, 2) X(1, 2, 16, 2) X(2, 2, 4, 4) X(2, 2, 8, 4) X(2, 2, 8, 2) X(2, 2, 16, 2)     \
    X(3, 2, 4, 4) X(3, 2, 8, 4) X(3, 2, 8, 2) X(3, 2, 16, 2) X(4, 2, 4, 4) X(4, 2, 8, 4) X(4, 2, 8, 2) X(4, 2, 16, 2)     \
    X(6, 2, 4, 4) X(6, 2, 8, 2)                                                                             \
    X(1, 4, 4, 4) X(1, 4, 8, 4) X(1, 4, 8, 2) X(1, 4, 16, 2) X(2, 4, 4, 4) X(2, 4, 8, 4) X(2, 4, 8, 2) X(2, 4, 16, 2)     \
    X(3, 4, 4, 4) X(3, 4, 8, 4) X(3, 4, 8, 2) X(4, 4, 4, 4) X(4, 4, 8, 2) X(6, 4, 4, 2)

// The LDS-DMA pixel path keeps one KiB per (wave, four tile rows, unit in flight): slices with two units in flight and at most 64 KiB of ring
// (what the other window lane's kernels leave free on a CU).
static constexpr bool os2_xl_ok(int mt4, int waves, int depth) { return depth == 2 && mt4 * waves <= 32; }

// One layer's override of the stage-2 planner: RY_PLAN / RY_WINO / RY_OS2 for the layers of a predictor (read_plan_env), the path and tile
// arguments of ry_conv2d for the single operator.  Zeros: the planner's choice.
struct LayerForce {
    int tile = 0, splits = 0, kg = 0;                   // RY_PLAN: implicit-GEMM tile, external splits, K groups
    bool wino_set = false; int wino[3] = {0, 0, 0};     // RY_WINO: cfg (0: the layer stays off the Winograd form), M-blocks per tile row, splits
    bool os2_set = false; int os2[4] = {0, 0, 0, 0};    // RY_OS2: mt4 (0: the layer stays on the implicit GEMM), nt4, waves, depth
    int path = 0;                                       // ry_conv2d: the path the caller names, run whatever the switches say (0: the planner's)
    bool fixed() const { return tile || splits || kg; } // RY_PLAN fixes the layer's implicit-GEMM plan
};

// The rows one enqueue of a plan computes (plan_window_rows): rows [k0, k1) of the window are kept; layer i runs on crop_hi[i] input rows from
// crop_lo[i] (0: all) and leaves output rows [hole_lo[i], hole_lo[i] + hole_n[i]) to ry_rep_rows (0: none)
struct WindowRows {
    int k0 = 0, k1 = 0;
    int crop_lo[16] = {}, crop_hi[16] = {}, hole_lo[16] = {}, hole_n[16] = {};
};

// ---- what the units share (definitions: ry_plan.cpp / ry_exec.cpp) ----
std::vector<Layer> build_topology(const ry_net_desc& d);
size_t ipow(size_t b, int e);
size_t layer_param_count(const Layer& l, int ndim);
int check_desc(const ry_net_desc* d);
TapTable make_taps(const Layer& l);
bool wino_eligible(const Layer& l, int ndim);
int prepare_layer(ry_ctx* ctx, Arena& arena, Layer& l, int ndim, float eps, const float* W, const float* b, const float* bn, bool want_os2 = false);
int prepare_bf16(ry_ctx* ctx, Arena& arena, Layer& l, int dtype);
int upload_wwin(ry_ctx* ctx, Arena& arena, const Layer& l, float** out);
// filter build mode (ry_set_filter_build / RY_FILTER_BUILD): 0 host loops + one upload per layout, 1 one upload of the raw filter + layout kernels
int filter_build_mode();
int set_filter_build(int mode);
int finish_filter_build(ry_ctx* ctx);                         // device mode: wait for the layout kernels, give the staging buffer back
size_t filter_layout_floats(const Layer& l, int kind);        // floats of layout `kind` (RY_LAYOUT_*) of a layer that has it
int net_wwin(ry_net* net, int layer, const float** out);      // the Winograd filters of a predictor layer, built if need be and waited for
// the layout kernels of relayout_kernels.h on ctx->stream (ry_exec.cpp): the raw filter `W` on the card -> layout `kind` in `out`; wdir -> wwin
int launch_relayout(ry_ctx* ctx, const Layer& l, int kind, const float* W, float* out);
int launch_relayout_wino(ry_ctx* ctx, const Layer& l, const float* wdir, float* out);
int alloc_ztail(ry_ctx* ctx, Arena& arena, float** p, size_t nfloats);
int poison_fill(ry_ctx* ctx, float* p, size_t nfloats);       // RY_POISON: NaN patterns over a buffer a launch is about to write (else nothing)
void tile_dims(int tile, int* bm, int* bn);
extern int g_x3_min_m;
extern int g_autotune;
extern int g_autotune_reps, g_autotune_max;
extern int g_autotune_pick;
bool layer_plan_fixed(int i);
const char* tile_name(int tile, int kg, bool bf16, int patch);
int tile_occ(int tile, int kg);
double est_time(long blocks, int bm, int bn, int s, int occ, int kg, int M, int N, int nk);
void choose_igemm(const Layer& l, int M, int nphases, int nk, int* tile, int* splits, int* kg, int bf16 = 0 /* 1 bf16, 2 split-bf16 */);
bool choose_os2(int M, int N, int nphases, int U, int* mt4, int* nt4, int* waves, int* depth, double* cost_out = nullptr);
bool wino_cfg_dims(int cfg, int* wm, int* wn, int* nsl);
void wino_tile_hw(int cfg, int mbw, int* th, int* tw);
const char* wino_name(int cfg, int mode);
bool choose_wino(int Mh, int Mw, int N, int nphases, int npatches, int B, int* cfg, int* mbw, int* splits);
int c1d_mode(const Layer& l);
int c1d_tile_len(int mode);
int choose_splits_1d(const Layer& l, int B, int rows, int mode);
bool c1d_os_capable(const Layer& l);
void plan_s1_os(const Layer& l, LayerPlan& lp, int B);        // ry_c1d_os: ci waves per position group (os_kt) and the slice (os_cb x os_tp) of a stage-1 layer
bool plan_tile_rows(const LayerPlan& lp, int Mh, int Mw, int* th, int* tw_out = nullptr);
bool plan_hole_ok(const Layer& l, const LayerPlan& lp, int lo, int n);
int plan_s2_layer(ry_ctx* ctx, Arena& arena, const Layer& l, LayerPlan& lp, int B, int dtype, const LayerForce& f, bool src16, bool out_layer, int mode);
WindowRows plan_window_rows(const ry_net* net, const Plan& P);
// What the launchers derive from a layer's plan at enqueue time, in one place for them and for ry_net_debug_plan:
// the reduce kernel behind an external split of `total` output floats (many slabs, few outputs: ry_splitk_reduce_wide) ...
inline bool plan_reduce_wide(int splits, long long total) { return splits >= 16 && total <= (1 << 20); }
// ... and the input-patch variant of the implicit GEMM on 16-pixel-wide 2-D tiles (K units = whole channel chunks): 1: sub-pixel deconvolution, one patch
// per channel chunk; 2: k4 s2 p1 convolution, one patch per (chunk, input parity); 0: none.  Small layers: the longer set-up costs more than the reuse
// saves (measured at M = 192).  M: GEMM rows of the launch, tw: tile width (0: raster tiles), cpt: channel chunks per tap.
inline int plan_igemm_patch(const Layer& l, const LayerPlan& lp, int M, int tw, int cpt) {
    if (tw != 16 || !(M >= 512 || lp.any_m_patch)) return 0;
    if (l.deconv && lp.splits * lp.kg <= cpt) return 1;
    if (!l.deconv && l.k == 4 && l.stride == 2 && l.pad == 1 && l.dil == 1 && lp.splits * lp.kg <= 4 * cpt) return 2;
    return 0;
}
// Does the first stage-1 layer of this enqueue pad the caller's block itself (no ry_pad_min_rows node, Plan::x_in stays unwritten)?  The fused pad
// takes the column minimum inside the workgroups that reach the padding: one chain of n_frames / 8 load rounds, worth it while the window is
// short (measured: 300 frames -3 us, 1000 frames +14 us against the separate node; the cooperative minimum: one round of loads per 1024 frames)
inline bool plan_padfuse_now(const ry_net* net, const Plan& P) { return net->desc.ndim == 1 && P.s1_padfuse && P.n_frames <= 2048; }
int build_plan(ry_net* net, Plan& P);
int autotune_plan(ry_net* net, Plan& P);
int get_plan(ry_net* net, int B, int T, int mode, int n_frames, Plan** out);
int run_plan(ry_net* net, Plan& P, const float* x, float* y, int on_device);
int read_plan_env();
int read_env_switches();
unsigned short host_f2bf(float f);
float host_bf2f(unsigned short h);
int profile_plan(ry_net* net, Plan* P, int reps, ry_kernel_stat* stats, int max_stats, int* n_stats);
