/* ry355.h -- C ABI of libry355.so: the MI355X-native convert hot path of realtime-yukarin.
 *
 * The reference has no FFI for this path: its boundary is the Python surface of two un-vendored
 * packages.  Each entry point below names the reference call it stands in for; the ctypes binding a
 * maintainer adds is realtime_yukarin_amd/_lib.py.
 *
 * Conventions: plain pointers and sizes, no torch types.  Every function returning int returns 0 on
 * success and a negative RY_E* code on failure (never aborts); ry_last_error() gives the message for
 * the calling thread.  All tensors are float32, channels-last:
 *   stage-1  [batch][frames][channels]      (= the (N, C) feature matrix of encode_feature, untransposed)
 *   stage-2  [batch][frames][bins]
 * Threading: a context and its predictors are used by one thread at a time (the reference converts from a single-threaded worker
 * loop, convert_worker.py:45-59); different contexts / processes are independent.
 * `on_device` = 0: x / y are host pointers, the call returns after the result is in y.
 * `on_device` = 1: x / y are device pointers on the context's GPU; the call only enqueues work on the
 *                  context stream (ry_stream); use ry_sync or your own event to wait.
 */
#ifndef RY355_H
#define RY355_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RY_OK 0
#define RY_EINVAL (-1)   /* bad argument / shape the predictor cannot take */
#define RY_EHIP (-2)     /* HIP runtime error (message carries hipGetErrorString) */
#define RY_ENOMEM (-3)
#define RY_ESTATE (-4)   /* wrong context / destroyed handle */

#define RY_ACT_NONE 0
#define RY_ACT_LRELU 1
#define RY_ACT_RELU 2
#define RY_ACT_GLU 3

typedef struct ry_ctx ry_ctx;
typedef struct ry_net ry_net;

/* `create_predictor(config.model)` / `create_predictor_sr(config.model)` arguments ([MEM], built inside
 * yukarin.AcousticConverter.__init__ / become_yukarin.SuperResolution.__init__; reference call sites
 * realtime_voice_conversion/converter/yukarin_converter.py:40-55, check.py:54-63). */
typedef struct ry_net_desc {
    int ndim;               /* 1 = stage-1 Predictor (Convolution1D), 2 = stage-2 SRPredictor (Convolution2D) */
    int in_ch, out_ch;      /* stage-2: 1, 1 */
    int base;               /* generator_base_channels */
    int extensive_layers;   /* generator_extensive_layers */
    int width;              /* stage-2: bins fed to the predictor (fft_size/2 = 512); stage-1: 1 */
    float bn_eps;           /* Chainer BatchNormalization eps = 2e-5 */
    float lrelu_slope;      /* F.leaky_relu slope = 0.2 */
    int glu;                /* stage-1 only, UNVERIFIED [MEM]: `model.glu_generator` of the stage-1 config -- every conv + BatchNormalization block of
                             * the U-Net produces twice the channels and is gated, a * sigmoid(b), instead of (leaky) ReLU.  The upstream class lives in
                             * the un-vendored `yukarin` package; the strict K-list / shape check of the loader decides whether a real model fits. */
} ry_net_desc;

/* One context per (process, GPU).  Create it in the process that converts (after fork), cf. the
 * convert worker process of run.py:69-79.  `chainer.cuda.get_device(gpu).use()` equivalent. */
int ry_init(int device_ordinal, ry_ctx** out);
void ry_shutdown(ry_ctx* ctx);
int ry_sync(ry_ctx* ctx);
void* ry_stream(ry_ctx* ctx);                 /* hipStream_t the context enqueues on */
int ry_device_count(void);
const char* ry_last_error(void);

/* Number of floats of the flat weight blob = K-list order of the Chainer save_npz keys:
 * encoder/c0/{W,b}, encoder/c{1..7}/{c/W,c/b,batchnorm/gamma,beta,avg_mean,avg_var}, decoder/c{0..6}/..., decoder/c7/{W,b}. */
size_t ry_net_param_count(const ry_net_desc* desc);

/* `chainer.serializers.load_npz(model_path, model)` + `model.to_gpu(gpu)` ([MEM]): takes the flat blob
 * (host, or device when weights_on_device -- e.g. the buffer an RCCL broadcast just filled), folds
 * BatchNormalization into per-channel scale/shift and re-lays the filters out for the kernels. */
int ry_net_create(ry_ctx* ctx, const ry_net_desc* desc, const float* weights, size_t n_floats,
                  int weights_on_device, ry_net** out);
void ry_net_destroy(ry_net* net);
/* A second handle on the same predictor: the filters are shared (freed with the last handle), the clone has its own stream, launch
 * plans, activation buffers and captured graphs.  ry_net_set_dtype on one handle does not change the others. */
int ry_net_clone(ry_net* net, ry_net** out);
/* BASELINE config #5: dtype 1 runs the stage-2 implicit-GEMM layers with bf16 operands on v_mfma_f32_32x32x16_bf16 (fp32 accumulate,
 * bf16 activations between those layers; filters converted once).  dtype 2 ("split-bf16") runs them as three bf16 products per fp32
 * product -- x = hi + lo, w = hi + lo, x w ~ hi hi + lo hi + hi lo -- on the same instruction with fp32 accumulation: results agree
 * with the fp32 path to ~2e-6 (inside the 1e-4 parity bar) at 3/16 of the matrix-pipe time.  dtype 0 (default) is exact fp32.
 * Tolerances: DESIGN.md 5.1 (bf16, split-bf16). */
int ry_net_set_dtype(ry_net* net, int dtype);

/* `Predictor.__call__` / `SRPredictor.__call__` on an already padded block (frames % 128 == 0 when
 * extensive_layers == 8).  stage-1: x [batch][frames][in_ch] -> y [batch][frames][out_ch];
 * stage-2: x [batch][frames][width] -> y [batch][frames][width]. */
int ry_net_forward(ry_net* net, const float* x, float* y, int batch, int frames, int on_device);

/* Array part of `AcousticConverter.convert` (voice_changer.py:33): x [batch][n_frames][in_ch] ->
 * pad time to n + (128 - n % 128) with the per-channel minimum -> Predictor -> crop -> y [batch][n_frames][out_ch]. */
int ry_ac_convert(ry_net* stage1, const float* x, float* y, int batch, int n_frames, int on_device);

/* `SuperResolution.convert` (voice_changer.py:41): sp [batch][n_frames][width+1] -> pad 'minimum' -> log ->
 * drop last bin -> SRPredictor -> edge-pad one bin -> exp -> crop -> out [batch][n_frames][width+1]. */
int ry_sr_convert(ry_net* stage2, const float* sp, float* out, int batch, int n_frames, int on_device);
/* ry_sr_convert for a caller that discards the first `discard_front` / last `discard_back` frames of every window: rows
 * [discard_front, n_frames - discard_back) of `out` are written (bit-identical to ry_sr_convert); the others come back as zeros
 * (host arrays) or are left untouched (device pointers). */
int ry_sr_convert_rows(ry_net* net, const float* sp, float* out, int batch, int n_frames, int discard_front, int discard_back, int on_device);

/* ---- single operators (the Chainer links of SURVEY.md section 2.1), host pointers, Chainer weight layouts ---- */
/* L.ConvolutionND(1) / L.DeconvolutionND(1) [+ L.BatchNormalization] [+ activation].  x [B][L][Cin] ->
 * y [B][Lout][Cout] (GLU: Cout/2 channels).  W: (Cout,Cin,k) or, transposed, (Cin,Cout,k); bn = gamma|beta|avg_mean|avg_var
 * (4*Cout floats) or NULL.  k <= 4; transposed requires k4 s2 p1.  splits = 0 lets the library choose. */
int ry_conv1d(ry_ctx* ctx, const float* x, int B, int L, int Cin, const float* W, const float* bias, const float* bn,
              int Cout, int k, int stride, int pad, int dilate, int transposed, int act, int splits, float* y);
/* the same layer on the output-stationary stage-1 kernel of the predictors (ry_c1d_os), one launch.  xa [B][rows][Ca] with rows = Lin, or
 * n_real when n_real > 0 (the fused pad of the convert wrapper: rows n_real .. Lin - 1 are the per-channel minimum of the real rows; one source
 * of at most 64 channels into a stride-1 layer); xb [B][Lin][Cb] the second source of a skip concat, or NULL with Cb = 0.  W over Ca + Cb input
 * channels as in ry_conv1d, k <= 4, no dilation; the kernel takes k4 s2 p1 (de)convolutions and stride-1 convolutions with pad <= 3, no GLU.
 * Slice cb x tp: 4x8, 4x4, 2x8 or 2x4 (no 4x8 for a deconvolution; 2x4 only when Cb > 0 and Ca % 64 != 0), 0 / 0 = the planner's pick.
 * keep: rows stored per window, 0 = all Lout.  y [B][keep][Cout].  Other inputs are refused with RY_EINVAL. */
int ry_conv1d_os(ry_ctx* ctx, const float* xa, const float* xb, int B, int Lin, int Ca, int Cb, const float* W, const float* bias, const float* bn,
                 int Cout, int k, int stride, int pad, int transposed, int act, int cb, int tp, int n_real, int keep, float* y);
/* L.Convolution2D / L.Deconvolution2D.  x [B][H][W][Cin] -> y [B][Ho][Wo][Cout].  path: 0 auto, 1 implicit-GEMM (MFMA),
 * 2 direct (VALU), 3 SR first layer (1 -> N, 3x3), 4 SR last layer (C -> 1, 3x3, channels read as two sources), 5 implicit-GEMM with bf16 operands,
 * 6 implicit-GEMM in split-bf16 form (x_hi w_hi + x_lo w_hi + x_hi w_lo, fp32 accumulate; the input is split on the host here); tile: 0 auto, 1 = 128x128, 3 = 64x128, 4 = 32x128, 5 = 128x64, 6 = 96x128 (+16: two K groups per workgroup, +32: one). */
int ry_conv2d(ry_ctx* ctx, const float* x, int B, int H, int W, int Cin, const float* Wt, const float* bias, const float* bn,
              int Cout, int k, int stride, int pad, int transposed, int act, int path, int tile, int splits, float* y);
/* the same with a dilation (plain convolution on the implicit-GEMM or the direct path): out = (H + 2 pad - dilate (k - 1) - 1) / stride + 1 */
int ry_conv2d_dilated(ry_ctx* ctx, const float* x, int B, int H, int W, int Cin, const float* Wt, const float* bias, const float* bn,
                      int Cout, int k, int stride, int pad, int dilate, int transposed, int act, int path, int tile, int splits, float* y);

/* ---- the whole device-resident convert: stage-1 -> combine_silent -> mc2sp -> +floor -> stage-2 (voice_changer.py:27-41) ----
 * mc2sp(mc) = exp(mc @ mtx) with mtx [(order+1)][bins] precomputed on the host (every step of pysptk.mc2sp before the exp is
 * linear); see realtime_yukarin_amd/sptk.py.  One H2D and one D2H per window instead of two round trips + a CPU mc2sp. */
typedef struct ry_vc ry_vc;
int ry_vc_create(ry_net* stage1, ry_net* stage2, const float* mtx, int order_plus_1, int bins, ry_vc** out);
void ry_vc_destroy(ry_vc* vc);
/* x_eff [n_eff][in_ch]: encode_feature of the effective (non-silent) frames; row_of[i] = frame index of row i;
 * mc_out [n_frames][order+1] (zeros on silent frames), sp_out [n_frames][bins].  n_eff may be 0 (all silent). */
int ry_vc_convert(ry_vc* vc, const float* x_eff, const int* row_of, int n_eff, int n_frames, float sp_floor,
                  float* mc_out, float* sp_out);
/* The same in two halves, for a convert loop that keeps several windows in flight (the live caller is the worker loop of
 * realtime_voice_conversion/worker/convert_worker.py:45-59: get -> convert -> put).  ry_vc_submit copies the window into a pinned
 * ring slot (six slots), queues H2D -> stage-1 -> combine_silent -> mc2sp -> stage-2 -> D2H on the two predictor streams and returns
 * a ticket WITHOUT waiting; ry_vc_wait blocks for that ticket and copies the results out.  H2D of window i + 1 and D2H of window i - 1
 * run under the kernels of window i.  ry_vc_convert == submit + wait.  RY_ESTATE when all slots are in flight. */
int ry_vc_submit(ry_vc* vc, const float* x_eff, const int* row_of, int n_eff, int n_frames, float sp_floor, int* ticket);
/* The caller will throw away the first `front` and the last `back` frames of every window it gets back -- ConvertStream.process converts
 * buffer + 2 x extra_time and picks the buffer (realtime_voice_conversion/stream/convert_stream.py:40-42).  Stage 2 then computes only the
 * rows that are kept (decoder layers on the row range they depend on; encoder and bottom of the U-Net whole); the kept rows are bit-identical
 * to the full result, the discarded rows of the returned spectrogram are zero (device-pointer calls: left untouched), mc is always complete.
 * Applies to every following ry_vc_submit / ry_vc_submit_wave / ry_vc_enqueue_device(_batch) / ry_vc_stage2_from_mc until changed;
 * (0, 0) = everything. */
int ry_vc_set_discard(ry_vc* vc, int front, int back);
/* Lanes: with `lanes` = 2 or 3 the ring slots run on their own predictor handles (ry_net_clone of the pair given to ry_vc_create: one
 * copy of the filters, separate streams / launch plans / activations), so that the windows in flight execute side by side instead of
 * one stage-2 forward after the other.  Same results.  Device-pointer callers (ry_vc_enqueue_device) must then give windows that are in
 * flight together their own output blocks.  No ticket may be in flight when the lane count changes.  Default 1. */
int ry_vc_set_lanes(ry_vc* vc, int lanes);
/* Streams of the lanes.  WIDE (0): a stage-1 and a stage-2 stream per lane, 2 x lanes + 2 users of hardware queues with the context and the
 * null stream.  When GPU_MAX_HW_QUEUES (read in ry_vc_create; absent = 4, HIP's default) is smaller than that, the core enqueues on fewer
 * streams: one stage-1 stream for all lanes beside a stage-2 stream per lane (2); RY_VC_STREAMS = wide | compact | compact-a | compact-b
 * forces a form (compact-a, 1: one stream per lane).  Same kernels in the same order per window: the results do not depend on the form.
 * TESTS ONLY: the form in use and the number of distinct streams the calls have enqueued on since ry_vc_create / ry_vc_set_lanes. */
int ry_vc_debug_streams(ry_vc* vc, int* form, int* n_streams);
int ry_vc_wait(ry_vc* vc, int ticket, float* mc_out, float* sp_out);
/* All pointers on the device, nothing waited for (ry_sync / your own event): consecutive calls pipeline by themselves -- stage-1 of
 * window i + 1 runs on its stream under stage-2 of window i.  bench.py times this. */
int ry_vc_enqueue_device(ry_vc* vc, const float* x_eff_dev, const int* row_of_dev, int n_eff, int n_frames, float sp_floor,
                         float* mc_out_dev, float* sp_out_dev);
/* Several independent windows of n_frames each in one call (streams served side by side; the backlog of run.py's queue): x_eff_dev /
 * row_of_dev hold the effective rows / row maps of the windows one after the other (sum of n_eff[] rows), n_eff is a HOST array of
 * n_windows counts, mc_out_dev [n_windows][n_frames][order+1], sp_out_dev [n_windows][n_frames][bins].  Stage 2 runs as one batch.
 * Window w of the result equals ry_vc_enqueue_device on that window up to summation order (the batch may run under another launch plan). */
int ry_vc_enqueue_device_batch(ry_vc* vc, int n_windows, const float* x_eff_dev, const int* row_of_dev, const int* n_eff, int n_frames,
                               float sp_floor, float* mc_out_dev, float* sp_out_dev);
/* The chain cut where the reference's own class cuts it, so that its unchanged step-by-step calls (voice_changer.py:33-41) keep
 * the data on the device between the two CNNs:
 *   ry_vc_stage1         `acoustic_converter.convert(f_in_effective)`: x_eff [n_eff][in_ch] -> y1_out [n_eff][order+1]; the rows
 *                        also stay on the device;
 *   ry_vc_stage2_from_mc `combine_silent` + `decode_spectrogram` + `sp += floor` + `super_resolution.convert` from those rows:
 *                        sp_out [n_frames][bins]; the intermediate spectrogram never visits the host;
 *   ry_vc_mid_sp         the intermediate spectrogram exp(mc @ mtx) + floor, for a caller that does read it. */
int ry_vc_stage1(ry_vc* vc, const float* x_eff, int n_eff, float* y1_out);
int ry_vc_stage2_from_mc(ry_vc* vc, const int* row_of, int n_eff, int n_frames, float sp_floor, float* sp_out);
int ry_vc_mid_sp(ry_vc* vc, const int* row_of, int n_eff, int n_frames, float sp_floor, float* sp_mid_out);
int ry_vc_reserve_frames(ry_vc* vc, int n_frames);   /* optional: size the ring ahead of the first window */
/* ry_vc_submit with `separate_effective` (voice_changer.py:27-31) ON THE DEVICE: the raw wave (float32) and the feature block of ALL
 * frames go up; frame powers (librosa.feature.rms(center=True, pad 'reflect') ** 2 in float32, numpy's summation order), the gate, the
 * ordered compaction of the effective rows and the scatter back happen there.  The gate is evaluated in the power domain: effective =
 * mse >= p_effective, or every frame when max(mse) >= p_all (power_to_db's top_db clamp); both thresholds come from the host's own
 * float32 log10 by bisection (realtime_yukarin_amd/gate.py), so the mask equals the host formula's bit for bit.  fft_length: a power
 * of two in 128 .. 1024.  ry_vc_wait_wave also returns the mask (n_frames bytes) and the count. */
int ry_vc_submit_wave(ry_vc* vc, const float* wave, int n_samples, int hop, int fft_length, float p_effective, float p_all,
                      const float* feat, int n_frames, float sp_floor, int* ticket);
int ry_vc_wait_wave(ry_vc* vc, int ticket, float* mc_out, float* sp_out, unsigned char* effective_out, int* n_eff_out);
/* The gate alone (`separate_effective`): mask [n_frames], count, and optionally the gathered rows x_eff [n_eff][in_ch] and their
 * frame indices row_of [n_eff] (null to skip). */
int ry_vc_gate(ry_vc* vc, const float* wave, int n_samples, int hop, int fft_length, float p_effective, float p_all,
               const float* feat, int n_frames, unsigned char* effective_out, int* n_eff_out, float* x_eff_out, int* row_of_out);
/* ry_vc_submit_wave for a wave and a feature block that are ALREADY ON THE CARD (what ry_crepe_track and ry_analysis_extract_resident left there),
 * with the results left there too: wave_dev [n_samples] float32 and feat_dev [n_frames][in_ch] are read in place (no staging, no H2D copy);
 * mc_out_dev [n_frames][M], sp_out_dev [n_frames][F] and mask_dev_out [n_frames] (bytes: 1 = effective) stay on the card (no mc / sp copy to the
 * host).  The call waits once, for the count (it picks the stage-1 plan), and returns it in *n_eff_out with the mask in effective_out [n_frames]
 * (host).  Ring slots, lanes and ry_vc_set_discard as ry_vc_enqueue_device (discarded rows of sp_out_dev are left untouched).  Order: the call
 * makes its stage-1 stream wait for what the CONTEXT stream holds at the time of the call -- inputs produced there (ry_crepe_track, the analysis)
 * need no wait by the caller, inputs produced on another stream must be complete (ry_sync) -- and makes the context stream wait for the end of
 * the window, so work enqueued on the context stream afterwards (ry_mask_rows, ry_synth_run / ry_synth_push with on_device = 1, ry_dev_download)
 * reads complete rows; a reader on another stream waits with ry_sync.  Refusals: those of ry_vc_submit_wave, and null outputs. */
int ry_vc_enqueue_wave_device(ry_vc* vc, const float* wave_dev, int n_samples, int hop, int fft_length, float p_effective, float p_all,
                              const float* feat_dev, int n_frames, float sp_floor, float* mc_out_dev, float* sp_out_dev,
                              unsigned char* mask_dev_out, unsigned char* effective_out, int* n_eff_out);
/* `combine_silent` for rows that stay where they are (the aperiodicity of a resident chain): rows k0 .. k1 - 1 of rows_dev [n][cols] (float32)
 * whose byte in mask_dev [n] is 0 become +0.0f in place; every other row keeps its bits.  Enqueue only, on `stream` (a HIP stream; null: the
 * context stream); nothing is waited for.  Refused: null pointers, n < 1, cols < 1, a range outside 0 <= k0 <= k1 <= n. */
int ry_mask_rows(ry_ctx* ctx, float* rows_dev, const unsigned char* mask_dev, int n, int cols, int k0, int k1, void* stream);
/* Rows picked by an index table, packed back to back: dst_dev [n_out][cols] row j = rows_dev [n_rows][cols] row src_row_dev[j] (an int table on the
 * card), or +0.0f where mask_dev [n_rows] (may be null: every row is kept) holds 0 for that source row -- `combine_silent` folded into the pick.
 * One launch packs the rows [front, n_b - back) of every stream of a call in the order ry_synth_bank_push (on_device = 1) reads them.  Source
 * and destination rows may start at any 4-byte alignment, independently; nothing outside a row is read or written; an index outside
 * 0 .. n_rows - 1 reads nothing and gives a row of zeros.  Source and destination must not overlap.  Enqueue only, on `stream` (null: the
 * context stream).  Refused: null pointers (the mask excepted), n_rows < 1, cols < 1, n_out < 0; n_out = 0 does nothing. */
int ry_gather_rows(ry_ctx* ctx, const float* rows_dev, int n_rows, int cols, const int* src_row_dev, const unsigned char* mask_dev, float* dst_dev,
                   int n_out, void* stream);
/* `separate_effective` of n_waves >= 1 waves that are on the card with ONE launch pair and ONE wait: wave i has the samples
 * [sample_offsets[i], sample_offsets[i + 1]) of wave_dev and the frames [frame_offsets[i], frame_offsets[i + 1]) of feat_dev [sum n][in_ch] (HOST
 * arrays of n_waves + 1 entries, starting at 0, ascending: what ry_crepe_track_many_buffers reports).  Frame powers: one wave of lanes per frame
 * over all waves, reflected at the ends of the frame's own wave; gate: one workgroup per wave, the maximum (the top_db clamp) over that wave's own
 * powers.  mask_dev_out (device) / effective_out (host) [sum n]: the masks in wave order; n_eff_out [n_waves]; x_eff_dev_out [sum n][in_ch] /
 * row_of_dev_out [sum n] (device; both null: blocks of the core): wave i's effective rows and their frame indices, counted from the wave's first
 * frame, from row frame_offsets[i] on.  Everything of wave i has the bits of ry_vc_gate on wave i alone.  The stage-1 stream waits for the context
 * stream first.  Refused, nothing launched: null pointers, n_waves < 1 or > 65536, offsets that do not start at 0 or do not ascend, hop < 1, an fft_length
 * ry_vc_gate refuses, more than 2^31 - 1 samples or 2^22 frames in all (the message names the wave). */
int ry_vc_gate_waves_device(ry_vc* vc, const float* wave_dev, const long long* sample_offsets, const int* frame_offsets, int n_waves, int hop,
                            int fft_length, float p_effective, float p_all, const float* feat_dev, unsigned char* mask_dev_out,
                            unsigned char* effective_out, int* n_eff_out, float* x_eff_dev_out, int* row_of_dev_out);
/* ry_vc_enqueue_wave_device for n_waves waves in ONE call: the one gate of ry_vc_gate_waves_device (one wait for all counts and masks), then,
 * wave by wave in order, the rest of the single call on that wave's rows: stage 1 under the plan its own count picks (none for a wave without an
 * effective frame), scatter, mc2sp, stage 2.  Ring slots and lanes are taken round robin as a sequence of single calls takes them; a slot that
 * comes round again within the call is ordered behind its previous window on the stream, so n_waves may exceed the ring.  feat_dev [sum n][in_ch],
 * mc_out_dev [sum n][M], sp_out_dev [sum n][F], mask_dev_out / effective_out [sum n], n_eff_out [n_waves]; ry_vc_set_discard applies to every
 * window (the discarded rows of each wave's part of sp_out_dev stay untouched).  mc, sp, mask and count of wave i have the bits of
 * ry_vc_enqueue_wave_device on wave i alone, whatever the other waves hold and wherever wave i stands.  Stream order as in the single call: the
 * gate waits for the context stream, the context stream waits for the end of every window before the call returns.  Refused, nothing launched:
 * what ry_vc_gate_waves_device refuses, null outputs, a ring slot of the call held by a ticket (RY_ESTATE).  That covers the arguments only: a
 * failure after the gate (a slot that cannot grow, a launch error) ends the call as it ends a sequence of single calls -- the windows queued so far
 * stay queued, the slots they took stay taken and the outputs are partly written. */
int ry_vc_enqueue_waves_device(ry_vc* vc, const float* wave_dev, const long long* sample_offsets, const int* frame_offsets, int n_waves, int hop,
                               int fft_length, float p_effective, float p_all, const float* feat_dev, float sp_floor, float* mc_out_dev,
                               float* sp_out_dev, unsigned char* mask_dev_out, unsigned char* effective_out, int* n_eff_out);
/* ---- gate before encode: the verdict first, the tracker and the analysis for the audible waves only, then the window call on that verdict.
 * The verdict of ry_vc_gate_waves_device alone, for waves whose feature rows do not exist yet: the same frame-power and gate launches and the same ONE
 * wait, with no feature row read and no feature row written (the gate kernel still writes the frame indices of the effective frames into the core's
 * own row_of block, which the compaction of the window call that follows overwrites in stream order).  mask_dev_out (device) / effective_out (host)
 * [sum n] and n_eff_out [n_waves] have the bits of ry_vc_gate_waves_device.  Refused, nothing launched: what that call refuses of the arguments this one has. */
int ry_vc_gate_verdict_waves_device(ry_vc* vc, const float* wave_dev, const long long* sample_offsets, const int* frame_offsets, int n_waves, int hop,
                                    int fft_length, float p_effective, float p_all, unsigned char* mask_dev_out, unsigned char* effective_out,
                                    int* n_eff_out);
/* The ordered compaction of the gate alone, from a verdict that exists: mask_dev [sum n] (device, the gate's mask), effective [sum n] and n_eff
 * [n_waves] (host, its copies), feat_dev [sum n][in_ch] -> x_eff_dev_out [sum n][in_ch] / row_of_dev_out [sum n] (device; both null: blocks of the
 * core): from row frame_offsets[i] on, the effective rows of wave i and their frame indices counted from the wave's first frame, with the bits and
 * the order ry_vc_gate_waves_device writes.  One workgroup per wave, a fixed order, no atomics.  The feature row of a frame whose mask byte is 0 is
 * not read and the rows behind n_eff[i] of a wave are not written: a wave with n_eff = 0 leaves its region as it was and its feature rows need not
 * exist.  The call waits for the kernel.  Refused (RY_EINVAL), nothing launched or written: null pointers (one output without the other),
 * n_waves < 1 or > 65536, offsets that do not start at 0 or do not ascend, more than 2^22 frames, n_eff[i] outside 0 .. frames of wave i, a host
 * mask whose ones in wave i are not n_eff[i] of them. */
int ry_vc_compact_waves_device(ry_vc* vc, const int* frame_offsets, int n_waves, const unsigned char* mask_dev, const unsigned char* effective,
                               const int* n_eff, const float* feat_dev, float* x_eff_dev_out, int* row_of_dev_out);
/* ry_vc_enqueue_waves_device with the verdict as an INPUT: the frame-power and gate kernels do not run and the call waits for nothing.  One
 * compaction launch (that of ry_vc_compact_waves_device, into the core's blocks; none when no wave has an effective frame), then, wave by wave in
 * order, the rest of ry_vc_enqueue_waves_device -- stage 1 only where n_eff[i] > 0, scatter, mc2sp, stage 2 -- with the same ring slots and
 * lanes.  mc and sp of wave i have the bits of ry_vc_enqueue_wave_device on wave i alone.  No feature row of a wave with n_eff = 0 is read.  Stream
 * order as there: the stage-1 streams wait for the context stream, the context stream waits for the end of every window.  Refused, nothing
 * launched or written: what ry_vc_compact_waves_device refuses, null outputs, a ring slot of the call held by a ticket (RY_ESTATE). */
int ry_vc_enqueue_waves_masked_device(ry_vc* vc, const int* frame_offsets, int n_waves, const float* feat_dev, float sp_floor, float* mc_out_dev,
                                      float* sp_out_dev, const unsigned char* mask_dev, const unsigned char* effective, const int* n_eff);
/* `AcousticConverter.decode_spectrogram` alone (host pointers): sp [n][bins] = exp(mc [n][m] @ mtx [m][bins]) + floor. */
int ry_mc2sp(ry_ctx* ctx, const float* mc, const float* mtx, int n, int m, int bins, float floor, float* sp);

/* ---- chunk parallelism over the GPUs of one node: one RCCL broadcast of each predictor's weight blob from rank 0
 * at start-up, no collective in the steady state; results are re-ordered by window index on the host exactly as run.py:171-183
 * re-orders its `Item.index`.  RCCL is bound at run time (dlopen of librccl.so.1, RY_RCCL_LIB overrides), so the library has no
 * link-time dependency on it and no tensor library is needed: rank 0 calls ry_comm_unique_id and hands the 128 bytes to the other
 * ranks by any host channel (a file, a socket, MPI, a torch.distributed store -- realtime_yukarin_amd/dist.py uses a file next to
 * MASTER_PORT), every rank calls ry_comm_init, ry_dev_alloc, (rank 0: ry_dev_upload,) ry_comm_bcast_weights and
 * ry_net_create(..., weights_on_device = 1). */
typedef struct ry_comm ry_comm;
#define RY_COMM_ID_BYTES 128
int ry_comm_unique_id(void* id128);                                   /* ncclGetUniqueId */
int ry_comm_init(ry_ctx* ctx, const void* id128, int rank, int world, ry_comm** out);   /* ncclCommInitRank on the context's GPU */
void ry_comm_destroy(ry_comm* comm);
int ry_comm_bcast_weights(ry_comm* comm, float* blob_dev, size_t n_floats, int root);  /* in place; returns when it has arrived */
int ry_comm_allreduce_max(ry_comm* comm, double* value);              /* max over the ranks (timing) */
int ry_comm_barrier(ry_comm* comm);
/* device buffers for callers without a tensor library */
int ry_dev_alloc(ry_ctx* ctx, size_t n_floats, float** out);
int ry_dev_free(ry_ctx* ctx, float* p);
int ry_dev_upload(ry_ctx* ctx, float* dst_dev, const float* src_host, size_t n_floats);
int ry_dev_download(ry_ctx* ctx, float* dst_host, const float* src_dev, size_t n_floats);

/* ---- measurement ---- */
int ry_timer_start(ry_ctx* ctx);              /* hipEventRecord on the context stream */
int ry_timer_stop(ry_ctx* ctx, float* ms);    /* record + synchronize + elapsed */

typedef struct ry_kernel_stat {
    char name[48];          /* kernel family as rocprofv3 prints it, e.g. "ry_igemm_ldsdma<96,128,1,4,2,false,1>" */
    char layer[24];         /* e.g. "encoder/c3" */
    float ms;               /* average duration over `reps` launches (hipEvents on the context stream) */
    double flops;           /* algorithmic FLOPs of this launch */
    double bytes;           /* algorithmic bytes: weights + input + output once */
    int grid[3];
    double flops_exec;      /* matrix-pipe FLOPs the launch executes: = flops, except 9 / 16 of it for the Winograd F(2x2, 2x2) kernels */
} ry_kernel_stat;
/* Runs the forward `reps` times launch by launch, bracketing every kernel with HIP events. */
int ry_net_profile(ry_net* net, int batch, int frames, int reps, ry_kernel_stat* stats, int max_stats, int* n_stats);
/* The same for the convert wrapper on ONE window of n_frames (what ry_ac_convert / ry_sr_convert / the ry_vc_* window call run:
 * pad kernel, layers, fused crop; stage 2 skips the decoder rows that only feed the padding the wrapper throws away). */
int ry_net_profile_window(ry_net* net, int n_frames, int reps, ry_kernel_stat* stats, int max_stats, int* n_stats);

/* diagnostics: ratio[i * n + j] = wall time of a `us`-microsecond spin kernel on each of two fresh streams i and j, divided by `us`:
 * ~1 when the two streams run side by side, ~2 when one waits for the other (scripts/gpu_queues.py). */
int ry_debug_stream_overlap(ry_ctx* ctx, int n, int us, float* ratio);

/* diagnostics / tests: read the process-wide RY_* environment switches again (otherwise read by ry_init).  Launch plans
 * that exist keep their choices until ry_net_set_dtype drops them. */
int ry_debug_reload_env(void);

/* diagnostics: the launch configuration the stage-2 planner picks for an implicit-GEMM layer with M output rows (pixels of
 * one sub-pixel phase), Cout output channels, `nphases` phases (4 for the k4s2 deconvolution, else 1) and K = 32 * nk:
 * tile code (see ry_conv2d), external split-K count, K groups per workgroup, estimated microseconds.  No device work. */
int ry_debug_plan_igemm(int M, int Cout, int nphases, int nk, int* tile, int* splits, int* kgroups, double* est_us);
/* the same for the bf16 (mode 1) / split-bf16 (mode 2) kernels (nk in 64-channel chunks; non-zero tile / splits / kgroups on entry are kept) */
int ry_debug_plan_igemm_bf16(int mode, int M, int Cout, int nphases, int nk, int* tile, int* splits, int* kgroups, double* est_us);

/* diagnostics: the slice the planner picks for an output-stationary layer (ry_c2d_os, round 5) with M rows per phase (batch x pixels), Cout
 * output channels, `nphases` phases and K = 64 * units: tile rows / 4, tile channels / 4, waves per workgroup, units in flight per wave, and the
 * slice cost (x units: what is compared with RY_OS2_MAXCOST to decide between this kernel and the implicit GEMM).  Non-zero values on entry
 * are kept.  Returns RY_EINVAL when no slice fits the shape.  No device work. */
int ry_debug_plan_os2(int M, int Cout, int nphases, int units, int* mt4, int* nt4, int* waves, int* depth, double* cost);

/* diagnostics: the plan the planner picks for a k4 s2 p1 stage-2 layer in Winograd F(2x2, 2x2) form (ry_wino_ldsdma, round 6) whose stencil output grid is
 * Mh x Mw pixels per phase and window, with Cout output channels, `nphases` phases (4: transposed convolution, 1: convolution), K = 16 * npatches input
 * channels (x 4 parities for a convolution: count them in npatches) and `batch` windows: workgroup shape (1 = 2 x 2 waves, 2 = 4 x 2 waves), M-blocks of
 * 8 x 16 pixels per tile row, external split-K.  Non-zero values on entry are kept.  Returns RY_EINVAL when no tile of a shape divides the grid (the layer
 * then stays on the direct implicit GEMM).  No device work. */
int ry_debug_plan_wino(int Mh, int Mw, int Cout, int nphases, int npatches, int batch, int* cfg, int* mbw, int* splits);

/* ---- CREPE pitch tracker (`crepe.predict(audio, 16000, viterbi=True, model_capacity=..., step_size=...)`, called by the reference's
 * CrepeAcousticFeatureWrapper.extract_f0, yukarin_wrapper/acoustic_feature_wrapper.py:65-80).  Semantics: INTEGRATION.md section 9.
 * `capacity` is the filter multiplier m: tiny 4, small 8, medium 16, large 24, full 32 (any 1 .. 32 is accepted).  Layer filters
 * [32, 4, 4, 4, 8, 16] x m, widths [512, 64 x 5], conv1 stride 4; conv -> ReLU -> BatchNorm -> max-pool 2; dense 360 + sigmoid.
 * Weight blob, per conv layer i = 1 .. 6: weight (Cout, Cin, width), bias, BN gamma, beta, running mean, running var (Cout each);
 * then classifier weight (360, 4 C6) (input index = position * C6 + channel) and bias (360). */
typedef struct ry_crepe ry_crepe;
size_t ry_crepe_param_count(int capacity);         /* 0 (and ry_last_error) for a bad capacity */
int ry_crepe_create(ry_ctx* ctx, int capacity, const float* weights, size_t n_floats, float bn_eps, ry_crepe** out);
void ry_crepe_destroy(ry_crepe* crepe);
/* The arithmetic of the seven GEMMs (conv1 .. conv6, dense), numbered as ry_net_set_dtype: 0 (default) fp32 MFMA; 2 split-bf16 -- every fp32
 * product x w runs as x_lo w_hi + x_hi w_lo + x_hi w_hi on the bf16 MFMA with fp32 accumulation (hi = bf16(v), lo = bf16(v - hi)): fp32-class
 * results (bars: INTEGRATION.md section 9), not the bits of mode 0.  Activations stay fp32 in memory; the filters are split into two bf16 planes
 * on the device at the first switch to 2 and kept until ry_crepe_destroy.  May be called between calls; back in 0 the results have the bits of a
 * handle that never switched.  Framing, resampling and the decode do not depend on it.  Refused (RY_EINVAL, the handle keeps its mode): 1 (there is
 * no plain bf16 form) and every other value. */
int ry_crepe_set_dtype(ry_crepe* crepe, int dtype);
/* audio16k: float32 samples at 16 kHz.  Frames: 1 + (n_samples + (center ? 1024 : 0) - 1024) / hop, each 1024 samples from
 * frame * hop - (center ? 512 : 0), mean / std normalised (std clamped at 1e-10).  f0 [frames] (Hz, 0 where the average is undefined),
 * confidence [frames] (max of the activation), activation [frames][360] (may be null).  viterbi = 1: the 360-state Viterbi path;
 * 0: the argmax of each frame.  on_device = 1: every pointer is a device pointer, the call only enqueues on the context stream. */
int ry_crepe_predict(ry_crepe* crepe, const float* audio16k, int n_samples, int hop, int center, int viterbi,
                     float* f0, float* confidence, float* activation, int on_device);
/* Audio at another rate.  The resampler is resampy's 'kaiser_best' interpolation, one device thread per 16 kHz sample, float64 sums in the
 * order of realtime_yukarin_amd.crepe.resample: the float32 result has that function's bits.  Two tables per input rate come from the caller:
 * win [n_win], the half filter (Kaiser window x sinc, num_table entries per zero crossing, scaled by 16000 / sr when sr > 16000; the
 * interpolation slope is taken as win[j + 1] - win[j]), walked in steps of `step` = int(min(1, 16000 / sr) * num_table) entries; and
 * time_register [n_times], the input time of every output: 0, then the running float64 sum of sr / 16000 (summed one by one: any other
 * order rounds differently).  The first call for a rate needs both; a later call may pass win = NULL and a longer time register only.
 * Several rates may be installed on one handle.  Refused: sr < 1, a time register that is negative, decreasing or not finite. */
int ry_crepe_set_resampler(ry_crepe* crepe, int sr, const double* win, int n_win, int num_table, int step,
                           const double* time_register, int n_times);
/* The resampler alone: n_samples at sr -> int(n_samples * (16000.0 / sr)) samples at 16 kHz in out16k (on_device = 1: both are device
 * pointers, the call only enqueues).  Refused before anything is launched: no tables for sr, a time register shorter than the output,
 * an empty output. */
int ry_crepe_resample(ry_crepe* crepe, const float* audio, int n_samples, int sr, float* out16k, int on_device);
/* ry_crepe_predict on audio at sr: resampled on the context stream into the handle's 16 kHz buffer, then exactly what ry_crepe_predict
 * runs on it (frames are counted on the resampled length).  sr = 16000 is ry_crepe_predict itself.  Refusals: those of
 * ry_crepe_resample and of ry_crepe_predict (center = 0 with fewer than 1024 resampled samples). */
int ry_crepe_predict_sr(ry_crepe* crepe, const float* audio, int n_samples, int sr, int hop, int center, int viterbi,
                        float* f0, float* confidence, float* activation, int on_device);
/* The decode alone on a host activation [n_frames][360]: f0, confidence and (may be null) the centre bin of every frame -- the Viterbi
 * path, or with viterbi = 0 the argmax. */
int ry_crepe_decode(ry_crepe* crepe, const float* activation, int n_frames, int viterbi, float* f0, float* confidence, int* path);
/* The float64 log tables of the Viterbi pass: logT [360][360] (from, to), logE [360][360] (state, observation), logS [360].
 * ry_crepe_create builds them with the C library's log; a caller whose decode must match its own restatement bit for bit uploads
 * that restatement's values (realtime_yukarin_amd/crepe.py uploads numpy's). */
int ry_crepe_set_viterbi_tables(ry_crepe* crepe, const double* logT, const double* logE, const double* logS);
/* The voicing of a track (`crepe.predict_voicing(confidence)` and the mask the reference's wrapper makes of it): confidence [n] and f0 [n] are the
 * float32 outputs of ry_crepe_predict / ry_crepe_predict_sr.  voiced [n] (0 / 1) = (path == 1) | (confidence > threshold), where path is the Viterbi
 * path of the two-state Gaussian HMM over the confidence (float64, the order of realtime_yukarin_amd.crepe.predict_voicing, no fma; the lowest state
 * wins a tie) and the comparison is strict and made in float32 against (float)threshold -- how numpy evaluates `confidence > 0.1` on a float32 array:
 * float32(0.1) itself is not above 0.1 --; f0_64 [n] = voiced ? (double)f0 : 0; t_64 [n] = k * step_ms / 1000 in float64, the
 * time axis of `crepe.predict`.  One workgroup, any n up to 2^24.  on_device = 1: all five are device pointers and the call only enqueues on the
 * context stream; 0: host pointers, the call returns after the results are written.  Refused: a null pointer, n < 1, a NaN threshold, a step that
 * is not finite and positive. */
int ry_crepe_voicing(ry_crepe* crepe, const float* confidence, const float* f0, int n, double threshold, double step_ms,
                     unsigned char* voiced, double* f0_64, double* t_64, int on_device);
/* The constants of that HMM, two states each (1 = voiced): c = log(2 pi var), the means, the variances, logT [2][2] (from, to) and the log of the
 * start probabilities.  ry_crepe_create installs the values of `predict_voicing` with the C library's log; a caller whose mask must match its own
 * restatement bit for bit uploads that restatement's values (realtime_yukarin_amd/crepe.py uploads numpy's).  The device never takes a logarithm. */
int ry_crepe_set_voicing_tables(ry_crepe* crepe, const double* c, const double* mu, const double* var, const double* logT, const double* logS);
/* One enqueue for a window: audio (HOST, float32, at sr; uploaded once) -> ry_crepe_predict_sr with center = 1, viterbi = 1 and no activation
 * output -> ry_crepe_voicing on its confidence and f0, all on the context stream.  *n_frames: the frames of the call.  The masked track stays in
 * buffers of the handle (ry_crepe_track_buffers).  on_device_out = 0: voiced / f0_64 / t_64 are host arrays of at least *n_frames entries, written
 * before the call returns; 1: they are not read (may be null), nothing is copied back and the call does not wait.  Refusals: those of
 * ry_crepe_predict_sr and of ry_crepe_voicing. */
int ry_crepe_track(ry_crepe* crepe, const float* audio, int n_samples, int sr, int hop, double step_ms, double threshold, int* n_frames,
                   unsigned char* voiced, double* f0_64, double* t_64, int on_device_out);
/* What the last ry_crepe_track left on the card, as device addresses (any pointer may be null): the uploaded float32 wave at the caller's rate and
 * its length, the frames, voiced [n] (bytes), f0_64 [n], t_64 [n].  They are read in stream order (ry_analysis_extract_dev on the same context) and
 * hold until the next call on this handle.  RY_ESTATE when no track is there: none has run, or a later call has reused the buffers. */
int ry_crepe_track_buffers(ry_crepe* crepe, const float** wave_dev, int* n_samples, int* n_frames, const unsigned char** voiced_dev,
                           const double** f0_dev, const double** t_dev);
/* ry_crepe_track for n_waves >= 1 waves at one rate in ONE enqueue.  audio (HOST, float32): the waves back to back, wave i of n_samples[i] samples;
 * they are uploaded once, with one segment table (per wave: first sample and length at sr, the same at 16 kHz, first frame and frame count).  The
 * resampler runs over all waves in one launch -- an output indexes the rate's time register by its index within its wave and reads that wave's samples
 * only --; the frames of all waves are packed back to back into the network's passes of 256, each frame centred and padded inside its own wave; the
 * Viterbi decode and the voicing run one workgroup per wave, each from its own first frame, the time axis counted from it.  Everything written for wave i
 * has the bits ry_crepe_track writes for wave i alone, in both modes of ry_crepe_set_dtype, whatever the other waves hold and wherever it stands in
 * the list.  n_frames [n_waves]: the frames of every wave.  The masked tracks stay in the handle, concatenated in wave order
 * (ry_crepe_track_many_buffers); on_device_out = 0: voiced / f0_64 / t_64 are host arrays of the sum of n_frames entries, written before the call
 * returns; 1: as in ry_crepe_track.  Refused before anything is launched or written (n_frames included): n_waves < 1, a wave with no sample, a wave
 * ry_crepe_track refuses (no sample at 16 kHz, a time register too short, ...), a rate without resampler tables (RY_ESTATE), more than 2^24 frames
 * or 2^31 - 1 samples (at sr or at 16 kHz) in all, and what ry_crepe_voicing refuses. */
int ry_crepe_track_many(ry_crepe* crepe, const float* audio, const int* n_samples, int n_waves, int sr, int hop, double step_ms, double threshold,
                        int* n_frames, unsigned char* voiced, double* f0_64, double* t_64, int on_device_out);
/* What the last ry_crepe_track_many left on the card (any pointer may be null): the device addresses of the uploaded float32 waves (back to back, at
 * the caller's rate) and of the concatenated voiced (bytes), f0_64 and t_64; the number of waves; and two HOST arrays of n_waves + 1 entries that
 * belong to the handle: sample_offsets[i] / frame_offsets[i] = the first sample / first frame of wave i, the last entry the total -- what
 * ry_analysis_extract_many_dev takes.  All hold until the next call on this handle.  RY_ESTATE when no such tracks are there: none has run, or a later
 * call (ry_crepe_track included) has reused the buffers; ry_crepe_track_buffers in turn reports no track after ry_crepe_track_many.  Unlike
 * ry_crepe_track, which looks at its arguments first, ry_crepe_track_many forgets the tracks before it validates anything: after ANY refused
 * ry_crepe_track_many, a null argument included, no track is reported. */
int ry_crepe_track_many_buffers(ry_crepe* crepe, const float** wave_dev, int* n_waves, const long long** sample_offsets, const int** frame_offsets,
                                const unsigned char** voiced_dev, const double** f0_dev, const double** t_dev);
/* ry_crepe_track_many in two steps, for a caller that decides between them which waves are worth tracking (the silence gate of the window call).
 * ry_crepe_upload_waves: the ONE upload -- n_waves >= 1 float32 waves back to back at sr, n_samples[i] each -> *wave_dev, their device address;
 * wave i starts at the sum of the counts in front of it.  The table holds until the next call on this handle that is not one of the two tracking
 * calls below; those may follow each other on one table.  Refused, nothing written: null pointers, n_waves < 1, a wave with no sample, a wave
 * ry_crepe_track refuses at this rate, a rate without resampler tables (RY_ESTATE), more than 2^31 - 1 samples in all.
 * ry_crepe_track_uploaded: ry_crepe_track_many on n_waves >= 1 waves OF THAT TABLE, read where they lie: first_sample[i] / n_samples[i] name wave
 * i's first sample in the table and its length.  The same segment table, passes of 256 frames and decode / voicing workgroup per wave: the tracked
 * waves get the bits of ry_crepe_track_many on them alone.  The masked tracks stay in the handle, back to back in the order of the call
 * (ry_crepe_uploaded_buffers; ry_crepe_track_many_buffers reports no track).  Refused before anything is launched or written: what
 * ry_crepe_track_many refuses, no table on the card (RY_ESTATE), another rate than the upload's, an entry that is not a wave of the table (first
 * sample and length), entries that do not ascend.
 * ry_crepe_uploaded_buffers (any pointer may be null): the table's address and samples, the waves the last tracking call tracked (0: none since
 * the upload), a HOST array of n_tracked + 1 frame offsets that belongs to the handle, and the addresses of voiced / f0_64 / t_64.  RY_ESTATE
 * without a table. */
int ry_crepe_upload_waves(ry_crepe* crepe, const float* audio, const int* n_samples, int n_waves, int sr, const float** wave_dev);
int ry_crepe_track_uploaded(ry_crepe* crepe, const int* first_sample, const int* n_samples, int n_waves, int sr, int hop, double step_ms,
                            double threshold, int* n_frames, unsigned char* voiced, double* f0_64, double* t_64, int on_device_out);
int ry_crepe_uploaded_buffers(ry_crepe* crepe, const float** wave_dev, long long* n_samples, int* n_tracked, const int** frame_offsets,
                              const unsigned char** voiced_dev, const double** f0_dev, const double** t_dev);
/* tests: how many frames have gone through the network on this handle so far (every pass of every call, streams and banks over it included) */
int ry_crepe_debug_frames(ry_crepe* crepe, long long* n_frames);
/* ry_crepe_decode / ry_crepe_voicing on n_tracks >= 1 tracks side by side, one workgroup each: the arrays hold the tracks back to back, track i of
 * n_frames[i] >= 1 frames (at most 2^24 in all); every track gets the bits of the single call on it alone.  Pointers and on_device as in the single
 * calls. */
int ry_crepe_decode_many(ry_crepe* crepe, const float* activation, const int* n_frames, int n_tracks, int viterbi, float* f0, float* confidence, int* path);
int ry_crepe_voicing_many(ry_crepe* crepe, const float* confidence, const float* f0, const int* n_frames, int n_tracks, double threshold, double step_ms,
                          unsigned char* voiced, double* f0_64, double* t_64, int on_device);
/* tests: the first n_frames rows of the buffers of the last pass of ry_crepe_predict (its last <= 256 frames): layer 0 the normalised
 * frames [n][1024], 1 .. 6 the pooled conv outputs [n][positions][channels], 7 the logits [n][360].  n_frames may exceed the frames of
 * that pass, up to the largest pass the handle has run: the rows behind it hold what an earlier call or ry_crepe_debug_poison left. */
int ry_crepe_debug_layer(ry_crepe* crepe, int layer, int n_frames, float* out);
/* tests: fills every element the next ry_crepe_predict / ry_crepe_decode / ry_crepe_voicing / ry_crepe_track (and their _many forms) must write with NaN bit patterns (all
 * bits set; -1 as an index) -- the samples of the frame rows, the interior rows of every layer's input, logits, split-K slabs, activation, confidence,
 * f0, observations, back-pointers, path, the 16 kHz audio buffer (the resampler's output), the voicing's back-pointers and the masked track (voiced,
 * f0_64, t_64; ry_crepe_track_buffers and ry_crepe_track_many_buffers then report no track) and the segment table -- and leaves the zero padding rows as they are: a later call that reads anything it did not write shows it. */
int ry_crepe_debug_poison(ry_crepe* crepe);
/* diagnostics: the split-K count of conv1 .. conv6 and the dense layer (7 ints) in the mode in force (ry_crepe_set_dtype). */
int ry_crepe_debug_splits(ry_crepe* crepe, int* splits);
/* ---- A streaming tracker: ry_crepe_track window by window, with the activation rows of the frames two consecutive windows share taken from the
 * previous call instead of being run through the network again (DESIGN.md section 18 states which rows).  A stream belongs to the model it was
 * created from and is destroyed before it; a model serves any number of streams.  What a stream keeps (two activation blocks used in turn, the
 * packed rows of the computed frames, two index tables) is its own: no call on the model, ry_crepe_debug_poison included, touches it. */
typedef struct ry_crepe_stream ry_crepe_stream;
int ry_crepe_stream_create(ry_crepe* crepe, ry_crepe_stream** out);
void ry_crepe_stream_destroy(ry_crepe_stream* stream);
/* forgets the kept rows: the next call computes every frame */
int ry_crepe_stream_reset(ry_crepe_stream* stream);
/* ry_crepe_track on a window of a live signal.  advance >= 0 and overlap_ok = 1: the caller declares that sample i of this window is sample
 * i + advance of the previous window of this stream, and has verified it on the bit patterns of the overlap (the first
 * min(n_samples, previous n_samples - advance) samples).  Rows are then kept when the advance is a whole number of 16 kHz samples and of hops,
 * the rate's time register repeats exactly under it, and rate, hop, ry_crepe_set_dtype mode and filter table are those of the previous call: frame j
 * takes the row of previous frame j + advance16 / hop when both are portable (their 1024 samples lie inside the signal, untouched by centre padding
 * and by a resampler tap cut at an end of the signal).  Every other frame -- and with advance < 0 or overlap_ok = 0 every frame -- is computed;
 * the rows are kept for the next call either way.  voiced / f0_64 / t_64, the masked track, the uploaded wave and what ry_crepe_track_buffers
 * reports are bit for bit those of ry_crepe_track on the same window, whatever was kept.  *n_computed: the frames that went through the network.
 * Refusals: those of ry_crepe_track and a null n_computed, made before anything is launched or written; a refused call leaves the kept rows as they
 * were. */
int ry_crepe_stream_track(ry_crepe_stream* stream, const float* audio, int n_samples, int sr, int hop, double step_ms, double threshold, int advance,
                          int overlap_ok, int* n_frames, int* n_computed, unsigned char* voiced, double* f0_64, double* t_64, int on_device_out);
/* the activation [n_frames][360] of the last ry_crepe_stream_track as it was assembled (host array, or on_device = 1 a device pointer);
 * RY_ESTATE when the stream holds no window */
int ry_crepe_stream_activation(ry_crepe_stream* stream, float* out, int on_device);
/* tests: NaN bit patterns in the packed block, the tables on the card, the block the next call writes and every row of the kept block that is not
 * portable -- everything but the rows the rule may hand to the next call.  *rows_left: the rows left alone. */
int ry_crepe_stream_debug_poison(ry_crepe_stream* stream, int* rows_left);
/* tests: the assembling kernel alone.  Row j of out_dev [n_rows][360] becomes row src[j] of keep_dev [n_keep][360] when src[j] >= 0, else row
 * -1 - src[j] of fresh_dev [n_fresh][360]; a row whose source index lies outside its block is left as it is.  src is a host array; the blocks are
 * device pointers, 16-byte aligned.  Waits for the stream. */
int ry_crepe_stream_debug_assemble(ry_crepe_stream* stream, const float* keep_dev, int n_keep, const float* fresh_dev, int n_fresh, const int* src,
                                   int n_rows, float* out_dev);
/* ---- A bank of streaming trackers: ry_crepe_track_many on the next windows of several live streams, each wave under the rule of
 * ry_crepe_stream_track against the kept call of its own stream.  A bank belongs to the model it was created from and is
 * destroyed before it.  Every stream has a pair of activation slots of its own, used in turn by the calls it takes part in, so a stream that sits
 * calls out finds its rows intact; the packed rows of the computed frames and two sets of tables belong to the bank.  None of it is on the model's
 * buffer list: no call on the model, ry_crepe_debug_poison included, touches it, and streams and banks of one model do not disturb each other. */
typedef struct ry_crepe_bank ry_crepe_bank;
int ry_crepe_bank_create(ry_crepe* crepe, int n_streams, ry_crepe_bank** out);
void ry_crepe_bank_destroy(ry_crepe_bank* bank);
/* forgets the kept rows of one stream, or with stream = -1 of every stream */
int ry_crepe_bank_reset(ry_crepe_bank* bank, int stream);
/* ry_crepe_track_many on n_waves waves (audio: the waves back to back, n_samples[i] each), wave i being the next window of stream stream_of[i]:
 * advance[i] / overlap_ok[i] are what ry_crepe_stream_track takes for it, n_computed[i] the frames of wave i that went through the network.  One
 * upload of the audio, one segment table, one resample launch, the computed frames of all waves packed into the passes of the network, one launch
 * that assembles every wave's block, one Viterbi and one voicing workgroup per wave.  Everything written for wave i has the bits of ry_crepe_track on
 * it alone, and the track is left on the card as ry_crepe_track_many leaves it (ry_crepe_track_many_buffers, ry_analysis_extract_many_resident).
 * The tables go up in one copy, and only when the card holds them in neither of its two sets.
 * Refusals, made before anything is launched or written (a refused call leaves every stream's kept rows as they were and no track reported): those
 * of ry_crepe_track_many, a stream_of entry outside [0, n_streams), a stream named twice, a null stream_of, advance, overlap_ok or n_computed. */
int ry_crepe_bank_track(ry_crepe_bank* bank, const float* audio, const int* n_samples, const int* stream_of, int n_waves, int sr, int hop, double step_ms,
                        double threshold, const int* advance, const int* overlap_ok, int* n_frames, int* n_computed, unsigned char* voiced,
                        double* f0_64, double* t_64, int on_device_out);
/* ry_crepe_bank_track on waves of the table ry_crepe_upload_waves left on the bank's model (first_sample[i] / n_samples[i] as in
 * ry_crepe_track_uploaded): nothing is uploaded but the tables; a stream whose wave of the table is not named sits the call out and keeps its rows.
 * The same bits, the track reported by ry_crepe_uploaded_buffers.  Refusals: those of ry_crepe_bank_track and of ry_crepe_track_uploaded. */
int ry_crepe_bank_track_uploaded(ry_crepe_bank* bank, const int* first_sample, const int* n_samples, const int* stream_of, int n_waves, int sr, int hop,
                                 double step_ms, double threshold, const int* advance, const int* overlap_ok, int* n_frames, int* n_computed,
                                 unsigned char* voiced, double* f0_64, double* t_64, int on_device_out);
/* the activation [n_frames][360] of the last window of `stream` as it was assembled (host array, or on_device = 1 a device pointer); RY_ESTATE when
 * the stream holds none */
int ry_crepe_bank_activation(ry_crepe_bank* bank, int stream, float* out, int on_device);
/* tests: NaN bit patterns in the packed block, both sets of tables, the slot every stream writes next and every row of every kept slot that is not
 * portable.  rows_left [n_streams]: the rows of each stream left alone. */
int ry_crepe_bank_debug_poison(ry_crepe_bank* bank, int* rows_left);
/* tests: how many times ry_crepe_bank_track has uploaded its tables so far */
int ry_crepe_bank_debug_uploads(ry_crepe_bank* bank, long long* n_uploads);
/* tests: the assembling kernel alone on n_waves waves of n_frames[i] rows.  Row j of wave i (row frame0_i + j of out_dev) becomes row src of
 * keep_dev[i] [n_keep[i]][360] when src >= 0, else row -1 - src of fresh_dev [n_fresh][360], and is written to row j of write_dev[i] as well; a row
 * whose source index lies outside its block is left as it is in both.  n_frames, keep_dev, n_keep, write_dev and src (one entry per row of the call)
 * are host arrays; the blocks are device pointers, 16-byte aligned (keep_dev[i] may be null when n_keep[i] is 0).  Waits for the stream. */
int ry_crepe_bank_debug_assemble(ry_crepe_bank* bank, const int* n_frames, int n_waves, const float* const* keep_dev, const int* n_keep,
                                 float* const* write_dev, const float* fresh_dev, int n_fresh, const int* src, float* out_dev);
/* tests (the predictors' counterpart of ry_crepe_debug_layer): one buffer of the launch plan that ran last on this handle (ry_net_forward, ry_ac_convert,
 * ry_sr_convert, ry_sr_convert_rows), copied to the host once its stream has drained.  layer -1, kind 0: the convert wrapper's padded input
 * [batch][T][cols] (stage 1: in_ch columns; stage 2: log of the spectrogram without its last bin, width columns).  layer 0 .. 15 (stage 2), kind 0:
 * that layer's fp32 output [batch][Ho][Wo][Cout]; kind 1: its 16-bit copy as raw uint16, plain bf16 [pixel][Cout] or split-bf16 [pixel][hi (Cout) |
 * lo (Cout)].  Rows a cropped window did not compute hold what the allocation (RY_POISON=1: NaN patterns) or an earlier run left.
 * dims[5] = batch, rows, columns, elements per pixel, format (0 fp32, 1 bf16, 2 split-bf16); out = NULL returns the dims alone, else out_bytes must
 * be the block's exact size.  RY_EINVAL when the plan has no such buffer or nothing wrote it: a copy no consumer reads, the last layer when it stores
 * into the caller's block (the raw forward; the fused 3x3 end layer of a convert), the padded input of a raw forward or of a stage-1 window whose
 * first layer pads for itself.  Adds nothing to the forward / convert path: the handle only remembers which plan ran. */
int ry_net_debug_activation(ry_net* net, int layer, int kind, void* out, size_t out_bytes, int* dims);

/* tests: what the stage-2 planner decided for one layer of a (batch, frames) launch plan, and the rows one enqueue of it computes.  Zeros where a
 * field does not apply to the layer's path. */
typedef struct ry_plan_record {
    int layer;                  /* 0 .. 15 */
    int path;                   /* 1 implicit GEMM, 2 direct, 3 first layer, 4 fused end layer, 5 16-bit implicit GEMM, 7 output-stationary, 8 Winograd */
    int tile;                   /* implicit GEMM: 1 128x128, 3 64x128, 4 32x128, 5 128x64, 6 96x128 */
    int splits, kgroups;        /* external split-K, K groups per workgroup */
    int wino_cfg, wino_mbw;     /* Winograd: workgroup shape (1: 2 x 2 waves, 2: 4 x 2), M-blocks per tile row */
    int os2[4];                 /* output-stationary: mt4, nt4, waves, depth */
    int reads16;                /* sources: 0 fp32, 1 the producers' bf16 copies, 2 their split-bf16 copies */
    int writes32, writes16;     /* copies of the output: fp32 (0 / 1); 16-bit (0 none, 1 bf16, 2 split-bf16) */
    int patch;                  /* implicit GEMM: input-patch variant of the kernel (0 none, 1 deconvolution, 2 k4 s2 p1 convolution) */
    int reduce;                 /* node behind an external split: 0 none, 1 ry_splitk_reduce, 2 ry_splitk_reduce_wide */
    int last_exp;               /* fused end layer: exp / edge bin / crop of the convert wrapper */
    int rows_out;               /* output rows of the layer (per window) */
    int grid_rows, grid_cols;   /* rows and columns of the whole pixel grid the launch tiles (a deconvolution: its input pixels) */
    int tile_rows, tile_cols;   /* 2-D pixel tile of the launch; 0: raster tiles or no GEMM grid */
    int out_lo, out_n;          /* output rows [out_lo, out_lo + out_n) the launch computes (the dead-row crop; the end layer: the kept frames) */
    int crop_lo, crop_n;        /* the same as grid rows; crop_n = 0: the launch runs whole */
    int hole_lo, hole_n;        /* output rows the launch leaves out and ry_rep_rows copies from row hole_lo - 1; hole_n = 0: none */
} ry_plan_record;
/* tests (the planner's counterpart of ry_net_debug_activation): the launch plan of (batch, frames) of a stage-2 predictor, built if it does not
 * exist yet, one record per layer; nothing is enqueued and nothing is added to the forward / convert path.  window = 1: the convert wrapper on
 * `frames` real frames per window, for a caller that throws away discard_front / discard_back of them (ry_sr_convert_rows); window = 0: the raw
 * forward at `frames` padded rows (the discards must be 0).  *n = records written (16); RY_EINVAL when max is smaller. */
int ry_net_debug_plan(ry_net* net, int batch, int frames, int window, int discard_front, int discard_back, ry_plan_record* records, int max, int* n);

/* ---- where the filter layouts of a predictor are built.  Process-wide.  0 = host, the default:
 * ry_net_create lays every filter out in host loops and uploads each layout; the Winograd filters of a layer are read back from the card,
 * transformed on the host and uploaded when the first launch plan takes the layer onto that path.  1 = device: the raw filter of a layer is uploaded
 * once and kernels write every layout (same allocations, same bits); the Winograd transform is one launch, without a download.  Also set by the
 * environment variable RY_FILTER_BUILD=host|device, read by ry_init and ry_debug_reload_env; an absent variable leaves the mode as it is.  Any other
 * mode number / value: RY_EINVAL, the mode stays as it was.  Predictors that exist keep their filters; the mode applies to what is built next (the
 * filters ry_net_create builds, a lazy Winograd build, the single operators). */
int ry_set_filter_build(int mode);
typedef struct ry_build_stats {
    unsigned long long bytes_uploaded;        /* host -> card copies into the predictor's filter arena (raw filters or layouts, scale / shift, 16-bit copies) */
    unsigned long long bytes_downloaded;      /* card -> host copies the build made (host mode: the direct layout for the Winograd transform; ry_net_set_dtype) */
    unsigned long long layout_launches;       /* layout kernels launched (device mode: one per layout built) */
    unsigned long long host_relayout_floats;  /* floats of the layouts that host loops wrote (host mode) */
    unsigned long long arena_bytes;           /* bytes allocated in the filter arena so far */
} ry_build_stats;
/* What building the filters of this predictor has taken so far.  The counters belong to the filter arena, which the clones of a predictor share
 * (ry_net_clone): every handle reports the same totals, and they go on counting across lazy builds. */
int ry_net_build_stats(ry_net* net, ry_build_stats* out);
/* tests: one filter layout of predictor layer 0 .. 15, copied to the host.  kind: 0 w1d, 1 w1os (stage 1), 2 wig (implicit GEMM), 3 wdir (direct),
 * 4 w2os (output-stationary), 5 wwin (Winograd; built on demand in the mode in force, as a launch plan would).  *n_floats = the layout's size.
 * RY_ESTATE: the layer has no such layout.  RY_EINVAL: bad layer / kind, or out_floats < the size (*n_floats is set: out = NULL, out_floats = 0 asks
 * for the size).  A refused call writes nothing to out and builds nothing. */
int ry_net_debug_filters(ry_net* net, int layer, int kind, float* out, size_t out_floats, size_t* n_floats);
/* tests: the same for one layer of any shape outside a predictor: the layer's filters are built from the raw Chainer filter W (HOST; conv (Cout, Cin, k[, k]),
 * transposed (Cin, Cout, 4[, 4]), Cin = cin_a + cin_b for two skip sources) in the mode in force, into memory of the call, and layout `kind` comes back.
 * ndim 1 / 2; k <= 4; transposed: k4 s2 p1 only; want_os2: build the output-stationary layout whatever the filter's size.  Refusals as above. */
int ry_debug_layer_filters(ry_ctx* ctx, int ndim, int cin_a, int cin_b, int cout, int k, int stride, int pad, int transposed, int want_os2,
                           const float* W, int kind, float* out, size_t out_floats, size_t* n_floats);

/* ---- WORLD synthesizer (`pyworld.synthesize(f0, sp, ap, fs, frame_period)` in the reference's Vocoder.decode and world4py's realtime
 * synthesizer in RealtimeVocoder.decode, yukarin_wrapper/vocoder.py:50-120).  Semantics: INTEGRATION.md section 10 and
 * tests/world_synth_ref.py (WORLD's Synthesis restated; counter-based noise of `seed`, phase wrapped at every step).
 * fft_size: 1024 (CheapTrick's size at 16 and 24 kHz) -- anything else is refused.  Frames: f0 [n_frames] float64 on the HOST (Hz; below
 * fs / fft_size + 1 = unvoiced), sp / ap [n_frames][bins] float32 with bins = fft_size / 2 + 1, host pointers or, with on_device = 1, device
 * pointers on the context's GPU (the rows stage 2 leaves there).  y: float64 samples on the HOST; every call returns after its samples are
 * in y.  Domain: 8000 <= fs <= 48000, fs * frame_period_ms / 1000 >= 1 (a frame is at least one sample), f0 finite and below fs / 2 (negative:
 * unvoiced).  Refused: a rate or a frame period outside that, n_frames < 1, bins != fft_size / 2 + 1, a y too small, f0 that is not finite or
 * not below fs / 2 (a phase step of 2 pi or more per sample has no pulse train). */
typedef struct ry_synth ry_synth;
int ry_synth_create(ry_ctx* ctx, int fs, double frame_period_ms, int fft_size, unsigned seed, ry_synth** out);
void ry_synth_destroy(ry_synth* synth);
/* samples of a signal of n_frames frames: int((n_frames - 1) * frame_period / 1000 * fs) + 1 (negative: error) */
int ry_synth_length(ry_synth* synth, int n_frames);
/* One shot: the whole signal (ry_synth_length samples).  Drops a stream in progress. */
int ry_synth_run(ry_synth* synth, const double* f0, const float* sp, const float* ap, int n_frames, int bins, int on_device,
                 double* y, int y_capacity, int* n_out);
/* Stream: after pushes of N1, N2, ... frames and a flush the concatenated output equals ry_synth_run on the concatenated frames bit for
 * bit, for any cut.  A push returns only samples that can no longer change -- every pulse within fft_size / 2 behind them has a successor,
 * and the frame after the last pushed one is not needed -- so the output lags the input by about fft_size / 2 samples + one frame + one
 * pulse period.  y must hold what the call MAY return: ry_synth_bound(synth, n_frames, final) samples (n_frames about to be pushed; final = 1:
 * for the flush after them).  ry_synth_flush ends the signal with the frames pushed so far and resets the stream. */
int ry_synth_bound(ry_synth* synth, int n_frames, int final);
int ry_synth_push(ry_synth* synth, const double* f0, const float* sp, const float* ap, int n_frames, int bins, int on_device,
                  double* y, int y_capacity, int* n_out);
int ry_synth_flush(ry_synth* synth, double* y, int y_capacity, int* n_out);
/* The same two calls with the samples left on the card: y_dev is a DEVICE pointer of the caller's with room for y_capacity samples (the rule of
 * ry_synth_bound), and the overlap-add kernel writes the *n_out emitted samples straight to y_dev[0 .. *n_out) -- one 8-byte store per sample,
 * so any double-aligned address will do, e.g. y_dev + k behind the k samples of the push before, and no byte outside that range is written.
 * Nothing is staged, copied or brought down, and the call does not wait for that launch: it is enqueued on the context stream, where a reader
 * (ry_outgate_push with on_device = 1) finds the samples in order.  *n_out is known on the host when the call returns.  The bits are those of
 * ry_synth_push / ry_synth_flush; so are the refusals, in the same order (a null y_dev among the bad output arguments), each before anything is
 * launched or any carried state changes.  ry_synth_flush_dev resets the stream in stream order, without the wait of ry_synth_reset.
 * DESIGN.md section 24, INTEGRATION.md section 22. */
int ry_synth_push_dev(ry_synth* synth, const double* f0, const float* sp, const float* ap, int n_frames, int bins, int on_device,
                      double* y_dev, long long y_capacity, long long* n_out);
int ry_synth_flush_dev(ry_synth* synth, double* y_dev, long long y_capacity, long long* n_out);
int ry_synth_reset(ry_synth* synth);
/* One shot, many waves: wave b has n_frames[b] frames; f0 (HOST), sp and ap (rows on the host, or with on_device on the card, read where
 * they are) hold the waves back to back.  y receives the waves back to back, wave b at y[sample_offsets[b]] with
 * sample_offsets[b + 1] - sample_offsets[b] = ry_synth_length(n_frames[b]) samples; sample_offsets has n_waves + 1 entries.  Every wave has the
 * bits of ry_synth_run on it alone.  Drops a stream in progress and leaves the stream reset.  Refused before anything is launched or written
 * (y and sample_offsets untouched): null pointers, n_waves < 1, a wave without a frame, bins != 513, f0 that ry_synth_run refuses (the message
 * names wave and frame), y_capacity below the total, more than 2^22 frames or 2^30 - n_waves samples in all.  INTEGRATION.md section 10. */
int ry_synth_run_many(ry_synth* synth, const double* f0, const float* sp, const float* ap, const int* n_frames, int n_waves, int bins,
                      int on_device, double* y, long long y_capacity, long long* sample_offsets);
/* tests: the pulses the last run / push / flush found: sample index, fractional shift in samples [0, 1), voiced flag.  All three arrays
 * null: the count alone.  After ry_synth_run_many: none (count 0) -- its pulse lists stay on the card, see ry_synth_debug_pulses_many. */
int ry_synth_debug_pulses(ry_synth* synth, long long* index, double* shift, int* voiced, int capacity, int* n);
/* tests: the same for wave `wave` of the last ry_synth_run_many, indices counted from the wave's first sample (read from the card here).
 * RY_ESTATE when the last call was another one or ry_synth_debug_poison has run since. */
int ry_synth_debug_pulses_many(ry_synth* synth, int wave, long long* index, double* shift, int* voiced, int capacity, int* n);
/* tests: fills every scratch buffer and the unused part of the frame window with NaN bit patterns: a later call that reads anything it
 * did not write shows it in its output. */
int ry_synth_debug_poison(ry_synth* synth);

/* ---- A bank of WORLD synthesis streams: B independent streams at one rate and one frame period, each with a seed of its own, advanced by ONE
 * device call per buffer (the realtime decode of a process that serves B sessions).  Contract, without a tolerance: for every stream b and every
 * call, the samples returned for b and the pulses found for b equal, bit for bit, those of a lone ry_synth handle with seed seeds[b] that
 * received the same frames in the same cuts through ry_synth_push / ry_synth_flush -- whatever the other streams do in the same call (their
 * frame counts, sitting out, ending, restarting, their values and seeds).  All carried state -- phase, pulse lists, frame windows -- lives on
 * the card; the cost of a push (two stream waits, five kernel launches, a fixed number of copies) does not depend on B.  Frames, y and the
 * domain: as ry_synth_*.  INTEGRATION.md section 10, DESIGN.md section 12.2. */
typedef struct ry_synth_bank ry_synth_bank;
/* seeds [n_streams]; the domain and the refusals of ry_synth_create, and n_streams >= 1 */
int ry_synth_bank_create(ry_ctx* ctx, int fs, double frame_period_ms, int fft_size, int n_streams, const unsigned* seeds, ry_synth_bank** out);
void ry_synth_bank_destroy(ry_synth_bank* bank);
/* samples a push may return for `stream` (n_frames about to be pushed; final = 1: its signal ends with them), as ry_synth_bound */
int ry_synth_bank_bound(ry_synth_bank* bank, int stream, int n_frames, int final);
/* One call for all streams.  n_frames [n_streams] >= 0: 0 = the stream sits the call out.  final (may be null) [n_streams]: 1 = the stream's
 * signal ends with these frames -- everything left is returned and the slot is a new stream from the next call on (ry_synth_flush; with no
 * frames a plain flush; RY_ESTATE on a stream without a frame).  f0 (HOST), sp and ap (host rows, or with on_device rows on the card, read where
 * they are) hold the streams' new frames back to back in stream order.  y receives stream b's samples at y[sample_offsets[b]], sample_offsets
 * has n_streams + 1 entries; y must hold the sum of ry_synth_bank_bound over the streams that take part.  Refused before anything is launched,
 * uploaded or changed (y and sample_offsets untouched, the bank continues as if the call had not been made): null pointers, a negative count,
 * no stream with a frame or final, bins != 513, f0 that ry_synth_push refuses (the message names stream and frame), y_capacity below the sum of
 * the bounds, more than 2^22 frames or 2^30 pulse entries in all. */
int ry_synth_bank_push(ry_synth_bank* bank, const double* f0, const float* sp, const float* ap, const int* n_frames, const int* final, int bins,
                       int on_device, double* y, long long y_capacity, long long* sample_offsets);
/* The same call with the samples left on the card: y_dev is a DEVICE pointer of the caller's, stream b's samples are written at
 * y_dev[sample_offsets[b]], back to back -- the layout ry_outgate_bank_push (on_device = 1) reads.  sample_offsets is on the HOST and valid when
 * the call returns.  The records of the retired pulses still come down and the call still ends with its second wait (the next push needs them):
 * against ry_synth_bank_push one device-to-host copy fewer, the same launches.  The bits, the refusals and their order: ry_synth_bank_push. */
int ry_synth_bank_push_dev(ry_synth_bank* bank, const double* f0, const float* sp, const float* ap, const int* n_frames, const int* final, int bins,
                           int on_device, double* y_dev, long long y_capacity, long long* sample_offsets);
/* forgets the signal of `stream` (-1: of every stream) */
int ry_synth_bank_reset(ry_synth_bank* bank, int stream);
/* tests: the pulses the last push found for `stream` (as ry_synth_debug_pulses; read from the card here; RY_ESTATE after a poison) */
int ry_synth_bank_debug_pulses(ry_synth_bank* bank, int stream, long long* index, double* shift, int* voiced, int capacity, int* n);
/* tests: NaN bit patterns in every scratch buffer and in the unused parts of the window buffers; carried state is not touched */
int ry_synth_bank_debug_poison(ry_synth_bank* bank);
/* tests: out[4] = stream waits, kernel launches, host-to-device copies, device-to-host copies of the last push */
int ry_synth_bank_debug_counts(ry_synth_bank* bank, int* out);
/* tests: window rows kept for `stream` */
int ry_synth_bank_debug_rows(ry_synth_bank* bank, int stream);

/* ---- WORLD analysis that feeds the networks (`pyworld.cheaptrick(x, f0, t, fs)` and `pysptk.sp2mc(sp, order, alpha)` in the reference's
 * AcousticFeature.extract, reached from Vocoder.encode).  Semantics: INTEGRATION.md section 11 and tests/world_analysis_ref.py (CheapTrick
 * and sp2mc restated; WORLD's two randn() terms are counter-based functions of (seed, centre sample, index), so a frame's rows depend on
 * (x, f0, t, seed) only).  fft_size: 1024 -- anything else is refused; 8000 <= fs <= 48000; order: 0 .. 63; -0.9 <= alpha <= 0.9;
 * -0.4 <= q1 <= 0; 1 <= f0_floor <= 1000 (Hz) -- outside: refused at ry_analysis_create.  x [x_len] float64, f0 [n] (Hz; at or below
 * max(f0_floor, 3 fs / (fft_size - 3)) = unvoiced, analysed at 500 Hz) and t [n] (seconds) float64, all on the HOST.  Outputs, any may be
 * null: sp64_out [n][513] float64 and mc_out [n][order + 1] float64 on the HOST, sp32_dev_out [n][513] float32 on the DEVICE (the rows
 * ry_synth_* and stage 2 read; = (float)sp64, left on the card).  The call returns after everything is written.  n = 0 or x_len = 0: success,
 * nothing written.  Refused: n < 0, x_len < 0, a null wave / f0 / t with n > 0, f0 that is not finite, f0 >= fs / 2, t outside -1 .. 1e6 s
 * (CheapTrick and D4C alike). */
typedef struct ry_analysis ry_analysis;
int ry_analysis_create(ry_ctx* ctx, int fs, int fft_size, int order, double alpha, double q1, double f0_floor, unsigned seed, ry_analysis** out);
void ry_analysis_destroy(ry_analysis* analysis);
int ry_analysis_run(ry_analysis* analysis, const double* x, long long x_len, const double* f0, const double* t, int n,
                    double* sp64_out, float* sp32_dev_out, double* mc_out);
/* sp2mc of a spectrogram that comes from elsewhere: on_device = 0: sp is [n][513] float64 on the host; 1: [n][513] float32 on the device.
 * mc_out [n][order + 1] float64 on the host. */
int ry_analysis_sp2mc(ry_analysis* analysis, const void* sp, int n, int on_device, double* mc_out);
/* tests: on = 1: every later ry_analysis_run also stores and downloads the integers it decided (off by default: one store per frame and one
 * copy the product path does not pay for). */
int ry_analysis_debug_record(ry_analysis* analysis, int on);
/* tests: the integers the last recorded ry_analysis_run decided, [n][4]: window half length, centre sample, DC-correction bin limit,
 * smoothing boundary (none when recording is off).  out null: the count alone. */
int ry_analysis_debug_ints(ry_analysis* analysis, long long* out, int capacity, int* n);
/* tests: fills every buffer the calls grow with NaN bit patterns. */
int ry_analysis_debug_poison(ry_analysis* analysis);

/* ---- D4C, the band aperiodicity of the same stage (`pyworld.d4c(x, f0, t, fs, threshold)` + `pyworld.code_aperiodicity(ap, fs)`).  Semantics:
 * tests/world_d4c_ref.py (D4C restated; its randn() term is counter-based like CheapTrick's, with keys of its own).  Inputs and refusals as
 * ry_analysis_run, and t >= -1 s.  A frame with f0 == 0 or whose Love-Train ratio is <= threshold is off: its row is 1 - 1e-12; only the
 * other frames pay for the general body.  Outputs, any may be null: ap64_out [n][513] float64 and coded_out [n][B] float64 (dB at 3000 i Hz,
 * B = ry_analysis_d4c_bands) on the HOST, ap32_dev_out [n][513] float32 on the DEVICE (= (float)ap64; the rows ry_synth_* read).  Built for the
 * rates whose D4C transforms are 2048 points and whose band centres are bins of the row (16 and 24 kHz): other rates are refused here (the
 * handle itself is still good for ry_analysis_run). */
int ry_analysis_d4c(ry_analysis* analysis, const double* x, long long x_len, const double* f0, const double* t, int n, double threshold,
                    double* ap64_out, float* ap32_dev_out, double* coded_out);
/* ry_analysis_run and ry_analysis_d4c over one upload of the wave and the track: the same bits as the two calls. */
int ry_analysis_extract(ry_analysis* analysis, const double* x, long long x_len, const double* f0, const double* t, int n, double threshold,
                        double* sp64_out, float* sp32_dev_out, double* mc_out, double* ap64_out, float* ap32_dev_out, double* coded_out);
/* ry_analysis_extract on a wave and a track that are already on the card (what ry_crepe_track left there): x32_dev [x_len] float32, widened on the
 * device ((double)x is exact: the frame kernels see the bits of the host's float64 copy), f0_dev / t_dev [n] float64 device pointers, read in place.
 * The refusals ry_analysis_run makes on the host's track are made by a kernel; the host reads its verdict (one wait) BEFORE any frame kernel is
 * launched, so a refused call (RY_EINVAL: f0 not finite or >= fs / 2, t outside -1 .. 1e6 s) writes no output.  Outputs and everything else as
 * ry_analysis_extract: the same bits.  The inputs are read in the order of the context stream, which the call drains before it returns. */
int ry_analysis_extract_dev(ry_analysis* analysis, const float* x32_dev, long long x_len, const double* f0_dev, const double* t_dev, int n, double threshold,
                            double* sp64_out, float* sp32_dev_out, double* mc_out, double* ap64_out, float* ap32_dev_out, double* coded_out);
/* ry_analysis_extract_dev for the n_waves >= 1 waves and tracks ry_crepe_track_many left on the card.  x32_dev: the waves back to back; f0_dev / t_dev:
 * the tracks back to back; sample_offsets / frame_offsets: HOST arrays of n_waves + 1 entries, both starting at 0 (ry_crepe_track_many_buffers).  The
 * wave is widened and the track checked over the whole call, and the host reads ONE verdict (one wait) before any frame kernel is launched; the frame
 * kernels then run per wave on that wave's samples, so a frame's window is clamped at the ends of its own wave and its noise keys are those of the
 * single call.  Output rows are concatenated in wave order; rows of wave i have the bits of ry_analysis_extract_dev on wave i alone.  Refused, with
 * nothing written: n_waves < 1, offsets that do not start at 0, a wave with no sample or no frame, more than 2^22 frames in all, and what
 * ry_analysis_extract_dev refuses (the frame index in the message counts over the whole call). */
int ry_analysis_extract_many_dev(ry_analysis* analysis, const float* x32_dev, const long long* sample_offsets, const double* f0_dev, const double* t_dev,
                                 const int* frame_offsets, int n_waves, double threshold,
                                 double* sp64_out, float* sp32_dev_out, double* mc_out, double* ap64_out, float* ap32_dev_out, double* coded_out);
/* ry_analysis_extract_dev with DEVICE OUTPUTS ONLY, for a chain that keeps the rows on the card: mc32_dev_out [n][order + 1] float32 = (float)mc, the
 * bits of the host's `mc.astype(float32)` (stored by the sp2mc step itself), sp32_dev_out [n][513] and ap32_dev_out [n][513] as the float32 rows of
 * ry_analysis_extract_dev.  No host row is written and nothing but the verdict of the track check is copied to the host.  Refusals: those of
 * ry_analysis_extract_dev, and a null output; a refused call writes nothing.  The call drains the context stream before it returns. */
int ry_analysis_extract_resident(ry_analysis* analysis, const float* x32_dev, long long x_len, const double* f0_dev, const double* t_dev, int n,
                                 double threshold, float* mc32_dev_out, float* sp32_dev_out, float* ap32_dev_out);
/* ry_analysis_extract_many_dev with the outputs of ry_analysis_extract_resident: mc32_dev_out [sum n][order + 1], sp32_dev_out [sum n][513] and
 * ap32_dev_out [sum n][513] float32 on the DEVICE, rows in wave order; nothing but the ONE verdict of the track check goes to the host.  Rows of wave i
 * have the bits ry_analysis_extract_resident writes for wave i alone.  Refusals: those of the two calls it combines; a refused call writes nothing. */
int ry_analysis_extract_many_resident(ry_analysis* analysis, const float* x32_dev, const long long* sample_offsets, const double* f0_dev,
                                      const double* t_dev, const int* frame_offsets, int n_waves, double threshold,
                                      float* mc32_dev_out, float* sp32_dev_out, float* ap32_dev_out);
/* ry_analysis_extract_many_resident for waves that lie anywhere in an uploaded block and rows that go anywhere in the caller's blocks (what
 * ry_crepe_track_uploaded left, into the frame layout of a call that holds more waves than were tracked): wave i has the samples
 * [first_sample[i], first_sample[i] + n_samples[i]) of x32_dev (x_len samples in all), the frames [frame_offsets[i], frame_offsets[i + 1]) of
 * f0_dev / t_dev (n_waves + 1 entries from 0) and writes rows [row_offsets[i], row_offsets[i] + its frames) of the three blocks; no other row is
 * written.  All tables are HOST arrays.  The same launches and the same one verdict; every row has the bits of ry_analysis_extract_resident on its
 * wave alone.  Refused: what ry_analysis_extract_many_resident refuses, null tables, waves that overlap, do not ascend or leave the block, row
 * ranges that overlap or do not ascend. */
int ry_analysis_extract_spans_resident(ry_analysis* analysis, const float* x32_dev, long long x_len, const long long* first_sample, const int* n_samples,
                                       const double* f0_dev, const double* t_dev, const int* frame_offsets, const int* row_offsets, int n_waves,
                                       double threshold, float* mc32_dev_out, float* sp32_dev_out, float* ap32_dev_out);
/* ---- A track of the caller's own (WORLD mode: f0 from a host tracker such as Harvest) for the device entries above; no ry_crepe handle is needed.
 * ry_analysis_upload_waves: ONE upload -- n_waves >= 1 float32 waves back to back, n_samples[i] each, into a growable block of the handle ->
 * *wave_dev, its device address (the x32_dev of the extract calls, the wave of the ry_vc gate entries).  The call returns once the caller's array is
 * free.  Refused before anything is uploaded: null pointers, n_waves < 1, a wave without a sample, more than 2^31 - 1 samples in all.
 * ry_analysis_ingest_tracks: ONE upload (f0 [sum n_frames] float64 on the HOST, the tracks back to back, and the segment table) and ONE launch of
 * analysis_ingest_tracks, one thread per frame.  For frame k of every track, counted from that track's first frame: t = (k * frame_period_ms) / 1000
 * in two separately rounded float64 operations (numpy's arange(n) * frame_period / 1000.0), voiced = (f0 != 0), f0 as it came -- so a track has the
 * bits of the call on it alone, wherever it stands.  The tracks need not be those of all uploaded waves (a caller that gates first ingests the
 * audible ones and names their waves to ry_analysis_extract_spans_resident).  NOTHING about the f0 values is checked here: the extract calls refuse
 * a non-finite f0 or one at or above fs / 2 by their kernel's verdict, with nothing written.  Refused before anything is uploaded: null pointers,
 * n_waves < 1, a track without a frame, more than 2^22 frames in all, a frame period that is not finite and positive.
 * A refused call of either leaves the waves and the track of the last good call in place and reported.
 * ry_analysis_track_buffers (any pointer may be null): the uploaded block, its waves and sample_offsets (HOST, n_waves + 1 entries from 0; null and
 * 0 when no waves are on the card), the tracks of the last ingest and frame_offsets (HOST, n_tracks + 1 entries from 0), and the device addresses
 * of voiced (bytes), f0 and t (float64).  The host tables hold until the next upload / ingest on the handle.  RY_ESTATE when no track is there:
 * before the first ingest, and after ry_analysis_debug_poison (which covers these buffers and forgets waves and track). */
int ry_analysis_upload_waves(ry_analysis* analysis, const float* audio, const int* n_samples, int n_waves, const float** wave_dev);
int ry_analysis_ingest_tracks(ry_analysis* analysis, const double* f0, const int* n_frames, int n_waves, double frame_period_ms);
int ry_analysis_track_buffers(ry_analysis* analysis, const float** wave_dev, int* n_waves, const long long** sample_offsets, int* n_tracks,
                              const int** frame_offsets, const unsigned char** voiced_dev, const double** f0_dev, const double** t_dev);
/* the number of bands B (1 at 16 kHz, 3 at 24 kHz); negative (an error code) where D4C is not built for the handle's rate */
int ry_analysis_d4c_bands(ry_analysis* analysis);
/* tests: what the last recorded (ry_analysis_debug_record) D4C run decided.  ints_out [n][9]: half length of the Love-Train window, of the other
 * windows, origin sample of the window at t - 0.25 / f, at t, at t + 0.25 / f, DC-correction bin limit, smoothing boundary of width f, of width
 * f / 2, on (1) / off (0); values_out [n][4]: the Love-Train ratio a0 and the coarse dB values of bands 1 .. 3 (0 where there is none).  Both
 * null: the count alone. */
int ry_analysis_debug_d4c(ry_analysis* analysis, long long* ints_out, double* values_out, int capacity, int* n);

/* ---- The output gate: the tail of the reference's decode worker (worker/decode_worker.py:53-59, run.py:194-198, stream/decode_stream.py:38).
 * Samples (float64, NaN replaced by 0.0) are appended to a carried fragment; once it holds `chunk` samples ONE chunk is cut per call and the
 * rest stays carried.  The chunk is silent iff mean_db < -threshold_db, where, in float64,
 *     mean_db = mean(max(db, max(db) - 80)),  db = 10 log10(max(1e-10, |rfft(frame * hann)|^2))
 * over the 1 + chunk / 512 frames of 2048 samples at hop 512 of the chunk padded by 1024 reflected samples on each side (periodic Hann window,
 * 1025 bins): librosa's power_to_db(abs(stft(wave)) ** 2).mean().  An audible chunk is returned as sample * scale, float64 or (out_f32) rounded
 * once to float32: the bits of numpy's (wave * scale).astype(float32).  A chunk that holds +-inf is audible, mean_db NaN, returned as it is.
 * Semantics: tests/output_gate_ref.py, INTEGRATION.md section 18, DESIGN.md section 20.
 * Refused by ry_outgate_create: a null pointer, chunk < 1025 (the reflection would wrap twice) or > 2^24, a NaN threshold or scale. */
typedef struct ry_outgate ry_outgate;
int ry_outgate_create(ry_ctx* ctx, int chunk, double threshold_db, double scale, int out_f32, ry_outgate** out);
void ry_outgate_destroy(ry_outgate* gate);
/* forgets the carried samples */
int ry_outgate_reset(ry_outgate* gate);
/* samples [n] float64, n >= 0, on the host or (on_device = 1) a device pointer read in the order of the context stream.  At most one chunk comes
 * out: *n_out = chunk when one was completed (0 otherwise), *silent = 1 when it is silent -- `out` is then untouched --, *mean_db its mean.  out:
 * HOST, room for out_capacity >= chunk elements of float64 (float32 with out_f32) whenever the call completes a chunk.  A call that completes no
 * chunk does not wait for the stream; one that does waits once for the record and, for an audible chunk, once more for the samples.  Refused
 * before anything is launched or changed: null pointers, n < 0, an `out` too small for the chunk this call completes. */
int ry_outgate_push(ry_outgate* gate, const double* samples, int n, int on_device, void* out, int out_capacity, int* n_out, int* silent, double* mean_db);
/* the samples carried at the moment (negative: error) */
int ry_outgate_held(ry_outgate* gate);
/* tests: out[5] = stream waits, kernel launches, host-to-device copies, device-to-host copies, sample bytes brought to the host by the last push */
int ry_outgate_debug_counts(ry_outgate* gate, long long* out);
/* tests: the bytes of the last push's one upload: the stream table and the chunk map, and the new samples when they came from the host
 * (on_device = 0) -- with on_device = 1 it does not depend on n (negative: error) */
long long ry_outgate_debug_upload_bytes(ry_outgate* gate);
/* tests: NaN bit patterns in every scratch buffer and in every part of the two fragment buffers that holds no carried sample */
int ry_outgate_debug_poison(ry_outgate* gate);

/* ---- A bank of output gates: B streams with one chunk size, threshold, scale and output type, served by ONE call per buffer -- one og_append,
 * one og_frame_db, one og_finish and one og_emit launch, one upload, one download of all records and one wait for the audible chunks, whatever B
 * is.  Contract, without a tolerance: stream b returns, call by call, the records and the chunks a lone ry_outgate returns for the same samples,
 * whatever the other streams do. */
typedef struct ry_outgate_bank ry_outgate_bank;
int ry_outgate_bank_create(ry_ctx* ctx, int n_streams, int chunk, double threshold_db, double scale, int out_f32, ry_outgate_bank** out);
void ry_outgate_bank_destroy(ry_outgate_bank* bank);
/* forgets the carried samples of `stream` (-1: of every stream) */
int ry_outgate_bank_reset(ry_outgate_bank* bank, int stream);
/* samples: the streams' new samples back to back, stream b at samples[sample_offsets[b] .. sample_offsets[b + 1]) (n_streams + 1 entries on the
 * HOST, starting at 0).  A stream without a new sample sits the call out: nothing of it changes and no chunk is cut.  out_offsets [n_streams + 1]:
 * stream b's chunk is at out[out_offsets[b]], out_offsets[b + 1] - out_offsets[b] = chunk when it completed one (silent or not), 0 otherwise.
 * silent [n_streams]: -1 no chunk, 0 audible, 1 silent (its part of `out` untouched); mean_db [n_streams].  Refused before anything is launched or
 * any stream changes: null pointers, offsets that do not start at 0 or fall, out_capacity below chunk times the chunks this call completes. */
int ry_outgate_bank_push(ry_outgate_bank* bank, const double* samples, const long long* sample_offsets, int on_device, void* out, long long out_capacity,
                         long long* out_offsets, int* silent, double* mean_db);
int ry_outgate_bank_held(ry_outgate_bank* bank, int stream);
int ry_outgate_bank_debug_counts(ry_outgate_bank* bank, long long* out);
long long ry_outgate_bank_debug_upload_bytes(ry_outgate_bank* bank);
int ry_outgate_bank_debug_poison(ry_outgate_bank* bank);

/* ---- The row store: the feature segments of a live stream (the reference's stream.stream list, stream/base_stream.py) kept as device rows.
 * Three float32 rings on the card: mc [cap_rows][mc_cols], ap [cap_rows][ap_cols], wave [cap_samples].  Segments are appended in arrival order
 * from blocks that are already on the card and read back as the spans BaseStream.fetch would concatenate; which spans those are, and when a
 * segment may go, is decided on the host (realtime_yukarin_amd/streams.py: fetch_plan, wave_spans, retire).  Every call is enqueued on the
 * context stream; every refusal is made before anything is enqueued or changed.  Semantics: INTEGRATION.md section 23, DESIGN.md section 25.
 * Refused by ry_rowstore_create: null pointers, widths outside 1 .. 65536, cap_rows outside 1 .. 2^22 or more than 2^30 floats in a ring,
 * cap_samples outside 1 .. 2^30. */
typedef struct ry_rowstore ry_rowstore;
int ry_rowstore_create(ry_ctx* ctx, int mc_cols, int ap_cols, int cap_rows, int cap_samples, ry_rowstore** out);
void ry_rowstore_destroy(ry_rowstore* store);
/* rows [row0, row0 + n_rows) of the device blocks mc_dev [.][mc_cols] and ap_dev [.][ap_cols] and samples [sample0, sample0 + n_samples) of
 * wave_dev go behind what the rings hold, in ONE launch that wraps at the ring ends; nothing is waited for.  *row_pos / *sample_pos: the ring
 * positions the segment starts at.  Refused: null pointers, counts or offsets below 0, more rows or samples than the rings have free -- what is
 * live is never overwritten; ry_rowstore_retire makes room. */
int ry_rowstore_append(ry_rowstore* store, const float* mc_dev, const float* ap_dev, int row0, int n_rows, const float* wave_dev, int sample0,
                       int n_samples, int* row_pos, int* sample_pos);
/* the oldest n_rows rows and n_samples samples may be overwritten from now on (host bookkeeping only) */
int ry_rowstore_retire(ry_rowstore* store, int n_rows, int n_samples);
/* the live rows and samples */
int ry_rowstore_held(ry_rowstore* store, int* rows, int* samples);
/* row_spans [n_row_spans][3], sample_spans [n_sample_spans][3] (HOST, int): ring position or -1 for a pad, destination offset, count -- in rows
 * of mc_dst_dev [dst_rows][mc_cols] / ap_dst_dev [dst_rows][ap_cols] and in samples of wave_dst_dev [dst_samples].  ONE upload carries both
 * tables and ONE launch writes all three destinations; a pad writes +0.0f; a span may cross the ring end; rows and samples may start at any
 * 4-byte alignment; nothing outside the destination spans is written; count 0 is accepted.  The call waits for the upload of the table (the
 * host tables are free when it returns), not for the launch.  Refused: null pointers, counts below 0, spans outside the ring or the
 * destination, a position that is retired or was never written. */
int ry_rowstore_fetch(ry_rowstore* store, const int* row_spans, int n_row_spans, const int* sample_spans, int n_sample_spans, float* mc_dst_dev,
                      float* ap_dst_dev, float* wave_dst_dev, int dst_rows, int dst_samples);
/* forgets every segment (host bookkeeping only) */
int ry_rowstore_reset(ry_rowstore* store);
/* tests: the device addresses of the three rings (any pointer may be null) */
int ry_rowstore_debug_buffers(ry_rowstore* store, const float** mc_dev, const float** ap_dev, const float** wave_dev);
/* tests: out[4] = kernel launches, uploads, waits, bytes uploaded by the last append / fetch */
int ry_rowstore_debug_counts(ry_rowstore* store, long long* out);
/* tests: NaN bit patterns in the table buffer and in every part of the rings that holds nothing live */
int ry_rowstore_debug_poison(ry_rowstore* store);

/* ---- The row bank: the row store for the B live streams of one process.  B independent sets of the three rings, all of one shape, each with
 * its own live range; every call names the streams it serves (stream_of [n], HOST, strictly ascending) and runs ONE launch for all of them.
 * Semantics: INTEGRATION.md section 24, DESIGN.md section 26.  Refused by the create call: what the row store's refuses per stream, n_streams
 * outside 1 .. 65536, more than 2^40 floats in one of the three arrays.  Every refusal of every call is made before anything is enqueued or
 * changed for any stream; a repeated or descending stream index is one. */
typedef struct ry_rowbank ry_rowbank;
int ry_rowbank_create(ry_ctx* ctx, int n_streams, int mc_cols, int ap_cols, int cap_rows, int cap_samples, ry_rowbank** out);
void ry_rowbank_destroy(ry_rowbank* bank);
/* For entry i: rows [row0[i], row0[i] + n_rows[i]) of the SHARED device blocks mc_dev / ap_dev and samples [sample0[i], sample0[i] + n_samples[i])
 * of the shared wave_dev (the blocks a many-wave encode leaves on the card) go behind what the rings of stream stream_of[i] hold, wrapping at the
 * ring ends.  ONE launch whatever n is; up to six pieces travel in the kernel arguments, a longer table goes up in ONE upload that is waited
 * for.  row_pos [n] / sample_pos [n]: where each segment starts in its stream's rings.  Refused per entry as the row store's append refuses. */
int ry_rowbank_append(ry_rowbank* bank, int n, const int* stream_of, const float* mc_dev, const float* ap_dev, const int* row0, const int* n_rows,
                      const float* wave_dev, const long long* sample0, const int* n_samples, int* row_pos, int* sample_pos);
/* The convert windows of n streams, back to back in the layout ry_vc_enqueue_waves_device reads: entry i's mc rows from row frame_offsets[i] of
 * mc_dst_dev, its samples from sample sample_offsets[i] of wave_dst_dev (n + 1 entries each, HOST, from 0, ascending).  Its spans are
 * row_spans [row_span_offsets[i] .. row_span_offsets[i + 1]) and the like for the samples: (position in that stream's ring or -1 for a pad,
 * destination offset relative to the entry's first row / sample, count); a pad writes +0.0f.  ONE upload, ONE launch, the upload alone is waited
 * for.  Refused per entry as the row store's fetch refuses, with the entry's slice as the destination, and: offset tables that do not start at 0
 * or fall.  ap is not fetched: the pick call below reads it. */
int ry_rowbank_fetch(ry_rowbank* bank, int n, const int* stream_of, const int* row_spans, const int* row_span_offsets, const int* sample_spans,
                     const int* sample_span_offsets, float* mc_dst_dev, float* wave_dst_dev, const int* frame_offsets, const long long* sample_offsets);
/* The ap rows the synthesizers read, with the silence mask applied: for entry i the rows [keep[2 i], keep[2 i + 1]) of its convert window (the row
 * spans of the fetch call) go to ap_pack_dev [pack_rows][ap_cols], entry after entry -- the order ry_synth_bank_push reads with on_device = 1.  A
 * row is +0.0f where it lies in a pad span or where mask_dev[frame_offsets[i] + row] is 0 (the mask the window call wrote: this call goes behind
 * it on the context stream), else the ring's row, word for word: what ry_rowstore_fetch, ry_mask_rows and the slice give, without the full ap
 * window being written anywhere.  A kept row that no span covers is left as it was.  ONE launch; ONE upload, waited for, when a row is kept.
 * Refused: what the fetch call refuses of the row tables, keep outside the window, pack_rows other than the sum of the kept rows. */
int ry_rowbank_pick_ap(ry_rowbank* bank, int n, const int* stream_of, const int* row_spans, const int* row_span_offsets, const int* frame_offsets,
                       const int* keep, const unsigned char* mask_dev, float* ap_pack_dev, int pack_rows);
/* host bookkeeping only, per stream: the oldest rows / samples may be overwritten; forget every segment (stream -1: of all); the live counts */
int ry_rowbank_retire(ry_rowbank* bank, int stream, int n_rows, int n_samples);
int ry_rowbank_reset(ry_rowbank* bank, int stream);
int ry_rowbank_held(ry_rowbank* bank, int stream, int* rows, int* samples);
/* tests, as the row store's: the three arrays (stream b's rings start b * cap_rows * cols / b * cap_samples floats in); out[4] of the last
 * append / fetch / pick; NaN bit patterns in the table buffers and in every part of every stream's rings that holds nothing live */
int ry_rowbank_debug_buffers(ry_rowbank* bank, const float** mc_dev, const float** ap_dev, const float** wave_dev);
int ry_rowbank_debug_counts(ry_rowbank* bank, long long* out);
int ry_rowbank_debug_poison(ry_rowbank* bank);

#ifdef __cplusplus
}
#endif
#endif
