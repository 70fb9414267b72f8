// synth.cpp -- the WORLD synthesizer of libry355.so (`pyworld.synthesize` / world4py's realtime synthesizer, called by the reference's
// Vocoder.decode / RealtimeVocoder.decode): f0 / spectrogram / aperiodicity frames -> float64 waveform.  Kernels: synth_kernels.h.
// One code path serves the one-shot call and the stream: frames are appended to a window on the device, `advance` scans the samples whose
// two neighbouring frames are there, computes the response of every pulse that has a successor and emits the samples no later pulse can
// reach.  Nothing but the wrapped phase, the pulse list and the frame window is carried from one push to the next: responses of pulses that
// straddle a push boundary are computed again from the same inputs (the same bits), so any cut of a stream equals the one-shot call.
// ry_synth_run_many is the one-shot call for a list of waves: the same three kernels over a segment table (SynthSeg), one scan workgroup per
// wave, the pulses and the samples of all waves in one launch each.  It keeps no stream state and brings no pulse list to the host.
// ry_synth_bank is the stream for many sessions: B streams advanced by one call per buffer, the same three kernels over a stream table
// (SynthStream), the pulse lists and the frame windows carried on the card (synth_gather, synth_retire).  The rules -- what can be scanned, what
// can be emitted, which pulses leave, which frames are still needed -- are the functions `advance` uses.
#include "synth_kernels.h"
#include "ry_host.h"

struct ry_synth {
    ry_ctx* ctx = nullptr;
    int fs = 0;
    double frame_period = 0, spf = 0, lowest_f0 = 0;
    unsigned seed = 0, seed_hash = 0;
    Arena tables;
    sy_c* tw = nullptr;
    double* dc = nullptr;
    SynthScanState* st = nullptr;
    // the stream
    long long n_frames = 0;                  // frames pushed since the last reset
    long long frame0 = 0;                    // absolute index of row 0 of the window
    std::vector<double> f0;                  // thresholded f0 of the window's frames
    long long scanned = 0, done = 0;         // samples whose phase is known / samples emitted
    struct Pulse { long long idx; double shift; int voiced; };
    std::vector<Pulse> live;                 // pulses that can still reach an unemitted sample, and the last one found
    std::vector<Pulse> last_call;            // ry_synth_debug_pulses: the pulses the last call found
    // device buffers: the frame window (two sets: the live rows move to the other set when frames are appended), scratch of a call
    Arena win[2];
    float *sp[2] = {}, *ap[2] = {};
    long long win_cap[2] = {0, 0};
    int cur = 0;
    DevBufList scratch;
    DevBuf<double> d_f0{scratch}, d_pshift{scratch}, d_resp{scratch}, d_y{scratch};
    DevBuf<long long> d_pidx{scratch};                // d_pidx / d_pshift / d_pvoiced: the pulse list, grown together
    DevBuf<int> d_pvoiced{scratch};
    // many waves in one call: the packed f0, the zeroed scan states and the segment table in ONE buffer (one upload), the first response row of
    // every wave, host rows brought over; what the last ry_synth_run_many left for ry_synth_debug_pulses_many (empty: no such call)
    DevBuf<double> d_many{scratch};
    DevBuf<int> d_rstart{scratch};
    DevBuf<float> d_sp_many{scratch}, d_ap_many{scratch};
    std::vector<double> many_host;
    std::vector<int> rstart_host;
    std::vector<int> many_pulse0;
};

// One stream of a bank on the host: what ry_synth keeps for its one stream, except the pulse list, which stays on the card -- the host knows
// its length and the indices of its first and last entry, which is all the rules ask for.
struct BankStream {
    unsigned seed_hash = 0;
    long long n_frames = 0, frame0 = 0, scanned = 0, done = 0;
    std::vector<double> f0;                  // thresholded f0 of the window's frames
    int n_live = 0;
    long long first_idx = -1, last_idx = 0;
    long long row0 = 0;                      // first row of its window in the window buffer in use
    long long dbg_p0 = 0; int dbg_n = 0;     // ry_synth_bank_debug_pulses: where the pulses the last push found are
};

enum { SYNTH_CARRY = 1040 };                 // entries of a stream's carry slot: live pulses lie in [done - 512, done + 511] plus the last one

struct ry_synth_bank {
    ry_ctx* ctx = nullptr;
    ry_synth* core = nullptr;                // rate, frame period, tables, the call buffers of the three kernels and their parameter builders
    int n_streams = 0;
    std::vector<BankStream> s;
    // carried on the card: scan state and carry slot of every stream, the frame windows of all streams back to back (two sets, as ry_synth's)
    Arena carried;
    SynthScanState* st = nullptr;
    long long* c_idx = nullptr; double* c_shift = nullptr; int* c_voiced = nullptr;
    Arena win[2];
    float *sp[2] = {}, *ap[2] = {};
    long long win_cap[2] = {0, 0}, win_rows = 0;
    int cur = 0;
    // scratch of a call: [rows] f0 | [streams] table in ONE buffer, what synth_retire reports
    DevBufList scratch;
    DevBuf<double> d_tab{scratch};
    DevBuf<SynthRetired> d_ret{scratch};
    std::vector<double> tab_host;
    std::vector<SynthStream> ent;
    std::vector<SynthScanState> hs;
    std::vector<SynthRetired> ret;
    bool pulses_valid = false;
    int counts[4] = {0, 0, 0, 0};            // stream waits, kernel launches, host-to-device and device-to-host copies of the last push
};

namespace {
void reset_stream(ry_synth* s) {
    s->n_frames = 0; s->frame0 = 0; s->f0.clear();
    s->scanned = 0; s->done = 0; s->live.clear();
}

long long y_length(const ry_synth* s, long long n) { return (long long)((double)(n - 1) * s->frame_period / 1000 * s->fs) + 1; }

// samples n with n / spf < m - 1: both frames of their interpolation are among the first m
long long known_samples(const ry_synth* s, long long m) {
    if (m < 2) return 0;
    long long n = (long long)std::ceil((double)(m - 1) * s->spf);
    while (n > 0 && !((double)(n - 1) / s->spf < (double)(m - 1))) --n;
    while ((double)n / s->spf < (double)(m - 1)) ++n;
    return n;
}

long long frame_of(const ry_synth* s, long long sample) { return sample <= 0 ? 0 : (long long)std::floor((double)sample / s->spf); }

enum { SYNTH_MAX_FRAMES = 1 << 22, SYNTH_MAX_PULSES = 1 << 30 };      // frames of one call; entries of the pulse arrays of one call

// wave >= 0: the frames are those of that wave of a batched call, or of that stream of a bank (the message names it)
int check_f0(const ry_synth* s, const double* f0, int n_frames, int wave = -1, const char* what = "wave") {
    for (int i = 0; i < n_frames; ++i)
        if (!std::isfinite(f0[i]) || !(f0[i] < 0.5 * s->fs))
            return wave < 0 ? fail(RY_EINVAL, "f0[%d] = %g: finite and below fs / 2", i, f0[i])
                            : fail(RY_EINVAL, "%s %d: f0[%d] = %g: finite and below fs / 2", what, wave, i, f0[i]);
    return RY_OK;
}

int check_frames(const ry_synth* s, const double* f0, const float* sp, const float* ap, int n_frames) {
    if (!f0 || !sp || !ap) return fail(RY_EINVAL, "null f0 / sp / ap");
    if (n_frames < 1) return fail(RY_EINVAL, "n_frames = %d: at least one frame", n_frames);
    if (n_frames > SYNTH_MAX_FRAMES) return fail(RY_EINVAL, "%d frames in one call", n_frames);
    return check_f0(s, f0, n_frames);
}

double threshold_f0(const ry_synth* s, double f0) { return f0 < s->lowest_f0 ? 0.0 : f0; }

// The pulse arrays, grown together, and the parameters of the three kernels that do not depend on the call: what `advance` and
// ry_synth_run_many share.  The caller adds the frames, the sample range and, for many waves, the segment table.
int grow_pulses(ry_synth* s, long long n_p) {
    RY_TRY(s->d_pidx.grow(s->ctx, n_p));
    RY_TRY(s->d_pshift.grow(s->ctx, n_p));
    RY_TRY(s->d_pvoiced.grow(s->ctx, n_p));
    return RY_OK;
}

SynthScanParams scan_params(const ry_synth* s) {
    SynthScanParams p;
    memset(&p, 0, sizeof p);
    p.spf = s->spf; p.fs = (double)s->fs; p.st = s->st;
    p.pidx = s->d_pidx.ptr(); p.pshift = s->d_pshift.ptr(); p.pvoiced = s->d_pvoiced.ptr(); p.cap = (int)s->d_pidx.cap;
    return p;
}

SynthPulseParams pulse_params(const ry_synth* s) {
    SynthPulseParams p;
    memset(&p, 0, sizeof p);
    p.pidx = s->d_pidx.ptr(); p.pshift = s->d_pshift.ptr(); p.pvoiced = s->d_pvoiced.ptr();
    p.spf = s->spf; p.seed_hash = s->seed_hash; p.tw = s->tw; p.dc = s->dc; p.resp = s->d_resp.ptr();
    return p;
}

SynthOverlapParams overlap_params(const ry_synth* s) {
    SynthOverlapParams p;
    memset(&p, 0, sizeof p);
    p.pidx = s->d_pidx.ptr(); p.resp = s->d_resp.ptr(); p.y = s->d_y.ptr();
    return p;
}

// appends frames to the window; rows before `keep_from` (absolute) are dropped on the way
int append_frames(ry_synth* s, const double* f0, const float* sp, const float* ap, int n, int on_device, long long keep_from) {
    const ry_stream_t st = s->ctx->stream;
    keep_from = std::max(keep_from, s->frame0);
    const long long old_rows = s->frame0 + (long long)s->f0.size() - keep_from;     // live rows
    const long long rows = old_rows + n;
    const int from = s->cur, to = 1 - s->cur;
    if (rows > s->win_cap[to]) {
        RT_TRY(rt::stream_sync(st));
        s->win[to].release();
        s->sp[to] = s->ap[to] = nullptr; s->win_cap[to] = 0;
        const long long cap = rows + rows / 2 + 16;
        RY_TRY(s->win[to].alloc(&s->sp[to], (size_t)cap * SYNTH_BINS));
        RY_TRY(s->win[to].alloc(&s->ap[to], (size_t)cap * SYNTH_BINS));
        s->win_cap[to] = cap;
    }
    const size_t row = SYNTH_BINS * sizeof(float);
    if (old_rows > 0) {
        const size_t off = (size_t)(keep_from - s->frame0) * SYNTH_BINS;
        RT_TRY(rt::d2d(s->sp[to], s->sp[from] + off, (size_t)old_rows * row, st));
        RT_TRY(rt::d2d(s->ap[to], s->ap[from] + off, (size_t)old_rows * row, st));
    }
    float* dsp = s->sp[to] + (size_t)old_rows * SYNTH_BINS;
    float* dap = s->ap[to] + (size_t)old_rows * SYNTH_BINS;
    if (on_device) {
        RT_TRY(rt::d2d(dsp, sp, (size_t)n * row, st));
        RT_TRY(rt::d2d(dap, ap, (size_t)n * row, st));
    } else {
        RT_TRY(rt::h2d(dsp, sp, (size_t)n * row, st));
        RT_TRY(rt::h2d(dap, ap, (size_t)n * row, st));
        RT_TRY(rt::stream_sync(st));                               // the caller's arrays are free when the call returns
    }
    s->f0.erase(s->f0.begin(), s->f0.begin() + (keep_from - s->frame0));
    for (int i = 0; i < n; ++i) s->f0.push_back(threshold_f0(s, f0[i]));
    s->frame0 = keep_from;
    s->cur = to;
    s->n_frames += n;
    return RY_OK;
}

// The rules of a stream, shared by the single stream (`advance`, whose pulse list is on the host) and the bank (whose lists are on the card).
// the first frame a later call can still read: the frames of the oldest live pulse (has_live) and of the next sample to scan
long long needed_frame(const ry_synth* s, long long scanned, bool has_live, long long first_idx) {
    long long f = frame_of(s, scanned);
    if (has_live) f = std::min(f, frame_of(s, first_idx));
    return std::max(0LL, f - 1);
}

long long first_needed_frame(const ry_synth* s) { return needed_frame(s, s->scanned, !s->live.empty(), s->live.empty() ? 0 : s->live.front().idx); }

// the sample a call scans up to: with m frames pushed, the whole signal (final) or what both neighbouring frames are there for
long long scan_end(const ry_synth* s, long long m, bool final, long long scanned) {
    return std::max(final ? y_length(s, m) : known_samples(s, m), scanned);
}

// what can be emitted after a scan up to k1 that left `total` pulses, the last at last_idx: everything (final), or the samples the last pulse
// -- the one without a successor -- cannot reach; `complete` pulses have a response
void emit_range(bool final, long long total, long long last_idx, long long done, long long k1, long long* complete, long long* fin) {
    *complete = final ? total : std::max(0LL, total - 1);
    const long long f = final ? k1 : (total > 0 ? std::max(done, last_idx - SYNTH_HALF + 1) : done);
    *fin = std::min(f, k1);
}

// samples a call with n more frames may return
long long may_return(const ry_synth* s, long long pushed, long long scanned, long long done, long long n, bool final) {
    const long long m = pushed + n;
    if (m < 1) return 0;
    return std::max(0LL, scan_end(s, m, final, scanned) - done);
}

// scans what can be scanned, emits what can be emitted.  final: the signal ends with the frames pushed so far.  y_on_device: y is a block of
// the caller's on the card -- synth_overlap writes the samples there and the call returns behind that launch, without download or wait.
int advance(ry_synth* s, bool final, double* y, long long y_capacity, long long* n_out, bool y_on_device = false) {
    const ry_stream_t st = s->ctx->stream;
    const long long m = s->n_frames;
    const long long k1 = scan_end(s, m, final, s->scanned);
    if (final && y_length(s, m) < s->scanned) return fail(RY_ESTATE, "stream state: %lld samples scanned, the signal has %lld", s->scanned, y_length(s, m));
    if (k1 - s->done > y_capacity)
        return fail(RY_EINVAL, "y holds %lld samples, this call may return up to %lld", y_capacity, k1 - s->done);
    const long long n_new = k1 - s->scanned;
    const long long n_old = (long long)s->live.size();
    if (n_old + n_new + 1 > SYNTH_MAX_PULSES) return fail(RY_EINVAL, "%lld samples in one call", n_new);
    // the pulse arrays: the live pulses, then what the scan appends (at most one pulse per sample)
    const long long n_p = n_old + n_new + 1;                       // (grow's n_p + n_p / 2 + 64 is the n_p * 3 / 2 + 64 these have always had)
    RY_TRY(grow_pulses(s, n_p));
    RY_TRY(s->d_f0.grow(s->ctx, (long long)s->f0.size()));
    std::vector<long long> hidx(n_old); std::vector<double> hshift(n_old); std::vector<int> hvo(n_old);
    for (long long i = 0; i < n_old; ++i) { hidx[i] = s->live[i].idx; hshift[i] = s->live[i].shift; hvo[i] = s->live[i].voiced; }
    if (n_old) {
        RT_TRY(rt::h2d(s->d_pidx.ptr(), hidx.data(), n_old * sizeof(long long), st));
        RT_TRY(rt::h2d(s->d_pshift.ptr(), hshift.data(), n_old * sizeof(double), st));
        RT_TRY(rt::h2d(s->d_pvoiced.ptr(), hvo.data(), n_old * sizeof(int), st));
    }
    RT_TRY(rt::h2d(s->d_f0.ptr(), s->f0.data(), s->f0.size() * sizeof(double), st));
    RT_TRY(rt::stream_sync(st));                                   // hidx / hshift / hvo are reused below
    SynthScanState hs;
    long long total = n_old;
    s->last_call.clear();
    s->many_pulse0.clear();
    if (n_new > 0) {
        const int n_old_i = (int)n_old;
        RT_TRY(rt::h2d(&s->st->n_pulses, &n_old_i, sizeof(int), st));
        SynthScanParams sp = scan_params(s);
        sp.f0 = s->d_f0.ptr(); sp.frame0 = s->frame0; sp.last_frame = m - 1; sp.n0 = s->scanned; sp.n1 = k1;
        RY_LAUNCH(synth_scan, dim3(1), 256, st, sp);
        RT_TRY(rt::last_error());
        RT_TRY(rt::d2h(&hs, s->st, sizeof hs, st));
        RT_TRY(rt::stream_sync(st));
        if (hs.overflow) return fail(RY_ESTATE, "pulse list overflow (%d)", hs.overflow);
        total = hs.n_pulses;
        const long long added = total - n_old;
        if (added > 0) {
            hidx.resize(added); hshift.resize(added); hvo.resize(added);
            RT_TRY(rt::d2h(hidx.data(), s->d_pidx.ptr() + n_old, added * sizeof(long long), st));
            RT_TRY(rt::d2h(hshift.data(), s->d_pshift.ptr() + n_old, added * sizeof(double), st));
            RT_TRY(rt::d2h(hvo.data(), s->d_pvoiced.ptr() + n_old, added * sizeof(int), st));
            RT_TRY(rt::stream_sync(st));
            for (long long i = 0; i < added; ++i) {
                ry_synth::Pulse p = {hidx[i], hshift[i], hvo[i]};
                s->live.push_back(p);
                s->last_call.push_back(p);
            }
        }
        s->scanned = k1;
    }
    // what can be emitted: everything (final), or the samples the last pulse found -- the one without a successor -- cannot reach
    long long complete = 0, fin = 0;
    emit_range(final, total, total > 0 ? s->live.back().idx : 0, s->done, k1, &complete, &fin);
    const long long n_emit = fin - s->done;
    if (n_emit > 0) {
        if (complete > 0) {
            RY_TRY(s->d_resp.grow(s->ctx, complete * SYNTH_FFT));
            SynthPulseParams pp = pulse_params(s);
            pp.n_pulses = (int)total; pp.n_complete = (int)complete;
            pp.sp = s->sp[s->cur]; pp.ap = s->ap[s->cur]; pp.frame0 = s->frame0; pp.last_frame = m - 1;
            RY_LAUNCH(synth_pulse, dim3((unsigned)complete), 256, st, pp);
            RT_TRY(rt::last_error());
        }
        if (!y_on_device) RY_TRY(s->d_y.grow(s->ctx, n_emit));
        SynthOverlapParams op = overlap_params(s);
        op.n_complete = (int)complete; op.s0 = s->done; op.s1 = fin;
        if (y_on_device) op.y = y;                                 // one 8-byte store per sample: any double-aligned destination, nothing outside [y, y + n_emit)
        RY_LAUNCH(synth_overlap, dim3((unsigned)((n_emit + 255) / 256)), 256, st, op);
        RT_TRY(rt::last_error());
        if (!y_on_device) {
            RT_TRY(rt::d2h(y, s->d_y.ptr(), (size_t)n_emit * sizeof(double), st));
            RT_TRY(rt::stream_sync(st));
        }
        s->done = fin;
    }
    *n_out = n_emit;
    // pulses that cannot reach an unemitted sample leave the list (the last one stays: it has no successor yet)
    size_t drop = 0;
    while (drop + 1 < s->live.size() && s->live[drop].idx < s->done - SYNTH_HALF) ++drop;
    s->live.erase(s->live.begin(), s->live.begin() + (long)drop);
    return RY_OK;
}

int reset_device_state(ry_synth* s) {
    SynthScanState z;
    memset(&z, 0, sizeof z);
    RT_TRY(rt::h2d(s->st, &z, sizeof z, s->ctx->stream));
    RT_TRY(rt::stream_sync(s->ctx->stream));
    return RY_OK;
}

// ry_synth_push and ry_synth_push_dev: the refusals, the frames, the advance.  y_on_device: see `advance`.
int push_frames(ry_synth* s, const double* f0, const float* sp, const float* ap, int n_frames, int bins, int on_device,
                double* y, long long y_capacity, long long* n_out, bool y_on_device) {
    RY_TRY(check_handle(s, "synthesizer"));
    if (n_out) *n_out = 0;
    if (!y || !n_out || y_capacity < 0) return fail(RY_EINVAL, "bad output arguments");
    if (bins != SYNTH_BINS) return fail(RY_EINVAL, "%d bins per frame, fft_size / 2 + 1 = %d expected", bins, SYNTH_BINS);
    RY_TRY(check_frames(s, f0, sp, ap, n_frames));
    const long long m = s->n_frames + n_frames;
    const long long may = std::max(known_samples(s, m), s->scanned) - s->done;
    if (may > y_capacity) return fail(RY_EINVAL, "y holds %lld samples, this push may return up to %lld (ry_synth_bound)", y_capacity, may);
    RY_TRY(append_frames(s, f0, sp, ap, n_frames, on_device, first_needed_frame(s)));
    return advance(s, false, y, y_capacity, n_out, y_on_device);
}

// ry_synth_flush and ry_synth_flush_dev.  The device form resets the stream in stream order, as ry_synth_run_many does: it waits for nothing.
int flush_frames(ry_synth* s, double* y, long long y_capacity, long long* n_out, bool y_on_device) {
    RY_TRY(check_handle(s, "synthesizer"));
    if (n_out) *n_out = 0;
    if (!y || !n_out || y_capacity < 0) return fail(RY_EINVAL, "bad output arguments");
    if (s->n_frames < 1) return fail(RY_ESTATE, "flush of an empty stream");
    RY_TRY(advance(s, true, y, y_capacity, n_out, y_on_device));
    if (!y_on_device) return ry_synth_reset(s);
    static const SynthScanState zero_state = {0.0, 0, 0, 0, 0, 0};
    reset_stream(s);
    RT_TRY(rt::h2d(s->st, &zero_state, sizeof zero_state, s->ctx->stream));
    return RY_OK;
}
}  // namespace

extern "C" {

int ry_synth_create(ry_ctx* ctx, int fs, double frame_period_ms, int fft_size, unsigned seed, ry_synth** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    if (!ctx) return fail(RY_EINVAL, "null context");
    if (fs < 8000 || fs > 48000) return fail(RY_EINVAL, "sampling rate %d: 8000 .. 48000", fs);
    if (!(frame_period_ms > 0) || !std::isfinite(frame_period_ms)) return fail(RY_EINVAL, "frame period %g ms", frame_period_ms);
    if (fft_size != SYNTH_FFT) return fail(RY_EINVAL, "fft_size %d: the transforms are built for %d (CheapTrick's size at 16 and 24 kHz)", fft_size, SYNTH_FFT);
    const double spf = fs * frame_period_ms / 1000;
    if (!(spf >= 1.0)) return fail(RY_EINVAL, "a frame of %g ms at %d Hz is shorter than a sample", frame_period_ms, fs);
    RT_TRY(rt::set_device(ctx->device));
    std::unique_ptr<ry_synth> s(new ry_synth());
    s->ctx = ctx; s->fs = fs; s->frame_period = frame_period_ms; s->spf = spf; s->lowest_f0 = (double)fs / fft_size + 1.0;
    s->seed = seed; s->seed_hash = synth_hash32(seed);
    const std::vector<double> tw = twiddles(SYNTH_FFT);
    std::vector<double> dc(SYNTH_FFT);
    double sum = 0;
    for (int i = 0; i < SYNTH_HALF; ++i) {
        dc[i] = 0.5 - 0.5 * std::cos(SYNTH_TWO_PI * (i + 1.0) / (1.0 + SYNTH_FFT));
        dc[SYNTH_FFT - 1 - i] = dc[i];
        sum += 2 * dc[i];
    }
    for (int i = 0; i < SYNTH_FFT; ++i) dc[i] /= sum;
    SynthScanState z;
    memset(&z, 0, sizeof z);
    RY_TRY(upload_table(s->tables, ctx, (const sy_c*)tw.data(), (size_t)SYNTH_FFT, &s->tw));
    RY_TRY(upload_table(s->tables, ctx, dc.data(), dc.size(), &s->dc));
    RY_TRY(upload_table(s->tables, ctx, &z, (size_t)1, &s->st));
    *out = s.release();
    return RY_OK;
}

void ry_synth_destroy(ry_synth* s) {
    if (!s) return;
    rt::set_device(s->ctx->device);
    rt::stream_sync(s->ctx->stream);
    delete s;
}

int ry_synth_reset(ry_synth* s) {
    RY_TRY(check_handle(s, "synthesizer"));
    reset_stream(s);
    return reset_device_state(s);
}

int ry_synth_length(ry_synth* s, int n_frames) {
    if (!s || n_frames < 1) return fail(RY_EINVAL, "bad argument");
    return (int)y_length(s, n_frames);
}

int ry_synth_bound(ry_synth* s, int n_frames, int final) {
    if (!s || n_frames < 0) return fail(RY_EINVAL, "bad argument");
    return (int)may_return(s, s->n_frames, s->scanned, s->done, n_frames, final != 0);
}

int ry_synth_push(ry_synth* s, const double* f0, const float* sp, const float* ap, int n_frames, int bins, int on_device,
                  double* y, int y_capacity, int* n_out) {
    if (n_out) *n_out = 0;
    long long n = 0;
    const int rc = push_frames(s, f0, sp, ap, n_frames, bins, on_device, y, n_out ? (long long)y_capacity : -1, &n, false);
    if (n_out) *n_out = (int)n;
    return rc;
}

int ry_synth_push_dev(ry_synth* s, const double* f0, const float* sp, const float* ap, int n_frames, int bins, int on_device,
                      double* y_dev, long long y_capacity, long long* n_out) {
    return push_frames(s, f0, sp, ap, n_frames, bins, on_device, y_dev, y_capacity, n_out, true);
}

int ry_synth_flush(ry_synth* s, double* y, int y_capacity, int* n_out) {
    if (n_out) *n_out = 0;
    long long n = 0;
    const int rc = flush_frames(s, y, n_out ? (long long)y_capacity : -1, &n, false);
    if (n_out) *n_out = (int)n;
    return rc;
}

int ry_synth_flush_dev(ry_synth* s, double* y_dev, long long y_capacity, long long* n_out) {
    return flush_frames(s, y_dev, y_capacity, n_out, true);
}

int ry_synth_run(ry_synth* s, const double* f0, const float* sp, const float* ap, int n_frames, int bins, int on_device,
                 double* y, int y_capacity, int* n_out) {
    RY_TRY(check_handle(s, "synthesizer"));
    if (n_out) *n_out = 0;
    if (!y || !n_out || y_capacity < 0) return fail(RY_EINVAL, "bad output arguments");
    if (bins != SYNTH_BINS) return fail(RY_EINVAL, "%d bins per frame, fft_size / 2 + 1 = %d expected", bins, SYNTH_BINS);
    RY_TRY(check_frames(s, f0, sp, ap, n_frames));
    if (y_length(s, n_frames) > y_capacity) return fail(RY_EINVAL, "y holds %d samples, %d frames give %lld", y_capacity, n_frames, y_length(s, n_frames));
    RY_TRY(ry_synth_reset(s));
    RY_TRY(append_frames(s, f0, sp, ap, n_frames, on_device, 0));
    long long n = 0;
    const int rc = advance(s, true, y, y_capacity, &n);
    *n_out = (int)n;
    const int rc2 = ry_synth_reset(s);
    return rc != RY_OK ? rc : rc2;
}

int ry_synth_run_many(ry_synth* s, const double* f0, const float* sp, const float* ap, const int* n_frames, int n_waves, int bins, int on_device,
                      double* y, long long y_capacity, long long* sample_offsets) {
    RY_TRY(check_handle(s, "synthesizer"));
    // every refusal comes before anything is launched or written
    if (!f0 || !sp || !ap || !n_frames || !y || !sample_offsets) return fail(RY_EINVAL, "null f0 / sp / ap / n_frames / y / sample_offsets");
    if (n_waves < 1) return fail(RY_EINVAL, "%d waves", n_waves);
    if (bins != SYNTH_BINS) return fail(RY_EINVAL, "%d bins per frame, fft_size / 2 + 1 = %d expected", bins, SYNTH_BINS);
    std::vector<SynthSeg> segs((size_t)n_waves);
    long long rows = 0, samples = 0, pulses = 0;
    for (int b = 0; b < n_waves; ++b) {
        if (n_frames[b] < 1) return fail(RY_EINVAL, "wave %d has %d frames: at least one", b, n_frames[b]);
        if (n_frames[b] > SYNTH_MAX_FRAMES - rows) return fail(RY_EINVAL, "more than %d frames in one call", (int)SYNTH_MAX_FRAMES);
        const long long len = y_length(s, n_frames[b]);
        if (pulses + len + 1 > SYNTH_MAX_PULSES) return fail(RY_EINVAL, "more than %d samples in one call", (int)SYNTH_MAX_PULSES);
        SynthSeg& g = segs[(size_t)b];
        g.row0 = (int)rows; g.n_frames = n_frames[b]; g.pulse0 = (int)pulses; g.pulse_cap = (int)len + 1; g.sample0 = (int)samples; g.n_samples = (int)len;
        rows += n_frames[b]; samples += len; pulses += len + 1;
    }
    for (int b = 0; b < n_waves; ++b) RY_TRY(check_f0(s, f0 + segs[(size_t)b].row0, n_frames[b], b));
    if (samples > y_capacity) return fail(RY_EINVAL, "y holds %lld samples, the %d waves give %lld", y_capacity, n_waves, samples);
    const ry_stream_t st = s->ctx->stream;
    // drops a stream in progress, as ry_synth_run does, and leaves the stream reset: nothing below touches its state.  The zeroed state goes up
    // in stream order, without ry_synth_reset's wait.
    static const SynthScanState zero_state = {0.0, 0, 0, 0, 0, 0};
    reset_stream(s);
    RT_TRY(rt::h2d(s->st, &zero_state, sizeof zero_state, st));
    s->last_call.clear();
    s->many_pulse0.clear();
    // one upload: [rows] thresholded f0 | [n_waves] zeroed scan states | [n_waves] segments, in units of a double
    const size_t st_off = (size_t)rows, seg_off = st_off + (size_t)n_waves * (sizeof(SynthScanState) / sizeof(double));
    const size_t n_many = seg_off + ((size_t)n_waves * sizeof(SynthSeg) + sizeof(double) - 1) / sizeof(double);
    static_assert(sizeof(SynthScanState) % sizeof(double) == 0, "the scan states sit between two arrays of doubles");
    s->many_host.assign(n_many, 0.0);                              // the handle's own: the host array of the upload outlives the call
    for (long long i = 0; i < rows; ++i) s->many_host[(size_t)i] = threshold_f0(s, f0[i]);
    memcpy(s->many_host.data() + seg_off, segs.data(), segs.size() * sizeof(SynthSeg));
    RY_TRY(s->d_many.grow(s->ctx, (long long)n_many));
    RY_TRY(s->d_rstart.grow(s->ctx, n_waves + 1));
    RY_TRY(grow_pulses(s, pulses));
    RY_TRY(s->d_y.grow(s->ctx, samples));
    if (!on_device) {
        RY_TRY(s->d_sp_many.grow(s->ctx, rows * SYNTH_BINS));
        RY_TRY(s->d_ap_many.grow(s->ctx, rows * SYNTH_BINS));
        RT_TRY(rt::h2d(s->d_sp_many.ptr(), sp, (size_t)rows * SYNTH_BINS * sizeof(float), st));
        RT_TRY(rt::h2d(s->d_ap_many.ptr(), ap, (size_t)rows * SYNTH_BINS * sizeof(float), st));
        sp = s->d_sp_many.ptr(); ap = s->d_ap_many.ptr();
    }
    RT_TRY(rt::h2d(s->d_many.ptr(), s->many_host.data(), n_many * sizeof(double), st));
    const double* d_f0 = s->d_many.ptr();
    SynthScanState* d_st = (SynthScanState*)(s->d_many.ptr() + st_off);
    const SynthSeg* d_seg = (const SynthSeg*)(s->d_many.ptr() + seg_off);
    SynthScanParams cp = scan_params(s);
    cp.f0 = d_f0; cp.st = d_st; cp.seg = d_seg;
    RY_LAUNCH(synth_scan, dim3((unsigned)n_waves), 256, st, cp);
    RT_TRY(rt::last_error());
    std::vector<SynthScanState> hs((size_t)n_waves);
    RT_TRY(rt::d2h(hs.data(), d_st, hs.size() * sizeof(SynthScanState), st));
    RT_TRY(rt::stream_sync(st));                                   // wait 1 of 2: the pulse counts and overflow words (the host rows are free from here on)
    s->rstart_host.assign((size_t)n_waves + 1, 0);
    for (int b = 0; b < n_waves; ++b) {
        if (hs[(size_t)b].overflow) return fail(RY_ESTATE, "wave %d: pulse list overflow (%d)", b, hs[(size_t)b].overflow);
        s->rstart_host[(size_t)b + 1] = s->rstart_host[(size_t)b] + hs[(size_t)b].n_pulses;      // at most `pulses` in all: fits
    }
    const int total = s->rstart_host[(size_t)n_waves];
    RT_TRY(rt::h2d(s->d_rstart.ptr(), s->rstart_host.data(), s->rstart_host.size() * sizeof(int), st));
    if (total > 0) {
        RY_TRY(s->d_resp.grow(s->ctx, (long long)total * SYNTH_FFT));
        SynthPulseParams pp = pulse_params(s);
        pp.sp = sp; pp.ap = ap; pp.seg = d_seg; pp.rstart = s->d_rstart.ptr(); pp.n_seg = n_waves;
        RY_LAUNCH(synth_pulse, dim3((unsigned)total), 256, st, pp);
        RT_TRY(rt::last_error());
    }
    SynthOverlapParams op = overlap_params(s);
    op.s0 = 0; op.s1 = samples; op.seg = d_seg; op.rstart = s->d_rstart.ptr(); op.n_seg = n_waves;
    RY_LAUNCH(synth_overlap, dim3((unsigned)((samples + 255) / 256)), 256, st, op);
    RT_TRY(rt::last_error());
    RT_TRY(rt::d2h(y, s->d_y.ptr(), (size_t)samples * sizeof(double), st));
    RT_TRY(rt::stream_sync(st));                                   // wait 2 of 2
    for (int b = 0; b < n_waves; ++b) sample_offsets[b] = segs[(size_t)b].sample0;
    sample_offsets[n_waves] = samples;
    s->many_pulse0.resize((size_t)n_waves);
    for (int b = 0; b < n_waves; ++b) s->many_pulse0[(size_t)b] = segs[(size_t)b].pulse0;
    return RY_OK;
}

int ry_synth_debug_pulses_many(ry_synth* s, int wave, long long* index, double* shift, int* voiced, int capacity, int* n) {
    RY_TRY(check_handle(s, "synthesizer"));
    if (!n) return fail(RY_EINVAL, "bad argument");
    *n = 0;
    if (s->many_pulse0.empty()) return fail(RY_ESTATE, "the last call was not ry_synth_run_many");
    if (wave < 0 || wave >= (int)s->many_pulse0.size()) return fail(RY_EINVAL, "wave %d of %d", wave, (int)s->many_pulse0.size());
    const int count = s->rstart_host[(size_t)wave + 1] - s->rstart_host[(size_t)wave], p0 = s->many_pulse0[(size_t)wave];
    *n = count;
    if (!index && !shift && !voiced) return RY_OK;                 // the count alone
    if (capacity < count) return fail(RY_EINVAL, "%d pulses, room for %d", count, capacity);
    const ry_stream_t st = s->ctx->stream;
    if (index) RT_TRY(rt::d2h(index, s->d_pidx.ptr() + p0, (size_t)count * sizeof(long long), st));
    if (shift) RT_TRY(rt::d2h(shift, s->d_pshift.ptr() + p0, (size_t)count * sizeof(double), st));
    if (voiced) RT_TRY(rt::d2h(voiced, s->d_pvoiced.ptr() + p0, (size_t)count * sizeof(int), st));
    RT_TRY(rt::stream_sync(st));
    return RY_OK;
}

int ry_synth_debug_pulses(ry_synth* s, long long* index, double* shift, int* voiced, int capacity, int* n) {
    if (!s || !n) return fail(RY_EINVAL, "bad argument");
    *n = (int)s->last_call.size();
    if (!index && !shift && !voiced) return RY_OK;                 // the count alone
    if (capacity < *n) return fail(RY_EINVAL, "%d pulses, room for %d", *n, capacity);
    for (int i = 0; i < *n; ++i) {
        if (index) index[i] = s->last_call[i].idx;
        if (shift) shift[i] = s->last_call[i].shift;
        if (voiced) voiced[i] = s->last_call[i].voiced;
    }
    return RY_OK;
}

int ry_synth_debug_poison(ry_synth* s) {
    RY_TRY(check_handle(s, "synthesizer"));
    const ry_stream_t st = s->ctx->stream;
    RT_TRY(rt::stream_sync(st));
    s->many_pulse0.clear();                                        // the pulse slices of a batched call are gone
    // every scratch buffer and the set of the frame window that is not in use: all bits set (NaN as a float or a double, -1 as an index)
    for (DevBufBase* b : s->scratch) RY_TRY(b->poison(st));
    const int idle = 1 - s->cur;
    if (s->sp[idle]) {
        RT_TRY(rt::dmemset(s->sp[idle], 0xff, (size_t)s->win_cap[idle] * SYNTH_BINS * sizeof(float), st));
        RT_TRY(rt::dmemset(s->ap[idle], 0xff, (size_t)s->win_cap[idle] * SYNTH_BINS * sizeof(float), st));
    }
    if (s->sp[s->cur]) {                                            // behind the live rows of the set in use
        const size_t used = s->f0.size() * SYNTH_BINS, cap = (size_t)s->win_cap[s->cur] * SYNTH_BINS;
        RT_TRY(rt::dmemset(s->sp[s->cur] + used, 0xff, (cap - used) * sizeof(float), st));
        RT_TRY(rt::dmemset(s->ap[s->cur] + used, 0xff, (cap - used) * sizeof(float), st));
    }
    RT_TRY(rt::stream_sync(st));
    return RY_OK;
}

// ---- the bank of streams ---------------------------------------------------------------------------------------------------------------------
static void bank_reset_stream(BankStream& t) {
    t.n_frames = 0; t.frame0 = 0; t.scanned = 0; t.done = 0; t.f0.clear();
    t.n_live = 0; t.first_idx = -1; t.last_idx = 0;
}

int ry_synth_bank_create(ry_ctx* ctx, int fs, double frame_period_ms, int fft_size, int n_streams, const unsigned* seeds, ry_synth_bank** out) {
    if (!out) return fail(RY_EINVAL, "null out pointer");
    *out = nullptr;
    if (!seeds) return fail(RY_EINVAL, "null seeds");
    if (n_streams < 1 || n_streams > (1 << 16)) return fail(RY_EINVAL, "%d streams: 1 .. 65536", n_streams);
    ry_synth* core = nullptr;
    RY_TRY(ry_synth_create(ctx, fs, frame_period_ms, fft_size, seeds[0], &core));       // the domain and the refusals of a single stream
    std::unique_ptr<ry_synth_bank> k(new ry_synth_bank());
    k->ctx = ctx; k->core = core; k->n_streams = n_streams;
    k->s.resize((size_t)n_streams);
    for (int b = 0; b < n_streams; ++b) k->s[(size_t)b].seed_hash = synth_hash32(seeds[b]);
    const std::vector<SynthScanState> z((size_t)n_streams, SynthScanState{0.0, 0, 0, 0, 0, 0});
    const size_t slots = (size_t)n_streams * SYNTH_CARRY;
    int rc = upload_table(k->carried, ctx, z.data(), z.size(), &k->st);
    if (rc == RY_OK) rc = k->carried.alloc((float**)&k->c_idx, slots * 2);
    if (rc == RY_OK) rc = k->carried.alloc((float**)&k->c_shift, slots * 2);
    if (rc == RY_OK) rc = k->carried.alloc((float**)&k->c_voiced, slots);
    if (rc != RY_OK) { ry_synth_destroy(core); return rc; }
    *out = k.release();
    return RY_OK;
}

void ry_synth_bank_destroy(ry_synth_bank* k) {
    if (!k) return;
    rt::set_device(k->ctx->device);
    rt::stream_sync(k->ctx->stream);
    ry_synth_destroy(k->core);
    delete k;
}

int ry_synth_bank_bound(ry_synth_bank* k, int stream, int n_frames, int final) {
    if (!k || stream < 0 || stream >= k->n_streams || n_frames < 0) return fail(RY_EINVAL, "bad argument");
    const BankStream& t = k->s[(size_t)stream];
    return (int)may_return(k->core, t.n_frames, t.scanned, t.done, n_frames, final != 0);
}

int ry_synth_bank_reset(ry_synth_bank* k, int stream) {
    RY_TRY(check_handle(k, "synthesizer bank"));
    if (stream < -1 || stream >= k->n_streams) return fail(RY_EINVAL, "stream %d of %d", stream, k->n_streams);
    const int b0 = stream < 0 ? 0 : stream, b1 = stream < 0 ? k->n_streams : stream + 1;
    const std::vector<SynthScanState> z((size_t)(b1 - b0), SynthScanState{0.0, 0, 0, 0, 0, 0});
    for (int b = b0; b < b1; ++b) bank_reset_stream(k->s[(size_t)b]);
    RT_TRY(rt::h2d(k->st + b0, z.data(), z.size() * sizeof(SynthScanState), k->ctx->stream));
    RT_TRY(rt::stream_sync(k->ctx->stream));
    return RY_OK;
}

// ry_synth_bank_push and ry_synth_bank_push_dev.  y_on_device: y is a block of the caller's on the card -- synth_overlap writes stream b's
// samples at y[out0 of b] and no sample comes down; the records of synth_retire and the second wait stay, the next push needs them.
static int bank_push_frames(ry_synth_bank* k, const double* f0, const float* sp, const float* ap, const int* n_frames, const int* final, int bins,
                            int on_device, double* y, long long y_capacity, long long* sample_offsets, bool y_on_device) {
    RY_TRY(check_handle(k, "synthesizer bank"));
    // every refusal comes before anything is launched, uploaded or changed in any stream's state
    if (!f0 || !sp || !ap || !n_frames || !y || !sample_offsets) return fail(RY_EINVAL, "null f0 / sp / ap / n_frames / y / sample_offsets");
    if (bins != SYNTH_BINS) return fail(RY_EINVAL, "%d bins per frame, fft_size / 2 + 1 = %d expected", bins, SYNTH_BINS);
    ry_synth* const c = k->core;
    const int B = k->n_streams;
    std::vector<SynthStream>& ent = k->ent;
    ent.assign((size_t)B, SynthStream());
    std::vector<long long> keep_from((size_t)B), k1s((size_t)B);
    long long rows = 0, new_rows = 0, pulses = 0, bound = 0;
    bool any = false;
    for (int b = 0; b < B; ++b) {
        const BankStream& t = k->s[(size_t)b];
        SynthStream& e = ent[(size_t)b];
        memset(&e, 0, sizeof e);
        const int n = n_frames[b];
        const bool fin = final && final[b];
        if (n < 0) return fail(RY_EINVAL, "stream %d has %d frames", b, n);
        if (n > SYNTH_MAX_FRAMES - new_rows) return fail(RY_EINVAL, "more than %d frames in one call", (int)SYNTH_MAX_FRAMES);
        const long long m = t.n_frames + n;
        if (fin && m < 1) return fail(RY_ESTATE, "stream %d: final on an empty stream", b);
        if (fin && y_length(c, m) < t.scanned) return fail(RY_ESTATE, "stream %d: %lld samples scanned, the signal has %lld", b, t.scanned, y_length(c, m));
        e.active = n > 0 || fin; e.final = fin;
        any = any || e.active;
        const long long kf = std::max(needed_frame(c, t.scanned, t.n_live > 0, t.first_idx), t.frame0);
        const long long kept = t.frame0 + (long long)t.f0.size() - kf;
        const long long k1 = e.active ? scan_end(c, m, fin, t.scanned) : t.scanned;
        const long long cap = e.active ? t.n_live + (k1 - t.scanned) + 1 : 0;
        if (pulses + cap > SYNTH_MAX_PULSES) return fail(RY_EINVAL, "more than %d samples in one call", (int)SYNTH_MAX_PULSES);
        keep_from[(size_t)b] = kf; k1s[(size_t)b] = k1;
        e.frame0 = kf; e.last_frame = m - 1; e.n0 = t.scanned; e.n1 = k1;
        e.row0 = (int)rows; e.rows = (int)(kept + n); e.kept = (int)kept; e.src_row0 = (int)(t.row0 + (kf - t.frame0)); e.new_row0 = (int)new_rows;
        e.pulse0 = (int)pulses; e.pulse_cap = (int)cap; e.n_live = t.n_live; e.seed_hash = t.seed_hash;
        e.done = e.fin = t.done;
        rows += kept + n; new_rows += n; pulses += cap;
        if (rows > 2LL * SYNTH_MAX_FRAMES) return fail(RY_EINVAL, "more than %d window rows in one call", 2 * (int)SYNTH_MAX_FRAMES);
        if (e.active) bound += k1 - t.done;
    }
    if (!any) return fail(RY_EINVAL, "no stream has a frame or ends");
    for (int b = 0; b < B; ++b) RY_TRY(check_f0(c, f0 + ent[(size_t)b].new_row0, n_frames[b], b, "stream"));
    if (bound > y_capacity) return fail(RY_EINVAL, "y holds %lld samples, this push may return up to %lld (ry_synth_bank_bound)", y_capacity, bound);

    const ry_stream_t st = k->ctx->stream;
    int* const cnt = k->counts;
    cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
    // room first: a buffer that grows waits for the stream, and a failure here leaves every stream as it was
    const int to = 1 - k->cur;
    if (rows > k->win_cap[to]) {
        RT_TRY(rt::stream_sync(st)); ++cnt[0];
        k->win[to].release();
        k->sp[to] = k->ap[to] = nullptr; k->win_cap[to] = 0;
        const long long cap = rows + rows / 2 + 16;
        RY_TRY(k->win[to].alloc(&k->sp[to], (size_t)cap * SYNTH_BINS));
        RY_TRY(k->win[to].alloc(&k->ap[to], (size_t)cap * SYNTH_BINS));
        k->win_cap[to] = cap;
    }
    static_assert(sizeof(SynthStream) % sizeof(double) == 0, "the stream table follows an array of doubles");
    const size_t ent_off = (size_t)rows, n_tab = ent_off + (size_t)B * (sizeof(SynthStream) / sizeof(double));
    auto grow = [&](DevBufBase& buf, long long need) { if (need > buf.cap) ++cnt[0]; return buf.grow(k->ctx, need); };
    RY_TRY(grow(c->d_pidx, pulses));
    RY_TRY(grow(c->d_pshift, pulses));
    RY_TRY(grow(c->d_pvoiced, pulses));
    RY_TRY(grow(k->d_tab, (long long)n_tab));
    RY_TRY(grow(k->d_ret, B));
    if (!on_device && new_rows > 0) {
        RY_TRY(grow(c->d_sp_many, new_rows * SYNTH_BINS));
        RY_TRY(grow(c->d_ap_many, new_rows * SYNTH_BINS));
    }
    // the windows' f0 on the host, then ONE upload: [rows] thresholded f0 | [streams] table
    k->pulses_valid = false;
    k->tab_host.assign(n_tab, 0.0);
    for (int b = 0; b < B; ++b) {
        BankStream& t = k->s[(size_t)b];
        const SynthStream& e = ent[(size_t)b];
        t.f0.erase(t.f0.begin(), t.f0.begin() + (keep_from[(size_t)b] - t.frame0));
        for (int i = 0; i < n_frames[b]; ++i) t.f0.push_back(threshold_f0(c, f0[e.new_row0 + i]));
        t.frame0 = keep_from[(size_t)b]; t.row0 = e.row0; t.n_frames += n_frames[b];
        if (!t.f0.empty()) memcpy(k->tab_host.data() + e.row0, t.f0.data(), t.f0.size() * sizeof(double));
        t.dbg_n = 0;
    }
    memcpy(k->tab_host.data() + ent_off, ent.data(), (size_t)B * sizeof(SynthStream));
    RT_TRY(rt::h2d(k->d_tab.ptr(), k->tab_host.data(), n_tab * sizeof(double), st)); ++cnt[2];
    const float *new_sp = sp, *new_ap = ap;
    if (!on_device && new_rows > 0) {
        RT_TRY(rt::h2d(c->d_sp_many.ptr(), sp, (size_t)new_rows * SYNTH_BINS * sizeof(float), st)); ++cnt[2];
        RT_TRY(rt::h2d(c->d_ap_many.ptr(), ap, (size_t)new_rows * SYNTH_BINS * sizeof(float), st)); ++cnt[2];
        new_sp = c->d_sp_many.ptr(); new_ap = c->d_ap_many.ptr();
    }
    const double* d_f0 = k->d_tab.ptr();
    const SynthStream* d_ent = (const SynthStream*)(k->d_tab.ptr() + ent_off);
    SynthGatherParams gp;
    memset(&gp, 0, sizeof gp);
    gp.bank = d_ent; gp.n_streams = B; gp.rows = (int)rows;
    gp.old_sp = k->sp[k->cur]; gp.old_ap = k->ap[k->cur]; gp.new_sp = new_sp; gp.new_ap = new_ap; gp.sp = k->sp[to]; gp.ap = k->ap[to];
    gp.c_idx = k->c_idx; gp.c_shift = k->c_shift; gp.c_voiced = k->c_voiced; gp.carry_cap = SYNTH_CARRY;
    gp.pidx = c->d_pidx.ptr(); gp.pshift = c->d_pshift.ptr(); gp.pvoiced = c->d_pvoiced.ptr();
    RY_LAUNCH(synth_gather, dim3((unsigned)std::max(rows, (long long)B), 3), 256, st, gp); ++cnt[1];
    RT_TRY(rt::last_error());
    k->cur = to; k->win_rows = rows;
    SynthScanParams cp = scan_params(c);
    cp.f0 = d_f0; cp.st = k->st; cp.bank = d_ent;
    RY_LAUNCH(synth_scan, dim3((unsigned)B), 256, st, cp); ++cnt[1];
    RT_TRY(rt::last_error());
    k->hs.resize((size_t)B);
    RT_TRY(rt::d2h(k->hs.data(), k->st, (size_t)B * sizeof(SynthScanState), st)); ++cnt[3];
    RT_TRY(rt::stream_sync(st)); ++cnt[0];                          // wait 1 of 2: pulse counts, overflow words, last indices (the host rows are free from here on)
    long long resp = 0, samples = 0;
    for (int b = 0; b < B; ++b) {
        BankStream& t = k->s[(size_t)b];
        SynthStream& e = ent[(size_t)b];
        e.out0 = samples; e.resp0 = (int)resp;
        if (!e.active) continue;
        const SynthScanState& h = k->hs[(size_t)b];
        if (h.overflow) return fail(RY_ESTATE, "stream %d: pulse list overflow (%d)", b, h.overflow);
        long long complete = 0, fin = 0;
        emit_range(e.final != 0, h.n_pulses, h.last_idx, t.done, k1s[(size_t)b], &complete, &fin);
        e.n_pulses = h.n_pulses; e.fin = fin;
        e.n_complete = fin - t.done > 0 ? (int)complete : 0;       // as `advance`: no sample, no response
        resp += e.n_complete; samples += fin - t.done;
        t.dbg_p0 = e.pulse0 + e.n_live; t.dbg_n = h.n_pulses - e.n_live;
    }
    memcpy(k->tab_host.data() + ent_off, ent.data(), (size_t)B * sizeof(SynthStream));
    RY_TRY(grow(c->d_resp, resp * SYNTH_FFT));
    if (!y_on_device) RY_TRY(grow(c->d_y, samples));
    RT_TRY(rt::h2d(k->d_tab.ptr() + ent_off, k->tab_host.data() + ent_off, (size_t)B * sizeof(SynthStream), st)); ++cnt[2];
    if (resp > 0) {
        SynthPulseParams pp = pulse_params(c);
        pp.sp = k->sp[to]; pp.ap = k->ap[to]; pp.bank = d_ent; pp.n_streams = B;
        RY_LAUNCH(synth_pulse, dim3((unsigned)resp), 256, st, pp); ++cnt[1];
        RT_TRY(rt::last_error());
    }
    if (samples > 0) {
        SynthOverlapParams op = overlap_params(c);
        op.s0 = 0; op.s1 = samples; op.bank = d_ent; op.n_streams = B;
        if (y_on_device) op.y = y;
        RY_LAUNCH(synth_overlap, dim3((unsigned)((samples + 255) / 256)), 256, st, op); ++cnt[1];
        RT_TRY(rt::last_error());
    }
    SynthRetireParams rp;
    memset(&rp, 0, sizeof rp);
    rp.bank = d_ent; rp.st = k->st; rp.pidx = c->d_pidx.ptr(); rp.pshift = c->d_pshift.ptr(); rp.pvoiced = c->d_pvoiced.ptr();
    rp.c_idx = k->c_idx; rp.c_shift = k->c_shift; rp.c_voiced = k->c_voiced; rp.carry_cap = SYNTH_CARRY; rp.out = k->d_ret.ptr();
    RY_LAUNCH(synth_retire, dim3((unsigned)B), 256, st, rp); ++cnt[1];
    RT_TRY(rt::last_error());
    if (samples > 0 && !y_on_device) { RT_TRY(rt::d2h(y, c->d_y.ptr(), (size_t)samples * sizeof(double), st)); ++cnt[3]; }
    k->ret.resize((size_t)B);
    RT_TRY(rt::d2h(k->ret.data(), k->d_ret.ptr(), (size_t)B * sizeof(SynthRetired), st)); ++cnt[3];
    RT_TRY(rt::stream_sync(st)); ++cnt[0];                          // wait 2 of 2: the samples and what synth_retire carried
    for (int b = 0; b < B; ++b) {
        BankStream& t = k->s[(size_t)b];
        const SynthStream& e = ent[(size_t)b];
        sample_offsets[b] = e.out0;
        if (!e.active) continue;
        if (k->ret[(size_t)b].overflow) return fail(RY_ESTATE, "stream %d: %d live pulses beyond the carry slot", b, k->ret[(size_t)b].overflow);
        if (e.final) { bank_reset_stream(t); continue; }
        t.scanned = e.n1; t.done = e.fin;
        t.n_live = k->ret[(size_t)b].n_live; t.first_idx = k->ret[(size_t)b].first_idx; t.last_idx = k->hs[(size_t)b].last_idx;
    }
    sample_offsets[B] = samples;
    k->pulses_valid = true;
    return RY_OK;
}

int ry_synth_bank_push(ry_synth_bank* k, const double* f0, const float* sp, const float* ap, const int* n_frames, const int* final, int bins,
                       int on_device, double* y, long long y_capacity, long long* sample_offsets) {
    return bank_push_frames(k, f0, sp, ap, n_frames, final, bins, on_device, y, y_capacity, sample_offsets, false);
}

int ry_synth_bank_push_dev(ry_synth_bank* k, const double* f0, const float* sp, const float* ap, const int* n_frames, const int* final, int bins,
                           int on_device, double* y_dev, long long y_capacity, long long* sample_offsets) {
    return bank_push_frames(k, f0, sp, ap, n_frames, final, bins, on_device, y_dev, y_capacity, sample_offsets, true);
}

int ry_synth_bank_debug_pulses(ry_synth_bank* k, int stream, long long* index, double* shift, int* voiced, int capacity, int* n) {
    RY_TRY(check_handle(k, "synthesizer bank"));
    if (!n) return fail(RY_EINVAL, "bad argument");
    *n = 0;
    if (stream < 0 || stream >= k->n_streams) return fail(RY_EINVAL, "stream %d of %d", stream, k->n_streams);
    if (!k->pulses_valid) return fail(RY_ESTATE, "no push since the bank was made or poisoned");
    const BankStream& t = k->s[(size_t)stream];
    *n = t.dbg_n;
    if (!index && !shift && !voiced) return RY_OK;                 // the count alone
    if (capacity < t.dbg_n) return fail(RY_EINVAL, "%d pulses, room for %d", t.dbg_n, capacity);
    const ry_stream_t st = k->ctx->stream;
    const ry_synth* c = k->core;
    if (index) RT_TRY(rt::d2h(index, c->d_pidx.ptr() + t.dbg_p0, (size_t)t.dbg_n * sizeof(long long), st));
    if (shift) RT_TRY(rt::d2h(shift, c->d_pshift.ptr() + t.dbg_p0, (size_t)t.dbg_n * sizeof(double), st));
    if (voiced) RT_TRY(rt::d2h(voiced, c->d_pvoiced.ptr() + t.dbg_p0, (size_t)t.dbg_n * sizeof(int), st));
    RT_TRY(rt::stream_sync(st));
    return RY_OK;
}

int ry_synth_bank_debug_poison(ry_synth_bank* k) {
    RY_TRY(check_handle(k, "synthesizer bank"));
    const ry_stream_t st = k->ctx->stream;
    k->pulses_valid = false;                                       // the pulse arrays are scratch: what the streams carry is in the carry slots
    RY_TRY(ry_synth_debug_poison(k->core));
    for (DevBufBase* b : k->scratch) RY_TRY(b->poison(st));
    const int idle = 1 - k->cur;
    if (k->sp[idle]) {
        RT_TRY(rt::dmemset(k->sp[idle], 0xff, (size_t)k->win_cap[idle] * SYNTH_BINS * sizeof(float), st));
        RT_TRY(rt::dmemset(k->ap[idle], 0xff, (size_t)k->win_cap[idle] * SYNTH_BINS * sizeof(float), st));
    }
    if (k->sp[k->cur]) {                                           // behind the windows of the set in use
        const size_t used = (size_t)k->win_rows * SYNTH_BINS, cap = (size_t)k->win_cap[k->cur] * SYNTH_BINS;
        RT_TRY(rt::dmemset(k->sp[k->cur] + used, 0xff, (cap - used) * sizeof(float), st));
        RT_TRY(rt::dmemset(k->ap[k->cur] + used, 0xff, (cap - used) * sizeof(float), st));
    }
    RT_TRY(rt::stream_sync(st));
    return RY_OK;
}

int ry_synth_bank_debug_counts(ry_synth_bank* k, int* out) {
    if (!k || !out) return fail(RY_EINVAL, "bad argument");
    for (int i = 0; i < 4; ++i) out[i] = k->counts[i];
    return RY_OK;
}

int ry_synth_bank_debug_rows(ry_synth_bank* k, int stream) {
    if (!k || stream < 0 || stream >= k->n_streams) return fail(RY_EINVAL, "bad argument");
    return (int)k->s[(size_t)stream].f0.size();
}

}  // extern "C"
