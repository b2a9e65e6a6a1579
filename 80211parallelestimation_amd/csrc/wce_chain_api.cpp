// wce_chain_api.cpp -- C ABI (include/wce.h) of the receive and transmit chain: the front end, synchronisation,
// demodulation and tracking, receive diversity, decoding, re-encoding, payload framing, the transmitter and the
// channel.  Every call checks its arguments first, then takes the context's device and launches: nothing of the
// context is read before the checks hold, and a count of 0 returns WCE_OK without a launch.  A check_* function
// holds what several calls ask alike and returns what is wrong (null: nothing); the entry point puts its name in
// front.  The front-end and synchronisation calls' messages carry no name.
#include <cmath>
#include <string>

#include "wce_api_check.h"

// the refusal of a call that puts its name in front: const Refuse refuse{"wce_combine"}; return refuse("...");
namespace {
struct Refuse {
    const char *call;
    int operator()(const char *what) const { return fail(WCE_EINVAL, (std::string(call) + ": " + what).c_str()); }
};
}  // namespace

static int launched(int rc, const char *what) { return rc ? fail(rc, what) : WCE_OK; }

static const double *re(const wce_complex *p) { return reinterpret_cast<const double *>(p); }
static double *re(wce_complex *p) { return reinterpret_cast<double *>(p); }

namespace wce {
// 802.11a's short sequence on the bins k = -24, -20 .. 24 without DC: the signs of sqrt(13/6) (1 + j)
static const int kShortSign[12] = {+1, -1, +1, -1, -1, +1, -1, -1, +1, +1, +1, +1};

void short_field_period(double *t32)
{
    const long double pi = 3.14159265358979323846264338327950288L;
    const long double amp = sqrtl(13.0L / 6.0L) / 64.0L;
    for (int m = 0; m < 16; ++m) {
        // t[m] = (1/64) sum_k S_k exp(2 pi i k m / 64), k = 4 j: the twiddle's argument is (j m mod 16) / 16 of a turn
        long double re = 0.0L, im = 0.0L;
        for (int i = 0; i < 12; ++i) {
            const int j = i < 6 ? i - 6 : i - 5;
            const int turn = ((j * m) % 16 + 16) % 16;
            const long double cs = cosl(2.0L * pi * turn / 16.0L), sn = sinl(2.0L * pi * turn / 16.0L);
            re += kShortSign[i] * (cs - sn);   // (1 + j) (cs + j sn)
            im += kShortSign[i] * (cs + sn);
        }
        t32[2 * m] = (double)(amp * re);
        t32[2 * m + 1] = (double)(amp * im);
    }
}
}  // namespace wce

// ---------------------------------------------------------------- shared checks that are templates (no C linkage)
// what wce_front_end_sync (stf == false: one threshold, given twice) and wce_front_end_sync_stf ask of the window,
// the thresholds, the backoff and the buffers both have; fills those fields of `a`
template <class Args>
static const char *check_sync(bool stf, const wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                              int64_t n_frames, const wce_complex *ltf, double threshold, double threshold_ltf,
                              int32_t backoff, int32_t *start, Args *a)
{
    if (n_frames < 0) return "n_frames < 0";
    if (capture_len < 2 * WCE_FFT_SIZE + (stf ? 16 : 0) || capture_len >= (int64_t)1 << 31)
        return stf ? "capture_len outside [144, 2^31)" : "capture_len outside [128, 2^31)";
    if (capture_stride < capture_len) return "capture_stride < capture_len";
    if (!in_unit(threshold)) return stf ? "threshold_stf outside [0, 1]" : "threshold outside [0, 1]";
    if (!in_unit(threshold_ltf)) return "threshold_ltf outside [0, 1]";
    if (backoff < 0 || backoff > 31) return "backoff outside [0, 31]";
    if (!start || misaligned(start, 4)) return "start null or not 4-byte aligned";
    if (!ltf || misaligned(ltf, 16)) return "ltf null or not 16-byte aligned";
    if (!capture || misaligned(capture, 16)) return "capture null or not 16-byte aligned";
    a->capture = re(capture);
    a->ltf = re(ltf);
    a->stride = capture_stride; a->len = capture_len; a->n = n_frames;
    a->backoff = backoff; a->start = start;
    return nullptr;
}

// what wce_demodulate and wce_track_demodulate (more: it has an output beyond the five) ask of the frames' pointers,
// of h, modulation, flags, scale and of the five outputs both have; fills those fields of `a`
template <class Par, class Out, class Args>
static const char *check_demod(const wce_frames *in, const Par *p, const Out *out, bool more, uint32_t flag_bits,
                               Args *a)
{
    if (!in || !p || !out) return "null frames, parameters or outputs";
    if (!in->tx || !in->rx) return "tx/rx required";
    if (!p->h) return "h required";
    if (!out->eq && !out->sym && !out->theta && !out->evm && !out->nerr && !more) return "no output requested";
    if (p->h_stride < wce::NSC) return "h_stride < 53";
    if (mod_K(p->modulation) == 0.0) return "unknown modulation";
    if (p->flags & ~flag_bits) return "unknown flag bits";
    if (!positive_finite(p->scale)) return "scale not positive and finite";
    const int64_t n = in->n_frames;
    if (out->eq && !strides_hold(n, out->eq_frame_stride, out->eq_block_stride, wce::NSC)) return "eq strides too small";
    if (out->sym && !strides_hold(n, out->sym_frame_stride, out->sym_block_stride, wce::NSC))
        return "sym strides too small";
    if (misaligned(out->theta, 8) || misaligned(out->evm, 8)) return "theta or evm not 8-byte aligned";
    if (misaligned(out->nerr, 4)) return "nerr not 4-byte aligned";
    a->tx = re(in->tx);
    a->rx = re(in->rx);
    a->h = re(p->h);
    a->fs = in->frame_stride; a->bs = in->block_stride; a->hs = p->h_stride; a->n = n;
    a->mod = p->modulation; a->flags = p->flags;
    a->scale = p->scale; a->d = p->scale * mod_K(p->modulation);
    a->eq = re(out->eq);
    a->sym = out->sym; a->theta = out->theta; a->evm = out->evm; a->nerr = out->nerr;
    a->eqfs = out->eq_frame_stride; a->eqbs = out->eq_block_stride;
    a->symfs = out->sym_frame_stride; a->symbs = out->sym_block_stride;
    return nullptr;
}

extern "C" {

// ---------------------------------------------------------------- front end
// the _at calls' window: start[] and capture_len (win); at == false: neither is looked at
static int check_window(bool at, const int32_t *start, int64_t win, int64_t stride)
{
    if (!at) return WCE_OK;
    if (!start) return fail(WCE_EINVAL, "null start");
    if (misaligned(start, 4)) return fail(WCE_EINVAL, "start not 4-byte aligned");
    if (win < 2 * WCE_FFT_SIZE || win >= (int64_t)1 << 31) return fail(WCE_EINVAL, "capture_len outside [128, 2^31)");
    if (stride < win) return fail(WCE_EINVAL, "capture_stride < capture_len");
    return WCE_OK;
}

// cfo == null: the plain build (sample_offset is not looked at).  at: the per-frame-start build, frame f's
// packet at samples[f*packet_stride + start[f] + 128 + sample_offset] of a window of win samples
static int front_blocks(wce_ctx *c, const wce_complex *samples, int64_t packet_stride, int64_t n_frames,
                        int32_t n_blocks, const double *cfo, int64_t sample_offset, wce_complex *sym,
                        int64_t frame_stride, int64_t block_stride, void *stream, bool at = false,
                        const int32_t *start = nullptr, int64_t win = 0)
{
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (n_frames < 0 || n_blocks < 1) return fail(WCE_EINVAL, "n_frames < 0 or n_blocks < 1");
    if (n_frames == 0) return WCE_OK;
    if (!samples || !sym) return fail(WCE_EINVAL, "null buffer");
    if (int rc = check_window(at, start, win, packet_stride)) return rc;
    if (!at && packet_stride < (int64_t)n_blocks * WCE_SAMPLES_PER_BLOCK)
        return fail(WCE_EINVAL, "packet_stride < 80 n_blocks");
    if (block_stride < wce::NSC || frame_stride < (int64_t)(n_blocks - 1) * block_stride + wce::NSC)
        return fail(WCE_EINVAL, "output strides too small");
    if (n_frames * n_blocks >= (int64_t)1 << 31) return fail(WCE_EINVAL, "n_frames * n_blocks >= 2^31");
    if (cfo || at) {
        if (misaligned(cfo, 8)) return fail(WCE_EINVAL, "cfo not 8-byte aligned");
        if (sample_offset >= (int64_t)1 << 31 || sample_offset <= -((int64_t)1 << 31))
            return fail(WCE_EINVAL, "|sample_offset| >= 2^31");
    }
    wce::FrontArgs a{};
    a.src = re(samples);
    a.dst = re(sym);
    a.ps = packet_stride; a.off = WCE_SAMPLES_PER_BLOCK - WCE_FFT_SIZE; a.fs = frame_stride; a.bs = block_stride;
    a.n_units = (uint32_t)(n_frames * n_blocks); a.nb = (uint32_t)n_blocks;
    a.cfo = const_cast<double *>(cfo);   // est = 0: read only
    a.n0 = cfo ? sample_offset + a.off : 0;
    if (at) {   // the packet follows the 128-sample field; the time axis (n0) is the CFO call's
        a.n0 = sample_offset + a.off;
        a.off += 2 * WCE_FFT_SIZE + sample_offset;
        a.start = start; a.win = win;
        a.span = (int64_t)(n_blocks - 1) * WCE_SAMPLES_PER_BLOCK + WCE_FFT_SIZE;
    }
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_front(a, false, stream), "front end launch");
}

int wce_front_end_blocks(wce_ctx *c, const wce_complex *samples, int64_t packet_stride, int64_t n_frames,
                         int32_t n_blocks, wce_complex *sym, int64_t frame_stride, int64_t block_stride,
                         void *stream)
{
    return front_blocks(c, samples, packet_stride, n_frames, n_blocks, nullptr, 0, sym, frame_stride, block_stride,
                        stream);
}

int wce_front_end_blocks_cfo(wce_ctx *c, const wce_complex *samples, int64_t packet_stride, int64_t n_frames,
                             int32_t n_blocks, const double *cfo, int64_t sample_offset, wce_complex *sym,
                             int64_t frame_stride, int64_t block_stride, void *stream)
{
    return front_blocks(c, samples, packet_stride, n_frames, n_blocks, cfo, sample_offset, sym, frame_stride,
                        block_stride, stream);
}

int wce_front_end_blocks_at(wce_ctx *c, const wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                            int64_t n_frames, int32_t n_blocks, const int32_t *start, const double *cfo,
                            int64_t sample_offset, wce_complex *sym, int64_t frame_stride, int64_t block_stride,
                            void *stream)
{
    return front_blocks(c, capture, capture_stride, n_frames, n_blocks, cfo, sample_offset, sym, frame_stride,
                        block_stride, stream, true, start, capture_len);
}

// cfo == null: the plain build.  start != null: the per-frame-start build, lptot the capture windows of
// lptot_len samples, frame f's field at lptot[f*lptot_stride + start[f] + (0..127)]
static int front_preamble(wce_ctx *c, const wce_complex *lptot, int64_t lptot_stride, int64_t lptot_len,
                          int64_t n_frames, wce_complex *pre_fft, int64_t pre_stride, double *ow2, double *cfo,
                          int estimate, void *stream, bool at = false, const int32_t *start = nullptr)
{
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (n_frames < 0) return fail(WCE_EINVAL, "n_frames < 0");
    if (n_frames == 0) return WCE_OK;
    if (!lptot || !pre_fft) return fail(WCE_EINVAL, "null buffer");
    if (int rc = check_window(at, start, lptot_len, lptot_stride)) return rc;
    if (at && estimate && !cfo) return fail(WCE_EINVAL, "estimate without cfo");
    if (lptot_len < 2 * WCE_FFT_SIZE || lptot_stride < lptot_len) return fail(WCE_EINVAL, "lptot_len < 128 or stride < len");
    if (pre_stride < wce::NSC) return fail(WCE_EINVAL, "pre_stride < 53");
    if (n_frames >= (int64_t)1 << 31) return fail(WCE_EINVAL, "n_frames >= 2^31");
    if (misaligned(cfo, 8)) return fail(WCE_EINVAL, "cfo not 8-byte aligned");
    wce::FrontArgs a{};
    a.src = re(lptot);
    a.dst = re(pre_fft);
    a.ow2 = ow2;
    a.ps = lptot_stride; a.off = lptot_len - 2 * WCE_FFT_SIZE; a.fs = pre_stride; a.bs = 0;
    a.n_units = (uint32_t)n_frames; a.nb = 1;
    a.cfo = cfo;
    a.n0 = -2 * WCE_FFT_SIZE;   // the long training field ends at n = 0
    a.est = cfo && estimate;
    if (at) { a.off = 0; a.start = start; a.win = lptot_len; a.span = 2 * WCE_FFT_SIZE; }
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_front(a, true, stream), "front end launch");
}

int wce_front_end_preamble(wce_ctx *c, const wce_complex *lptot, int64_t lptot_stride, int64_t lptot_len,
                           int64_t n_frames, wce_complex *pre_fft, int64_t pre_stride, double *ow2, void *stream)
{
    return front_preamble(c, lptot, lptot_stride, lptot_len, n_frames, pre_fft, pre_stride, ow2, nullptr, 0, stream);
}

int wce_front_end_preamble_cfo(wce_ctx *c, const wce_complex *lptot, int64_t lptot_stride, int64_t lptot_len,
                               int64_t n_frames, wce_complex *pre_fft, int64_t pre_stride, double *ow2, double *cfo,
                               int estimate, void *stream)
{
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (!cfo) return fail(WCE_EINVAL, "null cfo");
    return front_preamble(c, lptot, lptot_stride, lptot_len, n_frames, pre_fft, pre_stride, ow2, cfo, estimate,
                          stream);
}

int wce_front_end_preamble_at(wce_ctx *c, const wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                              int64_t n_frames, const int32_t *start, wce_complex *pre_fft, int64_t pre_stride,
                              double *ow2, double *cfo, int estimate, void *stream)
{
    return front_preamble(c, capture, capture_stride, capture_len, n_frames, pre_fft, pre_stride, ow2, cfo, estimate,
                          stream, true, start);
}

// ---------------------------------------------------------------- synchronisation
int wce_front_end_sync(wce_ctx *c, const wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                       int64_t n_frames, const wce_complex *ltf, double threshold, int32_t backoff, int32_t *start,
                       double *metric, void *stream)
{
    if (!c) return fail(WCE_EINVAL, "null ctx");
    wce::SyncArgs a{};
    if (const char *bad = check_sync(false, capture, capture_stride, capture_len, n_frames, ltf, threshold, threshold,
                                     backoff, start, &a))
        return fail(WCE_EINVAL, bad);
    if (misaligned(metric, 8)) return fail(WCE_EINVAL, "metric not 8-byte aligned");
    if (n_frames == 0) return WCE_OK;
    a.threshold = threshold; a.metric = metric;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_sync(a, wce::ctx_cus(c), stream), "sync launch");
}

int wce_front_end_sync_stf(wce_ctx *c, const wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                           int64_t n_frames, const wce_complex *ltf, double threshold_stf, double threshold_ltf,
                           int32_t backoff, int32_t *start, double *cfo, double *metric_stf, double *metric_ltf,
                           void *stream)
{
    if (!c) return fail(WCE_EINVAL, "null ctx");
    wce::SyncStfArgs a{};
    if (const char *bad = check_sync(true, capture, capture_stride, capture_len, n_frames, ltf, threshold_stf,
                                     threshold_ltf, backoff, start, &a))
        return fail(WCE_EINVAL, bad);
    if (!cfo || misaligned(cfo, 8)) return fail(WCE_EINVAL, "cfo null or not 8-byte aligned");
    if (misaligned(metric_stf, 8) || misaligned(metric_ltf, 8)) return fail(WCE_EINVAL, "metric not 8-byte aligned");
    if (n_frames == 0) return WCE_OK;
    a.threshold_stf = threshold_stf; a.threshold_ltf = threshold_ltf;
    a.cfo = cfo; a.metric_stf = metric_stf; a.metric_ltf = metric_ltf;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_sync_stf(a, wce::ctx_cus(c), stream), "sync_stf launch");
}

int wce_short_field(wce_ctx *c, double amplitude, wce_complex *wave, int64_t wave_stride, int64_t n_frames,
                    void *stream)
{
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (n_frames < 0) return fail(WCE_EINVAL, "n_frames < 0");
    if (!wave || misaligned(wave, 16)) return fail(WCE_EINVAL, "wave null or not 16-byte aligned");
    if (wave_stride < wce::SHORT_FIELD_LEN) return fail(WCE_EINVAL, "wave_stride < 160");
    if (!std::isfinite(amplitude)) return fail(WCE_EINVAL, "amplitude not finite");
    if (n_frames == 0) return WCE_OK;
    wce::ShortFieldArgs a{};
    a.wave = re(wave);
    a.stride = wave_stride; a.n = n_frames; a.amplitude = amplitude;
    wce::short_field_period(a.t);
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_short_field(a, wce::ctx_cus(c), stream), "short field launch");
}

// ---------------------------------------------------------------- demodulation and per-block tracking
// the frames, by the estimator's rules for the fields the two calls read (block, semantics and the preambles are
// ignored); its messages come without the call's name
static int check_demod_frames(const wce_frames *in)
{
    wce_frames fr = *in;
    fr.rx_pre = fr.tx_pre = nullptr;
    fr.block = 0;
    fr.semantics = WCE_SEM_C;
    return wce::api_check_frames(&fr, true);
}

int wce_demodulate(wce_ctx *c, const wce_frames *in, const wce_demod *p, const wce_demod_out *out, void *stream)
{
    const Refuse refuse{"wce_demodulate"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    wce::DemodArgs a{};
    if (const char *bad = check_demod(in, p, out, false, WCE_DEMOD_TRACK | WCE_DEMOD_REF_TX, &a)) return refuse(bad);
    if (misaligned(p->h, 16) || misaligned(p->h_lt, 16) || misaligned(out->eq, 16))
        return refuse("h, h_lt or eq not 16-byte aligned");
    if (int rc = check_demod_frames(in)) return rc;
    if (a.n == 0) return WCE_OK;
    a.hlt = re(p->h_lt);
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_demod(a, stream), "demod launch");
}

int wce_track_demodulate(wce_ctx *c, const wce_frames *in, const wce_track *p, const wce_track_out *out, void *stream)
{
    const Refuse refuse{"wce_track_demodulate"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    wce::TrackArgs a{};
    if (const char *bad = check_demod(in, p, out, out && (out->h_blocks || out->h_last),
                                      WCE_TRACK_PHASE | WCE_TRACK_REF_TX | WCE_TRACK_KNOWN_TX, &a))
        return refuse(bad);
    if (!in_unit(p->mu)) return refuse("mu outside [0, 1]");
    if (p->beta < 0 || p->beta > 4) return refuse("beta outside 0..4");
    if (out->h_blocks && !strides_hold(a.n, out->hb_frame_stride, out->hb_block_stride, wce::NSC))
        return refuse("h_blocks strides too small");
    if (out->h_last && out->h_last_stride < wce::NSC) return refuse("h_last_stride < 53");
    if (misaligned(p->h, 16) || misaligned(out->eq, 16)) return refuse("h or eq not 16-byte aligned");
    if (misaligned(out->h_blocks, 16) || misaligned(out->h_last, 16))
        return refuse("h_blocks or h_last not 16-byte aligned");
    if (int rc = check_demod_frames(in)) return rc;
    if (a.n == 0) return WCE_OK;
    a.mu = p->mu; a.beta = p->beta;
    a.hb = re(out->h_blocks);
    a.hbfs = out->hb_frame_stride; a.hbbs = out->hb_block_stride;
    a.hl = re(out->h_last);
    a.hls = out->h_last_stride;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_track(a, stream), "track launch");
}

// ---------------------------------------------------------------- receive diversity
// A branches of stride s on top of frames [n][15][53] of strides fs / bs: no two branches share an element where
// the branch stride spans a whole branch, or fits the branches inside a block stride, or between frame and block.
// 128-bit products: the strides are the caller's
static bool branches_apart(int64_t A, int64_t s, int64_t n, int64_t fs, int64_t bs)
{
    typedef __int128 i128;
    if (A <= 1) return true;
    if (s < wce::NSC) return false;
    const i128 blocks = (i128)(wce::NBLK - 1) * bs + wce::NSC, all = (i128)(A - 1) * s;
    if ((i128)s >= (i128)(n > 1 ? n - 1 : 0) * fs + blocks) return true;
    if (all + wce::NSC <= (i128)bs) return true;
    return (i128)s >= blocks && all + blocks <= (i128)fs;
}
// the same for rows [n][53] of stride hs
static bool rows_apart(int64_t A, int64_t s, int64_t n, int64_t hs)
{
    typedef __int128 i128;
    if (A <= 1) return true;
    if (s < wce::NSC) return false;
    if ((i128)s >= (i128)(n > 1 ? n - 1 : 0) * hs + wce::NSC) return true;
    return (i128)(A - 1) * s + wce::NSC <= (i128)hs;
}

int wce_combine(wce_ctx *c, const wce_combine_par *p, int64_t n_frames, const wce_combine_out *out, void *stream)
{
    const Refuse refuse{"wce_combine"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (!p || !out) return refuse("null parameters or outputs");
    if (!p->rx || !p->h) return refuse("rx and h required");
    if (!out->rx && !out->h) return refuse("no output requested");
    const int64_t A = p->n_branches, n = n_frames;
    if (A < 1 || A > WCE_COMBINE_MAX_BRANCHES) return refuse("n_branches outside 1..8");
    if (!count_holds(n)) return refuse("n_frames < 0 or > 2^31 - 1");
    if (!strides_hold(n, p->rx_frame_stride, p->rx_block_stride, wce::NSC)) return refuse("rx strides too small");
    if (p->h_stride < wce::NSC) return refuse("h_stride < 53");
    if (out->rx && !strides_hold(n, out->rx_frame_stride, out->rx_block_stride, wce::NSC))
        return refuse("output rx strides too small");
    if (out->h && out->h_stride < wce::NSC) return refuse("output h_stride < 53");
    if (!branches_apart(A, p->rx_branch_stride, n, p->rx_frame_stride, p->rx_block_stride))
        return refuse("rx_branch_stride makes branches overlap");
    if (!rows_apart(A, p->h_branch_stride, n, p->h_stride)) return refuse("h_branch_stride makes branches overlap");
    if (p->ow2 && A > 1 && p->ow2_branch_stride < n) return refuse("ow2_branch_stride < n_frames");
    if (misaligned(p->rx, 16) || misaligned(p->h, 16) || misaligned(out->rx, 16) || misaligned(out->h, 16))
        return refuse("rx, h or an output not 16-byte aligned");
    if (misaligned(p->ow2, 8)) return refuse("ow2 not 8-byte aligned");
    if (n == 0) return WCE_OK;
    wce::CombineArgs a{};
    a.rx = re(p->rx);
    a.h = re(p->h);
    a.ow2 = p->ow2;
    a.rbs = A > 1 ? p->rx_branch_stride : 0; a.rfs = p->rx_frame_stride; a.rks = p->rx_block_stride;
    a.hbs = A > 1 ? p->h_branch_stride : 0; a.hs = p->h_stride;
    a.obs = A > 1 ? p->ow2_branch_stride : 0; a.n = n; a.na = (int32_t)A;
    a.orx = re(out->rx);
    a.ofs = out->rx_frame_stride; a.oks = out->rx_block_stride;
    a.oh = re(out->h);
    a.ohs = out->h_stride;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_combine(a, stream), "combine launch");
}

int wce_sync_share(wce_ctx *c, int32_t n_branches, int64_t branch_stride, int64_t n_packets, const double *metric,
                   int32_t *start, double *cfo, void *stream)
{
    const Refuse refuse{"wce_sync_share"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (!metric || misaligned(metric, 8)) return refuse("metric null or not 8-byte aligned");
    if (!start && !cfo) return refuse("start and cfo both null");
    if (misaligned(start, 4)) return refuse("start not 4-byte aligned");
    if (misaligned(cfo, 8)) return refuse("cfo not 8-byte aligned");
    if (n_branches < 1 || n_branches > WCE_COMBINE_MAX_BRANCHES) return refuse("n_branches outside 1..8");
    if (!count_holds(n_packets)) return refuse("n_packets < 0 or > 2^31 - 1");
    if (n_branches > 1 && branch_stride < n_packets) return refuse("branch_stride < n_packets");
    if (n_packets == 0) return WCE_OK;
    wce::SyncShareArgs a{};
    a.metric = metric; a.start = start; a.cfo = cfo;
    a.bs = n_branches > 1 ? branch_stride : 0; a.n = n_packets; a.na = n_branches;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_sync_share(a, stream), "sync_share launch");
}

// ---------------------------------------------------------------- decoding
int wce_decode_info_bits(int32_t modulation, int32_t rate)
{
    const int T = wce::decode_info_bits(modulation, rate);
    return T < 0 ? fail(WCE_EINVAL, "wce_decode_info_bits: unknown modulation or rate") : T;
}

// what both soft demappers ask of eq, modulation, scale, n_frames and llr, none of them null; fills those fields of `a`
static const char *check_demap(const wce_complex *eq, int64_t eq_frame_stride, int64_t eq_block_stride,
                               int32_t modulation, double scale, int64_t n, float *llr, int64_t llr_frame_stride,
                               int64_t llr_block_stride, wce::DemapArgs *a)
{
    if (mod_K(modulation) == 0.0) return "unknown modulation";
    if (!positive_finite(scale)) return "scale not positive and finite";
    if (!count_holds(n)) return "n_frames < 0 or > 2^31 - 1";
    if (!strides_hold(n, eq_frame_stride, eq_block_stride, wce::NSC)) return "eq strides too small";
    if (!strides_hold(n, llr_frame_stride, llr_block_stride, 48 * (int64_t)modulation)) return "llr strides too small";
    if (misaligned(llr, 4)) return "llr not 4-byte aligned";
    a->eq = re(eq);
    a->efs = eq_frame_stride; a->ebs = eq_block_stride; a->n = n;
    a->mod = modulation; a->d = scale * mod_K(modulation);
    a->llr = llr; a->lfs = llr_frame_stride; a->lbs = llr_block_stride;
    return nullptr;
}

int wce_soft_demap(wce_ctx *c, const wce_complex *eq, int64_t eq_frame_stride, int64_t eq_block_stride,
                   const wce_demod *p, int64_t n, float *llr, int64_t llr_frame_stride, int64_t llr_block_stride,
                   void *stream)
{
    const Refuse refuse{"wce_soft_demap"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (!eq || !p || !llr) return refuse("null eq, parameters or llr");
    if (!p->h) return refuse("h required");
    if (p->h_stride < wce::NSC) return refuse("h_stride < 53");
    wce::DemapArgs a{};
    if (const char *bad = check_demap(eq, eq_frame_stride, eq_block_stride, p->modulation, p->scale, n, llr,
                                      llr_frame_stride, llr_block_stride, &a))
        return refuse(bad);
    if (misaligned(eq, 16) || misaligned(p->h, 16) || misaligned(p->h_lt, 16))
        return refuse("eq, h or h_lt not 16-byte aligned");
    if (n == 0) return WCE_OK;
    a.h = re(p->h);
    a.hlt = re(p->h_lt);
    a.hs = p->h_stride;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_demap(a, stream), "soft demap launch");
}

int wce_soft_demap_blocks(wce_ctx *c, const wce_complex *eq, int64_t eq_frame_stride, int64_t eq_block_stride,
                          const wce_complex *hb, int64_t hb_frame_stride, int64_t hb_block_stride, int32_t modulation,
                          double scale, int64_t n, float *llr, int64_t llr_frame_stride, int64_t llr_block_stride,
                          void *stream)
{
    const Refuse refuse{"wce_soft_demap_blocks"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (!eq || !hb || !llr) return refuse("null eq, hb or llr");
    wce::DemapArgs a{};
    if (const char *bad = check_demap(eq, eq_frame_stride, eq_block_stride, modulation, scale, n, llr,
                                      llr_frame_stride, llr_block_stride, &a))
        return refuse(bad);
    if (!strides_hold(n, hb_frame_stride, hb_block_stride, wce::NSC)) return refuse("hb strides too small");
    if (misaligned(eq, 16) || misaligned(hb, 16)) return refuse("eq or hb not 16-byte aligned");
    if (n == 0) return WCE_OK;
    a.hb = re(hb);
    a.hbfs = hb_frame_stride; a.hbbs = hb_block_stride;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_demap(a, stream), "soft demap launch");
}

int wce_viterbi_decode(wce_ctx *c, const float *llr, int64_t llr_frame_stride, int64_t llr_block_stride,
                       int32_t modulation, int32_t rate, uint32_t flags, int64_t n, uint8_t *bits,
                       int64_t bits_stride, const uint8_t *ref_bits, int64_t ref_stride, uint32_t *nbiterr,
                       void *stream)
{
    const Refuse refuse{"wce_viterbi_decode"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (!llr) return refuse("null llr");
    const int T = wce::decode_info_bits(modulation, rate);
    if (T < 0) return refuse("unknown modulation or rate");
    if (flags & ~WCE_DEC_TERMINATED) return refuse("unknown flag bits");
    if (!bits && !nbiterr) return refuse("no output requested");
    if (nbiterr && !ref_bits) return refuse("nbiterr needs ref_bits");
    if (!count_holds(n)) return refuse("n_frames < 0 or > 2^31 - 1");
    if (!strides_hold(n, llr_frame_stride, llr_block_stride, 48 * (int64_t)modulation))
        return refuse("llr strides too small");
    const int64_t nbytes = (T + 7) / 8;
    if (bits && bits_stride < nbytes) return refuse("bits_stride < ceil(T / 8)");
    if (ref_bits && ref_stride < nbytes) return refuse("ref_stride < ceil(T / 8)");
    if (misaligned(llr, 4) || misaligned(nbiterr, 4)) return refuse("llr or nbiterr not 4-byte aligned");
    if (n == 0) return WCE_OK;
    wce::ViterbiArgs a{};
    a.llr = llr; a.lfs = llr_frame_stride; a.lbs = llr_block_stride; a.n = n;
    a.mod = modulation; a.rate = rate; a.T = T; a.flags = flags;
    a.bits = bits; a.bits_stride = bits_stride;
    a.ref = ref_bits; a.ref_stride = ref_stride;
    a.nbiterr = nbiterr;
    DeviceGuard g(wce::ctx_device(c));
    const int rc = wce::launch_viterbi(a, stream);
    if (rc == WCE_EINVAL) return refuse("the survivor memory of T steps does not fit the LDS");
    return launched(rc, "viterbi launch");
}

// ---------------------------------------------------------------- decision-directed estimation
int wce_reencode(wce_ctx *c, const wce_reencode_par *p, const wce_frames *in, int64_t n,
                 const wce_reencode_out *out, void *stream)
{
    const Refuse refuse{"wce_reencode"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (!p || !out) return refuse("null parameters or outputs");
    if (!p->bits) return refuse("bits required");
    if (!out->tx && !out->h) return refuse("no output requested");
    if (out->h && (!in || !in->rx)) return refuse("h needs the frames' rx");
    if (!count_holds(n)) return refuse("n_frames < 0 or > 2^31 - 1");
    if (in && in->n_frames != n) return refuse("the frames' n_frames differs from n_frames");
    const int T = wce::decode_info_bits(p->modulation, p->rate);
    if (T < 0) return refuse("unknown modulation or rate");
    if (!positive_finite(p->scale)) return refuse("scale not positive and finite");
    if (p->bits_stride < (T + 7) / 8) return refuse("bits_stride < ceil(T / 8)");
    if (out->tx && !strides_hold(n, out->tx_frame_stride, out->tx_block_stride, wce::NSC))
        return refuse("tx strides too small");
    if (in && !strides_hold(n, in->frame_stride, in->block_stride, wce::NSC))
        return refuse("the frames' strides too small");
    if (out->h && out->h_stride < wce::NSC) return refuse("h_stride < 53");
    if (misaligned(out->tx, 16) || misaligned(out->h, 16) || (in && (misaligned(in->rx, 16) || misaligned(in->tx, 16))))
        return refuse("tx, h or the frames' rx or tx not 16-byte aligned");
    if (misaligned(p->theta, 8)) return refuse("theta not 8-byte aligned");
    if (n == 0) return WCE_OK;
    wce::ReencodeArgs a{};
    a.bits = p->bits; a.bits_stride = p->bits_stride;
    a.theta = out->h ? p->theta : nullptr;
    a.ptx = in ? re(in->tx) : nullptr;
    a.rx = out->h ? re(in->rx) : nullptr;
    if (in) { a.fs = in->frame_stride; a.bs = in->block_stride; }
    a.n = n; a.mod = p->modulation; a.rate = p->rate;
    a.scale = p->scale; a.d = p->scale * mod_K(p->modulation);
    a.tx = re(out->tx); a.tfs = out->tx_frame_stride; a.tbs = out->tx_block_stride;
    a.h = re(out->h); a.hs = out->h_stride;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_reencode(a, stream), "reencode launch");
}

// ---------------------------------------------------------------- framing the payload
int wce_psdu_max_len(int32_t modulation, int32_t rate)
{
    const int T = wce::decode_info_bits(modulation, rate);
    return T < 0 ? fail(WCE_EINVAL, "wce_psdu_max_len: unknown modulation or rate") : (T - 22) / 8;
}

// what both calls ask of p, n_frames and bits_stride.  Fills T, nbytes, max_len, length, seed, lengths, seeds,
// bits_stride and n of `a`
static const char *check_psdu(const wce_psdu_par *p, int64_t n, int64_t bits_stride, bool framing, wce::PsduArgs *a)
{
    const int T = wce::decode_info_bits(p->modulation, p->rate);
    if (T < 0) return "unknown modulation or rate";
    const int32_t max = (T - 22) / 8;
    if (!p->lengths && (p->length < 4 || p->length > max)) return "length outside 4..max";
    if (framing && !p->seeds && (p->seed < 1 || p->seed > 127)) return "seed outside 1..127";
    if (bits_stride < (T + 7) / 8) return "bits_stride < ceil(T / 8)";
    if (misaligned(p->lengths, 4)) return "lengths not 4-byte aligned";
    if (!count_holds(n)) return "n_frames < 0 or > 2^31 - 1";
    a->T = T; a->nbytes = (T + 7) / 8; a->max_len = max;
    a->length = p->lengths ? max : p->length;
    a->seed = framing && !p->seeds ? p->seed : 1;
    a->lengths = p->lengths;
    a->seeds = framing ? p->seeds : nullptr;
    a->bits_stride = bits_stride; a->n = n;
    return nullptr;
}

int wce_psdu_frame(wce_ctx *c, const wce_psdu_par *p, const uint8_t *payload, int64_t payload_stride, int64_t n,
                   uint8_t *bits, int64_t bits_stride, void *stream)
{
    const Refuse refuse{"wce_psdu_frame"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (!p || !bits) return refuse("null parameters or bits");
    wce::PsduArgs a{};
    if (const char *bad = check_psdu(p, n, bits_stride, true, &a)) return refuse(bad);
    if (!payload && (p->lengths || p->length > 4)) return refuse("payload NULL with length > 4 or with lengths");
    if (payload && payload_stride < a.length - 4) return refuse("payload_stride < L - 4 (max - 4 with lengths)");
    if (n == 0) return WCE_OK;
    a.payload = payload; a.payload_stride = payload ? payload_stride : 0;
    a.bits_w = bits;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_psdu_frame(a, stream), "psdu frame launch");
}

int wce_psdu_deframe(wce_ctx *c, const wce_psdu_par *p, const uint8_t *bits, int64_t bits_stride, int64_t n,
                     const wce_psdu_out *out, void *stream)
{
    const Refuse refuse{"wce_psdu_deframe"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (!p || !bits || !out) return refuse("null parameters, bits or outputs");
    if (!out->psdu && !out->seed && !out->fcs_ok && !out->n_good) return refuse("no output requested");
    wce::PsduArgs a{};
    if (const char *bad = check_psdu(p, n, bits_stride, false, &a)) return refuse(bad);
    if (out->psdu && out->psdu_stride < a.length) return refuse("psdu_stride < L (max with lengths)");
    if (misaligned(out->fcs_ok, 4) || misaligned(out->n_good, 4)) return refuse("fcs_ok or n_good not 4-byte aligned");
    if (n == 0) return WCE_OK;
    a.bits_r = bits;
    a.psdu = out->psdu; a.psdu_stride = out->psdu_stride;
    a.oseed = out->seed; a.fcs_ok = out->fcs_ok; a.n_good = out->n_good;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_psdu_deframe(a, stream), "psdu deframe launch");
}

// ---------------------------------------------------------------- transmitter and channel
// the symbol side of wce_modulate and the transmit calls
static const char *check_symbols(const wce_complex *tx_pre, int64_t pre_stride, const wce_complex *sym,
                                 int64_t frame_stride, int64_t block_stride, int32_t n_blocks, int64_t n_frames)
{
    if (n_blocks < 0 || n_blocks > wce::NBLK) return "n_blocks outside 0..15";
    if (!tx_pre && n_blocks == 0) return "no field and n_blocks == 0";
    if (n_blocks > 0 && !sym) return "sym required";
    if (!count_holds(n_frames)) return "n_frames < 0 or > 2^31 - 1";
    if (n_blocks > 0 && block_stride < wce::NSC) return "block_stride < 53";
    if (n_blocks > 0 && n_frames > 1 && frame_stride < (int64_t)(n_blocks - 1) * block_stride + wce::NSC)
        return "frame_stride < (n_blocks - 1) block_stride + 53";
    if (tx_pre && pre_stride != 0 && pre_stride < wce::NSC) return "pre_stride neither 0 nor >= 53";
    if (misaligned(tx_pre, 16) || misaligned(sym, 16)) return "tx_pre or sym not 16-byte aligned";
    return nullptr;
}

// the waveform wce_channel and wce_channel_tv read
static const char *check_wave(const wce_complex *wave, int64_t wave_stride, int64_t wave_len)
{
    if (!wave) return "wave required";
    if (wave_len < 1 || wave_len > 0x7fffffffll) return "wave_len < 1 or >= 2^31";
    if (wave_stride < wave_len) return "wave_stride < wave_len";
    if (misaligned(wave, 16)) return "wave not 16-byte aligned";
    return nullptr;
}

// p and the capture side of the static channel calls
static const char *check_channel(const wce_channel_par *p, const wce_complex *capture, int64_t capture_stride,
                                 int64_t capture_len, int64_t n_frames)
{
    if (!p || !capture) return "null parameters or capture";
    if (!count_holds(n_frames)) return "n_frames < 0 or > 2^31 - 1";
    if (p->n_taps < 1 || p->n_taps > 16) return "n_taps outside 1..16";
    if (p->taps && p->taps_stride != 0 && p->taps_stride < p->n_taps) return "taps_stride neither 0 nor >= n_taps";
    if (capture_len < 1 || capture_len > 0x7fffffffll) return "capture_len < 1 or >= 2^31";
    if (capture_stride < capture_len) return "capture_stride < capture_len";
    if (misaligned(p->taps, 16) || misaligned(capture, 16)) return "taps or capture not 16-byte aligned";
    if (misaligned(p->cfo, 8) || misaligned(p->ow2, 8)) return "cfo or ow2 not 8-byte aligned";
    if (misaligned(p->delay, 4)) return "delay not 4-byte aligned";
    return nullptr;
}

static void tx_symbols(wce::TxArgs &a, const wce_complex *tx_pre, int64_t pre_stride, const wce_complex *sym,
                       int64_t frame_stride, int64_t block_stride, int32_t n_blocks, int64_t n_frames)
{
    a.pre = re(tx_pre); a.pre_stride = pre_stride;
    a.sym = re(sym); a.fs = frame_stride; a.bs = block_stride;
    a.nb = n_blocks; a.field = tx_pre ? 1 : 0; a.n = n_frames;
}

static void tx_wave(wce::TxArgs &a, const wce_complex *wave, int64_t wave_stride, int64_t wave_len, int64_t n_frames)
{
    a.wave = re(wave); a.ws = wave_stride; a.wlen = wave_len; a.n = n_frames;
}

static void tx_channel(wce::TxArgs &a, const wce_channel_par *p, int field, wce_complex *capture,
                       int64_t capture_stride, int64_t capture_len)
{
    a.taps = re(p->taps); a.ts = p->taps_stride;
    a.nt = p->taps ? p->n_taps : 1;
    a.chan_field = field;
    a.cfo = p->cfo; a.ow2 = p->ow2; a.delay = p->delay; a.seed = p->seed; a.first = p->first_frame;
    a.out = re(capture); a.os = capture_stride; a.olen = capture_len;
}

int wce_modulate(wce_ctx *c, const wce_complex *tx_pre, int64_t pre_stride, const wce_complex *sym,
                 int64_t frame_stride, int64_t block_stride, int32_t n_blocks, int64_t n_frames, wce_complex *wave,
                 int64_t wave_stride, void *stream)
{
    const Refuse refuse{"wce_modulate"};
    if (!c) return fail(WCE_EINVAL, "null ctx");
    if (!wave) return refuse("wave required");
    if (const char *bad = check_symbols(tx_pre, pre_stride, sym, frame_stride, block_stride, n_blocks, n_frames))
        return refuse(bad);
    if (wave_stride < (tx_pre ? 160 : 0) + 80 * (int64_t)n_blocks) return refuse("wave_stride < the waveform's length");
    if (misaligned(wave, 16)) return refuse("wave not 16-byte aligned");
    if (n_frames == 0) return WCE_OK;
    wce::TxArgs a{};
    tx_symbols(a, tx_pre, pre_stride, sym, frame_stride, block_stride, n_blocks, n_frames);
    a.out = re(wave); a.os = wave_stride;
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_modulate(a, stream), "modulate launch");
}

int wce_channel(wce_ctx *c, const wce_complex *wave, int64_t wave_stride, int64_t wave_len, int64_t n_frames,
                const wce_channel_par *p, wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                void *stream)
{
    if (!c) return fail(WCE_EINVAL, "null ctx");
    const char *bad = check_wave(wave, wave_stride, wave_len);
    if (!bad) bad = check_channel(p, capture, capture_stride, capture_len, n_frames);
    if (bad) return Refuse{"wce_channel"}(bad);
    if (n_frames == 0) return WCE_OK;
    wce::TxArgs a{};
    tx_wave(a, wave, wave_stride, wave_len, n_frames);
    tx_channel(a, p, p->field ? 1 : 0, capture, capture_stride, capture_len);
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_channel(a, stream), "channel launch");
}

int wce_transmit(wce_ctx *c, const wce_complex *tx_pre, int64_t pre_stride, const wce_complex *sym,
                 int64_t frame_stride, int64_t block_stride, int32_t n_blocks, int64_t n_frames,
                 const wce_channel_par *p, wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                 void *stream)
{
    if (!c) return fail(WCE_EINVAL, "null ctx");
    const char *bad = check_symbols(tx_pre, pre_stride, sym, frame_stride, block_stride, n_blocks, n_frames);
    if (!bad) bad = check_channel(p, capture, capture_stride, capture_len, n_frames);
    if (bad) return Refuse{"wce_transmit"}(bad);
    if (n_frames == 0) return WCE_OK;
    wce::TxArgs a{};
    tx_symbols(a, tx_pre, pre_stride, sym, frame_stride, block_stride, n_blocks, n_frames);
    tx_channel(a, p, a.field, capture, capture_stride, capture_len);
    DeviceGuard g(wce::ctx_device(c));
    return launched(wce::launch_transmit(a, stream), "transmit launch");
}

// ---- the time-varying pair: the static calls' checks on the fields the two structures share, then the knots'
static wce_channel_par static_side(const wce_fading_par *p)
{
    return wce_channel_par{nullptr, 0, p->n_taps, p->field, p->cfo, p->ow2, p->delay, p->seed, p->first_frame};
}

// wave_len: the samples the channel runs over; the knots reach past its last output
static const char *check_fading(const wce_fading_par *p, wce_complex *capture, int64_t capture_stride,
                                int64_t capture_len, int64_t n_frames, int64_t wave_len)
{
    if (!p) return "null parameters or capture";
    const wce_channel_par s = static_side(p);
    if (const char *bad = check_channel(&s, capture, capture_stride, capture_len, n_frames)) return bad;
    if (!p->knots) return "knots required";
    if (misaligned(p->knots, 16)) return "knots not 16-byte aligned";
    if (p->n_knots < 2) return "n_knots < 2";
    if (p->knot_period < 16 || p->knot_period > (1 << 20)) return "knot_period outside 16..2^20";
    if (p->knot_stride < p->n_taps) return "knot_stride < n_taps";
    if (p->frame_stride != 0 && p->frame_stride < (int64_t)(p->n_knots - 1) * p->knot_stride + p->n_taps)
        return "frame_stride neither 0 nor >= (n_knots - 1) knot_stride + n_taps";
    if ((int64_t)(p->n_knots - 1) * p->knot_period <= wave_len + p->n_taps - 2) return "the knots do not cover the output";
    return nullptr;
}

// the channel side of `g`: the static calls' fields with every frame's own taps, and the knots
static void tx_fading(wce::TxTvArgs &g, const wce_fading_par *p, int field, wce_complex *capture,
                      int64_t capture_stride, int64_t capture_len)
{
    const wce_channel_par s = static_side(p);
    tx_channel(g.a, &s, field, capture, capture_stride, capture_len);
    g.a.nt = p->n_taps;
    g.k.knots = re(p->knots); g.k.fs = p->frame_stride; g.k.ks = p->knot_stride;
    g.k.nk = p->n_knots; g.k.period = p->knot_period;
}

int wce_channel_tv(wce_ctx *c, const wce_complex *wave, int64_t wave_stride, int64_t wave_len, int64_t n_frames,
                   const wce_fading_par *p, wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                   void *stream)
{
    if (!c) return fail(WCE_EINVAL, "null ctx");
    const char *bad = check_wave(wave, wave_stride, wave_len);
    if (!bad) bad = check_fading(p, capture, capture_stride, capture_len, n_frames, wave_len);
    if (bad) return Refuse{"wce_channel_tv"}(bad);
    if (n_frames == 0) return WCE_OK;
    wce::TxTvArgs g{};
    tx_wave(g.a, wave, wave_stride, wave_len, n_frames);
    tx_fading(g, p, p->field ? 1 : 0, capture, capture_stride, capture_len);
    DeviceGuard dg(wce::ctx_device(c));
    return launched(wce::launch_channel_tv(g, stream), "channel_tv launch");
}

int wce_transmit_tv(wce_ctx *c, const wce_complex *tx_pre, int64_t pre_stride, const wce_complex *sym,
                    int64_t frame_stride, int64_t block_stride, int32_t n_blocks, int64_t n_frames,
                    const wce_fading_par *p, wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                    void *stream)
{
    if (!c) return fail(WCE_EINVAL, "null ctx");
    const char *bad = check_symbols(tx_pre, pre_stride, sym, frame_stride, block_stride, n_blocks, n_frames);
    if (!bad)
        bad = check_fading(p, capture, capture_stride, capture_len, n_frames, (tx_pre ? 160 : 0) + 80 * (int64_t)n_blocks);
    if (bad) return Refuse{"wce_transmit_tv"}(bad);
    if (n_frames == 0) return WCE_OK;
    wce::TxTvArgs g{};
    tx_symbols(g.a, tx_pre, pre_stride, sym, frame_stride, block_stride, n_blocks, n_frames);
    tx_fading(g, p, g.a.field, capture, capture_stride, capture_len);
    DeviceGuard dg(wce::ctx_device(c));
    return launched(wce::launch_transmit_tv(g, stream), "transmit_tv launch");
}

// ---------------------------------------------------------------- debug hooks of the chain
long long wce_debug_chain_grid(long long blocks, long long own_cap) { return wce::chain_grid(blocks, own_cap); }

int wce_debug_short_field_period(double *out)
{
    if (!out) return fail(WCE_EINVAL, "null buffer");
    wce::short_field_period(out);
    return WCE_OK;
}

int wce_debug_sync_stf_tiles(int *lags_stf, int *lags_ltf)
{
    if (!lags_stf || !lags_ltf) return fail(WCE_EINVAL, "null buffer");
    wce::sync_stf_tiles(lags_stf, lags_ltf);
    return WCE_OK;
}

}  // extern "C"
