/*
 * wce.h -- C ABI of the MI355X 802.11 channel-estimation engine (libwce.so).
 *
 * Drop-in boundary for the estimator path of usmandroid/80211ParallelEstimation
 * (main.c / utils.c).  Plain pointers and sizes only: no HIP or torch types in
 * the signatures (streams are passed as `void *` hipStream_t, NULL = default
 * stream).  Every call returns an int status (0 ok, < 0 error); the reference
 * functions return void and print on dimension mismatch (utils.c:18-19).
 *
 * Two layers:
 *   1. the batched API below (wce_ctx_*, wce_estimate, wce_mmse_*) that runs
 *      B frames resident in HBM through hand-written gfx950 kernels;
 *   2. include/wce_compat.h: the five reference signatures of main.c:4-8,
 *      one frame in host memory, implemented on top of layer 1.
 *
 * Data layout: complex fp64 is {re, im} (16 B, binary-compatible with C99
 * double _Complex and hipDoubleComplex).  Frame f, OFDM block b, subcarrier k
 * lives at base[f*frame_stride + b*block_stride + k] (strides in elements);
 * the reference's block-major inputs.h layout (tx_symb[53*15]) is
 * frame_stride = 795, block_stride = 53.
 */
#ifndef WCE_H
#define WCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WCE_NSC 53   /* SAMPUTIL, utils.h:13 */
#define WCE_NBLK 15  /* OFDMBLK,  utils.h:15 */
#define WCE_DC 26    /* main.c:74 H_EST[26] = 0 */
#define WCE_P0 5     /* utils.h:16-19 pilot subcarriers */
#define WCE_P1 19
#define WCE_P2 33
#define WCE_P3 47

typedef struct { double re, im; } wce_complex;

enum {
    WCE_OK = 0,
    WCE_EINVAL = -1,   /* bad argument / shape */
    WCE_EHIP = -2,     /* HIP runtime error */
    WCE_ENOMEM = -3,
    WCE_ESTATE = -4,   /* context has no valid shared state */
    WCE_ENODEV = -5    /* no usable gfx950 device */
};

/* estimator mask bits (one per reference entry point, main.c:4-8) */
#define WCE_EST_LT_LS     (1u << 0)  /* WiFi_channel_estimation_LT_LS     main.c:66  */
#define WCE_EST_PS_LINEAR (1u << 1)  /* WiFi_channel_estimation_PS_Linear main.c:77  */
#define WCE_EST_PS_CUBIC  (1u << 2)  /* WiFi_channel_estimation_PS_Cubic  main.c:103 */
#define WCE_EST_PS_SINC   (1u << 3)  /* WiFi_channel_estimation_PS_Sinc   main.c:124 */
#define WCE_EST_PS_MMSE   (1u << 4)  /* WiFi_channel_estimation_PS_MMSE   main.c:148 */
#define WCE_EQUALIZE      (1u << 5)  /* WiFi_Equalization.m (no C original) */
#define WCE_EST_LS_ALL    (0xFu)
/* PS_MMSE with each frame's own covariance: Rhh_f from the frame's preamble
 * (wce_frames.rx_pre required) instead of the context's shared preamble, i.e.
 * main.c's PS_MMSE called with H_EST_LS = that frame's LT_LS (main.c:41-53 per
 * frame).  C_f = F Rhh_f F^H is rank 1, so it is never formed: two batched
 * MFMA matrix-vector products give its factors and the solve writes H.  On a
 * WCE_MMSE_COV context the modifier replaces the model covariance: the request
 * gives what a TEXTBOOK context on the same preamble gives, bit for bit. */
#define WCE_MMSE_FRAME_COV (1u << 6)

/* MMSE semantics (DESIGN.md "MMSE contract"):
 *  REF      : main.c:148-212 with the NaN inverse(Ryy) repaired:
 *             H = C_ref X4 (2 ow2 I)^-1 rx, C_ref = F Rhh FH, X4 = pilots of tx.
 *  TEXTBOOK : WiFi_channel_estimation_PS_MMSE.m per block:
 *             H = C X (X C X' + ow2 I)^-1 rx, C = F Rhh F', X = diag(tx).
 * Both run the same kernel: H = C X (a X C X' + b I)^-1 rx. */
enum { WCE_MMSE_REF = 0, WCE_MMSE_TEXTBOOK = 1, WCE_MMSE_COV = 2 };
/*  COV      : TEXTBOOK with a caller-supplied channel covariance Rhh instead
 *             of the single-preamble estimate ifft(H_LT) ifft(H_LT)' (e.g. a
 *             power-delay-profile model or an average over many preambles):
 *             C = F Rhh F', generally full rank -- the dense per-frame solve
 *             is then the only way to apply it.  See wce_state_build_cov. */

typedef struct wce_ctx wce_ctx;

/* Build the shared state on the host (F as main.c:18-26 builds it, the
 * reference's cofactor invF of utils.c:141-170 in 80-bit long double, H_LT
 * from the shared preamble (main.c:66-75), the MMSE covariance C of
 * main.c:186-203, the sinc table of utils.c:727-733) and upload it to `device`.  tx_pre/rx_pre: the shared
 * preamble FFTs (53 each, host).  The first call in a process spends
 * ~0.5 s (8 threads) on invF; later calls reuse it. */
int wce_ctx_create(wce_ctx **ctx, int device, const wce_complex *tx_pre,
                   const wce_complex *rx_pre, double ow2, int mmse_mode);

/* A context whose device state is filled later (e.g. by an RCCL broadcast
 * into the buffer returned by wce_ctx_state). */
int wce_ctx_create_empty(wce_ctx **ctx, int device);
int wce_ctx_destroy(wce_ctx *ctx);

/* WCE_MMSE_COV: Rhh is the 53 x 53 time-domain channel covariance (row-major,
 * Hermitian positive semidefinite, host); tx_pre/rx_pre still give H_LT for
 * LT_LS and equalization.  Rhh is checked: WCE_EINVAL unless every entry is
 * finite, Rhh = Rhh^H to 1e-12 of its largest entry, and its eigenvalues are
 * >= -1e-12 of the largest.  The 80-bit eigendecomposition Rhh = V Lambda V^H
 * (eigenvalues at or below 2^-46 of the largest -- the rounding level of an
 * fp64 input -- count as zero) gives C = F Rhh F^H = U U^H, U = F V sqrt(Lambda),
 * r columns.  The per-frame solve then runs in one of two forms:
 *   low rank (r < 53, or a spectrum wider than 1e5): the r x r Gram system
 *     (a G^H G + b I) t = G^H rx, G = X U, and H = U s -- accurate to ~1e-13
 *     at any rank (the dense form loses ~eps cond(Ryy) there);
 *   dense (r = 53 and a spectrum within 1e5): Cholesky of Ryy, then H = C W on MFMA. */
int wce_ctx_create_cov(wce_ctx **ctx, int device, const wce_complex *tx_pre, const wce_complex *rx_pre,
                       const wce_complex *Rhh, double ow2);
/* WCE_MMSE_COV context: the rank r, whether the low-rank path runs (1) or the
 * dense one (0), and the largest / smallest kept eigenvalue of C (outputs may be NULL). */
int wce_ctx_cov_info(wce_ctx *ctx, int *rank, int *low_rank, double *lambda_max, double *lambda_min);
/* WCE_MMSE_COV, constant-modulus frames (round 4; WiFi_channel_estimation_PS_MMSE.m:29-32).
 * Ryy depends on a frame's symbols only through P = diag |x_k|^2 (and their
 * phases), and for PSK frames -- the reference's BPSK data (inputs.h), QPSK --
 * P is the same for every frame.  x_ref: one frame's 53 symbols; p_k = |x_ref,k|^2
 * (0 off the X mask) is the pattern.  The ctx forms once, in 80-bit on the
 * host, K = (a C P + b I)^-1 C (the push-through of C X^H Ryy^-1) and uploads
 * it.  Estimates in C semantics then check every frame on the device: a frame
 * whose |x_k|^2 equals p_k bit for bit on all subcarriers takes
 *     H = K (conj(x) o rx)   [+ C ((x - conj x) o (rx - a x o H1)) / b for non-real x]
 * -- two batched f64-MFMA products, no per-frame factorisation -- and every
 * other frame the per-frame solve, as without the pattern.  Ranks <= 8 keep
 * the one-frame-per-lane kernels (already bound by the frames' HBM traffic).
 * x_ref NULL: off.  Needs the ctx that built the state (wce_ctx_create_cov);
 * it updates the shared state, so a multi-GPU run sets it before the
 * broadcast.  Not safe against estimates in flight on this ctx. */
int wce_ctx_set_modulus(wce_ctx *ctx, const wce_complex *x_ref);

/* Device pointer and size of the packed shared state (C, H_LT, tx_pre, sinc
 * table, MMSE coefficients): the single buffer a multi-GPU run broadcasts
 * from rank 0.  After writing it externally call wce_ctx_mark_ready. */
int wce_ctx_state(wce_ctx *ctx, void **device_ptr, size_t *bytes);
int wce_ctx_mark_ready(wce_ctx *ctx);

/* Host-only shared state: build it once (no device needed), ship the bytes
 * to other processes / devices (RCCL broadcast, file, ...), and load them
 * into a context.  wce_state_size() is the byte size of that blob. */
size_t wce_state_size(void);
int wce_state_build(void *host_state, size_t bytes, const wce_complex *tx_pre, const wce_complex *rx_pre,
                    double ow2, int mmse_mode);
int wce_state_build_cov(void *host_state, size_t bytes, const wce_complex *tx_pre, const wce_complex *rx_pre,
                        const wce_complex *Rhh, double ow2);
int wce_ctx_load_state(wce_ctx *ctx, const void *host_state, size_t bytes);
/* wce_ctx_set_modulus on a host blob built by wce_state_build_cov from the same Rhh. */
int wce_state_set_modulus(void *host_state, size_t bytes, const wce_complex *Rhh, const wce_complex *x_ref);
/* Host-only check of a state blob (e.g. bytes received from another rank):
 * WCE_OK and its MMSE mode (may be NULL) if it holds a valid state, else
 * WCE_EINVAL (too short) / WCE_ESTATE (no valid magic). */
int wce_state_validate(const void *host_state, size_t bytes, int *mmse_mode);

/* Copy back the shared vectors (host outputs, may be NULL): H_LT (53),
 * C (53*53 row-major), and the MMSE coefficients a, b. */
int wce_ctx_get_shared(wce_ctx *ctx, wce_complex *h_lt, wce_complex *C, double *a, double *b);

typedef struct {
    const wce_complex *tx;      /* device; tx[f*frame_stride + b*block_stride + k] */
    const wce_complex *rx;      /* device; same layout as tx */
    const wce_complex *rx_pre;  /* device; per-frame preamble FFT rx_pre[f*pre_stride + k],
                                   NULL = use the context's shared H_LT */
    const wce_complex *tx_pre;  /* device; shared preamble (53), NULL = context's */
    int64_t frame_stride;
    int64_t block_stride;
    int64_t pre_stride;
    int64_t n_frames;
    int32_t block;              /* OFDM block read by PS_* / MMSE (main.c:16 uses 0) */
    int32_t semantics;          /* WCE_SEM_C (main.c) or WCE_SEM_MATLAB (WiFi_*.m) */
} wce_frames;

/* Frames: what a frame's outputs may depend on.  In every call that takes a batch
 * (wce_frames, n_frames, n_packets) the outputs of frame f depend on frame f's
 * own inputs and on the arguments every frame shares (the context, strides, masks,
 * scalars, shared arrays such as tx_pre or ltf), and on nothing else: not on f,
 * not on the batch size, not on what any other frame holds, non-finite values
 * included.  So a batch permuted gives the same rows permuted, a slice of a batch
 * run alone gives the slice of the rows, and both hold bit for bit.
 *  - Indexed calls add one thing: wce_synth_frames, wce_channel, wce_transmit and
 *    their _tv forms key their random numbers on the global index first_frame + f.
 *    A slice [s, s + n) run with first_frame raised by s gives the slice of the
 *    rows; with the noise off (ow2 = 0 or NULL) they are as every other call.
 *  - Totals are sums: a batch-wide count (wce_psdu_deframe's *n_good increment,
 *    wce_nonfinite_scan's *n_bad) is the sum of its per-frame flags.
 *  - wce_combine and wce_sync_share are branch-major: the law holds per packet,
 *    across all of its branches.
 * tests/frame_model.py is the table of the calls, and tests/test_frame_law_gpu.py
 * holds each to it. */

/* Estimator semantics (wce_frames.semantics):
 *  WCE_SEM_C      : main.c -- one OFDM block (`block`), LT_LS "conj" quirk
 *                   (main.c:69), every cubic divided difference by 14 (main.c:116-118).
 *  WCE_SEM_MATLAB : WiFi_channel_estimation_*.m -- proper conj in LT_LS, PS_* and
 *                   PS_MMSE averaged over OFDM blocks 1..4 (0..3 here; `block`
 *                   ignored), cubic divisors 14/28/42 (PS_Cubic.m:11-13). */
enum { WCE_SEM_C = 0, WCE_SEM_MATLAB = 1 };

/* An output is written if and only if its bit is in `mask`: lt_ls, ps_linear,
 * ps_cubic, ps_sinc and ps_mmse by their WCE_EST_* bits, eq by WCE_EQUALIZE.  A
 * buffer whose bit is not in `mask` is never written, whatever its pointer --
 * one wce_outputs with every pointer set serves any mask -- and that holds for
 * the eq_source estimate too, which WCE_EQUALIZE computes for its blend. */
typedef struct {
    wce_complex *lt_ls;         /* device [n_frames][out_stride]; may be NULL where its bit is not in mask */
    wce_complex *ps_linear;
    wce_complex *ps_cubic;
    wce_complex *ps_sinc;
    wce_complex *ps_mmse;
    wce_complex *eq;            /* equalized symbols, eq[f*eq_frame_stride + b*eq_block_stride + k] */
    int64_t out_stride;         /* >= 53 */
    int64_t eq_frame_stride;
    int64_t eq_block_stride;
    uint32_t eq_source;         /* PS estimate blended with H_LT (WiFi_RX.m:60 uses PS_Linear): one of
                                   WCE_EST_PS_LINEAR, WCE_EST_PS_CUBIC, WCE_EST_PS_SINC; 0 = WCE_EST_PS_LINEAR.
                                   With WCE_EQUALIZE in mask any other value is WCE_EINVAL; without it the
                                   field is not looked at.  The source need not be in mask */
    uint32_t flags;             /* WCE_OUT_* */
} wce_outputs;

/* wce_outputs.flags.  WCE_OUT_LS_F32: the LS family (lt_ls, ps_linear,
 * ps_cubic, ps_sinc) and eq are stored as complex float ({re, im} float, 8 B)
 * (BASELINE configs[4] "mixed fp64 solve / fp32 interp").  ps_mmse stays complex
 * double.  Strides count elements of each buffer's own type.
 *  - The LS family is computed in fp64 and rounded once (<= 1e-7 relative).
 *  - eq divides in fp32: H_UTIL = wlt H_LT + wps H_PS is blended in fp64 (where
 *    the two cancel, fp32 operands would lose the quotient), scaled by a power
 *    of two and rounded to fp32; rx is rounded to fp32; the quotient is formed
 *    in fp32 with v_rcp_f32.  Every element lies within 5.6e-7 of the exact
 *    quotient, relative and by complex modulus, also where the blend cancels
 *    down to 1e-6 of its terms (twice the worst element of the host model
 *    tests/eq_model.py, 2.8e-7; tests/test_equalize_gpu.py checks each element).
 *  - rx is rounded to fp32 before it is scaled, so under this flag each part of
 *    rx must be 0 or lie in fp32's normal range (2^-126 <= |x| < 2^128) for that
 *    bound to hold (checked with the channel, and rx with it, scaled by 2^100
 *    and by 2^-100); inputs outside that range are not treated specially. */
#define WCE_OUT_LS_F32 (1u << 0)

/* Threading: one ctx may serve calls on several streams at once, from one
 * host thread or several.  The shared state is read-only after creation, and
 * the scratch that WCE_MMSE_FRAME_COV and MATLAB-semantics PS_MMSE need
 * (5 KB per frame) is kept per stream, so calls on different streams never
 * share it; calls on the same stream are serialised (as the stream would).
 * Plans own their scratch.  wce_last_error() is per thread.
 *
 * Every call that takes a `stream` -- the receive and transmit chain, the
 * front end, wce_estimate and its kin, the conversions and the _async and
 * device copies -- is ordered on that stream behind the work queued there
 * before it and returns without waiting for it: it reads no device memory on
 * the host and allocates nothing (wce_estimate: once the stream's scratch is
 * sized, below).  A refused call (WCE_EINVAL) launches nothing.  Each call may
 * run beside itself and beside every other on other streams, from one host
 * thread or several, and gives the bytes of the same calls run one after
 * another (tests/test_chain_streams_gpu.py); nothing orders two streams
 * against each other but the host (wce_stream_synchronize, wce_event_query).
 *
 * Pre-size that scratch for batches of up to n_frames so that wce_estimate
 * never allocates: _stream for one stream; wce_ctx_reserve for the NULL
 * stream, and as the minimum size of every stream's scratch created later,
 * by a call or by wce_ctx_reserve_stream.  Scratch that exists is only ever
 * grown to the batch in hand or to the size asked for here, never to
 * wce_ctx_reserve's: a reserved stream does not wait.
 * Without it the first larger batch on a stream allocates (synchronously on
 * that stream) and keeps the buffer until wce_ctx_destroy. */
int wce_ctx_reserve(wce_ctx *ctx, int64_t n_frames);
int wce_ctx_reserve_stream(wce_ctx *ctx, int64_t n_frames, void *stream);

/* Run the estimators selected in `mask` over all frames, asynchronously on
 * `stream`.  Replaces the per-frame calls of main.c:37-54 (and the frame
 * loops of main_openmp.c / main_mpi.c) with one batched call.  LS family + equalization: one HBM-streaming kernel; MMSE: the
 * LDS/register-resident Cholesky solve kernel followed by the MFMA GEMM
 * (the ps_mmse buffer doubles as the solve->GEMM workspace). */
int wce_estimate(wce_ctx *ctx, const wce_frames *in, const wce_outputs *out,
                 uint32_t mask, void *stream);

/* wce_estimate with each frame's own noise variance: ow2[f] (device, n_frames
 * doubles, contiguous -- the array wce_front_end_preamble writes) replaces the
 * context's ow2 in frame f's PS_MMSE, as WiFi_RX.m estimates sigma^2 per packet
 * (WiFi_RX.m:30) and hands it to WiFi_channel_estimation_PS_MMSE (WiFi_RX.m:57).
 * ow2 == NULL: exactly wce_estimate.  With ow2 != NULL:
 *  - Supported: a WCE_MMSE_TEXTBOOK context (the .m model, the only one where
 *    ow2 is per packet) and WCE_EST_PS_MMSE in `mask`; with or without
 *    WCE_MMSE_FRAME_COV; WCE_SEM_C and WCE_SEM_MATLAB; any LS-family and
 *    WCE_EQUALIZE bits alongside (they do not depend on ow2 and run as the LS
 *    pass, then the closed-form rank-1 solve).  The request always runs that
 *    closed form, whatever the wce_debug_* A/B knobs say.
 *  - WCE_EINVAL with a wce_last_error() text, before any launch: a WCE_MMSE_REF
 *    or WCE_MMSE_COV context; a mask without WCE_EST_PS_MMSE; an ow2 pointer
 *    that is not 8-byte aligned.
 *  - The host never reads ow2[] (no synchronisation).  A frame whose ow2[f] is
 *    not a positive finite number gets every entry of its ps_mmse row set to
 *    NaN, both parts, so wce_nonfinite_scan flags it; no other frame and no
 *    other output of that frame is affected.
 *  - With every ow2[f] equal to the context's ow2, every output is
 *    bit-identical to wce_estimate on the same request; a frame's bits depend
 *    on its own data and its own ow2[f] only.
 * Launch plans (wce_plan_create) keep the context's ow2. */
int wce_estimate_noise(wce_ctx *ctx, const wce_frames *in, const wce_outputs *out,
                       uint32_t mask, const double *ow2, void *stream);

/* Launch plans: one wce_estimate call (fixed buffers, strides, mask, batch)
 * captured into a HIP graph once and replayed with a single graph launch --
 * for serving loops that re-run small batches into the same buffers, where
 * per-call host checks and kernel launch latency dominate.  Arguments are
 * validated and the plan's own workspace sized at creation; the plan keeps
 * raw pointers, so the buffers and the ctx (its device state) must outlive
 * it.  Capture runs on a private stream; launches go to the stream given, and
 * replays may run beside direct calls on other streams.  A replay is one
 * graph launch; on ROCm 7 that measured slightly SLOWER than the direct
 * call's launches (bench small_batch), so a plan buys validation once and a
 * fixed argument set, not speed. */
typedef struct wce_plan wce_plan;
int wce_plan_create(wce_plan **plan, wce_ctx *ctx, const wce_frames *in, const wce_outputs *out,
                    uint32_t mask);
int wce_plan_launch(wce_plan *plan, void *stream);
int wce_plan_destroy(wce_plan *plan);

/* The two MMSE stages, exposed for profiling:
 *   solve: W[f] = X_f (a X_f C X_f' + b I)^-1 rx_f        (FP64 VALU, per frame)
 *   apply: H[f] = C W[f]                                  (FP64 MFMA batched GEMM)
 * W and H may alias (in place). */
int wce_mmse_solve(wce_ctx *ctx, const wce_frames *in, wce_complex *W, int64_t w_stride, void *stream);
int wce_mmse_apply(wce_ctx *ctx, const wce_complex *W, wce_complex *H, int64_t stride,
                   int64_t n_frames, void *stream);

/* Synthetic 802.11 frames generated on the device from a counter-based RNG
 * keyed by (seed, global frame index), so any shard regenerates identical
 * frames: BPSK data +-A, pilots A*(1,1,1,-1)*p_b (802.11 polarity), DC = 0,
 * a 6-tap exponential-PDP channel (or h_shared for every frame, if non-NULL),
 * CN(0, ow2) noise.  rx_pre (may be NULL) = per-frame preamble H*tx_pre + noise/sqrt2.
 * The noise is an Irwin-Hall sum of four uniforms (unit variance, no sample beyond 3.46 sigma): fine for
 * timing and parity runs, not for error rates, which should draw theirs from wce_channel. */
int wce_synth_frames(wce_ctx *ctx, wce_complex *tx, wce_complex *rx, wce_complex *rx_pre,
                     int64_t frame_stride, int64_t block_stride, int64_t pre_stride,
                     int64_t first_frame, int64_t n_frames, uint64_t seed,
                     const wce_complex *h_shared, double amplitude, double ow2, void *stream);

/* ---- time-domain front end (MATLAB only, no C original) ----
 * WiFi_blocks_extraction.m:1-11: OFDM block b of frame f is the 80 samples
 * samples[f*packet_stride + 80 b + (0..79)]; the 16-sample cyclic prefix is
 * dropped and the last 64 go through a 64-point DFT, circshift(., 26), and
 * the first 53 bins are kept:
 *     sym[f*frame_stride + b*block_stride + i] = DFT64[(i - 26) mod 64],  i < 53.
 * Used for tx and rx packets alike (WiFi_RX.m:42-43).  The output is the
 * wce_frames layout, so wce_estimate can consume it directly.  The ctx only
 * selects the device (its state need not be loaded). */
enum { WCE_FFT_SIZE = 64, WCE_SAMPLES_PER_BLOCK = 80 };
int wce_front_end_blocks(wce_ctx *ctx, const wce_complex *samples, int64_t packet_stride, int64_t n_frames,
                         int32_t n_blocks, wce_complex *sym, int64_t frame_stride, int64_t block_stride,
                         void *stream);

/* WiFi_RX.m:18-30: the long training field of frame f is
 * lptot[f*lptot_stride + (0..lptot_len-1)]; its last 64 samples are p1 and
 * the 64 before them p2.  pre_fft[f*pre_stride + i] = circshift(DFT64((p1+p2)/2), 26)[i],
 * i < 53 (feed it to wce_frames.rx_pre / tx_pre), and, if ow2 != NULL,
 * ow2[f] = sum |p2 - p1|^2 / (2*64), the noise estimate of WiFi_RX.m:30. */
int wce_front_end_preamble(wce_ctx *ctx, const wce_complex *lptot, int64_t lptot_stride, int64_t lptot_len,
                           int64_t n_frames, wce_complex *pre_fft, int64_t pre_stride, double *ow2,
                           void *stream);

/* ---- carrier frequency offset (WiFi_RX.m:4-9 declares one, FO / Fs; no
 * reference code removes it) ----
 * cfo[f] (device, n_frames doubles, contiguous, 8-byte aligned) is frame f's
 * offset in cycles per sample, FO / Fs.  One time axis serves the long training
 * field and the packet, counted from the end of the field: lptot[i] is sample
 * n = i - lptot_len, packet sample m is n = m + sample_offset (0: the packet
 * follows the field directly).  Every sample is derotated in registers,
 *     y[n] = x[n] exp(-2 pi i cfo[f] n),
 * before anything else is computed from it; the rest is the plain call.
 *
 * wce_front_end_preamble_cfo, estimate != 0: cfo[f] is written, the two-copy
 * estimate arg(sum_n p1[n] conj(p2[n])) / (2 pi 64) over the 64 sample pairs
 * of WiFi_RX.m:25-26 (|cfo| < 1/128, +-78 kHz at 10 MHz; an all-zero field
 * gives 0), and used in the same launch; estimate == 0: cfo[f] is read.  The
 * mean of the two copies, its DFT and ow2 = sum |p2' - p1'|^2 / 128 are taken
 * from the derotated copies.  wce_front_end_blocks_cfo reads cfo[f]; cfo ==
 * NULL: exactly wce_front_end_blocks (sample_offset is ignored).
 *
 *  - The host never reads cfo[]; neither call synchronises: the preamble call's
 *    estimate feeds the blocks call on the same stream with no host hop.
 *  - WCE_EINVAL (text in wce_last_error()) before any launch: cfo not 8-byte
 *    aligned; cfo == NULL in the preamble call; |sample_offset| >= 2^31; and
 *    whatever the plain calls reject.
 *  - A frame whose given cfo[f] is not finite gets NaN in every bin the call
 *    writes for it (and in its ow2[f]); a frame whose long training field
 *    holds a non-finite sample gets NaN in the same bins, in its ow2[f] and,
 *    when estimated, its cfo[f].  No other frame changes by a bit
 *    (wce_nonfinite_scan finds such frames).
 *  - A frame's output bits depend only on its own samples, its cfo[f] and
 *    sample_offset, not on its place in the batch or the batch's size.
 *  - A given cfo[f] == 0.0 on finite samples: bit-identical to the plain calls. */
int wce_front_end_blocks_cfo(wce_ctx *ctx, const wce_complex *samples, int64_t packet_stride, int64_t n_frames,
                             int32_t n_blocks, const double *cfo, int64_t sample_offset, wce_complex *sym,
                             int64_t frame_stride, int64_t block_stride, void *stream);
int wce_front_end_preamble_cfo(wce_ctx *ctx, const wce_complex *lptot, int64_t lptot_stride, int64_t lptot_len,
                               int64_t n_frames, wce_complex *pre_fft, int64_t pre_stride, double *ow2,
                               double *cfo, int estimate, void *stream);

/* ---- packet detection and symbol timing (WiFi_RX.m:7 declares `threshold`,
 * "Threshold for signal detection"; no reference code uses it) ----
 * The calls above expect every packet cut out of the sample stream.  These
 * take raw capture windows instead: frame f's window is
 *     x[i] = capture[f*capture_stride + i],  i < capture_len,
 * and the packet starts somewhere inside it.
 *
 * wce_front_end_sync finds where.  ltf (device, 64 samples, 16-byte aligned,
 * shared by all frames) is one clean period of the long training symbol, the
 * last 64 samples of the transmitted field.  With
 *     c[d] = sum_{n<64}  x[d+n] conj(ltf[n]),       0 <= d <= capture_len - 64
 *     E[d] = sum_{n<128} |x[d+n]|^2,  El = sum |ltf[n]|^2
 *     M[d] = 2 |c[d]| |c[d+64]| / (El E[d]),        0 <= d <= capture_len - 128
 * (M[d] = 0 where El E[d] == 0; M is in [0, 1] by Cauchy-Schwarz), d* is the
 * smallest d that attains max M, metric[f] = M[d*] (metric may be NULL), and
 *     start[f] = d* - backoff   if M[d*] >= threshold and d* - backoff >= 0,
 *     start[f] = -1             otherwise.
 * start[f] indexes the first sample of the earlier of the two 64-sample copies
 * (rx_preamble2 of WiFi_RX.m:26).  The product of the two moduli needs both
 * copies present at once (half a field scores 0) and ignores the phase turn
 * between them, but a carrier offset of e cycles per sample costs the metric
 * sinc^2(64 e): 0.95 at 20 kHz, 0.44 at 77 kHz (10 MHz sampling) -- choose the
 * threshold with that in mind.  backoff (0..31) moves every FFT window that
 * many samples into the cyclic prefix, against a strongest path that is not
 * the first; field and blocks shift alike, so the estimators see one common
 * phase ramp.  E[d] is summed from non-negative block partials, never as a
 * running difference: its error is relative to E[d] itself, whatever came
 * earlier in the window.
 *
 * wce_front_end_preamble_at and wce_front_end_blocks_at are the calls above
 * reading frame f at start[f] (device, n_frames int32): the field is
 * x[start[f] .. start[f]+128), the earlier copy then the later one; packet
 * sample m is x[start[f] + 128 + sample_offset + m]; the time axis of the
 * carrier offset is the same, counted from the end of the field.  cfo == NULL:
 * no derotation (estimate != 0 then is WCE_EINVAL).  No aligned copy, no extra
 * pass over the samples: the start is one 4-byte load per unit.
 *
 *  - No call reads anything back or waits: sync feeds the _at calls on the
 *    same stream with no host hop.  The ctx only selects the device.
 *  - WCE_EINVAL (text in wce_last_error()) before any launch: capture_len <
 *    128 or >= 2^31; capture_stride < capture_len; threshold not in [0, 1];
 *    backoff outside [0, 31]; start NULL or not 4-byte aligned; metric not
 *    8-byte aligned; ltf or capture NULL or not 16-byte aligned; n_frames < 0;
 *    and, for the _at calls, whatever the calls above reject.
 *  - sync: a window holding a non-finite sample, or a non-finite ltf, gives
 *    start[f] = -1 and metric[f] = NaN, for that frame only.
 *  - _at: a frame with start[f] < 0, or one whose samples would not all lie in
 *    [0, capture_len), reads nothing outside its window and gets NaN in every
 *    bin the call writes for it, in its ow2[f] and in its estimated cfo[f]; no
 *    other frame changes by a bit.  So an undetected packet reaches
 *    wce_estimate_noise as a NaN row, which wce_nonfinite_scan finds.
 *  - _at, every other frame: bit-identical to the calls above run on the same
 *    samples copied into aligned arrays (cfo == NULL: the plain calls on finite
 *    samples; cfo != NULL: the _cfo calls).
 *  - A frame's results depend only on its own window and the call's arguments,
 *    not on its place in the batch or the batch's size; no call reads outside
 *    [0, capture_len) of any window. */
int wce_front_end_sync(wce_ctx *ctx, const wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                       int64_t n_frames, const wce_complex *ltf, double threshold, int32_t backoff,
                       int32_t *start, double *metric, void *stream);
int wce_front_end_preamble_at(wce_ctx *ctx, const wce_complex *capture, int64_t capture_stride,
                              int64_t capture_len, int64_t n_frames, const int32_t *start, wce_complex *pre_fft,
                              int64_t pre_stride, double *ow2, double *cfo, int estimate, void *stream);
int wce_front_end_blocks_at(wce_ctx *ctx, const wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                            int64_t n_frames, int32_t n_blocks, const int32_t *start, const double *cfo,
                            int64_t sample_offset, wce_complex *sym, int64_t frame_stride, int64_t block_stride,
                            void *stream);

/* ---- short training field: detection at any carrier offset, coarse offset ----
 * wce_front_end_sync's metric loses sinc^2(64 e) to an offset of e cycles per
 * sample and the two-copy estimate is unambiguous only for |e| < 1/128 (78 kHz
 * at 10 MHz), a third of what 802.11p's +-20 ppm at each end of a 5.9 GHz link
 * allow.  The short training field (STF), ten repetitions of a 16-sample period
 * in front of the long field, carries a receiver over the rest: a lag-16
 * autocorrelation detects it whatever the offset (which only turns the
 * correlation's phase), that phase gives the offset within +-1/32 cycles per
 * sample, and the long field gives timing and the fine offset once the coarse
 * one is removed.
 *
 * wce_short_field is the transmitter's: wave[f*wave_stride + m] = amplitude *
 * t[m mod 16] for m < 160, nothing else written.  t is the 64-point MATLAB ifft
 * (1/64) of 802.11a's short sequence S = sqrt(13/6) (1 + j) s_k on the bins
 * k = -24, -20 .. 24 without DC, signs {+ - + - - + - - + + + +}, placed by the
 * library's bin map Y[(i - 26) mod 64] = S[i].  At amplitude 1 its mean sample
 * power is 52/4096, the long field's for unit bins.  The 16 values of t are
 * computed once on the host in 80-bit arithmetic and rounded to double; the
 * kernel replicates them, so samples m and m + 16 of a row are the same bits.
 * A packet with an STF is assembled from three calls: wce_short_field writes
 * wave[0..160), wce_modulate writes from wave + 160, and wce_channel /
 * wce_channel_tv runs with wave_len = 1520 and field = 1.  The channel's time
 * origin then sits 160 samples early: one common phase exp(2 pi i cfo 160) on
 * field and data alike, which the estimators absorb.  wce_transmit sends no STF.
 * WCE_EINVAL: NULL ctx or wave; wave not 16-byte aligned; wave_stride < 160; a
 * non-finite amplitude; n_frames < 0.  n_frames == 0 is WCE_OK.
 *
 * wce_front_end_sync_stf, per window x[0..L), L = capture_len, every frame on its
 * own:
 *  1. Detection.  For 0 <= d <= L - 144
 *         P[d] = sum_{n<128} x[d+n+16] conj(x[d+n])
 *         A[d] = sum_{n<128} |x[d+n]|^2,  B[d] = sum_{n<128} |x[d+n+16]|^2
 *     d_s is the smallest d attaining max |P[d]|^2 and Ms = |P[d_s]|^2 /
 *     (A[d_s] B[d_s]), 0 where the denominator is 0; Ms is in [0, 1] by
 *     Cauchy-Schwarz.  The maximum is taken un-normalised on purpose: in a
 *     noise-free capture the normalised ratio is 1 as soon as the window touches
 *     the STF.
 *  2. Coarse offset.  e_c = arg P[d_s] / (2 pi 16).
 *  3. Timing.  wce_front_end_sync's metric with the template turned by e_c,
 *         c[d] = sum_{n<64} x[d+n] conj(ltf[n] exp(2 pi i e_c n)),
 *     E[d], El, M[d] = 2 |c[d]| |c[d+64]| / (El E[d]) over 0 <= d <= L - 128 as
 *     there; d* is the smallest d attaining max M and Ml = M[d*].  (The device
 *     derotates the samples as it stages them, with an exactly reduced phase: the
 *     same moduli up to rounding.)
 *  4. Start.  s = d* - backoff.  The frame is detected iff Ms >= threshold_stf,
 *     Ml >= threshold_ltf and s >= 0; then start[f] = s, with
 *     wce_front_end_sync's meaning, and feeds the _at calls unchanged.
 *     Otherwise start[f] = -1 and cfo[f] = NaN.
 *  5. Fine offset, unwrapped.  For a detected frame
 *         e_f = arg(sum_{n<64} x[s+64+n] conj(x[s+n])) / (2 pi 64),
 *     the _at call's two-copy estimate on the same samples, and
 *         cfo[f] = e_f + rint((e_c - e_f) 64) / 64,
 *     to be given to wce_front_end_preamble_at (estimate = 0) and
 *     wce_front_end_blocks_at.  The total range is |e| < 1/32.
 *  - metric_stf[f] = Ms and metric_ltf[f] = Ml (either pointer may be NULL),
 *    written whether or not the frame is detected.
 *  - A window holding a non-finite sample, or a non-finite ltf, gives start -1
 *    and NaN in cfo and both metrics: a sample marks its own frame only, the ltf
 *    is shared and marks every frame.
 *  - A frame's bits depend only on its own window and the arguments; nothing is
 *    read outside [0, L); nothing is read back or allocated, and the call is
 *    asynchronous on stream.
 *  - WCE_EINVAL before any launch: capture_len < 144 or >= 2^31; capture_stride <
 *    capture_len; either threshold outside [0, 1] or not finite; backoff outside
 *    [0, 31]; start or cfo NULL or not 4-byte / 8-byte aligned; a metric pointer
 *    not 8-byte aligned; ltf or capture NULL or not 16-byte aligned; n_frames < 0.
 *    n_frames == 0 is WCE_OK. */
int wce_short_field(wce_ctx *ctx, double amplitude, wce_complex *wave, int64_t wave_stride, int64_t n_frames,
                    void *stream);
int wce_front_end_sync_stf(wce_ctx *ctx, const wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                           int64_t n_frames, const wce_complex *ltf, double threshold_stf, double threshold_ltf,
                           int32_t backoff, int32_t *start, double *cfo, double *metric_stf, double *metric_ltf,
                           void *stream);

/* ---- demodulation: pilot phase tracking, slicer, EVM (the reference's README
 * applies the estimate "before the symbols are decoded"; WiFi_Equalization.m
 * stops at the equalized symbols) ----
 * wce_demodulate equalizes frame f with any channel estimate the caller holds,
 * h[f*h_stride + k] (a wce_outputs array, PS_MMSE included), removes each
 * block's common phase, decides every symbol and scores the frame.  It reads
 * in->tx, in->rx, the strides and n_frames; rx_pre, tx_pre, block and
 * semantics are ignored.  The ctx only selects the device.
 *
 * Frame f, block b = 0..14, subcarrier k != 26 (k = 26 is DC: eq = 0, sym = 0);
 * pilots P = {5, 19, 33, 47}:
 *   blend     h_lt == NULL: Hu_b = h.  Else Hu_b = ((15-(b+1))/15) h_lt + ((b+1)/15) h
 *             (WiFi_Equalization.m:4-5), in WCE_EQUALIZE's operation order.
 *   tracking  (WCE_DEMOD_TRACK) z_b = sum_{p in P, ascending} rx_b[p] conj(Hu_b[p] tx_b[p]),
 *             theta_b = atan2(Im z_b, Re z_b) in (-pi, pi], rotor r_b = conj(z_b) / |z_b|;
 *             z_b = 0: r_b = 1, theta_b = 0.  Without the flag r_b = 1, theta_b = 0.
 *             This is the maximum-likelihood common phase: each pilot weighs |H|^2 |x|^2.
 *   equalize  e_b[k] = (rx_b[k] / Hu_b[k]) r_b; where r_b = 1 the product is skipped, so
 *             with h_lt = the frame's lt_ls and h = a PS estimate an untracked eq is
 *             WCE_EQUALIZE's, bit for bit.
 *   slice     d = scale K, K the double nearest to 1, 1/sqrt 2, 1/sqrt 10, 1/sqrt 42 for
 *             BPSK, QPSK, 16-QAM, 64-QAM.  An axis of M levels (2, 2, 4, 8): level
 *             i = clamp(floor(v / (2d) + M/2), 0, M-1), decided coordinate (2i - (M-1)) d;
 *             v / (2d) is taken as v times the double 1 / (2d), so a coordinate within
 *             an ulp of a boundary may fall either way.  Gray label g(i) = i ^ (i >> 1)
 *             (802.11's 16- and 64-QAM tables, b0 first); sym = g(i_I) << (bits/2) | g(i_Q).
 *             BPSK slices the real axis only (sym = i_I, decided point on the real axis);
 *             pilots are sliced as BPSK with d = scale whatever `modulation` is.
 *   score     over the 48 x 15 data symbols: evm[f] = sqrt(sum |e - ref|^2 / sum |ref|^2),
 *             ref = the tx symbol (WCE_DEMOD_REF_TX) or the decided point; nerr[f] = the
 *             number of data symbols whose sym differs from the sym of the tx symbol put
 *             through the same slicer.
 *
 *  - A symbol whose e is not finite gets sym = 0xFF and counts in nerr; a frame with
 *    such a data symbol gets evm = NaN.  No other frame changes by a bit.
 *  - A frame's bits depend only on its own data and the call's arguments, not on
 *    its place in the batch or the batch's size.
 *  - Asynchronous on `stream`; nothing is read back, so it follows wce_estimate on
 *    the same stream with no host hop.  Absent outputs cost no stores.
 *  - WCE_EINVAL (text in wce_last_error()) before any launch: a NULL in, p, out,
 *    p->h, in->tx or in->rx; every output NULL; h_stride < 53; an unknown
 *    modulation or flag bit; scale not positive and finite; eq or sym strides
 *    too small (block stride < 53, or, with more than one frame, frame stride <
 *    14 block strides + 53); theta or evm not 8-byte aligned; nerr not 4-byte
 *    aligned; h, h_lt or eq not 16-byte aligned; n_frames < 0 or > 2^31 - 1; the
 *    frames' block_stride < 53 or, with more than one frame, frame_stride < 14
 *    block strides + 53.  n_frames == 0 is WCE_OK. */
enum { WCE_MOD_BPSK = 1, WCE_MOD_QPSK = 2, WCE_MOD_QAM16 = 4, WCE_MOD_QAM64 = 6 };  /* bits per symbol */
#define WCE_DEMOD_TRACK  (1u << 0)   /* remove each block's common pilot phase */
#define WCE_DEMOD_REF_TX (1u << 1)   /* EVM against in->tx instead of the decided point */

typedef struct {
    const wce_complex *h;     /* device; h[f*h_stride + k]: any complex-double estimate, e.g. a wce_outputs array */
    const wce_complex *h_lt;  /* device, same stride; NULL = no blend */
    int64_t h_stride;         /* >= 53 */
    int32_t modulation;       /* WCE_MOD_*, of the 48 data subcarriers (pilots are BPSK) */
    uint32_t flags;           /* WCE_DEMOD_* */
    double scale;             /* amplitude of a unit-energy constellation point in eq units (inputs.h: 8.8753) */
} wce_demod;

typedef struct {              /* every pointer device, each may be NULL = not wanted */
    wce_complex *eq;          /* eq[f*eq_frame_stride + b*eq_block_stride + k] */
    uint8_t *sym;             /* sym[f*sym_frame_stride + b*sym_block_stride + k] */
    double *theta;            /* theta[f*15 + b], radians, (-pi, pi] */
    double *evm;              /* evm[f] */
    uint32_t *nerr;           /* nerr[f] */
    int64_t eq_frame_stride, eq_block_stride, sym_frame_stride, sym_block_stride;
} wce_demod_out;

int wce_demodulate(wce_ctx *ctx, const wce_frames *in, const wce_demod *p, const wce_demod_out *out, void *stream);

/* ---- per-block decision-directed tracking ("spectral temporal averaging", Fernandez
 * et al., IEEE Trans. Veh. Technol., 2012; the reference assumes the channel of a frame
 * does not move over its 15 blocks) ----
 * wce_track_demodulate is wce_demodulate for a channel that moves inside the frame
 * (the reference samples at 10 MHz, 802.11p's numerology: a vehicular channel
 * decorrelates noticeably within the 120 us of a frame).  Frame f starts from
 * H_0 = h[f*h_stride + k], any estimate (LT_LS, PS_MMSE, wce_reencode's H_dd ...),
 * and re-estimates the channel block by block from its own decisions, smoothed over
 * frequency and time.  It reads in->tx, in->rx, the strides and n_frames as
 * wce_demodulate does.  V = {0..52} without 26, pilots P = {5, 19, 33, 47}; for
 * b = 0..14 in order:
 *   phase     z_b, theta_b and r_b are wce_demodulate's with Hu_b = H_b (WCE_TRACK_PHASE;
 *             z_b = 0: r_b = 1, theta_b = 0; without the flag r_b = 1, theta_b = 0).  The
 *             rotor is conj(z_b) / sqrt(|z_b|^2) with |z_b|^2 formed in fp64: |z_b| outside
 *             about 1e-150 .. 1e150 is outside the call's range.
 *   equalize  e_b[k] = (rx_b[k] / H_b[k]) r_b, e_b[26] = 0.
 *   decide    wce_demodulate's slicer: the same d, labels, 0xFF rule and BPSK pilots with
 *             d = scale; it gives sym and the decided point dec_b[k].
 *   known     x^_b[k] = in->tx on the pilots always, and on every k with WCE_TRACK_KNOWN_TX
 *             (the data-aided bound: nothing decided is fed back); else x^_b[k] = dec_b[k].
 *   estimate  G_b[k] = rx_b[k] r_b / x^_b[k], k in V.
 *   frequency S_b[k] = the sum of G_b[j] over N_k = {j in V : |j - k| <= beta}, divided by
 *             |N_k|.  The window is in index space: it runs across DC and is clipped at 0
 *             and 52.  The order of the sum is the implementation's.
 *   time      H_{b+1}[k] = H_b[k] + mu (S_b[k] - H_b[k]), k in V.  mu == 0 skips the update:
 *             every H_b is h, bit for bit.  Entry 26 is carried from h unchanged.
 *   score     evm and nerr as wce_demodulate (WCE_TRACK_REF_TX: EVM against in->tx).
 * h_blocks[f][b] = H_b, the estimate block b was equalized with (wce_soft_demap_blocks
 * weighs the soft bits by it); h_last[f] = H_15.
 *
 *  - Asynchronous on `stream`; nothing is read back and nothing allocated; the ctx only
 *    selects the device.  Absent outputs cost no stores.
 *  - A frame's bits depend only on its own data and the call's arguments.  A non-finite
 *    rx or h entry may make later blocks of that frame non-finite within beta of it (a
 *    non-finite pilot: the whole block and what follows); its data symbols get 0xFF and
 *    the frame gets evm = NaN.  No other frame changes by a bit.
 *  - WCE_EINVAL (text in wce_last_error()) before any launch: everything wce_demodulate
 *    rejects; mu outside [0, 1] or not finite; beta outside 0..4; an unknown flag bit;
 *    h_blocks strides too small (the rule of eq); h_last_stride < 53 (with h_last);
 *    h_blocks or h_last not 16-byte aligned; every output NULL.  n_frames == 0 is WCE_OK. */
#define WCE_TRACK_PHASE    (1u << 0)  /* per-block common pilot phase, as WCE_DEMOD_TRACK */
#define WCE_TRACK_REF_TX   (1u << 1)  /* EVM against in->tx, as WCE_DEMOD_REF_TX */
#define WCE_TRACK_KNOWN_TX (1u << 2)  /* x^ = in->tx on every subcarrier: the data-aided bound, nothing decided is fed back */

typedef struct {
    const wce_complex *h;     /* device; H_0 = h[f*h_stride + k], any estimate (LT_LS, PS_MMSE, H_dd ...) */
    int64_t h_stride;         /* >= 53 */
    int32_t modulation;       /* WCE_MOD_*, as wce_demod */
    uint32_t flags;           /* WCE_TRACK_* */
    double scale;             /* as wce_demod.scale */
    double mu;                /* time weight 1/alpha, 0 <= mu <= 1 */
    int32_t beta;             /* frequency half-window, 0..4 subcarriers */
} wce_track;

typedef struct {              /* every pointer device, each may be NULL = not wanted; not all */
    wce_complex *eq;          /* as wce_demod_out */
    uint8_t *sym;
    double *theta;
    double *evm;
    uint32_t *nerr;
    int64_t eq_frame_stride, eq_block_stride, sym_frame_stride, sym_block_stride;
    wce_complex *h_blocks;    /* h_blocks[f*hb_frame_stride + b*hb_block_stride + k] = H_b */
    int64_t hb_frame_stride, hb_block_stride;
    wce_complex *h_last;      /* h_last[f*h_last_stride + k] = H_15 */
    int64_t h_last_stride;
} wce_track_out;

int wce_track_demodulate(wce_ctx *ctx, const wce_frames *in, const wce_track *p, const wce_track_out *out, void *stream);

/* ---- decoding: soft demapper, deinterleaver, Viterbi decoder (IEEE 802.11-2020
 * 17.3.5.5 to 17.3.5.8; the reference stops at the equalized symbols) ----
 * Every 802.11a/g/p payload is convolutionally coded, punctured and interleaved;
 * these two calls take wce_demodulate's eq to information bits on the device.
 * A frame is the 15 blocks of 48 data subcarriers every other call uses
 * (k = 0..52 ascending without the pilots 5, 19, 33, 47 and DC 26).  With bpsc =
 * the WCE_MOD_* value (1, 2, 4, 6) and R the WCE_RATE_* fraction:
 *     N_CBPS = 48 bpsc  coded bits per block,   N_TX = 15 N_CBPS  per frame,
 *     T = N_TX R  information bits per frame = trellis steps (360 .. 3240).
 *
 *   code         shift register with input u_t, K = 7:
 *                A_t = u_t ^ u_{t-2} ^ u_{t-3} ^ u_{t-5} ^ u_{t-6}   (133 octal)
 *                B_t = u_t ^ u_{t-1} ^ u_{t-2} ^ u_{t-3} ^ u_{t-6}   (171 octal)
 *                mother stream A_0 B_0 A_1 B_1 ...  State s, 6 bits: bit 5 = u_{t-1}, bit 0 =
 *                u_{t-6}; the successor of s on input u is (u << 5) | (s >> 1); the encoder starts
 *                in state 0.
 *   puncturing   (17.3.5.6) rate 2/3 keeps the mother positions marked 1 of 1 1 1 0 (A0 B0 A1,
 *                not B1), rate 3/4 those of 1 1 1 0 0 1 (A0 B0 A1 B2), repeating.  Depuncturing
 *                puts LLR 0 at the dropped positions.
 *   interleaver  (17.3.5.7) per block, s = max(bpsc / 2, 1): coded bit k goes to
 *                i = (N_CBPS / 16)(k mod 16) + floor(k / 16), then to
 *                j = s floor(i / s) + (i + N_CBPS - floor(16 i / N_CBPS)) mod s.
 *                Transmitted bit j belongs to data subcarrier floor(j / bpsc), counted over the 48
 *                data subcarriers in ascending k, and is its bit j mod bpsc, b0 first.  b0 is the
 *                top bit of wce_demodulate's label: the first bpsc / 2 bits set the I level, the
 *                rest the Q level, by the same Gray tables.
 *   soft bit     (wce_soft_demap; max-log, weighted by the channel, no noise variance in it)
 *                from e = eq[f][b][k] and Hu_b[k] = h, or the h / h_lt blend exactly as
 *                wce_demodulate defines it:  L = |Hu_b[k]|^2 (D0 - D1),  D_c = the minimum, over
 *                the axis levels (2 i - (M-1)) d whose Gray label has the bit equal to c, of
 *                (v - level)^2;  v = Re e for an I bit, Im e for a Q bit;  d = scale K as in
 *                wce_demodulate.  L > 0 favours bit 1.  A per-frame factor 1 / sigma^2 changes no
 *                decision and is left out; scale by 1 / ow2[f] for true LLRs.  If e or Hu is not
 *                finite every bit of that symbol gets L = 0, an erasure (the NaN row of an
 *                undetected packet decodes from all-zero LLRs).  fp64 arithmetic, rounded once to
 *                float.  A soft bit of finite e and Hu is clamped to +-WCE_LLR_MAX = 2^100, so that
 *                a strong signal saturates and never leaves float's range to be read as an erasure;
 *                the decoder then cannot overflow either: 2 x 3240 x 2^100 < 2^128.
 *                Signal level: Hu times g = 2^k multiplies every unclamped soft bit by g^2, and so do
 *                eq and scale both times g, bit for bit while the soft bits stay normal floats.
 *                Output in DEINTERLEAVED coded order:
 *                llr[f*llr_frame_stride + b*llr_block_stride + k], k < N_CBPS.
 *   decoder      (wce_viterbi_decode) maximum-correlation Viterbi over the depunctured stream,
 *                float metrics, pm_0[0] = 0, pm_0[s != 0] = -inf.  Per step, with the pair
 *                (L_A, L_B) (a non-finite LLR reads as 0), the branch metric of predecessor p into
 *                s' is (+-L_A) + (+-L_B), + where the branch's coded bit is 1; the predecessors of
 *                s' are p0 = 2 (s' & 31) and p1 = p0 + 1; pm[s'] = max(pm[p0] + bm0, pm[p1] + bm1),
 *                p0 wins a tie.  No renormalisation (3240 steps of float need none).  With
 *                WCE_DEC_TERMINATED the traceback starts from state 0 (the caller's last six
 *                information bits are 0), else from the state of the largest final metric, the
 *                lowest state of a tie.  Decoded bit t is bit 5 of the survivor's state after step t.
 *
 *  - bits[f*bits_stride + (t >> 3)], bit t & 7, is information bit t (packed, LSB first); the
 *    unused high bits of the last byte are written 0.  ref_bits is packed the same way and
 *    nbiterr[f] is the number of the T decoded bits that differ from it.
 *  - Both calls are asynchronous on `stream`, read nothing back, allocate nothing and need
 *    only a device-selecting ctx: demodulate, demap and decode queue on one stream with no
 *    host hop.  A frame's results depend only on its own data and the call's arguments.
 *    wce_soft_demap reads p->h, h_lt, h_stride, modulation and scale; p->flags is ignored.
 *  - WCE_EINVAL (text in wce_last_error()) before any launch: a NULL ctx, eq, p, p->h or llr;
 *    an unknown modulation or rate, or an unknown flag bit; scale not positive and finite;
 *    h_stride < 53; a block stride < N_CBPS (< 53 for eq) or, with more than one frame, a frame
 *    stride < 14 block strides + one row (N_CBPS, 53 for eq); bits_stride < ceil(T / 8) (with
 *    bits), ref_stride likewise (with ref_bits); nbiterr without ref_bits; neither bits nor
 *    nbiterr; eq, h or h_lt not 16-byte aligned; llr or nbiterr not 4-byte aligned; n_frames < 0
 *    or > 2^31 - 1.  n_frames == 0 is WCE_OK.
 *  - wce_soft_demap_blocks is wce_soft_demap with an estimate per block, as a tracked
 *    receiver has it: Hu_b[k] = hb[f*hb_frame_stride + b*hb_block_stride + k] (wce_track_demodulate's
 *    h_blocks), 15 more loads per lane, everything else as it is.  Where every block row of a frame
 *    holds the same h its soft bits are wce_soft_demap's with h_lt = NULL, bit for bit.  The same
 *    validation: a NULL ctx, eq, hb or llr; an unknown modulation; scale not positive and finite; eq,
 *    hb or llr strides too small (a row of hb is 53); eq or hb not 16-byte aligned; llr not 4-byte
 *    aligned; n_frames < 0 or > 2^31 - 1.
 *  - wce_decode_info_bits: T for a modulation and rate, or WCE_EINVAL. */
enum { WCE_RATE_1_2 = 0, WCE_RATE_2_3 = 1, WCE_RATE_3_4 = 2 };
#define WCE_DEC_TERMINATED (1u << 0)   /* trace back from state 0 */
#define WCE_LLR_MAX 1267650600228229401496703205376.0   /* 2^100: the largest magnitude of a soft bit */

int wce_soft_demap(wce_ctx *ctx, const wce_complex *eq, int64_t eq_frame_stride, int64_t eq_block_stride,
                   const wce_demod *p, int64_t n_frames, float *llr, int64_t llr_frame_stride,
                   int64_t llr_block_stride, void *stream);
int wce_soft_demap_blocks(wce_ctx *ctx, const wce_complex *eq, int64_t eq_frame_stride, int64_t eq_block_stride,
                          const wce_complex *hb, int64_t hb_frame_stride, int64_t hb_block_stride,
                          int32_t modulation, double scale, int64_t n_frames, float *llr, int64_t llr_frame_stride,
                          int64_t llr_block_stride, void *stream);
int wce_viterbi_decode(wce_ctx *ctx, const float *llr, int64_t llr_frame_stride, int64_t llr_block_stride,
                       int32_t modulation, int32_t rate, uint32_t flags, int64_t n_frames, uint8_t *bits,
                       int64_t bits_stride, const uint8_t *ref_bits, int64_t ref_stride, uint32_t *nbiterr,
                       void *stream);
int wce_decode_info_bits(int32_t modulation, int32_t rate);

/* ---- decision-directed estimation: re-encoder and data-aided LS (the reference
 * estimates from the preamble and the 4 pilots of a block only) ----
 * Once a frame is decoded its 48 x 15 data symbols are known again, with far fewer
 * errors than the slicer made.  wce_reencode runs wce_viterbi_decode's information
 * bits forwards through the code, puncturing, interleaver and bit-to-subcarrier
 * mapping defined above to the transmitted symbols x^ (out->tx), and estimates the
 * channel from all of them (out->h).  It is the transmitter of this library too.
 *
 *   x^, frame f, block b = 0..14, subcarrier k:
 *     encoder    starts in state 0 and runs continuously over the frame's T bits,
 *                bits[f*bits_stride + (t >> 3)], bit t & 7; the unused high bits of a row's
 *                last byte are ignored.
 *     punctured  the kept mother bits in order; coded bit k of block b is punctured-stream bit
 *                b N_CBPS + k.  It is transmitted as bit j(k); data subcarrier floor(j / bpsc)
 *                gets bit j mod bpsc, b0 first.
 *     data       an axis whose Gray label is g has the level index i with i ^ (i >> 1) = g and
 *                the coordinate fl((2 i - (M - 1)) d), d = fl(scale K): exactly the slicer's
 *                decided coordinate in wce_demodulate, so a re-encoded symbol is bit-identical
 *                to the point the slicer decides for that label.  BPSK: Im = 0.
 *     DC         x^ = 0.
 *     pilots     (5, 19, 33, 47) in != NULL and in->tx != NULL: copied from in->tx, the only
 *                entries of in->tx the call reads.  Else 802.11's, scale {1, 1, 1, -1} p_b with
 *                p_0..14 = 1 1 1 1 -1 -1 -1 1 -1 -1 -1 -1 1 1 -1 (17.3.5.10's first 15 terms).
 *   H_dd (out->h; needs in and in->rx), the LS estimate of the channel after the block phases
 *   the demodulator tracked are removed:
 *       H_dd[k] = sum_b conj(x^_b[k]) rx_b[k] r_b / sum_b |x^_b[k]|^2,   H_dd[26] = 0,
 *   b ascending; r_b = cos theta_b - i sin theta_b with p->theta, 1 without it (and where
 *   r_b = 1 the product is skipped, so theta = 0 gives the bits of theta == NULL).  The second
 *   pass equalizes with it: wce_demodulate with h = H_dd, h_lt = NULL, WCE_DEMOD_TRACK.
 *
 *  - One launch serves both outputs; out->h alone never writes or re-reads x^ through memory,
 *    and gives the bits the call with both outputs gives.
 *  - A non-finite rx or theta makes the affected entries of H_dd non-finite (a theta all 53 of
 *    them but DC); no other frame changes by a bit.  A frame's result depends only on its own
 *    data and the call's arguments.
 *  - Asynchronous on `stream`; reads nothing back and allocates nothing; the ctx only selects
 *    the device: decode, re-encode and the second demodulation queue on one stream with no
 *    host hop.
 *  - WCE_EINVAL (text in wce_last_error()) before any launch: a NULL ctx, p, out or p->bits;
 *    both outputs NULL; out->h without in or in->rx; in given with in->n_frames != n_frames; an
 *    unknown modulation or rate; scale not positive and finite; bits_stride < ceil(T / 8);
 *    tx_block_stride < 53 or, with more than one frame, tx_frame_stride < 14 tx_block_stride +
 *    53 (with out->tx), likewise the frames' own strides (with in); h_stride < 53 (with out->h);
 *    out->tx, out->h, in->rx or in->tx not 16-byte aligned; theta not 8-byte aligned; n_frames
 *    < 0 or > 2^31 - 1.  n_frames == 0 is WCE_OK. */
typedef struct {
    const uint8_t *bits;      /* device; wce_viterbi_decode's packed bits: bits[f*bits_stride + (t>>3)], bit t&7 */
    int64_t bits_stride;      /* bytes, >= ceil(T/8); rows need no alignment */
    int32_t modulation, rate; /* WCE_MOD_*, WCE_RATE_* */
    double scale;             /* as wce_demod.scale */
    const double *theta;      /* device, theta[f*15+b] as wce_demodulate writes it; NULL = 0 */
} wce_reencode_par;
typedef struct {              /* each pointer may be NULL = not wanted; not both */
    wce_complex *tx;          /* tx[f*tx_frame_stride + b*tx_block_stride + k], k < 53 */
    int64_t tx_frame_stride, tx_block_stride;
    wce_complex *h;           /* h[f*h_stride + k]: the data-aided estimate */
    int64_t h_stride;
} wce_reencode_out;
int wce_reencode(wce_ctx *ctx, const wce_reencode_par *p, const wce_frames *in, int64_t n_frames,
                 const wce_reencode_out *out, void *stream);

/* ---- framing the payload: SERVICE, PSDU, tail and pad, scrambler, CRC-32 FCS (IEEE
 * 802.11-2020 17.3.5.2 to 17.3.5.5 and 9.2.4.8; the reference stops at channel estimates) ----
 * A receiver in the field has no reference bits: it descrambles the DATA field, cuts the
 * PSDU out of it and checks the frame check sequence.  wce_psdu_frame builds the T =
 * wce_decode_info_bits(modulation, rate) information bits of a frame from a payload, packed
 * as wce_reencode reads them; wce_psdu_deframe takes the rows wce_viterbi_decode writes
 * (decode with flags = 0: the tail is not at the end of the field, so the encoder does not
 * end in state 0) back to the PSDU and says whether its FCS holds.
 *
 *   L          the PSDU length in octets, the 4 of the FCS included: 4 <= L <= max =
 *              wce_psdu_max_len(modulation, rate) = (T - 22) / 8 rounded down (42 at BPSK 1/2,
 *              402 at 64-QAM 3/4).
 *   field      bit t before scrambling: t = 0..15 SERVICE, 0;  t = 16 + 8 i + j bit j (LSB
 *              first) of PSDU octet i < L;  the next six bits the tail;  the rest, up to T - 1,
 *              pad, 0 (there always is some).  PSDU octet i is byte i + 2 of a packed row.
 *   scrambler  x^7 + x^4 + 1: state x1..x7, each step outputs s = x4 ^ x7, then x7 <- x6 ..
 *              x2 <- x1, x1 <- s; bit i - 1 of the seed (1..127) is the initial x_i, so
 *              s_t = s_(t-4) ^ s_(t-7) from t = 7 on.  Seed 127 sends 00001110 11110010 ..., seed 93
 *              (x7..x1 = 1011101) 01101100 00011001 ...  Information bit t = field bit t ^ s_t,
 *              but the six tail positions, which are 0 after scrambling.
 *   FCS        CRC-32 (polynomial 0x04C11DB7, register preset to ones, result complemented:
 *              zlib's crc32, "123456789" -> 0xCBF43926) over PSDU octets 0 .. L - 5, stored in
 *              octets L - 4 .. L - 1, least significant octet first.  A good PSDU has
 *              crc32(all L octets) == 0x2144DF1C.
 *
 *  - wce_psdu_frame reads payload[f*payload_stride + i], i < L_f - 4 (nothing with L_f = 4;
 *    payload may be NULL when every frame has L = 4), appends the FCS, scrambles with the
 *    frame's seed and writes bits[f*bits_stride + (t >> 3)], bit t & 7; the unused high bits of
 *    the last byte are 0 and bytes of a row beyond ceil(T / 8) are not touched.
 *  - wce_psdu_deframe takes the first seven bits of a row as s_0..s_6 (SERVICE bits 0..6 are
 *    0), continues the sequence by the recurrence and descrambles.  out->seed[f] is the
 *    initial state that sends those seven bits.  If all seven are 0 (what an undetected
 *    packet's all-zero decode gives) seed = 0, fcs_ok = 0 and the PSDU is written
 *    undescrambled.  out->psdu[f*psdu_stride + i], i < L_f, and nothing beyond; fcs_ok[f] = 1
 *    where the CRC over the L_f octets leaves the residue; *n_good += the number of such
 *    frames (one atomic add per workgroup).  SERVICE bits 7..15, the tail and the pad are not
 *    checked (the standard's receiver ignores them).  p->seed and p->seeds are ignored.
 *  - p->lengths / p->seeds give every frame its own length / seed.  One that is out of range
 *    cannot be refused on the host (nothing is read back): framing writes that frame's row
 *    as zeros; deframing gives fcs_ok = 0, seed = 0 and writes no PSDU octet.  No other frame
 *    changes: a frame's result depends only on its own row and the arguments.
 *  - Asynchronous on `stream`; nothing is read back, nothing allocated, the ctx only selects
 *    the device.  Rows need no alignment (45-byte strides are the normal case).  All offsets
 *    are 64-bit.
 *  - WCE_EINVAL (text in wce_last_error()) before any launch: a NULL ctx, p, bits or out;
 *    every output NULL; payload NULL with length > 4 or with lengths; an unknown modulation
 *    or rate; length outside 4..max (without lengths); seed outside 1..127 (framing, without
 *    seeds); bits_stride < ceil(T / 8); payload_stride < max - 4 or psdu_stride < max with
 *    lengths, else < L - 4 / < L; lengths, fcs_ok or n_good not 4-byte aligned; n_frames < 0
 *    or > 2^31 - 1.  n_frames == 0 is WCE_OK. */
typedef struct {
    int32_t modulation, rate; /* WCE_MOD_*, WCE_RATE_*: they give T */
    int32_t length;           /* L for every frame, where lengths == NULL */
    int32_t seed;             /* 1..127 for every frame, where seeds == NULL (framing only) */
    const int32_t *lengths;   /* device, [n_frames], each 4..max; NULL = length */
    const uint8_t *seeds;     /* device, [n_frames], each 1..127; NULL = seed (framing only) */
} wce_psdu_par;
typedef struct {              /* each pointer may be NULL = not wanted; not all */
    uint8_t *psdu;            /* psdu[f*psdu_stride + i], i < L_f: the descrambled octets, FCS included */
    int64_t psdu_stride;
    uint8_t *seed;            /* [n_frames]: the recovered seed, 0 = none */
    uint32_t *fcs_ok;         /* [n_frames]: 1 good, 0 bad */
    uint32_t *n_good;         /* one counter: the call ADDS the number of good frames */
} wce_psdu_out;
int wce_psdu_max_len(int32_t modulation, int32_t rate);
int wce_psdu_frame(wce_ctx *ctx, const wce_psdu_par *p, const uint8_t *payload, int64_t payload_stride,
                   int64_t n_frames, uint8_t *bits, int64_t bits_stride, void *stream);
int wce_psdu_deframe(wce_ctx *ctx, const wce_psdu_par *p, const uint8_t *bits, int64_t bits_stride,
                     int64_t n_frames, const wce_psdu_out *out, void *stream);

/* ---- transmitter and channel: symbols -> clean waveform -> raw capture windows (the
 * reference's WiFi_RX.m:4-9 declares SNR, channel_model, FO and Pawgn and uses none of
 * them: its input is one recorded capture) ----
 * wce_reencode stops at the frequency-domain symbols.  These three calls take them to
 * what an antenna would have recorded, on the device, so that wce_front_end_sync and the
 * receive chain behind it run on as many packets as an error-rate experiment needs, at a
 * chosen SNR, through a chosen multipath channel and carrier offset.
 *
 * wce_modulate is the inverse of wce_front_end_blocks / _preamble:
 *   block     from 53 bins X[i]: Y[(i - 26) mod 64] = X[i], the other 11 bins 0;
 *             y[n] = (1/64) sum_k Y[k] e^(+2 pi i k n / 64): MATLAB's ifft, the exact
 *             inverse of circshift(fft(., 64), 26)(1:53).
 *   field     present iff tx_pre != NULL; 160 samples: y[32..63], y, y of
 *             tx_pre[f*pre_stride + i] (pre_stride == 0: one shared preamble).  y is computed
 *             once: the two copies, and the prefix, are the same bits.
 *   data      block b is 80 samples: y_b[48..63], y_b of sym[f*frame_stride + b*block_stride + i].
 *   waveform  wave[f*wave_stride + m], m < S = 160 [field] + 80 n_blocks: the field, then
 *             blocks 0 .. n_blocks - 1.  n_blocks == 0 with a field is allowed.
 *   There is no spectral windowing: the recorded tx_packet has the first prefix sample of
 *   every block, and of the field, shaped by a window; this call does not do that.
 *
 * wce_channel turns a clean waveform into a capture window.  s[m] = the waveform for m in
 * [0, wave_len), 0 outside; frame f, window sample i < capture_len:
 *   y[m] = sum_{t < n_taps, t ascending} h[f][t] s[m - t]       0 <= m < wave_len + n_taps - 1
 *   r[m] = y[m] exp(+2 pi i cfo[f] n),   n = m - 160 field
 *   capture[f][i] = w[f][i] + (r[i - delay[f]] if 0 <= i - delay[f] < wave_len + n_taps - 1, else 0)
 *   time      the axis of wce_front_end_*_cfo: n = 0 at the packet's first sample after the
 *             field.  The rotor is that call's exact-phase construction with the opposite sign
 *             (the phase cfo n is reduced exactly before sincospi sees it); where cfo[f] == 0.0
 *             the product is skipped.  A waveform that overhangs the window on either side is
 *             clipped silently.
 *   noise     exactly Gaussian, by Box-Muller on the counter RNG of wce_synth_frames:
 *             key = mix64(seed ^ mix64(first_frame + f)), a = mix64(key ^ 2i), b = mix64(key ^ (2i + 1)),
 *             u1 = ((a >> 11) + 1) 2^-53 in (0, 1], u2 = (b >> 11) 2^-53,
 *             w = sqrt(ow2[f] / 2) sqrt(-2 ln u1) (cos 2 pi u2 + i sin 2 pi u2)
 *             (mix64: splitmix64's finaliser, x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30)
 *             0xBF58476D1CE4E5B9; x = (x ^ x >> 27) 0x94D049BB133111EB; x ^ x >> 31).
 *             It depends on (seed, first_frame + f, i) only: shards regenerate identical windows,
 *             and the same seed with another channel gives the same noise.  ow2[f] == 0 is
 *             allowed: that frame gets no noise, as every frame does with ow2 == NULL.
 *   guard     a frame whose ow2[f] is negative or not finite, whose cfo[f] or one of whose
 *             taps is not finite, or whose waveform holds a non-finite sample gets NaN in every
 *             sample of its window (so wce_front_end_sync gives it start = -1); no other frame
 *             changes by a bit.  Padding beyond capture_len is never written.
 *
 * wce_transmit is both in one launch, bit-identical to wce_modulate followed by wce_channel
 * on the same arguments (p->field is ignored: the field is present iff tx_pre != NULL), and
 * the clean waveform never goes through memory.
 *
 *  - All three are asynchronous on `stream`, read nothing back and allocate nothing; the
 *    ctx only selects the device.  A frame's bits depend only on its own data, its global
 *    index first_frame + f and the call's arguments.
 *  - WCE_EINVAL (text in wce_last_error()) before any launch: a NULL ctx, p, wave or capture;
 *    sym NULL with n_blocks > 0; n_blocks outside 0..15; no field and n_blocks == 0; n_taps
 *    outside 1..16; taps_stride neither 0 nor >= n_taps; with n_blocks > 0, block_stride < 53
 *    or, with more than one frame, frame_stride < (n_blocks - 1) block_stride + 53; pre_stride
 *    neither 0 nor >= 53; wave_stride < S, or < wave_len; capture_stride < capture_len;
 *    capture_len or wave_len < 1 or >= 2^31; a complex pointer not 16-byte aligned; cfo or
 *    ow2 not 8-byte aligned; delay not 4-byte aligned; n_frames < 0 or > 2^31 - 1.
 *    n_frames == 0 is WCE_OK. */
typedef struct {
    const wce_complex *taps;  /* device; taps[f*taps_stride + t], t < n_taps; NULL = one unit tap */
    int64_t taps_stride;      /* >= n_taps; 0 = one set shared by all frames */
    int32_t n_taps;           /* 1..16 (within the 16-sample cyclic prefix) */
    int32_t field;            /* 1: the waveform starts with a 160-sample field (sets the time origin) */
    const double *cfo;        /* device, cycles per sample per frame; NULL = 0 */
    const double *ow2;        /* device, noise variance per complex sample per frame; NULL = no noise */
    const int32_t *delay;     /* device, window index of waveform sample 0 per frame; NULL = 0; any sign */
    uint64_t seed;
    int64_t first_frame;      /* global index of frame 0, as in wce_synth_frames */
} wce_channel_par;

int wce_modulate(wce_ctx *ctx, const wce_complex *tx_pre, int64_t pre_stride, const wce_complex *sym,
                 int64_t frame_stride, int64_t block_stride, int32_t n_blocks, int64_t n_frames,
                 wce_complex *wave, int64_t wave_stride, void *stream);
int wce_channel(wce_ctx *ctx, const wce_complex *wave, int64_t wave_stride, int64_t wave_len, int64_t n_frames,
                const wce_channel_par *p, wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                void *stream);
int wce_transmit(wce_ctx *ctx, const wce_complex *tx_pre, int64_t pre_stride, const wce_complex *sym,
                 int64_t frame_stride, int64_t block_stride, int32_t n_blocks, int64_t n_frames,
                 const wce_channel_par *p, wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                 void *stream);

/* ---- a channel that fades within the packet: wce_channel_tv, wce_transmit_tv ----
 * wce_channel and wce_transmit hold one set of taps per frame for the whole packet.  These
 * two calls are theirs with taps that move sample by sample: each tap is interpolated
 * linearly between knots, n_knots sets of n_taps taps knot_period (P) samples apart.  The
 * channel travels with the packet: knot k sits at waveform-output sample m = k P, m = 0
 * being the output under the first clean sample, whatever delay[f] is.
 * For 0 <= m < wave_len + n_taps - 1, with a[k][t] = knots[f*frame_stride + k*knot_stride + t]:
 *   k = floor(m / P),  j = m - k P                          (an integer below P: exact)
 *   d[k][t] = (a[k+1][t] - a[k][t]) / P                     real and imaginary part each: one fp64
 *                                                           subtraction, one fp64 division
 *   h_t(m)  = ( fma(j, d.re, a[k][t].re), fma(j, d.im, a[k][t].im) )
 *   y[m]    = sum_{t < n_taps, t ascending} h_t(m) s[m - t]  wce_channel's two fmas a part
 * and the rotor, the placement by delay[f], the clipping and the noise are wce_channel's, word
 * for word; the noise depends on (seed, first_frame + f, i) only, so the same seed gives a
 * static and a fading channel the same noise.
 *   cover     the knots cover every output, nothing is extrapolated:
 *             (n_knots - 1) P > wave_len + n_taps - 2; the smallest such count is
 *             floor((wave_len + n_taps - 2) / P) + 2: 19 knots for a full packet (1,360 samples)
 *             at P = 80, one at every block boundary, two segments under the field.  Knots beyond
 *             the last output's segment are read by the guard only.
 *   guard     wce_channel's, and a frame one of whose n_knots x n_taps knot values is not finite,
 *             used by an output or not: NaN in every sample of its window; no other frame changes
 *             by a bit.
 *   constant  where every knot of a frame equals h[t] (and no part of h is a negative zero),
 *             d is +0 and h_t(m) is h[t] exactly: that frame's window is wce_channel's (or
 *             wce_transmit's) with taps = h, bit for bit.
 *   fused     wce_transmit_tv is wce_modulate followed by wce_channel_tv on the same arguments,
 *             bit for bit (p->field is ignored, as in wce_transmit).
 *  - Asynchronous on `stream`, nothing read back, nothing allocated, as the static calls; a
 *    frame's bits depend only on its own data, its knots, first_frame + f and the arguments.
 *  - WCE_EINVAL before any launch: every refusal of wce_channel (for wce_channel_tv) or
 *    wce_transmit (for wce_transmit_tv) that does not concern taps, and: knots NULL or not
 *    16-byte aligned; n_knots < 2; knot_period outside 16..2^20 (16 is the cyclic prefix: a
 *    run of 8 outputs then meets one knot at most); knot_stride < n_taps; frame_stride neither
 *    0 nor >= (n_knots - 1) knot_stride + n_taps; knots that do not cover the output.
 *    n_frames == 0 is WCE_OK. */
typedef struct {
    const wce_complex *knots; /* device; knots[f*frame_stride + k*knot_stride + t], k < n_knots, t < n_taps */
    int64_t frame_stride;     /* >= (n_knots - 1) knot_stride + n_taps; 0 = one trajectory shared by all frames */
    int64_t knot_stride;      /* >= n_taps */
    int32_t n_knots;          /* >= 2, and enough to cover the output */
    int32_t knot_period;      /* P, samples between knots: 16..2^20 */
    int32_t n_taps;           /* 1..16 */
    int32_t field;            /* as wce_channel_par's, and so are the five below */
    const double *cfo;
    const double *ow2;
    const int32_t *delay;
    uint64_t seed;
    int64_t first_frame;
} wce_fading_par;

int wce_channel_tv(wce_ctx *ctx, const wce_complex *wave, int64_t wave_stride, int64_t wave_len, int64_t n_frames,
                   const wce_fading_par *p, wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                   void *stream);
int wce_transmit_tv(wce_ctx *ctx, const wce_complex *tx_pre, int64_t pre_stride, const wce_complex *sym,
                    int64_t frame_stride, int64_t block_stride, int32_t n_blocks, int64_t n_frames,
                    const wce_fading_par *p, wce_complex *capture, int64_t capture_stride, int64_t capture_len,
                    void *stream);

/* ---- receive diversity: maximal-ratio combining of antenna branches (the reference
 * has one receive antenna; 802.11p radios ship with two, because a deep fade on one
 * branch is what loses a packet) ----
 * A radio with A antennas records A captures of each packet.  Every stage in front of
 * the combiner runs on the A x B windows as on any batch: sync, the _at front end,
 * wce_estimate / wce_estimate_noise over A x B frames.  wce_combine then folds the A
 * branches of each packet into one received stream and one channel estimate with the
 * layouts every later call reads, so wce_demodulate, wce_track_demodulate,
 * wce_soft_demap(_blocks), wce_viterbi_decode and wce_reencode run on them unchanged.
 *
 * Branch a < A = n_branches of packet f < n_frames holds
 *     rx_a[b][k] = rx[a*rx_branch_stride + f*rx_frame_stride + b*rx_block_stride + k],
 *     h_a[k]     = h[a*h_branch_stride + f*h_stride + k]   any estimate (LT_LS, PS_MMSE, H_dd ...),
 *     ow2_a      = ow2[a*ow2_branch_stride + f]             its noise variance, with ow2 != NULL.
 * Branch-major arrays ([A][B]..., what one transmit call per branch with first_frame =
 * a*B leaves) have branch strides that span a whole branch; a branch-minor layout (the
 * branches of a block, or of a packet, next to each other) has a small one.  With
 * V = {0..52} without 26 and v_a = 1 / ow2_a (1 when ow2 == NULL):
 *     live(a)    every h_a[k], k in V, is finite, and (ow2 == NULL or ow2_a is finite and > 0)
 *     g2[k]      = sum over live a, a ascending, of v_a |h_a[k]|^2,    g[k] = sqrt(g2[k])
 *     rx_c[b][k] = (sum over live a, a ascending, of v_a conj(h_a[k]) rx_a[b][k]) / g[k]    k in V
 *     h_c[k]     = g[k] + 0i                                                               k in V
 *     rx_c[b][26] = 0, h_c[26] = 0; where g[k] == 0, rx_c[b][k] = 0 and h_c[k] = 0.
 * out->rx[f*rx_frame_stride + b*rx_block_stride + k] = rx_c, out->h[f*h_stride + k] = h_c.
 *
 *  - With ow2 the combined stream is whitened: rx_c = g x + n with noise of unit variance
 *    per complex sample whatever the branches' own variances, so wce_soft_demap's
 *    |Hu|^2 (D0 - D1) on (rx_c, h_c) is a true LLR: the factor 1 / ow2[f] its comment says
 *    to scale in by hand is already there.  With ow2 == NULL every weight is 1 and the
 *    branches' common variance sigma^2 is preserved: rx_c = g x + n, var n = sigma^2.
 *    A common factor on every ow2 changes no equalized symbol rx_c / h_c.
 *  - A branch that is not live contributes nothing: the output is, bit for bit, that of
 *    the call made on the live branches alone.  (This is how a lost branch arrives: the
 *    _at calls give an undetected packet a NaN pre_fft, hence a NaN h row and a NaN
 *    ow2.)  A packet with no live branch gets NaN in every entry the call writes for
 *    it, entry 26 included.  A non-finite rx_a[b][k] of a live branch makes rx_c[b][k]
 *    non-finite and changes nothing else.  No sum crosses subcarriers or packets: a
 *    packet's bits depend only on its own data and the arguments.
 *  - Asynchronous on `stream`; nothing is read back and nothing allocated; the ctx only
 *    selects the device.  Each output may be NULL (not both); an absent output costs no
 *    stores, and out->h alone reads no rx.  All offsets are 64-bit.
 *  - WCE_EINVAL (text in wce_last_error()) before any launch: a NULL ctx, p, out, p->rx
 *    or p->h; both outputs NULL; n_branches outside 1..8; n_frames < 0 or > 2^31 - 1; a
 *    block stride < 53 or, with more than one frame, a frame stride < 14 block strides +
 *    53 (p->rx and out->rx, each by its own strides); h_stride < 53 (p->h, out->h); with
 *    more than one branch, a branch stride under which branches overlap: rx_branch_stride
 *    must be >= 53 and either span a branch ((n_frames - 1) frame strides + 14 block strides
 *    + 53), or fit the branches inside a block stride ((A - 1) branch strides + 53 <= block
 *    stride), or between frame and block (>= 14 block strides + 53 and (A - 1) branch strides
 *    + 14 block strides + 53 <= frame stride); h_branch_stride must be >= 53 and either
 *    >= (n_frames - 1) h_stride + 53 or fit (A - 1) of it + 53 inside h_stride;
 *    ow2_branch_stride >= n_frames; rx, h or an output not 16-byte aligned; ow2 not 8-byte
 *    aligned.  n_frames == 0 is WCE_OK.
 *
 * wce_sync_share.  All antennas of a radio share one oscillator and see the packet at the
 * same sample, but a branch in a fade misses its own detection and would arrive at the
 * combiner dead although it has something to contribute at the right start.  For packet
 * p < n_packets and branch a < n_branches let i(a) = a*branch_stride + p.  A branch is live
 * when start[i] >= 0 (start != NULL) and metric[i] is finite; a* is the live branch with the
 * largest metric, the lowest a on a tie.  If there is none nothing is written for p.
 * Otherwise start[i(a)] = start[i(a*)] for every a (start != NULL) and cfo[i(a)] =
 * cfo[i(a*)] (cfo != NULL).  In place, one thread per packet.  metric is
 * wce_front_end_sync's, or wce_front_end_sync_stf's metric_ltf.  start == NULL shares the
 * offset alone (live: a finite metric): for the path without a short field, where
 * wce_front_end_preamble_at estimates each branch's offset once the shared start is known.
 * A shared start that does not fit another branch's window falls to the _at calls' own
 * guard.  Asynchronous on `stream`, nothing read back.  WCE_EINVAL: a NULL ctx or metric;
 * start and cfo both NULL; n_branches outside 1..8; n_packets < 0 or > 2^31 - 1; with
 * more than one branch, branch_stride < n_packets; start not 4-byte, metric or cfo not
 * 8-byte aligned.  n_packets == 0 is WCE_OK. */
#define WCE_COMBINE_MAX_BRANCHES 8

typedef struct {
    const wce_complex *rx;    /* device; rx[a*rx_branch_stride + f*rx_frame_stride + b*rx_block_stride + k] */
    int64_t rx_branch_stride, rx_frame_stride, rx_block_stride;
    const wce_complex *h;     /* device; h[a*h_branch_stride + f*h_stride + k] */
    int64_t h_branch_stride, h_stride;
    const double *ow2;        /* device; ow2[a*ow2_branch_stride + f]; NULL = unit weights */
    int64_t ow2_branch_stride;
    int32_t n_branches;       /* A, 1..WCE_COMBINE_MAX_BRANCHES */
} wce_combine_par;

typedef struct {              /* each pointer may be NULL = not wanted; not both */
    wce_complex *rx;          /* rx[f*rx_frame_stride + b*rx_block_stride + k] = rx_c */
    int64_t rx_frame_stride, rx_block_stride;
    wce_complex *h;           /* h[f*h_stride + k] = h_c */
    int64_t h_stride;
} wce_combine_out;

int wce_combine(wce_ctx *ctx, const wce_combine_par *p, int64_t n_frames, const wce_combine_out *out, void *stream);
int wce_sync_share(wce_ctx *ctx, int32_t n_branches, int64_t branch_stride, int64_t n_packets, const double *metric,
                   int32_t *start, double *cfo, void *stream);

/* ---- Signal level: what a gain g does to every call ----
 * A capture arrives at whatever level the ADC and the AGC give, and two antennas run two
 * AGCs.  No call has a constant with units, an absolute threshold or an absolute guard:
 * multiplying its inputs by g multiplies its outputs by the power of g its definition
 * carries and changes nothing else.  For g = 2^k that holds bit for bit (integers: equal)
 * while nothing overflows or goes subnormal; tests/gain_model.py is the table and the tests
 * hold it at 2^+-11 and 2^+-40, and at 2^+-100 where every output is fp64.
 *  - wce_front_end_blocks*:  samples g -> sym g.   wce_front_end_preamble*:  lptot g ->
 *    pre_fft g, ow2 g^2, the estimated cfo unchanged.
 *  - wce_front_end_sync, _sync_stf:  capture g, or ltf g -> start, cfo and the metrics unchanged.
 *  - wce_estimate, wce_estimate_noise, every estimator and route.  The channel's gain: rx g,
 *    the frames' rx_pre g, the context's rx_pre g and ow2 g^2 (per-frame ow2 g^2, Rhh g^2) ->
 *    every estimate g, eq unchanged.  The transmitter's convention: tx g, tx_pre g (Rhh / g^2,
 *    the constant-modulus pattern g) -> every estimate / g, eq g.
 *  - wce_demodulate, wce_track_demodulate:  rx g, h g, h_lt g -> eq, sym, theta, evm, nerr
 *    unchanged, h_blocks g, h_last g.  tx g, rx g, scale g -> eq g, everything else unchanged.
 *  - wce_soft_demap, _blocks:  h g (hb g), or eq g and scale g -> llr g^2, up to the clamp.
 *    wce_viterbi_decode:  llr g -> bits and nbiterr unchanged.
 *  - wce_reencode:  rx g -> h g, tx unchanged.  scale g (and the pilots g) -> tx g, h / g.
 *  - wce_combine with ow2: each branch its own gain, rx_a g_a, h_a g_a, ow2_a g_a^2 -> rx_c and
 *    h_c unchanged.  Without: one gain for all, rx_c g and h_c g.
 *  - wce_modulate:  sym g, tx_pre g -> wave g.   wce_channel, wce_transmit and the _tv pair:
 *    taps g (knots g), or the wave (the symbols and tx_pre) g, with ow2 g^2 -> capture g.
 *    wce_short_field:  amplitude g -> wave g. */

/* Non-finite guard.  The reference passes NaN/Inf through
 * silently: main.c's PS_MMSE returns NaN x 53 (main.c:148-212), a zero pilot
 * makes PS_* divide by zero (main.c:82-84), and its dimension checks only
 * print (utils.c:18-19).  One HBM pass over an output array H[f*stride + k]
 * (k < 53; complex double, or complex float with flags = WCE_OUT_LS_F32):
 * bit f % 32 of bitmap[f / 32] (device, ceil(n/32) words, zeroed here) is set
 * iff any of frame f's 53 entries has a NaN or Inf part; *n_bad (device,
 * optional) receives the number of such frames.  Any ctx selects the device
 * (its state need not be loaded).  Asynchronous on `stream`. */
int wce_nonfinite_scan(wce_ctx *ctx, const void *H, int64_t stride, int64_t n_frames, uint32_t flags,
                       uint32_t *bitmap, unsigned long long *n_bad, void *stream);

/* The reference's data format on the device.  Its arrays are `long double
 * complex` (main.c:4-8): on x86-64, two x87 80-bit extended values in 16-byte
 * slots (32 B per complex; bytes 10-15 of a slot are padding).  A host that
 * keeps frames in that format copies the raw bytes to the device and converts
 * there:
 *   wce_ldc_to_complex: n complex values, x87 -> fp64, rounded exactly as the
 *     C cast (double)x on x86 (nearest-even, overflow to Inf, gradual
 *     underflow; NaNs quieted and truncated; invalid encodings -> the x87
 *     default NaN);
 *   wce_complex_to_ldc: fp64 -> x87, exact (the C cast (long double)x),
 *     padding written as zero.
 * Device pointers, 16-byte aligned, not overlapping; asynchronous on
 * `stream` (current device). */
int wce_ldc_to_complex(const void *src, wce_complex *dst, int64_t n, void *stream);
int wce_complex_to_ldc(const wce_complex *src, void *dst, int64_t n, void *stream);

/* ---- multi-GPU: frames are independent, so a batch is sharded
 * over GPUs with no data-path collective; the only exchange is ONE RCCL
 * broadcast of the packed shared state (wce_ctx_state) over xGMI, the
 * analogue of the reference's MPI_Bcast of F / Ryy (main_mpi.c:687-688,
 * 727-728).  RCCL (librccl.so.1) is loaded on first use, so hosts that never
 * call these need no RCCL.  Two launch models:
 *   - one process per GPU (the MPI model of main_mpi.c): rank 0 calls
 *     wce_comm_unique_id, the host distributes the WCE_COMM_ID_BYTES bytes
 *     (MPI_Bcast, a file, a socket), every rank calls wce_comm_init_rank;
 *   - one process driving several GPUs: wce_comm_init_all. */
#define WCE_COMM_ID_BYTES 128
typedef struct wce_comm wce_comm;
int wce_comm_unique_id(void *id);
int wce_comm_init_rank(wce_comm **comm, const void *id, int nranks, int rank, int device);
int wce_comm_init_all(wce_comm **comms, int ndev, const int *devices);
int wce_comm_destroy(wce_comm *comm);
int wce_comm_info(const wce_comm *comm, int *rank, int *nranks, int *device);

/* ONE in-place ncclBroadcast of ctx's shared state from `root` (whose ctx
 * must hold a valid state) into every rank's ctx (which may be empty, see
 * wce_ctx_create_empty); ctx and comm must be on the same device.  Returns
 * once the state has arrived and been validated (a once-per-process setup
 * call, not a per-batch one).  The _all form does the same for n contexts of
 * one process (comms from wce_comm_init_all), as one RCCL group. */
int wce_ctx_broadcast_state(wce_ctx *ctx, wce_comm *comm, int root, void *stream);
int wce_ctx_broadcast_state_all(wce_ctx **ctxs, wce_comm **comms, int n, int root, void **streams);

/* max over ranks of one double (e.g. each shard's parity error, or its time):
 * an 8-byte ncclAllReduce, synchronous.  _all: one value per context of one
 * process, every entry replaced by the maximum. */
int wce_comm_max_f64(wce_comm *comm, double *value, void *stream);
int wce_comm_max_f64_all(wce_comm **comms, int n, double *values, void **streams);

/* Contiguous frame range [first, first + count) of `rank` out of `total`
 * (the first total % nranks ranks take one extra frame). */
int wce_shard(int64_t total, int nranks, int rank, int64_t *first, int64_t *count);

/* ---- thin runtime helpers (so C hosts and tests need no other HIP binding) ---- */
int wce_device_count(int *count);
int wce_set_device(int device);
int wce_malloc(void **ptr, size_t bytes);
int wce_free(void *ptr);
int wce_memcpy_htod(void *dst, const void *src, size_t bytes);
int wce_memcpy_dtoh(void *dst, const void *src, size_t bytes);
int wce_memcpy_dtod(void *dst, const void *src, size_t bytes, void *stream);
int wce_memset(void *dst, int value, size_t bytes);
/* pinned (page-locked) host memory and stream-ordered copies, for hosts that
 * keep frames in host memory and overlap PCIe transfers with estimation */
int wce_host_alloc(void **ptr, size_t bytes);
int wce_host_free(void *ptr);
int wce_memcpy_htod_async(void *dst, const void *src, size_t bytes, void *stream);
int wce_memcpy_dtoh_async(void *dst, const void *src, size_t bytes, void *stream);
int wce_stream_create(void **stream);
int wce_stream_destroy(void *stream);
int wce_stream_synchronize(void *stream);
int wce_event_create(void **event);
int wce_event_destroy(void *event);
int wce_event_record(void *event, void *stream);
/* 1: everything the stream held when the event was recorded has completed; 0: still pending (never waits);
 * negative: an error code. */
int wce_event_query(void *event);
int wce_event_elapsed_ms(float *ms, void *start, void *stop);
const char *wce_last_error(void);
const char *wce_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WCE_H */
