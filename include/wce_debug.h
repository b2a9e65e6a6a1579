/* wce_debug.h -- host-only hooks of libwce.so used by the parity tests to
 * check the 80-bit shared-state precompute without a GPU. */
#ifndef WCE_DEBUG_H
#define WCE_DEBUG_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
/* F and the reference's cofactor invF (utils.c:141-170), 53*53 {re, im} long double pairs */
int wce_debug_reference_F(long double *out);
int wce_debug_reference_invF(long double *out);
/* the State wce_ctx_create builds: C (53*53 {re,im}), H_LT (53), sinc table (4*53), {a, b}, X mask */
int wce_debug_build_state(const double *tx_pre, const double *rx_pre, double ow2, int mode, double *C,
                          double *h_lt, double *sinc, double *ab, unsigned long long *xmask);
/* WCE_MMSE_COV state blob (wce_state_build_cov): the low-rank factor U
 * (C = U U^H; 53 rows x 64 columns {re, im}, zero past the rank), the rank,
 * the solve form (-1 dense, else the Gram system's first block row) and the
 * largest / smallest kept eigenvalue of C.  Outputs may be NULL. */
int wce_debug_cov_factor(const void *blob, size_t bytes, double *U, int *rank, int *k0, double *lmax, double *lmin);
/* A/B switch for the config-5 fusion (LS family + equalization in the MMSE
 * solve's epilogue); on by default.  ctx is a wce_ctx* (include/wce.h). */
struct wce_ctx;
int wce_debug_set_fusion(struct wce_ctx *ctx, int on);
/* A/B switch for the rank-1 path (TEXTBOOK / REF / FRAME_COV): a second
 * bordered row replaces the back-substitution and the C W product; on by
 * default.  Off: back-substitution + MFMA apply (shared modes). */
int wce_debug_set_border_dot(struct wce_ctx *ctx, int on);
/* Frames per launch of the flat-index kernels (LT_LS + PS_Linear, REF
 * PS_MMSE, the non-finite scan): 2^26 by default, so that 53 * frames < 2^32;
 * a smaller multiple of 32 makes tests reach the multi-launch path at small
 * sizes.  0 restores the default.  Process-wide. */
int wce_debug_set_flat_chunk(long long frames);
/* Kernel variant knobs for interleaved A/B timing and the gate's cross-checks
 * in one process (same buffers, same placement).  which 0: REF PS_MMSE (0 =
 * by batch size, default: one element per thread, mmse_ref_elem_kernel, past
 * 196,608 frames, else 512-element chunks on a capped grid; 1 = always the
 * capped chunks; 2 = the chunks on an uncapped grid; 3 = always one element
 * per thread).
 * which 1: LT_LS + PS_Linear in C semantics (2 = one element per thread,
 * ls_elem_kernel, default; 3 = the per-frame LIGHT kernel).  which 2: REF
 * PS_MMSE with LS outputs in one call (0 = one element per thread,
 * ref_ls_elem_kernel, default; 1 = the wave-per-frame fused solve, and REF +
 * WCE_MMSE_FRAME_COV on the general factors).  which 2, 4 and 5 are facts of
 * the route planner (csrc/wce_route.h, wce_debug_route below): wce_estimate
 * reads each once per call, and no launcher reads them.
 * which 3: WCE_MMSE_COV low-rank path (0 = ranks 1..8 one frame per lane in
 * the LDS-staged form, mmse_lr_lane_staged_kernel, ranks 7 and 8 in its
 * two-workgroups-per-CU build past 65,536 units on a 256-CU device, and
 * ranks 9..16 16 lanes per frame, mmse_lr_quad_kernel, default; 1 = every
 * rank one frame per wave; 2 = the lane kernel's direct form,
 * mmse_lr_lane_kernel; 3 / 4 = the staged form with ranks 7 and 8 in the
 * one- / two-workgroups-per-CU build at any size; 2..4: ranks past 8 one
 * frame per wave).  which 4: WCE_MMSE_FRAME_COV in C semantics (0 = REF
 * ref_fc_kernel, one launch, TEXTBOOK LT_LS and u in one launch, default;
 * 1 = the general factors: the LT_LS pass, the matvec launch and, REF, the w
 * rows, then the solve).  which 5: PS_MMSE with a rank-1
 * covariance, i.e. TEXTBOOK and WCE_MMSE_FRAME_COV (0 = the closed form,
 * mmse_rank1_kernel: Ryy is the identity plus rank 1, so two dot products and
 * a correction sum give H, 16 lanes per (frame, block), default; a call that
 * also asks for LS outputs or equalization runs the LS pass, then this kernel;
 * 1 = the 53 x 53 factorisation, mmse_solve_fc_kernel, one wave per (frame,
 * block), and with LS outputs the fused mmse_solve_ls_kernel; 2 = the closed
 * form with nontemporal loads and stores; 3..19 are launch shapes, cache
 * policies and builds of the closed form, the same route as 0 and read by its launcher
 * alone: 3 = one unit per 16-lane row, the grid covers the batch, so no row
 * loops and nothing is prefetched -- the shape 0 launches too; 4 = the grid
 * capped at 3 workgroups, 48 rows per sweep, so a few hundred frames make
 * many ragged loop trips; 5 = nontemporal stores with default loads; 6 =
 * nontemporal loads with default stores; 7 = the persistent grid, at most
 * wce_debug_rank1_rows_per_sweep rows that loop over the batch with the next
 * unit's loads in flight -- built, tested and measured no faster than 0;
 * 8 / 9 = the default grid in workgroups of 64 / 128 threads; 10 = the
 * default grid with the previous prologue, the shared u waited for before the
 * first tx / rx load); 11 = the general build under the default policy, which
 * reads State::acoef and State::xmask and applies them -- on a State with
 * a = 1 and a full mask (every TEXTBOOK State) 0 runs a build without them;
 * 12 = that build with tx and rx loads alternating and the shared u last,
 * where 0 issues tx, u and rx row by row; 13..19 = mmse_rank1_head_kernel,
 * the headline launch's kernel with preloaded scalar arguments, switched off
 * (13) or in one of its six shapes: wce_debug_rank1_head below).
 * Process-wide; the variants of which 0, 1, 2, 4 give bit-identical results,
 * which 3's kernels sum in different orders and agree to rounding (tests
 * check both); which 5's 0 and 2..19 are bit-identical, 0 and 1 agree to ~1e-11
 * (both within 1e-10 of the long double closed form).  (Round 4 retired ls_flat_kernel -- which 1 = 0, 1 -- and the
 * REF frame tiles -- which 0 = 1.)
 * which 6: the grids of the receive and transmit chain, a test seam rather than
 * an A/B (0 = every launcher its own cap, default; any other value = at most 3
 * workgroups, so that a few dozen frames make every wave take several trips
 * round its frame loop, the last one ragged).  Read by the launchers whose
 * kernels loop over frames: the front end's six builds, wce_front_end_sync,
 * wce_front_end_sync_stf, wce_short_field, wce_demodulate without evm and nerr, wce_soft_demap and _blocks,
 * wce_viterbi_decode, wce_reencode, wce_modulate, wce_channel, wce_transmit,
 * wce_channel_tv, wce_transmit_tv, wce_combine, wce_sync_share,
 * wce_psdu_frame, wce_psdu_deframe.  Each reads it on the host when it launches,
 * so a kernel already queued keeps the grid it was launched with.
 * A frame's outputs depend on its own data alone, so 1 gives the bits of 0.
 * Ignored by wce_demodulate with evm or nerr and by wce_track_demodulate:
 * their kernels run one wave per frame with no loop, on a grid that covers the
 * batch, and a capped grid would leave frames unvisited.  wce_estimate's
 * launchers never read it (which 5 = 4 is their capped grid). */
int wce_debug_set_variant(int which, int value);
/* What a looping chain launcher makes of `blocks` workgroups of work under its
 * own cap and the current which 6: min(blocks, own_cap), or min(blocks, 3) with
 * the knob set.  Needs no device. */
long long wce_debug_chain_grid(long long blocks, long long own_cap);
/* One period of wce_short_field's field at amplitude 1: 16 {re, im} pairs, as the call passes them to its
 * kernel.  Needs no device. */
int wce_debug_short_field_period(double *out);
/* The lags one tile of wce_front_end_sync_stf's kernel covers in its first (STF) and second (LTF) pass: a window
 * takes another tile of the first pass when capture_len - 144 reaches a multiple of *lags_stf, of the second
 * when capture_len - 128 reaches a multiple of *lags_ltf.  Needs no device. */
int wce_debug_sync_stf_tiles(int *lags_stf, int *lags_ltf);
/* (frame, block) units one sweep of mmse_rank1_kernel's persistent grid
 * (which 5 = 7) covers on ctx's device: 16 per workgroup times the workgroups
 * resident at once (4 per CU, the CU count read when ctx was made).  A larger
 * batch makes every 16-lane row loop; a smaller one launches one unit per
 * row.  Negative: an error code. */
int wce_debug_rank1_rows_per_sweep(struct wce_ctx *ctx);
/* Which of the closed form's two kernels one launch runs, as launch_mmse_rank1 decides it from these facts:
 * a shared u, MATLAB split, per-frame noise, a given w, a State with a = 1 and a full mask, the nontemporal
 * build asked for, the value of which 5, the frame and H row strides in complex elements, the frames and the
 * device's XCD labels.  Returns the threads per workgroup of mmse_rank1_head_kernel (64, 128 or 256), whose
 * arguments are preloaded scalars with 32-bit strides, or 0 for mmse_rank1_kernel; *remap (may be NULL) says
 * whether neighbouring groups are placed on one XCD.  which 5 = 13 never runs the head kernel, 14 / 15 / 16 run
 * it in workgroups of 64 / 128 / 256 threads in dispatch order, 17 / 18 / 19 the same with the remap; 0 runs
 * what was adopted.  All bit-identical to 0.  Needs no device. */
int wce_debug_rank1_head(int shared, int split, int noise, int cw, int plain, int nt, int variant, long long fs,
                         long long ws, long long n, int nx, int *remap);
/* The head kernel's placement of `groups` groups of rows over nx XCD labels: out[b] is the group that
 * workgroup b serves, b < the returned grid size nx * ceil(groups / nx); an entry >= groups has no rows.
 * WCE_EINVAL for no groups, no labels or a short buffer. */
int wce_debug_rank1_head_groups(unsigned groups, unsigned nx, unsigned *out, unsigned cap);
/* The kernel families one wce_estimate call launches, in order, as the route
 * planner (csrc/wce_route.h) decides them from these facts: the context's mode,
 * border dot and fusion switches, cm (a constant-modulus operator loaded and
 * enabled), the WCE_MMSE_COV low-rank block row (-1 dense) and rank, the
 * request's semantics, mask and WCE_OUT_LS_F32, and variants 5, 4 and 2.
 * Written to buf as names separated by ';', e.g. "ls;fc_u;mmse_rank1;fc_finish"
 * ("" for a request that launches nothing).  Needs no device and no context.
 * WCE_EINVAL for facts wce_estimate's validation rejects, or a short buffer. */
int wce_debug_route(int mode, int bdot, int fuse, int cm, int lr_k0, int cov_rank, int semantics, unsigned mask,
                    int ls_f32, int r1, int ref_fc, int ref_ls, char *buf, size_t cap);
/* The same for a wce_estimate_noise call: noise != 0 adds the fact that the
 * request carries per-frame ow2 (WCE_EINVAL unless the mode is
 * WCE_MMSE_TEXTBOOK and WCE_EST_PS_MMSE is in the mask; the route is then the
 * closed form whatever bdot and r1 say).  noise == 0: wce_debug_route. */
int wce_debug_route_noise(int mode, int bdot, int fuse, int cm, int lr_k0, int cov_rank, int semantics,
                          unsigned mask, int ls_f32, int r1, int ref_fc, int ref_ls, int noise, char *buf,
                          size_t cap);
/* WCE_MMSE_COV solve form for A/B and accuracy probes: 0 = as the state
 * chose (default), 1 = always the dense Ryy solve, 2 = always the low-rank
 * Gram path (at the state's rank).  ctx is a wce_ctx*. */
int wce_debug_set_cov_path(struct wce_ctx *ctx, int path);
/* The kernel a WCE_MMSE_COV low-rank estimate over `units` (frame, block)
 * units runs under the current variant (e.g. "mmse_lr_lane_staged_kernel<8, 2>");
 * "" for a ctx on the dense path.  For bench labels and the gate's checks. */
const char *wce_debug_lr_kernel(struct wce_ctx *ctx, long long units);
/* A/B switch of the constant-modulus path (wce_ctx_set_modulus); on by default. */
int wce_debug_set_cm(struct wce_ctx *ctx, int on);
/* How many times the compat WiFi_channel_estimation_PS_MMSE built and
 * uploaded its shared state (main.c:148's F / H_EST_LS / ow2): once per
 * distinct (F, H_EST_LS, ow2), not once per call.  0 before the first call. */
unsigned long long wce_debug_compat_state_builds(void);
#ifdef __cplusplus
}
#endif
#endif
