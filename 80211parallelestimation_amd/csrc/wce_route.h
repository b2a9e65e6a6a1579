// wce_route.h -- which kernel families one wce_estimate call launches, decided
// in one place.  Host-only and pure: plan_route() maps the facts of a request
// to its launches; wce_api.cpp's estimate_impl gathers the facts (reading each
// A/B variant once), runs the steps in order and fills in the buffers, and
// every launcher of wce_internal.h starts the one family it is named after.
// Choices that depend on the batch size or the device (REF flat / element
// kernel, ls_elem_kernel / ls_kernel, the low-rank forms) stay inside that
// family's launcher.  A new kernel on this dispatch is a new enumerator and
// a new line in plan_route().
#pragma once
#include <cstddef>
#include <cstdint>

namespace wce {

struct RouteFacts {
    int mode;          // the context's WCE_MMSE_REF / TEXTBOOK / COV
    bool bdot;         // rank-1 border dot (wce_debug_set_border_dot)
    bool fuse;         // config-5 fusion switch (wce_debug_set_fusion)
    bool cm;           // a constant-modulus operator is loaded and enabled
    int lr_k0;         // WCE_MMSE_COV low-rank block row, -1 = dense solve
    int cov_rank;
    int semantics;     // WCE_SEM_C / WCE_SEM_MATLAB
    uint32_t mask;     // estimator bits of the request
    bool ls_f32;       // WCE_OUT_LS_F32
    int r1, ref_fc, ref_ls;   // WCE_VARIANT_R1 / REF_FC / REF_LS, read once by the caller
    bool noise;        // wce_estimate_noise: each frame's own ow2 (TEXTBOOK + PS_MMSE; always the closed form)
};

// WCE_MMSE_FRAME_COV: how the per-frame factors u_f (and w_f) come about
enum class FcPrep : uint8_t {
    None,
    RefFc,     // ref_fc_kernel<false>: REF, C semantics, writes H itself (no workspace, no solve)
    FcU,       // ref_fc_kernel<true>: TEXTBOOK, C semantics, LT_LS and u = Mu h in one launch
    General,   // (LT_LS pass unless Route::fc_lt_ready) -> matvec u -> (REF: ref_w)
};

// the form of the 53 x 53 factorisation (launch_mmse_factor, launch_mmse_solve_ls)
enum class SolveForm : uint8_t {
    Bordered,     // rank-1 C = cu cw^T, second bordered row: H (split: the dots) straight from the solve
    Rank1Build,   // Ryy built from the rank-1 cu, W = Ryy^-1 X rx written (apply step follows)
    Dense,        // Ryy from the dense State::C, W written (apply step follows)
};

enum class SolveStep : uint8_t {
    None,            // no PS_MMSE, or ref_fc_kernel wrote H and nothing rides along
    RefPilots,       // REF pilot form (launch_mmse_ref_pilots)
    RefLsElem,       // ref_ls_elem_kernel: REF PS_MMSE + the LS family, one element per thread
    RefLsElemDone,   // the same kernel with the MMSE part skipped (ref_fc_kernel wrote H)
    Closed,          // mmse_rank1_kernel (launch_mmse_rank1)
    ClosedNt,        // its nontemporal build (variant R1 = 2)
    Factor,          // launch_mmse_factor(Route::form)
    Fused,           // launch_mmse_solve_ls(Route::form): solve + LS family + equalization
    LowRank,         // launch_mmse_lr
};

enum class Finish : uint8_t { None, FcFinish, MatvecAvg, Apply, AvgBlocks };

struct Route {
    bool ls_pass = false;        // a separate LS pass runs first
    FcPrep prep = FcPrep::None;
    bool fc_lt_ready = false;    // General: the caller's LT_LS output serves as H_LT
    bool fc_ref_w = false;       // General: REF's w rows (ref_w_kernel); SolveArgs::cw is set
    bool cm = false;             // the constant-modulus launch runs (flags in the workspace's aux array)
    SolveStep solve = SolveStep::None;
    SolveForm form = SolveForm::Dense;   // Factor / Fused only
    Finish finish = Finish::None;
    bool workspace = false;
};

// 0 (WCE_OK), or WCE_EINVAL for facts the API's validation rejects before planning
int check_route_facts(const RouteFacts &f);
Route plan_route(const RouteFacts &f);
// the planned launches as kernel-family names in order, ';'-separated
// (wce_debug_route); returns the length, or -1 if it does not fit in cap
int route_names(const Route &r, char *buf, size_t cap);

// ---- the closed form's two kernels.  To plan_route() both are SolveStep::Closed; launch_mmse_rank1 asks
// rank1_head_shape() which of them one launch runs, and nothing else decides it.
// mmse_rank1_head_kernel (wce_rank1_head.hip) serves the headline's launch alone: its arguments are scalars that
// arrive preloaded in SGPRs, the strides and the batch as 32-bit values.
struct R1HeadFacts {
    bool shared;       // one u for every unit (SolveArgs::cs == 0)
    bool split;        // MATLAB averaging
    bool noise;        // per-frame ow2
    bool cw;           // a given w
    bool plain;        // State::acoef == 1 and a full State::xmask
    bool nt;           // the nontemporal build was asked for (SolveStep::ClosedNt)
    int variant;       // WCE_VARIANT_R1
    int64_t fs, ws, n; // frame stride, H row stride (complex elements), frames
};
struct R1HeadShape {
    int threads;       // 64, 128 or 256 per workgroup; 0: mmse_rank1_kernel runs
    bool remap;        // neighbouring groups share an XCD (rank1_head_group with nx > 1)
};
// WCE_VARIANT_R1 values that name the head kernel's shapes: 13 = never the head kernel, 14 / 15 / 16 = 64 / 128 /
// 256 threads with groups in dispatch order, 17 / 18 / 19 = the same with neighbouring groups on one XCD
constexpr int R1_VARIANT_HEAD_OFF = 13, R1_VARIANT_HEAD_FIRST = 14, R1_VARIANT_HEAD_LAST = 19;
// what variant 0 launches where the head kernel is eligible: 128 threads, neighbours on one XCD -- the shape that
// beat 13 at 65,536 frames and was not slower at 1,048,576 (DESIGN s6, profiles/rank1s_ab_*)
constexpr int R1_VARIANT_ADOPTED = 18;
// nx: XCD labels of the device: R1_HEAD_XCDS on gfx950, the count the kernel's remap is built for; 1 elsewhere: no remap
constexpr int R1_HEAD_XCDS = 8;
R1HeadShape rank1_head_shape(const R1HeadFacts &f, int nx);

// Workgroup b of the head kernel's grid -> the group of rows it serves.  The dispatcher hands workgroup b to XCD
// b % nx; with G groups and per = ceil(G / nx), XCD x gets the groups x per .. x per + per - 1, neighbours in
// memory, so that an H line two groups share is written from one L2.  The grid is nx per workgroups; a result
// >= G has no rows.  A bijection of [0, nx per), so every group is served once: placement changes no bit.
#ifdef __HIPCC__
__host__ __device__
#endif
inline uint32_t rank1_head_group(uint32_t b, uint32_t nx, uint32_t per) { return (b % nx) * per + b / nx; }

}  // namespace wce
