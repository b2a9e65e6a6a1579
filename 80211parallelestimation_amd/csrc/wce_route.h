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

}  // namespace wce
