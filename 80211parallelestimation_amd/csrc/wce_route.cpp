// wce_route.cpp -- the PS_MMSE launch route of one wce_estimate call (wce_route.h).
// Host-only: no device call, no global read.
#include <cstring>
#include <string>

#include "wce_internal.h"
#include "wce_route.h"
#include "../../include/wce_debug.h"

namespace wce {

int check_route_facts(const RouteFacts &f)
{
    if (f.mode != WCE_MMSE_REF && f.mode != WCE_MMSE_TEXTBOOK && f.mode != WCE_MMSE_COV) return WCE_EINVAL;
    if (f.semantics != WCE_SEM_C && f.semantics != WCE_SEM_MATLAB) return WCE_EINVAL;
    if (f.mask & ~0x7Fu) return WCE_EINVAL;
    if ((f.mask & WCE_MMSE_FRAME_COV) && !(f.mask & WCE_EST_PS_MMSE)) return WCE_EINVAL;
    if (f.mode != WCE_MMSE_COV && (f.lr_k0 >= 0 || f.cm)) return WCE_EINVAL;   // no such context
    // per-frame ow2 is the .m model's: b = ow2 enters the TEXTBOOK closed form only
    if (f.noise && (f.mode != WCE_MMSE_TEXTBOOK || !(f.mask & WCE_EST_PS_MMSE))) return WCE_EINVAL;
    return WCE_OK;
}

Route plan_route(const RouteFacts &f)
{
    Route r;
    const bool ls = (f.mask & (WCE_EST_LS_ALL | WCE_EQUALIZE)) != 0;
    const bool mmse = (f.mask & WCE_EST_PS_MMSE) != 0;
    const bool fc = (f.mask & WCE_MMSE_FRAME_COV) != 0;
    const bool c_sem = f.semantics == WCE_SEM_C;
    const bool split = !c_sem;   // MATLAB: one unit per (frame, block 0..3), averaged after
    // FRAME_COV replaces the model covariance: no low-rank path, no constant-modulus path
    const int lr_k0 = fc ? -1 : f.lr_k0;
    // constant-modulus frames on the shared operator K; not for ranks 1..LRL_RMAX
    // (the lane kernels are already bound by the frames' HBM traffic)
    r.cm = mmse && f.mode == WCE_MMSE_COV && f.cm && c_sem && !fc && (lr_k0 < 0 || f.cov_rank > LRL_RMAX);
    // The covariance the solve sees.  pilots: REF's C_ref = u w^T with a = 0, X = the 4 pilots.
    // rank1: C = cu cw^T (TEXTBOOK's shared c c', REF's pair, or any per-frame C).  bordered:
    // the second bordered row gives H = cu (cw . W) without the apply step.
    const bool pilots = f.mode == WCE_MMSE_REF && f.bdot;
    const bool rank1 = fc || pilots || f.mode == WCE_MMSE_TEXTBOOK;
    const bool bordered = fc || pilots || (f.mode == WCE_MMSE_TEXTBOOK && (f.bdot || f.noise));
    // A bordered rank-1 solve off REF's pilot form has a closed form bound by the frames' HBM
    // traffic: no VALU-bound solve is left for the LS traffic to hide under, so such a request
    // runs the LS pass, then that kernel.  Variant R1 = 1 keeps the factorisation -- except with
    // per-frame noise (TEXTBOOK only, check_route_facts): the factorising kernels read State::bcoef,
    // so that request takes the closed form whatever the border dot and R1 knobs say.
    const bool closed = bordered && !pilots && (f.r1 != 1 || f.noise);
    // Config-5 fusion: the LS family and equalization ride in the solve's epilogue (C semantics)
    const bool fuse = f.fuse && ls && mmse && c_sem && lr_k0 < 0 && !r.cm && !closed;
    r.ls_pass = ls && !fuse;
    if (!mmse) return r;
    // REF + FRAME_COV in C semantics: ref_fc_kernel alone.  A fused LS epilogue after it must be
    // ref_ls_elem_kernel (the default REF_LS form); either variant set sends it down the general path.
    const bool ref_fc = fc && pilots && c_sem && f.ref_fc == 0 && f.ref_ls == 0;
    r.workspace = (fc && !ref_fc) || split || r.cm;
    if (ref_fc) {
        r.prep = FcPrep::RefFc;
        r.solve = fuse ? SolveStep::RefLsElemDone : SolveStep::None;
        return r;
    }
    if (fc) {
        r.fc_lt_ready = !fuse && (f.mask & WCE_EST_LT_LS) && !f.ls_f32;
        if (f.mode == WCE_MMSE_TEXTBOOK && c_sem && !r.fc_lt_ready && f.ref_fc == 0) {
            r.prep = FcPrep::FcU;
        } else {
            r.prep = FcPrep::General;
            r.fc_ref_w = f.mode == WCE_MMSE_REF;
        }
    }
    if (lr_k0 >= 0) {   // H = U s straight from the solve (split: H_b rows, then the block mean)
        r.solve = SolveStep::LowRank;
        r.finish = split ? Finish::AvgBlocks : Finish::None;
        return r;
    }
    r.form = bordered ? SolveForm::Bordered : rank1 ? SolveForm::Rank1Build : SolveForm::Dense;
    if (fuse) r.solve = pilots && f.ref_ls == 0 ? SolveStep::RefLsElem : SolveStep::Fused;
    else if (pilots && !split) r.solve = SolveStep::RefPilots;
    else if (closed) r.solve = f.r1 == 2 ? SolveStep::ClosedNt : SolveStep::Closed;
    else r.solve = SolveStep::Factor;
    if (bordered) r.finish = split ? Finish::FcFinish : Finish::None;
    else r.finish = split ? Finish::MatvecAvg : Finish::Apply;
    return r;
}

int route_names(const Route &r, char *buf, size_t cap)
{
    static const char *const form[] = {"bordered", "rank1_build", "dense"};
    std::string s;
    auto add = [&s](const std::string &name) { s += (s.empty() ? "" : ";") + name; };
    if (r.ls_pass) add("ls");
    switch (r.prep) {
    case FcPrep::None: break;
    case FcPrep::RefFc: add("ref_fc"); break;
    case FcPrep::FcU: add("fc_u"); break;
    case FcPrep::General:
        if (!r.fc_lt_ready) add("ls");
        add("matvec");
        if (r.fc_ref_w) add("ref_w");
        break;
    }
    if (r.cm) add("cm");
    switch (r.solve) {
    case SolveStep::None: break;
    case SolveStep::RefPilots: add("ref_pilots"); break;
    case SolveStep::RefLsElem: add("ref_ls_elem"); break;
    case SolveStep::RefLsElemDone: add("ref_ls_elem_done"); break;
    case SolveStep::Closed: add("mmse_rank1"); break;
    case SolveStep::ClosedNt: add("mmse_rank1_nt"); break;
    case SolveStep::Factor: add(std::string("factor_") + form[(int)r.form]); break;
    case SolveStep::Fused: add(std::string("fused_") + form[(int)r.form]); break;
    case SolveStep::LowRank: add("mmse_lr"); break;
    }
    switch (r.finish) {
    case Finish::None: break;
    case Finish::FcFinish: add("fc_finish"); break;
    case Finish::MatvecAvg: add("matvec_avg"); break;
    case Finish::Apply: add("apply"); break;
    case Finish::AvgBlocks: add("avg_blocks"); break;
    }
    if (s.size() + 1 > cap || !buf) return -1;
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
}

R1HeadShape rank1_head_shape(const R1HeadFacts &f, int nx)
{
    const R1HeadShape old{0, false};
    if (!f.shared || f.split || f.noise || f.cw || !f.plain || f.nt) return old;
    // the kernel's strides and row index are 32-bit values
    if (f.fs < 0 || f.fs > 0xffffffffll || f.ws < 0 || f.ws > 0xffffffffll || f.n > 0x7fffffffll) return old;
    const int v = f.variant == 0 ? R1_VARIANT_ADOPTED : f.variant;
    if (v < R1_VARIANT_HEAD_FIRST || v > R1_VARIANT_HEAD_LAST) return old;   // 1..13: mmse_rank1_kernel's own shapes
    const int k = (v - R1_VARIANT_HEAD_FIRST) % 3;
    return R1HeadShape{64 << k, v >= R1_VARIANT_HEAD_FIRST + 3 && nx == R1_HEAD_XCDS};
}

}  // namespace wce

extern "C" int wce_debug_rank1_head(int shared, int split, int noise, int cw, int plain, int nt, int variant,
                                    long long fs, long long ws, long long n, int nx, int *remap)
{
    const wce::R1HeadFacts f{shared != 0, split != 0, noise != 0, cw != 0, plain != 0, nt != 0, variant, fs, ws, n};
    const wce::R1HeadShape h = wce::rank1_head_shape(f, nx);
    if (remap) *remap = h.remap;
    return h.threads;
}

extern "C" int wce_debug_rank1_head_groups(unsigned groups, unsigned nx, unsigned *out, unsigned cap)
{
    if (!groups || !nx || groups > 0x7fffffffu || nx > 64) return WCE_EINVAL;
    const unsigned per = (groups + nx - 1) / nx, grid = nx * per;
    if (!out || cap < grid) return WCE_EINVAL;
    for (unsigned b = 0; b < grid; b++) out[b] = wce::rank1_head_group(b, nx, per);
    return (int)grid;
}

extern "C" int wce_debug_route(int mode, int bdot, int fuse, int cm, int lr_k0, int cov_rank, int semantics,
                               unsigned mask, int ls_f32, int r1, int ref_fc, int ref_ls, char *buf, size_t cap)
{
    const wce::RouteFacts f{mode, bdot != 0, fuse != 0, cm != 0, lr_k0, cov_rank, semantics, mask, ls_f32 != 0, r1, ref_fc, ref_ls};
    if (wce::check_route_facts(f)) return WCE_EINVAL;
    return wce::route_names(wce::plan_route(f), buf, cap) < 0 ? WCE_EINVAL : WCE_OK;
}

extern "C" int wce_debug_route_noise(int mode, int bdot, int fuse, int cm, int lr_k0, int cov_rank, int semantics,
                                     unsigned mask, int ls_f32, int r1, int ref_fc, int ref_ls, int noise, char *buf,
                                     size_t cap)
{
    wce::RouteFacts f{mode, bdot != 0, fuse != 0, cm != 0, lr_k0, cov_rank, semantics, mask, ls_f32 != 0, r1, ref_fc, ref_ls};
    f.noise = noise != 0;
    if (wce::check_route_facts(f)) return WCE_EINVAL;
    return wce::route_names(wce::plan_route(f), buf, cap) < 0 ? WCE_EINVAL : WCE_OK;
}
