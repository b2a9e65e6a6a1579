// wce_rank1.hip -- PS_MMSE with a rank-1 covariance in closed form:
// mmse_rank1_kernel, the headline (TEXTBOOK) and WCE_MMSE_FRAME_COV solve.
//
// C = u w^T (TEXTBOOK: w = conj(u), u = State::cvec or the frame's own u_f), so
//     Ryy = a X C X^H + b I = al be^T + b I,   al = a x o u,  be = w o conj(x),
// is the identity plus rank 1 and Sherman-Morrison inverts it:
//     Ryy^-1 rx = (rx - al t) / b,   t = q / (b + g),  g = be^T al,  q = be^T rx.
// The read-out s = (w o x)^T Ryy^-1 rx is split as
//     s = t + (1 / b) sum_k w_k (x_k - conj x_k) (rx_k - al_k t)
// because (w o conj x)^T Ryy^-1 rx = (q - g t) / b = t exactly: for real
// symbols every x_k - conj x_k is 0 and s = t without cancellation; for complex
// symbols the sum is the low-rank path's correction term (DESIGN "Model
// covariances of any rank").  The naive (rho^T rx - (rho^T al) t) / b cancels
// 6 digits at cond(Ryy) = 4e6 (9.5e-10 norm-relative on BPSK frames against
// 5e-16 for this form; tests/test_rank1_model.py).  H = u s.
//
// A given w (SolveArgs::cw, rank1_s's cwg) comes from REF with the border dot
// off under WCE_MMSE_FRAME_COV only, where a = 0 and so g = 0
// (tests/test_rank1_routes_gpu.py).  g != 0 with a given w has no caller today:
// that arithmetic is pinned by the CPU model alone (tests/test_rank1_model.py
// against the mpmath fixture tests/golden/rank1_cw_mp.npz).
//
// 16 lanes per (frame, block) unit, 16 units per 256-thread workgroup.  Lane i
// owns subcarriers i, i + 16, i + 32, i + 48 (< 53): every load and store
// instruction moves 256 contiguous bytes of a frame.  The three sums are
// 16-lane DPP row sums of per-lane partials taken in the order m = 0..3, so a
// unit's bits depend on its own data only -- not on the batch, its position in
// it, or its neighbours.  No LDS.  2,544 B of HBM traffic per unit (tx block,
// rx block, H) against ~400 flop: the kernel is bound by HBM.
#include "wce_internal.h"
#include "wce_device.h"

namespace wce {

// Plain IEEE products, sums and quotients, never contracted into FMAs: the
// numpy transcription in tests/test_rank1_model.py rounds alike.
__device__ __forceinline__ double2 r1_mul(double2 a, double2 b)
{
#pragma clang fp contract(off)
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 r1_add(double2 a, double2 b)
{
#pragma clang fp contract(off)
    return make_double2(a.x + b.x, a.y + b.y);
}

// s of one unit.  Lane i of the unit's 16-lane row holds subcarriers i + 16 m
// in x, r (rx), u, w; entries past subcarrier 52 (and x off State::xmask) are
// zero.  cwg: w was given (SolveArgs::cw) -- g may be complex; otherwise
// w = conj(u) and g = a sum |x|^2 |u|^2 is real.  Every lane returns the same bits.
__device__ __forceinline__ double2 rank1_s(const double2 (&x)[4], const double2 (&r)[4], const double2 (&u)[4],
                                           const double2 (&w)[4], bool cwg, double ac, double bc)
{
#pragma clang fp contract(off)
    double2 g = make_double2(0.0, 0.0), q = g;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const double2 p = cwg ? r1_mul(w[m], u[m]) : make_double2(u[m].x * u[m].x + u[m].y * u[m].y, 0.0);
        const double ax2 = ac * (x[m].x * x[m].x + x[m].y * x[m].y);
        const double2 gk = make_double2(ax2 * p.x, ax2 * p.y);          // be_k al_k = a |x_k|^2 w_k u_k
        const double2 qk = r1_mul(r1_mul(w[m], cconj(x[m])), r[m]);     // be_k rx_k
        g = m ? r1_add(g, gk) : gk;
        q = m ? r1_add(q, qk) : qk;
    }
    g = row16_sum(g);
    q = row16_sum(q);
    const double2 d = make_double2(bc + g.x, g.y);
    double2 t;
    if (cwg) {
        const double den = d.x * d.x + d.y * d.y;
        t = make_double2((q.x * d.x + q.y * d.y) / den, (q.y * d.x - q.x * d.y) / den);
    } else {
        t = make_double2(q.x / d.x, q.y / d.x);
    }
    double2 c = make_double2(0.0, 0.0);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const double2 xu = r1_mul(x[m], u[m]);
        const double2 at = r1_mul(make_double2(ac * xu.x, ac * xu.y), t);   // al_k t
        const double2 rho = make_double2(r[m].x - at.x, r[m].y - at.y);
        const double ti = 2.0 * x[m].y;                                      // x - conj x = (0, 2 Im x)
        const double2 ck = r1_mul(w[m], make_double2(-(ti * rho.y), ti * rho.x));
        c = m ? r1_add(c, ck) : ck;
    }
    c = row16_sum(c);
    return make_double2(t.x + c.x / bc, t.y + c.y / bc);
}

// One 16-lane row per unit g = frame (or, split, frame * nblk + block): H = u s
// to row f of a.w, or (split, MATLAB averaging) s_b to a.dots[g] for
// fc_finish_kernel.  NT: nontemporal tx / rx loads and H stores (A/B).
// NOISE (wce_estimate_noise): b = a.ow2[f], the frame's own noise variance (TEXTBOOK's b is
// ow2 itself), one 8-byte load per lane at the row's common address, issued with the other
// 16.  A frame whose ow2 is not positive and finite gets s = NaN through the same stores
// (split: a NaN dot, so fc_finish_kernel's mean is NaN): its row is all NaN, and no address
// depends on the value.  The build without NOISE never reads a.ow2.
template <bool NT, bool NOISE>
__global__ __launch_bounds__(256) void mmse_rank1_kernel(const State *__restrict__ st, SolveArgs a)
{
    const int i = threadIdx.x & 15;
    const int64_t units = a.split ? a.n * a.nblk : a.n;
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (g >= units) return;   // whole 16-lane rows: the DPP sums stay inside a live row
    const int64_t f = a.split ? g / a.nblk : g;
    const int b = a.split ? (int)(g - f * a.nblk) : 0;
    const int64_t base = f * a.fs + (int64_t)(a.blk + b) * a.bs;
    const int64_t cb = f * a.cs;
    const bool cwg = a.cw != nullptr;
    const double ac = st->acoef, bc = NOISE ? a.ow2[f] : st->bcoef;
    const uint64_t xm = st->xmask;
    const double2 zero = make_double2(0.0, 0.0);
    double2 x[4], r[4], u[4], w[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {   // the 16 loads are independent: one memory round trip
        const int k = i + 16 * m, kc = k < NSC ? k : NSC - 1;
        const bool live = k < NSC;
        const double2 xl = NT ? ld2_nt(a.tx, base + kc) : ld2(a.tx, base + kc);
        const double2 rl = NT ? ld2_nt(a.rx, base + kc) : ld2(a.rx, base + kc);
        const double2 ul = ld2(a.cu, cb + kc);
        const double2 wl = cwg ? ld2(a.cw, cb + kc) : cconj(ul);
        // each array element is written once (a select on an element already stored keeps the array in scratch)
        x[m] = live && ((xm >> (k & 63)) & 1ull) ? xl : zero;
        r[m] = live ? rl : zero;
        u[m] = live ? ul : zero;
        w[m] = live ? wl : zero;
    }
    double2 s = rank1_s(x, r, u, w, cwg, ac, bc);
    if (NOISE && !(bc > 0.0 && bc < __builtin_inf())) s = make_double2(__builtin_nan(""), __builtin_nan(""));
    if (a.split) {
        if (i == 0) st2(a.dots, g, s);
        return;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int k = i + 16 * m;
        if (k < NSC) {
            const double2 h = r1_mul(u[m], s);
            if (NT) st2_nt(a.w, f * a.ws + k, h);
            else st2(a.w, f * a.ws + k, h);
        }
    }
}

int launch_mmse_rank1(const State *st, const SolveArgs &a, bool nt, void *stream)
{
    if (!a.cu) return WCE_EINVAL;
    if (a.split ? !a.dots : !a.w) return WCE_EINVAL;
    if (a.n <= 0) return WCE_OK;
    if (a.nblk > 1 && !a.split) return WCE_EINVAL;
    const int64_t units = a.split ? a.n * a.nblk : a.n;
    if (units > 0x7fffffffll) return WCE_EINVAL;
    const dim3 g((unsigned)((units + 15) / 16)), b(256);
    hipStream_t s = (hipStream_t)stream;
    if (a.ow2) {   // per-frame noise: TEXTBOOK only (check_route_facts), so w = conj(u)
        if (a.cw) return WCE_EINVAL;
        if (nt) hipLaunchKernelGGL((mmse_rank1_kernel<true, true>), g, b, 0, s, st, a);
        else hipLaunchKernelGGL((mmse_rank1_kernel<false, true>), g, b, 0, s, st, a);
    } else if (nt) {
        hipLaunchKernelGGL((mmse_rank1_kernel<true, false>), g, b, 0, s, st, a);
    } else {
        hipLaunchKernelGGL((mmse_rank1_kernel<false, false>), g, b, 0, s, st, a);
    }
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce
