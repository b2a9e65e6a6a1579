// wce_rank1_body.h -- the arithmetic of the closed-form rank-1 PS_MMSE solve and the row-by-row fetch, shared by
// mmse_rank1_kernel (wce_rank1.hip) and mmse_rank1_head_kernel (wce_rank1_head.hip): one source, so the two
// kernels round alike and a unit's bits do not depend on which of them ran.  wce_rank1.hip's header comment
// derives the form.
#pragma once
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

// p_k = w_k u_k, the factor of g's terms that the covariance alone decides: |u_k|^2 for
// w = conj(u).  With a shared u it stays in registers from unit to unit.
__device__ __forceinline__ double2 rank1_p(double2 u, double2 w, bool cwg)
{
#pragma clang fp contract(off)
    return cwg ? r1_mul(w, u) : make_double2(u.x * u.x + u.y * u.y, 0.0);
}

// s of one unit.  Lane i of the unit's 16-lane row holds subcarriers i + 16 m
// in x, r (rx), u, w and p (rank1_p); entries past subcarrier 52 (and x off
// State::xmask) are zero.  cwg: w was given (SolveArgs::cw) -- g may be complex;
// otherwise w = conj(u) and g = a sum |x|^2 |u|^2 is real.  Every lane returns the same bits.
template <bool PLAIN>
__device__ __forceinline__ double2 rank1_s(const double2 (&x)[4], const double2 (&r)[4], const double2 (&u)[4],
                                           const double2 (&w)[4], const double2 (&p)[4], bool cwg, double ac,
                                           double bc)
{
#pragma clang fp contract(off)
    double2 g = make_double2(0.0, 0.0), q = g;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const double x2 = x[m].x * x[m].x + x[m].y * x[m].y;
        const double ax2 = PLAIN ? x2 : ac * x2;
        const double2 gk = make_double2(ax2 * p[m].x, ax2 * p[m].y);    // be_k al_k = a |x_k|^2 w_k u_k
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
        const double2 at = r1_mul(PLAIN ? xu : make_double2(ac * xu.x, ac * xu.y), t);   // al_k t
        const double2 rho = make_double2(r[m].x - at.x, r[m].y - at.y);
        const double ti = 2.0 * x[m].y;                                      // x - conj x = (0, 2 Im x)
        const double2 ck = r1_mul(w[m], make_double2(-(ti * rho.y), ti * rho.x));
        c = m ? r1_add(c, ck) : ck;
    }
    c = row16_sum(c);
    return make_double2(t.x + c.x / bc, t.y + c.y / bc);
}

// One 53-entry row (a unit's tx or rx block, or u) as lane i of its 16-lane row loads it: subcarriers i, i + 16
// and i + 32 from every lane, 48..52 from lanes 0..4 alone, at the address of the other three plus an immediate,
// and zero in the other lanes.  Loads only, so that rows fetched one after another are one memory round trip.
__device__ __forceinline__ void r1_fetch_row(const double *p, int64_t base, int i, double2 (&v)[4])
{
#pragma unroll
    for (int m = 0; m < 3; ++m) v[m] = ld2(p, base + 16 * m);
    v[3] = make_double2(0.0, 0.0);
    if (i < NSC - 48) v[3] = ld2(p, base + 48);
}

// Workgroups resident per CU, and so per CU of the persistent grid: 4 waves per SIMD at up to 128
// VGPRs, the occupancy every instantiation is held to (DESIGN s6 lists each one's registers).
constexpr int R1_WG_PER_CU = 4;

}  // namespace wce
