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
// 16 lanes per (frame, block) unit, 16 units per 256-thread workgroup (8 or 4 in the
// 128- and 64-thread launch shapes: no LDS and no barrier, so the size only decides how
// many waves must retire before a workgroup slot is refilled).  Lane i
// owns subcarriers i, i + 16, i + 32, i + 48 (< 53): every load and store
// instruction moves 256 contiguous bytes of a frame.  The three sums are
// 16-lane DPP row sums of per-lane partials taken in the order m = 0..3, so a
// unit's bits depend on its own data only -- not on the batch, its position in
// it, its neighbours, or the launch shape.  No LDS.  2,544 B of HBM traffic per
// unit (tx block, rx block, H) against ~400 flop: the kernel is bound by memory.
//
// By default the grid covers the batch, one unit per row.  A persistent grid (at
// most R1_WG_PER_CU workgroups per CU, every row looping over units g, g + rows,
// g + 2 rows, ... with the next unit's tx / rx loads issued before the current
// unit's sums) is built and tested but measured no faster: WCE_VARIANT_R1 = 7,
// DESIGN s6.
//
// a = 1 and a full State::xmask (every TEXTBOOK State; the context caches the fact with the State's mode) run a
// build without the mask selects and the scale: X is the tx block as loaded.  REF (a = 0, the four pilots) and
// any other State keep the general build, which WCE_VARIANT_R1 = 11 also runs for the same-binary A/B.  The two
// give the same bits.  Fused products and one reciprocal per denominator (a third fewer VALU instructions
// again, and other bits) were built and measured no faster: the arithmetic below is unchanged (DESIGN s6).
//
// A wave's prologue is one scalar round trip (the kernel arguments, a.n among them),
// the bounds test, and then every vector load of its first unit, one wait chain in front
// of the arithmetic.  The headline's order is tx, the shared u, rx, each row's loads together;
// the other builds alternate tx and rx and load u behind them.
//
// The headline's own launch (shared u, not split, no per-frame noise, the build without mask and scale, default
// policy, strides and batch that fit 32 bits) does not run this kernel by default: rank1_head_shape
// (wce_route.cpp) hands it to mmse_rank1_head_kernel (wce_rank1_head.hip) -- the same loads, arithmetic
// (wce_rank1_body.h) and bits in workgroups of 128 threads whose neighbours share an XCD.  WCE_VARIANT_R1 = 13
// keeps it here, and every other launch runs here whatever the variant.
#include "wce_rank1_body.h"

namespace wce {

// cache policy of the tx / rx loads and the H stores (A/B, WCE_VARIANT_R1 = 2, 5, 6)
constexpr int R1_POL_DEFAULT = 0, R1_POL_NT = 1, R1_POL_NT_STORES = 2, R1_POL_NT_LOADS = 3;
// the default cache policy behind the previous prologue (A/B, WCE_VARIANT_R1 = 10): u and the State scalars
// are loaded and waited for before the first tx / rx load is issued
constexpr int R1_POL_U_FIRST = 4;
// the default cache policy with the loads issued row by row: a unit's four tx loads, the shared u, its four rx
// loads -- where R1_POL_DEFAULT alternates tx and rx and puts u last.  What the shared-u launches of the build
// without mask and scale run (WCE_VARIANT_R1 = 12 keeps them on R1_POL_DEFAULT for the A/B): 0.35 to 0.4 us
// less at 65,536 frames in every same-binary A/B, nothing past the Infinity Cache; moving g and the other
// sums that need tx and u alone ahead of the rx wait as well measured the same as the order alone (DESIGN s6)
constexpr int R1_POL_TX_FIRST = 5;

// One 16-lane row per unit g = frame (or, SPLIT, frame * nblk + block): H = u s
// to row f of a.w, or (SPLIT, MATLAB averaging) s_b to a.dots[g] for
// fc_finish_kernel.  A row takes the units g, g + rows, ... below `units`, rows = gridDim.x blockDim.x / 16.
// Rows of one wave may make different numbers of trips: the DPP sums stay inside a row.
// POL: R1_POL_*.  NOISE (wce_estimate_noise): b = a.ow2[f], the frame's own noise
// variance (TEXTBOOK's b is ow2 itself), one 8-byte load per lane at the row's common
// address, issued with the unit's other loads.  A frame whose ow2 is not positive and
// finite gets s = NaN through the same stores (SPLIT: a NaN dot, so fc_finish_kernel's
// mean is NaN): its row is all NaN, and no address depends on the value.  The build
// without NOISE never reads a.ow2.
// SHARED (a.cs == 0, no a.cw): one u for every unit -- u and conj(u) are loaded once per
// wave, before the loop, and stay in registers (|u|^2 too, except under PF).  Otherwise u
// (and a given w) are the unit's own and are loaded in its trip.
// PF (the looping launch shapes, where r1_prefetch allows): the tx / rx loads of the row's
// next unit are issued before the sums of the current one, under `more` -- no address is
// formed for a unit past the end, so every address lies in a live unit's block.  Two
// units' tx / rx and u are 80 of the 128 registers that 4 waves per SIMD leave: the
// instantiations that hold more (ow2, a unit's own u and w) would spill, and load each
// unit in its own trip whatever the shape.
constexpr bool r1_prefetch(bool noise, bool shared) { return shared && !noise; }
// PLAIN (launch_mmse_rank1's `plain`): State::acoef is 1.0 and State::xmask is full, a fact of the State fixed
// when the context took it.  X is the loaded tx block as it is, a drops out of al and g, and neither
// State::acoef nor State::xmask is read.  Multiplying by 1.0 and selecting under a full mask change no bit:
// the build's results are those of the general one.

template <int POL, bool NOISE, bool SHARED, bool SPLIT, bool PF, bool PLAIN>
__global__ __launch_bounds__(256, R1_WG_PER_CU) void mmse_rank1_kernel(const State *__restrict__ st, SolveArgs a)
{
    static_assert(!PF || r1_prefetch(NOISE, SHARED), "this instantiation has no registers for a second unit");
    constexpr bool NTL = POL == R1_POL_NT || POL == R1_POL_NT_LOADS;
    constexpr bool NTS = POL == R1_POL_NT || POL == R1_POL_NT_STORES;
    constexpr bool LF = POL != R1_POL_U_FIRST;   // loads first
    constexpr bool TXF = POL == R1_POL_TX_FIRST;
    static_assert(!TXF || (SHARED && PLAIN), "the tx-first order is built for the shared-u builds without mask and scale");
    const int i = threadIdx.x & 15;
    const uint32_t rpw = blockDim.x >> 4;   // rows per workgroup: 16, 8 or 4
    int64_t n = a.n;
    if (LF) {
        // The launch shape and every argument an address needs are inputs of an empty asm that hands n on
        // to the bounds test, so they are in SGPRs ahead of the branch: one batch of scalar loads, where
        // the compiler would fetch a.n alone, wait, branch, and only then start on the rest.  Not volatile
        // and inputs only: the pointers keep their address spaces, and the loads through st stay scalar
        auto held = [](int64_t &c, auto v) __attribute__((always_inline)) { asm("" : "+s"(c) : "s"(v)); };
        held(n, st), held(n, a.tx), held(n, a.rx), held(n, a.fs), held(n, a.bs), held(n, a.blk), held(n, a.cu);
        held(n, rpw), held(n, gridDim.x);
        if (SPLIT) held(n, a.nblk), held(n, a.dots);
        else held(n, a.w), held(n, a.ws);
        if (NOISE) held(n, a.ow2);
        if (!SHARED) held(n, a.cs), held(n, a.cw);
    }
    // units < 2^31 (launch_mmse_rank1) and rows <= units + 15: unit and frame indices fit 32 bits
    const uint32_t units = (uint32_t)(SPLIT ? n * a.nblk : n);
    const uint32_t rows = gridDim.x * rpw;
    uint32_t g = blockIdx.x * rpw + (threadIdx.x >> 4);
    if (g >= units) return;   // whole 16-lane rows: the DPP sums stay inside a live row
    const bool cwg = !SHARED && a.cw != nullptr;
    double ac;     // State::acoef, State::xmask and (off NOISE) State::bcoef: scalar loads through st,
    uint64_t xm;   // needed only by the arithmetic
    auto scalars = [&](double &b) __attribute__((always_inline)) {
        ac = PLAIN ? 1.0 : st->acoef;
        xm = PLAIN ? ~0ull : st->xmask;
        if (!NOISE) b = st->bcoef;
    };
    const double2 zero = make_double2(0.0, 0.0);
    // i, hidden from loop-invariant code motion: the per-lane parts of the addresses (a.tx + 16 i, ...) are
    // three VALU instructions to form again and would otherwise each hold a register pair across the loop
    auto lane_again = [](int l) __attribute__((always_inline)) {
        asm volatile("" : "+v"(l));
        return l;
    };
    auto frame_of = [&](uint32_t gu) __attribute__((always_inline)) { return SPLIT ? gu / (uint32_t)a.nblk : gu; };
    // the tx / rx loads of unit gu and (NOISE) its b, all independent: one memory round trip.  Subcarriers
    // 48..52 (m = 3) are loaded by lanes 0..4 alone, at the address of the other three plus an immediate,
    // and are zero in the other lanes
    // TXF: tx whole, then rx (`part` 1 / 2: one side only, so that the shared u can stand between them)
    auto fetch = [&](uint32_t gu, double2(&xl)[4], double2(&rl)[4], double &bc, int part = 0) __attribute__((always_inline)) {
        const uint32_t f = frame_of(gu);
        const int b = SPLIT ? (int)(gu - f * (uint32_t)a.nblk) : 0;
        const int64_t base = (int64_t)f * a.fs + (int64_t)(a.blk + b) * a.bs + lane_again(i);
        if (TXF) {
            if (part != 2) r1_fetch_row(a.tx, base, i, xl);
            if (part != 1) {
                r1_fetch_row(a.rx, base, i, rl);
                if (NOISE) bc = a.ow2[f];
            }
            return;
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            xl[m] = NTL ? ld2_nt(a.tx, base + 16 * m) : ld2(a.tx, base + 16 * m);
            rl[m] = NTL ? ld2_nt(a.rx, base + 16 * m) : ld2(a.rx, base + 16 * m);
        }
        xl[3] = zero;
        rl[3] = zero;
        if (i < NSC - 48) {
            xl[3] = NTL ? ld2_nt(a.tx, base + 48) : ld2(a.tx, base + 48);
            rl[3] = NTL ? ld2_nt(a.rx, base + 48) : ld2(a.rx, base + 48);
        }
        if (NOISE) bc = a.ow2[f];
    };
    // u, w and p of the unit whose u row starts at cb, loaded like tx / rx: zero past subcarrier 52
    auto factors = [&](int64_t cb, double2(&u)[4], double2(&w)[4], double2(&p)[4]) __attribute__((always_inline)) {
        const int64_t ub = cb + i;
        const bool live = i < NSC - 48;
        if (SHARED) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                u[m] = ld2(a.cu, ub + 16 * m);
                w[m] = cconj(u[m]);
            }
            u[3] = zero;
            w[3] = zero;
            if (live) {
                u[3] = ld2(a.cu, ub + 48);
                w[3] = cconj(u[3]);
            }
        } else {
            // a unit's own u (and given w): every load is issued before the first conj(u) -- formed beside
            // its load, each sign flip under the run-time cwg waited for all loads so far, four round trips
#pragma unroll
            for (int m = 0; m < 3; ++m) u[m] = ld2(a.cu, ub + 16 * m);
            u[3] = zero;
            if (live) u[3] = ld2(a.cu, ub + 48);
            if (cwg) {
#pragma unroll
                for (int m = 0; m < 3; ++m) w[m] = ld2(a.cw, ub + 16 * m);
                w[3] = zero;
                if (live) w[3] = ld2(a.cw, ub + 48);
            } else {
#pragma unroll
                for (int m = 0; m < 3; ++m) w[m] = cconj(u[m]);
                w[3] = live ? cconj(u[3]) : zero;
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) p[m] = rank1_p(u[m], w[m], cwg);
    };
    double2 u[4], w[4], p[4];
    double2 xc[4], rc[4], xn[4], rn[4];
    double bc = 0.0, bn;   // NOISE: b is the unit's own, loaded by fetch
    // The scalar loads through st are issued here and waited for at their first use, behind the vector loads
    // (after fetch's asm they would no longer be provably unclobbered, and would become vector loads)
    scalars(bc);
    // LF: the first unit's tx / rx loads (and b) lead and the shared u follows -- every load of the wave is in
    // flight before the first wait of the arithmetic
    if (TXF) {
        // tx, the shared u, rx: loads only, and conj(u) and |u|^2 behind the last of them -- a sign flip beside
        // the lane-masked u load would wait for tx and u inside its branch, ahead of the first rx load
        fetch(g, xc, rc, bc, 1);
        r1_fetch_row(a.cu, i, i, u);
        fetch(g, xc, rc, bc, 2);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            w[m] = m < 3 || i < NSC - 48 ? cconj(u[m]) : zero;
            p[m] = rank1_p(u[m], w[m], cwg);
        }
    } else {
        if (LF) fetch(g, xc, rc, bc);
        if (SHARED) factors(0, u, w, p);
    }
    bn = bc;
    // One trip: unit g from (xc, rc, bc) -- loaded by the caller, or here without PF and LF -- while unit
    // g + rows loads into (xn, rn, bn).  False after the row's last unit; otherwise g has moved on.
    auto trip = [&](double2(&xc)[4], double2(&rc)[4], double &bc, double2(&xn)[4], double2(&rn)[4], double &bn)
                    __attribute__((always_inline)) {
        if (!PF && !LF) fetch(g, xc, rc, bc);
        const uint32_t f = frame_of(g);
        if (!SHARED) factors((int64_t)f * a.cs, u, w, p);
        const bool more = g + rows < units;
        if (PF && more) fetch(g + rows, xn, rn, bn);
        double2 x[4];
#pragma unroll
        for (int m = 0; m < 4; ++m)   // subcarriers off State::xmask do not enter X
            x[m] = PLAIN || ((xm >> ((i + 16 * m) & 63)) & 1ull) ? xc[m] : zero;
        // PF: |u|^2 is formed again in every trip, from a u hidden from loop-invariant code motion.  Held
        // across the trips it is the 8 registers that tip this build into scratch (DESIGN s6); u itself stays
        double2 pl[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double2 um = u[m];
            if (PF) asm volatile("" : "+v"(um.x), "+v"(um.y));
            pl[m] = PF ? rank1_p(um, w[m], cwg) : p[m];
        }
        double2 s = rank1_s<PLAIN>(x, rc, u, w, pl, cwg, ac, bc);
        if (NOISE && !(bc > 0.0 && bc < __builtin_inf())) s = make_double2(__builtin_nan(""), __builtin_nan(""));
        if (SPLIT) {
            if (i == 0) st2(a.dots, g, s);
        } else {
            const int64_t hb = (int64_t)f * a.ws + lane_again(i);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (i + 16 * m < NSC) {
                    const double2 h = r1_mul(u[m], s);
                    if (NTS) st2_nt(a.w, hb + 16 * m, h);
                    else st2(a.w, hb + 16 * m, h);
                }
            }
        }
        g += rows;
        return more;
    };
    if (!PF) {
        while (trip(xc, rc, bc, xn, rn, bn))
            if (LF) fetch(g, xc, rc, bc);
        return;
    }
    // The row's first trip stands apart from the loop, so that every later trip starts in one state, whichever
    // way it was reached: its unit's loads issued a whole trip ago, with only the last trip's stores behind them
    if (!LF) fetch(g, xc, rc, bc);
    bool more = trip(xc, rc, bc, xn, rn, bn);
    while (more) {
        bc = bn;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            xc[m] = xn[m];
            rc[m] = rn[m];
        }
        more = trip(xc, rc, bc, xn, rn, bn);
    }
}

int rank1_rows_per_sweep(int cus) { return (cus > 0 ? cus : 256) * R1_WG_PER_CU * 16; }

// The launch of one call: grid, workgroup size (256, 128 or 64 threads: 16, 8 or 4 rows) and whether rows loop
struct R1Shape {
    dim3 g, b;
    bool pf;   // a looping shape: the prefetching build where r1_prefetch allows
};

template <int POL, bool NOISE, bool SHARED, bool PLAIN>
static void launch_r1_split(const State *st, const SolveArgs &a, const R1Shape &h, hipStream_t s)
{
    if constexpr (r1_prefetch(NOISE, SHARED)) {
        if (h.pf) {
            if (a.split) hipLaunchKernelGGL((mmse_rank1_kernel<POL, NOISE, SHARED, true, true, PLAIN>), h.g, h.b, 0, s, st, a);
            else hipLaunchKernelGGL((mmse_rank1_kernel<POL, NOISE, SHARED, false, true, PLAIN>), h.g, h.b, 0, s, st, a);
            return;
        }
    }
    if (a.split) hipLaunchKernelGGL((mmse_rank1_kernel<POL, NOISE, SHARED, true, false, PLAIN>), h.g, h.b, 0, s, st, a);
    else hipLaunchKernelGGL((mmse_rank1_kernel<POL, NOISE, SHARED, false, false, PLAIN>), h.g, h.b, 0, s, st, a);
}
template <int POL, bool PLAIN = false>
static void launch_r1_pol(const State *st, const SolveArgs &a, const R1Shape &h, hipStream_t s)
{
    const bool shared = a.cs == 0 && !a.cw;
    if constexpr (POL == R1_POL_TX_FIRST) {   // the shared-u builds only (launch_mmse_rank1)
        if (a.ow2) launch_r1_split<POL, true, true, PLAIN>(st, a, h, s);
        else launch_r1_split<POL, false, true, PLAIN>(st, a, h, s);
    } else if (a.ow2) {
        if (shared) launch_r1_split<POL, true, true, PLAIN>(st, a, h, s);
        else launch_r1_split<POL, true, false, PLAIN>(st, a, h, s);
    } else {
        if (shared) launch_r1_split<POL, false, true, PLAIN>(st, a, h, s);
        else launch_r1_split<POL, false, false, PLAIN>(st, a, h, s);
    }
}

void launch_mmse_rank1_head(const State *st, const SolveArgs &a, const R1HeadShape &h, void *stream);

int launch_mmse_rank1(const State *st, const SolveArgs &a, bool nt, int cus, int nx, bool plain, void *stream)
{
    if (!a.cu) return WCE_EINVAL;
    if (a.split ? !a.dots : !a.w) return WCE_EINVAL;
    if (a.n <= 0) return WCE_OK;
    if (a.nblk > 1 && !a.split) return WCE_EINVAL;
    if (a.ow2 && a.cw) return WCE_EINVAL;   // per-frame noise: TEXTBOOK only (check_route_facts), so w = conj(u)
    const int64_t units = a.split ? a.n * a.nblk : a.n;
    if (units > 0x7fffffffll) return WCE_EINVAL;
    // the launch shape and the A/B builds (WCE_VARIANT_R1 = 3..19) are this launcher's alone: to the route
    // planner they are the closed form.  The build without mask and scale exists under the default cache
    // policy only (with a shared u: loads row by row, unless 12): the A/B policies (2, 5, 6, 10) run the
    // general build whatever the State, and 11 runs it under the default policy
    const int shape = variant_value(WCE_VARIANT_R1);
    // mmse_rank1_head_kernel (wce_rank1_head.hip) where rank1_head_shape says so: the headline's launch, under
    // variant 0 if a head shape was adopted and under 14..19; 13 is variant 0 without it
    const R1HeadShape head = rank1_head_shape(
        R1HeadFacts{a.cs == 0 && !a.cw, a.split != 0, a.ow2 != nullptr, a.cw != nullptr, plain, nt, shape, a.fs, a.ws, a.n}, nx);
    if (head.threads) {
        launch_mmse_rank1_head(st, a, head, stream);
        return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
    }
    const int rpw = shape == 8 ? 4 : shape == 9 ? 8 : 16;   // rows per workgroup: the kernel reads blockDim.x
    int64_t wgs = (units + rpw - 1) / rpw;   // one unit per row: the default, and what a batch below one sweep gets anyway
    const bool looping = shape == 4 || shape == 7;
    const int64_t cap = shape == 4 ? 3 : shape == 7 ? rank1_rows_per_sweep(cus) / 16 : wgs;
    if (wgs > cap) wgs = cap;
    const R1Shape h{dim3((unsigned)wgs), dim3(16u * rpw), looping};
    hipStream_t s = (hipStream_t)stream;
    if (nt) launch_r1_pol<R1_POL_NT>(st, a, h, s);
    else if (shape == 5) launch_r1_pol<R1_POL_NT_STORES>(st, a, h, s);
    else if (shape == 6) launch_r1_pol<R1_POL_NT_LOADS>(st, a, h, s);
    else if (shape == 10) launch_r1_pol<R1_POL_U_FIRST>(st, a, h, s);
    else if (!plain || shape == 11) launch_r1_pol<R1_POL_DEFAULT>(st, a, h, s);
    else if (a.cs == 0 && !a.cw && shape != 12) launch_r1_pol<R1_POL_TX_FIRST, true>(st, a, h, s);
    else launch_r1_pol<R1_POL_DEFAULT, true>(st, a, h, s);
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce
