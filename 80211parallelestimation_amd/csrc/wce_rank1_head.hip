// wce_rank1_head.hip -- mmse_rank1_head_kernel: the closed-form rank-1 PS_MMSE solve (wce_rank1.hip derives it)
// for the one launch the headline makes: a shared u, no MATLAB split, no per-frame noise, a State with a = 1 and a
// full mask, the default cache policy, one unit per 16-lane row.  Same loads in the same order (tx, the shared u,
// rx, row by row), same arithmetic (wce_rank1_body.h), same stores: a unit's bits are mmse_rank1_kernel's.
//
// What differs is the part of a wave's life before its first load.  The arguments are 13 dwords of scalars -- no
// struct, the block offset folded into tx and rx by the host, strides and batch as 32-bit values -- and this file
// alone is compiled with -mllvm -amdgpu-kernarg-preload-count (csrc/Makefile): they arrive in SGPRs with the wave,
// and the prologue has no scalar load and no wait in front of the address arithmetic.  The workgroup size is a
// template constant, so nothing is read from the dispatch packet either.  State::bcoef stays a scalar load through
// st, needed by the arithmetic only and waited for behind the vector loads.
//
// XCD8: the dispatcher deals workgroups round-robin over the 8 XCDs, whose L2s are not coherent with each other; H
// rows are 848 B, so groups of 4 or 8 rows end inside a 128-B line that the next group also writes.
// rank1_head_group (wce_route.h) renumbers the workgroups so that neighbouring groups run on one XCD.
// Which launches run this kernel, and in which shape, is rank1_head_shape's decision (wce_route.cpp).
#include "wce_rank1_body.h"

namespace wce {

template <int T, bool XCD8>
__global__ __launch_bounds__(T, R1_WG_PER_CU) void mmse_rank1_head_kernel(const State *st, const double *tx,
                                                                          const double *rx, const double *cu,
                                                                          double *H, uint32_t n, uint32_t fs,
                                                                          uint32_t ws)
{
    static_assert(T == 64 || T == 128 || T == 256, "whole waves, at most mmse_rank1_kernel's workgroup");
    constexpr uint32_t RPW = T / 16;   // rows per workgroup
    const int i = threadIdx.x & 15;
    constexpr uint32_t NX = R1_HEAD_XCDS;
    uint32_t wg = blockIdx.x;
    if (XCD8) {
        const uint32_t groups = (n + RPW - 1) / RPW;   // n < 2^31 (rank1_head_shape)
        wg = rank1_head_group(wg, NX, (groups + NX - 1) / NX);
        if (wg >= groups) return;   // the grid is rounded up to NX per: at most NX - 1 workgroups without rows
    }
    // wg < groups + NX and 16 groups < 2^31 + 16: the row index fits 32 bits
    const uint32_t g = wg * RPW + (threadIdx.x >> 4);
    if (g >= n) return;   // whole 16-lane rows: the DPP sums stay inside a live row
    const double bc = st->bcoef;   // a scalar load, issued here and waited for at its first use
    double2 x[4], r[4], u[4], w[4], p[4];
    const int64_t base = (int64_t)((uint64_t)g * fs) + i;
    r1_fetch_row(tx, base, i, x);
    r1_fetch_row(cu, i, i, u);
    r1_fetch_row(rx, base, i, r);
    // conj(u) and |u|^2 behind the last load: a sign flip beside the lane-masked u load would wait inside its branch
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        w[m] = m < 3 || i < NSC - 48 ? cconj(u[m]) : make_double2(0.0, 0.0);
        p[m] = rank1_p(u[m], w[m], false);
    }
    const double2 s = rank1_s<true>(x, r, u, w, p, false, 1.0, bc);
    const int64_t hb = (int64_t)((uint64_t)g * ws) + i;
#pragma unroll
    for (int m = 0; m < 4; ++m)
        if (i + 16 * m < NSC) st2(H, hb + 16 * m, r1_mul(u[m], s));
}

template <int T>
static void launch_head(const State *st, const SolveArgs &a, bool remap, hipStream_t s)
{
    constexpr int64_t RPW = T / 16;
    const int64_t groups = (a.n + RPW - 1) / RPW;
    const double *tx = a.tx + 2 * ((int64_t)a.blk * a.bs), *rx = a.rx + 2 * ((int64_t)a.blk * a.bs);
    const uint32_t n = (uint32_t)a.n, fs = (uint32_t)a.fs, ws = (uint32_t)a.ws;
    if (remap) {
        const int64_t per = (groups + R1_HEAD_XCDS - 1) / R1_HEAD_XCDS;
        hipLaunchKernelGGL((mmse_rank1_head_kernel<T, true>), dim3((unsigned)(R1_HEAD_XCDS * per)), dim3(T), 0, s, st, tx, rx,
                           a.cu, a.w, n, fs, ws);
    } else {
        hipLaunchKernelGGL((mmse_rank1_head_kernel<T, false>), dim3((unsigned)groups), dim3(T), 0, s, st, tx, rx,
                           a.cu, a.w, n, fs, ws);
    }
}

// h: rank1_head_shape's answer for this launch (threads != 0)
void launch_mmse_rank1_head(const State *st, const SolveArgs &a, const R1HeadShape &h, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (h.threads == 64) launch_head<64>(st, a, h.remap, s);
    else if (h.threads == 128) launch_head<128>(st, a, h.remap, s);
    else launch_head<256>(st, a, h.remap, s);
}

}  // namespace wce
