// wce_front.hip -- gfx950 time-domain front end, the GPU
// version of WiFi_blocks_extraction.m:1-11 and WiFi_RX.m:18-30:
//   80-sample OFDM block -> drop the 16-sample cyclic prefix -> 64-point DFT
//   -> circshift(., 26) -> the 53 useful bins, and for the long training field
//   the same on the mean of its two 64-sample copies plus sigma^2.
//
// HBM-bound (1024 B in, 848 B out per block; ~2.3 kflop).  One wave holds 8
// blocks, 8 lanes per block; each lane owns 8 samples.  The 64-point DFT is
// an 8 x 8 Cooley-Tukey: n = 8 n1 + n2, k = k1 + 8 k2,
//   X[k1 + 8 k2] = sum_n2 W8^(n2 k2) W64^(n2 k1) sum_n1 x[8 n1 + n2] W8^(n1 k1)
// stage 1 on lane n2 (8-point DFT in registers), twiddle, an 8x8 transpose
// through LDS (XOR-swizzled, wave-local), stage 2 on lane k1.  Loads are
// 128-B runs per block per instruction; no MFMA (not GEMM-shaped work).
#include <hip/hip_runtime.h>
#include "wce_internal.h"
#include "wce_device.h"
#include "wce_dft64.h"

namespace wce {

// Memory policy per variant, chosen by interleaved A/B on the box
// (tools/ab_front.py, profiles/r01_ab_front.txt): the block kernel stages its
// bins through LDS and stores them as one run per wave, with nontemporal loads
// and stores (5.35 -> 5.98 TB/s); the preamble kernel is fastest with plain
// loads and direct stores (nt: 5.85 -> 5.11 TB/s).
template <bool NT>
__device__ __forceinline__ double2 fe_ld(const double2 *p)
{
    if constexpr (NT) {
        const v2d t = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(p));
        return make_double2(t.x, t.y);
    } else {
        return *p;
    }
}
template <bool NT>
__device__ __forceinline__ void fe_st(double2 *p, double2 v)
{
    if constexpr (NT) {
        v2d t = {v.x, v.y};
        __builtin_nontemporal_store(t, reinterpret_cast<v2d *>(p));
    } else {
        *p = v;
    }
}

constexpr int FE_WAVES = 4;      // waves per 256-thread workgroup
constexpr int FE_UNITS = 8;      // blocks per wave iteration

// ---- carrier frequency offset (the CFO builds) ----
// Sample n (counted from the end of the long training field) is derotated by
// exp(-2 pi i e n), e = the frame's offset in cycles per sample.  A lane's 8
// samples sit 8 apart: one base rotor at its first sample, the step rotor
// exp(-2 pi i 8 e), and products for the other seven -- two sincospi per lane
// and unit, not one per sample.

// x[k] *= r0 s^k.  s^2 and s^4 first: no rotor is more than three products from
// r0.  rot = false (e == 0, every rotor (1, -0)) leaves x as loaded, so that a
// zero offset keeps the plain build's bits down to the sign of a zero.
__device__ __forceinline__ void cfo_derotate(double2 (&x)[8], double2 r0, double2 s, bool rot)
{
    const double2 s2 = cmul(s, s), s4 = cmul(s2, s2);
    const double2 r1 = cmul(r0, s);
    const double2 r[4] = {r0, r1, cmul(r0, s2), cmul(r1, s2)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double2 a = x[k], b = x[k + 4];
        const double2 lo = cmul(a, r[k]), hi = cmul(b, cmul(r[k], s4));
        x[k] = make_double2(rot ? lo.x : a.x, rot ? lo.y : a.y);
        x[k + 4] = make_double2(rot ? hi.x : b.x, rot ? hi.y : b.y);
    }
}

// PRE = false: unit = OFDM block (80 samples, CP 16).  PRE = true: unit =
// one frame's long training field (two 64-sample copies at a.off, a.off + 64).
// The kernels' one body is wce_front_body.h, included into each kernel as it
// stands: the plain builds compile to the code they had before the CFO builds
// existed (as a function shared by both, the body is simplified before it is
// inlined, and the plain builds come out differently scheduled and, in one
// twiddle product, differently rounded).
template <bool PRE>
__global__ __launch_bounds__(256) void front_kernel(FrontArgs a)
{
    constexpr bool CFO = false, AT = false;
#include "wce_front_body.h"
}
// CFO: derotate the samples first (a.cfo, a.n0, a.est).
template <bool PRE>
__global__ __launch_bounds__(256) void front_cfo_kernel(FrontArgs a)
{
    constexpr bool CFO = true, AT = false;
#include "wce_front_body.h"
}
// AT: the frame's units begin a.start[f] samples into its capture window (a.win, a.span); a frame without
// a start, or one that would leave its window, reads nothing of it and comes out NaN.  The CFO build's
// arithmetic with offset 0 where a.cfo is null, so one build serves both.
template <bool PRE>
__global__ __launch_bounds__(256) void front_at_kernel(FrontArgs a)
{
    constexpr bool CFO = true, AT = true;
#include "wce_front_body.h"
}

// a.start != null: the per-frame-start builds; else a.cfo != null: the CFO builds
int launch_front(const FrontArgs &a, bool preamble, void *stream)
{
    if (a.n_units == 0) return 0;
    const uint32_t units_per_wg = FE_WAVES * FE_UNITS;
    // grid-stride beyond ~40 workgroups per CU
    const uint32_t blocks = (uint32_t)chain_grid((a.n_units + units_per_wg - 1) / units_per_wg, 256 * 40);
    const dim3 grid(blocks), blk(256);
    if (a.start && preamble)
        hipLaunchKernelGGL(front_at_kernel<true>, grid, blk, 0, (hipStream_t)stream, a);
    else if (a.start)
        hipLaunchKernelGGL(front_at_kernel<false>, grid, blk, 0, (hipStream_t)stream, a);
    else if (a.cfo && preamble)
        hipLaunchKernelGGL(front_cfo_kernel<true>, grid, blk, 0, (hipStream_t)stream, a);
    else if (a.cfo)
        hipLaunchKernelGGL(front_cfo_kernel<false>, grid, blk, 0, (hipStream_t)stream, a);
    else if (preamble)
        hipLaunchKernelGGL(front_kernel<true>, grid, blk, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(front_kernel<false>, grid, blk, 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce

