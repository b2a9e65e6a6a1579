// wce_combine.hip -- gfx950 receive diversity: maximal-ratio combining of antenna
// branches (wce_combine) and the antennas' shared timing (wce_sync_share).
// Per packet f and subcarrier k in V = {0..52} without 26, over the live branches a
// in ascending order, v_a = 1 / ow2_a[f] (1 without ow2):
//   g2[k]      = sum_a v_a |h_a[k]|^2,  g = sqrt(g2)
//   rx_c[b][k] = (sum_a v_a conj(h_a[k]) rx_a[b][k]) / g[k],  h_c[k] = g[k]
// include/wce.h has the definition.
//
// Mapping: demod_kernel's.  One wave per packet, lane k = subcarrier k, the frame loop on
// a capped grid.  A is a template parameter: the A weights v_a conj(h_a) and 1 / g stay in
// registers for the packet and the branch loop unrolls over them.  The packet's A h rows
// are issued first, then its blocks in chunks of CB blocks x A branches (about 16 loads of
// 848 B), the next chunk's loads issued before the current one is consumed, so that a wave
// has up to 32 rows in flight.  A branch that is not live is skipped by a branch on a
// wave-uniform mask: its loads are issued (they cost bandwidth on a lost branch only) and
// never read, so nothing of it reaches a sum.  Every term is two spelled-out fmas per
// component onto an accumulator that starts at +0, whatever its place among the live
// branches: the call on the live branches alone runs the same operations on the same
// values.  HBM-bound: A x 13.6 KB read and 13.6 KB written per packet.
#include <hip/hip_runtime.h>
#include "wce_internal.h"
#include "wce_device.h"

namespace wce {

constexpr int CB_WAVES = 4;        // packets per 256-thread workgroup
constexpr int CB_GRID_CAP = 4096;  // demod_kernel's: the waves stride over the packets

// blocks per chunk: about 16 rows per chunk, two chunks in registers
template <int NA> struct CbChunk {
    static constexpr int value = NA == 1 ? NBLK : NA == 2 ? 8 : NA == 3 ? 5 : NA == 4 ? 4 : NA <= 6 ? 3 : 2;
};

template <int NA, int CB>
__device__ __forceinline__ void cb_load(const CombineArgs &a, int64_t base, int b0, uint32_t ko, double2 (&r)[CB][NA])
{
#pragma unroll
    for (int j = 0; j < CB; j++) {
        if (b0 + j < NBLK) {
#pragma unroll
            for (int q = 0; q < NA; q++) r[j][q] = dm_ld_nt(a.rx, q * a.rbs + base + (b0 + j) * a.rks, ko);
        }
    }
}

// packet f (the same in every lane) on one wave.  RX / H: those outputs exist
template <int NA, bool RX, bool H>
__device__ __forceinline__ void combine_frame(const CombineArgs &a, int64_t f, int lane)
{
#pragma clang fp contract(off)
    constexpr int CB = CbChunk<NA>::value;
    const bool act = lane < NSC;
    const int k = act ? lane : 0;
    const uint32_t ko = 16u * (uint32_t)k;
    const bool inv = act && k != WCE_DC;   // k in V

    double2 hv[NA];
#pragma unroll
    for (int q = 0; q < NA; q++) hv[q] = dm_ld_nt(a.h, q * a.hbs + f * a.hs, ko);
    double2 cur[CB][NA];
    const int64_t base = f * a.rfs;
    if constexpr (RX) cb_load<NA, CB>(a, base, 0, ko, cur);

    // the live branches, the same mask in every lane, and their weights
    uint32_t live = 0;
    double2 w[NA];
    double g2 = 0.0;
#pragma unroll
    for (int q = 0; q < NA; q++) {
        const bool bad = inv && !(isfinite(hv[q].x) && isfinite(hv[q].y));
        bool ok = __ballot(bad) == 0;
        double v = 1.0;
        if (a.ow2) {
            const double s2 = a.ow2[q * a.obs + f];
            ok = ok && isfinite(s2) && s2 > 0.0;
            v = 1.0 / s2;
        }
        w[q] = make_double2(v * hv[q].x, v * hv[q].y);
        if (ok) {
            live |= 1u << q;
            g2 = fma(w[q].x, hv[q].x, g2);
            g2 = fma(w[q].y, hv[q].y, g2);
        }
    }
    live = (uint32_t)__builtin_amdgcn_readfirstlane((int)live);
    const double g = sqrt(g2);
    const bool zero = live != 0 && (!inv || g == 0.0);
    const double ig = live == 0 ? __builtin_nan("") : 1.0 / g;   // no live branch: 0 * NaN in every entry

    if constexpr (H) {
        const double2 hc = live == 0 ? make_double2(ig, ig) : make_double2(zero ? 0.0 : g, 0.0);
        if (act) dm_st_nt(a.oh, f * a.ohs, ko, hc);
    }
    if constexpr (RX) {
#pragma unroll
        for (int b0 = 0; b0 < NBLK; b0 += CB) {
            double2 nxt[CB][NA];
            if (b0 + CB < NBLK) cb_load<NA, CB>(a, base, b0 + CB, ko, nxt);
#pragma unroll
            for (int j = 0; j < CB; j++) {
                if (b0 + j < NBLK) {
                    double2 acc = make_double2(0.0, 0.0);
#pragma unroll
                    for (int q = 0; q < NA; q++) {
                        if (live & (1u << q)) {
                            const double2 r = cur[j][q];
                            acc.x = fma(w[q].x, r.x, acc.x);
                            acc.x = fma(w[q].y, r.y, acc.x);
                            acc.y = fma(w[q].x, r.y, acc.y);
                            acc.y = fma(-w[q].y, r.x, acc.y);
                        }
                    }
                    const double2 o = zero ? make_double2(0.0, 0.0) : make_double2(acc.x * ig, acc.y * ig);
                    if (act) dm_st_nt(a.orx, f * a.ofs + (b0 + j) * a.oks, ko, o);
                }
            }
            if (b0 + CB < NBLK) {
#pragma unroll
                for (int j = 0; j < CB; j++) {
#pragma unroll
                    for (int q = 0; q < NA; q++) cur[j][q] = nxt[j][q];
                }
            }
        }
    }
}

template <int NA, bool RX, bool H>
__global__ __launch_bounds__(256) void combine_kernel(CombineArgs a)
{
    const int lane = threadIdx.x & 63;
    // the wave's packet from its first lane: a scalar, and so is every address but the lane's own offset
    const int64_t w = (int64_t)blockIdx.x * CB_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#pragma unroll 1
    for (int64_t f = w; f < a.n; f += (int64_t)gridDim.x * CB_WAVES) combine_frame<NA, RX, H>(a, f, lane);
}

template <int NA>
static void combine_launch(const CombineArgs &a, dim3 g, hipStream_t s)
{
    if (a.orx && a.oh) hipLaunchKernelGGL((combine_kernel<NA, true, true>), g, dim3(256), 0, s, a);
    else if (a.orx) hipLaunchKernelGGL((combine_kernel<NA, true, false>), g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((combine_kernel<NA, false, true>), g, dim3(256), 0, s, a);
}

int launch_combine(const CombineArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    if (a.n > 0x7fffffffll || a.na < 1 || a.na > WCE_COMBINE_MAX_BRANCHES || (!a.orx && !a.oh)) return WCE_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((uint32_t)chain_grid((a.n + CB_WAVES - 1) / CB_WAVES, CB_GRID_CAP));
    switch (a.na) {
    case 1: combine_launch<1>(a, g, s); break;
    case 2: combine_launch<2>(a, g, s); break;
    case 3: combine_launch<3>(a, g, s); break;
    case 4: combine_launch<4>(a, g, s); break;
    case 5: combine_launch<5>(a, g, s); break;
    case 6: combine_launch<6>(a, g, s); break;
    case 7: combine_launch<7>(a, g, s); break;
    default: combine_launch<8>(a, g, s); break;
    }
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

// ---------------------------------------------------------------- shared timing
// one thread per packet: the live branch of the largest metric (the lowest on a tie) gives every branch its start
// and its offset
constexpr int SH_GRID_CAP = 4096;
__global__ __launch_bounds__(256) void sync_share_kernel(SyncShareArgs a)
{
#pragma unroll 1
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.n; p += (int64_t)gridDim.x * 256) {
        int best = -1;
        double bm = 0.0;
        for (int q = 0; q < a.na; q++) {
            const int64_t i = q * a.bs + p;
            const double m = a.metric[i];
            const bool ok = isfinite(m) && (!a.start || a.start[i] >= 0);
            if (ok && (best < 0 || m > bm)) {
                best = q;
                bm = m;
            }
        }
        if (best < 0) continue;
        const int64_t ib = best * a.bs + p;
        const int32_t s = a.start ? a.start[ib] : 0;
        const double c = a.cfo ? a.cfo[ib] : 0.0;
        for (int q = 0; q < a.na; q++) {
            const int64_t i = q * a.bs + p;
            if (a.start) a.start[i] = s;
            if (a.cfo) a.cfo[i] = c;
        }
    }
}

int launch_sync_share(const SyncShareArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    if (a.n > 0x7fffffffll || a.na < 1 || a.na > WCE_COMBINE_MAX_BRANCHES || !a.metric || (!a.start && !a.cfo))
        return WCE_EINVAL;
    const dim3 g((uint32_t)chain_grid((a.n + 255) / 256, SH_GRID_CAP));
    hipLaunchKernelGGL(sync_share_kernel, g, dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce
