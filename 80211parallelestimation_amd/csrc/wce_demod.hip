// wce_demod.hip -- gfx950 demodulation (wce_demodulate): the last stage of the
// receive chain, behind wce_estimate.  Per frame, from rx and a channel
// estimate h (blended with h_lt over the 15 blocks as WiFi_Equalization.m:4-5):
//   z_b     = sum_{p in pilots} rx_b[p] conj(Hu_b[p] tx_b[p])      (WCE_DEMOD_TRACK)
//   theta_b = arg z_b,  r_b = conj(z_b) / |z_b|
//   e_b[k]  = (rx_b[k] / Hu_b[k]) r_b
// then each e is sliced to its constellation point and Gray label, and the
// frame's EVM and symbol error count are accumulated.  include/wce.h has the
// definition.
//
// Mapping: ls_kernel's.  One wave per frame, lane k = subcarrier k; the 15 rx
// loads (and the tx loads the request needs: the pilot lanes for tracking,
// every data lane for EVM against tx or the error count) are issued before the
// first use.  The blend and the quotient round as ls_store_rv's do (dm_blend, cdiv),
// so an untracked eq has WCE_EQUALIZE's bits.  z_b is summed from
// lane reads of the four pilot lanes in ascending order; lane b then owns block
// b's modulus, rotor and angle (one hypot, two divisions and one atan2 per wave,
// not per block) and the block loop reads r_b back from lane b.  The EVM sums
// are a butterfly over the wave, the error count a ballot per block.  HBM-bound:
// 12.7 KB of rx per frame, as much eq, up to as much tx, 0.8 KB of labels.
#include <hip/hip_runtime.h>
#include "wce_internal.h"
#include "wce_device.h"

namespace wce {

constexpr int DM_WAVES = 4;   // frames per 256-thread workgroup

// the slicer (DmLane, dm_slice) and the addressing helpers (dm_at, dm_ld ...) are in wce_device.h: wce_track.hip
// shares them

// Hu_b = wlt h_lt + wps h.  ls_store_rv writes cadd(cscale(hlt, wlt), cscale(hps, wps)) and the compiler contracts
// it to fma(hlt, wlt, hps wps); here that fma is spelled out with contraction off, so that the code around it
// cannot change the rounding (inside the frame loop the helpers' expression contracted the other way round).
// tests/test_demod_gpu.py holds the two kernels' eq to the same bits
__device__ __forceinline__ double2 dm_blend(double2 hlt, double2 hps, int b)
{
#pragma clang fp contract(off)
    const double wlt = (double)(NBLK - (b + 1)) / NBLK, wps = (double)(b + 1) / NBLK;
    return make_double2(fma(hlt.x, wlt, hps.x * wps), fma(hlt.y, wlt, hps.y * wps));
}

// frame f (the same in every lane, and known to be: the caller reads the wave's index from its first lane) on one wave.  EQ / SYM: those outputs exist; STAT: evm or nerr does; TRACK: WCE_DEMOD_TRACK
template <bool EQ, bool SYM, bool STAT, bool TRACK>
__device__ __forceinline__ void demod_frame(const DemodArgs &a, int64_t f, int lane)
{
    const bool act = lane < NSC;
    const int k = act ? lane : 0;
    const uint32_t ko = 16u * (uint32_t)k;
    const bool pilot = k == WCE_P0 || k == WCE_P1 || k == WCE_P2 || k == WCE_P3;
    const bool data = act && !pilot && k != WCE_DC;
    const bool blend = a.hlt != nullptr;
    const bool ref_tx = (a.flags & WCE_DEMOD_REF_TX) != 0;
    const bool need_tx = a.nerr != nullptr || (a.evm != nullptr && ref_tx);

    // every load of the frame, issued before any use
    const int64_t base = f * a.fs;
    double2 rv[NBLK], tv[NBLK];
#pragma unroll
    for (int b = 0; b < NBLK; b++) rv[b] = dm_ld_nt(a.rx, base + b * a.bs, ko);
    if constexpr (TRACK || STAT) {
#pragma unroll
        for (int b = 0; b < NBLK; b++) tv[b] = make_double2(1, 0);
        if ((TRACK && pilot) || (STAT && need_tx && data)) {
#pragma unroll
            for (int b = 0; b < NBLK; b++) tv[b] = dm_ld_nt(a.tx, base + b * a.bs, ko);
        }
    }
    const double2 hps = dm_ld(a.h, f * a.hs, ko);
    const double2 hlt = blend ? dm_ld(a.hlt, f * a.hs, ko) : make_double2(0, 0);

    DmLane c;
    {
        const int bits = pilot ? 1 : a.mod;
        c.shift = bits >> 1;
        c.m1 = (1 << (bits == 1 ? 1 : c.shift)) - 1;
        c.d = pilot ? a.scale : a.d;
        c.inv2d = 1.0 / (2.0 * c.d);
        c.half = 0.5 * (double)(c.m1 + 1);
        c.top = (double)c.m1;
    }

    // common pilot phase: z_b in every lane, then lane b keeps block b's and forms its rotor and angle
    double2 rot = make_double2(1, 0);
    double th = 0.0;
    if constexpr (TRACK) {
        double2 zs = make_double2(0, 0);
#pragma unroll
        for (int b = 0; b < NBLK; b++) {
            const double2 hu = blend ? dm_blend(hlt, hps, b) : hps;
            const double2 w = cmul(hu, tv[b]);
            const double2 t = make_double2(rv[b].x * w.x + rv[b].y * w.y, rv[b].y * w.x - rv[b].x * w.y);
            const double2 z = cadd(cadd(cadd(readlane_c(t, WCE_P0), readlane_c(t, WCE_P1)), readlane_c(t, WCE_P2)),
                                   readlane_c(t, WCE_P3));
            if (lane == b) zs = z;
        }
        if (!(zs.x == 0.0 && zs.y == 0.0)) {
            const double m = hypot(zs.x, zs.y);
            rot = make_double2(zs.x / m, -zs.y / m);
            th = atan2(zs.y, zs.x);
        }
    }
    if (a.theta && lane < NBLK) a.theta[f * NBLK + lane] = th;

    double num = 0.0, den = 0.0;
    uint32_t nerr = 0;
    bool bad = false;
#pragma unroll
    for (int b = 0; b < NBLK; b++) {
        const double2 hu = blend ? dm_blend(hlt, hps, b) : hps;
        double2 e = k == WCE_DC ? make_double2(0, 0) : cdiv(rv[b], hu);
        if constexpr (TRACK) {
            const double2 r = readlane_c(rot, b);
            if (!(r.x == 1.0 && r.y == 0.0)) e = cmul(e, r);   // r = 1: the quotient's bits
        }
        if constexpr (EQ) {
            if (act) dm_st_nt(a.eq, f * a.eqfs + b * a.eqbs, ko, e);
        }
        if constexpr (SYM || STAT) {
            double2 dec;
            uint32_t s = dm_slice(e, c, dec);
            if (k == WCE_DC) s = 0;
            if constexpr (SYM) {
                if (act) (a.sym + (f * a.symfs + b * a.symbs))[(uint32_t)k] = (uint8_t)s;
            }
            if constexpr (STAT) {
                double2 tdec;
                const uint32_t ts = need_tx ? dm_slice(tv[b], c, tdec) : s;
                const double2 ref = ref_tx ? tv[b] : dec;
                const double dx = e.x - ref.x, dy = e.y - ref.y;
                if (data) {
                    num += dx * dx + dy * dy;
                    den += ref.x * ref.x + ref.y * ref.y;
                }
                bad |= data && s == 0xFFu;
                nerr += (uint32_t)__popcll(__ballot(data && (s == 0xFFu || s != ts)));
            }
        }
    }
    if constexpr (STAT) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            num += __shfl_xor(num, m, 64);
            den += __shfl_xor(den, m, 64);
        }
        const bool poisoned = __ballot(bad) != 0;   // a non-finite data symbol: the frame has no EVM
        if (lane == 0) {
            if (a.evm) a.evm[f] = poisoned ? __builtin_nan("") : sqrt(num / den);
            if (a.nerr) a.nerr[f] = nerr;
        }
    }
}

// The builds without the frame's sums run a capped grid whose waves stride over the frames, as ls_kernel does:
// at 1,048,576 frames eq alone then measured 4% over the LS pass beside it where a grid covering the batch had
// measured 12 to 17%, and the same at 65,536.  The builds with the sums keep one wave per frame and a grid that
// covers the batch: inside the loop, even with one trip, they measured 1.3 to 1.6 times slower
// (profiles/demod_grid_ab.txt).
constexpr int DM_GRID_CAP = 4096;
template <bool EQ, bool SYM, bool STAT, bool TRACK>
__global__ __launch_bounds__(256) void demod_kernel(DemodArgs a)
{
    const int lane = threadIdx.x & 63;
    // the wave's frame from its first lane: a scalar, and so is every address but the lane's own offset
    const int64_t w = (int64_t)blockIdx.x * DM_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if constexpr (STAT) {
        if (w < a.n) demod_frame<EQ, SYM, STAT, TRACK>(a, w, lane);
    } else {
#pragma unroll 1
        for (int64_t f = w; f < a.n; f += (int64_t)gridDim.x * DM_WAVES) demod_frame<EQ, SYM, STAT, TRACK>(a, f, lane);
    }
}

template <bool EQ, bool SYM, bool STAT>
static void demod_launch(const DemodArgs &a, dim3 g, hipStream_t s)
{
    if (a.flags & WCE_DEMOD_TRACK) hipLaunchKernelGGL((demod_kernel<EQ, SYM, STAT, true>), g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((demod_kernel<EQ, SYM, STAT, false>), g, dim3(256), 0, s, a);
}

int launch_demod(const DemodArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    if (a.n > 0x7fffffffll) return WCE_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int which = (a.eq ? 4 : 0) | (a.sym ? 2 : 0) | ((a.evm || a.nerr) ? 1 : 0);
    int64_t blocks = (a.n + DM_WAVES - 1) / DM_WAVES;
    if (!(which & 1)) blocks = chain_grid(blocks, DM_GRID_CAP);   // the builds with the sums have no frame loop
    const dim3 g((uint32_t)blocks);
    switch (which) {
    case 0: demod_launch<false, false, false>(a, g, s); break;   // theta alone
    case 1: demod_launch<false, false, true>(a, g, s); break;
    case 2: demod_launch<false, true, false>(a, g, s); break;
    case 3: demod_launch<false, true, true>(a, g, s); break;
    case 4: demod_launch<true, false, false>(a, g, s); break;
    case 5: demod_launch<true, false, true>(a, g, s); break;
    case 6: demod_launch<true, true, false>(a, g, s); break;
    default: demod_launch<true, true, true>(a, g, s); break;
    }
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce
