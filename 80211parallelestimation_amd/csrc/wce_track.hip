// wce_track.hip -- gfx950 per-block decision-directed channel tracker
// (wce_track_demodulate): wce_demodulate for a channel that moves inside the
// frame.  Per frame, from H_0 = h, for b = 0..14 in order (V = 0..52 without DC):
//   z_b, theta_b, r_b   wce_demodulate's, with Hu_b = H_b
//   e_b[k]   = (rx_b[k] / H_b[k]) r_b, sliced as wce_demodulate slices it
//   x^_b[k]  = tx_b[k] on the pilots (everywhere with WCE_TRACK_KNOWN_TX), else the decided point
//   G_b[k]   = rx_b[k] r_b / x^_b[k]
//   S_b[k]   = mean of G_b[j] over j in V, |j - k| <= beta
//   H_{b+1}  = H_b + mu (S_b - H_b)
// include/wce.h has the definition.
//
// Mapping: demod_frame's.  One wave per frame, lane k = subcarrier k; the 15 rx
// loads (and the tx loads the request needs: the pilot lanes always, every data
// lane for WCE_TRACK_KNOWN_TX, EVM against tx or the error count) are issued
// before the first use.  Unlike demod_frame the block loop is a recurrence: H_b
// needs block b - 1's rotor, decisions and window sums, so the rotor cannot wait
// for a lane of its own after the loop.  z_b is summed from lane reads of the four
// pilot lanes in ascending order and is the same in every lane; the rotor is
// conj(z) rsq(|z|^2), one reciprocal square root (5 VALU) where demod_frame takes a
// hypot and two divisions.  Lane b keeps z_b and the one atan2 per wave runs behind
// the loop, only where theta is wanted.  The window sum reads G from lanes k -+ 1 ..
// beta with ds_bpermute (__shfl: it crosses the 16-lane DPP rows); G is forced to 0
// on lane 26 and on lanes 53..63, so the window needs no clipping at DC or at the
// upper edge and the lanes that wrap below 0 read the zero lanes 60..63; 1 / |N_k| is a
// per-lane constant from a population count.
#include <hip/hip_runtime.h>
#include "wce_internal.h"
#include "wce_device.h"

namespace wce {

constexpr int TK_WAVES = 4;       // frames per 256-thread workgroup

// a b with the fmas spelled out and contraction off: every build of the kernel (with and without the frame's sums,
// with and without a known tx) rounds H, e and the rotor alike, so a subset of the outputs has the full call's bits
__device__ __forceinline__ double2 tk_cmul(double2 a, double2 b)
{
#pragma clang fp contract(off)
    return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x));
}

// frame f (the same in every lane) on one wave.  STAT: evm or nerr exists; PHASE: WCE_TRACK_PHASE;
// KNOWN: WCE_TRACK_KNOWN_TX.  eq, sym, h_blocks and h_last are wave-uniform branches around their stores
template <bool STAT, bool PHASE, bool KNOWN>
__device__ __forceinline__ void track_frame(const TrackArgs &a, int64_t f, int lane)
{
#pragma clang fp contract(off)
    const bool act = lane < NSC;
    const int k = act ? lane : 0;
    const uint32_t ko = 16u * (uint32_t)k;
    const bool pilot = k == WCE_P0 || k == WCE_P1 || k == WCE_P2 || k == WCE_P3;
    const bool inv = act && k != WCE_DC;          // k in V
    const bool data = inv && !pilot;
    const bool ref_tx = (a.flags & WCE_TRACK_REF_TX) != 0;
    const bool need_tx = a.nerr != nullptr || (a.evm != nullptr && ref_tx);
    const bool update = a.mu != 0.0;

    // every load of the frame, issued before any use
    const int64_t base = f * a.fs;
    double2 rv[NBLK], tv[NBLK];
#pragma unroll
    for (int b = 0; b < NBLK; b++) rv[b] = dm_ld_nt(a.rx, base + b * a.bs, ko);
#pragma unroll
    for (int b = 0; b < NBLK; b++) tv[b] = make_double2(1, 0);
    if (pilot || (data && (KNOWN || (STAT && need_tx)))) {
#pragma unroll
        for (int b = 0; b < NBLK; b++) tv[b] = dm_ld_nt(a.tx, base + b * a.bs, ko);
    }
    double2 H = dm_ld(a.h, f * a.hs, ko);

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
    // 1 / |N_k|, N_k = {j in V : |j - k| <= beta}: the window clipped at 0 and 52, DC taken out
    double invn;
    {
        const int lo = max(k - a.beta, 0), hi = min(k + a.beta, NSC - 1);
        const uint64_t win = ((2ull << hi) - 1) & ~((1ull << lo) - 1);
        const uint64_t valid = ((1ull << NSC) - 1) & ~(1ull << WCE_DC);
        invn = 1.0 / (double)max(__popcll(win & valid), 1);
    }

    double2 zs = make_double2(0, 0);
    double num = 0.0, den = 0.0;
    uint32_t nerr = 0;
    bool bad = false;
#pragma unroll
    for (int b = 0; b < NBLK; b++) {
        if (a.hb && act) dm_st_nt(a.hb, f * a.hbfs + b * a.hbbs, ko, H);
        // common pilot phase with Hu_b = H_b: z_b, the same in every lane, and its rotor
        double2 r = make_double2(1, 0);
        if constexpr (PHASE) {
            const double2 w = tk_cmul(H, tv[b]);
            const double2 t = make_double2(fma(rv[b].x, w.x, rv[b].y * w.y), fma(rv[b].y, w.x, -(rv[b].x * w.y)));
            const double2 z = cadd(cadd(cadd(readlane_c(t, WCE_P0), readlane_c(t, WCE_P1)), readlane_c(t, WCE_P2)),
                                   readlane_c(t, WCE_P3));
            if (lane == b) zs = z;
            if (!(z.x == 0.0 && z.y == 0.0)) {
                const double s = rsq_nr(fma(z.x, z.x, z.y * z.y));
                r = make_double2(z.x * s, -z.y * s);
            }
        }
        const bool turn = PHASE && !(r.x == 1.0 && r.y == 0.0);
        double2 e = k == WCE_DC ? make_double2(0, 0) : cdiv(rv[b], H);
        if (turn) e = tk_cmul(e, r);
        if (a.eq && act) dm_st_nt(a.eq, f * a.eqfs + b * a.eqbs, ko, e);
        double2 dec;
        uint32_t s = dm_slice(e, c, dec);
        if (k == WCE_DC) s = 0;
        if (a.sym && act) (a.sym + (f * a.symfs + b * a.symbs))[(uint32_t)k] = (uint8_t)s;
        if constexpr (STAT) {
            double2 tdec;
            const uint32_t ts = need_tx ? dm_slice(tv[b], c, tdec) : s;
            const double2 ref = ref_tx ? tv[b] : dec;
            const double dx = e.x - ref.x, dy = e.y - ref.y;
            if (data) {
                num += fma(dx, dx, dy * dy);
                den += fma(ref.x, ref.x, ref.y * ref.y);
            }
            bad |= data && s == 0xFFu;
            nerr += (uint32_t)__popcll(__ballot(data && (s == 0xFFu || s != ts)));
        }
        if (update) {   // H_{b+1}
            const double2 xh = (KNOWN || pilot) ? tv[b] : dec;
            const double2 q = cdiv(turn ? tk_cmul(rv[b], r) : rv[b], xh);
            const double2 G = inv ? q : make_double2(0, 0);   // lane 26 and lanes 53..63 contribute nothing
            double2 S = G;
#pragma unroll 1
            for (int o = 1; o <= a.beta; o++)
                S = cadd(S, cadd(shfl_c(G, (lane - o) & 63), shfl_c(G, (lane + o) & 63)));
            if (inv) {
                H.x = fma(a.mu, fma(S.x, invn, -H.x), H.x);
                H.y = fma(a.mu, fma(S.y, invn, -H.y), H.y);
            }
        }
    }
    if (a.hl && act) dm_st_nt(a.hl, f * a.hls, ko, H);
    if (a.theta) {
        double th = 0.0;
        if constexpr (PHASE) {
            if (!(zs.x == 0.0 && zs.y == 0.0)) th = atan2(zs.y, zs.x);
        }
        if (lane < NBLK) a.theta[f * NBLK + lane] = th;
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

// One wave per frame and a grid that covers the batch, in every build: a frame holds 30 loaded values in 120
// registers, and in a loop over frames (demod_kernel's capped grid) the compiler hoisted the next frame's loads over
// the block chain and took 221 to 256 registers, one or two waves per SIMD.  Three workgroups per CU, 3 waves per
// SIMD, is what 168 registers allow and what hides the serial chain
template <bool STAT, bool PHASE, bool KNOWN>
__global__ __launch_bounds__(64 * TK_WAVES, 3) void track_kernel(TrackArgs a)
{
    const int lane = threadIdx.x & 63;
    // the wave's frame from its first lane: a scalar, and so is every address but the lane's own offset
    const int64_t w = (int64_t)blockIdx.x * TK_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w < a.n) track_frame<STAT, PHASE, KNOWN>(a, w, lane);
}

template <bool STAT, bool PHASE>
static void track_launch(const TrackArgs &a, dim3 g, hipStream_t s)
{
    if (a.flags & WCE_TRACK_KNOWN_TX)
        hipLaunchKernelGGL((track_kernel<STAT, PHASE, true>), g, dim3(64 * TK_WAVES), 0, s, a);
    else hipLaunchKernelGGL((track_kernel<STAT, PHASE, false>), g, dim3(64 * TK_WAVES), 0, s, a);
}

int launch_track(const TrackArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    if (a.n > 0x7fffffffll || a.beta < 0 || a.beta > 4) return WCE_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool stat = a.evm || a.nerr, phase = (a.flags & WCE_TRACK_PHASE) != 0;
    const dim3 g((uint32_t)((a.n + TK_WAVES - 1) / TK_WAVES));
    if (stat) {
        if (phase) track_launch<true, true>(a, g, s);
        else track_launch<true, false>(a, g, s);
    } else {
        if (phase) track_launch<false, true>(a, g, s);
        else track_launch<false, false>(a, g, s);
    }
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce
