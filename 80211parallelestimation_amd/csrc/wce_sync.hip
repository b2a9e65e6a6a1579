// wce_sync.hip -- gfx950 packet detection and symbol timing (wce_front_end_sync):
// the first stage of the receive chain, in front of wce_front.hip.  Per capture
// window x[0..L) and the clean 64-sample long training symbol ltf:
//   c[d] = sum_{n<64}  x[d+n] conj(ltf[n])            0 <= d <= L - 64
//   E[d] = sum_{n<128} |x[d+n]|^2
//   M[d] = 2 |c[d]| |c[d+64]| / (El E[d])             0 <= d <= L - 128
// and the first d that attains max M.  (L - 63) x 64 complex MACs per frame
// against L x 16 B of HBM: FP64-compute-bound, unlike the rest of the front end.
//
// Mapping (VALU sliding form): one wave per frame.  The window goes through LDS
// in tiles of 576 samples; lane l owns the 8 consecutive lags 8 l .. 8 l + 7 of
// the tile, so one 16-B LDS read feeds 8 complex MACs (32 DFMA) from an 8-sample
// register window, and ltf[n] is wave-uniform (scalar loads, an SGPR operand of
// the DFMA).  c[d + 64] is lane l + 8's c[d]: lanes 0..55 give 448 lags of M per
// tile.  The register window slides by one sample per tap, its slots renamed by
// unrolling 8 taps.  A lane's 8 samples are 128 B apart from its neighbour's; the LDS slot of
// sample i is i + i / 8, a lane stride of 9 x 16 B, which spreads 16 lanes over
// all 64 banks.
//
// E[d] is never a running difference: |x|^2 is summed per aligned block of 8
// (pairwise), and E[8 l + r] = (tail of block l from r) + (blocks l+1 .. l+15) +
// (head of block l + 16 up to r), sums of non-negative terms only, so its error
// is relative to E[d] itself (31 roundings) whatever came earlier in the window.
#include <hip/hip_runtime.h>
#include "wce_internal.h"
#include "wce_device.h"

namespace wce {

constexpr int SY_WAVES = 4;                 // frames per 256-thread workgroup
constexpr int SY_LAGS = 448;                // lags of M per tile (56 lanes x 8)
constexpr int SY_BLKS = 72;                 // 8-sample blocks per tile: 512 lags of c + 63, rounded up
constexpr int SY_SAMPLES = 8 * SY_BLKS;     // 576
constexpr int SY_SLOTS = 9 * SY_BLKS;       // padded LDS slots
constexpr int SY_WGS_PER_CU = 2;            // resident workgroups per CU (222 VGPRs, no scratch; the LDS would admit 3,
                                            // but at 168 VGPRs the build spills 88 and measured 26% slower)
constexpr int SY_GRID_PER_CU = 4;           // workgroups launched per CU: 2, 3 and 4 measured 460, 451 and 443 us at
                                            // 65,536 windows of 488 samples (profiles/sync_ab_65536.txt)

__device__ __forceinline__ bool sy_bad(double2 v) { return !(isfinite(v.x) && isfinite(v.y)); }
__device__ __forceinline__ double sy_abs2(double2 v)
{
#pragma clang fp contract(off)
    return fma(v.x, v.x, v.y * v.y);
}

// one tile's samples for this lane, zero past the window's end: x[D0 + lane + 64 k]
__device__ __forceinline__ void sy_load(const double2 *x, int64_t D0, int64_t L, int lane, double2 (&v)[SY_SAMPLES / 64])
{
#pragma unroll
    for (int k = 0; k < SY_SAMPLES / 64; ++k) {
        const int64_t i = D0 + lane + 64 * k;
        v[k] = make_double2(0.0, 0.0);
        if (i < L) v[k] = x[i];
    }
}

// Capped grid (SY_GRID_PER_CU workgroups per CU, SY_WGS_PER_CU of them resident at once): a wave walks its frames'
// tiles, and the loads of the tile after this one are in flight while this one is computed.
// ltf is an argument of its own, const and restrict: its loads are then known invariant and go to the scalar unit
__global__ __launch_bounds__(256, SY_WGS_PER_CU) void sync_kernel(SyncArgs a, const double2 *__restrict__ ltf)
{
    __shared__ double2 xs[SY_WAVES][SY_SLOTS];
    __shared__ double s8[SY_WAVES][SY_BLKS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double2 *X = xs[w];
    double *S = s8[w];
    const double2 *src = reinterpret_cast<const double2 *>(a.capture);
    const int64_t L = a.len;
    const int64_t fstep = (int64_t)gridDim.x * SY_WAVES;
    int64_t f = (int64_t)blockIdx.x * SY_WAVES + w, D0 = 0;
    double2 nv[SY_SAMPLES / 64];
    if (f < a.n) sy_load(src + f * a.stride, 0, L, lane, nv);

    // El = sum |ltf|^2, the same bits in every lane; a non-finite ltf marks every frame
    const double2 lv = ltf[lane];
    const bool ltf_bad = __ballot(sy_bad(lv)) != 0;
    double El = sy_abs2(lv);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) El += __shfl_xor(El, m, 64);

    // the lane's running first maximum of q = M^2 / 4 (every frame has lag 0, whose q >= 0), and what M needs there
    bool bad = false;
    double bq = -1.0, ba1 = 0.0, ba2 = 0.0, bden = 0.0;
    int32_t bestd = 0;
    while (f < a.n) {
        // the tile's samples, loaded while the tile before was computed
#pragma unroll
        for (int k = 0; k < SY_SAMPLES / 64; ++k) {
            const int i = lane + 64 * k;
            bad |= sy_bad(nv[k]);
            X[i + (i >> 3)] = nv[k];
        }
        // the tile after this one: the frame's next, or the first of the wave's next frame
        int64_t nf = f, nD = D0 + SY_LAGS;
        if (nD > L - 128) { nf = f + fstep; nD = 0; }
        wave_lds_sync();
        if (nf < a.n) sy_load(src + nf * a.stride, nD, L, lane, nv);
        // block sums of |x|^2 (blocks lane and lane + 64)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int blk = lane + 64 * h;
            if (blk < SY_BLKS) {
                double p[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) p[i] = sy_abs2(X[9 * blk + i]);
                S[blk] = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
            }
        }
        // c[8 lane + r] over a sliding 8-sample register window: tap n = 8 it + k meets sample
        // 8 lane + n + r, kept in win[(k + r) & 7]; the sample that enters next replaces the one that left
        double2 acc[8], win[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = make_double2(0.0, 0.0);
#pragma unroll
        for (int i = 0; i < 8; ++i) win[i] = X[9 * lane + i];
#pragma unroll 1
        for (int it = 0; it < 8; ++it) {
            const double2 *nx = X + 9 * (lane + it + 1);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double2 nxt = nx[k];
                const double2 l = ltf[8 * it + k];
#pragma unroll
                for (int r = 0; r < 8; ++r) {   // acc += x conj(l)
                    const double2 v = win[(k + r) & 7];
                    acc[r].x = fma(v.x, l.x, acc[r].x);
                    acc[r].x = fma(v.y, l.y, acc[r].x);
                    acc[r].y = fma(v.y, l.x, acc[r].y);
                    acc[r].y = fma(-v.x, l.y, acc[r].y);
                }
                win[k] = nxt;
            }
        }
        wave_lds_sync();   // S is complete (the wave barrier), and read from here on
        // E[8 lane + r], r < 8 (lanes past 55 give no M: their indices are clamped, their sums unused)
        double E[8];
        {
            double mid = 0.0;
#pragma unroll
            for (int k = 1; k < 16; ++k) mid += S[min(lane + k, SY_BLKS - 1)];
            const int hb = min(lane + 16, SY_BLKS - 1);
            double tail = 0.0, head = 0.0, t[8];
#pragma unroll
            for (int r = 7; r >= 0; --r) { tail += sy_abs2(X[9 * lane + r]); t[r] = tail; }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                E[r] = (t[r] + mid) + head;
                head += sy_abs2(X[9 * hb + r]);
            }
        }
        // the lags are ranked by q = (|c[d]|^2 / den) (|c[d+64]|^2 / den) = M^2 / 4, den = El E[d]: a
        // reciprocal and three products per lag; the square roots and the division of M itself are
        // taken once per frame, at the lag that won.  Lags ascend with r and with the tile
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const double a1 = sy_abs2(acc[r]);
            const double a2 = __shfl_down(a1, 8, 64);   // |c[d + 64]|^2
            const int64_t d = D0 + 8 * lane + r;
            const double den = El * E[r];
            const double ri = rcp_nr(den);
            const double q = den == 0.0 ? 0.0 : (a1 * ri) * (a2 * ri);
            if (lane < SY_LAGS / 8 && d <= L - 128 && q > bq) { bq = q; ba1 = a1; ba2 = a2; bden = den; bestd = (int32_t)d; }
        }
        if (nf != f) {   // the frame's last tile
            // M at the lane's best lag; then the first maximum over the wave: the larger q, then the lower lag
            double M = bden == 0.0 ? 0.0 : 2.0 * sqrt(ba1) * sqrt(ba2) / bden;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const double oq = __shfl_xor(bq, m, 64), oM = __shfl_xor(M, m, 64);
                const int32_t od = __shfl_xor(bestd, m, 64);
                if (oq > bq || (oq == bq && od < bestd)) { bq = oq; M = oM; bestd = od; }
            }
            const bool poisoned = ltf_bad || __ballot(bad) != 0;
            if (lane == 0) {
                const int32_t s = bestd - a.backoff;
                a.start[f] = (!poisoned && M >= a.threshold && s >= 0) ? s : -1;
                if (a.metric) a.metric[f] = poisoned ? __builtin_nan("") : M;
            }
            bad = false;
            bq = -1.0; ba1 = ba2 = bden = 0.0;
            bestd = 0;
        }
        wave_lds_sync();   // the next tile overwrites X and S
        f = nf;
        D0 = nD;
    }
}

int launch_sync(const SyncArgs &a, int cus, void *stream)
{
    if (a.n == 0) return 0;
    const int64_t blocks = chain_grid((a.n + SY_WAVES - 1) / SY_WAVES, SY_GRID_PER_CU * (int64_t)cus);
    hipLaunchKernelGGL(sync_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, a,
                       reinterpret_cast<const double2 *>(a.ltf));
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce
