// wce_sync_stf.hip -- gfx950 detection on the short training field, coarse carrier offset, symbol timing on
// the derotated long field and the unwrapped fine offset (wce_front_end_sync_stf), and the transmitter's short
// field (wce_short_field).  Per capture window x[0..L):
//   P[d] = sum_{n<128} x[d+n+16] conj(x[d+n]),  A[d] = sum_{n<128} |x[d+n]|^2,  B[d] = A[d+16]   0 <= d <= L - 144
//   d_s the first maximum of |P|^2;  Ms = |P|^2 / (A B) there;  e_c = arg P[d_s] / (32 pi)
//   wce_sync.hip's c, E, M on x[i] exp(-2 pi i e_c i), first maximum d*, s = d* - backoff
//   e_f = arg sum_{n<64} x[s+64+n] conj(x[s+n]) / (128 pi);  cfo = e_f + rint(64 (e_c - e_f)) / 64
//
// Mapping: wce_sync.hip's, one wave per frame, the window through LDS in tiles of 576 samples, lane l on the 8
// lags 8 l .. 8 l + 7 of the tile.  e_c is known only once the whole window has been seen, so a frame takes
// two passes of tiles, both prefetched one tile ahead from global memory (the second visit reads what the
// first left in the caches; the window never stays in LDS).
//   Pass 1 (432 lags a tile, lanes 0..53): q[i] = x[i+16] conj(x[i]) is one complex MAC per sample.  Like E[d]
//   in wce_sync.hip, P and A are never running differences: q and |x|^2 are summed per aligned block of 8
//   (pairwise), and a lag's sum is (tail of block l from r) + (blocks l+1 .. l+15) + (head of block l+16 up to
//   r).  B[8 l + r] is lane l + 2's A.  The lags are ranked by |P|^2, un-normalised.
//   Pass 2 (448 lags a tile, lanes 0..55): the samples are derotated while they are staged -- |c| is the
//   modulus the rotated template would give, and ltf stays the wave-uniform scalar operand of the inner loop.
//   A lane's 9 samples of a tile sit 64 apart: one exact-phase rotor at its first, the step exp(-2 pi i 64 e_c)
//   and its 2nd, 4th and 8th power; no rotor is more than three products from an exact one.
#include <hip/hip_runtime.h>
#include <math.h>
#include "wce_internal.h"
#include "wce_device.h"

namespace wce {

constexpr int SS_WAVES = 4;                 // frames per 256-thread workgroup
constexpr int SS_BLKS = 72;                 // 8-sample blocks per tile
constexpr int SS_SAMPLES = 8 * SS_BLKS;     // 576
constexpr int SS_BLKS_PAD = 64 + 18;        // blocks the LDS arrays hold: lane 63 reads up to block 63 + 18 unclamped (one
                                            // address register, immediate offsets); what lies past the tile is stale and
                                            // only reaches lanes whose lags are masked out
constexpr int SS_SLOTS_PAD = 9 * SS_BLKS_PAD;   // padded LDS slots: sample i at i + i / 8
constexpr int SS_LAGS_STF = 432;            // pass 1: 54 lanes x 8; lag d reads up to sample d + 143, block l + 18
constexpr int SS_LAGS_LTF = 448;            // pass 2: 56 lanes x 8, as wce_sync.hip
constexpr int SS_WGS_PER_CU = 2;            // resident workgroups per CU, as wce_sync.hip (the inner loop is its)
constexpr int SS_GRID_PER_CU = 4;           // workgroups launched per CU

static_assert(SS_LAGS_STF + 143 <= SS_SAMPLES && SS_LAGS_LTF + 127 <= SS_SAMPLES, "a tile's lags read inside it");

__device__ __forceinline__ bool ss_bad(double2 v) { return !(isfinite(v.x) && isfinite(v.y)); }
__device__ __forceinline__ double ss_abs2(double2 v)
{
#pragma clang fp contract(off)
    return fma(v.x, v.x, v.y * v.y);
}
// b conj(a)
__device__ __forceinline__ double2 ss_q(double2 b, double2 a)
{
#pragma clang fp contract(off)
    return make_double2(fma(b.x, a.x, b.y * a.y), fma(b.y, a.x, -(b.x * a.y)));
}
__device__ __forceinline__ double2 ss_cmul(double2 a, double2 b)
{
#pragma clang fp contract(off)
    return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.y, b.x, a.x * b.y));
}
// exp(-2 pi i e n), the phase reduced exactly before sincospi sees it (wce_dft64.h's cfo_rotor)
__device__ __forceinline__ double2 ss_rotor(double e, double n)
{
#pragma clang fp contract(off)
    const double hi = e * n, lo = fma(e, n, -hi);
    const double t = (hi - rint(hi)) + lo;
    double s, c;
    sincospi(-2.0 * t, &s, &c);
    return make_double2(c, s);
}

// one tile's samples for this lane, zero past the window's end: x[D0 + lane + 64 k]
__device__ __forceinline__ void ss_load(const double2 *x, int64_t D0, int64_t L, int lane, double2 (&v)[SS_SAMPLES / 64])
{
#pragma unroll
    for (int k = 0; k < SS_SAMPLES / 64; ++k) {
        const int64_t i = D0 + lane + 64 * k;
        v[k] = make_double2(0.0, 0.0);
        if (i < L) v[k] = x[i];
    }
}

// Capped grid: a wave walks its frames' tiles, pass 1's then pass 2's, and the loads of the tile after this one
// are in flight while this one is computed.  ltf is an argument of its own, const and restrict, as in sync_kernel
__global__ __launch_bounds__(256, SS_WGS_PER_CU) void sync_stf_kernel(SyncStfArgs a, const double2 *__restrict__ ltf)
{
    __shared__ double2 xs[SS_WAVES][SS_SLOTS_PAD];
    __shared__ double2 sq8[SS_WAVES][SS_BLKS_PAD];
    __shared__ double s8[SS_WAVES][SS_BLKS_PAD];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double2 *X = xs[w];
    double2 *SQ = sq8[w];
    double *S = s8[w];
    const double2 *src = reinterpret_cast<const double2 *>(a.capture);
    const int64_t L = a.len;
    const int64_t fstep = (int64_t)gridDim.x * SS_WAVES;
    int64_t f = (int64_t)blockIdx.x * SS_WAVES + w;
    double2 nv[SS_SAMPLES / 64];
    if (f < a.n) ss_load(src + f * a.stride, 0, L, lane, nv);

    // El = sum |ltf|^2, the same bits in every lane; a non-finite ltf marks every frame
    const double2 lv = ltf[lane];
    const bool ltf_bad = __ballot(ss_bad(lv)) != 0;
    double El = ss_abs2(lv);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) El += __shfl_xor(El, m, 64);
    El = readlane_f64(El, 0);

    while (f < a.n) {
        const double2 *xf = src + f * a.stride;
        bool bad = false;
        // ---- pass 1: the lane's running first maximum of |P|^2 (every frame has lag 0, whose |P|^2 >= 0), and
        // what Ms needs there
        double bpp = -1.0, bA = 0.0, bB = 0.0;
        double2 bP = make_double2(0.0, 0.0);
        int32_t bds = 0;
        for (int64_t D0 = 0; D0 <= L - 144; D0 += SS_LAGS_STF) {
            // the tile's samples, loaded while the tile before was computed
#pragma unroll
            for (int k = 0; k < SS_SAMPLES / 64; ++k) {
                const int i = lane + 64 * k;
                bad |= ss_bad(nv[k]);
                X[i + (i >> 3)] = nv[k];
            }
            wave_lds_sync();
            // the tile after this one: the pass's next, or the first of the frame's second pass
            ss_load(xf, D0 + SS_LAGS_STF <= L - 144 ? D0 + SS_LAGS_STF : 0, L, lane, nv);
            // block sums of q and |x|^2 (blocks lane and lane + 64).  q of a block reads the block two on: past
            // the tile that index is clamped and the sum unused (lanes 0..53 read q's sums of blocks <= 69 only)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int blk = lane + 64 * h;
                if (blk < SS_BLKS) {
                    const int b2 = blk + 2;
                    double2 q[8];
                    double p[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const double2 x1 = X[9 * blk + i];
                        q[i] = ss_q(X[9 * b2 + i], x1);
                        p[i] = ss_abs2(x1);
                    }
                    S[blk] = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
                    SQ[blk] = cadd(cadd(cadd(q[0], q[1]), cadd(q[2], q[3])), cadd(cadd(q[4], q[5]), cadd(q[6], q[7])));
                }
            }
            wave_lds_sync();
            // P[8 lane + r] and A[8 lane + r], r < 8; indices past the tile are clamped, their sums unused
            double2 midq = make_double2(0.0, 0.0);
            double midp = 0.0;
#pragma unroll
            for (int k = 1; k < 16; ++k) {
                const int b = lane + k;
                midq = cadd(midq, SQ[b]);
                midp += S[b];
            }
            const int t2 = lane + 2, hb = lane + 16, hb2 = lane + 18;
            double2 tq[8], tailq = make_double2(0.0, 0.0), headq = make_double2(0.0, 0.0);
            double tp[8], tailp = 0.0, headp = 0.0;
#pragma unroll
            for (int r = 7; r >= 0; --r) {
                const double2 x1 = X[9 * lane + r];
                tailq = cadd(tailq, ss_q(X[9 * t2 + r], x1));
                tailp += ss_abs2(x1);
                tq[r] = tailq;
                tp[r] = tailp;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const double2 P = cadd(cadd(tq[r], midq), headq);
                const double A = (tp[r] + midp) + headp;
                const double B = __shfl_down(A, 2, 64);   // A[d + 16]
                const double2 x1 = X[9 * hb + r];
                headq = cadd(headq, ss_q(X[9 * hb2 + r], x1));
                headp += ss_abs2(x1);
                const double pp = ss_abs2(P);
                const int64_t d = D0 + 8 * lane + r;
                if (lane < SS_LAGS_STF / 8 && d <= L - 144 && pp > bpp) { bpp = pp; bP = P; bA = A; bB = B; bds = (int32_t)d; }
            }
            wave_lds_sync();   // the next tile overwrites X, S and SQ
        }
        // the first maximum over the wave, then Ms, e_c and the step rotor: the same bits in every lane, kept in
        // scalar registers through pass 2
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const double opp = __shfl_xor(bpp, m, 64), oA = __shfl_xor(bA, m, 64), oB = __shfl_xor(bB, m, 64);
            const double2 oP = shfl_xor_c(bP, m);
            const int32_t od = __shfl_xor(bds, m, 64);
            if (opp > bpp || (opp == bpp && od < bds)) { bpp = opp; bA = oA; bB = oB; bP = oP; bds = od; }
        }
        const double den_s = bA * bB;
        const double Ms = readlane_f64(den_s == 0.0 ? 0.0 : bpp / den_s, 0);
        const double ec = readlane_f64(atan2(bP.y, bP.x) * 0x1.45f306dc9c883p-7, 0);   // 1 / (32 pi)
        const double2 step = readlane_c(ss_rotor(ec, 64.0), 0);

        // ---- pass 2, as sync_kernel: the lane's running first maximum of q = M^2 / 4 and what M needs there
        double bq = -1.0, ba1 = 0.0, ba2 = 0.0, bden = 0.0;
        int32_t bestd = 0;
        const int64_t nf = f + fstep;
        for (int64_t D0 = 0; D0 <= L - 128; D0 += SS_LAGS_LTF) {
            // the tile's samples, derotated on their way into LDS
            {
                const double2 r0 = ss_rotor(ec, (double)(D0 + lane));
                const double2 s2 = ss_cmul(step, step), s4 = ss_cmul(s2, s2), s8p = ss_cmul(s4, s4);
                double2 rot[SS_SAMPLES / 64];
                rot[0] = r0;
                rot[1] = ss_cmul(r0, step);
                rot[2] = ss_cmul(r0, s2);
                rot[3] = ss_cmul(rot[1], s2);
                rot[4] = ss_cmul(r0, s4);
                rot[5] = ss_cmul(rot[1], s4);
                rot[6] = ss_cmul(rot[2], s4);
                rot[7] = ss_cmul(rot[3], s4);
                rot[8] = ss_cmul(r0, s8p);
#pragma unroll
                for (int k = 0; k < SS_SAMPLES / 64; ++k) {
                    const int i = lane + 64 * k;
                    bad |= ss_bad(nv[k]);
                    X[i + (i >> 3)] = ss_cmul(nv[k], rot[k]);
                }
            }
            wave_lds_sync();
            // the tile after this one: the pass's next, or the first of the wave's next frame
            if (D0 + SS_LAGS_LTF <= L - 128) ss_load(xf, D0 + SS_LAGS_LTF, L, lane, nv);
            else if (nf < a.n) ss_load(src + nf * a.stride, 0, L, lane, nv);
            // block sums of |x|^2 (blocks lane and lane + 64)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int blk = lane + 64 * h;
                if (blk < SS_BLKS) {
                    double p[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) p[i] = ss_abs2(X[9 * blk + i]);
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
                for (int k = 1; k < 16; ++k) mid += S[lane + k];
                const int hb = lane + 16;
                double tail = 0.0, head = 0.0, t[8];
#pragma unroll
                for (int r = 7; r >= 0; --r) { tail += ss_abs2(X[9 * lane + r]); t[r] = tail; }
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    E[r] = (t[r] + mid) + head;
                    head += ss_abs2(X[9 * hb + r]);
                }
            }
            // ranked by q = M^2 / 4 as in sync_kernel; lags ascend with r and with the tile
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const double a1 = ss_abs2(acc[r]);
                const double a2 = __shfl_down(a1, 8, 64);   // |c[d + 64]|^2
                const int64_t d = D0 + 8 * lane + r;
                const double den = El * E[r];
                const double ri = rcp_nr(den);
                const double q = den == 0.0 ? 0.0 : (a1 * ri) * (a2 * ri);
                if (lane < SS_LAGS_LTF / 8 && d <= L - 128 && q > bq) { bq = q; ba1 = a1; ba2 = a2; bden = den; bestd = (int32_t)d; }
            }
            wave_lds_sync();   // the next tile overwrites X and S
        }
        // M at the lane's best lag; then the first maximum over the wave: the larger q, then the lower lag
        double M = bden == 0.0 ? 0.0 : 2.0 * sqrt(ba1) * sqrt(ba2) / bden;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const double oq = __shfl_xor(bq, m, 64), oM = __shfl_xor(M, m, 64);
            const int32_t od = __shfl_xor(bestd, m, 64);
            if (oq > bq || (oq == bq && od < bestd)) { bq = oq; M = oM; bestd = od; }
        }
        const bool poisoned = ltf_bad || __ballot(bad) != 0;
        const int32_t s = bestd - a.backoff;
        const bool det = !poisoned && Ms >= a.threshold_stf && M >= a.threshold_ltf && s >= 0;
        double e = __builtin_nan("");
        if (det) {   // the same in every lane.  s + 128 <= L: the two copies lie inside the window
            double2 c = ss_q(xf[s + 64 + lane], xf[s + lane]);
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) c = cadd(c, shfl_xor_c(c, m));
            const double ef = atan2(c.y, c.x) * 0x1.45f306dc9c883p-9;   // 1 / (128 pi)
            e = ef + rint((ec - ef) * 64.0) * 0.015625;
        }
        if (lane == 0) {
            a.start[f] = det ? s : -1;
            a.cfo[f] = e;
            if (a.metric_stf) a.metric_stf[f] = poisoned ? __builtin_nan("") : Ms;
            if (a.metric_ltf) a.metric_ltf[f] = poisoned ? __builtin_nan("") : M;
        }
        f = nf;
    }
}

int launch_sync_stf(const SyncStfArgs &a, int cus, void *stream)
{
    if (a.n == 0) return 0;
    const int64_t blocks = chain_grid((a.n + SS_WAVES - 1) / SS_WAVES, SS_GRID_PER_CU * (int64_t)cus);
    hipLaunchKernelGGL(sync_stf_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, a,
                       reinterpret_cast<const double2 *>(a.ltf));
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

void sync_stf_tiles(int *lags_stf, int *lags_ltf)
{
    *lags_stf = SS_LAGS_STF;
    *lags_ltf = SS_LAGS_LTF;
}

// ---------------------------------------------------------------- the transmitter's short field
// 160 samples a row, amplitude x the 16-sample period: a store stream, one thread per sample
__global__ __launch_bounds__(256) void short_field_kernel(ShortFieldArgs a)
{
    const int64_t total = a.n * SHORT_FIELD_LEN;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t f = i / SHORT_FIELD_LEN;
        const int m = (int)(i - f * SHORT_FIELD_LEN);
        reinterpret_cast<double2 *>(a.wave)[f * a.stride + m] =
            make_double2(a.amplitude * a.t[2 * (m & 15)], a.amplitude * a.t[2 * (m & 15) + 1]);
    }
}

int launch_short_field(const ShortFieldArgs &a, int cus, void *stream)
{
    if (a.n == 0) return 0;
    const int64_t blocks = chain_grid((a.n * SHORT_FIELD_LEN + 255) / 256, 8 * (int64_t)cus);
    hipLaunchKernelGGL(short_field_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce
