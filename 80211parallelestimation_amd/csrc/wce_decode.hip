// wce_decode.hip -- gfx950 soft demapper (wce_soft_demap) and soft-decision
// Viterbi decoder (wce_viterbi_decode): what follows wce_demodulate's eq on the
// way to information bits.  include/wce.h has the definitions (802.11's K = 7
// code 133/171, its puncturing and its interleaver).
//
// Demapper.  demod_kernel's mapping: one wave per frame, lane k = subcarrier k,
// the 15 eq loads issued before the first use, the blend rounded as dm_blend
// rounds it.  The max-log difference of a Gray axis needs no search: with q_c
// the level nearest to v whose label has the bit equal to c,
//     D0 - D1 = (v - q0)^2 - (v - q1)^2 = (q1 - q0) (2 v - q0 - q1),
// and of the two one is the slicer's decision for v and the other the nearest
// level with the opposite bit, which depends on the decision alone (the
// midpoints between the levels of either set are slicer boundaries): a 3-bit
// entry per level, packed into one constant per bit.  A lane's soft bits (up to
// 6) go to their deinterleaved places of the block through LDS, so the float
// row leaves as contiguous 256-byte stores.  HBM-bound: 12.7 KB of eq in, 2.9 to
// 17.3 KB of soft bits out per frame.  demap_kernel<MOD, true> (wce_soft_demap_blocks)
// reads Hu_b from a row per block, wce_track_demodulate's h_blocks, 12.7 KB more.
//
// Decoder.  One wave per frame, lane s' = successor state.  A step is two
// ds_bpermute reads of the metrics of the predecessors 2 (s' & 31) and + 1, one
// branch metric (the other branch's is its negative: both generators tap u_t
// and u_{t-6}), two adds, a compare that gives the state's decision
// bit, and a select.  The step's LLR pair is wave-uniform: lane l loads and
// depunctures the pair of step 64 c + l one chunk ahead, and the step reads it
// with v_readlane.  Each lane shifts its own decision into a history word and
// stores it every 32 steps (a 256-byte LDS store per wave): 8 B per step per
// wave of survivor memory, as one 64-bit ballot word per step would take, for
// one VALU instruction per step and none on the scalar side.  It is dynamic
// LDS, sized on the host from T.  Traceback loads a group's 64 words with one
// LDS read (lane = state) and walks it on the scalar unit, one v_readlane by
// the current state per step; 64 information bits at a time are stored (and
// compared with the reference bits) a byte per lane.
#include <hip/hip_runtime.h>
#include "wce_internal.h"
#include "wce_device.h"

namespace wce {

constexpr int NDATA = 48;          // data subcarriers per block
constexpr int DC_WAVES = 4;        // demapper: frames per 256-thread workgroup
constexpr int DC_GRID_CAP = 4096;
constexpr int VT_WAVES = 4;        // decoder: most frames per workgroup
constexpr int VT_LDS_MAX = 65536;  // dynamic LDS a workgroup asks for at most
constexpr int VT_GRID_CAP = 1 << 16;
constexpr int64_t VT_LDS_CU = 160 * 1024;   // LDS of a CU
constexpr int VT_SLOTS = 32;                // waves a CU holds

int decode_info_bits(int mod, int rate)
{
    if (mod != WCE_MOD_BPSK && mod != WCE_MOD_QPSK && mod != WCE_MOD_QAM16 && mod != WCE_MOD_QAM64) return WCE_EINVAL;
    const int ntx = NBLK * NDATA * mod;
    switch (rate) {
    case WCE_RATE_1_2: return ntx / 2;
    case WCE_RATE_2_3: return ntx / 3 * 2;
    case WCE_RATE_3_4: return ntx / 4 * 3;
    default: return WCE_EINVAL;
    }
}

// ---------------------------------------------------------------- demapper
// For an axis of NB bits (M = 2^NB levels, level index i, Gray label i ^ (i >> 1), b0 the label's top bit):
// entry i, 3 bits, is the index of the level nearest to level i whose label differs from i's in bit j
constexpr uint32_t dc_opposite(int nb, int j)
{
    const int M = 1 << nb;
    uint32_t t = 0;
    for (int i = 0; i < M; i++) {
        int best = -1, bestd = 2 * M;
        for (int l = 0; l < M; l++) {
            const int dist = l > i ? l - i : i - l;
            if ((((i ^ (i >> 1)) ^ (l ^ (l >> 1))) >> (nb - 1 - j)) & 1)
                if (dist < bestd) { best = l; bestd = dist; }
        }
        t |= (uint32_t)best << (3 * i);
    }
    return t;
}

// the NB soft bits of coordinate v, each w (D0 - D1)
template <int NB>
__device__ __forceinline__ void dc_axis(double v, double w, double d, double inv2d, float *L)
{
    constexpr int M = 1 << NB;
    constexpr uint32_t OPP[3] = {dc_opposite(NB, 0), dc_opposite(NB, NB > 1 ? 1 : 0), dc_opposite(NB, NB > 2 ? 2 : 0)};
    const double t = floor(v * inv2d + 0.5 * M);
    const int i = (int)fmin(fmax(t, 0.0), (double)(M - 1));   // the slicer's level; a NaN goes to 0 and is zeroed later
    const int g = i ^ (i >> 1);
    const int own = 2 * i - (M - 1);
#pragma unroll
    for (int j = 0; j < NB; j++) {
        const int opp = 2 * (int)((OPP[j] >> (3 * i)) & 7u) - (M - 1);
        const bool one = (g >> (NB - 1 - j)) & 1;
        const int dq = one ? own - opp : opp - own;            // q1 - q0
        // saturate, never overflow: a soft bit beyond float's range would leave as Inf and be read as an erasure
        // by vt_llr, the most reliable bits of a strong frame first.  A NaN (Inf 0 of finite e and Hu) is a 0
        const double s = (w * ((double)dq * d)) * (2.0 * v - (double)(own + opp) * d);
        L[j] = s != s ? 0.0f : (float)fmin(fmax(s, -WCE_LLR_MAX), WCE_LLR_MAX);
    }
}

__device__ __forceinline__ const v2d *dc_at(const double *p, int64_t u, uint32_t ko)
{
    return reinterpret_cast<const v2d *>(reinterpret_cast<const char *>(p + 2 * u) + ko);
}
__device__ __forceinline__ double2 dc_ld(const double *p, int64_t u, uint32_t ko)
{
    const v2d t = *dc_at(p, u, ko);
    return make_double2(t[0], t[1]);
}
__device__ __forceinline__ double2 dc_ld_nt(const double *p, int64_t u, uint32_t ko)
{
    const v2d t = __builtin_nontemporal_load(dc_at(p, u, ko));
    return make_double2(t[0], t[1]);
}

// Hu_b = wlt h_lt + wps h with dm_blend's rounding (wce_demod.hip): the fma spelled out, contraction off
__device__ __forceinline__ double2 dc_blend(double2 hlt, double2 hps, int b)
{
#pragma clang fp contract(off)
    const double wlt = (double)(NBLK - (b + 1)) / NBLK, wps = (double)(b + 1) / NBLK;
    return make_double2(fma(hlt.x, wlt, hps.x * wps), fma(hlt.y, wlt, hps.y * wps));
}

// frame f on one wave; buf: this wave's two block rows of MOD * 48 floats in LDS.  BLK: Hu_b is the row a.hb holds
// for block b (15 more loads per lane, issued with eq's), not h or the h / h_lt blend
template <int MOD, bool BLK>
__device__ __forceinline__ void demap_frame(const DemapArgs &a, int64_t f, int lane, float *buf)
{
    constexpr int NB = MOD == 1 ? 1 : MOD / 2;   // bits per axis; also the interleaver's s
    constexpr int NCB = NDATA * MOD;             // coded bits per block
    const bool act = lane < NSC;
    const int k = act ? lane : 0;
    const uint32_t ko = 16u * (uint32_t)k;
    const bool data = act && k != WCE_P0 && k != WCE_P1 && k != WCE_P2 && k != WCE_P3 && k != WCE_DC;
    const bool blend = !BLK && a.hlt != nullptr;

    // every load of the frame, issued before any use
    double2 ev[NBLK], hv[BLK ? NBLK : 1];
#pragma unroll
    for (int b = 0; b < NBLK; b++) ev[b] = dc_ld_nt(a.eq, f * a.efs + b * a.ebs, ko);
    double2 hps = make_double2(0, 0), hlt = make_double2(0, 0);
    if constexpr (BLK) {
#pragma unroll
        for (int b = 0; b < NBLK; b++) hv[b] = dc_ld_nt(a.hb, f * a.hbfs + b * a.hbbs, ko);
    } else {
        hps = dc_ld(a.h, f * a.hs, ko);
        if (blend) hlt = dc_ld(a.hlt, f * a.hs, ko);
    }

    // where this lane's bits go: transmitted bit j = MOD * (index among the data subcarriers) + m is coded bit
    // 16 i - (NCB - 1) floor(16 i / NCB), i = s floor(j / s) + (j + floor(16 j / NCB)) mod s  (17.3.5.7's inverse)
    const int dsc = k - (k > WCE_P0) - (k > WCE_P1) - (k > WCE_DC) - (k > WCE_P2) - (k > WCE_P3);
    int dest[MOD];
#pragma unroll
    for (int m = 0; m < MOD; m++) {
        const int j = data ? MOD * dsc + m : 0;
        const int i = NB * (j / NB) + (j + 16 * j / NCB) % NB;
        dest[m] = 16 * i - (NCB - 1) * (16 * i / NCB);
    }
    const double inv2d = 1.0 / (2.0 * a.d);

#pragma unroll
    for (int b = 0; b < NBLK; b++) {
        const double2 hu = BLK ? hv[BLK ? b : 0] : blend ? dc_blend(hlt, hps, b) : hps;
        const double w = hu.x * hu.x + hu.y * hu.y;
        const bool ok = isfinite(ev[b].x) && isfinite(ev[b].y) && isfinite(hu.x) && isfinite(hu.y);
        float L[MOD];
        dc_axis<NB>(ev[b].x, w, a.d, inv2d, L);
        if constexpr (MOD > 1) dc_axis<NB>(ev[b].y, w, a.d, inv2d, L + NB);
        float *row = buf + (b & 1) * NCB;
        if (data) {
#pragma unroll
            for (int m = 0; m < MOD; m++) row[dest[m]] = ok ? L[m] : 0.0f;   // not finite: an erasure
        }
        wave_lds_sync();
        float *out = a.llr + (f * a.lfs + b * a.lbs);
#pragma unroll
        for (int o = 0; o < NCB; o += 64)
            if (o + lane < NCB) __builtin_nontemporal_store(row[o + lane], out + (o + lane));
        // the row written next is the other one; the one after that comes behind the next block's sync
    }
    wave_lds_sync();
}

template <int MOD, bool BLK>
__global__ __launch_bounds__(64 * DC_WAVES) void demap_kernel(DemapArgs a)
{
    __shared__ float rows[DC_WAVES][2 * NDATA * MOD];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#pragma unroll 1
    for (int64_t f = (int64_t)blockIdx.x * DC_WAVES + wv; f < a.n; f += (int64_t)gridDim.x * DC_WAVES)
        demap_frame<MOD, BLK>(a, f, lane, rows[wv]);
}

template <int MOD>
static void demap_launch(const DemapArgs &a, dim3 g, dim3 t, hipStream_t s)
{
    if (a.hb) hipLaunchKernelGGL((demap_kernel<MOD, true>), g, t, 0, s, a);
    else hipLaunchKernelGGL((demap_kernel<MOD, false>), g, t, 0, s, a);
}

int launch_demap(const DemapArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    if (a.n > 0x7fffffffll) return WCE_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = chain_grid((a.n + DC_WAVES - 1) / DC_WAVES, DC_GRID_CAP);
    const dim3 g((uint32_t)blocks), t(64 * DC_WAVES);
    switch (a.mod) {
    case WCE_MOD_BPSK: demap_launch<1>(a, g, t, s); break;
    case WCE_MOD_QPSK: demap_launch<2>(a, g, t, s); break;
    case WCE_MOD_QAM16: demap_launch<4>(a, g, t, s); break;
    case WCE_MOD_QAM64: demap_launch<6>(a, g, t, s); break;
    default: return WCE_EINVAL;
    }
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

// ---------------------------------------------------------------- decoder
__device__ __forceinline__ float vt_readlane(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ float vt_gather(float v, int byte_addr)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute(byte_addr, __float_as_int(v)));
}

// element n of the frame's punctured stream (n < 0: a punctured place); a non-finite LLR reads as 0
__device__ __forceinline__ float vt_llr(const float *fr, int64_t lbs, int ncb, int n)
{
    if (n < 0) return 0.0f;
    const int b = n / ncb;
    const float v = fr[b * lbs + (n - b * ncb)];
    return isfinite(v) ? v : 0.0f;
}

// the depunctured pair (L_A, L_B) of trellis step t (0, 0 from step T on)
template <int RATE>
__device__ __forceinline__ void vt_pair(const float *fr, int64_t lbs, int ncb, int T, int t, float &la, float &lb)
{
    int ia = -1, ib = -1;
    if (t < T) {
        if constexpr (RATE == WCE_RATE_1_2) {
            ia = 2 * t;
            ib = 2 * t + 1;
        } else if constexpr (RATE == WCE_RATE_2_3) {   // A0 B0 A1 of A0 B0 A1 B1
            const int q = t >> 1, r = t & 1;
            ia = 3 * q + 2 * r;
            ib = r ? -1 : 3 * q + 1;
        } else {                                       // A0 B0 A1 B2 of A0 B0 A1 B1 A2 B2
            const int q = t / 3, r = t - 3 * q;
            ia = r == 2 ? -1 : 4 * q + 2 * r;
            ib = r == 0 ? 4 * q + 1 : (r == 2 ? 4 * q + 3 : -1);
        }
    }
    la = vt_llr(fr, lbs, ncb, ia);
    lb = vt_llr(fr, lbs, ncb, ib);
}

struct VtLane {
    float sa, sb;   // +1 where the coded bit of the branch from p0 is 1, else -1
    int a0, a1;     // byte addresses of lanes p0 and p1 for ds_bpermute
};

// one trellis step: the pair is lane i's of (la, lb); the lane's decision is shifted into its history word
__device__ __forceinline__ void vt_step(const VtLane &c, float la, float lb, int i, float &pm, uint32_t &hist)
{
    const float bm = fmaf(c.sa, vt_readlane(la, i), c.sb * vt_readlane(lb, i));   // exact: the factors are +-1
    const float x0 = vt_gather(pm, c.a0) + bm, x1 = vt_gather(pm, c.a1) - bm;
    const bool d = x1 > x0;                                                        // p0 wins a tie
    pm = d ? x1 : x0;
    hist = hist << 1 | (uint32_t)d;
}

template <int RATE>
__global__ __launch_bounds__(64 * VT_WAVES) void viterbi_kernel(ViterbiArgs a)
{
    extern __shared__ uint32_t vt_words[];   // [waves][ceil(T / 32)][64] decision histories
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = (int)(blockDim.x >> 6);
    const int T = a.T, ncb = NDATA * a.mod, ngr = (T + 31) >> 5, nbytes = (T + 7) >> 3;
    uint32_t *dec = vt_words + (size_t)wv * ngr * 64;

    VtLane c;
    {
        const int p0 = 2 * (lane & 31), u = lane >> 5;
        // the register before the step: bit 5 = u_{t-1} ... bit 0 = u_{t-6}; 133: u_t, t-2, t-3, t-5, t-6; 171: u_t, t-1, t-2, t-3, t-6
        const int ca = (u ^ (p0 >> 4) ^ (p0 >> 3) ^ (p0 >> 1) ^ p0) & 1;
        const int cb = (u ^ (p0 >> 5) ^ (p0 >> 4) ^ (p0 >> 3) ^ p0) & 1;
        c.sa = ca ? 1.0f : -1.0f;
        c.sb = cb ? 1.0f : -1.0f;
        c.a0 = 4 * p0;
        c.a1 = 4 * (p0 + 1);
    }

#pragma unroll 1
    for (int64_t f = (int64_t)blockIdx.x * waves + wv; f < a.n; f += (int64_t)gridDim.x * waves) {
        const float *fr = a.llr + f * a.lfs;
        float pm = lane == 0 ? 0.0f : -__builtin_inff();
        float la, lb;
        vt_pair<RATE>(fr, a.lbs, ncb, T, lane, la, lb);
        // groups of 32 steps: group g's word of state s', dec[64 g + s'], holds the decision of step 32 g + i
        // in bit (steps of the group) - 1 - i
#pragma unroll 1
        for (int g = 0; g < ngr; g += 2) {
            float na, nb;   // the next 64 steps' pairs, in flight during these
            vt_pair<RATE>(fr, a.lbs, ncb, T, 32 * (g + 2) + lane, na, nb);
            const int n = min(64, T - 32 * g);
            uint32_t h0 = 0, h1 = 0;
            if (n == 64) {
#pragma unroll
                for (int i = 0; i < 32; i++) vt_step(c, la, lb, i, pm, h0);
#pragma unroll
                for (int i = 32; i < 64; i++) vt_step(c, la, lb, i, pm, h1);
            } else {
#pragma unroll 1
                for (int i = 0; i < min(n, 32); i++) vt_step(c, la, lb, i, pm, h0);
#pragma unroll 1
                for (int i = 32; i < n; i++) vt_step(c, la, lb, i, pm, h1);
            }
            dec[64 * g + lane] = h0;
            if (n > 32) dec[64 * (g + 1) + lane] = h1;
            la = na;
            lb = nb;
        }
        wave_lds_sync();

        // where the survivor ends: state 0, or the best final metric (the lowest state of a tie)
        uint32_t s = 0;
        if (!(a.flags & WCE_DEC_TERMINATED)) {
            float mx = pm;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
            s = (uint32_t)__ffsll((unsigned long long)__ballot(pm == mx)) - 1u;
        }
        s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);

        // back over the groups, two at a time so that 64 information bits leave together, a byte per lane
        uint32_t errs = 0;
#pragma unroll 1
        for (int g = (ngr - 1) & ~1; g >= 0; g -= 2) {
            const int n = min(64, T - 32 * g);
            const int w0 = (int)dec[64 * g + lane], w1 = n > 32 ? (int)dec[64 * (g + 1) + lane] : 0;
            uint64_t out = 0;   // bit i: information bit 32 g + i
#pragma unroll 1
            for (int i = n - 1; i >= 32; i--) {
                out |= (uint64_t)(s >> 5) << i;
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane(w1, (int)s);
                s = ((s & 31u) << 1) | ((w >> (n - 1 - i)) & 1u);
            }
            const int n0 = min(n, 32);
#pragma unroll 1
            for (int i = n0 - 1; i >= 0; i--) {
                out |= (uint64_t)(s >> 5) << i;
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane(w0, (int)s);
                s = ((s & 31u) << 1) | ((w >> (n0 - 1 - i)) & 1u);
            }
            const int byte = 4 * g + lane;
            if (lane < 8 && byte < nbytes) {
                const uint32_t v = (uint32_t)(out >> (8 * lane)) & 0xffu;
                if (a.bits) a.bits[f * a.bits_stride + byte] = (uint8_t)v;
                if (a.ref) {
                    const int left = T - 8 * byte;   // bits of this byte that are information bits
                    const uint32_t mask = left >= 8 ? 0xffu : (1u << left) - 1u;
                    errs += (uint32_t)__popc((v ^ a.ref[f * a.ref_stride + byte]) & mask);
                }
            }
        }
        if (a.nbiterr) {
            errs += __shfl_xor(errs, 1, 64);
            errs += __shfl_xor(errs, 2, 64);
            errs += __shfl_xor(errs, 4, 64);
            if (lane == 0) a.nbiterr[f] = errs;
        }
        wave_lds_sync();   // the next frame's words go where these were read
    }
}

// survivor memory per wave: 64 states x 4 B per 32 steps
static int64_t vt_lds_bytes(int T) { return (int64_t)((T + 31) / 32) * 256; }

int launch_viterbi(const ViterbiArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    if (a.n > 0x7fffffffll || a.T <= 0) return WCE_EINVAL;
    // waves per workgroup: of 4, 2 and 1 (within VT_LDS_MAX) the count that lets a CU's LDS hold the most waves,
    // the larger of equals; the survivor memory, not registers, sets the decoder's occupancy
    int waves = 0, best = 0;
    for (int w = VT_WAVES; w >= 1; w >>= 1) {
        const int64_t need = w * vt_lds_bytes(a.T);
        if (need > VT_LDS_MAX) continue;
        const int64_t per_cu = VT_LDS_CU / need * w;
        const int held = per_cu > VT_SLOTS ? VT_SLOTS : (int)per_cu;
        if (held > best) { best = held; waves = w; }
    }
    if (waves == 0) return WCE_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = chain_grid((a.n + waves - 1) / waves, VT_GRID_CAP);
    const dim3 g((uint32_t)blocks), t(64 * waves);
    const size_t lds = (size_t)(waves * vt_lds_bytes(a.T));
    switch (a.rate) {
    case WCE_RATE_1_2: hipLaunchKernelGGL(viterbi_kernel<WCE_RATE_1_2>, g, t, lds, s, a); break;
    case WCE_RATE_2_3: hipLaunchKernelGGL(viterbi_kernel<WCE_RATE_2_3>, g, t, lds, s, a); break;
    case WCE_RATE_3_4: hipLaunchKernelGGL(viterbi_kernel<WCE_RATE_3_4>, g, t, lds, s, a); break;
    default: return WCE_EINVAL;
    }
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce
