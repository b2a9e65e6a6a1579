// wce_reencode.hip -- gfx950 re-encoder and data-aided LS estimate (wce_reencode):
// the decoder's information bits run forwards through 802.11's code, puncturing,
// interleaver and mapper to the symbols x^ the transmitter sent, and, against the
// received frame, to the decision-directed channel estimate
//     H_dd[k] = sum_b conj(x^_b[k]) rx_b[k] r_b / sum_b |x^_b[k]|^2.
// include/wce.h has the definition.
//
// Mapping: demap_kernel's.  One wave per frame, lane k = subcarrier k, a capped
// grid whose waves stride over the frames; the 15 rx loads are issued before the
// first use.  The frame's packed bits (at most 405 B) are staged once into LDS, a
// byte per lane and load (rows are unaligned and nothing is read past a row's
// ceil(T / 8) bytes), behind one zero word that stands for the encoder's state 0.
// No coded stream is materialised: a lane's transmitted bit j of a block is coded
// bit k = (17.3.5.7's inverse)(j), which is punctured-stream bit b N_CBPS + k, which
// is generator A or B of trellis step b (N_CBPS R) + t0 -- t0 and the generator
// depend on the lane alone and are worked out once per kernel.  Per block the bit
// is the parity of (the 7 information bits ending at that step) & (the generator's
// taps): two LDS words, v_alignbit, an and, a popcount.  The Gray labels index the
// levels the slicer of wce_demodulate decides, (2 i - (M - 1)) d, so x^ has the
// slicer's bits.  Pilots copied from the frames' tx go through LDS as the bits do.
// Lanes 0..14 turn theta, loaded one frame ahead, into the 15 rotors and the block
// loop reads rotor b back from lane b.  The products are spelled out with contraction
// off, so that the build that also stores x^ and the build that does not round
// H_dd alike.  HBM-bound: x^ writes 12.7 KB per frame and reads the bits; H_dd
// alone reads 12.7 KB of rx (x^ never leaves the registers) and writes 848 B.
#include <hip/hip_runtime.h>
#include "wce_internal.h"
#include "wce_device.h"

namespace wce {

constexpr int RE_WAVES = 4;        // frames per 256-thread workgroup
constexpr int RE_GRID_CAP = 4096;
// the generators as masks of the window whose bit 6 is u_t and bit 0 u_{t-6}: 133 and 171 octal
constexpr uint32_t RE_GEN_A = 0133, RE_GEN_B = 0171;
// bit b: the polarity p_b of block b is -1 (the first 15 terms of 802.11's sequence)
constexpr uint32_t RE_POLARITY_NEG = 0x4F70;

template <int MOD, int RATE>
struct ReShape {
    static constexpr int NCB = 48 * MOD;                                         // coded bits per block
    static constexpr int TB = RATE == WCE_RATE_1_2 ? NCB / 2 : (RATE == WCE_RATE_2_3 ? NCB / 3 * 2 : NCB / 4 * 3);
    static constexpr int T = NBLK * TB;                                          // information bits per frame
    static constexpr int NBYTES = (T + 7) / 8;
    static constexpr int NWORDS = 1 + (T + 31) / 32 + 1;   // the zero word, the bits, one word a window's upper read may touch
};

// punctured-stream bit n of a block -> its trellis step within the block and its generator
template <int RATE>
__device__ __forceinline__ void re_step(int n, int &t, uint32_t &gen)
{
    if constexpr (RATE == WCE_RATE_1_2) {
        t = n >> 1;
        gen = (n & 1) ? RE_GEN_B : RE_GEN_A;
    } else if constexpr (RATE == WCE_RATE_2_3) {   // A0 B0 A1 of A0 B0 A1 B1
        const int q = n / 3, r = n - 3 * q;
        t = 2 * q + (r == 2);
        gen = r == 1 ? RE_GEN_B : RE_GEN_A;
    } else {                                       // A0 B0 A1 B2 of A0 B0 A1 B1 A2 B2
        const int q = n >> 2, r = n & 3;
        t = 3 * q + (r == 2 ? 1 : (r == 3 ? 2 : 0));
        gen = (r & 1) ? RE_GEN_B : RE_GEN_A;
    }
}

__device__ __forceinline__ const v2d *re_at(const double *p, int64_t u, uint32_t ko)
{
    return reinterpret_cast<const v2d *>(reinterpret_cast<const char *>(p + 2 * u) + ko);
}
__device__ __forceinline__ double2 re_ld_nt(const double *p, int64_t u, uint32_t ko)
{
    const v2d t = __builtin_nontemporal_load(re_at(p, u, ko));
    return make_double2(t[0], t[1]);
}
__device__ __forceinline__ void re_st_nt(double *p, int64_t u, uint32_t ko, double2 v)
{
    v2d t = {v.x, v.y};
    __builtin_nontemporal_store(t, const_cast<v2d *>(re_at(p, u, ko)));
}
__device__ __forceinline__ void re_st(double *p, int64_t u, uint32_t ko, double2 v)
{
    v2d t = {v.x, v.y};
    *const_cast<v2d *>(re_at(p, u, ko)) = t;
}

// num += conj(x) rx r, den += |x|^2; turn == false: r is 1 and the product is skipped
__device__ __forceinline__ void re_acc(double2 x, double2 rx, double2 r, bool turn, double2 &num, double &den)
{
#pragma clang fp contract(off)
    double2 t = make_double2(fma(x.x, rx.x, x.y * rx.y), fma(x.x, rx.y, -(x.y * rx.x)));
    if (turn) t = make_double2(fma(t.x, r.x, -(t.y * r.y)), fma(t.x, r.y, t.y * r.x));
    num.x = num.x + t.x;
    num.y = num.y + t.y;
    den = den + fma(x.x, x.x, x.y * x.y);
}

// a wave's LDS: the pilots copied from the frames' tx, [block][which pilot], and the frame's bits behind the zero word
template <int MOD, int RATE>
struct alignas(16) ReLds {
    double2 pil[NBLK * 4];
    uint32_t w[ReShape<MOD, RATE>::NWORDS];
};

// frame f on one wave; lds.w[0] = 0; pos[m], gen[m]: where in the frame's bits (counted from w[0]'s bit 0) the window
// of this lane's bit m of block 0 starts, and its generator; rot: lane b's rotor of block b (turn: theta given)
template <int MOD, int RATE, bool TX, bool H>
__device__ __forceinline__ void reencode_frame(const ReencodeArgs &a, int64_t f, int lane, ReLds<MOD, RATE> &lds,
                                               const uint32_t (&pos)[MOD], const uint32_t (&gen)[MOD], double2 rot,
                                               bool turn)
{
    using S = ReShape<MOD, RATE>;
    constexpr int NB = MOD == 1 ? 1 : MOD / 2;   // bits per axis
    constexpr int M = 1 << NB;
    const bool act = lane < NSC;
    const int k = act ? lane : 0;
    const uint32_t ko = 16u * (uint32_t)k;
    const bool pilot = k == WCE_P0 || k == WCE_P1 || k == WCE_P2 || k == WCE_P3;
    const int pi = (k > WCE_P0) + (k > WCE_P1) + (k > WCE_P2);   // which pilot, on a pilot lane
    const bool own_pilots = a.ptx != nullptr;
    const uint32_t *w = lds.w;

    // every load of the frame, issued before any use; the bits and the pilots go through LDS
    double2 rv[NBLK];
    if constexpr (H) {
#pragma unroll
        for (int b = 0; b < NBLK; b++) rv[b] = re_ld_nt(a.rx, f * a.fs + b * a.bs, ko);
    }
    const uint8_t *row = a.bits + f * a.bits_stride;
    uint8_t *wb = reinterpret_cast<uint8_t *>(lds.w + 1);
#pragma unroll
    for (int o = 0; o < S::NBYTES; o += 64)
        if (o + lane < S::NBYTES) wb[o + lane] = row[o + lane];
    if (own_pilots && pilot) {
#pragma unroll
        for (int b = 0; b < NBLK; b++) lds.pil[4 * b + pi] = re_ld_nt(a.ptx, f * a.fs + b * a.bs, ko);
    }
    wave_lds_sync();

    // the 15 x MOD window addresses are formed here, block by block, from values the compiler cannot see through:
    // they do not depend on the frame, and hoisted out of the frame loop they would take 2 registers each
    uint32_t q[MOD];
#pragma unroll
    for (int m = 0; m < MOD; m++) {
        q[m] = pos[m];
        asm volatile("" : "+v"(q[m]));
    }
    const double pil = k == WCE_P3 ? -a.scale : a.scale;
    double2 num = make_double2(0, 0);
    double den = 0.0;
#pragma unroll
    for (int b = 0; b < NBLK; b++) {
        uint32_t lab = 0;
#pragma unroll
        for (int m = 0; m < MOD; m++) {
            const uint32_t p = q[m] + (uint32_t)(b * S::TB);
            const uint32_t win = __builtin_amdgcn_alignbit(w[(p >> 5) + 1], w[p >> 5], p & 31u) & gen[m];
            lab = lab << 1 | ((uint32_t)__popc(win) & 1u);
        }
        double2 x;
        if constexpr (MOD == 1) {
            x = make_double2((double)(2 * (int)lab - 1) * a.d, 0.0);
        } else {
            const uint32_t gi = lab >> NB, gq = lab & (uint32_t)(M - 1);
            const int ii = (int)(gi ^ (gi >> 1) ^ (gi >> 2)), iq = (int)(gq ^ (gq >> 1) ^ (gq >> 2));   // Gray's inverse, <= 3 bits
            x = make_double2((double)(2 * ii - (M - 1)) * a.d, (double)(2 * iq - (M - 1)) * a.d);
        }
        if (pilot) x = own_pilots ? lds.pil[4 * b + pi] : make_double2(((RE_POLARITY_NEG >> b) & 1u) ? -pil : pil, 0.0);
        if (k == WCE_DC) x = make_double2(0, 0);
        if constexpr (TX) {
            if (act) re_st_nt(a.tx, f * a.tfs + b * a.tbs, ko, x);
        }
        if constexpr (H) {
            const double2 r = turn ? readlane_c(rot, b) : rot;
            re_acc(x, rv[b], r, turn && !(r.x == 1.0 && r.y == 0.0), num, den);   // r = 1: the product's bits
            // summed here, block by block: left alone the compiler moves all 15 products down into the store's
            // `if`, and keeps every block's x^ and rx in registers until then
            asm volatile("" : "+v"(num.x), "+v"(num.y), "+v"(den));
        }
    }
    if constexpr (H) {
        double2 hd = make_double2(num.x / den, num.y / den);
        if (k == WCE_DC) hd = make_double2(0, 0);
        if (act) re_st(a.h, f * a.hs, ko, hd);
    }
    wave_lds_sync();   // the next frame's bits go where these were read
}

template <int MOD, int RATE, bool TX, bool H>
__global__ __launch_bounds__(64 * RE_WAVES) void reencode_kernel(ReencodeArgs a)
{
    using S = ReShape<MOD, RATE>;
    constexpr int NB = MOD == 1 ? 1 : MOD / 2;   // bits per axis; also the interleaver's s
    __shared__ ReLds<MOD, RATE> lds[RE_WAVES];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (lane == 0) lds[wv].w[0] = 0;   // u_t = 0 for t < 0: the encoder starts in state 0

    // transmitted bit j = MOD * (index among the data subcarriers) + m is coded bit
    // 16 i - (NCB - 1) floor(16 i / NCB), i = s floor(j / s) + (j + floor(16 j / NCB)) mod s  (17.3.5.7's inverse)
    const int k = lane < NSC ? lane : 0;
    const bool data = lane < NSC && k != WCE_P0 && k != WCE_P1 && k != WCE_P2 && k != WCE_P3 && k != WCE_DC;
    const int dsc = k - (k > WCE_P0) - (k > WCE_P1) - (k > WCE_DC) - (k > WCE_P2) - (k > WCE_P3);
    uint32_t pos[MOD], gen[MOD];
#pragma unroll
    for (int m = 0; m < MOD; m++) {
        const int j = data ? MOD * dsc + m : 0;
        const int i = NB * (j / NB) + (j + 16 * j / S::NCB) % NB;
        const int kc = 16 * i - (S::NCB - 1) * (16 * i / S::NCB);
        int t0;
        re_step<RATE>(kc, t0, gen[m]);
        pos[m] = (uint32_t)(t0 + 32 - 6);   // the window u_{t-6} .. u_t starts 6 bits before bit t; w[0] shifts all by 32
    }

    // a frame's 15 angles are loaded one frame ahead, and turned into the rotors before the frame's own loads are
    // issued: sin and cos beside 15 rx values in flight would double the registers
    const bool turn = H && a.theta != nullptr;
    const int64_t step = (int64_t)gridDim.x * RE_WAVES;
    int64_t f = (int64_t)blockIdx.x * RE_WAVES + wv;
    double th = turn && f < a.n && lane < NBLK ? a.theta[f * NBLK + lane] : 0.0;
#pragma unroll 1
    for (; f < a.n; f += step) {
        double2 rot = turn ? make_double2(cos(th), -sin(th)) : make_double2(1, 0);
        asm volatile("" : "+v"(rot.x), "+v"(rot.y) : : "memory");   // no load of the frame moves up beside sin and cos
        th = turn && f + step < a.n && lane < NBLK ? a.theta[(f + step) * NBLK + lane] : 0.0;
        reencode_frame<MOD, RATE, TX, H>(a, f, lane, lds[wv], pos, gen, rot, turn);
    }
}

template <int MOD, int RATE>
static void reencode_launch(const ReencodeArgs &a, dim3 g, hipStream_t s)
{
    const dim3 t(64 * RE_WAVES);
    if (a.tx && a.h) hipLaunchKernelGGL((reencode_kernel<MOD, RATE, true, true>), g, t, 0, s, a);
    else if (a.h) hipLaunchKernelGGL((reencode_kernel<MOD, RATE, false, true>), g, t, 0, s, a);
    else hipLaunchKernelGGL((reencode_kernel<MOD, RATE, true, false>), g, t, 0, s, a);
}

template <int MOD>
static int reencode_rate(const ReencodeArgs &a, dim3 g, hipStream_t s)
{
    switch (a.rate) {
    case WCE_RATE_1_2: reencode_launch<MOD, WCE_RATE_1_2>(a, g, s); break;
    case WCE_RATE_2_3: reencode_launch<MOD, WCE_RATE_2_3>(a, g, s); break;
    case WCE_RATE_3_4: reencode_launch<MOD, WCE_RATE_3_4>(a, g, s); break;
    default: return WCE_EINVAL;
    }
    return WCE_OK;
}

int launch_reencode(const ReencodeArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    if (a.n > 0x7fffffffll || (!a.tx && !a.h) || (a.h && !a.rx)) return WCE_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = chain_grid((a.n + RE_WAVES - 1) / RE_WAVES, RE_GRID_CAP);
    const dim3 g((uint32_t)blocks);
    int rc;
    switch (a.mod) {
    case WCE_MOD_BPSK: rc = reencode_rate<1>(a, g, s); break;
    case WCE_MOD_QPSK: rc = reencode_rate<2>(a, g, s); break;
    case WCE_MOD_QAM16: rc = reencode_rate<4>(a, g, s); break;
    case WCE_MOD_QAM64: rc = reencode_rate<6>(a, g, s); break;
    default: return WCE_EINVAL;
    }
    if (rc) return rc;
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce
