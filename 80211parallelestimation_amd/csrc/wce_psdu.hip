// wce_psdu.hip -- gfx950 DATA-field framing (wce_psdu_frame) and its inverse (wce_psdu_deframe):
// SERVICE, PSDU, tail and pad, 802.11's scrambler (x^7 + x^4 + 1) and the CRC-32 frame check
// sequence, on the packed information bits wce_reencode reads and wce_viterbi_decode writes.
// include/wce.h has the definition.
//
// Mapping: LPF = 8, 16, 32 or 64 lanes serve a frame, the smallest that covers its ceil(T / 8)
// bytes with a run of 8 consecutive bytes per lane, so a wave serves 8, 4, 2 or 1 frames; the
// frame loop runs on a capped grid.  Row byte r is PSDU octet r - 2 (SERVICE is 16 bits), so a
// lane's run is message octets 8 j - 2 .. 8 j + 5.  Nothing is serial in T:
//   scrambler  every seed's sequence is the seed-127 sequence at a phase (period 127); a lane's
//              64 bits are a funnel shift out of that sequence held twice over (three 64-bit
//              constants), at (64 j + phase) mod 127.  Seed -> phase and first seven bits -> seed
//              are 128-entry tables.
//   CRC        a lane's partial CRC over its own 8 octets (register 0, 64 shift steps; octets
//              outside the message masked to 0, the preset an XOR of ones into message octets
//              0..3), times x^(8 d) mod P, d the octets of the message behind the run (32
//              shift-and-XOR steps against a table of powers), XOR-reduced across the frame's
//              lanes.  Framing runs the same sum over payload || 00 00 00 00 and takes it times
//              x^-32, which is the table four entries lower: a payload shorter than the preset
//              needs no case of its own.
// All tables are computed at compile time from the two polynomials.
#include <hip/hip_runtime.h>
#include "wce_internal.h"

namespace wce {

constexpr int PS_WAVES = 4;          // waves per 256-thread workgroup
constexpr int PS_GRID_CAP = 4096;    // the waves stride over the frame groups
constexpr int PS_GRID_CAP_GOOD = 1024;   // deframing into n_good: a workgroup's add to the one counter takes about
                                         // 10 ns behind the others' (profiles/psdu_65536.txt), so there are fewer
constexpr uint32_t CRC_POLY = 0xEDB88320u;   // 0x04C11DB7, bit-reversed: bit 31 is x^0, bit 0 is x^31
constexpr uint32_t CRC_RESIDUE = 0xDEBB20E3u;   // the register over a good PSDU: ~0x2144DF1C
constexpr int X8_OFF = 12;           // x8[e] = x^(8 (e - 12)) mod P: a run may end 7 octets past the message,
constexpr int X8_N = 424;            // and framing wants 4 octets less; the longest message leaves e <= 408

constexpr uint32_t crc_mulx(uint32_t v) { return (v >> 1) ^ (CRC_POLY & (0u - (v & 1u))); }
constexpr uint32_t crc_divx(uint32_t v) { return (v & 0x80000000u) ? (((v ^ CRC_POLY) << 1) | 1u) : (v << 1); }
// one step of the scrambler: state bit i - 1 is x_i; -> the new state, whose bit 0 is the output x4 ^ x7
constexpr uint32_t scr_step(uint32_t st) { return ((st << 1) | (((st >> 3) ^ (st >> 6)) & 1u)) & 0x7fu; }

struct PsduTab {
    uint32_t x8[X8_N];
    uint8_t phase[128];   // seed -> t with (seed-127 sequence at t ..) = the seed's sequence
    uint8_t seed7[128];   // s_0..s_6 (bit t = s_t) -> the seed that sends them; 0 for 0
};
constexpr PsduTab make_tab()
{
    PsduTab t{};
    uint32_t x = 0x80000000u;   // 1
    for (int i = 0; i < 8 * X8_OFF; i++) x = crc_divx(x);
    for (int e = 0; e < X8_N; e++) {
        t.x8[e] = x;
        for (int i = 0; i < 8; i++) x = crc_mulx(x);
    }
    uint32_t st = 127;
    for (int p = 0; p < 127; p++) {
        t.phase[st] = (uint8_t)p;
        st = scr_step(st);
    }
    for (uint32_t seed = 1; seed < 128; seed++) {
        uint32_t s = seed, v = 0;
        for (int i = 0; i < 7; i++) {
            s = scr_step(s);
            v |= (s & 1u) << i;
        }
        t.seed7[v] = (uint8_t)seed;
    }
    return t;
}
// bits 64 w .. 64 w + 63 of the seed-127 sequence repeated
constexpr uint64_t scr_word(int w)
{
    uint32_t st = 127;
    uint64_t out = 0;
    for (int p = 0; p < 64 * (w + 1); p++) {
        st = scr_step(st);
        if ((p >> 6) == w) out |= (uint64_t)(st & 1u) << (p & 63);
    }
    return out;
}
constexpr uint64_t SCR0 = scr_word(0), SCR1 = scr_word(1), SCR2 = scr_word(2);
static_assert((SCR0 & 0xffffu) == 0x4f70u, "seed 127 begins 00001110 11110010");
static_assert(make_tab().x8[X8_OFF] == 0x80000000u && make_tab().x8[X8_OFF + 1] == 0x00800000u, "x^0 and x^8");
static_assert(make_tab().phase[127] == 0 && make_tab().seed7[0x36] == 93, "seed 93 begins 0110110");

__constant__ const PsduTab PSDU_TAB = make_tab();

// 64 bits of the seed-127 sequence from bit p, p < 127
__device__ __forceinline__ uint64_t scr_run(int p)
{
    const uint64_t lo = p < 64 ? SCR0 : SCR1, hi = p < 64 ? SCR1 : SCR2;
    const int sh = p & 63;
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}
// the register after 8 octets (the low octet first) from register 0: m(x) x^32 mod P
__device__ __forceinline__ uint32_t crc_run(uint64_t m)
{
    uint32_t c = (uint32_t)m;
#pragma unroll
    for (int i = 0; i < 32; i++) c = crc_mulx(c);
    c ^= (uint32_t)(m >> 32);
#pragma unroll
    for (int i = 0; i < 32; i++) c = crc_mulx(c);
    return c;
}
// a b mod P
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = crc_mulx(b);
    }
    return p;
}
// the low k octets set: k <= 0 none, k >= 8 all
__device__ __forceinline__ uint64_t octets_below(int k)
{
    return k <= 0 ? 0ull : k >= 8 ? ~0ull : (1ull << (8 * k)) - 1ull;
}
// up to 8 octets p[i0 .. i0 + 7], those outside [0, n) read as 0; n >= 1 and the run meets [0, n)
__device__ __forceinline__ uint64_t load_run(const uint8_t *p, int i0, int n)
{
    uint64_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int i = i0 + k, ic = i < 0 ? 0 : i >= n ? n - 1 : i;
        m |= (uint64_t)p[ic] << (8 * k);
    }
    return m & octets_below(n - i0) & ~octets_below(-i0);
}

// The register over the frame's L message octets (the lane's own in m, masked) with the preset, times
// x^(8 (off - X8_OFF)): every lane of the frame gets it
template <int LPF>
__device__ __forceinline__ uint32_t frame_crc(uint64_t m, int sub, int L, int off)
{
    if (sub == 0) m ^= 0x0000ffffffff0000ull;   // message octets 0..3 are the first lane's octets 2..5
    int e = L - (8 * sub + 6) + off;            // the run ends at message octet 8 sub + 6
    e = e < 0 ? 0 : e;                          // a run wholly behind the message is 0 whatever it is multiplied by
    uint32_t c = crc_mul(crc_run(m), PSDU_TAB.x8[e]);
#pragma unroll
    for (int d = 1; d < LPF; d <<= 1) c ^= (uint32_t)__shfl_xor((int)c, d, 64);
    return c;
}

template <int LPF, bool DEFRAME>
__global__ __launch_bounds__(256) void psdu_kernel(PsduArgs a)
{
    constexpr int FPW = 64 / LPF;   // frames per wave
    const int lane = threadIdx.x & 63, sub = lane & (LPF - 1);
    const int64_t w = (int64_t)blockIdx.x * PS_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t groups = (a.n + FPW - 1) / FPW;
    const int i0 = 8 * sub - 2;     // the message octet of the lane's first byte
    const int r0 = 8 * sub;         // its row byte
    uint32_t good = 0;
#pragma unroll 1
    for (int64_t g = w; g < groups; g += (int64_t)gridDim.x * PS_WAVES) {
        const int64_t f = g * FPW + lane / LPF;
        const bool act = f < a.n;
        int L = a.length, sd = a.seed;
        if (act && a.lengths) L = a.lengths[f];
        if (!DEFRAME && act && a.seeds) sd = a.seeds[f];
        const bool ok = act && L >= 4 && L <= a.max_len && (DEFRAME || (sd >= 1 && sd <= 127));
        if (!ok) {   // in range for the arithmetic below; nothing of it is kept
            L = 4;
            sd = 1;
        }
        if constexpr (!DEFRAME) {
            const int n = L - 4;
            uint64_t m = 0;
            if (ok && i0 < n && n > 0) m = load_run(a.payload + f * a.payload_stride, i0, n);
            const uint32_t fcs = ~frame_crc<LPF>(m, sub, L, X8_OFF - 4);
            // the FCS, low octet first, at message octets n .. n + 3
            const int q = n - i0;
            m |= q >= 8 || q <= -4 ? 0ull : q >= 0 ? (uint64_t)fcs << (8 * q) : (uint64_t)(fcs >> (-8 * q));
            m ^= scr_run((64 * sub + PSDU_TAB.phase[sd]) % 127);
            // the six tail bits open row byte 2 + L; no bit from T on
            const int kt = 2 + L - r0, nb = a.T - 64 * sub;
            if (kt >= 0 && kt < 8) m &= ~(0x3full << (8 * kt));
            m &= nb <= 0 ? 0ull : nb >= 64 ? ~0ull : (1ull << nb) - 1ull;
            if (!ok) m = 0;
            if (act) {
                uint8_t *row = a.bits_w + f * a.bits_stride;
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (r0 + k < a.nbytes) row[r0 + k] = (uint8_t)(m >> (8 * k));
            }
        } else {
            uint64_t m = 0;
            if (act && r0 < a.nbytes) m = load_run(a.bits_r + f * a.bits_stride, r0, a.nbytes);
            const int first7 = __shfl((int)((uint32_t)m & 0x7fu), lane & ~(LPF - 1), 64);
            const int seed = ok ? PSDU_TAB.seed7[first7] : 0;
            if (seed) m ^= scr_run((64 * sub + PSDU_TAB.phase[seed]) % 127);
            m &= octets_below(L - i0) & ~octets_below(-i0);   // message octets 0 .. L - 1
            const bool fine = ok && seed != 0 && frame_crc<LPF>(m, sub, L, X8_OFF) == CRC_RESIDUE;
            if (ok && a.psdu) {
                uint8_t *row = a.psdu + f * a.psdu_stride;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int i = i0 + k;
                    if (i >= 0 && i < L) row[i] = (uint8_t)(m >> (8 * k));
                }
            }
            if (act && sub == 0) {
                if (a.fcs_ok) a.fcs_ok[f] = fine ? 1u : 0u;
                if (a.oseed) a.oseed[f] = (uint8_t)seed;
            }
            good += (uint32_t)__popcll(__ballot(fine && sub == 0));
        }
    }
    if constexpr (DEFRAME) {
        // one add per workgroup: every add lands on the same word, and they queue there
        __shared__ uint32_t wg_good;
        if (a.n_good) {
            if (threadIdx.x == 0) wg_good = 0;
            __syncthreads();
            if (good && lane == 0) atomicAdd(&wg_good, good);
            __syncthreads();
            if (threadIdx.x == 0 && wg_good) atomicAdd(a.n_good, wg_good);
        }
    }
}

template <bool DEFRAME>
static int psdu_launch(const PsduArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    // 64 lanes of 8 bytes hold the row, the tail's byte 2 + L is in it, and the table reaches the longest message
    if (a.n > 0x7fffffffll || a.nbytes != (a.T + 7) / 8 || a.nbytes > 8 * 64 || a.max_len < 4 ||
        a.max_len + 3 > a.nbytes || a.max_len + X8_OFF >= X8_N)
        return WCE_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int lpf = a.nbytes <= 64 ? 8 : a.nbytes <= 128 ? 16 : a.nbytes <= 256 ? 32 : 64;
    const int64_t groups = (a.n + 64 / lpf - 1) / (64 / lpf);
    const dim3 g((uint32_t)chain_grid((groups + PS_WAVES - 1) / PS_WAVES,
                                      DEFRAME && a.n_good ? PS_GRID_CAP_GOOD : PS_GRID_CAP));
    switch (lpf) {
    case 8: hipLaunchKernelGGL((psdu_kernel<8, DEFRAME>), g, dim3(256), 0, s, a); break;
    case 16: hipLaunchKernelGGL((psdu_kernel<16, DEFRAME>), g, dim3(256), 0, s, a); break;
    case 32: hipLaunchKernelGGL((psdu_kernel<32, DEFRAME>), g, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((psdu_kernel<64, DEFRAME>), g, dim3(256), 0, s, a); break;
    }
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

int launch_psdu_frame(const PsduArgs &a, void *stream)
{
    if (!a.bits_w) return WCE_EINVAL;
    return psdu_launch<false>(a, stream);
}

int launch_psdu_deframe(const PsduArgs &a, void *stream)
{
    if (!a.bits_r || (!a.psdu && !a.oseed && !a.fcs_ok && !a.n_good)) return WCE_EINVAL;
    return psdu_launch<true>(a, stream);
}

}  // namespace wce
