// wce_transmit.hip -- gfx950 transmitter and channel (wce_modulate, wce_channel,
// wce_transmit): 53-bin symbols -> 64-point inverse DFT with cyclic prefix ->
// multipath FIR, carrier offset, Gaussian noise -> raw capture windows, the input
// of wce_front_end_sync.  include/wce.h has the definitions.
//
// One wave per frame.  The inverse DFT is wce_front.hip's 8 x 8 Cooley-Tukey run
// backwards, 8 lanes per unit (the field or a block), with the same table
// conjugated: k = 8 a + b, n = c + 8 d,
//   y[c + 8 d] = 1/64 sum_b W8^(-b d) W64^(-b c) sum_a Y[8 a + b] W8^(-a c)
// stage 1 on lane b, twiddle, the 8 x 8 transpose through LDS, stage 2 on lane c.
// A unit's 64 samples go to the frame's clean waveform in LDS, the prefix and the
// field's second copy as second stores of the same registers.
//
// The channel works on tiles of 512 window samples.  Lane l owns the 8 consecutive
// outputs 8 l .. 8 l + 7 of a tile: it reads the 23 clean samples under them once
// (2.9 LDS reads per output where a lane per output would read n_taps) and runs
// the taps over them in registers, t ascending, each tap read from lane t's
// register.  The waveform is kept with one pad slot after every 8 samples, so that
// lanes 8 samples apart are 9 slots apart: 16 lanes' 16-B reads fall on 16
// different slots of the 256-B bank row.  The 8 sums go through a second, equally
// padded LDS tile and come back lane-contiguous: rotor, noise and the store then
// run once per sample in one loop, and a wave's 64 lanes store 1 KB contiguous.
//
// wce_transmit never writes the clean waveform to memory; wce_modulate copies it
// out of LDS, and wce_channel stages each tile's 527 samples from memory into the
// same layout.  All three run tx_idft_units and tx_channel_tile, and this file is
// compiled with contraction off (its fmas are spelled out), so the fused call
// gives the bits of the pair.
#include <hip/hip_runtime.h>
#include "wce_internal.h"
#include "wce_device.h"
#include "wce_dft64.h"

namespace wce {

constexpr int TX_FIELD = 160, TX_BLOCK = 80;
constexpr int TX_SMAX = TX_FIELD + TX_BLOCK * NBLK;   // 1,360 clean samples at most
constexpr int TX_RUN = 8;                             // consecutive outputs a lane owns
constexpr int TX_TILE = 64 * TX_RUN;                  // outputs per tile
constexpr int TX_HALO = 15;                           // samples before a tile its first output reads (16 taps)
constexpr int TX_WIN = TX_RUN + TX_HALO;              // clean samples under a lane's run
constexpr int TX_GRID_CAP = 1 << 20;
// slot of sample r: one pad slot after every 8
__host__ __device__ constexpr int tx_slot(int r) { return r + (r >> 3); }
constexpr int TX_WAVE_SLOTS = tx_slot(TX_SMAX - 1) + 1;            // the clean waveform of a frame
constexpr int TX_STAGE_SLOTS = tx_slot(TX_TILE + TX_HALO - 1) + 1;   // the clean samples under one tile
constexpr int TX_TILE_SLOTS = tx_slot(TX_TILE - 1) + 1;            // a tile's sums; also the 8 units' transposes
static_assert(TX_TILE_SLOTS >= 8 * 64, "the tile buffer holds the inverse DFT's transposes");
// the time-varying channel's knots under a tile: a segment (two neighbouring knots) is a row of 16 (a, d) pairs,
// a the knot and d the step per sample to the next.  A knot period is at least 16 samples, so a tile's 512 outputs
// lie in at most 33 segments.  A row is 2 n_taps + 1 slots, one of them a pad: lanes in one segment read one
// address (a broadcast), lanes in neighbouring segments read an odd number of 16-B slots apart (16 taps: 528 B, 16 B
// on in the 256-B bank row), where unpadded rows of 16 taps (512 B) would put every segment of a 16-lane read group
// on the same banks.  The rows are dynamic LDS, as many as the call needs (tx_knot_rows): 18 rows of 13 slots,
// 3.7 KB, for a full packet of 6 taps at a period of 80, which leaves transmit_tv_kernel four workgroups a CU as
// transmit_kernel has; 33 rows of 33 slots, 17.4 KB, at the most (three workgroups a CU).
// (-DWCE_TX_KNOT_PAD=0 and -DWCE_TX_KNOT_ONCE=0 build the alternatives tools/ab_fading.py timed: DESIGN s5)
#ifndef WCE_TX_KNOT_PAD
#define WCE_TX_KNOT_PAD 1
#endif
#ifndef WCE_TX_KNOT_ONCE
#define WCE_TX_KNOT_ONCE 1
#endif
constexpr int TX_PMIN = 16;                                        // the shortest knot period
constexpr int TX_KSEG = (TX_TILE - 1) / TX_PMIN + 2;               // segments under a tile at most
__host__ __device__ constexpr int tx_krow(int nt) { return 2 * nt + WCE_TX_KNOT_PAD; }   // slots a segment

// in-register 8-point inverse DFT (unscaled): conj, dft8, conj
__device__ __forceinline__ void idft8(double2 (&x)[8])
{
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i].y = -x[i].y;
    dft8(x);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i].y = -x[i].y;
}

// exp(+2 pi i e n): cfo_rotor's exact-phase construction with the opposite sign
__device__ __forceinline__ double2 tx_rotor(double e, double n)
{
    const double hi = e * n, lo = fma(e, n, -hi);
    const double t = (hi - rint(hi)) + lo;
    double s, c;
    sincospi(2.0 * t, &s, &c);
    return make_double2(c, s);
}

// a b, two products rounded and two fused (cmul_tw's roundings)
__device__ __forceinline__ double2 tx_cmul(double2 a, double2 b)
{
    return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.y, b.x, a.x * b.y));
}

// Units u0 .. u0 + 7 of frame f (unit 0 is the field where a.field, the blocks follow) -> clean samples in buf,
// sample r at buf[tx_slot(r)].  Lane group g = lane >> 3 has unit u0 + g; T: 8 x 64 entries of transpose space.
__device__ __forceinline__ void tx_idft_units(const TxArgs &a, int64_t f, int u0, int lane, double2 *T, double2 *buf)
{
    const int g = lane >> 3, j = lane & 7;
    const int u = u0 + g, n_units = a.field + a.nb;
    const bool live = u < n_units;
    const bool pre = a.field && u == 0;
    const int blk = u - a.field;
    const double *X = pre ? a.pre + 2 * (f * a.pre_stride) : a.sym + 2 * (f * a.fs + (int64_t)(live ? blk : 0) * a.bs);
    // stage 1 (lane = b): Y[8 a + b] = X[(8 a + b + 26) mod 64] where that is below 53, else 0
    double2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int i = (8 * q + j + 26) & 63;
        v[q] = live && i < NSC ? ld2(X, i) : make_double2(0.0, 0.0);
    }
    idft8(v);
#pragma unroll
    for (int c = 1; c < 8; ++c) v[c] = tx_cmul(v[c], cconj(kW64[(j * c) & 63]));
    // transpose: element (b, c) at b * 8 + (c ^ b)
    double2 *Tu = T + 64 * g;
#pragma unroll
    for (int c = 0; c < 8; ++c) Tu[j * 8 + (c ^ j)] = v[c];
    wave_lds_sync();
#pragma unroll
    for (int b = 0; b < 8; ++b) v[b] = Tu[b * 8 + (j ^ b)];
    wave_lds_sync();
    // stage 2 (lane = c): sample n = c + 8 d
    idft8(v);
    if (!live) return;
    const int base = pre ? 0 : a.field * TX_FIELD + blk * TX_BLOCK;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const int n = j + 8 * d;
        const double2 y = cscale(v[d], 1.0 / 64.0);
        if (pre) {   // y[32..63], y, y
            buf[tx_slot(32 + n)] = y;
            buf[tx_slot(96 + n)] = y;
            if (n >= 32) buf[tx_slot(n - 32)] = y;
        } else {     // y[48..63], y
            buf[tx_slot(base + 16 + n)] = y;
            if (n >= 48) buf[tx_slot(base + n - 48)] = y;
        }
    }
}

// the whole clean waveform of frame f into buf; every lane returns
__device__ __forceinline__ void tx_modulate_frame(const TxArgs &a, int64_t f, int lane, double2 *T, double2 *buf)
{
    const int n_units = a.field + a.nb;
#pragma unroll 1
    for (int u0 = 0; u0 < n_units; u0 += 8) tx_idft_units(a, f, u0, lane, T, buf);
    wave_lds_sync();
}

// what the channel needs of a frame, the same on every lane but tap
struct TxFrame {
    double2 tap;       // lane t: h[t], 0 from n_taps on
    double e, sg;      // offset; sqrt(ow2 / 2)
    uint64_t key;
    int64_t delay;
    bool rot, noisy, bad;
};

__device__ __forceinline__ bool tx_nonfinite(double v) { return v * 0.0 != 0.0; }
__device__ __forceinline__ bool tx_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

// bad so far: a non-finite clean sample
__device__ __forceinline__ TxFrame tx_frame(const TxArgs &a, int64_t f, int lane, bool bad)
{
    TxFrame c;
    c.tap = make_double2(0.0, 0.0);
    if (lane < a.nt) c.tap = a.taps ? ld2(a.taps, f * a.ts + lane) : make_double2(lane == 0 ? 1.0 : 0.0, 0.0);
    c.e = a.cfo ? a.cfo[f] : 0.0;
    const double o = a.ow2 ? a.ow2[f] : 0.0;
    c.bad = tx_any(bad || tx_nonfinite(c.tap.x) || tx_nonfinite(c.tap.y) || tx_nonfinite(c.e) || tx_nonfinite(o) ||
                   o < 0.0);
    c.rot = c.e != 0.0;
    c.noisy = o != 0.0;
    c.sg = sqrt(o * 0.5);
    c.key = mix64(a.seed ^ mix64((uint64_t)(a.first + f)));
    c.delay = a.delay ? a.delay[f] : 0;
    return c;
}

// window sample i's noise: Box-Muller on two mix64 draws
__device__ __forceinline__ double2 tx_noise(uint64_t key, uint64_t i, double sg)
{
    const uint64_t ra = mix64(key ^ (2 * i)), rb = mix64(key ^ (2 * i + 1));
    const double u1 = (double)((ra >> 11) + 1) * 0x1p-53, u2 = (double)(rb >> 11) * 0x1p-53;
    const double amp = sg * sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    return make_double2(amp * c, amp * s);
}

// ---- the time-varying channel's knots
// what tx_channel_tile<true> needs beside the static path's arguments
struct TxSegs {
    const TxKnots *kn;
    double2 *K;        // the rows, tx_krow(nt) slots each
    int64_t f;
    int64_t k0;        // the first staged segment
    int nseg;          // how many are staged, 1 .. TX_KSEG
    bool once;         // staged by the kernel for the whole frame
};

// +0, or NaN when one of frame f's nk x nt knot values is not finite.  Lane = 16 k' + t: four knots a trip
__device__ __forceinline__ double tx_knots_scan(const TxKnots &kn, int nt, int64_t f, int lane)
{
    const double *base = kn.knots + 2 * (f * kn.fs);
    const int t = lane & 15;
    double z = 0.0;
    if (t < nt) {
#pragma unroll 2
        for (int64_t k = lane >> 4; k < kn.nk; k += 4) {
            const double2 s = ld2(base, k * kn.ks + t);
            z = fma(s.x, 0.0, fma(s.y, 0.0, z));
        }
    }
    return z;
}

// segments k0 .. k0 + nseg - 1 of frame f into K: row s holds (a[k0 + s][t], d[k0 + s][t]) at slots 2 t, 2 t + 1,
// d = (a[k + 1] - a[k]) / period, subtracted and divided once here, in fp64, part by part
__device__ __forceinline__ void tx_stage_knots(const TxKnots &kn, int nt, int64_t f, int64_t k0, int nseg, int lane,
                                               double2 *K)
{
    const double *base = kn.knots + 2 * (f * kn.fs);
    const double P = (double)kn.period;
    const int t = lane & 15;
    if (t < nt) {
#pragma unroll 1
        for (int s = lane >> 4; s < nseg; s += 4) {
            const double2 lo = ld2(base, (k0 + s) * kn.ks + t), hi = ld2(base, (k0 + s + 1) * kn.ks + t);
            K[s * tx_krow(nt) + 2 * t] = lo;
            K[s * tx_krow(nt) + 2 * t + 1] = make_double2((hi.x - lo.x) / P, (hi.y - lo.y) / P);
        }
    }
    wave_lds_sync();
}

// Window samples i0 .. i0 + 511 (below clen) of frame f's capture row `out`.  buf holds the clean samples
// mbase .. of a waveform of wlen samples, sample m at buf[tx_slot(m - mbase)]: every m of [0, wlen) within
// [i0 - delay - 15, i0 - delay + 512) is there.  T: the tile's sums.
//
// TV: the taps of output m are interpolated between the knots of m's segment (include/wce.h, wce_channel_tv):
// v.K holds the (a, d) rows of segments v.k0 .. v.k0 + v.nseg - 1 -- every segment an output of [0, sig) of this
// tile lies in -- staged here per tile unless v.once (then the kernel staged the frame's).  A lane takes the pair
// of its run's first segment and of the next, forms each output's tap with two fmas and runs the static path's
// sums over them: where d is +0 the tap is a and the sums are the static path's bits.
template <bool TV>
__device__ __forceinline__ void tx_channel_tile(const TxArgs &a, const TxFrame &c, const double2 *buf, int64_t mbase,
                                                int64_t wlen, double2 *T, int64_t i0, int64_t clen, double *out, int lane,
                                                TxSegs v = TxSegs{})
{
    const int64_t m0 = i0 - c.delay;   // the waveform sample under the tile's first output
    const bool any = m0 + TX_TILE > 0 && m0 - TX_HALO < wlen;   // else every sum is 0
    if (TV && any && !v.once) {
        // the tile's outputs within [0, last]; any: m0 + 511 >= 0, but with fewer than 16 taps m0 may lie past the
        // last output (then one segment is staged and every sum is dropped)
        const int64_t last = wlen + a.nt - 2;
        const uint32_t lo = (uint32_t)(m0 < 0 ? 0 : m0 > last ? last : m0);
        const uint32_t hi = (uint32_t)(m0 + TX_TILE - 1 < last ? m0 + TX_TILE - 1 : last);
        v.k0 = lo / (uint32_t)v.kn->period;
        v.nseg = (int)(hi / (uint32_t)v.kn->period - v.k0) + 1;
        tx_stage_knots(*v.kn, a.nt, v.f, v.k0, v.nseg, lane, v.K);
    }
    if (any) {
        double2 win[TX_WIN];
        const int64_t mlo = m0 + TX_RUN * lane - TX_HALO;
#pragma unroll
        for (int q = 0; q < TX_WIN; ++q) {
            const int64_t m = mlo + q;
            const bool ok = m >= 0 && m < wlen;
            const double2 s = buf[tx_slot(ok ? (int)(m - mbase) : 0)];
            win[q] = ok ? s : make_double2(0.0, 0.0);
        }
        double2 acc[TX_RUN];
#pragma unroll
        for (int r = 0; r < TX_RUN; ++r) acc[r] = make_double2(0.0, 0.0);
        if constexpr (TV) {
            // the run's first output m = mf lies in segment kf at j0 samples past its knot; the outputs from
            // j0 + r >= period on lie in the next (a period is at least 16 > 8: one knot a run at most).  A run
            // that begins before 0 is in segment 0 with j0 < 0, one that begins past the last output reads
            // rows that are there and gives sums that are dropped below.
            const int64_t mf = m0 + TX_RUN * lane, last = wlen + a.nt - 2;
            const int64_t P = v.kn->period;
            const uint32_t kf = (uint32_t)(mf < 0 ? 0 : mf > last ? last : mf) / (uint32_t)P;
            const int64_t j0 = mf - (int64_t)kf * P, row = (int64_t)kf - v.k0;
            const int row0 = row < 0 ? 0 : row > v.nseg - 1 ? v.nseg - 1 : (int)row;
            const int row1 = row0 + 1 > v.nseg - 1 ? v.nseg - 1 : row0 + 1;
            const double2 *K0 = v.K + row0 * tx_krow(a.nt), *K1 = v.K + row1 * tx_krow(a.nt);
            double jr[TX_RUN];
            bool next[TX_RUN];
#pragma unroll
            for (int r = 0; r < TX_RUN; ++r) {
                next[r] = j0 + r >= P;
                jr[r] = (double)(next[r] ? j0 + r - P : j0 + r);
            }
#pragma unroll
            for (int t = 0; t <= TX_HALO; ++t) {
                if (t < a.nt) {
                    const double2 a0 = K0[2 * t], d0 = K0[2 * t + 1], a1 = K1[2 * t], d1 = K1[2 * t + 1];
#pragma unroll
                    for (int r = 0; r < TX_RUN; ++r) {
                        const double2 ka = next[r] ? a1 : a0, kd = next[r] ? d1 : d0;
                        const double2 h = make_double2(fma(jr[r], kd.x, ka.x), fma(jr[r], kd.y, ka.y));
                        const double2 s = win[TX_HALO + r - t];
                        acc[r].x = fma(-h.y, s.y, fma(h.x, s.x, acc[r].x));
                        acc[r].y = fma(h.y, s.x, fma(h.x, s.y, acc[r].y));
                    }
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t <= TX_HALO; ++t) {
                if (t < a.nt) {
                    const double2 h = readlane_c(c.tap, t);
#pragma unroll
                    for (int r = 0; r < TX_RUN; ++r) {
                        const double2 s = win[TX_HALO + r - t];
                        acc[r].x = fma(-h.y, s.y, fma(h.x, s.x, acc[r].x));
                        acc[r].y = fma(h.y, s.x, fma(h.x, s.y, acc[r].y));
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < TX_RUN; ++r) T[tx_slot(TX_RUN * lane + r)] = acc[r];
    }
    wave_lds_sync();
    const int64_t sig = wlen + a.nt - 1;   // the channel's output is sig samples long
    // one sample a lane and trip.  Four at a time, each step for the four together (four independent chains
    // through sincospi, log and sqrt), measured slower: 2.50 ms against 1.72 ms at 65,536 frames (DESIGN s5)
#pragma unroll 1
    for (int k = 0; k < TX_RUN; ++k) {
        const int jj = lane + 64 * k;
        const int64_t i = i0 + jj, m = m0 + jj;
        if (i >= clen) break;
        double2 v = make_double2(0.0, 0.0);
        if (any && m >= 0 && m < sig) {
            v = T[tx_slot(jj)];
            if (c.rot) v = tx_cmul(v, tx_rotor(c.e, (double)(m - TX_FIELD * a.chan_field)));
        }
        if (c.noisy) {
            const double2 w = tx_noise(c.key, (uint64_t)i, c.sg);
            v = make_double2(w.x + v.x, w.y + v.y);
        }
        if (c.bad) v = make_double2(__builtin_nan(""), __builtin_nan(""));
        st2_nt(out, i, v);
    }
    wave_lds_sync();   // the next tile's sums go where these were read
}

// ---------------------------------------------------------------- kernels
__global__ __launch_bounds__(64) void modulate_kernel(TxArgs a)
{
    __shared__ double2 buf[TX_WAVE_SLOTS];
    __shared__ double2 T[TX_TILE_SLOTS];
    const int lane = threadIdx.x;
    const int S = a.field * TX_FIELD + a.nb * TX_BLOCK;
#pragma unroll 1
    for (int64_t f = blockIdx.x; f < a.n; f += gridDim.x) {
        tx_modulate_frame(a, f, lane, T, buf);
        double *row = a.out + 2 * (f * a.os);
        for (int r = lane; r < S; r += 64) st2_nt(row, r, buf[tx_slot(r)]);
        wave_lds_sync();
    }
}

__global__ __launch_bounds__(64) void channel_kernel(TxArgs a)
{
    __shared__ double2 buf[TX_STAGE_SLOTS];
    __shared__ double2 T[TX_TILE_SLOTS];
    const int lane = threadIdx.x;
#pragma unroll 1
    for (int64_t f = blockIdx.x; f < a.n; f += gridDim.x) {
        const double *row = a.wave + 2 * (f * a.ws);
        double z = 0.0;   // +0, or NaN when one of the frame's clean samples is not finite
#pragma unroll 4
        for (int64_t m = lane; m < a.wlen; m += 64) {
            const double2 s = ld2(row, m);
            z = fma(s.x, 0.0, fma(s.y, 0.0, z));
        }
        const TxFrame c = tx_frame(a, f, lane, z != 0.0);
        double *out = a.out + 2 * (f * a.os);
#pragma unroll 1
        for (int64_t i0 = 0; i0 < a.olen; i0 += TX_TILE) {
            const int64_t mbase = i0 - c.delay - TX_HALO;
            if (mbase + TX_TILE + TX_HALO > 0 && mbase < a.wlen) {
                for (int r = lane; r < TX_TILE + TX_HALO; r += 64) {
                    const int64_t m = mbase + r;
                    if (m >= 0 && m < a.wlen) buf[tx_slot(r)] = ld2(row, m);
                }
            }
            wave_lds_sync();
            tx_channel_tile<false>(a, c, buf, mbase, a.wlen, T, i0, a.olen, out, lane);
        }
    }
}

__global__ __launch_bounds__(64) void transmit_kernel(TxArgs a)
{
    __shared__ double2 buf[TX_WAVE_SLOTS];
    __shared__ double2 T[TX_TILE_SLOTS];
    const int lane = threadIdx.x;
    const int S = a.field * TX_FIELD + a.nb * TX_BLOCK;
#pragma unroll 1
    for (int64_t f = blockIdx.x; f < a.n; f += gridDim.x) {
        tx_modulate_frame(a, f, lane, T, buf);
        double z = 0.0;
        for (int r = lane; r < S; r += 64) {
            const double2 s = buf[tx_slot(r)];
            z = fma(s.x, 0.0, fma(s.y, 0.0, z));
        }
        const TxFrame c = tx_frame(a, f, lane, z != 0.0);
        double *out = a.out + 2 * (f * a.os);
#pragma unroll 1
        for (int64_t i0 = 0; i0 < a.olen; i0 += TX_TILE) tx_channel_tile<false>(a, c, buf, 0, S, T, i0, a.olen, out, lane);
    }
}

// The time-varying pair: the static kernels with the knots' scan in the guard and tx_channel_tile<true>.  Where a
// frame's outputs lie in TX_KSEG segments or fewer (a full packet from a period of 42 on) they are staged once a
// frame (kn.once, decided by the launcher, which sizes K for it), else under every tile.
__device__ __forceinline__ TxSegs tx_frame_knots(const TxKnots &kn, int nt, int64_t f, int64_t wlen, int lane, double2 *K)
{
    TxSegs v{&kn, K, f, 0, 0, false};
    const int64_t nseg = (wlen + nt - 2) / kn.period + 1;   // tx_knot_rows' `all`
    if (kn.once) {
        v.once = true;
        v.nseg = (int)nseg;
        tx_stage_knots(kn, nt, f, 0, v.nseg, lane, K);
    }
    return v;
}

__global__ __launch_bounds__(64) void channel_tv_kernel(TxTvArgs g)
{
    __shared__ double2 buf[TX_STAGE_SLOTS];
    __shared__ double2 T[TX_TILE_SLOTS];
    extern __shared__ double2 K[];   // tx_knot_rows(...) rows
    const TxArgs &a = g.a;
    const int lane = threadIdx.x;
#pragma unroll 1
    for (int64_t f = blockIdx.x; f < a.n; f += gridDim.x) {
        const double *row = a.wave + 2 * (f * a.ws);
        double z = tx_knots_scan(g.k, a.nt, f, lane);
#pragma unroll 4
        for (int64_t m = lane; m < a.wlen; m += 64) {
            const double2 s = ld2(row, m);
            z = fma(s.x, 0.0, fma(s.y, 0.0, z));
        }
        const TxFrame c = tx_frame(a, f, lane, z != 0.0);
        const TxSegs v = tx_frame_knots(g.k, a.nt, f, a.wlen, lane, K);
        double *out = a.out + 2 * (f * a.os);
#pragma unroll 1
        for (int64_t i0 = 0; i0 < a.olen; i0 += TX_TILE) {
            const int64_t mbase = i0 - c.delay - TX_HALO;
            if (mbase + TX_TILE + TX_HALO > 0 && mbase < a.wlen) {
                for (int r = lane; r < TX_TILE + TX_HALO; r += 64) {
                    const int64_t m = mbase + r;
                    if (m >= 0 && m < a.wlen) buf[tx_slot(r)] = ld2(row, m);
                }
            }
            wave_lds_sync();
            tx_channel_tile<true>(a, c, buf, mbase, a.wlen, T, i0, a.olen, out, lane, v);
        }
    }
}

__global__ __launch_bounds__(64) void transmit_tv_kernel(TxTvArgs g)
{
    __shared__ double2 buf[TX_WAVE_SLOTS];
    __shared__ double2 T[TX_TILE_SLOTS];
    extern __shared__ double2 K[];   // tx_knot_rows(...) rows
    const TxArgs &a = g.a;
    const int lane = threadIdx.x;
    const int S = a.field * TX_FIELD + a.nb * TX_BLOCK;
#pragma unroll 1
    for (int64_t f = blockIdx.x; f < a.n; f += gridDim.x) {
        tx_modulate_frame(a, f, lane, T, buf);
        double z = tx_knots_scan(g.k, a.nt, f, lane);
        for (int r = lane; r < S; r += 64) {
            const double2 s = buf[tx_slot(r)];
            z = fma(s.x, 0.0, fma(s.y, 0.0, z));
        }
        const TxFrame c = tx_frame(a, f, lane, z != 0.0);
        const TxSegs v = tx_frame_knots(g.k, a.nt, f, S, lane, K);
        double *out = a.out + 2 * (f * a.os);
#pragma unroll 1
        for (int64_t i0 = 0; i0 < a.olen; i0 += TX_TILE)
            tx_channel_tile<true>(a, c, buf, 0, S, T, i0, a.olen, out, lane, v);
    }
}

static dim3 tx_grid(int64_t n) { return dim3((uint32_t)chain_grid(n, TX_GRID_CAP)); }

int launch_modulate(const TxArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    hipLaunchKernelGGL(modulate_kernel, tx_grid(a.n), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

int launch_channel(const TxArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    hipLaunchKernelGGL(channel_kernel, tx_grid(a.n), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

int launch_transmit(const TxArgs &a, void *stream)
{
    if (a.n <= 0) return WCE_OK;
    hipLaunchKernelGGL(transmit_kernel, tx_grid(a.n), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

// The rows of knot LDS a call over waveforms of wlen samples needs, and whether they hold a frame's segments all at
// once (g.k.once): every segment an output lies in where those are TX_KSEG or fewer, else the segments under a tile
static size_t tx_knot_rows(TxTvArgs &g, int64_t wlen)
{
    const int64_t all = (wlen + g.a.nt - 2) / g.k.period + 1, tile = (TX_TILE - 1) / g.k.period + 2;
    g.k.once = WCE_TX_KNOT_ONCE && all <= TX_KSEG;
    const int64_t rows = g.k.once || all < tile ? all : tile;
    return (size_t)rows * tx_krow(g.a.nt) * sizeof(double2);
}

int launch_channel_tv(const TxTvArgs &a, void *stream)
{
    if (a.a.n <= 0) return WCE_OK;
    TxTvArgs g = a;
    const size_t lds = tx_knot_rows(g, g.a.wlen);
    hipLaunchKernelGGL(channel_tv_kernel, tx_grid(g.a.n), dim3(64), lds, (hipStream_t)stream, g);
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

int launch_transmit_tv(const TxTvArgs &a, void *stream)
{
    if (a.a.n <= 0) return WCE_OK;
    TxTvArgs g = a;
    const size_t lds = tx_knot_rows(g, g.a.field * TX_FIELD + g.a.nb * TX_BLOCK);
    hipLaunchKernelGGL(transmit_tv_kernel, tx_grid(g.a.n), dim3(64), lds, (hipStream_t)stream, g);
    return hipGetLastError() == hipSuccess ? WCE_OK : WCE_EHIP;
}

}  // namespace wce
