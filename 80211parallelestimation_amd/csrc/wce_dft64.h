// wce_dft64.h -- the 64-point DFT's pieces shared by the front end (wce_front.hip) and the
// transmitter (wce_transmit.hip, which runs the same 8 x 8 Cooley-Tukey backwards): the twiddle
// table, the in-register 8-point DFT, the exact-phase rotor and the twiddle product.
#pragma once
#include <hip/hip_runtime.h>
#include "wce_device.h"

namespace wce {

// W64^m = exp(-2 pi i m / 64), correctly rounded (mpmath, 40 digits)
static __constant__ double2 kW64[64] = {
    {0x1.0000000000000p+0, 0x0.0p+0}, {0x1.fd88da3d12526p-1, -0x1.917a6bc29b42cp-4},
    {0x1.f6297cff75cb0p-1, -0x1.8f8b83c69a60bp-3}, {0x1.e9f4156c62ddap-1, -0x1.294062ed59f06p-2},
    {0x1.d906bcf328d46p-1, -0x1.87de2a6aea963p-2}, {0x1.c38b2f180bdb1p-1, -0x1.e2b5d3806f63bp-2},
    {0x1.a9b66290ea1a3p-1, -0x1.1c73b39ae68c8p-1}, {0x1.8bc806b151741p-1, -0x1.44cf325091dd6p-1},
    {0x1.6a09e667f3bcdp-1, -0x1.6a09e667f3bcdp-1}, {0x1.44cf325091dd6p-1, -0x1.8bc806b151741p-1},
    {0x1.1c73b39ae68c8p-1, -0x1.a9b66290ea1a3p-1}, {0x1.e2b5d3806f63bp-2, -0x1.c38b2f180bdb1p-1},
    {0x1.87de2a6aea963p-2, -0x1.d906bcf328d46p-1}, {0x1.294062ed59f06p-2, -0x1.e9f4156c62ddap-1},
    {0x1.8f8b83c69a60bp-3, -0x1.f6297cff75cb0p-1}, {0x1.917a6bc29b42cp-4, -0x1.fd88da3d12526p-1},
    {0x0.0p+0, -0x1.0000000000000p+0}, {-0x1.917a6bc29b42cp-4, -0x1.fd88da3d12526p-1},
    {-0x1.8f8b83c69a60bp-3, -0x1.f6297cff75cb0p-1}, {-0x1.294062ed59f06p-2, -0x1.e9f4156c62ddap-1},
    {-0x1.87de2a6aea963p-2, -0x1.d906bcf328d46p-1}, {-0x1.e2b5d3806f63bp-2, -0x1.c38b2f180bdb1p-1},
    {-0x1.1c73b39ae68c8p-1, -0x1.a9b66290ea1a3p-1}, {-0x1.44cf325091dd6p-1, -0x1.8bc806b151741p-1},
    {-0x1.6a09e667f3bcdp-1, -0x1.6a09e667f3bcdp-1}, {-0x1.8bc806b151741p-1, -0x1.44cf325091dd6p-1},
    {-0x1.a9b66290ea1a3p-1, -0x1.1c73b39ae68c8p-1}, {-0x1.c38b2f180bdb1p-1, -0x1.e2b5d3806f63bp-2},
    {-0x1.d906bcf328d46p-1, -0x1.87de2a6aea963p-2}, {-0x1.e9f4156c62ddap-1, -0x1.294062ed59f06p-2},
    {-0x1.f6297cff75cb0p-1, -0x1.8f8b83c69a60bp-3}, {-0x1.fd88da3d12526p-1, -0x1.917a6bc29b42cp-4},
    {-0x1.0000000000000p+0, 0x0.0p+0}, {-0x1.fd88da3d12526p-1, 0x1.917a6bc29b42cp-4},
    {-0x1.f6297cff75cb0p-1, 0x1.8f8b83c69a60bp-3}, {-0x1.e9f4156c62ddap-1, 0x1.294062ed59f06p-2},
    {-0x1.d906bcf328d46p-1, 0x1.87de2a6aea963p-2}, {-0x1.c38b2f180bdb1p-1, 0x1.e2b5d3806f63bp-2},
    {-0x1.a9b66290ea1a3p-1, 0x1.1c73b39ae68c8p-1}, {-0x1.8bc806b151741p-1, 0x1.44cf325091dd6p-1},
    {-0x1.6a09e667f3bcdp-1, 0x1.6a09e667f3bcdp-1}, {-0x1.44cf325091dd6p-1, 0x1.8bc806b151741p-1},
    {-0x1.1c73b39ae68c8p-1, 0x1.a9b66290ea1a3p-1}, {-0x1.e2b5d3806f63bp-2, 0x1.c38b2f180bdb1p-1},
    {-0x1.87de2a6aea963p-2, 0x1.d906bcf328d46p-1}, {-0x1.294062ed59f06p-2, 0x1.e9f4156c62ddap-1},
    {-0x1.8f8b83c69a60bp-3, 0x1.f6297cff75cb0p-1}, {-0x1.917a6bc29b42cp-4, 0x1.fd88da3d12526p-1},
    {0x0.0p+0, 0x1.0000000000000p+0}, {0x1.917a6bc29b42cp-4, 0x1.fd88da3d12526p-1},
    {0x1.8f8b83c69a60bp-3, 0x1.f6297cff75cb0p-1}, {0x1.294062ed59f06p-2, 0x1.e9f4156c62ddap-1},
    {0x1.87de2a6aea963p-2, 0x1.d906bcf328d46p-1}, {0x1.e2b5d3806f63bp-2, 0x1.c38b2f180bdb1p-1},
    {0x1.1c73b39ae68c8p-1, 0x1.a9b66290ea1a3p-1}, {0x1.44cf325091dd6p-1, 0x1.8bc806b151741p-1},
    {0x1.6a09e667f3bcdp-1, 0x1.6a09e667f3bcdp-1}, {0x1.8bc806b151741p-1, 0x1.44cf325091dd6p-1},
    {0x1.a9b66290ea1a3p-1, 0x1.1c73b39ae68c8p-1}, {0x1.c38b2f180bdb1p-1, 0x1.e2b5d3806f63bp-2},
    {0x1.d906bcf328d46p-1, 0x1.87de2a6aea963p-2}, {0x1.e9f4156c62ddap-1, 0x1.294062ed59f06p-2},
    {0x1.f6297cff75cb0p-1, 0x1.8f8b83c69a60bp-3}, {0x1.fd88da3d12526p-1, 0x1.917a6bc29b42cp-4}};

// in-register 8-point DFT, radix-2 (W8^1 = c(1 - i), W8^2 = -i, W8^3 = -c(1 + i))
__device__ __forceinline__ void dft8(double2 (&x)[8])
{
    const double c = 0x1.6a09e667f3bcdp-1;   // sqrt(2)/2
    const double2 b0 = cadd(x[0], x[4]), b1 = csub(x[0], x[4]), b2 = cadd(x[2], x[6]), b3 = csub(x[2], x[6]);
    const double2 b4 = cadd(x[1], x[5]), b5 = csub(x[1], x[5]), b6 = cadd(x[3], x[7]), b7 = csub(x[3], x[7]);
    const double2 e0 = cadd(b0, b2), e2 = csub(b0, b2);
    const double2 e1 = make_double2(b1.x + b3.y, b1.y - b3.x), e3 = make_double2(b1.x - b3.y, b1.y + b3.x);
    const double2 o0 = cadd(b4, b6), o2 = csub(b4, b6);
    const double2 o1 = make_double2(b5.x + b7.y, b5.y - b7.x), o3 = make_double2(b5.x - b7.y, b5.y + b7.x);
    const double2 t1 = make_double2(c * (o1.x + o1.y), c * (o1.y - o1.x));
    const double2 t2 = make_double2(o2.y, -o2.x);
    const double2 t3 = make_double2(c * (o3.y - o3.x), -c * (o3.x + o3.y));
    x[0] = cadd(e0, o0); x[4] = csub(e0, o0);
    x[1] = cadd(e1, t1); x[5] = csub(e1, t1);
    x[2] = cadd(e2, t2); x[6] = csub(e2, t2);
    x[3] = cadd(e3, t3); x[7] = csub(e3, t3);
}

// exp(-2 pi i e n).  The phase e n (cycles) is reduced before sincospi sees it:
// hi + lo = e n exactly, hi - rint(hi) is exact, so the rotor's error does not
// grow with |e n|.  Contraction is off: fusing e * n into the subtraction would
// count lo twice.  A non-finite e gives (NaN, NaN).
__device__ __forceinline__ double2 cfo_rotor(double e, double n)
{
#pragma clang fp contract(off)
    const double hi = e * n, lo = fma(e, n, -hi);
    const double t = (hi - rint(hi)) + lo;
    double s, c;
    sincospi(-2.0 * t, &s, &c);
    return make_double2(c, s);
}
// v tw with the roundings spelled out: a.y b.y and a.x b.y round, the other two products fuse.  These
// are the plain builds' roundings; left to contraction, the compiler picks per build which product of
// each pair to fuse, and a CFO build given a zero offset would part from the plain build's bits.
__device__ __forceinline__ double2 cmul_tw(double2 a, double2 b)
{
#pragma clang fp contract(off)
    return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.y, b.x, a.x * b.y));
}

}  // namespace wce
