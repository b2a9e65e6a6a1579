// wce_front_body.h -- the body of front_kernel<PRE>, front_cfo_kernel<PRE> and
// front_at_kernel<PRE> (wce_front.hip), included inside each: `a` is the
// kernel's FrontArgs, PRE its template parameter, CFO and AT constexpr bools
// of the including kernel (AT: each frame starts at a.start[f] of its capture
// window; it implies CFO).  Not a header in its own right.
    __shared__ double2 lds[FE_WAVES][FE_UNITS][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 3, j = lane & 7;
    double2 *T = lds[w][g];
    const double2 *src = reinterpret_cast<const double2 *>(a.src);
    double2 *dst = reinterpret_cast<double2 *>(a.dst);
    constexpr bool NT = !PRE, STAGED = !PRE;
    double2 tw[8];
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) tw[k1] = kW64[(j * k1) & 63];
    const uint32_t stride = gridDim.x * FE_WAVES * FE_UNITS;
    for (uint32_t u0 = (blockIdx.x * FE_WAVES + w) * FE_UNITS; u0 < a.n_units; u0 += stride) {
        const bool live = u0 + g < a.n_units;
        const uint32_t u = live ? u0 + g : a.n_units - 1;
        const uint32_t f = u / a.nb, b = u - f * a.nb;
        const double2 *x = src + (int64_t)f * a.ps + a.off + (int64_t)b * 80 + j;
        bool ok = true;           // AT: the frame has a start and every sample it reads lies in its window
        if constexpr (AT) {       // one 4-B load per unit; a frame that is not ok reads its window's head
            const int64_t s = a.start[f], lo = s + a.off;
            ok = s >= 0 && lo >= 0 && lo + a.span <= a.win;
            x = src + (int64_t)f * a.ps + (ok ? lo + (int64_t)b * 80 : 0) + j;
        }
        double2 v[8];
        double s2 = 0.0;
        double e = 0.0;           // CFO: the frame's offset, cycles per sample
        if constexpr (AT) {       // null cfo: offset 0, the plain call's bits
            if (a.cfo && !(PRE && a.est)) e = a.cfo[f];
            if (!ok) e = __builtin_nan("");
        } else if constexpr (CFO) {   // one 8-B load at the frame's address, in flight with the samples
            if (!(PRE && a.est)) e = a.cfo[f];
        }
        if constexpr (PRE) {      // WiFi_RX.m:24-30: p2 = x[0..64), p1 = x[64..128)
            double2 p2[8], p1[8];
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) { p2[n1] = fe_ld<NT>(x + 8 * n1); p1[n1] = fe_ld<NT>(x + 64 + 8 * n1); }
            if constexpr (CFO) {
                // z: +0, or NaN when one of the frame's 128 samples is not finite
                double z = 0.0;
                if constexpr (AT) z = ok ? 0.0 : __builtin_nan("");
#pragma unroll
                for (int n1 = 0; n1 < 8; ++n1)
                    z = fma(p2[n1].x, 0.0, fma(p2[n1].y, 0.0, fma(p1[n1].x, 0.0, fma(p1[n1].y, 0.0, z))));
                if (a.est) {
                    // c = sum p1 conj(p2) over the 64 pairs; e = arg c / (2 pi 64).  + z: NaN marks the
                    // frame, and an all-zero field gives c = (+0, +-0), e = +-0 whatever its zeros' signs
                    double2 c = make_double2(0.0, 0.0);
#pragma unroll
                    for (int n1 = 0; n1 < 8; ++n1) {
                        c.x = fma(p1[n1].x, p2[n1].x, fma(p1[n1].y, p2[n1].y, c.x));
                        c.y = fma(p1[n1].y, p2[n1].x, fma(-p1[n1].x, p2[n1].y, c.y));
                    }
                    c.x += z;
                    c = cadd(c, shfl_xor_c(c, 1));
                    c = cadd(c, shfl_xor_c(c, 2));
                    c = cadd(c, shfl_xor_c(c, 4));   // the same bits on the frame's 8 lanes
                    e = atan2(c.y, c.x) * 0x1.45f306dc9c883p-9;   // 1 / (128 pi)
                    if (live && j == 0) a.cfo[f] = e;
                } else if (!AT || a.cfo) {   // AT without cfo: samples pass as the plain call passes them
                    z += __shfl_xor(z, 1, 64);
                    z += __shfl_xor(z, 2, 64);
                    z += __shfl_xor(z, 4, 64);
                    e += z;
                }
                // p2 starts at sample a.n0 (-128), p1 64 samples later
                const double2 r2 = cfo_rotor(e, (double)(a.n0 + j)), step = cfo_rotor(e, 8.0);
                const bool rot = e != 0.0;
                cfo_derotate(p2, r2, step, rot);
                cfo_derotate(p1, cmul(r2, cfo_rotor(e, 64.0)), step, rot);
            }
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) {
                v[n1] = cscale(cadd(p1[n1], p2[n1]), 0.5);
                const double2 d = csub(p2[n1], p1[n1]);
                s2 += d.x * d.x + d.y * d.y;
            }
        } else {
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) v[n1] = fe_ld<NT>(x + 8 * n1);
            if constexpr (CFO)    // the lane's first sample: a.n0 (sample_offset + 16) + 80 b + j
                cfo_derotate(v, cfo_rotor(e, (double)(a.n0 + (int64_t)b * 80 + j)), cfo_rotor(e, 8.0), e != 0.0);
        }
        // stage 1 (lane = n2): DFT over n1, then W64^(n2 k1)
        dft8(v);
#pragma unroll
        for (int k1 = 1; k1 < 8; ++k1) {
            if constexpr (CFO) v[k1] = cmul_tw(v[k1], tw[k1]);
            else v[k1] = cmul(v[k1], tw[k1]);
        }
        // transpose: element (n2, k1) at n2 * 8 + (k1 ^ n2)
#pragma unroll
        for (int k1 = 0; k1 < 8; ++k1) T[j * 8 + (k1 ^ j)] = v[k1];
        wave_lds_sync();
#pragma unroll
        for (int n2 = 0; n2 < 8; ++n2) v[n2] = T[n2 * 8 + (j ^ n2)];
        wave_lds_sync();
        // stage 2 (lane = k1): DFT over n2 -> bin k = k1 + 8 k2
        dft8(v);
        if constexpr (STAGED) {
            // stage the 8 x 53 bins in LDS, then store them as one run per wave
            // (contiguous when consecutive blocks are adjacent, block_stride 53)
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2) T[(j + 8 * k2 + 26) & 63] = v[k2];
            wave_lds_sync();
#pragma unroll
            for (int t = 0; t < (FE_UNITS * NSC + 63) / 64; ++t) {
                const int e = lane + 64 * t;
                const int ug = e / NSC, i = e - ug * NSC;
                const uint32_t uu = u0 + ug;
                if (e < FE_UNITS * NSC && uu < a.n_units) {
                    const uint32_t ff = uu / a.nb, bb = uu - ff * a.nb;
                    fe_st<NT>(dst + (int64_t)ff * a.fs + (int64_t)bb * a.bs + i, lds[w][ug][i]);
                }
            }
            wave_lds_sync();
        } else {
            double2 *y = dst + (int64_t)f * a.fs + (int64_t)b * a.bs;
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2) {
                const int i = (j + 8 * k2 + 26) & 63;   // circshift(., 26), keep 1:53
                if (live && i < NSC) fe_st<NT>(y + i, v[k2]);
            }
        }
        if constexpr (PRE) {
            if (a.ow2) {
                s2 += __shfl_xor(s2, 1, 64);
                s2 += __shfl_xor(s2, 2, 64);
                s2 += __shfl_xor(s2, 4, 64);
                if (live && j == 0) a.ow2[f] = s2 / 128.0;   // 2 K, K = 64
            }
        }
    }
