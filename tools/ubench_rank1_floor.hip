// ubench_rank1_floor.hip -- the floor of mmse_rank1_kernel's access pattern
// (profiles/rank1q_floor.txt): exactly the headline's loads and stores per
// 16-lane row, and no sums.  Buffers laid out like bench.py's: tx and rx frames
// 12,720 B apart (15 blocks x 53 complex fp64, block 0 read), one shared 848-B
// u, H rows contiguous (848 B).  Lane i of a row moves subcarriers i, i + 16,
// i + 32 and (lanes 0..4) i + 48 of tx, rx and u -- all eleven loads issued
// before the first use, tx / rx first -- and stores H = x + rx + u, so that
// nothing is optimised away.  One unit per row, the grid covers the batch;
// rows per workgroup follow blockDim.x (64, 128, 256 threads).
// k_floor<true> issues them row by row instead -- tx, u, rx, the headline's order since
// profiles/rank1r_* -- so that the floor describes the kernel's own load order.
// Medians of five timings of 20 launches at 16,384, 32,768, 65,536 and 1,048,576 frames
// (profiles/rank1s_floor.txt: the gap to the kernel against the batch size).
// build: hipcc -O3 --offload-arch=gfx950 tools/ubench_rank1_floor.hip -o tools/ubench_rank1_floor
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <unistd.h>
#include <algorithm>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

typedef double v2d __attribute__((ext_vector_type(2)));
constexpr int NSC = 53, FS = 795;   // complex elements per row / per frame

template <bool ROWS>
__global__ __launch_bounds__(256, 4) void k_floor(const v2d *__restrict__ tx, const v2d *__restrict__ rx,
                                                  const v2d *__restrict__ u, v2d *__restrict__ H, uint32_t n)
{
    const int i = threadIdx.x & 15;
    const uint32_t rpw = blockDim.x >> 4;
    const uint32_t f = blockIdx.x * rpw + (threadIdx.x >> 4);
    if (f >= n) return;   // whole 16-lane rows leave before any address is formed
    const int64_t base = (int64_t)f * FS + i;
    const v2d zero = {0.0, 0.0};
    v2d x[4], r[4], c[4];
    x[3] = r[3] = c[3] = zero;
    if (ROWS) {
#pragma unroll
        for (int m = 0; m < 3; ++m) x[m] = tx[base + 16 * m];
        if (i < NSC - 48) x[3] = tx[base + 48];
#pragma unroll
        for (int m = 0; m < 3; ++m) c[m] = u[i + 16 * m];
        if (i < NSC - 48) c[3] = u[i + 48];
#pragma unroll
        for (int m = 0; m < 3; ++m) r[m] = rx[base + 16 * m];
        if (i < NSC - 48) r[3] = rx[base + 48];
    } else {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            x[m] = tx[base + 16 * m];
            r[m] = rx[base + 16 * m];
        }
        if (i < NSC - 48) {
            x[3] = tx[base + 48];
            r[3] = rx[base + 48];
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) c[m] = u[i + 16 * m];
        if (i < NSC - 48) c[3] = u[i + 48];
    }
    const int64_t hb = (int64_t)f * NSC + i;
#pragma unroll
    for (int m = 0; m < 4; ++m)
        if (i + 16 * m < NSC) H[hb + 16 * m] = x[m] + r[m] + c[m];
}

int main()
{
    alarm(120);   // the run's own time limit
    const int64_t nmax = 1 << 20;
    v2d *tx, *rx, *u, *H;
    CK(hipMalloc(&tx, nmax * FS * 16));
    CK(hipMalloc(&rx, nmax * FS * 16));
    CK(hipMalloc(&u, 64 * 16));
    CK(hipMalloc(&H, nmax * NSC * 16));
    CK(hipMemset(tx, 0, nmax * FS * 16));
    CK(hipMemset(rx, 0, nmax * FS * 16));
    CK(hipMemset(u, 0, 64 * 16));
    CK(hipMemset(H, 0, nmax * NSC * 16));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const int reps = 20, rounds = 5, wgs[3] = {64, 128, 256};
    for (int64_t n : {(int64_t)16384, (int64_t)32768, (int64_t)65536, nmax}) {
        float t[6][rounds];   // k = 3 * order + workgroup size
        for (int r = 0; r < rounds; ++r) {   // interleaved, like tools/ab_variant.py
            for (int k = 0; k < 6; ++k) {
                const int rpw = wgs[k % 3] / 16;
                const dim3 g((unsigned)((n + rpw - 1) / rpw)), b(wgs[k % 3]);
                auto launch = [&] {
                    if (k < 3) hipLaunchKernelGGL(k_floor<false>, g, b, 0, 0, tx, rx, u, H, (uint32_t)n);
                    else hipLaunchKernelGGL(k_floor<true>, g, b, 0, 0, tx, rx, u, H, (uint32_t)n);
                };
                for (int j = 0; j < 3; ++j) launch();
                CK(hipEventRecord(e0));
                for (int j = 0; j < reps; ++j) launch();
                CK(hipEventRecord(e1));
                CK(hipEventSynchronize(e1));
                CK(hipEventElapsedTime(&t[k][r], e0, e1));
                t[k][r] /= reps;
            }
        }
        for (int k = 0; k < 6; ++k) {
            float s[rounds];
            std::copy(t[k], t[k] + rounds, s);
            std::sort(s, s + rounds);
            const double us = s[rounds / 2] * 1e3;
            printf("floor %8lld frames, %3d threads, %s: median %7.1f us  min %7.1f  %5.2f TB/s of 2,544 B, "
                   "%5.2f TB/s of the 2,770 B counted  (", (long long)n, wgs[k % 3],
                   k < 3 ? "tx / rx alternating, u last" : "tx, u, rx row by row     ", us, s[0] * 1e3,
                   2544.0 * n / (us * 1e-6) / 1e12, 2770.0 * n / (us * 1e-6) / 1e12);
            for (int r = 0; r < rounds; ++r) printf("%s%.1f", r ? ", " : "", t[k][r] * 1e3);
            printf(")\n");
        }
    }
    CK(hipDeviceSynchronize());
    return 0;
}
