// wce_api_check.h -- what the two files of the C ABI (wce_api.cpp: contexts, the estimator, plans, runtime
// helpers; wce_chain_api.cpp: the receive and transmit chain) share: the refusal, the device guard, a context's
// device and CU count, and the predicates argument checks are written in.  Included by those two files only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "wce_internal.h"

// refuse: the text goes to wce_last_error() (a copy: a temporary will do), the code back to the caller
static inline int fail(int code, const char *what) { return wce::api_fail(code, what); }

namespace {   // internal to each of the two files: no symbol of it leaves the library
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int d)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d) (void)hipSetDevice(d);
    }
    ~DeviceGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};
}  // namespace

namespace wce {
// wce_api.cpp, beside ctx_device (wce_internal.h): the context's CU count, and the estimator's check of a
// wce_frames (its messages come without a call's name)
int ctx_cus(const wce_ctx *c);
int api_check_frames(const wce_frames *in, bool need_blocks);
}  // namespace wce

static inline bool misaligned(const void *p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; }

// block stride >= row and, with more than one frame, frame stride >= 14 block strides + one row
static inline bool strides_hold(int64_t n, int64_t fs, int64_t bs, int64_t row)
{
    return bs >= row && (n <= 1 || fs >= (wce::NBLK - 1) * bs + row);
}

// a frame or packet count the 1-D grids take: 0 .. 2^31 - 1
static inline bool count_holds(int64_t n) { return n >= 0 && n <= 0x7fffffffll; }

static inline bool positive_finite(double x) { return x > 0.0 && x * 0.0 == 0.0; }

// thresholds and weights: 0 <= x <= 1, which no NaN is
static inline bool in_unit(double x) { return x >= 0.0 && x <= 1.0; }

// the constellation scale K: the doubles nearest to 1 / sqrt(1, 2, 10, 42); 0 for an unknown modulation
static inline double mod_K(int32_t modulation)
{
    switch (modulation) {
    case WCE_MOD_BPSK: return 1.0;
    case WCE_MOD_QPSK: return 0.70710678118654752440;
    case WCE_MOD_QAM16: return 0.31622776601683793320;
    case WCE_MOD_QAM64: return 0.15430334996209191026;
    default: return 0.0;
    }
}
