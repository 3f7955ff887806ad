// zupt_check_ops.hpp -- k_zupt_check: the reference's zero-velocity test on IMU samples (checkZUPTIMU, src/orcvio.cpp:3129-3323) on the
// device-resident covariance, in the Woodbury form of host/zupt_check_model.hpp.  ONE launch, ONE workgroup of two wavefronts, FP64.
//
//   phase 1  the m = S - 1 <= 127 row blocks are independent: thread i evaluates zupt_check_row -- the header's own function, the
//            arithmetic the host build runs -- for block i; the threads behind m hold zeros.  Threads 0..80 read the marginal's 81
//            entries out of P (both triangles: (P_ij + P_ji) / 2) and test them.
//   phase 2  the 56 sums: a butterfly over the 64 lanes of each wavefront (xor 32, 16, .. 1), then wavefront 0's total + wavefront 1's.
//            The order depends on nothing at all -- a lane without a row adds an exact zero --, so the same input gives the same bits.
//   phase 3  lane 0 of wavefront 0 runs zupt_check_solve (two 9 x 9 Cholesky factorisations, again the header's function) and leaves the
//            verdict: out = chi^2 | c | dt_sum | the limit it compared with, status[0] = status[2] = 0 (accepted) or the reason
//            (ZCHK_*: rejected, not evaluated, or the status block in front of it already set).
// P is read at 81 places and never written; no other workgroup, no device-wide counter.
#pragma once
#include <hip/hip_runtime.h>

#include "host/zupt_check_model.hpp"

namespace orcvio_amd {

enum { ZCHK_THREADS = 128, ZCHK_REJECTED = 5 };   // (ZCHK_REJECTED: evaluated, and chi^2 > limit or the caller's speed test failed)

struct ZuptCheckArgs {
    const double* P;      // resident covariance [n][n]
    const double* rows;   // [m][ZCHK_ROW]
    double* out;          // [4] out
    int* status;          // [16] out: [0] = [2] (word 2: where an update's commit looks, ZuptArgs::also); the other words stay zero
    const int* also;      // optional: the status block of an armed IMU propagation in front; [2] != 0 refuses the check too
    int n, m;
    int force_reject;     // the host's speed test failed: chi^2 is evaluated and reported all the same
    double limit;         // chi2_multiplier x quantile(6 m)
    double R[9], ba[3], g[3];
    ZuptCheckConsts k;
};

__global__ __launch_bounds__(ZCHK_THREADS) void k_zupt_check(ZuptCheckArgs a) {
    __shared__ double s_sum[2][ZCHK_SUMS];
    __shared__ double s_Pm[81];
    __shared__ int s_bad;
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    if (t == 0) s_bad = 0;
    __syncthreads();
    // ---- phase 1
    double v[ZCHK_SUMS];
    if (t < a.m) zupt_check_row(a.rows + (size_t)t * ZCHK_ROW, a.R, a.ba, a.g, a.k, v);
    else {
#pragma unroll
        for (int e = 0; e < ZCHK_SUMS; ++e) v[e] = 0.0;
    }
    if (t < 81) {
        const int i = zupt_check_state(t / 9), j = zupt_check_state(t % 9);   // (i, j <= 14 < n: the callers refuse n < 22)
        const double u = a.P[(size_t)i * a.n + j], lo = a.P[(size_t)j * a.n + i];
        if (!isfinite(u) || !isfinite(lo)) atomicOr(&s_bad, 1);
        s_Pm[t] = 0.5 * (u + lo);
    }
    // ---- phase 2
#pragma unroll
    for (int e = 0; e < ZCHK_SUMS; ++e) {
        double x = v[e];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if (l == 0) s_sum[w][e] = x;
    }
    __syncthreads();
    // ---- phase 3
    if (t == 0) {
        double sums[ZCHK_SUMS], chi2 = 0.0;
        for (int e = 0; e < ZCHK_SUMS; ++e) sums[e] = s_sum[0][e] + s_sum[1][e];
        int st = ZCHK_OK;
        if (a.also && a.also[2] != 0) st = ZCHK_UPSTREAM;
        else if (s_bad) st = ZCHK_NOT_FINITE;
        else st = zupt_check_solve(s_Pm, sums, a.k, &chi2);
        if (st == ZCHK_OK && (chi2 > a.limit || a.force_reject)) st = ZCHK_REJECTED;
        a.out[0] = chi2; a.out[1] = sums[ZCHK_C]; a.out[2] = sums[ZCHK_DT]; a.out[3] = a.limit;
        a.status[0] = st;
        a.status[2] = st;
    }
}

}  // namespace orcvio_amd
