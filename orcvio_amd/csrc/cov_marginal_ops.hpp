// cov_marginal_ops.hpp -- k_cov_marginal: a small congruence of a sub-block of the device-resident covariance, stored into
// host-coherent pinned memory (orcvio_msckf_cov_get_marginal / _marginal_submit, capi_cov.inc).
//
// ONE launch of ONE workgroup, FP64, no wait on anything and no device-wide counter: it reads P where the stream has brought it and
// writes nothing resident.  With k = n_idx:
//   P_m [k][k]  = P[idx[i]][idx[j]]           gathered into LDS as it stands (nothing symmetrised, nothing examined)
//   Y   [m][k]  = T P_m                       Y(i, j)   = sum_l T(i, l) P_m(l, j),  l = 0 .. k-1 ascending, one FMA chain
//   out [m][m]  = Y T^T                       out(i, j) = sum_l Y(i, l) T(j, l),    l = 0 .. k-1 ascending, one FMA chain
// m == 0 stores P_m itself.  An element is the work of one lane and the order of its sum is a function of (k, m) alone: the same input
// twice gives the same bits.  Each sum has k terms, so |out - exact| <= (2 k + O(1)) 2^-53 (|T| |P_m| |T|^T) componentwise.
// LDS: P_m, T and Y with an odd row stride (the second product reads T by columns of lanes) -- at 64 x 64 three times 64 x 65 doubles,
// 97.5 KB of dynamic LDS: beyond the 64 KB a kernel gets without asking (cov_marginal_lds_bytes; the opt-in is set at create).
// Publication as k_finish_pub / k_triangulate / k_cov_change_anchors do it: the results, a system-scope fence by the lanes that stored
// them, a workgroup barrier, then the sequence word the host spins on.
#pragma once
#include <hip/hip_runtime.h>

#include "host/cov_marginal_spec.hpp"

namespace orcvio_amd {

enum { COV_MARGINAL_THREADS = 256 };
struct CovMarginalIdx { int v[MARGINAL_MAX]; };   // (travels as a kernel argument: 256 bytes)
struct CovMarginalArgs {
    const double* P; int n;        // the resident covariance [n][n]
    int k, m;                      // n_idx; rows of T (0: the gather alone)
    const double* T;               // device staging [m][k] row-major
    double* out;                   // host-coherent result block [m ? m : k][m ? m : k]
    unsigned long long* out_seq; unsigned long long seq;   // stored behind the block (system scope)
    CovMarginalIdx idx;
};
static inline int cov_marginal_ld(int k) { return k | 1; }
static inline size_t cov_marginal_lds_bytes(int k, int m) {
    return sizeof(double) * (size_t)cov_marginal_ld(k) * (size_t)(k + 2 * m);
}

__global__ __launch_bounds__(COV_MARGINAL_THREADS) void k_cov_marginal(CovMarginalArgs a) {
    extern __shared__ double s_marg[];
    const int t = threadIdx.x, k = a.k, m = a.m, ld = k | 1;
    double* sP = s_marg;              // [k][ld]
    double* sT = sP + k * ld;         // [m][ld]
    double* sY = sT + m * ld;         // [m][ld]
    if (m == 0) {   // the gather: bit copies, straight to the result block
        for (int e = t; e < k * k; e += COV_MARGINAL_THREADS) {
            const int i = e / k, j = e - i * k;
            a.out[e] = a.P[(size_t)a.idx.v[i] * a.n + a.idx.v[j]];
        }
    } else {
        for (int e = t; e < k * k; e += COV_MARGINAL_THREADS) {
            const int i = e / k, j = e - i * k;
            sP[i * ld + j] = a.P[(size_t)a.idx.v[i] * a.n + a.idx.v[j]];
        }
        for (int e = t; e < m * k; e += COV_MARGINAL_THREADS) {
            const int i = e / k, j = e - i * k;
            sT[i * ld + j] = a.T[e];
        }
        __syncthreads();
        for (int e = t; e < m * k; e += COV_MARGINAL_THREADS) {
            const int i = e / k, j = e - i * k;
            double acc = 0.0;
            for (int l = 0; l < k; ++l) acc = fma(sT[i * ld + l], sP[l * ld + j], acc);
            sY[i * ld + j] = acc;
        }
        __syncthreads();
        for (int e = t; e < m * m; e += COV_MARGINAL_THREADS) {
            const int i = e / m, j = e - i * m;
            double acc = 0.0;
            for (int l = 0; l < k; ++l) acc = fma(sY[i * ld + l], sT[j * ld + l], acc);
            a.out[e] = acc;
        }
    }
    __threadfence_system();   // (every lane that stored a result: its stores are out before the barrier lets the word go)
    __syncthreads();
    if (t == 0) __hip_atomic_store(a.out_seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace orcvio_amd
