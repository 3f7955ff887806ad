// imu_ops.hpp -- k_imu_phi_q: the accumulated error-state transition Phi = Phi_S ... Phi_1 and noise Q (Q <- Phi_k Q Phi_k^T + Q_k)
// of one frame's IMU samples (processModel, src/orcvio.cpp:761-798, S <= 128 times per image), from the per-sample records the host
// half left (host/imu_model.hpp: the states before and after every sample).  ONE launch, ONE workgroup of four wavefronts, FP64.
//
//   phase 1  the S pairs are independent: lane i of wavefront w evaluates imu_phi / imu_noise -- the header's own functions, the
//            arithmetic the host build runs -- for sample w C + i (C = ceil(S / 4) <= 32) and leaves the nine 3 x 3 blocks of Phi_k
//            that differ from the identity's and the block-diagonal N_k = G Q_c G^T dt in LDS (105 doubles a sample).
//   phase 2  every wavefront runs its chunk in order on the 15 x 15 block padded to ONE 16 x 16 tile, v_mfma_f64_16x16x4_f64:
//                W = (Q + N_k) Phi_k^T,   Q <- Phi_k W,   Phi <- Phi_k Phi        (12 MFMA a sample)
//            An MFMA result tile (lane l: rows (l >> 4) + 4 r, column l & 15) IS the B operand of the next product, and the A operand of
//            a symmetric tile, so nothing moves between lanes: Q + N_k enters as A by symmetry, Phi_k is read from LDS once as
//            Phi_k[l & 15][4 s + (l >> 4)] and serves as A (Phi_k) and as B (Phi_k^T).
//   phase 3  wavefront 0 combines the (up to) four partial pairs in chunk order, (Phi_b, Q_b) o (Phi_a, Q_a) = (Phi_b Phi_a,
//            Phi_b Q_a Phi_b^T + Q_b); every thread then writes a piece of Phi, Q [22][22] (identity / zero outside the 15 x 15 block,
//            Q symmetrised) and tests it: status[0] = status[2] = 1 if an entry is not finite (the right closed form divides by |w|^2).
// The order of every sum depends on S alone: the same input gives the same bits.  No other workgroup, no device-wide counter.
#pragma once
#include <hip/hip_runtime.h>

#include "msckf_kernels.hpp"
#include "host/imu_model.hpp"

namespace orcvio_amd {

enum { IMU_WAVES = 4, IMU_LDS_STRIDE = IMU_COMPACT };   // (105 doubles: an odd stride, lanes of one sample column spread over the banks)

struct ImuKernArgs {
    const double* recs;   // [S][IMU_REC]
    double* Phi;          // [22][22] out
    double* Q;            // [22][22] out
    int* status;          // [16] out: [0] = [2] = 1 if Phi or Q has a non-finite entry (word 2: where an update's commit looks, info_also);
                          //      the other words stay zero
    int* status_host;     // optional, host-coherent: the same word for the host to read behind the frame's wait (the armed form)
    int S;
    ImuFlags flags;
    double grav[3];
    double qc[12];
};
static inline size_t imu_lds_bytes(int S) { return sizeof(double) * IMU_LDS_STRIDE * (size_t)(IMU_WAVES * ((S + IMU_WAVES - 1) / IMU_WAVES)); }

// offset of Phi_k(i, j) in a sample's compact record, or -1 (one) / -2 (zero): i, j < 16, the padding row / column is the identity's
__device__ __forceinline__ int imu_phi_off(int i, int j) {
    if (i < 9 && j < 15) {
        const int b = imu_block(i / 3, j / 3);
        if (b >= 0) return b * 9 + (i % 3) * 3 + j % 3;
    }
    return i == j ? -1 : -2;
}
// ... and of N_k(i, j) (-2: zero)
__device__ __forceinline__ int imu_noise_off(int i, int j) {
    if (i < 6 && j < 6) return i / 3 == j / 3 ? IMU_COMPACT_N00 + 9 * (i / 3) + (i % 3) * 3 + j % 3 : -2;
    if (i >= 9 && i < 15 && i == j) return IMU_COMPACT_ND + i - 9;
    return -2;
}
__device__ __forceinline__ double imu_pick(const double* c, int off) { return off >= 0 ? c[off] : (off == -1 ? 1.0 : 0.0); }

// one step of the ordered product on a wavefront: (phi, q) <- (pa phi, pa (q + nq) pa^T), pa[s] = Phi_k[l & 15][4 s + (l >> 4)]
__device__ __forceinline__ void imu_combine(const double pa[4], d4 add, d4& phi, d4& q, bool add_before) {
    d4 qn = q;
    if (add_before) qn += add;
    d4 W = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) W = mfma_f64(qn[s], pa[s], W);        // W = (Q + N)^T Phi_k^T  (Q + N symmetric to rounding)
    d4 qo = {0.0, 0.0, 0.0, 0.0};
    if (!add_before) qo = add;
#pragma unroll
    for (int s = 0; s < 4; ++s) qo = mfma_f64(pa[s], W[s], qo);      // Phi_k W (+ Q_b)
    d4 po = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) po = mfma_f64(pa[s], phi[s], po);    // Phi_k Phi
    q = qo;
    phi = po;
}

__global__ __launch_bounds__(64 * IMU_WAVES) void k_imu_phi_q(ImuKernArgs a) {
    extern __shared__ double s_comp[];                 // [IMU_WAVES * C][IMU_LDS_STRIDE]
    __shared__ double s_part[IMU_WAVES][2][256];       // the wavefronts' partial (Phi, Q) tiles, [row][column]
    __shared__ int s_bad;
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const int S = a.S, C = (S + IMU_WAVES - 1) / IMU_WAVES;
    const int k0 = w * C, k1 = k0 + C < S ? k0 + C : S;   // this wavefront's chunk [k0, k1)
    if (t == 0) s_bad = 0;
    // ---- phase 1
    if (k0 + l < k1) {
        const double* rec = a.recs + (size_t)(k0 + l) * IMU_REC;
        double* c = s_comp + (size_t)(k0 + l) * IMU_LDS_STRIDE;
        ImuCompactSink sink{c};
        imu_phi(rec, a.flags, a.grav, sink);
        imu_noise(rec, a.flags, a.qc, c + IMU_COMPACT_N00);
    }
    __syncthreads();
    // ---- phase 2
    const int col = l & 15, g = l >> 4;
    int po[4], no[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) { po[s] = imu_phi_off(col, 4 * s + g); no[s] = imu_noise_off(g + 4 * s, col); }
    d4 phi, q = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) phi[r] = (g + 4 * r == col) ? 1.0 : 0.0;
    for (int k = k0; k < k1; ++k) {
        const double* c = s_comp + (size_t)k * IMU_LDS_STRIDE;
        double pa[4];
        d4 nk;
#pragma unroll
        for (int s = 0; s < 4; ++s) { pa[s] = imu_pick(c, po[s]); nk[s] = imu_pick(c, no[s]); }
        imu_combine(pa, nk, phi, q, true);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        s_part[w][0][(g + 4 * r) * 16 + col] = phi[r];
        s_part[w][1][(g + 4 * r) * 16 + col] = q[r];
    }
    __syncthreads();
    // ---- phase 3
    if (w == 0) {
        for (int b = 1; b < IMU_WAVES && b * C < S; ++b) {
            double pa[4];
            d4 qb;
#pragma unroll
            for (int s = 0; s < 4; ++s) { pa[s] = s_part[b][0][col * 16 + 4 * s + g]; qb[s] = s_part[b][1][(g + 4 * s) * 16 + col]; }
            imu_combine(pa, qb, phi, q, false);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s_part[0][0][(g + 4 * r) * 16 + col] = phi[r];
            s_part[0][1][(g + 4 * r) * 16 + col] = q[r];
        }
    }
    __syncthreads();
    int bad = 0;
    for (int e = t; e < IMU_LEG * IMU_LEG; e += 64 * IMU_WAVES) {
        const int i = e / IMU_LEG, j = e - i * IMU_LEG;
        const bool in = i < IMU_DIM && j < IMU_DIM;
        const double p = in ? s_part[0][0][i * 16 + j] : (i == j ? 1.0 : 0.0);
        const double v = in ? 0.5 * (s_part[0][1][i * 16 + j] + s_part[0][1][j * 16 + i]) : 0.0;
        a.Phi[e] = p;
        a.Q[e] = v;
        if (!isfinite(p) || !isfinite(v)) bad = 1;
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (t == 0) {
        a.status[0] = s_bad;
        a.status[2] = s_bad;
        if (a.status_host) { *a.status_host = s_bad; __threadfence_system(); }
    }
}

}  // namespace orcvio_amd
