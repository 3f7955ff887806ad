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
// k_imu_phi_q46, at the end of this header, is the same with the 24 IMU intrinsics in the state (leg_dim 46).
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

// ---- leg_dim = 46 -----------------------------------------------------------------------------------------------------------------
// k_imu_phi_q46: the same contract (one launch, one workgroup of four wavefronts, FP64, no other workgroup, the order of every sum a
// function of S alone) with the 24 IMU intrinsics in the state.  Rows 15 .. 45 of every Phi_k are identity rows and N_k lives in the
// leading 15 x 15, so Q and A = Phi[0:15, 0:15] follow k_imu_phi_q's recursion and only B = Phi[0:15, 22:46] is new:
// B <- A_k B + B_k, B_k non-zero in rows 0 .. 8, on two 16 x 16 tiles (24 columns padded to 32): 8 more MFMA a sample.  A_k is already
// in registers as the A operand, B stays in the result layout, which is the next product's B operand.
//   A sample's compact form is 330 doubles (ten 3 x 3 blocks, N_k, B_k [9][24]): 128 of them do not fit the LDS.  Phases 1 and 2 run in
//   ROUNDS of eight samples a wavefront (one round covers S <= 32), and only a round's compact forms are in LDS: 4 x 8 x 331 doubles.
//   phase 1  lane (i, j) = (l >> 3, l & 7) of a wavefront makes column group j (one of T1 T2 T3 A1 A2 A3 M1 M2: 9 x 3) of the round's
//            sample i -- imu_phi46_triple, the header's function; lane (i, 0) also makes the ten leading blocks and N_k.  The Euler forms
//            and the right closed form have no intrinsic blocks: zeros are written, and B stays exactly zero.
//   phase 2  as k_imu_phi_q, and B <- A_k B + B_k.
//   phase 3  wavefront 0 combines in chunk order, B = A_b B_a + B_b with the pair; every thread writes a piece of Phi, Q [46][46]
//            (identity / zero outside A, B and the 15 x 15 of Q; Q symmetrised) and tests it.
enum { IMU46_ROUND = 8, IMU46_STRIDE = IMU_COMPACT46 + 1 };   // (331 doubles: odd, as IMU_LDS_STRIDE)

struct ImuKernArgs46 {
    const double* recs;   // [S][IMU_REC46]
    double* Phi;          // [46][46] out
    double* Q;            // [46][46] out
    int* status;          // as ImuKernArgs::status
    int S;
    ImuFlags flags;
    double grav[3];
    double qc[12];
    ImuIntrinsicMx mx;
};
static inline size_t imu46_lds_bytes() { return sizeof(double) * IMU46_STRIDE * (size_t)(IMU_WAVES * IMU46_ROUND); }

__device__ __forceinline__ int imu_phi_off46(int i, int j) {
    if (i < 9 && j < 15) {
        const int b = imu_block46(i / 3, j / 3);
        if (b >= 0) return b * 9 + (i % 3) * 3 + j % 3;
    }
    return i == j ? -1 : -2;
}
__device__ __forceinline__ int imu_noise_off46(int i, int j) {
    if (i < 6 && j < 6) return i / 3 == j / 3 ? IMU_COMPACT46_N00 + 9 * (i / 3) + (i % 3) * 3 + j % 3 : -2;
    if (i >= 9 && i < 15 && i == j) return IMU_COMPACT46_ND + i - 9;
    return -2;
}
// offset of B_k(i, j), i < 16, j < 32 (-2: zero)
__device__ __forceinline__ int imu_b_off46(int i, int j) { return (i < 9 && j < IMU_NI) ? IMU_COMPACT46_B + i * IMU_NI + j : -2; }
// pa b + add on a wavefront, pa as in imu_combine, b and add in the result layout
__device__ __forceinline__ d4 imu_mul_add(const double pa[4], d4 b, d4 add) {
    d4 o = add;
#pragma unroll
    for (int s = 0; s < 4; ++s) o = mfma_f64(pa[s], b[s], o);
    return o;
}

__global__ __launch_bounds__(64 * IMU_WAVES) void k_imu_phi_q46(ImuKernArgs46 a) {
    extern __shared__ double s_comp[];                 // [IMU_WAVES * IMU46_ROUND][IMU46_STRIDE]
    __shared__ double s_part[IMU_WAVES][4][256];       // the wavefronts' partial Phi (A), Q and the two tiles of B, [row][column]
    __shared__ ImuIntrinsicMx s_mx;
    __shared__ int s_bad;
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const int S = a.S, C = (S + IMU_WAVES - 1) / IMU_WAVES;
    const int k0 = w * C, k1 = k0 + C < S ? k0 + C : S;   // this wavefront's chunk [k0, k1)
    const int rounds = (C + IMU46_ROUND - 1) / IMU46_ROUND;   // (of every wavefront: the barriers below are uniform)
    if (t == 0) s_bad = 0;
    if (t < 9) { s_mx.Tg[t] = a.mx.Tg[t]; s_mx.As[t] = a.mx.As[t]; s_mx.Ma[t] = a.mx.Ma[t]; s_mx.TA[t] = a.mx.TA[t]; }
    __syncthreads();
    const bool intr = imu_has_intrinsic_blocks(a.flags);
    const int col = l & 15, g = l >> 4;
    int po[4], no[4], bo[2][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        po[s] = imu_phi_off46(col, 4 * s + g);
        no[s] = imu_noise_off46(g + 4 * s, col);
        bo[0][s] = imu_b_off46(g + 4 * s, col);
        bo[1][s] = imu_b_off46(g + 4 * s, col + 16);
    }
    d4 phi, q = {0.0, 0.0, 0.0, 0.0}, b0 = {0.0, 0.0, 0.0, 0.0}, b1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) phi[r] = (g + 4 * r == col) ? 1.0 : 0.0;
    for (int rd = 0; rd < rounds; ++rd) {
        const int kb = k0 + rd * IMU46_ROUND;
        // ---- phase 1
        {
            const int i = l >> 3, j = l & 7;
            if (kb + i < k1) {
                const double* rec = a.recs + (size_t)(kb + i) * IMU_REC46;
                double* c = s_comp + (size_t)(w * IMU46_ROUND + i) * IMU46_STRIDE;
                if (j == 0) {
                    ImuCompactSink46 sink{c};
                    imu_phi46_lead(rec, a.flags, a.grav, s_mx, sink);
                    imu_noise(rec, a.flags, a.qc, c + IMU_COMPACT46_N00);
                }
                double o[27];
                if (intr) {
                    imu_phi46_triple(rec, s_mx, j, o);
                } else {
#pragma unroll
                    for (int e = 0; e < 27; ++e) o[e] = 0.0;
                }
#pragma unroll
                for (int r = 0; r < 9; ++r)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) c[IMU_COMPACT46_B + r * IMU_NI + 3 * j + cc] = o[r * 3 + cc];
            }
        }
        __syncthreads();
        // ---- phase 2
        const int ke = kb + IMU46_ROUND < k1 ? kb + IMU46_ROUND : k1;
        for (int k = kb; k < ke; ++k) {
            const double* c = s_comp + (size_t)(w * IMU46_ROUND + k - kb) * IMU46_STRIDE;
            double pa[4];
            d4 nk, bk0, bk1;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                pa[s] = imu_pick(c, po[s]); nk[s] = imu_pick(c, no[s]);
                bk0[s] = imu_pick(c, bo[0][s]); bk1[s] = imu_pick(c, bo[1][s]);
            }
            b0 = imu_mul_add(pa, b0, bk0);
            b1 = imu_mul_add(pa, b1, bk1);
            imu_combine(pa, nk, phi, q, true);
        }
        __syncthreads();   // (the next round overwrites s_comp)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = (g + 4 * r) * 16 + col;
        s_part[w][0][e] = phi[r]; s_part[w][1][e] = q[r]; s_part[w][2][e] = b0[r]; s_part[w][3][e] = b1[r];
    }
    __syncthreads();
    // ---- phase 3
    if (w == 0) {
        for (int b = 1; b < IMU_WAVES && b * C < S; ++b) {
            double pa[4];
            d4 qb, bb0, bb1;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int e = (g + 4 * s) * 16 + col;
                pa[s] = s_part[b][0][col * 16 + 4 * s + g];
                qb[s] = s_part[b][1][e]; bb0[s] = s_part[b][2][e]; bb1[s] = s_part[b][3][e];
            }
            b0 = imu_mul_add(pa, b0, bb0);
            b1 = imu_mul_add(pa, b1, bb1);
            imu_combine(pa, qb, phi, q, false);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = (g + 4 * r) * 16 + col;
            s_part[0][0][e] = phi[r]; s_part[0][1][e] = q[r]; s_part[0][2][e] = b0[r]; s_part[0][3][e] = b1[r];
        }
    }
    __syncthreads();
    int bad = 0;
    for (int e = t; e < IMU_LEG46 * IMU_LEG46; e += 64 * IMU_WAVES) {
        const int i = e / IMU_LEG46, j = e - i * IMU_LEG46;
        const bool in = i < IMU_DIM && j < IMU_DIM;
        double p = i == j ? 1.0 : 0.0;
        if (in) p = s_part[0][0][i * 16 + j];
        else if (i < IMU_DIM && j >= IMU_LEG) p = s_part[0][2 + ((j - IMU_LEG) >> 4)][i * 16 + ((j - IMU_LEG) & 15)];
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
    }
}

}  // namespace orcvio_amd
