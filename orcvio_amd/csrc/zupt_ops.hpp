// zupt_ops.hpp -- the zero-velocity update (OrcVIO::measurementUpdate_ZUPT_vpq, src/orcvio.cpp:3326-3454) on the device-resident
// covariance P and its resident square-root factor S (P = S S^T).
//
// The measurement Jacobian has fixed sparsity (:3329-3334): with b = leg + 6 N its nine rows are
//   rows 0..2   +I at columns 3:6                                   (current velocity)
//   rows 3..5   +I at columns b-3:b,   -I at columns b-9:b-6        (position of the two newest clones)
//   rows 6..8   -I/2 at columns b-6:b-3, +I/2 at columns b-12:b-9   (their orientation)
// so Y = H P is three combinations of 15 rows of P and nothing of size 9 x n is uploaded.
//   k_zupt_cov   M = Y H^T + R = C C^T, V = C^-1 Y, dx = V^T C^-1 r, P+ = (P + P^T)/2 - V^T V   (= sym((I - K H) P) for a symmetric P),
//                the trailing nuisance block of ORCVIO_OPT_SCHMIDT_STATES kept (:3432-3441); one 32 x 32 tile of P+ per workgroup
//   k_zupt_fac   S+ with S+ S+^T = P+: the array form -- [R^1/2 | W] (W = H S, 9 x k) is brought to lower-triangular form from the right
//                by nine Householder reflectors, the same reflectors applied to every row [0_9 | S_i]; 64 rows of S per workgroup
// Every workgroup derives M, C (k_zupt_cov) and the reflectors (k_zupt_fac) redundantly from the 15 rows it needs: no workgroup waits
// for another, and the results go to the spare buffers (the host swaps), so no workgroup reads what another has written.
// The update is REFUSED when one of the 15 rows of P is not finite or M is not positive definite: every workgroup sees the same 15
// rows and takes the same decision; P+ is then a bit copy of P, dx = 0, the status word is raised and k_zupt_fac copies S.
//   k_zupt_cov_keep / k_zupt_fac_keep   the same update for the stationary frame of a HYBRID filter, where every in-state feature
//                leaves in FRONT of the update (checkZUPTFeat :3102-3119, checkZUPTIMU :3302-3319) and the previous clone behind it
//                (:2641-2645): both are gathers of P+ / S+, which these kernels write anyway, so they write them COMPACTED -- the
//                states 0 .. b-1 without the previous clone's six.  One body per pair (zupt_cov_body, zupt_fac_body): the gate, M, C,
//                V, dx and the tile arithmetic are k_zupt_cov's on the leading b x b block, bit for bit gather -> update -> gather.
//                Refused (or rejected by the check in front: a.also): the bit copy at the input's dimension, nothing leaves.
#pragma once
#include <hip/hip_runtime.h>

namespace orcvio_amd {

enum { ZUPT_TILE = 32, ZUPT_FAC_ROWS = 64, ZUPT_KMAX = 448 };   // (ZUPT_KMAX: columns of S the reflectors of k_zupt_fac hold in LDS)

struct ZuptArgs {
    double r[9];
    double noise[3];   // variances of r_v, r_p, r_q
    int n, b, nui6;    // state dimension, leg + 6 N, 6 x nuisance states (the trailing block P+ keeps)
    const int* also = nullptr;   // optional: a status block whose refusal ([2] != 0: k_imu_phi_q's Phi not finite) refuses this update too
};

// state index of the l-th of the 15 rows H touches: 3..5, then b-12 .. b-1
__device__ __forceinline__ int zupt_row(int l, int b) { return l < 3 ? 3 + l : b - 15 + l; }
// y = H p for p = the 15 entries (zupt_row order) of one column
__device__ __forceinline__ void zupt_combine(const double* p, double* y) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        y[a] = p[a];
        y[3 + a] = p[12 + a] - p[6 + a];
        y[6 + a] = 0.5 * (p[3 + a] - p[9 + a]);
    }
}

// column `col` of V = C^-1 Y from the 15 rows of P (leading dimension ld), C in the lower triangle of sM
__device__ __forceinline__ void zupt_v_col(const double* __restrict__ P, int ld, int b, int col, const double (*sM)[9], double* v) {
    double p[15];
    for (int l = 0; l < 15; ++l) p[l] = P[(size_t)zupt_row(l, b) * ld + col];
    zupt_combine(p, v);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        double x = v[i];
#pragma unroll
        for (int k = 0; k < i; ++k) x -= sM[i][k] * v[k];
        v[i] = x / sM[i][i];
    }
}
__device__ __forceinline__ double zupt_dx_entry(const double* v, const double* sz) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) s += v[i] * sz[i];
    return s;
}

// What stays behind a fused update (k_zupt_cov_keep, k_zupt_fac_keep): the states 0 .. b-1 without the six rows that begin at `hole`
// (hole >= m: none), so kept state i is state zupt_src(i, hole) of the prior -- a prefix and at most one hole, no index map.
struct ZuptKeep {
    int m, hole;   // the kept dimension, the first row of the dropped clone
};
__device__ __forceinline__ int zupt_src(int i, int hole) { return i < hole ? i : i + 6; }

// ONE body for both covariance kernels.  KEEP = false: k_zupt_cov, P and out are [n][n].  KEEP = true: P is [n][n], the gate and the
// update see its leading b x b block only (the states behind b have left BEFORE the update: they are neither scanned nor written),
// applied: out is [m][m], one tile of the OUTPUT index space per workgroup (the workgroups behind ceil(m / 32) have nothing to
// do); not applied: out is the bit copy [n][n], the tile loop running over the input's index space.
template <bool KEEP>
__device__ __forceinline__ void zupt_cov_body(const double* __restrict__ P, const ZuptArgs& a, const ZuptKeep kp, double* __restrict__ out,
                                              double* __restrict__ dx, int* __restrict__ status) {
    __shared__ double s15[15][16];   // P at the 15 x 15 rows / columns of H
    __shared__ double sYs[9][16];    // Y at those 15 columns
    __shared__ double sM[9][9];      // M, then its Cholesky factor C in the lower triangle
    __shared__ double sz[9];         // C^-1 r
    __shared__ double sV[2][9][ZUPT_TILE + 1];   // V at the tile's columns [0] and rows [1]
    __shared__ double sT[ZUPT_TILE][ZUPT_TILE + 1];   // the transposed tile of P
    __shared__ int sBad;
    const int tid = threadIdx.x, n = a.n, b = a.b;
    const int ns = KEEP ? b : n;   // the columns the gate scans and dx covers
    const int J0 = blockIdx.x * ZUPT_TILE, I0 = blockIdx.y * ZUPT_TILE;
    if (tid == 0) sBad = 0;
    __syncthreads();
    {   // the gate's scan: every entry of the 15 rows
        bool bad = false;
        for (int idx = tid; idx < 15 * ns; idx += 256) {
            const int l = idx / ns, j = idx - l * ns;
            bad = bad || !isfinite(P[(size_t)zupt_row(l, b) * n + j]);
        }
        if (tid < 225) s15[tid / 15][tid % 15] = P[(size_t)zupt_row(tid / 15, b) * n + zupt_row(tid % 15, b)];
        if (bad) sBad = 1;
    }
    __syncthreads();
    if (tid < 15) {   // column tid of Y
        double p[15], y[9];
        for (int l = 0; l < 15; ++l) p[l] = s15[l][tid];
        zupt_combine(p, y);
        for (int i = 0; i < 9; ++i) sYs[i][tid] = y[i];
    }
    __syncthreads();
    if (tid < 9) {   // row tid of M = Y H^T + R
        double p[15], y[9];
        for (int l = 0; l < 15; ++l) p[l] = sYs[tid][l];
        zupt_combine(p, y);
        y[tid] += a.noise[tid / 3];
        for (int j = 0; j < 9; ++j) sM[tid][j] = y[j];
    }
    __syncthreads();
    if (tid == 0) {   // M = C C^T (lower triangle, as the reference's ldlt reads it), z = C^-1 r
        bool bad = false;
        for (int j = 0; j < 9; ++j) {
            double d = sM[j][j];
            for (int k = 0; k < j; ++k) d -= sM[j][k] * sM[j][k];
            if (!(d > 0.0) || !isfinite(d)) { bad = true; break; }
            const double c = sqrt(d);
            sM[j][j] = c;
            for (int i = j + 1; i < 9; ++i) {
                double v = sM[i][j];
                for (int k = 0; k < j; ++k) v -= sM[i][k] * sM[j][k];
                sM[i][j] = v / c;
            }
        }
        if (!bad)
            for (int i = 0; i < 9; ++i) {
                double v = a.r[i];
                for (int k = 0; k < i; ++k) v -= sM[i][k] * sz[k];
                sz[i] = v / sM[i][i];
                bad = bad || !isfinite(sz[i]);
            }
        if (bad) sBad = 1;
    }
    __syncthreads();
    const bool refused = sBad != 0 || (a.also && a.also[2] != 0);
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *status = refused ? 1 : 0;
    const int no = KEEP && !refused ? kp.m : n;        // the dimension of what this launch writes
    const int hole = KEEP && !refused ? kp.hole : no;  // (a copy has no hole)
    if (KEEP && (J0 >= no || I0 >= no)) return;        // (uniform: a tile of the input's grid the smaller output does not have)
    if (!refused && tid < 2 * ZUPT_TILE) {   // V = C^-1 Y at the tile's columns (tid < 32) and rows (tid >= 32): ONE code path for both
        const int w = tid / ZUPT_TILE, t = tid - w * ZUPT_TILE;
        const int oc = (w == 0 ? J0 : I0) + t;
        const int col = KEEP ? zupt_src(oc, hole) : oc;
        double v[9];
        if (oc < no) {
            zupt_v_col(P, n, b, col, sM, v);
        } else {
#pragma unroll
            for (int i = 0; i < 9; ++i) v[i] = 0.0;
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) sV[w][i][t] = v[i];
        if (w == 0 && blockIdx.y == 0 && oc < no) dx[col] = zupt_dx_entry(v, sz);
    }
    if (KEEP && !refused && blockIdx.x == 0 && blockIdx.y == 0 && tid >= 2 * ZUPT_TILE && tid < 2 * ZUPT_TILE + 6 && hole < no) {
        double v[9];   // dx at the dropped clone's six states, which no tile of the output has
        zupt_v_col(P, n, b, hole + (tid - 2 * ZUPT_TILE), sM, v);
        dx[hole + (tid - 2 * ZUPT_TILE)] = zupt_dx_entry(v, sz);
    }
    if (refused && blockIdx.y == 0 && tid < ZUPT_TILE && J0 + tid < ns) dx[J0 + tid] = 0.0;
    const int tx = tid & (ZUPT_TILE - 1), ty = tid / ZUPT_TILE;   // 32 x 8 lanes over the tile
    for (int rr = ty; rr < ZUPT_TILE; rr += 256 / ZUPT_TILE) {   // sT[rr][tx] = P[J0 + rr][I0 + tx]
        const int i = J0 + rr, j = I0 + tx;
        sT[rr][tx] = (i < no && j < no) ? P[(size_t)(KEEP ? zupt_src(i, hole) : i) * n + (KEEP ? zupt_src(j, hole) : j)] : 0.0;
    }
    __syncthreads();
    const int keep = n - a.nui6;
    for (int rr = ty; rr < ZUPT_TILE; rr += 256 / ZUPT_TILE) {
        const int i = I0 + rr, j = J0 + tx;
        if (i >= no || j >= no) continue;
        const double pij = P[(size_t)(KEEP ? zupt_src(i, hole) : i) * n + (KEEP ? zupt_src(j, hole) : j)], pji = sT[tx][rr];
        double v;
        if (refused) v = pij;
        else {
            v = 0.5 * (pij + pji);
            if (KEEP || !(i >= keep && j >= keep)) {   // (KEEP: no nuisance states, the calls refuse them)
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) s = fma(sV[1][k][rr], sV[0][k][tx], s);
                v -= s;
            }
        }
        out[(size_t)i * no + j] = v;
    }
}

__global__ __launch_bounds__(256) void k_zupt_cov(const double* __restrict__ P, ZuptArgs a, double* __restrict__ out, double* __restrict__ dx,
                                                  int* __restrict__ status) {
    zupt_cov_body<false>(P, a, ZuptKeep{a.n, a.n}, out, dx, status);
}
// the update that writes what stays: grid ceil(n / 32)^2 (the refused form copies [n][n])
__global__ __launch_bounds__(256) void k_zupt_cov_keep(const double* __restrict__ P, ZuptArgs a, ZuptKeep kp, double* __restrict__ out,
                                                       double* __restrict__ dx, int* __restrict__ status) {
    zupt_cov_body<true>(P, a, kp, out, dx, status);
}

// S(state i, column c) = F[c * ld + i], c < k.  KEEP = false (k_zupt_fac): out has the same shape and leading dimension.  KEEP = true:
// applied, row i of S+ goes to its kept position with leading dimension ld_out, the rows >= b and the dropped clone's are not written;
// refused, the bit copy at ld.  ONE body for both.
template <bool KEEP>
__device__ __forceinline__ void zupt_fac_body(const double* __restrict__ F, int ld, int k, const ZuptArgs& a, const ZuptKeep kp, int ld_out,
                                              const int* __restrict__ status, double* __restrict__ out) {
    __shared__ double sW[9][ZUPT_KMAX];   // W = H S, row j becoming reflector j's part over the columns of S
    __shared__ double sRed[2][4][9];
    __shared__ double sG[9][9];           // sG[j][i] = w~_j . w~_i (i < j)
    __shared__ double sBeta[9];
    __shared__ double sZ[4][9][ZUPT_FAC_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = a.n, b = a.b;
    const int i = blockIdx.x * ZUPT_FAC_ROWS + lane;
    if (*status != 0) {   // refused: the factor stays (a bit copy into the spare buffer)
        if (i < n)
            for (int c = wv; c < k; c += 4) out[(size_t)c * ld + i] = F[(size_t)c * ld + i];
        return;
    }
    for (int c = tid; c < k; c += 256) {
        double p[15], y[9];
        for (int l = 0; l < 15; ++l) p[l] = F[(size_t)c * ld + zupt_row(l, b)];
        zupt_combine(p, y);
        for (int j = 0; j < 9; ++j) sW[j][c] = y[j];
    }
    // (each lane touches its own columns of sW only: no barrier but the reductions')
    for (int j = 0; j < 9; ++j) {
        double part[9];
#pragma unroll
        for (int m = 0; m < 9; ++m) part[m] = 0.0;
        for (int c = tid; c < k; c += 256) {
            const double wj = sW[j][c];
#pragma unroll
            for (int m = 0; m < 9; ++m) part[m] = fma(wj, sW[m][c], part[m]);
        }
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            double v = part[m];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            part[m] = v;
        }
        if (lane == 0)
            for (int m = 0; m < 9; ++m) sRed[j & 1][wv][m] = part[m];
        __syncthreads();
        double tot[9];
#pragma unroll
        for (int m = 0; m < 9; ++m) tot[m] = (sRed[j & 1][0][m] + sRed[j & 1][1][m]) + (sRed[j & 1][2][m] + sRed[j & 1][3][m]);
        // reflector j: u = (d_j + sigma at position j of the leading block | w~_j), beta = 2 / u^T u = 1 / (sigma (d_j + sigma))
        const double dj = sqrt(a.noise[j / 3]);
        const double sigma = sqrt(a.noise[j / 3] + tot[j]);
        const double beta = 1.0 / (sigma * (dj + sigma));
        if (tid == 0) {
            sBeta[j] = beta;
            for (int m = 0; m < j; ++m) sG[j][m] = tot[m];
        }
        for (int c = tid; c < k; c += 256) {   // the rows of W behind row j (their leading-block entry in column j is zero)
            const double wj = sW[j][c];
#pragma unroll
            for (int m = 0; m < 9; ++m)
                if (m > j) sW[m][c] -= beta * tot[m] * wj;
        }
    }
    __syncthreads();
    // the reflectors on row [0_9 | S_i]: z = W~ s;  t_j = beta_j (z_j - sum_{m<j} G_jm t_m);  s+ = s - sum_j t_j w~_j
    const bool mine = KEEP ? (i < b && !(i >= kp.hole && i < kp.hole + 6)) : i < n;   // this lane's row is written
    const int io = KEEP && i >= kp.hole ? i - 6 : i;
    double z[9];
#pragma unroll
    for (int m = 0; m < 9; ++m) z[m] = 0.0;
    if (mine)
        for (int c = wv; c < k; c += 4) {
            const double s = F[(size_t)c * ld + i];
#pragma unroll
            for (int m = 0; m < 9; ++m) z[m] = fma(sW[m][c], s, z[m]);
        }
#pragma unroll
    for (int m = 0; m < 9; ++m) sZ[wv][m][lane] = z[m];
    __syncthreads();
    double t[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        double v = (sZ[0][j][lane] + sZ[1][j][lane]) + (sZ[2][j][lane] + sZ[3][j][lane]);
#pragma unroll
        for (int m = 0; m < j; ++m) v -= sG[j][m] * t[m];
        t[j] = sBeta[j] * v;
    }
    if (mine)
        for (int c = wv; c < k; c += 4) {
            double s = F[(size_t)c * ld + i];
#pragma unroll
            for (int j = 0; j < 9; ++j) s -= t[j] * sW[j][c];
            out[(size_t)c * ld_out + io] = s;
        }
}

__global__ __launch_bounds__(256) void k_zupt_fac(const double* __restrict__ F, int ld, int k, ZuptArgs a, const int* __restrict__ status,
                                                  double* __restrict__ out) {
    zupt_fac_body<false>(F, ld, k, a, ZuptKeep{a.n, a.n}, ld, status, out);
}
// grid ceil(n / 64) (the refused form copies every row)
__global__ __launch_bounds__(256) void k_zupt_fac_keep(const double* __restrict__ F, int ld, int k, ZuptArgs a, ZuptKeep kp, int ld_out,
                                                       const int* __restrict__ status, double* __restrict__ out) {
    zupt_fac_body<true>(F, ld, k, a, kp, ld_out, status, out);
}

}  // namespace orcvio_amd
