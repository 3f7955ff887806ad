// cov_ops.hpp -- covariance bookkeeping on a device-resident P: the three places
// besides the update where the reference touches state_cov, so that P never has to cross PCIe between updates.
//   k_cov_propagate_*  OrcVIO::processModel      (src/orcvio.cpp:800-816)
//   k_cov_augment      OrcVIO::stateAugmentation (:962-1010, feature / nuisance states behind the clones included)
//   k_cov_remove       OrcVIO::pruneImuStateBuffer (:2935-2951, non-Schmidt branch); with a map that drops feature rows,
//                      rmLostFeaturesCov (:3776-3828)
//   k_cov_change_anchors  the in-state features' anchor change of pruneImuStateBuffer (:2664-2720, updateFeatureCov_*)
// All three are HBM-bound element kernels over an n x n matrix (n <= 406): coalesced row-major reads and writes.
#pragma once
#include <hip/hip_runtime.h>

#include "feature_anchor.hpp"

namespace orcvio_amd {

// T[i][j] = sum_k Phi[i][k] P[k][j],  i < leg, j < n   (the first leg rows of Phi * P)
__global__ __launch_bounds__(256) void k_cov_propagate_rows(const double* __restrict__ P, int n, const double* __restrict__ Phi, int leg,
                                                            double* __restrict__ T) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= leg * n) return;
    const int i = idx / n, j = idx - i * n;
    double s = 0.0;
    for (int k = 0; k < leg; ++k) s += Phi[i * leg + k] * P[(size_t)k * n + j];
    T[idx] = s;
}
// out = P with  P_LL <- sym(T[:, :leg] Phi^T + Q),  P_LC <- T[:, leg:],  P_CL <- its transpose,  P_CC unchanged
// refuse != nullptr and *refuse != 0 (k_imu_phi_q found Phi or Q not finite): out = P bit for bit
__global__ __launch_bounds__(256) void k_cov_propagate_finish(const double* __restrict__ P, int n, const double* __restrict__ Phi,
                                                              const double* __restrict__ Q, int leg, const double* __restrict__ T,
                                                              double* __restrict__ out, const int* __restrict__ refuse) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    if (refuse && *refuse) { out[idx] = P[idx]; return; }
    const int i = idx / n, j = idx - i * n;
    double v;
    if (i < leg && j < leg) {
        double a = Q[i * leg + j], b = Q[j * leg + i];
        for (int k = 0; k < leg; ++k) { a += T[(size_t)i * n + k] * Phi[j * leg + k]; b += T[(size_t)j * n + k] * Phi[i * leg + k]; }
        v = 0.5 * (a + b);
    } else if (i < leg) {
        v = T[(size_t)i * n + j];
    } else if (j < leg) {
        v = T[(size_t)j * n + i];
    } else {
        v = P[idx];
    }
    out[idx] = v;
}
// out (n+6)^2: the new clone copies rows/cols (0:3, 6:9) of P and is inserted at `pose` = n - rest_rows, i.e. behind the
// clones and in front of the feature / nuisance states (src/orcvio.cpp:976-1003: the rest block moves down / right by 6)
__global__ __launch_bounds__(256) void k_cov_augment(const double* __restrict__ P, int n, int pose, double* __restrict__ out) {
    const int m = n + 6;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * m) return;
    const int i = idx / m, j = idx - i * m;
    const bool ni = i >= pose && i < pose + 6, nj = j >= pose && j < pose + 6;
    // source row: old states keep their index (shifted back by 6 behind the new clone); new 0..2 -> theta, 3..5 -> p (6:9)
    const int si = ni ? (i - pose < 3 ? i - pose : i - pose + 3) : (i < pose ? i : i - 6);
    const int sj = nj ? (j - pose < 3 ? j - pose : j - pose + 3) : (j < pose ? j : j - 6);
    // [[P, P12^T], [P12, P11]] then (X + X^T)/2 as :1008-1010: the off-diagonal blocks are transposes of each other already
    double v;
    if (ni == nj) v = 0.5 * (P[(size_t)si * n + sj] + P[(size_t)sj * n + si]);
    else if (ni) v = P[(size_t)si * n + sj];
    else v = P[(size_t)sj * n + si];
    out[idx] = v;
}
// out m^2 = P without the rows/cols flagged in drop[] (drop[k] = 1: state k is removed); map[k'] = k precomputed
__global__ __launch_bounds__(256) void k_cov_remove(const double* __restrict__ P, int n, const int* __restrict__ map, int m,
                                                    double* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * m) return;
    const int i = idx / m, j = idx - i * m;
    out[idx] = P[(size_t)map[i] * n + map[j]];
}


// ---- the resident square-root factor S (P = S S^T), stored transposed: S(j, i) = F[i * ld + j], i < k (columns of S),
//      j < n (states) -- the layout of the Cholesky factor of the prior and of Z = L_M^-1 S^T --------------------------------
// commit: S+ = sigma Z^T if the update was applied (apply == nullptr or *apply != 0, and *fail == 0), else the prior's own factor
__global__ __launch_bounds__(256) void k_fac_commit(const double* __restrict__ Z, int ldz, int k, int n, double sigma,
                                                    const int* __restrict__ apply, const double* __restrict__ prior, long sLi, long sLj,
                                                    double* __restrict__ out, int ldo, const int* __restrict__ fail) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * n) return;
    const int i = idx / n, j = idx - i * n;
    const bool app = (apply ? (*apply != 0) : true) && fail[0] == 0 && fail[1] == 0;   // (fail: the pivot counters of chol(M); k_finish_sqrt kept P)
    out[(size_t)i * ldo + j] = app ? sigma * Z[(size_t)i * ldz + j] : prior[(long)j * sLi + (long)i * sLj];
}
// prefactor: the Cholesky of the REVERSED covariance (potrf_reg_body, rev) gives S(j, i) = L'(n-1-j, i); stored in the resident
// factor's own layout F[i * ld + j] (rows of the state in natural order), padding zeroed
__global__ __launch_bounds__(256) void k_fac_flip(const double* __restrict__ Rrev, int ldr, int n, double* __restrict__ out, int ldo) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * ldo) return;
    const int i = idx / ldo, j = idx - i * ldo;
    out[(size_t)i * ldo + j] = (j < n) ? Rrev[(size_t)i * ldr + (n - 1 - j)] : 0.0;
}
// stateAugmentation on the factor: the new clone's six rows of S are copies of the IMU's (theta, p) rows
__global__ __launch_bounds__(256) void k_fac_augment(const double* __restrict__ F, int ld, int k, int n, int pose,
                                                     double* __restrict__ out, int ldo) {
    const int m = n + 6;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * m) return;
    const int i = idx / m, j = idx - i * m;
    const bool nj = j >= pose && j < pose + 6;
    const int sj = nj ? (j - pose < 3 ? j - pose : j - pose + 3) : (j < pose ? j : j - 6);
    out[(size_t)i * ldo + j] = F[(size_t)i * ld + sj];
}
// marginalisation on the factor: the rows of S of the removed states are deleted (map[j'] = old index of new state j')
__global__ __launch_bounds__(256) void k_fac_remove(const double* __restrict__ F, int ld, int k, const int* __restrict__ map, int m,
                                                    double* __restrict__ out, int ldo) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * m) return;
    const int i = idx / m, j = idx - i * m;
    out[(size_t)i * ldo + j] = F[(size_t)i * ld + map[j]];
}


// ---- features entering the state, on the resident covariance: the tail of measurementUpdate_hybrid (src/orcvio.cpp:1818-1821,
//      :1904-1947) from the blocks k_ekf_new left on the device -------------------------------------------------------------
// HH = H_2^-1 H_1 (block back-substitution, H_2 upper triangular d x d per feature), column n: x = H_2^-1 r_1;
// W[j] = (H_2^T H_2)^-1 = R^-1 R^-T.  One thread per (feature, column).
__global__ __launch_bounds__(256) void k_aug_hh(const double* __restrict__ H1, const double* __restrict__ H2, const double* __restrict__ r1,
                                                int n, int n_new, int d, double* __restrict__ HH /* [d n_new][n + 1] */,
                                                double* __restrict__ W /* [n_new][d][d] */, int* __restrict__ singular, int diag_only = 0) {
    // diag_only: the reference's literal H_2.ldlt().solve(..) on an upper-triangular H_2 = division by its diagonal (src/orcvio.cpp:1826-1827)
    const int j = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_new || c > n) return;
    const double* R = H2 + (size_t)j * d * d;
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = d - 1; i >= 0; --i) {
        double m = c < n ? H1[(size_t)(d * j + i) * n + c] : r1[d * j + i];
        if (!diag_only)
            for (int k = i + 1; k < d; ++k) m -= R[i * d + k] * v[k];
        v[i] = m / R[i * d + i];
        HH[(size_t)(d * j + i) * (n + 1) + c] = v[i];
    }
    if (c == 0) {
        double Ri[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        bool bad = false;
        for (int i = 0; i < d; ++i) bad = bad || R[i * d + i] == 0.0;
        if (bad) *singular = 1;
        for (int cc = 0; cc < d; ++cc)
            for (int i = d - 1; i >= 0; --i) {
                double m = i == cc ? 1.0 : 0.0;
                for (int k = i + 1; k < d; ++k) m -= R[i * d + k] * Ri[k * d + cc];
                Ri[i * d + cc] = m / R[i * d + i];
            }
        for (int i = 0; i < d; ++i)
            for (int cc = 0; cc < d; ++cc) {
                double m = 0.0;
                for (int k = 0; k < d; ++k) m += Ri[i * d + k] * Ri[cc * d + k];
                W[(size_t)j * d * d + i * d + cc] = m;
            }
    }
}
// dx_new[r] = x[r] - HH[r][:] dx: one wavefront per row
__global__ __launch_bounds__(64) void k_aug_dx(const double* __restrict__ HH, int n, const double* __restrict__ dx, double* __restrict__ dx_new) {
    const int r = blockIdx.x;
    const double* row = HH + (size_t)r * (n + 1);
    double s = 0.0;
    for (int c = threadIdx.x; c < n; c += 64) s += row[c] * dx[c];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) dx_new[r] = row[n] - s;
}
// P_aug [(n + sz)^2] in the order [old (n - tail) | new (sz) | tail]: P+ , nHHP = -HH P+ (sz x n), Q = nHHP HH^T (sz x sz, so that
// P22 = -Q + s2 W), symmetrised as :1946 does
__global__ __launch_bounds__(256) void k_aug_assemble(const double* __restrict__ Pp, int n, int sz, int tail, int d, const double* __restrict__ nHHP,
                                                      const double* __restrict__ Q, const double* __restrict__ W, double s2,
                                                      double* __restrict__ out) {
    const int nt = n + sz, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nt * nt) return;
    const int i = idx / nt, j = idx - i * nt, n0 = n - tail;
    auto src = [&](int q) { return q < n0 ? q : (q < n0 + sz ? n + (q - n0) : q - sz); };   // index in the [old + tail | new] order
    const int a = src(i), b = src(j);
    double v;
    if (a < n && b < n) v = 0.5 * (Pp[(size_t)a * n + b] + Pp[(size_t)b * n + a]);
    else if (a >= n && b < n) v = nHHP[(size_t)(a - n) * n + b];
    else if (a < n && b >= n) v = nHHP[(size_t)(b - n) * n + a];
    else {
        const int r = a - n, c = b - n;
        double p = -0.5 * (Q[(size_t)r * sz + c] + Q[(size_t)c * sz + r]);
        if (r / d == c / d) p += 0.5 * s2 * (W[(size_t)(r / d) * d * d + (r % d) * d + (c % d)] + W[(size_t)(r / d) * d * d + (c % d) * d + (r % d)]);
        v = p;
    }
    out[idx] = v;
}

// ---- ... with the resident square-root factor carried along (orcvio_msckf_cov_commit_new_features_fac): two launches, no memset.
// With P+ = S+ S+^T, HH = H_2^-1 H_1 and W = R^-1 R^-T (R = H_2 upper triangular),
//     P_aug = S_aug S_aug^T,   S_aug = [  S+       0             ]   n rows,   kf columns | sz columns
//                                      [ -HH S+    sigma R^-1 (bd) ]   sz rows
// (block-diagonal second block, one d x d block per feature; under ORCVIO_OPT_REF_H2_LDLT too: there only HH and x divide by
// diag(H_2), W does not).  The factor is carried only without nuisance states, so its new rows stand behind ALL old ones.
//   k_aug_rows    grid (new row r, 64-column share y): every workgroup does the back-substitution of its feature's rows i >= r % d
//                 of [HH | x] in LDS (k_aug_hh's arithmetic; the rows below its own and the other shares' copies are recomputed,
//                 d <= 3: no workgroup waits for another), then its 64 columns of row r of -HH P+ into scratch and its 64
//                 columns of row r of -HH S+ straight into the spare factor buffer; one share stores row r of HH, one dx_new[r]
//                 (k_aug_dx's arithmetic), workgroup (0, 0) the singular word (stored, not raised: nothing to clear in front)
//   k_aug_finish  behind the launch boundary: P_aug but its new-new block element by element (k_aug_assemble's cases), S_aug but
//                 the rows k_aug_rows wrote (old rows as k_fac_commit writes them, exact zeros, sigma R^-1, zeros in the padding up to
//                 the leading dimension), and one wavefront per pair (r <= c) of the new-new block: Q(r, c) and Q(c, r) = rows of
//                 -HH P+ times rows of HH, P22 = -(Q + Q^T) / 2 + s2 (W + W^T) / 2 stored at (r, c) and (c, r) -- symmetric exactly
// S+ of the old rows: sigma Z^T, or the prior's own factor behind a refused or rejected update, by k_fac_commit's status words.
// Measured on MI355X (scripts/gpu_entering_commit_ab.py, profiles/r32a_entering_commit_ab.json: leg 22, 20 clones, 12 in-state
// features, n = 154 / 178, 1 and 3 entering features, both calls alternating in one process): the call 32-40 us against 62-79 us for
// orcvio_msckf_cov_commit_new_features; the call plus the frame's next update 137-146 us against 175-183 us (35-39 us less, the old
// route's own spread over the repeats at most 5 us).  Nearly all of it is the call: k_aug_rows 10-12 us + k_aug_finish 5-6 us against
// a memset and five launches of 21 us together, one fetch and one wait fewer; the next update itself gains 0-7 us, because the
// Cholesky chain of its prior runs inside k_front beside the tracks' workgroups and was mostly hidden already.
struct AugFacArgs {
    int on;                         // 0: the factor is dropped -- nothing below is read or written
    const double* Z; int ldz, kf;   // Z = L_M^-1 S^T of the update: S+(c, i) = sigma Z[i ldz + c]
    double sigma;
    const int* apply; const int* fail;
    const double* prior; long sLi, sLj;
    double* Sout; int ldo;          // S_aug(j, i) = Sout[i ldo + j]
};
__device__ __forceinline__ bool aug_fac_applied(const AugFacArgs& f) { return (f.apply ? (*f.apply != 0) : true) && f.fail[0] == 0 && f.fail[1] == 0; }
__device__ __forceinline__ double aug_fac_old(const AugFacArgs& f, bool app, int c, int i) {
    return app ? f.sigma * f.Z[(size_t)i * f.ldz + c] : f.prior[(long)c * f.sLi + (long)i * f.sLj];
}
// R^-1 of one feature's upper-triangular D x D block, column by column (k_aug_hh's arithmetic; D a constant: registers, no scratch)
template <int D>
__device__ __forceinline__ void aug_rinv(const double* __restrict__ R, double (&Ri)[D * D]) {
#pragma unroll
    for (int q = 0; q < D * D; ++q) Ri[q] = 0.0;
#pragma unroll
    for (int cc = 0; cc < D; ++cc)
#pragma unroll
        for (int i = D - 1; i >= 0; --i) {
            double m = i == cc ? 1.0 : 0.0;
#pragma unroll
            for (int k = i + 1; k < D; ++k) m -= R[i * D + k] * Ri[k * D + cc];
            Ri[i * D + cc] = m / R[i * D + i];
        }
}
// entry (a, b) of a D x D array in registers, a and b not known at compile time
template <int D>
__device__ __forceinline__ double aug_pick(const double (&M)[D * D], int a, int b) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < D * D; ++q) v = (q == a * D + b) ? M[q] : v;
    return v;
}
enum { AUG_ROWS_THREADS = 1024, AUG_ROWS_WAVES = AUG_ROWS_THREADS / 64 };
// dynamic LDS of k_aug_rows: [d][n + 1] rows of [HH | x], then the partial sums of -HH P+ [waves][64]
static inline size_t aug_rows_lds_bytes(int n, int d) { return sizeof(double) * ((size_t)d * (n + 1) + (size_t)AUG_ROWS_WAVES * 64); }
// grid.y of k_aug_rows: the workgroups of one row -- workgroup y takes the 64 columns y of -HH P+ and the 64 columns Y-1-y of -HH S+
static inline int aug_rows_split(int n, int kf_or_0) { const int a = (n + 63) / 64, b = (kf_or_0 + 63) / 64; return a > b ? a : b; }
template <int D>
__global__ __launch_bounds__(AUG_ROWS_THREADS) void k_aug_rows(const double* __restrict__ H1, const double* __restrict__ H2,
                                                               const double* __restrict__ r1, int n, int n_new, int diag_only,
                                                               const double* __restrict__ Pp, const double* __restrict__ dx,
                                                               double* __restrict__ HH /* [d n_new][n + 1] */, double* __restrict__ nHHP /* [d n_new][n] */,
                                                               double* __restrict__ dx_new, int* __restrict__ singular, AugFacArgs f) {
    extern __shared__ double aug_lds[];
    constexpr int d = D;
    const int r = blockIdx.x, j = r / d, i0 = r - j * d;
    const int y = blockIdx.y, Y = gridDim.y;           // this row's workgroups: each recomputes the row, each has columns of its own
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double* sH = aug_lds;                              // [d][n + 1]
    double* sPart = aug_lds + (size_t)d * (n + 1);     // [waves][64]
    const double* R = H2 + (size_t)j * d * d;
    for (int c = tid; c <= n; c += AUG_ROWS_THREADS) {
        double v[D], mine = 0.0;
#pragma unroll
        for (int i = d - 1; i >= 0; --i) {
            v[i] = 0.0;
            if (i < i0) continue;   // (uniform over the workgroup)
            double m = c < n ? H1[(size_t)(d * j + i) * n + c] : r1[d * j + i];
            if (!diag_only) {
#pragma unroll
                for (int k = i + 1; k < d; ++k) m -= R[i * d + k] * v[k];
            }
            v[i] = m / R[i * d + i];
            sH[i * (n + 1) + c] = v[i];
            if (i == i0) mine = v[i];
        }
        if (y == 0) HH[(size_t)r * (n + 1) + c] = mine;
    }
    if (r == 0 && y == 0 && tid == 0) {
        bool bad = false;
        for (int q = 0; q < n_new; ++q)
            for (int i = 0; i < d; ++i) bad = bad || H2[(size_t)q * d * d + i * d + i] == 0.0;
        *singular = bad ? 1 : 0;
    }
    __syncthreads();
    const double* hrow = sH + i0 * (n + 1);
    if (y == Y - 1 && wave == AUG_ROWS_WAVES - 1) {   // dx_new[r] = x[r] - HH[r][:] dx
        double s = 0.0;
        for (int c = lane; c < n; c += 64) s += hrow[c] * dx[c];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) dx_new[r] = hrow[n] - s;
    }
    // -HH P+, the 64 columns y: every wavefront a slice of the sum, the slices added in their order afterwards
    const int cl = (n + AUG_ROWS_WAVES - 1) / AUG_ROWS_WAVES;
    const bool has_P = y * 64 < n;
    if (has_P) {
        const int b = y * 64 + lane, c0 = wave * cl, c1 = c0 + cl < n ? c0 + cl : n;
        const double* col = Pp + (b < n ? b : n - 1);
        double acc = 0.0;
#pragma unroll 8
        for (int c = c0; c < c1; ++c) acc += hrow[c] * col[(size_t)c * n];
        sPart[wave * 64 + lane] = acc;
    }
    if (f.on) {   // -HH S+, the 64 columns Y-1-y: one wavefront per column of S+, four columns in flight
        const bool app = aug_fac_applied(f);
        for (int ib = (Y - 1 - y) * 64 + wave * 4; ib < f.kf; ib += Y * 64) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int c = lane; c < n; c += 64) {
                const double hv = hrow[c];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = ib + u < f.kf ? ib + u : f.kf - 1;
                    acc[u] += hv * aug_fac_old(f, app, c, i);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                double s = acc[u];
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                if (lane == 0 && ib + u < f.kf) f.Sout[(size_t)(ib + u) * f.ldo + n + r] = -s;
            }
        }
    }
    __syncthreads();
    if (has_P && tid < 64 && y * 64 + tid < n) {
        double s = 0.0;
        for (int sl = 0; sl < AUG_ROWS_WAVES; ++sl) s += sPart[sl * 64 + tid];
        nHHP[(size_t)r * n + y * 64 + tid] = -s;
    }
}
// grid: nb_P blocks over P_aug, nb_S over S_aug (0 without the factor), then four pairs of the new-new block per block
template <int D>
__global__ __launch_bounds__(256) void k_aug_finish(const double* __restrict__ Pp, int n, int sz, int tail, const double* __restrict__ H2,
                                                    const double* __restrict__ HH, const double* __restrict__ nHHP, double s2,
                                                    double* __restrict__ out, int nb_P, int nb_S, AugFacArgs f) {
    constexpr int d = D;
    const int nt = n + sz, n0 = n - tail;
    const int blk = blockIdx.x, tid = threadIdx.x;
    if (blk < nb_P) {
        const int idx = blk * 256 + tid;
        if (idx >= nt * nt) return;
        const int i = idx / nt, j = idx - i * nt;
        auto src = [&](int q) { return q < n0 ? q : (q < n0 + sz ? n + (q - n0) : q - sz); };   // index in the [old + tail | new] order
        const int a = src(i), b = src(j);
        if (a < n && b < n) out[idx] = 0.5 * (Pp[(size_t)a * n + b] + Pp[(size_t)b * n + a]);
        else if (a >= n && b < n) out[idx] = nHHP[(size_t)(a - n) * n + b];
        else if (a < n && b >= n) out[idx] = nHHP[(size_t)(b - n) * n + a];
        return;   // (new-new: the pair blocks)
    }
    if (blk < nb_P + nb_S) {   // (f.on; the factor's new rows stand at n .. nt-1: no nuisance states)
        const int idx = (blk - nb_P) * 256 + tid;
        if (idx >= (f.kf + sz) * f.ldo) return;
        const int i = idx / f.ldo, j = idx - i * f.ldo;
        double v = 0.0;
        if (i < f.kf) {
            if (j >= n && j < nt) return;   // k_aug_rows wrote -HH S+
            if (j < n) v = aug_fac_old(f, aug_fac_applied(f), j, i);
        } else if (j >= n && j < nt && (j - n) / d == (i - f.kf) / d) {
            const int q = (j - n) / d;
            double Ri[D * D];
            aug_rinv<D>(H2 + (size_t)q * d * d, Ri);
            v = f.sigma * aug_pick<D>(Ri, j - n - q * d, i - f.kf - q * d);
        }
        f.Sout[idx] = v;
        return;
    }
    const int p = (blk - nb_P - nb_S) * 4 + (tid >> 6), lane = tid & 63;
    if (p >= sz * (sz + 1) / 2) return;
    int r = 0, c = p;
    while (c >= sz - r) { c -= sz - r; ++r; }   // pair p -> (r, c), r <= c  (wave-uniform)
    c += r;
    double q1 = 0.0, q2 = 0.0;
    for (int b = lane; b < n; b += 64) {
        q1 += nHHP[(size_t)r * n + b] * HH[(size_t)c * (n + 1) + b];
        q2 += nHHP[(size_t)c * n + b] * HH[(size_t)r * (n + 1) + b];
    }
    for (int o = 32; o > 0; o >>= 1) { q1 += __shfl_xor(q1, o); q2 += __shfl_xor(q2, o); }
    if (lane != 0) return;
    double v = -0.5 * (q1 + q2);
    if (r / d == c / d) {
        const int q = r / d, ri = r - q * d, ci = c - q * d;
        double Ri[D * D];
        aug_rinv<D>(H2 + (size_t)q * d * d, Ri);
        double w1 = 0.0, w2 = 0.0;   // W(ri, ci) and W(ci, ri), W = R^-1 R^-T summed in k_aug_hh's order
#pragma unroll
        for (int k = 0; k < d; ++k) { w1 += aug_pick<D>(Ri, ri, k) * aug_pick<D>(Ri, ci, k); w2 += aug_pick<D>(Ri, ci, k) * aug_pick<D>(Ri, ri, k); }
        v += 0.5 * s2 * (w1 + w2);
    }
    out[(size_t)(n0 + r) * nt + n0 + c] = v;
    out[(size_t)(n0 + c) * nt + n0 + r] = v;
}



// ---- in-state SLAM features on the resident covariance (src/orcvio.cpp:2664-2720, updateFeatureCov_1didp :3611-3774,
//      _3didp :3457-3609) ----------------------------------------------------------------------------------------------------
// Anchor change of k <= 16 features in ONE workgroup: P <- T P T^T, T = I except the changed features' d rows, which are their J
// (feature_anchor.hpp: d x 21 non-zeros -- the feature, the old and new anchor clones, the extrinsics).  No J row reads another
// changed feature's rows, so this equals the reference's one-feature-after-the-other loop in real arithmetic.
//   1. J and the new parameters per feature (one lane per feature) -> LDS
//   2. Y = J P (k d rows) -> scratch Y [k d][n] (HBM/L2: 3-d at k = 16, n = 406 would be 156 KB, beyond a workgroup's LDS);
//      the factor, if given: S <- T S, row by row in place (a feature's new rows read only its own rows, clones and extrinsics)
//   3. the feature rows and columns of P from Y, the (k d)^2 block from Y J^T, symmetrised (Pff of the 3-d form is, :3602)
// P is changed in place: only the k d rows and columns are written.  chg_i [k][4] = slot, old, new anchor, unused; chg_d [k][6] = p_w,
// p_fej; ext = R_b2c 9 | t_c_b 3; params out [k][4] = param 3 | rho.
// (512 lanes for 1-d; the 3-d form's per-feature math needs ~300 VGPRs in lane q: 256 lanes, one wave per SIMD, no spill)
enum { ANCHOR_MAX_K = 16 };
// The launch inside the frame call (orcvio_msckf_io_step_frame_ex), enqueued between the frame's two updates; all null: the separate call.
//   refuse       device word of the feature step: a changed feature's position is not finite -> P and S stay as they are,
//                *refuse_also (the kept status word the prune update's commit reads) and *status_host are raised
//   first_info   kept status words of the frame's first update: [8] != 0 = it lost an in-launch hand-off and committed nothing -- this
//                launch does nothing either (P would be changed in place under the repeat): the call runs it again behind the repeat
//   par_host     [ANCHOR_MAX_K][3] param | [ANCHOR_MAX_K] rho in the pinned output block, stored ahead of the flag the call waits on
//                (system-scope fence by the storing lanes, as k_finish_pub's)
//   seq, flag    not null: no update follows in the frame -- this launch raises the flag itself
struct AnchorFrameArgs {
    const int* refuse; const int* first_info; int* refuse_also;
    double* par_host; int* status_host;
    unsigned long long* seq; unsigned long long* flag;
};
template <int d> struct AnchorThreads { enum { value = d == 3 ? 256 : 512 }; };
enum { ANCHOR_CHG_STRIDE = 4 };   // chg_i [k][4]: slot, old anchor, new anchor, (frame call: the feature's slam_features record)
__device__ __forceinline__ void anchor_publish(unsigned long long* seq, unsigned long long* flag) {
    __threadfence_system();
    const unsigned long long v = atomicAdd(seq, 1ull) + 1ull;
    __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ int anchor_col(int t, int fcol, int oc, int nc) {
    return t < ANCHOR_J_OLD ? fcol + t : (t < ANCHOR_J_NEW ? oc + t - ANCHOR_J_OLD : (t < ANCHOR_J_EXT ? nc + t - ANCHOR_J_NEW : 15 + t - ANCHOR_J_EXT));
}
template <int d>
__global__ __launch_bounds__(AnchorThreads<d>::value) void k_cov_change_anchors(double* __restrict__ P, int n, double* __restrict__ F, int ld, int fk,
                                                                   const double* __restrict__ poses, const double* __restrict__ ext,
                                                                   const int* __restrict__ chg_i, const double* __restrict__ chg_d, int k,
                                                                   int base, int leg, int if_fej, int literal_3d,
                                                                   double* __restrict__ params, double* __restrict__ Y, AnchorFrameArgs fr) {
    __shared__ double sJ[ANCHOR_MAX_K * 3 * ANCHOR_J_STRIDE];
    __shared__ int sC[ANCHOR_MAX_K * ANCHOR_J_STRIDE];   // state column of entry t of feature q's J rows
    __shared__ int sF[ANCHOR_MAX_K];                     // first column of feature q
    constexpr int ANCHOR_THREADS = AnchorThreads<d>::value;
    const int tid = threadIdx.x;
    {   // (the same words for every lane: a uniform branch)
        const bool lost = fr.first_info && fr.first_info[8] != 0;
        const bool bad = fr.refuse && *fr.refuse != 0;
        if (lost || bad) {
            if (tid == 0) {
                if (bad && !lost && fr.refuse_also) *fr.refuse_also = 1;
                if (fr.status_host) *fr.status_host = bad && !lost ? 1 : 0;
                if (fr.flag) anchor_publish(fr.seq, fr.flag);
            }
            return;
        }
    }
    if (tid < k) {
        const int q = tid;
        const int slot = chg_i[ANCHOR_CHG_STRIDE * q], o = chg_i[ANCHOR_CHG_STRIDE * q + 1], nw = chg_i[ANCHOR_CHG_STRIDE * q + 2];
        double par[3], rho;   // (J straight into LDS: 63 doubles fewer in registers)
        anchor_change(poses + (size_t)o * POSE_STRIDE, poses + (size_t)nw * POSE_STRIDE, ext, ext + 9, chg_d + 6 * q, chg_d + 6 * q + 3,
                      d, if_fej, literal_3d, par, &rho, sJ + q * 3 * ANCHOR_J_STRIDE);
        const int fcol = base + d * slot;
        const int oc = leg + 6 * o, nc = leg + 6 * ((d == 3 && literal_3d) ? o : nw);
        for (int t = 0; t < ANCHOR_J_STRIDE; ++t) sC[q * ANCHOR_J_STRIDE + t] = anchor_col(t, fcol, oc, nc);
        sF[q] = fcol;
        params[4 * q + 0] = par[0]; params[4 * q + 1] = par[1]; params[4 * q + 2] = par[2]; params[4 * q + 3] = rho;
        if (fr.par_host) {
            fr.par_host[3 * q + 0] = par[0]; fr.par_host[3 * q + 1] = par[1]; fr.par_host[3 * q + 2] = par[2];
            fr.par_host[3 * ANCHOR_MAX_K + q] = rho;
            if (q == 0) *fr.status_host = 0;
            __threadfence_system();
        }
    }
    __syncthreads();
    // (entries 0 .. d-1 of the feature block, then the 18 pose / extrinsic entries)
#define ANCHOR_DOT(acc, r, q, ld_, off)                                                                            \
    {                                                                                                            \
        const double* Jr = sJ + (q) * 3 * ANCHOR_J_STRIDE + (r) * ANCHOR_J_STRIDE;                               \
        const int* Cq = sC + (q) * ANCHOR_J_STRIDE;                                                              \
        acc = 0.0;                                                                                               \
        for (int t = 0; t < d; ++t) acc += Jr[t] * src[(size_t)Cq[t] * (ld_) + (off)];                            \
        for (int t = ANCHOR_J_OLD; t < ANCHOR_J_STRIDE; ++t) acc += Jr[t] * src[(size_t)Cq[t] * (ld_) + (off)];   \
    }
    {   // 2. Y = J P  (j fastest: coalesced reads of P's rows)
        const double* src = P;
        for (int idx = tid; idx < k * n; idx += ANCHOR_THREADS) {
            const int q = idx / n, j = idx - q * n;
            for (int r = 0; r < d; ++r) {
                double acc;
                ANCHOR_DOT(acc, r, q, n, j)
                Y[(size_t)(q * d + r) * n + j] = acc;
            }
        }
    }
    if (F) {   // S <- T S: S(state c, column i) = F[i ld + c]; feature q fastest (threads of a wave share column i)
        for (int idx = tid; idx < k * fk; idx += ANCHOR_THREADS) {
            const int i = idx / k, q = idx - i * k;
            double* col = F + (size_t)i * ld;
            const double* src = col;
            double acc[3] = {0.0, 0.0, 0.0};
            for (int r = 0; r < d; ++r) ANCHOR_DOT(acc[r], r, q, 1, 0)
            for (int r = 0; r < d; ++r) col[sF[q] + r] = acc[r];
        }
    }
    __syncthreads();
    {   // 3. rows / columns of P from Y; the (k d)^2 block from Y J^T, symmetrised
        const int m = k * d;
        for (int idx = tid; idx < m * n; idx += ANCHOR_THREADS) {
            const int rr = idx / n, j = idx - rr * n;
            const int frow = sF[rr / d] + rr % d;
            int s = -1;
            for (int q = 0; q < k; ++q)
                if (j >= sF[q] && j < sF[q] + d) s = q * d + (j - sF[q]);
            double v;
            if (s < 0) {
                v = Y[(size_t)rr * n + j];
                P[(size_t)j * n + frow] = v;
            } else {
                double z1, z2;
                { const double* src = Y + (size_t)rr * n; ANCHOR_DOT(z1, s % d, s / d, 1, 0) }
                { const double* src = Y + (size_t)s * n; ANCHOR_DOT(z2, rr % d, rr / d, 1, 0) }
                v = 0.5 * (z1 + z2);
            }
            P[(size_t)frow * n + j] = v;
        }
    }
#undef ANCHOR_DOT
    if (fr.flag) {   // (the frame's last launch the call waits for: every lane's stores are out before the flag rises)
        __threadfence();
        __syncthreads();
        if (tid == 0) anchor_publish(fr.seq, fr.flag);
    }
}

}  // namespace orcvio_amd
