// zupt_check_model.hpp -- the reference's zero-velocity test on IMU samples (checkZUPTIMU, src/orcvio.cpp:3129-3323) at leg_dim = 22
// (Tg = Ma = I, As = 0), in plain C++ that compiles for the host and for the device (the guard pattern of imu_model.hpp, no Eigen).
//
// The reference stacks m = S - 1 blocks of six rows over the nine states (theta, b_g, b_a) -- gyro rows [0 I 0] with a ZERO residual
// (:3194) and noise sigma_w^2 / dt_i, accelerometer rows [J_i 0 R] with r_i = -R a_i - g and noise sigma_a^2 / dt_i -- forms
// S = H P_m H^T + R of order 6 m and evaluates chi^2 = r^T S^-1 r.  H has nine columns and R is diagonal, so with W = R^-1,
//   A = H^T W H (9 x 9),  b = H^T W r,  c = r^T W r   (56 sums over the rows: 45 + 9 + 1 and the sum of the dt_i)
//   P_m = L L^T,  M = I + L^T A L = C C^T,  chi^2 = c - |C^-1 L^T b|^2
// is the same number (Woodbury).  P_m is the 9 x 9 marginal of P over the rows / columns {0,1,2, 9..14} with
// diag(dt_sum sigma_wb I, dt_sum sigma_ab I) added to its b_g / b_a block: sigma_wb, sigma_ab NOT squared, as :3228-3229 have them.
//
//   zupt_check_pack     samples [S][7] (t | gyro | acc) -> rows [S - 1][4] (dt_i = t_i+1 - t_i | acc of sample i); refuses dt_i <= 0
//   zupt_check_row      one row block's 56 contributions
//   zupt_check_marginal the marginal out of P, both triangles read ((P_ij + P_ji) / 2); reports a non-finite entry
//   zupt_check_solve    the 9 x 9 part
//   zupt_check_host     all of it on the host, the sums in row order: the fall-back of the C++ host layer without a resident covariance.
// k_zupt_check (zupt_check_ops.hpp) calls zupt_check_row and zupt_check_solve: one source for both.
#pragma once

#if defined(__HIPCC__)
#define ORC_ZCHK_HD __host__ __device__ inline
#else
#define ORC_ZCHK_HD inline
#endif

#include <math.h>
#include <stddef.h>

namespace orcvio_amd {

enum { ZCHK_MAX_SAMPLES = 128, ZCHK_ROW = 4, ZCHK_SUMS = 56, ZCHK_B = 45, ZCHK_C = 54, ZCHK_DT = 55 };
// what zupt_check_solve / the kernel's status word report (non-zero: not evaluated)
enum { ZCHK_OK = 0, ZCHK_NOT_FINITE = 1, ZCHK_P_NOT_SPD = 2, ZCHK_M_NOT_SPD = 3, ZCHK_UPSTREAM = 4 };

struct ZuptCheckConsts {
    double sigma_w2, sigma_a2;   // variances (:3140-3142)
    double sigma_wb, sigma_ab;   // used unsquared (:3228-3229)
    int left;                    // use_left_perturbation_flag
};

// one validated check: what the launch (or the host fall-back) and the verdict need
struct ZuptCheckJob {
    ZuptCheckConsts k;
    double R[9], ba[3], g[3];
    double limit, threshold, speed, max_velocity;   // limit = chi2_multiplier x threshold
    int m, dof, force_reject;                       // force_reject: the speed test failed
    double rows[(ZCHK_MAX_SAMPLES - 1) * ZCHK_ROW];
};

// state index of the k-th of the nine marginal states: theta 0..2, b_g 9..11, b_a 12..14
ORC_ZCHK_HD int zupt_check_state(int k) { return k < 3 ? k : k + 6; }
// A(i, j), i <= j, in the packed upper triangle (45 entries, row by row)
ORC_ZCHK_HD int zupt_check_tri(int i, int j) { return i * 9 - i * (i - 1) / 2 + (j - i); }

// rows [S - 1][ZCHK_ROW] from the selected samples.  Returns 0, or 1 + the index of the first interval that is not finite or <= 0
// (the reference divides by it: a zero gives NaN, and NaN > threshold is false -- it would ACCEPT).
ORC_ZCHK_HD int zupt_check_pack(const double* samples, int S, double* rows) {
    for (int i = 0; i + 1 < S; ++i) {
        const double dt = samples[(i + 1) * 7] - samples[i * 7];
        if (!(dt > 0.0) || !isfinite(dt)) return 1 + i;
        rows[i * ZCHK_ROW] = dt;
        for (int a = 0; a < 3; ++a) rows[i * ZCHK_ROW + 1 + a] = samples[i * 7 + 4 + a];
    }
    return 0;
}

// One row block's share of A (packed upper triangle), b, c and dt_sum: out [ZCHK_SUMS] is written, not added to.
ORC_ZCHK_HD void zupt_check_row(const double* row, const double* R, const double* ba, const double* g, const ZuptCheckConsts& k, double* out) {
    const double dt = row[0];
    const double a[3] = {row[1] - ba[0], row[2] - ba[1], row[3] - ba[2]};
    double Ra[3];
    for (int i = 0; i < 3; ++i) Ra[i] = R[i * 3] * a[0] + R[i * 3 + 1] * a[1] + R[i * 3 + 2] * a[2];
    // the accelerometer rows [J 0 R] (3 x 9) and their residual
    double H[3][9], r[3];
    double J[9];
    if (k.left) {   // skew(R a)
        J[0] = 0.0; J[1] = -Ra[2]; J[2] = Ra[1];
        J[3] = Ra[2]; J[4] = 0.0; J[5] = -Ra[0];
        J[6] = -Ra[1]; J[7] = Ra[0]; J[8] = 0.0;
    } else {        // R skew(a)
        const double K[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) J[i * 3 + j] = R[i * 3] * K[j] + R[i * 3 + 1] * K[3 + j] + R[i * 3 + 2] * K[6 + j];
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { H[i][j] = J[i * 3 + j]; H[i][3 + j] = 0.0; H[i][6 + j] = R[i * 3 + j]; }
        r[i] = -Ra[i] - g[i];
    }
    const double wa = dt / k.sigma_a2, wg = dt / k.sigma_w2;   // 1 / (sigma^2 / dt)
    int e = 0;
    for (int i = 0; i < 9; ++i)
        for (int j = i; j < 9; ++j, ++e) {
            double s = (H[0][i] * H[0][j] + H[1][i] * H[1][j] + H[2][i] * H[2][j]) * wa;
            if (i == j && i >= 3 && i < 6) s += wg;   // the gyro rows [0 I 0]: zero residual, but they stay in A
            out[e] = s;
        }
    for (int i = 0; i < 9; ++i) out[ZCHK_B + i] = (H[0][i] * r[0] + H[1][i] * r[1] + H[2][i] * r[2]) * wa;
    out[ZCHK_C] = (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * wa;
    out[ZCHK_DT] = dt;
}

// Pm [81] (row-major) from P (leading dimension ld).  Returns false when one of the 81 entries read is not finite.
ORC_ZCHK_HD bool zupt_check_marginal(const double* P, int ld, double* Pm) {
    bool ok = true;
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) {
            const double u = P[(size_t)zupt_check_state(i) * ld + zupt_check_state(j)], l = P[(size_t)zupt_check_state(j) * ld + zupt_check_state(i)];
            ok = ok && isfinite(u) && isfinite(l);
            Pm[i * 9 + j] = 0.5 * (u + l);
        }
    return ok;
}

// The 9 x 9 part.  Pm [81]: the marginal (symmetric), Q_bias not yet added; sums [56].  Returns ZCHK_OK with *chi2, or the refusal.
ORC_ZCHK_HD int zupt_check_solve(const double* Pm, const double* sums, const ZuptCheckConsts& k, double* chi2) {
    double L[9][9], M[9][9], T[9][9], y[9];
    const double dts = sums[ZCHK_DT];
    // P_m = L L^T (lower)
    for (int j = 0; j < 9; ++j) {
        double d = Pm[j * 9 + j] + (j >= 6 ? dts * k.sigma_ab : (j >= 3 ? dts * k.sigma_wb : 0.0));
        for (int q = 0; q < j; ++q) d -= L[j][q] * L[j][q];
        if (!(d > 0.0) || !isfinite(d)) return ZCHK_P_NOT_SPD;
        const double c = sqrt(d);
        L[j][j] = c;
        for (int i = 0; i < j; ++i) L[i][j] = 0.0;
        for (int i = j + 1; i < 9; ++i) {
            double v = Pm[i * 9 + j];
            for (int q = 0; q < j; ++q) v -= L[i][q] * L[j][q];
            L[i][j] = v / c;
        }
    }
    // T = A L (A symmetric from its packed upper triangle), M = I + L^T T
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) {
            double s = 0.0;
            for (int q = j; q < 9; ++q) s += sums[q >= i ? zupt_check_tri(i, q) : zupt_check_tri(q, i)] * L[q][j];
            T[i][j] = s;
        }
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = i == j ? 1.0 : 0.0;
            for (int q = i; q < 9; ++q) s += L[q][i] * T[q][j];
            M[i][j] = s;
        }
    // y = L^T b
    for (int i = 0; i < 9; ++i) {
        double s = 0.0;
        for (int q = i; q < 9; ++q) s += L[q][i] * sums[ZCHK_B + q];
        y[i] = s;
    }
    // M = C C^T in place (lower), z = C^-1 y, chi^2 = c - |z|^2
    double zz = 0.0;
    for (int j = 0; j < 9; ++j) {
        double d = M[j][j];
        for (int q = 0; q < j; ++q) d -= M[j][q] * M[j][q];
        if (!(d > 0.0) || !isfinite(d)) return ZCHK_M_NOT_SPD;
        const double c = sqrt(d);
        M[j][j] = c;
        for (int i = j + 1; i < 9; ++i) {
            double v = M[i][j];
            for (int q = 0; q < j; ++q) v -= M[i][q] * M[j][q];
            M[i][j] = v / c;
        }
        double v = y[j];
        for (int q = 0; q < j; ++q) v -= M[j][q] * y[q];
        y[j] = v / c;
        zz += y[j] * y[j];
    }
    *chi2 = sums[ZCHK_C] - zz;
    return isfinite(*chi2) ? ZCHK_OK : ZCHK_NOT_FINITE;
}

// All of it on the host.  rows [m][ZCHK_ROW]; P with leading dimension ld (at least 15 x 15).  out3: chi^2 | c | dt_sum.
inline int zupt_check_host(const double* P, int ld, const double* rows, int m, const double* R, const double* ba, const double* g,
                           const ZuptCheckConsts& k, double* out3) {
    double sums[ZCHK_SUMS] = {0.0}, one[ZCHK_SUMS], Pm[81];
    for (int i = 0; i < m; ++i) {
        zupt_check_row(rows + (size_t)i * ZCHK_ROW, R, ba, g, k, one);
        for (int e = 0; e < ZCHK_SUMS; ++e) sums[e] += one[e];
    }
    out3[0] = 0.0; out3[1] = sums[ZCHK_C]; out3[2] = sums[ZCHK_DT];
    if (!zupt_check_marginal(P, ld, Pm)) return ZCHK_NOT_FINITE;
    return zupt_check_solve(Pm, sums, k, out3);
}

}  // namespace orcvio_amd
