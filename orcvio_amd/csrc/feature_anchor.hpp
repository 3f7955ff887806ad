// feature_anchor.hpp -- anchor change of one in-state SLAM feature of the hybrid filter, shared by the HIP kernel
// (device, cov_ops.hpp k_cov_change_anchors) and by a host-compiled unit test of the same inline function.
//
// Follows reference src/orcvio.cpp:
//   pruneImuStateBuffer, in-state features   :2664-2720  (the new parameters the caller sets before the covariance update)
//   updateFeatureCov_3didp                    :3457-3609
//   updateFeatureCov_1didp                    :3611-3774
// Camera pose of a clone from its own pose record: R_w2c = R_b2c R_b2w^T, t_c_w = t_b_w + R_b2w t_c_b (orientation_cam /
// position_cam, :955-961).  R_b2c / t_c_b passed separately are the CURRENT extrinsics (state_server.imu_state), which the
// reference reads for p_old under if_FEJ and for the extrinsic columns.
//
// J row layout (stride 21, idp rows): [0, 3) the feature's own columns (the first idp used), [3, 9) the old anchor clone
// (theta, p), [9, 15) the new anchor clone, [15, 21) the extrinsics (state columns 15..20).
// literal_3d (3-d only): the reference as written -- the "new" pose and column are looked up under old_state_id (:3487, :3544),
// so the Jacobian is evaluated with the old pose in place of the new one and H_x_new lands in the old clone's block, over
// H_x_old; the new clone's block stays zero.  literal_3d = 0: the consistent Jacobian with the new anchor's pose and columns.
#pragma once
#include <cmath>

#include "msckf_math.hpp"

namespace orcvio_amd {

enum { ANCHOR_J_STRIDE = 21, ANCHOR_J_OLD = 3, ANCHOR_J_NEW = 9, ANCHOR_J_EXT = 15 };

// C = A B (3 x 3, row-major)
ORC_HD void am_mul(const double* A, const double* B, double* C) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[a * 3 + b] = A[a * 3 + 0] * B[0 * 3 + b] + A[a * 3 + 1] * B[1 * 3 + b] + A[a * 3 + 2] * B[2 * 3 + b];
}
// C = A^T B
ORC_HD void am_tmul(const double* A, const double* B, double* C) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[a * 3 + b] = A[0 * 3 + a] * B[0 * 3 + b] + A[1 * 3 + a] * B[1 * 3 + b] + A[2 * 3 + a] * B[2 * 3 + b];
}
// C = A B^T
ORC_HD void am_mult(const double* A, const double* B, double* C) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[a * 3 + b] = A[a * 3 + 0] * B[b * 3 + 0] + A[a * 3 + 1] * B[b * 3 + 1] + A[a * 3 + 2] * B[b * 3 + 2];
}
ORC_HD void am_mv(const double* A, const double* x, double* y) {
    for (int a = 0; a < 3; ++a) y[a] = A[a * 3 + 0] * x[0] + A[a * 3 + 1] * x[1] + A[a * 3 + 2] * x[2];
}
ORC_HD void am_tmv(const double* A, const double* x, double* y) {
    for (int a = 0; a < 3; ++a) y[a] = A[0 * 3 + a] * x[0] + A[1 * 3 + a] * x[1] + A[2 * 3 + a] * x[2];
}
ORC_HD void am_skew(const double* w, double* S) {
    S[0] = 0.0;   S[1] = -w[2]; S[2] = w[1];
    S[3] = w[2];  S[4] = 0.0;   S[5] = -w[0];
    S[6] = -w[1]; S[7] = w[0];  S[8] = 0.0;
}
// B = A^-1 by cofactors (the reference takes R_c2w.inverse(), not the transpose, where it maps a point into a camera: the two
// differ by the rotation's departure from orthonormality -- 6e-13 for the EuRoC extrinsics as the YAML gives them)
ORC_HD void am_inv(const double* A, double* B) {
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double id = 1.0 / (A[0] * c00 + A[1] * c01 + A[2] * c02);
    B[0] = c00 * id; B[1] = (A[2] * A[7] - A[1] * A[8]) * id; B[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    B[3] = c01 * id; B[4] = (A[0] * A[8] - A[2] * A[6]) * id; B[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    B[6] = c02 * id; B[7] = (A[1] * A[6] - A[0] * A[7]) * id; B[8] = (A[0] * A[4] - A[1] * A[3]) * id;
}
// a world point in a camera: (R_c2w)^-1 (p - t_c_w), R_c2w = R_w2c^T
ORC_HD void am_to_cam(const double* Rwc, const double* tcw, const double* p, double* out) {
    double Rcw[9], Ri[9], d[3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) Rcw[a * 3 + b] = Rwc[b * 3 + a];
    am_inv(Rcw, Ri);
    for (int a = 0; a < 3; ++a) d[a] = p[a] - tcw[a];
    am_mv(Ri, d, out);
}
// camera pose of a clone record: R_w2c, t_c_w
ORC_HD void am_cam_pose(const double* pose, double* Rwc, double* tcw) {
    am_mult(pose + POSE_R_B2C, pose + POSE_R_B2W, Rwc);
    double r[3];
    am_mv(pose + POSE_R_B2W, pose + POSE_T_C_B, r);
    for (int a = 0; a < 3; ++a) tcw[a] = pose[POSE_T_B_W + a] + r[a];
}

// measurementUpdate_hybrid's increment of ONE in-state feature (:1842-1889): the parameters take their own entries of dx (3-d:
// invParam += dxf[0..2]; 1-d: invDepth += dxf[0], obs_anchor stays), the world position follows from the anchor's camera pose as
// the clones' increment has left it: p_w = R_c2w p_c + t_c_w, p_c = (a, b, 1) / rho.  pose_anchor: the anchor clone's record (its
// own frozen extrinsic).  A rho of zero gives a non-finite p_w: the caller checks it.
ORC_HD void feature_increment(const double* pose_anchor, const double* param, double rho, const double* dxf, int idp_dim, double p_w[3]) {
    double a = param[0], b = param[1], r = rho;
    if (idp_dim == 3) { a += dxf[0]; b += dxf[1]; r = param[2] + dxf[2]; }
    else r += dxf[0];
    const double pc[3] = {a / r, b / r, 1.0 / r};
    double Rwc[9], tcw[3], q[3];
    am_cam_pose(pose_anchor, Rwc, tcw);
    am_tmv(Rwc, pc, q);
    for (int c = 0; c < 3; ++c) p_w[c] = q[c] + tcw[c];
}
// incrementState_IMUCam's extrinsic part (:4512-4517, smallAngleQuaternion math_utils.hpp:104-121, Eigen's toRotationMatrix without
// normalisation): ext = R_b2c 9 | t_c_b 3 of the IMU, de = dx[15:21].  The arithmetic of orcvio_msckf_increment_state (capi_state.inc).
ORC_HD void extrinsic_increment(const double* de, double ext[12]) {
    double q[4] = {0.5 * de[0], 0.5 * de[1], 0.5 * de[2], 0.0};
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
    if (n2 <= 1.0) q[3] = sqrt(1.0 - n2);
    else {
        q[3] = 1.0;
        const double s = 1.0 / sqrt(1.0 + n2);
        for (int c = 0; c < 4; ++c) q[c] *= s;
    }
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double RqT[9] = {1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w),
                           2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w),
                           2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)};
    double R[9];
    am_mul(ext, RqT, R);
    for (int c = 0; c < 9; ++c) ext[c] = R[c];
    for (int c = 0; c < 3; ++c) ext[9 + c] += de[3 + c];
}

// The new parameters (1-d: param = obs_anchor (u, v, 1), rho = invDepth; 3-d: param = invParam (alpha, beta, rho), rho = param[2])
// of a feature at world position p_w in the new anchor's camera frame (:2680-2687, :2700-2712), and its J rows (layout above).
ORC_HD void anchor_change(const double* pose_old, const double* pose_new, const double* R_b2c, const double* t_c_b,
                          const double* p_w, const double* p_fej, int idp_dim, int if_fej, int literal_3d,
                          double param[3], double* rho_out, double J[3 * ANCHOR_J_STRIDE]) {
    for (int q = 0; q < 3 * ANCHOR_J_STRIDE; ++q) J[q] = 0.0;
    double Rwc_o[9], tcw_o[3], Rwc_n[9], tcw_n[3];
    am_cam_pose(pose_old, Rwc_o, tcw_o);
    am_cam_pose(pose_new, Rwc_n, tcw_n);
    // new parameters, from the TRUE new anchor in both 3-d forms
    double p_new[3];
    am_to_cam(Rwc_n, tcw_n, p_w, p_new);
    param[0] = p_new[0] / p_new[2];
    param[1] = p_new[1] / p_new[2];
    param[2] = idp_dim == 3 ? 1.0 / p_new[2] : 1.0;
    const double rho_new = 1.0 / p_new[2];
    *rho_out = rho_new;
    // the pose the Jacobian calls "new": the old one under the 3-d quirk
    const bool lit = idp_dim == 3 && literal_3d;
    const double* pn = lit ? pose_old : pose_new;
    if (lit) { am_cam_pose(pose_old, Rwc_n, tcw_n); }
    const double* Rbw_o = pose_old + POSE_R_B2W;
    const double* Rbw_n = pn + POSE_R_B2W;
    // p_old: the feature in the old camera frame (FEJ: from position_FEJ and the CURRENT extrinsics)
    double p_old_[3], p_old[3];
    am_to_cam(Rwc_o, tcw_o, p_w, p_old_);
    if (if_fej) {
        double e[3], q[3];
        for (int a = 0; a < 3; ++a) e[a] = p_fej[a] - pose_old[POSE_T_FEJ + a];
        am_tmv(Rbw_o, e, q);
        for (int a = 0; a < 3; ++a) q[a] -= t_c_b[a];
        am_mv(R_b2c, q, p_old);
    } else {
        for (int a = 0; a < 3; ++a) p_old[a] = p_old_[a];
    }
    double pbf_o[3], pbf_n[3];
    for (int a = 0; a < 3; ++a) {
        pbf_o[a] = if_fej ? p_fej[a] - pose_old[POSE_T_FEJ + a] : p_w[a] - pose_old[POSE_T_B_W + a];
        pbf_n[a] = if_fej ? p_fej[a] - pn[POSE_T_FEJ + a] : p_w[a] - pn[POSE_T_B_W + a];
    }
    // pieces shared by both forms
    double Jp[9];   // R_w2c_new R_c2w_old
    am_mult(Rwc_n, Rwc_o, Jp);
    double S[9], Jto[9], Jtn[9];
    am_skew(pbf_o, S);
    am_mul(Rwc_n, S, Jto);   // J_theta_old = -Jto
    am_skew(pbf_n, S);
    am_mul(Rwc_n, S, Jtn);   // J_theta_new = Jtn
    double Mn[9], v[3], w[3];   // Mn = R_w2b_new R_b2w_old
    am_tmul(Rbw_n, Rbw_o, Mn);
    am_tmv(Rbw_n, pbf_n, v);
    for (int a = 0; a < 3; ++a) v[a] -= t_c_b[a];
    double SkewMx[9], Mx[9], T[9];
    am_skew(v, SkewMx);
    am_tmv(R_b2c, p_old, w);
    am_skew(w, S);
    am_mul(Mn, S, Mx);
    for (int q = 0; q < 9; ++q) T[q] = SkewMx[q] - Mx[q];
    double Je_t[9], Je_p[9];
    am_mul(R_b2c, T, Je_t);
    for (int q = 0; q < 9; ++q) T[q] = Mn[q] - ((q % 4) == 0 ? 1.0 : 0.0);
    am_mul(R_b2c, T, Je_p);
    if (idp_dim == 1) {
        // :3660-3706, bottom rows (z) of the 3 x 3 blocks
        const double invDepth_old = 1.0 / p_old_[2];
        const double f_old[3] = {p_old_[0] / p_old_[2], p_old_[1] / p_old_[2], 1.0};
        const double J_rho_d_new = -rho_new * rho_new;
        const double J_d = Jp[6] * f_old[0] + Jp[7] * f_old[1] + Jp[8] * f_old[2];
        const double J_d_rho_old = -1.0 / (invDepth_old * invDepth_old);
        J[0] = J_rho_d_new * J_d * J_d_rho_old;
        for (int b = 0; b < 3; ++b) {
            J[ANCHOR_J_OLD + b] = J_rho_d_new * (-Jto[6 + b]);
            J[ANCHOR_J_OLD + 3 + b] = J_rho_d_new * Rwc_n[6 + b];
            J[ANCHOR_J_NEW + b] = J_rho_d_new * Jtn[6 + b];
            J[ANCHOR_J_NEW + 3 + b] = J_rho_d_new * (-Rwc_n[6 + b]);
            J[ANCHOR_J_EXT + b] = J_rho_d_new * Je_t[6 + b];
            J[ANCHOR_J_EXT + 3 + b] = J_rho_d_new * Je_p[6 + b];
        }
        return;
    }
    // 3-d, :3512-3538: H = J_fp_new [J_p J_pf_old | J_x_old | J_x_new | J_e]
    const double* inv = param;
    double Jfp[9] = {1.0, 0.0, -inv[0], 0.0, 1.0, -inv[1], 0.0, 0.0, -inv[2]};
    for (int q = 0; q < 9; ++q) Jfp[q] *= inv[2];
    double Jpf[9] = {1.0, 0.0, -p_old[0], 0.0, 1.0, -p_old[1], 0.0, 0.0, -p_old[2]};
    for (int q = 0; q < 9; ++q) Jpf[q] *= p_old[2];
    double A[9], Hf[9];
    am_mul(Jfp, Jp, A);
    am_mul(A, Jpf, Hf);
    double Hto[9], Hpo[9], Htn[9], Hpn[9], Het[9], Hep[9];
    for (int q = 0; q < 9; ++q) T[q] = -Jto[q];
    am_mul(Jfp, T, Hto);
    am_mul(Jfp, Rwc_n, Hpo);
    am_mul(Jfp, Jtn, Htn);
    for (int q = 0; q < 9; ++q) Hpn[q] = -Hpo[q];
    am_mul(Jfp, Je_t, Het);
    am_mul(Jfp, Je_p, Hep);
    for (int a = 0; a < 3; ++a) {
        double* row = J + a * ANCHOR_J_STRIDE;
        for (int b = 0; b < 3; ++b) {
            row[b] = Hf[a * 3 + b];
            if (lit) {   // H_x_new over H_x_old in the old clone's block; nothing in the new clone's
                row[ANCHOR_J_OLD + b] = Htn[a * 3 + b];
                row[ANCHOR_J_OLD + 3 + b] = Hpn[a * 3 + b];
            } else {
                row[ANCHOR_J_OLD + b] = Hto[a * 3 + b];
                row[ANCHOR_J_OLD + 3 + b] = Hpo[a * 3 + b];
                row[ANCHOR_J_NEW + b] = Htn[a * 3 + b];
                row[ANCHOR_J_NEW + 3 + b] = Hpn[a * 3 + b];
            }
            row[ANCHOR_J_EXT + b] = Het[a * 3 + b];
            row[ANCHOR_J_EXT + 3 + b] = Hep[a * 3 + b];
        }
    }
}

}  // namespace orcvio_amd
