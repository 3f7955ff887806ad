// imu_model.hpp -- the reference's IMU step (batchImuProcessing -> processModel, src/orcvio.cpp:664-823) at leg_dim = 22, in plain
// C++ that compiles for the host and for the device (the guard pattern of msckf_math.hpp, no Eigen).  With calib_imu_instrinsic = 0
// (every shipped YAML) Tg = Ma = I and As = 0: gyro = m_gyro - b_g, acc = m_acc - b_a, and the calib_imu block of calPhiClosedForm
// does not exist.  leg_dim = 46 (calib_imu_instrinsic = 1) has functions of its own at the end of this header: imu_*46.
//
//   imu_propagate_mean   sample selection (:678-709) + one predictor per selected sample: predictNewStateLARVIO (:825-897) or
//                        predictNewStateOrcVIO (:899-928).  HOST: 3-vectors and 3 x 3 matrices.  Leaves one RECORD per sample --
//                        everything Phi_k, G_k need, so that the S pairs (Phi_k, Q_k) are independent of one another.
//   imu_phi              Phi_k (leading 15 x 15) from a record: calPhiEulerMethod (:3952-3978, left and right),
//                        calPhiClosedForm left / LARVIO (:3997-4037) and right (:4308-4367, as written: it divides by |w|^2).
//   imu_noise            N_k = G Q_c G^T dt (:776-798, Q_c diagonal as :429-438 fill it); Q_k = Phi_k N_k Phi_k^T is the reference's Phi G Q_c G^T Phi^T dt.
//   imu_accumulate_host  the ordered product on the host: Phi <- Phi_k Phi, Q <- Phi_k (Q + N_k) Phi_k^T  (= Phi_k Q Phi_k^T + Q_k).
//                        k_imu_phi_q (imu_ops.hpp) does the same on the device from the same records.
//
// Which state each formula reads: calPhiEulerMethod the orientation AFTER the predictor (:3955); calPhiClosedForm and G the state
// BEFORE it (imu_state_old, :3995, :776); the left / LARVIO closed form v_k, p_k, v_k+1, p_k+1 -- under if_FEJ those of the FEJ pair
// (imu_state_FEJ_old / _now, :4003-4014), which the predictors roll (:893-894, :923-924) -- and the PREVIOUS sample's gyro
// measurement (m_gyro_old, :745, :3992), carried from frame to frame by the caller.
#pragma once

#if defined(__HIPCC__)
#define ORC_IMU_HD __host__ __device__ inline
#else
#define ORC_IMU_HD inline
#endif

#include <math.h>

namespace orcvio_amd {

enum { IMU_MAX_SAMPLES = 128, IMU_DIM = 15, IMU_LEG = 22 };
// one record per selected sample (doubles)
enum { IMU_REC_DT = 0, IMU_REC_GYRO = 1, IMU_REC_ACC = 4, IMU_REC_GYRO_OLD = 7, IMU_REC_R_OLD = 10, IMU_REC_R_NEW = 19,
       IMU_REC_VK = 28, IMU_REC_PK = 31, IMU_REC_VK1 = 34, IMU_REC_PK1 = 37, IMU_REC = 40 };

struct ImuFlags {
    int use_larvio, use_left, use_closed_form, if_fej;
};

// ---- 3 x 3 helpers (row-major) ---------------------------------------------------------------------------------------------------
ORC_IMU_HD void m3_mul(const double* A, const double* B, double* C) {   // C = A B (C may not alias)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
ORC_IMU_HD void m3_mulv(const double* A, const double* x, double* y) {
    for (int i = 0; i < 3; ++i) y[i] = A[i * 3] * x[0] + A[i * 3 + 1] * x[1] + A[i * 3 + 2] * x[2];
}
ORC_IMU_HD void m3_skew(const double* w, double* S) {   // skewSymmetric, math_utils.hpp:27-39
    S[0] = 0.0; S[1] = -w[2]; S[2] = w[1];
    S[3] = w[2]; S[4] = 0.0; S[5] = -w[0];
    S[6] = -w[1]; S[7] = w[0]; S[8] = 0.0;
}
ORC_IMU_HD void m3_eye(double* A, double s) {
    for (int i = 0; i < 9; ++i) A[i] = 0.0;
    A[0] = A[4] = A[8] = s;
}
ORC_IMU_HD double v3_norm(const double* w) { return sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]); }
ORC_IMU_HD void v3_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// Eigen::Quaterniond(w, x, y, z).toRotationMatrix(): no normalisation
ORC_IMU_HD void quat_wxyz_to_matrix(double w, double x, double y, double z, double* R) {
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
// Sophus SO3d::exp: the unit quaternion of the rotation vector, then its matrix
ORC_IMU_HD void imu_so3_exp(const double* w, double* R) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double th = sqrt(th2);
    double imag, real;
    if (th < 1e-10) {
        const double th4 = th2 * th2;
        imag = 0.5 - th2 / 48.0 + th4 / 3840.0;
        real = 1.0 - th2 / 8.0 + th4 / 384.0;
    } else {
        imag = sin(0.5 * th) / th;
        real = cos(0.5 * th);
    }
    quat_wxyz_to_matrix(real, imag * w[0], imag * w[1], imag * w[2], R);
}
// quaternionToRotation / rotationToQuaternion (math_utils.hpp:164-227), q = [x, y, z, w]
ORC_IMU_HD void quat_to_rotation(const double* q, double* R) {
    const double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
    R[0] = 1 - 2 * (qy * qy + qz * qz); R[1] = 2 * (qx * qy - qw * qz); R[2] = 2 * (qx * qz + qw * qy);
    R[3] = 2 * (qx * qy + qw * qz); R[4] = 1 - 2 * (qx * qx + qz * qz); R[5] = 2 * (qy * qz - qw * qx);
    R[6] = 2 * (qx * qz - qw * qy); R[7] = 2 * (qy * qz + qw * qx); R[8] = 1 - 2 * (qx * qx + qy * qy);
}
ORC_IMU_HD void rotation_to_quat(const double* R, double* q) {
    const double tr = R[0] + R[4] + R[8];
    const double score[4] = {R[0], R[4], R[8], tr};
    int m = 0;
    for (int i = 1; i < 4; ++i)
        if (score[i] > score[m]) m = i;   // (maxCoeff: the first of equal maxima)
    if (m == 0) {
        q[0] = sqrt(1 + 2 * R[0] - tr) / 2.0;
        q[1] = (R[1] + R[3]) / (4 * q[0]); q[2] = (R[2] + R[6]) / (4 * q[0]); q[3] = (R[7] - R[5]) / (4 * q[0]);
    } else if (m == 1) {
        q[1] = sqrt(1 + 2 * R[4] - tr) / 2.0;
        q[0] = (R[1] + R[3]) / (4 * q[1]); q[2] = (R[5] + R[7]) / (4 * q[1]); q[3] = (R[2] - R[6]) / (4 * q[1]);
    } else if (m == 2) {
        q[2] = sqrt(1 + 2 * R[8] - tr) / 2.0;
        q[0] = (R[2] + R[6]) / (4 * q[2]); q[1] = (R[5] + R[7]) / (4 * q[2]); q[3] = (R[3] - R[1]) / (4 * q[2]);
    } else {
        q[3] = sqrt(1 + tr) / 2.0;
        q[0] = (R[7] - R[5]) / (4 * q[3]); q[1] = (R[2] - R[6]) / (4 * q[3]); q[2] = (R[3] - R[1]) / (4 * q[3]);
    }
    if (q[3] < 0)
        for (int i = 0; i < 4; ++i) q[i] = -q[i];
    const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] = q[i] / nrm;
}
// Hl_operator / Jl_operator (math_utils.hpp:230-270), their < 1e-5 branches
ORC_IMU_HD void imu_Hl(const double* g, double* H) {
    const double n = v3_norm(g);
    m3_eye(H, 0.5);
    if (n < 1.0e-5) return;
    double S[9], SS[9];
    m3_skew(g, S);
    m3_mul(S, S, SS);
    const double c2 = (n - sin(n)) / pow(n, 3), c3 = (2 * (cos(n) - 1) + pow(n, 2)) / (2 * pow(n, 4));
    for (int i = 0; i < 9; ++i) H[i] = H[i] + c2 * S[i] + c3 * SS[i];
}
ORC_IMU_HD void imu_Jl(const double* g, double* J) {
    const double n = v3_norm(g);
    m3_eye(J, 1.0);
    if (n < 1.0e-5) return;
    double S[9], cS[9], SS[9];
    m3_skew(g, S);
    const double c2 = (1 - cos(n)) / pow(n, 2), c3 = (n - sin(n)) / pow(n, 3);
    for (int i = 0; i < 9; ++i) cS[i] = c3 * S[i];
    m3_mul(cS, S, SS);   // (scalar * skew * skew, left to right as the reference writes it)
    for (int i = 0; i < 9; ++i) J[i] = J[i] + c2 * S[i] + SS[i];
}

// ---- Phi_k --------------------------------------------------------------------------------------------------------------------------
// Only nine 3 x 3 blocks of Phi_k ever differ from the identity's (calib_imu off): (theta, theta) (theta, b_g) (v, theta) (v, b_g)
// (v, b_a) (p, theta) (p, v) (p, b_g) (p, b_a).  imu_block numbers them 0..8 by block row / block column, -1 for every other block.
ORC_IMU_HD int imu_block(int bi, int bj) {
    switch (bi * 5 + bj) {
        case 0: return 0;
        case 3: return 1;
        case 5: return 2;
        case 8: return 3;
        case 9: return 4;
        case 10: return 5;
        case 11: return 6;
        case 13: return 7;
        case 14: return 8;
        default: return -1;
    }
}
enum { IMU_PHI_BLOCKS = 9, IMU_COMPACT_PHI = 81, IMU_COMPACT_N00 = 81, IMU_COMPACT_N11 = 90, IMU_COMPACT_ND = 99, IMU_COMPACT = 105 };
// where imu_phi puts its blocks: a dense [15][ld] matrix (host), or the compact record [block][3][3] (device, LDS)
struct ImuDenseSink {
    double* Phi; int ld;
    ORC_IMU_HD void init() {
        for (int i = 0; i < IMU_DIM; ++i)
            for (int j = 0; j < IMU_DIM; ++j) Phi[i * ld + j] = i == j ? 1.0 : 0.0;
    }
    ORC_IMU_HD void put(int r, int c, const double* B, double s) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Phi[(r + i) * ld + c + j] = s * B[i * 3 + j];
    }
};
struct ImuCompactSink {
    double* c;
    ORC_IMU_HD void init() {
        for (int i = 0; i < IMU_COMPACT_PHI; ++i) c[i] = 0.0;
        c[0] = c[4] = c[8] = 1.0;   // (theta, theta) is the one diagonal block among the nine
    }
    ORC_IMU_HD void put(int r, int cc, const double* B, double s) {
        const int b = imu_block(r / 3, cc / 3);
        for (int i = 0; i < 9; ++i) c[b * 9 + i] = s * B[i];
    }
};
// the leading 15 x 15 block of Phi_k; rows / columns 15 .. 21 of the reference's matrix are the identity's
template <class Sink>
ORC_IMU_HD void imu_phi(const double* rec, ImuFlags f, const double* grav, Sink& out) {
    out.init();
    const double dt = rec[IMU_REC_DT];
    const double* gyro = rec + IMU_REC_GYRO;
    const double* acc = rec + IMU_REC_ACC;
    double I3[9];
    m3_eye(I3, 1.0);
    if (!(f.use_larvio || f.use_closed_form)) {   // calPhiEulerMethod: the orientation AFTER the predictor
        const double* wRi = rec + IMU_REC_R_NEW;
        double S[9], T[9];
        if (f.use_left) {
            double Ra[3];
            m3_mulv(wRi, acc, Ra);
            m3_skew(Ra, S);
            out.put(0, 9, wRi, -dt);
            out.put(3, 0, S, -dt);
        } else {
            m3_skew(gyro, S);
            for (int i = 0; i < 9; ++i) T[i] = I3[i] - dt * S[i];
            out.put(0, 0, T, 1.0);
            out.put(0, 9, I3, -dt);
            m3_skew(acc, S);
            m3_mul(wRi, S, T);
            out.put(3, 0, T, -dt);
        }
        out.put(3, 12, wRi, -dt);
        out.put(6, 3, I3, dt);
        return;
    }
    const double* C = rec + IMU_REC_R_OLD;   // imu_state_old.orientation
    if (f.use_larvio || f.use_left) {
        const double* go = rec + IMU_REC_GYRO_OLD;
        const double *vk = rec + IMU_REC_VK, *pk = rec + IMU_REC_PK, *vk1 = rec + IMU_REC_VK1, *pk1 = rec + IMU_REC_PK1;
        double cr[3], aa[3], Ah[9];
        v3_cross(go, gyro, cr);
        for (int i = 0; i < 3; ++i) aa[i] = dt * (go[i] + gyro[i]) / 2 + dt * dt * cr[i] / 12;
        m3_skew(aa, Ah);
        double M[9], T[9], U[9], S[9], w[3];
        // Phi_q_bg = -0.5 C (2 I + Ah) dt  (Tg = I);  Phi_q_ba = 0  (TA = 0)
        for (int i = 0; i < 9; ++i) M[i] = 2 * I3[i] + Ah[i];
        m3_mul(C, M, T);                                   // T = C (2 I + Ah)
        out.put(0, 9, T, -0.5 * dt);
        // Phi_v_q
        for (int i = 0; i < 3; ++i) w[i] = vk1[i] - vk[i] - grav[i] * dt;
        m3_skew(w, S);
        out.put(3, 0, S, -1.0);
        // Phi_v_bg
        for (int i = 0; i < 3; ++i) w[i] = -pk1[i] + pk[i] + vk1[i] * dt - 0.5 * grav[i] * dt * dt;
        m3_skew(w, S);
        m3_mul(S, C, U);
        for (int i = 0; i < 3; ++i) w[i] = -0.5 * pk1[i] + 0.5 * pk[i] + 0.5 * vk1[i] * dt - grav[i] * dt * dt / 6;
        m3_skew(w, S);
        m3_mul(S, C, M);
        m3_mul(M, Ah, S);
        for (int i = 0; i < 9; ++i) U[i] = U[i] + S[i];
        out.put(3, 9, U, 1.0);
        // Phi_v_ba = -0.5 C (2 I + Ah) dt  (Ma = I, TA = 0)
        out.put(3, 12, T, -0.5 * dt);
        // Phi_p_q
        for (int i = 0; i < 3; ++i) w[i] = pk1[i] - pk[i] - vk[i] * dt - 0.5 * grav[i] * dt * dt;
        m3_skew(w, S);
        out.put(6, 0, S, -1.0);
        out.put(6, 3, I3, dt);
        // Phi_p_bg = -dt^3 skew(g) C / 6 + dt skew(pk1 - pk - g dt^2 / 6) C Ah / 4
        m3_skew(grav, S);
        m3_mul(S, C, U);
        for (int i = 0; i < 3; ++i) w[i] = pk1[i] - pk[i] - grav[i] * dt * dt / 6;
        m3_skew(w, S);
        m3_mul(S, C, M);
        m3_mul(M, Ah, S);
        for (int i = 0; i < 9; ++i) U[i] = -dt * dt * dt * U[i] / 6 + dt * S[i] / 4;
        out.put(6, 9, U, 1.0);
        // Phi_p_ba = -C (3 I + Ah) dt^2 / 6
        for (int i = 0; i < 9; ++i) M[i] = 3 * I3[i] + Ah[i];
        m3_mul(C, M, T);
        out.put(6, 12, T, -(dt * dt) / 6);
        return;
    }
    // right closed form, as written (:4308-4367): the b_g blocks divide by |gyro|^2 -- a zero gyro gives a non-finite Phi
    const double* wRi = C;
    double aS[9], gS[9], gg[9], T[9], U[9], V[9], W[9], w[3];
    m3_skew(acc, aS);
    m3_skew(gyro, gS);
    const double gn = v3_norm(gyro);
    const double gn2 = gn * gn;
    double tt[9], JLp[9], JLm[9], HLp[9], HLm[9], Delta[9], K[9];
    for (int i = 0; i < 3; ++i) w[i] = -dt * gyro[i];
    imu_so3_exp(w, tt);
    imu_Jl(w, JLm);
    imu_Hl(w, HLm);
    for (int i = 0; i < 3; ++i) w[i] = dt * gyro[i];
    imu_Jl(w, JLp);
    imu_Hl(w, HLp);
    // Delta = -(gS / gn2) (tt^T (dt gS - I) + I)
    for (int i = 0; i < 9; ++i) T[i] = dt * gS[i] - I3[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) U[i * 3 + j] = tt[0 * 3 + i] * T[0 * 3 + j] + tt[1 * 3 + i] * T[1 * 3 + j] + tt[2 * 3 + i] * T[2 * 3 + j] + I3[i * 3 + j];
    for (int i = 0; i < 9; ++i) T[i] = -(gS[i] / gn2);
    m3_mul(T, U, Delta);
    // K = I + gS gS / gn2
    m3_mul(gS, gS, gg);
    for (int i = 0; i < 9; ++i) K[i] = I3[i] + gg[i] / gn2;
    // theta row
    out.put(0, 0, tt, 1.0);
    out.put(0, 9, JLm, -dt);
    // v_theta = -dt wRi skew(JLp acc)
    m3_mulv(JLp, acc, w);
    m3_skew(w, T);
    m3_mul(wRi, T, U);
    out.put(3, 0, U, -dt);
    // ag = aS gS / gn2,  ga = gyro acc^T / gn2,  adg = acc . gyro
    double ag[9], ga[9];
    m3_mul(aS, gS, ag);
    for (int i = 0; i < 9; ++i) ag[i] = ag[i] / gn2;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) ga[i * 3 + j] = gyro[i] * acc[j] / gn2;
    const double adg = acc[0] * gyro[0] + acc[1] * gyro[1] + acc[2] * gyro[2];
    // v_gyro = wRi Delta aS K + dt wRi JLp ag + dt wRi ga JLm - dt (adg / gn2) I
    m3_mul(wRi, Delta, T);
    m3_mul(T, aS, U);
    m3_mul(U, K, V);                         // V = wRi Delta aS K
    m3_mul(wRi, JLp, T);
    m3_mul(T, ag, U);                        // U = wRi JLp ag
    m3_mul(wRi, ga, T);
    m3_mul(T, JLm, W);                       // W = wRi ga JLm
    for (int i = 0; i < 9; ++i) V[i] = V[i] + dt * U[i] + dt * W[i] - dt * (adg / gn2) * I3[i];
    out.put(3, 9, V, 1.0);
    // v_acc = -dt wRi JLp
    m3_mul(wRi, JLp, T);
    out.put(3, 12, T, -dt);
    // p_theta = -dt^2 wRi skew(HLp acc)
    m3_mulv(HLp, acc, w);
    m3_skew(w, T);
    m3_mul(wRi, T, U);
    out.put(6, 0, U, -(dt * dt));
    out.put(6, 3, I3, dt);
    // p_gyro = wRi (-gS Delta - dt JLp + dt I) aS K (gS / gn2) + dt^2 wRi HLp ag + dt^2 wRi ga HLm - dt^2 (adg / (2 gn2)) wRi
    m3_mul(gS, Delta, T);
    for (int i = 0; i < 9; ++i) T[i] = -T[i] - dt * JLp[i] + dt * I3[i];
    m3_mul(wRi, T, U);
    m3_mul(U, aS, T);
    m3_mul(T, K, U);
    for (int i = 0; i < 9; ++i) T[i] = gS[i] / gn2;
    m3_mul(U, T, V);                         // V = first term
    m3_mul(wRi, HLp, T);
    m3_mul(T, ag, U);                        // U = wRi HLp ag
    m3_mul(wRi, ga, T);
    m3_mul(T, HLm, W);                       // W = wRi ga HLm
    for (int i = 0; i < 9; ++i) V[i] = V[i] + dt * dt * U[i] + dt * dt * W[i] - dt * dt * (adg / (2 * gn2)) * wRi[i];
    out.put(6, 9, V, 1.0);
    // p_acc = -dt^2 wRi HLp
    m3_mul(wRi, HLp, T);
    out.put(6, 12, T, -(dt * dt));
}

// N_k = G Q_c G^T dt with G of :776-794 and the DIAGONAL Q_c of :429-438 (qc [12]: gyro, acc, gyro bias, acc bias, three each).  G's
// blocks are -C (or -I), -C, I, I on block rows theta, v, b_g, b_a, so N_k is block diagonal:
//   nc [24] = N(theta, theta) [3][3] | N(v, v) [3][3] | diag N(b_g, b_g) [3] | diag N(b_a, b_a) [3]
ORC_IMU_HD void imu_noise(const double* rec, ImuFlags f, const double* qc, double* nc) {
    const double dt = rec[IMU_REC_DT];
    const double* C = rec + IMU_REC_R_OLD;
    const bool rot0 = f.use_larvio || f.use_left;   // G(0:3, 0:3) = -C (left / LARVIO) or -I (right)
    for (int b = 0; b < 2; ++b)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double s;
                if (b == 0 && !rot0) s = i == j ? qc[i] : 0.0;
                else s = C[i * 3] * qc[3 * b] * C[j * 3] + C[i * 3 + 1] * qc[3 * b + 1] * C[j * 3 + 1] + C[i * 3 + 2] * qc[3 * b + 2] * C[j * 3 + 2];
                nc[9 * b + i * 3 + j] = s * dt;
            }
    for (int i = 0; i < 6; ++i) nc[18 + i] = qc[6 + i] * dt;
}
// element (i, j) of N_k, i, j < 15, from the compact form
ORC_IMU_HD double imu_noise_at(const double* nc, int i, int j) {
    if (i < 6 && j < 6) return (i / 3 == j / 3) ? nc[9 * (i / 3) + (i % 3) * 3 + j % 3] : 0.0;
    if (i >= 9 && i == j) return nc[18 + i - 9];
    return 0.0;
}

// ---- the mean propagation (host) ----------------------------------------------------------------------------------------------------
struct ImuMeanState {   // state_server.imu_state, and the velocity / position of imu_state_FEJ_now
    double time;
    double R[9], v[3], p[3], bg[3], ba[3];
    double v_fej[3], p_fej[3];
};
struct ImuModelConfig {
    ImuFlags flags;
    double gravity[3];
    double imu_img_time_th;
};
struct ImuBatchInfo {
    int n_used, n_propagated;
    double dt, mean_sforce[3];
};

// predictNewStateLARVIO (:825-897) on R, v, p
inline void imu_predict_larvio(double dt, const double* gyro, const double* acc, const double* grav, double* R, double* v, double* p) {
    const double gn = v3_norm(gyro);
    // Omega = [[-skew(gyro), gyro], [-gyro^T, 0]]
    double Om[16] = {0};
    double S[9];
    m3_skew(gyro, S);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Om[i * 4 + j] = -S[i * 3 + j];
        Om[i * 4 + 3] = gyro[i];
        Om[3 * 4 + i] = -gyro[i];
    }
    double q[4];
    rotation_to_quat(R, q);
    double dq[4], dq2[4];
    auto apply = [&](double cI, double cO, double post, double* out) {   // out = ((cI I + cO Omega) post) q
        for (int i = 0; i < 4; ++i) {
            double s = 0.0;
            for (int j = 0; j < 4; ++j) s += (((i == j ? cI : 0.0) + cO * Om[i * 4 + j]) * post) * q[j];
            out[i] = s;
        }
    };
    if (gn > 1e-5) {
        apply(cos(gn * dt * 0.5), 1 / gn * sin(gn * dt * 0.5), 1.0, dq);
        apply(cos(gn * dt * 0.25), 1 / gn * sin(gn * dt * 0.25), 1.0, dq2);
    } else {
        apply(1.0, 0.5 * dt, cos(gn * dt * 0.5), dq);
        apply(1.0, 0.25 * dt, cos(gn * dt * 0.25), dq2);
    }
    double dR[9], dR2[9], R0[9];
    quat_wxyz_to_matrix(dq[3], dq[0], dq[1], dq[2], dR);
    quat_wxyz_to_matrix(dq2[3], dq2[0], dq2[1], dq2[2], dR2);
    quat_wxyz_to_matrix(q[3], q[0], q[1], q[2], R0);
    double k1[3], k2[3], k4[3], t[3];
    m3_mulv(R0, acc, t);  for (int i = 0; i < 3; ++i) k1[i] = t[i] + grav[i];
    m3_mulv(dR2, acc, t); for (int i = 0; i < 3; ++i) k2[i] = t[i] + grav[i];   // (k3_v_dot == k2_v_dot, :874)
    m3_mulv(dR, acc, t);  for (int i = 0; i < 3; ++i) k4[i] = t[i] + grav[i];
    for (int i = 0; i < 3; ++i) {
        const double k1p = v[i], k2p = v[i] + k1[i] * dt / 2, k3p = v[i] + k2[i] * dt / 2, k4p = v[i] + k2[i] * dt;
        const double vn = v[i] + dt / 6 * (k1[i] + 2 * k2[i] + 2 * k2[i] + k4[i]);
        p[i] = p[i] + dt / 6 * (k1p + 2 * k2p + 2 * k3p + k4p);
        v[i] = vn;
    }
    const double nrm = sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
    for (int i = 0; i < 4; ++i) q[i] = dq[i] / nrm;
    quat_to_rotation(q, R);
}
// predictNewStateOrcVIO (:899-928)
inline void imu_predict_orcvio(double dt, const double* gyro, const double* acc, const double* grav, double* R, double* v, double* p) {
    double w[3] = {dt * gyro[0], dt * gyro[1], dt * gyro[2]};
    double Hl[9], Jl[9], T[9], E[9], x[3];
    imu_Hl(w, Hl);
    m3_mul(R, Hl, T);
    m3_mulv(T, acc, x);
    for (int i = 0; i < 3; ++i) p[i] = p[i] + dt * v[i] + grav[i] * (dt * dt / 2) + x[i] * (dt * dt);
    imu_Jl(w, Jl);
    m3_mul(R, Jl, T);
    m3_mulv(T, acc, x);
    for (int i = 0; i < 3; ++i) v[i] = v[i] + grav[i] * dt + x[i] * dt;
    imu_so3_exp(w, E);
    m3_mul(R, E, T);
    for (int i = 0; i < 9; ++i) R[i] = T[i];
}

// batchImuProcessing's loop.  samples [n][7]: t | gyro | acc;  prev_meas [6]: m_gyro_old | m_acc_old, in and out;  recs [<= cap][IMU_REC].
// Returns false (state, prev_meas untouched, info filled) when more than `cap` samples are selected.
inline bool imu_propagate_mean(const ImuModelConfig& c, ImuMeanState* st, double* prev_meas, const double* samples, int n, double time_bound,
                               double* recs, int cap, ImuBatchInfo* info) {
    // selection first: it depends on state.time before the call and on the sample times only
    int used = 0, count = 0;
    double dt_img = 0.0, cur = st->time;
    for (int k = 0; k < n; ++k) {
        const double t = samples[k * 7];
        if (t <= cur) { ++used; continue; }   // (also a sample out of order behind a processed one: imu_state.time has moved on)
        if (t - time_bound > c.imu_img_time_th) break;
        ++count; ++used;
        dt_img = t - time_bound;
        cur = t;
    }
    info->n_used = used; info->n_propagated = count; info->dt = dt_img;
    info->mean_sforce[0] = info->mean_sforce[1] = info->mean_sforce[2] = 0.0;
    if (count > cap) return false;
    double sum[3] = {0, 0, 0};
    int s = 0;
    for (int k = 0; k < n && s < count; ++k) {
        const double* row = samples + k * 7;
        const double t = row[0];
        if (t <= st->time) continue;
        double* rec = recs + (size_t)s * IMU_REC;
        const double dt = t - st->time;
        rec[IMU_REC_DT] = dt;
        for (int i = 0; i < 3; ++i) {
            rec[IMU_REC_GYRO + i] = row[1 + i] - st->bg[i];
            rec[IMU_REC_ACC + i] = row[4 + i] - st->ba[i];
            rec[IMU_REC_GYRO_OLD + i] = prev_meas[i] - st->bg[i];
            rec[IMU_REC_VK + i] = c.flags.if_fej ? st->v_fej[i] : st->v[i];
            rec[IMU_REC_PK + i] = c.flags.if_fej ? st->p_fej[i] : st->p[i];
        }
        for (int i = 0; i < 9; ++i) rec[IMU_REC_R_OLD + i] = st->R[i];
        if (!c.flags.use_larvio) imu_predict_orcvio(dt, rec + IMU_REC_GYRO, rec + IMU_REC_ACC, c.gravity, st->R, st->v, st->p);
        else imu_predict_larvio(dt, rec + IMU_REC_GYRO, rec + IMU_REC_ACC, c.gravity, st->R, st->v, st->p);
        for (int i = 0; i < 3; ++i) { st->v_fej[i] = st->v[i]; st->p_fej[i] = st->p[i]; }   // imu_state_FEJ_now = imu_state
        for (int i = 0; i < 9; ++i) rec[IMU_REC_R_NEW + i] = st->R[i];
        for (int i = 0; i < 3; ++i) { rec[IMU_REC_VK1 + i] = st->v[i]; rec[IMU_REC_PK1 + i] = st->p[i]; }
        st->time = t;
        for (int i = 0; i < 6; ++i) prev_meas[i] = row[1 + i];
        for (int i = 0; i < 3; ++i) sum[i] += row[4 + i];
        ++s;
    }
    if (count > 0)
        for (int i = 0; i < 3; ++i) info->mean_sforce[i] = sum[i] / count;
    return true;
}

// C [15][15] = A B, all row-major 15 x 15
inline void imu_mul15(const double* A, const double* B, double* C) {
    for (int i = 0; i < IMU_DIM; ++i)
        for (int j = 0; j < IMU_DIM; ++j) {
            double s = 0.0;
            for (int k = 0; k < IMU_DIM; ++k) s += A[i * IMU_DIM + k] * B[k * IMU_DIM + j];
            C[i * IMU_DIM + j] = s;
        }
}
// The ordered product on the host.  Phi, Q [22][22] out; per-sample pairs (leading 15 x 15) into Phi_k / Q_k when not NULL.
inline void imu_accumulate_host(const double* recs, int S, ImuFlags f, const double* grav, const double* qc, double* Phi, double* Q,
                                double* Phi_k = nullptr, double* Q_k = nullptr) {
    double A[IMU_DIM * IMU_DIM], B[IMU_DIM * IMU_DIM], P[IMU_DIM * IMU_DIM], N[IMU_DIM * IMU_DIM], T[IMU_DIM * IMU_DIM], U[IMU_DIM * IMU_DIM];
    for (int i = 0; i < IMU_DIM * IMU_DIM; ++i) { A[i] = (i / IMU_DIM == i % IMU_DIM) ? 1.0 : 0.0; B[i] = 0.0; }
    for (int k = 0; k < S; ++k) {
        const double* rec = recs + (size_t)k * IMU_REC;
        ImuDenseSink sink{P, IMU_DIM};
        imu_phi(rec, f, grav, sink);
        double nc[24];
        imu_noise(rec, f, qc, nc);
        for (int i = 0; i < IMU_DIM; ++i)
            for (int j = 0; j < IMU_DIM; ++j) N[i * IMU_DIM + j] = imu_noise_at(nc, i, j);
        if (Phi_k) for (int i = 0; i < IMU_DIM * IMU_DIM; ++i) Phi_k[(size_t)k * IMU_DIM * IMU_DIM + i] = P[i];
        if (Q_k) {   // Q_k = Phi_k N_k Phi_k^T
            imu_mul15(P, N, T);
            for (int i = 0; i < IMU_DIM; ++i)
                for (int j = 0; j < IMU_DIM; ++j) {
                    double s = 0.0;
                    for (int l = 0; l < IMU_DIM; ++l) s += T[i * IMU_DIM + l] * P[j * IMU_DIM + l];
                    Q_k[(size_t)k * IMU_DIM * IMU_DIM + i * IMU_DIM + j] = s;
                }
        }
        for (int i = 0; i < IMU_DIM * IMU_DIM; ++i) U[i] = B[i] + N[i];
        imu_mul15(P, U, T);                                 // T = Phi_k (Q + N_k)
        for (int i = 0; i < IMU_DIM; ++i)
            for (int j = 0; j < IMU_DIM; ++j) {
                double s = 0.0;
                for (int l = 0; l < IMU_DIM; ++l) s += T[i * IMU_DIM + l] * P[j * IMU_DIM + l];
                B[i * IMU_DIM + j] = s;
            }
        imu_mul15(P, A, T);
        for (int i = 0; i < IMU_DIM * IMU_DIM; ++i) A[i] = T[i];
    }
    for (int i = 0; i < IMU_LEG; ++i)
        for (int j = 0; j < IMU_LEG; ++j) {
            const bool in = i < IMU_DIM && j < IMU_DIM;
            Phi[i * IMU_LEG + j] = in ? A[i * IMU_DIM + j] : (i == j ? 1.0 : 0.0);
            Q[i * IMU_LEG + j] = in ? 0.5 * (B[i * IMU_DIM + j] + B[j * IMU_DIM + i]) : 0.0;
        }
}

// =====================================================================================================================================
// leg_dim = 46 (calib_imu_instrinsic = 1): the 24 IMU intrinsics T1 T2 T3 A1 A2 A3 M1 M2 (three each) are error-state columns 22 .. 45.
//   imu_intrinsic_matrices  updateImuMx (:4373-4418): Tg, As from the triples, Ma lower triangular (M1 strict lower part, M2 diagonal)
//   imu_measurement46       :733-746: f = m_acc - b_a, acc = Ma f, w = m_gyro - As acc - b_g, gyro = Tg w (the predictors get gyro, acc)
//   imu_propagate_mean46    imu_propagate_mean on the corrected gyro, acc; records of IMU_REC46 doubles: today's 40 (gyro, acc and
//                           gyro_old are the corrected ones) and f, w, f_old, w_old, acc_old behind them
//   imu_phi46_lead          the leading 15 x 15: the left / LARVIO closed form with Tg, TA = Tg As, Ma (:4016-4037; a tenth block,
//                           (theta, b_a), is no longer zero); the Euler forms and the right closed form are imu_phi's (they write no
//                           intrinsic block and read no intrinsic matrix, :3952-3978, :4308-4367: as written)
//   imu_phi46_triple        one of the eight 9 x 3 column groups Phi_k[0:9, 22 + 3 j : 25 + 3 j] of the left / LARVIO closed form (:4039-4305)
//   imu_accumulate_host46   Phi, Q [46][46] on the host.  Rows 15 .. 45 of every Phi_k are identity rows and G has nothing below row 15:
//                           Q lives in the leading 15 x 15 (today's recursion) and Phi = [[A, B], [0, I]], A <- A_k A, B <- A_k B + B_k
//                           with B [15][24] (its columns 22 .. 45 of Phi), B_k non-zero in rows 0 .. 8 only.
// Not at 46: the armed form (orcvio_msckf_io_propagate_imu) and the zero-velocity check (checkZUPTIMU reads Ma, As, Tg too, :3184-3188).
enum { IMU_LEG46 = 46, IMU_NI = 24, IMU_TRIPLES = 8 };
enum { IMU_REC_F = 40, IMU_REC_W = 43, IMU_REC_F_OLD = 46, IMU_REC_W_OLD = 49, IMU_REC_ACC_OLD = 52, IMU_REC46 = 55 };
// a sample's compact form at 46: ten 3 x 3 blocks | N_k (24) | B_k [9][24]
enum { IMU_PHI_BLOCKS46 = 10, IMU_COMPACT46_N00 = 90, IMU_COMPACT46_ND = 108, IMU_COMPACT46_B = 114, IMU_COMPACT46 = 330 };

struct ImuIntrinsicMx { double Tg[9], As[9], Ma[9], TA[9]; };   // TA = Tg As (:4000)

ORC_IMU_HD void imu_intrinsic_matrices(const double* x, double* Tg, double* As, double* Ma) {
    const double *T1 = x, *T2 = x + 3, *T3 = x + 6, *A1 = x + 9, *A2 = x + 12, *A3 = x + 15, *M1 = x + 18, *M2 = x + 21;
    Tg[0] = T2[0]; Tg[1] = T3[0]; Tg[2] = T3[1];
    Tg[3] = T1[0]; Tg[4] = T2[1]; Tg[5] = T3[2];
    Tg[6] = T1[1]; Tg[7] = T1[2]; Tg[8] = T2[2];
    As[0] = A2[0]; As[1] = A3[0]; As[2] = A3[1];
    As[3] = A1[0]; As[4] = A2[1]; As[5] = A3[2];
    As[6] = A1[1]; As[7] = A1[2]; As[8] = A2[2];
    Ma[0] = M2[0]; Ma[1] = 0.0;   Ma[2] = 0.0;
    Ma[3] = M1[0]; Ma[4] = M2[1]; Ma[5] = 0.0;
    Ma[6] = M1[1]; Ma[7] = M1[2]; Ma[8] = M2[2];
}
ORC_IMU_HD void imu_intrinsic_mx(const double* x, ImuIntrinsicMx* m) {
    imu_intrinsic_matrices(x, m->Tg, m->As, m->Ma);
    m3_mul(m->Tg, m->As, m->TA);
}
ORC_IMU_HD void imu_measurement46(const double* m_gyro, const double* m_acc, const double* bg, const double* ba, const ImuIntrinsicMx& m,
                                  double* f, double* w, double* acc, double* gyro) {
    double t[3];
    for (int i = 0; i < 3; ++i) f[i] = m_acc[i] - ba[i];
    m3_mulv(m.Ma, f, acc);
    m3_mulv(m.As, acc, t);
    for (int i = 0; i < 3; ++i) w[i] = m_gyro[i] - t[i] - bg[i];
    m3_mulv(m.Tg, w, gyro);
}

// the ten blocks: imu_block's nine, and (theta, b_a) as the tenth
ORC_IMU_HD int imu_block46(int bi, int bj) { return (bi == 0 && bj == 4) ? 9 : imu_block(bi, bj); }
struct ImuCompactSink46 {
    double* c;
    ORC_IMU_HD void init() {
        for (int i = 0; i < 9 * IMU_PHI_BLOCKS46; ++i) c[i] = 0.0;
        c[0] = c[4] = c[8] = 1.0;
    }
    ORC_IMU_HD void put(int r, int cc, const double* B, double s) {
        const int b = imu_block46(r / 3, cc / 3);
        for (int i = 0; i < 9; ++i) c[b * 9 + i] = s * B[i];
    }
};

template <class Sink>
ORC_IMU_HD void imu_phi46_lead(const double* rec, ImuFlags f, const double* grav, const ImuIntrinsicMx& mx, Sink& out) {
    if (!((f.use_larvio || f.use_closed_form) && (f.use_larvio || f.use_left))) {   // Euler forms, right closed form: today's blocks
        imu_phi(rec, f, grav, out);
        return;
    }
    out.init();
    const double dt = rec[IMU_REC_DT];
    const double *gyro = rec + IMU_REC_GYRO, *go = rec + IMU_REC_GYRO_OLD, *C = rec + IMU_REC_R_OLD;
    const double *vk = rec + IMU_REC_VK, *pk = rec + IMU_REC_PK, *vk1 = rec + IMU_REC_VK1, *pk1 = rec + IMU_REC_PK1;
    double I3[9], cr[3], aa[3], Ah[9], M[9], T[9], U[9], V[9], S[9], X[9], Y[9], w[3];
    m3_eye(I3, 1.0);
    v3_cross(go, gyro, cr);
    for (int i = 0; i < 3; ++i) aa[i] = dt * (go[i] + gyro[i]) / 2 + dt * dt * cr[i] / 12;
    m3_skew(aa, Ah);
    // B1 = -0.5 C (2 I + Ah) dt;  Phi_q_bg = B1 Tg;  Phi_q_ba = -B1 TA Ma
    for (int i = 0; i < 9; ++i) M[i] = 2 * I3[i] + Ah[i];
    m3_mul(C, M, T);
    for (int i = 0; i < 9; ++i) T[i] = -0.5 * T[i] * dt;
    m3_mul(T, mx.Tg, X);
    out.put(0, 9, X, 1.0);
    m3_mul(T, mx.TA, X);
    m3_mul(X, mx.Ma, Y);
    out.put(0, 12, Y, -1.0);
    // Phi_v_q
    for (int i = 0; i < 3; ++i) w[i] = vk1[i] - vk[i] - grav[i] * dt;
    m3_skew(w, S);
    out.put(3, 0, S, -1.0);
    // Phi_v_bg (as written: no Tg)
    for (int i = 0; i < 3; ++i) w[i] = -pk1[i] + pk[i] + vk1[i] * dt - 0.5 * grav[i] * dt * dt;
    m3_skew(w, S);
    m3_mul(S, C, U);
    for (int i = 0; i < 3; ++i) w[i] = -0.5 * pk1[i] + 0.5 * pk[i] + 0.5 * vk1[i] * dt - grav[i] * dt * dt / 6;
    m3_skew(w, S);
    m3_mul(S, C, M);
    m3_mul(M, Ah, S);
    for (int i = 0; i < 9; ++i) U[i] = U[i] + S[i];
    out.put(3, 9, U, 1.0);
    // Phi_v_ba = B1 Ma - Phi_v_bg TA Ma
    m3_mul(T, mx.Ma, X);
    m3_mul(U, mx.TA, M);
    m3_mul(M, mx.Ma, Y);
    for (int i = 0; i < 9; ++i) X[i] = X[i] - Y[i];
    out.put(3, 12, X, 1.0);
    // Phi_p_q, Phi_p_v
    for (int i = 0; i < 3; ++i) w[i] = pk1[i] - pk[i] - vk[i] * dt - 0.5 * grav[i] * dt * dt;
    m3_skew(w, S);
    out.put(6, 0, S, -1.0);
    out.put(6, 3, I3, dt);
    // Phi_p_bg
    m3_skew(grav, S);
    m3_mul(S, C, V);
    for (int i = 0; i < 3; ++i) w[i] = pk1[i] - pk[i] - grav[i] * dt * dt / 6;
    m3_skew(w, S);
    m3_mul(S, C, M);
    m3_mul(M, Ah, S);
    for (int i = 0; i < 9; ++i) V[i] = -dt * dt * dt * V[i] / 6 + dt * S[i] / 4;
    out.put(6, 9, V, 1.0);
    // Phi_p_ba = -C (3 I + Ah) dt^2 / 6 Ma - Phi_p_bg TA Ma
    for (int i = 0; i < 9; ++i) M[i] = 3 * I3[i] + Ah[i];
    m3_mul(C, M, T);
    for (int i = 0; i < 9; ++i) T[i] = -T[i] * dt * dt / 6;
    m3_mul(T, mx.Ma, X);
    m3_mul(V, mx.TA, M);
    m3_mul(M, mx.Ma, Y);
    for (int i = 0; i < 9; ++i) X[i] = X[i] - Y[i];
    out.put(6, 12, X, 1.0);
}

// whether the form writes intrinsic blocks at all: the left / LARVIO closed form only
ORC_IMU_HD bool imu_has_intrinsic_blocks(ImuFlags f) { return (f.use_larvio || f.use_closed_form) && (f.use_larvio || f.use_left); }

// WL / WD / WU of :4042-4137 (kind 0, 1, 2) from a 3-vector
ORC_IMU_HD void imu_pattern(int kind, const double* x, double* M) {
    for (int i = 0; i < 9; ++i) M[i] = 0.0;
    if (kind == 0) { M[3] = x[0]; M[7] = x[0]; M[8] = x[1]; }
    else if (kind == 1) { M[0] = x[0]; M[4] = x[1]; M[8] = x[2]; }
    else { M[0] = x[1]; M[1] = x[2]; M[5] = x[2]; }
}
// Column group j (0 .. 7: T1 T2 T3 A1 A2 A3 M1 M2) of the left / LARVIO closed form, out [9][3]: rows theta, v, p.  The three families
// differ in the vector the pattern is made from (w, acc, f: old, mid, new), the factor in front of it (I, Tg, TA), the sign, and -- the M
// family only -- a direct term in the velocity rows (:4235-4241).
ORC_IMU_HD void imu_phi46_triple(const double* rec, const ImuIntrinsicMx& mx, int j, double* out) {
    const double dt = rec[IMU_REC_DT];
    const double *gyro = rec + IMU_REC_GYRO, *go = rec + IMU_REC_GYRO_OLD, *acc = rec + IMU_REC_ACC, *acco = rec + IMU_REC_ACC_OLD;
    const double* C = rec + IMU_REC_R_OLD;
    const int grp = j < 3 ? 0 : (j < 6 ? 1 : 2), kind = j < 6 ? j % 3 : j - 6;
    double cr[3], aa[3], Ah[9], Rm[9], Rp[9], I3[9];
    m3_eye(I3, 1.0);
    v3_cross(go, gyro, cr);
    for (int i = 0; i < 3; ++i) aa[i] = dt * (go[i] + gyro[i]) / 2 + dt * dt * cr[i] / 12;
    m3_skew(aa, Ah);
    for (int i = 0; i < 9; ++i) { Rm[i] = I3[i] + 0.5 * Ah[i]; Rp[i] = I3[i] + Ah[i]; }
    const double* so = rec + (grp == 0 ? (int)IMU_REC_W_OLD : (grp == 1 ? (int)IMU_REC_ACC_OLD : (int)IMU_REC_F_OLD));
    const double* sn = rec + (grp == 0 ? (int)IMU_REC_W : (grp == 1 ? (int)IMU_REC_ACC : (int)IMU_REC_F));
    double sm[3];
    if (grp == 0) {
        v3_cross(so, sn, cr);
        for (int i = 0; i < 3; ++i) sm[i] = (so[i] + sn[i]) / 2 + dt * cr[i] / 12;
    } else {
        for (int i = 0; i < 3; ++i) sm[i] = (sn[i] + so[i]) / 2;
    }
    double X1[9], Xh[9], Xp[9], k1[9], k2[9], k4[9], T[9], Rq[9];
    imu_pattern(kind, so, X1);
    imu_pattern(kind, sm, Xh);
    imu_pattern(kind, sn, Xp);
    if (grp == 0) {
        for (int i = 0; i < 9; ++i) k1[i] = X1[i];
        m3_mul(Rm, Xh, k2);
        m3_mul(Rp, Xp, k4);
    } else {
        const double* L = grp == 1 ? mx.Tg : mx.TA;
        m3_mul(L, X1, k1);
        m3_mul(Rm, L, T);
        m3_mul(T, Xh, k2);
        m3_mul(Rp, L, T);
        m3_mul(T, Xp, k4);
    }
    for (int i = 0; i < 9; ++i) Rq[i] = dt * (k1[i] + 4 * k2[i] + k4[i]) / 6;
    const double sq = grp == 0 ? 1.0 : -1.0, sv = grp == 0 ? -1.0 : 1.0;
    m3_mul(C, Rq, T);
    for (int i = 0; i < 9; ++i) out[i] = sq * T[i];
    // velocity rows
    double am[3], y[3], Sm[9], Sp[9], kv1[9], kv2[9], kv3[9], kv4[9], E[9], fR[9];
    for (int i = 0; i < 3; ++i) am[i] = (acc[i] + acco[i]) / 2;
    m3_mulv(Rm, am, y);
    m3_skew(y, Sm);
    m3_mulv(Rp, acc, y);
    m3_skew(y, Sp);
    for (int i = 0; i < 9; ++i) Sm[i] = Sm[i] * dt;
    m3_mul(Sm, k1, kv2);
    m3_mul(Sm, k2, kv3);
    m3_mul(Sp, Rq, kv4);
    for (int i = 0; i < 9; ++i) { kv1[i] = 0.0; kv2[i] = kv2[i] / 2; kv3[i] = kv3[i] / 2; }
    if (grp == 2) {
        for (int i = 0; i < 9; ++i) kv1[i] = X1[i];
        m3_mul(Rm, Xh, E);
        for (int i = 0; i < 9; ++i) { kv2[i] = E[i] + kv2[i]; kv3[i] = E[i] + kv3[i]; }
        m3_mul(Rp, Xp, E);
        for (int i = 0; i < 9; ++i) kv4[i] = E[i] + kv4[i];
    }
    for (int i = 0; i < 9; ++i) fR[i] = dt * (kv1[i] + 2 * kv2[i] + 2 * kv3[i] + kv4[i]) / 6;
    m3_mul(C, fR, T);
    for (int i = 0; i < 9; ++i) out[9 + i] = sv * T[i];
    // position rows: kp1 = 0, kp2 = dt kv1 / 2, kp3 = dt kv2 / 2, kp4 = fR
    for (int i = 0; i < 9; ++i) E[i] = 2 * (dt * kv1[i] / 2) + 2 * (dt * kv2[i] / 2) + fR[i];
    m3_mul(C, E, T);
    for (int i = 0; i < 9; ++i) out[18 + i] = sv * (T[i] * dt) / 6;
}

// imu_propagate_mean at 46: the same selection and predictors, on the measurement of :733-746.  recs [<= cap][IMU_REC46].
inline bool imu_propagate_mean46(const ImuModelConfig& c, const ImuIntrinsicMx& mx, ImuMeanState* st, double* prev_meas, const double* samples,
                                 int n, double time_bound, double* recs, int cap, ImuBatchInfo* info) {
    int used = 0, count = 0;
    double dt_img = 0.0, cur = st->time;
    for (int k = 0; k < n; ++k) {
        const double t = samples[k * 7];
        if (t <= cur) { ++used; continue; }
        if (t - time_bound > c.imu_img_time_th) break;
        ++count; ++used;
        dt_img = t - time_bound;
        cur = t;
    }
    info->n_used = used; info->n_propagated = count; info->dt = dt_img;
    info->mean_sforce[0] = info->mean_sforce[1] = info->mean_sforce[2] = 0.0;
    if (count > cap) return false;
    double sum[3] = {0, 0, 0};
    int s = 0;
    for (int k = 0; k < n && s < count; ++k) {
        const double* row = samples + k * 7;
        const double t = row[0];
        if (t <= st->time) continue;
        double* rec = recs + (size_t)s * IMU_REC46;
        const double dt = t - st->time;
        rec[IMU_REC_DT] = dt;
        imu_measurement46(row + 1, row + 4, st->bg, st->ba, mx, rec + IMU_REC_F, rec + IMU_REC_W, rec + IMU_REC_ACC, rec + IMU_REC_GYRO);
        imu_measurement46(prev_meas, prev_meas + 3, st->bg, st->ba, mx, rec + IMU_REC_F_OLD, rec + IMU_REC_W_OLD, rec + IMU_REC_ACC_OLD, rec + IMU_REC_GYRO_OLD);
        for (int i = 0; i < 3; ++i) {
            rec[IMU_REC_VK + i] = c.flags.if_fej ? st->v_fej[i] : st->v[i];
            rec[IMU_REC_PK + i] = c.flags.if_fej ? st->p_fej[i] : st->p[i];
        }
        for (int i = 0; i < 9; ++i) rec[IMU_REC_R_OLD + i] = st->R[i];
        if (!c.flags.use_larvio) imu_predict_orcvio(dt, rec + IMU_REC_GYRO, rec + IMU_REC_ACC, c.gravity, st->R, st->v, st->p);
        else imu_predict_larvio(dt, rec + IMU_REC_GYRO, rec + IMU_REC_ACC, c.gravity, st->R, st->v, st->p);
        for (int i = 0; i < 3; ++i) { st->v_fej[i] = st->v[i]; st->p_fej[i] = st->p[i]; }
        for (int i = 0; i < 9; ++i) rec[IMU_REC_R_NEW + i] = st->R[i];
        for (int i = 0; i < 3; ++i) { rec[IMU_REC_VK1 + i] = st->v[i]; rec[IMU_REC_PK1 + i] = st->p[i]; }
        st->time = t;
        for (int i = 0; i < 6; ++i) prev_meas[i] = row[1 + i];
        for (int i = 0; i < 3; ++i) sum[i] += row[4 + i];
        ++s;
    }
    if (count > 0)
        for (int i = 0; i < 3; ++i) info->mean_sforce[i] = sum[i] / count;
    return true;
}

// The ordered product on the host at 46.  Phi, Q [46][46] out.
inline void imu_accumulate_host46(const double* recs, int S, ImuFlags f, const double* grav, const double* qc, const ImuIntrinsicMx& mx,
                                  double* Phi, double* Q) {
    double A[IMU_DIM * IMU_DIM], B[IMU_DIM * IMU_DIM], P[IMU_DIM * IMU_DIM], T[IMU_DIM * IMU_DIM], U[IMU_DIM * IMU_DIM];
    double Bi[IMU_DIM * IMU_NI], Bt[IMU_DIM * IMU_NI], Bk[9 * IMU_NI];
    for (int i = 0; i < IMU_DIM * IMU_DIM; ++i) { A[i] = (i / IMU_DIM == i % IMU_DIM) ? 1.0 : 0.0; B[i] = 0.0; }
    for (int i = 0; i < IMU_DIM * IMU_NI; ++i) Bi[i] = 0.0;
    const bool intr = imu_has_intrinsic_blocks(f);
    for (int k = 0; k < S; ++k) {
        const double* rec = recs + (size_t)k * IMU_REC46;
        ImuDenseSink sink{P, IMU_DIM};
        imu_phi46_lead(rec, f, grav, mx, sink);
        double nc[24];
        imu_noise(rec, f, qc, nc);
        for (int i = 0; i < 9 * IMU_NI; ++i) Bk[i] = 0.0;
        if (intr)
            for (int j = 0; j < IMU_TRIPLES; ++j) {
                double g[27];
                imu_phi46_triple(rec, mx, j, g);
                for (int r = 0; r < 9; ++r)
                    for (int c = 0; c < 3; ++c) Bk[r * IMU_NI + 3 * j + c] = g[r * 3 + c];
            }
        for (int i = 0; i < IMU_DIM; ++i)
            for (int j = 0; j < IMU_DIM; ++j) U[i * IMU_DIM + j] = B[i * IMU_DIM + j] + imu_noise_at(nc, i, j);
        imu_mul15(P, U, T);                                 // T = Phi_k (Q + N_k)
        for (int i = 0; i < IMU_DIM; ++i)
            for (int j = 0; j < IMU_DIM; ++j) {
                double s = 0.0;
                for (int l = 0; l < IMU_DIM; ++l) s += T[i * IMU_DIM + l] * P[j * IMU_DIM + l];
                B[i * IMU_DIM + j] = s;
            }
        for (int i = 0; i < IMU_DIM; ++i)                   // B <- A_k B + B_k
            for (int j = 0; j < IMU_NI; ++j) {
                double s = 0.0;
                for (int l = 0; l < IMU_DIM; ++l) s += P[i * IMU_DIM + l] * Bi[l * IMU_NI + j];
                Bt[i * IMU_NI + j] = i < 9 ? s + Bk[i * IMU_NI + j] : s;
            }
        for (int i = 0; i < IMU_DIM * IMU_NI; ++i) Bi[i] = Bt[i];
        imu_mul15(P, A, T);
        for (int i = 0; i < IMU_DIM * IMU_DIM; ++i) A[i] = T[i];
    }
    for (int i = 0; i < IMU_LEG46; ++i)
        for (int j = 0; j < IMU_LEG46; ++j) {
            const bool in = i < IMU_DIM && j < IMU_DIM;
            double p = i == j ? 1.0 : 0.0;
            if (in) p = A[i * IMU_DIM + j];
            else if (i < IMU_DIM && j >= IMU_LEG) p = Bi[i * IMU_NI + j - IMU_LEG];
            Phi[i * IMU_LEG46 + j] = p;
            Q[i * IMU_LEG46 + j] = in ? 0.5 * (B[i * IMU_DIM + j] + B[j * IMU_DIM + i]) : 0.0;
        }
}

}  // namespace orcvio_amd
