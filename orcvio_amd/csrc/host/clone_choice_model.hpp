// clone_choice_model.hpp -- the reference's choice of the two clones that leave the window (findRedundantImuStates,
// src/orcvio.cpp:2582-2626, called by pruneImuStateBuffer :2629-2645 AFTER removeLostFeatures has applied its update), in plain C++ that
// compiles for the host and for the device (the guard pattern of zupt_check_model.hpp, no Eigen).  k_clone_choice (clone_choice_ops.hpp),
// the C++ host layer (MsckfBackend::findRedundantImuStates) and tests/cpp/test_clone_choice_model.cpp compile this one source.
//
// Window of N clones, index 0 the oldest; key = N - 4.  Two iterations:
//   iteration 1 compares clone N - 3 with the key.  Taken (angle < rotation_threshold && distance < translation_threshold &&
//   tracking_ok): N - 3 leaves, the next compared clone is N - 2.  Not taken: the OLDEST clone leaves, the oldest pointer advances and
//   the compared clone moves back by TWO (:2615-2618, kept as written): N - 5, a clone OLDER than the key.
//   iteration 2 does the same with the clone it has arrived at.
// The four possible results, ascending: {N-3, N-2}, {0, N-3}, {0, N-5}, {0, 1}.  At N = 5 the clone N - 5 IS the oldest one and the
// reference's loop can name clone 0 twice: N >= 6 is required here (a documented divergence, include/orcvio_msckf.h).
//
//   distance = |position_cam(c) - position_cam(key)|
//   angle    = the rotation angle in [0, pi] of orientation_cam(c)^T orientation_cam(key), evaluated as Eigen 3.3's
//              AngleAxisd(Matrix3d) does: the quaternion of the matrix (Shoemake's branches, Eigen/src/Geometry/Quaternion.h), then
//              2 atan2(|vec|, |w|).  The choice of THIS form is deliberate: the reference pins no Eigen version, and the older
//              acos((trace - 1) / 2) form loses half the digits at the small angles the threshold sits at (d acos / dx is unbounded at 1).
//
// Camera poses ("cam": orientation_cam 9 row-major | position_cam 3):
//   clone_choice_cam_pose   incrementState_IMUCam's rewrite (:4555-4564) from the body pose as the first update's dx has left it and the
//                           IMU state's CURRENT extrinsic, itself incremented by dx[15:21] (not the clone's frozen one):
//                           orientation_cam = R_b2w R_imu_cam0^T,  position_cam = t_b_w + R_b2w t_cam0_imu
//   when dx is not applied (no first update, a refused one, a dx that discard_large_update discards, prune_apply_dx = 0) the
//   reference's containers are untouched: the caller's cam records are read as they are.
#pragma once

#if defined(__HIPCC__)
#define ORC_CCH_HD __host__ __device__ inline
#else
#define ORC_CCH_HD inline
#endif

#include <math.h>

namespace orcvio_amd {

enum { CLONE_CHOICE_MIN_N = 6, CLONE_CHOICE_CAM = 12 };

// the layout of orcvio_msckf_clone_choice (include/orcvio_msckf.h)
struct CloneChoice {
    int evaluated, agree, chosen[2], compared[2], taken[2];
    double angle[2], distance[2];
};

ORC_CCH_HD void clone_choice_cam_pose(const double* R_b2w, const double* t_b_w, const double* R_imu_cam0, const double* t_cam0_imu, double* cam) {
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b)
            cam[a * 3 + b] = R_b2w[a * 3 + 0] * R_imu_cam0[b * 3 + 0] + R_b2w[a * 3 + 1] * R_imu_cam0[b * 3 + 1] + R_b2w[a * 3 + 2] * R_imu_cam0[b * 3 + 2];
        cam[9 + a] = t_b_w[a] + (R_b2w[a * 3 + 0] * t_cam0_imu[0] + R_b2w[a * 3 + 1] * t_cam0_imu[1] + R_b2w[a * 3 + 2] * t_cam0_imu[2]);
    }
}

// rotation angle of M = Rc^T Rk (both row-major) the way Eigen 3.3 evaluates AngleAxisd(M).angle()
ORC_CCH_HD double clone_choice_angle(const double* Rc, const double* Rk) {
    double m[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) m[a * 3 + b] = Rc[0 * 3 + a] * Rk[0 * 3 + b] + Rc[1 * 3 + a] * Rk[1 * 3 + b] + Rc[2 * 3 + a] * Rk[2 * 3 + b];
    double w, v[3];
    double t = m[0] + m[4] + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        w = 0.5 * t;
        t = 0.5 / t;
        v[0] = (m[7] - m[5]) * t; v[1] = (m[2] - m[6]) * t; v[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
        v[i] = 0.5 * t;
        t = 0.5 / t;
        w = (m[k * 3 + j] - m[j * 3 + k]) * t;
        v[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        v[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    return 2.0 * atan2(n, fabs(w));
}

ORC_CCH_HD double clone_choice_distance(const double* pc, const double* pk) {
    const double d0 = pc[0] - pk[0], d1 = pc[1] - pk[1], d2 = pc[2] - pk[2];
    return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}

// is {a, b} (ascending) one of the four sets the loop can give at N clones
ORC_CCH_HD bool clone_choice_possible(int N, int a, int b) {
    return N >= CLONE_CHOICE_MIN_N && ((a == N - 3 && b == N - 2) || (a == 0 && (b == N - 3 || b == N - 5 || b == 1)));
}

// The loop.  cam(c, out): the camera record of clone c (called for the key and for the two compared clones only).  predicted: the
// caller's two clones (ascending) or nullptr (agree = 1).
template <class CamFn>
ORC_CCH_HD void clone_choice_run(int N, double rotation_threshold, double translation_threshold, int tracking_ok, CamFn cam, const int* predicted, CloneChoice* o) {
    double key[CLONE_CHOICE_CAM], cur[CLONE_CHOICE_CAM];
    cam(N - 4, key);
    int c = N - 3, first = 0;
    for (int i = 0; i < 2; ++i) {
        cam(c, cur);
        const double distance = clone_choice_distance(cur + 9, key + 9);
        const double angle = clone_choice_angle(cur, key);
        const bool take = angle < rotation_threshold && distance < translation_threshold && tracking_ok != 0;
        o->compared[i] = c; o->taken[i] = take ? 1 : 0; o->angle[i] = angle; o->distance[i] = distance;
        if (take) { o->chosen[i] = c; ++c; }
        else { o->chosen[i] = first; ++first; c -= 2; }
    }
    if (o->chosen[1] < o->chosen[0]) { const int s = o->chosen[0]; o->chosen[0] = o->chosen[1]; o->chosen[1] = s; }   // (sort, :2623)
    o->agree = (!predicted || (predicted[0] == o->chosen[0] && predicted[1] == o->chosen[1])) ? 1 : 0;
    o->evaluated = 1;
}

// on cam records as they stand, [N][12]
ORC_CCH_HD void clone_choice_on_records(int N, const double* cam_poses, double rotation_threshold, double translation_threshold, int tracking_ok,
                                        const int* predicted, CloneChoice* o) {
    clone_choice_run(N, rotation_threshold, translation_threshold, tracking_ok,
                     [cam_poses](int c, double* out) { for (int i = 0; i < CLONE_CHOICE_CAM; ++i) out[i] = cam_poses[c * CLONE_CHOICE_CAM + i]; }, predicted, o);
}

}  // namespace orcvio_amd
