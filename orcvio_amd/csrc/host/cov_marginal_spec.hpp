// cov_marginal_spec.hpp -- what orcvio_msckf_cov_get_marginal / _marginal_submit accept, and the one spec the odometry getters use;
// free of HIP.  The library validates a request with marginal_refusal before anything is enqueued; the host layer
// (orcvio_msckf_host.hpp, MsckfBackend::odometryCovariance) builds its request with odometry_marginal_spec.
// tests/cpp/cov_marginal_spec_main.cpp runs both under the address and undefined-behaviour sanitizers.
#pragma once
#include <cmath>
#include <cstdint>

namespace orcvio_amd {

enum { MARGINAL_MAX = 64 };   // (= ORCVIO_MARGINAL_MAX)

// nullptr: the request is acceptable for a resident covariance of dimension res_n; otherwise the reason it is refused.  Entries of P
// are not looked at; idx may be in any order and repeat.
inline const char* marginal_refusal(int32_t n_idx, const int32_t* idx, int32_t m, const double* T, int32_t res_n) {
    if (res_n <= 0) return "no resident covariance";
    if (n_idx < 1 || n_idx > MARGINAL_MAX) return "n_idx outside 1..64";
    if (!idx) return "idx is NULL";
    for (int32_t i = 0; i < n_idx; ++i)
        if (idx[i] < 0 || idx[i] >= res_n) return "a state index outside the resident covariance";
    if (m < 0 || m > MARGINAL_MAX) return "m outside 0..64";
    if (m == 0) return T ? "T given with m == 0" : nullptr;
    if (!T) return "T is NULL with m > 0";
    for (int32_t i = 0; i < m * n_idx; ++i)
        if (!std::isfinite(T[i])) return "a non-finite entry of T";
    return nullptr;
}

// The odometry message's two covariances as ONE congruence (src/orcvio.cpp:2999-3026): idx = {6,7,8, 0,1,2, 3,4,5} (position,
// orientation, velocity) and T = blkdiag(R, R, R) with R = T_imu_body's rotation, row-major [9][9].  The leading 6 x 6 of
// T P[idx, idx] T^T is getPpose()'s matrix in its own order (position first), the trailing 3 x 3 getPvel()'s.
enum { ODOMETRY_MARGINAL_DIM = 9 };
inline void odometry_marginal_spec(const double R_imu_body[9], int32_t idx[9], double T[81]) {
    static const int32_t order[9] = {6, 7, 8, 0, 1, 2, 3, 4, 5};
    for (int i = 0; i < 9; ++i) idx[i] = order[i];
    for (int i = 0; i < 81; ++i) T[i] = 0.0;
    for (int b = 0; b < 3; ++b)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) T[(3 * b + r) * 9 + 3 * b + c] = R_imu_body[3 * r + c];
}
// the 9 x 9 result taken apart: P_body_pose [6][6], P_body_vel [3][3]
inline void odometry_marginal_split(const double out[81], double P_body_pose[36], double P_body_vel[9]) {
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) P_body_pose[6 * i + j] = out[9 * i + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) P_body_vel[3 * i + j] = out[9 * (6 + i) + 6 + j];
}

}  // namespace orcvio_amd
