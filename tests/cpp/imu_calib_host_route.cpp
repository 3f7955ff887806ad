// imu_calib_host_route.cpp -- what a caller has to run on the host at leg_dim 46 WITHOUT orcvio_msckf_cov_propagate_imu_calib: the mean
// propagation and the accumulation of Phi, Q [46][46] (imu_propagate_mean46 + imu_accumulate_host46 of host/imu_model.hpp), in front of
// orcvio_msckf_cov_propagate.  scripts/gpu_imu_calib_timing.py builds it with -O3 as a shared library: the parent leg of its timing.
#include <vector>

#include "../../orcvio_amd/csrc/host/imu_model.hpp"

using namespace orcvio_amd;

// flags [4]: use_larvio use_left use_closed_form if_fej;  st [28]: time | R 9 | v 3 | p 3 | b_g 3 | b_a 3 | v_fej 3 | p_fej 3 (in / out)
// Returns the number of propagated samples, or -1 beyond 128.
extern "C" int orc_imu_calib_host_route(const double* flags, const double* gravity, double time_th, const double* Qc, const double* intr,
                                        double* st, double* prev, const double* samples, int n, double time_bound, double* Phi, double* Q) {
    static std::vector<double> recs((size_t)IMU_MAX_SAMPLES * IMU_REC46);
    ImuModelConfig c{};
    c.flags = ImuFlags{(int)flags[0], (int)flags[1], (int)flags[2], (int)flags[3]};
    for (int i = 0; i < 3; ++i) c.gravity[i] = gravity[i];
    c.imu_img_time_th = time_th;
    ImuIntrinsicMx mx;
    imu_intrinsic_mx(intr, &mx);
    ImuMeanState s;
    const double* p = st;
    s.time = *p++;
    for (int i = 0; i < 9; ++i) s.R[i] = *p++;
    for (int i = 0; i < 3; ++i) s.v[i] = *p++;
    for (int i = 0; i < 3; ++i) s.p[i] = *p++;
    for (int i = 0; i < 3; ++i) s.bg[i] = *p++;
    for (int i = 0; i < 3; ++i) s.ba[i] = *p++;
    for (int i = 0; i < 3; ++i) s.v_fej[i] = *p++;
    for (int i = 0; i < 3; ++i) s.p_fej[i] = *p++;
    ImuBatchInfo info{};
    if (!imu_propagate_mean46(c, mx, &s, prev, samples, n, time_bound, recs.data(), IMU_MAX_SAMPLES, &info)) return -1;
    imu_accumulate_host46(recs.data(), info.n_propagated, c.flags, c.gravity, Qc, mx, Phi, Q);
    st[0] = s.time;
    for (int i = 0; i < 9; ++i) st[1 + i] = s.R[i];
    for (int i = 0; i < 3; ++i) { st[10 + i] = s.v[i]; st[13 + i] = s.p[i]; st[22 + i] = s.v_fej[i]; st[25 + i] = s.p_fej[i]; }
    return info.n_propagated;
}
