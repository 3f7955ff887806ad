// imu_calib_shim.cpp -- MsckfBackend::processImu (orcvio_amd/csrc/host/orcvio_msckf_host.hpp) at leg_dim 46 as a filter calls it, for
// tests/test_gpu_imu_calib_host.py: a backend of its own, the covariance made resident, the buffered IMU messages processed with the
// state's IMU intrinsics, the covariance fetched back.
#include <cstring>
#include <vector>

#include "../../orcvio_amd/csrc/host/orcvio_msckf_host.hpp"

using namespace orcvio_amd;

// cfg [20]: use_larvio use_left use_closed_form if_fej | gravity 3 | imu_img_timeTh | Q_c diagonal 12;  intr [24]: T1 T2 T3 A1 A2 A3 M1 M2
// imu [28] in / out: time | R 9 | v 3 | p 3 | b_g 3 | b_a 3 | v_fej 3 | p_fej 3;  prev [6] in / out: m_gyro_old | m_acc_old
// msgs [n_msgs][7]: t | gyro | acc.  Out: P (resident covariance behind the call), outcome [4] = status | n_used | n_propagated |
// messages left in the buffer, info [4] = dt | meanSForce.
extern "C" int orc_test_process_imu_calib(const double* cfg, const double* intr, double* imu, double* prev, const double* msgs, int n_msgs,
                                          double time_bound, int wait, double* P, int n, int* outcome, double* info) {
    try {
        MsckfBackend be(0, 24, 16, 256);
        orcvio_msckf_imu_config c{};
        c.leg_dim = 46; c.use_larvio = (int)cfg[0]; c.use_left_perturbation = (int)cfg[1]; c.use_closed_form = (int)cfg[2]; c.if_fej = (int)cfg[3];
        for (int k = 0; k < 3; ++k) c.gravity[k] = cfg[4 + k];
        c.imu_img_time_th = cfg[7];
        for (int k = 0; k < 12; ++k) c.Q_c_diag[k] = cfg[8 + k];
        StateServer ss;
        std::memcpy(ss.imu_intrinsics, intr, sizeof(ss.imu_intrinsics));
        IMUState& s = ss.imu_state;
        s.time = imu[0];
        std::memcpy(s.orientation, imu + 1, sizeof(double) * 9);
        for (int k = 0; k < 3; ++k) { s.velocity[k] = imu[10 + k]; s.position[k] = imu[13 + k]; s.gyro_bias[k] = imu[16 + k]; s.acc_bias[k] = imu[19 + k]; }
        ss.imu_state_FEJ_now = s;
        for (int k = 0; k < 3; ++k) { ss.imu_state_FEJ_now.velocity[k] = imu[22 + k]; ss.imu_state_FEJ_now.position[k] = imu[25 + k]; }
        for (int k = 0; k < 3; ++k) { ss.m_gyro_old[k] = prev[k]; ss.m_acc_old[k] = prev[3 + k]; }
        std::vector<ImuData> buf((size_t)n_msgs);
        for (int i = 0; i < n_msgs; ++i) {
            buf[i].timeStampToSec = msgs[7 * i];
            for (int k = 0; k < 3; ++k) { buf[i].angular_velocity[k] = msgs[7 * i + 1 + k]; buf[i].linear_acceleration[k] = msgs[7 * i + 4 + k]; }
        }
        ss.state_cov.assign(P, P + (size_t)n * n);
        int rc = be.covarianceToDevice(ss);
        if (rc != ORCVIO_OK) return rc;
        const ImuOutcome out = be.processImu(ss, c, time_bound, buf, wait != 0);
        outcome[0] = out.status; outcome[1] = out.n_used; outcome[2] = out.n_propagated; outcome[3] = (int)buf.size();
        info[0] = out.dt;
        for (int k = 0; k < 3; ++k) info[1 + k] = out.meanSForce[k];
        rc = be.covarianceToHost(ss);
        if (rc != ORCVIO_OK || ss.dim() != n) return rc != ORCVIO_OK ? rc : ORCVIO_ERR_INVALID;
        std::memcpy(P, ss.state_cov.data(), sizeof(double) * (size_t)n * n);
        imu[0] = s.time;
        std::memcpy(imu + 1, s.orientation, sizeof(double) * 9);
        for (int k = 0; k < 3; ++k) {
            imu[10 + k] = s.velocity[k]; imu[13 + k] = s.position[k];
            imu[22 + k] = ss.imu_state_FEJ_now.velocity[k]; imu[25 + k] = ss.imu_state_FEJ_now.position[k];
            prev[k] = ss.m_gyro_old[k]; prev[3 + k] = ss.m_acc_old[k];
        }
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}
