// MsckfBackend::odometryCovariance and the pair odometryCovarianceSubmit / odometryCovarianceCollect
// (orcvio_amd/csrc/host/orcvio_msckf_host.hpp) as a filter calls them, for tests/test_gpu_cov_marginal_host.py: a backend of its own,
// the covariance made resident, then
//   "blocking"  odometryCovariance on the covariance as it stands
//   "behind"    one frame call that propagates, augments and marginalises the oldest clone (orcvio_msckf_io_step_frame on an empty
//               window: its last launches are enqueued and not waited for), odometryCovarianceSubmit directly behind it, the caller's
//               state increment, odometryCovarianceCollect
//   "again"     odometryCovariance once more on what the frame left
// One line per route: the name, P_body_pose 36, P_body_vel 9 (%.17g).  The case file: R 9 | leg | N | n | P n^2 | Phi leg^2 | Q leg^2.
#include <cstdio>
#include <vector>

#include "../../orcvio_amd/csrc/host/orcvio_msckf_host.hpp"

using namespace orcvio_amd;

static void print(const char* route, const double* pose, const double* vel) {
    std::printf("%s", route);
    for (int i = 0; i < 36; ++i) std::printf(" %.17g", pose[i]);
    for (int i = 0; i < 9; ++i) std::printf(" %.17g", vel[i]);
    std::printf("\n");
}
#define CHK(expr)                                                                                      \
    do {                                                                                               \
        const int rc_ = (expr);                                                                        \
        if (rc_ != ORCVIO_OK) { std::printf("FAILED: %s -> %d: %s\n", #expr, rc_, orcvio_msckf_last_error()); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<double> v;
    double x;
    while (std::fscanf(f, "%lf", &x) == 1) v.push_back(x);
    std::fclose(f);
    try {
        size_t o = 0;
        double R[9];
        for (int k = 0; k < 9; ++k) R[k] = v.at(o++);
        const int leg = (int)v.at(o++), N = (int)v.at(o++), n = (int)v.at(o++);
        if (n != leg + 6 * N || v.size() != o + (size_t)n * n + 2 * (size_t)leg * leg) return 3;
        StateServer ss;
        ss.state_cov.assign(v.begin() + (long)o, v.begin() + (long)(o + (size_t)n * n));
        o += (size_t)n * n;
        const std::vector<double> Phi(v.begin() + (long)o, v.begin() + (long)(o + (size_t)leg * leg));
        o += (size_t)leg * leg;
        const std::vector<double> Q(v.begin() + (long)o, v.begin() + (long)(o + (size_t)leg * leg));

        MsckfBackend be(0, 24, 16, 256);
        be.flags.leg_dim = leg;
        double pose[36], vel[9];
        if (be.odometryCovariance(R, pose, vel) != ORCVIO_ERR_INVALID) { std::printf("FAILED: no resident covariance was not refused\n"); return 1; }
        if (be.odometryCovarianceCollect(pose, vel) != ORCVIO_ERR_INVALID) { std::printf("FAILED: a collect without a submit was not refused\n"); return 1; }
        // (dim() counts the containers: the covariance goes in through the C-ABI the backend wraps)
        CHK(orcvio_msckf_cov_set(be.handle(), n, ss.state_cov.data()));
        CHK(be.odometryCovariance(R, pose, vel));
        print("blocking", pose, vel);

        // the frame: N + 1 clones behind its augmentation, no tracks, the oldest clone marginalised
        orcvio_msckf_io io{};
        CHK(orcvio_msckf_io_begin(be.handle(), &be.flags, N + 1, 0, 0, 2, &io));
        for (int i = 0; i <= N; ++i) {
            double* p = io.poses + (size_t)ORCVIO_POSE_STRIDE * i;
            for (int k = 0; k < ORCVIO_POSE_STRIDE; ++k) p[k] = 0.0;
            p[0] = p[4] = p[8] = 1.0;
            p[15] = p[19] = p[23] = 1.0;
            p[9] = 0.1 * i;
        }
        io.obs_ptr[0] = 0;
        const int32_t rm[1] = {0};
        orcvio_msckf_frame_step st{};
        st.leg_dim = leg; st.Phi = Phi.data(); st.Q = Q.data(); st.augment = 1; st.remove_clones = rm; st.n_remove = 1;
        orcvio_msckf_frame_result res{};
        CHK(orcvio_msckf_io_step_frame(be.handle(), &st, &res));
        if (res.n_after != n) { std::printf("FAILED: n_after %d\n", res.n_after); return 1; }
        CHK(be.odometryCovarianceSubmit(R));
        if (be.odometryCovarianceSubmit(R) != ORCVIO_ERR_INVALID) { std::printf("FAILED: a second submit was not refused\n"); return 1; }
        // the caller's state increment (incrementState_IMUCam on the frame's dx), while the launch runs
        orcvio_msckf_state state{};
        state.R_b2w_imu[0] = state.R_b2w_imu[4] = state.R_b2w_imu[8] = 1.0;
        state.R_b2c[0] = state.R_b2c[4] = state.R_b2c[8] = 1.0;
        std::vector<double> dx(res.dx, res.dx + n + 6);
        (void)orcvio_msckf_increment_state(&be.flags, dx.data(), &state);
        CHK(be.odometryCovarianceCollect(pose, vel));
        print("behind", pose, vel);
        CHK(be.odometryCovariance(R, pose, vel));
        print("again", pose, vel);
    } catch (const std::exception& e) {
        std::printf("exception %s\n", e.what());
        return 5;
    }
    std::printf("host cov marginal ok\n");
    return 0;
}
