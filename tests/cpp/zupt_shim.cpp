// Host-compiled view of the zero-velocity frame's host half (orcvio_amd/csrc/host/orcvio_msckf_host.hpp: zuptResidual and the
// increments behind orcvio_msckf_cov_zupt's dx, MsckfBackend::applyZuptIncrement), tests only: lets the CPU test-suite check both
// against tests/mirror_zupt.py without a GPU.  Linked against the product library for orcvio_msckf_increment_state (host arithmetic).
#include "../../orcvio_amd/csrc/host/orcvio_msckf_host.hpp"

using namespace orcvio_amd;

// the two newest clones (ids 6 and 7, imu_state.id = 7) with the given orientations (row-major R_b2w) and positions
extern "C" void orc_test_zupt_residual(const double* v, const double* R_prev, const double* p_prev, const double* R_cur, const double* p_cur,
                                       double* r) {
    StateServer ss;
    ss.imu_state.id = 7;
    std::memcpy(ss.imu_state.velocity, v, 24);
    IMUState_Aug a, b;
    a.id = 6; std::memcpy(a.orientation, R_prev, 72); std::memcpy(a.position, p_prev, 24);
    b.id = 7; std::memcpy(b.orientation, R_cur, 72); std::memcpy(b.position, p_cur, 24);
    ss.imu_states_augment[3] = IMUState_Aug{};   // (an older clone the residual must not read)
    ss.imu_states_augment[6] = a;
    ss.imu_states_augment[7] = b;
    const std::vector<double> out = zuptResidual(ss);
    std::memcpy(r, out.data(), 72);
}

namespace {

// A window of N clones (ids 10 .. 10 + N - 1) and nf in-state features anchored at window ranks anchor[] (rank >= N: nuisance state
// rank - N, its camera pose in nui_cam [.][12] = R_c2w 9 | t_c_w 3).  clone_R [N][9], clone_t [N][3],
// imu [33] = R_b2w 9 | v 3 | p 3 | bg 3 | ba 3 | R_b2c 9 | t_c_b 3, param [nf][3] (3-d: invParam; 1-d: obs_anchor), rho [nf].
void fillState(StateServer& ss, MapServer& ms, int N, const double* clone_R, const double* clone_t, const double* imu, int idp_dim, int nf,
               const int* anchor, const double* nui_cam, int n_nui, const double* param, const double* rho) {
    for (int i = 0; i < N; ++i) {
        IMUState_Aug a;
        a.id = 10 + i;
        std::memcpy(a.orientation, clone_R + 9 * i, 72);
        std::memcpy(a.position, clone_t + 3 * i, 24);
        std::memcpy(a.R_imu_cam0, imu + 21, 72);
        std::memcpy(a.t_cam0_imu, imu + 30, 24);
        ss.imu_states_augment[a.id] = a;
    }
    for (int j = 0; j < n_nui; ++j) {
        IMUState_Aug a;
        a.id = 1 + j;
        std::memcpy(a.orientation_cam, nui_cam + 12 * j, 72);
        std::memcpy(a.position_cam, nui_cam + 12 * j + 9, 24);
        ss.nui_ids.push_back(a.id);
        ss.nui_imu_states[a.id] = a;
    }
    ss.imu_state.id = 10 + N - 1;
    std::memcpy(ss.imu_state.orientation, imu, 72);
    std::memcpy(ss.imu_state.velocity, imu + 9, 24); std::memcpy(ss.imu_state.position, imu + 12, 24);
    std::memcpy(ss.imu_state.gyro_bias, imu + 15, 24); std::memcpy(ss.imu_state.acc_bias, imu + 18, 24);
    std::memcpy(ss.imu_state.R_imu_cam0, imu + 21, 72); std::memcpy(ss.imu_state.t_cam0_imu, imu + 30, 24);
    for (int i = 0; i < nf; ++i) {
        Feature f;
        f.id = 100 + i; f.in_state = true;
        f.id_anchor = anchor[i] < N ? 10 + anchor[i] : 1 + (anchor[i] - N);
        if (idp_dim == 3) std::memcpy(f.invParam, param + 3 * i, 24);
        else { std::memcpy(f.obs_anchor, param + 3 * i, 24); f.invDepth = rho[i]; }
        ms[f.id] = f;
        ss.feature_states.push_back(f.id);
    }
}

// the same arrays back, and cam [N][12] = R_c2w | t_c_w of the clones, position [nf][3]
void readState(const StateServer& ss, const MapServer& ms, double* clone_R, double* clone_t, double* imu, int idp_dim, int nf, double* param,
               double* rho, double* cam, double* position) {
    int i = 0;
    for (const auto& kv : ss.imu_states_augment) {
        std::memcpy(clone_R + 9 * i, kv.second.orientation, 72);
        std::memcpy(clone_t + 3 * i, kv.second.position, 24);
        std::memcpy(cam + 12 * i, kv.second.orientation_cam, 72);
        std::memcpy(cam + 12 * i + 9, kv.second.position_cam, 24);
        ++i;
    }
    std::memcpy(imu, ss.imu_state.orientation, 72);
    std::memcpy(imu + 9, ss.imu_state.velocity, 24); std::memcpy(imu + 12, ss.imu_state.position, 24);
    std::memcpy(imu + 15, ss.imu_state.gyro_bias, 24); std::memcpy(imu + 18, ss.imu_state.acc_bias, 24);
    std::memcpy(imu + 21, ss.imu_state.R_imu_cam0, 72); std::memcpy(imu + 30, ss.imu_state.t_cam0_imu, 24);
    for (int q = 0; q < nf; ++q) {
        const Feature& f = ms.at(100 + q);
        if (idp_dim == 3) std::memcpy(param + 3 * q, f.invParam, 24);
        else { std::memcpy(param + 3 * q, f.obs_anchor, 24); rho[q] = f.invDepth; }
        std::memcpy(position + 3 * q, f.position, 24);
    }
}

orcvio_msckf_flags makeFlags(int leg_dim, int use_larvio, int use_left, int discard_large) {
    orcvio_msckf_flags fl{};
    fl.leg_dim = leg_dim; fl.use_larvio = use_larvio; fl.use_left_perturbation = use_left; fl.discard_large_update = discard_large;
    fl.noise_feature = 0.008; fl.chi2_prob = 0.95;
    return fl;
}

}  // namespace

// The increments behind a given dx [leg + 6 N + d nf + ..] on the state fillState describes (in / out: clone_R, clone_t, imu, param,
// rho; out: cam, position).  Returns 1 if the state was incremented, 0 if the large update was discarded, -1 on an exception.
extern "C" int orc_test_zupt_increment(int leg_dim, int use_larvio, int use_left, int discard_large, int N, double* clone_R, double* clone_t,
                                       double* imu, const double* dx, int n_dx, int idp_dim, int nf, const int* anchor, const double* nui_cam,
                                       int n_nui, double* param, double* rho, double* cam, double* position) {
    const orcvio_msckf_flags fl = makeFlags(leg_dim, use_larvio, use_left, discard_large);
    StateServer ss;
    MapServer ms;
    fillState(ss, ms, N, clone_R, clone_t, imu, idp_dim, nf, anchor, nui_cam, n_nui, param, rho);
    const std::vector<double> d(dx, dx + n_dx);
    int inc;
    try {
        inc = MsckfBackend::applyZuptIncrement(fl, ss, ms, d, idp_dim, n_nui > 0) ? 1 : 0;
    } catch (const std::exception&) {
        return -1;
    }
    readState(ss, ms, clone_R, clone_t, imu, idp_dim, nf, param, rho, cam, position);
    return inc;
}

// NEEDS A GPU.  MsckfBackend::zuptUpdate as a filter calls it: a backend of its own, the state of fillState with P [n][n]
// (n = leg + 6 N + d nf + 6 n_nui) made resident (and factored when prefactor != 0), ORCVIO_OPT_EXTRA_STATES / _SCHMIDT_STATES declared,
// the update, the covariance fetched back.  noise [3]: variances.  Out: P (the resident covariance behind the update), dx [n],
// outcome [3] = status | updated | state_incremented, and the state as orc_test_zupt_increment returns it.  Returns 0, -1 on an
// exception, or the status of the call that failed before the update.
extern "C" int orc_test_zupt_update(int leg_dim, int use_larvio, int use_left, int discard_large, int N, double* clone_R, double* clone_t,
                                    double* imu, int idp_dim, int nf, const int* anchor, const double* nui_cam, int n_nui, double* param,
                                    double* rho, double* cam, double* position, double* P, int n, const double* noise, int prefactor, double* dx,
                                    int* outcome) {
    try {
        MsckfBackend be(0, 40, 64, 1024);
        be.flags = makeFlags(leg_dim, use_larvio, use_left, discard_large);
        StateServer ss;
        MapServer ms;
        fillState(ss, ms, N, clone_R, clone_t, imu, idp_dim, nf, anchor, nui_cam, n_nui, param, rho);
        ss.state_cov.assign(P, P + (size_t)n * n);
        int rc = be.covarianceToDevice(ss);
        if (rc == ORCVIO_OK && prefactor) rc = be.prefactorCovariance();
        if (rc == ORCVIO_OK) rc = orcvio_msckf_set_option(be.handle(), ORCVIO_OPT_EXTRA_STATES, idp_dim * nf + 6 * n_nui);
        if (rc == ORCVIO_OK) rc = orcvio_msckf_set_option(be.handle(), ORCVIO_OPT_SCHMIDT_STATES, n_nui);
        if (rc != ORCVIO_OK) return rc;
        const UpdateOutcome out = be.zuptUpdate(ss, ms, noise[0], noise[1], noise[2], idp_dim, n_nui > 0);
        outcome[0] = out.status; outcome[1] = out.updated ? 1 : 0; outcome[2] = out.state_incremented ? 1 : 0;
        for (int i = 0; i < n; ++i) dx[i] = i < (int)out.delta_x.size() ? out.delta_x[i] : 0.0;
        rc = be.covarianceToHost(ss);
        if (rc != ORCVIO_OK || ss.dim() != n) return rc != ORCVIO_OK ? rc : ORCVIO_ERR_INVALID;
        std::memcpy(P, ss.state_cov.data(), sizeof(double) * (size_t)n * n);
        readState(ss, ms, clone_R, clone_t, imu, idp_dim, nf, param, rho, cam, position);
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}
