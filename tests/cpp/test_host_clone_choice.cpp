// GPU test of the host layer's checked choice of the clones that leave (MsckfBackend::findRedundantImuStates and the frame call site
// ::stepFrameChosen: orcvio_msckf_io_choose_clones + orcvio_msckf_io_triangulate_prune + orcvio_msckf_io_step_frame) on std::map
// containers.  Two prune frames on the scene of tests/cpp/test_host_prune_tri.cpp, one whose prediction holds and one whose prediction
// does not: the rotation threshold of the second is placed at the midpoint between the compared clone's angle before and after the
// first update.  Each frame runs twice -- through the new call site, and through the separate calls in the reference's order (the first
// half as a frame, findRedundantImuStates on the host on the incremented containers, the second half as a frame) -- and the state and
// the covariance are compared afterwards (1e-6 relative: the tolerance tests/test_gpu_prune_tri.py uses for this chain).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../orcvio_amd/csrc/host/orcvio_msckf_host.hpp"

using namespace orcvio_amd;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Scene { StateServer ss; MapServer map; std::vector<FeatureIDType> lost; StateIDType curr_id; };

static Scene make_scene() {
    Scene sc;
    const int N = 8, F = 48;
    std::mt19937 rng(11);
    std::normal_distribution<double> G(0, 1);
    std::uniform_real_distribution<double> U(0, 1);
    StateServer& ss = sc.ss;
    const double Rbc[9] = {0, -1, 0, 0, 0, -1, 1, 0, 0};   // the camera looks along body x
    for (int i = 0; i < N; ++i) {
        IMUState_Aug a; a.id = 100 + 2 * i;
        const double ang = 0.02 * i + 0.004 * std::sin(1.3 * i);
        const double R[9] = {std::cos(ang), -std::sin(ang), 0, std::sin(ang), std::cos(ang), 0, 0, 0, 1};
        std::memcpy(a.orientation, R, sizeof(R));
        a.position[0] = 0.03 * i; a.position[1] = 0.3 * i; a.position[2] = 0.02 * std::sin(0.7 * i);
        for (int k = 0; k < 3; ++k) a.position_FEJ[k] = a.position[k];
        std::memcpy(a.R_imu_cam0, Rbc, sizeof(Rbc));
        a.t_cam0_imu[0] = 0.05; a.t_cam0_imu[1] = 0.02; a.t_cam0_imu[2] = -0.01;
        double cam[12];
        clone_choice_cam_pose(a.orientation, a.position, a.R_imu_cam0, a.t_cam0_imu, cam);
        std::memcpy(a.orientation_cam, cam, 72); std::memcpy(a.position_cam, cam + 9, 24);
        ss.imu_states_augment[a.id] = a;
    }
    ss.imu_state = IMUState();
    std::memcpy(ss.imu_state.R_imu_cam0, Rbc, 72);
    std::memcpy(ss.imu_state.t_cam0_imu, ss.imu_states_augment.begin()->second.t_cam0_imu, 24);
    const int n = 22 + 6 * N;
    ss.state_cov.assign((size_t)n * n, 0.0);
    std::vector<double> A((size_t)n * n);
    for (auto& v : A) v = G(rng) / std::sqrt((double)n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0;
            for (int k = 0; k < n; ++k) s += A[(size_t)i * n + k] * A[(size_t)j * n + k];
            ss.state_cov[(size_t)i * n + j] = 1e-4 * s + (i == j ? 1e-3 : 0.0);
        }
    for (int i = 15; i < 22; ++i)
        for (int j = 0; j < n; ++j) ss.state_cov[(size_t)i * n + j] = ss.state_cov[(size_t)j * n + i] = 0.0;
    sc.curr_id = ss.imu_states_augment.rbegin()->first;
    for (int j = 0; j < F; ++j) {
        Feature f; f.id = 1000 + 3 * j;
        const double pt[3] = {5.0 + 5.0 * U(rng), 0.5 + 1.5 * U(rng), -1.0 + 2.0 * U(rng)};
        const bool tracked = j % 3 != 1;
        const int M = tracked ? N - (j % 2) : 2 + (int)(U(rng) * (N - 2));   // tracked features see (nearly) the whole window: every remove set has its prune features
        const int s0 = tracked ? N - M : (int)(U(rng) * (N - M));
        int i = 0;
        for (auto& kv : ss.imu_states_augment) {
            if (i >= s0 && i < s0 + M) {
                const IMUState_Aug& a = kv.second;
                double d[3], pc[3];
                for (int k = 0; k < 3; ++k) d[k] = pt[k] - a.position_cam[k];
                for (int k = 0; k < 3; ++k) pc[k] = a.orientation_cam[k] * d[0] + a.orientation_cam[3 + k] * d[1] + a.orientation_cam[6 + k] * d[2];   // R_c2w^T d
                const double noise = (j % 7 == 0) ? 0.1 : 0.002;
                f.observations[kv.first] = {pc[0] / pc[2] + noise * G(rng), pc[1] / pc[2] + noise * G(rng)};
                f.observations_vel[kv.first] = {0.01 * G(rng), 0.01 * G(rng)};
            }
            ++i;
        }
        const bool lost = !tracked && f.observations.size() >= 3;
        if (lost || j % 5 == 2) {
            f.is_initialized = true;
            for (int k = 0; k < 3; ++k) f.position[k] = f.position_FEJ[k] = pt[k] + 0.01 * G(rng);
            f.id_anchor = f.observations.begin()->first; f.invDepth = 0.125; f.invParam[0] = 0.1; f.invParam[1] = -0.2; f.invParam[2] = 0.125;
        } else {
            for (int k = 0; k < 3; ++k) f.position[k] = std::nan("");
        }
        if (lost) sc.lost.push_back(f.id);
        sc.map[f.id] = f;
    }
    return sc;
}

static double rel_diff(const std::vector<double>& a, const std::vector<double>& b) {
    if (a.size() != b.size()) return 1e300;
    double num = 0, den = 0;
    for (size_t i = 0; i < a.size(); ++i) { num += (a[i] - b[i]) * (a[i] - b[i]); den += b[i] * b[i]; }
    return std::sqrt(num / (den > 0 ? den : 1.0));
}
static std::vector<double> state_vector(const StateServer& ss) {
    std::vector<double> v;
    for (const auto& kv : ss.imu_states_augment) {
        const IMUState_Aug& a = kv.second;
        v.insert(v.end(), a.orientation, a.orientation + 9); v.insert(v.end(), a.position, a.position + 3);
        v.insert(v.end(), a.orientation_cam, a.orientation_cam + 9); v.insert(v.end(), a.position_cam, a.position_cam + 3);
    }
    v.insert(v.end(), ss.imu_state.R_imu_cam0, ss.imu_state.R_imu_cam0 + 9); v.insert(v.end(), ss.imu_state.t_cam0_imu, ss.imu_state.t_cam0_imu + 3);
    return v;
}

// one frame both ways; differ: place the rotation threshold between the pre- and the post-update angle of the clone compared first
static int run_frame(bool differ) {
    typedef MsckfBackend::CloneChoiceThresholds Thr;
    const double tracking_rate = 0.9;
    Scene ref = make_scene(), one = make_scene();
    CHECK(ref.lost.size() >= 5);
    const int n = ref.ss.dim();
    // ---- the reference's order through the separate calls
    MsckfBackend br(0, 16, 256, 8192), bo(0, 16, 256, 8192);
    Thr thr;
    thr.translation_threshold = 1e3;
    CloneChoice pre{}, post{};
    MsckfBackend::findRedundantImuStates(ref.ss, tracking_rate, thr, &pre);
    CHECK(br.covarianceToDevice(ref.ss) == ORCVIO_OK);
    UpdateOutcome o1 = br.stepFramePruneArmed(ref.ss, ref.map, ref.lost, {}, ref.curr_id);
    if (o1.status != ORCVIO_OK) { std::printf("FAILED: first half %d: %s\n", o1.status, orcvio_msckf_last_error()); return 1; }
    CHECK(o1.updated && o1.state_incremented);
    MsckfBackend::findRedundantImuStates(ref.ss, tracking_rate, thr, &post);
    CHECK(pre.compared[0] == post.compared[0] && std::fabs(pre.angle[0] - post.angle[0]) > 1e-9);
    thr.rotation_threshold = differ ? 0.5 * (pre.angle[0] + post.angle[0]) : 4.0 * std::fmax(std::fmax(pre.angle[0], pre.angle[1]), std::fmax(post.angle[0], post.angle[1]));
    const std::vector<StateIDType> predicted = MsckfBackend::findRedundantImuStates(one.ss, tracking_rate, thr);
    const std::vector<StateIDType> chosen = MsckfBackend::findRedundantImuStates(ref.ss, tracking_rate, thr, &post);
    CHECK(predicted.size() == 2 && chosen.size() == 2 && (predicted != chosen) == differ);
    CHECK(std::fabs(post.angle[0] - thr.rotation_threshold) > 1e-6 * std::fmax(1.0, thr.rotation_threshold) && std::fabs(pre.angle[0] - thr.rotation_threshold) > 1e-6 * std::fmax(1.0, thr.rotation_threshold));
    UpdateOutcome o2 = br.stepFramePruneArmed(ref.ss, ref.map, {}, chosen, ref.curr_id);
    if (o2.status != ORCVIO_OK) { std::printf("FAILED: second half %d: %s\n", o2.status, orcvio_msckf_last_error()); return 1; }
    CHECK(o2.updated);
    StateServer Pr;
    CHECK(br.covarianceToHost(Pr) == ORCVIO_OK && Pr.dim() == n - 12);
    // ---- the new call site
    CHECK(bo.covarianceToDevice(one.ss) == ORCVIO_OK);
    MsckfBackend::FrameChosenReport rep;
    UpdateOutcome oc = bo.stepFrameChosen(one.ss, one.map, one.lost, tracking_rate, thr, one.curr_id, &rep);
    if (oc.status != ORCVIO_OK) { std::printf("FAILED: stepFrameChosen %d: %s\n", oc.status, orcvio_msckf_last_error()); return 1; }
    CHECK(rep.path == (differ ? 2 : 1) && rep.predicted == predicted && rep.chosen == chosen && rep.choice.evaluated == 1 && rep.choice.agree == (differ ? 0 : 1));
    CHECK(rep.choice.compared[0] == post.compared[0] && rep.choice.taken[0] == post.taken[0] && rep.choice.taken[1] == post.taken[1]);
    CHECK(oc.updated && oc.state_incremented);
    StateServer Po;
    CHECK(bo.covarianceToHost(Po) == ORCVIO_OK && Po.dim() == n - 12);
    const double e_state = rel_diff(state_vector(one.ss), state_vector(ref.ss)), e_P = rel_diff(Po.state_cov, Pr.state_cov);
    double e_feat = 0.0;
    int n_init = 0;
    for (const auto& kv : ref.map) {
        const Feature& a = one.map.at(kv.first);
        CHECK(a.is_initialized == kv.second.is_initialized);
        if (!a.is_initialized) continue;
        ++n_init;
        for (int k = 0; k < 3; ++k) e_feat = std::fmax(e_feat, std::fabs(a.position[k] - kv.second.position[k]) / std::fmax(1.0, std::fabs(kv.second.position[k])));
    }
    std::printf("%s: predicted {%lld, %lld} chosen {%lld, %lld} path %d | angle %.6f -> %.6f threshold %.6f | state %.2e  P %.2e  features %.2e (%d initialised)\n",
                differ ? "differ" : "agree", predicted[0], predicted[1], chosen[0], chosen[1], rep.path, pre.angle[0], post.angle[0], thr.rotation_threshold,
                e_state, e_P, e_feat, n_init);
    CHECK(e_state < 1e-6 && e_P < 1e-6 && e_feat < 1e-6);
    return 0;
}

int main() {
    setvbuf(stdout, nullptr, _IONBF, 0);
    {   // findRedundantImuStates on containers: fewer than six clones -> nothing
        Scene s = make_scene();
        while (s.ss.imu_states_augment.size() > 5) s.ss.imu_states_augment.erase(s.ss.imu_states_augment.begin());
        CHECK(MsckfBackend::findRedundantImuStates(s.ss, 0.9, MsckfBackend::CloneChoiceThresholds()).empty());
    }
    if (run_frame(false)) return 1;
    if (run_frame(true)) return 1;
    std::printf("host clone choice ok\n");
    return 0;
}
