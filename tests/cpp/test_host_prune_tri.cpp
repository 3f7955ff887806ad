// GPU test of the host layer's prune triangulation (MsckfBackend::buildPruneTriLists, ::writeBackPruneTriangulation and the frame call
// site ::stepFramePruneArmed: orcvio_msckf_io_triangulate_prune + orcvio_msckf_io_step_frame).  The selection and the write-back are
// checked here against the reference's rules (src/orcvio.cpp:2647-2793, feature.hpp:485-497); the frame's inputs and results are
// printed (hex floats) for tests/test_gpu_prune_tri_host.py, which makes the same frame through the ctypes binding and holds the two
// bit for bit.  The scene is tests/cpp/test_host_io_triangulate.cpp's: a window moving sideways to its viewing direction.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "../../orcvio_amd/csrc/host/orcvio_msckf_host.hpp"

using namespace orcvio_amd;

static void dump(const char* key, const double* v, size_t n) {
    std::printf("D %s %zu", key, n);
    for (size_t i = 0; i < n; ++i) std::printf(" %a", v[i]);
    std::printf("\n");
}
static void dump(const char* key, const std::vector<double>& v) { dump(key, v.data(), v.size()); }
static void dumpi(const char* key, const int32_t* v, size_t n) {
    std::printf("I %s %zu", key, n);
    for (size_t i = 0; i < n; ++i) std::printf(" %d", v[i]);
    std::printf("\n");
}
static void dumpi(const char* key, const std::vector<int32_t>& v) { dumpi(key, v.data(), v.size()); }
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    setvbuf(stdout, nullptr, _IONBF, 0);
    const int N = 8, F = 48;
    std::mt19937 rng(11);
    std::normal_distribution<double> G(0, 1);
    std::uniform_real_distribution<double> U(0, 1);
    StateServer ss;
    for (int i = 0; i < N; ++i) {
        IMUState_Aug a; a.id = 100 + 2 * i;
        const double ang = 0.02 * i;
        const double R[9] = {std::cos(ang), -std::sin(ang), 0, std::sin(ang), std::cos(ang), 0, 0, 0, 1};
        std::memcpy(a.orientation, R, sizeof(R));
        a.position[0] = 0.03 * i; a.position[1] = 0.3 * i; a.position[2] = 0.02 * std::sin(0.7 * i);
        for (int k = 0; k < 3; ++k) a.position_FEJ[k] = a.position[k];
        const double Rbc[9] = {0, -1, 0, 0, 0, -1, 1, 0, 0};   // the camera looks along body x
        std::memcpy(a.R_imu_cam0, Rbc, sizeof(Rbc));
        a.t_cam0_imu[0] = 0.05; a.t_cam0_imu[1] = 0.02; a.t_cam0_imu[2] = -0.01;
        ss.imu_states_augment[a.id] = a;
    }
    ss.imu_state = IMUState();
    std::memcpy(ss.imu_state.R_imu_cam0, ss.imu_states_augment.begin()->second.R_imu_cam0, 72);
    std::memcpy(ss.imu_state.t_cam0_imu, ss.imu_states_augment.begin()->second.t_cam0_imu, 24);
    const int n = 22 + 6 * N;
    ss.state_cov.assign((size_t)n * n, 0.0);
    {
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
    }
    std::vector<StateIDType> clone_ids;
    for (auto& kv : ss.imu_states_augment) clone_ids.push_back(kv.first);
    const StateIDType curr_id = clone_ids[N - 1];
    const std::vector<StateIDType> rm = {clone_ids[N - 2], clone_ids[N - 3]};   // (the reference lists them newest first)
    MapServer map_server;
    std::vector<FeatureIDType> lost_ids;
    std::set<FeatureIDType> expect;
    int n_init = 0;
    for (int j = 0; j < F; ++j) {
        Feature f; f.id = 1000 + 3 * j;
        const double pt[3] = {5.0 + 5.0 * U(rng), 0.5 + 1.5 * U(rng), -1.0 + 2.0 * U(rng)};
        const bool tracked = j % 3 != 1;
        const int M = 2 + (int)(U(rng) * (N - 2));
        const int s0 = tracked ? N - M : (int)(U(rng) * (N - M));   // a tracked feature's track ends at the newest clone
        int i = 0;
        for (auto& kv : ss.imu_states_augment) {
            if (i >= s0 && i < s0 + M && !(j % 11 == 4 && i == N - 3)) {   // (every 11th misses the third-newest clone: one involved clone only)
                const IMUState_Aug& a = kv.second;
                double tcw[3], d[3], pc[3], Rwc[9];
                for (int k = 0; k < 3; ++k) tcw[k] = a.position[k] + a.orientation[k * 3] * a.t_cam0_imu[0] + a.orientation[k * 3 + 1] * a.t_cam0_imu[1] + a.orientation[k * 3 + 2] * a.t_cam0_imu[2];
                for (int k = 0; k < 3; ++k) d[k] = pt[k] - tcw[k];
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rwc[r * 3 + c] = a.R_imu_cam0[r * 3] * a.orientation[c * 3] + a.R_imu_cam0[r * 3 + 1] * a.orientation[c * 3 + 1] + a.R_imu_cam0[r * 3 + 2] * a.orientation[c * 3 + 2];
                for (int k = 0; k < 3; ++k) pc[k] = Rwc[k * 3] * d[0] + Rwc[k * 3 + 1] * d[1] + Rwc[k * 3 + 2] * d[2];
                const double noise = (j % 7 == 0) ? 0.1 : 0.002;   // every 7th track is an outlier
                f.observations[kv.first] = {pc[0] / pc[2] + noise * G(rng), pc[1] / pc[2] + noise * G(rng)};
                f.observations_vel[kv.first] = {0.01 * G(rng), 0.01 * G(rng)};
            }
            ++i;
        }
        f.in_state = tracked && j % 13 == 5;   // an EKF-SLAM feature: not for the prune update
        const bool lost = !tracked && f.observations.size() >= 3;
        if (lost || j % 5 == 2 || f.in_state) {   // has its position already
            f.is_initialized = true;
            for (int k = 0; k < 3; ++k) f.position[k] = f.position_FEJ[k] = pt[k] + 0.01 * G(rng);
            f.id_anchor = f.observations.begin()->first; f.invDepth = 0.125; f.invParam[0] = 0.1; f.invParam[1] = -0.2; f.invParam[2] = 0.125;
        } else {
            for (int k = 0; k < 3; ++k) f.position[k] = std::nan("");   // nothing may read it
        }
        if (lost) lost_ids.push_back(f.id);
        if (tracked && !f.in_state && f.observations.count(rm[0]) && f.observations.count(rm[1])) { expect.insert(f.id); n_init += f.is_initialized; }
        map_server[f.id] = f;
    }
    CHECK(expect.size() >= 12 && n_init >= 2 && (int)expect.size() - n_init >= 8 && lost_ids.size() >= 5);

    // ---- the selection
    const MsckfBackend::PruneTriLists l0 = MsckfBackend::buildPruneTriLists(ss, map_server, rm, curr_id);
    CHECK(std::set<FeatureIDType>(l0.ids.begin(), l0.ids.end()) == expect && l0.ids.size() == expect.size());
    CHECK(std::is_sorted(l0.ids.begin(), l0.ids.end()));   // map_server order
    CHECK(l0.remove_idx == (std::vector<int32_t>{N - 3, N - 2}));
    for (size_t k = 0; k < l0.ids.size(); ++k) {
        const Feature& f = map_server.at(l0.ids[k]);
        CHECK(l0.mode[k] == (f.is_initialized ? ORCVIO_TRI_KEEP : ORCVIO_TRI_ALL_MOTION_BUT_LAST));
        CHECK(l0.tri_ptr[k + 1] - l0.tri_ptr[k] == (int)f.observations.size() && l0.prune_ptr[k + 1] - l0.prune_ptr[k] == 2);
        CHECK(l0.tri_clone[l0.tri_ptr[k + 1] - 1] == N - 1 && l0.anchor[k] == curr_id);
        CHECK(l0.prune_clone[l0.prune_ptr[k]] == N - 3 && l0.prune_clone[l0.prune_ptr[k] + 1] == N - 2);
        for (int o = l0.tri_ptr[k]; o + 1 < l0.tri_ptr[k + 1]; ++o) CHECK(l0.tri_clone[o] < l0.tri_clone[o + 1]);
    }

    // ---- the frame
    MsckfBackend be(0, 16, 256, 8192);
    {   // what the binding's call needs: the window, P, the first update's tracks
        std::vector<double> R_b2w, t_b_w, t_fej, R_b2c, t_c_b, p_w, z, zv;
        std::vector<int32_t> ptr, cl;
        std::map<StateIDType, int> index_of;
        MsckfBackend::flattenWindow(ss, R_b2w, t_b_w, t_fej, R_b2c, t_c_b, index_of);
        MsckfBackend::flattenTracks(map_server, lost_ids, index_of, {}, p_w, ptr, cl, z, zv);
        dump("R_b2w", R_b2w); dump("t_b_w", t_b_w); dump("t_fej", t_fej); dump("R_b2c", R_b2c); dump("t_c_b", t_c_b); dump("P", ss.state_cov);
        dump("first_p_w", p_w); dumpi("first_ptr", ptr); dumpi("first_clone", cl); dump("first_z", z); dump("first_zvel", zv);
    }
    CHECK(be.covarianceToDevice(ss) == ORCVIO_OK);
    MapServer before = map_server;
    MsckfBackend::PruneTriLists l;
    orcvio_msckf_frame_result res{};
    orcvio_msckf_io_tri tri{};
    const UpdateOutcome out = be.stepFramePruneArmed(ss, map_server, lost_ids, rm, curr_id, &l, &res, &tri);
    if (out.status != ORCVIO_OK) { std::printf("FAILED: frame status %d: %s\n", out.status, orcvio_msckf_last_error()); return 1; }
    CHECK(l.ids == l0.ids && l.tri_clone == l0.tri_clone && l.prune_z == l0.prune_z && res.status_first == ORCVIO_OK && res.status_prune == ORCVIO_OK);
    const size_t F2 = l.ids.size();
    dump("prune_p_w", l.p_w); dumpi("mode", l.mode); dumpi("remove", l.remove_idx);
    dumpi("tri_ptr", l.tri_ptr); dumpi("tri_clone", l.tri_clone); dump("tri_z", l.tri_z);
    dumpi("prune_ptr", l.prune_ptr); dumpi("prune_clone", l.prune_clone); dump("prune_z", l.prune_z); dump("prune_zvel", l.prune_zvel);
    dump("dx", res.dx, n); dump("prune_dx", res.prune_dx, n); dump("prune_gamma", res.prune_gamma, F2); dumpi("prune_accept", res.prune_accept, F2);
    dumpi("tri_valid", tri.valid, F2); dumpi("tri_flags", tri.flags, F2); dump("tri_p_w", tri.p_w, 3 * F2); dump("tri_solution", tri.inv_param, 3 * F2);
    dump("tri_cost", tri.cost, F2);
    {
        StateServer got;
        CHECK(be.covarianceToHost(got) == ORCVIO_OK && got.dim() == n - 12 && res.n_after == n - 12);
        dump("P_after", got.state_cov);
    }
    // ---- the write-back (feature.hpp:485-497)
    int n_valid = 0, n_failed = 0;
    for (size_t k = 0; k < F2; ++k) {
        const Feature& f = map_server.at(l.ids[k]);
        const Feature& b = before.at(l.ids[k]);
        if (l.mode[k] == ORCVIO_TRI_KEEP) {
            CHECK(tri.valid[k] == 1 && std::memcmp(f.position, b.position, 24) == 0 && std::memcmp(f.invParam, b.invParam, 24) == 0 && f.id_anchor == b.id_anchor);
            continue;
        }
        if (!tri.valid[k]) { ++n_failed; CHECK(!f.is_initialized && res.prune_accept[k] == 0 && std::isnan(res.prune_gamma[k])); continue; }
        ++n_valid;
        CHECK(f.is_initialized && std::memcmp(f.position, tri.p_w + 3 * k, 24) == 0 && std::memcmp(f.invParam, tri.inv_param + 3 * k, 24) == 0);
        CHECK(std::memcmp(f.position_FEJ, b.position, 24) == 0);   // (the position in front of the first initialisation, :485-486)
        CHECK(f.id_anchor == curr_id && f.invDepth == tri.inv_param[3 * k + 2] && f.obs_anchor[0] == tri.inv_param[3 * k] && f.obs_anchor[1] == tri.inv_param[3 * k + 1] && f.obs_anchor[2] == 1.0);
        CHECK(f.failed_by_neg_dpth == false && f.failed_by_big_proj == false);
    }
    for (const auto& kv : map_server)   // nothing else was touched
        if (!expect.count(kv.first)) CHECK(std::memcmp(kv.second.position, before.at(kv.first).position, 24) == 0 || std::isnan(kv.second.position[0]));
    std::printf("selected %zu (initialised %d), valid %d, failed %d, lost %zu\n", F2, n_init, n_valid, n_failed, lost_ids.size());
    CHECK(n_valid >= 5 && n_failed >= 1 && out.updated);
    std::printf("host prune tri ok\n");
    return 0;
}
