// Host half of orcvio_msckf_object_init / orcvio_msckf_object_init_lm (orcvio_amd/csrc/object_mapper_pack.hpp: validation, packing,
// unpacking) on its own, built with -fsanitize=address,undefined by tests/test_object_init_mirror.py: every buffer is a heap block of
// exactly the size the layout asks for, so a write or read past it is reported.  No device, no library.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../../orcvio_amd/csrc/object_mapper_pack.hpp"

using namespace orcvio_amd;

struct Case {
    int K, F;
    std::vector<double> ms, mk, wTc, zs, bb, wTo, kpw, cond, lm;
    std::vector<int32_t> used, obs;
    Case(int K_, int F_, double seed) : K(K_), F(F_), ms(3), mk(3 * K_), wTc(16 * F_), zs(2 * K_ * F_), bb(4 * F_), wTo(16), kpw(3 * K_), cond(K_),
                                        lm(19 + 3 * K_), used(K_), obs(K_) {
        double v = seed;
        for (auto* a : {&ms, &mk, &wTc, &zs, &bb})
            for (double& x : *a) x = (v += 1.0);
        zs[zs.size() / 2] = std::numeric_limits<double>::quiet_NaN();   // a missed detection is data, not an error
    }
    // what the initialiser does not read is NULL
    orcvio_object_track track(bool with_bbox) const {
        return orcvio_object_track{K, F, nullptr, nullptr, nullptr, wTc.data(), zs.data(), with_bbox ? bb.data() : nullptr, nullptr};
    }
    orcvio_object_lm_prior prior() const { return orcvio_object_lm_prior{ms.data(), mk.data()}; }
    orcvio_object_init_result result() {
        orcvio_object_init_result r{};
        r.wTo = wTo.data(); r.kps_world = kpw.data(); r.kp_used = used.data(); r.kp_obs = obs.data(); r.kp_cond = cond.data();
        return r;
    }
    orcvio_object_lm_result lm_result() { orcvio_object_lm_result r{}; r.wTo = lm.data(); r.shape = lm.data() + 16; r.kps = lm.data() + 19; return r; }
};

static bool same(double a, double b) { return a == b || (a != a && b != b); }   // (a NaN detection travels as it is)

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// Doubly faulty inputs: which of two simultaneous faults the two validators report.  One pair from each two refusal classes (null
// argument, config, capacity of the handle, the per-track checks) and pairs within the per-track checks, for both entry points.  The
// expected code and text of every row were recorded by running the same inputs through the validators of the three pack headers this
// header replaced.
static int double_faults() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<Case> cs;
    const int shapes[][2] = {{3, 4}, {16, 128}, {12, 47}, {5, 2}, {2, 3}};
    for (auto& s : shapes) cs.emplace_back(s[0], s[1], 1000.0 * cs.size());
    Case nan_pose(2, 3, 50.0), nan_bbox(12, 47, 60.0), nan_shape(5, 2, 70.0);
    nan_pose.wTc[7] = nan; nan_bbox.bb.back() = nan; nan_shape.ms[1] = nan;
    struct Args {
        orcvio_object_init_config c{1, 3, 3};
        orcvio_object_lm_config lc{1, 0, {1, 1, 1, 1}, 60, 1e-18};
        std::vector<orcvio_object_track> t;
        std::vector<const double*> m;
        std::vector<orcvio_object_lm_prior> p;
        std::vector<orcvio_object_init_result> r;
        std::vector<orcvio_object_lm_result> l;
        int n = 0;
        bool no_cfg = false, no_lm_cfg = false, no_tracks = false, no_means = false, no_priors = false, no_results = false, no_lm_results = false;
    };
    struct Row { bool lm; const char* name; int rc; const char* why; void (*change)(Args&, const Case&, const Case&, const Case&); };
    #define CH [](Args& a, const Case& np, const Case& nb, const Case& ns)
    #define UNUSED (void)np; (void)nb; (void)ns;
    const Row rows[] = {
        // orcvio_msckf_object_init
        {false, "null results + bad config", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_results = true; a.c.pose_form = 3; }},
        {false, "null means + too many tracks", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_means = true; a.n = 65; }},
        {false, "null config + a track without frames", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_cfg = true; a.t[0].n_frames = 0; }},
        {false, "bad config + too many tracks", ORCVIO_ERR_INVALID, "config: pose_form 0..2, min_obs >= 0, min_kps >= 0", CH { UNUSED a.c.min_obs = -1; a.n = 65; }},
        {false, "bad config + a track without keypoints", ORCVIO_ERR_INVALID, "config: pose_form 0..2, min_obs >= 0, min_kps >= 0", CH { UNUSED a.c.min_kps = -1; a.t[2].n_keypoints = 0; }},
        {false, "too many tracks + 17 keypoints", ORCVIO_ERR_CAPACITY, "more tracks than the handle's capacity (max_features)", CH { UNUSED a.n = 65; a.t[0].n_keypoints = 17; }},
        {false, "null result array + non-finite pose, one track", ORCVIO_ERR_INVALID, "null pointer in a track, mean keypoints or result",
         CH { UNUSED a.t[4] = np.track(false); a.m[4] = np.mk.data(); a.r[4].kp_obs = nullptr; }},
        {false, "no keypoints + 129 frames, one track", ORCVIO_ERR_INVALID, "a track without keypoints (the bbox-only initialiser is another function: not served)",
         CH { UNUSED a.t[3].n_keypoints = 0; a.t[3].n_frames = 129; }},
        {false, "non-finite pose in track 4 + null mean in track 1", ORCVIO_ERR_INVALID, "null pointer in a track, mean keypoints or result",
         CH { UNUSED a.t[4] = np.track(false); a.m[4] = np.mk.data(); a.m[1] = nullptr; }},
        {false, "no frames in track 3 + non-finite pose in track 4", ORCVIO_ERR_INVALID, "a track without frames",
         CH { UNUSED a.t[4] = np.track(false); a.m[4] = np.mk.data(); a.t[3].n_frames = 0; }},
        // orcvio_msckf_object_init_lm
        {true, "null lm results + bad lm config", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_lm_results = true; a.lc.max_iter = 0; }},
        {true, "null results + bad lm config", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights", CH { UNUSED a.no_results = true; a.lc.max_iter = 0; }},
        {true, "null init config + bad lm config", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights", CH { UNUSED a.no_cfg = true; a.lc.ptol = -1.0; }},
        {true, "null tracks + bad init config", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_tracks = true; a.c.pose_form = -1; }},
        {true, "bad lm config + bad init config", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights", CH { UNUSED a.lc.use_new_bbox_residual = 3; a.c.pose_form = 3; }},
        {true, "no tracks + bad init config", ORCVIO_ERR_INVALID, "config: pose_form 0..2, min_obs >= 0, min_kps >= 0", CH { UNUSED a.n = 0; a.c.pose_form = 3; }},
        {true, "no tracks + null init config", ORCVIO_ERR_INVALID, "config: pose_form 0..2, min_obs >= 0, min_kps >= 0", CH { UNUSED a.n = 0; a.no_cfg = true; }},
        {true, "no tracks + bad lm config + bad init config", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights", CH { UNUSED a.n = 0; a.lc.max_iter = 0; a.c.pose_form = 3; }},
        {true, "negative count + bad init config", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.n = -1; a.c.pose_form = 3; }},
        {true, "bad init config + too many tracks", ORCVIO_ERR_INVALID, "config: pose_form 0..2, min_obs >= 0, min_kps >= 0", CH { UNUSED a.c.min_obs = -1; a.n = 65; }},
        {true, "bad lm config + a track without frames", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights", CH { UNUSED a.lc.max_iter = 100001; a.t[0].n_frames = 0; }},
        {true, "too many tracks + null bbox", ORCVIO_ERR_CAPACITY, "more tracks than the handle's capacity (max_features)", CH { UNUSED a.n = 65; a.t[0].frame_bbox = nullptr; }},
        {true, "null bbox + null init result array, one track", ORCVIO_ERR_INVALID, "null pointer in a track, mean keypoints or result",
         CH { UNUSED a.t[1].frame_bbox = nullptr; a.r[1].kp_cond = nullptr; }},
        {true, "null lm result array + non-finite pose, one track", ORCVIO_ERR_INVALID, "null pointer in a track, prior or result of the optimiser",
         CH { UNUSED a.t[4] = np.track(true); a.p[4] = np.prior(); a.l[4].kps = nullptr; }},
        {true, "non-finite bbox + non-finite pose, one track", ORCVIO_ERR_INVALID, "non-finite number in a camera pose or a mean keypoint",
         CH { UNUSED a.t[4] = np.track(true); a.p[4] = np.prior(); a.t[4].frame_bbox = nb.bb.data(); }},
        {true, "non-finite mean shape in track 3 + null mean shape in track 4", ORCVIO_ERR_INVALID, "non-finite number in a mean shape or a bounding box",
         CH { UNUSED a.t[3] = ns.track(true); a.p[3] = ns.prior(); a.p[4].mean_shape = nullptr; }},
        {true, "non-finite bbox in track 2 + 129 frames in track 3", ORCVIO_ERR_INVALID, "non-finite number in a mean shape or a bounding box",
         CH { UNUSED a.t[2] = nb.track(true); a.p[2] = nb.prior(); a.t[3].n_frames = 129; }},
    };
    #undef CH
    #undef UNUSED
    int failed = 0;
    for (const Row& row : rows) {
        Args a;
        for (auto& c : cs) { a.t.push_back(c.track(row.lm)); a.m.push_back(c.mk.data()); a.p.push_back(c.prior()); a.r.push_back(c.result()); a.l.push_back(c.lm_result()); }
        a.n = (int)cs.size();
        row.change(a, nan_pose, nan_bbox, nan_shape);
        const char* why = nullptr;
        size_t nd = 1;
        const int rc = row.lm ? obj_init_lm_validate(a.no_cfg ? nullptr : &a.c, a.no_lm_cfg ? nullptr : &a.lc, a.no_tracks ? nullptr : a.t.data(),
                                                     a.no_priors ? nullptr : a.p.data(), a.n, a.no_results ? nullptr : a.r.data(),
                                                     a.no_lm_results ? nullptr : a.l.data(), 64, &why, &nd)
                              : obj_init_validate(a.no_cfg ? nullptr : &a.c, a.no_tracks ? nullptr : a.t.data(), a.no_means ? nullptr : a.m.data(), a.n,
                                                  a.no_results ? nullptr : a.r.data(), 64, &why, &nd);
        if (rc != row.rc || nd != 0 || !why || std::strcmp(why, row.why) != 0) {
            std::printf("FAILED double fault '%s' (%s): %d \"%s\"\n", row.name, row.lm ? "object_init_lm" : "object_init", rc, why ? why : "(null)");
            ++failed;
        }
    }
    return failed;
}

int main() {
    const orcvio_object_init_config cfg{1, 3, 3};
    const orcvio_object_lm_config lcfg{1, 0, {1, 1, 1, 1}, 60, 1e-18};
    std::vector<Case> cs;
    const int shapes[][2] = {{1, 1}, {16, 128}, {12, 47}, {4, 4}, {16, 1}, {1, 128}, {12, 65}};   // a mixed batch
    for (auto& s : shapes) cs.emplace_back(s[0], s[1], 1000.0 * cs.size());
    const int n = (int)cs.size();
    std::vector<orcvio_object_track> tracks, tracks_lm;
    std::vector<const double*> mean;
    std::vector<orcvio_object_lm_prior> priors;
    std::vector<orcvio_object_init_result> results;
    std::vector<orcvio_object_lm_result> lm_results;
    for (auto& c : cs) {
        tracks.push_back(c.track(false)); tracks_lm.push_back(c.track(true)); mean.push_back(c.mk.data());
        priors.push_back(c.prior()); results.push_back(c.result()); lm_results.push_back(c.lm_result());
    }
    const char* why = nullptr;
    size_t nd = 0, nd_lm = 0;
    // the NULL optional pointers (wTo, shape, kps, frame_bbox, frame_clone) pass the initialiser's validation
    CHECK(obj_init_validate(&cfg, tracks.data(), mean.data(), n, results.data(), 64, &why, &nd) == ORCVIO_OK);
    CHECK(obj_init_lm_validate(&cfg, &lcfg, tracks_lm.data(), priors.data(), n, results.data(), lm_results.data(), 64, &why, &nd_lm) == ORCVIO_OK);
    size_t want = 0;
    for (auto& c : cs) want += 16 + 3 + 3 * c.K + 3 + 3 * c.K + c.F * (16 + 2 * c.K + 4);
    CHECK(nd == want && nd_lm == want);
    // pack into blocks of exactly the announced size: offsets of the mixed batch, zeros where the kernel writes or nothing is given
    for (int with_lm = 0; with_lm < 2; ++with_lm) {
        std::unique_ptr<ObjLmTrack[]> recs(new ObjLmTrack[n]);
        std::unique_ptr<double[]> in(new double[nd]);
        for (size_t i = 0; i < nd; ++i) in[i] = -7.0;
        const ObjMapIo io = with_lm ? obj_io_init(nullptr, priors.data(), results.data(), lm_results.data()) : obj_io_init(mean.data(), nullptr, results.data(), nullptr);
        obj_map_pack(io, with_lm ? tracks_lm.data() : tracks.data(), n, recs.get(), in.get());
        size_t off = 0;
        for (int q = 0; q < n; ++q) {
            const Case& c = cs[q];
            CHECK(recs[q].K == c.K && recs[q].F == c.F && (size_t)recs[q].off == off && recs[q].pad == 0);
            const double* p = in.get() + off;
            for (int i = 0; i < 19 + 3 * c.K; ++i) CHECK(p[i] == 0.0);
            CHECK(p[19 + 3 * c.K] == (with_lm ? c.ms[0] : 0.0) && p[21 + 3 * c.K] == (with_lm ? c.ms[2] : 0.0));
            CHECK(p[22 + 3 * c.K] == c.mk[0] && p[22 + 6 * c.K - 1] == c.mk.back());
            CHECK(p[22 + 6 * c.K] == c.wTc[0] && p[22 + 6 * c.K + 16 * c.F - 1] == c.wTc.back());
            for (int i = 0; i < 2 * c.K * c.F; ++i) CHECK(same(p[22 + 6 * c.K + 16 * c.F + i], c.zs[i]));
            const size_t last = obj_lm_track_doubles(c.K, c.F) - 1;
            CHECK(p[last - 4 * c.F + 1] == (with_lm ? c.bb[0] : 0.0) && p[last] == (with_lm ? c.bb.back() : 0.0));
            off += last + 1;
        }
        CHECK(off == nd);
    }
    // unpack from a block of exactly n x OBJ_INIT_OUT
    std::unique_ptr<double[]> out(new double[(size_t)n * OBJ_INIT_OUT]);
    for (size_t i = 0; i < (size_t)n * OBJ_INIT_OUT; ++i) out[i] = (double)(i % 1000);
    obj_init_unpack(out.get(), tracks.data(), n, results.data());
    for (int q = 0; q < n; ++q) {
        const double* o = out.get() + (size_t)q * OBJ_INIT_OUT;
        const Case& c = cs[q];
        CHECK(c.wTo[0] == o[0] && c.wTo[15] == o[15] && results[q].R_kabsch[0] == o[16] && results[q].R_kabsch[8] == o[24]);
        CHECK(results[q].t_kabsch[0] == o[25] && results[q].t_kabsch[2] == o[27] && results[q].scale == o[28]);
        CHECK(results[q].sigma[0] == o[29] && results[q].sigma[2] == o[31]);
        CHECK(c.kpw[0] == o[32] && c.kpw.back() == o[32 + 3 * c.K - 1]);
        CHECK(c.used[0] == (int32_t)o[80] && c.used.back() == (int32_t)o[80 + c.K - 1] && c.obs[0] == (int32_t)o[96] && c.obs.back() == (int32_t)o[96 + c.K - 1]);
        CHECK(c.cond[0] == o[112] && c.cond.back() == o[112 + c.K - 1]);
        CHECK(results[q].n_used == (int32_t)o[128] && results[q].status == (int32_t)o[129]);
    }
    // refusals: nothing read beyond what the refusal needs
    using T = std::vector<orcvio_object_track>; using M = std::vector<const double*>; using R = std::vector<orcvio_object_init_result>;
    using Cf = orcvio_object_init_config;
    auto refuse = [&](int want_rc, auto&& change) {
        T t = tracks; M m = mean; R r = results; Cf c = cfg;
        change(t, m, r, c);
        size_t nd2 = 1;
        const int rc = obj_init_validate(&c, t.data(), m.data(), n, r.data(), 64, &why, &nd2);
        return rc == want_rc && nd2 == 0 && why && why[0];
    };
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, M&, R&, Cf&) { t[2].n_keypoints = 0; }));      // K = 0: the bbox-only initialiser, another function
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, M&, R&, Cf&) { t[2].n_keypoints = -1; }));
    CHECK(refuse(ORCVIO_ERR_CAPACITY, [](T& t, M&, R&, Cf&) { t[2].n_keypoints = 17; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, M&, R&, Cf&) { t[5].n_frames = 0; }));
    CHECK(refuse(ORCVIO_ERR_CAPACITY, [](T& t, M&, R&, Cf&) { t[5].n_frames = 129; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, M&, R&, Cf&) { t[1].frame_wTc = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, M&, R&, Cf&) { t[3].frame_zs = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, M& m, R&, Cf&) { m[4] = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, M&, R& r, Cf&) { r[0].wTo = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, M&, R& r, Cf&) { r[6].kps_world = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, M&, R& r, Cf&) { r[6].kp_used = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, M&, R& r, Cf&) { r[6].kp_obs = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, M&, R& r, Cf&) { r[6].kp_cond = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, M&, R&, Cf& c) { c.pose_form = 3; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, M&, R&, Cf& c) { c.pose_form = -1; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, M&, R&, Cf& c) { c.min_obs = -1; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, M&, R&, Cf& c) { c.min_kps = -1; }));
    {   // a NaN in the last camera pose of the longest track, an infinity in a mean keypoint
        Case bad(16, 128, 5.0);
        bad.wTc.back() = std::numeric_limits<double>::quiet_NaN();
        CHECK(refuse(ORCVIO_ERR_INVALID, [&](T& t, M& m, R&, Cf&) { t[1] = bad.track(false); m[1] = bad.mk.data(); }));
        Case bad2(12, 47, 6.0);
        bad2.mk.back() = std::numeric_limits<double>::infinity();
        CHECK(refuse(ORCVIO_ERR_INVALID, [&](T& t, M& m, R&, Cf&) { t[2] = bad2.track(false); m[2] = bad2.mk.data(); }));
    }
    size_t nd3 = 1;
    CHECK(obj_init_validate(&cfg, tracks.data(), mean.data(), 65, results.data(), 64, &why, &nd3) == ORCVIO_ERR_CAPACITY);   // (refused before track 7 would be read)
    CHECK(obj_init_validate(&cfg, nullptr, nullptr, 0, nullptr, 64, &why, &nd3) == ORCVIO_OK && nd3 == 0);
    CHECK(obj_init_validate(nullptr, tracks.data(), mean.data(), n, results.data(), 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    CHECK(obj_init_validate(&cfg, nullptr, mean.data(), n, results.data(), 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    CHECK(obj_init_validate(&cfg, tracks.data(), nullptr, n, results.data(), 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    CHECK(obj_init_validate(&cfg, tracks.data(), mean.data(), n, nullptr, 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    // the one call with the optimiser behind: the optimiser's inputs are checked as well
    using P = std::vector<orcvio_object_lm_prior>; using L = std::vector<orcvio_object_lm_result>; using Lc = orcvio_object_lm_config;
    auto refuse_lm = [&](int want_rc, auto&& change) {
        T t = tracks_lm; P p = priors; R r = results; L l = lm_results; Cf c = cfg; Lc lc = lcfg;
        change(t, p, r, l, c, lc);
        size_t nd2 = 1;
        const int rc = obj_init_lm_validate(&c, &lc, t.data(), p.data(), n, r.data(), l.data(), 64, &why, &nd2);
        return rc == want_rc && nd2 == 0 && why && why[0];
    };
    CHECK(refuse_lm(ORCVIO_ERR_INVALID, [](T& t, P&, R&, L&, Cf&, Lc&) { t[1].frame_bbox = nullptr; }));
    CHECK(refuse_lm(ORCVIO_ERR_INVALID, [](T&, P& p, R&, L&, Cf&, Lc&) { p[3].mean_shape = nullptr; }));
    CHECK(refuse_lm(ORCVIO_ERR_INVALID, [](T&, P& p, R&, L&, Cf&, Lc&) { p[3].mean_kps = nullptr; }));
    CHECK(refuse_lm(ORCVIO_ERR_INVALID, [](T&, P&, R&, L& l, Cf&, Lc&) { l[4].shape = nullptr; }));
    CHECK(refuse_lm(ORCVIO_ERR_INVALID, [](T&, P&, R& r, L&, Cf&, Lc&) { r[4].kp_cond = nullptr; }));
    CHECK(refuse_lm(ORCVIO_ERR_INVALID, [](T&, P&, R&, L&, Cf& c, Lc&) { c.pose_form = 3; }));
    CHECK(refuse_lm(ORCVIO_ERR_INVALID, [](T&, P&, R&, L&, Cf&, Lc& lc) { lc.max_iter = 0; }));
    CHECK(refuse_lm(ORCVIO_ERR_INVALID, [](T&, P&, R&, L&, Cf&, Lc& lc) { lc.residual_weights[1] = std::numeric_limits<double>::quiet_NaN(); }));
    CHECK(refuse_lm(ORCVIO_ERR_CAPACITY, [](T& t, P&, R&, L&, Cf&, Lc&) { t[0].n_frames = 129; }));
    {
        Case bad(12, 47, 7.0);
        bad.bb[5] = std::numeric_limits<double>::quiet_NaN();
        CHECK(refuse_lm(ORCVIO_ERR_INVALID, [&](T& t, P& p, R&, L&, Cf&, Lc&) { t[2] = bad.track(true); p[2] = bad.prior(); }));
    }
    CHECK(obj_init_lm_validate(&cfg, nullptr, tracks_lm.data(), priors.data(), n, results.data(), lm_results.data(), 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    CHECK(obj_init_lm_validate(nullptr, &lcfg, tracks_lm.data(), priors.data(), n, results.data(), lm_results.data(), 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    CHECK(obj_init_lm_validate(&cfg, &lcfg, tracks_lm.data(), nullptr, n, results.data(), lm_results.data(), 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    CHECK(obj_init_lm_validate(&cfg, &lcfg, tracks_lm.data(), priors.data(), n, results.data(), nullptr, 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    CHECK(obj_init_lm_validate(&cfg, &lcfg, tracks_lm.data(), priors.data(), 65, results.data(), lm_results.data(), 64, &why, &nd3) == ORCVIO_ERR_CAPACITY);
    CHECK(obj_init_lm_validate(&cfg, &lcfg, nullptr, nullptr, 0, nullptr, nullptr, 64, &why, &nd3) == ORCVIO_OK && nd3 == 0);
    CHECK(double_faults() == 0);
    std::printf("object init pack ok\n");
    return 0;
}
