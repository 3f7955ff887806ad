// Host half of orcvio_msckf_object_lm (orcvio_amd/csrc/object_mapper_pack.hpp: validation, packing, unpacking) on its own, built with
// -fsanitize=address,undefined by tests/test_object_lm_pack.py: every buffer is a heap block of exactly the size the layout asks
// for, so a write or read past it is reported.  No device, no library.
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
    std::vector<double> wTo, shape, kps, ms, mk, wTc, zs, bb, out;
    Case(int K_, int F_, double seed) : K(K_), F(F_), wTo(16), shape(3), kps(3 * K_), ms(3), mk(3 * K_), wTc(16 * F_), zs(2 * K_ * F_), bb(4 * F_),
                                        out(19 + 3 * K_) {
        double v = seed;
        for (auto* a : {&wTo, &shape, &kps, &ms, &mk, &wTc, &zs, &bb})
            for (double& x : *a) x = (v += 1.0);
        if (!zs.empty()) zs[zs.size() / 2] = std::numeric_limits<double>::quiet_NaN();   // a missed detection is data, not an error
    }
    orcvio_object_track track() const { return orcvio_object_track{K, F, wTo.data(), shape.data(), kps.data(), wTc.data(), zs.data(), bb.data(), nullptr}; }
    orcvio_object_lm_prior prior() const { return orcvio_object_lm_prior{ms.data(), mk.data()}; }
    orcvio_object_lm_result result() { orcvio_object_lm_result r{}; r.wTo = out.data(); r.shape = out.data() + 16; r.kps = out.data() + 19; return r; }
};

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// Doubly faulty inputs: which of two simultaneous faults the validator reports.  One pair from each two refusal classes (null
// argument, config, capacity of the handle, the per-track checks) and pairs within the per-track checks.  The expected code and text
// of every row were recorded by running the same inputs through the validators of the three pack headers this header replaced.
static int double_faults() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<Case> cs;
    const int shapes[][2] = {{3, 4}, {16, 128}, {12, 47}, {5, 2}, {2, 3}};
    for (auto& s : shapes) cs.emplace_back(s[0], s[1], 1000.0 * cs.size());
    Case nan_pose(2, 3, 50.0), nan_start(16, 128, 60.0);
    nan_pose.wTc[7] = nan; nan_start.kps.back() = nan;
    struct Args {
        orcvio_object_lm_config c{1, 0, {1, 1, 1, 1}, 60, 1e-18};
        std::vector<orcvio_object_track> t;
        std::vector<orcvio_object_lm_prior> p;
        std::vector<orcvio_object_lm_result> r;
        int n = 0;
        bool no_cfg = false, no_tracks = false, no_priors = false, no_results = false;
    };
    struct Row { const char* name; int rc; const char* why; void (*change)(Args&, const Case&, const Case&); };
    const Row rows[] = {
        {"null results + bad config", ORCVIO_ERR_INVALID, "null argument", [](Args& a, const Case&, const Case&) { a.no_results = true; a.c.max_iter = 0; }},
        {"null priors + too many tracks", ORCVIO_ERR_INVALID, "null argument", [](Args& a, const Case&, const Case&) { a.no_priors = true; a.n = 65; }},
        {"null config + a track without frames", ORCVIO_ERR_INVALID, "null argument", [](Args& a, const Case&, const Case&) { a.no_cfg = true; a.t[0].n_frames = 0; }},
        {"negative count + bad config", ORCVIO_ERR_INVALID, "null argument", [](Args& a, const Case&, const Case&) { a.n = -1; a.c.ptol = -1.0; }},
        {"bad config + too many tracks", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights",
         [](Args& a, const Case&, const Case&) { a.c.max_iter = 0; a.n = 65; }},
        {"bad config + a track without keypoints", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights",
         [](Args& a, const Case&, const Case&) { a.c.ptol = -1.0; a.t[2].n_keypoints = 0; }},
        {"too many tracks + a track without frames", ORCVIO_ERR_CAPACITY, "more tracks than the handle's capacity (max_features)",
         [](Args& a, const Case&, const Case&) { a.n = 65; a.t[0].n_frames = 0; }},
        {"null bbox + non-finite start, one track", ORCVIO_ERR_INVALID, "null pointer in a track, prior or result",
         [](Args& a, const Case&, const Case& ns) { a.t[1] = ns.track(); a.p[1] = ns.prior(); a.t[1].frame_bbox = nullptr; }},
        {"null result + non-finite pose, one track", ORCVIO_ERR_INVALID, "null pointer in a track, prior or result",
         [](Args& a, const Case& np, const Case&) { a.t[4] = np.track(); a.p[4] = np.prior(); a.r[4].shape = nullptr; }},
        {"17 keypoints + no frames, one track", ORCVIO_ERR_INVALID, "a track without frames", [](Args& a, const Case&, const Case&) { a.t[2].n_keypoints = 17; a.t[2].n_frames = 0; }},
        {"17 keypoints + 129 frames, one track", ORCVIO_ERR_CAPACITY, "more than 16 keypoints", [](Args& a, const Case&, const Case&) { a.t[2].n_keypoints = 17; a.t[2].n_frames = 129; }},
        {"no keypoints + 129 frames, one track", ORCVIO_ERR_INVALID, "a track without keypoints (bbox-only tracks are the reference's lite functor: not served)",
         [](Args& a, const Case&, const Case&) { a.t[3].n_keypoints = 0; a.t[3].n_frames = 129; }},
        {"non-finite pose in track 4 + 129 frames in track 1", ORCVIO_ERR_CAPACITY, "more than 128 frames",
         [](Args& a, const Case& np, const Case&) { a.t[4] = np.track(); a.p[4] = np.prior(); a.t[1].n_frames = 129; }},
        {"non-finite start in track 1 + null prior in track 3", ORCVIO_ERR_INVALID, "non-finite number in a start value, prior, camera pose or bounding box",
         [](Args& a, const Case&, const Case& ns) { a.t[1] = ns.track(); a.p[1] = ns.prior(); a.p[3].mean_kps = nullptr; }},
    };
    int failed = 0;
    for (const Row& row : rows) {
        Args a;
        for (auto& c : cs) { a.t.push_back(c.track()); a.p.push_back(c.prior()); a.r.push_back(c.result()); }
        a.n = (int)cs.size();
        row.change(a, nan_pose, nan_start);
        const char* why = nullptr;
        size_t nd = 1;
        const int rc = obj_lm_validate(a.no_cfg ? nullptr : &a.c, a.no_tracks ? nullptr : a.t.data(), a.no_priors ? nullptr : a.p.data(), a.n,
                                       a.no_results ? nullptr : a.r.data(), 64, &why, &nd);
        if (rc != row.rc || nd != 0 || !why || std::strcmp(why, row.why) != 0) {
            std::printf("FAILED double fault '%s': %d \"%s\"\n", row.name, rc, why ? why : "(null)");
            ++failed;
        }
    }
    return failed;
}

int main() {
    orcvio_object_lm_config cfg{1, 0, {1, 1, 1, 1}, 60, 1e-18};
    std::vector<Case> cs;
    const int shapes[][2] = {{1, 1}, {16, 128}, {12, 47}, {5, 2}, {16, 1}, {1, 128}};
    for (auto& s : shapes) cs.emplace_back(s[0], s[1], 1000.0 * cs.size());
    const int n = (int)cs.size();
    std::vector<orcvio_object_track> tracks;
    std::vector<orcvio_object_lm_prior> priors;
    std::vector<orcvio_object_lm_result> results;
    for (auto& c : cs) { tracks.push_back(c.track()); priors.push_back(c.prior()); results.push_back(c.result()); }
    const char* why = nullptr;
    size_t nd = 0;
    CHECK(obj_lm_validate(&cfg, tracks.data(), priors.data(), n, results.data(), 64, &why, &nd) == ORCVIO_OK);
    size_t want = 0;
    for (auto& c : cs) want += 16 + 3 + 3 * c.K + 3 + 3 * c.K + c.F * (16 + 2 * c.K + 4);
    CHECK(nd == want);
    // pack into blocks of exactly the announced size
    std::unique_ptr<ObjLmTrack[]> recs(new ObjLmTrack[n]);
    std::unique_ptr<double[]> in(new double[nd]);
    obj_map_pack(obj_io_lm(priors.data(), results.data()), tracks.data(), n, recs.get(), in.get());
    size_t off = 0;
    for (int q = 0; q < n; ++q) {
        const Case& c = cs[q];
        CHECK(recs[q].K == c.K && recs[q].F == c.F && (size_t)recs[q].off == off);
        const double* p = in.get() + off;
        CHECK(p[0] == c.wTo[0] && p[15] == c.wTo[15] && p[16] == c.shape[0] && p[19] == c.kps[0]);
        CHECK(p[19 + 3 * c.K] == c.ms[0] && p[22 + 3 * c.K] == c.mk[0] && p[22 + 6 * c.K] == c.wTc[0]);
        CHECK(p[22 + 6 * c.K + 16 * c.F] == c.zs[0]);
        const size_t last = obj_lm_track_doubles(c.K, c.F) - 1;
        CHECK(p[last] == c.bb.back());
        off += last + 1;
    }
    CHECK(off == nd);
    // unpack from a block of exactly n x OBJ_LM_OUT
    std::unique_ptr<double[]> out(new double[(size_t)n * OBJ_LM_OUT]);
    for (size_t i = 0; i < (size_t)n * OBJ_LM_OUT; ++i) out[i] = (double)i;
    for (int q = 0; q < n; ++q) { out[(size_t)q * OBJ_LM_OUT + 69] = 7; out[(size_t)q * OBJ_LM_OUT + 70] = 8; out[(size_t)q * OBJ_LM_OUT + 71] = 1; }
    obj_lm_unpack(out.get(), tracks.data(), n, results.data());
    for (int q = 0; q < n; ++q) {
        const double* o = out.get() + (size_t)q * OBJ_LM_OUT;
        CHECK(cs[q].out[0] == o[0] && cs[q].out[18] == o[18] && cs[q].out.back() == o[19 + 3 * cs[q].K - 1]);
        CHECK(results[q].cost0 == o[67] && results[q].cost == o[68] && results[q].iterations == 7 && results[q].evaluations == 8 && results[q].status == 1);
    }
    // refusals: nothing read beyond what the refusal needs
    auto refuse = [&](int want_rc, auto&& change) {
        std::vector<orcvio_object_track> t = tracks;
        std::vector<orcvio_object_lm_prior> p = priors;
        std::vector<orcvio_object_lm_result> r = results;
        orcvio_object_lm_config c = cfg;
        change(t, p, r, c);
        size_t nd2 = 1;
        const int rc = obj_lm_validate(&c, t.data(), p.data(), n, r.data(), 64, &why, &nd2);
        return rc == want_rc && nd2 == 0 && why && why[0];
    };
    using T = std::vector<orcvio_object_track>; using P = std::vector<orcvio_object_lm_prior>; using R = std::vector<orcvio_object_lm_result>;
    using Cf = orcvio_object_lm_config;
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, P&, R&, Cf&) { t[2].n_keypoints = 0; }));
    CHECK(refuse(ORCVIO_ERR_CAPACITY, [](T& t, P&, R&, Cf&) { t[2].n_keypoints = 17; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, P&, R&, Cf&) { t[5].n_frames = 0; }));
    CHECK(refuse(ORCVIO_ERR_CAPACITY, [](T& t, P&, R&, Cf&) { t[5].n_frames = 129; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, P&, R&, Cf&) { t[1].frame_bbox = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P& p, R&, Cf&) { p[3].mean_shape = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P&, R& r, Cf&) { r[4].shape = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P&, R&, Cf& c) { c.max_iter = 0; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P&, R&, Cf& c) { c.ptol = -1.0; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P&, R&, Cf& c) { c.use_new_bbox_residual = 3; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P&, R&, Cf& c) { c.residual_weights[2] = std::numeric_limits<double>::infinity(); }));
    {   // a NaN in the last camera pose of the longest track
        Case bad(16, 128, 5.0);
        bad.wTc.back() = std::numeric_limits<double>::quiet_NaN();
        CHECK(refuse(ORCVIO_ERR_INVALID, [&](T& t, P& p, R&, Cf&) { t[1] = bad.track(); p[1] = bad.prior(); }));
    }
    size_t nd3 = 1;
    CHECK(obj_lm_validate(&cfg, tracks.data(), priors.data(), 65, results.data(), 64, &why, &nd3) == ORCVIO_ERR_CAPACITY);   // (refused before track 6 would be read)
    CHECK(obj_lm_validate(&cfg, nullptr, nullptr, 0, nullptr, 64, &why, &nd3) == ORCVIO_OK && nd3 == 0);
    CHECK(obj_lm_validate(nullptr, tracks.data(), priors.data(), n, results.data(), 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    CHECK(double_faults() == 0);
    std::printf("object lm pack ok\n");
    return 0;
}
