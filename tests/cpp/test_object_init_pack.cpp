// Host half of orcvio_msckf_object_init / orcvio_msckf_object_init_lm (orcvio_amd/csrc/object_init_pack.hpp: validation, packing,
// unpacking) on its own, built with -fsanitize=address,undefined by tests/test_object_init_mirror.py: every buffer is a heap block of
// exactly the size the layout asks for, so a write or read past it is reported.  No device, no library.
#include <cassert>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "../../orcvio_amd/csrc/object_init_pack.hpp"

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
        obj_init_pack(with_lm ? tracks_lm.data() : tracks.data(), with_lm ? nullptr : mean.data(), with_lm ? priors.data() : nullptr, n, recs.get(), in.get());
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
    std::printf("object init pack ok\n");
    return 0;
}
