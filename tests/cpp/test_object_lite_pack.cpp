// Host half of the lite object mapper (orcvio_amd/csrc/object_mapper_pack.hpp: validation, packing, unpacking) on its own, built with
// -fsanitize=address,undefined by tests/test_object_lite_pack.py: every buffer is a heap block of exactly the size the layout asks
// for, so a write or read past it is reported; what the calls do not read (kps, frame_zs, frame_clone, mean_kps, the result's kps)
// is NULL.  No device, no library.
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../../orcvio_amd/csrc/object_mapper_pack.hpp"

using namespace orcvio_amd;

struct Case {
    int F;
    std::vector<double> wTo, shape, ms, wTc, bb, out, iout;
    Case(int F_, double seed) : F(F_), wTo(16), shape(3), ms(3), wTc(16 * F_), bb(4 * F_), out(19), iout(16) {
        double v = seed;
        for (auto* a : {&wTo, &shape, &ms, &wTc, &bb})
            for (double& x : *a) x = (v += 1.0);
    }
    orcvio_object_track track(bool with_start = true) const {
        return orcvio_object_track{0, F, with_start ? wTo.data() : nullptr, with_start ? shape.data() : nullptr, nullptr, wTc.data(), nullptr, bb.data(), nullptr};
    }
    orcvio_object_lm_prior prior() const { return orcvio_object_lm_prior{ms.data(), nullptr}; }
    orcvio_object_lm_result result() { orcvio_object_lm_result r{}; r.wTo = out.data(); r.shape = out.data() + 16; r.kps = nullptr; return r; }
    orcvio_object_init_lite_result iresult() { orcvio_object_init_lite_result r{}; r.wTo = iout.data(); return r; }
};

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// Doubly faulty inputs: which of two simultaneous faults the three validators report.  One pair from each two refusal classes (null
// argument, config, capacity of the handle, the per-track checks) and pairs within the per-track checks, for each entry point.  The
// expected code and text of every row were recorded by running the same inputs through the validators of the three pack headers this
// header replaced.
static int double_faults() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<Case> cs;
    for (int F : {4, 128, 47, 2, 17}) cs.emplace_back(F, 1000.0 * cs.size());
    Case nan_pose(3, 50.0), nan_start(128, 60.0);
    nan_pose.wTc[7] = nan; nan_start.shape[2] = nan;
    struct Args {
        orcvio_object_lite_config c{1, 0, {1, 1}, 0, 60, 1e-18};
        orcvio_object_init_lite_config ic{1, {1, 1, 1}};
        std::vector<orcvio_object_track> t;
        std::vector<const double*> m;
        std::vector<orcvio_object_lm_prior> p;
        std::vector<orcvio_object_init_lite_result> ir;
        std::vector<orcvio_object_lm_result> r;
        int n = 0;
        bool no_cfg = false, no_init_cfg = false, no_tracks = false, no_means = false, no_priors = false, no_init_results = false, no_results = false;
    };
    enum { LM, INIT, INIT_LM };
    struct Row { int call; const char* name; int rc; const char* why; void (*change)(Args&, const Case&, const Case&); };
    #define CH [](Args& a, const Case& np, const Case& ns)
    #define UNUSED (void)np; (void)ns;
    const Row rows[] = {
        // orcvio_msckf_object_lm_lite
        {LM, "null results + bad config", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_results = true; a.c.max_iter = 0; }},
        {LM, "null priors + too many tracks", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_priors = true; a.n = 65; }},
        {LM, "null config + a track with keypoints", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_cfg = true; a.t[0].n_keypoints = 1; }},
        {LM, "bad config + too many tracks", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights", CH { UNUSED a.c.ptol = -1.0; a.n = 65; }},
        {LM, "bad config + a track without frames", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights", CH { UNUSED a.c.residual_weights[1] = 1.0 / 0.0; a.t[2].n_frames = 0; }},
        {LM, "too many tracks + a track with keypoints", ORCVIO_ERR_CAPACITY, "more tracks than the handle's capacity (max_features)", CH { UNUSED a.n = 65; a.t[0].n_keypoints = 2; }},
        {LM, "keypoints + 129 frames, one track", ORCVIO_ERR_INVALID, "a track with keypoints (the lite mapper serves bbox-only tracks: n_keypoints = 0)", CH { UNUSED a.t[3].n_keypoints = 1; a.t[3].n_frames = 129; }},
        {LM, "null start + non-finite pose, one track", ORCVIO_ERR_INVALID, "null pointer in a track, mean shape or result", CH { UNUSED a.t[4] = np.track(); a.p[4] = np.prior(); a.t[4].shape = nullptr; }},
        {LM, "non-finite start in track 1 + null result in track 3", ORCVIO_ERR_INVALID, "non-finite number in a start value, mean shape, camera pose or bounding box", CH { UNUSED a.t[1] = ns.track(); a.p[1] = ns.prior(); a.r[3].wTo = nullptr; }},
        {LM, "non-finite pose in track 4 + 129 frames in track 1", ORCVIO_ERR_CAPACITY, "more than 128 frames", CH { UNUSED a.t[4] = np.track(); a.p[4] = np.prior(); a.t[1].n_frames = 129; }},
        // orcvio_msckf_object_init_lite
        {INIT, "null means + bad config", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_means = true; a.ic.pose_form = 3; }},
        {INIT, "null results + too many tracks", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_init_results = true; a.n = 65; }},
        {INIT, "negative count + a track without frames", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.n = -1; a.t[0].n_frames = 0; }},
        {INIT, "bad config + too many tracks", ORCVIO_ERR_INVALID, "config: pose_form 0..2, finite bbox_scale", CH { UNUSED a.ic.bbox_scale[0] = 1.0 / 0.0; a.n = 65; }},
        {INIT, "bad config + null bbox", ORCVIO_ERR_INVALID, "config: pose_form 0..2, finite bbox_scale", CH { UNUSED a.ic.pose_form = -1; a.t[2].frame_bbox = nullptr; }},
        {INIT, "too many tracks + a track without frames", ORCVIO_ERR_CAPACITY, "more tracks than the handle's capacity (max_features)", CH { UNUSED a.n = 65; a.t[0].n_frames = 0; }},
        {INIT, "null result array + non-finite pose, one track", ORCVIO_ERR_INVALID, "null pointer in a track, mean shape or result", CH { UNUSED a.t[4] = np.track(false); a.m[4] = np.ms.data(); a.ir[4].wTo = nullptr; }},
        {INIT, "non-finite start (not read) + null mean, one track", ORCVIO_ERR_INVALID, "null pointer in a track, mean shape or result", CH { UNUSED a.t[1] = ns.track(); a.m[1] = nullptr; }},
        {INIT, "no frames + keypoints, one track", ORCVIO_ERR_INVALID, "a track with keypoints (the lite mapper serves bbox-only tracks: n_keypoints = 0)", CH { UNUSED a.t[3].n_frames = 0; a.t[3].n_keypoints = 3; }},
        // orcvio_msckf_object_init_lm_lite
        {INIT_LM, "null lm config + bad init config", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_cfg = true; a.ic.pose_form = 3; }},
        {INIT_LM, "null lm results + too many tracks", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_results = true; a.n = 65; }},
        {INIT_LM, "null init results + a track with keypoints", ORCVIO_ERR_INVALID, "null argument", CH { UNUSED a.no_init_results = true; a.t[0].n_keypoints = 1; }},
        {INIT_LM, "bad init config + bad lm config", ORCVIO_ERR_INVALID, "config: pose_form 0..2, finite bbox_scale", CH { UNUSED a.ic.pose_form = 3; a.c.max_iter = 0; }},
        {INIT_LM, "no tracks + bad init config + bad lm config", ORCVIO_ERR_INVALID, "config: pose_form 0..2, finite bbox_scale", CH { UNUSED a.n = 0; a.ic.pose_form = 3; a.c.max_iter = 0; }},
        {INIT_LM, "no tracks + bad lm config", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights", CH { UNUSED a.n = 0; a.c.use_new_bbox_residual = -1; }},
        {INIT_LM, "bad lm config + too many tracks", ORCVIO_ERR_INVALID, "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights", CH { UNUSED a.c.max_iter = 0; a.n = 65; }},
        {INIT_LM, "bad init config + a track without frames", ORCVIO_ERR_INVALID, "config: pose_form 0..2, finite bbox_scale", CH { UNUSED a.ic.bbox_scale[2] = 0.0 / 0.0; a.t[1].n_frames = 0; }},
        {INIT_LM, "too many tracks + null pose", ORCVIO_ERR_CAPACITY, "more tracks than the handle's capacity (max_features)", CH { UNUSED a.n = 65; a.t[0].frame_wTc = nullptr; }},
        {INIT_LM, "null lm result array + non-finite pose, one track", ORCVIO_ERR_INVALID, "null pointer in a track, mean shape or result", CH { UNUSED a.t[4] = np.track(false); a.p[4] = np.prior(); a.r[4].shape = nullptr; }},
        {INIT_LM, "non-finite pose in track 4 + null init result in track 0", ORCVIO_ERR_INVALID, "null pointer in a track, mean shape or result", CH { UNUSED a.t[4] = np.track(false); a.p[4] = np.prior(); a.ir[0].wTo = nullptr; }},
        {INIT_LM, "non-finite pose in track 0 + 129 frames in track 2", ORCVIO_ERR_INVALID, "non-finite number in a start value, mean shape, camera pose or bounding box", CH { UNUSED a.t[0] = np.track(false); a.p[0] = np.prior(); a.t[2].n_frames = 129; }},
    };
    #undef CH
    #undef UNUSED
    int failed = 0;
    for (const Row& row : rows) {
        Args a;
        for (auto& c : cs) { a.t.push_back(c.track(row.call == LM)); a.m.push_back(c.ms.data()); a.p.push_back(c.prior()); a.ir.push_back(c.iresult()); a.r.push_back(c.result()); }
        a.n = (int)cs.size();
        row.change(a, nan_pose, nan_start);
        const char* why = nullptr;
        size_t nd = 1;
        const orcvio_object_lite_config* cfg = a.no_cfg ? nullptr : &a.c;
        const orcvio_object_init_lite_config* icfg = a.no_init_cfg ? nullptr : &a.ic;
        const orcvio_object_track* t = a.no_tracks ? nullptr : a.t.data();
        const orcvio_object_lm_prior* p = a.no_priors ? nullptr : a.p.data();
        const orcvio_object_init_lite_result* ir = a.no_init_results ? nullptr : a.ir.data();
        const orcvio_object_lm_result* r = a.no_results ? nullptr : a.r.data();
        const int rc = row.call == LM     ? obj_lite_lm_validate(cfg, t, p, a.n, r, 64, &why, &nd)
                       : row.call == INIT ? obj_lite_init_validate(icfg, t, a.no_means ? nullptr : a.m.data(), a.n, ir, 64, &why, &nd)
                                          : obj_lite_init_lm_validate(icfg, cfg, t, p, a.n, ir, r, 64, &why, &nd);
        if (rc != row.rc || nd != 0 || !why || std::strcmp(why, row.why) != 0) {
            std::printf("FAILED double fault '%s' (call %d): %d \"%s\"\n", row.name, row.call, rc, why ? why : "(null)");
            ++failed;
        }
    }
    return failed;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    orcvio_object_lite_config cfg{1, 0, {1, 1}, 0, 60, 1e-18};
    orcvio_object_init_lite_config icfg{1, {1, 1, 1}};
    std::vector<Case> cs;
    for (int F : {1, 128, 47, 2, 17, 65}) cs.emplace_back(F, 1000.0 * cs.size());
    const int n = (int)cs.size();
    std::vector<orcvio_object_track> tracks, bare;
    std::vector<orcvio_object_lm_prior> priors;
    std::vector<orcvio_object_lm_result> results;
    std::vector<orcvio_object_init_lite_result> iresults;
    std::vector<const double*> means;
    for (auto& c : cs) {
        tracks.push_back(c.track()); bare.push_back(c.track(false)); priors.push_back(c.prior()); results.push_back(c.result());
        iresults.push_back(c.iresult()); means.push_back(c.ms.data());
    }
    const char* why = nullptr;
    size_t nd = 0, want = 0;
    for (auto& c : cs) want += 22 + 20 * (size_t)c.F;
    CHECK(obj_lite_lm_validate(&cfg, tracks.data(), priors.data(), n, results.data(), 64, &why, &nd) == ORCVIO_OK && nd == want);
    // the start is the kernel's: tracks without wTo and shape pass the two calls that initialise, not the optimiser alone
    CHECK(obj_lite_init_validate(&icfg, bare.data(), means.data(), n, iresults.data(), 64, &why, &nd) == ORCVIO_OK && nd == want);
    CHECK(obj_lite_init_lm_validate(&icfg, &cfg, bare.data(), priors.data(), n, iresults.data(), results.data(), 64, &why, &nd) == ORCVIO_OK && nd == want);
    CHECK(obj_lite_lm_validate(&cfg, bare.data(), priors.data(), n, results.data(), 64, &why, &nd) == ORCVIO_ERR_INVALID && nd == 0);
    // pack into blocks of exactly the announced size, with and without the caller's start
    for (int with_start = 0; with_start < 2; ++with_start) {
        std::unique_ptr<ObjLmTrack[]> recs(new ObjLmTrack[n]);
        std::unique_ptr<double[]> in(new double[want]);
        for (size_t i = 0; i < want; ++i) in[i] = -1.0;
        const ObjMapIo io = with_start ? obj_io_lite(nullptr, means.data(), nullptr, results.data()) : obj_io_lite(nullptr, means.data(), iresults.data(), nullptr);
        obj_map_pack(io, with_start ? tracks.data() : bare.data(), n, recs.get(), in.get());
        size_t off = 0;
        for (int q = 0; q < n; ++q) {
            const Case& c = cs[q];
            CHECK(recs[q].K == 0 && recs[q].F == c.F && (size_t)recs[q].off == off && recs[q].pad == 0);
            const double* p = in.get() + off;
            if (with_start) CHECK(p[0] == c.wTo[0] && p[15] == c.wTo[15] && p[16] == c.shape[0] && p[18] == c.shape[2]);
            else for (int i = 0; i < 19; ++i) CHECK(p[i] == 0.0);
            CHECK(p[OBJ_LITE_O_MEAN] == c.ms[0] && p[OBJ_LITE_O_MEAN + 2] == c.ms[2] && p[OBJ_LITE_O_WTC] == c.wTc[0]);
            CHECK(p[OBJ_LITE_O_WTC + 16 * c.F - 1] == c.wTc.back() && p[OBJ_LITE_O_WTC + 16 * c.F] == c.bb[0]);
            const size_t last = obj_lm_track_doubles(0, c.F) - 1;
            CHECK(p[last] == c.bb.back());
            off += last + 1;
        }
        CHECK(off == want);
    }
    // unpack from blocks of exactly n x OBJ_LITE_OUT and n x OBJ_LITE_INIT_OUT
    std::unique_ptr<double[]> out(new double[(size_t)n * OBJ_LITE_OUT]);
    for (size_t i = 0; i < (size_t)n * OBJ_LITE_OUT; ++i) out[i] = (double)i;
    for (int q = 0; q < n; ++q) { double* o = out.get() + (size_t)q * OBJ_LITE_OUT; o[21] = 7; o[22] = 8; o[23] = 2; }
    obj_lite_unpack(out.get(), n, results.data());
    for (int q = 0; q < n; ++q) {
        const double* o = out.get() + (size_t)q * OBJ_LITE_OUT;
        CHECK(cs[q].out[0] == o[0] && cs[q].out[18] == o[18]);
        CHECK(results[q].cost0 == o[19] && results[q].cost == o[20] && results[q].iterations == 7 && results[q].evaluations == 8 && results[q].status == 2);
    }
    std::unique_ptr<double[]> iout(new double[(size_t)n * OBJ_LITE_INIT_OUT]);
    for (size_t i = 0; i < (size_t)n * OBJ_LITE_INIT_OUT; ++i) iout[i] = (double)i;
    for (int q = 0; q < n; ++q) iout[(size_t)q * OBJ_LITE_INIT_OUT + 17] = 4;
    obj_lite_init_unpack(iout.get(), n, iresults.data());
    for (int q = 0; q < n; ++q) {
        const double* o = iout.get() + (size_t)q * OBJ_LITE_INIT_OUT;
        CHECK(cs[q].iout[0] == o[0] && cs[q].iout[15] == o[15] && iresults[q].d == o[16] && iresults[q].status == 4);
    }
    // refusals: nothing read beyond what the refusal needs
    using T = std::vector<orcvio_object_track>; using P = std::vector<orcvio_object_lm_prior>; using R = std::vector<orcvio_object_lm_result>;
    using I = std::vector<orcvio_object_init_lite_result>; using Cf = orcvio_object_lite_config; using Ic = orcvio_object_init_lite_config;
    auto refuse = [&](int want_rc, auto&& change) {
        T t = tracks; P p = priors; R r = results; I ir = iresults; Cf c = cfg; Ic ic = icfg;
        std::vector<const double*> m = means;
        change(t, p, r, ir, c, ic, m);
        size_t a = 1, b = 1, d = 1;
        const int r1 = obj_lite_lm_validate(&c, t.data(), p.data(), n, r.data(), 64, &why, &a);
        const bool w1 = why && why[0];
        const int r2 = obj_lite_init_validate(&ic, t.data(), m.data(), n, ir.data(), 64, &why, &b);
        const bool w2 = why && why[0];
        const int r3 = obj_lite_init_lm_validate(&ic, &c, t.data(), p.data(), n, ir.data(), r.data(), 64, &why, &d);
        const bool w3 = why && why[0];
        // (a change that one of the calls does not look at leaves that call accepting)
        return (r1 == want_rc ? (a == 0 && w1) : r1 == ORCVIO_OK) && (r2 == want_rc ? (b == 0 && w2) : r2 == ORCVIO_OK) &&
               (r3 == want_rc ? (d == 0 && w3) : r3 == ORCVIO_OK) && (r1 == want_rc || r2 == want_rc) && r3 == want_rc;
    };
    Case bad(128, 5.0);
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, P&, R&, I&, Cf&, Ic&, auto&) { t[2].n_keypoints = 1; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, P&, R&, I&, Cf&, Ic&, auto&) { t[5].n_frames = 0; }));
    CHECK(refuse(ORCVIO_ERR_CAPACITY, [](T& t, P&, R&, I&, Cf&, Ic&, auto&) { t[5].n_frames = 129; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, P&, R&, I&, Cf&, Ic&, auto&) { t[1].frame_bbox = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T& t, P&, R&, I&, Cf&, Ic&, auto&) { t[1].frame_wTc = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P& p, R&, I&, Cf&, Ic&, auto& m) { p[3].mean_shape = nullptr; m[3] = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P&, R& r, I& ir, Cf&, Ic&, auto&) { r[4].shape = nullptr; ir[4].wTo = nullptr; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P&, R&, I&, Cf& c, Ic&, auto&) { c.max_iter = 0; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P&, R&, I&, Cf& c, Ic&, auto&) { c.ptol = -1.0; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P&, R&, I&, Cf& c, Ic&, auto&) { c.use_new_bbox_residual = 3; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [&](T&, P&, R&, I&, Cf& c, Ic&, auto&) { c.residual_weights[1] = nan; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [](T&, P&, R&, I&, Cf&, Ic& ic, auto&) { ic.pose_form = 3; }));
    CHECK(refuse(ORCVIO_ERR_INVALID, [&](T&, P&, R&, I&, Cf&, Ic& ic, auto&) { ic.bbox_scale[2] = nan; }));
    bad.wTc.back() = nan;      // a NaN in the last camera pose of the longest track
    CHECK(refuse(ORCVIO_ERR_INVALID, [&](T& t, P& p, R&, I&, Cf&, Ic&, auto& m) { t[1] = bad.track(); p[1] = bad.prior(); m[1] = bad.ms.data(); }));
    bad.wTc.back() = 1.0; bad.bb[0] = nan;
    CHECK(refuse(ORCVIO_ERR_INVALID, [&](T& t, P& p, R&, I&, Cf&, Ic&, auto& m) { t[1] = bad.track(); p[1] = bad.prior(); m[1] = bad.ms.data(); }));
    bad.bb[0] = 1.0; bad.ms[1] = nan;
    CHECK(refuse(ORCVIO_ERR_INVALID, [&](T& t, P& p, R&, I&, Cf&, Ic&, auto& m) { t[1] = bad.track(); p[1] = bad.prior(); m[1] = bad.ms.data(); }));
    size_t nd3 = 1;
    CHECK(obj_lite_lm_validate(&cfg, tracks.data(), priors.data(), 65, results.data(), 64, &why, &nd3) == ORCVIO_ERR_CAPACITY);   // (refused before track 6 would be read)
    CHECK(obj_lite_init_validate(&icfg, tracks.data(), means.data(), 65, iresults.data(), 64, &why, &nd3) == ORCVIO_ERR_CAPACITY);
    CHECK(obj_lite_lm_validate(&cfg, nullptr, nullptr, 0, nullptr, 64, &why, &nd3) == ORCVIO_OK && nd3 == 0);
    CHECK(obj_lite_init_lm_validate(&icfg, &cfg, nullptr, nullptr, 0, nullptr, nullptr, 64, &why, &nd3) == ORCVIO_OK && nd3 == 0);
    CHECK(obj_lite_lm_validate(nullptr, tracks.data(), priors.data(), n, results.data(), 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    CHECK(obj_lite_init_lm_validate(&icfg, nullptr, tracks.data(), priors.data(), n, iresults.data(), results.data(), 64, &why, &nd3) == ORCVIO_ERR_INVALID);
    CHECK(double_faults() == 0);
    std::printf("object lite pack ok\n");
    return 0;
}
