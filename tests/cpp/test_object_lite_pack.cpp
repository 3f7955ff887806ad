// Host half of the lite object mapper (orcvio_amd/csrc/object_lite_pack.hpp: validation, packing, unpacking) on its own, built with
// -fsanitize=address,undefined by tests/test_object_lite_pack.py: every buffer is a heap block of exactly the size the layout asks
// for, so a write or read past it is reported; what the calls do not read (kps, frame_zs, frame_clone, mean_kps, the result's kps)
// is NULL.  No device, no library.
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "../../orcvio_amd/csrc/object_lite_pack.hpp"

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
        obj_lite_pack(with_start ? tracks.data() : bare.data(), [&](int q) { return means[q]; }, n, with_start != 0, recs.get(), in.get());
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
    std::printf("object lite pack ok\n");
    return 0;
}
