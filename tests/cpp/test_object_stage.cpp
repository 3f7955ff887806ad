// The host's staging of the object update (orcvio_amd/csrc/host/object_stage.hpp) on its own, built with -fsanitize=address,undefined by
// tests/test_object_stage.py: synthetic tracks and row blocks through the header's functions, every arena a heap block of exactly the
// size the layout asks for (a write or read past it is reported), a fake address standing in for the device arena.  The results are
// compared with a second builder (Ref, below) written from the description of the layout: it walks the frames in order, lists each
// frame's rows, groups them by clone with a stable sort and takes the arrow lists from build_arrow over a rowkp derived from the masks.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../orcvio_amd/csrc/host/object_stage.hpp"

using namespace orcvio_amd;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#define RUN(call) do { if ((call) != 0) { std::printf("  ... in %s (line %d)\n", #call, __LINE__); return 1; } } while (0)

static const double kNaN = std::numeric_limits<double>::quiet_NaN();

struct Track {
    int K, F;
    std::vector<double> wTo, shape, kps, wTc, zs, bb;
    std::vector<int> clone;
    Track(int K_, std::vector<int> cl, double seed) : K(K_), F((int)cl.size()), wTo(16), shape(3), kps(3 * K_), wTc(16 * cl.size()), zs(2 * K_ * cl.size()),
                                                     bb(4 * cl.size()), clone(std::move(cl)) {
        double v = seed;
        for (auto* a : {&wTo, &shape, &kps, &wTc, &zs, &bb})
            for (double& x : *a) x = (v += 1.0);
    }
    Track& miss(int f, int k, int coord) { zs[(size_t)(f * K + k) * 2 + coord] = kNaN; return *this; }
    bool seen(int f, int k) const { return std::isfinite(zs[(size_t)(f * K + k) * 2]) && std::isfinite(zs[(size_t)(f * K + k) * 2 + 1]); }
    orcvio_object_track c() const { return orcvio_object_track{K, F, wTo.data(), shape.data(), kps.data(), wTc.data(), zs.data(), bb.data(), clone.data()}; }
};

// ---- the reference: rows in frame order, one record per row ---------------------------------------------------------------------------
struct RefRow { int obj, clone, kp; };
struct Ref {
    std::vector<RefRow> rows;
    std::vector<int> rowptr{0}, used;                    // used: indices of the usable tracks
    std::vector<std::vector<int>> frame_row0;            // per usable track, per frame (0 outside the window)
    int dof = 0, no_max = 0, Fmax = 1;
    size_t nd = 0, ni = 0;
};
static Ref reference(const std::vector<Track>& ts, bool ref_stack) {
    Ref R;
    for (size_t t = 0; t < ts.size(); ++t) {
        const Track& T = ts[t];
        std::vector<RefRow> mine;
        std::vector<int> fr0(T.F, 0);
        for (int f = 0; f < T.F; ++f) {
            if (T.clone[f] < 0) continue;
            fr0[f] = (int)(R.rows.size() + mine.size());
            for (int k = 0; k < T.K; ++k)
                if (T.seen(f, k)) { mine.push_back({(int)R.used.size(), T.clone[f], k}); mine.push_back({(int)R.used.size(), T.clone[f], k}); }
            for (int b = 0; b < 4; ++b) mine.push_back({(int)R.used.size(), T.clone[f], -1});
        }
        const int ncol = 9 + 3 * T.K;
        if (ref_stack ? mine.empty() : (int)mine.size() <= ncol) continue;
        R.used.push_back((int)t);
        R.rows.insert(R.rows.end(), mine.begin(), mine.end());
        R.rowptr.push_back((int)R.rows.size());
        R.frame_row0.push_back(fr0);
        R.dof += (int)mine.size() - ncol;
        R.no_max = std::max(R.no_max, ncol);
        R.Fmax = std::max(R.Fmax, T.F);
        R.nd += 19 + 3 * (size_t)T.K + (size_t)T.F * (20 + 2 * T.K);
        R.ni += 2 * (size_t)T.F;
    }
    if (ref_stack) {
        if ((int)R.rows.size() <= R.no_max) { R.rows.clear(); R.used.clear(); R.rowptr.assign(1, 0); R.frame_row0.clear(); }
        R.dof = R.used.empty() ? 0 : (int)R.rows.size() - R.no_max;
    }
    return R;
}
// the groups as sequences of rows: per object (or, merged, over all rows), clones ascending, rows of a clone in their order
struct RefGroup { int clone, obj; std::vector<int> rows; };
static std::vector<RefGroup> ref_groups(const std::vector<RefRow>& rows, const std::vector<int>& rowptr, bool merged) {
    std::vector<RefGroup> out;
    const int nobj = merged ? 1 : (int)rowptr.size() - 1;
    for (int o = 0; o < nobj; ++o) {
        const int r0 = merged ? 0 : rowptr[o], r1 = merged ? (int)rows.size() : rowptr[o + 1];
        std::vector<int> idx;
        for (int r = r0; r < r1; ++r) idx.push_back(r);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return rows[a].clone < rows[b].clone; });
        for (int r : idx) {
            if (out.empty() || out.back().obj != o || out.back().clone != rows[r].clone) out.push_back({rows[r].clone, o, {}});
            out.back().rows.push_back(r);
        }
    }
    return out;
}
static int same_groups(const std::vector<RefGroup>& want, const ObjGroup* groups, int ng, const int* ridx, int rows) {
    CHECK(ng == (int)want.size());
    for (int g = 0; g < ng; ++g) {
        CHECK(groups[g].clone == want[g].clone && groups[g].obj == want[g].obj);
        CHECK(groups[g].r0 >= 0 && groups[g].r0 <= groups[g].r1 && groups[g].r1 <= rows);
        CHECK(groups[g].r1 - groups[g].r0 == (int)want[g].rows.size());
        for (int k = groups[g].r0; k < groups[g].r1; ++k) CHECK(ridx[k] == want[g].rows[k - groups[g].r0]);
    }
    return 0;
}

// ---- the header's functions, run as the general pack and the fused pack run them -------------------------------------------------------------
static double* const DD = reinterpret_cast<double*>(uintptr_t(0x700000000000ull));   // the device arena's doubles
static bool same(const double* p, const std::vector<double>& v) { return v.empty() || std::memcmp(p, v.data(), v.size() * 8) == 0; }
static size_t off_of(const void* p, const void* base) { return (size_t)(reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(base)); }

struct Staged {
    ObjScan sc;
    std::vector<ObjUse> use;
    std::vector<signed char> nvs;
    std::vector<double> hd;
    std::vector<int> hi;
    ObjIntLayout lay;
    size_t args_off = 0;
    int ng = 0;
    ObjArrowBuild ab;
};
static orcvio_object_eval_flags eval_flags() {
    orcvio_object_eval_flags fl{};
    fl.use_left_perturbation = 1; fl.use_new_bbox_residual = 2; fl.vio_use_left_perturbation = 0; fl.fix_dcampose_dimupose_to_identity = 1;
    for (int i = 0; i < 9; ++i) fl.R_b2c[i] = 0.5 + i;
    for (int i = 0; i < 3; ++i) fl.t_c_b[i] = 20.5 + i;
    return fl;
}
static const size_t ARG_DBL = OBJ_ARG_DOUBLES;

// general = false: the one-launch compression's pack (no row arrays, ints [frame_clone, frame_row0 | arrows])
static int stage(const std::vector<Track>& ts, int N, bool ref_stack, bool general, Staged& S) {
    std::vector<orcvio_object_track> ct;
    for (const Track& t : ts) ct.push_back(t.c());
    const char* why = "";
    CHECK(objects_tracks_scan(N, ref_stack, ct.data(), (int)ct.size(), S.use, S.nvs, S.sc, &why) == ORCVIO_OK);
    const orcvio_object_eval_flags fl = eval_flags();
    const int ldf = (S.sc.no_max + 1 + 15) / 16 * 16;
    size_t sumK = 0;
    for (const ObjUse& u : S.use) sumK += (size_t)ts[u.t].K;
    S.args_off = S.sc.nd;
    const size_t nd = S.sc.nd + ARG_DBL * S.use.size();
    S.lay = obj_int_layout((size_t)S.sc.rows_tot, S.sc.nobj, sumK, N, S.sc.ni);
    S.hd.assign(nd, -7.0);
    S.hi.assign(general ? S.lay.ni : S.sc.ni + 4 * S.use.size(), -7);
    int* DI = reinterpret_cast<int*>(DD + nd);
    ObjRowArrays ra;
    if (general) { ra.Hx6 = DD + 100000; ra.Hf = DD + 200000; ra.res = DD + 300000; ra.row_clone = DI + 400000; ra.row_cols = DI + 500000; }
    const ObjIntViews hv = S.lay.views(S.hi.data());
    std::vector<unsigned long long> vmask;
    S.ab.ok = !(ref_stack && S.sc.nobj > 1);
    if (general && S.sc.nobj > 0) hv.rowptr[0] = 0;
    for (size_t ui = 0; ui < S.use.size(); ++ui) {
        const ObjUse& u = S.use[ui];
        const signed char* nvp = S.nvs.data() + u.off_nv;
        const int rows = obj_pack_track(ct[u.t], u, nvp, &fl, ldf, S.sc.no_max, ra, S.hd.data(), S.hi.data(), DD, DI,
                                        reinterpret_cast<ObjEvalArgs*>(S.hd.data() + S.args_off + ARG_DBL * ui));
        CHECK(rows == u.rows);
        if (!general) continue;
        const int *fc = S.hi.data() + u.off_i, *fr0 = fc + ts[u.t].F;
        obj_group_rows(fc, fr0, nvp, ts[u.t].F, N, u.row0, (int)ui, hv.ridx, hv.groups, &S.ng);
        hv.rowptr[ui + 1] = u.row0 + rows;
        obj_arrow_from_masks(ct[u.t], fc, fr0, u.row0, rows, vmask, S.ab, hv.arrows + ui, hv.kp_range, hv.kp_rows);
    }
    if (general && ref_stack && S.sc.nobj > 1) merge_objects_ref_stack(N, S.sc.rows_tot, hv.ridx, hv.rowptr, hv.groups, &S.ng);
    return 0;
}

// one set of tracks: the scan, both packs, the grouping and the arrow lists against the reference.  arrow_fits: what the limits allow.
static int check_tracks(const char* name, const std::vector<Track>& ts, int N, bool ref_stack, bool arrow_fits, int want_nobj) {
    const Ref R = reference(ts, ref_stack);
    Staged G, Fz;
    RUN(stage(ts, N, ref_stack, true, G));
    RUN(stage(ts, N, ref_stack, false, Fz));
    const int rows = (int)R.rows.size(), nobj = (int)R.used.size();
    // 6: the scan against sums computed the slow way
    CHECK(nobj == want_nobj);
    CHECK(G.sc.nobj == nobj && G.sc.rows_tot == rows && G.sc.no_max == R.no_max && G.sc.dof == R.dof);
    if (nobj > 0) CHECK(G.sc.Fmax == R.Fmax && G.sc.nd == R.nd && G.sc.ni == R.ni);
    const ObjIntViews hv = G.lay.views(G.hi.data());
    const int* DI = reinterpret_cast<const int*>(DD + G.hd.size());
    for (int ui = 0; ui < nobj; ++ui) {
        const ObjUse& u = G.use[ui];
        const Track& T = ts[u.t];
        CHECK(u.t == R.used[ui] && u.row0 == R.rowptr[ui] && u.rows == R.rowptr[ui + 1] - R.rowptr[ui] && u.ncol == 9 + 3 * T.K);
        // 1: frame_clone, frame_row0
        const int *fc = G.hi.data() + u.off_i, *fr0 = fc + T.F;
        for (int f = 0; f < T.F; ++f) CHECK(fc[f] == T.clone[f] && fr0[f] == R.frame_row0[ui][f]);
        // 2: the argument record, rebased to offsets, addresses exactly the bytes copied from the track
        ObjEvalArgs a;
        std::memcpy(&a, G.hd.data() + G.args_off + ARG_DBL * ui, sizeof(a));
        const double* q = G.hd.data() + u.off_d;
        CHECK(off_of(a.wTo, DD) == u.off_d * 8 && same(q, T.wTo));
        CHECK(a.shape == a.wTo + 16 && same(q + 16, T.shape));
        CHECK(a.kps == a.wTo + 19 && same(q + 19, T.kps));
        CHECK(a.frame_wTc == a.wTo + 19 + 3 * T.K && same(q + 19 + 3 * T.K, T.wTc));
        CHECK(a.frame_zs == a.frame_wTc + 16 * T.F && same(q + 19 + 3 * T.K + 16 * T.F, T.zs));
        CHECK(a.frame_bbox == a.frame_zs + 2 * T.K * T.F && same(q + 19 + 3 * T.K + (16 + 2 * T.K) * T.F, T.bb));
        CHECK(off_of(a.frame_bbox + 4 * T.F, DD) <= G.sc.nd * 8);
        CHECK(off_of(a.frame_clone, DI) == u.off_i * 4 && a.frame_row0 == a.frame_clone + T.F && u.off_i + 2 * (size_t)T.F <= G.sc.ni);
        const orcvio_object_eval_flags fl = eval_flags();
        CHECK(a.K == T.K && a.F == T.F && a.ncol == u.ncol && a.rcol == G.sc.no_max && a.ldhf >= G.sc.no_max + 1 && a.ldhf % 16 == 0);
        CHECK(a.obj_left == 1 && a.new_bbox == 2 && a.vio_left == 0 && a.fix_D == 1 && std::memcmp(a.R_b2c, fl.R_b2c, 72) == 0 && std::memcmp(a.t_c_b, fl.t_c_b, 24) == 0);
        CHECK(a.Hx6 == DD + 100000 && a.Hf == DD + 200000 && a.res == DD + 300000 && a.row_clone == DI + 400000 && a.row_cols == DI + 500000);
        // 5: the fused pack: the same track data, frame_clone and frame_row0, no row arrays, its arrow record
        const ObjUse& uf = Fz.use[ui];
        CHECK(uf.off_d == u.off_d && uf.off_i == u.off_i && uf.row0 == u.row0);
        CHECK(std::memcmp(Fz.hd.data() + uf.off_d, q, (19 + 3 * (size_t)T.K + (size_t)T.F * (20 + 2 * T.K)) * 8) == 0);
        CHECK(std::memcmp(Fz.hi.data() + uf.off_i, fc, 2 * (size_t)T.F * 4) == 0);
        ObjEvalArgs af;
        std::memcpy(&af, Fz.hd.data() + Fz.args_off + ARG_DBL * ui, sizeof(af));
        CHECK(!af.Hx6 && !af.Hf && !af.res && !af.row_clone && !af.row_cols && af.wTo == a.wTo && af.frame_bbox == a.frame_bbox && af.K == a.K && af.rcol == a.rcol && af.ldhf == a.ldhf);
    }
    if (nobj == 0) { std::printf("  %-28s nothing usable\n", name); return 0; }
    // 1, 3: rowptr, the groups' row sequences, every index inside the layout's extents (the arenas are heap blocks of exactly the layout's size)
    const bool merged = ref_stack && nobj > 1;
    CHECK(hv.rowptr[0] == 0);
    if (merged) CHECK(hv.rowptr[1] == rows);
    else for (int o = 0; o < nobj; ++o) CHECK(hv.rowptr[o + 1] == R.rowptr[o + 1]);
    for (int r = 0; r < rows; ++r) CHECK(hv.ridx[r] >= 0 && hv.ridx[r] < rows);
    CHECK(G.ng <= nobj * N);
    RUN(same_groups(ref_groups(R.rows, R.rowptr, merged), hv.groups, G.ng, hv.ridx, rows));
    // 1, 4: the arrow lists from the masks against build_arrow over the reference's rowkp
    std::vector<int> rowkp, Ks;
    for (const RefRow& r : R.rows) rowkp.push_back(r.kp);
    size_t sumK = 0;
    for (int t : R.used) { Ks.push_back(ts[t].K); sumK += ts[t].K; }
    std::vector<ObjArrow> arrows(nobj);
    std::vector<int> ranges(2 * (sumK + nobj), -1), kp_rows(rows, -1);
    int Kmax = 0, rows_max = 0;
    const bool fits = build_arrow(rowkp.data(), R.rowptr.data(), Ks.data(), nobj, arrows.data(), ranges.data(), kp_rows.data(), &Kmax, &rows_max);
    CHECK(fits == arrow_fits);
    if (merged) { std::printf("  %-28s %d objects merged, %d rows, %d groups\n", name, nobj, rows, G.ng); return 0; }
    CHECK(G.ab.ok == arrow_fits);
    if (arrow_fits) {
        CHECK(G.ab.Kmax == Kmax && G.ab.rows_max == rows_max);
        CHECK(std::memcmp(hv.arrows, arrows.data(), sizeof(ObjArrow) * nobj) == 0);
        CHECK(std::memcmp(hv.kp_range, ranges.data(), ranges.size() * 4) == 0 && std::memcmp(hv.kp_rows, kp_rows.data(), (size_t)rows * 4) == 0);
        for (int r = 0; r < rows; ++r) CHECK(hv.kp_rows[r] >= 0 && hv.kp_rows[r] < rows);
        for (size_t i = 0; i < ranges.size(); ++i) CHECK(hv.kp_range[i] >= 0 && hv.kp_range[i] <= rows);
    }
    std::printf("  %-28s %d objects, %d rows, %d groups, arrow %s\n", name, nobj, rows, G.ng, arrow_fits ? "yes" : "refused");
    return 0;
}

// ---- the rows path: blocks made from tracks' reference rows ------------------------------------------------------------------------------------
struct Block { int n_rows, nc; std::vector<int> clone; std::vector<double> hx, hf, res; std::vector<int> kp;
               orcvio_msckf_object_rows c() const { return orcvio_msckf_object_rows{n_rows, nc, clone.data(), hx.data(), hf.data(), res.data()}; } };
static Block block_of(const Track& T, double seed) {
    Block B{0, 9 + 3 * T.K, {}, {}, {}, {}, {}};
    double v = seed;
    auto row = [&](int clone, int kp) {
        B.clone.push_back(clone); B.kp.push_back(kp); B.res.push_back(v += 1.0);
        for (int i = 0; i < 6; ++i) B.hx.push_back(v += 1.0);
        for (int c = 0; c < B.nc; ++c) B.hf.push_back(c < 9 || (kp >= 0 && (c - 9) / 3 == kp) ? (v += 1.0) : 0.0);
        ++B.n_rows;
    };
    for (int f = 0; f < T.F; ++f) {
        if (T.clone[f] < 0) continue;
        for (int k = 0; k < T.K; ++k) if (T.seen(f, k)) { row(T.clone[f], k); row(T.clone[f], k); }
        for (int b = 0; b < 4; ++b) row(T.clone[f], -1);
    }
    return B;
}
static int check_blocks(const char* name, const std::vector<Block>& bs, int N, bool want_structured) {
    std::vector<orcvio_msckf_object_rows> cb;
    for (const Block& b : bs) cb.push_back(b.c());
    std::vector<int> use;
    ObjScan sc;
    const char* why = "";
    CHECK(objects_rows_scan(N, false, cb.data(), (int)cb.size(), use, sc, &why) == ORCVIO_OK);
    std::vector<RefRow> rows;
    std::vector<int> rowptr{0};
    int dof = 0, no_max = 0;
    size_t sumK = 0;
    for (size_t o = 0; o < bs.size(); ++o) {
        if (bs[o].n_rows <= bs[o].nc) continue;
        for (int r = 0; r < bs[o].n_rows; ++r) rows.push_back({(int)rowptr.size() - 1, bs[o].clone[r], bs[o].kp[r]});
        rowptr.push_back((int)rows.size());
        dof += bs[o].n_rows - bs[o].nc; no_max = std::max(no_max, bs[o].nc);
        sumK += (size_t)std::max((bs[o].nc - 9) / 3, 0);
    }
    CHECK(sc.nobj == (int)rowptr.size() - 1 && sc.rows_tot == (int)rows.size() && sc.dof == dof && sc.no_max == no_max);
    const size_t nrows = rows.size(), ldf = (size_t)(no_max + 1 + 15) / 16 * 16;
    const ObjIntLayout lay = obj_int_layout(nrows, sc.nobj, sumK, N, 0);
    std::vector<double> hx(nrows * 6, -7.0), hf(nrows * ldf, 0.0);
    std::vector<int> hi(lay.ni, -7), rowkp(nrows, -1), Ks(sc.nobj, 0);
    const ObjIntViews hv = lay.views(hi.data());
    bool structured = true;
    int r0 = 0, ng = 0;
    hv.rowptr[0] = 0;
    for (size_t ui = 0; ui < use.size(); ++ui) {
        const orcvio_msckf_object_rows& ob = cb[use[ui]];
        Ks[ui] = obj_pack_rows(ob, r0, ldf, no_max, hx.data(), hf.data(), rowkp.data(), structured);
        obj_group_rows(ob.row_clone, ob.n_rows, N, r0, (int)ui, hv.ridx, hv.groups, &ng);
        for (int r = 0; r < ob.n_rows; ++r) {
            CHECK(std::memcmp(&hx[(size_t)(r0 + r) * 6], ob.Hx6 + (size_t)r * 6, 48) == 0 && hf[(size_t)(r0 + r) * ldf + no_max] == ob.res[r]);
            CHECK(std::memcmp(&hf[(size_t)(r0 + r) * ldf], ob.Hf + (size_t)r * ob.n_obj_cols, (size_t)ob.n_obj_cols * 8) == 0);
        }
        r0 += ob.n_rows;
        hv.rowptr[ui + 1] = r0;
    }
    for (size_t r = 0; r < nrows; ++r) CHECK(hv.ridx[r] >= 0 && hv.ridx[r] < (int)nrows);
    RUN(same_groups(ref_groups(rows, rowptr, false), hv.groups, ng, hv.ridx, (int)nrows));
    CHECK(structured == want_structured);
    if (structured) {   // 4: rowkp as found from the non-zeros is the masks' rowkp, so build_arrow gives what the mask builder gives (check_tracks)
        for (size_t r = 0; r < nrows; ++r) CHECK(rowkp[r] == rows[r].kp);
        for (int o = 0; o < sc.nobj; ++o) CHECK(Ks[o] == (bs[use[o]].nc - 9) / 3);
        int Kmax = 0, rows_max = 0;
        CHECK(build_arrow(rowkp.data(), hv.rowptr, Ks.data(), sc.nobj, hv.arrows, hv.kp_range, hv.kp_rows, &Kmax, &rows_max));
        for (size_t r = 0; r < nrows; ++r) CHECK(hv.kp_rows[r] >= 0 && hv.kp_rows[r] < (int)nrows);
    }
    std::printf("  %-28s %d blocks, %zu rows, %d groups, %s\n", name, sc.nobj, nrows, ng, structured ? "structured" : "not structured");
    return 0;
}

// ---- 7: the refusals ----------------------------------------------------------------------------------------------------------------------------------
static int refusals() {
    std::vector<ObjUse> use;
    std::vector<signed char> nvs;
    ObjScan sc;
    auto scan = [&](const orcvio_object_track& t, int N, bool ref_stack, const orcvio_object_track* second, const char* text) {
        std::vector<orcvio_object_track> ts{t};
        if (second) ts.push_back(*second);
        const char* why = "";
        const int rc = objects_tracks_scan(N, ref_stack, ts.data(), (int)ts.size(), use, nvs, sc, &why);
        return rc == ORCVIO_ERR_INVALID && std::string(why) == text;
    };
    const char* shape = "objects_local_tracks: 0..34 keypoints (object state <= 112 columns), >= 1 frame";
    const char* nul = "objects_local_tracks: null track arrays";
    Track good(3, {0, 1, 2, 3}, 1.0), wide(4, {0, 1, 2, 3}, 500.0);
    orcvio_object_track t = good.c();
    t.n_keypoints = -1; CHECK(scan(t, 4, false, nullptr, shape));
    t.n_keypoints = 35; CHECK(scan(t, 4, false, nullptr, shape));
    t = good.c(); t.n_frames = 0; CHECK(scan(t, 4, false, nullptr, shape));
    t = good.c(); t.frame_bbox = nullptr; CHECK(scan(t, 4, false, nullptr, nul));
    t = good.c(); t.frame_zs = nullptr; CHECK(scan(t, 4, false, nullptr, nul));
    t = good.c(); CHECK(scan(t, 3, false, nullptr, "objects_local_tracks: frame_clone out of the window"));
    const orcvio_object_track w = wide.c();
    CHECK(scan(t, 4, true, &w, "objects_local_tracks: ORCVIO_OPT_REF_STACK_HF needs equal object state sizes"));
    // the rows path
    Block b = block_of(good, 9000.0);
    std::vector<int> used;
    auto rscan = [&](const orcvio_msckf_object_rows& r, const char* text) {
        const char* why = "";
        return objects_rows_scan(4, false, &r, 1, used, sc, &why) == ORCVIO_ERR_INVALID && std::string(why) == text;
    };
    const char* bad = "objects_local: bad block shape (object state columns must be 1..112)";
    orcvio_msckf_object_rows r = b.c();
    r.n_obj_cols = 0; CHECK(rscan(r, bad));
    r.n_obj_cols = 113; CHECK(rscan(r, bad));
    r = b.c(); r.res = nullptr; CHECK(rscan(r, "objects_local: null block arrays"));
    b.clone[5] = 4; r = b.c(); CHECK(rscan(r, "objects_local: row_clone out of range"));
    b.clone[5] = -1; r = b.c(); CHECK(rscan(r, "objects_local: row_clone out of range"));
    return 0;
}

static std::vector<int> iota_clones(int F, int N) { std::vector<int> c(F); for (int f = 0; f < F; ++f) c[f] = f % N; return c; }

int main() {
    // K in {0, 1, 3} x F in {1, 3, 5}: every pair as one update of nine tracks (F = 1 tracks of K > 0 are skipped: 2K + 4 <= 9 + 3K), and each alone
    {
        std::vector<Track> all;
        for (int K : {0, 1, 3})
            for (int F : {1, 3, 5}) {
                all.emplace_back(K, iota_clones(F, 6), 100.0 * all.size());
                const bool usable = F * (2 * K + 4) > 9 + 3 * K;
                RUN(check_tracks("K,F alone", {all.back()}, 6, false, true, usable ? 1 : 0));
            }
        RUN(check_tracks("K x F together", all, 6, false, true, 6));
    }
    RUN(check_tracks("outside first/last/middle", {Track(3, {-1, 0, -1, 2, 3, -1}, 1.0), Track(1, {1, -1, 2, 3}, 50.0)}, 4, false, true, 2));
    RUN(check_tracks("a NaN coordinate", {Track(3, {0, 1, 2, 3}, 1.0).miss(1, 2, 1).miss(2, 0, 0)}, 4, false, true, 1));
    RUN(check_tracks("clones descending", {Track(3, {3, 2, 1, 0}, 1.0), Track(1, {5, 3, 2, 0}, 70.0)}, 6, false, true, 2));
    RUN(check_tracks("two frames on one clone", {Track(3, {0, 2, 0, 1}, 1.0).miss(2, 1, 0), Track(3, {1, 1, 2, 3}, 90.0)}, 4, false, true, 2));
    RUN(check_tracks("a skipped track", {Track(3, {0, -1, -1}, 1.0), Track(3, {0, 1, 2}, 40.0)}, 4, false, true, 1));
    RUN(check_tracks("every track skipped", {Track(3, {0, -1}, 1.0), Track(1, {2}, 40.0)}, 4, false, true, 0));
    RUN(check_tracks("ref stack: two merged", {Track(3, {0, 1, 2, 3}, 1.0), Track(3, {3, 1, 0}, 300.0).miss(0, 0, 0)}, 4, true, true, 2));
    RUN(check_tracks("ref stack: rows <= columns", {Track(3, {0}, 1.0), Track(3, {-1, 2}, 300.0).miss(1, 0, 0)}, 4, true, true, 0));
    RUN(check_tracks("K = 17", {Track(17, {0, 1, 2, 3}, 1.0).miss(3, 16, 0)}, 4, false, true, 1));
    RUN(check_tracks("K = 34", {Track(34, {0, 1, 2}, 1.0), Track(0, {0, 1, 2}, 5000.0)}, 4, false, true, 2));
    RUN(check_tracks("65 frames of one keypoint", {Track(1, iota_clones(65, 60), 1.0)}, 60, false, false, 1));
    RUN(check_tracks("an object of 2160 rows", {Track(34, iota_clones(30, 60), 1.0)}, 60, false, false, 1));
    // the rows path
    {
        Track a(3, {2, 0, 1, 0}, 1.0), b(1, {3, 1, 0}, 700.0);
        a.miss(1, 1, 0);
        RUN(check_blocks("blocks of two tracks", {block_of(a, 1.0), block_of(b, 2000.0)}, 4, true));
        Block two = block_of(a, 1.0);
        two.hf[(size_t)0 * two.nc + 9 + 3 * 2] = 1.0;   // row 0 (keypoint block 0) gets a non-zero in keypoint block 2
        RUN(check_blocks("a row in two keypoint blocks", {two, block_of(b, 2000.0)}, 4, false));
        Block ten{14, 10, {}, std::vector<double>(14 * 6, 1.5), std::vector<double>(14 * 10, 2.5), std::vector<double>(14, 0.5), std::vector<int>(14, -1)};
        for (int r = 0; r < 14; ++r) ten.clone.push_back((r * 7) % 4);
        RUN(check_blocks("n_obj_cols = 10", {ten}, 4, false));
    }
    RUN(refusals());
    std::printf("object stage ok\n");
    return 0;
}
