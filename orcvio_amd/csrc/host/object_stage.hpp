// object_stage.hpp -- the host's staging of the object update: everything between the caller's tracks (or row blocks) and the
// launches k_object_rows_batch / k_obj_front / k_obj_fused.  Pure index arithmetic on host memory -- which rows every workgroup reads
// is decided here: the scan of the tracks, the layout of the integer arena, the per-track pack, the grouping of rows by clone, the
// arrow structure of Hf.  Plain C++ (no HIP, no handle): tests/cpp/test_object_stage.cpp compiles it alone, with the sanitizers.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>
#include "../../../include/orcvio_msckf.h"
#include "object_types.hpp"

namespace orcvio_amd {

// limits of an object's state and of the structured QR of Hf (k_obj_front's keypoint blocks, k_obj_border_qr)
constexpr int OBJ_MAX_K = 34;                // keypoints per object: the state [pose 6 | shape 3 | 3 per keypoint] within 112 columns
constexpr int OBJ_ARROW_MAX_KP_ROWS = 128;   // rows of one keypoint block
constexpr int OBJ_ARROW_MAX_ROWS = 2048;     // rows of one object

struct ObjUse {   // a usable object track of the current object update
    int t, row0, rows, ncol;
    size_t off_d, off_i;   // the track's data in the doubles / its frame_clone, frame_row0 in the ints of the staging arena
    int fin, distinct;   // in-window frames; 1: every one on a clone of its own (the one-launch compression's condition)
    size_t off_nv;  // first entry of the track's per-frame keypoint counts in nvs (-1 entries: frame not in the window)
};

// what a scan of an update's tracks (or row blocks) finds
// (usable objects, their rows, the widest object state; the gate's degrees of freedom, most frames of a usable track; staged doubles / ints)
struct ObjScan { int nobj = 0, rows_tot = 0, no_max = 0, dof = 0, Fmax = 1; size_t nd = 0, ni = 0; };

// The end of a scan.  ORCVIO_OPT_REF_STACK_HF: one stacked block, projectable only if it has more rows than columns; dof = its rows - columns
template <class Use>
inline int obj_scan_close(bool ref_stack_hf, std::vector<Use>& use, ObjScan& sc) {
    if (ref_stack_hf && sc.rows_tot <= sc.no_max) { use.clear(); sc.rows_tot = 0; }
    if (ref_stack_hf) sc.dof = use.empty() ? 0 : sc.rows_tot - sc.no_max;
    sc.nobj = (int)use.size();
    return ORCVIO_OK;
}

// Pass 1 over the object tracks of an update: which are usable (more in-window rows than state columns, math_utils.hpp:292), their
// row offsets, the staged sizes, the gate's degrees of freedom; nvs: detected keypoints of every frame of every track scanned (the ONE
// pass over the observations the fused pack needs).  ORCVIO_OK, or the refusal and its text in *why.
inline int objects_tracks_scan(int N, bool ref_stack_hf, const orcvio_object_track* tracks, int n_tracks, std::vector<ObjUse>& use,
                               std::vector<signed char>& nvs, ObjScan& sc, const char** why) {
    sc = ObjScan{};
    use.clear();
    nvs.clear();
    for (int t = 0; t < n_tracks; ++t) {
        const orcvio_object_track& ob = tracks[t];
        const int K = ob.n_keypoints, F = ob.n_frames, ncol = 9 + 3 * K;
        if (K < 0 || K > OBJ_MAX_K || F < 1) { *why = "objects_local_tracks: 0..34 keypoints (object state <= 112 columns), >= 1 frame"; return ORCVIO_ERR_INVALID; }
        // (K = 0: a bbox-only track -- object state [pose 6 | shape 3], four rows per frame; kps / frame_zs are not read)
        if (!ob.wTo || !ob.shape || (K > 0 && (!ob.kps || !ob.frame_zs)) || !ob.frame_wTc || !ob.frame_bbox || !ob.frame_clone) { *why = "objects_local_tracks: null track arrays"; return ORCVIO_ERR_INVALID; }
        int rows = 0, fin = 0, distinct = 1;
        unsigned long long seen = 0ull;   // (N <= ORCVIO_MAX_CLONES = 60)
        const size_t off_nv = nvs.size();
        nvs.resize(off_nv + (size_t)F);
        signed char* nvp = nvs.data() + off_nv;
        for (int f = 0; f < F; ++f) {
            const int c = ob.frame_clone[f];
            if (c >= N) { *why = "objects_local_tracks: frame_clone out of the window"; return ORCVIO_ERR_INVALID; }
            if (c < 0) { nvp[f] = -1; continue; }
            if (seen >> c & 1ull) distinct = 0;
            seen |= 1ull << c;
            ++fin;
            int nv = 0;
            const double* zs = ob.frame_zs + (size_t)f * K * 2;
            for (int k = 0; k < K; ++k)
                if (std::isfinite(zs[2 * k]) && std::isfinite(zs[2 * k + 1])) ++nv;   // row finite test, ObjectLM.cpp:171-198
            nvp[f] = (signed char)nv;
            rows += 2 * nv + 4;
        }
        if (ref_stack_hf ? rows == 0 : rows <= ncol) continue;   // nullspace_project_inplace_svd returns false
        if (ref_stack_hf && sc.no_max > 0 && ncol != sc.no_max) { *why = "objects_local_tracks: ORCVIO_OPT_REF_STACK_HF needs equal object state sizes"; return ORCVIO_ERR_INVALID; }
        use.push_back(ObjUse{t, sc.rows_tot, rows, ncol, sc.nd, sc.ni, fin, distinct, off_nv});
        sc.nd += 16 + 3 + (size_t)3 * K + (size_t)F * (16 + 2 * K + 4);
        sc.ni += (size_t)2 * F;
        sc.rows_tot += rows;
        sc.dof += rows - ncol;
        if (ncol > sc.no_max) sc.no_max = ncol;
        if (F > sc.Fmax) sc.Fmax = F;
    }
    return obj_scan_close(ref_stack_hf, use, sc);
}

// The same over row blocks (orcvio_msckf_objects_local): use lists the usable blocks.
inline int objects_rows_scan(int N, bool ref_stack_hf, const orcvio_msckf_object_rows* objs, int n_objects, std::vector<int>& use, ObjScan& sc,
                             const char** why) {
    sc = ObjScan{};
    use.clear();
    for (int o = 0; o < n_objects; ++o) {
        const orcvio_msckf_object_rows& ob = objs[o];
        if (ob.n_rows < 0 || ob.n_obj_cols < 1 || ob.n_obj_cols > 9 + 3 * OBJ_MAX_K + 1) { *why = "objects_local: bad block shape (object state columns must be 1..112)"; return ORCVIO_ERR_INVALID; }
        if (ob.n_rows > 0 && (!ob.row_clone || !ob.Hx6 || !ob.Hf || !ob.res)) { *why = "objects_local: null block arrays"; return ORCVIO_ERR_INVALID; }
        if (ref_stack_hf ? ob.n_rows == 0 : ob.n_rows <= ob.n_obj_cols) continue;   // nullspace_project_inplace_svd returns false
        for (int r = 0; r < ob.n_rows; ++r)
            if (ob.row_clone[r] < 0 || ob.row_clone[r] >= N) { *why = "objects_local: row_clone out of range"; return ORCVIO_ERR_INVALID; }
        if (ref_stack_hf && sc.no_max > 0 && ob.n_obj_cols != sc.no_max) { *why = "objects_local: ORCVIO_OPT_REF_STACK_HF needs equal object state sizes"; return ORCVIO_ERR_INVALID; }
        use.push_back(o);
        sc.rows_tot += ob.n_rows;
        sc.dof += ob.n_rows - ob.n_obj_cols;
        if (ob.n_obj_cols > sc.no_max) sc.no_max = ob.n_obj_cols;
    }
    return obj_scan_close(ref_stack_hf, use, sc);
}

// ---- the integer arena of the general pipeline: [ni0 ints of the caller (the tracks' frame_clone, frame_row0) | ridx rows | rowptr nobj + 1 |
// arrows 4 nobj | keypoint ranges 2 (sum K + nobj) | kp_rows rows | groups 4 x <= nobj N]: offsets in ints, and the arrays behind a base
// pointer (the pinned arena's ints or their device copy)
struct ObjIntViews { int *ridx, *rowptr; ObjArrow* arrows; int *kp_range /* (begin, end) pairs */, *kp_rows; ObjGroup* groups; };
struct ObjIntLayout {
    size_t ridx, rowptr, arrow, range, kprows, groups, ni;
    ObjIntViews views(int* base) const {
        return ObjIntViews{base + ridx, base + rowptr, reinterpret_cast<ObjArrow*>(base + arrow), base + range, base + kprows,
                           reinterpret_cast<ObjGroup*>(base + groups)};
    }
    // bytes the ingest moves: nd doubles, then the ints up to the last of ng groups
    size_t ingest_bytes(size_t nd, int ng) const { return nd * 8 + (groups + (size_t)4 * ng) * 4; }
};
inline ObjIntLayout obj_int_layout(size_t rows, int nobj, size_t sumK, int N, size_t ni0) {
    const size_t rowptr = ni0 + rows, arrow = rowptr + nobj + 1, range = arrow + (size_t)4 * nobj, kprows = range + 2 * (sumK + (size_t)nobj);
    return ObjIntLayout{ni0, rowptr, arrow, range, kprows, kprows + rows, kprows + rows + (size_t)4 * nobj * N};
}

// ---- the per-track pack: the device row arrays a track's rows are evaluated into (the general pipeline); all null: the one-launch compression, which keeps its rows
struct ObjRowArrays { double *Hx6 = nullptr, *Hf = nullptr, *res = nullptr; int *row_clone = nullptr, *row_cols = nullptr; };

// Track u into the staging arena: [wTo | shape | kps | frame_wTc | frame_zs | frame_bbox] at hd + u.off_d, [frame_clone | frame_row0] at
// hi + u.off_i (rows of the frames in frame order, the reference's interleaved layout; nvp: the scan's keypoint counts), and the kernel's
// argument record *arg, whose pointers address the same offsets behind the device bases dd / di.  Returns the track's rows.
static_assert(sizeof(ObjEvalArgs) % sizeof(double) == 0, "ObjEvalArgs is copied as doubles");
constexpr size_t OBJ_ARG_DOUBLES = sizeof(ObjEvalArgs) / sizeof(double);
inline int obj_pack_track(const orcvio_object_track& ob, const ObjUse& u, const signed char* nvp, const orcvio_object_eval_flags* fl, int ldf,
                          int no_max, const ObjRowArrays& ra, double* hd, int* hi, double* dd, int* di, ObjEvalArgs* arg) {
    const int K = ob.n_keypoints, F = ob.n_frames;
    double* q = hd + u.off_d;
    auto put = [&q](const double* src, size_t n) { if (n > 0) std::memcpy(q, src, n * 8); q += n; };   // (K = 0: kps / frame_zs are not read)
    put(ob.wTo, 16); put(ob.shape, 3); put(ob.kps, (size_t)3 * K);
    put(ob.frame_wTc, (size_t)16 * F); put(ob.frame_zs, (size_t)2 * K * F); put(ob.frame_bbox, (size_t)4 * F);
    int* fc = hi + u.off_i;
    int* fr0 = fc + F;
    int rr = u.row0;
    for (int f = 0; f < F; ++f) {
        fc[f] = ob.frame_clone[f];
        fr0[f] = 0;
        if (fc[f] < 0) continue;
        fr0[f] = rr;
        rr += 2 * (int)nvp[f] + 4;
    }
    ObjEvalArgs a;
    a.wTo = dd + u.off_d; a.shape = a.wTo + 16; a.kps = a.shape + 3; a.frame_wTc = a.kps + 3 * K;
    a.frame_zs = a.frame_wTc + (size_t)16 * F; a.frame_bbox = a.frame_zs + (size_t)2 * K * F;
    a.frame_clone = di + u.off_i; a.frame_row0 = a.frame_clone + F;
    a.K = K; a.F = F; a.ncol = u.ncol; a.ldhf = ldf; a.rcol = no_max; a.row_cols = ra.row_cols;
    a.obj_left = fl->use_left_perturbation; a.new_bbox = fl->use_new_bbox_residual; a.vio_left = fl->vio_use_left_perturbation;
    a.fix_D = fl->fix_dcampose_dimupose_to_identity;
    std::memcpy(a.R_b2c, fl->R_b2c, sizeof(a.R_b2c));
    std::memcpy(a.t_c_b, fl->t_c_b, sizeof(a.t_c_b));
    a.Hx6 = ra.Hx6; a.Hf = ra.Hf; a.res = ra.res; a.row_clone = ra.row_clone;
    std::memcpy(arg, &a, sizeof(a));
    return rr - u.row0;
}

// Block ob of the rows path into the compact row arrays at row r0: hx [rows][6], hf [rows][ldf] = [Hf | 0 | res at column no_max | 0]
// (hf zeroed by the caller).  rowkp[row] = keypoint block of the row (-1: border only) while `structured` holds: the block has the shape
// [pose 6 | shape 3 | 3 per keypoint] (ObjectLM.h:117-123), every row's non-zeros behind the border in ONE block.  Returns its keypoint count.
inline int obj_pack_rows(const orcvio_msckf_object_rows& ob, int r0, size_t ldf, int no_max, double* hx, double* hf, int* rowkp, bool& structured) {
    const int nc = ob.n_obj_cols;
    const bool shape_ok = nc >= 9 && (nc - 9) % 3 == 0;
    structured = structured && shape_ok;
    for (int r = 0; r < ob.n_rows; ++r) {
        std::memcpy(hx + (size_t)(r0 + r) * 6, ob.Hx6 + (size_t)r * 6, 6 * sizeof(double));
        double* row = hf + (size_t)(r0 + r) * ldf;
        const double* src = ob.Hf + (size_t)r * nc;
        std::memcpy(row, src, nc * sizeof(double));
        row[no_max] = ob.res[r];
        if (!structured) continue;
        int blk = -1;
        for (int c = 9; c < nc; ++c)
            if (src[c] != 0.0) {
                const int b = (c - 9) / 3;
                if (blk >= 0 && b != blk) { structured = false; break; }
                blk = b;
            }
        rowkp[r0 + r] = blk;
    }
    return shape_ok ? (nc - 9) / 3 : 0;
}

// ---- rows grouped by clone: a track's frames (fc, fr0 as obj_pack_track left them, nvp the scan's counts) -> ridx [row0, row0 + rows) and one ObjGroup per clone
// with rows, clones ascending, appended at groups[*ng].  Every clone's rows one contiguous run (frames on distinct clones, or the frames
// of a clone adjacent): ridx is the identity and the groups address the rows where they lie; else the rows are grouped through ridx.
inline void obj_group_rows(const int* fc, const int* fr0, const signed char* nvp, int F, int N, int row0, int obj, int* ridx,
                           ObjGroup* groups, int* ng) {
    int first[ORCVIO_MAX_CLONES], count[ORCVIO_MAX_CLONES];
    for (int c = 0; c < N; ++c) { first[c] = -1; count[c] = 0; }
    bool contiguous = true;
    int rr = row0;
    for (int f = 0; f < F; ++f) {
        if (fc[f] < 0) continue;
        const int c = fc[f], nr = 2 * (int)nvp[f] + 4;
        if (first[c] < 0) first[c] = rr; else if (first[c] + count[c] != rr) contiguous = false;
        count[c] += nr;
        rr += nr;
    }
    if (contiguous) {
        for (int r = row0; r < rr; ++r) ridx[r] = r;
        for (int c = 0; c < N; ++c)
            if (count[c] > 0) groups[(*ng)++] = ObjGroup{first[c], first[c] + count[c], c, obj};
        return;
    }
    int pos = row0;
    for (int c = 0; c < N; ++c) {
        if (count[c] == 0) continue;
        const int g0 = pos;
        for (int f = 0; f < F; ++f)
            if (fc[f] == c)
                for (int r = 0; r < 2 * (int)nvp[f] + 4; ++r) ridx[pos++] = fr0[f] + r;
        groups[(*ng)++] = ObjGroup{g0, pos, c, obj};
    }
}
// The same for a block of the rows path, from its rows' clones: a stable counting sort.
inline void obj_group_rows(const int* row_clone, int n_rows, int N, int r0, int obj, int* ridx, ObjGroup* groups, int* ng) {
    int cnt[ORCVIO_MAX_CLONES + 1] = {0};
    for (int r = 0; r < n_rows; ++r) cnt[row_clone[r] + 1]++;
    for (int c = 0; c < N; ++c) cnt[c + 1] += cnt[c];
    for (int c = 0; c < N; ++c)
        if (cnt[c + 1] > cnt[c]) groups[(*ng)++] = ObjGroup{r0 + cnt[c], r0 + cnt[c + 1], c, obj};
    for (int r = 0; r < n_rows; ++r) ridx[r0 + cnt[row_clone[r]]++] = r0 + r;
}

// ORCVIO_OPT_REF_STACK_HF: System::processObjects stacks Hx, Hf and r of all objects VERTICALLY, Hf with its 45 columns
// shared (ros_wrapper/src/orcvio/src/System.cpp:684-702), and removeLostObjects projects the whole stack against that one Hf
// (src/orcvio.cpp:2154-2193): the objects become ONE block of rows.  Host arrays of the staged update are rewritten in
// place: one object, its rows regrouped by clone through the index list.
inline void merge_objects_ref_stack(int N, int rows_tot, int* ridx, int* rowptr, ObjGroup* groups, int* ng) {
    std::vector<int> old_ridx(ridx, ridx + rows_tot);
    std::vector<ObjGroup> old(groups, groups + *ng);
    int pos = 0, g = 0;
    for (int c = 0; c < N; ++c) {
        const int g0 = pos;
        for (const ObjGroup& q : old)
            if (q.clone == c)
                for (int k = q.r0; k < q.r1; ++k) ridx[pos++] = old_ridx[k];
        if (pos > g0) groups[g++] = ObjGroup{g0, pos, c, 0};
    }
    *ng = g;
    rowptr[0] = 0; rowptr[1] = rows_tot;
}

// ---- the arrow structure of Hf for the structured QR (k_obj_front's keypoint blocks, k_obj_border_qr): per object K + 1 ranges into kp_rows -- the rows of keypoint
// block 0 .. K-1, then the border-only rows, rows ascending within a list.
// From rowkp[row] = keypoint block of the row (-1: a border-only row), Ks[o] = keypoint blocks of object o.  Returns false if some
// object does not fit the kernels' limits.
inline bool build_arrow(const int* rowkp, const int* rowptr, const int* Ks, int nobj, ObjArrow* arrows, int* ranges, int* kp_rows, int* Kmax,
                        int* rows_max) {
    int off = 0, pos = 0;
    *Kmax = 0; *rows_max = 0;
    for (int o = 0; o < nobj; ++o) {
        const int r0 = rowptr[o], r1 = rowptr[o + 1], K = Ks[o];
        if (r1 - r0 > OBJ_ARROW_MAX_ROWS || K > OBJ_MAX_K) return false;
        int cnt[OBJ_MAX_K + 2] = {0};
        for (int r = r0; r < r1; ++r) cnt[rowkp[r] >= 0 ? rowkp[r] : K]++;
        int start[OBJ_MAX_K + 2];
        for (int k = 0; k <= K; ++k) {
            if (k < K && cnt[k] > OBJ_ARROW_MAX_KP_ROWS) return false;
            start[k] = pos;
            ranges[2 * (off + k)] = pos; ranges[2 * (off + k) + 1] = pos + cnt[k];
            pos += cnt[k];
        }
        for (int r = r0; r < r1; ++r) kp_rows[start[rowkp[r] >= 0 ? rowkp[r] : K]++] = r;
        arrows[o] = ObjArrow{r0, r1 - r0, K, off};
        off += K + 1;
        if (K > *Kmax) *Kmax = K;
        if (r1 - r0 > *rows_max) *rows_max = r1 - r0;
    }
    return true;
}

// The same, track by track, straight from the observation masks (the order of build_arrow, without a pass over the 15 000 rows of a
// config-3 update per array).  ok turns false, for good, at the first track beyond the kernels' limits.
struct ObjArrowBuild { bool ok = true; int off = 0, pos = 0, Kmax = 0, rows_max = 0; };
inline void obj_arrow_from_masks(const orcvio_object_track& ob, const int* fc, const int* fr0, int row0, int rows, std::vector<unsigned long long>& vmask,
                                 ObjArrowBuild& b, ObjArrow* arrow, int* ranges, int* kp_rows) {
    if (!b.ok) return;
    const int K = ob.n_keypoints, F = ob.n_frames;
    if (rows > OBJ_ARROW_MAX_ROWS) { b.ok = false; return; }
    int kcnt[OBJ_MAX_K + 2] = {0};   // rows of every keypoint block, [K]: border-only rows
    vmask.assign(F, 0ull);           // observed keypoints of every frame
    for (int f = 0; f < F; ++f) {
        if (fc[f] < 0) continue;
        const double* zs = ob.frame_zs + (size_t)f * K * 2;
        for (int k = 0; k < K; ++k)
            if (std::isfinite(zs[2 * k]) && std::isfinite(zs[2 * k + 1])) { vmask[f] |= 1ull << k; kcnt[k] += 2; }
        kcnt[K] += 4;
    }
    int start[OBJ_MAX_K + 2];
    for (int k = 0; k <= K; ++k) {
        if (k < K && kcnt[k] > OBJ_ARROW_MAX_KP_ROWS) { b.ok = false; return; }
        start[k] = b.pos;
        ranges[2 * (b.off + k)] = b.pos; ranges[2 * (b.off + k) + 1] = b.pos + kcnt[k];
        b.pos += kcnt[k];
    }
    for (int f = 0; f < F; ++f) {
        if (fc[f] < 0) continue;
        int rj = fr0[f];
        for (int k = 0; k < K; ++k)
            if (vmask[f] >> k & 1ull) { int& st = start[k]; kp_rows[st] = rj; kp_rows[st + 1] = rj + 1; st += 2; rj += 2; }
        int& sb = start[K];
        kp_rows[sb] = rj; kp_rows[sb + 1] = rj + 1; kp_rows[sb + 2] = rj + 2; kp_rows[sb + 3] = rj + 3;
        sb += 4;
    }
    *arrow = ObjArrow{row0, rows, K, b.off};
    b.off += K + 1;
    if (K > b.Kmax) b.Kmax = K;
    if (rows > b.rows_max) b.rows_max = rows;
}

}  // namespace orcvio_amd
