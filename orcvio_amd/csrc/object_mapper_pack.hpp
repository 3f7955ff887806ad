// object_mapper_pack.hpp -- host half of the object mapper's six entry points (orcvio_msckf_object_lm / _object_init /
// _object_init_lm and their bbox-only _lite forms): validation of the caller's tracks, packing into the staged input block,
// unpacking of the result blocks.  There is ONE staged layout -- the lite block is the same layout at K = 0 -- so the track records,
// the skip word and the offsets are the same for every kernel, and an optimiser can run on what an initialiser leaves there.
// Plain C++ (no HIP): tests/cpp/test_object_{lm,init,lite}_pack.cpp compile it alone, with the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/orcvio_msckf.h"

namespace orcvio_amd {

#define OBJ_LM_MAXK 16          // keypoints per object
#define OBJ_LM_MAXF 128         // frames per track
#define OBJ_LM_MAX_ITER 100000  // bound of the in-launch loop a caller may ask for
#define OBJ_LM_OUT 72           // doubles per object in the optimiser's output block: wTo 16 | shape 3 | kps 48 | cost0 | cost | iterations | evaluations | status
// doubles per object in the initialiser's output block:
// wTo 16 | R_kabsch 9 | t_kabsch 3 | scale | sigma 3 | kps_world 48 | kp_used 16 | kp_obs 16 | kp_cond 16 | n_used | status
#define OBJ_INIT_OUT 130
#define OBJ_INIT_O_R 16
#define OBJ_INIT_O_T 25
#define OBJ_INIT_O_SCALE 28
#define OBJ_INIT_O_SIGMA 29
#define OBJ_INIT_O_KPS 32
#define OBJ_INIT_O_USED 80
#define OBJ_INIT_O_OBS 96
#define OBJ_INIT_O_COND 112
#define OBJ_INIT_O_NUSED 128
#define OBJ_INIT_O_STATUS 129
// a lite object in the staged input block (obj_lm_track_doubles(0, F) doubles): wTo 16 | shape 3 | mean_shape 3 | frame_wTc 16F | frame_bbox 4F
#define OBJ_LITE_O_MEAN 19
#define OBJ_LITE_O_WTC 22
#define OBJ_LITE_OUT 24         // doubles per object in the lite optimiser's output block: wTo 16 | shape 3 | cost0 | cost | iterations | evaluations | status
#define OBJ_LITE_INIT_OUT 18    // doubles per object in the lite initialiser's output block: wTo 16 | d | status

struct ObjLmTrack {             // one object of the launch (offset in doubles into the staged input block)
    int K, F;
    int off;                    // wTo 16 | shape 3 | kps 3K | mean_shape 3 | mean_kps 3K | frame_wTc 16F | frame_zs 2KF | frame_bbox 4F
    int pad;                    // the skip word: 0 from the host; an initialiser stores 1 where the optimiser behind it must not optimise
};

inline size_t obj_lm_track_doubles(int K, int F) { return 22 + (size_t)6 * K + (size_t)F * (20 + 2 * K); }

inline bool obj_lm_all_finite(const double* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// ---- the configs ----------------------------------------------------------------------------------------------------------------
#define OBJ_WHY_NULL "null argument"
#define OBJ_WHY_LM_CFG "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights"
#define OBJ_WHY_INIT_CFG "config: pose_form 0..2, min_obs >= 0, min_kps >= 0"
#define OBJ_WHY_INIT_LITE_CFG "config: pose_form 0..2, finite bbox_scale"

// orcvio_object_lm_config (four weights) and orcvio_object_lite_config (two)
template <class Cfg>
inline bool obj_lm_config_ok(const Cfg* cfg) {
    return cfg->max_iter >= 1 && cfg->max_iter <= OBJ_LM_MAX_ITER && cfg->ptol >= 0.0 && std::isfinite(cfg->ptol) &&
           cfg->use_new_bbox_residual >= 0 && cfg->use_new_bbox_residual <= 2 &&
           obj_lm_all_finite(cfg->residual_weights, sizeof(cfg->residual_weights) / sizeof(double));
}
inline bool obj_init_config_ok(const orcvio_object_init_config* cfg) {
    return cfg->pose_form >= 0 && cfg->pose_form <= 2 && cfg->min_obs >= 0 && cfg->min_kps >= 0;
}
inline bool obj_lite_init_config_ok(const orcvio_object_init_lite_config* cfg) {
    return cfg->pose_form >= 0 && cfg->pose_form <= 2 && obj_lm_all_finite(cfg->bbox_scale, 3);
}

// ---- what an entry point reads and writes -----------------------------------------------------------------------------------------
struct ObjMapIo {
    bool keypoints;             // tracks of 1..16 keypoints; false: the lite calls, n_keypoints = 0 and nothing per keypoint is read
    bool start;                 // the start (wTo, shape, kps) is the caller's; false: made on the device, staged as zeros
    bool bbox;                  // frame_bbox is read; false (the keypoint initialiser alone): staged as zeros
    // where the means come from: the priors, or per track the mean keypoints (keypoints) / the mean shape (lite)
    const orcvio_object_lm_prior* priors;
    const double* const* means;
    // the result arrays that must be present
    const orcvio_object_init_result* init;
    const orcvio_object_init_lite_result* init_lite;
    const orcvio_object_lm_result* lm;
    // the refusals' texts: every call words its per-track refusals its own way, and the texts are part of the API.  Only
    // orcvio_msckf_object_init_lm has two tiers (why_null_lm / why_finite_lm): it was written as object_init's checks followed by
    // "the optimiser's inputs as well", so what the optimiser reads on top of the initialiser -- bounding boxes, mean shape, its result
    // arrays -- is refused with a text of its own, after the initialiser's; the other five calls report one tier.
    const char *why_kps, *why_null, *why_finite, *why_null_lm, *why_finite_lm;

    const double* mean_kps(int q) const { return !keypoints ? nullptr : (priors ? priors[q].mean_kps : means[q]); }
    const double* mean_shape(int q) const { return priors ? priors[q].mean_shape : (keypoints ? nullptr : means[q]); }
    bool reads_mean_shape() const { return priors != nullptr || !keypoints; }
};

#define OBJ_WHY_LM_FINITE "non-finite number in a start value, prior, camera pose or bounding box"
#define OBJ_WHY_LITE_KPS "a track with keypoints (the lite mapper serves bbox-only tracks: n_keypoints = 0)"
#define OBJ_WHY_LITE_NULL "null pointer in a track, mean shape or result"
#define OBJ_WHY_LITE_FINITE "non-finite number in a start value, mean shape, camera pose or bounding box"

inline ObjMapIo obj_io_lm(const orcvio_object_lm_prior* priors, const orcvio_object_lm_result* results) {
    return ObjMapIo{true, true, true, priors, nullptr, nullptr, nullptr, results,
                    "a track without keypoints (bbox-only tracks are the reference's lite functor: not served)",
                    "null pointer in a track, prior or result", OBJ_WHY_LM_FINITE, nullptr, nullptr};
}
// mean_kps_per_track (object_init) or priors with lm_results (object_init_lm)
inline ObjMapIo obj_io_init(const double* const* mean_kps_per_track, const orcvio_object_lm_prior* priors,
                            const orcvio_object_init_result* results, const orcvio_object_lm_result* lm_results) {
    const bool lm = priors != nullptr || lm_results != nullptr;
    return ObjMapIo{true, false, lm, priors, mean_kps_per_track, results, nullptr, lm_results,
                    "a track without keypoints (the bbox-only initialiser is another function: not served)",
                    "null pointer in a track, mean keypoints or result", "non-finite number in a camera pose or a mean keypoint",
                    lm ? "null pointer in a track, prior or result of the optimiser" : nullptr,
                    lm ? "non-finite number in a mean shape or a bounding box" : nullptr};
}
// the three lite calls: the optimiser alone (priors, lm_results), the initialiser alone (mean_shape_per_track, init_results), both
inline ObjMapIo obj_io_lite(const orcvio_object_lm_prior* priors, const double* const* mean_shape_per_track,
                            const orcvio_object_init_lite_result* init_results, const orcvio_object_lm_result* lm_results) {
    return ObjMapIo{false, init_results == nullptr, true, priors, mean_shape_per_track, nullptr, init_results, lm_results,
                    OBJ_WHY_LITE_KPS, OBJ_WHY_LITE_NULL, OBJ_WHY_LITE_FINITE, nullptr, nullptr};
}

// ---- validation -----------------------------------------------------------------------------------------------------------------
// The capacity and the per-track checks of every entry point, behind its null-argument and config checks.
// ORCVIO_OK, or the refusal and its reason; *n_doubles = size of the input block.
inline int obj_map_validate_tracks(const ObjMapIo& io, const orcvio_object_track* tracks, int n_tracks, int max_tracks, const char** why,
                                   size_t* n_doubles) {
    if (n_tracks > max_tracks) { *why = "more tracks than the handle's capacity (max_features)"; return ORCVIO_ERR_CAPACITY; }
    const bool kp = io.keypoints;
    size_t nd = 0;
    for (int q = 0; q < n_tracks; ++q) {
        const orcvio_object_track& t = tracks[q];
        const int K = t.n_keypoints, F = t.n_frames;
        if (kp ? K < 1 : K != 0) { *why = io.why_kps; return ORCVIO_ERR_INVALID; }
        if (F < 1) { *why = "a track without frames"; return ORCVIO_ERR_INVALID; }
        if (K > OBJ_LM_MAXK) { *why = "more than 16 keypoints"; return ORCVIO_ERR_CAPACITY; }
        if (F > OBJ_LM_MAXF) { *why = "more than 128 frames"; return ORCVIO_ERR_CAPACITY; }
        const double *mk = io.mean_kps(q), *ms = io.mean_shape(q);
        const bool null_own = !t.frame_wTc || (kp && (!t.frame_zs || !mk)) || (io.start && (!t.wTo || !t.shape || (kp && !t.kps))) ||
                              (io.init && (!io.init[q].wTo || !io.init[q].kps_world || !io.init[q].kp_used || !io.init[q].kp_obs || !io.init[q].kp_cond)) ||
                              (io.init_lite && !io.init_lite[q].wTo);
        const bool null_lm = (io.bbox && !t.frame_bbox) || (io.reads_mean_shape() && !ms) ||
                             (io.lm && (!io.lm[q].wTo || !io.lm[q].shape || (kp && !io.lm[q].kps)));
        if (null_own || (!io.why_null_lm && null_lm)) { *why = io.why_null; return ORCVIO_ERR_INVALID; }
        if (null_lm) { *why = io.why_null_lm; return ORCVIO_ERR_INVALID; }
        const bool inf_own = !obj_lm_all_finite(t.frame_wTc, (size_t)16 * F) || (kp && !obj_lm_all_finite(mk, (size_t)3 * K)) ||   // (frame_zs: NaN = not detected)
                             (io.start && (!obj_lm_all_finite(t.wTo, 16) || !obj_lm_all_finite(t.shape, 3) || (kp && !obj_lm_all_finite(t.kps, (size_t)3 * K))));
        const bool inf_lm = (io.reads_mean_shape() && !obj_lm_all_finite(ms, 3)) || (io.bbox && !obj_lm_all_finite(t.frame_bbox, (size_t)4 * F));
        if (inf_own || (!io.why_finite_lm && inf_lm)) { *why = io.why_finite; return ORCVIO_ERR_INVALID; }
        if (inf_lm) { *why = io.why_finite_lm; return ORCVIO_ERR_INVALID; }
        nd += obj_lm_track_doubles(K, F);
    }
    *n_doubles = nd;
    *why = "";
    return ORCVIO_OK;
}

// The six entry points' validators: the null arguments, then the configs, then obj_map_validate_tracks.  Nothing is touched on a refusal.
#define OBJ_REFUSE_IF(cond, text) do { if (cond) { *why = text; return ORCVIO_ERR_INVALID; } } while (0)

inline int obj_lm_validate(const orcvio_object_lm_config* cfg, const orcvio_object_track* tracks, const orcvio_object_lm_prior* priors,
                           int n_tracks, const orcvio_object_lm_result* results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    OBJ_REFUSE_IF(!cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !priors || !results)), OBJ_WHY_NULL);
    OBJ_REFUSE_IF(!obj_lm_config_ok(cfg), OBJ_WHY_LM_CFG);
    return obj_map_validate_tracks(obj_io_lm(priors, results), tracks, n_tracks, max_tracks, why, n_doubles);
}

inline int obj_init_validate(const orcvio_object_init_config* cfg, const orcvio_object_track* tracks, const double* const* mean_kps_per_track,
                             int n_tracks, const orcvio_object_init_result* results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    OBJ_REFUSE_IF(!cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !results || !mean_kps_per_track)), OBJ_WHY_NULL);
    OBJ_REFUSE_IF(!obj_init_config_ok(cfg), OBJ_WHY_INIT_CFG);
    return obj_map_validate_tracks(obj_io_init(mean_kps_per_track, nullptr, results, nullptr), tracks, n_tracks, max_tracks, why, n_doubles);
}

// (the optimiser's config is looked at before the initialiser's, and without tracks a missing init config is a config refusal)
inline int obj_init_lm_validate(const orcvio_object_init_config* cfg, const orcvio_object_lm_config* lm_cfg, const orcvio_object_track* tracks,
                                const orcvio_object_lm_prior* priors, int n_tracks, const orcvio_object_init_result* results,
                                const orcvio_object_lm_result* lm_results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    OBJ_REFUSE_IF(!lm_cfg || (n_tracks > 0 && (!priors || !lm_results)), OBJ_WHY_NULL);
    OBJ_REFUSE_IF(!obj_lm_config_ok(lm_cfg), OBJ_WHY_LM_CFG);
    OBJ_REFUSE_IF(n_tracks == 0 && (!cfg || !obj_init_config_ok(cfg)), OBJ_WHY_INIT_CFG);
    OBJ_REFUSE_IF(!cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !results)), OBJ_WHY_NULL);
    OBJ_REFUSE_IF(!obj_init_config_ok(cfg), OBJ_WHY_INIT_CFG);
    return obj_map_validate_tracks(obj_io_init(nullptr, priors, results, lm_results), tracks, n_tracks, max_tracks, why, n_doubles);
}

inline int obj_lite_lm_validate(const orcvio_object_lite_config* cfg, const orcvio_object_track* tracks, const orcvio_object_lm_prior* priors,
                                int n_tracks, const orcvio_object_lm_result* results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    OBJ_REFUSE_IF(!cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !priors || !results)), OBJ_WHY_NULL);
    OBJ_REFUSE_IF(!obj_lm_config_ok(cfg), OBJ_WHY_LM_CFG);
    return obj_map_validate_tracks(obj_io_lite(priors, nullptr, nullptr, results), tracks, n_tracks, max_tracks, why, n_doubles);
}

inline int obj_lite_init_validate(const orcvio_object_init_lite_config* cfg, const orcvio_object_track* tracks, const double* const* mean_shape_per_track,
                                  int n_tracks, const orcvio_object_init_lite_result* results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    OBJ_REFUSE_IF(!cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !mean_shape_per_track || !results)), OBJ_WHY_NULL);
    OBJ_REFUSE_IF(!obj_lite_init_config_ok(cfg), OBJ_WHY_INIT_LITE_CFG);
    return obj_map_validate_tracks(obj_io_lite(nullptr, mean_shape_per_track, results, nullptr), tracks, n_tracks, max_tracks, why, n_doubles);
}

inline int obj_lite_init_lm_validate(const orcvio_object_init_lite_config* cfg, const orcvio_object_lite_config* lm_cfg, const orcvio_object_track* tracks,
                                     const orcvio_object_lm_prior* priors, int n_tracks, const orcvio_object_init_lite_result* results,
                                     const orcvio_object_lm_result* lm_results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    OBJ_REFUSE_IF(!cfg || !lm_cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !priors || !results || !lm_results)), OBJ_WHY_NULL);
    OBJ_REFUSE_IF(!obj_lite_init_config_ok(cfg), OBJ_WHY_INIT_LITE_CFG);
    OBJ_REFUSE_IF(!obj_lm_config_ok(lm_cfg), OBJ_WHY_LM_CFG);
    return obj_map_validate_tracks(obj_io_lite(priors, nullptr, results, lm_results), tracks, n_tracks, max_tracks, why, n_doubles);
}
#undef OBJ_REFUSE_IF

// ---- packing --------------------------------------------------------------------------------------------------------------------
// n doubles of the staged block: a copy of src, or zeros where there is none (what a kernel writes, what a call does not read)
inline void obj_map_put(double*& p, const double* src, size_t n) {
    if (n == 0) return;
    if (src) std::memcpy(p, src, n * sizeof(double)); else std::memset(p, 0, n * sizeof(double));
    p += n;
}

// recs [n_tracks], dst [n_doubles of the validation]
inline void obj_map_pack(const ObjMapIo& io, const orcvio_object_track* tracks, int n_tracks, ObjLmTrack* recs, double* dst) {
    size_t off = 0;
    for (int q = 0; q < n_tracks; ++q) {
        const orcvio_object_track& t = tracks[q];
        const int K = t.n_keypoints, F = t.n_frames;
        recs[q] = ObjLmTrack{K, F, (int)off, 0};
        double* p = dst + off;
        obj_map_put(p, io.start ? t.wTo : nullptr, 16);
        obj_map_put(p, io.start ? t.shape : nullptr, 3);
        obj_map_put(p, io.start ? t.kps : nullptr, (size_t)3 * K);
        obj_map_put(p, io.mean_shape(q), 3);
        obj_map_put(p, io.mean_kps(q), (size_t)3 * K);
        obj_map_put(p, t.frame_wTc, (size_t)16 * F);
        obj_map_put(p, t.frame_zs, (size_t)2 * K * F);
        obj_map_put(p, io.bbox ? t.frame_bbox : nullptr, (size_t)4 * F);
        off += obj_lm_track_doubles(K, F);
    }
}

// ---- unpacking ------------------------------------------------------------------------------------------------------------------
// src [n_tracks][OBJ_LM_OUT] -> the caller's result records
inline void obj_lm_unpack(const double* src, const orcvio_object_track* tracks, int n_tracks, orcvio_object_lm_result* results) {
    for (int q = 0; q < n_tracks; ++q) {
        const double* o = src + (size_t)q * OBJ_LM_OUT;
        orcvio_object_lm_result& r = results[q];
        std::memcpy(r.wTo, o, 16 * sizeof(double));
        std::memcpy(r.shape, o + 16, 3 * sizeof(double));
        std::memcpy(r.kps, o + 19, (size_t)3 * tracks[q].n_keypoints * sizeof(double));
        r.cost0 = o[67]; r.cost = o[68];
        r.iterations = (int32_t)o[69]; r.evaluations = (int32_t)o[70]; r.status = (int32_t)o[71];
    }
}

// src [n_tracks][OBJ_INIT_OUT] -> the caller's result records
inline void obj_init_unpack(const double* src, const orcvio_object_track* tracks, int n_tracks, orcvio_object_init_result* results) {
    for (int q = 0; q < n_tracks; ++q) {
        const double* o = src + (size_t)q * OBJ_INIT_OUT;
        const int K = tracks[q].n_keypoints;
        orcvio_object_init_result& r = results[q];
        std::memcpy(r.wTo, o, 16 * sizeof(double));
        std::memcpy(r.R_kabsch, o + OBJ_INIT_O_R, 9 * sizeof(double));
        std::memcpy(r.t_kabsch, o + OBJ_INIT_O_T, 3 * sizeof(double));
        r.scale = o[OBJ_INIT_O_SCALE];
        std::memcpy(r.sigma, o + OBJ_INIT_O_SIGMA, 3 * sizeof(double));
        std::memcpy(r.kps_world, o + OBJ_INIT_O_KPS, (size_t)3 * K * sizeof(double));
        for (int k = 0; k < K; ++k) { r.kp_used[k] = (int32_t)o[OBJ_INIT_O_USED + k]; r.kp_obs[k] = (int32_t)o[OBJ_INIT_O_OBS + k]; }
        std::memcpy(r.kp_cond, o + OBJ_INIT_O_COND, (size_t)K * sizeof(double));
        r.n_used = (int32_t)o[OBJ_INIT_O_NUSED]; r.status = (int32_t)o[OBJ_INIT_O_STATUS];
    }
}

// src [n_tracks][OBJ_LITE_OUT] -> the caller's result records (kps is not written: a lite track has none)
inline void obj_lite_unpack(const double* src, int n_tracks, orcvio_object_lm_result* results) {
    for (int q = 0; q < n_tracks; ++q) {
        const double* o = src + (size_t)q * OBJ_LITE_OUT;
        orcvio_object_lm_result& r = results[q];
        std::memcpy(r.wTo, o, 16 * sizeof(double));
        std::memcpy(r.shape, o + 16, 3 * sizeof(double));
        r.cost0 = o[19]; r.cost = o[20];
        r.iterations = (int32_t)o[21]; r.evaluations = (int32_t)o[22]; r.status = (int32_t)o[23];
    }
}

// src [n_tracks][OBJ_LITE_INIT_OUT] -> the caller's result records
inline void obj_lite_init_unpack(const double* src, int n_tracks, orcvio_object_init_lite_result* results) {
    for (int q = 0; q < n_tracks; ++q) {
        const double* o = src + (size_t)q * OBJ_LITE_INIT_OUT;
        std::memcpy(results[q].wTo, o, 16 * sizeof(double));
        results[q].d = o[16];
        results[q].status = (int32_t)o[17];
    }
}

}  // namespace orcvio_amd
