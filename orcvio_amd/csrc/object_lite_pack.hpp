// object_lite_pack.hpp -- host half of the lite (bbox-only) object mapper, orcvio_msckf_object_init_lite / _object_lm_lite /
// _object_init_lm_lite: validation of the caller's tracks, packing into the staged input block, unpacking of the result blocks.
// The staged block is the optimiser's at K = 0 (object_lm_pack.hpp: the same records, the same offsets), so the track records and
// the skip word are shared.  Plain C++ (no HIP): tests/cpp/test_object_lite_pack.cpp compiles it alone, with the sanitizers.
#pragma once
#include "object_lm_pack.hpp"

namespace orcvio_amd {

// per object in the staged input block (obj_lm_track_doubles(0, F) doubles): wTo 16 | shape 3 | mean_shape 3 | frame_wTc 16F | frame_bbox 4F
#define OBJ_LITE_O_MEAN 19
#define OBJ_LITE_O_WTC 22
// doubles per object in the optimiser's output block: wTo 16 | shape 3 | cost0 | cost | iterations | evaluations | status
#define OBJ_LITE_OUT 24
// doubles per object in the initialiser's output block: wTo 16 | d | status
#define OBJ_LITE_INIT_OUT 18

inline bool obj_lite_config_ok(const orcvio_object_lite_config* cfg) {
    return cfg->max_iter >= 1 && cfg->max_iter <= OBJ_LM_MAX_ITER && cfg->ptol >= 0.0 && std::isfinite(cfg->ptol) &&
           cfg->use_new_bbox_residual >= 0 && cfg->use_new_bbox_residual <= 2 && obj_lm_all_finite(cfg->residual_weights, 2);
}
inline bool obj_lite_init_config_ok(const orcvio_object_init_lite_config* cfg) {
    return cfg->pose_form >= 0 && cfg->pose_form <= 2 && obj_lm_all_finite(cfg->bbox_scale, 3);
}
#define OBJ_LITE_WHY_CFG "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights"
#define OBJ_LITE_WHY_INIT_CFG "config: pose_form 0..2, finite bbox_scale"

// The checks the three entry points share.  init: the start is the kernel's (the tracks' wTo and shape are not read; only frame 0
// is, but every frame handed over is checked: the optimiser may follow).  lm: the optimiser's result arrays are checked.
// mean(q) -> the mean shape of track q.
template <class Mean>
inline int obj_lite_validate_tracks(const orcvio_object_track* tracks, int n_tracks, Mean&& mean, const bool start_from_caller,
                                    const orcvio_object_init_lite_result* init_results, const orcvio_object_lm_result* lm_results,
                                    int max_tracks, const char** why, size_t* n_doubles) {
    if (n_tracks > max_tracks) { *why = "more tracks than the handle's capacity (max_features)"; return ORCVIO_ERR_CAPACITY; }
    size_t nd = 0;
    for (int q = 0; q < n_tracks; ++q) {
        const orcvio_object_track& t = tracks[q];
        const int F = t.n_frames;
        if (t.n_keypoints != 0) { *why = "a track with keypoints (the lite mapper serves bbox-only tracks: n_keypoints = 0)"; return ORCVIO_ERR_INVALID; }
        if (F < 1) { *why = "a track without frames"; return ORCVIO_ERR_INVALID; }
        if (F > OBJ_LM_MAXF) { *why = "more than 128 frames"; return ORCVIO_ERR_CAPACITY; }
        const double* ms = mean(q);
        if (!t.frame_wTc || !t.frame_bbox || !ms || (start_from_caller && (!t.wTo || !t.shape)) || (init_results && !init_results[q].wTo) ||
            (lm_results && (!lm_results[q].wTo || !lm_results[q].shape))) {
            *why = "null pointer in a track, mean shape or result"; return ORCVIO_ERR_INVALID;
        }
        if ((start_from_caller && (!obj_lm_all_finite(t.wTo, 16) || !obj_lm_all_finite(t.shape, 3))) || !obj_lm_all_finite(ms, 3) ||
            !obj_lm_all_finite(t.frame_wTc, (size_t)16 * F) || !obj_lm_all_finite(t.frame_bbox, (size_t)4 * F)) {
            *why = "non-finite number in a start value, mean shape, camera pose or bounding box"; return ORCVIO_ERR_INVALID;
        }
        nd += obj_lm_track_doubles(0, F);
    }
    *n_doubles = nd;
    *why = "";
    return ORCVIO_OK;
}

// ORCVIO_OK, or the refusal and its reason; *n_doubles = size of the input block.  Nothing is touched on a refusal.
inline int obj_lite_lm_validate(const orcvio_object_lite_config* cfg, const orcvio_object_track* tracks, const orcvio_object_lm_prior* priors,
                                int n_tracks, const orcvio_object_lm_result* results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    if (!cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !priors || !results))) { *why = "null argument"; return ORCVIO_ERR_INVALID; }
    if (!obj_lite_config_ok(cfg)) { *why = OBJ_LITE_WHY_CFG; return ORCVIO_ERR_INVALID; }
    return obj_lite_validate_tracks(tracks, n_tracks, [&](int q) { return priors[q].mean_shape; }, true, nullptr, results, max_tracks, why, n_doubles);
}

inline int obj_lite_init_validate(const orcvio_object_init_lite_config* cfg, const orcvio_object_track* tracks, const double* const* mean_shape_per_track,
                                  int n_tracks, const orcvio_object_init_lite_result* results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    if (!cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !mean_shape_per_track || !results))) { *why = "null argument"; return ORCVIO_ERR_INVALID; }
    if (!obj_lite_init_config_ok(cfg)) { *why = OBJ_LITE_WHY_INIT_CFG; return ORCVIO_ERR_INVALID; }
    return obj_lite_validate_tracks(tracks, n_tracks, [&](int q) { return mean_shape_per_track[q]; }, false, results, nullptr, max_tracks, why, n_doubles);
}

inline int obj_lite_init_lm_validate(const orcvio_object_init_lite_config* cfg, const orcvio_object_lite_config* lm_cfg, const orcvio_object_track* tracks,
                                     const orcvio_object_lm_prior* priors, int n_tracks, const orcvio_object_init_lite_result* results,
                                     const orcvio_object_lm_result* lm_results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    if (!cfg || !lm_cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !priors || !results || !lm_results))) { *why = "null argument"; return ORCVIO_ERR_INVALID; }
    if (!obj_lite_init_config_ok(cfg)) { *why = OBJ_LITE_WHY_INIT_CFG; return ORCVIO_ERR_INVALID; }
    if (!obj_lite_config_ok(lm_cfg)) { *why = OBJ_LITE_WHY_CFG; return ORCVIO_ERR_INVALID; }
    return obj_lite_validate_tracks(tracks, n_tracks, [&](int q) { return priors[q].mean_shape; }, false, results, lm_results, max_tracks, why, n_doubles);
}

// recs [n_tracks], dst [n_doubles of the validation].  with_start: the tracks' wTo and shape are the start (the optimiser alone);
// otherwise the start is the kernel's to write and is staged as zeros.  mean(q) as above.
template <class Mean>
inline void obj_lite_pack(const orcvio_object_track* tracks, Mean&& mean, int n_tracks, const bool with_start, ObjLmTrack* recs, double* dst) {
    size_t off = 0;
    for (int q = 0; q < n_tracks; ++q) {
        const orcvio_object_track& t = tracks[q];
        const int F = t.n_frames;
        recs[q] = ObjLmTrack{0, F, (int)off, 0};
        double* p = dst + off;
        if (with_start) { std::memcpy(p, t.wTo, 16 * sizeof(double)); std::memcpy(p + 16, t.shape, 3 * sizeof(double)); }
        else std::memset(p, 0, 19 * sizeof(double));
        std::memcpy(p + OBJ_LITE_O_MEAN, mean(q), 3 * sizeof(double));
        std::memcpy(p + OBJ_LITE_O_WTC, t.frame_wTc, (size_t)16 * F * sizeof(double));
        std::memcpy(p + OBJ_LITE_O_WTC + (size_t)16 * F, t.frame_bbox, (size_t)4 * F * sizeof(double));
        off += obj_lm_track_doubles(0, F);
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
