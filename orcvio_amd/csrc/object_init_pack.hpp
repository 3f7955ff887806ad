// object_init_pack.hpp -- host half of orcvio_msckf_object_init / orcvio_msckf_object_init_lm: validation of the caller's tracks,
// packing into the optimiser's staged input block (object_lm_pack.hpp: the same records, the same layout, so k_object_lm can run on
// what k_object_init leaves there), unpacking of the initialiser's result block.  Plain C++ (no HIP):
// tests/cpp/test_object_init_pack.cpp compiles it alone, with the sanitizers.
#pragma once
#include "object_lm_pack.hpp"

namespace orcvio_amd {

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

inline bool obj_init_config_ok(const orcvio_object_init_config* cfg) {
    return cfg->pose_form >= 0 && cfg->pose_form <= 2 && cfg->min_obs >= 0 && cfg->min_kps >= 0;
}

// The checks both entry points share.  mean_kps_per_track (object_init) or priors (object_init_lm) carries the mean keypoints; with
// priors the optimiser's inputs are checked as well (mean shape, bounding boxes, its result arrays).
inline int obj_init_validate_common(const orcvio_object_init_config* cfg, const orcvio_object_track* tracks, const double* const* mean_kps_per_track,
                                    const orcvio_object_lm_prior* priors, int n_tracks, const orcvio_object_init_result* results,
                                    const orcvio_object_lm_result* lm_results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    const bool lm = priors != nullptr || lm_results != nullptr;
    if (!cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !results || (!lm && !mean_kps_per_track) || (lm && (!priors || !lm_results))))) {
        *why = "null argument"; return ORCVIO_ERR_INVALID;
    }
    if (!obj_init_config_ok(cfg)) { *why = "config: pose_form 0..2, min_obs >= 0, min_kps >= 0"; return ORCVIO_ERR_INVALID; }
    if (n_tracks > max_tracks) { *why = "more tracks than the handle's capacity (max_features)"; return ORCVIO_ERR_CAPACITY; }
    size_t nd = 0;
    for (int q = 0; q < n_tracks; ++q) {
        const orcvio_object_track& t = tracks[q];
        const int K = t.n_keypoints, F = t.n_frames;
        if (K < 1) { *why = "a track without keypoints (the bbox-only initialiser is another function: not served)"; return ORCVIO_ERR_INVALID; }
        if (F < 1) { *why = "a track without frames"; return ORCVIO_ERR_INVALID; }
        if (K > OBJ_LM_MAXK) { *why = "more than 16 keypoints"; return ORCVIO_ERR_CAPACITY; }
        if (F > OBJ_LM_MAXF) { *why = "more than 128 frames"; return ORCVIO_ERR_CAPACITY; }
        const double* mk = lm ? priors[q].mean_kps : mean_kps_per_track[q];
        const orcvio_object_init_result& r = results[q];
        if (!t.frame_wTc || !t.frame_zs || !mk || !r.wTo || !r.kps_world || !r.kp_used || !r.kp_obs || !r.kp_cond) {
            *why = "null pointer in a track, mean keypoints or result"; return ORCVIO_ERR_INVALID;
        }
        if (lm && (!t.frame_bbox || !priors[q].mean_shape || !lm_results[q].wTo || !lm_results[q].shape || !lm_results[q].kps)) {
            *why = "null pointer in a track, prior or result of the optimiser"; return ORCVIO_ERR_INVALID;
        }
        if (!obj_lm_all_finite(t.frame_wTc, (size_t)16 * F) || !obj_lm_all_finite(mk, (size_t)3 * K)) {
            *why = "non-finite number in a camera pose or a mean keypoint"; return ORCVIO_ERR_INVALID;   // (frame_zs: NaN = not detected)
        }
        if (lm && (!obj_lm_all_finite(priors[q].mean_shape, 3) || !obj_lm_all_finite(t.frame_bbox, (size_t)4 * F))) {
            *why = "non-finite number in a mean shape or a bounding box"; return ORCVIO_ERR_INVALID;
        }
        nd += obj_lm_track_doubles(K, F);
    }
    *n_doubles = nd;
    *why = "";
    return ORCVIO_OK;
}

// ORCVIO_OK, or the refusal and its reason; *n_doubles = size of the input block.  Nothing is touched on a refusal.
inline int obj_init_validate(const orcvio_object_init_config* cfg, const orcvio_object_track* tracks, const double* const* mean_kps_per_track,
                             int n_tracks, const orcvio_object_init_result* results, int max_tracks, const char** why, size_t* n_doubles) {
    return obj_init_validate_common(cfg, tracks, mean_kps_per_track, nullptr, n_tracks, results, nullptr, max_tracks, why, n_doubles);
}

inline int obj_init_lm_validate(const orcvio_object_init_config* cfg, const orcvio_object_lm_config* lm_cfg, const orcvio_object_track* tracks,
                                const orcvio_object_lm_prior* priors, int n_tracks, const orcvio_object_init_result* results,
                                const orcvio_object_lm_result* lm_results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    if (!lm_cfg || (n_tracks > 0 && (!priors || !lm_results))) { *why = "null argument"; return ORCVIO_ERR_INVALID; }
    if (lm_cfg->max_iter < 1 || lm_cfg->max_iter > OBJ_LM_MAX_ITER || !(lm_cfg->ptol >= 0.0) || !std::isfinite(lm_cfg->ptol) ||
        lm_cfg->use_new_bbox_residual < 0 || lm_cfg->use_new_bbox_residual > 2 || !obj_lm_all_finite(lm_cfg->residual_weights, 4)) {
        *why = "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights"; return ORCVIO_ERR_INVALID;
    }
    if (n_tracks == 0) { if (!cfg || !obj_init_config_ok(cfg)) { *why = "config: pose_form 0..2, min_obs >= 0, min_kps >= 0"; return ORCVIO_ERR_INVALID; } *why = ""; return ORCVIO_OK; }
    return obj_init_validate_common(cfg, tracks, nullptr, priors, n_tracks, results, lm_results, max_tracks, why, n_doubles);
}

// recs [n_tracks], dst [n_doubles of the validation].  The layout is obj_lm_pack's; the start (wTo, shape, kps) is the kernel's to
// write and is staged as zeros, as are the mean shape and the bounding boxes of a call without the optimiser (priors == nullptr).
inline void obj_init_pack(const orcvio_object_track* tracks, const double* const* mean_kps_per_track, const orcvio_object_lm_prior* priors,
                          int n_tracks, ObjLmTrack* recs, double* dst) {
    size_t off = 0;
    for (int q = 0; q < n_tracks; ++q) {
        const orcvio_object_track& t = tracks[q];
        const int K = t.n_keypoints, F = t.n_frames;
        recs[q] = ObjLmTrack{K, F, (int)off, 0};
        double* p = dst + off;
        std::memset(p, 0, (size_t)(19 + 3 * K) * sizeof(double)); p += 19 + 3 * K;
        if (priors) std::memcpy(p, priors[q].mean_shape, 3 * sizeof(double)); else std::memset(p, 0, 3 * sizeof(double));
        p += 3;
        std::memcpy(p, priors ? priors[q].mean_kps : mean_kps_per_track[q], (size_t)3 * K * sizeof(double)); p += 3 * K;
        std::memcpy(p, t.frame_wTc, (size_t)16 * F * sizeof(double)); p += (size_t)16 * F;
        std::memcpy(p, t.frame_zs, (size_t)2 * K * F * sizeof(double)); p += (size_t)2 * K * F;
        if (priors) std::memcpy(p, t.frame_bbox, (size_t)4 * F * sizeof(double)); else std::memset(p, 0, (size_t)4 * F * sizeof(double));
        off += obj_lm_track_doubles(K, F);
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

}  // namespace orcvio_amd
