// object_lm_pack.hpp -- host half of orcvio_msckf_object_lm: validation of the caller's tracks, packing into the staged input block,
// unpacking of the result block.  Plain C++ (no HIP): tests/cpp/test_object_lm_pack.cpp compiles it alone, with the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/orcvio_msckf.h"

namespace orcvio_amd {

#define OBJ_LM_MAXK 16          // keypoints per object
#define OBJ_LM_MAXF 128         // frames per track
#define OBJ_LM_OUT 72           // doubles per object in the output block: wTo 16 | shape 3 | kps 48 | cost0 | cost | iterations | evaluations | status
#define OBJ_LM_MAX_ITER 100000  // bound of the in-launch loop a caller may ask for

struct ObjLmTrack {             // one object of the launch (offset in doubles into the staged input block)
    int K, F;
    int off;                    // wTo 16 | shape 3 | kps 3K | mean_shape 3 | mean_kps 3K | frame_wTc 16F | frame_zs 2KF | frame_bbox 4F
    int pad;                    // the skip word: 0 from the host; k_object_init stores 1 where k_object_lm must not optimise
};

inline size_t obj_lm_track_doubles(int K, int F) { return 22 + (size_t)6 * K + (size_t)F * (20 + 2 * K); }

inline bool obj_lm_all_finite(const double* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// ORCVIO_OK, or the refusal and its reason; *n_doubles = size of the input block.  Nothing is touched on a refusal.
inline int obj_lm_validate(const orcvio_object_lm_config* cfg, const orcvio_object_track* tracks, const orcvio_object_lm_prior* priors,
                           int n_tracks, const orcvio_object_lm_result* results, int max_tracks, const char** why, size_t* n_doubles) {
    *n_doubles = 0;
    if (!cfg || n_tracks < 0 || (n_tracks > 0 && (!tracks || !priors || !results))) { *why = "null argument"; return ORCVIO_ERR_INVALID; }
    if (cfg->max_iter < 1 || cfg->max_iter > OBJ_LM_MAX_ITER || !(cfg->ptol >= 0.0) || !std::isfinite(cfg->ptol) ||
        cfg->use_new_bbox_residual < 0 || cfg->use_new_bbox_residual > 2 || !obj_lm_all_finite(cfg->residual_weights, 4)) {
        *why = "config: max_iter 1..100000, finite ptol >= 0, use_new_bbox_residual 0..2, finite weights"; return ORCVIO_ERR_INVALID;
    }
    if (n_tracks > max_tracks) { *why = "more tracks than the handle's capacity (max_features)"; return ORCVIO_ERR_CAPACITY; }
    size_t nd = 0;
    for (int q = 0; q < n_tracks; ++q) {
        const orcvio_object_track& t = tracks[q];
        const int K = t.n_keypoints, F = t.n_frames;
        if (K < 1) { *why = "a track without keypoints (bbox-only tracks are the reference's lite functor: not served)"; return ORCVIO_ERR_INVALID; }
        if (F < 1) { *why = "a track without frames"; return ORCVIO_ERR_INVALID; }
        if (K > OBJ_LM_MAXK) { *why = "more than 16 keypoints"; return ORCVIO_ERR_CAPACITY; }
        if (F > OBJ_LM_MAXF) { *why = "more than 128 frames"; return ORCVIO_ERR_CAPACITY; }
        if (!t.wTo || !t.shape || !t.kps || !t.frame_wTc || !t.frame_zs || !t.frame_bbox || !priors[q].mean_shape || !priors[q].mean_kps ||
            !results[q].wTo || !results[q].shape || !results[q].kps) { *why = "null pointer in a track, prior or result"; return ORCVIO_ERR_INVALID; }
        if (!obj_lm_all_finite(t.wTo, 16) || !obj_lm_all_finite(t.shape, 3) || !obj_lm_all_finite(t.kps, (size_t)3 * K) ||
            !obj_lm_all_finite(priors[q].mean_shape, 3) || !obj_lm_all_finite(priors[q].mean_kps, (size_t)3 * K) ||
            !obj_lm_all_finite(t.frame_wTc, (size_t)16 * F) || !obj_lm_all_finite(t.frame_bbox, (size_t)4 * F)) {
            *why = "non-finite number in a start value, prior, camera pose or bounding box"; return ORCVIO_ERR_INVALID;   // (frame_zs: NaN = not detected)
        }
        nd += obj_lm_track_doubles(K, F);
    }
    *n_doubles = nd;
    *why = "";
    return ORCVIO_OK;
}

// recs [n_tracks], dst [n_doubles of obj_lm_validate]
inline void obj_lm_pack(const orcvio_object_track* tracks, const orcvio_object_lm_prior* priors, int n_tracks, ObjLmTrack* recs, double* dst) {
    size_t off = 0;
    for (int q = 0; q < n_tracks; ++q) {
        const orcvio_object_track& t = tracks[q];
        const int K = t.n_keypoints, F = t.n_frames;
        recs[q] = ObjLmTrack{K, F, (int)off, 0};
        double* p = dst + off;
        std::memcpy(p, t.wTo, 16 * sizeof(double)); p += 16;
        std::memcpy(p, t.shape, 3 * sizeof(double)); p += 3;
        std::memcpy(p, t.kps, (size_t)3 * K * sizeof(double)); p += 3 * K;
        std::memcpy(p, priors[q].mean_shape, 3 * sizeof(double)); p += 3;
        std::memcpy(p, priors[q].mean_kps, (size_t)3 * K * sizeof(double)); p += 3 * K;
        std::memcpy(p, t.frame_wTc, (size_t)16 * F * sizeof(double)); p += (size_t)16 * F;
        std::memcpy(p, t.frame_zs, (size_t)2 * K * F * sizeof(double)); p += (size_t)2 * K * F;
        std::memcpy(p, t.frame_bbox, (size_t)4 * F * sizeof(double)); p += (size_t)4 * F;
        off += obj_lm_track_doubles(K, F);
    }
}

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

}  // namespace orcvio_amd
