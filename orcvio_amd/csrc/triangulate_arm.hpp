// triangulate_arm.hpp -- host half of orcvio_msckf_io_triangulate: validation of the config and of the per-track modes, and the layout
// of the handle's pinned triangulation block [mode F | valid F | flags F | cost F | p_w 3F | inv_param 3F] (256-byte aligned parts, laid
// out for the handle's capacity).  orcvio_msckf_io_triangulate_prune has a SECOND block of that layout with the staged observation list
// of the prune features behind it (tri_prune_layout, tri_prune_arm_stage).  Plain C++ (no HIP): tests/cpp/test_triangulate_arm.cpp and
// tests/cpp/test_prune_tri_arm.cpp compile it alone, with the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "../../include/orcvio_msckf.h"

namespace orcvio_amd {

inline bool tri_config_ok(const orcvio_triangulation_config* c) {
    return c && std::isfinite(c->translation_threshold) && std::isfinite(c->huber_epsilon) && std::isfinite(c->estimation_precision) &&
           std::isfinite(c->initial_damping) && std::isfinite(c->cost_threshold) && std::isfinite(c->init_final_dist_threshold) &&
           c->outer_loop_max_iteration >= 0 && c->inner_loop_max_iteration >= 0;
}
// index of the first mode outside ORCVIO_TRI_KEEP .. top, or -1 (mode == nullptr: every track the call's default).  top: the first
// update's arming takes ORCVIO_TRI_KEEP .. ORCVIO_TRI_ALL_BUT_LAST, the prune update's ORCVIO_TRI_ALL_MOTION_BUT_LAST as well
inline int tri_first_bad_mode(const int32_t* mode, int F, int top = ORCVIO_TRI_ALL_BUT_LAST) {
    if (!mode) return -1;
    for (int j = 0; j < F; ++j)
        if (mode[j] < ORCVIO_TRI_KEEP || mode[j] > top) return j;
    return -1;
}

struct TriBlock {   // byte offsets into the pinned block of a handle of max_features tracks
    size_t mode, valid, flags, cost, p_w, inv_param, bytes;
};
inline TriBlock tri_block_layout(int max_features) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t F = max_features > 0 ? (size_t)max_features : 1;
    TriBlock b;
    size_t o = 0;
    b.mode = o; o += al(sizeof(int32_t) * F);
    b.valid = o; o += al(sizeof(int32_t) * F);
    b.flags = o; o += al(sizeof(int32_t) * F);
    b.cost = o; o += al(sizeof(double) * F);
    b.p_w = o; o += al(sizeof(double) * 3 * F);
    b.inv_param = o; o += al(sizeof(double) * 3 * F);
    b.bytes = o;
    return b;
}

// ORCVIO_OK and the modes copied into the block (when there are any), or ORCVIO_ERR_INVALID with its reason and NOTHING written
inline int tri_arm_stage(const orcvio_triangulation_config* cfg, const int32_t* mode, int F, int max_features, char* block, const char** why) {
    if (!tri_config_ok(cfg)) { *why = "a NULL or non-finite config (iteration counts must not be negative)"; return ORCVIO_ERR_INVALID; }
    if (F < 0 || F > max_features) { *why = "more tracks than the handle's capacity"; return ORCVIO_ERR_INVALID; }
    if (tri_first_bad_mode(mode, F) >= 0) { *why = "a mode outside 0 .. 2 (keep, all observations, all but the last)"; return ORCVIO_ERR_INVALID; }
    if (mode && F > 0) std::memcpy(block + tri_block_layout(max_features).mode, mode, sizeof(int32_t) * (size_t)F);
    *why = "";
    return ORCVIO_OK;
}

// ---- the prune update's arming (orcvio_msckf_io_triangulate_prune) -----------------------------------------------------------------
// The staged list [obs_ptr F+1 | obs_clone nobs | obs_z 2 nobs], packed for the F tracks and nobs observations it holds (256-byte
// aligned parts: ONE contiguous segment of `bytes` travels), at `list` behind the results of the second block; `bytes` at the handle's
// capacity is what the block reserves for it.
struct TriList {
    size_t obs_ptr, obs_clone, obs_z, bytes;   // offsets from the head of the list
};
inline TriList tri_list_layout(int F, int nobs) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t Fz = F > 0 ? (size_t)F : 0, nz = nobs > 0 ? (size_t)nobs : 0;
    TriList l;
    size_t o = 0;
    l.obs_ptr = o; o += al(sizeof(int32_t) * (Fz + 1));
    l.obs_clone = o; o += al(sizeof(int32_t) * (nz > 0 ? nz : 1));
    l.obs_z = o; o += al(sizeof(double) * 2 * (nz > 0 ? nz : 1));
    l.bytes = o;
    return l;
}
struct TriPruneBlock {
    TriBlock res;         // the results (and the modes), as the first block
    size_t list, bytes;   // the staged list behind them; the whole block
};
inline TriPruneBlock tri_prune_layout(int max_features, int max_obs) {
    TriPruneBlock b;
    b.res = tri_block_layout(max_features);
    b.list = b.res.bytes;
    b.bytes = b.list + tri_list_layout(max_features > 0 ? max_features : 1, max_obs > 0 ? max_obs : 1).bytes;
    return b;
}
// ORCVIO_OK with the modes (ORCVIO_TRI_ALL_MOTION_BUT_LAST for every track when mode == nullptr) and the list copied into the block, or
// the refusal's code with its reason and NOTHING written.  N: clones of the open window.
inline int tri_prune_arm_stage(const orcvio_triangulation_config* cfg, const orcvio_msckf_tracks* tr, const int32_t* mode, int N, int max_features,
                               int max_obs, char* block, const char** why) {
    if (!tri_config_ok(cfg)) { *why = "a NULL or non-finite config (iteration counts must not be negative)"; return ORCVIO_ERR_INVALID; }
    if (!tr || !tr->obs_ptr || tr->n_features < 0) { *why = "tri_tracks: null obs_ptr / bad count"; return ORCVIO_ERR_INVALID; }
    const int F = tr->n_features;
    if (F > max_features) { *why = "more tracks than the handle's capacity"; return ORCVIO_ERR_CAPACITY; }
    if (tr->obs_ptr[0] != 0) { *why = "tri_tracks: obs_ptr must start at zero"; return ORCVIO_ERR_INVALID; }
    for (int j = 0; j < F; ++j) {
        const int M = tr->obs_ptr[j + 1] - tr->obs_ptr[j];
        if (M < 0 || tr->obs_ptr[j + 1] < 0) { *why = "tri_tracks: obs_ptr not monotone"; return ORCVIO_ERR_INVALID; }
        if (M > ORCVIO_MAX_TRACK) { *why = "tri_tracks: track longer than ORCVIO_MAX_TRACK"; return ORCVIO_ERR_TRACK_TOO_LONG; }
    }
    const int nobs = tr->obs_ptr[F];
    if (nobs > max_obs) { *why = "more observations than the handle's capacity"; return ORCVIO_ERR_CAPACITY; }
    if (nobs > 0 && (!tr->obs_clone || !tr->obs_z)) { *why = "tri_tracks: null track arrays"; return ORCVIO_ERR_INVALID; }
    if (tri_first_bad_mode(mode, F, ORCVIO_TRI_ALL_MOTION_BUT_LAST) >= 0) { *why = "a mode outside 0 .. 3 (keep, all observations, all but the last, all with the motion check but the last)"; return ORCVIO_ERR_INVALID; }
    for (int j = 0; j < F; ++j)
        for (int o = tr->obs_ptr[j]; o < tr->obs_ptr[j + 1]; ++o) {
            if ((unsigned)tr->obs_clone[o] >= (unsigned)N) { *why = "tri_tracks: obs_clone outside the window"; return ORCVIO_ERR_INVALID; }
            if (o > tr->obs_ptr[j] && tr->obs_clone[o] <= tr->obs_clone[o - 1]) { *why = "tri_tracks: clones not ascending within a track"; return ORCVIO_ERR_INVALID; }
        }
    const TriPruneBlock b = tri_prune_layout(max_features, max_obs);
    const TriList l = tri_list_layout(F, nobs);
    int32_t* md = reinterpret_cast<int32_t*>(block + b.res.mode);
    for (int j = 0; j < F; ++j) md[j] = mode ? mode[j] : (int32_t)ORCVIO_TRI_ALL_MOTION_BUT_LAST;
    std::memcpy(block + b.list + l.obs_ptr, tr->obs_ptr, sizeof(int32_t) * ((size_t)F + 1));
    if (nobs > 0) {
        std::memcpy(block + b.list + l.obs_clone, tr->obs_clone, sizeof(int32_t) * (size_t)nobs);
        std::memcpy(block + b.list + l.obs_z, tr->obs_z, sizeof(double) * 2 * (size_t)nobs);
    }
    *why = "";
    return ORCVIO_OK;
}
// Does every observation of the prune tracks occur, by its clone, in the staged list of its track?  (the frame call, before anything is
// enqueued: the Jacobian rows use a subset of what the triangulation used)
inline bool tri_prune_covers(const char* block, int max_features, int max_obs, int F, const int32_t* p_ptr, const int32_t* p_clone) {
    const TriPruneBlock b = tri_prune_layout(max_features, max_obs);
    const int32_t* l_ptr = reinterpret_cast<const int32_t*>(block + b.list);
    const TriList l = tri_list_layout(F, l_ptr[F]);
    const int32_t* l_clone = reinterpret_cast<const int32_t*>(block + b.list + l.obs_clone);
    for (int j = 0; j < F; ++j)
        for (int o = p_ptr[j]; o < p_ptr[j + 1]; ++o) {
            bool hit = false;
            for (int q = l_ptr[j]; q < l_ptr[j + 1] && !hit; ++q) hit = l_clone[q] == p_clone[o];
            if (!hit) return false;
        }
    return true;
}

}  // namespace orcvio_amd
