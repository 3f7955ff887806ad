// triangulate_arm.hpp -- host half of orcvio_msckf_io_triangulate: validation of the config and of the per-track modes, and the layout
// of the handle's pinned triangulation block [mode F | valid F | flags F | cost F | p_w 3F | inv_param 3F] (256-byte aligned parts, laid
// out for the handle's capacity).  Plain C++ (no HIP): tests/cpp/test_triangulate_arm.cpp compiles it alone, with the sanitizers.
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
// index of the first mode outside ORCVIO_TRI_KEEP .. ORCVIO_TRI_ALL_BUT_LAST, or -1 (mode == nullptr: every track ORCVIO_TRI_ALL)
inline int tri_first_bad_mode(const int32_t* mode, int F) {
    if (!mode) return -1;
    for (int j = 0; j < F; ++j)
        if (mode[j] < ORCVIO_TRI_KEEP || mode[j] > ORCVIO_TRI_ALL_BUT_LAST) return j;
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

}  // namespace orcvio_amd
