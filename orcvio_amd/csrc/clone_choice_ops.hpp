// clone_choice_ops.hpp -- k_clone_choice: findRedundantImuStates (src/orcvio.cpp:2582-2626) on the poses the frame's first update leaves,
// between the two updates of orcvio_msckf_io_step_frame / _io_step_frame_ex (armed by orcvio_msckf_io_choose_clones, capi_clone_choice.inc).
// The arithmetic is host/clone_choice_model.hpp's; this file is the launch around it.
//
// One wavefront, directly behind the pose step (k_frame_head's pose block, k_pose_step, k_event_step) and in front of
// k_cov_change_anchors, the armed prune triangulation and the prune update.  Lanes 0..3 make the camera records of the four clones
// the loop can look at (key N-4, N-3, N-2, N-5) into LDS; lane 0 runs the loop, stores the result block into pinned memory and, when
// its choice is not the caller's, raises the words that make the frame's second half refuse itself:
//   raise      word [2] of the frame's kept status words (the prune update's commit: EpilogueArgs.info_also)
//   raise_evt  the feature step's status word (k_cov_change_anchors' refuse), when the frame carries anchor changes
// dx counts as applied exactly when the pose step applies it AND the first update committed: otherwise the reference's containers are
// untouched and the caller's records (cfg.cam_poses) are read as they are.  A first update that lost an in-launch hand-off (word [8])
// leaves nothing to evaluate: the call runs the frame again and this launch with it.
#pragma once
#include <hip/hip_runtime.h>

#include "frame_ops.hpp"
#include "host/clone_choice_model.hpp"

namespace orcvio_amd {

// the staged configuration, doubles in pinned memory: [0] rotation_threshold, [1] translation_threshold, [2..14) R_imu_cam0 9 |
// t_cam0_imu 3, [16 ..) cam_poses [N][12]
enum { CCH_CFG_EXT = 2, CCH_CFG_CAM = 16, CCH_SEQ_OFFSET = 128 };   // (the sequence word behind the result block, byte offset)
struct CloneChoiceArgs {
    const double* poses; int stride;   // the pose step's output: R_b2w 9 | t_b_w 3 | ..
    const double* dx;                  // the first update's
    int N, leg, apply, discard_large;
    const int* words;                  // the first update's status words as the pose step kept them (nullptr: no first update)
    const double* cfg;                 // host-coherent, layout above
    int tracking_ok, pred0, pred1;
    CloneChoice* out;                  // host-coherent result block
    unsigned long long* out_seq; unsigned long long seq;   // stored behind the block (system scope): the block of THIS frame stands
    int* raise; int* raise_evt;        // nullptr: nothing to raise (the repair path: the host reads the block before it goes on)
};

__global__ __launch_bounds__(64) void k_clone_choice(CloneChoiceArgs a) {
    __shared__ double sCam[4][CLONE_CHOICE_CAM];
    const int l = threadIdx.x, N = a.N;
    const bool lost = a.words && a.words[8] != 0;
    const bool refused = a.words && (a.words[2] != 0 || a.words[3] != 0);
    const bool app = !lost && !refused && pose_step_applies(a.dx, a.apply, a.discard_large);
    if (l < 4 && !lost) {
        const int c = l == 3 ? N - 5 : N - 4 + l;   // (N >= 6: all four in the window)
        if (app) {
            double ext[12];
            for (int i = 0; i < 12; ++i) ext[i] = a.cfg[CCH_CFG_EXT + i];
            extrinsic_increment(a.dx + 15, ext);
            const double* r = a.poses + (size_t)c * a.stride;
            clone_choice_cam_pose(r, r + 9, ext, ext + 9, sCam[l]);
        } else {
            for (int i = 0; i < CLONE_CHOICE_CAM; ++i) sCam[l][i] = a.cfg[CCH_CFG_CAM + (size_t)c * CLONE_CHOICE_CAM + i];
        }
    }
    __syncthreads();
    if (l != 0) return;
    CloneChoice o{};
    if (!lost) {
        const int pred[2] = {a.pred0, a.pred1};
        clone_choice_run(N, a.cfg[0], a.cfg[1], a.tracking_ok,
                         [&](int c, double* out) { const int slot = c == N - 5 ? 3 : c - (N - 4); for (int i = 0; i < CLONE_CHOICE_CAM; ++i) out[i] = sCam[slot][i]; },
                         pred, &o);
        if (!o.agree) {
            if (a.raise) *a.raise = 1;
            if (a.raise_evt) *a.raise_evt = 1;
        }
    }
    *a.out = o;
    __threadfence_system();
    __hip_atomic_store(a.out_seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace orcvio_amd
