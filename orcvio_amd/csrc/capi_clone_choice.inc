// capi_clone_choice.inc -- part of msckf_capi.hip (ONE translation unit: included there, in front of capi_step.inc; not compiled on its own).
// orcvio_msckf_io_choose_clones: the one-call frame checks the caller's remove_clones -- a prediction made on the poses from BEFORE the
// frame's first update -- against findRedundantImuStates (src/orcvio.cpp:2582-2626) on the poses that update LEAVES, which is where the
// reference evaluates it (pruneImuStateBuffer :2629-2645 runs behind removeLostFeatures).  k_clone_choice (clone_choice_ops.hpp) goes
// between the frame's two updates; on a disagreement the frame's second half -- anchor change, prune update, marginalisation -- is held
// back and the device's choice reported.  Nothing is enqueued here: the call stages the configuration and arms the next frame call.

enum { CCH_CFG_BYTES0 = 256 };   // pinned block: [orcvio_msckf_clone_choice | sequence word at CCH_SEQ_OFFSET | configuration doubles from here]
static_assert(sizeof(orcvio_msckf_clone_choice) == sizeof(CloneChoice) && sizeof(CloneChoice) <= CCH_SEQ_OFFSET, "the result block's layout is the model's");

static inline orcvio_msckf_clone_choice* cc_block(const orcvio_msckf_handle* h) { return reinterpret_cast<orcvio_msckf_clone_choice*>(h->h_cc); }
static inline double* cc_cfg_host(const orcvio_msckf_handle* h) { return reinterpret_cast<double*>(h->h_cc + CCH_CFG_BYTES0); }

int32_t orcvio_msckf_io_choose_clones(orcvio_msckf_handle* h, const orcvio_msckf_clone_choice_config* cfg, const orcvio_msckf_clone_choice** out) {
    const char* who = "orcvio_msckf_io_choose_clones: ";
    if (!h || !cfg || !out) { g_last_error = std::string(who) + "null argument"; return ORCVIO_ERR_INVALID; }
    if (!h->io_open) { g_last_error = std::string(who) + "call orcvio_msckf_io_begin first"; return ORCVIO_ERR_INVALID; }
    if (h->io_submitted) { g_last_error = std::string(who) + "an update submitted with orcvio_msckf_io_submit has not been collected"; return ORCVIO_ERR_INVALID; }
    if (h->comm || h->ipc) { g_last_error = std::string(who) + "not with a communicator on the handle"; return ORCVIO_ERR_INVALID; }
    const int N = h->N;
    if (N < CLONE_CHOICE_MIN_N) { g_last_error = std::string(who) + "a window of fewer than six clones (at five the reference's loop can name the oldest clone twice)"; return ORCVIO_ERR_INVALID; }
    if (!cfg->cam_poses) { g_last_error = std::string(who) + "cam_poses is NULL"; return ORCVIO_ERR_INVALID; }
    if (!(cfg->rotation_threshold > 0.0) || !(cfg->translation_threshold > 0.0) || !std::isfinite(cfg->rotation_threshold) || !std::isfinite(cfg->translation_threshold)) {
        g_last_error = std::string(who) + "thresholds must be finite and positive"; return ORCVIO_ERR_INVALID;
    }
    if (!all_finite(cfg->R_imu_cam0, 9) || !all_finite(cfg->t_cam0_imu, 3) || !all_finite(cfg->cam_poses, (size_t)CLONE_CHOICE_CAM * N)) {
        g_last_error = std::string(who) + "non-finite extrinsic or camera pose"; return ORCVIO_ERR_INVALID;
    }
    if (!h->h_cc) {
        HIPCHK(hipSetDevice(h->device));
        const size_t bytes = CCH_CFG_BYTES0 + sizeof(double) * (CCH_CFG_CAM + (size_t)CLONE_CHOICE_CAM * h->maxN);
        HIPCHK(hipHostMalloc(&h->h_cc, bytes, hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_cc_dev), h->h_cc, 0));
        std::memset(h->h_cc, 0, bytes);
    }
    // (every reader and writer of the block on the device belongs to a frame whose wait has returned)
    double* c = cc_cfg_host(h);
    c[0] = cfg->rotation_threshold; c[1] = cfg->translation_threshold;
    std::memcpy(c + CCH_CFG_EXT, cfg->R_imu_cam0, sizeof(double) * 9);
    std::memcpy(c + CCH_CFG_EXT + 9, cfg->t_cam0_imu, sizeof(double) * 3);
    std::memcpy(c + CCH_CFG_CAM, cfg->cam_poses, sizeof(double) * CLONE_CHOICE_CAM * (size_t)N);
    h->cc_tracking_ok = cfg->tracking_ok != 0 ? 1 : 0;
    h->cc_armed = true;
    *out = cc_block(h);
    return ORCVIO_OK;
}

// what a frame call that has taken the arming carries through its second half
struct StepChoice {
    int pred[2];
    int* raise_evt = nullptr;   // the feature step's status word, when the frame has anchor changes
};
// the launch: directly behind the pose step.  poses: that step's output; words: the first update's status words as the frame reads them
// at this point (the kept ones, or on the repair path the repeat's own; nullptr: no first update); raise = false: the repair path
static int launch_clone_choice(orcvio_msckf_handle* h, hipStream_t s, const orcvio_msckf_flags& fl, int N, const StepChoice& cc, const double* poses,
                               const double* dx, int apply, const int* words, bool raise) {
    CloneChoiceArgs a{};
    a.poses = poses; a.stride = POSE_STRIDE; a.dx = dx; a.N = N; a.leg = fl.leg_dim; a.apply = apply; a.discard_large = fl.discard_large_update;
    a.words = words;
    a.cfg = reinterpret_cast<const double*>(h->h_cc_dev + CCH_CFG_BYTES0);
    a.tracking_ok = h->cc_tracking_ok; a.pred0 = cc.pred[0]; a.pred1 = cc.pred[1];
    a.out = reinterpret_cast<CloneChoice*>(h->h_cc_dev);
    a.out_seq = reinterpret_cast<unsigned long long*>(h->h_cc_dev + CCH_SEQ_OFFSET); a.seq = ++h->cc_seq;
    a.raise = raise ? h->d_step_words + 2 : nullptr;
    a.raise_evt = raise ? cc.raise_evt : nullptr;
    hipLaunchKernelGGL(k_clone_choice, dim3(1), dim3(64), 0, s, a);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
// the block of the last launch stands in pinned memory (the frame's flag was raised behind it; a frame whose wait ended elsewhere drains the stream)
static int clone_choice_collect(orcvio_msckf_handle* h, hipStream_t s) {
    const unsigned long long* seq = reinterpret_cast<const unsigned long long*>(h->h_cc + CCH_SEQ_OFFSET);
    if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) != h->cc_seq) HIPCHK(hipStreamSynchronize(s));
    if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) != h->cc_seq) { g_last_error = "k_clone_choice: the result block did not arrive"; return ORCVIO_ERR_HIP; }
    return ORCVIO_OK;
}
