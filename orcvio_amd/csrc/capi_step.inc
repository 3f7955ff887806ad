// capi_step.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// One FILTER frame in one call (orcvio_msckf_io_step_frame): what OrcVIO::processFeatures does to state_cov per image
// (src/orcvio.cpp:567-594) -- processModel's covariance propagation (:800-816), stateAugmentation (:962-1010), removeLostFeatures'
// update (:2497-2560), pruneImuStateBuffer's update (:2803-2851) and marginalisation (:2874-2956) -- enqueued at once on the handle's
// stream on the resident covariance; the calling thread waits once, for the flag word behind the last update.
//
// orcvio_msckf_io_step_frame_ex is the same call with the frame's feature events (ONE implementation, step_frame_impl): the lost
// in-state features leave inside the first launch (an index map on k_frame_head's output), the changed features' positions and the
// IMU's extrinsics are made by the launch in front of the second update, k_cov_change_anchors is enqueued between the two updates and
// stores its results into pinned memory ahead of the flag the call waits on.
//
// The second update's tracks go through a SECOND pinned / device arena pair (the first update's inputs and results must stay where
// they are: its kernels have their pointers, the caller reads its results when the call returns); the arenas are swapped in and out of
// the handle's fields around the second update, so that every layout / launch helper works on it unchanged.

// ---- the second arena ----------------------------------------------------------------------------------------------------------
static int step_arena2(orcvio_msckf_handle* h) {
    if (h->d_in2) return ORCVIO_OK;
    HIPCHK(hipMalloc(&h->d_in2, h->in_cap));
    HIPCHK(hipMemset(h->d_in2, 0, h->in_cap));
    HIPCHK(hipHostMalloc(&h->h_stage2, h->stage_bytes, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_stage2_dev), h->h_stage2, 0));
    return step_words(h);
}
static void step_arena_swap(orcvio_msckf_handle* h) {
    std::swap(h->d_in, h->d_in2);
    std::swap(h->h_stage, h->h_stage2);
    std::swap(h->h_stage_dev, h->h_stage2_dev);
    if (h->d_skip2) std::swap(h->d_skip, h->d_skip2);   // (an armed first update's dropped tracks stay where its repeat looks for them)
    h->arena_swapped = !h->arena_swapped;
}

// index arrays of a track set, checked as upload_finalize checks them -- BEFORE anything of the frame is enqueued
static int step_validate_tracks(const orcvio_msckf_handle* h, const orcvio_msckf_tracks* tr, int N, bool need_zvel, const char* who) {
    if (!tr->obs_ptr || tr->n_features < 0) { g_last_error = std::string(who) + ": prune_tracks: null obs_ptr / bad count"; return ORCVIO_ERR_INVALID; }
    const int F = tr->n_features;
    if (F > h->maxF) { g_last_error = std::string(who) + ": prune_tracks exceed the handle's capacity"; return ORCVIO_ERR_CAPACITY; }
    if (F > 0 && tr->obs_ptr[0] != 0) { g_last_error = std::string(who) + ": prune_tracks: obs_ptr must start at zero"; return ORCVIO_ERR_INVALID; }
    const int nobs = F > 0 ? tr->obs_ptr[F] : 0;
    if (nobs < 0) { g_last_error = std::string(who) + ": prune_tracks: obs_ptr not monotone"; return ORCVIO_ERR_INVALID; }
    if (nobs > h->maxObs) { g_last_error = std::string(who) + ": prune_tracks: too many observations"; return ORCVIO_ERR_CAPACITY; }
    if (F > 0 && !tr->p_w) { g_last_error = std::string(who) + ": prune_tracks need positions (p_w)"; return ORCVIO_ERR_INVALID; }
    if (nobs > 0 && (!tr->obs_clone || !tr->obs_z || (need_zvel && !tr->obs_zvel))) { g_last_error = std::string(who) + ": prune_tracks: null track arrays"; return ORCVIO_ERR_INVALID; }
    for (int j = 0; j < F; ++j) {
        const int M = tr->obs_ptr[j + 1] - tr->obs_ptr[j];
        if (M < 0) { g_last_error = std::string(who) + ": prune_tracks: obs_ptr not monotone"; return ORCVIO_ERR_INVALID; }
        if (M > ORCVIO_MAX_TRACK) { g_last_error = std::string(who) + ": prune_tracks: track longer than ORCVIO_MAX_TRACK"; return ORCVIO_ERR_TRACK_TOO_LONG; }
    }
    for (int o = 0; o < nobs; ++o)
        if ((unsigned)tr->obs_clone[o] >= (unsigned)N) { g_last_error = std::string(who) + ": prune_tracks: obs_clone out of range"; return ORCVIO_ERR_INVALID; }
    return ORCVIO_OK;
}

// marginalisation of the listed clones (ascending, checked by the caller), enqueued: the covariance and its resident factor in ONE
// launch, the removed clones by value (k_cov_remove_fac) -- orcvio_msckf_cov_remove_clones' arithmetic (a gather), no index map to copy
static int step_remove(orcvio_msckf_handle* h, int leg, const int32_t* idx, int count) {
    if (!h->step_fused) return orcvio_msckf_cov_remove_clones(h, leg, idx, count);
    RemoveArgs r{};
    r.leg = leg; r.count = count;
    for (int k = 0; k < count; ++k) r.clone[k] = idx[k];   // (ascending: remove_map walks the list with the index already shifted by the earlier removals)
    const CovEdit e = h->gather(h->res_n - 6 * count);
    const int nb_P = (e.m * e.m + 255) / 256, nb_F = e.fac ? (e.fac_k * e.m + 255) / 256 : 0;
    hipLaunchKernelGGL(k_cov_remove_fac, dim3(nb_P + nb_F), dim3(256), 0, h->stream, e.P, e.n, e.m, r, e.Pout, nb_P, e.S, e.ld_in, e.fac ? e.fac_k : 0, e.Sout, e.ld_out);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// pieces of the ingest part of a k_frame_head launch
static inline int head_pieces(const FrameHeadArgs& fa) {
    int p = 0;
    for (int i = 0; i < fa.nseg; ++i) p += (int)((fa.bytes[i] + FH_PIECE - 1) / FH_PIECE);
    return p;
}
static int launch_frame_head(orcvio_msckf_handle* h, hipStream_t s, FrameHeadArgs& fa) {
    const int pieces = head_pieces(fa);
    fa.nb_ing = pieces < 1 ? 1 : (pieces > 48 ? 48 : pieces);
    if (fa.pose_block >= 0) fa.pose_block = fa.nb_ing - 1;   // (the last ingest workgroup: the least loaded one)
    if (fa.leg == 46) hipLaunchKernelGGL(k_frame_head<46>, dim3(fa.nb_cov + fa.nb_ing), dim3(256), 0, s, fa);
    else hipLaunchKernelGGL(k_frame_head<22>, dim3(fa.nb_cov + fa.nb_ing), dim3(256), 0, s, fa);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// ---- the frame's feature events (orcvio_msckf_io_step_frame_ex) --------------------------------------------------------------------
// Staging of their own: pinned [chg_i 16 x 4 | chg_d FS_DOUBLES | par_host 64 doubles | status] and device [p_w, p_fej, extrinsics
// FS_DOUBLES | params 64 doubles | status word | poses maxN records (a frame without a second update)].  The pinned block is written
// by the host once per call, behind a wait that covers every reader of the call before (the anchor change runs in front of the flag
// the call waits on, or raises it itself).
enum { EVT_H_CHGD = 256, EVT_H_PAR = 1152, EVT_H_STATUS = 1664, EVT_H_BYTES = 2048, EVT_D_PAR = 1024, EVT_D_STATUS = 1536, EVT_D_POSES = 2048 };
static int step_events(orcvio_msckf_handle* h) {
    if (h->d_evt) return ORCVIO_OK;
    HIPCHK(hipMalloc(&h->d_evt, EVT_D_POSES + sizeof(double) * POSE_STRIDE * (size_t)h->maxN));
    HIPCHK(hipMemset(h->d_evt, 0, EVT_D_POSES));
    HIPCHK(hipHostMalloc(&h->h_evt, EVT_H_BYTES, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_evt_dev), h->h_evt, 0));
    std::memset(h->h_evt, 0, EVT_H_BYTES);
    return ORCVIO_OK;
}
struct StepEvents {   // validated; k == 0 and lost.count == 0: a frame without events
    int idp = 1, literal_3d = 0, k = 0;
    LostMap lost{};
    std::vector<int> lost_slots;
    FeatureStepArgs fs{};
};
static inline int* evt_status_host(const orcvio_msckf_handle* h) { return reinterpret_cast<int*>(h->h_evt + EVT_H_STATUS); }
// k_cov_change_anchors on the resident covariance as the stream leaves it at this point, its inputs the feature step's outputs
static int launch_change_anchors(orcvio_msckf_handle* h, hipStream_t s, const StepEvents& e, const double* poses, const int* first_info, bool wire, bool publish) {
    const int leg = h->flags.leg_dim, base = leg + 6 * h->N;
    const double* dev = reinterpret_cast<const double*>(h->d_evt);
    AnchorFrameArgs fr{};
    fr.refuse = reinterpret_cast<const int*>(h->d_evt + EVT_D_STATUS);
    fr.first_info = first_info;
    fr.refuse_also = wire ? h->d_step_words + 3 : nullptr;
    fr.par_host = reinterpret_cast<double*>(h->h_evt_dev + EVT_H_PAR);
    fr.status_host = reinterpret_cast<int*>(h->h_evt_dev + EVT_H_STATUS);
    if (publish) { fr.seq = h->d_seq; fr.flag = h->h_flag_dev; }
    // (Y = J P goes to the spare covariance buffer: the buffer the commit in front has just left)
    const AnchorLaunch a{e.idp, e.literal_3d ? 1 : 0, h->flags.if_fej ? 1 : 0, e.k, base, leg, poses, dev + FS_EXT, reinterpret_cast<const int*>(h->h_evt_dev), dev,
                         reinterpret_cast<double*>(h->d_evt + EVT_D_PAR)};
    return launch_cov_change_anchors(h, s, h->change_anchors(), a, fr);
}

struct StepSecond {   // what the second update of the frame needs besides the handle
    const orcvio_msckf_tracks* tr = nullptr;
    const double* posesA = nullptr;   // device: the first update's window poses
    const double* dxA = nullptr;      // device: its dx
    const int* infoA = nullptr;       // device: its status words
    int apply_dx = 0;
    const StepEvents* ev = nullptr;   // anchor changes between the pose step and the update (nullptr: none)
    const int* also = nullptr;   // the armed IMU launch's status block: its refusal goes into the kept status words (PoseStepArgs.also)
    bool tri = false;            // armed by orcvio_msckf_io_triangulate_prune: k_triangulate on the staged list in front of the update
    const StepChoice* cc = nullptr;   // armed by orcvio_msckf_io_choose_clones: k_clone_choice directly behind the pose step
};
// the staged list of the armed prune update: where it stands in pinned memory, and its bytes
static inline size_t tri2_list_bytes(const orcvio_msckf_handle* h) { return tri_list_layout(h->tri2_F, h->tri2_nobs).bytes; }
static inline const char* tri2_list_src(const orcvio_msckf_handle* h) { return h->h_tri2_dev + tri_prune_layout(h->maxF, h->maxObs).list; }

// window poses behind the first update: its own, on the device (incremented by its dx or copied) into `out`; the first update's status
// words are kept -- not on the repair path (safe): the host has run the first update again or read its outcome
static inline PoseStepArgs step_pose_args(const orcvio_msckf_handle* h, const orcvio_msckf_flags& fl, int N, const StepSecond& b, double* out, bool safe) {
    return PoseStepArgs{b.posesA, out, N, POSE_STRIDE, b.dxA, fl.leg_dim, b.apply_dx, (fl.use_larvio || fl.use_left_perturbation) ? 1 : 0,
                        fl.discard_large_update, b.infoA, safe ? (int*)nullptr : h->d_step_words, safe ? (const int*)nullptr : b.also};
}

// An update of the frame has been enqueued (rc: what io_enqueue returned): the launch counters, the marks and the commit's bookkeeping,
// which rides in the update's last launch.  Returns the publication to wait for; 0: the enqueue failed, nothing counted.
static unsigned long long frame_update_enqueued(orcvio_msckf_handle* h, int rc) {
    h->A_deferred = h->last_update_thin ? false : front_defers_assembly(h, false);
    if (rc != ORCVIO_OK) return 0;
    h->cnt_plain_runs++;
    h->pub_enqueued++;
    mark_update_enqueued(h, 0);
    commit_bookkeeping(h);
    return h->pub_enqueued;
}

// The second update, the part both of its forms share: its inputs into the (swapped-in) second arena, the pose-step arguments, the
// validation.  separate (ORCVIO_STEP_FUSED=0, the repair path): the pose step and the pulls go out as launches of their own, in front
// of the host's validation -- they travel while it runs; the fused head pulls the derived index arrays too and goes out behind it.
static int step_second_stage(orcvio_msckf_handle* h, const orcvio_msckf_flags& fl, int N, const StepSecond& b, bool safe, PoseStepArgs& ps, const char* who) {
    hipStream_t s = h->stream;
    const orcvio_msckf_tracks* tr = b.tr;
    const int F2 = tr->n_features, nobs2 = F2 > 0 ? tr->obs_ptr[F2] : 0;
    int rc = upload_begin(h, &fl, N, F2, nobs2, false, tr->obs_zvel != nullptr, who);
    if (rc != ORCVIO_OK) return rc;
    char* st = h->h_stage;
    std::memcpy(st + h->io_optr, tr->obs_ptr, sizeof(int) * (F2 + 1));
    if (F2 > 0) {
        std::memcpy(st + h->io_pw, tr->p_w, sizeof(double) * 3 * F2);
        if (nobs2 > 0) {
            std::memcpy(st + h->io_oclone, tr->obs_clone, sizeof(int) * nobs2);
            std::memcpy(st + h->io_z, tr->obs_z, sizeof(double) * 2 * nobs2);
            if (h->io_zvel != h->io_z) std::memcpy(st + h->io_zvel, tr->obs_zvel, sizeof(double) * 2 * nobs2);
        }
    }
    ps = step_pose_args(h, fl, N, b, h->d_poses, safe);
    if (!h->step_fused || safe) {
        if (b.ev && b.ev->k > 0) hipLaunchKernelGGL(k_event_step, dim3(1), dim3(128), 0, s, ps, b.ev->fs);
        else hipLaunchKernelGGL(k_pose_step, dim3(1), dim3(64), 0, s, ps);
        HIPCHK(hipGetLastError());
        // everything the caller's tracks hold, behind the poses
        rc = launch_ingest(h, s, h->h_stage_dev + h->io_optr, h->d_in + h->io_optr, upload_bytes(h) - h->io_optr);
        if (rc == ORCVIO_OK && b.tri) rc = launch_ingest(h, s, tri2_list_src(h), h->d_tri2_list, tri2_list_bytes(h));   // (the separate launches' form of the head's segment)
        if (rc != ORCVIO_OK) return rc;
    }
    rc = upload_finalize(h, who);
    if (rc != ORCVIO_OK) return rc;
    h->pw_missing = false;
    return ORCVIO_OK;
}

// ... enqueued behind the first update, nothing waited for (the one-pass form).  *pub: the publication to wait for.
static int step_second_enqueue(orcvio_msckf_handle* h, const orcvio_msckf_flags& fl, int N, const StepSecond& b, unsigned long long* pub, const char* who) {
    hipStream_t s = h->stream;
    PoseStepArgs ps;
    int rc = step_second_stage(h, fl, N, b, false, ps, who);
    if (rc != ORCVIO_OK) return rc;
    const bool events = b.ev && b.ev->k > 0;
    h->last_stream = s;
    if (h->step_fused) {   // ONE launch in front of the update: the pose step and the pull of the tracks + derived index arrays
        FrameHeadArgs fa{};
        fa.nb_cov = 0; fa.pose_block = 0; fa.ps = ps;
        if (events) fa.fs = b.ev->fs;
        fa.nseg = 2;
        fa.src[0] = h->h_stage_dev; fa.dst[0] = h->d_in; fa.bytes[0] = (unsigned)h->io_poses;
        fa.src[1] = h->h_stage_dev + h->io_optr; fa.dst[1] = h->d_in + h->io_optr; fa.bytes[1] = (unsigned)(upload_bytes(h) - h->io_optr);
        if (b.tri) { fa.nseg = 3; fa.src[2] = tri2_list_src(h); fa.dst[2] = h->d_tri2_list; fa.bytes[2] = (unsigned)tri2_list_bytes(h); }   // (the armed prune update's list rides along)
        rc = launch_frame_head(h, s, fa);
        if (rc != ORCVIO_OK) return rc;
    }
    if (b.cc) {   // behind the pose step, in front of everything of the second half that writes the covariance
        rc = launch_clone_choice(h, s, fl, N, *b.cc, h->d_poses, b.dxA, b.apply_dx, h->d_step_words, true);
        if (rc != ORCVIO_OK) return rc;
    }
    if (events) {   // enqueued, not waited for: between the first update's commit and this update
        rc = launch_change_anchors(h, s, *b.ev, h->d_poses, h->d_step_words, true, false);
        if (rc != ORCVIO_OK) return rc;
    }
    UpdateCall c;
    c.already_ingested = h->step_fused;   // (k_frame_head has pulled the whole arena)
    c.info_also = h->d_step_words;        // (a refused first update refuses this update's commit as well)
    if (b.tri) tri_consume_prune(h, c);   // (k_triangulate behind the pull and the anchor change, in front of the tracks' launch: io_enqueue)
    rc = io_enqueue(h, s, false, true, c, true);
    *pub = frame_update_enqueued(h, rc);
    return rc;
}

// ... run the safe way on the repair path: separate launches, the forked front end, the outcome checked and the commit made by the host
static int step_second_safe(orcvio_msckf_handle* h, const orcvio_msckf_flags& fl, int N, const StepSecond& b, int32_t* stats, const char* who) {
    hipStream_t s = h->stream;
    PoseStepArgs ps;
    int rc = step_second_stage(h, fl, N, b, true, ps, who);
    if (rc != ORCVIO_OK) return rc;
    if (b.cc) {   // the same launch, the same bits; the host reads the verdict itself: on a disagreement nothing of the second half runs
        // (no status words: the host has run the first update again or read its outcome, and comes here only behind a committed one)
        rc = launch_clone_choice(h, s, fl, N, *b.cc, h->d_poses, b.dxA, b.apply_dx, nullptr, false);
        if (rc == ORCVIO_OK) rc = clone_choice_collect(h, s);
        if (rc != ORCVIO_OK) return rc;
        if (!cc_block(h)->agree) {
            std::memset(h->h_stage + h->in_cap, 0, h->outs_small);   // (prune_dx = 0, no status words)
            return ORCVIO_OK;
        }
    }
    if (b.ev && b.ev->k > 0) {   // the repair path waits anyway: the changed features' status is read before the update goes out
        rc = launch_change_anchors(h, s, *b.ev, h->d_poses, nullptr, false, false);
        if (rc != ORCVIO_OK) return rc;
        HIPCHK(hipStreamSynchronize(s));
        if (*evt_status_host(h) != 0) { g_last_error = std::string(who) + ": a changed feature's position is not finite: no anchor change, no prune update"; return ORCVIO_ERR_NOT_SPD; }
    }
    if (b.tri) {   // triangulated again: a lost FIRST update left the poses of the attempt without its dx (same poses, same bits otherwise)
        UpdateCall ct;
        ct.retry_forked = true;
        tri_consume_prune(h, ct);
        rc = launch_triangulate(h, &h->tri2_cfg, false, true, s, true, true, true, nullptr);
        if (rc != ORCVIO_OK) return rc;
    }
    return io_run_forked(h, stats);
}

// A frame without a second update that carries anchor changes: the pose step into the events' own pose records, the feature step and
// the anchor change as two launches.  publish: nothing of the frame follows that the call could wait for -- the anchor change
// raises the flag.  safe: the repair path (no kept status words: the first update has been run again and checked by the host).
static int step_events_alone(orcvio_msckf_handle* h, hipStream_t s, const orcvio_msckf_flags& fl, int N, const StepSecond& b, bool safe, bool publish) {
    double* poses = reinterpret_cast<double*>(h->d_evt + EVT_D_POSES);
    const PoseStepArgs ps = step_pose_args(h, fl, N, b, poses, safe);
    hipLaunchKernelGGL(k_event_step, dim3(1), dim3(128), 0, s, ps, b.ev->fs);
    HIPCHK(hipGetLastError());
    return launch_change_anchors(h, s, *b.ev, poses, safe ? (const int*)nullptr : h->d_step_words, false, publish);
}

// The events of a frame checked against the frame's step and what stands in the arena -- BEFORE anything of the frame is enqueued --
// and marshalled: the lost slots as the head's index map, the changes into the pinned staging.  first: the frame has a first update.
static int step_validate_events(orcvio_msckf_handle* h, const orcvio_msckf_frame_step* st, const orcvio_msckf_frame_events* ev, bool first,
                                StepEvents& e, const char* who) {
    auto bad = [&](const char* what) { g_last_error = std::string(who) + ": " + what; return ORCVIO_ERR_INVALID; };
    if (!ev || (ev->n_lost == 0 && ev->n_changes == 0)) {
        if (h->res_n + (st->augment ? 6 : 0) != h->n) return bad("the resident covariance (+ this frame's augmentation) does not match the window of io_begin");
        return ORCVIO_OK;
    }
    const int d = ev->idp_dim, nfs = ev->n_feature_states, leg = h->flags.leg_dim, N = h->N;
    if (h->n_nui > 0) return bad("feature events with Schmidt nuisance states (ORCVIO_OPT_SCHMIDT_STATES) take the separate calls");
    if ((d != 1 && d != 3) || nfs < 0 || ev->n_lost < 0 || ev->n_lost > nfs || (ev->n_lost > 0 && !ev->lost_slots)) return bad("events: idp_dim is 1 or 3, 0 <= n_lost <= n_feature_states");
    if (nfs > 64 * FH_LOST_WORDS) { g_last_error = std::string(who) + ": more in-state features than the frame call's removal map holds"; return ORCVIO_ERR_CAPACITY; }
    if (ev->n_changes < 0 || ev->n_changes > ANCHOR_MAX_K) return bad("at most 16 anchor changes");
    for (int q = 0; q < ev->n_lost; ++q)
        if (ev->lost_slots[q] < 0 || ev->lost_slots[q] >= nfs || (q > 0 && ev->lost_slots[q] <= ev->lost_slots[q - 1])) return bad("lost_slots must be ascending and in range");
    const int nkeep = nfs - ev->n_lost;
    if (h->res_n + (st->augment ? 6 : 0) - d * ev->n_lost != h->n) return bad("the resident covariance (+ this frame's augmentation - the lost features) does not match the window of io_begin");
    if (h->n_extra != d * nkeep) return bad("ORCVIO_OPT_EXTRA_STATES is not idp_dim x the in-state features that stay");
    e.idp = d; e.literal_3d = ev->literal_3d; e.k = ev->n_changes;
    e.lost.count = ev->n_lost; e.lost.idp = d; e.lost.nkeep = nkeep;
    e.lost.fbase = h->n - h->n_extra;   // (the augmented state in front of the removal: the features begin where they do behind it)
    e.lost_slots.assign(ev->lost_slots, ev->lost_slots + ev->n_lost);
    for (int q = 0; q < ev->n_lost; ++q) e.lost.bits[ev->lost_slots[q] >> 6] |= 1ull << (ev->lost_slots[q] & 63);
    if (e.k == 0) return ORCVIO_OK;
    if (!ev->changes || !ev->R_b2c || !ev->t_c_b) return bad("changes need changes[], R_b2c and t_c_b");
    if (N < 2) return bad("an anchor change needs two clones");
    const bool derive = first && st->prune_apply_dx != 0;
    const orcvio_msckf_slam_features* sf = st->slam_features;
    { const int re = step_events(h); if (re != ORCVIO_OK) return re; }
    int ci[4 * ANCHOR_MAX_K] = {0};
    double cd[FS_DOUBLES] = {0};
    for (int q = 0; q < e.k; ++q) {
        const orcvio_msckf_anchor_change& c = ev->changes[q];
        if (c.slot < 0 || c.slot >= nkeep) return bad("change: slot out of range (slots are positions AFTER the removals)");
        for (int p2 = 0; p2 < q; ++p2)
            if (ev->changes[p2].slot == c.slot) return bad("change: a slot listed twice");
        if (c.old_anchor < 0 || c.old_anchor >= N || c.new_anchor < 0 || c.new_anchor >= N) return bad("change: anchor outside the window");
        if (c.old_anchor == c.new_anchor) return bad("change: old anchor == new anchor");
        for (int r = 0; r < st->n_remove; ++r)
            if (st->remove_clones[r] == c.new_anchor) return bad("change: the new anchor is in remove_clones");
        int rec = -1;
        if (sf && sf->idp_dim == d)
            for (int f = 0; f < sf->n_features && rec < 0; ++f)
                if (sf->slot[f] == c.slot) rec = f;
        if (rec >= 0 && sf->anchor[rec] != c.old_anchor) return bad("change: the feature's slam_features record is anchored elsewhere than old_anchor");
        if (derive && rec < 0) return bad("change: with prune_apply_dx the changed feature needs its slam_features record (every in-state feature is tracked)");
        if ((!derive && !all_finite(c.p_w, 3)) || (h->flags.if_fej && !all_finite(c.p_fej, 3))) return bad("change: non-finite feature position");
        pack_anchor_change(c, h->flags.if_fej != 0, rec < 0 ? 0 : rec, ci + ANCHOR_CHG_STRIDE * q, cd + 6 * q);
    }
    pack_extrinsics(ev->R_b2c, ev->t_c_b, cd + FS_EXT);
    if (!all_finite(cd + FS_EXT, 12)) return bad("non-finite extrinsics");
    const double* poses = reinterpret_cast<const double*>(h->h_stage + h->io_poses);
    for (int i = 0; i < N; ++i)
        if (!all_finite(poses + (size_t)i * POSE_STRIDE, 27)) return bad("non-finite pose record");
    std::memcpy(h->h_evt, ci, sizeof(ci));
    std::memcpy(h->h_evt + EVT_H_CHGD, cd, sizeof(cd));
    *evt_status_host(h) = 0;
    e.fs.k = e.k; e.fs.idp = d; e.fs.base = leg + 6 * N;
    e.fs.chg_i = reinterpret_cast<const int*>(h->h_evt_dev);
    e.fs.chg_d = reinterpret_cast<const double*>(h->h_evt_dev + EVT_H_CHGD);
    e.fs.out = reinterpret_cast<double*>(h->d_evt);
    e.fs.status = reinterpret_cast<int*>(h->d_evt + EVT_D_STATUS);
    return ORCVIO_OK;   // (fs.slam / fs.cap: once the records' device buffers stand, slam_prepare)
}

// ---- one frame: its record, its phases, its one exit ---------------------------------------------------------------------------------
// What ONE call of step_frame_impl knows, on that call's stack and passed by reference through the phases below (as UpdateCall is for
// one update).  Nothing of it is state of the filter or kept in the handle: it dies with the call.
enum { PLAN_HEAD_FAC, PLAN_PROPAGATE, PLAN_AUGMENT, PLAN_GATHER };
struct FrameRun {
    // ---- the arguments
    const orcvio_msckf_frame_step* st = nullptr;
    const orcvio_msckf_frame_events* ev = nullptr;
    orcvio_msckf_frame_result* res = nullptr;
    orcvio_msckf_frame_result_ex* rex = nullptr;
    const char* who = "";
    // ---- set by the checks (frame_check)
    orcvio_msckf_flags fl{};
    int leg = 0, N = 0, n = 0;
    bool imu = false, tri2 = false, cc = false;   // the armings found on the handle (io_propagate_imu, io_triangulate_prune, io_choose_clones): taken in frame_head
    bool prop = false;                            // the frame propagates (Phi / Q given, or made on the device by the armed launch)
    StepEvents evs;
    int d_lost = 0;                               // states that leave in front of the first update
    // ---- left by frame_head
    bool begun = false;                           // nothing can refuse the frame any more: the armings are taken, launches go out (frame_leave)
    bool fused = false;
    FrameHeadArgs fa{};
    struct { int kind; CovEdit e; } plan[3];      // (fused: the factor's launch behind the head; unfused: propagation, augmentation, lost features)
    int n_plan = 0;
    std::vector<int> lost_map;                    // (the unfused removal's index map, staged when its launch goes out)
    int aug_pose = 0;                             // the new clone: in front of the feature states as they are BEFORE the removal
    StepChoice choice{};
    const int* imu_also = nullptr;                // the armed IMU launch's status block (a refused Phi refuses both updates' commits)
    CovState cov0, cov_before_second, cov_before_remove;   // the covariance's bookkeeping at entry, behind the first update, behind the second
    // ---- left by frame_first: what the first update's outcome needs on the host once the handle's fields belong to the second
    bool first = false;
    FeatureView vA{};
    const char* soA = nullptr;
    const double *posesA = nullptr, *dxA = nullptr;
    const int* infoA = nullptr;
    int FA = 0, nobsA = 0;
    bool tri_frame = false, tri_frame_empty = false;   // the first update triangulates its own tracks (orcvio_msckf_io_triangulate)
    // ---- left by frame_second_half
    bool second = false;
    StepSecond sb;
    FeatureView vB{};
    const char* soB = nullptr;
    unsigned long long pubA = 0, pubB = 0, pubE = 0;   // the publications of the first update, the second, the anchor change alone
    int rcB = ORCVIO_OK, rcR = ORCVIO_OK;              // what enqueueing the second half / the marginalisation returned
    // ---- left by frame_results
    bool held = false;            // the choice's verdict: the second half was (or is to be) held back -- no anchor change, no prune update, no marginalisation
    bool lostA = false, lostB = false, imu_bad = false;
    PhaseTimer::Run tm;           // ORCVIO_TIMING
};

// The one exit behind frame_check.  A frame that was refused before it began leaves nothing to put back (frame_head has restored the
// covariance's bookkeeping itself; the arena stays open: the caller may repair its arrays and call again).
static int frame_leave(orcvio_msckf_handle* h, FrameRun& f, int code) {
    if (!f.begun) return code;
    if (h->arena_swapped) step_arena_swap(h);
    h->io_open = false;
    f.res->n_after = h->res_n;
    return code;
}

// Every refusal that precedes the first change of filter state: covariance, factor, armings and arena stay as they were.
static int frame_check(orcvio_msckf_handle* h, FrameRun& f) {
    const orcvio_msckf_frame_step* st = f.st;
    const char* who = f.who;
    if (!h || !st || !f.res) { g_last_error = std::string(who) + ": null argument"; return ORCVIO_ERR_INVALID; }
    if (h->io_submitted) { g_last_error = std::string(who) + ": an update submitted with orcvio_msckf_io_submit has not been collected"; return ORCVIO_ERR_INVALID; }
    if (!h->io_open || h->io_with_P) { g_last_error = std::string(who) + ": call orcvio_msckf_io_begin with with_P = 2 (or 0) first: the frame runs on the resident covariance"; return ORCVIO_ERR_INVALID; }
    if (h->comm || h->ipc) { g_last_error = std::string(who) + ": not with a communicator on the handle (the sharded calls are the multi-GPU form)"; return ORCVIO_ERR_INVALID; }
    f.fl = h->flags;
    f.leg = f.fl.leg_dim; f.N = h->N; f.n = h->n;
    const int leg = f.leg, N = f.N;
    if (st->leg_dim != leg) { g_last_error = std::string(who) + ": leg_dim differs from the flags of io_begin"; return ORCVIO_ERR_INVALID; }
    if ((st->Phi == nullptr) != (st->Q == nullptr)) { g_last_error = std::string(who) + ": Phi and Q come together"; return ORCVIO_ERR_INVALID; }
    // armed by orcvio_msckf_io_propagate_imu: Phi and Q are made on the device (k_imu_phi_q) in front of the head launch
    f.imu = h->imu_armed;
    if (f.imu && st->Phi) { g_last_error = std::string(who) + ": the handle is armed by orcvio_msckf_io_propagate_imu: Phi and Q must be NULL"; return ORCVIO_ERR_INVALID; }
    if (f.imu && leg != 22) { g_last_error = std::string(who) + ": armed IMU propagation at leg_dim 22 only"; return ORCVIO_ERR_INVALID; }
    if (f.imu && h->tri_armed) { g_last_error = std::string(who) + ": armed by orcvio_msckf_io_propagate_imu AND by orcvio_msckf_io_triangulate: one of the two per frame"; return ORCVIO_ERR_INVALID; }
    f.prop = st->Phi != nullptr || f.imu;
    if (st->n_remove < 0 || st->n_remove > 8 || (st->n_remove > 0 && !st->remove_clones)) { g_last_error = std::string(who) + ": remove_clones: at most eight"; return ORCVIO_ERR_INVALID; }
    for (int k = 0; k < st->n_remove; ++k)
        if (st->remove_clones[k] < 0 || st->remove_clones[k] >= N || (k > 0 && st->remove_clones[k] <= st->remove_clones[k - 1])) {
            g_last_error = std::string(who) + ": remove_clones must be ascending window indices"; return ORCVIO_ERR_INVALID;
        }
    if (st->prune_tracks) { const int rv = step_validate_tracks(h, st->prune_tracks, N, f.fl.estimate_td != 0, who); if (rv != ORCVIO_OK) return rv; }
    // armed by orcvio_msckf_io_triangulate_prune: the second update's positions are made on the device between the two updates
    f.tri2 = h->tri2_armed;
    if (f.tri2) {
        auto bad = [&](const char* what) { g_last_error = std::string(who) + ": armed by orcvio_msckf_io_triangulate_prune: " + what; return ORCVIO_ERR_INVALID; };
        if (!st->prune_tracks) return bad("the frame has no prune_tracks");
        if (st->prune_tracks->n_features != h->tri2_F) return bad("tri_tracks and prune_tracks differ in their number of tracks");
        if (!tri_prune_covers(h->h_tri2, h->maxF, h->maxObs, h->tri2_F, st->prune_tracks->obs_ptr, st->prune_tracks->obs_clone))
            return bad("a prune observation's clone does not occur in its track's list");
    }
    // armed by orcvio_msckf_io_choose_clones: remove_clones is the caller's PREDICTION, checked on the device between the two updates
    f.cc = h->cc_armed;
    if (f.cc) {
        auto bad = [&](const char* what) { g_last_error = std::string(who) + ": armed by orcvio_msckf_io_choose_clones: " + what; return ORCVIO_ERR_INVALID; };
        if (st->n_remove != 2) return bad("n_remove must be 2");
        if (!clone_choice_possible(N, st->remove_clones[0], st->remove_clones[1])) return bad("remove_clones is not one of {N-3, N-2}, {0, N-3}, {0, N-5}, {0, 1}");
        if (!st->prune_tracks) return bad("the frame has no prune_tracks (the check rides in front of the prune update: pass a track set)");
    }
    HIPCHK(hipSetDevice(h->device));
    { const int rv = step_validate_events(h, st, f.ev, h->F > 0 || (st->slam_features && st->slam_features->n_features > 0), f.evs, who); if (rv != ORCVIO_OK) return rv; }
    f.d_lost = f.evs.idp * f.evs.lost.count;
    if (st->augment && h->n_extra + f.d_lost > h->res_n - 15) { g_last_error = std::string(who) + ": more extra states than the resident covariance has"; return ORCVIO_ERR_INVALID; }
    return ORCVIO_OK;
}

// The covariance's bookkeeping ahead of the first update and the plan of its launches; the first update's tracks validated (a refusal
// there leaves nothing done); behind that the armings are taken, k_frame_head and the planned edits go out.
static int frame_head(orcvio_msckf_handle* h, FrameRun& f) {
    const orcvio_msckf_frame_step* st = f.st;
    const int leg = f.leg;
    if (h->arena_swapped) step_arena_swap(h);   // (an earlier call left through an error path)
    { const int rw = step_words(h); if (rw != ORCVIO_OK) return rw; }   // (the kept status words and the two words that join the side stream)
    if (st->prune_tracks) { const int ra = step_arena2(h); if (ra != ORCVIO_OK) return ra; }
    hipStream_t s = h->stream;
    std::memset(f.res, 0, sizeof(*f.res));
    f.res->n_after = h->res_n;
    if (h->dl_pending) { HIPCHK(hipStreamSynchronize(h->dl_stream)); h->dl_pending = false; }

    // ---- propagation and augmentation.  The handle's fields are set first and the launches recorded; they go out once the first
    // update's tracks have passed their checks (a validation failure leaves nothing done)
    f.cov0 = cov_state(h);
    double* dPhi = h->d_covT + (size_t)46 * h->n_max; double* dQ = dPhi + 46 * 46;   // (the unfused propagation's Phi and Q, as orcvio_msckf_cov_propagate stages them)
    f.aug_pose = h->res_n - (h->n_extra + f.d_lost);
    // the fused form: ONE launch (k_frame_head) propagates and augments, pulls the whole arena and the in-state features' records out of
    // pinned memory and clears their dense rows; Phi, Q and the records are staged behind the tracks in the pinned arena
    const size_t slam_bytes = st->slam_features ? (size_t)st->slam_features->n_features * 160 + 9 * 64 : 0;
    const size_t off_aux = al256(upload_bytes(h));
    f.fused = h->step_fused && off_aux + 2 * al256(sizeof(double) * leg * leg) + slam_bytes <= h->in_cap;
    FrameHeadArgs& fa = f.fa;
    fa.pose_block = -1;
    if (f.fused && (f.prop || st->augment || f.d_lost > 0)) {
        const CovEdit e = h->head(f.prop, st->augment != 0, f.d_lost);   // (e.m: the state the first update sees)
        fa.P = e.P; fa.n = e.n; fa.out = e.Pout; fa.m = e.m; fa.leg = leg; fa.pose = st->augment ? f.aug_pose : -1;
        fa.lost = f.evs.lost;
        fa.nb_cov = (e.m * e.m + 255) / 256;   // (the three regions enumerate every output element once)
        if (st->Phi) {
            char* hp = h->h_stage + off_aux;
            std::memcpy(hp, st->Phi, sizeof(double) * leg * leg);
            std::memcpy(hp + al256(sizeof(double) * leg * leg), st->Q, sizeof(double) * leg * leg);
            fa.Phi = reinterpret_cast<const double*>(h->h_stage_dev + off_aux);
            fa.Q = reinterpret_cast<const double*>(h->h_stage_dev + off_aux + al256(sizeof(double) * leg * leg));
        }
        if (f.imu) { fa.Phi = dPhi; fa.Q = dQ; fa.refuse = imu_status(h); }   // (device memory: where k_imu_phi_q leaves them)
        if (e.fac) f.plan[f.n_plan++] = {PLAN_HEAD_FAC, e};   // no propagation: the factor's rows copied and deleted in a launch of their own
    }
    if (!f.fused && f.prop) f.plan[f.n_plan++] = {PLAN_PROPAGATE, h->propagate()};
    if (!f.fused && st->augment) f.plan[f.n_plan++] = {PLAN_AUGMENT, h->augment()};
    if (!f.fused && f.d_lost > 0) {   // the separate call's kernels (k_cov_remove / k_fac_remove) with its map
        f.lost_map = lost_features_map(h->res_n, f.evs.lost.fbase, f.evs.idp, f.evs.lost_slots.data(), f.evs.lost.count);
        f.plan[f.n_plan++] = {PLAN_GATHER, h->gather((int)f.lost_map.size())};
    }
    // ---- the first update's tracks: validated, the derived index arrays written (upload_finalize needs the prior's bookkeeping above)
    int rc = ORCVIO_OK;
    if (st->slam_features) rc = f.fused ? slam_prepare(h, st->slam_features) : orcvio_msckf_upload_slam_features(h, st->slam_features);   // (validation; the copies touch the records' own buffers only)
    if (rc == ORCVIO_OK) rc = upload_finalize(h, f.who);
    if (rc != ORCVIO_OK) { cov_restore(h, f.cov0); (void)arena_mark_read(h, s); return rc; }
    h->pw_missing = false;
    f.tm.mark(0);
    // ---- nothing can refuse the frame any more: the armings are taken, here and nowhere else
    f.begun = true;
    if (f.imu) { rc = imu_consume(h, s); if (rc != ORCVIO_OK) return rc; }
    drop_one_shot_armings(h, false);   // (the prune update's, the check of the clones that leave; the first update's own: tri_consume, frame_first)
    if (f.cc) {
        f.choice.pred[0] = st->remove_clones[0]; f.choice.pred[1] = st->remove_clones[1];
        std::memset(cc_block(h), 0, sizeof(orcvio_msckf_clone_choice));   // (evaluated = 0 until this frame's launch has stored its block)
    }
    f.imu_also = f.imu ? imu_status(h) : nullptr;
    if (f.fused) {
        fa.nseg = 1;
        fa.src[0] = h->h_stage_dev; fa.dst[0] = h->d_in; fa.bytes[0] = (unsigned)upload_bytes(h);
        if (st->slam_features && st->slam_features->n_features > 0) {   // the nine arrays of the records, staged packed behind Phi / Q
            AuxCopy cp[9];
            const int nc = slam_copies(h, st->slam_features, cp);
            size_t o = off_aux + 2 * al256(sizeof(double) * leg * leg);
            for (int i = 0; i < nc; ++i) {
                if (cp[i].bytes == 0) continue;
                std::memcpy(h->h_stage + o, cp[i].src, cp[i].bytes);
                fa.src[fa.nseg] = h->h_stage_dev + o; fa.dst[fa.nseg] = static_cast<char*>(cp[i].dst); fa.bytes[fa.nseg] = (unsigned)cp[i].bytes;
                ++fa.nseg;
                o += (cp[i].bytes + 63) & ~(size_t)63;
            }
        }
        rc = launch_frame_head(h, s, fa);
        if (rc != ORCVIO_OK) return rc;
    }
    for (int i = 0; i < f.n_plan && rc == ORCVIO_OK; ++i) {   // the launches of the edits planned above
        const CovEdit& e = f.plan[i].e;
        if (f.plan[i].kind == PLAN_HEAD_FAC) {   // the factor's rows as orcvio_msckf_cov_augment copies them and as orcvio_msckf_cov_remove_features deletes them, in one gather
            const dim3 grid((e.fac_k * e.m + 255) / 256);
            if (f.evs.lost.count > 0) hipLaunchKernelGGL(k_fac_head, grid, dim3(256), 0, s, e.S, e.ld_in, e.fac_k, fa.pose, f.evs.lost, e.m, e.Sout, e.ld_out);
            else hipLaunchKernelGGL(k_fac_augment, grid, dim3(256), 0, s, e.S, e.ld_in, e.fac_k, e.n, fa.pose, e.Sout, e.ld_out);
            HIPCHK(hipGetLastError());
        } else if (f.plan[i].kind == PLAN_PROPAGATE) {
            if (!f.imu) {
                const AuxCopy cp[] = {{dPhi, st->Phi, sizeof(double) * (size_t)leg * leg}, {dQ, st->Q, sizeof(double) * (size_t)leg * leg}};
                rc = aux_copies(h, s, cp, 2);
            }
            if (rc == ORCVIO_OK) rc = launch_cov_propagate(h, s, e, leg, dPhi, dQ, f.imu_also);
        } else if (f.plan[i].kind == PLAN_AUGMENT) rc = launch_cov_augment(h, s, e, f.aug_pose);
        else rc = launch_cov_gather(h, s, e, f.lost_map);
    }
    if (rc != ORCVIO_OK) return rc;
    f.res->n_after = h->res_n;
    if (!f.fused) rc = ingest_raw(h, s);
    return rc;
}

// The first update on what the head leaves.
// (a frame without lost features and without in-state features has no first update: the covariance bookkeeping and, if there is one,
//  the prune update are the whole frame -- the reference's removeLostFeatures returns before any arithmetic, src/orcvio.cpp:2440-2446)
static int frame_first(orcvio_msckf_handle* h, FrameRun& f) {
    hipStream_t s = h->stream;
    h->frame_row_ptr = h->h_row_ptr;
    f.vA = feature_view(h);
    f.vA.row_ptr = h->frame_row_ptr.data();
    f.soA = h->h_stage + h->in_cap;
    f.posesA = h->d_poses; f.dxA = h->d_dx; f.infoA = h->d_info;
    f.FA = h->F; f.nobsA = h->nobs;
    h->last_stream = s;
    f.first = f.FA > 0 || h->ekf_F > 0;
    h->ekf_side_used = false;
    if (!f.first) {
        std::memset(h->h_stage + h->in_cap, 0, h->outs_small);   // (dx = 0, no status words)
        f.infoA = nullptr;
        return ORCVIO_OK;
    }
    UpdateCall c;
    c.ekf_side = f.fused;           // (the in-state rows beside k_front: enqueue_update)
    c.already_ingested = f.fused;   // (k_frame_head has pulled the whole arena)
    c.info_also = f.imu_also;       // (a refused Phi refuses this update's commit)
    tri_consume(h, c);              // (armed: k_triangulate behind the head, in front of the tracks' launch)
    f.tri_frame = c.tri; f.tri_frame_empty = h->tri_refuse_empty;
    const int rc = io_enqueue(h, s, false, true, c, true);
    f.pubA = frame_update_enqueued(h, rc);
    if (rc != ORCVIO_OK && h->ekf_side_used) {   // (a launch failed with the side stream's wait already out: let it through and drain it)
        hipLaunchKernelGGL(k_obj_done, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned*>(h->d_step_words) + 32, h->ekf_side_seq);
        (void)hipStreamSynchronize(h->side);
    }
    return rc;
}

// The second half, on what the first update commits: the anchor changes alone, or the second update through the swapped-in second
// arena; the marginalisation behind them.
static int frame_second_half(orcvio_msckf_handle* h, FrameRun& f) {
    const orcvio_msckf_frame_step* st = f.st;
    hipStream_t s = h->stream;
    StepEvents& evs = f.evs;
    f.second = st->prune_tracks != nullptr;
    if (evs.k > 0) { evs.fs.slam = h->d_slam; evs.fs.cap = h->ekf_cap; }   // (the records' buffers stand: slam_prepare above)
    f.sb = StepSecond{st->prune_tracks, f.posesA, f.dxA, f.infoA, f.first ? st->prune_apply_dx : 0, evs.k > 0 ? &evs : nullptr, f.imu_also, f.tri2};
    if (f.cc) {
        if (evs.k > 0) f.choice.raise_evt = evs.fs.status;   // (a disagreement refuses the anchor change through the feature step's word)
        f.sb.cc = &f.choice;
    }
    if (!f.second && evs.k > 0) {   // no update behind the changes: the anchor change is what the call waits for
        f.rcB = step_events_alone(h, s, f.fl, f.N, f.sb, false, true);
        if (f.rcB == ORCVIO_OK) f.pubE = ++h->pub_enqueued;
    }
    f.cov_before_second = cov_state(h);
    if (f.second) {
        step_arena_swap(h);
        f.rcB = step_second_enqueue(h, f.fl, f.N, f.sb, &f.pubB, f.who);
        if (f.rcB == ORCVIO_OK) {
            h->step_row_ptr = h->h_row_ptr;
            f.vB = feature_view(h);
            f.vB.row_ptr = h->step_row_ptr.data();
            f.soB = h->h_stage + h->in_cap;
        }
    }
    // ---- marginalisation, enqueued behind the updates
    f.cov_before_remove = cov_state(h);
    // (an armed choice: the marginalisation goes out behind the wait, once the device's verdict is known, and is not waited for)
    if (f.rcB == ORCVIO_OK && st->n_remove > 0 && !f.cc) f.rcR = step_remove(h, f.leg, st->remove_clones, st->n_remove);
    return ORCVIO_OK;
}

// ONE wait: the flag word behind the last update
static int frame_wait(orcvio_msckf_handle* h, FrameRun& f) {
    const unsigned long long pub = f.pubB ? f.pubB : (f.pubE ? f.pubE : f.pubA);
    const int rc = pub ? io_wait(h, h->stream, pub) : ORCVIO_OK;
    if (rc != ORCVIO_OK) { h->ran = false; return rc; }
    if (f.imu && !pub) HIPCHK(hipStreamSynchronize(h->stream));   // (a frame without an update: the armed launch's status word is the one thing to wait for)
    return ORCVIO_OK;
}
static void frame_timing(orcvio_msckf_handle* h) {
    PhaseTimer* t = step_timer_of(h);
    if (!t || !t->due(128)) return;
    fprintf(stderr, "io_step_frame (mean of 128, us after entry): checks + finalize %.1f | head launched %.1f | first update enqueued %.1f | second + removal enqueued %.1f | results %.1f\n",
            t->mean(0, 128), t->mean(1, 128), t->mean(2, 128), t->mean(3, 128), t->mean(4, 128));
    t->reset();
}

// the word the anchor change left: a changed feature's position was not finite
static int frame_changes_status(const orcvio_msckf_handle* h, FrameRun& f) {
    const int sc = f.evs.k > 0 && *evt_status_host(h) != 0 && !f.held ? ORCVIO_ERR_NOT_SPD : ORCVIO_OK;   // (held: the word was raised by the choice)
    if (f.rex) f.rex->status_changes = sc;
    if (sc != ORCVIO_OK) g_last_error = std::string(f.who) + ": a changed feature's position is not finite (an incremented inverse depth of zero): no anchor change, no prune update";
    return sc;
}
static void frame_prune_results(orcvio_msckf_frame_result* res, const char* so, const FeatureView& v) {
    res->prune_dx = reinterpret_cast<const double*>(so + v.oo_dx);
    res->prune_gamma = reinterpret_cast<const double*>(so + v.oo_gamma);
    res->prune_accept = reinterpret_cast<const int32_t*>(so + v.oo_accept);
}
static FrameFacts frame_facts(const FrameRun& f, bool repaired) {
    FrameFacts k;
    k.repaired = repaired; k.first = f.first; k.second = f.second; k.held = f.held; k.imu_bad = f.imu_bad; k.rcB = f.rcB; k.rcR = f.rcR;
    return k;
}

// What the results on the host say before any outcome is evaluated: the choice's verdict, the result pointers, a lost hand-off.
static int frame_results(orcvio_msckf_handle* h, FrameRun& f) {
    orcvio_msckf_frame_result* res = f.res;
    f.held = f.cc && f.rcB != ORCVIO_OK;
    if (f.cc && f.rcB == ORCVIO_OK) {
        const int rc = clone_choice_collect(h, h->stream);
        if (rc != ORCVIO_OK) { h->ran = false; return rc; }
        f.held = cc_block(h)->evaluated != 0 && cc_block(h)->agree == 0;
        // held back, and the prune update took the direct form of a thin stack: that form writes no factor and its commit's bookkeeping
        // drops the resident one -- but the commit refused itself, the first update's factor stands untouched where it was
        if (f.held && h->last_update_thin) h->keep_factor_of(f.cov_before_second);
    }
    if (f.rex && f.evs.k > 0) {
        f.rex->new_param = reinterpret_cast<const double*>(h->h_evt + EVT_H_PAR);
        f.rex->new_inv_depth = f.rex->new_param + 3 * ANCHOR_MAX_K;
    }
    res->dx = reinterpret_cast<const double*>(f.soA + f.vA.oo_dx);
    res->gamma = reinterpret_cast<const double*>(f.soA + f.vA.oo_gamma);
    res->accept = reinterpret_cast<const int32_t*>(f.soA + f.vA.oo_accept);
    if (f.second && f.rcB == ORCVIO_OK) frame_prune_results(res, f.soB, f.vB);
    f.lostA = f.first && reinterpret_cast<const int*>(f.soA)[8] != 0;
    f.lostB = f.soB && reinterpret_cast<const int*>(f.soB)[8] != 0 && !f.lostA;
    // the armed launch found Phi or Q not finite: the head ran without propagation, both updates refused their commits
    f.imu_bad = f.imu && imu_refused(h);
    return ORCVIO_OK;
}

// An in-launch hand-off was lost (another tenant of the device held compute units): that update's commit refused itself on the
// device, and so did the second update's if the first was hit.  Drain, take the marginalisation back (it read the covariance, its
// result is simply dropped), and run what was lost again the safe way -- separate launches, the outcome checked by the host.
// A failure that is not a refusal of the device ends the call with its code.
static int frame_repair(orcvio_msckf_handle* h, FrameRun& f) {
    const orcvio_msckf_frame_step* st = f.st;
    orcvio_msckf_frame_result* res = f.res;
    hipStream_t s = h->stream;
    HIPCHK(hipStreamSynchronize(s));
    if (h->ekf_side_used) {
        HIPCHK(hipStreamSynchronize(h->side));
        h->ekf_side_skip_until = h->cnt_step_frames + 4096;
    }
    { const int rh = handoff_reset(h); if (rh != ORCVIO_OK) return rh; }
    cov_restore(h, f.cov_before_remove);
    h->fac_valid = false;   // (the factor a lost update left in the spare buffer is garbage or the prior's: the repeat factors P itself)
    FrameFacts k = frame_facts(f, true);
    int rc = ORCVIO_OK;
    if (f.lostA) {
        if (h->arena_swapped) step_arena_swap(h);
        rc = upload_begin(h, &f.fl, f.N, f.FA, f.nobsA, false, true, f.who);
        if (rc == ORCVIO_OK && st->slam_features) { h->io_open = true; rc = orcvio_msckf_upload_slam_features(h, st->slam_features); }
        if (rc == ORCVIO_OK) { h->io_open = true; rc = upload_finalize(h, f.who); }
        if (rc == ORCVIO_OK) {
            h->pw_missing = false;
            if (f.tri_frame) { h->skip_active = true; h->tri_live = true; h->tri_refuse_empty = f.tri_frame_empty; }   // (the positions and d_skip of the lost attempt stand in HBM)
            rc = f.imu_bad ? (int)ORCVIO_ERR_NOT_SPD : io_run_forked(h, res->stats);   // (a refused Phi: nothing to run again)
        }
        res->repaired++; h->cnt_step_repairs++;
        res->status_first = rc;
        if (rc != ORCVIO_OK && rc != ORCVIO_ERR_NOT_SPD) return rc;
        if (f.second) step_arena_swap(h);
        k.first_code = rc;
    } else {
        k.first_code = f.first ? feature_outcome_view(h, f.vA, f.soA, res->stats) : (int)ORCVIO_OK;
        // the anchor changes went through behind the first update's commit and stand: the repeat of the second update does not
        // apply them again.  Its pose step reads the first update's dx, which the lost update has overwritten on the device: put back
        f.sb.ev = nullptr;
        if (f.first) HIPCHK(hipMemcpyAsync(const_cast<double*>(f.dxA), f.soA + f.vA.oo_dx, sizeof(double) * (size_t)f.n, hipMemcpyHostToDevice, s));
    }
    FrameOutcome o = frame_outcome(k, ORCVIO_OK, ORCVIO_ERR_NOT_SPD);
    res->status_first = o.status_first;
    if (f.cc && o.status_first != ORCVIO_OK) {   // no second update will carry the choice: on the caller's records as they are (dx not applied)
        rc = launch_clone_choice(h, s, f.fl, f.N, f.choice, nullptr, f.dxA, 0, nullptr, false);
        if (rc == ORCVIO_OK) rc = clone_choice_collect(h, s);
        if (rc != ORCVIO_OK) return rc;
        f.held = cc_block(h)->agree == 0;
    }
    // (lostA: the anchor change refused itself on the first update's kept status word; it runs behind the repeat, once)
    if (f.sb.ev && !f.held && (!f.second || o.status_first != ORCVIO_OK)) {   // no second update to carry them: the changes are bookkeeping and stand
        rc = step_events_alone(h, s, f.fl, f.N, f.sb, true, false);
        if (rc != ORCVIO_OK) return rc;
        HIPCHK(hipStreamSynchronize(s));
    }
    if (f.second) {
        HIPCHK(hipStreamSynchronize(s));
        if (o.eval_second) {   // (a refused first update refuses the second, as in the one-pass form: it is not run again)
            f.rcB = step_second_safe(h, f.fl, f.N, f.sb, res->prune_stats, f.who);
            res->repaired++; h->cnt_step_repairs++;
            frame_outcome_second(k, o, f.rcB, ORCVIO_OK);
        }
        res->status_prune = o.status_prune;
        if (o.eval_second) {
            if (f.rcB != ORCVIO_OK && f.rcB != ORCVIO_ERR_NOT_SPD) return f.rcB;
            if (f.cc) f.held = cc_block(h)->agree == 0;   // (held: step_second_safe ran nothing behind the choice)
            frame_prune_results(res, h->h_stage + h->in_cap, feature_view(h));
        }
    }
    if (st->n_remove > 0 && !f.held) { f.rcR = step_remove(h, f.leg, st->remove_clones, st->n_remove); if (f.rcR != ORCVIO_OK) return f.rcR; }
    h->cnt_step_frames++;
    k.changes = frame_changes_status(h, f);
    return frame_outcome_return(k, o, ORCVIO_OK);
}

// The one-pass outcomes (the refusals of the device: M not positive definite, a non-finite result), by the table of
// host/frame_outcome.hpp, and the marginalisation behind an agreed choice.
static int frame_outcomes(orcvio_msckf_handle* h, FrameRun& f) {
    const orcvio_msckf_frame_step* st = f.st;
    orcvio_msckf_frame_result* res = f.res;
    FrameFacts k = frame_facts(f, false);
    k.first_code = f.first ? feature_outcome_view(h, f.vA, f.soA, res->stats) : (int)ORCVIO_OK;
    if (f.imu_bad) g_last_error = std::string(f.who) + ": Phi or Q of the armed IMU propagation not finite: no propagation, no update";
    k.changes = frame_changes_status(h, f);
    FrameOutcome o = frame_outcome(k, ORCVIO_OK, ORCVIO_ERR_NOT_SPD);
    if (o.eval_second) frame_outcome_second(k, o, feature_outcome_view(h, f.vB, f.soB, res->prune_stats), ORCVIO_OK);
    res->status_first = o.status_first;
    if (f.second) res->status_prune = o.status_prune;
    if (o.clear_stats3) res->stats[3] = 0;
    if (o.clear_prune_stats3) res->prune_stats[3] = 0;
    h->ran = false;   // (both commits are part of the call: nothing is left for orcvio_msckf_cov_commit)
    h->cnt_step_frames++;
    if (f.cc && !f.held && f.rcB == ORCVIO_OK && st->n_remove > 0) f.rcR = step_remove(h, f.leg, st->remove_clones, st->n_remove);   // (enqueued behind the wait, not waited for)
    k.rcR = f.rcR;
    return frame_outcome_return(k, o, ORCVIO_OK);
}

// One implementation behind both calls: ev == nullptr (or empty) is orcvio_msckf_io_step_frame.
static int step_frame_impl(orcvio_msckf_handle* h, const orcvio_msckf_frame_step* st, const orcvio_msckf_frame_events* ev, orcvio_msckf_frame_result* res,
                           orcvio_msckf_frame_result_ex* rex, const char* who) {
    FrameRun f;
    f.st = st; f.ev = ev; f.res = res; f.rex = rex; f.who = who;
    int rc = frame_check(h, f);
    if (rc != ORCVIO_OK) return rc;   // nothing done
    f.tm = PhaseTimer::begin(step_timer_of(h));
    rc = frame_head(h, f);
    if (rc != ORCVIO_OK) return frame_leave(h, f, rc);
    f.tm.mark(1);
    rc = frame_first(h, f);
    if (rc != ORCVIO_OK) return frame_leave(h, f, rc);
    f.tm.mark(2);
    rc = frame_second_half(h, f);
    if (rc != ORCVIO_OK) return frame_leave(h, f, rc);
    f.tm.mark(3);
    rc = frame_wait(h, f);
    f.tm.mark(4);
    frame_timing(h);
    if (rc == ORCVIO_OK) rc = frame_results(h, f);
    if (rc != ORCVIO_OK) return frame_leave(h, f, rc);
    return frame_leave(h, f, f.lostA || f.lostB ? frame_repair(h, f) : frame_outcomes(h, f));
}

int32_t orcvio_msckf_io_step_frame(orcvio_msckf_handle* h, const orcvio_msckf_frame_step* st, orcvio_msckf_frame_result* res) {
    return step_frame_impl(h, st, nullptr, res, nullptr, "orcvio_msckf_io_step_frame");
}
int32_t orcvio_msckf_io_step_frame_ex(orcvio_msckf_handle* h, const orcvio_msckf_frame_step* st, const orcvio_msckf_frame_events* ev,
                                      orcvio_msckf_frame_result_ex* res) {
    const char* who = "orcvio_msckf_io_step_frame_ex";
    if (!res) { g_last_error = std::string(who) + ": null argument"; return ORCVIO_ERR_INVALID; }
    res->new_param = nullptr; res->new_inv_depth = nullptr; res->status_changes = ORCVIO_OK;
    return step_frame_impl(h, st, ev, &res->frame, res, who);
}
