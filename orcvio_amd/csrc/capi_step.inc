// capi_step.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// One FILTER frame in one call (orcvio_msckf_io_step_frame): what OrcVIO::processFeatures does to state_cov per image
// (src/orcvio.cpp:567-594) -- processModel's covariance propagation (:800-816), stateAugmentation (:962-1010), removeLostFeatures'
// update (:2497-2560), pruneImuStateBuffer's update (:2803-2851) and marginalisation (:2874-2956) -- enqueued at once on the handle's
// stream on the resident covariance; the calling thread waits once, for the flag word behind the last update.
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
    const int n = h->res_n, m = n - 6 * count;
    RemoveArgs r{};
    r.leg = leg; r.count = count;
    for (int k = 0; k < count; ++k) r.clone[k] = idx[k];   // (ascending: remove_map walks the list with the index already shifted by the earlier removals)
    const bool fac = h->fac_valid && h->fac_n == n;
    const int ldo = round_up(m + 1, 16);
    const int nb_P = (m * m + 255) / 256, nb_F = fac ? (h->fac_k * m + 255) / 256 : 0;
    hipLaunchKernelGGL(k_cov_remove_fac, dim3(nb_P + nb_F), dim3(256), 0, h->stream, (const double*)h->d_Pres, n, m, r, h->d_Ptmp, nb_P,
                       (const double*)h->d_Sres, h->fac_ld, fac ? h->fac_k : 0, h->d_Stmp, ldo);
    HIPCHK(hipGetLastError());
    if (fac) fac_adopt(h, m, h->fac_k, ldo, h->fac_tail);
    else h->fac_valid = false;
    std::swap(h->d_Pres, h->d_Ptmp);
    h->res_n = m;
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

struct StepSecond {   // what the second update of the frame needs besides the handle
    const orcvio_msckf_tracks* tr;
    const double* posesA;   // device: the first update's window poses
    const double* dxA;      // device: its dx
    const int* infoA;       // device: its status words
    int apply_dx;
};

// the second update's inputs into the (swapped-in) second arena and its launches; `wait` = run it the safe way (separate launches, the
// forked front end, the outcome checked and the commit made by the host) -- the repair path
static int step_second_update(orcvio_msckf_handle* h, const orcvio_msckf_flags& fl, int N, const StepSecond& b, bool safe, int32_t* stats, const char* who) {
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
    // window poses: the first update's, on the device (incremented by its dx or copied); the first update's status words are kept
    PoseStepArgs ps{b.posesA, h->d_poses, N, POSE_STRIDE, b.dxA, fl.leg_dim, b.apply_dx, (fl.use_larvio || fl.use_left_perturbation) ? 1 : 0,
                    fl.discard_large_update, b.infoA, safe ? (int*)nullptr : h->d_step_words};
    if (!h->step_fused || safe) {
        hipLaunchKernelGGL(k_pose_step, dim3(1), dim3(64), 0, s, ps);
        HIPCHK(hipGetLastError());
        // everything the caller's tracks hold, behind the poses
        rc = launch_ingest(h, s, h->h_stage_dev + h->io_optr, h->d_in + h->io_optr, upload_bytes(h) - h->io_optr);
        if (rc != ORCVIO_OK) return rc;
    }
    if (rc == ORCVIO_OK) rc = upload_finalize(h, who);
    if (rc != ORCVIO_OK) return rc;
    h->pw_missing = false;
    if (safe) return io_run_forked(h, stats);
    h->last_stream = s;
    if (h->step_fused) {   // ONE launch in front of the update: the pose step and the pull of the tracks + derived index arrays
        FrameHeadArgs fa{};
        fa.nb_cov = 0; fa.pose_block = 0; fa.ps = ps;
        fa.nseg = 2;
        fa.src[0] = h->h_stage_dev; fa.dst[0] = h->d_in; fa.bytes[0] = (unsigned)h->io_poses;
        fa.src[1] = h->h_stage_dev + h->io_optr; fa.dst[1] = h->d_in + h->io_optr; fa.bytes[1] = (unsigned)(upload_bytes(h) - h->io_optr);
        rc = launch_frame_head(h, s, fa);
        if (rc != ORCVIO_OK) return rc;
    }
    UpdateCall c;
    c.already_ingested = h->step_fused;   // (k_frame_head has pulled the whole arena)
    c.info_also = h->d_step_words;        // (a refused first update refuses this update's commit as well)
    rc = io_enqueue(h, s, false, true, c, true);
    h->A_deferred = h->last_update_thin ? false : front_defers_assembly(h, false);
    if (rc != ORCVIO_OK) return rc;
    h->cnt_plain_runs++;
    h->pub_enqueued++;
    h->ran = true; h->last_update_objects = false; h->last_run_kind = 0; h->last_sharded = false;
    commit_bookkeeping(h);
    return ORCVIO_OK;
}

int32_t orcvio_msckf_io_step_frame(orcvio_msckf_handle* h, const orcvio_msckf_frame_step* st, orcvio_msckf_frame_result* res) {
    const char* who = "orcvio_msckf_io_step_frame";
    if (!h || !st || !res) { g_last_error = std::string(who) + ": null argument"; return ORCVIO_ERR_INVALID; }
    if (h->io_submitted) { g_last_error = std::string(who) + ": an update submitted with orcvio_msckf_io_submit has not been collected"; return ORCVIO_ERR_INVALID; }
    if (!h->io_open || h->io_with_P) { g_last_error = std::string(who) + ": call orcvio_msckf_io_begin with with_P = 2 (or 0) first: the frame runs on the resident covariance"; return ORCVIO_ERR_INVALID; }
    if (h->comm || h->ipc) { g_last_error = std::string(who) + ": not with a communicator on the handle (the sharded calls are the multi-GPU form)"; return ORCVIO_ERR_INVALID; }
    const orcvio_msckf_flags fl = h->flags;
    const int leg = fl.leg_dim, N = h->N, n = h->n;
    if (st->leg_dim != leg) { g_last_error = std::string(who) + ": leg_dim differs from the flags of io_begin"; return ORCVIO_ERR_INVALID; }
    if ((st->Phi == nullptr) != (st->Q == nullptr)) { g_last_error = std::string(who) + ": Phi and Q come together"; return ORCVIO_ERR_INVALID; }
    if (h->res_n + (st->augment ? 6 : 0) != n) { g_last_error = std::string(who) + ": the resident covariance (+ this frame's augmentation) does not match the window of io_begin"; return ORCVIO_ERR_INVALID; }
    if (st->augment && h->n_extra > h->res_n - 15) { g_last_error = std::string(who) + ": more extra states than the resident covariance has"; return ORCVIO_ERR_INVALID; }
    if (st->n_remove < 0 || st->n_remove > 8 || (st->n_remove > 0 && !st->remove_clones)) { g_last_error = std::string(who) + ": remove_clones: at most eight"; return ORCVIO_ERR_INVALID; }
    for (int k = 0; k < st->n_remove; ++k)
        if (st->remove_clones[k] < 0 || st->remove_clones[k] >= N || (k > 0 && st->remove_clones[k] <= st->remove_clones[k - 1])) {
            g_last_error = std::string(who) + ": remove_clones must be ascending window indices"; return ORCVIO_ERR_INVALID;
        }
    if (st->prune_tracks) { const int rv = step_validate_tracks(h, st->prune_tracks, N, fl.estimate_td != 0, who); if (rv != ORCVIO_OK) return rv; }
    HIPCHK(hipSetDevice(h->device));
    static const bool timing = dbg_getenv("ORCVIO_TIMING") != nullptr;   // diagnostics: host wall time of the parts of this call
    const auto tt0 = std::chrono::steady_clock::now();
    static double tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    static int tcalls = 0;
    auto tmark = [&](int i) { if (timing) tacc[i] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tt0).count(); };
    if (h->arena_swapped) step_arena_swap(h);   // (an earlier call left through an error path)
    { const int rw = step_words(h); if (rw != ORCVIO_OK) return rw; }   // (the kept status words and the two words that join the side stream)
    if (st->prune_tracks) { const int ra = step_arena2(h); if (ra != ORCVIO_OK) return ra; }
    hipStream_t s = h->stream;
    std::memset(res, 0, sizeof(*res));
    res->n_after = h->res_n;
    if (h->dl_pending) { HIPCHK(hipStreamSynchronize(h->dl_stream)); h->dl_pending = false; }

    // ---- the covariance's bookkeeping ahead of the first update: propagation and augmentation.  The handle's fields are set first and
    // the launches recorded; they go out once the first update's tracks have passed their checks (a validation failure leaves nothing done)
    const CovState cov0 = cov_state(h);
    std::vector<std::function<int()>> head;
    // the fused form: ONE launch (k_frame_head) propagates and augments, pulls the whole arena and the in-state features' records out of
    // pinned memory and clears their dense rows; Phi, Q and the records are staged behind the tracks in the pinned arena
    const size_t slam_bytes = st->slam_features ? (size_t)st->slam_features->n_features * 160 + 9 * 64 : 0;
    const size_t off_aux = al256(upload_bytes(h));
    const bool fused = h->step_fused && off_aux + 2 * al256(sizeof(double) * leg * leg) + slam_bytes <= h->in_cap;
    FrameHeadArgs fa{};
    fa.pose_block = -1;
    if (fused && (st->Phi || st->augment)) {
        const int nn = h->res_n, m = nn + (st->augment ? 6 : 0);
        fa.P = h->d_Pres; fa.n = nn; fa.out = h->d_Ptmp; fa.m = m; fa.leg = leg; fa.pose = st->augment ? nn - h->n_extra : -1;
        fa.nb_cov = (m * m + 255) / 256;   // (the three regions enumerate every output element once)
        if (st->Phi) {
            char* hp = h->h_stage + off_aux;
            std::memcpy(hp, st->Phi, sizeof(double) * leg * leg);
            std::memcpy(hp + al256(sizeof(double) * leg * leg), st->Q, sizeof(double) * leg * leg);
            fa.Phi = reinterpret_cast<const double*>(h->h_stage_dev + off_aux);
            fa.Q = reinterpret_cast<const double*>(h->h_stage_dev + off_aux + al256(sizeof(double) * leg * leg));
        }
        std::swap(h->d_Pres, h->d_Ptmp);
        h->res_n = m;
        if (st->Phi) h->fac_valid = false;
        else if (h->fac_valid && h->fac_n == nn) {   // augmentation alone: the factor's rows are copied as orcvio_msckf_cov_augment copies them
            const int pose = fa.pose, ldo = round_up(m + 1, 16), fk = h->fac_k, fld = h->fac_ld;
            double* fs = h->d_Sres; double* fd = h->d_Stmp;
            head.push_back([=]() -> int {
                hipLaunchKernelGGL(k_fac_augment, dim3((fk * m + 255) / 256), dim3(256), 0, s, (const double*)fs, fld, fk, nn, pose, fd, ldo);
                HIPCHK(hipGetLastError());
                return ORCVIO_OK;
            });
            fac_adopt(h, m, fk, ldo, 0);
        } else h->fac_valid = false;
    }
    if (!fused && st->Phi) {
        const int nn = h->res_n;
        double* src = h->d_Pres; double* dst = h->d_Ptmp;
        double* dPhi = h->d_covT + (size_t)46 * h->n_max;
        double* dQ = dPhi + 46 * 46;
        const double* Phi = st->Phi; const double* Q = st->Q;
        head.push_back([=]() -> int {
            const AuxCopy cp[] = {{dPhi, Phi, sizeof(double) * (size_t)leg * leg}, {dQ, Q, sizeof(double) * (size_t)leg * leg}};
            const int rc = aux_copies(h, s, cp, 2);
            if (rc != ORCVIO_OK) return rc;
            hipLaunchKernelGGL(k_cov_propagate_rows, dim3((leg * nn + 255) / 256), dim3(256), 0, s, (const double*)src, nn, (const double*)dPhi, leg, h->d_covT);
            hipLaunchKernelGGL(k_cov_propagate_finish, dim3((nn * nn + 255) / 256), dim3(256), 0, s, (const double*)src, nn, (const double*)dPhi, (const double*)dQ, leg, (const double*)h->d_covT, dst);
            HIPCHK(hipGetLastError());
            return ORCVIO_OK;
        });
        std::swap(h->d_Pres, h->d_Ptmp);
        h->fac_valid = false;
    }
    if (!fused && st->augment) {
        const int nn = h->res_n, m = nn + 6, pose = nn - h->n_extra;
        double* src = h->d_Pres; double* dst = h->d_Ptmp;
        head.push_back([=]() -> int {
            hipLaunchKernelGGL(k_cov_augment, dim3((m * m + 255) / 256), dim3(256), 0, s, (const double*)src, nn, pose, dst);
            HIPCHK(hipGetLastError());
            return ORCVIO_OK;
        });
        std::swap(h->d_Pres, h->d_Ptmp);
        h->res_n = m;
        if (h->fac_valid && h->fac_n == nn) {
            const int ldo = round_up(m + 1, 16), fk = h->fac_k, fld = h->fac_ld;
            double* fs = h->d_Sres; double* fd = h->d_Stmp;
            head.push_back([=]() -> int {
                hipLaunchKernelGGL(k_fac_augment, dim3((fk * m + 255) / 256), dim3(256), 0, s, (const double*)fs, fld, fk, nn, pose, fd, ldo);
                HIPCHK(hipGetLastError());
                return ORCVIO_OK;
            });
            fac_adopt(h, m, fk, ldo, 0);
        } else h->fac_valid = false;
    }
    // ---- the first update's tracks: validated, the derived index arrays written (upload_finalize needs the prior's bookkeeping above)
    int rc = ORCVIO_OK;
    if (st->slam_features) rc = fused ? slam_prepare(h, st->slam_features) : orcvio_msckf_upload_slam_features(h, st->slam_features);   // (validation; the copies touch the records' own buffers only)
    if (rc == ORCVIO_OK) rc = upload_finalize(h, who);
    if (rc != ORCVIO_OK) { cov_restore(h, cov0); (void)arena_mark_read(h, s); return rc; }
    h->pw_missing = false;
    tmark(0);
    if (fused) {
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
    for (auto& f : head) { rc = f(); if (rc != ORCVIO_OK) return rc; }
    res->n_after = h->res_n;
    if (!fused) { rc = ingest_raw(h, s); if (rc != ORCVIO_OK) return rc; }
    tmark(1);
    // what the first update's outcome needs on the host once the handle's fields belong to the second
    std::vector<int>& keep_rows = h->frame_row_ptr;
    keep_rows = h->h_row_ptr;
    FeatureView vA = feature_view(h);
    vA.row_ptr = keep_rows.data();
    const char* soA = h->h_stage + h->in_cap;
    const double* posesA = h->d_poses; const double* dxA = h->d_dx; const int* infoA = h->d_info;
    const int FA = h->F, nobsA = h->nobs;
    h->last_stream = s;
    // (a frame without lost features and without in-state features has no first update: the covariance bookkeeping and, if there is one,
    //  the prune update are the whole frame -- the reference's removeLostFeatures returns before any arithmetic, src/orcvio.cpp:2440-2446)
    const bool first = FA > 0 || h->ekf_F > 0;
    unsigned long long pubA = 0;
    h->ekf_side_used = false;
    if (first) {
        UpdateCall c;
        c.ekf_side = fused;           // (the in-state rows beside k_front: enqueue_update)
        c.already_ingested = fused;   // (k_frame_head has pulled the whole arena)
        rc = io_enqueue(h, s, false, true, c, true);
        h->A_deferred = h->last_update_thin ? false : front_defers_assembly(h, false);
        if (rc != ORCVIO_OK) {
            if (h->ekf_side_used) {   // (a launch failed with the side stream's wait already out: let it through and drain it)
                hipLaunchKernelGGL(k_obj_done, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned*>(h->d_step_words) + 32, h->ekf_side_seq);
                (void)hipStreamSynchronize(h->side);
            }
            return rc;
        }
        h->cnt_plain_runs++;
        h->pub_enqueued++;
        pubA = h->pub_enqueued;
        h->ran = true; h->last_update_objects = false; h->last_run_kind = 0; h->last_sharded = false;
        commit_bookkeeping(h);
    } else {
        std::memset(h->h_stage + h->in_cap, 0, h->outs_small);   // (dx = 0, no status words)
        infoA = nullptr;
    }
    tmark(2);
    // ---- the second update, on what the first commits
    const bool second = st->prune_tracks != nullptr;
    FeatureView vB{};
    const char* soB = nullptr;
    unsigned long long pubB = 0;
    StepSecond sb{st->prune_tracks, posesA, dxA, infoA, first ? st->prune_apply_dx : 0};
    int rcB = ORCVIO_OK;
    if (second) {
        step_arena_swap(h);
        rcB = step_second_update(h, fl, N, sb, false, nullptr, who);
        if (rcB == ORCVIO_OK) {
            pubB = h->pub_enqueued;
            h->step_row_ptr = h->h_row_ptr;
            vB = feature_view(h);
            vB.row_ptr = h->step_row_ptr.data();
            soB = h->h_stage + h->in_cap;
        }
    }
    // ---- marginalisation, enqueued behind the updates
    const CovState cov_before_remove = cov_state(h);
    int rcR = ORCVIO_OK;
    if (rcB == ORCVIO_OK && st->n_remove > 0) rcR = step_remove(h, leg, st->remove_clones, st->n_remove);
    tmark(3);
    // ---- ONE wait: the flag word behind the last update
    rc = (pubB || pubA) ? io_wait(h, s, pubB ? pubB : pubA) : ORCVIO_OK;
    tmark(4);
    if (timing && (++tcalls % 128) == 0) {
        fprintf(stderr, "io_step_frame (mean of 128, us after entry): checks + finalize %.1f | head launched %.1f | first update enqueued %.1f | second + removal enqueued %.1f | results %.1f\n",
                tacc[0] / 128, tacc[1] / 128, tacc[2] / 128, tacc[3] / 128, tacc[4] / 128);
        for (double& v : tacc) v = 0.0;
    }
    auto leave = [&](int code) {
        if (h->arena_swapped) step_arena_swap(h);
        h->io_open = false;
        res->n_after = h->res_n;
        return code;
    };
    if (rc != ORCVIO_OK) { h->ran = false; return leave(rc); }
    res->dx = reinterpret_cast<const double*>(soA + vA.oo_dx);
    res->gamma = reinterpret_cast<const double*>(soA + vA.oo_gamma);
    res->accept = reinterpret_cast<const int32_t*>(soA + vA.oo_accept);
    if (second && rcB == ORCVIO_OK) {
        res->prune_dx = reinterpret_cast<const double*>(soB + vB.oo_dx);
        res->prune_gamma = reinterpret_cast<const double*>(soB + vB.oo_gamma);
        res->prune_accept = reinterpret_cast<const int32_t*>(soB + vB.oo_accept);
    }
    const int* infA = reinterpret_cast<const int*>(soA);
    const int* infB = soB ? reinterpret_cast<const int*>(soB) : nullptr;
    const bool lostA = first && infA[8] != 0, lostB = infB && infB[8] != 0 && !lostA;
    if (lostA || lostB) {
        // An in-launch hand-off was lost (another tenant of the device held compute units): that update's commit refused itself on the
        // device, and so did the second update's if the first was hit.  Drain, take the marginalisation back (it read the covariance, its
        // result is simply dropped), and run what was lost again the safe way -- separate launches, the outcome checked by the host.
        HIPCHK(hipStreamSynchronize(s));
        if (h->ekf_side_used) {
            HIPCHK(hipStreamSynchronize(h->side));
            h->ekf_side_skip_until = h->cnt_step_frames + 4096;
        }
        { const int rh = handoff_reset(h); if (rh != ORCVIO_OK) return rh; }
        cov_restore(h, cov_before_remove);
        h->fac_valid = false;   // (the factor a lost update left in the spare buffer is garbage or the prior's: the repeat factors P itself)
        if (lostA) {
            if (h->arena_swapped) step_arena_swap(h);
            rc = upload_begin(h, &fl, N, FA, nobsA, false, true, who);
            if (rc == ORCVIO_OK && st->slam_features) { h->io_open = true; rc = orcvio_msckf_upload_slam_features(h, st->slam_features); }
            if (rc == ORCVIO_OK) { h->io_open = true; rc = upload_finalize(h, who); }
            if (rc == ORCVIO_OK) {
                h->pw_missing = false;
                rc = io_run_forked(h, res->stats);
            }
            res->repaired++; h->cnt_step_repairs++;
            res->status_first = rc;
            if (rc != ORCVIO_OK && rc != ORCVIO_ERR_NOT_SPD) return leave(rc);
            if (second) step_arena_swap(h);
        } else {
            res->status_first = first ? feature_outcome_view(h, vA, soA, res->stats) : ORCVIO_OK;
        }
        if (second) {
            HIPCHK(hipStreamSynchronize(s));
            if (res->status_first != ORCVIO_OK) {   // (a refused first update refuses the second, as in the one-pass form)
                res->status_prune = res->status_first;
            } else {
                rcB = step_second_update(h, fl, N, sb, true, res->prune_stats, who);
                res->repaired++; h->cnt_step_repairs++;
                res->status_prune = rcB;
                if (rcB != ORCVIO_OK && rcB != ORCVIO_ERR_NOT_SPD) return leave(rcB);
                soB = h->h_stage + h->in_cap;
                res->prune_dx = reinterpret_cast<const double*>(soB + h->oo_dx);
                res->prune_gamma = reinterpret_cast<const double*>(soB + h->oo_gamma);
                res->prune_accept = reinterpret_cast<const int32_t*>(soB + h->oo_accept);
            }
        }
        if (st->n_remove > 0) { rcR = step_remove(h, leg, st->remove_clones, st->n_remove); if (rcR != ORCVIO_OK) return leave(rcR); }
        h->cnt_step_frames++;
        return leave(res->status_first != ORCVIO_OK ? res->status_first : res->status_prune);
    }
    // ---- outcomes (the refusals of the device: M not positive definite, a non-finite result)
    res->status_first = first ? feature_outcome_view(h, vA, soA, res->stats) : ORCVIO_OK;
    if (res->status_first != ORCVIO_OK) res->stats[3] = 0;
    if (second) {
        if (rcB != ORCVIO_OK) res->status_prune = rcB;
        else if (res->status_first != ORCVIO_OK) { res->status_prune = res->status_first; res->prune_stats[3] = 0; }   // (refused with the first: info_also)
        else {
            res->status_prune = feature_outcome_view(h, vB, soB, res->prune_stats);
            if (res->status_prune != ORCVIO_OK) res->prune_stats[3] = 0;
        }
    }
    h->ran = false;   // (both commits are part of the call: nothing is left for orcvio_msckf_cov_commit)
    h->cnt_step_frames++;
    if (rcR != ORCVIO_OK) return leave(rcR);
    return leave(res->status_first != ORCVIO_OK ? res->status_first : res->status_prune);
}
