// capi_update.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// upload, the launches of one update, the launch-graph cache, run_local / run_finish.

// ---- upload --------------------------------------------------------------------------------
// Three steps: upload_begin (sizes -> problem dimensions, arena layout), the caller's arrays written into the pinned arena
// (by orcvio_msckf_upload from its arguments, or by the caller itself through orcvio_msckf_io_begin's pointers), and
// upload_finalize (validation of what stands in the arena, the derived index arrays).  The arena reaches the device by one
// asynchronous copy (staged callers) or by the first kernel of the update's graph (k_ingest, orcvio_msckf_io_update).
static int upload_begin(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int N, int F, int nobs, bool with_P, bool have_zvel,
                        const char* who, bool pending_aug = false) {
    if (flags->leg_dim != 22 && flags->leg_dim != 46) { g_last_error = std::string(who) + ": leg_dim must be 22 or 46"; return ORCVIO_ERR_INVALID; }
    if (N < 1 || F < 0) { g_last_error = std::string(who) + ": bad sizes"; return ORCVIO_ERR_INVALID; }
    if (h->io_submitted) { g_last_error = std::string(who) + ": an update submitted with orcvio_msckf_io_submit has not been collected"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    { const int rw = arena_wait_free(h); if (rw != ORCVIO_OK) return rw; }   // the pinned staging buffer of the previous upload is free again
    if (h->dl_pending) { HIPCHK(hipStreamSynchronize(h->dl_stream)); h->dl_pending = false; }
    if (N > h->maxN || F > h->maxF) { g_last_error = std::string(who) + ": exceeds handle capacity"; return ORCVIO_ERR_CAPACITY; }
    if (nobs < 0) { g_last_error = std::string(who) + ": obs_ptr not monotone"; return ORCVIO_ERR_INVALID; }
    if (nobs > h->maxObs) { g_last_error = std::string(who) + ": too many observations"; return ORCVIO_ERR_CAPACITY; }
    if (flags->estimate_td && F > 0 && !have_zvel) { g_last_error = std::string(who) + ": obs_zvel required with estimate_td"; return ORCVIO_ERR_INVALID; }
    const int n = flags->leg_dim + 6 * N + h->n_extra;   // (n_extra: states behind the clones that no row of this update touches)
    if (n > h->n_max) { g_last_error = "window + extra states exceed the handle's capacity"; return ORCVIO_ERR_CAPACITY; }
    if (6 * h->n_nui > h->n_extra || N + h->n_nui > h->maxN) { g_last_error = std::string(who) + ": nuisance states do not fit the extra states / the pose capacity"; return ORCVIO_ERR_CAPACITY; }
    // (pending_aug: orcvio_msckf_io_begin with_P = 2 -- the window of a frame whose augmentation orcvio_msckf_io_step_frame is about to enqueue;
    //  smaller than that by the in-state features orcvio_msckf_io_step_frame_ex removes first: the frame call checks the exact dimension)
    if (!with_P && h->res_n != n && !(pending_aug && n <= h->res_n + 6)) { g_last_error = std::string(who) + ": P == NULL but the resident covariance does not match the window"; return ORCVIO_ERR_INVALID; }
    h->uploaded = false; h->ran = false; h->io_open = false;
    drop_one_shot_armings(h);      // (orcvio_msckf_io_triangulate's, _io_triangulate_prune's, _io_choose_clones' belong to the arena they were made on; the frame call has taken the last two by now)
    h->last_update_thin = false;   // (set again by the update itself if it takes the direct form of a thin stack)
    h->flags = *flags;
    h->N = N; h->F = F; h->nobs = nobs;
    h->n = n;
    h->NA = h->ekf_mode ? h->n - 15 : flags->leg_dim + 6 * N - 15;   // (EKF-SLAM rows reach into the extra states)
    h->ekf_F = 0; h->dense_rows = 0; h->new_F = 0;
    h->NAP = round_up(h->NA + 1, 16);
    // chi-square table (src/orcvio.cpp:481-494)
    if (h->chi2_prob_cached != flags->chi2_prob) {
        h->h_chi2.assign(ORCVIO_CHI2_TABLE, 0.0);
        for (int d = 1; d < ORCVIO_CHI2_TABLE; ++d) h->h_chi2[d] = orcvio_msckf_chi2_quantile(d, flags->chi2_prob);
        HIPCHK(hipMemcpyAsync(h->d_chi2, h->h_chi2.data(), sizeof(double) * ORCVIO_CHI2_TABLE, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->chi2_prob_cached = flags->chi2_prob;
    }
    const bool with_zvel = have_zvel && flags->estimate_td;   // read by the kernels only under estimate_td
    layout_inputs(h, N + h->n_nui, F, nobs, with_zvel, with_P, h->n);   // (pose slots of the nuisance states behind the window's)
    layout_outputs(h, h->n, F);
    h->io_with_P = with_P;
    return ORCVIO_OK;
}

// bytes of the arena that travel: everything in front of P, and P itself when the prior comes from the host
static inline size_t upload_bytes(const orcvio_msckf_handle* h) {
    return h->io_with_P ? h->io_P + sizeof(double) * (size_t)h->n * h->n : h->in_used;
}
// The caller-written part of the arena (poses, tracks, P: everything behind the derived index arrays) pulled into HBM by a launch
// of its own, issued BEFORE the host validates the index arrays and derives the per-clone lists (upload_finalize, ~8 us at
// config 2): the transfer runs under that host work, and the launch graph of the update only has the derived arrays left to fetch.
// With a prior from the host the same launch brings P in as its upper tile-trapezoid and mirrors it on the device (launch_ingest_P).
static int ingest_raw(orcvio_msckf_handle* h, hipStream_t s) {
    if (h->io_with_P) return launch_ingest_P(h, s, h->io_poses, h->n);
    return launch_ingest(h, s, h->h_stage_dev + h->io_poses, h->d_in + h->io_poses, upload_bytes(h) - h->io_poses);
}

// The arena holds poses, obs_ptr, p_w, obs_clone, obs_z (obs_zvel, P): validate the index arrays and derive row_ptr (rows of
// every projected block), clone_obs / clone_ptr (observations grouped by clone: the sparse part of the compression).
static int upload_finalize(orcvio_msckf_handle* h, const char* who) {
    const int N = h->N, F = h->F, nobs = h->nobs;
    // the prior: the caller's P in the arena, or the resident covariance -- with its square-root factor if that is known NOW
    // (an orcvio_msckf_io_update may follow a commit, a cov_set, an augmentation of the previous one)
    if (!h->io_with_P) {
        if (h->res_n != h->n) { g_last_error = std::string(who) + ": P == NULL but the resident covariance does not match the window"; return ORCVIO_ERR_INVALID; }
        h->d_P = h->d_Pres;
    }
    select_prior_factor(h, h->io_with_P);
    h->NP = round_up(h->n > h->kf ? h->n : h->kf, 16);
    h->ldz = round_up(h->n + 1, 16);
    h->reg_path = (h->NP / 16) <= 14;
    select_tail(h);
    { const int rcl = factor_layout_clean(h); if (rcl != ORCVIO_OK) return rcl; }
    char* st = h->h_stage;
    const int* obs_ptr = reinterpret_cast<const int*>(st + h->io_optr);
    const int* obs_clone = reinterpret_cast<const int*>(st + h->io_oclone);
    if (F > 0 && obs_ptr[0] < 0) { g_last_error = std::string(who) + ": obs_ptr starts below zero"; return ORCVIO_ERR_INVALID; }
    if (F > 0 && obs_ptr[F] != nobs) { g_last_error = std::string(who) + ": obs_ptr[F] differs from the number of observations"; return ORCVIO_ERR_INVALID; }
    // row offsets, track-length limits
    h->h_row_ptr.resize(F + 1);
    int* row_ptr = h->h_row_ptr.data();
    row_ptr[0] = 0;
    int Mmax = 2;
    for (int j = 0; j < F; ++j) {
        const int M = obs_ptr[j + 1] - obs_ptr[j];
        if (M < 0) { g_last_error = std::string(who) + ": obs_ptr not monotone"; return ORCVIO_ERR_INVALID; }
        if (M > ORCVIO_MAX_TRACK) { g_last_error = std::string(who) + ": track longer than ORCVIO_MAX_TRACK"; return ORCVIO_ERR_TRACK_TOO_LONG; }
        if (M > Mmax) Mmax = M;
        row_ptr[j + 1] = row_ptr[j] + (M >= 2 ? 2 * M - 3 : 0);
    }
    std::memcpy(st + h->io_rptr, row_ptr, sizeof(int) * (F + 1));
    // observations grouped by clone: position of every observation in the clone-sorted order, and the row range of
    // every clone (two rows per observation) for the sparse part of the compression; the clone indices are checked on the way.
    // (Two scalar passes over the observations, ~8 us at 12 000 of them, on the critical path of a zero-copy update.  Tried in
    //  round 3 and not kept: the same stable counting sort by one workgroup of the ingest kernel while the others copy -- the
    //  host's part fell to 1.6 us, but that workgroup needed ~30 us (a PCIe round trip for the keys, then 47 dependent LDS
    //  byte updates per thread, twice) against 9.5 us for the copy it was to hide under: 0.148 ms per update instead of 0.127.)
    {
        // A stable counting sort by clone, two passes over the observations.  A track's clones are normally a contiguous run
        // c0, c0 + 1, ... (a feature is seen in consecutive camera states): such a run is counted and placed with plain
        // element-wise loops over the run (which the compiler vectorises) instead of one dependent increment per observation;
        // any other track takes the scalar form.  Same positions either way.  (~8 us -> ~3 us at 12 000 observations: this stands
        // between the caller's call and the launch of the update.)
        int cnt[ORCVIO_MAX_CLONES + 2] = {0};
        unsigned bad = 0;
        std::vector<unsigned char>& is_run = h->track_is_run;
        is_run.resize(F > 0 ? F : 1);
        const int o_first = F > 0 ? obs_ptr[0] : 0;   // (observations in front of obs_ptr[0] are carried along unused)
        for (int j = 0; j < F; ++j) {
            const int o0 = obs_ptr[j], M = obs_ptr[j + 1] - o0;
            const int* oc = obs_clone + o0;
            const int c0 = M > 0 ? oc[0] : 0;
            unsigned brk = 0;
            for (int k = 0; k < M; ++k) brk |= (unsigned)(oc[k] != c0 + k);
            const bool run = !brk && c0 >= 0 && c0 + M <= N;
            is_run[j] = run;
            if (run) {
                int* cc = cnt + c0 + 1;
                for (int k = 0; k < M; ++k) cc[k] += 1;
            } else {
                for (int k = 0; k < M; ++k) {
                    const unsigned c = (unsigned)oc[k];
                    bad |= (c >= (unsigned)N);
                    cnt[(c < (unsigned)N ? c : 0u) + 1]++;
                }
            }
        }
        // (... checked, NOT counted: no track writes their rows of Xobs, and a clone's Gram item sums every row of the clone's range --
        //  counted, they brought whatever an earlier update had left at their positions into S)
        for (int o = 0; o < o_first; ++o) bad |= ((unsigned)obs_clone[o] >= (unsigned)N);
        if (bad) { g_last_error = std::string(who) + ": obs_clone out of range"; return ORCVIO_ERR_INVALID; }
        for (int i = 0; i < N; ++i) cnt[i + 1] += cnt[i];
        int* clone_obs = reinterpret_cast<int*>(st + h->io_cobs);
        int fill[ORCVIO_MAX_CLONES + 2];
        std::memcpy(fill, cnt, sizeof(int) * (N + 1));
        for (int o = 0; o < o_first; ++o) clone_obs[o] = 0;   // (never read: no track owns them)
        for (int j = 0; j < F; ++j) {
            const int o0 = obs_ptr[j], M = obs_ptr[j + 1] - o0;
            if (M <= 0) continue;
            if (is_run[j]) {
                int* __restrict__ out = clone_obs + o0;
                int* __restrict__ ff = fill + obs_clone[o0];
                for (int k = 0; k < M; ++k) out[k] = ff[k];
                for (int k = 0; k < M; ++k) ff[k] += 1;
            } else {
                for (int k = 0; k < M; ++k) clone_obs[o0 + k] = fill[obs_clone[o0 + k]]++;
            }
        }
        int* cptr = reinterpret_cast<int*>(st + h->io_cptr);   // [0..N] row offsets
        for (int i = 0; i <= N; ++i) cptr[i] = 2 * cnt[i];
        h->s_chunks = N;
    }
    h->m_tot = row_ptr[F];
    h->Mmax = Mmax;
    // Gram chunking: a workgroup of 16 wavefronts per (tile, chunk); up to 1024 rows per chunk keeps every wavefront
    // at one batch of loads (64 rows) and the number of partial Grams small
    int chunks = (3 * F + 1023) / 1024;
    if (chunks > h->gram_chunks_cap) chunks = h->gram_chunks_cap;
    if (chunks < 1) chunks = 1;
    const int t3rows = 3 * F;   // the dense part of the compression: three rows per track
    int rpc = round_up((t3rows + chunks - 1) / chunks, 8);
    if (rpc < 8) rpc = 8;
    h->rows_per_chunk = rpc;
    h->chunks = t3rows > 0 ? (t3rows + rpc - 1) / rpc : 1;
    h->uploaded = true;
    h->ran = false;
    h->skip_active = false; h->tri_live = false; h->tri_refuse_empty = false; h->tri_live_prune = false;
    h->objects_mode = false;   // (a staged object update may have left it set)
    return ORCVIO_OK;
}

// the caller's arrays -> the arena (orcvio_msckf_upload and the copying one-shot calls); P_upper_only: the arena goes to the device through
// ingest_raw, which fetches the upper tile-trapezoid of P only (stage_prior)
static void stage_inputs(orcvio_msckf_handle* h, const orcvio_msckf_window* w, const orcvio_msckf_tracks* tr, const double* P, bool P_upper_only) {
    const int N = h->N, F = h->F, nobs = h->nobs;
    char* st = h->h_stage;
    if (P) stage_prior(h, P, h->n, P_upper_only);
    double* poses = reinterpret_cast<double*>(st + h->io_poses);
    const double* tfej = w->t_fej ? w->t_fej : w->t_b_w;
    for (int i = 0; i < N; ++i) {
        double* r = poses + (size_t)POSE_STRIDE * i;
        std::memcpy(r + POSE_R_B2W, w->R_b2w + 9 * i, 9 * sizeof(double));
        std::memcpy(r + POSE_T_B_W, w->t_b_w + 3 * i, 3 * sizeof(double));
        std::memcpy(r + POSE_T_FEJ, tfej + 3 * i, 3 * sizeof(double));
        std::memcpy(r + POSE_R_B2C, w->R_b2c + 9 * i, 9 * sizeof(double));
        std::memcpy(r + POSE_T_C_B, w->t_c_b + 3 * i, 3 * sizeof(double));
        r[27] = 0.0;
    }
    std::memcpy(st + h->io_optr, tr->obs_ptr, sizeof(int) * (F + 1));
    if (F > 0) {
        if (tr->p_w) std::memcpy(st + h->io_pw, tr->p_w, sizeof(double) * 3 * F);
        else std::memset(st + h->io_pw, 0, sizeof(double) * 3 * F);   // positions come from orcvio_msckf_triangulate_uploaded
        if (nobs > 0) {
            std::memcpy(st + h->io_oclone, tr->obs_clone, sizeof(int) * nobs);
            std::memcpy(st + h->io_z, tr->obs_z, sizeof(double) * 2 * nobs);
            if (h->io_zvel != h->io_z) std::memcpy(st + h->io_zvel, tr->obs_zvel, sizeof(double) * 2 * nobs);
        }
    }
}

static int upload_to_arena(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, const orcvio_msckf_window* w,
                           const orcvio_msckf_tracks* tr, const double* P, const char* who, bool early_ingest = false) {
    if (!h || !flags || !w || !tr || !w->R_b2w || !w->t_b_w || !w->R_b2c || !w->t_c_b || !tr->obs_ptr) {
        g_last_error = std::string(who) + ": null argument";
        return ORCVIO_ERR_INVALID;
    }
    const int N = w->n_clones, F = tr->n_features;
    if (N < 1 || F < 0) { g_last_error = std::string(who) + ": bad sizes"; return ORCVIO_ERR_INVALID; }
    if (F > h->maxF) { g_last_error = std::string(who) + ": exceeds handle capacity"; return ORCVIO_ERR_CAPACITY; }
    if (F > 0 && tr->obs_ptr[0] < 0) { g_last_error = std::string(who) + ": obs_ptr starts below zero"; return ORCVIO_ERR_INVALID; }
    const int nobs = F > 0 ? tr->obs_ptr[F] : 0;   // (observations in front of obs_ptr[0] are carried along unused)
    if (F > 0 && nobs > 0 && (!tr->obs_clone || !tr->obs_z)) { g_last_error = std::string(who) + ": null track arrays"; return ORCVIO_ERR_INVALID; }
    int rc = upload_begin(h, flags, N, F, nobs, P != nullptr, tr->obs_zvel != nullptr, who);
    if (rc != ORCVIO_OK) return rc;
    stage_inputs(h, w, tr, P, early_ingest);
    if (early_ingest) { rc = ingest_raw(h, h->stream); if (rc != ORCVIO_OK) return rc; }   // (io path: what was just staged travels under the finalize)
    rc = upload_finalize(h, who);
    if (rc != ORCVIO_OK) return rc;
    h->pw_missing = (F > 0 && !tr->p_w);
    return ORCVIO_OK;
}

int32_t orcvio_msckf_upload(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, const orcvio_msckf_window* w,
                            const orcvio_msckf_tracks* tr, const double* P) {
    const int rc = upload_to_arena(h, flags, w, tr, P, "orcvio_msckf_upload");
    if (rc != ORCVIO_OK) return rc;
    // ONE asynchronous copy (no synchronisation: the staging buffer is rewritten only by the next upload, which the caller
    // issues after the download / sync of this update; the kernels are ordered behind the copy on the same stream)
    HIPCHK(hipMemcpyAsync(h->d_in, h->h_stage, upload_bytes(h), hipMemcpyHostToDevice, h->stream));
    h->lists_stale = false;   // (the derived lists travel with the rest)
    return arena_mark_read(h, h->stream);
}

// ---- launches --------------------------------------------------------------------------------
// The three lists upload_finalize derives on the host (row_ptr, clone_ptr, clone_obs) stand at the head of the pinned arena.  The plain
// in-place update (io_launch) does not pull them into HBM: k_front reads clone_obs and clone_ptr where the host wrote them -- 120 bytes
// per track and 8 per clone item, each loaded once and well ahead of its use (msckf_kernels.hpp, feature_body) -- and never reads
// row_ptr (materialised stack only).  ONE predicate decides it for the enqueue, the launch signature and the host's flag; everything
// else (the forked front end, the repeat of a lost hand-off, the frame calls, the thin form, armed updates, staged and sharded
// updates, object updates) keeps the pull and its HBM pointers.
static inline bool thin_possible(const orcvio_msckf_handle* h, const UpdateCall& c);
static bool front_fused_active(const orcvio_msckf_handle* h, bool retry_forked);
static inline bool lists_in_place_active(const orcvio_msckf_handle* h, const UpdateCall& c) {
    return c.io_single && !c.already_ingested && front_fused_active(h, c.retry_forked) && !h->materialize && !(c.fin_pub && thin_possible(h, c)) &&
           !c.tri && !c.tri_prune && !h->objects_mode;
}
// After such an update the HBM image of the lists is an earlier upload's (h->lists_stale; cleared wherever the whole head travels).  The
// launches that read d_clone_obs / d_clone_ptr / d_row_ptr call this first: the pull the update left out, on their stream -- the repeat
// of a lost hand-off inside the same call, a staged run_update behind an in-place update.  The arena holds the lists of the last
// upload_finalize until the next one.
static int lists_refresh(orcvio_msckf_handle* h, hipStream_t s) {
    if (!h->lists_stale) return ORCVIO_OK;
    h->lists_stale = false;
    const int rc = launch_ingest(h, s, h->h_stage_dev, h->d_in, h->io_poses);
    // (one more reader of the arena, never a node of a captured graph: launch_signature gives such a sequence no signature)
    return rc == ORCVIO_OK ? arena_mark_read(h, s) : rc;
}

static FeatArgs feature_args(const orcvio_msckf_handle* h, bool lists_in_place = false) {
    FeatArgs a;
    a.poses = h->d_poses; a.p_w = h->d_pw; a.obs_ptr = h->d_obs_ptr; a.obs_clone = h->d_obs_clone;
    a.obs_z = h->d_obs_z; a.obs_zvel = h->d_obs_zvel; a.P = h->d_P; a.chi2 = h->d_chi2;
    a.row_ptr = h->d_row_ptr;   // (read with Hs only -- never by an update that reads its lists in place, whose HBM copy is stale)
    a.obs_pos = lists_in_place ? reinterpret_cast<const int*>(h->h_stage_dev + h->io_cobs) : h->d_clone_obs;
    a.skip = h->skip_active ? h->d_skip : nullptr;
    a.Hs = h->materialize ? h->d_Hs : nullptr; a.T3 = h->d_T3; a.Xobs = h->d_Xobs; a.gamma = h->d_gamma; a.accept = h->d_accept; a.Rf = h->d_Rf;
    a.sigma2 = h->flags.noise_feature * h->flags.noise_feature;
    a.n = h->n; a.leg = h->flags.leg_dim; a.N = h->N; a.NA = h->NA; a.NAP = h->NAP; a.Mmax = h->Mmax; a.F = h->F;
    a.use_larvio = h->flags.use_larvio; a.use_left = h->flags.use_left_perturbation; a.if_fej = h->flags.if_fej;
    a.estimate_td = h->flags.estimate_td;
    a.ablate = h->feat_ablate;
    return a;
}

static int launch_feature(orcvio_msckf_handle* h, hipStream_t s) {
    if (h->F == 0) return ORCVIO_OK;
    { const int rl = lists_refresh(h, s); if (rl != ORCVIO_OK) return rl; }
    const FeatArgs a = feature_args(h);
    const size_t lds = feat_lds_bytes(h->Mmax, h->NAP, h->N);
    const int npass = (h->NAP + 63) / 64;
    dim3 grid(h->F), block(256);
    switch (npass) {
        case 1: hipLaunchKernelGGL(k_feature<1>, grid, block, lds, s, a); break;
        case 2: hipLaunchKernelGGL(k_feature<2>, grid, block, lds, s, a); break;
        case 3: hipLaunchKernelGGL(k_feature<3>, grid, block, lds, s, a); break;
        case 4: hipLaunchKernelGGL(k_feature<4>, grid, block, lds, s, a); break;
        case 5: hipLaunchKernelGGL(k_feature<5>, grid, block, lds, s, a); break;
        case 6: hipLaunchKernelGGL(k_feature<6>, grid, block, lds, s, a); break;
        case 7: hipLaunchKernelGGL(k_feature<7>, grid, block, lds, s, a); break;
        default: g_last_error = "window too wide for k_feature"; return ORCVIO_ERR_CAPACITY;
    }
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// The Cholesky of the prior and the feature tracks in one launch (k_front) when everything is co-resident: register
// path (n <= 224), 1 + ceil(F/2) workgroups on the device's CUs, two feature teams + the factorisation's LDS within one
// CU's 160 KB.  Otherwise the caller forks the factorisation to the side stream and launches k_feature.
static bool front_fused_active(const orcvio_msckf_handle* h, bool retry_forked) {
    if (!h->front_fused || h->front_blocked_by_comm || !h->reg_path || h->F < 1) return false;
    if (1 + (h->F + 1) / 2 > h->n_cus) return false;   // one workgroup per CU (by LDS size), all resident at once
    if (retry_forked) return false;   // a hand-off of the fused launch timed out: this update is re-run on the forked path
    const size_t team = feat_lds_bytes(h->Mmax, h->NAP, h->N);
    const size_t lds = 2 * team > sizeof(double) * POTRF_LDS_DOUBLES ? 2 * team : sizeof(double) * POTRF_LDS_DOUBLES;
    return lds <= (size_t)160 * 1024 && (h->NAP + 63) / 64 <= 4;
}
// far workgroups of the prior's factorisation inside k_front (the look-ahead form, potrf_lookahead.hpp): from six block steps, while
// they too fit on the device beside the tracks' workgroups, and not when the prior's factor is resident (nothing to factor)
static int front_far_workgroups(const orcvio_msckf_handle* h) {
    if (h->la_solve != 3 || h->use_factor) return 0;
    const int nb = (h->n + 15) / 16;
    if (nb < 6 || nb > LA_NBMAX) return 0;
    const int nfar = la_far_workgroups(nb, 3);
    if (1 + nfar + (h->F + 1) / 2 > h->n_cus) return 0;
    return nfar;
}

static int front_row_chunks(const orcvio_msckf_handle* h) {
    const int c = (3 * h->F + 639) / 640;   // eight wavefronts x 80 rows: one batch of loads each
    return c < 1 ? 1 : c;
}
// U = [A; b^T] L_a can assemble A on the fly (k_gemm_asmA) when there are at most four partial Grams: k_front then stops
// after the Grams (one device-wide barrier instead of two, no assembly pass)
static bool front_defers_assembly(const orcvio_msckf_handle* h, bool retry_forked) { return front_fused_active(h, retry_forked) && front_row_chunks(h) <= 4 && h->NA <= 192; }

// compress_dst != nullptr: the compression (Grams + assembly of A into compress_dst) runs inside the same launch;
// grams_only: ... without the assembly (the caller's next kernel is k_gemm_asmA)
static int launch_front(orcvio_msckf_handle* h, hipStream_t s, UpdateCall& c, double* compress_dst, bool grams_only = false) {
    const bool in_place = lists_in_place_active(h, c);
    if (!in_place) { const int rl = lists_refresh(h, s); if (rl != ORCVIO_OK) return rl; }
    const FeatArgs a = feature_args(h, in_place);
    const double eps = 2.220446049250313e-16;
    const int nfar = front_far_workgroups(h);
    FrontPotrfArgs q{h->d_P, h->n, h->n, 8.0 * eps, h->d_RP, h->NP, h->d_DinvP, h->d_info, h->use_factor ? 1 : 0, rev_prior_active(h) ? 1 : 0,
                     nfar, h->d_la_rdy + 32, h->d_la_rdy + 16, h->la_spin};
    const size_t team = feat_lds_bytes(h->Mmax, h->NAP, h->N);
    size_t lds = 2 * team > sizeof(double) * POTRF_LDS_DOUBLES ? 2 * team : sizeof(double) * POTRF_LDS_DOUBLES;
    if (nfar > 0 && lds < sizeof(double) * la_lds_doubles<3>()) lds = sizeof(double) * la_lds_doubles<3>();
    const int team_doubles = (int)(team / sizeof(double));
    FrontGramArgs g{};
    g.enabled = compress_dst != nullptr ? (grams_only ? 2 : 1) : 0;
    const int t3rows = 3 * h->F;
    g.chunks = front_row_chunks(h);
    h->front_chunks = g.chunks;
    g.rows_per_chunk = round_up((t3rows + g.chunks - 1) / g.chunks, 4);
    g.Gpart = h->d_Gpart; g.S = h->d_S; g.clone_rows = in_place ? reinterpret_cast<const int*>(h->h_stage_dev + h->io_cptr) : h->d_clone_ptr; g.counter = h->d_sync; g.lost = h->d_info + 8;
    g.A_dst = compress_dst; g.cb0 = h->flags.leg_dim - 15; g.plus = extra_gram(h); g.spin_limit = h->front_spin_limit;
    g.started = c.front_mark; g.started_val = c.front_mark_val;
    if (g.enabled && g.chunks > h->gram_chunks_cap) { g_last_error = "launch_front: too many row chunks"; return ORCVIO_ERR_CAPACITY; }
    // (few tracks: workgroups without tracks join at the device-wide counter and share the Gram items -- 65 of them for a 20-clone window,
    //  seven rounds over the ten workgroups of a 20-track frame: the Grams ended 6 us behind the prior's factorisation)
    int nfb = (h->F + 1) / 2;
    if (g.enabled) {
        const int nbt = h->NAP / 16, nitems = nbt * (nbt + 1) / 2 * g.chunks + h->N;
        const int want = nitems < 64 ? nitems : 64;
        if (nfb < want && 1 + nfar + want <= h->n_cus) nfb = want;
    }
    dim3 grid(1 + nfar + nfb), block(512);
    // the window width fixes both template arguments: NPASS = ceil(NAP/64) column passes, and enough register slots
    // for the widest matrix of that class (n <= 79 / 143 / 207 / 224)
#define LAUNCH_FRONT(NPS, NSL)                                                                                                  \
    do {                                                                                                                        \
        static bool attr_set = false;                                                                                           \
        if (!attr_set) {                                                                                                        \
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_front<NPS, NSL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024))); \
            attr_set = true;                                                                                                    \
        }                                                                                                                       \
        hipLaunchKernelGGL((k_front<NPS, NSL>), grid, block, lds, s, a, q, team_doubles, g);                                    \
    } while (0)
    switch ((h->NAP + 63) / 64) {
        case 1: LAUNCH_FRONT(1, 4); break;
        case 2: LAUNCH_FRONT(2, 8); break;
        case 3: LAUNCH_FRONT(3, 16); break;
        case 4: LAUNCH_FRONT(4, 16); break;
        default: g_last_error = "launch_front: window too wide"; return ORCVIO_ERR_CAPACITY;
    }
#undef LAUNCH_FRONT
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

static int asm_dbg() {   // diagnostics switch of the assembly kernels, read once (ADVICE r2: getenv on the hot path)
    static const int v = [] { const char* e = dbg_getenv("ORCVIO_ASM_DBG"); return e ? atoi(e) : 0; }();
    return v;
}

// compression: A = X^T X - T3^T T3  (sparse rows summed per clone, dense rows by MFMA Gram)
static int launch_gram(orcvio_msckf_handle* h, hipStream_t s) {
    const int nb = h->NAP / 16, ntiles = nb * (nb + 1) / 2;
    if (h->F == 0) {
        HIPCHK(hipMemsetAsync(h->d_Gpart, 0, sizeof(double) * (size_t)h->NAP * h->NAP, s));
        return ORCVIO_OK;
    }
    { const int rl = lists_refresh(h, s); if (rl != ORCVIO_OK) return rl; }
    // grid.y < chunks: T3 tiles; grid.y == chunks: one workgroup per clone for the sparse rows
    dim3 grid(ntiles > h->N ? ntiles : h->N, h->chunks + 1), block(1024);
    hipLaunchKernelGGL(k_gram_pair, grid, block, 0, s, h->d_T3, 3 * h->F, h->NAP, h->rows_per_chunk, h->chunks, h->d_Gpart, h->d_Xobs,
                       h->d_S, (const int*)h->d_clone_ptr, h->N);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

static int launch_assemble_from(orcvio_msckf_handle* h, hipStream_t s, double* dst, int chunks, int dbg) {
    const int total = h->NAP * h->NAP;
    hipLaunchKernelGGL(k_assemble_A, dim3((total + 255) / 256), dim3(256), 0, s, h->d_S, h->F > 0 ? h->N : 0,
                       h->flags.leg_dim - 15, h->NA, h->NAP, h->d_Gpart, chunks, (size_t)total, dst, dbg, extra_gram(h));
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
static int launch_assemble(orcvio_msckf_handle* h, hipStream_t s, double* dst) { return launch_assemble_from(h, s, dst, h->chunks, asm_dbg()); }

// d_A on demand (optional outputs, tests) after an update whose k_front left the Grams only
static int assemble_deferred(orcvio_msckf_handle* h, hipStream_t s) {
    if (!h->A_deferred) return ORCVIO_OK;
    const int rc = launch_assemble_from(h, s, h->d_A, h->front_chunks, 0);
    if (rc == ORCVIO_OK) h->A_deferred = false;
    return rc;
}

// stride: doubles between consecutive blocks (0: packed); meta0: the status words behind the first block of a sharded update
// (nullptr: none) -- the launch leaves [first failing rank + 1, its status, total dof, total accepted rows] in info[9..12]
static int launch_reduce(orcvio_msckf_handle* h, hipStream_t s, const double* parts, int nparts, double* dst, size_t stride = 0,
                         const double* meta0 = nullptr) {
    const int total = h->NAP * h->NAP;
    hipLaunchKernelGGL(k_gram_reduce, dim3((total + 255) / 256), dim3(256), 0, s, parts, nparts, stride ? stride : (size_t)total, h->NAP, dst,
                       meta0, h->d_info + 9);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// k_potrf_reg / k_potrf_solve write the upper tiles of d_RP / d_RM only and rely on the strictly-lower tiles being zero
// (the consumers read the factors as dense matrices).  They are: zeroed at creation, and again whenever the leading
// dimension or the factorisation path changes -- a change of window size, not a per-update event.
static int factor_layout_clean(orcvio_msckf_handle* h) {
    if (h->NP == h->clean_NP && (int)h->reg_path == h->clean_path) return ORCVIO_OK;
    HIPCHK(hipDeviceSynchronize());   // an earlier update may still be reading the factors
    const size_t bytes = sizeof(double) * (size_t)h->NP_max * h->NP_max;
    HIPCHK(hipMemset(h->d_RP, 0, bytes));
    HIPCHK(hipMemset(h->d_RM, 0, bytes));
    HIPCHK(hipDeviceSynchronize());
    h->clean_NP = h->NP;
    h->clean_path = (int)h->reg_path;
    return ORCVIO_OK;
}

// ---- windows beyond the register-resident factorisations (15 .. 26 block steps, n <= 416): a 2 x 2 BLOCK factorisation out of the
// register kernels instead of the LDS-panel k_potrf (380-860 us per factorisation) and k_trsm_rl (110-250 us):
//     X = [X11 X12; X12^T X22],  R11 = chol(X11),  W = R11^-T X12,  S = X22 - W^T W,  R22 = chol(S),   R = [R11 W; 0 R22]
// with both diagonal blocks <= 224.  The upper factor is assembled in scratch (d_W) and handed to the consumers of this path in THEIR
// layout (lower, in place of `out`): nothing else of the LDS-panel path's conventions changes.  ORCVIO_BLK2=0: the LDS-panel kernels.
static inline bool blk2_active(const orcvio_msckf_handle* h, int nn) {
    const int nb = (nn + 15) / 16;
    return h->blk2_opt && !h->reg_path && nb > 14 && nb <= 26 && h->NP <= POTRF_MAXN;
}
static inline int blk2_split(int nn) { return 16 * (((nn + 15) / 16 + 1) / 2); }   // rows of the leading block (a multiple of 16)

// the register-resident factorisations are compiled for 4, 8, 12 and 16 register slots per worker: index of the smallest that holds a
// matrix of nb block steps, into the kernel tables below
static inline int potrf_slot_index(int nb) {
    const int need = potrf_slots_needed(nb);
    return need <= 4 ? 0 : need <= 8 ? 1 : need <= 12 ? 2 : 3;
}
// k_potrf_reg of X (nn x nn, ld ldx) into Rf (ld ldr) with no stamps and no ablation
static int launch_potrf_reg_slots(hipStream_t s, const double* X, int ldx, int nn, double tol_rel, double* Rf, int ldr, double* Dinv, int* info, int zero_lower, int rev) {
    static constexpr decltype(&k_potrf_reg<4>) kern[4] = {k_potrf_reg<4>, k_potrf_reg<8>, k_potrf_reg<12>, k_potrf_reg<16>};
    hipLaunchKernelGGL(kern[potrf_slot_index((nn + 15) / 16)], dim3(1), dim3(512), 0, s, X, ldx, nn, tol_rel, Rf, ldr, Dinv, info,
                       (unsigned long long*)nullptr, (size_t)0, (size_t)0, (size_t)0, 0, 0, zero_lower, rev);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
static int launch_potrf_reg_at(hipStream_t s, const double* X, int ldx, int nn, double tol_rel, double* Rf, int ldr, double* Dinv, int* info) {
    return launch_potrf_reg_slots(s, X, ldx, nn, tol_rel, Rf, ldr, Dinv, info, 1, 0);
}
// k_potrf_solve: chol(X) and Z = L^-1 [B1 | bx] in one launch (one factorisation workgroup, solver workgroups trailing it)
static int launch_potrf_solve_slots(hipStream_t s, const double* X, int ldx, int nn, double* Rf, int ldr, double* Dinv, int* info, int* flag, int* lost,
                                    const double* B1, long sB1i, long sB1c, int nc1, const double* bx, long sbx, double* Z, int ldz, int tail, double tail_scale) {
    const int ncb = (nc1 + (bx ? 1 : 0) + 15) / 16;
    const dim3 grid(1 + (ncb + SOLVE_WPB - 1) / SOLVE_WPB), block(512);
    static constexpr decltype(&k_potrf_solve<4>) kern[4] = {k_potrf_solve<4>, k_potrf_solve<8>, k_potrf_solve<12>, k_potrf_solve<16>};
    hipLaunchKernelGGL(kern[potrf_slot_index((nn + 15) / 16)], grid, block, 0, s, X, ldx, nn, 0.0, Rf, ldr, Dinv, info, flag, lost, B1, sB1i, sB1c, nc1,
                       bx, sbx, Z, ldz, tail, tail_scale);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
static int launch_trsm_lds_at(hipStream_t s, const double* Rf, int ldr, const double* Dinv, int nn, const double* B1, long sB1i, long sB1c, int nc1,
                              const double* bx, long sbx, double* Z, int ldz) {
    const int nwave = (nc1 + (bx ? 1 : 0) + 15) / 16;
    hipLaunchKernelGGL(k_trsm_lds, dim3((nwave + 3) / 4), dim3(256), 0, s, Rf, ldr, Dinv, nn, B1, sB1i, sB1c, nc1, bx, sbx, Z, ldz);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
static int launch_potrf_solve_at(hipStream_t s, const double* X, int ldx, int nn, double* Rf, int ldr, double* Dinv, int* info, int* flag, int* lost,
                                 const double* B1, long sB1i, long sB1c, int nc1, double* Z, int ldz) {
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), s));   // (no k_gemm of the usual sequence stands ahead of this launch)
    return launch_potrf_solve_slots(s, X, ldx, nn, Rf, ldr, Dinv, info, flag, lost, B1, sB1i, sB1c, nc1, nullptr, 0L, Z, ldz, 0, 0.0);
}
static int launch_gemm(hipStream_t s, const double* A, long sAi, long sAk, const double* B, long sBk, long sBj, int M, int N,
                       int K, double alpha, double diag_add, int upper_only, double* C, long sCi, long sCj, int* clear = nullptr,
                       const unsigned* wait = nullptr, unsigned expect = 0u, int* lost = nullptr, int* clear16 = nullptr,
                       const double* Cin = nullptr, int* clear1 = nullptr) {
    const int tiles = ((M + 15) / 16) * ((N + 15) / 16);
    hipLaunchKernelGGL(k_gemm, dim3(tiles), dim3(256), 0, s, A, sAi, sAk, B, sBk, sBj, M, N, K, alpha, diag_add,
                       upper_only, C, sCi, sCj, Cin, clear, wait, expect, lost, 1 << 19, clear16, clear1);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// semi-definite X (the prior: pivots <= tol are dropped), n x n with ld ldx, NOT modified; out: the lower factor (ld NP), Dinv per block
static int launch_potrf_blk2(orcvio_msckf_handle* h, hipStream_t s, const double* X, int ldx, int nn, double tol_rel, double* out, double* Dinv, int* info) {
    const int NP = h->NP, n1 = blk2_split(nn), n2 = nn - n1;
    double* Rs = h->d_W;                  // the upper factor [R11 W; . R22], ld NP
    double* S = h->d_Y;                   // X22 - W^T W, ld NP
    int* info_a = h->d_info + 44;         // pivot counters of the leading block (merged below)
    int rc = launch_potrf_reg_at(s, X, ldx, n1, tol_rel, Rs, NP, Dinv, info_a);
    if (rc == ORCVIO_OK) rc = launch_trsm_lds_at(s, Rs, NP, Dinv, n1, X + n1, (long)ldx, 1L, n2, nullptr, 0L, Rs + n1, NP);   // W = R11^-T X12
    if (rc != ORCVIO_OK) return rc;
    HIPCHK(hipMemcpy2DAsync(S, sizeof(double) * NP, X + (size_t)n1 * ldx + n1, sizeof(double) * ldx, sizeof(double) * n2, n2, hipMemcpyDeviceToDevice, s));
    rc = launch_gemm(s, Rs + n1, 1L, (long)NP, Rs + n1, (long)NP, 1L, n2, n2, n1, -1.0, 0.0, 1, S, (long)NP, 1L, nullptr, nullptr, 0u, nullptr, nullptr, S);
    if (rc == ORCVIO_OK) rc = launch_potrf_reg_at(s, S, NP, n2, tol_rel, Rs + (size_t)n1 * NP + n1, NP, Dinv + (size_t)256 * (n1 / 16), info);
    if (rc != ORCVIO_OK) return rc;
    hipLaunchKernelGGL(k_info_merge, dim3(1), dim3(64), 0, s, info, (const int*)info_a);
    hipLaunchKernelGGL(k_factor_to_lower, dim3((nn * nn + 255) / 256), dim3(256), 0, s, (const double*)Rs, NP, nn, out, NP);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// Cholesky X = L L^T.  reg path: upper factor R (L = R^T) written to `out` (ld = NP), L(i,j) = out[j*NP + i];
// LDS-panel path: X copied to `out`, factored in place (lower), L(i,j) = out[i*NP + j].
static int launch_potrf(orcvio_msckf_handle* h, hipStream_t s, const double* X, int ldx, int nn, double tol_rel, double* out,
                        double* Dinv, int* info, int rev = 0) {
    const int NP = h->NP;
    if (h->reg_path) {
        // (wave 0 keeps the diagonal tiles in LDS, the workers the rest in registers)
        // zero_lower = 0: `out` is d_RP / d_RM, whose strictly-lower tiles factor_layout_clean() keeps zero
        return launch_potrf_reg_slots(s, X, ldx, nn, tol_rel, out, NP, Dinv, info, 0, rev);
    } else if (blk2_active(h, nn)) {
        return launch_potrf_blk2(h, s, X, ldx, nn, tol_rel, out, Dinv, info);
    } else {
        HIPCHK(hipMemcpy2DAsync(out, sizeof(double) * NP, X, sizeof(double) * ldx, sizeof(double) * nn, nn, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_potrf, dim3(1), dim3(1024), 0, s, out, nn, NP, tol_rel, Dinv, info);
    }
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

static inline void factor_strides(const orcvio_msckf_handle* h, long& sLi, long& sLj) {
    if (h->reg_path) { sLi = 1; sLj = h->NP; } else { sLi = h->NP; sLj = 1; }
}

static int launch_trsm(orcvio_msckf_handle* h, hipStream_t s, const double* L, const double* Dinv, int nn, const double* B1,
                       long sB1i, long sB1c, int nc1, const double* bx, long sbx, double* Z, int ldz) {
    const int ncols = nc1 + (bx ? 1 : 0);
    if (h->reg_path) {   // L = R^T, R row-major with ld NP: LDS-staged panels
        const int nwave = (ncols + 15) / 16;
        hipLaunchKernelGGL(k_trsm_lds, dim3((nwave + 3) / 4), dim3(256), 0, s, L, h->NP, Dinv, nn, B1, sB1i, sB1c, nc1, bx, sbx, Z, ldz);
    } else {
        long sLi, sLj;
        factor_strides(h, sLi, sLj);
        hipLaunchKernelGGL(k_trsm_rl<TRSM_MAXBLK>, dim3((ncols + 15) / 16), dim3(64), 0, s, L, sLi, sLj, Dinv, nn, B1, sB1i, sB1c,
                           nc1, bx, sbx, Z, ldz);
    }
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

static inline bool fused_solve_active(const orcvio_msckf_handle* h) { return h->reg_path && h->fused_solve; }

// k_potrf_solve_la instead of k_potrf_solve: from six block steps (below that the whole trailing matrix is a handful of tiles), never
// in the re-run of an update whose in-launch hand-off timed out (the far workgroups are one more thing that has to be co-resident)
static inline bool la_solve_active(const orcvio_msckf_handle* h, int nb, bool retry_forked) {
    return (h->la_solve == 2 || h->la_solve == 3) && nb >= 6 && nb <= LA_NBMAX && !retry_forked;
}
static int launch_potrf_solve_la(orcvio_msckf_handle* h, hipStream_t s, int la, const double* X, int ldx, int nn, double* Rf, int ldr, double* Dinv,
                                 int* info, int* flag, int* rdy, int* lost, const double* B1, long sB1i, long sB1c, int nc1, const double* bx,
                                 long sbx, double* Z, int ldz, int tail, double tail_scale, unsigned long long* stamps, LaEnd end = LaEnd(),
                                 LaFin fin = LaFin(), int nfin = 0) {
    if (!h->la_attr) {
        HIPCHK(hipFuncSetAttribute((const void*)k_potrf_solve_la<2, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, la_lds_doubles<2>() * 8));
        HIPCHK(hipFuncSetAttribute((const void*)k_potrf_solve_la<3, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, la_lds_doubles<3>() * 8));
        HIPCHK(hipFuncSetAttribute((const void*)k_potrf_solve_la<2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, la_lds_doubles<2>() * 8));
        HIPCHK(hipFuncSetAttribute((const void*)k_potrf_solve_la<3, false>, hipFuncAttributeMaxDynamicSharedMemorySize, la_lds_doubles<3>() * 8));
        HIPCHK(hipFuncSetAttribute((const void*)k_potrf_solve_la<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, la_lds_doubles<2>() * 8));
        HIPCHK(hipFuncSetAttribute((const void*)k_potrf_solve_la<3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, la_lds_doubles<3>() * 8));
        h->la_attr = true;
    }
    const int nb = (nn + 15) / 16;
    const int ncb = (nc1 + (bx ? 1 : 0) + 15) / 16, nsolve = (ncb + SOLVE_WPB - 1) / SOLVE_WPB;
    if (stamps) nfin = 0;
    fin.first = 1 + nsolve + la_far_workgroups(nb, la);   // (the finish workgroups last: every workgroup they wait for is dispatched before them)
    const dim3 grid(fin.first + nfin), block(512);
#define LAUNCH_LA(L, T, F) hipLaunchKernelGGL((k_potrf_solve_la<L, T, F>), grid, block, (size_t)la_lds_doubles<L>() * 8, s, X, ldx, nn, Rf, ldr, Dinv, info, flag, rdy, \
                                              lost, nsolve, B1, sB1i, sB1c, nc1, bx, sbx, Z, ldz, tail, tail_scale, h->la_spin, stamps, end, fin)
    if (la == 2) { if (stamps) LAUNCH_LA(2, true, false); else if (nfin) LAUNCH_LA(2, false, true); else LAUNCH_LA(2, false, false); }
    else { if (stamps) LAUNCH_LA(3, true, false); else if (nfin) LAUNCH_LA(3, false, true); else LAUNCH_LA(3, false, false); }
#undef LAUNCH_LA
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// P+ and dx (and an object update's chi-square gate: h->obj_thr is set before the solve's stages are launched) inside the factorisation +
// solve launch (LaFin) instead of a k_finish_sqrt behind it: updates whose solve runs in the look-ahead form
static inline bool finish_fused_active(const orcvio_msckf_handle* h, const UpdateCall& c) {
    return (h->fuse_finish >= 2 || (h->fuse_finish == 1 && c.fin_frame)) && fused_solve_active(h) && la_solve_active(h, (h->kf - h->tail + 15) / 16, c.retry_forked);
}

// the joint chi-square gate of an object update (h->obj_thr is set before the solve's stages are launched): k_finish_sqrt decides it, or the
// finish workgroups of the solve's launch (LaFin::gate, which does not read `fail`); *_out: where the decision is published from
static inline ObjGate object_gate(const orcvio_msckf_handle* h, double thr, double* gamma_out, int* accept_out, const int* fail) {
    ObjGate gate;
    gate.fail = fail;
    gate.rr = h->d_A + (size_t)h->NA * h->NAP + h->NA; gate.thr = thr;
    gate.gamma = h->d_obj_gamma; gate.accept = h->d_obj_accept; gate.gamma_out = gamma_out; gate.accept_out = accept_out;
    return gate;
}

// stages of the square-root Kalman solve (see msckf_kernels.hpp)
enum { ST_POTRF_P = 0, ST_FORM_U, ST_FORM_M, ST_POTRF_M, ST_TRSM, ST_FINISH, ST_COUNT };

// chol(M) and Z = L_M^-1 [Lf^T | g] of a window beyond the register-resident kernels, by the same 2 x 2 blocks (blk2): M (full, ld NP) is
// overwritten in its trailing block, Z is complete when this returns, the lower factor goes to d_RM for the optional outputs
static int launch_potrf_solve_blk2(orcvio_msckf_handle* h, hipStream_t s, const PriorFactor& pf, int n, int kf, int NA) {
    const int NP = h->NP, ldz = h->ldz, n1 = blk2_split(kf), n2 = kf - n1;
    const long sLi = pf.sLi, sLj = pf.sLj;
    double* Rs = h->d_W;
    int* info_a = h->d_info + 44;
    int* flag = h->d_flag;
    const double* g = h->d_U + (size_t)NA * NP;
    // R11 = chol(M11) and W = R11^-T M12 in one launch
    int rc = launch_potrf_solve_at(s, h->d_M, NP, n1, Rs, NP, h->d_DinvM, info_a, flag, h->d_info + 8, h->d_M + n1, (long)NP, 1L, n2, Rs + n1, NP);
    // Z1 = R11^-T [Lf^T | g] (rows < n1)
    if (rc == ORCVIO_OK) rc = launch_trsm_lds_at(s, Rs, NP, h->d_DinvM, n1, pf.base, sLj, sLi, n, g, 1L, h->d_Z, ldz);
    // S = M22 - W^T W, in place (upper tiles)
    double* S = h->d_M + (size_t)n1 * NP + n1;
    if (rc == ORCVIO_OK) rc = launch_gemm(s, Rs + n1, 1L, (long)NP, Rs + n1, (long)NP, 1L, n2, n2, n1, -1.0, 0.0, 1, S, (long)NP, 1L, nullptr, nullptr, 0u, nullptr, nullptr, S);
    if (rc != ORCVIO_OK) return rc;
    // B2' = B2 - W^T Z1 into the rows >= n1 of Z
    hipLaunchKernelGGL(k_copy_rhs, dim3((n2 * (n + 1) + 255) / 256), dim3(256), 0, s, pf.base, sLj, sLi, n, g, 1L, n1, n2, h->d_Z, ldz);
    HIPCHK(hipGetLastError());
    double* Z2 = h->d_Z + (size_t)n1 * ldz;
    rc = launch_gemm(s, Rs + n1, 1L, (long)NP, h->d_Z, (long)ldz, 1L, n2, n + 1, n1, -1.0, 0.0, 0, Z2, (long)ldz, 1L, nullptr, nullptr, 0u, nullptr, nullptr, Z2);
    // R22 = chol(S), Z2 = R22^-T B2' (in place: every solver wavefront loads its sixteen columns before it stores them)
    if (rc == ORCVIO_OK) rc = launch_potrf_solve_at(s, S, NP, n2, Rs + (size_t)n1 * NP + n1, NP, h->d_DinvM + (size_t)256 * (n1 / 16), h->d_info + 2, flag, h->d_info + 8,
                                                    Z2, (long)ldz, 1L, n + 1, Z2, ldz);
    if (rc != ORCVIO_OK) return rc;
    hipLaunchKernelGGL(k_info_merge, dim3(1), dim3(64), 0, s, h->d_info + 2, (const int*)info_a);
    hipLaunchKernelGGL(k_factor_to_lower, dim3((kf * kf + 255) / 256), dim3(256), 0, s, (const double*)Rs, NP, kf, h->d_RM, NP);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// bound of the two polled joins of the frame call's side stream: a few milliseconds (k_front starts microseconds after the wait is
// enqueued, the rows take 20 us) -- where dispatches are serialised in another order (rocprofv3 --pmc) the join can never succeed, and the
// frame must not wait tens of milliseconds to find out; the call then repairs the frame and keeps the rows on one stream for a while
static inline int side_spin_limit(const orcvio_msckf_handle* h) { return h->front_spin_limit < (1 << 14) ? h->front_spin_limit : (1 << 14); }

// A wait inside a launch gave up (info[8]): the words of the in-launch hand-offs are put back -- the lost flag, k_front's device-wide
// counter, the words of the look-ahead factorisations (a lost hand-off leaves them as they were) -- once the caller has drained what
// may still read them; `counted`: the update is going to be run again (orcvio_msckf_counters [0])
static int handoff_reset(orcvio_msckf_handle* h, bool counted = true) {
    HIPCHK(hipMemset(h->d_info + 8, 0, sizeof(int)));
    HIPCHK(hipMemset(h->d_sync, 0, 256));
    HIPCHK(hipMemset(h->d_la_rdy, 0, 256));
    if (counted) h->front_fallbacks++;
    return ORCVIO_OK;
}

static int launch_solve_stage(orcvio_msckf_handle* h, hipStream_t s, int stage, UpdateCall& c) {
    // n = states (rows of the prior's factor), kf = columns of that factor = dimension of M (kf == n unless the resident
    // factor of an earlier update of the frame is used)
    const int NA = h->NA, NAP = h->NAP, n = h->n, kf = h->kf, NP = h->NP, ldz = h->ldz;
    const double sigma2 = h->flags.noise_feature * h->flags.noise_feature;
    const double eps = 2.220446049250313e-16;
    const PriorFactor pf = prior_factor(h);
    const long sLi = pf.sLi, sLj = pf.sLj;
    const double* La = pf.base + 15 * sLi;   // L_a(k, j) = Lf(15 + k, j)
    const int kfa = kf - h->tail;            // columns of the factor that are not zero in the active rows: dimension of M' (M = diag(M', s2 I))
    switch (stage) {
        case ST_POTRF_P:   // P = Lf Lf^T
            if (h->use_factor) return ORCVIO_OK;   // the factor is resident
            return launch_potrf(h, s, h->d_P, n, n, 8.0 * eps, h->d_RP, h->d_DinvP, h->d_info, rev_prior_active(h) ? 1 : 0);
        case ST_FORM_U:    // U[(NA+1) x kf] = [A; b^T] * L_a
            if (h->A_deferred) {   // A = scatter(S) - sum Gpart assembled inside the product (k_front left the Grams only)
                AsmArgs aa{h->d_S, h->N, h->flags.leg_dim - 15, NA, NAP, h->d_Gpart, h->front_chunks, (size_t)NAP * NAP, asm_dbg(),
                           extra_gram(h)};
                const int tiles = ((NA + 1 + 15) / 16) * ((kfa + 15) / 16);
                if (c.asm_wait) {   // (the Gram of the in-state rows comes from the side stream: enqueue_update)
                    hipLaunchKernelGGL(k_gemm_asmA_w, dim3(tiles), dim3(256), 0, s, aa, La, sLi, sLj, NA + 1, kfa, NA, h->d_U, (long)NP, 1L, c.asm_wait,
                                       c.asm_wait_val, side_spin_limit(h), h->d_info + 8);
                } else
                hipLaunchKernelGGL(k_gemm_asmA, dim3(tiles), dim3(256), 0, s, aa, La, sLi, sLj, NA + 1, kfa, NA, h->d_U, (long)NP, 1L, (int*)nullptr);
                HIPCHK(hipGetLastError());
                return ORCVIO_OK;
            }
            if (c.join_wait)   // (the frame call: A' comes from another stream; the product polls its completion counter, no stream-level join)
                return launch_gemm(s, h->d_A, NAP, 1, La, sLi, sLj, NA + 1, kfa, NA, 1.0, 0.0, 0, h->d_U, NP, 1, nullptr, c.join_wait, c.join_expect, h->d_info + 8);
            return launch_gemm(s, h->d_A, NAP, 1, La, sLi, sLj, NA + 1, kfa, NA, 1.0, 0.0, 0, h->d_U, NP, 1);
        case ST_FORM_M:    // M = s2 I + L_a^T U[0:NA]   (upper tiles)
            // (the register-resident Cholesky reads the upper tiles only; the LDS-panel fallback factors the lower triangle in place)
        {
            const int rm = launch_gemm(s, La, sLj, sLi, h->d_U, NP, 1, kfa, kfa, NA, 1.0, sigma2, h->reg_path ? 1 : 0, h->d_M, NP, 1, h->d_flag,
                                       nullptr, 0u, nullptr, h->d_la_rdy, nullptr, h->d_la_rdy + 48);
            if (rm == ORCVIO_OK && c.mark_M_word && !(fused_solve_active(h) && la_solve_active(h, (kfa + 15) / 16, c.retry_forked))) {
                // (the frame call's chained object solve waits for M on another stream: the word rises behind the product's kernel
                //  boundary -- stored by the first instruction of the look-ahead solve launch that follows (LaEnd.mark), or by a launch
                //  of its own where that form is not the one that runs)
                hipLaunchKernelGGL(k_obj_done, dim3(1), dim3(64), 0, s, c.mark_M_word, c.mark_M_val);
                c.mark_M_word = nullptr;
                HIPCHK(hipGetLastError());
            }
            return rm;
        }
        case ST_POTRF_M:
            if (fused_solve_active(h)) {   // chol(M) + Z = L_M^-1 [Lf^T | g] in one launch (solver workgroups trail the factorisation)
                const int nbm = (kfa + 15) / 16;
                const int ncb = (n + 1 + 15) / 16;
                const double* g = h->d_U + (size_t)NA * NP;
                if (la_solve_active(h, nbm, c.retry_forked)) {   // the trailing update spread over far workgroups (potrf_lookahead.hpp)
                    LaFin fin;
                    int nfin = 0;
                    if (finish_fused_active(h, c)) {   // ... and P+ / dx by finish workgroups of the same launch
                        fin.done = reinterpret_cast<unsigned*>(h->d_la_rdy + 48);   // (a line of its own; cleared by ST_FORM_M's product like the block rows' words)
                        fin.step = h->d_flag; fin.last_step = nbm - 1;
                        { static const int acq = dbg_getenv("ORCVIO_FIN_ACQ") ? atoi(dbg_getenv("ORCVIO_FIN_ACQ")) : 0; fin.acq = acq; }
                        fin.nstate = n; fin.kdim = kf; fin.s2 = sigma2; fin.P_out = h->d_Pout; fin.dx = h->d_dx; fin.P = h->d_P; fin.keep_tail = 6 * h->n_nui;
                        nfin = (ncb * (ncb + 1) / 2 + 1) / 2;
                        if (h->objects_mode) fin.gate = object_gate(h, h->obj_thr, h->d_gamma, h->d_accept, nullptr);
                    }
                    LaEnd end;
                    if (c.mark_M_word) { end.mark = c.mark_M_word; end.mark_val = c.mark_M_val; c.mark_M_word = nullptr; }
                    const int rl = launch_potrf_solve_la(h, s, h->la_solve, h->d_M, NP, kfa, h->d_RM, NP, h->d_DinvM, h->d_info + 2, h->d_flag, h->d_la_rdy,
                                                         h->d_info + 8, pf.base, sLj, sLi, n, g, 1L, h->d_Z, ldz, h->tail, 1.0 / h->flags.noise_feature, nullptr,
                                                         end, fin, nfin);
                    return rl;
                }
                return launch_potrf_solve_slots(s, h->d_M, NP, kfa, h->d_RM, NP, h->d_DinvM, h->d_info + 2, h->d_flag, h->d_info + 8, pf.base, sLj, sLi, n, g, 1L,
                                                h->d_Z, ldz, h->tail, 1.0 / h->flags.noise_feature);
            }
            if (blk2_active(h, kf)) return launch_potrf_solve_blk2(h, s, pf, n, kf, NA);   // (the triangular solve with it: ST_TRSM has nothing left to do)
            return launch_potrf(h, s, h->d_M, NP, kf, 0.0, h->d_RM, h->d_DinvM, h->d_info + 2);
        case ST_TRSM:      // Z = L_M^-1 [Lf^T | g],  g = U[NA][:]
            if (fused_solve_active(h)) return ORCVIO_OK;   // done inside k_potrf_solve
            if (blk2_active(h, kf)) return ORCVIO_OK;      // done with the 2 x 2 block factorisation
            return launch_trsm(h, s, h->d_RM, h->d_DinvM, kf, pf.base, sLj, sLi, n, h->d_U + (size_t)NA * NP, 1, h->d_Z, ldz);
        case ST_FINISH: {
            if (finish_fused_active(h, c)) return ORCVIO_OK;   // done inside k_potrf_solve_la (LaFin)
            const int nb = (n + 1 + 15) / 16, tiles = nb * (nb + 1) / 2;
            if (c.fin_pub) {   // (io_enqueue: the finish, the commit and the publication in ONE launch, frame_ops.hpp k_finish_pub)
                hipLaunchKernelGGL(k_finish_pub, dim3(tiles), dim3(256), 0, s, c.pub);
                HIPCHK(hipGetLastError());
                return ORCVIO_OK;
            }
            ObjGate gate;
            gate.fail = h->d_info + 2;   // chol(M) of this update met a non-positive pivot: P+ = P, dx = 0
            if (h->objects_mode) gate = object_gate(h, h->obj_thr, h->d_gamma, h->d_accept, gate.fail);
            hipLaunchKernelGGL(k_finish_sqrt, dim3(tiles), dim3(256), 0, s, h->d_Z, ldz, n, kf, sigma2, h->d_Pout, h->d_dx, gate, h->d_P, 6 * h->n_nui);
            HIPCHK(hipGetLastError());
            return ORCVIO_OK;
        }
        default: return ORCVIO_ERR_INVALID;
    }
}

// fork: Cholesky of the prior on the side stream (depends on P only)
static int launch_prior_fork(orcvio_msckf_handle* h, hipStream_t s) {
    h->prior_forked = !h->use_factor;
    if (h->use_factor) return ORCVIO_OK;   // the prior's factor is resident: nothing to fork, nothing to join
    HIPCHK(hipEventRecord(h->ev_fork, s));
    HIPCHK(hipStreamWaitEvent(h->side, h->ev_fork, 0));
    UpdateCall none;   // (the prior's factorisation takes nothing of the call's record)
    int rc = launch_solve_stage(h, h->side, ST_POTRF_P, none);   // writes d_info[0..1] itself
    if (rc != ORCVIO_OK) return rc;
    HIPCHK(hipEventRecord(h->ev_side, h->side));
    return ORCVIO_OK;
}

static int launch_solve_tail(orcvio_msckf_handle* h, hipStream_t s, UpdateCall& c) {
    if (h->prior_forked) HIPCHK(hipStreamWaitEvent(s, h->ev_side, 0));   // join the Cholesky of the prior
    int rc = ORCVIO_OK;
    for (int st = ST_FORM_U; st < ST_COUNT && rc == ORCVIO_OK; ++st) rc = launch_solve_stage(h, s, st, c);
    return rc;
}

static hipStream_t pick_stream(orcvio_msckf_handle* h, void* stream) { return stream ? (hipStream_t)stream : h->stream; }

// ---- launch graphs ------------------------------------------------------------------------------------
// A sequence of launches can be replayed from a captured hipGraph: same kernels, same arguments, fewer host calls and
// tighter dispatch.  Capturing costs several hundred microseconds, so a slot captures only when the same launch
// signature (sizes, flags, options, pointers, stream) shows up twice in a row -- a caller that replays one shape (the
// benchmark, a fixed-size window) gets the graph, a caller whose track count changes every frame gets plain launches.
static unsigned long long launch_signature(const orcvio_msckf_handle* h, hipStream_t s, const void* p0, long extra, const UpdateCall& c) {
    unsigned long long sig = 1469598103934665603ull;
    auto mix = [&](unsigned long long v) { sig = (sig ^ v) * 1099511628211ull; };
    mix(h->N); mix(h->F); mix(h->nobs); mix(h->m_tot); mix(h->thin_opt); mix(h->Mmax); mix(h->chunks); mix(h->s_chunks); mix(h->rows_per_chunk);
    mix(h->flags.leg_dim); mix(h->flags.use_larvio); mix(h->flags.use_left_perturbation); mix(h->flags.if_fej);
    mix(h->flags.estimate_td); mix(h->materialize); mix(h->skip_active); mix(h->fused_solve); mix(h->la_solve); mix(h->la_spin); mix(h->fuse_finish); mix(c.fin_frame); mix(h->front_fused); mix(h->front_blocked_by_comm); mix(h->feat_ablate); mix(h->ekf_F); mix(h->ekf_mode); mix(h->n_extra); mix(h->n_nui); mix(h->dense_rows);
    unsigned long long bits;
    double sg = h->flags.noise_feature;
    std::memcpy(&bits, &sg, 8); mix(bits);
    double cp = h->flags.chi2_prob;
    std::memcpy(&bits, &cp, 8); mix(bits);
    mix(c.retry_forked); mix(h->front_spin_limit); mix(h->use_factor); mix(h->kf); mix(h->fac_ld); mix(h->graph_epoch); mix(h->ekf_idp); mix(h->ekf_eval); mix(h->ekf_cap); mix(h->dense_cap);
    mix((unsigned long long)(size_t)h->d_ekf_i); mix((unsigned long long)(size_t)h->d_ekf_d); mix((unsigned long long)(size_t)h->d_ekf_E);
    mix((unsigned long long)(size_t)h->d_slam); mix((unsigned long long)(size_t)h->d_dense); mix((unsigned long long)(size_t)h->d_Gekf);
    mix((unsigned long long)(size_t)h->d_Hs); mix((unsigned long long)(size_t)h->d_P);
    // the resident square-root factor is double-buffered and every user of it is a captured kernel argument (prior_factor):
    // its address belongs to the signature (ADVICE r2, high: a same-shape update after cov_commit replayed the OTHER buffer)
    mix(h->use_factor ? (unsigned long long)(size_t)h->d_Sres : 0ull);
    mix(h->tail); mix(rev_prior_active(h));
    mix((unsigned long long)(size_t)s); mix((unsigned long long)(size_t)p0); mix((unsigned long long)extra);
    // k_front's list pointers are captured: the arena's (lists_in_place_active) or the HBM copy's.  A sequence that has to pull a stale
    // HBM copy first (lists_refresh) gets NO signature -- plain launches, once: that pull is not part of the sequence's graph
    const bool in_place = lists_in_place_active(h, c);
    mix(in_place);
    if (!in_place && h->lists_stale) return 0ull;
    return sig;
}

static int run_with_graph(orcvio_msckf_handle* h, orcvio_msckf_handle::GraphSlot& slot, unsigned long long sig, hipStream_t s,
                          const std::function<int(bool)>& enqueue) {
    typedef orcvio_msckf_handle::GraphSlot::Way Way;
    if (h->use_graph && s != nullptr) {
        Way* hit = nullptr;
        for (Way& w : slot.way)
            if (w.exec && w.sig == sig) { hit = &w; break; }
        if (!hit) {
            bool seen = false;
            for (unsigned long long v : slot.seen) seen = seen || (v == sig && sig != 0);
            if (seen) {   // second time: capture into a free way, or over the least recently used one
                Way* dst = &slot.way[0];
                for (Way& w : slot.way) {
                    if (!w.exec) { dst = &w; break; }
                    if (w.used < dst->used) dst = &w;
                }
                if (dst->exec) { (void)hipGraphExecDestroy(dst->exec); dst->exec = nullptr; }
                if (dst->graph) { (void)hipGraphDestroy(dst->graph); dst->graph = nullptr; }
                if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess) {
                    const int rc_c = enqueue(true);
                    hipGraph_t g = nullptr;
                    const hipError_t e_end = hipStreamEndCapture(s, &g);
                    if (rc_c == ORCVIO_OK && e_end == hipSuccess && g && hipGraphInstantiate(&dst->exec, g, nullptr, nullptr, 0) == hipSuccess) {
                        dst->graph = g;
                        dst->sig = sig;
                        hit = dst;
                        h->cnt_graph_captures++;
                    } else {
                        if (g) (void)hipGraphDestroy(g);
                        dst->exec = nullptr;
                        (void)hipGetLastError();
                        h->use_graph = false;   // capture is not available here: plain launches from now on
                    }
                } else {
                    (void)hipGetLastError();
                    h->use_graph = false;
                }
            } else {
                slot.seen[slot.seen_at] = sig;
                slot.seen_at = (slot.seen_at + 1) & 7;
            }
        }
        if (hit) {
            hit->used = ++slot.tick;
            HIPCHK(hipGraphLaunch(hit->exec, s));
            h->cnt_graph_replays++;
            return ORCVIO_OK;
        }
    }
    h->cnt_plain_runs++;
    return enqueue(false);
}

// this rank's part of a sharded update: the Cholesky of the prior goes to the side stream with plain launches (it is
// joined by run_finish, so it overlaps the feature kernels AND the collective), the rest replays from a graph
static int run_local_impl(orcvio_msckf_handle* h, hipStream_t s, double* dst) {
    h->last_stream = s;
    { const int re = launch_ekf(h, s); if (re != ORCVIO_OK) return re; }
    UpdateCall c;
    if (front_fused_active(h, c.retry_forked)) { h->prior_forked = false; return launch_front(h, s, c, dst); }   // one launch: tracks, compression, and the prior's factor
    int rc = launch_prior_fork(h, s);
    if (rc != ORCVIO_OK) return rc;
    return run_with_graph(h, h->g_local, launch_signature(h, s, dst, 0, c), s, [&](bool) {
        int r = launch_feature(h, s);
        if (r == ORCVIO_OK) r = launch_gram(h, s);
        if (r == ORCVIO_OK) r = launch_assemble(h, s, dst);
        return r;
    });
}

int32_t orcvio_msckf_run_local(orcvio_msckf_handle* h, void* stream) {
    if (!h || !h->uploaded || h->pw_missing) { g_last_error = "run_local: nothing uploaded (or positions missing)"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    return run_local_impl(h, pick_stream(h, stream), h->d_Ab);
}

int32_t orcvio_msckf_run_local_to(orcvio_msckf_handle* h, double* d_dst, void* stream) {
    if (!h || !h->uploaded || !d_dst || h->pw_missing) { g_last_error = "run_local_to: invalid"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    return run_local_impl(h, pick_stream(h, stream), d_dst);
}

int32_t orcvio_msckf_block_ptr(orcvio_msckf_handle* h, double** d_block, int64_t* n_elems) {
    if (!h || !h->uploaded || !d_block || !n_elems) { g_last_error = "block_ptr: invalid"; return ORCVIO_ERR_INVALID; }
    *d_block = h->d_Ab;
    *n_elems = (int64_t)h->NAP * h->NAP;
    return ORCVIO_OK;
}

static int run_finish_impl(orcvio_msckf_handle* h, const double* d_blocks, int n_blocks, size_t stride, const double* meta0, hipStream_t s) {
    h->last_stream = s;
    if (h->dl_pending) { HIPCHK(hipStreamSynchronize(h->dl_stream)); h->dl_pending = false; }
    // the Cholesky of the prior was forked by run_local: join it here (outside the captured part)
    if (h->prior_forked) HIPCHK(hipStreamWaitEvent(s, h->ev_side, 0));
    h->A_deferred = false;   // d_A is the sum of the gathered blocks
    UpdateCall c;
    unsigned long long sig = launch_signature(h, s, d_blocks, n_blocks, c);
    sig = (sig ^ (unsigned long long)stride) * 1099511628211ull;
    sig = (sig ^ (unsigned long long)(size_t)meta0) * 1099511628211ull;
    int rc = run_with_graph(h, h->g_finish, sig, s, [&](bool) {
        int r = launch_reduce(h, s, d_blocks, n_blocks, h->d_A, stride, meta0);   // rank-ordered sum of the gathered blocks
        for (int st = ST_FORM_U; st < ST_COUNT && r == ORCVIO_OK; ++st) r = launch_solve_stage(h, s, st, c);
        return r;
    });
    if (rc == ORCVIO_OK) mark_update_enqueued(h, 1);
    return rc;
}

int32_t orcvio_msckf_run_finish(orcvio_msckf_handle* h, const double* d_blocks, int32_t n_blocks, void* stream) {
    if (!h || !h->uploaded || !d_blocks || n_blocks < 1) { g_last_error = "run_finish: invalid"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    return run_finish_impl(h, d_blocks, n_blocks, 0, nullptr, pick_stream(h, stream));
}

// EKF-SLAM rows of this upload: gate every feature against the prior (2 degrees of freedom), accepted rows -> dense
// [H | r] rows -> their Gram, which assembly adds to the compressed block (ekf_rows.hpp)
static int launch_ekf(orcvio_msckf_handle* h, hipStream_t s) {
    if (h->ekf_F <= 0 && h->dense_rows <= 0) return ORCVIO_OK;
    const int F = h->ekf_F, cap = h->ekf_cap;
    const int nb = h->NAP / 16, ntiles = nb * (nb + 1) / 2;
    if (F > 0) {
        EkfEvalArgs e{};
        if (h->ekf_eval) {   // measurementJacobian_ekf_{3,1}didp on the device: the compact row blocks from the SLAM features
            e.F = F; e.idp_dim = h->ekf_idp; e.if_fej = h->flags.if_fej; e.poses = h->d_poses;
            e.anchor = h->d_ekf_i; e.state = h->d_ekf_i + cap;
            e.param = h->d_slam; e.inv_depth = e.param + (size_t)3 * cap; e.p_w = e.inv_depth + cap; e.p_fej = e.p_w + (size_t)3 * cap;
            e.z = e.p_fej + (size_t)3 * cap;
            e.He = h->d_ekf_d; e.Ha = e.He + (size_t)12 * cap; e.Hx = e.Ha + (size_t)12 * cap; e.Hf = e.Hx + (size_t)12 * cap;
            e.r = e.Hf + (size_t)6 * cap + (size_t)2 * cap;
        }
        EkfGateArgs a;
        a.F = F; a.idp_dim = h->ekf_idp; a.n = h->n; a.leg = h->flags.leg_dim; a.N = h->N; a.NA = h->NA; a.NAP = h->NAP;
        a.estimate_td = h->flags.estimate_td; a.n_nui = h->n_nui;
        a.anchor = h->d_ekf_i; a.state = h->d_ekf_i + cap; a.slot = h->d_ekf_i + 2 * cap;
        a.He = h->d_ekf_d; a.Ha = a.He + (size_t)12 * cap; a.Hx = a.Ha + (size_t)12 * cap; a.Hf = a.Hx + (size_t)12 * cap;
        a.zvel = a.Hf + (size_t)6 * cap; a.r = a.zvel + (size_t)2 * cap;
        a.P = h->d_P; a.sigma2 = h->flags.noise_feature * h->flags.noise_feature;
        a.threshold = orcvio_msckf_chi2_quantile(2, h->flags.chi2_prob);
        a.E = h->d_ekf_E; a.gamma = h->d_ekf_gamma; a.accept = h->d_ekf_accept;
        if (h->ekf_one_launch) {   // a wavefront per feature: evaluation, fill and gate in ONE launch (frame_ops.hpp)
            hipLaunchKernelGGL(k_ekf_evalgate, dim3(F), dim3(64), 0, s, e, h->ekf_eval ? 1 : 0, a, (const int*)(s == h->side ? h->d_info + 8 : nullptr));
        } else {
            HIPCHK(hipMemsetAsync(h->d_ekf_E, 0, sizeof(double) * (size_t)2 * F * h->NAP, s));
            if (h->ekf_eval) hipLaunchKernelGGL(k_ekf_eval, dim3((F + 63) / 64), dim3(64), 0, s, e);
            hipLaunchKernelGGL(k_ekf_gate, dim3(F), dim3(64), 0, s, a);
        }
        hipLaunchKernelGGL(k_gram, dim3((ntiles + 3) / 4, 1), dim3(256), 0, s, (const double*)h->d_ekf_E, 2 * F, h->NAP, round_up(2 * F, 8),
                           h->d_Gekf, (const int*)nullptr);
    }
    if (h->dense_rows > 0) {   // their Gram into the scratch behind d_Gekf, then summed (fixed order)
        double* G2 = h->d_Gekf + (size_t)h->NAP_max * h->NAP_max;
        hipLaunchKernelGGL(k_gram, dim3((ntiles + 3) / 4, 1), dim3(256), 0, s, (const double*)h->d_dense, h->dense_rows, h->NAP,
                           round_up(h->dense_rows, 8), F > 0 ? G2 : h->d_Gekf, (const int*)nullptr);
        if (F > 0) {
            const int total = h->NAP * h->NAP;
            hipLaunchKernelGGL(k_add_inplace, dim3((total + 255) / 256), dim3(256), 0, s, h->d_Gekf, (const double*)G2, total);
        }
    }
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// mid: called once the tracks' launch is out (fused front end only) -- the frame call enqueues its objects' compression there, so that
// it is on its way before the host spends its time on the feature update's remaining launches
// A stack of at most THIN_MAX_ROWS projected rows (pruneImuStateBuffer's update: one row per feature seen in both clones that leave):
// the reference's direct form, S = H P H^T + s2 I of dimension m, instead of the square-root form of dimension n (frame_ops.hpp).
// Only where the finish is k_finish_pub's (the in-place paths: io_update / io_submit / io_step_frame without P+ to the host) -- the
// commit and the publication ride in k_thin_apply the same way.
static inline bool thin_possible(const orcvio_msckf_handle* h, const UpdateCall& c) {
    return h->thin_opt && !c.thin_blocked &&h->F > 0 && h->m_tot > 0 && h->m_tot <= THIN_MAX_ROWS && h->ekf_F == 0 && h->dense_rows == 0 && h->n_nui == 0 &&
           !h->objects_mode && !h->materialize && h->feat_ablate == 0 && (h->NAP + 63) / 64 <= 7 &&
           sizeof(double) * thin_gain_lds_doubles(h->m_tot, h->NA, h->n) <= (size_t)150 * 1024;   // (k_thin_gain is ONE workgroup: everything in its LDS)
}
static int enqueue_thin(orcvio_msckf_handle* h, hipStream_t s, const FinishPubArgs& fp) {
    const int n = h->n, NA = h->NA, m = h->m_tot;
    // the tracks, with the projected rows of the accepted ones materialised (zero rows for the others) into the thin stack
    double* keep_Hs = h->d_Hs;
    h->d_Hs = h->d_Hthin; h->materialize = true;
    int rc = launch_feature(h, s);
    h->d_Hs = keep_Hs; h->materialize = false;
    if (rc != ORCVIO_OK) return rc;
    ThinGainArgs g{h->d_Hthin, m, h->NAP, NA, n, h->d_P, h->flags.noise_feature * h->flags.noise_feature, h->d_Vthin, h->d_uthin, h->d_info};
    const size_t lds = sizeof(double) * thin_gain_lds_doubles(m, NA, n);
    {
        static bool attr_set = false;
        if (!attr_set) { HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_thin_gain), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(152 * 1024))); attr_set = true; }
    }
    hipLaunchKernelGGL(k_thin_gain, dim3(1), dim3(1024), lds, s, g);
    ThinApplyArgs a{h->d_Vthin, h->d_uthin, m, n, h->d_P, fp.P_dst, h->d_dx, fp.commit, fp.info, fp.info_also,
                    fp.small_src, fp.small_dst, fp.small16, fp.counter, fp.seq, fp.flag};
    hipLaunchKernelGGL(k_thin_apply, dim3((n * n + n + 255) / 256), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    h->A_deferred = false; h->prior_forked = false;
    h->last_update_thin = true;
    return ORCVIO_OK;
}

static int enqueue_update(orcvio_msckf_handle* h, hipStream_t s, UpdateCall& c) {
    const std::function<int()>* mid = c.mid;
    h->last_update_thin = false;
    c.asm_wait = nullptr; c.front_mark = nullptr;
    if (c.fin_pub && !mid && thin_possible(h, c)) return enqueue_thin(h, s, c.pub);
    // The frame call's first update: the in-state features' rows and their Gram need the frame head's covariance and nothing of k_front,
    // and only the assembly behind k_front needs them -- they run on the side stream while k_front does, joined by two polled words
    // instead of stream-level events (a one-word launch is 2-5 us of stream time, a cross-queue event dependency 8).  Their launches go
    // out BEHIND k_front's: a wait enqueued ahead of what it waits for would stall a hardware queue the two streams happen to share (the
    // runtime maps any number of streams onto a few), and the host's time for four launches would stand in front of k_front.
    const bool ekf_side = c.ekf_side && h->ekf_side_opt && h->cnt_step_frames >= h->ekf_side_skip_until && !mid && h->ekf_F > 0 && h->dense_rows == 0 && h->ekf_one_launch && h->d_step_words &&
                          front_defers_assembly(h, c.retry_forked) && h->F > 0;
    unsigned* side_words = ekf_side ? reinterpret_cast<unsigned*>(h->d_step_words) + 32 : nullptr;
    if (ekf_side) { c.front_mark = side_words; c.front_mark_val = ++h->ekf_side_seq; }
    else { const int re = launch_ekf(h, s); if (re != ORCVIO_OK) return re; }
    // (the other way round -- prior on the origin stream, feature branch forked -- measured 15 us slower)
    h->A_deferred = front_defers_assembly(h, c.retry_forked);
    if (front_fused_active(h, c.retry_forked)) {   // one stream, no fork: the prior is factored by workgroup 0 of the feature launch
        // ... and the compression behind the tracks, under the factorisation
        h->prior_forked = false;
        int rc = launch_front(h, s, c, h->d_A, h->A_deferred);
        if (rc == ORCVIO_OK && ekf_side) {
            const unsigned seq = h->ekf_side_seq;
            h->ekf_side_used = true;
            hipLaunchKernelGGL(k_wait_word, dim3(1), dim3(64), 0, h->side, (const unsigned*)side_words, seq, side_spin_limit(h), h->d_info + 8);
            rc = launch_ekf(h, h->side);
            hipLaunchKernelGGL(k_obj_done, dim3(1), dim3(64), 0, h->side, side_words + 1, seq);
            HIPCHK(hipGetLastError());
            c.asm_wait = side_words + 1; c.asm_wait_val = seq;
        }
        if (rc == ORCVIO_OK && mid) rc = (*mid)();
        for (int st = ST_FORM_U; st < ST_COUNT && rc == ORCVIO_OK; ++st) rc = launch_solve_stage(h, s, st, c);
        return rc;
    }
    if (mid) { const int rm = (*mid)(); if (rm != ORCVIO_OK) return rm; }
    int rc = launch_prior_fork(h, s);
    if (rc == ORCVIO_OK) rc = launch_feature(h, s);
    if (rc == ORCVIO_OK) rc = launch_gram(h, s);
    if (rc == ORCVIO_OK) rc = launch_assemble(h, s, h->d_A);
    if (rc == ORCVIO_OK) rc = launch_solve_tail(h, s, c);
    return rc;
}
