// capi_io.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// download, the zero-copy update (io_begin / io_update), the copying one-shot call, gate_tracks.

// ---- download --------------------------------------------------------------------------------
// Optional outputs in the reference's own terms (computed on the device, on request only):
//   H_thin = R_A (A = R_A^T R_A, zero rows on rank-deficient directions), r_thin = R_A^-T b,
//   K = P H_thin^T S^-1 = Lf M^-1 L_a^T R_A^T,   G = K H_thin = Lf M^-1 L_a^T A.
static int compute_optional(orcvio_msckf_handle* h, bool want_thin_or_K, bool want_K, bool want_G) {
    if (h->last_update_thin) { g_last_error = "H_thin / K / G are derived from the square-root path's factors: not available behind an update that took the direct form of a thin stack (ask for them in the update call itself)"; return ORCVIO_ERR_INVALID; }
    // (kf: the columns of the prior's factor that take part in M' -- the trailing h->tail ones are zero in the active rows, so
    //  U, W and the products below have nothing there)
    const int NA = h->NA, NAP = h->NAP, n = h->n, kf = h->kf - h->tail, NP = h->NP, ldz = h->ldz;
    hipStream_t s = h->stream;
    const PriorFactor pf = prior_factor(h);
    const long sLi = pf.sLi, sLj = pf.sLj;
    const double* La_P = pf.base + 15 * sLi;
    { const int ra = assemble_deferred(h, s); if (ra != ORCVIO_OK) return ra; }
    if (want_thin_or_K) {   // lower Cholesky factor of the Gram block with the LDS-panel kernel
        HIPCHK(hipMemcpyAsync(h->d_La, h->d_A, sizeof(double) * (size_t)NAP * NAP, hipMemcpyDeviceToDevice, s));
        // the Gram block is singular in every update (gauge freedom): factor A + 1e-11 max(diag) I, which needs no
        // rank decision and changes H_thin^T H_thin by 1e-11 relative
        hipLaunchKernelGGL(k_potrf, dim3(1), dim3(1024), 0, s, h->d_La, NA + 1, NAP, 0.0, h->d_DinvA, h->d_info + 4, 1e-11);
        HIPCHK(hipGetLastError());
    }
    if (want_G) {   // W = L_M^-1 U[0:NA]^T (n x NA);  G[:, 15:] = Zn^T W
        int rc = launch_trsm(h, s, h->d_RM, h->d_DinvM, kf, h->d_U, 1, NP, NA, nullptr, 0, h->d_W, NP);
        if (rc == ORCVIO_OK) rc = launch_gemm(s, h->d_Z, 1, ldz, h->d_W, NP, 1, n, NA, kf, 1.0, 0.0, 0, h->d_KG, NP, 1);
        if (rc != ORCVIO_OK) return rc;
    }
    if (want_K) {   // Y = L_a^T R_A^T (n x NA); W = L_M^-1 Y; K = Zn^T W  -> stored after G in d_KG
        int rc = launch_gemm(s, La_P, sLj, sLi, h->d_La, NAP, 1, kf, NA, NA, 1.0, 0.0, 0, h->d_Y, NP, 1);
        if (rc == ORCVIO_OK) rc = launch_trsm(h, s, h->d_RM, h->d_DinvM, kf, h->d_Y, NP, 1, NA, nullptr, 0, h->d_W, NP);
        if (rc == ORCVIO_OK) rc = launch_gemm(s, h->d_Z, 1, ldz, h->d_W, NP, 1, n, NA, kf, 1.0, 0.0, 0, h->d_Y, NP, 1);
        if (rc != ORCVIO_OK) return rc;
    }
    HIPCHK(hipStreamSynchronize(s));
    return ORCVIO_OK;
}

// Device -> host copy of the outputs arena ([info | dx | gamma | accept], with P+ behind it if wanted) into the pinned
// mirror, enqueued on `sd` behind the update: ONE copy.  download() waits for it (or issues it itself).
static int download_enqueue(orcvio_msckf_handle* h, hipStream_t sd, bool with_P) {
    const size_t bytes = with_P ? h->oo_Pout + sizeof(double) * (size_t)h->n * h->n : h->outs_small;
    HIPCHK(hipMemcpyAsync(h->h_stage + h->in_cap + h->out_shift, h->d_outs, bytes, hipMemcpyDeviceToHost, sd));
    h->dl_pending = true; h->dl_with_P = with_P; h->dl_stream = sd;
    return ORCVIO_OK;
}

// An update whose in-launch hand-off was lost, run again on the forked path (plain launches, no in-launch device-wide wait, the
// one-workgroup factorisation + solve) on what is uploaded already, with the copy of its results behind it
static int rerun_forked(orcvio_msckf_handle* h, hipStream_t s, bool want_P) {
    UpdateCall c;
    c.retry_forked = true;
    int rr = run_update_impl(h, s, c);
    if (rr == ORCVIO_OK) rr = download_enqueue(h, s ? s : h->stream, want_P);
    return rr;
}

// retried: this is the look at the results of the repeat
static int download_impl(orcvio_msckf_handle* h, orcvio_msckf_result* res, bool retried) {
    if (!h || !res || !h->ran) { g_last_error = "download: no finished update"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    const int n = h->n, NA = h->NA, NAP = h->NAP, NP = h->NP, F = h->F;
    const bool want_P = res->P_out != nullptr;
    if (!(h->dl_pending && (h->dl_with_P || !want_P))) {   // not enqueued behind the update (staged callers), or without P+
        hipStream_t sd = h->last_stream ? h->last_stream : h->stream;
        if (h->dl_pending) HIPCHK(hipStreamSynchronize(h->dl_stream));
        HIPCHK(hipStreamSynchronize(h->side));
        const int rq = download_enqueue(h, sd, want_P);
        if (rq != ORCVIO_OK) return rq;
    }
    HIPCHK(hipStreamSynchronize(h->dl_stream));
    h->dl_pending = false;
    if (h->last_sharded) {   // (ipc transport: a polling wavefront that gave up waiting for a peer's block leaves a word behind)
        const int rl = ipc_check_lost(h, "orcvio_msckf_download");
        if (rl != ORCVIO_OK) return rl;
    }
    const char* so = h->h_stage + h->in_cap;
    const double* dx = reinterpret_cast<const double*>(so + h->oo_dx);
    const double* gam = reinterpret_cast<const double*>(so + h->oo_gamma);
    const int* acc = reinterpret_cast<const int*>(so + h->oo_accept);
    if (res->dx) std::memcpy(res->dx, dx, sizeof(double) * n);
    if (res->P_out) std::memcpy(res->P_out, so + h->oo_Pout, sizeof(double) * (size_t)n * n);
    if (res->accept && F > 0) std::memcpy(res->accept, acc, sizeof(int) * F);
    if (res->gamma && F > 0) std::memcpy(res->gamma, gam, sizeof(double) * F);
    int info[16] = {0};
    std::memcpy(info, so, sizeof(int) * 16);
    if (info[8] != 0) {   // a wait inside a launch gave up: a workgroup of k_front at its device-wide counter (somebody else's kernel
                          // held CUs it needed), or a solver wavefront of k_potrf_solve
        const bool again = h->last_run_kind == 0 && !retried;   // single-GPU update: run it again inside this call
        { const int rh = handoff_reset(h, again); if (rh != ORCVIO_OK) return rh; }
        if (again) {
            const int rr = rerun_forked(h, h->last_stream, want_P);
            if (rr != ORCVIO_OK) return rr;
            return download_impl(h, res, true);   // (a second time-out in the forked form is reported as an error below)
        }
        // the solve ran through on stale bytes: nothing of this update may be committed (ADVICE r2)
        h->ran = false;
        g_last_error = "k_potrf_solve / k_front: an in-launch hand-off timed out";
        return ORCVIO_ERR_TIMEOUT;
    }
    if (h->last_sharded && info[9] != 0) {   // sharded update: another rank took part with an empty share and a status word
        h->ran = false;                            // (no rank commits: every rank returns an error)
        g_last_error = "sharded update: rank " + std::to_string(info[9] - 1) + " could not take part with its tracks (status " + std::to_string(info[10]) + ")";
        return ORCVIO_ERR_PEER;
    }
    {
        const int ro = feature_outcome(h, so, res->stats);
        if (ro != ORCVIO_OK) return ro;
    }
    if (h->last_sharded) {   // the joint update is applied whenever ANY rank stacked rows (the gathered status words)
        res->stats[1] = info[12] > 0 ? NA : 0;
        res->stats[3] = info[12] > 0 ? 1 : 0;
    }
    const bool want_thin = res->H_thin || res->r_thin;
    if (want_thin || res->K || res->G) {
        int rc = compute_optional(h, want_thin || res->K, res->K != nullptr, res->G != nullptr);
        if (rc != ORCVIO_OK) return rc;
        if (want_thin) {
            std::vector<double> La((size_t)NAP * NAP);
            HIPCHK(hipMemcpy(La.data(), h->d_La, sizeof(double) * La.size(), hipMemcpyDeviceToHost));
            if (res->H_thin) {
                std::memset(res->H_thin, 0, sizeof(double) * (size_t)NA * n);
                for (int i = 0; i < NA; ++i)
                    for (int k = i; k < NA; ++k) res->H_thin[(size_t)i * n + 15 + k] = La[(size_t)k * NAP + i];
            }
            if (res->r_thin)
                for (int i = 0; i < NA; ++i) res->r_thin[i] = La[(size_t)NA * NAP + i];
        }
        if (res->G) {
            std::vector<double> Gd((size_t)n * NP);
            HIPCHK(hipMemcpy(Gd.data(), h->d_KG, sizeof(double) * Gd.size(), hipMemcpyDeviceToHost));
            std::memset(res->G, 0, sizeof(double) * (size_t)n * n);
            for (int i = 0; i < n; ++i)
                for (int c = 0; c < NA; ++c) res->G[(size_t)i * n + 15 + c] = Gd[(size_t)i * NP + c];
        }
        if (res->K) {
            std::vector<double> Kd((size_t)n * NP);
            HIPCHK(hipMemcpy(Kd.data(), h->d_Y, sizeof(double) * Kd.size(), hipMemcpyDeviceToHost));
            for (int i = 0; i < n; ++i)
                for (int c = 0; c < NA; ++c) res->K[(size_t)i * NA + c] = Kd[(size_t)i * NP + c];
        }
    }
    return ORCVIO_OK;
}
int32_t orcvio_msckf_download(orcvio_msckf_handle* h, orcvio_msckf_result* res) { return download_impl(h, res, false); }

// ---- the zero-copy update (orcvio_msckf_io_begin / _io_update; the copying one-shot calls run on it too) ----------------------
// ONE graph launch per update: k_ingest (pinned arena -> HBM) -> the update's kernels -> k_epilogue (results -> host-coherent
// memory, [the commit of P+ and its square-root factor], then the flag).  No copy-engine transfer, no stream
// synchronisation: the calling thread spins on the flag.
static int launch_triangulate(orcvio_msckf_handle* h, const orcvio_triangulation_config* cfg, bool have_init, bool mark_skip, hipStream_t s,
                              bool io, bool with_mode, bool prune, int* raise);   // (capi_state.inc)
// An update armed by orcvio_msckf_io_triangulate: from here on it runs as behind orcvio_msckf_triangulate_uploaded (d_skip is read by
// every form of the front end).  Called behind upload_finalize, which resets both words; the arming is consumed.
static inline void tri_consume(orcvio_msckf_handle* h, UpdateCall& c) {
    if (!h->tri_armed) return;
    h->tri_armed = false;
    c.tri = true;
    h->skip_active = true; h->tri_live = true;
    // nothing but the tracks in this update: without a single valid one it is refused on the device the way a refused first update
    // refuses the frame's second (info_also: P and its factor stay, bit for bit) -- and is no error: stats[3] = 0
    h->tri_refuse_empty = h->F > 0 && h->ekf_F == 0 && h->dense_rows == 0 && h->new_F == 0 && !c.info_also;
    if (h->tri_refuse_empty) c.info_also = h->d_tri_words;
}
// The frame's second update armed by orcvio_msckf_io_triangulate_prune (behind upload_finalize on the swapped-in second arena; the frame
// call has taken the arming).  The prune update has nothing but its tracks, so it always refuses itself without a valid one -- and its
// commit already reads the frame's kept status words (info_also): the launch RAISES word [2] of those instead of taking info_also over,
// so that both refusals reach the commit (io_enqueue).  The repair path keeps no words: it reads the launch's own block (io_run_forked).
static inline void tri_consume_prune(orcvio_msckf_handle* h, UpdateCall& c) {
    c.tri = true; c.tri_prune = true;
    h->skip_active = true; h->tri_live = true; h->tri_live_prune = true;
    h->tri_refuse_empty = h->F > 0;
}
static unsigned long long io_signature(const orcvio_msckf_handle* h, hipStream_t s, bool want_P, bool commit, const UpdateCall& c, bool finpub = false) {
    unsigned long long sig = launch_signature(h, s, h->h_stage_dev, (long)(0x100 | (want_P ? 1 : 0) | (commit ? 2 : 0) | (finpub ? 4 : 0)), c);
    auto mix = [&](unsigned long long v) { sig = (sig ^ v) * 1099511628211ull; };
    mix((unsigned long long)upload_bytes(h)); mix((unsigned long long)h->io_poses); mix((unsigned long long)(size_t)h->d_Stmp); mix((unsigned long long)(size_t)h->d_Pres);
    mix(h->factor_opt); mix((unsigned long long)h->outs_small); mix((unsigned long long)(size_t)h->d_Ptmp); mix(h->finpub_opt);
    mix(c.tri); mix(h->tri_live);
    if (c.tri) {   // (a captured k_triangulate has the config by value and the mode pointer frozen in it)
        const orcvio_triangulation_config& t = h->tri_cfg;
        const double d[6] = {t.translation_threshold, t.huber_epsilon, t.estimation_precision, t.initial_damping, t.cost_threshold, t.init_final_dist_threshold};
        for (double v : d) { unsigned long long bits; std::memcpy(&bits, &v, 8); mix(bits); }
        mix((unsigned long long)t.outer_loop_max_iteration); mix((unsigned long long)t.inner_loop_max_iteration);
        mix(h->tri_with_mode); mix((unsigned long long)(size_t)h->h_tri_dev); mix((unsigned long long)(size_t)c.info_also);
    }
    mix(c.tri_prune);
    return sig;
}

// sixteen status words of a frame's first update, kept on the device for the second update's commit (EpilogueArgs.info_also)
static int step_words(orcvio_msckf_handle* h) {
    if (h->d_step_words) return ORCVIO_OK;
    HIPCHK(hipMalloc(&h->d_step_words, 256));
    HIPCHK(hipMemset(h->d_step_words, 0, 256));
    return ORCVIO_OK;
}

// k_finish_sqrt + k_epilogue as ONE launch (k_finish_pub): feature updates on the in-place paths whose finish is a launch of its own
static inline bool finpub_active(const orcvio_msckf_handle* h, const UpdateCall& c) {
    return h->finpub_opt && !h->objects_mode && h->n_nui == 0 && !finish_fused_active(h, c);
}
static int io_enqueue(orcvio_msckf_handle* h, hipStream_t s, bool want_P, bool commit, UpdateCall& c, bool allow_finpub = false) {
    const int mode = commit ? (h->factor_opt && h->n_nui == 0 ? 2 : 1) : 0;
    const SolveOut so = solve_out(h);
    c.fin_pub = allow_finpub && finpub_active(h, c) && !want_P;   // (P+ to the host: k_finish_sqrt + k_epilogue's copy workgroups are faster, profiles/r6a)
    if (c.fin_pub) c.pub = finish_pub_args(h, so, mode, c.info_also);
    h->last_finpub_commit = c.fin_pub && commit;
    // inputs: the derived index arrays at the head of the arena (the caller-written part behind them went ahead: ingest_raw)
    int rc = ORCVIO_OK;
    // (the repeat of an armed update -- tri_live without c.tri -- pulls no more either: the positions in HBM are the device's own)
    // (... and none where k_front reads the lists in the arena itself: lists_in_place_active -- the HBM copy is then an earlier upload's)
    const bool in_place = lists_in_place_active(h, c);
    if (!c.already_ingested && !in_place) rc = launch_ingest(h, s, h->h_stage_dev, h->d_in, h->io_poses);
    if (!in_place) h->lists_stale = false;   // (the whole head has travelled: this node, or k_frame_head)
    // the armed update's triangulation: ONE launch behind the pull of the arena, in front of the first kernel that reads p_w or d_skip
    if (rc == ORCVIO_OK && c.tri && !c.tri_prune) rc = launch_triangulate(h, &h->tri_cfg, false, true, s, true, h->tri_with_mode, false, nullptr);
    // ... the prune update's, out of its own list: behind the pose step and the pull, with the frame's kept status words to raise
    if (rc == ORCVIO_OK && c.tri_prune) rc = launch_triangulate(h, &h->tri2_cfg, false, true, s, true, true, true, c.retry_forked ? nullptr : h->d_step_words + 2);
    if (rc == ORCVIO_OK) rc = enqueue_update(h, s, c);
    if (rc != ORCVIO_OK || c.fin_pub) return rc;
    // ONE launch behind the update: the results to host-coherent memory, the commit (refused on the device if the update is),
    // and the flag the caller waits on (k_epilogue)
    return launch_epilogue(s, epilogue_args(h, so, 0, want_P, mode, nullptr, c.info_also, c.info_keep));
}

// Wait for the next publication: spin on the host-coherent flag (bounded), then fall back to a stream synchronisation.
static int io_wait(orcvio_msckf_handle* h, hipStream_t s, unsigned long long expected_pub) {
    // (the latest publication on the stream: earlier ones nobody waited for are covered; the frame call waits for its feature half
    //  with the count it noted when it launched that half, its object half's publication being enqueued behind it)
    const unsigned long long expected = expected_pub ? expected_pub : h->pub_enqueued;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    bool late = false;
    while (__atomic_load_n(h->h_flag, __ATOMIC_ACQUIRE) < expected) {
        _mm_pause();
        if ((++spins & 4095u) == 0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > h->io_spin_seconds) { late = true; break; }
    }
    if (late) {
        HIPCHK(hipStreamSynchronize(s));   // (the in-launch waits of the kernels are bounded: the stream drains)
        const unsigned long long now = __atomic_load_n(h->h_flag, __ATOMIC_ACQUIRE);
        if (now < expected) {
            h->pub_enqueued = now;   // (the stream has drained: a launch that never ran does not publish later either -- whichever publication was
                                     //  waited for; left ahead of the device's count, every later wait on this handle would time out, ADVICE r3)
            g_last_error = "io_update: the results were not published";
            return ORCVIO_ERR_TIMEOUT;
        }
    }
    return ORCVIO_OK;
}

// statistics and refusals of a finished feature update from the published small block (shared with orcvio_msckf_download)
// (what the outcome depends on besides the published block: orcvio_msckf_io_update_frame keeps a copy while the object update
//  that follows in the same call re-uses the handle's fields)
struct FeatureView { int n, F, NA; size_t oo_dx, oo_gamma, oo_accept; const int* row_ptr; int discard_large_update; };
static inline FeatureView feature_view(const orcvio_msckf_handle* h) {
    return FeatureView{h->n, h->F, h->NA, h->oo_dx, h->oo_gamma, h->oo_accept, h->h_row_ptr.data(), h->flags.discard_large_update};
}
static int feature_outcome_view(orcvio_msckf_handle* h, const FeatureView& v, const char* so, int32_t* stats);
static int feature_outcome(orcvio_msckf_handle* h, const char* so, int32_t* stats) { return feature_outcome_view(h, feature_view(h), so, stats); }
static int feature_outcome_view(orcvio_msckf_handle* h, const FeatureView& v, const char* so, int32_t* stats) {
    const int n = v.n, F = v.F;
    const double* dx = reinterpret_cast<const double*>(so + v.oo_dx);
    const int* acc = reinterpret_cast<const int*>(so + v.oo_accept);
    const int* info = reinterpret_cast<const int*>(so);
    int stacked = 0, nacc = 0;
    const int* row_ptr = v.row_ptr;
    for (int j = 0; j < F; ++j)
        if (acc[j]) { stacked += row_ptr[j + 1] - row_ptr[j]; ++nacc; }
    if (stats) {
        std::memset(stats, 0, sizeof(int32_t) * 8);
        stats[0] = stacked;
        stats[1] = stacked > 0 ? v.NA : 0;
        stats[2] = nacc;
        stats[3] = stacked > 0 ? 1 : 0;
        if (v.discard_large_update) {
            const double nv = std::sqrt(dx[3] * dx[3] + dx[4] * dx[4] + dx[5] * dx[5]);
            const double np = std::sqrt(dx[6] * dx[6] + dx[7] * dx[7] + dx[8] * dx[8]);
            stats[4] = (nv > 1.0 || np > 1.5) ? 1 : 0;   // src/orcvio.cpp:4479-4494
        }
        stats[5] = info[0];   // zero-variance directions of the prior (dropped pivots of chol(P))
        stats[6] = info[1];   // pivots of chol(P) below -tol: the prior was not PSD
    }
    if (info[2] != 0 || info[3] != 0) {   // the device left P and x alone (k_finish_sqrt: P+ = P, dx = 0); the resident covariance is intact
        h->ran = false;                    // (nothing to commit)
        g_last_error = "M = s2 I + L^T A L is not positive definite (a prior beyond ~1e16 s2 in scale, or non-finite input): no update";
        return ORCVIO_ERR_NOT_SPD;
    }
    bool finite = true;
    for (int i = 0; i < n; ++i) finite = finite && std::isfinite(dx[i]);
    if (!finite) {   // NaN / Inf somewhere in the inputs (a NaN pivot does not show in the smallest pivot)
        h->ran = false;   // (cov_commit would make a non-finite P+ the resident covariance)
        g_last_error = "non-finite result (NaN / Inf in the prior, the poses or the noise): no update";
        return ORCVIO_ERR_NOT_SPD;
    }
    return ORCVIO_OK;
}

// the update on what stands in the arena (after upload_finalize), first half: ONE launch (captured graph or plain), nothing waited for
static int io_launch(orcvio_msckf_handle* h, bool want_P, bool commit, UpdateCall& c) {
    if (h->pw_missing) { g_last_error = "update: tracks were uploaded without positions and have not been triangulated"; return ORCVIO_ERR_INVALID; }
    hipStream_t s = h->stream;
    h->last_stream = s;
    if (h->dl_pending) { HIPCHK(hipStreamSynchronize(h->dl_stream)); h->dl_pending = false; }
    const bool finpub = finpub_active(h, c) && !want_P;
    c.io_single = true; c.fin_pub = finpub;   // (what io_enqueue is going to find: the predicate below is a function of the handle and this record)
    const bool in_place = lists_in_place_active(h, c);
    int rc = run_with_graph(h, h->g_io, io_signature(h, s, want_P, commit, c, finpub), s, [&](bool) { return io_enqueue(h, s, want_P, commit, c, true); });
    h->A_deferred = front_defers_assembly(h, c.retry_forked);   // (a replayed graph does not pass through enqueue_update)
    h->lists_stale = in_place;   // (... nor through io_enqueue: the launch has either pulled the three lists into HBM or read them in the arena)
    if (in_place && rc == ORCVIO_OK) h->cnt_lists_in_place++;
    h->last_finpub_commit = commit && finpub;   // (... nor through io_enqueue)
    h->last_update_thin = finpub && thin_possible(h, c);
    if (h->last_update_thin) h->A_deferred = false;
    if (rc != ORCVIO_OK) return rc;
    h->pub_enqueued++;   // (one k_epilogue per launch, captured or not)
    mark_update_enqueued(h, 0);
    // (the event stands behind the WHOLE launch: its ingest node at the head reads the arena, and so does k_front where it reads the
    //  derived lists in place -- its clone_ptr entries as late as the Gram items behind its device-wide barrier)
    return arena_mark_read(h, s);
}
// ... second half: the results are in the pinned output block when this returns
static int io_finish(orcvio_msckf_handle* h, bool want_P, bool commit, int32_t* stats);
static int io_run(orcvio_msckf_handle* h, bool want_P, bool commit, int32_t* stats, UpdateCall& c) {
    static PhaseTimer timer;   // diagnostics (ORCVIO_TIMING): the means of 64 calls
    PhaseTimer::Run tm = PhaseTimer::begin(&timer);
    int rc = io_launch(h, want_P, commit, c);
    if (rc != ORCVIO_OK) return rc;
    tm.mark(0);
    rc = io_finish(h, want_P, commit, stats);
    tm.mark(1);
    if (timer.due(64)) {
        fprintf(stderr, "io_run: launch %.1f us, wait + outcome %.1f us\n", timer.mean(0, 64), timer.mean(1, 64) - timer.mean(0, 64));
        timer.reset();
    }
    return rc;
}
// the committing update on what stands in the arena, run the safe way: the repeat of an update of a frame that lost an in-launch hand-off
static int io_run_forked(orcvio_msckf_handle* h, int32_t* stats) {
    UpdateCall c;
    c.retry_forked = true;
    if (h->tri_live && h->tri_refuse_empty) c.info_also = h->tri_live_prune ? h->d_tri2_words : h->d_tri_words;   // (the word of the attempt that triangulated stands)
    return io_run(h, false, true, stats, c);
}
static int io_finish(orcvio_msckf_handle* h, bool want_P, bool commit, int32_t* stats) {
    hipStream_t s = h->stream;
    int rc = io_wait(h, s);
    if (rc != ORCVIO_OK) { h->ran = false; return rc; }
    const char* so = h->h_stage + h->in_cap;
    const int* info = reinterpret_cast<const int*>(so);
    if (info[8] != 0) {
        // a workgroup of k_front gave up at its device-wide counter (somebody else's kernel held compute units it needed), or a
        // solver wavefront of k_potrf_solve: run the update again on the forked path (plain launches, no in-launch device-wide
        // wait), inside this call; the inputs are in HBM already.  The commit workgroups of the first attempt refuse themselves
        // on info[8] -- and may still be at it (the flag rises before they are done): the stream is drained before the word is cleared.
        HIPCHK(hipStreamSynchronize(s));
        int rr = handoff_reset(h);
        if (rr == ORCVIO_OK) rr = rerun_forked(h, s, want_P);
        if (rr != ORCVIO_OK) { h->ran = false; return rr; }
        HIPCHK(hipStreamSynchronize(s));
        h->dl_pending = false;
        if (info[8] != 0) {   // (the copy has refreshed the pinned block)
            HIPCHK(hipMemset(h->d_info + 8, 0, sizeof(int)));
            h->ran = false;
            g_last_error = "k_potrf_solve / k_front: an in-launch hand-off timed out twice";
            return ORCVIO_ERR_TIMEOUT;
        }
        rr = feature_outcome(h, so, stats);
        if (rr == ORCVIO_OK && commit) rr = orcvio_msckf_cov_commit(h);
        return rr;
    }
    rc = feature_outcome(h, so, stats);
    if (rc != ORCVIO_OK) return rc;
    // the kernels have written S+ into the spare factor buffer and P+ over the resident covariance (k_epilogue) or into the spare one (k_finish_pub)
    if (commit) commit_bookkeeping(h);
    return ORCVIO_OK;
}

int32_t orcvio_msckf_io_begin(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int32_t n_clones, int32_t n_features,
                              int32_t n_observations, int32_t with_P, orcvio_msckf_io* io) {
    if (!h || !flags || !io) { g_last_error = "io_begin: null argument"; return ORCVIO_ERR_INVALID; }
    if (with_P < 0 || with_P > 2) { g_last_error = "io_begin: with_P is 0, 1 or 2"; return ORCVIO_ERR_INVALID; }
    const int rc = upload_begin(h, flags, n_clones, n_features, n_observations, with_P == 1, true, "orcvio_msckf_io_begin", with_P == 2);
    if (rc != ORCVIO_OK) return rc;
    char* st = h->h_stage;
    io->n = h->n;
    io->poses = reinterpret_cast<double*>(st + h->io_poses);
    io->obs_ptr = reinterpret_cast<int32_t*>(st + h->io_optr);
    io->p_w = reinterpret_cast<double*>(st + h->io_pw);
    io->obs_clone = reinterpret_cast<int32_t*>(st + h->io_oclone);
    io->obs_z = reinterpret_cast<double*>(st + h->io_z);
    io->obs_zvel = h->io_zvel != h->io_z ? reinterpret_cast<double*>(st + h->io_zvel) : nullptr;
    io->P = with_P == 1 ? reinterpret_cast<double*>(st + h->io_P) : nullptr;
    const char* so = st + h->in_cap;
    io->dx = reinterpret_cast<const double*>(so + h->oo_dx);
    io->gamma = reinterpret_cast<const double*>(so + h->oo_gamma);
    io->accept = reinterpret_cast<const int32_t*>(so + h->oo_accept);
    io->P_out = reinterpret_cast<const double*>(so + h->oo_Pout);
    h->io_open = true;
    return ORCVIO_OK;
}

int32_t orcvio_msckf_io_update(orcvio_msckf_handle* h, int32_t want_P, int32_t commit, int32_t* stats) {
    if (!h || !h->io_open) { g_last_error = "io_update: call orcvio_msckf_io_begin first"; return ORCVIO_ERR_INVALID; }
    if (h->io_submitted) { g_last_error = "io_update: an update submitted with orcvio_msckf_io_submit has not been collected"; return ORCVIO_ERR_INVALID; }
    static PhaseTimer timer;   // diagnostics (ORCVIO_TIMING): the means of 64 calls
    PhaseTimer::Run tm = PhaseTimer::begin(&timer);
    HIPCHK(hipSetDevice(h->device));
    int rc = ingest_raw(h, h->stream);   // what the caller wrote travels while the host checks it
    if (rc != ORCVIO_OK) return rc;
    tm.mark(0);
    rc = upload_finalize(h, "orcvio_msckf_io_update");
    tm.mark(1);
    if (timer.due(64)) {
        fprintf(stderr, "io_update: set device %.1f us, finalize %.1f us\n", timer.mean(0, 64), timer.mean(1, 64) - timer.mean(0, 64));
        timer.reset();
    }
    if (rc != ORCVIO_OK) {   // (the arena keeps its layout: the caller may repair its arrays and call again -- once the early pull
                             //  of what it wrote, still in flight, has read the arena: the next writer waits for this event, ADVICE r3)
        (void)arena_mark_read(h, h->stream);
        return rc;
    }
    h->pw_missing = false;
    h->io_open = true;   // ... and may run the next update of the same shape without a new io_begin
    UpdateCall c;
    tri_consume(h, c);
    return io_run(h, want_P != 0, commit != 0, stats, c);
}

// orcvio_msckf_io_update in two halves: submit returns when the update has been LAUNCHED (the calling thread is free for ~0.1 ms:
// the front end's next image, the object mapper's results ..), collect waits for the flag word and reports the outcome.
int32_t orcvio_msckf_io_submit(orcvio_msckf_handle* h, int32_t want_P, int32_t commit) {
    if (!h || !h->io_open) { g_last_error = "io_submit: call orcvio_msckf_io_begin first"; return ORCVIO_ERR_INVALID; }
    if (h->io_submitted) { g_last_error = "io_submit: the previous submission has not been collected"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    int rc = ingest_raw(h, h->stream);
    if (rc == ORCVIO_OK) rc = upload_finalize(h, "orcvio_msckf_io_submit");
    if (rc != ORCVIO_OK) { (void)arena_mark_read(h, h->stream); return rc; }   // (the early pull may still be reading the arena)
    h->pw_missing = false;
    h->io_open = true;
    UpdateCall c;
    tri_consume(h, c);
    rc = io_launch(h, want_P != 0, commit != 0, c);
    if (rc != ORCVIO_OK) return rc;
    h->io_submitted = true; h->io_sub_P = want_P != 0; h->io_sub_commit = commit != 0;
    return ORCVIO_OK;
}
int32_t orcvio_msckf_io_collect(orcvio_msckf_handle* h, int32_t* stats) {
    if (!h || !h->io_submitted) { g_last_error = "io_collect: nothing submitted"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    h->io_submitted = false;
    return io_finish(h, h->io_sub_P, h->io_sub_commit, stats);
}

int32_t orcvio_msckf_update_features(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, const orcvio_msckf_window* window,
                                     const orcvio_msckf_tracks* tracks, const double* P, orcvio_msckf_result* result) {
    // the copying form of orcvio_msckf_io_begin / _io_update: the caller's arrays are copied into the arena, the results out of it
    static const bool timing = dbg_getenv("ORCVIO_TIMING") != nullptr;   // diagnostics: calls slower than 2 ms are broken down
    if (!result) { g_last_error = "update_features: null result"; return ORCVIO_ERR_INVALID; }
    const auto t0 = std::chrono::steady_clock::now();
    int rc = upload_to_arena(h, flags, window, tracks, P, "orcvio_msckf_update_features", true);
    if (rc != ORCVIO_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    const bool want_P = result->P_out != nullptr;
    UpdateCall c;
    c.thin_blocked = result->H_thin || result->r_thin || result->K || result->G;   // (derived from the general path's factors)
    rc = io_run(h, want_P, false, result->stats, c);
    const auto t3 = std::chrono::steady_clock::now();
    if (rc != ORCVIO_OK) return rc;
    const int n = h->n, F = h->F;
    const char* so = h->h_stage + h->in_cap;
    if (result->dx) std::memcpy(result->dx, so + h->oo_dx, sizeof(double) * n);
    if (result->P_out) std::memcpy(result->P_out, so + h->oo_Pout, sizeof(double) * (size_t)n * n);
    if (result->accept && F > 0) std::memcpy(result->accept, so + h->oo_accept, sizeof(int) * F);
    if (result->gamma && F > 0) std::memcpy(result->gamma, so + h->oo_gamma, sizeof(double) * F);
    if (result->H_thin || result->r_thin || result->K || result->G) {   // optional outputs: the staged download computes them
        orcvio_msckf_result opt = *result;
        opt.dx = nullptr; opt.P_out = nullptr; opt.accept = nullptr; opt.gamma = nullptr;
        rc = orcvio_msckf_download(h, &opt);
        if (rc != ORCVIO_OK) return rc;
    }
    const auto t4 = std::chrono::steady_clock::now();
    if (timing) {
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        static int calls = 0;
        if (us(t0, t4) > 2000.0 || (++calls % 64) == 0)
            fprintf(stderr, "update_features: staging %.0f us, launch + wait %.0f us, unpack %.0f us\n", us(t0, t1), us(t1, t3), us(t3, t4));
    }
    return rc;
}

// The gate alone: gatingTestFeature (src/orcvio.cpp:1953-1976) of featureJacobian_msckf for every listed track, against the
// prior -- what the reference asks of a feature before it lets it ENTER the state as a SLAM feature (:2361-2367) -- without
// an update.  gamma[F], accept[F].
int32_t orcvio_msckf_gate_tracks(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, const orcvio_msckf_window* window,
                                 const orcvio_msckf_tracks* tracks, const double* P, double* gamma, int32_t* accept) {
    if (!gamma || !accept) { g_last_error = "gate_tracks: null output"; return ORCVIO_ERR_INVALID; }
    int rc = orcvio_msckf_upload(h, flags, window, tracks, P);
    if (rc != ORCVIO_OK) return rc;
    if (h->pw_missing) { g_last_error = "gate_tracks: tracks without positions"; return ORCVIO_ERR_INVALID; }
    const int F = h->F;
    if (F == 0) return ORCVIO_OK;
    rc = launch_feature(h, h->stream);
    if (rc != ORCVIO_OK) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(gamma, h->d_gamma, sizeof(double) * F, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(accept, h->d_accept, sizeof(int) * F, hipMemcpyDeviceToHost));
    h->uploaded = false;   // nothing here is an update: the next update call uploads its own tracks
    return ORCVIO_OK;
}

// Object update: OrcVIO::removeLostObjects (src/orcvio.cpp:2154-2193).  Every object block is projected
// onto the left nullspace of its own Hf (SURVEY.md note N3: equal to the reference whenever one object
// arrives per call); the blocks are stacked, gated jointly with dof = sum(rows - cols) and applied in one
// update.  Objects with rows <= cols cannot be projected (math_utils.hpp:292) and are skipped.
