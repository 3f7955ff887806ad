// capi_frame.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// One frame in one call: the feature update and the object update that follows it in System::imageCallback
// (ros_wrapper/src/orcvio/src/System.cpp:548-554: Estimator->processFeatures, then processObjects).
//
// The object update has two halves.  The COMPRESSION -- tracks -> residual rows -> structured QR of H_f -> A' = sum B - Y^T Y --
// depends on the object tracks alone: not on the prior, not on the feature update.  The SOLVE needs the covariance the feature
// update leaves.  In two calls the device runs  [features: tracks | solve]  [objects: compression | solve]  one behind the
// other, and during both solves (single-workgroup Cholesky chains) it is almost idle.  Here the compression is enqueued on a
// stream of its own right behind the launch of the feature update and runs BESIDE the features' solve; the object solve joins
// both.  Same kernels, same arguments, same results as orcvio_msckf_io_update(commit) + orcvio_msckf_update_object_tracks.

// the two calls in sequence on what stands in the arena (the reference form; also the fall-back of the overlapped form);
// retry_forked: the repeat of a frame that lost an in-launch hand-off -- BOTH halves take the one-workgroup factorisation + solve
static int frame_sequential(orcvio_msckf_handle* h, orcvio_msckf_result* res_f, const FeatureView& v, const orcvio_msckf_flags* oflags,
                            const orcvio_object_eval_flags* efl, int N, const orcvio_object_track* tracks, int n_tracks, int commit_objects,
                            orcvio_msckf_result* res_o, bool retry_forked = false) {
    UpdateCall cf, co;
    cf.retry_forked = co.retry_forked = retry_forked;
    int rc = io_run(h, false, true, res_f->stats, cf);
    if (rc != ORCVIO_OK) { res_f->stats[3] = 0; return rc; }   // (refused: nothing was applied)
    const char* so = h->h_stage + h->in_cap;
    if (res_f->dx) std::memcpy(res_f->dx, so + v.oo_dx, sizeof(double) * v.n);
    if (res_f->gamma) std::memcpy(res_f->gamma, so + v.oo_gamma, sizeof(double) * v.F);
    if (res_f->accept) std::memcpy(res_f->accept, so + v.oo_accept, sizeof(int32_t) * v.F);
    rc = update_object_tracks_impl(h, oflags, efl, N, tracks, n_tracks, nullptr, res_o, co);
    if (rc == ORCVIO_OK && commit_objects) rc = orcvio_msckf_cov_commit(h);
    return rc;
}

// The object half's results to the pinned block AND its commit in one launch (k_epilogue with commit workgroups, as the feature half
// has had it): P+ over the resident covariance, S+ = sigma Z^T -- or the prior's own factor if the gate rejected the update -- into the
// spare factor buffer; refused on the device if the solve failed.  The host-side bookkeeping of orcvio_msckf_cov_commit follows at
// once (it is valid either way: a refused commit leaves the prior and a copy of its factor).  Saves the frame the host round trip of a
// separate cov_commit (k_fac_commit + a device-to-device copy of P+, ~10 us after the results were read).
static int publish_commit_enqueue(orcvio_msckf_handle* h, hipStream_t s) {
    // info_also: the feature half's status words, kept by its epilogue -- a refused feature half (chol(M1) not PD) refuses this commit too; ADVICE r5
    const int rc = launch_epilogue(s, epilogue_args(h, solve_out(h), h->out_shift, false, 2, h->d_obj_accept, h->d_step_words));
    if (rc != ORCVIO_OK) return rc;
    h->pub_pending = true;
    h->pub_enqueued++;
    fac_adopt_update(h);
    return ORCVIO_OK;
}

// ---- ORCVIO_FRAME_CHAIN=1: the object solve of the frame WITHOUT the covariance the feature update leaves --------------------------
// With P = L_f L_f^T the prior of the FEATURE update and M1 = s2 I + L_a^T A L_a its matrix (both still on the device), the object update
// on P+ = s2 L_f M1^-1 L_f^T is, exactly (Woodbury),
//     M12 = M1 + L_a^T A' L_a,   dx2 = L_f M12^-1 L_a^T b',   P++ = s2 L_f M12^-1 L_f^T,   gamma = (|r'|^2 - |z|^2) / s2,  z = L_M12^-1 L_a^T b':
// the sequential update of the reference (src/orcvio.cpp:2154-2193 behind :2497-2560) without ever reading P+, dx1 or the factor the
// feature half commits -- it depends on k_gemm(M) of the feature half and on A' only.  It runs on the objects' stream, on solve buffers
// of its own (U2, M2, R2, Z2, an outputs arena of its own), behind the compression, BESIDE the feature half's solve / finish / commit;
// only its finish (the gate's rejected branch copies P+) and its commit wait for the feature half's commit (a word the factorisation launch
// polls before it ends: LaEnd).
// Arithmetic differs from the two-call form in the last bits (another factor of the same matrix): opt-in, tested at 1e-10.
struct ChainGeom { PriorFactor pf; int n, NA, NAP, NP, ldz, kf, tail; double sigma; };

static int chain_buffers(orcvio_msckf_handle* h) {
    // (the gate's words: the in-launch finish of the chained solve writes them before the object half's bookkeeping would allocate them)
    if (!h->d_obj_accept) { HIPCHK(hipMalloc(&h->d_obj_accept, sizeof(int) * 4)); HIPCHK(hipMalloc(&h->d_obj_gamma, sizeof(double) * 4)); }
    if (h->d_U2) return ORCVIO_OK;
    const size_t np2 = (size_t)h->NP_max * h->NP_max;
    HIPCHK(hipMalloc(&h->d_U2, sizeof(double) * np2));
    HIPCHK(hipMalloc(&h->d_M2, sizeof(double) * np2));
    HIPCHK(hipMalloc(&h->d_RM2, sizeof(double) * np2));
    HIPCHK(hipMalloc(&h->d_Z2, sizeof(double) * np2));
    HIPCHK(hipMalloc(&h->d_DinvM2, sizeof(double) * 256 * TRSM_MAXBLK));
    HIPCHK(hipMalloc(&h->d_outs2, h->outs_cap));
    HIPCHK(hipMalloc(&h->d_chain_words, 512));
    HIPCHK(hipMemset(h->d_RM2, 0, sizeof(double) * np2));   // (strictly-lower tiles of the upper factor stay zero, as d_RM's)
    HIPCHK(hipMemset(h->d_outs2, 0, 256));
    HIPCHK(hipMemset(h->d_chain_words, 0, 512));
    return ORCVIO_OK;
}

// part 1, enqueued right behind the compression (before the host has finished staging the feature half's remaining launches, so that
// the device never waits for the host here): U', M12 and the factorisation + solve
static int frame_chain_solve(orcvio_msckf_handle* h, const ChainGeom& g, unsigned w1, unsigned w2, int dof, double chi2_prob) {
    hipStream_t sb = h->obj_stream;
    const int n = g.n, NA = g.NA, NAP = g.NAP, NP = g.NP, ldz = g.ldz, kfa = g.kf - g.tail;
    const long sLi = g.pf.sLi, sLj = g.pf.sLj;
    const double* La = g.pf.base + 15 * sLi;
    int* info2 = reinterpret_cast<int*>(h->d_outs2);
    int* flag2 = reinterpret_cast<int*>(h->d_chain_words + 32);
    int* rdy2 = reinterpret_cast<int*>(h->d_chain_words + 48);
    // U' = [A'; b'^T] L_a: behind the compression (this stream) and behind the feature half's k_gemm(M) (the word; L_a is older than that);
    // it also puts the second context's "lost" word back to zero (a frame that was abandoned half-way may have left it up)
    int rc = launch_gemm(sb, h->d_A, NAP, 1, La, sLi, sLj, NA + 1, kfa, NA, 1.0, 0.0, 0, h->d_U2, NP, 1, info2 + 8, h->d_chain_words, w1, info2 + 8);
    // M12 = M1 + L_a^T U' (upper tiles; M1 carries s2 I); the words of the factorisation behind it are cleared here, one kernel ahead
    if (rc == ORCVIO_OK) rc = launch_gemm(sb, La, sLj, sLi, h->d_U2, NP, 1, kfa, kfa, NA, 1.0, 0.0, 1, h->d_M2, NP, 1, flag2, nullptr, 0u, nullptr, rdy2, h->d_M,
                                          reinterpret_cast<int*>(h->d_chain_words + 64));
    // P++, dx2 and the gate by finish workgroups of the same launch (LaFin): the degrees of freedom are the scan's; should the bookkeeping
    // behind the compression count otherwise, frame_chain_finish decides again with a k_finish_sqrt of its own
    LaFin fin;
    int nfin = 0;
    h->chain_fin_dof = -1;
    if (h->fuse_finish) {
        const int ncb = (n + 1 + 15) / 16;
        fin.done = h->d_chain_words + 64; fin.step = flag2; fin.last_step = (kfa + 15) / 16 - 1;
        fin.nstate = n; fin.kdim = g.kf; fin.s2 = g.sigma * g.sigma;
        // (the OBJECT half's layout of the outputs arena -- layout_outputs(h, n, 1), which its bookkeeping sets up after this was enqueued)
        const size_t o_dx = 256, o_gamma = o_dx + al256(sizeof(double) * n), o_accept = o_gamma + al256(sizeof(double)), o_Pout = o_accept + al256(sizeof(int));
        fin.P_out = reinterpret_cast<double*>(h->d_outs2 + o_Pout); fin.dx = reinterpret_cast<double*>(h->d_outs2 + o_dx);
        fin.P = h->d_Pres; fin.keep_tail = 0;
        // (the threshold from the OBJECT update's flags: h->flags are still the feature half's here, as are h->NA / h->NAP = g's)
        fin.gate = object_gate(h, dof > 0 ? orcvio_msckf_chi2_quantile(dof, chi2_prob) : -1.0, reinterpret_cast<double*>(h->d_outs2 + o_gamma),
                               reinterpret_cast<int*>(h->d_outs2 + o_accept), nullptr);
        h->chain_fin_oo = o_Pout;
        fin.wait_word = h->d_chain_words + 1; fin.wait_expect = w2;   // (a rejected update copies P+: what the feature half commits)
        nfin = (ncb * (ncb + 1) / 2 + 1) / 2;
        h->chain_fin_dof = dof; h->chain_fin_thr = fin.gate.thr;
    }
    if (rc == ORCVIO_OK) rc = launch_potrf_solve_la(h, sb, 3, h->d_M2, NP, kfa, h->d_RM2, NP, h->d_DinvM2, info2 + 2, flag2, rdy2, info2 + 8, g.pf.base, sLj, sLi, n,
                                                     h->d_U2 + (size_t)NA * NP, 1L, h->d_Z2, ldz, g.tail, 1.0 / g.sigma, nullptr,
                                                     LaEnd{h->d_chain_words + 1, w2, h->d_info, info2}, fin, nfin);   // (does not end before the feature half's commit: LaEnd)
    return rc;
}

// part 2: the gate + P++ + dx, the results and the commit
static int frame_chain_finish(orcvio_msckf_handle* h, const ChainGeom& g, int dof, size_t obj_shift, unsigned w2) {
    hipStream_t sb = h->obj_stream;
    const int n = g.n, ldz = g.ldz, kf = g.kf;
    const double sigma2 = g.sigma * g.sigma;
    int* info2 = reinterpret_cast<int*>(h->d_outs2);
    double* dx2 = reinterpret_cast<double*>(h->d_outs2 + h->oo_dx);
    double* Pout2 = reinterpret_cast<double*>(h->d_outs2 + h->oo_Pout);
    h->obj_dof = dof;
    h->A_deferred = false;
    // (the feature half's commit -- P+ in d_Pres, S+ in d_Sres -- is done: the factorisation launch in front does not end before it, LaEnd)
    h->obj_thr = dof > 0 ? orcvio_msckf_chi2_quantile(dof, h->flags.chi2_prob) : -1.0;
    if (h->chain_fin_dof != dof || h->chain_fin_thr != h->obj_thr || h->chain_fin_oo != h->oo_Pout) {   // (else: decided and written by the finish workgroups of the factorisation launch, LaFin)
        const int nb = (n + 1 + 15) / 16, tiles = nb * (nb + 1) / 2;
        const ObjGate gate = object_gate(h, h->obj_thr, reinterpret_cast<double*>(h->d_outs2 + h->oo_gamma), reinterpret_cast<int*>(h->d_outs2 + h->oo_accept), info2 + 2);
        hipLaunchKernelGGL(k_finish_sqrt, dim3(tiles), dim3(256), 0, sb, (const double*)h->d_Z2, ldz, n, kf, sigma2, Pout2, dx2, gate, (const double*)h->d_Pres, 0);
    }
    HIPCHK(hipGetLastError());
    // results + commit in one launch (as publish_commit_enqueue), from the second outputs arena; the flag rises behind the commit too
    // (a rejected object update keeps the factor the feature half committed; info_also = the feature half's status words: a refused
    //  feature half -- its M1 is not to be trusted -- refuses this commit too)
    const SolveOut so2{h->d_outs2, Pout2, dx2, info2, h->d_Z2, ldz, kf, g.sigma, PriorFactor{h->d_Sres, 1L, (long)h->fac_ld}};
    const int re = launch_epilogue(sb, epilogue_args(h, so2, obj_shift, false, 2, h->d_obj_accept, h->d_info, nullptr, 1));
    if (re != ORCVIO_OK) return re;
    h->pub_pending = true;
    h->pub_enqueued++;
    h->commit_update(n, kf, ldz, g.tail, false, FacAfter::adopt);
    mark_update_enqueued(h, 2);
    h->last_stream = sb;
    h->cnt_chained++;
    return ORCVIO_OK;
}

// The object tracks of the NEXT orcvio_msckf_io_update_frame call, scanned and staged ahead of it (the caller has them before the frame's
// feature update starts: they come from the object mapper, src/orcvio/src/System.cpp:622-708): the frame call then finds its lists and the
// pinned staging arena filled and goes straight to the launches -- as the feature tracks are written into the arena before the call.
// Between io_begin (the window's clone count must stand) and the frame call; the SAME tracks pointer, count and flags must be handed to
// the frame call (anything else, or any other object call in between, and the frame call stages for itself).  The track data are COPIED
// here: later changes to them are not seen.
int32_t orcvio_msckf_io_stage_object_tracks(orcvio_msckf_handle* h, const orcvio_msckf_flags* oflags, const orcvio_object_eval_flags* efl,
                                            const orcvio_object_track* tracks, int32_t n_tracks) {
    const char* who = "orcvio_msckf_io_stage_object_tracks";
    if (!h || !oflags || !efl || !tracks || n_tracks < 1) { g_last_error = std::string(who) + ": null argument / no tracks"; return ORCVIO_ERR_INVALID; }
    if (!h->io_open || h->io_with_P) { g_last_error = std::string(who) + ": call orcvio_msckf_io_begin with with_P = 0 first"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    ObjPrestage& ps = h->prestage;
    ps.valid = false;
    const int oN = h->N;
    const int on = oflags->leg_dim + 6 * oN + h->n_extra;
    const int oNA = h->ekf_mode ? on - 15 : oflags->leg_dim + 6 * oN - 15, oNAP = round_up(oNA + 1, 16);
    if (!(oflags->leg_dim == 22 || oflags->leg_dim == 46) || oNAP > h->NAP_max) return ORCVIO_OK;   // (not a frame the one-launch compression takes: nothing staged)
    int rc = objects_scan(h, oN, tracks, n_tracks, ps.scan);
    if (rc != ORCVIO_OK) return rc;
    if (!obj_fused_eligible(h, tracks, oN, ps.scan.no_max)) return ORCVIO_OK;
    // (the compression of an earlier call may still be reading the staging arena: its stream is drained first -- it is, in a filter loop,
    //  long done)
    if (h->obj_stream) HIPCHK(hipStreamSynchronize(h->obj_stream));
    rc = objects_fused_pack(h, efl, tracks, ps.scan, ps.pl, oN, oNAP, ps.st);
    if (rc != ORCVIO_OK) return rc;
    ps.tracks = tracks; ps.n_tracks = n_tracks; ps.N = oN; ps.leg_dim = oflags->leg_dim; ps.efl = *efl;
    ps.valid = true;
    return ORCVIO_OK;
}

int32_t orcvio_msckf_io_update_frame(orcvio_msckf_handle* h, orcvio_msckf_result* res_f, const orcvio_msckf_flags* oflags,
                                     const orcvio_object_eval_flags* efl, const orcvio_object_track* tracks, int32_t n_tracks,
                                     int32_t commit_objects, orcvio_msckf_result* res_o) {
    const char* who = "orcvio_msckf_io_update_frame";
    if (!h || !res_f || !res_o || !oflags || !efl || n_tracks < 0) { g_last_error = std::string(who) + ": null argument"; return ORCVIO_ERR_INVALID; }
    if (h->io_submitted) { g_last_error = std::string(who) + ": an update submitted with orcvio_msckf_io_submit has not been collected"; return ORCVIO_ERR_INVALID; }
    if (!h->io_open || h->io_with_P) { g_last_error = std::string(who) + ": call orcvio_msckf_io_begin with with_P = 0 first (the frame runs on the resident covariance)"; return ORCVIO_ERR_INVALID; }
    if (h->tri_armed) { g_last_error = std::string(who) + ": the arena is armed by orcvio_msckf_io_triangulate (io_update, io_submit and the io_step_frame calls carry it; open the arena again for this call)"; return ORCVIO_ERR_INVALID; }
    if (res_f->P_out || res_f->K || res_f->G || res_f->H_thin || res_f->r_thin) { g_last_error = std::string(who) + ": the feature half returns dx, gamma, accept and stats (P+ stays resident)"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    static const bool overlap = [] { const char* e = getenv("ORCVIO_FRAME_OVERLAP"); return !e || atoi(e) != 0; }();   // 0: the two calls in sequence
    PhaseTimer timer;   // diagnostics (ORCVIO_TIMING): host wall time of the parts of THIS call, microseconds after its start
    PhaseTimer::Run tm = PhaseTimer::begin(&timer);
    auto tmark = [&](int i) { tm.mark(i); };
    int rc = ingest_raw(h, h->stream);   // what the caller wrote travels while the host checks it
    if (rc == ORCVIO_OK) rc = upload_finalize(h, who);
    if (rc != ORCVIO_OK) { (void)arena_mark_read(h, h->stream); return rc; }   // (the early pull may still be reading the arena)
    h->pw_missing = false;
    h->io_open = true;
    tmark(0);
    // what the feature half needs on the host once its results are published (the object half re-uses the handle's fields)
    const orcvio_msckf_flags fflags = h->flags;
    const int N = h->N, F = h->F, nobs = h->nobs;
    std::vector<int>& keep_rows = h->frame_row_ptr;
    keep_rows = h->h_row_ptr;
    FeatureView v = feature_view(h);
    v.row_ptr = keep_rows.data();
    // the factor the commit leaves (kf columns) must be one the object solve can take without factoring P+ again
    const int kf16 = round_up(h->kf, 16);
    const bool fac_ok = kf16 <= POTRF_MAXN && kf16 / 16 <= TRSM_MAXBLK && kf16 <= h->NP_max;
    // The overlapped form compresses the objects into h->d_A (scratch h->d_Ab) on a stream of its own while the feature update is in
    // flight: legal only while the feature half never touches those blocks, i.e. while it defers the assembly of A (k_front leaves the
    // Grams, k_gemm_asmA assembles strips in LDS).  Whenever it assembles A in memory -- no tracks, more than ~510 tracks, NA > 192
    // (leg_dim 46 with N >= 27), more than four row chunks, ORCVIO_OPT_FUSED_FRONT = 0 -- the two halves run in sequence (ADVICE r3).
    if (!overlap || !fac_ok || h->n_nui > 0 || !h->factor_opt || h->obj_dof_rank || res_o->P_out || res_o->G || !front_defers_assembly(h, false))
        return frame_sequential(h, res_f, v, oflags, efl, N, tracks, n_tracks, commit_objects, res_o);
    if (!h->obj_stream) {
        HIPCHK(hipStreamCreateWithFlags(&h->obj_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&h->ev_obj, hipEventDisableTiming));
    }
    hipStream_t s = h->stream;
    h->last_stream = s;
    if (h->dl_pending) { HIPCHK(hipStreamSynchronize(h->dl_stream)); h->dl_pending = false; }
    // ---- features: ingest, the five kernels, results + commit + flag, as orcvio_msckf_io_update(commit)
    // The feature half of a FRAME goes out as plain launches, not as a replayed graph: behind a hipGraphLaunch the stream's next plain
    // launch starts ~14 us late (the graph's completion marker; measured with and without the cross-stream join below), and the object
    // solve is such a launch -- 14 us of the frame.  Seven plain launches cost the host ~15 us more to enqueue, which it has (the
    // device is busy with the tracks for 40 us).
    // ... and the objects' compression is enqueued in the MIDDLE of them: right behind the tracks' launch (k_front: 40 us of device time),
    // ahead of the feature update's remaining five launches, which the host has 40 us to put out.  The compression then starts ~20 us
    // earlier and is done well before the feature half; possible when every object takes the one-launch compression (k_obj_fused), whose
    // staging and launches touch none of the handle's feature-problem fields.
    ObjScan early_scan;   // what the scan of the tracks found, here or ahead of the call
    bool early = false;
    int early_rc = ORCVIO_OK;
    const int oN = N;
    const int on = oflags->leg_dim + 6 * oN + h->n_extra;
    const int oNA = h->ekf_mode ? on - 15 : oflags->leg_dim + 6 * oN - 15, oNAP = round_up(oNA + 1, 16);
    // (orcvio_msckf_io_stage_object_tracks ahead of this call: the scan and the staging of these very tracks are done -- ~14 us of host time
    //  that stood between the tracks' launch and the compression's)
    const ObjPrestage& ps = h->prestage;
    const bool pre = ps.valid && ps.tracks == tracks && ps.n_tracks == n_tracks && ps.N == oN && ps.leg_dim == oflags->leg_dim &&
                     std::memcmp(&ps.efl, efl, sizeof(*efl)) == 0 && oNAP <= h->NAP_max;
    h->prestage.valid = false;   // (one use)
    if (pre) {
        early_scan = ps.scan;
        early = true;
        h->cnt_prestaged++;
    } else if (n_tracks > 0 && (oflags->leg_dim == 22 || oflags->leg_dim == 46) && oNAP <= h->NAP_max) {
        if (objects_scan(h, oN, tracks, n_tracks, early_scan) == ORCVIO_OK && obj_fused_eligible(h, tracks, oN, early_scan.no_max)) early = true;
    }
    // the chained object solve (above): opt-in, for frames whose objects all take the one-launch compression and commit in the call
    bool chain = h->frame_chain && early && commit_objects != 0 && !h->ekf_mode && h->n_extra == 0 && oflags->leg_dim == fflags.leg_dim &&
                 oflags->noise_feature == fflags.noise_feature &&   // (M12 = M1 + L_a^T A' L_a holds for ONE sigma)
                 fused_solve_active(h) && la_solve_active(h, (h->kf - h->tail + 15) / 16, false) && front_fused_active(h, false);
    const bool signal_done = !chain;   // (the chained solve runs on the compression's own stream: no completion word to poll)
    unsigned w1 = 0u, w2 = 0u;
    int chain_rc = ORCVIO_OK;
    bool chain_part1 = false;
    if (chain) {
        const int rb = chain_buffers(h);
        if (rb != ORCVIO_OK) return rb;
        w1 = ++h->chain_seq; w2 = w1;
    }
    const ChainGeom cgeom{prior_factor(h), h->n, h->NA, h->NAP, h->NP, h->ldz, h->kf, h->tail, h->flags.noise_feature};   // (the FEATURE update's solve, before the book-keeping below)
    std::function<int()> mid = [&]() -> int {
        prof_begin(h, h->obj_stream);
        early_rc = pre ? objects_fused_launch(h, h->obj_stream, h->d_A, ps.pl, ps.st, early_scan.nobj, oN, oNA, oNAP, oflags->leg_dim - 15, signal_done)
                       : objects_tracks_fused(h, h->obj_stream, h->d_A, efl, tracks, early_scan, oN, oNA, oNAP, oflags->leg_dim - 15, signal_done);
        // (the event the main stream joins on: not in the chained form, whose solve runs on this stream -- a record costs ~5 us of stream
        //  time between k_gemm_objA and the solve's first product; if the chain is dropped after all, it is recorded then)
        if (!chain && early_rc == ORCVIO_OK && hipEventRecord(h->ev_obj, h->obj_stream) != hipSuccess) { (void)hipGetLastError(); early_rc = ORCVIO_ERR_HIP; }
        if (chain && early_rc == ORCVIO_OK) { chain_rc = frame_chain_solve(h, cgeom, w1, w2, early_scan.dof, oflags->chi2_prob); chain_part1 = true; }
        return ORCVIO_OK;   // (a refusal of the object half must not stop the feature half: it is reported below)
    };
    { const int rw = step_words(h); if (rw != ORCVIO_OK) return rw; }
    UpdateCall cf;   // the feature half
    cf.fin_frame = chain;   // (its P+ / dx by finish workgroups of its solve launch: finish_fused_active)
    cf.info_keep = h->d_step_words;   // (its epilogue keeps a copy of its status words for the object half's commit)
    if (chain) { cf.mark_M_word = h->d_chain_words; cf.mark_M_val = w1; }   // (launch_solve_stage(ST_FORM_M) stores it)
    cf.mid = early ? &mid : nullptr;
    rc = io_enqueue(h, s, false, true, cf);
    h->cnt_plain_runs++;
    h->A_deferred = front_defers_assembly(h, false);
    tmark(1);
    if (chain && rc == ORCVIO_OK) {   // the word behind the feature half's epilogue (its commit): a launch of its own, behind the kernel boundary
        if (cf.mark_M_word) {   // (the feature half did not pass ST_FORM_M -- not the shape this is for: release what waits for the word, drop the chain)
            chain = false;
            hipLaunchKernelGGL(k_obj_done, dim3(1), dim3(64), 0, s, h->d_chain_words, w1);
        }
        else hipLaunchKernelGGL(k_obj_done, dim3(1), dim3(64), 0, s, h->d_chain_words + 1, w2);
    }
    if (rc != ORCVIO_OK) {
        // The feature half could not be enqueued to its end, but `mid` may have put the objects' compression and the chained solve on the
        // objects' stream already: its launches poll words that will never rise.  Release them, drain both streams, clear the second
        // context's status words -- and leave the arena to the next writer only then (ADVICE r5).
        if (chain_part1 && h->d_chain_words) {
            hipLaunchKernelGGL(k_obj_done, dim3(1), dim3(64), 0, s, h->d_chain_words, w1);
            hipLaunchKernelGGL(k_obj_done, dim3(1), dim3(64), 0, s, h->d_chain_words + 1, w2);
            (void)hipGetLastError();
        }
        if (h->obj_stream) (void)hipStreamSynchronize(h->obj_stream);
        (void)hipStreamSynchronize(s);
        if (h->d_outs2) (void)hipMemset(h->d_outs2, 0, 256);
        if (h->d_chain_words) (void)hipMemset(h->d_chain_words + 32, 0, 256);
        h->ran = false;
        return rc;
    }
    h->pub_enqueued++;
    const unsigned long long feat_pub = h->pub_enqueued;   // (the feature half's publication: what io_wait below waits for)
    mark_update_enqueued(h, 0);
    // (No event behind the arena's last reader here -- the ingest kernels at the head of the feature half: a hipEventRecord costs ~5 us of
    //  stream time, and it would stand between the feature half's epilogue and the object solve.  This call does not return before the
    //  feature half has published -- behind its ingest -- or, on the failure paths below, before the streams are drained: the arena is
    //  free again whenever the caller can write it.)
    // the host-side book-keeping of that commit, AHEAD of its results (undone below if the device refuses the update): the object
    // solve enqueued next takes the factor the epilogue is going to write
    const CovState undo = cov_state(h);
    fac_adopt_update(h);
    // the feature results land at the start of the pinned output block; the object results go where P+ would have gone
    const size_t obj_shift = (h->oo_Pout + 63) & ~(size_t)63;
    // ---- objects: staging on the host while the tracks of the feature update run, compression on its own stream
    int32_t dof = 0;
    bool commit_in_launch = false;
    h->frame_mode = true;
    h->obj_early = early && early_rc == ORCVIO_OK ? &early_scan : nullptr;   // (the compression is out already: the call below does the bookkeeping only)
    int rco = early && early_rc != ORCVIO_OK ? early_rc
                                              : orcvio_msckf_objects_local_tracks(h, oflags, efl, N, tracks, n_tracks, nullptr, h->d_A, &dof, (void*)h->obj_stream);
    h->obj_early = nullptr;
    h->frame_mode = false;
    h->last_stream = s;
    tmark(2);
    if (rco == ORCVIO_OK && chain && chain_part1 && h->obj_last_fused && h->n == cgeom.n && h->NA == cgeom.NA && h->NAP == cgeom.NAP) {
        rco = chain_rc == ORCVIO_OK ? frame_chain_finish(h, cgeom, dof, obj_shift, w2) : chain_rc;
        if (rco == ORCVIO_OK) { h->out_shift = obj_shift; commit_in_launch = true; }
    } else if (rco == ORCVIO_OK) {
        chain = false;
        // the object solve: behind the features' commit (stream order) AND the compression.  The one-launch compression ends with a
        // one-word launch (k_obj_done) that stores its sequence number; the solve's first product polls that word -- no stream-level join,
        // which costs ~10 us of dispatch on this stream even when the event fired long ago (the general path takes the event)
        UpdateCall co;   // the object half's solve
        if (h->obj_last_fused && signal_done) { co.join_wait = h->d_obj_done; co.join_expect = h->obj_done_total; }
        else {
            if (!early || !signal_done) HIPCHK(hipEventRecord(h->ev_obj, h->obj_stream));   // (!signal_done: the chain was dropped after the compression went out without its event)
            HIPCHK(hipStreamWaitEvent(s, h->ev_obj, 0));
        }
        rco = objects_finish_impl(h, h->d_A, 1, 0, nullptr, dof, s, co);
    }
    if (rco == ORCVIO_OK && !chain) {
        h->out_shift = obj_shift;
        // (k_epilogue + the flag word: 3-5 us sooner than a copy and a stream synchronisation here -- the calling thread is spinning on that word for
        //  the feature half anyway; for the object update on its own the copy wins.)  With commit_objects the commit rides in the same launch.
        commit_in_launch = commit_objects != 0;
        rco = commit_in_launch ? publish_commit_enqueue(h, s) : publish_enqueue(h, s, false);
    }
    tmark(3);
    // ---- the feature results (flag word of k_epilogue)
    rc = io_wait(h, s, feat_pub);
    tmark(4);
    const char* so = h->h_stage + h->in_cap;
    const int* info = reinterpret_cast<const int*>(so);
    bool redo = false;
    if (rc == ORCVIO_OK && info[8] != 0) redo = true;   // an in-launch hand-off of the feature update was lost (somebody else held compute units)
    if (rc == ORCVIO_OK && !redo) rc = feature_outcome_view(h, v, so, res_f->stats);
    if (rc != ORCVIO_OK || redo) {
        // the device refused the feature update (its commit too), or has to run it again: whatever the object half did meanwhile
        // ran on the wrong prior.  Drain, undo the book-keeping, and -- after a lost hand-off -- run the frame again as two calls.
        (void)hipStreamSynchronize(h->obj_stream);
        (void)hipStreamSynchronize(s);
        h->dl_pending = false; h->pub_pending = false; h->out_shift = 0; h->objects_mode = false; h->ran = false;
        cov_restore(h, undo);
        if (!redo) { res_f->stats[3] = 0; return rc; }   // (refused: nothing was applied)
        { const int rh = handoff_reset(h); if (rh != ORCVIO_OK) return rh; }
        const bool keep_fused = h->front_fused;
        h->front_fused = false;   // (plain launches, no in-launch device-wide wait, for the repeat ... and, retry_forked, the one-workgroup
                                  //  factorisation + solve: the far workgroups of the look-ahead form are one more thing that has to be
                                  //  co-resident; both halves of the repeat)
        rc = upload_begin(h, &fflags, N, F, nobs, false, true, who);
        if (rc == ORCVIO_OK) rc = ingest_raw(h, h->stream);
        if (rc == ORCVIO_OK) { h->io_open = true; rc = upload_finalize(h, who); }
        if (rc == ORCVIO_OK) { h->pw_missing = false; rc = frame_sequential(h, res_f, v, oflags, efl, N, tracks, n_tracks, commit_objects, res_o, true); }
        h->front_fused = keep_fused;
        return rc;
    }
    if (res_f->dx) std::memcpy(res_f->dx, so + v.oo_dx, sizeof(double) * v.n);
    if (res_f->gamma) std::memcpy(res_f->gamma, so + v.oo_gamma, sizeof(double) * v.F);
    if (res_f->accept) std::memcpy(res_f->accept, so + v.oo_accept, sizeof(int32_t) * v.F);
    // ---- the object results
    if (rco != ORCVIO_OK) {   // the object half could not be enqueued (its tracks were refused): the feature update stands, committed
        (void)hipStreamSynchronize(h->obj_stream);
        (void)hipStreamSynchronize(s);
        h->dl_pending = false; h->pub_pending = false; h->out_shift = 0; h->objects_mode = false;
        h->ran = false;   // (nothing left to commit: the feature half is committed already, the object half did not run to its end)
        return rco;
    }
    rc = orcvio_msckf_objects_download(h, res_o);
    tmark(5);
    if (timer.due(1)) fprintf(stderr, "io_update_frame: ingest + checks %.1f | feature half + compression%s enqueued %.1f | object bookkeeping %.1f | object solve enqueued %.1f | feature results %.1f | object results %.1f us\n",
                              timer.mean(0, 1), chain ? " + chained solve" : "", timer.mean(1, 1), timer.mean(2, 1), timer.mean(3, 1), timer.mean(4, 1), timer.mean(5, 1));
    h->out_shift = 0;
    h->objects_mode = false;
    if (chain) {   // (the chained object solve ran on the objects' stream, with status words of its own)
        h->last_stream = s;
        if (rc == ORCVIO_ERR_TIMEOUT) { HIPCHK(hipStreamSynchronize(h->obj_stream)); HIPCHK(hipMemset(h->d_outs2, 0, 256)); HIPCHK(hipMemset(h->d_chain_words + 32, 0, 128)); }
    }
    if (rc == ORCVIO_OK && commit_objects && !commit_in_launch) rc = orcvio_msckf_cov_commit(h);
    return rc;
}
