// capi_zupt.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// zero-velocity frames on the resident covariance (measurementUpdate_ZUPT_vpq, src/orcvio.cpp:3326-3454; zupt_ops.hpp).

// Everything that can be refused before a launch.  `n` is the resident dimension the update will see.
static int zupt_validate(const orcvio_msckf_handle* h, const orcvio_msckf_zupt* z, int n, const char* who) {
    if (h->comm || h->ipc) { g_last_error = std::string(who) + ": not with a communicator on the handle"; return ORCVIO_ERR_INVALID; }
    if (z->leg_dim != 22 && z->leg_dim != 46) { g_last_error = std::string(who) + ": leg_dim must be 22 or 46"; return ORCVIO_ERR_INVALID; }
    if (z->n_clones < 2) { g_last_error = std::string(who) + ": the update needs the two newest clones (n_clones >= 2)"; return ORCVIO_ERR_INVALID; }
    if (6 * h->n_nui > h->n_extra && h->n_nui > 0) { g_last_error = std::string(who) + ": ORCVIO_OPT_EXTRA_STATES counts the nuisance states of ORCVIO_OPT_SCHMIDT_STATES"; return ORCVIO_ERR_INVALID; }
    if (h->res_n == 0 || n > h->n_max || (long)z->leg_dim + 6L * z->n_clones + h->n_extra != (long)n) {
        g_last_error = std::string(who) + ": leg_dim + 6 n_clones + ORCVIO_OPT_EXTRA_STATES is not the resident dimension"; return ORCVIO_ERR_INVALID;
    }
    const double var[3] = {z->noise_v, z->noise_p, z->noise_q};
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(var[k]) || !(var[k] > 0.0)) { g_last_error = std::string(who) + ": the variances must be finite and positive"; return ORCVIO_ERR_INVALID; }
    if (!all_finite(z->r, 9)) { g_last_error = std::string(who) + ": non-finite residual"; return ORCVIO_ERR_INVALID; }
    return ORCVIO_OK;
}

// dx [n] and the status word of the launch: in the propagation scratch (46 n_max + 2 46^2 doubles), which nothing behind the update reads
static inline double* zupt_dx(orcvio_msckf_handle* h) { return h->d_covT; }
static inline int* zupt_status(orcvio_msckf_handle* h) { return reinterpret_cast<int*>(h->d_covT + h->n_max); }

// The launches: P+ and dx into the spare covariance buffer, S+ into the spare factor buffer; the buffers change roles on the host.
// A refusal on the device leaves bit copies there, so what is enqueued behind this reads the prior.
static int zupt_enqueue(orcvio_msckf_handle* h, const orcvio_msckf_zupt* z, const int* also = nullptr) {
    const int n = h->res_n;
    hipStream_t s = h->stream;
    ZuptArgs a;
    for (int k = 0; k < 9; ++k) a.r[k] = z->r[k];
    a.noise[0] = z->noise_v; a.noise[1] = z->noise_p; a.noise[2] = z->noise_q;
    a.n = n; a.b = z->leg_dim + 6 * z->n_clones; a.nui6 = 6 * h->n_nui; a.also = also;
    const int nt = (n + ZUPT_TILE - 1) / ZUPT_TILE;
    const CovEdit e = h->zupt(h->n_nui == 0, ZUPT_KMAX);   // (nuisance states: the restored block breaks P = S S^T, no factor)
    hipLaunchKernelGGL(k_zupt_cov, dim3(nt, nt), dim3(256), 0, s, e.P, a, e.Pout, zupt_dx(h), zupt_status(h));
    if (e.fac) hipLaunchKernelGGL(k_zupt_fac, dim3((n + ZUPT_FAC_ROWS - 1) / ZUPT_FAC_ROWS), dim3(256), 0, s, e.S, e.ld_in, e.fac_k, a,
                                  (const int*)zupt_status(h), e.Sout);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// the one wait: dx [n_dx] and the status word
static int zupt_collect(orcvio_msckf_handle* h, int n_dx, double* dx, int* refused) {
    int st = 0;
    const FetchCopy fc[] = {{dx, zupt_dx(h), sizeof(double) * (size_t)n_dx}, {&st, zupt_status(h), sizeof(int)}};
    const int rc = fetch_copies(h, h->stream, fc, 2);
    if (rc != ORCVIO_OK) return rc;
    *refused = st != 0;
    return ORCVIO_OK;
}

int32_t orcvio_msckf_cov_zupt(orcvio_msckf_handle* h, const orcvio_msckf_zupt* z, double* dx, int32_t* applied) {
    if (!h || !z || !dx || !applied) { g_last_error = "cov_zupt: null argument"; return ORCVIO_ERR_INVALID; }
    { const int rv = zupt_validate(h, z, h->res_n, "cov_zupt"); if (rv != ORCVIO_OK) return rv; }
    HIPCHK(hipSetDevice(h->device));
    const CovState before = cov_state(h);
    { const int rc = zupt_enqueue(h, z); if (rc != ORCVIO_OK) { cov_restore(h, before); return rc; } }
    int refused = 0;
    // (a failed wait: the outcome is unknown, but the launches wrote the spare buffers only -- the prior and its factor stand)
    { const int rc = zupt_collect(h, h->res_n, dx, &refused); if (rc != ORCVIO_OK) { cov_restore(h, before); return rc; } }
    *applied = refused ? 0 : 1;
    if (refused) {   // nothing is swapped: P, its factor and their bookkeeping are the prior's own
        cov_restore(h, before);
        g_last_error = "cov_zupt: H P H^T + R not positive definite, or a non-finite covariance: nothing applied";
        return ORCVIO_ERR_NOT_SPD;
    }
    return ORCVIO_OK;
}

// What both stationary-frame calls refuse about Phi / Q and an arming, before their validation of the window
static int zupt_frame_args(const orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame* f, const char* who, bool* armed) {
    if ((f->Phi == nullptr) != (f->Q == nullptr)) { g_last_error = std::string(who) + ": Phi and Q come together"; return ORCVIO_ERR_INVALID; }
    *armed = h->imu_armed;   // orcvio_msckf_io_propagate_imu: Phi, Q come from k_imu_phi_q, in front of the propagation launches
    if (*armed && f->Phi) { g_last_error = std::string(who) + ": the handle is armed by orcvio_msckf_io_propagate_imu: Phi and Q must be NULL"; return ORCVIO_ERR_INVALID; }
    if (*armed && f->zupt.leg_dim != 22) { g_last_error = std::string(who) + ": armed IMU propagation at leg_dim 22 only"; return ORCVIO_ERR_INVALID; }
    return ORCVIO_OK;
}
// ... and the launches in front of their update: propagation (given, or armed) and augmentation
// (with the dimensions validated, cov_propagate and cov_augment have nothing left to refuse)
static int zupt_frame_head(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame* f, bool armed) {
    HIPCHK(hipSetDevice(h->device));
    int rc = ORCVIO_OK;
    if (f->Phi) rc = orcvio_msckf_cov_propagate(h, f->zupt.leg_dim, f->Phi, f->Q);
    if (armed) {   // a refused Phi (status word) leaves P as it is in the propagation and refuses the update; the augmentation stands
        rc = imu_consume(h, h->stream);
        if (rc == ORCVIO_OK) rc = launch_cov_propagate(h, h->stream, h->propagate(), 22, imu_dphi(h), imu_dq(h), imu_status(h));
    }
    if (rc == ORCVIO_OK && f->augment) rc = orcvio_msckf_cov_augment(h);
    return rc;
}

int32_t orcvio_msckf_cov_zupt_frame(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame* f, double* dx, int32_t* applied, int32_t* n_after) {
    if (!h || !f || !dx || !applied || !n_after) { g_last_error = "cov_zupt_frame: null argument"; return ORCVIO_ERR_INVALID; }
    const orcvio_msckf_zupt* z = &f->zupt;
    bool armed = false;
    { const int rv = zupt_frame_args(h, f, "cov_zupt_frame", &armed); if (rv != ORCVIO_OK) return rv; }
    const int n = h->res_n + (f->augment ? 6 : 0);   // what the update sees
    { const int rv = zupt_validate(h, z, n, "cov_zupt_frame"); if (rv != ORCVIO_OK) return rv; }
    // (with the dimensions above, cov_remove_clones has nothing left to refuse either)
    if (f->augment && h->n_extra > h->res_n - 15) { g_last_error = "cov_zupt_frame: more extra states than the resident covariance has"; return ORCVIO_ERR_INVALID; }
    int rc = zupt_frame_head(h, f, armed);   // (behind a refused armed Phi the marginalisation stands too)
    if (rc != ORCVIO_OK) return rc;
    const CovState before = cov_state(h);
    rc = zupt_enqueue(h, z, armed ? imu_status(h) : nullptr);
    if (rc != ORCVIO_OK) { cov_restore(h, before); return rc; }   // (a launch that failed: nothing changed roles, propagation and augmentation stand)
    if (f->remove_previous) {
        const int32_t prev = z->n_clones - 2;
        rc = orcvio_msckf_cov_remove_clones(h, z->leg_dim, &prev, 1);
    }
    int refused = 0;
    if (rc == ORCVIO_OK) rc = zupt_collect(h, n, dx, &refused);
    if (rc != ORCVIO_OK) {   // a HIP error behind the update: its outcome is unknown and the row deletion may have overwritten the prior's
        h->res_n = 0;        // buffer, so NOTHING is resident any more -- the caller sets the covariance again (cov_set)
        h->fac_valid = false;
        return rc;
    }
    *n_after = h->res_n;
    *applied = refused ? 0 : 1;
    if (refused) {   // the spare buffers took bit copies of the prior and of its factor, whose zero trailing columns are still zero
        h->zupt_refused(before.fac_tail);
        g_last_error = armed && imu_refused(h) ? "cov_zupt_frame: Phi or Q of the armed IMU propagation not finite: no propagation, no update"
                                               : "cov_zupt_frame: H P H^T + R not positive definite, or a non-finite covariance: the update was not applied";
        return ORCVIO_ERR_NOT_SPD;
    }
    return ORCVIO_OK;
}

// ---- the stationary frame of a hybrid filter: every in-state feature leaves in front of the update (checkZUPTFeat :3102-3119,
// checkZUPTIMU :3302-3319), the previous clone behind it -- ONE launch that writes what stays (k_zupt_cov_keep / k_zupt_fac_keep)

// what the hybrid calls refuse on top of zupt_validate; `n` is the resident dimension the update will see
static int zupt_hybrid_validate(const orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame_hybrid* f, int n, const char* who) {
    if (f->idp_dim != 1 && f->idp_dim != 3) { g_last_error = std::string(who) + ": idp_dim must be 1 or 3"; return ORCVIO_ERR_INVALID; }
    if (f->n_feature_states < 0) { g_last_error = std::string(who) + ": n_feature_states must not be negative"; return ORCVIO_ERR_INVALID; }
    if (h->n_nui > 0) { g_last_error = std::string(who) + ": not with nuisance states (ORCVIO_OPT_SCHMIDT_STATES > 0)"; return ORCVIO_ERR_INVALID; }
    { const int rv = zupt_validate(h, &f->frame.zupt, n, who); if (rv != ORCVIO_OK) return rv; }
    if ((long)f->idp_dim * f->n_feature_states != (long)h->n_extra) {
        g_last_error = std::string(who) + ": idp_dim n_feature_states is not ORCVIO_OPT_EXTRA_STATES"; return ORCVIO_ERR_INVALID;
    }
    return ORCVIO_OK;
}

// The launches of the fused update on the resident covariance (dimension n = h->res_n): what stays of P+ into the spare covariance
// buffer, of S+ into the spare factor buffer, dx [b] and the status word.  No buffer changes roles here: CovBook::zupt_keep_done, with
// the outcome, behind the wait.
static int zupt_keep_enqueue(orcvio_msckf_handle* h, const orcvio_msckf_zupt* z, bool remove_previous, const int* also, CovEdit* edit) {
    const int n = h->res_n;
    hipStream_t s = h->stream;
    ZuptArgs a;
    for (int k = 0; k < 9; ++k) a.r[k] = z->r[k];
    a.noise[0] = z->noise_v; a.noise[1] = z->noise_p; a.noise[2] = z->noise_q;
    a.n = n; a.b = z->leg_dim + 6 * z->n_clones; a.nui6 = 0; a.also = also;
    const ZuptKeep kp{a.b - (remove_previous ? 6 : 0), remove_previous ? a.b - 12 : a.b};   // the clone at window rank N-2
    const int nt = (n + ZUPT_TILE - 1) / ZUPT_TILE;
    const CovEdit e = h->zupt_keep(kp.m, h->n_nui == 0, ZUPT_KMAX);
    hipLaunchKernelGGL(k_zupt_cov_keep, dim3(nt, nt), dim3(256), 0, s, e.P, a, kp, e.Pout, zupt_dx(h), zupt_status(h));
    if (e.fac) hipLaunchKernelGGL(k_zupt_fac_keep, dim3((n + ZUPT_FAC_ROWS - 1) / ZUPT_FAC_ROWS), dim3(256), 0, s, e.S, e.ld_in, e.fac_k, a, kp,
                                  e.ld_out, (const int*)zupt_status(h), e.Sout);
    HIPCHK(hipGetLastError());
    *edit = e;
    return ORCVIO_OK;
}

int32_t orcvio_msckf_cov_zupt_frame_hybrid(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame_hybrid* hy, double* dx, int32_t* applied,
                                           int32_t* n_after) {
    if (!h || !hy || !dx || !applied || !n_after) { g_last_error = "cov_zupt_frame_hybrid: null argument"; return ORCVIO_ERR_INVALID; }
    const orcvio_msckf_zupt_frame* f = &hy->frame;
    const orcvio_msckf_zupt* z = &f->zupt;
    bool armed = false;
    { const int rv = zupt_frame_args(h, f, "cov_zupt_frame_hybrid", &armed); if (rv != ORCVIO_OK) return rv; }
    const int n = h->res_n + (f->augment ? 6 : 0);   // what the update sees
    { const int rv = zupt_hybrid_validate(h, hy, n, "cov_zupt_frame_hybrid"); if (rv != ORCVIO_OK) return rv; }
    if (f->augment && h->n_extra > h->res_n - 15) { g_last_error = "cov_zupt_frame_hybrid: more extra states than the resident covariance has"; return ORCVIO_ERR_INVALID; }
    int rc = zupt_frame_head(h, f, armed);
    if (rc != ORCVIO_OK) return rc;
    CovEdit e;
    rc = zupt_keep_enqueue(h, z, f->remove_previous != 0, armed ? imu_status(h) : nullptr, &e);
    if (rc != ORCVIO_OK) return rc;   // (a launch that failed: nothing changed roles, propagation and augmentation stand)
    int refused = 0;
    // (a failed wait: the outcome is unknown, but the launches wrote the spare buffers only -- the propagated, augmented prior and its factor stand)
    rc = zupt_collect(h, z->leg_dim + 6 * z->n_clones, dx, &refused);
    if (rc != ORCVIO_OK) return rc;
    h->zupt_keep_done(e, !refused);
    *n_after = h->res_n;
    *applied = refused ? 0 : 1;
    if (refused) {
        g_last_error = armed && imu_refused(h) ? "cov_zupt_frame_hybrid: Phi or Q of the armed IMU propagation not finite: no propagation, no update"
                                               : "cov_zupt_frame_hybrid: H P H^T + R not positive definite, or a non-finite covariance: nothing applied, no state has left";
        return ORCVIO_ERR_NOT_SPD;
    }
    return ORCVIO_OK;
}

// checkZUPTFeat's decision (src/orcvio.cpp:3081-3100) on the pixel distances the front end computed: host arithmetic, no handle
int32_t orcvio_msckf_zupt_check_feat(const double* dis, int32_t n, double max_dis, int32_t* accept, double* kth) {
    if (!accept || !kth || n < 0 || (n > 0 && !dis) || !std::isfinite(max_dis)) { g_last_error = "zupt_check_feat: null argument, negative count or non-finite threshold"; return ORCVIO_ERR_INVALID; }
    if (!all_finite(dis, (size_t)n)) { g_last_error = "zupt_check_feat: non-finite distance"; return ORCVIO_ERR_INVALID; }
    *accept = 0;
    *kth = std::nan("");
    if (n < 20) return ORCVIO_OK;   // :3082-3086: too few tracked features to decide on
    std::vector<double> d(dis, dis + n);
    std::nth_element(d.begin(), d.end() - 9, d.end());   // the element nine decrements from end() of the sorted list (:3089-3093)
    *kth = d[(size_t)n - 9];
    *accept = *kth < max_dis ? 1 : 0;
    return ORCVIO_OK;
}
