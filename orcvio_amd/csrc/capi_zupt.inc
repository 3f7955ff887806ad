// capi_zupt.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// zero-velocity frames on the resident covariance (measurementUpdate_ZUPT_vpq, src/orcvio.cpp:3326-3454; zupt_ops.hpp).

static int zupt_refuse(const char* who, const char* what) { g_last_error = std::string(who) + what; return ORCVIO_ERR_INVALID; }

// Everything that can be refused before a launch.  `n` is the resident dimension the update will see.
static int zupt_validate(const orcvio_msckf_handle* h, const orcvio_msckf_zupt* z, int n, const char* who) {
    if (h->comm || h->ipc) return zupt_refuse(who, ": not with a communicator on the handle");
    if (z->leg_dim != 22 && z->leg_dim != 46) return zupt_refuse(who, ": leg_dim must be 22 or 46");
    if (z->n_clones < 2) return zupt_refuse(who, ": the update needs the two newest clones (n_clones >= 2)");
    if (6 * h->n_nui > h->n_extra && h->n_nui > 0) return zupt_refuse(who, ": ORCVIO_OPT_EXTRA_STATES counts the nuisance states of ORCVIO_OPT_SCHMIDT_STATES");
    if (h->res_n == 0 || n > h->n_max || (long)z->leg_dim + 6L * z->n_clones + h->n_extra != (long)n) return zupt_refuse(who, ": leg_dim + 6 n_clones + ORCVIO_OPT_EXTRA_STATES is not the resident dimension");
    const double var[3] = {z->noise_v, z->noise_p, z->noise_q};
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(var[k]) || !(var[k] > 0.0)) return zupt_refuse(who, ": the variances must be finite and positive");
    if (!all_finite(z->r, 9)) return zupt_refuse(who, ": non-finite residual");
    return ORCVIO_OK;
}

// dx [n] and the status word of the launch: in the propagation scratch (46 n_max + 2 46^2 doubles), which nothing behind the update reads
static inline double* zupt_dx(orcvio_msckf_handle* h) { return h->d_covT; }
static inline int* zupt_status(orcvio_msckf_handle* h) { return reinterpret_cast<int*>(h->d_covT + h->n_max); }

// ---- one stationary frame: its record, its phases, its one outcome ---------------------------------------------------------------------
// The five calls run the same frame: propagate and augment, optionally k_zupt_check, the 9-row update, the previous clone
// marginalised, ONE wait.  What they plan and what they report: host/zupt_frame_outcome.hpp.
struct ZuptCall {
    ZuptForm form;
    const char* who;
    const orcvio_msckf_zupt* z;
    const double *Phi = nullptr, *Q = nullptr;             // the frame forms ...
    bool augment = false, remove_previous = false;
    int idp_dim = 0, n_feature_states = 0;                 // ... the hybrid forms ...
    const orcvio_msckf_zupt_check* chk = nullptr;          // ... the checked forms
    double* dx = nullptr;
    int32_t *applied = nullptr, *n_after = nullptr;
    orcvio_msckf_zupt_verdict* verdict = nullptr;
};
static ZuptCall zupt_call(ZuptForm form, const char* who, const orcvio_msckf_zupt_frame* f, const orcvio_msckf_zupt_frame_hybrid* hy,
                          double* dx, int32_t* applied, int32_t* n_after) {
    ZuptCall c{form, who, &f->zupt};
    c.Phi = f->Phi; c.Q = f->Q; c.augment = f->augment != 0; c.remove_previous = f->remove_previous != 0;
    if (hy) { c.idp_dim = hy->idp_dim; c.n_feature_states = hy->n_feature_states; }
    c.dx = dx; c.applied = applied; c.n_after = n_after;
    return c;
}

// 1. Everything that can be refused before a launch, in the order the forms have always refused it.  The check's own validation
// (zchk_prepare: it fills the job) belongs here: behind it nothing can refuse the frame any more and the head takes the arming.
static int zupt_frame_validate(const orcvio_msckf_handle* h, const ZuptCall& c, const ZuptPlan& p, ZchkJob* j) {
    const orcvio_msckf_zupt* z = c.z;
    if (c.chk) {
        if (!h->imu_armed) return zupt_refuse(c.who, ": the handle is not armed by orcvio_msckf_io_propagate_imu (whose samples the check reads)");
        if (c.Phi || c.Q) return zupt_refuse(c.who, ": Phi and Q must be NULL (they come from the armed IMU propagation)");
        if (z->leg_dim != 22) return zupt_refuse(c.who, ": leg_dim must be 22");
    } else {   // (orcvio_msckf_io_propagate_imu: Phi, Q come from k_imu_phi_q, in front of the propagation launches)
        if ((c.Phi == nullptr) != (c.Q == nullptr)) return zupt_refuse(c.who, ": Phi and Q come together");
        if (p.armed && c.Phi) return zupt_refuse(c.who, ": the handle is armed by orcvio_msckf_io_propagate_imu: Phi and Q must be NULL");
        if (p.armed && z->leg_dim != 22) return zupt_refuse(c.who, ": armed IMU propagation at leg_dim 22 only");
    }
    if (zupt_hybrid(c.form)) {
        if (c.idp_dim != 1 && c.idp_dim != 3) return zupt_refuse(c.who, ": idp_dim must be 1 or 3");
        if (c.n_feature_states < 0) return zupt_refuse(c.who, ": n_feature_states must not be negative");
        if (h->n_nui > 0) return zupt_refuse(c.who, ": not with nuisance states (ORCVIO_OPT_SCHMIDT_STATES > 0)");
    }
    { const int rv = zupt_validate(h, z, p.n, c.who); if (rv != ORCVIO_OK) return rv; }
    if (zupt_hybrid(c.form) && (long)c.idp_dim * c.n_feature_states != (long)h->n_extra)
        return zupt_refuse(c.who, ": idp_dim n_feature_states is not ORCVIO_OPT_EXTRA_STATES");
    // (with the dimensions above, cov_propagate, cov_augment and cov_remove_clones have nothing left to refuse)
    if (c.augment && h->n_extra > h->res_n - 15) return zupt_refuse(c.who, ": more extra states than the resident covariance has");
    if (!c.chk) return ORCVIO_OK;
    if (!p.check) return zchk_constants(c.chk, c.who);
    return zchk_prepare(c.chk, h->imu_after.R, h->imu_after.v, h->imu_after.ba, h->imu_cfg.gravity, h->imu_sel.data(), h->imu_S, c.who, j);
}

// 2. The launches in front of the update: propagation (given, or armed) and augmentation.  A refused armed Phi (status word) leaves P
// as it is in the propagation and refuses the update; the augmentation stands.
static int zupt_frame_head(orcvio_msckf_handle* h, const ZuptCall& c, const ZuptPlan& p) {
    HIPCHK(hipSetDevice(h->device));
    int rc = ORCVIO_OK;
    if (c.Phi) rc = orcvio_msckf_cov_propagate(h, c.z->leg_dim, c.Phi, c.Q);
    if (p.armed) {
        rc = imu_consume(h, h->stream);
        if (rc == ORCVIO_OK) rc = launch_cov_propagate(h, h->stream, h->propagate(), 22, imu_dphi(h), imu_dq(h), imu_status(h));
    }
    if (rc == ORCVIO_OK && c.augment) rc = orcvio_msckf_cov_augment(h);
    return rc;
}

// 4. The update's launches on the resident covariance (dimension n = h->res_n): P+ (the fused form: what stays of it) into the spare
// covariance buffer, S+ into the spare factor buffer, dx and the status word.  A refusal on the device leaves bit copies there, so
// what is enqueued behind this reads the prior.  Eager bookkeeping: the buffers change roles here, on the host; deferred: `edit`
// goes to CovBook::zupt_keep_done with the outcome, behind the wait.
static int zupt_enqueue(orcvio_msckf_handle* h, const ZuptCall& c, const ZuptPlan& p, CovEdit* edit) {
    const orcvio_msckf_zupt* z = c.z;
    const int n = h->res_n;
    hipStream_t s = h->stream;
    const bool fused = p.marg == ZuptMarg::in_launch;
    ZuptArgs a;
    for (int k = 0; k < 9; ++k) a.r[k] = z->r[k];
    a.noise[0] = z->noise_v; a.noise[1] = z->noise_p; a.noise[2] = z->noise_q;
    a.n = n; a.b = z->leg_dim + 6 * z->n_clones; a.nui6 = 6 * h->n_nui;
    a.also = p.also == ZuptAlso::zchk_status ? zchk_status(h) : p.also == ZuptAlso::imu_status ? imu_status(h) : nullptr;
    const ZuptKeep kp{a.b - (c.remove_previous ? 6 : 0), c.remove_previous ? a.b - 12 : a.b};   // fused: the clone at window rank N-2
    const int nt = (n + ZUPT_TILE - 1) / ZUPT_TILE, nf = (n + ZUPT_FAC_ROWS - 1) / ZUPT_FAC_ROWS;
    // (nuisance states: the restored block breaks P = S S^T, no factor)
    CovEdit e = p.eager ? h->zupt(h->n_nui == 0, ZUPT_KMAX) : h->zupt_keep(fused ? kp.m : n, h->n_nui == 0, ZUPT_KMAX);
    if (!p.eager && !fused) e.ld_out = e.ld_in;   // (cov_zupt: S+ keeps the factor's leading dimension, as CovBook::zupt has it)
    *edit = e;
    if (fused) {
        hipLaunchKernelGGL(k_zupt_cov_keep, dim3(nt, nt), dim3(256), 0, s, e.P, a, kp, e.Pout, zupt_dx(h), zupt_status(h));
        if (e.fac) hipLaunchKernelGGL(k_zupt_fac_keep, dim3(nf), dim3(256), 0, s, e.S, e.ld_in, e.fac_k, a, kp, e.ld_out, (const int*)zupt_status(h), e.Sout);
    } else {
        hipLaunchKernelGGL(k_zupt_cov, dim3(nt, nt), dim3(256), 0, s, e.P, a, e.Pout, zupt_dx(h), zupt_status(h));
        if (e.fac) hipLaunchKernelGGL(k_zupt_fac, dim3(nf), dim3(256), 0, s, e.S, e.ld_in, e.fac_k, a, (const int*)zupt_status(h), e.Sout);
    }
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// 5. / 8. the previous clone (window rank N-2) leaves: enqueued, not waited for
static int zupt_remove_previous(orcvio_msckf_handle* h, const orcvio_msckf_zupt* z) {
    const int32_t prev = z->n_clones - 2;
    return orcvio_msckf_cov_remove_clones(h, z->leg_dim, &prev, 1);
}

static int zupt_frame_run(orcvio_msckf_handle* h, const ZuptCall& c) {
    if (c.verdict) zchk_verdict_clear(c.verdict);
    const ZuptPlan p = zupt_plan(c.form, h->res_n, c.augment, c.z->leg_dim, c.z->n_clones, h->imu_armed, h->imu_S);
    ZchkJob j;
    { const int rv = zupt_frame_validate(h, c, p, &j); if (rv != ORCVIO_OK) return rv; }   // 1. refused: nothing is enqueued
    ZuptFacts f;
    f.form = c.form; f.check_ran = p.check; f.remove_previous = c.remove_previous;
    int rc = f.rc_head = zupt_frame_head(h, c, p);                                                           // 2.
    // 3. (the check's status block carries the propagation's refusal on: the update reads one block)
    if (rc == ORCVIO_OK && p.check) rc = f.rc_check = zchk_enqueue(h, h->stream, j, imu_status(h));
    const CovState before = cov_state(h);
    CovEdit e;
    if (rc == ORCVIO_OK && p.update) rc = f.rc_update = zupt_enqueue(h, c, p, &e);                           // 4.
    if (rc == ORCVIO_OK && p.marg == ZuptMarg::before_wait && c.remove_previous) rc = f.rc_marg = zupt_remove_previous(h, c.z);   // 5.
    double out[4] = {0, 0, 0, 0};
    int st[4] = {0, 0, 0, 0}, word = 0;   // word: the update's status, or without an update the armed launch's
    if (rc == ORCVIO_OK) {                                                                                   // 6. the one wait
        if (!p.update) for (int i = 0; i < p.n_dx; ++i) c.dx[i] = 0.0;
        const FetchCopy fc[] = {{c.dx, zupt_dx(h), sizeof(double) * (size_t)(p.update ? p.n_dx : 0)},
                                {&word, p.update ? zupt_status(h) : imu_status(h), sizeof(int)},
                                {out, zchk_out(h), sizeof(out)}, {st, zchk_status(h), sizeof(st)}};
        rc = f.rc_wait = fetch_copies(h, h->stream, fc, p.check ? 4 : 2);
    }
    if (rc == ORCVIO_OK) {                                                                                   // 7. the outcome
        f.upd = p.update ? word : 0;
        f.imu_refused = p.update ? p.also == ZuptAlso::imu_status && imu_refused(h) : word != 0;
        if (p.check) { f.rc_verdict = zchk_verdict(j, out, st[2], c.who, c.verdict); f.evaluated = c.verdict->evaluated != 0; f.accept = c.verdict->accept != 0; }
    }
    ZuptOutcome o = zupt_frame_outcome(p, f, ORCVIO_OK, ORCVIO_ERR_NOT_SPD);
    zupt_book_apply(*h, before, e, o);                                                                       // 8.
    // (behind the wait, and only now that the update is known to be applied)
    if (o.marg_behind) zupt_frame_outcome_marg(p, o, zupt_remove_previous(h, c.z), ORCVIO_OK);
    if (o.write_applied) *c.applied = o.applied;
    if (o.write_n_after) *c.n_after = o.n_after;
    if (const char* text = zupt_message(o.msg)) g_last_error = std::string(c.who) + text;
    return o.ret;
}

int32_t orcvio_msckf_cov_zupt(orcvio_msckf_handle* h, const orcvio_msckf_zupt* z, double* dx, int32_t* applied) {
    if (!h || !z || !dx || !applied) { g_last_error = "cov_zupt: null argument"; return ORCVIO_ERR_INVALID; }
    ZuptCall c{ZuptForm::update, "cov_zupt", z};
    c.dx = dx; c.applied = applied;
    return zupt_frame_run(h, c);
}

int32_t orcvio_msckf_cov_zupt_frame(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame* f, double* dx, int32_t* applied, int32_t* n_after) {
    if (!h || !f || !dx || !applied || !n_after) { g_last_error = "cov_zupt_frame: null argument"; return ORCVIO_ERR_INVALID; }
    return zupt_frame_run(h, zupt_call(ZuptForm::frame, "cov_zupt_frame", f, nullptr, dx, applied, n_after));
}

// The stationary frame of a hybrid filter: every in-state feature leaves in front of the update (checkZUPTFeat :3102-3119, checkZUPTIMU
// :3302-3319), the previous clone behind it -- ONE launch that writes what stays (k_zupt_cov_keep / k_zupt_fac_keep)
int32_t orcvio_msckf_cov_zupt_frame_hybrid(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame_hybrid* hy, double* dx, int32_t* applied,
                                           int32_t* n_after) {
    if (!h || !hy || !dx || !applied || !n_after) { g_last_error = "cov_zupt_frame_hybrid: null argument"; return ORCVIO_ERR_INVALID; }
    return zupt_frame_run(h, zupt_call(ZuptForm::frame_hybrid, "cov_zupt_frame_hybrid", &hy->frame, hy, dx, applied, n_after));
}

// The checked forms, on a handle armed by orcvio_msckf_io_propagate_imu: k_zupt_check in front of the update it decides on
int32_t orcvio_msckf_cov_zupt_frame_checked(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame* f, const orcvio_msckf_zupt_check* chk,
                                            double* dx, int32_t* applied, int32_t* n_after, orcvio_msckf_zupt_verdict* verdict) {
    if (!h || !f || !chk || !dx || !applied || !n_after || !verdict) { g_last_error = "cov_zupt_frame_checked: null argument"; return ORCVIO_ERR_INVALID; }
    ZuptCall c = zupt_call(ZuptForm::checked, "cov_zupt_frame_checked", f, nullptr, dx, applied, n_after);
    c.chk = chk; c.verdict = verdict;
    return zupt_frame_run(h, c);
}

int32_t orcvio_msckf_cov_zupt_frame_checked_hybrid(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame_hybrid* hy, const orcvio_msckf_zupt_check* chk,
                                                   double* dx, int32_t* applied, int32_t* n_after, orcvio_msckf_zupt_verdict* verdict) {
    if (!h || !hy || !chk || !dx || !applied || !n_after || !verdict) { g_last_error = "cov_zupt_frame_checked_hybrid: null argument"; return ORCVIO_ERR_INVALID; }
    ZuptCall c = zupt_call(ZuptForm::checked_hybrid, "cov_zupt_frame_checked_hybrid", &hy->frame, hy, dx, applied, n_after);
    c.chk = chk; c.verdict = verdict;
    return zupt_frame_run(h, c);
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
