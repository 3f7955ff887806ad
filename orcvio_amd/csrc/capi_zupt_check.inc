// capi_zupt_check.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// Zero-velocity DETECTION from IMU samples on the resident covariance (checkZUPTIMU, src/orcvio.cpp:3129-3323): the packing and the
// validation of host/zupt_check_model.hpp, k_zupt_check (zupt_check_ops.hpp), its verdict, and two of its three call sites -- stand-alone
// and behind the propagation from raw samples.  The third, inside the stationary frame in front of the update it decides on, is
// capi_zupt.inc's (zupt_frame_run), which follows in the translation unit and uses the zchk_* helpers here.

void orcvio_msckf_zupt_check_default(orcvio_msckf_zupt_check* c) {
    if (!c) return;
    c->sigma_w2 = 1.6968e-04 * 1.6968e-04; c->sigma_a2 = 2.0000e-3 * 2.0000e-3;   // :3140-3142
    c->sigma_wb = 1.9393e-05; c->sigma_ab = 3.0000e-03;                           // :3144-3146
    c->chi2_prob = 0.95; c->chi2_multiplier = 1.0; c->max_velocity = 0.25;
    c->use_left_perturbation = 0;
}

// d_zchk: the packed rows [128][ZCHK_ROW], then chi^2 | c | dt_sum | limit (eight doubles reserved), then the sixteen status words
static inline double* zchk_out(orcvio_msckf_handle* h) { return h->d_zchk + (size_t)ZCHK_MAX_SAMPLES * ZCHK_ROW; }
static inline int* zchk_status(orcvio_msckf_handle* h) { return reinterpret_cast<int*>(zchk_out(h) + 8); }

using ZchkJob = ZuptCheckJob;

static void zchk_verdict_clear(orcvio_msckf_zupt_verdict* v) {
    v->evaluated = 0; v->accept = 0; v->dof = 0; v->status = ORCVIO_OK;
    v->chi2 = 0.0; v->chi2_check = 0.0; v->speed = 0.0;
}

static int zchk_constants(const orcvio_msckf_zupt_check* c, const char* who) {
    const double pos[5] = {c->sigma_w2, c->sigma_a2, c->sigma_wb, c->sigma_ab, c->max_velocity};
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(pos[i]) || !(pos[i] > 0.0)) { g_last_error = std::string(who) + ": the noise constants and max_velocity must be finite and positive"; return ORCVIO_ERR_INVALID; }
    if (!(c->chi2_prob > 0.0) || !(c->chi2_prob < 1.0)) { g_last_error = std::string(who) + ": chi2_prob must lie inside (0, 1)"; return ORCVIO_ERR_INVALID; }
    if (!std::isfinite(c->chi2_multiplier) || !(c->chi2_multiplier > 0.0)) { g_last_error = std::string(who) + ": chi2_multiplier must be finite and positive"; return ORCVIO_ERR_INVALID; }
    return ORCVIO_OK;
}

// Everything that can be refused before a launch, S >= 2 samples [S][7].  Fills the job (rows, threshold, the speed test).
static int zchk_prepare(const orcvio_msckf_zupt_check* c, const double* R, const double* v, const double* ba, const double* g,
                        const double* samples, int S, const char* who, ZchkJob* j) {
    { const int rc = zchk_constants(c, who); if (rc != ORCVIO_OK) return rc; }
    if (S > ZCHK_MAX_SAMPLES) { g_last_error = std::string(who) + ": more than 128 IMU samples"; return ORCVIO_ERR_CAPACITY; }
    if (!all_finite(R, 9) || !all_finite(v, 3) || !all_finite(ba, 3) || !all_finite(g, 3)) { g_last_error = std::string(who) + ": non-finite state or gravity"; return ORCVIO_ERR_INVALID; }
    if (!all_finite(samples, (size_t)S * 7)) { g_last_error = std::string(who) + ": non-finite IMU sample"; return ORCVIO_ERR_INVALID; }
    if (zupt_check_pack(samples, S, j->rows) != 0) {
        g_last_error = std::string(who) + ": the sample times must increase strictly (the reference divides by t[i+1] - t[i] and accepts on the NaN)";
        return ORCVIO_ERR_INVALID;
    }
    j->k = ZuptCheckConsts{c->sigma_w2, c->sigma_a2, c->sigma_wb, c->sigma_ab, c->use_left_perturbation ? 1 : 0};
    for (int i = 0; i < 9; ++i) j->R[i] = R[i];
    for (int i = 0; i < 3; ++i) { j->ba[i] = ba[i]; j->g[i] = g[i]; }
    j->m = S - 1; j->dof = 6 * (S - 1);
    j->threshold = orcvio_msckf_chi2_quantile(j->dof, c->chi2_prob);
    j->limit = c->chi2_multiplier * j->threshold;
    j->speed = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    j->max_velocity = c->max_velocity;
    j->force_reject = j->speed > c->max_velocity ? 1 : 0;
    return ORCVIO_OK;
}

// the rows to the device (through the pinned bounce buffer: nothing to wait for) and the launch, on the resident P as the stream leaves it
static int zchk_enqueue(orcvio_msckf_handle* h, hipStream_t s, const ZchkJob& j, const int* also) {
    const AuxCopy cp[] = {{h->d_zchk, j.rows, sizeof(double) * (size_t)j.m * ZCHK_ROW}};
    { const int rc = aux_copies(h, s, cp, 1); if (rc != ORCVIO_OK) return rc; }
    ZuptCheckArgs a{};
    a.P = h->d_Pres; a.rows = h->d_zchk; a.out = zchk_out(h); a.status = zchk_status(h); a.also = also;
    a.n = h->res_n; a.m = j.m; a.force_reject = j.force_reject; a.limit = j.limit;
    for (int i = 0; i < 9; ++i) a.R[i] = j.R[i];
    for (int i = 0; i < 3; ++i) { a.ba[i] = j.ba[i]; a.g[i] = j.g[i]; }
    a.k = j.k;
    hipLaunchKernelGGL(k_zupt_check, dim3(1), dim3(ZCHK_THREADS), 0, s, a);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// the verdict from what the kernel left (out [4], its status word); returns ORCVIO_OK or ORCVIO_ERR_NOT_SPD behind a device refusal
static int zchk_verdict(const ZchkJob& j, const double* out, int st, const char* who, orcvio_msckf_zupt_verdict* v) {
    v->dof = j.dof; v->chi2_check = j.threshold; v->speed = j.speed;
    v->evaluated = (st == ZCHK_OK || st == ZCHK_REJECTED) ? 1 : 0;
    v->accept = st == ZCHK_OK ? 1 : 0;
    v->chi2 = v->evaluated ? out[0] : 0.0;
    v->status = v->evaluated ? ORCVIO_OK : ORCVIO_ERR_NOT_SPD;
    if (v->evaluated) return ORCVIO_OK;
    g_last_error = std::string(who) + (st == ZCHK_UPSTREAM ? ": Phi or Q of the IMU propagation in front not finite: not evaluated"
                                      : st == ZCHK_NOT_FINITE ? ": a non-finite entry in the 9 x 9 marginal of P: not evaluated"
                                                              : ": the marginal of P (or I + L^T A L) is not positive definite: not evaluated");
    return ORCVIO_ERR_NOT_SPD;
}

int32_t orcvio_msckf_cov_zupt_check_imu(orcvio_msckf_handle* h, const orcvio_msckf_zupt_check* chk, const double* R_b2w, const double* v,
                                        const double* acc_bias, const double* gravity, const double* samples, int32_t n_samples,
                                        orcvio_msckf_zupt_verdict* verdict) {
    if (!h || !chk || !R_b2w || !v || !acc_bias || !gravity || !verdict || n_samples < 0 || (n_samples > 0 && !samples)) { g_last_error = "cov_zupt_check_imu: null argument"; return ORCVIO_ERR_INVALID; }
    zchk_verdict_clear(verdict);
    if (h->res_n < 22) { g_last_error = "cov_zupt_check_imu: no resident covariance"; return ORCVIO_ERR_INVALID; }
    if (h->comm || h->ipc) { g_last_error = "cov_zupt_check_imu: not with a communicator on the handle"; return ORCVIO_ERR_INVALID; }
    if (n_samples < 2) {   // :3134: nothing to test with -- no launch (the constants are validated all the same)
        return zchk_constants(chk, "cov_zupt_check_imu");
    }
    ZchkJob j;
    { const int rc = zchk_prepare(chk, R_b2w, v, acc_bias, gravity, samples, n_samples, "cov_zupt_check_imu", &j); if (rc != ORCVIO_OK) return rc; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    { const int rc = zchk_enqueue(h, s, j, nullptr); if (rc != ORCVIO_OK) return rc; }
    double out[4] = {0, 0, 0, 0};
    int st[4] = {0, 0, 0, 0};
    const FetchCopy fc[] = {{out, zchk_out(h), sizeof(out)}, {st, zchk_status(h), sizeof(st)}};
    { const int rc = fetch_copies(h, s, fc, 2); if (rc != ORCVIO_OK) return rc; }
    return zchk_verdict(j, out, st[2], "cov_zupt_check_imu", verdict);
}

int32_t orcvio_msckf_cov_propagate_imu_checked(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg, orcvio_msckf_imu_state* state,
                                               double* prev_meas, const double* samples, int32_t n_samples, double time_bound,
                                               orcvio_msckf_imu_info* info, double* Phi_out, double* Q_out,
                                               const orcvio_msckf_zupt_check* chk, orcvio_msckf_zupt_verdict* verdict) {
    if (!chk || !verdict) { g_last_error = "cov_propagate_imu_checked: null argument"; return ORCVIO_ERR_INVALID; }
    zchk_verdict_clear(verdict);
    if (h && (h->comm || h->ipc)) { g_last_error = "cov_propagate_imu_checked: not with a communicator on the handle"; return ORCVIO_ERR_INVALID; }
    { const int rc = zchk_constants(chk, "cov_propagate_imu_checked"); if (rc != ORCVIO_OK) return rc; }
    return imu_propagate_call(h, cfg, state, prev_meas, samples, n_samples, time_bound, info, Phi_out, Q_out, chk, verdict, "cov_propagate_imu_checked");
}
