// capi_imu.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// IMU propagation from raw samples (batchImuProcessing -> processModel, src/orcvio.cpp:664-823): the host half of host/imu_model.hpp,
// k_imu_phi_q (imu_ops.hpp), then the propagation launches of orcvio_msckf_cov_propagate on the pair the kernel left on the device.

// the kernel's status word stands behind the per-sample records (d_imu: allocated at create, with the kernel's dynamic-LDS opt-in)
static inline int* imu_status(orcvio_msckf_handle* h) { return reinterpret_cast<int*>(h->d_imu + (size_t)IMU_MAX_SAMPLES * IMU_REC); }

static void imu_state_in(const orcvio_msckf_imu_state* s, ImuMeanState* m) {
    m->time = s->time;
    for (int i = 0; i < 9; ++i) m->R[i] = s->R_b2w[i];
    for (int i = 0; i < 3; ++i) {
        m->v[i] = s->v[i]; m->p[i] = s->p[i]; m->bg[i] = s->gyro_bias[i]; m->ba[i] = s->acc_bias[i];
        m->v_fej[i] = s->v_fej[i]; m->p_fej[i] = s->p_fej[i];
    }
}
static void imu_state_out(const ImuMeanState& m, orcvio_msckf_imu_state* s) {
    s->time = m.time;
    for (int i = 0; i < 9; ++i) s->R_b2w[i] = m.R[i];
    for (int i = 0; i < 3; ++i) { s->v[i] = m.v[i]; s->p[i] = m.p[i]; s->v_fej[i] = m.v_fej[i]; s->p_fej[i] = m.p_fej[i]; }
}

// The host half: selection and one predictor per sample on COPIES of the state and of prev_meas (the caller's are written when nothing
// can refuse the call any more); recs [<= 128][IMU_REC].
static int imu_host_half(const orcvio_msckf_imu_config* cfg, const orcvio_msckf_imu_state* state, const double* prev_meas, const double* samples,
                         int n_samples, double time_bound, ImuMeanState* st, double* prev, double* recs, ImuBatchInfo* bi,
                         ImuFlags* fl, const char* who) {
    ImuModelConfig mc{};
    mc.flags = ImuFlags{cfg->use_larvio ? 1 : 0, cfg->use_left_perturbation ? 1 : 0, cfg->use_closed_form ? 1 : 0, cfg->if_fej ? 1 : 0};
    for (int i = 0; i < 3; ++i) mc.gravity[i] = cfg->gravity[i];
    mc.imu_img_time_th = cfg->imu_img_time_th;
    *fl = mc.flags;
    imu_state_in(state, st);
    for (int i = 0; i < 6; ++i) prev[i] = prev_meas[i];
    if (!imu_propagate_mean(mc, st, prev, samples, n_samples, time_bound, recs, IMU_MAX_SAMPLES, bi)) {
        g_last_error = std::string(who) + ": more than 128 IMU samples selected";
        return ORCVIO_ERR_CAPACITY;
    }
    return ORCVIO_OK;
}

// the records to the device (through the pinned bounce buffer: nothing to wait for) and the launch; Phi, Q [22][22] land at dPhi, dQ
static int imu_enqueue(orcvio_msckf_handle* h, hipStream_t s, const orcvio_msckf_imu_config* cfg, ImuFlags fl, const double* recs, int S,
                       double* dPhi, double* dQ, int* status_host = nullptr) {
    const AuxCopy cp[] = {{h->d_imu, recs, sizeof(double) * (size_t)S * IMU_REC}};
    { const int rc = aux_copies(h, s, cp, 1); if (rc != ORCVIO_OK) return rc; }
    ImuKernArgs a{};
    a.recs = h->d_imu; a.Phi = dPhi; a.Q = dQ; a.status = imu_status(h); a.status_host = status_host; a.S = S; a.flags = fl;
    for (int i = 0; i < 3; ++i) a.grav[i] = cfg->gravity[i];
    for (int i = 0; i < 12; ++i) a.qc[i] = cfg->Q_c_diag[i];
    hipLaunchKernelGGL(k_imu_phi_q, dim3(1), dim3(64 * IMU_WAVES), imu_lds_bytes(S), s, a);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
// where orcvio_msckf_cov_propagate stages Phi, then Q: the slots launch_cov_propagate and an armed frame's head read
static inline double* imu_dphi(orcvio_msckf_handle* h) { return h->d_covT + (size_t)46 * h->n_max; }
static inline double* imu_dq(orcvio_msckf_handle* h) { return imu_dphi(h) + 46 * 46; }
// An armed frame call takes the arming: k_imu_phi_q goes out on `s` in front of the frame's head launch, its status also into the
// host-coherent word the call reads behind its one wait (imu_refused).
static int imu_consume(orcvio_msckf_handle* h, hipStream_t s) {
    h->imu_armed = false;
    *h->h_imu_status = 0;
    return imu_enqueue(h, s, &h->imu_cfg, h->imu_fl, h->imu_recs.data(), h->imu_S, imu_dphi(h), imu_dq(h), h->h_imu_status_dev);
}
static inline bool imu_refused(const orcvio_msckf_handle* h) { return *reinterpret_cast<const volatile int*>(h->h_imu_status) != 0; }

// The samples the host half selected (:678-709), in order: they ARE imu_recent_zupt (:676-690), what the zero-velocity check reads.
// t0: state.time before the host half; sel [S][7].
static void imu_selected(const double* samples, int n, double t0, int S, double* sel) {
    double cur = t0;
    int s = 0;
    for (int k = 0; k < n && s < S; ++k) {
        if (samples[k * 7] <= cur) continue;
        for (int i = 0; i < 7; ++i) sel[(size_t)s * 7 + i] = samples[k * 7 + i];
        cur = samples[k * 7];
        ++s;
    }
}

// the zero-velocity check behind the propagation (capi_zupt_check.inc, which follows in the translation unit)
static int zchk_prepare(const orcvio_msckf_zupt_check* c, const double* R, const double* v, const double* ba, const double* g,
                        const double* samples, int S, const char* who, ZuptCheckJob* j);
static int zchk_enqueue(orcvio_msckf_handle* h, hipStream_t s, const ZuptCheckJob& j, const int* also);
static int zchk_verdict(const ZuptCheckJob& j, const double* out, int st, const char* who, orcvio_msckf_zupt_verdict* v);
static inline double* zchk_out(orcvio_msckf_handle* h);
static inline int* zchk_status(orcvio_msckf_handle* h);

// orcvio_msckf_cov_propagate_imu (chk = NULL) and orcvio_msckf_cov_propagate_imu_checked: the same host half and launches, the checked
// form with k_zupt_check behind the propagation launches and ONE wait for both
static int imu_propagate_call(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg, orcvio_msckf_imu_state* state,
                              double* prev_meas, const double* samples, int32_t n_samples, double time_bound,
                              orcvio_msckf_imu_info* info, double* Phi_out, double* Q_out,
                              const orcvio_msckf_zupt_check* chk, orcvio_msckf_zupt_verdict* verdict, const char* who) {
    const std::string w(who);
    if (!h || !cfg || !state || !prev_meas || !info || n_samples < 0 || (n_samples > 0 && !samples)) { g_last_error = w + ": null argument"; return ORCVIO_ERR_INVALID; }
    if (cfg->leg_dim != 22) { g_last_error = w + ": leg_dim must be 22 (this call has no intrinsics to read: orcvio_msckf_cov_propagate_imu_calib serves 46, without the check)"; return ORCVIO_ERR_INVALID; }
    if (h->res_n < 22) { g_last_error = w + ": no resident covariance"; return ORCVIO_ERR_INVALID; }
    if ((Phi_out == nullptr) != (Q_out == nullptr)) { g_last_error = w + ": Phi_out and Q_out come together"; return ORCVIO_ERR_INVALID; }
    if (h->imu_armed) { g_last_error = w + ": the handle is armed by orcvio_msckf_io_propagate_imu (its records wait for the frame call)"; return ORCVIO_ERR_INVALID; }
    ImuMeanState st;
    double prev[6];
    double* recs = h->imu_recs.data();
    ImuBatchInfo bi{};
    ImuFlags fl{};
    const double t0 = state->time;
    const int rh = imu_host_half(cfg, state, prev_meas, samples, n_samples, time_bound, &st, prev, recs, &bi, &fl, who);
    info->n_used = bi.n_used; info->n_propagated = bi.n_propagated; info->dt = bi.dt; info->applied = 0;
    for (int i = 0; i < 3; ++i) info->mean_sforce[i] = bi.mean_sforce[i];
    if (rh != ORCVIO_OK) return rh;
    const int S = bi.n_propagated;
    if (S == 0) {   // nothing selected: no launch, the covariance untouched
        imu_state_out(st, state);
        if (Phi_out)
            for (int i = 0; i < 22 * 22; ++i) { Phi_out[i] = (i / 22 == i % 22) ? 1.0 : 0.0; Q_out[i] = 0.0; }
        return ORCVIO_OK;
    }
    const bool check = chk && S >= 2;   // (one selected sample: :3134, nothing to test with)
    if (check) {   // the check's own validation, with *state and prev_meas still untouched: the PROPAGATED state, the selected samples
        imu_selected(samples, n_samples, t0, S, h->imu_sel.data());
        const int rc = zchk_prepare(chk, st.R, st.v, st.ba, cfg->gravity, h->imu_sel.data(), S, who, &h->zchk_job);
        if (rc != ORCVIO_OK) return rc;
    }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    double* dPhi = imu_dphi(h);
    double* dQ = imu_dq(h);
    { const int rc = imu_enqueue(h, s, cfg, fl, recs, S, dPhi, dQ); if (rc != ORCVIO_OK) return rc; }
    { const int rc = launch_cov_propagate(h, s, h->propagate(), 22, dPhi, dQ, imu_status(h)); if (rc != ORCVIO_OK) return rc; }
    imu_state_out(st, state);
    for (int i = 0; i < 6; ++i) prev_meas[i] = prev[i];
    info->applied = 1;
    if (check) { const int rc = zchk_enqueue(h, s, h->zchk_job, imu_status(h)); if (rc != ORCVIO_OK) return rc; }
    if (!chk && !info->wait && !Phi_out) return ORCVIO_OK;
    int refused = 0;
    double out[4] = {0, 0, 0, 0};
    int zst[4] = {0, 0, 0, 0};
    const FetchCopy fc[] = {{Phi_out, dPhi, sizeof(double) * 22 * 22}, {Q_out, dQ, sizeof(double) * 22 * 22}, {&refused, imu_status(h), sizeof(int)},
                            {out, zchk_out(h), sizeof(out)}, {zst, zchk_status(h), sizeof(zst)}};
    { const int rc = fetch_copies(h, s, fc, check ? 5 : 3); if (rc != ORCVIO_OK) return rc; }
    if (check) (void)zchk_verdict(h->zchk_job, out, zst[2], who, verdict);   // (behind a refused Phi: evaluated = 0, ORCVIO_ERR_NOT_SPD)
    if (refused) {
        info->applied = 0;
        g_last_error = w + ": Phi or Q not finite (the right closed form with a zero gyro sample): the covariance was not propagated";
        return ORCVIO_ERR_NOT_SPD;
    }
    return check ? verdict->status : ORCVIO_OK;
}

int32_t orcvio_msckf_cov_propagate_imu(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg, orcvio_msckf_imu_state* state,
                                       double* prev_meas, const double* samples, int32_t n_samples, double time_bound,
                                       orcvio_msckf_imu_info* info, double* Phi_out, double* Q_out) {
    return imu_propagate_call(h, cfg, state, prev_meas, samples, n_samples, time_bound, info, Phi_out, Q_out, nullptr, nullptr, "cov_propagate_imu");
}

// Arms the next orcvio_msckf_io_step_frame / _io_step_frame_ex / _cov_zupt_frame on the handle, in the manner of
// orcvio_msckf_io_triangulate: the host half runs NOW (*state, prev_meas and info are valid on return), nothing is enqueued.
int32_t orcvio_msckf_io_propagate_imu(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg, orcvio_msckf_imu_state* state,
                                      double* prev_meas, const double* samples, int32_t n_samples, double time_bound,
                                      orcvio_msckf_imu_info* info) {
    if (!h || !cfg || !state || !prev_meas || !info || n_samples < 0 || (n_samples > 0 && !samples)) { g_last_error = "io_propagate_imu: null argument"; return ORCVIO_ERR_INVALID; }
    if (cfg->leg_dim != 22) { g_last_error = "io_propagate_imu: leg_dim must be 22 (the armed form has no 46: orcvio_msckf_cov_propagate_imu_calib in front of the frame call)"; return ORCVIO_ERR_INVALID; }
    if (h->res_n < 22) { g_last_error = "io_propagate_imu: no resident covariance"; return ORCVIO_ERR_INVALID; }
    if (h->comm || h->ipc) { g_last_error = "io_propagate_imu: not with a communicator on the handle"; return ORCVIO_ERR_INVALID; }
    if (h->imu_armed) { g_last_error = "io_propagate_imu: the handle is armed already"; return ORCVIO_ERR_INVALID; }
    ImuMeanState st;
    double prev[6];
    ImuBatchInfo bi{};
    ImuFlags fl{};
    const double t0 = state->time;
    const int rh = imu_host_half(cfg, state, prev_meas, samples, n_samples, time_bound, &st, prev, h->imu_recs.data(), &bi, &fl, "io_propagate_imu");
    info->n_used = bi.n_used; info->n_propagated = bi.n_propagated; info->dt = bi.dt; info->applied = 0;   // (applied: nothing is, yet)
    for (int i = 0; i < 3; ++i) info->mean_sforce[i] = bi.mean_sforce[i];
    if (rh != ORCVIO_OK) return rh;
    imu_state_out(st, state);
    if (bi.n_propagated == 0) return ORCVIO_OK;   // nothing selected: nothing armed, the frame call runs without propagation
    for (int i = 0; i < 6; ++i) prev_meas[i] = prev[i];
    h->imu_armed = true; h->imu_S = bi.n_propagated; h->imu_fl = fl; h->imu_cfg = *cfg;
    // what orcvio_msckf_cov_zupt_frame_checked tests: the selected samples and the propagated state
    imu_selected(samples, n_samples, t0, bi.n_propagated, h->imu_sel.data());
    h->imu_after = st;
    return ORCVIO_OK;
}
