// capi_imu_calib.inc -- part of msckf_capi.hip (ONE translation unit: included there behind capi_imu.inc; not compiled on its own).
// IMU propagation from raw samples at leg_dim 46 (calib_imu_instrinsic = 1): the imu_*46 host half of host/imu_model.hpp,
// k_imu_phi_q46 (imu_ops.hpp), then the propagation launches of orcvio_msckf_cov_propagate at 46 on the pair the kernel left on the
// device.  The status word, the staging slots of Phi / Q and the state conversion are capi_imu.inc's.

// the host half at 46, on COPIES of the state and of prev_meas; recs [<= 128][IMU_REC46]
static int imu_host_half46(const orcvio_msckf_imu_config* cfg, const ImuIntrinsicMx& mx, const orcvio_msckf_imu_state* state, const double* prev_meas,
                           const double* samples, int n_samples, double time_bound, ImuMeanState* st, double* prev, double* recs,
                           ImuBatchInfo* bi, ImuFlags* fl, const char* who) {
    ImuModelConfig mc{};
    mc.flags = ImuFlags{cfg->use_larvio ? 1 : 0, cfg->use_left_perturbation ? 1 : 0, cfg->use_closed_form ? 1 : 0, cfg->if_fej ? 1 : 0};
    for (int i = 0; i < 3; ++i) mc.gravity[i] = cfg->gravity[i];
    mc.imu_img_time_th = cfg->imu_img_time_th;
    *fl = mc.flags;
    imu_state_in(state, st);
    for (int i = 0; i < 6; ++i) prev[i] = prev_meas[i];
    if (!imu_propagate_mean46(mc, mx, st, prev, samples, n_samples, time_bound, recs, IMU_MAX_SAMPLES, bi)) {
        g_last_error = std::string(who) + ": more than 128 IMU samples selected";
        return ORCVIO_ERR_CAPACITY;
    }
    return ORCVIO_OK;
}

static ImuKernArgs46 imu_args46(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg, ImuFlags fl, const ImuIntrinsicMx& mx, int S,
                                double* dPhi, double* dQ) {
    ImuKernArgs46 a{};
    a.recs = h->d_imu46; a.Phi = dPhi; a.Q = dQ; a.status = imu_status(h); a.S = S; a.flags = fl; a.mx = mx;
    for (int i = 0; i < 3; ++i) a.grav[i] = cfg->gravity[i];
    for (int i = 0; i < 12; ++i) a.qc[i] = cfg->Q_c_diag[i];
    return a;
}
// the records to the device (through the pinned bounce buffer) and the launch; Phi, Q [46][46] land at dPhi, dQ
static int imu_enqueue46(orcvio_msckf_handle* h, hipStream_t s, const orcvio_msckf_imu_config* cfg, ImuFlags fl, const ImuIntrinsicMx& mx,
                         const double* recs, int S, double* dPhi, double* dQ) {
    const AuxCopy cp[] = {{h->d_imu46, recs, sizeof(double) * (size_t)S * IMU_REC46}};
    { const int rc = aux_copies(h, s, cp, 1); if (rc != ORCVIO_OK) return rc; }
    hipLaunchKernelGGL(k_imu_phi_q46, dim3(1), dim3(64 * IMU_WAVES), imu46_lds_bytes(), s, imu_args46(h, cfg, fl, mx, S, dPhi, dQ));
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

int32_t orcvio_msckf_cov_propagate_imu_calib(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg,
                                             const orcvio_msckf_imu_intrinsics* intr, orcvio_msckf_imu_state* state, double* prev_meas,
                                             const double* samples, int32_t n_samples, double time_bound, orcvio_msckf_imu_info* info,
                                             double* Phi_out, double* Q_out) {
    const std::string w("cov_propagate_imu_calib");
    if (!h || !cfg || !intr || !state || !prev_meas || !info || n_samples < 0 || (n_samples > 0 && !samples)) { g_last_error = w + ": null argument"; return ORCVIO_ERR_INVALID; }
    if (cfg->leg_dim != 46) { g_last_error = w + ": leg_dim must be 46 (orcvio_msckf_cov_propagate_imu serves 22)"; return ORCVIO_ERR_INVALID; }
    for (int i = 0; i < IMU_NI; ++i)
        if (!std::isfinite(intr->x[i])) { g_last_error = w + ": an IMU intrinsic is not finite"; return ORCVIO_ERR_INVALID; }
    if (h->res_n < 46) { g_last_error = w + ": no resident covariance of at least 46 states"; return ORCVIO_ERR_INVALID; }
    if ((Phi_out == nullptr) != (Q_out == nullptr)) { g_last_error = w + ": Phi_out and Q_out come together"; return ORCVIO_ERR_INVALID; }
    if (h->imu_armed) { g_last_error = w + ": the handle is armed by orcvio_msckf_io_propagate_imu (its records wait for the frame call)"; return ORCVIO_ERR_INVALID; }
    ImuIntrinsicMx mx;
    imu_intrinsic_mx(intr->x, &mx);
    ImuMeanState st;
    double prev[6];
    double* recs = h->imu_recs46.data();
    ImuBatchInfo bi{};
    ImuFlags fl{};
    const int rh = imu_host_half46(cfg, mx, state, prev_meas, samples, n_samples, time_bound, &st, prev, recs, &bi, &fl, w.c_str());
    info->n_used = bi.n_used; info->n_propagated = bi.n_propagated; info->dt = bi.dt; info->applied = 0;
    for (int i = 0; i < 3; ++i) info->mean_sforce[i] = bi.mean_sforce[i];
    if (rh != ORCVIO_OK) return rh;
    const int S = bi.n_propagated;
    if (S == 0) {   // nothing selected: no launch, the covariance untouched
        imu_state_out(st, state);
        if (Phi_out)
            for (int i = 0; i < 46 * 46; ++i) { Phi_out[i] = (i / 46 == i % 46) ? 1.0 : 0.0; Q_out[i] = 0.0; }
        return ORCVIO_OK;
    }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    double* dPhi = imu_dphi(h);
    double* dQ = imu_dq(h);
    { const int rc = imu_enqueue46(h, s, cfg, fl, mx, recs, S, dPhi, dQ); if (rc != ORCVIO_OK) return rc; }
    { const int rc = launch_cov_propagate(h, s, h->propagate(), 46, dPhi, dQ, imu_status(h)); if (rc != ORCVIO_OK) return rc; }
    imu_state_out(st, state);
    for (int i = 0; i < 6; ++i) prev_meas[i] = prev[i];
    info->applied = 1;
    if (!info->wait && !Phi_out) return ORCVIO_OK;
    int refused = 0;
    const FetchCopy fc[] = {{Phi_out, dPhi, sizeof(double) * 46 * 46}, {Q_out, dQ, sizeof(double) * 46 * 46}, {&refused, imu_status(h), sizeof(int)}};
    { const int rc = fetch_copies(h, s, fc, 3); if (rc != ORCVIO_OK) return rc; }
    if (refused) {
        info->applied = 0;
        g_last_error = w + ": Phi or Q not finite (the right closed form with a zero gyro sample): the covariance was not propagated";
        return ORCVIO_ERR_NOT_SPD;
    }
    return ORCVIO_OK;
}
