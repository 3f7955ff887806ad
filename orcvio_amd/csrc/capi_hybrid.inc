// capi_hybrid.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// EKF-SLAM rows of the hybrid filter, features entering the state, the H_1 / H_2 tail.

// ---- EKF-SLAM rows (SURVEY.md 8f rank 3) ---------------------------------------------------------------------
static int ekf_reserve(orcvio_msckf_handle* h, int F) {
    if (F <= h->ekf_cap) return ORCVIO_OK;
    HIPCHK(hipDeviceSynchronize());
    void* old[] = {h->d_ekf_i, h->d_ekf_d, h->d_ekf_E, h->d_ekf_gamma, h->d_ekf_accept, h->d_slam};
    for (void* q : old) if (q) (void)hipFree(q);
    const int cap = round_up(F, 32);
    HIPCHK(hipMalloc(&h->d_ekf_i, sizeof(int) * 3 * cap));
    HIPCHK(hipMalloc(&h->d_ekf_d, sizeof(double) * 46 * cap));
    HIPCHK(hipMalloc(&h->d_ekf_E, sizeof(double) * (size_t)2 * cap * h->NAP_max));
    HIPCHK(hipMalloc(&h->d_ekf_gamma, sizeof(double) * cap));
    HIPCHK(hipMalloc(&h->d_ekf_accept, sizeof(int) * cap));
    HIPCHK(hipMalloc(&h->d_slam, sizeof(double) * 12 * cap));
    if (!h->d_Gekf) HIPCHK(hipMalloc(&h->d_Gekf, sizeof(double) * (size_t)2 * h->NAP_max * h->NAP_max));
    h->ekf_cap = cap;
    h->graph_epoch++;   // captured graphs hold the freed pointers
    return ORCVIO_OK;
}

// validation of the in-state features' records and the device buffers for them; the nine (destination, source, bytes) triples of the
// records (shared by orcvio_msckf_upload_slam_features, which copies them, and orcvio_msckf_io_step_frame, whose first launch pulls them)
static int slam_prepare(orcvio_msckf_handle* h, const orcvio_msckf_slam_features* ft) {
    // (behind orcvio_msckf_upload, or between orcvio_msckf_io_begin and orcvio_msckf_io_update / _io_submit: the window's sizes are known)
    if (!h || !ft || !(h->uploaded || h->io_open)) { g_last_error = "upload_slam_features: upload the window first"; return ORCVIO_ERR_INVALID; }
    if (!h->ekf_mode) { g_last_error = "upload_slam_features: set ORCVIO_OPT_EKF_ROWS before the upload"; return ORCVIO_ERR_INVALID; }
    const int F = ft->n_features, d = ft->idp_dim;
    if (F < 0 || (d != 1 && d != 3)) { g_last_error = "upload_slam_features: idp_dim must be 1 or 3"; return ORCVIO_ERR_INVALID; }
    if (F > 0 && (!ft->anchor || !ft->state || !ft->slot || !ft->param || !ft->p_w || !ft->z || (d == 1 && !ft->inv_depth) ||
                  (h->flags.if_fej && !ft->p_fej) || (h->flags.estimate_td && !ft->z_vel))) { g_last_error = "upload_slam_features: null array"; return ORCVIO_ERR_INVALID; }
    for (int f = 0; f < F; ++f) {
        if (ft->anchor[f] < 0 || ft->anchor[f] >= h->N + h->n_nui || ft->state[f] < 0 || ft->state[f] >= h->N) { g_last_error = "upload_slam_features: clone index outside the window"; return ORCVIO_ERR_INVALID; }
        if (ft->slot[f] < 0 || d * (ft->slot[f] + 1) > h->n_extra - 6 * h->n_nui) { g_last_error = "upload_slam_features: feature slot outside the extra states"; return ORCVIO_ERR_INVALID; }
    }
    HIPCHK(hipSetDevice(h->device));
    { const int rc = ekf_reserve(h, F); if (rc != ORCVIO_OK) return rc; }
    h->ekf_F = F; h->ekf_idp = d; h->ekf_eval = true;
    return ORCVIO_OK;
}
static int slam_copies(const orcvio_msckf_handle* h, const orcvio_msckf_slam_features* ft, AuxCopy cp[9]) {
    const size_t cap = (size_t)h->ekf_cap, Fz = (size_t)ft->n_features;
    double* q = h->d_slam;   // [param 3 | inv_depth 1 | p_w 3 | p_fej 3 | z 2][cap]
    const AuxCopy c[9] = {
        {h->d_ekf_i, ft->anchor, sizeof(int) * Fz}, {h->d_ekf_i + cap, ft->state, sizeof(int) * Fz}, {h->d_ekf_i + 2 * cap, ft->slot, sizeof(int) * Fz},
        {q, ft->param, sizeof(double) * 3 * Fz}, {q + 3 * cap, ft->inv_depth, ft->inv_depth ? sizeof(double) * Fz : 0},
        {q + 4 * cap, ft->p_w, sizeof(double) * 3 * Fz}, {q + 7 * cap, ft->p_fej, ft->p_fej ? sizeof(double) * 3 * Fz : 0},
        {q + 10 * cap, ft->z, sizeof(double) * 2 * Fz},
        {h->d_ekf_d + 42 * cap, ft->z_vel, ft->z_vel ? sizeof(double) * 2 * Fz : 0}};   // (the gate's z_vel slot)
    for (int i = 0; i < 9; ++i) cp[i] = c[i];
    return 9;
}
int32_t orcvio_msckf_upload_slam_features(orcvio_msckf_handle* h, const orcvio_msckf_slam_features* ft) {
    const int rc = slam_prepare(h, ft);
    if (rc != ORCVIO_OK || ft->n_features == 0) return rc;
    AuxCopy cp[9];
    const int nc = slam_copies(h, ft, cp);
    return aux_copies(h, h->stream, cp, nc);   // (in order behind the window's upload on the same stream)
}

int32_t orcvio_msckf_upload_ekf_rows(orcvio_msckf_handle* h, const orcvio_msckf_ekf_rows* rows) {
    if (!h || !rows || !(h->uploaded || h->io_open)) { g_last_error = "upload_ekf_rows: upload the window first"; return ORCVIO_ERR_INVALID; }
    if (!h->ekf_mode) { g_last_error = "upload_ekf_rows: set ORCVIO_OPT_EKF_ROWS before the upload"; return ORCVIO_ERR_INVALID; }
    const int F = rows->n_features, d = rows->idp_dim;
    if (F < 0 || (d != 1 && d != 3)) { g_last_error = "upload_ekf_rows: idp_dim must be 1 or 3"; return ORCVIO_ERR_INVALID; }
    if (F > 0 && (!rows->anchor || !rows->state || !rows->slot || !rows->H_e || !rows->H_a || !rows->H_x || !rows->H_f || !rows->r ||
                  (h->flags.estimate_td && !rows->z_vel))) { g_last_error = "upload_ekf_rows: null array"; return ORCVIO_ERR_INVALID; }
    for (int f = 0; f < F; ++f) {
        if (rows->anchor[f] < 0 || rows->anchor[f] >= h->N + h->n_nui || rows->state[f] < 0 || rows->state[f] >= h->N) { g_last_error = "upload_ekf_rows: clone index outside the window"; return ORCVIO_ERR_INVALID; }
        if (rows->slot[f] < 0 || d * (rows->slot[f] + 1) > h->n_extra - 6 * h->n_nui) { g_last_error = "upload_ekf_rows: feature slot outside the extra states"; return ORCVIO_ERR_INVALID; }
    }
    HIPCHK(hipSetDevice(h->device));
    { const int rc = ekf_reserve(h, F); if (rc != ORCVIO_OK) return rc; }
    h->ekf_F = F; h->ekf_idp = d; h->ekf_eval = false;
    if (F == 0) return ORCVIO_OK;
    const size_t cap = (size_t)h->ekf_cap, Fz = (size_t)F;
    double* q = h->d_ekf_d;   // [H_e 12 | H_a 12 | H_x 12 | H_f 6 | z_vel 2 | r 2][cap]
    const AuxCopy cp[] = {
        {h->d_ekf_i, rows->anchor, sizeof(int) * Fz}, {h->d_ekf_i + cap, rows->state, sizeof(int) * Fz}, {h->d_ekf_i + 2 * cap, rows->slot, sizeof(int) * Fz},
        {q, rows->H_e, sizeof(double) * 12 * Fz}, {q + 12 * cap, rows->H_a, sizeof(double) * 12 * Fz}, {q + 24 * cap, rows->H_x, sizeof(double) * 12 * Fz},
        {q + 36 * cap, rows->H_f, sizeof(double) * 2 * (size_t)d * Fz}, {q + 42 * cap, rows->z_vel, rows->z_vel ? sizeof(double) * 2 * Fz : 0},
        {q + 44 * cap, rows->r, sizeof(double) * 2 * Fz}};
    return aux_copies(h, h->stream, cp, (int)(sizeof(cp) / sizeof(cp[0])));
}

static int dense_reserve(orcvio_msckf_handle* h, int rows);
int32_t orcvio_msckf_upload_dense_rows(orcvio_msckf_handle* h, int32_t n_rows, const double* H, const double* r) {
    if (!h || !h->uploaded || n_rows < 0 || (n_rows > 0 && (!H || !r))) { g_last_error = "upload_dense_rows: upload the window first"; return ORCVIO_ERR_INVALID; }
    if (h->n_extra > 0 && !h->ekf_mode) { g_last_error = "upload_dense_rows: with extra states set ORCVIO_OPT_EKF_ROWS before the upload"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    h->dense_rows = 0;   // (these rows come first; orcvio_msckf_upload_new_features appends)
    { const int rc = dense_reserve(h, n_rows); if (rc != ORCVIO_OK) return rc; }
    if (!h->d_Gekf) HIPCHK(hipMalloc(&h->d_Gekf, sizeof(double) * (size_t)2 * h->NAP_max * h->NAP_max));
    h->dense_rows = n_rows;
    if (n_rows == 0) return ORCVIO_OK;
    const int n = h->n, NA = h->NA, NAP = h->NAP;
    for (int i = 0; i < n_rows; ++i)
        for (int c = 0; c < 15; ++c)
            if (H[(size_t)i * n + c] != 0.0) { g_last_error = "upload_dense_rows: the first 15 columns (IMU state) must be zero"; return ORCVIO_ERR_INVALID; }
    std::vector<double> st((size_t)n_rows * NAP, 0.0);   // [H(:, 15:15+NA) | r | 0]
    for (int i = 0; i < n_rows; ++i) {
        std::memcpy(&st[(size_t)i * NAP], H + (size_t)i * n + 15, sizeof(double) * NA);
        st[(size_t)i * NAP + NA] = r[i];
    }
    const AuxCopy cp[] = {{h->d_dense, st.data(), sizeof(double) * st.size()}};
    return aux_copies(h, h->stream, cp, 1);
}

// Schmidt-EKF: the poses of the nuisance states (state_server.nui_imu_states: clones that left the window but stay in state_cov as
// nuisance parameters, src/orcvio.cpp:2881-2920), in the pose slots behind the window's: SLAM features may be anchored there
// (anchor index N + j, :1247-1256, :1591-1606).  After orcvio_msckf_upload, with ORCVIO_OPT_SCHMIDT_STATES = nui->n_clones.
int32_t orcvio_msckf_upload_nuisance_poses(orcvio_msckf_handle* h, const orcvio_msckf_window* nui) {
    if (!h || !nui || !h->uploaded) { g_last_error = "upload_nuisance_poses: upload the window first"; return ORCVIO_ERR_INVALID; }
    if (nui->n_clones != h->n_nui) { g_last_error = "upload_nuisance_poses: count differs from ORCVIO_OPT_SCHMIDT_STATES"; return ORCVIO_ERR_INVALID; }
    if (h->n_nui == 0) return ORCVIO_OK;
    if (!nui->R_b2w || !nui->t_b_w || !nui->R_b2c || !nui->t_c_b) { g_last_error = "upload_nuisance_poses: null array"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    std::vector<double> rec((size_t)POSE_STRIDE * h->n_nui, 0.0);
    const double* tfej = nui->t_fej ? nui->t_fej : nui->t_b_w;
    for (int i = 0; i < h->n_nui; ++i) {
        double* r = rec.data() + (size_t)POSE_STRIDE * i;
        std::memcpy(r + POSE_R_B2W, nui->R_b2w + 9 * i, 72); std::memcpy(r + POSE_T_B_W, nui->t_b_w + 3 * i, 24);
        std::memcpy(r + POSE_T_FEJ, tfej + 3 * i, 24);
        std::memcpy(r + POSE_R_B2C, nui->R_b2c + 9 * i, 72); std::memcpy(r + POSE_T_C_B, nui->t_c_b + 3 * i, 24);
    }
    const AuxCopy cp[] = {{h->d_poses + (size_t)POSE_STRIDE * h->N, rec.data(), sizeof(double) * rec.size()}};
    return aux_copies(h, h->stream, cp, 1);   // (on the stream: behind the copy of the input arena)
}

// Dense-row scratch [cap][NAP_max] (caller-projected rows, V parts of entering features); the contents are kept.
static int dense_reserve(orcvio_msckf_handle* h, int rows) {
    if (rows <= h->dense_cap) return ORCVIO_OK;
    HIPCHK(hipDeviceSynchronize());
    const int cap = round_up(rows, 64);
    double* nb = nullptr;
    HIPCHK(hipMalloc(&nb, sizeof(double) * (size_t)cap * h->NAP_max));
    if (h->d_dense) {
        if (h->dense_rows > 0) HIPCHK(hipMemcpy(nb, h->d_dense, sizeof(double) * (size_t)h->dense_rows * h->NAP, hipMemcpyDeviceToDevice));
        (void)hipFree(h->d_dense);
    }
    h->d_dense = nb; h->dense_cap = cap;
    h->graph_epoch++;   // captured graphs hold the freed pointer
    return ORCVIO_OK;
}

// Features ENTERING the state, on the device: featureJacobian_ekf_new (src/orcvio.cpp:1481-1572) for every listed feature and
// the rotation of its rows by W = [V | U] (:2416-2436), k_ekf_new.  The V parts (zero in the new columns) are appended to the
// dense rows of this upload and take part in the update; the U parts H_1, H_2, r_1 stay on the device for
// orcvio_msckf_download_new_feature_blocks (-> orcvio_msckf_augment_state after the update).
int32_t orcvio_msckf_upload_new_features(orcvio_msckf_handle* h, const orcvio_msckf_new_features* nf) {
    if (!h || !nf || !h->uploaded) { g_last_error = "upload_new_features: upload the window first"; return ORCVIO_ERR_INVALID; }
    if (h->n_extra > 0 && !h->ekf_mode) { g_last_error = "upload_new_features: with extra states set ORCVIO_OPT_EKF_ROWS before the upload"; return ORCVIO_ERR_INVALID; }
    const int k = nf->n_features, d = nf->idp_dim, N = h->N;
    if (k < 0 || (d != 1 && d != 3)) { g_last_error = "upload_new_features: idp_dim must be 1 or 3"; return ORCVIO_ERR_INVALID; }
    if (h->new_F > 0) { g_last_error = "upload_new_features: already called for this upload (list all entering features in one call)"; return ORCVIO_ERR_INVALID; }
    if (k == 0) return ORCVIO_OK;
    if (!nf->anchor || !nf->param || !nf->p_w || !nf->obs_ptr || !nf->obs_clone || !nf->obs_z || (d == 1 && !nf->inv_depth) ||
        (h->flags.if_fej && !nf->p_fej) || (h->flags.estimate_td && !nf->obs_zvel)) { g_last_error = "upload_new_features: null array"; return ORCVIO_ERR_INVALID; }
    if (nf->obs_ptr[0] < 0) { g_last_error = "upload_new_features: obs_ptr starts below zero"; return ORCVIO_ERR_INVALID; }
    const int nobs = nf->obs_ptr[k];
    std::vector<int> row0(k + 1, 0);
    for (int j = 0; j < k; ++j) {
        const int a = nf->anchor[j];
        if (a < 0 || a >= N + h->n_nui) { g_last_error = "upload_new_features: anchor outside the window"; return ORCVIO_ERR_INVALID; }
        const int M = nf->obs_ptr[j + 1] - nf->obs_ptr[j];
        if (M < 0 || M > ORCVIO_MAX_TRACK) { g_last_error = "upload_new_features: track longer than ORCVIO_MAX_TRACK"; return ORCVIO_ERR_TRACK_TOO_LONG; }
        int kept = 0;
        for (int o = nf->obs_ptr[j]; o < nf->obs_ptr[j + 1]; ++o) {
            if (nf->obs_clone[o] < 0 || nf->obs_clone[o] >= N) { g_last_error = "upload_new_features: obs_clone outside the window"; return ORCVIO_ERR_INVALID; }
            if (!(d == 1 && nf->obs_clone[o] == a)) ++kept;   // :1494-1496
        }
        if (2 * kept <= d) { g_last_error = "upload_new_features: a feature with too few observations"; return ORCVIO_ERR_INVALID; }
        row0[j + 1] = row0[j] + 2 * kept;
    }
    HIPCHK(hipSetDevice(h->device));
    const int base = h->dense_rows, rows = row0[k];
    { const int rc = dense_reserve(h, base + rows); if (rc != ORCVIO_OK) return rc; }
    if (!h->d_Gekf) HIPCHK(hipMalloc(&h->d_Gekf, sizeof(double) * (size_t)2 * h->NAP_max * h->NAP_max));
    for (int j = 0; j <= k; ++j) row0[j] += base;
    // one staging block: doubles [param 3k | inv_depth k | p_w 3k | p_fej 3k | obs_z 2 nobs | obs_zvel 2 nobs], ints [anchor k |
    // obs_ptr k+1 | obs_clone nobs | row0 k+1]; outputs behind it on the device [H_1 d k n | H_2 k d d | r_1 d k]
    const size_t nd_in = (size_t)10 * k + (size_t)4 * nobs, ni = (size_t)3 * k + 2 + nobs, n_out = (size_t)d * k * h->n + (size_t)k * d * d + (size_t)d * k;
    const size_t bytes_in = nd_in * 8 + ((ni * 4 + 7) & ~(size_t)7);
    if (bytes_in + n_out * 8 > h->new_cap) {
        HIPCHK(hipDeviceSynchronize());
        if (h->d_new) (void)hipFree(h->d_new);
        h->new_cap = (bytes_in + n_out * 8) * 2;
        HIPCHK(hipMalloc(&h->d_new, h->new_cap));
    }
    std::vector<char> st(bytes_in, 0);
    double* sd = reinterpret_cast<double*>(st.data());
    int* si = reinterpret_cast<int*>(st.data() + nd_in * 8);
    std::memcpy(sd, nf->param, sizeof(double) * 3 * k);
    if (nf->inv_depth) std::memcpy(sd + 3 * k, nf->inv_depth, sizeof(double) * k);
    std::memcpy(sd + 4 * k, nf->p_w, sizeof(double) * 3 * k);
    if (nf->p_fej) std::memcpy(sd + 7 * k, nf->p_fej, sizeof(double) * 3 * k);
    std::memcpy(sd + 10 * k, nf->obs_z, sizeof(double) * 2 * nobs);
    if (nf->obs_zvel) std::memcpy(sd + 10 * k + 2 * nobs, nf->obs_zvel, sizeof(double) * 2 * nobs);
    std::memcpy(si, nf->anchor, sizeof(int) * k);
    std::memcpy(si + k, nf->obs_ptr, sizeof(int) * (k + 1));
    std::memcpy(si + 2 * k + 1, nf->obs_clone, sizeof(int) * nobs);
    std::memcpy(si + 2 * k + 1 + nobs, row0.data(), sizeof(int) * (k + 1));
    hipStream_t s = h->stream;
    {
        const AuxCopy cp[] = {{h->d_new, st.data(), bytes_in}};
        const int rc = aux_copies(h, s, cp, 1);
        if (rc != ORCVIO_OK) return rc;
    }
    const double* dd = reinterpret_cast<const double*>(h->d_new);
    const int* di = reinterpret_cast<const int*>(h->d_new + nd_in * 8);
    double* dout = reinterpret_cast<double*>(h->d_new + bytes_in);
    EkfNewArgs a;
    a.n_new = k; a.idp_dim = d; a.if_fej = h->flags.if_fej; a.estimate_td = h->flags.estimate_td; a.leg = h->flags.leg_dim;
    a.NA = h->NA; a.NAP = h->NAP; a.n = h->n; a.N = h->N; a.n_nui = h->n_nui;
    a.poses = h->d_poses;
    a.param = dd; a.inv_depth = dd + 3 * k; a.p_w = dd + 4 * k; a.p_fej = nf->p_fej ? dd + 7 * k : nullptr;
    a.obs_z = dd + 10 * k; a.obs_zvel = dd + 10 * k + 2 * nobs;
    a.anchor = di; a.obs_ptr = di + k; a.obs_clone = di + 2 * k + 1; a.row0 = di + 2 * k + 1 + nobs;
    a.dense = h->d_dense;
    a.H1 = dout; a.H2 = dout + (size_t)d * k * h->n; a.r1 = a.H2 + (size_t)k * d * d;
    hipLaunchKernelGGL(k_ekf_new, dim3(k), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    h->dense_rows = base + rows;
    h->new_F = k; h->new_idp = d; h->new_out_off = bytes_in;
    return ORCVIO_OK;
}

// H_1 [d k][n], H_2 [k][d][d] (upper triangular blocks), r_1 [d k] of the features of the last orcvio_msckf_upload_new_features
int32_t orcvio_msckf_download_new_feature_blocks(orcvio_msckf_handle* h, double* H_1, double* H_2, double* r_1) {
    if (!h || h->new_F <= 0 || !H_1 || !H_2 || !r_1) { g_last_error = "download_new_feature_blocks: no entering features uploaded"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    const int k = h->new_F, d = h->new_idp, n = h->n;
    const double* dout = reinterpret_cast<const double*>(h->d_new + h->new_out_off);
    const FetchCopy fc[] = {{H_1, dout, sizeof(double) * (size_t)d * k * n}, {H_2, dout + (size_t)d * k * n, sizeof(double) * (size_t)k * d * d},
                            {r_1, dout + (size_t)d * k * n + (size_t)k * d * d, sizeof(double) * (size_t)d * k}};
    return fetch_copies(h, h->stream, fc, 3);
}

// New SLAM features, 3-parameter form, listed among the tracks of the last update: their correction and the augmented
// covariance (measurementUpdate_hybrid, src/orcvio.cpp:1811-1821 and :1904-1947, without nuisance states).  Host
// arithmetic on a few 3 x n blocks.  For a track, k_feature left T3 = Q1^T [J_msckf | r] and R = Q1^T H_f(xyz); the rows
// of featureJacobian_ekf_new differ from the MSCKF rows by H_f(xyz) X, X = d p_w / d(state) at fixed inverse-depth
// parameters (anchor pose, extrinsics), and H_f(idp) = H_f(xyz) J_pf, J_pf = R_ca2w J_f, so that
//   H_1 = T3_J + R X,   H_2 = R J_pf,   r_1 = T3_r        (:2433-2436 with U = Q1).
int32_t orcvio_msckf_augment_new_features(orcvio_msckf_handle* h, const orcvio_msckf_window* win, int32_t n_new,
                                          const int32_t* track, const int32_t* anchor, const double* inv_param,
                                          const double* dx, const double* P_upd, double* dx_new, double* P_aug) {
    if (!h || !win || !h->ran || n_new < 0 || (n_new > 0 && (!track || !anchor || !inv_param)) || !dx || !P_upd || !dx_new || !P_aug) {
        g_last_error = "augment_new_features: null argument or no finished update"; return ORCVIO_ERR_INVALID;
    }
    if (h->flags.if_fej || !h->flags.use_larvio) {
        // the equivalence "V part = MSCKF block" needs the MSCKF rows in the SLAM rows' own error-state convention
        g_last_error = "augment_new_features: needs use_larvio = 1 and if_FEJ = 0 (use orcvio_msckf_new_feature_rows / _augment_state otherwise)";
        return ORCVIO_ERR_INVALID;
    }
    const int n = h->n, NA = h->NA, NAP = h->NAP, leg = h->flags.leg_dim, N = h->N, k3 = 3 * n_new, nt = n + k3;
    for (int j = 0; j < n_new; ++j)
        if (track[j] < 0 || track[j] >= h->F || anchor[j] < 0 || anchor[j] >= N) { g_last_error = "augment_new_features: index out of range"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->last_stream ? h->last_stream : h->stream));
    std::vector<double> T3((size_t)3 * NAP), Rf(6), H1((size_t)k3 * n, 0.0), H2i((size_t)n_new * 9), HtH_i((size_t)n_new * 9), r1s(k3);
    const double s2 = h->flags.noise_feature * h->flags.noise_feature;
    auto inv3 = [](const double* A, double* B) {   // B = A^-1 (3 x 3)
        const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
        const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
        B[0] = c00 / det; B[1] = (A[2] * A[7] - A[1] * A[8]) / det; B[2] = (A[1] * A[5] - A[2] * A[4]) / det;
        B[3] = c01 / det; B[4] = (A[0] * A[8] - A[2] * A[6]) / det; B[5] = (A[2] * A[3] - A[0] * A[5]) / det;
        B[6] = c02 / det; B[7] = (A[1] * A[6] - A[0] * A[7]) / det; B[8] = (A[0] * A[4] - A[1] * A[3]) / det;
    };
    for (int j = 0; j < n_new; ++j) {
        HIPCHK(hipMemcpy(T3.data(), h->d_T3 + (size_t)3 * track[j] * NAP, sizeof(double) * 3 * NAP, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(Rf.data(), h->d_Rf + (size_t)6 * track[j], sizeof(double) * 6, hipMemcpyDeviceToHost));
        const double R[9] = {Rf[0], Rf[1], Rf[2], 0.0, Rf[3], Rf[4], 0.0, 0.0, Rf[5]};
        const int a = anchor[j];
        const double* Ra = win->R_b2w + 9 * a;      // R_ba2w
        const double* Rbc = win->R_b2c + 9 * a;
        const double* tcb = win->t_c_b + 3 * a;
        const double* f = inv_param + 3 * j;
        const double p_ca[3] = {f[0] / f[2], f[1] / f[2], 1.0 / f[2]};
        double q[3], pb[3], pw_rel[3];            // q = R_b2c^T p_ca ; pb = q + t_c_b ; pw_rel = R_ba2w pb = p_w - t_ba
        for (int i = 0; i < 3; ++i) q[i] = Rbc[i] * p_ca[0] + Rbc[3 + i] * p_ca[1] + Rbc[6 + i] * p_ca[2];
        for (int i = 0; i < 3; ++i) pb[i] = q[i] + tcb[i];
        for (int i = 0; i < 3; ++i) pw_rel[i] = Ra[3 * i] * pb[0] + Ra[3 * i + 1] * pb[1] + Ra[3 * i + 2] * pb[2];
        // X (3 x n): anchor clone [-skew(p_w - t_ba), I]; extrinsics [-R_ba2w skew(q), R_ba2w]
        std::vector<double> X((size_t)3 * n, 0.0);
        const double S[9] = {0, -pw_rel[2], pw_rel[1], pw_rel[2], 0, -pw_rel[0], -pw_rel[1], pw_rel[0], 0};
        const double Sq[9] = {0, -q[2], q[1], q[2], 0, -q[0], -q[1], q[0], 0};
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) {
                X[(size_t)i * n + leg + 6 * a + c] = -S[3 * i + c];
                X[(size_t)i * n + leg + 6 * a + 3 + c] = (i == c) ? 1.0 : 0.0;
                double m = 0.0;
                for (int k = 0; k < 3; ++k) m += Ra[3 * i + k] * Sq[3 * k + c];
                X[(size_t)i * n + 15 + c] = -m;
                X[(size_t)i * n + 18 + c] = Ra[3 * i + c];
            }
        // H_1 = T3_J (active columns 15 .. 15+NA) + R X
        for (int i = 0; i < 3; ++i) {
            double* row = &H1[(size_t)(3 * j + i) * n];
            for (int c = 0; c < NA; ++c) row[15 + c] = T3[(size_t)i * NAP + c];
            for (int c = 0; c < n; ++c) {
                double m = 0.0;
                for (int k = i; k < 3; ++k) m += R[3 * i + k] * X[(size_t)k * n + c];
                row[c] += m;
            }
            r1s[3 * j + i] = T3[(size_t)i * NAP + NA];
        }
        // H_2 = R R_ca2w J_f,  R_ca2w = R_ba2w R_b2c^T,  J_f = d p_ca / d(alpha, beta, rho)
        double Rca[9], Jf[9] = {1.0 / f[2], 0.0, -f[0] / (f[2] * f[2]), 0.0, 1.0 / f[2], -f[1] / (f[2] * f[2]), 0.0, 0.0, -1.0 / (f[2] * f[2])};
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) Rca[3 * i + c] = Ra[3 * i] * Rbc[3 * c] + Ra[3 * i + 1] * Rbc[3 * c + 1] + Ra[3 * i + 2] * Rbc[3 * c + 2];
        double M1[9], H2[9];
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) M1[3 * i + c] = Rca[3 * i] * Jf[c] + Rca[3 * i + 1] * Jf[3 + c] + Rca[3 * i + 2] * Jf[6 + c];
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) H2[3 * i + c] = R[3 * i] * M1[c] + R[3 * i + 1] * M1[3 + c] + R[3 * i + 2] * M1[6 + c];
        if (h->ref_h2_ldlt) {
            // The reference's literal tail: its U is the Q factor of H_f in the INVERSE-DEPTH parametrisation (SPQR, :2421-2428), so
            // its H_2 is that matrix's upper-triangular R, and H_2.ldlt() (:1826-1827) reads the lower triangle of it -- the diagonal.
            // Here U = Q_1 of H_f(xyz) (same column space): H_2 = Q_3 R_idp by a 3 x 3 Gram-Schmidt QR, the three rows of H_1 and r_1
            // are rotated by Q_3^T into the reference's basis (up to the signs of the rows, which the diagonal division cancels).
            double Q3[9], Rr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int c = 0; c < 3; ++c) {
                double v[3] = {H2[c], H2[3 + c], H2[6 + c]};
                for (int q = 0; q < c; ++q) {
                    const double dq = Q3[q] * v[0] + Q3[3 + q] * v[1] + Q3[6 + q] * v[2];
                    Rr[3 * q + c] = dq;
                    for (int i = 0; i < 3; ++i) v[i] -= dq * Q3[3 * i + q];
                }
                const double nv = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                Rr[3 * c + c] = nv;
                for (int i = 0; i < 3; ++i) Q3[3 * i + c] = v[i] / nv;
            }
            double rot[3];
            for (int c = 0; c < n; ++c) {
                for (int i = 0; i < 3; ++i) rot[i] = Q3[i] * H1[(size_t)(3 * j) * n + c] + Q3[3 + i] * H1[(size_t)(3 * j + 1) * n + c] + Q3[6 + i] * H1[(size_t)(3 * j + 2) * n + c];
                for (int i = 0; i < 3; ++i) H1[(size_t)(3 * j + i) * n + c] = rot[i];
            }
            for (int i = 0; i < 3; ++i) rot[i] = Q3[i] * r1s[3 * j] + Q3[3 + i] * r1s[3 * j + 1] + Q3[6 + i] * r1s[3 * j + 2];
            for (int i = 0; i < 3; ++i) r1s[3 * j + i] = rot[i];
            std::memcpy(H2, Rr, sizeof(Rr));
            for (int i = 0; i < 9; ++i) H2i[9 * j + i] = 0.0;
            for (int i = 0; i < 3; ++i) H2i[9 * j + 4 * i] = 1.0 / H2[4 * i];
        } else inv3(H2, &H2i[9 * j]);
        double HtH[9];
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) HtH[3 * i + c] = H2[i] * H2[c] + H2[3 + i] * H2[3 + c] + H2[6 + i] * H2[6 + c];
        inv3(HtH, &HtH_i[9 * j]);
    }
    // HH = H_2^-1 H_1 (block rows), dx_new = -HH dx + H_2^-1 r_1, nHHP = -HH P, P22 = HH P HH^T + s2 (H_2^T H_2)^-1
    std::vector<double> HH((size_t)k3 * n, 0.0), nHHP((size_t)k3 * n, 0.0);
    for (int j = 0; j < n_new; ++j)
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < n; ++c) {
                double m = 0.0;
                for (int k = 0; k < 3; ++k) m += H2i[9 * j + 3 * i + k] * H1[(size_t)(3 * j + k) * n + c];
                HH[(size_t)(3 * j + i) * n + c] = m;
            }
    for (int j = 0; j < n_new; ++j)
        for (int i = 0; i < 3; ++i) {
            double m = 0.0;
            for (int k = 0; k < 3; ++k) m += H2i[9 * j + 3 * i + k] * r1s[3 * j + k];
            for (int c = 0; c < n; ++c) m -= HH[(size_t)(3 * j + i) * n + c] * dx[c];
            dx_new[3 * j + i] = m;
        }
    for (int r = 0; r < k3; ++r)
        for (int k = 0; k < n; ++k) {
            const double hv = HH[(size_t)r * n + k];
            if (hv == 0.0) continue;
            const double* prow = P_upd + (size_t)k * n;
            double* o = &nHHP[(size_t)r * n];
            for (int c = 0; c < n; ++c) o[c] -= hv * prow[c];
        }
    for (int r = 0; r < n; ++r) std::memcpy(P_aug + (size_t)r * nt, P_upd + (size_t)r * n, sizeof(double) * n);
    for (int r = 0; r < k3; ++r)
        for (int c = 0; c < n; ++c) { P_aug[(size_t)(n + r) * nt + c] = nHHP[(size_t)r * n + c]; P_aug[(size_t)c * nt + n + r] = nHHP[(size_t)r * n + c]; }
    for (int r = 0; r < k3; ++r)
        for (int c = 0; c < k3; ++c) {
            double m = 0.0;
            for (int k = 0; k < n; ++k) m -= nHHP[(size_t)r * n + k] * HH[(size_t)c * n + k];
            if (r / 3 == c / 3) m += s2 * HtH_i[9 * (r / 3) + 3 * (r % 3) + (c % 3)];
            P_aug[(size_t)(n + r) * nt + n + c] = m;
        }
    for (int r = 0; r < nt; ++r)   // (:1946) symmetrise
        for (int c = r + 1; c < nt; ++c) { const double m = 0.5 * (P_aug[(size_t)r * nt + c] + P_aug[(size_t)c * nt + r]); P_aug[(size_t)r * nt + c] = m; P_aug[(size_t)c * nt + r] = m; }
    return ORCVIO_OK;
}

// ---- host arithmetic for features entering the state, either parametrisation (no device, no handle) -----------------
// Rows of featureJacobian_ekf_new (src/orcvio.cpp:1481-1572) for every listed feature and their rotation by W = [V | U]
// (:2416-2436): H_f of different features share no column, so the split is one small Householder QR per feature
// (U = the first d columns of Q, V the rest; only the two subspaces matter, DESIGN.md section 7).
//   out: H_top [*rows_top][n_cols], r_top  -- the V parts, zero in the new columns: to orcvio_msckf_upload_dense_rows
//        H_1 [d n_new][n_cols], H_2 [n_new][d][d] (upper triangular blocks), r_1 [d n_new]  -- the U parts
int32_t orcvio_msckf_new_feature_rows(const orcvio_msckf_flags* flags, const orcvio_msckf_window* win, int32_t idp_dim, int32_t n_cols,
                                      int32_t n_new, const int32_t* anchor, const double* param, const double* inv_depth,
                                      const double* p_w, const double* p_fej, const int32_t* obs_ptr, const int32_t* obs_clone,
                                      const double* obs_z, const double* obs_zvel, int32_t* rows_top, double* H_top, double* r_top,
                                      double* H_1, double* H_2, double* r_1) {
    if (!flags || !win || n_new < 0 || (idp_dim != 1 && idp_dim != 3) || !rows_top || (n_new > 0 && (!anchor || !param || !p_w || !obs_ptr ||
        !obs_clone || !obs_z || !H_top || !r_top || !H_1 || !H_2 || !r_1 || (idp_dim == 1 && !inv_depth) || (flags->if_fej && !p_fej) ||
        (flags->estimate_td && !obs_zvel)))) { g_last_error = "new_feature_rows: null argument"; return ORCVIO_ERR_INVALID; }
    const int d = idp_dim, N = win->n_clones, leg = flags->leg_dim;
    if (n_cols < leg + 6 * N) { g_last_error = "new_feature_rows: n_cols smaller than the window"; return ORCVIO_ERR_INVALID; }
    auto pose = [&](int i, double* rec) {
        std::memcpy(rec + POSE_R_B2W, win->R_b2w + 9 * i, 72); std::memcpy(rec + POSE_T_B_W, win->t_b_w + 3 * i, 24);
        std::memcpy(rec + POSE_T_FEJ, (win->t_fej ? win->t_fej : win->t_b_w) + 3 * i, 24);
        std::memcpy(rec + POSE_R_B2C, win->R_b2c + 9 * i, 72); std::memcpy(rec + POSE_T_C_B, win->t_c_b + 3 * i, 24);
    };
    int top = 0;
    for (int j = 0; j < n_new; ++j) {
        const int a = anchor[j];
        if (a < 0 || a >= N) { g_last_error = "new_feature_rows: anchor outside the window"; return ORCVIO_ERR_INVALID; }
        std::vector<int> obs;
        for (int o = obs_ptr[j]; o < obs_ptr[j + 1]; ++o) {
            if (obs_clone[o] < 0 || obs_clone[o] >= N) { g_last_error = "new_feature_rows: obs_clone outside the window"; return ORCVIO_ERR_INVALID; }
            if (d == 1 && obs_clone[o] == a) continue;   // :1494-1496
            obs.push_back(o);
        }
        const int m = 2 * (int)obs.size();
        if (m <= d) { g_last_error = "new_feature_rows: a feature with too few observations"; return ORCVIO_ERR_INVALID; }
        std::vector<double> Hx((size_t)m * n_cols, 0.0), Hf((size_t)m * d, 0.0), r(m, 0.0);
        double Pa[POSE_STRIDE], Pk[POSE_STRIDE];
        pose(a, Pa);
        for (size_t c = 0; c < obs.size(); ++c) {
            const int o = obs[c], k = obs_clone[o];
            pose(k, Pk);
            double He[12], Ha[12], Hxk[12], Hfk[6], rr[2];
            ekf_row_blocks(Pk, Pa, k == a, d, flags->if_fej, param + 3 * j, d == 1 ? inv_depth[j] : 0.0, p_w + 3 * j,
                           p_fej ? p_fej + 3 * j : nullptr, obs_z + 2 * o, He, Ha, Hxk, Hfk, rr);
            for (int b = 0; b < 2; ++b) {
                double* row = &Hx[(size_t)(2 * c + b) * n_cols];
                for (int e = 0; e < 6; ++e) row[leg + 6 * a + e] = Ha[6 * b + e];            // :1561
                for (int e = 0; e < 6; ++e) row[leg + 6 * k + e] = Hxk[6 * b + e];           // :1562 (overwrites if k == a)
                for (int e = 0; e < 6; ++e) row[15 + e] = He[6 * b + e];                     // :1563
                if (flags->estimate_td) row[21] = obs_zvel[2 * o + b];                       // :1564-1565
                for (int e = 0; e < d; ++e) Hf[(size_t)(2 * c + b) * d + e] = Hfk[b * d + e];
                r[2 * c + b] = rr[b];
            }
        }
        // Householder QR of H_f (m x d), applied to [H_x | r]
        for (int q = 0; q < d; ++q) {
            double nrm2 = 0.0;
            for (int i = q + 1; i < m; ++i) nrm2 += Hf[(size_t)i * d + q] * Hf[(size_t)i * d + q];
            const double alpha = Hf[(size_t)q * d + q];
            if (nrm2 == 0.0) continue;
            const double nu = std::sqrt(alpha * alpha + nrm2), bk = alpha >= 0.0 ? -nu : nu;
            const double beta = (bk - alpha) / bk, sc = 1.0 / (alpha - bk);
            std::vector<double> v(m, 0.0);
            v[q] = 1.0;
            for (int i = q + 1; i < m; ++i) v[i] = Hf[(size_t)i * d + q] * sc;
            auto apply = [&](double* M, int ld, int c0, int c1) {
                for (int c = c0; c < c1; ++c) {
                    double w = 0.0;
                    for (int i = q; i < m; ++i) w += v[i] * M[(size_t)i * ld + c];
                    w *= beta;
                    for (int i = q; i < m; ++i) M[(size_t)i * ld + c] -= w * v[i];
                }
            };
            apply(Hf.data(), d, q, d);
            apply(Hx.data(), n_cols, 0, n_cols);
            apply(r.data(), 1, 0, 1);
        }
        for (int i = 0; i < d; ++i) {   // U part
            std::memcpy(H_1 + (size_t)(d * j + i) * n_cols, &Hx[(size_t)i * n_cols], sizeof(double) * n_cols);
            for (int e = 0; e < d; ++e) H_2[(size_t)j * d * d + i * d + e] = e >= i ? Hf[(size_t)i * d + e] : 0.0;
            r_1[d * j + i] = r[i];
        }
        for (int i = d; i < m; ++i) {   // V part
            std::memcpy(H_top + (size_t)top * n_cols, &Hx[(size_t)i * n_cols], sizeof(double) * n_cols);
            r_top[top++] = r[i];
        }
    }
    *rows_top = top;
    return ORCVIO_OK;
}

// measurementUpdate_hybrid, the part behind the update of the legacy state (src/orcvio.cpp:1818-1821, :1904-1947, no
// nuisance states): dx_new = H_2^-1 (r_1 - H_1 dx), P_aug = [[P, (-HH P)^T], [-HH P, HH P HH^T + s2 (H_2^T H_2)^-1]],
// HH = H_2^-1 H_1, with H_2 block diagonal (one upper-triangular d x d block per feature).
// (The reference writes H_2.ldlt().solve(.), which for d = 3 reads only the lower triangle of an upper-triangular H_2;
// the triangular system is solved here.  For the 1-parameter form of the shipped configurations H_2 is diagonal and the
// two coincide.)
// diag_only: the reference's literal arithmetic for HH and dx_new -- `H_2.ldlt().solve(..)` (src/orcvio.cpp:1826-1827) on an
// UPPER-triangular H_2: Eigen's LDLT reads the lower triangle only, i.e. diag(H_2) (the same thing for the 1 x 1 blocks of
// feature_idp_dim = 1, every shipped configuration).  P22 uses (H_2^T H_2)^-1 in both modes, as the reference does (:1907-1908).
static int augment_state_impl(int32_t n, int32_t n_new, int32_t idp_dim, const double* H_1, const double* H_2, const double* r_1,
                              double sigma2, const double* dx, const double* P_upd, bool diag_only, double* dx_new, double* P_aug) {
    if (n < 1 || n_new < 0 || (idp_dim != 1 && idp_dim != 3) || !dx || !P_upd || !dx_new || !P_aug || (n_new > 0 && (!H_1 || !H_2 || !r_1))) {
        g_last_error = "augment_state: invalid argument"; return ORCVIO_ERR_INVALID;
    }
    const int d = idp_dim, sz = d * n_new, nt = n + sz;
    std::vector<double> HH((size_t)sz * n, 0.0), nHHP((size_t)sz * n, 0.0), W((size_t)n_new * d * d, 0.0);
    for (int j = 0; j < n_new; ++j) {
        const double* R = H_2 + (size_t)j * d * d;
        for (int i = 0; i < d; ++i)
            if (R[i * d + i] == 0.0) { g_last_error = "augment_state: singular H_2"; return ORCVIO_ERR_NOT_SPD; }
        // back substitution on the block: HH_j = R^-1 H_1_j, x_j = R^-1 r_1_j
        for (int c = 0; c <= n; ++c)
            for (int i = d - 1; i >= 0; --i) {
                double m = c < n ? H_1[(size_t)(d * j + i) * n + c] : r_1[d * j + i];
                if (!diag_only)
                    for (int k = i + 1; k < d; ++k) m -= R[i * d + k] * (c < n ? HH[(size_t)(d * j + k) * n + c] : dx_new[d * j + k]);
                m /= R[i * d + i];
                if (c < n) HH[(size_t)(d * j + i) * n + c] = m; else dx_new[d * j + i] = m;
            }
        // (R^T R)^-1 = R^-1 R^-T
        double Ri[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int c = 0; c < d; ++c)
            for (int i = d - 1; i >= 0; --i) {
                double m = i == c ? 1.0 : 0.0;
                for (int k = i + 1; k < d; ++k) m -= R[i * d + k] * Ri[k * d + c];
                Ri[i * d + c] = m / R[i * d + i];
            }
        for (int i = 0; i < d; ++i)
            for (int c = 0; c < d; ++c) {
                double m = 0.0;
                for (int k = 0; k < d; ++k) m += Ri[i * d + k] * Ri[c * d + k];
                W[(size_t)j * d * d + i * d + c] = m;
            }
    }
    for (int r = 0; r < sz; ++r) {
        double m = 0.0;
        for (int c = 0; c < n; ++c) m += HH[(size_t)r * n + c] * dx[c];
        dx_new[r] -= m;
    }
    for (int r = 0; r < sz; ++r)
        for (int k = 0; k < n; ++k) {
            const double hv = HH[(size_t)r * n + k];
            if (hv == 0.0) continue;
            const double* prow = P_upd + (size_t)k * n;
            double* o = &nHHP[(size_t)r * n];
            for (int c = 0; c < n; ++c) o[c] -= hv * prow[c];
        }
    for (int r = 0; r < n; ++r) std::memcpy(P_aug + (size_t)r * nt, P_upd + (size_t)r * n, sizeof(double) * n);
    for (int r = 0; r < sz; ++r)
        for (int c = 0; c < n; ++c) { P_aug[(size_t)(n + r) * nt + c] = nHHP[(size_t)r * n + c]; P_aug[(size_t)c * nt + n + r] = nHHP[(size_t)r * n + c]; }
    for (int r = 0; r < sz; ++r)
        for (int c = 0; c < sz; ++c) {
            double m = 0.0;
            for (int k = 0; k < n; ++k) m -= nHHP[(size_t)r * n + k] * HH[(size_t)c * n + k];
            if (r / d == c / d) m += sigma2 * W[(size_t)(r / d) * d * d + (r % d) * d + (c % d)];
            P_aug[(size_t)(n + r) * nt + n + c] = m;
        }
    for (int r = 0; r < nt; ++r)   // (:1946)
        for (int c = r + 1; c < nt; ++c) { const double m = 0.5 * (P_aug[(size_t)r * nt + c] + P_aug[(size_t)c * nt + r]); P_aug[(size_t)r * nt + c] = m; P_aug[(size_t)c * nt + r] = m; }
    return ORCVIO_OK;
}

int32_t orcvio_msckf_augment_state(int32_t n, int32_t n_new, int32_t idp_dim, const double* H_1, const double* H_2, const double* r_1,
                                   double sigma2, const double* dx, const double* P_upd, double* dx_new, double* P_aug) {
    return augment_state_impl(n, n_new, idp_dim, H_1, H_2, r_1, sigma2, dx, P_upd, false, dx_new, P_aug);
}

// ... with Schmidt nuisance states: the new feature states go IN FRONT of the trailing nui_rows nuisance rows / columns
// (src/orcvio.cpp:1920-1935).  n counts the nuisance states; P_aug [(n + d n_new)^2] in the order [old | new | nuisance].
static int augment_state_nuisance_impl(int32_t n, int32_t n_new, int32_t idp_dim, int32_t nui_rows, const double* H_1, const double* H_2,
                                       const double* r_1, double sigma2, const double* dx, const double* P_upd, bool diag_only, double* dx_new,
                                       double* P_aug) {
    if (nui_rows < 0 || nui_rows > n) { g_last_error = "augment_state_nuisance: invalid argument"; return ORCVIO_ERR_INVALID; }
    const int sz = idp_dim * n_new, nt = n + sz;
    std::vector<double> T((size_t)nt * nt);
    const int rc = augment_state_impl(n, n_new, idp_dim, H_1, H_2, r_1, sigma2, dx, P_upd, diag_only, dx_new, T.data());   // [old + nuisance | new]
    if (rc != ORCVIO_OK) return rc;
    std::vector<int> map(nt);   // map[i] = index in T of row / column i of P_aug
    const int n0 = n - nui_rows;
    for (int i = 0; i < n0; ++i) map[i] = i;
    for (int i = 0; i < sz; ++i) map[n0 + i] = n + i;
    for (int i = 0; i < nui_rows; ++i) map[n0 + sz + i] = n0 + i;
    for (int i = 0; i < nt; ++i)
        for (int j = 0; j < nt; ++j) P_aug[(size_t)i * nt + j] = T[(size_t)map[i] * nt + map[j]];
    return ORCVIO_OK;
}

int32_t orcvio_msckf_augment_state_nuisance(int32_t n, int32_t n_new, int32_t idp_dim, int32_t nui_rows, const double* H_1, const double* H_2,
                                            const double* r_1, double sigma2, const double* dx, const double* P_upd, double* dx_new,
                                            double* P_aug) {
    return augment_state_nuisance_impl(n, n_new, idp_dim, nui_rows, H_1, H_2, r_1, sigma2, dx, P_upd, false, dx_new, P_aug);
}
int32_t orcvio_msckf_augment_state_ref_ldlt(int32_t n, int32_t n_new, int32_t idp_dim, int32_t nui_rows, const double* H_1, const double* H_2,
                                            const double* r_1, double sigma2, const double* dx, const double* P_upd, double* dx_new,
                                            double* P_aug) {
    return augment_state_nuisance_impl(n, n_new, idp_dim, nui_rows, H_1, H_2, r_1, sigma2, dx, P_upd, true, dx_new, P_aug);
}

int32_t orcvio_msckf_download_ekf(orcvio_msckf_handle* h, double* gamma, int32_t* accept) {
    if (!h || !h->ran) { g_last_error = "download_ekf: no finished update"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->last_stream ? h->last_stream : h->stream;
    if (h->ekf_F > 0) {
        const FetchCopy fc[] = {{gamma, h->d_ekf_gamma, sizeof(double) * (size_t)h->ekf_F}, {accept, h->d_ekf_accept, sizeof(int) * (size_t)h->ekf_F}};
        return fetch_copies(h, s, fc, 2);
    }
    HIPCHK(hipStreamSynchronize(s));
    return ORCVIO_OK;
}

static int run_update_impl(orcvio_msckf_handle* h, void* stream, UpdateCall& c) {
    if (!h || !h->uploaded) { g_last_error = "run_update: nothing uploaded"; return ORCVIO_ERR_INVALID; }
    if (h->pw_missing) { g_last_error = "run_update: tracks were uploaded without positions and have not been triangulated"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = pick_stream(h, stream);
    h->last_stream = s;
    if (h->dl_pending) { HIPCHK(hipStreamSynchronize(h->dl_stream)); h->dl_pending = false; }   // (a copy of the previous results nobody fetched)
    int rc = run_with_graph(h, h->g_update, launch_signature(h, s, nullptr, 0, c), s, [&](bool) { return enqueue_update(h, s, c); });
    h->A_deferred = front_defers_assembly(h, c.retry_forked);   // (a replayed graph does not pass through enqueue_update)
    if (rc == ORCVIO_OK) mark_update_enqueued(h, 0);
    return rc;
}
int32_t orcvio_msckf_run_update(orcvio_msckf_handle* h, void* stream) {
    UpdateCall c;
    return run_update_impl(h, stream, c);
}

int32_t orcvio_msckf_sync(orcvio_msckf_handle* h, void* stream) {
    if (!h) return ORCVIO_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    if (h->comm || h->ipc) {   // the stream may carry a collective: a bounded wait (ORCVIO_ERR_TIMEOUT instead of a hang)
        const int rw = comm_stream_wait(h, pick_stream(h, stream), "orcvio_msckf_sync");
        if (rw != ORCVIO_OK) return rw;
        { const int rl = ipc_check_lost(h, "orcvio_msckf_sync"); if (rl != ORCVIO_OK) return rl; }
    } else
        HIPCHK(hipStreamSynchronize(pick_stream(h, stream)));
    HIPCHK(hipStreamSynchronize(h->side));
    return ORCVIO_OK;
}
