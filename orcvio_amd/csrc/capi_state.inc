// capi_state.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// triangulation, incrementState_IMUCam (host arithmetic).

// ---- feature triangulation (SURVEY.md 8f rank 1) --------------------------------------------------
void orcvio_msckf_triangulation_config_default(orcvio_triangulation_config* c) {
    if (!c) return;
    c->translation_threshold = 0.2; c->huber_epsilon = 0.01; c->estimation_precision = 5e-7; c->initial_damping = 1e-3;
    c->outer_loop_max_iteration = 10; c->inner_loop_max_iteration = 10; c->cost_threshold = 4.7673e-04;
    c->init_final_dist_threshold = 5.0;
}

// io: the launch inside an armed in-place update (orcvio_msckf_io_triangulate) -- the modes out of the handle's pinned block (with_mode),
// the results published into it
// prune: the launch of the frame's second update (orcvio_msckf_io_triangulate_prune) -- the CSR is the staged list in HBM, the modes and
// the results the second block's, p_w / d_skip the (swapped-in) second arena's; raise: word [2] of the kept status words
static int launch_triangulate(orcvio_msckf_handle* h, const orcvio_triangulation_config* cfg, bool have_init, bool mark_skip, hipStream_t s,
                              bool io, bool with_mode, bool prune, int* raise) {
    if (h->F == 0) return ORCVIO_OK;
    TriArgs a{};
    if (prune) {
        const TriBlock b = tri_block_layout(h->maxF);
        const TriList l = tri_list_layout(h->tri2_F, h->tri2_nobs);
        char* d = h->h_tri2_dev;
        a.mode = reinterpret_cast<const int*>(d + b.mode);
        a.pub_valid = reinterpret_cast<int*>(d + b.valid); a.pub_flags = reinterpret_cast<int*>(d + b.flags);
        a.pub_cost = reinterpret_cast<double*>(d + b.cost); a.pub_pw = reinterpret_cast<double*>(d + b.p_w);
        a.pub_sol = reinterpret_cast<double*>(d + b.inv_param);
        a.words = h->d_tri2_words; a.raise = raise;
        a.obs_ptr = reinterpret_cast<const int*>(h->d_tri2_list + l.obs_ptr); a.obs_clone = reinterpret_cast<const int*>(h->d_tri2_list + l.obs_clone);
        a.obs_z = reinterpret_cast<const double*>(h->d_tri2_list + l.obs_z);
    } else if (io) {
        const TriBlock b = tri_block_layout(h->maxF);
        char* d = h->h_tri_dev;
        a.mode = with_mode ? reinterpret_cast<const int*>(d + b.mode) : nullptr;
        a.pub_valid = reinterpret_cast<int*>(d + b.valid); a.pub_flags = reinterpret_cast<int*>(d + b.flags);
        a.pub_cost = reinterpret_cast<double*>(d + b.cost); a.pub_pw = reinterpret_cast<double*>(d + b.p_w);
        a.pub_sol = reinterpret_cast<double*>(d + b.inv_param);
        a.words = h->d_tri_words;
    }
    a.poses = h->d_poses;
    if (!prune) { a.obs_ptr = h->d_obs_ptr; a.obs_clone = h->d_obs_clone; a.obs_z = h->d_obs_z; }
    a.is_init = have_init ? h->d_tri_init : nullptr;
    a.p_w = h->d_pw; a.valid = h->d_tri_valid; a.flags = h->d_tri_flags; a.solution = h->d_tri_sol; a.cost = h->d_tri_cost;
    a.skip = mark_skip ? h->d_skip : nullptr;
    a.translation_threshold = cfg->translation_threshold; a.huber_epsilon = cfg->huber_epsilon;
    a.estimation_precision = cfg->estimation_precision; a.initial_damping = cfg->initial_damping;
    a.cost_threshold = cfg->cost_threshold; a.init_final_dist_threshold = cfg->init_final_dist_threshold;
    a.outer_max = cfg->outer_loop_max_iteration; a.inner_max = cfg->inner_loop_max_iteration;
    a.F = h->F;
    hipLaunchKernelGGL(k_triangulate, dim3(h->F), dim3(64), 0, s, a);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

int32_t orcvio_msckf_triangulate_uploaded(orcvio_msckf_handle* h, const orcvio_triangulation_config* cfg,
                                          const int32_t* is_initialized, void* stream) {
    if (!h || !cfg || !h->uploaded || h->objects_mode) { g_last_error = "triangulate_uploaded: no uploaded tracks"; return ORCVIO_ERR_INVALID; }
    if (h->pw_missing && is_initialized) { g_last_error = "triangulate_uploaded: is_initialized needs uploaded positions"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = pick_stream(h, stream);
    if (is_initialized && h->F > 0) {
        const AuxCopy cp[] = {{h->d_tri_init, is_initialized, sizeof(int) * (size_t)h->F}};   // (the caller's memory: through the bounce buffer)
        { const int rc = aux_copies(h, s, cp, 1); if (rc != ORCVIO_OK) return rc; }
    }
    int rc = launch_triangulate(h, cfg, is_initialized != nullptr, true, s, false, false, false, nullptr);
    if (rc != ORCVIO_OK) return rc;
    h->skip_active = true;
    h->pw_missing = false;
    return ORCVIO_OK;
}

// Arms the next update on the open arena (capi_io.inc tri_consume / io_enqueue): nothing is enqueued here.  The modes are copied into
// the handle's pinned block, out of which the kernel reads them; the config is kept by value.
int32_t orcvio_msckf_io_triangulate(orcvio_msckf_handle* h, const orcvio_triangulation_config* cfg, const int32_t* mode, orcvio_msckf_io_tri* out) {
    const char* who = "orcvio_msckf_io_triangulate: ";
    if (!h || !out) { g_last_error = std::string(who) + "null argument"; return ORCVIO_ERR_INVALID; }
    if (!h->io_open) { g_last_error = std::string(who) + "call orcvio_msckf_io_begin first"; return ORCVIO_ERR_INVALID; }
    if (h->io_submitted) { g_last_error = std::string(who) + "an update submitted with orcvio_msckf_io_submit has not been collected"; return ORCVIO_ERR_INVALID; }
    if (h->objects_mode) { g_last_error = std::string(who) + "the arena holds an object update"; return ORCVIO_ERR_INVALID; }
    if (h->comm || h->ipc) { g_last_error = std::string(who) + "not with a communicator on the handle"; return ORCVIO_ERR_INVALID; }
    const TriBlock b = tri_block_layout(h->maxF);
    if (!h->h_tri) {
        if (!tri_config_ok(cfg)) { g_last_error = std::string(who) + "a NULL or non-finite config (iteration counts must not be negative)"; return ORCVIO_ERR_INVALID; }
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipHostMalloc(&h->h_tri, b.bytes, hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_tri_dev), h->h_tri, 0));
        std::memset(h->h_tri, 0, b.bytes);
        HIPCHK(hipMalloc(&h->d_tri_words, 64));
        HIPCHK(hipMemset(h->d_tri_words, 0, 64));
    }
    // (every reader and writer of the block on the device belongs to an update whose wait has returned: io_submitted is refused above)
    const char* why = "";
    const int rc = tri_arm_stage(cfg, mode, h->F, h->maxF, h->h_tri, &why);
    if (rc != ORCVIO_OK) { g_last_error = std::string(who) + why; return rc; }
    h->tri_cfg = *cfg;
    h->tri_with_mode = mode != nullptr;
    h->tri_armed = true;
    out->valid = reinterpret_cast<const int32_t*>(h->h_tri + b.valid);
    out->flags = reinterpret_cast<const int32_t*>(h->h_tri + b.flags);
    out->cost = reinterpret_cast<const double*>(h->h_tri + b.cost);
    out->p_w = reinterpret_cast<const double*>(h->h_tri + b.p_w);
    out->inv_param = reinterpret_cast<const double*>(h->h_tri + b.inv_param);
    return ORCVIO_OK;
}

// Arms the SECOND update of the next frame call (capi_step.inc): nothing is enqueued here.  The list and the modes are copied into the
// handle's second pinned block (tri_prune_arm_stage), the config is kept by value.
int32_t orcvio_msckf_io_triangulate_prune(orcvio_msckf_handle* h, const orcvio_triangulation_config* cfg, const orcvio_msckf_tracks* tri_tracks,
                                          const int32_t* mode, orcvio_msckf_io_tri* out) {
    const char* who = "orcvio_msckf_io_triangulate_prune: ";
    if (!h || !out) { g_last_error = std::string(who) + "null argument"; return ORCVIO_ERR_INVALID; }
    if (!h->io_open) { g_last_error = std::string(who) + "call orcvio_msckf_io_begin first"; return ORCVIO_ERR_INVALID; }
    if (h->io_submitted) { g_last_error = std::string(who) + "an update submitted with orcvio_msckf_io_submit has not been collected"; return ORCVIO_ERR_INVALID; }
    if (h->objects_mode) { g_last_error = std::string(who) + "the arena holds an object update"; return ORCVIO_ERR_INVALID; }
    if (h->comm || h->ipc) { g_last_error = std::string(who) + "not with a communicator on the handle"; return ORCVIO_ERR_INVALID; }
    const TriPruneBlock b = tri_prune_layout(h->maxF, h->maxObs);
    if (!h->h_tri2) {
        if (!tri_config_ok(cfg)) { g_last_error = std::string(who) + "a NULL or non-finite config (iteration counts must not be negative)"; return ORCVIO_ERR_INVALID; }
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipMalloc(&h->d_tri2_list, b.bytes - b.list));
        HIPCHK(hipMemset(h->d_tri2_list, 0, b.bytes - b.list));
        HIPCHK(hipMalloc(&h->d_tri2_words, 64));
        HIPCHK(hipMemset(h->d_tri2_words, 0, 64));
        HIPCHK(hipMalloc(&h->d_skip2, sizeof(int) * (size_t)(h->maxF > 0 ? h->maxF : 1)));
        HIPCHK(hipMemset(h->d_skip2, 0, sizeof(int) * (size_t)(h->maxF > 0 ? h->maxF : 1)));
        HIPCHK(hipHostMalloc(&h->h_tri2, b.bytes, hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_tri2_dev), h->h_tri2, 0));
        std::memset(h->h_tri2, 0, b.bytes);
    }
    // (every reader and writer of the block on the device belongs to a frame whose wait has returned)
    const char* why = "";
    const int rc = tri_prune_arm_stage(cfg, tri_tracks, mode, h->N, h->maxF, h->maxObs, h->h_tri2, &why);
    if (rc != ORCVIO_OK) { g_last_error = std::string(who) + why; return rc; }
    h->tri2_cfg = *cfg;
    h->tri2_F = tri_tracks->n_features; h->tri2_nobs = tri_tracks->obs_ptr[tri_tracks->n_features];
    h->tri2_armed = true;
    out->valid = reinterpret_cast<const int32_t*>(h->h_tri2 + b.res.valid);
    out->flags = reinterpret_cast<const int32_t*>(h->h_tri2 + b.res.flags);
    out->cost = reinterpret_cast<const double*>(h->h_tri2 + b.res.cost);
    out->p_w = reinterpret_cast<const double*>(h->h_tri2 + b.res.p_w);
    out->inv_param = reinterpret_cast<const double*>(h->h_tri2 + b.res.inv_param);
    return ORCVIO_OK;
}

int32_t orcvio_msckf_triangulate(orcvio_msckf_handle* h, const orcvio_triangulation_config* cfg, const orcvio_msckf_window* w,
                                 const orcvio_msckf_tracks* tr, const int32_t* is_initialized, orcvio_triangulation_result* res) {
    if (!h || !cfg || !w || !tr || !res || !w->R_b2w || !w->t_b_w || !w->R_b2c || !w->t_c_b || !tr->obs_ptr) {
        g_last_error = "orcvio_msckf_triangulate: null argument";
        return ORCVIO_ERR_INVALID;
    }
    const int N = w->n_clones, F = tr->n_features;
    if (N < 1 || F < 0) { g_last_error = "orcvio_msckf_triangulate: bad sizes"; return ORCVIO_ERR_INVALID; }
    if (N > h->maxN || F > h->maxF) { g_last_error = "orcvio_msckf_triangulate: exceeds handle capacity"; return ORCVIO_ERR_CAPACITY; }
    if (F > 0 && tr->obs_ptr[0] < 0) { g_last_error = "orcvio_msckf_triangulate: obs_ptr starts below zero"; return ORCVIO_ERR_INVALID; }
    const int nobs = F > 0 ? tr->obs_ptr[F] : 0;
    if (nobs < 0) { g_last_error = "orcvio_msckf_triangulate: obs_ptr not monotone"; return ORCVIO_ERR_INVALID; }
    if (nobs > h->maxObs) { g_last_error = "orcvio_msckf_triangulate: too many observations"; return ORCVIO_ERR_CAPACITY; }
    if (F > 0 && (!tr->obs_clone || !tr->obs_z)) { g_last_error = "orcvio_msckf_triangulate: null track arrays"; return ORCVIO_ERR_INVALID; }
    if (is_initialized && !tr->p_w) { g_last_error = "orcvio_msckf_triangulate: is_initialized needs tracks->p_w"; return ORCVIO_ERR_INVALID; }
    for (int j = 0; j < F; ++j) {
        const int M = tr->obs_ptr[j + 1] - tr->obs_ptr[j];
        if (M < 0) { g_last_error = "orcvio_msckf_triangulate: obs_ptr not monotone"; return ORCVIO_ERR_INVALID; }
        if (M > 64) { g_last_error = "orcvio_msckf_triangulate: track longer than 64 observations"; return ORCVIO_ERR_TRACK_TOO_LONG; }
    }
    for (int o = 0; o < nobs; ++o)
        if (tr->obs_clone[o] < 0 || tr->obs_clone[o] >= N) { g_last_error = "orcvio_msckf_triangulate: obs_clone out of range"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    // this call owns the track buffers: whatever was uploaded for an update is gone
    h->uploaded = false; h->ran = false; h->skip_active = false; h->objects_mode = false; h->io_open = false;
    drop_one_shot_armings(h);
    h->tri_live = false; h->tri_refuse_empty = false; h->tri_live_prune = false;
    h->N = N; h->F = F; h->nobs = nobs;
    HIPCHK(hipStreamSynchronize(s));
    if (h->dl_pending) { HIPCHK(hipStreamSynchronize(h->dl_stream)); h->dl_pending = false; }
    layout_inputs(h, N, F, nobs, false, true, h->n_max);
    h->h_poses.assign((size_t)POSE_STRIDE * N, 0.0);
    const double* tfej = w->t_fej ? w->t_fej : w->t_b_w;
    for (int i = 0; i < N; ++i) {
        double* r = &h->h_poses[(size_t)POSE_STRIDE * i];
        std::memcpy(r + POSE_R_B2W, w->R_b2w + 9 * i, 9 * sizeof(double));
        std::memcpy(r + POSE_T_B_W, w->t_b_w + 3 * i, 3 * sizeof(double));
        std::memcpy(r + POSE_T_FEJ, tfej + 3 * i, 3 * sizeof(double));
        std::memcpy(r + POSE_R_B2C, w->R_b2c + 9 * i, 9 * sizeof(double));
        std::memcpy(r + POSE_T_C_B, w->t_c_b + 3 * i, 3 * sizeof(double));
    }
    {   // the caller's (pageable) arrays through the pinned bounce buffer: asynchronous copies, nothing to wait for
        const size_t Fz = (size_t)F, nz = (size_t)nobs;
        const AuxCopy cp[] = {
            {h->d_poses, h->h_poses.data(), sizeof(double) * POSE_STRIDE * (size_t)N}, {h->d_obs_ptr, tr->obs_ptr, sizeof(int) * (Fz + 1)},
            {h->d_pw, tr->p_w, (F > 0 && tr->p_w) ? sizeof(double) * 3 * Fz : 0}, {h->d_tri_init, is_initialized, (F > 0 && is_initialized) ? sizeof(int) * Fz : 0},
            {h->d_obs_clone, tr->obs_clone, (F > 0 && nobs > 0) ? sizeof(int) * nz : 0}, {h->d_obs_z, tr->obs_z, (F > 0 && nobs > 0) ? sizeof(double) * 2 * nz : 0}};
        const int rc = aux_copies(h, s, cp, (int)(sizeof(cp) / sizeof(cp[0])));
        if (rc != ORCVIO_OK) return rc;
    }
    int rc = launch_triangulate(h, cfg, is_initialized != nullptr, false, s, false, false, false, nullptr);
    if (rc != ORCVIO_OK) return rc;
    if (F > 0) {
        // results: into ONE pinned block by asynchronous copies, one synchronisation, then into the caller's arrays
        const size_t Fz = (size_t)F;
        const FetchCopy fc[] = {{res->valid, h->d_tri_valid, sizeof(int) * Fz}, {res->flags, h->d_tri_flags, sizeof(int) * Fz},
                                {res->p_w, h->d_pw, sizeof(double) * 3 * Fz}, {res->inv_param, h->d_tri_sol, sizeof(double) * 3 * Fz},
                                {res->cost, h->d_tri_cost, sizeof(double) * Fz}};
        return fetch_copies(h, s, fc, (int)(sizeof(fc) / sizeof(fc[0])));
    }
    HIPCHK(hipStreamSynchronize(s));
    return ORCVIO_OK;
}

// ---- incrementState_IMUCam (src/orcvio.cpp:4468-4567): host arithmetic -------------------------
static void so3_exp(const double w[3], double R[9]);
static void so3_exp_decl(const double w[3], double R[9]) { so3_exp(w, R); }
static void so3_exp(const double w[3], double R[9]) {
    // Sophus v1.0.0 SO3d::exp: unit quaternion from the rotation vector, then to a matrix
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double th = std::sqrt(th2);
    double imag, real;
    if (th < 1e-10) {
        const double th4 = th2 * th2;
        imag = 0.5 - th2 / 48.0 + th4 / 3840.0;
        real = 1.0 - th2 / 8.0 + th4 / 384.0;
    } else {
        imag = std::sin(0.5 * th) / th;
        real = std::cos(0.5 * th);
    }
    const double x = imag * w[0], y = imag * w[1], z = imag * w[2], q = real;
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * q); R[2] = 2 * (x * z + y * q);
    R[3] = 2 * (x * y + z * q); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * q);
    R[6] = 2 * (x * z - y * q); R[7] = 2 * (y * z + x * q); R[8] = 1 - 2 * (x * x + y * y);
}
static void mat3_mul(const double* A, const double* B, double* C) {
    double T[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
    std::memcpy(C, T, sizeof(T));
}

int32_t orcvio_msckf_increment_state(const orcvio_msckf_flags* f, const double* dx, orcvio_msckf_state* st) {
    if (!f || !dx || !st || !st->clone_R_b2w || !st->clone_t_b_w) { g_last_error = "increment_state: null argument"; return -1; }
    const int leg = f->leg_dim;
    const double nv = std::sqrt(dx[3] * dx[3] + dx[4] * dx[4] + dx[5] * dx[5]);
    const double np = std::sqrt(dx[6] * dx[6] + dx[7] * dx[7] + dx[8] * dx[8]);
    if ((nv > 1.0 || np > 1.5) && f->discard_large_update) return 0;   // :4479-4494
    const bool left = f->use_larvio || f->use_left_perturbation;          // :4498, :4543
    double Rt[9];
    so3_exp(dx, Rt);
    if (left) mat3_mul(Rt, st->R_b2w_imu, st->R_b2w_imu); else mat3_mul(st->R_b2w_imu, Rt, st->R_b2w_imu);
    for (int i = 0; i < 3; ++i) {
        st->v[i] += dx[3 + i];
        st->p[i] += dx[6 + i];
        st->bg[i] += dx[9 + i];
        st->ba[i] += dx[12 + i];
    }
    {   // extrinsic: R_b2c <- R_b2c * R(smallAngleQuaternion(dtheta))^T  (:4512-4516, math_utils.hpp:104-121)
        double q[4] = {0.5 * dx[15], 0.5 * dx[16], 0.5 * dx[17], 0.0};
        const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
        if (n2 <= 1.0) q[3] = std::sqrt(1.0 - n2);
        else {
            q[3] = 1.0;
            const double s = 1.0 / std::sqrt(1.0 + n2);
            for (double& v : q) v *= s;
        }
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        // Eigen Quaterniond(w,x,y,z).toRotationMatrix() -- no normalisation, as Eigen does
        const double Rq[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                              2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                              2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
        double RqT[9];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) RqT[i * 3 + j] = Rq[j * 3 + i];
        mat3_mul(st->R_b2c, RqT, st->R_b2c);
        for (int i = 0; i < 3; ++i) st->t_c_b[i] += dx[18 + i];
    }
    st->td += dx[21];
    if (leg == 46) for (int i = 0; i < 24; ++i) st->imu_intrinsics[i] += dx[22 + i];   // :4522-4533
    for (int c = 0; c < st->n_clones; ++c) {
        const double* da = dx + leg + 6 * c;
        double* R = st->clone_R_b2w + 9 * c;
        double* t = st->clone_t_b_w + 3 * c;
        so3_exp(da, Rt);
        if (left) mat3_mul(Rt, R, R); else mat3_mul(R, Rt, R);
        for (int i = 0; i < 3; ++i) t[i] += da[3 + i];
        if (st->clone_R_c2w) {   // orientation_cam = R_b2w * R_b2c^T (:4555-4561)
            double RbcT[9];
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) RbcT[i * 3 + j] = st->R_b2c[j * 3 + i];
            mat3_mul(R, RbcT, st->clone_R_c2w + 9 * c);
        }
        if (st->clone_t_c_w)
            for (int i = 0; i < 3; ++i)
                st->clone_t_c_w[3 * c + i] = t[i] + R[i * 3] * st->t_c_b[0] + R[i * 3 + 1] * st->t_c_b[1] + R[i * 3 + 2] * st->t_c_b[2];
    }
    return 1;
}
