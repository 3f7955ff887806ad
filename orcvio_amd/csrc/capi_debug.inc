// capi_debug.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// diagnostics build only: test hooks and ablation timers.

// ---- diagnostics: test hooks and ablation timers.  NOT part of the product ABI: compiled only into the diagnostics build
//      (orcvio_amd/lib/liborcvio_msckf_dbg.so, -DORCVIO_DEBUG_HOOKS), which the tests that need them load explicitly ----------
#ifdef ORCVIO_DEBUG_HOOKS
// ---- debug access to intermediate device buffers (tests only; not part of the public header) ---
// which: 0 Hs [m_tot x NAP], 1 Ab, 2 A (summed block), 3 RP, 4 M, 5 RM, 6 Z, 8 U, 7 dims -> int32[8],
//        11 {fac_valid, fac_n, fac_k, res_n} -> int32[4], 12 the resident factor [fac_k][fac_n],
//        13 the dense rows [dense_rows][NAP] (caller-projected rows, then the rows of the entering features: zero U part, V part),
//        14 {dense_rows, NAP} -> int32[2],
//        15 did the last object update take the one-launch compression (k_obj_fused)? -> int32,
//        16 the n x n prior of the last update as it stands in device memory (h->d_P: a host P as its pull left it),
//        17 T3 [3F][NAP], 18 Xobs [2 nobs][16], 19 obs_pos -> int32[nobs], 20 S [N][256], 21 Gpart [chunks][NAP^2],
//        22 {F, N, nobs, chunks, rows per chunk, k_front?, A deferred?, prior forked?} -> int32[8]
int32_t orcvio_msckf_debug_read(orcvio_msckf_handle* h, int32_t which, void* dst, int64_t max_bytes) {
    if (!h || !dst) return ORCVIO_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t pp = (size_t)h->NAP * h->NAP * sizeof(double);
    const size_t np2 = (size_t)h->NP * h->NP * sizeof(double);
    const void* src = nullptr;
    size_t bytes = 0;
    switch (which) {
        case 0:
            if (!h->materialize) { g_last_error = "debug_read: stack not materialised (ORCVIO_OPT_MATERIALIZE_STACK)"; return ORCVIO_ERR_INVALID; }
            src = h->d_Hs; bytes = (size_t)h->m_tot * h->NAP * sizeof(double); break;
        case 1: src = h->d_Ab; bytes = pp; break;
        case 2: {
            const int ra = assemble_deferred(h, h->stream);
            if (ra != ORCVIO_OK) return ra;
            HIPCHK(hipDeviceSynchronize());
            src = h->d_A; bytes = pp; break;
        }
        case 3: src = h->d_RP; bytes = np2; break;
        case 4: src = h->d_M; bytes = np2; break;
        case 5: src = h->d_RM; bytes = np2; break;
        case 6: src = h->d_Z; bytes = (size_t)h->n * h->ldz * sizeof(double); break;
        case 8: src = h->d_U; bytes = np2; break;
        case 9: src = h->d_sync; bytes = 256; break;   // k_front: counter + diagnostic time stamps
        case 10: {   // how often an update was re-run on the forked path because the fused front end lost a hand-off
            if ((size_t)max_bytes < sizeof(int32_t)) return ORCVIO_ERR_INVALID;
            *reinterpret_cast<int32_t*>(dst) = h->front_fallbacks;
            return ORCVIO_OK;
        }
        case 11: {   // the resident covariance and its square-root factor: {fac_valid, fac_n, fac_k, res_n}
            int32_t st[4] = {h->fac_valid ? 1 : 0, h->fac_n, h->fac_k, h->res_n};
            if ((size_t)max_bytes < sizeof(st)) return ORCVIO_ERR_INVALID;
            std::memcpy(dst, st, sizeof(st));
            return ORCVIO_OK;
        }
        case 12: {   // the resident factor itself: [fac_k][fac_n] (S(j, i) at [i][j]), the padding to fac_ld dropped
            if (!h->fac_valid) { g_last_error = "debug_read: no resident factor"; return ORCVIO_ERR_INVALID; }
            if ((size_t)max_bytes < (size_t)h->fac_k * h->fac_n * sizeof(double)) { g_last_error = "debug_read: buffer too small"; return ORCVIO_ERR_INVALID; }
            HIPCHK(hipMemcpy2D(dst, sizeof(double) * h->fac_n, h->d_Sres, sizeof(double) * h->fac_ld, sizeof(double) * h->fac_n, h->fac_k,
                               hipMemcpyDeviceToHost));
            return ORCVIO_OK;
        }
        case 13: src = h->d_dense; bytes = (size_t)h->dense_rows * h->NAP * sizeof(double); break;
        case 14: {
            int32_t dd[2] = {h->dense_rows, h->NAP};
            if ((size_t)max_bytes < sizeof(dd)) return ORCVIO_ERR_INVALID;
            std::memcpy(dst, dd, sizeof(dd));
            return ORCVIO_OK;
        }
        case 15: {   // the route of the last object update: 1 k_obj_fused, 0 the three-launch pipeline
            if ((size_t)max_bytes < sizeof(int32_t)) return ORCVIO_ERR_INVALID;
            *reinterpret_cast<int32_t*>(dst) = h->obj_last_fused ? 1 : 0;
            return ORCVIO_OK;
        }
        case 16: src = h->d_P; bytes = (size_t)h->n * h->n * sizeof(double); break;   // the prior as the pull left it in device memory
        // ---- the front end of the last feature update, as its launches left it (tests/test_gpu_front_blocks.py) ----
        case 17: src = h->d_T3; bytes = (size_t)3 * h->F * h->NAP * sizeof(double); break;      // T3 [3F][NAP]
        case 18: src = h->d_Xobs; bytes = (size_t)32 * h->nobs * sizeof(double); break;         // Xobs [2 nobs][16]
        case 19: {   // obs_pos [nobs]: the position of every observation in the clone-sorted order (rows 2 pos, 2 pos + 1 of Xobs), as
                     // upload_finalize left it in the arena -- the list every route reads, there or through its pull
            const size_t b = sizeof(int32_t) * (size_t)h->nobs;
            if (!h->uploaded || h->objects_mode) { g_last_error = "debug_read: no feature upload"; return ORCVIO_ERR_INVALID; }
            if ((size_t)max_bytes < b) { g_last_error = "debug_read: buffer too small"; return ORCVIO_ERR_INVALID; }
            if (b) std::memcpy(dst, h->h_stage + h->io_cobs, b);
            return ORCVIO_OK;
        }
        case 20: src = h->d_S; bytes = (size_t)256 * h->N * sizeof(double); break;              // S [N][256], one tile per clone
        case 21: {   // Gpart [chunks][NAP^2]: the partial Grams of T3 the last front end wrote (lower tiles; both triangles behind k_front)
            const int ch = front_fused_active(h, false) ? h->front_chunks : h->chunks;
            src = h->d_Gpart; bytes = (size_t)ch * pp; break;
        }
        case 22: {   // {F, N, nobs, row chunks of the last front end, rows per chunk, would this upload take k_front?, is A still to be
                     //  assembled (k_front left the Grams only)?, was the prior's factorisation forked?}
            const bool fused = front_fused_active(h, false);
            const int ch = fused ? h->front_chunks : h->chunks;
            const int t3 = 3 * h->F;
            const int rpc = fused ? round_up((t3 + ch - 1) / ch, 4) : h->rows_per_chunk;
            int32_t st[8] = {h->F, h->N, h->nobs, ch, rpc, fused ? 1 : 0, h->A_deferred ? 1 : 0, h->prior_forked ? 1 : 0};
            if ((size_t)max_bytes < sizeof(st)) return ORCVIO_ERR_INVALID;
            std::memcpy(dst, st, sizeof(st));
            return ORCVIO_OK;
        }
        case 7: {
            int32_t dims[8] = {h->n, h->NA, h->NAP, h->NP, h->m_tot, h->Mmax, h->ldz, h->reg_path ? 1 : 0};
            if ((size_t)max_bytes < sizeof(dims)) return ORCVIO_ERR_INVALID;
            std::memcpy(dst, dims, sizeof(dims));
            return ORCVIO_OK;
        }
        default: return ORCVIO_ERR_INVALID;
    }
    if ((size_t)max_bytes < bytes) { g_last_error = "debug_read: buffer too small"; return ORCVIO_ERR_INVALID; }
    if (bytes) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return ORCVIO_OK;
}

// Test hook: advance the ipc transport's update counter of THIS rank by `by` without an update -- what a rank-local early return used
// to leave behind (ADVICE r4).  The next sharded update must fail loudly on every rank, never sum another update's blocks.
int32_t orcvio_msckf_debug_ipc_skew(orcvio_msckf_handle* h, int32_t by) {
    if (!h || !h->ipc) return ORCVIO_ERR_INVALID;
    h->ipc->seq += (unsigned long long)by;
    return ORCVIO_OK;
}

// Test hook: hold `n_cus` compute units for `ms` milliseconds with a spinning kernel on the handle's SIDE stream (returns at once).
int32_t orcvio_msckf_debug_occupy(orcvio_msckf_handle* h, int32_t n_cus, double ms) {
    if (!h || n_cus < 1 || ms <= 0.0) return ORCVIO_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    static bool attr = false;
    if (!attr) { HIPCHK(hipFuncSetAttribute((const void*)k_debug_occupy, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr = true; }
    hipLaunchKernelGGL(k_debug_occupy, dim3(n_cus), dim3(64), (size_t)150 * 1024, h->side, (unsigned long long)(ms * 1e5), h->d_info + 40);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

// Test hook: factor an arbitrary symmetric n x n host matrix with the same kernels the update uses.
// rev: factor the reversed matrix X'(i, j) = X(n-1-i, n-1-j), as the update factors its prior (register path only).
// Out: L (n x n lower, row-major, host; with rev the factor L' of X' as stored), Dinv ([nb][16][16]), info[2] (dropped / negative pivots).
int32_t orcvio_msckf_debug_potrf(orcvio_msckf_handle* h, const double* X, int32_t n, double tol_rel, int32_t force_lds_path,
                                 double* L_out, double* Dinv_out, int32_t* info_out, int32_t rev) {
    if (!h || !X || n < 1 || n > h->n_max) return ORCVIO_ERR_INVALID;
    if (rev && (force_lds_path || (n + 15) / 16 > 14)) return ORCVIO_ERR_INVALID;   // (only k_potrf_reg reads its input reversed)
    HIPCHK(hipSetDevice(h->device));
    const int saveNP = h->NP;
    const bool save_path = h->reg_path;
    h->NP = round_up(n, 16);
    h->reg_path = !force_lds_path && (h->NP / 16) <= 14;
    const int NP = h->NP;
    HIPCHK(hipMemcpy(h->d_M, X, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(h->d_info, 0, sizeof(int) * 8));
    HIPCHK(hipMemset(h->d_RM, 0, sizeof(double) * (size_t)h->NP_max * h->NP_max));   // lower tiles: zero for any layout
    int rc = launch_potrf(h, h->stream, h->d_M, n, n, tol_rel, h->d_RM, h->d_DinvM, h->d_info, rev ? 1 : 0);
    if (rc == ORCVIO_OK) {
        HIPCHK(hipStreamSynchronize(h->stream));
        std::vector<double> buf((size_t)NP * NP);
        HIPCHK(hipMemcpy(buf.data(), h->d_RM, sizeof(double) * buf.size(), hipMemcpyDeviceToHost));
        long sLi, sLj;
        factor_strides(h, sLi, sLj);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) L_out[(size_t)i * n + j] = buf[(size_t)i * sLi + (size_t)j * sLj];
        if (Dinv_out) HIPCHK(hipMemcpy(Dinv_out, h->d_DinvM, sizeof(double) * 256 * ((n + 15) / 16), hipMemcpyDeviceToHost));
        if (info_out) HIPCHK(hipMemcpy(info_out, h->d_info, sizeof(int) * 2, hipMemcpyDeviceToHost));
        HIPCHK(hipMemset(h->d_info, 0, sizeof(int) * 8));
        // d_RM lower tiles may now hold data of another leading dimension: restore the invariant
        HIPCHK(hipMemset(h->d_RM, 0, sizeof(double) * (size_t)h->NP_max * h->NP_max));
    }
    h->NP = saveNP;
    h->reg_path = save_path;
    return rc;
}

// Test hook: Z = L^-1 B with the factor left in the handle by orcvio_msckf_debug_potrf_keep (same call
// with keep = 1 semantics: call debug_potrf first, then this before anything else).
int32_t orcvio_msckf_debug_trsm(orcvio_msckf_handle* h, const double* X, int32_t n, const double* B, int32_t nrhs, double* Z_out) {
    if (!h || !X || !B || n < 1 || n > h->n_max || nrhs < 1 || nrhs > h->NP_max) return ORCVIO_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    const int saveNP = h->NP, saveldz = h->ldz;
    const bool save_path = h->reg_path;
    h->NP = round_up(n, 16);
    h->reg_path = (h->NP / 16) <= 14;
    const int NP = h->NP;
    HIPCHK(hipMemcpy(h->d_M, X, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_U, B, sizeof(double) * (size_t)n * nrhs, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(h->d_RM, 0, sizeof(double) * (size_t)h->NP_max * h->NP_max));
    int rc = launch_potrf(h, h->stream, h->d_M, n, n, 0.0, h->d_RM, h->d_DinvM, h->d_info);
    if (rc == ORCVIO_OK) rc = launch_trsm(h, h->stream, h->d_RM, h->d_DinvM, n, h->d_U, nrhs, 1, nrhs, nullptr, 0, h->d_Z, h->NP_max);
    if (rc == ORCVIO_OK) {
        HIPCHK(hipStreamSynchronize(h->stream));
        std::vector<double> buf((size_t)n * h->NP_max);
        HIPCHK(hipMemcpy(buf.data(), h->d_Z, sizeof(double) * buf.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < nrhs; ++c) Z_out[(size_t)i * nrhs + c] = buf[(size_t)i * h->NP_max + c];
        HIPCHK(hipMemset(h->d_info, 0, sizeof(int) * 8));
        HIPCHK(hipMemset(h->d_RM, 0, sizeof(double) * (size_t)h->NP_max * h->NP_max));
    }
    (void)NP;
    h->NP = saveNP; h->ldz = saveldz; h->reg_path = save_path;
    return rc;
}

// Diagnostic: time k_potrf_reg on the handle's current P with parts of the algorithm switched off
// (results are garbage for ablate != 0).  Returns the average kernel time in microseconds.
int32_t orcvio_msckf_debug_potrf_ablate(orcvio_msckf_handle* h, int32_t ablate, int32_t reps, double* us_out) {
    if (!h || !h->uploaded || !h->reg_path || !us_out) return ORCVIO_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    const int n = h->n, NP = h->NP;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int rep = 0; rep < 3; ++rep)
        hipLaunchKernelGGL(k_potrf_reg<16>, dim3(1), dim3(512), 0, h->stream, h->d_P, n, n, 1.8e-15, h->d_RP, NP, h->d_DinvP,
                           h->d_info + 6, (unsigned long long*)nullptr, (size_t)0, (size_t)0, (size_t)0, 0, ablate);
    HIPCHK(hipEventRecord(e0, h->stream));
    for (int rep = 0; rep < reps; ++rep)
        hipLaunchKernelGGL(k_potrf_reg<16>, dim3(1), dim3(512), 0, h->stream, h->d_P, n, n, 1.8e-15, h->d_RP, NP, h->d_DinvP,
                           h->d_info + 6, (unsigned long long*)nullptr, (size_t)0, (size_t)0, (size_t)0, 0, ablate);
    HIPCHK(hipEventRecord(e1, h->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *us_out = 1e3 * ms / reps;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ORCVIO_OK;
}

// Diagnostic: core-clock stamps of one k_potrf_reg<12> run on the handle's current P (256 values; layout in potrf_reg_body)
int32_t orcvio_msckf_debug_potrf_stamps(orcvio_msckf_handle* h, unsigned long long* out256) {
    if (!h || !h->uploaded || !h->reg_path || !out256) return ORCVIO_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc(&d, sizeof(unsigned long long) * 256));
    HIPCHK(hipMemset(d, 0, sizeof(unsigned long long) * 256));
    const int n = h->n, NP = h->NP;
    const char* ab = dbg_getenv("ORCVIO_POTRF_ABLATE");   // diagnostic only: phases switched off (results are garbage)
    const int ablate = ab ? atoi(ab) : 0;
    // ORCVIO_POTRF_COLD (after a finished update): factor M instead, each time right behind the k_gemm that writes it from all
    // XCDs -- the conditions of the replayed graph (cold L2 of the factorising CU's XCD) instead of a warm repetition
    const bool cold = dbg_getenv("ORCVIO_POTRF_COLD") != nullptr && h->ran;
    for (int rep = 0; rep < 4; ++rep) {
        if (cold) {
            UpdateCall c;
            const int rcf = launch_solve_stage(h, h->stream, ST_FORM_M, c);
            if (rcf != ORCVIO_OK) return rcf;
            hipLaunchKernelGGL(k_potrf_reg<16>, dim3(1), dim3(512), 0, h->stream, h->d_M, NP, h->kf, 0.0, h->d_RM, NP, h->d_DinvM,
                               h->d_info + 6, d, (size_t)0, (size_t)0, (size_t)0, 0, ablate, 0);
        } else
            hipLaunchKernelGGL(k_potrf_reg<16>, dim3(1), dim3(512), 0, h->stream, h->d_P, n, n, 1.8e-15, h->d_RP, NP, h->d_DinvP,
                               h->d_info + 6, d, (size_t)0, (size_t)0, (size_t)0, 0, ablate);
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out256, d, sizeof(unsigned long long) * 256, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return ORCVIO_OK;
}

// Diagnostic: average time of k_feature with phases switched off (outputs are garbage for ablate != 0).
int32_t orcvio_msckf_debug_feature_ablate(orcvio_msckf_handle* h, int32_t ablate, int32_t reps, double* us_out) {
    if (!h || !h->uploaded || !us_out) return ORCVIO_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    h->feat_ablate = ablate;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int r = 0; r < 3; ++r) launch_feature(h, h->stream);
    HIPCHK(hipEventRecord(e0, h->stream));
    for (int r = 0; r < reps; ++r) launch_feature(h, h->stream);
    HIPCHK(hipEventRecord(e1, h->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *us_out = 1e3 * ms / reps;
    h->feat_ablate = 0;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ORCVIO_OK;
}

// Test hook / diagnostic: chol(X) and Z = L^-1 [B | bx] in ONE launch, through k_potrf_solve (la = 0) or k_potrf_solve_la (la = 2, 3), on an
// arbitrary SPD host matrix X (n x n) and right-hand sides B ((n + tail) x nrhs, row-major), in the argument forms of the update's own
// call (launch_solve_stage, ST_POTRF_M):
//   bx (optional, n values): the extra column behind B, stride 1 (the update's g);
//   tail, tail_scale: `tail` more rows of B behind the n that take part in the factorisation; their rows of Z are tail_scale * B, the
//     extra column's are zero;
//   product_strides: B lies on the device as the update finds the prior's factor -- rows of stride ld (= NP_max), the columns stored in
//     reverse (column stride -1), the base pointer at the last column.  0: rows of stride nrhs, column stride 1.
// The padding of M, the right-hand-side scratch around B and bx, and all of Z are filled with NaN before the launch.
// L_out n x n (lower); Z_out (n + tail + 1) x (ncols + 1), ncols = nrhs + (bx != NULL): Z, then one guard row and one guard column of the
// scratch as the launch left them (NaN = untouched; NaN too where the scratch ends with Z); outside_out (optional): how many entries of the
// whole Z scratch outside Z's extent are no longer NaN; info_out[3] (dropped pivots, non-positive pivots, lost hand-offs), stamps
// (optional, 512 words: potrf_lookahead.hpp), us_out (optional: average launch time over `reps` launches, each behind the two small clears
// it needs).
int32_t orcvio_msckf_debug_potrf_solve(orcvio_msckf_handle* h, const double* X, int32_t n, const double* B, int32_t nrhs, int32_t la,
                                       double* L_out, double* Z_out, int32_t* info_out, unsigned long long* stamps, int32_t reps, double* us_out,
                                       const double* bx, int32_t tail, double tail_scale, int32_t product_strides, int32_t* outside_out) {
    if (!h || !X || !B || n < 1 || n > h->n_max || n > 224 || nrhs < 1 || nrhs > h->NP_max || (la != 0 && la != 2 && la != 3)) return ORCVIO_ERR_INVALID;
    const int ncols = nrhs + (bx ? 1 : 0), nrows = n + tail;
    // B and bx share the right-hand-side scratch (NP_max x NP_max): B in its first rows, bx in its last row
    if (tail < 0 || nrows > h->NP_max - 1 || ncols > h->NP_max) return ORCVIO_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    const int NP = round_up(n, 16), ldz = h->NP_max;
    const size_t np2 = (size_t)h->NP_max * h->NP_max;
    const long ldb = product_strides ? (long)h->NP_max : (long)nrhs;
    HIPCHK(hipMemset(h->d_M, 0xff, sizeof(double) * (size_t)NP * NP));   // (NaN in the padding: the kernels must mask it)
    HIPCHK(hipMemcpy2D(h->d_M, sizeof(double) * NP, X, sizeof(double) * n, sizeof(double) * n, n, hipMemcpyHostToDevice));
    double* d_bx = h->d_U + (size_t)(h->NP_max - 1) * h->NP_max;
    {
        std::vector<double> stage(np2, __builtin_nan(""));
        for (int i = 0; i < nrows; ++i)
            for (int c = 0; c < nrhs; ++c) stage[(size_t)i * ldb + (product_strides ? nrhs - 1 - c : c)] = B[(size_t)i * nrhs + c];
        if (bx) std::memcpy(stage.data() + (size_t)(h->NP_max - 1) * h->NP_max, bx, sizeof(double) * n);
        HIPCHK(hipMemcpy(h->d_U, stage.data(), sizeof(double) * np2, hipMemcpyHostToDevice));
    }
    const double* dB = product_strides ? h->d_U + (nrhs - 1) : h->d_U;
    const long sBc = product_strides ? -1L : 1L;
    HIPCHK(hipMemset(h->d_Z, 0xff, sizeof(double) * np2));
    HIPCHK(hipMemset(h->d_RM, 0, sizeof(double) * np2));
    HIPCHK(hipMemset(h->d_info, 0, sizeof(int) * 16));
    unsigned long long* d_st = nullptr;
    if (stamps) { HIPCHK(hipMalloc(&d_st, sizeof(unsigned long long) * 512)); HIPCHK(hipMemset(d_st, 0, sizeof(unsigned long long) * 512)); }
    hipStream_t s = h->stream;
    auto once = [&](unsigned long long* st) -> int {
        HIPCHK(hipMemsetAsync(h->d_flag, 0, sizeof(int), s));
        HIPCHK(hipMemsetAsync(h->d_la_rdy, 0, 64, s));
        if (la) return launch_potrf_solve_la(h, s, la, h->d_M, NP, n, h->d_RM, NP, h->d_DinvM, h->d_info + 2, h->d_flag, h->d_la_rdy, h->d_info + 8,
                                             dB, ldb, sBc, nrhs, bx ? d_bx : nullptr, bx ? 1L : 0L, h->d_Z, ldz, tail, tail_scale, st);
        return launch_potrf_solve_slots(s, h->d_M, NP, n, h->d_RM, NP, h->d_DinvM, h->d_info + 2, h->d_flag, h->d_info + 8, dB, ldb, sBc, nrhs,
                                        bx ? d_bx : nullptr, bx ? 1L : 0L, h->d_Z, ldz, tail, tail_scale);
    };
    int rc = once(d_st);
    if (rc == ORCVIO_OK && reps > 0 && us_out) {
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        for (int r = 0; r < 3 && rc == ORCVIO_OK; ++r) rc = once(nullptr);
        HIPCHK(hipEventRecord(e0, s));
        for (int r = 0; r < reps && rc == ORCVIO_OK; ++r) rc = once(nullptr);
        HIPCHK(hipEventRecord(e1, s));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *us_out = 1e3 * ms / reps;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    if (rc == ORCVIO_OK) {
        HIPCHK(hipStreamSynchronize(s));
        std::vector<double> buf((size_t)NP * NP);
        HIPCHK(hipMemcpy(buf.data(), h->d_RM, sizeof(double) * buf.size(), hipMemcpyDeviceToHost));
        if (L_out)
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) L_out[(size_t)i * n + j] = buf[(size_t)j * NP + i];   // L = R^T
        if (Z_out || outside_out) {
            std::vector<double> zb(np2);
            HIPCHK(hipMemcpy(zb.data(), h->d_Z, sizeof(double) * np2, hipMemcpyDeviceToHost));
            if (Z_out)
                for (int i = 0; i <= nrows; ++i)
                    for (int c = 0; c <= ncols; ++c)
                        Z_out[(size_t)i * (ncols + 1) + c] = (i < h->NP_max && c < ldz) ? zb[(size_t)i * ldz + c] : __builtin_nan("");
            if (outside_out) {
                int outside = 0;
                for (int i = 0; i < h->NP_max; ++i)
                    for (int c = 0; c < ldz; ++c)
                        if (!(i < nrows && c < ncols) && zb[(size_t)i * ldz + c] == zb[(size_t)i * ldz + c]) ++outside;
                *outside_out = outside;
            }
        }
        if (info_out) {
            int inf[16];
            HIPCHK(hipMemcpy(inf, h->d_info, sizeof(inf), hipMemcpyDeviceToHost));
            info_out[0] = inf[2]; info_out[1] = inf[3]; info_out[2] = inf[8];
        }
        if (stamps) HIPCHK(hipMemcpy(stamps, d_st, sizeof(unsigned long long) * 512, hipMemcpyDeviceToHost));
    }
    if (d_st) (void)hipFree(d_st);
    HIPCHK(hipMemset(h->d_info, 0, sizeof(int) * 16));
    HIPCHK(hipMemset(h->d_flag, 0, sizeof(int)));
    HIPCHK(hipMemset(h->d_la_rdy, 0, 64));
    HIPCHK(hipMemset(h->d_RM, 0, sizeof(double) * np2));   // lower tiles: zero for any layout
    HIPCHK(hipMemset(h->d_U, 0, sizeof(double) * np2));    // (no NaN left behind in the handle's scratch)
    HIPCHK(hipMemset(h->d_Z, 0, sizeof(double) * np2));
    return rc;
}

// k_imu_phi_q alone, by events on the handle's stream: the host half once, the records copied once, one warm-up launch, then `reps`
// launches each between two events; ms_out [reps] (scripts/gpu_imu_propagate_timing.py takes the median).  The covariance is not touched.
int32_t orcvio_msckf_debug_imu_kernel_ms(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg, const orcvio_msckf_imu_state* state,
                                         const double* prev_meas, const double* samples, int32_t n_samples, double time_bound, int32_t reps,
                                         float* ms_out) {
    if (!h || !cfg || !state || !prev_meas || !samples || !ms_out || reps < 1 || cfg->leg_dim != 22) return ORCVIO_ERR_INVALID;
    ImuMeanState st;
    double prev[6];
    double* recs = h->imu_recs.data();
    ImuBatchInfo bi{};
    ImuFlags fl{};
    { const int rh = imu_host_half(cfg, state, prev_meas, samples, n_samples, time_bound, &st, prev, recs, &bi, &fl, "debug_imu_kernel_ms"); if (rh != ORCVIO_OK) return rh; }
    if (bi.n_propagated < 1) return ORCVIO_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    double* dPhi = h->d_covT + (size_t)46 * h->n_max;
    double* dQ = dPhi + 46 * 46;
    int rc = imu_enqueue(h, s, cfg, fl, recs, bi.n_propagated, dPhi, dQ);   // (records staged, warm-up)
    if (rc != ORCVIO_OK) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    ImuKernArgs a{};
    a.recs = h->d_imu; a.Phi = dPhi; a.Q = dQ; a.status = imu_status(h); a.S = bi.n_propagated; a.flags = fl;
    for (int i = 0; i < 3; ++i) a.grav[i] = cfg->gravity[i];
    for (int i = 0; i < 12; ++i) a.qc[i] = cfg->Q_c_diag[i];
    for (int r = 0; r < reps && he == hipSuccess; ++r) {   // (the first HIP error ends the loop; the events are destroyed on every path)
        he = hipEventRecord(e0, s);
        hipLaunchKernelGGL(k_imu_phi_q, dim3(1), dim3(64 * IMU_WAVES), imu_lds_bytes(a.S), s, a);
        if (he == hipSuccess) he = hipEventRecord(e1, s);
        if (he == hipSuccess) he = hipEventSynchronize(e1);
        if (he == hipSuccess) he = hipEventElapsedTime(&ms_out[r], e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (he != hipSuccess) { g_last_error = std::string("debug_imu_kernel_ms: ") + hipGetErrorString(he); return ORCVIO_ERR_HIP; }
    return ORCVIO_OK;
}

// k_imu_phi_q46 alone, in the same manner (scripts/gpu_imu_calib_timing.py).  The covariance is not touched.
int32_t orcvio_msckf_debug_imu_kernel46_ms(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg, const orcvio_msckf_imu_intrinsics* intr,
                                           const orcvio_msckf_imu_state* state, const double* prev_meas, const double* samples,
                                           int32_t n_samples, double time_bound, int32_t reps, float* ms_out) {
    if (!h || !cfg || !intr || !state || !prev_meas || !samples || !ms_out || reps < 1 || cfg->leg_dim != 46) return ORCVIO_ERR_INVALID;
    ImuIntrinsicMx mx;
    imu_intrinsic_mx(intr->x, &mx);
    ImuMeanState st;
    double prev[6];
    double* recs = h->imu_recs46.data();
    ImuBatchInfo bi{};
    ImuFlags fl{};
    { const int rh = imu_host_half46(cfg, mx, state, prev_meas, samples, n_samples, time_bound, &st, prev, recs, &bi, &fl, "debug_imu_kernel46_ms"); if (rh != ORCVIO_OK) return rh; }
    if (bi.n_propagated < 1) return ORCVIO_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    double* dPhi = imu_dphi(h);
    double* dQ = imu_dq(h);
    int rc = imu_enqueue46(h, s, cfg, fl, mx, recs, bi.n_propagated, dPhi, dQ);   // (records staged, warm-up)
    if (rc != ORCVIO_OK) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    const ImuKernArgs46 a = imu_args46(h, cfg, fl, mx, bi.n_propagated, dPhi, dQ);
    for (int r = 0; r < reps && he == hipSuccess; ++r) {
        he = hipEventRecord(e0, s);
        hipLaunchKernelGGL(k_imu_phi_q46, dim3(1), dim3(64 * IMU_WAVES), imu46_lds_bytes(), s, a);
        if (he == hipSuccess) he = hipEventRecord(e1, s);
        if (he == hipSuccess) he = hipEventSynchronize(e1);
        if (he == hipSuccess) he = hipEventElapsedTime(&ms_out[r], e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (he != hipSuccess) { g_last_error = std::string("debug_imu_kernel46_ms: ") + hipGetErrorString(he); return ORCVIO_ERR_HIP; }
    return ORCVIO_OK;
}

#endif  // ORCVIO_DEBUG_HOOKS
