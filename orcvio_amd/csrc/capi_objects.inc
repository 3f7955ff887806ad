// capi_objects.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// the object update: staging, compression pipeline, finish / download, ObjectLM messages, row evaluation.

// ---- per-stage device times (HIP events between the stages of an update; off unless switched on) -------------------
static void prof_begin(orcvio_msckf_handle* h, hipStream_t s) {
    if (!h->prof_on) return;
    h->prof_n = 0;
    h->prof_names.clear();
    if (h->prof_ev.empty()) { h->prof_ev.resize(24); for (auto& e : h->prof_ev) (void)hipEventCreate(&e); }
    (void)hipEventRecord(h->prof_ev[0], s);
    h->prof_n = 1;
}
static void prof_mark(orcvio_msckf_handle* h, hipStream_t s, const char* name) {
    if (!h->prof_on || h->prof_n == 0 || h->prof_n >= (int)h->prof_ev.size()) return;
    (void)hipEventRecord(h->prof_ev[h->prof_n++], s);
    h->prof_names.push_back(name);
}

// ---- object update: device scratch and host staging (the plan records: msckf_capi.hip; the staging itself: host/object_stage.hpp) ----
static int obj_stage_reserve(orcvio_msckf_handle* h, size_t bytes) {
    if (bytes <= h->obj_stage_cap) return ORCVIO_OK;
    HIPCHK(hipDeviceSynchronize());
    if (h->h_obj_stage) (void)hipHostFree(h->h_obj_stage);
    if (h->d_obj_in) (void)hipFree(h->d_obj_in);
    h->h_obj_stage = nullptr; h->d_obj_in = nullptr; h->obj_stage_cap = 0;
    const size_t cap = (bytes * 3 / 2 + 4095) & ~(size_t)4095;
    HIPCHK(hipHostMalloc(&h->h_obj_stage, cap, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_obj_stage_dev), h->h_obj_stage, 0));
    HIPCHK(hipMalloc(&h->d_obj_in, cap));
    h->obj_stage_cap = cap;
    return ORCVIO_OK;
}
// device scratch of the compression: row arrays [Hx6 | HfR (ld ldf) | res | row_clone | row_cols] and [Cd | Sg | Gff]
static int objects_scratch(orcvio_msckf_handle* h, ObjPlan* pl) {
    const int NAP = h->NAP, N = h->N;
    pl->NOP = round_up(pl->no_max, 16);
    pl->ldf = round_up(pl->no_max + 1, 16);
    const size_t rows = (size_t)pl->rows_tot, nobj = (size_t)pl->nobj;
    int rc;
    if ((rc = grow(&h->d_obj_i, &h->cap_obj_i, 2 * rows + 16)) != ORCVIO_OK) return rc;
    if ((rc = grow(&h->d_objH, &h->cap_objH, rows * (6 + pl->ldf + 1) + 16)) != ORCVIO_OK) return rc;
    const size_t nCd = nobj * pl->NOP * NAP, nSg = nobj * N * 64, nHr = nobj * N * pl->NOP, nGff = nobj * pl->ldf * pl->ldf;
    const size_t nRa = nobj * (size_t)arrow_stride(pl->Kmax > 0 ? pl->Kmax : 1);
    if ((rc = grow(&h->d_Gobj, &h->cap_Gobj, nCd + nSg + nHr + nGff + nRa + rows * 9 + nobj * (pl->NOP + 1) + rows * OBJ_REFINE_ROW_DOUBLES)) != ORCVIO_OK) return rc;
    if ((rc = grow(&h->d_RF, &h->cap_RF, nobj * ((size_t)pl->NOP * pl->NOP + 7 * 256))) != ORCVIO_OK) return rc;
    if ((rc = grow(&h->d_Yobj, &h->cap_Yobj, nobj * pl->NOP * NAP)) != ORCVIO_OK) return rc;
    pl->d_clone = h->d_obj_i;
    pl->d_cols = h->d_obj_i + rows;
    pl->d_hx = h->d_objH;
    pl->d_hf = pl->d_hx + rows * 6;
    pl->d_res = pl->d_hf + rows * pl->ldf;
    pl->d_Cd = h->d_Gobj;
    pl->d_Sg = pl->d_Cd + nCd;
    pl->d_Hr = pl->d_Sg + nSg;
    pl->d_Gff = pl->d_Hr + nHr;
    pl->d_Rarrow = pl->d_Gff + nGff;
    pl->d_Bred = pl->d_Rarrow + nRa;
    pl->d_Hfr = pl->d_Bred + rows * 9;
    pl->d_Qt = pl->d_Hfr + nobj * (pl->NOP + 1);
    return ORCVIO_OK;
}

// From the compact rows in device memory to this rank's block in dst (P already in d_P).  The prior's Cholesky factor is
// forked to the side stream (joined by objects_finish).
static int objects_pipeline(orcvio_msckf_handle* h, hipStream_t s, double* dst, const ObjPlan& pl, bool zeroed = false, bool forked = false) {
    // zeroed: k_object_rows_batch has cleared Cd / Sg / Hr and the pivot counters;  forked: the caller has forked the Cholesky of
    // the prior already (right behind the copy of P, before it staged the tracks)
    const int NA = h->NA, NAP = h->NAP, N = h->N, nobj = pl.nobj, NOP = pl.NOP, ldf = pl.ldf, no_max = pl.no_max;
    double* d_RF = h->d_RF;
    double* d_DinvF = h->d_RF + (size_t)nobj * NOP * NOP;
    // zero: C (clones an object does not see) and the clone tiles; for the Gram route also Y (padded rows) and R_F
    // (strictly-lower tiles) -- the arrow route writes every entry of Y it reads
    if (!pl.arrow) {
        HIPCHK(hipMemsetAsync(h->d_Yobj, 0, sizeof(double) * (size_t)nobj * NOP * NAP, s));
        HIPCHK(hipMemsetAsync(d_RF, 0, sizeof(double) * (size_t)nobj * NOP * NOP, s));
    }
    if (!zeroed) HIPCHK(hipMemsetAsync(pl.d_Cd, 0, sizeof(double) * ((size_t)nobj * NOP * NAP + (size_t)nobj * N * 64 + (size_t)nobj * N * NOP), s));   // Cd, Sg, Hr are adjacent
    int rc = forked ? ORCVIO_OK : launch_prior_fork(h, s);   // Cholesky of P on the side stream
    if (rc != ORCVIO_OK) return rc;
    prof_mark(h, s, "rows+copies");
    {   // cross products (they also give Hf^T r and |r|^2), the keypoint blocks of the structured QR (arrow route) or the compact Grams
        // [Hf | r]^T [Hf | r] (Gram route, which needs F = Hf^T Hf): one launch
        const int nbf = ldf / 16, gram_tiles = pl.arrow ? 0 : nbf * (nbf + 1) / 2, kp_blocks = pl.arrow ? (pl.Kmax + 1 + 7) / 8 : 0;
        const int blocks = (pl.ngroups + 7) / 8 + gram_tiles * nobj + kp_blocks * nobj;
        hipLaunchKernelGGL(k_obj_front, dim3(blocks), dim3(512), 0, s, pl.d_groups, pl.ngroups, pl.d_ridx, pl.d_hx, pl.d_hf, ldf, no_max,
                           h->flags.leg_dim - 15, NAP, NOP, N, pl.d_Cd, pl.d_Sg, pl.d_Hr, pl.d_rowptr, pl.d_Gff, nobj, gram_tiles, pl.d_arrow,
                           pl.d_kp_range, pl.d_kp_rows, pl.Kmax, pl.d_Rarrow, pl.d_Bred, kp_blocks);
    }
    prof_mark(h, s, "k_obj_front");
    // ill-conditioned Hf (|R|_F |R^-1|_F above 3e6; every real car: the gauge of the keypoint rows) takes Y from an explicit basis of
    // range(Hf) instead of the semi-normal equations (obj_refine_body): inside the border launch, rows staged in LDS when they fit
    RefineArgs ra{};
    size_t refine_lds = 0;
    if (pl.arrow && h->obj_refine_mode != 0) {
        const size_t base = sizeof(double) * (2 * (size_t)arrow_stride(pl.Kmax > 0 ? pl.Kmax : 1) + NOP + (size_t)N * (pl.Kmax > 0 ? pl.Kmax : 1));   // factor, T, Q~^T r, (clone, keypoint) table
        // dynamic LDS a workgroup of the border launch may take: the CU's 160 KB minus the kernel's own static arrays (asked of the runtime
        // once; the three instantiations and the stand-alone kernel are opted in to that much)
        size_t& budget = h->obj_lds_budget;   // per handle (= per device: hipFuncSetAttribute applies to the current device only; ADVICE r4)
        if (budget == 0) {
            size_t stat = 0;
            const void* fns[4] = {(const void*)k_obj_border_solve_assemble<2>, (const void*)k_obj_border_solve_assemble<4>,
                                  (const void*)k_obj_border_solve_assemble<8>, (const void*)k_obj_refine};
            for (const void* f : fns) {
                hipFuncAttributes at;
                HIPCHK(hipFuncGetAttributes(&at, f));
                if (at.sharedSizeBytes > stat) stat = at.sharedSizeBytes;
            }
            hipDeviceProp_t prop;
            HIPCHK(hipGetDeviceProperties(&prop, h->device));
            const size_t cu_lds = prop.maxSharedMemoryPerMultiProcessor > 0 ? (size_t)prop.maxSharedMemoryPerMultiProcessor : (size_t)160 * 1024;
            const size_t b = cu_lds - stat - 512;
            for (const void* f : fns) HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b));
            budget = b;
        }
        const size_t per_row = sizeof(double) * OBJ_REFINE_ROW_DOUBLES;
        int lds_rows = budget > base ? (int)((budget - base) / per_row) : 0;   // (what does not fit is staged in global scratch instead)
        if (lds_rows > pl.rows_max) lds_rows = pl.rows_max;
        ra.kp_range = pl.d_kp_range; ra.kp_rows = pl.d_kp_rows; ra.groups = pl.d_groups; ra.ngroups = pl.ngroups; ra.ridx = pl.d_ridx;
        ra.Hx6 = pl.d_hx; ra.HfR = pl.d_hf; ra.ldf = ldf; ra.no_max = no_max; ra.scratch = pl.d_Qt; ra.lds_rows = lds_rows;
        ra.mode = h->obj_refine_mode; ra.refined = h->d_info + 5; ra.cb0 = h->flags.leg_dim - 15; ra.N = N;
        refine_lds = base + per_row * (size_t)lds_rows;
        static const bool want_stamps = dbg_getenv("ORCVIO_REFINE_STAMPS") != nullptr;   // diagnostics
        if (want_stamps) {
            static unsigned long long* d_st = nullptr;
            if (!d_st) { HIPCHK(hipMalloc(&d_st, 64)); HIPCHK(hipMemset(d_st, 0, 64)); }
            ra.stamps = d_st;
        }
    }
    const int solve_xblocks = (NAP + 255) / 256, nb_solve = pl.arrow ? solve_xblocks * nobj : 0;
    const bool fuse_border = pl.arrow && solve_xblocks == 1;   // border QR + Y + sum B in one launch (one solve workgroup per object)
    if (pl.arrow && !fuse_border) {
        // R of Hf by structured Householder QR (cond(Hf), not its square: msckf_kernels.hpp); the keypoint blocks are done, the border:
        if (!zeroed) HIPCHK(hipMemsetAsync(h->d_info + 4, 0, sizeof(int) * 2, s));
#define LAUNCH_BORDER(RPT) hipLaunchKernelGGL(k_obj_border_qr<RPT>, dim3(nobj), dim3(256), 0, s, pl.d_arrow, (const double*)pl.d_Bred, pl.Kmax, \
                                              pl.d_Rarrow, (const double*)pl.d_Hr, (const double*)pl.d_Sg, N, NOP, pl.d_Hfr)
        if (pl.rows_max <= 512) LAUNCH_BORDER(2);
        else if (pl.rows_max <= 1024) LAUNCH_BORDER(4);
        else LAUNCH_BORDER(8);
#undef LAUNCH_BORDER
        prof_mark(h, s, "k_obj_border_qr(Hf)");
    } else if (!pl.arrow) {
    // (Hf without the arrow structure of ObjectLM's state: the Gram route.)  F_o = Hf^T Hf (lower tiles of Gff) -> R_F ;
    // Y_o = L_F^-1 C_o, C_o = [Cd_o | Hf^T r]
    {
        const int nbf = NOP / 16, need = potrf_slots_needed(nbf);
        if (!zeroed) HIPCHK(hipMemsetAsync(h->d_info + 4, 0, sizeof(int) * 2, s));   // the batched factorisation ADDS its pivot counters
        const double tolF = (double)no_max * 2.220446049250313e-16;
        if (need <= 4)
            hipLaunchKernelGGL(k_potrf_reg<4>, dim3(nobj), dim3(512), 0, s, pl.d_Gff, ldf, no_max, tolF, d_RF, NOP, d_DinvF, h->d_info + 4,
                               (unsigned long long*)nullptr, (size_t)ldf * ldf, (size_t)NOP * NOP, (size_t)7 * 256, 1);
        else
            hipLaunchKernelGGL(k_potrf_reg<8>, dim3(nobj), dim3(512), 0, s, pl.d_Gff, ldf, no_max, tolF, d_RF, NOP, d_DinvF, h->d_info + 4,
                               (unsigned long long*)nullptr, (size_t)ldf * ldf, (size_t)NOP * NOP, (size_t)7 * 256, 1);
        prof_mark(h, s, "k_potrf_reg(F) batched");
        const int nwave = (NA + 1 + 15) / 16;
        hipLaunchKernelGGL(k_trsm_lds, dim3((nwave + 3) / 4, nobj), dim3(256), 0, s, d_RF, NOP, d_DinvF, no_max,
                           pl.d_Cd, (long)NAP, 1L, NA, pl.d_Gff + (size_t)no_max * ldf, 1L, h->d_Yobj, NAP,
                           (size_t)NOP * NOP, (size_t)7 * 256, (size_t)NOP * NAP, (size_t)NOP * NAP, (size_t)ldf * ldf);
        prof_mark(h, s, "k_trsm_lds(Y) batched");
    }
    }
    // Y_o = R^-T C_o (arrow route) and sum_o B_o in one launch; then A' = sum_o B_o - Y^T Y (Y = all Y_o stacked; padded rows are zero)
    if (fuse_border) {
        if (!zeroed) HIPCHK(hipMemsetAsync(h->d_info + 4, 0, sizeof(int) * 2, s));
        const dim3 grid(nobj + (NAP * NAP + 255) / 256);
        const size_t lds = refine_lds > 0 ? refine_lds : sizeof(double) * arrow_stride(pl.Kmax > 0 ? pl.Kmax : 1);
#define LAUNCH_BSA(RPT) hipLaunchKernelGGL(k_obj_border_solve_assemble<RPT>, grid, dim3(256), lds, s, pl.d_arrow, (const double*)pl.d_Bred, pl.Kmax, \
                                           pl.d_Rarrow, (const double*)pl.d_Hr, (const double*)pl.d_Sg, N, NOP, pl.d_Hfr, (const double*)pl.d_Cd, NAP, NA, \
                                           h->d_Yobj, h->d_info + 4, nobj, h->flags.leg_dim - 15, h->d_Ab, ra)
        if (pl.rows_max <= 512) LAUNCH_BSA(2);
        else if (pl.rows_max <= 1024) LAUNCH_BSA(4);
        else LAUNCH_BSA(8);
#undef LAUNCH_BSA
        prof_mark(h, s, "k_obj_border_solve_assemble");
        if (ra.stamps) {
            unsigned long long st[8];
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(hipMemcpy(st, ra.stamps, 64, hipMemcpyDeviceToHost));
            fprintf(stderr, "refine stamps (us after the kernel's first instruction): qr done %.2f | start %.2f P %.2f A %.2f B1 %.2f B2 %.2f C %.2f\n", (st[0] - st[7]) * 0.01,
                    (st[1] - st[7]) * 0.01, (st[2] - st[7]) * 0.01, (st[3] - st[7]) * 0.01, (st[4] - st[7]) * 0.01, (st[5] - st[7]) * 0.01, (st[6] - st[7]) * 0.01);
        }
    } else
    {   // |r|^2 per object: arrow route Hfr[o][NOP] (k_obj_border_qr), Gram route the corner of the compact Gram
        const double* rr = pl.arrow ? pl.d_Hfr + NOP : pl.d_Gff + (size_t)no_max * ldf + no_max;
        const size_t rr_stride = pl.arrow ? (size_t)NOP + 1 : (size_t)ldf * ldf;
        hipLaunchKernelGGL(k_obj_solve_assemble, dim3(nb_solve + (NAP * NAP + 255) / 256), dim3(256), sizeof(double) * arrow_stride(pl.Kmax > 0 ? pl.Kmax : 1), s,
                           nb_solve, solve_xblocks, pl.d_arrow, pl.d_Rarrow, pl.Kmax, pl.d_Cd, NOP, NAP, NA, (const double*)pl.d_Hfr, h->d_Yobj, h->d_info + 4,
                           pl.d_Sg, nobj, N, h->flags.leg_dim - 15, rr, rr_stride, h->d_Ab);
    }
    if (pl.arrow && !fuse_border && h->obj_refine_mode != 0) {
        // (wide windows: border QR and substitution are separate launches, the explicit-basis projection of ill-conditioned objects a third)
        hipLaunchKernelGGL(k_obj_refine, dim3(nobj), dim3(256), refine_lds, s, pl.d_arrow, pl.Kmax, (const double*)pl.d_Rarrow, ra, h->d_Yobj, NOP, NAP, NA);
        prof_mark(h, s, "k_obj_refine");
    }
    hipLaunchKernelGGL(k_gemm, dim3((NAP / 16) * (NAP / 16)), dim3(256), 0, s, h->d_Yobj, 1L, (long)NAP, h->d_Yobj, (long)NAP, 1L,
                       NAP, NAP, nobj * NOP, -1.0, 0.0, 0, dst, (long)NAP, 1L, h->d_Ab);
    HIPCHK(hipGetLastError());
    prof_mark(h, s, fuse_border ? "k_gemm(A')" : "k_obj_assemble_B+k_gemm(A')");
    return ORCVIO_OK;
}

// Prior of an object update: the caller's P staged through pinned memory and pulled from there by one launch (launch_ingest_P: of an
// even n only the upper tiles are staged and travel; the caller's buffer is free when the call returns), or the resident covariance in
// place (no copy at all).
static int objects_prior(orcvio_msckf_handle* h, hipStream_t s, const double* P, const char* who) {
    const int n = h->n;
    if (!P && h->res_n != n) { g_last_error = std::string(who) + ": P == NULL but the resident covariance does not match the window"; return ORCVIO_ERR_INVALID; }
    if (!h->frame_mode) {   // (orcvio_msckf_io_update_frame: the feature update of the same call is in flight on h->stream and must stay so;
                            //  its prior is resident, nothing of the pinned arena is written here)
        { const int rw = arena_wait_free(h); if (rw != ORCVIO_OK) return rw; }   // the pinned staging of the previous call is free again
        HIPCHK(hipStreamSynchronize(h->stream));   // (and the outputs arena, which this update lays out anew, is not being written)
        if (s != h->stream) HIPCHK(hipStreamSynchronize(s));
        if (h->dl_pending) { HIPCHK(hipStreamSynchronize(h->dl_stream)); h->dl_pending = false; }
    } else if (P) { g_last_error = std::string(who) + ": the frame call takes the resident covariance as the prior"; return ORCVIO_ERR_INVALID; }
    layout_inputs(h, h->N, 0, 0, false, P != nullptr, n);
    layout_outputs(h, n, 1);
    if (P) {
        stage_prior(h, P, n, true);   // (what the pull below fetches: the upper tile-trapezoid when n is even)
        const int ri = launch_ingest_P(h, s, h->io_P, n);
        if (ri != ORCVIO_OK) return ri;
        { const int rm = arena_mark_read(h, s); if (rm != ORCVIO_OK) return rm; }
    }
    return ORCVIO_OK;
}
// window-dependent sizes of an object update (no tracks)
static int objects_problem(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int N, const double* P, const char* who) {
    if (flags->leg_dim != 22 && flags->leg_dim != 46) { g_last_error = std::string(who) + ": leg_dim must be 22 or 46"; return ORCVIO_ERR_INVALID; }
    if (N < 1 || N > h->maxN) { g_last_error = std::string(who) + ": window exceeds capacity"; return ORCVIO_ERR_CAPACITY; }
    if (h->io_submitted) { g_last_error = std::string(who) + ": an update submitted with orcvio_msckf_io_submit has not been collected"; return ORCVIO_ERR_INVALID; }
    h->flags = *flags;
    h->io_open = false;   // (the object update lays the arenas out for itself: a feature update needs a new io_begin)
    h->N = N; h->F = 0; h->nobs = 0;
    h->n = flags->leg_dim + 6 * N + h->n_extra;   // (n_extra: states behind the clones that no row of this update touches)
    h->NA = h->ekf_mode ? h->n - 15 : flags->leg_dim + 6 * N - 15;   // (EKF-SLAM rows reach into the extra states)
    h->ekf_F = 0; h->dense_rows = 0; h->new_F = 0;
    if (h->n > h->n_max) { g_last_error = "window + extra states exceed the handle's capacity"; return ORCVIO_ERR_CAPACITY; }
    h->NAP = round_up(h->NA + 1, 16);
    select_prior_factor(h, P != nullptr);
    h->NP = round_up(h->n > h->kf ? h->n : h->kf, 16);
    h->ldz = round_up(h->n + 1, 16);
    h->reg_path = (h->NP / 16) <= 14;
    select_tail(h);
    { const int rcl = factor_layout_clean(h); if (rcl != ORCVIO_OK) return rcl; }
    h->m_tot = 0; h->Mmax = 2; h->chunks = 1; h->rows_per_chunk = 8;
    h->h_row_ptr.assign(1, 0);
    return ORCVIO_OK;
}
// Scan of an update's object tracks into the handle's lists (objects_tracks_scan, host/object_stage.hpp); voids what was staged ahead.
static int objects_scan(orcvio_msckf_handle* h, int N, const orcvio_object_track* tracks, int n_tracks, ObjScan& sc) {
    h->prestage.valid = false;   // (the lists and the staging arena of a pre-staged frame are about to be overwritten)
    const char* why = "";
    const int rc = objects_tracks_scan(N, h->ref_stack_hf, tracks, n_tracks, h->obj_use, h->obj_nv, sc, &why);
    if (rc != ORCVIO_OK) g_last_error = why;
    return rc;
}
static ObjPlan plan_of(const ObjScan& sc) { ObjPlan pl; pl.nobj = sc.nobj; pl.rows_tot = sc.rows_tot; pl.no_max = sc.no_max; return pl; }
// device views of the integer arena
static void plan_views(ObjPlan& pl, const ObjIntViews& v) {
    pl.d_ridx = v.ridx; pl.d_rowptr = v.rowptr; pl.d_groups = v.groups;
    pl.d_arrow = v.arrows; pl.d_kp_range = reinterpret_cast<int2*>(v.kp_range); pl.d_kp_rows = v.kp_rows;
}

// The shared head of the two objects_local* entry points, behind the scan: the prior, the handle's record of the update and -- nothing
// usable on this rank (sc.nobj == 0) -- the zero block, behind which the caller returns.
static int objects_begin(orcvio_msckf_handle* h, hipStream_t s, const double* P, const char* who, const ObjScan& sc, double* dst) {
    h->last_stream = s;
    prof_begin(h, s);
    { const int rp = objects_prior(h, s, P, who); if (rp != ORCVIO_OK) return rp; }
    h->uploaded = true;
    h->objects_mode = true;
    h->last_update_thin = false;
    h->obj_dof = sc.dof; h->obj_rows = sc.rows_tot; h->obj_count = sc.nobj;
    if (!h->d_obj_accept) { HIPCHK(hipMalloc(&h->d_obj_accept, sizeof(int) * 4)); HIPCHK(hipMalloc(&h->d_obj_gamma, sizeof(double) * 4)); }
    if (sc.nobj > 0) return ORCVIO_OK;
    HIPCHK(hipMemsetAsync(dst, 0, sizeof(double) * (size_t)h->NAP * h->NAP, s));   // a zero block
    return launch_prior_fork(h, s);
}

// Local part of an object update: this rank's objects -> its compressed block [A' b'; b'^T c'] (NAP x NAP) in d_dst
// (the handle's own block if NULL), Cholesky of P forked on the side stream.
int32_t orcvio_msckf_objects_local(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int32_t n_clones,
                                   const orcvio_msckf_object_rows* objs, int32_t n_objects, const double* P, double* d_dst,
                                   int32_t* dof_out, void* stream) {
    if (!h || !flags || n_objects < 0 || (n_objects > 0 && !objs)) { g_last_error = "objects_local: null argument"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    { const int rp = objects_problem(h, flags, n_clones, P, "objects_local"); if (rp != ORCVIO_OK) return rp; }
    const int N = n_clones;
    std::vector<int> use;   // usable objects
    ObjScan sc;
    { const char* why = ""; const int rs = objects_rows_scan(N, h->ref_stack_hf, objs, n_objects, use, sc, &why); if (rs != ORCVIO_OK) { g_last_error = why; return rs; } }
    hipStream_t s = pick_stream(h, stream);
    double* dst = d_dst ? d_dst : h->d_Ab;
    if (dof_out) *dof_out = sc.dof;
    int rc = objects_begin(h, s, P, "objects_local", sc, dst);
    if (rc != ORCVIO_OK || sc.nobj == 0) return rc;
    ObjPlan pl = plan_of(sc);
    if ((rc = objects_scratch(h, &pl)) != ORCVIO_OK) return rc;
    // staging arena: [Hx6 rows x 6 | HfR rows x ldf] doubles, then the ints (ObjIntLayout)
    const size_t rows = (size_t)pl.rows_tot, ldf = (size_t)pl.ldf;
    size_t sumK = 0;
    for (int o : use) sumK += (size_t)((objs[o].n_obj_cols - 9) / 3 > 0 ? (objs[o].n_obj_cols - 9) / 3 : 0);
    const size_t nd = rows * 6 + rows * ldf;
    const ObjIntLayout lay = obj_int_layout(rows, pl.nobj, sumK, N, 0);
    if ((rc = obj_stage_reserve(h, nd * 8 + lay.ni * 4)) != ORCVIO_OK) return rc;
    double* hx = reinterpret_cast<double*>(h->h_obj_stage);
    double* hf = hx + rows * 6;
    const ObjIntViews hv = lay.views(reinterpret_cast<int*>(h->h_obj_stage + nd * 8));
    std::memset(hf, 0, sizeof(double) * rows * ldf);
    std::vector<int>& rowkp = h->obj_fnr;   // (scratch) keypoint block of every row, -1: border only
    rowkp.assign(rows, -1);
    std::vector<int> Ks(pl.nobj, 0);
    bool structured = true;
    int r0 = 0, ng = 0;
    hv.rowptr[0] = 0;
    for (size_t ui = 0; ui < use.size(); ++ui) {
        const orcvio_msckf_object_rows& ob = objs[use[ui]];
        Ks[ui] = obj_pack_rows(ob, r0, ldf, pl.no_max, hx, hf, rowkp.data(), structured);
        obj_group_rows(ob.row_clone, ob.n_rows, N, r0, (int)ui, hv.ridx, hv.groups, &ng);
        r0 += ob.n_rows;
        hv.rowptr[ui + 1] = r0;
    }
    if (h->ref_stack_hf && pl.nobj > 1) {
        merge_objects_ref_stack(N, pl.rows_tot, hv.ridx, hv.rowptr, hv.groups, &ng);
        pl.nobj = 1; h->obj_count = 1; structured = false;
        rc = objects_scratch(h, &pl);   // the scratch of ONE block: Cd | Sg | Hr adjacent again (the row arrays depend on the row count only)
        if (rc != ORCVIO_OK) return rc;
    }
    pl.ngroups = ng;
    pl.arrow = structured && h->arrow_opt &&
               build_arrow(rowkp.data(), hv.rowptr, Ks.data(), pl.nobj, hv.arrows, hv.kp_range, hv.kp_rows, &pl.Kmax, &pl.rows_max);
    if (pl.arrow) { rc = objects_scratch(h, &pl); if (rc != ORCVIO_OK) return rc; }   // (room for the arrow factors)
    // device views of the arena
    double* dd = reinterpret_cast<double*>(h->d_obj_in);
    pl.d_hx = dd; pl.d_hf = dd + rows * 6;
    plan_views(pl, lay.views(reinterpret_cast<int*>(h->d_obj_in + nd * 8)));
    { const int ri = launch_ingest(h, s, h->h_obj_stage_dev, h->d_obj_in, lay.ingest_bytes(nd, ng)); if (ri != ORCVIO_OK) return ri; }
    return objects_pipeline(h, s, dst, pl);
}

// ---- object tracks, one-launch compression (object_fused.hpp) ------------------------------------------------------------------
// Rows an object of K keypoints may have so that its workgroup's LDS staging fits (0: the kernel cannot run here).
static int obj_fused_lds_rows(orcvio_msckf_handle* h, int Kmax, int NOP, int N) {
    if (h->obj_fused_budget == 0) {
        hipFuncAttributes at;
        if (hipFuncGetAttributes(&at, (const void*)k_obj_fused) != hipSuccess) { (void)hipGetLastError(); return 0; }
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
        const size_t cu_lds = prop.maxSharedMemoryPerMultiProcessor > 0 ? (size_t)prop.maxSharedMemoryPerMultiProcessor : (size_t)160 * 1024;
        if (cu_lds < at.sharedSizeBytes + 4096) return 0;
        const size_t b = cu_lds - at.sharedSizeBytes - 512;
        if (hipFuncSetAttribute((const void*)k_obj_fused, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b) != hipSuccess) { (void)hipGetLastError(); return 0; }
        h->obj_fused_budget = b;
    }
    const size_t base = sizeof(double) * obj_fused_lds_doubles(Kmax, NOP, N, 0);
    if (h->obj_fused_budget <= base) return 0;
    return (int)((h->obj_fused_budget - base) / (sizeof(double) * OBJ_REFINE_ROW_DOUBLES));
}
// Can every usable track of this update take the one-launch compression?  (In-window frames on distinct clones, at most
// OBJ_FUSED_MAXF of them, at most 8 * OBJ_FUSED_KPW keypoints, rows within the LDS staging.)
static bool obj_fused_eligible(orcvio_msckf_handle* h, const orcvio_object_track* tracks, int N, int no_max) {
    const std::vector<ObjUse>& use = h->obj_use;
    if (!h->obj_fused_opt || !h->arrow_opt || h->ref_stack_hf || h->obj_refine_mode == 0 || use.empty()) return false;
    int Kmax = 0;
    for (const ObjUse& u : use) Kmax = std::max(Kmax, tracks[u.t].n_keypoints);
    if (Kmax > OBJ_FUSED_NW * OBJ_FUSED_KPW) return false;
    const int lds_rows = obj_fused_lds_rows(h, Kmax, round_up(no_max, 16), N);
    for (const ObjUse& u : use)
        if (u.rows > lds_rows || u.rows > 65535 || !u.distinct || u.fin > OBJ_FUSED_MAXF) return false;   // (two frames on one clone: the general pipeline)
    return true;
}

// Staging and launches of the one-launch compression: [track data | kernel arguments] doubles, [frame_clone, frame_row0 per track |
// arrows] ints -> k_ingest (which also clears the pivot counters and the shard status words) -> k_obj_fused -> k_gemm_objA.
// (N, NA, NAP, cb0: the window of the object update, passed in -- the frame call launches this beside a feature update whose own
//  problem still stands in the handle's fields)
// In two parts: the host's staging (objects_fused_pack: the pinned arena, the device scratch, the plan) and the launches
// (objects_fused_launch) -- orcvio_msckf_io_stage_object_tracks runs the first ahead of the frame call.
static int objects_fused_pack(orcvio_msckf_handle* h, const orcvio_object_eval_flags* fl, const orcvio_object_track* tracks, const ObjScan& sc,
                              ObjPlan& pl, const int N, const int NAP, ObjFusedStage& st) {
    const std::vector<ObjUse>& use = h->obj_use;
    const size_t arg_dbl = OBJ_ARG_DOUBLES, args_off = sc.nd, nd = sc.nd + arg_dbl * use.size();
    const size_t o_arrow = sc.ni, ni_tot = o_arrow + (size_t)4 * use.size();
    int rc = obj_stage_reserve(h, nd * 8 + ni_tot * 4);
    if (rc != ORCVIO_OK) return rc;
    pl = plan_of(sc);
    pl.NOP = round_up(pl.no_max, 16);
    pl.ldf = round_up(pl.no_max + 1, 16);
    {   // device scratch: Y, the clone tiles, |r|^2
        const size_t nobj = use.size();
        if ((rc = grow(&h->d_Yobj, &h->cap_Yobj, nobj * pl.NOP * NAP)) != ORCVIO_OK) return rc;
        if ((rc = grow(&h->d_Gobj, &h->cap_Gobj, nobj * (size_t)N * 64 + nobj + 16)) != ORCVIO_OK) return rc;
        pl.d_Sg = h->d_Gobj;
        pl.d_Hfr = h->d_Gobj + nobj * (size_t)N * 64;
    }
    double* hd = reinterpret_cast<double*>(h->h_obj_stage);
    int* hi = reinterpret_cast<int*>(h->h_obj_stage + nd * 8);
    double* dd = reinterpret_cast<double*>(h->d_obj_in);
    int* di = reinterpret_cast<int*>(h->d_obj_in + nd * 8);
    ObjArrow* arrows = reinterpret_cast<ObjArrow*>(hi + o_arrow);
    int Kmax = 0, rows_max = 0;
    for (size_t ui = 0; ui < use.size(); ++ui) {
        const ObjUse& u = use[ui];
        const orcvio_object_track& ob = tracks[u.t];
        const int rows = obj_pack_track(ob, u, h->obj_nv.data() + u.off_nv, fl, pl.ldf, pl.no_max, ObjRowArrays{}, hd, hi, dd, di,
                                        reinterpret_cast<ObjEvalArgs*>(hd + args_off + arg_dbl * ui));
        arrows[ui] = ObjArrow{u.row0, rows, ob.n_keypoints, 0};
        if (ob.n_keypoints > Kmax) Kmax = ob.n_keypoints;
        if (rows > rows_max) rows_max = rows;
    }
    pl.arrow = true; pl.Kmax = Kmax; pl.rows_max = rows_max; pl.ngroups = 0;
    st.nd_tot = nd; st.ni_tot = ni_tot; st.args_off = args_off; st.o_arrow = o_arrow; st.Kmax = Kmax; st.rows_max = rows_max;
    return ORCVIO_OK;
}
static int objects_fused_launch(orcvio_msckf_handle* h, hipStream_t s, double* dst, const ObjPlan& pl, const ObjFusedStage& st, const int nobj,
                                const int N, const int NA, const int NAP, const int cb0, const bool signal_done) {
    const size_t nd = st.nd_tot, ni_tot = st.ni_tot, args_off = st.args_off, o_arrow = st.o_arrow;
    const int Kmax = st.Kmax, rows_max = st.rows_max;
    double* dd = reinterpret_cast<double*>(h->d_obj_in);
    int* di = reinterpret_cast<int*>(h->d_obj_in + nd * 8);
    // info[4], [5] (dropped pivots, objects through the flagged branch) and info[9..12] (shard status words): cleared by the ingest launch
    { const int ri = launch_ingest(h, s, h->h_obj_stage_dev, h->d_obj_in, nd * 8 + ni_tot * 4, h->d_info + 4, 0x1E3u); if (ri != ORCVIO_OK) return ri; }
    h->obj_status_cleared = true;
    prof_mark(h, s, "staging + k_ingest");
    ObjFusedArgs fa{};
    fa.args = reinterpret_cast<const ObjEvalArgs*>(dd + args_off);
    fa.objs = reinterpret_cast<const ObjArrow*>(di + o_arrow);
    fa.nobj = nobj; fa.N = N; fa.cb0 = cb0; fa.NA = NA; fa.NAP = NAP; fa.NOP = pl.NOP; fa.Kmax = Kmax;
    fa.Y = h->d_Yobj; fa.Sg = pl.d_Sg; fa.rr = pl.d_Hfr; fa.rr_stride = 1; fa.info = h->d_info + 4; fa.mode = h->obj_refine_mode;
    static const bool want_stamps = dbg_getenv("ORCVIO_FUSED_STAMPS") != nullptr;   // diagnostics
    static unsigned long long* d_st = nullptr;
    if (want_stamps) {
        if (!d_st) { HIPCHK(hipMalloc(&d_st, 128)); HIPCHK(hipMemset(d_st, 0, 128)); }
        fa.stamps = d_st;
    }
    static const double tol_rel = [] { const char* e = dbg_getenv("ORCVIO_FUSED_TOL"); const double v = e ? atof(e) : 0.0; return v > 0.0 ? v : 1e-10; }();
    fa.tol_rel = tol_rel;
    static const bool want_dbg = dbg_getenv("ORCVIO_FUSED_DBG") != nullptr;   // diagnostics
    static double* d_dbg = nullptr;
    if (want_dbg) {
        if (!d_dbg) { HIPCHK(hipMalloc(&d_dbg, 8 * 80)); HIPCHK(hipMemset(d_dbg, 0, 8 * 80)); }
        fa.dbg = d_dbg;
    }
    const size_t lds = sizeof(double) * obj_fused_lds_doubles(Kmax, pl.NOP, N, rows_max);
    hipLaunchKernelGGL(k_obj_fused, dim3(fa.nobj), dim3(64 * OBJ_FUSED_NW), lds, s, fa);
    if (want_dbg) {
        double pv[80];
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(pv, d_dbg, 8 * 80, hipMemcpyDeviceToHost));
        fprintf(stderr, "k_obj_fused object 0: tolerance %.3e, border pivots", pv[64]);
        for (int i = 0; i < 9; ++i) fprintf(stderr, " %.3e", pv[i]);
        fprintf(stderr, "; keypoint pivots");
        for (int i = 9; i < 9 + 3 * Kmax && i < 64; ++i) fprintf(stderr, " %.2e", pv[i]);
        fprintf(stderr, "\n");
    }
    HIPCHK(hipGetLastError());
    prof_mark(h, s, "k_obj_fused");
    if (!h->d_obj_done) { HIPCHK(hipMalloc(&h->d_obj_done, 128)); HIPCHK(hipMemset(h->d_obj_done, 0, 128)); }
    hipLaunchKernelGGL(k_gemm_objA, dim3((NAP / 16) * (NAP / 16)), dim3(512), 0, s, (const double*)h->d_Yobj, NAP, fa.nobj * pl.NOP, (const double*)pl.d_Sg,
                       fa.nobj, N, (const double*)pl.d_Hfr, 1, cb0, NA, dst, (unsigned*)nullptr);
    if (signal_done) {   // (the frame call: the object solve on the other stream polls this word; a stand-alone update is ordered by its stream)
        h->obj_done_total += 1u;
        hipLaunchKernelGGL(k_obj_done, dim3(1), dim3(64), 0, s, h->d_obj_done, h->obj_done_total);
    }
    HIPCHK(hipGetLastError());
    prof_mark(h, s, "k_gemm_objA (A')");
    if (want_stamps) {
        unsigned long long st[16];
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(st, d_st, 128, hipMemcpyDeviceToHost));
        auto at = [&](int i) { return (st[i] - st[0]) * 0.01; };
        fprintf(stderr, "k_obj_fused stamps, object 0 (us after its first instruction): rows %.2f | clear %.2f | lists %.2f | keypoint blocks %.2f | border %.2f | cond %.2f | Q~ %.2f | "
                        "T %.2f | orthonormalised %.2f | Y, tiles (matrix cores) %.2f | end %.2f\n",
                at(1), at(9), at(10), at(2), at(3), at(11), at(4), at(7), at(5), at(8), at(6));
    }
    h->obj_last_fused = true;
    return ORCVIO_OK;
}
static int objects_tracks_fused(orcvio_msckf_handle* h, hipStream_t s, double* dst, const orcvio_object_eval_flags* fl,
                                const orcvio_object_track* tracks, const ObjScan& sc, const int N, const int NA, const int NAP, const int cb0,
                                const bool signal_done) {
    ObjPlan pl;
    ObjFusedStage st;
    int rc = objects_fused_pack(h, fl, tracks, sc, pl, N, NAP, st);
    if (rc == ORCVIO_OK) rc = objects_fused_launch(h, s, dst, pl, st, sc.nobj, N, NA, NAP, cb0, signal_done);
    return rc;
}

// ---- object tracks, the general pipeline: rows materialised (k_object_rows_batch), then objects_pipeline ----------------------------------
// The host's staging: [track data (doubles) | kernel arguments (doubles)], then ints [frame_clone, frame_row0 per track | ObjIntLayout].
struct ObjGeneralStage { size_t nd_tot = 0, args_off = 0; ObjIntLayout lay; bool stacked = false; };
static int objects_general_pack(orcvio_msckf_handle* h, const orcvio_object_eval_flags* fl, const orcvio_object_track* tracks, const ObjScan& sc,
                                ObjPlan& pl, ObjGeneralStage& st) {
    const int N = h->N;
    const std::vector<ObjUse>& use = h->obj_use;
    pl = plan_of(sc);
    int rc = objects_scratch(h, &pl);
    if (rc != ORCVIO_OK) return rc;
    const size_t arg_dbl = OBJ_ARG_DOUBLES, args_off = sc.nd, nd = sc.nd + arg_dbl * use.size();
    size_t sumK = 0;
    for (const ObjUse& u : use) sumK += (size_t)tracks[u.t].n_keypoints;
    const ObjIntLayout lay = obj_int_layout((size_t)pl.rows_tot, pl.nobj, sumK, N, sc.ni);
    if ((rc = obj_stage_reserve(h, nd * 8 + lay.ni * 4)) != ORCVIO_OK) return rc;
    double* hd = reinterpret_cast<double*>(h->h_obj_stage);
    int* hi = reinterpret_cast<int*>(h->h_obj_stage + nd * 8);
    double* dd = reinterpret_cast<double*>(h->d_obj_in);
    int* di = reinterpret_cast<int*>(h->d_obj_in + nd * 8);
    const ObjIntViews hv = lay.views(hi);
    const ObjRowArrays ra{pl.d_hx, pl.d_hf, pl.d_res, pl.d_clone, pl.d_cols};
    ObjArrowBuild ab;
    ab.ok = h->arrow_opt && !(h->ref_stack_hf && pl.nobj > 1);
    int ng = 0;
    hv.rowptr[0] = 0;
    for (size_t ui = 0; ui < use.size(); ++ui) {
        const ObjUse& u = use[ui];
        const orcvio_object_track& ob = tracks[u.t];
        const signed char* nvp = h->obj_nv.data() + u.off_nv;
        const int *fc = hi + u.off_i, *fr0 = fc + ob.n_frames;
        const int rows = obj_pack_track(ob, u, nvp, fl, pl.ldf, pl.no_max, ra, hd, hi, dd, di, reinterpret_cast<ObjEvalArgs*>(hd + args_off + arg_dbl * ui));
        obj_group_rows(fc, fr0, nvp, ob.n_frames, N, u.row0, (int)ui, hv.ridx, hv.groups, &ng);
        hv.rowptr[ui + 1] = u.row0 + rows;
        obj_arrow_from_masks(ob, fc, fr0, u.row0, rows, h->obj_vmask, ab, hv.arrows + ui, hv.kp_range, hv.kp_rows);
    }
    st.stacked = h->ref_stack_hf && pl.nobj > 1;
    if (st.stacked) {
        merge_objects_ref_stack(N, pl.rows_tot, hv.ridx, hv.rowptr, hv.groups, &ng);
        pl.nobj = 1; h->obj_count = 1;
        rc = objects_scratch(h, &pl);   // the scratch of ONE block: Cd | Sg | Hr adjacent again (the row arrays depend on the row count only)
        if (rc != ORCVIO_OK) return rc;
    }
    pl.ngroups = ng;
    pl.arrow = ab.ok;   // (never after a merge)
    if (pl.arrow) {   // room for the arrow factors (the row arrays the kernel arguments point at do not move: same sizes)
        pl.Kmax = ab.Kmax; pl.rows_max = ab.rows_max;
        double* keep_objH = h->d_objH; int* keep_obj_i = h->d_obj_i;
        rc = objects_scratch(h, &pl);
        if (rc != ORCVIO_OK) return rc;
        if (h->d_objH != keep_objH || h->d_obj_i != keep_obj_i) { g_last_error = "objects_local_tracks: scratch moved"; return ORCVIO_ERR_HIP; }
    }
    plan_views(pl, lay.views(di));
    st.nd_tot = nd; st.args_off = args_off; st.lay = lay;
    return ORCVIO_OK;
}
// The launches: the ingest, the rows of n_eval tracks of at most Fmax frames, the compression (no synchronisation: the staging is pinned).
static int objects_general_launch(orcvio_msckf_handle* h, hipStream_t s, double* dst, const ObjPlan& pl, const ObjGeneralStage& st, const int n_eval,
                                  const int Fmax) {
    const int N = h->N, NAP = h->NAP;
    { const int ri = launch_ingest(h, s, h->h_obj_stage_dev, h->d_obj_in, st.lay.ingest_bytes(st.nd_tot, pl.ngroups)); if (ri != ORCVIO_OK) return ri; }
    // the rows, and in the same launch the zeroing of what the compression accumulates into (Cd, Sg, Hr: adjacent) and of the
    // two pivot counters.  After a merge for ORCVIO_OPT_REF_STACK_HF the scratch layout is another one: plain fills there.
    const bool fold_zero = !st.stacked;
    const size_t nzero = (size_t)pl.nobj * pl.NOP * NAP + (size_t)pl.nobj * N * 64 + (size_t)pl.nobj * N * pl.NOP;
    const unsigned zero_rows = fold_zero ? (unsigned)((nzero / 2 + (size_t)Fmax * 64 * 8 - 1) / ((size_t)Fmax * 64 * 8)) : 0u;   // ~8 double2 per thread
    hipLaunchKernelGGL(k_object_rows_batch, dim3(Fmax, (unsigned)n_eval + zero_rows), dim3(64), 0, s,
                       reinterpret_cast<const ObjEvalArgs*>(reinterpret_cast<double*>(h->d_obj_in) + st.args_off), n_eval, pl.d_Cd, nzero, h->d_info + 4);
    HIPCHK(hipGetLastError());
    h->obj_status_cleared = fold_zero;   // (info[9..12] zeroed by that launch: objects_finish_impl need not)
    return objects_pipeline(h, s, dst, pl, fold_zero, true);
}

// The same from object TRACKS (state at the LM optimum + observations): the residual rows and Jacobians of SURVEY 8a rows
// 12-16 are evaluated on the device (k_object_rows) straight into the compact row arrays -- nothing but the tracks
// crosses PCIe.  Tracks whose in-window rows do not exceed their state columns are skipped (math_utils.hpp:292).
int32_t orcvio_msckf_objects_local_tracks(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, const orcvio_object_eval_flags* fl,
                                          int32_t n_clones, const orcvio_object_track* tracks, int32_t n_tracks, const double* P,
                                          double* d_dst, int32_t* dof_out, void* stream) {
    if (!h || !flags || !fl || n_tracks < 0 || (n_tracks > 0 && !tracks)) { g_last_error = "objects_local_tracks: null argument"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    static const bool timing = dbg_getenv("ORCVIO_TIMING") != nullptr;   // diagnostics: host wall time of the parts of this call
    const auto tt0 = std::chrono::steady_clock::now();
    { const int rp = objects_problem(h, flags, n_clones, P, "objects_local_tracks"); if (rp != ORCVIO_OK) return rp; }
    const int N = n_clones, NAP = h->NAP;
    ObjScan sc;
    if (h->obj_early) sc = *h->obj_early;   // (the frame call has scanned the tracks already, for the compression it launched ahead)
    else { const int rs = objects_scan(h, N, tracks, n_tracks, sc); if (rs != ORCVIO_OK) return rs; }
    hipStream_t s = pick_stream(h, stream);
    double* dst = d_dst ? d_dst : h->d_Ab;
    if (dof_out) *dof_out = sc.dof;
    const auto tt1 = std::chrono::steady_clock::now();
    int rc = objects_begin(h, s, P, "objects_local_tracks", sc, dst);
    if (rc != ORCVIO_OK || sc.nobj == 0) return rc;
    const auto tt2 = std::chrono::steady_clock::now();
    rc = launch_prior_fork(h, s);   // the Cholesky of P runs on the side stream while the tracks are staged and their rows evaluated
    if (rc != ORCVIO_OK) return rc;
    h->obj_last_fused = false;
    if (h->obj_early) { h->obj_early = nullptr; h->obj_last_fused = true; return ORCVIO_OK; }   // (the frame call launched the compression ahead: objects_tracks_fused on its stream)
    if (obj_fused_eligible(h, tracks, N, sc.no_max)) return objects_tracks_fused(h, s, dst, fl, tracks, sc, N, h->NA, NAP, h->flags.leg_dim - 15, h->frame_mode);
    ObjPlan pl;
    ObjGeneralStage st;
    if ((rc = objects_general_pack(h, fl, tracks, sc, pl, st)) != ORCVIO_OK) return rc;
    const auto tt3 = std::chrono::steady_clock::now();
    rc = objects_general_launch(h, s, dst, pl, st, sc.nobj, sc.Fmax);
    if (timing) {
        const auto tt4 = std::chrono::steady_clock::now();
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "objects_local_tracks: sizes %.1f us, prior (sync + P staging + copy) %.1f us, staging %.1f us, enqueue %.1f us\n", us(tt0, tt1),
                us(tt1, tt2), us(tt2, tt3), us(tt3, tt4));
    }
    return rc;
}

// Second part: rank-ordered sum of the gathered blocks, replicated solve, joint chi-square gate with the TOTAL degrees
// of freedom of all ranks' objects, gated write-back.
static int objects_finish_impl(orcvio_msckf_handle* h, const double* d_blocks, int n_blocks, size_t stride, const double* meta0, int dof_total,
                               hipStream_t s, UpdateCall& c) {
    h->last_stream = s;
    if (h->dl_pending) { HIPCHK(hipStreamSynchronize(h->dl_stream)); h->dl_pending = false; }
    h->obj_dof = dof_total;
    h->A_deferred = false;
    int rc = ORCVIO_OK;
    if (!(n_blocks == 1 && d_blocks == h->d_A)) {   // (one-shot single-GPU calls compress into d_A: nothing to sum)
        rc = launch_reduce(h, s, d_blocks, n_blocks, h->d_A, stride, meta0);
        if (rc != ORCVIO_OK) return rc;
        prof_mark(h, s, "k_gram_reduce");
    } else if (!h->obj_status_cleared) {
        HIPCHK(hipMemsetAsync(h->d_info + 9, 0, sizeof(int) * 4, s));   // (no shard status words in this update)
    }
    h->obj_status_cleared = false;
    // Kalman solve in square-root form, gate, gated write-back
    if (h->prior_forked) HIPCHK(hipStreamWaitEvent(s, h->ev_side, 0));
    prof_mark(h, s, "join chol(P) (side stream)");
    // table value below 500 dof, on the fly above (:1962-1968); dof 0 (no usable object anywhere) can never pass.  The gate is
    // decided inside k_finish_sqrt (ObjGate) -- or by the finish workgroups of the solve's launch (LaFin), which is why it is known here.
    h->obj_thr = dof_total > 0 ? orcvio_msckf_chi2_quantile(dof_total, h->flags.chi2_prob) : -1.0;
    for (int st = ST_FORM_U; st <= ST_TRSM && rc == ORCVIO_OK; ++st) rc = launch_solve_stage(h, s, st, c);
    if (rc != ORCVIO_OK) return rc;
    prof_mark(h, s, "k_gemm(U)+k_gemm(M)+k_potrf_solve(M)");
    rc = launch_solve_stage(h, s, ST_FINISH, c);
    prof_mark(h, s, "k_finish_sqrt (gate inside)");
    if (rc == ORCVIO_OK) mark_update_enqueued(h, 2, meta0 != nullptr);
    return rc;
}

// Second part: rank-ordered sum of the gathered blocks, replicated solve, joint chi-square gate with the TOTAL degrees
// of freedom of all ranks' objects, gated write-back.
static int objects_finish_checked(orcvio_msckf_handle* h, const double* d_blocks, int32_t n_blocks, int32_t dof_total, void* stream, UpdateCall& c) {
    if (!h || !h->uploaded || !h->objects_mode || !d_blocks || n_blocks < 1) { g_last_error = "objects_finish: no local object block"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    return objects_finish_impl(h, d_blocks, n_blocks, 0, nullptr, dof_total, pick_stream(h, stream), c);
}
int32_t orcvio_msckf_objects_finish(orcvio_msckf_handle* h, const double* d_blocks, int32_t n_blocks, int32_t dof_total, void* stream) {
    UpdateCall c;
    return objects_finish_checked(h, d_blocks, n_blocks, dof_total, stream, c);
}

// Results of an object update (after orcvio_msckf_objects_finish): accept[0], gamma[0], dx, P_out, stats, optional G.
int32_t orcvio_msckf_objects_download(orcvio_msckf_handle* h, orcvio_msckf_result* res) {
    if (!h || !res || !h->ran || !h->objects_mode) { g_last_error = "objects_download: no finished object update"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    const int n = h->n, NA = h->NA, dof = h->obj_dof, nobj = h->obj_count;
    const orcvio_msckf_flags* flags = &h->flags;
    int rc = ORCVIO_OK;
    // results: ONE copy of the outputs arena [info | dx | gamma | accept | (P+)] into its pinned mirror (enqueued behind the
    // update by the one-shot entry points; here for staged callers), one synchronisation
    const bool want_P = res->P_out != nullptr;
    if (h->pub_pending) {   // the one-shot calls: k_epilogue is pushing the results into the pinned block; wait on its flag
        h->pub_pending = false;
        const int rw = io_wait(h, h->last_stream ? h->last_stream : h->stream);
        if (rw != ORCVIO_OK) { h->ran = false; return rw; }
    } else {
        if (!(h->dl_pending && (h->dl_with_P || !want_P))) {
            hipStream_t sd = h->last_stream ? h->last_stream : h->stream;
            if (h->dl_pending) HIPCHK(hipStreamSynchronize(h->dl_stream));
            const int rq = download_enqueue(h, sd, want_P);
            if (rq != ORCVIO_OK) return rq;
        }
        HIPCHK(hipStreamSynchronize(h->dl_stream));
        h->dl_pending = false;
    }
    const char* so = h->h_stage + h->in_cap + h->out_shift;
    const double* dx = reinterpret_cast<const double*>(so + h->oo_dx);
    const int acc = *reinterpret_cast<const int*>(so + h->oo_accept);
    double gam = *reinterpret_cast<const double*>(so + h->oo_gamma);
    int info[16] = {0};
    std::memcpy(info, so, sizeof(int) * 16);
    if (info[8] != 0) {   // a solver wavefront of k_potrf_solve gave up waiting for the factorisation workgroup: the solve ran
                          // through on stale bytes and nothing of this update may be committed
        HIPCHK(hipMemset(h->d_info + 8, 0, sizeof(int)));
        h->ran = false;
        g_last_error = "k_potrf_solve: an in-launch hand-off timed out";
        return ORCVIO_ERR_TIMEOUT;
    }
    if (h->last_sharded && info[9] != 0) {   // sharded update: another rank took part with an empty share and a status word
        h->ran = false;
        g_last_error = "sharded object update: rank " + std::to_string(info[9] - 1) + " could not take part with its tracks (status " + std::to_string(info[10]) + ")";
        return ORCVIO_ERR_PEER;
    }
    if (info[2] != 0 || info[3] != 0) {   // as orcvio_msckf_download: the device left P and x alone, nothing to commit
        h->ran = false;
        g_last_error = "M = s2 I + L^T A L is not positive definite (a prior beyond ~1e16 s2 in scale, or non-finite input): no update";
        return ORCVIO_ERR_NOT_SPD;
    }
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(dx[i])) {
            h->ran = false;   // (cov_commit would make a non-finite P+ the resident covariance)
            g_last_error = "non-finite result (NaN / Inf in the prior, the rows or the noise): no update";
            return ORCVIO_ERR_NOT_SPD;
        }
    if (res->dx) std::memcpy(res->dx, dx, sizeof(double) * n);
    if (res->P_out) std::memcpy(res->P_out, so + h->oo_Pout, sizeof(double) * (size_t)n * n);
    if (dof == 0) gam = NAN;   // no usable object on any rank (the reference returns before the gate, :2157)
    if (res->accept) res->accept[0] = acc;
    if (res->gamma) res->gamma[0] = gam;
    std::memset(res->stats, 0, sizeof(res->stats));
    res->stats[0] = acc ? dof : 0;
    res->stats[1] = acc ? NA : 0;
    res->stats[2] = acc ? nobj : 0;
    res->stats[3] = acc;
    if (flags->discard_large_update) {
        const double nv = std::sqrt(dx[3] * dx[3] + dx[4] * dx[4] + dx[5] * dx[5]);
        const double np = std::sqrt(dx[6] * dx[6] + dx[7] * dx[7] + dx[8] * dx[8]);
        res->stats[4] = (nv > 1.0 || np > 1.5) ? 1 : 0;
    }
    res->stats[5] = info[0];
    res->stats[6] = info[1];
    res->stats[7] = info[4];   // rank-deficient directions met in some Hf
    h->obj_refined = info[5];  // objects projected through the explicit basis (orcvio_msckf_objects_refined)
    if (res->G) {   // basis-independent K*H of the applied update (zero if rejected)
        if (acc) {
            rc = compute_optional(h, false, false, true);
            if (rc != ORCVIO_OK) return rc;
            std::vector<double> Gd((size_t)n * h->NP);
            HIPCHK(hipMemcpy(Gd.data(), h->d_KG, sizeof(double) * Gd.size(), hipMemcpyDeviceToHost));
            std::memset(res->G, 0, sizeof(double) * (size_t)n * n);
            for (int i = 0; i < n; ++i)
                for (int c = 0; c < NA; ++c) res->G[(size_t)i * n + 15 + c] = Gd[(size_t)i * h->NP + c];
        } else {
            std::memset(res->G, 0, sizeof(double) * (size_t)n * n);
        }
    }
    return ORCVIO_OK;
}

// Cumulative counters of the handle (since create): what the caller cannot see from one update's stats[].
int32_t orcvio_msckf_counters(orcvio_msckf_handle* h, int64_t* counters, int32_t count) {
    if (!h || !counters || count < 1) { g_last_error = "counters: null argument"; return ORCVIO_ERR_INVALID; }
    const int64_t v[ORCVIO_COUNTERS] = {h->front_fallbacks, h->cnt_graph_captures, h->cnt_graph_replays, h->cnt_plain_runs,
                                        h->front_blocked_by_comm ? 1 : 0, h->obj_last_fused ? 1 : 0, h->cnt_chained, (int64_t)h->cnt_prestaged,
                                        h->cnt_step_frames, h->cnt_step_repairs, h->cnt_sym_pulls, h->cnt_lists_in_place};
    for (int i = 0; i < count && i < ORCVIO_COUNTERS; ++i) counters[i] = v[i];
    for (int i = ORCVIO_COUNTERS; i < count; ++i) counters[i] = 0;
    return ORCVIO_OK;
}

int32_t orcvio_msckf_objects_refined(orcvio_msckf_handle* h, int32_t* count) {
    if (!h || !count) { g_last_error = "objects_refined: null argument"; return ORCVIO_ERR_INVALID; }
    *count = h->obj_refined;
    return ORCVIO_OK;
}

// ORCVIO_OPT_OBJECT_DOF = 1: the gate's degrees of freedom are rows - rank(H_f) instead of the reference's rows - columns
// (src/orcvio.cpp:2172): the device projects onto the WHOLE left null space of a rank-deficient H_f (rows - rank directions,
// DESIGN.md 3.4), and this makes the threshold count what gamma sums.  The rank is what the structured QR found (dropped
// pivots, info[4]): one small copy and a synchronisation between the compression and the solve, in this mode only.
static int objects_rank_dof(orcvio_msckf_handle* h, hipStream_t s, int32_t* dof) {
    if (!h->obj_dof_rank || h->obj_count == 0) return ORCVIO_OK;
    int dropped = 0;
    HIPCHK(hipMemcpyAsync(&dropped, h->d_info + 4, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *dof += dropped;
    return ORCVIO_OK;
}

int32_t orcvio_msckf_update_objects(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int32_t n_clones,
                                    const orcvio_msckf_object_rows* objs, int32_t n_objects, const double* P,
                                    orcvio_msckf_result* res) {
    if (!res) { g_last_error = "update_objects: null argument"; return ORCVIO_ERR_INVALID; }
    int32_t dof = 0;
    int rc = orcvio_msckf_objects_local(h, flags, n_clones, objs, n_objects, P, h->d_A, &dof, nullptr);
    if (rc == ORCVIO_OK) rc = objects_rank_dof(h, h->stream, &dof);
    if (rc != ORCVIO_OK) return rc;
    rc = orcvio_msckf_objects_finish(h, h->d_A, 1, dof, nullptr);
    if (rc == ORCVIO_OK) rc = download_enqueue(h, h->stream, res->P_out != nullptr);
    if (rc != ORCVIO_OK) return rc;
    rc = orcvio_msckf_objects_download(h, res);
    h->objects_mode = false;
    return rc;
}

// c: the record of the solve (the repeat of a frame call that lost a hand-off asks for the one-workgroup factorisation + solve)
static int update_object_tracks_impl(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, const orcvio_object_eval_flags* fl,
                                     int32_t n_clones, const orcvio_object_track* tracks, int32_t n_tracks, const double* P,
                                     orcvio_msckf_result* res, UpdateCall& c) {
    if (!res) { g_last_error = "update_object_tracks: null argument"; return ORCVIO_ERR_INVALID; }
    int32_t dof = 0;
    static const bool timing = dbg_getenv("ORCVIO_TIMING") != nullptr;   // diagnostics: host wall time of the three parts
    const auto t0 = std::chrono::steady_clock::now();
    int rc = orcvio_msckf_objects_local_tracks(h, flags, fl, n_clones, tracks, n_tracks, P, h->d_A, &dof, nullptr);
    if (rc == ORCVIO_OK) rc = objects_rank_dof(h, h->stream, &dof);
    if (rc != ORCVIO_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    rc = objects_finish_checked(h, h->d_A, 1, dof, nullptr, c);
    if (rc == ORCVIO_OK) rc = download_enqueue(h, h->stream, res->P_out != nullptr);
    if (rc != ORCVIO_OK) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    rc = orcvio_msckf_objects_download(h, res);
    const auto t3 = std::chrono::steady_clock::now();
    if (timing) {
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "update_object_tracks: local %.1f us, finish (enqueue) %.1f us, download %.1f us\n", us(t0, t1), us(t1, t2), us(t2, t3));
    }
    h->objects_mode = false;
    return rc;
}
int32_t orcvio_msckf_update_object_tracks(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, const orcvio_object_eval_flags* fl,
                                          int32_t n_clones, const orcvio_object_track* tracks, int32_t n_tracks, const double* P,
                                          orcvio_msckf_result* res) {
    UpdateCall c;
    return update_object_tracks_impl(h, flags, fl, n_clones, tracks, n_tracks, P, res, c);
}

// ---- the object update from ObjectLM messages (SURVEY.md 8f rank 4) ----------------------------------------------------
// Sophus v1.0.0 SE3d::exp, tangent (upsilon, omega): R = exp(omega), t = V upsilon
static void se3_exp_wire(const double xi[6], double T[16]) {
    const double* u = xi;
    const double* w = xi + 3;
    double R[9];
    so3_exp_decl(w, R);
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
    const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double W2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
    double a, b;
    if (th < 1e-10) { a = 0.5; b = 1.0 / 6.0; }
    else { a = (1.0 - std::cos(th)) / th2; b = (th - std::sin(th)) / (th2 * th); }
    double V[9];
    for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * W[i] + b * W2[i];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
        T[4 * i + 3] = V[3 * i] * u[0] + V[3 * i + 1] * u[1] + V[3 * i + 2] * u[2];
    }
    T[12] = T[13] = T[14] = 0.0; T[15] = 1.0;
}

int32_t orcvio_msckf_update_object_lm_msgs(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int32_t n_clones,
                                           const double* cur_window_timestamps, const double* R_b2c, const double* t_c_b,
                                           int32_t fix_D, int32_t wire_row_major, const orcvio_object_lm_msg* msgs, int32_t n_msgs,
                                           const double* P, orcvio_msckf_result* result) {
    if (!h || !flags || !cur_window_timestamps || !R_b2c || !t_c_b || n_msgs < 0 || (n_msgs > 0 && !msgs) || !result) {
        g_last_error = "update_object_lm_msgs: null argument"; return ORCVIO_ERR_INVALID;
    }
    // constructObjectResidualJacobians per message (host arithmetic on a few hundred rows), into compact row blocks
    struct Block { std::vector<int32_t> clone; std::vector<double> hx6, hf, res; int ncol = 0; };
    std::vector<Block> blocks;
    std::vector<orcvio_msckf_object_rows> rows;
    blocks.reserve(n_msgs);
    for (int q = 0; q < n_msgs; ++q) {
        const orcvio_object_lm_msg& m = msgs[q];
        if (m.n_rows < 0 || m.n_obj_cols < 1 || m.n_frames < 0 || (m.n_rows > 0 && (!m.residual || !m.jacobian_wrt_object_state || !m.jacobian_wrt_sensor_state)) ||
            (m.n_frames > 0 && (!m.valid_camera_pose_mat || !m.timestamps || !m.zs_num_wrt_timestamps))) {
            g_last_error = "update_object_lm_msgs: malformed message"; return ORCVIO_ERR_INVALID;
        }
        if (m.n_obj_cols > 112) { g_last_error = "update_object_lm_msgs: object state columns must be 1..112"; return ORCVIO_ERR_INVALID; }
        long sum_zs_l = 0;
        for (int f = 0; f < m.n_frames; ++f) {
            // counts arrive from the wire: a negative one would lower the sum and let a row range start outside the arrays (ADVICE r2)
            if (m.zs_num_wrt_timestamps[f] < 0 || m.zs_num_wrt_timestamps[f] > (1 << 20)) { g_last_error = "update_object_lm_msgs: negative keypoint count"; return ORCVIO_ERR_INVALID; }
            sum_zs_l += 2L * m.zs_num_wrt_timestamps[f];
        }
        if (sum_zs_l + 4L * m.n_frames > (long)m.n_rows) { g_last_error = "update_object_lm_msgs: fewer rows than 2 x keypoints + 4 x frames"; return ORCVIO_ERR_INVALID; }
        const int sum_zs = (int)sum_zs_l;
        const int nr = m.n_rows, nc = m.n_obj_cols, nf = m.n_frames;
        // element (i, j) of a rows x cols wire matrix
        auto at = [&](const double* d, int rws, int cls, int i, int j) { return wire_row_major ? d[(size_t)i * cls + j] : d[(size_t)j * rws + i]; };
        Block b;
        b.ncol = nc;
        int src = 0;
        for (int f = 0; f < nf; ++f) {
            const int zf = 2 * m.zs_num_wrt_timestamps[f];
            int idx = -1;
            for (int c = 0; c < n_clones; ++c)
                if (cur_window_timestamps[c] == m.timestamps[f]) { idx = c; break; }   // exact match (std::find on doubles, :2073)
            if (idx >= 0) {
                double D[36];
                std::memset(D, 0, sizeof(D));
                if (fix_D) { for (int i = 0; i < 6; ++i) D[6 * i + i] = 1.0; }
                else {   // :2079-2093
                    double xi[6], wTc[16];
                    for (int i = 0; i < 6; ++i) xi[i] = at(m.valid_camera_pose_mat, 6, nf, i, f);
                    se3_exp_wire(xi, wTc);
                    double v[3], tbw[3];
                    for (int i = 0; i < 3; ++i) v[i] = -(R_b2c[3 * i] * t_c_b[0] + R_b2c[3 * i + 1] * t_c_b[1] + R_b2c[3 * i + 2] * t_c_b[2]);
                    for (int i = 0; i < 3; ++i) tbw[i] = wTc[4 * i] * v[0] + wTc[4 * i + 1] * v[1] + wTc[4 * i + 2] * v[2] + wTc[4 * i + 3];
                    if (flags->use_left_perturbation) {   // se3_ops.hpp:531-552, rows (upsilon, omega), cols (theta, p)
                        const double S[9] = {0, -tbw[2], tbw[1], tbw[2], 0, -tbw[0], -tbw[1], tbw[0], 0};
                        for (int i = 0; i < 3; ++i) {
                            for (int j = 0; j < 3; ++j) D[6 * i + j] = S[3 * i + j];
                            D[6 * (3 + i) + i] = 1.0;
                            D[6 * i + 3 + i] = 1.0;
                        }
                    } else {
                        const double S[9] = {0, -t_c_b[2], t_c_b[1], t_c_b[2], 0, -t_c_b[0], -t_c_b[1], t_c_b[0], 0};
                        for (int i = 0; i < 3; ++i)
                            for (int j = 0; j < 3; ++j) {
                                double sm = 0;
                                for (int k = 0; k < 3; ++k) sm += R_b2c[3 * i + k] * S[3 * k + j];
                                D[6 * i + j] = -sm;
                                D[6 * (3 + i) + j] = R_b2c[3 * i + j];
                                D[6 * i + 3 + j] = wTc[4 * j + i];   // R_w2c = R_c2w^T
                            }
                    }
                }
                auto emit = [&](int r) {
                    for (int c = 0; c < 6; ++c) {
                        double sm = 0;
                        for (int k = 0; k < 6; ++k) sm += at(m.jacobian_wrt_sensor_state, nr, 6, r, k) * D[6 * k + c];
                        b.hx6.push_back(sm);
                    }
                    for (int c = 0; c < nc; ++c) b.hf.push_back(at(m.jacobian_wrt_object_state, nr, nc, r, c));
                    b.res.push_back(m.residual[r]);
                    b.clone.push_back(idx);
                };
                for (int r = src; r < src + zf; ++r) emit(r);
                for (int r = sum_zs + 4 * f; r < sum_zs + 4 * f + 4; ++r) emit(r);
            }
            src += zf;
        }
        if (b.clone.empty()) continue;   // no pose of the object in the window (:2149): the message contributes nothing
        blocks.push_back(std::move(b));
    }
    for (const Block& b : blocks)
        rows.push_back(orcvio_msckf_object_rows{(int32_t)b.clone.size(), b.ncol, b.clone.data(), b.hx6.data(), b.hf.data(), b.res.data()});
    return orcvio_msckf_update_objects(h, flags, n_clones, rows.data(), (int32_t)rows.size(), P, result);
}

// ---- object residual rows (SURVEY.md 8a rows 12-16) ------------------------------------------------------
int32_t orcvio_msckf_object_rows_eval(orcvio_msckf_handle* h, const orcvio_object_eval_flags* fl, const orcvio_object_track* ob,
                                      int32_t cap_rows, int32_t* n_rows, int32_t* row_clone, double* Hx6, double* Hf, double* res) {
    if (!h || !fl || !ob || !n_rows || !ob->wTo || !ob->shape || !ob->frame_wTc || !ob->frame_bbox || !ob->frame_clone ||
        (ob->n_keypoints > 0 && (!ob->kps || !ob->frame_zs))) { g_last_error = "object_rows_eval: null argument"; return ORCVIO_ERR_INVALID; }
    const int K = ob->n_keypoints, F = ob->n_frames;
    if (K < 0 || K > 60 || F < 1) { g_last_error = "object_rows_eval: 0..60 keypoints (one wavefront per frame), >= 1 frame"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    const int ncol = 9 + 3 * K;
    // row offsets of the in-window frames (valid keypoint rows first, then 4 bbox rows)
    std::vector<int> row0(F, 0);
    int rows = 0;
    for (int f = 0; f < F; ++f) {
        if (ob->frame_clone[f] < 0) continue;
        int nv = 0;
        for (int k = 0; k < K; ++k) {
            const double a = ob->frame_zs[((size_t)f * K + k) * 2], b = ob->frame_zs[((size_t)f * K + k) * 2 + 1];
            if (std::isfinite(a) && std::isfinite(b)) ++nv;   // row finite test, ObjectLM.cpp:171-198
        }
        row0[f] = rows;
        rows += 2 * nv + 4;
    }
    *n_rows = rows;
    if (rows == 0) return ORCVIO_OK;
    if (rows > cap_rows || !row_clone || !Hx6 || !Hf || !res) { g_last_error = "object_rows_eval: output buffers too small"; return ORCVIO_ERR_CAPACITY; }
    // pack inputs / outputs into the (growable) object scratch buffers
    const size_t in_d = 16 + 3 + (size_t)3 * K + (size_t)F * (16 + 2 * K + 4);
    const size_t out_d = (size_t)rows * (6 + ncol + 1);
    int rc;
    if ((rc = grow(&h->d_objH, &h->cap_objH, in_d + out_d)) != ORCVIO_OK) return rc;
    if ((rc = grow(&h->d_obj_i, &h->cap_obj_i, (size_t)2 * F + rows)) != ORCVIO_OK) return rc;
    std::vector<double> hin(in_d);
    double* q = hin.data();
    std::memcpy(q, ob->wTo, 16 * 8); q += 16;
    std::memcpy(q, ob->shape, 3 * 8); q += 3;
    if (K > 0) std::memcpy(q, ob->kps, (size_t)3 * K * 8);
    q += 3 * K;
    std::memcpy(q, ob->frame_wTc, (size_t)16 * F * 8); q += (size_t)16 * F;
    if (K > 0) std::memcpy(q, ob->frame_zs, (size_t)2 * K * F * 8);
    q += (size_t)2 * K * F;
    std::memcpy(q, ob->frame_bbox, (size_t)4 * F * 8);
    std::vector<int> hi(2 * F);
    for (int f = 0; f < F; ++f) { hi[f] = ob->frame_clone[f]; hi[F + f] = row0[f]; }
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->d_objH, hin.data(), sizeof(double) * in_d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->d_obj_i, hi.data(), sizeof(int) * 2 * F, hipMemcpyHostToDevice, s));
    ObjEvalArgs a;
    a.wTo = h->d_objH; a.shape = a.wTo + 16; a.kps = a.shape + 3; a.frame_wTc = a.kps + 3 * K;
    a.frame_zs = a.frame_wTc + (size_t)16 * F; a.frame_bbox = a.frame_zs + (size_t)2 * K * F;
    a.frame_clone = h->d_obj_i; a.frame_row0 = h->d_obj_i + F;
    a.K = K; a.F = F; a.ncol = ncol; a.ldhf = ncol; a.rcol = -1; a.row_cols = nullptr;
    a.obj_left = fl->use_left_perturbation; a.new_bbox = fl->use_new_bbox_residual; a.vio_left = fl->vio_use_left_perturbation;
    a.fix_D = fl->fix_dcampose_dimupose_to_identity;
    std::memcpy(a.R_b2c, fl->R_b2c, sizeof(a.R_b2c));
    std::memcpy(a.t_c_b, fl->t_c_b, sizeof(a.t_c_b));
    double* outd = h->d_objH + in_d;
    a.Hx6 = outd; a.Hf = outd + (size_t)rows * 6; a.res = a.Hf + (size_t)rows * ncol;
    a.row_clone = h->d_obj_i + 2 * F;
    hipLaunchKernelGGL(k_object_rows, dim3(F), dim3(64), 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(Hx6, a.Hx6, sizeof(double) * (size_t)rows * 6, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(Hf, a.Hf, sizeof(double) * (size_t)rows * ncol, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(res, a.res, sizeof(double) * rows, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(row_clone, a.row_clone, sizeof(int) * rows, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ORCVIO_OK;
}
