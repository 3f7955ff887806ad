// capi_handle.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// chi-square quantile, the arenas, create / destroy, options.

// ---- chi-square quantile (replaces boost::math::quantile, src/orcvio.cpp:486-494) --------
static double reg_lower_gamma(double a, double x) {
    if (x <= 0.0) return 0.0;
    const double lg = std::lgamma(a);
    if (x < a + 1.0) {   // series
        double term = 1.0 / a, sum = term, ap = a;
        for (int i = 0; i < 200000; ++i) {
            ap += 1.0;
            term *= x / ap;
            sum += term;
            if (std::fabs(term) < std::fabs(sum) * 1e-17) break;
        }
        return sum * std::exp(a * std::log(x) - x - lg);
    }
    // modified Lentz continued fraction for Q(a,x)
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int i = 1; i < 200000; ++i) {
        const double an = -(double)i * ((double)i - a);
        b += 2.0;
        d = an * d + b;
        if (std::fabs(d) < tiny) d = tiny;
        c = b + an / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < 1e-16) break;
    }
    return 1.0 - std::exp(a * std::log(x) - x - lg) * h;
}

double orcvio_msckf_chi2_quantile(int32_t dof, double prob) {
    if (dof < 1 || !(prob > 0.0 && prob < 1.0)) return NAN;
    const double a = 0.5 * dof;
    // normal quantile by bisection, Wilson-Hilferty start, then safeguarded Newton
    double zl = -12.0, zh = 12.0;
    for (int i = 0; i < 100; ++i) {
        const double zm = 0.5 * (zl + zh);
        if (0.5 * std::erfc(-zm / std::sqrt(2.0)) < prob) zl = zm; else zh = zm;
    }
    const double zq = 0.5 * (zl + zh);
    const double wh = 1.0 - 2.0 / (9.0 * dof) + zq * std::sqrt(2.0 / (9.0 * dof));
    double x = dof * wh * wh * wh;
    if (!(x > 0.0)) x = 1e-3;
    double lo = 0.0, hi = 4.0 * x + 60.0;
    for (int it = 0; it < 300; ++it) {
        const double f = reg_lower_gamma(a, 0.5 * x) - prob;
        if (f > 0.0) hi = x; else lo = x;
        const double lpdf = (a - 1.0) * std::log(0.5 * x) - 0.5 * x - std::lgamma(a) - std::log(2.0);
        double xn = x - f / std::exp(lpdf);
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
        const bool done = std::fabs(xn - x) <= 1e-15 * std::fabs(x);
        x = xn;
        if (done) break;
    }
    return x;
}

// ---- arenas -----------------------------------------------------------------------------------
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
// [poses | obs_ptr | row_ptr | clone_ptr | p_w | obs_clone | clone_obs | obs_z | (obs_zvel) | (P)], 256-byte aligned parts
static size_t inputs_bytes(int N, int F, int nobs, bool zvel, size_t n_with_P) {
    return al256(sizeof(double) * POSE_STRIDE * N) + 2 * al256(sizeof(int) * (F + 1)) + al256(sizeof(int) * (2 * N + 4)) +
           al256(sizeof(double) * 3 * F) + 2 * al256(sizeof(int) * nobs) + al256(sizeof(double) * 2 * nobs) +
           (zvel ? al256(sizeof(double) * 2 * nobs) : 0) + al256(sizeof(double) * n_with_P * n_with_P);
}
static size_t outputs_bytes(int n, int F) {
    return 256 + al256(sizeof(double) * n) + al256(sizeof(double) * F) + al256(sizeof(int) * F) + al256(sizeof(double) * (size_t)n * n);
}
// Compact layout of the inputs for the sizes of this upload; with_P = false: the prior is the resident covariance and
// does not travel.  The device pointers are functions of (N, F, nobs, zvel, with_P) only, so equal shapes give equal
// pointers (the captured launch graphs stay valid; d_P is part of the launch signature all the same).
static void layout_inputs(orcvio_msckf_handle* h, int N, int F, int nobs, bool zvel, bool with_P, int n) {
    // the arrays the HOST derives from the caller's (row offsets, per-clone lists: upload_finalize) stand in front, everything the
    // caller writes behind them: the caller-written part can travel before the derived part exists (ingest_raw)
    size_t o = 0;
    h->io_rptr = o; o += al256(sizeof(int) * (F + 1));
    h->io_cptr = o; o += al256(sizeof(int) * (2 * N + 4));
    h->io_cobs = o; o += al256(sizeof(int) * nobs);
    h->io_poses = o; o += al256(sizeof(double) * POSE_STRIDE * N);
    h->io_optr = o; o += al256(sizeof(int) * (F + 1));
    h->io_pw = o; o += al256(sizeof(double) * 3 * F);
    h->io_oclone = o; o += al256(sizeof(int) * nobs);
    h->io_z = o; o += al256(sizeof(double) * 2 * nobs);
    h->io_zvel = h->io_z;   // (never read without estimate_td: any valid address)
    if (zvel) { h->io_zvel = o; o += al256(sizeof(double) * 2 * nobs); }
    h->io_P = o;
    h->in_used = o;         // what travels besides P
    char* d = h->d_in;
    h->d_poses = reinterpret_cast<double*>(d + h->io_poses);
    h->d_obs_ptr = reinterpret_cast<int*>(d + h->io_optr);
    h->d_row_ptr = reinterpret_cast<int*>(d + h->io_rptr);
    h->d_clone_ptr = reinterpret_cast<int*>(d + h->io_cptr);
    h->d_pw = reinterpret_cast<double*>(d + h->io_pw);
    h->d_obs_clone = reinterpret_cast<int*>(d + h->io_oclone);
    h->d_clone_obs = reinterpret_cast<int*>(d + h->io_cobs);
    h->d_obs_z = reinterpret_cast<double*>(d + h->io_z);
    h->d_obs_zvel = reinterpret_cast<double*>(d + h->io_zvel);
    h->d_P = with_P ? reinterpret_cast<double*>(d + h->io_P) : h->d_Pres;
    (void)n;
}
// [info 64 ints | dx | gamma | accept | P+]: the small part is one copy, with P+ behind it one longer copy
static void layout_outputs(orcvio_msckf_handle* h, int n, int F) {
    size_t o = 256;
    h->d_info = reinterpret_cast<int*>(h->d_outs);
    h->d_flag = h->d_info + 32;
    h->oo_dx = o; o += al256(sizeof(double) * n);
    h->oo_gamma = o; o += al256(sizeof(double) * (F > 0 ? F : 1));
    h->oo_accept = o; o += al256(sizeof(int) * (F > 0 ? F : 1));
    h->oo_Pout = o;
    h->outs_small = o;
    h->d_dx = reinterpret_cast<double*>(h->d_outs + h->oo_dx);
    h->d_gamma = reinterpret_cast<double*>(h->d_outs + h->oo_gamma);
    h->d_accept = reinterpret_cast<int*>(h->d_outs + h->oo_accept);
    h->d_Pout = reinterpret_cast<double*>(h->d_outs + h->oo_Pout);
}

// The pinned input arena is read by the device (a copy, an ingest kernel) some time after the call that filled it returns; the next
// call that wants to write it waits for the event behind that read -- not for the whole stream.
static int arena_mark_read(orcvio_msckf_handle* h, hipStream_t s) {
    if (!h->ev_arena) HIPCHK(hipEventCreateWithFlags(&h->ev_arena, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->ev_arena, s));
    h->arena_busy = true;
    return ORCVIO_OK;
}
static int arena_wait_free(orcvio_msckf_handle* h) {
    if (h->arena_busy) { HIPCHK(hipEventSynchronize(h->ev_arena)); h->arena_busy = false; }
    return ORCVIO_OK;
}

// A handful of small host arrays -> device memory without a synchronisation: each is copied into a pinned bounce buffer (one of
// a ring of four: a buffer is reused only after the event behind its last copies has fired) and from there by an asynchronous
// copy on `s`, in order with whatever the stream carries.  (The synchronous hipMemcpy of pageable memory this replaces costs
// 10-20 us per array and needs the stream drained first.)
struct AuxCopy { void* dst; const void* src; size_t bytes; };
static int aux_copies(orcvio_msckf_handle* h, hipStream_t s, const AuxCopy* c, int n) {
    size_t tot = 0;
    for (int i = 0; i < n; ++i) tot += (c[i].bytes + 63) & ~(size_t)63;
    if (tot == 0) return ORCVIO_OK;
    const int k = h->aux_next;
    h->aux_next = (k + 1) & 3;
    if (!h->ev_aux[k]) HIPCHK(hipEventCreateWithFlags(&h->ev_aux[k], hipEventDisableTiming));
    if (h->aux_busy[k]) { HIPCHK(hipEventSynchronize(h->ev_aux[k])); h->aux_busy[k] = false; }
    if (tot > h->aux_cap[k]) {
        if (h->h_aux[k]) (void)hipHostFree(h->h_aux[k]);
        h->h_aux[k] = nullptr; h->aux_cap[k] = 0;
        const size_t cap = (tot * 2 + 4095) & ~(size_t)4095;
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->h_aux[k]), cap, hipHostMallocDefault));
        h->aux_cap[k] = cap;
    }
    size_t o = 0;
    for (int i = 0; i < n; ++i) {
        if (c[i].bytes == 0) continue;
        std::memcpy(h->h_aux[k] + o, c[i].src, c[i].bytes);
        HIPCHK(hipMemcpyAsync(c[i].dst, h->h_aux[k] + o, c[i].bytes, hipMemcpyHostToDevice, s));
        o += (c[i].bytes + 63) & ~(size_t)63;
    }
    HIPCHK(hipEventRecord(h->ev_aux[k], s));
    h->aux_busy[k] = true;
    return ORCVIO_OK;
}

// The other direction: a handful of small device arrays into the caller's (pageable) memory -- asynchronous copies into ONE pinned
// block, one synchronisation of `s`, then host copies.  (A synchronous hipMemcpy to pageable memory costs 10-20 us per array.)
struct FetchCopy { void* dst; const void* src; size_t bytes; };
static int fetch_copies(orcvio_msckf_handle* h, hipStream_t s, const FetchCopy* c, int n) {
    size_t tot = 0;
    for (int i = 0; i < n; ++i) tot += (c[i].bytes + 63) & ~(size_t)63;
    if (tot > h->fetch_cap) {
        HIPCHK(hipStreamSynchronize(s));
        if (h->h_fetch) (void)hipHostFree(h->h_fetch);
        h->h_fetch = nullptr; h->fetch_cap = 0;
        const size_t cap = (tot * 2 + 4095) & ~(size_t)4095;
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->h_fetch), cap, hipHostMallocDefault));
        h->fetch_cap = cap;
    }
    size_t o = 0;
    for (int i = 0; i < n; ++i) {
        if (c[i].bytes == 0 || !c[i].dst) continue;
        HIPCHK(hipMemcpyAsync(h->h_fetch + o, c[i].src, c[i].bytes, hipMemcpyDeviceToHost, s));
        o += (c[i].bytes + 63) & ~(size_t)63;
    }
    HIPCHK(hipStreamSynchronize(s));
    o = 0;
    for (int i = 0; i < n; ++i) {
        if (c[i].bytes == 0 || !c[i].dst) continue;
        std::memcpy(c[i].dst, h->h_fetch + o, c[i].bytes);
        o += (c[i].bytes + 63) & ~(size_t)63;
    }
    return ORCVIO_OK;
}

// host-pinned (device-visible) -> HBM by a kernel instead of a copy-engine transfer: lower latency for the few hundred KB an
// update moves, and it can be a node of a captured graph like any other launch
static int launch_ingest(orcvio_msckf_handle* h, hipStream_t s, const void* src_dev, void* dst, size_t bytes,
                         int* zero = nullptr, unsigned zero_mask = 0u) {
    if (bytes == 0) return ORCVIO_OK;
    const size_t n16 = (bytes + 15) / 16;
    int grid = (int)((n16 + 255) / 256);
    if (grid > 4 * h->n_cus) grid = 4 * h->n_cus;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(k_ingest, dim3(grid), dim3(256), 0, s, reinterpret_cast<const u32x4*>(src_dev), reinterpret_cast<u32x4*>(dst), n16, zero, zero_mask);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
// Every inbound P: [lin_off, io_P) of the arena (the caller-written arrays in front of P; lin_off = io_P: P alone) and the n x n prior
// at io_P behind it -> HBM in ONE launch.  n even (ingest_sym_ok): only the upper tile-trapezoid of P crosses the link and the device
// mirrors it (k_ingest_sym; counted in orcvio_msckf_counters [10]).  n odd: rows are only 8-byte aligned -- the call takes the linear
// pull of the whole range, as before.
static int launch_ingest_P(orcvio_msckf_handle* h, hipStream_t s, size_t lin_off, int n) {
    const size_t P_bytes = sizeof(double) * (size_t)n * n;
    if (!ingest_sym_ok(n)) return launch_ingest(h, s, h->h_stage_dev + lin_off, h->d_in + lin_off, h->io_P - lin_off + P_bytes);
    const size_t lin16 = (h->io_P - lin_off) / 16;   // (the parts of the arena are 256-byte aligned: whole units, none straddles into P)
    const size_t lanes = lin16 + ingest_sym_lanes(n);
    int grid = (int)((lanes + 255) / 256);   // one round of loads covers everything, as k_ingest's grid does
    if (grid > 4 * h->n_cus) grid = 4 * h->n_cus;
    hipLaunchKernelGGL(k_ingest_sym, dim3(grid), dim3(256), 0, s, reinterpret_cast<const u32x4*>(h->h_stage_dev + lin_off),
                       reinterpret_cast<u32x4*>(h->d_in + lin_off), lin16, reinterpret_cast<const double*>(h->h_stage_dev + h->io_P),
                       reinterpret_cast<double*>(h->d_in + h->io_P), n);
    HIPCHK(hipGetLastError());
    h->cnt_sym_pulls++;
    return ORCVIO_OK;
}
// the copying calls' half of it: the caller's P -> the arena.  upper_only: the arena is read by launch_ingest_P alone, so only what
// that pull fetches is copied (the same predicate, the same row segments); otherwise (the staged upload's copy of the whole arena) all of it
static void stage_prior(orcvio_msckf_handle* h, const double* P, int n, bool upper_only) {
    double* dst = reinterpret_cast<double*>(h->h_stage + h->io_P);
    if (!upper_only || !ingest_sym_ok(n)) { std::memcpy(dst, P, sizeof(double) * (size_t)n * n); return; }
    for (int i = 0; i < n; ++i) {
        const size_t o = (size_t)i * n + ingest_sym_seg_start(i);
        std::memcpy(dst + o, P + o, sizeof(double) * (size_t)ingest_sym_seg_len(n, i));
    }
}
// ---- create / destroy ---------------------------------------------------------------------
// the pinned block of orcvio_msckf_cov_marginal_*: [result doubles [64][64] | sequence word on a line of its own]
enum { MARG_SEQ_OFFSET = sizeof(double) * MARGINAL_MAX * MARGINAL_MAX, MARG_BLOCK_BYTES = MARG_SEQ_OFFSET + 128 };
static_assert(MARGINAL_MAX == ORCVIO_MARGINAL_MAX, "the header's bound is the kernel's");
static void free_all(orcvio_msckf_handle* h) {
    (void)hipDeviceSynchronize();   // (asynchronous copies out of the pinned buffers, a commit's tail: nothing of this handle is in flight any more)
    void* ptrs[] = {h->d_in, h->d_outs,
                    h->d_chi2, h->d_Hs, h->d_Gpart, h->d_Ab, h->d_A, h->d_RP,
                    h->d_DinvP, h->d_U, h->d_M, h->d_RM, h->d_DinvM, h->d_Z, h->d_La, h->d_DinvA,
                    h->d_W, h->d_Y, h->d_KG, h->d_Gobj, h->d_RF, h->d_DinvF, h->d_Yobj, h->d_objH,
                    h->d_obj_gamma, h->d_obj_i, h->d_obj_accept, h->d_T3, h->d_Xobs, h->d_S,
                    h->d_Pres, h->d_Ptmp, h->d_Sres, h->d_Stmp, h->d_covT, h->d_covmap, h->d_imu, h->d_imu46, h->d_zchk, h->d_skip, h->d_tri_valid, h->d_tri_flags, h->d_tri_init, h->d_tri_sol, h->d_tri_cost, h->d_sync, h->d_la_rdy, h->d_U2, h->d_M2, h->d_RM2, h->d_DinvM2, h->d_Z2, h->d_outs2, h->d_chain_words, h->d_obj_done,
                    h->d_ekf_i, h->d_ekf_d, h->d_ekf_E, h->d_Gekf, h->d_ekf_gamma, h->d_ekf_accept, h->d_slam, h->d_dense, h->d_Rf, h->d_new, h->d_aug};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->h_obj_stage) (void)hipHostFree(h->h_obj_stage);
    if (h->h_lm) (void)hipHostFree(h->h_lm);
    if (h->d_lm) (void)hipFree(h->d_lm);
    if (h->h_stage2) (void)hipHostFree(h->h_stage2);
    if (h->h_tri) (void)hipHostFree(h->h_tri);
    if (h->h_imu_status) (void)hipHostFree(h->h_imu_status);
    if (h->d_tri_words) (void)hipFree(h->d_tri_words);
    if (h->h_tri2) (void)hipHostFree(h->h_tri2);
    if (h->h_cc) (void)hipHostFree(h->h_cc);
    if (h->h_marg) (void)hipHostFree(h->h_marg);
    if (h->d_margT) (void)hipFree(h->d_margT);
    for (void* q : {(void*)h->d_tri2_list, (void*)h->d_tri2_words, (void*)h->d_skip2}) if (q) (void)hipFree(q);
    if (h->d_in2) (void)hipFree(h->d_in2);
    if (h->d_step_words) (void)hipFree(h->d_step_words);
    if (h->h_evt) (void)hipHostFree(h->h_evt);
    if (h->d_evt) (void)hipFree(h->d_evt);
    for (double* q : {h->d_Hthin, h->d_Vthin, h->d_uthin}) if (q) (void)hipFree(q);
    if (h->d_obj_in) (void)hipFree(h->d_obj_in);
    for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
    if (h->h_fetch) (void)hipHostFree(h->h_fetch);
    if (h->ev_arena) (void)hipEventDestroy(h->ev_arena);
    for (int i = 0; i < 4; ++i) {
        if (h->h_aux[i]) (void)hipHostFree(h->h_aux[i]);
        if (h->ev_aux[i]) (void)hipEventDestroy(h->ev_aux[i]);
    }
    if (h->obj_stream) (void)hipStreamDestroy(h->obj_stream);
    if (h->ev_obj) (void)hipEventDestroy(h->ev_obj);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_side) (void)hipEventDestroy(h->ev_side);
    for (auto* g : {&h->g_update, &h->g_local, &h->g_finish, &h->g_io})
        for (auto& w : g->way) {
            if (w.exec) (void)hipGraphExecDestroy(w.exec);
            if (w.graph) (void)hipGraphDestroy(w.graph);
        }
    if (h->h_flag) (void)hipHostFree(h->h_flag);
    if (h->d_seq) (void)hipFree(h->d_seq);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->side) (void)hipStreamDestroy(h->side);
}

int32_t orcvio_msckf_create(int32_t device, int32_t max_clones, int32_t max_features, int32_t max_observations,
                            orcvio_msckf_handle** out) {
    if (!out || max_clones < 1 || max_clones > ORCVIO_MAX_CLONES || max_features < 1 || max_observations < 1) {
        g_last_error = "orcvio_msckf_create: invalid capacity";
        return ORCVIO_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        g_last_error = "orcvio_msckf_create: no HIP device (this library has no CPU path)";
        return ORCVIO_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        g_last_error = "hipGetDeviceProperties failed";
        return ORCVIO_ERR_NO_DEVICE;
    }
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        g_last_error = std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only";
        return ORCVIO_ERR_NO_DEVICE;
    }
    auto* h = new orcvio_msckf_handle();
    h->device = device;
    h->n_cus = prop.multiProcessorCount;
    if (const char* e = getenv("ORCVIO_LA_SPIN")) h->la_spin = atoi(e);
    if (const char* e = dbg_getenv("ORCVIO_FUSE_FINISH")) h->fuse_finish = atoi(e);
    if (const char* e = getenv("ORCVIO_FRAME_CHAIN")) h->frame_chain = atoi(e) != 0;
    if (const char* e = dbg_getenv("ORCVIO_BLK2")) h->blk2_opt = atoi(e) != 0;
    if (const char* e = dbg_getenv("ORCVIO_OBJ_FUSED")) h->obj_fused_opt = atoi(e);
    if (const char* e = getenv("ORCVIO_FRONT_SPIN")) h->front_spin_limit = atoi(e);
    if (const char* e = dbg_getenv("ORCVIO_STEP_FUSED")) h->step_fused = atoi(e) != 0;
    if (const char* e = dbg_getenv("ORCVIO_THIN_UPDATE")) h->thin_opt = atoi(e) != 0;
    if (const char* e = dbg_getenv("ORCVIO_STEP_EKF_SIDE")) h->ekf_side_opt = atoi(e) != 0;
    if (const char* e = dbg_getenv("ORCVIO_FINISH_PUB")) h->finpub_opt = atoi(e) != 0;
    if (const char* e = dbg_getenv("ORCVIO_EKF_ONE_LAUNCH")) h->ekf_one_launch = atoi(e) != 0;
    h->maxN = max_clones;
    h->maxF = max_features;
    h->maxObs = max_observations;
    h->n_max = 46 + 6 * max_clones;
    h->NAP_max = round_up(h->n_max - 15 + 1, 16);
    h->NP_max = round_up(h->n_max + 1, 16);
    if (h->NP_max > POTRF_MAXN || h->NP_max / 16 > TRSM_MAXBLK) {
        delete h;
        g_last_error = "orcvio_msckf_create: window too large for the single-workgroup factorisation";
        return ORCVIO_ERR_CAPACITY;
    }
    int rc = [&]() -> int {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_side, hipEventDisableTiming));
        const size_t nn = (size_t)h->n_max * h->n_max, pp = (size_t)h->NAP_max * h->NAP_max;
        const size_t np2 = (size_t)h->NP_max * h->NP_max;
        h->hs_rows_cap = (size_t)2 * max_observations + 16;
        {   // input / output arenas at their worst-case size, pinned mirror of both
            h->in_cap = inputs_bytes(max_clones, max_features, max_observations, true, (size_t)h->n_max);
            h->outs_cap = outputs_bytes(h->n_max, max_features);
            HIPCHK(hipMalloc(&h->d_in, h->in_cap));
            HIPCHK(hipMalloc(&h->d_outs, h->outs_cap));
            HIPCHK(hipMemset(h->d_in, 0, h->in_cap));
            h->stage_bytes = h->in_cap + h->outs_cap;
            // pinned, mapped into the device's address space, host-coherent (fine-grained): kernels read the inputs from it
            // (k_ingest) and write the results into it (k_epilogue); the copy engines can use it as before
            HIPCHK(hipHostMalloc(&h->h_stage, h->stage_bytes, hipHostMallocMapped | hipHostMallocCoherent));
            HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_stage_dev), h->h_stage, 0));
            HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->h_flag), 256, hipHostMallocMapped | hipHostMallocCoherent));
            HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_flag_dev), h->h_flag, 0));
            std::memset(h->h_flag, 0, 256);
            HIPCHK(hipMalloc(&h->d_seq, 256));
            HIPCHK(hipMemset(h->d_seq, 0, 256));
            h->d_pubcnt = reinterpret_cast<int*>(h->d_seq) + 32;   // (own 128-byte line)
            if (const char* e = getenv("ORCVIO_IO_SPIN_SECONDS")) h->io_spin_seconds = atof(e);
            layout_inputs(h, max_clones, max_features, max_observations, true, true, h->n_max);
            layout_outputs(h, h->n_max, max_features);
        }
        HIPCHK(hipMalloc(&h->d_skip, sizeof(int) * max_features));
        HIPCHK(hipMalloc(&h->d_Pres, sizeof(double) * nn));
        HIPCHK(hipMalloc(&h->d_Ptmp, sizeof(double) * nn));
        HIPCHK(hipMalloc(&h->d_Sres, sizeof(double) * np2));
        HIPCHK(hipMalloc(&h->d_Stmp, sizeof(double) * np2));
        HIPCHK(hipMalloc(&h->d_covT, sizeof(double) * (46 * (size_t)h->n_max + 2 * 46 * 46)));   // Phi P rows, then Phi and Q
        HIPCHK(hipMalloc(&h->d_covmap, sizeof(int) * h->n_max));
        // orcvio_msckf_cov_propagate_imu: the per-sample records, then the status word of k_imu_phi_q; its dynamic LDS at 128 samples
        // (105 KB) is beyond the 64 KB a kernel gets without asking.  Here, so that the call itself never allocates or synchronises
        HIPCHK(hipMalloc(&h->d_imu, sizeof(double) * ((size_t)IMU_MAX_SAMPLES * IMU_REC + 8)));
        HIPCHK(hipFuncSetAttribute((const void*)k_imu_phi_q, hipFuncAttributeMaxDynamicSharedMemorySize, (int)imu_lds_bytes(IMU_MAX_SAMPLES)));
        h->imu_recs.resize((size_t)IMU_MAX_SAMPLES * IMU_REC);
        HIPCHK(hipMemset(h->d_imu + (size_t)IMU_MAX_SAMPLES * IMU_REC, 0, 64));   // (the sixteen status words: the kernel writes [0] and [2] only)
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->h_imu_status), 64, hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_imu_status_dev), h->h_imu_status, 0));
        std::memset(h->h_imu_status, 0, 64);
        h->imu_sel.resize((size_t)IMU_MAX_SAMPLES * 7);
        // orcvio_msckf_cov_propagate_imu_calib: the wider records of leg_dim 46 and k_imu_phi_q46's dynamic LDS (a round's compact forms, 83 KB)
        HIPCHK(hipMalloc(&h->d_imu46, sizeof(double) * (size_t)IMU_MAX_SAMPLES * IMU_REC46));
        HIPCHK(hipFuncSetAttribute((const void*)k_imu_phi_q46, hipFuncAttributeMaxDynamicSharedMemorySize, (int)imu46_lds_bytes()));
        h->imu_recs46.resize((size_t)IMU_MAX_SAMPLES * IMU_REC46);
        HIPCHK(hipMalloc(&h->d_zchk, sizeof(double) * ((size_t)ZCHK_MAX_SAMPLES * ZCHK_ROW + 16)));   // k_zupt_check: rows, results, status words
        HIPCHK(hipMemset(h->d_zchk, 0, sizeof(double) * ((size_t)ZCHK_MAX_SAMPLES * ZCHK_ROW + 16)));
        // orcvio_msckf_cov_marginal_submit: the pinned result block with its sequence word, the staging of T, and k_cov_marginal's dynamic
        // LDS at 64 x 64 (97.5 KB).  Here, so that neither the submit nor the collect ever allocates
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->h_marg), MARG_BLOCK_BYTES, hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_marg_dev), h->h_marg, 0));
        std::memset(h->h_marg, 0, MARG_BLOCK_BYTES);
        HIPCHK(hipMalloc(&h->d_margT, sizeof(double) * MARGINAL_MAX * MARGINAL_MAX));
        HIPCHK(hipFuncSetAttribute((const void*)k_cov_marginal, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cov_marginal_lds_bytes(MARGINAL_MAX, MARGINAL_MAX)));
        HIPCHK(hipMalloc(&h->d_tri_valid, sizeof(int) * max_features));
        HIPCHK(hipMalloc(&h->d_tri_flags, sizeof(int) * max_features));
        HIPCHK(hipMalloc(&h->d_tri_init, sizeof(int) * max_features));
        HIPCHK(hipMalloc(&h->d_tri_sol, sizeof(double) * 3 * max_features));
        HIPCHK(hipMalloc(&h->d_tri_cost, sizeof(double) * max_features));
        HIPCHK(hipMalloc(&h->d_chi2, sizeof(double) * ORCVIO_CHI2_TABLE));
        HIPCHK(hipMalloc(&h->d_T3, sizeof(double) * (size_t)3 * max_features * h->NAP_max));
        HIPCHK(hipMalloc(&h->d_Rf, sizeof(double) * (size_t)6 * max_features));
        HIPCHK(hipMalloc(&h->d_Xobs, sizeof(double) * (size_t)32 * max_observations));
        HIPCHK(hipMalloc(&h->d_S, sizeof(double) * (size_t)256 * (2 * max_observations / 256 + max_clones + 2)));
        HIPCHK(hipMalloc(&h->d_Gpart, sizeof(double) * pp * h->gram_chunks_cap));
        HIPCHK(hipMalloc(&h->d_Ab, sizeof(double) * pp));
        HIPCHK(hipMalloc(&h->d_A, sizeof(double) * pp));
        HIPCHK(hipMalloc(&h->d_RP, sizeof(double) * np2));
        HIPCHK(hipMalloc(&h->d_DinvP, sizeof(double) * 256 * TRSM_MAXBLK));
        HIPCHK(hipMalloc(&h->d_U, sizeof(double) * np2));
        HIPCHK(hipMalloc(&h->d_M, sizeof(double) * np2));
        HIPCHK(hipMalloc(&h->d_RM, sizeof(double) * np2));
        HIPCHK(hipMalloc(&h->d_DinvM, sizeof(double) * 256 * TRSM_MAXBLK));
        HIPCHK(hipMalloc(&h->d_Z, sizeof(double) * np2));
        HIPCHK(hipMalloc(&h->d_La, sizeof(double) * pp));
        HIPCHK(hipMalloc(&h->d_DinvA, sizeof(double) * 256 * TRSM_MAXBLK));
        HIPCHK(hipMalloc(&h->d_W, sizeof(double) * np2));
        HIPCHK(hipMalloc(&h->d_Y, sizeof(double) * np2));
        HIPCHK(hipMalloc(&h->d_KG, sizeof(double) * np2));
        HIPCHK(hipMemset(h->d_info, 0, sizeof(int) * 64));   // (head of the outputs arena)
        HIPCHK(hipMalloc(&h->d_Hthin, sizeof(double) * (size_t)THIN_MAX_ROWS * h->NAP_max));
        HIPCHK(hipMalloc(&h->d_Vthin, sizeof(double) * (size_t)h->n_max * THIN_MAX_ROWS));
        HIPCHK(hipMalloc(&h->d_uthin, sizeof(double) * THIN_MAX_ROWS));
        HIPCHK(hipFuncSetAttribute((const void*)k_thin_gain, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));
        HIPCHK(hipMalloc(&h->d_sync, 256));
        HIPCHK(hipMemset(h->d_sync, 0, 256));
        HIPCHK(hipMalloc(&h->d_la_rdy, 256));
        HIPCHK(hipMemset(h->d_la_rdy, 0, 256));
        HIPCHK(hipMemset(h->d_RP, 0, sizeof(double) * np2));   // strictly-lower tiles of the upper factors stay 0
        HIPCHK(hipMemset(h->d_RM, 0, sizeof(double) * np2));
        // opt in to large dynamic LDS for the feature kernel instantiations
        const int lds_max = 160 * 1024;
        HIPCHK(hipFuncSetAttribute((const void*)k_feature<1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        HIPCHK(hipFuncSetAttribute((const void*)k_feature<2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        HIPCHK(hipFuncSetAttribute((const void*)k_feature<3>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        HIPCHK(hipFuncSetAttribute((const void*)k_feature<4>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        HIPCHK(hipFuncSetAttribute((const void*)k_feature<5>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        HIPCHK(hipFuncSetAttribute((const void*)k_feature<6>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        HIPCHK(hipFuncSetAttribute((const void*)k_feature<7>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        return ORCVIO_OK;
    }();
    if (rc != ORCVIO_OK) {
        free_all(h);
        delete h;
        return rc;
    }
    *out = h;
    return ORCVIO_OK;
}

void orcvio_msckf_destroy(orcvio_msckf_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)orcvio_msckf_comm_destroy(h);
    free_all(h);
    delete h;
}

int32_t orcvio_msckf_set_option(orcvio_msckf_handle* h, int32_t option, int32_t value) {
    if (!h) return ORCVIO_ERR_INVALID;
    if (option == ORCVIO_OPT_MATERIALIZE_STACK) {
        HIPCHK(hipSetDevice(h->device));
        if (value && !h->d_Hs) HIPCHK(hipMalloc(&h->d_Hs, sizeof(double) * h->hs_rows_cap * h->NAP_max));
        h->materialize = value != 0;
        h->graph_epoch++;
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_FUSED_SOLVE) {
        h->fused_solve = value != 0;
        h->graph_epoch++;
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_LOOKAHEAD_SOLVE) {
        if (value != 0 && value != 2 && value != 3) { g_last_error = "orcvio_msckf_set_option: ORCVIO_OPT_LOOKAHEAD_SOLVE is 0, 2 or 3"; return ORCVIO_ERR_INVALID; }
        h->la_solve = value;
        h->graph_epoch++;
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_FUSED_FRONT) {
        h->front_fused = value != 0;
        h->graph_epoch++;
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_EKF_ROWS) {
        h->ekf_mode = value != 0;   // takes effect with the next upload (part of the launch signature)
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_EXTRA_STATES) {
        if (value < 0 || 22 + 6 + value > h->n_max) { g_last_error = "orcvio_msckf_set_option: extra states out of range"; return ORCVIO_ERR_INVALID; }
        h->n_extra = value;   // takes effect with the next upload / update call (part of the launch signature)
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_RESIDENT_FACTOR) {
        h->factor_opt = value != 0;
        if (!h->factor_opt) h->fac_valid = false;
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_REF_STACK_HF) {
        h->ref_stack_hf = value != 0;
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_SCHMIDT_STATES) {
        if (value < 0 || value > h->maxN) { g_last_error = "orcvio_msckf_set_option: nuisance states out of range"; return ORCVIO_ERR_INVALID; }
        h->n_nui = value;   // takes effect with the next upload (part of the launch signature)
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_OBJECT_DOF) {
        h->obj_dof_rank = value != 0;
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_REF_H2_LDLT) {
        h->ref_h2_ldlt = value != 0;
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_OBJECT_QR) {
        h->arrow_opt = value != 0;
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_OBJECT_REFINE) {
        if (value < 0 || value > 2) { g_last_error = "orcvio_msckf_set_option: ORCVIO_OPT_OBJECT_REFINE takes 0, 1 or 2"; return ORCVIO_ERR_INVALID; }
        h->obj_refine_mode = value;
        return ORCVIO_OK;
    }
    if (option == ORCVIO_OPT_STAGE_PROFILE) {
        h->prof_on = value != 0;
        h->prof_n = 0;
        return ORCVIO_OK;
    }
    g_last_error = "orcvio_msckf_set_option: unknown option";
    return ORCVIO_ERR_INVALID;
}

static int factor_layout_clean(orcvio_msckf_handle* h);
static int launch_ekf(orcvio_msckf_handle* h, hipStream_t s);
static int io_wait(orcvio_msckf_handle* h, hipStream_t s, unsigned long long expected_pub = 0);
static int comm_stream_wait(orcvio_msckf_handle* h, hipStream_t s, const char* who);
static int ipc_check_lost(orcvio_msckf_handle* h, const char* who);
static int feature_outcome(orcvio_msckf_handle* h, const char* so, int32_t* stats);
static int run_finish_impl(orcvio_msckf_handle* h, const double* d_blocks, int n_blocks, size_t stride, const double* meta0, hipStream_t s);
static int objects_finish_impl(orcvio_msckf_handle* h, const double* d_blocks, int n_blocks, size_t stride, const double* meta0, int dof_total, hipStream_t s, UpdateCall& c);
// Gram of the rows stacked under the MSCKF rows (EKF-SLAM rows that passed their gate, caller-projected dense rows)
static inline const double* extra_gram(const orcvio_msckf_handle* h) { return (h->ekf_F > 0 || h->dense_rows > 0) ? h->d_Gekf : nullptr; }

// The prior of this update comes as P == NULL (resident covariance): if its square-root factor is resident too, the update
// uses it instead of factoring P (kf = its column count = the dimension of M).
static void select_prior_factor(orcvio_msckf_handle* h, bool with_P) {
    h->use_factor = !with_P && h->factor_opt && h->fac_valid && h->fac_n == h->n && h->res_n == h->n &&
                    round_up(h->fac_k, 16) <= POTRF_MAXN && round_up(h->fac_k, 16) / 16 <= TRSM_MAXBLK &&
                    round_up(h->fac_k, 16) <= h->NP_max;
    h->kf = h->use_factor ? h->fac_k : h->n;
}
// ... and whether the factor in use ends in columns that are zero in the active rows (call when reg_path is known)
static inline bool rev_prior_active(const orcvio_msckf_handle* h) { return h->reg_path && h->fused_solve && !h->use_factor; }
static void select_tail(orcvio_msckf_handle* h) {
    const int t = h->use_factor ? h->fac_tail : (rev_prior_active(h) ? 15 : 0);
    h->tail = (h->reg_path && h->fused_solve && t > 0 && h->kf - t >= 16) ? t : 0;
}
// L(i,j) of the prior's factor = base[i * sLi + j * sLj], i < n, j < kf
struct PriorFactor { const double* base; long sLi, sLj; };
static inline void factor_strides(const orcvio_msckf_handle* h, long& sLi, long& sLj);
static PriorFactor prior_factor(const orcvio_msckf_handle* h) {
    if (h->use_factor) return PriorFactor{h->d_Sres, 1L, (long)h->fac_ld};
    if (rev_prior_active(h)) return PriorFactor{h->d_RP + (h->n - 1), -1L, (long)h->NP};   // S(i, c) = L'(n-1-i, c) = RP[c NP + n-1-i]
    long sLi, sLj;
    factor_strides(h, sLi, sLj);
    return PriorFactor{h->d_RP, sLi, sLj};
}

// ---- what the last launch of an update publishes and commits -------------------------------------------------------------------
// The buffers one solve leaves its results in: the handle's own (solve_out), or the frame call's second context (capi_frame.inc).
struct SolveOut {
    const char* outs;         // outputs arena: [info | dx | gamma | accept | P+]
    const double* Pout;       // P+ inside it
    const double* dx;
    const int* info;          // its status words
    const double* Z; int ldz, kf;
    double sigma;
    PriorFactor prior;        // the factor a rejected or refused update keeps
};
static inline SolveOut solve_out(const orcvio_msckf_handle* h) {
    return SolveOut{h->d_outs, h->d_Pout, h->d_dx, h->d_info, h->d_Z, h->ldz, h->kf, h->flags.noise_feature, prior_factor(h)};
}
// k_epilogue's arguments: the small block (and P+ if want_P) to the pinned output block at dst_shift, the commit (0: none, 1: P+ over the
// resident covariance, 2: ... and S+ = sigma Z^T into the spare factor buffer), then the flag.  accept: the gate's word of an object update.
static EpilogueArgs epilogue_args(const orcvio_msckf_handle* h, const SolveOut& so, size_t dst_shift, bool want_P, int commit, const int* accept,
                                  const int* info_also, int* info_keep = nullptr, int pub_all = 0) {
    const int n = h->n;
    EpilogueArgs ea{};
    ea.small_src = reinterpret_cast<const u32x4*>(so.outs);
    ea.small_dst = reinterpret_cast<u32x4*>(h->h_stage_dev + h->in_cap + dst_shift);
    ea.small16 = h->outs_small / 16;
    if (want_P) {
        ea.P_src = reinterpret_cast<const u32x4*>(so.outs + h->oo_Pout);
        ea.P_dst = reinterpret_cast<u32x4*>(h->h_stage_dev + h->in_cap + dst_shift + h->oo_Pout);
        ea.P16 = (sizeof(double) * (size_t)n * n + 15) / 16;
        ea.nb_P = 40;
    }
    ea.commit = commit;
    ea.Pout = so.Pout; ea.Pres = h->d_Pres; ea.nn = (size_t)n * n;
    ea.Z = so.Z; ea.ldz = so.ldz; ea.kf = so.kf; ea.n = n; ea.sigma = so.sigma;
    ea.prior = so.prior.base; ea.sLi = so.prior.sLi; ea.sLj = so.prior.sLj; ea.Sout = h->d_Stmp; ea.ldo = so.ldz;
    ea.dx = so.dx; ea.info = so.info; ea.accept = accept;
    ea.counter = h->d_pubcnt; ea.seq = h->d_seq; ea.flag = h->h_flag_dev;
    ea.info_also = info_also; ea.info_keep = info_keep; ea.pub_all = pub_all;
    return ea;
}
static int launch_epilogue(hipStream_t s, const EpilogueArgs& ea) {
    hipLaunchKernelGGL(k_epilogue, dim3(1 + ea.nb_P + (ea.commit ? 40 : 0)), dim3(256), 0, s, ea);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
// k_finish_pub's: the finish of a feature update, its commit (P+ into the SPARE covariance buffer) and the publication in one launch
static FinishPubArgs finish_pub_args(const orcvio_msckf_handle* h, const SolveOut& so, int commit, const int* info_also) {
    FinishPubArgs fp{};
    fp.Z = so.Z; fp.ldz = so.ldz; fp.n = h->n; fp.kdim = so.kf; fp.s2 = so.sigma * so.sigma; fp.P = h->d_P; fp.dx = h->d_dx;
    fp.commit = commit;
    fp.P_dst = commit ? h->d_Ptmp : h->d_Pout;
    fp.sigma = so.sigma; fp.prior = so.prior.base; fp.sLi = so.prior.sLi; fp.sLj = so.prior.sLj; fp.Sout = h->d_Stmp; fp.ldo = so.ldz;
    fp.info = so.info; fp.info_also = info_also;
    fp.small_src = reinterpret_cast<const u32x4*>(so.outs);
    fp.small_dst = reinterpret_cast<u32x4*>(h->h_stage_dev + h->in_cap);
    fp.small16 = h->outs_small / 16;
    fp.counter = h->d_pubcnt; fp.seq = h->d_seq; fp.flag = h->h_flag_dev;
    return fp;
}
// the results of the update on `s` -> the pinned output block, then the flag (k_epilogue without a commit): what replaces
// the device-to-host copy + stream synchronisation of the one-shot calls
static int publish_enqueue(orcvio_msckf_handle* h, hipStream_t s, bool want_P) {
    const int rc = launch_epilogue(s, epilogue_args(h, solve_out(h), h->out_shift, want_P, 0, nullptr, nullptr));
    if (rc != ORCVIO_OK) return rc;
    h->pub_pending = true;
    h->pub_enqueued++;
    return ORCVIO_OK;
}
