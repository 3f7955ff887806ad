// capi_cov.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// per-kernel profile, the device-resident covariance and its square-root factor.

// ---- per-kernel profile -------------------------------------------------------------------------
int32_t orcvio_msckf_profile_update(orcvio_msckf_handle* h, void* stream, int32_t reps, const char** names, double* ms,
                                    int32_t* count) {
    if (!h || !h->uploaded || !names || !ms || !count || reps < 1) { g_last_error = "profile_update: invalid"; return ORCVIO_ERR_INVALID; }
    static const char* kn[] = {"k_feature", "k_gram", "k_assemble", "k_potrf(P)", "k_gemm(U)", "k_gemm(M)", "k_potrf(M)", "k_trsm", "k_finish"};
    const int nk = 9;
    if (*count < nk) { g_last_error = "profile_update: need room for 9 entries"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = pick_stream(h, stream);
    // One pass = the update's launches back to back on the stream, an event between two stages and no host wait inside the pass: the
    // stages see the stream as the update itself does (a host round trip per stage would add its dispatch latency to every figure).
    hipEvent_t ev[10];
    for (int k = 0; k <= nk; ++k) HIPCHK(hipEventCreate(&ev[k]));
    UpdateCall c;   // (a plain update)
    const bool front = front_fused_active(h, false);   // k_front = tracks + compression + chol(P) in one launch: reported as entry 0
    const bool defer = front_defers_assembly(h, false);
    for (int k = 0; k < nk; ++k) ms[k] = 0.0;
    std::vector<float> samples[9];   // per kernel: the MEDIAN over the repetitions is reported (one preempted launch is not the kernel's time)
    for (int r = 0; r < reps; ++r) {
        bool ran[9] = {false, false, false, false, false, false, false, false, false};
        HIPCHK(hipEventRecord(ev[0], s));
        for (int k = 0; k < nk; ++k) {
            if (!(front && k >= 1 && k <= 3)) {
                int rc = ORCVIO_OK;
                h->A_deferred = defer;
                if (k == 0) rc = front ? launch_front(h, s, c, h->d_A, defer) : launch_feature(h, s);
                else if (k == 1) rc = launch_gram(h, s);
                else if (k == 2) rc = launch_assemble(h, s, h->d_A);
                else rc = launch_solve_stage(h, s, k - 3, c);
                if (rc != ORCVIO_OK) return rc;
                ran[k] = true;
            }
            HIPCHK(hipEventRecord(ev[k + 1], s));
        }
        HIPCHK(hipEventSynchronize(ev[nk]));
        for (int k = 0; k < nk; ++k) {
            if (!ran[k]) continue;
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
            samples[k].push_back(t);
        }
    }
    // The factorisation + solve launch, the one the bench prices against the roofline, once more without an event on either side of it:
    // K x [k_gemm(M); solve] against K x [k_gemm(M)] (the product puts the launch's hand-off words back, so the pair can be repeated; M is
    // not modified by the factorisation), events around each run of K -- (T_pair - T_single) / K is the launch with ONE launch gap, as it
    // sits in the update's graph.  An event record on either side costs it 3-5 us (34-35 against the kernel trace's 30).
    if (fused_solve_active(h) && !blk2_active(h, h->kf)) {
        const int K = 10;
        std::vector<float>& d = samples[3 + ST_POTRF_M];
        d.clear();
        for (int r = 0; r < reps; ++r) {
            int rc = ORCVIO_OK;
            HIPCHK(hipEventRecord(ev[0], s));
            for (int q = 0; q < K && rc == ORCVIO_OK; ++q) {
                rc = launch_solve_stage(h, s, ST_FORM_M, c);
                if (rc == ORCVIO_OK) rc = launch_solve_stage(h, s, ST_POTRF_M, c);
            }
            HIPCHK(hipEventRecord(ev[1], s));
            for (int q = 0; q < K && rc == ORCVIO_OK; ++q) rc = launch_solve_stage(h, s, ST_FORM_M, c);
            HIPCHK(hipEventRecord(ev[2], s));
            HIPCHK(hipEventSynchronize(ev[2]));
            if (rc != ORCVIO_OK) return rc;
            float tp = 0.f, ts = 0.f;
            HIPCHK(hipEventElapsedTime(&tp, ev[0], ev[1]));
            HIPCHK(hipEventElapsedTime(&ts, ev[1], ev[2]));
            d.push_back((tp - ts) / K);
        }
    }
    for (int k = 0; k < nk; ++k)
        if (!samples[k].empty()) {
            std::sort(samples[k].begin(), samples[k].end());
            const size_t m = samples[k].size();
            ms[k] = (m & 1) ? samples[k][m / 2] : 0.5 * (samples[k][m / 2 - 1] + samples[k][m / 2]);
        }
    int no = 0;
    for (int k = 0; k < nk; ++k) {
        if (k == 3 + ST_TRSM && fused_solve_active(h)) continue;   // nothing launched: part of k_potrf_solve(M)
        if (k == 3 + ST_FINISH && finish_fused_active(h, c)) continue;   // nothing launched: part of k_potrf_solve_la(M) (LaFin)
        if (front && k >= 1 && k <= 3) continue;                   // part of k_front
        ms[no] = ms[k];
        names[no] = (k == 3 + ST_POTRF_M && fused_solve_active(h))
                        ? (la_solve_active(h, (h->kf - h->tail + 15) / 16, false) ? "k_potrf_solve_la(M)" : "k_potrf_solve(M)")
                        : ((front && k == 0) ? "k_front" : kn[k]);
        ++no;
    }
    *count = no;
    for (int k = 0; k <= nk; ++k) (void)hipEventDestroy(ev[k]);
    HIPCHK(hipMemsetAsync(h->d_info, 0, sizeof(int) * 8, s));
    HIPCHK(hipStreamSynchronize(s));
    h->ran = true;
    return ORCVIO_OK;
}

// ---- device-resident covariance (SURVEY.md 8f rank 2) --------------------------------------------------
int32_t orcvio_msckf_cov_set(orcvio_msckf_handle* h, int32_t n, const double* P) {
    if (!h || !P || n < 1 || n > h->n_max) { g_last_error = "cov_set: invalid"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));   // (a commit may still be writing the resident covariance: the flag of an in-place
                                               //  update rises when its RESULTS are out, not when its commit workgroups are done)
    HIPCHK(hipMemcpy(h->d_Pres, P, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice));
    h->set(n);
    return ORCVIO_OK;
}

// ---- the launches of an edit, ONE per kernel family: what to read and write comes in the record the edit's bookkeeping left
// (CovBook, host/cov_book.hpp); Phi and Q are device pointers, their staging stays with the caller
// refuse: a device word behind which Phi / Q are not to be applied (orcvio_msckf_cov_propagate_imu), or nullptr
static int launch_cov_propagate(orcvio_msckf_handle* h, hipStream_t s, const CovEdit& e, int leg, const double* dPhi, const double* dQ,
                                const int* refuse = nullptr) {
    hipLaunchKernelGGL(k_cov_propagate_rows, dim3((leg * e.n + 255) / 256), dim3(256), 0, s, e.P, e.n, dPhi, leg, h->d_covT);
    hipLaunchKernelGGL(k_cov_propagate_finish, dim3((e.n * e.n + 255) / 256), dim3(256), 0, s, e.P, e.n, dPhi, dQ, leg, (const double*)h->d_covT, e.Pout, refuse);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
// the new clone goes in at `pose`: BEHIND the clones and IN FRONT of the feature / nuisance states (rest_rows, src/orcvio.cpp:976-1003)
static int launch_cov_augment(orcvio_msckf_handle*, hipStream_t s, const CovEdit& e, int pose) {
    hipLaunchKernelGGL(k_cov_augment, dim3((e.m * e.m + 255) / 256), dim3(256), 0, s, e.P, e.n, pose, e.Pout);
    if (e.fac) hipLaunchKernelGGL(k_fac_augment, dim3((e.fac_k * e.m + 255) / 256), dim3(256), 0, s, e.S, e.ld_in, e.fac_k, e.n, pose, e.Sout, e.ld_out);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
// new state i <- old state map[i], i < e.m (states removed, or a permutation): rows of S with it.  The map travels through the pinned
// bounce buffer: nothing to wait for, and it may be a local of the caller (aux_copies has copied it when it returns)
static int launch_cov_gather(orcvio_msckf_handle* h, hipStream_t s, const CovEdit& e, const std::vector<int>& map) {
    const AuxCopy cp[] = {{h->d_covmap, map.data(), sizeof(int) * map.size()}};
    const int rc = aux_copies(h, s, cp, 1);
    if (rc != ORCVIO_OK) return rc;
    hipLaunchKernelGGL(k_cov_remove, dim3((e.m * e.m + 255) / 256), dim3(256), 0, s, e.P, e.n, (const int*)h->d_covmap, e.m, e.Pout);   // (m = map.size())
    if (e.fac) hipLaunchKernelGGL(k_fac_remove, dim3((e.fac_k * e.m + 255) / 256), dim3(256), 0, s, e.S, e.ld_in, e.fac_k, (const int*)h->d_covmap, e.m, e.Sout, e.ld_out);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}
struct AnchorLaunch {   // k_cov_change_anchors' inputs besides the covariance
    int idp, literal_3d, if_fej, count, base, leg;
    const double* poses; const double* ext; const int* chg_i; const double* chg_d;
    double* par;
};
// Y = J P [k d][n] goes to the spare covariance buffer (n_max^2 >= k d n: k d <= n - base), overwritten as a whole by whatever writes it next
static int launch_cov_change_anchors(orcvio_msckf_handle*, hipStream_t s, const CovEdit& e, const AnchorLaunch& a, const AnchorFrameArgs& fr) {
    const auto kernel = a.idp == 3 ? k_cov_change_anchors<3> : k_cov_change_anchors<1>;
    const int threads = a.idp == 3 ? AnchorThreads<3>::value : AnchorThreads<1>::value;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(threads), 0, s, const_cast<double*>(e.P), e.n, e.fac ? const_cast<double*>(e.S) : (double*)nullptr, e.ld_in, e.fac_k,
                       a.poses, a.ext, a.chg_i, a.chg_d, a.count, a.base, a.leg, a.if_fej, a.literal_3d, a.par, e.Pout, fr);
    HIPCHK(hipGetLastError());
    return ORCVIO_OK;
}

int32_t orcvio_msckf_cov_get(orcvio_msckf_handle* h, int32_t* n_out, double* P_out) {
    if (!h || h->res_n == 0) { g_last_error = "cov_get: no resident covariance"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    if (n_out) *n_out = h->res_n;
    if (P_out) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(P_out, h->d_Pres, sizeof(double) * (size_t)h->res_n * h->res_n, hipMemcpyDeviceToHost));
    }
    return ORCVIO_OK;
}

// ---- marginals of the resident covariance without fetching all of P (k_cov_marginal, cov_marginal_ops.hpp) ------------------------
// The launch goes onto the handle's stream where cov_get's copy would go: it sees what the last cov_* call, commit or frame call left
// (a frame call's marginalisation that is enqueued and not waited for included) and changes nothing resident -- not P, not the
// factor, not the bookkeeping, no arming, not the open arena.  Everything is validated before anything is enqueued
// (host/cov_marginal_spec.hpp).
int32_t orcvio_msckf_cov_marginal_submit(orcvio_msckf_handle* h, const orcvio_msckf_marginal* q) {
    const char* who = "cov_marginal_submit: ";
    if (!h || !q) { g_last_error = std::string(who) + "null argument"; return ORCVIO_ERR_INVALID; }
    if (h->comm || h->ipc) { g_last_error = std::string(who) + "not with a communicator on the handle"; return ORCVIO_ERR_INVALID; }
    if (h->marg_submitted) { g_last_error = std::string(who) + "the previous submit has not been collected"; return ORCVIO_ERR_INVALID; }
    if (const char* why = marginal_refusal(q->n_idx, q->idx, q->m, q->T, h->res_n)) { g_last_error = std::string(who) + why; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int k = q->n_idx, m = q->m;
    if (m > 0) {   // T is caller memory: through the pinned bounce buffer, nothing to wait for
        const AuxCopy cp[] = {{h->d_margT, q->T, sizeof(double) * (size_t)m * k}};
        const int rc = aux_copies(h, s, cp, 1);
        if (rc != ORCVIO_OK) return rc;
    }
    CovMarginalArgs a{};
    a.P = h->d_Pres; a.n = h->res_n; a.k = k; a.m = m; a.T = h->d_margT;
    a.out = reinterpret_cast<double*>(h->h_marg_dev);
    a.out_seq = reinterpret_cast<unsigned long long*>(h->h_marg_dev + MARG_SEQ_OFFSET); a.seq = h->marg_seq + 1;
    for (int i = 0; i < k; ++i) a.idx.v[i] = q->idx[i];
    hipLaunchKernelGGL(k_cov_marginal, dim3(1), dim3(COV_MARGINAL_THREADS), m > 0 ? cov_marginal_lds_bytes(k, m) : 0, s, a);
    HIPCHK(hipGetLastError());
    h->marg_seq = a.seq;
    h->marg_submitted = true;
    h->marg_rows = m > 0 ? m : k;
    return ORCVIO_OK;
}

// The wait of io_wait on the block's own word: a bounded spin, then a stream synchronisation, then ORCVIO_ERR_TIMEOUT.  No copy by the
// runtime and no pageable memory on the way: the kernel stored into the pinned block, the host copies out of it.
int32_t orcvio_msckf_cov_marginal_collect(orcvio_msckf_handle* h, double* out, int32_t* rows) {
    const char* who = "cov_marginal_collect: ";
    if (!h || !out) { g_last_error = std::string(who) + "null argument"; return ORCVIO_ERR_INVALID; }
    if (!h->marg_submitted) { g_last_error = std::string(who) + "nothing has been submitted"; return ORCVIO_ERR_INVALID; }
    const unsigned long long* seq = reinterpret_cast<const unsigned long long*>(h->h_marg + MARG_SEQ_OFFSET);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (__atomic_load_n(seq, __ATOMIC_ACQUIRE) < h->marg_seq) {
        _mm_pause();
        if ((++spins & 4095u) == 0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > h->io_spin_seconds) break;
    }
    h->marg_submitted = false;   // (whatever comes of it: the request is spent)
    if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) < h->marg_seq) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) < h->marg_seq) { g_last_error = std::string(who) + "the result was not published"; return ORCVIO_ERR_TIMEOUT; }
    }
    const int r = h->marg_rows;
    std::memcpy(out, h->h_marg, sizeof(double) * (size_t)r * r);
    if (rows) *rows = r;
    return ORCVIO_OK;
}

int32_t orcvio_msckf_cov_get_marginal(orcvio_msckf_handle* h, const orcvio_msckf_marginal* q, double* out) {
    if (!h || !q || !out) { g_last_error = "cov_get_marginal: null argument"; return ORCVIO_ERR_INVALID; }
    const int rc = orcvio_msckf_cov_marginal_submit(h, q);
    return rc != ORCVIO_OK ? rc : orcvio_msckf_cov_marginal_collect(h, out, nullptr);
}

int32_t orcvio_msckf_cov_propagate(orcvio_msckf_handle* h, int32_t leg, const double* Phi, const double* Q) {
    if (!h || !Phi || !Q || (leg != 22 && leg != 46) || h->res_n < leg) { g_last_error = "cov_propagate: invalid"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    double* dPhi = h->d_covT + (size_t)46 * h->n_max;   // behind the Phi P rows: Phi, then Q
    double* dQ = dPhi + 46 * 46;
    {   // Phi and Q are caller memory: through the pinned bounce buffer, so that nothing has to be waited for
        const AuxCopy cp[] = {{dPhi, Phi, sizeof(double) * (size_t)leg * leg}, {dQ, Q, sizeof(double) * (size_t)leg * leg}};
        const int rc = aux_copies(h, s, cp, 2);
        if (rc != ORCVIO_OK) return rc;
    }
    return launch_cov_propagate(h, s, h->propagate(), leg, dPhi, dQ);
}

int32_t orcvio_msckf_cov_augment(orcvio_msckf_handle* h) {
    if (!h || h->res_n < 9 || h->res_n + 6 > h->n_max) { g_last_error = "cov_augment: no resident covariance, or window full"; return ORCVIO_ERR_CAPACITY; }
    HIPCHK(hipSetDevice(h->device));
    const int n = h->res_n;
    if (h->n_extra > n - 15) { g_last_error = "cov_augment: more extra states than the resident covariance has"; return ORCVIO_ERR_INVALID; }
    return launch_cov_augment(h, h->stream, h->augment(), n - h->n_extra);
}

// The states in `map` (ascending) stay in the resident covariance, the others leave (rows and columns deleted); deleting states
// deletes rows of the resident square-root factor, which is kept.
static int cov_keep_states(orcvio_msckf_handle* h, const std::vector<int>& map) {
    return launch_cov_gather(h, h->stream, h->gather((int)map.size()), map);
}
// the states that stay when the d rows of the listed in-state features (slots ascending, the features begin at `base`) leave a state of n
static std::vector<int> lost_features_map(int n, int base, int d, const int32_t* slots, int count) {
    std::vector<int> map;
    int q = 0;
    for (int i = 0; i < n; ++i) {
        while (q < count && base + d * (slots[q] + 1) <= i) ++q;
        if (q == count || i < base + d * slots[q]) map.push_back(i);
    }
    return map;
}

int32_t orcvio_msckf_cov_remove_clones(orcvio_msckf_handle* h, int32_t leg, const int32_t* idx, int32_t count) {
    if (!h || (count > 0 && !idx) || count < 0 || (leg != 22 && leg != 46) || h->res_n < leg) { g_last_error = "cov_remove_clones: invalid"; return ORCVIO_ERR_INVALID; }
    if (count == 0) return ORCVIO_OK;
    HIPCHK(hipSetDevice(h->device));
    const int n = h->res_n, N = (n - leg) / 6;
    std::vector<char> drop(n, 0);
    for (int k = 0; k < count; ++k) {
        if (idx[k] < 0 || idx[k] >= N) { g_last_error = "cov_remove_clones: index out of the window"; return ORCVIO_ERR_INVALID; }
        for (int c = 0; c < 6; ++c) drop[leg + 6 * idx[k] + c] = 1;
    }
    std::vector<int> map;
    for (int i = 0; i < n; ++i)
        if (!drop[i]) map.push_back(i);
    return cov_keep_states(h, map);
}

// Schmidt branch of pruneImuStateBuffer (src/orcvio.cpp:2881-2920): the listed clones leave the window but STAY in the covariance
// as nuisance states -- their 6 x 6 blocks and cross terms move to the end, one clone after the other in the listed order.
// A symmetric permutation: rows of the resident square-root factor move with it.
int32_t orcvio_msckf_cov_clones_to_nuisance(orcvio_msckf_handle* h, int32_t leg, const int32_t* idx, int32_t count) {
    if (!h || (count > 0 && !idx) || count < 0 || (leg != 22 && leg != 46) || h->res_n < leg) { g_last_error = "cov_clones_to_nuisance: invalid"; return ORCVIO_ERR_INVALID; }
    if (count == 0) return ORCVIO_OK;
    HIPCHK(hipSetDevice(h->device));
    const int n = h->res_n;
    std::vector<int> map(n);
    for (int i = 0; i < n; ++i) map[i] = i;
    std::vector<int> moved_before;   // window ranks are those BEFORE any of the listed clones has moved (ascending, as rm_imu_state_ids)
    for (int k = 0; k < count; ++k) {
        int shift = 0;
        for (int q : moved_before) if (q < idx[k]) ++shift;
        const int start = leg + 6 * (idx[k] - shift);
        if (idx[k] < 0 || start + 6 > n) { g_last_error = "cov_clones_to_nuisance: index out of the window"; return ORCVIO_ERR_INVALID; }
        std::rotate(map.begin() + start, map.begin() + start + 6, map.end());   // the block goes to the end, everything behind it moves up
        moved_before.push_back(idx[k]);
    }
    return launch_cov_gather(h, h->stream, h->permute(), map);
}

// rmLostFeaturesCov (src/orcvio.cpp:3776-3828) on the resident covariance: the d rows and columns of the listed in-state features
// (slots in feature_states before the call, ascending) are deleted; the nuisance block behind the features stays.  A gather with
// a map (k_cov_remove), the factor's rows with it (k_fac_remove): the factor is kept.
int32_t orcvio_msckf_cov_remove_features(orcvio_msckf_handle* h, int32_t leg, int32_t n_clones, int32_t idp_dim, int32_t n_feature_states,
                                         const int32_t* slots, int32_t count) {
    if (!h || (count > 0 && !slots) || count < 0 || (leg != 22 && leg != 46) || (idp_dim != 1 && idp_dim != 3) || n_clones < 0 ||
        n_feature_states < 0 || count > n_feature_states) { g_last_error = "cov_remove_features: invalid"; return ORCVIO_ERR_INVALID; }
    const int n = h->res_n, base = leg + 6 * n_clones, end = base + idp_dim * n_feature_states;
    if (n == 0 || end > n || (n - end) % 6 != 0) { g_last_error = "cov_remove_features: leg + 6N + d nf does not fit the resident covariance, or what is behind it is not whole nuisance blocks"; return ORCVIO_ERR_INVALID; }
    for (int q = 0; q < count; ++q)
        if (slots[q] < 0 || slots[q] >= n_feature_states || (q > 0 && slots[q] <= slots[q - 1])) { g_last_error = "cov_remove_features: slots must be ascending and in range"; return ORCVIO_ERR_INVALID; }
    if (count == 0) return ORCVIO_OK;
    HIPCHK(hipSetDevice(h->device));
    return cov_keep_states(h, lost_features_map(n, base, idp_dim, slots, count));
}

// The in-state branch of pruneImuStateBuffer (src/orcvio.cpp:2664-2720) for up to 16 features at once: new parameters in the new
// anchor's camera frame and P <- T P T^T (updateFeatureCov_1didp :3611-3774 / _3didp :3457-3609), in one launch
// (k_cov_change_anchors); the resident factor goes along as S <- T S.
static bool all_finite(const double* x, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return false;
    return true;
}
// one change as k_cov_change_anchors reads it: ci [4] slot | old anchor | new anchor | rec (the frame call: the feature's slam_features
// record), cd [6] p_w | p_fej (p_w again without FEJ); the 12 doubles of the extrinsics R_b2c | t_c_b
static inline void pack_anchor_change(const orcvio_msckf_anchor_change& c, bool if_fej, int rec, int* ci, double* cd) {
    ci[0] = c.slot; ci[1] = c.old_anchor; ci[2] = c.new_anchor; ci[3] = rec;
    for (int a = 0; a < 3; ++a) { cd[a] = c.p_w[a]; cd[3 + a] = if_fej ? c.p_fej[a] : c.p_w[a]; }
}
static inline void pack_extrinsics(const double* R_b2c, const double* t_c_b, double* ext) {
    for (int a = 0; a < 9; ++a) ext[a] = R_b2c[a];
    for (int a = 0; a < 3; ++a) ext[9 + a] = t_c_b[a];
}
int32_t orcvio_msckf_cov_change_anchors(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int32_t idp_dim, int32_t literal_3d,
                                        int32_t n_clones, const double* poses, const double* R_b2c, const double* t_c_b,
                                        const orcvio_msckf_anchor_change* changes, int32_t count, double* new_param, double* new_inv_depth) {
    if (!h || !flags || (idp_dim != 1 && idp_dim != 3) || count < 0 || count > ANCHOR_MAX_K || (count > 0 && (!changes || !poses || !R_b2c || !t_c_b)) ||
        (flags->leg_dim != 22 && flags->leg_dim != 46) || n_clones < 2) { g_last_error = "cov_change_anchors: invalid"; return ORCVIO_ERR_INVALID; }
    const int n = h->res_n, leg = flags->leg_dim, base = leg + 6 * n_clones, d = idp_dim;
    if (n == 0 || base > n) { g_last_error = "cov_change_anchors: the window does not fit the resident covariance"; return ORCVIO_ERR_INVALID; }
    // the feature states end where the nuisance block of ORCVIO_OPT_SCHMIDT_STATES begins: a slot may not reach into it
    const int feat_end = n - 6 * h->n_nui;
    if (feat_end < base || (feat_end - base) % d != 0) { g_last_error = "cov_change_anchors: the states behind the clones are not d-wide feature states followed by the ORCVIO_OPT_SCHMIDT_STATES nuisance block"; return ORCVIO_ERR_INVALID; }
    if (count == 0) return ORCVIO_OK;
    std::vector<int> ci(ANCHOR_CHG_STRIDE * count, 0);
    std::vector<double> cd(6 * count);
    for (int q = 0; q < count; ++q) {
        const orcvio_msckf_anchor_change& c = changes[q];
        if (c.slot < 0 || base + d * (c.slot + 1) > feat_end) { g_last_error = "cov_change_anchors: slot out of range"; return ORCVIO_ERR_INVALID; }
        for (int p = 0; p < q; ++p)
            if (changes[p].slot == c.slot) { g_last_error = "cov_change_anchors: a slot listed twice"; return ORCVIO_ERR_INVALID; }
        if (c.old_anchor < 0 || c.old_anchor >= n_clones || c.new_anchor < 0 || c.new_anchor >= n_clones) { g_last_error = "cov_change_anchors: anchor outside the window"; return ORCVIO_ERR_INVALID; }
        if (c.old_anchor == c.new_anchor) { g_last_error = "cov_change_anchors: old anchor == new anchor"; return ORCVIO_ERR_INVALID; }
        if (!all_finite(c.p_w, 3) || (flags->if_fej && !all_finite(c.p_fej, 3))) { g_last_error = "cov_change_anchors: non-finite feature position"; return ORCVIO_ERR_INVALID; }
        pack_anchor_change(c, flags->if_fej != 0, 0, &ci[ANCHOR_CHG_STRIDE * q], &cd[6 * q]);
    }
    double ext[12];
    pack_extrinsics(R_b2c, t_c_b, ext);
    if (!all_finite(ext, 12)) { g_last_error = "cov_change_anchors: non-finite extrinsics"; return ORCVIO_ERR_INVALID; }
    for (int i = 0; i < n_clones; ++i)
        if (!all_finite(poses + (size_t)i * ORCVIO_POSE_STRIDE, 27)) { g_last_error = "cov_change_anchors: non-finite pose record"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    // staging in the propagation scratch (46 n_max + 2 46^2 doubles >= 28 N + 12 + 10 k): poses | ext | p_w, p_fej | params out
    double* dposes = h->d_covT;
    double* dext = dposes + (size_t)ORCVIO_POSE_STRIDE * n_clones;
    double* dcd = dext + 12;
    double* dpar = dcd + 6 * count;
    {
        const AuxCopy cp[] = {{dposes, poses, sizeof(double) * (size_t)ORCVIO_POSE_STRIDE * n_clones}, {dext, ext, sizeof(ext)},
                              {dcd, cd.data(), sizeof(double) * cd.size()}, {h->d_covmap, ci.data(), sizeof(int) * ci.size()}};
        const int rc = aux_copies(h, s, cp, 4);
        if (rc != ORCVIO_OK) return rc;
    }
    {
        const AnchorLaunch a{d, literal_3d ? 1 : 0, flags->if_fej ? 1 : 0, count, base, leg, dposes, dext, h->d_covmap, dcd, dpar};
        const int rc = launch_cov_change_anchors(h, s, h->change_anchors(), a, AnchorFrameArgs{});
        if (rc != ORCVIO_OK) return rc;
    }
    std::vector<double> par(4 * count);
    const FetchCopy fc[] = {{par.data(), dpar, sizeof(double) * par.size()}};
    const int rc = fetch_copies(h, s, fc, 1);
    if (rc != ORCVIO_OK) return rc;
    for (int q = 0; q < count; ++q) {
        if (new_param)
            for (int a = 0; a < 3; ++a) new_param[3 * q + a] = par[4 * q + a];
        if (new_inv_depth) new_inv_depth[q] = par[4 * q + 3];
    }
    return ORCVIO_OK;
}

int32_t orcvio_msckf_cov_commit(orcvio_msckf_handle* h) {
    if (!h || !h->ran) { g_last_error = "cov_commit: no finished update"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->last_stream ? h->last_stream : h->stream;
    const int n = h->n, kf = h->kf;
    // the rule of commit_bookkeeping (a Schmidt update and the direct form of a thin stack leave no factor), with P+ copied into the
    // resident buffer instead of written into the spare one, and S+ made by a launch of its own
    const FacAfter fa = update_fac_after(h);
    if (fa == FacAfter::adopt) {   // S+ = sigma Z^T (or the prior's own factor if a gated object update was rejected): read before Pres changes
        const PriorFactor pf = prior_factor(h);
        hipLaunchKernelGGL(k_fac_commit, dim3((kf * n + 255) / 256), dim3(256), 0, s, h->d_Z, h->ldz, kf, n, h->flags.noise_feature,
                           h->last_update_objects ? h->d_obj_accept : (const int*)nullptr, pf.base, pf.sLi, pf.sLj, h->d_Stmp, h->ldz,
                           (const int*)(h->d_info + 2));
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(h->d_Pres, h->d_Pout, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToDevice, s));
    if (s != h->stream) HIPCHK(hipStreamSynchronize(s));   // the other cov_* calls run on the handle's own stream
    h->commit_update(n, kf, h->ldz, h->tail, false, fa);
    return ORCVIO_OK;
}

// The tail of measurementUpdate_hybrid on the device (src/orcvio.cpp:1818-1821, :1904-1947): after an update that carried entering
// features (orcvio_msckf_upload_new_features), the resident covariance becomes the AUGMENTED one -- P+ of the update with the d k
// new feature states behind it (in front of the nuisance block under ORCVIO_OPT_SCHMIDT_STATES, :1920-1935) -- from the blocks
// H_1, H_2, r_1 that are still on the device; dx_new [d k] comes back.  Replaces cov_commit + cov_get + augment_state + cov_set for a
// caller that keeps the covariance in HBM.  The caller raises ORCVIO_OPT_EXTRA_STATES by d k for its next upload.
int32_t orcvio_msckf_cov_commit_new_features(orcvio_msckf_handle* h, double* dx_new) {
    if (!h || !h->ran || h->new_F <= 0 || !dx_new) { g_last_error = "cov_commit_new_features: no finished update with entering features"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    const int n = h->n, k = h->new_F, d = h->new_idp, sz = d * k, nt = n + sz, tail = 6 * h->n_nui;
    if (nt > h->n_max) { g_last_error = "cov_commit_new_features: the augmented state exceeds the handle's capacity"; return ORCVIO_ERR_CAPACITY; }
    hipStream_t s = h->last_stream ? h->last_stream : h->stream;
    // scratch behind the blocks: HH [sz][n + 1] | W [k][d][d] | nHHP [sz][n] | Q [sz][sz] | dx_new [sz] | flag
    const size_t need = ((size_t)sz * (n + 1) + (size_t)k * d * d + (size_t)sz * n + (size_t)sz * sz + sz + 2) * sizeof(double);
    if (need > h->aug_cap) {
        HIPCHK(hipDeviceSynchronize());
        if (h->d_aug) (void)hipFree(h->d_aug);
        HIPCHK(hipMalloc(&h->d_aug, need * 2));
        h->aug_cap = need * 2;
    }
    double* HH = reinterpret_cast<double*>(h->d_aug);
    double* W = HH + (size_t)sz * (n + 1);
    double* nHHP = W + (size_t)k * d * d;
    double* Q = nHHP + (size_t)sz * n;
    double* dxn = Q + (size_t)sz * sz;
    int* flag = reinterpret_cast<int*>(dxn + sz);
    const double* dout = reinterpret_cast<const double*>(h->d_new + h->new_out_off);
    const double* H1 = dout; const double* H2 = dout + (size_t)sz * n; const double* r1 = H2 + (size_t)k * d * d;
    const double s2 = h->flags.noise_feature * h->flags.noise_feature;
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_aug_hh, dim3((n + 1 + 255) / 256, k), dim3(256), 0, s, H1, H2, r1, n, k, d, HH, W, flag, h->ref_h2_ldlt ? 1 : 0);
    hipLaunchKernelGGL(k_aug_dx, dim3(sz), dim3(64), 0, s, (const double*)HH, n, (const double*)h->d_dx, dxn);
    int rc = launch_gemm(s, HH, (long)(n + 1), 1L, h->d_Pout, (long)n, 1L, sz, n, n, -1.0, 0.0, 0, nHHP, (long)n, 1L);                 // nHHP = -HH P+
    if (rc == ORCVIO_OK) rc = launch_gemm(s, nHHP, (long)n, 1L, HH, 1L, (long)(n + 1), sz, sz, n, 1.0, 0.0, 0, Q, (long)sz, 1L);       // Q = nHHP HH^T
    if (rc != ORCVIO_OK) return rc;
    hipLaunchKernelGGL(k_aug_assemble, dim3((nt * nt + 255) / 256), dim3(256), 0, s, (const double*)h->d_Pout, n, sz, tail, d, (const double*)nHHP,
                       (const double*)Q, (const double*)W, s2, h->d_Ptmp);
    HIPCHK(hipGetLastError());
    int bad = 0;
    HIPCHK(hipMemcpyAsync(dx_new, dxn, sizeof(double) * sz, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad) { g_last_error = "cov_commit_new_features: singular H_2"; return ORCVIO_ERR_NOT_SPD; }
    h->commit_new_features(nt);   // (the factor of the augmented covariance would have d k more columns: not kept)
    h->new_F = 0;
    return ORCVIO_OK;
}

// The same tail with the resident square-root factor CARRIED ALONG (cov_ops.hpp, k_aug_rows / k_aug_finish): two launches, no
// memset, dx_new and the singular word in one fetch behind one wait.  The factor follows exactly when the update's own commit
// would adopt S+ = sigma Z^T (update_fac_after) and the widened factor fits the factor buffers; otherwise it is dropped, as the
// call above drops it.  Preconditions, refusals and dx_new are that call's.
int32_t orcvio_msckf_cov_commit_new_features_fac(orcvio_msckf_handle* h, double* dx_new) {
    if (!h || !h->ran || h->new_F <= 0 || !dx_new) { g_last_error = "cov_commit_new_features_fac: no finished update with entering features"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    const int n = h->n, k = h->new_F, d = h->new_idp, sz = d * k, nt = n + sz, tail = 6 * h->n_nui, kf = h->kf;
    if (nt > h->n_max) { g_last_error = "cov_commit_new_features_fac: the augmented state exceeds the handle's capacity"; return ORCVIO_ERR_CAPACITY; }
    if (d != 1 && d != 3) { g_last_error = "cov_commit_new_features_fac: feature states are 1 or 3 wide"; return ORCVIO_ERR_INVALID; }
    const size_t lds = aug_rows_lds_bytes(n, d);
    if (lds > (size_t)64 * 1024) { g_last_error = "cov_commit_new_features_fac: state too wide for a workgroup's LDS"; return ORCVIO_ERR_CAPACITY; }
    hipStream_t s = h->last_stream ? h->last_stream : h->stream;
    const bool follows = CovBook::new_features_fac_follows(update_fac_after(h), kf, sz, h->NP_max);
    // scratch: HH [sz][n + 1] | nHHP [sz][n] | dx_new [sz] | singular word (the last two contiguous: ONE fetch)
    const size_t need = ((size_t)sz * (n + 1) + (size_t)sz * n + sz + 1) * sizeof(double);
    if (need > h->aug_cap) {
        HIPCHK(hipDeviceSynchronize());
        if (h->d_aug) (void)hipFree(h->d_aug);
        h->d_aug = nullptr; h->aug_cap = 0;
        HIPCHK(hipMalloc(&h->d_aug, need * 2));
        h->aug_cap = need * 2;
    }
    double* HH = reinterpret_cast<double*>(h->d_aug);
    double* nHHP = HH + (size_t)sz * (n + 1);
    double* dxn = nHHP + (size_t)sz * n;
    int* flag = reinterpret_cast<int*>(dxn + sz);
    const double* dout = reinterpret_cast<const double*>(h->d_new + h->new_out_off);
    const double* H1 = dout; const double* H2 = dout + (size_t)sz * n; const double* r1 = H2 + (size_t)k * d * d;
    const double sigma = h->flags.noise_feature;
    AugFacArgs f{};
    if (follows) {   // S+ as k_fac_commit writes it (orcvio_msckf_cov_commit), into the spare factor buffer with the augmented state's leading dimension
        const PriorFactor pf = prior_factor(h);
        f.on = 1; f.Z = h->d_Z; f.ldz = h->ldz; f.kf = kf; f.sigma = sigma;
        f.apply = h->last_update_objects ? h->d_obj_accept : (const int*)nullptr; f.fail = h->d_info + 2;
        f.prior = pf.base; f.sLi = pf.sLi; f.sLj = pf.sLj;
        f.Sout = h->d_Stmp; f.ldo = CovBook::ld_for(nt);
    }
    const int nb_P = (nt * nt + 255) / 256, nb_S = follows ? ((kf + sz) * f.ldo + 255) / 256 : 0, nb_Q = (sz * (sz + 1) / 2 + 3) / 4;
#define LAUNCH_AUG(D)                                                                                                                   \
    do {                                                                                                                                \
        hipLaunchKernelGGL(k_aug_rows<D>, dim3(sz, aug_rows_split(n, follows ? kf : 0)), dim3(AUG_ROWS_THREADS), lds, s, H1, H2, r1, n, k, h->ref_h2_ldlt ? 1 : 0, \
                           (const double*)h->d_Pout, (const double*)h->d_dx, HH, nHHP, dxn, flag, f);                                   \
        hipLaunchKernelGGL(k_aug_finish<D>, dim3(nb_P + nb_S + nb_Q), dim3(256), 0, s, (const double*)h->d_Pout, n, sz, tail, H2,       \
                           (const double*)HH, (const double*)nHHP, sigma * sigma, h->d_Ptmp, nb_P, nb_S, f);                            \
    } while (0)
    if (d == 3) LAUNCH_AUG(3); else LAUNCH_AUG(1);
#undef LAUNCH_AUG
    HIPCHK(hipGetLastError());
    std::vector<double> back((size_t)sz + 1, 0.0);
    const FetchCopy fc[] = {{back.data(), dxn, sizeof(double) * ((size_t)sz + 1)}};
    const int rc = fetch_copies(h, s, fc, 1);   // (the one wait; `s` may be another stream than the handle's own: nothing is left on it)
    if (rc != ORCVIO_OK) return rc;
    int bad = 0;
    std::memcpy(&bad, &back[sz], sizeof(int));
    if (bad) { g_last_error = "cov_commit_new_features_fac: singular H_2"; return ORCVIO_ERR_NOT_SPD; }
    std::memcpy(dx_new, back.data(), sizeof(double) * sz);
    h->commit_new_features_fac(nt, kf, sz, follows);
    h->new_F = 0;
    return ORCVIO_OK;
}

// Factor the resident covariance NOW (asynchronously, on the handle's stream): P = L L^T, L kept as the resident square-root
// factor.  processModel adds Q to the IMU block, after which no factor of P is known; a caller that propagates and augments when
// the image arrives and updates when the front end has finished tracking it (milliseconds later) takes the Cholesky of the
// prior -- the one part of the first update of a frame that does not depend on the tracks -- off the update's critical path.
int32_t orcvio_msckf_cov_prefactor(orcvio_msckf_handle* h) {
    if (!h || h->res_n == 0) { g_last_error = "cov_prefactor: no resident covariance"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    const int n = h->res_n, nb = (n + 15) / 16;
    if (!h->factor_opt || h->fac_follows()) return ORCVIO_OK;   // switched off, or the factor is known already
    if (nb > 14 || nb * 16 > h->NP_max) return ORCVIO_OK;   // no register-resident factorisation of this size: the update factors P itself
    hipStream_t s = h->stream;
    // L(i, j) = R[j * ld + i] (k_potrf_reg writes the upper factor R, P = R^T R, full 16 x 16 tiles, zeros below the diagonal): the
    // layout of the resident factor S (S(i, j) = d_Sres[i + j * fac_ld]).  With the reversed factorisation the
    // factor comes out with its rows in reverse order: it is written to scratch and flipped into place, and its last 15 columns
    // are zero in the active rows (fac_tail)
    const double eps = 2.220446049250313e-16;
    const bool rev = h->fused_solve && n - 15 >= 16;
    const int ld = CovBook::ld_for(n);
    double* dst = rev ? h->d_KG : h->d_Stmp;   // (d_KG: scratch of the optional outputs, free between updates)
    { const int rp = launch_potrf_reg_slots(s, h->d_Pres, n, n, 8.0 * eps, dst, ld, h->d_DinvP, h->d_info, 1, rev ? 1 : 0); if (rp != ORCVIO_OK) return rp; }
    if (rev) hipLaunchKernelGGL(k_fac_flip, dim3((n * ld + 255) / 256), dim3(256), 0, s, (const double*)dst, ld, n, h->d_Stmp, ld);
    HIPCHK(hipGetLastError());
    h->prefactor(rev);
    return ORCVIO_OK;
}
