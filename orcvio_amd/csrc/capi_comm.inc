// capi_comm.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// the handle's RCCL communicator, bounded waits, the sharded updates.

// ---- multi-GPU: RCCL communicator owned by the handle (SURVEY.md 8b / 8e) ---------------------------------------
// RCCL is loaded with dlopen on first use, so the library has no link-time dependency on it and a single-GPU caller
// never loads it.  In a process that already holds librccl.so.1 (PyTorch ships one) the same instance is reused.
// Every wait that another rank can strand is BOUNDED (ORCVIO_COMM_TIMEOUT_S, default 180 s): the creation of the
// communicator runs on a helper thread the caller stops waiting for, the streams that carry a collective are polled; a
// time-out aborts the communicator and returns ORCVIO_ERR_TIMEOUT -- never a hang.
namespace {
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
RcclApi g_rccl;
}  // namespace

static int rccl_load() {
    if (g_rccl.lib) return ORCVIO_OK;
    const char* env = getenv("ORCVIO_RCCL_LIB");
    const char* cands[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void* lib = nullptr;
    std::string tried;
    for (const char* c : cands) {
        if (!c || !*c) continue;
        lib = dlopen(c, RTLD_NOW | RTLD_GLOBAL);
        if (lib) break;
        tried += std::string(c) + " ";
    }
    if (!lib) { g_last_error = "RCCL not found (tried " + tried + "; set ORCVIO_RCCL_LIB)"; return ORCVIO_ERR_NO_DEVICE; }
    RcclApi a;
    a.lib = lib;
#define RCCL_SYM(name) a.name = reinterpret_cast<decltype(a.name)>(dlsym(lib, "nccl" #name)); \
    if (!a.name) { g_last_error = "RCCL: symbol nccl" #name " missing"; dlclose(lib); return ORCVIO_ERR_NO_DEVICE; }
    RCCL_SYM(GetUniqueId) RCCL_SYM(CommInitRank) RCCL_SYM(CommDestroy) RCCL_SYM(CommAbort) RCCL_SYM(AllGather) RCCL_SYM(AllReduce)
    RCCL_SYM(GroupStart) RCCL_SYM(GroupEnd) RCCL_SYM(GetErrorString)
#undef RCCL_SYM
    g_rccl = a;
    return ORCVIO_OK;
}
#define RCCLCHK(expr)                                                                                       \
    do {                                                                                                    \
        ncclResult_t _r = (expr);                                                                           \
        if (_r != ncclSuccess) {                                                                            \
            g_last_error = std::string(#expr) + ": " + g_rccl.GetErrorString(_r);                           \
            return ORCVIO_ERR_HIP;                                                                          \
        }                                                                                                   \
    } while (0)

// A blocking RCCL call on a helper thread, waited for with a bound.  If the caller gives up, the thread is left to finish (or
// to sit) on its own and cleans up what it produced; the shared state outlives both.
namespace {
struct BoundedCall {
    std::mutex m;
    std::condition_variable cv;
    bool done = false, abandoned = false;
    ncclResult_t result = ncclSuccess;
    ncclComm_t comm = nullptr;
    ncclUniqueId id;
};
}  // namespace

int32_t orcvio_msckf_comm_unique_id(uint8_t* id) {
    if (!id) { g_last_error = "comm_unique_id: null"; return ORCVIO_ERR_INVALID; }
    if (ipc_transport_selected()) return ipc_unique_id(id);   // (ORCVIO_COMM_TRANSPORT=ipc: RCCL is never loaded)
    { const int rl = rccl_load(); if (rl != ORCVIO_OK) return rl; }
    static_assert(sizeof(ncclUniqueId) == ORCVIO_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    auto st = std::make_shared<BoundedCall>();
    std::thread([st] {
        ncclUniqueId u;
        const ncclResult_t r = g_rccl.GetUniqueId(&u);
        std::lock_guard<std::mutex> lk(st->m);
        st->id = u; st->result = r; st->done = true;
        st->cv.notify_all();
    }).detach();
    std::unique_lock<std::mutex> lk(st->m);
    if (!st->cv.wait_for(lk, std::chrono::duration<double>(comm_timeout_seconds()), [&] { return st->done; })) {
        st->abandoned = true;
        g_last_error = "comm_unique_id: ncclGetUniqueId did not return within ORCVIO_COMM_TIMEOUT_S";
        return ORCVIO_ERR_TIMEOUT;
    }
    if (st->result != ncclSuccess) { g_last_error = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(st->result); return ORCVIO_ERR_HIP; }
    std::memcpy(id, &st->id, sizeof(ncclUniqueId));
    return ORCVIO_OK;
}

// a rank that never arrives leaves the others in a collective for ever: give the communicator up instead
static void comm_abort(orcvio_msckf_handle* h) {
    if (h->comm) { (void)g_rccl.CommAbort(h->comm); h->comm = nullptr; }
    if (h->ipc) ipc_close(h);
    h->comm_world = 0; h->comm_rank = 0;
    h->graph_epoch++;
}

// Wait for a stream that carries a collective: polled, bounded.  Spins for the first two milliseconds (an update takes a
// fraction of one), then naps between polls.
static int comm_stream_wait(orcvio_msckf_handle* h, hipStream_t s, const char* who) {
    if (!h->comm && !h->ipc) { HIPCHK(hipStreamSynchronize(s)); return ORCVIO_OK; }
    const auto t0 = std::chrono::steady_clock::now();
    const double limit = comm_timeout_seconds();
    for (unsigned it = 0;; ++it) {
        const hipError_t e = hipStreamQuery(s);
        if (e == hipSuccess) return ORCVIO_OK;
        if (e != hipErrorNotReady) { g_last_error = std::string(who) + ": " + hipGetErrorString(e); return ORCVIO_ERR_HIP; }
        if ((it & 63u) == 63u) {
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (el > limit) {
                comm_abort(h);
                g_last_error = std::string(who) + ": a rank did not arrive at the collective within ORCVIO_COMM_TIMEOUT_S; the communicator has been aborted";
                return ORCVIO_ERR_TIMEOUT;
            }
            if (el > 2e-3) std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
    }
}

int32_t orcvio_msckf_comm_destroy(orcvio_msckf_handle* h) {
    if (!h) return ORCVIO_ERR_INVALID;
    if (h->ipc) {
        (void)hipSetDevice(h->device);
        (void)comm_stream_wait(h, h->stream, "comm_destroy");
        if (h->ipc) ipc_close(h);
    }
    if (h->comm) {
        (void)hipSetDevice(h->device);
        (void)comm_stream_wait(h, h->stream, "comm_destroy");
        if (h->comm && h->comm_stream) (void)comm_stream_wait(h, h->comm_stream, "comm_destroy");
        if (h->comm) (void)g_rccl.CommDestroy(h->comm);
        h->comm = nullptr;
    }
    if (h->d_gather) { (void)hipFree(h->d_gather); h->d_gather = nullptr; }
    if (h->d_dofs) { (void)hipFree(h->d_dofs); h->d_dofs = nullptr; }
    if (h->h_dofs) { (void)hipHostFree(h->h_dofs); h->h_dofs = nullptr; }
    if (h->comm_stream) { (void)hipStreamDestroy(h->comm_stream); h->comm_stream = nullptr; }
    h->comm_world = 0; h->comm_rank = 0;
    h->graph_epoch++;
    return ORCVIO_OK;
}

int32_t orcvio_msckf_comm_init(orcvio_msckf_handle* h, const uint8_t* id, int32_t rank, int32_t world) {
    if (!h || !id || world < 1 || rank < 0 || rank >= world) { g_last_error = "comm_init: invalid rank / world"; return ORCVIO_ERR_INVALID; }
    if (h->comm || h->ipc || h->d_gather) (void)orcvio_msckf_comm_destroy(h);
    if (ipc_transport_selected()) return ipc_init(h, id, rank, world);
    { const int rl = rccl_load(); if (rl != ORCVIO_OK) return rl; }
    HIPCHK(hipSetDevice(h->device));
    auto st = std::make_shared<BoundedCall>();
    std::memcpy(&st->id, id, sizeof(ncclUniqueId));
    const int device = h->device;
    std::thread([st, device, world, rank] {
        (void)hipSetDevice(device);
        ncclComm_t c = nullptr;
        const ncclResult_t r = g_rccl.CommInitRank(&c, world, st->id, rank);
        std::unique_lock<std::mutex> lk(st->m);
        st->result = r; st->comm = c; st->done = true;
        const bool orphan = st->abandoned;
        st->cv.notify_all();
        lk.unlock();
        if (orphan && r == ncclSuccess && c) (void)g_rccl.CommAbort(c);   // nobody is waiting for it any more
    }).detach();
    {
        std::unique_lock<std::mutex> lk(st->m);
        if (!st->cv.wait_for(lk, std::chrono::duration<double>(comm_timeout_seconds()), [&] { return st->done; })) {
            st->abandoned = true;
            g_last_error = "comm_init: ncclCommInitRank did not return within ORCVIO_COMM_TIMEOUT_S (a rank missing, or the bootstrap stuck)";
            return ORCVIO_ERR_TIMEOUT;
        }
        if (st->result != ncclSuccess) { g_last_error = std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(st->result); return ORCVIO_ERR_HIP; }
        h->comm = st->comm;
    }
    h->comm_rank = rank; h->comm_world = world;
    const size_t slot = (size_t)h->NAP_max * h->NAP_max + ORCVIO_SHARD_META;
    HIPCHK(hipMalloc(&h->d_gather, sizeof(double) * slot * world));
    HIPCHK(hipMalloc(&h->d_dofs, sizeof(double) * 2 * (world + 8)));
    HIPCHK(hipHostMalloc(&h->h_dofs, sizeof(double) * 2 * (world + 8), hipHostMallocDefault));
    HIPCHK(hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
    h->graph_epoch++;
    return ORCVIO_OK;
}

int32_t orcvio_msckf_comm_info(orcvio_msckf_handle* h, int32_t* rank, int32_t* world) {
    if (!h) return ORCVIO_ERR_INVALID;
    if (rank) *rank = h->comm_rank;
    if (world) *world = h->comm_world;
    return ORCVIO_OK;
}

// max over the ranks of count <= 8 doubles (the bench contract's MAX over ranks; a caller's own consistency checks), through the
// handle's communicator on the handle's stream: everything enqueued there before is finished on every rank when it returns, so
// with count = 0 this is the barrier.
int32_t orcvio_msckf_comm_allreduce_max(orcvio_msckf_handle* h, double* values, int32_t count) {
    if (!h || count < 0 || count > 8 || (count > 0 && !values)) { g_last_error = "comm_allreduce_max: 0..8 values"; return ORCVIO_ERR_INVALID; }
    if (!h->comm && !h->ipc) { g_last_error = "comm_allreduce_max: no communicator (orcvio_msckf_comm_init)"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    if (h->ipc) return ipc_allreduce_max(h, values, count);
    hipStream_t s = h->stream;
    double* hb = h->h_dofs + 2 * h->comm_world;       // pinned scratch behind the dofs: [8]
    double* db = h->d_dofs + 2 * h->comm_world;
    for (int i = 0; i < 8; ++i) hb[i] = i < count ? values[i] : 0.0;
    HIPCHK(hipMemcpyAsync(db, hb, sizeof(double) * 8, hipMemcpyHostToDevice, s));
    RCCLCHK(g_rccl.AllReduce(db, db, 8, ncclDouble, ncclMax, h->comm, s));
    HIPCHK(hipMemcpyAsync(hb, db, sizeof(double) * 8, hipMemcpyDeviceToHost, s));
    { const int rw = comm_stream_wait(h, s, "comm_allreduce_max"); if (rw != ORCVIO_OK) return rw; }
    for (int i = 0; i < count; ++i) values[i] = hb[i];
    return ORCVIO_OK;
}
int32_t orcvio_msckf_comm_barrier(orcvio_msckf_handle* h) { return orcvio_msckf_comm_allreduce_max(h, nullptr, 0); }

// this rank's tracks -> its block, written straight into its slot of the gather buffer, a few status words behind it -> in-place
// all-gather (the one data-path collective; <= 295 KB per rank, latency-bound over xGMI) -> rank-ordered sum + replicated solve
static inline size_t shard_slot(const orcvio_msckf_handle* h) { return (size_t)h->NAP * h->NAP + ORCVIO_SHARD_META; }

int32_t orcvio_msckf_run_update_sharded(orcvio_msckf_handle* h, void* stream) {
    if (!h) { g_last_error = "run_update_sharded: null handle"; return ORCVIO_ERR_INVALID; }
    if (!h->comm && !h->ipc) { g_last_error = "run_update_sharded: no communicator (orcvio_msckf_comm_init)"; return ORCVIO_ERR_INVALID; }
    // (ipc: the one-shot call took the sequence number at its top; the staged form takes it HERE, before any return only this rank can
    //  take -- nothing uploaded, positions missing, a HIP error: such a rank then leaves its peers waiting for a block that never comes
    //  (a loud ORCVIO_ERR_TIMEOUT there) instead of staying one count behind for good, ADVICE r5)
    unsigned long long q = 0ull;
    if (h->ipc) { q = h->ipc->q_pending ? h->ipc->q_pending : ++h->ipc->seq; h->ipc->q_pending = 0; }
    if (!h->uploaded || h->pw_missing) { g_last_error = "run_update_sharded: nothing uploaded (or positions missing)"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = pick_stream(h, stream);
    const size_t ne = (size_t)h->NAP * h->NAP, slot = shard_slot(h);
    double* base = h->ipc ? ipc_generation(h, q) : h->d_gather;   // (ipc: two generations of slots, capi_ipc.inc)
    double* mine = base + slot * h->comm_rank;
    hipEvent_t* ev = h->shard_ev;   // orcvio_msckf_profile_sharded: events between the three parts, on the stream the update runs on
    if (ev) HIPCHK(hipEventRecord(ev[0], s));
    int rc = run_local_impl(h, s, mine);
    if (rc != ORCVIO_OK) return rc;
    { const int rl = lists_refresh(h, s); if (rl != ORCVIO_OK) return rl; }   // (d_row_ptr; the tracks' launch has been through it already)
    hipLaunchKernelGGL(k_shard_meta, dim3(1), dim3(64), 0, s, mine + ne, h->shard_status, 0, h->F > 0 ? (const int*)h->d_accept : (const int*)nullptr,
                       (const int*)h->d_row_ptr, h->F, q, h->comm_rank);
    HIPCHK(hipGetLastError());
    if (ev) HIPCHK(hipEventRecord(ev[1], s));
    if (h->ipc) { rc = ipc_exchange(h, s, mine, slot, slot, q); if (rc != ORCVIO_OK) return rc; }
    else RCCLCHK(g_rccl.AllGather(mine, h->d_gather, slot, ncclDouble, h->comm, s));
    if (ev) HIPCHK(hipEventRecord(ev[2], s));
    rc = run_finish_impl(h, base, h->comm_world, slot, base + ne, s);
    if (ev && rc == ORCVIO_OK) HIPCHK(hipEventRecord(ev[3], s));
    h->last_sharded = rc == ORCVIO_OK;
    return rc;
}

// Device time of the three parts of the sharded update on this rank, medians over `reps` updates of the uploaded share (HIP events on
// the handle's stream): us[0] local tracks + compression, us[1] the exchange (RCCL all-gather, or the ipc push + signal + wait --
// the wait for the slowest peer included), us[2] rank-ordered sum + replicated solve, us[3] the whole update.  COLLECTIVE: every rank
// calls it with the same reps.
int32_t orcvio_msckf_profile_sharded(orcvio_msckf_handle* h, int32_t reps, double* us) {
    if (!h || !us || reps < 1 || !h->uploaded) { g_last_error = "profile_sharded: invalid"; return ORCVIO_ERR_INVALID; }
    if (!h->comm && !h->ipc) { g_last_error = "profile_sharded: no communicator (orcvio_msckf_comm_init)"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipEvent_t ev[4];
    for (int i = 0; i < 4; ++i) HIPCHK(hipEventCreate(&ev[i]));
    std::vector<float> t[4];
    int rc = ORCVIO_OK;
    for (int r = 0; r < reps && rc == ORCVIO_OK; ++r) {
        h->shard_ev = ev;
        rc = orcvio_msckf_run_update_sharded(h, nullptr);
        h->shard_ev = nullptr;
        if (rc == ORCVIO_OK) rc = comm_stream_wait(h, h->stream, "profile_sharded");
        if (rc != ORCVIO_OK) break;
        for (int i = 0; i < 4; ++i) {
            float v = 0.f;
            if (hipEventElapsedTime(&v, ev[i < 3 ? i : 0], ev[i < 3 ? i + 1 : 3]) != hipSuccess) { v = 0.f; (void)hipGetLastError(); }
            t[i].push_back(v * 1e3f);
        }
    }
    for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ev[i]);
    if (rc != ORCVIO_OK) return rc;
    for (int i = 0; i < 4; ++i) {
        std::sort(t[i].begin(), t[i].end());
        const size_t m = t[i].size();
        us[i] = (m & 1) ? t[i][m / 2] : 0.5 * (t[i][m / 2 - 1] + t[i][m / 2]);
    }
    return ORCVIO_OK;
}

// What the handle's communicator is: out[0] transport (0 none, 1 RCCL, 2 ipc), [1] rank, [2] world, [3] ranks whose block was present
// (its own rank id behind it) in the last sharded update that was downloaded / profiled, [4] 1 if a peer shares this rank's device
// (ipc), [5] 1 if the ipc gather buffer is fine-grained / uncached memory, [6] 1 if a peer runs on ANOTHER device under the ipc transport
// (ORCVIO_IPC_XDEV=1: UNVERIFIED -- it has run with several ranks on one device only), [7] 0.
int32_t orcvio_msckf_comm_details(orcvio_msckf_handle* h, int32_t* out, int32_t count) {
    if (!h || !out || count < 1) { g_last_error = "comm_details: null argument"; return ORCVIO_ERR_INVALID; }
    int seen = h->ranks_seen;
    if (h->last_sharded && (h->comm || h->ipc)) {   // (fresh: straight from the device's status words of the last sharded update)
        HIPCHK(hipSetDevice(h->device));
        if (comm_stream_wait(h, h->last_stream ? h->last_stream : h->stream, "comm_details") == ORCVIO_OK)
            if (hipMemcpy(&seen, h->d_info + 13, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); seen = h->ranks_seen; }
        h->ranks_seen = seen;
    }
    const int32_t v[8] = {h->ipc ? 2 : (h->comm ? 1 : 0), h->comm_rank, h->comm_world, seen, h->ipc && h->ipc->shared_device ? 1 : 0,
                          h->ipc && h->ipc->gather_uncached ? 1 : 0, h->ipc && h->ipc->cross_device ? 1 : 0, 0};
    for (int i = 0; i < count; ++i) out[i] = i < 8 ? v[i] : 0;
    return ORCVIO_OK;
}

// a status that only THIS rank's share can have caused (the window and the prior are replicated, so every other refusal hits
// all ranks alike, before the collective)
static inline bool per_rank_status(int rc) { return rc == ORCVIO_ERR_CAPACITY || rc == ORCVIO_ERR_TRACK_TOO_LONG || rc == ORCVIO_ERR_INVALID; }

int32_t orcvio_msckf_update_features_sharded(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, const orcvio_msckf_window* window,
                                             const orcvio_msckf_tracks* tracks, const double* P, orcvio_msckf_result* result) {
    if (!h || !result) { g_last_error = "update_features_sharded: null argument"; return ORCVIO_ERR_INVALID; }
    if (!h->comm && !h->ipc) { g_last_error = "update_features_sharded: no communicator (orcvio_msckf_comm_init)"; return ORCVIO_ERR_INVALID; }
    int own = ORCVIO_OK;
    std::string own_error;
    // ipc: this update's sequence number, before any return only this rank can take (ADVICE r4: a rank that left early used to stay
    // one count behind for good and then summed its peers' previous blocks)
    if (h->ipc) h->ipc->q_pending = ++h->ipc->seq;
    struct ClearPending { orcvio_msckf_handle* h; ~ClearPending() { if (h->ipc) h->ipc->q_pending = 0; } } clear_pending{h};
    int rc = upload_to_arena(h, flags, window, tracks, P, "orcvio_msckf_update_features_sharded");
    if (rc != ORCVIO_OK && per_rank_status(rc)) {
        // This rank's tracks were refused.  The other ranks are on their way into the all-gather: take part with an EMPTY share
        // and a status word, so that nobody waits for ever and every rank learns of it (ORCVIO_ERR_PEER).
        own = rc; own_error = g_last_error;
        const int32_t zero = 0;
        orcvio_msckf_tracks none{};
        none.n_features = 0; none.obs_ptr = &zero;
        rc = upload_to_arena(h, flags, window, &none, P, "orcvio_msckf_update_features_sharded");
        if (rc != ORCVIO_OK) { g_last_error = own_error; return own; }   // the window itself is unusable: every rank returns here alike
    }
    if (rc != ORCVIO_OK) return rc;
    HIPCHK(hipMemcpyAsync(h->d_in, h->h_stage, upload_bytes(h), hipMemcpyHostToDevice, h->stream));
    { const int rm = arena_mark_read(h, h->stream); if (rm != ORCVIO_OK) return rm; }
    h->shard_status = own;
    rc = orcvio_msckf_run_update_sharded(h, nullptr);
    h->shard_status = 0;
    if (rc != ORCVIO_OK) return rc;
    rc = download_enqueue(h, h->stream, result->P_out != nullptr);
    if (rc != ORCVIO_OK) return rc;
    { const int rw = comm_stream_wait(h, h->stream, "update_features_sharded"); if (rw != ORCVIO_OK) { h->ran = false; h->dl_pending = false; return rw; } }
    { const int rl = ipc_check_lost(h, "update_features_sharded"); if (rl != ORCVIO_OK) { h->dl_pending = false; return rl; } }
    rc = orcvio_msckf_download(h, result);
    if (own != ORCVIO_OK) { g_last_error = own_error; return own; }
    return rc;
}

int32_t orcvio_msckf_update_object_tracks_sharded(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags,
                                                  const orcvio_object_eval_flags* eval_flags, int32_t n_clones,
                                                  const orcvio_object_track* tracks, int32_t n_tracks, const double* P,
                                                  orcvio_msckf_result* res) {
    if (!h || !res) { g_last_error = "update_object_tracks_sharded: null argument"; return ORCVIO_ERR_INVALID; }
    if (!h->comm && !h->ipc) { g_last_error = "update_object_tracks_sharded: no communicator (orcvio_msckf_comm_init)"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int world = h->comm_world, rank = h->comm_rank;
    // ipc: the counters of this update advance before any return only this rank can take (ADVICE r4)
    const unsigned long long q = h->ipc ? ++h->ipc->seq : 0ull;
    const unsigned long long dq = h->ipc ? ++h->ipc->dof_count : 0ull;
    // NAP is a function of the window only: known before the local part runs
    const int n = flags ? flags->leg_dim + 6 * n_clones + h->n_extra : 0;
    const int NA = h->ekf_mode ? n - 15 : n - h->n_extra - 15;
    const size_t ne = (size_t)round_up(NA + 1, 16) * round_up(NA + 1, 16), slot = ne + ORCVIO_SHARD_META;
    if (flags && (NA < 1 || round_up(NA + 1, 16) > h->NAP_max)) { g_last_error = "update_object_tracks_sharded: window exceeds capacity"; return ORCVIO_ERR_CAPACITY; }
    double* base = h->ipc ? ipc_generation(h, q) : h->d_gather;
    double* mine = base + slot * rank;
    int32_t dof = 0;
    int own = ORCVIO_OK;
    std::string own_error;
    int rc = orcvio_msckf_objects_local_tracks(h, flags, eval_flags, n_clones, tracks, n_tracks, P, mine, &dof, nullptr);
    if (rc != ORCVIO_OK && per_rank_status(rc) && flags && eval_flags) {   // this rank's tracks were refused: an empty share + a status word
        own = rc; own_error = g_last_error;
        rc = orcvio_msckf_objects_local_tracks(h, flags, eval_flags, n_clones, nullptr, 0, P, mine, &dof, nullptr);
        if (rc != ORCVIO_OK) { g_last_error = own_error; return own; }   // the window / prior is unusable: every rank returns here alike
        dof = 0;
    }
    if (rc == ORCVIO_OK) rc = objects_rank_dof(h, s, &dof);
    if (rc != ORCVIO_OK) return rc;
    hipLaunchKernelGGL(k_shard_meta, dim3(1), dim3(64), 0, s, mine + ne, own, (int)dof, (const int*)nullptr, (const int*)nullptr, 0, q, rank);
    HIPCHK(hipGetLastError());
    // The gate's threshold is the chi-square quantile of the TOTAL degrees of freedom, host arithmetic above 500 like the
    // reference's (src/orcvio.cpp:1962-1968), and every rank knows its own share of them before its kernels have run: the
    // dofs travel FIRST, on a stream of their own, and the host reads them while the device works on this rank's rows -- no
    // synchronisation in the middle of the update.
    int dof_total = 0;
    if (h->ipc) {   // (host values through the shared segment while the device works on this rank's rows)
        rc = ipc_exchange(h, s, mine, slot, slot, q);
        if (rc == ORCVIO_OK) rc = ipc_sum_dofs(h, (int)dof, &dof_total, dq, q);
        if (rc != ORCVIO_OK) return rc;
    } else {
        h->h_dofs[world + rank] = (double)dof;
        HIPCHK(hipMemcpyAsync(h->d_dofs + rank, h->h_dofs + world + rank, sizeof(double), hipMemcpyHostToDevice, h->comm_stream));
        RCCLCHK(g_rccl.AllGather(h->d_dofs + rank, h->d_dofs, 1, ncclDouble, h->comm, h->comm_stream));
        HIPCHK(hipMemcpyAsync(h->h_dofs, h->d_dofs, sizeof(double) * world, hipMemcpyDeviceToHost, h->comm_stream));
        RCCLCHK(g_rccl.AllGather(mine, h->d_gather, slot, ncclDouble, h->comm, s));
        { const int rw = comm_stream_wait(h, h->comm_stream, "update_object_tracks_sharded"); if (rw != ORCVIO_OK) return rw; }
        for (int r = 0; r < world; ++r) dof_total += (int)h->h_dofs[r];
    }
    UpdateCall c;
    rc = objects_finish_impl(h, base, world, slot, base + ne, dof_total, s, c);
    if (rc != ORCVIO_OK) return rc;
    rc = download_enqueue(h, s, res->P_out != nullptr);
    if (rc != ORCVIO_OK) return rc;
    { const int rw = comm_stream_wait(h, s, "update_object_tracks_sharded"); if (rw != ORCVIO_OK) { h->ran = false; h->dl_pending = false; return rw; } }
    { const int rl = ipc_check_lost(h, "update_object_tracks_sharded"); if (rl != ORCVIO_OK) { h->dl_pending = false; h->objects_mode = false; return rl; } }
    rc = orcvio_msckf_objects_download(h, res);
    h->objects_mode = false;
    if (own != ORCVIO_OK) { g_last_error = own_error; return own; }
    return rc;
}

int32_t orcvio_msckf_profile_stages(orcvio_msckf_handle* h, const char** names, double* ms, int32_t* count) {
    if (!h || !names || !ms || !count) { g_last_error = "profile_stages: null argument"; return ORCVIO_ERR_INVALID; }
    const int ns = h->prof_n > 0 ? h->prof_n - 1 : 0;
    if (*count < ns) { g_last_error = "profile_stages: output arrays too small"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    if (ns > 0) HIPCHK(hipEventSynchronize(h->prof_ev[ns]));
    for (int i = 0; i < ns; ++i) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, h->prof_ev[i], h->prof_ev[i + 1]));
        ms[i] = t;
        names[i] = h->prof_names[i];
    }
    *count = ns;
    return ORCVIO_OK;
}
