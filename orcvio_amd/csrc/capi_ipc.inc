// capi_ipc.inc -- part of msckf_capi.hip (ONE translation unit: included there, in this order; not compiled on its own).
// The second transport of the handle's communicator (ORCVIO_COMM_TRANSPORT=ipc): ranks of ONE node exchange their compressed
// blocks by storing them straight into each other's gather buffers (HIP IPC memory handles), announced through sequence words in a
// POSIX shared-memory segment that every rank maps into its device address space.  Same entry points, same results as the RCCL
// transport (System::processObjects / removeLostFeatures sharded over ranks, SURVEY.md 8e); what it adds:
//   * it runs with SEVERAL RANKS ON ONE DEVICE (RCCL refuses two ranks per device), so the N > 1 product path can be executed and
//     tested on a one-GPU box: two processes, one MI355X;
//   * over xGMI it takes the collective's launch (10-20 us of RCCL kernel start + ring steps for 295 KB) off the critical path:
//     one store kernel per rank (every peer's slot written directly, all links at once), one flag store, one polling wavefront.
// Protocol of one sharded update with sequence number q (parity p = q & 1; the gather buffer holds two generations of slots):
//     local tracks -> this rank's block in its OWN slot of generation p
//     k_ipc_push     the block -> slot `rank` of generation p in every peer's gather buffer, then __threadfence_system() by every
//                    storing thread (the ordering is explicit: ADVICE r4; kernel end = a second release)
//     k_ipc_signal   flags[peer][rank] <- q for every peer                                         (host-coherent memory, release)
//     k_ipc_wait     one wavefront polls flags[rank][*] >= q (bounded: wall clock), then checks that the sequence word behind the
//                    peer's block in THIS rank's buffer (ORCVIO_SHARD_META_SEQ, written by k_shard_meta, travelling with the block)
//                    is q as well -- a rank whose counter has slipped, or a slot still holding another update, is a lost block
//     rank-ordered sum of the slots of generation p + replicated solve                             (kernel START = acquire)
// The gather buffer is allocated fine-grained / uncached (hipExtMallocWithFlags, as RCCL allocates its exchange buffers) so that
// no L2 of the owning device keeps lines of generation q - 2 (plain hipMalloc when that allocation fails).
// NOT VERIFIED ACROSS DEVICES: every test and soak so far is several ranks on ONE device (no multi-GPU box was available).
// The counters: `seq` (one per sharded update), `dof_count` (one per sharded object update), `red_count` (one per host reduction)
// advance at the TOP of the call that uses them, before any return only one rank can take, so that a rank-local failure (a HIP
// error, a time-out) leaves that rank's peers waiting for a block that never comes (a loud ORCVIO_ERR_TIMEOUT) and not the rank
// one count behind for good; the dof slots carry the update's sequence number and the reader checks it.
// Two generations are enough: a peer sends block q + 1 only after its own finish of q (stream order), and this rank pushes q + 2
// (same parity as q) only after it has seen the peer's q + 1.
// Host-side exchanges (the degrees of freedom of a sharded object update, the bench's barrier / max): slots in the same segment,
// double-buffered by the same argument, every wait bounded by ORCVIO_COMM_TIMEOUT_S.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#define ORCVIO_IPC_MAX_RANKS 16
#include "host/ipc_protocol.hpp"
namespace {
struct IpcShm {
    uint32_t magic, world;
    volatile uint32_t stage[ORCVIO_IPC_MAX_RANKS];                      // rendezvous: 1 = handle published, 2 = peers opened, 3 = leaving
    hipIpcMemHandle_t handles[ORCVIO_IPC_MAX_RANKS];                    // every rank's gather buffer
    alignas(128) volatile unsigned long long flags[ORCVIO_IPC_MAX_RANKS][ORCVIO_IPC_MAX_RANKS];   // [dst][src]: sequence number of src's block in dst's buffer
    IpcHostSlots host;                                                   // the host exchanges (host/ipc_protocol.hpp: all-reduce, degrees of freedom)
    char bus_id[ORCVIO_IPC_MAX_RANKS][32];                               // PCI bus id of every rank's device
};
}  // namespace
struct IpcComm {
    int fd = -1;
    IpcShm* shm = nullptr;           // host mapping
    IpcShm* shm_dev = nullptr;       // the same segment in the device's address space (hipHostRegister)
    bool registered = false;
    std::string name;
    double* peer_gather[ORCVIO_IPC_MAX_RANKS] = {nullptr};   // peers' gather buffers (IPC-opened; own entry = own buffer)
    bool opened[ORCVIO_IPC_MAX_RANKS] = {false};
    double** d_peer = nullptr;       // device copy of peer_gather
    size_t gen_stride = 0;           // doubles between the two generations of slots
    unsigned long long seq = 0, red_count = 0, dof_count = 0;
    int* d_lost = nullptr;           // set by k_ipc_wait when a peer's block did not arrive in time
    bool gather_uncached = false;    // the gather buffer is fine-grained / uncached memory (else plain hipMalloc)
    bool cross_device = false;       // some peer runs on ANOTHER device: unverified (no multi-GPU machine was available): refused unless ORCVIO_IPC_XDEV=1
    bool shared_device = false;      // some peer runs on THIS rank's device: the fused front end is blocked for this handle (front_fused_active)
    unsigned long long q_pending = 0;   // sequence number taken at the top of a one-shot sharded call for the run_update_sharded inside it
};

static double comm_timeout_seconds() {
    static const double t = [] { const char* e = getenv("ORCVIO_COMM_TIMEOUT_S"); const double v = e ? atof(e) : 180.0; return v > 0.0 ? v : 180.0; }();
    return t;
}
static bool ipc_transport_selected() {
    const char* e = getenv("ORCVIO_COMM_TRANSPORT");
    return e && (std::strcmp(e, "ipc") == 0 || std::strcmp(e, "IPC") == 0);
}

namespace orcvio_amd {
// this rank's block (n doubles at src) -> slot `rank` of every peer's gather buffer: grid (chunks, world), 16-byte stores
__global__ __launch_bounds__(256) void k_ipc_push(const double* __restrict__ src, double* const* __restrict__ peers, size_t dst_off, size_t n, int rank) {
    const int p = blockIdx.y;
    if (p == rank) return;
    double2* dst = reinterpret_cast<double2*>(peers[p] + dst_off);
    const double2* s2 = reinterpret_cast<const double2*>(src);
    const size_t n2 = n / 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256) dst[i] = s2[i];
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) peers[p][dst_off + n - 1] = src[n - 1];
    __threadfence_system();   // the block is visible to the peer's device before anything this stream does next (the signal)
}
// "my block q is in your buffer": one release store per peer into the shared segment (host-coherent memory)
__global__ __launch_bounds__(64) void k_ipc_signal(IpcShm* shm, int rank, int world, unsigned long long q) {
    const int p = threadIdx.x;
    if (p < world && p != rank) __hip_atomic_store(const_cast<unsigned long long*>(&shm->flags[p][rank]), q, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// wait until every peer's block q has been announced; bounded by `ticks` of the 100 MHz wall clock
// (seq0: the sequence word behind slot 0 of the generation being summed, `slot` doubles between slots; lost = 1 + p: the block of
// rank p never came, 1001 + p: it came with another update's sequence number)
__global__ __launch_bounds__(64) void k_ipc_wait(IpcShm* shm, int rank, int world, unsigned long long q, unsigned long long ticks, int* lost,
                                                 const double* seq0, size_t slot) {
    const int p = threadIdx.x;
    if (p >= world || p == rank) return;
    const unsigned long long t0 = wall_clock64();
    const unsigned long long* f = const_cast<const unsigned long long*>(&shm->flags[rank][p]);
    while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < q) {
        if (wall_clock64() - t0 > ticks) { atomicExch(lost, 1 + p); return; }
        __builtin_amdgcn_s_sleep(32);
    }
    const unsigned long long bits = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(seq0 + slot * p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (__longlong_as_double((long long)bits) != (double)q) atomicExch(lost, 1001 + p);
}
}  // namespace orcvio_amd

static void ipc_close(orcvio_msckf_handle* h) {
    IpcComm* c = h->ipc;
    if (!c) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (c->shm) c->shm->stage[h->comm_rank] = 3;
    h->front_blocked_by_comm = false;
    for (int p = 0; p < ORCVIO_IPC_MAX_RANKS; ++p)
        if (c->opened[p] && c->peer_gather[p]) (void)hipIpcCloseMemHandle(c->peer_gather[p]);
    if (c->d_peer) (void)hipFree(c->d_peer);
    if (c->d_lost) (void)hipFree(c->d_lost);
    if (c->registered) (void)hipHostUnregister(c->shm);
    if (c->shm) (void)munmap(c->shm, sizeof(IpcShm));
    if (c->fd >= 0) (void)close(c->fd);
    if (!c->name.empty() && h->comm_rank == 0) (void)shm_unlink(c->name.c_str());   // (normally unlinked right after the rendezvous already)
    delete c;
    h->ipc = nullptr;
}

// bounded spin on a host condition
static bool ipc_host_wait(const std::function<bool()>& done, double limit_s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0;; ++it) {
        if (done()) return true;
        _mm_pause();
        if ((it & 1023u) == 1023u) {
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (el > limit_s) return false;
            if (el > 2e-3) std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    }
}

static int ipc_unique_id(uint8_t* id) {
    // 128 random bytes: the name of the shared-memory segment is derived from them
    int fd = open("/dev/urandom", O_RDONLY | O_CLOEXEC);
    if (fd < 0) { g_last_error = "comm_unique_id (ipc): /dev/urandom"; return ORCVIO_ERR_HIP; }
    size_t got = 0;
    while (got < ORCVIO_COMM_ID_BYTES) {
        const ssize_t r = read(fd, id + got, ORCVIO_COMM_ID_BYTES - got);
        if (r <= 0) { close(fd); g_last_error = "comm_unique_id (ipc): short read"; return ORCVIO_ERR_HIP; }
        got += (size_t)r;
    }
    close(fd);
    return ORCVIO_OK;
}

static int ipc_init(orcvio_msckf_handle* h, const uint8_t* id, int rank, int world) {
    if (world > ORCVIO_IPC_MAX_RANKS) { g_last_error = "comm_init (ipc): at most 16 ranks"; return ORCVIO_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<IpcComm> c(new IpcComm);
    char nm[64];
    std::snprintf(nm, sizeof nm, "/orcvio_comm_%02x%02x%02x%02x%02x%02x%02x%02x%02x%02x%02x%02x", id[0], id[1], id[2], id[3], id[4], id[5], id[6], id[7],
                  id[8], id[9], id[10], id[11]);
    c->name = nm;
    const double limit = comm_timeout_seconds();
    // ---- the segment: rank 0 creates it (exclusively, owner-only), the others open it when it is there and complete
    if (rank == 0) {
        (void)shm_unlink(nm);
        c->fd = shm_open(nm, O_RDWR | O_CREAT | O_EXCL | O_CLOEXEC, 0600);
        if (c->fd < 0 || ftruncate(c->fd, (off_t)sizeof(IpcShm)) != 0) { g_last_error = std::string("comm_init (ipc): shm_open ") + nm; if (c->fd >= 0) close(c->fd); return ORCVIO_ERR_HIP; }
    } else {
        const bool ok = ipc_host_wait([&] {
            c->fd = shm_open(nm, O_RDWR | O_CLOEXEC, 0600);
            if (c->fd < 0) return false;
            struct stat st;
            if (fstat(c->fd, &st) == 0 && (size_t)st.st_size >= sizeof(IpcShm)) return true;
            close(c->fd); c->fd = -1;
            return false;
        }, limit);
        if (!ok) { g_last_error = "comm_init (ipc): rank 0 did not create the shared segment within ORCVIO_COMM_TIMEOUT_S"; return ORCVIO_ERR_TIMEOUT; }
    }
    void* m = mmap(nullptr, sizeof(IpcShm), PROT_READ | PROT_WRITE, MAP_SHARED, c->fd, 0);
    if (m == MAP_FAILED) { g_last_error = "comm_init (ipc): mmap"; close(c->fd); if (rank == 0) shm_unlink(nm); return ORCVIO_ERR_HIP; }
    c->shm = static_cast<IpcShm*>(m);
    h->ipc = c.release();
    IpcComm* ic = h->ipc;
    h->comm_rank = rank; h->comm_world = world;
    auto fail = [&](int code, const std::string& msg) { g_last_error = msg; ipc_close(h); h->comm_rank = 0; h->comm_world = 0; return code; };
    if (rank == 0) {   // (a fresh segment is zero-filled; the magic word is written last)
        ic->shm->world = (uint32_t)world;
        __atomic_store_n(&ic->shm->magic, 0x4F524356u, __ATOMIC_RELEASE);
    } else {
        if (!ipc_host_wait([&] { return __atomic_load_n(&ic->shm->magic, __ATOMIC_ACQUIRE) == 0x4F524356u; }, limit))
            return fail(ORCVIO_ERR_TIMEOUT, "comm_init (ipc): the shared segment was never initialised");
        if (ic->shm->world != (uint32_t)world) return fail(ORCVIO_ERR_INVALID, "comm_init (ipc): the ranks disagree about the world size");
    }
    {   // the segment in the device's address space
        const hipError_t e = hipHostRegister(ic->shm, sizeof(IpcShm), hipHostRegisterMapped | hipHostRegisterPortable);
        if (e != hipSuccess) return fail(ORCVIO_ERR_HIP, std::string("comm_init (ipc): hipHostRegister: ") + hipGetErrorString(e));
        ic->registered = true;
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, ic->shm, 0) != hipSuccess) return fail(ORCVIO_ERR_HIP, "comm_init (ipc): hipHostGetDevicePointer");
        ic->shm_dev = static_cast<IpcShm*>(dp);
    }
    // ---- gather buffer: two generations of `world` slots; its IPC handle goes into the segment
    const size_t slot = (size_t)h->NAP_max * h->NAP_max + ORCVIO_SHARD_META;
    ic->gen_stride = slot * world;
    {
        // fine-grained / uncached like RCCL's exchange buffers: no cache of the owning device keeps lines a peer has rewritten
        void* g = nullptr;
        hipIpcMemHandle_t mh;
        hipError_t e = hipExtMallocWithFlags(&g, sizeof(double) * slot * world * 2, hipDeviceMallocUncached);
        if (e == hipSuccess) { e = hipIpcGetMemHandle(&mh, g); if (e != hipSuccess) { (void)hipFree(g); g = nullptr; } }
        ic->gather_uncached = (e == hipSuccess);
        (void)hipGetLastError();
        if (!g) {   // (the plain, coarse-grained allocation when the uncached one is not to be had)
            if (hipMalloc(&g, sizeof(double) * slot * world * 2) != hipSuccess) return fail(ORCVIO_ERR_HIP, "comm_init (ipc): hipMalloc(gather)");
            e = hipIpcGetMemHandle(&mh, g);
        }
        h->d_gather = static_cast<double*>(g);
        (void)hipMemset(h->d_gather, 0, sizeof(double) * slot * world * 2);
        if (e != hipSuccess) return fail(ORCVIO_ERR_HIP, std::string("comm_init (ipc): hipIpcGetMemHandle: ") + hipGetErrorString(e) + " (HSA_ENABLE_IPC_MODE_LEGACY=0 ?)");
        std::memcpy(&ic->shm->handles[rank], &mh, sizeof mh);
        char bus[32] = {0};
        (void)hipDeviceGetPCIBusId(bus, (int)sizeof bus, h->device);
        std::memcpy(const_cast<char*>(ic->shm->bus_id[rank]), bus, sizeof bus);
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail(ORCVIO_ERR_HIP, "comm_init (ipc): hipDeviceSynchronize");
    __atomic_store_n(&ic->shm->stage[rank], 1u, __ATOMIC_RELEASE);
    for (int p = 0; p < world; ++p) {
        if (!ipc_host_wait([&] { return __atomic_load_n(&ic->shm->stage[p], __ATOMIC_ACQUIRE) >= 1u; }, limit))
            return fail(ORCVIO_ERR_TIMEOUT, "comm_init (ipc): rank " + std::to_string(p) + " did not arrive within ORCVIO_COMM_TIMEOUT_S");
        if (p == rank) { ic->peer_gather[p] = h->d_gather; continue; }
        if (std::memcmp(const_cast<const char*>(ic->shm->bus_id[p]), const_cast<const char*>(ic->shm->bus_id[rank]), 32) == 0) ic->shared_device = true;
        else ic->cross_device = true;
        hipIpcMemHandle_t mh;
        std::memcpy(&mh, &ic->shm->handles[p], sizeof mh);
        void* dp = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&dp, mh, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) return fail(ORCVIO_ERR_HIP, std::string("comm_init (ipc): hipIpcOpenMemHandle(rank ") + std::to_string(p) + "): " + hipGetErrorString(e));
        ic->peer_gather[p] = static_cast<double*>(dp);
        ic->opened[p] = true;
    }
    if (ic->cross_device) {   // (every rank takes the same decision: if the ranks are not all on one device, each of them has a peer on another)
        const char* x = getenv("ORCVIO_IPC_XDEV");
        if (!(x && x[0] == '1'))
            return fail(ORCVIO_ERR_INVALID, "comm_init (ipc): ranks on DIFFERENT devices -- this transport has run with several ranks on one device only; "
                                            "set ORCVIO_IPC_XDEV=1 to use it across devices (unverified), or leave ORCVIO_COMM_TRANSPORT unset for RCCL");
    }
    if (hipMalloc(&ic->d_peer, sizeof(double*) * ORCVIO_IPC_MAX_RANKS) != hipSuccess || hipMalloc(&ic->d_lost, sizeof(int)) != hipSuccess)
        return fail(ORCVIO_ERR_HIP, "comm_init (ipc): hipMalloc");
    if (hipMemcpy(ic->d_peer, ic->peer_gather, sizeof(double*) * ORCVIO_IPC_MAX_RANKS, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(ic->d_lost, 0, sizeof(int)) != hipSuccess)
        return fail(ORCVIO_ERR_HIP, "comm_init (ipc): the peer table could not be set up");
    __atomic_store_n(&ic->shm->stage[rank], 2u, __ATOMIC_RELEASE);
    for (int p = 0; p < world; ++p)
        if (!ipc_host_wait([&] { return __atomic_load_n(&ic->shm->stage[p], __ATOMIC_ACQUIRE) >= 2u; }, limit))
            return fail(ORCVIO_ERR_TIMEOUT, "comm_init (ipc): rank " + std::to_string(p) + " did not open its peers within ORCVIO_COMM_TIMEOUT_S");
    if (rank == 0) { (void)shm_unlink(nm); }   // everybody holds the mapping: the name can go (nothing is left behind by a crash later)
    if (ic->shared_device) {
        // Ranks that SHARE a device must not use launches that wait for their own workgroups to be co-resident: k_front's device-wide
        // counter needs all 1 + F/2 workgroups on the device at once, and the other rank's kernels hold compute units (found by
        // scripts/gpu_soak_ipc.py: with updates queued on both ranks an in-launch hand-off timed out every ~200 windows -- a flagged
        // no-update, never a wrong result).  The forked seven-launch form has no such wait (INTEGRATION.md 8, ORCVIO_OPT_FUSED_FRONT).
        // The user's ORCVIO_OPT_FUSED_FRONT is left untouched: front_fused_active() consults this flag (ADVICE r4).
        h->front_blocked_by_comm = true;
    }
    if (hipMalloc(&h->d_dofs, sizeof(double) * 2 * (world + 8)) != hipSuccess ||
        hipHostMalloc(&h->h_dofs, sizeof(double) * 2 * (world + 8), hipHostMallocDefault) != hipSuccess ||
        hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking) != hipSuccess) {
        const int code = fail(ORCVIO_ERR_HIP, "comm_init (ipc): allocation of the dof exchange failed");
        (void)orcvio_msckf_comm_destroy(h);   // (frees d_gather / d_dofs / h_dofs / comm_stream)
        return code;
    }
    h->graph_epoch++;
    return ORCVIO_OK;
}

static inline double* ipc_generation(orcvio_msckf_handle* h, unsigned long long q) { return h->d_gather + ipc_slot_offset(q, 0, 0, h->ipc->gen_stride); }

// the exchange of one sharded update on stream s: `mine` (this rank's slot of generation q & 1, `count` doubles) -> every peer,
// then wait for theirs.  Returns the base of the generation the finish sums.
static int ipc_exchange(orcvio_msckf_handle* h, hipStream_t s, double* mine, size_t count, size_t slot, unsigned long long q) {
    IpcComm* c = h->ipc;
    const int world = h->comm_world, rank = h->comm_rank;
    if (world > 1) {
        const size_t off = ipc_slot_offset(q, rank, slot, c->gen_stride);
        const unsigned chunks = (unsigned)std::min<size_t>(16, (count / 2 + 255) / 256 + 1);
        hipLaunchKernelGGL(k_ipc_push, dim3(chunks, world), dim3(256), 0, s, (const double*)mine, (double* const*)c->d_peer, off, count, rank);
        hipLaunchKernelGGL(k_ipc_signal, dim3(1), dim3(64), 0, s, c->shm_dev, rank, world, q);
        // a polling wavefront gives up after min(ORCVIO_COMM_TIMEOUT_S, ORCVIO_IPC_WAIT_S [default 20]) seconds: a wavefront that spins for
        // minutes holds its stream and, on a shared device, a compute unit; raise ORCVIO_IPC_WAIT_S for peers that may stall longer
        static const double wait_s = [] { const char* e = getenv("ORCVIO_IPC_WAIT_S"); const double v = e ? atof(e) : 20.0; return v > 0.0 ? v : 20.0; }();
        const double lim = std::min(comm_timeout_seconds(), wait_s);
        const double* seq0 = ipc_generation(h, q) + (slot - ORCVIO_SHARD_META) + ORCVIO_SHARD_META_SEQ;
        hipLaunchKernelGGL(k_ipc_wait, dim3(1), dim3(64), 0, s, c->shm_dev, rank, world, q, (unsigned long long)(lim * 1e8), c->d_lost, seq0, slot);
        HIPCHK(hipGetLastError());
    }
    return ORCVIO_OK;
}

// after the stream that carried an exchange has drained: did a polling wavefront give up?
static int ipc_check_lost(orcvio_msckf_handle* h, const char* who) {
    IpcComm* c = h->ipc;
    if (!c || h->comm_world < 2) return ORCVIO_OK;
    int lost = 0;
    HIPCHK(hipMemcpy(&lost, c->d_lost, sizeof(int), hipMemcpyDeviceToHost));
    if (lost) {
        HIPCHK(hipMemset(c->d_lost, 0, sizeof(int)));
        h->ran = false;
        if (lost > 1000) {
            g_last_error = std::string(who) + ": the block of rank " + std::to_string(lost - 1001) + " carries another update's sequence number (ipc transport: a rank's "
                           "counter has slipped): no update";
            return ORCVIO_ERR_PEER;
        }
        g_last_error = std::string(who) + ": the block of rank " + std::to_string(lost - 1) + " did not arrive (ipc transport): no update";
        return ORCVIO_ERR_TIMEOUT;
    }
    return ORCVIO_OK;
}

// host all-reduce (max) of eight doubles through the segment; everything enqueued on the handle's stream before is finished first
static int ipc_allreduce_max(orcvio_msckf_handle* h, double* values, int count) {
    IpcComm* c = h->ipc;
    const int world = h->comm_world, rank = h->comm_rank;
    const unsigned long long q = ++c->red_count;   // (first: a rank-local failure below must not leave this rank one count behind)
    { const int rw = comm_stream_wait(h, h->stream, "comm_allreduce_max"); if (rw != ORCVIO_OK) return rw; }
    const int miss = ipc_slots_allreduce_max(&c->shm->host, rank, world, q, values, count,
                                             [&](const std::function<bool()>& pred) { return ipc_host_wait(pred, comm_timeout_seconds()); });
    if (miss >= 0) {
        g_last_error = "comm_allreduce_max (ipc): rank " + std::to_string(miss) + " did not arrive within ORCVIO_COMM_TIMEOUT_S";
        return ORCVIO_ERR_TIMEOUT;
    }
    return ORCVIO_OK;
}

// the degrees of freedom of every rank's objects (host values, known before the kernels run): sum over the ranks
// (q: this object update's dof_count, taken at the top of the call; useq: its sequence number among all sharded updates)
static int ipc_sum_dofs(orcvio_msckf_handle* h, int dof, int* total, unsigned long long q, unsigned long long useq) {
    IpcComm* c = h->ipc;
    const int world = h->comm_world, rank = h->comm_rank;
    const int r = ipc_slots_sum_dofs(&c->shm->host, rank, world, q, useq, dof, total,
                                     [&](const std::function<bool()>& pred) { return ipc_host_wait(pred, comm_timeout_seconds()); });
    if (r >= 0) {
        g_last_error = "update_object_tracks_sharded (ipc): rank " + std::to_string(r) + " did not arrive within ORCVIO_COMM_TIMEOUT_S";
        return ORCVIO_ERR_TIMEOUT;
    }
    if (r <= -2) {   // a value of another update: the ranks' counters disagree
        g_last_error = "update_object_tracks_sharded (ipc): the degrees of freedom of rank " + std::to_string(-2 - r) + " belong to another update";
        return ORCVIO_ERR_PEER;
    }
    return ORCVIO_OK;
}
