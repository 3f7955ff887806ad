// msckf_capi.hip -- C-ABI (include/orcvio_msckf.h) over the gfx950 kernels.
// No CPU fallback exists: every compute entry point fails with ORCVIO_ERR_NO_DEVICE /
// ORCVIO_ERR_HIP when the HIP runtime or a gfx950 device is missing.
#include "../../include/orcvio_msckf.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is loaded with dlopen (comm_* section), never linked
#include <dlfcn.h>
#include <chrono>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <functional>
#include "msckf_kernels.hpp"
#include "triangulate.hpp"
#include "triangulate_arm.hpp"
#include "cov_ops.hpp"
#include "cov_marginal_ops.hpp"
#include "zupt_ops.hpp"
#include "imu_ops.hpp"
#include "zupt_check_ops.hpp"
#include "ekf_rows.hpp"
#include "object_rows.hpp"
#include "object_fused.hpp"
#include "object_lm.hpp"
#include "object_init.hpp"
#include "object_lite.hpp"
#include "io_ops.hpp"
#include "frame_ops.hpp"
#include "clone_choice_ops.hpp"
#include "host/cov_book.hpp"
#include "host/frame_outcome.hpp"
#include "host/object_stage.hpp"
#include "host/zupt_frame_outcome.hpp"
#include <immintrin.h>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

using namespace orcvio_amd;

static thread_local std::string g_last_error;

// Environment switches.  The PRODUCT library reads ten, all documented in include/orcvio_msckf.h ("Environment"): the communicator's
// transport and bounds, the bounds of the in-launch waits, the two numerics-relevant forms of the frame call.  Every ablation, stamp and
// reference path the tests compare the fused kernels against is read through dbg_getenv, which the product build compiles to "unset" (VERDICT r5 #6): those
// switches exist in the diagnostics build only (liborcvio_msckf_dbg.so, -DORCVIO_DEBUG_HOOKS; tests/test_abi.py checks the strings).
#ifdef ORCVIO_DEBUG_HOOKS
static inline const char* dbg_getenv(const char* name) { return getenv(name); }
#else
static inline const char* dbg_getenv(const char*) { return nullptr; }
#endif

// Host wall time of the parts of a call (ORCVIO_TIMING; diagnostics build only: the product build's dbg_getenv says "unset" and every
// mark is a test of a null pointer).  Marks are microseconds after the call's entry, summed over k calls and printed as means by the
// caller.  The sums live in the OBJECT: a static of the function where the process has one timeline of that call, a member of the
// handle where two handles must not share them (the frame call).
struct PhaseTimer {
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int calls = 0;
    static bool on() { static const bool t = dbg_getenv("ORCVIO_TIMING") != nullptr; return t; }
    struct Run {   // the marks of ONE call
        PhaseTimer* t = nullptr;
        std::chrono::steady_clock::time_point t0{};
        void mark(int i) { if (t) t->acc[i] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
    };
    static Run begin(PhaseTimer* t) { return on() && t ? Run{t, std::chrono::steady_clock::now()} : Run{}; }
    bool due(int k) { return on() && (++calls % k) == 0; }   // every k-th call: acc holds the sums of the last k
    double mean(int i, int k) const { return acc[i] / k; }
    void reset() { for (double& v : acc) v = 0.0; }
};

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            g_last_error = std::string(#expr) + ": " + hipGetErrorString(_e);                \
            return ORCVIO_ERR_HIP;                                                           \
        }                                                                                    \
    } while (0)

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
static void so3_exp_decl(const double w[3], double R[9]);   // Sophus SO3d::exp (defined with incrementState_IMUCam below)

// ---- object update: what a call, or orcvio_msckf_io_stage_object_tracks ahead of one, plans and stages ----------------------------------
// ONE input arena per object update, mirrored in pinned host memory (grown on demand) and pulled by one launch: [doubles ... | ints ...].
// Device-side scratch (row arrays written by k_object_rows_batch, Cd, Sg, Gff, factors) is separate and never crosses PCIe.
struct ObjPlan {
    int nobj = 0, rows_tot = 0, no_max = 0, ngroups = 0;
    int NOP = 0, ldf = 0;
    // device pointers
    int *d_ridx = nullptr, *d_rowptr = nullptr, *d_clone = nullptr, *d_cols = nullptr;
    ObjGroup* d_groups = nullptr;
    double *d_hx = nullptr, *d_hf = nullptr, *d_res = nullptr;
    double *d_Cd = nullptr, *d_Sg = nullptr, *d_Gff = nullptr;
    // arrow structure of Hf (structured Householder QR instead of chol(Hf^T Hf)); arrow = false: the Gram route
    bool arrow = false;
    int Kmax = 0, rows_max = 0;
    ObjArrow* d_arrow = nullptr;
    int2* d_kp_range = nullptr;
    int* d_kp_rows = nullptr;
    double* d_Rarrow = nullptr;
    double *d_Hr = nullptr, *d_Hfr = nullptr;   // [nobj][N][NOP] per-clone parts of Hf^T r; [nobj][NOP + 1] their sums and |r|^2
    double* d_Bred = nullptr;   // [rows][9] the border of every row after the keypoint blocks have been eliminated
    double* d_Qt = nullptr;     // [rows][OBJ_REFINE_ROW_DOUBLES] obj_refine_body: staging of objects too long for the LDS staging
};
// the staged arena of the one-launch compression: sizes, and where the kernel arguments and the arrows lie
struct ObjFusedStage { size_t nd_tot = 0, ni_tot = 0, args_off = 0, o_arrow = 0; int Kmax = 0, rows_max = 0; };
// What orcvio_msckf_io_stage_object_tracks leaves for the frame call that follows it (one use; any other scan of object tracks voids it)
struct ObjPrestage {
    bool valid = false;
    const orcvio_object_track* tracks = nullptr;
    int n_tracks = 0, N = 0, leg_dim = 0;
    orcvio_object_eval_flags efl;
    ObjScan scan;
    ObjPlan pl;
    ObjFusedStage st;
};

struct IpcComm;
struct orcvio_msckf_handle : CovBook {   // (the resident covariance, its factor and their bookkeeping: host/cov_book.hpp)
    int device = 0;
    int maxN = 0, maxF = 0, maxObs = 0;
    int n_max = 0, NAP_max = 0, NP_max = 0;
    hipStream_t stream = nullptr;       // default launch stream
    hipStream_t side = nullptr;         // Cholesky of the prior, overlapped with the feature kernels
    hipEvent_t ev_fork = nullptr, ev_side = nullptr;
    // problem of the current upload
    orcvio_msckf_flags flags{};
    int N = 0, F = 0, nobs = 0, n = 0, NA = 0, NAP = 0, NP = 0, ldz = 0, m_tot = 0, Mmax = 0;
    int chunks = 0, rows_per_chunk = 0;
    bool uploaded = false, ran = false;
    bool reg_path = true;               // register-resident Cholesky (n <= 224), else the LDS-panel kernel
    bool fused_solve = true;            // chol(M) and the triangular solve in one launch (k_potrf_solve), reg path only
    int* d_skip = nullptr;              // [maxF] tracks dropped by triangulate_uploaded (nullptr semantics: skip_active)
    bool skip_active = false;
    // host <-> device traffic of the one-shot calls: small inputs share one device arena (one copy), everything is staged
    // through pinned host memory (a copy from pageable memory is synchronous and several times slower), the small
    // outputs share one arena (one copy back)
    // ONE input arena and ONE output arena, laid out compactly for the sizes of the current upload (layout_inputs /
    // layout_outputs) and mirrored in pinned host memory: an update moves one block in and one block out
    char *d_in = nullptr, *d_outs = nullptr;         // device arenas
    char* h_stage = nullptr;                          // pinned: [inputs | outputs]
    size_t in_cap = 0, outs_cap = 0, in_used = 0, outs_small = 0, stage_bytes = 0;
    size_t io_poses = 0, io_optr = 0, io_rptr = 0, io_cptr = 0, io_pw = 0, io_oclone = 0, io_cobs = 0, io_z = 0, io_zvel = 0, io_P = 0;
    size_t oo_dx = 0, oo_gamma = 0, oo_accept = 0, oo_Pout = 0;
    bool dl_pending = false, dl_with_P = false;      // a device -> host copy of the outputs is in flight on dl_stream
    hipStream_t dl_stream = nullptr;
    // graph policy: a launch graph is captured when a launch signature is seen for the SECOND time (not necessarily in a
    // row); a slot keeps up to GRAPH_WAYS captured graphs (least recently used one replaced).  More than one way, because
    // the signature contains every pointer a graph bakes in and some of them alternate: the resident square-root factor
    // is double-buffered (cov_commit / cov_prefactor / cov_augment swap d_Sres and d_Stmp), so a filter that repeats one
    // shape replays two graphs in turn (a single slot keyed without that pointer replayed a stale factor).
    static constexpr int GRAPH_WAYS = 6;
    struct GraphSlot {
        struct Way { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; unsigned long long sig = 0, used = 0; };
        Way way[GRAPH_WAYS];
        unsigned long long seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // signatures met once (no graph yet), ring
        int seen_at = 0;
        unsigned long long tick = 0;
    };
    GraphSlot g_update, g_local, g_finish, g_io;
    // ---- zero-copy boundary (orcvio_msckf_io_*): the pinned arena is device-visible and host-coherent, the first kernel of the
    // graph pulls the inputs out of it, the last one pushes the results into it and raises h_flag
    char* h_stage_dev = nullptr;              // device-visible address of h_stage
    unsigned long long* h_flag = nullptr;     // host-coherent word: publications so far (k_epilogue)
    unsigned long long* h_flag_dev = nullptr;
    unsigned long long* d_seq = nullptr;      // device-side twin (the value k_epilogue stores to the flag)
    int* d_pubcnt = nullptr;                  // arrival counter of k_epilogue's workgroups
    unsigned long long pub_enqueued = 0;      // publications enqueued so far (k_epilogue launches, stream order): the flag value to wait for
    bool io_submitted = false, io_sub_P = false, io_sub_commit = false;   // orcvio_msckf_io_submit: launched, not yet collected
    bool io_open = false, io_with_P = false;  // orcvio_msckf_io_begin has laid the arena out and the caller is filling it
    double io_spin_seconds = 2.0;             // bound of the host's wait on h_flag (then: stream synchronisation, then ERR_TIMEOUT)
    bool last_sharded = false;                // the last finished update went through the handle's all-gather (status words in info[9..12])
    hipEvent_t* shard_ev = nullptr;           // orcvio_msckf_profile_sharded: four events the next run_update_sharded records between its parts
    int ranks_seen = 0;                       // ranks whose block was present in the last sharded update looked at (orcvio_msckf_comm_details)
    int shard_status = 0;                     // sharded calls: this rank's own status travelling with its block (ORCVIO_ERR_PEER)
    hipStream_t last_stream = nullptr;   // stream of the last run_update / run_finish (download waits for it)
    double* d_covT = nullptr;   // Phi*P rows of the propagation (d_Pres / d_Ptmp, the resident covariance and its spare buffer: CovBook)
    // Resident SQUARE-ROOT FACTOR of the resident covariance: P_res = S S^T with S (fac_n x fac_k), stored like the
    // Cholesky factor of the prior (d_RP): S(i,j) = d_Sres[j * fac_ld + i].  cov_commit keeps S+ = sigma Z^T of the update
    // that has just run (Z = L_M^-1 S^T is what the solve produces anyway), so the NEXT update of the same frame
    // (pruneImuStateBuffer, processObjects: src/orcvio.cpp:591-594, System.cpp:551-555) skips the Cholesky of its prior.
    // cov_augment / cov_remove_clones carry it along (rows copied / deleted); cov_set / cov_propagate invalidate it.
    // (d_Sres / d_Stmp, fac_n, fac_k, fac_ld, fac_tail, fac_valid: CovBook, with the rule of every edit)
    bool factor_opt = true;             // ORCVIO_OPT_RESIDENT_FACTOR
    int n_nui = 0;                      // ORCVIO_OPT_SCHMIDT_STATES: Schmidt nuisance states (6 columns each) at the END of the extra states
    bool obj_dof_rank = false;          // ORCVIO_OPT_OBJECT_DOF = 1: the object gate counts rows - rank(H_f) degrees of freedom (default: rows - columns, the reference's count)
    bool ref_h2_ldlt = false;           // ORCVIO_OPT_REF_H2_LDLT: the reference's literal H_2.ldlt() (diag(H_2)) in the tail of the hybrid update
    bool ref_stack_hf = false;          // ORCVIO_OPT_REF_STACK_HF: the reference's literal shared-Hf stacking of several objects
    int obj_refine_mode = 1;            // ORCVIO_OPT_OBJECT_REFINE: 0 never, 1 objects with cond_F(R) above 3e6 (default), 2 every object
    int obj_refined = 0;                // objects of the last downloaded object update that took the explicit-basis projection (k_obj_refine)
    size_t obj_fused_budget = 0;        // dynamic LDS a workgroup of k_obj_fused may take on this device (0: not asked yet)
    int obj_fused_opt = 1;              // ORCVIO_OBJ_FUSED=0: object tracks always through the three-launch pipeline (rows materialised)
    unsigned* d_obj_done = nullptr;     // completion counter of k_gemm_objA (cumulative; never reset)
    unsigned obj_done_total = 0u;       // what that counter reads once every compression enqueued so far has finished
    const ObjScan* obj_early = nullptr; // orcvio_msckf_io_update_frame has enqueued this update's compression already (objects_local_tracks skips it): what its scan of the tracks found
    bool obj_last_fused = false;        // the last object update from tracks took the one-launch compression
    size_t obj_lds_budget = 0;          // dynamic LDS the border launch of the object update may take on THIS handle's device (0: not asked yet)
    bool arrow_opt = true;              // ORCVIO_OPT_OBJECT_QR: structured Householder QR of Hf (0: chol(Hf^T Hf), round 1's route)
    bool use_factor = false;            // the current upload's prior comes with its factor: no Cholesky of P
    // The prior's Cholesky is taken of the REVERSED matrix (potrf_reg_body, rev; rev_prior_active): P = S S^T with S(i, c) = L'(n-1-i, c), whose
    // rows 15 .. n-1 (the states measurement rows touch) are zero in the last 15 columns -- M = s2 I + L_a^T A L_a is
    // diag(M', s2 I_15) and only M' (kf - 15) is formed and factored.  `tail` = those trailing columns of the factor in use
    // (15, or 0: LDS-panel path, unfused solve, a resident factor that has been through an augmentation); fac_tail = the same
    // for the resident factor (kept by commit / remove_clones / clones_to_nuisance, dropped by augment).
    int tail = 0;
    // orcvio_msckf_io_update_frame: the object tracks' compression runs on a stream of its own beside the feature update's solve
    hipStream_t obj_stream = nullptr;
    hipEvent_t ev_obj = nullptr;
    bool frame_mode = false;            // (objects_prior: no stream synchronisation, nothing of the prior is staged)
    size_t out_shift = 0;               // host mirror of the outputs arena: offset of the block the next download lands in / is read from
    // small host -> device transfers (SLAM feature records, Phi / Q, nuisance poses) go through a ring of pinned bounce buffers:
    // a host memcpy and an asynchronous copy each, no stream synchronisation (aux_copies)
    char* h_fetch = nullptr;            // pinned block behind fetch_copies (small device arrays -> the caller's pageable memory)
    size_t fetch_cap = 0;
    hipEvent_t ev_arena = nullptr;      // behind the last device read of the pinned input arena that was enqueued (upload_begin waits
    bool arena_busy = false;            //  for THAT, not for whatever else the stream carries: a prefactorisation, a commit ..)
    char* h_aux[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t aux_cap[4] = {0, 0, 0, 0};
    hipEvent_t ev_aux[4] = {nullptr, nullptr, nullptr, nullptr};
    bool aux_busy[4] = {false, false, false, false};
    int aux_next = 0;
    bool obj_status_cleared = false;    // k_object_rows_batch of the current object update has zeroed the shard status words (info[9..12])
    int last_run_kind = 0;              // 0: run_update (single GPU), 1: run_local / run_finish (staged or sharded), 2: objects
    int front_spin_limit = 1 << 19;    // polls before a workgroup of k_front gives up at the device-wide counter (tens of ms)
    int front_fallbacks = 0;            // how often that happened (orcvio_msckf_counters [0])
    long long cnt_graph_captures = 0, cnt_graph_replays = 0, cnt_plain_runs = 0;   // launch sequences captured / replayed from a graph / enqueued as plain launches
    bool last_update_objects = false;   // the last finished update was a (gated) object update
    bool prior_forked = false;          // the Cholesky of the prior runs on the side stream (ev_side must be joined)
    int kf = 0;                         // columns of the prior's factor = dimension of M (n unless a resident factor is used)
    int* d_covmap = nullptr;
    double* d_imu = nullptr;            // orcvio_msckf_cov_propagate_imu: the per-sample records [128][IMU_REC], then the status word of k_imu_phi_q
    std::vector<double> imu_recs;       // ... and their host copy, sized at create: the host half writes them, aux_copies stages them
    double* d_imu46 = nullptr;          // orcvio_msckf_cov_propagate_imu_calib: the records at leg_dim 46 [128][IMU_REC46] (the status word is d_imu's)
    std::vector<double> imu_recs46;     // ... and their host copy
    // orcvio_msckf_io_propagate_imu: the next frame call on the handle enqueues k_imu_phi_q in front of its head launch (one-shot; the
    // frame call consumes it).  The records wait in imu_recs.
    bool imu_armed = false;
    int imu_S = 0;
    ImuFlags imu_fl{};
    orcvio_msckf_imu_config imu_cfg{};
    std::vector<double> imu_sel;        // the samples the host half selected [128][7] (imu_recent_zupt): what a checked call tests
    ImuMeanState imu_after{};           // ... and the state it propagated to (armed form: kept for orcvio_msckf_cov_zupt_frame_checked)
    double* d_zchk = nullptr;           // k_zupt_check: the packed rows [128][4], its four result doubles (eight reserved), sixteen status words
    ZuptCheckJob zchk_job{};            // the check validated in front of a checked propagation's launches
    int *h_imu_status = nullptr, *h_imu_status_dev = nullptr;   // host-coherent word: the armed launch's status, read behind the frame's one wait
    bool pw_missing = false;            // uploaded without positions: triangulate_uploaded must run before the update
    int *d_tri_valid = nullptr, *d_tri_flags = nullptr, *d_tri_init = nullptr;
    double *d_tri_sol = nullptr, *d_tri_cost = nullptr;
    // orcvio_msckf_io_triangulate: the next update on the open arena triangulates its own tracks (one-shot; the update consumes it)
    char *h_tri = nullptr, *h_tri_dev = nullptr;   // pinned [mode | valid | flags | cost | p_w | inv_param] (triangulate_arm.hpp), on first use
    bool tri_armed = false, tri_with_mode = false;
    orcvio_triangulation_config tri_cfg{};
    int* d_tri_words = nullptr;         // [16] status block of the armed launch (TriArgs.words): [2] != 0 = no track is valid -- the update's info_also
    bool tri_refuse_empty = false;      // the current armed update has nothing but its tracks: without a valid one it leaves P and its factor alone
    bool tri_live = false;              // the positions of the current upload were made on the device by an armed update: a repeat of that update
                                        // (a lost hand-off) keeps them and d_skip -- it pulls the derived index arrays only and does not triangulate again
    // orcvio_msckf_io_triangulate_prune: the SECOND update of the next frame call triangulates its tracks, from an observation list of its
    // own (one-shot: the frame consumes it, an orcvio_msckf_io_begin drops it); all of it on first use
    char *h_tri2 = nullptr, *h_tri2_dev = nullptr;   // pinned second block: modes and results as h_tri, the staged list behind them (tri_prune_layout)
    char* d_tri2_list = nullptr;        // the list in HBM (tri_list_layout of the armed counts), pulled by the second update's head
    int* d_tri2_words = nullptr;        // [16] status block of that launch (TriArgs.words)
    int* d_skip2 = nullptr;             // [maxF] the second arena's d_skip (swapped with it: step_arena_swap)
    bool tri2_armed = false;
    int tri2_F = 0, tri2_nobs = 0;      // tracks and observations of the staged list
    orcvio_triangulation_config tri2_cfg{};
    bool tri_live_prune = false;        // tri_live, and the launch was the prune update's: the repeat's refusal word is d_tri2_words
    // orcvio_msckf_io_choose_clones: the next frame call checks the caller's remove_clones against findRedundantImuStates on the poses its
    // first update leaves (k_clone_choice between the two updates; one-shot as the armings above); allocated on first use
    char *h_cc = nullptr, *h_cc_dev = nullptr;   // pinned: the result block | its sequence word (CCH_SEQ_OFFSET) | the staged configuration (CCH_CFG_BYTES0)
    bool cc_armed = false;
    int cc_tracking_ok = 0;
    unsigned long long cc_seq = 0;      // launches of k_clone_choice so far: the value the next one stores behind its block
    // orcvio_msckf_cov_marginal_submit / _collect (k_cov_marginal): all of it allocated at create
    char *h_marg = nullptr, *h_marg_dev = nullptr;   // pinned, host-coherent: the result block [64][64] | its sequence word (MARG_SEQ_OFFSET)
    double* d_margT = nullptr;          // device staging of T [64][64]
    unsigned long long marg_seq = 0;    // launches of k_cov_marginal so far: the value the next one stores behind its block
    bool marg_submitted = false;        // a submit has not been collected
    int marg_rows = 0;                  // rows (= columns) of the outstanding result
    int* d_flag = nullptr;              // step counter of that launch (inside the d_info allocation, own 128-byte line)
    // device buffers
    double *d_poses = nullptr, *d_pw = nullptr, *d_obs_z = nullptr, *d_obs_zvel = nullptr, *d_P = nullptr;
    int *d_obs_ptr = nullptr, *d_obs_clone = nullptr, *d_row_ptr = nullptr, *d_accept = nullptr, *d_info = nullptr;
    double *d_chi2 = nullptr, *d_Hs = nullptr, *d_gamma = nullptr, *d_Gpart = nullptr, *d_Ab = nullptr, *d_A = nullptr;
    int front_fused = 1;                // ORCVIO_OPT_FUSED_FRONT
    bool front_blocked_by_comm = false; // ipc transport, ranks sharing this device: k_front's co-residency cannot be had (capi_ipc.inc); the option above is not touched
    int n_extra = 0;                    // ORCVIO_OPT_EXTRA_STATES
    int ekf_mode = 0;                   // ORCVIO_OPT_EKF_ROWS: the extra states are active columns (EKF-SLAM rows may follow an upload)
    int ekf_F = 0, ekf_idp = 3;         // SLAM features of the current upload (orcvio_msckf_upload_ekf_rows)
    int ekf_cap = 0;
    int* d_ekf_i = nullptr;             // [3 cap] anchor | state | slot
    double* d_ekf_d = nullptr;          // [46 cap] H_e 12 | H_a 12 | H_x 12 | H_f 6 | z_vel 2 | r 2
    double* d_ekf_E = nullptr;          // [2 cap][NAP_max] dense accepted rows [H | r]
    double* d_Gekf = nullptr;           // [NAP_max^2] their Gram (lower tiles)
    double* d_ekf_gamma = nullptr; int* d_ekf_accept = nullptr;
    int dense_rows = 0, dense_cap = 0;  // caller-projected dense rows [H | r] stacked as they are (orcvio_msckf_upload_dense_rows)
    double* d_dense = nullptr;          // [dense_cap][NAP_max]
    bool ekf_eval = false;              // the four blocks are evaluated on the device from the SLAM features (k_ekf_eval)
    double* d_slam = nullptr;           // [12 cap] param 3 | inv_depth 1 | p_w 3 | p_fej 3 | z 2
    char* d_aug = nullptr; size_t aug_cap = 0;   // scratch of orcvio_msckf_cov_commit_new_features and of _fac (each lays it out for itself)
    char* d_new = nullptr; size_t new_cap = 0, new_out_off = 0;   // entering features (orcvio_msckf_upload_new_features): inputs, then H_1 | H_2 | r_1
    int new_F = 0, new_idp = 3;
    double* d_Rf = nullptr;             // [maxF][6] R factor of every track's H_f (k_feature), for orcvio_msckf_augment_new_features
    int* d_sync = nullptr;              // device-wide counter of k_front (own allocation, zero between launches)
    int* d_la_rdy = nullptr;            // k_potrf_solve_la: one word per block row a far workgroup brings forward (own 128-byte line, cleared by the k_gemm ahead of it); [16..31] / [32] the same and the step counter for chol(P) inside k_front; [48] the finish workgroups' counter (LaFin)
    int la_solve = 3;                   // look-ahead depth of the fused solve (0: k_potrf_solve, one workgroup holds the whole trailing matrix; 2 / 3: k_potrf_solve_la)
    size_t chain_fin_oo = 0;            // ... and where in the second outputs arena it put P++ (checked against the object half's layout)
    double chain_fin_thr = 0.0;         // ... and the threshold it used
    ObjPrestage prestage;               // what orcvio_msckf_io_stage_object_tracks left for the next frame call (valid: it still stands, no other scan of object tracks since)
    unsigned long long cnt_prestaged = 0;   // frame calls that found their object tracks staged ahead
    int chain_fin_dof = -1;             // degrees of freedom the chained object solve's in-launch finish gated with (-1: it did not)
    int fuse_finish = 1;                // P+ / dx (and an object update's gate) by finish workgroups of k_potrf_solve_la (LaFin) instead of a k_finish_sqrt
                                        // launch behind it: 1 = in the chained frame call (both halves: 8-9 us off the frame), 2 = every update whose solve
                                        // takes the look-ahead form (measured 2 us SLOWER per queued update: the in-launch hand-off costs what the launch
                                        // boundary does, and the longer launch delays the next replay), 0 = never (ORCVIO_FUSE_FINISH)
    int la_spin = 1 << 22;              // polls (~1 us each) before a wait inside k_potrf_solve_la gives up: the update is then run again through k_potrf_solve
    // second solve context of the frame call's chained object solve (capi_frame.inc, ORCVIO_FRAME_CHAIN): allocated on first use
    double *d_U2 = nullptr, *d_M2 = nullptr, *d_RM2 = nullptr, *d_DinvM2 = nullptr, *d_Z2 = nullptr;
    char* d_outs2 = nullptr;
    unsigned* d_chain_words = nullptr;  // [0] feature half: M formed, [1] feature half: committed (cumulative values); [32] step counter, [48..63] block-row words of the second solve, [64] its finish workgroups' counter (LaFin)
    unsigned chain_seq = 0u;
    long long cnt_chained = 0;          // frames whose object solve ran chained (orcvio_msckf_counters [6])
    long long cnt_sym_pulls = 0;        // pulls of a host P that took the upper-trapezoid form (launch_ingest_P; orcvio_msckf_counters [10])
    long long cnt_lists_in_place = 0;   // updates whose k_front read row_ptr / clone_ptr / clone_obs in the pinned arena (lists_in_place_active; orcvio_msckf_counters [11])
    bool lists_stale = false;           // ... and the HBM image of those three lists belongs to an earlier upload since: whoever reads it pulls it first (lists_refresh)
    bool frame_chain = true;            // ORCVIO_FRAME_CHAIN (read at create, default 1): orcvio_msckf_io_update_frame runs the object solve chained (capi_frame.inc)
    bool blk2_opt = true;               // ORCVIO_BLK2 (read at create): windows of 15 .. 26 block steps factor by 2 x 2 blocks out of the register kernels
    bool la_attr = false;               // the dynamic-LDS opt-in of k_potrf_solve_la is set for this handle's device
    // multi-GPU: RCCL communicator of this handle (orcvio_msckf_comm_init), the all-gather buffer [world][NAP_max^2] and
    // the gathered degrees of freedom of a sharded object update
    ncclComm_t comm = nullptr;
    struct IpcComm* ipc = nullptr;      // the second transport (ORCVIO_COMM_TRANSPORT=ipc, capi_ipc.inc): shared memory + HIP IPC, ranks of one node
    int comm_rank = 0, comm_world = 0;
    double *d_gather = nullptr, *d_dofs = nullptr;
    hipStream_t comm_stream = nullptr;  // carries the early exchange of the degrees of freedom of a sharded object update
    double* h_dofs = nullptr;           // pinned [2 * world]
    bool A_deferred = false;            // the last run left S / Gpart only: d_A is assembled on demand (assemble_deferred)
    int front_chunks = 1;               // T3 row chunks of the last k_front launch
    int n_cus = 0;                      // compute units of the device
    int clean_NP = -1, clean_path = -1;   // layout for which the strictly-lower tiles of d_RP / d_RM are known to be zero
    double *d_RP = nullptr, *d_DinvP = nullptr, *d_U = nullptr, *d_M = nullptr, *d_RM = nullptr, *d_DinvM = nullptr;
    double *d_Z = nullptr, *d_Pout = nullptr, *d_dx = nullptr;
    double *d_La = nullptr, *d_DinvA = nullptr, *d_W = nullptr, *d_Y = nullptr, *d_KG = nullptr;   // optional outputs
    // object blocks (allocated on first use, grown on demand)
    double *d_Gobj = nullptr, *d_RF = nullptr, *d_DinvF = nullptr, *d_Yobj = nullptr, *d_objH = nullptr;
    double *d_obj_gamma = nullptr;
    double obj_thr = -1.0;   // chi-square threshold of the object update being finished (host value, passed to k_finish_sqrt)
    int *d_obj_i = nullptr, *d_obj_accept = nullptr;
    size_t cap_Gobj = 0, cap_RF = 0, cap_Yobj = 0, cap_objH = 0, cap_obj_i = 0;
    char* h_obj_stage_dev = nullptr;   // device-visible address of h_obj_stage (k_ingest pulls the staged tracks / rows out of it)
    bool pub_pending = false;          // the results of the last one-shot object update are on their way to the pinned block (k_epilogue): wait on h_flag
    char *h_obj_stage = nullptr, *d_obj_in = nullptr;   // input arena of an object update: pinned mirror + device copy (grown on demand)
    size_t obj_stage_cap = 0;
    char *h_lm = nullptr, *d_lm = nullptr;             // staging of orcvio_msckf_object_lm, its own (an open io_begin's arena and the object update's staging stay as they are): pinned [inputs | outputs] + device copy
    size_t lm_cap = 0;
    std::vector<ObjUse> obj_use;        // (objects_local_tracks: per-track records, kept across calls: no allocation per frame)
    std::vector<int> obj_fnr;           // (objects_local) keypoint block of every row
    std::vector<signed char> obj_nv;    // (objects_tracks_scan) detected keypoints of every frame of every usable track: the ONE pass over the observations
    std::vector<int> obj_rowkp, obj_Ks; // keypoint block of every row / keypoint count of every object (structured QR of Hf)
    std::vector<unsigned long long> obj_vmask;   // (objects_local_tracks) observed keypoints of every frame of the track being staged
    // per-stage device times of the last object update (orcvio_msckf_profile_stages): events recorded between the stages
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;
    std::vector<const char*> prof_names;
    int prof_n = 0;
    bool objects_mode = false;
    int obj_dof = 0, obj_rows = 0, obj_count = 0;
    double *d_T3 = nullptr, *d_Xobs = nullptr, *d_S = nullptr;
    int *d_clone_ptr = nullptr, *d_clone_obs = nullptr;   // d_clone_ptr: [0..N] first sparse row of every clone; d_clone_obs: obs_pos
    std::vector<int> h_clone_ptr, h_clone_obs;
    int s_chunks = 0;
    bool materialize = false;
    int feat_ablate = 0;
    // captured launch graph of run_update (valid for the current upload and launch stream)
    // every captured graph bakes in device pointers and launch arguments: anything that reallocates a buffer a graph may
    // reference, or changes an option / gate threshold, bumps this epoch; the epoch is part of the launch signature, so a
    // stale graph can never be replayed (use-after-free through ekf_reserve / upload_dense_rows)
    unsigned long long graph_epoch = 1;
    bool use_graph = true;
    size_t hs_rows_cap = 0;
    int gram_chunks_cap = 64;
    // host staging
    std::vector<double> h_poses, h_chi2;
    std::vector<int> h_row_ptr;
    std::vector<unsigned char> track_is_run;   // upload_finalize: the track's clones are a contiguous run
    std::vector<int> frame_row_ptr;     // orcvio_msckf_io_update_frame: the feature half's row offsets while the object half uses h_row_ptr
    // orcvio_msckf_io_step_frame (capi_step.inc): the second update of a frame goes through an arena pair of its own, swapped in and out
    char *d_in2 = nullptr, *h_stage2 = nullptr, *h_stage2_dev = nullptr;
    bool arena_swapped = false;
    // orcvio_msckf_io_step_frame_ex: staging of the frame's feature events, of their own (step_events, capi_step.inc) -- the propagation
    // scratch and the index map the separate cov_* calls stage in are in use inside a frame
    char *h_evt = nullptr, *h_evt_dev = nullptr, *d_evt = nullptr;
    int* d_step_words = nullptr;        // [0..15] status words of the frame's first update, kept for the second update's commit (info_also)
    std::vector<int> step_row_ptr;      // the second update's row offsets
    long long cnt_step_frames = 0, cnt_step_repairs = 0;   // frames through orcvio_msckf_io_step_frame; updates of such frames run again after a lost hand-off
#ifdef ORCVIO_DEBUG_HOOKS
    PhaseTimer step_timer;              // ORCVIO_TIMING of the frame call, per handle (step_timer_of)
#endif
    bool ekf_one_launch = true;         // the in-state features' evaluation, fill and gate in ONE launch (k_ekf_evalgate) instead of three (ORCVIO_EKF_ONE_LAUNCH=0, diagnostics)
    bool finpub_opt = true;             // a feature update's k_finish_sqrt + k_epilogue as ONE launch (k_finish_pub) on the in-place paths (ORCVIO_FINISH_PUB=0, diagnostics)
    bool last_finpub_commit = false;    // the update enqueued last committed by writing P+ into the spare covariance buffer: the host swaps d_Pres / d_Ptmp
    bool thin_opt = true;               // updates of at most THIN_MAX_ROWS projected rows on the in-place paths take the reference's direct form (k_thin_gain / k_thin_apply;
                                        // ORCVIO_THIN_UPDATE=0, diagnostics): pruneImuStateBuffer's update is a handful of rows
    double *d_Hthin = nullptr, *d_Vthin = nullptr, *d_uthin = nullptr;   // its projected rows [THIN_MAX_ROWS][NAP_max], V [n_max][THIN_MAX_ROWS], u
    bool last_update_thin = false;      // the update enqueued last took it: its commit leaves NO square-root factor
    bool step_fused = true;             // ORCVIO_STEP_FUSED=0 (diagnostics build): the frame's small steps as the separate launches and copies of the round-5 calls
    // the frame call's in-state rows beside k_front (enqueue_update): k_wait_word -> k_ekf_evalgate -> k_gram -> k_obj_done on `side`, joined
    // by two polled words (d_step_words[32]: k_front has started = the frame head is complete; [33]: the rows' Gram is complete, k_gemm_asmA_w)
    bool ekf_side_opt = true;           // ORCVIO_STEP_EKF_SIDE=0 (diagnostics build): the rows on the update's own stream, in front of k_front
    bool ekf_side_used = false;         // the frame being enqueued has work on `side` (a repair drains it)
    long long ekf_side_skip_until = 0;  // a frame whose side-stream join gave up was repaired: the next 4 096 frames keep the rows on the update's own stream
                                        // (a profiler that serialises dispatches, another tenant: the join must not cost its bound on every frame)
    unsigned ekf_side_seq = 0;
    double chi2_prob_cached = -1.0;
};

// What ONE enqueue of an update is asked for, passed by reference down io_enqueue -> enqueue_update -> launch_front / launch_solve_stage.
// Nothing of it is state of the filter: it dies with the scope of the caller that owns it.  A default-constructed record is a plain update.
struct UpdateCall {
    // ---- set by the caller
    bool fin_pub = false;               // launch_solve_stage(ST_FINISH) launches k_finish_pub with pub (io_enqueue fills it); enqueue_thin takes its commit / publication part
    FinishPubArgs pub{};
    int* info_keep = nullptr;           // k_epilogue keeps a copy of this update's status words there (EpilogueArgs.info_keep: the frame call's feature half)
    const int* info_also = nullptr;     // a second status block whose refusal refuses this update's commit too (the step call's second update)
    bool fin_frame = false;             // the chained frame call is enqueueing its feature half (finish_fused_active)
    bool ekf_side = false;              // the step call's first update: the in-state rows beside k_front, on the side stream
    bool already_ingested = false;      // k_frame_head has pulled the arena of this update (io_enqueue skips its ingest launch)
    bool io_single = false;             // io_launch's: ONE update on the arena, whose host-derived lists stay as they are until the launch has ended (lists_in_place_active)
    bool tri = false;                   // armed by orcvio_msckf_io_triangulate: k_triangulate behind the pull of the arena (io_enqueue; h->tri_cfg, h->tri_with_mode)
    bool tri_prune = false;             // ... by orcvio_msckf_io_triangulate_prune: the frame's second update (h->tri2_cfg, the staged list, the second block)
    unsigned* mark_M_word = nullptr;    // ST_FORM_M / ST_POTRF_M store mark_M_val there once M is formed, and put the pointer back to null: the caller
    unsigned mark_M_val = 0u;           //  sees from its record whether the mark went out
    const unsigned* join_wait = nullptr;   // the ST_FORM_U product polls this counter (the frame call's object half) ...
    unsigned join_expect = 0u;          // ... until it reaches this value
    bool thin_blocked = false;          // K / G / H_thin requested: those are derived from the general path's factors (thin_possible)
    bool retry_forked = false;          // the repeat of an update that lost an in-launch hand-off: forked front end, one-workgroup factorisation + solve
    const std::function<int()>* mid = nullptr;   // called once the tracks' launch is out (enqueue_update)
    // ---- left by one stage for a later stage of the same enqueue
    unsigned* front_mark = nullptr; unsigned front_mark_val = 0;       // enqueue_update -> launch_front: FrontGramArgs.started
    const unsigned* asm_wait = nullptr; unsigned asm_wait_val = 0;     // enqueue_update -> launch_solve_stage(ST_FORM_U): k_gemm_asmA_w
};

// ---- resident covariance / factor bookkeeping of the handle (host/cov_book.hpp) ---------------------------------------------------
// saved and restored around steps that are enqueued ahead of their outcome
using CovState = CovBook;
static inline CovState cov_state(const orcvio_msckf_handle* h) { return *h; }
static inline void cov_restore(orcvio_msckf_handle* h, const CovState& c) { static_cast<CovBook&>(*h) = c; }
// what the commit of the update enqueued last does to the resident factor
static inline FacAfter update_fac_after(const orcvio_msckf_handle* h) {
    if (h->last_update_thin) return FacAfter::drop;   // (the direct form of a thin stack leaves no square-root factor)
    if (h->factor_opt && h->n_nui == 0) return FacAfter::adopt;   // S+ = sigma Z^T
    return h->n_nui > 0 ? FacAfter::drop : FacAfter::leave;   // Schmidt: the nuisance block of P+ is the prior's, so P+ != s2 Z^T Z
}
// the factor S+ = sigma Z^T of the update that has just been enqueued, and its covariance
static inline void fac_adopt_update(orcvio_msckf_handle* h) { h->commit_update(h->n, h->kf, h->ldz, h->tail, false, FacAfter::adopt); }
// the host-side bookkeeping of a commit that rides in the update's last launch (valid whether or not the device refuses the update:
// a refused commit leaves the prior and a copy of its factor, io_ops.hpp k_epilogue)
static inline void commit_bookkeeping(orcvio_msckf_handle* h) {
    h->commit_update(h->n, h->kf, h->ldz, h->tail, h->last_finpub_commit, update_fac_after(h));   // (k_finish_pub wrote P+ into the spare buffer)
    h->last_finpub_commit = false;
}

// an update has been enqueued: what the host remembers of the launch (orcvio_msckf_cov_commit, the repeat of a lost hand-off and the
// counters read these four).  kind: last_run_kind -- 0 run_update, 1 run_local / run_finish, 2 objects
static inline void mark_update_enqueued(orcvio_msckf_handle* h, int kind, bool sharded = false) {
    h->ran = true; h->last_update_objects = kind == 2; h->last_run_kind = kind; h->last_sharded = sharded;
}
// the one-shot armings that belong to the open arena are dropped: a new upload (upload_begin), a call that takes the track buffers
// (orcvio_msckf_triangulate), the frame call once nothing can refuse the frame any more.  first_update_too = false: the frame call --
// its first update's arming (orcvio_msckf_io_triangulate) is taken by tri_consume when that update is enqueued.
static inline void drop_one_shot_armings(orcvio_msckf_handle* h, bool first_update_too = true) {
    if (first_update_too) h->tri_armed = false;
    h->tri2_armed = false;
    h->cc_armed = false;
}
static inline PhaseTimer* step_timer_of(orcvio_msckf_handle* h) {
#ifdef ORCVIO_DEBUG_HOOKS
    return &h->step_timer;
#else
    (void)h; return nullptr;
#endif
}

template <typename T>
static int grow(T** p, size_t* cap, size_t need) {
    if (*cap >= need) return ORCVIO_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIPCHK(hipMalloc(p, sizeof(T) * need));
    *cap = need;
    return ORCVIO_OK;
}

extern "C" {

int32_t orcvio_msckf_abi_version(void) { return ORCVIO_MSCKF_ABI_VERSION; }
const char* orcvio_msckf_last_error(void) { return g_last_error.c_str(); }

#include "capi_handle.inc"   // chi-square quantile, the arenas, create / destroy, options
#include "capi_update.inc"   // upload, the launches of one update, the launch-graph cache, run_local / run_finish
#include "capi_hybrid.inc"   // EKF-SLAM rows of the hybrid filter, features entering the state, the H_1 / H_2 tail
#include "capi_io.inc"   // download, the zero-copy update (io_begin / io_update), the copying one-shot call, gate_tracks
#include "capi_objects.inc"   // the object update: staging, compression pipeline, finish / download, ObjectLM messages, row evaluation
#include "capi_ipc.inc"   // the second transport of the communicator: HIP IPC + shared memory (several ranks per device possible)
#include "capi_comm.inc"   // the handle's RCCL communicator, bounded waits, the sharded updates
#include "capi_cov.inc"   // per-kernel profile, the device-resident covariance and its square-root factor
#include "capi_object_mapper.inc"   // the object mapper: the start and the Levenberg-Marquardt refinement of object tracks, with keypoints and bbox-only
#include "capi_imu.inc"   // IMU propagation from raw samples: the host half (host/imu_model.hpp), k_imu_phi_q, the propagation behind it
#include "capi_imu_calib.inc"   // ... at leg_dim 46 (IMU intrinsics in the state): the imu_*46 host half, k_imu_phi_q46
#include "capi_zupt_check.inc"   // zero-velocity detection from IMU samples: k_zupt_check's packing, launch and verdict; stand-alone and behind the IMU propagation
#include "capi_zupt.inc"   // zero-velocity frames on the resident covariance: ONE driver for the update and the four stationary frames (unchecked / checked, hybrid)
#include "capi_frame.inc"   // one frame in one call: feature update + object update, the objects' compression beside the features' solve
#include "capi_clone_choice.inc"   // the check of the clones that leave inside the one-call frame: arming, k_clone_choice's launch, its result
#include "capi_step.inc"   // one FILTER frame in one call: propagate, augment, update, prune update, marginalise on the resident covariance
#include "capi_state.inc"   // triangulation, incrementState_IMUCam (host arithmetic)
#include "capi_debug.inc"   // diagnostics build only: test hooks and ablation timers

}  // extern "C"
