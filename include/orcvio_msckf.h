/*
 * orcvio_msckf.h -- C-ABI of the MI355X-native MSCKF measurement-update path.
 *
 * This is the drop-in boundary for ONE hot path of shanmo/OrcVIO: everything the
 * reference does between "a set of feature tracks / object residual rows is ready"
 * and "delta_x and the updated covariance are available" (SURVEY.md section 8).
 * The reference has no FFI layer; the seam is cut inside class OrcVIO
 * (reference include/orcvio/orcvio.h:200-214,393-396).  Each entry point below
 * names the reference code it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - plain C, caller-owned buffers, no exceptions, int status codes;
 *   - all floating point is FP64, ids / indices are int32;
 *   - matrices handed over by the host are dense.  P is symmetric so row- and
 *     column-major coincide; every other matrix states its layout.  P MUST be
 *     symmetric: of each pair P[i][j], P[j][i] outside the diagonal 16 x 16 tiles
 *     (floor(i/16) != floor(j/16)) the update may read either one.  The in-place form
 *     (orcvio_msckf_io.P) and the copying calls that pull P into device memory
 *     themselves (orcvio_msckf_update_features, the object updates' P) read the UPPER
 *     one (floor(j/16) > floor(i/16)) and never touch the other: only the rows'
 *     suffixes from their diagonal tile on cross the link, the device mirrors them
 *     (orcvio_msckf_counters [10]).  The diagonal tiles are read whole;
 *   - error-state order is the reference's (src/orcvio.cpp:202-225,4497-4533):
 *       theta(0:3) v(3:6) p(6:9) bg(9:12) ba(12:15) theta_ext(15:18) t_ext(18:21)
 *       td(21) [IMU intrinsics 22:46 if leg_dim==46] | clone i: theta,p at leg_dim+6i
 *   - one update in flight per handle; calls return after the result is in the
 *     caller's buffers unless the name says _async / _device.
 *
 * Environment.  The library reads TEN environment variables, all of them here (tests/test_abi.py checks the built
 * library against this list); every ablation / stamp / experiment switch of docs/LAB_NOTES.md exists in the diagnostics
 * build only (liborcvio_msckf_dbg.so, -DORCVIO_DEBUG_HOOKS):
 *   ORCVIO_COMM_TRANSPORT    "ipc": the communicator uses HIP IPC + shared memory instead of RCCL (ranks of one node)
 *   ORCVIO_COMM_TIMEOUT_S    bound of every wait another rank can strand, seconds (default 60)
 *   ORCVIO_IPC_WAIT_S        bound of the ipc transport's device-side wait for a peer's block, seconds (default 20)
 *   ORCVIO_IPC_XDEV          "1": allow the ipc transport between ranks on DIFFERENT devices (unverified: refused otherwise)
 *   ORCVIO_RCCL_LIB          path of the RCCL library to dlopen (default librccl.so.1 / librccl.so)
 *   ORCVIO_IO_SPIN_SECONDS   how long the calling thread spins on the result flag before it falls back to a stream
 *                            synchronisation (default 2)
 *   ORCVIO_LA_SPIN           polls (~1 us each) before a wait inside the look-ahead factorisation gives up and the update is
 *                            run again in separate launches (default 1 << 22)
 *   ORCVIO_FRONT_SPIN        the same for the device-wide counter of the fused front end (default 1 << 19)
 *   ORCVIO_FRAME_CHAIN       "0": orcvio_msckf_io_update_frame solves the object update behind the feature update's commit
 *                            (bit-identical to the two calls) instead of chained to its factor (equal to rounding; default 1)
 *   ORCVIO_FRAME_OVERLAP     "0": orcvio_msckf_io_update_frame runs its two halves one behind the other
 */
#ifndef ORCVIO_MSCKF_H
#define ORCVIO_MSCKF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORCVIO_MSCKF_ABI_VERSION 1

/* status codes */
enum {
    ORCVIO_OK = 0,
    ORCVIO_ERR_INVALID = 1,        /* bad argument / null pointer / size mismatch      */
    ORCVIO_ERR_NO_DEVICE = 2,      /* no gfx950 device or HIP runtime failure at create */
    ORCVIO_ERR_CAPACITY = 3,       /* window / tracks exceed the handle's capacity      */
    ORCVIO_ERR_TRACK_TOO_LONG = 4, /* a track has more than ORCVIO_MAX_TRACK observations */
    ORCVIO_ERR_HIP = 5,            /* HIP runtime error during the call (see last_error) */
    ORCVIO_ERR_NOT_SPD = 6,        /* S = H P H^T + sigma^2 I not positive definite in double (sigma^2 lost beside H P H^T: a
                                      prior beyond ~1e16 sigma^2 in scale, sigma = 0), or a non-finite result (NaN / Inf in the
                                      prior, the poses or the noise).  NO UPDATE: the device leaves P and x alone (P+ = P,
                                      dx = 0), the resident covariance and its factor are untouched, and cov_commit refuses
                                      until the next successful update.  (The reference has no such guard: its LDLT
                                      returns whatever comes out, src/orcvio.cpp:1690-1697.) */
    ORCVIO_ERR_TIMEOUT = 7,        /* a bounded wait gave up: an in-launch hand-off (k_front's device-wide counter, a solver
                                      wavefront of k_potrf_solve) after its retry, the creation of the communicator, or a rank
                                      that never arrived at a collective.  NO UPDATE, nothing to commit (cov_commit refuses);
                                      after a time-out inside a collective the communicator has been aborted (comm_info
                                      reports world = 0) and must be created again */
    ORCVIO_ERR_PEER = 8            /* sharded calls: ANOTHER rank could not take part with its share (its tracks were refused:
                                      capacity, a track too long, an index out of range).  Every rank still went through the
                                      collective (the failing rank with an empty share), so nobody hangs; every rank returns an
                                      error (the failing rank its own status, the others this one) and NO rank has an update
                                      to commit */
};

#define ORCVIO_MAX_TRACK 32   /* observations per feature track handled by the wave kernel */
#define ORCVIO_MAX_CLONES 60  /* sliding-window clones per handle                          */
#define ORCVIO_CHI2_TABLE 500 /* reference chi_squre_num_threshold, src/orcvio.cpp:483      */

/* Flags that change hot-path arithmetic (reference YAML keys; src/orcvio.cpp:62-415). */
typedef struct orcvio_msckf_flags {
    int32_t leg_dim;               /* 22, or 46 with calib_imu_instrinsic (src/orcvio.cpp:196-199) */
    int32_t use_larvio;            /* use_larvio_flag                                      */
    int32_t use_left_perturbation; /* use_left_perturbation_flag                           */
    int32_t if_fej;                /* if_FEJ: position_FEJ in the Jacobians (:1104)         */
    int32_t estimate_td;           /* estimate_td: column 21 = observations_vel (:1211)     */
    int32_t discard_large_update;  /* discard_large_update_flag (:4479-4494), see stats     */
    double noise_feature;          /* noise_feature (sigma); squared inside (:106,113)      */
    double chi2_prob;              /* chi_square_threshold_feat, e.g. 0.95                  */
} orcvio_msckf_flags;

/* Sliding window of augmented IMU states (reference struct IMUState_Aug,
 * include/orcvio/imu_state.h:103-148; std::map order = index order here). */
typedef struct orcvio_msckf_window {
    int32_t n_clones;
    const double* R_b2w; /* [N][9] row-major: orientation (body -> world)          */
    const double* t_b_w; /* [N][3] position                                        */
    const double* t_fej; /* [N][3] position_FEJ (may alias t_b_w when !if_fej)      */
    const double* R_b2c; /* [N][9] row-major: R_imu_cam0 (per-clone copy)           */
    const double* t_c_b; /* [N][3] t_cam0_imu                                       */
} orcvio_msckf_window;

/* Feature tracks to be used in this update, CSR over observations (reference struct
 * Feature / MapServer, include/orcvio/feat/feature.hpp:34-269).  The caller lists
 * only the observations that take part: all of them for removeLostFeatures
 * (src/orcvio.cpp:2503-2519), only those of the clones being removed for
 * pruneImuStateBuffer (:2810-2845).  Tracks with fewer than 2 listed observations
 * are skipped (accept = 0, gamma = NaN). */
typedef struct orcvio_msckf_tracks {
    int32_t n_features;
    const double* p_w;        /* [F][3] Feature::position (world)                          */
    const int32_t* obs_ptr;   /* [F+1]                                                     */
    const int32_t* obs_clone; /* [nobs] window index of the observing clone, ascending     */
    const double* obs_z;      /* [nobs][2] Feature::observations (normalised coordinates)   */
    const double* obs_zvel;   /* [nobs][2] Feature::observations_vel; may be NULL if !estimate_td */
} orcvio_msckf_tracks;

/* Pre-evaluated object residual rows in window coordinates: the output of
 * OrcVIO::constructObjectResidualJacobians (src/orcvio.cpp:2017-2151) for one object,
 * i.e. the arguments of OrcVIO::removeLostObjects (:2154-2193), in compact form:
 * every row touches exactly one clone. */
typedef struct orcvio_msckf_object_rows {
    int32_t n_rows;           /* rows of Hx / Hf / res                                     */
    int32_t n_obj_cols;       /* columns of Hf (object state dim, 45 for a 12-keypoint car) */
    const int32_t* row_clone; /* [n_rows] window index of the clone the row belongs to     */
    const double* Hx6;        /* [n_rows][6] the 6 non-zeros of the Hx row (theta, p of that clone) */
    const double* Hf;         /* [n_rows][n_obj_cols] row-major                            */
    const double* res;        /* [n_rows]                                                  */
} orcvio_msckf_object_rows;

/* Caller-allocated outputs.  NULL pointers are skipped. */
typedef struct orcvio_msckf_result {
    double* dx;       /* [n]    delta_x = K r                      (src/orcvio.cpp:1697,1824) */
    double* P_out;    /* [n*n]  (I-KH)P, symmetrised              (:1741-1753)               */
    int32_t* accept;  /* [F]    chi-square gate result             (:1953-1976)               */
    double* gamma;    /* [F]    Mahalanobis distance of each block                            */
    double* H_thin;   /* [(n-15)*n] row-major compressed Jacobian: upper-triangular R placed in state
                         columns 15..n-1 with R^T R = H^T H (+1e-11 max(diag) I: the stacked Jacobian is
                         rank deficient in every update, the shift avoids a rank decision)           */
    double* r_thin;   /* [n-15]                                                              */
    double* K;        /* [n*(n-15)] row-major Kalman gain w.r.t. H_thin                       */
    double* G;        /* [n*n] row-major K*H_thin (basis independent, SURVEY.md note N1)      */
    /* dx, P_out, gamma, accept and G are the results, accurate to ~1e-12 against the double restatement (bar: 1e-6).  H_thin,
       r_thin and K are DIAGNOSTIC outputs: the update is computed in square-root form from the Gram block and never
       needs them; they are derived afterwards from a Cholesky factor of the singular Gram with the shift above and reproduce
       K * H_thin = G and K * r_thin = dx to ~1e-5 relative only (tests/test_gpu_parity.py).  K is basis dependent in any case
       (SURVEY.md note N1): compare G, not K, across implementations. */
    int32_t stats[8]; /* [0] stacked rows (accepted)  [1] rows of H_thin  [2] accepted blocks
                         [3] 1 if an update was applied to P  [4] 1 if the reference's
                         large-update test (:4479) would discard delta_x  [5] zero-variance
                         directions of the prior (dropped pivots of chol(P))  [6] != 0: some pivot of chol(P)
                         fell below -tol (the prior was not PSD)  [7] objects: rank-deficient H_f columns */
} orcvio_msckf_result;

typedef struct orcvio_msckf_handle orcvio_msckf_handle;

/* Version / capability probes (no device needed). */
int32_t orcvio_msckf_abi_version(void);
const char* orcvio_msckf_last_error(void);

/* Chi-square quantile used for the gating tables: replaces boost::math::quantile
 * (src/orcvio.cpp:486-494, 1962-1968).  Host-side, no device needed. */
double orcvio_msckf_chi2_quantile(int32_t dof, double prob);

/* Create / destroy a handle that owns device buffers, streams and the cache of captured launch
 * graphs.  device = HIP device ordinal.  Capacity bounds what later calls may pass.
 * A handle is NOT thread-safe: one thread at a time per handle (the filter thread of the reference is the only caller of these
 * call sites); different handles may be used from different threads.  orcvio_msckf_last_error() is thread-local. */
int32_t orcvio_msckf_create(int32_t device, int32_t max_clones, int32_t max_features,
                            int32_t max_observations, orcvio_msckf_handle** out);
void orcvio_msckf_destroy(orcvio_msckf_handle* h);

/* Options.  ORCVIO_OPT_MATERIALIZE_STACK (default 0): also write the stacked projected blocks
 * [H' | r'] (what the reference builds in H_msckf, src/orcvio.cpp:2497-2527) to device memory.  The
 * update itself never needs them; tests and callers that want H' switch it on. */
/* ORCVIO_OPT_FUSED_SOLVE (default 1): factor M and solve for Z in one launch (solver workgroups trail the
 * factorisation block step by block step); 0 = two launches (k_potrf_reg, k_trsm_lds).  Same arithmetic. */
/* ORCVIO_OPT_LOOKAHEAD_SOLVE (default 3; with ORCVIO_OPT_FUSED_SOLVE on, from six block steps = 81 active states): the one-launch solve
 * spreads the trailing update of chol(M) over one "far" workgroup per block row (k_potrf_solve_la, look-ahead depth 3: a far workgroup
 * applies the published panels to its row and hands it to the factorising workgroup three block steps before it is due); 0 = the whole
 * trailing matrix in the registers of ONE workgroup (k_potrf_solve).  Same arithmetic in the same order: bit-identical results; 32 against
 * 38 us at 30 clones.  The far workgroups are eight to ten more workgroups that must become resident while the launch runs: every wait is
 * bounded (seconds), and an update whose hand-off was lost is run again through k_potrf_solve inside the same call (counted in
 * orcvio_msckf_counters [0]); object updates report ORCVIO_ERR_TIMEOUT instead, as they do for k_potrf_solve's own hand-off. */
/* ORCVIO_OPT_FUSED_FRONT (default 1): the Cholesky of the prior runs as workgroup 0 of the feature launch (k_front)
 * whenever the whole front end is co-resident (n <= 224, 1 + ceil(F/2) workgroups <= compute units); 0 = always fork
 * it to the handle's side stream around k_feature.  Same kernels' bodies, same arithmetic. */
/* ORCVIO_OPT_EXTRA_STATES (default 0): number of state columns BEHIND the clones that no row of the update touches --
 * the EKF-SLAM feature states (and Schmidt nuisance states) the reference keeps at the end of state_cov when
 * max_features_in_one_grid > 0 (src/orcvio.cpp:1495-1510): its H_msckf then has zero columns there
 * (featureJacobian_msckf builds its rows state_cov.cols() wide, :1191-1192) and the update still moves those states and
 * their covariance through the cross terms.  With value k, P / P_out are (LEG + 6N + k)^2 and dx has that length. */
/* ORCVIO_OPT_EKF_ROWS (default 0): the next uploads may be followed by orcvio_msckf_upload_ekf_rows -- the extra states
 * are then active columns of the compressed block (the rows of the SLAM features reach into them). */
/* ORCVIO_OPT_STAGE_PROFILE (default 0): record HIP events between the stages of the object update (rows, compression, the
 * batched factorisation of F, Y, A', the solve, the gate); orcvio_msckf_profile_stages returns the per-stage device times
 * of the last object update (SURVEY.md 8d "device-only time per stage from hipEvents"). */
/* ORCVIO_OPT_RESIDENT_FACTOR (default 1): orcvio_msckf_cov_commit also keeps a square-root factor of the committed
 * covariance (S+ = sigma Z^T, a by-product of the solve), and an update whose prior is the resident covariance (P == NULL)
 * uses it instead of a Cholesky factorisation of P: the second and third update of a frame (pruneImuStateBuffer,
 * processObjects; src/orcvio.cpp:591-594, System.cpp:551-555) skip that 45 us chain.  cov_augment / cov_remove_clones carry
 * the factor along, cov_set / cov_propagate drop it.  0 = always factor P. */
/* ORCVIO_OPT_OBJECT_QR (default 1): the left-nullspace projection of an object's rows against Hf (math_utils.hpp:287-312,
 * the reference takes a full-U SVD) needs the triangular factor of Hf.  1: a structured Householder QR that uses the arrow
 * shape of ObjectLM's state ([pose 6 | shape 3 | 3 per keypoint], include/orcvio/obj/ObjectLM.h:117-123; accuracy
 * cond(Hf) eps -- Hf of a real object has cond ~ 1e8: the keypoint rows have a gauge that only the bbox rows break).  0, and
 * for rows whose Hf does not have that shape: chol(Hf^T Hf) (cond^2: directions below ~1e-8 of the largest are treated as
 * null; stats[7] counts them). */
/* ORCVIO_OPT_SCHMIDT_STATES (default 0) = k: the Schmidt-EKF of the reference (use_schmidt, src/orcvio.cpp:1730-1751, :1893-1935,
 * :2881-2920): the LAST 6 k of the extra states are nuisance states -- clones that left the window but stay in state_cov.  The
 * update leaves the 6k x 6k nuisance block of the covariance as it was (:1740-1751); SLAM features may
 * be anchored at them: anchor index N + j in orcvio_msckf_slam_features / _ekf_rows / _new_features addresses nuisance state j,
 * whose pose comes from orcvio_msckf_upload_nuisance_poses and whose Jacobian block lands in its columns of the nuisance block
 * (:1591-1606).  N + k <= max_clones.  See also orcvio_msckf_cov_clones_to_nuisance, orcvio_msckf_augment_state_nuisance. */
/* ORCVIO_OPT_REF_STACK_HF (default 0): compatibility with the reference's stacking of SEVERAL objects in one call.
 * System::processObjects concatenates Hx, Hf and r of all objects vertically with Hf's 45 columns SHARED
 * (ros_wrapper/src/orcvio/src/System.cpp:684-702) and removeLostObjects projects the whole stack against that single Hf
 * (src/orcvio.cpp:2154-2193) -- the objects are treated as one object observed many times (SURVEY note N3; right for one
 * object per call only).  0: every object is projected against its own Hf (block-diagonal Hf; equal to the reference whenever
 * one object arrives).  1: the literal shared-Hf stack, dof = total rows - columns; all objects must have the same state size. */
/* ORCVIO_OPT_OBJECT_DOF (default 0): degrees of freedom of the object gate (src/orcvio.cpp:2172-2176).  0: rows - columns of H_f,
 * the reference's count.  1: rows - rank(H_f).  They differ only for a rank-deficient H_f (a keypoint never seen inside the window
 * has three zero columns, one seen in a single frame two rows for three columns): the reference keeps rows - columns directions of
 * the left null space -- which ones is decided by rounding noise in its SVD -- while this library projects onto the whole null
 * space (rows - rank directions), so that with the reference's count gamma sums more directions than its threshold
 * counts (biased towards rejection); 1 makes the threshold count what gamma sums.  (One more host synchronisation per object
 * update in that mode: the rank is what the structured QR finds on the device.) */
/* ORCVIO_OPT_REF_H2_LDLT (default 0): the tail of measurementUpdate_hybrid for features ENTERING the state.  The reference solves
 * with `H_2.ldlt()` (src/orcvio.cpp:1826-1827) where H_2 is the upper-triangular R of the new features' H_f (SPQR, :2421-2436):
 * Eigen's LDLT reads the LOWER triangle only, so the reference divides by diag(H_2).  0 (default): the triangular system is
 * solved (what the algebra of :1818-1821 means; identical to the reference for feature_idp_dim = 1, every shipped configuration).
 * 1: the reference's literal arithmetic (affects orcvio_msckf_augment_new_features and orcvio_msckf_cov_commit_new_features; the
 * handle-less orcvio_msckf_augment_state has the twin orcvio_msckf_augment_state_ref_ldlt).  P22 uses (H_2^T H_2)^-1 either way,
 * as the reference does (:1907-1908). */
/* ORCVIO_OPT_OBJECT_REFINE (default 1): how an object whose H_f is ill conditioned is projected (structured-QR route only).  The
 * fast route takes Y = Q_1^T [H_x | r] from the semi-normal equations R^-T (H_f^T [H_x | r]), accurate to cond(H_f) eps; the
 * reference's full-U SVD (math_utils.hpp:287-312) is backward stable.  1: objects whose triangular factor R has |R|_F |R^-1|_F above 3e6
 * (an estimate of cond(H_f) from above, formed on the device; every real car: cond(H_f) ~ 3e8 on the reference's one_car frames) form the basis explicitly, row by row (q_i R = h_i), take
 * Y from it and correct for its loss of orthonormality -- delta_x within 1e-9 of a 50-digit evaluation where the fast
 * route has 1.4e-6.  0: never.  2: every object.  orcvio_msckf_objects_refined reports how many objects of the last update took it.
 * Object TRACKS that qualify for the one-launch compression (orcvio_msckf_counters [5]) take the explicit basis for every object in
 * modes 1 and 2 alike -- there it is the only route, with the orthonormalisation applied to the rows of the basis (to first order,
 * like the correction above); mode 0 sends the tracks through the three-launch pipeline and its fast route. */
enum { ORCVIO_OPT_MATERIALIZE_STACK = 1, ORCVIO_OPT_FUSED_SOLVE = 2, ORCVIO_OPT_FUSED_FRONT = 3, ORCVIO_OPT_EXTRA_STATES = 4,
       ORCVIO_OPT_EKF_ROWS = 5, ORCVIO_OPT_STAGE_PROFILE = 6, ORCVIO_OPT_RESIDENT_FACTOR = 7, ORCVIO_OPT_OBJECT_QR = 8,
       ORCVIO_OPT_REF_STACK_HF = 9, ORCVIO_OPT_SCHMIDT_STATES = 10, ORCVIO_OPT_OBJECT_DOF = 11, ORCVIO_OPT_REF_H2_LDLT = 12,
       ORCVIO_OPT_OBJECT_REFINE = 13, ORCVIO_OPT_LOOKAHEAD_SOLVE = 14 };
int32_t orcvio_msckf_set_option(orcvio_msckf_handle* h, int32_t option, int32_t value);

/* EKF-SLAM rows of the hybrid filter (existing SLAM features).  For every SLAM feature the current
 * state observes, the reference evaluates featureJacobian_ekf (src/orcvio.cpp:1575-1651: measurementJacobian_ekf_3didp
 * :1229-1353 or _1didp :1356-1478), gates the row pair with 2 degrees of freedom (:2457) and stacks what passed under
 * the MSCKF rows for ONE update (measurementUpdate_hybrid, :1766-1950).  The rows come in the compact form of those
 * functions' outputs; gate and stacking happen on the device.  Call order: set_option(ORCVIO_OPT_EXTRA_STATES, k),
 * set_option(ORCVIO_OPT_EKF_ROWS, 1), upload(...) [P is (LEG+6N+k)^2], upload_ekf_rows, run_update, download,
 * download_ekf.  The rows belong to the upload they follow.  New features (the H_1 / H_2 initialisation) stay with the
 * caller. */
typedef struct orcvio_msckf_ekf_rows {
    int32_t n_features;
    int32_t idp_dim;         /* feature_idp_dim: 3 (invParam) or 1 (invDepth)                               */
    const int32_t* anchor;   /* [F] anchor clone (index in the window, Feature::id_anchor)                  */
    const int32_t* state;    /* [F] observing clone (state_server.imu_state.id)                             */
    const int32_t* slot;     /* [F] position in feature_states: columns LEG + 6N + idp_dim*slot ...         */
    const double* H_e;       /* [F][2][6]  -> columns 15..20 (:1641)                                        */
    const double* H_a;       /* [F][2][6]  -> the anchor clone (:1639)                                      */
    const double* H_x;       /* [F][2][6]  -> the observing clone (:1640)                                   */
    const double* H_f;       /* [F][2][idp_dim] -> the feature's own columns (:1630, :1636)                 */
    const double* z_vel;     /* [F][2] observations_vel -> column 21 under estimate_td (:1642), else unused  */
    const double* r;         /* [F][2]                                                                      */
} orcvio_msckf_ekf_rows;
int32_t orcvio_msckf_upload_ekf_rows(orcvio_msckf_handle* h, const orcvio_msckf_ekf_rows* rows);
/* ... or the SLAM features themselves: the four blocks are then evaluated on the device (measurementJacobian_ekf_3didp,
 * src/orcvio.cpp:1229-1353, / _1didp, :1356-1478) from the window poses already uploaded -- observations in, delta_x out.
 * Same call order, this call instead of orcvio_msckf_upload_ekf_rows. */
typedef struct orcvio_msckf_slam_features {
    int32_t n_features;
    int32_t idp_dim;          /* feature_idp_dim: 3 or 1                                                     */
    const int32_t* anchor;    /* [F] Feature::id_anchor as a window index                                    */
    const int32_t* state;     /* [F] the observing clone (state_server.imu_state.id)                         */
    const int32_t* slot;      /* [F] position in feature_states                                              */
    const double* param;      /* [F][3] idp 3: Feature::invParam; idp 1: Feature::obs_anchor                 */
    const double* inv_depth;  /* [F]    idp 1: Feature::invDepth (NULL for idp 3)                            */
    const double* p_w;        /* [F][3] Feature::position                                                    */
    const double* p_fej;      /* [F][3] Feature::position_FEJ, read under if_fej (may be NULL otherwise)      */
    const double* z;          /* [F][2] observations[imu_state.id]                                           */
    const double* z_vel;      /* [F][2] observations_vel[imu_state.id], read under estimate_td               */
} orcvio_msckf_slam_features;
int32_t orcvio_msckf_upload_slam_features(orcvio_msckf_handle* h, const orcvio_msckf_slam_features* feats);
/* The gate alone, no update: gatingTestFeature (src/orcvio.cpp:1953-1976) of featureJacobian_msckf for every listed
 * track against the prior P -- the test the reference applies to a feature before it may enter the state as a SLAM
 * feature (:2361-2367).  gamma [F], accept [F]. */
int32_t orcvio_msckf_gate_tracks(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, const orcvio_msckf_window* window,
                                 const orcvio_msckf_tracks* tracks, const double* P, double* gamma, int32_t* accept);

/* Rows the caller has projected and gated itself, stacked under everything else as they are: H [n_rows][n] over the
 * WHOLE state (n = LEG + 6N + extra states; the first 15 columns must be zero, as for every feature row), r [n_rows].
 * This is how a frame that initialises NEW SLAM features keeps the heavy update on the device: the caller evaluates
 * featureJacobian_ekf_new and the W = [V | U] split of src/orcvio.cpp:2337-2436 (a few features, small), hands the
 * V-part rows (zero in the new features' columns) over here, and applies the reference's own H_1 / H_2 algebra
 * (:1811-1947) to the downloaded delta_x and covariance.  The rows belong to the upload they follow. */
int32_t orcvio_msckf_upload_dense_rows(orcvio_msckf_handle* h, int32_t n_rows, const double* H, const double* r);
/* New SLAM features in the 3-parameter form need no special rows when the MSCKF rows are LARVIO's (use_larvio = 1: the SLAM
 * rows' own error-state convention) and if_FEJ = 0: list them among the tracks (the V part of their rows is their MSCKF
 * block).  After the update, this call returns their correction and the augmented
 * covariance -- measurementUpdate_hybrid, src/orcvio.cpp:1811-1821 and :1904-1947, without nuisance states -- from what the
 * feature kernel left on the device for those tracks (host arithmetic on a few 3 x n blocks):
 *   track[j]      index of new feature j among the tracks of the last upload (it must have been accepted)
 *   anchor[j]     its anchor clone (window index);  inv_param [j][3] = Feature::invParam
 *   dx, P_upd     delta_x [n] and covariance [n][n] of the update just downloaded
 *   dx_new [3 n_new];  P_aug [(n + 3 n_new)^2] = [[P_upd, (-HH P)^T], [-HH P, P22]] */
int32_t orcvio_msckf_augment_new_features(orcvio_msckf_handle* h, const orcvio_msckf_window* window, int32_t n_new,
                                          const int32_t* track, const int32_t* anchor, const double* inv_param,
                                          const double* dx, const double* P_upd, double* dx_new, double* P_aug);
/* Host arithmetic for features entering the state, either parametrisation (no device involved):
 * orcvio_msckf_new_feature_rows -- featureJacobian_ekf_new (src/orcvio.cpp:1481-1572) for the listed features (CSR of ALL
 *   their observations; the 1-parameter form drops the anchor's own, :1494-1496) and the rotation by W = [V | U]
 *   (:2416-2436), one small Householder QR per feature.  H_top [*rows_top][n_cols], r_top: the V parts, for
 *   orcvio_msckf_upload_dense_rows (capacity: 2 x observations rows).  H_1 [d n_new][n_cols], H_2 [n_new][d][d], r_1.
 *   param: invParam (d = 3) or obs_anchor (d = 1); inv_depth: d = 1 only.  n_cols = state_cov.cols() before the update.
 * orcvio_msckf_augment_state -- the tail of measurementUpdate_hybrid (:1818-1821, :1904-1947, no nuisance states) from
 *   the delta_x [n] and covariance [n][n] of the update: dx_new [d n_new], P_aug [(n + d n_new)^2]. */
int32_t orcvio_msckf_new_feature_rows(const orcvio_msckf_flags* flags, const orcvio_msckf_window* window, int32_t idp_dim, int32_t n_cols,
                                      int32_t n_new, const int32_t* anchor, const double* param, const double* inv_depth,
                                      const double* p_w, const double* p_fej, const int32_t* obs_ptr, const int32_t* obs_clone,
                                      const double* obs_z, const double* obs_zvel, int32_t* rows_top, double* H_top, double* r_top,
                                      double* H_1, double* H_2, double* r_1);
int32_t orcvio_msckf_augment_state(int32_t n, int32_t n_new, int32_t idp_dim, const double* H_1, const double* H_2, const double* r_1,
                                   double sigma2, const double* dx, const double* P_upd, double* dx_new, double* P_aug);
/* ... or on the device (either parametrisation, FEJ, td): featureJacobian_ekf_new (src/orcvio.cpp:1481-1572) and the W = [V | U]
 * split (:2416-2436) for the features that enter the state, evaluated from the window poses of the upload they follow.  The V
 * parts are appended to the dense rows of that upload (behind those of orcvio_msckf_upload_dense_rows, if any) and take part in
 * the update; the U parts stay on the device until orcvio_msckf_download_new_feature_blocks fetches H_1 [d k][n], H_2 [k][d][d],
 * r_1 [d k] for orcvio_msckf_augment_state.  param: invParam (d = 3) or obs_anchor (d = 1); CSR of ALL observations of each
 * feature (the 1-parameter form drops the anchor's own, :1494-1496).  Call order: upload, [upload_slam_features],
 * [upload_dense_rows], upload_new_features, run_update, download, download_new_feature_blocks, augment_state. */
typedef struct orcvio_msckf_new_features {
    int32_t n_features;
    int32_t idp_dim;          /* feature_idp_dim: 3 or 1                                      */
    const int32_t* anchor;    /* [k] Feature::id_anchor as a window index                     */
    const double* param;      /* [k][3] idp 3: invParam; idp 1: obs_anchor                    */
    const double* inv_depth;  /* [k]    idp 1: invDepth (NULL for idp 3)                      */
    const double* p_w;        /* [k][3] Feature::position                                     */
    const double* p_fej;      /* [k][3] Feature::position_FEJ, read under if_fej              */
    const int32_t* obs_ptr;   /* [k+1] CSR over the features' observations                    */
    const int32_t* obs_clone; /* [nobs] window index of the observing state                   */
    const double* obs_z;      /* [nobs][2]                                                    */
    const double* obs_zvel;   /* [nobs][2], read under estimate_td                            */
} orcvio_msckf_new_features;
int32_t orcvio_msckf_upload_new_features(orcvio_msckf_handle* h, const orcvio_msckf_new_features* feats);
int32_t orcvio_msckf_download_new_feature_blocks(orcvio_msckf_handle* h, double* H_1, double* H_2, double* r_1);
/* Schmidt-EKF (ORCVIO_OPT_SCHMIDT_STATES): poses of the nuisance states (state_server.nui_imu_states), after orcvio_msckf_upload;
 * nui->n_clones must equal the option's value. */
int32_t orcvio_msckf_upload_nuisance_poses(orcvio_msckf_handle* h, const orcvio_msckf_window* nui);
/* orcvio_msckf_augment_state with nui_rows nuisance rows at the end of the state: the new feature states are inserted in front
 * of them (src/orcvio.cpp:1920-1935); P_aug in the order [old | new | nuisance]. */
int32_t orcvio_msckf_augment_state_nuisance(int32_t n, int32_t n_new, int32_t idp_dim, int32_t nui_rows, const double* H_1, const double* H_2,
                                            const double* r_1, double sigma2, const double* dx, const double* P_upd, double* dx_new,
                                            double* P_aug);
/* orcvio_msckf_augment_state_nuisance (nui_rows may be 0) with the reference's LITERAL `H_2.ldlt().solve(..)` for HH and dx_new
 * (src/orcvio.cpp:1826-1827: an LDLT of the lower triangle of the upper-triangular H_2, i.e. division by its diagonal); see
 * ORCVIO_OPT_REF_H2_LDLT.  Differs from the corrected form for feature_idp_dim = 3 only. */
int32_t orcvio_msckf_augment_state_ref_ldlt(int32_t n, int32_t n_new, int32_t idp_dim, int32_t nui_rows, const double* H_1, const double* H_2,
                                            const double* r_1, double sigma2, const double* dx, const double* P_upd, double* dx_new,
                                            double* P_aug);
/* gamma[F], accept[F] of the SLAM features of the last update (either may be NULL) */
int32_t orcvio_msckf_download_ekf(orcvio_msckf_handle* h, double* gamma, int32_t* accept);

/* Feature update: replaces the loop + compression + update of
 * OrcVIO::removeLostFeatures (src/orcvio.cpp:2497-2560) and of
 * OrcVIO::pruneImuStateBuffer (:2803-2851): featureJacobian_msckf ->
 * nullspace_project_inplace_svd -> gatingTestFeature -> stack -> QR compression ->
 * measurementUpdate_{hybrid(pure MSCKF case),msckf}.  Host buffers in, host buffers out;
 * P is n x n with n = leg_dim + 6*n_clones, symmetric: outside the diagonal 16 x 16 tiles only the upper
 * entries are read (Conventions; n odd: all of them). */
int32_t orcvio_msckf_update_features(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags,
                                     const orcvio_msckf_window* window,
                                     const orcvio_msckf_tracks* tracks, const double* P,
                                     orcvio_msckf_result* result);

/* ---- The same update without the copies: the handle's pinned arena, written and read in place ------------------------------
 * SURVEY.md 8d measures the update from "flat inputs in host memory" to "delta_x, P+ in host memory".  orcvio_msckf_update_features
 * copies the caller's arrays into the handle's pinned input arena and the results out of its pinned output block; a caller that
 * flattens its containers (StateServer / MapServer, src/orcvio.cpp:2497-2527, :2803-2848) STRAIGHT INTO the arena and reads the
 * results where they land saves both copies (326 KB of P each way at 30 clones).
 *   io_begin   lays the arena out for (n_clones, n_features, n_observations; with_P = 0: the prior is the resident covariance; 2: ... as the propagation and
 *              augmentation of orcvio_msckf_io_step_frame will leave it, for that call)
 *              and returns the pointers.  Inputs, to be written by the caller: poses [N][ORCVIO_POSE_STRIDE] (one record per
 *              clone: R_b2w 9 row-major | t_b_w 3 | t_fej 3 | R_b2c 9 | t_c_b 3 | 1 unused), p_w [F][3], obs_ptr [F+1] (CSR,
 *              obs_ptr[F] == n_observations), obs_clone, obs_z [nobs][2], obs_zvel [nobs][2] (NULL unless flags->estimate_td),
 *              P [n][n] (NULL when with_P == 0).  Outputs, valid after io_update returns ORCVIO_OK and until the next call on
 *              the handle that takes tracks: dx [n], gamma [F], accept [F], P_out [n][n] (written only with want_P).
 *   io_update  validates what stands in the arena (the index arrays, as orcvio_msckf_upload does), and runs the update: ONE
 *              launch of a captured graph that pulls the arena into HBM and whose last kernel pushes the results
 *              into the (host-coherent) output block and raises a flag word there; the calling thread spins on that word -- no
 *              copy-engine transfer, no stream synchronisation.  The arena is read until that launch has ENDED, not by its first
 *              kernel alone: the index lists the library derives from the caller's arrays stay in the arena and the tracks' kernel
 *              reads them there (orcvio_msckf_counters [11]), so the arena is the caller's to write again when io_update (or
 *              io_collect) has returned, not before.  commit != 0: orcvio_msckf_cov_commit is part of the same launch
 *              (P+ and its square-root factor become resident; refused on the device if the update is).  stats as in
 *              orcvio_msckf_result.  The same arena may be updated again (next frame, same sizes) without a new io_begin.
 * Status codes as orcvio_msckf_update_features; ORCVIO_ERR_TIMEOUT if the results were never published. */
#define ORCVIO_POSE_STRIDE 28
typedef struct orcvio_msckf_io {
    int32_t n;            /* leg_dim + 6 n_clones (+ extra states) */
    double* poses;
    double* p_w;
    int32_t* obs_ptr;
    int32_t* obs_clone;
    double* obs_z;
    double* obs_zvel;
    double* P;            /* n x n, symmetric; of the entries outside the diagonal 16 x 16 tiles the update reads the upper ones only
                             (floor(j/16) > floor(i/16)): the lower ones need not be written (Conventions; n odd: all are read) */
    const double* dx;
    const double* gamma;
    const int32_t* accept;
    const double* P_out;
} orcvio_msckf_io;
int32_t orcvio_msckf_io_begin(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int32_t n_clones, int32_t n_features,
                              int32_t n_observations, int32_t with_P, orcvio_msckf_io* io);
int32_t orcvio_msckf_io_update(orcvio_msckf_handle* h, int32_t want_P, int32_t commit, int32_t* stats /* [8] or NULL */);
/* The same in two halves, for a caller with work of its own to do meanwhile (the next image, the object mapper's reply):
 *   io_submit   validates the arena and LAUNCHES the update (returns after ~20 us of host time; nothing is waited for)
 *   io_collect  waits for the results (the flag word) and reports the outcome exactly as io_update does
 * Between the two calls the handle must not be used for anything else, and the arena must not be written.
 * Hybrid filter: the rows of the in-state features (orcvio_msckf_upload_slam_features / _upload_ekf_rows, with ORCVIO_OPT_EKF_ROWS and
 * ORCVIO_OPT_EXTRA_STATES set) may be handed over between io_begin and io_update / io_submit; they ride in the same launch. */
int32_t orcvio_msckf_io_submit(orcvio_msckf_handle* h, int32_t want_P, int32_t commit);
int32_t orcvio_msckf_io_collect(orcvio_msckf_handle* h, int32_t* stats /* [8] or NULL */);


/* Object update: replaces OrcVIO::removeLostObjects (src/orcvio.cpp:2154-2193) for one
 * object block (nullspace projection against Hf -> gate with dof = rows -> NaN check ->
 * measurementUpdate_msckf).  result->accept/gamma have length 1. */
int32_t orcvio_msckf_update_objects(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags,
                                    int32_t n_clones, const orcvio_msckf_object_rows* rows,
                                    int32_t n_objects, const double* P,
                                    orcvio_msckf_result* result);

/* Object residual rows at a fixed state: the CameraLM / ObjectLM functor evaluation exported by
 * ObjectFeatureInitializer::single_levenberg_marquardt (src/obj/ObjectFeatureInitializer.cpp:394-434; functors
 * src/obj/ObjectResJacCam.cpp:153-519, src/obj/ObjectLM.cpp:250-632) followed by
 * OrcVIO::constructObjectResidualJacobians (src/orcvio.cpp:2017-2151), evaluated on the device.  Output rows are
 * interleaved per in-window frame [keypoint rows ; 4 bbox rows] and can be passed to
 * orcvio_msckf_update_objects as they are.  The state at which the rows are evaluated is the caller's: the optimum of
 * orcvio_msckf_object_lm below (the LM solver on the device), or one the caller has found by other means.
 * The rows are evaluated with UNIT residual weights and the Huber loss OFF: the functors' `residual_weight` and
 * `use_valid` / huber arguments (src/obj/ObjectResJacCam.cpp:535, 567-576; src/obj/ObjectLM.cpp:775-811) are ones / infinity
 * at every shipped call site (include/orcvio/obj/ObjectFeatureInitializer.h:40, ObjectLM.h:301), so no entry point exposes them. */
typedef struct orcvio_object_eval_flags {
    int32_t use_left_perturbation;      /* the object mapper's flag (ObjectInitNode.cpp:140)             */
    int32_t use_new_bbox_residual;      /* use_new_bbox_residual_flag (:206).  1: the reference's rows LITERALLY -- its Jacobians take the
                                           plane in the world frame (src/obj/ObjectResJacCam.cpp:405,446) although the residual uses the
                                           object frame, and the shape derivative lacks -sign(b4) (src/obj/ObjectLM.cpp:602-603): SURVEY
                                           note N8, the parity target.  2 (opt-in): the same residual with CORRECTED Jacobians (plane in
                                           the object frame, sign restored), which match central differences to 1e-9 */
    int32_t vio_use_left_perturbation;  /* the filter's flag: selects D (src/orcvio.cpp:2092)            */
    int32_t fix_dcampose_dimupose_to_identity; /* OrcVIO::fixDcamposeDimuposeToI (orcvio.h:115-119)      */
    double R_b2c[9];                    /* current extrinsics: state_server.imu_state.R_imu_cam0         */
    double t_c_b[3];                    /*                      state_server.imu_state.t_cam0_imu         */
} orcvio_object_eval_flags;

typedef struct orcvio_object_track {
    int32_t n_keypoints;        /* K (12 for the car class, config/object_feat_unity.yaml).  K = 0: a BBOX-ONLY track -- object state
                                   [pose 6 | shape 3], four bbox rows per in-window frame (src/obj/ObjectResJacCam.cpp:308-519 alone), H_f
                                   has 9 columns; kps / frame_zs are not read.  An EXTENSION (BASELINE config 5's "bbox-only OrcVIO-lite"
                                   read literally): the reference's lite mode sends no residuals at all (SURVEY note N4) */
    int32_t n_frames;
    const double* wTo;          /* [16] row-major object -> world                                        */
    const double* shape;        /* [3]  ellipsoid semi-axes                                              */
    const double* kps;          /* [K][3] keypoints in the object frame                                  */
    const double* frame_wTc;    /* [F][16] camera -> world of every frame (exp of valid_camera_pose_mat) */
    const double* frame_zs;     /* [F][K][2] normalised keypoint detections, NaN = not detected          */
    const double* frame_bbox;   /* [F][4] xmin, ymin, xmax, ymax (normalised)                            */
    const int32_t* frame_clone; /* [F] window index of the clone with that exact timestamp, or -1 (:2073) */
} orcvio_object_track;

/* Returns ORCVIO_OK and *n_rows = 0 if no frame of the object is in the window (the reference returns false,
 * :2149).  Hf has 9 + 3K columns.  cap_rows bounds the caller's buffers. */
int32_t orcvio_msckf_object_rows_eval(orcvio_msckf_handle* h, const orcvio_object_eval_flags* flags,
                                      const orcvio_object_track* obj, int32_t cap_rows, int32_t* n_rows,
                                      int32_t* row_clone, double* Hx6, double* Hf, double* res);

/* The object optimiser: replaces ObjectFeatureInitializer::single_levenberg_marquardt (src/obj/ObjectFeatureInitializer.cpp:346-440)
 * for every object of a frame in ONE launch, one workgroup per object, the whole iteration on the device.
 *
 * Problem (ObjectLM::operator(), src/obj/ObjectLM.cpp:761-788; Huber off as above).  State x = (wTo, shape v, keypoints m_k), 9 + 3K
 * degrees of freedom in the column order [pose 6 | shape 3 | 3 per keypoint]; cost c = |r|^2 over, with F = n_frames,
 *   residual_weights[0] x the keypoint reprojection rows (a NaN detection is not a row),
 *   residual_weights[1] x the 4 bbox rows of every frame (use_new_bbox_residual 0 / 1 / 2 as in orcvio_object_eval_flags),
 *   residual_weights[2] x (m_k - mean_kps_k), repeated once per frame (ErrorDeformRegularization, :652-684),
 *   residual_weights[3] x (v - mean_shape),   repeated once per frame (ErrorQuadVRegularization, :732-743).
 * EVERY frame of the track is used, in the window or not: frame_clone is not read (it may be NULL).
 * Retraction: pose exp(xi) wTo (use_left_perturbation = 1) or wTo exp(xi) (0), xi = (upsilon, omega) in Sophus order; shape and
 * keypoints additive.  The start's wTo MUST BE RIGID (rotation block orthonormal to rounding, last row 0 0 0 1): the left and the
 * right iteration move a non-rigid matrix along different orbits (a float32 pose, orthonormal to 1e-7, ends 3e-5 apart).
 *
 * Iteration -- NOT MINPACK's trajectory (the reference's Eigen LM carries a custom scaled_norm): only the optimum is comparable.
 * With A = J^T J, g = J^T r:  D_j = max over the iterations so far of sqrt(A_jj);  (A + lambda D^2) delta = -g, lambda_0 = 1e-3;
 * pred = -2 g^T delta - delta^T A delta.  status 1 (converged) when pred <= ptol c, tested before the trial point is evaluated;
 * otherwise rho = (c - c+) / pred: accepted if rho > 1e-4 with lambda <- max(lambda max(1/3, 1 - (2 rho - 1)^3), 1e-12), else
 * lambda <- 4 lambda.  status 2 (stalled) when lambda > 1e12; status 3 after max_iter solves; status 4 when a number stops being
 * finite or a pivot of the damped system is not positive (the last accepted state is returned).  A keypoint detected in no frame
 * has only its regulariser and stays at its mean (it needs residual_weights[2] > 0).
 *
 * Limits: 1 <= K <= 16 (K = 0 is refused here: the reference's lite mode is another functor, orcvio_msckf_object_lm_lite below), 1 <= F <= 128,
 * n_tracks <= the handle's max_features, max_iter 1..100000.  A violation or a non-finite input (start, prior, camera pose, bbox,
 * config) returns ORCVIO_ERR_INVALID / ORCVIO_ERR_CAPACITY before anything is enqueued.  A per-object status other than 1 is NOT an
 * error of the call.  Synchronous: one launch, one wait; staging of its own -- neither the resident covariance nor the arena of an
 * open orcvio_msckf_io_begin is touched.
 *
 * Intended sequence: point a track's wTo / shape / kps at the arrays of its result and pass the SAME track records to
 * orcvio_msckf_update_object_tracks (or to orcvio_msckf_object_rows_eval for the reference's fvec_all / fjac_*). */
typedef struct orcvio_object_lm_config {
    int32_t use_left_perturbation, use_new_bbox_residual;
    double  residual_weights[4];
    int32_t max_iter;
    double  ptol;
} orcvio_object_lm_config;

/* weights 1, 1, 1, 1; max_iter 60; ptol 1e-18; left perturbation; the old bbox residual */
void orcvio_msckf_object_lm_config_default(orcvio_object_lm_config* cfg);

typedef struct orcvio_object_lm_prior {
    const double* mean_shape;   /* [3]     */
    const double* mean_kps;     /* [K][3]  */
} orcvio_object_lm_prior;

typedef struct orcvio_object_lm_result {
    double* wTo;                /* [16]   caller-owned, as are shape [3] and kps [K][3] */
    double* shape;
    double* kps;
    double cost0, cost;         /* |r|^2 at the start and at the returned state */
    int32_t iterations;         /* damped solves that went on to a trial point (accepted or not) */
    int32_t evaluations;        /* evaluations of the cost (the start's included) */
    int32_t status;             /* 1 converged, 2 stalled, 3 iteration cap, 4 non-finite */
} orcvio_object_lm_result;

int32_t orcvio_msckf_object_lm(orcvio_msckf_handle* h, const orcvio_object_lm_config* cfg,
                               const orcvio_object_track* tracks, const orcvio_object_lm_prior* priors,
                               int32_t n_tracks, orcvio_object_lm_result* results);

/* The start of an object track: replaces ObjectFeatureInitializer::single_object_initialization
 * (src/obj/ObjectFeatureInitializer.cpp:33-198) for every object of a frame in ONE launch (k_object_init, one workgroup per object).
 *
 * Keypoints.  Keypoint k is USED if the number of frames in which both of its coordinates are finite is strictly greater than
 * min_obs (ObjectFeature.cpp:118).  A used keypoint is triangulated linearly over those frames (single_triangulation_common,
 * src/feat/FeatureInitializer.cpp:6-111): anchor = the LAST of them (per keypoint), rows Bperp_i p = Bperp_i p_CiinA, solved by the
 * normal equations (the reference: a pivoted QR; forward error cond(A)^2 eps instead of cond(A) eps), p_FinG = R_GtoA^T p + p_AinG;
 * kp_cond = cond(A), the reference's condA.
 * Alignment.  If the number of used keypoints is strictly greater than min_kps, findTransform (:265-344) over the used keypoints in
 * increasing id: scale = ratio of the summed chords between CONSECUTIVE used keypoints, Cov = in out^T of the centred sets
 * (out divided by scale), its 3 x 3 SVD (one-sided Jacobi on the device), R = V diag(1, 1, sign det(V U^T)) U^T,
 * t_kabsch = scale (out_ctr / scale - R in_ctr).  The reference's literal result [scale R | t_kabsch] is NOT rigid; it is returned
 * in pieces (R_kabsch, t_kabsch, scale; sigma = the singular values of Cov) and wTo is one of three RIGID forms:
 *   pose_form 1  the reference as shipped (estimate_SE2_pose_flag = true, poseSE32SE2, se3_ops.hpp:272-300):
 *                yaw = pi / atan2(T10, T00), 0 if that is not finite; translation (t_kabsch x, t_kabsch y, 0);
 *   pose_form 2  the same with yaw = atan2(T10, T00) (opt-in correction, as use_new_bbox_residual = 2 is);
 *   pose_form 0  rigid SE(3): R_kabsch and out_ctr - R in_ctr on the unscaled points (an extension).
 * status 1 initialised; 2 too few usable keypoints (wTo = identity, as the reference returns); 4 a number stopped being finite
 * (wTo = identity).  No conditioning threshold is applied: sigma and kp_cond are reported, the caller judges.
 *
 * Of a track, n_keypoints, n_frames, frame_wTc and frame_zs are read; wTo, shape, kps, frame_bbox and frame_clone are not and may
 * be NULL.  Limits and refusals as orcvio_msckf_object_lm's (1 <= K <= 16, 1 <= F <= 128, n_tracks <= max_features, null pointers,
 * a non-finite camera pose or mean keypoint; pose_form outside 0..2, a negative threshold), before anything is enqueued.  A NaN
 * detection is data.  Synchronous: one upload, one launch, one download, one wait, on the optimiser's own staging. */
typedef struct orcvio_object_init_config {
    int32_t pose_form, min_obs, min_kps;
} orcvio_object_init_config;

/* the reference's values: pose_form 1, min_obs 3, min_kps 3 */
void orcvio_msckf_object_init_config_default(orcvio_object_init_config* cfg);

typedef struct orcvio_object_init_result {
    double* wTo;                /* [16]    caller-owned, as are the four arrays below                                */
    double* kps_world;          /* [K][3]  valid_shape_global_frame; NaN where the keypoint is not used              */
    int32_t* kp_used;           /* [K]     1 / 0                                                                     */
    int32_t* kp_obs;            /* [K]     frames with a finite detection                                            */
    double* kp_cond;            /* [K]     cond(A) of the triangulation; NaN where the keypoint is not used          */
    double R_kabsch[9], t_kabsch[3], scale;   /* the reference's literal matrix is [scale R_kabsch | t_kabsch]       */
    double sigma[3];            /* singular values of Cov, descending                                                */
    int32_t n_used;
    int32_t status;             /* 1 initialised, 2 too few usable keypoints, 4 non-finite                           */
} orcvio_object_init_result;

/* mean_kps_per_track [n_tracks]: pointers to [K][3], the class's mean keypoints in the object frame */
int32_t orcvio_msckf_object_init(orcvio_msckf_handle* h, const orcvio_object_init_config* cfg,
                                 const orcvio_object_track* tracks, const double* const* mean_kps_per_track,
                                 int32_t n_tracks, orcvio_object_init_result* results);

/* Initialisation and optimisation in ONE call: packs and uploads once, k_object_init writes each track's start (its wTo, the mean
 * shape, the mean keypoints: the reference's LMObjectState start) into the staged block, k_object_lm follows on the same stream, both
 * result blocks come back in one download behind one wait.  An object whose initialisation did not end with status 1 is not
 * optimised: its LM status is 0, its LM arrays hold the identity, the mean shape and the mean keypoints, its costs and counters 0.
 * The tracks' wTo, shape, kps and frame_clone are not read and may be NULL; frame_bbox is.  Equal, bit for bit, to
 * orcvio_msckf_object_init followed by orcvio_msckf_object_lm from its wTo and the means. */
int32_t orcvio_msckf_object_init_lm(orcvio_msckf_handle* h, const orcvio_object_init_config* init_cfg,
                                    const orcvio_object_lm_config* lm_cfg, const orcvio_object_track* tracks,
                                    const orcvio_object_lm_prior* priors, int32_t n_tracks,
                                    orcvio_object_init_result* init_results, orcvio_object_lm_result* lm_results);

/* ---- the LITE object mapper: bbox-only tracks (n_keypoints = 0), the reference's use_bbox_only_flag branch ----
 * Replaces ObjectFeatureInitializer::single_object_initialization_lite (src/obj/ObjectFeatureInitializer.cpp:495-584) and
 * single_levenberg_marquardt_lite (:442-493, the ObjectLMLite functor: src/obj/ObjectLMLite.cpp) for every object of a frame at once.
 * What comes back goes into orcvio_msckf_update_object_tracks as a track with n_keypoints = 0.
 *
 * The optimiser (orcvio_msckf_object_lm_lite; k_object_lm_lite: one WAVEFRONT per object, no workgroup barrier, no LDS).
 * Problem (ObjectLMLite::operator(), ObjectLMLite.cpp:389-415; Huber off).  State x = (wTo, shape v): 9 degrees of freedom in the
 * column order [pose 6 | shape 3]; cost c = |r|^2 over, with F = n_frames,
 *   residual_weights[0] x the 4 bbox rows of every frame (the rows of orcvio_msckf_object_lm; use_new_bbox_residual 0 / 1 / 2),
 *   residual_weights[1] x (v - mean_shape), repeated F - 1 times: the reference LITERALLY (include/orcvio/obj/ObjectLMLite.h:288-297,
 *                         NErrors = 3 (zb.size() - 1) under a "TODO FIXME why -1"), so a one-frame track has no regulariser;
 *                         reg_every_frame = 1 (opt-in correction, as use_new_bbox_residual = 2 is): F times.
 * The two weights are in the REFERENCE'S OWN ORDER: ObjectLMLite reads the initialiser's four-vector from index 0, so the bbox rows
 * get residual_weights(0) and the regulariser residual_weights(1) -- not the (1) and (3) of the full functor.  Every shipped call
 * site passes ones.  Retraction and iteration: exactly those of orcvio_msckf_object_lm (lambda_0 = 1e-3, the running-maximum
 * scaling D, pred, the rho rule, status 1..4), on the 9 x 9 system.  The start's wTo must be rigid.
 * The bbox-only optimum is NOT unique in wTo (the ellipsoid is invariant under the half-turns about its axes); the cost depends on
 * wTo diag(v^2, -1) wTo^T, which is what two runs can be compared by.
 * Of a track, n_keypoints (must be 0), n_frames, wTo, shape, frame_wTc and frame_bbox are read; kps, frame_zs and frame_clone are
 * not and may be NULL.  Of a prior, mean_shape; mean_kps may be NULL.  Of a result, wTo and shape are written; kps may be NULL and is
 * not written: a lite track has no keypoints (the reference's lite state zeroes its keypoints on the first step,
 * ObjectLMLite.cpp:74-90, so its object_keypoints_shape_global_frame is the object origin repeated).
 * Limits: n_keypoints = 0, 1 <= F <= 128, n_tracks <= max_features, max_iter 1..100000; a violation, a null pointer or a non-finite
 * pose, box, mean or config value returns ORCVIO_ERR_INVALID / ORCVIO_ERR_CAPACITY before anything is enqueued.  A batch equals one
 * object per call bit for bit.  Synchronous, on the optimiser's own staging. */
typedef struct orcvio_object_lite_config {
    int32_t use_left_perturbation, use_new_bbox_residual;
    double  residual_weights[2];    /* bbox rows, shape regulariser */
    int32_t reg_every_frame;        /* 0: F - 1 repeats of the regulariser (the reference); 1: F */
    int32_t max_iter;
    double  ptol;
} orcvio_object_lite_config;

/* weights 1, 1; reg_every_frame 0; max_iter 60; ptol 1e-18; left perturbation; the old bbox residual */
void orcvio_msckf_object_lite_config_default(orcvio_object_lite_config* cfg);

int32_t orcvio_msckf_object_lm_lite(orcvio_msckf_handle* h, const orcvio_object_lite_config* cfg,
                                    const orcvio_object_track* tracks, const orcvio_object_lm_prior* priors,
                                    int32_t n_tracks, orcvio_object_lm_result* results);

/* The start (orcvio_msckf_object_init_lite; k_object_init_lite: one thread per object), from the FIRST frame alone:
 * (R_GtoA, p_AinG) = frame 0's camera, A = diag((mean_shape o bbox_scale)^2), the four lines l of frame 0's box in the scale
 * poly2lineh(bbox2poly(.)) gives them (the bbox rows' lines; the ratio is not invariant to a per-line scaling), b = (cx, cy, 1) the
 * box's centre, B = R_GtoA:
 *   d = 1 / sqrt( b^T (sum l l^T) b / sum l^T B A B^T l ),   wPq = d B^T b + p_AinG,   rotation = identity.
 * pose_form as in orcvio_msckf_object_init: 1 = poseSE32SE2 as shipped (on an identity rotation: yaw 0, translation (x, y, 0)),
 * 2 coincides with 1 here, 0 keeps the full translation.  status 1, or 4 when wPq is not finite (the reference's allFinite; wTo =
 * identity).  d is returned with the pose.  Only n_keypoints (must be 0), n_frames, frame_wTc[0], frame_bbox[0] and the mean shape
 * are read.  Limits and refusals as orcvio_msckf_object_lm_lite's; pose_form outside 0..2 or a non-finite bbox_scale is refused. */
typedef struct orcvio_object_init_lite_config {
    int32_t pose_form;
    double  bbox_scale[3];          /* the reference's empirical_bbox_scale: ones as shipped (.8, .6, .7 commented out for KITTI) */
} orcvio_object_init_lite_config;

/* pose_form 1, bbox_scale 1, 1, 1 */
void orcvio_msckf_object_init_lite_config_default(orcvio_object_init_lite_config* cfg);

typedef struct orcvio_object_init_lite_result {
    double* wTo;                    /* [16] caller-owned */
    double d;                       /* the depth along the centre ray */
    int32_t status;                 /* 1 initialised, 4 non-finite */
} orcvio_object_init_lite_result;

/* mean_shape_per_track [n_tracks]: pointers to [3] */
int32_t orcvio_msckf_object_init_lite(orcvio_msckf_handle* h, const orcvio_object_init_lite_config* cfg,
                                      const orcvio_object_track* tracks, const double* const* mean_shape_per_track,
                                      int32_t n_tracks, orcvio_object_init_lite_result* results);

/* Both in ONE call: packs and uploads once, k_object_init_lite writes each track's start (its wTo and the mean shape: the
 * reference's LMObjectStateLite start) into the staged block, k_object_lm_lite follows on the same stream, both result blocks come
 * back in one download behind one wait.  An object whose start failed (status 4) is not optimised: its LM status is 0, its LM
 * arrays hold the identity and the mean shape, its costs and counters 0.  The tracks' wTo and shape are not read and may be NULL.
 * Equal, bit for bit, to orcvio_msckf_object_init_lite followed by orcvio_msckf_object_lm_lite from its wTo and the mean shape. */
int32_t orcvio_msckf_object_init_lm_lite(orcvio_msckf_handle* h, const orcvio_object_init_lite_config* init_cfg,
                                         const orcvio_object_lite_config* lm_cfg, const orcvio_object_track* tracks,
                                         const orcvio_object_lm_prior* priors, int32_t n_tracks,
                                         orcvio_object_init_lite_result* init_results, orcvio_object_lm_result* lm_results);

/* ---- staged, device-resident form (what bench.py times; also the multi-GPU path) ----
 * upload:      copy window / tracks / P to the handle's device buffers (host -> HBM);
 * run_local:   Jacobians -> nullspace -> gate -> stacked [H'|r'] -> Gram compression.
 *              Leaves this rank's compressed block [A | b] ((n-14) x (n-14), symmetric,
 *              row-major, padded to a multiple of 16) in device memory;
 * block_ptr:   device pointer / element count of that block (for an RCCL all-gather);
 * run_finish:  sums `n_blocks` compressed blocks found at d_blocks (device pointer,
 *              consecutive, same size) and performs the Kalman solve: dx, P+ on device;
 * run_update:  run_local + run_finish on the handle's own block (single GPU);
 * download:    copy results to host buffers.
 * `stream` is a hipStream_t passed as void* (NULL = the handle's own stream). */
int32_t orcvio_msckf_upload(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags,
                            const orcvio_msckf_window* window, const orcvio_msckf_tracks* tracks,
                            const double* P);
int32_t orcvio_msckf_run_local(orcvio_msckf_handle* h, void* stream);
int32_t orcvio_msckf_block_ptr(orcvio_msckf_handle* h, double** d_block, int64_t* n_elems);
/* run_local writing the block straight into caller-owned device memory (e.g. the send buffer of the
 * all-gather), n_elems doubles as reported by block_ptr. */
int32_t orcvio_msckf_run_local_to(orcvio_msckf_handle* h, double* d_dst, void* stream);
int32_t orcvio_msckf_run_finish(orcvio_msckf_handle* h, const double* d_blocks, int32_t n_blocks,
                                void* stream);
int32_t orcvio_msckf_run_update(orcvio_msckf_handle* h, void* stream);
int32_t orcvio_msckf_sync(orcvio_msckf_handle* h, void* stream);
int32_t orcvio_msckf_download(orcvio_msckf_handle* h, orcvio_msckf_result* result);

/* Per-kernel device time of the last run_update, measured with HIP events on the launch
 * stream.  names[i] / ms[i] for i < *count (count in: capacity, out: filled). */
int32_t orcvio_msckf_profile_update(orcvio_msckf_handle* h, void* stream, int32_t reps,
                                    const char** names, double* ms, int32_t* count);

/* Per-stage device times of the last object update (ORCVIO_OPT_STAGE_PROFILE must be on): names[i] / ms[i] for
 * i < *count (count in: capacity, out: filled). */
int32_t orcvio_msckf_profile_stages(orcvio_msckf_handle* h, const char** names, double* ms, int32_t* count);

/* State correction: replaces OrcVIO::incrementState_IMUCam (src/orcvio.cpp:4468-4567).
 * Pure host arithmetic (15 + 6N small updates); returns 1 if the correction was applied,
 * 0 if the reference's large-update test discarded it. */
typedef struct orcvio_msckf_state {
    double R_b2w_imu[9]; /* current IMU orientation (row-major) */
    double v[3], p[3], bg[3], ba[3];
    double R_b2c[9], t_c_b[3]; /* extrinsics of the current IMU state */
    double td;
    double imu_intrinsics[24]; /* T1..M2 when leg_dim == 46 */
    int32_t n_clones;
    double* clone_R_b2w; /* [N][9] in/out */
    double* clone_t_b_w; /* [N][3] in/out */
    double* clone_R_c2w; /* [N][9] out: orientation_cam */
    double* clone_t_c_w; /* [N][3] out: position_cam    */
} orcvio_msckf_state;
int32_t orcvio_msckf_increment_state(const orcvio_msckf_flags* flags, const double* dx,
                                     orcvio_msckf_state* state);

/* ---- Object update in two halves (the multi-GPU form of orcvio_msckf_update_objects) -----------------
 * Objects are dealt across the ranks; P and the window are replicated.  objects_local leaves this rank's compressed
 * block [A' b'; b'^T c'] (NAP x NAP doubles, NAP = 16*ceil((6*n_clones + leg_dim - 14)/16)) in d_dst (device memory;
 * NULL = the handle's own block, orcvio_msckf_block_ptr) and reports the degrees of freedom of its usable objects;
 * the caller all-gathers the blocks and sums the dofs; objects_finish sums the blocks in rank order, solves, gates
 * jointly with dof_total (src/orcvio.cpp:2172-2176) and applies or discards the update; objects_download returns
 * accept[0], gamma[0], dx, P_out (and G on request). */
int32_t orcvio_msckf_objects_local(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int32_t n_clones,
                                   const orcvio_msckf_object_rows* objects, int32_t n_objects, const double* P,
                                   double* d_dst, int32_t* dof_out, void* stream);
int32_t orcvio_msckf_objects_finish(orcvio_msckf_handle* h, const double* d_blocks, int32_t n_blocks,
                                    int32_t dof_total, void* stream);
int32_t orcvio_msckf_objects_download(orcvio_msckf_handle* h, orcvio_msckf_result* result);
/* Cumulative counters of the handle since orcvio_msckf_create (count <= ORCVIO_COUNTERS values are written):
 *   [0] front_fallbacks   updates whose fused front end (k_front, ORCVIO_OPT_FUSED_FRONT) or look-ahead solve (ORCVIO_OPT_LOOKAHEAD_SOLVE) lost
 *                         an in-launch hand-off: for k_front its co-residency bet -- a workgroup gave
 *                         up at the launch's device-wide counter because another tenant of the device (a second handle, another
 *                         stream's long kernel, another process) held compute units -- and were re-run on the forked seven-launch
 *                         path inside the same call.  The results are the same; each such update costs the bounded wait (tens of ms)
 *                         plus a second run.  A caller that sees this grow shares the device: set ORCVIO_OPT_FUSED_FRONT = 0
 *                         
 *   [1] launch sequences captured into a hipGraph   [2] replayed from one   [3] enqueued as plain launches
 *   [4] 1 while the communicator blocks the fused front end (ipc transport with ranks sharing this device)
 *   [5] 1 if the last object update from tracks compressed its objects in ONE launch (k_obj_fused: rows evaluated into LDS, never
 *       materialised; every object through the explicit basis), 0 if it took the three-launch pipeline over materialised rows
 *       (an object with two frames on one clone, more than 32 in-window frames or 16 keypoints, rows beyond the LDS staging,
 *       ORCVIO_OPT_OBJECT_REFINE = 0, ORCVIO_OPT_REF_STACK_HF, ORCVIO_OPT_OBJECT_QR = 0)
 *   [6] frames (orcvio_msckf_io_update_frame) whose object solve ran chained to the feature update's factor (ORCVIO_FRAME_CHAIN)
 *   [7] frame calls that found their object tracks staged ahead (orcvio_msckf_io_stage_object_tracks)
 *   [8] filter frames through orcvio_msckf_io_step_frame   [9] updates of such frames run again after a lost in-launch hand-off
 *   [10] pulls of a host P into device memory that moved its upper tile-trapezoid only and mirrored it on the device (n even; an odd
 *        n, possible with extra states, takes the linear pull of the whole matrix and is not counted)
 *   [11] in-place updates (orcvio_msckf_io_update / _io_submit, the copying orcvio_msckf_update_features) whose fused front end read the
 *        host-derived index lists (per-clone rows and positions) in the pinned arena itself instead of pulling them into device memory
 *        first: every such update but a materialised-stack one, the direct form of a thin stack, one armed by
 *        orcvio_msckf_io_triangulate, and one that takes the forked front end */
#define ORCVIO_COUNTERS 12
int32_t orcvio_msckf_counters(orcvio_msckf_handle* h, int64_t* counters, int32_t count);

/* Objects of the last downloaded object update (any entry point) whose projection against H_f went through the explicit basis
 * (ORCVIO_OPT_OBJECT_REFINE; math_utils.hpp:287-312 is the step it stands for): this rank's objects only. */
int32_t orcvio_msckf_objects_refined(orcvio_msckf_handle* h, int32_t* count);

/* The object update straight from object TRACKS (state at the LM optimum + observations; the structs of
 * orcvio_msckf_object_rows_eval): the residual rows and Jacobians of CameraLM::Error{Feature,BBox}Quadric /
 * ObjectLM::df and constructObjectResidualJacobians are evaluated on the device into the compact row arrays, so only
 * the tracks cross PCIe (a 12-keypoint car seen in 30 frames is 9 KB of input against 360 KB of rows).
 * objects_local_tracks is the sharded first half (followed by orcvio_msckf_objects_finish / _objects_download). */
int32_t orcvio_msckf_update_object_tracks(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags,
                                          const orcvio_object_eval_flags* eval_flags, int32_t n_clones,
                                          const orcvio_object_track* tracks, int32_t n_tracks, const double* P,
                                          orcvio_msckf_result* result);
int32_t orcvio_msckf_objects_local_tracks(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags,
                                          const orcvio_object_eval_flags* eval_flags, int32_t n_clones,
                                          const orcvio_object_track* tracks, int32_t n_tracks, const double* P,
                                          double* d_dst, int32_t* dof_out, void* stream);

/* The object tracks of the NEXT orcvio_msckf_io_update_frame call, scanned and staged ahead of it.  The caller has them before the
 * frame's feature update starts -- they come from the object mapper (ros_wrapper/src/orcvio/src/System.cpp:622-708), not from the
 * image -- so their packing into the handle's pinned staging arena (~14 us of host time for twenty objects) need not sit inside the
 * frame call, between the tracks' launch and the compression's: it is done here, as the feature tracks are written into the arena by
 * the caller before the call.  Call between orcvio_msckf_io_begin (with_P = 0; the window's clone count is taken from it) and
 * orcvio_msckf_io_update_frame, and hand the SAME `tracks` pointer, count, flags and eval flags to the frame call: anything else -- or
 * any other object call in between -- and the frame call stages for itself, as without this call (orcvio_msckf_counters [7] counts the
 * frames that found their tracks staged).  The track data are COPIED here: later changes to them are not seen by the frame call.
 * Results are the frame call's, bit for bit, either way. */
int32_t orcvio_msckf_io_stage_object_tracks(orcvio_msckf_handle* h, const orcvio_msckf_flags* object_flags,
                                            const orcvio_object_eval_flags* eval_flags, const orcvio_object_track* tracks, int32_t n_tracks);

/* ---- One frame in one call: the feature update, then the object update on the covariance it leaves -------------------------
 * System::imageCallback runs Estimator->processFeatures (its last update: OrcVIO::removeLostFeatures / pruneImuStateBuffer) and
 * then processObjects -> OrcVIO::removeLostObjects on the same state (ros_wrapper/src/orcvio/src/System.cpp:548-554).  This call
 * is orcvio_msckf_io_update(h, 0, commit = 1, ..) on what stands in the arena (orcvio_msckf_io_begin with with_P = 0: the prior
 * is the resident covariance) followed by orcvio_msckf_update_object_tracks(.., P = NULL, ..) -- same kernels, same results --
 * except that the object tracks' COMPRESSION (rows, structured QR, A': it depends on neither the prior nor the feature update)
 * runs on a stream of its own beside the feature update's solve, where the device is otherwise idle; only the object solve
 * waits for the feature update's commit.
 *   features   dx [n], gamma [F], accept [F] (caller-owned, each may be NULL) and stats; P_out / K / G / thin outputs must be NULL
 *   objects    as orcvio_msckf_update_object_tracks (dx, gamma[0], accept[0], stats; P_out / G are served by the two calls in
 *              sequence); commit_objects != 0: orcvio_msckf_cov_commit after an accepted object update
 * Status: a refused feature update (ORCVIO_ERR_NOT_SPD ..) returns its code and NOTHING of the frame is applied; a failure of the
 * object half returns its code with the feature update applied and committed (features->stats[3] says so).  After the call the
 * arena belongs to the object update: the next frame starts with orcvio_msckf_io_begin.  ORCVIO_FRAME_OVERLAP=0 (environment)
 * runs the two halves one behind the other. */
int32_t orcvio_msckf_io_update_frame(orcvio_msckf_handle* h, orcvio_msckf_result* features, const orcvio_msckf_flags* object_flags,
                                     const orcvio_object_eval_flags* eval_flags, const orcvio_object_track* tracks, int32_t n_tracks,
                                     int32_t commit_objects, orcvio_msckf_result* objects);

/* ---- One FILTER frame in one call: propagate, augment, update, prune update, marginalise -- on the resident covariance ---------
 * What OrcVIO::processFeatures does to state_cov per image (src/orcvio.cpp:567-594): batchImuProcessing -> processModel's
 * covariance propagation (:800-816), stateAugmentation (:962-1010), removeLostFeatures' update (:2497-2560), pruneImuStateBuffer's
 * update on the clones that leave (:2803-2851) and their marginalisation (:2874-2956).  As separate calls these are
 * cov_propagate, cov_augment, io_begin + upload_slam_features + io_update(commit), io_begin + io_update(commit), cov_remove_clones:
 * ~30 launches and copies and two host round trips per frame.  Here everything is enqueued at once on the handle's stream -- the
 * covariance never leaves HBM, the calling thread waits ONCE, for the flag word behind the last update -- with the small steps
 * folded into a few launches (frame_ops.hpp).  Same arithmetic in the same order as the separate calls: bit-identical results
 * (tests/test_gpu_stream.py).
 * Call order:  io_begin(flags, N, F, nobs, with_P = 2)   N = clones AFTER this frame's augmentation; with_P = 2: "the prior is the
 *                                                         resident covariance as this frame's propagation + augmentation leave it"
 *              the caller writes poses / tracks of the first update into the arena (as for io_update)
 *              io_step_frame(step, result)
 *   Phi, Q           [leg][leg] accumulated state transition and process noise of the IMU block (NULL, NULL: no propagation)
 *   augment          != 0: a clone is appended behind the window's clones (in front of the extra states)
 *   slam_features    hybrid filter (ORCVIO_OPT_EKF_ROWS): the in-state features the current state observes; NULL: none
 *   prune_tracks     the second update of the frame: observations of the clones that leave only (CSR, window indices, p_w given);
 *                    NULL: none.  Its window is the first update's, its prior what the first update commits.
 *   prune_apply_dx   != 0: the window poses of the second update are the arena's poses incremented by the first update's dx ON THE
 *                    DEVICE (incrementState_IMUCam, src/orcvio.cpp:4468-4567: clone orientation / position; every clone keeps its
 *                    own R_b2c / t_c_b, frozen at its augmentation; skipped when discard_large_update discards dx) -- what the
 *                    reference's state is when pruneImuStateBuffer runs;
 *                    0: the same poses as the first update (the caller's state increment does not reach into this call)
 *   remove_clones    window indices (ascending) of the clones marginalised at the end; n_remove <= 8
 * Not in this call: features ENTERING the state (orcvio_msckf_upload_new_features / _cov_commit_new_features change the state's dimension
 * between the updates: such frames take the separate calls), Schmidt nuisance poses, a communicator on the handle.  In-state features
 * that LEAVE the state or change anchor: orcvio_msckf_io_step_frame_ex below.
 * Results: pointers into the handle's pinned output blocks, valid until the next call on the handle that takes tracks.
 * Status: a validation failure returns its code with NOTHING done.  A refusal on the device (ORCVIO_ERR_NOT_SPD: M not positive definite or
 * non-finite input) of the first update refuses the second as well; the covariance bookkeeping of the frame (propagation, augmentation,
 * marginalisation) stands either way, stats[3] / prune_stats[3] say which updates were applied, n_after is the dimension left.  A lost
 * in-launch hand-off is repaired inside the call (the affected updates run again in separate launches; orcvio_msckf_counters [0]). */
typedef struct orcvio_msckf_frame_step {
    int32_t leg_dim;
    const double* Phi;
    const double* Q;
    int32_t augment;
    const orcvio_msckf_slam_features* slam_features;
    const orcvio_msckf_tracks* prune_tracks;
    int32_t prune_apply_dx;
    const int32_t* remove_clones;
    int32_t n_remove;
} orcvio_msckf_frame_step;
typedef struct orcvio_msckf_frame_result {
    int32_t stats[8];              /* first update, as orcvio_msckf_result.stats                        */
    int32_t prune_stats[8];        /* second update                                                     */
    const double* dx;              /* [n]                                                               */
    const double* gamma;           /* [F]                                                               */
    const int32_t* accept;         /* [F]                                                               */
    const double* prune_dx;        /* [n]   NULL without prune_tracks                                   */
    const double* prune_gamma;     /* [F2]                                                              */
    const int32_t* prune_accept;   /* [F2]                                                              */
    int32_t n_after;               /* dimension of the resident covariance when the call returns        */
    int32_t status_first;          /* ORCVIO_OK or the refusal of the first update                      */
    int32_t status_prune;          /* ... of the second                                                 */
    int32_t repaired;              /* updates of this frame that were run again after a lost hand-off   */
} orcvio_msckf_frame_result;
int32_t orcvio_msckf_io_step_frame(orcvio_msckf_handle* h, const orcvio_msckf_frame_step* step, orcvio_msckf_frame_result* result);

/* ---- Object update straight from the wire format of the object mapper ------------------------------
 * One element per orcvio_ros_msgs/ObjectLM message (ros_wrapper/src/orcvio_ros_msgs/msg/ObjectLM.msg) as ObjectInitNode fills it
 * (ros_wrapper/src/orcvio/src/ObjectInitNode.cpp:1180-1207): the export block of single_levenberg_marquardt
 * (src/obj/ObjectFeatureInitializer.cpp:394-434).  Matrices are the `data` arrays of the std_msgs/Float64MultiArray fields;
 * tf::matrixEigenToMsg writes them ROW-MAJOR (dim[0] = rows, dim[1] = cols).  The reference's System::msgToEigen maps that
 * buffer as COLUMN-major (System.cpp:710-723: SURVEY note N4, the object update could never have been right over ROS);
 * wire_row_major = 1 (default semantics: what the sender meant) reads the buffers as they were written, 0 reproduces msgToEigen
 * literally.  Rows are ordered [2 per valid keypoint of frame 0, frame 1, ... ; 4 bbox rows of frame 0, frame 1, ...].
 * orcvio_msckf_update_object_lm_msgs does, per message, OrcVIO::constructObjectResidualJacobians (src/orcvio.cpp:2017-2151:
 * exact timestamp match against cur_window_timestamps, D = get_cam_wrt_imu_se3_jacobian of SE3::exp(valid_camera_pose_mat
 * column) with the CURRENT extrinsics, rows re-interleaved per in-window frame; host arithmetic), then the stacking of
 * System::processObjects (System.cpp:684-702; per-object projection unless ORCVIO_OPT_REF_STACK_HF) and
 * OrcVIO::removeLostObjects (:2154-2193) on the device. */
typedef struct orcvio_object_lm_msg {
    int64_t object_id;
    int32_t n_rows;                          /* rows of residual / both Jacobians                                     */
    int32_t n_obj_cols;                      /* columns of jacobian_wrt_object_state (45 for a 12-keypoint class)     */
    int32_t n_frames;                        /* timestamps.size() == zs_num_wrt_timestamps.size() == pose columns      */
    const double* residual;                  /* [n_rows]                                                              */
    const double* jacobian_wrt_object_state; /* n_rows x n_obj_cols                                                   */
    const double* jacobian_wrt_sensor_state; /* n_rows x 6                                                            */
    const double* valid_camera_pose_mat;     /* 6 x n_frames: se3 log (upsilon, omega) of every frame's wTc           */
    const double* timestamps;                /* [n_frames]                                                            */
    const int32_t* zs_num_wrt_timestamps;    /* [n_frames] valid keypoints per frame                                  */
} orcvio_object_lm_msg;
int32_t orcvio_msckf_update_object_lm_msgs(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int32_t n_clones,
                                           const double* cur_window_timestamps /* [n_clones] */, const double* R_b2c /* [9] */,
                                           const double* t_c_b /* [3] */, int32_t fix_dcampose_dimupose_to_identity,
                                           int32_t wire_row_major, const orcvio_object_lm_msg* msgs, int32_t n_msgs, const double* P,
                                           orcvio_msckf_result* result);

/* ---- Multi-GPU: the handle owns an RCCL communicator (SURVEY.md 8b "handle owns ... RCCL comm", 8e) --------------------
 * One process per GPU, one handle per process.  The reference has no collectives; the callers this serves are the same
 * three call sites (OrcVIO::removeLostFeatures src/orcvio.cpp:2497-2560, ::pruneImuStateBuffer :2803-2851,
 * System::processObjects -> removeLostObjects ros_wrapper/src/orcvio/src/System.cpp:622-708), each rank holding a share of the
 * tracks / objects and ALL of the window and the prior.  Per update: local tracks -> local compressed block -> ONE
 * ncclAllGather of the blocks over xGMI -> rank-ordered sum (bit-identical on every rank) -> replicated Kalman solve, so
 * every rank ends with the same delta_x and P+ and nothing is broadcast back.
 *   comm_unique_id   rank 0: ncclGetUniqueId into id[ORCVIO_COMM_ID_BYTES]; the caller ships the bytes to the other ranks
 *                    by whatever channel it has (MPI, a TCP store, torch.distributed, a file)
 *   comm_init        ncclCommInitRank on the handle's device; allocates the gather buffer
 *   comm_destroy     (also done by orcvio_msckf_destroy)
 * RCCL (librccl.so.1) is loaded with dlopen on the first of these calls: a single-GPU caller never needs it.
 * A second transport behind the same calls: with ORCVIO_COMM_TRANSPORT=ipc in the environment of every rank the blocks travel by
 * direct stores into the peers' gather buffers (HIP IPC) announced through a shared-memory segment (ranks of ONE node;
 * comm_unique_id then returns 128 random bytes and RCCL is never loaded).  Unlike RCCL it accepts several ranks on one device
 * (INTEGRATION.md 7a).  It has run with several ranks on ONE device only: ranks on DIFFERENT devices are unverified
 * (no multi-GPU machine was available; the gather buffer is fine-grained / uncached and every pushing thread fences at system scope,
 * which is what the case needs on paper).  Its device-side wait for a peer's block gives up after
 * min(ORCVIO_COMM_TIMEOUT_S, ORCVIO_IPC_WAIT_S [default 20]) seconds: the update then reports ORCVIO_ERR_TIMEOUT (no update); a block
 * that arrives with another update's sequence number (a rank whose call count has slipped) reports ORCVIO_ERR_PEER. */
#define ORCVIO_COMM_ID_BYTES 128
int32_t orcvio_msckf_comm_unique_id(uint8_t* id /* [ORCVIO_COMM_ID_BYTES] */);
int32_t orcvio_msckf_comm_init(orcvio_msckf_handle* h, const uint8_t* id, int32_t rank, int32_t world);
int32_t orcvio_msckf_comm_destroy(orcvio_msckf_handle* h);
int32_t orcvio_msckf_comm_info(orcvio_msckf_handle* h, int32_t* rank, int32_t* world); /* world = 0: no communicator */
/* What the communicator is, for logs and benchmarks (count <= 8 values are written): out[0] transport (0 none, 1 RCCL, 2 ipc),
 * [1] rank, [2] world, [3] ranks_seen: slots of the last sharded update that carried their sender's own number behind the block
 * (= world when every rank's block arrived), [4] 1 if a peer shares this rank's device (ipc), [5] 1 if the ipc gather buffer is
 * fine-grained / uncached memory, [6] 1 if a peer runs on ANOTHER device under the ipc transport: that case is UNVERIFIED (the transport
 * has only ever run with several ranks on one device) and comm_init refuses it unless ORCVIO_IPC_XDEV=1 is set. */
int32_t orcvio_msckf_comm_details(orcvio_msckf_handle* h, int32_t* out, int32_t count);
/* Device time of the three parts of orcvio_msckf_run_update_sharded on THIS rank (HIP events on the handle's stream, medians over
 * `reps` updates of the uploaded share), microseconds: us[0] local tracks + compression, us[1] the exchange (the RCCL all-gather, or
 * the ipc push + signal + wait; the wait for the slowest peer is part of it), us[2] rank-ordered sum + replicated solve, us[3] the
 * whole update.  COLLECTIVE: every rank calls it with the same reps.  What bench.py --gpus N reports beside DESIGN.md 5's model. */
int32_t orcvio_msckf_profile_sharded(orcvio_msckf_handle* h, int32_t reps, double* us /* [4] */);
/* Bounded waits: nothing here hangs on a rank that never arrives.  comm_unique_id / comm_init give up after ORCVIO_COMM_TIMEOUT_S
 * seconds (environment, default 180) and return ORCVIO_ERR_TIMEOUT; so does every call below that waits for a stream carrying a
 * collective (comm_barrier, comm_allreduce_max, the one-shot sharded updates, orcvio_msckf_sync on a handle with a communicator) --
 * the communicator is then ABORTED (comm_info reports world = 0) and must be created again by all ranks.
 *   comm_barrier         everything enqueued on the handle's stream before is finished on EVERY rank when it returns
 *   comm_allreduce_max   values[i] <- max over the ranks, count <= 8 (e.g. the slowest rank's time of a timed region)
 * so that a process needs no second communicator (and no second RCCL stream) beside the handle's for its bookkeeping. */
int32_t orcvio_msckf_comm_barrier(orcvio_msckf_handle* h);
int32_t orcvio_msckf_comm_allreduce_max(orcvio_msckf_handle* h, double* values, int32_t count);
/* The sharded feature update.  run_update_sharded: staged form on the tracks of the last orcvio_msckf_upload (this rank's
 * share), results stay in HBM (orcvio_msckf_download fetches them).  update_features_sharded: host buffers in and out like
 * orcvio_msckf_update_features; `tracks` are THIS RANK's tracks, result->accept / gamma are theirs, result->dx / P_out are
 * the joint update's (identical on every rank); stats[0], [2] count this rank's accepted rows / tracks.
 * Every rank must make the same call in the same order (it contains a collective).
 * Errors and the collective: the window and the prior are replicated, so a refusal they cause (null argument, leg_dim, capacity of
 * the window, P == NULL without a matching resident covariance) hits every rank alike BEFORE the collective and every rank
 * returns it.  A refusal only THIS rank's share can cause (capacity, a track longer than ORCVIO_MAX_TRACK, an index out of range)
 * does not leave the others waiting: the rank takes part with an empty share and a status word behind its block, every rank
 * finishes the collective, the failing rank returns its own status, all others ORCVIO_ERR_PEER, and no rank has an update to
 * commit.  A HIP / RCCL failure between the local part and the collective (ORCVIO_ERR_HIP) cannot be repaired that way: the
 * other ranks run into the bounded wait (ORCVIO_ERR_TIMEOUT, communicator aborted).  An in-launch time-out AFTER the collective
 * (ORCVIO_ERR_TIMEOUT from download) is rank-local: that rank has no update, the others do -- treat it as fatal for the joint
 * filter. */
int32_t orcvio_msckf_run_update_sharded(orcvio_msckf_handle* h, void* stream);
int32_t orcvio_msckf_update_features_sharded(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags,
                                             const orcvio_msckf_window* window, const orcvio_msckf_tracks* tracks,
                                             const double* P, orcvio_msckf_result* result);
/* The sharded object update (System::processObjects): this rank's object tracks -> local block -> all-gather of the blocks
 * and of the local degrees of freedom -> joint gate with the total dof (src/orcvio.cpp:2172-2176) -> replicated solve. */
int32_t orcvio_msckf_update_object_tracks_sharded(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags,
                                                  const orcvio_object_eval_flags* eval_flags, int32_t n_clones,
                                                  const orcvio_object_track* tracks, int32_t n_tracks, const double* P,
                                                  orcvio_msckf_result* result);

/* ---- Feature triangulation --------------------------------------
 * Replaces, for every listed track, Feature::checkMotion followed by Feature::initializePosition
 * (include/orcvio/feat/feature.hpp:354-449; the Levenberg-Marquardt of ::triangulate_position, :583-719, with
 * ::generateInitialGuess :332-352, ::cost :270-290, ::jacobian :292-330) as called from
 * OrcVIO::removeLostFeatures (src/orcvio.cpp:2258-2270).  The tracks list the observations to use, in the order of
 * the reference's std::map (ascending clone); the caller has already dropped the current frame (curr_id).
 * The camera poses are the cached orientation_cam / position_cam of src/orcvio.cpp:954-961, formed from the window. */
typedef struct orcvio_triangulation_config { /* Feature::OptimizationConfig, feature.hpp:41-63 */
    double translation_threshold;     /* 0.2      */
    double huber_epsilon;             /* 0.01     */
    double estimation_precision;      /* 5e-7     */
    double initial_damping;           /* 1e-3     */
    int32_t outer_loop_max_iteration; /* 10       */
    int32_t inner_loop_max_iteration; /* 10       */
    double cost_threshold;            /* 4.7673e-4 */
    double init_final_dist_threshold; /* 5        */
} orcvio_triangulation_config;
void orcvio_msckf_triangulation_config_default(orcvio_triangulation_config* cfg);

enum { ORCVIO_TRI_NO_MOTION = 1, ORCVIO_TRI_NEG_DEPTH = 2, ORCVIO_TRI_BIG_PROJ = 4 };
typedef struct orcvio_triangulation_result { /* every pointer may be NULL */
    int32_t* valid;    /* [F] is_valid_solution */
    double* p_w;       /* [F][3] Feature::position (NaN where invalid and not initialised before) */
    double* inv_param; /* [F][3] Feature::invParam = (alpha, beta, rho) in the anchor (last listed) camera frame */
    int32_t* flags;    /* [F] ORCVIO_TRI_* bits: why a track is invalid (failed_by_neg_dpth, failed_by_big_proj) */
    double* cost;      /* [F] total squared reprojection error at the solution */
} orcvio_triangulation_result;
/* is_initialized: NULL, or [F]; where non-zero the track starts from tracks->p_w (feature.hpp:604-606) and the motion
 * check is skipped.  tracks->p_w may be NULL when is_initialized is NULL. */
int32_t orcvio_msckf_triangulate(orcvio_msckf_handle* h, const orcvio_triangulation_config* cfg,
                                 const orcvio_msckf_window* window, const orcvio_msckf_tracks* tracks,
                                 const int32_t* is_initialized, orcvio_triangulation_result* result);
/* The same on the tracks of the last orcvio_msckf_upload, in place on the device: valid tracks get their triangulated
 * position, the others are marked and take no part in the following orcvio_msckf_run_update (as the reference drops them
 * into invalid_feature_ids, src/orcvio.cpp:2262-2268).  Inputs never leave HBM between the two calls. */
int32_t orcvio_msckf_triangulate_uploaded(orcvio_msckf_handle* h, const orcvio_triangulation_config* cfg,
                                          const int32_t* is_initialized, void* stream);

/* The same INSIDE the in-place update: arms the NEXT update on the open arena (orcvio_msckf_io_update, _io_submit, or the
 * first update of orcvio_msckf_io_step_frame / _io_step_frame_ex) to triangulate its own tracks on the device, on the
 * update's stream behind the pull of the arena and in front of the first kernel that reads a position -- what
 * OrcVIO::removeLostFeatures does before it updates (src/orcvio.cpp:2258-2270, :2296-2312, :2325-2327).  Call it between
 * orcvio_msckf_io_begin and that update.  The arming holds for ONE update: the update consumes it, a later update on the same
 * arena is a plain one unless the call is made again; a new orcvio_msckf_io_begin drops it.
 *   mode[j]  ORCVIO_TRI_KEEP          the arena's p_w[j] is used as it is (the reference's is_initialized feature, :2260)
 *            ORCVIO_TRI_ALL           checkMotion + initializePosition over all listed observations (a lost feature)
 *            ORCVIO_TRI_ALL_BUT_LAST  the same over all but the LAST listed observation (if_tracked_now / curr_id,
 *                                     include/orcvio/feat/feature.hpp:358-359, :414): the newest observation enters the update,
 *                                     not the triangulation; a track with fewer than two observations left is ORCVIO_TRI_NO_MOTION
 *   mode == NULL: every track ORCVIO_TRI_ALL.
 * The arena's p_w of a track that is not KEEP is never read (it may hold anything, NaN included).  A track that fails takes
 * no part in the update, as behind orcvio_msckf_triangulate_uploaded: accept = 0, gamma = NaN, its rows count nowhere.
 * out: pointers into pinned host memory of the handle, filled when the update's own wait returns (no second wait, no
 * copy call) and valid until the next armed update or orcvio_msckf_destroy.  A KEEP track reports valid = 1, flags = 0, its
 * p_w echoed, NaN in inv_param and cost.
 * ORCVIO_ERR_INVALID, nothing armed and *out untouched: no open arena, a pending orcvio_msckf_io_submit, a mode outside
 * 0..2, a NULL or non-finite config (or negative iteration counts), an object update in the arena, a communicator on
 * the handle.  The prune update of the frame calls is armed by orcvio_msckf_io_triangulate_prune below
 * (initializePosition_AssignAnchor, :2782-2791, uses observations the prune tracks do not list). */
enum { ORCVIO_TRI_KEEP = 0, ORCVIO_TRI_ALL = 1, ORCVIO_TRI_ALL_BUT_LAST = 2, ORCVIO_TRI_ALL_MOTION_BUT_LAST = 3 };
typedef struct orcvio_msckf_io_tri {
    const int32_t* valid;     /* [F] 1: the track has a position (given or triangulated) and took part in the update */
    const int32_t* flags;     /* [F] ORCVIO_TRI_NO_MOTION / _NEG_DEPTH / _BIG_PROJ bits                              */
    const double* p_w;        /* [F][3] */
    const double* inv_param;  /* [F][3] */
    const double* cost;       /* [F]    */
} orcvio_msckf_io_tri;
int32_t orcvio_msckf_io_triangulate(orcvio_msckf_handle* h, const orcvio_triangulation_config* cfg,
                                    const int32_t* mode /* [F] or NULL */, orcvio_msckf_io_tri* out);

/* The same for the SECOND (prune) update of orcvio_msckf_io_step_frame / _io_step_frame_ex: what pruneImuStateBuffer does to a tracked
 * feature that is not initialised yet (src/orcvio.cpp:2776-2793) -- checkMotion(imu_states_augment, if_tracked), then
 * initializePosition_AssignAnchor over EVERY observation in the window, on the poses as the frame's first update has left them
 * (prune_apply_dx: incremented on the device by the first update's dx).  Call it between orcvio_msckf_io_begin and the frame call; it
 * holds for ONE frame, a new orcvio_msckf_io_begin drops it.  The launch goes behind the pose step and the pull of the second
 * update's tracks, in front of the first kernel of the prune update that reads a position.
 *   tri_tracks  track j of step->prune_tracks gets track j of tri_tracks: ALL its observations in the window (ascending clone,
 *               window indices, obs_z), the current image's included; p_w and obs_zvel are not read.  The list is COPIED into pinned
 *               staging of the handle by this call: the caller's memory need not outlive it.
 *   mode[j]     as above, and ORCVIO_TRI_ALL_MOTION_BUT_LAST (this call only): every listed observation in the triangulation, the
 *               motion check on the first and the SECOND-TO-LAST (feature.hpp:358-359, :451-500); of two listed observations the
 *               second-to-last is the first: no motion, ORCVIO_TRI_NO_MOTION, as in the reference.  mode == NULL: every track that
 *               mode.  ORCVIO_TRI_KEEP takes prune_tracks->p_w[j] (a feature that is initialised, :2782); the p_w of every other
 *               track is never read and may be NaN.
 * out: a SECOND pinned block of the handle (the first update's own arming keeps its block: both armings in one frame are allowed, and so
 * is this one beside orcvio_msckf_io_propagate_imu), filled when the frame's one wait returns and whatever becomes of the update (the
 * reference initialises the feature before it gates it).  inv_param is in the LAST listed camera's frame: id_anchor, invParam, invDepth
 * and obs_anchor follow from it.  A failing track takes no part in the prune update (prune_accept = 0, prune_gamma = NaN, no rows);
 * without a single valid track the prune update is refused on the device -- prune_stats[3] = 0, status_prune = ORCVIO_OK, P and its
 * factor bit for bit as the first update left them (used_IDs.size() != 0, :2804).
 * ORCVIO_ERR_INVALID, nothing armed and *out untouched: no open arena, a pending orcvio_msckf_io_submit, a NULL or non-finite config, a
 * mode outside 0..3, an index outside the window, clones not ascending within a track, a communicator on the handle.  A track longer
 * than ORCVIO_MAX_TRACK: ORCVIO_ERR_TRACK_TOO_LONG; more tracks or observations than the handle holds: ORCVIO_ERR_CAPACITY.
 * In the frame call (ORCVIO_ERR_INVALID, nothing done, the arming stands): armed but prune_tracks == NULL, tri_tracks->n_features !=
 * prune_tracks->n_features, a prune observation whose clone does not occur in its track's list. */
int32_t orcvio_msckf_io_triangulate_prune(orcvio_msckf_handle* h, const orcvio_triangulation_config* cfg,
                                          const orcvio_msckf_tracks* tri_tracks, const int32_t* mode /* [F2] or NULL */,
                                          orcvio_msckf_io_tri* out);

/* The choice of the two clones that leave, CHECKED inside orcvio_msckf_io_step_frame / _io_step_frame_ex.  The reference chooses them
 * (findRedundantImuStates, src/orcvio.cpp:2582-2626) in pruneImuStateBuffer, i.e. on position_cam / orientation_cam as
 * removeLostFeatures' update has just rewritten them (incrementState_IMUCam, :4535-4565).  A one-call frame is issued before that
 * update's dx exists, so its remove_clones -- and the prune_tracks that follow from them -- are a PREDICTION made on the poses from
 * before the update; near rotation_threshold / translation_threshold the prediction can differ from the reference's choice.  This call
 * arms the next frame call (between orcvio_msckf_io_begin and the frame call; it holds for ONE frame, a new orcvio_msckf_io_begin drops
 * it; allowed beside orcvio_msckf_io_propagate_imu and beside both triangulation armings): one small launch between the frame's two
 * updates evaluates the reference's loop on the poses the first update leaves and compares the result with remove_clones.
 *   window of N clones, key = N-4.  Iteration 1 compares clone N-3 with the key; taken (angle < rotation_threshold && distance <
 *   translation_threshold && tracking_ok): N-3 leaves, next N-2; not taken: the oldest clone leaves and the compared clone moves back by
 *   two, to N-5 (:2615-2618, as written).  Iteration 2 likewise.  Results, ascending: {N-3, N-2}, {0, N-3}, {0, N-5}, {0, 1}.
 *   distance = |position_cam(c) - position_cam(key)|; angle = the rotation angle of orientation_cam(c)^T orientation_cam(key) as Eigen
 *   3.3's AngleAxisd(Matrix3d) gives it (quaternion of the matrix, 2 atan2(|vec|, |w|)).
 *   dx applied (a committed first update, prune_apply_dx != 0, not discarded by discard_large_update): orientation_cam = R_b2w+
 *   R_imu_cam0+^T, position_cam = t_b_w+ + R_b2w+ t_cam0_imu+, the body pose as the frame's pose step leaves it, the extrinsic the one
 *   given HERE incremented by dx[15:21] (the IMU state's, not the clone's frozen one).  dx not applied (no first update, a refused one,
 *   a discarded dx, prune_apply_dx = 0): the reference's containers are untouched -- cam_poses are read as they are.
 * The choices AGREE: the frame is the unarmed frame bit for bit, except that its marginalisation is enqueued behind the frame's one wait
 * (and not waited for).  They DIFFER: the frame's second half -- anchor changes, prune update, marginalisation -- is held back on the
 * device: P and its factor stay bit for bit as the first update left them, status_prune = ORCVIO_OK, prune_stats[3] = 0,
 * status_changes = ORCVIO_OK with no new parameters to read, n_after is the dimension BEFORE the marginalisation, the frame call
 * returns ORCVIO_OK (a disagreement is not an error), and `chosen` names the clones to run that half again with (a frame call without
 * propagation, augmentation and first update that carries prune_tracks, the events' changes and remove_clones).
 * Divergence: N >= 6 is required.  At N = 5 clone N-5 IS the oldest and the reference's own loop can name clone 0 twice.
 * ORCVIO_ERR_INVALID, nothing armed: no open arena, a pending orcvio_msckf_io_submit, a communicator on the handle, N < 6, a NULL
 * cam_poses, a non-finite entry, a threshold <= 0.  In the armed frame call (ORCVIO_ERR_INVALID, nothing done, the arming stands):
 * n_remove != 2, remove_clones not one of the four sets above, prune_tracks == NULL (the launch rides in front of the prune update). */
typedef struct orcvio_msckf_clone_choice_config {
    double rotation_threshold, translation_threshold;
    int32_t tracking_ok;      /* tracking_rate > tracking_rate_threshold, evaluated by the caller                                    */
    double R_imu_cam0[9];     /* the IMU state's extrinsic at the time of the call (row-major) ...                                  */
    double t_cam0_imu[3];
    const double* cam_poses;  /* [N][12] orientation_cam 9 (row-major) | position_cam 3, as the containers hold them before the
                                 frame's first update; COPIED by this call                                                          */
} orcvio_msckf_clone_choice_config;
typedef struct orcvio_msckf_clone_choice {   /* pinned block of the handle, filled when the frame's wait returns                       */
    int32_t evaluated;        /* 1: this frame's launch has stored the block                                                          */
    int32_t agree;            /* chosen == the frame's remove_clones                                                                  */
    int32_t chosen[2];        /* ascending window indices                                                                             */
    int32_t compared[2];      /* the clone compared with the key in iteration 1, 2                                                    */
    int32_t taken[2];         /* ... and whether it was taken                                                                         */
    double angle[2], distance[2];
} orcvio_msckf_clone_choice;
int32_t orcvio_msckf_io_choose_clones(orcvio_msckf_handle* h, const orcvio_msckf_clone_choice_config* cfg,
                                      const orcvio_msckf_clone_choice** out);

/* ---- Device-resident covariance ------------------------------------------
 * The three places besides the update where the reference touches state_cov, on a copy of P that stays in HBM, so that
 * P does not cross PCIe every frame.  n = leg_dim + 6 * (clones in the window); no EKF-SLAM / nuisance states.
 *   cov_set / cov_get     host <-> resident P (n x n, row-major)
 *   cov_propagate         OrcVIO::processModel, src/orcvio.cpp:800-816: P_LL <- Phi P_LL Phi^T + Q (leg x leg blocks,
 *                         row-major), cross terms, symmetrised
 *   cov_augment           OrcVIO::stateAugmentation, :962-1010: n -> n + 6, the new clone copies the IMU (theta, p) covariance
 *   cov_remove_clones     OrcVIO::pruneImuStateBuffer, :2935-2951 (non-Schmidt branch): rows/cols of the listed window
 *                         indices (ascending rank in the window) are deleted
 *   cov_commit            resident P <- P+ of the update that has just run (features: always defined; objects: P if rejected)
 *   cov_prefactor         factor the resident P now, asynchronously (ORCVIO_OPT_RESIDENT_FACTOR): after cov_propagate no
 *                         square-root factor of P is known and the next update would start with the Cholesky of its prior;
 *                         called when the image arrives (behind propagate + augment), it moves that off the update's critical
 *                         path -- the update then finds the factor resident, as the later updates of a frame do.  No-op when
 *                         the factor is known or the window is too large for the register-resident factorisation (n > 224).
 * orcvio_msckf_upload / orcvio_msckf_update_features / orcvio_msckf_objects_local accept P == NULL: the resident P is
 * used (its dimension must match the window). */
int32_t orcvio_msckf_cov_set(orcvio_msckf_handle* h, int32_t n, const double* P);
int32_t orcvio_msckf_cov_get(orcvio_msckf_handle* h, int32_t* n_out, double* P_out /* may be NULL */);
int32_t orcvio_msckf_cov_propagate(orcvio_msckf_handle* h, int32_t leg_dim, const double* Phi, const double* Q);
int32_t orcvio_msckf_cov_augment(orcvio_msckf_handle* h);
int32_t orcvio_msckf_cov_remove_clones(orcvio_msckf_handle* h, int32_t leg_dim, const int32_t* clone_indices, int32_t count);
int32_t orcvio_msckf_cov_commit(orcvio_msckf_handle* h);
int32_t orcvio_msckf_cov_prefactor(orcvio_msckf_handle* h);
/* Marginals of the resident covariance without fetching all of P: the per-image readers of state_cov (getPpose / getPvel behind the
 * odometry message, src/orcvio.cpp:2999-3026) want a few dozen numbers, cov_get moves n^2 doubles behind a drained stream.
 *   out = P[idx, idx]                 (m == 0)   [n_idx][n_idx], bit copies
 *   out = T P[idx, idx] T^T           (m >= 1)   [m][m]
 * with P indexed as cov_get returns it (row-major, P_m[i][j] = P[idx[i]][idx[j]]).  Nothing is symmetrised and no entry of P is
 * examined: a NaN at a gathered entry passes through, one elsewhere has no effect.  ONE launch of one workgroup (k_cov_marginal, FP64)
 * on the handle's stream, where cov_get's copy would go: it sees whatever the last cov_* call, commit or frame call left -- a frame
 * call's marginalisation that is enqueued and not waited for included -- and changes nothing resident (P, the factor, their
 * bookkeeping, the armings and the open arena stay as they are).  Every sum runs over l = 0 .. n_idx-1 in ascending order as one FMA
 * chain: the same input twice gives the same bits, and |out - exact| <= (2 n_idx + 4) 2^-53 (|T| |P_m| |T|^T) componentwise.
 *   cov_marginal_submit    validates, stages T (no synchronisation) and enqueues the launch, which stores its result into a pinned
 *                          block of the handle and a sequence word behind it.  At most ONE submit is outstanding per handle; other
 *                          calls on the handle are legal before the collect (the kernel reads P at its own place in stream order).
 *   cov_marginal_collect   waits for that word as the io_* calls wait for theirs -- a bounded spin (ORCVIO_IO_SPIN_SECONDS), then a
 *                          stream synchronisation, then ORCVIO_ERR_TIMEOUT -- and copies the block to out; *rows = m, or n_idx for a
 *                          gather.  No copy by the runtime, no pageable memory on the device's side.
 *   cov_get_marginal       submit followed by collect.
 * Refused with ORCVIO_ERR_INVALID before anything is enqueued (nothing changed, a later good call succeeds): a NULL argument, no
 * resident covariance, n_idx outside 1..64, an index outside [0, n), m outside 0..64, T NULL with m > 0 or given with m == 0, a
 * non-finite entry of T, a second submit before the collect, a collect without a submit, a communicator on the handle. */
#define ORCVIO_MARGINAL_MAX 64
typedef struct orcvio_msckf_marginal {
    int32_t n_idx;        /* 1..64 */
    const int32_t* idx;   /* [n_idx] state indices of the resident covariance; any order, repeats allowed */
    int32_t m;            /* 0: out = P[idx, idx], [n_idx][n_idx];  1..64: out = T P[idx, idx] T^T, [m][m] */
    const double* T;      /* [m][n_idx] row-major; NULL exactly when m == 0 */
} orcvio_msckf_marginal;
int32_t orcvio_msckf_cov_get_marginal(orcvio_msckf_handle* h, const orcvio_msckf_marginal* marginal, double* out);
int32_t orcvio_msckf_cov_marginal_submit(orcvio_msckf_handle* h, const orcvio_msckf_marginal* marginal);
int32_t orcvio_msckf_cov_marginal_collect(orcvio_msckf_handle* h, double* out, int32_t* rows /* may be NULL */);
/* The tail of measurementUpdate_hybrid on the device (src/orcvio.cpp:1818-1821, :1904-1947; with ORCVIO_OPT_SCHMIDT_STATES :1920-1935):
 * after an update that carried entering features (orcvio_msckf_upload_new_features) the resident covariance becomes the augmented
 * one -- P+ with the d k new feature states behind it (in front of the nuisance block) -- computed from H_1, H_2, r_1 still on the
 * device; dx_new [d k] is returned.  Instead of orcvio_msckf_cov_commit for such an update.  The caller raises
 * ORCVIO_OPT_EXTRA_STATES by d k before its next upload.  This call DROPS the resident square-root factor (the frame's next update
 * factors the augmented prior again); see orcvio_msckf_cov_commit_new_features_fac. */
int32_t orcvio_msckf_cov_commit_new_features(orcvio_msckf_handle* h, double* dx_new);
/* The same tail with the resident square-root factor carried along.  With P+ = S+ S+^T, HH = H_2^-1 H_1 and sigma = noise_feature,
 *     P_aug = S_aug S_aug^T,   S_aug = [  S+       0              ]   (d k more columns, block-diagonal sigma H_2^-1 in the new rows)
 *                                      [ -HH S+    sigma H_2^-1    ]
 * so the frame's second update (pruneImuStateBuffer's) starts from the factor instead of a Cholesky chain of the augmented prior.
 * Preconditions, refusals and dx_new are those of orcvio_msckf_cov_commit_new_features: no finished update with entering features
 * ORCVIO_ERR_INVALID, n + d k beyond the handle's capacity ORCVIO_ERR_CAPACITY, a zero on diag(H_2) ORCVIO_ERR_NOT_SPD; a refusal
 * leaves the resident covariance, its factor and the bookkeeping untouched.  The old block and the moved nuisance block of P are
 * 0.5 (P+ + P+^T) bit for bit, P21 = -HH P+ and P22 = HH P+ HH^T + sigma^2 W symmetrised as the call above forms them (the order of
 * summation differs: the new blocks agree to rounding, not bit for bit), P_aug is symmetric exactly.
 * The factor follows exactly when orcvio_msckf_cov_commit would have kept S+ for this update -- ORCVIO_OPT_RESIDENT_FACTOR on, no
 * ORCVIO_OPT_SCHMIDT_STATES, not the direct form of a thin stack -- and its columns, those of S+ plus d k, fit the handle's factor
 * buffers (round_up(n_max + 1, 16) columns).  In every other case it is dropped as above; that is not an error.  Device work: two
 * launches (k_aug_rows, k_aug_finish), one fetch, one wait.  The caller raises ORCVIO_OPT_EXTRA_STATES by d k, as above.
 * Measured on MI355X (leg 22, 20 clones, 12 in-state features, 1 and 3 entering features, profiles/r32a_entering_commit_ab.json): the
 * call 32-40 us against 62-79 us for the call above, the call plus the frame's next update 137-146 us against 175-183 us; the next
 * update itself gains 0-7 us of that (the Cholesky chain of its prior was mostly hidden beside the tracks already). */
int32_t orcvio_msckf_cov_commit_new_features_fac(orcvio_msckf_handle* h, double* dx_new);
/* Schmidt branch of pruneImuStateBuffer (src/orcvio.cpp:2881-2920): the listed clones (window ranks before the call, ascending)
 * leave the window but stay in the resident covariance as nuisance states -- their blocks move to the end, in the listed order. */
int32_t orcvio_msckf_cov_clones_to_nuisance(orcvio_msckf_handle* h, int32_t leg_dim, const int32_t* clone_indices, int32_t count);
/* In-state SLAM features of the hybrid filter on the resident covariance.  State layout [LEG | 6 n_clones | idp_dim per feature
 * state, in feature_states order | 6 per nuisance state].  Both calls keep the resident square-root factor, so the next update
 * starts from it instead of a Cholesky factorisation of P.
 *   cov_remove_features   removeLostFeatures -> rmLostFeaturesCov, src/orcvio.cpp:2233, :3776-3828: the idp_dim rows and columns of
 *                         each listed feature are deleted; slots are positions in feature_states BEFORE the call, strictly
 *                         ascending; what stands behind the n_feature_states features must be whole 6-wide nuisance blocks (they
 *                         stay).  Refused (ORCVIO_ERR_INVALID, nothing changed): leg + 6 n_clones + idp_dim n_feature_states > the
 *                         resident dimension, a rest that is not a multiple of 6, slots out of range or not ascending.  The caller
 *                         lowers ORCVIO_OPT_EXTRA_STATES by idp_dim count before its next upload.
 *   cov_change_anchors    pruneImuStateBuffer, in-state features whose anchor clone leaves (:2664-2720): the new parameters in the
 *                         new anchor's camera frame (3-d :2680-2687 invParam; 1-d :2700-2712 invDepth and obs_anchor) and the
 *                         covariance update updateFeatureCov_3didp (:3457-3609) / _1didp (:3611-3774), for up to 16 features
 *                         in ONE launch: P <- T P T^T with T = I except the changed features' rows (their J: the feature, the old
 *                         and new anchor clones, the extrinsics -- no J reads another changed feature's row, so this equals the
 *                         reference's one-feature-after-the-other loop up to rounding).  poses: [n_clones][ORCVIO_POSE_STRIDE]
 *                         records as in the io arena (a clone's camera pose comes from its own record); R_b2c [9] / t_c_b [3]:
 *                         the CURRENT extrinsics (state_server.imu_state), read for p_old under if_FEJ and for the extrinsic
 *                         columns.  flags: leg_dim and if_fej are read.  literal_3d (idp_dim 3): 1 = the reference as written,
 *                         whose "new" pose and column are looked up under old_state_id (:3487, :3544: the new clone gets no
 *                         entries, H_x_new lands in the old clone's block); 0 = the consistent Jacobian with the new anchor's
 *                         pose and columns.  The new anchor is the caller's choice (3-d: the newest clone; 1-d: getNewAnchorId,
 *                         :3892-3950).  Out: new_param [count][3] (3-d: invParam; 1-d: obs_anchor (u, v, 1)), new_inv_depth
 *                         [count] (may be NULL), to be written back to map_server with id_anchor = new_anchor.  The feature
 *                         states are taken to be everything behind the clones except the last 6 k states when
 *                         ORCVIO_OPT_SCHMIDT_STATES = k is set (the nuisance block): with nuisance states in the resident covariance,
 *                         set that option first, or a slot that reaches into the nuisance block cannot be told from a feature's.
 *                         Refused (ORCVIO_ERR_INVALID, P and its factor unchanged): a slot beyond the feature states or listed
 *                         twice, a feature region that is not a multiple of idp_dim, old == new, an anchor >= n_clones, a
 *                         non-finite pose / extrinsic / position, more than 16 changes. */
typedef struct orcvio_msckf_anchor_change {
    int32_t slot;          /* position of the feature in feature_states                                  */
    int32_t old_anchor;    /* window rank of Feature::id_anchor (the clone about to leave)                */
    int32_t new_anchor;    /* window rank of the new anchor                                              */
    double p_w[3];         /* Feature::position                                                          */
    double p_fej[3];       /* Feature::position_FEJ, read under if_fej                                   */
} orcvio_msckf_anchor_change;
int32_t orcvio_msckf_cov_remove_features(orcvio_msckf_handle* h, int32_t leg_dim, int32_t n_clones, int32_t idp_dim, int32_t n_feature_states,
                                         const int32_t* slots, int32_t count);
int32_t orcvio_msckf_cov_change_anchors(orcvio_msckf_handle* h, const orcvio_msckf_flags* flags, int32_t idp_dim, int32_t literal_3d,
                                        int32_t n_clones, const double* poses, const double* R_b2c, const double* t_c_b,
                                        const orcvio_msckf_anchor_change* changes, int32_t count, double* new_param, double* new_inv_depth);

/* ---- Zero-velocity frames on the resident covariance (measurementUpdate_ZUPT_vpq, src/orcvio.cpp:3326-3454) --------------------------
 * On a frame the zero-velocity check accepts (checkZUPTFeat, :3081-3126: pixel distances, the caller's; checkZUPTIMU, :3129-3323: IMU
 * samples against the covariance, the caller's or orcvio_msckf_cov_zupt_check_imu / _cov_zupt_frame_checked below), the
 * reference runs a 9-row update on the current velocity and on the pose difference of the two newest clones instead of the MSCKF
 * updates, and marginalises the previous clone (:2641-2645).  The Jacobian's sparsity is fixed (:3329-3334), so nothing of size 9 x n
 * is passed: the call takes the residual and the three variances.
 *   cov_zupt         the update on the resident covariance: with Y = H P (three combinations of 15 rows of P), M = Y H^T + R = C C^T and
 *                    V = C^-1 Y:  dx = V^T C^-1 r,  P+ = (P + P^T)/2 - V^T V  -- the reference's (I - K H) P followed by (P + P^T)/2 for a
 *                    symmetric prior.  With ORCVIO_OPT_SCHMIDT_STATES = k the trailing 6 k x 6 k block of P+ is the prior's
 *                    (:3432-3441); dx covers every state, as the reference's K r does.  The resident dimension must be
 *                    leg_dim + 6 n_clones + ORCVIO_OPT_EXTRA_STATES (which counts the nuisance states).  dx [n] is the caller's, for
 *                    orcvio_msckf_increment_state and the in-state features' parameters (:3391-3428); the covariance is updated whether
 *                    or not the caller's increment later discards a large dx (:3389, then :3431-3447).
 *                    The resident square-root factor: valid on entry and no nuisance states -> S+ of the same shape with
 *                    S+ S+^T = P+ (array form: nine Householder reflectors bring [R^1/2 | H S] to lower-triangular form from the right
 *                    and are applied to every row of S); with nuisance states, or without a valid factor, it is invalid afterwards.
 *                    The factor is also invalid afterwards when it has more than 448 columns (what the reflectors hold in LDS; a
 *                    factor of cov_prefactor, cov_augment or a committed update has at most n <= 232 plus a few).
 *                    Refused on the device (ORCVIO_ERR_NOT_SPD, *applied = 0, dx = 0, P and its factor exactly as before): M not
 *                    positive definite, or a non-finite entry in one of the 15 rows of P that enter H P (rows 3..5 and the twelve
 *                    rows of the two newest clones).  The gate reads those rows whole; the other entries of P are NOT examined: a
 *                    NaN or Inf elsewhere in P passes through (symmetrised) into P+, as it passes through every other cov_* call.
 *                    A HIP error while waiting (ORCVIO_ERR_HIP / _TIMEOUT): the prior and its factor stay resident, nothing applied.
 *                    Refused before anything is enqueued (ORCVIO_ERR_INVALID, nothing done): a null argument, leg_dim not 22 / 46,
 *                    n_clones < 2, a dimension that does not match, a variance that is not finite or <= 0, a non-finite r, a
 *                    communicator on the handle.
 *   cov_zupt_frame   ONE stationary frame: the launches of cov_propagate (Phi, Q not NULL), cov_augment (augment != 0), cov_zupt and
 *                    cov_remove_clones of the clone at window rank n_clones - 2 (remove_previous != 0), back to back on the handle's
 *                    stream; the calling thread waits once.  Results bit-identical to the four separate calls.  zupt.n_clones is the
 *                    window AFTER this frame's augmentation.  A validation failure leaves nothing done; a refusal on the device leaves
 *                    propagation, augmentation and marginalisation standing (*applied = 0, ORCVIO_ERR_NOT_SPD).  *n_after: the resident
 *                    dimension behind the frame.  The factor behind a refused frame: kept where cov_zupt would have kept it
 *                    (valid on entry to the update, no nuisance states, at most 448 columns); in the other cases -- nuisance states
 *                    declared, or more than 448 columns -- it is DROPPED although P is the prior's: conservative, the next update
 *                    factors P again.  A HIP error behind the update's launches (ORCVIO_ERR_HIP / _TIMEOUT from the row deletion or
 *                    the wait) leaves NOTHING resident: the outcome is unknown and the row deletion may have reused the prior's buffer,
 *                    so every cov_* call refuses until orcvio_msckf_cov_set.
 * Frames on which an in-state feature is lost or changes its anchor use the separate calls in the reference's order: cov_propagate,
 * cov_augment, cov_zupt, cov_remove_features, cov_change_anchors, cov_remove_clones -- all of which keep the factor. */
typedef struct orcvio_msckf_zupt {
    int32_t leg_dim;        /* 22 or 46 */
    int32_t n_clones;       /* N >= 2: the window with this frame's clone in it */
    double  r[9];           /* r_v, r_p, r_q as :3337-3368 forms them */
    double  noise_v, noise_p, noise_q;   /* VARIANCES (the yaml's std squared, :119-121) */
} orcvio_msckf_zupt;
int32_t orcvio_msckf_cov_zupt(orcvio_msckf_handle* h, const orcvio_msckf_zupt* zupt, double* dx /* [n] */, int32_t* applied);

typedef struct orcvio_msckf_zupt_frame {
    orcvio_msckf_zupt zupt;   /* n_clones AFTER this frame's augmentation */
    const double* Phi; const double* Q;   /* NULL, NULL: no propagation */
    int32_t augment;
    int32_t remove_previous;  /* != 0: the clone at window rank N-2 is marginalised behind the update (:2641-2645) */
} orcvio_msckf_zupt_frame;
int32_t orcvio_msckf_cov_zupt_frame(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame* frame, double* dx, int32_t* applied, int32_t* n_after);

/* ---- One filter frame in one call WITH the life cycle of the in-state features (hybrid filter) ------------------------------------
 * orcvio_msckf_io_step_frame plus the frame's feature events, in the reference's order (processFeatures, src/orcvio.cpp:567-594):
 *   1 propagation   2 augmentation   3 REMOVAL of the lost in-state features (removeLostFeatures -> rmLostFeaturesCov, :2233,
 *   :3776-3828)   4 the first update, on the tracks and the in-state features that stay   5 the in-state features' INCREMENT
 *   (measurementUpdate_hybrid :1842-1889) and the window's pose step   6 the ANCHOR CHANGES of the features whose anchor clone
 *   leaves (pruneImuStateBuffer :2664-2720, updateFeatureCov_*)   7 the prune update   8 marginalisation
 * -- still one call and one wait: the removal is an index map inside the frame's first launch, the feature step rides in the launch
 * in front of the second update, the anchor change is enqueued between the two updates and stores its results into the pinned
 * output block ahead of the flag the call waits on.
 * Call order as orcvio_msckf_io_step_frame; io_begin takes the window and ORCVIO_OPT_EXTRA_STATES as they are AFTER the removals:
 * the resident dimension + 6 augment - idp_dim n_lost must equal io_begin's n, and ORCVIO_OPT_EXTRA_STATES idp_dim x the features that stay.
 *   lost_slots       positions in feature_states before the call, strictly ascending; n_lost <= n_feature_states
 *   changes          as orcvio_msckf_cov_change_anchors', at most 16; slots are positions AFTER the removals; the new anchor is the
 *                    caller's choice (planAnchorChanges / getNewAnchorId, orcvio_msckf_host.hpp) and may not be in remove_clones
 *   R_b2c, t_c_b     the IMU's CURRENT extrinsics (state_server.imu_state) before this frame's first update
 *   prune_apply_dx != 0 (and the frame has a first update): the changed features' world positions are what the reference's state
 *                    holds when pruneImuStateBuffer runs, derived ON THE DEVICE: the feature's parameters from its slam_features
 *                    record (every change's slot must have one, anchored at old_anchor) take dx at the feature's own columns, p_w
 *                    follows from the OLD anchor's camera pose as the pose step leaves it; changes[].p_w is ignored, p_fej used as
 *                    given; the extrinsics take dx[15:21] (incrementState_IMUCam :4512-4517).  Under discard_large_update a
 *                    discarded dx leaves poses and extrinsics alone but the parameters are STILL incremented (the reference's feature
 *                    loop runs after incrementState_IMUCam's early return); a refused first update increments nothing (the record's
 *                    p_w, the given extrinsics).
 *   prune_apply_dx == 0 (or no first update: dx is zero): changes[].p_w and the given extrinsics as they are -- bit for bit the
 *                    separate calls cov_propagate, cov_augment, cov_remove_features, update, cov_change_anchors, update, cov_remove_clones.
 * Results: new_param [n_changes][3], new_inv_depth [n_changes] (as orcvio_msckf_cov_change_anchors') in the pinned output block.
 * Status: every validation failure (those of orcvio_msckf_cov_remove_features / _cov_change_anchors too) returns its code with NOTHING
 * done.  Removals and anchor changes are bookkeeping: like propagation and marginalisation they stand when an update is refused on
 * the device.  A changed feature whose derived position is not finite (an incremented inverse depth of zero) leaves P and its factor
 * without ANY of the frame's anchor changes and refuses the prune update: status_changes = status_prune = ORCVIO_ERR_NOT_SPD.  A lost
 * in-launch hand-off is repaired inside the call; the anchor changes are applied once.
 * Not in this call: features ENTERING the state, Schmidt nuisance states (ORCVIO_OPT_SCHMIDT_STATES) together with events, a
 * communicator on the handle, more than 512 in-state features (ORCVIO_ERR_CAPACITY). */
typedef struct orcvio_msckf_frame_events {
    int32_t idp_dim;               /* 1 or 3                                                                    */
    int32_t literal_3d;            /* as orcvio_msckf_cov_change_anchors                                        */
    int32_t n_feature_states;      /* in-state features BEFORE this frame's removals                            */
    const int32_t* lost_slots;     /* [n_lost]                                                                  */
    int32_t n_lost;
    const orcvio_msckf_anchor_change* changes;   /* [n_changes]                                                 */
    int32_t n_changes;
    const double* R_b2c;           /* [9]                                                                       */
    const double* t_c_b;           /* [3]                                                                       */
} orcvio_msckf_frame_events;
typedef struct orcvio_msckf_frame_result_ex {
    orcvio_msckf_frame_result frame;   /* as orcvio_msckf_io_step_frame's                                       */
    const double* new_param;       /* [n_changes][3]  NULL without changes                                      */
    const double* new_inv_depth;   /* [n_changes]                                                               */
    int32_t status_changes;        /* ORCVIO_OK, or ORCVIO_ERR_NOT_SPD: a changed feature's position not finite */
} orcvio_msckf_frame_result_ex;
int32_t orcvio_msckf_io_step_frame_ex(orcvio_msckf_handle* h, const orcvio_msckf_frame_step* step, const orcvio_msckf_frame_events* events,
                                      orcvio_msckf_frame_result_ex* result);

/* ---- IMU propagation from raw samples (batchImuProcessing -> processModel, src/orcvio.cpp:664-928, :3952-4367) -----------------------
 * What the reference runs in front of every image: per IMU sample a state predictor, one of three forms of Phi, Q = Phi G Q_c G^T Phi^T dt
 * and three products against P.  The call takes the raw samples.  Its HOST half (csrc/host/imu_model.hpp) selects the samples as
 * :678-709 do (t <= state.time skipped; stop at the first t - time_bound > imu_img_time_th) and runs one predictor per selected sample
 * (predictNewStateLARVIO or predictNewStateOrcVIO): *state and prev_meas are updated when the call returns, without a wait.  Its DEVICE
 * half is one launch (k_imu_phi_q, one workgroup): the S pairs (Phi_k, Q_k) from the states the host half left, accumulated in order to
 * Phi = Phi_S ... Phi_1 and Q (Q <- Phi_k Q Phi_k^T + Q_k), written where the propagation launches of orcvio_msckf_cov_propagate read
 * them, which follow on the handle's stream: the resident factor is dropped as cov_propagate drops it.  The accumulated pair applied once
 * equals the reference's per-sample application to rounding ("IMU propagation from raw samples").
 *   cfg       leg_dim 22 only (calib_imu_instrinsic = 0: Tg = Ma = I, As = 0); use_larvio / use_left_perturbation / use_closed_form /
 *             if_fej choose the predictor and the form of Phi as :750-773, :3960, :3997 do; Q_c_diag: the diagonal of
 *             continuous_noise_cov (:429-438: gyro, acc, gyro bias, acc bias VARIANCES, three each)
 *   state     in: imu_state (and the velocity / position of imu_state_FEJ_now, read under if_fej); out: the propagated state
 *   prev_meas [6] m_gyro_old | m_acc_old (:703-704), in and out: carried from frame to frame by the caller
 *   samples   [n_samples][7]: t | angular_velocity | linear_acceleration
 *   info      wait (in): != 0 makes the call wait for the device once and report a refusal.  Out: n_used (skipped + processed: what the
 *             reference erases from its buffer), n_propagated (S), dt = t_last - time_bound (imu_state.dt), mean_sforce (meanSForce;
 *             zero when S = 0, where the reference divides by zero), applied (1; 0 after a refusal the call has seen, or S = 0)
 *   Phi_out, Q_out   [22][22] or NULL; not NULL makes the call wait, as info->wait does
 * S = 0 after selection: no launch, the covariance and its factor untouched, Phi_out = I, Q_out = 0.
 * Refused on the device: a non-finite entry in Phi or Q -- the reference's right closed form (:4343, :4348) divides by |gyro|^2, so an
 * exactly zero unbiased gyro sample gives NaN.  The kernel leaves a status word that the propagation launches behind it read: they
 * copy P bit for bit.  A call that waits returns ORCVIO_ERR_NOT_SPD with applied = 0 (*state is propagated all the same: the mean does
 * not depend on Phi); a call that does not wait cannot report it.  Either way the resident factor is dropped.
 * Refused before anything is done (*state and prev_meas untouched): a null argument, leg_dim != 22, no resident covariance
 * (ORCVIO_ERR_INVALID); more than 128 selected samples (ORCVIO_ERR_CAPACITY; info->n_used / n_propagated are filled). */
typedef struct orcvio_msckf_imu_config {
    int32_t leg_dim;                /* 22; 46 for orcvio_msckf_cov_propagate_imu_calib */
    int32_t use_larvio, use_left_perturbation, use_closed_form, if_fej;
    double  gravity[3];             /* IMUState::gravity */
    double  imu_img_time_th;        /* 1 / (2 imu_rate), :76 */
    double  Q_c_diag[12];
} orcvio_msckf_imu_config;
typedef struct orcvio_msckf_imu_state {
    double time;
    double R_b2w[9], v[3], p[3];    /* imu_state.orientation (row-major), velocity, position */
    double gyro_bias[3], acc_bias[3];
    double v_fej[3], p_fej[3];      /* imu_state_FEJ_now.velocity / position */
} orcvio_msckf_imu_state;
typedef struct orcvio_msckf_imu_info {
    int32_t wait;
    int32_t n_used, n_propagated, applied;
    double  dt, mean_sforce[3];
} orcvio_msckf_imu_info;
int32_t orcvio_msckf_cov_propagate_imu(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg, orcvio_msckf_imu_state* state,
                                       double* prev_meas, const double* samples, int32_t n_samples, double time_bound,
                                       orcvio_msckf_imu_info* info, double* Phi_out, double* Q_out);
/* The ARMED form (same inputs): the host half runs now -- *state, prev_meas and info are valid on return, info->applied = 0 -- and the
 * next orcvio_msckf_io_step_frame / _io_step_frame_ex / _cov_zupt_frame / _cov_zupt_frame_checked on the handle is armed, in the manner of
 * orcvio_msckf_io_triangulate: given Phi = Q = NULL, it enqueues k_imu_phi_q in front of its head launch (the propagation launches, for
 * cov_zupt_frame) and hands them the device's Phi / Q instead of a staged copy -- the frame's one wait stays one wait, and the results
 * are bit for bit those of the frame given Phi_out / Q_out of orcvio_msckf_cov_propagate_imu.  S = 0 after selection arms nothing.
 * An armed handle given Phi != NULL: ORCVIO_ERR_INVALID, nothing done, the arming stands; so does it behind every other validation
 * failure of the frame call.  orcvio_msckf_cov_propagate_imu and a second arming on an armed handle: ORCVIO_ERR_INVALID.
 * A refused Phi / Q (non-finite) refuses the frame's propagation and BOTH updates (cov_zupt_frame: the zero-velocity update);
 * augmentation, removals, anchor changes and marginalisation stand.  The frame call returns ORCVIO_ERR_NOT_SPD with status_first =
 * status_prune = ORCVIO_ERR_NOT_SPD and stats[3] = 0 (cov_zupt_frame: *applied = 0).
 * Not with a communicator on the handle (as io_step_frame), not together with orcvio_msckf_io_triangulate on the same frame, leg_dim 22. */
int32_t orcvio_msckf_io_propagate_imu(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg, orcvio_msckf_imu_state* state,
                                      double* prev_meas, const double* samples, int32_t n_samples, double time_bound,
                                      orcvio_msckf_imu_info* info);

/* ---- IMU propagation with intrinsic calibration: leg_dim 46 (calib_imu_instrinsic = 1) ------------------------------------------------
 * orcvio_msckf_cov_propagate_imu with the 24 IMU intrinsics in the state (error-state columns 22 .. 45, T1 T2 T3 A1 A2 A3 M1 M2, three
 * each: the order of orcvio_msckf_state.imu_intrinsics).  Semantics, info, S = 0, S > 128, the refusal of a non-finite Phi and "waits
 * only if asked" are that call's, word for word; what differs:
 *   measurement  updateImuMx (:4373-4418) makes Tg, As, Ma from intr; f = m_acc - b_a, acc = Ma f, w = m_gyro - As acc - b_g,
 *                gyro = Tg w (:733-746), and the same from prev_meas -- BOTH halves of prev_meas are read.  The predictors get gyro, acc.
 *   Phi          the left / LARVIO closed form carries Tg, Tg As, Ma in its bias blocks, a (theta, b_a) block, and 24 blocks
 *                Phi[0:9, 22:46] (:4016-4305).  The Euler forms and the right closed form write no intrinsic block, as the reference
 *                writes them (:3952-3978, :4308-4367): their Phi is the 15 x 15 of leg_dim 22 inside an identity.
 *   device       one launch, k_imu_phi_q46: rows 15 .. 45 of every Phi_k are identity rows and Q lives in the leading 15 x 15, so only
 *                Phi[0:15, 22:46] is accumulated beside the 22 recursion ("IMU propagation at leg_dim 46").
 *   Phi_out, Q_out   [46][46] or NULL.  S = 0: Phi_out = I, Q_out = 0.
 * A frame at 46 is this call without a wait followed by orcvio_msckf_io_step_frame with Phi = NULL, or Phi_out / Q_out handed to the frame.
 * Refused before anything is done (ORCVIO_ERR_INVALID, *state and prev_meas untouched): a null argument (intr included), leg_dim != 46
 * (orcvio_msckf_cov_propagate_imu serves 22), a non-finite intrinsic, a resident covariance of fewer than 46 states, an armed handle.
 * NOT at 46: the armed form (orcvio_msckf_io_propagate_imu; arming was measured slower than handing Phi, Q to the frame, and the frame
 * head reads a 22-wide pair on that path), the zero-velocity check (checkZUPTIMU reads Ma, As, Tg too, :3184-3188: the _checked
 * calls stay at 22), and any "corrected" mode of what the reference writes. */
typedef struct orcvio_msckf_imu_intrinsics {
    double x[24];   /* T1 T2 T3 A1 A2 A3 M1 M2, as orcvio_msckf_state.imu_intrinsics */
} orcvio_msckf_imu_intrinsics;
int32_t orcvio_msckf_cov_propagate_imu_calib(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg,
                                             const orcvio_msckf_imu_intrinsics* intr, orcvio_msckf_imu_state* state, double* prev_meas,
                                             const double* samples, int32_t n_samples, double time_bound, orcvio_msckf_imu_info* info,
                                             double* Phi_out, double* Q_out);   /* [46][46] or NULL */

/* ---- Zero-velocity DETECTION from IMU samples on the resident covariance (checkZUPTIMU, src/orcvio.cpp:3129-3323) ----------------------
 * The test the configurations with if_use_feature_zupt_flag = 0 run on every image, between stateAugmentation and removeLostFeatures:
 * over the S samples of the frame (imu_recent_zupt: the samples the IMU call's host half selected) it stacks m = S - 1 blocks of six
 * rows on the nine states (theta, b_g, b_a) -- gyro rows [0 I 0] with a ZERO residual (:3194) and noise sigma_w2 / dt_i,
 * accelerometer rows [J_i 0 R] with r_i = -R a_i - g, a_i = m_acc_i - b_a, J_i = skew(R a_i) (left perturbation) or R skew(a_i), noise
 * sigma_a2 / dt_i, dt_i = t_i+1 - t_i -- and compares chi^2 = r^T (H P_m H^T + R)^-1 r with the quantile of 6 m degrees of freedom.
 * P_m is the 9 x 9 marginal of the covariance AS PROPAGATION LEFT IT (rows and columns 0..2, 9..14) plus
 * diag(dt_sum sigma_wb I, dt_sum sigma_ab I) on its bias block (sigma_wb, sigma_ab unsquared, as :3228-3229 write it).
 * The device does not form the 6 m x 6 m matrix (762 x 762 at 128 samples): H has nine columns and R is diagonal, so
 *   A = H^T R^-1 H,  b = H^T R^-1 r,  c = r^T R^-1 r;   P_m = L L^T,  M = I + L^T A L = C C^T,  chi^2 = c - |C^-1 L^T b|^2
 * is the same number ("Zero-velocity detection": the measured distance to the dense form).  One launch
 * (k_zupt_check, one workgroup), which reads 81 entries of P -- both triangles, averaged -- and writes nothing of P or its factor.
 *   chk       the reference's constants (orcvio_msckf_zupt_check_default fills them) and use_left_perturbation
 *   verdict   evaluated (0: fewer than two samples, :3134, or refused), accept (do_zupt), dof = 6 (S - 1), chi2, chi2_check =
 *             orcvio_msckf_chi2_quantile(dof, chi2_prob) (the reference's table below 500 rows and its boost quantile above are this
 *             function), speed = |v|;  accept = evaluated && !(chi2 > chi2_multiplier chi2_check) && !(speed > max_velocity).
 *             The speed test is host arithmetic; chi2 is evaluated and reported whatever it says.
 *             status: ORCVIO_OK, or ORCVIO_ERR_NOT_SPD behind a refusal on the device (then evaluated = 0).
 *   cov_zupt_check_imu            tests the resident covariance as it stands: R_b2w [9] row-major, v, acc_bias, gravity [3], samples
 *                                 [n_samples][7] (t | gyro | acc) the SELECTED ones.  One launch, one wait; n_samples < 2: no launch,
 *                                 evaluated = 0, ORCVIO_OK.  P, its factor and the factor's validity are untouched.
 *   cov_propagate_imu_checked     orcvio_msckf_cov_propagate_imu (same arguments, same host half and launches) with k_zupt_check behind the
 *                                 propagation launches, on the propagated P, the propagated state and the samples the host half selected;
 *                                 the call always waits, once.  P is bit for bit what the unchecked call leaves, the verdict bit for bit
 *                                 that of cov_zupt_check_imu behind it.  A refused Phi / Q: evaluated = 0, ORCVIO_ERR_NOT_SPD, as the unchecked
 *                                 call; one selected sample: propagated, evaluated = 0.  A moving frame on these configurations is this
 *                                 call followed by orcvio_msckf_io_step_frame with Phi = NULL: two waits, no cov_get, no dense solve.
 *   cov_zupt_frame_checked        the stationary frame on a handle ARMED by orcvio_msckf_io_propagate_imu (frame->Phi = Q = NULL,
 *                                 zupt.leg_dim 22): the launches of cov_zupt_frame with k_zupt_check behind the augmentation; the update
 *                                 reads the check's status block, which carries the armed propagation's refusal on.  The calling thread waits
 *                                 ONCE.  Accepted: dx, P, the factor and *n_after bit for bit those of io_propagate_imu + cov_zupt_frame --
 *                                 but the previous clone (remove_previous) is marginalised BEHIND the wait and only when the update was
 *                                 applied (enqueued, no second wait), where cov_zupt_frame enqueues it in front of the wait.  Rejected by
 *                                 the check: ORCVIO_OK, *applied = 0, dx = 0, verdict.accept = 0; propagation and augmentation stand,
 *                                 nothing is marginalised, P is what cov_propagate_imu + cov_augment leave, the factor kept or dropped by
 *                                 cov_zupt_frame's rule for a refused update; the caller goes on with orcvio_msckf_io_step_frame
 *                                 (Phi = NULL, augment = 0).  A parked platform spends one wait per frame.  Refused on the device (the check
 *                                 or the update): ORCVIO_ERR_NOT_SPD, *applied = 0, nothing marginalised.  One selected sample: no check, no
 *                                 update (*applied = 0, evaluated = 0), propagation and augmentation stand.  An unarmed handle:
 *                                 ORCVIO_ERR_INVALID, nothing done.
 * Refused on the device (evaluated = 0, status ORCVIO_ERR_NOT_SPD): a non-finite entry among the marginal's 81 entries, P_m or M not
 * positive definite, the status word of an IMU propagation in front already set.  The rest of P is NOT examined.
 * Refused before anything is enqueued (ORCVIO_ERR_INVALID, nothing done, an arming stands): a null argument, leg_dim != 22, no resident
 * covariance, a communicator on the handle, non-finite samples, state or constants, a variance, sigma_wb / sigma_ab, chi2_multiplier or
 * max_velocity <= 0, chi2_prob outside (0, 1), and a sample interval dt_i <= 0.  THE LAST DIVERGES FROM THE REFERENCE, which divides by
 * dt_i: a zero gives NaN, NaN > threshold is false, and checkZUPTIMU ACCEPTS the frame.  More than 128 samples: ORCVIO_ERR_CAPACITY.
 * Not in this call: the check inside orcvio_msckf_io_step_frame / _io_step_frame_ex (it would have to choose between two frame kinds
 * and two sets of clones to marginalise in front of the frame's wait); checkZUPTFeat, a sort of pixel distances the front end owns. */
typedef struct orcvio_msckf_zupt_check {
    double sigma_w2, sigma_a2;      /* :3140-3142, variances                         */
    double sigma_wb, sigma_ab;      /* :3144-3146, used unsquared as :3228-3229 do    */
    double chi2_prob;               /* chi_square_threshold_zupt, 0.95               */
    double chi2_multiplier;         /* 1                                             */
    double max_velocity;            /* 0.25                                          */
    int32_t use_left_perturbation;
} orcvio_msckf_zupt_check;
typedef struct orcvio_msckf_zupt_verdict {
    int32_t evaluated;   /* 0: fewer than two samples (:3134), or refused             */
    int32_t accept;      /* do_zupt                                                   */
    int32_t dof;         /* 6 (S - 1)                                                 */
    int32_t status;      /* ORCVIO_OK, or ORCVIO_ERR_NOT_SPD behind a device refusal  */
    double chi2, chi2_check, speed;
} orcvio_msckf_zupt_verdict;
void orcvio_msckf_zupt_check_default(orcvio_msckf_zupt_check* chk);
int32_t orcvio_msckf_cov_zupt_check_imu(orcvio_msckf_handle* h, const orcvio_msckf_zupt_check* chk, const double* R_b2w, const double* v,
                                        const double* acc_bias, const double* gravity, const double* samples, int32_t n_samples,
                                        orcvio_msckf_zupt_verdict* verdict);
int32_t orcvio_msckf_cov_propagate_imu_checked(orcvio_msckf_handle* h, const orcvio_msckf_imu_config* cfg, orcvio_msckf_imu_state* state,
                                               double* prev_meas, const double* samples, int32_t n_samples, double time_bound,
                                               orcvio_msckf_imu_info* info, double* Phi_out, double* Q_out,
                                               const orcvio_msckf_zupt_check* chk, orcvio_msckf_zupt_verdict* verdict);
int32_t orcvio_msckf_cov_zupt_frame_checked(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame* frame, const orcvio_msckf_zupt_check* chk,
                                            double* dx, int32_t* applied, int32_t* n_after, orcvio_msckf_zupt_verdict* verdict);

/* ---- Zero-velocity frames of a HYBRID filter: the in-state features leave in front of the update ----------------------------------------
 * When either zero-velocity check accepts a frame, the reference deletes ALL in-state (EKF-SLAM) features before
 * measurementUpdate_ZUPT_vpq runs (checkZUPTFeat, src/orcvio.cpp:3102-3119; checkZUPTIMU, :3302-3319: a conservativeResize that cuts the
 * trailing feature_idp_dim x feature_states.size() rows and columns, feature_states.clear()); the update then runs on b = leg + 6 N
 * states and pruneImuStateBuffer marginalises the previous clone (:2641-2645).  cov_zupt / cov_zupt_frame / _checked above keep the
 * extra states through the update: another filter.  The calls below are the reference's frame, and the drop, the update and the
 * marginalisation are ONE launch (k_zupt_cov_keep; k_zupt_fac_keep for the factor): the update writes only what stays, the P buffers
 * change roles once.
 *   cov_zupt_frame_hybrid          frame as cov_zupt_frame reads it, idp_dim (1 or 3) and n_feature_states F >= 0, ALL of which leave when
 *                                  the update is applied.  The launches of cov_propagate (Phi, Q given, or armed by
 *                                  orcvio_msckf_io_propagate_imu exactly as cov_zupt_frame), cov_augment, the fused update; one wait.
 *                                  Applied: P, dx [leg + 6 n_clones] (as the reference's K r has after the resize), the factor's validity,
 *                                  shape and contents and *n_after = b - 6 (remove_previous != 0) are bit for bit those of cov_propagate,
 *                                  cov_augment, cov_remove_features (all F slots), cov_zupt, cov_remove_clones.  The gate reads the 15 rows
 *                                  at the columns < b only, as those calls do: a NaN behind b leaves with the features.
 *                                  Refused on the device (ORCVIO_ERR_NOT_SPD, *applied = 0, dx = 0): propagation and augmentation stand, NO
 *                                  feature leaves and NOTHING is marginalised, *n_after is the dimension behind the augmentation -- this
 *                                  DIFFERS from cov_zupt_frame, whose marginalisation stands behind a refusal.  P and the factor are the
 *                                  prior's own, bit for bit.  A HIP error at the wait (ORCVIO_ERR_HIP / _TIMEOUT): the launches wrote the
 *                                  spare buffers only, the propagated and augmented prior and its factor stand, as in cov_zupt -- not
 *                                  cov_zupt_frame's "nothing resident".  F = 0 is allowed: applied results are cov_zupt_frame's, bit for bit.
 *   cov_zupt_frame_checked_hybrid  everything cov_zupt_frame_checked documents (an armed handle only, leg_dim 22, Phi = Q = NULL, the
 *                                  one-sample case, the verdict), the fused update reading the check's status block.  Accepted and
 *                                  applied: as above, and nothing is enqueued behind the wait.  Rejected by the check: ORCVIO_OK,
 *                                  *applied = 0, P bit for bit what io_propagate_imu + cov_augment leave, every feature in place; the
 *                                  caller goes on with orcvio_msckf_io_step_frame_ex.
 *   zupt_check_feat                checkZUPTFeat's decision (:3081-3100) on the n pixel distances the front end computed; host
 *                                  arithmetic, no handle.  n < 20: *accept = 0, *kth = NaN.  Otherwise *kth is the ninth largest distance
 *                                  and *accept = *kth < max_dis.  A null pointer, n < 0, a non-finite distance or threshold:
 *                                  ORCVIO_ERR_INVALID.
 * Refused before anything is enqueued (ORCVIO_ERR_INVALID, nothing done, an arming stands): everything cov_zupt_frame (_checked)
 * refuses; idp_dim not 1 or 3; F < 0; a resident dimension behind the augmentation that is not leg + 6 N + idp_dim F, or
 * idp_dim F != ORCVIO_OPT_EXTRA_STATES; nuisance states declared (ORCVIO_OPT_SCHMIDT_STATES > 0): the reference's resize cuts the
 * TRAILING rows, which are then nuisance rows and not feature rows -- not reproduced here, and use_schmidt is 0 in every shipped
 * configuration.  The calls do not change ORCVIO_OPT_EXTRA_STATES: the caller sets it to 0 when *applied = 1, by the convention of
 * cov_remove_features. */
typedef struct orcvio_msckf_zupt_frame_hybrid {
    orcvio_msckf_zupt_frame frame;      /* as orcvio_msckf_cov_zupt_frame reads it */
    int32_t idp_dim;                    /* 1 or 3 */
    int32_t n_feature_states;           /* F >= 0: ALL of them leave when the update is applied */
} orcvio_msckf_zupt_frame_hybrid;
int32_t orcvio_msckf_cov_zupt_frame_hybrid(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame_hybrid* frame, double* dx /* [leg + 6 n_clones] */,
                                           int32_t* applied, int32_t* n_after);
int32_t orcvio_msckf_cov_zupt_frame_checked_hybrid(orcvio_msckf_handle* h, const orcvio_msckf_zupt_frame_hybrid* frame, const orcvio_msckf_zupt_check* chk,
                                                   double* dx, int32_t* applied, int32_t* n_after, orcvio_msckf_zupt_verdict* verdict);
int32_t orcvio_msckf_zupt_check_feat(const double* dis, int32_t n, double max_dis, int32_t* accept, double* kth);

/* ---- Environment switches (read once per process; diagnostics and A/B measurements -- every one of them leaves the results unchanged) ----
 *   ORCVIO_COMM_TIMEOUT_S   bound of every wait another rank can strand, seconds (default 180)
 *   ORCVIO_IPC_WAIT_S       ipc transport: bound of the device-side wait for a peer's block, seconds (default 20, at most the above)
 *   ORCVIO_RCCL_LIB         path of the RCCL library to dlopen first (then librccl.so.1 / librccl.so by the loader's search -- an already
 *                           loaded one, e.g. torch's bundled copy, wins --, then /opt/rocm/lib)
 *   ORCVIO_FRAME_OVERLAP    0: orcvio_msckf_io_update_frame runs its two halves one behind the other
 *   ORCVIO_FRAME_CHAIN      0 (read at create; the ONE switch of this list that changes results, in the last bits): the frame call's object
 *                           solve runs BEHIND the feature half, on the covariance and factor it commits -- bit-identical to the two calls.
 *                           Default 1 (windows from six block steps): the object solve is chained to the FEATURE update's prior factor and
 *                           M (M12 = M1 + L_a^T A' L_a: the same sequential update, by Woodbury) and runs on the objects' stream beside the
 *                           feature half's solve and commit -- 7 % of the config-3 frame; equal to the two calls to rounding (1e-10;
 *                           DESIGN.md 3.6), counted in orcvio_msckf_counters [6]
 *   ORCVIO_FUSE_FINISH      (read at create) P+ = s2 Z^T Z, dx and an object update's gate by finish workgroups of the factorisation + solve
 *                           launch instead of a k_finish_sqrt launch behind it (bit-identical either way): 1 (default) in the chained frame
 *                           call, both halves (0.167-0.170 -> 0.160 ms); 2 in every update whose solve takes the look-ahead form (measured
 *                           ~2 us slower per queued update); 0 never
 *   ORCVIO_OBJ_FUSED        0: object tracks always through the three-launch compression over materialised rows (default 1: the one-launch
 *                           compression k_obj_fused whenever every track qualifies, orcvio_msckf_counters [5])
 *   ORCVIO_FUSED_STAMPS     phase stamps of k_obj_fused (object 0) on stderr
 *   ORCVIO_FUSED_TOL        k_obj_fused's pivot tolerance relative to the largest pivot (default 1e-10; tests of its verification step)
 *   ORCVIO_BLK2             0 (read at create): windows beyond the register-resident factorisations (n > 224: 34 .. 60 clones) through the LDS-panel
 *                           Cholesky and k_trsm_rl (0.95-2.1 ms per update) instead of the 2 x 2 block factorisation out of the register kernels
 *                           (0.26-0.41 ms); same results to rounding
 *   ORCVIO_LA_SPIN          polls before a wait inside k_potrf_solve_la gives up
 *                           (default 4 M, seconds; 0 makes every hand-off fail at once: the test of the fall-back)
 *   ORCVIO_FRONT_SPIN, ORCVIO_IO_SPIN_SECONDS   bounds of the in-launch hand-off of k_front (polls) and of the host's flag spin
 *   ORCVIO_TIMING           host wall times of the parts of the one-shot calls on stderr
 *   ORCVIO_ASM_DBG, ORCVIO_POTRF_ABLATE, ORCVIO_POTRF_COLD   kernel diagnostics (scripts/gpu_*.py) */

#ifdef __cplusplus
}
#endif
#endif /* ORCVIO_MSCKF_H */
