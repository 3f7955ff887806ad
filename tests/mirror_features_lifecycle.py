"""TEST INFRASTRUCTURE ONLY -- literal numpy restatement of what the reference's hybrid filter does to state_cov when an
in-state SLAM feature is lost or its anchor clone is pruned.

Follows src/orcvio.cpp:
  rmLostFeaturesCov             :3776-3828  (one feature after the other; the nuisance block behind the features stays)
  pruneImuStateBuffer           :2664-2720  (the new anchor and the new parameters the caller sets before the update of P)
  updateFeatureCov_3didp        :3457-3609
  updateFeatureCov_1didp        :3611-3774
  getNewAnchorId                :3892-3950
  measurementUpdate_hybrid      :1698-1735  (the in-state features' increment: parameters += dx, p_w from the anchor pose)
State layout: [legacy LEG | clones 6N | feature states d each | Schmidt nuisance states 6 each].
Clone poses come as [N][28] records (ORCVIO_POSE_STRIDE: R_b2w 9 | t_b_w 3 | t_fej 3 | R_b2c 9 | t_c_b 3 | 1 unused); the camera
pose of a clone is built from its own record as stateAugmentation does (:955-961).  R_b2c / t_c_b passed separately are the
current extrinsics (state_server.imu_state).
Nothing under orcvio_amd/ may import this module.
"""
import dataclasses

import numpy as np

from oracle.mirror import skew


@dataclasses.dataclass
class AnchorChange:
    """One feature whose anchor clone leaves: its slot in feature_states, old and new anchor (window ranks), Feature::position
    and Feature::position_FEJ."""
    slot: int
    old: int
    new: int
    p_w: np.ndarray
    p_fej: np.ndarray = None


def record(poses, i):
    """(R_b2w, t_b_w, t_fej, R_b2c, t_c_b) of pose record i"""
    r = np.asarray(poses[i], dtype=np.float64)
    return r[0:9].reshape(3, 3), r[9:12], r[12:15], r[15:24].reshape(3, 3), r[24:27]


def cam_pose(poses, i):
    """(R_c2w, t_c_w) of clone i: orientation_cam = (R_b2c R_b2w^T)^T, position_cam = t_b_w + R_b2w t_c_b (:955-961)"""
    R_b2w, t_b_w, _, R_b2c, t_c_b = record(poses, i)
    R_w2c = R_b2c @ R_b2w.T
    return R_w2c.T, t_b_w + R_b2w @ t_c_b


# ---- rmLostFeaturesCov ------------------------------------------------------------------------------------------------------
def rm_lost_features_cov(P, leg, N, d, slots):
    """:3776-3828 -- the features at `slots` (positions in feature_states BEFORE the call) leave, one after the other: their d
    rows and columns are deleted, everything behind them (later features, nuisance states) moves up."""
    P = np.array(P, dtype=np.float64, copy=True)
    nf = (P.shape[0] - leg - 6 * N) // d   # (at most: a nuisance block may follow)
    order = list(range(nf))                 # feature_states as slot numbers
    for s in slots:
        seq = order.index(s)
        start = leg + 6 * N + d * seq
        end = start + d
        n = P.shape[0]
        if end < n:
            P[start:n - d, :] = P[end:n, :].copy()
            P[:, start:n - d] = P[:, end:n].copy()
        P = P[:n - d, :n - d].copy()
        order.pop(seq)
    return P


# ---- pruneImuStateBuffer: the new parameters --------------------------------------------------------------------------------
def new_parameters(poses, new, p_w, d):
    """:2680-2687 (3-d: invParam) / :2700-2712 (1-d: invDepth, obs_anchor): (param [3], rho).  1-d param = (u, v, 1)."""
    R_c2w_new, t_c_w_new = cam_pose(poses, new)
    p_new = np.linalg.inv(R_c2w_new) @ (np.asarray(p_w) - t_c_w_new)
    if d == 3:
        inv = np.array([p_new[0] / p_new[2], p_new[1] / p_new[2], 1 / p_new[2]])
        return inv, float(inv[2])
    return np.array([p_new[0] / p_new[2], p_new[1] / p_new[2], 1.0]), float(1 / p_new[2])


# ---- updateFeatureCov_1didp / _3didp ----------------------------------------------------------------------------------------
def feature_cov_jacobian(n, leg, N, d, slot, old, new, poses, R_b2c, t_c_b, p_w, p_fej, param, rho, if_fej, literal_3d=0):
    """The d rows J [d, n] of updateFeatureCov_1didp (:3611-3774) / _3didp (:3457-3609), built as the reference builds them
    (zero row, then block assignments in its order).  param / rho: the NEW parameters the caller has set (invParam, or
    obs_anchor and invDepth).  literal_3d: the 3-d function as written looks the "new" pose and column up under old_state_id."""
    R_b2c = np.asarray(R_b2c, dtype=np.float64).reshape(3, 3)
    t_c_b = np.asarray(t_c_b, dtype=np.float64)
    p_w = np.asarray(p_w, dtype=np.float64)
    p_fej = p_w if p_fej is None else np.asarray(p_fej, dtype=np.float64)
    R_b2w_old, t_b_w_old, tfej_old, _, _ = record(poses, old)
    R_c2w_old, t_c_w_old = cam_pose(poses, old)
    if if_fej:
        p_old = R_b2c @ (R_b2w_old.T @ (p_fej - tfej_old) - t_c_b)
    else:
        p_old = np.linalg.inv(R_c2w_old) @ (p_w - t_c_w_old)
    if d == 3:
        new_look = old if literal_3d else new          # :3487 imu_states_augment[old_state_id]
    else:
        new_look = new
    R_b2w_new, t_b_w_new, tfej_new, _, _ = record(poses, new_look)
    R_w2b_new = R_b2w_new.T
    R_c2w_new, _ = cam_pose(poses, new_look)
    R_w2c_new = R_c2w_new.T
    if if_fej:
        p_bf_w_old = p_fej - tfej_old
        p_bf_w_new = p_fej - tfej_new
    else:
        p_bf_w_old = p_w - t_b_w_old
        p_bf_w_new = p_w - t_b_w_new
    SkewMx = skew(R_w2b_new @ p_bf_w_new - t_c_b)
    Mx = R_w2b_new @ R_b2w_old @ skew(R_b2c.T @ p_old)
    fcol = leg + 6 * N + d * slot
    J = np.zeros((d, n))
    if d == 3:
        inv_new = np.asarray(param, dtype=np.float64)
        J_fp_new = np.eye(3)
        J_fp_new[0, 2] = -inv_new[0]
        J_fp_new[1, 2] = -inv_new[1]
        J_fp_new[2, 2] = -inv_new[2]
        J_fp_new = inv_new[2] * J_fp_new
        J_p = R_w2c_new @ R_c2w_old
        J_x_old = np.zeros((3, 6))
        J_x_old[:, :3] = -R_w2c_new @ skew(p_bf_w_old)
        J_x_old[:, 3:] = R_w2c_new
        J_x_new = np.zeros((3, 6))
        J_x_new[:, :3] = R_w2c_new @ skew(p_bf_w_new)
        J_x_new[:, 3:] = -R_w2c_new
        J_e = np.zeros((3, 6))
        J_e[:, :3] = R_b2c @ (SkewMx - Mx)
        J_e[:, 3:] = R_b2c @ (R_w2b_new @ R_b2w_old - np.eye(3))
        J_pf_old = np.eye(3)
        J_pf_old[0, 2] = -p_old[0]
        J_pf_old[1, 2] = -p_old[1]
        J_pf_old[2, 2] = -p_old[2]
        J_pf_old = p_old[2] * J_pf_old
        H_f_new = J_fp_new @ J_p @ J_pf_old
        H_x_old = J_fp_new @ J_x_old
        H_x_new = J_fp_new @ J_x_new
        H_e = J_fp_new @ J_e
        old_c = leg + 6 * old
        new_c = leg + 6 * (old if literal_3d else new)   # :3544 find(old_state_id)
        J[:, fcol:fcol + 3] = H_f_new
        J[:, old_c:old_c + 6] = H_x_old
        J[:, new_c:new_c + 6] = H_x_new
        J[:, 15:21] = H_e
        return J
    p_old_ = np.linalg.inv(R_c2w_old) @ (p_w - t_c_w_old)
    invDepth_old = 1 / p_old_[2]
    f_old = np.array([p_old_[0] / p_old_[2], p_old_[1] / p_old_[2], 1.0])
    invDepth_new = rho
    J_rho_d_new = -invDepth_new * invDepth_new
    J_d = (R_w2c_new @ R_c2w_old @ f_old)[2]
    J_theta_old = (-R_w2c_new @ skew(p_bf_w_old))[2]
    J_p_old = R_w2c_new[2]
    J_theta_new = (R_w2c_new @ skew(p_bf_w_new))[2]
    J_p_new = (-R_w2c_new)[2]
    J_e_theta = (R_b2c @ (SkewMx - Mx))[2]
    J_e_p = (R_b2c @ (R_w2b_new @ R_b2w_old - np.eye(3)))[2]
    J_d_rho_old = -1 / (invDepth_old * invDepth_old)
    old_c = leg + 6 * old
    new_c = leg + 6 * new
    J[0, fcol] = J_rho_d_new * J_d * J_d_rho_old
    J[0, old_c:old_c + 3] = J_rho_d_new * J_theta_old
    J[0, old_c + 3:old_c + 6] = J_rho_d_new * J_p_old
    J[0, new_c:new_c + 3] = J_rho_d_new * J_theta_new
    J[0, new_c + 3:new_c + 6] = J_rho_d_new * J_p_new
    J[0, 15:18] = J_rho_d_new * J_e_theta
    J[0, 18:21] = J_rho_d_new * J_e_p
    return J


def update_feature_cov(P, J, fcol, d):
    """The covariance part of updateFeatureCov_*: Pfleg = J P, Pff = Pfleg J^T, the feature's rows and columns left and right
    of its own block (right: later features and, under use_schmidt, the nuisance block), then (P + P^T) / 2 of the whole."""
    P = np.array(P, dtype=np.float64, copy=True)
    Pfleg = J @ P
    Pff = Pfleg @ J.T
    left = Pfleg[:, :fcol]
    right = Pfleg[:, fcol + d:]
    P[fcol:fcol + d, fcol:fcol + d] = Pff
    P[fcol:fcol + d, :fcol] = left
    P[:fcol, fcol:fcol + d] = left.T
    P[fcol:fcol + d, fcol + d:] = right
    P[fcol + d:, fcol:fcol + d] = right.T
    return (P + P.T) / 2.0


def change_anchors(P, leg, N, d, poses, R_b2c, t_c_b, changes, if_fej=0, literal_3d=0):
    """pruneImuStateBuffer's in-state branch for every listed change, one feature after the other in the listed order
    (:2664-2720): new parameters, then updateFeatureCov_*.  Returns (P, params [k, 3], rhos [k], J rows [k, d, n])."""
    P = np.array(P, dtype=np.float64, copy=True)
    n = P.shape[0]
    params, rhos, Js = [], [], []
    for c in changes:
        param, rho = new_parameters(poses, c.new, c.p_w, d)
        J = feature_cov_jacobian(n, leg, N, d, c.slot, c.old, c.new, poses, R_b2c, t_c_b, c.p_w, c.p_fej, param, rho, if_fej,
                                 literal_3d)
        P = update_feature_cov(P, J, leg + 6 * N + d * c.slot, d)
        params.append(param)
        rhos.append(rho)
        Js.append(J)
    return P, np.array(params).reshape(-1, 3), np.array(rhos), Js


def change_anchors_batched(P, leg, N, d, Js, changes):
    """The same as one congruence: T = I except the changed features' d rows, which are J; T P T^T, symmetrised."""
    n = P.shape[0]
    T = np.eye(n)
    for c, J in zip(changes, Js):
        f = leg + 6 * N + d * c.slot
        T[f:f + d, :] = J
    Q = T @ P @ T.T
    return (Q + Q.T) / 2.0


# ---- getNewAnchorId -------------------------------------------------------------------------------------------------------
def get_new_anchor_id(clone_ids, poses, observations, rm_ids, p_w):
    """:3892-3950.  clone_ids: the window's state ids, ascending (imu_states_augment order), poses[i] the record of clone_ids[i];
    observations: {state id: (u, v)} of the feature; rm_ids: the involved ids that are about to leave.  The clone among the
    first size - 2 that observed the feature, does not leave and reprojects p_w closest to its observation; else the newest."""
    size = len(clone_ids)
    if size <= 2:
        return clone_ids[-1]
    best, best_id = 99999.0, None
    for i in range(size - 2):
        sid = clone_ids[i]
        if sid not in observations or sid in rm_ids:
            continue
        R_c2w, t_c_w = cam_pose(poses, i)
        p_new = np.linalg.inv(R_c2w) @ (np.asarray(p_w) - t_c_w)
        z = observations[sid]
        dis = float(np.linalg.norm([p_new[0] / p_new[2] - z[0], p_new[1] / p_new[2] - z[1]]))
        if best > dis:
            best, best_id = dis, sid
    return best_id if best_id is not None else clone_ids[-1]


# ---- measurementUpdate_hybrid: the in-state features' increment -------------------------------------------------------------
def increment_features(poses, anchors, params, rhos, dx_feat, d):
    """:1698-1735: parameters += dx (3-d invParam, 1-d invDepth), p_w from the anchor's camera pose.  anchors: window ranks
    (poses: the records AFTER the clones' increment).  Returns (params, rhos, p_w [F, 3])."""
    params = np.array(params, dtype=np.float64, copy=True).reshape(-1, 3)
    rhos = np.array(rhos, dtype=np.float64, copy=True)
    p_w = np.zeros((len(anchors), 3))
    for i, a in enumerate(anchors):
        R_c2w, t_c_w = cam_pose(poses, a)
        if d == 3:
            params[i] += dx_feat[3 * i:3 * i + 3]
            rhos[i] = params[i][2]
            p_c = np.array([params[i][0] / params[i][2], params[i][1] / params[i][2], 1 / params[i][2]])
        else:
            rhos[i] += dx_feat[i]
            p_c = np.array([params[i][0] / rhos[i], params[i][1] / rhos[i], 1 / rhos[i]])
        p_w[i] = R_c2w @ p_c + t_c_w
    return params, rhos, p_w
