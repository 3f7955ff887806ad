"""TEST INFRASTRUCTURE ONLY -- numpy restatement of OrcVIO::measurementUpdate_ZUPT_vpq (src/orcvio.cpp:3326-3454), written to be
read beside those lines; the checker of orcvio_msckf_cov_zupt / orcvio_msckf_cov_zupt_frame and of the host layer's zuptResidual /
zuptUpdate.  It shares no formula with the device code: the dense H, R_ZUPT, S, the solve, K, (I - K H) P, as the reference has them.

  jacobian            :3329-3334
  residual            :3337-3368 (rotationToQuaternion math_utils.hpp, Eigen's quaternion product)
  measurement_update  :3374-3386, :3431-3447
  increment_features  :3391-3428
  stationary_frame    the frame class of processFeatures on a frame the zero-velocity check accepts (:567-594): propagate, augment,
                      the update, the previous clone marginalised (:2641-2645)
Nothing under orcvio_amd/ may import this module.
"""
import numpy as np


def jacobian(leg, N, n):
    H = np.zeros((9, n))
    H[0:3, 3:6] = np.eye(3)                                   # zupt_v current
    H[3:6, leg + 6 * N - 3: leg + 6 * N] = np.eye(3)          # zupt_p current
    H[3:6, leg + 6 * N - 9: leg + 6 * N - 6] = -np.eye(3)     # zupt_p previous
    H[6:9, leg + 6 * N - 6: leg + 6 * N - 3] = -0.5 * np.eye(3)   # zupt_q current
    H[6:9, leg + 6 * N - 12: leg + 6 * N - 9] = 0.5 * np.eye(3)   # zupt_q previous
    return H


def noise(noise_v, noise_p, noise_q):
    R = np.zeros((9, 9))
    R[0:3, 0:3] = noise_v * np.eye(3)
    R[3:6, 3:6] = noise_p * np.eye(3)
    R[6:9, 6:9] = noise_q * np.eye(3)
    return R


def rotation_to_quaternion(R):
    """math_utils.hpp rotationToQuaternion: (x, y, z, w), Hamilton convention, the branch on the largest of the diagonal and the trace, the scalar part
    made non-negative, then normalised."""
    score = np.array([R[0, 0], R[1, 1], R[2, 2], np.trace(R)])
    k = int(np.argmax(score))
    q = np.zeros(4)
    if k == 0:
        q[0] = np.sqrt(1 + 2 * R[0, 0] - R.trace()) / 2.0
        q[1] = (R[0, 1] + R[1, 0]) / (4 * q[0])
        q[2] = (R[0, 2] + R[2, 0]) / (4 * q[0])
        q[3] = (R[2, 1] - R[1, 2]) / (4 * q[0])
    elif k == 1:
        q[1] = np.sqrt(1 + 2 * R[1, 1] - R.trace()) / 2.0
        q[0] = (R[0, 1] + R[1, 0]) / (4 * q[1])
        q[2] = (R[1, 2] + R[2, 1]) / (4 * q[1])
        q[3] = (R[0, 2] - R[2, 0]) / (4 * q[1])
    elif k == 2:
        q[2] = np.sqrt(1 + 2 * R[2, 2] - R.trace()) / 2.0
        q[0] = (R[0, 2] + R[2, 0]) / (4 * q[2])
        q[1] = (R[1, 2] + R[2, 1]) / (4 * q[2])
        q[3] = (R[1, 0] - R[0, 1]) / (4 * q[2])
    else:
        q[3] = np.sqrt(1 + R.trace()) / 2.0
        q[0] = (R[2, 1] - R[1, 2]) / (4 * q[3])
        q[1] = (R[0, 2] - R[2, 0]) / (4 * q[3])
        q[2] = (R[1, 0] - R[0, 1]) / (4 * q[3])
    if q[3] < 0:
        q = -q
    return q / np.linalg.norm(q)


def _quat_mul(a, b):
    """Eigen's Quaterniond product, both as (w, x, y, z)."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx])


def residual(v, R_prev, p_prev, R_cur, p_cur):
    r = np.zeros(9)
    r[0:3] = -np.asarray(v)
    r[3:6] = -(np.asarray(p_cur) - np.asarray(p_prev))
    q_c = rotation_to_quaternion(np.asarray(R_cur))
    q_p = rotation_to_quaternion(np.asarray(R_prev))
    q_curr = np.array([q_c[3], q_c[0], q_c[1], q_c[2]])
    q_prev = np.array([q_p[3], q_p[0], q_p[1], q_p[2]])
    conj = q_prev * np.array([1.0, -1.0, -1.0, -1.0])
    dq = _quat_mul(q_curr, conj)
    r[6:9] = dq[1:4]
    return r


def measurement_update(P, leg, N, r, noise_v, noise_p, noise_q, n_nui=0):
    """Returns (delta_x, P_new).  n_nui: nuisance states of the Schmidt branch, 6 columns each at the end of the state."""
    n = P.shape[0]
    H = jacobian(leg, N, n)
    R_ZUPT = noise(noise_v, noise_p, noise_q)
    S = H @ P @ H.T + R_ZUPT
    K_transpose = np.linalg.solve(S, H @ P)
    K = K_transpose.T
    delta_x = K @ r
    I_KH = np.eye(n) - K @ H
    if n_nui > 0:
        P_nui = P[n - 6 * n_nui:, n - 6 * n_nui:].copy()
        P_new = I_KH @ P
        P_new[n - 6 * n_nui:, n - 6 * n_nui:] = P_nui
    else:
        P_new = I_KH @ P
    P_new = (P_new + P_new.T) / 2.0
    return delta_x, P_new


def increment_features(delta_x, base_cntr, idp_dim, params, cam_poses):
    """The feature loop (:3391-3428).  params: idp_dim 3 -> invParam [3] per feature; idp_dim 1 -> (obs_anchor [2 or 3], invDepth).
    cam_poses: (R_c2w, t_c_w) of every feature's anchor.  Returns the new parameters (same layout) and the world positions."""
    out, p_ws = [], []
    for i, (par, (R_c2w, t_c_w)) in enumerate(zip(params, cam_poses)):
        if idp_dim == 3:
            inv = np.asarray(par, dtype=np.float64) + delta_x[base_cntr + i * 3: base_cntr + i * 3 + 3]
            p_c = np.array([inv[0] / inv[2], inv[1] / inv[2], 1 / inv[2]])
            out.append(inv)
        else:
            obs, rho = par
            rho = rho + delta_x[base_cntr + i]
            p_c = np.array([obs[0] / rho, obs[1] / rho, 1 / rho])
            out.append((obs, rho))
        p_ws.append(np.asarray(R_c2w) @ p_c + np.asarray(t_c_w))
    return out, np.array(p_ws)


def stationary_frame(P, leg, N_after, r, noises, Phi=None, Q=None, augment=True, remove_previous=True, rest=0, n_nui=0):
    """The host chain of one stationary frame on the covariance: propagate, augment (rest = the states behind the clones), the
    update, the clone at window rank N - 2 marginalised.  Returns (delta_x, P_after)."""
    from oracle import mirror_cov
    if Phi is not None:
        P = mirror_cov.propagate(P, Phi, Q)
    if augment:
        P = mirror_cov.augment(P, rest=rest)
    dx, P = measurement_update(P, leg, N_after, r, *noises, n_nui=n_nui)
    if remove_previous:
        P = mirror_cov.remove_clones(P, leg, [N_after - 2])
    return dx, P
