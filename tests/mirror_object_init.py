"""numpy mirror of the object initialiser (orcvio_msckf_object_init) and its 60-digit evaluation -- TEST INFRASTRUCTURE ONLY.

The arithmetic is ObjectFeatureInitializer::single_object_initialization's (src/obj/ObjectFeatureInitializer.cpp:33-198): a linear
triangulation of every keypoint over the frames that detected it (single_triangulation_common, src/feat/FeatureInitializer.cpp:6-111:
anchor = the last such frame, rows Bperp_i p = Bperp_i p_CiinA), solved here with np.linalg.lstsq on the 2M x 3 matrix (the device
forms the normal equations), then findTransform (:265-344) with np.linalg.svd (the device: a one-sided Jacobi), then one of three
rigid pose forms (include/orcvio_msckf.h).  `solve_mp` evaluates both stages with mpmath at 60 digits from the same inputs.
"""
from __future__ import annotations

import dataclasses

import numpy as np

STATUS_OK, STATUS_TOO_FEW, STATUS_NON_FINITE = 1, 2, 4


@dataclasses.dataclass
class Config:
    pose_form: int = 1
    min_obs: int = 3
    min_kps: int = 3


def track_arrays(obj):
    """(wTc [F][4][4], zs [F][K][2]) of a synth.ObjectTrack-shaped track."""
    wTc = np.stack([np.asarray(fr['wTc'], dtype=np.float64) for fr in obj.frames])
    zs = np.stack([np.asarray(fr['zs'], dtype=np.float64).reshape(-1, 2) for fr in obj.frames])
    return wTc, zs


def detected(zs, k):
    """Frames in which keypoint k has both coordinates finite."""
    return np.flatnonzero(np.isfinite(zs[:, k, 0]) & np.isfinite(zs[:, k, 1]))


def triangulation_system(wTc, zs, k, frames):
    """(A [2M][3], b [2M], R_GtoA^T, p_AinG) of keypoint k over `frames`, anchored at the last of them (:45-86)."""
    a = frames[-1]
    Ra, ta = wTc[a, :3, :3], wTc[a, :3, 3]            # R_GtoA = Ra^T, p_AinG = ta
    A = np.zeros((2 * len(frames), 3))
    b = np.zeros(2 * len(frames))
    for c, f in enumerate(frames):
        Ri, ti = wTc[f, :3, :3], wTc[f, :3, 3]
        R_AtoCi = Ri.T @ Ra
        p_CiinA = Ra.T @ (ti - ta)
        bi = R_AtoCi.T @ np.array([zs[f, k, 0], zs[f, k, 1], 1.0])
        bi = bi / np.linalg.norm(bi)
        Bperp = np.array([[-bi[2], 0.0, bi[0]], [0.0, bi[2], -bi[1]]])
        A[2 * c:2 * c + 2] = Bperp
        b[2 * c:2 * c + 2] = Bperp @ p_CiinA
    return A, b, Ra, ta


def triangulate(wTc, zs, k, frames, normal_equations=False):
    """(p_FinG, cond(A)) of keypoint k."""
    A, b, Ra, ta = triangulation_system(wTc, zs, k, frames)
    if normal_equations:
        p = np.linalg.solve(A.T @ A, A.T @ b)
    else:
        p = np.linalg.lstsq(A, b, rcond=None)[0]
    sv = np.linalg.svd(A, compute_uv=False)
    return Ra @ p + ta, float(sv[0] / sv[-1])


def pose_from_literal(R, t, scale, in_ctr, out_ctr, pose_form):
    """The three rigid forms of include/orcvio_msckf.h from the pieces of findTransform's literal matrix [scale R | t]."""
    T = np.eye(4)
    if pose_form == 0:
        T[:3, :3] = R
        T[:3, 3] = out_ctr - R @ in_ctr
        return T
    at = np.arctan2(scale * R[1, 0], scale * R[0, 0])
    with np.errstate(divide='ignore'):
        yaw = np.pi / at if pose_form == 1 else at
    if not np.isfinite(yaw):
        yaw = 0.0
    T[0, 0], T[0, 1], T[0, 3] = np.cos(yaw), -np.sin(yaw), t[0]
    T[1, 0], T[1, 1], T[1, 3] = np.sin(yaw), np.cos(yaw), t[1]
    return T


def kabsch(mean_kps, kps_world, used, cfg: Config):
    """findTransform (:265-344) over the used keypoints in increasing id and the pose form.  Returns dict(status, wTo, R, t, scale,
    sigma, d, ratio) with ratio = sigma_1 / (sigma_2 + d sigma_3), the factor of the rotation's perturbation bound."""
    ids = [int(k) for k in np.flatnonzero(used)]
    out = dict(status=STATUS_TOO_FEW, wTo=np.eye(4), R=np.full((3, 3), np.nan), t=np.full(3, np.nan), scale=np.nan,
               sigma=np.full(3, np.nan), d=np.nan, ratio=np.nan, n_used=len(ids))
    if not len(ids) > cfg.min_kps:
        return out
    pin = np.asarray(mean_kps, dtype=np.float64)[ids].T          # 3 x n
    pout = np.asarray(kps_world, dtype=np.float64)[ids].T
    dist_in = sum(np.linalg.norm(pin[:, c + 1] - pin[:, c]) for c in range(len(ids) - 1))
    dist_out = sum(np.linalg.norm(pout[:, c + 1] - pout[:, c]) for c in range(len(ids) - 1))
    with np.errstate(all='ignore'):
        scale = dist_out / dist_in
        ps = pout / scale
        in_ctr, out_ctr = pin.mean(axis=1), ps.mean(axis=1)
        Cov = (pin - in_ctr[:, None]) @ (ps - out_ctr[:, None]).T
        if not np.all(np.isfinite(Cov)):
            out['status'] = STATUS_NON_FINITE
            return out
        U, S, Vt = np.linalg.svd(Cov)
        V = Vt.T
        d = 1.0 if np.linalg.det(V @ U.T) > 0 else -1.0
        R = V @ np.diag([1.0, 1.0, d]) @ U.T
        t = scale * (out_ctr - R @ in_ctr)
    out.update(R=R, t=t, scale=float(scale), sigma=S, d=d, ratio=float(S[0] / (S[1] + d * S[2])))
    if not (np.isfinite(scale) and np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        out['status'] = STATUS_NON_FINITE
        return out
    out['status'] = STATUS_OK
    out['wTo'] = pose_from_literal(R, t, scale, in_ctr, pout.mean(axis=1), cfg.pose_form)
    return out


def literal_matrix(res):
    """findTransform's return value, which is not rigid: [scale R | t]."""
    T = np.eye(4)
    T[:3, :3] = res['scale'] * np.asarray(res['R'])
    T[:3, 3] = res['t']
    return T


def solve(obj, mean_kps, cfg: Config = Config(), normal_equations=False):
    """obj: synth.ObjectTrack-shaped (its frames are read).  Returns dict(status, wTo, R, t, scale, sigma, d, ratio, kps_world [K][3],
    kp_used [K], kp_obs [K], kp_cond [K], n_used)."""
    wTc, zs = track_arrays(obj)
    K = zs.shape[1]
    kps_world = np.full((K, 3), np.nan)
    used = np.zeros(K, dtype=np.int32)
    obs = np.zeros(K, dtype=np.int32)
    cond = np.full(K, np.nan)
    for k in range(K):
        fr = detected(zs, k)
        obs[k] = len(fr)
        if len(fr) > cfg.min_obs:
            used[k] = 1
            with np.errstate(all='ignore'):
                kps_world[k], cond[k] = triangulate(wTc, zs, k, fr, normal_equations)
    out = kabsch(mean_kps, kps_world, used, cfg)
    out.update(kps_world=kps_world, kp_used=used, kp_obs=obs, kp_cond=cond)
    return out


# ---- the 60-digit evaluation -----------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath


def triangulate_mp(wTc, zs, k, frames):
    """p_FinG of keypoint k at 60 digits (the least-squares solution through the normal equations, exact to ~60 - 2 log10 cond digits)."""
    mp = _mp()
    a = frames[-1]
    M = lambda X: mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(X)])
    Ra, ta = M(wTc[a, :3, :3]), M(wTc[a, :3, 3]).T
    A = mp.zeros(2 * len(frames), 3)
    b = mp.zeros(2 * len(frames), 1)
    for c, f in enumerate(frames):
        Ri, ti = M(wTc[f, :3, :3]), M(wTc[f, :3, 3]).T
        p_CiinA = Ra.T * (ti - ta)
        bi = (Ri.T * Ra).T * mp.matrix([mp.mpf(float(zs[f, k, 0])), mp.mpf(float(zs[f, k, 1])), mp.mpf(1)])
        bi = bi / mp.norm(bi)
        Bp = mp.matrix([[-bi[2], 0, bi[0]], [0, bi[2], -bi[1]]])
        bb = Bp * p_CiinA
        for r in range(2):
            for j in range(3):
                A[2 * c + r, j] = Bp[r, j]
            b[2 * c + r] = bb[r]
    p = mp.lu_solve(A.T * A, A.T * b)
    return Ra * p + ta


def kabsch_mp(mean_kps, kps_world_mp, ids, pose_form):
    """(wTo, R, t, scale, sigma) at 60 digits from mp points (a list of 3 x 1 mp matrices indexed by keypoint id)."""
    mp = _mp()
    pin = [mp.matrix([mp.mpf(float(v)) for v in mean_kps[k]]) for k in ids]
    pout = [kps_world_mp[k] for k in ids]
    n = len(ids)
    dist_in = sum(mp.norm(pin[c + 1] - pin[c]) for c in range(n - 1))
    dist_out = sum(mp.norm(pout[c + 1] - pout[c]) for c in range(n - 1))
    scale = dist_out / dist_in
    ps = [p / scale for p in pout]
    in_ctr = sum(pin[1:], pin[0]) / n
    out_ctr = sum(ps[1:], ps[0]) / n
    raw_ctr = sum(pout[1:], pout[0]) / n
    Cov = mp.zeros(3, 3)
    for a, b in zip(pin, ps):
        Cov += (a - in_ctr) * (b - out_ctr).T
    U, S, Vt = mp.svd_r(Cov)
    V = Vt.T
    d = 1 if mp.det(V * U.T) > 0 else -1
    R = V * mp.diag([1, 1, d]) * U.T
    t = scale * (out_ctr - R * in_ctr)
    T = mp.eye(4)
    if pose_form == 0:
        tt = raw_ctr - R * in_ctr
        for i in range(3):
            for j in range(3):
                T[i, j] = R[i, j]
            T[i, 3] = tt[i]
    else:
        at = mp.atan2(scale * R[1, 0], scale * R[0, 0])
        yaw = (mp.pi / at if pose_form == 1 else at) if at != 0 or pose_form == 2 else mp.mpf(0)
        T[0, 0], T[0, 1], T[0, 3] = mp.cos(yaw), -mp.sin(yaw), t[0]
        T[1, 0], T[1, 1], T[1, 3] = mp.sin(yaw), mp.cos(yaw), t[1]
    return T, R, t, scale, S


def solve_mp(obj, mean_kps, cfg: Config = Config()):
    """The 60-digit evaluation of both stages, rounded to float64 at the very end.  Returns dict(status, wTo, R, t, scale, sigma,
    kps_world, kp_used) (status 1 or 2 only: measured tracks do not reach the non-finite branch)."""
    mp = _mp()
    wTc, zs = track_arrays(obj)
    K = zs.shape[1]
    pts, ids = {}, []
    for k in range(K):
        fr = detected(zs, k)
        if len(fr) > cfg.min_obs:
            pts[k] = triangulate_mp(wTc, zs, k, fr)
            ids.append(k)
    to_np = lambda X: np.array([[float(X[i, j]) for j in range(X.cols)] for i in range(X.rows)])
    kps_world = np.full((K, 3), np.nan)
    for k in ids:
        kps_world[k] = to_np(pts[k]).ravel()
    used = np.zeros(K, dtype=np.int32)
    used[ids] = 1
    out = dict(status=STATUS_TOO_FEW, wTo=np.eye(4), kps_world=kps_world, kp_used=used)
    if len(ids) > cfg.min_kps:
        T, R, t, scale, S = kabsch_mp(np.asarray(mean_kps, dtype=np.float64), pts, ids, cfg.pose_form)
        out.update(status=STATUS_OK, wTo=to_np(T), R=to_np(R), t=to_np(t).ravel(), scale=float(scale),
                   sigma=np.array(sorted((float(S[i]) for i in range(3)), reverse=True)))
    return out


def relative_error(a, b):
    """max |a - b| / max |b| over the finite entries of b (the mirror's error against the 60-digit evaluation)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.isfinite(b)
    return float(np.abs(a[m] - b[m]).max() / np.abs(b[m]).max())
