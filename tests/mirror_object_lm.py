"""numpy mirror of the batched object Levenberg-Marquardt (orcvio_msckf_object_lm) -- TEST INFRASTRUCTURE ONLY.

The problem is the reference's ObjectLM (src/obj/ObjectLM.cpp:761-816): weighted keypoint rows, weighted bbox rows, the deformation
regulariser w2 (m_k - mean_k) and the shape regulariser w3 (v - mean_v), both repeated once per frame (:652-684, :732-743), Huber
off.  The rows and their Jacobian w.r.t. the object state come from oracle.mirror_objects.object_rows; the regularisers are written
here as EXPLICIT rows, and the damped system is solved DENSE (np.linalg.solve on the full (9 + 3K)^2 matrix), so that the device's
arrow structure, its Schur elimination and its row-free regularisers are checked against something that shares none of them.

The iteration is the one include/orcvio_msckf.h documents (not MINPACK's trajectory: only the optimum is comparable with Eigen's):
    A = J^T J, g = J^T r, c = |r|^2, D_j = max over the iterations so far of sqrt(A_jj), lambda_0 = 1e-3
    (A + lambda D^2) delta = -g,  pred = -2 g^T delta - delta^T A delta
    pred <= ptol c                  -> status 1 (converged), tested before the trial point is evaluated
    rho = (c - c+) / pred > 1e-4    -> accept, lambda <- max(lambda max(1/3, 1 - (2 rho - 1)^3), 1e-12); else lambda <- 4 lambda
    lambda > 1e12                   -> status 2 (stalled);  max_iter solves -> status 3;  a non-finite number -> status 4
"""
from __future__ import annotations

import dataclasses

import numpy as np

from oracle import mirror_objects as mo

STATUS_CONVERGED, STATUS_STALLED, STATUS_MAX_ITER, STATUS_NON_FINITE = 1, 2, 3, 4


@dataclasses.dataclass
class Config:
    left: bool = True
    new_bbox: int = 0
    weights: tuple = (1.0, 1.0, 1.0, 1.0)
    max_iter: int = 60
    ptol: float = 1e-18


def project_rigid(T):
    """The nearest rigid transform: rotation block projected onto SO(3), last row (0, 0, 0, 1)."""
    T = np.array(T, dtype=np.float64)
    U, _, Vt = np.linalg.svd(T[:3, :3])
    T[:3, :3] = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    T[3] = [0.0, 0.0, 0.0, 1.0]
    return T


def retract(wTo, shape, kps, d, left):
    """Pose: exp(xi) wTo (left) / wTo exp(xi) (right), xi = (upsilon, omega) = d[:6]; shape and keypoints additive."""
    E = mo.se3_exp(np.asarray(d[:6], dtype=np.float64))
    T = E @ wTo if left else wTo @ E
    return T, shape + d[6:9], kps + np.asarray(d[9:]).reshape(-1, 3)


def regulariser_rows(shape, kps, mean_shape, mean_kps, n_frames, w2, w3):
    """The two regulariser blocks as explicit rows: (r_deform [F 3K], J_deform [F 3K x ncol], r_shape [3F], J_shape [3F x ncol]).
    Frame-major; inside a frame keypoint-major (x, y, z of keypoint 0, then keypoint 1, ..: the column-major 3 x K map of
    ObjectLM.cpp:658-661)."""
    K = len(kps)
    ncol = 9 + 3 * K
    Jd1 = np.zeros((3 * K, ncol))
    Jd1[:, 9:] = np.eye(3 * K)
    Js1 = np.zeros((3, ncol))
    Js1[:, 6:9] = np.eye(3)
    rd = np.tile(w2 * (kps - mean_kps).reshape(-1), n_frames)
    rs = np.tile(w3 * (shape - mean_shape), n_frames)
    return rd, np.tile(w2 * Jd1, (n_frames, 1)), rs, np.tile(w3 * Js1, (n_frames, 1))


def residual_jacobian(wTo, shape, kps, frames, mean_shape, mean_kps, cfg: Config):
    """The stacked weighted residual and its Jacobian w.r.t. [pose 6 | shape 3 | 3 per keypoint]:
    [w0 keypoint rows ; w1 bbox rows ; w2 deformation rows ; w3 shape rows]."""
    w = cfg.weights
    res, Hf, _, counts = mo.object_rows(wTo, shape, kps, frames, cfg.left, cfg.new_bbox)
    nk = 2 * sum(counts)
    wt = np.concatenate([np.full(nk, w[0]), np.full(len(res) - nk, w[1])])
    rd, Jd, rs, Js = regulariser_rows(shape, kps, mean_shape, mean_kps, len(frames), w[2], w[3])
    return np.concatenate([wt * res, rd, rs]), np.vstack([wt[:, None] * Hf, Jd, Js])


def lm_iterate(evaluate, retract, state0, max_iter, ptol, first_accepted=False):
    """The iteration of include/orcvio_msckf.h over any state tuple: evaluate(*state) -> (A, g, c), retract(state, d) -> state.
    Returns (state, dict(cost0, cost, iterations, evaluations, status)).  first_accepted: stop behind the first accepted trial
    point (status 3)."""
    state = state0
    A, g, c = evaluate(*state)
    out = dict(cost0=c, evaluations=1, iterations=0, status=STATUS_MAX_ITER)
    lam = 1e-3
    D = np.zeros(len(g))
    if not np.isfinite(c):
        out['status'] = STATUS_NON_FINITE
    else:
        for _ in range(max_iter):
            D = np.maximum(D, np.sqrt(np.diag(A)))
            with np.errstate(all='ignore'):
                try:
                    d = np.linalg.solve(A + lam * np.diag(D * D), -g)
                except np.linalg.LinAlgError:
                    d = np.full(len(g), np.nan)
                pred = -2.0 * (g @ d) - d @ A @ d
            if not np.isfinite(pred):
                out['status'] = STATUS_NON_FINITE
                break
            if pred <= ptol * c:
                out['status'] = STATUS_CONVERGED
                break
            trial = retract(state, d)
            An, gn, cn = evaluate(*trial)
            out['evaluations'] += 1
            out['iterations'] += 1
            if not np.isfinite(cn):
                out['status'] = STATUS_NON_FINITE
                break
            rho = (c - cn) / pred
            accepted = rho > 1e-4
            if accepted:
                state, A, g, c = trial, An, gn, cn
                lam = max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e-12)
            else:
                lam *= 4.0
            if lam > 1e12:
                out['status'] = STATUS_STALLED
                break
            if accepted and first_accepted:
                break
    out['cost'] = c
    return state, out


def solve(obj, mean_shape, mean_kps, cfg: Config):
    """obj: synth.ObjectTrack-shaped start (wTo rigid).  Returns dict(wTo, shape, kps, cost0, cost, iterations, evaluations, status)."""
    mean_shape = np.asarray(mean_shape, dtype=np.float64)
    mean_kps = np.asarray(mean_kps, dtype=np.float64).reshape(-1, 3)
    frames = obj.frames

    def evaluate(T, v, m):
        with np.errstate(all='ignore'):
            r, J = residual_jacobian(T, v, m, frames, mean_shape, mean_kps, cfg)
            return J.T @ J, J.T @ r, float(r @ r)

    state0 = (np.array(obj.wTo, dtype=np.float64), np.array(obj.shape, dtype=np.float64), np.array(obj.kps, dtype=np.float64).reshape(-1, 3))
    (wTo, shape, kps), out = lm_iterate(evaluate, lambda st, d: retract(*st, d, cfg.left), state0, cfg.max_iter, cfg.ptol)
    out.update(wTo=wTo, shape=shape, kps=kps)
    return out


def gradient_norm(wTo, shape, kps, frames, mean_shape, mean_kps, cfg: Config):
    """|J^T r| of the weighted problem at a state (what a first-order optimum makes small)."""
    r, J = residual_jacobian(np.asarray(wTo), np.asarray(shape), np.asarray(kps).reshape(-1, 3), frames,
                             np.asarray(mean_shape), np.asarray(mean_kps).reshape(-1, 3), cfg)
    return float(np.linalg.norm(J.T @ r))
