"""numpy mirror of the bbox-only ("lite") object mapper: orcvio_msckf_object_init_lite and orcvio_msckf_object_lm_lite -- TEST
INFRASTRUCTURE ONLY.

The problem is the reference's ObjectLMLite (src/obj/ObjectLMLite.cpp:389-415): state x = (wTo, shape v), 9 degrees of freedom in the
column order [pose 6 | shape 3]; w[0] x the four bbox rows of every frame and w[1] x (v - mean_shape) repeated F - 1 times
(include/orcvio/obj/ObjectLMLite.h:288-297: NErrors = 3 (zb.size() - 1), "TODO FIXME why -1"), or F times with reg_every_frame.  The
weights are the initialiser's four-vector read from index 0, not the full functor's (1) and (3).  Huber off.

The bbox rows and their Jacobian come from oracle.mirror_objects.object_rows on frames without keypoints (K = 0); the regulariser is
written here as EXPLICIT rows and the damped system is solved DENSE (np.linalg.solve), so the device's row-free regulariser, its
lane sums and its in-wave Cholesky are checked against something that shares none of them.  The iteration is the one
include/orcvio_msckf.h documents for orcvio_msckf_object_lm (tests/mirror_object_lm.py restates it).

The start follows single_object_initialization_lite (src/obj/ObjectFeatureInitializer.cpp:495-584) matrix by matrix.

The bbox-only optimum is NOT unique in wTo: the ellipsoid is invariant under the half-turns about its axes.  What the cost depends on
is the world dual quadric Q_w = wTo diag(v^2, -1) wTo^T; two results are compared by Q_w (relative to its largest entry), v and the
cost, never by wTo element by element."""
from __future__ import annotations

import dataclasses

import numpy as np

from oracle import mirror_objects as mo
import mirror_object_lm
from mirror_object_lm import STATUS_CONVERGED, STATUS_STALLED, STATUS_MAX_ITER, STATUS_NON_FINITE   # noqa: F401 (re-exported)


@dataclasses.dataclass
class Config:
    left: bool = True
    new_bbox: int = 0
    weights: tuple = (1.0, 1.0)     # (bbox rows, regulariser): the reference's residual_weights(0), (1)
    reg_every_frame: int = 0        # 0: F - 1 repeats (the reference literally); 1: F repeats
    max_iter: int = 60
    ptol: float = 1e-18


def bare_frames(frames):
    """The frames of a track without their keypoint detections (K = 0)."""
    return [dict(fr, zs=np.zeros((0, 2))) for fr in frames]


def reg_repeats(n_frames, cfg: Config):
    return n_frames if cfg.reg_every_frame else n_frames - 1


def regulariser_rows(shape, mean_shape, repeats, w):
    """(r [3 repeats], J [3 repeats x 9]): w (v - mean_shape), once per repeat."""
    J1 = np.zeros((3, 9))
    J1[:, 6:9] = np.eye(3)
    return np.tile(w * (shape - mean_shape), repeats), np.tile(w * J1, (repeats, 1))


def residual_jacobian(wTo, shape, frames, mean_shape, cfg: Config):
    """The stacked weighted residual and its Jacobian w.r.t. [pose 6 | shape 3]: [w0 bbox rows ; w1 regulariser rows].
    frames: bare_frames(..)."""
    res, Hf, _, _ = mo.object_rows(wTo, shape, np.zeros((0, 3)), frames, cfg.left, cfg.new_bbox)
    rs, Js = regulariser_rows(shape, mean_shape, reg_repeats(len(frames), cfg), cfg.weights[1])
    return np.concatenate([cfg.weights[0] * res, rs]), np.vstack([cfg.weights[0] * Hf, Js])


def retract(wTo, shape, d, left):
    """Pose: exp(xi) wTo (left) / wTo exp(xi) (right), xi = (upsilon, omega) = d[:6]; shape additive."""
    E = mo.se3_exp(np.asarray(d[:6], dtype=np.float64))
    return (E @ wTo if left else wTo @ E), shape + d[6:9]


def solve(obj, mean_shape, cfg: Config, first_accepted=False):
    """obj: synth.ObjectTrack-shaped start (wTo rigid; its kps and the frames' zs are ignored).  Returns dict(wTo, shape, cost0, cost,
    iterations, evaluations, status).  first_accepted: stop behind the first accepted trial point (status 3)."""
    mean_shape = np.asarray(mean_shape, dtype=np.float64)
    frames = bare_frames(obj.frames)

    def evaluate(T, v):
        with np.errstate(all='ignore'):
            r, J = residual_jacobian(T, v, frames, mean_shape, cfg)
            return J.T @ J, J.T @ r, float(r @ r)

    state0 = (np.array(obj.wTo, dtype=np.float64), np.array(obj.shape, dtype=np.float64))
    (wTo, shape), out = mirror_object_lm.lm_iterate(evaluate, lambda st, d: retract(*st, d, cfg.left), state0, cfg.max_iter, cfg.ptol, first_accepted)
    out.update(wTo=wTo, shape=shape)
    return out


def quadric_world(wTo, shape):
    """Q_w = wTo diag(v^2, -1) wTo^T: the dual quadric of the ellipsoid in the world frame, what the bbox rows depend on."""
    wTo = np.asarray(wTo, dtype=np.float64)
    return wTo @ mo.ellipse_from_shape(np.asarray(shape, dtype=np.float64)) @ wTo.T


def distance(a, b, mean_shape=None):
    """(Q_w difference relative to the largest entry of b's Q_w, largest difference of v) between two results.  With mean_shape, v is
    compared up to the permutations of the axes that leave the mean shape as it is: where two entries of the mean are EQUAL (one_car's
    class: 1.5, 3, 1.5) the quarter-turn about the third axis together with the exchange of the two semi-axes is one more symmetry of
    the whole cost, regulariser included, and both labellings are the same optimum."""
    import itertools
    Qa, Qb = quadric_world(a['wTo'], a['shape']), quadric_world(b['wTo'], b['shape'])
    va, vb = np.asarray(a['shape'], dtype=np.float64), np.asarray(b['shape'], dtype=np.float64)
    perms = [(0, 1, 2)]
    if mean_shape is not None:
        m = np.asarray(mean_shape, dtype=np.float64)
        perms = [p for p in itertools.permutations(range(3)) if np.array_equal(m[list(p)], m)]
    dv = min(float(np.abs(va[list(p)] - vb).max()) for p in perms)
    return float(np.abs(Qa - Qb).max() / np.abs(Qb).max()), dv


def gradient_norm(wTo, shape, frames, mean_shape, cfg: Config):
    r, J = residual_jacobian(np.asarray(wTo), np.asarray(shape), bare_frames(frames), np.asarray(mean_shape), cfg)
    return float(np.linalg.norm(J.T @ r))


# ---------------------------------------------------------------------------------------------------------------------------------
# the start: single_object_initialization_lite (src/obj/ObjectFeatureInitializer.cpp:495-584)
# ---------------------------------------------------------------------------------------------------------------------------------
def init(frames, mean_shape, bbox_scale=(1.0, 1.0, 1.0), pose_form=1):
    """Returns dict(wTo, d, status): status 1, or 4 (wTo = identity) when wPq is not finite.  pose_form 1 / 2: poseSE32SE2 of an
    identity rotation -- yaw 0 and the translation (x, y, 0); pose_form 0: the full translation."""
    wTc = np.asarray(frames[0]['wTc'], dtype=np.float64)
    R_GtoA = wTc[:3, :3].T                      # Rot_GtoC of the first clone
    p_AinG = wTc[:3, 3]
    cPw = -R_GtoA @ p_AinG
    K = np.eye(3)
    vv = (np.asarray(mean_shape, dtype=np.float64) * np.asarray(bbox_scale, dtype=np.float64)) ** 2
    wRq = np.eye(3)
    A = wRq @ np.diag(vv) @ wRq.T
    B = K @ R_GtoA
    bbox = np.asarray(frames[0]['bbox'], dtype=np.float64)
    lines = mo.poly2lineh(mo.bbox2poly(bbox))
    line_sum = np.zeros((3, 3))
    denominator = 0.0
    for line in lines:
        line_sum += np.outer(line, line)
        denominator += line @ B @ A @ B.T @ line
    with np.errstate(all='ignore'):
        E = B.T @ line_sum @ B / denominator
        b = np.array([(bbox[0] + bbox[2]) / 2, (bbox[1] + bbox[3]) / 2, 1.0])
        Binv = np.linalg.inv(B)
        d = 1.0 / np.sqrt(b @ Binv.T @ E @ Binv @ b)
        wPq = d * Binv @ b - R_GtoA.T @ cPw
    T = np.eye(4)
    if not np.isfinite(wPq).all():
        return dict(wTo=T, d=float(d), status=STATUS_NON_FINITE)
    T[:3, 3] = wPq
    if pose_form != 0:
        T[2, 3] = 0.0
    return dict(wTo=T, d=float(d), status=1)


def init_mp(frames, mean_shape, bbox_scale=(1.0, 1.0, 1.0), pose_form=1):
    """init() evaluated with mpmath at 60 digits from the same float64 inputs, matrix by matrix as the reference writes it (the inverse
    of B included).  Returns dict(wTo [4x4 float64], d)."""
    import mpmath as mp
    mp.mp.dps = 60
    wTc = np.asarray(frames[0]['wTc'], dtype=np.float64)
    R_GtoA = mp.matrix(wTc[:3, :3].T.tolist())
    p_AinG = mp.matrix(wTc[:3, 3].tolist())
    cPw = -R_GtoA * p_AinG
    vv = [(mp.mpf(float(m)) * mp.mpf(float(s))) ** 2 for m, s in zip(mean_shape, bbox_scale)]
    A = mp.diag(vv)
    B = R_GtoA
    bb = [mp.mpf(float(v)) for v in frames[0]['bbox']]
    pts = [(bb[0], bb[1]), (bb[2], bb[1]), (bb[2], bb[3]), (bb[0], bb[3])]
    line_sum = mp.zeros(3, 3)
    denominator = mp.mpf(0)
    for i in range(4):
        (x, y), (xn, yn) = pts[i], pts[(i + 1) % 4]
        line = mp.matrix([y - yn, xn - x, x * yn - y * xn])       # cross((x, y, 1), (x', y', 1))
        line_sum += line * line.T
        denominator += (line.T * B * A * B.T * line)[0]
    E = B.T * line_sum * B / denominator
    b = mp.matrix([(bb[0] + bb[2]) / 2, (bb[1] + bb[3]) / 2, 1])
    Binv = B ** -1
    d = 1 / mp.sqrt((b.T * Binv.T * E * Binv * b)[0])
    wPq = d * Binv * b - R_GtoA.T * cPw
    T = np.eye(4)
    T[:3, 3] = [float(wPq[i]) for i in range(3)]
    if pose_form != 0:
        T[2, 3] = 0.0
    return dict(wTo=T, d=float(d))
