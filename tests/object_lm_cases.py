"""The cases the object Levenberg-Marquardt is checked on, shared by the mirror's own tests (CPU) and the device tests: the
reference's one_car track (tests/golden/ref_one_car.npz) cut to 47 / 33 / 1 / 2 frames, synthetic tracks in the style of
synth.make_objects for the shapes the fixture does not have (K = 1, K = 16, F = 65, F = 128), projected starts, and the
element-wise distance between two optima.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from orcvio_amd import synth
from oracle import mirror_objects as mo
from helpers import GOLDEN
import mirror_object_lm as mlm

WEIGHTS_REF = (1.0, 3e-2, 1.0, 1.0)    # the reference's test weights (test_object_lm_multiframe.cpp)
WEIGHTS_UNIT = (1.0, 1.0, 1.0, 1.0)


@functools.lru_cache(maxsize=None)
def _one_car_frames():
    g = np.load(GOLDEN + '/ref_one_car.npz')
    frames = []
    for i in range(g['zs'].shape[0]):
        x, y, w, h = g['zb'][i].ravel()
        frames.append(dict(clone=-1, wTc=mlm.project_rigid(g['wTo'][i]), zs=g['zs'][i].astype(np.float64),
                           bbox=np.array([x, y, x + w, y + h], dtype=np.float64)))   # xywh -> xmin, ymin, xmax, ymax
    prior = (g['ellipsoid_shape'][0].ravel().astype(np.float64), g['mean_shape'][0].astype(np.float64))
    return frames, mlm.project_rigid(g['wTq'][0]), prior


def perturbed(T, xi):
    """A start: exp(xi) T, projected onto a rigid transform (the fixture's float32 rotations are orthonormal to 1e-7 only, and the
    left and the right iteration move a non-rigid matrix along different orbits: 3e-5 apart at the end)."""
    return mlm.project_rigid(mo.se3_exp(np.asarray(xi, dtype=np.float64)) @ T)


# Starts as tangent vectors off the fixture's pose.  0 / 1: 1.1 m, 0.14 rad and 7.1 m, 0.37 rad, for the old bbox residual, whose
# cost has ONE minimum within that reach at the reference's weights (measured with the mirror: every run ends at the same point).
# 2 / 3: 0.44 m, 0.07 rad and 0.71 m, 0.09 rad, for the cases with the new bbox residual at unit weights or with one or two
# frames at unit weights: that cost has further local minima (from start 0 the mirror's right chart ends at cost 153.9 instead of
# 1.36 on all 47 frames, from start 1 the one-frame track ends 12 m away), so a comparison of optima needs starts inside one basin.
START_XI = (np.array([0.8, -0.5, 0.6, 0.05, -0.08, 0.10]),
            np.array([-4.0, 3.0, 5.0, -0.20, 0.25, -0.18]),
            np.array([0.3, -0.2, 0.25, 0.03, -0.04, 0.05]),
            np.array([-0.4, 0.3, 0.5, -0.05, 0.06, -0.04]),
            np.array([0.2, 0.3, -0.3, -0.04, 0.03, 0.04]),       # 4 / 5: two more of the near kind (0.47 m, 0.06 rad; 0.44 m, 0.07 rad)
            np.array([-0.3, -0.25, 0.2, 0.05, 0.04, -0.03]))
NEAR_STARTS = (2, 3, 4, 5)

# the five cases of the optimiser's checks: frames of the one_car track, NaN pattern, bbox form, weights, the two starts
CASES = {
    'f47': dict(n_frames=47, nan_case=0, new_bbox=0, weights=WEIGHTS_REF, starts=(0, 1)),
    'f47_unit_bbox2': dict(n_frames=47, nan_case=0, new_bbox=2, weights=WEIGHTS_UNIT, starts=(2, 3)),
    'f33': dict(n_frames=33, nan_case=0, new_bbox=0, weights=WEIGHTS_REF, starts=(0, 1)),
    'f1': dict(n_frames=1, nan_case=0, new_bbox=0, weights=WEIGHTS_REF, starts=(0, 1)),
    'f2_nan': dict(n_frames=2, nan_case=1, new_bbox=0, weights=WEIGHTS_REF, starts=(0, 1)),
}


def one_car(n_frames=47, nan_case=0, start=0):
    """The first n_frames frames of the one_car track, started `start` away from the fixture's object pose at the mean keypoints and
    the mean ellipsoid.  nan_case 1 (two frames): keypoint 3 detected in neither frame, keypoints 0, 7, 9 missing in frame 1 (five NaN
    detections); nan_case 2: keypoint 3 detected nowhere and frame 1 without any detection (its four bbox rows only).  Returns (track, mean_shape, mean_kps)."""
    frames, wTq, (mean_shape, mean_kps) = _one_car_frames()
    frames = [dict(fr, zs=fr['zs'].copy()) for fr in frames[:n_frames]]
    if nan_case == 1:
        frames[0]['zs'][3] = np.nan
        frames[1]['zs'][[0, 3, 7, 9]] = np.nan
    elif nan_case == 2:
        frames[0]['zs'][3] = np.nan
        frames[1]['zs'][:] = np.nan
    obj = synth.ObjectTrack(wTo=perturbed(wTq, START_XI[start]), shape=mean_shape.copy(), kps=mean_kps.copy(), frames=frames)
    return obj, mean_shape, mean_kps


def one_car_truth():
    return _one_car_frames()[1]


def synthetic(K, F, seed, missing_frac=0.1, blind_frame=None, start_scale=1.0, start=0):
    """A synth.make_objects-style track with K keypoints over F frames: a camera moving sideways past a car-sized object 8-15 m
    ahead, keypoint detections with noise and drop-outs, a box around the projected ellipsoid.  blind_frame: that frame has no
    keypoint detection at all.  The start is the truth moved by a few decimetres / hundredths of a radian; `start` = 1, 2, .. gives
    further starts of the same size on the SAME track.
    Returns (track, mean_shape, mean_kps)."""
    rng = np.random.default_rng(1000 * K + F + 7919 * seed)
    sig = 2e-3
    mean_kps = np.vstack([synth.CAR_KEYPOINTS_MEAN, 0.5 * synth.CAR_KEYPOINTS_MEAN[:4] + np.array([0.0, 0.0, 0.3])])[:K].copy()
    mean_shape = synth.CAR_MEAN_SHAPE.copy()
    depth = rng.uniform(8.0, 15.0)
    yaw = rng.uniform(-np.pi, np.pi)
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])
    Rx = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0.0]])      # object z (up) -> camera -y
    T = np.eye(4)
    T[:3, :3] = Rx @ Rz
    T[:3, 3] = [rng.uniform(-0.2, 0.2) * depth, rng.uniform(-0.05, 0.1) * depth, depth]
    kps = mean_kps + 0.03 * rng.standard_normal(mean_kps.shape)
    shape = mean_shape * (1 + 0.05 * rng.standard_normal(3))
    frames = []
    for i in range(F):
        wTc = np.eye(4)
        wTc[:3, :3] = synth.so3_exp(0.03 * rng.standard_normal(3))
        wTc[:3, 3] = [6.0 * (i - 0.5 * (F - 1)) / max(F, 8), 0.05 * rng.standard_normal(), 0.1 * rng.standard_normal()]
        cTw = np.linalg.inv(wTc)
        Xc = (cTw @ T @ np.hstack([kps, np.ones((K, 1))]).T).T
        zs = Xc[:, :2] / Xc[:, 2:3] + sig * rng.standard_normal((K, 2))
        zs[rng.random(K) < missing_frac] = np.nan
        if blind_frame == i:
            zs[:] = np.nan
        cor = np.array([[sx * shape[0], sy * shape[1], sz * shape[2], 1.0] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
        Cc = (cTw @ T @ cor.T).T
        cuv = Cc[:, :2] / Cc[:, 2:3]
        bbox = np.array([cuv[:, 0].min(), cuv[:, 1].min(), cuv[:, 0].max(), cuv[:, 1].max()]) + sig * rng.standard_normal(4)
        frames.append(dict(clone=-1, wTc=wTc, zs=zs, bbox=bbox))
    if start:
        rng = np.random.default_rng(1000 * K + F + 7919 * seed + 104729 * start)
    xi = start_scale * np.concatenate([0.3 * rng.standard_normal(3), 0.03 * rng.standard_normal(3)])
    obj = synth.ObjectTrack(wTo=perturbed(T, xi), shape=mean_shape.copy(), kps=mean_kps.copy(), frames=frames)
    return obj, mean_shape, mean_kps


def distance(a, b):
    """Largest element-wise difference of wTo, shape and keypoints between two results."""
    return max(float(np.abs(np.asarray(a['wTo']) - np.asarray(b['wTo'])).max()),
               float(np.abs(np.asarray(a['shape']) - np.asarray(b['shape'])).max()),
               float(np.abs(np.asarray(a['kps']) - np.asarray(b['kps'])).max()))


@functools.lru_cache(maxsize=None)
def mirror_one_car(n_frames, nan_case, start, left, new_bbox, weights, max_iter=60):
    """The mirror's result on a one_car case (computed once per session and shared: do not modify)."""
    obj, ms, mk = one_car(n_frames, nan_case, start)
    return mlm.solve(obj, ms, mk, mlm.Config(left=left, new_bbox=new_bbox, weights=weights, max_iter=max_iter))


@functools.lru_cache(maxsize=None)
def mirror_spread(n_frames, nan_case, new_bbox, weights, starts=(0, 1), max_iter=60):
    """The mirror's own start-to-start spread on a one_car case: two starts x left / right perturbation.  Returns (spread, runs),
    runs in the order (start a, left), (start a, right), (start b, left), (start b, right)."""
    runs = [mirror_one_car(n_frames, nan_case, s, left, new_bbox, weights, max_iter) for s in starts for left in (True, False)]
    return max(distance(a, b) for a in runs for b in runs), runs


def case_spread(name):
    c = CASES[name]
    return mirror_spread(c['n_frames'], c['nan_case'], c['new_bbox'], c['weights'], c['starts'])


@functools.lru_cache(maxsize=None)
def mirror_synthetic(K, F, seed, start, left, weights=WEIGHTS_UNIT, start_scale=0.3):
    """The mirror's result on a synthetic track (old bbox residual), computed once per session: do not modify."""
    obj, ms, mk = synthetic(K, F, seed, start_scale=start_scale, start=start)
    return mlm.solve(obj, ms, mk, mlm.Config(left=left, new_bbox=0, weights=weights))


def synthetic_spread(K, F, seed, weights=WEIGHTS_UNIT, start_scale=0.3):
    """The mirror's own spread on a synthetic track: two projected starts x left / right perturbation, as case_spread.  Returns
    (spread, runs), runs in the order (start 0, left), (start 0, right), (start 1, left), (start 1, right)."""
    runs = [mirror_synthetic(K, F, seed, s, left, weights, start_scale) for s in (0, 1) for left in (True, False)]
    return max(distance(a, b) for a in runs for b in runs), runs
