"""The cases the lite (bbox-only) object mapper is checked on, shared by the mirror's own tests (CPU) and the device tests: synthetic
tracks of object_lm_cases.synthetic with the keypoints dropped, the reference's one_car track, and the mirror's runs on them, each
computed once per session.  TEST INFRASTRUCTURE ONLY.

The bbox-only cost has further local minima on some tracks (the mirror's own four runs -- two starts x both charts -- end up to 1e-2
apart in Q_w), so a case enters a comparison of optima only if those four runs agree in Q_w and v within CAP = 1e-7.  The lists
below are the (F, seed) pairs on which they do, at unit weights and reg_every_frame = 0, max_iter = 400 (the mirror needs up to 326
iterations at F = 2); tests/test_object_lite_mirror.py re-checks the short ones, the device tests assert the cap on every case they
use."""
import dataclasses
import functools

import numpy as np

import mirror_object_lite as ml
import object_lm_cases as oc

CAP = 1e-7
MAX_ITER = 400
START_SCALE = 0.3
UNIT = (1.0, 1.0)
REFW = (3e-2, 1.0)      # the bbox weight of the reference's test (test_object_lm_multiframe.cpp) in the lite functor's slot

# (F, seed) with a unique optimum among the mirror's four runs
UNIQUE_OLD = [(2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (16, 1), (16, 2), (17, 1), (17, 2), (65, 1), (65, 2), (128, 2)]   # use_new_bbox_residual = 0
UNIQUE_NEW = [(2, 2), (3, 2), (4, 1), (17, 2), (65, 2), (128, 1), (128, 2)]                                              # = 2


def lite(obj):
    """The track without its keypoints (K = 0): what the lite calls return and what update_object_tracks takes as a bbox-only track."""
    return dataclasses.replace(obj, kps=np.zeros((0, 3)))


@functools.lru_cache(maxsize=None)
def synthetic(F, seed, start=0):
    """(track, mean_shape): object_lm_cases.synthetic(4, F, seed) started START_SCALE away from the truth at the mean shape."""
    obj, ms, _ = oc.synthetic(4, F, seed, start_scale=START_SCALE, start=start)
    return lite(obj), ms


@functools.lru_cache(maxsize=None)
def mirror_synthetic(F, seed, start, left, new_bbox, weights=UNIT, reg_every_frame=0):
    """The mirror's result on a synthetic track, computed once per session: do not modify."""
    obj, ms = synthetic(F, seed, start)
    return ml.solve(obj, ms, ml.Config(left=left, new_bbox=new_bbox, weights=weights, reg_every_frame=reg_every_frame, max_iter=MAX_ITER))


def spread_of(runs):
    """The largest pairwise distance among runs, in Q_w (relative to its largest entry) and in v."""
    return max(max(ml.distance(a, b)) for a in runs for b in runs)


@functools.lru_cache(maxsize=None)
def synthetic_spread(F, seed, new_bbox, weights=UNIT, reg_every_frame=0):
    """(spread, runs): two starts x left / right, runs in the order (start 0, left), (start 0, right), (start 1, left), (start 1, right)."""
    runs = [mirror_synthetic(F, seed, s, left, new_bbox, weights, reg_every_frame) for s in (0, 1) for left in (True, False)]
    return spread_of(runs), runs


@functools.lru_cache(maxsize=None)
def one_car(n_frames=47, start=2):
    """The first n_frames frames of the reference's one_car track without keypoints, from one of object_lm_cases' near starts."""
    obj, ms, _ = oc.one_car(n_frames, 0, start)
    return lite(obj), ms


@functools.lru_cache(maxsize=None)
def mirror_one_car(n_frames, start, left, new_bbox=0, weights=UNIT):
    obj, ms = one_car(n_frames, start)
    return ml.solve(obj, ms, ml.Config(left=left, new_bbox=new_bbox, weights=weights, max_iter=MAX_ITER))


@functools.lru_cache(maxsize=None)
def one_car_spread(n_frames=47, starts=(2, 3)):
    runs = [mirror_one_car(n_frames, s, left) for s in starts for left in (True, False)]
    return spread_of(runs), runs
