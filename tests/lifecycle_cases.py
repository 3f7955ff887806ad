"""Inputs of the in-state feature lifecycle tests (tests/test_features_lifecycle*.py): a window, SLAM features with their
world positions, anchor changes and an SPD covariance over [LEG | clones | features | nuisance]."""
import numpy as np

from orcvio_amd import synth
from mirror_features_lifecycle import AnchorChange, cam_pose


def spd(n, seed, scale=1e-3):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    P = scale * (A @ A.T) + np.diag(rng.uniform(1e-4, 1e-2, n))
    return 0.5 * (P + P.T)


def window(N, seed, leg=22):
    w = synth.make_window(N=N, F=4, seed=seed, track_len=(2, 3), flags=synth.Flags(leg_dim=leg))
    poses = synth.pack_poses(w)
    rng = np.random.default_rng(seed + 77)
    poses[:, 12:15] = poses[:, 9:12] + 0.01 * rng.standard_normal((N, 3))   # t_fej != t_b_w
    return w, poses


def feature_at(poses, anchor, rng):
    """a world point 4-12 m in front of clone `anchor`'s camera, and a nearby FEJ position"""
    R_c2w, t_c_w = cam_pose(poses, anchor)
    pc = np.array([rng.uniform(-1.0, 1.0), rng.uniform(-0.7, 0.7), rng.uniform(4.0, 12.0)])
    p_w = R_c2w @ pc + t_c_w
    return p_w, p_w + 0.02 * rng.standard_normal(3)


def changes(poses, N, nf, k, seed, new_at='newest'):
    """k anchor changes over distinct slots of nf features; old anchors among the two oldest clones, new anchor the newest or
    a middle clone"""
    rng = np.random.default_rng(seed)
    slots = sorted(rng.choice(nf, size=k, replace=False).tolist())
    out = []
    for s in slots:
        old = int(rng.integers(0, 2))
        new = N - 1 if new_at == 'newest' else N // 2
        p_w, p_fej = feature_at(poses, old, rng)
        out.append(AnchorChange(slot=int(s), old=old, new=new, p_w=p_w, p_fej=p_fej))
    return out


def extrinsics(w):
    """the current extrinsics (state_server.imu_state): the window's (all clones share them)"""
    return w.R_b2c[-1].copy(), w.t_c_b[-1].copy()
