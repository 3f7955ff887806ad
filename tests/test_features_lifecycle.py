"""CPU tests of the in-state feature lifecycle: the restatement (tests/mirror_features_lifecycle.py) against central differences
of the reparametrisation map and against itself in batched form, the host-compiled anchor-change math
(orcvio_amd/csrc/feature_anchor.hpp) and the host helper getNewAnchorId against the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import lifecycle_cases as lc
import mirror_features_lifecycle as mfl

_dp = C.POINTER(C.c_double)
_lp = C.POINTER(C.c_longlong)
LEG = 22


def _lib():
    return C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cpp', 'libfeatureanchor.so'))


def _map(poses, old, new, t_old, t_new, t_cb, R_b2c, p_c_old, d):
    """the reparametrisation: the feature at p_c_old in the old camera (old pose t_old, extrinsic t_cb) -> new parameters in
    the new camera (new pose t_new)"""
    ps = poses.copy()
    ps[old, 9:12] = t_old
    ps[new, 9:12] = t_new
    ps[:, 24:27] = t_cb
    R_c2w, t_c_w = mfl.cam_pose(ps, old)
    p_w = R_c2w @ p_c_old + t_c_w
    param, rho = mfl.new_parameters(ps, new, p_w, d)
    return param if d == 3 else np.array([rho]), ps, p_w


def _fd_case(d, seed):
    N = 6
    w, poses = lc.window(N, seed)
    R_b2c, t_c_b = lc.extrinsics(w)
    old, new = 0, 3
    rng = np.random.default_rng(seed)
    p_w, _ = lc.feature_at(poses, old, rng)
    R_c2w, t_c_w = mfl.cam_pose(poses, old)
    p_c = R_c2w.T @ (p_w - t_c_w)
    return N, w, poses, R_b2c, t_c_b, old, new, p_w, p_c


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_1d_jacobian_matches_central_differences(seed):
    N, w, poses, R_b2c, t_c_b, old, new, p_w, p_c = _fd_case(1, seed)
    nf, slot = 3, 1
    n = LEG + 6 * N + nf
    param, rho = mfl.new_parameters(poses, new, p_w, 1)
    J = mfl.feature_cov_jacobian(n, LEG, N, 1, slot, old, new, poses, R_b2c, t_c_b, p_w, None, param, rho, if_fej=0)[0]
    t_old, t_new = poses[old, 9:12].copy(), poses[new, 9:12].copy()
    f = lambda to, tn, tcb, pc: _map(poses, old, new, to, tn, tcb, R_b2c, pc, 1)[0][0]
    h = 1e-6
    # rho column: p_c_old = f_old / rho_old
    rho_old = 1 / p_c[2]
    f_old = p_c * rho_old
    g = lambda r: f(t_old, t_new, t_c_b, f_old / r)
    fd = (g(rho_old + h) - g(rho_old - h)) / (2 * h)
    col = LEG + 6 * N + slot
    assert abs(fd - J[col]) <= 1e-6 * max(1.0, abs(J[col]))
    e = np.eye(3)
    for name, c0, fn in (('old p', LEG + 6 * old + 3, lambda v: f(t_old + v, t_new, t_c_b, p_c)),
                         ('new p', LEG + 6 * new + 3, lambda v: f(t_old, t_new + v, t_c_b, p_c)),
                         ('extrinsic p', 18, lambda v: f(t_old, t_new, t_c_b + v, p_c))):
        fd = np.array([(fn(h * e[a]) - fn(-h * e[a])) / (2 * h) for a in range(3)])
        assert np.abs(fd - J[c0:c0 + 3]).max() <= 1e-6 * max(1.0, np.abs(J[c0:c0 + 3]).max()), name


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_3d_consistent_jacobian_matches_central_differences(seed):
    N, w, poses, R_b2c, t_c_b, old, new, p_w, p_c = _fd_case(3, seed)
    nf, slot = 3, 2
    n = LEG + 6 * N + 3 * nf
    param, rho = mfl.new_parameters(poses, new, p_w, 3)
    J = mfl.feature_cov_jacobian(n, LEG, N, 3, slot, old, new, poses, R_b2c, t_c_b, p_w, None, param, rho, if_fej=0, literal_3d=0)
    t_old, t_new = poses[old, 9:12].copy(), poses[new, 9:12].copy()
    f = lambda to, tn, tcb, pc: _map(poses, old, new, to, tn, tcb, R_b2c, pc, 3)[0]
    h = 1e-6
    inv_old = np.array([p_c[0] / p_c[2], p_c[1] / p_c[2], 1 / p_c[2]])
    pc_of = lambda iv: np.array([iv[0] / iv[2], iv[1] / iv[2], 1 / iv[2]])
    e = np.eye(3)
    col = LEG + 6 * N + 3 * slot
    fd = np.stack([(f(t_old, t_new, t_c_b, pc_of(inv_old + h * e[a])) - f(t_old, t_new, t_c_b, pc_of(inv_old - h * e[a]))) / (2 * h)
                   for a in range(3)], axis=1)
    assert np.abs(fd - J[:, col:col + 3]).max() <= 1e-6 * max(1.0, np.abs(J[:, col:col + 3]).max())
    for name, c0, fn in (('old p', LEG + 6 * old + 3, lambda v: f(t_old + v, t_new, t_c_b, p_c)),
                         ('new p', LEG + 6 * new + 3, lambda v: f(t_old, t_new + v, t_c_b, p_c)),
                         ('extrinsic p', 18, lambda v: f(t_old, t_new, t_c_b + v, p_c))):
        fd = np.stack([(fn(h * e[a]) - fn(-h * e[a])) / (2 * h) for a in range(3)], axis=1)
        assert np.abs(fd - J[:, c0:c0 + 3]).max() <= 1e-6 * max(1.0, np.abs(J[:, c0:c0 + 3]).max()), name


def test_3d_literal_reproduces_the_quirk():
    N, w, poses, R_b2c, t_c_b, old, new, p_w, p_c = _fd_case(3, 5)
    n = LEG + 6 * N + 6
    param, rho = mfl.new_parameters(poses, new, p_w, 3)
    args = (n, LEG, N, 3, 1, old, new, poses, R_b2c, t_c_b, p_w, None, param, rho, 0)
    Jl = mfl.feature_cov_jacobian(*args, literal_3d=1)
    Jc = mfl.feature_cov_jacobian(*args, literal_3d=0)
    nc = LEG + 6 * new
    assert not Jl[:, nc:nc + 6].any()          # the new clone gets no entries
    assert Jc[:, nc:nc + 6].any()
    assert np.abs(Jl - Jc).max() > 1e-3


@pytest.mark.parametrize('d,literal,fej,nui', [(1, 0, 0, 0), (1, 0, 1, 2), (3, 0, 0, 0), (3, 1, 1, 0), (3, 0, 1, 1)])
@pytest.mark.parametrize('k', [1, 5, 16])
def test_batched_congruence_equals_sequential_loop(d, literal, fej, nui, k):
    N, nf = 10, 20
    w, poses = lc.window(N, 11 + k)
    R_b2c, t_c_b = lc.extrinsics(w)
    n = LEG + 6 * N + d * nf + 6 * nui
    P = lc.spd(n, k + 100 * d)
    ch = lc.changes(poses, N, nf, k, seed=k + 7 * d, new_at='newest' if k % 2 else 'middle')
    P_seq, params, rhos, Js = mfl.change_anchors(P, LEG, N, d, poses, R_b2c, t_c_b, ch, if_fej=fej, literal_3d=literal)
    P_bat = mfl.change_anchors_batched(P, LEG, N, d, Js, ch)
    assert np.abs(P_seq - P_bat).max() <= 1e-13 * np.abs(P_seq).max()
    assert np.array_equal(P_seq, P_seq.T)
    # the rows of nothing but the changed features move
    changed = np.zeros(n, bool)
    for c in ch:
        changed[LEG + 6 * N + d * c.slot:LEG + 6 * N + d * c.slot + d] = True
    assert np.array_equal(P_seq[np.ix_(~changed, ~changed)], P[np.ix_(~changed, ~changed)])


def test_remove_features_keeps_order_and_nuisance_block():
    N, d, nf, nui = 4, 3, 6, 2
    n = LEG + 6 * N + d * nf + 6 * nui
    P = lc.spd(n, 3)
    slots = [1, 4, 5]
    got = mfl.rm_lost_features_cov(P, LEG, N, d, slots)
    keep = [i for i in range(n) if not any(LEG + 6 * N + d * s <= i < LEG + 6 * N + d * s + d for s in slots)]
    assert np.array_equal(got, P[np.ix_(keep, keep)])
    assert np.array_equal(got[-12:, -12:], P[-12:, -12:])


@pytest.mark.parametrize('d,literal,fej', [(1, 0, 0), (1, 0, 1), (3, 0, 0), (3, 0, 1), (3, 1, 0), (3, 1, 1)])
def test_host_compiled_math_equals_restatement(built, d, literal, fej):
    lib = _lib()
    N, nf = 8, 5
    w, poses = lc.window(N, 21)
    R_b2c, t_c_b = lc.extrinsics(w)
    n = LEG + 6 * N + d * nf
    worst = 0.0
    for seed in range(6):
        for c in lc.changes(poses, N, nf, 3, seed=seed, new_at='newest' if seed % 2 else 'middle'):
            param, rho = mfl.new_parameters(poses, c.new, c.p_w, d)
            Jr = mfl.feature_cov_jacobian(n, LEG, N, d, c.slot, c.old, c.new, poses, R_b2c, t_c_b, c.p_w, c.p_fej, param, rho, fej, literal)
            po = np.ascontiguousarray(poses[c.old]); pn = np.ascontiguousarray(poses[c.new])
            Rb = np.ascontiguousarray(R_b2c.ravel()); tb = np.ascontiguousarray(t_c_b)
            pw = np.ascontiguousarray(c.p_w); pf = np.ascontiguousarray(c.p_fej)
            gp = np.zeros(3); gr = np.zeros(1); gJ = np.zeros(63)
            lib.orc_test_anchor_change(po.ctypes.data_as(_dp), pn.ctypes.data_as(_dp), Rb.ctypes.data_as(_dp), tb.ctypes.data_as(_dp),
                                       pw.ctypes.data_as(_dp), pf.ctypes.data_as(_dp), d, fej, literal, gp.ctypes.data_as(_dp),
                                       gr.ctypes.data_as(_dp), gJ.ctypes.data_as(_dp))
            # scatter the compact rows to the state's columns, as the kernel does
            Jg = np.zeros((d, n))
            fcol = LEG + 6 * N + d * c.slot
            nc = LEG + 6 * (c.old if (d == 3 and literal) else c.new)
            for r in range(d):
                row = gJ[21 * r:21 * r + 21]
                Jg[r, fcol:fcol + d] += row[:d]
                Jg[r, LEG + 6 * c.old:LEG + 6 * c.old + 6] += row[3:9]
                Jg[r, nc:nc + 6] += row[9:15]
                Jg[r, 15:21] += row[15:21]
            assert not gJ.reshape(3, 21)[d:].any() and not gJ.reshape(3, 21)[:, d:3].any()
            worst = max(worst, np.abs(Jg - Jr).max() / np.abs(Jr).max(), np.abs(gp - param).max() / np.abs(param).max(),
                        abs(gr[0] - rho) / abs(rho))
    assert worst < 1e-13


def _anchor_py_and_cpp(lib, N, poses, p_w, obs, rm):
    ids = np.arange(100, 100 + N, dtype=np.int64) * 3
    want = mfl.get_new_anchor_id(list(ids), poses, {int(ids[i]): z for i, z in obs.items()}, [int(ids[i]) for i in rm], p_w)
    oi = np.ascontiguousarray([ids[i] for i in obs], dtype=np.int64)
    oz = np.ascontiguousarray([obs[i] for i in obs], dtype=np.float64).reshape(-1, 2)
    ri = np.ascontiguousarray([ids[i] for i in rm], dtype=np.int64)
    ps = np.ascontiguousarray(poses)
    pw = np.ascontiguousarray(p_w)
    lib.orc_test_get_new_anchor_id.restype = C.c_longlong
    got = lib.orc_test_get_new_anchor_id(N, ids.ctypes.data_as(_lp), ps.ctypes.data_as(_dp), pw.ctypes.data_as(_dp), len(oi),
                                         oi.ctypes.data_as(_lp) if len(oi) else None, oz.ctypes.data_as(_dp) if len(oi) else None,
                                         len(ri), ri.ctypes.data_as(_lp) if len(ri) else None)
    return int(got), int(want), ids


def test_get_new_anchor_id_host_helper_equals_restatement(built):
    lib = _lib()
    N = 8
    w, poses = lc.window(N, 31)
    rng = np.random.default_rng(31)
    hits = set()
    for trial in range(60):
        p_w, _ = lc.feature_at(poses, int(rng.integers(0, N)), rng)
        obs = {}
        for i in range(N):
            if rng.random() < 0.6:
                R_c2w, t_c_w = mfl.cam_pose(poses, i)
                pc = R_c2w.T @ (p_w - t_c_w)
                obs[i] = pc[:2] / pc[2] + 0.01 * rng.standard_normal(2)
        rm = [i for i in (0, 1) if rng.random() < 0.7]
        got, want, ids = _anchor_py_and_cpp(lib, N, poses, p_w, obs, rm)
        assert got == want
        hits.add('fallback' if want == ids[-1] else 'chosen')
    assert hits == {'fallback', 'chosen'}
    # nobody observed it among the first N - 2: the newest clone; a window of two: the newest
    p_w, _ = lc.feature_at(poses, 0, rng)
    got, want, ids = _anchor_py_and_cpp(lib, N, poses, p_w, {N - 1: np.zeros(2)}, [])
    assert got == want == ids[-1]
    got, want, ids = _anchor_py_and_cpp(lib, 2, poses[:2], p_w, {0: np.zeros(2)}, [])
    assert got == want == ids[-1]


def test_increment_features_moves_p_w_with_the_parameters():
    N = 5
    w, poses = lc.window(N, 41)
    rng = np.random.default_rng(41)
    p_w, _ = lc.feature_at(poses, 2, rng)
    for d in (1, 3):
        param, rho = mfl.new_parameters(poses, 2, p_w, d)
        _, _, pw0 = mfl.increment_features(poses, [2], [param], [rho], np.zeros(d), d)
        assert np.abs(pw0[0] - p_w).max() < 1e-12
        pa, ra, pw1 = mfl.increment_features(poses, [2], [param], [rho], np.full(d, 1e-3), d)
        assert abs(ra[0] - rho - 1e-3) < 1e-15 and np.abs(pw1[0] - p_w).max() > 1e-4


def test_plan_anchor_changes_reports_instead_of_throwing(built):
    lib = _lib()
    assert lib.orc_test_plan_anchor_changes(3, 1) == 1     # OK, one change (to the newest clone)
    assert lib.orc_test_plan_anchor_changes(4, 1) == 10    # the new anchor is not a clone of the window: ORCVIO_ERR_INVALID
    assert lib.orc_test_plan_anchor_changes(3, 0) == 0     # not in the state: nothing to change


def _rot_map(poses, old, new, R_b2c, t_c_b, p_c_old, d, which, delta):
    """the reparametrisation with a rotation perturbed: the old / new clone's R_b2w <- exp(delta) R_b2w (the world-frame error the
    reference's H_theta columns are written for), or the extrinsic R_b2c <- R_b2c exp(-delta) in every record and the current one"""
    from orcvio_amd.synth import so3_exp
    ps = poses.copy()
    Rb = R_b2c.copy()
    if which in ('old', 'new'):
        i = old if which == 'old' else new
        ps[i, 0:9] = (so3_exp(delta) @ ps[i, 0:9].reshape(3, 3)).ravel()
    else:
        Rb = Rb @ so3_exp(-delta)
        ps[:, 15:24] = Rb.ravel()
    R_c2w, t_c_w = mfl.cam_pose(ps, old)
    p_w = R_c2w @ p_c_old + t_c_w
    param, rho = mfl.new_parameters(ps, new, p_w, d)
    return param if d == 3 else np.array([rho])


@pytest.mark.parametrize('d', [1, 3])
@pytest.mark.parametrize('seed', [1, 2])
def test_theta_columns_match_central_differences(d, seed):
    N, w, poses, R_b2c, t_c_b, old, new, p_w, p_c = _fd_case(d, seed)
    n = LEG + 6 * N + 3 * d
    param, rho = mfl.new_parameters(poses, new, p_w, d)
    J = mfl.feature_cov_jacobian(n, LEG, N, d, 1, old, new, poses, R_b2c, t_c_b, p_w, None, param, rho, if_fej=0, literal_3d=0)
    h = 1e-6
    e = np.eye(3)
    for which, c0 in (('old', LEG + 6 * old), ('new', LEG + 6 * new), ('extrinsic', 15)):
        fd = np.stack([(_rot_map(poses, old, new, R_b2c, t_c_b, p_c, d, which, h * e[a]) -
                        _rot_map(poses, old, new, R_b2c, t_c_b, p_c, d, which, -h * e[a])) / (2 * h) for a in range(3)], axis=1)
        Jb = J[:, c0:c0 + 3]
        assert np.abs(fd - Jb).max() <= 1e-6 * max(1.0, np.abs(Jb).max()), which


@pytest.mark.parametrize('d,literal', [(1, 0), (3, 0), (3, 1)])
def test_fej_form_at_the_estimates_equals_the_plain_form(built, d, literal):
    """if_FEJ with position_FEJ = position and every clone's t_fej = t_b_w evaluates the Jacobian at the same point as the plain form:
    the FEJ branch of p_old (from the current extrinsics) is pinned by the plain form, which the central differences pin"""
    lib = _lib()
    N, w, poses, R_b2c, t_c_b, old, new, p_w, p_c = _fd_case(d, 4)
    poses = poses.copy()
    poses[:, 12:15] = poses[:, 9:12]
    n = LEG + 6 * N + 3 * d
    param, rho = mfl.new_parameters(poses, new, p_w, d)
    args = (n, LEG, N, d, 1, old, new, poses, R_b2c, t_c_b, p_w, p_w, param, rho)
    J0 = mfl.feature_cov_jacobian(*args, if_fej=0, literal_3d=literal)
    J1 = mfl.feature_cov_jacobian(*args, if_fej=1, literal_3d=literal)
    assert np.abs(J1 - J0).max() <= 1e-12 * np.abs(J0).max()
    outs = []
    for fej in (0, 1):
        a = [np.ascontiguousarray(x) for x in (poses[old], poses[new], R_b2c.ravel(), t_c_b, p_w, p_w)]
        gp = np.zeros(3); gr = np.zeros(1); gJ = np.zeros(63)
        lib.orc_test_anchor_change(*[x.ctypes.data_as(_dp) for x in a], d, fej, literal, gp.ctypes.data_as(_dp), gr.ctypes.data_as(_dp),
                                   gJ.ctypes.data_as(_dp))
        outs.append(gJ)
    assert np.abs(outs[1] - outs[0]).max() <= 1e-12 * np.abs(outs[0]).max()
