"""CPU tests around the zero-velocity update: the restatement in tests/mirror_zupt.py against two other forms of the same update
(information form, Joseph form), and the host layers (capi.zupt_residual, the C++ zuptResidual and the increments behind
orcvio_msckf_cov_zupt's dx, through tests/cpp/zupt_shim.cpp) against the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror
import lifecycle_cases as lc
import mirror_zupt as mz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISES = synth.ZUPT_NOISES
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope='module')
def shim(built):
    capi.load()
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'cpp', 'libzuptshim.so'))
    lib.orc_test_zupt_residual.argtypes = [_dp] * 6
    lib.orc_test_zupt_residual.restype = None
    lib.orc_test_zupt_increment.argtypes = [C.c_int] * 5 + [_dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), _dp, C.c_int,
                                            _dp, _dp, _dp, _dp]
    lib.orc_test_zupt_increment.restype = C.c_int
    return lib


def _d(a):
    return a.ctypes.data_as(_dp)


@pytest.mark.parametrize('leg,N,extra', [(22, 2, 0), (22, 7, 1), (46, 5, 6), (22, 20, 12)])
def test_mirror_equals_the_information_form_and_the_joseph_form(leg, N, extra):
    n = leg + 6 * N + extra
    P = lc.spd(n, n)
    r = np.random.default_rng(n).standard_normal(9) * 1e-3
    dx, Pn = mz.measurement_update(P, leg, N, r, *NOISES)
    H, R = mz.jacobian(leg, N, n), mz.noise(*NOISES)
    Pinfo = np.linalg.inv(np.linalg.inv(P) + H.T @ np.linalg.solve(R, H))
    cond = np.linalg.cond(P)
    assert np.abs(Pn - Pinfo).max() <= 1e-13 * cond * np.abs(Pn).max(), (np.abs(Pn - Pinfo).max(), cond)   # (two inversions of P)
    K = P @ H.T @ np.linalg.inv(H @ P @ H.T + R)
    A = np.eye(n) - K @ H
    Pj = A @ P @ A.T + K @ R @ K.T
    assert np.abs(Pn - Pj).max() <= 1e-13 * np.abs(Pn).max()
    assert np.abs(dx - K @ r).max() <= 1e-13 * np.abs(dx).max()
    assert np.array_equal(Pn, Pn.T)
    # the update takes information in: the measured directions' variance drops, nothing grows
    assert np.all(np.diag(Pn) <= np.diag(P) * (1 + 1e-12)) and np.diag(H @ Pn @ H.T).sum() < 0.9 * np.diag(H @ P @ H.T).sum()


@pytest.mark.parametrize('nui', [1, 2])
def test_schmidt_block_is_the_priors(nui):
    leg, N = 22, 4
    n = leg + 6 * N + 6 * nui
    P = lc.spd(n, 3 + nui)
    r = np.random.default_rng(nui).standard_normal(9) * 1e-3
    _, Pn = mz.measurement_update(P, leg, N, r, *NOISES, n_nui=nui)
    _, Pfull = mz.measurement_update(P, leg, N, r, *NOISES)
    k = n - 6 * nui
    assert np.array_equal(Pn[k:, k:], P[k:, k:])
    assert np.array_equal(Pn[:k, :], Pfull[:k, :]) and np.array_equal(Pn[:, :k], Pfull[:, :k])
    assert np.abs(Pfull[k:, k:] - P[k:, k:]).max() > 0


def _rotations(seed, count):
    """random pose pairs; every third pair a rotation within 1e-3 .. 1e-6 of pi about a random axis (each branch of rotationToQuaternion)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        w = rng.standard_normal(3)
        if k % 3 == 0:
            w *= (np.pi - 10.0 ** -rng.uniform(3, 6)) / np.linalg.norm(w)
        Rp = synth.so3_exp(rng.standard_normal(3))
        out.append((Rp, synth.so3_exp(w) @ Rp if k % 2 else Rp @ synth.so3_exp(w)))
    return out


def test_residual_of_both_host_layers_equals_the_mirror(shim):
    rng = np.random.default_rng(11)
    branches = set()
    for R_prev, R_cur in _rotations(5, 60) + [(np.eye(3), np.eye(3))]:
        v, p_prev = rng.standard_normal(3) * 0.01, rng.standard_normal(3)
        p_cur = p_prev + 1e-3 * rng.standard_normal(3)
        ref = mz.residual(v, R_prev, p_prev, R_cur, p_cur)
        got = capi.zupt_residual(v, R_prev, p_prev, R_cur, p_cur)
        cpp = np.zeros(9)
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (v, R_prev, p_prev, R_cur, p_cur)]
        shim.orc_test_zupt_residual(*[_d(x) for x in a], _d(cpp))
        assert np.abs(got - ref).max() <= 1e-15, np.abs(got - ref).max()
        assert np.abs(cpp - ref).max() <= 1e-15, np.abs(cpp - ref).max()
        for R in (R_prev, R_cur):
            branches.add(int(np.argmax([R[0, 0], R[1, 1], R[2, 2], np.trace(R)])))
        # what the residual means: dq is the rotation from prev to cur, |vector part| = sin(angle / 2)
        dR = R_cur @ R_prev.T
        ang = np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))
        assert abs(np.linalg.norm(ref[6:9]) - np.sin(ang / 2)) < 1e-7
    assert branches == {0, 1, 2, 3}


@pytest.mark.parametrize('idp', [1, 3])
@pytest.mark.parametrize('flags', [dict(use_larvio=1), dict(use_larvio=0, use_left_perturbation=1), dict(use_larvio=0, use_left_perturbation=0)],
                         ids=['larvio', 'left', 'right'])
@pytest.mark.parametrize('nui', [0, 1])
def test_state_and_feature_increments_equal_the_mirror(shim, idp, flags, nui):
    N, nf, leg = 5, 4, 22
    f = synth.Flags(**flags)
    rng = np.random.default_rng(7 + idp + 10 * nui)
    w = synth.make_window(N=N, F=2, seed=3, track_len=3)
    st = dict(R_b2w_imu=w.R_b2w[-1].copy(), v=rng.standard_normal(3), p=w.t_b_w[-1].copy(), bg=rng.standard_normal(3) * 1e-2,
              ba=rng.standard_normal(3) * 1e-2, R_b2c=w.R_b2c[0].copy(), t_c_b=w.t_c_b[0].copy(), td=np.float64(0.0),
              R_b2w=w.R_b2w.copy(), t_b_w=w.t_b_w.copy())
    n = leg + 6 * N + idp * nf + 6 * nui
    dx = rng.standard_normal(n) * 0.01
    anchors = np.array([0, N - 1, 2, N if nui else 1], dtype=np.int32)   # (the last one at the nuisance state when there is one)
    nui_cam = np.concatenate([synth.so3_exp(rng.standard_normal(3)).ravel(), rng.standard_normal(3)])[None, :].repeat(max(nui, 1), 0).copy()
    if idp == 3:
        param = np.stack([rng.uniform(-0.3, 0.3, nf), rng.uniform(-0.3, 0.3, nf), rng.uniform(0.1, 0.3, nf)], axis=1)
        rho = np.zeros(nf)
        params = [p.copy() for p in param]
    else:
        param = np.stack([rng.uniform(-0.3, 0.3, nf), rng.uniform(-0.3, 0.3, nf), np.ones(nf)], axis=1)
        rho = rng.uniform(0.1, 0.3, nf)
        params = [(param[i].copy(), float(rho[i])) for i in range(nf)]
    # the mirror: incrementState_IMUCam, then the feature loop on the incremented clones' camera poses
    ref, applied = mirror.increment_state(st, dx[:leg + 6 * N], f)
    assert applied
    cams = [(ref['R_c2w'][a], ref['t_c_w'][a]) if a < N else (nui_cam[a - N, :9].reshape(3, 3), nui_cam[a - N, 9:]) for a in anchors]
    new_params, p_ws = mz.increment_features(dx, leg + 6 * N, idp, params, cams)
    # the host layer
    cR, ct = np.ascontiguousarray(st['R_b2w']).copy(), np.ascontiguousarray(st['t_b_w']).copy()
    imu = np.concatenate([st['R_b2w_imu'].ravel(), st['v'], st['p'], st['bg'], st['ba'], st['R_b2c'].ravel(), st['t_c_b']]).copy()
    cam, pos = np.zeros((N, 12)), np.zeros((nf, 3))
    par, rh = np.ascontiguousarray(param).copy(), rho.copy()
    rc = shim.orc_test_zupt_increment(leg, f.use_larvio, f.use_left_perturbation, 0, N, _d(cR), _d(ct), _d(imu), _d(dx), n, idp, nf,
                                      anchors.ctypes.data_as(C.POINTER(C.c_int32)), _d(nui_cam), nui, _d(par), _d(rh), _d(cam), _d(pos))
    assert rc == 1
    tol = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-12 * max(np.abs(np.asarray(b)).max(), 1.0)
    assert tol(cR, ref['R_b2w']) and tol(ct, ref['t_b_w'])
    assert tol(cam[:, :9].reshape(N, 3, 3), ref['R_c2w']) and tol(cam[:, 9:], ref['t_c_w'])
    assert tol(imu[9:12], ref['v']) and tol(imu[12:15], ref['p']) and tol(imu[:9].reshape(3, 3), ref['R_b2w_imu'])
    if idp == 3:
        assert tol(par, np.array(new_params))
        assert np.abs(par - param).max() > 1e-4   # (the increment moved them)
    else:
        assert tol(rh, np.array([p[1] for p in new_params])) and np.array_equal(par, param)
    assert tol(pos, p_ws)


def test_feature_loop_runs_when_the_large_update_is_discarded(shim):
    """incrementState_IMUCam returns early on a large dx (src/orcvio.cpp:4479-4494); the feature loop behind it (:3391-3428) runs all the same"""
    N, nf, leg = 3, 2, 22
    w = synth.make_window(N=N, F=2, seed=4, track_len=2)
    n = leg + 6 * N + nf
    dx = np.zeros(n)
    dx[3] = 1.5
    dx[leg + 6 * N:] = [0.01, -0.02]
    cR, ct = w.R_b2w.copy(), w.t_b_w.copy()
    imu = np.concatenate([np.eye(3).ravel(), np.zeros(12), w.R_b2c[0].ravel(), w.t_c_b[0]]).copy()
    anchors = np.array([0, 2], dtype=np.int32)
    par = np.array([[0.1, 0.2, 1.0], [-0.1, 0.05, 1.0]])
    rho = np.array([0.2, 0.25])
    cam, pos, nui_cam = np.zeros((N, 12)), np.zeros((nf, 3)), np.zeros((1, 12))
    rc = shim.orc_test_zupt_increment(leg, 1, 0, 1, N, _d(cR), _d(ct), _d(imu), _d(dx), n, 1, nf, anchors.ctypes.data_as(C.POINTER(C.c_int32)),
                                      _d(nui_cam), 0, _d(par), _d(rho), _d(cam), _d(pos))
    assert rc == 0
    assert np.array_equal(ct, w.t_b_w) and imu[9] == 0.0
    assert np.allclose(rho, [0.21, 0.23], rtol=0, atol=1e-15)


def test_make_zupt_stream_is_a_consistent_stream():
    fl = synth.Flags(use_larvio=1)
    frames, P0 = synth.make_zupt_stream(fl, n_frames=30)
    n = P0.shape[0]
    still = 0
    for fr in frames:
        if fr['zupt'] is None:
            assert fr['w'].n == n + 6
            n = fr['w'].n - 6 * len(fr['remove'])
        else:
            still += 1
            assert fr['w'] is None and fr['zupt']['r'].shape == (9,) and fl.leg_dim + 6 * fr['zupt']['n_clones'] + 12 == n + 6
            assert np.abs(fr['Phi'] - np.eye(fl.leg_dim)).max() < 1e-4 and np.abs(fr['Q']).max() < 1e-8
    assert 10 <= still <= 20
