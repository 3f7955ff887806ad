"""GPU test of the C++ host layer's MsckfBackend::zuptUpdate as a filter calls it (through tests/cpp/zupt_shim.cpp: a backend of its own,
the covariance made resident, the options declared, the update, the covariance fetched back) against tests/mirror_zupt.py: the residual
it forms from the two newest clones, dx, P+, the IMU / clone increments and the in-state features' parameters and positions.

Shapes: N = 5, leg 22, four in-state features (1-d: n = 56, 3-d: n = 64, with one nuisance block 62 / 70) -- two tiles of the
covariance kernel, with and without the resident factor.  Tolerances: 1e-12 max|.| for P+ and dx as in tests/test_gpu_zupt.py; the state
is ref + dx with |dx| << 1, so 1e-12 max(|ref|, 1) holds it to the same bar."""
import ctypes as C
import os

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror
import lifecycle_cases as lc
import mirror_zupt as mz

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISES = synth.ZUPT_NOISES
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
N, NF, LEG = 5, 4, 22


@pytest.fixture(scope='module')
def shim(built):
    capi.load()
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'cpp', 'libzuptshim.so'))
    lib.orc_test_zupt_update.argtypes = ([C.c_int] * 5 + [_dp, _dp, _dp, C.c_int, C.c_int, _ip, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp,
                                                        C.c_int, _dp, _ip])
    lib.orc_test_zupt_update.restype = C.c_int
    return lib


def _d(a):
    return a.ctypes.data_as(_dp)


def _case(idp, nui, seed):
    """a window whose two newest clones are a stationary pair (a millimetre and a milliradian apart), a small velocity, four features"""
    rng = np.random.default_rng(seed)
    w = synth.make_window(N=N, F=2, seed=3, track_len=3)
    R_b2w, t_b_w = w.R_b2w.copy(), w.t_b_w.copy()
    R_b2w[N - 1] = R_b2w[N - 2] @ synth.so3_exp(1e-3 * rng.standard_normal(3))
    t_b_w[N - 1] = t_b_w[N - 2] + 1e-3 * rng.standard_normal(3)
    st = dict(R_b2w_imu=R_b2w[-1].copy(), v=rng.standard_normal(3) * 1e-2, p=t_b_w[-1].copy(), bg=rng.standard_normal(3) * 1e-2,
              ba=rng.standard_normal(3) * 1e-2, R_b2c=w.R_b2c[0].copy(), t_c_b=w.t_c_b[0].copy(), td=np.float64(0.0), R_b2w=R_b2w, t_b_w=t_b_w)
    anchors = np.array([0, N - 1, 2, N if nui else 1], dtype=np.int32)   # (the last one at the nuisance state when there is one)
    nui_cam = np.concatenate([synth.so3_exp(rng.standard_normal(3)).ravel(), rng.standard_normal(3)])[None, :].repeat(max(nui, 1), 0).copy()
    if idp == 3:
        param = np.stack([rng.uniform(-0.3, 0.3, NF), rng.uniform(-0.3, 0.3, NF), rng.uniform(0.1, 0.3, NF)], axis=1)
        rho = np.zeros(NF)
        params = [p.copy() for p in param]
    else:
        param = np.stack([rng.uniform(-0.3, 0.3, NF), rng.uniform(-0.3, 0.3, NF), np.ones(NF)], axis=1)
        rho = rng.uniform(0.1, 0.3, NF)
        params = [(param[i].copy(), float(rho[i])) for i in range(NF)]
    return st, anchors, nui_cam, param, rho, params


def _run(shim, f, st, anchors, nui_cam, nui, idp, param, rho, P, prefactor, discard_large=0):
    n = P.shape[0]
    out = dict(cR=np.ascontiguousarray(st['R_b2w']).copy(), ct=np.ascontiguousarray(st['t_b_w']).copy(),
               imu=np.concatenate([st['R_b2w_imu'].ravel(), st['v'], st['p'], st['bg'], st['ba'], st['R_b2c'].ravel(), st['t_c_b']]).copy(),
               cam=np.zeros((N, 12)), pos=np.zeros((NF, 3)), par=np.ascontiguousarray(param).copy(), rho=rho.copy(),
               P=np.ascontiguousarray(P).copy(), dx=np.full(n, np.nan), outcome=np.full(3, -1, dtype=np.int32))
    nz = np.array(NOISES, dtype=np.float64)
    rc = shim.orc_test_zupt_update(LEG, f.use_larvio, f.use_left_perturbation, discard_large, N, _d(out['cR']), _d(out['ct']), _d(out['imu']), idp, NF,
                                   anchors.ctypes.data_as(_ip), _d(nui_cam), nui, _d(out['par']), _d(out['rho']), _d(out['cam']), _d(out['pos']),
                                   _d(out['P']), n, _d(nz), int(prefactor), _d(out['dx']), out['outcome'].ctypes.data_as(_ip))
    assert rc == 0, rc
    return out


def _close(got, ref, what, floor=0.0):
    err, top = np.abs(np.asarray(got) - np.asarray(ref)).max(), max(np.abs(np.asarray(ref)).max(), floor)
    print(f'{what}: max err {err:.3e}, scale {top:.3e}, ratio {err / top:.3e}')
    assert err <= 1e-12 * top, (what, err, top)


@pytest.mark.parametrize('idp,nui,prefactor,flags', [(1, 0, True, dict(use_larvio=1)), (3, 0, True, dict(use_larvio=0, use_left_perturbation=1)),
                                                     (1, 1, False, dict(use_larvio=0, use_left_perturbation=0)), (3, 1, True, dict(use_larvio=1))],
                         ids=['1d-factor', '3d-factor-left', '1d-nuisance-right', '3d-nuisance'])
def test_zupt_update_of_the_host_layer_equals_the_mirror(shim, idp, nui, prefactor, flags):
    f = synth.Flags(**flags)
    st, anchors, nui_cam, param, rho, params = _case(idp, nui, 20 + idp + 10 * nui)
    n = LEG + 6 * N + idp * NF + 6 * nui
    P = lc.spd(n, 40 + n)
    got = _run(shim, f, st, anchors, nui_cam, nui, idp, param, rho, P, prefactor)
    # the mirror: the residual of the two newest clones, the update, incrementState_IMUCam, the feature loop
    r = mz.residual(st['v'], st['R_b2w'][N - 2], st['t_b_w'][N - 2], st['R_b2w'][N - 1], st['t_b_w'][N - 1])
    dx, P_ref = mz.measurement_update(P, LEG, N, r, *NOISES, n_nui=nui)
    assert np.abs(dx).max() < 0.1   # (what the state tolerance below rests on)
    ref, applied = mirror.increment_state(st, dx[:LEG + 6 * N], f)
    assert applied
    cams = [(ref['R_c2w'][a], ref['t_c_w'][a]) if a < N else (nui_cam[a - N, :9].reshape(3, 3), nui_cam[a - N, 9:]) for a in anchors]
    new_params, p_ws = mz.increment_features(dx, LEG + 6 * N, idp, params, cams)
    assert list(got['outcome']) == [0, 1, 1]
    _close(got['dx'], dx, 'dx')
    _close(got['P'], P_ref, 'P+')
    assert np.array_equal(got['P'], got['P'].T)
    if nui:
        assert np.array_equal(got['P'][n - 6 * nui:, n - 6 * nui:], P[n - 6 * nui:, n - 6 * nui:])
    _close(got['cR'], ref['R_b2w'], 'clone R', 1.0)
    _close(got['ct'], ref['t_b_w'], 'clone t', 1.0)
    _close(got['cam'][:, :9].reshape(N, 3, 3), ref['R_c2w'], 'camera R', 1.0)
    _close(got['cam'][:, 9:], ref['t_c_w'], 'camera t', 1.0)
    _close(got['imu'][:9].reshape(3, 3), ref['R_b2w_imu'], 'imu R', 1.0)
    _close(got['imu'][9:12], ref['v'], 'v', 1.0)
    _close(got['imu'][12:15], ref['p'], 'p', 1.0)
    _close(got['imu'][15:18], ref['bg'], 'bg', 1.0)
    _close(got['imu'][18:21], ref['ba'], 'ba', 1.0)
    assert np.abs(got['imu'][9:12] - st['v']).max() > 1e-4   # (the update moved the velocity towards zero)
    if idp == 3:
        _close(got['par'], np.array(new_params), 'invParam', 1.0)
    else:
        _close(got['rho'], np.array([p[1] for p in new_params]), 'invDepth', 1.0)
        assert np.array_equal(got['par'], param)
    _close(got['pos'], p_ws, 'feature positions', 1.0)


def test_zupt_update_of_the_host_layer_returns_a_refusal_untouched(shim):
    """a prior the update must reject (negative velocity block): NOT_SPD, nothing updated, the state, the features and P as before"""
    f = synth.Flags(use_larvio=1)
    st, anchors, nui_cam, param, rho, _ = _case(1, 0, 5)
    n = LEG + 6 * N + NF
    P = lc.spd(n, 77)
    P[3:6, 3:6] = -np.eye(3)
    got = _run(shim, f, st, anchors, nui_cam, 0, 1, param, rho, P, False)
    assert list(got['outcome']) == [6, 0, 0]
    assert not got['dx'].any() and np.array_equal(got['P'], P)
    assert np.array_equal(got['cR'], st['R_b2w']) and np.array_equal(got['ct'], st['t_b_w']) and np.array_equal(got['imu'][9:12], st['v'])
    assert np.array_equal(got['rho'], rho) and not got['pos'].any()
