"""GPU test of the C++ host layer's MsckfBackend::zuptFrame -- the stationary frame of a hybrid filter in one call -- as a filter calls
it (through tests/cpp/test_host_zupt_hybrid.cpp: a backend of its own, the covariance made resident, the frame, the covariance fetched
back) against tests/zupt_hybrid_cases.py: P and dx, the reference's bookkeeping of the in-state features (src/orcvio.cpp:3108-3114:
flags cleared, feature_states empty, their parameters untouched) and the increment on dx[0:b].

Shapes: tests/test_gpu_zupt_host.py's state (N = 5, leg 22, four in-state features, 1-d and 3-d), with and without propagation and the
resident factor.  Tolerances: that test's."""
import ctypes as C
import os

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror
import lifecycle_cases as lc
import mirror_zupt as mz
import imu_cases as ic
import zupt_hybrid_cases as zh
from test_gpu_zupt_host import _case, _close, N, NF, LEG
from test_gpu_zupt_hybrid import _chk, _imu_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISES = synth.ZUPT_NOISES
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


@pytest.fixture(scope='module')
def shim(built):
    capi.load()
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'cpp', 'libzupthybridshim.so'))
    lib.orc_test_zupt_frame_hybrid.argtypes = ([C.c_int] * 4 + [_dp, _dp, _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp,
                                                              C.c_int, C.c_int, C.c_int, _dp, _ip, _dp, _ip, _ip, _ip,
                                                              C.c_void_p, C.c_void_p, _dp, _dp, C.c_int, C.c_double, C.c_void_p, _ip, _dp])
    lib.orc_test_zupt_frame_hybrid.restype = C.c_int
    return lib


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _run(shim, f, st, anchors, idp, param, rho, P0, Phi, Q, aug, rm, prefactor, armed=None):
    """armed: (imu case of tests/imu_cases.py, orcvio_msckf_zupt_check) -- MsckfBackend::zuptFrameChecked on a handle armed with it"""
    n0, b = P0.shape[0], LEG + 6 * N
    out = dict(cR=np.ascontiguousarray(st['R_b2w']).copy(), ct=np.ascontiguousarray(st['t_b_w']).copy(),
               imu=np.concatenate([st['R_b2w_imu'].ravel(), st['v'], st['p'], st['bg'], st['ba'], st['R_b2c'].ravel(), st['t_c_b']]).copy(),
               cam=np.zeros((N, 12)), pos=np.zeros((NF, 3)), par=np.ascontiguousarray(param).copy(), rho=rho.copy(),
               P=np.zeros((n0 + 6) * (n0 + 6)), n_after=C.c_int32(-1), dx=np.full(b, np.nan), outcome=np.full(3, -1, dtype=np.int32),
               flags=np.full((NF, 2), -1, dtype=np.int32), nfs=C.c_int32(-1), vi=np.full(4, -1, dtype=np.int32), vd=np.full(3, np.nan))
    nz = np.array(NOISES, dtype=np.float64)
    if armed is None:
        imu = (None, None, None, None, 0, 0.0, None)
    else:
        case, chk = armed
        cfg, state, prev = ic.to_capi(case)
        smp = np.ascontiguousarray(case['samples'], dtype=np.float64)
        imu = (C.cast(C.byref(cfg), C.c_void_p), C.cast(C.byref(state), C.c_void_p), _d(prev), _d(smp), smp.shape[0], float(case['time_bound']),
               C.cast(C.byref(chk), C.c_void_p))
    rc = shim.orc_test_zupt_frame_hybrid(LEG, f.use_larvio, f.use_left_perturbation, N, _d(out['cR']), _d(out['ct']), _d(out['imu']), idp, NF,
                                         anchors.ctypes.data_as(_ip), _d(out['par']), _d(out['rho']), _d(out['cam']), _d(out['pos']),
                                         _d(np.ascontiguousarray(P0)), n0, _d(nz), _d(Phi), _d(Q), int(aug), int(rm), int(prefactor), _d(out['P']),
                                         C.byref(out['n_after']), _d(out['dx']), out['outcome'].ctypes.data_as(_ip),
                                         out['flags'].ctypes.data_as(_ip), C.byref(out['nfs']), *imu, out['vi'].ctypes.data_as(_ip), _d(out['vd']))
    assert rc == 0, rc
    m = out['n_after'].value
    out['P'] = out['P'][:m * m].reshape(m, m).copy()
    return out


@pytest.mark.parametrize('idp,prop,aug,rm,prefactor,flags', [(1, 0, 1, 1, True, dict(use_larvio=1)), (3, 1, 1, 1, False, dict(use_larvio=0, use_left_perturbation=1)),
                                                              (3, 0, 0, 0, True, dict(use_larvio=0, use_left_perturbation=0)), (1, 1, 0, 1, False, dict(use_larvio=1))],
                         ids=['1d-factor', '3d-propagated-left', '3d-update-only-right', '1d-propagated'])
def test_zupt_frame_of_the_host_layer_equals_the_restatement(shim, idp, prop, aug, rm, prefactor, flags):
    f = synth.Flags(**flags)
    st, anchors, _, param, rho, _ = _case(idp, 0, 30 + idp + 2 * prop)
    b = LEG + 6 * N
    n0 = b - 6 * aug + idp * NF
    P0 = lc.spd(n0, 50 + n0)
    Phi, Q = zh.frame_inputs(LEG, n0) if prop else (None, None)
    got = _run(shim, f, st, anchors, idp, param, rho, P0, Phi, Q, aug, rm, prefactor)
    r = mz.residual(st['v'], st['R_b2w'][N - 2], st['t_b_w'][N - 2], st['R_b2w'][N - 1], st['t_b_w'][N - 1])
    ref = zh.hybrid_frame(P0, LEG, N, idp, NF, r, NOISES, Phi, Q, bool(aug), bool(rm))
    assert list(got['outcome']) == [0, 1, 1]
    zh.check_frame(dict(dx=got['dx'], P=got['P'], n_after=got['n_after'].value, applied=1), ref)
    # the reference's bookkeeping: every in-state feature has left the state, its parameters are not incremented
    assert got['nfs'].value == 0 and not got['flags'].any()
    assert np.array_equal(got['par'], param) and np.array_equal(got['rho'], rho) and not got['pos'].any()
    # the increment on dx[0:b]
    assert np.abs(ref['dx']).max() < 0.1
    inc, applied = mirror.increment_state(st, ref['dx'], f)
    assert applied
    _close(got['cR'], inc['R_b2w'], 'clone R', 1.0)
    _close(got['ct'], inc['t_b_w'], 'clone t', 1.0)
    _close(got['imu'][:9].reshape(3, 3), inc['R_b2w_imu'], 'imu R', 1.0)
    _close(got['imu'][9:12], inc['v'], 'v', 1.0)
    _close(got['imu'][12:15], inc['p'], 'p', 1.0)
    assert np.abs(got['imu'][9:12] - st['v']).max() > 1e-4   # (the update moved the velocity towards zero)


def test_zupt_frame_of_the_host_layer_returns_a_refusal_with_every_feature_in_place(shim):
    f = synth.Flags(use_larvio=1)
    st, anchors, _, param, rho, _ = _case(1, 0, 6)
    n0 = LEG + 6 * N + NF
    P0 = lc.spd(n0, 78)
    P0[3:6, 3:6] = -np.eye(3)
    got = _run(shim, f, st, anchors, 1, param, rho, P0, None, None, 0, 1, False)
    assert list(got['outcome']) == [6, 0, 0] and got['n_after'].value == n0
    assert not got['dx'].any() and np.array_equal(got['P'], P0)
    assert got['nfs'].value == NF and (got['flags'] == 1).all()
    assert np.array_equal(got['cR'], st['R_b2w']) and np.array_equal(got['imu'][9:12], st['v']) and np.array_equal(got['rho'], rho)


def _python_checked(case, idp, P0, r):
    """the same checked frame through the ctypes binding on a handle of its own: (frame dict, verdict dict, P behind it)"""
    u = capi.MsckfUpdater(device=0, max_clones=40, max_features=64, max_observations=1024)   # (the product library, as the shim's backend)
    try:
        u.set_extra_states(idp * NF)
        u.cov_set(P0)
        cfg, state, prev = ic.to_capi(case)
        u.io_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])
        g, v = u.cov_zupt_frame_checked_hybrid(_chk(case), LEG, N, r, NOISES, idp, NF, True, True)
        return g, v, u.cov_get()
    finally:
        u.close()


@pytest.mark.parametrize('idp,resid,accept', [(1, 0.1, 1), (3, 30.0, 0)], ids=['1d-accepted', '3d-rejected'])
def test_checked_zupt_frame_of_the_host_layer(shim, idp, resid, accept):
    """MsckfBackend::zuptFrameChecked on an armed handle: the verdict it copies, and behind an acceptance the bookkeeping and the
    increment, behind a rejection nothing -- P, dx and the verdict bit for bit those of the binding's call on a handle of its own."""
    f = synth.Flags(use_larvio=1)
    st, anchors, _, param, rho, _ = _case(idp, 0, 40 + idp)
    n0 = LEG + 6 * (N - 1) + idp * NF
    P0 = ic.make_cov(n0, np.random.default_rng(n0))
    case = _imu_case(resid, seed=65 + idp)
    got = _run(shim, f, st, anchors, idp, param, rho, P0, None, None, 1, 1, False, armed=(case, _chk(case)))
    r = mz.residual(st['v'], st['R_b2w'][N - 2], st['t_b_w'][N - 2], st['R_b2w'][N - 1], st['t_b_w'][N - 1])
    g, v, P = _python_checked(case, idp, P0, r)
    assert (v['evaluated'], v['accept']) == (1, accept), v
    assert list(got['vi']) == [v['status'], v['evaluated'], v['accept'], v['dof']]
    assert list(got['vd']) == [v['chi2'], v['chi2_check'], v['speed']]
    assert np.array_equal(got['dx'], g['dx']) and np.array_equal(got['P'], P) and got['n_after'].value == g['n_after']
    if accept:
        assert list(got['outcome']) == [0, 1, 1] and g['applied'] == 1 and got['n_after'].value == LEG + 6 * (N - 1)
        assert got['nfs'].value == 0 and not got['flags'].any()
        assert np.array_equal(got['par'], param) and np.array_equal(got['rho'], rho)
        inc, applied = mirror.increment_state(st, g['dx'], f)
        assert applied
        _close(got['cR'], inc['R_b2w'], 'clone R', 1.0)
        _close(got['imu'][9:12], inc['v'], 'v', 1.0)
    else:
        assert list(got['outcome']) == [0, 0, 0] and g['applied'] == 0 and got['n_after'].value == n0 + 6 and not got['dx'].any()
        assert got['nfs'].value == NF and (got['flags'] == 1).all()
        assert np.array_equal(got['cR'], st['R_b2w']) and np.array_equal(got['imu'][9:12], st['v']) and np.array_equal(got['rho'], rho)
