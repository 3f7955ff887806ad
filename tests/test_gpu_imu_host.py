"""GPU test of the C++ host layer's MsckfBackend::processImu as a filter calls it (through tests/cpp/imu_shim.cpp: a backend of its own,
the covariance made resident, the buffered IMU messages processed, the covariance fetched back) against tests/mirror_imu.py: the
propagated state and FEJ copy, the carried measurement, the messages erased from the buffer, the resident covariance.  Bars as in
tests/test_gpu_imu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from orcvio_amd import capi
import imu_cases as ic
import mirror_imu as mi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


@pytest.fixture(scope='module')
def shim(built):
    capi.load()
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'cpp', 'libimushim.so'))
    lib.orc_test_process_imu.argtypes = [_dp, _dp, _dp, _dp, C.c_int, C.c_double, C.c_int, _dp, C.c_int, _ip, _dp, _dp]
    lib.orc_test_process_imu.restype = C.c_int
    return lib


def _d(a):
    return a.ctypes.data_as(_dp)


def run(shim, case, wait):
    c, st, fej = case['cfg'], case['state'], case['fej']
    cfg = np.array([c.use_larvio, c.use_left, c.use_closed_form, c.if_fej, *c.gravity, c.imu_img_time_th, *np.diag(c.Qc)], dtype=np.float64)
    imu = np.concatenate([[st.time], st.R.ravel(), st.v, st.p, st.bg, st.ba, fej.v, fej.p]).astype(np.float64)
    prev = case['prev'].copy()
    msgs = np.ascontiguousarray(case['samples'])
    P = np.ascontiguousarray(case['P']).copy()
    outcome = np.full(4, -1, dtype=np.int32)
    info, left_t = np.zeros(4), np.zeros(1)
    rc = shim.orc_test_process_imu(_d(cfg), _d(imu), _d(prev), _d(msgs), msgs.shape[0], float(case['time_bound']), int(wait), _d(P), P.shape[0],
                                   outcome.ctypes.data_as(_ip), _d(info), _d(left_t))
    assert rc == 0, rc
    return dict(imu=imu, prev=prev, P=P, outcome=outcome, info=info, left_t=float(left_t[0]))


@pytest.mark.parametrize('fs,S,n,wait', [('larvio_fej', 10, 145, False), ('right_closed', 33, 28, True)])
def test_process_imu_of_the_host_layer_equals_the_mirror(shim, fs, S, n, wait):
    case = ic.make_case(fs, S, n=n, seed=41, rate=ic.rate_for(S), skipped=2, beyond=3)
    srv, info = ic.run_mirror(case)
    got = run(shim, case, wait)
    assert list(got['outcome']) == [0, S + 2, S, 3]   # (the three messages behind the cut stay in the buffer)
    assert got['left_t'] == case['samples'][S + 2, 0]
    assert got['info'][0] == info['dt']
    np.testing.assert_allclose(got['info'][1:], info['mean_sforce'], rtol=1e-15)
    assert got['imu'][0] == srv.imu.time
    assert np.array_equal(got['imu'][1:16], np.concatenate([srv.imu.R.ravel(), srv.imu.v, srv.imu.p]))   # (bit for bit, as tests/test_gpu_imu.py)
    assert np.array_equal(got['imu'][22:25], got['imu'][10:13]) and np.array_equal(got['imu'][25:28], got['imu'][13:16])   # FEJ_now = imu_state
    assert np.array_equal(got['prev'], case['samples'][S + 1, 1:7])
    Phi, Q = mi.accumulate_sequential(srv.steps)
    e_p = ic.block_error(got['P'], mi.apply_once(case['P'], Phi, 0.5 * (Q + Q.T)))
    hard = float(np.linalg.norm(got['P'] - srv.P) / np.linalg.norm(srv.P))
    print('%s S=%d n=%d: P blocks %.2e (bar %.1e), against the per-sample application %.2e' % (fs, S, n, e_p, ic.REGRESSION_BAR, hard))
    assert hard < 1e-6 and e_p <= ic.REGRESSION_BAR


def test_process_imu_reports_a_refused_phi_and_keeps_the_covariance(shim):
    case = ic.make_case('right_closed', 4, n=28, seed=42)
    case['samples'][1, 1:4] = case['state'].bg
    srv, info = ic.run_mirror(case)
    got = run(shim, case, True)
    assert list(got['outcome']) == [6, 4, 4, 0]   # ORCVIO_ERR_NOT_SPD: the covariance was not propagated, the mean was
    assert np.array_equal(got['P'], case['P'])
    assert got['imu'][0] == srv.imu.time and np.array_equal(got['prev'], case['samples'][3, 1:7])
