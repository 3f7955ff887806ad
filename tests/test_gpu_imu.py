"""orcvio_msckf_cov_propagate_imu on the GPU against the numpy restatement of the reference's IMU step (tests/mirror_imu.py): the
accumulated Phi, Q of k_imu_phi_q and the resident covariance behind the propagation, block by block; sample selection; the refusal of
a non-finite Phi; the documented error codes; determinism."""
import numpy as np
import pytest

from orcvio_amd import capi
import imu_cases as ic
import mirror_imu as mi

pytestmark = pytest.mark.gpu

HARD_BAR = 1e-6                    # the project's parity bar: relative Frobenius on P, against the reference's per-sample application
REGRESSION_BAR = ic.REGRESSION_BAR   # 9.7e-14 = ten times the mirror's own spread between two accumulation orders (9.7e-15, measured by
                                     # tests/test_imu_mirror.py::test_spread_between_two_accumulation_orders on the mirror alone)


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=21, max_features=16, max_observations=256)
    u.set_extra_states(3)
    yield u
    u.close()


to_capi = ic.to_capi


def rel_fro(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


_mirror_cache = {}


def mirror_of(key):
    """the mirror's results for a comparison case, computed once"""
    if key not in _mirror_cache:
        case = ic.gpu_case(*key)
        srv, info = ic.run_mirror(case)
        Phi, Q = mi.accumulate_sequential(srv.steps)
        _mirror_cache[key] = (case, srv, info, Phi, 0.5 * (Q + Q.T))
    return _mirror_cache[key]


@pytest.mark.parametrize('fs,S,n', ic.gpu_cases())
def test_phi_q_and_covariance_against_the_mirror(upd, fs, S, n):
    case, srv, info, Phi, Q = mirror_of((fs, S, n))
    cfg, state, prev = to_capi(case)
    upd.cov_set(case['P'])
    got = upd.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'], want_PhiQ=True)
    P = upd.cov_get()
    assert (got['n_used'], got['n_propagated'], got['dt'], got['applied']) == (info['n_used'], S, info['dt'], 1)
    e_phi, e_q = ic.block_error(got['Phi'], Phi), ic.block_error(got['Q'], Q)
    e_p = ic.block_error(P, mi.apply_once(case['P'], Phi, Q))
    hard = rel_fro(P, srv.P)
    print('%s S=%d n=%d: Phi %.2e Q %.2e P %.2e (blocks, bar %.1e); P against the per-sample application %.2e' % (fs, S, n, e_phi, e_q, e_p, REGRESSION_BAR, hard))
    assert hard < HARD_BAR
    assert e_phi <= REGRESSION_BAR and e_q <= REGRESSION_BAR and e_p <= REGRESSION_BAR
    assert np.array_equal(P, P.T)
    # the host half: state, FEJ pair, the carried measurement.  BIT FOR BIT: the mirror's predictors and the header's run the same IEEE
    # operations in the same order, and the bar above rests on it -- the closed forms subtract nearly equal positions, so one ulp in
    # the propagated p is 1e-13 of a block of Phi (tests/mirror_imu.py)
    assert state.time == srv.imu.time
    for name, ref in (('R_b2w', srv.imu.R.ravel()), ('v', srv.imu.v), ('p', srv.imu.p), ('v_fej', srv.fej_now.v), ('p_fej', srv.fej_now.p)):
        assert np.array_equal(np.array(getattr(state, name)[:]), ref), name
    assert np.array_equal(prev, np.concatenate([srv.m_gyro_old, srv.m_acc_old]))
    np.testing.assert_allclose(got['mean_sforce'], info['mean_sforce'], rtol=1e-15)


def test_selection_skipped_samples_the_cut_and_an_empty_selection(upd):
    # two samples at or before state.time, five processed, three beyond the cut
    case = ic.make_case('larvio', 5, n=28, seed=8, rate=250.0, skipped=2, beyond=3)
    srv, info = ic.run_mirror(case)
    cfg, state, prev = to_capi(case)
    upd.cov_set(case['P'])
    got = upd.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])   # (no wait)
    assert (got['n_used'], got['n_propagated'], got['dt']) == (info['n_used'], info['n_propagated'], info['dt']) == (7, 5, info['dt'])
    assert rel_fro(upd.cov_get(), srv.P) < HARD_BAR
    # every sample skipped: nothing launched, the covariance bit for bit what it was
    case = ic.make_case('larvio', 0, n=28, seed=8, skipped=3)
    cfg, state, prev = to_capi(case)
    upd.cov_set(case['P'])
    got = upd.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'], want_PhiQ=True)
    assert (got['n_used'], got['n_propagated'], got['dt'], got['applied']) == (3, 0, 0.0, 0)
    assert np.array_equal(upd.cov_get(), case['P']) and np.array_equal(got['Phi'], np.eye(22)) and not got['Q'].any()
    assert np.array_equal(prev, case['prev']) and state.time == case['state'].time
    # no samples at all
    got = upd.cov_propagate_imu(cfg, state, prev, np.zeros((0, 7)), case['time_bound'], wait=True)
    assert (got['n_used'], got['n_propagated']) == (0, 0) and np.array_equal(upd.cov_get(), case['P'])


def test_a_zero_gyro_sample_in_the_right_closed_form_is_refused_and_the_handle_stays_usable(upd):
    """A status word, not a fault: Phi is NaN (the reference divides by |gyro|^2), the propagation behind the kernel copies P."""
    case = ic.make_case('right_closed', 5, n=28, seed=9)
    case['samples'][2, 1:4] = case['state'].bg
    cfg, state, prev = to_capi(case)
    upd.cov_set(case['P'])
    got = upd.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'], want_PhiQ=True, raise_on_refusal=False)
    assert got['status'] == 6 and got['applied'] == 0   # ORCVIO_ERR_NOT_SPD
    assert not np.isfinite(got['Phi']).all()
    assert np.array_equal(upd.cov_get(), case['P'])
    # a good call behind it
    key = ('right_closed', 5, 28)
    good, srv, info, Phi, Q = mirror_of(key)
    cfg, state, prev = to_capi(good)
    upd.cov_set(good['P'])
    got = upd.cov_propagate_imu(cfg, state, prev, good['samples'], good['time_bound'], want_PhiQ=True)
    assert got['status'] == 0 and got['applied'] == 1
    assert ic.block_error(got['Phi'], Phi) <= REGRESSION_BAR and ic.block_error(upd.cov_get(), mi.apply_once(good['P'], Phi, Q)) <= REGRESSION_BAR


def test_documented_error_codes_leave_everything_as_it_was(upd):
    case = ic.make_case('larvio', 129, n=28, seed=4, rate=650.0)
    cfg, state, prev = to_capi(case)
    upd.cov_set(case['P'])
    with pytest.raises(capi.MsckfError) as e:
        upd.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'], wait=True)
    assert e.value.code == 3   # ORCVIO_ERR_CAPACITY
    assert state.time == case['state'].time and np.array_equal(prev, case['prev'])
    cfg46 = capi.MsckfUpdater.imu_config(46)
    with pytest.raises(capi.MsckfError) as e:
        upd.cov_propagate_imu(cfg46, state, prev, case['samples'][:3], case['time_bound'])
    assert e.value.code == 1   # ORCVIO_ERR_INVALID
    lib = upd.lib
    info = capi.ImuInfo()
    import ctypes as C
    smp = np.ascontiguousarray(case['samples'][:3])
    args = [upd.h, C.byref(cfg), C.byref(state), capi._d(prev), capi._d(smp), 3, float(case['time_bound']), C.byref(info), None, None]
    for k in (0, 1, 2, 3, 4, 7):
        a = list(args)
        a[k] = None
        assert lib.orcvio_msckf_cov_propagate_imu(*a) == 1, k
    Phi = np.zeros((22, 22))
    a = list(args)
    a[8] = capi._d(Phi)   # Phi_out without Q_out
    assert lib.orcvio_msckf_cov_propagate_imu(*a) == 1
    assert np.array_equal(upd.cov_get(), case['P']) and state.time == case['state'].time


def test_the_same_input_twice_gives_the_same_bits(upd):
    for key in (('larvio', 33, 142), ('right_closed', 127, 28)):
        case = ic.gpu_case(*key)
        out = []
        for _ in range(2):
            cfg, state, prev = to_capi(case)
            upd.cov_set(case['P'])
            got = upd.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'], want_PhiQ=True)
            out.append((got['Phi'], got['Q'], upd.cov_get()))
        for a, b in zip(out[0], out[1]):
            assert np.array_equal(a, b)
