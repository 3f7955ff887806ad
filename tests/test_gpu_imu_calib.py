"""orcvio_msckf_cov_propagate_imu_calib on the GPU (leg_dim 46: the 24 IMU intrinsics in the state) against the numpy restatement of
the reference's IMU step at 46 (tests/mirror_imu_calib.py): the accumulated Phi, Q of k_imu_phi_q46 and the resident covariance behind
the propagation, block by block; their exact structure; identity intrinsics against the leg_dim 22 call; the refusal of a non-finite
Phi; the documented error codes; determinism; one frame at 46 by both routes."""
import ctypes as C

import numpy as np
import pytest

from orcvio_amd import capi, synth
import imu_cases as ic
import imu_calib_cases as icc
import mirror_imu_calib as mc

pytestmark = pytest.mark.gpu

HARD_BAR = 1e-6                          # the project's parity bar: relative Frobenius on P, against the reference's per-sample application
REGRESSION_BAR = icc.REGRESSION_BAR_46   # ten times the mirror's own spread between two accumulation orders (tests/test_imu_calib_mirror.py)
LEFT_CLOSED = ('larvio', 'larvio_fej', 'left_closed')


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=21, max_features=16, max_observations=256)
    u.set_extra_states(3)
    yield u
    u.close()


def rel_fro(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


_mirror_cache = {}


def mirror_of(key):
    """the mirror's results for a comparison case, computed once"""
    if key not in _mirror_cache:
        case = icc.gpu_case(*key)
        srv, info = icc.run_mirror(case)
        Phi, Q = mc.accumulate_sequential(srv.steps)
        _mirror_cache[key] = (case, srv, info, Phi, 0.5 * (Q + Q.T))
    return _mirror_cache[key]


def assert_structure(Phi, Q, fs):
    """(d) of tests/test_imu_calib_mirror.py on the device's pair, exactly"""
    assert np.array_equal(Phi[15:, :], np.eye(46)[15:, :]) and not Phi[:15, 15:22].any()
    Qo = Q.copy()
    Qo[:15, :15] = 0.0
    assert not Qo.any()
    if fs not in LEFT_CLOSED:
        assert not Phi[:15, 22:].any()
    assert np.array_equal(Q, Q.T)


@pytest.mark.parametrize('fs,S,n,intr', icc.gpu_cases())
def test_phi_q_and_covariance_against_the_mirror(upd, fs, S, n, intr):
    case, srv, info, Phi, Q = mirror_of((fs, S, n, intr))
    cfg, xi, state, prev = icc.to_capi(case)
    upd.cov_set(case['P'])
    got = upd.cov_propagate_imu_calib(cfg, xi, state, prev, case['samples'], case['time_bound'], want_PhiQ=True)
    P = upd.cov_get()
    assert (got['n_used'], got['n_propagated'], got['dt'], got['applied']) == (info['n_used'], S, info['dt'], 1)
    e_phi, e_q = icc.block_error(got['Phi'], Phi), icc.block_error(got['Q'], Q)
    e_p = icc.block_error(P, mc.apply_once(case['P'], Phi, Q))
    hard = rel_fro(P, srv.P)
    print('%s %s S=%d n=%d: Phi %.2e Q %.2e P %.2e (blocks, bar %.1e); P against the per-sample application %.2e' % (fs, intr, S, n, e_phi, e_q, e_p, REGRESSION_BAR, hard))
    assert hard < HARD_BAR
    assert e_phi <= REGRESSION_BAR and e_q <= REGRESSION_BAR and e_p <= REGRESSION_BAR
    assert np.array_equal(P, P.T)
    assert_structure(got['Phi'], got['Q'], fs)
    # the host half, bit for bit (as tests/test_gpu_imu.py: the bar above rests on it)
    assert state.time == srv.imu.time
    for name, ref in (('R_b2w', srv.imu.R.ravel()), ('v', srv.imu.v), ('p', srv.imu.p), ('v_fej', srv.fej_now.v), ('p_fej', srv.fej_now.p)):
        assert np.array_equal(np.array(getattr(state, name)[:]), ref), name
    assert np.array_equal(prev, np.concatenate([srv.m_gyro_old, srv.m_acc_old]))
    np.testing.assert_allclose(got['mean_sforce'], info['mean_sforce'], rtol=1e-15)


@pytest.mark.parametrize('fs,S', [('larvio', 33), ('right_closed', 9), ('left_euler', 128)])
def test_identity_intrinsics_agree_with_the_leg_dim_22_call(upd, fs, S):
    """The leading 22 x 22 of Phi, Q against orcvio_msckf_cov_propagate_imu on the same samples, within the 22 call's regression bar.
    Whether they are bit for bit the same is printed (the two kernels run the same recursion on the leading block; the left closed
    form's bias blocks go through products with Tg = Ma = I and TA = 0 at 46)."""
    case = icc.gpu_case(fs, S, 52, 'identity')
    cfg, xi, state, prev = icc.to_capi(case)
    upd.cov_set(case['P'])
    g46 = upd.cov_propagate_imu_calib(cfg, xi, state, prev, case['samples'], case['time_bound'], want_PhiQ=True)
    cfg22, state22, prev22 = ic.to_capi(case)
    upd.cov_set(case['P'][:28, :28])
    g22 = upd.cov_propagate_imu(cfg22, state22, prev22, case['samples'], case['time_bound'], want_PhiQ=True)
    e_phi, e_q = ic.block_error(g46['Phi'][:22, :22], g22['Phi']), ic.block_error(g46['Q'][:22, :22], g22['Q'])
    same = np.array_equal(g46['Phi'][:22, :22], g22['Phi']) and np.array_equal(g46['Q'][:22, :22], g22['Q'])
    print('%s S=%d identity intrinsics against leg_dim 22: Phi %.2e Q %.2e, bit for bit: %s' % (fs, S, e_phi, e_q, same))
    assert e_phi <= ic.REGRESSION_BAR and e_q <= ic.REGRESSION_BAR
    assert np.array_equal(np.array(state.p[:]), np.array(state22.p[:])) and np.array_equal(np.array(state.R_b2w[:]), np.array(state22.R_b2w[:]))


def test_a_zero_gyro_in_the_right_closed_form_is_refused_and_the_handle_stays_usable(upd):
    """A status word, not a fault.  With general intrinsics the unbiased gyro is Tg (m_gyro - As acc - b_g): the sample's m_gyro is set
    to As acc + b_g, so w = 0 and gyro = Tg 0 = 0 exactly, and the right closed form divides by |gyro|^2."""
    case = icc.make_case('right_closed', 5, intr='general', n=52, seed=9)
    Tg, As, Ma = mc.intrinsic_matrices(case['intr'])
    f = case['samples'][2, 4:7] - case['state'].ba
    acc = mc.mv(Ma, f)
    t = mc.mv(As, acc)
    m_gyro = t + case['state'].bg
    case['state'].bg = m_gyro - t   # (the bias as the rounded sum holds it: w is formed as (m_gyro - As acc) - b_g, and is zero exactly)
    case['fej'].bg = case['state'].bg.copy()
    assert np.array_equal(m_gyro - t - case['state'].bg, np.zeros(3))
    case['samples'][2, 1:4] = m_gyro
    cfg, xi, state, prev = icc.to_capi(case)
    upd.cov_set(case['P'])
    got = upd.cov_propagate_imu_calib(cfg, xi, state, prev, case['samples'], case['time_bound'], want_PhiQ=True, raise_on_refusal=False)
    assert got['status'] == 6 and got['applied'] == 0   # ORCVIO_ERR_NOT_SPD
    assert not np.isfinite(got['Phi']).all()
    assert np.array_equal(upd.cov_get(), case['P'])
    # a good call behind it
    good, srv, info, Phi, Q = mirror_of(('right_closed', 5, 52, 'general'))
    cfg, xi, state, prev = icc.to_capi(good)
    upd.cov_set(good['P'])
    got = upd.cov_propagate_imu_calib(cfg, xi, state, prev, good['samples'], good['time_bound'], want_PhiQ=True)
    assert got['status'] == 0 and got['applied'] == 1
    assert icc.block_error(got['Phi'], Phi) <= REGRESSION_BAR and icc.block_error(upd.cov_get(), mc.apply_once(good['P'], Phi, Q)) <= REGRESSION_BAR


def test_documented_error_codes_leave_everything_as_it_was(upd):
    case = icc.make_case('larvio', 129, n=52, seed=4, rate=650.0)
    cfg, xi, state, prev = icc.to_capi(case)
    upd.cov_set(case['P'])

    def untouched():
        return state.time == case['state'].time and np.array_equal(np.array(state.p[:]), case['state'].p) and \
            np.array_equal(prev, case['prev']) and np.array_equal(upd.cov_get(), case['P'])
    with pytest.raises(capi.MsckfError) as e:
        upd.cov_propagate_imu_calib(cfg, xi, state, prev, case['samples'], case['time_bound'], wait=True)
    assert e.value.code == 3 and untouched()   # ORCVIO_ERR_CAPACITY: 129 samples selected
    smp = np.ascontiguousarray(case['samples'][:3])
    tb = float(smp[2, 0])
    cfg22 = capi.MsckfUpdater.imu_config(22)
    with pytest.raises(capi.MsckfError) as e:
        upd.cov_propagate_imu_calib(cfg22, xi, state, prev, smp, tb)
    assert e.value.code == 1 and untouched()   # leg_dim 22: the plain call serves it
    bad = capi.MsckfUpdater.imu_intrinsics(case['intr'])
    bad.x[17] = float('nan')
    with pytest.raises(capi.MsckfError) as e:
        upd.cov_propagate_imu_calib(cfg, bad, state, prev, smp, tb)
    assert e.value.code == 1 and untouched()
    lib = upd.lib
    info = capi.ImuInfo()
    args = [upd.h, C.byref(cfg), C.byref(xi), C.byref(state), capi._d(prev), capi._d(smp), 3, tb, C.byref(info), None, None]
    for k in (0, 1, 2, 3, 4, 5, 8):   # every null pointer (intr = NULL is k = 2)
        a = list(args)
        a[k] = None
        assert lib.orcvio_msckf_cov_propagate_imu_calib(*a) == 1, k
    Phi = np.zeros((46, 46))
    a = list(args)
    a[9] = capi._d(Phi)   # Phi_out without Q_out
    assert lib.orcvio_msckf_cov_propagate_imu_calib(*a) == 1
    assert untouched()
    # a resident covariance of fewer than 46 states
    small = ic.make_cov(28, np.random.default_rng(3))
    upd.cov_set(small)
    with pytest.raises(capi.MsckfError) as e:
        upd.cov_propagate_imu_calib(cfg, xi, state, prev, smp, tb)
    assert e.value.code == 1 and np.array_equal(upd.cov_get(), small) and state.time == case['state'].time and np.array_equal(prev, case['prev'])
    # an empty selection: nothing launched, Phi = I, Q = 0
    upd.cov_set(case['P'])
    none = icc.make_case('larvio', 0, n=52, seed=8, skipped=3)
    cfg, xi, state, prev = icc.to_capi(none)
    got = upd.cov_propagate_imu_calib(cfg, xi, state, prev, none['samples'], none['time_bound'], want_PhiQ=True)
    assert (got['n_used'], got['n_propagated'], got['dt'], got['applied']) == (3, 0, 0.0, 0)
    assert np.array_equal(upd.cov_get(), case['P']) and np.array_equal(got['Phi'], np.eye(46)) and not got['Q'].any()


def test_the_same_input_twice_gives_the_same_bits(upd):
    for key in (('larvio', 33, 166, 'general'), ('right_closed', 127, 52, 'general')):
        case = icc.gpu_case(*key)
        out = []
        for _ in range(2):
            cfg, xi, state, prev = icc.to_capi(case)
            upd.cov_set(case['P'])
            got = upd.cov_propagate_imu_calib(cfg, xi, state, prev, case['samples'], case['time_bound'], want_PhiQ=True)
            out.append((got['Phi'], got['Q'], upd.cov_get()))
        for a, b in zip(out[0], out[1]):
            assert np.array_equal(a, b)


def test_one_frame_at_46_by_both_routes(built):
    """A window of four clones with four tracks on a resident covariance of three (n = 64).  Route 1: cov_propagate_imu_calib without
    a wait, then io_step_frame with Phi = NULL.  Route 2, on a second handle: io_step_frame given that call's Phi_out / Q_out.
    dx and P bit for bit."""
    fl = synth.Flags(use_larvio=1, leg_dim=46)
    w = synth.make_window(N=4, F=4, seed=3, track_len=(3, 4), flags=fl)
    P0 = np.ascontiguousarray(synth.make_window(N=3, F=1, seed=5, flags=fl).P)
    assert P0.shape[0] == 64
    case = icc.make_case('larvio', 10, intr='general', n=64, seed=51, rate=200.0, skipped=1, beyond=2)
    hs = [capi.MsckfUpdater(device=0, max_clones=8, max_features=64, max_observations=1024) for _ in range(3)]
    aux, a, b = hs
    try:
        cfg, xi, state, prev = icc.to_capi(case)
        aux.cov_set(P0)
        pq = aux.cov_propagate_imu_calib(cfg, xi, state, prev, case['samples'], case['time_bound'], want_PhiQ=True)
        a.cov_set(P0); b.cov_set(P0)
        cfg, xi, state, prev = icc.to_capi(case)
        got = a.cov_propagate_imu_calib(cfg, xi, state, prev, case['samples'], case['time_bound'])   # (no wait)
        assert got['applied'] == 1 and got['Phi'] is None
        ga = a.io_step_frame(w, None, None, True)
        gb = b.io_step_frame(w, pq['Phi'], pq['Q'], True)
        assert gb['status_first'] == 0 and gb['stats'][3] == 1
        assert np.array_equal(ga['dx'], gb['dx']) and ga['n_after'] == gb['n_after'] == 70
        assert np.array_equal(a.cov_get(), b.cov_get())
    finally:
        for u in hs:
            u.close()
