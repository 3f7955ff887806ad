"""The ARMED form of the IMU propagation on the GPU: orcvio_msckf_io_propagate_imu in front of orcvio_msckf_io_step_frame /
_io_step_frame_ex / _cov_zupt_frame given Phi = Q = NULL, against the same frame call given Phi_out / Q_out of the stand-alone
orcvio_msckf_cov_propagate_imu taken on another handle -- bit for bit --, against the mirror chained into oracle/mirror_frame.py, and
its refusals."""
import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror_frame
import imu_cases as ic
import mirror_imu as mi

pytestmark = pytest.mark.gpu
LEG = 22


def _handle(extra=0, ekf=False):
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096)
    if ekf:
        u.set_ekf_rows_mode(True)
    u.set_extra_states(extra)
    return u


@pytest.fixture(scope='module')
def aux(built):
    """a handle of its own for the stand-alone call that yields Phi_out, Q_out"""
    u = capi.MsckfUpdater(device=0, max_clones=2, max_features=16, max_observations=256)
    yield u
    u.close()


def phi_q(aux, case, raise_on_refusal=True):
    cfg, state, prev = ic.to_capi(case)
    aux.cov_set(np.eye(LEG))
    got = aux.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'], want_PhiQ=True, raise_on_refusal=raise_on_refusal)
    return got['Phi'], got['Q']


def arm(u, case):
    cfg, state, prev = ic.to_capi(case)
    info = u.io_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])
    return info, state, prev


def same_frame(ga, gb):
    for k in ('dx', 'gamma', 'accept', 'stats', 'prune_dx', 'prune_gamma', 'prune_accept', 'prune_stats'):
        if gb[k] is None:
            assert ga[k] is None, k
        else:
            assert np.array_equal(ga[k], gb[k], equal_nan=True), k
    for k in ('n_after', 'status_first', 'status_prune', 'repaired', 'rc'):
        assert ga[k] == gb[k], k


def window8(with_prune):
    """an 8-clone window with 6 lost tracks on a 7-clone resident covariance; with_prune: the prune update on the two oldest clones and
    their marginalisation"""
    fl = synth.Flags(use_larvio=1)
    w = synth.make_window(N=8, F=6, seed=3, track_len=(5, 8), flags=fl)
    P0 = np.ascontiguousarray(synth.make_window(N=7, F=1, seed=5, flags=fl).P)
    prune, remove = None, []
    if with_prune:
        prune = synth.subset_tracks(w, [0, 1], min_obs=2)
        assert int(prune.obs_ptr[-1]) > 0
        remove = [0, 1]
    return w, P0, prune, remove


@pytest.mark.parametrize('with_prune', [False, True])
def test_armed_step_frame_equals_the_frame_given_phi_q_bit_for_bit(built, aux, with_prune):
    w, P0, prune, remove = window8(with_prune)
    case = ic.make_case('larvio', 10, n=LEG, seed=51 + with_prune, rate=200.0, skipped=1, beyond=2)
    Phi, Q = phi_q(aux, case)
    a, b = _handle(), _handle()
    try:
        a.cov_set(P0); b.cov_set(P0)
        info, state, prev = arm(a, case)
        assert info['n_propagated'] == 10
        srv, minfo = ic.run_mirror(case, with_P=False)
        assert state.time == srv.imu.time and np.array_equal(np.array(state.p[:]), srv.imu.p)   # (the host half ran when the call returned)
        # armed AND Phi given: refused with nothing done, the arming stands
        with pytest.raises(capi.MsckfError) as e:
            a.io_step_frame(w, Phi, Q, True, None, 1, prune, False, remove)
        assert e.value.code == 1 and np.array_equal(a.cov_get(), P0)
        ga = a.io_step_frame(w, None, None, True, None, 1, prune, False, remove)
        gb = b.io_step_frame(w, Phi, Q, True, None, 1, prune, False, remove)
        assert gb['status_first'] == 0 and gb['stats'][3] == 1 and (prune is None or gb['prune_dx'] is not None)
        same_frame(ga, gb)
        assert np.array_equal(a.cov_get(), b.cov_get())
        # the arming was consumed: the next frame call without Phi does not propagate
        n1 = a.cov_get().shape[0]
        assert n1 == LEG + 6 * (8 - len(remove))
    finally:
        a.close(); b.close()


def test_armed_step_frame_against_the_mirror_chain(built):
    """mirror_imu (Phi, Q accumulated from the samples) chained into oracle/mirror_frame.step_frame: the project's parity bar, 1e-6
    relative Frobenius, on dx, the prune update's dx and the covariance behind the frame."""
    w, P0, prune, remove = window8(True)
    case = ic.make_case('larvio', 10, n=LEG, seed=52, rate=200.0, skipped=1, beyond=2)
    srv, _ = ic.run_mirror(case, with_P=False)
    Phi, Q = mi.accumulate_sequential(srv.steps)
    ref = mirror_frame.step_frame(P0, dict(w=w, slam=[], prune=prune, Phi=Phi, Q=0.5 * (Q + Q.T), remove=remove), 1, False)
    a = _handle()
    try:
        a.cov_set(P0)
        arm(a, case)
        got = a.io_step_frame(w, None, None, True, None, 1, prune, False, remove)
        rel = lambda x, y: float(np.linalg.norm(x - y) / np.linalg.norm(y))
        figs = (rel(got['dx'], ref['dx']), rel(got['prune_dx'], ref['prune_dx']), rel(a.cov_get(), ref['P']))
        print('armed frame against the mirror chain: dx %.2e, prune dx %.2e, P %.2e' % figs)
        assert np.array_equal(got['accept'], ref['accept']) and got['n_after'] == ref['n_after']
        assert max(figs) < 1e-6
    finally:
        a.close()


def test_armed_step_frame_ex_with_a_lost_in_state_feature(built, aux):
    """the first frames of synth.make_lifecycle_stream, every one armed on one handle and given Phi_out / Q_out on the other: lost
    in-state features, anchor changes, the prune update"""
    fl = synth.Flags(use_larvio=1)
    frames, P0 = synth.make_lifecycle_stream(fl)
    a, b = _handle(ekf=True), _handle(ekf=True)
    seen_lost = seen_prune = False
    try:
        a.cov_set(P0); b.cov_set(P0)
        for it, fr in enumerate(frames[:4]):
            case = ic.make_case('larvio', 5 + it, n=LEG, seed=60 + it, rate=200.0)
            Phi, Q = phi_q(aux, case)
            kw = dict(win=fr['w'], augment=True, slam=fr['slam'], idp_dim=1, prune=fr['prune'], prune_apply_dx=True, remove=fr['remove'],
                      n_feature_states=fr['n_feature_states'], lost=fr['lost'], changes=fr['changes'], R_b2c=fr['R_b2c'], t_c_b=fr['t_c_b'])
            for u in (a, b):
                u.set_extra_states(fr['w'].n_extra)
            arm(a, case)
            ga = a.io_step_frame_ex(Phi=None, Q=None, **kw)
            gb = b.io_step_frame_ex(Phi=Phi, Q=Q, **kw)
            same_frame(ga, gb)
            assert ga['status_changes'] == gb['status_changes'] == 0
            if len(fr['changes']):
                assert np.array_equal(ga['new_param'], gb['new_param']) and np.array_equal(ga['new_inv_depth'], gb['new_inv_depth'])
            assert np.array_equal(a.cov_get(), b.cov_get()), it
            seen_lost |= len(fr['lost']) > 0
            seen_prune |= fr['prune'] is not None
        assert seen_lost and seen_prune
    finally:
        a.close(); b.close()


def test_armed_zupt_frame_equals_the_frame_given_phi_q_bit_for_bit(built, aux):
    N = 6   # the window the update sees
    rng = np.random.default_rng(71)
    P0 = ic.make_cov(LEG + 6 * (N - 1), rng)
    r = 1e-3 * rng.standard_normal(9)
    case = ic.make_case('larvio', 10, n=LEG, seed=72, rate=200.0)
    Phi, Q = phi_q(aux, case)
    a, b = _handle(), _handle()
    try:
        a.cov_set(P0); b.cov_set(P0)
        arm(a, case)
        with pytest.raises(capi.MsckfError) as e:
            a.cov_zupt_frame(LEG, N, r, synth.ZUPT_NOISES, Phi, Q, True, True)
        assert e.value.code == 1
        ga = a.cov_zupt_frame(LEG, N, r, synth.ZUPT_NOISES, None, None, True, True)
        gb = b.cov_zupt_frame(LEG, N, r, synth.ZUPT_NOISES, Phi, Q, True, True)
        assert ga['applied'] == gb['applied'] == 1 and ga['n_after'] == gb['n_after']
        assert np.array_equal(ga['dx'], gb['dx']) and np.array_equal(a.cov_get(), b.cov_get())
    finally:
        a.close(); b.close()


def test_a_refused_phi_refuses_the_armed_frames_propagation_and_both_updates(built):
    """The armed path's own refusal (the head launch, the two updates' commits, the kept status words): the right closed form with an
    exactly zero gyro sample.  A status word, not a fault.  Augmentation and marginalisation stand: the covariance is the one the
    separate calls cov_augment + cov_remove_clones leave, bit for bit."""
    w, P0, prune, remove = window8(True)
    case = ic.make_case('right_closed', 5, n=LEG, seed=53)
    case['samples'][2, 1:4] = case['state'].bg
    a, b = _handle(), _handle()
    try:
        a.cov_set(P0); b.cov_set(P0)
        arm(a, case)
        got = a.io_step_frame(w, None, None, True, None, 1, prune, False, remove, raise_on_refusal=False)
        assert got['rc'] == 6 and got['status_first'] == 6 and got['status_prune'] == 6   # ORCVIO_ERR_NOT_SPD
        assert got['stats'][3] == 0 and got['prune_stats'][3] == 0 and got['repaired'] == 0
        b.cov_augment()
        b.cov_remove_clones(LEG, remove)
        assert np.array_equal(a.cov_get(), b.cov_get())
        # the handle is usable: a good armed frame behind it equals the frame given Phi, Q
        good = ic.make_case('right_closed', 5, n=LEG, seed=53)
        w2 = synth.make_window(N=7, F=6, seed=4, track_len=(4, 7), flags=synth.Flags(use_larvio=1))
        arm(a, good)
        ga = a.io_step_frame(w2, None, None, True)
        assert ga['status_first'] == 0 and ga['stats'][3] == 1 and np.isfinite(a.cov_get()).all()
    finally:
        a.close(); b.close()


def test_a_refused_phi_on_a_stream_frame_through_the_general_update_path(built):
    """The same refusal where the updates take the square-root path and its one-launch finish (a 20-clone frame of the config-1 stream
    with twelve in-state features and the prune update; the 6-track window above takes the direct form of a thin stack)."""
    fl = synth.Flags(use_larvio=1)
    frames, P0 = synth.make_stream(fl)
    f0, f1 = frames[0], frames[1]
    assert f1['prune'] is not None and f1['w'].N == 20 and f1['w'].F > 16
    case = ic.make_case('right_closed', 5, n=LEG, seed=54)
    case['samples'][2, 1:4] = case['state'].bg
    a, b = _handle(12, ekf=True), _handle(12, ekf=True)
    try:
        a.cov_set(P0); b.cov_set(P0)
        for u in (a, b):   # (the 19-clone frame in front of it, as the stream runs)
            g0 = u.io_step_frame(f0['w'], f0['Phi'], f0['Q'], True, f0['slam'], 1, f0['prune'], False, f0['remove'])
            assert g0['status_first'] == 0
        arm(a, case)
        got = a.io_step_frame(f1['w'], None, None, True, f1['slam'], 1, f1['prune'], False, f1['remove'], raise_on_refusal=False)
        assert got['rc'] == 6 and got['status_first'] == 6 and got['status_prune'] == 6 and got['stats'][3] == 0 and got['prune_stats'][3] == 0
        b.cov_augment()
        b.cov_remove_clones(LEG, f1['remove'])
        assert np.array_equal(a.cov_get(), b.cov_get())
    finally:
        a.close(); b.close()
