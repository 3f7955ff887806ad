"""GPU tests of the zero-velocity frame class on the resident covariance: orcvio_msckf_cov_zupt and orcvio_msckf_cov_zupt_frame against
the literal restatement of measurementUpdate_ZUPT_vpq in tests/mirror_zupt.py (dense H, S, K, (I - K H) P), element by element.

Shapes: the smallest at which the kernels can go wrong -- the minimum window for both LEG sizes, the 32-tile edge and one past it, 3-d
feature states, one and two nuisance blocks, the shipped operating point (more than one workgroup of the factor kernel) and the largest
window that still carries a resident factor.  Tolerances: 1e-12 max|.| for P+ and dx (the two forms differ by < 1e-15 on such priors,
tests/test_zupt_mirror.py), exact symmetry, and 1e-9 for an MSCKF update that follows."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror, mirror_cov, mirror_frame, oracle
from helpers import rel
import lifecycle_cases as lc
import mirror_zupt as mz

pytestmark = pytest.mark.gpu
NOISES = synth.ZUPT_NOISES
# name: leg, N, idp_dim, feature states, nuisance blocks
CASES = {
    'min22': (22, 2, 1, 0, 0),       # n = 34
    'min46': (46, 2, 1, 0, 0),       # n = 58
    'edge64': (22, 7, 1, 0, 0),      # n = 64: exactly two tiles
    'edge65': (22, 7, 1, 1, 0),      # n = 65: one past the tile edge, and past one workgroup of the factor kernel
    'feat3d': (22, 3, 3, 3, 0),      # n = 49
    'nui1': (22, 4, 1, 0, 1),        # n = 52
    'nui2': (22, 4, 1, 0, 2),        # n = 58
    'ship142': (22, 20, 1, 0, 0),    # n = 142
    'big226': (46, 30, 1, 0, 0),     # n = 226: beyond cov_prefactor's 224 -- the factor comes from n = 220 through cov_augment
}
SCALED = [(name, 1.0) for name in CASES] + [('ship142', 1e4), ('edge65', 1e-4)]


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=40, max_features=512, max_observations=16384, debug_hooks=True)
    yield u
    u.close()


def _dims(name):
    leg, N, d, nf, nui = CASES[name]
    extra = d * nf + 6 * nui
    return leg, N, extra, nui, leg + 6 * N + extra


def _prior(name, seed=0):
    leg, N, extra, nui, n = _dims(name)
    if name == 'ship142':   # the filter's own prior: zero rows for the states that are not estimated
        return synth.make_prior_cov(N, np.random.default_rng(142 + seed), leg_dim=leg)
    return lc.spd(n, n + seed)


def _residual(seed):
    rng = np.random.default_rng(900 + seed)
    return np.concatenate([2e-3 * rng.standard_normal(3), 1e-3 * rng.standard_normal(3), 5e-4 * rng.standard_normal(3)])


class _Options:
    """ORCVIO_OPT_EXTRA_STATES / _SCHMIDT_STATES for the block, zero afterwards"""
    def __init__(self, upd, extra, nui):
        self.upd, self.extra, self.nui = upd, extra, nui

    def __enter__(self):
        self.upd.set_extra_states(self.extra)
        self.upd.set_schmidt_states(self.nui)

    def __exit__(self, *exc):
        self.upd.set_extra_states(0)
        self.upd.set_schmidt_states(0)


def _close(got, ref, what):
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    print(f'{what}: max err {err:.3e}, max |ref| {top:.3e}, ratio {err / top:.3e}')
    assert err <= 1e-12 * top, (what, err, top)


def _update_after(upd, P_ref, N, leg, seed):
    """an MSCKF update on the resident covariance (everything behind the clones as plain extra states) against the oracle's update on
    P_ref -- the numpy restatement where the oracle has no extra states"""
    extra = P_ref.shape[0] - leg - 6 * N
    w = synth.make_window(N=N, F=30, seed=seed, track_len=(2, min(N, 6)), flags=synth.Flags(leg_dim=leg))
    w = dataclasses.replace(w, P=np.ascontiguousarray(P_ref), n_extra=extra)
    upd.set_extra_states(extra)
    try:
        got = upd.update_features(w, resident_cov=True, want_P=True)
    finally:
        upd.set_extra_states(0)
    ref = oracle.msckf_update(w) if extra == 0 else mirror.msckf_update(w)
    assert np.array_equal(got['accept'], ref['accept'])
    assert rel(got['dx'], ref['dx']) < 1e-9, rel(got['dx'], ref['dx'])
    assert rel(got['P_new'], ref['P_new']) < 1e-9, rel(got['P_new'], ref['P_new'])


@pytest.mark.parametrize('name,scale', SCALED)
def test_update_equals_the_mirror_without_a_factor(upd, name, scale):
    leg, N, extra, nui, n = _dims(name)
    P, r = _prior(name), _residual(n)
    nz = tuple(scale * v for v in NOISES)
    upd.cov_set(P)
    with _Options(upd, extra, nui):
        got = upd.cov_zupt(leg, N, r, nz)
    dx_ref, P_ref = mz.measurement_update(P, leg, N, r, *nz, n_nui=nui)
    Pg = upd.cov_get()
    assert got['applied'] == 1 and got['rc'] == 0 and Pg.shape == (n, n)
    _close(Pg, P_ref, 'P+')
    _close(got['dx'], dx_ref, 'dx')
    assert np.array_equal(Pg, Pg.T)
    if nui:
        assert np.array_equal(Pg[n - 6 * nui:, n - 6 * nui:], P[n - 6 * nui:, n - 6 * nui:])
        assert np.abs(Pg[:n - 6 * nui, n - 6 * nui:] - P[:n - 6 * nui, n - 6 * nui:]).max() > 0   # (only the block is the prior's)
    st = capi.debug_factor_state(upd)
    assert st['fac_valid'] == 0 and st['res_n'] == n


def _resident_with_factor(upd, name, seed=1):
    """the case's prior resident WITH its factor; returns the resident matrix"""
    leg, N, extra, nui, n = _dims(name)
    P = lc.spd(n, n + seed)
    if n <= 224:
        upd.cov_set(P)
        upd.cov_prefactor()
    else:   # (no register-resident factorisation of this size: factor one clone less, then augment)
        upd.cov_set(mirror_cov.remove_clones(P, leg, [N - 1]))
        upd.cov_prefactor()
        upd.set_extra_states(extra)
        try:
            upd.cov_augment()
        finally:
            upd.set_extra_states(0)
    st = capi.debug_factor_state(upd)
    assert st['fac_valid'] == 1 and st['fac_n'] == st['res_n'] == n, st
    return upd.cov_get()


@pytest.mark.parametrize('name', list(CASES))
def test_update_with_a_factor_keeps_it_and_the_next_update_is_right(upd, name):
    leg, N, extra, nui, n = _dims(name)
    P, r = _resident_with_factor(upd, name), _residual(n + 1)
    k_before = capi.debug_factor_state(upd)['fac_k']
    with _Options(upd, extra, nui):
        got = upd.cov_zupt(leg, N, r, NOISES)
    dx_ref, P_ref = mz.measurement_update(P, leg, N, r, *NOISES, n_nui=nui)
    Pg = upd.cov_get()
    assert got['applied'] == 1
    _close(Pg, P_ref, 'P+')
    _close(got['dx'], dx_ref, 'dx')
    assert np.array_equal(Pg, Pg.T)
    st = capi.debug_factor_state(upd)
    if nui:
        assert st['fac_valid'] == 0   # (the restored nuisance block breaks P = S S^T)
    else:
        assert st['fac_valid'] == 1 and st['fac_n'] == n and st['fac_k'] == k_before, st
        S = capi.debug_factor(upd)
        e = rel(S @ S.T, Pg)
        print(f'{name}: rel(S+ S+^T, P+) = {e:.3e}')
        assert e < 1e-12, e
    _update_after(upd, P_ref, N, leg, seed=n)


FRAME_VARIANTS = [(p, a, rm) for p in (0, 1) for a in (0, 1) for rm in (0, 1)]


def _frame_inputs(leg, seed):
    rng = np.random.default_rng(seed)
    Phi = np.eye(leg) + 1e-3 * rng.standard_normal((leg, leg))
    G = rng.standard_normal((leg, 12))
    return np.ascontiguousarray(Phi), np.ascontiguousarray(1e-8 * G @ G.T)


@pytest.mark.parametrize('name', ['edge65', 'nui1', 'min46'])
@pytest.mark.parametrize('prop,aug,rm', FRAME_VARIANTS)
def test_frame_call_equals_the_separate_calls_bit_for_bit(upd, name, prop, aug, rm):
    leg, N, extra, nui, n = _dims(name)   # (N: the window the update sees)
    P = lc.spd(n - 6 * aug, 7 * n + aug)
    Phi, Q = _frame_inputs(leg, n)
    r = _residual(n + 2)
    out = []
    for frame in (False, True):
        upd.cov_set(P)
        upd.cov_prefactor()
        with _Options(upd, extra, nui):
            if frame:
                got = upd.cov_zupt_frame(leg, N, r, NOISES, Phi if prop else None, Q if prop else None, bool(aug), bool(rm))
                n_after = got['n_after']
            else:
                if prop:
                    upd.cov_propagate(Phi, Q)
                if aug:
                    upd.cov_augment()
                got = upd.cov_zupt(leg, N, r, NOISES)
                if rm:
                    upd.cov_remove_clones(leg, [N - 2])
                n_after = upd.cov_get().shape[0]
        st = capi.debug_factor_state(upd)
        out.append((upd.cov_get(), got['dx'].copy(), n_after, got['applied'], st, capi.debug_factor(upd) if st['fac_valid'] else None))
    a, b = out
    assert a[2] == b[2] == n - 6 * rm and a[3] == b[3] == 1
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[4] == b[4]
    assert a[4]['fac_valid'] == (0 if (prop or nui) else 1)
    if a[5] is not None:
        assert np.array_equal(a[5], b[5])
        assert rel(a[5] @ a[5].T, a[0]) < 1e-12   # the row deletion behind the update keeps S+


@pytest.mark.parametrize('leg,N,d,nf,nui', [(22, 20, 1, 12, 0), (46, 5, 3, 2, 0), (22, 6, 1, 3, 1)])
@pytest.mark.parametrize('prop,aug,rm', [(1, 1, 1), (0, 1, 1), (1, 0, 0)])
def test_frame_call_equals_the_host_chain(upd, leg, N, d, nf, nui, prop, aug, rm):
    extra = d * nf + 6 * nui
    n = leg + 6 * N + extra
    P = lc.spd(n - 6 * aug, 3 * n + aug)
    Phi, Q = _frame_inputs(leg, n + 1)
    r = _residual(n + 3)
    upd.cov_set(P)
    with _Options(upd, extra, nui):
        got = upd.cov_zupt_frame(leg, N, r, NOISES, Phi if prop else None, Q if prop else None, bool(aug), bool(rm))
    dx_ref, P_ref = mz.stationary_frame(P, leg, N, r, NOISES, Phi if prop else None, Q if prop else None, bool(aug), bool(rm), rest=extra, n_nui=nui)
    Pg = upd.cov_get()
    assert got['applied'] == 1 and got['n_after'] == P_ref.shape[0] == Pg.shape[0]
    _close(Pg, P_ref, 'P after the frame')
    _close(got['dx'], dx_ref, 'dx')


@pytest.mark.parametrize('propagate_stationary', [True, False], ids=['propagated', 'factor-carried'])
def test_loop_of_moving_and_stationary_frames(built, propagate_stationary):
    """Thirty frames of synth.make_zupt_stream on ONE resident covariance: moving frames through io_step_frame, stationary ones through
    cov_zupt_frame, each against the host chain.  A stationary frame that propagates has no factor behind it (Phi P Phi^T + Q is not
    a row operation on S); one that does not carries the factor the moving frame in front of it left."""
    idp, nslam = 1, 12
    fl = synth.Flags(use_larvio=1)
    frames, P0 = synth.make_zupt_stream(fl, n_frames=30, n_slam=nslam, idp=idp, propagate_stationary=propagate_stationary)
    assert sum(fr['zupt'] is not None for fr in frames) >= 10 and sum(fr['zupt'] is None for fr in frames) >= 10
    table = mirror.chi2_table(fl.chi2_prob)
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096, debug_hooks=True)
    try:
        u.set_extra_states(idp * nslam)
        u.set_ekf_rows_mode(True)
        u.cov_set(P0)
        P, carried = P0, 0
        for it, fr in enumerate(frames):
            if fr['zupt'] is None:
                got = u.io_step_frame(fr['w'], fr['Phi'], fr['Q'], True, fr['slam'], idp, fr['prune'], False, fr['remove'])
                ref = mirror_frame.step_frame(P, fr, idp, 0, table=table)
                assert got['rc'] == 0 and np.array_equal(got['accept'], ref['accept']), it
                assert rel(got['dx'], ref['dx']) < 1e-9, it
                P = ref['P']
            else:
                z = fr['zupt']
                before = capi.debug_factor_state(u)
                got = u.cov_zupt_frame(fl.leg_dim, z['n_clones'], z['r'], z['noises'], fr['Phi'], fr['Q'], True, fr['remove_previous'])
                dx_ref, P = mz.stationary_frame(P, fl.leg_dim, z['n_clones'], z['r'], z['noises'], fr['Phi'], fr['Q'], True,
                                                fr['remove_previous'], rest=idp * nslam)
                assert got['applied'] == 1 and rel(got['dx'], dx_ref) < 1e-9, it
                st = capi.debug_factor_state(u)
                if propagate_stationary:
                    assert st['fac_valid'] == 0, it
                else:
                    assert st['fac_valid'] == before['fac_valid'], it
                    if st['fac_valid']:
                        S = capi.debug_factor(u)
                        assert st['fac_n'] == P.shape[0] and rel(S @ S.T, P) < 1e-9, it
                        carried += 1
            Pg = u.cov_get()
            assert got['n_after'] == P.shape[0] == Pg.shape[0], it
            assert rel(Pg, P) < 1e-9, (it, rel(Pg, P))
        assert propagate_stationary or carried >= 5, carried
    finally:
        u.close()


def _state(upd):
    st = capi.debug_factor_state(upd)
    return upd.cov_get(), st, capi.debug_factor(upd) if st['fac_valid'] else None


def _unchanged(upd, ref, what):
    P, st, S = _state(upd)
    assert np.array_equal(P, ref[0]), what
    assert st == ref[1], what
    assert (S is None) == (ref[2] is None) and (S is None or np.array_equal(S, ref[2])), what


def test_validation_failures_leave_everything_as_it_was(upd):
    leg, N = 22, 6
    n = leg + 6 * N
    upd.cov_set(lc.spd(n, 5))
    upd.cov_prefactor()
    ref = _state(upd)
    assert ref[1]['fac_valid'] == 1
    r = _residual(1)
    Phi, Q = _frame_inputs(leg, 2)
    bad_r = r.copy(); bad_r[7] = np.inf
    bad = {
        'leg_dim': dict(leg_dim=23),
        'one clone': dict(n_clones=1),
        'dimension': dict(n_clones=N + 1),
        'zero variance': dict(noises=(1e-4, 0.0, 1e-3)),
        'negative variance': dict(noises=(-1e-4, 1e-4, 1e-3)),
        'nan variance': dict(noises=(1e-4, 1e-4, np.nan)),
        'infinite variance': dict(noises=(np.inf, 1e-4, 1e-3)),
        'non-finite r': dict(r=bad_r),
    }
    for what, kw in bad.items():
        args = dict(leg_dim=leg, n_clones=N, r=r, noises=NOISES)
        args.update(kw)
        with pytest.raises(capi.MsckfError) as e:
            upd.cov_zupt(**args)
        assert e.value.code == 1, what
        _unchanged(upd, ref, what)
        with pytest.raises(capi.MsckfError) as e:   # (the frame call: the same window after its augmentation)
            upd.cov_zupt_frame(args['leg_dim'], args['n_clones'] + 1, args['r'], args['noises'], Phi, Q, True, True)
        assert e.value.code == 1, what
        _unchanged(upd, ref, 'frame: ' + what)
    with pytest.raises(capi.MsckfError):   # Phi without Q
        upd.cov_zupt_frame(leg, N + 1, r, NOISES, Phi, None, True, True)
    _unchanged(upd, ref, 'Phi without Q')
    upd.set_extra_states(3)   # the options declare states the resident covariance does not have
    try:
        with pytest.raises(capi.MsckfError):
            upd.cov_zupt(leg, N, r, NOISES)
        with pytest.raises(capi.MsckfError):
            upd.cov_zupt_frame(leg, N + 1, r, NOISES, None, None, True, False)
    finally:
        upd.set_extra_states(0)
    _unchanged(upd, ref, 'extra states')
    import ctypes as C
    z = capi.MsckfUpdater._zupt_struct(leg, N, r, NOISES)
    dx = np.zeros(n)
    ap = C.c_int32(0)
    dp = dx.ctypes.data_as(C.POINTER(C.c_double))
    assert upd.lib.orcvio_msckf_cov_zupt(upd.h, None, dp, C.byref(ap)) == 1
    assert upd.lib.orcvio_msckf_cov_zupt(upd.h, C.byref(z), None, C.byref(ap)) == 1
    assert upd.lib.orcvio_msckf_cov_zupt(upd.h, C.byref(z), dp, None) == 1
    assert upd.lib.orcvio_msckf_cov_zupt(None, C.byref(z), dp, C.byref(ap)) == 1
    assert upd.lib.orcvio_msckf_cov_zupt_frame(upd.h, None, dp, C.byref(ap), C.byref(ap)) == 1
    _unchanged(upd, ref, 'null arguments')


def test_a_communicator_on_the_handle_is_refused(built):
    leg, N = 22, 3
    u = capi.MsckfUpdater(device=0, max_clones=8, max_features=64, max_observations=1024, debug_hooks=True)
    try:
        P = lc.spd(leg + 6 * N, 8)
        u.cov_set(P)
        u.comm_init(capi.comm_unique_id(), 0, 1)
        for call in (lambda: u.cov_zupt(leg, N, _residual(3), NOISES), lambda: u.cov_zupt_frame(leg, N + 1, _residual(3), NOISES, None, None, True, True)):
            with pytest.raises(capi.MsckfError) as e:
                call()
            assert e.value.code == 1
            assert np.array_equal(u.cov_get(), P)
        u.comm_destroy()
        assert u.cov_zupt(leg, N, _residual(3), NOISES)['applied'] == 1
    finally:
        u.close()


@pytest.mark.parametrize('what', ['nan in row 4', 'indefinite M'])
def test_device_refusals_apply_nothing(upd, what):
    """Inputs the update must reject: NOT_SPD, applied = 0, dx = 0, P and the factor state as before."""
    leg, N = 22, 12
    n = leg + 6 * N
    P = lc.spd(n, 21)
    if what == 'nan in row 4':
        P[4, n - 1] = np.nan   # (a column only the last tile's workgroups hold: every workgroup must still refuse)
    else:
        P[3:6, 3:6] = -np.eye(3)
    r = _residual(5)
    upd.cov_set(P)
    ref = _state(upd)
    got = upd.cov_zupt(leg, N, r, NOISES, raise_on_refusal=False)
    assert got['rc'] == 6 and got['applied'] == 0 and not got['dx'].any()
    P1, st1, _ = _state(upd)
    assert np.array_equal(P1, ref[0], equal_nan=True) and st1 == ref[1]
    with pytest.raises(capi.MsckfError) as e:
        upd.cov_zupt(leg, N, r, NOISES)
    assert e.value.code == 6
    # the frame call: marginalisation stands, the update does not
    got = upd.cov_zupt_frame(leg, N, r, NOISES, None, None, False, True, raise_on_refusal=False)
    assert got['rc'] == 6 and got['applied'] == 0 and not got['dx'].any() and got['n_after'] == n - 6
    assert np.array_equal(upd.cov_get(), mirror_cov.remove_clones(P, leg, [N - 2]), equal_nan=True)
