"""GPU tests of the in-state feature lifecycle on the resident covariance: orcvio_msckf_cov_remove_features (rmLostFeaturesCov)
and orcvio_msckf_cov_change_anchors (pruneImuStateBuffer's in-state branch, updateFeatureCov_*) against the restatement in
tests/mirror_features_lifecycle.py; both keep the resident square-root factor, and the update after them is right."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror
from helpers import rel
import lifecycle_cases as lc
import mirror_features_lifecycle as mfl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=40, max_features=512, max_observations=16384, debug_hooks=True)
    yield u
    u.close()


def _factor_kept(upd, P):
    st = capi.debug_factor_state(upd)
    assert st['fac_valid'] == 1 and st['fac_n'] == st['res_n'] == P.shape[0]
    S = capi.debug_factor(upd)
    assert rel(S @ S.T, P) < 1e-12


def _update_after(upd, P, N, leg, seed):
    """an MSCKF update on the resident covariance (and its factor) with everything behind the clones as extra states, against
    the numpy restatement"""
    extra = P.shape[0] - leg - 6 * N
    w = synth.make_window(N=N, F=30, seed=seed, track_len=(3, N), flags=synth.Flags(leg_dim=leg))
    w = dataclasses.replace(w, P=np.ascontiguousarray(P), n_extra=extra)
    upd.set_extra_states(extra)
    try:
        got = upd.update_features(w, resident_cov=True, want_P=True)
    finally:
        upd.set_extra_states(0)
    ref = mirror.msckf_update(w)
    assert rel(got['dx'], ref['dx']) < 1e-6
    assert rel(got['P_new'], ref['P_new']) < 1e-6


@pytest.mark.parametrize('leg', [22, 46])
@pytest.mark.parametrize('d', [1, 3])
@pytest.mark.parametrize('nui', [0, 2])
def test_remove_features_equals_restatement_and_keeps_the_factor(upd, leg, d, nui):
    N, nf = 8, 10
    n = leg + 6 * N + d * nf + 6 * nui
    P = lc.spd(n, leg + d + nui)
    upd.cov_set(P)
    upd.cov_prefactor()
    slots = [0, 3, 4, 9]
    upd.cov_remove_features(leg, N, d, nf, slots)
    ref = mfl.rm_lost_features_cov(P, leg, N, d, slots)
    got = upd.cov_get()
    assert np.array_equal(got, ref)
    _factor_kept(upd, ref)
    _update_after(upd, ref, N, leg, seed=leg + d)


@pytest.mark.parametrize('d,literal', [(1, 0), (3, 0), (3, 1)])
@pytest.mark.parametrize('fej', [0, 1])
@pytest.mark.parametrize('k,new_at', [(1, 'newest'), (4, 'middle'), (16, 'newest'), (16, 'middle')])
def test_change_anchors_equals_restatement_and_keeps_the_factor(upd, d, literal, fej, k, new_at):
    leg, N, nf = 22, 10, 18
    w, poses = lc.window(N, 5 + k)
    R_b2c, t_c_b = lc.extrinsics(w)
    n = leg + 6 * N + d * nf
    P = lc.spd(n, 3 * k + d)
    ch = lc.changes(poses, N, nf, k, seed=k + d + 10 * fej, new_at=new_at)
    upd.cov_set(P)
    upd.cov_prefactor()
    flags = synth.Flags(leg_dim=leg, if_fej=fej)
    param, rho = upd.cov_change_anchors(flags, d, poses, R_b2c, t_c_b, ch, literal_3d=literal)
    P_ref, param_ref, rho_ref, _ = mfl.change_anchors(P, leg, N, d, poses, R_b2c, t_c_b, ch, if_fej=fej, literal_3d=literal)
    got = upd.cov_get()
    assert np.abs(got - P_ref).max() <= 1e-12 * np.abs(P_ref).max()
    assert np.array_equal(got, got.T)
    assert np.abs(param - param_ref).max() <= 1e-14 * np.abs(param_ref).max()
    assert np.abs(rho - rho_ref).max() <= 1e-14 * np.abs(rho_ref).max()
    _factor_kept(upd, got)
    _update_after(upd, got, N, leg, seed=k + d)


def test_refusals_leave_the_covariance_and_factor_unchanged(upd):
    leg, N, nf, d = 22, 6, 5, 1
    w, poses = lc.window(N, 3)
    R_b2c, t_c_b = lc.extrinsics(w)
    n = leg + 6 * N + d * nf
    P = lc.spd(n, 9)
    upd.cov_set(P)
    upd.cov_prefactor()
    before = upd.cov_get()
    st0 = capi.debug_factor_state(upd)
    S0 = capi.debug_factor(upd)
    flags = synth.Flags(leg_dim=leg)
    good = lc.changes(poses, N, nf, 2, seed=1)
    bad_cases = {
        'slot out of range': [dataclasses.replace(good[0], slot=nf)],
        'slot listed twice': [good[0], dataclasses.replace(good[1], slot=good[0].slot)],
        'old == new': [dataclasses.replace(good[0], new=good[0].old)],
        'anchor outside the window': [dataclasses.replace(good[0], new=N)],
        'negative anchor': [dataclasses.replace(good[0], old=-1)],
        'non-finite position': [good[0], dataclasses.replace(good[1], p_w=np.array([np.nan, 0.0, 1.0]))],
        'more than 16': [dataclasses.replace(good[0], slot=s) for s in range(17)],
    }
    for name, ch in bad_cases.items():
        with pytest.raises(capi.MsckfError) as e:
            upd.cov_change_anchors(flags, d, poses if name != 'more than 16' else poses, R_b2c, t_c_b, ch)
        assert e.value.code == 1, name
        assert np.array_equal(upd.cov_get(), before), name
    bad_pose = poses.copy()
    bad_pose[2, 10] = np.inf
    with pytest.raises(capi.MsckfError):
        upd.cov_change_anchors(flags, d, bad_pose, R_b2c, t_c_b, good)
    with pytest.raises(capi.MsckfError):
        upd.cov_change_anchors(flags, d, poses, R_b2c, np.array([0.0, np.nan, 0.0]), good)
    for args in ((leg, N, d, nf + 1, [0]),      # the features do not fit
                 (leg, N, d, 2, [0]),           # what is behind them is not whole nuisance blocks
                 (leg, N, d, nf, [3, 1]),       # not ascending
                 (leg, N, d, nf, [1, 1]),
                 (leg, N, d, nf, [nf])):
        with pytest.raises(capi.MsckfError):
            upd.cov_remove_features(*args)
    assert np.array_equal(upd.cov_get(), before)
    assert capi.debug_factor_state(upd) == st0
    assert np.array_equal(capi.debug_factor(upd), S0)


@pytest.mark.parametrize('d', [1, 3])
def test_resident_loop_of_updates_anchor_changes_and_removals(upd, d):
    """Six rounds of update + commit, anchor change, removal of a lost feature on the resident covariance -- P is set once; the
    factor stays alive through every anchor change and removal and is what the next update starts from."""
    leg, N = 22, 10
    nf = 16
    w0, poses = lc.window(N, 60 + d)
    R_b2c, t_c_b = lc.extrinsics(w0)
    P = lc.spd(leg + 6 * N + d * nf, 61 + d)
    upd.cov_set(P)
    flags = synth.Flags(leg_dim=leg)
    for it in range(6):
        extra = P.shape[0] - leg - 6 * N
        w = synth.make_window(N=N, F=30, seed=100 + it, track_len=(3, N))
        w = dataclasses.replace(w, P=np.ascontiguousarray(P), n_extra=extra)
        upd.set_extra_states(extra)
        try:
            got = upd.update_features(w, resident_cov=True, want_P=False)
            upd.cov_commit()
        finally:
            upd.set_extra_states(0)
        ref = mirror.msckf_update(w)
        assert rel(got['dx'], ref['dx']) < 1e-9
        P = ref['P_new']
        assert rel(upd.cov_get(), P) < 1e-9
        nf = extra // d
        ch = lc.changes(poses, N, nf, 3, seed=200 + it)
        upd.cov_change_anchors(flags, d, poses, R_b2c, t_c_b, ch)
        P = mfl.change_anchors(P, leg, N, d, poses, R_b2c, t_c_b, ch)[0]
        assert rel(upd.cov_get(), P) < 1e-9
        st = capi.debug_factor_state(upd)
        assert st['fac_valid'] == 1 and st['fac_n'] == P.shape[0]
        lost = [it % nf]
        upd.cov_remove_features(leg, N, d, nf, lost)
        P = mfl.rm_lost_features_cov(P, leg, N, d, lost)
        assert rel(upd.cov_get(), P) < 1e-9
        st = capi.debug_factor_state(upd)
        assert st['fac_valid'] == 1 and st['fac_n'] == P.shape[0]


def test_slot_in_the_nuisance_block_is_refused(upd):
    """with ORCVIO_OPT_SCHMIDT_STATES = k the last 6 k states are nuisance states: a slot reaching into them is refused, P unchanged;
    the features in front of them change as the restatement says"""
    leg, N, nf, d, nui = 22, 6, 4, 1, 2
    w, poses = lc.window(N, 8)
    R_b2c, t_c_b = lc.extrinsics(w)
    n = leg + 6 * N + d * nf + 6 * nui
    P = lc.spd(n, 12)
    upd.cov_set(P)
    flags = synth.Flags(leg_dim=leg)
    good = lc.changes(poses, N, nf, 2, seed=4)
    upd.set_schmidt_states(nui)
    try:
        with pytest.raises(capi.MsckfError) as e:
            upd.cov_change_anchors(flags, d, poses, R_b2c, t_c_b, [dataclasses.replace(good[0], slot=nf)])
        assert e.value.code == 1
        assert np.array_equal(upd.cov_get(), P)
        upd.cov_change_anchors(flags, d, poses, R_b2c, t_c_b, good)
    finally:
        upd.set_schmidt_states(0)
    P_ref = mfl.change_anchors(P, leg, N, d, poses, R_b2c, t_c_b, good)[0]
    got = upd.cov_get()
    assert np.abs(got - P_ref).max() <= 1e-12 * np.abs(P_ref).max()
    assert np.array_equal(got[-12:, -12:], P[-12:, -12:])
