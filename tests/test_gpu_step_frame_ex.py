"""One filter frame WITH the in-state features' life cycle in one call (orcvio_msckf_io_step_frame_ex): against the host chain
(tests/mirror_frame_lifecycle.py) over synth.make_lifecycle_stream, bit for bit against the library's separate calls, the
resident factor, the refusals, the non-finite position made on the device, and the other launch paths."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
import mirror_frame_lifecycle as mfl
from helpers import rel

pytestmark = pytest.mark.gpu
TOL = 1e-8   # tests/test_gpu_step_oracle.py's
EUROC = dict(use_larvio=1)
KITTI = dict(use_larvio=0, use_left_perturbation=0, noise_feature=1.0, discard_large_update=1)
# name: (flags, sigma_px, idp, leg, literal_3d)
FLAG_SETS = {
    'euroc': (EUROC, None, 1, 22, 0),
    'kitti': (KITTI, 0.008, 1, 22, 0),
    'fej_td': (dict(use_larvio=1, if_fej=1, estimate_td=1), None, 1, 22, 0),
    'leg46': (dict(use_larvio=1, leg_dim=46), None, 1, 46, 0),
    'idp3': (EUROC, None, 3, 22, 0),
    'idp3_literal': (EUROC, None, 3, 22, 1),
}
_CHAINS = {}


def _stream(name):
    fl, sigma_px, idp, leg, lit = FLAG_SETS[name]
    frames, P0 = synth.make_lifecycle_stream(synth.Flags(**fl), sigma_px=sigma_px, idp=idp, leg=leg)
    return frames, P0, idp, lit


def _chain(name, apply_dx):
    key = (name, apply_dx)
    if key not in _CHAINS:
        frames, P0, idp, lit = _stream(name)
        _CHAINS[key] = (frames, P0, idp, lit, mfl.run_stream(frames, P0, idp, apply_dx, literal_3d=lit))
    return _CHAINS[key]


def _handle(debug_hooks=False):
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096, debug_hooks=debug_hooks)
    u.set_ekf_rows_mode(True)
    return u


def _step_ex(u, fr, idp, apply_dx, lit=0, **over):
    u.set_extra_states(fr['w'].n_extra)
    kw = dict(win=fr['w'], Phi=fr['Phi'], Q=fr['Q'], augment=True, slam=fr['slam'], idp_dim=idp, prune=fr['prune'], prune_apply_dx=apply_dx,
              remove=fr['remove'], n_feature_states=fr['n_feature_states'], lost=fr['lost'], changes=fr['changes'], R_b2c=fr['R_b2c'],
              t_c_b=fr['t_c_b'], literal_3d=lit)
    kw.update(over)
    return u.io_step_frame_ex(**kw)


def _gamma_err(got, ref):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    return rel(got[~nan], ref[~nan]) if (~nan).any() else 0.0


def _run(u, name, apply_dx, repaired=False):
    frames, P0, idp, lit, refs = _chain(name, apply_dx)
    worst = dict(dx=0.0, prune_dx=0.0, P=0.0, gamma=0.0, new_param=0.0, new_inv_depth=0.0)
    u.cov_set(P0)
    for it, (fr, ref) in enumerate(zip(frames, refs)):
        got = _step_ex(u, fr, idp, apply_dx, lit)
        assert got['rc'] == 0 and got['status_first'] == 0 and got['status_prune'] == 0 and got['status_changes'] == 0, (it, got['rc'])
        if repaired:
            assert got['repaired'] == (2 if fr['prune'] is not None else 1), (it, got['repaired'])
        else:
            assert got['repaired'] == 0, it
        assert np.array_equal(got['accept'], ref['accept']), it
        worst['gamma'] = max(worst['gamma'], _gamma_err(got['gamma'], ref['gamma']))
        worst['dx'] = max(worst['dx'], rel(got['dx'], ref['dx']))
        if fr['prune'] is not None:
            assert np.array_equal(got['prune_accept'], ref['prune_accept']), it
            worst['prune_dx'] = max(worst['prune_dx'], rel(got['prune_dx'], ref['prune_dx']))
        else:
            assert got['prune_dx'] is None
        if fr['changes']:
            worst['new_param'] = max(worst['new_param'], rel(got['new_param'], ref['new_param']))
            worst['new_inv_depth'] = max(worst['new_inv_depth'], rel(got['new_inv_depth'], ref['new_inv_depth']))
        else:
            assert got['new_param'] is None
        Pg = u.cov_get()
        assert got['n_after'] == ref['n_after'] == Pg.shape[0], it
        worst['P'] = max(worst['P'], rel(Pg, ref['P']))
        assert max(worst.values()) <= TOL, (it, worst)
    return worst


@pytest.mark.parametrize('apply_dx', [0, 1], ids=['copy', 'increment'])
@pytest.mark.parametrize('name', list(FLAG_SETS))
def test_step_frame_ex_against_the_chain(built, name, apply_dx):
    u = _handle()
    try:
        worst = _run(u, name, apply_dx)
    finally:
        u.close()
    print(f'{name} prune_apply_dx={apply_dx}: worst rel err', worst)


def _frame_by_calls(u, fr, idp, lit):
    """cov_propagate, cov_augment, cov_remove_features, update, cov_change_anchors, update, cov_remove_clones."""
    w = fr['w']
    leg = w.flags.leg_dim
    u.set_extra_states(idp * fr['n_feature_states'])   # (the new clone goes in front of the feature states as they are before the removals)
    u.cov_propagate(fr['Phi'], fr['Q'])
    u.cov_augment()
    u.cov_remove_features(leg, w.N, idp, fr['n_feature_states'], fr['lost'])
    u.set_extra_states(w.n_extra)
    io = u.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=False)
    u.io_fill(io, w, with_P=False)
    u.make_slam_call(idp, fr['slam'])()
    u.io_update(want_P=False, commit=True)
    out = dict(dx=io['dx'].copy(), gamma=io['gamma'].copy(), accept=io['accept'].copy(), prune_dx=None, new_param=None, new_inv_depth=None)
    if fr['changes']:
        out['new_param'], out['new_inv_depth'] = u.cov_change_anchors(w.flags, idp, synth.pack_poses(w), fr['R_b2c'], fr['t_c_b'], fr['changes'], lit)
    if fr['prune'] is not None:
        p = fr['prune']
        io = u.io_begin(p.flags, p.N, p.F, int(p.obs_ptr[-1]), with_P=False)
        u.io_fill(io, p, with_P=False)
        u.io_update(want_P=False, commit=True)
        out['prune_dx'] = io['dx'].copy()
    if fr['remove']:
        u.cov_remove_clones(leg, fr['remove'])
    return out


@pytest.mark.parametrize('name', ['euroc', 'kitti', 'fej_td', 'idp3', 'idp3_literal'])
def test_step_frame_ex_equals_the_separate_calls_bit_for_bit(built, name):
    frames, P0, idp, lit = _stream(name)
    a, b = _handle(), _handle()
    try:
        a.cov_set(P0); b.cov_set(P0)
        for it, fr in enumerate(frames):
            ref = _frame_by_calls(a, fr, idp, lit)
            got = _step_ex(b, fr, idp, 0, lit)
            assert got['repaired'] == 0 and got['rc'] == 0
            assert np.array_equal(got['dx'], ref['dx']), it
            assert np.array_equal(got['gamma'], ref['gamma'], equal_nan=True) and np.array_equal(got['accept'], ref['accept'])
            if fr['prune'] is not None:
                assert np.array_equal(got['prune_dx'], ref['prune_dx']), it
            if fr['changes']:
                assert np.array_equal(got['new_param'], ref['new_param']) and np.array_equal(got['new_inv_depth'], ref['new_inv_depth']), it
            assert np.array_equal(a.cov_get(), b.cov_get()), it
    finally:
        a.close(); b.close()


def test_step_frame_ex_without_events_is_step_frame_bit_for_bit(built):
    frames, P0 = synth.make_stream(synth.Flags(**EUROC))
    a, b = _handle(), _handle()
    try:
        a.set_extra_states(12); b.set_extra_states(12)
        a.cov_set(P0); b.cov_set(P0)
        for it, fr in enumerate(frames):
            ref = a.io_step_frame(fr['w'], fr['Phi'], fr['Q'], True, fr['slam'], 1, fr['prune'], True, fr['remove'])
            got = b.io_step_frame_ex(fr['w'], fr['Phi'], fr['Q'], True, fr['slam'], 1, fr['prune'], True, fr['remove'], n_feature_states=12)
            for k in ('dx', 'gamma', 'accept', 'prune_dx', 'prune_gamma', 'prune_accept'):
                assert (ref[k] is None and got[k] is None) or np.array_equal(ref[k], got[k], equal_nan=True), (it, k)
            assert got['new_param'] is None and got['status_changes'] == 0
            assert np.array_equal(a.cov_get(), b.cov_get()), it
    finally:
        a.close(); b.close()


def _factor_ok(u):
    st = capi.debug_factor_state(u)
    if not st['fac_valid']:
        return False
    S = capi.debug_factor(u)
    P = u.cov_get()
    assert st['fac_n'] == P.shape[0]
    assert rel(S @ S.T, P) < 1e-12, rel(S @ S.T, P)
    return True


def test_resident_factor_through_the_events(built):
    """Wherever the separate calls leave a valid resident factor the one call does too, and S S^T = P; with an augmentation-only
    frame (no Phi) that loses features: the factor's removal inside the head."""
    frames, P0, idp, lit = _stream('euroc')
    a, b = _handle(debug_hooks=True), _handle(debug_hooks=True)
    try:
        a.cov_set(P0); b.cov_set(P0)
        seen = 0
        for it, fr in enumerate(frames):
            if it in (4, 6):   # augmentation-only frames that lose features
                fr = dict(fr, Phi=None, Q=None)
                assert fr['lost'] and fr['w'].N == 19
            if it == 6:   # (frame 5 has no prune update: its first update's factor comes through the anchor change and the marginalisation)
                assert capi.debug_factor_state(b)['fac_valid'] == 1
            w = fr['w']
            # the separate calls
            a.set_extra_states(idp * fr['n_feature_states'])
            if fr['Phi'] is not None:
                a.cov_propagate(fr['Phi'], fr['Q'])
            a.cov_augment()
            a.cov_remove_features(w.flags.leg_dim, w.N, idp, fr['n_feature_states'], fr['lost'])
            a.set_extra_states(w.n_extra)
            io = a.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=False)
            a.io_fill(io, w, with_P=False)
            a.make_slam_call(idp, fr['slam'])()
            a.io_update(want_P=False, commit=True)
            if fr['changes']:
                a.cov_change_anchors(w.flags, idp, synth.pack_poses(w), fr['R_b2c'], fr['t_c_b'], fr['changes'], lit)
                fa_mid = _factor_ok(a)
            if fr['prune'] is not None:
                p = fr['prune']
                io = a.io_begin(p.flags, p.N, p.F, int(p.obs_ptr[-1]), with_P=False)
                a.io_fill(io, p, with_P=False)
                a.io_update(want_P=False, commit=True)
            if fr['remove']:
                a.cov_remove_clones(w.flags.leg_dim, fr['remove'])
            got = _step_ex(b, fr, idp, 0, lit)
            assert got['rc'] == 0 and got['repaired'] == 0
            assert np.array_equal(a.cov_get(), b.cov_get()), it
            fa, fb = _factor_ok(a), _factor_ok(b)
            assert fb or not fa, it
            seen += int(fb)
        assert seen >= 3
    finally:
        a.close(); b.close()


def test_refusals_leave_nothing_done(built):
    frames, P0, idp, lit = _stream('euroc')
    u, v = _handle(debug_hooks=True), _handle(debug_hooks=True)
    try:
        u.cov_set(P0); v.cov_set(P0)
        _step_ex(u, frames[0], idp, 1); _step_ex(v, frames[0], idp, 1)
        fr = frames[1]
        assert fr['lost'] and fr['changes'] and fr['prune'] is not None
        P1, st1, S1 = u.cov_get(), capi.debug_factor_state(u), capi.debug_factor(u)
        C = synth.LifecycleChange
        ch = fr['changes']
        free = [j for j, f in enumerate(fr['slam']) if f.anchor not in (0, 1)][0]
        cases = {
            'slots descending': dict(lost=[5, 2], n_feature_states=fr['n_feature_states'] + 1),
            'slot out of range': dict(lost=[fr['n_feature_states']]),
            'no record': dict(slam=None),
            'record anchored elsewhere': dict(changes=[C(free, 0, 5, fr['slam'][free].p_w, fr['slam'][free].p_fej)] + ch[1:]),
            'new anchor leaves': dict(changes=[dataclasses.replace(ch[0], new=1 - ch[0].old)] + ch[1:]),
            '17 changes': dict(changes=[C(j % len(fr['slam']), 0, 5, ch[0].p_w, ch[0].p_fej) for j in range(17)]),
            'dimension': dict(n_feature_states=fr['n_feature_states'] + 1),
        }
        for what, over in cases.items():
            with pytest.raises(capi.MsckfError) as e:
                _step_ex(u, fr, idp, 1, **over)
            assert e.value.code in (1, 3), what
            assert np.array_equal(u.cov_get(), P1), what
            assert capi.debug_factor_state(u) == st1 and np.array_equal(capi.debug_factor(u), S1), what
        u.set_schmidt_states(1)
        with pytest.raises(capi.MsckfError):
            _step_ex(u, fr, idp, 1)
        u.set_schmidt_states(0)
        assert np.array_equal(u.cov_get(), P1)
        # the next ordinary frame is what it is on a handle that saw no refusal
        a, b = _step_ex(u, fr, idp, 1), _step_ex(v, fr, idp, 1)
        assert np.array_equal(a['dx'], b['dx']) and np.array_equal(a['prune_dx'], b['prune_dx']) and np.array_equal(a['new_param'], b['new_param'])
        assert np.array_equal(u.cov_get(), v.cov_get())
    finally:
        u.close(); v.close()


def test_a_non_finite_position_made_on_the_device_refuses_the_changes(built):
    """inv_depth + dx[col] == 0 exactly: a changed feature whose observation is a gross outlier (the 2-dof gate rejects its rows, so
    its inverse depth does not enter dx), dx[col] read from a first run of the same frame (the call is deterministic bit for bit),
    inv_depth = -dx[col], the frame again from the same covariance.  P keeps the first update's result WITHOUT any anchor change,
    the prune update is refused, status_changes says so."""
    frames, P0, idp, lit = _stream('euroc')
    u = _handle()
    try:
        u.cov_set(P0)
        _step_ex(u, frames[0], idp, 1)
        P1 = u.cov_get()
        fr = frames[1]
        c = fr['changes'][0]
        slam = list(fr['slam'])
        slam[c.slot] = dataclasses.replace(slam[c.slot], z=slam[c.slot].z + 5.0)   # a gross outlier: gated out
        fr = dict(fr, slam=slam)
        col = fr['w'].flags.leg_dim + 6 * fr['w'].N + c.slot
        first = _step_ex(u, fr, idp, 1)
        assert first['rc'] == 0 and first['status_changes'] == 0
        dxc = float(first['dx'][col])
        slam[c.slot] = dataclasses.replace(slam[c.slot], inv_depth=-dxc)
        u.cov_set(P1)
        again = _step_ex(u, fr, idp, 1, raise_on_refusal=False)
        if not np.array_equal(again['dx'], first['dx']):
            pytest.fail('the changed inverse depth entered dx: the construction does not hold (the feature was not gated out)')
        assert again['rc'] == 6 and again['status_first'] == 0 and again['status_changes'] == 6 and again['status_prune'] == 6
        assert again['prune_stats'][3] == 0
        # what is left: the first update's covariance, no anchor change, no prune update, the marginalisation
        u.cov_set(P1)
        ref = _step_ex(u, dict(fr, changes=[], prune=None), idp, 1)
        Pref = u.cov_get()
        u.cov_set(P1)
        _step_ex(u, fr, idp, 1, raise_on_refusal=False)
        assert ref['rc'] == 0 and np.array_equal(u.cov_get(), Pref)
    finally:
        u.close()


@pytest.mark.parametrize('off', ['ORCVIO_STEP_FUSED', 'ORCVIO_LA_SPIN'])
def test_the_other_launch_paths(built, monkeypatch, off):
    """ORCVIO_STEP_FUSED=0 (diagnostics build): the frame's small steps as launches of their own; ORCVIO_LA_SPIN=0: every update
    gives its hand-off up and is repaired -- the anchor change refuses itself behind the lost first update and runs once, behind
    the repeat."""
    monkeypatch.setenv(off, '0')
    u = _handle(debug_hooks=off == 'ORCVIO_STEP_FUSED')
    monkeypatch.delenv(off)
    try:
        worst = _run(u, 'euroc', 1, repaired=off == 'ORCVIO_LA_SPIN')
    finally:
        u.close()
    print(f'{off}=0: worst rel err', worst)
