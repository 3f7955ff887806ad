"""GPU tests of the stationary frame of a HYBRID filter: orcvio_msckf_cov_zupt_frame_hybrid / _cov_zupt_frame_checked_hybrid -- every
in-state feature leaves in front of the zero-velocity update, the previous clone behind it, ONE fused launch (k_zupt_cov_keep,
k_zupt_fac_keep) -- bit for bit against the separate calls cov_propagate, cov_augment, cov_remove_features (all slots), cov_zupt,
cov_remove_clones, and element by element (1e-12 max|.|, tests/test_gpu_zupt.py's bar) against the float64 restatement in
tests/zupt_hybrid_cases.py.  Shapes: that module's table."""
import ctypes as C

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror, mirror_cov, mirror_frame
from helpers import rel
import imu_cases as ic
import zupt_check_cases as zc
import zupt_hybrid_cases as zh

pytestmark = pytest.mark.gpu
NOISES = synth.ZUPT_NOISES
NOT_SPD, INVALID = 6, 1
LEG = 22


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=40, max_features=512, max_observations=16384, debug_hooks=True)
    yield u
    u.set_extra_states(0)
    u.close()


def _state(u):
    st = capi.debug_factor_state(u)
    return u.cov_get(), st, capi.debug_factor(u) if st['fac_valid'] else None


def _same(a, b, what):
    assert np.array_equal(a[0], b[0], equal_nan=True), what
    assert a[1] == b[1], (what, a[1], b[1])
    assert (a[2] is None) == (b[2] is None) and (a[2] is None or np.array_equal(a[2], b[2])), what


def _make_resident(u, P, leg, extra, factor=True):
    """P resident on u, with its factor where one can be made: cov_prefactor up to 224 states, beyond that the factor of fewer
    clones carried through cov_augment.  Returns the resident matrix (the augmentation's own bits)."""
    n = P.shape[0]
    k = 0 if n <= 224 else -(-(n - 224) // 6)
    N = (n - leg - extra) // 6
    u.set_extra_states(extra)
    u.cov_set(mirror_cov.remove_clones(P, leg, list(range(N - k, N))) if k else P)
    if factor:
        u.cov_prefactor()
    for _ in range(k):
        u.cov_augment()
    return u.cov_get()


def _separate(u, leg, N, d, F, r, Phi, Q, aug, rm):
    """the parent's only route; ORCVIO_OPT_EXTRA_STATES = d F on entry, 0 on return"""
    if Phi is not None:
        u.cov_propagate(Phi, Q)
    if aug:
        u.cov_augment()
    if F:
        u.cov_remove_features(leg, N, d, F, list(range(F)))
    u.set_extra_states(0)
    got = u.cov_zupt(leg, N, r, NOISES, raise_on_refusal=False)
    if rm and got['applied']:
        u.cov_remove_clones(leg, [N - 2])
    return dict(got, n_after=u.cov_get().shape[0])


@pytest.mark.parametrize('name', list(zh.CASES))
@pytest.mark.parametrize('prop,aug,rm', zh.VARIANTS)
def test_frame_equals_the_separate_calls_bit_for_bit_and_the_restatement(upd, name, prop, aug, rm):
    leg, N, d, F, b, n = zh.dims(name)
    Phi, Q = zh.frame_inputs(leg, n) if prop else (None, None)
    r = zh.residual(n + 2)
    out = []
    for fused in (False, True):
        P0 = _make_resident(upd, zh.prior(name, aug), leg, d * F)
        if fused:
            got = upd.cov_zupt_frame_hybrid(leg, N, r, NOISES, d, F, Phi, Q, bool(aug), bool(rm))
            upd.set_extra_states(0)
        else:
            got = _separate(upd, leg, N, d, F, r, Phi, Q, aug, rm)
        out.append((got, _state(upd)))
    (ga, sa), (gb, sb) = out
    assert ga['applied'] == gb['applied'] == 1 and gb['rc'] == 0
    assert ga['n_after'] == gb['n_after'] == b - 6 * rm
    assert gb['dx'].shape == (b,) and np.array_equal(ga['dx'], gb['dx'])
    _same(sa, sb, 'fused against separate')
    assert sb[1]['fac_valid'] == (0 if prop else 1), sb[1]   # (Phi P Phi^T + Q is not a row operation on S)
    ref = zh.hybrid_frame(P0, leg, N, d, F, r, NOISES, Phi, Q, bool(aug), bool(rm))
    zh.check_frame(dict(gb, P=sb[0]), ref)
    if sb[2] is not None:
        e = rel(sb[2] @ sb[2].T, sb[0])
        print(f'{name}: rel(S S^T, P) = {e:.3e}')
        assert sb[1]['fac_n'] == b - 6 * rm and e < 1e-12, e


def test_f0_equals_the_plain_frame_call_bit_for_bit(upd):
    leg, N, d, F, b, n = zh.dims('edge64')
    r = zh.residual(6)
    out = []
    for hybrid in (False, True):
        _make_resident(upd, zh.prior('edge64', 1), leg, 0)
        got = (upd.cov_zupt_frame_hybrid(leg, N, r, NOISES, 1, 0, None, None, True, True) if hybrid
               else upd.cov_zupt_frame(leg, N, r, NOISES, None, None, True, True))
        out.append((got, _state(upd)))
    assert np.array_equal(out[0][0]['dx'], out[1][0]['dx']) and out[0][0]['n_after'] == out[1][0]['n_after'] == b - 6
    _same(out[0][1], out[1][1], 'F = 0')
    assert out[1][1][1]['fac_valid'] == 1


@pytest.mark.parametrize('name', ['edge65', 'grid64'])
@pytest.mark.parametrize('what', ['nan below b', 'indefinite M', 'nan behind b'])
def test_device_refusals_and_what_leaves_with_the_features(upd, name, what):
    """The ordinary refusal path: a NaN in one of the 15 rows at a column < b, or an indefinite M, refuse the frame -- P and the factor
    state bit for bit the prior's at dimension n, no feature gone, nothing marginalised.  A NaN only at columns >= b of those rows
    leaves with the features: applied, as the separate calls apply it."""
    leg, N, d, F, b, n = zh.dims(name)
    P = zh.prior(name, 0)
    if what == 'nan below b':
        P[4, b - 1] = np.nan      # (a column only the last kept tile's workgroups hold: every workgroup must still refuse)
    elif what == 'indefinite M':
        P[3:6, 3:6] = -np.eye(3)
    else:
        P[3, b] = np.nan          # one of the 15 rows, a column that leaves with the features: the separate calls never see it
        P[b - 2, n - 1] = np.nan
    r = zh.residual(3)
    upd.set_extra_states(d * F)
    upd.cov_set(P)
    ref = _state(upd)
    got = upd.cov_zupt_frame_hybrid(leg, N, r, NOISES, d, F, None, None, False, True, raise_on_refusal=False)
    if what == 'nan behind b':
        upd.set_extra_states(0)
        fused = _state(upd)
        upd.set_extra_states(d * F)
        upd.cov_set(P)
        sep = _separate(upd, leg, N, d, F, r, None, None, 0, 1)
        assert got['rc'] == 0 and got['applied'] == sep['applied'] == 1 and got['n_after'] == sep['n_after'] == b - 6
        assert np.array_equal(got['dx'], sep['dx'])
        _same(fused, _state(upd), what)
        assert np.isfinite(fused[0]).all()
    else:
        assert (got['rc'], got['applied'], got['n_after']) == (NOT_SPD, 0, n) and not got['dx'].any()
        _same(_state(upd), ref, what)
        with pytest.raises(capi.MsckfError) as e:
            upd.cov_zupt_frame_hybrid(leg, N, r, NOISES, d, F, None, None, False, True)
        assert e.value.code == NOT_SPD
        _same(_state(upd), ref, what)
    upd.set_extra_states(0)


def _unchanged(u, ref, what):
    _same(_state(u), ref, what)


def test_validation_failures_leave_everything_as_it_was(upd):
    leg, N, d, F, b, n = zh.dims('feat3d')
    _make_resident(upd, zh.prior('feat3d', 1), leg, d * F)
    ref = _state(upd)
    assert ref[1]['fac_valid'] == 1
    r = zh.residual(1)
    Phi, Q = zh.frame_inputs(leg, 2)
    base = dict(leg_dim=leg, n_clones=N, r=r, noises=NOISES, idp_dim=d, n_feature_states=F, Phi=Phi, Q=Q, augment=True, remove_previous=True)
    bad = {
        'dimension': dict(n_clones=N + 1),
        'F too small': dict(n_feature_states=F - 1),
        'd F != extra states': dict(idp_dim=1, n_feature_states=F),
        'idp_dim 2': dict(idp_dim=2),
        'F < 0': dict(n_feature_states=-1),
        'leg_dim': dict(leg_dim=23),
        'one clone': dict(n_clones=1),
        'zero variance': dict(noises=(1e-4, 0.0, 1e-3)),
        'non-finite r': dict(r=np.where(np.arange(9) == 7, np.inf, r)),
        'Phi without Q': dict(Q=None),
    }
    for what, kw in bad.items():
        with pytest.raises(capi.MsckfError) as e:
            upd.cov_zupt_frame_hybrid(**dict(base, **kw))
        assert e.value.code == INVALID, what
        _unchanged(upd, ref, what)
    upd.set_extra_states(d * F - 1)   # the option and the call disagree although the call matches the covariance
    with pytest.raises(capi.MsckfError) as e:
        upd.cov_zupt_frame_hybrid(**base)
    assert e.value.code == INVALID
    upd.set_extra_states(d * F + 6)   # nuisance states declared
    upd.set_schmidt_states(1)
    try:
        with pytest.raises(capi.MsckfError) as e:
            upd.cov_zupt_frame_hybrid(**base)
        assert e.value.code == INVALID
    finally:
        upd.set_schmidt_states(0)
        upd.set_extra_states(d * F)
    _unchanged(upd, ref, 'options')
    f = upd._zupt_hybrid_struct(leg, N, r, NOISES, d, F, None, None, True, True, [])
    dx = np.zeros(b)
    ap, na = C.c_int32(0), C.c_int32(0)
    call = upd.lib.orcvio_msckf_cov_zupt_frame_hybrid
    assert call(None, C.byref(f), capi._d(dx), C.byref(ap), C.byref(na)) == INVALID
    assert call(upd.h, None, capi._d(dx), C.byref(ap), C.byref(na)) == INVALID
    assert call(upd.h, C.byref(f), None, C.byref(ap), C.byref(na)) == INVALID
    assert call(upd.h, C.byref(f), capi._d(dx), None, C.byref(na)) == INVALID
    assert call(upd.h, C.byref(f), capi._d(dx), C.byref(ap), None) == INVALID
    _unchanged(upd, ref, 'null arguments')
    assert upd.cov_zupt_frame_hybrid(**dict(base, Phi=None, Q=None))['applied'] == 1   # ... and the frame itself is a valid one
    upd.set_extra_states(0)


def test_a_communicator_on_the_handle_is_refused(built):
    leg, N, d, F, b, n = zh.dims('min35')
    u = capi.MsckfUpdater(device=0, max_clones=8, max_features=64, max_observations=1024, debug_hooks=True)
    try:
        P = zh.prior('min35', 0)
        u.set_extra_states(d * F)
        u.cov_set(P)
        u.comm_init(capi.comm_unique_id(), 0, 1)
        with pytest.raises(capi.MsckfError) as e:
            u.cov_zupt_frame_hybrid(leg, N, zh.residual(3), NOISES, d, F, None, None, False, True)
        assert e.value.code == INVALID and np.array_equal(u.cov_get(), P)
        u.comm_destroy()
        assert u.cov_zupt_frame_hybrid(leg, N, zh.residual(3), NOISES, d, F, None, None, False, True)['applied'] == 1
    finally:
        u.close()


# ---- the checked call ---------------------------------------------------------------------------------------------------------------
def _handle():
    return capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096, debug_hooks=True)


def _imu_case(resid, seed, S=10):
    """an IMU case whose state and samples are a tests/zupt_check_cases.py sample set: resid scales the accelerometer's departure
    from rest (small: a parked platform, large: a moving one)"""
    c = ic.make_case('larvio', S, n=LEG, seed=seed, rate=200.0)
    z = zc.make_case(S, left=bool(c['cfg'].use_left), resid=resid, seed=seed)
    st = c['state']
    st.time, st.R, st.v, st.ba, st.bg = z['t_state'], z['R'].copy(), z['v'].copy(), z['ba'].copy(), np.zeros(3)
    c['fej'] = st.copy()
    c['cfg'].gravity = z['g'].copy()
    c['samples'] = z['samples'].copy()
    c['time_bound'] = float(z['samples'][-1, 0]) + 0.3 / 200.0
    c['prev'] = z['samples'][0, 1:7].copy()
    return c


def _arm(u, case):
    cfg, state, prev = ic.to_capi(case)
    u.io_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])
    return cfg, state


def _chk(case):
    return capi.MsckfUpdater.zupt_check(use_left=int(case['cfg'].use_left))   # the reference's constants


@pytest.mark.parametrize('name', ['edge65', 'feat3d'])
def test_an_accepted_checked_frame_equals_the_unchecked_hybrid_frame_bit_for_bit(built, name):
    leg, N, d, F, b, n = zh.dims(name)
    P0 = ic.make_cov(n - 6, np.random.default_rng(n))
    r = zh.residual(n)
    case = _imu_case(0.1, seed=61)
    a, c, u = _handle(), _handle(), _handle()
    try:
        for h in (a, c, u):
            h.set_extra_states(d * F)
            h.cov_set(P0)
        _arm(a, case)
        ga, verdict = a.cov_zupt_frame_checked_hybrid(_chk(case), leg, N, r, NOISES, d, F, True, True)
        # the unchecked hybrid frame on the Phi and Q the device made
        cfg, st, prev = ic.to_capi(case)
        info = u.cov_propagate_imu(cfg, st, prev, case['samples'], case['time_bound'], wait=True, want_PhiQ=True)
        u.cov_augment()
        ref = u.cov_zupt_check_imu(_chk(case), np.array(st.R_b2w[:]), np.array(st.v[:]), np.array(st.acc_bias[:]), case['cfg'].gravity, case['samples'])
        print('verdict', verdict)
        assert verdict == ref and (verdict['evaluated'], verdict['accept'], verdict['dof']) == (1, 1, 54)
        gc = c.cov_zupt_frame_hybrid(leg, N, r, NOISES, d, F, info['Phi'], info['Q'], True, True)
        assert ga['rc'] == 0 and ga['applied'] == gc['applied'] == 1 and ga['n_after'] == gc['n_after'] == b - 6
        assert np.array_equal(ga['dx'], gc['dx'])
        _same(_state(a), _state(c), 'checked against unchecked')
    finally:
        a.close(); c.close(); u.close()


def test_a_rejected_checked_frame_keeps_every_feature_and_the_moving_frame_follows(built):
    """the first moving frame of make_zupt_stream behind a check that rejects: P bit for bit io_propagate_imu + cov_augment, every
    feature resident, and the frame's io_step_frame_ex equal to the one behind the separate calls"""
    idp, nslam = 1, 12
    fl = synth.Flags(use_larvio=1)
    frames, P0 = synth.make_zupt_stream(fl, n_frames=1, n_slam=nslam, idp=idp)
    fr = frames[0]
    N = fr['w'].N
    n0 = P0.shape[0]
    assert fr['zupt'] is None and n0 == LEG + 6 * (N - 1) + idp * nslam
    r = zh.residual(5)
    case = _imu_case(30.0, seed=62)
    a, c = _handle(), _handle()
    try:
        for h in (a, c):
            h.set_extra_states(idp * nslam)
            h.set_ekf_rows_mode(True)
            h.cov_set(P0)
            h.cov_prefactor()
        _arm(a, case)
        ga, verdict = a.cov_zupt_frame_checked_hybrid(_chk(case), LEG, N, r, NOISES, idp, nslam, True, True)
        print('verdict', verdict)
        assert (ga['rc'], ga['applied'], ga['n_after']) == (0, 0, n0 + 6) and not ga['dx'].any() and ga['dx'].shape == (LEG + 6 * N,)
        assert (verdict['evaluated'], verdict['accept'], verdict['status'], verdict['dof']) == (1, 0, 0, 54)
        cfg, st, prev = ic.to_capi(case)
        c.cov_propagate_imu(cfg, st, prev, case['samples'], case['time_bound'])
        c.cov_augment()
        ref = c.cov_zupt_check_imu(_chk(case), np.array(st.R_b2w[:]), np.array(st.v[:]), np.array(st.acc_bias[:]), case['cfg'].gravity, case['samples'])
        assert verdict == ref
        _same(_state(a), _state(c), 'behind the rejection')
        assert a.cov_get().shape[0] == n0 + 6   # the F features are still resident
        with pytest.raises(capi.MsckfError) as e:   # the arming was consumed
            a.cov_zupt_frame_checked_hybrid(_chk(case), LEG, N, r, NOISES, idp, nslam, False, True)
        assert e.value.code == INVALID
        out = [h.io_step_frame_ex(fr['w'], None, None, False, fr['slam'], idp, fr['prune'], False, fr['remove']) for h in (a, c)]
        assert out[0]['rc'] == out[1]['rc'] == 0 and np.array_equal(out[0]['accept'], out[1]['accept'])
        assert np.array_equal(out[0]['dx'], out[1]['dx']) and np.array_equal(a.cov_get(), c.cov_get())
    finally:
        a.close(); c.close()


def test_checked_hybrid_refusals(built):
    leg, N, d, F, b, n = zh.dims('edge65')
    P0 = ic.make_cov(n - 6, np.random.default_rng(9))
    r = zh.residual(9)
    case = _imu_case(0.1, seed=63)
    a = _handle()
    try:
        a.set_extra_states(d * F)
        a.cov_set(P0)
        with pytest.raises(capi.MsckfError) as e:   # an unarmed handle
            a.cov_zupt_frame_checked_hybrid(_chk(case), leg, N, r, NOISES, d, F, True, True)
        assert e.value.code == INVALID and np.array_equal(a.cov_get(), P0)
        _arm(a, case)
        Phi, Q = zh.frame_inputs(leg, 1)
        with pytest.raises(capi.MsckfError) as e:   # an armed handle given Phi
            a.cov_zupt_frame_hybrid(leg, N, r, NOISES, d, F, Phi, Q, True, True)
        assert e.value.code == INVALID and np.array_equal(a.cov_get(), P0)
        for what, call in (('idp_dim', lambda: a.cov_zupt_frame_checked_hybrid(_chk(case), leg, N, r, NOISES, 2, F, True, True)),
                           ('F', lambda: a.cov_zupt_frame_checked_hybrid(_chk(case), leg, N, r, NOISES, d, F + 1, True, True)),
                           ('leg_dim 46', lambda: a.cov_zupt_frame_checked_hybrid(_chk(case), 46, N - 4, r, NOISES, d, F, True, True))):
            with pytest.raises(capi.MsckfError) as e:
                call()
            assert e.value.code == INVALID and np.array_equal(a.cov_get(), P0), what
        ga, verdict = a.cov_zupt_frame_checked_hybrid(_chk(case), leg, N, r, NOISES, d, F, True, True)   # the arming stood
        assert ga['applied'] == 1 and verdict['accept'] == 1 and ga['n_after'] == b - 6
        # a refused Phi of the armed propagation refuses the unchecked frame too: augmentation stands, every feature in place
        bad = ic.make_case('right_closed', 5, n=LEG, seed=53)
        bad['samples'][2, 1:4] = bad['state'].bg
        a.set_extra_states(d * F)
        a.cov_set(P0)
        _arm(a, bad)
        ga = a.cov_zupt_frame_hybrid(leg, N, r, NOISES, d, F, None, None, True, True, raise_on_refusal=False)
        assert (ga['rc'], ga['applied'], ga['n_after']) == (NOT_SPD, 0, n) and not ga['dx'].any()
        assert np.array_equal(a.cov_get(), mirror_cov.augment(P0, rest=d * F))
        # one selected sample: no check, no update, propagation and augmentation stand with every feature
        one = _imu_case(0.1, seed=64, S=1)
        a.cov_set(P0)
        _arm(a, one)
        ga, verdict = a.cov_zupt_frame_checked_hybrid(_chk(one), leg, N, r, NOISES, d, F, True, True)
        assert (ga['rc'], ga['applied'], ga['n_after'], verdict['evaluated']) == (0, 0, n, 0) and not ga['dx'].any()
    finally:
        a.close()


# ---- a handle's history -------------------------------------------------------------------------------------------------------------
def test_moving_then_stationary_hybrid_then_moving(built):
    """make_zupt_stream's first frames on ONE resident covariance: moving frames through io_step_frame with the in-state features'
    rows, the first stationary frame through the hybrid call -- every feature leaves --, ORCVIO_OPT_EXTRA_STATES = 0, the parked
    frames behind it with F = 0, then a moving frame of a filter without in-state features; every update against the host chain
    within tests/test_gpu_zupt.py's loop bar, 1e-9."""
    idp, nslam = 1, 12
    fl = synth.Flags(use_larvio=1)
    frames, P0 = synth.make_zupt_stream(fl, n_frames=9, n_slam=nslam, idp=idp, propagate_stationary=True)
    table = mirror.chi2_table(fl.chi2_prob)
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096, debug_hooks=True)
    try:
        u.set_extra_states(idp * nslam)
        u.set_ekf_rows_mode(True)
        u.cov_set(P0)
        P, F, seen = P0, nslam, ''
        for it, fr in enumerate(frames):
            if fr['zupt'] is None:
                assert F == nslam
                got = u.io_step_frame(fr['w'], fr['Phi'], fr['Q'], True, fr['slam'], idp, fr['prune'], False, fr['remove'])
                ref = mirror_frame.step_frame(P, fr, idp, 0, table=table)
                assert got['rc'] == 0 and np.array_equal(got['accept'], ref['accept']), it
                assert rel(got['dx'], ref['dx']) < 1e-9, it
                P = ref['P']
                seen += 'm'
            else:
                z = fr['zupt']
                got = u.cov_zupt_frame_hybrid(fl.leg_dim, z['n_clones'], z['r'], z['noises'], idp, F, fr['Phi'], fr['Q'], True, fr['remove_previous'])
                ref = zh.hybrid_frame(P, fl.leg_dim, z['n_clones'], idp, F, z['r'], z['noises'], fr['Phi'], fr['Q'], True, fr['remove_previous'])
                assert got['applied'] == 1 and got['dx'].shape == ref['dx'].shape and rel(got['dx'], ref['dx']) < 1e-9, it
                P, F = ref['P'], 0
                u.set_extra_states(0)   # the caller's, by the convention of cov_remove_features
                seen += 's'
            Pg = u.cov_get()
            assert got['n_after'] == P.shape[0] == Pg.shape[0], it
            assert rel(Pg, P) < 1e-9, (it, rel(Pg, P))
        assert seen == 'mmmssssss', seen
        # the platform moves again: no in-state feature is left
        N = (P.shape[0] - fl.leg_dim) // 6 + 1
        w = synth.make_window(N=N, F=30, seed=77, track_len=(3, 6), flags=fl)
        Phi, Q = zh.frame_inputs(fl.leg_dim, 78)
        u.set_ekf_rows_mode(False)
        got = u.io_step_frame(w, Phi, Q, True, None, idp, None, False, [])
        ref = mirror_frame.step_frame(P, dict(w=w, slam=[], prune=None, Phi=Phi, Q=Q, remove=[]), idp, 0, table=table)
        assert got['rc'] == 0 and np.array_equal(got['accept'], ref['accept'])
        assert rel(got['dx'], ref['dx']) < 1e-9 and rel(u.cov_get(), ref['P']) < 1e-9
    finally:
        u.close()


@pytest.mark.parametrize('d,route', [(1, 'marginalised'), (3, 'augmented')])
def test_entering_features_then_stationary_hybrid_then_moving(built, d, route):
    """A moving hybrid frame whose update brings SIX features into the state beside the four already there
    (tests/entering_cases.py, committed with orcvio_msckf_cov_commit_new_features_fac: the factor widened to kf + d k columns,
    kf = n + 6 or n - 6, tail 0), then the stationary hybrid frame with F taken from that commit and NO propagation -- the widened
    factor meets k_zupt_fac_keep --, then ORCVIO_OPT_EXTRA_STATES = 0 and a moving frame's update on the kept factor.  Every step
    against the host chain (oracle/mirror_hybrid.hybrid_update_full, tests/zupt_hybrid_cases.py, oracle/mirror.py) within
    tests/test_gpu_zupt.py's loop bar, 1e-9; the stationary frame also bit for bit against the separate calls on a twin handle."""
    import dataclasses
    import entering_cases as ec
    from oracle import mirror_hybrid as mh
    from test_gpu_entering_factor import _new, options, prepare, stage_and_run
    case = ec.make_case(ec.CaseId('small', d, 6))
    w = case.win
    leg, N, n, sz = w.flags.leg_dim, w.N, w.n, d * 6
    r = zh.residual(40 + d)
    a, t = _new(), _new()
    try:
        out = []
        for u in (a, t):
            with options(u, case):
                st0 = prepare(u, case, route)
                P_res = u.cov_get()
                got = stage_and_run(u, case)
                dx_new = u.cov_commit_new_features_fac()
            st = capi.debug_factor_state(u)
            kf = st0['fac_k']
            assert kf == (n + 6 if route == 'marginalised' else n - 6)
            assert st == dict(fac_valid=1, fac_n=n + sz, fac_k=kf + sz, res_n=n + sz), st
            out.append((got, dx_new, u.cov_get()))
        # the moving frame with entering features against the literal restatement of the whole hybrid update
        full = mh.hybrid_update_full(dataclasses.replace(w, P=P_res), case.slam, case.new, d)
        assert full['new_accept'] == list(range(6))
        got, dx_new, P_aug = out[0]
        assert np.array_equal(got['accept'], full['accept'])
        assert rel(np.concatenate([got['dx'], dx_new]), full['dx']) < 1e-9 and rel(P_aug, full['P_new']) < 1e-9
        assert np.array_equal(P_aug, out[1][2])
        F = (capi.debug_factor_state(a)['res_n'] - leg - 6 * N) // d   # from that commit: the four that were there and the six that entered
        assert F == 10
        # the stationary frame: fused on a, the separate calls on t
        a.set_extra_states(d * F)
        ga = a.cov_zupt_frame_hybrid(leg, N + 1, r, NOISES, d, F, None, None, True, True)
        a.set_extra_states(0)
        t.set_extra_states(d * F)
        gt = _separate(t, leg, N + 1, d, F, r, None, None, 1, 1)
        sa, stw = _state(a), _state(t)
        b = leg + 6 * (N + 1)
        assert ga['applied'] == gt['applied'] == 1 and ga['n_after'] == gt['n_after'] == b - 6
        assert np.array_equal(ga['dx'], gt['dx'])
        _same(sa, stw, 'fused against separate behind entering features')
        assert sa[1] == dict(fac_valid=1, fac_n=b - 6, fac_k=kf + sz, res_n=b - 6), sa[1]
        ref = zh.hybrid_frame(full['P_new'], leg, N + 1, d, F, r, NOISES, None, None, True, True)
        e = (rel(ga['dx'], ref['dx']), rel(sa[0], ref['P']), rel(sa[2] @ sa[2].T, sa[0]))
        print('stationary frame behind entering features (d = %d, %s): dx %.2e, P %.2e, S S^T %.2e' % ((d, route) + e))
        assert max(e) < 1e-9 and np.array_equal(sa[0], sa[0].T)
        # the platform moves again without in-state features: the update reads the factor k_zupt_fac_keep wrote
        w2 = synth.make_window(N=N, F=40, seed=50 + d, track_len=(3, min(N, 12)), flags=synth.Flags(leg_dim=leg))
        w2 = dataclasses.replace(w2, P=np.ascontiguousarray(ref['P']), n_extra=0)
        got2 = a.update_features(w2, resident_cov=True, want_P=True)
        ref2 = mirror.msckf_update(w2)
        assert got2['updated'] and np.array_equal(got2['accept'], ref2['accept'])
        assert rel(got2['dx'], ref2['dx']) < 1e-9 and rel(got2['P_new'], ref2['P_new']) < 1e-9
    finally:
        a.close(); t.close()


def test_a_refusal_with_a_resident_factor_leaves_both_bit_for_bit(upd):
    """The one refusal a prior WITH a Cholesky factor can meet: P is positive definite, but the position variances of the two newest
    clones are so large that their sum in M = H P H^T + R is not finite.  The ordinary refusal path (NOT_SPD), with the factor
    resident: k_zupt_fac_keep takes its copy form, no buffer changes roles, P, the factor's state and its bits are the prior's."""
    leg, N, d, F, b, n = zh.dims('edge65')
    A = np.random.default_rng(n).standard_normal((n, n)) / np.sqrt(n)
    C_ = np.eye(n) + 0.05 * (A @ A.T)
    P = np.ascontiguousarray(0.5 * (C_ + C_.T) / C_.max() * 1.2e308)   # every entry finite, every variance close to 1.2e308
    assert np.isfinite(P).all() and np.isfinite(np.linalg.cholesky(P)).all() and not np.isfinite(P[b - 1, b - 1] + P[b - 7, b - 7])
    r = zh.residual(8)
    upd.set_extra_states(d * F)
    upd.cov_set(P)
    upd.cov_prefactor()
    ref = _state(upd)
    assert ref[1]['fac_valid'] == 1 and ref[1]['fac_n'] == n
    try:
        got = upd.cov_zupt_frame_hybrid(leg, N, r, NOISES, d, F, None, None, False, True, raise_on_refusal=False)
        assert (got['rc'], got['applied'], got['n_after']) == (NOT_SPD, 0, n) and not got['dx'].any()
        _same(_state(upd), ref, 'refused with a factor')
    finally:
        upd.set_extra_states(0)
