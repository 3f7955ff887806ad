"""Zero-velocity detection from IMU samples on the GPU (k_zupt_check): orcvio_msckf_cov_zupt_check_imu against the reference's dense
form (tests/mirror_zupt_check.py) at the kernel's edge shapes, its refusals and validation, the covariance and its factor untouched;
orcvio_msckf_cov_propagate_imu_checked and orcvio_msckf_cov_zupt_frame_checked bit for bit against the separate calls.

The bar on chi^2 is zupt_check_cases.CHI2_BAR: ten times the dense form's own distance from 60-digit arithmetic over the same cases
(tests/test_zupt_check_mirror.py measures it), floored at 1e-12."""
import ctypes as C

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror_frame
import imu_cases as ic
import mirror_imu as mi
import mirror_zupt_check as mz
import zupt_check_cases as zc

pytestmark = pytest.mark.gpu
LEG = 22
NOT_SPD, INVALID, CAPACITY = 6, 1, 3


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=21, max_features=16, max_observations=256, debug_hooks=True)
    yield u
    u.close()


def chk_of(case, **over):
    c = case['consts']
    kw = dict(sigma_w2=c['sigma_w2'], sigma_a2=c['sigma_a2'], sigma_wb=c['sigma_wb'], sigma_ab=c['sigma_ab'], chi2_prob=c['chi2_prob'],
              chi2_multiplier=c['chi2_multiplier'], max_velocity=c['max_velocity'])
    kw.update(over)
    return capi.MsckfUpdater.zupt_check(use_left=int(case['left']), **kw)


def run(upd, case, raise_on_refusal=True, **over):
    return upd.cov_zupt_check_imu(chk_of(case, **over), case['R'], case['v'], case['ba'], case['g'], case['samples'], raise_on_refusal=raise_on_refusal)


_dense = {}


def dense_of(name):
    if name not in _dense:
        _dense[name] = mz.dense(zc.case(name))
    return _dense[name]


@pytest.mark.parametrize('name', zc.names())
def test_chi2_and_the_accept_bit_against_the_dense_form(upd, name):
    case = zc.case(name)
    ref, dof = dense_of(name)
    upd.set_extra_states(12 if case['n'] == 154 else 0)
    upd.cov_set(case['P'])
    got = run(upd, case)
    err = abs(got['chi2'] - ref) / ref
    print('%-20s S %3d n %3d: chi2 %.10g dense %.10g  |device - dense| / dense %.2e (bar %.1e)' % (name, case['S'], case['n'], got['chi2'], ref, err, zc.CHI2_BAR))
    assert (got['rc'], got['evaluated'], got['status'], got['dof']) == (0, 1, 0, dof)
    thr = mz.threshold(case, dof)
    assert abs(got['chi2_check'] - thr) / thr < 1e-12
    assert got['speed'] == float(np.sqrt(case['v'][0] ** 2 + case['v'][1] ** 2 + case['v'][2] ** 2))
    assert err <= zc.CHI2_BAR
    assert got['accept'] == int(mz.decide(case, ref, dof))   # (every case is at least 1e-6 from its threshold: test_zupt_check_mirror.py)
    assert np.array_equal(upd.cov_get(), case['P'])


def test_the_decision_pairs_differ_in_the_accept_bit_alone(upd):
    for base in zc.PAIRS:
        got = []
        for side in ('_below', '_above'):
            case = zc.case(base + side)
            upd.set_extra_states(0)
            upd.cov_set(case['P'])
            got.append(run(upd, case))
        assert (got[0]['accept'], got[1]['accept']) == (1, 0) and got[0]['evaluated'] == got[1]['evaluated'] == 1, base
    a, b = zc.case('speed_below'), zc.case('speed_above')
    upd.cov_set(a['P'])
    ga, gb = run(upd, a), run(upd, b)
    assert (ga['accept'], gb['accept']) == (1, 0) and ga['chi2'] == gb['chi2'] and gb['evaluated'] == 1 and gb['chi2'] < gb['chi2_check']
    # the multiplier scales the threshold the device compares with
    case = zc.case('pair_S3_above')
    upd.cov_set(case['P'])
    assert run(upd, case, chi2_multiplier=1.05)['accept'] == 1 and run(upd, case, chi2_multiplier=1.0)['accept'] == 0


def test_sample_counts_without_a_launch_and_beyond_the_capacity(upd):
    case = zc.case('S5_right')
    upd.cov_set(case['P'])
    for S in (0, 1):
        got = run(upd, dict(case, samples=case['samples'][:S]))
        assert (got['rc'], got['evaluated'], got['accept'], got['dof'], got['chi2']) == (0, 0, 0, 0, 0.0)
    big = zc.make_case(129, seed=1)
    with pytest.raises(capi.MsckfError) as e:
        run(upd, dict(big, P=case['P']))
    assert e.value.code == CAPACITY
    assert np.array_equal(upd.cov_get(), case['P'])


def test_the_same_input_twice_gives_the_same_bits(upd):
    for name in ('S65_left', 'n154_S128', 'S3_right'):
        case = zc.case(name)
        upd.cov_set(case['P'])
        assert run(upd, case) == run(upd, case)


def test_both_triangles_of_the_marginal_are_read_and_averaged(upd):
    case = zc.case('S5_right')
    P = case['P'].copy()
    P[0, 12] *= 1.0 + 1e-3
    P[1, 9] += 1e-6
    upd.cov_set(P)
    both = run(upd, case)
    upd.cov_set(0.5 * (P + P.T))
    assert run(upd, case) == both
    for tri in (np.triu, np.tril):
        upd.cov_set(tri(P) + tri(P, 0).T - np.diag(np.diag(P)))
        one = run(upd, case)
        assert abs(one['chi2'] - both['chi2']) / both['chi2'] > 100 * zc.CHI2_BAR


def _state(upd):
    st = capi.debug_factor_state(upd)
    return upd.cov_get(), st, capi.debug_factor(upd) if st['fac_valid'] else None


def _unchanged(upd, ref, what):
    P, st, S = _state(upd)
    assert np.array_equal(P, ref[0], equal_nan=True), what
    assert st == ref[1], what
    assert (S is None) == (ref[2] is None) and (S is None or np.array_equal(S, ref[2])), what


def test_the_covariance_and_its_factor_are_untouched(upd):
    case = zc.case('n142_S65')
    upd.set_extra_states(0)
    upd.cov_set(ic.make_cov(142, np.random.default_rng(3)))
    upd.cov_prefactor()
    ref = _state(upd)
    assert ref[1]['fac_valid'] == 1
    got = run(upd, case)
    assert got['evaluated'] == 1
    _unchanged(upd, ref, 'with a factor')
    upd.cov_set(case['P'])   # ... and without one
    ref = _state(upd)
    assert ref[1]['fac_valid'] == 0
    run(upd, case)
    _unchanged(upd, ref, 'without a factor')


def test_device_refusals(upd):
    case = zc.case('S5_left')
    for what in ('nan in the marginal', 'nan in its lower triangle', 'negative diagonal', 'indefinite', 'nan elsewhere'):
        P = case['P'].copy()
        if what == 'nan in the marginal':
            P[1, 13] = np.nan
        elif what == 'nan in its lower triangle':
            P[14, 0] = np.inf
        elif what == 'negative diagonal':
            P[10, 10] = -P[10, 10]
        elif what == 'indefinite':
            P[0, 1] = P[1, 0] = 1.0
        else:
            P[3:9, :] = np.nan; P[:, 3:9] = np.nan; P[15:, :] = np.nan; P[:, 15:] = np.nan   # every entry the check does not read
        if what == 'nan elsewhere':
            upd.cov_set(case['P'])
            good = run(upd, case)
        upd.cov_set(P)
        got = run(upd, case, raise_on_refusal=False)
        if what == 'nan elsewhere':
            assert got == good and got['evaluated'] == 1, what
        else:
            assert (got['rc'], got['evaluated'], got['accept'], got['status'], got['chi2']) == (NOT_SPD, 0, 0, NOT_SPD, 0.0), what
            with pytest.raises(capi.MsckfError) as e:
                run(upd, case)
            assert e.value.code == NOT_SPD
        assert np.array_equal(upd.cov_get(), P, equal_nan=True), what


def test_validation_failures_leave_everything_as_it_was(upd):
    case = zc.case('S5_right')
    upd.cov_set(case['P'])
    upd.cov_prefactor()
    ref = _state(upd)
    smp = case['samples']
    dt0 = smp.copy(); dt0[3, 0] = dt0[2, 0]
    dtneg = smp.copy(); dtneg[3, 0] = dtneg[2, 0] - 1e-3
    nan_smp = smp.copy(); nan_smp[1, 5] = np.nan
    inf_t = smp.copy(); inf_t[4, 0] = np.inf
    bad_cases = {
        'dt = 0': dict(samples=dt0), 'dt < 0': dict(samples=dtneg), 'non-finite sample': dict(samples=nan_smp), 'non-finite stamp': dict(samples=inf_t),
        'non-finite R': dict(R=case['R'] * np.nan), 'non-finite v': dict(v=np.array([0.0, np.inf, 0.0])),
        'non-finite bias': dict(ba=np.array([np.nan, 0.0, 0.0])), 'non-finite gravity': dict(g=np.array([0.0, 0.0, np.nan])),
    }
    for what, kw in bad_cases.items():
        with pytest.raises(capi.MsckfError) as e:
            run(upd, dict(case, **kw))
        assert e.value.code == INVALID, what
        _unchanged(upd, ref, what)
    bad_consts = {
        'sigma_w2 = 0': dict(sigma_w2=0.0), 'sigma_a2 < 0': dict(sigma_a2=-1e-6), 'sigma_wb = 0': dict(sigma_wb=0.0), 'sigma_ab nan': dict(sigma_ab=np.nan),
        'max_velocity = 0': dict(max_velocity=0.0), 'max_velocity inf': dict(max_velocity=np.inf), 'chi2_prob = 0': dict(chi2_prob=0.0),
        'chi2_prob = 1': dict(chi2_prob=1.0), 'chi2_prob nan': dict(chi2_prob=np.nan), 'multiplier = 0': dict(chi2_multiplier=0.0),
    }
    for what, kw in bad_consts.items():
        with pytest.raises(capi.MsckfError) as e:
            run(upd, case, **kw)
        assert e.value.code == INVALID, what
        with pytest.raises(capi.MsckfError) as e:   # (also where nothing would be launched)
            run(upd, dict(case, samples=smp[:1]), **kw)
        assert e.value.code == INVALID, what
        _unchanged(upd, ref, what)
    # null arguments
    chk = chk_of(case)
    out = capi.ZuptVerdict()
    arr = [np.ascontiguousarray(x, dtype=np.float64) for x in (case['R'].ravel(), case['v'], case['ba'], case['g'], smp)]
    args = [upd.h, C.byref(chk)] + [capi._d(a) for a in arr] + [smp.shape[0], C.byref(out)]
    for k in (0, 1, 2, 3, 4, 5, 6, 8):
        a = list(args)
        a[k] = None
        assert upd.lib.orcvio_msckf_cov_zupt_check_imu(*a) == INVALID, k
    _unchanged(upd, ref, 'null arguments')
    # no resident covariance
    u = capi.MsckfUpdater(device=0, max_clones=2, max_features=16, max_observations=256)
    try:
        with pytest.raises(capi.MsckfError) as e:
            run(u, case)
        assert e.value.code == INVALID
        # a communicator on the handle
        u.cov_set(case['P'])
        u.comm_init(capi.comm_unique_id(), 0, 1)
        with pytest.raises(capi.MsckfError) as e:
            run(u, case)
        assert e.value.code == INVALID
        u.comm_destroy()
        assert run(u, case)['evaluated'] == 1
    finally:
        u.close()


# ---- behind the propagation from raw samples ---------------------------------------------------------------------------------------
def _selected(case):
    """the samples the host half selects: gpu_case puts one at state.time in front (skipped) and two beyond the cut"""
    return case['samples'][1:1 + case['S']]


def _loose(case, **over):
    """constants under which an imu_cases platform (moving, |v| ~ 0.5) passes: the decision is not what these tests are about"""
    kw = dict(chi2_multiplier=1e12, max_velocity=1e3)
    kw.update(over)
    return capi.MsckfUpdater.zupt_check(use_left=int(case['cfg'].use_left), **kw)


@pytest.mark.parametrize('fs,S,n', [('larvio', 10, 142), ('left_closed', 2, 28), ('right_euler', 128, 145), ('larvio', 1, 28), ('larvio', 0, 28)])
def test_checked_propagation_equals_propagation_plus_the_stand_alone_check_bit_for_bit(upd, fs, S, n):
    case = ic.gpu_case(fs, S, n) if S else ic.make_case(fs, 0, n=n, seed=8, skipped=3)
    upd.set_extra_states(3 if n == 145 else 0)
    chk = _loose(case, chi2_multiplier=1.0)
    # the separate calls
    cfg, state, prev = ic.to_capi(case)
    upd.cov_set(case['P'])
    ref_info = upd.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'], wait=True, want_PhiQ=True)
    ref_P = upd.cov_get()
    ref_v = upd.cov_zupt_check_imu(chk, np.array(state.R_b2w[:]), np.array(state.v[:]), np.array(state.acc_bias[:]), case['cfg'].gravity,
                                   _selected(case) if S else np.zeros((0, 7)))
    # the checked call
    cfg2, state2, prev2 = ic.to_capi(case)
    upd.cov_set(case['P'])
    info, verdict = upd.cov_propagate_imu_checked(cfg2, state2, prev2, case['samples'], case['time_bound'], chk, want_PhiQ=True)
    assert verdict == ref_v and verdict['evaluated'] == (1 if S >= 2 else 0) and verdict['dof'] == (6 * (S - 1) if S >= 2 else 0)
    assert np.array_equal(upd.cov_get(), ref_P)
    for k in ('status', 'n_used', 'n_propagated', 'dt', 'applied'):
        assert info[k] == ref_info[k], k
    assert np.array_equal(info['Phi'], ref_info['Phi']) and np.array_equal(info['Q'], ref_info['Q']) and np.array_equal(prev, prev2)
    assert bytes(state) == bytes(state2)
    if S >= 2:   # ... and the number itself against the dense form on the covariance the device propagated
        c = dict(P=ref_P, R=np.array(state.R_b2w[:]).reshape(3, 3), ba=np.array(state.acc_bias[:]), g=case['cfg'].gravity, v=np.array(state.v[:]),
                 samples=_selected(case), left=bool(case['cfg'].use_left), consts=mz.CONSTS)
        d, dof = mz.dense(c)
        assert dof == verdict['dof'] and abs(verdict['chi2'] - d) / d <= zc.CHI2_BAR


def test_checked_propagation_with_a_refused_phi_and_its_validation(upd):
    case = ic.make_case('right_closed', 5, n=28, seed=9)
    case['samples'][2, 1:4] = case['state'].bg   # a zero unbiased gyro sample: the right closed form divides by |w|^2
    upd.set_extra_states(0)
    cfg, state, prev = ic.to_capi(case)
    upd.cov_set(case['P'])
    info, verdict = upd.cov_propagate_imu_checked(cfg, state, prev, case['samples'], case['time_bound'], _loose(case), want_PhiQ=True, raise_on_refusal=False)
    assert info['status'] == NOT_SPD and info['applied'] == 0 and not np.isfinite(info['Phi']).all()
    assert (verdict['evaluated'], verdict['accept'], verdict['status']) == (0, 0, NOT_SPD)
    assert np.array_equal(upd.cov_get(), case['P'])
    # validation: nothing done, the state and the carried measurement untouched
    good = ic.gpu_case('larvio', 5, 28)
    upd.cov_set(good['P'])
    nan_smp = good['samples'].copy(); nan_smp[3, 6] = np.nan
    for what, kw, smp in (('a constant', dict(sigma_a2=0.0), good['samples']), ('chi2_prob', dict(chi2_prob=1.5), good['samples']), ('a sample', {}, nan_smp)):
        cfg, state, prev = ic.to_capi(good)
        with pytest.raises(capi.MsckfError) as e:
            upd.cov_propagate_imu_checked(cfg, state, prev, smp, good['time_bound'], _loose(good, **kw))
        assert e.value.code == INVALID, what
        assert state.time == good['state'].time and np.array_equal(prev, good['prev']) and np.array_equal(upd.cov_get(), good['P']), what
    cfg, state, prev = ic.to_capi(good)
    cfg46 = capi.MsckfUpdater.imu_config(46)
    with pytest.raises(capi.MsckfError) as e:
        upd.cov_propagate_imu_checked(cfg46, state, prev, good['samples'], good['time_bound'], _loose(good))
    assert e.value.code == INVALID
    big = ic.make_case('larvio', 129, n=28, seed=4, rate=650.0)
    cfg, state, prev = ic.to_capi(big)
    with pytest.raises(capi.MsckfError) as e:
        upd.cov_propagate_imu_checked(cfg, state, prev, big['samples'], big['time_bound'], _loose(big))
    assert e.value.code == CAPACITY and np.array_equal(upd.cov_get(), good['P'])


# ---- inside the stationary frame --------------------------------------------------------------------------------------------------
def _handle():
    return capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096, debug_hooks=True)


def _arm(u, case):
    cfg, state, prev = ic.to_capi(case)
    u.io_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])
    return state


@pytest.mark.parametrize('prefactor', [False, True])
def test_an_accepted_checked_frame_equals_the_armed_frame_bit_for_bit(built, prefactor):
    N = 6   # the window the update sees
    rng = np.random.default_rng(71)
    P0 = ic.make_cov(LEG + 6 * (N - 1), rng)
    r = 1e-3 * rng.standard_normal(9)
    case = ic.make_case('larvio', 10, n=LEG, seed=72, rate=200.0)
    a, b = _handle(), _handle()
    try:
        a.cov_set(P0); b.cov_set(P0)
        if prefactor:
            a.cov_prefactor(); b.cov_prefactor()
        state = _arm(a, case)
        _arm(b, case)
        ga, verdict = a.cov_zupt_frame_checked(_loose(case), LEG, N, r, synth.ZUPT_NOISES, True, True)
        gb = b.cov_zupt_frame(LEG, N, r, synth.ZUPT_NOISES, None, None, True, True)
        assert (verdict['evaluated'], verdict['accept'], verdict['dof']) == (1, 1, 54)
        assert ga['rc'] == 0 and ga['applied'] == gb['applied'] == 1 and ga['n_after'] == gb['n_after'] == LEG + 6 * (N - 1)
        assert np.array_equal(ga['dx'], gb['dx'])
        Pa, sa, Sa = _state(a)
        Pb, sb, Sb = _state(b)
        assert np.array_equal(Pa, Pb) and sa == sb and (Sa is None) == (Sb is None) and (Sa is None or np.array_equal(Sa, Sb))
        # the verdict is the stand-alone call's on the propagated, augmented covariance
        c = ic.make_case('larvio', 10, n=LEG, seed=72, rate=200.0)
        u = _handle()
        try:
            cfg, st2, prev = ic.to_capi(c)
            u.cov_set(P0)
            u.cov_propagate_imu(cfg, st2, prev, c['samples'], c['time_bound'])
            u.cov_augment()
            ref = u.cov_zupt_check_imu(_loose(case), np.array(st2.R_b2w[:]), np.array(st2.v[:]), np.array(st2.acc_bias[:]), c['cfg'].gravity, c['samples'])
        finally:
            u.close()
        assert verdict == ref and bytes(state) == bytes(st2)
    finally:
        a.close(); b.close()


def test_a_rejected_checked_frame_leaves_propagation_and_augmentation_and_the_moving_frame_follows(built):
    fl = synth.Flags(use_larvio=1)
    w = synth.make_window(N=8, F=6, seed=3, track_len=(5, 8), flags=fl)
    P0 = np.ascontiguousarray(synth.make_window(N=7, F=1, seed=5, flags=fl).P)
    prune = synth.subset_tracks(w, [0, 1], min_obs=2)
    remove = [0, 1]
    r = 1e-3 * np.random.default_rng(5).standard_normal(9)
    case = ic.make_case('larvio', 10, n=LEG, seed=52, rate=200.0, skipped=1, beyond=2)
    chk = capi.MsckfUpdater.zupt_check(use_left=0)   # the reference's constants: this platform moves
    a, b = _handle(), _handle()
    try:
        a.cov_set(P0); b.cov_set(P0)
        a.cov_prefactor(); b.cov_prefactor()
        _arm(a, case)
        ga, verdict = a.cov_zupt_frame_checked(chk, LEG, 8, r, synth.ZUPT_NOISES, True, True)
        assert (ga['rc'], ga['applied'], ga['n_after']) == (0, 0, LEG + 6 * 8) and not ga['dx'].any()
        assert (verdict['evaluated'], verdict['accept'], verdict['status'], verdict['dof']) == (1, 0, 0, 54) and verdict['chi2'] > verdict['chi2_check']
        # b: the separate calls
        cfg, state, prev = ic.to_capi(case)
        b.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])
        b.cov_augment()
        ref = b.cov_zupt_check_imu(chk, np.array(state.R_b2w[:]), np.array(state.v[:]), np.array(state.acc_bias[:]), case['cfg'].gravity, _selected(dict(case, S=10)))
        assert verdict == ref
        assert np.array_equal(a.cov_get(), b.cov_get())
        assert capi.debug_factor_state(a)['fac_valid'] == 0   # (propagation dropped it, as cov_propagate does)
        # the arming was consumed; the moving frame goes on without propagation and augmentation
        with pytest.raises(capi.MsckfError) as e:
            a.cov_zupt_frame_checked(chk, LEG, 8, r, synth.ZUPT_NOISES, False, True)
        assert e.value.code == INVALID
        got = a.io_step_frame(w, None, None, False, None, 1, prune, False, remove)
        srv, _ = ic.run_mirror(case, with_P=False)
        Phi, Q = mi.accumulate_sequential(srv.steps)
        oracle = mirror_frame.step_frame(P0, dict(w=w, slam=[], prune=prune, Phi=Phi, Q=0.5 * (Q + Q.T), remove=remove), 1, False)
        rel = lambda x, y: float(np.linalg.norm(x - y) / np.linalg.norm(y))
        figs = (rel(got['dx'], oracle['dx']), rel(got['prune_dx'], oracle['prune_dx']), rel(a.cov_get(), oracle['P']))
        print('moving frame behind a rejected check against the oracle chain: dx %.2e, prune dx %.2e, P %.2e' % figs)
        assert np.array_equal(got['accept'], oracle['accept']) and got['n_after'] == oracle['n_after'] and max(figs) < 1e-6
    finally:
        a.close(); b.close()


def test_checked_frame_refusals_and_validation(built):
    N = 6
    rng = np.random.default_rng(73)
    P0 = ic.make_cov(LEG + 6 * (N - 1), rng)
    r = 1e-3 * rng.standard_normal(9)
    case = ic.make_case('larvio', 10, n=LEG, seed=74, rate=200.0)
    a, b = _handle(), _handle()
    try:
        a.cov_set(P0); b.cov_set(P0)
        # an unarmed handle
        with pytest.raises(capi.MsckfError) as e:
            a.cov_zupt_frame_checked(_loose(case), LEG, N, r, synth.ZUPT_NOISES, True, True)
        assert e.value.code == INVALID and np.array_equal(a.cov_get(), P0)
        # validation on an armed handle: nothing done, the arming stands
        _arm(a, case)
        for what, call in (('a constant', lambda: a.cov_zupt_frame_checked(_loose(case, sigma_w2=-1.0), LEG, N, r, synth.ZUPT_NOISES, True, True)),
                           ('the window', lambda: a.cov_zupt_frame_checked(_loose(case), LEG, N + 1, r, synth.ZUPT_NOISES, True, True)),
                           ('a variance', lambda: a.cov_zupt_frame_checked(_loose(case), LEG, N, r, (0.0, 1e-4, 1e-4), True, True))):
            with pytest.raises(capi.MsckfError) as e:
                call()
            assert e.value.code == INVALID and np.array_equal(a.cov_get(), P0), what
        ga, verdict = a.cov_zupt_frame_checked(_loose(case), LEG, N, r, synth.ZUPT_NOISES, True, True)
        assert ga['applied'] == 1 and verdict['accept'] == 1
        # a refused Phi: no propagation, no verdict, no update, nothing marginalised; augmentation stands
        bad = ic.make_case('right_closed', 5, n=LEG, seed=53)
        bad['samples'][2, 1:4] = bad['state'].bg
        a.cov_set(P0)
        _arm(a, bad)
        ga, verdict = a.cov_zupt_frame_checked(_loose(bad), LEG, N, r, synth.ZUPT_NOISES, True, True, raise_on_refusal=False)
        assert (ga['rc'], ga['applied'], ga['n_after']) == (NOT_SPD, 0, LEG + 6 * N) and not ga['dx'].any()
        assert (verdict['evaluated'], verdict['accept'], verdict['status']) == (0, 0, NOT_SPD)
        b.cov_augment()
        assert np.array_equal(a.cov_get(), b.cov_get())
    finally:
        a.close(); b.close()
