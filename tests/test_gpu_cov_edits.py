"""The edits of the device-resident covariance P and the square-root factor S (P = S S^T) that follows them, at the edge shapes
(tests/cov_cases.py has the inputs, the references, the derived propagation bar, the row maps and the expected-tail model;
tests/test_cov_cases.py runs the same checks on the numpy mirror and on mutations):

  a  propagation, element by element against the derived bar, through cov_propagate and through the frame call's fused head, both
     LEG instantiations; the two routes bit for bit
  b  the copies (augment, remove_clones, clones_to_nuisance, remove_features; the frame call's marginalisation): P equals the mirror,
     S equals S_before[map], the bookkeeping's dimensions, the trailing-zero structure -- all bit for bit
  c  cov_prefactor's S tile by tile (potrf_cases.check_factor), forward and reversed; nothing claimed at 15 tiles
  d  an update's commit: S+ = sigma Z^T and the resident P = P+ bit for bit, the separate and the in-launch commit alike
  e  lost in-state features beyond the first 64-bit word of the frame head's set: the frame call against the separate calls
  f  the factor is still usable: an update on the resident factor after a chain of edits against oracle/mirror.py
  g  history: a handle that held a larger state gives the bits of a fresh one

The propagation bar is derived, the prefactor's bar is potrf_cases.factor_bar, the update's 1e-6 is the existing tests'; everything else
is bit equality.  Every figure is printed before it is asserted (pytest -s)."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror, mirror_cov as mc
from helpers import rel
import potrf_cases as pc
import cov_cases as cc

pytestmark = pytest.mark.gpu
UPDATE_TOL = 1e-6   # tests/test_gpu_cov.py's


def _new(factor=True):
    u = capi.MsckfUpdater(device=0, max_clones=40, max_features=64, max_observations=1024, debug_hooks=True)
    if not factor:
        u._chk(u.lib.orcvio_msckf_set_option(u.h, 7, 0), 'set_option')   # ORCVIO_OPT_RESIDENT_FACTOR off
    return u


@pytest.fixture(scope='module')
def upd(built):
    u = _new()
    yield u
    u.close()


@pytest.fixture(scope='module')
def upd2(built):
    u = _new()
    yield u
    u.close()


@pytest.fixture(scope='module')
def upd_nofac(built):
    u = _new(factor=False)
    yield u
    u.close()


N_MAX = 46 + 6 * 40


def _flags(leg):
    return synth.Flags(use_larvio=1, leg_dim=leg)


@pytest.fixture(scope='module')
def windows():
    made = {}

    def get(N, leg, F=0, extra=0):
        key = (N, leg, F)
        if key not in made:
            made[key] = synth.make_window(N=N, F=F, seed=300 + N, track_len=None if N < 3 else (2, min(N, 6)), flags=_flags(leg))
        return dataclasses.replace(made[key], n_extra=extra)
    return get


def _state(u):
    return capi.debug_factor_state(u)


def _frame(u, win, extra, **kw):
    """one frame call on an empty window: the head (and the marginalisation) are the whole frame"""
    win = dataclasses.replace(win, n_extra=extra)
    u.set_extra_states(extra)
    try:
        if 'n_feature_states' in kw:
            got = u.io_step_frame_ex(win, **kw)
        else:
            got = u.io_step_frame(win, **kw)
    finally:
        u.set_extra_states(0)
    assert got['rc'] == 0 and got['repaired'] == 0 and got['stats'][3] == 0 and not np.any(got['dx'])
    return got


# ---- a. propagation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('leg,N,extra', cc.PROP_SHAPES)
def test_propagation_element_by_element_on_both_routes(upd, windows, leg, N, extra):
    c = cc.prop_case(leg, N, extra)
    P, Phi, Q, n = c['P'], c['Phi'], c['Q'], c['n']
    upd.cov_set(P)
    upd.cov_propagate(Phi, Q)
    got = upd.cov_get()
    print('FIG cov_propagate leg=%d N=%d extra=%d Frobenius %.2e' % (leg, N, extra, cc.frobenius(got, c['ref64'])))
    frac = cc.check_propagation(got, P, c['ref'], c['bar'], leg)
    print('FIG cov_propagate leg=%d N=%d extra=%d fraction of the bar %.3f' % (leg, N, extra, frac))
    if N >= 1:   # the fused head without augmentation: the same bits
        upd.cov_set(P)
        _frame(upd, windows(N, leg), extra, Phi=Phi, Q=Q, augment=False)
        head = upd.cov_get()
        frac_h = cc.check_propagation(head, P, c['ref'], c['bar'], leg)
        print('FIG k_frame_head leg=%d N=%d extra=%d fraction of the bar %.3f' % (leg, N, extra, frac_h))
        assert np.array_equal(head, got)
    if n + 6 <= N_MAX and N + 1 <= 40:   # ... and with it (the only form the call takes at N = 0): the new clone's rows and columns are copies
        upd.cov_set(P)
        upd.cov_propagate(Phi, Q)
        _device_edit(upd, 'augment', leg, rest=extra)
        by_calls = upd.cov_get()
        m = cc.augment_map(n, extra)
        assert np.array_equal(by_calls, cc.apply_map(got, m)) and np.array_equal(by_calls, mc.augment(got, rest=extra))
        upd.cov_set(P)
        res = _frame(upd, windows(N + 1, leg), extra, Phi=Phi, Q=Q, augment=True)
        assert res['n_after'] == n + 6
        head = upd.cov_get()
        assert np.array_equal(head, by_calls)
        inv = np.r_[np.arange(n - extra), np.arange(n - extra + 6, n + 6)]   # the old states inside the augmented matrix
        frac_h = cc.check_propagation(cc.apply_map(head, inv), P, c['ref'], c['bar'], leg)
        print('FIG k_frame_head+augment leg=%d N=%d extra=%d fraction of the bar %.3f' % (leg, N, extra, frac_h))


# ---- b. the copies ----------------------------------------------------------------------------------------------------------------------
def _start(u, P, prefactor=True):
    """cov_set + cov_prefactor; returns (S, ops) -- S None where no factor is claimed"""
    n = P.shape[0]
    u.cov_set(P)
    if not prefactor:
        return None, []
    u.cov_prefactor()
    st = _state(u)
    assert st == dict(fac_valid=1, fac_n=n, fac_k=n, res_n=n), st
    ops = ['prefactor_rev' if cc.prefactor_reversed(n) else 'prefactor_fwd']
    S = capi.debug_factor(u)
    cc.check_tail(S, cc.expected_tail(ops))
    return S, ops


def _device_edit(u, kind, leg, **a):
    if kind == 'augment':
        u.set_extra_states(a.get('rest', 0))
        try:
            u.cov_augment()
        finally:
            u.set_extra_states(0)
    elif kind == 'remove_clones':
        u.cov_remove_clones(leg, a['clones'])
    elif kind == 'clones_to_nuisance':
        u.cov_clones_to_nuisance(leg, a['clones'])
    elif kind == 'remove_features':
        u.cov_remove_features(leg, a['N'], a['d'], a['nf'], a['slots'])
    else:
        raise ValueError(kind)


def _check_edit(u, P, S, ops, fac_k, what):
    """the device's P, S and bookkeeping after an edit against the host's (P, S, ops); returns the device's (P, S)"""
    got = u.cov_get()
    assert got.shape == P.shape and np.array_equal(got, P), what
    st = _state(u)
    assert st['res_n'] == P.shape[0], what
    if S is None:
        assert st['fac_valid'] == 0, what
        return got, None
    assert st == dict(fac_valid=1, fac_n=P.shape[0], fac_k=fac_k, res_n=P.shape[0]), (what, st)
    Sg = capi.debug_factor(u)
    assert Sg.shape == S.shape and np.array_equal(Sg, S), what
    cc.check_tail(Sg, cc.expected_tail(ops))
    return got, Sg


def _chain(u, leg, P0, edits, prefactor=True):
    """cov_set, cov_prefactor and the edits, each checked bit for bit; returns (P, S, ops) as they stand at the end"""
    S, ops = _start(u, P0, prefactor)
    P, k = np.array(P0), P0.shape[0]
    for i, (kind, a) in enumerate(edits):
        _device_edit(u, kind, leg, **a)
        P, S, m, op = cc.edit_host(P, S, kind, leg, **{q: v for q, v in a.items() if q != 'nf'})
        ops = ops + [op]
        _check_edit(u, P, S, ops, k, (i, kind, a))
    return P, S, ops


# (leg, N, extra): n = 58, 63, 64, 65 in front of the augmentation for both legs (ld_for(n) != ld_for(n + 6) at 58, 63; n on and beside a
# multiple of 16), N = 0, 1 and 8, an extra block of 9 behind the clones
COPY_SHAPES = [(22, 6, 0), (22, 6, 5), (22, 7, 0), (22, 7, 1), (46, 2, 0), (46, 2, 5), (46, 3, 0), (46, 3, 1),
               (22, 0, 0), (22, 0, 9), (22, 1, 0), (22, 1, 9), (46, 0, 0), (46, 1, 9), (22, 8, 0), (22, 8, 9), (46, 8, 0), (46, 8, 9)]


@pytest.mark.parametrize('leg,N,extra', COPY_SHAPES)
def test_augment_and_marginalise_copy_P_and_S(upd, leg, N, extra):
    """augment, then the first clone, the last clone (the one that has just entered) and all the others leave; without an augmentation in
    front (the tail stays): all clones at once -- eight at N = 8"""
    n = leg + 6 * N + extra
    P0 = cc.graded_factorable(n)
    edits = [('augment', dict(rest=extra)), ('remove_clones', dict(clones=[0]))]
    if N >= 1:
        edits.append(('remove_clones', dict(clones=[N - 1])))
    if N >= 2:
        edits.append(('remove_clones', dict(clones=list(range(N - 1)))))
    P, S, ops = _chain(upd, leg, P0, edits)
    assert P.shape[0] == leg + extra and S.shape == (P.shape[0], n) and cc.expected_tail(ops) == 0
    if N >= 1:
        P, S, ops = _chain(upd, leg, P0, [('remove_clones', dict(clones=list(range(N))))])
        assert P.shape[0] == leg + extra and cc.expected_tail(ops) == (15 if n >= 31 else 0)
    P, S, ops = _chain(upd, leg, P0, [('augment', dict(rest=extra))], prefactor=False)   # no factor: none is made up
    assert S is None


@pytest.mark.parametrize('leg,N,extra', [(22, 7, 0), (22, 7, 1), (46, 3, 1), (22, 8, 9), (46, 8, 9), (22, 2, 0)])
def test_clones_to_nuisance_and_the_edits_behind_a_nuisance_block(upd, leg, N, extra):
    """the first and the last clone become nuisance states (12 columns at the end); then a clone enters in front of the extra and the
    nuisance states, the extra block's features leave in front of the nuisance block, and a clone is marginalised"""
    n = leg + 6 * N + extra
    P0 = cc.graded_factorable(n)
    edits = [('clones_to_nuisance', dict(clones=[0, N - 1])), ('augment', dict(rest=extra + 12))]
    Nw = N - 2 + 1
    if extra == 9:
        edits.append(('remove_features', dict(N=Nw, d=3, nf=3, slots=[0, 2])))
        edits.append(('remove_features', dict(N=Nw, d=1, nf=3, slots=[1])))
    edits.append(('remove_clones', dict(clones=[Nw - 1])))
    _chain(upd, leg, P0, edits)
    _chain(upd, leg, P0, [('clones_to_nuisance', dict(clones=list(range(N))))])   # every clone (eight at N = 8)


@pytest.mark.parametrize('leg,N,d,nf,slots', [(22, 6, 1, 5, [0]), (22, 6, 1, 5, [4]), (22, 6, 1, 5, [0, 1, 2, 3, 4]), (46, 1, 3, 3, [0, 2]),
                                               (22, 0, 3, 3, [1]), (46, 3, 1, 1, [0]), (22, 8, 1, 9, [0, 4, 8])])
def test_remove_features_copies_P_and_S(upd, leg, N, d, nf, slots):
    n = leg + 6 * N + d * nf
    edits = [('remove_features', dict(N=N, d=d, nf=nf, slots=slots)), ('augment', dict(rest=d * (nf - len(slots))))]
    _chain(upd, leg, cc.graded_factorable(n), edits)


@pytest.mark.parametrize('leg,N,extra,clones', [(22, 7, 0, [0]), (22, 7, 1, [6]), (46, 3, 1, [0, 1, 2]), (22, 8, 9, list(range(8))),
                                                (46, 8, 0, list(range(8))), (22, 10, 0, [0, 1, 2, 4, 5, 6, 8, 9])])
def test_the_frame_calls_marginalisation_copies_P_and_S(upd, windows, leg, N, extra, clones):
    """k_cov_remove_fac (the clones by value, eight at the most) against the mirror and the row map, with and without a factor"""
    n = leg + 6 * N + extra
    P0 = cc.graded_factorable(n)
    for prefactor in (True, False):
        S, ops = _start(upd, P0, prefactor)
        got = _frame(upd, windows(N, leg), extra, augment=False, remove=clones)
        assert got['n_after'] == n - 6 * len(clones)
        Pn, Sn, m, op = cc.edit_host(P0, S, 'remove_clones', leg, clones=clones)
        _check_edit(upd, Pn, Sn, ops + [op], n, (prefactor, clones))


# ---- c. prefactor -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', cc.PREFACTOR_N)
def test_prefactor_tile_by_tile(upd, n):
    X = cc.graded_factorable(n)
    rev = cc.prefactor_reversed(n)
    bar, a, b = pc.factor_bar(X, pc.TOL_PRIOR, (), rev)
    S, ops = _start(upd, X)
    w = pc.omega_tiles(S, X, rev)
    print('FIG cov_prefactor n=%d rev=%d %.3f bar %.3f fraction %.3f' % (n, rev, w, bar, w / bar))
    pc.check_factor(S, X, bar, (), rev)
    L = S[::-1, :] if rev else S   # (the factor as the Cholesky left it: lower triangular)
    assert np.abs(np.triu(L, 1)).max() == 0.0


def test_prefactor_claims_nothing_at_fifteen_tiles(upd):
    n = cc.PREFACTOR_N_NONE
    upd.cov_set(cc.graded_factorable(n))
    upd.cov_prefactor()
    assert _state(upd)['fac_valid'] == 0 and _state(upd)['res_n'] == n


# ---- d. commit --------------------------------------------------------------------------------------------------------------------------
def _update_window(windows, N, leg, P, extra=0, F=12):
    w = windows(N, leg, F, extra)
    assert w.n == P.shape[0]
    return dataclasses.replace(w, P=np.ascontiguousarray(P))


def _sigma_Zt(u, n, kf):
    ldz = capi.debug_read(u, 'dims')['ldz']
    Z = capi.debug_read(u, 'Z').reshape(-1)[:kf * ldz].reshape(kf, ldz)[:, :n]
    return np.ascontiguousarray(0.008 * Z.T)   # (noise_feature: one multiplication, bit for bit)


@pytest.mark.parametrize('leg,N,how', [(22, 7, 'no factor'), (22, 7, 'prefactored'), (22, 7, 'augmented'), (46, 3, 'prefactored'), (22, 2, 'no factor')])
def test_commit_leaves_sigma_Zt_and_P_new(upd, upd2, windows, leg, N, how):
    """the separate commit (update_features, cov_commit) and the in-launch commit (io_update with commit): S+ = sigma Z^T, the resident
    P = P+, the two forms alike -- bit for bit.  (40 tracks: more than the 16 projected rows up to which the in-launch form takes the
    direct update of a thin stack, which is another algorithm and leaves no factor -- the test below.)"""
    n0 = leg + 6 * (N - (how == 'augmented'))
    P0 = cc.graded_factorable(n0)
    edits = [('augment', {})] if how == 'augmented' else []
    for u in (upd, upd2):
        P, S, ops = _chain(u, leg, P0, edits, prefactor=how != 'no factor')
    n = P.shape[0]
    w = _update_window(windows, N, leg, P, F=40)
    assert w.flags.noise_feature == 0.008
    got = upd.update_features(w, resident_cov=True, want_P=True)
    assert got['updated'] and got['accept'].sum() > 0 and got['stats'][0] > 16
    upd.cov_commit()
    st = _state(upd)
    assert st['fac_valid'] == 1 and st['fac_n'] == n and st['res_n'] == n and st['fac_k'] == (n0 if S is not None else n), st
    assert np.array_equal(upd.cov_get(), got['P_new'])
    Sp = capi.debug_factor(upd)
    assert np.array_equal(Sp, _sigma_Zt(upd, n, st['fac_k']))
    print('FIG commit %s leg=%d N=%d rel(S+ S+^T, P+) %.2e' % (how, leg, N, rel(Sp @ Sp.T, got['P_new'])))
    assert rel(Sp @ Sp.T, got['P_new']) < 1e-12   # (the existing tests' figure for a committed factor)
    # the in-launch commit
    io = upd2.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=False)
    upd2.io_fill(io, w, with_P=False)
    stats = upd2.io_update(want_P=False, commit=True)
    assert stats[3] == 1
    assert np.array_equal(io['dx'], got['dx']) and np.array_equal(io['accept'], got['accept'])
    assert _state(upd2) == st
    assert np.array_equal(upd2.cov_get(), got['P_new'])
    S2 = capi.debug_factor(upd2)
    assert np.array_equal(S2, _sigma_Zt(upd2, n, st['fac_k'])) and np.array_equal(S2, Sp)


def test_the_thin_in_launch_commit_keeps_no_factor(upd2, windows):
    """at most 16 projected rows: the in-launch update takes the direct form (k_thin_gain / k_thin_apply), whose commit leaves P+ resident
    and NO factor -- a resident factor from before it must not survive it"""
    leg, N = 22, 2
    P, S, ops = _chain(upd2, leg, cc.graded_factorable(leg + 6 * N), [])
    assert S is not None
    w = _update_window(windows, N, leg, P, F=12)
    io = upd2.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=False)
    upd2.io_fill(io, w, with_P=False)
    stats = upd2.io_update(want_P=False, commit=True)
    assert stats[3] == 1 and stats[0] <= 16, stats
    ref = mirror.msckf_update(w)
    assert _state(upd2)['fac_valid'] == 0
    assert rel(io['dx'], ref['dx']) < UPDATE_TOL and rel(upd2.cov_get(), ref['P_new']) < UPDATE_TOL


# ---- e. lost slots beyond one word ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cc.LOST_CASES))
def test_lost_features_beyond_the_first_word(upd, upd2, windows, name):
    """The frame call (handle b) against cov_propagate -> cov_augment -> cov_remove_features (handle a), with and without propagation
    (without: the resident factor goes through k_fac_head or k_fac_augment), with and without augmentation: P and S bit for bit between
    the handles, P against the numpy deletion of the mirror's edits, S against the row map.  The call takes the events on an empty window."""
    d, N, nf, slots = cc.LOST_CASES[name]
    leg = cc.LOST_LEG
    n = leg + 6 * N + d * nf
    P0 = cc.graded_factorable(n)
    Phi, Q = cc.phi_q(leg, n)
    a, b = upd, upd2
    for prop in (False, True):
        for aug in (True, False):
            Sa, ops = _start(a, P0)
            Sb, _ = _start(b, P0)
            assert np.array_equal(Sa, Sb)
            # handle a: the separate calls
            Pp = P0
            if prop:
                a.cov_propagate(Phi, Q)
                Pp = a.cov_get()
            if aug:
                _device_edit(a, 'augment', leg, rest=d * nf)
            Nw = N + int(aug)
            a.cov_remove_features(leg, Nw, d, nf, list(slots))
            # handle b: the one call
            got = _frame(b, windows(Nw, leg), d * (nf - len(slots)), Phi=Phi if prop else None, Q=Q if prop else None, augment=aug,
                         idp_dim=d, n_feature_states=nf, lost=list(slots))
            m = cc.head_map_plain(n, leg, N, d, nf, slots, aug)
            assert got['n_after'] == len(m)
            # the host: numpy deletion of the mirror's edits of the (device-propagated) matrix, the row map for S
            Ph = mc.augment(Pp, rest=d * nf) if aug else Pp
            Ph = cc.apply_map(Ph, cc.remove_features_map(Ph.shape[0], leg, Nw, d, slots))
            assert np.array_equal(Ph, cc.apply_map(Pp, m))
            Sh = None if prop else np.ascontiguousarray(Sa[m])
            ops_h = ops + (['augment'] if aug else []) + ['gather']
            what = (name, prop, aug)
            _check_edit(a, Ph, Sh, ops_h, n, what + ('calls',))
            _check_edit(b, Ph, Sh, ops_h, n, what + ('frame',))
            if prop:
                assert cc.check_propagation(Pp, P0, *cc.prop_reference(P0, Phi, Q), leg) <= 1.0


def test_lost_features_up_to_the_sixth_word(built, windows):
    """The largest handle (60 clones: 406 states) holds 372 1-d features beside one clone: the walk reaches word 5 of its eight.  Words 6
    and 7 and the stop at the last word cannot be reached on a device (the set holds 512 slots, a handle at most 384 features): they
    run in tests/test_cov_cases.py only.  No factor at this size: P alone, against the separate calls and plain deletion."""
    leg, N, d, nf = 22, 1, 1, 372
    slots = [0, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 371]
    n = leg + 6 * N + nf
    P0 = cc.graded_prior(n, 5)
    Phi, Q = cc.phi_q(leg, n)
    a = capi.MsckfUpdater(device=0, max_clones=60, max_features=8, max_observations=64, debug_hooks=True)
    b = capi.MsckfUpdater(device=0, max_clones=60, max_features=8, max_observations=64, debug_hooks=True)
    try:
        for prop in (False, True):
            for aug in (True, False):
                a.cov_set(P0); b.cov_set(P0)
                Pp = P0
                if prop:
                    a.cov_propagate(Phi, Q)
                    Pp = a.cov_get()
                if aug:
                    _device_edit(a, 'augment', leg, rest=nf)
                a.cov_remove_features(leg, N + int(aug), d, nf, slots)
                got = _frame(b, windows(N + int(aug), leg), nf - len(slots), Phi=Phi if prop else None, Q=Q if prop else None, augment=aug,
                             idp_dim=d, n_feature_states=nf, lost=slots)
                m = cc.head_map_plain(n, leg, N, d, nf, slots, aug)
                assert np.array_equal(m, cc.head_map(n, leg, N, d, nf, slots, aug)) and got['n_after'] == len(m)
                Ph = cc.apply_map(Pp, m)
                assert np.array_equal(a.cov_get(), Ph), (prop, aug)
                assert np.array_equal(b.cov_get(), Ph), (prop, aug)
                assert _state(a)['fac_valid'] == 0 and _state(b)['fac_valid'] == 0
    finally:
        a.close(); b.close()


# ---- f. the factor is still usable ------------------------------------------------------------------------------------------------------
_REFS = {}   # family -> the mirror's update (computed once, shared by the two handles)


def _family(name):
    """(leg, N in front, extra in front, P0's n, edits or a frame, window N behind, extra behind)"""
    if name == 'marginalise':     # tail 15 kept: 70 -> 64
        return dict(leg=22, n=70, edits=[('remove_clones', dict(clones=[0]))], N=7, extra=0)
    if name == 'augment':         # tail 0, fac_k = 64 < n = 70 -> 64
        return dict(leg=22, n=64, edits=[('augment', {}), ('remove_clones', dict(clones=[3]))], N=7, extra=0)
    if name == 'leg46':
        return dict(leg=46, n=46 + 6 * 5, edits=[('remove_clones', dict(clones=[0, 4]))], N=3, extra=0)
    if name == 'remove_features':  # 22 + 36 + 9 -> the features 0 and 8 leave
        return dict(leg=22, n=67, edits=[('remove_features', dict(N=6, d=1, nf=9, slots=[0, 8]))], N=6, extra=7)
    if name == 'nuisance':        # two clones become Schmidt nuisance states (a permutation: tail 15 kept), 6 clones + 12 columns
        return dict(leg=22, n=70, edits=[('clones_to_nuisance', dict(clones=[1, 4]))], N=6, extra=12, schmidt=2)
    if name == 'lost_frame':      # 170 states, six slots over three words leave inside the frame call, no augmentation: tail 15, n = 164
        return dict(leg=22, n=170, frame=cc.LOST_CASES['word_edges'], N=3, extra=124)
    raise ValueError(name)


def _run_family(u, windows, name, with_factor):
    f = _family(name)
    leg = f['leg']
    P0 = cc.graded_factorable(f['n'])
    if 'edits' in f:
        if with_factor:
            P, S, ops = _chain(u, leg, P0, f['edits'])
        else:
            u.cov_set(P0)
            P = np.array(P0)
            for kind, a in f['edits']:
                _device_edit(u, kind, leg, **a)
                P = cc.edit_host(P, None, kind, leg, **{q: v for q, v in a.items() if q != 'nf'})[0]
            S, ops = None, []
    else:
        d, N, nf, slots = f['frame']
        S, ops = _start(u, P0, with_factor)
        _frame(u, windows(N, leg), d * (nf - len(slots)), augment=False, idp_dim=d, n_feature_states=nf, lost=list(slots))
        m = cc.head_map_plain(f['n'], leg, N, d, nf, slots, False)
        P, S, ops = cc.apply_map(P0, m), (None if S is None else S[m]), ops + ['gather']
    return f, P, S, ops


@pytest.mark.parametrize('name', ['marginalise', 'augment', 'leg46', 'remove_features', 'nuisance', 'lost_frame'])
def test_update_on_the_factor_that_came_through_the_edits(upd, upd_nofac, windows, name):
    results = []
    for u, with_factor in ((upd, True), (upd_nofac, False)):
        f, P, S, ops = _run_family(u, windows, name, with_factor)
        n = P.shape[0]
        assert n <= 224 and np.array_equal(u.cov_get(), P)
        st = _state(u)
        if with_factor:   # (not vacuous: the update below finds a valid factor of its dimension, and its tail where the model says so)
            assert st['fac_valid'] == 1 and st['fac_n'] == n and st['res_n'] == n, st
            assert np.array_equal(capi.debug_factor(u), S)
            cc.check_tail(S, cc.expected_tail(ops))
        else:
            assert st['fac_valid'] == 0
        w = _update_window(windows, f['N'], f['leg'], P, f['extra'])
        u.set_extra_states(f['extra'])
        u.set_schmidt_states(f.get('schmidt', 0))
        try:
            got = u.update_features(w, resident_cov=True, want_P=True)
        finally:
            u.set_schmidt_states(0)
            u.set_extra_states(0)
        if name not in _REFS:
            _REFS[name] = mirror.msckf_update(w)
            k = 6 * f.get('schmidt', 0)
            if k:   # (a Schmidt update leaves the nuisance block as it was: tests/test_gpu_cov.py)
                _REFS[name]['P_new'][-k:, -k:] = P[-k:, -k:]
        ref = _REFS[name]
        assert ref['updated'] and np.array_equal(got['accept'], ref['accept'])
        e_dx, e_P = rel(got['dx'], ref['dx']), rel(got['P_new'], ref['P_new'])
        print('FIG update after %s factor=%d n=%d tail=%d dx %.2e P %.2e' % (name, with_factor, n, cc.expected_tail(ops), e_dx, e_P))
        assert e_dx < UPDATE_TOL and e_P < UPDATE_TOL
        results.append(got)
    assert rel(results[0]['dx'], results[1]['dx']) < UPDATE_TOL


# ---- g. history -------------------------------------------------------------------------------------------------------------------------
def test_a_handle_that_held_a_larger_state_gives_the_same_bits(upd2, windows):
    """Handle a first holds the largest factorable state (n = 220: prefactor, a marginalisation, a committed update, so that both buffers of
    P and of S have been written at the large leading dimension), then runs the small chains; handle b is fresh and runs only those.
    P, S, dx and P+ bit for bit."""
    a, b = upd2, _new()
    try:
        leg = 22
        Pbig = cc.graded_factorable(220)
        P, S, ops = _chain(a, leg, Pbig, [('remove_clones', dict(clones=[0])), ('clones_to_nuisance', dict(clones=[5]))])
        a.cov_set(Pbig); a.cov_prefactor()
        wbig = _update_window(windows, 33, leg, Pbig)
        io = a.io_begin(wbig.flags, wbig.N, wbig.F, int(wbig.obs_ptr[-1]), with_P=False)
        a.io_fill(io, wbig, with_P=False)
        assert a.io_update(want_P=False, commit=True)[3] == 1
        a.cov_remove_clones(leg, [32])
        assert _state(a)['fac_valid'] == 1 and _state(a)['fac_n'] == 214
        a.cov_set(cc.graded_factorable(N_MAX))   # ... and the largest the handle takes, which has no factor

        def small(u):
            out = []
            # a chain of copies, then a committed update on its factor, then an augmentation and a marginalisation of the committed factor
            P0 = cc.graded_factorable(70)
            P, S, ops = _chain(u, leg, P0, [('remove_clones', dict(clones=[0]))])
            w = _update_window(windows, 7, leg, P)
            io = u.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=False)
            u.io_fill(io, w, with_P=False)
            assert u.io_update(want_P=False, commit=True)[3] == 1
            out += [io['dx'].copy(), u.cov_get(), capi.debug_factor(u)]
            u.cov_augment()
            u.cov_remove_clones(leg, [7])
            out += [u.cov_get(), capi.debug_factor(u), _state(u)]
            w2 = _update_window(windows, 7, leg, out[-3])
            got = u.update_features(w2, resident_cov=True, want_P=True)
            out += [got['dx'], got['P_new']]
            # lost features over three words inside the frame call, without propagation (k_fac_head), then an update on that factor
            d, N, nf, slots = cc.LOST_CASES['word_edges']
            P0 = cc.graded_factorable(170)
            _start(u, P0)
            _frame(u, windows(N + 1, leg), d * (nf - len(slots)), augment=True, idp_dim=d, n_feature_states=nf, lost=list(slots))
            out += [u.cov_get(), capi.debug_factor(u), _state(u)]
            w3 = _update_window(windows, N + 1, leg, out[-3], extra=nf - len(slots))
            u.set_extra_states(nf - len(slots))
            try:
                got = u.update_features(w3, resident_cov=True, want_P=True)
            finally:
                u.set_extra_states(0)
            assert got['updated']
            out += [got['dx'], got['P_new']]
            return out

        ra, rb = small(a), small(b)
        assert len(ra) == len(rb)
        for i, (x, y) in enumerate(zip(ra, rb)):
            assert (x == y) if isinstance(x, dict) else np.array_equal(x, y), i
    finally:
        b.close()
