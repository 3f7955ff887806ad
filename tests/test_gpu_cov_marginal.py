"""GPU tests of the marginal read of the resident covariance (orcvio_msckf_cov_get_marginal / _marginal_submit / _marginal_collect,
k_cov_marginal) with the cases and the checker of tests/cov_marginal_cases.py: gathers bit for bit against cov_get()[idx][:, idx],
congruences inside the derived bar (2 n_idx + 4) 2^-53 (|T| |P_m| |T|^T) against the 60-digit value, the same call twice the same bits;
NaN in and beside the gathered entries; the read after every kind of edit of a handle's history (the buffers change roles across them);
its place in stream order; every refusal, each followed by a good call."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
import cov_cases as cc
import cov_marginal_cases as mc

pytestmark = pytest.mark.gpu


def _new(max_clones=40):
    return capi.MsckfUpdater(device=0, max_clones=max_clones, max_features=512, max_observations=16384, debug_hooks=True)


@pytest.fixture(scope='module')
def upd(built):
    u = _new()
    yield u
    u.close()


@pytest.fixture(scope='module')
def twin(built):
    u = _new()
    yield u
    u.close()


@pytest.fixture(scope='module')
def upd_full(built):
    """a handle whose capacity is the covariance: n_max = 46 + 6 * 3 = 64"""
    u = _new(max_clones=3)
    yield u
    u.close()


def _run(u, case):
    u.cov_set(case.P)
    out = u.cov_get_marginal(case.idx, case.T)
    frac = mc.check(case, out, 'device')
    again = u.cov_get_marginal(case.idx, case.T)
    assert np.array_equal(out, again, equal_nan=True), (repr(case), 'the same call twice')
    print('FIG %r fraction of the bar %.3f' % (case, frac))
    return out


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', mc.shape_cases(73), ids=repr)
def test_every_shape_on_an_odd_state_with_extra_states(upd, case):
    """n = 73 = 22 + 6 * 8 + 3: n_idx in {1, 2, 9, 16, 17, 63, 64} x m in {0, 1, 6, 9, 17, 64}"""
    out = _run(upd, case)
    if case.m == 0:
        full = upd.cov_get()
        ix = case.idx.astype(np.int64)
        assert np.array_equal(out, full[np.ix_(ix, ix)])


@pytest.mark.parametrize('n', [34, 58])
def test_every_kind_of_idx_at_the_smallest_states_of_both_legs(upd, n):
    """n = 34 (leg 22, two clones) and 58 (leg 46): ascending, reversed, permuted, with a repeat, with 0 and n - 1; both kinds of P"""
    for case in mc.kind_cases(n):
        _run(upd, case)
    big = mc.shape_case(n, 64, 17, 'repeat', 'graded')   # more indices than states: repeats
    _run(upd, big)


def test_a_handle_at_its_capacity(upd_full):
    """n = n_max = 64: the whole matrix as one gather, reversed, and a 64 x 64 congruence of it"""
    n = 64
    for case in mc.kind_cases(n) + [mc.shape_case(n, 64, 0, 'reversed', 'asym'), mc.shape_case(n, 64, 64, 'permuted', 'graded'),
                                    mc.shape_case(n, 64, 0, 'ends', 'graded')]:
        out = _run(upd_full, case)
    full = upd_full.cov_get()
    ix = case.idx.astype(np.int64)
    assert np.array_equal(out, full[np.ix_(ix, ix)])


# ---- NaN ------------------------------------------------------------------------------------------------------------------------------
def test_nan_outside_has_no_effect_and_inside_lands_where_the_gather_puts_it(upd):
    base = mc.shape_case(73, 9, 6, 'permuted', 'asym')
    ix = base.idx.astype(np.int64)
    outside = [i for i in range(73) if i not in set(ix.tolist())]
    # every entry that is not gathered: rows and columns of states not listed, and the listed states' entries against them
    P = base.P.copy()
    P[np.ix_(outside, range(73))] = np.nan
    P[np.ix_(range(73), outside)] = np.inf
    c = mc.Case(73, 9, 6, P=P, idx=base.idx, T=base.T)
    assert np.array_equal(c.Pm, base.Pm)
    out = _run(upd, c)
    assert np.all(np.isfinite(out))
    g = mc.Case(73, 9, 0, P=P, idx=base.idx)
    assert np.all(np.isfinite(_run(upd, g)))
    # one gathered entry: (idx[2], idx[5]) -- not its transpose
    P2 = base.P.copy()
    P2[ix[2], ix[5]] = np.nan
    g2 = mc.Case(73, 9, 0, P=P2, idx=base.idx)
    out = _run(upd, g2)
    where = np.argwhere(np.isnan(out))
    assert where.tolist() == [[2, 5]]
    # ... and through a congruence it spreads as the arithmetic says: P_m(2, 5) is a term of every Y(i, 5), Y(i, 5) of every out(i, j)
    # (a zero in T does not stop a NaN: the entries of P are not examined)
    out = upd.cov_get_marginal(base.idx, base.T)
    assert np.all(np.isnan(out))


# ---- a handle's history -----------------------------------------------------------------------------------------------------------------
def _against_cov_get(u, what, seed):
    """the gather FIRST (behind whatever the last call left enqueued), then cov_get: bit for bit; returns the covariance"""
    n = capi.debug_factor_state(u)['res_n']
    rng = np.random.default_rng(seed)
    k = min(n, 64)
    lists = [rng.permutation(n)[:k].astype(np.int32), np.array(mc.ODOMETRY_IDX, dtype=np.int32), np.arange(n - k, n, dtype=np.int32)[::-1].copy()]
    got = [u.cov_get_marginal(ix) for ix in lists]
    P = u.cov_get()
    assert P.shape == (n, n), what
    for ix, g in zip(lists, got):
        j = ix.astype(np.int64)
        assert np.array_equal(g, P[np.ix_(j, j)], equal_nan=True), what
    R = mc.rotation(seed)
    idx, T = mc.odometry_spec(R)
    c = mc.Case(n, 9, 9, P=P, idx=idx, T=T)
    mc.check(c, u.cov_get_marginal(idx, T), what)
    return P


def test_the_read_follows_every_edit_of_a_handles_history(upd):
    u, leg, N = upd, 22, 7
    fl = synth.Flags(use_larvio=1, leg_dim=leg)
    seen = []

    def step(what):
        P = _against_cov_get(u, what, 100 + len(seen))
        seen.append((what, P))
        return P

    P0 = cc.graded_factorable(leg + 6 * N)
    u.cov_set(P0)
    assert np.array_equal(step('cov_set'), P0)
    Phi, Q = cc.phi_q(leg, 5)
    u.cov_propagate(Phi, Q)
    P = step('cov_propagate')
    assert not np.array_equal(P, P0)
    u.cov_augment()
    N += 1
    assert step('cov_augment').shape[0] == leg + 6 * N
    w = synth.make_window(N=N, F=40, seed=300 + N, track_len=(2, 6), flags=fl)
    io = u.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=False)
    u.io_fill(io, w, with_P=False)
    stats = u.io_update(want_P=False, commit=True)
    assert stats[3] == 1
    Pu = step('io_update with commit')
    assert not np.array_equal(Pu, seen[-2][1])
    u.cov_remove_clones(leg, [0, 3])
    N -= 2
    assert step('cov_remove_clones').shape[0] == leg + 6 * N
    r = np.concatenate([2e-3 * np.ones(3), 1e-3 * np.ones(3), 5e-4 * np.ones(3)])
    got = u.cov_zupt(leg, N, r, synth.ZUPT_NOISES)
    assert got['applied'] == 1
    assert not np.array_equal(step('cov_zupt'), seen[-2][1])
    # an object update on the resident covariance and its commit
    ofl = synth.Flags(use_larvio=0, use_left_perturbation=0)
    ow = synth.make_window(N=N, F=4, seed=0, flags=ofl, track_len=4)
    objs = synth.make_objects(ow, n_objects=3, seed=1, sigma_kp=0.004)
    u.cov_set(ow.P)
    obj = u.update_object_tracks(ofl, ow.N, objs, None, ow.R_b2c[0], ow.t_c_b[0], True, False, 0)
    u.cov_commit()
    Po = step('update_object_tracks(P = NULL) with its commit')
    assert (not np.array_equal(Po, ow.P)) == bool(obj['accept'])
    # one frame call that marginalises: its last launches are enqueued and not waited for
    wf = synth.make_window(N=N, F=0, seed=300 + N, track_len=None, flags=fl)
    res = u.io_step_frame(wf, augment=False, remove=[1])
    assert res['rc'] == 0 and res['n_after'] == leg + 6 * (N - 1)
    assert step('io_step_frame with marginalisation').shape[0] == leg + 6 * (N - 1)
    # features entering the state, the factor carried along
    import entering_cases as ec
    from test_gpu_entering_factor import options, prepare, stage_and_run
    case = ec.make_case(ec.CaseId('small', 1, 6))
    with options(u, case):
        prepare(u, case, 'augmented')
        step('cov_augment behind a prefactorisation')
        stage_and_run(u, case)
        u.cov_commit_new_features_fac()
    assert step('cov_commit_new_features_fac').shape[0] == case.win.n + 6
    assert len(seen) == 10


# ---- stream order -----------------------------------------------------------------------------------------------------------------------
def test_a_submit_reads_at_its_own_place_in_stream_order(upd, twin):
    """submit, then an enqueued cov_augment, then collect: the values from BEFORE the edit; the read changes no bookkeeping, and the next
    update is bit for bit that of a twin handle that never read"""
    leg, N, extra = 22, 7, 3
    n = leg + 6 * N + extra
    P0 = cc.graded_factorable(n)
    fl = synth.Flags(use_larvio=1, leg_dim=leg)
    idx = np.array([0, 63, 64, 65, 66, 7, 30, 66], dtype=np.int32)   # the extra states move when the clone enters in front of them
    T = mc.make_T(5, len(idx))
    outs = []
    for u, reads in ((upd, True), (twin, False)):
        u.cov_set(P0)
        u.cov_prefactor()
        st0 = capi.debug_factor_state(u)
        u.set_extra_states(extra)
        try:
            if reads:
                u.cov_marginal_submit(idx, T)
                assert capi.debug_factor_state(u) == st0
            u.cov_augment()
            st1 = capi.debug_factor_state(u)
            if reads:
                before = u.cov_marginal_collect()
                assert capi.debug_factor_state(u) == st1
                after = u.cov_get_marginal(idx, T)
                gather_after = u.cov_get_marginal(idx)
            w = dataclasses.replace(synth.make_window(N=N + 1, F=40, seed=300 + N + 1, track_len=(2, 6), flags=fl), n_extra=extra)
            io = u.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=False)
            u.io_fill(io, w, with_P=False)
            stats = u.io_update(want_P=False, commit=True)
            assert stats[3] == 1
            outs.append((st1, io['dx'].copy(), u.cov_get(), capi.debug_factor_state(u)))
        finally:
            u.set_extra_states(0)
    c_before = mc.Case(n, len(idx), 5, P=P0, idx=idx, T=T)
    mc.check(c_before, before, 'before the edit')
    P1 = cc.apply_map(P0, cc.augment_map(n, extra))
    j = idx.astype(np.int64)
    assert np.array_equal(gather_after, P1[np.ix_(j, j)])
    mc.check(mc.Case(n + 6, len(idx), 5, P=P1, idx=idx, T=T), after, 'after the edit')
    assert not np.array_equal(before, after)
    a, b = outs
    assert a[0] == b[0] and a[3] == b[3]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _raw(u, n_idx, idx, m, T, out):
    q = capi.Marginal()
    q.n_idx, q.m = n_idx, m
    q.idx = idx.ctypes.data_as(C.POINTER(C.c_int32)) if idx is not None else None
    q.T = T.ctypes.data_as(C.POINTER(C.c_double)) if T is not None else None
    return u.lib.orcvio_msckf_cov_get_marginal(u.h, C.byref(q), out.ctypes.data_as(C.POINTER(C.c_double)) if out is not None else None)


def test_every_refusal_is_followed_by_a_good_call(built):
    u = capi.MsckfUpdater(device=0, max_clones=8, max_features=64, max_observations=1024, debug_hooks=True)
    try:
        n = 34
        case = mc.shape_case(n, 9, 6, 'permuted', 'asym')
        idx, T = case.idx, case.T
        out = np.full((64, 64), -7.0)
        dp = C.POINTER(C.c_double)

        def good(what):
            assert np.array_equal(u.cov_get(), case.P), what
            assert capi.debug_factor_state(u) == st, what
            mc.check(case, u.cov_get_marginal(idx, T), what)

        assert _raw(u, 9, idx, 6, T, out) == 1   # no resident covariance
        u.cov_set(case.P)
        st = capi.debug_factor_state(u)
        good('after: no resident covariance')
        bad_hi, bad_lo = idx.copy(), idx.copy()
        bad_hi[4], bad_lo[8] = n, -1
        T_nan, T_inf = T.copy(), T.copy()
        T_nan[5, 8], T_inf[0, 0] = np.nan, np.inf
        long_idx = np.zeros(65, dtype=np.int32)
        long_T = np.zeros((65, 9))
        for what, args in (('idx NULL', (9, None, 6, T, out)), ('out NULL', (9, idx, 6, T, None)), ('n_idx = 0', (0, idx, 0, None, out)),
                           ('n_idx = 65', (65, long_idx, 0, None, out)), ('n_idx < 0', (-1, idx, 0, None, out)),
                           ('index = n', (9, bad_hi, 6, T, out)), ('index < 0', (9, bad_lo, 6, T, out)), ('m < 0', (9, idx, -1, T, out)),
                           ('m = 65', (9, idx, 65, long_T, out)), ('T NULL with m > 0', (9, idx, 6, None, out)),
                           ('T given with m = 0', (9, idx, 0, T, out)), ('NaN in T', (9, idx, 6, T_nan, out)), ('Inf in T', (9, idx, 6, T_inf, out))):
            assert _raw(u, *args) == 1, what
            assert np.all(out == -7.0), what
            good('after: ' + what)
        q, keep = u._marginal(idx, T)
        assert u.lib.orcvio_msckf_cov_get_marginal(None, C.byref(q), out.ctypes.data_as(dp)) == 1
        assert u.lib.orcvio_msckf_cov_get_marginal(u.h, None, out.ctypes.data_as(dp)) == 1
        assert u.lib.orcvio_msckf_cov_marginal_submit(u.h, None) == 1 and u.lib.orcvio_msckf_cov_marginal_submit(None, C.byref(q)) == 1
        good('after: null arguments')
        # a collect without a submit; a second submit before the collect -- the first one stands and is collected
        rows = C.c_int32(-1)
        assert u.lib.orcvio_msckf_cov_marginal_collect(u.h, out.ctypes.data_as(dp), C.byref(rows)) == 1 and rows.value == -1
        good('after: collect without submit')
        u.cov_marginal_submit(idx, T)
        with pytest.raises(capi.MsckfError) as e:
            u.cov_marginal_submit(idx[:3])
        assert e.value.code == 1
        assert u.lib.orcvio_msckf_cov_marginal_collect(u.h, None, C.byref(rows)) == 1   # (out NULL: the submit still stands)
        first = u.cov_marginal_collect()
        assert first.shape == (6, 6)
        mc.check(case, first, 'the first submit')
        with pytest.raises(capi.MsckfError) as e:
            u.cov_marginal_collect()
        assert e.value.code == 1
        good('after: second submit / second collect')
        assert np.all(out == -7.0)
        # a communicator on the handle, as cov_zupt
        u.comm_init(capi.comm_unique_id(), 0, 1)
        assert _raw(u, 9, idx, 6, T, out) == 1 and np.all(out == -7.0)
        with pytest.raises(capi.MsckfError) as e:
            u.cov_marginal_submit(idx)
        assert e.value.code == 1
        u.comm_destroy()
        good('after: a communicator on the handle')
    finally:
        u.close()
