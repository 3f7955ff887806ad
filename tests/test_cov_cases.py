"""CPU tests of tests/cov_cases.py: the numpy mirror stays inside the derived propagation bar (and uses a known part of it), the row
maps reproduce the mirror's edits of P, the restated 512-bit walk of lost_unmap equals plain deletion, and every mutation fails the
check that is meant to see it -- the same checks tests/test_gpu_cov_edits.py makes on the device's results."""
import numpy as np
import pytest

from oracle import mirror_cov as mc
import mirror_features_lifecycle as mfl
import potrf_cases as pc
import cov_cases as cc


def _fails(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


# ---- propagation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('leg,N,extra', cc.PROP_SHAPES)
def test_mirror_propagation_is_inside_the_bar_and_the_bar_is_not_loose(leg, N, extra):
    c = cc.prop_case(leg, N, extra)
    got = mc.propagate(c['P'], c['Phi'], c['Q'])
    frac = cc.check_propagation(got, c['P'], c['ref'], c['bar'], leg)
    print('FIG mirror_cov.propagate leg=%d N=%d extra=%d fraction of the bar %.3f' % (leg, N, extra, frac))
    assert frac < 0.5
    assert np.log10(np.diag(c['P']).max() / np.diag(c['P']).min()) > 10.0   # (more than ten decades of variance)


def _smallest_imu_state(ref64, leg):
    return int(np.argmin(np.diag(ref64)[:leg]))


@pytest.mark.parametrize('leg,N,extra', [s for s in cc.PROP_SHAPES if s[1] > 0])
def test_planted_relative_error_in_the_smallest_imu_row_passes_the_old_bar_and_fails_the_new(leg, N, extra):
    c = cc.prop_case(leg, N, extra)
    got = mc.propagate(c['P'], c['Phi'], c['Q'])
    i = _smallest_imu_state(c['ref64'], leg)
    fro0 = cc.frobenius(got, c['ref64'])
    got[i, :] *= 1.0 + 1e-13
    got[:, i] = got[i, :]
    fro = cc.frobenius(got, c['ref64'])
    print('planted 1e-13 in row %d: Frobenius %.2e (before: %.2e)' % (i, fro, fro0))
    assert fro < cc.OLD_FROBENIUS_BAR   # the old test could not see it
    assert _fails(cc.check_propagation, got, c['P'], c['ref'], c['bar'], leg)


def test_q_unsymmetrised_fails():
    c = cc.prop_case(22, 7, 0)
    leg = 22
    Q = c['Q'] + 1e-6 * np.triu(np.abs(c['Q']), 1)   # (a Q whose two triangles differ: the library takes (Q + Q^T) / 2)
    ref, bar = cc.prop_reference(c['P'], c['Phi'], Q)
    good = mc.propagate(c['P'], c['Phi'], Q)
    assert cc.check_propagation(good, c['P'], ref, bar, leg) < 0.5
    PP = c['Phi'] @ c['P'][:leg, :leg] @ c['Phi'].T
    bad = good.copy()
    bad[:leg, :leg] = 0.5 * (PP + PP.T) + Q          # Q as it stands
    assert _fails(cc.check_propagation, bad, c['P'], ref, bar, leg)
    bad[:leg, :leg] = 0.5 * (PP + PP.T) + np.triu(Q) + np.triu(Q, 1).T   # ... or its upper triangle mirrored: symmetric, outside the bar
    assert np.array_equal(bad, bad.T)
    assert _fails(cc.check_propagation, bad, c['P'], ref, bar, leg)


@pytest.mark.parametrize('leg,N,extra', [(22, 7, 1), (46, 3, 0)])
def test_cross_block_not_transposed_fails(leg, N, extra):
    c = cc.prop_case(leg, N, extra)
    bad = mc.propagate(c['P'], c['Phi'], c['Q'])
    bad[leg:, :leg] = c['P'][leg:, :leg] @ c['Phi']   # (P_CL Phi instead of P_CL Phi^T)
    assert _fails(cc.check_propagation, bad, c['P'], c['ref'], c['bar'], leg)
    bad[:leg, leg:] = bad[leg:, :leg].T               # ... on both sides: symmetric, outside the bar
    assert _fails(cc.check_propagation, bad, c['P'], c['ref'], c['bar'], leg)


def test_changed_clone_block_fails():
    c = cc.prop_case(22, 7, 1)
    bad = mc.propagate(c['P'], c['Phi'], c['Q'])
    bad[30, 31] = bad[31, 30] = np.nextafter(bad[30, 31], np.inf)
    assert _fails(cc.check_propagation, bad, c['P'], c['ref'], c['bar'], 22)


# ---- row maps ----------------------------------------------------------------------------------------------------------------------------
EDIT_CASES = [(leg, N, extra) for leg in (22, 46) for N in (0, 1, 8) for extra in (0, 9)]


@pytest.mark.parametrize('leg,N,extra', EDIT_CASES)
def test_row_maps_reproduce_the_mirror(leg, N, extra):
    n = leg + 6 * N + extra
    P = cc.graded_prior(n, 3)
    assert np.array_equal(cc.apply_map(P, cc.augment_map(n, extra)), mc.augment(P, rest=extra))
    for clones in ([0], [N - 1], list(range(N))):
        if N == 0 or clones[0] < 0:
            continue
        assert np.array_equal(cc.apply_map(P, cc.remove_clones_map(n, leg, clones)), mc.remove_clones(P, leg, clones))
        assert np.array_equal(cc.apply_map(P, cc.nuisance_map(n, leg, clones)), mc.clones_to_nuisance(P, leg, clones))
    if extra:
        for d, slots in ((1, [0, 4, 8]), (3, [0, 2]), (3, [1])):
            assert np.array_equal(cc.apply_map(P, cc.remove_features_map(n, leg, N, d, slots)), mfl.rm_lost_features_cov(P, leg, N, d, slots))


def test_row_map_mutations_fail():
    leg, N, extra = 22, 4, 9
    n = leg + 6 * N + extra
    P = cc.graded_prior(n, 3)
    ref = mc.augment(P, rest=extra)
    good = cc.augment_map(n, extra)
    assert np.array_equal(cc.apply_map(P, good), ref)
    rows36 = good.copy()
    rows36[n - extra + 3: n - extra + 6] = [3, 4, 5]            # the new clone takes rows 3:6 instead of 6:9
    assert not np.array_equal(cc.apply_map(P, rows36), ref)
    behind = cc.augment_map(n, 0)                               # the new clone behind the extra block
    assert not np.array_equal(cc.apply_map(P, behind), ref)
    # the rows of S left unmoved: what the device test compares (S_before[map]) differs from S_before[:m]
    X = cc.graded_factorable(n)
    S = np.linalg.cholesky(X)
    m = cc.remove_clones_map(n, leg, [0])
    assert not np.array_equal(S[:len(m)], S[m])
    assert np.allclose(S[m] @ S[m].T, cc.apply_map(X, m), rtol=1e-12, atol=0) and not np.allclose(S[:len(m)] @ S[:len(m)].T, cc.apply_map(X, m), rtol=1e-6, atol=0)


# ---- lost_unmap --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('augment', [False, True])
@pytest.mark.parametrize('name', list(cc.LOST_CASES))
def test_lost_unmap_restatement_equals_plain_deletion(name, augment):
    d, N, nf, slots = cc.LOST_CASES[name]
    n = cc.LOST_LEG + 6 * N + d * nf
    assert n == (170 if d == 1 else 172)
    got = cc.head_map(n, cc.LOST_LEG, N, d, nf, slots, augment)
    assert np.array_equal(got, cc.head_map_plain(n, cc.LOST_LEG, N, d, nf, slots, augment))
    P = cc.graded_prior(n, 9)
    if not augment:
        assert np.array_equal(cc.apply_map(P, got), mfl.rm_lost_features_cov(P, cc.LOST_LEG, N, d, slots))


# mutation -> the slot sets on which it MUST be seen (on the others it may or may not be)
LOST_MUTATIONS = {
    'off by one word': (dict(word_shift=1), ('bit63', 'bit64', 'last', 'every_second', 'idp3')),
    'without the carry': (dict(carry=False), ('bit63', 'bits63_64', 'word_edges', 'all_of_word0', 'every_second')),
    # (seen where a lost slot stands behind the last one that stays: what the set [129] is for)
    'nkeep short by one': (dict(nkeep_short=1), ('word_edges', 'last', 'idp3')),
}


@pytest.mark.parametrize('what', list(LOST_MUTATIONS))
def test_lost_unmap_mutations_fail(what):
    mut, must = LOST_MUTATIONS[what]
    for name in must:
        d, N, nf, slots = cc.LOST_CASES[name]
        n = cc.LOST_LEG + 6 * N + d * nf
        for augment in (False, True):
            assert not np.array_equal(cc.head_map(n, cc.LOST_LEG, N, d, nf, slots, augment, **mut),
                                      cc.head_map_plain(n, cc.LOST_LEG, N, d, nf, slots, augment)), (what, name, augment)


def test_every_word_and_the_last_word_stop_are_walked():
    """the slot sets reach words 0, 1 and 2 of the set; the walk's stop at the last word is reached with 512 slots"""
    words = set()
    for d, N, nf, slots in cc.LOST_CASES.values():
        words |= {s >> 6 for s in slots}
    assert words == {0, 1, 2}
    nf, slots = 512, tuple(range(0, 448)) + (500,)
    n = 22 + 6 + nf
    assert np.array_equal(cc.head_map(n, 22, 1, 1, nf, slots, False), cc.head_map_plain(n, 22, 1, 1, nf, slots, False))


# ---- tail, prefactor --------------------------------------------------------------------------------------------------------------------
def test_expected_tail_model_and_check():
    assert cc.expected_tail(['prefactor_rev']) == 15
    assert cc.expected_tail(['prefactor_rev', 'gather', 'permute', 'anchors']) == 15
    assert cc.expected_tail(['prefactor_rev', 'gather', 'augment']) == 0
    assert cc.expected_tail(['prefactor_rev', 'zupt', 'gather']) == 0
    assert cc.expected_tail(['prefactor_fwd', 'gather']) == 0
    n = 64
    X = cc.graded_factorable(n)
    S = pc.from_reversed(np.linalg.cholesky(pc.reverse(X)))   # the reversed form's factor: S S^T = X, rows >= 15 zero in the last 15 columns
    assert np.allclose(S @ S.T, X, rtol=1e-10, atol=0)
    cc.check_tail(S, 15)
    m = cc.remove_clones_map(n, 22, [0, 6])
    cc.check_tail(S[m], cc.expected_tail(['prefactor_rev', 'gather']))
    bad = S.copy()
    bad[40, n - 15] = 1e-300   # one non-zero entry in a column that the tail claims is zero
    assert _fails(cc.check_tail, bad, 15)
    aug = S[cc.augment_map(n, 0)]   # the new clone's rows are copies of rows 0:3, 6:9: not zero there
    assert _fails(cc.check_tail, aug, 15)
    cc.check_tail(aug, cc.expected_tail(['prefactor_rev', 'augment']))


@pytest.mark.parametrize('n', cc.PREFACTOR_N + (58, 63, 65, 76))
def test_factorable_priors_drop_no_pivot(n):
    X = cc.graded_factorable(n)   # (asserts inside)
    assert np.array_equal(X, X.T)
    assert cc.prefactor_reversed(n) == (n >= 31)
