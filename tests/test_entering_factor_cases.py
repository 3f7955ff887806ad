"""CPU: the float64 restatement of the augmented square-root factor (tests/entering_factor_cases.py) against its extended-precision
reference over every case of tests/entering_cases.py and three factor shapes -- its worst block errors are what G_TOL, RINV_TOL and
SST_TOL are 100 times of -- and the mutations: each planted fault fails the check it is there for."""
import numpy as np
import pytest

import entering_cases as ec
import entering_factor_cases as fc

IDS = [str(c) for c in ec.CASES]
SLACK = 4.0   # the recorded worst errors were measured with one BLAS; another summation order may move them by a small factor


def inputs(cid, shape):
    """(H_1, H_2, r_1, S+, sigma, tail, P+ = S+ S+^T rounded once) of one case with a factor of the given shape"""
    case = ec.make_case(cid)
    H_1, H_2, r_1, _, _, _ = ec.restatement_split(case)
    S = fc.factor_of(case.win.P, shape)
    return H_1, H_2, r_1, S, case.win.flags.noise_feature, case.tail, fc.covariance_of(S)


def measure(cid, shape):
    H_1, H_2, r_1, S, sigma, tail, P = inputs(cid, shape)
    n, kf = S.shape
    sz = cid.d * cid.k
    got = fc.s_aug_f64(H_1, H_2, r_1, S, sigma, tail, cid.ldlt)
    ref = fc.s_aug_ext(H_1, H_2, r_1, S, sigma, tail, cid.ldlt)
    P_aug = ec.tail_ext(H_1, H_2, r_1, np.zeros(n), P, sigma ** 2, tail, ref_ldlt=cid.ldlt)['P_aug']
    assert got['S_aug'].shape == (n + sz, kf + sz) and P_aug.shape == (n + sz, n + sz)
    bad, fig = fc.violations(got['S_aug'], S, ref, cid.d, tail, P_aug)
    # the reference itself: its own product against P_aug (what the identity holds to in extended precision, P+ rounded once)
    fig['ref_sst'] = fc.sst_err(ref['S_aug'], P_aug, n, sz, tail)
    return bad, fig


def test_factor_shapes_are_what_they_are_named():
    case = ec.make_case(ec.CaseId('small', 3, 6))
    n = case.win.n
    assert [fc.factor_of(case.win.P, s).shape for s in fc.FACTOR_SHAPES] == [(n, n), (n, n - 6), (n, n + 6)]


@pytest.mark.parametrize('cid', ec.CASES, ids=IDS)
def test_float64_restatement_of_the_factor_agrees_with_the_extended_reference(cid):
    for shape in fc.FACTOR_SHAPES:
        bad, fig = measure(cid, shape)
        print('entering-factor %s %s: %s' % (cid, shape, {q: '%.2e' % v for q, v in fig.items()}))
        assert not bad, (shape, bad, fig)
        assert fig['G'] <= SLACK * fc.G_WORST and fig['own'] <= SLACK * fc.RINV_WORST and fig['sst'] <= SLACK * fc.SST_WORST, (shape, fig)
        assert fig['ref_sst'] <= fc.SST_WORST, (shape, fig)
    assert fc.G_TOL == 100 * fc.G_WORST and fc.RINV_TOL == 100 * fc.RINV_WORST and fc.SST_TOL == 100 * fc.SST_WORST


def test_under_ref_ldlt_only_hh_changes():
    """HH divides by diag(H_2) under ORCVIO_OPT_REF_H2_LDLT, the factor's own block does not: G differs, sigma R^-1 does not."""
    H_1, H_2, r_1, S, sigma, tail, _ = inputs(ec.CaseId('small', 3, 6, ldlt=True), 'square')
    a = fc.s_aug_ext(H_1, H_2, r_1, S, sigma, tail, True)
    b = fc.s_aug_ext(H_1, H_2, r_1, S, sigma, tail, False)
    assert np.array_equal(a['sRinv'], b['sRinv'])
    assert ec.block_err(a['G'], b['G']) > 1e3 * fc.G_TOL


MUTATIONS = ['sign of G', 'R^-T for R^-1', 'sigma missing', 'new rows behind the nuisance block', 'a stale old row']


@pytest.mark.parametrize('what', MUTATIONS)
def test_each_mutation_fails_its_check(what):
    cid = ec.CaseId('schmidt', 3, 6)   # nuisance states (the order of the rows matters), d = 3 (R^-1 is not symmetric), sigma != 1
    H_1, H_2, r_1, S, sigma, tail, P = inputs(cid, 'square')
    assert tail == 12 and sigma != 1.0
    n, kf = S.shape
    sz, d = 18, 3
    ref = fc.s_aug_ext(H_1, H_2, r_1, S, sigma, tail)
    P_aug = ec.tail_ext(H_1, H_2, r_1, np.zeros(n), P, sigma ** 2, tail)['P_aug']
    good = fc.s_aug_f64(H_1, H_2, r_1, S, sigma, tail)['S_aug']
    assert fc.violations(good, S, ref, d, tail, P_aug)[0] == []
    n0 = n - tail
    new = slice(n0, n0 + sz)
    m = good.copy()
    if what == 'sign of G':
        m[new, :kf] = -m[new, :kf]
        expect = {'G', 'S S^T'}
    elif what == 'R^-T for R^-1':
        for j in range(6):
            q, c = slice(n0 + d * j, n0 + d * j + d), slice(kf + d * j, kf + d * j + d)
            m[q, c] = m[q, c].T.copy()
        expect = {'sigma R^-1', 'S S^T'}
    elif what == 'sigma missing':
        m[new, kf:] = m[new, kf:] / sigma
        expect = {'sigma R^-1', 'S S^T'}
    elif what == 'new rows behind the nuisance block':
        m = np.vstack([good[:n0], good[n0 + sz:], good[new]])
        expect = {'old rows', 'zero block', 'G', 'sigma R^-1', 'off the diagonal blocks', 'S S^T'}
    else:
        m[20] = good[20] * (1 + 1e-13)     # a row of another factor of the same state, 1e-13 off
        expect = {'old rows', 'S S^T'}
    bad, fig = fc.violations(m, S, ref, d, tail, P_aug)
    print('mutation %r: fails %s, figures %s' % (what, bad, {q: '%.2e' % v for q, v in fig.items()}))
    assert bad and set(bad) <= expect, (bad, fig)
    # ... and the check that is there for it is among them
    first ={'sign of G': 'G', 'R^-T for R^-1': 'sigma R^-1', 'sigma missing': 'sigma R^-1',
             'new rows behind the nuisance block': 'old rows', 'a stale old row': 'old rows'}[what]
    assert first in bad, (first, bad)
