"""The checkers of the hybrid stationary frame (tests/zupt_hybrid_cases.py) on the CPU: they accept the restatement, they fail every
mutation of it, and the algebraic fact the fused kernel rests on holds in float64 on every case -- the leading b x b block of the
update on the full n states IS the update on the truncated covariance, because H has no column behind b."""
import numpy as np
import pytest

from orcvio_amd import synth
import mirror_zupt as mz
import zupt_hybrid_cases as zh

NOISES = synth.ZUPT_NOISES


def _inputs(name, prop, aug):
    leg, N, d, F, b, n = zh.dims(name)
    Phi, Q = zh.frame_inputs(leg, n) if prop else (None, None)
    return zh.prior(name, aug), zh.residual(n), Phi, Q


@pytest.mark.parametrize('name', list(zh.CASES))
@pytest.mark.parametrize('prop,aug,rm', zh.VARIANTS)
def test_the_checkers_accept_the_restatement_and_fail_every_mutation(name, prop, aug, rm):
    leg, N, d, F, b, n = zh.dims(name)
    P0, r, Phi, Q = _inputs(name, prop, aug)
    ref = zh.hybrid_frame(P0, leg, N, d, F, r, NOISES, Phi, Q, bool(aug), bool(rm))
    assert ref['n_after'] == b - 6 * rm and ref['dx'].shape == (b,)
    zh.check_frame(ref, ref)
    failed = 0
    for what, mut in zh.mutations(P0, leg, N, d, F, r, NOISES, Phi, Q, bool(aug), bool(rm)).items():
        if mut is None:
            continue
        with pytest.raises(AssertionError):
            zh.check_frame(mut, ref)
        failed += 1
    assert failed >= (6 if (F and rm) else 1)
    rej = zh.hybrid_frame(P0, leg, N, d, F, r, NOISES, Phi, Q, bool(aug), bool(rm), accept=False)
    assert rej['n_after'] == n and rej['applied'] == 0
    zh.check_frame(rej, rej)
    mut = zh.mutation_rejected(P0, leg, N, d, F, Phi, Q, bool(aug))
    if mut is not None:
        with pytest.raises(AssertionError):
            zh.check_frame(mut, rej)


@pytest.mark.parametrize('name', list(zh.CASES))
def test_the_leading_block_of_the_full_update_is_the_update_of_the_truncated_covariance(name):
    leg, N, d, F, b, n = zh.dims(name)
    P = zh.head(zh.prior(name, 1), d, F, *zh.frame_inputs(leg, n), True)
    r = zh.residual(n)
    dx_full, P_full = mz.measurement_update(P, leg, N, r, *NOISES)
    dx_cut, P_cut = mz.measurement_update(np.ascontiguousarray(P[:b, :b]), leg, N, r, *NOISES)
    zh.close(P_full[:b, :b], P_cut, 'leading block of P+')
    zh.close(dx_full[:b], dx_cut, 'dx[0:b]')
