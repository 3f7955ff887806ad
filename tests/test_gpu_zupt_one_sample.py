"""GPU tests of the checked stationary frames armed with ONE selected IMU sample (S < 2: checkZUPTIMU has nothing to test with):
orcvio_msckf_cov_zupt_frame_checked / _checked_hybrid run no check and no update -- propagation and augmentation stand, one wait on
the armed launch's status.  At the smallest window (leg 22, two clones behind the augmentation: n = 34; the hybrid form with one 1-d
feature state: n = 35), bit for bit against the separate calls cov_propagate_imu and cov_augment."""
import numpy as np
import pytest

from orcvio_amd import capi, synth
import imu_cases as ic

pytestmark = pytest.mark.gpu
LEG, N = 22, 2


@pytest.mark.parametrize('hybrid', [False, True], ids=['checked', 'checked_hybrid'])
def test_one_selected_sample_leaves_propagation_and_augmentation_and_nothing_else(built, hybrid):
    F = 1 if hybrid else 0
    n = LEG + 6 * N + F
    assert n == (35 if hybrid else 34)
    P0 = ic.make_cov(n - 6, np.random.default_rng(81 + F))
    r = 1e-3 * np.random.default_rng(82).standard_normal(9)
    case = ic.make_case('larvio', 1, n=LEG, seed=83, rate=200.0)
    chk = capi.MsckfUpdater.zupt_check(use_left=int(case['cfg'].use_left))
    a, c = (capi.MsckfUpdater(device=0, max_clones=8, max_features=64, max_observations=1024) for _ in range(2))
    try:
        for h in (a, c):
            h.set_extra_states(F)
            h.cov_set(P0)
        cfg, state, prev = ic.to_capi(case)
        a.io_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])
        if hybrid:
            got, verdict = a.cov_zupt_frame_checked_hybrid(chk, LEG, N, r, synth.ZUPT_NOISES, 1, F, True, True)
        else:
            got, verdict = a.cov_zupt_frame_checked(chk, LEG, N, r, synth.ZUPT_NOISES, True, True)
        assert (got['rc'], got['applied'], got['n_after']) == (0, 0, n)
        assert got['dx'].shape == (LEG + 6 * N if hybrid else n,) and not got['dx'].any()
        assert (verdict['evaluated'], verdict['accept'], verdict['dof'], verdict['status']) == (0, 0, 0, 0)   # no check ran
        cfg, state, prev = ic.to_capi(case)
        c.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])
        c.cov_augment()
        Pa, Pc = a.cov_get(), c.cov_get()
        assert Pa.shape == (n, n) and np.array_equal(Pa, Pc)
    finally:
        for h in (a, c):
            h.set_extra_states(0)
            h.close()
