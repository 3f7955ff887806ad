"""The UNFUSED form of the one-call frame in the PRODUCT library.  orcvio_msckf_io_step_frame folds propagation, augmentation and the
pull of the arena into one launch (k_frame_head) when Phi and Q fit into the input arena behind the frame's tracks; when they do
not, it takes the separate launches (k_cov_propagate_*, k_cov_augment, k_cov_remove with an index map) -- the form the other tests
reach only through ORCVIO_STEP_FUSED=0 on the diagnostics build."""
import numpy as np
import pytest

from orcvio_amd import capi, synth

pytestmark = pytest.mark.gpu
LEG, MAXN, F, TRACK = 46, 3, 8, 3
NOBS = F * TRACK


def _al256(x):
    return (x + 255) & ~255


def _inputs_bytes(N, nF, nobs, zvel, n_with_P):
    """capi_handle.inc inputs_bytes: [poses | obs_ptr | row_ptr | clone_ptr | p_w | obs_clone | clone_obs | obs_z | (obs_zvel) | (P)]."""
    return (_al256(8 * capi.POSE_STRIDE * N) + 2 * _al256(4 * (nF + 1)) + _al256(4 * (2 * N + 4)) + _al256(8 * 3 * nF) + 2 * _al256(4 * nobs) +
            _al256(8 * 2 * nobs) + (_al256(8 * 2 * nobs) if zvel else 0) + _al256(8 * n_with_P * n_with_P))


def _frame(seed, N, n_extra, rng):
    fl = synth.Flags(use_larvio=1, leg_dim=LEG)
    w = synth.make_window(N=N, F=F, seed=seed, track_len=TRACK, flags=fl, outlier_frac=0.0)
    w = synth.with_extra_states(w, n_extra, seed=seed)
    Phi = np.eye(LEG) + 0.002 * rng.standard_normal((LEG, LEG))
    G = rng.standard_normal((LEG, 12))
    return w, np.ascontiguousarray(Phi), np.ascontiguousarray(1e-7 * G @ G.T)


def _update(u, w, slam=None):
    io = u.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=False)
    u.io_fill(io, w, with_P=False)
    if slam:
        u.make_slam_call(1, slam)()
    u.io_update(want_P=False, commit=True)
    return io['dx'].copy(), io['gamma'].copy(), io['accept'].copy()


def test_the_unfused_fall_back_of_the_product_build_equals_the_separate_calls_bit_for_bit(built):
    """A handle of three clones whose window is at capacity, leg_dim 46: the fused head needs Phi and Q behind the frame's tracks,
    2 al256(8 46^2) = 34 304 bytes.  The arena was sized for the tracks WITH their image velocities and the prior P of n_max = 46 + 6 3 = 64
    states; a frame on the resident covariance without estimate_td leaves al256(8 64^2) = 32 768 bytes (the absent P) + al256(16 24) = 512
    bytes (the absent velocities of F x TRACK = 24 observations) = 33 280 < 34 304 (a two-clone frame: 256 bytes of poses more, 33 536), so
    `fused` is false in step_frame_impl and the product library takes the separate launches.  Three frames at capacity (propagation,
    augmentation to three clones, update, one of them with the prune update, the oldest clone removed), then a frame of two clones that
    loses one of its two in-state features (k_cov_remove with lost_features_map's index map) -- each against cov_propagate, cov_augment,
    cov_remove_features, io_update, cov_remove_clones: dx, gamma, accept and the covariance equal bit for bit after every frame."""
    n_max = LEG + 6 * MAXN
    in_cap = _inputs_bytes(MAXN, F, NOBS, True, n_max)
    need = 2 * _al256(8 * LEG * LEG)
    assert need == 34304 and _al256(8 * n_max * n_max) == 32768
    for N in (2, 3):   # off_aux + need <= in_cap is what the fused head asks for
        assert _al256(_inputs_bytes(N, F, NOBS, False, 0)) + need > in_cap, N
    rng = np.random.default_rng(7)
    a = capi.MsckfUpdater(device=0, max_clones=MAXN, max_features=F, max_observations=NOBS)
    b = capi.MsckfUpdater(device=0, max_clones=MAXN, max_features=F, max_observations=NOBS)
    try:
        P0 = synth.make_window(N=2, F=1, seed=5, flags=synth.Flags(use_larvio=1, leg_dim=LEG)).P
        a.cov_set(P0); b.cov_set(P0)
        for it in range(3):   # two clones resident, the third enters, the oldest leaves
            w, Phi, Q = _frame(100 + it, 3, 0, rng)
            prune = synth.subset_tracks(w, [0, 1], min_obs=2) if it == 1 else None
            assert prune is None or int(prune.obs_ptr[-1]) > 0
            a.cov_propagate(Phi, Q); a.cov_augment()
            ref = _update(a, w)
            ref2 = _update(a, prune) if prune is not None else None
            a.cov_remove_clones(LEG, [0])
            got = b.io_step_frame(w, Phi, Q, True, None, 1, prune, False, [0])
            assert got['rc'] == 0 and got['repaired'] == 0 and got['status_first'] == 0 and got['status_prune'] == 0, it
            assert np.array_equal(got['dx'], ref[0]), it
            assert np.array_equal(got['gamma'], ref[1], equal_nan=True) and np.array_equal(got['accept'], ref[2]), it
            if ref2 is not None:
                assert np.array_equal(got['prune_dx'], ref2[0]) and np.array_equal(got['prune_accept'], ref2[2]), it
            Pa, Pb = a.cov_get(), b.cov_get()
            assert got['n_after'] == Pa.shape[0] == Pb.shape[0] == LEG + 12 and np.array_equal(Pa, Pb), it
        # one clone and two in-state features (idp 1) resident; the frame augments to two clones and loses feature 0: 54 -> 60 -> 59 states
        w, Phi, Q = _frame(200, 2, 1, rng)
        slam = synth.make_slam_features(w, 1, seed=3)
        P1 = synth.with_extra_states(synth.make_window(N=1, F=1, seed=6, flags=w.flags), 2, seed=2).P
        for u in (a, b):
            u.set_ekf_rows_mode(True)
            u.cov_set(P1)
        a.set_extra_states(2)
        a.cov_propagate(Phi, Q); a.cov_augment()
        a.cov_remove_features(LEG, 2, 1, 2, [0])
        a.set_extra_states(1)
        ref = _update(a, w, slam)
        b.set_extra_states(1)
        got = b.io_step_frame_ex(win=w, Phi=Phi, Q=Q, augment=True, slam=slam, idp_dim=1, n_feature_states=2, lost=[0])
        assert got['rc'] == 0 and got['repaired'] == 0 and got['status_first'] == 0
        assert np.array_equal(got['dx'], ref[0])
        assert np.array_equal(got['gamma'], ref[1], equal_nan=True) and np.array_equal(got['accept'], ref[2])
        Pa, Pb = a.cov_get(), b.cov_get()
        assert got['n_after'] == Pa.shape[0] == Pb.shape[0] == LEG + 12 + 1 and np.array_equal(Pa, Pb)
    finally:
        a.close(); b.close()
