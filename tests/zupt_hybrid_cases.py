"""TEST INFRASTRUCTURE ONLY -- the stationary frame of a HYBRID filter: case table, float64 restatement and checkers, shared by
tests/test_zupt_hybrid_cases.py (CPU) and tests/test_gpu_zupt_hybrid.py.

When a zero-velocity check accepts a frame the reference deletes every in-state feature BEFORE measurementUpdate_ZUPT_vpq runs
(checkZUPTFeat src/orcvio.cpp:3102-3119, checkZUPTIMU :3302-3319: conservativeResize to b = leg + 6 N, feature_states.clear()); the
update runs on b states and pruneImuStateBuffer marginalises the previous clone (:2641-2645).  The restatement is that sentence:
oracle.mirror_cov propagate / augment, truncation to b, tests/mirror_zupt.measurement_update, mirror_cov.remove_clones.
Nothing under orcvio_amd/ may import this module."""
import numpy as np

from oracle import mirror_cov
import lifecycle_cases as lc
import mirror_zupt as mz

# name: (leg, N after augmentation, idp_dim d, feature states F)
CASES = {
    'min35': (22, 2, 1, 1),        # 35 -> 34: the smallest window; with remove_previous m = 28, one clone left
    'edge64': (22, 7, 1, 0),       # 64 -> 64: F = 0, exactly two tiles; the hole 52..57 moves rows 58..63 across nothing
    'edge65': (22, 7, 1, 1),       # 65 -> 64: the dropped feature alone in the last tile row / column and the factor kernel's 2nd workgroup
    'grid64': (22, 2, 1, 30),      # 64 -> 34: a full 5 x 6 grid behind the smallest window; fewer output tiles than input tiles
    'feat3d': (22, 3, 3, 3),       # 49 -> 40: d = 3
    'leg46': (46, 3, 3, 30),       # 154 -> 64: leg_dim 46 (unchecked call only)
    'ship232': (22, 20, 3, 30),    # 232 -> 142: the shipped window with a full grid at d = 3
}
VARIANTS = [(p, a, rm) for p in (0, 1) for a in (0, 1) for rm in (0, 1)]   # propagation given, augment, remove_previous


def dims(name):
    """leg, N, d, F, b, n"""
    leg, N, d, F = CASES[name]
    b = leg + 6 * N
    return leg, N, d, F, b, b + d * F


def prior(name, aug, seed=0):
    """the covariance resident BEFORE the frame (one clone less when the frame augments)"""
    n = dims(name)[5]
    return lc.spd(n - 6 * aug, 11 * n + aug + seed)


def frame_inputs(leg, seed):
    rng = np.random.default_rng(seed)
    Phi = np.eye(leg) + 1e-3 * rng.standard_normal((leg, leg))
    G = rng.standard_normal((leg, 12))
    return np.ascontiguousarray(Phi), np.ascontiguousarray(1e-8 * G @ G.T)


def residual(seed):
    rng = np.random.default_rng(900 + seed)
    return np.concatenate([2e-3 * rng.standard_normal(3), 1e-3 * rng.standard_normal(3), 5e-4 * rng.standard_normal(3)])


def head(P, d, F, Phi, Q, augment):
    """propagation and augmentation: what the update (or a rejected verdict) sees"""
    if Phi is not None:
        P = mirror_cov.propagate(P, Phi, Q)
    if augment:
        P = mirror_cov.augment(P, rest=d * F)
    return P


def hybrid_frame(P, leg, N, d, F, r, noises, Phi=None, Q=None, augment=True, remove_previous=True, accept=True):
    """The frame.  accept = False: the check rejected it (or the device refused): nothing leaves, nothing is updated."""
    b = leg + 6 * N
    P = head(P, d, F, Phi, Q, augment)
    assert P.shape[0] == b + d * F
    if not accept:
        return dict(dx=np.zeros(b), P=P, n_after=P.shape[0], applied=0)
    P = np.ascontiguousarray(P[:b, :b])                    # conservativeResize: the trailing d F rows and columns
    dx, P = mz.measurement_update(P, leg, N, r, *noises)
    if remove_previous:
        P = mirror_cov.remove_clones(P, leg, [N - 2])
    return dict(dx=dx, P=P, n_after=P.shape[0], applied=1)


def close(got, ref, what, tol=1e-12):
    """element by element within tol max|ref| (tests/test_gpu_zupt.py's bar; tests/test_zupt_mirror.py measures where it comes from)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    top = np.abs(ref).max()
    err = np.abs(got - ref).max() if ref.size else 0.0
    print(f'{what}: max err {err:.3e}, max |ref| {top:.3e}')
    assert err <= tol * top, (what, err, top)


def check_frame(got, ref, tol=1e-12):
    """a frame's result dict(dx, P, n_after, applied) against the restatement's"""
    assert got['applied'] == ref['applied'], ('applied', got['applied'], ref['applied'])
    assert got['n_after'] == ref['n_after'], ('n_after', got['n_after'], ref['n_after'])
    assert got['P'].shape == (ref['n_after'], ref['n_after']), ('shape of P', got['P'].shape)
    close(got['P'], ref['P'], 'P', tol)
    if ref['applied']:
        assert np.array_equal(got['P'], got['P'].T), 'P+ is not exactly symmetric'
        close(got['dx'], ref['dx'], 'dx', tol)
    else:
        assert got['dx'].shape == ref['dx'].shape and not np.asarray(got['dx']).any(), 'dx behind a frame that was not applied'


def _sym(P):
    return (P + P.T) / 2.0


# ---- mutations: each a plausible wrong frame; check_frame must fail every one (None: the mutation is the frame itself on this case)
def mutations(P0, leg, N, d, F, r, noises, Phi, Q, augment, remove_previous):
    b = leg + 6 * N
    P = head(P0, d, F, Phi, Q, augment)
    n = P.shape[0]
    rm = [N - 2] if remove_previous else []
    out = {}

    def finish(dx, Pp, clones=rm):
        Pp = mirror_cov.remove_clones(Pp, leg, clones) if clones else Pp
        return dict(dx=dx, P=_sym(Pp), n_after=Pp.shape[0], applied=1)

    dx_full, P_full = mz.measurement_update(P, leg, N, r, *noises)
    out['features kept'] = finish(dx_full[:b], P_full) if F else None
    if d * F >= 1:
        dx1, P1 = mz.measurement_update(np.ascontiguousarray(P[:b + 1, :b + 1]), leg, N, r, *noises)
        out['prefix b+1'] = finish(dx1[:b], P1)
    else:
        out['prefix b+1'] = None
    dxb, Pb = mz.measurement_update(np.ascontiguousarray(P[:b, :b]), leg, N, r, *noises)
    good = finish(dxb, Pb)
    out['prefix b-1'] = dict(dx=dxb, P=np.ascontiguousarray(good['P'][:-1, :-1]), n_after=good['n_after'] - 1, applied=1)
    out['previous clone not removed'] = finish(dxb, Pb, []) if remove_previous else None
    out['newest clone removed'] = finish(dxb, Pb, [N - 1]) if remove_previous else None
    out['dx at a shifted offset'] = dict(good, dx=np.ascontiguousarray(dx_full[1:b + 1])) if F else None
    return out


def mutation_rejected(P0, leg, N, d, F, Phi, Q, augment):
    """truncation applied on a rejected verdict"""
    if not F:
        return None
    b = leg + 6 * N
    P = head(P0, d, F, Phi, Q, augment)
    return dict(dx=np.zeros(b), P=_sym(P[:b, :b]), n_after=b, applied=0)
