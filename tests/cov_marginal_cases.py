"""Cases, references and the checker of the resident covariance's marginals (orcvio_msckf_cov_get_marginal: out = P[idx, idx], or
T P[idx, idx] T^T), shared by tests/test_cov_marginal_cases.py (CPU) and tests/test_gpu_cov_marginal*.py.

  make_P / make_idx / make_T   the inputs: P deliberately ASYMMETRIC (cov_set stores what it is given, and the reference reads P_po and
                               P_op separately), random or graded over fourteen decades; idx ascending, reversed, permuted, with a
                               repeat, containing 0 and n - 1
  restate                      the float64 restatement
  exact                        the same in 60-digit arithmetic (mpmath, as oracle/mp_reference.py), computed once per case
  literal_getters              getPpose() / getPvel() (src/orcvio.cpp:2999-3026) statement by statement in numpy
  odometry_spec                the ONE spec the host layer's getters use (host/cov_marginal_spec.hpp)
  check                        the bar, derived and not measured: each of the two products is a sum of n_idx terms, so whatever the order
                               of the sums (gamma_k <= k u / (1 - k u), twice, and the cross term)

                                   |out - exact|_ij <= (2 n_idx + 4) 2^-53 (|T| |P_m| |T|^T)_ij          componentwise

                               and the gather (m == 0) is bit for bit.
  planted                      the errors the checks must catch
"""
import functools

import mpmath as mp
import numpy as np

U = 2.0 ** -53
MARGINAL_MAX = 64
# (n_idx, m) of the issue: m below and above n_idx, one and sixty-four, beside and on the sixteens
N_IDX = (1, 2, 9, 16, 17, 63, 64)
M_ROWS = (0, 1, 6, 9, 17, 64)
IDX_KINDS = ('ascending', 'reversed', 'permuted', 'repeat', 'ends')
P_KINDS = ('asym', 'graded')
ODOMETRY_IDX = (6, 7, 8, 0, 1, 2, 3, 4, 5)


def make_P(n, kind='asym', seed=0):
    """[n][n], asymmetric.  graded: sqrt(d_i d_j) A_ij with d over fourteen decades (1e3 .. 1e-11), as a filter's covariance is graded
    between its positions and its biases."""
    rng = np.random.default_rng(1000 + 17 * n + seed)
    A = rng.standard_normal((n, n))
    if kind == 'asym':
        return A
    if kind == 'graded':
        d = 10.0 ** np.linspace(3.0, -11.0, n) if n > 1 else np.ones(1)
        d = d[rng.permutation(n)]
        return A * np.sqrt(np.outer(d, d))
    raise ValueError(kind)


def make_idx(n, k, kind, seed=0):
    """k state indices of a covariance of dimension n (k <= n except with repeats)."""
    rng = np.random.default_rng(2000 + 31 * n + 7 * k + seed)
    if kind == 'repeat':
        ix = rng.integers(0, n, size=k)
        if k >= 2:
            ix[-1] = ix[0]
        return ix.astype(np.int32)
    assert k <= n, (k, n)
    pick = np.sort(rng.choice(n, size=k, replace=False))
    if kind == 'ascending':
        ix = pick
    elif kind == 'reversed':
        ix = pick[::-1]
    elif kind == 'permuted':
        ix = pick[rng.permutation(k)]
    elif kind == 'ends':   # 0 and n - 1 among them (k == 1: n - 1 alone), not at the ends of the list
        ix = pick.copy()
        ix[0] = n - 1
        if k >= 2:
            ix[-1] = 0
            if k >= 3:
                inner = np.sort(rng.choice(np.arange(1, n - 1), size=k - 2, replace=False))
                ix[1:-1] = inner
                ix = np.roll(ix, 1)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(ix, dtype=np.int32)


def make_T(m, k, seed=0):
    return np.random.default_rng(3000 + 64 * m + k + seed).standard_normal((m, k))


def gather(P, idx):
    ix = np.asarray(idx, dtype=np.int64)
    return P[np.ix_(ix, ix)]


def restate(P, idx, T=None):
    """float64: the gather, then Y = T P_m, then out = Y T^T."""
    Pm = gather(P, idx)
    if T is None:
        return Pm.copy()
    Y = T @ Pm
    return Y @ T.T


def _mp_rows(a):
    return [[mp.mpf(float(v)) for v in row] for row in np.asarray(a, dtype=np.float64)]


def exact_of(Pm, T):
    """T P_m T^T in 60-digit arithmetic: [m][m] of mpf (mp.fdot sums a row's products exactly and rounds once to 60 digits)."""
    with mp.workdps(60):
        Pc = _mp_rows(np.asarray(Pm).T)   # columns of P_m
        Tr = _mp_rows(T)
        Y = [[mp.fdot(t, c) for c in Pc] for t in Tr]
        return [[mp.fdot(y, t) for t in Tr] for y in Y]


def bound_of(Pm, T):
    k = Pm.shape[0]
    return (2 * k + 4) * U * (np.abs(T) @ np.abs(Pm) @ np.abs(T).T)


def errors(out, ex):
    """|out - exact| componentwise, the difference taken in 60 digits."""
    out = np.asarray(out, dtype=np.float64)
    with mp.workdps(60):
        return np.array([[float(abs(mp.mpf(float(out[i, j])) - ex[i][j])) for j in range(out.shape[1])] for i in range(out.shape[0])])


class Case:
    """One request on one covariance; the 60-digit value is computed on first use and kept."""

    def __init__(self, n, k, m, idx_kind='permuted', p_kind='asym', seed=0, P=None, idx=None, T=None):
        self.n, self.k, self.m, self.idx_kind, self.p_kind = n, k, m, idx_kind, p_kind
        self.P = make_P(n, p_kind, seed) if P is None else np.asarray(P, dtype=np.float64)
        self.idx = make_idx(n, k, idx_kind, seed) if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        self.T = (make_T(m, k, seed) if m > 0 else None) if T is None else np.ascontiguousarray(T, dtype=np.float64)
        self.Pm = gather(self.P, self.idx)

    @functools.cached_property
    def exact(self):
        return exact_of(self.Pm, self.T)

    @functools.cached_property
    def bound(self):
        return bound_of(self.Pm, self.T)

    def __repr__(self):
        return 'n%d_k%d_m%d_%s_%s' % (self.n, self.k, self.m, self.idx_kind, self.p_kind)


def check(case, out, what=''):
    """The gather bit for bit, the congruence inside the derived bar componentwise.  Returns the largest fraction of the bar used."""
    out = np.asarray(out, dtype=np.float64)
    if case.m == 0:
        assert out.shape == case.Pm.shape, (what, out.shape)
        assert np.array_equal(out, case.Pm, equal_nan=True), (what, repr(case), 'the gather is not bit for bit')
        return 0.0
    assert out.shape == (case.m, case.m), (what, out.shape)
    err, bar = errors(out, case.exact), case.bound
    assert np.all(err <= bar), (what, repr(case), float(np.max(err - bar)), np.unravel_index(np.argmax(err - bar), err.shape))
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(bar > 0, err / bar, 0.0)
    return float(np.max(frac))


def passes(case, out):
    try:
        check(case, out)
    except AssertionError:
        return False
    return True


@functools.lru_cache(maxsize=None)
def shape_case(n, k, m, idx_kind='permuted', p_kind='asym', seed=0):
    return Case(n, k, m, idx_kind, p_kind, seed)


def shape_cases(n=73):
    """every (n_idx, m) of the issue on a covariance of dimension n >= 64, the kinds of idx and of P taken in turn"""
    out = []
    for a, k in enumerate(N_IDX):
        for b, m in enumerate(M_ROWS):
            kind = IDX_KINDS[(a + 2 * b) % len(IDX_KINDS)]
            if kind == 'ends' and k == 1:
                kind = 'ascending'
            out.append(shape_case(n, k, m, kind, P_KINDS[(a + b) % 2]))
    return out


def kind_cases(n):
    """every kind of idx against both kinds of P at one shape that fits any handle (9 of n >= 22, rows below and above)"""
    return [shape_case(n, 9, m, kind, pk) for kind in IDX_KINDS for pk, m in (('asym', 6), ('graded', 17))] + \
           [shape_case(n, 9, 0, kind, 'graded') for kind in IDX_KINDS]


# ---- the odometry getters -----------------------------------------------------------------------------------------------------------
def rotation(seed=0):
    q, r = np.linalg.qr(np.random.default_rng(4000 + seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return np.ascontiguousarray(q)


def odometry_spec(R, order=ODOMETRY_IDX):
    """idx = {6,7,8, 0,1,2, 3,4,5}, T = blkdiag(R, R, R): the leading 6 x 6 of the result is getPpose()'s matrix, the trailing 3 x 3
    getPvel()'s."""
    T = np.zeros((9, 9))
    for b in range(3):
        T[3 * b:3 * b + 3, 3 * b:3 * b + 3] = R
    return np.array(order, dtype=np.int32), T


def literal_getters(P, R):
    """getPpose() and getPvel(), src/orcvio.cpp:2999-3026, statement by statement."""
    P_oo = P[0:3, 0:3]
    P_op = P[0:3, 6:9]
    P_po = P[6:9, 0:3]
    P_pp = P[6:9, 6:9]
    P_imu_pose = np.block([[P_pp, P_po], [P_op, P_oo]])
    H_pose = np.zeros((6, 6))
    H_pose[0:3, 0:3] = R
    H_pose[3:6, 3:6] = R
    P_body_pose = H_pose @ P_imu_pose @ H_pose.T
    P_imu_vel = P[3:6, 3:6]
    H_vel = R
    P_body_vel = H_vel @ P_imu_vel @ H_vel.T
    return P_body_pose, P_body_vel


def odometry_case(n, p_kind='asym', seed=0):
    R = rotation(seed)
    idx, T = odometry_spec(R)
    c = Case(n, 9, 9, 'odometry', p_kind, seed, idx=idx, T=T)
    c.R = R
    return c


def getters_as_block(pose, vel):
    """the literal getters' two matrices where the 9 x 9 result has them; the pose / velocity cross blocks are not theirs (NaN)"""
    out = np.full((9, 9), np.nan)
    out[0:6, 0:6] = pose
    out[6:9, 6:9] = vel
    return out


def check_getters(case, pose, vel, what=''):
    """the two matrices against the 60-digit 9 x 9 of the spec, inside the bar, on the blocks the getters define"""
    blk = getters_as_block(pose, vel)
    err, bar = errors(np.nan_to_num(blk), case.exact), case.bound
    mask = ~np.isnan(blk)
    assert np.all(err[mask] <= bar[mask]), (what, float(np.max((err - bar)[mask])))
    return float(np.max((err / bar)[mask]))


# ---- planted errors -------------------------------------------------------------------------------------------------------------------
PLANTED = ('T_transposed', 'idx_rows_only', 'Pm_transposed', 'symmetrised', 'sum_cut_short')


def planted(case, kind):
    """what a wrong implementation would return for the case (congruences: m == n_idx where T is used transposed)"""
    P, ix, T = case.P, np.asarray(case.idx, dtype=np.int64), case.T
    Pm = case.Pm
    if kind == 'idx_rows_only':
        Pm_bad = P[ix][:, :len(ix)]
        return Pm_bad.copy() if T is None else T @ Pm_bad @ T.T
    if kind == 'Pm_transposed':
        return Pm.T.copy() if T is None else T @ Pm.T @ T.T
    if kind == 'T_transposed':
        return T.T @ Pm @ T
    if kind == 'symmetrised':
        out = restate(P, case.idx, T)
        return 0.5 * (out + out.T)
    if kind == 'sum_cut_short':
        return (T[:, :-1] @ Pm[:-1, :]) @ T.T
    raise ValueError(kind)
