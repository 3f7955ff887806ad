"""Inputs, measures and references of the Cholesky-chain tests (CPU: tests/test_potrf_cases.py, device: tests/test_gpu_potrf_tiles.py).

Matrices.  graded(n, seed, cond, decades): a correlation matrix of the given condition (eigenvalues log-spaced, unit diagonal after
rescaling) times s s^T, s log-spaced over `decades` and randomly permuted -- a prior whose sigmas run over four decades, correlated.
prior(n): imu_cases.make_cov (zero rows and columns at the states 15 .. 21, n = 22 + 6 N + extra).

Measures, evaluated in np.longdouble (64-bit mantissa; mpmath where the platform's long double is no wider than a double), in units of
u = 2^-52:
  omega_tiles(L, X): for every 16 x 16 tile, max |L L^T - X| over the tile / max (|L| |L|^T) over the tile; the largest tile value.
  omega_solve(L, Z, B): for every 16-row x 16-column tile, max |L Z - B| / max (|L| |Z| + |B|).
A tile whose denominator is zero must have a zero residual (otherwise the measure is infinite).  Tile-wise, not element-wise, on
purpose: element-wise ratios have a heavy tail from tiny denominators, the tile maximum does not -- and it still sees a relative error
of 1e-9 in the row of the smallest state, which the Frobenius-norm comparisons of tests/test_gpu_kernels.py miss by orders of
magnitude (tests/test_potrf_cases.py::test_planted_error_*).

References (never the code under test): (a) np.linalg.cholesky on the kept submatrix (zero-variance states removed) and a row-by-row
forward substitution; (b) tile_chol / tile_solve, a float64 mirror of the device's tile algorithm: 16 x 16 diagonal tiles, explicit
inv(L11) (by substitution, as the device's sweep forms it), panel = X21 inv(L11)^T, pivots <= tol_rel * max diag dropped (zero column), the solve multiplying by inv(L11) block step by
block step.  The mirror carries the one property LAPACK lacks, the inverse-based panel.

Bar.  Per case, ten times the larger of (a)'s and (b)'s own figure on that case, computed in the test run (the factor of ten is the
project's precedent, imu_cases.REGRESSION_BAR: the device sums in another order -- 4-wide MFMA chunks, the DPP sweep).

Recorded figures, worst case in units of u (tests/test_potrf_cases.py measures the references' and asserts them within a factor of two):
  factor, graded cond 1e2 / 1e4 / 1e6 and prior over FACTOR_N, forward and reversed:  LAPACK 5.1, mirror 2.7
  solve, graded cond 1e4 / 1e6 over SOLVE_N x SOLVE_NC1 (with the column bx):         LAPACK 0.72, mirror 1.02
  device (MI355X), worst over tests/test_gpu_potrf_tiles.py (DEVICE_WORST; the bar of that very case, and the largest figure / bar):
    k_potrf_reg, forward and reversed      17.8  (graded cond 1e4, n = 224, reversed; bar 27.9; at most 0.77 of a bar)
    k_front's chol(P) after a real update  11.7  (prior, n = 220; bar 21.9; at most 0.59 of a bar)
    k_potrf_solve, k_potrf_solve_la 2 / 3  factor 10.5 (cond 1e4, n = 224; bar 26.2; 0.40), solve 3.8 (n = 192, 210 columns; bar 7.5;
                                           at most 0.83 of a bar) -- the three kernels agree bit for bit on every case
Information only, no assertion: element-wise (max over the entries of |L L^T - X| / (|L| |L|^T), graded cond 1e6 over FACTOR_N)
LAPACK gives 0.9 .. 7.2 u, the mirror 1.1 .. 2.3 u and k_potrf_reg on the device 1.2 .. 11.5 u: the inverse-based panel is as good as a
triangular solve as long as inv(L11) itself is accurate entry by entry, which the substitution on the identity's columns (the
device's sweep, _tri_inv) is.  It is the LU-based inverse that is not: the same mirror with np.linalg.inv gives 1.1 .. 41 000 u
(8 200 u at cond 1e2, n = 113: the grading is enough), while tile by tile it still reads about 1 u (ELEMENTWISE_*).
"""
from __future__ import annotations

import functools

import numpy as np

import imu_cases

LD = np.longdouble
U = float(np.finfo(np.float64).eps)   # 2.2e-16
TS = 16
TOL_PRIOR = 8.0 * U                   # the update's tol_rel for chol(P)
BAR_FACTOR = 10.0                     # (imu_cases.REGRESSION_BAR's factor)
LD_WIDE = bool(np.finfo(LD).eps < 1e-18)

CONDS = (1e2, 1e4, 1e6)
# block steps nb = ceil(n / 16): 1, 2, each boundary of the four register-slot instantiations of k_potrf_reg / k_potrf_solve
# (potrf_slots_needed(nb) = ceil(nb (nb - 1) / 12) <= 4, 8, 12, 16: nb <= 7, 10, 12, 14 -- one n short of the last full tile, at it, and
# the first n of the next instantiation) and nb = 14 with one row in the last tile, one row short of full, and full
FACTOR_N = (16, 17, 111, 112, 113, 159, 160, 161, 191, 192, 193, 209, 223, 224)
# nb = 5 | 6: la_solve_active and the far workgroups begin; 7: odd nb (padding step nb2); 12; 14 with one row in the last tile and full
SOLVE_N = (80, 96, 112, 192, 209, 224)
# with bx the column count is nc1 + 1: 2, 16, 17, 64 (one solver workgroup), 65 (two), 210
SOLVE_NC1 = (1, 15, 16, 63, 64, 209)
TAIL = 15
TAIL_SCALE = 1.0 / 0.0123

# ---- recorded figures (units of u) -------------------------------------------------------------------------------------------------
REF_FACTOR_LAPACK = 5.1    # measured 5.085 (graded cond 1e6)
REF_FACTOR_MIRROR = 2.7    # measured 2.733
REF_SOLVE_LAPACK = 0.72    # measured 0.718
REF_SOLVE_MIRROR = 1.02    # measured 1.020
ELEMENTWISE_LAPACK_1E6 = (0.9, 7.2)       # (smallest, largest) over FACTOR_N, graded cond 1e6 -- information only
ELEMENTWISE_MIRROR_1E6 = (1.1, 2.3)
ELEMENTWISE_MIRROR_LU_INVERSE_1E6 = (1.1, 41431.0)
DEVICE_ELEMENTWISE_1E6 = (1.2, 11.5)      # k_potrf_reg, forward and reversed, measured on the MI355X
DEVICE_WORST = {'k_potrf_reg': 17.8, 'k_front': 11.7, 'k_potrf_solve factor': 10.5, 'k_potrf_solve solve': 3.8,
                'k_potrf_solve_la factor': 10.5, 'k_potrf_solve_la solve': 3.8}   # measured on the MI355X, information only


# ---- matrices ----------------------------------------------------------------------------------------------------------------------
def _spd(n, seed, cond):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.logspace(0, -np.log10(cond), n)
    return (Q * ev) @ Q.T


def graded_scales(n, seed, decades=4):
    rng = np.random.default_rng(seed + 7919)
    return np.logspace(0, -decades, n)[rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def _graded(n, seed, cond, decades):
    C = _spd(n, seed, cond)
    d = np.sqrt(np.diag(C))
    C = C / np.outer(d, d)
    s = graded_scales(n, seed, decades)
    G = C * np.outer(s, s)
    G = np.ascontiguousarray(0.5 * (G + G.T))
    np.fill_diagonal(G, s * s)   # (the unit diagonal of the correlation matrix exactly: the largest entry is exactly 1)
    G.setflags(write=False)
    return G


def graded(n, seed, cond, decades=4):
    """read-only: copy before editing"""
    return _graded(int(n), int(seed), float(cond), int(decades))


@functools.lru_cache(maxsize=None)
def prior(n):
    P = imu_cases.make_cov(int(n), np.random.default_rng(int(n)))
    P.setflags(write=False)
    return P


DEAD = tuple(range(15, 22))   # prior(n)'s zero-variance states


def reverse(X):
    """X'(i, j) = X(n-1-i, n-1-j)"""
    return np.ascontiguousarray(X[::-1, ::-1])


def rhs(n, nc, seed):
    """right-hand sides with graded rows (the prior's factor, transposed, is what the update solves for)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, nc)) * graded_scales(n, seed + 1)[:, None]


# ---- measures ----------------------------------------------------------------------------------------------------------------------
def _mm(A, B):
    """A @ B in extended precision: long double where it is wider than double, else mpmath (113 bits)"""
    if LD_WIDE:
        return np.asarray(A, dtype=LD) @ np.asarray(B, dtype=LD)
    return _mm_mp(A, B)


def _mm_mp(A, B):
    import mpmath
    with mpmath.workprec(113):
        C = mpmath.matrix(np.asarray(A, dtype=np.float64).tolist()) * mpmath.matrix(np.asarray(B, dtype=np.float64).tolist())
        return np.array([[C[i, j] for j in range(C.cols)] for i in range(C.rows)], dtype=object)


def _sub_abs(C, X):
    """|C - X| for an extended-precision C (long double or mpmath entries) and a float64 X, rounded to float64 at the end"""
    if C.dtype == object:
        return np.array([[float(abs(C[i, j] - float(X[i, j]))) for j in range(C.shape[1])] for i in range(C.shape[0])])
    return np.abs(C - np.asarray(X, dtype=LD)).astype(np.float64)


def _tile_worst(R, D, ts=TS):
    worst = 0.0
    for i in range(0, R.shape[0], ts):
        for j in range(0, R.shape[1], ts):
            r = float(R[i:i + ts, j:j + ts].max())
            d = float(D[i:i + ts, j:j + ts].max())
            if not (r == r and d == d):
                return float('inf')   # (a NaN anywhere)
            if d == 0.0:
                if r != 0.0:
                    return float('inf')
                continue
            worst = max(worst, r / d)
    return worst / U


def factor_fields(L, X):
    """(|L L^T - X|, |L| |L|^T) as float64 arrays"""
    R = _sub_abs(_mm(L, L.T), X)
    D = np.asarray(_mm(np.abs(L), np.abs(L).T), dtype=np.float64 if LD_WIDE else object).astype(np.float64)
    return R, D


def omega_tiles(L, X, rev=False):
    """rev: L is S(i, c) = L'(n-1-i, c), the square-root factor that comes from factoring the reversed matrix; the tiles of the measure
    then start at the far corner of X, where the algorithm's own tiles start (the same residuals, tiled as the algorithm tiles them;
    for n no multiple of 16 tiles counted from the near corner would straddle the algorithm's)"""
    if rev:
        L, X = L[::-1, :], X[::-1, ::-1]
    return _tile_worst(*factor_fields(L, X))


def omega_elementwise(L, X):
    """information only (module docstring): the largest element-wise ratio"""
    R, D = factor_fields(L, X)
    m = D > 0
    return float(np.max(R[m] / D[m])) / U if m.any() else 0.0


def solve_fields(L, Z, B):
    """(|L Z - B|, |L| |Z| + |B|) as float64 arrays"""
    R = _sub_abs(_mm(L, Z), B)
    D = np.asarray(_mm(np.abs(L), np.abs(Z)), dtype=np.float64 if LD_WIDE else object).astype(np.float64) + np.abs(B)
    return R, D


def omega_solve(L, Z, B):
    return _tile_worst(*solve_fields(L, Z, B))


# ---- reference (a): LAPACK ------------------------------------------------------------------------------------------------------------
def lapack_chol(X, dead=()):
    """np.linalg.cholesky on the kept submatrix; the columns (and rows) of the removed zero-variance states are zero"""
    n = X.shape[0]
    keep = [i for i in range(n) if i not in set(dead)]
    L = np.zeros((n, n))
    L[np.ix_(keep, keep)] = np.linalg.cholesky(X[np.ix_(keep, keep)])
    return L


def forward_solve(L, B):
    """Z = L^-1 B row by row (plain forward substitution)"""
    Z = np.zeros_like(B, dtype=np.float64)
    for i in range(L.shape[0]):
        Z[i] = (B[i] - L[i, :i] @ Z[:i]) / L[i, i]
    return Z


# ---- reference (b): the mirror of the tile algorithm ----------------------------------------------------------------------------------
def _tri_inv(L):
    """inverse of a lower-triangular tile by forward substitution on the columns of the identity, as the device's sweep forms it (an
    LU-based inverse -- np.linalg.inv -- of a graded triangular tile is not accurate entry by entry, and the panel inherits that)"""
    m = L.shape[0]
    Y = np.zeros((m, m))
    for c in range(m):
        Y[c, c] = 1.0 / L[c, c]
        for i in range(c + 1, m):
            Y[i, c] = -(L[i, c:i] @ Y[c:i, c]) / L[i, i]
    return Y


def _tile_factor(A, tol, drop, inv=None):
    """unblocked Cholesky of one diagonal tile with dropped pivots, and the explicit (generalised) inverse of its factor"""
    m = A.shape[0]
    L = np.zeros((m, m))
    dropped, negative = [], []
    for j in range(m):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if drop and d <= tol:
            dropped.append(j)
            if d < -tol:
                negative.append(j)
            continue
        if not drop and not d > 0.0:
            negative.append(j)
            L[j:, j] = np.nan   # (no pivot test on this chain: the device's reciprocal square root gives NaN, and so does the mirror)
            continue
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    kept = [j for j in range(m) if j not in dropped]
    Li = np.zeros((m, m))
    if kept:
        Li[np.ix_(kept, kept)] = (inv or _tri_inv)(L[np.ix_(kept, kept)]) if np.isfinite(L).all() else np.nan
    return L, Li, dropped, negative


def tile_chol(X, tol_rel=0.0, drop=True, inv=None):
    """The tile algorithm in float64: returns dict(L, Linv [nb], dropped, negative) -- `dropped` / `negative` are the positions of the pivots
    <= tol and < -tol (drop: chol(P)'s chain) or of the non-positive pivots (not drop: chol(M)'s chain, which has no pivot test).
    inv: how a diagonal tile's factor is inverted (default: by substitution, _tri_inv)."""
    n = X.shape[0]
    nb = (n + TS - 1) // TS
    tol = tol_rel * float(np.max(np.diag(X))) if tol_rel > 0.0 else 0.0
    A = np.array(X, dtype=np.float64)
    L = np.zeros((n, n))
    Linv, dropped, negative = [], [], []
    for k in range(nb):
        k0, k1 = TS * k, min(n, TS * k + TS)
        L11, Li, dr, ng = _tile_factor(A[k0:k1, k0:k1], tol, drop, inv)
        L[k0:k1, k0:k1] = L11
        Linv.append(Li)
        dropped += [k0 + j for j in dr]
        negative += [k0 + j for j in ng]
        if k1 < n:
            Pn = A[k1:, k0:k1] @ Li.T   # the inverse-based panel
            L[k1:, k0:k1] = Pn
            A[k1:, k1:] -= Pn @ Pn.T
    return dict(L=L, Linv=Linv, dropped=dropped, negative=negative)


def tile_solve(L, Linv, B):
    """Z = L^-1 B, right-looking, multiplying by inv(L11) block step by block step"""
    n = L.shape[0]
    W = np.array(B[:n], dtype=np.float64)
    Z = np.zeros_like(W)
    for k, Li in enumerate(Linv):
        k0, k1 = TS * k, min(n, TS * k + TS)
        Z[k0:k1] = Li @ W[k0:k1]
        if k1 < n:
            W[k1:] -= L[k1:, k0:k1] @ Z[k0:k1]
    return Z


# ---- the device's call forms, restated on the host (what the hooks and the tests do around the kernels) ------------------------------
def from_reversed(Lr):
    """S(i, c) = L'(n-1-i, c): the square-root factor of X from the factor L' of the reversed matrix (capi_handle.inc, prior_factor)"""
    return np.ascontiguousarray(Lr[::-1, :])


def product_layout(B, ld):
    """B as the update finds the prior's factor: (buffer, base offset, row stride, column stride) with B(r, c) = buffer[base + r ld - c];
    the rest of the buffer is NaN"""
    rows, nc1 = B.shape
    buf = np.full(rows * ld, np.nan)
    for r in range(rows):
        buf[r * ld + (nc1 - 1) - np.arange(nc1)] = B[r]
    return buf, nc1 - 1, ld, -1


def solve_call(Lfac, Linv, n, buf, base, srow, scol, nc1, bx, tail, tail_scale, guard=1):
    """The solve's contract restated over strided right-hand sides: Z [(n + tail + guard) x (nc1 + (bx is not None) + guard)], NaN where nothing
    is written; rows < n: L^-1 [B | bx]; tail rows: tail_scale * B, the extra column zero."""
    ncols = nc1 + (bx is not None)
    B = np.array([[buf[base + r * srow + c * scol] for c in range(nc1)] for r in range(n + tail)])
    Z = np.full((n + tail + guard, ncols + guard), np.nan)
    full = B[:n] if bx is None else np.hstack([B[:n], np.asarray(bx, dtype=np.float64).reshape(n, 1)])
    Z[:n, :ncols] = tile_solve(Lfac, Linv, full)
    Z[n:n + tail, :nc1] = tail_scale * B[n:]
    if bx is not None:
        Z[n:n + tail, nc1] = 0.0
    return Z


# ---- the assertions the device tests make, as functions of the result (so that the mirror's output can be fed through them) ---------
def factor_bar(X, tol_rel=0.0, dead=(), rev=False):
    """(bar, lapack's figure, mirror's figure) of a factorisation case.  rev: the references factor the reversed matrix too, and their
    S(i, c) = L'(n-1-i, c) is measured against X exactly as the device's is."""
    n = X.shape[0]
    if rev:
        Xr = reverse(X)
        Sa = from_reversed(lapack_chol(Xr, dead_columns(n, dead, True)))
        Sb = from_reversed(tile_chol(Xr, tol_rel)['L'])
    else:
        Sa, Sb = lapack_chol(X, dead), tile_chol(X, tol_rel)['L']
    a, b = omega_tiles(Sa, X, rev), omega_tiles(Sb, X, rev)
    return BAR_FACTOR * max(a, b), a, b


def solve_refs(X, B, bx=None):
    """(bar, lapack's figure, mirror's figure) of a solve case: each reference's own L with its own Z"""
    full = B if bx is None else np.hstack([B, np.asarray(bx).reshape(-1, 1)])
    La = lapack_chol(X)
    a = omega_solve(La, forward_solve(La, full), full)
    t = tile_chol(X)
    b = omega_solve(t['L'], tile_solve(t['L'], t['Linv'], full), full)
    return BAR_FACTOR * max(a, b), a, b


def dead_columns(n, dead, rev):
    """the zero columns of the factor for zero-variance states `dead`: their own, or mirrored in the reversed form"""
    return [n - 1 - i for i in dead] if rev else list(dead)


def check_factor(S, X, bar, dead=(), rev=False):
    """S S^T = X within the bar tile by tile; the rows of the zero-variance states and the columns of their dropped pivots exactly
    zero.  Returns the figure."""
    assert np.isfinite(S).all()
    w = omega_tiles(S, X, rev)
    assert w <= bar, (w, bar)
    if len(dead):
        assert not S[list(dead), :].any()
        assert not S[:, dead_columns(X.shape[0], dead, rev)].any()
    return w


def check_solve(r, X, B, bx, tail, tail_scale, bar_L, bar_Z):
    """The assertions on one fused-solve result r = dict(L, Z, info, guard_row, guard_col[, outside]); returns (factor's figure, solve's)."""
    n, nc1 = X.shape[0], B.shape[1]
    ncols = nc1 + (bx is not None)
    assert list(r['info']) == [0, 0, 0]
    assert r['Z'].shape == (n + tail, ncols) and np.isfinite(r['Z']).all()
    assert np.abs(np.triu(r['L'], 1)).max() == 0.0
    wl = omega_tiles(r['L'], X)
    assert wl <= bar_L, (wl, bar_L)
    full = B[:n] if bx is None else np.hstack([B[:n], np.asarray(bx, dtype=np.float64).reshape(n, 1)])
    wz = omega_solve(r['L'], r['Z'][:n], full)
    assert wz <= bar_Z, (wz, bar_Z)
    if tail:
        assert np.array_equal(r['Z'][n:, :nc1], tail_scale * B[n:])   # one multiplication: bit for bit
        if bx is not None:
            assert not r['Z'][n:, nc1].any()
    assert np.isnan(r['guard_row']).all() and np.isnan(r['guard_col']).all()
    if r.get('outside') is not None:
        assert r['outside'] == 0
    return wl, wz


# ---- the cases of the non-positive pivot and of the dropped-pivot threshold ----------------------------------------------------------
def negative_pivot_case(pos, n=100, seed=5, cond=1e4):
    """graded(n) with the diagonal entry at `pos` lowered until the pivot at `pos` is -(half the entry): every other pivot stays positive"""
    X = graded(n, seed, cond).copy()
    t = tile_chol(X)
    piv = t['L'][pos, pos] ** 2
    X[pos, pos] = X[pos, pos] - piv - 0.5 * X[pos, pos]
    return X


THRESH_VARS = (1e-13, 1e-16)   # tol = 8 eps * 1 = 1.8e-15 lies between them
# (n, first of the two rows): rows 15 | 16 straddle the first tile boundary -- at n = 32 in the reversed matrix too (rows 16 | 15) --, and
# the last two rows of an n with a partial last tile, which are the first two pivots of the reversed matrix
THRESH_SHAPES = ((32, 15), (50, 48))


def threshold_case(n, at, seed=3, cond=1e4):
    """graded(n - 2) with two uncorrelated states of variance 1e-13 and 1e-16 inserted at the rows `at`, `at + 1` (largest diagonal
    entry exactly 1)"""
    G = graded(n - 2, seed, cond)
    assert float(np.max(np.diag(G))) == 1.0
    idx = [i for i in range(n) if i not in (at, at + 1)]
    X = np.zeros((n, n))
    X[np.ix_(idx, idx)] = G
    X[at, at], X[at + 1, at + 1] = THRESH_VARS
    return X


def check_threshold(S, info, at):
    """the first state kept (its column sqrt(1e-13) to one ulp on the diagonal, nothing else: it is uncorrelated), the second dropped"""
    assert int(info[0]) == 1 and int(info[1]) == 0
    want = np.sqrt(THRESH_VARS[0])
    col = S[:, :]
    # the kept state's column is the one that holds its diagonal entry: find it by its row (S may be the reversed form)
    row = col[at]
    nz = np.flatnonzero(row)
    assert nz.size == 1, nz
    assert abs(row[nz[0]] - want) <= np.spacing(want), (row[nz[0]], want)
    assert np.count_nonzero(col[:, nz[0]]) == 1
    assert not col[at + 1].any()     # the dropped state: its row of the factor ...
    zero_cols = [c for c in range(S.shape[1]) if not col[:, c].any()]
    assert len(zero_cols) == 1       # ... and exactly one zero column


# ---- the cases, with their bars (computed once per run and shared) ---------------------------------------------------------------------
FACTOR_KINDS = ('g1e4', 'g1e6', 'prior')     # on the device; the CPU tests add 'g1e2'


def factor_kinds(n, with_1e2=False):
    kinds = (('g1e2',) if with_1e2 else ()) + FACTOR_KINDS
    return tuple(k for k in kinds if k != 'prior' or n >= 22)


@functools.lru_cache(maxsize=None)
def factor_case(kind, n, rev=False):
    """dict(X, tol_rel, dead, bar, lapack, mirror): with rev the references factor the reversed matrix, as the device does"""
    if kind == 'prior':
        X, tol_rel, dead = prior(n), TOL_PRIOR, DEAD
    else:
        X, tol_rel, dead = graded(n, n, float(kind[1:])), 0.0, ()
    bar, a, b = factor_bar(X, tol_rel, dead, rev)
    return dict(X=X, tol_rel=tol_rel, dead=dead, bar=bar, lapack=a, mirror=b)


@functools.lru_cache(maxsize=None)
def solve_case(n, cond, nc1):
    """dict(X, B [(n + TAIL) x nc1], bx [n], bar_L, bar_Z, lapack, mirror): the solve's figures are those of [B | bx]"""
    X = graded(n, 11 * n, cond)
    B = rhs(n + TAIL, nc1, 1000 * n + nc1)
    bx = rhs(n, 1, 77 * n + nc1)[:, 0]
    for a in (B, bx):
        a.setflags(write=False)
    bar_L = factor_bar(X)[0]
    bar_Z, a, b = solve_refs(X, B[:n], bx)
    return dict(X=X, B=B, bx=bx, bar_L=bar_L, bar_Z=bar_Z, lapack=a, mirror=b)
