"""TEST INFRASTRUCTURE ONLY -- the square-root factor of the covariance AUGMENTED by entering features
(orcvio_msckf_cov_commit_new_features_fac: k_aug_rows, k_aug_finish).  With P+ = S+ S+^T, HH = H_2^-1 H_1, W = R^-1 R^-T (R = H_2),

    P_aug = S_aug S_aug^T,   S_aug = [  S+       0           ]   rows in the state's order [old | new | nuisance],
                                     [ -HH S+    sigma R^-1   ]   columns: those of S+, then one per new state (block-diagonal)

a float64 restatement of S_aug from (H_1, H_2, r_1, S+, sigma, tail, ref_ldlt) and the same in extended precision (np.longdouble),
built on entering_cases' helpers; P_aug itself is entering_cases.tail_ext's.  Under ref_ldlt only HH (and x) divide by diag(H_2);
W, and with it the factor's new block, does not.

Used by tests/test_entering_factor_cases.py (CPU: the restatement against the reference, the mutations) and
tests/test_gpu_entering_factor.py (the kernels against the reference)."""
import numpy as np

import entering_cases as ec

LD = ec.LD

# ---- tolerances ---------------------------------------------------------------------------------------------------------------
# 100 x the worst error the float64 restatement below shows against the extended reference over ALL (case, factor shape) pairs of
# tests/test_entering_factor_cases.py (entering_cases' own rule: ROW_TOL, TAIL_TOL); error = max|got - ref| / max|ref| per block
# (entering_cases.block_err).  Never derived from what the device returns.
#   measured (x86-64, 80-bit long double), worst over 22 cases x 3 factor shapes:
#     G = -HH S+ 1.83e-15 (wide_d3_k1, kf = n)   sigma R^-1 1.47e-16 (small_d3_k20)
#     S_aug S_aug^T against P_aug, worst block 3.53e-16 (wide_d3_k1, kf = n); the extended reference's own product 1.07e-16
G_WORST = 1.9e-15
RINV_WORST = 1.5e-16
SST_WORST = 3.6e-16
G_TOL = 100 * G_WORST
RINV_TOL = 100 * RINV_WORST
SST_TOL = 100 * SST_WORST

FACTOR_SHAPES = ('square', 'narrow', 'wide')   # kf = n, n - 6 (a factor that came through an augmentation), n + 6 (through a marginalisation)


def factor_of(P, shape):
    """A factor S [n, kf] of the given shape from the symmetric square root of P by its eigenvectors (a window's prior is only
    semi-definite: a new clone copies the IMU pose); the covariance it stands for is S S^T, whatever the shape."""
    lam, V = np.linalg.eigh(0.5 * (P + P.T))
    L = V[:, ::-1] * np.sqrt(np.clip(lam[::-1], 0.0, None))
    if shape == 'square':
        return L
    if shape == 'narrow':
        return np.ascontiguousarray(L[:, :-6])
    assert shape == 'wide'
    return np.hstack([L, 0.25 * L[:, 3:9]])


def covariance_of(S):
    """S S^T, formed in extended precision and rounded once (the float64 P+ the tail reference is fed with)."""
    Sl = np.asarray(S, dtype=np.float64).astype(LD)
    P = Sl @ Sl.T
    return (0.5 * (P + P.T)).astype(np.float64)


def _order(n, sz, tail):
    n0 = n - tail
    return np.concatenate([np.arange(n0), n + np.arange(sz), np.arange(n0, n)])   # index in the [old + tail | new] order


def _s_aug(H_1, H_2, S_upd, sigma, tail, ref_ldlt, dtype, inverse):
    k, d, _ = H_2.shape
    n, kf = S_upd.shape
    sz = d * k
    H1, S = np.asarray(H_1, dtype=np.float64).astype(dtype), np.asarray(S_upd, dtype=np.float64).astype(dtype)
    HH = np.zeros((sz, n), dtype=dtype)
    Rinv = np.zeros((k, d, d), dtype=dtype)
    for j in range(k):
        R = np.asarray(H_2[j], dtype=np.float64).astype(dtype)
        q = slice(d * j, d * j + d)
        HH[q] = inverse(R, ref_ldlt) @ H1[q]
        Rinv[j] = inverse(R, False)
    G = -(HH @ S)
    full = np.zeros((n + sz, kf + sz), dtype=dtype)
    full[:n, :kf] = S
    full[n:, :kf] = G
    for j in range(k):
        full[n + d * j:n + d * j + d, kf + d * j:kf + d * j + d] = dtype(sigma) * Rinv[j]
    return dict(S_aug=full[_order(n, sz, tail)], G=G, sRinv=dtype(sigma) * Rinv)


def _upper_inverse_f64(R, diag_only):
    d = R.shape[0]
    Ri = np.zeros((d, d))
    for c in range(d):
        for i in range(d - 1, -1, -1):
            m = 1.0 if i == c else 0.0
            if not diag_only:
                for q in range(i + 1, d):
                    m -= R[i, q] * Ri[q, c]
            Ri[i, c] = m / R[i, i]
    return Ri


def s_aug_f64(H_1, H_2, r_1, S_upd, sigma, tail=0, ref_ldlt=False):
    """The float64 restatement: dict(S_aug [n + sz, kf + sz] rows in the [old | new | tail] order, G = -HH S+ [sz, kf],
    sRinv = sigma R^-1 [k, d, d]).  r_1 does not enter the factor (it is taken so that the signature names every block of the tail)."""
    return _s_aug(H_1, H_2, S_upd, sigma, tail, ref_ldlt, np.float64, _upper_inverse_f64)


def s_aug_ext(H_1, H_2, r_1, S_upd, sigma, tail=0, ref_ldlt=False):
    """The same in extended precision (entering_cases._upper_inverse_ld)."""
    return _s_aug(H_1, H_2, S_upd, sigma, tail, ref_ldlt, LD, lambda R, diag: ec._upper_inverse_ld(R, diag_only=diag))


def factor_blocks(S_aug, n, kf, sz, tail):
    """The blocks of an augmented factor whose rows stand in the [old | new | tail] order: the rows that only moved, G, the block of
    the new rows' own columns, and the zero block over it."""
    n0 = n - tail
    keep = np.concatenate([np.arange(n0), np.arange(n0 + sz, n + sz)])
    new = slice(n0, n0 + sz)
    return dict(old=S_aug[keep, :kf], zero=S_aug[keep, kf:], G=S_aug[new, :kf], own=S_aug[new, kf:])


def own_blocks(own, d):
    """(the k diagonal d x d blocks [k, d, d], what is off them) of the new rows' own columns"""
    sz = own.shape[0]
    k = sz // d
    diag = np.array([own[d * j:d * j + d, d * j:d * j + d] for j in range(k)])
    off = own.copy()
    for j in range(k):
        off[d * j:d * j + d, d * j:d * j + d] = 0
    return diag, off


def sst_err(S_aug, P_aug, n, sz, tail):
    """worst block_err over entering_cases.tail_blocks of S_aug S_aug^T (formed in extended precision) against P_aug"""
    Sl = np.asarray(S_aug).astype(LD)
    gb, rb = ec.tail_blocks(Sl @ Sl.T, n, sz, tail), ec.tail_blocks(P_aug, n, sz, tail)
    return max(ec.block_err(gb[q], rb[q]) for q in gb)


def violations(S_aug, S_old, ref, d, tail=0, P_aug=None):
    """The checks an augmented factor S_aug [n + sz, kf + sz] fails (empty: none), and the measured figures.
    S_old [n, kf]: what its old rows must equal BIT FOR BIT; ref: s_aug_ext's dict; P_aug: the extended augmented covariance of
    S_old S_old^T (None: the product is not checked)."""
    n, kf = S_old.shape
    sz = S_aug.shape[0] - n
    assert S_aug.shape == (n + sz, kf + sz), (S_aug.shape, n, kf, sz)
    b = factor_blocks(S_aug, n, kf, sz, tail)
    diag, off = own_blocks(b['own'], d)
    fig = dict(G=ec.block_err(b['G'], ref['G']), own=ec.block_err(diag, ref['sRinv']))
    bad = []
    if not np.array_equal(b['old'], S_old):
        bad.append('old rows')
    if b['zero'].any():
        bad.append('zero block')
    if off.any():
        bad.append('off the diagonal blocks')
    if not fig['G'] <= G_TOL:
        bad.append('G')
    if not fig['own'] <= RINV_TOL:
        bad.append('sigma R^-1')
    if P_aug is not None:
        fig['sst'] = sst_err(S_aug, P_aug, n, sz, tail)
        if not fig['sst'] <= SST_TOL:
            bad.append('S S^T')
    return bad, fig
