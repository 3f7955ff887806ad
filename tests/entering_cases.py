"""TEST INFRASTRUCTURE ONLY -- features ENTERING the state (featureJacobian_ekf_new, the W = [V | U] split and the H_1 / H_2 tail of
measurementUpdate_hybrid, reference src/orcvio.cpp:1481-1572, :2416-2436, :1811-1947) at the shapes where k_ekf_new, k_aug_hh,
k_aug_dx and k_aug_assemble take another branch: a generator of windows and entering features from explicit
(anchor, observing clones) specs, and a reference in extended precision (np.longdouble, 64-bit mantissa) that is compared BLOCK BY
BLOCK and does not depend on the orthonormal bases or the sign convention of anybody's QR.

Row invariants of one feature with stacked rows [H_x | H_f | r] (mirror_hybrid.feature_jacobian_ekf_new), and what a split
H_1, H_2, r_1, V-part rows [V_x | r_V] of the same rows must give:
    HH = (H_f^T H_f)^-1 H_f^T H_x        = H_2^-1 H_1
    x  = (H_f^T H_f)^-1 H_f^T r          = H_2^-1 r_1
    W  = (H_f^T H_f)^-1                  = (H_2^T H_2)^-1
    A  = H_x^T (I - H_f W H_f^T) H_x     = V_x^T V_x
    b  = H_x^T (I - H_f W H_f^T) r       = V_x^T r_V
Tail from H_1, H_2, r_1, dx, P+, s2: dx_new = x - HH dx, P21 = -HH P+, P22 = HH P+ HH^T + s2 W, placed [old | new | tail].

Used by tests/test_entering_cases.py (CPU: generator, conditioning, the float64 restatement against this reference) and
tests/test_gpu_entering_features.py (the kernels against it)."""
import dataclasses
import functools

import numpy as np

from orcvio_amd import synth
from oracle import mirror_hybrid as mh

LD = np.longdouble

# ---- tolerances of the block comparisons --------------------------------------------------------------------------------------
# 100 x the worst error the float64 restatement (numpy QR per feature + mirror_hybrid.augment_after_update) shows against the
# extended reference over ALL cases below (tests/test_entering_cases.py measures it; error = max|got - ref| / max|ref| per block,
# dx_new scaled by max(|x| + |HH| |dx|)).  The factor 100 covers the device's summation order, FMA contraction and 64-row
# reflections; a missing term, a wrong column or a wrong sign shows at 1e-3 of the block's scale or more.  Never derived from what
# the device returns.
#   measured, worst over the 22 cases (x86-64, 80-bit long double):
#     rows  HH 8.7e-16   x 1.6e-15   W 1.2e-15   A 8.6e-16   b 2.1e-15   (b: small_d3_k20)
#     tail  dx_new 7.4e-17   P21 1.4e-15 (wide_d3_k1)   P22 1.4e-15 (schmidt_d3_k6)
ROW_WORST = 2.1e-15
TAIL_WORST = 1.4e-15
ROW_TOL = 100 * ROW_WORST
TAIL_TOL = 100 * TAIL_WORST
COND_CAP = 50.0      # cond(H_f) of every generated feature (a prototype of the specs gave at most 14)

JAC = {'larvio': dict(use_larvio=1), 'orcvio_right': dict(use_larvio=0, use_left_perturbation=0),
       'orcvio_left': dict(use_larvio=0, use_left_perturbation=1),
       'kitti_raw': dict(use_larvio=0, use_left_perturbation=0, noise_feature=1.0, discard_large_update=1)}
SHAPES = {'small': dict(leg=22, N=12, extra=None, nui=0, F=30),      # extra None: 4 in-state features of width d
          'wide': dict(leg=46, N=36, extra=18, nui=0, F=40),         # n = 280: n + 1 > 256 and n > 224 (LDS-panel factorisation)
          'schmidt': dict(leg=22, N=12, extra=None, nui=2, F=30)}


@dataclasses.dataclass(frozen=True)
class CaseId:
    shape: str
    d: int
    k: int
    fej: int = 0
    jac: str = 'larvio'
    ldlt: bool = False

    def __str__(self):
        return '%s_d%d_k%d%s%s%s' % (self.shape, self.d, self.k, '_fej' if self.fej else '', '' if self.jac == 'larvio' else '_' + self.jac,
                                     '_ldlt' if self.ldlt else '')


CASES = ([CaseId(s, d, k) for s in SHAPES for d in (1, 3) for k in (1, 6)] + [CaseId('small', 3, 20)] +
         [CaseId('small', d, 6, fej=1) for d in (1, 3)] +
         [CaseId('small', d, 6, jac=j) for j in ('orcvio_right', 'orcvio_left', 'kitti_raw') for d in (1, 3)] +
         [CaseId('small', 3, 6, ldlt=True)])


def specs_for(shape, N, k):
    """[(anchor, [observing clones])] of the k entering features."""
    s = {1: (0, [0, 1]),                                # the minimum: d = 1 keeps ONE observation (2 rows), d = 3 two (4 rows)
         2: (N - 1, [N - 2, N - 1]),                    # the same at the other end; the anchor's observation is the LAST one
         3: (N // 2, [2, N // 2, N - 1]),               # the anchor's observation in the middle
         4: (3, list(range(min(N, 32)))),               # the longest track: 64 rows at N >= 32 (d = 3), 62 (d = 1)
         5: (5, [0, 2, 7, 9, 11]),                      # scattered clones, the anchor does not observe the feature
         6: (1, [4, 6, 8]),                             # the anchor does not observe the feature
         '7a': (N, [0, 1, 2]), '7b': (N + 1, [1, N // 2, N - 1])}   # anchored at nuisance states
    if shape == 'schmidt':
        order = ['7a'] if k == 1 else ['7a', '7b', 3, 4, 5, 6]
    else:
        order = [4] if k == 1 else [1, 2, 3, 4, 5, 6]
    return [s[order[i % len(order)]] for i in range(k)]


def make_entering_features(win, specs, seed=0, fej=False, sigma=None):
    """As synth.make_new_slam_features, from explicit specs: the position is drawn in the anchor's camera frame, the estimate is that
    position perturbed there, p_w and the inverse-depth parameters are consistent; observations carry HALF the filter's noise so that
    every feature passes its gate.  fej: p_fej differs from p_w."""
    rng = np.random.default_rng(60_000 + seed)
    sig = 0.5 * (win.flags.noise_feature if sigma is None else sigma)
    out = []
    for i, (a, clones) in enumerate(specs):
        if a < win.N:
            Ra, ta, Rbc, tcb = win.R_b2w[a], win.t_b_w[a], win.R_b2c[a], win.t_c_b[a]
        else:
            j = a - win.N
            Ra, ta, Rbc, tcb = win.nui['R_b2w'][j], win.nui['t_b_w'][j], win.nui['R_b2c'][j], win.nui['t_c_b'][j]
        R_c2w = Ra @ Rbc.T
        t_c_w = ta + Ra @ tcb
        pc = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(4.0, 12.0)])
        pw = R_c2w @ pc + t_c_w
        obs = []
        for k in clones:
            Rk = win.R_b2c[k] @ win.R_b2w[k].T
            tk = win.t_b_w[k] + win.R_b2w[k] @ win.t_c_b[k]
            pk = Rk @ (pw - tk)
            assert pk[2] > 0.5, (a, k, pk)
            obs.append((int(k), pk[:2] / pk[2] + sig * rng.standard_normal(2), 0.05 * rng.standard_normal(2)))
        pce = pc + 0.01 * rng.standard_normal(3)
        inve = np.array([pce[0] / pce[2], pce[1] / pce[2], 1.0 / pce[2]])
        p_w = R_c2w @ pce + t_c_w
        out.append(mh.NewSlamFeature(anchor=int(a), inv_param=inve, obs_anchor=np.array([inve[0], inve[1], 1.0]), inv_depth=float(inve[2]),
                                     p_w=p_w, obs=obs, p_fej=(p_w + 0.01 * np.array([1.0, -0.5, 0.3]) * (i % 6 + 1)) if fej else None))
    return out


@dataclasses.dataclass
class Case:
    cid: CaseId
    win: object        # synth.Window with the in-state features' and the nuisance states' columns
    slam: list         # in-state SLAM features (synth.SlamFeature)
    new: list          # entering features (mirror_hybrid.NewSlamFeature)

    @property
    def tail(self):
        return 6 * self.win.n_nui


@functools.lru_cache(maxsize=None)
def make_case(cid: CaseId) -> Case:
    sh = SHAPES[cid.shape]
    d = cid.d
    sigma_px = 0.008 if cid.jac == 'kitti_raw' else None
    fl = synth.Flags(**dict(dict(estimate_td=1, leg_dim=sh['leg'], if_fej=cid.fej), **JAC[cid.jac]))
    w0 = synth.make_window(N=sh['N'], F=sh['F'], seed=71, track_len=(3, 9), flags=fl, sigma_px=sigma_px)
    nf = 4 if sh['extra'] is None else sh['extra'] // d
    w = synth.with_extra_states(w0, d * nf, seed=4)
    if sh['nui']:
        w = synth.with_nuisance_states(w, sh['nui'], seed=8)
    slam = synth.make_slam_features(w, nf, seed=5 + d, outlier_frac=0.25, nui_frac=0.5 if sh['nui'] else 0.0, sigma_px=sigma_px)
    new = make_entering_features(w, specs_for(cid.shape, w.N, cid.k), seed=10 * d + cid.k, fej=bool(cid.fej), sigma=sigma_px)
    return Case(cid, w, slam, new)


# ---- extended precision ---------------------------------------------------------------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _spd_inverse_ld(G):
    """(d x d SPD)^-1 in extended precision: the float64 inverse, Newton-refined X <- X (2 I - G X)."""
    X = np.linalg.inv(G.astype(np.float64)).astype(LD)
    two = 2 * np.eye(G.shape[0], dtype=LD)
    for _ in range(4):
        X = X @ (two - G @ X)
    return 0.5 * (X + X.T)


def _upper_inverse_ld(R, diag_only=False):
    """(upper triangular d x d)^-1 by back-substitution; diag_only: of diag(R) (the reference's literal H_2.ldlt(), :1826-1827)."""
    d = R.shape[0]
    Ri = np.zeros((d, d), dtype=LD)
    for c in range(d):
        for i in range(d - 1, -1, -1):
            m = LD(1.0 if i == c else 0.0)
            if not diag_only:
                for q in range(i + 1, d):
                    m -= R[i, q] * Ri[q, c]
            Ri[i, c] = m / R[i, i]
    return Ri


def feature_rows(win, ft, d):
    """(H_x [m, n], H_f [m, d], r [m]) of one entering feature: mirror_hybrid.feature_jacobian_ekf_new (float64: the DATA of the reference)."""
    H, r = mh.feature_jacobian_ekf_new(win, ft, 0, 1, d)
    return H[:, :win.n], H[:, win.n:], r


def row_invariants_ext(H_x, H_f, r):
    """dict(HH [d, n], x [d], W [d, d], A [n, n], b [n]) in extended precision from the stacked rows."""
    Hx, Hf, rr = _ld(H_x), _ld(H_f), _ld(r)
    W = _spd_inverse_ld(Hf.T @ Hf)
    HH = W @ (Hf.T @ Hx)
    x = W @ (Hf.T @ rr)
    Rx = Hx - Hf @ HH            # (I - H_f W H_f^T) H_x
    rv = rr - Hf @ x
    return dict(HH=HH, x=x, W=W, A=Hx.T @ Rx, b=Hx.T @ rv)


def split_invariants_ext(H_1, H_2, r_1, V_x, r_V):
    """The same five from a split (H_1 [d, n], H_2 [d, d] upper triangular, r_1 [d], V-part rows V_x [*, n], r_V): the arithmetic in
    extended precision, so that what is measured is the split."""
    H1, R, r1, Vx, rV = _ld(H_1), _ld(H_2), _ld(r_1), _ld(V_x), _ld(r_V)
    Ri = _upper_inverse_ld(R)
    return dict(HH=Ri @ H1, x=Ri @ r1, W=Ri @ Ri.T, A=Vx.T @ Vx, b=Vx.T @ rV)


def block_err(got, ref):
    """max|got - ref| / max|ref|"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def qr_split(H_x, H_f, r):
    """The float64 restatement of the split of one feature (:2416-2436): numpy's Householder QR of H_f, U = the first d columns of Q,
    V the rest.  Returns (H_1, H_2, r_1, V_x, r_V)."""
    d = H_f.shape[1]
    Q, R = np.linalg.qr(H_f, mode='complete')
    U, V = Q[:, :d], Q[:, d:]
    return U.T @ H_x, np.triu(R[:d]), U.T @ r, V.T @ H_x, V.T @ r


def restatement_split(case):
    """(H_1 [d k, n], H_2 [k, d, d], r_1 [d k], H_top [rows, n], r_top, per feature (first row, rows) of H_top) of all entering features."""
    d = case.cid.d
    H1, H2, r1, Vx, rV, span = [], [], [], [], [], []
    at = 0
    for ft in case.new:
        a, b, c, vx, rv = qr_split(*feature_rows(case.win, ft, d))
        H1.append(a); H2.append(b); r1.append(c); Vx.append(vx); rV.append(rv)
        span.append((at, vx.shape[0])); at += vx.shape[0]
    return np.vstack(H1), np.array(H2), np.concatenate(r1), np.vstack(Vx), np.concatenate(rV), span


def block_diag(H_2):
    k, d, _ = H_2.shape
    out = np.zeros((d * k, d * k))
    for j in range(k):
        out[d * j:d * j + d, d * j:d * j + d] = H_2[j]
    return out


def tail_ext(H_1, H_2, r_1, dx, P_upd, s2, tail=0, ref_ldlt=False):
    """The tail in extended precision.  H_2 [k, d, d].  Returns dict(dx_new [sz], dx_scale, P_aug [(n + sz)^2] in the order
    [old (n - tail) | new (sz) | tail], symmetrised as :1946 does).  ref_ldlt: HH and x divide by diag(H_2); W does not (:1907-1908)."""
    H1, r1, dxl, P = _ld(H_1), _ld(r_1), _ld(dx), _ld(P_upd)
    k, d, _ = H_2.shape
    n, sz, n0 = P.shape[0], d * k, P.shape[0] - tail
    HH = np.zeros((sz, n), dtype=LD); x = np.zeros(sz, dtype=LD); W = np.zeros((sz, sz), dtype=LD)
    for j in range(k):
        R = _ld(H_2[j])
        Ri = _upper_inverse_ld(R, diag_only=ref_ldlt)
        Rf = _upper_inverse_ld(R)
        q = slice(d * j, d * j + d)
        HH[q] = Ri @ H1[q]; x[q] = Ri @ r1[q]; W[q, q] = Rf @ Rf.T
    dx_new = x - HH @ dxl
    scale = float((np.abs(x) + np.abs(HH) @ np.abs(dxl)).max())
    P21 = -(HH @ P)
    P22 = -(P21 @ HH.T) + LD(s2) * W
    src = np.concatenate([np.arange(n0), n + np.arange(sz), np.arange(n0, n)])   # index in the [old + tail | new] order
    full = np.zeros((n + sz, n + sz), dtype=LD)
    full[:n, :n] = P; full[n:, :n] = P21; full[:n, n:] = P21.T; full[n:, n:] = P22
    aug = full[np.ix_(src, src)]
    return dict(dx_new=dx_new, dx_scale=scale, P_aug=0.5 * (aug + aug.T))


def tail_blocks(P_aug, n, sz, tail):
    """The blocks of an augmented covariance in the [old | new | tail] order: P21 in front of and behind the nuisance block (the
    piece behind is empty without nuisance states), P22, the old block, the moved nuisance block and its cross terms with the old one."""
    n0 = n - tail
    new = slice(n0, n0 + sz)
    out = dict(P21_front=P_aug[new, :n0], P22=P_aug[new, new], old=P_aug[:n0, :n0])
    if tail:
        out.update(P21_behind=P_aug[new, n0 + sz:], nui=P_aug[n0 + sz:, n0 + sz:], old_nui=P_aug[:n0, n0 + sz:])
    return out
