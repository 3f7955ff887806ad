"""TEST INFRASTRUCTURE -- the reference's zero-velocity test on IMU samples (OrcVIO::checkZUPTIMU, src/orcvio.cpp:3129-3323) restated in
numpy, at leg_dim 22 (Tg = Ma = I, As = 0).

  dense(...)      the reference literally: H (6 m x 9), the diagonal R and S = H P_m H^T + R of order 6 m, chi^2 = r . S^-1 r through
                  numpy.linalg.cholesky (Eigen's llt: the lower triangle of S)
  woodbury(...)   the device's form (orcvio_amd/csrc/host/zupt_check_model.hpp): 56 sums over the rows and two 9 x 9 factorisations
  chi2_mp(...)    the same number in 60-digit arithmetic (mpmath), the yardstick both are measured against
  decide(...)     the accept bit as :3291 takes it

A case is a dict: P [n][n], R [3][3], ba, g, v [3], samples [S][7] (t | gyro | acc), left (bool), consts (dict: sigma_w2, sigma_a2,
sigma_wb, sigma_ab, chi2_prob, chi2_multiplier, max_velocity).  `mutate` names a deliberate mistake (tests/test_zupt_check_mirror.py)."""
from __future__ import annotations

import numpy as np

IDX = np.array([0, 1, 2, 9, 10, 11, 12, 13, 14])
CONSTS = dict(sigma_w2=1.6968e-04 ** 2, sigma_a2=2.0000e-3 ** 2, sigma_wb=1.9393e-05, sigma_ab=3.0000e-03, chi2_prob=0.95,
              chi2_multiplier=1.0, max_velocity=0.25)
MUTATIONS = ('no_gyro_rows', 'bias_walk_squared', 'dt_from_process_model', 'left_right_swapped', 'velocity_rows')


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def marginal(P, mutate=None):
    """P_m as :3235-3254 copy it, both triangles as they stand"""
    idx = IDX.copy()
    if mutate == 'velocity_rows':
        idx[3:6] = [3, 4, 5]
    return P[np.ix_(idx, idx)].copy()


def intervals(case, mutate=None):
    t = case['samples'][:, 0]
    if mutate == 'dt_from_process_model':   # processModel's interval: from the state's time (before the first sample) to the sample
        return np.diff(np.concatenate([[case['t_state']], t]))[:-1]
    return np.diff(t)


def rows(case, mutate=None):
    """H [6 m][9], r [6 m], the diagonal of R [6 m], dt_sum: the loop of :3171-3223"""
    smp, R, ba, g, c = case['samples'], case['R'], case['ba'], case['g'], case['consts']
    left = bool(case['left']) != (mutate == 'left_right_swapped')
    dts = intervals(case, mutate)
    m = smp.shape[0] - 1
    H = np.zeros((6 * m, 9))
    r = np.zeros(6 * m)
    Rd = np.ones(6 * m)
    for i in range(m):
        acc = smp[i, 4:7] - ba
        r[6 * i + 3: 6 * i + 6] = -R @ acc - g   # (the gyro rows' residual is multiplied by zero, :3194)
        if mutate != 'no_gyro_rows':
            H[6 * i: 6 * i + 3, 3:6] = np.eye(3)
        H[6 * i + 3: 6 * i + 6, 0:3] = skew(R @ acc) if left else R @ skew(acc)
        H[6 * i + 3: 6 * i + 6, 6:9] = R
        Rd[6 * i: 6 * i + 3] = c['sigma_w2'] / dts[i]
        Rd[6 * i + 3: 6 * i + 6] = c['sigma_a2'] / dts[i]
    return H, r, Rd, float(np.sum(dts))


def bias_walk(case, dt_sum, mutate=None):
    c = case['consts']
    wb, ab = c['sigma_wb'], c['sigma_ab']
    if mutate == 'bias_walk_squared':
        wb, ab = wb * wb, ab * ab
    q = np.zeros(9)
    q[3:6] = dt_sum * wb
    q[6:9] = dt_sum * ab
    return q


def dense(case, mutate=None):
    """(chi2, dof)"""
    H, r, Rd, dt_sum = rows(case, mutate)
    Pm = marginal(case['P'], mutate) + np.diag(bias_walk(case, dt_sum, mutate))
    S = H @ Pm @ H.T + np.diag(Rd)
    L = np.linalg.cholesky(S)
    y = np.linalg.solve(L, r)
    return float(y @ y), int(r.size)


def sums(case, mutate=None):
    """A [9][9], b [9], c, dt_sum"""
    H, r, Rd, dt_sum = rows(case, mutate)
    W = 1.0 / Rd
    return H.T @ (W[:, None] * H), H.T @ (W * r), float(r @ (W * r)), dt_sum


def woodbury(case, mutate=None):
    """(chi2, c, dt_sum): chi2 = c - |C^-1 L^T b|^2 with P_m = L L^T, I + L^T A L = C C^T"""
    A, b, c, dt_sum = sums(case, mutate)
    Pm = marginal(case['P'], mutate)
    Pm = 0.5 * (Pm + Pm.T) + np.diag(bias_walk(case, dt_sum, mutate))
    L = np.linalg.cholesky(Pm)
    C = np.linalg.cholesky(np.eye(9) + L.T @ A @ L)
    z = np.linalg.solve(C, L.T @ b)
    return float(c - z @ z), c, dt_sum


def chi2_mp(case, form='woodbury', digits=60):
    """chi2 in `digits`-digit arithmetic (mpmath) from the same doubles, returned as the nearest double.  form 'dense' factors S of
    order 6 m itself (pure Python: affordable up to a few dozen rows); form 'woodbury' evaluates the 9 x 9 identity, which in 60 digits
    is the same number to 50 (its subtraction loses log10(c / chi2) <= 5 of them) -- tests/test_zupt_check_mirror.py asserts the two
    agree wherever 'dense' is affordable, and uses 'woodbury' as the yardstick at every sample count."""
    import mpmath as mp
    with mp.workdps(digits):
        f = lambda x: mp.mpf(float(x))
        smp, R, ba, g, c = case['samples'], case['R'], case['ba'], case['g'], case['consts']
        m = smp.shape[0] - 1
        Rm = mp.matrix([[f(x) for x in row] for row in R])
        sk = lambda w: mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        Hm = mp.zeros(6 * m, 9)
        rm = mp.zeros(6 * m, 1)
        Rd = [mp.mpf(0)] * (6 * m)
        dts = mp.mpf(0)
        for i in range(m):
            dt = f(smp[i + 1, 0] - smp[i, 0])   # (the stamps are subtracted in double precision by the reference and by every form under test)
            acc = mp.matrix([f(smp[i, 4 + k]) - f(ba[k]) for k in range(3)])
            Ra = Rm * acc
            J = sk(Ra) if case['left'] else Rm * sk(acc)
            for a in range(3):
                rm[6 * i + 3 + a] = -Ra[a] - f(g[a])
                Hm[6 * i + a, 3 + a] = 1
                Rd[6 * i + a] = f(c['sigma_w2']) / dt
                Rd[6 * i + 3 + a] = f(c['sigma_a2']) / dt
                for k in range(3):
                    Hm[6 * i + 3 + a, k] = J[a, k]
                    Hm[6 * i + 3 + a, 6 + k] = Rm[a, k]
            dts += dt
        Pm = mp.matrix([[f(x) for x in row] for row in marginal(case['P'])])
        for k in range(3):
            Pm[3 + k, 3 + k] += dts * f(c['sigma_wb'])
            Pm[6 + k, 6 + k] += dts * f(c['sigma_ab'])
        if form == 'dense':
            S = Hm * Pm * Hm.T
            for k in range(6 * m):
                S[k, k] += Rd[k]
            return float((rm.T * mp.cholesky_solve(S, rm))[0])
        WH = mp.matrix(6 * m, 9)
        for k in range(6 * m):
            for q in range(9):
                WH[k, q] = Hm[k, q] / Rd[k]
        A = Hm.T * WH
        b = WH.T * rm
        cc = sum(rm[k] * rm[k] / Rd[k] for k in range(6 * m))
        # chi2 = c - b^T (P_m^-1 + A)^-1 b = c - b^T P_m (I + A P_m)^-1 b
        x = mp.lu_solve(mp.eye(9) + A * Pm, b)
        return float(cc - (b.T * Pm * x)[0])


def threshold(case, dof):
    from scipy.stats import chi2
    return float(chi2.ppf(case['consts']['chi2_prob'], dof))


def decide(case, chi2_value, dof, thr=None):
    """do_zupt (:3291-3300)"""
    c = case['consts']
    thr = threshold(case, dof) if thr is None else thr
    speed = float(np.linalg.norm(case['v']))
    return not (chi2_value > c['chi2_multiplier'] * thr or speed > c['max_velocity'])
