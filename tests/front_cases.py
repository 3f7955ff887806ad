"""Inputs, references and bars of the tests of the feature front end (CPU: tests/test_front_cases.py, device:
tests/test_gpu_front_blocks.py): feature_body (k_feature, k_front), the two Grams (k_gram_pair, the Gram items of k_front) and the
assembly of A (k_assemble_A, assemble_entry inside k_front, the deferred assembly).

What is compared.  T3, Hs, K and H_thin depend on the basis (the signs of the Householder vectors).  For a track with un-projected
rows X = [H_x(:, 15:) | r] (2M x (NA + 1)) and H_f (2M x 3) these do not:
    G_j     = X^T Pi X,  Pi = I - H_f (H_f^T H_f)^-1 H_f^T       = X^T X - T3^T T3  (what the device forms)  = Hs^T Hs
    gamma_j = (Pi r)^T (Pi H_x P H_x^T Pi + s2 I)^-1 (Pi r)
(the second: with N0 an orthonormal basis of the left null space of H_f, Pi = N0 N0^T, and N0 (N0^T E N0 + s2 I)^-1 N0^T =
Pi (Pi E Pi + s2 I)^-1 Pi, because Pi E Pi + s2 I = N0 (N0^T E N0 + s2 I) N0^T + s2 Q1 Q1^T is block diagonal in [N0 Q1]).
track_reference evaluates both in 60-digit mpmath from the rows of oracle/mp_reference.feature_jacobian_msckf_mp; only the columns the
track touches are carried (7 + 6 per observed clone + r): every other entry of G_j is exactly zero, and the device's must be.  Pi E Pi is
formed from its rank-3 expansion E - B C (B^T E) - (E B) C B^T + B C (B^T E B) C B^T (B = H_f, C = (B^T B)^-1), all in mp.
E = H_x P H_x^T is formed in mp for tracks of up to E_MP_MAX_M observations and in np.longdouble from the mp rows beyond (the rest in mp
either way); tests/test_front_cases.py holds the two evaluations to 1/100 of the bar on the short tracks.

Unit.  u = 2^-53.  Gram elements are measured in u B_j[i, k], B_j[i, k] = sqrt(G0_j[i, i] G0_j[k, k]), G0_j = X^T X the un-projected
Gram: the scale at which the subtraction X^T X - T3^T T3 rounds (diag(T3^T T3) <= diag(X^T X): T3 = Q1^T X).  Where B_j[i, k] = 0 the
column is zero in every row and the element must be exactly zero.  gamma is measured relative, in u.

Bars.  K_G and K_GAMMA are ten times the worst figure, over ALL cases of this file, of the two float64 restatements -- oracle.mirror
(projection by SVD) and the C oracle's projected rows (H_all / r_all) -- against the mp reference in those units, the larger of the two
(REF_FIGURES; tests/test_front_cases.py asserts that no case exceeds them).  Nothing the device returns enters them.
    per track     |(X^T X - T3^T T3)[i, k] - G_j[i, k]| <= K_G u B_j[i, k],   the same for Hs^T Hs;   |gamma - gamma_j| <= K_GAMMA u gamma_j
    A             |A[i, k] - sum_acc G_j[i, k]| <= (K_G + c) u sum_acc B_j[i, k]
c is derived, not measured.  Every element of A is s - (g0 + g1 + g2 + g3) with s one element of a clone's tile S (or the sum of all N
tiles' for the (ext|r) x (ext|r) entries) and g the partial Grams of T3.  Each is a sum of products of stored numbers evaluated as a
tree; the rounding error of such a sum is at most gamma_d sum |terms| with d the longest chain of additions any term passes through
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1 and 4.2: every term collects at most d factors (1 + delta)),
and sum over a track's rows of |x_i| |x_k| <= B_j[i, k] by Cauchy-Schwarz, for X and for T3 alike.  The chains, read from gramw_body and
assemble_entry (msckf_kernels.hpp):
    one Gram tile over R rows by W wavefronts   each wavefront takes rw = round_up(ceil(R / W), 4) rows in k-steps of four (one MFMA
                                                16x16x4: four products onto the accumulator, counted as four additions), alternating
                                                between two accumulators: 4 ceil(rw / 8), then acc0 + acc1 (1), then the pairwise sum of
                                                the W partial tiles (log2 W)                                    = gram_chain(R, W)
    S over the clones ((ext|r)^2 only)          eight interleaved sums of ceil(N / 8) tiles, then three pairwise   ceil(N / 8) + 3
    the partial Grams                           four interleaved sums of ceil(chunks / 4), then two pairwise        ceil(chunks / 4) + 2
    s - g                                       1, and 1 more for a product that is not fused
W = 16 in k_gram_pair (forked route), 8 in k_front.  summation_c(case, route) adds them for the case's own row counts.
The checks of S against the rows of Xobs and of sum Gpart against T3 use gram_chain alone, on |X|^T |X| and |T3|^T |T3| of the device's
own rows.

Cases (CASES; default flags unless said; every window with the extrinsics and, where td is on, the time offset in the prior; the
extrinsic rotation is the polar factor of the calibration file's, see _poses):
    a   column passes and the right-hand-side column: six tracks of 2..6 observations (one on the last two clones, one rejected) at
        N = 4, 9, 10, 20 (NA + 1 == NAP), 21, 31 (NA = 193: assembly inside k_front), 41 (off the register path), 42, 60, and leg 46 at
        N = 29 (n = 220) and 60 (NAP = 400, seven passes)
    b   gate blocks of eight observations: N = 32, accepted tracks of 2, 3, 8, 9, 16, 17, 24, 25, 32 and rejected ones of 8, 9, 32
    c   clone lists, N = 8: clones (0, 3, 7), a descending list, clone 0 and clone N - 1 alone with a neighbour, clone 5 seen by nobody,
        a track of one observation and one of none
    d   the six flag sets of test_flag_variants_ragged at N = 9 and 10 (td column, FEJ positions), two of eight tracks rejected
    e   tracks of 2, 8, 9 observations with the mp gamma at thr (1 - 1e-8) and, a copy, at thr (1 + 1e-8)
    f   row chunks and the sum over clones: eight distinct tracks (six accepted) repeated to F = 341, 342 (1023 / 1026 rows of T3: one
        and two chunks of k_gram_pair), 213, 214 (639 / 642: of k_front), 1366 (five partial Grams) at N = 4, and F = 17 at N = 20
        (every clone seen: the sixteen-wide clamp of the sum over clones)
    g   LEFTOVER_PAIR: the largest window of f, then the smallest of a, on one handle
Outside the gate-edge tracks of group e every track's mp gamma is further than 1e-6 thr from thr (asserted on the CPU), so the accept
mask admits no excuse.

The float64 stand-in.  model_front restates the front end in numpy (rows of oracle.mirror, Householder QR, the clone-sorted Xobs, S,
Gpart by row chunks, the assembly with assemble_entry's column map): tests/test_front_cases.py runs the checkers below on it unchanged
(they must pass) and after each of five mutations (they must fail), so the bars are not loose by decades."""
from __future__ import annotations

import dataclasses
import functools
import math

import mpmath as mp
import numpy as np

from orcvio_amd import synth
from oracle import mirror
from oracle import mp_reference as mpr

LD = np.longdouble
U = 2.0 ** -53
DIGITS = 60
E_MP_MAX_M = 9          # tracks up to this length: E = H_x P H_x^T in mp; beyond: in np.longdouble from the mp rows

# ---- bars: ten times the worst restatement figure over all cases, the larger of the two restatements (tests/test_front_cases.py
#      measures every case again and prints the table; docs/LAB_NOTES.md has it beside the device's) --------------------------------
REF_FIGURES = dict(mirror_G=130.0, mirror_gamma=1023.0, oracle_G=232.0, oracle_gamma=3160.0)   # worst over CASES, in u B_j and in u
K_G = 10.0 * max(REF_FIGURES['mirror_G'], REF_FIGURES['oracle_G'])
K_GAMMA = 10.0 * max(REF_FIGURES['mirror_gamma'], REF_FIGURES['oracle_gamma'])

FLAG_SETS = [(1, 0, 0, 0), (1, 0, 1, 1), (0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 1, 1), (0, 0, 1, 0)]   # test_flag_variants_ragged


# ---- windows --------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    cid: str
    win: synth.Window
    routes: tuple            # the routes the shape admits: 'forked', then 'deferred' or 'inlaunch' (k_front) where it runs
    rep: np.ndarray          # [F] the first track with the same inputs (windows built from repeated tracks: one reference each)
    want: np.ndarray         # [F] 1 accepted, 0 rejected, -1 fewer than two observations
    edge: dict               # track -> +1 (mp gamma at thr (1 + 1e-8): rejected), -1 (thr (1 - 1e-8): accepted)

    @property
    def NA(self):
        return self.win.flags.leg_dim - 15 + 6 * self.win.N

    @property
    def NAP(self):
        return (self.NA + 1 + 15) // 16 * 16

    @property
    def cb0(self):
        return self.win.flags.leg_dim - 15


def _poses(N):
    R_b2c0, t_c_b0 = synth.euroc_extrinsics()
    # The calibration file's rotation is orthonormal to 5e-13 only.  The reference's chain inverts the 4 x 4 pose numerically (so do
    # oracle.mirror and mp_reference), the C oracle and the device use [R^T, -R^T t]: on that input the two forms differ by 1e4 u B_j
    # with use_larvio = 0, which says nothing about either's arithmetic.  The polar factor is orthonormal to rounding.
    Us, _, Vt = np.linalg.svd(R_b2c0)
    R_b2c0 = Us @ Vt
    R_b2w = np.empty((N, 3, 3))
    t_b_w = np.empty((N, 3))
    for i in range(N):
        R_b2w[i] = synth.so3_exp(np.array([0.02 * i, 0.01 * np.sin(i), 0.015 * i]))
        t_b_w[i] = [0.15 * i, 0.05 * np.sin(0.3 * i), 0.03 * i]
    R_b2c = np.broadcast_to(R_b2c0, (N, 3, 3)).copy()
    t_c_b = np.broadcast_to(t_c_b0, (N, 3)).copy()
    return R_b2w, t_b_w, R_b2c, t_c_b


def _track_obs(poses, clones, seed, j, attempt, sig, outlier):
    """(p_w, z [M, 2], zvel [M, 2]) of one track seen by `clones` (any order): a point 4..12 m in front of the middle clone's camera,
    observed with noise sig; outlier: one observation displaced by 40 (1 + attempt) sig (the gate rejects the track)."""
    R_b2w, t_b_w, R_b2c, t_c_b = poses
    rng = np.random.default_rng([seed, j, attempt])
    M = len(clones)
    mid = sorted(clones)[M // 2] if M else 0
    R_c2w = lambda i: R_b2w[i] @ R_b2c[i].T
    t_c_w = lambda i: t_b_w[i] + R_b2w[i] @ t_c_b[i]
    depth = rng.uniform(4.0, 12.0)
    xy = rng.uniform(-0.35, 0.35, 2)
    p_true = R_c2w(mid) @ np.array([xy[0] * depth, xy[1] * depth, depth]) + t_c_w(mid)
    p_w = p_true + 0.02 * rng.standard_normal(3)
    z = np.zeros((M, 2))
    for k, i in enumerate(clones):
        pc = R_c2w(i).T @ (p_true - t_c_w(i))
        z[k] = pc[:2] / pc[2] + sig * rng.standard_normal(2)
    if outlier and M:
        z[M // 2] += 40.0 * (1 + attempt) * sig * np.array([0.8, -0.6])
    return p_w, z, 0.05 * rng.standard_normal((M, 2))


def _assemble(poses, P, flags, tracks, obs):
    R_b2w, t_b_w, R_b2c, t_c_b = poses
    ptr = np.concatenate([[0], np.cumsum([len(c) for c in tracks])]).astype(np.int32)
    cl = np.array([i for c in tracks for i in c], dtype=np.int32)
    F = len(tracks)
    return synth.Window(R_b2w=np.ascontiguousarray(R_b2w), t_b_w=np.ascontiguousarray(t_b_w), t_fej=None, R_b2c=R_b2c, t_c_b=t_c_b,
                        p_w=np.ascontiguousarray(np.array([o[0] for o in obs]).reshape(F, 3)), obs_ptr=ptr, obs_clone=cl,
                        obs_z=np.ascontiguousarray(np.concatenate([o[1] for o in obs] + [np.zeros((0, 2))]).reshape(-1, 2)),
                        obs_zvel=np.ascontiguousarray(np.concatenate([o[2] for o in obs] + [np.zeros((0, 2))]).reshape(-1, 2)),
                        P=P, flags=flags)


def build_window(N, tracks, want, seed, flags=None):
    """A window of N clones with one track per clone list in `tracks`; want[j]: 1 the track is to be accepted, 0 rejected (one
    observation is displaced).  A track whose float64 gamma (oracle.mirror) is not clearly on the wanted side -- below 0.7 thr, above
    1.5 thr -- gets new noise until it is: a rule about the inputs, fixed before any device saw them."""
    flags = flags or synth.Flags()
    poses = _poses(N)
    rng = np.random.default_rng(seed)
    t_fej = poses[1] + 1e-3 * rng.standard_normal((N, 3))
    P = np.ascontiguousarray(synth.make_prior_cov(N, rng, flags.leg_dim, True, bool(flags.estimate_td)))
    sig = flags.noise_feature
    table = mirror.chi2_table(flags.chi2_prob, 80)
    obs = []
    for j, cl in enumerate(tracks):
        for attempt in range(64):
            o = _track_obs(poses, cl, seed, j, attempt, sig, want[j] == 0)
            if len(cl) < 2:
                break
            w1 = _assemble(poses, P, flags, [list(cl)], [o])
            w1.t_fej = np.ascontiguousarray(t_fej)
            H, r, _ = mirror.feature_jacobian_msckf(w1, 0)
            g = mirror.gating_gamma(H, r, P, sig * sig)
            thr = mirror.chi2_threshold(2 * len(cl) - 3, flags.chi2_prob, table)
            if (want[j] == 1 and g < 0.7 * thr) or (want[j] == 0 and g > 1.5 * thr):
                break
        else:
            raise AssertionError('no noise draw puts track %d on the wanted side of the gate' % j)
        obs.append(o)
    win = _assemble(poses, P, flags, [list(c) for c in tracks], obs)
    win.t_fej = np.ascontiguousarray(t_fej)
    return win


def _runs(N, lens, rng):
    out = []
    for M in lens:
        s = int(rng.integers(0, N - M + 1))
        out.append(list(range(s, s + M)))
    return out


def _routes(win, F):
    """The routes the shape admits, restated from front_fused_active / front_defers_assembly (capi_update.inc): k_front needs the
    register path of the prior's factorisation (n <= 224), at most four column passes and one workgroup per two tracks resident at
    once (F <= 510 on 256 compute units); it leaves the assembly to the next kernel while NA <= 192 (at most four partial Grams:
    always, at F <= 510)."""
    n = win.n
    NA = n - 15
    NAP = (NA + 16) // 16 * 16
    if F < 1 or n > 224 or (NAP + 63) // 64 > 4 or 1 + (F + 1) // 2 > 256:
        return ('forked',)
    return ('forked', 'deferred' if NA <= 192 else 'inlaunch')


# group a: column passes and the right-hand-side column -- (leg, N)
A_SHAPES = [(22, 4), (22, 9), (22, 10), (22, 20), (22, 21), (22, 31), (46, 29), (22, 41), (22, 42), (22, 60), (46, 60)]
B_ACCEPTED = [2, 3, 8, 9, 16, 17, 24, 25, 32]
B_REJECTED = [8, 9, 32]
F_SHAPES = [(4, 341), (4, 342), (4, 213), (4, 214), (4, 1366), (20, 17)]   # (N, F)

CASES = (['a_leg%d_N%d' % s for s in A_SHAPES] + ['b_N32', 'c_N8'] +
         ['d_N%d_%d%d%d%d' % ((N,) + f) for N in (9, 10) for f in FLAG_SETS] + ['e_N9'] + ['f_N%d_F%d' % s for s in F_SHAPES])
LEFTOVER_PAIR = ('f_N4_F1366', 'a_leg22_N4')   # group g: the large case, then the small one, on one handle


def _distinct8(N, seed):
    """Eight distinct tracks, six accepted and two rejected, of 2..3 observations (N = 4) or 3..4 covering all N clones (N = 20)."""
    if N == 4:
        tracks = [[0, 1], [1, 2, 3], [2, 3], [0, 1, 2], [1, 2], [0, 1, 2], [2, 3], [1, 2, 3]]
    else:
        starts, lens = [0, 2, 5, 8, 11, 14, 16, 17], [3, 4, 3, 4, 3, 3, 3, 3]
        tracks = [list(range(s, s + m)) for s, m in zip(starts, lens)]
    want = [1, 1, 0, 1, 1, 1, 0, 1]
    return build_window(N, tracks, want, seed), want


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """read-only"""
    g = cid[0]
    edge = {}
    if g == 'a':
        leg, N = (int(x) for x in cid[5:].split('_N'))
        rng = np.random.default_rng(900 + 7 * N + leg)
        lens = [2, 3, 4, 5, 6, min(N, 6)]
        tracks = _runs(N, [min(m, N) for m in lens], rng)
        tracks[0] = [N - 2, N - 1]                      # (the last clone's columns: next to the right-hand side)
        want = [1, 1, 0, 1, 1, 1]
        win = build_window(N, tracks, want, 1000 + N + leg, synth.Flags(leg_dim=leg))
    elif g == 'b':
        N = 32
        rng = np.random.default_rng(901)
        tracks = _runs(N, B_ACCEPTED + B_REJECTED, rng)
        want = [1] * len(B_ACCEPTED) + [0] * len(B_REJECTED)
        win = build_window(N, tracks, want, 2000)
    elif g == 'c':
        N = 8   # clone 5 is seen by no track
        tracks = [[0, 3, 7], [6, 4, 2, 1], [0, 1, 2, 3], [3], [], [2, 3, 4], [7, 6], [1, 0], [6, 7, 4]]
        want = [1, 1, 1, -1, -1, 0, 1, 1, 1]
        win = build_window(N, tracks, want, 3000)
    elif g == 'd':
        N = int(cid[3:cid.index('_', 3)])
        larvio, left, fej, td = (int(x) for x in cid[-4:])
        rng = np.random.default_rng(902 + N)
        tracks = _runs(N, [2, 3, 4, 5, 6, 3, 4, N], rng)
        want = [1, 1, 0, 1, 1, 0, 1, 1]
        win = build_window(N, tracks, want, 4000 + N, synth.Flags(use_larvio=larvio, use_left_perturbation=left, if_fej=fej, estimate_td=td))
    elif g == 'e':
        win, edge = _edge_window()
        want = [1 if edge[j] < 0 else 0 for j in range(win.F)]
    elif g == 'f':
        N, F = (int(x) for x in cid[3:].split('_F'))
        base, w8 = _distinct8(N, 5000 + N)
        sl = [slice(int(base.obs_ptr[k]), int(base.obs_ptr[k + 1])) for k in range(8)]
        ks = [j % 8 for j in range(F)]
        tracks = [list(base.obs_clone[sl[k]]) for k in ks]
        win = _assemble((base.R_b2w, base.t_b_w, base.R_b2c, base.t_c_b), base.P, base.flags, tracks,
                        [(base.p_w[k], base.obs_z[sl[k]], base.obs_zvel[sl[k]]) for k in ks])
        win.t_fej = base.t_fej
        want = [w8[k] for k in ks]
        rep = np.array(ks, dtype=np.int64)
    else:
        raise KeyError(cid)
    if g != 'f':
        rep = np.arange(win.F)
    for a in (win.R_b2w, win.t_b_w, win.t_fej, win.R_b2c, win.t_c_b, win.p_w, win.obs_ptr, win.obs_clone, win.obs_z, win.obs_zvel, win.P):
        a.setflags(write=False)
    return Case(cid, win, _routes(win, win.F), rep, np.array(want, dtype=np.int64), edge)


def routes_of(cid):
    return make_case(cid).routes


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def _mpf_of_ld(x):
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


def _ld_of_mpf(v):
    hi = float(v)
    return LD(hi) + LD(float(v - mp.mpf(hi)))


def threshold(win, M):
    return mirror.chi2_threshold(2 * M - 3, win.flags.chi2_prob)


def track_rows_mp(win, j):
    """The un-projected rows of track j in mp, on the columns it touches: (idx [k] active columns, the last one NA = the right-hand
    side; rows [2M] lists of (position in idx, value); Hf [2M][3]; state [k - 1] the state columns behind idx[:-1])."""
    mp.mp.dps = DIGITS
    Hx, r, Hf = mpr.feature_jacobian_msckf_mp(win, j)
    n, M2 = win.n, Hx.rows
    NA = n - 15
    cols = [c for c in range(15, n) if any(Hx[i, c] != 0 for i in range(M2))]
    assert not any(Hx[i, c] != 0 for i in range(M2) for c in range(15))
    rows = [[(p, Hx[i, c]) for p, c in enumerate(cols) if Hx[i, c] != 0] + [(len(cols), r[i])] for i in range(M2)]
    return np.array([c - 15 for c in cols] + [NA]), rows, [[Hf[i, t] for t in range(3)] for i in range(M2)], cols


def _gamma_mp(win, rows, Hf, state, e_mode):
    k1 = len(state)
    M2 = len(rows)
    s2 = mp.mpf(float(win.flags.noise_feature)) ** 2
    Pd = np.asarray(win.P)[np.ix_(state, state)]
    hrows = [[(p, v) for p, v in row if p < k1] for row in rows]
    rv = [row[-1][1] for row in rows]
    if e_mode == 'mp':
        Pm = [[mp.mpf(float(Pd[a, b])) for b in range(k1)] for a in range(k1)]
        T = [[mp.fsum(v * Pm[a][b] for a, v in hr) for b in range(k1)] for hr in hrows]
        E = [[mp.fsum(T[i][b] * v for b, v in hrows[i2]) for i2 in range(M2)] for i in range(M2)]
    else:
        Hc = np.zeros((M2, k1), dtype=LD)
        for i, hr in enumerate(hrows):
            for p, v in hr:
                Hc[i, p] = _ld_of_mpf(v)
        El = Hc @ Pd.astype(LD) @ Hc.T
        E = [[_mpf_of_ld(El[i, i2]) for i2 in range(M2)] for i in range(M2)]
    B = mp.matrix(Hf)
    C = mp.inverse(B.T * B)
    Em = mp.matrix(E)
    Em = (Em + Em.T) / 2
    EB = Em * B
    BC = B * C
    S = Em - BC * EB.T - EB * BC.T + BC * (B.T * EB) * BC.T + s2 * mp.eye(M2)
    r = mp.matrix(rv)
    pr = r - BC * (B.T * r)
    return (pr.T * mp.lu_solve(S, pr))[0]


@functools.lru_cache(maxsize=None)
def _reference(cid, j, e_mode=None):
    """read-only; dict(idx, G [k, k] longdouble, G0d [k] the diagonal of G0, B [k, k], gamma, dof, thr, accept) of track j"""
    case = make_case(cid)
    win = case.win
    M = int(win.obs_ptr[j + 1] - win.obs_ptr[j])
    assert M >= 2
    mp.mp.dps = DIGITS
    idx, rows, Hf, state = track_rows_mp(win, j)
    k = len(idx)
    G0 = [[mp.mpf(0)] * k for _ in range(k)]
    W = [[mp.mpf(0)] * k for _ in range(3)]
    for row, hf in zip(rows, Hf):
        for a, va in row:
            for t in range(3):
                W[t][a] += hf[t] * va
            Ga = G0[a]
            for b, vb in row:
                Ga[b] += va * vb
    Bm = mp.matrix(Hf)
    C = mp.inverse(Bm.T * Bm)
    Y = [[C[t, 0] * W[0][b] + C[t, 1] * W[1][b] + C[t, 2] * W[2][b] for b in range(k)] for t in range(3)]
    G = np.array([[_ld_of_mpf(G0[a][b] - (W[0][a] * Y[0][b] + W[1][a] * Y[1][b] + W[2][a] * Y[2][b])) for b in range(k)] for a in range(k)])
    G0d = np.array([float(G0[a][a]) for a in range(k)])
    mode = e_mode or ('mp' if M <= E_MP_MAX_M else 'ld')
    gam = float(_gamma_mp(win, rows, Hf, state, mode))
    thr = threshold(win, M)
    out = dict(idx=idx, G=G, G0d=G0d, B=np.sqrt(np.outer(G0d, G0d)), gamma=gam, dof=2 * M - 3, thr=thr, accept=int(gam < thr))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def reference(case, j, e_mode=None):
    return _reference(case.cid, int(case.rep[j]), e_mode)


def track_reference(case, j):
    """(G_j, G0_j's diagonal, gamma_j, dof) of track j, G_j on all NA + 1 columns (longdouble)."""
    ref = reference(case, j)
    G = np.zeros((case.NA + 1, case.NA + 1), dtype=LD)
    G[np.ix_(ref['idx'], ref['idx'])] = ref['G']
    d = np.zeros(case.NA + 1)
    d[ref['idx']] = ref['G0d']
    return G, d, ref['gamma'], ref['dof']


def live_tracks(case):
    win = case.win
    return [j for j in range(win.F) if win.obs_ptr[j + 1] - win.obs_ptr[j] >= 2]


@functools.lru_cache(maxsize=None)
def window_reference(cid):
    """read-only; (sum over the accepted tracks of G_j, of B_j) on all NA + 1 columns, and accept [F], gamma [F] (NaN below two
    observations)"""
    case = make_case(cid)
    n1 = case.NA + 1
    G, B = np.zeros((n1, n1), dtype=LD), np.zeros((n1, n1), dtype=LD)
    acc, gam = np.zeros(case.win.F, dtype=np.int32), np.full(case.win.F, np.nan)
    count = {}
    for j in live_tracks(case):
        ref = reference(case, j)
        acc[j], gam[j] = ref['accept'], ref['gamma']
        if ref['accept']:
            count[int(case.rep[j])] = count.get(int(case.rep[j]), 0) + 1
    for k, c in count.items():
        ref = _reference(cid, k, None)
        ix = np.ix_(ref['idx'], ref['idx'])
        G[ix] += c * ref['G']
        B[ix] += c * ref['B'].astype(LD)
    for a in (G, B, acc, gam):
        a.setflags(write=False)
    return G, B, acc, gam


# ---- group e: tracks at the edge of the gate ---------------------------------------------------------------------------------------------
EDGE_LENGTHS = [2, 8, 9]
EDGE_REL = 1e-8


def _edge_window():
    """Tracks of 2, 8 and 9 observations, each twice: the residual of the first copy rescaled until the mp gamma stands at
    thr (1 - 1e-8), that of the second at thr (1 + 1e-8).  r is linear in obs_z with slope one, so z <- z + (s - 1) r multiplies r by
    s and gamma by s^2; the double rounding of z is taken out by secant steps on the mp gamma."""
    N = 9
    rng = np.random.default_rng(903)
    singles = [list(range(s, s + m)) for m in EDGE_LENGTHS for s in [int(rng.integers(0, N - m + 1))]]
    b3 = build_window(N, singles, [1] * len(singles), 6000)
    sl3 = [slice(int(b3.obs_ptr[k]), int(b3.obs_ptr[k + 1])) for k in range(len(singles))]
    ks = [k for k in range(len(singles)) for _ in range(2)]
    base = _assemble((b3.R_b2w, b3.t_b_w, b3.R_b2c, b3.t_c_b), b3.P, b3.flags, [singles[k] for k in ks],
                     [(b3.p_w[k], b3.obs_z[sl3[k]], b3.obs_zvel[sl3[k]]) for k in ks])
    base.t_fej = b3.t_fej
    z = np.array(base.obs_z)
    edge = {}
    for j in range(len(ks)):
        side = -1 if j % 2 == 0 else 1
        target = threshold(base, len(singles[ks[j]])) * (1.0 + side * EDGE_REL)
        sl = slice(int(base.obs_ptr[j]), int(base.obs_ptr[j + 1]))
        for _ in range(6):
            w = dataclasses.replace(base, obs_z=z)
            _, rows, Hf, state = track_rows_mp(w, j)
            g = _gamma_mp(w, rows, Hf, state, 'mp')
            if abs(float(g) / target - 1.0) < 1e-11:
                break
            s = float(mp.sqrt(mp.mpf(target) / g))
            _, r, _ = mirror.feature_jacobian_msckf(w, j, project=False)
            z[sl] += (s - 1.0) * r.reshape(-1, 2)
        else:
            raise AssertionError('the secant steps did not reach the edge')
        edge[j] = side
    return dataclasses.replace(base, obs_z=np.ascontiguousarray(z)), edge


# ---- the derived summation terms -----------------------------------------------------------------------------------------------------
def gram_chain(rows, nwaves):
    """the longest chain of additions behind one element of a Gram tile of gramw_body over `rows` rows by `nwaves` wavefronts"""
    if rows <= 0:
        return 0
    rw = (-(-rows // nwaves) + 3) // 4 * 4
    return 4 * (-(-rw // 8)) + 1 + int(math.log2(nwaves))


def forked_chunks(F):
    """(chunks, rows per chunk) of k_gram_pair: upload_finalize (capi_update.inc)"""
    chunks = max(1, min((3 * F + 1023) // 1024, 64))
    rpc = max(8, (-(-3 * F // chunks) + 7) // 8 * 8)
    return (-(-3 * F // rpc) if F else 1), rpc


def fused_chunks(F):
    """(chunks, rows per chunk) of k_front's Gram items: front_row_chunks, launch_front"""
    chunks = max(1, (3 * F + 639) // 640)
    return chunks, (-(-3 * F // chunks) + 3) // 4 * 4


def clone_rows(win):
    return 2 * np.bincount(live_obs_clones(win), minlength=win.N)


def live_obs_clones(win):
    return np.asarray(win.obs_clone[int(win.obs_ptr[0]):int(win.obs_ptr[-1])], dtype=np.int64)


def summation_c(case, route, chunks=None, rpc=None):
    """c of the bar of A for this case on this route (doc-string): derived from the row counts, not measured"""
    win = case.win
    nw = 16 if route == 'forked' else 8
    if chunks is None:
        chunks, rpc = forked_chunks(win.F) if route == 'forked' else fused_chunks(win.F)
    c_s = max(gram_chain(int(r), nw) for r in clone_rows(win)) + -(-win.N // 8) + 3
    c_t = gram_chain(min(rpc, 3 * win.F), nw) + -(-chunks // 4) + 2
    return c_s + c_t + 2


# ---- the column map and the position list, restated ---------------------------------------------------------------------------------
def positions(win):
    """obs_pos: the position of every observation in the stable sort by clone (upload_finalize)"""
    oc = np.asarray(win.obs_clone, dtype=np.int64)
    pos = np.empty(len(oc), dtype=np.int32)
    pos[np.argsort(oc, kind='stable')] = np.arange(len(oc), dtype=np.int32)
    return pos


def rows_to_active(x16, clone, case):
    """a row pair of Xobs [2, 16] = [H_e(6) td | H_x(6) | r | 0 0] on the NA + 1 active columns (assemble_entry's map)"""
    X = np.zeros((x16.shape[0], case.NA + 1), dtype=x16.dtype)
    X[:, 0:7] = x16[:, 0:7]
    X[:, case.cb0 + 6 * clone: case.cb0 + 6 * clone + 6] = x16[:, 7:13]
    X[:, case.NA] = x16[:, 13]
    return X


def track_X(case, got, j):
    """the un-projected rows of track j gathered from Xobs through the position list: [2M, NA + 1]"""
    win = case.win
    lo, hi = int(win.obs_ptr[j]), int(win.obs_ptr[j + 1])
    out = []
    for o in range(lo, hi):
        p = int(got['obs_pos'][o])
        out.append(rows_to_active(got['Xobs'][2 * p: 2 * p + 2], int(win.obs_clone[o]), case))
    return np.concatenate(out) if out else np.zeros((0, case.NA + 1))


def row_ptr(win):
    M = np.diff(np.asarray(win.obs_ptr, dtype=np.int64))
    return np.concatenate([[0], np.cumsum(np.where(M >= 2, 2 * M - 3, 0))])


# ---- the checkers (device buffers, or the float64 stand-in) --------------------------------------------------------------------------
def _unit_err(got, ref, B):
    """max |got - ref| / (u B) where B > 0; (figure, were the entries with B == 0 exactly zero?)"""
    d = np.abs(np.asarray(got, dtype=LD) - ref)
    pos = B > 0
    fig = float((d[pos] / (U * B[pos].astype(LD))).max()) if pos.any() else 0.0
    return fig, not np.asarray(got)[~pos].any()


def check_tracks(case, got, need=('gamma', 'gram', 'Hs')):
    """Every track on its own.  got: gamma, accept [F]; T3 [3F, NAP], Xobs [2 nobs, 16], obs_pos [nobs], Hs [m_tot, NAP].  Returns
    (figures dict: the worst per quantity in its unit, problems list); the caller asserts the list empty."""
    win = case.win
    NA = case.NA
    fig = dict(gamma=0.0, gram=0.0, Hs=0.0)
    bad = []
    _, _, acc, gam = window_reference(case.cid)
    if not np.array_equal(np.asarray(got['accept'], dtype=np.int32), acc):
        bad.append(('accept', np.nonzero(np.asarray(got['accept']) != acc)[0].tolist()))
    rp = row_ptr(win)
    if 'gram' in need and not np.array_equal(np.asarray(got['obs_pos'])[int(win.obs_ptr[0]):], positions(win)[int(win.obs_ptr[0]):]):
        bad.append(('obs_pos',))
    for j in range(win.F):
        M = int(win.obs_ptr[j + 1] - win.obs_ptr[j])
        if M < 2:
            if not (np.isnan(got['gamma'][j]) and got['accept'][j] == 0):
                bad.append(('short track', j))
            if 'gram' in need and (got['T3'][3 * j: 3 * j + 3].any() or track_X(case, got, j).any()):
                bad.append(('short track rows', j))
            continue
        ref = reference(case, j)
        e = abs(float(got['gamma'][j]) - ref['gamma']) / (U * ref['gamma'])
        fig['gamma'] = max(fig['gamma'], e)
        if not e <= K_GAMMA:
            bad.append(('gamma', j, e))
        if 'gram' not in need:
            continue
        T3 = got['T3'][3 * j: 3 * j + 3]
        X = track_X(case, got, j)
        Hs = got['Hs'][rp[j]: rp[j + 1]] if 'Hs' in need else None
        if not acc[j]:
            if T3.any() or X.any() or (Hs is not None and Hs.any()):
                bad.append(('rows of a rejected track', j))
            continue
        if T3[:, NA + 1:].any() or (Hs is not None and Hs[:, NA + 1:].any()):
            bad.append(('padding columns', j))
        Gref = np.zeros((NA + 1, NA + 1), dtype=LD)
        Bj = np.zeros((NA + 1, NA + 1))
        ix = np.ix_(ref['idx'], ref['idx'])
        Gref[ix] = ref['G']
        Bj[ix] = ref['B']
        Xl, Tl = X.astype(LD), T3[:, :NA + 1].astype(LD)
        e, zero = _unit_err(Xl.T @ Xl - Tl.T @ Tl, Gref, Bj)
        fig['gram'] = max(fig['gram'], e)
        if not (e <= K_G and zero):
            bad.append(('gram', j, e, zero))
        if Hs is not None:
            Hl = Hs[:, :NA + 1].astype(LD)
            e, zero = _unit_err(Hl.T @ Hl, Gref, Bj)
            fig['Hs'] = max(fig['Hs'], e)
            if not (e <= K_G and zero):
                bad.append(('Hs', j, e, zero))
    return fig, bad


def check_window(case, got, route):
    """The window's sums.  got: Xobs, T3, S [N, 16, 16], Gpart [chunks, NAP, NAP], A [NAP, NAP], chunks, rows_per_chunk.  Returns
    (figures, problems)."""
    win = case.win
    NA, NAP, N = case.NA, case.NAP, win.N
    nw = 16 if route == 'forked' else 8
    fig = dict(S=0.0, Gpart=0.0, A=0.0)
    bad = []
    # S[c]: the Gram of the clone's rows of Xobs, both triangles
    crow = np.concatenate([[0], np.cumsum(clone_rows(win))])
    for c in range(N):
        Xc = got['Xobs'][crow[c]: crow[c + 1]]
        ref = Xc.astype(LD).T @ Xc.astype(LD)
        mag = np.abs(Xc).T @ np.abs(Xc)
        ch = max(gram_chain(Xc.shape[0], nw), 1)
        e, zero = _unit_err(got['S'][c], ref, ch * mag)
        fig['S'] = max(fig['S'], e)
        if not (e <= 1.0 and zero):
            bad.append(('S', c, e, zero))
    # sum Gpart = T3^T T3 on the lower tiles
    T3 = got['T3'].astype(LD)
    chunks, rpc = int(got['chunks']), int(got['rows_per_chunk'])
    if chunks != got['Gpart'].shape[0] or chunks * rpc < T3.shape[0]:
        bad.append(('chunks', chunks, rpc))
    low = (np.arange(NAP)[:, None] // 16) >= (np.arange(NAP)[None, :] // 16)
    ref = T3.T @ T3
    mag = np.abs(got['T3']).T @ np.abs(got['T3'])
    ch = gram_chain(min(rpc, T3.shape[0]), nw) + chunks   # (the chunks are summed here, in longdouble: no more than one rounding each)
    gs = got['Gpart'].astype(LD).sum(axis=0)
    e, zero = _unit_err(gs[low], ref[low], ch * mag[low])
    fig['Gpart'] = max(fig['Gpart'], e)
    if not (e <= 1.0 and zero):
        bad.append(('Gpart', e, zero))
    # A
    A = got['A']
    Gsum, Bsum, acc, _ = window_reference(case.cid)
    c = summation_c(case, route, chunks, rpc)
    e, zero = _unit_err(A[:NA + 1, :NA + 1], Gsum, np.asarray(Bsum, dtype=np.float64))
    fig['A'] = max(fig['A'], e)
    fig['A_bar'] = K_G + c
    if not (e <= K_G + c and zero):
        bad.append(('A', e, K_G + c, zero))
    if not np.array_equal(A, A.T):
        bad.append(('A not symmetric',))
    if A[NA + 1:].any() or A[:, NA + 1:].any():
        bad.append(('A beyond NA',))
    seen = np.zeros(N, dtype=bool)
    for j in np.nonzero(acc)[0]:
        seen[np.asarray(win.obs_clone[win.obs_ptr[j]: win.obs_ptr[j + 1]])] = True
    for cl in np.nonzero(~seen)[0]:
        s = slice(case.cb0 + 6 * cl, case.cb0 + 6 * cl + 6)
        if A[s].any() or A[:, s].any():
            bad.append(('columns of an unobserved clone', int(cl)))
    return fig, bad


# ---- the two float64 restatements against the reference --------------------------------------------------------------------------------
def restatement_figures(case):
    """dict(mirror_G, mirror_gamma, oracle_G, oracle_gamma): the worst error over the case's tracks of oracle.mirror's projected rows
    (SVD) and gamma, and of the C oracle's (H_all / r_all, gamma), in u B_j and in u."""
    from oracle import oracle as orc
    win = case.win
    out = dict(mirror_G=0.0, mirror_gamma=0.0, oracle_G=0.0, oracle_gamma=0.0)
    c = orc.msckf_update(win, want_K=False)
    s2 = win.flags.noise_feature ** 2
    for j in sorted(set(int(case.rep[j]) for j in live_tracks(case))):
        ref = reference(case, j)
        st = np.concatenate([ref['idx'][:-1] + 15, [0]])
        H, r, _ = mirror.feature_jacobian_msckf(win, j)
        b0, b1 = int(c['block_ptr'][j]), int(c['block_ptr'][j + 1])
        for name, Hp, rp, g in (('mirror', H, r, mirror.gating_gamma(H, r, win.P, s2)), ('oracle', c['H_all'][b0:b1], c['r_all'][b0:b1], c['gamma'][j])):
            Z = np.concatenate([Hp[:, st[:-1]], rp[:, None]], axis=1).astype(LD)
            e, _ = _unit_err(Z.T @ Z, ref['G'], ref['B'])
            out[name + '_G'] = max(out[name + '_G'], e)
            out[name + '_gamma'] = max(out[name + '_gamma'], abs(float(g) - ref['gamma']) / (U * ref['gamma']))
    return out


# ---- the float64 stand-in for the device -----------------------------------------------------------------------------------------------
def assemble_model(case, S, Gpart, rhs_e=13):
    """assemble_entry in numpy: A = scatter(sum S) - sum Gpart, the lower tiles mirrored.  rhs_e: the entry of a sparse row the
    right-hand-side column reads (13; a mutation reads 12)."""
    NA, NAP, N, cb0 = case.NA, case.NAP, case.win.N, case.cb0
    e_of = np.full(NAP, -1)
    c_of = np.full(NAP, -1)
    e_of[:7] = np.arange(7)
    e_of[NA] = rhs_e
    for c in range(N):
        e_of[cb0 + 6 * c: cb0 + 6 * c + 6] = 7 + np.arange(6)
        c_of[cb0 + 6 * c: cb0 + 6 * c + 6] = c
    A = np.zeros((NAP, NAP))
    Ssum = S.sum(axis=0)
    for i in range(NAP):
        for k in range(NAP):
            if e_of[i] < 0 or e_of[k] < 0:
                continue
            ei, ek = max(e_of[i], e_of[k]), min(e_of[i], e_of[k])
            if c_of[i] < 0 and c_of[k] < 0:
                A[i, k] = Ssum[ei, ek]
            elif c_of[i] >= 0 and c_of[k] >= 0:
                A[i, k] = S[c_of[i], ei, ek] if c_of[i] == c_of[k] else 0.0
            else:
                A[i, k] = S[max(c_of[i], c_of[k]), ei, ek]
    g = Gpart.sum(axis=0)
    low = (np.arange(NAP)[:, None] // 16) >= (np.arange(NAP)[None, :] // 16)
    g = np.where(low, g, g.T)
    return A - g


def model_grams(case, Xobs, T3, chunks, rpc, drop_row=None):
    """S [N, 16, 16] and Gpart [chunks, NAP, NAP] from the rows, summed in longdouble and rounded once (the bars of S and Gpart are
    those of the device's summation tree, not of a BLAS loop); drop_row: a row of T3 the Grams lose (a mutation)"""
    Xobs, T3 = Xobs.astype(LD), T3.astype(LD)
    win = case.win
    crow = np.concatenate([[0], np.cumsum(clone_rows(win))])
    S = np.stack([Xobs[crow[c]: crow[c + 1]].T @ Xobs[crow[c]: crow[c + 1]] for c in range(win.N)]).astype(np.float64)
    G = np.zeros((chunks, case.NAP, case.NAP))
    for ch in range(chunks):
        rows = [r for r in range(ch * rpc, min((ch + 1) * rpc, T3.shape[0])) if r != drop_row]
        G[ch] = T3[rows].T @ T3[rows]
    return S, G


def model_front(case):
    """The front end in float64 numpy from oracle.mirror's rows: what check_tracks and check_window take (forked chunking)."""
    win = case.win
    NA, NAP, F = case.NA, case.NAP, win.F
    nobs = int(win.obs_ptr[-1])
    pos = positions(win)
    rp = row_ptr(win)
    s2 = win.flags.noise_feature ** 2
    T3 = np.zeros((3 * F, NAP))
    Xobs = np.zeros((2 * nobs, 16))
    Hs = np.zeros((int(rp[-1]), NAP))
    gamma, accept = np.full(F, np.nan), np.zeros(F, dtype=np.int32)
    done = {}
    for j in range(F):
        lo, hi = int(win.obs_ptr[j]), int(win.obs_ptr[j + 1])
        if hi - lo < 2:
            continue
        k = int(case.rep[j])
        if k not in done:
            Hx, r, Hf = mirror.feature_jacobian_msckf(win, k, project=False)
            Q, _ = np.linalg.qr(Hf, mode='complete')
            X = np.concatenate([Hx[:, 15:], r[:, None]], axis=1)
            Y = Q.T @ X
            g = mirror.gating_gamma(Y[3:, :NA] @ np.eye(NA, win.n, 15), Y[3:, NA], win.P, s2)
            done[k] = (X, Y, g, int(g < threshold(win, hi - lo)))
        X, Y, g, ok = done[k]
        gamma[j], accept[j] = g, ok
        if not ok:
            continue
        T3[3 * j: 3 * j + 3, :NA + 1] = Y[:3]
        Hs[rp[j]: rp[j + 1], :NA + 1] = Y[3:]
        for t, o in enumerate(range(lo, hi)):
            c = int(win.obs_clone[o])
            x = np.zeros((2, 16))
            x[:, 0:7] = X[2 * t: 2 * t + 2, 0:7]
            x[:, 7:13] = X[2 * t: 2 * t + 2, case.cb0 + 6 * c: case.cb0 + 6 * c + 6]
            x[:, 13] = X[2 * t: 2 * t + 2, NA]
            Xobs[2 * pos[o]: 2 * pos[o] + 2] = x
    chunks, rpc = forked_chunks(F)
    S, G = model_grams(case, Xobs, T3, chunks, rpc)
    return dict(gamma=gamma, accept=accept, T3=T3, Xobs=Xobs, obs_pos=pos, Hs=Hs, S=S, Gpart=G, A=assemble_model(case, S, G),
                chunks=chunks, rows_per_chunk=rpc)
