"""Inputs, references and bars of the tests of the resident covariance's edits and of the square-root factor that follows them
(CPU: tests/test_cov_cases.py, device: tests/test_gpu_cov_edits.py).

Priors.  graded_factorable(n, seed): potrf_cases.graded at cond 1e4 over four decades -- a prior whose factor exists and whose
Cholesky drops no pivot (asserted with potrf_cases.tile_chol, the float64 mirror of the device's tile algorithm).  graded_prior(n, seed):
harsher, for the edits that need no factor -- a correlation matrix from a rank-4 factor model plus a diagonal, times s s^T with
s = 10**uniform(-6, 1) per state (variances over fourteen decades: bias against position).  Both exactly symmetric.
Phi = I + 0.05 randn with O(0.5) blocks at (6:9, 3:6) and (0:3, 9:12); Q = G G^T, the rows of G scaled by 10**uniform(-6, -2).

Propagation.  Reference in np.longdouble: P_LL' = Phi P_LL Phi^T + (Q + Q^T) / 2, P_LC' = Phi P_LC, P_CL' its transpose, P_CC as it stands.
Bar per element, derived and not measured: (2 leg + 4) 2^-53 B with
    IMU block    B = |Phi| |P_LL| |Phi|^T + (|Q| + |Q|^T) / 2
    cross block  B = |Phi| |P_LC|
u = 2^-53.  Each element is two nested dot products of length leg (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
section 3.1: |fl(x^T y) - x^T y| <= gamma_k |x|^T |y| with gamma_k = k u / (1 - k u), for ANY order of summation, with or without fused
multiply-add).  The inner product T = Phi P carries gamma_leg; the outer one, T Phi^T with Q added as one more term, gamma_(leg + 1)
on top of it; the symmetrisation's sum is one more rounding and its halving is exact: (1 + u)^(2 leg + 2) - 1 in all, which
(2 leg + 4) u covers with the second-order terms at leg <= 46.  The cross blocks are the inner product alone and are held to the same
factor.  P_CC must equal the input bit for bit and the output must be exactly symmetric.
The numpy mirror (oracle/mirror_cov.propagate) uses 0.10 of the bar at worst over PROP_SHAPES (tests/test_cov_cases.py asserts < 0.5: the bar
is not loose by decades).  Device figures: docs/LAB_NOTES.md.

Index edits.  P: oracle/mirror_cov.py and tests/mirror_features_lifecycle.rm_lost_features_cov.  S: row maps new state -> old state
written out here as plain numpy deletion and permutation, independent of the library (P_after = P[map][:, map], S_after = S[map]).
lost_unmap_np restates the 512-bit walk of the frame head (frame_ops.hpp, lost_unmap), so that the CPU test can compare it -- and its
mutations -- with plain deletion.

Expected tail.  expected_tail(ops) restates the documented rule for the trailing-zero structure of S (rows >= 15 zero in the last 15
columns): a reversed prefactor makes it 15; gather, permute and change of anchors keep it; augment, zupt and a forward prefactor make
it 0.  Written here, not read from the library."""
from __future__ import annotations

import functools

import numpy as np

import potrf_cases as pc
from oracle import mirror_cov as mc
import mirror_features_lifecycle as mfl

LD = pc.LD
U53 = 2.0 ** -53
FACTOR_COND = 1e4
OLD_FROBENIUS_BAR = 1e-14   # tests/test_gpu_cov.py::test_propagate


# ---- priors, Phi, Q -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graded_factorable(n, seed=0):
    """read-only; cond 1e4, four decades; no pivot dropped forward or reversed (what cov_prefactor factors)"""
    X = pc.graded(n, 1000 + n + seed, FACTOR_COND)
    for M in (X, pc.reverse(X)):
        t = pc.tile_chol(M, pc.TOL_PRIOR)
        assert not t['dropped'] and not t['negative'], (n, seed)
    return X


@functools.lru_cache(maxsize=None)
def graded_prior(n, seed=0):
    """read-only; correlation matrix of a rank-4 factor model plus a diagonal, times s s^T, s = 10**uniform(-6, 1)"""
    rng = np.random.default_rng(50021 + 131 * n + seed)
    F = rng.standard_normal((n, 4))
    C = F @ F.T + np.diag(rng.uniform(0.2, 1.0, n))
    d = np.sqrt(np.diag(C))
    C = C / np.outer(d, d)
    s = 10.0 ** rng.uniform(-6.0, 1.0, n)
    P = C * np.outer(s, s)
    P = np.ascontiguousarray(0.5 * (P + P.T))
    P.setflags(write=False)
    return P


def phi_q(leg, seed):
    rng = np.random.default_rng(70001 + 17 * leg + seed)
    Phi = np.eye(leg) + 0.05 * rng.standard_normal((leg, leg))
    Phi[6:9, 3:6] += 0.5 * rng.standard_normal((3, 3))
    Phi[0:3, 9:12] += 0.5 * rng.standard_normal((3, 3))
    G = rng.standard_normal((leg, 12)) * (10.0 ** rng.uniform(-6.0, -2.0, leg))[:, None]
    Q = G @ G.T
    return np.ascontiguousarray(Phi), np.ascontiguousarray(Q)


# (leg, N, extra): N = 0 and 1, both legs; n = 64 three ways and 65; an extra block behind the clones; full windows of 40 clones
PROP_SHAPES = ((22, 0, 0), (22, 1, 0), (46, 0, 0), (22, 7, 0), (22, 7, 1), (46, 3, 0), (22, 4, 9), (22, 40, 0), (46, 40, 0))


@functools.lru_cache(maxsize=None)
def prop_case(leg, N, extra):
    """dict(P, Phi, Q, ref [long double], bar [float64, zero in P_CC], ref64): computed once, shared, read-only"""
    n = leg + 6 * N + extra
    P = graded_prior(n, leg)
    Phi, Q = phi_q(leg, n)
    ref, bar = prop_reference(P, Phi, Q)
    out = dict(P=P, Phi=Phi, Q=Q, ref=ref, bar=bar, ref64=ref.astype(np.float64), leg=leg, n=n)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def prop_reference(P, Phi, Q):
    """(reference in long double, bar per element); the bar is zero on P_CC, where bit equality is asked"""
    leg, n = Phi.shape[0], P.shape[0]
    Pl, Fl, Ql = np.asarray(P, dtype=LD), np.asarray(Phi, dtype=LD), np.asarray(Q, dtype=LD)
    ref = Pl.copy()
    ref[:leg, :leg] = Fl @ Pl[:leg, :leg] @ Fl.T + (Ql + Ql.T) / 2
    ref[:leg, leg:] = Fl @ Pl[:leg, leg:]
    ref[leg:, :leg] = ref[:leg, leg:].T
    aP, aF, aQ = np.abs(Pl), np.abs(Fl), np.abs(Ql)
    B = np.zeros((n, n), dtype=LD)
    B[:leg, :leg] = aF @ aP[:leg, :leg] @ aF.T + (aQ + aQ.T) / 2
    B[:leg, leg:] = aF @ aP[:leg, leg:]
    B[leg:, :leg] = B[:leg, leg:].T
    return ref, ((2 * leg + 4) * U53 * B).astype(np.float64)


def check_propagation(got, P, ref, bar, leg):
    """exactly symmetric, P_CC bit for bit, every other element within its bar; returns the largest |got - ref| / bar"""
    assert got.shape == P.shape and np.isfinite(got).all()
    assert np.array_equal(got, got.T), 'not exactly symmetric'
    assert np.array_equal(got[leg:, leg:], P[leg:, leg:]), 'P_CC changed'
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    m = bar > 0
    assert not err[~m].any(), 'an element with a zero bar differs'
    frac = float(np.max(err[m] / bar[m])) if m.any() else 0.0
    assert frac <= 1.0, ('propagation outside its bar', frac, np.unravel_index(np.argmax(np.where(m, err / np.where(m, bar, 1.0), 0.0)), bar.shape))
    return frac


def frobenius(got, ref64):
    return float(np.linalg.norm(got - ref64) / np.linalg.norm(ref64))


# ---- row maps: new state -> old state ---------------------------------------------------------------------------------------------------
def augment_map(n, rest=0):
    """the new clone (theta <- 0:3, p <- 6:9) behind the clones and in front of the `rest` states"""
    pose = n - rest
    return np.r_[np.arange(pose), [0, 1, 2, 6, 7, 8], np.arange(pose, n)].astype(np.int64)


def remove_clones_map(n, leg, clones):
    gone = np.concatenate([np.arange(leg + 6 * c, leg + 6 * c + 6) for c in clones]) if len(clones) else np.zeros(0, np.int64)
    return np.delete(np.arange(n), gone)


def nuisance_map(n, leg, clones):
    """the listed clones (window ranks before the call, ascending): their blocks to the end in the listed order, the rest moves up"""
    assert list(clones) == sorted(set(clones))
    blocks = [np.arange(leg + 6 * c, leg + 6 * c + 6) for c in clones]
    return np.r_[remove_clones_map(n, leg, clones), np.concatenate(blocks)].astype(np.int64) if blocks else np.arange(n)


def remove_features_map(n, leg, N, d, slots):
    base = leg + 6 * N
    gone = np.concatenate([np.arange(base + d * s, base + d * s + d) for s in slots]) if len(slots) else np.zeros(0, np.int64)
    return np.delete(np.arange(n), gone)


def apply_map(P, m):
    return np.ascontiguousarray(P[np.ix_(m, m)])


# ---- the frame head's 512-bit walk, restated -------------------------------------------------------------------------------------------
LOST_WORDS = 8


def lost_bits(slots):
    bits = [0] * LOST_WORDS
    for s in slots:
        bits[s >> 6] |= 1 << (s & 63)
    return bits


def lost_unmap_np(o, count, fbase, idp, nkeep, bits, word_shift=0, carry=True):
    """output index o (the state after the removal) -> its index before it.  word_shift, carry: the mutations of tests/test_cov_cases.py"""
    if count == 0 or o < fbase:
        return o
    k = o - fbase
    slot, r = divmod(k, idp)
    if slot >= nkeep:
        return o + idp * count
    s, w = slot, 0
    while w < LOST_WORDS - 1:
        z = 64 - bin(bits[w]).count('1')
        if s < z:
            break
        if carry:
            s -= z
        w += 1
    free = ~bits[w] & ((1 << 64) - 1)
    for _ in range(s):
        free &= free - 1
    first = (free & -free).bit_length() - 1   # (the device's __ffsll(fr) - 1; -1 if no bit is left)
    return fbase + idp * (64 * (w + word_shift) + first) + r


def head_map(n, leg, N, d, nf, slots, augment, **mut):
    """The frame head's gather as the library enumerates it: the state AFTER augmentation and removal -> the state before both.
    n = leg + 6 N + d nf (+ nothing behind: the frame call takes no nuisance block with events).  mut: nkeep_short, word_shift, carry."""
    assert n == leg + 6 * N + d * nf
    count = len(slots)
    nkeep = nf - count - mut.pop('nkeep_short', 0)
    pose = leg + 6 * N if augment else -1
    fbase = leg + 6 * N + (6 if augment else 0)
    bits = lost_bits(slots)
    m = n + (6 if augment else 0) - d * count
    out = np.zeros(m, dtype=np.int64)
    for o in range(m):
        p = lost_unmap_np(o, count, fbase, d, nkeep, bits, **mut)
        if pose < 0:
            out[o] = p
        elif pose <= p < pose + 6:
            out[o] = (0, 1, 2, 6, 7, 8)[p - pose]
        else:
            out[o] = p if p < pose else p - 6
    return out


def head_map_plain(n, leg, N, d, nf, slots, augment):
    """the same by plain numpy: augmentation's map, then deletion of the lost features' rows (which stand behind the new clone)"""
    if not augment:
        return remove_features_map(n, leg, N, d, slots)
    a = augment_map(n, d * nf)
    return a[remove_features_map(n + 6, leg, N + 1, d, slots)]


# (idp, N, n_feature_states, lost slots): 170 states in front of the frame for the 1-d cases (leg 22)
LOST_CASES = {
    'bit63': (1, 3, 130, (63,)),
    'bit64': (1, 3, 130, (64,)),
    'bits63_64': (1, 3, 130, (63, 64)),
    'word_edges': (1, 3, 130, (0, 63, 64, 127, 128, 129)),
    'all_of_word0': (1, 3, 130, tuple(range(64))),
    'every_second': (1, 3, 130, tuple(range(0, 130, 2))),
    'last': (1, 3, 130, (129,)),
    'idp3': (3, 3, 44, (0, 21, 22, 43)),
}
LOST_LEG = 22


# ---- the expected tail ------------------------------------------------------------------------------------------------------------------
def expected_tail(ops, tail=0):
    for op in ops:
        assert op in ('prefactor_rev', 'prefactor_fwd', 'gather', 'permute', 'anchors', 'augment', 'zupt'), op
        if op == 'prefactor_rev':
            tail = 15
        elif op in ('augment', 'zupt', 'prefactor_fwd'):
            tail = 0
    return tail


def check_tail(S, tail):
    """rows >= 15 exactly zero in the last `tail` columns"""
    if tail:
        assert S.shape[1] > tail
        bad = np.argwhere(S[15:, S.shape[1] - tail:] != 0.0)
        assert bad.size == 0, ('a non-zero entry where the tail is claimed zero', bad[:4].tolist())


def prefactor_reversed(n):
    """cov_prefactor's choice of form (capi_cov.inc): reversed from n = 31, claimed up to 14 tiles"""
    return n - 15 >= 16


PREFACTOR_N = (22, 30, 31, 64, 170, 224)
PREFACTOR_N_NONE = 225   # 15 tiles: no factor is claimed


# ---- the edits of one chain, on the host ----------------------------------------------------------------------------------------------
def edit_host(P, S, kind, leg, **a):
    """One index edit on (P, S): P through oracle/mirror_cov.py or mirror_features_lifecycle, S through the row map.  Returns
    (P', S' or None, map, op) -- op names the rule of expected_tail."""
    n = P.shape[0]
    if kind == 'augment':
        m, Pn, op = augment_map(n, a.get('rest', 0)), mc.augment(P, rest=a.get('rest', 0)), 'augment'
    elif kind == 'remove_clones':
        m, Pn, op = remove_clones_map(n, leg, a['clones']), mc.remove_clones(P, leg, a['clones']), 'gather'
    elif kind == 'clones_to_nuisance':
        m, Pn, op = nuisance_map(n, leg, a['clones']), mc.clones_to_nuisance(P, leg, a['clones']), 'permute'
    elif kind == 'remove_features':
        m, op = remove_features_map(n, leg, a['N'], a['d'], a['slots']), 'gather'
        Pn = mfl.rm_lost_features_cov(P, leg, a['N'], a['d'], a['slots'])
    else:
        raise ValueError(kind)
    return Pn, (None if S is None else np.ascontiguousarray(S[m])), m, op
