"""TEST INFRASTRUCTURE ONLY -- the OBJECT rows (ObjectResJacCam / ObjectLM functors, constructObjectResidualJacobians: oracle/mirror_objects.py)
and the per-object projection at the shapes where object_rows_lane, k_obj_fused and the three-launch pipeline (k_object_rows_batch,
k_obj_front, border / solve / refine) take another branch: explicit cases (no randomised discovery) and a reference in extended
precision (np.longdouble, 64-bit mantissa) that is compared BLOCK BY BLOCK.

Rows of one object, in the order of construct_object_residual_jacobians (per in-window frame: the rows of its detected keypoints in
keypoint order, then the four bbox rows), split into
    res_kp, res_bbox                 the residual on keypoint rows / bbox rows
    Hx6_rot, Hx6_pos                 the three rotation / three position columns of J_cam D
    Hf_pose                          columns 0:6 of every row
    Hf_shape                         columns 6:9 of the bbox rows
    Hf_kp                            columns 9 + 3 kpid : 12 + 3 kpid of the rows of keypoint kpid
and everything else of H_f is a structural zero: exactly 0.

Projection of one object: G_o = X^T (I - Q_f Q_f^T) X with X = [H_x | r] over the active columns (15 .. n, then r): (NA + 1)^2,
independent of anybody's basis of range(H_f) and of its signs.  Blocks: the 6 x 6 tile of every pair of clones the object is seen
from, the r column of every such clone, r^T r; everything else (clones that do not see the object, the columns in front of the
clones) is exactly 0.

Error of a block: max|got - ref| / max|ref| over that block (entering_cases.block_err).

Used by tests/test_object_cases.py (CPU: coverage, conditioning, the float64 restatement against this reference) and
tests/test_gpu_object_blocks.py (the kernels against it)."""
import dataclasses
import functools

import numpy as np

from orcvio_amd import synth
from oracle import mirror_objects as mo
from entering_cases import block_err, LD   # noqa: F401  (block_err is the precedent's, unchanged)

# ---- tolerances ------------------------------------------------------------------------------------------------------------------
# Worst error of the float64 restatement (mirror_objects rows; numpy Householder QR of H_f, G = (Q_2^T X)^T (Q_2^T X)) against the
# extended reference over ALL cases and objects below, per block class (tests/test_object_cases.py measures and prints them; x86-64,
# 80-bit long double).  The device's bounds are 100 x these, the margin of tests/entering_cases.py: it covers another summation
# order, FMA contraction and the device's route to G_o (B - Y^T Y, a cancelling difference, where numpy's route sums squares).
# Never derived from what the device returns.
# These are 1e-12, not 1e-15, because of the DATA: the camera extrinsics of synth (EuRoC's, printed to a few decimals) are
# orthonormal to 5.7e-13 only, and so is every camera pose made with them.  The mirror inverts a pose with np.linalg.inv, the
# reference (and the device, and Eigen's Isometry3d::inverse) with the closed form [R^T | -R^T t]: the two differ by that much, and
# the projection amplifies it by |X^T X| / |G_o|.  A wrong column, mask or rank moves a block by 1e-2 or more of its scale.
# Rows: by block class (res_kp is a difference of O(1) projections, 1e-3 .. 1e-2 of them).  Projection: by perturbation side of the
# object state and block class.
ROW_WORST = dict(res_kp=2.8e-11, res_bbox=3.9e-12, Hx6_rot=1.1e-12, Hx6_pos=1.3e-12, Hf_pose=1.1e-12, Hf_shape=1.2e-12, Hf_kp=6.9e-13)
GRAM_WORST = dict(left=dict(tile=1.2e-11, r=1.3e-10, rr=3.8e-12), right=dict(tile=8.6e-12, r=2.8e-11, rr=3.3e-12))
ROW_TOL = {q: 100 * v for q, v in ROW_WORST.items()}
GRAM_TOL = {s: {q: 100 * v for q, v in d.items()} for s, d in GRAM_WORST.items()}
COND_CAP = 1e5   # cond(H_f) of every object below (measured: see tests/test_object_cases.py's print)

FLAGSETS = {'L': (1, 0, 0), 'R': (0, 0, 0), 'Rn': (0, 1, 1), 'Lc': (1, 2, 0)}   # (obj_left, new_bbox, vio_left)
WINDOWS = {'small': dict(leg=22, N=12, seed=31), 'leg46': dict(leg=46, N=12, seed=32), 'maxf': dict(leg=22, N=34, seed=33)}
KS = (0, 1, 3, 4, 5, 12, 13, 16, 17, 29, 34)
OBJ_FUSED_MAXF, OBJ_FUSED_MAXK = 32, 16   # object_fused.hpp: OBJ_FUSED_MAXF, OBJ_FUSED_NW * OBJ_FUSED_KPW
SIGMA_KP = 0.004
# Which draw of synth.make_objects a case takes (1000 x this is added to its seed).  A left-perturbation car far from the camera, or
# one seen in three frames only, has cond(H_f) of 1e5 .. 8e5 (the gauge between its pose and its keypoints); these draws keep every
# object below 5e4, inside COND_CAP with room for another BLAS.  Fixed numbers: a case is the same object in every run.
DRAW = {(4, 12): 1, (5, 12): 2, (13, 12): 2, (16, 12): 2, (13, 3): 3, 'multi': 19}


def lpf_of(K):
    """Lanes per frame of k_obj_fused's P1: the smallest power of two >= K + 4."""
    return 4 << max(0, int(np.ceil(np.log2((K + 4) / 4.0))))


@dataclasses.dataclass(frozen=True)
class CaseId:
    K: object              # keypoints: an int, or a tuple (one entry per object of the update)
    fl: str = 'L'
    win: str = 'small'
    frames: int = 12       # listed frames per object
    pat: str = ''          # '', nokp, first, last, outside, desc, odd, f32, f33, shared
    fix_D: bool = False

    def __str__(self):
        k = 'K' + ('x'.join(str(q) for q in self.K) if isinstance(self.K, tuple) else str(self.K))
        return '_'.join([self.win, k, self.fl, 'f%d' % self.frames] + ([self.pat] if self.pat else []) + (['fixD'] if self.fix_D else []))


PATTERNS = ('nokp', 'first', 'last', 'outside', 'desc', 'odd')
MULTI5 = CaseId((0, 3, 12, 13, 16), pat='odd', frames=5)
MULTI6 = CaseId((0, 3, 12, 13, 16, 17), pat='odd', frames=5)
CASES = ([CaseId(K, 'L', frames=12) for K in KS] + [CaseId(K, 'Rn', frames=5) for K in KS] +
         [CaseId(K, fl, frames=12) for K in (4, 13) for fl in ('R', 'Lc')] +
         [CaseId(4, 'L', frames=12, fix_D=True)] +
         [CaseId(K, 'L', frames=12, pat=p) for K in (4, 13) for p in PATTERNS if p != 'odd'] +
         [CaseId(4, 'L', frames=5, pat='odd'), CaseId(13, 'L', frames=3, pat='odd')] +
         [CaseId(12, 'Rn', win='leg46', frames=12), CaseId(13, 'L', win='leg46', frames=5)] +
         [CaseId(4, 'L', win='maxf', frames=34, pat='f32'), CaseId(4, 'L', win='maxf', frames=34, pat='f33'),
          CaseId(4, 'L', win='maxf', frames=12, pat='shared')] +
         [MULTI5, MULTI6])
IDS = [str(c) for c in CASES]


@dataclasses.dataclass
class Case:
    cid: CaseId
    win: object
    objs: list            # synth.ObjectTrack
    obj_left: int
    new_bbox: int
    vio_left: int
    fix_D: bool

    @property
    def flags3(self):
        return (self.obj_left, self.new_bbox, self.vio_left)

    @property
    def fused(self):
        """Does the library send this update to k_obj_fused (capi_objects.inc obj_fused_eligible: every object with at most 16 keypoints,
        at most 32 in-window frames, all on distinct clones; the rows of these cases are far inside the LDS staging)?"""
        for ob in self.objs:
            cl = [fr['clone'] for fr in ob.frames if fr['clone'] >= 0]
            if len(ob.kps) > OBJ_FUSED_MAXK or len(cl) > OBJ_FUSED_MAXF or len(set(cl)) != len(cl):
                return False
        return True


def _set_keypoints(ob, K, rng):
    """Trim to K keypoints, or extend: extra keypoints inside the ellipsoid, observed at the estimate's own projection plus noise."""
    if K <= len(ob.kps):
        ob.kps = ob.kps[:K].copy()
        for fr in ob.frames:
            fr['zs'] = fr['zs'][:K].copy()
        return
    extra = rng.uniform(-0.55, 0.55, (K - len(ob.kps), 3)) * ob.shape
    ob.kps = np.vstack([ob.kps, extra])
    for fr in ob.frames:
        X = (np.linalg.inv(fr['wTc']) @ ob.wTo @ np.hstack([extra, np.ones((len(extra), 1))]).T).T
        fr['zs'] = np.vstack([fr['zs'], X[:, :2] / X[:, 2:3] + SIGMA_KP * rng.standard_normal((len(extra), 2))])


def _apply_pattern(ob, K, pat):
    """The missing keypoints and the frame list of one object.  Without a pattern (and for desc / odd / the maxf cases) frame f of the
    list misses keypoint (7 f + 1) mod K when K >= 3: every frame another rank shift, every keypoint seen in all frames but a few."""
    F = len(ob.frames)
    if pat in ('', 'desc', 'odd', 'f32', 'f33', 'shared', 'outside') and K >= 3:
        for f, fr in enumerate(ob.frames):
            fr['zs'][(7 * f + 1) % K] = np.nan
    if pat == 'nokp':
        ob.frames[2]['zs'][:] = np.nan
        ob.frames[7]['zs'][1 % max(K, 1)] = np.nan
    elif pat == 'first':
        for f in (1, 4, 7):
            ob.frames[f]['zs'][0] = np.nan
    elif pat == 'last':
        for f in (0, 5, F - 1):
            ob.frames[f]['zs'][K - 1] = np.nan
    elif pat == 'outside':
        for f in (0, F // 2, F - 1):
            ob.frames[f]['clone'] = -1
    elif pat == 'desc':
        ob.frames = ob.frames[::-1]
    elif pat == 'f32':
        for f in (3, 20):
            ob.frames[f]['clone'] = -1
    elif pat == 'f33':
        ob.frames[20]['clone'] = -1
    elif pat == 'shared':
        ob.frames[5]['clone'] = ob.frames[4]['clone']   # two frames on one clone (each keeps its own camera pose)


@functools.lru_cache(maxsize=None)
def make_case(cid: CaseId) -> Case:
    w = WINDOWS[cid.win]
    obj_left, new_bbox, vio_left = FLAGSETS[cid.fl]
    flags = synth.Flags(use_larvio=0, use_left_perturbation=vio_left, leg_dim=w['leg'])
    win = synth.make_window(N=w['N'], F=4, seed=w['seed'], flags=flags, track_len=4)
    Ks = cid.K if isinstance(cid.K, tuple) else (cid.K,)
    seed = 1000 * DRAW.get('multi' if len(Ks) > 1 else (Ks[0], cid.frames), 0) + (500 if len(Ks) > 1 else 100 + 7 * Ks[0] + cid.frames)
    # (the objects of `multi` are the same in both lists: one seed, and make_objects draws object after object)
    objs = synth.make_objects(win, n_objects=len(Ks), seed=seed, sigma_kp=SIGMA_KP, missing_frac=0.0,
                              frames_per_object=None if cid.frames >= w['N'] else cid.frames)
    rng = np.random.default_rng(9000 + seed)
    for i, (ob, K) in enumerate(zip(objs, Ks)):
        if cid.pat == 'odd' and len(Ks) > 1 and lpf_of(K) >= 16:
            ob.frames = ob.frames[:3]           # lpf 16: four frames per wavefront, lpf 32: two -- three leave a lane group idle
        _set_keypoints(ob, K, rng)
        _apply_pattern(ob, K, cid.pat)
    return Case(cid, win, objs, obj_left, new_bbox, vio_left, cid.fix_D)


# ---- the layout of an object's rows ---------------------------------------------------------------------------------------------------
def row_layout(ob):
    """[(frame index in the list, clone, kpid or -1 - j for bbox line j)] of the rows, in output order."""
    out = []
    for f, fr in enumerate(ob.frames):
        if fr['clone'] < 0:
            continue
        zs = np.asarray(fr['zs']).reshape(-1, 2)
        for k in range(len(zs)):
            if np.all(np.isfinite(zs[k])):
                out += [(f, fr['clone'], k), (f, fr['clone'], k)]
        out += [(f, fr['clone'], -1 - j) for j in range(4)]
    return out


def row_blocks(ob, Hx6, Hf, res):
    """dict of the blocks above of the rows [m] of one object, and the structural zeros as one array (must be all 0)."""
    lay = row_layout(ob)
    assert len(lay) == len(res) == Hf.shape[0] == Hx6.shape[0], (len(lay), Hf.shape, Hx6.shape, len(res))
    kp = np.array([q[2] for q in lay])
    isk = kp >= 0
    out = dict(res_bbox=res[~isk], Hx6_rot=Hx6[:, :3], Hx6_pos=Hx6[:, 3:], Hf_pose=Hf[:, :6], Hf_shape=Hf[~isk][:, 6:9])
    mask = np.ones(Hf.shape, dtype=bool)
    mask[:, :6] = False
    mask[np.ix_(~isk, np.arange(Hf.shape[1]) < 9)] = False
    if isk.any():
        rows = np.nonzero(isk)[0]
        cols = 9 + 3 * kp[rows][:, None] + np.arange(3)[None, :]
        out.update(res_kp=res[isk], Hf_kp=Hf[rows[:, None], cols])
        mask[rows[:, None], cols] = False
    return out, Hf[mask]


# ---- float64: the mirror (the DATA of the projection's reference, and the restatement that is measured) ------------------------------
def mirror_rows(case, ob):
    """(Hx [m, n], Hf [m, 9 + 3K], res [m], row_clone [m], Hx6 [m, 6]) of one object through oracle/mirror_objects.py."""
    win = case.win
    res, Hf, Jc, counts = mo.object_rows(ob.wTo, ob.shape, ob.kps, ob.frames, case.obj_left, case.new_bbox)
    return mo.construct_object_residual_jacobians(Jc, [fr['clone'] for fr in ob.frames], Hf, res, counts, [fr['wTc'] for fr in ob.frames],
                                                  win.R_b2c[0], win.t_c_b[0], case.vio_left, win.flags.leg_dim, win.N, fix_D_identity=case.fix_D)


def active_X(win, Hx6, row_clone, res):
    """X = [H_x(:, 15:) | r] from the six window columns of every row."""
    NA = win.flags.leg_dim + 6 * win.N - 15
    cb0 = win.flags.leg_dim - 15
    X = np.zeros((len(res), NA + 1), dtype=np.asarray(Hx6).dtype)
    for q, c in enumerate(row_clone):
        X[q, cb0 + 6 * c: cb0 + 6 * c + 6] = Hx6[q]
    X[:, NA] = res
    return X


def gram_float64(win, Hx6, Hf, res, row_clone):
    """The float64 restatement of the projection: numpy's Householder QR of H_f, the columns of Q behind the first ncol as the basis of the
    left null space (the route of helpers.objects_update_reference with another factorisation), G = (Q_2^T X)^T (Q_2^T X)."""
    X = active_X(win, Hx6, row_clone, res)
    Q, _ = np.linalg.qr(Hf, mode='complete')
    H1 = Q[:, Hf.shape[1]:].T @ X
    return H1.T @ H1


def gram_blocks(win, ob, G):
    """dict((kind, ...) -> block) of an (NA + 1)^2 (or larger, padded) projected Gram, and everything else as one array (must be all 0)."""
    NA = win.flags.leg_dim + 6 * win.N - 15
    cb0 = win.flags.leg_dim - 15
    G = np.asarray(G)[:NA + 1, :NA + 1]
    seen = sorted({fr['clone'] for fr in ob.frames if fr['clone'] >= 0})
    out = {}
    mask = np.ones(G.shape, dtype=bool)
    for a in seen:
        sa = slice(cb0 + 6 * a, cb0 + 6 * a + 6)
        for b in seen:
            sb = slice(cb0 + 6 * b, cb0 + 6 * b + 6)
            out[('tile', a, b)] = G[sa, sb]
            mask[sa, sb] = False
        out[('r', a)] = G[sa, NA]
        out[('rT', a)] = G[NA, sa]
        mask[sa, NA] = False
        mask[NA, sa] = False
    out[('rr',)] = G[NA:NA + 1, NA]
    mask[NA, NA] = False
    return out, G[mask]


def gram_class(key):
    return {'tile': 'tile', 'r': 'r', 'rT': 'r', 'rr': 'rr'}[key[0]]


# ---- extended precision ------------------------------------------------------------------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _skew(w):
    z = LD(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=LD)


def _odot(x4):
    T = np.zeros((4, 6), dtype=LD)
    T[:3, 3:] = -_skew(x4[:3])
    T[0, 0] = T[1, 1] = T[2, 2] = x4[3]
    return T


def _circ(x4):
    T = np.zeros((6, 4), dtype=LD)
    T[3:6, 0:3] = -_skew(x4[:3])
    T[0:3, 3] = x4[:3]
    return T


def _rigid_inverse(T):
    """Closed form (np.linalg.inv is float64 only): [R^T | -R^T t]."""
    out = np.eye(4, dtype=LD)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def _norm(v):
    return np.sqrt(v @ v)


def _keypoint_rows_ext(cTw, wTo, kp, z, left):
    """mirror_objects.keypoint_rows for one detected keypoint: (res [2], J_cam [2, 6], Hf_pose [2, 6], Hf_kp [2, 3])."""
    P = cTw[:3, :]
    X = np.append(kp, LD(1))
    Xw = wTo @ X
    Mc = P @ Xw
    zc = Mc[2]
    dpi = np.array([[1 / zc, LD(0), -Mc[0] / (zc * zc)], [LD(0), 1 / zc, -Mc[1] / (zc * zc)]], dtype=LD)
    res = Mc[:2] / zc - z
    if left:
        Jc = -(dpi @ P @ _odot(Xw))
        Hp = dpi @ P @ _odot(Xw)
    else:
        Jc = -(dpi @ _odot(cTw @ Xw)[:3, :])
        Hp = dpi @ P @ wTo @ _odot(X)
    return res, Jc, Hp, dpi @ P @ wTo[:, :3]


def _bbox_rows_ext(cTw, wTo, shape, bbox, left, new_residual):
    """mirror_objects.bbox_rows: (res [4], J_cam [4, 6], Hf_pose [4, 6], Hf_shape [4, 3])."""
    one, zero = LD(1), LD(0)
    Qi = np.diag(np.array([shape[0] ** 2, shape[1] ** 2, shape[2] ** 2, -one], dtype=LD))
    pts = np.array([[bbox[0], bbox[1]], [bbox[2], bbox[1]], [bbox[2], bbox[3]], [bbox[0], bbox[3]]], dtype=LD)
    P_res = (cTw @ wTo)[:3, :]
    P = cTw[:3, :]
    P_prime = np.eye(4, dtype=LD)[:3, :]
    wTc_invT = cTw.T
    U2 = Qi[:3, :3]
    res = np.zeros(4, dtype=LD); Jc = np.zeros((4, 6), dtype=LD); Hp = np.zeros((4, 6), dtype=LD); Hs = np.zeros((4, 3), dtype=LD)
    for i in range(4):
        a = np.array([pts[i, 0], pts[i, 1], one], dtype=LD)
        b_ = np.array([pts[(i + 1) % 4, 0], pts[(i + 1) % 4, 1], one], dtype=LD)
        li = np.array([a[1] * b_[2] - a[2] * b_[1], a[2] * b_[0] - a[0] * b_[2], a[0] * b_[1] - a[1] * b_[0]], dtype=LD)
        if not new_residual:
            res[i] = li @ (P_res @ Qi @ P_res.T) @ li
        else:
            ub = P_res.T @ li
            b = ub[:3]
            sign = one if ub[3] > 0 else -one
            res[i] = (ub[3] - sign * np.sqrt(b @ U2 @ b)) / _norm(b)
        yyw = li @ P
        yyw_prime = li @ P_prime
        yyo = yyw @ wTo
        if not new_residual:
            if left:
                p = 2 * yyo @ Qi @ wTo.T @ _circ(yyw).T
                Jc[i] = -p
                Hp[i] = p
            else:
                Jc[i] = -2 * yyo @ Qi @ wTo.T @ wTc_invT @ _circ(yyw_prime).T
                Hp[i] = 2 * yyo @ Qi @ _circ(wTo.T @ yyw).T
            Hs[i] = 2 * shape * (yyo[:3] ** 2)
        else:
            corrected = int(new_residual) == 2
            ub = P_res.T @ li if corrected else P.T @ li
            b = ub[:3]
            bn = _norm(b)
            if left:
                dO = wTo.T @ _circ(yyw).T
                dC = dO
            else:
                dO = _circ(wTo.T @ yyw).T
                dC = wTo.T @ wTc_invT @ _circ(yyw_prime).T
            term1a = np.array([zero, zero, zero, one], dtype=LD)
            term2a = Qi.copy()
            term2a[3, 3] = zero
            sign = one if ub[3] > 0 else -one
            sq = np.sqrt(b @ U2 @ b)
            p_be_p_ua = term1a - sign * (ub @ term2a) / sq
            term2b = np.eye(4, dtype=LD)
            term2b[3, 3] = zero
            p_ua_ub = np.eye(4, dtype=LD) / bn - np.outer(ub, ub) @ term2b / bn ** 3
            Jc[i] = -(p_be_p_ua @ p_ua_ub @ dC)
            Hp[i] = p_be_p_ua @ p_ua_ub @ dO
            Hs[i] = shape * b * b / (bn * sq) * (-sign if corrected else one)
    return res, Jc, Hp, Hs


def rows_ext(case, ob):
    """(Hx6 [m, 6], Hf [m, 9 + 3K], res [m], row_clone [m]) of one object in extended precision, in the order of
    construct_object_residual_jacobians.  exp(log(wTc)) of the mirror is the identity here and inverses are closed forms."""
    win = case.win
    wTo, shape, kps = _ld(ob.wTo), _ld(ob.shape), _ld(np.asarray(ob.kps).reshape(-1, 3))
    Rbc, tcb = _ld(win.R_b2c[0]), _ld(win.t_c_b[0])
    K = len(kps)
    ncol = 9 + 3 * K
    Hx6, Hf, res, rc = [], [], [], []
    for fr in ob.frames:
        if fr['clone'] < 0:
            continue
        wTc = _ld(fr['wTc'])
        cTw = _rigid_inverse(wTc)
        D = np.zeros((6, 6), dtype=LD)
        if case.fix_D:
            D = np.eye(6, dtype=LD)
        elif case.vio_left:
            D[0:3, 0:3] = _skew(wTc[:3, :3] @ (-(Rbc @ tcb)) + wTc[:3, 3])
            D[3:6, 0:3] = np.eye(3, dtype=LD)
            D[0:3, 3:6] = np.eye(3, dtype=LD)
        else:
            D[0:3, 0:3] = -(Rbc @ _skew(tcb))
            D[3:6, 0:3] = Rbc
            D[0:3, 3:6] = cTw[:3, :3]
        zs = np.asarray(fr['zs'], dtype=np.float64).reshape(-1, 2)
        for k in range(K):
            if not np.all(np.isfinite(zs[k])):
                continue
            r, Jc, Hp, Hk = _keypoint_rows_ext(cTw, wTo, kps[k], _ld(zs[k]), case.obj_left)
            h = np.zeros((2, ncol), dtype=LD)
            h[:, 0:6] = Hp
            h[:, 9 + 3 * k: 12 + 3 * k] = Hk
            Hx6.append(Jc @ D); Hf.append(h); res.append(r); rc += [fr['clone']] * 2
        r, Jc, Hp, Hs = _bbox_rows_ext(cTw, wTo, shape, _ld(fr['bbox']), case.obj_left, case.new_bbox)
        h = np.zeros((4, ncol), dtype=LD)
        h[:, 0:6] = Hp
        h[:, 6:9] = Hs
        Hx6.append(Jc @ D); Hf.append(h); res.append(r); rc += [fr['clone']] * 4
    return np.vstack(Hx6), np.vstack(Hf), np.concatenate(res), np.array(rc, dtype=np.int32)


def gram_ext(win, Hx6, Hf, res, row_clone):
    """G_o in extended precision from rows in float64 or extended precision: an orthonormal basis of range(H_f) by Gram-Schmidt with
    re-orthogonalisation (twice is enough), X projected off it twice, G = X_perp^T X_perp."""
    X = active_X(win, np.asarray(Hx6, dtype=LD), row_clone, np.asarray(res, dtype=LD))
    A = np.asarray(Hf, dtype=LD)
    m, nc = A.shape
    Q = np.zeros((m, nc), dtype=LD)
    for j in range(nc):
        v = A[:, j].copy()
        n0 = _norm(v)
        for _ in range(3):
            v = v - Q[:, :j] @ (Q[:, :j].T @ v)
        nv = _norm(v)
        assert nv > 1e-9 * n0, ('H_f is rank deficient at column', j)
        Q[:, j] = v / nv
    for _ in range(2):
        X = X - Q @ (Q.T @ X)
    return X.T @ X


@functools.lru_cache(maxsize=None)
def reference(cid: CaseId):
    """Per object of the case: dict(rows=(Hx6, Hf, res, row_clone) in extended precision, mirror=(Hx6, Hf, res, row_clone) float64,
    G = G_o in extended precision from the extended rows: the exact quantity of the case's data).  Computed once and shared; nobody
    writes to it."""
    case = make_case(cid)
    out = []
    for ob in case.objs:
        Hx, Hf, r, rc, hx6 = mirror_rows(case, ob)
        ext = rows_ext(case, ob)
        out.append(dict(rows=ext, mirror=(hx6, Hf, r, rc), G=gram_ext(case.win, *ext)))
    return out


def bbox_plane_signs(ob):
    """The signs of yyo[3] (the plane's offset in the object frame: the branch of the new bbox residual and of its Jacobians) that
    occur among the bbox rows of the in-window frames."""
    signs = set()
    for fr in ob.frames:
        if fr['clone'] < 0:
            continue
        cTw = np.linalg.inv(fr['wTc'])
        for li in mo.poly2lineh(mo.bbox2poly(fr['bbox'])):
            signs.add(1 if (li @ cTw[:3, :] @ ob.wTo)[3] > 0 else -1)
    return signs
