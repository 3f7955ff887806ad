"""Inputs and the reference chain of the armed prune update (orcvio_msckf_io_triangulate_prune): what pruneImuStateBuffer does to a tracked
feature that is not initialised yet (reference src/orcvio.cpp:2776-2793) inside the one-call frame.

A case is a window whose tracks end at the newest clone (the reference's if_tracked_now) cut three ways:
  first   the lost tracks (they do not reach the newest clone): the frame's first update, at their given positions
  tri     the tracked tracks seen in at least two of the clones that leave, IN FULL: the list of the arming
  prune   the same tracks restricted to the clones that leave: the rows of the prune update
The chain: the mirror's first update -> mirror_frame.prune_window's poses (incremented by its dx or not) -> check_motion on the list
without its last entry and triangulate on all of it (prune_tri below) -> the invalid tracks removed -> mirror_frame.step_frame with the
prune tracks at those positions.  Everything here runs on the numpy mirror alone; every reference is computed once (tri_io_cases.cached).
The conditions a case must meet (margins of every decision, the failure kinds of the set) are asserted where the reference is made."""
import dataclasses

import numpy as np

from orcvio_amd import synth
from oracle import mirror, mirror_frame, mirror_triangulate as mt
import tri_io_cases as tc
from tri_io_cases import KEEP, ALL, ALL_BUT_LAST, cached, select_tracks

ALL_MOTION_BUT_LAST = 3
MARGIN = 1e-3        # relative distance of every motion figure and every valid cost from its threshold
MAX_FIRST = 60       # lost tracks in the first update (a handle of the GPU tests holds 256 features)

WINDOWS = {
    'n20': dict(N=20, F=400, seed=3, track_len=(2, 20), outlier_frac=0.2),
    'n12': dict(N=12, F=120, seed=17, track_len=(2, 12), outlier_frac=0.2),
    'n6': dict(N=6, F=64, seed=4, track_len=(2, 6), outlier_frac=0.2),
}


def remove_sets(N):
    return {'oldest': [0, 1], 'newest': [N - 3, N - 2], 'split': [0, N - 2]}


# (window, flag set, remove set, prune_apply_dx): the n12 window through the whole grid, the two others at the reference's shipped
# operating point (euroc, the increment applied) through the three remove sets, and the slowed-down copy with its no-motion tracks
CASES = [('n12', fs, rm, ap) for fs in tc.FLAG_SETS for rm in ('oldest', 'newest', 'split') for ap in (0, 1)] + \
        [(wn, 'euroc', rm, 1) for wn in ('n20', 'n6') for rm in ('oldest', 'newest', 'split')] + \
        [('n12_slow', 'euroc', 'newest', 1)]


def case_id(c):
    return '-'.join(str(x) for x in c)


def _project(w):
    """obs_z of every listed observation from p_w and the window's poses, noise-free."""
    z = np.zeros_like(w.obs_z)
    for j in range(w.F):
        for o in range(int(w.obs_ptr[j]), int(w.obs_ptr[j + 1])):
            c = int(w.obs_clone[o])
            R, t = mt.cam_pose(w.R_b2w[c], w.t_b_w[c], w.R_b2c[c], w.t_c_b[c])
            p = R.T @ (w.p_w[j] - t)
            z[o] = p[:2] / p[2]
    return z


def _slowed(w, s):
    """The window with its clones' translations shrunk towards the newest clone by s (slow motion), re-observed with a quarter of the
    filter's measurement noise (without any, dx and gamma of the reference are rounding noise and compare with nothing)."""
    t = w.t_b_w[-1] + s * (w.t_b_w - w.t_b_w[-1])
    out = dataclasses.replace(w, t_b_w=np.ascontiguousarray(t), t_fej=np.ascontiguousarray(t.copy()))
    noise = 0.25 * w.flags.noise_feature * np.random.default_rng(7).standard_normal(w.obs_z.shape)
    return dataclasses.replace(out, obs_z=np.ascontiguousarray(_project(out) + noise))


def window(name, flag_set):
    def make():
        fl, sigma_px = tc.FLAG_SETS[flag_set]
        base = name.split('_')[0]
        w = synth.make_window(flags=synth.Flags(**fl), sigma_px=sigma_px, **WINDOWS[base])
        if name.endswith('_slow'):   # shrunk until the mirror finds a track without motion (and still triangulates most)
            for s in (0.7, 0.6, 0.5, 0.4, 0.35, 0.3, 0.25):
                ws = _slowed(w, s)
                # (the newest clones leave: tracks of every length, the short ones stop moving first; on the poses the chain uses)
                tri = chain(ws, remove_sets(ws.N)['newest'], 1)['tri']
                if (tri['flags'] == mt.FLAG_NO_MOTION).any():
                    return ws
            raise AssertionError('no shrink factor gives a track without motion')
        return w
    return cached(('ptw', name, flag_set), make)


def split(w, remove):
    """dict(first, tri, prune, sel): the three cuts of a window (above); sel = the mask of the prune features over w's tracks."""
    tracked = tc.ends_at_newest(w)
    sub = synth.subset_tracks(w, remove, min_obs=2)
    sel = tracked & (np.diff(sub.obs_ptr) >= 2)
    lost = ~tracked & (np.diff(w.obs_ptr) >= 2)
    lost &= np.cumsum(lost) <= MAX_FIRST
    return dict(first=select_tracks(w, lost), tri=select_tracks(w, sel), prune=select_tracks(sub, sel), sel=sel)


def prune_tri(tri_win, mode=None, cfg=None, motion_last=-2, drop_last=False, p_w=None):
    """The mirror's form of mode ORCVIO_TRI_ALL_MOTION_BUT_LAST over a window listing every observation: check_motion on the list
    without its last entry, triangulate on all of it.  mode: per track (KEEP / ALL / ALL_BUT_LAST / ALL_MOTION_BUT_LAST); tracks of the
    other modes go through tri_io_cases.mirror_tri.  motion_last / drop_last: the mutations of tests/test_prune_tri_cases.py.
    Returns mirror_tri's dict plus motion [F]."""
    cfg = cfg or mt.OptimizationConfig()
    w = tri_win
    F = w.F
    mode = np.full(F, ALL_MOTION_BUT_LAST, np.int32) if mode is None else np.asarray(mode, np.int32)
    other = mode != ALL_MOTION_BUT_LAST
    out = tc.mirror_tri(w if p_w is None else dataclasses.replace(w, p_w=p_w), np.where(other, mode, ALL), cfg)
    out['motion'] = np.asarray(out.get('motion', np.full(F, np.nan)), dtype=np.float64).copy()
    pose = [mt.cam_pose(w.R_b2w[i], w.t_b_w[i], w.R_b2c[i], w.t_c_b[i]) for i in range(w.N)]
    for j in np.flatnonzero(~other):
        lo, hi = int(w.obs_ptr[j]), int(w.obs_ptr[j + 1])
        for k in ('p_w', 'solution', 'cost'):
            out[k][j] = np.nan
        out['valid'][j] = 0; out['flags'][j] = mt.FLAG_NO_MOTION; out['motion'][j] = np.nan
        if hi - lo < 2:
            continue
        Rs = [pose[c][0] for c in w.obs_clone[lo:hi]]
        ts = [pose[c][1] for c in w.obs_clone[lo:hi]]
        zs = [w.obs_z[o] for o in range(lo, hi)]
        end = len(Rs) + motion_last + 1   # (the listed observations the motion check sees: all but the last)
        mo = mt.check_motion(Rs[:end], ts[:end], zs[0])
        out['motion'][j] = mo
        if not (mo > cfg.translation_threshold):
            continue
        if drop_last:
            Rs, ts, zs = Rs[:-1], ts[:-1], zs[:-1]
        r = mt.triangulate(Rs, ts, zs, cfg)
        out['valid'][j] = 1 if r['valid'] else 0
        out['p_w'][j] = r['p_w']; out['solution'][j] = r['solution']; out['flags'][j] = r['flags']; out['cost'][j] = r['cost']
    return out


def chain(w, remove, apply_dx, mode=None, cfg=None, first_tri=False, increment=True, sp=None, **mut):
    """The reference chain on one window.  first_tri: the first update triangulates its own tracks too (both armings); sp: the three
    cuts, when they are not split()'s.  increment=False
    and **mut: mutations.  Returns dict(sp, first_tri, tri, keep, ref, win2, kept)."""
    sp = split(w, remove) if sp is None else sp
    table = mirror.chi2_table(w.flags.chi2_prob)
    first, t1 = sp['first'], None
    if first_tri:
        t1 = tc.mirror_tri(first)
        first = tc.kept_window(first, t1)
    head = mirror_frame.step_frame(w.P, dict(w=first), 1, apply_dx, augment=False, table=table)
    win2, applied = mirror_frame.prune_window(sp['tri'], head['dx'], w.flags, apply_dx and increment)
    tri = prune_tri(win2, mode, cfg, p_w=sp['prune'].p_w, **mut)
    keep = tri['valid'] == 1
    kept = select_tracks(sp['prune'], keep, tri['p_w']) if keep.any() else None
    ref = mirror_frame.step_frame(w.P, dict(w=first, prune=kept, remove=remove), 1, apply_dx, augment=False, table=table)
    return dict(sp=sp, first_tri=t1, tri=tri, keep=keep, ref=ref, win2=win2, kept=kept, head=head, first=first)


def check_conditions(ch, cfg=None):
    """The conditions of a case, on the mirror's figures alone: every decision of the chain has a margin."""
    cfg = cfg or mt.OptimizationConfig()
    tri, keep = ch['tri'], ch['keep']
    mo = tri['motion'][np.isfinite(tri['motion'])]
    assert (np.abs(mo - cfg.translation_threshold) >= MARGIN * cfg.translation_threshold).all(), 'a motion figure at the threshold'
    cost = tri['cost'][keep] / (2.0 * np.diff(ch['sp']['tri'].obs_ptr)[keep] ** 2)
    assert (np.abs(cost - cfg.cost_threshold) >= MARGIN * cfg.cost_threshold).all(), 'a valid cost at the threshold'
    assert 2 * keep.sum() >= len(keep) > 0, 'fewer than half the tracks are valid'
    if ch['kept'] is not None:
        w = ch['sp']['prune']
        assert tc.gate_margin(ch['kept'], ch['ref']['prune_gamma'], ch['ref']['prune_accept'], w.flags.chi2_prob) >= 1e-6, 'a gamma at its threshold'


def reference(case):
    """The chain of a case of CASES, its conditions checked; computed once."""
    def make():
        wn, fs, rm, ap = case
        w = window(wn, fs)
        ch = chain(w, remove_sets(w.N)[rm], ap)
        check_conditions(ch)
        return ch
    return cached(('ptref', case), make)


def failure_kinds():
    """The flag bits that occur among the failing tracks of the whole set."""
    bits = 0
    for c in CASES:
        r = reference(c)
        for f in r['tri']['flags'][~r['keep']]:
            bits |= int(f)
    return bits
