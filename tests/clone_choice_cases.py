"""Cases of the check of the clones that leave (orcvio_msckf_io_choose_clones): a window, the lost tracks of its first update, the IMU's
extrinsic, the camera records from before the update, and thresholds PLACED so that the verdict the case asks for comes out.

The placement: the angles and distances of the three clones the loop can compare with the key (N-3, N-2, N-5) are evaluated on the
pre-update records and on the records the mirror's first update leaves (oracle/mirror_frame.py's dx).  A threshold candidate is the
midpoint between two neighbouring values of that list -- in particular between a quantity's pre-update and its post-update value, which
is where a DISAGREEING case has to sit: the prediction (on the pre-update records) takes one side, the device (post-update) the other --
or a value far below / above all of them.  Among the candidates that give the asked pattern of taken / not taken on the post-update
records AND the asked agreement, the one with the largest margin is taken.  A case whose best margin is below MARGIN is rebuilt with a
wider prior (a larger dx) and, where the window's own geometry rules the pattern out at every prior (at N = 6 the clone N-5 sits as
close to the key as N-3 does), on the next draw of the window -- never dropped: case() asserts, it does not skip.  Everything here is numpy; every case is computed once."""
import dataclasses

import numpy as np

from orcvio_amd import synth
from oracle import mirror, mirror_frame
import mirror_clone_choice as mc
import tri_io_cases as tc
from tri_io_cases import cached, select_tracks

MARGIN = 1e-6          # x max(1, |threshold|): distance of every compared quantity from its threshold, on both sets of records
MAX_FIRST, MAX_PRUNE = 40, 20
PRIOR_SCALES = (1.0, 4.0, 16.0, 64.0)
DRAWS = (0, 1, 2, 3, 4, 5)   # added to the window's seed

# the mirror's largest distance from the 60-digit evaluation over the case set (relative; tests/test_clone_choice_mirror.py measures it
# and holds these within a factor of two); the GPU test's bar is ten times each
ANGLE_SPREAD = 1.0e-15
DISTANCE_SPREAD = 1.9e-15

EUROC = dict(use_larvio=1)
RIGHT = dict(use_larvio=0, use_left_perturbation=0)
LEFT = dict(use_larvio=0, use_left_perturbation=1)
WINDOWS = {6: dict(F=64, seed=4), 7: dict(F=80, seed=11), 20: dict(F=300, seed=3)}
PATTERNS = {'11': (1, 1), '10': (1, 0), '01': (0, 1), '00': (0, 0)}


def _spec(N, pat, agree, flags=EUROC, leg=22, extrin=False, tracking_ok=1):
    return dict(N=N, pattern=PATTERNS[pat], agree=agree, flags=flags, leg=leg, extrin=extrin, tracking_ok=tracking_ok)


SPECS = {}
for _N in (6, 7, 20):
    for _p in PATTERNS:
        for _a in (True, False):
            SPECS['n%d_%s_%s' % (_N, _p, 'agree' if _a else 'differ')] = _spec(_N, _p, _a)
SPECS.update({
    'right_10_differ': _spec(7, '10', False, RIGHT), 'right_01_agree': _spec(7, '01', True, RIGHT),
    'left_10_differ': _spec(7, '10', False, LEFT), 'left_00_agree': _spec(7, '00', True, LEFT),
    'extrin_11_differ': _spec(7, '11', False, extrin=True), 'extrin_01_agree': _spec(7, '01', True, extrin=True),
    'leg46_10_differ': _spec(7, '10', False, leg=46),
    'notrack_00_agree': _spec(7, '00', True, tracking_ok=0),
})


def names():
    return list(SPECS)


def possible_sets(N):
    return [[N - 3, N - 2], [0, N - 3], [0, N - 5], [0, 1]]


def _base(N, flags, leg, extrin, scale, draw=0):
    """the window, its first update's tracks, the mirror's dx, the records before and after -- shared by the cases of one shape"""
    def make():
        fl = synth.Flags(leg_dim=leg, **flags)
        w = synth.make_window(N=N, track_len=(2, N), flags=fl, estimate_extrin=extrin, outlier_frac=0.1, F=WINDOWS[N]['F'], seed=WINDOWS[N]['seed'] + draw)
        w = dataclasses.replace(w, P=np.ascontiguousarray(w.P * scale))
        tracked = tc.ends_at_newest(w)
        lost = ~tracked & (np.diff(w.obs_ptr) >= 2)
        lost &= np.cumsum(lost) <= MAX_FIRST
        first = select_tracks(w, lost)
        assert 10 <= first.F <= MAX_FIRST, first.F
        left = bool(fl.use_larvio or fl.use_left_perturbation)
        ext = (np.array(w.R_b2c[N - 1]), np.array(w.t_c_b[N - 1]))   # the IMU state's extrinsic: what the newest clone froze
        head = mirror_frame.step_frame(w.P, dict(w=first), 1, 1, augment=False, table=mirror.chi2_table(fl.chi2_prob))
        dx = np.asarray(head['dx'], dtype=np.float64)
        cam_pre = mc.cam_records(w.R_b2w, w.t_b_w, ext[0], ext[1])
        cam_post = mc.cam_after(w, dx, ext, left)
        if extrin:
            assert np.abs(dx[15:21]).min() > 0.0
        return dict(w=w, first=first, tracked=tracked, left=left, ext=ext, dx_ref=dx, cam_pre=cam_pre, cam_post=cam_post)
    return cached(('ccbase', N, tuple(sorted(flags.items())), leg, extrin, scale, draw), make)


def _candidates(values):
    v = np.unique(np.asarray(values, dtype=np.float64))
    return [0.5 * v[0]] + [0.5 * (a + b) for a, b in zip(v[:-1], v[1:])] + [2.0 * v[-1]]


def _margin(run, rt, tt):
    return min(min(abs(a - rt) / max(1.0, rt), abs(d - tt) / max(1.0, tt)) for a, d in zip(run['angle'], run['distance']))


def _place(base, spec):
    """(margin, rot_thr, trans_thr) of the best candidate pair, or None"""
    N = spec['N']
    cams = (base['cam_pre'], base['cam_post'])
    qs = [mc.quantities(cam, c, N - 4) for cam in cams for c in (N - 3, N - 2, N - 5)]
    best = None
    for rt in _candidates([q[0] for q in qs]):
        for tt in _candidates([q[1] for q in qs]):
            pre, post = (mc.choose(cam, rt, tt, spec['tracking_ok']) for cam in cams)
            if tuple(post['taken']) != spec['pattern'] or (pre['chosen'] == post['chosen']) != spec['agree']:
                continue
            m = min(_margin(pre, rt, tt), _margin(post, rt, tt))
            if best is None or m > best[0]:
                best = (m, rt, tt)
    return best


def case(name):
    def make():
        spec = SPECS[name]
        for draw, scale in ((d, sc) for d in DRAWS for sc in PRIOR_SCALES):   # (a wider prior: a larger dx, pre- and post-update values further apart)
            base = _base(spec['N'], spec['flags'], spec['leg'], spec['extrin'], scale, draw)
            got = _place(base, spec)
            if got is not None and got[0] >= MARGIN:
                break
        assert got is not None and got[0] >= MARGIN, (name, got)
        c = dict(base, name=name, rot_thr=got[1], trans_thr=got[2], tracking_ok=spec['tracking_ok'], margin=got[0], pattern=spec['pattern'],
                 agree=spec['agree'], N=spec['N'], prior_scale=scale, draw=draw)
        c['predicted'] = mc.choose(c['cam_pre'], c['rot_thr'], c['trans_thr'], c['tracking_ok'])['chosen']
        c['truth'] = mc.choose(c['cam_post'], c['rot_thr'], c['trans_thr'], c['tracking_ok'])['chosen']
        return c
    return cached(('cccase', name), make)


def prune_for(c, remove):
    """the prune tracks that follow from a remove set: the tracked features seen in both clones that leave, restricted to those clones"""
    w = c['w']
    sub = synth.subset_tracks(w, list(remove), min_obs=2)
    sel = c['tracked'] & (np.diff(sub.obs_ptr) >= 2)
    sel &= np.cumsum(sel) <= MAX_PRUNE
    return select_tracks(sub, sel)


def choose_kwargs(c, cam_poses=None, **over):
    """the keyword arguments of capi.MsckfUpdater.io_choose_clones for a case"""
    kw = dict(cam_poses=c['cam_pre'] if cam_poses is None else cam_poses, rotation_threshold=c['rot_thr'], translation_threshold=c['trans_thr'],
              tracking_ok=c['tracking_ok'], R_imu_cam0=c['ext'][0], t_cam0_imu=c['ext'][1])
    kw.update(over)
    return kw
