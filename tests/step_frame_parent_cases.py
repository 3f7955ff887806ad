"""The streams behind tests/golden/step_frame_parent.npz: what scripts/make_golden_step_frame.py records on a build of the parent commit
and tests/test_gpu_step_frame_parent.py replays.  Every stream is eight deterministic frames of orcvio_msckf_io_step_frame / _ex on a
handle of max_clones 24, max_features 256, max_observations 4096; each runs on the product build, on the diagnostics build with
ORCVIO_STEP_FUSED=0 and with ORCVIO_LA_SPIN=0 (every hand-off lost: the repair path).

Per frame the record holds the integers the call reports (rc, status_first, status_prune, status_changes, repaired, n_after, stats,
prune_stats, the choice block's evaluated / agree / chosen) and the first eight bytes of sha256 over the raw bytes of dx, gamma, accept,
prune_dx, prune_gamma, prune_accept, new_param, new_inv_depth and cov_get() -- equality of the bytes, NaN positions included.  (The raw
float64 arrays of 13 streams x 3 forms x 8 frames are about 2 MB; the file has to stay under 100 KB.)  So that a mismatch can be read,
the product form's last frame keeps dx and the covariance's diagonal as they are."""
import dataclasses
import hashlib
import os

import numpy as np

from orcvio_amd import capi, synth
import clone_choice_cases as cc
import imu_cases as ic
import tri_io_cases as tc

EUROC = dict(use_larvio=1)
MODES = ('product', 'unfused', 'repair')
HASHED = ('dx', 'gamma', 'accept', 'prune_dx', 'prune_gamma', 'prune_accept', 'new_param', 'new_inv_depth', 'P')
INTS = ('rc', 'status_first', 'status_prune', 'status_changes', 'repaired', 'n_after')
CHOICE_AGREE = ('n7_11_agree', 'n7_10_agree', 'n6_01_agree', 'n6_00_agree', 'right_01_agree', 'left_00_agree', 'extrin_01_agree', 'notrack_00_agree')
CHOICE_HELD = ('n7_11_differ', 'n7_10_differ', 'n6_01_differ', 'n6_00_differ', 'right_10_differ', 'left_10_differ', 'extrin_11_differ', 'leg46_10_differ')


def handle(mode):
    """A handle in one of MODES (the switches are read when the handle is made)."""
    env = {'unfused': 'ORCVIO_STEP_FUSED', 'repair': 'ORCVIO_LA_SPIN'}.get(mode)
    if env:
        os.environ[env] = '0'
    try:
        u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096, debug_hooks=mode == 'unfused')
    finally:
        if env:
            del os.environ[env]
    u.set_ekf_rows_mode(True)
    return u


def _hidden(w):
    return dataclasses.replace(w, p_w=np.full_like(np.asarray(w.p_w, dtype=np.float64), np.nan))


def _plain(u, fr, **kw):
    return u.io_step_frame(fr['w'], fr['Phi'], fr['Q'], True, fr['slam'], 1, fr['prune'], True, fr['remove'], raise_on_refusal=False, **kw)


def _ex(u, fr, idp, apply_dx, **over):
    u.set_extra_states(fr['w'].n_extra)
    kw = dict(win=fr['w'], Phi=fr['Phi'], Q=fr['Q'], augment=True, slam=fr['slam'], idp_dim=idp, prune=fr['prune'], prune_apply_dx=apply_dx,
              remove=fr['remove'], n_feature_states=fr['n_feature_states'], lost=fr['lost'], changes=fr['changes'], R_b2c=fr['R_b2c'],
              t_c_b=fr['t_c_b'], literal_3d=0, raise_on_refusal=False)
    kw.update(over)
    return u.io_step_frame_ex(**kw)


def _lifecycle(idp=1):
    return tc.cached(('sfp_lifecycle', idp), lambda: synth.make_lifecycle_stream(synth.Flags(**EUROC), n_slam=16, min_slam=8, idp=idp))


def _stream():
    return tc.cached('sfp_stream', lambda: synth.make_stream(synth.Flags(**EUROC)))


def _imu_arm(u, case):
    cfg, state, prev = ic.to_capi(case)
    u.io_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])


# ---- the streams: generators of (what the call returned, or the MsckfError it raised) ----------------------------------------------------
def s_plain(u):
    frames, P0 = _stream()
    u.set_extra_states(12)
    u.cov_set(P0)
    for fr in frames:
        yield lambda: _plain(u, fr)


def s_ex(idp, apply_dx):
    def run(u):
        frames, P0 = _lifecycle(idp)
        u.cov_set(P0)
        for fr in frames:
            yield lambda: _ex(u, fr, idp, apply_dx)
    return run


def s_tri(u):
    frames, P0 = _stream()
    u.set_extra_states(12)
    u.cov_set(P0)
    for fr in frames:
        yield lambda: _plain(u, dict(fr, w=_hidden(fr['w'])), triangulate=True)


def s_tri_prune(u):
    frames, P0 = _lifecycle(1)
    u.cov_set(P0)
    for fr in frames:
        if fr['prune'] is None:
            yield lambda: _ex(u, fr, 1, 0)
            continue
        sel = np.diff(fr['prune'].obs_ptr) >= 2
        tri_win, prune = tc.select_tracks(fr['w'], sel), tc.select_tracks(fr['prune'], sel)
        yield lambda: _ex(u, fr, 1, 0, prune=_hidden(prune), triangulate_prune=(tri_win, None))


def s_choice(names):
    def run(u):
        u.set_ekf_rows_mode(False)
        for name in names:
            c = cc.case(name)
            u.cov_set(c['w'].P)
            yield lambda: u.io_step_frame(c['first'], None, None, False, None, 1, cc.prune_for(c, c['predicted']), 1, c['predicted'],
                                          raise_on_refusal=False, choose_clones=cc.choose_kwargs(c))
    return run


def s_imu(u):
    frames, P0 = _lifecycle(1)
    u.cov_set(P0)
    for it, fr in enumerate(frames):
        def call():
            u.set_extra_states(fr['w'].n_extra)
            _imu_arm(u, ic.make_case('larvio', 5 + it, n=22, seed=60 + it, rate=200.0))
            return _ex(u, fr, 1, 1, Phi=None, Q=None)
        yield call


def s_imu_refused(u):
    """frame 1: the right closed form with an exactly zero gyro sample -- Phi is refused on the device"""
    frames, P0 = _stream()
    u.set_extra_states(12)
    u.cov_set(P0)
    for it, fr in enumerate(frames):
        if it != 1:
            yield lambda: _plain(u, fr)
            continue
        case = ic.make_case('right_closed', 5, n=22, seed=54)
        case['samples'][2, 1:4] = case['state'].bg

        def call():
            _imu_arm(u, case)
            return _plain(u, dict(fr, Phi=None, Q=None))
        yield call


def s_no_first(u):
    """frame 3 (20 clones, the prune update, the marginalisation) without a lost track and without in-state rows: no first update"""
    frames, P0 = _stream()
    u.set_extra_states(12)
    u.cov_set(P0)
    for it, fr in enumerate(frames):
        if it == 3:
            fr = dict(fr, w=tc.select_tracks(fr['w'], np.zeros(fr['w'].F, bool)), slam=None)
        yield lambda: _plain(u, fr)


def s_nonfinite_change(u):
    """tests/test_gpu_step_frame_ex.py's refusal: a changed feature's inverse depth + dx == 0 exactly (frames 1 and 2 are the frame
    that reads dx and its repeat from the same covariance)"""
    frames, P0 = _lifecycle(1)
    u.cov_set(P0)
    yield lambda: _ex(u, frames[0], 1, 1)
    P1 = u.cov_get()
    fr = frames[1]
    c = fr['changes'][0]
    slam = list(fr['slam'])
    slam[c.slot] = dataclasses.replace(slam[c.slot], z=slam[c.slot].z + 5.0)
    col = fr['w'].flags.leg_dim + 6 * fr['w'].N + c.slot
    seen = {}

    def first():
        seen['got'] = _ex(u, dict(fr, slam=slam), 1, 1)
        return seen['got']
    yield first
    slam2 = list(slam)
    slam2[c.slot] = dataclasses.replace(slam[c.slot], inv_depth=-float(seen['got']['dx'][col]))
    u.cov_set(P1)
    yield lambda: _ex(u, dict(fr, slam=slam2), 1, 1)
    for fr in frames[2:7]:
        yield lambda: _ex(u, fr, 1, 1)


STREAMS = {
    'plain': s_plain,
    'ex_idp1_copy': s_ex(1, 0), 'ex_idp1_increment': s_ex(1, 1), 'ex_idp3_copy': s_ex(3, 0), 'ex_idp3_increment': s_ex(3, 1),
    'tri': s_tri, 'tri_prune': s_tri_prune,
    'choice_agree': s_choice(CHOICE_AGREE), 'choice_held': s_choice(CHOICE_HELD),
    'imu': s_imu, 'imu_refused': s_imu_refused,
    'no_first': s_no_first, 'nonfinite_change': s_nonfinite_change,
}


def _digest(a):
    if a is None:
        return np.zeros(8, np.uint8)
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()[:8], np.uint8)


def run_stream(name, mode):
    """dict(ints [frames, 26], hash [frames, 9, 8], last_dx, last_diag) of one stream on a fresh handle"""
    u = handle(mode)
    ints, hashes, got = [], [], None
    try:
        for call in STREAMS[name](u):
            try:
                got = call()
            except capi.MsckfError as e:   # (a refusal of the whole call: its code is the record)
                got = dict(rc=int(e.code))
            got['P'] = u.cov_get()
            ch = got.get('choice')
            row = [int(got.get(k, 0)) for k in INTS] + list(got.get('stats', [0] * 8)) + list(got.get('prune_stats', [0] * 8))
            row += [ch['evaluated'], ch['agree']] + list(ch['chosen']) if ch else [-1, -1, -1, -1]
            ints.append(row)
            hashes.append(np.stack([_digest(got.get(k)) for k in HASHED]))
    finally:
        u.close()
    dx = got.get('dx')
    return dict(ints=np.array(ints, np.int32), hash=np.stack(hashes), last_dx=np.zeros(0) if dx is None else dx, last_diag=np.diag(got['P']).copy())
