"""The cases behind tests/golden/object_stage_parent.npz: what scripts/make_golden_object_stage.py records on a build of the parent of
the commit that gave the object update's host staging one home (csrc/host/object_stage.hpp), and tests/test_gpu_object_stage_parent.py
replays.  A window of N = 6 clones; object tracks of K in {0, 1, 3, 17} keypoints and at most five frames, one to three per update, at
the shapes where the staging takes another branch (frames outside the window, a NaN observation, clones in descending order, two frames
on one clone, a skipped track, nothing usable, a block that is not [6 | 3 | 3K]); every case through six entry points (ENTRIES) on four
handles (MODES: the product form, ORCVIO_OBJ_FUSED=0 on the diagnostics build, ORCVIO_OPT_OBJECT_QR = 0, ORCVIO_OPT_REF_STACK_HF = 1).

Per (case, mode, entry) the record holds integers -- rc, dof, accept, stats[0..7], objects_refined, counter [5] behind the call (obj_fused: did the
last object update take the one-launch compression) and what the call added to counter [7] (prestaged_frames) -- and four float arrays: the compressed block, dx, P and gamma (absent ones are empty)."""
import ctypes as C
import hashlib
import os

import numpy as np

from orcvio_amd import capi, synth
import tri_io_cases as tc

N = 6
MODES = ('product', 'unfused', 'gram', 'refstack')
ENTRIES = ('local_tracks', 'local_rows', 'update_tracks', 'update_rows', 'frame', 'frame_staged')
FLOATS = ('block', 'dx', 'P', 'gamma')
INTS = ('rc', 'dof', 'accept') + tuple('stats[%d]' % i for i in range(8)) + ('objects_refined', 'obj_fused', 'prestaged_frames')
PRIMER = 'one_k3'
FLAGS = synth.Flags(use_larvio=0, use_left_perturbation=0)


def window():
    return tc.cached('osp_window', lambda: synth.make_window(N=N, F=12, seed=4, flags=FLAGS, track_len=(3, N), outlier_frac=0.05))


def _with_keypoints(ob, K, seed):
    """the track with K keypoints: the first K of its twelve, or five more (observed where the estimate projects them, plus noise)"""
    K0 = ob.kps.shape[0]
    if K <= K0:
        ob.kps = ob.kps[:K].copy()
        for fr in ob.frames:
            fr['zs'] = fr['zs'][:K].copy()
        return ob
    rng = np.random.default_rng(seed)
    extra = ob.kps[:K - K0] + np.array([0.05, -0.04, 0.03])
    ob.kps = np.vstack([ob.kps, extra])
    for fr in ob.frames:
        Xc = (np.linalg.inv(fr['wTc']) @ ob.wTo @ np.hstack([extra, np.ones((len(extra), 1))]).T).T
        fr['zs'] = np.vstack([fr['zs'], Xc[:, :2] / Xc[:, 2:3] + 0.004 * rng.standard_normal((len(extra), 2))])
    return ob


def _tracks(spec, seed):
    """spec: (K, F) per track"""
    win, out = window(), []
    for k, (K, F) in enumerate(spec):
        ob = synth.make_objects(win, n_objects=1, seed=seed + 10 * k, sigma_kp=0.004, frames_per_object=F, missing_frac=0.0, bbox_only=K == 0)[0]
        out.append(ob if K == 0 else _with_keypoints(ob, K, seed + 10 * k + 1))
    return out


def _c_one():
    return _tracks([(3, 5)], 2)


def _c_mixed():
    return _tracks([(0, 3), (1, 3), (3, 5)], 3)


def _c_k17():
    return _tracks([(17, 4), (3, 5)], 4)


def _c_equal():   # (equal state sizes: the shape ORCVIO_OPT_REF_STACK_HF takes)
    return _tracks([(3, 5), (3, 4), (3, 3)], 5)


def _c_outside():
    objs = _tracks([(3, 5), (3, 5)], 6)
    for f in (0, 2, 4):
        objs[0].frames[f]['clone'] = -1
    objs[1].frames[1]['zs'][0, 0] = np.nan   # one coordinate of one observation
    objs[1].frames[3]['clone'] = -1
    return objs


def _c_descending():
    objs = _tracks([(3, 5), (1, 4)], 7)
    for ob in objs:
        ob.frames = ob.frames[::-1]
    return objs


def _c_shared_clone():
    objs = _tracks([(3, 5), (3, 4)], 8)
    fr = objs[0].frames
    fr[3] = dict(fr[3], clone=fr[0]['clone'], wTc=fr[0]['wTc'].copy())   # two frames on one clone, not adjacent
    return objs


def _c_skipped():
    objs = _tracks([(3, 5), (3, 5)], 9)
    for f in (1, 2, 3, 4):
        objs[0].frames[f]['clone'] = -1   # 10 rows <= 18 columns
    return objs


def _c_all_skipped():
    objs = _tracks([(3, 5), (1, 3)], 10)
    for ob in objs:
        for fr in ob.frames[1:]:
            fr['clone'] = -1
    return objs


def _c_rows_plain10():
    """rows only: a block of ten object-state columns -- not the [6 | 3 | 3K] shape, the Gram route"""
    rng = np.random.default_rng(11)
    return [dict(row_clone=rng.integers(0, N, 14).astype(np.int32), Hx6=rng.standard_normal((14, 6)), Hf=rng.standard_normal((14, 10)),
                 res=0.004 * rng.standard_normal(14))]


CASES = {
    'one_k3': _c_one, 'mixed_k0_k1_k3': _c_mixed, 'k17_k3': _c_k17, 'equal_k3': _c_equal, 'outside_nan': _c_outside, 'descending': _c_descending,
    'shared_clone': _c_shared_clone, 'skipped': _c_skipped, 'all_skipped': _c_all_skipped, 'rows_plain10': _c_rows_plain10,
}


def tracks_of(case):
    return None if case == 'rows_plain10' else tc.cached(('osp_tracks', case), CASES[case])


def handle(mode):
    """A handle in one of MODES (ORCVIO_OBJ_FUSED is read when the handle is made)."""
    if mode == 'unfused':
        os.environ['ORCVIO_OBJ_FUSED'] = '0'
    try:
        u = capi.MsckfUpdater(device=0, max_clones=8, max_features=64, max_observations=1024, debug_hooks=mode == 'unfused')
    finally:
        os.environ.pop('ORCVIO_OBJ_FUSED', None)
    if mode == 'gram':
        u._chk(u.lib.orcvio_msckf_set_option(u.h, 8, 0), 'set_option')   # ORCVIO_OPT_OBJECT_QR
    if mode == 'refstack':
        u._chk(u.lib.orcvio_msckf_set_option(u.h, 9, 1), 'set_option')   # ORCVIO_OPT_REF_STACK_HF
    return u


def blocks_of(u, case):
    """the rows entry points' input: the tracks' rows as orcvio_msckf_object_rows_eval gives them (tracks without a frame in the window left out)"""
    if case == 'rows_plain10':
        return CASES[case]()
    win = window()
    bl = [u.object_rows_eval(ob, win.R_b2c[0], win.t_c_b[0], True, False, 0) for ob in tracks_of(case)]
    return [b for b in bl if b is not None]


def _block(u):
    u.sync()
    ptr, ne = u.block_ptr()
    out = np.zeros(ne)
    assert C.CDLL('libamdhip64.so').hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(ne * 8), 2) == 0
    return out


def run_entry(u, case, entry):
    """dict(ints [len(INTS)], block, dx, P, gamma) of one entry point on handle u, or None where the case has no such input"""
    win, objs = window(), tracks_of(case)
    ext = (win.R_b2c[0], win.t_c_b[0], True, False, 0)
    if objs is None and entry not in ('local_rows', 'update_rows'):
        return None
    c0 = u.counters()
    got = dict(rc=0, dof=0, accept=0, stats=[0] * 8, refined=0)
    empty = np.zeros(0)
    arrs = dict(block=empty, dx=empty, P=empty, gamma=empty)
    try:
        if entry == 'local_tracks':
            got['dof'] = u.objects_local_tracks(FLAGS, N, objs, win.P, *ext)
            arrs['block'] = _block(u)
        elif entry == 'local_rows':
            got['dof'] = u.objects_local(FLAGS, N, blocks_of(u, case), win.P)
            arrs['block'] = _block(u)
        elif entry in ('update_tracks', 'update_rows'):
            o = u.update_object_tracks(FLAGS, N, objs, win.P, *ext) if entry == 'update_tracks' else u.update_objects(FLAGS, N, blocks_of(u, case), win.P)
            got.update(dof=int(o['stats'][0]), accept=int(o['accept']), stats=[int(x) for x in o['stats']], refined=u.objects_refined())
            arrs.update(dx=o['dx'], P=o['P_new'], gamma=np.array([o['gamma']]))
        else:
            u.cov_set(win.P)
            io = u.io_begin(win.flags, win.N, win.F, int(win.obs_ptr[-1]), with_P=False)
            u.io_fill(io, win, with_P=False)
            call, outs = u.make_frame_call(win, FLAGS, objs, *ext)
            if entry == 'frame_staged':
                call.stage()
            try:
                call()
                f, o = outs()
                got.update(dof=int(o['stats'][0]), accept=int(o['accept']), stats=[int(x) for x in o['stats']], refined=u.objects_refined())
                arrs.update(dx=np.concatenate([f['dx'], o['dx']]), gamma=np.concatenate([f['gamma'], [o['gamma']]]))
            finally:
                arrs['P'] = u.cov_get()
    except capi.MsckfError as e:   # (a refusal: its code is the record)
        got['rc'] = int(e.code)
    c1 = u.counters()
    ints = [got['rc'], got['dof'], got['accept']] + list(got['stats']) + [got['refined'], c1['obj_fused'], c1['prestaged_frames'] - c0['prestaged_frames']]
    return dict(ints=np.array(ints, np.int64), **{k: np.ascontiguousarray(v, dtype=np.float64).ravel() for k, v in arrs.items()})


def run_case(u, case):
    """{entry: run_entry's dict} of one case.  The handle first runs PRIMER through every entry point, so that what a call leaves
    untouched (the words behind objects_refined and counter [5] when nothing is usable or the call refuses) does not depend on the
    case that ran before."""
    for entry in ENTRIES:
        run_entry(u, PRIMER, entry)
    got = {entry: run_entry(u, case, entry) for entry in ENTRIES}
    return {e: g for e, g in got.items() if g is not None}


def keys():
    """the (case, mode, entry) triples of the golden, in its order"""
    return [(c, m, e) for m in MODES for c in CASES for e in ENTRIES if tracks_of(c) is not None or e in ('local_rows', 'update_rows')]


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()[:8], np.uint8)
