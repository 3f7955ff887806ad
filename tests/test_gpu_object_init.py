"""orcvio_msckf_object_init / orcvio_msckf_object_init_lm (k_object_init: keypoint triangulation, Kabsch alignment and the pose
form, one workgroup per object) against the numpy mirror (tests/mirror_object_init.py) on the same inputs.

Tolerances, element-wise and absolute, every one capped at the project's bar of 1e-6 (a case that would reach the cap is not a case):
  triangulated point k   10 max(e_mirror, cond(A_k)^2 2^-52) |p_k|   -- e_mirror: the mirror's relative error against the 60-digit
                         evaluation of that case; the second term: the forward error of the normal equations the device forms;
  pose, stage by stage   the mirror's Kabsch run ON THE DEVICE'S points: 10 max(e_mirror, K 2^-52 sigma_1 / (sigma_2 + d sigma_3));
  pose, end to end       the mirror from the detections: the above plus the largest triangulation tolerance times the same factor;
  kp_cond, sigma         relative 1e-6 (diagnostics).
Pose form 1 takes yaw = pi / atan2(T10, T00), unbounded near zero: its cases have |atan2| > 1.45, where d yaw / d atan2 < 1.5."""
import ctypes as C
import dataclasses
import functools
import subprocess

import numpy as np
import pytest

from orcvio_amd import capi, synth
from helpers import rel, objects_update_reference
from test_host_shim import _build
import mirror_object_init as mi
import mirror_object_lm as mlm
import object_lm_cases as oc

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
CAP = 1e-6


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=48, max_features=64, max_observations=1024)
    yield u
    u.close()


def _second_pass_track():
    """K = 12, F = 128, every keypoint detected everywhere but: keypoint 0 only in frames >= 64 (the second pass alone), keypoint 1
    last in frame 63 (anchor = the first pass's last lane), keypoint 2 last in frame 64 (anchor = the second pass's first lane)."""
    obj, ms, mk = oc.synthetic(12, 128, 1, missing_frac=0.0)
    for f, fr in enumerate(obj.frames):
        if f < 64:
            fr['zs'][0] = np.nan
        if f > 63:
            fr['zs'][1] = np.nan
        if f > 64:
            fr['zs'][2] = np.nan
    return obj, ms, mk


def _threshold_track(kp4_detections):
    """one_car cut to 6 frames, keypoints 1, 4, 6, 11 alone: 1 and 11 detected in all 6 frames, 6 in 4 (= min_obs + 1; in one of the
    others only ONE coordinate is NaN), 4 in `kp4_detections` frames."""
    obj, ms, mk = oc.one_car(6)
    for fr in obj.frames:
        fr['zs'][[0, 2, 3, 5, 7, 8, 9, 10]] = np.nan
    for f in range(kp4_detections, 6):
        obj.frames[f]['zs'][4] = np.nan
    obj.frames[0]['zs'][6] = np.nan
    obj.frames[5]['zs'][6, 1] = np.nan
    return obj, ms, mk


CASES = {
    'car_f4': lambda: oc.one_car(4), 'car_f5': lambda: oc.one_car(5), 'car_f47': lambda: oc.one_car(47),
    'K4_F64': lambda: oc.synthetic(4, 64, 2), 'K12_F65': lambda: oc.synthetic(12, 65, 1), 'K16_F128': lambda: oc.synthetic(16, 128, 1),
    'second_pass': _second_pass_track,
    'used_1_4_6_11': lambda: _threshold_track(4),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(track, mean_shape, mean_kps) -- built once per session: do not modify."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, pose_form):
    """(mirror, e_tri, e_pose): the mirror's result and its relative error against the 60-digit evaluation, triangulated points and
    pose (wTo, R_kabsch, t_kabsch, scale).  Computed once per session: do not modify."""
    obj, _, mk = case(name)
    cfg = mi.Config(pose_form=pose_form)
    m, ref = mi.solve(obj, mk, cfg), mi.solve_mp(obj, mk, cfg)
    assert m['status'] == ref['status'] == mi.STATUS_OK
    e_tri = mi.relative_error(m['kps_world'], ref['kps_world'])
    flat = lambda r: np.concatenate([np.ravel(r['wTo']), np.ravel(r['R']), np.ravel(r['t']), [r['scale']]])
    e_pose = mi.relative_error(flat(m), flat(ref))
    assert np.nanmax(m['kp_cond']) < 1e4 and m['ratio'] < 1e4      # (a valid case: no tolerance reaches the cap)
    return m, e_tri, e_pose


def _tri_tolerances(m, e_tri):
    K = len(m['kp_used'])
    tol = np.zeros(K)
    for k in np.flatnonzero(m['kp_used']):
        tol[k] = 10.0 * max(e_tri, m['kp_cond'][k] ** 2 * EPS) * float(np.linalg.norm(m['kps_world'][k]))
    assert tol.max() < CAP
    return tol


def _pose_diff(a, b):
    return max(float(np.abs(a['wTo'] - b['wTo']).max()), float(np.abs(a['R'] - b['R']).max()), float(np.abs(a['t'] - b['t']).max()),
               abs(a['scale'] - b['scale']))


def _check(tag, dev, name, pose_form):
    m, e_tri, e_pose = reference(name, pose_form)
    _, _, mk = case(name)
    K = len(mk)
    assert dev['status'] == m['status'] == 1 and dev['n_used'] == m['n_used']
    assert np.array_equal(dev['kp_used'], m['kp_used']) and np.array_equal(dev['kp_obs'], m['kp_obs'])
    used = m['kp_used'] != 0
    assert np.all(np.isnan(dev['kps_world'][~used])) and np.all(np.isnan(dev['kp_cond'][~used]))
    # triangulation
    tol_tri = _tri_tolerances(m, e_tri)
    d_tri = np.abs(dev['kps_world'][used] - m['kps_world'][used]).max(axis=1)
    assert np.all(d_tri <= tol_tri[used]), (tag, d_tri, tol_tri[used])
    assert np.all(np.abs(dev['kp_cond'][used] - m['kp_cond'][used]) <= 1e-6 * m['kp_cond'][used])
    # the pose, stage by stage: the mirror's Kabsch on the device's points
    stage = mi.kabsch(mk, dev['kps_world'], dev['kp_used'], mi.Config(pose_form=pose_form))
    tol_pose = 10.0 * max(e_pose, K * EPS * stage['ratio'])
    d_pose = _pose_diff(dev, stage)
    # ... and end to end from the detections
    tol_e2e = tol_pose + stage['ratio'] * float(tol_tri.max())
    d_e2e = _pose_diff(dev, m)
    assert tol_e2e < CAP
    print('%s form %d: points %.2e (tol %.2e .. %.2e, e_mirror %.1e, cond %.1f .. %.1f) | pose on the device points %.2e (tol %.2e, e_mirror %.1e, '
          'ratio %.2f) | end to end %.2e (tol %.2e) | atan2 %.3f'
          % (tag, pose_form, d_tri.max(), tol_tri[used].min(), tol_tri[used].max(), e_tri, m['kp_cond'][used].min(), m['kp_cond'][used].max(), d_pose,
             tol_pose, e_pose, stage['ratio'], d_e2e, tol_e2e, np.arctan2(stage['R'][1, 0], stage['R'][0, 0])))
    assert np.all(np.abs(dev['sigma'] - stage['sigma']) <= 1e-6 * stage['sigma'][0])
    assert d_pose <= tol_pose
    assert d_e2e <= tol_e2e
    # structure: rigid by construction, and the reference's literal matrix from its pieces
    T = dev['wTo']
    assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() <= 1e-14 and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    assert np.abs(dev['R'].T @ dev['R'] - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(dev['R']) - 1.0) <= 1e-14
    assert np.abs(mi.literal_matrix(dev) - mi.literal_matrix(stage)).max() <= tol_pose * max(1.0, stage['scale'])
    if pose_form:
        assert T[2, 3] == 0.0 and np.array_equal(T[2, :3], [0.0, 0.0, 1.0]) and np.array_equal(T[:2, 3], dev['t'][:2])
        if pose_form == 1:
            assert abs(np.arctan2(stage['R'][1, 0], stage['R'][0, 0])) > 1.45


@pytest.mark.parametrize('name', list(CASES))
def test_against_the_mirror(upd, name):
    """one_car at F = 4 (the minimum), 5 and 47 (K = 12); synthetic K = 4 / F = 64 (the last lane of one pass), K = 12 / F = 65 (one
    frame in the second pass), K = 16 / F = 128 (both caps), each with a tenth of the detections missing; F = 128 with a keypoint seen
    in the second pass only and anchors in frames 63 and 64; used ids 1, 4, 6, 11 (not contiguous).  All three pose forms."""
    obj, _, mk = case(name)
    for form in (0, 1, 2):
        dev = upd.object_init([obj], [mk], pose_form=form)[0]
        _check(name, dev, name, form)
    if name == 'second_pass':
        assert list(dev['kp_obs'][:3]) == [64, 64, 65]
    if name == 'used_1_4_6_11':
        assert list(np.flatnonzero(dev['kp_used'])) == [1, 4, 6, 11] and list(dev['kp_obs']) == [0, 6, 0, 0, 4, 0, 4, 0, 0, 0, 0, 6]
        ids = [1, 4, 6, 11]
        chord = lambda X: sum(np.linalg.norm(X[b] - X[a]) for a, b in zip(ids[:-1], ids[1:]))
        assert abs(dev['scale'] - chord(dev['kps_world']) / chord(mk)) <= 8 * EPS * dev['scale']   # the chords run over the used list


def test_thresholds_are_strict(upd):
    """A keypoint with exactly min_obs detections is not used (one with min_obs + 1 is: keypoint 6); exactly min_kps used keypoints
    is status 2 and the identity (min_kps + 1 is status 1: test_against_the_mirror's used_1_4_6_11); the thresholds are the config's."""
    obj, _, mk = _threshold_track(3)
    m = mi.solve(obj, mk)
    dev = upd.object_init([obj], [mk])[0]
    assert list(dev['kp_obs']) == list(m['kp_obs']) == [0, 6, 0, 0, 3, 0, 4, 0, 0, 0, 0, 6]
    assert list(np.flatnonzero(dev['kp_used'])) == [1, 6, 11] and dev['n_used'] == 3
    assert dev['status'] == m['status'] == 2 and np.array_equal(dev['wTo'], np.eye(4))
    assert np.all(np.isnan(dev['R'])) and np.all(np.isnan(dev['t'])) and np.isnan(dev['scale']) and np.all(np.isnan(dev['sigma']))
    tol = _tri_tolerances(m, reference('used_1_4_6_11', 1)[1])      # (the same frames: that case's mirror error)
    for k in (1, 6, 11):
        assert np.abs(dev['kps_world'][k] - m['kps_world'][k]).max() <= tol[k]
    assert np.all(np.isnan(dev['kps_world'][4]))
    # min_obs = 2 takes keypoint 4 with its three detections; min_kps = 4 refuses the four keypoints
    dev = upd.object_init([obj], [mk], min_obs=2)[0]
    assert dev['status'] == 1 and list(np.flatnonzero(dev['kp_used'])) == [1, 4, 6, 11]
    dev = upd.object_init([obj], [mk], min_obs=2, min_kps=4)[0]
    assert dev['status'] == 2 and dev['n_used'] == 4 and np.array_equal(dev['wTo'], np.eye(4))


def _same(a, b):
    for key in ('wTo', 'kps_world', 'kp_used', 'kp_obs', 'kp_cond', 'R', 't', 'sigma'):
        if not np.array_equal(a[key], b[key], equal_nan=True):
            return False
    return a['n_used'] == b['n_used'] and a['status'] == b['status'] and (a['scale'] == b['scale'] or (np.isnan(a['scale']) and np.isnan(b['scale'])))


def _twenty():
    shapes = [(1, 1), (1, 9), (2, 3), (3, 17), (4, 2), (4, 33), (5, 5), (6, 12), (7, 1), (8, 64), (9, 4), (10, 31), (11, 7), (12, 30),
              (12, 65), (13, 2), (14, 16), (15, 3), (16, 8), (16, 128)]
    return [oc.synthetic(K, F, seed=3 + i) for i, (K, F) in enumerate(shapes)]


def test_batch_of_twenty_equals_one_object_per_call_bit_for_bit(upd):
    """Twenty objects of different K, F and status (K < 4 or F < 4 cannot be initialised: status 2) in one launch against the same
    objects one per call: a workgroup's arithmetic does not depend on what else the launch holds."""
    cases = _twenty()
    objs, mk = [c[0] for c in cases], [c[2] for c in cases]
    for form in (0, 1):
        batch = upd.object_init(objs, mk, pose_form=form)
        status = [b['status'] for b in batch]
        assert 1 in status and 2 in status and all(s in (1, 2) for s in status)
        for i in range(len(objs)):
            one = upd.object_init([objs[i]], [mk[i]], pose_form=form)[0]
            assert _same(one, batch[i]), i
            want = mi.solve(objs[i], mk[i], mi.Config(pose_form=form))
            assert want['status'] == batch[i]['status'] and np.array_equal(want['kp_used'], batch[i]['kp_used'])
    print('batch: status %s' % status)


def test_one_call_equals_init_followed_by_lm_bit_for_bit(upd):
    """orcvio_msckf_object_init_lm against orcvio_msckf_object_init followed by orcvio_msckf_object_lm from its pose, the mean shape
    and the mean keypoints: the same bits.  The batch holds objects that cannot be initialised: LM status 0, the identity and the
    means, and the others are what they are without them."""
    cases = [oc.one_car(33), oc.one_car(47)] + _twenty()[:8]
    objs, ms, mk = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    w = oc.WEIGHTS_REF
    for form in (0, 2):
        inits, tracks, stats = upd.object_init_lm(objs, ms, mk, True, 0, w, pose_form=form)
        alone = upd.object_init(objs, mk, pose_form=form)
        good = [i for i in range(len(objs)) if alone[i]['status'] == 1]
        assert 0 in good and 1 in good and len(good) < len(objs)
        starts = [synth.ObjectTrack(wTo=alone[i]['wTo'], shape=ms[i].copy(), kps=mk[i].copy(), frames=objs[i].frames) for i in good]
        t2, s2 = upd.object_lm(starts, [ms[i] for i in good], [mk[i] for i in good], True, 0, w)
        for i in range(len(objs)):
            assert _same(inits[i], alone[i]), i
            if i in good:
                j = good.index(i)
                assert stats[i] == s2[j], (i, stats[i], s2[j])
                assert np.array_equal(tracks[i].wTo, t2[j].wTo) and np.array_equal(tracks[i].shape, t2[j].shape) and np.array_equal(tracks[i].kps, t2[j].kps)
            else:
                assert stats[i] == dict(cost0=0.0, cost=0.0, iterations=0, evaluations=0, status=0)
                assert np.array_equal(tracks[i].wTo, np.eye(4)) and np.array_equal(tracks[i].shape, ms[i]) and np.array_equal(tracks[i].kps, mk[i])
        print('form %d: init status %s, lm status %s, iterations %s' % (form, [a['status'] for a in alone], [s['status'] for s in stats],
                                                                         [s['iterations'] for s in stats]))
        assert stats[0]['status'] == 1 and stats[1]['status'] == 1


def test_detections_to_object_update_end_to_end(upd):
    """The closed chain: detections -> orcvio_msckf_object_init_lm -> orcvio_msckf_update_object_tracks, against mirror initialiser +
    mirror optimiser + the mirror's literal update (one_car, 30 of the 47 frames in the window).  The optimum is within the
    optimiser's existing tolerance of case_spread('f47')'s first run."""
    N = 30
    c = oc.CASES['f47']
    obj, ms, mk = oc.one_car(47)
    obj = dataclasses.replace(obj, frames=[dict(fr, clone=i if i < N else -1) for i, fr in enumerate(obj.frames)])
    flags = synth.Flags(use_larvio=0, use_left_perturbation=0, noise_feature=0.05)
    win = synth.make_window(N=N, F=2, seed=2, flags=flags, track_len=3)
    spread, runs = oc.case_spread('f47')
    mir = runs[0]
    ref = objects_update_reference(win, [dataclasses.replace(obj, wTo=mir['wTo'], shape=mir['shape'], kps=mir['kps'])], win.P, True, False, 0)
    inits, tracks, stats = upd.object_init_lm([obj], [ms], [mk], True, 0, c['weights'], pose_form=1)
    assert inits[0]['status'] == 1 and stats[0]['status'] == 1
    d = oc.distance(dict(wTo=tracks[0].wTo, shape=tracks[0].shape, kps=tracks[0].kps), mir)
    print('optimum from the device start: %.2e from the mirror (tol %.2e), cost %.13g / %.13g, iterations %d' % (d, min(CAP, 10 * spread), stats[0]['cost'], mir['cost'],
                                                                                                                 stats[0]['iterations']))
    assert d <= min(CAP, 10 * spread)
    got = upd.update_object_tracks(flags, win.N, tracks, win.P, win.R_b2c[0], win.t_c_b[0], True, False, 0)
    assert ref['accept'] == 1 and got['accept'] == ref['accept']
    assert abs(got['gamma'] - ref['gamma']) < 1e-6 * abs(ref['gamma'])
    assert rel(got['dx'], ref['dx']) < 1e-6 and rel(got['P_new'], ref['P_new']) < 1e-6


def _fmt(a):
    return ' '.join('nan' if not np.isfinite(v) else repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel())


def test_host_wrapper_equals_the_binding(upd, tmp_path):
    """MsckfBackend::single_object_initialization / object_initialization / levenberg_marquardt(.., initialize_on_device) run from
    tests/cpp/test_host_object_init.cpp: the same library calls as the binding's, so the same bits."""
    obj_nan, ms, mk = _threshold_track(3)      # status 2
    cases = [oc.one_car(5), (obj_nan, ms, mk), oc.one_car(33)]
    w = oc.WEIGHTS_REF
    lines = ['1 %d' % len(cases)]
    for obj, ms, mk in cases:
        lines.append('%d %d' % (mk.shape[0], len(obj.frames)))
        lines += [_fmt(w), _fmt(ms), _fmt(mk), _fmt([fr['wTc'] for fr in obj.frames]), _fmt([fr['zs'] for fr in obj.frames]),
                  _fmt([fr['bbox'] for fr in obj.frames])]
    path = tmp_path / 'cases.txt'
    path.write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'test_host_object_init')
    _build('test_host_object_init.cpp', exe)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'host object init ok' in out.stdout and 'refused 1 status 1' in out.stdout and 'short zs refused 1 status 1' in out.stdout
    objs, mss, mks = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    inits, tracks, stats = upd.object_init_lm(objs, mss, mks, True, 0, w, pose_form=1)
    alone = upd.object_init(objs, mks, pose_form=1)
    rows = {(t[0], int(t[1])): t for t in (ln.split() for ln in out.stdout.splitlines()) if t and t[0] in ('single', 'batch', 'chain_init', 'chain_lm')}
    for k in range(len(cases)):
        for tag, want in (('single', alone[k]), ('batch', alone[k]), ('chain_init', inits[k])):
            t = rows[(tag, k)]
            assert int(t[3]) == (1 if want['status'] == 1 else 0) and int(t[5]) == want['status'] and int(t[7]) == want['n_used']
            vals = np.array([float(t[9])] + [float(v) for v in t[11:]])
            exp = np.concatenate([[want['scale']], want['wTo'].ravel(), want['R'].ravel(), want['t'], want['sigma'], want['kps_world'].ravel(),
                                  want['kp_cond'], want['kp_used'], want['kp_obs']])
            assert np.array_equal(vals, exp, equal_nan=True), (tag, k)
        t = rows[('chain_lm', k)]
        assert int(t[3]) == stats[k]['status'] and int(t[5]) == stats[k]['iterations'] and int(t[7]) == stats[k]['evaluations']
        if stats[k]['status'] == 1:
            assert float(t[9]) == stats[k]['cost0'] and float(t[11]) == stats[k]['cost']
            assert np.array_equal(np.array([float(v) for v in t[13:]]), np.concatenate([tracks[k].wTo.ravel(), tracks[k].shape, tracks[k].kps.ravel()]))
        else:   # not initialised: not optimised, the caller's state stays
            assert stats[k]['status'] == 0 and np.array_equal(np.array([float(v) for v in t[13:29]]), np.eye(4).ravel())
    assert [s['status'] for s in stats] == [1, 0, 1]


def _raw(upd, obj, ms, mk, mutate, with_lm):
    """The library call on hand-made records; `mutate` edits them first.  Returns (rc, result arrays)."""
    lib = upd.lib
    K, F = mk.shape[0], len(obj.frames)
    wTc = np.ascontiguousarray(np.stack([fr['wTc'] for fr in obj.frames]), dtype=np.float64)
    zs = np.ascontiguousarray(np.stack([fr['zs'] for fr in obj.frames]), dtype=np.float64)
    bb = np.ascontiguousarray(np.stack([fr['bbox'] for fr in obj.frames]), dtype=np.float64)
    mkc, msc = np.array(mk, dtype=np.float64), np.array(ms, dtype=np.float64)      # (copies: `mutate` may write into them)
    out = [np.zeros(16), np.zeros((K, 3)), np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.int32), np.zeros(K), np.zeros(16), np.zeros(3), np.zeros((K, 3))]
    st = dict(n=1, keep=[])
    st['tracks'] = (capi.ObjectTrackC * 1)(capi.ObjectTrackC(K, F, None, None, None, capi._d(wTc), capi._d(zs), capi._d(bb) if with_lm else None, None))
    st['results'] = (capi.ObjectInitResult * 1)()
    r = st['results'][0]
    r.wTo, r.kps_world, r.kp_used, r.kp_obs, r.kp_cond = capi._d(out[0]), capi._d(out[1]), capi._i(out[2]), capi._i(out[3]), capi._d(out[4])
    st['cfg_rec'] = capi.ObjectInitConfig(1, 3, 3)
    st['cfg'] = C.pointer(st['cfg_rec'])
    st['mean'] = (capi._dp * 1)(capi._d(mkc))
    st['priors'] = (capi.ObjectLMPrior * 1)(capi.ObjectLMPrior(capi._d(msc), capi._d(mkc)))
    st['lm_results'] = (capi.ObjectLMResult * 1)()
    st['lm_results'][0].wTo, st['lm_results'][0].shape, st['lm_results'][0].kps = capi._d(out[5]), capi._d(out[6]), capi._d(out[7])
    st['lm_cfg_rec'] = capi.ObjectLMConfig(1, 0, (C.c_double * 4)(1, 1, 1, 1), 60, 1e-18)
    st['lm_cfg'] = C.pointer(st['lm_cfg_rec'])
    st['arrays'] = dict(wTc=wTc, mk=mkc, bb=bb)
    mutate(st)
    if with_lm:
        f = lib.orcvio_msckf_object_init_lm
        f.argtypes = [C.c_void_p] * 5 + [C.c_int32] + [C.c_void_p] * 2
        f.restype = C.c_int32
        cast = lambda x: None if x is None else C.cast(x, C.c_void_p)
        rc = f(upd.h, cast(st['cfg']), cast(st['lm_cfg']), cast(st['tracks']), cast(st['priors']), st['n'], cast(st['results']), cast(st['lm_results']))
    else:
        f = lib.orcvio_msckf_object_init
        f.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]
        f.restype = C.c_int32
        cast = lambda x: None if x is None else C.cast(x, C.c_void_p)
        rc = f(upd.h, cast(st['cfg']), cast(st['tracks']), cast(st['mean']), st['n'], cast(st['results']))
    return rc, out


def test_refusals_come_before_anything_runs(upd):
    """K = 0, K = 17, F = 0, F = 129, more tracks than the handle holds, null pointers, a NaN in a camera pose or a mean keypoint,
    pose_form 3, a negative threshold -- and for the one call the optimiser's inputs too: ORCVIO_ERR_INVALID (1) / ORCVIO_ERR_CAPACITY
    (3), the result arrays untouched (nothing was enqueued: a kernel would have written them); the handle serves the next call.  A NaN
    detection is data."""
    obj, ms, mk = oc.one_car(5)
    obj.frames[2]['zs'][3] = np.nan
    INVALID, CAPACITY = 1, 3

    def track(**kw):
        def f(st):
            for k, v in kw.items():
                setattr(st['tracks'][0], k, v)
        return f

    def key(k, v):
        def f(st):
            st[k] = v
        return f

    def poke(name, value):
        def f(st):
            st['arrays'][name].reshape(-1)[-1] = value
        return f

    def cfg(**kw):
        def f(st):
            for k, v in kw.items():
                setattr(st['cfg_rec'], k, v)
        return f

    def result(field):
        def f(st):
            setattr(st['results'][0], field, None)
        return f

    def no_mean(st):
        st['mean'][0] = None
        st['priors'][0].mean_kps = None

    common = [('K = 0', track(n_keypoints=0), INVALID), ('K = 17', track(n_keypoints=17), CAPACITY), ('F = 0', track(n_frames=0), INVALID),
              ('F = 129', track(n_frames=129), CAPACITY), ('more tracks than the handle holds', key('n', 65), CAPACITY),
              ('negative count', key('n', -1), INVALID), ('null config', key('cfg', None), INVALID), ('null tracks', key('tracks', None), INVALID),
              ('null results', key('results', None), INVALID), ('null frame_wTc', track(frame_wTc=None), INVALID),
              ('null frame_zs', track(frame_zs=None), INVALID), ('null mean keypoints', no_mean, INVALID), ('null result wTo', result('wTo'), INVALID),
              ('null result kp_cond', result('kp_cond'), INVALID), ('NaN camera pose', poke('wTc', np.nan), INVALID),
              ('infinite mean keypoint', poke('mk', np.inf), INVALID), ('pose_form 3', cfg(pose_form=3), INVALID),
              ('pose_form -1', cfg(pose_form=-1), INVALID), ('min_obs -1', cfg(min_obs=-1), INVALID), ('min_kps -1', cfg(min_kps=-1), INVALID)]

    def lm_cfg(st):
        st['lm_cfg_rec'].max_iter = 0

    def lm_result(st):
        st['lm_results'][0].kps = None

    def lm_prior(st):
        st['priors'][0].mean_shape = None

    chained = [('null mean keypoint list', key('mean', None), INVALID)], \
              [('null frame_bbox', track(frame_bbox=None), INVALID), ('NaN bbox', poke('bb', np.nan), INVALID), ('max_iter = 0', lm_cfg, INVALID),
               ('null optimiser config', key('lm_cfg', None), INVALID), ('null optimiser result array', lm_result, INVALID),
               ('null mean shape', lm_prior, INVALID), ('null priors', key('priors', None), INVALID), ('null optimiser results', key('lm_results', None), INVALID)]
    for with_lm in (False, True):
        for tag, mutate, want in common + chained[with_lm]:
            rc, out = _raw(upd, obj, ms, mk, mutate, with_lm)
            assert rc == want, (with_lm, tag, rc)
            assert not any(o.any() for o in out), (with_lm, tag)
        rc, out = _raw(upd, obj, ms, mk, lambda st: None, with_lm)
        assert rc == 0 and out[0].any() and out[1].any() and out[5].any() == with_lm
        rc, _ = _raw(upd, obj, ms, mk, key('n', 0), with_lm)   # no tracks: nothing to do
        assert rc == 0
