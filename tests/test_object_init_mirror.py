"""The numpy mirror of the object initialiser (tests/mirror_object_init.py) checked on its own, on the CPU: against its 60-digit
evaluation on the reference's one_car track, the conditioning of the triangulation, the fixture's figures and the reference's own
acceptance bounds, the thresholds and the branch of poseSE32SE2 that measured data cannot reach, the optimiser's optimum from each
pose form, and the host half of the library call (validation, packing) as a stand-alone program under the sanitizers.  The device
(tests/test_gpu_object_init.py) is compared with this mirror."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import mirror_objects as mo
import mirror_object_init as mi
import mirror_object_lm as mlm
import object_lm_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = (4, 5, 47)
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def one_car_mirror(n_frames, pose_form=1):
    """(mirror, 60-digit evaluation) of the first n_frames frames of one_car (computed once per session: do not modify)."""
    obj, _, mk = oc.one_car(n_frames)
    cfg = mi.Config(pose_form=pose_form)
    return mi.solve(obj, mk, cfg), mi.solve_mp(obj, mk, cfg)


def rotation_angle(Ra, Rb):
    T = np.eye(4)
    T[:3, :3] = Ra.T @ Rb
    return float(np.linalg.norm(mo.se3_log(T)[3:]))


@pytest.mark.parametrize('n_frames', FRAMES)
@pytest.mark.parametrize('pose_form', [0, 1, 2])
def test_mirror_matches_the_60_digit_evaluation(n_frames, pose_form):
    """Both stages in float64 against mpmath at 60 digits from the same inputs.  The bound is the forward error of a backward-stable
    least-squares solve and of the SVD behind it: 10 cond(A) eps relative for the triangulated points, and that times the rotation's
    factor sigma_1 / (sigma_2 + d sigma_3) for the pose (entries of size <= ~25).
    Measured (relative, triangulation | absolute, pose forms 0 / 1 / 2):
      47 frames  3.5e-16 | 1.8e-15  1.1e-15  9.0e-16      5 frames  1.0e-14 | 2.8e-14  2.8e-14  2.8e-14
       4 frames  1.8e-14 | 7.2e-14  2.0e-14  7.3e-14"""
    m, ref = one_car_mirror(n_frames, pose_form)
    assert m['status'] == ref['status'] == mi.STATUS_OK and np.array_equal(m['kp_used'], ref['kp_used'])
    e_tri = mi.relative_error(m['kps_world'], ref['kps_world'])
    e_pose = float(np.abs(m['wTo'] - ref['wTo']).max())
    e_lit = max(float(np.abs(m['R'] - ref['R']).max()), float(np.abs(m['t'] - ref['t']).max()), abs(m['scale'] - ref['scale']))
    cond = float(m['kp_cond'].max())
    print('F %d form %d: e_tri %.2e (cond %.1f), e_pose %.2e, e_literal %.2e, ratio %.2f' % (n_frames, pose_form, e_tri, cond, e_pose, e_lit, m['ratio']))
    assert e_tri <= 10 * cond * EPS
    scale = float(np.abs(ref['kps_world']).max())
    assert e_pose <= 10 * cond * EPS * scale * m['ratio'] and e_lit <= 10 * cond * EPS * scale * m['ratio']
    assert float(np.abs(m['sigma'] - ref['sigma']).max()) <= 1e-6 * ref['sigma'][0]


def test_conditioning_of_the_triangulation_on_one_car():
    """cond(A) per keypoint and the distance between the normal equations and lstsq, measured with numpy: 47 frames cond 4.02-12.55,
    5 frames 86.2-151.7, 4 frames 134.6-217.9 (4.0-12.6, 86-152, 135-218 to the digits they are quoted with); normal equations
    against lstsq, per keypoint relative to its largest coordinate, 7.1e-16 at 47 frames, 1.0e-12 at 5, 2.3e-12 at 4 -- a figure
    that moves with the LAPACK build (1.5e-12 and 2.4e-15 have been seen for 4 and 47 frames), so what is asserted is its bound
    cond(A)^2 eps with the project's factor ten.  Every case the device is checked on keeps cond(A) and
    sigma_1 / (sigma_2 + d sigma_3) below 1e4, where its tolerance would reach the project's bar of 1e-6."""
    want = {47: (4.0, 12.6), 5: (86.0, 152.0), 4: (135.0, 218.0)}
    for n_frames, (lo, hi) in want.items():
        obj, _, mk = oc.one_car(n_frames)
        m = one_car_mirror(n_frames)[0]
        mn = mi.solve(obj, mk, mi.Config(), normal_equations=True)
        d = max(float(np.abs(mn['kps_world'][k] - m['kps_world'][k]).max() / np.abs(m['kps_world'][k]).max()) for k in range(12))
        print('F %d: cond %.2f .. %.2f, normal equations vs lstsq %.2e, ratio %.2f' % (n_frames, m['kp_cond'].min(), m['kp_cond'].max(), d, m['ratio']))
        assert lo - 0.5 <= m['kp_cond'].min() and m['kp_cond'].max() <= hi + 0.5     # (the quoted digits)
        assert m['kp_cond'].max() < 1e4 and m['ratio'] < 1e4
        assert d <= 10 * m['kp_cond'].max() ** 2 * EPS       # the forward-error bound the device's tolerance uses


def test_fixture_values_and_the_references_bounds():
    """one_car at 47 frames: all 12 keypoints detected in every frame, scale 1.308, sigma 22.97 / 4.27 / 2.42; against the fixture's
    wTq the Kabsch rotation is 0.0020 rad away (geodesic angle) and the literal translation 0.189, inside the reference test's 0.5 rad
    and 0.35 (src/tests/test_object_init_multiframe.cpp:76-79).  The three pose forms (rotation angle to wTq's | translation distance):
      form 0 (rigid SE(3))      0.0020 rad | 0.195       form 2 (yaw = atan2)     0.057 rad | 0.710
      form 1 (yaw = pi / atan2) 0.230 rad  | 0.710   (its yaw is pi / -1.664 = -1.888 where atan2 gives -1.664; forms 1 and 2 put z = 0)
    The forms are recorded, not bounded: only the Kabsch result is what the reference's test looks at."""
    m = one_car_mirror(47)[0]
    Tq = oc.one_car_truth()
    assert np.array_equal(m['kp_obs'], np.full(12, 47)) and np.array_equal(m['kp_used'], np.ones(12)) and m['n_used'] == 12
    assert abs(m['scale'] - 1.308) < 5e-4
    assert np.abs(m['sigma'] - [22.97, 4.27, 2.42]).max() < 5e-3
    dR, dt = rotation_angle(Tq[:3, :3], m['R']), float(np.linalg.norm(m['t'] - Tq[:3, 3]))
    print('R_kabsch %.4f rad, t_kabsch %.3f from wTq; literal matrix scale %.4f' % (dR, dt, m['scale']))
    assert dR < 0.5 and dt < 0.35
    assert dR < 0.0025 and abs(dt - 0.189) < 5e-4
    for form in (0, 1, 2):
        T = one_car_mirror(47, form)[0]['wTo']
        a, d = rotation_angle(Tq[:3, :3], T[:3, :3]), float(np.linalg.norm(T[:3, 3] - Tq[:3, 3]))
        print('form %d: %.4f rad, %.3f' % (form, a, d))
        assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() < 1e-14 and np.array_equal(T[3], [0, 0, 0, 1])
    L = mi.literal_matrix(m)
    assert abs(np.linalg.det(L[:3, :3]) - m['scale'] ** 3) < 1e-12        # the reference's return value is not rigid


def test_thresholds_are_strict_and_the_chords_run_over_the_used_list():
    """A keypoint with exactly min_obs detections is not used, one with min_obs + 1 is; exactly min_kps used keypoints is status 2
    and the identity, min_kps + 1 is status 1; with used ids 1, 4, 6, 11 the scale is the chord ratio over that list."""
    obj, _, mk = oc.one_car(6)
    for fr in obj.frames:
        fr['zs'][[0, 2, 3, 5, 7, 8, 9, 10]] = np.nan
    for f in range(3, 6):
        obj.frames[f]['zs'][4] = np.nan          # 3 detections = min_obs: out
    obj.frames[0]['zs'][6] = np.nan
    obj.frames[5]['zs'][6, 1] = np.nan           # one coordinate is enough: 4 detections = min_obs + 1: in
    m = mi.solve(obj, mk)
    assert list(m['kp_obs']) == [0, 6, 0, 0, 3, 0, 4, 0, 0, 0, 0, 6] and list(np.flatnonzero(m['kp_used'])) == [1, 6, 11]
    assert m['status'] == mi.STATUS_TOO_FEW and np.array_equal(m['wTo'], np.eye(4)) and m['n_used'] == 3
    for f in range(3, 6):
        obj.frames[f]['zs'][4] = oc.one_car(6)[0].frames[f]['zs'][4]
    m = mi.solve(obj, mk)
    ids = [1, 4, 6, 11]
    assert list(np.flatnonzero(m['kp_used'])) == ids and m['status'] == mi.STATUS_OK
    P = m['kps_world']
    chord = lambda X: sum(np.linalg.norm(X[b] - X[a]) for a, b in zip(ids[:-1], ids[1:]))
    assert abs(m['scale'] - chord(P) / chord(mk)) <= 4 * EPS * m['scale']
    assert np.all(np.isnan(P[[0, 2, 3, 5, 7, 8, 9, 10]])) and np.all(np.isfinite(P[ids]))


def test_pose_form_1_takes_yaw_zero_when_the_quotient_is_not_finite():
    """poseSE32SE2's `if (!std::isfinite(yaw)) yaw = 0`: atan2 = 0 exactly (R = identity) makes pi / atan2 infinite.  Measured data
    does not get there, so the device test does not either."""
    T = mi.pose_from_literal(np.eye(3), np.array([1.0, 2.0, 3.0]), 1.3, np.zeros(3), np.zeros(3), 1)
    want = np.eye(4)
    want[:2, 3] = [1.0, 2.0]
    assert np.array_equal(T, want)
    R = mo.se3_exp(np.array([0, 0, 0, 0, 0, 0.7]))[:3, :3]
    T1 = mi.pose_from_literal(R, np.zeros(3), 1.3, np.zeros(3), np.zeros(3), 1)
    T2 = mi.pose_from_literal(R, np.zeros(3), 1.3, np.zeros(3), np.zeros(3), 2)
    assert abs(np.arctan2(T2[1, 0], T2[0, 0]) - 0.7) < 1e-15
    y1 = np.pi / 0.7
    assert np.abs(T1[:2, :2] - [[np.cos(y1), -np.sin(y1)], [np.sin(y1), np.cos(y1)]]).max() < 1e-14


@pytest.mark.parametrize('name', ['f47', 'f33'])
def test_the_optimiser_reaches_its_optimum_from_every_pose_form(name):
    """End to end with the optimiser's mirror: from the start of each pose form (the pose, the mean shape, the mean keypoints), both
    charts, at the reference's weights, every run ends with status 1 at the optimum of case_spread(name)'s first run, within ten times
    that case's own spread (the optimiser's existing tolerance: 4.8e-9 at 47 frames, 2.9e-8 at 33).
    Measured: 47 frames cost 0.6418765004636, 3.5e-11 .. 2.9e-10 away; 33 frames cost 0.1988724233842, 1.6e-11 .. 1.9e-9."""
    c = oc.CASES[name]
    spread, runs = oc.case_spread(name)
    obj, ms, mk = oc.one_car(c['n_frames'])
    dist = []
    for form in (0, 1, 2):
        init = mi.solve(obj, mk, mi.Config(pose_form=form))
        assert init['status'] == mi.STATUS_OK
        start = type(obj)(wTo=init['wTo'], shape=ms.copy(), kps=mk.copy(), frames=obj.frames)
        for left in (True, False):
            r = mlm.solve(start, ms, mk, mlm.Config(left=left, new_bbox=c['new_bbox'], weights=c['weights']))
            assert r['status'] == mlm.STATUS_CONVERGED
            dist.append(oc.distance(r, runs[0]))
            assert abs(r['cost'] - runs[0]['cost']) <= 1e-9 * runs[0]['cost']
    print('%s: cost %.13g, distance to the first run %.2e .. %.2e, tolerance %.2e' % (name, runs[0]['cost'], min(dist), max(dist), 10 * spread))
    assert max(dist) <= 10 * spread


def test_pack_and_validation_under_the_sanitizers(tmp_path):
    """Validation and packing of both entry points as a stand-alone program (its own main) under AddressSanitizer and
    UndefinedBehaviorSanitizer: every refusal, NULL optional pointers, the offsets of a mixed batch."""
    exe = str(tmp_path / 'test_object_init_pack')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_object_init_pack.cpp')])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'object init pack ok' in out.stdout


def test_the_library_exports_the_initialiser(built):
    from orcvio_amd import capi
    lib = capi.load()
    for name in ('orcvio_msckf_object_init', 'orcvio_msckf_object_init_lm', 'orcvio_msckf_object_init_config_default'):
        assert hasattr(lib, name) and name in capi.EXPORTS
    cfg = capi.ObjectInitConfig()
    lib.orcvio_msckf_object_init_config_default(__import__('ctypes').byref(cfg))
    assert (cfg.pose_form, cfg.min_obs, cfg.min_kps) == (1, 3, 3)
