"""The check of the clones that leave on the CPU: the numpy mirror (tests/mirror_clone_choice.py) against the same formulas in 60
digits; every case of tests/clone_choice_cases.py clear of its thresholds; the four branch patterns at N = 6, 7, 20; the mistakes the
case set must be able to see; and the shared host/device header (host/clone_choice_model.hpp) as a stand-alone program under the
sanitizers, on the case set."""
import os
import subprocess

import numpy as np
import pytest

import clone_choice_cases as cc
import mirror_clone_choice as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_mirror_against_60_digits():
    """angle and distance of every compared clone of every case, on the post-update records (the whole chain from the double inputs:
    exp, the body pose's increment, the extrinsic's, the camera record, the quaternion, atan2) and on the records as given"""
    worst = dict(angle=0.0, distance=0.0)
    for nm in cc.names():
        c = cc.case(nm)
        for applied in (True, False):
            run = mc.evaluate(c, c['dx_ref'], applied)
            for i, cl in enumerate(run['compared']):
                a, d = mc.quantities_mp(c['w'], c['dx_ref'], c['ext'], c['left'], cl, c['N'] - 4, applied, c['cam_pre'])
                worst['angle'] = max(worst['angle'], abs(run['angle'][i] - a) / a)
                worst['distance'] = max(worst['distance'], abs(run['distance'][i] - d) / d)
    print('mirror against 60 digits, largest relative distance: angle %.3e (recorded %.1e), distance %.3e (recorded %.1e)' %
          (worst['angle'], cc.ANGLE_SPREAD, worst['distance'], cc.DISTANCE_SPREAD))
    # the recorded spreads the GPU test's bars are ten times of are the ones measured here
    assert cc.ANGLE_SPREAD / 2 <= worst['angle'] <= cc.ANGLE_SPREAD * 2
    assert cc.DISTANCE_SPREAD / 2 <= worst['distance'] <= cc.DISTANCE_SPREAD * 2


def test_every_case_is_clear_of_its_thresholds_and_is_what_it_says():
    seen = set()
    for nm in cc.names():
        c = cc.case(nm)
        for applied in (True, False):
            run = mc.evaluate(c, c['dx_ref'], applied)
            for a, d in zip(run['angle'], run['distance']):
                assert abs(a - c['rot_thr']) >= cc.MARGIN * max(1.0, c['rot_thr']), nm
                assert abs(d - c['trans_thr']) >= cc.MARGIN * max(1.0, c['trans_thr']), nm
        post, pre = mc.evaluate(c, c['dx_ref'], True), mc.evaluate(c, c['dx_ref'], False)
        assert tuple(post['taken']) == c['pattern'] and post['chosen'] == c['truth'] and pre['chosen'] == c['predicted'], nm
        assert pre['agree'] == 1 and post['agree'] == int(c['agree']) == int(c['truth'] == c['predicted']), nm
        assert c['truth'] in cc.possible_sets(c['N']) and c['predicted'] in cc.possible_sets(c['N']), nm
        assert 10 <= c['first'].F <= 40 and 5 <= cc.prune_for(c, c['predicted']).F <= 20 and 5 <= cc.prune_for(c, c['truth']).F <= 20, nm
        seen.add((c['N'], c['pattern'], c['agree']))
    # all four branch patterns, agreeing and disagreeing, at N = 6, 7, 20
    assert {(N, p, a) for N in (6, 7, 20) for p in cc.PATTERNS.values() for a in (True, False)} <= seen
    N = 20
    want = {(1, 1): [N - 3, N - 2], (1, 0): [0, N - 3], (0, 1): [0, N - 5], (0, 0): [0, 1]}
    for p, s in want.items():
        assert cc.case('n20_%d%d_agree' % p)['truth'] == s


@pytest.mark.parametrize('mutation', mc.MUTATIONS)
def test_the_case_set_sees_each_mistake(mutation):
    """comparing N-4 or N-3 instead of N-5 after a first iteration that was not taken; R K instead of R^T K; the clone's frozen
    extrinsic instead of the IMU state's incremented one; pre-update instead of post-update poses; an unsorted result; tracking_ok
    ignored: each changes chosen / compared / taken, or moves angle or distance by more than a hundred times the GPU test's bar, on at
    least one case"""
    caught = []
    for nm in cc.names():
        c = cc.case(nm)
        good, bad = mc.evaluate(c, c['dx_ref'], True), mc.evaluate(c, c['dx_ref'], True, mutation)
        moved = any(good[k] != bad[k] for k in ('chosen', 'compared', 'taken'))
        if not moved:
            e_a = max(abs(a - b) / a for a, b in zip(good['angle'], bad['angle']))
            e_d = max(abs(a - b) / a for a, b in zip(good['distance'], bad['distance']))
            moved = e_a > 1000 * cc.ANGLE_SPREAD or e_d > 1000 * cc.DISTANCE_SPREAD
        if moved:
            caught.append(nm)
    print(mutation, 'caught by', len(caught), 'cases:', caught[:6])
    assert caught


@pytest.fixture(scope='module')
def model_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('cch') / 'test_clone_choice_model')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_clone_choice_model.cpp')])
    return exe


def test_host_header_edge_inputs_under_the_sanitizers(model_exe):
    out = subprocess.run([model_exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'clone choice model ok' in out.stdout


def _run(model_exe, path, c, applied):
    head = [c['N'], c['rot_thr'], c['trans_thr'], c['tracking_ok'], c['predicted'][0], c['predicted'][1], int(applied)]
    if applied:   # the body poses and the extrinsic as the increment leaves them: clone_choice_cam_pose makes the records
        w, dx, leg = c['w'], c['dx_ref'], c['w'].flags.leg_dim
        rec = []
        for i in range(c['N']):
            da = dx[leg + 6 * i: leg + 6 * i + 6]
            E = mc.so3_exp(da[:3])
            rec += list((E @ w.R_b2w[i] if c['left'] else w.R_b2w[i] @ E).ravel()) + list(w.t_b_w[i] + da[3:])
        Re, te = mc.extrinsic_increment(dx[15:21], c['ext'][0], c['ext'][1])
        vals = head + rec + list(Re.ravel()) + list(te)
    else:
        vals = head + list(c['cam_pre'].ravel())
    with open(path, 'w') as f:
        f.write(' '.join(repr(float(v)) for v in vals))
    out = subprocess.run([model_exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    t = out.stdout.split()
    return dict(evaluated=int(t[0]), agree=int(t[1]), chosen=[int(t[2]), int(t[3])], compared=[int(t[4]), int(t[5])], taken=[int(t[6]), int(t[7])],
                angle=[float(t[8]), float(t[9])], distance=[float(t[10]), float(t[11])])


def test_host_header_equals_the_mirror_on_every_case(model_exe, tmp_path):
    """the shared header is the arithmetic k_clone_choice runs: here on the host, on the post-update records (through its own camera
    record) and on the records as given"""
    worst = [0.0, 0.0]
    for nm in cc.names():
        c = cc.case(nm)
        for applied in (True, False):
            got, want = _run(model_exe, str(tmp_path / 'case.txt'), c, applied), mc.evaluate(c, c['dx_ref'], applied)
            assert got['evaluated'] == 1
            for k in ('chosen', 'compared', 'taken', 'agree'):
                assert got[k] == want[k], (nm, applied, k)
            worst[0] = max(worst[0], max(abs(a - b) / b for a, b in zip(got['angle'], want['angle'])))
            worst[1] = max(worst[1], max(abs(a - b) / b for a, b in zip(got['distance'], want['distance'])))
    print('host header against the mirror: angle %.2e (bar %.1e), distance %.2e (bar %.1e)' % (worst[0], 10 * cc.ANGLE_SPREAD, worst[1], 10 * cc.DISTANCE_SPREAD))
    assert worst[0] <= 10 * cc.ANGLE_SPREAD and worst[1] <= 10 * cc.DISTANCE_SPREAD
