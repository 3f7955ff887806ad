"""GPU test of the C++ host layer's MsckfBackend::checkZuptImu as a filter calls it (tests/cpp/test_host_zupt_check.cpp: a program of its
own, linked against the product library): on the mirror's containers, first on the host's own covariance -- the Woodbury fall-back of
the header the kernel is built from -- then with the covariance resident, against the reference's dense form
(tests/mirror_zupt_check.py) with the bar of tests/test_gpu_zupt_check.py."""
import os
import subprocess

import numpy as np
import pytest

import mirror_zupt_check as mz
import zupt_check_cases as zc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def exe(built, tmp_path_factory):
    out = str(tmp_path_factory.mktemp('zchk_host') / 'test_host_zupt_check')
    libdir = os.path.join(ROOT, 'orcvio_amd', 'lib')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-Wall', '-o', out, os.path.join(ROOT, 'tests', 'cpp', 'test_host_zupt_check.cpp'),
                           '-L', libdir, '-lorcvio_msckf', '-Wl,-rpath,' + libdir])
    return out


def _run(exe, tmp_path, case, **over):
    k = dict(case['consts'], **over)
    vals = [float(case['left']), k['sigma_w2'], k['sigma_a2'], k['sigma_wb'], k['sigma_ab'], k['chi2_prob'], k['chi2_multiplier'], k['max_velocity']]
    vals += list(case['R'].ravel()) + list(case['v']) + list(case['ba']) + list(case['g'])
    vals += [float(case['P'].shape[0])] + list(case['P'].ravel()) + [float(case['samples'].shape[0])] + list(case['samples'].ravel())
    p = str(tmp_path / 'case.txt')
    with open(p, 'w') as f:
        f.write(' '.join(repr(float(v)) for v in vals))
    out = subprocess.run([exe, p], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    res = {}
    for line in out.stdout.strip().splitlines():
        w = line.split()
        res[w[0]] = dict(status=int(w[1]), evaluated=int(w[2]), do_zupt=int(w[3]), dof=int(w[4]), chi2=float(w[5]), chi2_check=float(w[6]), speed=float(w[7]))
    return res


@pytest.mark.parametrize('name', ['S2_left', 'S65_right', 'n154_S128', 'large_S2', 'corr_S5', 'pair_S10_left_below', 'pair_S10_left_above', 'speed_above'])
def test_both_routes_of_the_host_layer_against_the_dense_form(exe, tmp_path, name):
    case = zc.case(name)
    ref, dof = mz.dense(case)
    got = _run(exe, tmp_path, case)
    for route in ('host', 'device'):
        g = got[route]
        err = abs(g['chi2'] - ref) / ref
        print('%s %s: chi2 %.10g dense %.10g  %.2e (bar %.1e)' % (name, route, g['chi2'], ref, err, zc.CHI2_BAR))
        assert (g['status'], g['evaluated'], g['dof']) == (0, 1, dof)
        assert err <= zc.CHI2_BAR
        assert g['do_zupt'] == int(mz.decide(case, ref, dof))
    assert got['host']['chi2_check'] == got['device']['chi2_check'] and got['host']['speed'] == got['device']['speed']


def test_both_routes_refuse_and_validate_alike(exe, tmp_path):
    case = zc.case('S5_right')
    smp = case['samples']
    P_nan = case['P'].copy(); P_nan[2, 14] = np.nan
    P_neg = case['P'].copy(); P_neg[9, 9] = -1e-4
    dt0 = smp.copy(); dt0[2, 0] = dt0[1, 0]
    for what, kw, over, expect in (('one sample', dict(samples=smp[:1]), {}, (0, 0, 0)),
                                   ('nan in the marginal', dict(P=P_nan), {}, (6, 0, 0)),
                                   ('negative diagonal', dict(P=P_neg), {}, (6, 0, 0)),
                                   ('dt = 0', dict(samples=dt0), {}, (1, 0, 0)),
                                   ('129 samples', dict(samples=zc.make_case(129, seed=1)['samples']), {}, (3, 0, 0)),
                                   ('a variance of zero', {}, dict(sigma_a2=0.0), (1, 0, 0)),
                                   ('chi2_prob = 1', {}, dict(chi2_prob=1.0), (1, 0, 0))):
        got = _run(exe, tmp_path, dict(case, **kw), **over)
        for route in ('host', 'device'):
            g = got[route]
            assert (g['status'], g['evaluated'], g['do_zupt']) == expect, (what, route, g)
