"""The zero-velocity check's two forms on the CPU (tests/mirror_zupt_check.py): the device's 9 x 9 form against the reference's dense one
and both against 60-digit arithmetic; the mistakes the case set must be able to see; the distance of every case from its threshold; the
chi-square quantile at the check's degrees of freedom; and the shared host header (packing, validation, the Woodbury fall-back) as a
stand-alone program under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import mirror_zupt_check as mz
import zupt_check_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def figures():
    """per case: dense chi2, dof, the 9 x 9 form's chi2, c, the 60-digit value -- computed once"""
    out = {}
    for nm in zc.names():
        c = zc.case(nm)
        d, dof = mz.dense(c)
        w, cc, _ = mz.woodbury(c)
        out[nm] = dict(dense=d, dof=dof, woodbury=w, c=cc, mp=mz.chi2_mp(c))
    return out


def test_the_two_forms_agree_with_each_other_and_with_60_digits(figures):
    worst_dense = worst_w = 0.0
    for nm, f in figures.items():
        e_d, e_w = abs(f['dense'] - f['mp']) / f['mp'], abs(f['woodbury'] - f['mp']) / f['mp']
        print('%-20s chi2 %.6g  c/chi2 %.2e  dense-mp %.2e  woodbury-mp %.2e' % (nm, f['dense'], f['c'] / f['dense'], e_d, e_w))
        worst_dense, worst_w = max(worst_dense, e_d), max(worst_w, e_w)
        assert e_w <= zc.CHI2_BAR, nm
        assert abs(f['woodbury'] - f['dense']) / f['dense'] <= zc.CHI2_BAR, nm
    print('largest dense-mp %.3e (recorded %.1e), largest woodbury-mp %.3e, bar %.1e' % (worst_dense, zc.DENSE_SPREAD, worst_w, zc.CHI2_BAR))
    # the recorded spread the bar is ten times of is the one measured here (numpy's LAPACK may move it a little, not by a factor of two)
    assert zc.DENSE_SPREAD / 2 <= worst_dense <= zc.DENSE_SPREAD * 2


def test_the_60_digit_yardstick_does_not_rest_on_the_identity_under_test():
    """where S of order 6 m can be factored in 60 digits (pure Python: up to a few dozen rows) it gives the very same double as the 9 x 9
    identity evaluated in 60 digits"""
    for nm in zc.names():
        c = zc.case(nm)
        if c['S'] <= 5:
            assert mz.chi2_mp(c, 'dense') == mz.chi2_mp(c, 'woodbury'), nm


@pytest.mark.parametrize('mutation', mz.MUTATIONS)
def test_the_case_set_sees_each_mistake(figures, mutation):
    """gyro rows dropped from A; sigma_wb / sigma_ab squared; dt from processModel's interval; left and right J exchanged; the velocity
    rows of P in place of b_g: each moves chi2 by more than the GPU test's tolerance on at least one case"""
    # (on the dense form: a mistaken marginal need not be positive definite, and S = H P_m H^T + R still is)
    moved = max(abs(mz.dense(zc.case(nm), mutation)[0] - f['dense']) / f['dense'] for nm, f in figures.items())
    print('%s: chi2 moves by up to %.2e (bar %.1e)' % (mutation, moved, zc.CHI2_BAR))
    assert moved > 100 * zc.CHI2_BAR


def test_one_triangle_of_the_marginal_is_not_enough():
    """The check reads both triangles of the marginal and averages them.  On a symmetric P a form that mirrors one triangle gives the same
    number, so this mistake needs an input of its own: the marginal with one triangle perturbed.  (No symmetric 9 x 9 form equals the
    dense one there -- Eigen's llt reads the LOWER triangle of S = H P_m H^T + R, which is neither triangle of P_m -- so the case is not
    in the set the forms are compared on; tests/test_gpu_zupt_check.py runs it on the device against the averaged marginal.)"""
    c = dict(zc.case('S5_right'))
    P = c['P'].copy()
    P[0, 12] *= 1.0 + 1e-3
    P[1, 9] += 1e-6
    both = mz.woodbury(dict(c, P=P))[0]
    for tri in (np.triu, np.tril):
        Pm = tri(P) + tri(P, 0).T - np.diag(np.diag(P))
        one = mz.woodbury(dict(c, P=Pm))[0]
        assert abs(one - both) / both > 100 * zc.CHI2_BAR


def test_every_case_is_clear_of_its_threshold(figures):
    """at least 1e-6 relative: the condition under which the accept bit is compared for ALL cases"""
    sides = {}
    for nm, f in figures.items():
        thr = mz.threshold(zc.case(nm), f['dof'])
        assert abs(f['dense'] - thr) / thr >= 1e-6, nm
        sides[nm] = f['dense'] > thr
    for base in zc.PAIRS:
        assert not sides[base + '_below'] and sides[base + '_above'], base
    # the speed pair passes chi2 and differs in the speed test alone
    a, b = zc.case('speed_below'), zc.case('speed_above')
    assert mz.decide(a, figures['speed_below']['dense'], figures['speed_below']['dof']) and not mz.decide(b, figures['speed_above']['dense'], figures['speed_above']['dof'])
    assert not sides['speed_above']


def test_chi2_quantile_at_the_checks_degrees_of_freedom(built):
    """dof = 6 .. 762 in steps of 6 (S = 2 .. 128), within what test_abi's table comparison allows below 500"""
    from orcvio_amd import capi
    try:
        from scipy.stats import chi2
        ref = lambda dof: float(chi2.ppf(0.95, dof))
    except ImportError:
        from oracle import oracle
        ref = lambda dof: float(oracle.chi2_quantile(dof, 0.95))
    for dof in range(6, 763, 6):
        r = ref(dof)
        assert abs(capi.chi2_quantile(dof, 0.95) - r) / r < 1e-12, dof


def _write_case(path, c):
    k = c['consts']
    vals = [float(c['left']), k['sigma_w2'], k['sigma_a2'], k['sigma_wb'], k['sigma_ab']] + list(c['R'].ravel()) + list(c['ba']) + list(c['g'])
    vals += [float(c['n'])] + list(c['P'].ravel()) + [float(c['S'])] + list(c['samples'].ravel())
    with open(path, 'w') as f:
        f.write(' '.join(repr(float(v)) for v in vals))


@pytest.fixture(scope='module')
def model_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('zchk') / 'test_zupt_check_model')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_zupt_check_model.cpp')])
    return exe


def test_host_header_edge_inputs_under_the_sanitizers(model_exe):
    out = subprocess.run([model_exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'zupt check model ok' in out.stdout


def test_host_header_equals_the_dense_form_on_every_case(model_exe, figures, tmp_path):
    """the shared header is the arithmetic k_zupt_check runs: here on the host, its sums in row order, against the reference's form"""
    worst = 0.0
    for nm, f in figures.items():
        p = str(tmp_path / 'case.txt')
        _write_case(p, zc.case(nm))
        out = subprocess.run([model_exe, p], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (nm, out.stdout + out.stderr)
        st, chi2, c, dts = out.stdout.split()
        e = abs(float(chi2) - f['dense']) / f['dense']
        worst = max(worst, e)
        assert int(st) == 0 and e <= zc.CHI2_BAR, (nm, e)
        assert abs(float(c) - f['c']) / f['c'] < 1e-13 and abs(float(dts) - np.sum(np.diff(zc.case(nm)['samples'][:, 0]))) < 1e-13
    print('host header against the dense form: %.2e (bar %.1e)' % (worst, zc.CHI2_BAR))


def test_the_programs_literal_dense_form_is_the_mirrors(model_exe, figures, tmp_path):
    """the plain C++ restatement of the reference's dense test that scripts/gpu_zupt_check_timing.py times as the parent's route"""
    for nm in ('S5_left', 'S65_right', 'large_S2'):
        p = str(tmp_path / 'case.txt')
        _write_case(p, zc.case(nm))
        out = subprocess.run([model_exe, p, 'dense', '1'], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (nm, out.stdout + out.stderr)
        chi2 = float(out.stdout.split()[0])
        assert abs(chi2 - figures[nm]['dense']) / figures[nm]['dense'] <= zc.CHI2_BAR, nm
