"""CPU tests of the marginal read's cases and checker (tests/cov_marginal_cases.py): the float64 restatement stays inside the derived bar
on every case, the literal getPpose / getPvel agree with the 9 x 9 the one spec builds, every planted error fails its check -- so a
device result that passes the same checker (tests/test_gpu_cov_marginal.py) has not made one of them.  And the HIP-free header the
library validates a request with (orcvio_amd/csrc/host/cov_marginal_spec.hpp) under the address and undefined-behaviour sanitizers, as
a stand-alone program (tests/cpp/cov_marginal_spec_main.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import cov_marginal_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('case', mc.shape_cases(), ids=repr)
def test_the_float64_restatement_stays_inside_the_bar(case):
    frac = mc.check(case, mc.restate(case.P, case.idx, case.T))
    print('FIG %r fraction of the bar %.3f' % (case, frac))


@pytest.mark.parametrize('case', mc.kind_cases(34), ids=repr)
def test_every_kind_of_idx_and_of_P(case):
    assert case.idx.min() >= 0 and case.idx.max() < case.n and len(case.idx) == case.k
    if case.idx_kind == 'ends':
        assert 0 in case.idx and case.n - 1 in case.idx
    if case.idx_kind == 'repeat':
        assert len(set(case.idx.tolist())) < case.k
    if case.idx_kind == 'reversed':
        assert np.all(np.diff(case.idx) < 0)
    assert not np.array_equal(case.P, case.P.T)
    mc.check(case, mc.restate(case.P, case.idx, case.T))


def test_graded_P_spans_fourteen_decades():
    P = mc.make_P(73, 'graded')
    scale = np.sqrt(np.mean(P * P, axis=1) * np.mean(P * P, axis=0))   # ~ d_i
    assert scale.max() / scale.min() > 1e12
    assert not np.array_equal(P, P.T)


@pytest.mark.parametrize('n,p_kind', [(34, 'asym'), (73, 'graded'), (154, 'graded')])
def test_the_literal_getters_agree_with_the_spec_built_block(n, p_kind):
    c = mc.odometry_case(n, p_kind, seed=n)
    pose, vel = mc.literal_getters(c.P, c.R)
    frac = mc.check_getters(c, pose, vel)
    out = mc.restate(c.P, c.idx, c.T)
    mc.check(c, out)
    print('FIG getters n=%d %s fraction of the bar %.3f' % (n, p_kind, frac))
    # the order {0..2, 6..8} in place of {6..8, 0..2}: orientation first is not getPpose()'s matrix
    idx_bad, T = mc.odometry_spec(c.R, order=(0, 1, 2, 6, 7, 8, 3, 4, 5))
    bad = mc.restate(c.P, idx_bad, T)
    with pytest.raises(AssertionError):
        mc.check_getters(c, bad[0:6, 0:6], bad[6:9, 6:9])
    assert not mc.passes(c, bad)
    # ... and the getters read P_po and P_op separately: on an asymmetric P their matrix is not symmetric
    assert not np.array_equal(pose, pose.T)


@pytest.mark.parametrize('kind', mc.PLANTED)
@pytest.mark.parametrize('p_kind', mc.P_KINDS)
def test_every_planted_error_fails_its_check(kind, p_kind):
    c = mc.shape_case(34, 9, 9, 'permuted', p_kind)
    assert mc.passes(c, mc.restate(c.P, c.idx, c.T))
    assert not mc.passes(c, mc.planted(c, kind)), kind
    if kind in ('idx_rows_only', 'Pm_transposed'):   # ... and as gathers, where the check is bit for bit
        g = mc.shape_case(34, 9, 0, 'permuted', p_kind)
        assert mc.passes(g, mc.restate(g.P, g.idx))
        assert not mc.passes(g, mc.planted(g, kind)), kind


def test_one_ulp_outside_the_bar_fails_and_the_rounded_exact_value_passes():
    c = mc.shape_case(34, 9, 6, 'ascending', 'asym')
    best =np.array([[float(v) for v in row] for row in c.exact])
    assert mc.check(c, best) <= 1.0 / (2 * 9 + 4) + 1e-12   # (half an ulp of the value is no more than u |value| <= the bar / 22)
    off = best.copy()
    off[2, 3] += 1.5 * c.bound[2, 3]
    assert not mc.passes(c, off)


def test_the_spec_header_under_the_sanitizers(tmp_path):
    """the argument validation and the odometry spec builder as a stand-alone program, -fsanitize=address,undefined, run directly"""
    exe = str(tmp_path / 'cov_marginal_spec_main')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'cov_marginal_spec_main.cpp')])
    R = mc.rotation(5)
    run = subprocess.run([exe] + [repr(float(v)) for v in R.ravel()], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == 'cov marginal spec ok', run.stdout
    idx = np.array(lines[0].split()[1:], dtype=np.int32)
    T = np.array(lines[1].split()[1:], dtype=np.float64).reshape(9, 9)
    ref_idx, ref_T = mc.odometry_spec(R)
    assert np.array_equal(idx, ref_idx) and np.array_equal(T, ref_T)
