"""The host build of orcvio_amd/csrc/host/imu_model.hpp as a stand-alone program (tests/cpp/imu_model_main.cpp) under
AddressSanitizer and UndefinedBehaviorSanitizer, against the numpy restatement tests/mirror_imu.py: sample selection, the propagated
state, every per-sample Phi_k / Q_k and the accumulated pair."""
import os
import subprocess

import numpy as np
import pytest

import imu_cases as ic
import mirror_imu as mi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The predictors of the header and of the mirror run the same scalar IEEE operations in the same order: the propagated state is compared
# bit for bit.  Phi_k, Q_k and the accumulated pair are evaluated with different association (the header's plain loops and
# Q_k = Phi_k (G Q_c G^T dt) Phi_k^T against the mirror's numpy `@`): a few ulp per 3 x 3 product, relative to the block's largest
# entry.  64 eps = 1.4e-14 per sample; the accumulated pair compounds over S samples, bounded by S times that.
EPS = 2.220446049250313e-16
PER_SAMPLE = 64 * EPS


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('imu') / 'imu_model_main')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', out, os.path.join(ROOT, 'tests', 'cpp', 'imu_model_main.cpp')])
    return out


def run_program(exe, case, tmp_path):
    path = str(tmp_path / 'case.txt')
    ic.write_case(path, case)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    res = {'phik': [], 'qk': [], 'rec': []}
    for line in out.stdout.splitlines():
        tag, *rest = line.split()
        if tag in ('phik', 'qk', 'rec'):
            res[tag].append(np.array([float(x) for x in rest]))
        elif tag in ('imu', 'capacity'):
            res[tag] = rest
        else:
            res[tag] = np.array([float(x) for x in rest])
    return res


@pytest.mark.parametrize('flag_set', list(ic.FLAG_SETS))
@pytest.mark.parametrize('S,rate', [(1, 200.0), (5, 250.0), (33, 650.0)])
def test_program_equals_the_mirror(exe, tmp_path, flag_set, S, rate):
    case = ic.make_case(flag_set, S, n=22, seed=3, rate=rate, skipped=2, beyond=3)
    srv, info = ic.run_mirror(case, with_P=False)
    got = run_program(exe, case, tmp_path)
    assert 'imu' in got   # ("imu model ok")
    assert [int(got['info'][0]), int(got['info'][1])] == [info['n_used'], info['n_propagated']] == [S + 2, S]
    assert got['info'][2] == info['dt']
    np.testing.assert_allclose(got['info'][3:6], info['mean_sforce'], rtol=4 * EPS)
    assert got['time'][0] == srv.imu.time
    # the state: bit for bit (see above; tests/test_gpu_imu.py's bar rests on it)
    for name, ref in (('R', srv.imu.R.ravel()), ('v', srv.imu.v), ('p', srv.imu.p), ('v_fej', srv.fej_now.v), ('p_fej', srv.fej_now.p)):
        assert np.array_equal(got[name], ref), name
    assert np.array_equal(got['prev'], case['samples'][S + 1, 1:7])
    worst = 0.0
    for k, step in enumerate(srv.steps):
        e1 = ic.block_error(got['phik'][k].reshape(15, 15), step['Phi'][:15, :15])
        e2 = ic.block_error(got['qk'][k].reshape(15, 15), step['Q'][:15, :15])
        worst = max(worst, e1, e2)
        assert e1 <= (k + 1) * PER_SAMPLE and e2 <= (k + 1) * PER_SAMPLE, (k, e1, e2)   # (the state behind sample k carries k steps' rounding)
        assert np.array_equal(step['Phi'][15:, 15:], np.eye(7)) and not step['Q'][15:, :].any()
    Phi, Q = mi.accumulate_sequential(srv.steps)
    e1 = ic.block_error(got['Phi'].reshape(22, 22), Phi)
    e2 = ic.block_error(got['Q'].reshape(22, 22), 0.5 * (Q + Q.T))
    print('%s S=%d: per-sample worst %.2e, accumulated Phi %.2e Q %.2e' % (flag_set, S, worst, e1, e2))
    assert e1 <= S * PER_SAMPLE and e2 <= S * PER_SAMPLE


def test_selection_skips_cuts_and_refuses_beyond_capacity(exe, tmp_path):
    case = ic.make_case('larvio', 129, n=22, seed=1, rate=650.0)
    got = run_program(exe, case, tmp_path)
    assert got['capacity'] == ['129', '129']
    # every sample at or before state.time: nothing processed, all of them used
    case = ic.make_case('larvio', 0, n=22, seed=1, skipped=4, beyond=2)
    srv, info = ic.run_mirror(case, with_P=False)
    got = run_program(exe, case, tmp_path)
    assert [int(got['info'][0]), int(got['info'][1]), got['info'][2]] == [4, 0, 0.0] == [info['n_used'], info['n_propagated'], info['dt']]
    assert np.array_equal(got['Phi'].reshape(22, 22), np.eye(22)) and not got['Q'].any()
    assert np.array_equal(got['R'], case['state'].R.ravel()) and np.array_equal(got['prev'], case['prev'])


def test_zero_gyro_right_closed_form_is_not_finite_and_larvio_is(exe, tmp_path):
    for flag_set, finite in (('right_closed', False), ('larvio', True), ('left_closed', True)):
        case = ic.make_case(flag_set, 3, n=22, seed=2)
        case['samples'][1, 1:4] = case['state'].bg   # the unbiased gyro of the middle sample is exactly zero
        got = run_program(exe, case, tmp_path)
        assert bool(np.isfinite(got['Phi']).all() and np.isfinite(got['Q']).all()) == finite, flag_set
