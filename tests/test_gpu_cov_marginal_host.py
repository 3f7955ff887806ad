"""GPU test of the C++ host layer's odometry getters on the resident covariance (orcvio_amd/csrc/host/orcvio_msckf_host.hpp:
MsckfBackend::odometryCovariance and the pair odometryCovarianceSubmit / odometryCovarianceCollect), run from
tests/cpp/test_host_cov_marginal.cpp as a filter calls them -- blocking, and as the pair behind a frame call with the caller's state
increment in between: against the ctypes call on a handle of this process that goes through the same history (bit for bit), and against
the literal getPpose / getPvel on the covariance cov_get brings back (inside the derived bar of tests/cov_marginal_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

from orcvio_amd import capi, synth
import cov_cases as cc
import cov_marginal_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def exe(built, tmp_path_factory):
    out = str(tmp_path_factory.mktemp('marg_host') / 'test_host_cov_marginal')
    libdir = os.path.join(ROOT, 'orcvio_amd', 'lib')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-Wall', '-o', out, os.path.join(ROOT, 'tests', 'cpp', 'test_host_cov_marginal.cpp'),
                           '-L', libdir, '-lorcvio_msckf', '-Wl,-rpath,' + libdir])
    return out


@pytest.mark.parametrize('leg,N', [(22, 7), (46, 2)])
def test_the_host_getters_against_the_ctypes_call_and_the_literal_getters(exe, tmp_path, leg, N):
    n = leg + 6 * N
    P0 = cc.graded_factorable(n)
    P0 = P0 + 1e-3 * np.triu(P0, 1)   # asymmetric: P_po and P_op are read separately
    Phi, Q = cc.phi_q(leg, 7)
    R = mc.rotation(leg)
    p = str(tmp_path / 'case.txt')
    with open(p, 'w') as f:
        f.write(' '.join(repr(float(v)) for v in list(R.ravel()) + [leg, N, n] + list(P0.ravel()) + list(Phi.ravel()) + list(Q.ravel())))
    run = subprocess.run([exe, p], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == 'host cov marginal ok', run.stdout
    got = {}
    for line in lines[:-1]:
        w = line.split()
        a = np.array(w[1:], dtype=np.float64)
        got[w[0]] = (a[:36].reshape(6, 6), a[36:].reshape(3, 3))
    assert set(got) == {'blocking', 'behind', 'again'}

    idx, T = mc.odometry_spec(R)
    fl = synth.Flags(use_larvio=1, leg_dim=leg)
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=16, max_observations=256)
    try:
        u.cov_set(P0)
        out0 = u.cov_get_marginal(idx, T)
        w = synth.make_window(N=N + 1, F=0, seed=300 + N, track_len=None, flags=fl)
        res = u.io_step_frame(w, Phi, Q, augment=True, remove=[0])
        assert res['rc'] == 0 and res['n_after'] == n
        u.cov_marginal_submit(idx, T)
        out1 = u.cov_marginal_collect()
        P1 = u.cov_get()
    finally:
        u.close()
    assert not np.array_equal(P1[:9, :9], P0[:9, :9])   # (the frame's propagation reached the leading IMU rows)
    for name, out, P in (('blocking', out0, P0), ('behind', out1, P1), ('again', out1, P1)):
        pose, vel = got[name]
        assert np.array_equal(pose, out[:6, :6]) and np.array_equal(vel, out[6:, 6:]), name
        c = mc.Case(n, 9, 9, P=P, idx=idx, T=T)
        frac = mc.check_getters(c, pose, vel, name)
        lit_pose, lit_vel = mc.literal_getters(P, R)
        lit = mc.check_getters(c, lit_pose, lit_vel, name + ' (literal)')
        print('FIG host getters leg=%d %s fraction of the bar: device %.3f literal %.3f' % (leg, name, frac, lit))
    assert not np.array_equal(got['blocking'][0], got['blocking'][0].T)   # (nothing symmetrised on the way)
