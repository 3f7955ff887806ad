"""The C++ host layer's MsckfBackend::single_levenberg_marquardt / levenberg_marquardt (orcvio_amd/csrc/host/orcvio_msckf_host.hpp)
run from tests/cpp/test_host_object_lm.cpp: the same library call as the Python binding's, so the same bits."""
import os
import subprocess

import numpy as np
import pytest

from orcvio_amd import capi
from test_host_shim import _build
import object_lm_cases as oc

pytestmark = pytest.mark.gpu


def _fmt(a):
    return ' '.join('nan' if not np.isfinite(v) else repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel())


def test_host_wrapper_equals_the_binding(built, tmp_path):
    cases = [oc.one_car(2, 1, 0), oc.one_car(5, 0, 0), oc.one_car(33, 0, 1)]
    w = oc.WEIGHTS_REF
    lines = [str(len(cases))]
    for obj, ms, mk in cases:
        lines.append('%d %d 1 0' % (obj.kps.shape[0], len(obj.frames)))
        lines += [_fmt(w), _fmt(ms), _fmt(mk), _fmt(obj.wTo), _fmt([fr['wTc'] for fr in obj.frames]), _fmt([fr['zs'] for fr in obj.frames]),
                  _fmt([fr['bbox'] for fr in obj.frames])]
    path = tmp_path / 'cases.txt'
    path.write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'test_host_object_lm')
    _build('test_host_object_lm.cpp', exe)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'host object lm ok' in out.stdout and 'refused 1 status 1' in out.stdout and 'short bbox refused 1 status 1' in out.stdout
    upd = capi.MsckfUpdater(device=0, max_clones=8, max_features=64, max_observations=256)
    try:
        tracks, stats = upd.object_lm([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], True, 0, w)
    finally:
        upd.close()
    rows = {(t[0], int(t[1])): t for t in (ln.split() for ln in out.stdout.splitlines()) if t and t[0] in ('single', 'batch')}
    for k in range(len(cases)):
        want = np.concatenate([tracks[k].wTo.ravel(), tracks[k].shape, tracks[k].kps.ravel()])
        for tag in ('single', 'batch'):
            t = rows[(tag, k)]
            assert int(t[3]) == 1 and int(t[5]) == stats[k]['status'] == 1
            assert int(t[7]) == stats[k]['iterations'] and int(t[9]) == stats[k]['evaluations']
            assert float(t[11]) == stats[k]['cost0'] and float(t[13]) == stats[k]['cost']
            assert np.array_equal(np.array([float(v) for v in t[15:]]), want)
