"""The C++ host layer's lite object mapper -- MsckfBackend::single_object_initialization_lite / single_levenberg_marquardt_lite /
levenberg_marquardt_lite (orcvio_amd/csrc/host/orcvio_msckf_host.hpp) -- run from tests/cpp/test_host_object_lite.cpp: the same
library calls as the Python binding's, so the same bits."""
import subprocess

import numpy as np
import pytest

from orcvio_amd import capi
from test_host_shim import _build
import object_lite_cases as lc

pytestmark = pytest.mark.gpu


def _fmt(a):
    return ' '.join(repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel())


def test_host_wrapper_equals_the_binding(built, tmp_path):
    cases = [lc.synthetic(2, 2), lc.synthetic(17, 2), lc.synthetic(30, 1)]
    w = lc.UNIT
    lines = [str(len(cases))]
    for obj, ms in cases:
        lines.append('%d 1 0' % len(obj.frames))
        lines += [_fmt(w), _fmt(ms), _fmt(obj.wTo), _fmt([fr['wTc'] for fr in obj.frames]), _fmt([fr['bbox'] for fr in obj.frames])]
    path = tmp_path / 'cases.txt'
    path.write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'test_host_object_lite')
    _build('test_host_object_lite.cpp', exe)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'host object lite ok' in out.stdout and 'refused 1 status 1' in out.stdout and 'short bbox refused 1 status 1' in out.stdout
    objs, ms = [c[0] for c in cases], [c[1] for c in cases]
    upd = capi.MsckfUpdater(device=0, max_clones=8, max_features=64, max_observations=256)
    try:
        tracks, stats = upd.object_lm_lite(objs, ms, True, 0, w, max_iter=lc.MAX_ITER)
        inits = upd.object_init_lite(objs, ms)
        cinits, ctracks, cstats = upd.object_init_lm_lite(objs, ms, True, 0, w, max_iter=lc.MAX_ITER)
    finally:
        upd.close()
    rows = {(t[0], int(t[1])): t for t in (ln.split() for ln in out.stdout.splitlines()) if t and t[0] in ('single', 'batch', 'chain', 'init', 'chaininit')}
    for k in range(len(cases)):
        for tag, tr, st in (('single', tracks, stats), ('batch', tracks, stats), ('chain', ctracks, cstats)):
            t = rows[(tag, k)]
            assert int(t[5]) == st[k]['status'] and int(t[3]) == (1 if st[k]['status'] == 1 else 0)
            assert int(t[7]) == st[k]['iterations'] and int(t[9]) == st[k]['evaluations']
            assert float(t[11]) == st[k]['cost0'] and float(t[13]) == st[k]['cost']
            assert t[-2] == 'kps' and int(t[-1]) == 0
            if st[k]['status'] == 1:
                assert np.array_equal(np.array([float(v) for v in t[15:34]]), np.concatenate([tr[k].wTo.ravel(), tr[k].shape]))
        assert stats[k]['status'] == 1
        t = rows[('init', k)]
        assert int(t[3]) == 1 and int(t[5]) == inits[k]['status'] == 1 and float(t[7]) == inits[k]['d']
        assert np.array_equal(np.array([float(v) for v in t[9:25]]), inits[k]['wTo'].ravel())
        t = rows[('chaininit', k)]
        assert int(t[3]) == cinits[k]['status'] and float(t[5]) == cinits[k]['d']
