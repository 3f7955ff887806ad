"""The C++ host layer's prune triangulation (orcvio_amd/csrc/host/orcvio_msckf_host.hpp: MsckfBackend::buildPruneTriLists,
::writeBackPruneTriangulation, the frame call site ::stepFramePruneArmed), run from tests/cpp/test_host_prune_tri.cpp: the program checks
the selection and the write-back against the reference's rules and prints its frame; the same frame through the ctypes binding gives
the same bits."""
import dataclasses
import subprocess

import numpy as np
import pytest

from orcvio_amd import capi, synth
from test_host_shim import _build
from tri_io_cases import same_bits

pytestmark = pytest.mark.gpu


def _parse(text):
    out = {}
    for line in text.splitlines():
        p = line.split()
        if len(p) >= 3 and p[0] in ('D', 'I') and int(p[2]) == len(p) - 3:
            out[p[1]] = np.array([float.fromhex(v) for v in p[3:]], np.float64) if p[0] == 'D' else np.array([int(v) for v in p[3:]], np.int32)
    return out


def test_host_frame_equals_the_ctypes_call_bit_for_bit(built, tmp_path):
    exe = str(tmp_path / 'test_host_prune_tri')
    _build('test_host_prune_tri.cpp', exe)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    tail = [ln for ln in run.stdout.splitlines() if not ln.startswith(('D ', 'I '))]
    print('\n'.join(tail))
    assert run.returncode == 0, '\n'.join(tail) + run.stderr
    assert 'host prune tri ok' in run.stdout
    d = _parse(run.stdout)
    N = len(d['t_b_w']) // 3
    n = 22 + 6 * N
    fl = synth.Flags(use_larvio=1, use_left_perturbation=0, if_fej=0, estimate_td=0, discard_large_update=0, noise_feature=0.008, chi2_prob=0.95)
    win = lambda pre, p_w: synth.Window(
        R_b2w=d['R_b2w'].reshape(N, 3, 3), t_b_w=d['t_b_w'].reshape(N, 3), t_fej=d['t_fej'].reshape(N, 3), R_b2c=d['R_b2c'].reshape(N, 3, 3),
        t_c_b=d['t_c_b'].reshape(N, 3), p_w=p_w.reshape(-1, 3), obs_ptr=d[pre + '_ptr'], obs_clone=d[pre + '_clone'], obs_z=d[pre + '_z'].reshape(-1, 2),
        obs_zvel=d.get(pre + '_zvel', np.zeros_like(d[pre + '_z'])).reshape(-1, 2), P=d['P'].reshape(n, n), flags=fl)
    first, tri_win, prune = win('first', d['first_p_w']), win('tri', d['prune_p_w']), win('prune', d['prune_p_w'])
    F2 = prune.F
    assert F2 >= 12 and (d['mode'] == 0).any() and (d['mode'] == 3).any() and np.isnan(d['prune_p_w'].reshape(-1, 3)[d['mode'] == 3]).all()
    u = capi.MsckfUpdater(device=0, max_clones=16, max_features=256, max_observations=8192)
    try:
        u.cov_set(first.P)
        got = u.io_step_frame(first, None, None, False, None, 1, prune, True, list(d['remove']), triangulate_prune=(tri_win, d['mode']))
        assert got['rc'] == 0 and got['repaired'] == 0
        t = got['prune_tri']
        for k, v in (('dx', got['dx']), ('prune_dx', got['prune_dx']), ('prune_gamma', got['prune_gamma']), ('prune_accept', got['prune_accept']),
                     ('tri_valid', t['valid']), ('tri_flags', t['flags']), ('tri_p_w', t['p_w'].reshape(-1)), ('tri_solution', t['solution'].reshape(-1)),
                     ('tri_cost', t['cost']), ('P_after', u.cov_get().reshape(-1))):
            assert same_bits(np.ascontiguousarray(v), d[k]), k
    finally:
        u.close()
