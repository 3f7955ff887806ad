"""orcvio_msckf_io_triangulate in front of the one-call frames (io_step_frame, io_step_frame_ex): the first update triangulates its
own tracks.  Reference chain (tests/tri_io_cases.py): the mirror's triangulation, the invalid tracks removed, then
oracle/mirror_frame.step_frame (tests/mirror_frame_lifecycle.step_frame for the frame with feature events) at the mirror's
positions.  Tolerances as tests/test_gpu_io_triangulate.py."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror
from helpers import rel
import mirror_frame_lifecycle as mfl
import tri_io_cases as tc
from tri_io_cases import same_bits

pytestmark = pytest.mark.gpu
TOL = tc.TOL


def _handle(n_extra=tc.NSLAM):
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096)
    u.set_extra_states(n_extra)
    u.set_ekf_rows_mode(True)
    return u


def _hidden(w):
    return dataclasses.replace(w, p_w=np.full_like(w.p_w, np.nan))


def _step(u, fr, w, apply_dx, tri):
    return u.io_step_frame(w, fr['Phi'], fr['Q'], True, fr['slam'], 1, fr['prune'], apply_dx, fr['remove'], triangulate=tri)


def _check_frame(it, got, r, Pg, has_prune, worst):
    tri, keep, ref = r['tri'], r['keep'], r['ref']
    assert got['rc'] == 0 and got['status_first'] == 0 and got['status_prune'] == 0, (it, got['rc'], got['status_first'], got['status_prune'])
    assert np.array_equal(got['tri']['valid'], tri['valid']) and np.array_equal(got['tri']['flags'], tri['flags']), it
    worst['p_w'] = max(worst['p_w'], rel(got['tri']['p_w'][keep], tri['p_w'][keep]))
    assert np.array_equal(got['accept'][keep], ref['accept']), it
    assert not got['accept'][~keep].any() and np.isnan(got['gamma'][~keep]).all(), it
    worst['gamma'] = max(worst['gamma'], tc.gamma_err(got['gamma'][keep], ref['gamma']))
    worst['dx'] = max(worst['dx'], rel(got['dx'], ref['dx']))
    if has_prune:
        assert np.array_equal(got['prune_accept'], ref['prune_accept']), it
        worst['prune_dx'] = max(worst['prune_dx'], rel(got['prune_dx'], ref['prune_dx']))
    assert got['n_after'] == ref['n_after'] == Pg.shape[0], it
    worst['P'] = max(worst['P'], rel(Pg, ref['P']))
    assert max(worst.values()) < TOL, (it, worst)


def _run_stream(u, name, repaired=False):
    frames, P0 = tc.stream(name)
    refs = tc.stream_reference(name)
    worst = dict(p_w=0.0, gamma=0.0, dx=0.0, prune_dx=0.0, P=0.0)
    u.cov_set(P0)
    for it, (fr, r) in enumerate(zip(frames, refs)):
        got = _step(u, fr, _hidden(fr['w']), 0, True)
        want_repairs = (2 if fr['prune'] is not None else 1) if repaired else 0   # (as the unarmed call reports it: tests/test_gpu_step_oracle.py)
        assert got['repaired'] == want_repairs, (it, got['repaired'])
        _check_frame(it, got, r, u.cov_get(), fr['prune'] is not None, worst)
    return worst


@pytest.mark.parametrize('name', list(tc.FLAG_SETS))
def test_armed_frames_against_the_reference_chain(built, name):
    u = _handle()
    try:
        print(name, 'worst rel err', _run_stream(u, name))
    finally:
        u.close()


def test_armed_frames_repaired_after_lost_hand_offs(built, monkeypatch):
    """ORCVIO_LA_SPIN=0: the look-ahead waits give up, both updates of a frame run again the safe way -- the repeat of the first keeps
    the positions and the dropped tracks of the attempt that triangulated."""
    monkeypatch.setenv('ORCVIO_LA_SPIN', '0')
    u = _handle()
    monkeypatch.delenv('ORCVIO_LA_SPIN')
    try:
        print('ORCVIO_LA_SPIN=0 worst rel err', _run_stream(u, 'euroc', repaired=True))
    finally:
        u.close()


def test_all_valid_frame_armed_equals_unarmed_at_the_devices_positions_bit_for_bit(built):
    frames, P0 = tc.stream('euroc')
    assert tc.stream_reference('euroc')[3]['keep'].all()
    a, b = _handle(), _handle()
    try:
        for u in (a, b):
            u.cov_set(P0)
            for fr in frames[:3]:
                _step(u, fr, fr['w'], 0, None)
        assert same_bits(a.cov_get(), b.cov_get())
        fr = frames[3]
        ga = _step(a, fr, _hidden(fr['w']), 0, True)
        assert ga['tri']['valid'].all() and ga['repaired'] == 0
        gb = _step(b, fr, dataclasses.replace(fr['w'], p_w=ga['tri']['p_w']), 0, None)
        for k in ('dx', 'gamma', 'accept', 'prune_dx', 'prune_gamma', 'prune_accept', 'stats', 'prune_stats'):
            assert same_bits(ga[k], gb[k]), k
        assert same_bits(a.cov_get(), b.cov_get())
    finally:
        a.close(); b.close()


def test_armed_frame_with_a_lost_slot_and_an_anchor_change(built):
    """io_step_frame_ex armed, on the first frame of synth.make_lifecycle_stream that loses an in-state feature, changes an anchor and
    has tracks of its own; the frames in front of it run unarmed at the given positions on both sides."""
    frames, P0 = synth.make_lifecycle_stream(synth.Flags(**tc.EUROC))
    k = next(i for i, fr in enumerate(frames) if fr['lost'] and fr['changes'] and fr['w'].F >= 10)
    table = mirror.chi2_table(frames[0]['w'].flags.chi2_prob)
    P = P0
    for fr in frames[:k]:
        P = mfl.step_frame(P, fr, 1, 0, table=table)['P']
    fr = frames[k]
    tri = tc.mirror_tri(fr['w'])
    keep = tri['valid'] == 1
    assert keep.sum() >= 10
    ref = mfl.step_frame(P, dict(fr, w=tc.kept_window(fr['w'], tri)), 1, 0, table=table)
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096)
    u.set_ekf_rows_mode(True)

    def step(f, w, arm):
        u.set_extra_states(f['w'].n_extra)
        return u.io_step_frame_ex(win=w, Phi=f['Phi'], Q=f['Q'], augment=True, slam=f['slam'], idp_dim=1, prune=f['prune'], prune_apply_dx=0,
                                  remove=f['remove'], n_feature_states=f['n_feature_states'], lost=f['lost'], changes=f['changes'],
                                  R_b2c=f['R_b2c'], t_c_b=f['t_c_b'], literal_3d=0, triangulate=arm)
    try:
        u.cov_set(P0)
        for f in frames[:k]:
            step(f, f['w'], None)
        got = step(fr, _hidden(fr['w']), True)
        assert got['status_changes'] == 0 and got['repaired'] == 0
        worst = dict(p_w=0.0, gamma=0.0, dx=0.0, prune_dx=0.0, P=0.0)
        _check_frame(k, got, dict(tri=tri, keep=keep, ref=ref), u.cov_get(), fr['prune'] is not None, worst)
        worst['new_param'] = rel(got['new_param'], ref['new_param'])
        worst['new_inv_depth'] = rel(got['new_inv_depth'], ref['new_inv_depth'])
        print('lifecycle frame', k, 'kept', int(keep.sum()), 'of', fr['w'].F, 'worst rel err', worst)
        assert max(worst.values()) < TOL, worst
    finally:
        u.close()
