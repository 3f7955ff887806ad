"""orcvio_msckf_io_triangulate_prune: the prune update of the one-call frames (io_step_frame, io_step_frame_ex) triangulating its own
tracks on the device between the frame's two updates, and mode ORCVIO_TRI_ALL_MOTION_BUT_LAST of k_triangulate.  Reference chain and
cases: tests/prune_tri_cases.py (their conditions: tests/test_prune_tri_cases.py).  Tolerances: valid / flags identical, accept identical
on kept tracks and 0 (gamma NaN) on dropped ones, p_w, dx, prune_dx and P within tri_io_cases.TOL relative."""
import dataclasses
import os

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror, mirror_triangulate as mt, oracle
from helpers import rel, GOLDEN
import mirror_frame_lifecycle as mfl
import prune_tri_cases as pc
import tri_io_cases as tc
from tri_io_cases import same_bits

pytestmark = pytest.mark.gpu
TOL = tc.TOL
INVALID, CAPACITY, TOO_LONG = 1, 3, 4
FAR = dict(translation_threshold=1e3)   # no track moves that far: every one is ORCVIO_TRI_NO_MOTION


def _handle(max_clones=24):
    return capi.MsckfUpdater(device=0, max_clones=max_clones, max_features=256, max_observations=4096)


@pytest.fixture(scope='module')
def upd(built):
    u = _handle()
    yield u
    u.close()


def _hidden(w, mode=None):
    pw = np.array(w.p_w, dtype=np.float64, copy=True).reshape(-1, 3)
    pw[np.ones(w.F, bool) if mode is None else np.asarray(mode) != tc.KEEP] = np.nan
    return dataclasses.replace(w, p_w=pw)


def frame(u, w, sp, remove, apply_dx, mode=None, cfg=None, arm=True, first_tri=None, prune_pw=None, no_remove=False):
    """One frame on the prior w.P: the first update on sp['first'], the prune update on sp['prune'] (its positions hidden when armed)."""
    u.cov_set(w.P)
    prune = sp['prune'] if prune_pw is None else dataclasses.replace(sp['prune'], p_w=prune_pw)
    first = _hidden(sp['first']) if first_tri else sp['first']
    got = u.io_step_frame(first, None, None, False, None, 1, _hidden(prune, mode) if arm else prune, apply_dx, [] if no_remove else remove,
                          triangulate=first_tri, triangulate_prune=(sp['tri'], mode, cfg) if arm else None)
    got['P'] = u.cov_get()
    return got


def check(got, ch, what=''):
    tri, keep, ref = ch['tri'], ch['keep'], ch['ref']
    assert got['rc'] == 0 and got['status_first'] == 0 and got['status_prune'] == 0, (what, got['rc'], got['status_first'], got['status_prune'])
    pt = got['prune_tri']
    assert np.array_equal(pt['valid'], tri['valid']) and np.array_equal(pt['flags'], tri['flags']), (what, pt['flags'], tri['flags'])
    errs = dict(dx=rel(got['dx'], ref['dx']), P=rel(got['P'], ref['P']))
    assert not got['prune_accept'][~keep].any() and np.isnan(got['prune_gamma'][~keep]).all(), what
    if keep.any():
        errs['p_w'] = rel(pt['p_w'][keep], tri['p_w'][keep])
        tried = keep & np.isfinite(tri['solution']).all(axis=1)   # (a KEEP track reports NaN in inv_param and cost)
        assert np.isnan(pt['solution'][keep & ~tried]).all() and np.isnan(pt['cost'][keep & ~tried]).all()
        if tried.any():
            errs['solution'] = rel(pt['solution'][tried], tri['solution'][tried])
        assert np.array_equal(got['prune_accept'][keep], ref['prune_accept']), what
        errs['prune_gamma'] = tc.gamma_err(got['prune_gamma'][keep], ref['prune_gamma'])
        errs['prune_dx'] = rel(got['prune_dx'], ref['prune_dx'])
    else:
        assert got['prune_stats'][3] == 0 and not got['prune_dx'].any()
    assert got['n_after'] == ref['n_after'] == got['P'].shape[0]
    print(what, 'kept', int(keep.sum()), 'of', len(keep), 'worst rel err', errs)
    assert all(e < TOL for e in errs.values()), (what, errs)
    return errs


# ---- mode 3 stand-alone, modes 0..2 unchanged -----------------------------------------------------------------------------------------
def _armed_update(u, w, mode, cfg=None):
    io = u.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=True)
    u.io_fill(io, _hidden(w, mode), with_P=True)
    tri = u.io_triangulate(cfg, mode)
    stats = u.io_update(True, False)
    return dict(dx=io['dx'].copy(), gamma=io['gamma'].copy(), accept=io['accept'].copy(), P=io['P_out'].copy(), stats=stats,
                tri={k: v.copy() for k, v in tri.items()})


def _whole_frame(u, w, mode=None, cfg=None):
    """The stand-alone form of the prune arming: a frame without a first update (no lost track) and without marginalisation, whose
    prune update -- every track of w, listing what the triangulation lists -- is the whole frame."""
    none = tc.select_tracks(w, np.zeros(w.F, bool))
    u.cov_set(w.P)
    got = u.io_step_frame(none, None, None, False, None, 1, _hidden(w, mode), 0, [], triangulate_prune=(w, mode, cfg))
    got['P'] = u.cov_get()
    return got


def test_mode_3_stand_alone_against_the_mirror(upd):
    w, _, _ = tc.window_case('small24')
    tri = pc.prune_tri(w)
    keep = tri['valid'] == 1
    assert keep.sum() >= 8 and (~keep).any()   # (the window's two-observation tracks have no motion in this mode)
    ref = oracle.msckf_update(tc.kept_window(w, tri), want_blocks=False, want_K=False)
    got = _whole_frame(upd, w)
    pt = got['prune_tri']
    assert got['rc'] == 0 and got['status_prune'] == 0 and got['prune_stats'][3] == 1 and not got['dx'].any()
    assert np.array_equal(pt['valid'], tri['valid']) and np.array_equal(pt['flags'], tri['flags'])
    assert np.array_equal(got['prune_accept'][keep], ref['accept']) and not got['prune_accept'][~keep].any() and np.isnan(got['prune_gamma'][~keep]).all()
    errs = dict(p_w=rel(pt['p_w'][keep], tri['p_w'][keep]), dx=rel(got['prune_dx'], ref['dx']), P=rel(got['P'], ref['P_new']),
                gamma=tc.gamma_err(got['prune_gamma'][keep], ref['gamma']))
    print('mode 3 stand-alone: kept', int(keep.sum()), 'of', w.F, errs)
    assert all(e < TOL for e in errs.values()), errs
    # ... and it is neither of its neighbours: ALL checks the motion on the last entry, ALL_BUT_LAST triangulates without it
    for md in (tc.ALL, tc.ALL_BUT_LAST):
        other = _whole_frame(upd, w, np.full(w.F, md, np.int32))['prune_tri']
        assert not (np.array_equal(other['valid'], pt['valid']) and same_bits(other['p_w'][keep], pt['p_w'][keep])), md
    # the first update's arming keeps its modes: 3 is refused there as it was
    io = upd.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=True)
    upd.io_fill(io, w, with_P=True)
    with pytest.raises(capi.MsckfError) as e:
        upd.io_triangulate(None, np.full(w.F, pc.ALL_MOTION_BUT_LAST, np.int32))
    assert e.value.code == INVALID


def test_modes_0_to_2_give_the_bits_recorded_on_the_parent_build(upd):
    """tests/golden/prune_tri_modes_parent.npz: the same input through modes 0..2 on a build of the commit in front of mode 3."""
    w, _, _ = tc.window_case('small24')
    g = np.load(os.path.join(GOLDEN, 'prune_tri_modes_parent.npz'))
    for md in (tc.KEEP, tc.ALL, tc.ALL_BUT_LAST):
        got = _armed_update(upd, w, np.full(w.F, md, np.int32))
        for k in ('valid', 'flags', 'p_w', 'solution', 'cost'):
            assert same_bits(got['tri'][k], g['m%d_%s' % (md, k)]), (md, k)
        for k in ('dx', 'gamma', 'accept', 'P'):
            assert same_bits(got[k], g['m%d_%s' % (md, k)]), (md, k)


# ---- the frame against the reference chain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', pc.CASES, ids=pc.case_id)
def test_armed_frame_against_the_reference_chain(upd, case):
    wn, fs, rm, ap = case
    w = pc.window(wn, fs)
    ch = pc.reference(case)
    got = frame(upd, w, ch['sp'], pc.remove_sets(w.N)[rm], ap)
    assert got['repaired'] == 0
    check(got, ch, pc.case_id(case))


def _all_valid(case):
    """The case with its valid prune tracks only: cuts, remove set, window."""
    wn, fs, rm, ap = case
    w = pc.window(wn, fs)
    ch = pc.reference(case)
    sp = dict(ch['sp'], tri=tc.select_tracks(ch['sp']['tri'], ch['keep']), prune=tc.select_tracks(ch['sp']['prune'], ch['keep']))
    return w, sp, pc.remove_sets(w.N)[rm]


@pytest.mark.parametrize('apply_dx', [0, 1])
def test_all_valid_frame_armed_equals_unarmed_at_the_devices_positions_bit_for_bit(built, apply_dx):
    w, sp, remove = _all_valid(('n12', 'euroc', 'newest', apply_dx))
    a, b = _handle(), _handle()
    try:
        ga = frame(a, w, sp, remove, apply_dx)
        assert ga['prune_tri']['valid'].all() and sp['prune'].F >= 10 and ga['repaired'] == 0
        gb = frame(b, w, sp, remove, apply_dx, arm=False, prune_pw=ga['prune_tri']['p_w'])
        for k in ('dx', 'prune_dx', 'prune_gamma', 'prune_accept', 'stats', 'prune_stats', 'P'):
            assert same_bits(ga[k], gb[k]), k
    finally:
        a.close(); b.close()


def test_both_armings_in_one_frame(upd):
    case = ('n12', 'euroc', 'newest', 1)
    w = pc.window(case[0], case[1])
    remove = pc.remove_sets(w.N)[case[2]]
    ch = tc.cached(('ptboth', case), lambda: pc.chain(w, remove, 1, first_tri=True))
    pc.check_conditions(ch)
    got = frame(upd, w, ch['sp'], remove, 1, first_tri=True)
    t1 = ch['first_tri']
    k1 = t1['valid'] == 1
    assert (~k1).any() and np.array_equal(got['tri']['valid'], t1['valid']) and np.array_equal(got['tri']['flags'], t1['flags'])
    assert rel(got['tri']['p_w'][k1], t1['p_w'][k1]) < TOL
    assert np.array_equal(got['accept'][k1], ch['ref']['accept']) and not got['accept'][~k1].any()
    check(got, ch, 'both armings')


def test_armed_lifecycle_frame_with_a_lost_slot_an_anchor_change_and_a_prune_update(built):
    frames, P0 = synth.make_lifecycle_stream(synth.Flags(**tc.EUROC))
    k = next(i for i, fr in enumerate(frames) if fr['lost'] and fr['changes'] and fr['prune'] is not None)
    table = mirror.chi2_table(frames[0]['w'].flags.chi2_prob)
    P = P0
    for fr in frames[:k]:
        P = mfl.step_frame(P, fr, 1, 0, table=table)['P']
    fr = frames[k]
    sel = np.diff(fr['prune'].obs_ptr) >= 2
    tri_win, prune = tc.select_tracks(fr['w'], sel), tc.select_tracks(fr['prune'], sel)
    tri = pc.prune_tri(tri_win)
    keep = tri['valid'] == 1
    assert keep.sum() >= 3
    ref = mfl.step_frame(P, dict(fr, prune=tc.select_tracks(prune, keep, tri['p_w'])), 1, 0, table=table)
    u = _handle()
    u.set_ekf_rows_mode(True)

    def step(f, pr, arm):
        u.set_extra_states(f['w'].n_extra)
        return u.io_step_frame_ex(win=f['w'], Phi=f['Phi'], Q=f['Q'], augment=True, slam=f['slam'], idp_dim=1, prune=pr, prune_apply_dx=0,
                                  remove=f['remove'], n_feature_states=f['n_feature_states'], lost=f['lost'], changes=f['changes'],
                                  R_b2c=f['R_b2c'], t_c_b=f['t_c_b'], literal_3d=0, triangulate_prune=arm)
    try:
        u.cov_set(P0)
        for f in frames[:k]:
            step(f, f['prune'], None)
        got = step(fr, _hidden(prune), (tri_win, None))
        got['P'] = u.cov_get()
        assert got['status_changes'] == 0 and got['repaired'] == 0
        errs = check(got, dict(tri=tri, keep=keep, ref=ref), 'lifecycle frame %d' % k)
        errs['new_param'] = rel(got['new_param'], ref['new_param'])
        errs['new_inv_depth'] = rel(got['new_inv_depth'], ref['new_inv_depth'])
        assert max(errs.values()) < TOL, errs
    finally:
        u.close()


def test_imu_arming_together_with_the_prune_arming(built):
    """orcvio_msckf_io_propagate_imu AND orcvio_msckf_io_triangulate_prune on one frame: bit for bit the frame given Phi, Q of the
    stand-alone propagation with the same prune arming (the idiom of tests/test_gpu_imu_frames.py)."""
    import imu_cases as ic
    fl = synth.Flags(use_larvio=1)
    w = synth.make_window(N=8, F=12, seed=3, track_len=(5, 8), flags=fl)
    P0 = np.ascontiguousarray(synth.make_window(N=7, F=1, seed=5, flags=fl).P)
    sub = synth.subset_tracks(w, [0, 1], min_obs=2)
    sel = np.diff(sub.obs_ptr) >= 2
    tri_win, prune = tc.select_tracks(w, sel), tc.select_tracks(sub, sel)
    assert prune.F >= 3
    case = ic.make_case('larvio', 10, n=22, seed=52, rate=200.0, skipped=1, beyond=2)
    cfg, state, prev = ic.to_capi(case)
    aux = capi.MsckfUpdater(device=0, max_clones=2, max_features=16, max_observations=256)
    a, b = _handle(), _handle()
    try:
        aux.cov_set(np.eye(22))
        pq = aux.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'], want_PhiQ=True)
        a.cov_set(P0); b.cov_set(P0)
        cfg, state, prev = ic.to_capi(case)
        a.io_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])
        ga = a.io_step_frame(w, None, None, True, None, 1, _hidden(prune), True, [0, 1], triangulate_prune=(tri_win, None))
        gb = b.io_step_frame(w, pq['Phi'], pq['Q'], True, None, 1, _hidden(prune), True, [0, 1], triangulate_prune=(tri_win, None))
        assert gb['rc'] == 0 and gb['stats'][3] == 1 and gb['prune_tri']['valid'].sum() >= 3 and gb['prune_stats'][3] == 1
        for k in ('dx', 'gamma', 'accept', 'stats', 'prune_dx', 'prune_gamma', 'prune_accept', 'prune_stats'):
            assert same_bits(ga[k], gb[k]), k
        for k in ga['prune_tri']:
            assert same_bits(ga['prune_tri'][k], gb['prune_tri'][k]), k
        assert same_bits(a.cov_get(), b.cov_get())
    finally:
        a.close(); b.close(); aux.close()


# ---- edge shapes ------------------------------------------------------------------------------------------------------------------------
def _whole(w, sel=None, first=None):
    """Cuts in which the prune update lists what the triangulation lists (every clone of a track `leaves`)."""
    sel = np.ones(w.F, bool) if sel is None else sel
    t = tc.select_tracks(w, sel)
    return dict(first=tc.select_tracks(w, ~sel if first is None else first), tri=t, prune=t, sel=sel)


EDGE = {
    'M2': (dict(N=6, F=6, seed=8, track_len=2), 24),             # of two listed observations the second-to-last is the first: no motion
    'M3': (dict(N=6, F=6, seed=8, track_len=3), 24),
    'M32': (dict(N=32, F=4, seed=2, track_len=32), 32),          # ORCVIO_MAX_TRACK
}


@pytest.mark.parametrize('name', list(EDGE))
def test_edge_track_lengths(built, name):
    kw, max_clones = EDGE[name]
    w = synth.make_window(**kw)
    sel = np.arange(w.F) >= 2   # (two tracks for the first update)
    sp = _whole(w, sel)
    cfg = mt.OptimizationConfig(translation_threshold=0.05)
    ch = pc.chain(w, [0, 1], 1, cfg=cfg, sp=sp)
    u = _handle(max_clones)
    try:
        got = frame(u, w, sp, [0, 1], 1, cfg=dataclasses.asdict(cfg))
        if name == 'M2':
            assert (got['prune_tri']['flags'] == 1).all() and not got['prune_tri']['valid'].any()
        else:
            assert ch['keep'].sum() >= 2
        check(got, ch, name)
    finally:
        u.close()


def test_one_prune_track(upd):
    w, sp, remove = _all_valid(('n6', 'euroc', 'oldest', 1))
    one = np.arange(sp['tri'].F) == 0
    sp = dict(sp, tri=tc.select_tracks(sp['tri'], one), prune=tc.select_tracks(sp['prune'], one))
    ch = pc.chain(w, remove, 1, sp=sp)
    assert ch['keep'].all() and ch['sp']['prune'].F == 1
    check(frame(upd, w, sp, remove, 1), ch, 'one prune track')


@pytest.mark.parametrize('apply_dx', [0, 1])
def test_no_valid_track_refuses_the_prune_update_and_leaves_the_first_updates_covariance(built, apply_dx):
    case = ('n12', 'euroc', 'newest', apply_dx)
    w = pc.window(case[0], case[1])
    sp, remove = pc.reference(case)['sp'], pc.remove_sets(w.N)[case[2]]
    a, b = _handle(), _handle()
    try:
        ga = frame(a, w, sp, remove, apply_dx, cfg=FAR, no_remove=True)
        pt = ga['prune_tri']
        assert not pt['valid'].any() and (pt['flags'] == 1).all() and np.isnan(pt['p_w']).all()
        assert ga['rc'] == 0 and ga['status_prune'] == 0 and ga['prune_stats'][3] == 0 and ga['stats'][3] == 1
        assert not ga['prune_accept'].any() and np.isnan(ga['prune_gamma']).all() and not ga['prune_dx'].any()
        # the first update alone, then one more plain frame on both handles: P bit for bit, and the factor behind it (it shapes the next dx)
        b.cov_set(w.P)
        gb = b.io_step_frame(sp['first'], None, None, False, None, 1, None, 0, [])
        assert same_bits(ga['dx'], gb['dx']) and same_bits(ga['P'], b.cov_get())
        nxt = [u.io_step_frame(sp['first'], None, None, False, None, 1, None, 0, remove) for u in (a, b)]
        assert same_bits(nxt[0]['dx'], nxt[1]['dx']) and same_bits(a.cov_get(), b.cov_get())
    finally:
        a.close(); b.close()


def test_every_track_keep_equals_the_unarmed_frame_bit_for_bit(built):
    case = ('n12', 'euroc', 'oldest', 1)
    w = pc.window(case[0], case[1])
    sp, remove = pc.reference(case)['sp'], pc.remove_sets(w.N)[case[2]]
    a, b = _handle(), _handle()
    try:
        ga = frame(a, w, sp, remove, 1, mode=np.zeros(sp['prune'].F, np.int32))
        gb = frame(b, w, sp, remove, 1, arm=False)
        pt = ga['prune_tri']
        assert pt['valid'].all() and not pt['flags'].any() and same_bits(pt['p_w'], np.ascontiguousarray(sp['prune'].p_w)) and np.isnan(pt['cost']).all()
        for k in ('dx', 'prune_dx', 'prune_gamma', 'prune_accept', 'stats', 'prune_stats', 'P'):
            assert same_bits(ga[k], gb[k]), k
    finally:
        a.close(); b.close()


def test_mixed_modes_in_one_arming(upd):
    case = ('n12', 'euroc', 'newest', 1)
    w = pc.window(case[0], case[1])
    sp, remove = pc.reference(case)['sp'], pc.remove_sets(w.N)[case[2]]
    mode = (np.arange(sp['prune'].F) % 4).astype(np.int32)
    ch = tc.cached(('ptmixed', case), lambda: pc.chain(w, remove, 1, mode=mode))
    check(frame(upd, w, sp, remove, 1, mode=mode), ch, 'modes 0..3 mixed')


# ---- the unfused form, repair ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('off', ['ORCVIO_STEP_FUSED', 'ORCVIO_LA_SPIN'])
def test_armed_frame_unfused_and_repaired_after_lost_hand_offs(built, monkeypatch, off):
    """ORCVIO_STEP_FUSED=0 (diagnostics build): the pose step and the pulls -- the list's too -- as launches of their own.
    ORCVIO_LA_SPIN=0: the look-ahead waits give up, both updates of the frame run again the safe way; the repeat of the prune update
    reports the same prune_tri."""
    case = ('n12', 'euroc', 'newest', 1)
    w = pc.window(case[0], case[1])
    ch = pc.reference(case)
    monkeypatch.setenv(off, '0')
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096, debug_hooks=off == 'ORCVIO_STEP_FUSED')
    monkeypatch.delenv(off)
    try:
        got = frame(u, w, ch['sp'], pc.remove_sets(w.N)[case[2]], 1)
        print(off, 'repaired', got['repaired'])
        assert got['repaired'] == (2 if off == 'ORCVIO_LA_SPIN' else 0)
        check(got, ch, off + '=0')
    finally:
        u.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _refused(code, call, *a, **kw):
    with pytest.raises(capi.MsckfError) as e:
        call(*a, **kw)
    assert e.value.code == code, (e.value.code, code)


def test_refusals(built):
    case = ('n12', 'euroc', 'newest', 1)
    w = pc.window(case[0], case[1])
    ch = pc.reference(case)
    sp, remove = ch['sp'], pc.remove_sets(w.N)[case[2]]
    tri_win, prune, first = sp['tri'], sp['prune'], sp['first']
    F2 = tri_win.F
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=64, max_observations=600)
    try:
        _refused(INVALID, u.io_triangulate_prune, tri_win)   # no open arena
        want = frame(u, w, sp, remove, 1)
        _refused(INVALID, u.io_triangulate_prune, tri_win)   # the frame has closed it
        u.cov_set(w.P)
        P0 = u.cov_get()

        def open_arena():
            io = u.io_begin(first.flags, first.N, first.F, int(first.obs_ptr[-1]), with_P=2)
            u.io_fill(io, first, with_P=False)

        open_arena()
        out = u.io_triangulate_prune(tri_win)
        before = {k: v.copy() for k, v in out.items()}
        rep = lambda **kw: dataclasses.replace(tri_win, **kw)
        oc = tri_win.obs_clone
        beyond = oc.copy(); beyond[-1] = w.N
        negative = oc.copy(); negative[0] = -1
        descending = oc.copy(); descending[[0, 1]] = descending[[1, 0]]
        twice = oc.copy(); twice[1] = twice[0]
        long_ptr = np.array([0, 33], np.int32)
        many = dataclasses.replace(tri_win, p_w=np.zeros((65, 3)), obs_ptr=np.arange(66, dtype=np.int32) * 2, obs_clone=np.tile([0, 1], 65).astype(np.int32), obs_z=np.zeros((130, 2)))
        wide = dataclasses.replace(tri_win, p_w=np.zeros((60, 3)), obs_ptr=np.arange(61, dtype=np.int32) * 11, obs_clone=np.tile(np.arange(11), 60).astype(np.int32), obs_z=np.zeros((660, 2)))
        bad4 = np.full(F2, 3, np.int32); bad4[-1] = 4
        neg = np.full(F2, 3, np.int32); neg[0] = -1
        arm_refusals = [
            (INVALID, dict(tri_win=tri_win, cfg=False)), (INVALID, dict(tri_win=tri_win, cfg=dict(huber_epsilon=float('nan')))),
            (INVALID, dict(tri_win=tri_win, cfg=dict(cost_threshold=float('inf')))), (INVALID, dict(tri_win=tri_win, mode=bad4)),
            (INVALID, dict(tri_win=tri_win, mode=neg)), (INVALID, dict(tri_win=False)), (INVALID, dict(tri_win=rep(obs_clone=beyond))),
            (INVALID, dict(tri_win=rep(obs_clone=negative))), (INVALID, dict(tri_win=rep(obs_clone=descending))), (INVALID, dict(tri_win=rep(obs_clone=twice))),
            (TOO_LONG, dict(tri_win=rep(p_w=np.zeros((1, 3)), obs_ptr=long_ptr, obs_clone=np.arange(33, dtype=np.int32), obs_z=np.zeros((33, 2))))),
            (CAPACITY, dict(tri_win=many)), (CAPACITY, dict(tri_win=wide))]
        for code, kw in arm_refusals:   # behind a good arming: the arming, its list and the block stay
            _refused(code, u.io_triangulate_prune, **kw)
            assert all(same_bits(out[k], before[k]) for k in out) and same_bits(u.cov_get(), P0)
        # a pending io_submit
        u.io_submit(False, False)
        _refused(INVALID, u.io_triangulate_prune, tri_win)
        u.io_collect()
        assert same_bits(u.cov_get(), P0)
        # in the frame call: nothing done, the arming stands
        short = tc.select_tracks(prune, np.arange(F2) > 0)
        j = next(j for j in range(F2) if tri_win.obs_clone[tri_win.obs_ptr[j]] > 0)   # a track that clone 0 has not seen
        strange_clone = prune.obs_clone.copy(); strange_clone[prune.obs_ptr[j]] = 0
        strange = dataclasses.replace(prune, obs_clone=strange_clone)
        for pr in (None, _hidden(short), _hidden(strange)):
            u.cov_set(w.P)
            io = u.io_begin(first.flags, first.N, first.F, int(first.obs_ptr[-1]), with_P=2)
            u.io_fill(io, first, with_P=False)
            out = u.io_triangulate_prune(tri_win)
            before = {k: v.copy() for k, v in out.items()}
            _refused(INVALID, _frame_on_open_arena, u, first, pr, 1, remove)
            assert all(same_bits(out[k], before[k]) for k in out) and same_bits(u.cov_get(), P0)
            got = _frame_on_open_arena(u, first, _hidden(prune), 1, remove)   # the arming stands: a good frame behind it succeeds
            got['prune_tri'] = {k: v.copy() for k, v in out.items()}
            got['P'] = u.cov_get()
            check(got, ch, 'behind a refused frame')
            for k in ('dx', 'prune_dx', 'P'):
                assert same_bits(got[k], want[k]), k
        # without an arming the refused arm calls leave nothing armed: the frame is the unarmed one
        u.cov_set(w.P)
        io = u.io_begin(first.flags, first.N, first.F, int(first.obs_ptr[-1]), with_P=2)
        u.io_fill(io, first, with_P=False)
        for code, kw in arm_refusals:
            _refused(code, u.io_triangulate_prune, **kw)
        plain = _frame_on_open_arena(u, first, prune, 1, remove)
        ref = frame(u, w, sp, remove, 1, arm=False)
        for k in ('dx', 'prune_dx', 'prune_accept'):
            assert same_bits(plain[k], ref[k]), k
        # a new io_begin drops the arming
        u.cov_set(w.P)
        io = u.io_begin(first.flags, first.N, first.F, int(first.obs_ptr[-1]), with_P=2)
        u.io_triangulate_prune(tri_win)
        got = frame(u, w, sp, remove, 1, arm=False)
        for k in ('dx', 'prune_dx', 'prune_accept', 'P'):
            assert same_bits(got[k], ref[k]), k
        # a communicator on the handle
        u.comm_init(capi.comm_unique_id(), 0, 1)
        u.cov_set(w.P)
        io = u.io_begin(first.flags, first.N, first.F, int(first.obs_ptr[-1]), with_P=False)
        _refused(INVALID, u.io_triangulate_prune, tri_win)
        u.comm_destroy()
    finally:
        u.close()


def _frame_on_open_arena(u, first, prune, apply_dx, remove):
    """orcvio_msckf_io_step_frame on the arena as it stands (io_begin and a possible arming made by the caller): the binding's io_step_frame
    opens the arena itself, which would drop the arming under test."""
    import ctypes as C
    st = capi.FrameStep()
    st.leg_dim = int(first.flags.leg_dim)
    st.augment = 0
    keep = []
    F2 = 0
    if prune is not None:
        F2 = int(prune.F)
        arrs = [np.ascontiguousarray(prune.p_w, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(prune.obs_ptr, dtype=np.int32),
                np.ascontiguousarray(prune.obs_clone, dtype=np.int32), np.ascontiguousarray(prune.obs_z, dtype=np.float64)]
        tr = capi.MsckfTracks(F2, arrs[0].ctypes.data_as(C.POINTER(C.c_double)), arrs[1].ctypes.data_as(C.POINTER(C.c_int32)),
                              arrs[2].ctypes.data_as(C.POINTER(C.c_int32)), arrs[3].ctypes.data_as(C.POINTER(C.c_double)), None)
        keep += arrs + [tr]
        st.prune_tracks = C.pointer(tr)
    st.prune_apply_dx = int(apply_dx)
    rm = np.ascontiguousarray(list(remove), dtype=np.int32)
    st.remove_clones = rm.ctypes.data_as(C.POINTER(C.c_int32))
    st.n_remove = len(rm)
    res = capi.FrameResult()
    rc = u.lib.orcvio_msckf_io_step_frame(u.h, C.byref(st), C.byref(res))
    if rc != 0:
        raise capi.MsckfError(rc, 'orcvio_msckf_io_step_frame')
    n = first.n
    arr = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(dt, copy=True) if p else None
    return dict(rc=rc, dx=arr(res.dx, n, np.float64), prune_dx=arr(res.prune_dx, n, np.float64), prune_gamma=arr(res.prune_gamma, F2, np.float64),
                prune_accept=arr(res.prune_accept, F2, np.int32), stats=np.array(res.stats[:], dtype=np.int32),
                prune_stats=np.array(res.prune_stats[:], dtype=np.int32), n_after=int(res.n_after), status_first=int(res.status_first),
                status_prune=int(res.status_prune), repaired=int(res.repaired))
