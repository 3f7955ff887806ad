"""orcvio_msckf_io_choose_clones: the one-call frames (io_step_frame, io_step_frame_ex) checking the caller's remove_clones against
findRedundantImuStates on the poses the frame's first update leaves (k_clone_choice between the two updates).  Cases and their
conditions: tests/clone_choice_cases.py (tests/test_clone_choice_mirror.py); mirror: tests/mirror_clone_choice.py.

The verdict is compared with the mirror evaluated on the DEVICE's own published dx and the records handed in, so the comparison tests
this kernel and not the update in front of it: chosen / compared / taken / agree identical, angle and distance within ten times the
mirror's own distance from the 60-digit evaluation (clone_choice_cases.ANGLE_SPREAD / DISTANCE_SPREAD, relative)."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror, mirror_frame
from helpers import rel
import clone_choice_cases as cc
import mirror_clone_choice as mc
import prune_tri_cases as pc
import tri_io_cases as tc
from tri_io_cases import same_bits

pytestmark = pytest.mark.gpu
TOL = tc.TOL   # tests/test_gpu_prune_tri.py's, for the chain of the re-issued second half
INVALID = 1
ANGLE_BAR, DISTANCE_BAR = 10 * cc.ANGLE_SPREAD, 10 * cc.DISTANCE_SPREAD
AGREE = [n for n in cc.names() if cc.SPECS[n]['agree']]
DIFFER = [n for n in cc.names() if not cc.SPECS[n]['agree']]
OUTS = ('dx', 'gamma', 'accept', 'stats', 'prune_dx', 'prune_gamma', 'prune_accept', 'prune_stats', 'n_after', 'status_first', 'status_prune')


def _handle(**kw):
    return capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096, **kw)


@pytest.fixture(scope='module')
def upd(built):
    u = _handle()
    yield u
    u.close()


@pytest.fixture(scope='module')
def upd2(built):
    u = _handle()
    yield u
    u.close()


def frame(u, c, remove=None, arm=True, apply_dx=1, first=None, prune='follow', cam=None, P=None, over=None, **kw):
    """One frame on the case's prior: the first update on its lost tracks, the prune update on the tracks that follow from `remove`
    (default: the case's prediction), armed with the case's configuration."""
    remove = c['predicted'] if remove is None else remove
    u.cov_set(c['w'].P if P is None else P)
    pr = cc.prune_for(c, remove) if isinstance(prune, str) else prune
    got = u.io_step_frame(c['first'] if first is None else first, None, None, False, None, 1, pr, apply_dx, remove,
                          choose_clones=cc.choose_kwargs(c, cam, **(over or {})) if arm else None, **kw)
    got['P'] = u.cov_get()
    return got


def against_mirror(got, c, applied, predicted=None, what=''):
    ch = got['choice']
    want = mc.evaluate(dict(c, predicted=c['predicted'] if predicted is None else predicted), got['dx'], applied)
    e_a = float(np.max(np.abs(ch['angle'] - want['angle']) / np.abs(want['angle'])))
    e_d = float(np.max(np.abs(ch['distance'] - want['distance']) / np.abs(want['distance'])))
    print('%s chosen %s compared %s taken %s agree %d | angle err %.2e (bar %.1e) distance err %.2e (bar %.1e)' %
          (what or c['name'], ch['chosen'], ch['compared'], ch['taken'], ch['agree'], e_a, ANGLE_BAR, e_d, DISTANCE_BAR))
    assert ch['evaluated'] == 1
    for k in ('chosen', 'compared', 'taken', 'agree'):
        assert ch[k] == want[k], (what, k, ch[k], want[k])
    assert e_a <= ANGLE_BAR and e_d <= DISTANCE_BAR, (what, e_a, e_d)
    return want


def same_outputs(ga, gb, keys=OUTS + ('P',)):
    for k in keys:
        assert same_bits(np.asarray(ga[k]), np.asarray(gb[k])), k


def next_frame_same(a, b, c):
    """the factor behind P shapes the next update's dx: one more plain frame on both handles"""
    nxt = [u.io_step_frame(c['first'], None, None, False, None, 1, None, 0, []) for u in (a, b)]
    assert same_bits(nxt[0]['dx'], nxt[1]['dx']) and same_bits(a.cov_get(), b.cov_get())


# ---- the verdict --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cc.names())
def test_the_verdict_is_the_mirrors_on_the_devices_dx(upd, name):
    c = cc.case(name)
    got = frame(upd, c)
    assert got['rc'] == 0 and got['status_first'] == 0 and got['status_prune'] == 0 and got['repaired'] == 0 and got['stats'][3] == 1
    assert mc.applies(got['dx'], 1, c['w'].flags.discard_large_update)
    if cc.SPECS[name]['extrin']:
        assert np.abs(got['dx'][15:21]).min() > 0.0
    want = against_mirror(got, c, True)
    # ... and the case is what its builder placed: the pattern, the agreement, the choice on the post-update records
    assert tuple(want['taken']) == c['pattern'] and want['agree'] == int(c['agree']) and want['chosen'] == c['truth']


# ---- dx not applied: the records handed in, as they are -----------------------------------------------------------------------------------
def _velocity_coupled(c, k_dx=3.0):
    """the case's prior with the IMU velocity tied to a clone's position (P' = T P T^T, T = I + k e_v e_p^T): the rows of the update do
    not touch the velocity, so dx' = T dx -- its velocity part k times the clone's position increment, far above discard_large_update's 1.0"""
    w = c['w']
    col = w.flags.leg_dim + 6 * (w.N - 2) + 3
    k = k_dx / abs(c['dx_ref'][col])
    T = np.eye(w.n)
    T[3, col] = k
    return np.ascontiguousarray(T @ w.P @ T.T)


@pytest.mark.parametrize('kind', ['no_first_update', 'refused_first_update', 'discarded_dx', 'prune_apply_dx_0'])
@pytest.mark.parametrize('predicted', ['pre', 'post'])
def test_dx_not_applied_reads_the_records_as_given(upd, kind, predicted):
    c = cc.case('n7_10_differ')
    pred = c['predicted'] if predicted == 'pre' else c['truth']
    # (records that are NOT what the window's poses give: the kernel must read them and nothing else)
    cam = c['cam_pre'].copy()
    cam[:, 9:] *= 1.0 + 1e-9
    ce = dict(c, cam_pre=cam)
    kw = dict(remove=pred, cam=cam)
    if kind == 'no_first_update':
        got = frame(upd, ce, first=tc.select_tracks(c['first'], np.zeros(c['first'].F, bool)), **kw)
        assert got['stats'][3] == 0 and not got['dx'].any()
    elif kind == 'refused_first_update':
        got = frame(upd, ce, P=c['w'].P * 1e30, raise_on_refusal=False, **kw)
        assert got['rc'] == 6 and got['status_first'] == 6 and got['status_prune'] == 6
    elif kind == 'discarded_dx':
        fl = dataclasses.replace(c['w'].flags, discard_large_update=1)
        cd = dict(ce, w=dataclasses.replace(c['w'], flags=fl), first=dataclasses.replace(c['first'], flags=fl))
        got = frame(upd, cd, P=_velocity_coupled(c), prune=dataclasses.replace(cc.prune_for(c, pred), flags=fl), **kw)
        assert got['stats'][3] == 1 and np.linalg.norm(got['dx'][3:6]) > 1.0 and not mc.applies(got['dx'], 1, 1)
    else:
        got = frame(upd, ce, apply_dx=0, **kw)
        assert got['stats'][3] == 1 and got['dx'].any()
    want = against_mirror(got, ce, False, pred, kind)
    assert want['chosen'] == c['predicted'] and want['agree'] == int(predicted == 'pre')
    assert got['n_after'] == c['w'].n - (12 if predicted == 'pre' else 0)


# ---- agreement: the unarmed frame, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', AGREE)
def test_an_agreeing_frame_is_the_unarmed_frame_bit_for_bit(upd, upd2, name):
    c = cc.case(name)
    ga = frame(upd, c)
    gb = frame(upd2, c, arm=False)
    assert ga['choice']['agree'] == 1 and ga['prune_stats'][3] == 1 and ga['n_after'] == c['w'].n - 12 == ga['P'].shape[0]
    same_outputs(ga, gb)
    next_frame_same(upd, upd2, _after_removal(c, c['predicted']))


def _after_removal(c, remove):
    """the case's first-update tracks on the window without the removed clones (for the frame that follows a marginalisation)"""
    w = c['first']
    keep = np.array([i for i in range(w.N) if i not in remove])
    new = -np.ones(w.N, int); new[keep] = np.arange(len(keep))
    ok = np.isin(w.obs_clone, keep)
    cnt = np.array([int(ok[w.obs_ptr[j]:w.obs_ptr[j + 1]].sum()) for j in range(w.F)])
    sel = cnt >= 2
    ptr = [0]; oc = []; oz = []; ov = []
    for j in np.flatnonzero(sel):
        idx = [o for o in range(w.obs_ptr[j], w.obs_ptr[j + 1]) if ok[o]]
        oc += [new[w.obs_clone[o]] for o in idx]; oz += [w.obs_z[o] for o in idx]; ov += [w.obs_zvel[o] for o in idx]
        ptr.append(len(oc))
    sub = dataclasses.replace(w, R_b2w=w.R_b2w[keep].copy(), t_b_w=w.t_b_w[keep].copy(), t_fej=w.t_fej[keep].copy(), R_b2c=w.R_b2c[keep].copy(),
                              t_c_b=w.t_c_b[keep].copy(), p_w=w.p_w[sel].copy(), obs_ptr=np.asarray(ptr, np.int32), obs_clone=np.asarray(oc, np.int32),
                              obs_z=np.asarray(oz, np.float64).reshape(-1, 2), obs_zvel=np.asarray(ov, np.float64).reshape(-1, 2))
    assert sub.F >= 3
    return dict(c, first=sub)


# ---- disagreement: the second half held back ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', DIFFER)
def test_a_disagreeing_frame_holds_its_second_half_back(upd, upd2, name):
    c = cc.case(name)
    w = c['w']
    ga = frame(upd, c)
    ch = ga['choice']
    assert ga['rc'] == 0 and ch['agree'] == 0 and ch['chosen'] == c['truth'] != c['predicted']
    assert ga['status_prune'] == 0 and ga['prune_stats'][3] == 0 and ga['n_after'] == w.n == ga['P'].shape[0]
    # the same frame without prune tracks and with n_remove = 0: the first update's results and P bit for bit, and the factor behind P
    gb = frame(upd2, c, remove=[], arm=False, prune=None)
    same_outputs(ga, gb, ('dx', 'gamma', 'accept', 'stats', 'status_first', 'P'))
    next_frame_same(upd, upd2, c)
    # the second half again with the device's choice, on the host's incremented poses: where the reference chain ends when its clones
    # are chosen on the post-update poses
    truth = ch['chosen']
    frame(upd, c)
    prune = cc.prune_for(c, truth)
    win2, applied, _ = mirror_frame.increment_window(prune, ga['dx'], w.flags)
    assert applied
    none = tc.select_tracks(win2, np.zeros(win2.F, bool))
    g2 = upd.io_step_frame(none, None, None, False, None, 1, win2, 0, truth)
    table = mirror.chi2_table(w.flags.chi2_prob)
    ref = mirror_frame.step_frame(w.P, dict(w=c['first'], prune=prune, remove=truth), 1, 1, augment=False, table=table)
    errs = dict(P=rel(upd.cov_get(), ref['P']), prune_dx=rel(g2['prune_dx'], ref['prune_dx']), dx=rel(ga['dx'], ref['dx']))
    print(name, 're-issued second half', errs)
    assert g2['rc'] == 0 and g2['prune_stats'][3] == 1 and g2['n_after'] == ref['n_after'] == w.n - 12
    assert np.array_equal(g2['prune_accept'], ref['prune_accept'])
    assert all(e < TOL for e in errs.values()), errs


# ---- combinations --------------------------------------------------------------------------------------------------------------------------
def _forced(thr):
    """thresholds that force the verdict whatever the poses: tiny -> nothing taken ({0, 1}), huge -> both taken ({N-3, N-2})"""
    return dict(rotation_threshold=thr, translation_threshold=thr)


@pytest.mark.parametrize('thr', [1e-9, 1e3], ids=['agree', 'differ'])
def test_beside_the_imu_arming(built, thr):
    """orcvio_msckf_io_propagate_imu AND the choice on one frame: bit for bit the frame given Phi, Q of the stand-alone propagation with
    the same choice armed (the idiom of tests/test_gpu_prune_tri.py)"""
    import imu_cases as ic
    fl = synth.Flags(use_larvio=1)
    w = synth.make_window(N=8, F=12, seed=3, track_len=(5, 8), flags=fl)
    P0 = np.ascontiguousarray(synth.make_window(N=7, F=1, seed=5, flags=fl).P)
    sub = synth.subset_tracks(w, [0, 1], min_obs=2)
    prune = tc.select_tracks(sub, np.diff(sub.obs_ptr) >= 2)
    assert prune.F >= 3
    case = ic.make_case('larvio', 10, n=22, seed=52, rate=200.0, skipped=1, beyond=2)
    cfg, state, prev = ic.to_capi(case)
    cam = mc.cam_records(w.R_b2w, w.t_b_w, w.R_b2c[-1], w.t_c_b[-1])
    kw = dict(cam_poses=cam, R_imu_cam0=w.R_b2c[-1], t_cam0_imu=w.t_c_b[-1], **_forced(thr))
    aux = capi.MsckfUpdater(device=0, max_clones=2, max_features=16, max_observations=256)
    a, b = _handle(), _handle()
    try:
        aux.cov_set(np.eye(22))
        pq = aux.cov_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'], want_PhiQ=True)
        a.cov_set(P0); b.cov_set(P0)
        cfg, state, prev = ic.to_capi(case)
        a.io_propagate_imu(cfg, state, prev, case['samples'], case['time_bound'])
        ga = a.io_step_frame(w, None, None, True, None, 1, prune, True, [0, 1], choose_clones=kw)
        gb = b.io_step_frame(w, pq['Phi'], pq['Q'], True, None, 1, prune, True, [0, 1], choose_clones=kw)
        assert gb['rc'] == 0 and gb['stats'][3] == 1 and gb['choice']['evaluated'] == 1
        assert gb['choice']['agree'] == int(thr < 1) and gb['choice']['chosen'] == ([0, 1] if thr < 1 else [5, 6])
        assert gb['prune_stats'][3] == int(thr < 1) and gb['n_after'] == w.n - (12 if thr < 1 else 0)
        same_outputs(ga, gb, OUTS)
        for k in ('chosen', 'compared', 'taken', 'agree'):
            assert ga['choice'][k] == gb['choice'][k]
        assert same_bits(ga['choice']['angle'], gb['choice']['angle']) and same_bits(ga['choice']['distance'], gb['choice']['distance'])
        assert same_bits(a.cov_get(), b.cov_get())
    finally:
        a.close(); b.close(); aux.close()


@pytest.mark.parametrize('thr', [1e-9, 1e3], ids=['agree', 'differ'])
def test_beside_the_prune_triangulation(upd, upd2, thr):
    case = ('n12', 'euroc', 'oldest', 1)
    w = pc.window(case[0], case[1])
    sp, remove = pc.reference(case)['sp'], pc.remove_sets(w.N)[case[2]]
    hidden = dataclasses.replace(sp['prune'], p_w=np.full((sp['prune'].F, 3), np.nan))
    cam = mc.cam_records(w.R_b2w, w.t_b_w, w.R_b2c[-1], w.t_c_b[-1])
    kw = dict(cam_poses=cam, R_imu_cam0=w.R_b2c[-1], t_cam0_imu=w.t_c_b[-1], **_forced(thr))
    upd.cov_set(w.P); upd2.cov_set(w.P)
    ga = upd.io_step_frame(sp['first'], None, None, False, None, 1, hidden, 1, remove, triangulate_prune=(sp['tri'], None), choose_clones=kw)
    ga['P'] = upd.cov_get()
    if thr < 1:
        gb = upd2.io_step_frame(sp['first'], None, None, False, None, 1, hidden, 1, remove, triangulate_prune=(sp['tri'], None))
        gb['P'] = upd2.cov_get()
        assert ga['choice']['agree'] == 1 and ga['choice']['chosen'] == remove and ga['prune_stats'][3] == 1
        same_outputs(ga, gb)
        for k in ga['prune_tri']:
            assert same_bits(ga['prune_tri'][k], gb['prune_tri'][k]), k
    else:
        gb = upd2.io_step_frame(sp['first'], None, None, False, None, 1, None, 0, [])
        gb['P'] = upd2.cov_get()
        assert ga['choice']['agree'] == 0 and ga['choice']['chosen'] == [w.N - 3, w.N - 2]
        assert ga['status_prune'] == 0 and ga['prune_stats'][3] == 0 and ga['n_after'] == w.n
        same_outputs(ga, gb, ('dx', 'gamma', 'accept', 'stats', 'P'))
        assert ga['prune_tri']['valid'].any()   # (the triangulation block is filled whatever becomes of the update)


@pytest.mark.parametrize('thr', [1e-9, 1e3], ids=['agree', 'differ'])
def test_with_lost_and_re_anchored_in_state_features(built, thr):
    """io_step_frame_ex: a lifecycle frame with a lost slot, two anchor changes and a prune update.  Agreement: every output and the
    anchor changes' results are the unarmed frame's bits.  Disagreement: the anchor change is not applied -- P is that of the frame
    without changes, without prune tracks and with n_remove = 0."""
    frames, P0 = synth.make_lifecycle_stream(synth.Flags(**tc.EUROC))
    k = next(i for i, fr in enumerate(frames) if fr['lost'] and len(fr['changes']) >= 2 and fr['prune'] is not None and fr['prune'].F <= 40)
    fr = frames[k]
    w = fr['w']
    assert list(fr['remove']) == [0, 1] and w.N >= 6
    cam = mc.cam_records(w.R_b2w, w.t_b_w, fr['R_b2c'], fr['t_c_b'])
    kw = dict(cam_poses=cam, R_imu_cam0=fr['R_b2c'], t_cam0_imu=fr['t_c_b'], **_forced(thr))
    a, b = _handle(), _handle()

    def step(u, f, choose=None, **over):
        u.set_extra_states(f['w'].n_extra)
        args = dict(win=f['w'], Phi=f['Phi'], Q=f['Q'], augment=True, slam=f['slam'], idp_dim=1, prune=f['prune'], prune_apply_dx=0, remove=f['remove'],
                    n_feature_states=f['n_feature_states'], lost=f['lost'], changes=f['changes'], R_b2c=f['R_b2c'], t_c_b=f['t_c_b'], literal_3d=0,
                    choose_clones=choose)
        args.update(over)
        return u.io_step_frame_ex(**args)
    try:
        for u in (a, b):
            u.set_ekf_rows_mode(True)
            u.cov_set(P0)
            for f in frames[:k]:
                step(u, f)
        ga = step(a, fr, kw)
        assert ga['rc'] == 0 and ga['choice']['evaluated'] == 1 and ga['status_changes'] == 0 and ga['repaired'] == 0
        if thr < 1:
            gb = step(b, fr)
            assert ga['choice']['agree'] == 1 and ga['prune_stats'][3] == 1
            same_outputs(ga, gb, OUTS + ('new_param', 'new_inv_depth', 'status_changes'))
        else:
            gb = step(b, fr, prune=None, changes=(), remove=[])
            assert ga['choice']['agree'] == 0 and ga['choice']['chosen'] == [w.N - 3, w.N - 2]
            assert ga['status_prune'] == 0 and ga['prune_stats'][3] == 0
            same_outputs(ga, gb, ('dx', 'gamma', 'accept', 'stats', 'n_after'))
        assert same_bits(a.cov_get(), b.cov_get())
    finally:
        a.close(); b.close()


# ---- the unfused form, the repair path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['n20_10_agree', 'n20_10_differ'])
@pytest.mark.parametrize('off', ['ORCVIO_STEP_FUSED', 'ORCVIO_LA_SPIN'])
def test_unfused_and_repaired_frames_report_the_same_bits(upd, monkeypatch, off, name):
    """ORCVIO_STEP_FUSED=0 (diagnostics build): the pose step as a launch of its own in front of k_clone_choice.  ORCVIO_LA_SPIN=0: the
    look-ahead waits give up and both updates run again the safe way, the choice with them -- the same launch, the same bits."""
    c = cc.case(name)
    want = frame(upd, c)
    monkeypatch.setenv(off, '0')
    u = _handle(debug_hooks=off == 'ORCVIO_STEP_FUSED')
    monkeypatch.delenv(off)
    try:
        got = frame(u, c)
        print(off, name, 'repaired', got['repaired'])
        assert got['repaired'] == (2 if off == 'ORCVIO_LA_SPIN' else 0)
        against_mirror(got, c, True, what=off + '=0 ' + name)
        assert got['choice']['agree'] == int(c['agree']) and got['n_after'] == want['n_after'] and got['prune_stats'][3] == want['prune_stats'][3]
        if off == 'ORCVIO_STEP_FUSED':   # (the same update launches: the same dx, and so the same figures)
            assert same_bits(got['dx'], want['dx'])
            assert same_bits(got['choice']['angle'], want['choice']['angle']) and same_bits(got['choice']['distance'], want['choice']['distance'])
        if not c['agree']:
            assert got['P'].shape[0] == c['w'].n and rel(got['P'], want['P']) < TOL
    finally:
        u.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def _refused(code, call, *a, **kw):
    with pytest.raises(capi.MsckfError) as e:
        call(*a, **kw)
    assert e.value.code == code, (e.value.code, code)


def _frame_on_open_arena(u, first, prune, apply_dx, remove):
    """orcvio_msckf_io_step_frame on the arena as it stands (the binding's io_step_frame opens the arena itself, which drops an arming)"""
    import ctypes as C
    st = capi.FrameStep()
    st.leg_dim = int(first.flags.leg_dim)
    st.augment = 0
    keep = []
    if prune is not None:
        arrs = [np.ascontiguousarray(prune.p_w, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(prune.obs_ptr, dtype=np.int32),
                np.ascontiguousarray(prune.obs_clone, dtype=np.int32), np.ascontiguousarray(prune.obs_z, dtype=np.float64)]
        tr = capi.MsckfTracks(int(prune.F), arrs[0].ctypes.data_as(C.POINTER(C.c_double)), arrs[1].ctypes.data_as(C.POINTER(C.c_int32)),
                              arrs[2].ctypes.data_as(C.POINTER(C.c_int32)), arrs[3].ctypes.data_as(C.POINTER(C.c_double)), None)
        keep += arrs + [tr]
        st.prune_tracks = C.pointer(tr)
    st.prune_apply_dx = int(apply_dx)
    rm = np.ascontiguousarray(list(remove), dtype=np.int32)
    if len(rm):
        st.remove_clones = rm.ctypes.data_as(C.POINTER(C.c_int32))
    st.n_remove = len(rm)
    res = capi.FrameResult()
    rc = u.lib.orcvio_msckf_io_step_frame(u.h, C.byref(st), C.byref(res))
    if rc != 0:
        raise capi.MsckfError(rc, 'orcvio_msckf_io_step_frame')
    return dict(rc=rc, dx=np.ctypeslib.as_array(res.dx, shape=(first.n,)).copy(), n_after=int(res.n_after),
                prune_stats=np.array(res.prune_stats[:], dtype=np.int32))


def test_refusals(built):
    c = cc.case('n7_10_agree')
    w, first, pred = c['w'], c['first'], c['predicted']
    prune = cc.prune_for(c, pred)
    kw = cc.choose_kwargs(c)
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=64, max_observations=600)

    def open_arena(win=first):
        io = u.io_begin(win.flags, win.N, win.F, int(win.obs_ptr[-1]), with_P=2)
        u.io_fill(io, win, with_P=False)
    try:
        _refused(INVALID, u.io_choose_clones, **kw)   # no open arena
        want = frame(u, c)
        _refused(INVALID, u.io_choose_clones, **kw)   # the frame has closed it
        u.cov_set(w.P)
        P0 = u.cov_get()
        open_arena()
        bad_cam = c['cam_pre'].copy(); bad_cam[3, 10] = np.nan
        bad_R = np.array(c['ext'][0]); bad_R[1, 1] = np.inf
        bad_t = np.array(c['ext'][1]); bad_t[2] = np.nan
        arm_refusals = [dict(rotation_threshold=0.0), dict(rotation_threshold=-1.0), dict(translation_threshold=0.0), dict(rotation_threshold=np.nan),
                        dict(translation_threshold=np.inf), dict(cam_poses=bad_cam), dict(cam_poses=False), dict(R_imu_cam0=bad_R), dict(t_cam0_imu=bad_t)]
        for over in arm_refusals:   # nothing armed: the frame behind them is the unarmed one
            _refused(INVALID, u.io_choose_clones, **dict(kw, **over))
        plain = _frame_on_open_arena(u, first, prune, 1, [0, 3])   # (not the prediction and not checked: nothing is armed)
        assert plain['rc'] == 0 and plain['n_after'] == w.n - 12
        # a pending io_submit
        u.cov_set(w.P)
        open_arena()
        u.io_submit(False, False)
        _refused(INVALID, u.io_choose_clones, **kw)
        u.io_collect()
        assert same_bits(u.cov_get(), P0)
        # N < 6
        w5 = synth.make_window(N=5, F=12, seed=2, track_len=(2, 5), flags=w.flags)
        u.cov_set(w5.P)
        open_arena(w5)
        _refused(INVALID, u.io_choose_clones, **dict(kw, cam_poses=c['cam_pre'][:5]))
        # in the frame call: nothing done, the arming stands
        u.cov_set(w.P)
        for rm, pr in (([0], prune), ([0, 1, 2], prune), ([1, 2], prune), ([0, 5], prune), (pred, None)):
            open_arena()
            blk = u.io_choose_clones(**kw)
            _refused(INVALID, _frame_on_open_arena, u, first, pr, 1, rm)
            assert same_bits(u.cov_get(), P0)
            got = _frame_on_open_arena(u, first, prune, 1, pred)   # the arming stands: a good frame behind the refused one is checked
            ch = capi.MsckfUpdater.choice_dict(blk)
            assert ch['evaluated'] == 1 and ch['agree'] == 1 and ch['chosen'] == pred
            assert same_bits(got['dx'], want['dx']) and same_bits(u.cov_get(), want['P'])
            u.cov_set(w.P)
        # a new io_begin drops the arming
        open_arena()
        blk = u.io_choose_clones(**kw)
        got = frame(u, c, remove=[0, 3] if pred != [0, 3] else [0, 1], arm=False)
        assert got['rc'] == 0 and got['n_after'] == w.n - 12   # (not checked: another set than the device would choose goes through)
        # a communicator on the handle
        u.comm_init(capi.comm_unique_id(), 0, 1)
        u.cov_set(w.P)
        u.io_begin(first.flags, first.N, first.F, int(first.obs_ptr[-1]), with_P=False)
        _refused(INVALID, u.io_choose_clones, **kw)
        u.comm_destroy()
    finally:
        u.close()
