"""orcvio_msckf_io_triangulate: the in-place update (io_update, io_submit / io_collect) triangulating its own tracks on the device.
Reference chain (tests/tri_io_cases.py): the mirror's triangulation with a mode per track, the invalid tracks removed, the oracle's
update at the mirror's positions.  Tolerances: valid / flags identical, positions, dx, P and finite gamma 1e-6 relative
(tests/test_gpu_triangulate.py's TOL), accept identical on kept tracks and 0 on dropped ones, NaN gamma exactly where the
reference drops.  The preconditions of the inputs are tests/test_tri_io_inputs.py's."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import oracle
from helpers import rel
import tri_io_cases as tc
from tri_io_cases import same_bits

pytestmark = pytest.mark.gpu
TOL = tc.TOL
INVALID = 1   # ORCVIO_ERR_INVALID


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=32, max_features=256, max_observations=8192)
    yield u
    u.close()


def _open(u, w, with_P=True, p_w=None):
    io = u.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=with_P)
    u.io_fill(io, w, with_P=with_P)
    if w.F and p_w is not None:
        io['p_w'][:] = p_w
    return io


def _results(io, stats, want_P, tri=None):
    out = dict(dx=io['dx'].copy(), gamma=io['gamma'].copy(), accept=io['accept'].copy(), P=io['P_out'].copy() if want_P else None, stats=stats)
    if tri is not None:
        out['tri'] = {k: v.copy() for k, v in tri.items()}
    return out


def hidden_positions(w, mode):
    """The arena's p_w of an armed update: NaN wherever the device is to make the position."""
    pw = np.array(w.p_w, dtype=np.float64, copy=True).reshape(-1, 3)
    m = np.full(w.F, tc.ALL) if mode is None else np.asarray(mode)
    pw[m != tc.KEEP] = np.nan
    return pw


def armed(u, w, mode=None, cfg=None, want_P=True, commit=False, with_P=True, submit=False):
    io = _open(u, w, with_P, hidden_positions(w, mode))
    tri = u.io_triangulate(cfg, mode)
    if submit:
        u.io_submit(want_P, commit)
        stats = u.io_collect()
    else:
        stats = u.io_update(want_P, commit)
    return _results(io, stats, want_P, tri), io


def plain(u, w, want_P=True, commit=False, with_P=True):
    io = _open(u, w, with_P)
    return _results(io, u.io_update(want_P, commit), want_P)


def check_against_chain(got, w, tri, upd_ref):
    keep = tri['valid'] == 1
    assert np.array_equal(got['tri']['valid'], tri['valid'])
    assert np.array_equal(got['tri']['flags'], tri['flags'])
    errs = {}
    if keep.any():
        errs['p_w'] = rel(got['tri']['p_w'][keep], tri['p_w'][keep])
        assert np.array_equal(got['accept'][keep], upd_ref['accept'])
        errs['gamma'] = tc.gamma_err(got['gamma'][keep], upd_ref['gamma'])
        errs['dx'] = rel(got['dx'], upd_ref['dx'])
        errs['P'] = rel(got['P'], upd_ref['P_new'])
    assert not got['accept'][~keep].any()
    assert np.isnan(got['gamma'][~keep]).all()
    print('worst rel err', errs)
    assert all(e < TOL for e in errs.values()), errs


@pytest.mark.parametrize('name', ['config1', 'mixed80', 'small24'])
def test_armed_triangulation_equals_the_call_of_its_own_bit_for_bit(upd, name):
    """valid, flags, inv_param, cost: every track; p_w: every track the kernel writes a position for (a track without motion keeps
    what stood in HBM: the arena's NaN here, whatever an earlier call left there in the call of its own, which uploads no positions)."""
    w, _, _ = tc.window_case(name)
    own = upd.triangulate(w)
    got, _ = armed(upd, w)
    t = got['tri']
    for k in ('valid', 'flags', 'solution', 'cost'):
        assert same_bits(t[k], own[k]), k
    wrote = own['flags'] != 1
    assert wrote.sum() >= 10 and same_bits(t['p_w'][wrote], own['p_w'][wrote])
    assert np.isnan(t['p_w'][~wrote]).all()


@pytest.mark.parametrize('variant', ['all', 'abl', 'keep'])
@pytest.mark.parametrize('name', ['config1', 'mixed80', 'small24'])
def test_armed_update_against_the_reference_chain(upd, name, variant):
    w, mode = tc.with_modes(name, variant)
    ref = tc.window_reference(name, variant)
    got, _ = armed(upd, w, mode if variant != 'all' else None)
    check_against_chain(got, w, ref['tri'], ref['upd'])
    if variant == 'keep':
        k = mode == tc.KEEP
        assert same_bits(got['tri']['p_w'][k], np.ascontiguousarray(w.p_w[k])) and np.isnan(got['tri']['solution'][k]).all() and np.isnan(got['tri']['cost'][k]).all()


@pytest.mark.parametrize('name', ['mixed80', 'small24'])
def test_all_valid_armed_equals_unarmed_at_the_devices_positions_bit_for_bit(upd, name):
    w, _, _ = tc.window_case(name)
    first, _ = armed(upd, w)
    wv = tc.select_tracks(w, first['tri']['valid'] == 1)
    a, _ = armed(upd, wv)
    assert a['tri']['valid'].all() and wv.F >= 10
    b = plain(upd, dataclasses.replace(wv, p_w=a['tri']['p_w']))
    for k in ('dx', 'gamma', 'accept', 'P'):
        assert same_bits(a[k], b[k]), k
    assert np.array_equal(a['stats'], b['stats'])


def test_every_track_invalid_leaves_the_resident_covariance_alone(upd):
    w, _, _ = tc.window_case('small24')
    upd.cov_set(w.P)
    P0 = upd.cov_get()
    got, _ = armed(upd, w, cfg=dict(translation_threshold=1e3), want_P=False, commit=True, with_P=False)
    assert not got['tri']['valid'].any() and (got['tri']['flags'] == 1).all()
    assert got['stats'][3] == 0 and not got['accept'].any() and np.isnan(got['gamma']).all()
    assert not got['dx'].any()
    assert same_bits(upd.cov_get(), P0)


# name: (make_window arguments, mode of every track, translation_threshold or None).  Two listed observations of neighbouring clones
# lie ~0.14 apart, below the default threshold 0.2: the cases that are to PASS with two observations lower it (both sides alike).
EDGES = {
    'F1': (dict(N=6, F=1, seed=3, track_len=4), tc.ALL, None),
    'odd_F': (dict(N=7, F=13, seed=5, track_len=(2, 7)), tc.ALL, None),
    'track32_N32': (dict(N=32, F=3, seed=2, track_len=32), tc.ALL, None),
    'M2_all': (dict(N=6, F=5, seed=8, track_len=2), tc.ALL, 0.05),
    'M3_all_but_last': (dict(N=6, F=5, seed=8, track_len=3), tc.ALL_BUT_LAST, 0.05),
    'M2_all_but_last': (dict(N=6, F=5, seed=8, track_len=2), tc.ALL_BUT_LAST, 0.05),
}


@pytest.mark.parametrize('name', list(EDGES))
def test_edge_shapes(upd, name):
    from oracle import mirror_triangulate as mt
    kw, md, thr = EDGES[name]
    w = synth.make_window(**kw)
    mode = np.full(w.F, md, np.int32)
    cfg = None if thr is None else mt.OptimizationConfig(translation_threshold=thr)
    tri = tc.mirror_tri(w, mode, cfg)
    keep = tri['valid'] == 1
    got, _ = armed(upd, w, mode, cfg)
    print(name, 'kept', int(keep.sum()), 'of', w.F, 'flags', tri['flags'])
    if name == 'M2_all_but_last':
        assert (got['tri']['flags'] == 1).all() and not got['tri']['valid'].any()
    elif thr is not None:
        assert keep.sum() >= 3   # (two observations do pass)
    if keep.any():
        check_against_chain(got, w, tri, oracle.msckf_update(tc.kept_window(w, tri), want_blocks=False, want_K=False))
    else:
        assert np.array_equal(got['tri']['valid'], tri['valid']) and np.array_equal(got['tri']['flags'], tri['flags'])
        assert got['stats'][3] == 0 and not got['dx'].any() and not got['accept'].any()


def test_no_tracks_armed(upd):
    w = synth.make_window(N=4, F=0, seed=1)
    got, _ = armed(upd, w)
    assert got['stats'][3] == 0 and not got['dx'].any() and got['tri']['valid'].shape == (0,)


def test_the_arming_holds_for_one_update(upd):
    w, _, _ = tc.window_case('mixed80')
    first, io = armed(upd, w)
    assert (first['tri']['valid'] == 0).any()
    io['p_w'][:] = w.p_w
    second = _results(io, upd.io_update(True, False), True)
    ref = plain(upd, w)
    for k in ('dx', 'gamma', 'accept', 'P'):
        assert same_bits(second[k], ref[k]), k
    assert np.array_equal(second['stats'], ref['stats']) and not same_bits(first['dx'], ref['dx'])


@pytest.mark.parametrize('name', ['mixed80', 'small24_abl'])
def test_submit_collect_armed_equals_io_update_armed(upd, name):
    w, mode, _ = tc.window_case(name)
    a, _ = armed(upd, w, mode)
    b, _ = armed(upd, w, mode, submit=True)
    for k in ('dx', 'gamma', 'accept', 'P'):
        assert same_bits(a[k], b[k]), k
    for k in a['tri']:
        assert same_bits(a['tri'][k], b['tri'][k]), k


def _refused(u, *a, **kw):
    with pytest.raises(capi.MsckfError) as e:
        u.io_triangulate(*a, **kw)
    assert e.value.code == INVALID


def test_refusals_leave_outputs_and_arming_untouched(upd):
    w, mode, _ = tc.window_case('small24_abl')
    want, _ = armed(upd, w, mode)
    unarmed = plain(upd, w)
    bad_mode = mode.copy(); bad_mode[3] = 3
    neg_mode = mode.copy(); neg_mode[-1] = -1
    refusals = [dict(mode=bad_mode), dict(mode=neg_mode), dict(cfg=False), dict(cfg=dict(huber_epsilon=float('nan'))),
                dict(cfg=dict(cost_threshold=float('inf'))), dict(cfg=dict(outer_loop_max_iteration=-1))]
    # behind a good arming: the arming (its modes, its config) and the output block stay as they are
    io = _open(upd, w, True, hidden_positions(w, mode))
    tri = upd.io_triangulate(None, mode)
    before = {k: v.copy() for k, v in tri.items()}
    for r in refusals:
        _refused(upd, r.get('cfg'), r.get('mode'))
        assert all(same_bits(tri[k], before[k]) for k in tri)
    got = _results(io, upd.io_update(True, False), True, tri)
    for k in ('dx', 'gamma', 'accept', 'P'):
        assert same_bits(got[k], want[k]), k
    for k in tri:
        assert same_bits(got['tri'][k], want['tri'][k]), k
    # without one: nothing is armed
    io = _open(upd, w)
    for r in refusals:
        _refused(upd, r.get('cfg'), r.get('mode'))
    got = _results(io, upd.io_update(True, False), True)
    for k in ('dx', 'gamma', 'accept', 'P'):
        assert same_bits(got[k], unarmed[k]), k
    # a pending io_submit
    io = _open(upd, w)
    upd.io_submit(True, False)
    _refused(upd)
    upd.io_collect()
    assert same_bits(io['dx'].copy(), unarmed['dx'])
    # no open arena: the call of its own has closed it
    upd.triangulate(w)
    _refused(upd)


def test_refused_without_io_begin_with_objects_and_with_a_communicator(built):
    w, mode, _ = tc.window_case('small24')
    u = capi.MsckfUpdater(device=0, max_clones=8, max_features=64, max_observations=1024)
    try:
        _refused(u)   # no io_begin yet
        # an object update in the arena
        u.cov_set(w.P)
        objs = synth.make_objects(w, n_objects=2, seed=2, sigma_kp=0.004)
        u.update_frame(w, w.flags, objs, w.R_b2c[0], w.t_c_b[0], True, False, 0)
        _refused(u)
        # a communicator on the handle
        u.comm_init(capi.comm_unique_id(), 0, 1)
        io = _open(u, w)
        _refused(u)
        u.comm_destroy()
    finally:
        u.close()
