"""The in-place update reads the host-derived index lists (clone_obs, clone_ptr) where the host wrote them, in the pinned arena, instead
of pulling them into device memory by a launch of their own (lists_in_place_active; orcvio_msckf_counters [11]).

The reference of every case is the staged form on the same handle -- upload + run_update + download: one copy of the whole arena, HBM
lists, the same kernels -- and every comparison with it is bit for bit.  Every case runs the in-place call four times (plain launch, plain
launch + capture, two replays of the captured graph) and looks at the counter.  Shapes: the smallest at which the index paths differ.

The issue's N = 6 case asks for tracks of 1..6 observations AND a clone nobody observes; a 6-observation track of a 6-clone window sees
every clone, so the case is two windows of that shape: 'n6_ragged' (1..5 observations, clone 4 unobserved, and the rest of the list) and
'n6_full_track' (the same with a 6-observation track instead of the 5-observation one)."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import oracle
from helpers import rel
import tri_io_cases as tc

pytestmark = pytest.mark.gpu
KEYS = ('dx', 'P_new', 'gamma', 'accept')


def _pick(full, clone_lists, lead=()):
    """A window of the tracks of `full` (every track seen in every clone) restricted to the listed clones, in the listed order, behind
    `lead` leading observations (clone indices) that no track owns: obs_ptr[0] = len(lead)."""
    N = full.N
    cl, z, zv, ptr = list(lead), [full.obs_z[k] for k in range(len(lead))], [full.obs_zvel[k] for k in range(len(lead))], [len(lead)]
    for j, ids in enumerate(clone_lists):
        for i in ids:
            cl.append(i); z.append(full.obs_z[j * N + i]); zv.append(full.obs_zvel[j * N + i])
        ptr.append(len(cl))
    return dataclasses.replace(full, obs_ptr=np.array(ptr, np.int32), obs_clone=np.array(cl, np.int32),
                               obs_z=np.array(z, np.float64).reshape(-1, 2), obs_zvel=np.array(zv, np.float64).reshape(-1, 2))


def _without_lead(w):
    """the same tracks without the leading observations (what the oracle is given)"""
    o = int(w.obs_ptr[0])
    return dataclasses.replace(w, obs_ptr=(w.obs_ptr - o).astype(np.int32), obs_clone=w.obs_clone[o:].copy(), obs_z=w.obs_z[o:].copy(),
                               obs_zvel=w.obs_zvel[o:].copy())


# tracks of the N = 6 windows: a non-consecutive one (clone_obs a true permutation, no run), a single observation (the dead-track branch
# writes its zero rows through obs_pos), clone 4 (ragged) / clone 1 (ragged_b) unobserved: an empty clone item
N6 = {
    'n6_ragged': ([(0, 2, 5), (1,), (2, 3), (0, 1, 2, 3), (0, 1, 2, 3, 5)], (3, 0)),
    'n6_ragged_b': ([(0, 3, 4), (5,), (4, 5), (2, 3, 4, 5), (0, 2, 3, 4, 5)], (2, 5)),   # the same lengths, other lists (fresh lists on replay)
    'n6_full_track': ([(0, 2, 5), (1,), (2, 3), (0, 1, 2, 3), (0, 1, 2, 3, 4, 5)], (3, 0)),
}


def _window(name):
    if name in N6:
        lists, lead = N6[name]
        return _pick(synth.make_window(N=6, F=5, seed=11 + len(name)), lists, lead)
    if name == 'n3_f1':        # one track of three observations: the second team idles, the clone items fall to workgroups without tracks
        return synth.make_window(N=3, F=1, seed=5)
    if name == 'n20_f120':     # config 1's shape
        return synth.make_window(N=20, F=120, seed=2, track_len=(3, 6))
    if name == 'n30_f37':      # n = 202, an odd track count, the look-ahead front with far workgroups
        return synth.make_window(N=30, F=37, seed=4)
    if name == 'n20_f40':      # (the shape change's other F)
        return synth.make_window(N=20, F=40, seed=6, track_len=(3, 6))
    raise KeyError(name)


CASES = ['n3_f1', 'n6_ragged', 'n6_full_track', 'n20_f120', 'n30_f37']


def _handle():
    return capi.MsckfUpdater(device=0, max_clones=32, max_features=128, max_observations=4096)


@pytest.fixture(scope='module')
def upd(built):
    u = _handle()
    yield u
    u.close()


_REFS = {}


def _staged(u, name):
    """upload + run_update + download of the case on this handle (computed once per case, kept unchanged)"""
    if name not in _REFS:
        u.upload(_window(name))
        u.run_update()
        _REFS[name] = u.download()
    return _REFS[name]


def _io(u, win, begin=True, io=None, want_P=True, commit=False):
    if begin:
        io = u.io_begin(win.flags, win.N, win.F, int(win.obs_ptr[-1]), with_P=True)
    u.io_fill(io, win)
    u.io_update(want_P=want_P, commit=commit)
    return dict(dx=io['dx'].copy(), P_new=io['P_out'].copy(), gamma=io['gamma'].copy(), accept=io['accept'].copy()), io


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)   # (a track without rows: gamma = NaN by contract)


def _check(got, ref):
    for k in KEYS:
        assert _eq(got[k], ref[k]), k


def _count(u):
    return u.counters()['lists_in_place']


def test_window_shapes_are_what_the_cases_are_for():
    w = _window('n6_ragged')
    assert w.obs_ptr[0] == 2 and sorted(np.diff(w.obs_ptr)) == [1, 2, 3, 4, 5] and 4 not in w.obs_clone[2:]
    assert sorted(np.diff(_window('n6_ragged_b').obs_ptr)) == [1, 2, 3, 4, 5] and np.diff(_window('n6_full_track').obs_ptr).max() == 6
    assert _window('n30_f37').n == 202 and _window('n3_f1').F == 1


@pytest.mark.parametrize('name', CASES)
def test_in_place_lists_equal_the_staged_form_bit_for_bit(upd, name):
    win = _window(name)
    ref = _staged(upd, name)
    assert np.isfinite(ref['dx']).all() and ref['accept'].any()
    c0, r0 = _count(upd), upd.counters()['graph_replays']
    for it in range(4):
        got, _ = _io(upd, win)
        _check(got, ref)
        assert _count(upd) == c0 + it + 1
    assert upd.counters()['graph_replays'] >= r0 + 1   # (the captured graph holds the arena's pointers)


def test_oracle_on_the_ragged_window(upd):
    win = _window('n6_ragged')
    ref = oracle.msckf_update(_without_lead(win), want_blocks=False, want_K=False)
    got, _ = _io(upd, win)
    assert np.array_equal(got['accept'], ref['accept'])
    fin = np.isfinite(ref['gamma'])
    assert np.array_equal(np.isfinite(got['gamma']), fin) and fin.any()
    assert rel(got['gamma'][fin], ref['gamma'][fin]) < 1e-9       # tests/test_gpu_parity.py's bars
    assert rel(got['dx'], ref['dx']) < 1e-6 and rel(got['P_new'], ref['P_new']) < 1e-6


def test_replayed_graph_reads_the_lists_the_host_has_just_rewritten(upd):
    """two windows of one shape (N, F, observations, longest track, rows) with different per-clone lists, written into the arena one after
    the other without a new io_begin: one signature, one graph, and each call's results are its own window's"""
    wa, wb = _window('n6_ragged'), _window('n6_ragged_b')
    ra, rb = _staged(upd, 'n6_ragged'), _staged(upd, 'n6_ragged_b')
    assert not _eq(ra['dx'], rb['dx'])
    c0, r0 = _count(upd), upd.counters()['graph_replays']
    got, io = _io(upd, wa)
    _check(got, ra)
    for it in range(6):
        w, r = (wb, rb) if it % 2 == 0 else (wa, ra)
        got, _ = _io(upd, w, begin=False, io=io)
        _check(got, r)
    assert _count(upd) == c0 + 7 and upd.counters()['graph_replays'] >= r0 + 3


def test_shape_change_between_two_calls(upd):
    ra, rb = _staged(upd, 'n20_f120'), _staged(upd, 'n20_f40')
    c0 = _count(upd)
    for name, ref in (('n20_f120', ra), ('n20_f40', rb), ('n20_f120', ra), ('n20_f40', rb)):
        got, _ = _io(upd, _window(name))
        _check(got, ref)
    assert _count(upd) == c0 + 4


@pytest.mark.parametrize('name', ['n6_ragged', 'n20_f120'])
def test_staged_run_behind_an_in_place_update_pulls_the_lists_first(upd, name):
    """io_update, then run_update + download with no upload in between: the HBM lists are an earlier upload's (another window's here) until
    the staged launch sequence pulls them"""
    ref = _staged(upd, name)
    other = 'n6_ragged_b' if name == 'n6_ragged' else 'n20_f40'
    upd.upload(_window(other))   # (what stands in HBM when the in-place update starts)
    c0 = _count(upd)
    got, _ = _io(upd, _window(name))
    _check(got, ref)
    assert _count(upd) == c0 + 1
    for _ in range(3):           # (the first pulls; the others find the lists fresh, then replay the staged graph)
        upd.run_update()
        _check(upd.download(), ref)


def test_repair_inside_the_call_feeds_the_forked_kernels_the_right_lists(built, upd, monkeypatch):
    """ORCVIO_LA_SPIN = 0 (the switch of tests/test_gpu_robustness.py): every bounded wait on another workgroup gives up at once, the
    launch flags itself and the update is run again on the forked path inside the same call -- k_feature / k_gram_pair on the HBM lists,
    which the in-place attempt had not pulled.  The bars are that test's: 1e-10 on dx, 1e-12 on P+ against the unrepaired update."""
    name = 'n30_f37'
    win, ref = _window(name), _staged(upd, name)
    monkeypatch.setenv('ORCVIO_LA_SPIN', '0')
    u = _handle()
    try:
        u.upload(_window('n20_f40'))   # (stale lists of another shape in HBM)
        for it in range(3):
            c0 = _count(u)
            got, _ = _io(u, win)
            assert u.counters()['front_fallbacks'] == it + 1 and _count(u) == c0 + 1
            assert _eq(got['accept'], ref['accept']) and rel(got['gamma'], ref['gamma']) < 1e-10
            assert rel(got['dx'], ref['dx']) < 1e-10 and rel(got['P_new'], ref['P_new']) < 1e-12
    finally:
        u.close()


def test_materialised_stack_keeps_the_pull(upd):
    name = 'n6_ragged'
    win, ref = _window(name), _staged(upd, name)
    upd.set_materialize_stack(True)
    try:
        c0 = _count(upd)
        for _ in range(3):
            got, _ = _io(upd, win)
            _check(got, ref)
        assert _count(upd) == c0
    finally:
        upd.set_materialize_stack(False)
    got, _ = _io(upd, win)
    _check(got, ref)
    assert _count(upd) == c0 + 1


def test_thin_update_keeps_the_pull(upd):
    """three projected rows, P+ not asked for: the direct form of a thin stack (another algorithm: 1e-9, tests/test_gpu_stream.py's bar
    for it), committed in the launch"""
    name = 'n3_f1'
    win, ref = _window(name), _staged(upd, name)
    c0 = _count(upd)
    for _ in range(3):
        got, _ = _io(upd, win, want_P=False, commit=True)
        assert _eq(got['accept'], ref['accept']) and rel(got['dx'], ref['dx']) < 1e-9 and rel(upd.cov_get(), ref['P_new']) < 1e-9
    assert _count(upd) == c0
    got, _ = _io(upd, win)   # (P+ to the host: the square-root form, lists in place)
    _check(got, ref)
    assert _count(upd) == c0 + 1


def test_armed_update_keeps_the_pull(upd):
    """orcvio_msckf_io_triangulate: the armed update, every track valid, against the staged form at the positions the device made"""
    w, _, _ = tc.window_case('small24')

    def armed(win):
        io = upd.io_begin(win.flags, win.N, win.F, int(win.obs_ptr[-1]), with_P=True)
        upd.io_fill(io, win)
        io['p_w'][:] = np.nan
        tri = upd.io_triangulate(None, None)
        upd.io_update(True, False)
        return dict(dx=io['dx'].copy(), P_new=io['P_out'].copy(), gamma=io['gamma'].copy(), accept=io['accept'].copy()), {k: v.copy() for k, v in tri.items()}
    c0 = _count(upd)
    _, tri = armed(w)
    wv = tc.select_tracks(w, tri['valid'] == 1)
    for _ in range(3):
        got, tri = armed(wv)
        assert tri['valid'].all() and wv.F >= 10
    assert _count(upd) == c0
    upd.upload(dataclasses.replace(wv, p_w=np.ascontiguousarray(tri['p_w'])))
    upd.run_update()
    _check(got, upd.download())
