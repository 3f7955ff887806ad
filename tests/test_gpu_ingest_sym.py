"""The pull of a host P as its upper tile-trapezoid (k_ingest_sym, host/ingest_sym_map.hpp): of every row only the suffix from its
diagonal 16 x 16 tile on crosses the link, the device mirrors it below the diagonal tiles.  For a symmetric P the image in device
memory is bit for bit the linear pull's, so nothing behind it changes; entries BELOW the diagonal tiles are never read.

Tiny windows (F = 4 tracks of up to 3-4 observations -- a window of one or two clones holds tracks that short) at the sizes where the
tiling can go wrong; every check is bit for bit (np.array_equal).  The staged form (upload + run_update + download: one copy-engine
transfer of the whole arena, untouched) is the independent reference of the results: on the parent build the two forms agree bit for
bit at every shape of CASES, so no recorded values are needed."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth

pytestmark = pytest.mark.gpu

# name: (leg_dim, clones, extra states) -> n = leg + 6 N + extra
CASES = {
    'n28': (22, 1, 0),       # two tiles, the last 12 wide
    'n34': (22, 2, 0),       # the last tile two columns = one 16-byte unit
    'n64': (22, 7, 0),       # an exact multiple of 16
    'n70': (22, 8, 0),
    'n52_leg46': (46, 1, 0),
    'n202': (22, 30, 0),     # the benchmark's width
    'n71_odd': (22, 8, 1),   # rows only 8-byte aligned: the linear pull (the documented fallback)
}
EVEN = [c for c in CASES if not c.endswith('odd')]
KEYS = ('dx', 'P_new', 'gamma', 'accept')


def _window(case, seed=3):
    leg, N, extra = CASES[case]
    win = synth.make_window(N=N, F=4, seed=seed, track_len=(3, 4), flags=synth.Flags(leg_dim=leg))
    if extra:
        win = synth.with_extra_states(win, extra, seed=1)
    assert win.n == leg + 6 * N + extra and np.array_equal(win.P, win.P.T)
    return win


def _handle(extra=0):
    u = capi.MsckfUpdater(device=0, max_clones=32, max_features=64, max_observations=1024, debug_hooks=True)
    if extra:
        u.set_extra_states(extra)
    return u


@pytest.fixture(scope='module')
def upd(built):
    u = _handle()
    yield u
    u.close()


@pytest.fixture(scope='module')
def upd_odd(built):
    u = _handle(1)
    yield u
    u.close()


def _tiles(n):
    t = np.arange(n) // 16
    return t[:, None], t[None, :]   # tile of the row, tile of the column


def _poison_lower(P):
    """NaN in every entry below the diagonal tiles"""
    ti, tj = _tiles(P.shape[0])
    Q = P.copy()
    Q[np.broadcast_to(ti > tj, P.shape)] = np.nan
    return Q


def _poison_image(P):
    """... and the two triangles inside the diagonal tiles differ (the strict lower one moved by 1)"""
    n = P.shape[0]
    ti, tj = _tiles(n)
    Q = _poison_lower(P)
    i = np.arange(n)
    Q[np.broadcast_to(ti == tj, P.shape) & (i[:, None] > i[None, :])] += 1.0
    return Q


def _mirror_of_upper_tiles(Q):
    ti, tj = _tiles(Q.shape[0])
    return np.where(tj >= ti, Q, Q.T)


def _io(u, win, P=None, may_refuse=False):
    io = u.io_begin(win.flags, win.N, win.F, int(win.obs_ptr[-1]), with_P=True)
    u.io_fill(io, win)
    if P is not None:
        io['P'][:] = P
    try:
        u.io_update(want_P=True)
    except capi.MsckfError:
        if not may_refuse:
            raise
    return dict(dx=io['dx'].copy(), P_new=io['P_out'].copy(), gamma=io['gamma'].copy(), accept=io['accept'].copy())


def _staged(u, win):
    u.upload(win)
    u.run_update()
    return u.download()


def _eq(a, b):
    """bit for bit; NaN equals NaN: a track of fewer than two observations (every track of a one-clone window) has no rows and the
    library reports gamma = NaN, accept = 0 for it by contract -- _finite() says where a NaN may stand"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _same(a, b, keys=KEYS):
    return all(_eq(a[k], b[k]) for k in keys)


def _finite(r, win):
    """dx and P+ finite; gamma finite exactly for the tracks that have rows (two observations or more)"""
    has_rows = np.diff(win.obs_ptr) >= 2
    return bool(np.isfinite(r['dx']).all() and np.isfinite(r['P_new']).all() and np.array_equal(np.isfinite(r['gamma']), has_rows))


@pytest.mark.parametrize('case', EVEN)
def test_image_of_a_symmetric_prior_is_the_prior(upd, case):
    win = _window(case)
    c0 = upd.counters()['sym_pulls']
    _io(upd, win)
    assert upd.counters()['sym_pulls'] == c0 + 1
    assert np.array_equal(capi.debug_read(upd, 'P'), win.P)


@pytest.mark.parametrize('case', EVEN)
def test_image_of_a_poisoned_prior_is_the_mirror_of_its_upper_tiles(upd, case):
    """NaN below the diagonal tiles never reaches the device; the diagonal tiles arrive as written, both triangles (the update itself
    may refuse such a prior: only the image is looked at)"""
    win = _window(case)
    Q = _poison_image(win.P)
    c0 = upd.counters()['sym_pulls']
    _io(upd, win, Q, may_refuse=True)
    assert upd.counters()['sym_pulls'] == c0 + 1
    img = capi.debug_read(upd, 'P')
    want = _mirror_of_upper_tiles(Q)
    assert np.isfinite(want).all() and not np.array_equal(want, want.T)
    assert np.array_equal(img, want)


@pytest.mark.parametrize('case', EVEN)
def test_results_equal_the_staged_form(upd, case):
    win = _window(case)
    ref = _staged(upd, win)
    c0 = upd.counters()['sym_pulls']
    got = _io(upd, win)
    assert upd.counters()['sym_pulls'] == c0 + 1
    for k in KEYS:
        assert _eq(got[k], ref[k]), k
    assert _finite(got, win)


def test_odd_n_takes_the_linear_pull_and_equals_the_staged_form(upd_odd):
    win = _window('n71_odd')
    assert win.n % 2 == 1
    ref = _staged(upd_odd, win)
    c0 = upd_odd.counters()['sym_pulls']
    got = _io(upd_odd, win)
    assert upd_odd.counters()['sym_pulls'] == c0   # the documented path: n odd -> the linear pull of the whole matrix
    assert np.array_equal(capi.debug_read(upd_odd, 'P'), win.P)
    assert _same(got, ref) and _finite(got, win)
    cp = upd_odd.update_features(win)
    assert upd_odd.counters()['sym_pulls'] == c0 and _same(cp, ref)


@pytest.mark.parametrize('case', EVEN)
def test_poisoned_lower_tiles_in_place_and_copying_forms(upd, case):
    """io_update and update_features on a prior with NaN below the diagonal tiles against the clean prior, bit for bit"""
    win = _window(case)
    Q = _poison_lower(win.P)
    clean = _io(upd, win)
    assert _finite(clean, win)
    assert _same(_io(upd, win, Q), clean)
    c0 = upd.counters()['sym_pulls']
    cp_clean = upd.update_features(win)
    cp = upd.update_features(dataclasses.replace(win, P=Q))
    assert upd.counters()['sym_pulls'] == c0 + 2
    assert _same(cp, cp_clean) and _same(cp, clean) and _finite(cp, win)


@pytest.mark.parametrize('case', ['n70', 'n202'])
def test_poisoned_lower_tiles_object_tracks_and_frame(upd, case):
    """the object update from tracks with a host P, and the one-call frame: the frame runs on the RESIDENT covariance (it takes no host
    P), so the poisoned prior reaches it through the io_update whose commit makes it resident"""
    win = _window(case)
    flags = dataclasses.replace(win.flags, use_larvio=0, use_left_perturbation=0)
    win = dataclasses.replace(win, flags=flags)
    Q = _poison_lower(win.P)
    objs = synth.make_objects(win, n_objects=2, seed=2, sigma_kp=0.004)
    args = (win.R_b2c[0], win.t_c_b[0], True, False, 0)
    c0 = upd.counters()['sym_pulls']
    o_clean = upd.update_object_tracks(flags, win.N, objs, win.P, *args)
    o = upd.update_object_tracks(flags, win.N, objs, Q, *args)
    assert upd.counters()['sym_pulls'] == c0 + 2
    assert _same(o, o_clean) and np.isfinite(o['dx']).all() and np.isfinite(o['P_new']).all() and np.isfinite(o['gamma'])

    def frame(P):
        io = upd.io_begin(win.flags, win.N, win.F, int(win.obs_ptr[-1]), with_P=True)
        upd.io_fill(io, win)
        io['P'][:] = P
        upd.io_update(want_P=False, commit=True)
        f, ob = upd.update_frame(win, flags, objs, *args)
        return f, ob, upd.cov_get()
    f0, ob0, P0 = frame(win.P)
    f1, ob1, P1 = frame(Q)
    small = ('dx', 'gamma', 'accept')
    assert _same(f1, f0, small) and _same(ob1, ob0, small) and np.array_equal(P1, P0)
    assert np.isfinite(f1['dx']).all() and np.isfinite(ob1['dx']).all() and np.isfinite(P1).all()


def test_buffer_reuse_reads_no_stale_tile_of_an_earlier_shape(built, upd):
    w70a, w34, w70b = _window('n70', seed=3), _window('n34', seed=4), _window('n70', seed=5)
    assert not np.array_equal(w70a.P, w70b.P)
    _io(upd, w70a)
    _io(upd, w34)
    got = _io(upd, w70b)
    img = capi.debug_read(upd, 'P')
    fresh = _handle()
    try:
        want = _io(fresh, w70b)
    finally:
        fresh.close()
    assert np.array_equal(img, w70b.P)
    assert _same(got, want) and _finite(got, w70b)


def test_refused_update_returns_the_prior(upd):
    """M not positive definite through an absurd noise scale (sigma^2 = 1e-80 is lost beside L^T A L, whose rank four short tracks
    leave far below the window's), finite P: the update is refused and P_out is the prior, bit for bit"""
    win = _window('n70')
    win = dataclasses.replace(win, flags=dataclasses.replace(win.flags, noise_feature=1e-40))
    io = upd.io_begin(win.flags, win.N, win.F, int(win.obs_ptr[-1]), with_P=True)
    upd.io_fill(io, win)
    with pytest.raises(capi.MsckfError) as e:
        upd.io_update(want_P=True)
    assert e.value.code == 6   # ORCVIO_ERR_NOT_SPD
    assert np.array_equal(io['P_out'], win.P)
