"""The two Cholesky chains of an update, tile by tile, in the update's own call forms (tests/potrf_cases.py has the matrices, the
measures, the references and the bar; tests/test_potrf_cases.py runs the same assertions on a CPU restatement and on mutations):

  k_potrf_reg, forward and reversed (the prior is factored reversed), on graded matrices and on a prior with zero-variance states;
  the dropped-pivot threshold 8 eps * max diag, forward and reversed;
  k_potrf_solve / k_potrf_solve_la with the product's right-hand sides: the strided, reversed read of the prior's factor, the extra
    column g, the 15 tail rows -- with NaN around every input and output;
  a non-positive pivot raises the status word (what ORCVIO_ERR_NOT_SPD rests on) and leaves the handle usable;
  k_front's own factorisation of the prior (the look-ahead chain with far workgroups from six block steps), read back after a real update.

Every figure is printed before it is asserted (pytest -s), in units of u = 2^-52."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import oracle
from helpers import rel
import potrf_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=40, max_features=64, max_observations=1024, debug_hooks=True)
    yield u
    u.close()


_SOLVE_BITS = {}   # (n, nc1, tail, cond) -> the bytes of L and Z from whichever of the three solve kernels ran the case first


def _fig(kernel, what, w, bar):
    print('FIG %s %s %.3f bar %.3f' % (kernel, what, w, bar))


@pytest.mark.parametrize('rev', [0, 1])
@pytest.mark.parametrize('n', pc.FACTOR_N)
def test_potrf_reg_tile_by_tile(upd, n, rev):
    for kind in pc.factor_kinds(n):
        c = pc.factor_case(kind, n, bool(rev))
        L, Dinv, info = capi.debug_potrf(upd, c['X'], tol_rel=c['tol_rel'], rev=bool(rev))
        assert np.abs(np.triu(L, 1)).max() == 0.0
        assert info.tolist() == [len(c['dead']), 0]
        S = pc.from_reversed(L) if rev else L
        w = pc.omega_tiles(S, c['X'], bool(rev))
        _fig('k_potrf_reg', '%s n=%d rev=%d' % (kind, n, rev), w, c['bar'])
        if kind == 'g1e6':   # information only: the inverse-based panel element by element (tests/potrf_cases.py)
            print('INFO k_potrf_reg element-wise %s n=%d rev=%d %.1f' % (kind, n, rev, pc.omega_elementwise(S, c['X'])))
        pc.check_factor(S, c['X'], c['bar'], c['dead'], bool(rev))


@pytest.mark.parametrize('rev', [0, 1])
@pytest.mark.parametrize('n,at', pc.THRESH_SHAPES)
def test_dropped_pivot_threshold(upd, n, at, rev):
    """variance 1e-13 is kept (its column sqrt(1e-13) to one ulp), 1e-16 is dropped: tol = 8 eps * 1 lies between them"""
    X = pc.threshold_case(n, at)
    L, Dinv, info = capi.debug_potrf(upd, X, tol_rel=pc.TOL_PRIOR, rev=bool(rev))
    S = pc.from_reversed(L) if rev else L
    print('FIG k_potrf_reg threshold n=%d at=%d rev=%d kept %.17g want %.17g info %s' % (n, at, rev, np.abs(S[at]).max(), np.sqrt(pc.THRESH_VARS[0]), info.tolist()))
    pc.check_threshold(S, info, at)


@pytest.mark.parametrize('nc1', pc.SOLVE_NC1)
@pytest.mark.parametrize('n', pc.SOLVE_N)
@pytest.mark.parametrize('la', [0, 2, 3])
def test_fused_solve_product_form(upd, la, n, nc1):
    """tail 0 and 15, cond 1e4 and 1e6 (paired, the pairing alternating from case to case: the tail rows never meet the factorisation);
    with tail = 0 the columns of B are bit for bit those of the plain form of the hook (unit strides, no extra column); the three kernels
    apply the panels in the same order and agree bit for bit on every case."""
    flip = (pc.SOLVE_N.index(n) + pc.SOLVE_NC1.index(nc1)) % 2
    kernel = 'k_potrf_solve_la%d' % la if la else 'k_potrf_solve'
    for tail, cond in ((0, (1e4, 1e6)[flip]), (pc.TAIL, (1e6, 1e4)[flip])):
        c = pc.solve_case(n, cond, nc1)
        B = c['B'][:n + tail]
        r = capi.debug_potrf_solve(upd, c['X'], B, la=la, bx=c['bx'], tail=tail, tail_scale=pc.TAIL_SCALE, product_strides=True)
        assert r['info'].tolist() == [0, 0, 0]
        full = np.hstack([B[:n], c['bx'].reshape(n, 1)])
        _fig(kernel, 'factor n=%d cond=%.0e' % (n, cond), pc.omega_tiles(r['L'], c['X']), c['bar_L'])
        _fig(kernel, 'solve n=%d nc1=%d tail=%d cond=%.0e' % (n, nc1, tail, cond), pc.omega_solve(r['L'], r['Z'][:n], full), c['bar_Z'])
        pc.check_solve(r, c['X'], B, c['bx'], tail, pc.TAIL_SCALE, c['bar_L'], c['bar_Z'])
        bits = (r['L'].tobytes(), r['Z'].tobytes())
        assert _SOLVE_BITS.setdefault((n, nc1, tail, cond), bits) == bits
        if tail == 0:
            plain = capi.debug_potrf_solve(upd, c['X'], B, la=la)
            assert plain['info'].tolist() == [0, 0, 0] and plain['outside'] == 0
            assert np.array_equal(plain['L'], r['L']) and np.array_equal(plain['Z'], r['Z'][:, :nc1])


@pytest.mark.parametrize('pos', [0, 16, 99])
def test_non_positive_pivot_raises_the_word(upd, pos):
    """A negative pivot at the first position, at the first of the second tile and at the last: info[1] is raised by both chains, no
    hand-off is lost, and the next factorisation on the same handle is as good as ever."""
    X = pc.negative_pivot_case(pos)
    n = X.shape[0]
    t = pc.tile_chol(X, 0.0)
    assert t['negative'] == [pos]
    L, Dinv, info = capi.debug_potrf(upd, X, tol_rel=0.0)
    assert info[1] >= 1
    L, Dinv, info = capi.debug_potrf(upd, pc.reverse(X), tol_rel=pc.TOL_PRIOR, rev=True)
    assert info[1] >= 1
    B = pc.rhs(n, 33, pos)
    for la in (0, 3):
        r = capi.debug_potrf_solve(upd, X, B, la=la)
        assert r['info'][1] >= 1 and r['info'][2] == 0
        assert r['outside'] == 0
    c = pc.solve_case(112, 1e4, 16)
    for la in (0, 3):
        r = capi.debug_potrf_solve(upd, c['X'], c['B'][:112], la=la, bx=c['bx'], product_strides=True)
        pc.check_solve(r, c['X'], c['B'][:112], c['bx'], 0, 0.0, c['bar_L'], c['bar_Z'])
    g = pc.factor_case('prior', 100, True)
    L, Dinv, info = capi.debug_potrf(upd, g['X'], tol_rel=g['tol_rel'], rev=True)
    assert info.tolist() == [len(pc.DEAD), 0]
    pc.check_factor(pc.from_reversed(L), g['X'], g['bar'], g['dead'], True)


@pytest.mark.parametrize('N', [9, 13, 33])
def test_front_prior_factor(upd, N):
    """chol(P) as k_front computes it inside a real update: n = 76 (five block steps: one workgroup), 100 and 220 (the look-ahead chain
    with far workgroups).  RP holds the factor of the reversed prior: S(i, c) = RP[c, n-1-i]."""
    w = synth.make_window(N=N, F=8, seed=40 + N, track_len=(3, 6))
    n = w.n
    c = pc.factor_case('prior', n, True)
    w = dataclasses.replace(w, P=c['X'].copy())
    got = upd.update_features(w)
    ref = oracle.msckf_update(w, want_blocks=False, want_K=False)
    assert np.array_equal(got['accept'], ref['accept']) and ref['accept'].sum() > 0
    assert rel(got['dx'], ref['dx']) < 1e-6 and rel(got['P_new'], ref['P_new']) < 1e-6
    dims = capi.debug_read(upd, 'dims')
    assert dims['n'] == n and dims['reg_path'] == 1
    RP = capi.debug_read(upd, 'RP')
    S = np.ascontiguousarray(RP[:n, :n][:, ::-1].T)
    w_ = pc.omega_tiles(S, c['X'], True)
    _fig('k_front', 'prior n=%d' % n, w_, c['bar'])
    pc.check_factor(S, c['X'], c['bar'], c['dead'], True)
    Lr = S[::-1, :]   # the stored factor L' of the reversed prior: lower triangular
    assert np.abs(np.triu(Lr, 1)).max() == 0.0
