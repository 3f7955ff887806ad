"""CPU tests of the Cholesky-chain cases (tests/potrf_cases.py): the two references against each other, the measure against a planted
error the norm tests miss, the mirror's dropped-pivot threshold, and every assertion of tests/test_gpu_potrf_tiles.py on a CPU
restatement of the call forms -- the mirror's output passes, the same output with one wrong entry fails."""
import numpy as np
import pytest

import potrf_cases as pc
from helpers import rel


def test_long_double_is_wide_enough_or_mpmath_takes_over():
    """The measures need a product with at least 64 bits of mantissa: long double here, mpmath otherwise -- the two agree."""
    assert pc.LD_WIDE == bool(np.finfo(np.longdouble).eps < 1e-18)
    X = pc.graded(17, 17, 1e4)
    L = np.linalg.cholesky(X)
    C = pc._mm_mp(L, L.T)
    assert C.dtype == object
    Rmp = pc._sub_abs(C, X)
    if pc.LD_WIDE:
        Rld = pc.factor_fields(L, X)[0]
        assert np.max(np.abs(Rmp - Rld)) <= 2.0 ** -63 * np.max(np.abs(X)) * 17


def _agree(a, b):
    """each reference within ten times the other's figure -- or within ten times 1 u, the rounding of the stored factor itself: a figure
    below 1 u (LAPACK's 0.06 u at n = 16) is luck, not a property the other reference has to share"""
    return a <= pc.BAR_FACTOR * max(b, 1.0) and b <= pc.BAR_FACTOR * max(a, 1.0)


def test_references_agree_on_the_factor_and_match_the_recorded_figures():
    """LAPACK and the mirror of the tile algorithm agree on every case; their worst figures are within a factor of two of the recorded ones
    (a band, not the figure: numpy's `@` and LAPACK sum in the order of their build)."""
    wa = wb = 0.0
    for n in pc.FACTOR_N:
        for kind in pc.factor_kinds(n, with_1e2=True):
            for rev in (False, True):
                c = pc.factor_case(kind, n, rev)
                assert _agree(c['lapack'], c['mirror']), (kind, n, rev, c['lapack'], c['mirror'])
                wa, wb = max(wa, c['lapack']), max(wb, c['mirror'])
    print('factor, tile-wise backward error in u: LAPACK %.3f, mirror %.3f' % (wa, wb))
    assert 0.5 * pc.REF_FACTOR_LAPACK <= wa <= 2.0 * pc.REF_FACTOR_LAPACK
    assert 0.5 * pc.REF_FACTOR_MIRROR <= wb <= 2.0 * pc.REF_FACTOR_MIRROR


def test_references_agree_on_the_solve_and_match_the_recorded_figures():
    wa = wb = 0.0
    for n in pc.SOLVE_N:
        for cond in (1e4, 1e6):
            for nc1 in pc.SOLVE_NC1:
                c = pc.solve_case(n, cond, nc1)
                assert _agree(c['lapack'], c['mirror']), (n, cond, nc1, c['lapack'], c['mirror'])
                wa, wb = max(wa, c['lapack']), max(wb, c['mirror'])
    print('solve, tile-wise backward error in u: LAPACK %.3f, mirror %.3f' % (wa, wb))
    assert 0.5 * pc.REF_SOLVE_LAPACK <= wa <= 2.0 * pc.REF_SOLVE_LAPACK
    assert 0.5 * pc.REF_SOLVE_MIRROR <= wb <= 2.0 * pc.REF_SOLVE_MIRROR


def test_elementwise_figures_are_information_only():
    """Element by element (no tile maximum), printed and not asserted: the inverse-based panel is as good as LAPACK's triangular solve
    when inv(L11) comes from substitution, and loses componentwise backward stability on graded matrices when it comes from an LU-based
    inverse (np.linalg.inv)."""
    ea, eb, ec = [], [], []
    for n in pc.FACTOR_N:
        X = pc.graded(n, n, 1e6)
        ea.append(pc.omega_elementwise(pc.lapack_chol(X), X))
        eb.append(pc.omega_elementwise(pc.tile_chol(X)['L'], X))
        ec.append(pc.omega_elementwise(pc.tile_chol(X, inv=np.linalg.inv)['L'], X))
    print('element-wise backward error in u at cond 1e6: LAPACK %.1f .. %.1f, mirror %.1f .. %.1f, mirror with an LU inverse %.1f .. %.1f'
          % (min(ea), max(ea), min(eb), max(eb), min(ec), max(ec)))


@pytest.mark.parametrize('cond', pc.CONDS)
@pytest.mark.parametrize('n', [17, 100, 224])
def test_planted_error_in_the_smallest_states_row_is_seen_by_the_tile_measure_only(n, cond):
    """A relative 1e-9 in the row of the smallest state of LAPACK's factor: the norm comparison of tests/test_gpu_kernels.py still
    passes, the tile-wise measure is far beyond the bar."""
    X = pc.graded(n, n, cond)
    L = np.linalg.cholesky(X)
    bar, a, b = pc.factor_bar(X)
    i = int(np.argmin(np.diag(X)))
    Lb = L.copy()
    Lb[i, :i + 1] *= 1.0 + 1e-9
    assert rel(Lb, L) < 1e-11 and rel(Lb @ Lb.T, X) < 1e-13   # the old bars: blind
    w = pc.omega_tiles(Lb, X)
    print('n %d cond %.0e: references %.2f / %.2f u, bar %.1f u, planted 1e-9 in row %d: %.3g u' % (n, cond, a, b, bar, i, w))
    assert w > bar
    with pytest.raises(AssertionError):
        pc.check_factor(Lb, X, bar)


@pytest.mark.parametrize('n,at', pc.THRESH_SHAPES)
@pytest.mark.parametrize('rev', [False, True])
def test_the_mirror_drops_pivots_at_the_threshold(n, at, rev):
    """tol = 8 eps * largest diagonal entry = 1.8e-15 lies between the variances 1e-13 (kept) and 1e-16 (dropped)."""
    X = pc.threshold_case(n, at)
    assert pc.THRESH_VARS[1] < pc.TOL_PRIOR * np.max(np.diag(X)) < pc.THRESH_VARS[0]
    t = pc.tile_chol(pc.reverse(X) if rev else X, pc.TOL_PRIOR)
    assert t['dropped'] == [n - 1 - (at + 1) if rev else at + 1] and t['negative'] == []
    S = pc.from_reversed(t['L']) if rev else t['L']
    pc.check_threshold(S, [1, 0], at)
    # mutations: the state dropped that should be kept, and the kept one off by more than an ulp
    bad = S.copy()
    bad[at, :] = 0.0
    with pytest.raises(AssertionError):
        pc.check_threshold(bad, [1, 0], at)
    bad = S.copy()
    bad[at, :] *= 1.0 + 4 * pc.U
    with pytest.raises(AssertionError):
        pc.check_threshold(bad, [1, 0], at)
    with pytest.raises(AssertionError):
        pc.check_threshold(S, [2, 0], at)


@pytest.mark.parametrize('pos', [0, 16, 99])
def test_the_negative_pivot_case_fails_at_exactly_that_pivot(pos):
    X = pc.negative_pivot_case(pos)
    t = pc.tile_chol(X, 0.0)
    assert t['negative'] == [pos] and t['dropped'] == [pos]
    t = pc.tile_chol(X, pc.TOL_PRIOR)
    assert t['negative'] == [pos] and t['dropped'] == [pos]
    t = pc.tile_chol(X, drop=False)   # the chain without a pivot test: nothing fails before, everything is NaN behind
    assert t['negative'][0] == pos and np.isfinite(t['L'][:, :pos]).all()


# ---- the device tests' assertions on a CPU restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,n', [('g1e6', 17), ('g1e4', 113), ('prior', 100), ('prior', 209)])
@pytest.mark.parametrize('rev', [False, True])
def test_factor_assertions_on_the_mirror_and_on_mutations(kind, n, rev):
    c = pc.factor_case(kind, n, rev)
    X = c['X']
    t = pc.tile_chol(pc.reverse(X) if rev else X, c['tol_rel'])
    assert len(t['dropped']) == len(c['dead'])
    S = pc.from_reversed(t['L']) if rev else t['L']
    pc.check_factor(S, X, c['bar'], c['dead'], rev)
    if rev:   # the rows of the stored factor taken as they are (S(i, c) = L'(i, c)): not a factor of X
        with pytest.raises(AssertionError):
            pc.check_factor(t['L'], X, c['bar'], c['dead'], rev)
    bad = S.copy()   # one entry of the smallest state's row off by a relative 1e-9
    i = int(np.argmin(np.where(np.diag(X) > 0, np.diag(X), np.inf)))
    j = int(np.argmax(np.abs(bad[i])))
    bad[i, j] *= 1.0 + 1e-9
    with pytest.raises(AssertionError):
        pc.check_factor(bad, X, c['bar'], c['dead'], rev)
    if c['dead']:   # a dropped pivot's column not zero
        bad = S.copy()
        bad[n - 1, pc.dead_columns(n, c['dead'], rev)[0]] = 1e-300
        with pytest.raises(AssertionError):
            pc.check_factor(bad, X, c['bar'], c['dead'], rev)


def _restated(c, tail, ld, **mut):
    """the fused solve in the product's call form, on the host: the mirror's factor, B read through the negative column stride"""
    X, bx = c['X'], c['bx']
    B = c['B'][:X.shape[0] + tail]
    n, nc1 = X.shape[0], B.shape[1]
    t = pc.tile_chol(X)
    buf, base, srow, scol = pc.product_layout(B, ld)
    if 'drop_row' in mut:   # a row lost under the strided indexing: every later row read one row further down
        k = mut['drop_row']
        keep = np.concatenate([buf[:k * ld], buf[(k + 1) * ld:], np.full(ld, np.nan)])
        buf = np.where(np.isnan(keep), 0.0, keep)
    if 'base' in mut:
        base = mut['base']
        buf = np.where(np.isnan(buf), 0.0, buf)
    bxu = np.roll(bx, 1) if mut.get('shift_bx') else bx
    Zg = pc.solve_call(t['L'], t['Linv'], n, buf, base, srow, scol, nc1, bxu, tail, mut.get('tail_scale', pc.TAIL_SCALE))
    if mut.get('write_outside'):
        Zg[n + tail, 0] = 0.0
    ncols = nc1 + 1
    return dict(L=t['L'], Z=Zg[:n + tail, :ncols], info=[0, 0, 0], guard_row=Zg[n + tail], guard_col=Zg[:, ncols], outside=None)


@pytest.mark.parametrize('n,nc1', [(80, 15), (112, 64), (209, 209)])
@pytest.mark.parametrize('tail', [0, pc.TAIL])
def test_solve_assertions_on_the_mirror_and_on_mutations(n, nc1, tail):
    c = pc.solve_case(n, 1e6, nc1)
    X, B, bx = c['X'], c['B'][:n + tail], c['bx']
    args = (X, B, bx, tail, pc.TAIL_SCALE, c['bar_L'], c['bar_Z'])
    pc.check_solve(_restated(c, tail, 288), *args)
    muts = [dict(drop_row=n // 2), dict(base=nc1 - 2), dict(shift_bx=True), dict(write_outside=True)]
    if tail:
        muts += [dict(tail_scale=1.0), dict(drop_row=n + 3)]
    for mut in muts:
        with pytest.raises(AssertionError):
            pc.check_solve(_restated(c, tail, 288, **mut), *args)
    r = _restated(c, tail, 288)   # the extra column not zero in a tail row
    if tail:
        r['Z'][n + 1, nc1] = 1e-300
        with pytest.raises(AssertionError):
            pc.check_solve(r, *args)
