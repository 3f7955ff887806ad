"""CPU: the case generator of tests/entering_cases.py and its extended-precision reference.  Every generated feature passes its gate
and is well conditioned; the float64 restatement (numpy QR per feature + mirror_hybrid.augment_after_update) agrees with the
reference on every block of every case -- its worst error is what ROW_TOL / TAIL_TOL of the GPU tests are 100 times of."""
import numpy as np
import pytest

from oracle import mirror_hybrid as mh
import entering_cases as ec

IDS = [str(c) for c in ec.CASES]
SLACK = 4.0   # the recorded worst errors were measured with one BLAS; another summation order may move them by a small factor


def test_extended_precision_is_extended():
    assert np.finfo(ec.LD).eps <= 2.0 ** -63


def test_case_list_covers_what_the_kernels_branch_on():
    got = {str(c) for c in ec.CASES}
    for s in ec.SHAPES:
        for d in (1, 3):
            for k in (1, 6):
                assert '%s_d%d_k%d' % (s, d, k) in got
    assert {'small_d3_k20', 'small_d1_k6_fej', 'small_d3_k6_fej', 'small_d3_k6_ldlt'} <= got
    assert all('small_d%d_k6_%s' % (d, j) in got for d in (1, 3) for j in ('orcvio_right', 'orcvio_left', 'kitti_raw'))
    wide = ec.make_case(ec.CaseId('wide', 3, 6))
    assert wide.win.n == 280 and wide.win.n + 1 > 256 and wide.win.n > 224
    assert max(len(ft.obs) for ft in wide.new) == 32                                   # 64 rows = EKF_NEW_MAXROWS
    sch = ec.make_case(ec.CaseId('schmidt', 1, 6))
    assert sorted(ft.anchor for ft in sch.new)[-2:] == [sch.win.N, sch.win.N + 1]     # nuisance anchors
    small = ec.make_case(ec.CaseId('small', 3, 6))
    assert any(ft.anchor not in [o[0] for o in ft.obs] for ft in small.new)          # an anchor that does not observe
    assert any(ft.anchor in [o[0] for o in ft.obs][1:] for ft in small.new)           # the anchor's observation is not the first
    assert min(len(ft.obs) for ft in small.new) == 2                                   # 4 rows (d = 3), 2 rows (d = 1) after the drop


@pytest.mark.parametrize('cid', ec.CASES, ids=IDS)
def test_generated_features_pass_the_gate_and_are_well_conditioned(cid):
    case = ec.make_case(cid)
    assert len(case.new) == cid.k
    for i, ft in enumerate(case.new):
        g, ok = mh.msckf_gate_of_feature(case.win, ft)
        assert ok, (i, g)
        H_x, H_f, r = ec.feature_rows(case.win, ft, cid.d)
        assert H_f.shape[0] > cid.d
        c = np.linalg.cond(H_f)
        assert c <= ec.COND_CAP, (i, c)


def measure(cid):
    """(row errors {HH, x, W, A, b}, tail errors {dx_new, P21, P22}) of the float64 restatement against the extended reference."""
    case = ec.make_case(cid)
    w, d = case.win, cid.d
    rows = dict(HH=0.0, x=0.0, W=0.0, A=0.0, b=0.0)
    for ft in case.new:
        H_x, H_f, r = ec.feature_rows(w, ft, d)
        ref = ec.row_invariants_ext(H_x, H_f, r)
        got = ec.split_invariants_ext(*ec.qr_split(H_x, H_f, r))
        for q in rows:
            rows[q] = max(rows[q], ec.block_err(got[q], ref[q]))
    # the tail on the update's own dx and P+ (mirror_hybrid.hybrid_update_full) and the restatement's blocks
    full = mh.hybrid_update_full(w, case.slam, case.new, d, ref_ldlt=cid.ldlt)
    assert full['new_accept'] == list(range(cid.k))
    H_1, H_2, r_1, _, _, _ = ec.restatement_split(case)
    s2 = w.flags.noise_feature ** 2
    dx, P = mh.augment_after_update(full['P_upd'], full['dx_leg'], H_1, ec.block_diag(H_2), r_1, s2, case.tail, ref_ldlt=cid.ldlt)
    ref = ec.tail_ext(H_1, H_2, r_1, full['dx_leg'], full['P_upd'], s2, case.tail, ref_ldlt=cid.ldlt)
    n, sz = w.n, d * cid.k
    assert P.shape == ref['P_aug'].shape == (n + sz, n + sz)
    gb, rb = ec.tail_blocks(P, n, sz, case.tail), ec.tail_blocks(ref['P_aug'], n, sz, case.tail)
    tail = dict(dx_new=float(np.abs(dx[n:].astype(ec.LD) - ref['dx_new']).max() / ref['dx_scale']),
                P21=max(ec.block_err(gb[q], rb[q]) for q in gb if q.startswith('P21')), P22=ec.block_err(gb['P22'], rb['P22']))
    # (the blocks the tail only moves: the restatement copies them)
    for q in gb:
        if not q.startswith('P2'):
            assert np.array_equal(gb[q], rb[q].astype(np.float64)), q
    return rows, tail


@pytest.mark.parametrize('cid', ec.CASES, ids=IDS)
def test_float64_restatement_agrees_with_the_extended_reference(cid):
    rows, tail = measure(cid)
    print('entering-case %s rows %s tail %s' % (cid, {q: '%.2e' % v for q, v in rows.items()}, {q: '%.2e' % v for q, v in tail.items()}))
    assert max(rows.values()) <= SLACK * ec.ROW_WORST, rows
    assert max(tail.values()) <= SLACK * ec.TAIL_WORST, tail
    assert ec.ROW_TOL == 100 * ec.ROW_WORST and ec.TAIL_TOL == 100 * ec.TAIL_WORST


def test_reference_notices_what_it_is_there_to_notice():
    """The three one-line faults of the mutation check, applied to the restatement's float64 blocks: each moves a block by far more
    than the tolerance (the reference is not blind to them)."""
    case = ec.make_case(ec.CaseId('schmidt', 3, 6))
    w, d, k = case.win, 3, 6
    full = mh.hybrid_update_full(w, case.slam, case.new, d)
    H_1, H_2, r_1, _, _, _ = ec.restatement_split(case)
    s2 = w.flags.noise_feature ** 2
    ref = ec.tail_ext(H_1, H_2, r_1, full['dx_leg'], full['P_upd'], s2, case.tail)
    n, sz = w.n, d * k
    _, P = mh.augment_after_update(full['P_upd'], full['dx_leg'], H_1, ec.block_diag(H_2), r_1, s2, case.tail)
    n0 = n - case.tail
    P22 = P[n0:n0 + sz, n0:n0 + sz].copy()
    W = np.linalg.inv(ec.block_diag(H_2).T @ ec.block_diag(H_2))
    wrong = P22 - s2 * (W - np.diag(np.diag(W)))                     # s2 W only where r == c
    assert ec.block_err(wrong, ec.tail_blocks(ref['P_aug'], n, sz, case.tail)['P22']) > 1e3 * ec.TAIL_TOL
    HH = np.linalg.solve(ec.block_diag(H_2), H_1); x = np.linalg.solve(ec.block_diag(H_2), r_1)
    wrong = x + HH @ full['dx_leg']                                  # row[n] + s
    assert float(np.abs(wrong.astype(ec.LD) - ref['dx_new']).max() / ref['dx_scale']) > 1e3 * ec.TAIL_TOL
    ft = case.new[0]                                                 # anchored at nuisance state 0: its H_a block 6 columns off
    H_x, H_f, r = ec.feature_rows(w, ft, d)
    ca = mh.anchor_col(w, ft.anchor)
    moved = H_x.copy()
    moved[:, ca:ca + 6] = 0.0
    moved[:, ca + 6:ca + 12] = H_x[:, ca:ca + 6]
    got = ec.split_invariants_ext(*ec.qr_split(moved, H_f, r))
    assert ec.block_err(got['HH'], ec.row_invariants_ext(H_x, H_f, r)['HH']) > 1e3 * ec.ROW_TOL
