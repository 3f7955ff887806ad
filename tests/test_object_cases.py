"""CPU: the cases of tests/object_cases.py and their extended-precision reference.  The case list covers the branches it names and
every structural fact it relies on holds; every H_f is well conditioned; the float64 restatement (mirror_objects rows, numpy QR
projection) agrees with the reference on every block of every object -- its worst errors are what ROW_TOL / GRAM_TOL of the GPU tests
are 100 times of; and the reference notices the three faults it is there to notice."""
import numpy as np
import pytest

import object_cases as oc

SLACK = 4.0   # the recorded worst errors were measured with one BLAS; another summation order may move them by a small factor


def test_extended_precision_is_extended():
    assert np.finfo(oc.LD).eps <= 2.0 ** -63


def _in_window(ob):
    return [fr for fr in ob.frames if fr['clone'] >= 0]


def test_case_list_covers_what_the_kernels_branch_on():
    got = {str(c) for c in oc.CASES}
    assert len(got) == len(oc.CASES)
    for K in oc.KS:
        assert 'small_K%d_L_f12' % K in got and 'small_K%d_Rn_f5' % K in got
    for K in (4, 13):
        assert {'small_K%d_R_f12' % K, 'small_K%d_Lc_f12' % K} <= got
        for p in ('nokp', 'first', 'last', 'outside', 'desc'):
            assert 'small_K%d_L_f12_%s' % (K, p) in got
    assert {'small_K4_L_f12_fixD', 'small_K4_L_f5_odd', 'small_K13_L_f3_odd', 'maxf_K4_L_f34_f32', 'maxf_K4_L_f34_f33', 'maxf_K4_L_f12_shared'} <= got
    assert any(c.win == 'leg46' for c in oc.CASES)
    assert oc.FLAGSETS == {'L': (1, 0, 0), 'R': (0, 0, 0), 'Rn': (0, 1, 1), 'Lc': (1, 2, 0)}
    # lanes per frame of k_obj_fused's P1: the smallest power of two >= K + 4
    assert [oc.lpf_of(K) for K in (0, 1, 3, 4, 5, 12, 13, 16)] == [4, 8, 8, 8, 16, 16, 32, 32]
    for K in range(0, 61):
        assert oc.lpf_of(K) >= K + 4 and (K == 0 or oc.lpf_of(K) // 2 < K + 4) and oc.lpf_of(K) & (oc.lpf_of(K) - 1) == 0
    # windows: another cb0 and NA on leg46, 34 clones on maxf
    for name, (leg, N) in dict(small=(22, 12), leg46=(46, 12), maxf=(22, 34)).items():
        c = oc.make_case(next(q for q in oc.CASES if q.win == name))
        assert (c.win.flags.leg_dim, c.win.N) == (leg, N)
    # K >= 17 leaves the fused kernel, K = 29 and 34 leave a wavefront half and give NOP = 96 and 112
    for K, nop in ((17, 64), (29, 96), (34, 112)):
        c = oc.make_case(oc.CaseId(K, 'L', frames=12))
        assert not c.fused and -(-(9 + 3 * K) // 16) * 16 == nop
    assert 29 + 4 > 32 and 9 + 3 * 34 == 111
    # object_rows_body leaves its LDS staging: ldhf = round_up(ncol + 1, 16) > 48 or 2 K + 4 > 28
    assert all((-(-(10 + 3 * K) // 16) * 16 > 48 or 2 * K + 4 > 28) == (K >= 13) for K in oc.KS)
    # the eligibility boundary
    f32, f33, sh = (oc.make_case(next(q for q in oc.CASES if q.pat == p)) for p in ('f32', 'f33', 'shared'))
    assert len(_in_window(f32.objs[0])) == 32 == oc.OBJ_FUSED_MAXF and f32.fused
    assert len(_in_window(f33.objs[0])) == 33 and not f33.fused
    cl = [fr['clone'] for fr in _in_window(sh.objs[0])]
    assert len(cl) == 12 and len(set(cl)) == 11 and not sh.fused
    # frame patterns
    for K in (4, 13):
        ob = oc.make_case(oc.CaseId(K, 'L', frames=12, pat='nokp')).objs[0]
        assert sum(1 for fr in _in_window(ob) if np.isnan(fr['zs']).all()) == 1
        ob = oc.make_case(oc.CaseId(K, 'L', frames=12, pat='first')).objs[0]
        assert sum(1 for fr in _in_window(ob) if np.isnan(fr['zs'][0]).all()) == 3 and not any(np.isnan(fr['zs'][1:]).any() for fr in ob.frames)
        ob = oc.make_case(oc.CaseId(K, 'L', frames=12, pat='last')).objs[0]
        assert sum(1 for fr in _in_window(ob) if np.isnan(fr['zs'][K - 1]).all()) == 3 and not any(np.isnan(fr['zs'][:K - 1]).any() for fr in ob.frames)
        ob = oc.make_case(oc.CaseId(K, 'L', frames=12, pat='outside')).objs[0]
        assert [f for f, fr in enumerate(ob.frames) if fr['clone'] < 0] == [0, 6, 11]
        ob = oc.make_case(oc.CaseId(K, 'L', frames=12, pat='desc')).objs[0]
        cl = [fr['clone'] for fr in ob.frames]
        assert cl == sorted(cl, reverse=True) and len(cl) == 12
    # odd: 5 in-window frames at lpf 8 (8 per wavefront), 3 at lpf 32 (2 per wavefront): the last lane group of the last busy wavefront idles
    a, b = oc.make_case(oc.CaseId(4, 'L', frames=5, pat='odd')), oc.make_case(oc.CaseId(13, 'L', frames=3, pat='odd'))
    assert len(_in_window(a.objs[0])) == 5 and 5 % (64 // oc.lpf_of(4)) != 0
    assert len(_in_window(b.objs[0])) == 3 and 3 % (64 // oc.lpf_of(13)) != 0
    # multi: five objects that take the fused kernel together, six that do not (one of 17 keypoints)
    m5, m6 = oc.make_case(oc.MULTI5), oc.make_case(oc.MULTI6)
    assert [len(o.kps) for o in m5.objs] == [0, 3, 12, 13, 16] and m5.fused
    assert [len(o.kps) for o in m6.objs] == [0, 3, 12, 13, 16, 17] and not m6.fused
    assert [len(_in_window(o)) for o in m5.objs] == [5, 5, 3, 3, 3]
    for o in m5.objs:
        assert len(_in_window(o)) % (64 // oc.lpf_of(len(o.kps))) != 0
    for a, b in zip(m5.objs, m6.objs):   # the same five objects
        assert np.array_equal(a.wTo, b.wTo) and np.array_equal(a.kps, b.kps) and len(a.frames) == len(b.frames)


@pytest.mark.parametrize('cid', oc.CASES, ids=oc.IDS)
def test_every_object_is_usable_and_well_conditioned(cid):
    case = oc.make_case(cid)
    assert case.fused == (not any(len(o.kps) > 16 for o in case.objs) and cid.pat not in ('f33', 'shared'))
    for i, (ob, ref) in enumerate(zip(case.objs, oc.reference(cid))):
        hx6, Hf, r, rc = ref['mirror']
        K = len(ob.kps)
        assert Hf.shape[1] == 9 + 3 * K and Hf.shape[0] > Hf.shape[1]                      # rows > cols: the projection exists
        assert Hf.shape[0] == len(oc.row_layout(ob))
        seen = np.zeros(K, dtype=int)
        for fr in _in_window(ob):
            seen += np.isfinite(np.asarray(fr['zs']).reshape(-1, 2)).all(axis=1)
        assert K == 0 or seen.min() >= 2                                                  # H_f keeps full column rank
        c = np.linalg.cond(Hf)
        print('object-case %s object %d: %d x %d, cond(H_f) %.2e' % (cid, i, Hf.shape[0], Hf.shape[1], c))
        assert c <= oc.COND_CAP, (i, c)


def test_signs_of_the_bbox_plane_offset():
    """Which signs of yyo[3] (the branch `ub[3] > 0` of the new bbox residual) the cases reach.  With the camera in front of the object
    and the box around its projection, the four lines of bbox2poly's winding all have the object's centre on the same side: one
    sign.  The other branch is not forced by a contorted case (tests/object_cases.py, docs/LAB_NOTES.md)."""
    signs = set()
    for cid in oc.CASES:
        for ob in oc.make_case(cid).objs:
            signs |= oc.bbox_plane_signs(ob)
    print('object-cases: signs of yyo[3] among the bbox rows:', sorted(signs))
    assert signs and signs <= {-1, 1}
    assert signs == SIGNS_REACHED


SIGNS_REACHED = {1}


def measure(cid):
    """(row errors per block class, projection errors per block class) of the float64 restatement against the extended reference, worst
    over the objects of the case."""
    case = oc.make_case(cid)
    rows, gram = {}, {}
    for ob, ref in zip(case.objs, oc.reference(cid)):
        hx6, Hf, r, rc = ref['mirror']
        ex6, eHf, er, erc = ref['rows']
        assert np.array_equal(rc, erc)
        gb, gz = oc.row_blocks(ob, hx6, Hf, r)
        rb, rz = oc.row_blocks(ob, ex6, eHf, er)
        assert not gz.any() and not rz.any()
        for q in gb:
            rows[q] = max(rows.get(q, 0.0), oc.block_err(gb[q], rb[q]))
        G = oc.gram_float64(case.win, hx6, Hf, r, rc)
        gb, gz = oc.gram_blocks(case.win, ob, G)
        rb, rz = oc.gram_blocks(case.win, ob, ref['G'])
        assert not rz.any() and not gz.any()
        for q in gb:
            k = oc.gram_class(q)
            gram[k] = max(gram.get(k, 0.0), oc.block_err(gb[q], rb[q]))
    return rows, gram


@pytest.mark.parametrize('cid', oc.CASES, ids=oc.IDS)
def test_float64_restatement_agrees_with_the_extended_reference(cid):
    rows, gram = measure(cid)
    side = 'left' if oc.make_case(cid).obj_left else 'right'
    print('object-case %s rows %s gram(%s) %s' % (cid, {q: '%.2e' % v for q, v in rows.items()}, side, {q: '%.2e' % v for q, v in gram.items()}))
    for q, v in rows.items():
        assert v <= SLACK * oc.ROW_WORST[q], (q, v)
    for q, v in gram.items():
        assert v <= SLACK * oc.GRAM_WORST[side][q], (q, v)
    assert all(oc.ROW_TOL[q] == 100 * oc.ROW_WORST[q] for q in oc.ROW_WORST)
    assert all(oc.GRAM_TOL[s][q] == 100 * oc.GRAM_WORST[s][q] for s in oc.GRAM_WORST for q in oc.GRAM_WORST[s])


def test_recorded_worst_errors_are_the_measured_ones():
    """The constants of the case file are what the restatement shows, not a ceiling far above it: the worst over all cases is within
    SLACK below each of them as well."""
    rows, gram = {}, dict(left={}, right={})
    for cid in oc.CASES:
        r, g = measure(cid)
        side = 'left' if oc.make_case(cid).obj_left else 'right'
        for q, v in r.items():
            rows[q] = max(rows.get(q, 0.0), v)
        for q, v in g.items():
            gram[side][q] = max(gram[side].get(q, 0.0), v)
    print('object-cases worst: rows %s gram %s' % ({q: '%.2e' % v for q, v in rows.items()}, {s: {q: '%.2e' % v for q, v in d.items()} for s, d in gram.items()}))
    for q, v in rows.items():
        assert oc.ROW_WORST[q] / SLACK <= v <= SLACK * oc.ROW_WORST[q], (q, v)
    for s in gram:
        for q, v in gram[s].items():
            assert oc.GRAM_WORST[s][q] / SLACK <= v <= SLACK * oc.GRAM_WORST[s][q], (s, q, v)


def _worst_excess(win, ob, got_rows, ref_rows, G_got, G_ref, side):
    """max over the blocks of error / tolerance, rows and projection."""
    worst = {}
    gb, _ = oc.row_blocks(ob, *got_rows)
    rb, _ = oc.row_blocks(ob, *ref_rows)
    for q in gb:
        worst[q] = oc.block_err(gb[q], rb[q]) / oc.ROW_TOL[q]
    gb, _ = oc.gram_blocks(win, ob, G_got)
    rb, _ = oc.gram_blocks(win, ob, G_ref)
    for q in gb:
        k = oc.gram_class(q)
        worst['G_' + k] = max(worst.get('G_' + k, 0.0), oc.block_err(gb[q], rb[q]) / oc.GRAM_TOL[side][k])
    return worst


def test_reference_notices_what_it_is_there_to_notice():
    """The three one-line faults of the mutation check, applied to the restatement's float64 blocks: each moves its block by more than
    1e3 x the tolerance (the reference is not blind to them)."""
    # (1) the keypoint block of keypoint K - 1 written 3 columns low
    cid = oc.CaseId(17, 'L', frames=12)
    case, ref = oc.make_case(cid), oc.reference(cid)[0]
    ob = case.objs[0]
    hx6, Hf, r, rc = ref['mirror']
    K = len(ob.kps)
    bad = Hf.copy()
    rows = [q for q, lay in enumerate(oc.row_layout(ob)) if lay[2] == K - 1]
    bad[rows, 9 + 3 * (K - 1): 12 + 3 * (K - 1)] = 0.0
    bad[rows, 9 + 3 * (K - 2): 12 + 3 * (K - 2)] = Hf[rows, 9 + 3 * (K - 1): 12 + 3 * (K - 1)]
    w = _worst_excess(case.win, ob, (hx6, bad, r), ref['rows'][:3], oc.gram_float64(case.win, hx6, bad, r, rc), ref['G'], 'left')
    assert w['Hf_kp'] > 1e3 and w['G_tile'] > 1e3, w
    assert oc.row_blocks(ob, hx6, bad, r)[1].any()                       # and the zero pattern is broken
    # (2) rank of the lanes above a missing keypoint off by one: in a frame that misses keypoint 0 the row pairs of keypoints 1 and 2
    #     change places (every array alike: a row permutation, which the projection cannot see -- the row blocks must)
    cid = oc.CaseId(4, 'L', frames=12, pat='first')
    case, ref = oc.make_case(cid), oc.reference(cid)[0]
    ob = case.objs[0]
    hx6, Hf, r, rc = ref['mirror']
    lay = oc.row_layout(ob)
    f = next(f for f, fr in enumerate(ob.frames) if np.isnan(fr['zs'][0]).all())
    a, b = (next(q for q, l in enumerate(lay) if l[0] == f and l[2] == k) for k in (1, 2))
    perm = np.arange(len(lay))
    perm[[a, a + 1, b, b + 1]] = [b, b + 1, a, a + 1]
    w = _worst_excess(case.win, ob, (hx6[perm], Hf[perm], r[perm]), ref['rows'][:3], ref['G'], ref['G'], 'left')
    assert w['res_kp'] > 1e3 and w['Hf_kp'] > 1e3 and w['Hx6_rot'] > 1e3, w
    # (3) the second frame of a wavefront (lpf = 32) using the first frame's observation mask: its keypoints are ranked by the
    #     other frame's detections
    cid = oc.CaseId(13, 'L', frames=12, pat='first')
    case, ref = oc.make_case(cid), oc.reference(cid)[0]
    ob = case.objs[0]
    hx6, Hf, r, rc = ref['mirror']
    lay = oc.row_layout(ob)
    assert not np.isnan(ob.frames[0]['zs']).any() and np.isnan(ob.frames[1]['zs'][0]).all()     # frames 0 and 1 share a wavefront
    m0 = [k for k in range(13) if np.isfinite(ob.frames[0]['zs'][k]).all()]
    first = next(q for q, l in enumerate(lay) if l[0] == 1)
    bx6, bHf, br = hx6.copy(), Hf.copy(), r.copy()
    for q, l in enumerate(lay):
        if l[0] == 1 and l[2] >= 0:                                      # keypoint rows of frame 1, placed by frame 0's mask
            to = first + 2 * sum(1 for k in m0 if k < l[2]) + (q - first) % 2
            bx6[to], bHf[to], br[to] = hx6[q], Hf[q], r[q]
    w = _worst_excess(case.win, ob, (bx6, bHf, br), ref['rows'][:3], oc.gram_float64(case.win, bx6, bHf, br, rc), ref['G'], 'left')
    assert w['res_kp'] > 1e3 and w['Hf_kp'] > 1e3 and w['G_tile'] > 1e3, w
