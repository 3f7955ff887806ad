"""GPU: the object rows (k_object_rows) and the per-object projection (k_obj_fused; k_object_rows_batch -> k_obj_front -> border / solve /
refine) BLOCK BY BLOCK against the extended-precision reference of tests/object_cases.py, at the keypoint counts, frame patterns and
flag sets where the kernels take another branch.  The bounds are 100 x the error of the float64 restatement measured on the CPU
(tests/test_object_cases.py); none of them comes from what the device returns.  Diagnostics build: the compressed block is read with
capi.debug_read(upd, 'Ab'), the route with capi.debug_read(upd, 'obj_fused')."""
import os

import numpy as np
import pytest

from orcvio_amd import capi
from helpers import rel, objects_update_reference
import object_cases as oc

pytestmark = pytest.mark.gpu
TOL = 1e-6   # the bars of tests/test_gpu_objects.py for the whole update


class Pipeline:
    """One handle of the diagnostics build with ORCVIO_OBJ_FUSED fixed when it was created, and the single-object projections taken on
    it so far (each is computed once and shared by the tests)."""

    def __init__(self, fused_opt):
        old = os.environ.get('ORCVIO_OBJ_FUSED')
        os.environ['ORCVIO_OBJ_FUSED'] = str(fused_opt)   # (a switch of the diagnostics build, read when the handle is created)
        try:
            self.upd = capi.MsckfUpdater(device=0, max_clones=36, max_features=64, max_observations=1024, debug_hooks=True)
        finally:
            if old is None:
                del os.environ['ORCVIO_OBJ_FUSED']
            else:
                os.environ['ORCVIO_OBJ_FUSED'] = old
        self.fused_opt = fused_opt
        self.done = {}

    def project(self, case, objs):
        """(G [(NA + 1)^2], route, dof) of one orcvio_msckf_objects_local_tracks call on `objs`."""
        win = case.win
        dof = self.upd.objects_local_tracks(win.flags, win.N, objs, win.P, win.R_b2c[0], win.t_c_b[0], *case.flags3, fix_D=case.fix_D)
        Ab = capi.debug_read(self.upd, 'Ab')
        NA = win.flags.leg_dim + 6 * win.N - 15
        assert capi.debug_read(self.upd, 'dims')['NA'] == NA and Ab.shape[0] >= NA + 1
        return Ab[:NA + 1, :NA + 1].copy(), capi.debug_read(self.upd, 'obj_fused'), dof

    def single(self, cid, i):
        if (cid, i) not in self.done:
            case = oc.make_case(cid)
            self.done[(cid, i)] = self.project(case, [case.objs[i]])
        return self.done[(cid, i)]


@pytest.fixture(scope='module')
def pipes(built):
    p = dict(fused=Pipeline(1), three=Pipeline(0))
    yield p
    for q in p.values():
        q.upd.close()


@pytest.fixture(scope='module')
def product(built):
    u = capi.MsckfUpdater(device=0, max_clones=32, max_features=64, max_observations=1024)
    yield u
    u.close()


def _alone(case, i):
    """The case with object i alone: is it one for k_obj_fused?"""
    return oc.Case(case.cid, case.win, [case.objs[i]], case.obj_left, case.new_bbox, case.vio_left, case.fix_D).fused


@pytest.mark.parametrize('cid', oc.CASES, ids=oc.IDS)
def test_rows_block_by_block(pipes, cid):
    """k_object_rows: every block of every object within ROW_TOL of the extended reference, the structural zeros exactly zero,
    row_clone identical."""
    case = oc.make_case(cid)
    upd = pipes['three'].upd
    for i, (ob, ref) in enumerate(zip(case.objs, oc.reference(cid))):
        got = upd.object_rows_eval(ob, case.win.R_b2c[0], case.win.t_c_b[0], *case.flags3, fix_D=case.fix_D)
        ex6, eHf, er, erc = ref['rows']
        assert got is not None and got['Hf'].shape == eHf.shape and got['Hx6'].shape == ex6.shape
        assert np.array_equal(got['row_clone'], erc)
        gb, gz = oc.row_blocks(ob, got['Hx6'], got['Hf'], got['res'])
        rb, _ = oc.row_blocks(ob, ex6, eHf, er)
        errs = {q: oc.block_err(gb[q], rb[q]) for q in gb}
        print('object-blocks %s object %d rows %s' % (cid, i, {q: '%.2e' % v for q, v in errs.items()}))
        assert not gz.any(), 'a structural zero of H_f is not zero'
        for q, v in errs.items():
            assert v <= oc.ROW_TOL[q], (i, q, v)


def _check_gram(case, ob, G, ref_G, tag):
    side = 'left' if case.obj_left else 'right'
    gb, gz = oc.gram_blocks(case.win, ob, G)
    rb, _ = oc.gram_blocks(case.win, ob, ref_G)
    errs = {}
    for q in gb:
        k = oc.gram_class(q)
        errs[k] = max(errs.get(k, 0.0), oc.block_err(gb[q], rb[q]))
    asym = float(np.abs(G - G.T).max())
    print('object-blocks %s gram(%s) %s asym %.2e' % (tag, side, {q: '%.2e' % v for q, v in errs.items()}, asym))
    assert not gz.any(), 'an entry outside the clones that see the object is not zero'
    assert np.array_equal(G, G.T), asym                         # symmetric to the bit
    for k, v in errs.items():
        assert v <= oc.GRAM_TOL[side][k], (tag, k, v)


@pytest.mark.parametrize('cid', oc.CASES, ids=oc.IDS)
def test_projection_block_by_block_on_both_pipelines(pipes, cid):
    """orcvio_msckf_objects_local_tracks with ONE object: the compressed block is G_o.  With ORCVIO_OBJ_FUSED=1 the objects the
    library sends to k_obj_fused must have run it (and the others not), with ORCVIO_OBJ_FUSED=0 nothing does; every block within
    GRAM_TOL of the extended reference on both, and the two pipelines within GRAM_TOL of each other."""
    case = oc.make_case(cid)
    side = 'left' if case.obj_left else 'right'
    for i, (ob, ref) in enumerate(zip(case.objs, oc.reference(cid))):
        rows, ncol = ref['rows'][1].shape
        got = {}
        for name, want_route in (('fused', int(_alone(case, i))), ('three', 0)):
            G, route, dof = pipes[name].single(cid, i)
            assert route == want_route, (name, i, route)
            assert dof == rows - ncol
            _check_gram(case, ob, G, ref['G'], '%s object %d %s' % (cid, i, name))
            got[name] = G
        if _alone(case, i):
            a, _ = oc.gram_blocks(case.win, ob, got['fused'])
            b, _ = oc.gram_blocks(case.win, ob, got['three'])
            for q in a:
                assert oc.block_err(a[q], b[q]) <= oc.GRAM_TOL[side][oc.gram_class(q)], (i, q)


def test_eligibility_boundary_routes(pipes):
    """32 in-window frames run k_obj_fused, 33 and an object with two frames on one clone the three-launch pipeline (the results are
    checked by the test above; this is the route alone, by name)."""
    by_pat = {c.pat: c for c in oc.CASES if c.win == 'maxf'}
    assert pipes['fused'].single(by_pat['f32'], 0)[1] == 1
    assert pipes['fused'].single(by_pat['f33'], 0)[1] == 0
    assert pipes['fused'].single(by_pat['shared'], 0)[1] == 0
    assert all(pipes['three'].single(by_pat[p], 0)[1] == 0 for p in ('f32', 'f33', 'shared'))


@pytest.mark.parametrize('cid,name', [(oc.MULTI5, 'fused'), (oc.MULTI5, 'three'), (oc.MULTI6, 'three'), (oc.MULTI6, 'fused')],
                         ids=['five_fused', 'five_three_launch', 'six_three_launch', 'six_refused_by_fused'])
def test_several_objects_sum_to_their_single_blocks(pipes, cid, name):
    """The block of one call with all objects of `multi` equals the sum of the single-object blocks of the same pipeline, tile by
    tile within GRAM_TOL of the summed tile (per-object offsets: row0, Y at o NOP, Sg at o N 64, the Kmax-sized LDS tables).  Six
    objects, one of 17 keypoints: the whole update leaves k_obj_fused."""
    case = oc.make_case(cid)
    p = pipes[name]
    G, route, dof = p.project(case, case.objs)
    assert route == int(name == 'fused' and case.fused)
    singles = [p.single(cid, i) for i in range(len(case.objs))]
    # (the singles of the ORCVIO_OBJ_FUSED=1 handle took k_obj_fused where they could, whatever the joint call took: the sum is the sum)
    assert dof == sum(s[2] for s in singles)
    S = np.sum([s[0].astype(oc.LD) for s in singles], axis=0)
    win = case.win
    NA = win.flags.leg_dim + 6 * win.N - 15
    cb0 = win.flags.leg_dim - 15
    spans = [slice(cb0 + 6 * c, cb0 + 6 * c + 6) for c in range(win.N)] + [slice(NA, NA + 1)]
    tol = oc.GRAM_TOL['left']
    assert case.obj_left == 1
    worst = 0.0
    covered = np.zeros(G.shape, dtype=bool)
    for a, sa in enumerate(spans):
        for b, sb in enumerate(spans):
            covered[sa, sb] = True
            ref = S[sa, sb]
            if not np.abs(ref).max() > 0:
                assert not G[sa, sb].any(), (a, b)
                continue
            k = 'rr' if a == b == win.N else ('r' if win.N in (a, b) else 'tile')
            e = oc.block_err(G[sa, sb], ref)
            worst = max(worst, e / tol[k])
            assert e <= tol[k], (a, b, k, e)
    assert not G[~covered].any()
    assert np.array_equal(G, G.T)
    print('object-blocks %s %s: worst error / tolerance over the tiles %.2e' % (cid, name, worst))


@pytest.mark.parametrize('K', [1, 13, 17, 34])
def test_whole_update_at_the_new_keypoint_counts(product, K):
    """update_object_tracks (product library) at K = 1, 13 (k_obj_fused, lpf 8 and 32) and 17, 34 (three-launch, NOP = 64 and 112,
    no_max = 60 and 111) against helpers.objects_update_reference: the bars of tests/test_gpu_objects.py."""
    case = oc.make_case(oc.CaseId(K, 'L', frames=12))
    win = case.win
    ref = objects_update_reference(win, case.objs, win.P, *case.flags3, full_nullspace=True)
    assert ref['rank_deficient'] == 0 and ref['accept'] == 1
    got = product.update_object_tracks(win.flags, win.N, case.objs, win.P, win.R_b2c[0], win.t_c_b[0], *case.flags3)
    assert product.counters()['obj_fused'] == int(case.fused)
    print('object-blocks whole update K=%d: gamma %.3e, dx %.2e, P_new %.2e' % (K, abs(got['gamma'] - ref['gamma']) / abs(ref['gamma']),
                                                                                 rel(got['dx'], ref['dx']), rel(got['P_new'], ref['P_new'])))
    assert got['accept'] == ref['accept'] and got['stats'][0] == ref['dof']
    assert abs(got['gamma'] - ref['gamma']) < 1e-6 * abs(ref['gamma'])
    assert rel(got['dx'], ref['dx']) < TOL and rel(got['P_new'], ref['P_new']) < TOL
