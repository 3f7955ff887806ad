"""orcvio_msckf_object_lm (k_object_lm: the batched Levenberg-Marquardt of the object tracks, one workgroup per object) against
the numpy mirror (tests/mirror_object_lm.py: same iteration, dense solve, regularisers as explicit rows), from the same start
with the same configuration.

Tolerance of an optimum: ten times the mirror's OWN spread for that case (two starts x left / right perturbation, measured by
tests/test_object_lm_mirror.py: 4e-10 .. 3e-9 on the one_car cases), never looser than 1e-6.  The factor ten covers the device's
summation order (lanes, wavefronts, roles) and its Schur elimination.  The final cost is compared relatively with the same number:
the cost is stationary at the optimum, so a state difference enters it in second order only.  Iteration counts are printed, not
asserted: the convergence test compares the predicted decrease with 1e-18 c, which is decided by rounding."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from helpers import rel, objects_update_reference
import mirror_object_lm as mlm
import object_lm_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=48, max_features=64, max_observations=1024)
    yield u
    u.close()


def _device(upd, obj, ms, mk, left, new_bbox, weights, **kw):
    tracks, stats = upd.object_lm([obj], [ms], [mk], left, new_bbox, weights, **kw)
    return dict(wTo=tracks[0].wTo, shape=tracks[0].shape, kps=tracks[0].kps, **stats[0])


def _tolerance(spread):
    return min(1e-6, 10.0 * spread)


def _check(tag, dev, mir, tol):
    d = oc.distance(dev, mir)
    dc = abs(dev['cost'] - mir['cost']) / mir['cost']
    print('%s: |device - mirror| %.2e (tol %.2e), cost rel %.2e, cost0 rel %.2e, iterations %d / %d, evaluations %d / %d, status %d / %d'
          % (tag, d, tol, dc, abs(dev['cost0'] - mir['cost0']) / mir['cost0'], dev['iterations'], mir['iterations'],
             dev['evaluations'], mir['evaluations'], dev['status'], mir['status']))
    assert dev['status'] == 1 and mir['status'] == 1
    assert abs(dev['cost0'] - mir['cost0']) <= 1e-11 * mir['cost0']   # (the same start: summation order only)
    assert d <= tol
    assert dc <= tol


@pytest.mark.parametrize('left', [True, False], ids=['left', 'right'])
@pytest.mark.parametrize('name', list(oc.CASES))
def test_one_car_cases_against_the_mirror(upd, name, left):
    """F = 47 (both weight sets), 33, 1 and 2 with NaN detections -- one keypoint detected nowhere -- on the reference's track."""
    c = oc.CASES[name]
    spread, _ = oc.case_spread(name)
    obj, ms, mk = oc.one_car(c['n_frames'], c['nan_case'], c['starts'][0])
    mir = oc.mirror_one_car(c['n_frames'], c['nan_case'], c['starts'][0], left, c['new_bbox'], c['weights'])
    dev = _device(upd, obj, ms, mk, left, c['new_bbox'], c['weights'])
    _check('%s %s' % (name, 'left' if left else 'right'), dev, mir, _tolerance(spread))
    if c['nan_case']:
        assert np.abs(dev['kps'][3] - mk[3]).max() <= 1e-12   # detected nowhere: stays at its mean


@pytest.mark.parametrize('weights', [oc.WEIGHTS_REF, oc.WEIGHTS_UNIT], ids=['refw', 'unitw'])
@pytest.mark.parametrize('new_bbox', [0, 2])
@pytest.mark.parametrize('left', [True, False], ids=['left', 'right'])
@pytest.mark.parametrize('n_frames,nan_case', [(1, 0), (2, 1), (2, 2)], ids=['f1', 'f2nan', 'f2blind'])
def test_flag_grid_on_the_small_shapes(upd, n_frames, nan_case, left, new_bbox, weights):
    """F = 1, K = 12; F = 2 with five NaNs; F = 2 with a keypoint detected nowhere and a frame without any detection: left / right
    x bbox form 0 / 2 x the two weight sets (the near starts: the new bbox form at unit weights has further minima within reach
    of the far ones, object_lm_cases.START_XI).  The mirror's spread is taken over FOUR starts x two charts here: one or two
    frames leave a direction of the optimum that the convergence test (pred <= 1e-18 c) resolves to 1e-8 only, and the largest
    difference among four runs under-estimates that -- on F = 1, bbox form 2, the reference's weights it is 2.9e-10 over starts
    2 / 3, 3.3e-9 over these four, 1.2e-8 over the far starts 0 / 1 (same optimum).  F = 1 and F = 2 with five NaNs run at the
    default max_iter = 60, which is what callers get; the blind-frame shape at max_iter = 200 on both sides: with bbox form 2 and
    unit weights the mirror needs up to 70 iterations there."""
    max_iter = 200 if nan_case == 2 else 60
    spread, _ = oc.mirror_spread(n_frames, nan_case, new_bbox, weights, oc.NEAR_STARTS, max_iter)
    obj, ms, mk = oc.one_car(n_frames, nan_case, 2)
    mir = oc.mirror_one_car(n_frames, nan_case, 2, left, new_bbox, weights, max_iter)
    dev = _device(upd, obj, ms, mk, left, new_bbox, weights, max_iter=None if max_iter == 60 else max_iter)
    _check('F %d left %d bbox %d w1 %g' % (n_frames, left, new_bbox, weights[1]), dev, mir, _tolerance(spread))


@pytest.mark.parametrize('K,F,weights', [(1, 5, oc.WEIGHTS_UNIT), (16, 4, oc.WEIGHTS_UNIT), (12, 65, oc.WEIGHTS_REF), (5, 128, oc.WEIGHTS_REF)],
                         ids=['K1', 'K16', 'F65', 'F128'])
def test_synthetic_shapes_against_the_mirror(upd, K, F, weights):
    """The shapes the fixture does not have: one keypoint (8 lanes per frame), sixteen (32 lanes per frame), F = 65 (one frame past
    four passes of a workgroup at 16 lanes per frame) and F = 128 (the cap).  Tolerance as everywhere: ten times the mirror's own
    spread over two projected starts x two charts on that track.  The two long tracks run at the reference's weights, where the
    mirror needs 6-22 iterations instead of 16-35 at unit weights: its time is what this test costs."""
    spread, runs = oc.synthetic_spread(K, F, 1, weights)
    print('K %d F %d: mirror spread %.2e, tolerance %.2e, mirror iterations %s' % (K, F, spread, _tolerance(spread), [r['iterations'] for r in runs]))
    obj, ms, mk = oc.synthetic(K, F, 1, start_scale=0.3, start=0)
    for left, mir in ((True, runs[0]), (False, runs[1])):
        dev = _device(upd, obj, ms, mk, left, 0, weights)
        _check('K %d F %d left %d' % (K, F, left), dev, mir, _tolerance(spread))


def test_batch_of_twenty_equals_one_object_per_call_bit_for_bit(upd):
    """Twenty objects of different K and F in one launch against the same objects one per call: a workgroup's arithmetic does not
    depend on what else the launch holds."""
    shapes = [(1, 1), (1, 9), (2, 3), (3, 17), (4, 2), (4, 33), (5, 5), (6, 12), (7, 1), (8, 64), (9, 4), (10, 31), (11, 7), (12, 30),
              (12, 65), (13, 2), (14, 16), (15, 3), (16, 8), (16, 128)]
    cases = [oc.synthetic(K, F, seed=3 + i) for i, (K, F) in enumerate(shapes)]
    objs, ms, mk = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    tb, sb = upd.object_lm(objs, ms, mk, True, 0, oc.WEIGHTS_UNIT)
    print('batch: status %s, iterations %s' % ([s['status'] for s in sb], [s['iterations'] for s in sb]))
    for i in range(len(objs)):
        t1, s1 = upd.object_lm([objs[i]], [ms[i]], [mk[i]], True, 0, oc.WEIGHTS_UNIT)
        assert s1[0] == sb[i]
        assert np.array_equal(t1[0].wTo, tb[i].wTo) and np.array_equal(t1[0].shape, tb[i].shape) and np.array_equal(t1[0].kps, tb[i].kps)
        assert np.isfinite(tb[i].wTo).all() and sb[i]['cost'] <= sb[i]['cost0']


@pytest.mark.parametrize('name', ['f47', 'f2_nan'])
def test_gradient_at_the_device_optimum_through_object_rows_eval(upd, name):
    """The device optimum handed to orcvio_msckf_object_rows_eval (the call that serves the reference's fvec_all / fjac_*): the
    weighted H_f^T r plus the regularisers' gradient -- added here -- is at the level of the mirror's own at its optimum."""
    c = oc.CASES[name]
    obj, ms, mk = oc.one_car(c['n_frames'], c['nan_case'], c['starts'][0])
    w = c['weights']
    tracks, stats = upd.object_lm([obj], [ms], [mk], True, c['new_bbox'], w)
    assert stats[0]['status'] == 1
    opt = dataclasses.replace(tracks[0], frames=[dict(fr, clone=i) for i, fr in enumerate(obj.frames)])
    rows = upd.object_rows_eval(opt, np.eye(3), np.zeros(3), True, c['new_bbox'], 0, fix_D=True)
    is_bbox = ~rows['Hf'][:, 9:].any(axis=1)
    wt = np.where(is_bbox, w[1], w[0])
    g = rows['Hf'].T @ (wt * wt * rows['res'])
    F = len(obj.frames)
    g[6:9] += w[3] ** 2 * F * (opt.shape - ms)
    g[9:] += w[2] ** 2 * F * (opt.kps - mk).reshape(-1)
    mir = oc.mirror_one_car(c['n_frames'], c['nan_case'], c['starts'][0], True, c['new_bbox'], w)
    cfg = mlm.Config(left=True, new_bbox=c['new_bbox'], weights=w)
    g_mir = mlm.gradient_norm(mir['wTo'], mir['shape'], mir['kps'], obj.frames, ms, mk, cfg)
    g_dev = float(np.linalg.norm(g))
    print('%s: |H_f^T r| device %.2e, mirror %.2e' % (name, g_dev, g_mir))
    assert g_dev <= 10.0 * g_mir


def test_literal_new_bbox_jacobians_terminate(upd):
    """use_new_bbox_residual = 1: the reference's literal Jacobians do not match its residual (SURVEY note N8) and nobody has run
    the iteration with them.  What can be asked: it ends (status 1 or 2, given room), the output is finite, the cost did not rise."""
    for n_frames, nan_case in [(2, 1), (47, 0)]:
        obj, ms, mk = oc.one_car(n_frames, nan_case, 2)
        for left in (True, False):
            dev = _device(upd, obj, ms, mk, left, 1, oc.WEIGHTS_REF, max_iter=2000)
            print('new_bbox 1, F %d, left %d: status %d after %d iterations, cost %.6g -> %.6g'
                  % (n_frames, left, dev['status'], dev['iterations'], dev['cost0'], dev['cost']))
            assert dev['status'] in (1, 2)
            assert np.isfinite(dev['wTo']).all() and np.isfinite(dev['shape']).all() and np.isfinite(dev['kps']).all()
            assert np.isfinite(dev['cost']) and dev['cost'] <= dev['cost0']


def test_one_iteration_is_the_mirrors_first_step(upd):
    """max_iter = 1: status 3 and the state after one step.  One damped solve: the two differ by rounding amplified by the
    system's condition (<= 3e7 here, times 2.2e-16, times a step of order one): 1e-8."""
    for name in ('f47', 'f2_nan'):
        c = oc.CASES[name]
        obj, ms, mk = oc.one_car(c['n_frames'], c['nan_case'], c['starts'][0])
        for left in (True, False):
            mir = mlm.solve(obj, ms, mk, mlm.Config(left=left, new_bbox=c['new_bbox'], weights=c['weights'], max_iter=1))
            dev = _device(upd, obj, ms, mk, left, c['new_bbox'], c['weights'], max_iter=1)
            d = oc.distance(dev, mir)
            print('%s left %d: one step, |device - mirror| %.2e, cost %.9g / %.9g' % (name, left, d, dev['cost'], mir['cost']))
            assert dev['status'] == 3 and mir['status'] == 3 and dev['iterations'] == 1 and dev['evaluations'] == 2
            assert oc.distance(mir, dict(wTo=obj.wTo, shape=obj.shape, kps=obj.kps)) > 1e-3   # (a step was taken)
            assert d <= 1e-8
            assert abs(dev['cost'] - mir['cost']) <= 1e-8 * mir['cost']


def _raw_call(upd, obj, ms, mk, mutate):
    """The C call on one object with the caller's records changed by `mutate` before it; returns (code, result arrays)."""
    lib = upd.lib
    cfg = capi.ObjectLMConfig()
    lib.orcvio_msckf_object_lm_config_default.argtypes = [C.POINTER(capi.ObjectLMConfig)]
    lib.orcvio_msckf_object_lm_config_default.restype = None
    lib.orcvio_msckf_object_lm_config_default(C.byref(cfg))
    _, arr, keep = upd._object_tracks([obj], np.eye(3), np.zeros(3), True, 0, 0, False)
    msc, mkc = np.ascontiguousarray(ms, dtype=np.float64), np.ascontiguousarray(mk, dtype=np.float64)
    pri = (capi.ObjectLMPrior * 1)(capi.ObjectLMPrior(capi._d(msc), capi._d(mkc)))
    out = [np.zeros(16), np.zeros(3), np.zeros(48)]
    res = (capi.ObjectLMResult * 1)()
    res[0].wTo, res[0].shape, res[0].kps = capi._d(out[0]), capi._d(out[1]), capi._d(out[2])
    state = dict(tracks=arr, priors=pri, results=res, n=1, cfg=C.byref(cfg), cfg_rec=cfg)
    mutate(state)
    lib.orcvio_msckf_object_lm.argtypes = [C.c_void_p, C.POINTER(capi.ObjectLMConfig), C.POINTER(capi.ObjectTrackC),
                                           C.POINTER(capi.ObjectLMPrior), C.c_int32, C.POINTER(capi.ObjectLMResult)]
    lib.orcvio_msckf_object_lm.restype = C.c_int32
    rc = lib.orcvio_msckf_object_lm(upd.h, state['cfg'], state['tracks'], state['priors'], state['n'], state['results'])
    return rc, out


def test_refusals_come_before_anything_runs(upd):
    """K = 0, K = 17, F = 0, F = 129, a NaN in wTo, null pointers, a bad configuration: refused with ORCVIO_ERR_INVALID (1) /
    ORCVIO_ERR_CAPACITY (3), the result arrays untouched; the handle serves the next call."""
    obj, ms, mk = oc.one_car(2, 1, 0)
    INVALID, CAPACITY = 1, 3

    def setter(**kw):
        def f(st):
            for k, v in kw.items():
                setattr(st['tracks'][0], k, v)
        return f

    def key(k, v):
        def f(st):
            st[k] = v
        return f

    def nan_pose(st):
        bad = np.ascontiguousarray(obj.wTo, dtype=np.float64).copy()
        bad[1, 2] = np.nan
        st['keep'] = bad
        st['tracks'][0].wTo = capi._d(bad)

    def null_result(st):
        st['results'][0].kps = None

    def null_prior(st):
        st['priors'][0].mean_kps = None

    def bad_cfg(st):
        st['cfg_rec'].max_iter = 0

    def nan_weight(st):
        st['cfg_rec'].residual_weights[1] = float('nan')

    cases = [('K = 0', setter(n_keypoints=0), INVALID), ('K = 17', setter(n_keypoints=17), CAPACITY),
             ('F = 0', setter(n_frames=0), INVALID), ('F = 129', setter(n_frames=129), CAPACITY),
             ('NaN in wTo', nan_pose, INVALID), ('null wTo', setter(wTo=None), INVALID), ('null frame_zs', setter(frame_zs=None), INVALID),
             ('null result array', null_result, INVALID), ('null prior', null_prior, INVALID), ('null config', key('cfg', None), INVALID),
             ('null tracks', key('tracks', None), INVALID), ('negative count', key('n', -1), INVALID),
             ('more tracks than the handle holds', key('n', 65), CAPACITY), ('max_iter = 0', bad_cfg, INVALID), ('NaN weight', nan_weight, INVALID)]
    for tag, mutate, want in cases:
        rc, out = _raw_call(upd, obj, ms, mk, mutate)
        assert rc == want, (tag, rc)
        assert not any(o.any() for o in out), tag
    rc, out = _raw_call(upd, obj, ms, mk, lambda st: None)
    assert rc == 0 and out[0].any()
    rc, _ = _raw_call(upd, obj, ms, mk, key('n', 0))   # no tracks: nothing to do
    assert rc == 0


def test_lm_then_object_update_end_to_end(upd):
    """The intended sequence: the optimiser's result goes into orcvio_msckf_update_object_tracks as it is.  Device LM + device
    update against mirror LM + the mirror's literal update (test_gpu_fixtures' one_car update: 30 of the 47 frames in the window)."""
    N = 30
    c = oc.CASES['f47']
    obj, ms, mk = oc.one_car(47, 0, c['starts'][0])
    obj = dataclasses.replace(obj, frames=[dict(fr, clone=i if i < N else -1) for i, fr in enumerate(obj.frames)])
    flags = synth.Flags(use_larvio=0, use_left_perturbation=0, noise_feature=0.05)
    win = synth.make_window(N=N, F=2, seed=2, flags=flags, track_len=3)
    mir = oc.mirror_one_car(47, 0, c['starts'][0], True, 0, c['weights'])
    ref = objects_update_reference(win, [dataclasses.replace(obj, wTo=mir['wTo'], shape=mir['shape'], kps=mir['kps'])], win.P, True, False, 0)
    tracks, stats = upd.object_lm([obj], [ms], [mk], True, 0, c['weights'])
    assert stats[0]['status'] == 1
    got = upd.update_object_tracks(flags, win.N, tracks, win.P, win.R_b2c[0], win.t_c_b[0], True, False, 0)
    print('end to end: accept %d / %d, gamma %.9g / %.9g' % (got['accept'], ref['accept'], got['gamma'], ref['gamma']))
    assert ref['accept'] == 1   # (the gate takes this object: the comparison of dx and P+ below is not optional)
    assert got['accept'] == ref['accept']
    assert abs(got['gamma'] - ref['gamma']) < 1e-6 * abs(ref['gamma'])
    assert got['stats'][0] == ref['dof']
    assert rel(got['dx'], ref['dx']) < 1e-6 and rel(got['P_new'], ref['P_new']) < 1e-6
