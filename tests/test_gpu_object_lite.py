"""The lite (bbox-only) object mapper on the device -- orcvio_msckf_object_init_lite (k_object_init_lite), orcvio_msckf_object_lm_lite
(k_object_lm_lite: one wavefront per object) and orcvio_msckf_object_init_lm_lite -- against the numpy mirror
(tests/mirror_object_lite.py: bbox rows from oracle.mirror_objects, the regulariser as explicit rows, a dense solve, the start matrix
by matrix), from the same start with the same configuration.

What is compared.  The bbox-only optimum is not unique in wTo (half-turns about the ellipsoid's axes), so optima are compared by the
world dual quadric Q_w = wTo diag(v^2, -1) wTo^T (relative to its largest entry), by v and by the relative cost -- never by wTo
element by element.  The cost has further local minima on some tracks: a case enters the comparison only if the mirror's own four
runs (two starts x both charts) agree within object_lite_cases.CAP = 1e-7, which every test asserts before it compares.
Tolerance: min(1e-6, ten times the mirror's own spread on that case), the rule of test_gpu_object_lm._tolerance; cost0 within 1e-11.
max_iter = 400 on both sides (the mirror needs up to 326 iterations at F = 2).  The mirror's runs on the 65- and 128-frame tracks
take it 10-40 s per case, once per session; the device calls themselves take milliseconds."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from helpers import rel, objects_update_reference
import mirror_object_lite as ml
import object_lite_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def upd(built):
    u = capi.MsckfUpdater(device=0, max_clones=48, max_features=64, max_observations=1024)
    yield u
    u.close()


def _device(upd, obj, ms, left, new_bbox, weights=lc.UNIT, reg=0, max_iter=lc.MAX_ITER):
    tracks, stats = upd.object_lm_lite([obj], [ms], left, new_bbox, weights, reg, max_iter=max_iter)
    return dict(wTo=tracks[0].wTo, shape=tracks[0].shape, **stats[0])


def _tolerance(spread):
    return min(1e-6, 10.0 * spread)


def _check(tag, dev, mir, tol, mean_shape=None):
    dq, dv = ml.distance(dev, mir, mean_shape)
    dc = abs(dev['cost'] - mir['cost']) / mir['cost']
    print('%s: Q_w %.2e, v %.2e, cost rel %.2e (tol %.2e), cost0 rel %.2e, iterations %d / %d, status %d / %d'
          % (tag, dq, dv, dc, tol, abs(dev['cost0'] - mir['cost0']) / mir['cost0'], dev['iterations'], mir['iterations'], dev['status'], mir['status']))
    assert dev['status'] == 1 and mir['status'] == 1
    assert abs(dev['cost0'] - mir['cost0']) <= 1e-11 * mir['cost0']   # (the same start: summation order only)
    assert dq <= tol and dv <= tol and dc <= tol


# one listed (F, seed) per frame count: F = 2 one regulariser repeat, 16 / 17 one wave pass and one frame past it, 65, 128 the cap
FRAME_CASES = [(0, 2, 1), (0, 16, 2), (0, 17, 2), (0, 65, 1), (0, 128, 2), (2, 2, 2), (2, 17, 2), (2, 65, 2), (2, 128, 1)]


@pytest.mark.parametrize('new_bbox,F,seed', FRAME_CASES, ids=['bbox%d-F%d-s%d' % c for c in FRAME_CASES])
def test_frame_counts_against_the_mirror(upd, new_bbox, F, seed):
    """Both charts at unit weights, the reference's F - 1 repeats."""
    spread, runs = lc.synthetic_spread(F, seed, new_bbox)
    print('bbox %d F %d seed %d: mirror spread %.2e, tolerance %.2e' % (new_bbox, F, seed, spread, _tolerance(spread)))
    assert spread <= lc.CAP
    obj, ms = lc.synthetic(F, seed)
    for left, mir in ((True, runs[0]), (False, runs[1])):
        _check('bbox %d F %d left %d' % (new_bbox, F, left), _device(upd, obj, ms, left, new_bbox), mir, _tolerance(spread))


@pytest.mark.parametrize('reg', [0, 1])
@pytest.mark.parametrize('weights', [lc.UNIT, lc.REFW], ids=['unitw', 'refw'])
@pytest.mark.parametrize('new_bbox', [0, 2])
@pytest.mark.parametrize('F', [2, 17])
def test_weights_and_regulariser_repeats_against_the_mirror(upd, F, new_bbox, weights, reg):
    """Unit weights and (3e-2, 1) x reg_every_frame 0 / 1 x bbox form 0 / 2 x both charts on the two- and the seventeen-frame track
    (seed 2: within the cap on all of these), each with the spread of its own four mirror runs."""
    spread, runs = lc.synthetic_spread(F, 2, new_bbox, weights, reg)
    assert spread <= lc.CAP
    obj, ms = lc.synthetic(F, 2)
    for left, mir in ((True, runs[0]), (False, runs[1])):
        _check('F %d bbox %d w0 %g reg %d left %d' % (F, new_bbox, weights[0], reg, left), _device(upd, obj, ms, left, new_bbox, weights, reg), mir,
               _tolerance(spread))


@pytest.mark.parametrize('F', [2, 17, 128])
def test_reg_every_frame_adds_exactly_one_block_at_the_start(upd, F):
    """cost0 with F repeats minus cost0 with F - 1 is one regulariser block w1^2 |v - mean|^2, at a start off the mean shape."""
    obj, ms = lc.synthetic(F, 2)
    obj = dataclasses.replace(obj, shape=obj.shape + np.array([0.3, -0.2, 0.25]))
    w = (0.5, 1.5)
    c = [_device(upd, obj, ms, True, 0, w, reg, max_iter=1)['cost0'] for reg in (0, 1)]
    block = w[1] ** 2 * float(np.sum((obj.shape - ms) ** 2))
    print('F %d: cost0 %.12g / %.12g, difference %.12g, one block %.12g' % (F, c[0], c[1], c[1] - c[0], block))
    assert block > 0.1 and abs((c[1] - c[0]) - block) <= 1e-12 * c[1]
    mir = ml.solve(obj, ms, ml.Config(weights=w, reg_every_frame=0, max_iter=1))
    assert abs(c[0] - mir['cost0']) <= 1e-11 * mir['cost0']


def test_one_car_against_the_mirror(upd):
    """The reference's track, 47 frames, near starts.  Its class has the mean shape (1.5, 3, 1.5): two EQUAL semi-axes, so the exchange
    of x and z with a quarter-turn about y is one more symmetry of the cost, regulariser included, and the rotation about y is all
    but free at the optimum (smallest eigenvalue of J^T J 3.9e-9 against 2.8 for the next).  The device's right chart ends at the
    exchanged labelling (v_x and v_z, 4.2e-5 apart, swapped; Q_w 3.8e-12 and the cost 3.6e-14 from the mirror's), so v is compared
    up to the permutations that leave the mean shape as it is (mirror_object_lite.distance); Q_w and the cost as everywhere."""
    spread, runs = lc.one_car_spread(47)
    assert spread <= lc.CAP
    obj, ms = lc.one_car(47, 2)
    assert ms[0] == ms[2] != ms[1]
    for left, mir in ((True, runs[0]), (False, runs[1])):
        dev = _device(upd, obj, ms, left, 0)
        print('one_car left %d: v device %s, mirror %s' % (left, dev['shape'], mir['shape']))
        _check('one_car left %d' % left, dev, mir, _tolerance(spread), ms)


@pytest.mark.parametrize('seed,new_bbox', [(2, 0), (1, 2)])
def test_one_frame_track(upd, seed, new_bbox):
    """F = 1: four rows, nine unknowns, no regulariser -- rank-deficient, and the residual can be driven to zero.  The mirror stalls
    (status 2) at a cost of rounding size, 1e-32 .. 1e-31 -- unless rounding makes the cost EXACTLY 0.0: then the gradient is zero,
    pred = 0 <= ptol c = 0 and the documented iteration says status 1.  The mirror does that itself on (seed 2, bbox form 2, right
    chart), tests/test_object_lite_mirror.py; which of the two a run meets is decided by the last bit.  So the status is checked by
    the iteration's own rule on both sides -- 1 if and only if the returned cost is exactly zero, else 2 -- not by equality of two
    roundings (measured: the device ends (seed 1, form 2, left) at cost 0 with status 1 after 8 iterations, the mirror at 2.9e-32
    with status 2 after 37; the other three runs are status 2 on both sides).
    Compared besides: the first step (max_iter = 1, which the mirror accepts on these tracks; one damped solve, 1e-10), and
    cost <= 1e-20 cost0."""
    obj, ms = lc.synthetic(1, seed)
    for left in (True, False):
        m1 = ml.solve(obj, ms, ml.Config(left=left, new_bbox=new_bbox, max_iter=1))
        d1 = _device(upd, obj, ms, left, new_bbox, max_iter=1)
        dq, dv = ml.distance(d1, m1)
        print('F 1 seed %d bbox %d left %d: first step Q_w %.2e, v %.2e, |wTo| %.2e, cost %.6g / %.6g' % (seed, new_bbox, left, dq, dv, np.abs(d1['wTo'] - m1['wTo']).max(), d1['cost'], m1['cost']))
        assert m1['cost'] < m1['cost0'] and m1['iterations'] == 1    # (accepted)
        assert d1['status'] == 3 and d1['iterations'] == 1 and d1['evaluations'] == 2
        assert dq <= 1e-10 and dv <= 1e-10 and np.abs(d1['wTo'] - m1['wTo']).max() <= 1e-10   # (one step from one start: wTo itself is comparable)
        assert abs(d1['cost'] - m1['cost']) <= 1e-9 * m1['cost0']
        mir = ml.solve(obj, ms, ml.Config(left=left, new_bbox=new_bbox, max_iter=lc.MAX_ITER))
        dev = _device(upd, obj, ms, left, new_bbox)
        print('   full run: status %d / %d after %d / %d iterations, cost %.3g / %.3g of %.3g' % (dev['status'], mir['status'], dev['iterations'], mir['iterations'], dev['cost'], mir['cost'], dev['cost0']))
        assert mir['status'] == (1 if mir['cost'] == 0.0 else 2) and dev['status'] == (1 if dev['cost'] == 0.0 else 2)
        assert dev['cost'] <= 1e-20 * dev['cost0'] and np.isfinite(dev['wTo']).all() and np.isfinite(dev['shape']).all()


def test_literal_new_bbox_jacobians_terminate(upd):
    """use_new_bbox_residual = 1, the reference's literal Jacobians (SURVEY note N8): it ends with a status in 1..3, the output is
    finite, the cost did not rise.  No parity claim on the optimum."""
    for F, seed in ((2, 2), (17, 2)):
        obj, ms = lc.synthetic(F, seed)
        for left in (True, False):
            dev = _device(upd, obj, ms, left, 1, max_iter=2000)
            print('new_bbox 1, F %d, left %d: status %d after %d iterations, cost %.6g -> %.6g' % (F, left, dev['status'], dev['iterations'], dev['cost0'], dev['cost']))
            assert dev['status'] in (1, 2, 3)
            assert np.isfinite(dev['wTo']).all() and np.isfinite(dev['shape']).all()
            assert np.isfinite(dev['cost']) and dev['cost'] <= dev['cost0']


def test_batch_of_five_equals_one_object_per_call_bit_for_bit(upd):
    """Five objects, one more than a workgroup holds, of 1, 2, 17, 65 and 128 frames: the wavefronts of the first workgroup finish at
    different iterations and none waits for another.  One batch call, then the same objects one per call: the same bits."""
    cases = [lc.synthetic(F, seed) for F, seed in ((1, 2), (2, 2), (17, 2), (65, 1), (128, 2))]
    objs, ms = [c[0] for c in cases], [c[1] for c in cases]
    tb, sb = upd.object_lm_lite(objs, ms, True, 0, max_iter=lc.MAX_ITER)
    print('batch: status %s, iterations %s' % ([s['status'] for s in sb], [s['iterations'] for s in sb]))
    assert len(set(s['iterations'] for s in sb)) > 1
    for i in range(len(objs)):
        t1, s1 = upd.object_lm_lite([objs[i]], [ms[i]], True, 0, max_iter=lc.MAX_ITER)
        assert s1[0] == sb[i]
        assert np.array_equal(t1[0].wTo, tb[i].wTo) and np.array_equal(t1[0].shape, tb[i].shape)
        assert np.isfinite(tb[i].wTo).all() and sb[i]['cost'] <= sb[i]['cost0']


def _start_cases():
    return [lc.one_car(47)] + [lc.synthetic(F, seed) for F, seed in ((2, 1), (17, 2), (65, 1))]


def _degenerate():
    """A box without width in front of an identity camera: exact zeros, d = 1 / sqrt(0) (test_object_lite_mirror explains)."""
    obj, ms = lc.synthetic(2, 1)
    frames = [dict(obj.frames[0], wTc=np.eye(4), bbox=np.array([0.25, -0.125, 0.25, 0.125]))] + list(obj.frames[1:])
    return dataclasses.replace(obj, frames=frames), ms


@pytest.mark.parametrize('pose_form', [0, 1, 2])
def test_start_against_the_mirror(upd, pose_form):
    """one_car's frame 0 and three synthetic tracks in one call, the shipped and a non-unit bbox_scale: 1e-12 relative."""
    cases = _start_cases()
    for scale in (None, (0.8, 0.6, 0.7)):
        got = upd.object_init_lite([c[0] for c in cases], [c[1] for c in cases], pose_form, scale)
        for (obj, ms), g in zip(cases, got):
            m = ml.init(obj.frames, ms, scale or (1.0, 1.0, 1.0), pose_form)
            e = max(float(np.abs(g['wTo'] - m['wTo']).max() / np.abs(m['wTo']).max()), abs(g['d'] - m['d']) / m['d'])
            print('form %d scale %s F %d: start rel %.2e, d %.6g' % (pose_form, scale, len(obj.frames), e, g['d']))
            assert g['status'] == m['status'] == 1 and e <= 1e-12
            assert np.array_equal(g['wTo'][:3, :3], np.eye(3)) and np.array_equal(g['wTo'][3], [0, 0, 0, 1])
            assert (g['wTo'][2, 3] == 0.0) == (pose_form != 0)


def test_start_that_is_not_finite_is_status_4(upd):
    obj, ms = _degenerate()
    m = ml.init(obj.frames, ms)
    g = upd.object_init_lite([obj], [ms])[0]
    assert m['status'] == 4 and g['status'] == 4 and not np.isfinite(g['d']) and np.array_equal(g['wTo'], np.eye(4))


def test_init_lm_lite_equals_the_two_calls_bit_for_bit(upd):
    """One call against object_init_lite followed by object_lm_lite from its pose and the mean shape; the object whose start fails
    (a box without width) comes back with LM status 0, the identity and the mean shape."""
    cases = _start_cases()[:3] + [_degenerate()] + [lc.synthetic(17, 1)]
    objs, ms = [c[0] for c in cases], [c[1] for c in cases]
    for pose_form, new_bbox in ((1, 0), (0, 2)):
        inits, tracks, stats = upd.object_init_lm_lite(objs, ms, True, new_bbox, max_iter=lc.MAX_ITER, pose_form=pose_form)
        alone = upd.object_init_lite(objs, ms, pose_form)
        print('init_lm_lite form %d bbox %d: init status %s, lm status %s, iterations %s' % (pose_form, new_bbox, [i['status'] for i in inits], [s['status'] for s in stats], [s['iterations'] for s in stats]))
        for k in range(len(objs)):
            assert inits[k]['status'] == alone[k]['status'] and np.array_equal(inits[k]['wTo'], alone[k]['wTo'])
            assert inits[k]['d'] == alone[k]['d'] or (np.isnan(inits[k]['d']) and np.isnan(alone[k]['d']))
            if inits[k]['status'] != 1:
                assert k == 3 and stats[k] == dict(cost0=0.0, cost=0.0, iterations=0, evaluations=0, status=0)
                assert np.array_equal(tracks[k].wTo, np.eye(4)) and np.array_equal(tracks[k].shape, ms[k])
                continue
            start = dataclasses.replace(objs[k], wTo=alone[k]['wTo'], shape=np.array(ms[k]))
            t2, s2 = upd.object_lm_lite([start], [ms[k]], True, new_bbox, max_iter=lc.MAX_ITER)
            assert s2[0] == stats[k] and stats[k]['status'] in (1, 2, 3)
            assert np.array_equal(t2[0].wTo, tracks[k].wTo) and np.array_equal(t2[0].shape, tracks[k].shape)
            assert tracks[k].kps.shape == (0, 3)


def _raw(upd, which, obj, ms, mutate):
    """One of the three C calls on one object with the caller's records changed by `mutate` before it; returns (code, result arrays)."""
    lib = upd.lib
    cfg = upd._lite_config(True, 0, lc.UNIT, 0, None, None)
    icfg = upd._lite_init_config(None, None)
    arr, keep = upd._lite_tracks([obj], True)
    msc = np.ascontiguousarray(ms, dtype=np.float64)
    pri = (capi.ObjectLMPrior * 1)(capi.ObjectLMPrior(capi._d(msc), None))
    ptr = (capi._dp * 1)(capi._d(msc))
    out = [np.zeros(16), np.zeros(3), np.zeros(16)]
    res = (capi.ObjectLMResult * 1)()
    res[0].wTo, res[0].shape = capi._d(out[0]), capi._d(out[1])
    ires = (capi.ObjectInitLiteResult * 1)()
    ires[0].wTo = capi._d(out[2])
    st = dict(tracks=arr, priors=pri, means=ptr, results=res, iresults=ires, n=1, cfg=C.byref(cfg), cfg_rec=cfg, icfg=C.byref(icfg), icfg_rec=icfg)
    mutate(st)
    if which == 'lm':
        rc = lib.orcvio_msckf_object_lm_lite(upd.h, st['cfg'], st['tracks'], st['priors'], st['n'], st['results'])
    elif which == 'init':
        rc = lib.orcvio_msckf_object_init_lite(upd.h, st['icfg'], st['tracks'], st['means'], st['n'], st['iresults'])
    else:
        rc = lib.orcvio_msckf_object_init_lm_lite(upd.h, st['icfg'], st['cfg'], st['tracks'], st['priors'], st['n'], st['iresults'], st['results'])
    return rc, out


def test_refusals_come_before_anything_runs(upd):
    """K != 0, F = 0, F = 129, NaN pose / box / mean / weight, null pointers, max_iter = 0, more tracks than the handle holds:
    ORCVIO_ERR_INVALID (1) / ORCVIO_ERR_CAPACITY (3) from all three calls, the result arrays untouched; the handle serves the next call."""
    obj, ms = lc.synthetic(2, 2)
    upd.object_init_lm_lite([obj], [ms], True, 0)    # (binds the argument types of the three calls)
    upd.object_init_lite([obj], [ms])
    upd.object_lm_lite([obj], [ms], True, 0)
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

    def nan_in(field, n):
        def f(st):
            bad = np.ascontiguousarray(np.ctypeslib.as_array(getattr(st['tracks'][0], field), shape=(n,))).copy()
            bad[n - 1] = np.nan
            st['keep_' + field] = bad
            setattr(st['tracks'][0], field, capi._d(bad))
        return f

    def nan_mean(st):
        bad = np.array([ms[0], np.nan, ms[2]])
        st['keep_mean'] = bad
        st['priors'][0].mean_shape = capi._d(bad)
        st['means'][0] = capi._d(bad)

    def null_result(st):
        st['results'][0].shape = None
        st['iresults'][0].wTo = None

    def null_mean(st):
        st['priors'][0].mean_shape = None
        st['means'][0] = None

    def max_iter_0(st):
        st['cfg_rec'].max_iter = 0

    def nan_weight(st):
        st['cfg_rec'].residual_weights[1] = float('nan')

    def bad_form(st):
        st['icfg_rec'].pose_form = 3

    def nan_scale(st):
        st['icfg_rec'].bbox_scale[2] = float('nan')

    every = ('lm', 'init', 'init_lm')
    cases = [('K = 1', setter(n_keypoints=1), INVALID, every), ('F = 0', setter(n_frames=0), INVALID, every),
             ('F = 129', setter(n_frames=129), CAPACITY, every), ('NaN pose', nan_in('frame_wTc', 32), INVALID, every),
             ('NaN box', nan_in('frame_bbox', 8), INVALID, every), ('NaN start', nan_in('wTo', 16), INVALID, ('lm',)),
             ('NaN mean', nan_mean, INVALID, every), ('null frame_bbox', setter(frame_bbox=None), INVALID, every),
             ('null start', setter(wTo=None), INVALID, ('lm',)), ('null result array', null_result, INVALID, every),
             ('null mean', null_mean, INVALID, every), ('null tracks', key('tracks', None), INVALID, every),
             ('negative count', key('n', -1), INVALID, every), ('more tracks than the handle holds', key('n', 65), CAPACITY, every),
             ('max_iter = 0', max_iter_0, INVALID, ('lm', 'init_lm')), ('NaN weight', nan_weight, INVALID, ('lm', 'init_lm')),
             ('null config', key('cfg', None), INVALID, ('lm', 'init_lm')), ('null start config', key('icfg', None), INVALID, ('init', 'init_lm')),
             ('pose_form = 3', bad_form, INVALID, ('init', 'init_lm')), ('NaN bbox_scale', nan_scale, INVALID, ('init', 'init_lm'))]
    for tag, mutate, want, calls in cases:
        for which in calls:
            rc, out = _raw(upd, which, obj, ms, mutate)
            assert rc == want, (tag, which, rc)
            assert not any(o.any() for o in out), (tag, which)
    for which in every:
        rc, out = _raw(upd, which, obj, ms, lambda st: None)
        assert rc == 0 and (out[0].any() or which == 'init') and (out[2].any() or which == 'lm')
        rc, _ = _raw(upd, which, obj, ms, key('n', 0))   # no tracks: nothing to do
        assert rc == 0
    # the keypoint calls keep refusing K = 0, the lite calls take what they refuse
    with pytest.raises(capi.MsckfError):
        upd.object_lm([obj], [ms], [np.zeros((0, 3))], True, 0, (1.0, 1.0, 1.0, 1.0))


def test_init_lm_lite_then_object_update_end_to_end(upd):
    """The intended sequence for a bbox-only deployment: orcvio_msckf_object_init_lm_lite's result goes into
    orcvio_msckf_update_object_tracks as a track with n_keypoints = 0, as it is.  Device chain against the mirror's chain (its start,
    its optimiser) plus the mirror's literal update, with the shipped pose form, on the 30-frame synthetic track of seed 1 with every
    frame in the window: from that start the mirror's two charts end at one optimum (1.9e-9 apart in Q_w) and the reference's gate
    accepts (gamma 40.7 at 111 degrees of freedom).  On one_car the start of frame 0 -- an identity rotation -- leads the two charts
    into different minima, so no chain is compared there."""
    N = 30
    obj, ms = lc.synthetic(N, 1)
    obj = dataclasses.replace(obj, frames=[dict(fr, clone=i, zs=np.zeros((0, 2))) for i, fr in enumerate(obj.frames)])
    flags = synth.Flags(use_larvio=0, use_left_perturbation=0, noise_feature=0.05)
    win = synth.make_window(N=N, F=2, seed=2, flags=flags, track_len=3)
    mi = ml.init(obj.frames, ms)
    start = dataclasses.replace(obj, wTo=mi['wTo'], shape=np.array(ms))
    mir, other = (ml.solve(start, ms, ml.Config(left=left, max_iter=lc.MAX_ITER)) for left in (True, False))
    assert max(ml.distance(mir, other)) <= lc.CAP
    ref = objects_update_reference(win, [dataclasses.replace(obj, wTo=mir['wTo'], shape=mir['shape'])], win.P, True, False, 0)
    inits, tracks, stats = upd.object_init_lm_lite([obj], [ms], True, 0, max_iter=lc.MAX_ITER)
    dq, dv = ml.distance(dict(wTo=tracks[0].wTo, shape=tracks[0].shape), mir)
    print('end to end: lm status %d / %d, iterations %d / %d, Q_w %.2e, v %.2e' % (stats[0]['status'], mir['status'], stats[0]['iterations'], mir['iterations'], dq, dv))
    assert inits[0]['status'] == 1 and stats[0]['status'] == 1 and mir['status'] == 1
    got = upd.update_object_tracks(flags, win.N, tracks, win.P, win.R_b2c[0], win.t_c_b[0], True, False, 0)
    print('end to end: accept %d / %d, gamma %.9g / %.9g, dof %d' % (got['accept'], ref['accept'], got['gamma'], ref['gamma'], ref['dof']))
    assert ref['accept'] == 1   # (the gate takes this object: the comparison of dx and P+ below is not optional)
    assert got['accept'] == ref['accept']
    assert abs(got['gamma'] - ref['gamma']) < 1e-6 * abs(ref['gamma'])
    assert got['stats'][0] == ref['dof']
    assert rel(got['dx'], ref['dx']) < 1e-6 and rel(got['P_new'], ref['P_new']) < 1e-6
