"""The numpy mirror of the object Levenberg-Marquardt (tests/mirror_object_lm.py) checked on its own, on the CPU: its Jacobian
against central differences through the retraction, its optimum's independence of start and chart on the reference's one_car
track, the reference's own acceptance bounds, and the row-free special case of a keypoint nobody detected.  The device
(tests/test_gpu_object_lm.py) is compared with this mirror, within ten times the spread measured here."""
import numpy as np
import pytest

from oracle import mirror_objects as mo
from helpers import GOLDEN
import mirror_object_lm as mlm
import object_lm_cases as oc


@pytest.mark.parametrize('left', [True, False], ids=['left', 'right'])
@pytest.mark.parametrize('new_bbox', [0, 2])
def test_jacobian_matches_central_differences_through_the_retraction(left, new_bbox):
    """J of the stacked weighted residual, regulariser columns included, against (r(x + h e_j) - r(x - h e_j)) / 2h with x moved by
    the retraction, at a state off the start and off the means, all 47 frames.  Step 1e-6, bar 1e-7 as the project's other
    central-difference tests (measured: <= 8.3e-10)."""
    obj, ms, mk = oc.one_car(47, 0, 2)
    rng = np.random.default_rng(5)
    cfg = mlm.Config(left=left, new_bbox=new_bbox, weights=(1.0, 0.7, 1.3, 0.9))
    shape = obj.shape + 0.05 * rng.standard_normal(3)
    kps = obj.kps + 0.03 * rng.standard_normal(obj.kps.shape)
    r0, J = mlm.residual_jacobian(obj.wTo, shape, kps, obj.frames, ms, mk, cfg)
    h = 1e-6
    Jn = np.zeros_like(J)
    for j in range(J.shape[1]):
        d = np.zeros(J.shape[1])
        d[j] = h
        rp, _ = mlm.residual_jacobian(*mlm.retract(obj.wTo, shape, kps, d, left), obj.frames, ms, mk, cfg)
        rm, _ = mlm.residual_jacobian(*mlm.retract(obj.wTo, shape, kps, -d, left), obj.frames, ms, mk, cfg)
        Jn[:, j] = (rp - rm) / (2 * h)
    err = float(np.abs(J - Jn).max())
    print('left %d bbox %d: max |J - J_numeric| = %.2e over %d x %d' % (left, new_bbox, err, *J.shape))
    assert err < 1e-7


@pytest.mark.parametrize('name', list(oc.CASES))
def test_optimum_does_not_depend_on_start_or_chart(name):
    """Two projected starts x left / right perturbation: status 1 everywhere, one optimum.  The spread (largest element-wise
    difference of wTo, shape, keypoints over the four runs) is what the device test's tolerance is ten times of."""
    spread, runs = oc.case_spread(name)
    print('%s: spread %.2e, iterations %s, evaluations %s, cost %.9g' % (name, spread, [r['iterations'] for r in runs],
                                                                          [r['evaluations'] for r in runs], runs[0]['cost']))
    assert all(r['status'] == mlm.STATUS_CONVERGED for r in runs)
    assert spread <= 1e-6


def test_47_frame_optimum_is_inside_the_references_bounds():
    """test_object_lm_multiframe.cpp:119-123: |log(R_gt^T R)| < 0.5 and |t - t_gt| < 0.05 |t_gt|."""
    _, runs = oc.case_spread('f47')
    T, Tq = runs[0]['wTo'], oc.one_car_truth()
    dR = float(np.linalg.norm(mo.se3_log(np.block([[Tq[:3, :3].T @ T[:3, :3], np.zeros((3, 1))], [np.zeros((1, 3)), np.ones((1, 1))]]))[3:]))
    dt = float(np.linalg.norm(T[:3, 3] - Tq[:3, 3]))
    print('dR %.3f (< 0.5), dt %.3f (< %.3f)' % (dR, dt, 0.05 * np.linalg.norm(Tq[:3, 3])))
    assert dR < 0.5 and dt < 0.05 * np.linalg.norm(Tq[:3, 3])


def test_a_keypoint_detected_nowhere_stays_at_its_mean():
    """Keypoint 3 of the two-frame NaN case has only its regulariser: its block of A is w2^2 F I and its gradient is zero at the mean."""
    _, runs = oc.case_spread('f2_nan')
    _, _, mk = oc.one_car(2, 1, 0)
    for r in runs:
        assert np.abs(r['kps'][3] - mk[3]).max() <= 1e-12
    assert np.abs(runs[0]['kps'] - mk).max() > 1e-3   # (the others did move)


def test_regulariser_blocks_repeat_per_frame_with_identity_columns():
    """The two regulariser blocks as rows: F copies of w2 (m - mean) keypoint-major and of w3 (v - mean), identity columns at the
    keypoints' / the shape's place (ErrorDeformRegularization / ErrorQuadVRegularization, ObjectLM.cpp:652-759), and what they
    add to the normal equations: w^2 F on the diagonal, w^2 F (x - mean) in the gradient."""
    rng = np.random.default_rng(2)
    K, F, w2, w3 = 5, 3, 0.7, 1.9
    v, mv = rng.standard_normal(3), rng.standard_normal(3)
    m, mm = rng.standard_normal((K, 3)), rng.standard_normal((K, 3))
    rd, Jd, rs, Js = mlm.regulariser_rows(v, m, mv, mm, F, w2, w3)
    assert rd.shape == (3 * K * F,) and rs.shape == (3 * F,)
    for f in range(F):
        assert np.array_equal(rd[3 * K * f: 3 * K * (f + 1)], w2 * (m - mm).reshape(-1))
        assert np.array_equal(rs[3 * f: 3 * f + 3], w3 * (v - mv))
        assert np.array_equal(Jd[3 * K * f: 3 * K * (f + 1), 9:], w2 * np.eye(3 * K)) and not Jd[:, :9].any()
        assert np.array_equal(Js[3 * f: 3 * f + 3, 6:9], w3 * np.eye(3)) and not Js[:, :6].any() and not Js[:, 9:].any()
    J = np.vstack([Jd, Js])
    r = np.concatenate([rd, rs])
    A = J.T @ J
    assert np.allclose(np.diag(A)[9:], w2 * w2 * F, rtol=1e-14) and np.allclose(np.diag(A)[6:9], w3 * w3 * F, rtol=1e-14)
    assert np.allclose((J.T @ r)[9:], w2 * w2 * F * (m - mm).reshape(-1), rtol=1e-13)
    assert np.allclose((J.T @ r)[6:9], w3 * w3 * F * (v - mv), rtol=1e-13)


def test_regulariser_blocks_against_the_references_own_vectors():
    """src/tests/test_object_lm.cpp:235-290 on src/tests/data/test_error_deform_reg.h5 / test_error_mean_shape_reg.h5 (converted by
    scripts/convert_ref_h5.py, data only): the reference's error and 45-column Jacobian of ErrorDeformRegularization (36 rows, one
    frame) and ErrorQuadVRegularization (3 rows) -- row order, sign and columns of the mirror's two blocks."""
    g = np.load(GOLDEN + '/ref_test_error_deform_reg.npz')
    rd, Jd, _, _ = mlm.regulariser_rows(np.zeros(3), g['M'][:, :3], np.zeros(3), g['Mhat'], 1, 1.0, 1.0)
    assert np.abs(g['error']).max() > 1e-3
    assert np.abs(rd - g['error']).max() <= 1e-15 and np.array_equal(Jd, g['jacobian'])
    h = np.load(GOLDEN + '/ref_test_error_mean_shape_reg.npz')
    _, _, rs, Js = mlm.regulariser_rows(h['v'], np.zeros((12, 3)), h['mean_v'], np.zeros((12, 3)), 1, 1.0, 1.0)
    assert np.abs(h['error']).max() > 1e-3
    assert np.abs(rs - h['error']).max() <= 1e-15 and np.array_equal(Js, h['jacobian'])
