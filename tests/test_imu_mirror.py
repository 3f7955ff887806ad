"""CPU tests of the numpy restatement of the reference's IMU step (tests/mirror_imu.py): its closed forms of Phi against central
differences of its own predictors, the Euler forms against the closed forms, the accumulated pair against the per-sample application,
the non-finite case the device must refuse, and the spread between two accumulation orders that sets the device's regression bar."""
import numpy as np
import pytest

import imu_cases as ic
import mirror_imu as mi

EPS = 2.220446049250313e-16
NAMES = ('theta', 'v', 'p', 'b_g', 'b_a')
NONTRIVIAL = [(0, 0), (0, 3), (1, 0), (1, 3), (1, 4), (2, 0), (2, 1), (2, 3), (2, 4)]   # block (row, column) in units of three states


def so3_log_small(R):
    return 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])   # (angles of 1e-6: the cubic term is 1e-18)


def one_step(cfg, st, prev, row, fej=None):
    srv = mi.Server(cfg, st, fej_now=fej, m_gyro_old=prev[:3], m_acc_old=prev[3:])
    srv.process_model(float(row[0]), np.array(row[1:4]), np.array(row[4:7]))
    return srv


def perturbed(st, e, left):
    s = st.copy()
    dR = mi.so3_exp(e[0:3])
    s.R = dR @ st.R if left else st.R @ dR
    s.v = st.v + e[3:6]
    s.p = st.p + e[6:9]
    s.bg = st.bg + e[9:12]   # (the measurement minus the bias: the bias error is subtracted from it)
    s.ba = st.ba + e[12:15]
    return s


def numeric_phi(cfg, st, prev, row, left, h=1e-6):
    """central differences of the predictor in the error state (left: R = exp(dtheta) R^, right: R = R^ exp(dtheta))"""
    nom = one_step(cfg, st, prev, row).imu
    J = np.zeros((15, 15))
    for j in range(15):
        out = []
        for sgn in (1.0, -1.0):
            e = np.zeros(15)
            e[j] = sgn * h
            s = one_step(cfg, perturbed(st, e, left), prev, row).imu
            dth = so3_log_small(s.R @ nom.R.T) if left else so3_log_small(nom.R.T @ s.R)
            out.append(np.concatenate([dth, s.v - nom.v, s.p - nom.p, s.bg - nom.bg, s.ba - nom.ba]))
        J[:, j] = (out[0] - out[1]) / (2 * h)
    return J


def block_devs(Phi, J):
    return {(a, b): float(np.max(np.abs(Phi[3 * a:3 * a + 3, 3 * b:3 * b + 3] - J[3 * a:3 * a + 3, 3 * b:3 * b + 3]))) for (a, b) in NONTRIVIAL}


@pytest.mark.parametrize('rate', ic.IMU_RATES)
def test_right_closed_form_against_central_differences(rate):
    """Seven of the nine blocks are the derivative of predictNewStateOrcVIO under right perturbation.  The two b_g blocks (v, b_g) and
    (p, b_g) are NOT (src/orcvio.cpp:4343, :4348 as written): excluded by name, their deviation printed ("IMU propagation from raw samples")."""
    case = ic.make_case('right_closed', 1, n=22, seed=11, rate=rate)
    cfg, st, prev, row = case['cfg'], case['state'], case['prev'], case['samples'][0]
    Phi = one_step(cfg, st, prev, row).steps[0]['Phi']
    J = numeric_phi(cfg, st, prev, row, left=False)
    dev = block_devs(Phi, J)
    excluded = {(1, 3), (2, 3)}
    for (a, b), d in dev.items():
        print('right closed form, %g Hz: block (%s, %s) deviates %.3e%s' % (rate, NAMES[a], NAMES[b], d, '  [excluded: reference quirk]' if (a, b) in excluded else ''))
    # measured on this restatement at step 1e-6: <= 1.2e-10 on every one of the seven blocks at the three shipped rates (the central
    # difference's own truncation and cancellation error, 1e-16 / 1e-6); asserted at 1e-9
    assert max(d for k, d in dev.items() if k not in excluded) < 1e-9
    # the quirk is there: the (v, b_g) block is of order |a| dt |w|^-1-ish, nowhere near its derivative (which is of order |a| dt^2)
    assert dev[(1, 3)] > 1e-3


@pytest.mark.parametrize('flag_set', ['larvio', 'left_closed'])
@pytest.mark.parametrize('rate', ic.IMU_RATES)
def test_left_closed_form_against_central_differences(flag_set, rate):
    """The left / LARVIO closed form under left perturbation.  (v, theta), (p, theta) and (p, v) are exact derivatives of either
    predictor (they are written in terms of the predictor's own v, p increments) and (theta, theta) is the identity on both sides:
    these four hold to the central difference's own error.  The five bias blocks (theta, b_g), (v, b_g), (v, b_a), (p, b_g), (p, b_a)
    are the reference's trapezoid expressions (they average the previous sample's gyro into the rotation): they agree with the
    derivative to first order in dt only, and are held to that."""
    case = ic.make_case(flag_set, 1, n=22, seed=12, rate=rate)
    cfg, st, prev, row = case['cfg'], case['state'], case['prev'], case['samples'][0]
    Phi = one_step(cfg, st, prev, row).steps[0]['Phi']
    J = numeric_phi(cfg, st, prev, row, left=True)
    dev = block_devs(Phi, J)
    dt = 1.0 / rate
    for (a, b), d in dev.items():
        print('%s, %g Hz: block (%s, %s) deviates %.3e' % (flag_set, rate, NAMES[a], NAMES[b], d))
    exact = [(0, 0), (1, 0), (2, 0), (2, 1)]
    assert max(dev[k] for k in exact) < 1e-9   # (measured <= 2.4e-10: the central difference's own error)
    # the bias blocks: first-order agreement.  Their size is dt (theta, v rows) or dt^2 (p row); the deviation is one order of dt
    # higher times the rates involved (|w| ~ 0.3 rad/s, |a| ~ 10 m/s^2): bounded by 10 dt^2 and 10 dt^3
    assert dev[(0, 3)] < 10 * dt ** 2 and dev[(1, 4)] < 10 * dt ** 2 and dev[(1, 3)] < 10 * dt ** 2
    assert dev[(2, 3)] < 10 * dt ** 3 and dev[(2, 4)] < 10 * dt ** 3


@pytest.mark.parametrize('left', [False, True])
def test_euler_form_is_the_closed_form_to_first_order(left):
    """Phi_Euler = I + dt F of its own closed form: the difference is O(dt^2), so halving dt quarters it.  Right: the two b_g blocks of
    the closed form are excluded by name (see above) -- the Euler form has zeros there."""
    errs = []
    for rate in (200.0, 400.0, 800.0):
        ce = ic.make_case('left_euler' if left else 'right_euler', 1, n=22, seed=13, rate=rate)
        cc = ic.make_case('left_closed' if left else 'right_closed', 1, n=22, seed=13, rate=rate)
        for c in (ce, cc):   # the same measurement at every rate: only dt changes
            c['samples'][0, 1:4] = ic.GYRO_MEAN
            c['samples'][0, 4:7] = ic.ACC_MEAN
            c['prev'][:] = np.concatenate([ic.GYRO_MEAN, ic.ACC_MEAN])
        st = ic.make_state(np.random.default_rng(99))
        Pe = one_step(ce['cfg'], st, ce['prev'], ce['samples'][0]).steps[0]['Phi']
        Pc = one_step(cc['cfg'], st, cc['prev'], cc['samples'][0]).steps[0]['Phi']
        D = np.abs(Pe - Pc)[:15, :15]
        if not left:
            D[3:9, 9:12] = 0.0
        errs.append(float(D.max()))
    print('euler vs closed (%s): %s, ratios %.3f %.3f' % ('left' if left else 'right', errs, errs[0] / errs[1], errs[1] / errs[2]))
    assert errs[0] > 0.0
    # second order: the ratio is 4 up to the third-order term's share, dt |w| ~ 2e-3 (and |a| dt / |v| for the position row): within 10 %
    assert 3.6 < errs[0] / errs[1] < 4.4 and 3.6 < errs[1] / errs[2] < 4.4


@pytest.mark.parametrize('flag_set,S,n', [('larvio', 128, 205), ('larvio', 10, 145), ('right_closed', 128, 205), ('left_euler', 33, 28)])
def test_accumulated_pair_applied_once_equals_the_per_sample_application(flag_set, S, n):
    case = ic.make_case(flag_set, S, n=n, seed=21, rate=ic.rate_for(S))
    srv, info = ic.run_mirror(case)
    assert info['n_propagated'] == S
    Phi, Q = mi.accumulate_sequential(srv.steps)
    once = mi.apply_once(case['P'], Phi, Q)
    rel = float(np.linalg.norm(once - srv.P) / np.linalg.norm(srv.P))
    print('%s S=%d n=%d: accumulated once against per sample, relative Frobenius %.2e' % (flag_set, S, n, rel))
    # every sample adds a few roundings of the IMU block's products (and one symmetrisation): 4 eps a sample.  Measured: 3e-15 at
    # S = 128, n = 205 and 3e-16 at S = 10, n = 145
    assert rel <= 4 * EPS * S


def test_zero_gyro_is_not_finite_in_the_right_closed_form_only():
    for flag_set, finite in (('right_closed', False), ('larvio', True), ('left_closed', True), ('right_euler', True)):
        case = ic.make_case(flag_set, 3, n=28, seed=2)
        case['samples'][1, 1:4] = case['state'].bg
        srv, _ = ic.run_mirror(case)
        Phi, Q = mi.accumulate_sequential(srv.steps)
        assert bool(np.isfinite(Phi).all() and np.isfinite(Q).all()) == finite, flag_set
        assert bool(np.isfinite(srv.steps[1]['Phi']).all()) == finite


def test_spread_between_two_accumulation_orders():
    """The device's regression bar is ten times this spread (imu_cases.MIRROR_SPREAD): measured here, on the mirror alone."""
    worst = 0.0
    where = None
    for (fs, S, n) in ic.gpu_cases():
        case = ic.gpu_case(fs, S, n)
        srv, _ = ic.run_mirror(case, with_P=False)
        Ps, Qs = mi.accumulate_sequential(srv.steps)
        Pp, Qp = mi.accumulate_pairwise(srv.steps)
        e = max(ic.block_error(Pp, Ps), ic.block_error(0.5 * (Qp + Qp.T), 0.5 * (Qs + Qs.T)),
                ic.block_error(mi.apply_once(case['P'], Pp, Qp), mi.apply_once(case['P'], Ps, Qs)))
        if e > worst:
            worst, where = e, (fs, S, n)
    print('mirror spread, sequential against pairwise: %.3e at %s' % (worst, where))
    # a band around the recorded figure, not the figure itself: accumulate_* and apply_once go through numpy's `@`, whose summation order
    # belongs to the BLAS build.  The device's bar stays the fixed constant ten times the RECORDED value
    assert 0.5 * ic.MIRROR_SPREAD <= worst <= 2.0 * ic.MIRROR_SPREAD
