"""TEST INFRASTRUCTURE ONLY -- the host chain of ONE filter frame (OrcVIO::processFeatures, src/orcvio.cpp:567-594) on the
covariance, built from the numpy mirrors; the checker of orcvio_msckf_io_step_frame.

  1  mirror_cov.propagate         processModel, :800-816
  2  mirror_cov.augment(rest=..)  stateAugmentation, :962-1010 (the new clone in front of the in-state feature rows)
  3  mirror_hybrid.hybrid_update  removeLostFeatures, :2444-2560: the lost tracks and the in-state features' rows
  4  increment_window (below)     incrementState_IMUCam, :4468-4567, with the first update's dx (only when apply_dx)
  5  mirror.msckf_update          pruneImuStateBuffer's update, :2803-2851, on the prune tracks (n_extra columns behind the clones)
  6  mirror_cov.remove_clones     the marginalisation, :2935-2951

Nothing under orcvio_amd/ may import this module.
"""
import dataclasses

import numpy as np

from oracle import mirror, mirror_cov, mirror_hybrid


def increment_window(win, dx, flags, imu_extrinsic=None):
    """incrementState_IMUCam (:4468-4567) on the clones of a synth.Window, with mirror.increment_state's arithmetic: the window
    the reference's state flattens to for the NEXT update of the frame.  Clone R_b2w / t_b_w are incremented; t_fej is the first
    estimate and stays; every clone keeps the R_b2c / t_c_b it froze at its augmentation (:950-951) -- the clone loop
    (:4535-4565) writes only orientation_cam / position_cam.  Only the IMU's extrinsic moves by dx[15:21] (:4512-4517): it is
    returned beside the window.  imu_extrinsic: the IMU's (R_b2c, t_c_b) before the increment (default: the newest clone's, which
    froze it at the augmentation in front of the update).
    Returns (window, applied, (R_b2c, t_c_b) of the IMU); discard_large_update: (win unchanged, False, imu_extrinsic)."""
    N = win.N
    R_ext, t_ext = (win.R_b2c[N - 1], win.t_c_b[N - 1]) if imu_extrinsic is None else imu_extrinsic
    state = dict(R_b2w_imu=np.eye(3), v=np.zeros(3), p=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3),
                 R_b2c=np.array(R_ext, dtype=np.float64), t_c_b=np.array(t_ext, dtype=np.float64), td=np.zeros(1),
                 R_b2w=np.array(win.R_b2w, dtype=np.float64), t_b_w=np.array(win.t_b_w, dtype=np.float64))
    s, applied = mirror.increment_state(state, np.asarray(dx, dtype=np.float64)[:flags.leg_dim + 6 * N], flags)
    if not applied:
        return win, False, (state['R_b2c'], state['t_c_b'])
    out = dataclasses.replace(win, R_b2w=np.ascontiguousarray(s['R_b2w']), t_b_w=np.ascontiguousarray(s['t_b_w']),
                              t_fej=win.t_fej.copy(), R_b2c=win.R_b2c.copy(), t_c_b=win.t_c_b.copy())
    return out, True, (s['R_b2c'], s['t_c_b'])


def prune_window(prune, dx, flags, apply_dx, increment=None):
    """The window of the frame's second update: the prune tracks on the first update's poses, incremented by its dx when
    apply_dx (step 4).  increment(win, dx, flags) -> (win, applied, ...); default: the literal increment_window above.
    Returns (window, applied)."""
    if not apply_dx or dx is None:
        return prune, False
    out = (increment or increment_window)(prune, dx, flags)
    return out[0], bool(out[1])


def step_frame(P, fr, idp, apply_dx, augment=True, increment=None, table=None):
    """P: the covariance in front of the frame; fr: a frame of synth.make_stream (w, slam, prune, Phi, Q, remove).
    Returns dict(dx, gamma, accept, ekf_accept, prune_dx, prune_gamma, prune_accept, applied, P, n_after) -- dx is None when the
    frame has no first update (no lost track, no in-state feature), prune_* None without prune tracks."""
    w, slam = fr['w'], fr.get('slam') or []
    fl = w.flags
    table = mirror.chi2_table(fl.chi2_prob) if table is None else table
    if fr.get('Phi') is not None:
        P = mirror_cov.propagate(P, fr['Phi'], fr['Q'])
    if augment:
        P = mirror_cov.augment(P, rest=w.n_extra)
    assert P.shape[0] == w.n, (P.shape, w.n)
    out = dict(dx=None, gamma=None, accept=None, ekf_accept=None, prune_dx=None, prune_gamma=None, prune_accept=None, applied=False)
    if w.F > 0 or slam:
        ref = mirror_hybrid.hybrid_update(dataclasses.replace(w, P=P), slam, idp, table=table)
        out.update(dx=ref['dx'], gamma=ref['gamma'], accept=ref['accept'], ekf_accept=ref['ekf_accept'])
        P = ref['P_new']
    if fr.get('prune') is not None:
        win2, out['applied'] = prune_window(fr['prune'], out['dx'], fl, apply_dx, increment)
        ref2 = mirror.msckf_update(dataclasses.replace(win2, P=P), table=table)
        out.update(prune_dx=ref2['dx'], prune_gamma=ref2['gamma'], prune_accept=ref2['accept'])
        P = ref2['P_new']
    if fr.get('remove'):
        P = mirror_cov.remove_clones(P, fl.leg_dim, fr['remove'])
    out.update(P=P, n_after=P.shape[0])
    return out
