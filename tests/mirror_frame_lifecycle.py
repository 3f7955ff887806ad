"""TEST INFRASTRUCTURE ONLY -- the host chain of ONE filter frame WITH the life cycle of the in-state features (OrcVIO::processFeatures,
src/orcvio.cpp:567-594), built from the numpy mirrors; the checker of orcvio_msckf_io_step_frame_ex.

  1  mirror_cov.propagate                               processModel, :800-816
  2  mirror_cov.augment                                 stateAugmentation, :962-1010
  3  mirror_features_lifecycle.rm_lost_features_cov     removeLostFeatures -> rmLostFeaturesCov, :2233, :3776-3828
  4  mirror_hybrid.hybrid_update                        the first update, on the tracks and the in-state features that stay
  5  mirror_frame.increment_window                      incrementState_IMUCam, :4468-4567 (only when apply_dx)
  6  mirror_features_lifecycle.increment_features       measurementUpdate_hybrid's feature loop, :1842-1889 -- it runs even when
                                                        incrementState_IMUCam has discarded dx (its early return is inside that function)
  7  mirror_features_lifecycle.change_anchors           pruneImuStateBuffer's in-state branch, :2664-2720
  8  mirror.msckf_update                                the prune update, :2803-2851
  9  mirror_cov.remove_clones                           the marginalisation, :2935-2951

With lost = [] and changes = [] the chain is oracle.mirror_frame.step_frame, call for call.  The keyword switches below are the
SHORTCUTS the tests guard against (each must move the result), not options of the filter.
Nothing under orcvio_amd/ may import this module.
"""
import dataclasses

import numpy as np

from orcvio_amd import synth
from oracle import mirror, mirror_cov, mirror_frame, mirror_hybrid
import mirror_features_lifecycle as mfl


def step_frame(P, fr, idp, apply_dx, literal_3d=0, table=None, skip_changes=False, increment_pw=True, increment_pose=True,
               increment_after_discard=True):
    """P: the covariance in front of the frame; fr: a frame of synth.make_lifecycle_stream (or of synth.make_stream).
    Returns mirror_frame.step_frame's dict plus new_param [k, 3], new_inv_depth [k], p_w_changed [k, 3]."""
    w, slam = fr['w'], fr.get('slam') or []
    fl = w.flags
    leg, N = fl.leg_dim, w.N
    lost, changes = list(fr.get('lost') or []), list(fr.get('changes') or [])
    table = mirror.chi2_table(fl.chi2_prob) if table is None else table
    if fr.get('Phi') is not None:
        P = mirror_cov.propagate(P, fr['Phi'], fr['Q'])
    P = mirror_cov.augment(P, rest=w.n_extra + idp * len(lost))
    if lost:
        P = mfl.rm_lost_features_cov(P, leg, N, idp, lost)
    assert P.shape[0] == w.n, (P.shape, w.n)
    out = dict(dx=None, gamma=None, accept=None, ekf_accept=None, prune_dx=None, prune_gamma=None, prune_accept=None, applied=False,
               new_param=None, new_inv_depth=None, p_w_changed=None)
    if w.F > 0 or slam:
        ref = mirror_hybrid.hybrid_update(dataclasses.replace(w, P=P), slam, idp, table=table)
        out.update(dx=ref['dx'], gamma=ref['gamma'], accept=ref['accept'], ekf_accept=ref['ekf_accept'])
        P = ref['P_new']
    derive = bool(apply_dx) and out['dx'] is not None
    win2 = None
    if fr.get('prune') is not None:
        win2, out['applied'] = mirror_frame.prune_window(fr['prune'], out['dx'], fl, apply_dx)
    if changes:
        base = fr['prune'] if fr.get('prune') is not None else w
        if win2 is None:
            win2, out['applied'] = mirror_frame.prune_window(base, out['dx'], fl, apply_dx)
        ext = (fr['R_b2c'], fr['t_c_b'])
        if derive:
            ext = mirror_frame.increment_window(base, out['dx'], fl, imu_extrinsic=ext)[2]
        poses = synth.pack_poses(win2 if increment_pose else base)
        p_w = [np.asarray(c.p_w, dtype=np.float64) for c in changes]
        if derive and increment_pw and (out['applied'] or increment_after_discard):
            by_slot = {j: f for j, f in enumerate(slam)}
            recs = [by_slot[c.slot] for c in changes]
            assert all(r.anchor == c.old for r, c in zip(recs, changes))
            fcol = leg + 6 * N
            dxf = np.concatenate([out['dx'][fcol + idp * c.slot: fcol + idp * (c.slot + 1)] for c in changes])
            _, _, pw_inc = mfl.increment_features(poses, [c.old for c in changes], [r.inv_param if idp == 3 else r.obs_anchor for r in recs],
                                                  [r.inv_depth for r in recs], dxf, idp)
            p_w = list(pw_inc)
        out['p_w_changed'] = np.array(p_w)
        if not skip_changes:
            chg = [mfl.AnchorChange(c.slot, c.old, c.new, pw, c.p_fej if fl.if_fej else None) for c, pw in zip(changes, p_w)]
            P, params, rhos, _ = mfl.change_anchors(P, leg, N, idp, poses, ext[0], ext[1], chg, if_fej=fl.if_fej, literal_3d=literal_3d)
            out.update(new_param=params, new_inv_depth=rhos)
    if fr.get('prune') is not None:
        ref2 = mirror.msckf_update(dataclasses.replace(win2, P=P), table=table)
        out.update(prune_dx=ref2['dx'], prune_gamma=ref2['gamma'], prune_accept=ref2['accept'])
        P = ref2['P_new']
    if fr.get('remove'):
        P = mirror_cov.remove_clones(P, fl.leg_dim, fr['remove'])
    out.update(P=P, n_after=P.shape[0])
    return out


def run_stream(frames, P0, idp, apply_dx, **kw):
    """The chain over a whole stream; returns the list of per-frame results (P carried from frame to frame)."""
    table = mirror.chi2_table(frames[0]['w'].flags.chi2_prob)
    P, refs = P0, []
    for fr in frames:
        ref = step_frame(P, fr, idp, apply_dx, table=table, **kw)
        refs.append(ref)
        P = ref['P']
    return refs
