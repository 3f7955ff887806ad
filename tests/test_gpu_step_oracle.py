"""One filter frame in one call (orcvio_msckf_io_step_frame) against the host chain of the same frame (oracle/mirror_frame.py:
propagation, augmentation, the hybrid update, the literal incrementState_IMUCam, the prune update, the marginalisation) -- not
against the separate calls of the library.  One cycle of synth.make_stream per flag set, with and without the state increment on
the device (prune_apply_dx); and a stream whose clones carry extrinsics of their own while P's extrinsic rows are live, on every
launch path of the frame's pose step."""
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror, mirror_frame
from helpers import rel

pytestmark = pytest.mark.gpu
NSLAM = 12
TOL = 1e-8
SPREAD = 5e-3   # per-clone extrinsic perturbation (rad, m)
EUROC = dict(use_larvio=1)
KITTI = dict(use_larvio=0, use_left_perturbation=0, noise_feature=1.0, discard_large_update=1)
# name: (flags, sigma_px, idp, leg)
FLAG_SETS = {
    'euroc': (EUROC, None, 1, 22),
    'kitti': (KITTI, 0.008, 1, 22),
    'left': (dict(use_larvio=0, use_left_perturbation=1), None, 1, 22),
    'fej_td': (dict(use_larvio=1, if_fej=1, estimate_td=1), None, 1, 22),
    'leg46': (dict(use_larvio=1, leg_dim=46), None, 1, 46),
    'idp3': (EUROC, None, 3, 22),
}
_CHAINS = {}


def _stream(name, extrin):
    fl, sigma_px, idp, leg = FLAG_SETS[name]
    kw = dict(estimate_extrin=True, clone_extrinsic_spread=SPREAD) if extrin else {}
    frames, P0 = synth.make_stream(synth.Flags(**fl), sigma_px=sigma_px, cycle=8, idp=idp, leg=leg, **kw)
    return frames, P0, idp


def _chain(name, extrin, apply_dx):
    """The oracle's frames of one stream (cached: the launch-path variants share it), each with the prune update as it would run
    if every clone's extrinsic took the IMU's extrinsic increment, from the same covariance."""
    key = (name, extrin, apply_dx)
    if key not in _CHAINS:
        frames, P0, idp = _stream(name, extrin)
        table = mirror.chi2_table(frames[0]['w'].flags.chi2_prob)
        P, refs = P0, []
        for fr in frames:
            ref = mirror_frame.step_frame(P, fr, idp, apply_dx, table=table)
            if extrin and fr['prune'] is not None:
                ref['prune_dx_every_clone'] = mirror_frame.step_frame(P, fr, idp, apply_dx, increment=_increment_every_clone, table=table)['prune_dx']
            refs.append(ref)
            P = ref['P']
        _CHAINS[key] = (frames, P0, idp, refs)
    return _CHAINS[key]


def _increment_every_clone(win, dx, flags):
    """The convention this test guards against: the IMU's extrinsic increment applied to every clone's extrinsic."""
    out, applied, ext = mirror_frame.increment_window(win, dx, flags)
    if not applied:
        return out, applied, ext
    Rq = mirror.quat_to_rot_hamilton(mirror.small_angle_quaternion(dx[15:18]))
    return dataclasses.replace(out, R_b2c=np.ascontiguousarray(win.R_b2c @ Rq.T), t_c_b=np.ascontiguousarray(win.t_c_b + dx[18:21])), True, ext


def _handle(idp, debug_hooks=False):
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096, debug_hooks=debug_hooks)
    u.set_extra_states(idp * NSLAM)
    u.set_ekf_rows_mode(True)
    return u


def _gamma_err(got, ref):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    return rel(got[~nan], ref[~nan]) if (~nan).any() else 0.0


def _run(u, name, extrin, apply_dx, repaired=False):
    """Every frame of the stream through io_step_frame on `u`, each against the oracle's; returns the worst errors."""
    frames, P0, idp, refs = _chain(name, extrin, apply_dx)
    worst = dict(dx=0.0, prune_dx=0.0, P=0.0, gamma=0.0)
    u.cov_set(P0)
    for it, (fr, ref) in enumerate(zip(frames, refs)):
        got = u.io_step_frame(fr['w'], fr['Phi'], fr['Q'], True, fr['slam'], idp, fr['prune'], apply_dx, fr['remove'])
        assert got['rc'] == 0 and got['status_first'] == 0 and got['status_prune'] == 0, (it, got['rc'], got['status_first'], got['status_prune'])
        if repaired:   # ORCVIO_LA_SPIN=0: every update of the frame run again the safe way
            assert got['repaired'] == (2 if fr['prune'] is not None else 1), (it, got['repaired'])
        else:
            assert got['repaired'] == 0, it
        assert np.array_equal(got['accept'], ref['accept']), it
        worst['gamma'] = max(worst['gamma'], _gamma_err(got['gamma'], ref['gamma']))
        worst['dx'] = max(worst['dx'], rel(got['dx'], ref['dx']))
        if fr['prune'] is not None:
            assert np.array_equal(got['prune_accept'], ref['prune_accept']), it
            worst['prune_dx'] = max(worst['prune_dx'], rel(got['prune_dx'], ref['prune_dx']))
        else:
            assert got['prune_dx'] is None
        Pg = u.cov_get()
        assert got['n_after'] == ref['n_after'] == Pg.shape[0], it
        worst['P'] = max(worst['P'], rel(Pg, ref['P']))
        assert max(worst.values()) <= TOL, (it, worst)
    return worst


@pytest.mark.parametrize('apply_dx', [0, 1], ids=['copy', 'increment'])
@pytest.mark.parametrize('name', list(FLAG_SETS))
def test_step_frame_against_the_oracle(built, name, apply_dx):
    idp = FLAG_SETS[name][2]
    u = _handle(idp)
    try:
        worst = _run(u, name, False, apply_dx)
    finally:
        u.close()
    print(f'{name} prune_apply_dx={apply_dx}: worst rel err', worst)


@pytest.mark.parametrize('name', ['euroc', 'kitti'])
def test_step_frame_with_per_clone_extrinsics(built, name):
    """estimate_extrin with clone extrinsics of their own and the increment on the device: every clone keeps the extrinsic it
    froze at its augmentation (reference src/orcvio.cpp:950-951, 4535-4565)."""
    frames, P0, idp, refs = _chain(name, True, 1)
    assert np.abs(refs[0]['dx'][15:21]).max() > 0   # the extrinsic rows are live
    guard = max(rel(r['prune_dx_every_clone'], r['prune_dx']) for r in refs if r['prune_dx'] is not None)
    assert guard > 1e-4, guard   # the convention of every clone's extrinsic moving would not pass
    u = _handle(idp)
    try:
        worst = _run(u, name, True, 1)
    finally:
        u.close()
    print(f'{name} per-clone extrinsics: worst rel err', worst, 'guard', guard)


@pytest.mark.parametrize('off', ['ORCVIO_STEP_FUSED', 'ORCVIO_LA_SPIN'])
def test_per_clone_extrinsics_on_the_other_launch_paths(built, monkeypatch, off):
    """ORCVIO_STEP_FUSED=0 (diagnostics build): k_pose_step as a launch of its own instead of inside k_frame_head;
    ORCVIO_LA_SPIN=0: the look-ahead waits give up and the call runs both updates again the safe way."""
    monkeypatch.setenv(off, '0')
    u = _handle(1, debug_hooks=off == 'ORCVIO_STEP_FUSED')
    monkeypatch.delenv(off)
    try:
        worst = _run(u, 'euroc', True, 1, repaired=off == 'ORCVIO_LA_SPIN')
    finally:
        u.close()
    print(f'{off}=0 per-clone extrinsics: worst rel err', worst)
