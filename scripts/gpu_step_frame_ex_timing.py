"""Host-visible time per frame class of the one-call frame with feature events (orcvio_msckf_io_step_frame_ex, GPU) against the
separate-call sequence it replaces (cov_propagate, cov_augment, cov_remove_features, update, cov_change_anchors, update,
cov_remove_clones) and, for plain frames, against orcvio_msckf_io_step_frame.  Frames of synth.make_lifecycle_stream (euroc flags,
idp 1) and variants of its first prune frame with 0 / 1 / 4 / 16 anchor changes.  Every sample starts from the same resident
covariance (cov_set + sync outside the timed region: no factor is known, for every way alike); the timed region is the call(s) of
the frame up to their return -- each ends in the wait for its last update's results (the marginalisation behind it is enqueued in
every way and synchronised outside).  The ways alternate in blocks; reported per class and way: median and p95 over all samples,
and the block medians (their spread is the yardstick for a difference).  Microseconds.
usage: python scripts/gpu_step_frame_ex_timing.py [--blocks 5] [--reps 40] [--tag r4c]"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from orcvio_amd import capi, synth  # noqa: E402
from orcvio_amd import build as b  # noqa: E402
import mirror_frame_lifecycle as mfl  # noqa: E402

IDP, LEG = 1, 22


def by_ex(u, fr):
    u.set_extra_states(fr['w'].n_extra)
    return u.io_step_frame_ex(fr['w'], fr['Phi'], fr['Q'], True, fr['slam'], IDP, fr['prune'], False, fr['remove'],
                              n_feature_states=fr['n_feature_states'], lost=fr['lost'], changes=fr['changes'], R_b2c=fr['R_b2c'], t_c_b=fr['t_c_b'])


def by_step(u, fr):
    u.set_extra_states(fr['w'].n_extra)
    return u.io_step_frame(fr['w'], fr['Phi'], fr['Q'], True, fr['slam'], IDP, fr['prune'], False, fr['remove'])


def by_calls(u, fr):
    w = fr['w']
    u.set_extra_states(IDP * fr['n_feature_states'])
    u.cov_propagate(fr['Phi'], fr['Q'])
    u.cov_augment()
    u.cov_remove_features(LEG, w.N, IDP, fr['n_feature_states'], fr['lost'])
    u.set_extra_states(w.n_extra)
    io = u.io_begin(w.flags, w.N, w.F, int(w.obs_ptr[-1]), with_P=False)
    u.io_fill(io, w, with_P=False)
    u.make_slam_call(IDP, fr['slam'])()
    u.io_update(want_P=False, commit=True)
    if fr['changes']:
        u.cov_change_anchors(w.flags, IDP, synth.pack_poses(w), fr['R_b2c'], fr['t_c_b'], fr['changes'])
    if fr['prune'] is not None:
        p = fr['prune']
        io = u.io_begin(p.flags, p.N, p.F, int(p.obs_ptr[-1]), with_P=False)
        u.io_fill(io, p, with_P=False)
        u.io_update(want_P=False, commit=True)
    if fr['remove']:
        u.cov_remove_clones(LEG, fr['remove'])


def prune_variant(fr, nf, k):
    """frames[1]'s window with nf in-state features, none lost, exactly k of them anchored in the leaving clones."""
    w = dataclasses.replace(fr['w'], n_extra=IDP * nf)
    slam = synth.make_slam_features(w, nf, seed=1, outlier_frac=0.1)
    changes = []
    for j in range(nf):
        if j < k:
            slam[j] = synth._reanchor(w, slam[j], j % 2)
            changes.append(synth.LifecycleChange(j, j % 2, 7, slam[j].p_w.copy(), slam[j].p_fej.copy()))
        elif slam[j].anchor in (0, 1):
            slam[j] = synth._reanchor(w, slam[j], 5)
    return dict(fr, w=w, prune=dataclasses.replace(fr['prune'], n_extra=IDP * nf), slam=slam, n_feature_states=nf, lost=[], changes=changes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--tag', default=None)
    args = ap.parse_args()
    fl = synth.Flags(use_larvio=1)
    frames, P0 = synth.make_lifecycle_stream(fl)
    P1 = mfl.step_frame(P0, frames[0], IDP, 0)['P']   # the covariance in front of the stream's first prune frame
    f0, f1 = frames[0], frames[1]
    assert f1['lost'] and f1['changes'] and f1['prune'] is not None
    w14 = dataclasses.replace(f0['w'], n_extra=IDP * 14)
    classes = {
        'plain': (P0, f0, True),
        'lost_only': (P0, dict(f0, w=w14, slam=f0['slam'][:14], lost=[3, 7]), False),
        'prune_no_change': (P1, prune_variant(f1, 16, 0), True),
        'prune_1_change': (P1, prune_variant(f1, 16, 1), False),
        'prune_4_changes': (P1, prune_variant(f1, 16, 4), False),
        'prune_16_changes': (P1, prune_variant(f1, 16, 16), False),
        'lost_prune_change': (P1, f1, False),
    }
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096)
    u.set_ekf_rows_mode(True)
    out = dict(build=dict(source_sha16=b.source_sha16()), blocks=args.blocks, reps=args.reps, unit='us', classes={})
    for name, (P, fr, plain) in classes.items():
        ways = dict(ex=by_ex, calls=by_calls)
        if plain:
            ways['step'] = by_step
        samples = {k: [] for k in ways}
        block_med = {k: [] for k in ways}
        for blk in range(args.blocks + 1):   # (block 0: warm-up of every way's shapes)
            for k, fn in ways.items():
                ts = []
                for _ in range(args.reps):
                    u.cov_set(P)
                    u.sync()
                    t0 = time.perf_counter()
                    fn(u, fr)
                    ts.append((time.perf_counter() - t0) * 1e6)
                    u.sync()
                if blk > 0:
                    samples[k] += ts
                    block_med[k].append(float(np.median(ts)))
        row = {}
        for k in ways:
            a = np.sort(samples[k])
            row[k] = dict(median=float(np.median(a)), p95=float(a[int(0.95 * (len(a) - 1))]), block_medians=block_med[k])
        row['n_changes'] = len(fr['changes']); row['n_lost'] = len(fr['lost']); row['n'] = int(fr['w'].n)
        out['classes'][name] = row
    out['counters'] = u.counters()
    u.close()
    line = json.dumps(out)
    if args.tag:
        with open(os.path.join(ROOT, 'profiles', f'{args.tag}_step_frame_ex_timing.json'), 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
