"""A/B of the two commits of an update with entering features on the resident covariance (GPU box), in ONE process, alternating,
after warm-up, with a host clock around work that ends in the call's own wait:
    route A   orcvio_msckf_cov_commit_new_features (drops the factor), then the frame's next committed resident update
    route B   orcvio_msckf_cov_commit_new_features_fac (carries the factor), then the same update
Operating point, the hybrid configurations': leg 22, 20 clones, 12 in-state features of width d = 1 and 3, 1 and 3 entering features,
a second update of 40 tracks.  Per (d, k): medians, quartiles, min and max of the commit call alone, of commit + update (to the update's
own wait) and of commit + update + cov_commit + sync.  The timed loop is run `--repeats` times; B counts as faster only if the median of
its repeats' medians beats A's by more than A's own max - min over the repeats.
usage: python scripts/gpu_entering_commit_ab.py [--steps 200] [--warmup 20] [--repeats 5] [--out record.json]
(without --out the record goes to standard output behind the per-configuration lines)"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from orcvio_amd import capi, synth
from orcvio_amd import build as b
from helpers import rel
import entering_cases as ec

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--warmup', type=int, default=20)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--out', default=None)
args = ap.parse_args()

LEG, N, NF, F2 = 22, 20, 12, 40
upd = capi.MsckfUpdater(device=0, max_clones=32, max_features=512, max_observations=16384)


def make(d, k):
    fl = synth.Flags(estimate_td=1, leg_dim=LEG, use_larvio=1)
    w0 = synth.make_window(N=N, F=30, seed=71, track_len=(3, 9), flags=fl)
    w = synth.with_extra_states(w0, d * NF, seed=4)
    slam = synth.make_slam_features(w, NF, seed=5 + d, outlier_frac=0.25)
    new = ec.make_entering_features(w, ec.specs_for('small', w.N, k), seed=10 * d + k)
    n2 = w.n + d * k
    w2 = synth.make_window(N=N, F=F2, seed=3, track_len=(3, 12), flags=synth.Flags(leg_dim=LEG))
    w2 = dataclasses.replace(w2, P=np.eye(n2), n_extra=n2 - LEG - 6 * N)
    return w, slam, new, w2


def frame(route, d, w, slam, new, w2):
    """one frame; returns (commit, commit + update, commit + update + commit + sync) in microseconds and the second update's dx"""
    upd.cov_set(w.P)
    upd.cov_prefactor()
    upd.set_extra_states(w.n_extra); upd.set_ekf_rows_mode(True)
    try:
        upd.upload(w, resident_cov=True)
        upd.upload_slam_features(d, slam)
        upd.upload_new_features(w, d, new)
        upd.run_update(); upd.sync()
        upd.download()
        t0 = time.perf_counter()
        if route == 'A':
            upd.cov_commit_new_features()
        else:
            upd.cov_commit_new_features_fac()
        t1 = time.perf_counter()
        upd.set_ekf_rows_mode(False)
        upd.set_extra_states(w2.n_extra)
        got = upd.update_features(w2, resident_cov=True, want_P=False)
        t2 = time.perf_counter()
        upd.cov_commit(); upd.sync()
        t3 = time.perf_counter()
    finally:
        upd.set_ekf_rows_mode(False); upd.set_extra_states(0)
    return (1e6 * (t1 - t0), 1e6 * (t2 - t0), 1e6 * (t3 - t0)), got['dx']


def summary(x):
    q = np.percentile(np.asarray(x), [0, 25, 50, 75, 100])
    return dict(min=float(q[0]), q1=float(q[1]), median=float(q[2]), q3=float(q[3]), max=float(q[4]))


out = dict(build=dict(source_sha16=b.source_sha16()), steps=args.steps, warmup=args.warmup, repeats=args.repeats,
           operating_point=dict(leg=LEG, clones=N, in_state_features=NF, second_update_tracks=F2), unit='us', configs=[])
for d in (1, 3):
    for k in (1, 3):
        w, slam, new, w2 = make(d, k)
        dxs = {}
        for i in range(args.warmup):
            for route in ('A', 'B'):
                _, dxs[route] = frame(route, d, w, slam, new, w2)
        agree = rel(dxs['B'], dxs['A'])
        assert agree < 1e-6, agree
        names = ('commit', 'commit_update', 'commit_update_commit')
        reps = {r: {q: [] for q in names} for r in 'AB'}
        for rep in range(args.repeats):
            t = {r: [] for r in 'AB'}
            for i in range(args.steps):
                for route in (('A', 'B') if i % 2 == 0 else ('B', 'A')):
                    t[route].append(frame(route, d, w, slam, new, w2)[0])
            for r in 'AB':
                a = np.asarray(t[r])
                for j, q in enumerate(names):
                    reps[r][q].append(summary(a[:, j]))
        rec = dict(d=d, k=k, n=w.n, sz=d * k, second_update_dx_rel_B_vs_A=agree, routes={})
        for r in 'AB':
            rec['routes'][r] = {q: dict(median_of_medians=float(np.median([s['median'] for s in reps[r][q]])),
                                        medians=[s['median'] for s in reps[r][q]], per_repeat=reps[r][q]) for q in names}
        verdict = {}
        for q in names:
            ma, mb = rec['routes']['A'][q]['medians'], rec['routes']['B'][q]['medians']
            spread = max(ma) - min(ma)
            gain = float(np.median(ma) - np.median(mb))
            verdict[q] = dict(gain_us=gain, spread_of_A_us=float(spread), B_faster=bool(gain > spread), B_slower=bool(-gain > spread))
        rec['verdict'] = verdict
        out['configs'].append(rec)
        print('d=%d k=%d n=%d: ' % (d, k, w.n) + '  '.join('%s A %.1f B %.1f (gain %.1f, spread of A %.1f)' % (
            q, rec['routes']['A'][q]['median_of_medians'], rec['routes']['B'][q]['median_of_medians'], verdict[q]['gain_us'], verdict[q]['spread_of_A_us'])
            for q in names), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
else:
    print(json.dumps(out, indent=1))
upd.close()
