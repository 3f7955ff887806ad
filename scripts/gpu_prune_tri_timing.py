"""Host-visible time of a frame whose prune update triangulates its own tracks (orcvio_msckf_io_triangulate_prune inside
orcvio_msckf_io_step_frame, GPU) against the two routes a caller had before it:
  exact    first update with its wait, host increment, orcvio_msckf_triangulate on the incremented poses, second update, cov_remove_clones
           (the reference's order; two more host round trips)
  approx   orcvio_msckf_triangulate on the poses BEFORE the first update, in front of an unarmed one-call frame (one call, but the
           positions depart from the reference's: their distance and that of prune_dx from the exact route's are recorded)
20 clones, 12 in-state features (idp 1), the second- and third-newest clones leave, 10 / 40 / 120 prune tracks, prune_apply_dx = 1.  Every
sample starts from the same resident covariance (cov_set + sync outside the timed region); the routes alternate inside ONE loop;
reported per size and route: median and quartiles over all samples behind the warm-up.  Microseconds.
The exact route's triangulation call checks the motion on the last listed observation (the call has no other form): same work, and a
different decision only for a track whose motion lies between the two figures (valid_differs_from_exact counts them).
--package-root DIR: import orcvio_amd from DIR (another build, e.g. the commit in front of the feature: the armed route is left out
when the library has no orcvio_msckf_io_triangulate_prune).
usage: python scripts/gpu_prune_tri_timing.py [--reps 240] [--warmup 40] [--tag r25a] [--package-root DIR]"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=240)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--tag', default=None)
    ap.add_argument('--package-root', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, ROOT)
    if args.package_root:
        sys.path.insert(0, os.path.abspath(args.package_root))
    from orcvio_amd import capi, synth
    import tri_io_cases as tc

    N, NSLAM, IDP = 20, 12, 1
    remove = [N - 3, N - 2]
    fl = synth.Flags(use_larvio=1)
    w0 = synth.with_extra_states(synth.make_window(N=N, F=900, seed=3, track_len=(2, 20), flags=fl, outlier_frac=0.05), IDP * NSLAM, seed=1)
    slam = synth.make_slam_features(w0, NSLAM, seed=1, outlier_frac=0.1)
    tracked = tc.ends_at_newest(w0)
    sub = synth.subset_tracks(w0, remove, min_obs=2)
    cand = np.flatnonzero(tracked & (np.diff(sub.obs_ptr) >= 2))
    lost = np.flatnonzero(~tracked & (np.diff(w0.obs_ptr) >= 3))[:60]
    mask = lambda idx: np.isin(np.arange(w0.F), idx)
    first = tc.select_tracks(w0, mask(lost))
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096)
    u.set_ekf_rows_mode(True)
    u.set_extra_states(IDP * NSLAM)
    armed_ok = hasattr(u, 'io_triangulate_prune')
    hide = lambda w: dataclasses.replace(w, p_w=np.full_like(w.p_w, np.nan))

    def exact(tri_win, prune):
        io = u.io_begin(first.flags, first.N, first.F, int(first.obs_ptr[-1]), with_P=False)
        u.io_fill(io, first, with_P=False)
        u.make_slam_call(IDP, slam)()
        u.io_update(want_P=False, commit=True)
        inc, _ = capi.increment_window(tri_win, io['dx'].copy())
        tri = u.triangulate(inc)
        keep = tri['valid'] == 1
        p = tc.select_tracks(dataclasses.replace(prune, R_b2w=inc.R_b2w, t_b_w=inc.t_b_w), keep, tri['p_w'])
        io2 = u.io_begin(p.flags, p.N, p.F, int(p.obs_ptr[-1]), with_P=False)
        u.io_fill(io2, p, with_P=False)
        u.io_update(want_P=False, commit=True)
        u.cov_remove_clones(22, remove)
        return dict(valid=tri['valid'], p_w=tri['p_w'], prune_dx=io2['dx'].copy())

    def approx(tri_win, prune):
        tri = u.triangulate(tri_win)
        keep = tri['valid'] == 1
        got = u.io_step_frame(first, None, None, False, slam, IDP, tc.select_tracks(prune, keep, tri['p_w']), True, remove)
        return dict(valid=tri['valid'], p_w=tri['p_w'], prune_dx=got['prune_dx'])

    def armed(tri_win, prune):
        got = u.io_step_frame(first, None, None, False, slam, IDP, hide(prune), True, remove, triangulate_prune=(tri_win, None))
        return dict(valid=got['prune_tri']['valid'], p_w=got['prune_tri']['p_w'], prune_dx=got['prune_dx'])

    routes = dict(exact=exact, approx=approx)
    if armed_ok:
        routes['armed'] = armed
    try:
        from orcvio_amd import build as b
        sha = b.source_sha16()
    except OSError:   # (a package copied without its sources)
        sha = None
    out = dict(build=dict(source_sha16=sha, other_package=bool(args.package_root)), reps=args.reps, warmup=args.warmup,
               unit='us', clones=N, in_state=NSLAM, first_tracks=int(first.F), sizes={})
    for K in (10, 40, 120):
        assert len(cand) >= K, len(cand)
        tri_win, prune = tc.select_tracks(w0, mask(cand[:K])), tc.select_tracks(sub, mask(cand[:K]))
        samples = {k: [] for k in routes}
        last = {}
        for rep in range(args.warmup + args.reps):
            for k, fn in routes.items():   # (the routes alternate: a drift of the machine touches every one alike)
                u.cov_set(w0.P)
                u.sync()
                t0 = time.perf_counter()
                last[k] = fn(tri_win, prune)
                dt = (time.perf_counter() - t0) * 1e6
                u.sync()
                if rep >= args.warmup:
                    samples[k].append(dt)
        row = {k: dict(median=float(np.median(v)), q25=float(np.percentile(v, 25)), q75=float(np.percentile(v, 75)), n=len(v)) for k, v in samples.items()}
        ex = last['exact']
        kx = ex['valid'] == 1
        rel = lambda a, b_: float(np.linalg.norm(a - b_) / max(np.linalg.norm(b_), 1e-300))
        for k in routes:
            if k == 'exact':
                continue
            both = kx & (last[k]['valid'] == 1)
            row[k]['valid_differs_from_exact'] = int((last[k]['valid'] != ex['valid']).sum())
            row[k]['p_w_rel_to_exact'] = rel(last[k]['p_w'][both], ex['p_w'][both])
            row[k]['prune_dx_rel_to_exact'] = rel(last[k]['prune_dx'], ex['prune_dx'])
        row['prune_tracks'] = K; row['valid_exact'] = int(kx.sum()); row['tri_observations'] = int(tri_win.obs_ptr[-1])
        out['sizes'][str(K)] = row
    u.close()
    if args.tag:
        with open(os.path.join(ROOT, 'profiles', f'{args.tag}_prune_tri_timing.json'), 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
