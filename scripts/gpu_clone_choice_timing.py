"""Host-visible time of a prune frame whose choice of the clones that leave is checked on the device (orcvio_msckf_io_choose_clones
inside orcvio_msckf_io_step_frame, GPU), at euroc.yaml's operating point -- 20 clones, 40 lost tracks in the first update, the prune
tracks that follow from the remove set (tests/clone_choice_cases.py, cases n20_10_agree / n20_10_differ):
  unarmed   (a) the one-call frame as it was: remove_clones taken from the caller, unchecked
  agree     (b) the armed frame whose prediction holds
  differ    (c) the armed frame whose prediction does not hold, the host increment of the window, and the second half re-issued with
            the device's choice as a second frame
  exact     (d) the only exact route without the call: the first half as a frame, the host increment, findRedundantImuStates on the
            host, the second half as a second frame
The choice on the host itself is NOT in (d)'s time (a few dozen flops in C++; the numpy mirror here would charge it a hundred
microseconds): its outcome is taken from the case.  The Python binding's own overhead is in every route alike.  Every sample starts from
the same resident covariance (cov_set + sync outside the timed region); the routes alternate inside ONE loop; reported per route: median
and quartiles over all samples behind the warm-up, and the run-to-run spread as the median's distance between the two halves of the
samples.  Microseconds.
--package-root DIR: import orcvio_amd from DIR (a build of the commit in front of the feature: routes (a) and (d) only).
usage: python scripts/gpu_clone_choice_timing.py [--reps 400] [--warmup 50] [--tag r26a] [--package-root DIR]"""
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
    ap.add_argument('--reps', type=int, default=400)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--tag', default=None)
    ap.add_argument('--package-root', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, ROOT)
    if args.package_root:
        sys.path.insert(0, os.path.abspath(args.package_root))
    from orcvio_amd import capi
    import clone_choice_cases as cc
    import tri_io_cases as tc

    ca, cd = cc.case('n20_10_agree'), cc.case('n20_10_differ')
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096)
    armed_ok = hasattr(u, 'io_choose_clones')

    def parts(c):
        pred, truth = cc.prune_for(c, c['predicted']), cc.prune_for(c, c['truth'])
        return dict(c=c, first=c['first'], pred=pred, truth=truth, none=tc.select_tracks(truth, np.zeros(truth.F, bool)), kw=cc.choose_kwargs(c))
    A, D = parts(ca), parts(cd)

    def second_half(p, dx):
        inc, _ = capi.increment_window(p['truth'], dx)
        none = dataclasses.replace(p['none'], R_b2w=inc.R_b2w, t_b_w=inc.t_b_w)
        return u.io_step_frame(none, None, None, False, None, 1, inc, 0, p['c']['truth'])

    def unarmed():
        return u.io_step_frame(A['first'], None, None, False, None, 1, A['pred'], 1, A['c']['predicted'])

    def agree():
        got = u.io_step_frame(A['first'], None, None, False, None, 1, A['pred'], 1, A['c']['predicted'], choose_clones=A['kw'])
        assert got['choice']['agree'] == 1
        return got

    def differ():
        got = u.io_step_frame(D['first'], None, None, False, None, 1, D['pred'], 1, D['c']['predicted'], choose_clones=D['kw'])
        assert got['choice']['agree'] == 0 and got['choice']['chosen'] == D['c']['truth']
        return second_half(D, got['dx'])

    def exact():
        got = u.io_step_frame(A['first'], None, None, False, None, 1, None, 0, [])
        return second_half(A, got['dx'])

    routes = dict(unarmed=unarmed, exact=exact)
    if armed_ok:
        routes.update(agree=agree, differ=differ)
    try:
        from orcvio_amd import build as b
        sha = b.source_sha16()
    except OSError:
        sha = None
    samples = {k: [] for k in routes}
    for rep in range(args.warmup + args.reps):
        for k, fn in routes.items():   # (the routes alternate: a drift of the machine touches every one alike)
            u.cov_set((D if k == 'differ' else A)['c']['w'].P)
            u.sync()
            t0 = time.perf_counter()
            got = fn()
            dt = (time.perf_counter() - t0) * 1e6
            u.sync()
            assert got['rc'] == 0 and got['prune_stats'][3] == 1
            if rep >= args.warmup:
                samples[k].append(dt)

    def row(v):
        h = len(v) // 2
        return dict(median=float(np.median(v)), q25=float(np.percentile(v, 25)), q75=float(np.percentile(v, 75)), n=len(v),
                    halves=[float(np.median(v[:h])), float(np.median(v[h:]))], spread=float(abs(np.median(v[:h]) - np.median(v[h:]))))
    out = dict(build=dict(source_sha16=sha, other_package=bool(args.package_root)), reps=args.reps, warmup=args.warmup, unit='us', clones=20,
               first_tracks=int(A['first'].F), prune_tracks=dict(agree=int(A['pred'].F), differ_predicted=int(D['pred'].F), differ_chosen=int(D['truth'].F)),
               routes={k: row(v) for k, v in samples.items()})
    u.close()
    if args.tag:
        name = f'{args.tag}_clone_choice_timing{"_parent" if args.package_root else ""}.json'
        with open(os.path.join(ROOT, 'profiles', name), 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
