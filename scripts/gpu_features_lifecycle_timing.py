"""Host-visible time of the in-state feature lifecycle on the resident covariance (GPU): an anchor change of k features and the
removal of lost features through orcvio_msckf_cov_change_anchors / _cov_remove_features, against the fall-back they replace --
cov_get, the same edit in numpy, cov_set and the Cholesky of the prior that cov_set forces on the next update (cov_prefactor).
Median and p95 over the repetitions, milliseconds; one JSON line on stdout.
usage: python scripts/gpu_features_lifecycle_timing.py [--reps 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from orcvio_amd import capi, synth  # noqa: E402
import lifecycle_cases as lc  # noqa: E402
import mirror_features_lifecycle as mfl  # noqa: E402


def stats(ts):
    a = np.sort(np.asarray(ts) * 1e3)
    return dict(median_ms=float(np.median(a)), p95_ms=float(a[int(0.95 * (len(a) - 1))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    leg, N, d, nf = 22, 20, 1, 20
    w, poses = lc.window(N, 1)
    R_b2c, t_c_b = lc.extrinsics(w)
    n = leg + 6 * N + d * nf
    P0 = lc.spd(n, 2)
    flags = synth.Flags(leg_dim=leg)
    upd = capi.MsckfUpdater(device=0, max_clones=40, max_features=512, max_observations=16384)
    out = dict(n=n, clones=N, idp_dim=d, features=nf)
    for k in (1, 4, 16):
        ch = lc.changes(poses, N, nf, k, seed=k)
        dev, host = [], []
        for r in range(args.reps + 10):
            upd.cov_set(P0)
            upd.cov_prefactor()
            upd.sync()
            t0 = time.perf_counter()
            upd.cov_change_anchors(flags, d, poses, R_b2c, t_c_b, ch)
            t1 = time.perf_counter()
            P = upd.cov_get()
            P = mfl.change_anchors(P, leg, N, d, poses, R_b2c, t_c_b, ch)[0]
            upd.cov_set(P)
            upd.cov_prefactor()
            upd.sync()
            t2 = time.perf_counter()
            if r >= 10:
                dev.append(t1 - t0)
                host.append(t2 - t1)
        out[f'change_anchors_k{k}'] = dict(device=stats(dev), fallback=stats(host))
    dev, host = [], []
    for r in range(args.reps + 10):
        upd.cov_set(P0)
        upd.cov_prefactor()
        upd.sync()
        t0 = time.perf_counter()
        upd.cov_remove_features(leg, N, d, nf, [2, 7])
        upd.sync()
        t1 = time.perf_counter()
        upd.cov_set(P0)
        upd.cov_prefactor()
        upd.sync()
        t2 = time.perf_counter()
        P = upd.cov_get()
        P = mfl.rm_lost_features_cov(P, leg, N, d, [2, 7])
        upd.cov_set(P)
        upd.cov_prefactor()
        upd.sync()
        t3 = time.perf_counter()
        if r >= 10:
            dev.append(t1 - t0)
            host.append(t3 - t2)
    out['remove_features_2'] = dict(device=stats(dev), fallback=stats(host))
    upd.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
