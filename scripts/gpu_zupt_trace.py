"""The zero-velocity update with a resident factor, repeated, for `rocprofv3 --kernel-trace --stats` (GPU): device-side durations of
k_zupt_cov and k_zupt_fac at one window size.  Every repetition starts from the same covariance and factor (cov_set + cov_prefactor).
usage: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python scripts/gpu_zupt_trace.py --clones 20 [--reps 200]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orcvio_amd import capi, synth  # noqa: E402

LEG = 22


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clones', type=int, default=20)
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    N, n = args.clones, LEG + 6 * args.clones
    g = np.random.default_rng(N)
    A = g.standard_normal((n, n)) / np.sqrt(n)
    P = 1e-3 * (A @ A.T) + np.diag(g.uniform(1e-4, 1e-2, n))
    P = 0.5 * (P + P.T)
    r = 1e-3 * g.standard_normal(9)
    u = capi.MsckfUpdater(device=0, max_clones=32, max_features=256, max_observations=4096)
    for _ in range(args.reps):
        u.cov_set(P)
        u.cov_prefactor()
        assert u.cov_zupt(LEG, N, r, synth.ZUPT_NOISES)['applied'] == 1
    u.close()
    print('done', n)


if __name__ == '__main__':
    main()
