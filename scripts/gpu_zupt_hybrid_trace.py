"""The hybrid stationary frame's fused update with a resident factor, repeated, for `rocprofv3 --kernel-trace --stats` (GPU): device-side
durations of k_zupt_cov_keep and k_zupt_fac_keep at (leg 22, N clones, idp_dim d, F feature states).  Every repetition starts from the
same covariance and factor (cov_set + cov_prefactor) and runs the update alone (no propagation, no augmentation), the previous clone
marginalised in the same launch.
usage: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python scripts/gpu_zupt_hybrid_trace.py --clones 20 --idp 1 --features 12 [--reps 200]"""
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
    ap.add_argument('--idp', type=int, default=1)
    ap.add_argument('--features', type=int, default=12)
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    N, d, F = args.clones, args.idp, args.features
    k = max(0, -(-(LEG + 6 * N + d * F - 224) // 6))   # beyond cov_prefactor's 224 states: factor k clones fewer, then cov_augment k times
    n = LEG + 6 * (N - k) + d * F
    g = np.random.default_rng(N)
    A = g.standard_normal((n, n)) / np.sqrt(n)
    P = 1e-3 * (A @ A.T) + np.diag(g.uniform(1e-4, 1e-2, n))
    P = 0.5 * (P + P.T)
    r = 1e-3 * g.standard_normal(9)
    u = capi.MsckfUpdater(device=0, max_clones=40, max_features=256, max_observations=4096)
    u.set_extra_states(d * F)
    for _ in range(args.reps):
        u.cov_set(P)
        u.cov_prefactor()
        for _k in range(k):
            u.cov_augment()
        assert u.cov_zupt_frame_hybrid(LEG, N, r, synth.ZUPT_NOISES, d, F, None, None, False, True)['applied'] == 1
    u.set_extra_states(0)
    u.close()
    print('done', n)


if __name__ == '__main__':
    main()
