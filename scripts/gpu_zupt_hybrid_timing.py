"""Host-visible time of one STATIONARY frame of a HYBRID filter on the resident covariance (GPU): every in-state feature leaves in front
of the zero-velocity update, the previous clone behind it.
  unchecked  fused      orcvio_msckf_cov_zupt_frame_hybrid: propagate, augment, ONE launch for drop + update + marginalisation; one wait
             calls      the five separate calls: cov_propagate, cov_augment, cov_remove_features (every slot), cov_zupt (the wait),
                        cov_remove_clones
  checked    fused      orcvio_msckf_io_propagate_imu + orcvio_msckf_cov_zupt_frame_checked_hybrid: one wait, nothing enqueued behind it
             calls      orcvio_msckf_cov_propagate_imu_checked (one wait) and, on acceptance, cov_augment, cov_remove_features, cov_zupt
                        (a second wait), cov_remove_clones
at (leg 22, N = 20 behind the augmentation, idp_dim d, F feature states) = (22, 20, 1, 12) and (22, 20, 3, 30).  Every sample starts from
the same resident covariance (cov_set + sync outside the timed region); the timed region is the call(s) up to their return (a
marginalisation that is only enqueued is synchronised outside).  The ways alternate in blocks; reported per way: median and p95 over
all samples and the block medians (their spread is the yardstick for a difference).  Microseconds.
usage: python scripts/gpu_zupt_hybrid_timing.py [--blocks 5] [--reps 40] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from orcvio_amd import capi, synth  # noqa: E402
from orcvio_amd import build as b  # noqa: E402
from gpu_zupt_timing import measure, spd  # noqa: E402
import imu_cases as ic  # noqa: E402   (the IMU sample sets of the test-suite: a state, ten samples at 200 Hz)

LEG = 22
NOISES = synth.ZUPT_NOISES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(3)
    u = capi.MsckfUpdater(device=0, max_clones=40, max_features=256, max_observations=4096)
    out = dict(build=dict(source_sha16=b.source_sha16()), blocks=args.blocks, reps=args.reps, unit='us', unchecked={}, checked={})
    case = ic.make_case('larvio', 10, n=LEG, seed=72, rate=200.0)
    chk = capi.MsckfUpdater.zupt_check(use_left=int(case['cfg'].use_left), chi2_multiplier=1e12, max_velocity=1e3)   # (always accepted)
    for N, d, F in ((20, 1, 12), (20, 3, 30)):
        n0 = LEG + 6 * (N - 1) + d * F
        P = spd(n0, N + F)
        G = rng.standard_normal((LEG, 12))
        r = 1e-3 * rng.standard_normal(9)
        Phi = np.ascontiguousarray(np.eye(LEG) + 1e-5 * rng.standard_normal((LEG, LEG)))
        Q = np.ascontiguousarray(1e-10 * G @ G.T)
        slots = list(range(F))

        def setup(_k):
            u.set_extra_states(d * F)
            u.cov_set(P)

        def fused():
            got = u.cov_zupt_frame_hybrid(LEG, N, r, NOISES, d, F, Phi, Q, True, True)
            u.set_extra_states(0)   # (what the caller owes behind applied = 1: inside the timed region in both routes)
            assert got['applied'] == 1

        def calls():
            u.cov_propagate(Phi, Q)
            u.cov_augment()
            u.cov_remove_features(LEG, N, d, F, slots)
            u.set_extra_states(0)
            assert u.cov_zupt(LEG, N, r, NOISES)['applied'] == 1
            u.cov_remove_clones(LEG, [N - 2])

        def fused_checked():
            cfg, st, prev = ic.to_capi(case)
            u.io_propagate_imu(cfg, st, prev, case['samples'], case['time_bound'])
            got, v = u.cov_zupt_frame_checked_hybrid(chk, LEG, N, r, NOISES, d, F, True, True)
            u.set_extra_states(0)
            assert got['applied'] == 1 and v['accept'] == 1

        def calls_checked():
            cfg, st, prev = ic.to_capi(case)
            _, v = u.cov_propagate_imu_checked(cfg, st, prev, case['samples'], case['time_bound'], chk)
            assert v['accept'] == 1
            u.cov_augment()
            u.cov_remove_features(LEG, N, d, F, slots)
            u.set_extra_states(0)
            assert u.cov_zupt(LEG, N, r, NOISES)['applied'] == 1
            u.cov_remove_clones(LEG, [N - 2])

        key = f'N{N}_d{d}_F{F}'
        row = measure(u, dict(fused=fused, calls=calls), setup, args.blocks, args.reps)
        row['n'], row['b'] = n0 + 6, LEG + 6 * N
        out['unchecked'][key] = row
        row = measure(u, dict(fused=fused_checked, calls=calls_checked), setup, args.blocks, args.reps)
        row['n'], row['b'] = n0 + 6, LEG + 6 * N
        out['checked'][key] = row
    u.set_extra_states(0)
    u.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
