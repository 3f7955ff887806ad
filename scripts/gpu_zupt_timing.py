"""Host-visible time of one STATIONARY frame on the resident covariance (GPU), three ways:
  frame   orcvio_msckf_cov_zupt_frame: propagate, augment, the zero-velocity update, the previous clone marginalised -- one call, one wait
  calls   the four separate calls: cov_propagate, cov_augment, cov_zupt, cov_remove_clones
  host    what a caller had to do before cov_zupt existed: cov_propagate, cov_augment, cov_get, the reference's update on the CPU (here a
          fixed-cost numpy solve of the same sizes: the 9 x 9 solve, K H P, the symmetrisation), cov_set, cov_remove_clones
at N = 20 and N = 30 clones behind the augmentation (leg 22), and the first MOVING frame behind a stationary one (io_step_frame),
with the factor the stationary frame kept and without one, with and without the moving frame's own propagation (which drops any factor).
Every sample starts from the same resident covariance (cov_set + sync outside the timed region); the timed region is the call(s) up to
their return (the marginalisation is enqueued in every way and synchronised outside).  The ways alternate in blocks; reported per way:
median and p95 over all samples and the block medians (their spread is the yardstick for a difference).  Microseconds.
usage: python scripts/gpu_zupt_timing.py [--blocks 5] [--reps 40] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orcvio_amd import capi, synth  # noqa: E402
from orcvio_amd import build as b  # noqa: E402

LEG = 22
NOISES = synth.ZUPT_NOISES


def host_update(P, N, r):
    """the sizes of measurementUpdate_ZUPT_vpq's arithmetic (src/orcvio.cpp:3374-3447) with the sparsity of H used: fixed cost"""
    bb = LEG + 6 * N
    HP = np.concatenate([P[3:6], P[bb - 3:bb] - P[bb - 9:bb - 6], 0.5 * (P[bb - 12:bb - 9] - P[bb - 6:bb - 3])])
    S = np.concatenate([HP[:, 3:6], HP[:, bb - 3:bb] - HP[:, bb - 9:bb - 6], 0.5 * (HP[:, bb - 12:bb - 9] - HP[:, bb - 6:bb - 3])], axis=1)
    S[np.arange(9), np.arange(9)] += np.repeat(NOISES, 3)
    Kt = np.linalg.solve(S, HP)
    dx = Kt.T @ r
    Pn = P - Kt.T @ HP
    return dx, 0.5 * (Pn + Pn.T)


def spd(n, seed):
    g = np.random.default_rng(seed)
    A = g.standard_normal((n, n)) / np.sqrt(n)
    P = 1e-3 * (A @ A.T) + np.diag(g.uniform(1e-4, 1e-2, n))
    return 0.5 * (P + P.T)


def way_frame(u, c):
    u.cov_zupt_frame(LEG, c['N'], c['r'], NOISES, c['Phi'], c['Q'], True, True)


def way_calls(u, c):
    u.cov_propagate(c['Phi'], c['Q'])
    u.cov_augment()
    u.cov_zupt(LEG, c['N'], c['r'], NOISES)
    u.cov_remove_clones(LEG, [c['N'] - 2])


def way_host(u, c):
    u.cov_propagate(c['Phi'], c['Q'])
    u.cov_augment()
    P = u.cov_get()
    _, Pn = host_update(P, c['N'], c['r'])
    u.cov_set(Pn)
    u.cov_remove_clones(LEG, [c['N'] - 2])


def measure(u, ways, setup, blocks, reps):
    samples = {k: [] for k in ways}
    block_med = {k: [] for k in ways}
    for blk in range(blocks + 1):   # (block 0: warm-up of every way's shapes)
        for k, fn in ways.items():
            ts = []
            for _ in range(reps):
                setup(k)
                u.sync()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e6)
                u.sync()
            if blk > 0:
                samples[k] += ts
                block_med[k].append(float(np.median(ts)))
    row = {}
    for k in ways:
        a = np.sort(samples[k])
        row[k] = dict(median=float(np.median(a)), p95=float(a[int(0.95 * (len(a) - 1))]), block_medians=block_med[k])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    fl = synth.Flags(use_larvio=1)
    rng = np.random.default_rng(3)
    u = capi.MsckfUpdater(device=0, max_clones=32, max_features=256, max_observations=4096)
    out = dict(build=dict(source_sha16=b.source_sha16()), blocks=args.blocks, reps=args.reps, unit='us', tile_update='fma', stationary={}, moving_after={})
    for N in (20, 30):
        P = spd(LEG + 6 * (N - 1), N)
        G = rng.standard_normal((LEG, 12))
        c = dict(N=N, r=1e-3 * rng.standard_normal(9), Phi=np.ascontiguousarray(np.eye(LEG) + 1e-5 * rng.standard_normal((LEG, LEG))),
                 Q=np.ascontiguousarray(1e-10 * G @ G.T))
        ways = dict(frame=lambda: way_frame(u, c), calls=lambda: way_calls(u, c), host=lambda: way_host(u, c))
        row = measure(u, ways, lambda k: u.cov_set(P), args.blocks, args.reps)
        row['n'] = LEG + 6 * N
        out['stationary'][f'N{N}'] = row
    # the first moving frame behind a stationary one (N = 20): the stationary frame WITHOUT propagation, so that a factor can survive it
    N = 20
    P = spd(LEG + 6 * (N - 1), 77)
    r = 1e-3 * rng.standard_normal(9)
    w = synth.make_window(N=N, F=60, seed=9, track_len=(3, 6), flags=fl, outlier_frac=0.05)
    G = rng.standard_normal((LEG, 12))
    Phi, Q = np.ascontiguousarray(np.eye(LEG) + 0.002 * rng.standard_normal((LEG, LEG))), np.ascontiguousarray(1e-7 * G @ G.T)

    def setup(k):
        u.cov_set(P)
        if k.startswith('kept'):
            u.cov_prefactor()
            u.cov_zupt_frame(LEG, N, r, NOISES, None, None, True, True)
        else:   # the host way leaves no factor (cov_set drops it)
            u.cov_augment()
            Pa = u.cov_get()
            u.cov_set(host_update(Pa, N, r)[1])
            u.cov_remove_clones(LEG, [N - 2])

    ways = {
        'kept_factor_no_propagation': lambda: u.io_step_frame(w, None, None, True),
        'no_factor_no_propagation': lambda: u.io_step_frame(w, None, None, True),
        'kept_factor_propagated': lambda: u.io_step_frame(w, Phi, Q, True),
        'no_factor_propagated': lambda: u.io_step_frame(w, Phi, Q, True),
    }
    out['moving_after'] = measure(u, ways, setup, args.blocks, args.reps)
    u.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
