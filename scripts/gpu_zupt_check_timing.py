"""Host-visible time of the zero-velocity DETECTION from IMU samples on the resident covariance (GPU), at 20 clones (n = 142) and
S = 10, 33, 128 selected samples (leg 22):
  a  check         orcvio_msckf_cov_zupt_check_imu alone: one launch (k_zupt_check), one wait
  b  propagate     orcvio_msckf_cov_propagate_imu with wait = 1   against   propagate_checked  orcvio_msckf_cov_propagate_imu_checked
  c  parent        the only route on the parent commit: orcvio_msckf_cov_get of the whole n x n matrix (timed here) plus the reference's
                   dense test on the host -- S = H P_m H^T + R of order 6 (S - 1), factored -- in plain C++ (tests/cpp/test_zupt_check_model.cpp,
                   its `dense` mode, g++ -O2, timed inside the program).  The plain C++ stands in for the reference's Eigen, which
                   this tree does not build: Eigen's blocked llt is faster than these loops at 762 rows, so read c as the PARENT's path
                   on this code base, not as the reference's own time.
  d  stationary frame   armed_checked  io_propagate_imu + cov_zupt_frame_checked (one wait)   against
                        checked_then_frame  cov_propagate_imu_checked + cov_zupt_frame (two waits)
Every sample starts from the same resident covariance (cov_set + sync outside the timed region).  The ways alternate in blocks;
reported per way: median and p95 over all samples and the block medians (their spread is the yardstick for a difference).  Microseconds.
usage: python scripts/gpu_zupt_check_timing.py [--blocks 5] [--reps 40] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from orcvio_amd import capi, synth  # noqa: E402
from orcvio_amd import build as b  # noqa: E402
import imu_cases as ic  # noqa: E402

LEG, N = 22, 20
NOISES = synth.ZUPT_NOISES


def measure(u, ways, setup, blocks, reps):
    samples = {k: [] for k in ways}
    block_med = {k: [] for k in ways}
    for blk in range(blocks + 1):   # (block 0: warm-up of every way's shapes)
        for k, fn in ways.items():
            ts = []
            for _ in range(reps):
                ctx = setup(k)
                u.sync()
                t0 = time.perf_counter()
                fn(ctx)
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


def dense_host(case_state, P, samples, reps):
    """the dense test in plain C++ on the host: median microseconds of `reps` evaluations (timed inside the program)"""
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, 'zupt_check_dense')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_zupt_check_model.cpp')])
    chk = capi.MsckfUpdater.zupt_check()
    vals = [0.0, chk.sigma_w2, chk.sigma_a2, chk.sigma_wb, chk.sigma_ab] + list(case_state['R']) + list(case_state['ba']) + [0.0, 0.0, -9.81]
    vals += [float(P.shape[0])] + list(P.ravel()) + [float(samples.shape[0])] + list(samples.ravel())
    path = os.path.join(tmp, 'case.txt')
    with open(path, 'w') as f:
        f.write(' '.join(repr(float(v)) for v in vals))
    out = subprocess.run([exe, path, 'dense', str(reps)], capture_output=True, text=True, check=True).stdout.split()
    return float(out[0]), float(out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=64, max_observations=1024)
    out = dict(build=dict(source_sha16=b.source_sha16()), blocks=args.blocks, reps=args.reps, unit='us', n=LEG + 6 * N, samples={})
    chk = capi.MsckfUpdater.zupt_check(chi2_multiplier=1e12, max_velocity=1e3)   # (accepts: the stationary frame applies its update)
    rng = np.random.default_rng(5)
    r = 1e-3 * rng.standard_normal(9)
    for S in (10, 33, 128):
        case = ic.make_case('larvio', S, n=LEG + 6 * N, seed=7, rate=ic.rate_for(S))
        P = case['P']                                   # n = 142: the covariance the check and the propagation see
        P_frame = ic.make_cov(LEG + 6 * (N - 1), rng)   # n = 136: a stationary frame augments to 20 clones
        smp = case['samples']

        def fresh():
            return ic.to_capi(case)

        # the propagated state the stand-alone check is given (what the checked call uses inside)
        cfg, st, prev = fresh()
        u.cov_set(P)
        u.cov_propagate_imu(cfg, st, prev, smp, case['time_bound'], wait=True)
        Pp = u.cov_get()
        state = dict(R=np.array(st.R_b2w[:]), v=np.array(st.v[:]), ba=np.array(st.acc_bias[:]))
        g = case['cfg'].gravity

        def setup(k):
            u.cov_set(P_frame if k in ('armed_checked', 'checked_then_frame') else (Pp if k in ('check', 'cov_get') else P))
            return fresh()

        def armed_checked(c):
            u.io_propagate_imu(c[0], c[1], c[2], smp, case['time_bound'])
            u.cov_zupt_frame_checked(chk, LEG, N, r, NOISES, True, True)

        def checked_then_frame(c):
            u.cov_propagate_imu_checked(c[0], c[1], c[2], smp, case['time_bound'], chk)
            u.cov_zupt_frame(LEG, N, r, NOISES, None, None, True, True)

        ways = dict(
            check=lambda c: u.cov_zupt_check_imu(chk, state['R'], state['v'], state['ba'], g, smp),
            propagate=lambda c: u.cov_propagate_imu(c[0], c[1], c[2], smp, case['time_bound'], wait=True),
            propagate_checked=lambda c: u.cov_propagate_imu_checked(c[0], c[1], c[2], smp, case['time_bound'], chk),
            cov_get=lambda c: u.cov_get(),
            armed_checked=armed_checked,
            checked_then_frame=checked_then_frame,
        )
        row = measure(u, ways, setup, args.blocks, args.reps)
        chi2_dense, dense_us = dense_host(state, Pp, smp, max(3, args.reps // 8))
        u.cov_set(Pp)
        got = u.cov_zupt_check_imu(chk, state['R'], state['v'], state['ba'], g, smp)
        row['dense_host_cpp'] = dict(median=dense_us, rows=6 * (S - 1))
        row['parent_route'] = dict(median=row['cov_get']['median'] + dense_us)
        row['chi2'] = dict(device=got['chi2'], dense_host_cpp=chi2_dense, rel=abs(got['chi2'] - chi2_dense) / chi2_dense)
        out['samples'][f'S{S}'] = row
    u.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
