"""Timing of the IMU propagation at leg_dim 46 (GPU): LARVIO closed form, general intrinsics, a 20-clone covariance (n = 166), at
S = 10, 33, 128 selected samples:

  kernel_us          k_imu_phi_q46 alone, HIP events around the launch (diagnostics build: orcvio_msckf_debug_imu_kernel46_ms), median
  imu_host_us        host time of orcvio_msckf_cov_propagate_imu_calib WITHOUT a wait (host half + staging + three launches enqueued)
  imu_total_us       the same call followed by a stream synchronisation: samples in, propagated covariance resident
  parent_host_us     the route without the call, in the same loop: mean and Phi, Q [46][46] on the host (imu_propagate_mean46 +
                     imu_accumulate_host46, tests/cpp/imu_calib_host_route.cpp built with -O3), then orcvio_msckf_cov_propagate(46, Phi, Q)
                     of THIS commit; host time without a wait
  parent_total_us    ... followed by a stream synchronisation
  host_accumulate_us the host arithmetic's share of the parent route

  kernel_model       k_imu_phi_q46 also at S = 4 (one round, one sample a wavefront) and S = 32 (one round, eight samples a wavefront):
                     with S = 128 (four rounds, 32 samples a wavefront) the three medians give, by t = a + rounds * p1 + samples * p2,
                     the cost of one round's phase 1 (p1) and of one sample's phase 2 (p2), and from them phase 1's share at 10, 33, 128.
                     A fit of three points, not a measurement of the phases.

The two routes alternate inside one loop, so both see the same box at the same time; spread = the quartiles of each figure.
usage: python scripts/gpu_imu_calib_timing.py [--reps 400] [--out profiles/NAME.json]"""
import argparse
import ctypes as C
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

from orcvio_amd import capi  # noqa: E402
import imu_cases as ic  # noqa: E402
import imu_calib_cases as icc  # noqa: E402

_dp = C.POINTER(C.c_double)


def stats(x):
    x = np.sort(np.asarray(x, dtype=np.float64))
    return dict(median=float(np.median(x)), q1=float(x[len(x) // 4]), q3=float(x[(3 * len(x)) // 4]))


def host_route_lib():
    so = os.path.join(tempfile.mkdtemp(), 'libimucalibroute.so')
    subprocess.check_call(['g++', '-std=c++17', '-O3', '-fPIC', '-shared', '-o', so, os.path.join(ROOT, 'tests', 'cpp', 'imu_calib_host_route.cpp')])
    lib = C.CDLL(so)
    lib.orc_imu_calib_host_route.argtypes = [_dp, _dp, C.c_double, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp, _dp]
    lib.orc_imu_calib_host_route.restype = C.c_int
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=400)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    u = capi.MsckfUpdater(device=0, max_clones=20, max_features=16, max_observations=256, debug_hooks=True)
    u.lib.orcvio_msckf_debug_imu_kernel46_ms.argtypes = [C.c_void_p, C.POINTER(capi.ImuConfig), C.POINTER(capi.ImuIntrinsics), C.POINTER(capi.ImuState),
                                                         capi._dp, capi._dp, C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_float)]
    route = host_route_lib()
    d = lambda a: a.ctypes.data_as(_dp)

    def kernel_us(case):
        smp = np.ascontiguousarray(case['samples'])
        cfg, xi, state, prev = icc.to_capi(case)
        ms = (C.c_float * args.reps)()
        rc = u.lib.orcvio_msckf_debug_imu_kernel46_ms(u.h, C.byref(cfg), C.byref(xi), C.byref(state), capi._d(prev), capi._d(smp), smp.shape[0],
                                                      float(case['time_bound']), args.reps, ms)
        assert rc == 0, rc
        return stats(np.array(ms[:]) * 1e3)

    out = {}
    kern = {}
    for S in (10, 33, 128):
        case = icc.make_case('larvio', S, intr='general', n=166, seed=31, rate=ic.rate_for(S))
        c, st, fej = case['cfg'], case['state'], case['fej']
        smp = np.ascontiguousarray(case['samples'])
        u.cov_set(case['P'])
        kern[S] = kernel_us(case)
        flags = np.array([c.use_larvio, c.use_left, c.use_closed_form, c.if_fej], dtype=np.float64)
        grav = np.ascontiguousarray(c.gravity, dtype=np.float64)
        Qc = np.ascontiguousarray(np.diag(c.Qc))
        x = np.ascontiguousarray(case['intr'])
        st0 = np.concatenate([[st.time], st.R.ravel(), st.v, st.p, st.bg, st.ba, fej.v, fej.p]).astype(np.float64)
        Phi, Q = np.zeros((46, 46)), np.zeros((46, 46))
        t = dict(imu_host=[], imu_total=[], parent_host=[], parent_total=[], host_accumulate=[])
        last = {}
        for r in range(args.reps + 20):
            u.cov_set(case['P'])
            cfg, xi, state, prev = icc.to_capi(case)
            t0 = time.perf_counter()
            u.cov_propagate_imu_calib(cfg, xi, state, prev, smp, case['time_bound'])
            t1 = time.perf_counter()
            u.sync()
            t2 = time.perf_counter()
            last['call'] = u.cov_get() if r == 0 else last['call']
            u.cov_set(case['P'])
            sv, pv = st0.copy(), case['prev'].copy()
            t3 = time.perf_counter()
            n_prop = route.orc_imu_calib_host_route(d(flags), d(grav), float(c.imu_img_time_th), d(Qc), d(x), d(sv), d(pv), d(smp), smp.shape[0],
                                                    float(case['time_bound']), d(Phi), d(Q))
            t4 = time.perf_counter()
            u.cov_propagate(Phi, Q)
            t5 = time.perf_counter()
            u.sync()
            t6 = time.perf_counter()
            last['route'] = u.cov_get() if r == 0 else last['route']
            assert n_prop == S
            if r >= 20:   # (warm-up: the first launches load code objects)
                t['imu_host'].append((t1 - t0) * 1e6); t['imu_total'].append((t2 - t0) * 1e6)
                t['parent_host'].append((t5 - t3) * 1e6); t['parent_total'].append((t6 - t3) * 1e6)
                t['host_accumulate'].append((t4 - t3) * 1e6)
        rel = float(np.linalg.norm(last['call'] - last['route']) / np.linalg.norm(last['route']))
        assert rel < 1e-12, rel   # (the two routes propagate the same covariance)
        out['S=%d' % S] = dict(kernel_us=kern[S], routes_agree_rel_fro=rel, **{k + '_us': stats(v) for k, v in t.items()})
        print('S=%d' % S, json.dumps(out['S=%d' % S]))
    for S in (4, 32):
        case = icc.make_case('larvio', S, intr='general', n=166, seed=31, rate=ic.rate_for(S))
        u.cov_set(case['P'])
        kern[S] = kernel_us(case)
    t4_, t32, t128 = kern[4]['median'], kern[32]['median'], kern[128]['median']
    p2 = (t32 - t4_) / 7.0
    p1 = (t128 - t32 - 24.0 * p2) / 3.0
    model = dict(kernel_us_S4=kern[4], kernel_us_S32=kern[32], round_phase1_us=p1, sample_phase2_us=p2, phase1_share={})
    for S in (10, 33, 128):
        Cw = (S + 3) // 4
        model['phase1_share']['S=%d' % S] = ((Cw + 7) // 8) * p1 / kern[S]['median']
    out['kernel_model'] = model
    print('kernel_model', json.dumps(model))
    u.close()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
