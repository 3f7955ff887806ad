"""Timing of the IMU propagation from raw samples (GPU), at S = 10, 33, 128 selected samples on a 20-clone covariance (n = 142):

  kernel_us          k_imu_phi_q alone, HIP events around the launch (diagnostics build: orcvio_msckf_debug_imu_kernel_ms), median
  imu_host_us        host time of orcvio_msckf_cov_propagate_imu WITHOUT a wait (host half + staging + three launches enqueued), median
  imu_total_us       the same call followed by a stream synchronisation: samples in, propagated covariance resident
  parent_host_us     orcvio_msckf_cov_propagate with Phi, Q given (what the parent commit offers), host time without a wait
  parent_total_us    ... followed by a stream synchronisation
  host_accumulate_us what the caller has to do in front of the parent's call: the mean propagation and the accumulation of Phi, Q on
                     the host, by the stand-alone program tests/cpp/imu_model_main.cpp built with -O3 (median of its own repetitions)

  frames             the config-1 stream (synth.make_stream, LARVIO flags): every frame through orcvio_msckf_io_step_frame, on one handle ARMED
                     (orcvio_msckf_io_propagate_imu + the frame call given Phi = Q = NULL; the arming call's host time is part of the frame's)
                     and on another GIVEN Phi_out / Q_out of the same samples (the parent's frame); median per frame over the loop, us,
                     for S = 10 and S = 33 samples per frame

The two paths alternate inside one loop, so both see the same box at the same time; spread = the interquartile range of each figure.
usage: python scripts/gpu_imu_propagate_timing.py [--reps 400] [--out profiles/NAME.json]"""
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
import mirror_imu as mi  # noqa: E402


def stats(x):
    x = np.sort(np.asarray(x, dtype=np.float64))
    return dict(median=float(np.median(x)), q1=float(x[len(x) // 4]), q3=float(x[(3 * len(x)) // 4]))


def frames_leg(reps):
    from orcvio_amd import synth
    fl = synth.Flags(use_larvio=1)
    frames, P0 = synth.make_stream(fl)
    aux = capi.MsckfUpdater(device=0, max_clones=2, max_features=16, max_observations=256)
    res = {}
    for S in (10, 33):
        case = ic.make_case('larvio', S, n=22, seed=33, rate=ic.rate_for(S))
        smp = np.ascontiguousarray(case['samples'])
        cfg, state, prev = ic.to_capi(case)
        aux.cov_set(np.eye(22))
        pq = aux.cov_propagate_imu(cfg, state, prev, smp, case['time_bound'], want_PhiQ=True)
        hs = []
        for _ in range(2):
            h = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096)
            h.set_extra_states(12)
            h.set_ekf_rows_mode(True)
            h.cov_set(P0)
            hs.append(h)
        t = dict(armed=[], given=[])
        n_frames = max(reps // 2, 2 * len(frames))
        for it in range(n_frames + 2 * len(frames)):
            fr = frames[it % len(frames)]
            cfg, state, prev = ic.to_capi(case)
            t0 = time.perf_counter()
            hs[0].io_propagate_imu(cfg, state, prev, smp, case['time_bound'])
            hs[0].io_step_frame(fr['w'], None, None, True, fr['slam'], 1, fr['prune'], False, fr['remove'])
            t1 = time.perf_counter()
            hs[1].io_step_frame(fr['w'], pq['Phi'], pq['Q'], True, fr['slam'], 1, fr['prune'], False, fr['remove'])
            t2 = time.perf_counter()
            if it >= 2 * len(frames):   # (two cycles of warm-up)
                t['armed'].append((t1 - t0) * 1e6); t['given'].append((t2 - t1) * 1e6)
        assert np.array_equal(hs[0].cov_get(), hs[1].cov_get())   # (the two handles ran the same filter, bit for bit)
        for h in hs:
            h.close()
        res['S=%d' % S] = dict(armed_us=stats(t['armed']), given_us=stats(t['given']), frames=len(t['armed']))
    aux.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=400)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    u = capi.MsckfUpdater(device=0, max_clones=20, max_features=16, max_observations=256, debug_hooks=True)
    u.lib.orcvio_msckf_debug_imu_kernel_ms.argtypes = [C.c_void_p, C.POINTER(capi.ImuConfig), C.POINTER(capi.ImuState), capi._dp, capi._dp, C.c_int32,
                                                       C.c_double, C.c_int32, C.POINTER(C.c_float)]
    exe = os.path.join(tempfile.mkdtemp(), 'imu_model_main')
    subprocess.check_call(['g++', '-std=c++17', '-O3', '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'imu_model_main.cpp')])
    out = {}
    for S in (10, 33, 128):
        case = ic.make_case('larvio', S, n=142, seed=31, rate=ic.rate_for(S))
        srv, _ = ic.run_mirror(case, with_P=False)
        Phi, Q = mi.accumulate_sequential(srv.steps)
        Q = 0.5 * (Q + Q.T)
        smp = np.ascontiguousarray(case['samples'])
        cfg, state, prev = ic.to_capi(case)
        ms = (C.c_float * args.reps)()
        rc = u.lib.orcvio_msckf_debug_imu_kernel_ms(u.h, C.byref(cfg), C.byref(state), capi._d(prev), capi._d(smp), smp.shape[0],
                                                    float(case['time_bound']), args.reps, ms)
        assert rc == 0, rc
        kernel = stats(np.array(ms[:]) * 1e3)
        t = dict(imu_host=[], imu_total=[], parent_host=[], parent_total=[])
        for r in range(args.reps + 20):
            u.cov_set(case['P'])
            cfg, state, prev = ic.to_capi(case)
            t0 = time.perf_counter()
            u.cov_propagate_imu(cfg, state, prev, smp, case['time_bound'])
            t1 = time.perf_counter()
            u.sync()
            t2 = time.perf_counter()
            u.cov_set(case['P'])
            t3 = time.perf_counter()
            u.cov_propagate(Phi, Q)
            t4 = time.perf_counter()
            u.sync()
            t5 = time.perf_counter()
            if r >= 20:   # (warm-up: the first launches load code objects)
                t['imu_host'].append((t1 - t0) * 1e6); t['imu_total'].append((t2 - t0) * 1e6)
                t['parent_host'].append((t4 - t3) * 1e6); t['parent_total'].append((t5 - t3) * 1e6)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, 'case.txt')
            ic.write_case(path, case)
            line = subprocess.run([exe, path, '2000'], capture_output=True, text=True, check=True).stdout.split()
        out['S=%d' % S] = dict(kernel_us=kernel, host_accumulate_us=float(line[1]) * 1e-3, **{k + '_us': stats(v) for k, v in t.items()})
        print('S=%d' % S, json.dumps(out['S=%d' % S]))
    u.close()
    out['frames'] = frames_leg(args.reps)
    print('frames', json.dumps(out['frames']))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
