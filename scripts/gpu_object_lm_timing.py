"""Host-visible time of orcvio_msckf_object_lm (GPU), through ctypes, median and p95 over --reps calls (default 200), microseconds:
  synth_1     one object,  F = 30, K = 12 (synth.make_objects on a 30-clone window, the start its noisy state, the priors the car means)
  synth_20    twenty such objects in one call
  one_car     the reference's 47-frame track from the 1.1 m start (tests/object_lm_cases.py)
  lm_update   synth_20's LM followed by orcvio_msckf_update_object_tracks on its result: two calls
and, with --trace N, nothing but N calls of each of the first three workloads in turn, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python scripts/gpu_object_lm_timing.py --trace 50); --kernel-stats CSV then merges the traced
device time of k_object_lm per launch, and per iteration with the iteration counts the calls reported, into the record.
There is NO baseline here: the reference's Eigen optimiser cannot be built in this tree and the numpy mirror is a checker, not an
implementation anyone would time.  The numbers say what the call costs, not what it saves.
usage: python scripts/gpu_object_lm_timing.py [--reps 200] [--out FILE] [--trace N] [--kernel-stats CSV]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from orcvio_amd import capi, synth  # noqa: E402
from orcvio_amd import build as b  # noqa: E402
import object_lm_cases as oc  # noqa: E402

W = (1.0, 1.0, 1.0, 1.0)


def timed(fn, reps, sync):
    for _ in range(10):
        fn()
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    a = np.sort(ts)
    return dict(median=float(np.median(a)), p95=float(a[int(0.95 * (len(a) - 1))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', type=int, default=0)
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    flags = synth.Flags(use_larvio=0, use_left_perturbation=0)
    win = synth.make_window(N=30, F=2, seed=4, flags=flags, track_len=3)
    objs = synth.make_objects(win, n_objects=20, seed=4)
    ms = [synth.CAR_MEAN_SHAPE] * 20
    mk = [synth.CAR_KEYPOINTS_MEAN] * 20
    car, car_ms, car_mk = oc.one_car(47, 0, 0)
    u = capi.MsckfUpdater(device=0, max_clones=32, max_features=64, max_observations=1024)
    work = {
        'synth_1': lambda: u.object_lm(objs[:1], ms[:1], mk[:1], True, 0, W),
        'synth_20': lambda: u.object_lm(objs, ms, mk, True, 0, W),
        'one_car': lambda: u.object_lm([car], [car_ms], [car_mk], True, 0, oc.WEIGHTS_REF),
    }
    out = dict(build=dict(source_sha16=b.source_sha16()), unit='us', reps=args.reps, shape=dict(F=30, K=12),
               baseline='none: the reference optimiser is not built here, the numpy mirror is a checker', workloads={})
    for k, fn in work.items():
        st = fn()[1]
        out['workloads'][k] = dict(objects=len(st), status=[s['status'] for s in st], iterations=[s['iterations'] for s in st],
                                   evaluations=[s['evaluations'] for s in st])
    if args.trace:
        for k, fn in work.items():
            for _ in range(args.trace):
                fn()
        out['traced_calls_per_workload'] = args.trace
    else:
        for k, fn in work.items():
            out['workloads'][k]['host_visible'] = timed(fn, args.reps, u.sync)

        def lm_update():
            tracks, _ = u.object_lm(objs, ms, mk, True, 0, W)
            u.update_object_tracks(flags, win.N, tracks, win.P, win.R_b2c[0], win.t_c_b[0], True, False, 0)
        out['workloads']['lm_update'] = dict(objects=20, host_visible=timed(lm_update, args.reps, u.sync))
        tr = u.object_lm(objs, ms, mk, True, 0, W)[0]
        out['workloads']['update_alone'] = dict(objects=20, host_visible=timed(
            lambda: u.update_object_tracks(flags, win.N, tr, win.P, win.R_b2c[0], win.t_c_b[0], True, False, 0), args.reps, u.sync))
    u.close()
    if args.kernel_stats:   # rocprofv3's kernel_stats.csv of a --trace run: Name, Calls, TotalDurationNs, AverageNs, ...
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if 'k_object_lm' in row.get('Name', ''):
                    calls, total = int(row['Calls']), float(row['TotalDurationNs'])
                    its = sum(max(out['workloads'][k]['iterations']) for k in work)   # (a launch lasts as long as its slowest object)
                    out['device'] = dict(kernel='k_object_lm', launches=calls, average_us_per_launch=total / calls / 1e3,
                                         min_us=float(row.get('MinNs', 'nan')) / 1e3, max_us=float(row.get('MaxNs', 'nan')) / 1e3,
                                         average_us_per_iteration_of_the_slowest_object=total / calls / 1e3 / (its / len(work)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
