"""Host-visible time of orcvio_msckf_object_init and orcvio_msckf_object_init_lm (GPU), through ctypes, median and p95 over --reps
calls (default 200), microseconds, on synth.make_objects tracks (F = 30, K = 12; the priors are the car means):
  init_1 / init_20          object_init for one object and for twenty in one call
  init_lm_1 / init_lm_20    object_init_lm: ONE call (one upload, k_object_init and k_object_lm on one stream, one wait)
  two_calls_1 / _20         object_init followed by object_lm from its result: two calls, two uploads, two waits, the host repacking
  lm_alone_1 / _20          object_lm alone from the same start (the second of the two calls), for comparison
and, with --trace N, nothing but N calls of init_1, init_20 and init_lm_20 in turn, for a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python scripts/gpu_object_init_timing.py --trace 50); --kernel-stats CSV then merges the traced
device time of k_object_init per launch into the record.
There is NO baseline here: the reference's Eigen initialiser cannot be built in this tree.  The numbers say what the calls cost and
what the one call saves over the two, not what either saves over the reference.
usage: python scripts/gpu_object_init_timing.py [--reps 200] [--out FILE] [--trace N] [--kernel-stats CSV] [--pose-form 0]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orcvio_amd import capi, synth  # noqa: E402
from orcvio_amd import build as b  # noqa: E402

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
    ap.add_argument('--pose-form', type=int, default=0)
    args = ap.parse_args()
    flags = synth.Flags(use_larvio=0, use_left_perturbation=0)
    win = synth.make_window(N=30, F=2, seed=4, flags=flags, track_len=3)
    objs = synth.make_objects(win, n_objects=20, seed=4)
    ms = [synth.CAR_MEAN_SHAPE] * 20
    mk = [synth.CAR_KEYPOINTS_MEAN] * 20
    u = capi.MsckfUpdater(device=0, max_clones=32, max_features=64, max_observations=1024)
    form = args.pose_form

    def two_calls(n):
        inits = u.object_init(objs[:n], mk[:n], pose_form=form)
        starts = [synth.ObjectTrack(wTo=i['wTo'], shape=ms[0], kps=mk[0], frames=o.frames) for i, o in zip(inits, objs[:n]) if i['status'] == 1]
        return u.object_lm(starts, ms[:len(starts)], mk[:len(starts)], True, 0, W)

    out = dict(build=dict(source_sha16=b.source_sha16()), unit='us', reps=args.reps, shape=dict(F=len(objs[0].frames), K=12), pose_form=form,
               baseline='none: the reference initialiser is not built here, the numpy mirror is a checker', workloads={})
    inits, _, stats = u.object_init_lm(objs, ms, mk, True, 0, W, pose_form=form)
    out['init_status'] = [i['status'] for i in inits]
    out['lm_status'] = [s['status'] for s in stats]
    out['lm_iterations'] = [s['iterations'] for s in stats]
    if args.trace:
        for _ in range(args.trace):
            u.object_init(objs[:1], mk[:1], pose_form=form)
            u.object_init(objs, mk, pose_form=form)
            u.object_init_lm(objs, ms, mk, True, 0, W, pose_form=form)
        out['traced_calls_per_workload'] = args.trace
    else:
        for n in (1, 20):
            wl = out['workloads']
            wl['init_%d' % n] = dict(objects=n, host_visible=timed(lambda: u.object_init(objs[:n], mk[:n], pose_form=form), args.reps, u.sync))
            wl['init_lm_%d' % n] = dict(objects=n, host_visible=timed(lambda: u.object_init_lm(objs[:n], ms[:n], mk[:n], True, 0, W, pose_form=form),
                                                                      args.reps, u.sync))
            wl['two_calls_%d' % n] = dict(objects=n, host_visible=timed(lambda: two_calls(n), args.reps, u.sync))
            starts = [synth.ObjectTrack(wTo=i['wTo'], shape=ms[0], kps=mk[0], frames=o.frames) for i, o in zip(inits[:n], objs[:n])]
            wl['lm_alone_%d' % n] = dict(objects=n, host_visible=timed(lambda: u.object_lm(starts, ms[:n], mk[:n], True, 0, W), args.reps, u.sync))
            wl['one_call_saves_%d' % n] = dict(median=wl['two_calls_%d' % n]['host_visible']['median'] - wl['init_lm_%d' % n]['host_visible']['median'])
    u.close()
    if args.kernel_stats:   # rocprofv3's kernel_stats.csv of a --trace run: Name, Calls, TotalDurationNs, AverageNs, ...
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if 'k_object_init' in row.get('Name', ''):
                    calls, total = int(row['Calls']), float(row['TotalDurationNs'])
                    out['device'] = dict(kernel='k_object_init', launches=calls, average_us_per_launch=total / calls / 1e3,
                                         min_us=float(row.get('MinNs', 'nan')) / 1e3, max_us=float(row.get('MaxNs', 'nan')) / 1e3)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
