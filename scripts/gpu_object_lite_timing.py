"""Host-visible time of the lite (bbox-only) object mapper (GPU), through ctypes, median and p95 over --reps calls (default 200),
microseconds, on synth.make_objects tracks without their keypoints (F = 30; the prior is the car's mean shape), for 1, 20 and 64
objects per call:
  init_lm_lite_N     object_init_lm_lite: ONE call (one upload, k_object_init_lite and k_object_lm_lite on one stream, one wait)
  two_calls_N        object_init_lite followed by object_lm_lite from its result: two calls, two uploads, two waits
  lm_lite_alone_N    object_lm_lite alone from the same start (the second of the two calls)
  lm_k1_context_N    FOR CONTEXT ONLY: orcvio_msckf_object_lm (k_object_lm, one workgroup per object) on the same tracks with ONE keypoint
                     kept, from the same start -- another problem (12 degrees of freedom, keypoint rows), not a baseline
The four are measured in alternating blocks (--blocks, default 4) so that a drift of the machine reaches all of them alike.
With --trace N, nothing but N calls of object_lm_lite on --trace-objects objects (default 1), for a kernel trace taken in a run of
its own (rocprofv3 --kernel-trace --stats -- python scripts/gpu_object_lite_timing.py --trace 50); --kernel-stats CSV then merges the
traced device time of k_object_lm_lite per launch, and per iteration of the traced objects' longest run, into the record.
There is NO baseline here: the reference's Eigen optimiser cannot be built in this tree, and the parent had no lite path.
usage: python scripts/gpu_object_lite_timing.py [--reps 200] [--blocks 4] [--out FILE] [--trace N] [--trace-objects 1] [--kernel-stats CSV]"""
import argparse
import csv
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orcvio_amd import capi, synth  # noqa: E402
from orcvio_amd import build as b  # noqa: E402

POSE_FORM = 0     # the full translation: the start the optimiser is given in the timed calls
MAX_ITER = 400


def timed_alternating(fns, reps, blocks, sync):
    """fns: dict name -> callable.  Each is called reps times, in `blocks` blocks that alternate between them."""
    ts = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(5):
            fn()
    per = max(reps // blocks, 1)
    for _ in range(blocks):
        for k, fn in fns.items():
            for _ in range(per):
                sync()
                t0 = time.perf_counter()
                fn()
                ts[k].append((time.perf_counter() - t0) * 1e6)
    out = {}
    for k, v in ts.items():
        a = np.sort(v)
        out[k] = dict(median=float(np.median(a)), p95=float(a[int(0.95 * (len(a) - 1))]), calls=len(a))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--blocks', type=int, default=4)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', type=int, default=0)
    ap.add_argument('--trace-objects', type=int, default=1)
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    flags = synth.Flags(use_larvio=0, use_left_perturbation=0)
    win = synth.make_window(N=30, F=2, seed=4, flags=flags, track_len=3)
    full = synth.make_objects(win, n_objects=64, seed=4)
    objs = [dataclasses.replace(o, kps=np.zeros((0, 3))) for o in full]
    ms = [synth.CAR_MEAN_SHAPE] * len(objs)
    u = capi.MsckfUpdater(device=0, max_clones=32, max_features=64, max_observations=1024)

    inits, _, stats = u.object_init_lm_lite(objs, ms, True, 0, max_iter=MAX_ITER, pose_form=POSE_FORM)
    starts = [dataclasses.replace(o, wTo=i['wTo'], shape=np.array(ms[0])) for i, o in zip(inits, objs)]
    # the same tracks with keypoint 0 kept, from the same start: the context workload of k_object_lm
    k1 = [dataclasses.replace(o, wTo=i['wTo'], shape=np.array(ms[0]), kps=synth.CAR_KEYPOINTS_MEAN[:1].copy(),
                              frames=[dict(fr, zs=np.asarray(fr['zs'])[:1]) for fr in o.frames]) for i, o in zip(inits, full)]
    mk1 = [synth.CAR_KEYPOINTS_MEAN[:1]] * len(objs)
    _, k1_stats = u.object_lm(k1, ms, mk1, True, 0, (1.0, 1.0, 1.0, 1.0), max_iter=MAX_ITER)
    out = dict(build=dict(source_sha16=b.source_sha16()), unit='us', reps=args.reps, blocks=args.blocks, shape=dict(F=len(objs[0].frames), K=0),
               pose_form=POSE_FORM, max_iter=MAX_ITER,
               baseline='none: the reference optimiser is not built here, the parent has no lite path, the numpy mirror is a checker',
               init_status=[i['status'] for i in inits], lm_status=[s['status'] for s in stats], lm_iterations=[s['iterations'] for s in stats],
               k1_context_status=[s['status'] for s in k1_stats], k1_context_iterations=[s['iterations'] for s in k1_stats], workloads={})

    def two_calls(n):
        ii = u.object_init_lite(objs[:n], ms[:n], POSE_FORM)
        st = [dataclasses.replace(o, wTo=i['wTo'], shape=np.array(ms[0])) for i, o in zip(ii, objs[:n]) if i['status'] == 1]
        return u.object_lm_lite(st, ms[:len(st)], True, 0, max_iter=MAX_ITER)

    if args.trace:
        n = args.trace_objects
        for _ in range(args.trace):
            u.object_lm_lite(starts[:n], ms[:n], True, 0, max_iter=MAX_ITER)
        out['traced'] = dict(calls=args.trace, objects=n, iterations=[s['iterations'] for s in stats[:n]])
    else:
        for n in (1, 20, 64):
            r = timed_alternating({
                'init_lm_lite_%d' % n: lambda: u.object_init_lm_lite(objs[:n], ms[:n], True, 0, max_iter=MAX_ITER, pose_form=POSE_FORM),
                'two_calls_%d' % n: lambda: two_calls(n),
                'lm_lite_alone_%d' % n: lambda: u.object_lm_lite(starts[:n], ms[:n], True, 0, max_iter=MAX_ITER),
                'lm_k1_context_%d' % n: lambda: u.object_lm(k1[:n], ms[:n], mk1[:n], True, 0, (1.0, 1.0, 1.0, 1.0), max_iter=MAX_ITER),
            }, args.reps, args.blocks, u.sync)
            for k, v in r.items():
                out['workloads'][k] = dict(objects=n, host_visible=v)
            out['workloads']['one_call_saves_%d' % n] = dict(median=r['two_calls_%d' % n]['median'] - r['init_lm_lite_%d' % n]['median'])
    u.close()
    if args.kernel_stats:   # rocprofv3's kernel_stats.csv of a --trace run: Name, Calls, TotalDurationNs, AverageNs, ...
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if 'k_object_lm_lite' in row.get('Name', ''):
                    calls, total = int(row['Calls']), float(row['TotalDurationNs'])
                    avg = total / calls / 1e3
                    its = max(out['lm_iterations'][:args.trace_objects])
                    out['device'] = dict(kernel='k_object_lm_lite', launches=calls, objects=args.trace_objects, average_us_per_launch=avg,
                                         longest_run_iterations=its, us_per_iteration=avg / (its + 1),   # (+ 1: the start's evaluation)
                                         min_us=float(row.get('MinNs', 'nan')) / 1e3, max_us=float(row.get('MaxNs', 'nan')) / 1e3)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
