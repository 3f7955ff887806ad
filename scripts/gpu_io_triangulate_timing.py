"""Host-visible time of an update that triangulates its own tracks (orcvio_msckf_io_triangulate, GPU) against the only route there
was before it and against the update alone.  Per workload three ways, alternating in blocks:
  a  orcvio_msckf_triangulate (a call of its own: upload, kernel, download, wait), the arena rebuilt WITHOUT the invalid tracks at the
     returned positions, then the unarmed update
  b  the arena filled with every track (positions NaN), orcvio_msckf_io_triangulate, the update
  c  the arena filled with every track at given positions, the unarmed update (what the stream figures of the README measure)
Reported per workload and way: median and p95 over all samples and the block medians (their spread is the yardstick for a
difference), a - b (the saving against the old route) and b - c (what triangulation costs on the frame's critical path).  Microseconds.
Workloads: config_window(1) through io_update (resident covariance, committed: the arena is filled through cached views, the library
calls are the ctypes calls themselves), and the four frames of make_stream(Flags(use_larvio=1), cycle=4) through io_step_frame
(the binding's marshalling of the frame is inside every way alike; every sample starts from the covariance in front of its frame).
--kernel-only: way b alone, for a rocprofv3 --kernel-trace --stats run of its own.
usage: python scripts/gpu_io_triangulate_timing.py [--blocks 5] [--reps 40] [--tag r16a] [--kernel-only]"""
import argparse
import ctypes as C
import dataclasses
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
import tri_io_cases as tc  # noqa: E402


def summarise(samples, block_med):
    row = {}
    for k, v in samples.items():
        a = np.sort(v)
        row[k] = dict(median=float(np.median(a)), p95=float(a[int(0.95 * (len(a) - 1))]), block_medians=block_med[k])
    row['a_minus_b'] = row['a']['median'] - row['b']['median'] if 'a' in row else None
    row['b_minus_c'] = row['b']['median'] - row['c']['median'] if 'c' in row else None
    return row


def run_ways(ways, reset, blocks, reps):
    samples = {k: [] for k in ways}
    block_med = {k: [] for k in ways}
    for blk in range(blocks + 1):   # (block 0: warm-up of every way's shapes and launch graphs)
        for k, fn in ways.items():
            ts = []
            for _ in range(reps):
                reset()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e6)
            if blk > 0:
                samples[k] += ts
                block_med[k].append(float(np.median(ts)))
    return summarise(samples, block_med)


class Arena:
    """io_begin for one shape with the views cached: fill() is the raw library call and five array copies."""

    def __init__(self, u, w):
        self.u, self.w = u, w
        self.shape = (w.N, w.F, int(w.obs_ptr[-1]))
        self.io = u.io_begin(w.flags, *self.shape, with_P=False)
        self.fl, self.ioc = u._io_keep
        self.poses = np.zeros((w.N, capi.POSE_STRIDE))
        self.poses[:, 0:9] = w.R_b2w.reshape(w.N, 9); self.poses[:, 9:12] = w.t_b_w; self.poses[:, 12:15] = w.t_fej
        self.poses[:, 15:24] = w.R_b2c.reshape(w.N, 9); self.poses[:, 24:27] = w.t_c_b

    def fill(self, p_w):
        u, io, w = self.u, self.io, self.w
        rc = u.lib.orcvio_msckf_io_begin(u.h, C.byref(self.fl), self.shape[0], self.shape[1], self.shape[2], 0, C.byref(self.ioc))
        if rc != 0:
            raise capi.MsckfError(rc, 'orcvio_msckf_io_begin')
        np.copyto(io['poses'], self.poses); np.copyto(io['obs_ptr'], w.obs_ptr); np.copyto(io['p_w'], p_w)
        np.copyto(io['obs_clone'], w.obs_clone); np.copyto(io['obs_z'], w.obs_z)


def window_workload(u, w, args):
    lib, h = u.lib, u.h
    nanpw = np.full((w.F, 3), np.nan)

    def reset():
        u.cov_set(w.P)
        u.sync()
    reset()
    # the call of its own, marshalled once
    _, ws, ts, arrs = u._structs(w)
    ts.p_w = None
    cfg = u._tri_config(None)
    tv, tp, tsol, tf, tcost = np.zeros(w.F, np.int32), np.zeros((w.F, 3)), np.zeros((w.F, 3)), np.zeros(w.F, np.int32), np.zeros(w.F)
    res = capi.TriangulationResult(capi._i(tv), capi._d(tp), capi._d(tsol), capi._i(tf), capi._d(tcost))
    assert lib.orcvio_msckf_triangulate(h, C.byref(cfg), C.byref(ws), C.byref(ts), None, C.byref(res)) == 0
    keep = tv == 1
    wk = tc.select_tracks(w, keep, tp)
    full, kept = Arena(u, w), None
    stats = np.zeros(8, np.int32)
    out = capi.MsckfIoTri()

    def update():
        rc = lib.orcvio_msckf_io_update(h, 0, 1, capi._i(stats))
        if rc != 0:
            raise capi.MsckfError(rc, 'orcvio_msckf_io_update')

    def way_a():
        assert lib.orcvio_msckf_triangulate(h, C.byref(cfg), C.byref(ws), C.byref(ts), None, C.byref(res)) == 0
        kept.fill(wk.p_w)
        update()

    def way_b():
        full.fill(nanpw)
        assert lib.orcvio_msckf_io_triangulate(h, C.byref(cfg), None, C.byref(out)) == 0
        update()

    def way_c():
        full.fill(w.p_w)
        update()

    kept = Arena(u, wk)
    ways = dict(b=way_b) if args.kernel_only else dict(a=way_a, b=way_b, c=way_c)
    row = run_ways(ways, reset, args.blocks, args.reps)
    row.update(tracks=int(w.F), kept=int(keep.sum()), clones=int(w.N))
    return row


def frame_workloads(u, args):
    frames, P0 = synth.make_stream(synth.Flags(use_larvio=1), cycle=4)
    u.set_extra_states(tc.NSLAM)
    u.set_ekf_rows_mode(True)
    step = lambda w, fr, arm: u.io_step_frame(w, fr['Phi'], fr['Q'], True, fr['slam'], 1, fr['prune'], 0, fr['remove'], triangulate=arm)
    priors, P = [], P0
    u.cov_set(P0)
    for fr in frames:   # the covariance in front of every frame (the frames at their given positions)
        priors.append(P)
        step(fr['w'], fr, None)
        P = u.cov_get()
    rows = {}
    for it, fr in enumerate(frames):
        w = fr['w']
        hidden = dataclasses.replace(w, p_w=np.full_like(w.p_w, np.nan))
        state = {}

        def reset(P=priors[it]):
            u.cov_set(P)
            u.sync()

        def way_a(w=w, fr=fr):
            t = u.triangulate(w)
            step(tc.select_tracks(w, t['valid'] == 1, t['p_w']), fr, None)
            state['kept'] = int(t['valid'].sum())

        def way_b(hidden=hidden, fr=fr):
            step(hidden, fr, True)

        def way_c(w=w, fr=fr):
            step(w, fr, None)
        ways = dict(b=way_b) if args.kernel_only else dict(a=way_a, b=way_b, c=way_c)
        row = run_ways(ways, reset, args.blocks, args.reps)
        row.update(tracks=int(w.F), kept=state.get('kept'), clones=int(w.N), prune=fr['prune'] is not None)
        rows[f'stream_frame_{it}'] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--tag', default=None)
    ap.add_argument('--kernel-only', action='store_true')
    args = ap.parse_args()
    out = dict(build=dict(source_sha16=b.source_sha16()), blocks=args.blocks, reps=args.reps, unit='us', workloads={})
    u = capi.MsckfUpdater(device=0, max_clones=32, max_features=256, max_observations=8192)
    out['workloads']['config1_io_update'] = window_workload(u, synth.config_window(1), args)
    u.close()
    u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096)
    out['workloads'].update(frame_workloads(u, args))
    out['counters'] = u.counters()
    u.close()
    if args.tag and not args.kernel_only:
        dst = os.environ.get('PROFILES_DST') or os.path.join(ROOT, 'profiles')
        os.makedirs(dst, exist_ok=True)
        with open(os.path.join(dst, f'{args.tag}_io_triangulate_timing.json'), 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
