"""Host-visible cost of reading the odometry message's covariances (getPpose / getPvel: 45 numbers of the leading 9 x 9 of P) from the
device-resident covariance (GPU), at n = 142, 154 and 178 (20 clones; 0 or 12 in-state features of width 1 or 3):
  get            (a) orcvio_msckf_cov_get of the whole matrix -- the only route before orcvio_msckf_cov_get_marginal; the getters
                     themselves (two 3 x 3 congruences, ~200 flops in C++) are NOT in its time, which favours this route
  marginal       (b) orcvio_msckf_cov_get_marginal with the one spec of the host layer (idx = {6,7,8, 0,1,2, 3,4,5}, T = blkdiag(R, R, R))
  frame          (c) orcvio_msckf_io_step_frame alone (propagation, augmentation, an update of 40 tracks, the oldest clone marginalised),
                     then the host's state increment (orcvio_msckf_increment_state on the frame's dx)
  frame_marginal     the frame, orcvio_msckf_cov_marginal_submit, the state increment, orcvio_msckf_cov_marginal_collect
  frame_get          the frame, the state increment, orcvio_msckf_cov_get
The additional cost per frame is frame_marginal - frame, and frame_get - frame for route (a).  Every call is the bare ctypes call on
arguments prepared outside the timed region (the binding's staging of a window is in no route); every frame sample starts from the same
resident covariance (cov_set, io_begin and the arena's fill outside the timed region).  The routes alternate inside one loop; a BLOCK is
`--block` samples of every route, and the figure of a route is the median over the blocks' medians with its own max - min over the
blocks beside it.  "Faster than cov_get" is claimed only where the gain exceeds route (a)'s own spread.  Microseconds.
usage: python scripts/gpu_cov_marginal_timing.py [--blocks 7] [--block 150] [--warmup 100] [--tag r35a]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--block', type=int, default=150)
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--tag', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, ROOT)
    from orcvio_amd import capi, synth
    from orcvio_amd import build as b
    import cov_cases as cc
    import cov_marginal_cases as mc

    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    leg, N = 22, 20
    fl = synth.Flags(use_larvio=1, leg_dim=leg)
    R = mc.rotation(1)
    idx, T = mc.odometry_spec(R)
    Phi, Q = cc.phi_q(leg, 3)
    clock = time.perf_counter
    results = {}
    for extra in (0, 12, 36):
        n = leg + 6 * N + extra
        u = capi.MsckfUpdater(device=0, max_clones=24, max_features=256, max_observations=4096)
        lib, h = u.lib, u.h
        u.set_extra_states(extra)
        P0 = cc.graded_factorable(n)   # 20 clones: the frame augments to 21 and marginalises the oldest
        win = dataclasses.replace(synth.make_window(N=N + 1, F=40, seed=5, track_len=(3, 8), flags=fl), n_extra=extra)
        nobs = int(win.obs_ptr[-1])
        # ---- the arguments of every call, once
        q, keep = u._marginal(idx, T)
        out = np.zeros((64, 64))
        rows = C.c_int32(0)
        Pbuf = np.zeros((n, n))
        nn = C.c_int32(0)
        Ph, Qc = np.ascontiguousarray(Phi), np.ascontiguousarray(Q)
        rm = np.zeros(1, dtype=np.int32)
        st = capi.FrameStep()
        st.leg_dim, st.Phi, st.Q, st.augment = leg, Ph.ctypes.data_as(dp), Qc.ctypes.data_as(dp), 1
        st.remove_clones, st.n_remove = rm.ctypes.data_as(ip), 1
        res = capi.FrameResult()
        cfl = capi.make_flags(fl)
        state = capi.MsckfState()
        state.R_b2w_imu[:] = list(np.eye(3).ravel())
        state.R_b2c[:] = list(np.eye(3).ravel())
        state.n_clones = N + 1
        sb = [win.R_b2w.copy(), win.t_b_w.copy(), np.zeros((N + 1, 3, 3)), np.zeros((N + 1, 3))]
        state.clone_R_b2w, state.clone_t_b_w, state.clone_R_c2w, state.clone_t_c_w = (a.ctypes.data_as(dp) for a in sb)
        dx = np.zeros(n + 6)

        def prepare_frame():
            u.cov_set(P0)
            io = u.io_begin(win.flags, win.N, win.F, nobs, with_P=2)
            u.io_fill(io, win, with_P=False)
            u.sync()

        def frame():
            rc = lib.orcvio_msckf_io_step_frame(h, C.byref(st), C.byref(res))
            assert rc == 0 and res.n_after == n, (rc, res.n_after)

        def increment():
            C.memmove(dx.ctypes.data, res.dx, 8 * (n + 6))
            lib.orcvio_msckf_increment_state(C.byref(cfl), dx.ctypes.data_as(dp), C.byref(state))

        def r_get():
            assert lib.orcvio_msckf_cov_get(h, C.byref(nn), Pbuf.ctypes.data_as(dp)) == 0

        def r_marginal():
            assert lib.orcvio_msckf_cov_get_marginal(h, C.byref(q), out.ctypes.data_as(dp)) == 0

        def r_frame():
            frame()
            increment()

        def r_frame_marginal():
            frame()
            assert lib.orcvio_msckf_cov_marginal_submit(h, C.byref(q)) == 0
            increment()
            assert lib.orcvio_msckf_cov_marginal_collect(h, out.ctypes.data_as(dp), C.byref(rows)) == 0

        def r_frame_get():
            frame()
            increment()
            assert lib.orcvio_msckf_cov_get(h, C.byref(nn), Pbuf.ctypes.data_as(dp)) == 0

        routes = dict(get=(r_get, False), marginal=(r_marginal, False), frame=(r_frame, True), frame_marginal=(r_frame_marginal, True),
                      frame_get=(r_frame_get, True))
        meds = {k: [] for k in routes}
        prepare_frame()
        r_frame()   # (a resident covariance of dimension n for the reads that come first)
        for blk in range(-1, args.blocks):
            samples = {k: [] for k in routes}
            for rep in range(args.warmup if blk < 0 else args.block):
                for k, (fn, is_frame) in routes.items():   # (the routes alternate: a drift of the machine touches every one alike)
                    if is_frame:
                        prepare_frame()
                    else:
                        u.sync()
                    t0 = clock()
                    fn()
                    dt = (clock() - t0) * 1e6
                    u.sync()
                    samples[k].append(dt)
            if blk >= 0:
                for k in routes:
                    meds[k].append(float(np.median(samples[k])))
        # the two reads agree (the frame's last state is what both see)
        prepare_frame()
        r_frame_marginal()
        r_get()
        assert rows.value == 9 and mc.passes(mc.Case(n, 9, 9, P=Pbuf, idx=idx, T=T), out.ravel()[:81].reshape(9, 9))
        u.close()

        def row(v):
            return dict(median=float(np.median(v)), spread=float(max(v) - min(v)), blocks=[round(x, 2) for x in v])
        r = {k: row(v) for k, v in meds.items()}
        add_m = [a - f for a, f in zip(meds['frame_marginal'], meds['frame'])]
        add_g = [a - f for a, f in zip(meds['frame_get'], meds['frame'])]
        r['added_per_frame'] = dict(marginal=row(add_m), get=row(add_g))
        gain_alone = r['get']['median'] - r['marginal']['median']
        gain_frame = float(np.median(add_g)) - float(np.median(add_m))
        r['claims'] = dict(blocking_gain=gain_alone, blocking_faster=bool(gain_alone > r['get']['spread']),
                           frame_gain=gain_frame, frame_faster=bool(gain_frame > r['added_per_frame']['get']['spread']))
        r['bytes_cov_get'] = 8 * n * n
        results['n%d' % n] = r
    outd = dict(build=dict(source_sha16=b.source_sha16()), unit='us', blocks=args.blocks, block=args.block, warmup=args.warmup, clones=N,
                tracks=40, states=results)
    if args.tag:
        with open(os.path.join(ROOT, 'profiles', f'{args.tag}_cov_marginal_timing.json'), 'w') as f:
            f.write(json.dumps(outd, indent=1) + '\n')
    print(json.dumps(outd))


if __name__ == '__main__':
    main()
