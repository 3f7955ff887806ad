"""Deterministic inputs of the leg_dim = 46 IMU-propagation tests (CPU and GPU): imu_cases' flag sets, rates, samples and states, with
the 24 IMU intrinsics in the state and a covariance whose intrinsic rows and columns are not zero.

Two intrinsics sets: 'identity' (T2 = M2 = 1, the rest 0: Tg = Ma = I, As = 0, what leg_dim = 22 assumes) and 'general' (identity +
0.01 N(0, 1) on all 24, seeded: As != 0, Ma and Tg neither diagonal nor symmetric)."""
from __future__ import annotations

import numpy as np

import imu_cases as ic
import mirror_imu_calib as mc

LEG = 46
INTRINSIC_SETS = ('identity', 'general')


def make_intrinsics(which: str, seed: int = 0) -> np.ndarray:
    x = mc.IDENTITY_INTRINSICS.copy()
    if which == 'general':
        x = x + 0.01 * np.random.default_rng(7700 + seed).standard_normal(24)
    else:
        assert which == 'identity'
    return x


def make_cov(n: int, rng: np.random.Generator) -> np.ndarray:
    """imu_cases.make_cov's recipe at dimension n = 46 + 6 N + extra; the intrinsics carry a prior of sigma 1e-2 (variance 1e-4) and
    are correlated with everything the low-rank part correlates."""
    N, extra = divmod(n - LEG, 6)
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    P = 1e-4 * (A @ A.T)
    d = np.zeros(n)
    d[0:3] = 4e-4
    d[3:6] = 0.25
    d[6:9] = 1.0
    d[9:12] = 4e-4
    d[12:15] = 0.01
    d[15:18] = 3.0462e-8
    d[18:21] = 9e-8
    d[21] = 4e-6
    d[22:46] = 1e-4
    for i in range(N):
        d[LEG + 6 * i: LEG + 6 * i + 3] = 1e-3
        d[LEG + 6 * i + 3: LEG + 6 * i + 6] = 1e-2
    d[LEG + 6 * N:] = 2.5e-3
    P += np.diag(d)
    P[15:22, :] = 0.0   # (extrinsics and time offset not estimated)
    P[:, 15:22] = 0.0
    return np.ascontiguousarray(0.5 * (P + P.T))


def make_case(flag_set: str, S: int, intr: str = 'general', n: int = 52, seed: int = 0, rate: float = 200.0, skipped: int = 0, beyond: int = 0,
              fej_offset: bool = True):
    """imu_cases.make_case's draw (the same generator stream for state, samples, previous sample and FEJ offset), then the covariance
    at 46 and the intrinsics."""
    case = ic.make_case(flag_set, S, n=n - 24, seed=seed, rate=rate, skipped=skipped, beyond=beyond, fej_offset=fej_offset)
    rng = np.random.default_rng(500000 + 1000 * seed + 17 * S + n)
    case['P'] = make_cov(n, rng)
    case['n'] = n
    case['intr'] = make_intrinsics(intr, seed)
    case['intr_set'] = intr
    return case


def run_mirror(case, with_P: bool = True):
    srv = mc.Server46(case['cfg'], case['state'], case['intr'], P=case['P'].copy() if with_P else None, fej_now=case['fej'],
                      m_gyro_old=case['prev'][:3], m_acc_old=case['prev'][3:])
    info = srv.batch(case['time_bound'], case['samples'])
    return srv, info


block_error = ic.block_error


def write_case(path, case):
    """a case as tests/cpp/imu_calib_model_main.cpp reads it: imu_cases.write_case's text with the 24 intrinsics in front"""
    ic.write_case(path, case)
    with open(path) as f:
        body = f.read()
    with open(path, 'w') as f:
        f.write(' '.join(repr(float(v)) for v in case['intr']) + ' ' + body)


def to_capi(case):
    """(ImuConfig at leg_dim 46, ImuIntrinsics, ImuState, prev_meas); the state and prev_meas are fresh copies"""
    from orcvio_amd import capi
    c, st, fej = case['cfg'], case['state'], case['fej']
    cfg = capi.MsckfUpdater.imu_config(46, c.use_larvio, c.use_left, c.use_closed_form, c.if_fej, c.gravity, c.imu_img_time_th, np.diag(c.Qc))
    state = capi.MsckfUpdater.imu_state(st.time, st.R, st.v, st.p, st.bg, st.ba, fej.v, fej.p)
    return cfg, capi.MsckfUpdater.imu_intrinsics(case['intr']), state, case['prev'].copy()


# ---- the cases the device is compared on (tests/test_gpu_imu_calib.py) and the mirror's own spread is measured on
# k_imu_phi_q46 maps sample k to wavefront k // C, C = ceil(S / 4), as k_imu_phi_q does, and runs a wavefront's chunk in rounds of eight
# samples: beside imu_cases.S_LIST (the counts at which C changes or a chunk is short or empty) the edges are the counts at which a
# chunk crosses a round boundary: C = 8 | 9 at S = 32 | 33, C = 16 | 17 at 64 | 65, C = 24 | 25 at 96 | 97.
S_LIST = (1, 2, 3, 4, 5, 8, 9, 32, 33, 64, 65, 96, 97, 127, 128)
N_LIST = (46, 52, 166, 169)   # no clone; one clone; 20 clones; 20 clones + three in-state feature states

rate_for = ic.rate_for


def gpu_cases():
    """(flag_set, S, n, intrinsics set) of every comparison case."""
    out = []
    for fs in ic.FLAG_SETS:
        for intr in INTRINSIC_SETS:
            out += [(fs, S, 52, intr) for S in S_LIST]
        out += [(fs, 3, 46, 'general'), (fs, 33, 166, 'general'), (fs, 5, 169, 'general'), (fs, 128, 169, 'general')]
    return out


def gpu_case(fs: str, S: int, n: int, intr: str):
    return make_case(fs, S, intr=intr, n=n, seed=5, rate=rate_for(S), skipped=1, beyond=2)


# The mirror's own spread at 46 (tests/test_imu_calib_mirror.py measures it and asserts it within a factor of two of this recorded
# figure): the largest element-wise difference, relative to the 3 x 3 block's largest entry, between the mirror's sequential and its
# pairwise accumulation order, over Phi, Q and the propagated P of every case above.  The device's regression bar is ten times it.
MIRROR_SPREAD_46 = 9.7e-15   # measured 9.678e-15, at (right_closed, S = 128, n = 52, identity intrinsics)
REGRESSION_BAR_46 = 10 * MIRROR_SPREAD_46
