"""Deterministic inputs of the IMU-propagation tests (CPU and GPU): samples at the shipped imu_rates (config/*.yaml: 200, 250,
650 Hz), gyro [0.1, -0.2, 0.15] + 0.02 N, accelerometer [0.3, 0.1, 9.8] + 0.1 N, Q_c from config/euroc.yaml's noise entries
(noise_gyro 0.004, noise_acc 0.08, noise_gyro_bias 2e-6, noise_acc_bias 4e-5, squared as src/orcvio.cpp:109-112 squares them),
P as orcvio_amd.synth.make_prior_cov draws it (extra states behind the clones as synth.with_extra_states)."""
from __future__ import annotations

import numpy as np

import mirror_imu as mi

IMU_RATES = (200.0, 250.0, 650.0)
FLAG_SETS = {   # use_larvio, use_left, use_closed_form, if_fej
    'larvio': (1, 0, 1, 0),
    'larvio_fej': (1, 0, 1, 1),
    'right_closed': (0, 0, 1, 0),
    'left_closed': (0, 1, 1, 0),
    'right_euler': (0, 0, 0, 0),
    'left_euler': (0, 1, 0, 0),
}
GYRO_MEAN = np.array([0.1, -0.2, 0.15])
ACC_MEAN = np.array([0.3, 0.1, 9.8])


def euroc_Qc():
    d = np.zeros(12)
    d[0:3] = 0.004 ** 2
    d[3:6] = 0.08 ** 2
    d[6:9] = 2e-6 ** 2
    d[9:12] = 4e-5 ** 2
    return np.diag(d)


def make_config(flag_set: str, rate: float) -> mi.Config:
    l, left, closed, fej = FLAG_SETS[flag_set]
    return mi.Config(use_larvio=bool(l), use_left=bool(left), use_closed_form=bool(closed), if_fej=bool(fej),
                     gravity=np.array([0.0, 0.0, -9.81]), imu_img_time_th=1.0 / (2.0 * rate), Qc=euroc_Qc())


def make_cov(n: int, rng: np.random.Generator) -> np.ndarray:
    """synth.make_prior_cov's recipe at dimension n = 22 + 6 N + extra (extra < 6: in-state feature states, variance 2.5e-3)."""
    N, extra = divmod(n - 22, 6)
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
    for i in range(N):
        d[22 + 6 * i: 22 + 6 * i + 3] = 1e-3
        d[22 + 6 * i + 3: 22 + 6 * i + 6] = 1e-2
    d[22 + 6 * N:] = 2.5e-3
    P += np.diag(d)
    P[15:22, :] = 0.0   # (extrinsics and time offset not estimated)
    P[:, 15:22] = 0.0
    return np.ascontiguousarray(0.5 * (P + P.T))


def make_state(rng: np.random.Generator, t0: float = 10.0) -> mi.ImuState:
    R = mi.so3_exp(rng.standard_normal(3) * 0.7)
    return mi.ImuState(time=t0, R=R, v=rng.standard_normal(3) * 0.5, p=rng.standard_normal(3) * 2.0,
                       bg=rng.standard_normal(3) * 1e-3, ba=rng.standard_normal(3) * 2e-2)


def make_samples(S: int, rate: float, rng: np.random.Generator, t0: float = 10.0, skipped: int = 0, beyond: int = 0):
    """rows [t, gyro, acc]: `skipped` samples at or before t0, S samples up to the image, `beyond` samples past the cut.
    Returns (samples, time_bound)."""
    dt = 1.0 / rate
    ts = [t0 - (skipped - 1 - k) * dt for k in range(skipped)]   # the last skipped sample sits exactly AT t0
    ts += [t0 + (k + 1) * dt for k in range(S)]
    time_bound = t0 + S * dt + 0.3 * dt   # the image falls between two samples; the cut is 1 / (2 rate) behind it
    ts += [t0 + (S + 1 + k) * dt for k in range(beyond)]
    rows = np.zeros((len(ts), 7))
    rows[:, 0] = ts
    rows[:, 1:4] = GYRO_MEAN + 0.02 * rng.standard_normal((len(ts), 3))
    rows[:, 4:7] = ACC_MEAN + 0.1 * rng.standard_normal((len(ts), 3))
    return rows, time_bound


def make_case(flag_set: str, S: int, n: int = 28, seed: int = 0, rate: float = 200.0, skipped: int = 0, beyond: int = 0,
              fej_offset: bool = True):
    rng = np.random.default_rng(1000 * seed + 17 * S + n)
    cfg = make_config(flag_set, rate)
    st = make_state(rng)
    samples, tb = make_samples(S, rate, rng, st.time, skipped, beyond)
    prev = np.concatenate([GYRO_MEAN + 0.02 * rng.standard_normal(3), ACC_MEAN + 0.1 * rng.standard_normal(3)])
    fej = st.copy()
    if cfg.if_fej and fej_offset:   # an update has moved imu_state since the FEJ copy was taken
        fej.v = st.v + 1e-3 * rng.standard_normal(3)
        fej.p = st.p + 1e-3 * rng.standard_normal(3)
    return dict(cfg=cfg, state=st, fej=fej, prev=prev, samples=samples, time_bound=tb, P=make_cov(n, rng), flag_set=flag_set, S=S, n=n)


def run_mirror(case, with_P: bool = True):
    """The mirror on a case: Server after batch(), and batch()'s return."""
    srv = mi.Server(case['cfg'], case['state'], P=case['P'].copy() if with_P else None, fej_now=case['fej'],
                    m_gyro_old=case['prev'][:3], m_acc_old=case['prev'][3:])
    info = srv.batch(case['time_bound'], case['samples'])
    return srv, info


def blocks3(n: int):
    """the 3 x 3 blocks (the last may be narrower) that tile an n x n matrix"""
    e = list(range(0, n, 3))
    return [(i, min(i + 3, n), j, min(j + 3, n)) for i in e for j in e]


def block_error(got: np.ndarray, ref: np.ndarray) -> float:
    """largest element-wise difference of a block, relative to the block's largest reference entry, over all 3 x 3 blocks; a block
    whose reference is all zero must be zero."""
    worst = 0.0
    for (i0, i1, j0, j1) in blocks3(ref.shape[0]):
        r, g = ref[i0:i1, j0:j1], got[i0:i1, j0:j1]
        m = float(np.max(np.abs(r)))
        d = float(np.max(np.abs(g - r)))
        if m == 0.0:
            if d != 0.0:
                return float('inf')
            continue
        worst = max(worst, d / m)
    return worst


def write_case(path, case):
    """a case as tests/cpp/imu_model_main.cpp reads it (text, whitespace separated)"""
    c, st, fej = case['cfg'], case['state'], case['fej']
    vals = [float(c.use_larvio), float(c.use_left), float(c.use_closed_form), float(c.if_fej)]
    vals += list(c.gravity) + [c.imu_img_time_th] + list(np.diag(c.Qc))
    vals += [st.time] + list(st.R.ravel()) + list(st.v) + list(st.p) + list(st.bg) + list(st.ba) + list(fej.v) + list(fej.p)
    vals += list(case['prev']) + [case['time_bound'], float(len(case['samples']))] + list(case['samples'].ravel())
    with open(path, 'w') as f:
        f.write(' '.join(repr(float(v)) for v in vals))


def to_capi(case):
    """a case as orcvio_amd.capi takes it: (ImuConfig, ImuState, prev_meas); the state and prev_meas are fresh copies"""
    from orcvio_amd import capi
    c, st, fej = case['cfg'], case['state'], case['fej']
    cfg = capi.MsckfUpdater.imu_config(22, c.use_larvio, c.use_left, c.use_closed_form, c.if_fej, c.gravity, c.imu_img_time_th, np.diag(c.Qc))
    state = capi.MsckfUpdater.imu_state(st.time, st.R, st.v, st.p, st.bg, st.ba, fej.v, fej.p)
    return cfg, state, case['prev'].copy()


# ---- the cases the device is compared on (tests/test_gpu_imu.py) and the mirror's own spread is measured on (tests/test_imu_mirror.py)
# k_imu_phi_q maps sample k to wavefront k // C, C = ceil(S / 4), and combines the four partial products in order: the edges are the
# sample counts at which C changes (4 -> 5, 8 -> 9), at which a wavefront's chunk is short or empty (5: 2 2 1 0, 9: 3 3 3 0, 33: 9 9 9 6,
# 127: 32 32 32 31) and the capacity itself.
S_LIST = (1, 2, 3, 4, 5, 8, 9, 33, 127, 128)
N_LIST = (22, 28, 142, 145)   # no clone; one clone; 20 clones; 20 clones + three in-state feature states


def rate_for(S: int) -> float:
    return 200.0 if S <= 5 else (250.0 if S <= 9 else 650.0)


def gpu_cases():
    """(flag_set, S, n) of every comparison case."""
    out = []
    for fs in FLAG_SETS:
        out += [(fs, S, 28) for S in S_LIST]
        out += [(fs, 3, 22), (fs, 33, 142), (fs, 5, 145), (fs, 128, 145)]
    return out


def gpu_case(fs: str, S: int, n: int):
    return make_case(fs, S, n=n, seed=5, rate=rate_for(S), skipped=1, beyond=2)


# The mirror's own spread (tests/test_imu_mirror.py measures it and asserts it within a factor of two of this recorded figure): the largest element-wise
# difference, relative to the 3 x 3 block's largest entry, between the mirror's sequential and its pairwise accumulation order, over
# Phi, Q and the propagated P of every case above.  The device's regression bar is ten times it.
MIRROR_SPREAD = 9.7e-15   # measured 9.678e-15, at (right_closed, S = 128, n = 28)
REGRESSION_BAR = 10 * MIRROR_SPREAD
