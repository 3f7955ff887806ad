"""numpy restatement of the reference's IMU step at leg_dim = 46 (calib_imu_instrinsic = 1), written from the reference on top of
tests/mirror_imu.py (predictors, Euler forms, right closed form, selection):

  updateImuMx        src/orcvio.cpp:4373-4418   Tg, As, Ma from T1 T2 T3 A1 A2 A3 M1 M2 (error-state columns 22 .. 45, in that order)
  processModel       :733-746                   f = m_acc - b_a, acc = Ma f, w = m_gyro - As acc - b_g, gyro = Tg w, and the same from
                                                m_gyro_old / m_acc_old
  calPhiClosedForm   :4016-4037                 the left / LARVIO bias blocks with Tg, TA = Tg As, Ma
                     :4039-4305                 the 24 intrinsic blocks Phi[0:9, 22:46]
The Euler forms and the right closed form write no intrinsic block (:3952-3978, :4308-4367): their Phi is mirror_imu's 15 x 15 inside
a 46 x 46 identity; only the measurement in front of them changes.

The mirror is the tests' reference for the imu_*46 functions of orcvio_amd/csrc/host/imu_model.hpp and for k_imu_phi_q46; it shares
no code with either.
"""
from __future__ import annotations

import numpy as np

import mirror_imu as mi
from mirror_imu import mm, mv, skew

LEG = 46
REC = 55   # a sample's record as imu_propagate_mean46 leaves it (imu_model.hpp, IMU_REC_*)

IDENTITY_INTRINSICS = np.array([0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1], float)   # T2 = M2 = 1


def intrinsic_matrices(x):
    T1, T2, T3, A1, A2, A3, M1, M2 = [np.asarray(x[3 * i:3 * i + 3], float) for i in range(8)]
    Tg = np.array([[T2[0], T3[0], T3[1]], [T1[0], T2[1], T3[2]], [T1[1], T1[2], T2[2]]])
    As = np.array([[A2[0], A3[0], A3[1]], [A1[0], A2[1], A3[2]], [A1[1], A1[2], A2[2]]])
    Ma = np.array([[M2[0], 0.0, 0.0], [M1[0], M2[1], 0.0], [M1[1], M1[2], M2[2]]])
    return Tg, As, Ma


def pat_L(x):
    M = np.zeros((3, 3))
    M[1, 0] = x[0]; M[2, 1] = x[0]; M[2, 2] = x[1]
    return M


def pat_D(x):
    return np.diag(np.asarray(x, float))


def pat_U(x):
    M = np.zeros((3, 3))
    M[0, 0] = x[1]; M[0, 1] = x[2]; M[1, 2] = x[2]
    return M


class Server46(mi.Server):
    def __init__(self, cfg, state, intrinsics, **kw):
        super().__init__(cfg, state, **kw)
        self.x = np.array(intrinsics, float)
        self.Tg, self.As, self.Ma = intrinsic_matrices(self.x)

    def measurement(self, m_gyro, m_acc):
        f = m_acc - self.imu.ba
        acc = mv(self.Ma, f)
        w = m_gyro - mv(self.As, acc) - self.imu.bg
        gyro = mv(self.Tg, w)
        return f, w, acc, gyro

    def G(self):
        G = np.zeros((LEG, 12))
        G[:mi.LEG] = super().G()
        return G

    def phi_closed_left46(self, dt, f, w, acc, gyro, f_old, w_old, acc_old, gyro_old):
        c = self.cfg
        Tg, Ma = self.Tg, self.Ma
        Phi = np.eye(LEG)
        f_mid = (f + f_old) / 2
        acc_mid = (acc + acc_old) / 2
        w_mid = (w_old + w) / 2 + dt * np.cross(w_old, w) / 12
        aa = dt * (gyro_old + gyro) / 2 + dt * dt * np.cross(gyro_old, gyro) / 12
        Ah = skew(aa)
        C = self.old.R
        I3 = np.eye(3)
        TA = Tg @ self.As
        vk = self.fej_old.v if c.if_fej else self.old.v
        pk = self.fej_old.p if c.if_fej else self.old.p
        vk1 = self.fej_now.v if c.if_fej else self.imu.v
        pk1 = self.fej_now.p if c.if_fej else self.imu.p
        g = c.gravity
        Phi[0:3, 9:12] = -0.5 * C @ (2 * I3 + Ah) * dt @ Tg
        Phi[0:3, 12:15] = 0.5 * C @ (2 * I3 + Ah) * dt @ TA @ Ma
        Phi[3:6, 0:3] = -skew(vk1 - vk - g * dt)
        Phi[3:6, 9:12] = skew(-pk1 + pk + vk1 * dt - 0.5 * g * dt * dt) @ C + \
            skew(-0.5 * pk1 + 0.5 * pk + 0.5 * vk1 * dt - g * dt * dt / 6) @ C @ Ah
        Phi[3:6, 12:15] = -0.5 * C @ (2 * I3 + Ah) * dt @ Ma - Phi[3:6, 9:12] @ TA @ Ma
        Phi[6:9, 0:3] = -skew(pk1 - pk - vk * dt - 0.5 * g * dt * dt)
        Phi[6:9, 3:6] = I3 * dt
        Phi[6:9, 9:12] = -dt * dt * dt * skew(g) @ C / 6 + dt * skew(pk1 - pk - g * dt * dt / 6) @ C @ Ah / 4
        Phi[6:9, 12:15] = -C @ (3 * I3 + Ah) * dt * dt / 6 @ Ma - Phi[6:9, 9:12] @ TA @ Ma
        # ---- :4039-4305
        R_mid = I3 + 0.5 * Ah
        R_kp1 = I3 + Ah
        Sm = skew(R_mid @ acc_mid)
        Sp = skew(R_kp1 @ acc)
        Z = np.zeros((3, 3))
        col = 22
        # (pattern, old / mid / new vector, factor in front, sign of the theta block, sign of the v and p blocks, direct velocity term)
        families = [(pat, (w_old, w_mid, w), I3, 1.0, -1.0, False) for pat in (pat_L, pat_D, pat_U)] + \
                   [(pat, (acc_old, acc_mid, acc), Tg, -1.0, 1.0, False) for pat in (pat_L, pat_D, pat_U)] + \
                   [(pat, (f_old, f_mid, f), TA, -1.0, 1.0, True) for pat in (pat_L, pat_D)]
        for pat, (xo, xm, xn), L, sq, sv, direct in families:
            X_k, X_kh, X_kp1 = pat(xo), pat(xm), pat(xn)
            kq1 = L @ X_k
            kq2 = R_mid @ L @ X_kh
            kq4 = R_kp1 @ L @ X_kp1
            Rq = dt * (kq1 + 4 * kq2 + kq4) / 6
            Phi[0:3, col:col + 3] = sq * C @ Rq
            kv1 = X_k if direct else Z
            kv2 = (R_mid @ X_kh if direct else Z) + Sm * dt @ kq1 / 2
            kv3 = (R_mid @ X_kh if direct else Z) + Sm * dt @ kq2 / 2
            kv4 = (R_kp1 @ X_kp1 if direct else Z) + Sp @ Rq
            fR = dt * (kv1 + 2 * kv2 + 2 * kv3 + kv4) / 6
            Phi[3:6, col:col + 3] = sv * C @ fR
            kp1 = Z
            kp2 = dt * kv1 / 2
            kp3 = dt * kv2 / 2
            kp4 = fR
            Phi[6:9, col:col + 3] = sv * C * dt @ (kp1 + 2 * kp2 + 2 * kp3 + kp4) / 6
            col += 3
        return Phi

    def process_model(self, time, m_gyro, m_acc):
        c = self.cfg
        f, w, acc, gyro = self.measurement(m_gyro, m_acc)
        f_old, w_old, acc_old, gyro_old = self.measurement(self.m_gyro_old, self.m_acc_old)
        dt = time - self.imu.time
        vk = (self.fej_now.v if c.if_fej else self.imu.v).copy()   # (the predictor rolls the FEJ pair: fej_old <- fej_now)
        pk = (self.fej_now.p if c.if_fej else self.imu.p).copy()
        R_old = self.imu.R.copy()
        if not c.use_larvio:
            self.predict_orcvio(dt, gyro, acc)
        else:
            self.predict_larvio(dt, gyro, acc)
        if c.use_larvio or c.use_closed_form:
            if c.use_larvio or c.use_left:
                Phi = self.phi_closed_left46(dt, f, w, acc, gyro, f_old, w_old, acc_old, gyro_old)
            else:
                Phi = np.eye(LEG)
                Phi[:mi.LEG, :mi.LEG] = self.phi_closed(dt, acc, gyro, gyro_old)
        else:
            Phi = np.eye(LEG)
            Phi[:mi.LEG, :mi.LEG] = self.phi_euler(dt, acc, gyro)
        G = self.G()
        with np.errstate(invalid='ignore'):
            Q = Phi @ G @ c.Qc @ G.T @ Phi.T * dt
            if self.P is not None:
                P = self.P
                P[:LEG, :LEG] = Phi @ P[:LEG, :LEG] @ Phi.T + Q
                if P.shape[0] > LEG:
                    P[:LEG, LEG:] = Phi @ P[:LEG, LEG:]
                    P[LEG:, :LEG] = P[LEG:, :LEG] @ Phi.T
                self.P = (P + P.T) / 2.0
        self.imu.time = time
        self.fej_now.time = time
        rec = np.concatenate([[dt], gyro, acc, gyro_old, R_old.ravel(), self.imu.R.ravel(), vk, pk, self.imu.v, self.imu.p,
                              f, w, f_old, w_old, acc_old])
        self.steps.append(dict(Phi=Phi, Q=Q, dt=dt, R=self.imu.R.copy(), v=self.imu.v.copy(), p=self.imu.p.copy(), rec=rec))


def accumulate_sequential(steps):
    Phi, Q = np.eye(LEG), np.zeros((LEG, LEG))
    for s in steps:
        Q = s['Phi'] @ Q @ s['Phi'].T + s['Q']
        Phi = s['Phi'] @ Phi
    return Phi, Q


def accumulate_pairwise(steps):
    items = [(s['Phi'], s['Q']) for s in steps]
    if not items:
        return np.eye(LEG), np.zeros((LEG, LEG))
    while len(items) > 1:
        nxt = []
        for i in range(0, len(items) - 1, 2):
            (Pa, Qa), (Pb, Qb) = items[i], items[i + 1]
            nxt.append((Pb @ Pa, Pb @ Qa @ Pb.T + Qb))
        if len(items) & 1:
            nxt.append(items[-1])
        items = nxt
    return items[0]


def apply_once(P, Phi, Q):
    """What the library's propagation does with the accumulated pair at leg_dim = 46: one application, the IMU block symmetrised."""
    P = np.array(P, float)
    T = Phi @ P[:LEG, :]
    out = P.copy()
    A = T[:, :LEG] @ Phi.T + Q
    out[:LEG, :LEG] = 0.5 * (A + A.T)
    out[:LEG, LEG:] = T[:, LEG:]
    out[LEG:, :LEG] = T[:, LEG:].T
    return out
