"""numpy restatement of the reference's IMU step at leg_dim = 22 (calib_imu off: Tg = Ma = I, As = 0), written from the reference:

  batchImuProcessing      src/orcvio.cpp:664-724   sample selection, dt to the image, mean specific force
  processModel            :727-823                 unbiased measurement, predictor, Phi, G, Q, three products against P, (P + P^T)/2
  predictNewStateLARVIO   :825-897                 quaternion RK4
  predictNewStateOrcVIO   :899-928                 Jl / Hl closed form
  calPhiEulerMethod       :3952-3978
  calPhiClosedForm        :3980-4037 (left / LARVIO), :4308-4367 (right)
  Jl_operator, Hl_operator, rotationToQuaternion, quaternionToRotation   include/orcvio/utils/math_utils.hpp:164-270

The mirror is the tests' reference for orcvio_amd/csrc/host/imu_model.hpp and k_imu_phi_q; it shares no code with either.
"""
from __future__ import annotations

import copy
import dataclasses
import math

import numpy as np

LEG = 22


# The predictors are written in scalar IEEE double operations in the reference's own order -- Eigen evaluates a fixed-size 3 x 3
# product coefficient by coefficient as a sum of three products, without BLAS and (on the reference's baseline x86-64 build) without
# fused multiply-adds; libm's sin / cos / pow through the math module.  The formulas of Phi subtract nearly equal positions
# (p_k+1 - p_k - v_k dt - g dt^2 / 2), so ONE ulp in the propagated position is 1e-13 of a block of Phi: numpy's BLAS-backed `@`
# (FMA kernels, unspecified summation order) is kept out of the state's path.
def mm(A, B):
    return A[:, [0]] * B[[0], :] + A[:, [1]] * B[[1], :] + A[:, [2]] * B[[2], :]


def mv(A, x):
    return A[:, 0] * x[0] + A[:, 1] * x[1] + A[:, 2] * x[2]


def norm3(w):
    return math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])


def norm4(q):
    return math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def quaternion_to_rotation(q):
    qx, qy, qz, qw = q
    return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                     [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                     [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])


def rotation_to_quaternion(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    score = np.array([R[0, 0], R[1, 1], R[2, 2], tr])
    m = int(np.argmax(score))
    q = np.zeros(4)
    if m == 0:
        q[0] = math.sqrt(1 + 2 * R[0, 0] - tr) / 2.0
        q[1] = (R[0, 1] + R[1, 0]) / (4 * q[0])
        q[2] = (R[0, 2] + R[2, 0]) / (4 * q[0])
        q[3] = (R[2, 1] - R[1, 2]) / (4 * q[0])
    elif m == 1:
        q[1] = math.sqrt(1 + 2 * R[1, 1] - tr) / 2.0
        q[0] = (R[0, 1] + R[1, 0]) / (4 * q[1])
        q[2] = (R[1, 2] + R[2, 1]) / (4 * q[1])
        q[3] = (R[0, 2] - R[2, 0]) / (4 * q[1])
    elif m == 2:
        q[2] = math.sqrt(1 + 2 * R[2, 2] - tr) / 2.0
        q[0] = (R[0, 2] + R[2, 0]) / (4 * q[2])
        q[1] = (R[1, 2] + R[2, 1]) / (4 * q[2])
        q[3] = (R[1, 0] - R[0, 1]) / (4 * q[2])
    else:
        q[3] = math.sqrt(1 + tr) / 2.0
        q[0] = (R[2, 1] - R[1, 2]) / (4 * q[3])
        q[1] = (R[0, 2] - R[2, 0]) / (4 * q[3])
        q[2] = (R[1, 0] - R[0, 1]) / (4 * q[3])
    if q[3] < 0:
        q = -q
    return q / norm4(q)


def eigen_quat_to_matrix(w, x, y, z):
    """Eigen::Quaterniond(w, x, y, z).toRotationMatrix(): no normalisation."""
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def so3_exp(w):
    """Sophus SO3d::exp: unit quaternion of the rotation vector, then its matrix."""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = math.sqrt(th2)
    if th < 1e-10:
        th4 = th2 * th2
        imag = 0.5 - th2 / 48.0 + th4 / 3840.0
        real = 1.0 - th2 / 8.0 + th4 / 384.0
    else:
        imag = math.sin(0.5 * th) / th
        real = math.cos(0.5 * th)
    return eigen_quat_to_matrix(real, imag * w[0], imag * w[1], imag * w[2])


def Hl_operator(g):
    n = norm3(g)
    t1 = 0.5 * np.eye(3)
    if n < 1.0e-5:
        return t1
    S = skew(g)
    t2 = ((n - math.sin(n)) / n ** 3) * S
    t3 = ((2 * (math.cos(n) - 1) + n ** 2) / (2 * n ** 4)) * mm(S, S)
    return t1 + t2 + t3


def Jl_operator(g):
    n = norm3(g)
    t1 = np.eye(3)
    if n < 1.0e-5:
        return t1
    S = skew(g)
    t2 = ((1 - math.cos(n)) / n ** 2) * S
    t3 = mm(((n - math.sin(n)) / n ** 3) * S, S)   # (scalar * skew * skew, left to right)
    return t1 + t2 + t3


@dataclasses.dataclass
class Config:
    use_larvio: bool = True
    use_left: bool = False
    use_closed_form: bool = True
    if_fej: bool = False
    gravity: np.ndarray = dataclasses.field(default_factory=lambda: np.array([0.0, 0.0, -9.81]))
    imu_img_time_th: float = 1.0 / 400.0
    Qc: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(12))


@dataclasses.dataclass
class ImuState:
    time: float = 0.0
    R: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(3))   # orientation, body to world
    v: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(3))
    p: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(3))
    bg: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(3))
    ba: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(3))

    def copy(self):
        return copy.deepcopy(self)


class Server:
    """state_server's IMU part: imu_state, imu_state_old, the FEJ pair, m_gyro_old / m_acc_old and state_cov."""

    def __init__(self, cfg: Config, state: ImuState, P=None, fej_now: ImuState = None, m_gyro_old=None, m_acc_old=None):
        self.cfg = cfg
        self.imu = state.copy()
        self.old = state.copy()
        self.fej_now = (fej_now or state).copy()
        self.fej_old = self.fej_now.copy()
        self.m_gyro_old = np.zeros(3) if m_gyro_old is None else np.array(m_gyro_old, float)
        self.m_acc_old = np.zeros(3) if m_acc_old is None else np.array(m_acc_old, float)
        self.P = None if P is None else np.array(P, float)
        self.steps = []   # per processed sample: dict(Phi, Q, state)

    # ---- predictors
    def predict_larvio(self, dt, gyro, acc):
        g = self.cfg.gravity
        gn = norm3(gyro)
        Om = np.zeros((4, 4))
        Om[:3, :3] = -skew(gyro)
        Om[:3, 3] = gyro
        Om[3, :3] = -gyro
        self.old = self.imu.copy()
        q = rotation_to_quaternion(self.imu.R)
        v, p = self.imu.v, self.imu.p
        I4 = np.eye(4)
        def mv4(M):
            return M[:, 0] * q[0] + M[:, 1] * q[1] + M[:, 2] * q[2] + M[:, 3] * q[3]
        if gn > 1e-5:
            dq_dt = mv4(math.cos(gn * dt * 0.5) * I4 + 1 / gn * math.sin(gn * dt * 0.5) * Om)
            dq_dt2 = mv4(math.cos(gn * dt * 0.25) * I4 + 1 / gn * math.sin(gn * dt * 0.25) * Om)
        else:
            dq_dt = mv4((I4 + 0.5 * dt * Om) * math.cos(gn * dt * 0.5))
            dq_dt2 = mv4((I4 + 0.25 * dt * Om) * math.cos(gn * dt * 0.25))
        dR_dt = eigen_quat_to_matrix(dq_dt[3], dq_dt[0], dq_dt[1], dq_dt[2])
        dR_dt2 = eigen_quat_to_matrix(dq_dt2[3], dq_dt2[0], dq_dt2[1], dq_dt2[2])
        k1_v_dot = mv(eigen_quat_to_matrix(q[3], q[0], q[1], q[2]), acc) + g
        k1_p_dot = v
        k1_v = v + k1_v_dot * dt / 2
        k2_v_dot = mv(dR_dt2, acc) + g
        k2_p_dot = k1_v
        k2_v = v + k2_v_dot * dt / 2
        k3_v_dot = mv(dR_dt2, acc) + g
        k3_p_dot = k2_v
        k3_v = v + k3_v_dot * dt
        k4_v_dot = mv(dR_dt, acc) + g
        k4_p_dot = k3_v
        q = dq_dt / norm4(dq_dt)
        self.imu.v = v + dt / 6 * (k1_v_dot + 2 * k2_v_dot + 2 * k3_v_dot + k4_v_dot)
        self.imu.p = p + dt / 6 * (k1_p_dot + 2 * k2_p_dot + 2 * k3_p_dot + k4_p_dot)
        self.imu.R = quaternion_to_rotation(q)
        self.fej_old = self.fej_now.copy()
        self.fej_now = self.imu.copy()

    def predict_orcvio(self, dt, gyro, acc):
        g = self.cfg.gravity
        self.old = self.imu.copy()
        R, v, p = self.imu.R, self.imu.v, self.imu.p
        Hl = Hl_operator(dt * gyro)
        p = p + dt * v + g * (dt ** 2 / 2) + mv(mm(R, Hl), acc) * dt ** 2
        Jl = Jl_operator(dt * gyro)
        v = v + g * dt + mv(mm(R, Jl), acc) * dt
        R = mm(R, so3_exp(dt * gyro))
        self.imu.R, self.imu.v, self.imu.p = R, v, p
        self.fej_old = self.fej_now.copy()
        self.fej_now = self.imu.copy()

    # ---- Phi
    def phi_euler(self, dt, acc, gyro):
        wRi = self.imu.R   # (AFTER the predictor, :3955)
        Phi = np.eye(LEG)
        if self.cfg.use_left:
            Phi[0:3, 9:12] = -dt * wRi
            Phi[3:6, 0:3] = -dt * skew(wRi @ acc)
            Phi[3:6, 12:15] = -dt * wRi
            Phi[6:9, 3:6] = dt * np.eye(3)
        else:
            Phi[0:3, 0:3] = np.eye(3) - dt * skew(gyro)
            Phi[0:3, 9:12] = -dt * np.eye(3)
            Phi[3:6, 0:3] = -dt * wRi @ skew(acc)
            Phi[3:6, 12:15] = -dt * wRi
            Phi[6:9, 3:6] = dt * np.eye(3)
        return Phi

    def phi_closed(self, dt, acc, gyro, gyro_old):
        c = self.cfg
        Phi = np.eye(LEG)
        aa = dt * (gyro_old + gyro) / 2 + dt * dt * np.cross(gyro_old, gyro) / 12
        Ah = skew(aa)
        C = self.old.R
        I3 = np.eye(3)
        if c.use_larvio or c.use_left:
            vk = self.fej_old.v if c.if_fej else self.old.v
            pk = self.fej_old.p if c.if_fej else self.old.p
            vk1 = self.fej_now.v if c.if_fej else self.imu.v
            pk1 = self.fej_now.p if c.if_fej else self.imu.p
            g = c.gravity
            Phi[0:3, 9:12] = -0.5 * C @ (2 * I3 + Ah) * dt
            Phi[0:3, 12:15] = 0.0   # (TA = Tg As = 0)
            Phi[3:6, 0:3] = -skew(vk1 - vk - g * dt)
            Phi[3:6, 9:12] = skew(-pk1 + pk + vk1 * dt - 0.5 * g * dt * dt) @ C + \
                skew(-0.5 * pk1 + 0.5 * pk + 0.5 * vk1 * dt - g * dt * dt / 6) @ C @ Ah
            Phi[3:6, 12:15] = -0.5 * C @ (2 * I3 + Ah) * dt
            Phi[6:9, 0:3] = -skew(pk1 - pk - vk * dt - 0.5 * g * dt * dt)
            Phi[6:9, 3:6] = I3 * dt
            Phi[6:9, 9:12] = -dt * dt * dt * skew(g) @ C / 6 + dt * skew(pk1 - pk - g * dt * dt / 6) @ C @ Ah / 4
            Phi[6:9, 12:15] = -C @ (3 * I3 + Ah) * dt * dt / 6
        else:
            wRi = C
            a_skew = skew(acc)
            g_skew = skew(gyro)
            gn = np.linalg.norm(gyro)
            with np.errstate(divide='ignore', invalid='ignore'):
                gn2 = np.float64(gn) ** 2
                theta_theta = so3_exp(-dt * gyro)
                JLp = Jl_operator(dt * gyro)
                JLm = Jl_operator(-dt * gyro)
                Delta = -(g_skew / gn2) @ (theta_theta.T @ (dt * g_skew - I3) + I3)
                HLp = Hl_operator(dt * gyro)
                HLm = Hl_operator(-dt * gyro)
                theta_gyro = -dt * JLm
                v_theta = -dt * wRi @ skew(JLp @ acc)
                ga = np.outer(gyro, acc)
                v_gyro = wRi @ Delta @ a_skew @ (I3 + (g_skew @ g_skew / gn2)) + dt * wRi @ JLp @ (a_skew @ g_skew / gn2) + \
                    dt * wRi @ (ga / gn2) @ JLm - dt * (float(acc @ gyro) / gn2) * I3
                v_acc = -dt * wRi @ JLp
                p_theta = -dt ** 2 * wRi @ skew(HLp @ acc)
                p_v = dt * I3
                p_gyro = wRi @ (-g_skew @ Delta - dt * JLp + dt * I3) @ a_skew @ (I3 + (g_skew @ g_skew / gn2)) @ (g_skew / gn2) + \
                    dt ** 2 * wRi @ HLp @ (a_skew @ g_skew / gn2) + dt ** 2 * wRi @ (ga / gn2) @ HLm - \
                    dt ** 2 * (float(acc @ gyro) / (2 * gn2)) * wRi
                p_acc = -dt ** 2 * wRi @ HLp
            Phi[0:3, 0:3] = theta_theta
            Phi[0:3, 9:12] = theta_gyro
            Phi[3:6, 0:3] = v_theta
            Phi[3:6, 9:12] = v_gyro
            Phi[3:6, 12:15] = v_acc
            Phi[6:9, 0:3] = p_theta
            Phi[6:9, 3:6] = p_v
            Phi[6:9, 9:12] = p_gyro
            Phi[6:9, 12:15] = p_acc
        return Phi

    def G(self):
        C = self.old.R
        G = np.zeros((LEG, 12))
        if self.cfg.use_larvio or self.cfg.use_left:
            G[0:3, 0:3] = -C
        else:
            G[0:3, 0:3] = -np.eye(3)
        G[3:6, 3:6] = -C
        G[9:12, 6:9] = np.eye(3)
        G[12:15, 9:12] = np.eye(3)
        return G

    # ---- processModel
    def process_model(self, time, m_gyro, m_acc):
        c = self.cfg
        acc = m_acc - self.imu.ba
        gyro = m_gyro - self.imu.bg
        gyro_old = self.m_gyro_old - self.imu.bg
        dt = time - self.imu.time
        if not c.use_larvio:
            self.predict_orcvio(dt, gyro, acc)
        else:
            self.predict_larvio(dt, gyro, acc)
        if c.use_larvio or c.use_closed_form:
            Phi = self.phi_closed(dt, acc, gyro, gyro_old)
        else:
            Phi = self.phi_euler(dt, acc, gyro)
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
        self.steps.append(dict(Phi=Phi, Q=Q, dt=dt, R=self.imu.R.copy(), v=self.imu.v.copy(), p=self.imu.p.copy()))

    # ---- batchImuProcessing
    def batch(self, time_bound, samples):
        """samples: rows [t, gyro 3, acc 3].  Returns dict(n_used, n_propagated, dt, mean_sforce)."""
        used = 0
        msum = np.zeros(3)
        counter = 0
        dt = 0.0
        for row in samples:
            t = float(row[0])
            if t <= self.imu.time:
                used += 1
                continue
            if t - time_bound > self.cfg.imu_img_time_th:
                break
            dt = t - time_bound
            m_gyro, m_acc = np.array(row[1:4], float), np.array(row[4:7], float)
            self.process_model(t, m_gyro, m_acc)
            used += 1
            self.m_gyro_old, self.m_acc_old = m_gyro, m_acc
            msum = msum + m_acc
            counter += 1
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = msum / np.float64(counter)
        return dict(n_used=used, n_propagated=counter, dt=dt, mean_sforce=mean)


def accumulate_sequential(steps):
    """Phi = Phi_S ... Phi_1, Q <- Phi_k Q Phi_k^T + Q_k, one sample after the other."""
    Phi, Q = np.eye(LEG), np.zeros((LEG, LEG))
    for s in steps:
        Q = s['Phi'] @ Q @ s['Phi'].T + s['Q']
        Phi = s['Phi'] @ Phi
    return Phi, Q


def accumulate_pairwise(steps):
    """The same ordered product as a balanced tree of (Phi_b, Q_b) o (Phi_a, Q_a) = (Phi_b Phi_a, Phi_b Q_a Phi_b^T + Q_b)."""
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
    """What the library's propagation does with the accumulated pair (cov_ops.hpp): one application, the IMU block symmetrised."""
    P = np.array(P, float)
    T = Phi @ P[:LEG, :]
    out = P.copy()
    A = T[:, :LEG] @ Phi.T + Q
    out[:LEG, :LEG] = 0.5 * (A + A.T)
    out[:LEG, LEG:] = T[:, LEG:]
    out[LEG:, :LEG] = T[:, LEG:].T
    return out
