"""numpy mirror of the check of the clones that leave (orcvio_msckf_io_choose_clones, host/clone_choice_model.hpp): the reference's
findRedundantImuStates (src/orcvio.cpp:2582-2626) on position_cam / orientation_cam as incrementState_IMUCam rewrites them
(:4535-4565), and the same formulas in 60-digit arithmetic (mpmath).  `mutation`: the mistakes tests/test_clone_choice_mirror.py shows
the case set can see."""
import numpy as np

MUTATIONS = ('back_to_key', 'back_to_same', 'R_times_K', 'frozen_extrinsic', 'pre_update_poses', 'unsorted', 'tracking_ignored')


def so3_exp(w):
    """Sophus v1.0.0 SO3d::exp: the unit quaternion of the rotation vector, then its matrix."""
    w = np.asarray(w, dtype=np.float64)
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-10:
        imag, real = 0.5 - th2 / 48.0 + th2 * th2 / 3840.0, 1.0 - th2 / 8.0 + th2 * th2 / 384.0
    else:
        imag, real = np.sin(0.5 * th) / th, np.cos(0.5 * th)
    x, y, z, q = imag * w[0], imag * w[1], imag * w[2], real
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * q), 2 * (x * z + y * q)],
                     [2 * (x * y + z * q), 1 - 2 * (x * x + z * z), 2 * (y * z - x * q)],
                     [2 * (x * z - y * q), 2 * (y * z + x * q), 1 - 2 * (x * x + y * y)]])


def extrinsic_increment(de, R, t):
    """smallAngleQuaternion (math_utils.hpp:104-121), R <- R Rq^T without normalisation, t += de[3:6] (:4512-4517)."""
    q = np.array([0.5 * de[0], 0.5 * de[1], 0.5 * de[2], 0.0])
    n2 = float(q[:3] @ q[:3])
    if n2 <= 1.0:
        q[3] = np.sqrt(1.0 - n2)
    else:
        q[3] = 1.0
        q = q / np.sqrt(1.0 + n2)
    x, y, z, w = q
    RqT = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w)],
                    [2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w)],
                    [2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)]])
    return R @ RqT, np.asarray(t, dtype=np.float64) + np.asarray(de[3:6], dtype=np.float64)


def applies(dx, apply_dx, discard_large):
    if not apply_dx:
        return False
    if discard_large and (np.linalg.norm(dx[3:6]) > 1.0 or np.linalg.norm(dx[6:9]) > 1.5):
        return False
    return True


def cam_records(R_b2w, t_b_w, R_ext, t_ext):
    """[N][12] orientation_cam (row-major) | position_cam from body poses and ONE extrinsic, or per-clone extrinsics [N,3,3] / [N,3]"""
    N = len(R_b2w)
    R_ext = np.broadcast_to(R_ext, (N, 3, 3))
    t_ext = np.broadcast_to(t_ext, (N, 3))
    out = np.empty((N, 12))
    for c in range(N):
        out[c, :9] = (R_b2w[c] @ R_ext[c].T).ravel()
        out[c, 9:] = t_b_w[c] + R_b2w[c] @ t_ext[c]
    return out


def cam_after(w, dx, ext, left, mutation=None):
    """the records after incrementState_IMUCam with dx: body poses incremented (left / right), the IMU's extrinsic ext = (R, t)
    incremented by dx[15:21]"""
    leg, N = w.flags.leg_dim, w.N
    R = np.empty((N, 3, 3)); t = np.empty((N, 3))
    for c in range(N):
        da = dx[leg + 6 * c: leg + 6 * c + 6]
        E = so3_exp(da[:3])
        R[c] = E @ w.R_b2w[c] if left else w.R_b2w[c] @ E
        t[c] = w.t_b_w[c] + da[3:]
    if mutation == 'frozen_extrinsic':
        return cam_records(R, t, w.R_b2c, w.t_c_b)
    Re, te = extrinsic_increment(dx[15:21], ext[0], ext[1])
    return cam_records(R, t, Re, te)


def quat_angle(M):
    """Eigen 3.3 AngleAxisd(Matrix3d).angle(): the quaternion of the matrix, 2 atan2(|vec|, |w|)"""
    t = M[0, 0] + M[1, 1] + M[2, 2]
    v = np.zeros(3)
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        v[:] = [(M[2, 1] - M[1, 2]) * t, (M[0, 2] - M[2, 0]) * t, (M[1, 0] - M[0, 1]) * t]
    else:
        i = 0
        if M[1, 1] > M[0, 0]:
            i = 1
        if M[2, 2] > M[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(M[i, i] - M[j, j] - M[k, k] + 1.0)
        v[i] = 0.5 * t
        t = 0.5 / t
        w = (M[k, j] - M[j, k]) * t
        v[j] = (M[j, i] + M[i, j]) * t
        v[k] = (M[k, i] + M[i, k]) * t
    return 2.0 * np.arctan2(np.sqrt(v @ v), abs(w))


def quantities(cam, c, key, mutation=None):
    Rc, Rk = cam[c, :9].reshape(3, 3), cam[key, :9].reshape(3, 3)
    M = Rc @ Rk if mutation == 'R_times_K' else Rc.T @ Rk
    return quat_angle(M), float(np.linalg.norm(cam[c, 9:] - cam[key, 9:]))


def choose(cam, rot_thr, trans_thr, tracking_ok, mutation=None):
    """the loop on records [N][12]; dict(chosen (ascending), compared, taken, angle, distance)"""
    N = len(cam)
    key, c, first = N - 4, N - 3, 0
    out = dict(chosen=[], compared=[], taken=[], angle=[], distance=[])
    for _ in range(2):
        a, d = quantities(cam, c, key, mutation)
        take = a < rot_thr and d < trans_thr and (bool(tracking_ok) or mutation == 'tracking_ignored')
        out['compared'].append(c); out['taken'].append(int(take)); out['angle'].append(a); out['distance'].append(d)
        if take:
            out['chosen'].append(c); c += 1
        else:
            out['chosen'].append(first); first += 1
            c -= {'back_to_key': 1, 'back_to_same': 0}.get(mutation, 2)
    if mutation != 'unsorted':
        out['chosen'].sort()
    return out


def evaluate(case, dx, applied, mutation=None):
    """what the device reports for a case of clone_choice_cases: on dx when `applied`, else on the records handed over"""
    cam = case['cam_pre']
    if applied and mutation != 'pre_update_poses':
        cam = cam_after(case['w'], dx, case['ext'], case['left'], mutation)
    out = choose(cam, case['rot_thr'], case['trans_thr'], case['tracking_ok'], mutation)
    out['agree'] = int(list(out['chosen']) == list(case['predicted']))
    return out


# ---- the same formulas in 60 digits ------------------------------------------------------------------------------------------------------
def quantities_mp(w, dx, ext, left, c, key, applied, cam_pre):
    """(angle, distance) of clone c against the key from the SAME double inputs, every operation in 60 digits"""
    import mpmath as mp
    mp.mp.dps = 60
    M = lambda A: mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(A, dtype=np.float64).reshape(3, 3)])
    V = lambda a: mp.matrix([mp.mpf(float(x)) for x in a])

    def exp(wv):
        wv = V(wv)
        th2 = wv[0] ** 2 + wv[1] ** 2 + wv[2] ** 2
        th = mp.sqrt(th2)
        if th == 0:
            return mp.eye(3)
        x, y, z = [mp.sin(th / 2) / th * wv[i] for i in range(3)]
        q = mp.cos(th / 2)
        return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - z * q), 2 * (x * z + y * q)],
                          [2 * (x * y + z * q), 1 - 2 * (x * x + z * z), 2 * (y * z - x * q)],
                          [2 * (x * z - y * q), 2 * (y * z + x * q), 1 - 2 * (x * x + y * y)]])

    def record(i):
        if not applied:
            return M(cam_pre[i, :9]), V(cam_pre[i, 9:])
        leg = w.flags.leg_dim
        da = dx[leg + 6 * i: leg + 6 * i + 6]
        E = exp(da[:3])
        R = E * M(w.R_b2w[i]) if left else M(w.R_b2w[i]) * E
        t = V(w.t_b_w[i]) + V(da[3:])
        de = V(dx[15:21])
        q = [de[0] / 2, de[1] / 2, de[2] / 2]
        n2 = q[0] ** 2 + q[1] ** 2 + q[2] ** 2
        if n2 <= 1:
            qw = mp.sqrt(1 - n2)
        else:
            s = 1 / mp.sqrt(1 + n2)
            q = [v * s for v in q]; qw = s
        x, y, z = q
        RqT = mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y + z * qw), 2 * (x * z - y * qw)],
                         [2 * (x * y - z * qw), 1 - 2 * (x * x + z * z), 2 * (y * z + x * qw)],
                         [2 * (x * z + y * qw), 2 * (y * z - x * qw), 1 - 2 * (x * x + y * y)]])
        Re = M(ext[0]) * RqT
        te = V(ext[1]) + V(dx[18:21])
        return R * Re.T, t + R * te

    (Rc, pc), (Rk, pk) = record(c), record(key)
    Mx = Rc.T * Rk
    t = Mx[0, 0] + Mx[1, 1] + Mx[2, 2]
    assert t > 0   # (every case of the set: angles far below pi / 2)
    t = mp.sqrt(t + 1)
    qw = t / 2
    t = 1 / (2 * t)
    v = [(Mx[2, 1] - Mx[1, 2]) * t, (Mx[0, 2] - Mx[2, 0]) * t, (Mx[1, 0] - Mx[0, 1]) * t]
    angle = 2 * mp.atan2(mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2), abs(qw))
    d = pc - pk
    return float(angle), float(mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2))
