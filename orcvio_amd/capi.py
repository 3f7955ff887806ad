"""ctypes binding of the C-ABI in include/orcvio_msckf.h (plumbing only).

The library is built in-tree by ``__graft_entry__.build()`` /
``orcvio_amd.build.build_library()`` into ``orcvio_amd/lib/liborcvio_msckf.so``.
There is no CPU fallback: if the shared object is missing, or no gfx950 device is
visible, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'liborcvio_msckf.so')
LIB_DBG_PATH = os.path.join(_HERE, 'lib', 'liborcvio_msckf_dbg.so')   # diagnostics build: + orcvio_msckf_debug_* (tests only)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

STATUS = {0: 'OK', 1: 'ERR_INVALID', 2: 'ERR_NO_DEVICE', 3: 'ERR_CAPACITY', 4: 'ERR_TRACK_TOO_LONG',
          5: 'ERR_HIP', 6: 'ERR_NOT_SPD', 7: 'ERR_TIMEOUT', 8: 'ERR_PEER'}

# every symbol include/orcvio_msckf.h declares (checked by tests/test_abi.py)
EXPORTS = [
    'orcvio_msckf_abi_version', 'orcvio_msckf_last_error', 'orcvio_msckf_chi2_quantile',
    'orcvio_msckf_create', 'orcvio_msckf_destroy', 'orcvio_msckf_update_features',
    'orcvio_msckf_update_objects', 'orcvio_msckf_upload', 'orcvio_msckf_run_local',
    'orcvio_msckf_block_ptr', 'orcvio_msckf_run_finish', 'orcvio_msckf_run_update',
    'orcvio_msckf_sync', 'orcvio_msckf_download', 'orcvio_msckf_profile_update',
    'orcvio_msckf_increment_state', 'orcvio_msckf_set_option', 'orcvio_msckf_run_local_to',
    'orcvio_msckf_object_rows_eval', 'orcvio_msckf_object_lm', 'orcvio_msckf_object_lm_config_default',
    'orcvio_msckf_object_init', 'orcvio_msckf_object_init_lm', 'orcvio_msckf_object_init_config_default', 'orcvio_msckf_triangulation_config_default', 'orcvio_msckf_triangulate',
    'orcvio_msckf_object_init_lite', 'orcvio_msckf_object_lm_lite', 'orcvio_msckf_object_init_lm_lite', 'orcvio_msckf_object_lite_config_default',
    'orcvio_msckf_object_init_lite_config_default',
    'orcvio_msckf_triangulate_uploaded', 'orcvio_msckf_objects_local', 'orcvio_msckf_objects_finish',
    'orcvio_msckf_objects_download', 'orcvio_msckf_cov_set', 'orcvio_msckf_cov_get', 'orcvio_msckf_cov_propagate',
    'orcvio_msckf_cov_augment', 'orcvio_msckf_cov_remove_clones', 'orcvio_msckf_cov_commit', 'orcvio_msckf_cov_prefactor', 'orcvio_msckf_upload_new_features', 'orcvio_msckf_download_new_feature_blocks', 'orcvio_msckf_upload_nuisance_poses',
    'orcvio_msckf_augment_state_nuisance', 'orcvio_msckf_cov_clones_to_nuisance', 'orcvio_msckf_cov_commit_new_features',
    'orcvio_msckf_cov_commit_new_features_fac',
    'orcvio_msckf_update_object_tracks', 'orcvio_msckf_objects_local_tracks',
    'orcvio_msckf_upload_ekf_rows', 'orcvio_msckf_download_ekf', 'orcvio_msckf_upload_slam_features', 'orcvio_msckf_upload_dense_rows', 'orcvio_msckf_augment_new_features', 'orcvio_msckf_gate_tracks', 'orcvio_msckf_new_feature_rows', 'orcvio_msckf_augment_state',
    'orcvio_msckf_profile_stages', 'orcvio_msckf_update_object_lm_msgs',
    'orcvio_msckf_comm_unique_id', 'orcvio_msckf_comm_init', 'orcvio_msckf_comm_destroy', 'orcvio_msckf_comm_info',
    'orcvio_msckf_run_update_sharded', 'orcvio_msckf_update_features_sharded', 'orcvio_msckf_update_object_tracks_sharded',
    'orcvio_msckf_comm_barrier', 'orcvio_msckf_comm_allreduce_max', 'orcvio_msckf_io_begin', 'orcvio_msckf_io_update',
    'orcvio_msckf_augment_state_ref_ldlt', 'orcvio_msckf_io_update_frame', 'orcvio_msckf_io_stage_object_tracks', 'orcvio_msckf_io_submit', 'orcvio_msckf_io_collect', 'orcvio_msckf_io_triangulate', 'orcvio_msckf_io_triangulate_prune', 'orcvio_msckf_io_choose_clones',
    'orcvio_msckf_objects_refined', 'orcvio_msckf_counters', 'orcvio_msckf_comm_details', 'orcvio_msckf_profile_sharded',
    'orcvio_msckf_io_step_frame', 'orcvio_msckf_io_step_frame_ex', 'orcvio_msckf_cov_remove_features', 'orcvio_msckf_cov_change_anchors',
    'orcvio_msckf_cov_zupt', 'orcvio_msckf_cov_zupt_frame', 'orcvio_msckf_cov_propagate_imu', 'orcvio_msckf_io_propagate_imu',
    'orcvio_msckf_zupt_check_default', 'orcvio_msckf_cov_zupt_check_imu', 'orcvio_msckf_cov_propagate_imu_checked',
    'orcvio_msckf_cov_zupt_frame_checked', 'orcvio_msckf_cov_propagate_imu_calib',
    'orcvio_msckf_cov_zupt_frame_hybrid', 'orcvio_msckf_cov_zupt_frame_checked_hybrid', 'orcvio_msckf_zupt_check_feat',
    'orcvio_msckf_cov_get_marginal', 'orcvio_msckf_cov_marginal_submit', 'orcvio_msckf_cov_marginal_collect',
]


class MsckfFlags(C.Structure):
    _fields_ = [('leg_dim', C.c_int32), ('use_larvio', C.c_int32), ('use_left_perturbation', C.c_int32),
                ('if_fej', C.c_int32), ('estimate_td', C.c_int32), ('discard_large_update', C.c_int32),
                ('noise_feature', C.c_double), ('chi2_prob', C.c_double)]


class MsckfWindow(C.Structure):
    _fields_ = [('n_clones', C.c_int32), ('R_b2w', _dp), ('t_b_w', _dp), ('t_fej', _dp), ('R_b2c', _dp), ('t_c_b', _dp)]


class MsckfTracks(C.Structure):
    _fields_ = [('n_features', C.c_int32), ('p_w', _dp), ('obs_ptr', _ip), ('obs_clone', _ip), ('obs_z', _dp),
                ('obs_zvel', _dp)]


class MsckfObjectRows(C.Structure):
    _fields_ = [('n_rows', C.c_int32), ('n_obj_cols', C.c_int32), ('row_clone', _ip), ('Hx6', _dp), ('Hf', _dp),
                ('res', _dp)]


class ObjectEvalFlags(C.Structure):
    _fields_ = [('use_left_perturbation', C.c_int32), ('use_new_bbox_residual', C.c_int32),
                ('vio_use_left_perturbation', C.c_int32), ('fix_dcampose_dimupose_to_identity', C.c_int32),
                ('R_b2c', C.c_double * 9), ('t_c_b', C.c_double * 3)]


class ObjectTrackC(C.Structure):
    _fields_ = [('n_keypoints', C.c_int32), ('n_frames', C.c_int32), ('wTo', _dp), ('shape', _dp), ('kps', _dp),
                ('frame_wTc', _dp), ('frame_zs', _dp), ('frame_bbox', _dp), ('frame_clone', _ip)]


class ObjectLMConfig(C.Structure):
    """orcvio_object_lm_config (include/orcvio_msckf.h)."""
    _fields_ = [('use_left_perturbation', C.c_int32), ('use_new_bbox_residual', C.c_int32), ('residual_weights', C.c_double * 4),
                ('max_iter', C.c_int32), ('ptol', C.c_double)]


class ObjectLMPrior(C.Structure):
    _fields_ = [('mean_shape', _dp), ('mean_kps', _dp)]


class ObjectLMResult(C.Structure):
    _fields_ = [('wTo', _dp), ('shape', _dp), ('kps', _dp), ('cost0', C.c_double), ('cost', C.c_double),
                ('iterations', C.c_int32), ('evaluations', C.c_int32), ('status', C.c_int32)]


class ObjectInitConfig(C.Structure):
    """orcvio_object_init_config (include/orcvio_msckf.h)."""
    _fields_ = [('pose_form', C.c_int32), ('min_obs', C.c_int32), ('min_kps', C.c_int32)]


class ObjectInitResult(C.Structure):
    _fields_ = [('wTo', _dp), ('kps_world', _dp), ('kp_used', _ip), ('kp_obs', _ip), ('kp_cond', _dp),
                ('R_kabsch', C.c_double * 9), ('t_kabsch', C.c_double * 3), ('scale', C.c_double), ('sigma', C.c_double * 3),
                ('n_used', C.c_int32), ('status', C.c_int32)]


class ObjectLiteConfig(C.Structure):
    """orcvio_object_lite_config (include/orcvio_msckf.h)."""
    _fields_ = [('use_left_perturbation', C.c_int32), ('use_new_bbox_residual', C.c_int32), ('residual_weights', C.c_double * 2),
                ('reg_every_frame', C.c_int32), ('max_iter', C.c_int32), ('ptol', C.c_double)]


class ObjectInitLiteConfig(C.Structure):
    """orcvio_object_init_lite_config (include/orcvio_msckf.h)."""
    _fields_ = [('pose_form', C.c_int32), ('bbox_scale', C.c_double * 3)]


class ObjectInitLiteResult(C.Structure):
    _fields_ = [('wTo', _dp), ('d', C.c_double), ('status', C.c_int32)]


class ObjectLMMsg(C.Structure):
    """orcvio_object_lm_msg: one orcvio_ros_msgs/ObjectLM message (include/orcvio_msckf.h)."""
    _fields_ = [('object_id', C.c_int64), ('n_rows', C.c_int32), ('n_obj_cols', C.c_int32), ('n_frames', C.c_int32),
                ('residual', _dp), ('jacobian_wrt_object_state', _dp), ('jacobian_wrt_sensor_state', _dp),
                ('valid_camera_pose_mat', _dp), ('timestamps', _dp), ('zs_num_wrt_timestamps', _ip)]


class MsckfIo(C.Structure):
    """orcvio_msckf_io: the handle's pinned arena, written and read in place (include/orcvio_msckf.h)."""
    _fields_ = [('n', C.c_int32), ('poses', _dp), ('p_w', _dp), ('obs_ptr', _ip), ('obs_clone', _ip), ('obs_z', _dp),
                ('obs_zvel', _dp), ('P', _dp), ('dx', _dp), ('gamma', _dp), ('accept', _ip), ('P_out', _dp)]


POSE_STRIDE = 28   # ORCVIO_POSE_STRIDE: R_b2w 9 | t_b_w 3 | t_fej 3 | R_b2c 9 | t_c_b 3 | 1 unused


class MsckfResult(C.Structure):
    _fields_ = [('dx', _dp), ('P_out', _dp), ('accept', _ip), ('gamma', _dp), ('H_thin', _dp), ('r_thin', _dp),
                ('K', _dp), ('G', _dp), ('stats', C.c_int32 * 8)]


class TriangulationConfig(C.Structure):
    _fields_ = [('translation_threshold', C.c_double), ('huber_epsilon', C.c_double), ('estimation_precision', C.c_double),
                ('initial_damping', C.c_double), ('outer_loop_max_iteration', C.c_int32),
                ('inner_loop_max_iteration', C.c_int32), ('cost_threshold', C.c_double),
                ('init_final_dist_threshold', C.c_double)]


class TriangulationResult(C.Structure):
    _fields_ = [('valid', _ip), ('p_w', _dp), ('inv_param', _dp), ('flags', _ip), ('cost', _dp)]


class MsckfIoTri(C.Structure):
    _fields_ = [('valid', C.POINTER(C.c_int32)), ('flags', C.POINTER(C.c_int32)), ('p_w', C.POINTER(C.c_double)),
                ('inv_param', C.POINTER(C.c_double)), ('cost', C.POINTER(C.c_double))]


TRI_KEEP, TRI_ALL, TRI_ALL_BUT_LAST = 0, 1, 2


class CloneChoiceConfig(C.Structure):
    """orcvio_msckf_clone_choice_config (include/orcvio_msckf.h)."""
    _fields_ = [('rotation_threshold', C.c_double), ('translation_threshold', C.c_double), ('tracking_ok', C.c_int32),
                ('R_imu_cam0', C.c_double * 9), ('t_cam0_imu', C.c_double * 3), ('cam_poses', C.POINTER(C.c_double))]


class CloneChoice(C.Structure):
    """orcvio_msckf_clone_choice: the pinned result block of the handle."""
    _fields_ = [('evaluated', C.c_int32), ('agree', C.c_int32), ('chosen', C.c_int32 * 2), ('compared', C.c_int32 * 2), ('taken', C.c_int32 * 2),
                ('angle', C.c_double * 2), ('distance', C.c_double * 2)]


class Zupt(C.Structure):
    """orcvio_msckf_zupt: the zero-velocity update's residual and VARIANCES (include/orcvio_msckf.h)."""
    _fields_ = [('leg_dim', C.c_int32), ('n_clones', C.c_int32), ('r', C.c_double * 9), ('noise_v', C.c_double),
                ('noise_p', C.c_double), ('noise_q', C.c_double)]


class ZuptFrame(C.Structure):
    """orcvio_msckf_zupt_frame: one stationary frame (include/orcvio_msckf.h)."""
    _fields_ = [('zupt', Zupt), ('Phi', _dp), ('Q', _dp), ('augment', C.c_int32), ('remove_previous', C.c_int32)]


class ZuptFrameHybrid(C.Structure):
    """orcvio_msckf_zupt_frame_hybrid: one stationary frame of a hybrid filter (include/orcvio_msckf.h)."""
    _fields_ = [('frame', ZuptFrame), ('idp_dim', C.c_int32), ('n_feature_states', C.c_int32)]


class ImuConfig(C.Structure):
    """orcvio_msckf_imu_config (include/orcvio_msckf.h)."""
    _fields_ = [('leg_dim', C.c_int32), ('use_larvio', C.c_int32), ('use_left_perturbation', C.c_int32), ('use_closed_form', C.c_int32),
                ('if_fej', C.c_int32), ('gravity', C.c_double * 3), ('imu_img_time_th', C.c_double), ('Q_c_diag', C.c_double * 12)]


class ImuState(C.Structure):
    """orcvio_msckf_imu_state: imu_state and the velocity / position of imu_state_FEJ_now."""
    _fields_ = [('time', C.c_double), ('R_b2w', C.c_double * 9), ('v', C.c_double * 3), ('p', C.c_double * 3), ('gyro_bias', C.c_double * 3),
                ('acc_bias', C.c_double * 3), ('v_fej', C.c_double * 3), ('p_fej', C.c_double * 3)]


class ImuInfo(C.Structure):
    _fields_ = [('wait', C.c_int32), ('n_used', C.c_int32), ('n_propagated', C.c_int32), ('applied', C.c_int32), ('dt', C.c_double),
                ('mean_sforce', C.c_double * 3)]


class ImuIntrinsics(C.Structure):
    """orcvio_msckf_imu_intrinsics: T1 T2 T3 A1 A2 A3 M1 M2, as orcvio_msckf_state.imu_intrinsics."""
    _fields_ = [('x', C.c_double * 24)]


class ZuptCheck(C.Structure):
    """orcvio_msckf_zupt_check: the constants of checkZUPTIMU (include/orcvio_msckf.h)."""
    _fields_ = [('sigma_w2', C.c_double), ('sigma_a2', C.c_double), ('sigma_wb', C.c_double), ('sigma_ab', C.c_double),
                ('chi2_prob', C.c_double), ('chi2_multiplier', C.c_double), ('max_velocity', C.c_double), ('use_left_perturbation', C.c_int32)]


class ZuptVerdict(C.Structure):
    """orcvio_msckf_zupt_verdict (include/orcvio_msckf.h)."""
    _fields_ = [('evaluated', C.c_int32), ('accept', C.c_int32), ('dof', C.c_int32), ('status', C.c_int32), ('chi2', C.c_double),
                ('chi2_check', C.c_double), ('speed', C.c_double)]


class Marginal(C.Structure):
    """orcvio_msckf_marginal (include/orcvio_msckf.h): out = P[idx, idx] (m == 0) or T P[idx, idx] T^T."""
    _fields_ = [('n_idx', C.c_int32), ('idx', _ip), ('m', C.c_int32), ('T', _dp)]


MARGINAL_MAX = 64


class MsckfState(C.Structure):
    _fields_ = [('R_b2w_imu', C.c_double * 9), ('v', C.c_double * 3), ('p', C.c_double * 3), ('bg', C.c_double * 3),
                ('ba', C.c_double * 3), ('R_b2c', C.c_double * 9), ('t_c_b', C.c_double * 3), ('td', C.c_double),
                ('imu_intrinsics', C.c_double * 24), ('n_clones', C.c_int32), ('clone_R_b2w', _dp),
                ('clone_t_b_w', _dp), ('clone_R_c2w', _dp), ('clone_t_c_w', _dp)]


_LIB = None
_LIB_DBG = None


def load(debug_hooks=False):
    """Loads the HIP library; raises if it has not been built (no fallback).  debug_hooks: the diagnostics build, which adds the
    orcvio_msckf_debug_* test hooks (a separate shared object with its own state: handles must stay with the library that
    created them)."""
    global _LIB, _LIB_DBG
    try:
        # PyTorch ships its own libamdhip64; importing it first makes this process use ONE HIP
        # runtime (two runtimes in one process cannot both own the device).
        import torch  # noqa: F401
    except Exception:
        pass
    if debug_hooks:
        if _LIB_DBG is None:
            if not os.path.exists(LIB_DBG_PATH):
                raise RuntimeError(f'{LIB_DBG_PATH} is missing: run __graft_entry__.build()')
            _LIB_DBG = _bind(C.CDLL(LIB_DBG_PATH))
        return _LIB_DBG
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'{LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)')
    _LIB = _bind(C.CDLL(LIB_PATH))
    return _LIB


def _bind(lib):
    lib.orcvio_msckf_abi_version.restype = C.c_int32
    lib.orcvio_msckf_last_error.restype = C.c_char_p
    lib.orcvio_msckf_chi2_quantile.restype = C.c_double
    lib.orcvio_msckf_chi2_quantile.argtypes = [C.c_int32, C.c_double]
    lib.orcvio_msckf_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.orcvio_msckf_destroy.argtypes = [C.c_void_p]
    lib.orcvio_msckf_destroy.restype = None
    lib.orcvio_msckf_update_features.argtypes = [C.c_void_p, C.POINTER(MsckfFlags), C.POINTER(MsckfWindow),
                                                 C.POINTER(MsckfTracks), _dp, C.POINTER(MsckfResult)]
    lib.orcvio_msckf_update_objects.argtypes = [C.c_void_p, C.POINTER(MsckfFlags), C.c_int32,
                                                C.POINTER(MsckfObjectRows), C.c_int32, _dp, C.POINTER(MsckfResult)]
    lib.orcvio_msckf_upload.argtypes = [C.c_void_p, C.POINTER(MsckfFlags), C.POINTER(MsckfWindow),
                                        C.POINTER(MsckfTracks), _dp]
    lib.orcvio_msckf_run_local.argtypes = [C.c_void_p, C.c_void_p]
    lib.orcvio_msckf_block_ptr.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.orcvio_msckf_run_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.orcvio_msckf_run_update.argtypes = [C.c_void_p, C.c_void_p]
    lib.orcvio_msckf_sync.argtypes = [C.c_void_p, C.c_void_p]
    lib.orcvio_msckf_download.argtypes = [C.c_void_p, C.POINTER(MsckfResult)]
    lib.orcvio_msckf_profile_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), _dp,
                                                C.POINTER(C.c_int32)]
    lib.orcvio_msckf_increment_state.argtypes = [C.POINTER(MsckfFlags), _dp, C.POINTER(MsckfState)]
    lib.orcvio_msckf_set_option.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.orcvio_msckf_run_local_to.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orcvio_msckf_triangulation_config_default.argtypes = [C.POINTER(TriangulationConfig)]
    lib.orcvio_msckf_triangulation_config_default.restype = None
    lib.orcvio_msckf_triangulate.argtypes = [C.c_void_p, C.POINTER(TriangulationConfig), C.POINTER(MsckfWindow),
                                             C.POINTER(MsckfTracks), _ip, C.POINTER(TriangulationResult)]
    lib.orcvio_msckf_triangulate_uploaded.argtypes = [C.c_void_p, C.POINTER(TriangulationConfig), _ip, C.c_void_p]
    lib.orcvio_msckf_objects_local.argtypes = [C.c_void_p, C.POINTER(MsckfFlags), C.c_int32, C.POINTER(MsckfObjectRows),
                                               C.c_int32, _dp, C.c_void_p, _ip, C.c_void_p]
    lib.orcvio_msckf_objects_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.orcvio_msckf_objects_download.argtypes = [C.c_void_p, C.POINTER(MsckfResult)]
    lib.orcvio_msckf_cov_set.argtypes = [C.c_void_p, C.c_int32, _dp]
    lib.orcvio_msckf_cov_get.argtypes = [C.c_void_p, _ip, _dp]
    lib.orcvio_msckf_cov_get_marginal.argtypes = [C.c_void_p, C.POINTER(Marginal), _dp]
    lib.orcvio_msckf_cov_marginal_submit.argtypes = [C.c_void_p, C.POINTER(Marginal)]
    lib.orcvio_msckf_cov_marginal_collect.argtypes = [C.c_void_p, _dp, _ip]
    lib.orcvio_msckf_cov_propagate.argtypes = [C.c_void_p, C.c_int32, _dp, _dp]
    lib.orcvio_msckf_cov_augment.argtypes = [C.c_void_p]
    lib.orcvio_msckf_cov_remove_clones.argtypes = [C.c_void_p, C.c_int32, _ip, C.c_int32]
    lib.orcvio_msckf_cov_commit.argtypes = [C.c_void_p]
    lib.orcvio_msckf_cov_prefactor.argtypes = [C.c_void_p]
    lib.orcvio_msckf_cov_clones_to_nuisance.argtypes = [C.c_void_p, C.c_int32, _ip, C.c_int32]
    lib.orcvio_msckf_cov_remove_features.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _ip, C.c_int32]
    lib.orcvio_msckf_cov_change_anchors.argtypes = [C.c_void_p, C.POINTER(MsckfFlags), C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp,
                                                    C.POINTER(AnchorChange), C.c_int32, _dp, _dp]
    lib.orcvio_msckf_cov_zupt.argtypes = [C.c_void_p, C.POINTER(Zupt), _dp, _ip]
    lib.orcvio_msckf_cov_zupt_frame.argtypes = [C.c_void_p, C.POINTER(ZuptFrame), _dp, _ip, _ip]
    lib.orcvio_msckf_cov_propagate_imu.argtypes = [C.c_void_p, C.POINTER(ImuConfig), C.POINTER(ImuState), _dp, _dp, C.c_int32, C.c_double,
                                                   C.POINTER(ImuInfo), _dp, _dp]
    lib.orcvio_msckf_io_propagate_imu.argtypes = [C.c_void_p, C.POINTER(ImuConfig), C.POINTER(ImuState), _dp, _dp, C.c_int32, C.c_double,
                                                  C.POINTER(ImuInfo)]
    lib.orcvio_msckf_cov_propagate_imu_calib.argtypes = [C.c_void_p, C.POINTER(ImuConfig), C.POINTER(ImuIntrinsics), C.POINTER(ImuState), _dp, _dp,
                                                         C.c_int32, C.c_double, C.POINTER(ImuInfo), _dp, _dp]
    lib.orcvio_msckf_zupt_check_default.argtypes = [C.POINTER(ZuptCheck)]
    lib.orcvio_msckf_zupt_check_default.restype = None
    lib.orcvio_msckf_cov_zupt_check_imu.argtypes = [C.c_void_p, C.POINTER(ZuptCheck), _dp, _dp, _dp, _dp, _dp, C.c_int32, C.POINTER(ZuptVerdict)]
    lib.orcvio_msckf_cov_propagate_imu_checked.argtypes = [C.c_void_p, C.POINTER(ImuConfig), C.POINTER(ImuState), _dp, _dp, C.c_int32, C.c_double,
                                                           C.POINTER(ImuInfo), _dp, _dp, C.POINTER(ZuptCheck), C.POINTER(ZuptVerdict)]
    lib.orcvio_msckf_cov_zupt_frame_checked.argtypes = [C.c_void_p, C.POINTER(ZuptFrame), C.POINTER(ZuptCheck), _dp, _ip, _ip, C.POINTER(ZuptVerdict)]
    lib.orcvio_msckf_cov_zupt_frame_hybrid.argtypes = [C.c_void_p, C.POINTER(ZuptFrameHybrid), _dp, _ip, _ip]
    lib.orcvio_msckf_cov_zupt_frame_checked_hybrid.argtypes = [C.c_void_p, C.POINTER(ZuptFrameHybrid), C.POINTER(ZuptCheck), _dp, _ip, _ip, C.POINTER(ZuptVerdict)]
    lib.orcvio_msckf_zupt_check_feat.argtypes = [_dp, C.c_int32, C.c_double, _ip, _dp]
    lib.orcvio_msckf_upload_nuisance_poses.argtypes = [C.c_void_p, C.c_void_p]
    lib.orcvio_msckf_update_object_tracks.argtypes = [C.c_void_p, C.POINTER(MsckfFlags), C.POINTER(ObjectEvalFlags), C.c_int32,
                                                      C.POINTER(ObjectTrackC), C.c_int32, _dp, C.POINTER(MsckfResult)]
    lib.orcvio_msckf_objects_local_tracks.argtypes = [C.c_void_p, C.POINTER(MsckfFlags), C.POINTER(ObjectEvalFlags), C.c_int32,
                                                      C.POINTER(ObjectTrackC), C.c_int32, _dp, C.c_void_p, _ip, C.c_void_p]
    lib.orcvio_msckf_io_update_frame.argtypes = [C.c_void_p, C.POINTER(MsckfResult), C.POINTER(MsckfFlags), C.POINTER(ObjectEvalFlags),
                                                 C.POINTER(ObjectTrackC), C.c_int32, C.c_int32, C.POINTER(MsckfResult)]
    lib.orcvio_msckf_io_stage_object_tracks.argtypes = [C.c_void_p, C.POINTER(MsckfFlags), C.POINTER(ObjectEvalFlags), C.POINTER(ObjectTrackC), C.c_int32]
    lib.orcvio_msckf_comm_unique_id.argtypes = [C.c_char_p]
    lib.orcvio_msckf_comm_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32]
    lib.orcvio_msckf_comm_destroy.argtypes = [C.c_void_p]
    lib.orcvio_msckf_comm_info.argtypes = [C.c_void_p, _ip, _ip]
    lib.orcvio_msckf_run_update_sharded.argtypes = [C.c_void_p, C.c_void_p]
    lib.orcvio_msckf_comm_barrier.argtypes = [C.c_void_p]
    lib.orcvio_msckf_comm_allreduce_max.argtypes = [C.c_void_p, _dp, C.c_int32]
    lib.orcvio_msckf_io_begin.argtypes = [C.c_void_p, C.POINTER(MsckfFlags), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(MsckfIo)]
    lib.orcvio_msckf_io_update.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _ip]
    lib.orcvio_msckf_io_submit.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.orcvio_msckf_io_triangulate.argtypes = [C.c_void_p, C.POINTER(TriangulationConfig), _ip, C.POINTER(MsckfIoTri)]
    lib.orcvio_msckf_io_triangulate_prune.argtypes = [C.c_void_p, C.POINTER(TriangulationConfig), C.POINTER(MsckfTracks), _ip, C.POINTER(MsckfIoTri)]
    lib.orcvio_msckf_io_choose_clones.argtypes = [C.c_void_p, C.POINTER(CloneChoiceConfig), C.POINTER(C.POINTER(CloneChoice))]
    lib.orcvio_msckf_io_collect.argtypes = [C.c_void_p, _ip]
    lib.orcvio_msckf_io_step_frame.argtypes = [C.c_void_p, C.POINTER(FrameStep), C.POINTER(FrameResult)]
    lib.orcvio_msckf_io_step_frame_ex.argtypes = [C.c_void_p, C.POINTER(FrameStep), C.POINTER(FrameEvents), C.POINTER(FrameResultEx)]
    lib.orcvio_msckf_update_features_sharded.argtypes = lib.orcvio_msckf_update_features.argtypes
    lib.orcvio_msckf_update_object_tracks_sharded.argtypes = lib.orcvio_msckf_update_object_tracks.argtypes
    return lib


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """ncclGetUniqueId (rank 0); ship the bytes to the other ranks, then every rank calls MsckfUpdater.comm_init."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().orcvio_msckf_comm_unique_id(buf)
    if rc != 0:
        raise MsckfError(rc, 'orcvio_msckf_comm_unique_id')
    return buf.raw


class MsckfError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = load().orcvio_msckf_last_error().decode(errors='replace')
        super().__init__(f'{where}: {STATUS.get(code, code)}: {msg}')


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


class EkfRows(C.Structure):
    """orcvio_msckf_ekf_rows (include/orcvio_msckf.h)."""
    _fields_ = [('n_features', C.c_int32), ('idp_dim', C.c_int32),
                ('anchor', C.POINTER(C.c_int32)), ('state', C.POINTER(C.c_int32)), ('slot', C.POINTER(C.c_int32)),
                ('H_e', C.POINTER(C.c_double)), ('H_a', C.POINTER(C.c_double)), ('H_x', C.POINTER(C.c_double)),
                ('H_f', C.POINTER(C.c_double)), ('z_vel', C.POINTER(C.c_double)), ('r', C.POINTER(C.c_double))]


class SlamFeatures(C.Structure):
    """orcvio_msckf_slam_features (include/orcvio_msckf.h)."""
    _fields_ = [('n_features', C.c_int32), ('idp_dim', C.c_int32),
                ('anchor', C.POINTER(C.c_int32)), ('state', C.POINTER(C.c_int32)), ('slot', C.POINTER(C.c_int32)),
                ('param', C.POINTER(C.c_double)), ('inv_depth', C.POINTER(C.c_double)), ('p_w', C.POINTER(C.c_double)),
                ('p_fej', C.POINTER(C.c_double)), ('z', C.POINTER(C.c_double)), ('z_vel', C.POINTER(C.c_double))]


class FrameStep(C.Structure):
    """orcvio_msckf_frame_step (include/orcvio_msckf.h)."""
    _fields_ = [('leg_dim', C.c_int32), ('Phi', C.POINTER(C.c_double)), ('Q', C.POINTER(C.c_double)), ('augment', C.c_int32),
                ('slam_features', C.POINTER(SlamFeatures)), ('prune_tracks', C.POINTER(MsckfTracks)), ('prune_apply_dx', C.c_int32),
                ('remove_clones', C.POINTER(C.c_int32)), ('n_remove', C.c_int32)]


class FrameResult(C.Structure):
    """orcvio_msckf_frame_result (include/orcvio_msckf.h)."""
    _fields_ = [('stats', C.c_int32 * 8), ('prune_stats', C.c_int32 * 8), ('dx', C.POINTER(C.c_double)), ('gamma', C.POINTER(C.c_double)),
                ('accept', C.POINTER(C.c_int32)), ('prune_dx', C.POINTER(C.c_double)), ('prune_gamma', C.POINTER(C.c_double)),
                ('prune_accept', C.POINTER(C.c_int32)), ('n_after', C.c_int32), ('status_first', C.c_int32), ('status_prune', C.c_int32),
                ('repaired', C.c_int32)]


class AnchorChange(C.Structure):
    """orcvio_msckf_anchor_change (include/orcvio_msckf.h)."""
    _fields_ = [('slot', C.c_int32), ('old_anchor', C.c_int32), ('new_anchor', C.c_int32), ('p_w', C.c_double * 3),
                ('p_fej', C.c_double * 3)]


class FrameEvents(C.Structure):
    """orcvio_msckf_frame_events (include/orcvio_msckf.h)."""
    _fields_ = [('idp_dim', C.c_int32), ('literal_3d', C.c_int32), ('n_feature_states', C.c_int32), ('lost_slots', C.POINTER(C.c_int32)),
                ('n_lost', C.c_int32), ('changes', C.POINTER(AnchorChange)), ('n_changes', C.c_int32), ('R_b2c', C.POINTER(C.c_double)),
                ('t_c_b', C.POINTER(C.c_double))]


class FrameResultEx(C.Structure):
    """orcvio_msckf_frame_result_ex (include/orcvio_msckf.h)."""
    _fields_ = [('frame', FrameResult), ('new_param', C.POINTER(C.c_double)), ('new_inv_depth', C.POINTER(C.c_double)),
                ('status_changes', C.c_int32)]


class MsckfNewFeatures(C.Structure):
    """orcvio_msckf_new_features (include/orcvio_msckf.h)."""
    _fields_ = [('n_features', C.c_int32), ('idp_dim', C.c_int32), ('anchor', C.POINTER(C.c_int32)),
                ('param', C.POINTER(C.c_double)), ('inv_depth', C.POINTER(C.c_double)), ('p_w', C.POINTER(C.c_double)),
                ('p_fej', C.POINTER(C.c_double)), ('obs_ptr', C.POINTER(C.c_int32)), ('obs_clone', C.POINTER(C.c_int32)),
                ('obs_z', C.POINTER(C.c_double)), ('obs_zvel', C.POINTER(C.c_double))]


def make_flags(f) -> MsckfFlags:
    return MsckfFlags(int(f.leg_dim), int(f.use_larvio), int(f.use_left_perturbation), int(f.if_fej),
                      int(f.estimate_td), int(f.discard_large_update), float(f.noise_feature), float(f.chi2_prob))


class MsckfUpdater:
    """Thin owner of one ``orcvio_msckf_handle`` taking ``synth.Window``-shaped inputs."""

    def __init__(self, device=0, max_clones=32, max_features=2048, max_observations=65536, debug_hooks=False):
        self.lib = load(debug_hooks)
        self.debug_hooks = bool(debug_hooks)
        self.h = C.c_void_p()
        rc = self.lib.orcvio_msckf_create(device, max_clones, max_features, max_observations, C.byref(self.h))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_create')
        self._keep = None
        self.n = None
        self.F = None
        self.n_extra = 0

    def set_materialize_stack(self, on: bool):
        """ORCVIO_OPT_MATERIALIZE_STACK: also write the stacked projected blocks [H' | r'] (debug_read 'Hs')."""
        rc = self.lib.orcvio_msckf_set_option(self.h, 1, int(bool(on)))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_set_option')

    def set_fused_solve(self, on: bool):
        """ORCVIO_OPT_FUSED_SOLVE: chol(M) and the triangular solve in one launch (default) or in two."""
        rc = self.lib.orcvio_msckf_set_option(self.h, 2, int(bool(on)))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_set_option')

    def set_lookahead_solve(self, depth: int):
        """ORCVIO_OPT_LOOKAHEAD_SOLVE: 3 (default) / 2 = k_potrf_solve_la with that look-ahead depth, 0 = k_potrf_solve (one workgroup)."""
        rc = self.lib.orcvio_msckf_set_option(self.h, 14, int(depth))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_set_option')

    def set_fused_front(self, on: bool):
        """ORCVIO_OPT_FUSED_FRONT: chol(P) as workgroup 0 of the feature launch (default) or forked to a side stream."""
        rc = self.lib.orcvio_msckf_set_option(self.h, 3, int(bool(on)))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_set_option')

    def set_ekf_rows_mode(self, on: bool):
        """ORCVIO_OPT_EKF_ROWS: the extra states become active columns (upload_ekf_rows may follow an upload)."""
        rc = self.lib.orcvio_msckf_set_option(self.h, 5, int(bool(on)))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_set_option')

    def upload_ekf_rows(self, idp_dim, anchor, state, slot, H_e, H_a, H_x, H_f, r, z_vel=None):
        """Row pairs of the SLAM features the current state observes, as featureJacobian_ekf produces them."""
        F = len(anchor)
        ia = [np.ascontiguousarray(a, dtype=np.int32) for a in (anchor, state, slot)]
        da = [np.ascontiguousarray(a, dtype=np.float64) for a in (H_e, H_a, H_x, H_f, r)]
        zv = None if z_vel is None else np.ascontiguousarray(z_vel, dtype=np.float64)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        rows = EkfRows(F, int(idp_dim), ip(ia[0]), ip(ia[1]), ip(ia[2]), _d(da[0]), _d(da[1]), _d(da[2]), _d(da[3]), _d(zv), _d(da[4]))
        rc = self.lib.orcvio_msckf_upload_ekf_rows(self.h, C.byref(rows))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_upload_ekf_rows')
        self._ekf_F = F

    def upload_slam_features(self, idp_dim, slam, slots=None):
        """SLAM features (synth.SlamFeature-shaped) observed by the current state: rows evaluated on the device."""
        F = len(slam)
        ia = [np.ascontiguousarray(a, dtype=np.int32) for a in ([f.anchor for f in slam], [f.state for f in slam],
                                                                 list(range(F)) if slots is None else slots)]
        param = np.ascontiguousarray([f.inv_param if idp_dim == 3 else f.obs_anchor for f in slam], dtype=np.float64).reshape(F, 3)
        rho = np.ascontiguousarray([f.inv_depth for f in slam], dtype=np.float64)
        pw = np.ascontiguousarray([f.p_w for f in slam], dtype=np.float64).reshape(F, 3)
        pf = np.ascontiguousarray([f.p_fej if f.p_fej is not None else f.p_w for f in slam], dtype=np.float64).reshape(F, 3)
        z = np.ascontiguousarray([f.z for f in slam], dtype=np.float64).reshape(F, 2)
        zv = np.ascontiguousarray([f.z_vel for f in slam], dtype=np.float64).reshape(F, 2)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        st = SlamFeatures(F, int(idp_dim), ip(ia[0]), ip(ia[1]), ip(ia[2]), _d(param), _d(rho), _d(pw), _d(pf), _d(z), _d(zv))
        rc = self.lib.orcvio_msckf_upload_slam_features(self.h, C.byref(st))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_upload_slam_features')
        self._ekf_F = F

    def make_slam_call(self, idp_dim, slam, slots=None):
        """orcvio_msckf_upload_slam_features with the records marshalled once: returns call()."""
        F = len(slam)
        ia = [np.ascontiguousarray(a, dtype=np.int32) for a in ([f.anchor for f in slam], [f.state for f in slam],
                                                                 list(range(F)) if slots is None else slots)]
        param = np.ascontiguousarray([f.inv_param if idp_dim == 3 else f.obs_anchor for f in slam], dtype=np.float64).reshape(F, 3)
        rho = np.ascontiguousarray([f.inv_depth for f in slam], dtype=np.float64)
        pw = np.ascontiguousarray([f.p_w for f in slam], dtype=np.float64).reshape(F, 3)
        pf = np.ascontiguousarray([f.p_fej if f.p_fej is not None else f.p_w for f in slam], dtype=np.float64).reshape(F, 3)
        z = np.ascontiguousarray([f.z for f in slam], dtype=np.float64).reshape(F, 2)
        zv = np.ascontiguousarray([f.z_vel for f in slam], dtype=np.float64).reshape(F, 2)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        st = SlamFeatures(F, int(idp_dim), ip(ia[0]), ip(ia[1]), ip(ia[2]), _d(param), _d(rho), _d(pw), _d(pf), _d(z), _d(zv))
        lib, h = self.lib, self.h

        def call():
            rc = lib.orcvio_msckf_upload_slam_features(h, C.byref(st))
            if rc != 0:
                raise MsckfError(rc, 'orcvio_msckf_upload_slam_features')
            self._ekf_F = F
        call.hold = (ia, param, rho, pw, pf, z, zv, st)
        return call

    def upload_new_features(self, win, idp_dim, feats):
        """Features entering the state (objects as for new_feature_rows): featureJacobian_ekf_new and the W split on the
        device; the V parts join the dense rows of this upload.  Call download_new_feature_blocks() after the update."""
        k, d = len(feats), int(idp_dim)
        ptr, cl, zz, zv = [0], [], [], []
        for ft in feats:
            for (c, z, v) in ft.obs:
                cl.append(c); zz.append(z); zv.append(v)
            ptr.append(len(cl))
        ia = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        da = lambda a, shape: np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
        keep = [ia([f.anchor for f in feats]), da([f.inv_param if d == 3 else f.obs_anchor for f in feats], (k, 3)),
                da([f.inv_depth for f in feats], (k,)), da([f.p_w for f in feats], (k, 3)),
                da([f.p_fej if f.p_fej is not None else f.p_w for f in feats], (k, 3)), ia(ptr), ia(cl), da(zz, (-1, 2)), da(zv, (-1, 2))]
        nf = MsckfNewFeatures(k, d, _i(keep[0]), _d(keep[1]), _d(keep[2]), _d(keep[3]), _d(keep[4]), _i(keep[5]), _i(keep[6]),
                              _d(keep[7]), _d(keep[8]))
        rc = self.lib.orcvio_msckf_upload_new_features(self.h, C.byref(nf))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_upload_new_features')
        self._new = (k, d, win.n)

    def download_new_feature_blocks(self):
        k, d, n = self._new
        H_1, H_2, r_1 = np.zeros((d * k, n)), np.zeros((k, d, d)), np.zeros(d * k)
        rc = self.lib.orcvio_msckf_download_new_feature_blocks(self.h, _d(H_1), _d(H_2), _d(r_1))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_download_new_feature_blocks')
        return H_1, H_2, r_1

    def upload_dense_rows(self, H, r):
        """Caller-projected dense rows over the whole state, stacked as they are (no gate)."""
        H = np.ascontiguousarray(H, dtype=np.float64)
        r = np.ascontiguousarray(r, dtype=np.float64)
        rc = self.lib.orcvio_msckf_upload_dense_rows(self.h, H.shape[0], _d(H), _d(r))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_upload_dense_rows')

    def augment_new_features(self, win, track, anchor, inv_param, dx, P_upd):
        """New 3-d SLAM features that were listed as tracks: (dx_new [3k], P_aug [(n+3k)^2]) after the update."""
        fl, wn, tr, keep = self._structs(win)
        k = len(track)
        n = P_upd.shape[0]
        ti = np.ascontiguousarray(track, dtype=np.int32)
        ai = np.ascontiguousarray(anchor, dtype=np.int32)
        ip = np.ascontiguousarray(inv_param, dtype=np.float64).reshape(k, 3)
        dxc = np.ascontiguousarray(dx, dtype=np.float64)
        Pc = np.ascontiguousarray(P_upd, dtype=np.float64)
        dx_new = np.zeros(3 * k)
        P_aug = np.zeros((n + 3 * k, n + 3 * k))
        rc = self.lib.orcvio_msckf_augment_new_features(self.h, C.byref(wn), k, ti.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        ai.ctypes.data_as(C.POINTER(C.c_int32)), _d(ip), _d(dxc), _d(Pc), _d(dx_new), _d(P_aug))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_augment_new_features')
        return dx_new, P_aug

    def gate_tracks(self, win):
        """gatingTestFeature of every track of `win` against win.P, no update: (gamma [F], accept [F])."""
        fl, wn, tr, keep = self._structs(win)
        gamma = np.zeros(win.F)
        accept = np.zeros(win.F, dtype=np.int32)
        rc = self.lib.orcvio_msckf_gate_tracks(self.h, C.byref(fl), C.byref(wn), C.byref(tr), _d(keep['P']), _d(gamma),
                                               accept.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_gate_tracks')
        return gamma, accept

    def download_ekf(self):
        F = getattr(self, '_ekf_F', 0)
        gamma = np.zeros(F)
        accept = np.zeros(F, dtype=np.int32)
        rc = self.lib.orcvio_msckf_download_ekf(self.h, _d(gamma), accept.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_download_ekf')
        return gamma, accept

    def set_extra_states(self, k: int):
        """ORCVIO_OPT_EXTRA_STATES: k state columns behind the clones (EKF-SLAM feature states) untouched by the rows."""
        rc = self.lib.orcvio_msckf_set_option(self.h, 4, int(k))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_set_option')
        self.n_extra = int(k)

    # -- multi-GPU: the handle's own RCCL communicator ---------------------------------------------
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == COMM_ID_BYTES
        self._chk(self.lib.orcvio_msckf_comm_init(self.h, unique_id, int(rank), int(world)), 'orcvio_msckf_comm_init')

    def comm_destroy(self):
        self._chk(self.lib.orcvio_msckf_comm_destroy(self.h), 'orcvio_msckf_comm_destroy')

    def counters(self):
        """Cumulative counters of the handle: front_fallbacks (fused front end re-run on the forked path because another tenant of the
        device held compute units), launch sequences captured / replayed from a graph / run as plain launches, ..., sym_pulls (pulls of a host P that moved its upper
        tiles only and mirrored them on the device: every even n), lists_in_place (in-place updates whose front end read the host-derived
        index lists in the pinned arena itself, without the launch that pulls them into device memory)."""
        v = (C.c_int64 * 12)()
        self.lib.orcvio_msckf_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]
        self._chk(self.lib.orcvio_msckf_counters(self.h, v, 12), 'orcvio_msckf_counters')
        return dict(front_fallbacks=int(v[0]), graph_captures=int(v[1]), graph_replays=int(v[2]), plain_runs=int(v[3]),
                    front_blocked_by_comm=int(v[4]), obj_fused=int(v[5]), chained_frames=int(v[6]), prestaged_frames=int(v[7]),
                    step_frames=int(v[8]), step_repairs=int(v[9]), sym_pulls=int(v[10]), lists_in_place=int(v[11]))

    def comm_info(self):
        r, w = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.orcvio_msckf_comm_info(self.h, C.byref(r), C.byref(w)), 'orcvio_msckf_comm_info')
        return r.value, w.value

    def comm_details(self):
        v = (C.c_int32 * 8)()
        self.lib.orcvio_msckf_comm_details.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
        self._chk(self.lib.orcvio_msckf_comm_details(self.h, v, 8), 'orcvio_msckf_comm_details')
        return dict(transport={0: 'none', 1: 'rccl', 2: 'ipc'}[int(v[0])], rank=int(v[1]), world=int(v[2]), ranks_seen=int(v[3]),
                    shared_device=bool(v[4]), gather_uncached=bool(v[5]), ipc_across_devices_unverified=bool(v[6]))

    def profile_sharded(self, reps=20):
        """COLLECTIVE.  Device microseconds of this rank's sharded update: local, exchange, replicated solve, total (medians)."""
        us = (C.c_double * 4)()
        self.lib.orcvio_msckf_profile_sharded.argtypes = [C.c_void_p, C.c_int32, _dp]
        self._chk(self.lib.orcvio_msckf_profile_sharded(self.h, int(reps), us), 'orcvio_msckf_profile_sharded')
        return dict(local_us=us[0], exchange_us=us[1], replicated_solve_us=us[2], total_us=us[3])

    def comm_barrier(self):
        """Everything enqueued on the handle's stream is finished on every rank (bounded wait: ERR_TIMEOUT, never a hang)."""
        self._chk(self.lib.orcvio_msckf_comm_barrier(self.h), 'orcvio_msckf_comm_barrier')

    def comm_allreduce_max(self, values):
        """max over the ranks of up to 8 doubles, through the handle's communicator."""
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._chk(self.lib.orcvio_msckf_comm_allreduce_max(self.h, _d(v), int(v.size)), 'orcvio_msckf_comm_allreduce_max')
        return v

    def run_update_sharded(self, stream=None):
        """This rank's uploaded tracks -> block -> RCCL all-gather -> rank-ordered sum -> replicated solve."""
        self._chk(self.lib.orcvio_msckf_run_update_sharded(self.h, C.c_void_p(stream) if stream else None),
                  'orcvio_msckf_run_update_sharded')

    def update_features_sharded(self, win, want_G=False, resident_cov=False, want_P=True):
        """Host buffers in and out; `win` holds THIS RANK's share of the tracks (sharding.shard_window)."""
        fl, w, t, arrs = self._structs(win)
        out, res = self._result(win.n, win.F, False, want_G, False)
        if not want_P:
            res.P_out = None
        rc = self.lib.orcvio_msckf_update_features_sharded(self.h, C.byref(fl), C.byref(w), C.byref(t),
                                                           None if resident_cov else _d(arrs['P']), C.byref(res))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_update_features_sharded')
        return self._finish(out, res, win.F)

    def update_object_tracks_sharded(self, flags, n_clones, objs, P, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D=False, want_G=False):
        """System::processObjects over the ranks: `objs` are THIS RANK's object tracks."""
        fl = make_flags(flags)
        ef, arr, keep = self._object_tracks(objs, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D)
        n = flags.leg_dim + 6 * n_clones + self.n_extra
        Pc = None if P is None else np.ascontiguousarray(P, dtype=np.float64)
        out, res = self._result(n, 1, False, want_G, False)
        rc = self.lib.orcvio_msckf_update_object_tracks_sharded(self.h, C.byref(fl), C.byref(ef), n_clones, arr, len(objs), _d(Pc), C.byref(res))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_update_object_tracks_sharded')
        out = self._finish(out, res, 1)
        out['gamma'] = float(out['gamma'][0])
        out['accept'] = int(out['accept'][0])
        return out

    def close(self):
        if self.h:
            self.lib.orcvio_msckf_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- argument marshalling -------------------------------------------------------------
    def _structs(self, win):
        fl = make_flags(win.flags)
        arrs = dict(R_b2w=np.ascontiguousarray(win.R_b2w, dtype=np.float64),
                    t_b_w=np.ascontiguousarray(win.t_b_w, dtype=np.float64),
                    t_fej=np.ascontiguousarray(win.t_fej, dtype=np.float64),
                    R_b2c=np.ascontiguousarray(win.R_b2c, dtype=np.float64),
                    t_c_b=np.ascontiguousarray(win.t_c_b, dtype=np.float64),
                    p_w=np.ascontiguousarray(win.p_w, dtype=np.float64),
                    obs_ptr=np.ascontiguousarray(win.obs_ptr, dtype=np.int32),
                    obs_clone=np.ascontiguousarray(win.obs_clone, dtype=np.int32),
                    obs_z=np.ascontiguousarray(win.obs_z, dtype=np.float64),
                    obs_zvel=np.ascontiguousarray(win.obs_zvel, dtype=np.float64),
                    P=np.ascontiguousarray(win.P, dtype=np.float64))
        w = MsckfWindow(win.N, _d(arrs['R_b2w']), _d(arrs['t_b_w']), _d(arrs['t_fej']), _d(arrs['R_b2c']),
                        _d(arrs['t_c_b']))
        t = MsckfTracks(win.F, _d(arrs['p_w']), _i(arrs['obs_ptr']), _i(arrs['obs_clone']), _d(arrs['obs_z']),
                        _d(arrs['obs_zvel']))
        return fl, w, t, arrs

    def _result(self, n, F, want_K=False, want_G=False, want_thin=False):
        out = dict(dx=np.zeros(n), P_new=np.zeros((n, n)), accept=np.zeros(max(F, 1), dtype=np.int32),
                   gamma=np.zeros(max(F, 1)))
        if want_thin:
            out['H_thin'] = np.zeros((n - 15, n))
            out['r_thin'] = np.zeros(n - 15)
        if want_K:
            out['K'] = np.zeros((n, n - 15))
        if want_G:
            out['G'] = np.zeros((n, n))
        res = MsckfResult(_d(out['dx']), _d(out['P_new']), _i(out['accept']), _d(out['gamma']),
                          _d(out.get('H_thin')), _d(out.get('r_thin')), _d(out.get('K')), _d(out.get('G')))
        return out, res

    @staticmethod
    def _finish(out, res, F):
        out['accept'] = out['accept'][:F]
        out['gamma'] = out['gamma'][:F]
        out['stats'] = np.array(list(res.stats), dtype=np.int32)
        out['updated'] = bool(out['stats'][3])
        return out

    # -- one-shot host-buffer update (the reference call sites) ---------------------------
    def update_features(self, win, want_K=False, want_G=False, want_thin=False, resident_cov=False, want_P=True):
        """resident_cov: the prior is the device-resident covariance (P is not sent); want_P=False: P+ stays in HBM
        (cov_commit makes it the resident covariance) and only dx, gamma, accept come back."""
        fl, w, t, arrs = self._structs(win)
        out, res = self._result(win.n, win.F, want_K, want_G, want_thin)
        if not want_P:
            res.P_out = None
        rc = self.lib.orcvio_msckf_update_features(self.h, C.byref(fl), C.byref(w), C.byref(t),
                                                   None if resident_cov else _d(arrs['P']), C.byref(res))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_update_features')
        return self._finish(out, res, win.F)

    # -- the zero-copy boundary: the handle's pinned arena written and read in place ----------------
    def io_begin(self, flags, N, F, nobs, with_P=True):
        """orcvio_msckf_io_begin: returns numpy VIEWS of the handle's pinned arena -- inputs to fill (poses [N, 28], p_w, obs_ptr,
        obs_clone, obs_z, obs_zvel or None, P or None) and outputs to read after io_update (dx, gamma, accept, P_out)."""
        fl = make_flags(flags)
        io = MsckfIo()
        self._chk(self.lib.orcvio_msckf_io_begin(self.h, C.byref(fl), int(N), int(F), int(nobs), 2 if with_P == 2 and with_P is not True else int(bool(with_P)), C.byref(io)), 'orcvio_msckf_io_begin')
        n = int(io.n)
        view = lambda ptr, shape: None if not ptr else np.ctypeslib.as_array(ptr, shape=shape)
        self.n, self.F = n, int(F)
        self._io_keep = (fl, io)
        return dict(n=n, poses=view(io.poses, (N, POSE_STRIDE)), p_w=view(io.p_w, (max(F, 1), 3))[:F], obs_ptr=view(io.obs_ptr, (F + 1,)),
                    obs_clone=view(io.obs_clone, (max(nobs, 1),))[:nobs], obs_z=view(io.obs_z, (max(nobs, 1), 2))[:nobs],
                    obs_zvel=None if not io.obs_zvel else view(io.obs_zvel, (max(nobs, 1), 2))[:nobs], P=view(io.P, (n, n)),
                    dx=view(io.dx, (n,)), gamma=view(io.gamma, (max(F, 1),))[:F], accept=view(io.accept, (max(F, 1),))[:F],
                    P_out=view(io.P_out, (n, n)))

    def io_fill(self, io, win, with_P=True):
        """Writes a synth.Window into the arena views of io_begin (what a caller's flatten step does in place)."""
        io['poses'][:, 0:9] = win.R_b2w.reshape(win.N, 9)
        io['poses'][:, 9:12] = win.t_b_w
        io['poses'][:, 12:15] = win.t_fej
        io['poses'][:, 15:24] = win.R_b2c.reshape(win.N, 9)
        io['poses'][:, 24:27] = win.t_c_b
        io['poses'][:, 27] = 0.0
        io['obs_ptr'][:] = win.obs_ptr
        if win.F:
            io['p_w'][:] = win.p_w
            io['obs_clone'][:] = win.obs_clone
            io['obs_z'][:] = win.obs_z
            if io['obs_zvel'] is not None:
                io['obs_zvel'][:] = win.obs_zvel
        if with_P:
            io['P'][:] = win.P

    def io_update(self, want_P=True, commit=False):
        """orcvio_msckf_io_update on what stands in the arena; returns the stats (the results are in the io_begin views)."""
        stats = np.zeros(8, dtype=np.int32)
        self._chk(self.lib.orcvio_msckf_io_update(self.h, int(bool(want_P)), int(bool(commit)), _i(stats)), 'orcvio_msckf_io_update')
        return stats

    def io_triangulate(self, cfg=None, mode=None):
        """orcvio_msckf_io_triangulate: arms the next update on the open arena (io_update, io_submit, the first update of
        io_step_frame / io_step_frame_ex) to triangulate its tracks on the device.  mode: None (every track TRI_ALL) or [F] of TRI_KEEP /
        TRI_ALL / TRI_ALL_BUT_LAST.  Returns numpy VIEWS of the handle's pinned block (valid, flags, p_w, solution, cost), filled when that
        update returns.  cfg: as for triangulate(); cfg=False passes NULL (a refusal)."""
        c = None if cfg is False else self._tri_config(cfg)
        md = None if mode is None else np.ascontiguousarray(mode, dtype=np.int32)
        out = MsckfIoTri()
        self._chk(self.lib.orcvio_msckf_io_triangulate(self.h, None if c is None else C.byref(c), _i(md), C.byref(out)), 'orcvio_msckf_io_triangulate')
        F = self.F
        view = lambda ptr, shape: np.ctypeslib.as_array(ptr, shape=shape)
        return dict(valid=view(out.valid, (max(F, 1),))[:F], flags=view(out.flags, (max(F, 1),))[:F], p_w=view(out.p_w, (max(F, 1), 3))[:F],
                    solution=view(out.inv_param, (max(F, 1), 3))[:F], cost=view(out.cost, (max(F, 1),))[:F])

    def io_triangulate_prune(self, tri_win, cfg=None, mode=None):
        """orcvio_msckf_io_triangulate_prune: arms the SECOND (prune) update of the next io_step_frame / io_step_frame_ex on the open
        arena.  tri_win: a synth.Window (or anything with F, obs_ptr, obs_clone, obs_z) listing EVERY observation of the prune tracks in
        the window, track j for track j of the prune set; tri_win=False passes NULL.  mode: None (every track TRI_ALL_MOTION_BUT_LAST) or
        [F2].  Returns numpy VIEWS of the handle's second pinned block (valid, flags, p_w, solution, cost), filled when the frame returns."""
        c = None if cfg is False else self._tri_config(cfg)
        md = None if mode is None else np.ascontiguousarray(mode, dtype=np.int32)
        out = MsckfIoTri()
        F, tr = 0, None
        if tri_win is not False:
            F = int(tri_win.F)
            arrs = [np.ascontiguousarray(tri_win.obs_ptr, dtype=np.int32), np.ascontiguousarray(tri_win.obs_clone, dtype=np.int32),
                    np.ascontiguousarray(tri_win.obs_z, dtype=np.float64)]
            tr = MsckfTracks(F, None, _i(arrs[0]), _i(arrs[1]), _d(arrs[2]), None)
        self._chk(self.lib.orcvio_msckf_io_triangulate_prune(self.h, None if c is None else C.byref(c), None if tr is None else C.byref(tr), _i(md),
                                                             C.byref(out)), 'orcvio_msckf_io_triangulate_prune')
        view = lambda ptr, shape: np.ctypeslib.as_array(ptr, shape=shape)
        return dict(valid=view(out.valid, (max(F, 1),))[:F], flags=view(out.flags, (max(F, 1),))[:F], p_w=view(out.p_w, (max(F, 1), 3))[:F],
                    solution=view(out.inv_param, (max(F, 1), 3))[:F], cost=view(out.cost, (max(F, 1),))[:F])

    def io_choose_clones(self, cam_poses, rotation_threshold, translation_threshold, tracking_ok=1, R_imu_cam0=None, t_cam0_imu=None):
        """orcvio_msckf_io_choose_clones: arms the next io_step_frame / io_step_frame_ex on the open arena -- the frame's remove_clones are
        checked on the device against findRedundantImuStates on the poses the first update leaves.  cam_poses [N][12] (orientation_cam
        row-major | position_cam) as they stand before the frame, or False for NULL; R_imu_cam0 / t_cam0_imu the IMU state's extrinsic.
        Returns the handle's pinned CloneChoice block (a ctypes structure, filled when the frame returns; choice_dict() copies it)."""
        cfg = CloneChoiceConfig()
        cfg.rotation_threshold, cfg.translation_threshold, cfg.tracking_ok = float(rotation_threshold), float(translation_threshold), int(tracking_ok)
        cfg.R_imu_cam0[:] = [float(x) for x in np.asarray(np.eye(3) if R_imu_cam0 is None else R_imu_cam0, dtype=np.float64).ravel()]
        cfg.t_cam0_imu[:] = [float(x) for x in np.asarray(np.zeros(3) if t_cam0_imu is None else t_cam0_imu, dtype=np.float64).ravel()]
        cp = None
        if cam_poses is not False:
            cp = np.ascontiguousarray(cam_poses, dtype=np.float64)
            cfg.cam_poses = _d(cp)
        out = C.POINTER(CloneChoice)()
        self._chk(self.lib.orcvio_msckf_io_choose_clones(self.h, C.byref(cfg), C.byref(out)), 'orcvio_msckf_io_choose_clones')
        return out.contents

    @staticmethod
    def choice_dict(blk):
        return dict(evaluated=int(blk.evaluated), agree=int(blk.agree), chosen=[int(x) for x in blk.chosen], compared=[int(x) for x in blk.compared],
                    taken=[int(x) for x in blk.taken], angle=np.array(blk.angle[:], dtype=np.float64), distance=np.array(blk.distance[:], dtype=np.float64))

    def io_submit(self, want_P=True, commit=False):
        """orcvio_msckf_io_submit: the update on what stands in the arena is launched; io_collect() waits for it."""
        self._chk(self.lib.orcvio_msckf_io_submit(self.h, int(bool(want_P)), int(bool(commit))), 'orcvio_msckf_io_submit')

    def io_collect(self):
        stats = np.zeros(8, dtype=np.int32)
        self._chk(self.lib.orcvio_msckf_io_collect(self.h, _i(stats)), 'orcvio_msckf_io_collect')
        return stats

    def make_io_call(self, win, resident_cov=False, want_P=True, commit=False):
        """io_begin + the window written into the arena ONCE: returns (call, views) where call() is orcvio_msckf_io_update alone --
        the per-frame cost of a caller that flattens its containers straight into the arena (bench.py's latency modes)."""
        io = self.io_begin(win.flags, win.N, win.F, int(win.obs_ptr[-1]), with_P=not resident_cov)
        self.io_fill(io, win, with_P=not resident_cov)
        lib, h = self.lib, self.h
        stats = np.zeros(8, dtype=np.int32)
        args = (h, int(bool(want_P)), int(bool(commit)), _i(stats))

        def call():
            rc = lib.orcvio_msckf_io_update(*args)
            if rc != 0:
                raise MsckfError(rc, 'orcvio_msckf_io_update')
        call._keep = (io, stats)
        io['stats'] = stats
        return call, io

    def make_update_call(self, win, resident_cov=False, want_P=True, commit=False):
        """The one-shot update with the argument structs marshalled ONCE: returns (call, out) where call() runs
        orcvio_msckf_update_features (and orcvio_msckf_cov_commit if `commit`) on the same buffers -- what a C++ caller's
        per-frame cost is, without this binding's numpy / ctypes marshalling (bench.py's latency modes)."""
        fl, w, t, arrs = self._structs(win)
        out, res = self._result(win.n, win.F)
        if not want_P:
            res.P_out = None
        Pp = None if resident_cov else _d(arrs['P'])
        lib, h = self.lib, self.h
        args = (h, C.byref(fl), C.byref(w), C.byref(t), Pp, C.byref(res))
        keep = (fl, w, t, arrs, res)

        def call():
            rc = lib.orcvio_msckf_update_features(*args)
            if rc == 0 and commit:
                rc = lib.orcvio_msckf_cov_commit(h)
            if rc != 0:
                raise MsckfError(rc, 'orcvio_msckf_update_features')
        call._keep = keep
        self.n, self.F = win.n, win.F
        return call, out

    # -- object blocks (OrcVIO::removeLostObjects) ---------------------------------------------
    def update_objects(self, flags, n_clones, blocks, P, want_G=False):
        """blocks: list of dict(row_clone [rows] int32, Hx6 [rows,6], Hf [rows,no], res [rows])."""
        fl = make_flags(flags)
        n = flags.leg_dim + 6 * n_clones + self.n_extra
        keep = []
        arr = (MsckfObjectRows * max(len(blocks), 1))()
        for k, b in enumerate(blocks):
            rc_ = np.ascontiguousarray(b['row_clone'], dtype=np.int32)
            hx = np.ascontiguousarray(b['Hx6'], dtype=np.float64)
            hf = np.ascontiguousarray(b['Hf'], dtype=np.float64)
            rs = np.ascontiguousarray(b['res'], dtype=np.float64)
            keep += [rc_, hx, hf, rs]
            arr[k] = MsckfObjectRows(len(rs), hf.shape[1] if hf.ndim == 2 else 0, _i(rc_), _d(hx), _d(hf), _d(rs))
        Pc = np.ascontiguousarray(P, dtype=np.float64)
        out, res = self._result(n, 1, False, want_G, False)
        rc = self.lib.orcvio_msckf_update_objects(self.h, C.byref(fl), n_clones, arr, len(blocks), _d(Pc), C.byref(res))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_update_objects')
        out = self._finish(out, res, 1)
        out['gamma'] = float(out['gamma'][0])
        out['accept'] = int(out['accept'][0])
        return out

    def update_object_lm_msgs(self, flags, n_clones, window_timestamps, R_b2c, t_c_b, msgs, P, fix_D=False, wire_row_major=True):
        """msgs: list of dict(object_id, residual [rows], jacobian_wrt_object_state [rows, no], jacobian_wrt_sensor_state [rows, 6],
        valid_camera_pose_mat [6, frames], timestamps [frames], zs_num_wrt_timestamps [frames]) -- the fields of ObjectLM.msg; the
        2-d arrays are flattened in the wire's order (row-major, or column-major when wire_row_major is False)."""
        fl = make_flags(flags)
        order = 'C' if wire_row_major else 'F'
        arr = (ObjectLMMsg * max(len(msgs), 1))()
        keep = []
        for k, m in enumerate(msgs):
            res = np.ascontiguousarray(m['residual'], dtype=np.float64)
            jo = np.asarray(m['jacobian_wrt_object_state'], dtype=np.float64)
            js = np.asarray(m['jacobian_wrt_sensor_state'], dtype=np.float64)
            pm = np.asarray(m['valid_camera_pose_mat'], dtype=np.float64)
            ts = np.ascontiguousarray(m['timestamps'], dtype=np.float64)
            zn = np.ascontiguousarray(m['zs_num_wrt_timestamps'], dtype=np.int32)
            flat = [np.ascontiguousarray(a.ravel(order=order)) for a in (jo, js, pm)]
            keep += [res, ts, zn] + flat
            arr[k] = ObjectLMMsg(int(m.get('object_id', k)), len(res), jo.shape[1], len(ts), _d(res), _d(flat[0]), _d(flat[1]), _d(flat[2]), _d(ts), _i(zn))
        wt = np.ascontiguousarray(window_timestamps, dtype=np.float64)
        Rb = np.ascontiguousarray(R_b2c, dtype=np.float64)
        tb = np.ascontiguousarray(t_c_b, dtype=np.float64)
        Pc = None if P is None else np.ascontiguousarray(P, dtype=np.float64)
        n = flags.leg_dim + 6 * n_clones + self.n_extra
        out, res_ = self._result(n, 1)
        self.lib.orcvio_msckf_update_object_lm_msgs.argtypes = [C.c_void_p, C.POINTER(MsckfFlags), C.c_int32, _dp, _dp, _dp, C.c_int32, C.c_int32,
                                                                C.POINTER(ObjectLMMsg), C.c_int32, _dp, C.POINTER(MsckfResult)]
        rc = self.lib.orcvio_msckf_update_object_lm_msgs(self.h, C.byref(fl), n_clones, _d(wt), _d(Rb), _d(tb), int(fix_D), int(wire_row_major),
                                                         arr, len(msgs), _d(Pc), C.byref(res_))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_update_object_lm_msgs')
        out = self._finish(out, res_, 1)
        out['gamma'] = float(out['gamma'][0])
        out['accept'] = int(out['accept'][0])
        return out

    def _object_blocks(self, blocks):
        keep = []
        arr = (MsckfObjectRows * max(len(blocks), 1))()
        for k, b in enumerate(blocks):
            rc_ = np.ascontiguousarray(b['row_clone'], dtype=np.int32)
            hx = np.ascontiguousarray(b['Hx6'], dtype=np.float64)
            hf = np.ascontiguousarray(b['Hf'], dtype=np.float64)
            rs = np.ascontiguousarray(b['res'], dtype=np.float64)
            keep += [rc_, hx, hf, rs]
            arr[k] = MsckfObjectRows(len(rs), hf.shape[1] if hf.ndim == 2 else 0, _i(rc_), _d(hx), _d(hf), _d(rs))
        return arr, keep

    def objects_local(self, flags, n_clones, blocks, P, d_dst=None, stream=None):
        """This rank's objects -> its compressed block (in d_dst or the handle's own block); returns the local dof."""
        fl = make_flags(flags)
        arr, keep = self._object_blocks(blocks)
        Pc = np.ascontiguousarray(P, dtype=np.float64)
        dof = C.c_int32(0)
        rc = self.lib.orcvio_msckf_objects_local(self.h, C.byref(fl), n_clones, arr, len(blocks), _d(Pc),
                                                 C.c_void_p(d_dst) if d_dst else None, C.byref(dof),
                                                 C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_objects_local')
        self.n = flags.leg_dim + 6 * n_clones + self.n_extra
        return int(dof.value)

    def objects_finish(self, d_blocks, n_blocks, dof_total, stream=None):
        rc = self.lib.orcvio_msckf_objects_finish(self.h, C.c_void_p(d_blocks), n_blocks, int(dof_total),
                                                  C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_objects_finish')

    def objects_download(self, want_G=False):
        out, res = self._result(self.n, 1, False, want_G, False)
        rc = self.lib.orcvio_msckf_objects_download(self.h, C.byref(res))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_objects_download')
        out = self._finish(out, res, 1)
        out['gamma'] = float(out['gamma'][0])
        out['accept'] = int(out['accept'][0])
        return out

    def object_rows_eval(self, obj, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D=False):
        """Residual rows of one object track (synth.ObjectTrack-shaped) in window coordinates, evaluated on the GPU.
        Returns dict(row_clone, Hx6, Hf, res) ready for update_objects, or None if no frame is in the window."""
        K = obj.kps.shape[0]
        F = len(obj.frames)
        fl = ObjectEvalFlags(int(obj_left), int(new_bbox), int(vio_left), int(fix_D))
        fl.R_b2c[:] = list(np.asarray(R_b2c, dtype=np.float64).ravel())
        fl.t_c_b[:] = list(np.asarray(t_c_b, dtype=np.float64).ravel())
        wTo = np.ascontiguousarray(obj.wTo, dtype=np.float64)
        shape = np.ascontiguousarray(obj.shape, dtype=np.float64)
        kps = np.ascontiguousarray(obj.kps, dtype=np.float64)
        wTc = np.ascontiguousarray(np.stack([fr['wTc'] for fr in obj.frames]), dtype=np.float64)
        zs = np.ascontiguousarray(np.stack([fr['zs'] for fr in obj.frames]), dtype=np.float64)
        bb = np.ascontiguousarray(np.stack([fr['bbox'] for fr in obj.frames]), dtype=np.float64)
        cl = np.ascontiguousarray([fr['clone'] for fr in obj.frames], dtype=np.int32)
        tr = ObjectTrackC(K, F, _d(wTo), _d(shape), _d(kps), _d(wTc), _d(zs), _d(bb), _i(cl))
        cap = F * (2 * K + 4)
        ncol = 9 + 3 * K
        row_clone = np.zeros(cap, dtype=np.int32)
        Hx6 = np.zeros((cap, 6)); Hf = np.zeros((cap, ncol)); res = np.zeros(cap)
        n_rows = C.c_int32(0)
        self.lib.orcvio_msckf_object_rows_eval.argtypes = [C.c_void_p, C.POINTER(ObjectEvalFlags), C.POINTER(ObjectTrackC),
                                                           C.c_int32, C.POINTER(C.c_int32), _ip, _dp, _dp, _dp]
        rc = self.lib.orcvio_msckf_object_rows_eval(self.h, C.byref(fl), C.byref(tr), cap, C.byref(n_rows), _i(row_clone),
                                                    _d(Hx6), _d(Hf), _d(res))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_object_rows_eval')
        m = n_rows.value
        if m == 0:
            return None
        return dict(row_clone=row_clone[:m].copy(), Hx6=Hx6[:m].copy(), Hf=Hf[:m].copy(), res=res[:m].copy())

    def _object_tracks(self, objs, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D):
        fl = ObjectEvalFlags(int(obj_left), int(new_bbox), int(vio_left), int(fix_D))
        fl.R_b2c[:] = list(np.asarray(R_b2c, dtype=np.float64).ravel())
        fl.t_c_b[:] = list(np.asarray(t_c_b, dtype=np.float64).ravel())
        arr = (ObjectTrackC * max(len(objs), 1))()
        keep = []
        for k, obj in enumerate(objs):
            wTo = np.ascontiguousarray(obj.wTo, dtype=np.float64)
            shape = np.ascontiguousarray(obj.shape, dtype=np.float64)
            kps = np.ascontiguousarray(np.asarray(obj.kps, dtype=np.float64).reshape(-1, 3))
            K = kps.shape[0]
            wTc = np.ascontiguousarray(np.stack([fr['wTc'] for fr in obj.frames]), dtype=np.float64)
            bb = np.ascontiguousarray(np.stack([fr['bbox'] for fr in obj.frames]), dtype=np.float64)
            cl = np.ascontiguousarray([fr['clone'] for fr in obj.frames], dtype=np.int32)
            if K == 0:   # bbox-only track: no keypoints (the library reads neither kps nor frame_zs; one-element dummies keep the pointers valid)
                kps = np.zeros((1, 3))
                zs = np.zeros((len(obj.frames), 1, 2))
            else:
                zs = np.ascontiguousarray(np.stack([np.asarray(fr['zs'], dtype=np.float64).reshape(-1, 2) for fr in obj.frames]))
            keep += [wTo, shape, kps, wTc, zs, bb, cl]
            arr[k] = ObjectTrackC(K, len(obj.frames), _d(wTo), _d(shape), _d(kps), _d(wTc), _d(zs), _d(bb), _i(cl))
        return fl, arr, keep

    def update_object_tracks(self, flags, n_clones, objs, P, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D=False, want_G=False):
        """removeLostObjects straight from object tracks (synth.ObjectTrack-shaped): rows evaluated on the device."""
        fl = make_flags(flags)
        ef, arr, keep = self._object_tracks(objs, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D)
        n = flags.leg_dim + 6 * n_clones + self.n_extra
        Pc = None if P is None else np.ascontiguousarray(P, dtype=np.float64)
        out, res = self._result(n, 1, False, want_G, False)
        rc = self.lib.orcvio_msckf_update_object_tracks(self.h, C.byref(fl), C.byref(ef), n_clones, arr, len(objs), _d(Pc), C.byref(res))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_update_object_tracks')
        out = self._finish(out, res, 1)
        out['gamma'] = float(out['gamma'][0])
        out['accept'] = int(out['accept'][0])
        return out

    # ---- the object mapper: what the four LM-bearing calls share -----------------------------------------------------------------
    def _lm_config(self, left, new_bbox, weights, max_iter, ptol, reg_every_frame=None):
        """ObjectLMConfig (four weights), or with reg_every_frame ObjectLiteConfig (two weights): the library's defaults, then the
        caller's values."""
        lite = reg_every_frame is not None
        cls = ObjectLiteConfig if lite else ObjectLMConfig
        default = self.lib.orcvio_msckf_object_lite_config_default if lite else self.lib.orcvio_msckf_object_lm_config_default
        cfg = cls()
        default.argtypes = [C.POINTER(cls)]
        default.restype = None
        default(C.byref(cfg))
        cfg.use_left_perturbation = int(left)
        cfg.use_new_bbox_residual = int(new_bbox)
        cfg.residual_weights[:] = [float(w) for w in weights]
        if lite:
            cfg.reg_every_frame = int(reg_every_frame)
        if max_iter is not None:
            cfg.max_iter = int(max_iter)
        if ptol is not None:
            cfg.ptol = float(ptol)
        return cfg

    @staticmethod
    def _lm_records(n, mean_shapes, mean_kps, keep):
        """The prior and result records of an optimiser and the arrays its results land in, per object (wTo, shape, kps).
        mean_kps: one contiguous [K][3] array per object, or None for bbox-only tracks (no keypoint pointers at all)."""
        priors = (ObjectLMPrior * max(n, 1))()
        results = (ObjectLMResult * max(n, 1))()
        outs = []
        for k in range(n):
            ms = np.ascontiguousarray(mean_shapes[k], dtype=np.float64).reshape(3)
            keep.append(ms)
            if mean_kps is None:
                o = (np.zeros((4, 4)), np.zeros(3), None)
                priors[k] = ObjectLMPrior(_d(ms), None)
            else:
                o = (np.zeros((4, 4)), np.zeros(3), np.zeros((max(mean_kps[k].shape[0], 1), 3)))
                priors[k] = ObjectLMPrior(_d(ms), _d(mean_kps[k]))
            outs.append(o)
            results[k].wTo, results[k].shape, results[k].kps = _d(o[0]), _d(o[1]), _d(o[2])
        return priors, results, outs

    @staticmethod
    def _lm_outs(objs, arr, results, outs):
        """(tracks, stats) of an optimiser: synth.ObjectTrack copies at the optimum (kps [0][3] for a bbox-only track; the frames
        shared with the inputs: update_object_tracks takes them as they are) and the statistics."""
        from . import synth
        tracks, stats = [], []
        for k, obj in enumerate(objs):
            kps = np.zeros((0, 3)) if outs[k][2] is None else outs[k][2][:arr[k].n_keypoints].copy()
            tracks.append(synth.ObjectTrack(wTo=outs[k][0], shape=outs[k][1], kps=kps, frames=obj.frames))
            stats.append(dict(cost0=float(results[k].cost0), cost=float(results[k].cost), iterations=int(results[k].iterations),
                              evaluations=int(results[k].evaluations), status=int(results[k].status)))
        return tracks, stats

    def object_lm(self, objs, mean_shapes, mean_kps, left, new_bbox, weights, max_iter=None, ptol=None):
        """orcvio_msckf_object_lm: Levenberg-Marquardt over every object track of `objs` (synth.ObjectTrack-shaped, their state the
        start) in one launch.  mean_shapes [n][3] / mean_kps [n][K][3]: the priors of the two regularisers, one per object.
        Returns (tracks, stats): synth.ObjectTrack copies at the optimum (frames shared with the inputs) and per object
        dict(cost0, cost, iterations, evaluations, status)."""
        cfg = self._lm_config(left, new_bbox, weights, max_iter, ptol)
        _, arr, keep = self._object_tracks(objs, np.eye(3), np.zeros(3), left, new_bbox, 0, False)
        n = len(objs)
        mks = [np.ascontiguousarray(np.asarray(mean_kps[k], dtype=np.float64).reshape(-1, 3)) for k in range(n)]
        for k, mk in enumerate(mks):
            if mk.shape[0] != arr[k].n_keypoints:
                raise ValueError('object_lm: mean_kps[%d] has %d keypoints, the track %d' % (k, mk.shape[0], arr[k].n_keypoints))
        priors, results, outs = self._lm_records(n, mean_shapes, mks, keep)
        self.lib.orcvio_msckf_object_lm.argtypes = [C.c_void_p, C.POINTER(ObjectLMConfig), C.POINTER(ObjectTrackC),
                                                    C.POINTER(ObjectLMPrior), C.c_int32, C.POINTER(ObjectLMResult)]
        self.lib.orcvio_msckf_object_lm.restype = C.c_int32
        rc = self.lib.orcvio_msckf_object_lm(self.h, C.byref(cfg), arr, priors, n, results)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_object_lm')
        return self._lm_outs(objs, arr, results, outs)

    def _object_init_args(self, objs, mean_kps, pose_form, min_obs, min_kps, with_bbox):
        """Track records with only what the initialiser reads (wTo / shape / kps / frame_clone NULL), its config and result records."""
        cfg = ObjectInitConfig()
        self.lib.orcvio_msckf_object_init_config_default.argtypes = [C.POINTER(ObjectInitConfig)]
        self.lib.orcvio_msckf_object_init_config_default.restype = None
        self.lib.orcvio_msckf_object_init_config_default(C.byref(cfg))
        if pose_form is not None:
            cfg.pose_form = int(pose_form)
        if min_obs is not None:
            cfg.min_obs = int(min_obs)
        if min_kps is not None:
            cfg.min_kps = int(min_kps)
        n = len(objs)
        arr = (ObjectTrackC * max(n, 1))()
        results = (ObjectInitResult * max(n, 1))()
        keep, outs, mks = [], [], []
        for k, obj in enumerate(objs):
            mk = np.ascontiguousarray(np.asarray(mean_kps[k], dtype=np.float64).reshape(-1, 3))
            K = mk.shape[0]
            wTc = np.ascontiguousarray(np.stack([fr['wTc'] for fr in obj.frames]), dtype=np.float64)
            zs = np.ascontiguousarray(np.stack([np.asarray(fr['zs'], dtype=np.float64).reshape(-1, 2) for fr in obj.frames]))
            if zs.shape[1] != K:
                raise ValueError('object_init: mean_kps[%d] has %d keypoints, the track %d' % (k, K, zs.shape[1]))
            bb = np.ascontiguousarray(np.stack([fr['bbox'] for fr in obj.frames]), dtype=np.float64) if with_bbox else None
            o = dict(wTo=np.zeros((4, 4)), kps_world=np.zeros((max(K, 1), 3)), kp_used=np.zeros(max(K, 1), dtype=np.int32),
                     kp_obs=np.zeros(max(K, 1), dtype=np.int32), kp_cond=np.zeros(max(K, 1)))
            keep += [mk, wTc, zs, bb]
            outs.append(o)
            mks.append(mk)
            arr[k] = ObjectTrackC(K, len(obj.frames), None, None, None, _d(wTc), _d(zs), _d(bb), None)
            results[k].wTo, results[k].kps_world, results[k].kp_cond = _d(o['wTo']), _d(o['kps_world']), _d(o['kp_cond'])
            results[k].kp_used, results[k].kp_obs = _i(o['kp_used']), _i(o['kp_obs'])
        return cfg, arr, results, outs, mks, keep

    @staticmethod
    def _object_init_outs(results, outs):
        res = []
        for k, o in enumerate(outs):
            r = results[k]
            res.append(dict(o, R=np.array(r.R_kabsch[:]).reshape(3, 3), t=np.array(r.t_kabsch[:]), scale=float(r.scale),
                            sigma=np.array(r.sigma[:]), n_used=int(r.n_used), status=int(r.status)))
        return res

    def object_init(self, objs, mean_kps, pose_form=None, min_obs=None, min_kps=None):
        """orcvio_msckf_object_init: the start pose of every object track of `objs` (synth.ObjectTrack-shaped: their frames' wTc and
        zs are read) in one launch -- keypoint triangulation, Kabsch alignment of mean_kps [n][K][3] onto the triangulated keypoints,
        the pose form of include/orcvio_msckf.h.  Returns per object dict(wTo, kps_world, kp_used, kp_obs, kp_cond, R, t, scale,
        sigma, n_used, status)."""
        cfg, arr, results, outs, mks, keep = self._object_init_args(objs, mean_kps, pose_form, min_obs, min_kps, False)
        n = len(objs)
        ptrs = (_dp * max(n, 1))(*[_d(m) for m in mks])
        self.lib.orcvio_msckf_object_init.argtypes = [C.c_void_p, C.POINTER(ObjectInitConfig), C.POINTER(ObjectTrackC), C.POINTER(_dp),
                                                      C.c_int32, C.POINTER(ObjectInitResult)]
        self.lib.orcvio_msckf_object_init.restype = C.c_int32
        rc = self.lib.orcvio_msckf_object_init(self.h, C.byref(cfg), arr, ptrs, n, results)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_object_init')
        return self._object_init_outs(results, outs)

    def object_init_lm(self, objs, mean_shapes, mean_kps, left, new_bbox, weights, max_iter=None, ptol=None, pose_form=None, min_obs=None,
                       min_kps=None):
        """orcvio_msckf_object_init_lm: object_init and object_lm from its start (the pose, the mean shape, the mean keypoints) in ONE
        call.  Returns (inits, tracks, stats): object_init's list, and object_lm's two; an object whose initialisation did not end
        with status 1 has LM status 0, the identity and the means."""
        icfg, arr, iresults, iouts, mks, keep = self._object_init_args(objs, mean_kps, pose_form, min_obs, min_kps, True)
        cfg = self._lm_config(left, new_bbox, weights, max_iter, ptol)
        n = len(objs)
        priors, results, outs = self._lm_records(n, mean_shapes, mks, keep)
        self.lib.orcvio_msckf_object_init_lm.argtypes = [C.c_void_p, C.POINTER(ObjectInitConfig), C.POINTER(ObjectLMConfig),
                                                         C.POINTER(ObjectTrackC), C.POINTER(ObjectLMPrior), C.c_int32,
                                                         C.POINTER(ObjectInitResult), C.POINTER(ObjectLMResult)]
        self.lib.orcvio_msckf_object_init_lm.restype = C.c_int32
        rc = self.lib.orcvio_msckf_object_init_lm(self.h, C.byref(icfg), C.byref(cfg), arr, priors, n, iresults, results)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_object_init_lm')
        tracks, stats = self._lm_outs(objs, arr, results, outs)
        return self._object_init_outs(iresults, iouts), tracks, stats

    # ---- the lite (bbox-only) object mapper ------------------------------------------------------------------------------------
    def _lite_tracks(self, objs, with_start):
        """Track records with n_keypoints = 0 and only what the lite calls read (kps / frame_zs / frame_clone NULL; wTo and shape
        too where the start is the device's)."""
        n = len(objs)
        arr = (ObjectTrackC * max(n, 1))()
        keep = []
        for k, obj in enumerate(objs):
            wTc = np.ascontiguousarray(np.stack([fr['wTc'] for fr in obj.frames]), dtype=np.float64)
            bb = np.ascontiguousarray(np.stack([fr['bbox'] for fr in obj.frames]), dtype=np.float64)
            wTo = np.ascontiguousarray(obj.wTo, dtype=np.float64) if with_start else None
            shape = np.ascontiguousarray(obj.shape, dtype=np.float64) if with_start else None
            keep += [wTc, bb, wTo, shape]
            arr[k] = ObjectTrackC(0, len(obj.frames), _d(wTo), _d(shape), None, _d(wTc), None, _d(bb), None)
        return arr, keep

    # (_lite_config and _lite_init_config are kept under these names and signatures: tests/test_gpu_object_lite.py builds raw calls with them)
    def _lite_config(self, left, new_bbox, weights, reg_every_frame, max_iter, ptol):
        return self._lm_config(left, new_bbox, weights, max_iter, ptol, reg_every_frame)

    def _lite_init_config(self, pose_form, bbox_scale):
        cfg = ObjectInitLiteConfig()
        self.lib.orcvio_msckf_object_init_lite_config_default.argtypes = [C.POINTER(ObjectInitLiteConfig)]
        self.lib.orcvio_msckf_object_init_lite_config_default.restype = None
        self.lib.orcvio_msckf_object_init_lite_config_default(C.byref(cfg))
        if pose_form is not None:
            cfg.pose_form = int(pose_form)
        if bbox_scale is not None:
            cfg.bbox_scale[:] = [float(v) for v in bbox_scale]
        return cfg

    def _lite_init_args(self, n, pose_form, bbox_scale):
        """The lite initialiser's config, its result records and the arrays its poses land in."""
        cfg = self._lite_init_config(pose_form, bbox_scale)
        results = (ObjectInitLiteResult * max(n, 1))()
        outs = [np.zeros((4, 4)) for _ in range(n)]
        for k in range(n):
            results[k].wTo = _d(outs[k])
        return cfg, results, outs

    @staticmethod
    def _lite_init_outs(results, outs):
        return [dict(wTo=o, d=float(results[k].d), status=int(results[k].status)) for k, o in enumerate(outs)]

    def object_lm_lite(self, objs, mean_shapes, left, new_bbox, weights=(1.0, 1.0), reg_every_frame=0, max_iter=None, ptol=None):
        """orcvio_msckf_object_lm_lite: the 9-dof Levenberg-Marquardt over every bbox-only track of `objs` (synth.ObjectTrack-shaped:
        wTo and shape are the start, the frames' wTc and bbox are read; kps and zs are ignored) in one launch, one wavefront per
        object.  weights: (bbox rows, shape regulariser).  Returns (tracks, stats) as object_lm does, the tracks without keypoints."""
        cfg = self._lm_config(left, new_bbox, weights, max_iter, ptol, reg_every_frame)
        arr, keep = self._lite_tracks(objs, True)
        n = len(objs)
        priors, results, outs = self._lm_records(n, mean_shapes, None, keep)
        self.lib.orcvio_msckf_object_lm_lite.argtypes = [C.c_void_p, C.POINTER(ObjectLiteConfig), C.POINTER(ObjectTrackC),
                                                         C.POINTER(ObjectLMPrior), C.c_int32, C.POINTER(ObjectLMResult)]
        self.lib.orcvio_msckf_object_lm_lite.restype = C.c_int32
        rc = self.lib.orcvio_msckf_object_lm_lite(self.h, C.byref(cfg), arr, priors, n, results)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_object_lm_lite')
        return self._lm_outs(objs, arr, results, outs)

    def object_init_lite(self, objs, mean_shapes, pose_form=None, bbox_scale=None):
        """orcvio_msckf_object_init_lite: the start pose of every bbox-only track from its first frame's camera and box.  Returns per
        object dict(wTo, d, status)."""
        arr, keep = self._lite_tracks(objs, False)
        n = len(objs)
        cfg, results, outs = self._lite_init_args(n, pose_form, bbox_scale)
        ms = [np.ascontiguousarray(m, dtype=np.float64).reshape(3) for m in mean_shapes]
        ptrs = (_dp * max(n, 1))(*[_d(m) for m in ms])
        self.lib.orcvio_msckf_object_init_lite.argtypes = [C.c_void_p, C.POINTER(ObjectInitLiteConfig), C.POINTER(ObjectTrackC), C.POINTER(_dp),
                                                           C.c_int32, C.POINTER(ObjectInitLiteResult)]
        self.lib.orcvio_msckf_object_init_lite.restype = C.c_int32
        rc = self.lib.orcvio_msckf_object_init_lite(self.h, C.byref(cfg), arr, ptrs, n, results)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_object_init_lite')
        return self._lite_init_outs(results, outs)

    def object_init_lm_lite(self, objs, mean_shapes, left, new_bbox, weights=(1.0, 1.0), reg_every_frame=0, max_iter=None, ptol=None,
                            pose_form=None, bbox_scale=None):
        """orcvio_msckf_object_init_lm_lite: object_init_lite and object_lm_lite from its start (the pose, the mean shape) in ONE call.
        Returns (inits, tracks, stats); an object whose start failed has LM status 0, the identity and the mean shape."""
        cfg = self._lm_config(left, new_bbox, weights, max_iter, ptol, reg_every_frame)
        arr, keep = self._lite_tracks(objs, False)
        n = len(objs)
        icfg, iresults, iouts = self._lite_init_args(n, pose_form, bbox_scale)
        priors, results, outs = self._lm_records(n, mean_shapes, None, keep)
        self.lib.orcvio_msckf_object_init_lm_lite.argtypes = [C.c_void_p, C.POINTER(ObjectInitLiteConfig), C.POINTER(ObjectLiteConfig),
                                                              C.POINTER(ObjectTrackC), C.POINTER(ObjectLMPrior), C.c_int32,
                                                              C.POINTER(ObjectInitLiteResult), C.POINTER(ObjectLMResult)]
        self.lib.orcvio_msckf_object_init_lm_lite.restype = C.c_int32
        rc = self.lib.orcvio_msckf_object_init_lm_lite(self.h, C.byref(icfg), C.byref(cfg), arr, priors, n, iresults, results)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_object_init_lm_lite')
        tracks, stats = self._lm_outs(objs, arr, results, outs)
        return self._lite_init_outs(iresults, iouts), tracks, stats

    def objects_local_tracks(self, flags, n_clones, objs, P, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D=False):
        """The first half of update_object_tracks alone: the rows of the tracks evaluated on the device and compressed into the handle's
        own block (debug_read 'Ab' of the diagnostics build: sum over the objects of X^T (I - Q_f Q_f^T) X); returns the local dof."""
        fl = make_flags(flags)
        ef, arr, keep = self._object_tracks(objs, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D)
        Pc = None if P is None else np.ascontiguousarray(P, dtype=np.float64)
        dof = C.c_int32(0)
        rc = self.lib.orcvio_msckf_objects_local_tracks(self.h, C.byref(fl), C.byref(ef), n_clones, arr, len(objs), _d(Pc), None, C.byref(dof), None)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_objects_local_tracks')
        self.n = flags.leg_dim + 6 * n_clones + self.n_extra
        self.sync()
        return int(dof.value)

    def update_frame(self, win, oflags, objs, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D=False, commit_objects=True):
        """orcvio_msckf_io_update_frame: the feature update of `win` on the resident covariance (arena written in place, committed
        inside the launch) and the object update of `objs` on the covariance it leaves, the objects' compression beside the
        features' solve.  Returns (features, objects) result dicts."""
        io = self.io_begin(win.flags, win.N, win.F, int(win.obs_ptr[-1]), with_P=False)
        self.io_fill(io, win, with_P=False)
        call, outs = self.make_frame_call(win, oflags, objs, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D, commit_objects)
        call()
        return outs()

    def make_frame_call(self, win, oflags, objs, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D=False, commit_objects=True):
        """Arguments of orcvio_msckf_io_update_frame marshalled once (the arena must have been laid out and filled: io_begin /
        io_fill with with_P=False): returns (call, outs) -- call() is the C call alone, outs() the two result dicts."""
        ofl = make_flags(oflags)
        ef, arr, keep = self._object_tracks(objs, R_b2c, t_c_b, obj_left, new_bbox, vio_left, fix_D)
        out_f, res_f = self._result(win.n, win.F)
        res_f.P_out = None
        out_o, res_o = self._result(win.n, 1)
        res_o.P_out = None
        lib, h, nobj, co = self.lib, self.h, len(objs), int(bool(commit_objects))
        hold = (ofl, ef, arr, keep, out_f, res_f, out_o, res_o)

        def call():
            rc = lib.orcvio_msckf_io_update_frame(h, C.byref(res_f), C.byref(ofl), C.byref(ef), arr, nobj, co, C.byref(res_o))
            if rc != 0:
                raise MsckfError(rc, 'orcvio_msckf_io_update_frame')

        def stage():
            # orcvio_msckf_io_stage_object_tracks: the same tracks staged AHEAD of the call (between io_fill and call())
            rc = lib.orcvio_msckf_io_stage_object_tracks(h, C.byref(ofl), C.byref(ef), arr, nobj)
            if rc != 0:
                raise MsckfError(rc, 'orcvio_msckf_io_stage_object_tracks')
        call.stage = stage

        def outs():
            f = self._finish(dict(out_f), res_f, win.F)
            o = self._finish(dict(out_o), res_o, 1)
            o['gamma'] = float(o['gamma'][0])
            o['accept'] = int(o['accept'][0])
            return f, o
        call.hold = hold
        return call, outs

    # -- staged, device-resident form -----------------------------------------------------
    def upload(self, win, without_positions=False, resident_cov=False):
        """without_positions: p_w is not sent (NULL); triangulate_uploaded() must run before the update.
        resident_cov: P is not sent (NULL): the device-resident covariance (cov_*) is the prior."""
        fl, w, t, arrs = self._structs(win)
        if without_positions:
            t.p_w = None
        rc = self.lib.orcvio_msckf_upload(self.h, C.byref(fl), C.byref(w), C.byref(t), None if resident_cov else _d(arrs['P']))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_upload')
        self.n, self.F = win.n, win.F

    # -- device-resident covariance ------------------------------------------------------------------
    def _chk(self, rc, where):
        if rc != 0:
            raise MsckfError(rc, where)

    def cov_set(self, P):
        Pc = np.ascontiguousarray(P, dtype=np.float64)
        self._chk(self.lib.orcvio_msckf_cov_set(self.h, Pc.shape[0], _d(Pc)), 'orcvio_msckf_cov_set')

    def cov_get(self):
        n = C.c_int32(0)
        self._chk(self.lib.orcvio_msckf_cov_get(self.h, C.byref(n), None), 'orcvio_msckf_cov_get')
        P = np.zeros((n.value, n.value))
        self._chk(self.lib.orcvio_msckf_cov_get(self.h, C.byref(n), _d(P)), 'orcvio_msckf_cov_get')
        return P

    @staticmethod
    def _marginal(idx, T):
        """The orcvio_msckf_marginal of (idx, T) and the arrays it points into (kept alive by the caller)."""
        ix = np.ascontiguousarray(idx, dtype=np.int32).ravel()
        q = Marginal()
        q.n_idx = int(ix.size)
        q.idx = ix.ctypes.data_as(_ip)
        Tc = None
        if T is not None:
            Tc = np.ascontiguousarray(T, dtype=np.float64)
            if Tc.ndim != 2 or Tc.shape[1] != ix.size:
                raise ValueError('T must be [m][len(idx)]')
            q.m = int(Tc.shape[0])
            q.T = _d(Tc)
        return q, (ix, Tc)

    def cov_get_marginal(self, idx, T=None):
        """orcvio_msckf_cov_get_marginal: P[idx, idx] of the resident covariance (T None: bit copies), or T P[idx, idx] T^T, by one
        one-workgroup launch that stores into pinned memory -- without fetching P."""
        q, keep = self._marginal(idx, T)
        r = q.m if q.m > 0 else q.n_idx
        out = np.zeros((r, r))
        self._chk(self.lib.orcvio_msckf_cov_get_marginal(self.h, C.byref(q), _d(out)), 'orcvio_msckf_cov_get_marginal')
        return out

    def cov_marginal_submit(self, idx, T=None):
        """orcvio_msckf_cov_marginal_submit: validates, stages and enqueues; cov_marginal_collect() brings the result."""
        q, keep = self._marginal(idx, T)
        self._chk(self.lib.orcvio_msckf_cov_marginal_submit(self.h, C.byref(q)), 'orcvio_msckf_cov_marginal_submit')

    def cov_marginal_collect(self):
        """orcvio_msckf_cov_marginal_collect: the result of the outstanding submit, [rows][rows]."""
        out = np.zeros((MARGINAL_MAX, MARGINAL_MAX))
        rows = C.c_int32(0)
        self._chk(self.lib.orcvio_msckf_cov_marginal_collect(self.h, _d(out), C.byref(rows)), 'orcvio_msckf_cov_marginal_collect')
        r = rows.value
        return out.ravel()[:r * r].reshape(r, r).copy()

    def io_step_frame_ex(self, win, Phi=None, Q=None, augment=True, slam=None, idp_dim=1, prune=None, prune_apply_dx=False, remove=(),
                         n_feature_states=0, lost=(), changes=(), R_b2c=None, t_c_b=None, literal_3d=0, raise_on_refusal=True, triangulate=None,
                         triangulate_prune=None, choose_clones=None):
        """orcvio_msckf_io_step_frame_ex: io_step_frame plus the frame's feature events.  `win` and set_extra_states are those AFTER the
        removals; lost: slots in feature_states before the call (ascending), n_feature_states their count before the removals;
        changes: objects with slot (after the removals), old, new, p_w, p_fej; R_b2c / t_c_b: the IMU's current extrinsics.
        Returns io_step_frame's dict plus new_param [k, 3], new_inv_depth [k], status_changes."""
        ls = np.ascontiguousarray(list(lost), dtype=np.int32)
        k = len(changes)
        arr = (AnchorChange * max(k, 1))()
        for q, c in enumerate(changes):
            arr[q].slot, arr[q].old_anchor, arr[q].new_anchor = int(c.slot), int(c.old), int(c.new)
            arr[q].p_w[:] = [float(x) for x in c.p_w]
            pf = c.p_w if getattr(c, 'p_fej', None) is None else c.p_fej
            arr[q].p_fej[:] = [float(x) for x in pf]
        Rb = None if R_b2c is None else np.ascontiguousarray(R_b2c, dtype=np.float64).reshape(9)
        tb = None if t_c_b is None else np.ascontiguousarray(t_c_b, dtype=np.float64).reshape(3)
        ev = FrameEvents(int(idp_dim), int(literal_3d), int(n_feature_states), _i(ls) if len(ls) else None, len(ls), arr if k else None, k,
                         _d(Rb), _d(tb))
        return self.io_step_frame(win, Phi, Q, augment, slam, idp_dim, prune, prune_apply_dx, remove, raise_on_refusal, _events=(ev, k, (ls, arr, Rb, tb)),
                                  triangulate=triangulate, triangulate_prune=triangulate_prune, choose_clones=choose_clones)

    def io_step_frame(self, win, Phi=None, Q=None, augment=True, slam=None, idp_dim=1, prune=None, prune_apply_dx=False, remove=(),
                      raise_on_refusal=True, _events=None, triangulate=None, triangulate_prune=None, choose_clones=None):
        """orcvio_msckf_io_step_frame: ONE filter frame on the resident covariance -- propagation, augmentation, the update on `win`'s
        tracks (+ the in-state features `slam`), the prune update on `prune`'s tracks (a synth.Window sharing win's poses), the
        marginalisation of `remove`.  Returns dict(dx, gamma, accept, stats, prune_dx, prune_gamma, prune_accept, prune_stats, n_after,
        status_first, status_prune, repaired) with copies of the results.  triangulate: None, True or dict(cfg=, mode=) -- the first
        update triangulates its tracks on the device (io_triangulate); the dict then has tri = copies of valid, flags, p_w, solution, cost.
        triangulate_prune: None, or a pair (window listing EVERY observation of the prune tracks, modes or None) [a third entry: the
        config] -- the prune update triangulates its tracks on the device between the two updates (io_triangulate_prune); the dict then
        has prune_tri with the keys of tri.  choose_clones: None, or the keyword arguments of io_choose_clones -- `remove` is then the
        caller's prediction, checked on the device between the two updates; the dict has choice (choice_dict)."""
        io = self.io_begin(win.flags, win.N, win.F, int(win.obs_ptr[-1]), with_P=2)
        self.io_fill(io, win, with_P=False)
        tri = None
        if triangulate:
            targ = triangulate if isinstance(triangulate, dict) else {}
            tri = self.io_triangulate(targ.get('cfg'), targ.get('mode'))
        tri2 = None
        if triangulate_prune is not None:
            tri2 = self.io_triangulate_prune(triangulate_prune[0], triangulate_prune[2] if len(triangulate_prune) > 2 else None, triangulate_prune[1])
        choice = None if choose_clones is None else self.io_choose_clones(**choose_clones)
        keep = []
        st = FrameStep()
        st.leg_dim = int(win.flags.leg_dim)
        if Phi is not None:
            Ph = np.ascontiguousarray(Phi, dtype=np.float64); Qc = np.ascontiguousarray(Q, dtype=np.float64)
            keep += [Ph, Qc]
            st.Phi = _d(Ph); st.Q = _d(Qc)
        st.augment = int(bool(augment))
        if slam is not None and len(slam) > 0:
            call = self.make_slam_call(idp_dim, slam)
            keep.append(call)
            st.slam_features = C.pointer(call.hold[-1])
        F2 = 0
        if prune is not None:
            F2 = int(prune.F)
            arrs = [np.ascontiguousarray(prune.p_w, dtype=np.float64), np.ascontiguousarray(prune.obs_ptr, dtype=np.int32),
                    np.ascontiguousarray(prune.obs_clone, dtype=np.int32), np.ascontiguousarray(prune.obs_z, dtype=np.float64),
                    np.ascontiguousarray(prune.obs_zvel, dtype=np.float64)]
            tr = MsckfTracks(F2, _d(arrs[0]), _i(arrs[1]), _i(arrs[2]), _d(arrs[3]), _d(arrs[4]) if win.flags.estimate_td else None)
            keep += arrs + [tr]
            st.prune_tracks = C.pointer(tr)
        st.prune_apply_dx = int(bool(prune_apply_dx))
        rm = np.ascontiguousarray(list(remove), dtype=np.int32)
        keep.append(rm)
        if len(rm):
            st.remove_clones = _i(rm)
        st.n_remove = len(rm)
        extra = {}
        if _events is None:
            res = FrameResult()
            rc = self.lib.orcvio_msckf_io_step_frame(self.h, C.byref(st), C.byref(res))
            where = 'orcvio_msckf_io_step_frame'
        else:
            rex = FrameResultEx()
            rc = self.lib.orcvio_msckf_io_step_frame_ex(self.h, C.byref(st), C.byref(_events[0]), C.byref(rex))
            where = 'orcvio_msckf_io_step_frame_ex'
            res = rex.frame
        if rc != 0 and (raise_on_refusal or rc != 6):
            raise MsckfError(rc, where)
        n = int(io['n'])
        arr = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(dt, copy=True) if p else None
        if _events is not None:
            k = _events[1]
            par = arr(rex.new_param, 3 * k, np.float64)
            extra = dict(new_param=None if par is None else par.reshape(k, 3), new_inv_depth=arr(rex.new_inv_depth, k, np.float64),
                         status_changes=int(rex.status_changes))
        if tri is not None:
            extra['tri'] = {k: v.copy() for k, v in tri.items()}
        if tri2 is not None:
            extra['prune_tri'] = {k: v.copy() for k, v in tri2.items()}
        if choice is not None:
            extra['choice'] = self.choice_dict(choice)
        return dict(**extra, rc=rc, dx=arr(res.dx, n, np.float64), gamma=arr(res.gamma, win.F, np.float64), accept=arr(res.accept, win.F, np.int32),
                    stats=np.array(res.stats[:], dtype=np.int32), prune_dx=arr(res.prune_dx, n, np.float64),
                    prune_gamma=arr(res.prune_gamma, F2, np.float64), prune_accept=arr(res.prune_accept, F2, np.int32),
                    prune_stats=np.array(res.prune_stats[:], dtype=np.int32), n_after=int(res.n_after), status_first=int(res.status_first),
                    status_prune=int(res.status_prune), repaired=int(res.repaired))

    def cov_propagate(self, Phi, Q):
        Ph = np.ascontiguousarray(Phi, dtype=np.float64)
        Qc = np.ascontiguousarray(Q, dtype=np.float64)
        self._chk(self.lib.orcvio_msckf_cov_propagate(self.h, Ph.shape[0], _d(Ph), _d(Qc)), 'orcvio_msckf_cov_propagate')

    @staticmethod
    def imu_config(leg_dim=22, use_larvio=1, use_left=0, use_closed_form=1, if_fej=0, gravity=(0.0, 0.0, -9.81), imu_img_time_th=0.0025,
                   Qc_diag=None):
        c = ImuConfig(leg_dim, int(use_larvio), int(use_left), int(use_closed_form), int(if_fej))
        c.gravity[:] = [float(x) for x in gravity]
        c.imu_img_time_th = float(imu_img_time_th)
        c.Q_c_diag[:] = [float(x) for x in (np.zeros(12) if Qc_diag is None else Qc_diag)]
        return c

    @staticmethod
    def imu_state(time, R, v, p, bg, ba, v_fej=None, p_fej=None):
        s = ImuState()
        s.time = float(time)
        s.R_b2w[:] = [float(x) for x in np.asarray(R).ravel()]
        for name, val in (('v', v), ('p', p), ('gyro_bias', bg), ('acc_bias', ba), ('v_fej', v if v_fej is None else v_fej),
                          ('p_fej', p if p_fej is None else p_fej)):
            getattr(s, name)[:] = [float(x) for x in val]
        return s

    def cov_propagate_imu(self, cfg, state, prev_meas, samples, time_bound, wait=False, want_PhiQ=False, raise_on_refusal=True):
        """orcvio_msckf_cov_propagate_imu: the IMU step from raw samples on the resident covariance.  cfg: ImuConfig; state: ImuState,
        propagated in place; prev_meas [6] (m_gyro_old | m_acc_old), updated in place; samples [n][7] t | gyro | acc.  Returns
        dict(status, n_used, n_propagated, dt, mean_sforce, applied, Phi, Q); Phi, Q [22][22] with want_PhiQ (the call then waits)."""
        smp = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 7)
        assert isinstance(prev_meas, np.ndarray) and prev_meas.dtype == np.float64 and prev_meas.size == 6 and prev_meas.flags.c_contiguous
        info = ImuInfo()
        info.wait = 1 if wait else 0
        Phi = np.zeros((22, 22)) if want_PhiQ else None
        Q = np.zeros((22, 22)) if want_PhiQ else None
        rc = self.lib.orcvio_msckf_cov_propagate_imu(self.h, C.byref(cfg), C.byref(state), _d(prev_meas), _d(smp) if smp.size else None,
                                                     smp.shape[0], float(time_bound), C.byref(info), _d(Phi) if want_PhiQ else None,
                                                     _d(Q) if want_PhiQ else None)
        if rc != 0 and (raise_on_refusal or rc != 6):
            raise MsckfError(rc, 'orcvio_msckf_cov_propagate_imu')
        return dict(status=int(rc), n_used=int(info.n_used), n_propagated=int(info.n_propagated), dt=float(info.dt),
                    mean_sforce=np.array(info.mean_sforce[:]), applied=int(info.applied), Phi=Phi, Q=Q)

    @staticmethod
    def imu_intrinsics(x=None):
        """ImuIntrinsics from 24 values (T1 T2 T3 A1 A2 A3 M1 M2); None: T2 = M2 = 1, the rest 0 (Tg = Ma = I, As = 0)."""
        s = ImuIntrinsics()
        vals = [0, 0, 0, 1, 1, 1] + [0] * 15 + [1, 1, 1] if x is None else np.asarray(x, dtype=np.float64).ravel()
        assert len(vals) == 24
        s.x[:] = [float(v) for v in vals]
        return s

    def cov_propagate_imu_calib(self, cfg, intr, state, prev_meas, samples, time_bound, wait=False, want_PhiQ=False, raise_on_refusal=True):
        """orcvio_msckf_cov_propagate_imu_calib: cov_propagate_imu at leg_dim 46, the 24 IMU intrinsics (ImuIntrinsics) in the state.
        Returns the dict of cov_propagate_imu; Phi, Q [46][46] with want_PhiQ (the call then waits)."""
        smp = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 7)
        assert isinstance(prev_meas, np.ndarray) and prev_meas.dtype == np.float64 and prev_meas.size == 6 and prev_meas.flags.c_contiguous
        info = ImuInfo()
        info.wait = 1 if wait else 0
        Phi = np.zeros((46, 46)) if want_PhiQ else None
        Q = np.zeros((46, 46)) if want_PhiQ else None
        rc = self.lib.orcvio_msckf_cov_propagate_imu_calib(self.h, C.byref(cfg), C.byref(intr), C.byref(state), _d(prev_meas),
                                                           _d(smp) if smp.size else None, smp.shape[0], float(time_bound), C.byref(info),
                                                           _d(Phi) if want_PhiQ else None, _d(Q) if want_PhiQ else None)
        if rc != 0 and (raise_on_refusal or rc != 6):
            raise MsckfError(rc, 'orcvio_msckf_cov_propagate_imu_calib')
        return dict(status=int(rc), n_used=int(info.n_used), n_propagated=int(info.n_propagated), dt=float(info.dt),
                    mean_sforce=np.array(info.mean_sforce[:]), applied=int(info.applied), Phi=Phi, Q=Q)

    def io_propagate_imu(self, cfg, state, prev_meas, samples, time_bound):
        """orcvio_msckf_io_propagate_imu: the host half now (state, prev_meas updated in place), the next io_step_frame / io_step_frame_ex /
        cov_zupt_frame on the handle -- given Phi = Q = None -- makes Phi and Q on the device in front of its head launch."""
        smp = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 7)
        assert isinstance(prev_meas, np.ndarray) and prev_meas.dtype == np.float64 and prev_meas.size == 6 and prev_meas.flags.c_contiguous
        info = ImuInfo()
        self._chk(self.lib.orcvio_msckf_io_propagate_imu(self.h, C.byref(cfg), C.byref(state), _d(prev_meas), _d(smp) if smp.size else None,
                                                         smp.shape[0], float(time_bound), C.byref(info)), 'orcvio_msckf_io_propagate_imu')
        return dict(n_used=int(info.n_used), n_propagated=int(info.n_propagated), dt=float(info.dt), mean_sforce=np.array(info.mean_sforce[:]))

    def cov_augment(self):
        self._chk(self.lib.orcvio_msckf_cov_augment(self.h), 'orcvio_msckf_cov_augment')

    def cov_remove_clones(self, leg_dim, indices):
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        self._chk(self.lib.orcvio_msckf_cov_remove_clones(self.h, leg_dim, _i(ix), len(ix)), 'orcvio_msckf_cov_remove_clones')

    def cov_commit(self):
        self._chk(self.lib.orcvio_msckf_cov_commit(self.h), 'orcvio_msckf_cov_commit')

    def cov_clones_to_nuisance(self, leg_dim, indices):
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        self._chk(self.lib.orcvio_msckf_cov_clones_to_nuisance(self.h, leg_dim, _i(ix), len(ix)), 'orcvio_msckf_cov_clones_to_nuisance')

    def cov_remove_features(self, leg_dim, n_clones, idp_dim, n_feature_states, slots):
        """orcvio_msckf_cov_remove_features: rmLostFeaturesCov on the resident covariance (slots ascending, numbered before the call)."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        self._chk(self.lib.orcvio_msckf_cov_remove_features(self.h, leg_dim, n_clones, idp_dim, n_feature_states, _i(sl) if len(sl) else None,
                                                            len(sl)), 'orcvio_msckf_cov_remove_features')

    def cov_change_anchors(self, flags, idp_dim, poses, R_b2c, t_c_b, changes, literal_3d=0):
        """orcvio_msckf_cov_change_anchors on the resident covariance.  poses [N][28] (synth.pack_poses); changes: objects with the
        attributes slot, old, new (window ranks), p_w, p_fej.  Returns (param [k, 3], rho [k])."""
        ps = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, POSE_STRIDE)
        Rb = np.ascontiguousarray(R_b2c, dtype=np.float64).reshape(9)
        tb = np.ascontiguousarray(t_c_b, dtype=np.float64).reshape(3)
        k = len(changes)
        arr = (AnchorChange * max(k, 1))()
        for q, c in enumerate(changes):
            arr[q].slot, arr[q].old_anchor, arr[q].new_anchor = int(c.slot), int(c.old), int(c.new)
            arr[q].p_w[:] = [float(x) for x in c.p_w]
            pf = c.p_w if getattr(c, 'p_fej', None) is None else c.p_fej
            arr[q].p_fej[:] = [float(x) for x in pf]
        fl = make_flags(flags)
        param = np.zeros((max(k, 1), 3))
        rho = np.zeros(max(k, 1))
        self._chk(self.lib.orcvio_msckf_cov_change_anchors(self.h, C.byref(fl), int(idp_dim), int(literal_3d), ps.shape[0], _d(ps), _d(Rb), _d(tb),
                                                           arr, k, _d(param), _d(rho)), 'orcvio_msckf_cov_change_anchors')
        return param[:k], rho[:k]

    @staticmethod
    def _zupt_struct(leg_dim, n_clones, r, noises):
        z = Zupt()
        z.leg_dim, z.n_clones = int(leg_dim), int(n_clones)
        z.r[:] = [float(x) for x in np.asarray(r, dtype=np.float64).reshape(9)]
        z.noise_v, z.noise_p, z.noise_q = (float(x) for x in noises)
        return z

    def _zupt_hybrid_struct(self, leg_dim, n_clones, r, noises, idp_dim, n_feature_states, Phi, Q, augment, remove_previous, keep):
        f = ZuptFrameHybrid()
        f.frame.zupt = self._zupt_struct(leg_dim, n_clones, r, noises)
        if Phi is not None:
            keep.append(np.ascontiguousarray(Phi, dtype=np.float64)); f.frame.Phi = _d(keep[-1])
        if Q is not None:
            keep.append(np.ascontiguousarray(Q, dtype=np.float64)); f.frame.Q = _d(keep[-1])
        f.frame.augment, f.frame.remove_previous = int(bool(augment)), int(bool(remove_previous))
        f.idp_dim, f.n_feature_states = int(idp_dim), int(n_feature_states)
        return f

    def _zupt_call(self, name, leg_dim, n_clones, r, noises, raise_on_refusal, frame=None, hybrid=None, chk=None):
        """The marshalling of the five zero-velocity calls.  frame: (Phi, Q, augment, remove_previous), None for cov_zupt; hybrid:
        (idp_dim, n_feature_states); chk: the check's constants.  Returns the result dict, with the verdict's dict where there is a check."""
        keep = []   # Phi / Q stay alive across the call
        f = self._zupt_hybrid_struct(leg_dim, n_clones, r, noises, *(hybrid or (0, 0)), *(frame or (None, None, False, False)), keep)
        if hybrid is None:   # the struct nests the frame's, which nests the update's
            f = f.frame if frame is not None else f.frame.zupt
        if hybrid is not None:   # the features have left in front of K r
            nu = int(leg_dim) + 6 * int(n_clones)
        else:
            n = C.c_int32(0)
            self._chk(self.lib.orcvio_msckf_cov_get(self.h, C.byref(n), None), 'orcvio_msckf_cov_get')
            nu = n.value + (6 if frame is not None and frame[2] else 0)
        dx = np.zeros(max(nu, 1))
        applied, n_after, out = C.c_int32(-1), C.c_int32(-1), ZuptVerdict()
        args = [self.h, C.byref(f)] + ([C.byref(chk)] if chk is not None else []) + [_d(dx), C.byref(applied)] + \
            ([C.byref(n_after)] if frame is not None else []) + ([C.byref(out)] if chk is not None else [])
        rc = getattr(self.lib, name)(*args)
        if rc != 0 and (raise_on_refusal or rc != 6):
            raise MsckfError(rc, name)
        res = dict(dx=dx[:nu], applied=int(applied.value))
        if frame is not None:
            res['n_after'] = int(n_after.value)
        res['rc'] = rc
        return (res, self._verdict(out, rc)) if chk is not None else res

    def cov_zupt(self, leg_dim, n_clones, r, noises, raise_on_refusal=True):
        """orcvio_msckf_cov_zupt: measurementUpdate_ZUPT_vpq on the resident covariance (its factor kept).  r [9]; noises: the three
        VARIANCES (v, p, q).  Returns dict(dx [n], applied, rc)."""
        return self._zupt_call('orcvio_msckf_cov_zupt', leg_dim, n_clones, r, noises, raise_on_refusal)

    def cov_zupt_frame(self, leg_dim, n_clones, r, noises, Phi=None, Q=None, augment=True, remove_previous=True, raise_on_refusal=True):
        """orcvio_msckf_cov_zupt_frame: one stationary frame in one call (propagate, augment, the zero-velocity update, the previous
        clone marginalised).  n_clones: the window AFTER the augmentation.  Returns dict(dx, applied, n_after, rc)."""
        return self._zupt_call('orcvio_msckf_cov_zupt_frame', leg_dim, n_clones, r, noises, raise_on_refusal, (Phi, Q, augment, remove_previous))

    @staticmethod
    def zupt_check(use_left=0, **over):
        """orcvio_msckf_zupt_check with the reference's constants (orcvio_msckf_zupt_check_default); keywords override fields."""
        c = ZuptCheck()
        load().orcvio_msckf_zupt_check_default(C.byref(c))
        c.use_left_perturbation = int(use_left)
        for k, v in over.items():
            setattr(c, k, v)
        return c

    @staticmethod
    def _verdict(v, rc):
        return dict(rc=int(rc), evaluated=int(v.evaluated), accept=int(v.accept), dof=int(v.dof), status=int(v.status), chi2=float(v.chi2),
                    chi2_check=float(v.chi2_check), speed=float(v.speed))

    def cov_zupt_check_imu(self, chk, R_b2w, v, acc_bias, gravity, samples, raise_on_refusal=True):
        """orcvio_msckf_cov_zupt_check_imu: checkZUPTIMU on the resident covariance as it stands.  samples [S][7] (t | gyro | acc): the
        selected ones.  Returns dict(rc, evaluated, accept, dof, status, chi2, chi2_check, speed)."""
        smp = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 7)
        arr = [np.ascontiguousarray(x, dtype=np.float64).reshape(k) for x, k in ((R_b2w, 9), (v, 3), (acc_bias, 3), (gravity, 3))]
        out = ZuptVerdict()
        rc = self.lib.orcvio_msckf_cov_zupt_check_imu(self.h, C.byref(chk), _d(arr[0]), _d(arr[1]), _d(arr[2]), _d(arr[3]),
                                                      _d(smp) if smp.size else None, smp.shape[0], C.byref(out))
        if rc != 0 and (raise_on_refusal or rc != 6):
            raise MsckfError(rc, 'orcvio_msckf_cov_zupt_check_imu')
        return self._verdict(out, rc)

    def cov_propagate_imu_checked(self, cfg, state, prev_meas, samples, time_bound, chk, want_PhiQ=False, raise_on_refusal=True):
        """orcvio_msckf_cov_propagate_imu_checked: cov_propagate_imu with the zero-velocity check on the propagated covariance behind it,
        one wait.  Returns (the dict of cov_propagate_imu, the dict of cov_zupt_check_imu)."""
        smp = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 7)
        assert isinstance(prev_meas, np.ndarray) and prev_meas.dtype == np.float64 and prev_meas.size == 6 and prev_meas.flags.c_contiguous
        info = ImuInfo()
        info.wait = 1
        Phi = np.zeros((22, 22)) if want_PhiQ else None
        Q = np.zeros((22, 22)) if want_PhiQ else None
        out = ZuptVerdict()
        rc = self.lib.orcvio_msckf_cov_propagate_imu_checked(self.h, C.byref(cfg), C.byref(state), _d(prev_meas), _d(smp) if smp.size else None,
                                                             smp.shape[0], float(time_bound), C.byref(info), _d(Phi) if want_PhiQ else None,
                                                             _d(Q) if want_PhiQ else None, C.byref(chk), C.byref(out))
        if rc != 0 and (raise_on_refusal or rc != 6):
            raise MsckfError(rc, 'orcvio_msckf_cov_propagate_imu_checked')
        return (dict(status=int(rc), n_used=int(info.n_used), n_propagated=int(info.n_propagated), dt=float(info.dt),
                     mean_sforce=np.array(info.mean_sforce[:]), applied=int(info.applied), Phi=Phi, Q=Q), self._verdict(out, rc))

    def cov_zupt_frame_checked(self, chk, leg_dim, n_clones, r, noises, augment=True, remove_previous=True, raise_on_refusal=True):
        """orcvio_msckf_cov_zupt_frame_checked: the stationary frame on a handle armed by io_propagate_imu, the zero-velocity check in
        front of its update, one wait.  Returns (dict(dx, applied, n_after, rc), the dict of cov_zupt_check_imu)."""
        return self._zupt_call('orcvio_msckf_cov_zupt_frame_checked', leg_dim, n_clones, r, noises, raise_on_refusal,
                               (None, None, augment, remove_previous), chk=chk)

    def cov_zupt_frame_hybrid(self, leg_dim, n_clones, r, noises, idp_dim, n_feature_states, Phi=None, Q=None, augment=True,
                              remove_previous=True, raise_on_refusal=True):
        """orcvio_msckf_cov_zupt_frame_hybrid: one stationary frame of a hybrid filter in one call -- every in-state feature leaves in
        front of the update, the previous clone behind it, one fused launch.  Returns dict(dx [leg + 6 n_clones], applied, n_after, rc)."""
        return self._zupt_call('orcvio_msckf_cov_zupt_frame_hybrid', leg_dim, n_clones, r, noises, raise_on_refusal,
                               (Phi, Q, augment, remove_previous), (idp_dim, n_feature_states))

    def cov_zupt_frame_checked_hybrid(self, chk, leg_dim, n_clones, r, noises, idp_dim, n_feature_states, augment=True, remove_previous=True,
                                      raise_on_refusal=True):
        """orcvio_msckf_cov_zupt_frame_checked_hybrid: the hybrid stationary frame on a handle armed by io_propagate_imu, the
        zero-velocity check in front of its fused update, one wait.  Returns (dict(dx, applied, n_after, rc), the verdict's dict)."""
        return self._zupt_call('orcvio_msckf_cov_zupt_frame_checked_hybrid', leg_dim, n_clones, r, noises, raise_on_refusal,
                               (None, None, augment, remove_previous), (idp_dim, n_feature_states), chk)

    def set_object_dof_rank(self, on: bool):
        """ORCVIO_OPT_OBJECT_DOF: 1 = the object gate counts rows - rank(H_f) degrees of freedom (default rows - columns)."""
        self._chk(self.lib.orcvio_msckf_set_option(self.h, 11, int(bool(on))), 'orcvio_msckf_set_option')

    def set_object_refine(self, mode: int):
        """ORCVIO_OPT_OBJECT_REFINE: 0 never, 1 objects with an ill-conditioned H_f (default), 2 every object take the explicit-basis projection."""
        self._chk(self.lib.orcvio_msckf_set_option(self.h, 13, int(mode)), 'orcvio_msckf_set_option')

    def objects_refined(self) -> int:
        """Objects of the last downloaded object update that took the explicit-basis projection."""
        c = C.c_int32(0)
        self.lib.orcvio_msckf_objects_refined.argtypes = [C.c_void_p, _ip]
        self._chk(self.lib.orcvio_msckf_objects_refined(self.h, C.byref(c)), 'orcvio_msckf_objects_refined')
        return int(c.value)

    def set_ref_h2_ldlt(self, on: bool):
        """ORCVIO_OPT_REF_H2_LDLT: the reference's literal H_2.ldlt() in the tail of the hybrid update (default: triangular solve)."""
        self._chk(self.lib.orcvio_msckf_set_option(self.h, 12, int(bool(on))), 'orcvio_msckf_set_option')

    def set_schmidt_states(self, k):
        """ORCVIO_OPT_SCHMIDT_STATES: the last 6 k extra states are Schmidt nuisance states."""
        self._chk(self.lib.orcvio_msckf_set_option(self.h, 10, int(k)), 'orcvio_msckf_set_option')

    def upload_nuisance_poses(self, nui):
        """Poses of the nuisance states (synth.Window.nui-shaped dict), after upload()."""
        arrs = [np.ascontiguousarray(nui[k], dtype=np.float64) for k in ('R_b2w', 't_b_w', 't_fej', 'R_b2c', 't_c_b')]
        wn = MsckfWindow(arrs[0].shape[0], *[_d(a) for a in arrs])
        self._chk(self.lib.orcvio_msckf_upload_nuisance_poses(self.h, C.byref(wn)), 'orcvio_msckf_upload_nuisance_poses')

    def cov_commit_new_features(self):
        """After an update with upload_new_features: the resident covariance becomes the augmented one; returns dx_new."""
        k, d, _ = self._new
        dx_new = np.zeros(d * k)
        self.lib.orcvio_msckf_cov_commit_new_features.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._chk(self.lib.orcvio_msckf_cov_commit_new_features(self.h, _d(dx_new)), 'orcvio_msckf_cov_commit_new_features')
        return dx_new

    def cov_commit_new_features_fac(self):
        """As cov_commit_new_features, with the resident square-root factor carried along (S_aug = [[S+, 0], [-HH S+, sigma H_2^-1]])
        where the update's own commit would have kept S+ and the widened factor fits; returns dx_new."""
        k, d, _ = self._new
        dx_new = np.zeros(d * k)
        self.lib.orcvio_msckf_cov_commit_new_features_fac.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._chk(self.lib.orcvio_msckf_cov_commit_new_features_fac(self.h, _d(dx_new)), 'orcvio_msckf_cov_commit_new_features_fac')
        return dx_new

    def cov_prefactor(self):
        """Factor the resident covariance now (asynchronously): the next update finds its prior's square-root factor resident."""
        self._chk(self.lib.orcvio_msckf_cov_prefactor(self.h), 'orcvio_msckf_cov_prefactor')

    # -- feature triangulation (Feature::checkMotion + ::initializePosition) ---------------------
    def _tri_config(self, cfg=None):
        c = TriangulationConfig()
        self.lib.orcvio_msckf_triangulation_config_default(C.byref(c))
        if cfg is not None:   # any object / dict with the reference's OptimizationConfig field names
            get = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
            for k, _ in TriangulationConfig._fields_:
                try:
                    setattr(c, k, get(k))
                except (KeyError, AttributeError):
                    pass
        return c

    def triangulate(self, win, cfg=None, is_initialized=None):
        """Host-buffer call: returns dict(valid, p_w, solution, flags, cost) over the tracks of ``win``."""
        _, w, t, arrs = self._structs(win)
        c = self._tri_config(cfg)
        F = win.F
        ini = None if is_initialized is None else np.ascontiguousarray(is_initialized, dtype=np.int32)
        if ini is None:
            t.p_w = None
        out = dict(valid=np.zeros(max(F, 1), np.int32), p_w=np.zeros((max(F, 1), 3)), solution=np.zeros((max(F, 1), 3)),
                   flags=np.zeros(max(F, 1), np.int32), cost=np.zeros(max(F, 1)))
        res = TriangulationResult(_i(out['valid']), _d(out['p_w']), _d(out['solution']), _i(out['flags']), _d(out['cost']))
        rc = self.lib.orcvio_msckf_triangulate(self.h, C.byref(c), C.byref(w), C.byref(t), _i(ini), C.byref(res))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_triangulate')
        return {k: v[:F] for k, v in out.items()}

    def triangulate_uploaded(self, cfg=None, is_initialized=None, stream=None):
        """Triangulates the uploaded tracks in place on the device; invalid ones are excluded from the update."""
        c = self._tri_config(cfg)
        ini = None if is_initialized is None else np.ascontiguousarray(is_initialized, dtype=np.int32)
        rc = self.lib.orcvio_msckf_triangulate_uploaded(self.h, C.byref(c), _i(ini), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_triangulate_uploaded')

    def run_update(self, stream=None):
        rc = self.lib.orcvio_msckf_run_update(self.h, C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_run_update')

    def run_local(self, stream=None):
        rc = self.lib.orcvio_msckf_run_local(self.h, C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_run_local')

    def run_local_to(self, d_dst, stream=None):
        rc = self.lib.orcvio_msckf_run_local_to(self.h, C.c_void_p(d_dst), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_run_local_to')

    def block_ptr(self):
        p = C.c_void_p()
        ne = C.c_int64()
        rc = self.lib.orcvio_msckf_block_ptr(self.h, C.byref(p), C.byref(ne))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_block_ptr')
        return p.value, ne.value

    def run_finish(self, d_blocks, n_blocks, stream=None):
        rc = self.lib.orcvio_msckf_run_finish(self.h, C.c_void_p(d_blocks), n_blocks,
                                              C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_run_finish')

    def sync(self, stream=None):
        rc = self.lib.orcvio_msckf_sync(self.h, C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_sync')

    def download(self, want_K=False, want_G=False, want_thin=False):
        out, res = self._result(self.n, self.F, want_K, want_G, want_thin)
        rc = self.lib.orcvio_msckf_download(self.h, C.byref(res))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_download')
        return self._finish(out, res, self.F)

    def download_dx(self):
        """dx alone of the finished update (P+ stays in HBM: orcvio_msckf_cov_commit makes it the resident covariance)."""
        if getattr(self, '_dx_n', None) != self.n:
            self._dx_buf = np.zeros(self.n)
            self._dx_res = MsckfResult(_d(self._dx_buf), None, None, None, None, None, None, None)
            self._dx_n = self.n
        rc = self.lib.orcvio_msckf_download(self.h, C.byref(self._dx_res))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_download')
        return self._dx_buf

    def set_stage_profile(self, on: bool):
        """ORCVIO_OPT_STAGE_PROFILE: HIP events between the stages of the object update."""
        self._chk(self.lib.orcvio_msckf_set_option(self.h, 6, int(bool(on))), 'orcvio_msckf_set_option')

    def profile_stages(self):
        """[(stage, ms)] of the last object update run with the stage profile on."""
        names = (C.c_char_p * 32)()
        ms = (C.c_double * 32)()
        cnt = C.c_int32(32)
        self.lib.orcvio_msckf_profile_stages.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), _dp, C.POINTER(C.c_int32)]
        self._chk(self.lib.orcvio_msckf_profile_stages(self.h, names, ms, C.byref(cnt)), 'orcvio_msckf_profile_stages')
        return [(names[i].decode(), ms[i]) for i in range(cnt.value)]

    def profile(self, reps=20, stream=None):
        names = (C.c_char_p * 16)()
        ms = (C.c_double * 16)()
        cnt = C.c_int32(16)
        rc = self.lib.orcvio_msckf_profile_update(self.h, C.c_void_p(stream) if stream else None, reps, names, ms,
                                                  C.byref(cnt))
        if rc != 0:
            raise MsckfError(rc, 'orcvio_msckf_profile_update')
        return {names[i].decode(): ms[i] for i in range(cnt.value)}


def new_feature_rows(win, idp_dim, feats):
    """Host arithmetic (no device): featureJacobian_ekf_new + the W = [V | U] split for features entering the state.
    feats: objects with anchor, inv_param / obs_anchor / inv_depth, p_w, p_fej (optional), obs = [(clone, z, z_vel)].
    Returns (H_top [rows, n], r_top, H_1 [d k, n], H_2 [k, d, d], r_1)."""
    lib = load()
    fl = make_flags(win.flags)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (win.R_b2w, win.t_b_w, win.t_fej, win.R_b2c, win.t_c_b)]
    wn = MsckfWindow(win.N, *[_d(a) for a in arrs])
    k, d, n = len(feats), int(idp_dim), win.n
    ptr, cl, zz, zv = [0], [], [], []
    for ft in feats:
        for (c, z, v) in ft.obs:
            cl.append(c); zz.append(z); zv.append(v)
        ptr.append(len(cl))
    ia = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    da = lambda a, shape: np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
    anchor, obs_ptr, obs_clone = ia([f.anchor for f in feats]), ia(ptr), ia(cl)
    param = da([f.inv_param if d == 3 else f.obs_anchor for f in feats], (k, 3))
    rho = da([f.inv_depth for f in feats], (k,))
    pw = da([f.p_w for f in feats], (k, 3))
    pf = da([f.p_fej if f.p_fej is not None else f.p_w for f in feats], (k, 3))
    oz, ozv = da(zz, (-1, 2)), da(zv, (-1, 2))
    cap = 2 * len(cl)
    H_top, r_top = np.zeros((cap, n)), np.zeros(cap)
    H_1, H_2, r_1 = np.zeros((d * k, n)), np.zeros((k, d, d)), np.zeros(d * k)
    rows = C.c_int32(0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.orcvio_msckf_new_feature_rows(C.byref(fl), C.byref(wn), d, n, k, ip(anchor), _d(param), _d(rho), _d(pw), _d(pf), ip(obs_ptr),
                                           ip(obs_clone), _d(oz), _d(ozv), C.byref(rows), _d(H_top), _d(r_top), _d(H_1), _d(H_2), _d(r_1))
    if rc != 0:
        raise MsckfError(rc, 'orcvio_msckf_new_feature_rows')
    return H_top[:rows.value].copy(), r_top[:rows.value].copy(), H_1, H_2, r_1


def augment_state_nuisance(idp_dim, nui_rows, H_1, H_2, r_1, sigma2, dx, P_upd, ref_ldlt=False):
    """Host arithmetic: augment_state with nui_rows Schmidt nuisance rows at the end (new states go in front of them).
    ref_ldlt: the reference's literal H_2.ldlt() (orcvio_msckf_augment_state_ref_ldlt)."""
    lib = load()
    fn = lib.orcvio_msckf_augment_state_ref_ldlt if ref_ldlt else lib.orcvio_msckf_augment_state_nuisance
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                        C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                        C.POINTER(C.c_double), C.POINTER(C.c_double)]
    d, k, n = int(idp_dim), H_2.shape[0], P_upd.shape[0]
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (H_1, H_2, r_1, dx, P_upd)]
    dx_new = np.zeros(d * k)
    P_aug = np.zeros((n + d * k, n + d * k))
    rc = fn(n, k, d, int(nui_rows), _d(a[0]), _d(a[1]), _d(a[2]), float(sigma2), _d(a[3]), _d(a[4]), _d(dx_new), _d(P_aug))
    if rc != 0:
        raise MsckfError(rc, 'orcvio_msckf_augment_state_nuisance')
    return dx_new, P_aug


def augment_state(idp_dim, H_1, H_2, r_1, sigma2, dx, P_upd):
    """Host arithmetic (no device): dx_new and the augmented covariance of measurementUpdate_hybrid's tail."""
    lib = load()
    lib.orcvio_msckf_augment_state.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.POINTER(C.c_double)]
    d = int(idp_dim)
    k = H_2.shape[0]
    n = P_upd.shape[0]
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (H_1, H_2, r_1, dx, P_upd)]
    dx_new = np.zeros(d * k)
    P_aug = np.zeros((n + d * k, n + d * k))
    rc = lib.orcvio_msckf_augment_state(n, k, d, _d(a[0]), _d(a[1]), _d(a[2]), float(sigma2), _d(a[3]), _d(a[4]), _d(dx_new), _d(P_aug))
    if rc != 0:
        raise MsckfError(rc, 'orcvio_msckf_augment_state')
    return dx_new, P_aug


def increment_window(win, dx):
    """incrementState_IMUCam (orcvio_msckf_increment_state, host arithmetic) applied to the clone poses of a synth.Window: the
    window a caller flattens for the NEXT update of the frame.  Every clone keeps its own R_b2c / t_c_b (frozen at its
    augmentation; only the IMU's extrinsic moves, and it is not part of the window).  Returns (window, applied)."""
    import dataclasses
    N = win.N
    s = MsckfState()
    s.R_b2w_imu[:] = list(np.eye(3).reshape(-1))
    s.R_b2c[:] = list(np.ascontiguousarray(win.R_b2c[0]).reshape(-1))
    s.t_c_b[:] = list(win.t_c_b[0])
    s.n_clones = N
    R = np.ascontiguousarray(win.R_b2w, dtype=np.float64).copy()
    t = np.ascontiguousarray(win.t_b_w, dtype=np.float64).copy()
    s.clone_R_b2w = _d(R); s.clone_t_b_w = _d(t)
    fl = make_flags(win.flags)
    dxc = np.ascontiguousarray(dx, dtype=np.float64)
    rc = load().orcvio_msckf_increment_state(C.byref(fl), _d(dxc), C.byref(s))
    if rc < 0:
        raise MsckfError(1, 'orcvio_msckf_increment_state')
    return dataclasses.replace(win, R_b2w=R, t_b_w=t, R_b2c=np.ascontiguousarray(win.R_b2c, dtype=np.float64).copy(),
                               t_c_b=np.ascontiguousarray(win.t_c_b, dtype=np.float64).copy()), rc == 1


def _rotation_to_quaternion(R):
    """The reference's rotationToQuaternion (math_utils.hpp): (x, y, z, w), Hamilton, scalar part >= 0."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    k = int(np.argmax([R[0, 0], R[1, 1], R[2, 2], tr]))
    q = np.zeros(4)
    if k == 3:
        q[3] = np.sqrt(1.0 + tr) / 2.0
        q[:3] = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4.0 * q[3])
    else:
        a, b = (k + 1) % 3, (k + 2) % 3
        q[k] = np.sqrt(1.0 + 2.0 * R[k, k] - tr) / 2.0
        q[a] = (R[k, a] + R[a, k]) / (4.0 * q[k])
        q[b] = (R[k, b] + R[b, k]) / (4.0 * q[k])
        q[3] = (R[b, a] - R[a, b]) / (4.0 * q[k])
    if q[3] < 0:
        q = -q
    return q / np.linalg.norm(q)


def zupt_check_feat(dis, max_dis):
    """orcvio_msckf_zupt_check_feat: checkZUPTFeat's decision on the pixel distances of the tracked features.  Returns
    dict(accept, kth); raises MsckfError on a refusal."""
    d = np.ascontiguousarray(dis, dtype=np.float64).reshape(-1)
    accept, kth = C.c_int32(-1), np.zeros(1)
    rc = load().orcvio_msckf_zupt_check_feat(_d(d) if d.size else None, int(d.size), float(max_dis), C.byref(accept), _d(kth))
    if rc != 0:
        raise MsckfError(rc, 'orcvio_msckf_zupt_check_feat')
    return dict(accept=int(accept.value), kth=float(kth[0]))


def zupt_residual(v, R_prev, p_prev, R_cur, p_cur):
    """r [9] of the zero-velocity update as measurementUpdate_ZUPT_vpq forms it (src/orcvio.cpp:3337-3368): -v, -(p_cur - p_prev) and
    the vector part of q_cur (x) q_prev* (Hamilton quaternions of the two newest clones' orientations, rotationToQuaternion).
    Pure numpy: no device, no library call."""
    qc, qp = _rotation_to_quaternion(R_cur), _rotation_to_quaternion(R_prev)
    vc, wc, vp, wp = qc[:3], qc[3], -qp[:3], qp[3]   # (q_prev conjugated)
    r = np.zeros(9)
    r[0:3] = -np.asarray(v, dtype=np.float64)
    r[3:6] = -(np.asarray(p_cur, dtype=np.float64) - np.asarray(p_prev, dtype=np.float64))
    r[6:9] = wc * vp + wp * vc + np.cross(vc, vp)
    return r


def chi2_quantile(dof, prob=0.95):
    return float(load().orcvio_msckf_chi2_quantile(int(dof), float(prob)))


def debug_read(upd: MsckfUpdater, which: str):
    """Test helper: copies an intermediate device buffer of the last run to the host."""
    lib = upd.lib
    lib.orcvio_msckf_debug_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    dims = np.zeros(8, dtype=np.int32)
    rc = lib.orcvio_msckf_debug_read(upd.h, 7, dims.ctypes.data_as(C.c_void_p), dims.nbytes)
    if rc != 0:
        raise MsckfError(rc, 'debug_read dims')
    n, NA, NAP, NP, m_tot = (int(x) for x in dims[:5])
    ldz = int(dims[6])
    if which == 'dims':
        return dict(n=n, NA=NA, NAP=NAP, NP=NP, m_tot=m_tot, Mmax=int(dims[5]), ldz=ldz, reg_path=int(dims[7]))
    if which == 'obj_fused':   # did the last object update take the one-launch compression (k_obj_fused)?
        v = np.zeros(1, dtype=np.int32)
        rc = lib.orcvio_msckf_debug_read(upd.h, 15, v.ctypes.data_as(C.c_void_p), v.nbytes)
        if rc != 0:
            raise MsckfError(rc, 'debug_read obj_fused')
        return int(v[0])
    if which == 'dense':   # [dense_rows][NAP]: H(:, 15 : 15 + NA) | r | 0 -- the rows handed over, then those of the entering features
        dd = np.zeros(2, dtype=np.int32)
        rc = lib.orcvio_msckf_debug_read(upd.h, 14, dd.ctypes.data_as(C.c_void_p), dd.nbytes)
        if rc != 0:
            raise MsckfError(rc, 'debug_read dense dims')
        out = np.zeros((int(dd[0]), int(dd[1])))
        if out.size:
            rc = lib.orcvio_msckf_debug_read(upd.h, 13, out.ctypes.data_as(C.c_void_p), out.nbytes)
            if rc != 0:
                raise MsckfError(rc, 'debug_read dense')
        return out
    if which in ('front', 'T3', 'Xobs', 'obs_pos', 'S', 'Gpart'):   # the front end of the last feature update as its launches left it
        st = np.zeros(8, dtype=np.int32)
        rc = lib.orcvio_msckf_debug_read(upd.h, 22, st.ctypes.data_as(C.c_void_p), st.nbytes)
        if rc != 0:
            raise MsckfError(rc, 'debug_read front')
        F, N, nobs, chunks = (int(x) for x in st[:4])
        if which == 'front':   # (fused: this upload takes k_front; deferred: k_front left the Grams only and A is assembled on demand)
            return dict(F=F, N=N, nobs=nobs, chunks=chunks, rows_per_chunk=int(st[4]), fused=int(st[5]), deferred=int(st[6]),
                        prior_forked=int(st[7]))
        code, shape, dt = {'T3': (17, (3 * F, NAP), np.float64), 'Xobs': (18, (2 * nobs, 16), np.float64),
                           'obs_pos': (19, (nobs,), np.int32), 'S': (20, (N, 16, 16), np.float64),
                           'Gpart': (21, (chunks, NAP, NAP), np.float64)}[which]
        out = np.zeros(shape, dtype=dt)
        if out.size:
            rc = lib.orcvio_msckf_debug_read(upd.h, code, out.ctypes.data_as(C.c_void_p), out.nbytes)
            if rc != 0:
                raise MsckfError(rc, f'debug_read {which}')
        return out
    shapes = {'Hs': (0, (m_tot, NAP)), 'Ab': (1, (NAP, NAP)), 'A': (2, (NAP, NAP)), 'RP': (3, (NP, NP)),
              'M': (4, (NP, NP)), 'RM': (5, (NP, NP)), 'Z': (6, (n, ldz)), 'U': (8, (NP, NP)),
              'P': (16, (n, n))}   # (the prior as its pull left it in device memory)
    code, shape = shapes[which]
    out = np.zeros(shape)
    if out.size:
        rc = lib.orcvio_msckf_debug_read(upd.h, code, out.ctypes.data_as(C.c_void_p), out.nbytes)
        if rc != 0:
            raise MsckfError(rc, f'debug_read {which}')
    return out


def debug_factor_state(upd: MsckfUpdater):
    """Test helper (diagnostics build): dict(fac_valid, fac_n, fac_k, res_n) of the resident covariance and its factor."""
    lib = upd.lib
    lib.orcvio_msckf_debug_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    st = np.zeros(4, dtype=np.int32)
    rc = lib.orcvio_msckf_debug_read(upd.h, 11, st.ctypes.data_as(C.c_void_p), st.nbytes)
    if rc != 0:
        raise MsckfError(rc, 'debug_read factor state')
    return dict(fac_valid=int(st[0]), fac_n=int(st[1]), fac_k=int(st[2]), res_n=int(st[3]))


def debug_factor(upd: MsckfUpdater):
    """Test helper (diagnostics build): the resident square-root factor S [fac_n, fac_k] (P = S S^T)."""
    st = debug_factor_state(upd)
    out = np.zeros((st['fac_k'], st['fac_n']))
    rc = upd.lib.orcvio_msckf_debug_read(upd.h, 12, out.ctypes.data_as(C.c_void_p), out.nbytes)
    if rc != 0:
        raise MsckfError(rc, 'debug_read factor')
    return out.T.copy()


def debug_potrf(upd: MsckfUpdater, X, tol_rel=0.0, force_lds_path=False, rev=False):
    """Test helper: Cholesky factor (lower), block inverses and pivot info of a host matrix.  rev: the matrix is factored reversed, as
    the update factors its prior (X'(i, j) = X(n-1-i, n-1-j)); L is then the factor L' of X' as stored, and S(i, c) = L'(n-1-i, c)
    has S S^T = X."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    L = np.zeros((n, n))
    nb = (n + 15) // 16
    Dinv = np.zeros((nb, 16, 16))
    info = np.zeros(2, dtype=np.int32)
    lib = upd.lib
    lib.orcvio_msckf_debug_potrf.argtypes = [C.c_void_p, _dp, C.c_int32, C.c_double, C.c_int32, _dp, _dp, _ip, C.c_int32]
    rc = lib.orcvio_msckf_debug_potrf(upd.h, _d(X), n, float(tol_rel), int(force_lds_path), _d(L), _d(Dinv), _i(info), int(bool(rev)))
    if rc != 0:
        raise MsckfError(rc, 'debug_potrf')
    return L, Dinv, info


def debug_trsm(upd: MsckfUpdater, X, B):
    """Test helper: Z = chol(X)^-1 B."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    n, nrhs = B.shape
    Z = np.zeros((n, nrhs))
    lib = upd.lib
    lib.orcvio_msckf_debug_trsm.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, C.c_int32, _dp]
    rc = lib.orcvio_msckf_debug_trsm(upd.h, _d(X), n, _d(B), nrhs, _d(Z))
    if rc != 0:
        raise MsckfError(rc, 'debug_trsm')
    return Z


def debug_potrf_solve(upd: MsckfUpdater, X, B, la=0, stamps=False, reps=0, bx=None, tail=0, tail_scale=0.0, product_strides=False):
    """Test helper / diagnostic: L = chol(X) and Z = L^-1 [B | bx] in ONE launch -- k_potrf_solve (la = 0) or k_potrf_solve_la
    (la = 2, 3: the trailing update spread over far workgroups) -- in the argument forms of the update's own call: X is n x n, B is
    (n + tail) x nc1; bx (n values) is one more column behind B; the `tail` rows of B behind the first n come back as tail_scale * B
    (zero in bx's column); product_strides lays B out on the device as the update finds the prior's factor (row stride = the leading
    dimension, columns in reverse order through a column stride of -1, the base at the last column).
    Returns dict(L, Z [n + tail, nc1 + (bx is not None)], info[dropped, non-positive, lost], stamps, us, guard_row, guard_col: the row and
    the column of the NaN-filled scratch just outside Z as the launch left them, outside: entries of the whole scratch outside Z that
    are no longer NaN)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    n = X.shape[0]
    tail = int(tail)
    if X.shape != (n, n) or B.ndim != 2 or B.shape[0] != n + tail:
        raise ValueError('debug_potrf_solve: X is n x n and B is (n + tail) x nc1')
    nrhs = B.shape[1]
    if bx is not None:
        bx = np.ascontiguousarray(bx, dtype=np.float64).ravel()
        if bx.size != n:
            raise ValueError('debug_potrf_solve: bx has n values')
    ncols = nrhs + (bx is not None)
    L = np.zeros((n, n))
    Zg = np.zeros((n + tail + 1, ncols + 1))
    info = np.zeros(3, dtype=np.int32)
    outside = C.c_int32(-1)
    st = np.zeros(512, dtype=np.uint64)
    us = C.c_double(0.0)
    lib = upd.lib
    lib.orcvio_msckf_debug_potrf_solve.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, C.c_int32, C.c_int32, _dp, _dp, C.c_void_p, C.c_void_p,
                                                   C.c_int32, C.POINTER(C.c_double), _dp, C.c_int32, C.c_double, C.c_int32,
                                                   C.POINTER(C.c_int32)]
    rc = lib.orcvio_msckf_debug_potrf_solve(upd.h, _d(X), n, _d(B), nrhs, int(la), _d(L), _d(Zg), info.ctypes.data,
                                            st.ctypes.data if stamps else None, int(reps), C.byref(us),
                                            _d(bx) if bx is not None else None, tail, float(tail_scale), int(bool(product_strides)),
                                            C.byref(outside))
    if rc != 0:
        raise MsckfError(rc, 'debug_potrf_solve')
    return dict(L=L, Z=np.ascontiguousarray(Zg[:n + tail, :ncols]), info=info, stamps=st.astype(np.int64) if stamps else None, us=us.value,
                guard_row=Zg[n + tail, :].copy(), guard_col=Zg[:, ncols].copy(), outside=int(outside.value))
