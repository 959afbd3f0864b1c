"""lisreg — thin ctypes binding of liblisreg.so (include/lisreg.h), used by tests/, bench.py and smoke().

The product is the C-ABI shared library built from lis-slam_amd/csrc (hand-written HIP for gfx950); this module
only marshals numpy arrays of PCL point structs (the reference's host layout, src/include/common.h:9,25-35)
and device pointers across that boundary.  It has NO compute of its own and NO CPU fallback: if the shared
library is missing or no HIP device is visible, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "liblisreg.so")
CSRC = os.path.join(_PKG, "csrc")

OK, NOT_ENOUGH_FEATURES, TOO_FEW_CORRESPONDENCES, LEAF_TOO_SMALL = 0, 1, 2, 3
ERR_ARG, ERR_HIP, ERR_NO_TARGET, ERR_NOMEM, ERR_COMM = -1, -2, -3, -4, -5
FMT_XYZI, FMT_XYZIL, FMT_DEVICE, FMT_XYZIRT, FMT_DEVICE_XYZI, FMT_XYZI_PACKED = 0, 1, 2, 3, 4, 5
VARIANT_ODOM, VARIANT_KEYFRAME, VARIANT_SUBMAP = 1, 2, 3
TRACE_STRIDE = 56
RESULT_SIZE = 12
SOLVE_STATE_STRIDE = 56

# every symbol include/lisreg.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "lisreg_device_count", "lisreg_create", "lisreg_destroy", "lisreg_last_error", "lisreg_set_stream",
    "lisreg_get_stream", "lisreg_default_params", "lisreg_set_target", "lisreg_set_target_slot",
    "lisreg_target_from_classes", "lisreg_align", "lisreg_align_batch", "lisreg_batch_prepare", "lisreg_batch_run",
    "lisreg_batch_fetch", "lisreg_stage_host_items", "lisreg_upload_cloud", "lisreg_concat_device", "lisreg_batch_result_device", "lisreg_set_option", "lisreg_get_option", "lisreg_get_counters", "lisreg_get_neighbors", "lisreg_get_partial_rows", "lisreg_test_fit_models", "lisreg_test_solve_steps", "lisreg_test_nn1", "lisreg_test_scan", "lisreg_get_map_grid", "lisreg_get_target_index", "lisreg_get_target_graph", "lisreg_get_target_cell_rows", "lisreg_keyframes_reset", "lisreg_keyframes_push", "lisreg_keyframes_target", "lisreg_get_trace",
    "lisreg_set_profiling", "lisreg_get_timing", "lisreg_pose_to_matrix", "lisreg_transform_update",
    "lisreg_comm_unique_id", "lisreg_comm_init", "lisreg_gather_results", "lisreg_comm_destroy",
    "lisreg_voxel_downsample", "lisreg_voxel_downsample_multi", "lisreg_voxel_downsample_batch", "lisreg_transform_cloud",
    "lisreg_extract_features", "lisreg_extract_features_deskew", "lisreg_extract_features_batch", "lisreg_default_feature_params", "lisreg_semantic_split",
    "lisreg_semantic_split_batch", "lisreg_concat_device_batch",
    "lisreg_map_index_set", "lisreg_map_index_set_batch", "lisreg_nearest", "lisreg_dynamic_filter", "lisreg_bbx_filter", "lisreg_cloud_bounds",
    "lisreg_localmap_default_params", "lisreg_localmap_reset", "lisreg_localmap_insert", "lisreg_localmap_extract",
    "lisreg_localmap_get", "lisreg_predict_pose", "lisreg_guess_state_init", "lisreg_update_initial_guess", "lisreg_submap_insert", "lisreg_submap_extract", "lisreg_submap_crop_boxes",
    "lisreg_default_gather_params", "lisreg_submap_gather_count", "lisreg_submap_gather",
    "lisreg_icp_default_params", "lisreg_icp_align", "lisreg_icp_align_batch", "lisreg_icp_gn_match", "lisreg_icp_gn_match_batch",
    "lisreg_loopdet_default_params", "lisreg_loopdet_reset", "lisreg_loopdet_detect", "lisreg_loopdet_candidates",
    "lisreg_loopdet_get", "lisreg_loop_descriptor",
    "lisreg_loopdet_configure", "lisreg_loopdet_matches", "lisreg_loopdet_candidate_scores", "lisreg_loopdet_get_descriptor",
    "lisreg_loop_descriptor_kind",
    "lisreg_default_pretreat_params", "lisreg_pretreat", "lisreg_pretreat_batch",
    "lisreg_extract_features_deskew_batch", "lisreg_default_motion", "lisreg_adjust_cloud", "lisreg_adjust_cloud_batch",
    "lisreg_default_rangenet_params", "lisreg_rangenet_project", "lisreg_rangenet_project_batch", "lisreg_rangenet_label",
    "lisreg_rangenet_label_batch",
    "lisreg_default_rangenet_knn_params", "lisreg_rangenet_knn_weights", "lisreg_rangenet_label_knn", "lisreg_rangenet_label_knn_batch",
    "lisreg_ndt_default_params", "lisreg_ndt_set_target", "lisreg_ndt_align", "lisreg_ndt_get_voxels", "lisreg_ndt_derivatives",
    "lisreg_ndt_align_batch", "lisreg_ndt_set_target_batch", "lisreg_ndt_get_target", "lisreg_ndt_target_batch_counts",
    "lisreg_vgicp_default_params", "lisreg_vgicp_set_target", "lisreg_vgicp_align", "lisreg_vgicp_covariances", "lisreg_vgicp_get_voxels",
    "lisreg_vgicp_linearize", "lisreg_vgicp_align_batch", "lisreg_vgicp_set_target_batch", "lisreg_vgicp_get_target",
    "lisreg_vgicp_target_batch_counts",
    "lisreg_fgicp_default_params", "lisreg_fgicp_set_target", "lisreg_fgicp_align", "lisreg_fgicp_correspondences", "lisreg_fgicp_linearize",
    "lisreg_fgicp_align_batch", "lisreg_fgicp_set_target_batch", "lisreg_fgicp_get_target", "lisreg_fgicp_grid_geometry",
    "lisreg_fgicp_target_batch_counts",
    "lisreg_gicp_default_params", "lisreg_gicp_align", "lisreg_gicp_moments", "lisreg_gicp_inner", "lisreg_gicp_align_batch",
]


ICP_NOT_CONVERGED, ICP_ITERATIONS, ICP_TRANSFORM, ICP_ABS_MSE, ICP_REL_MSE, ICP_NO_CORRESPONDENCES = range(6)


class IcpParams(C.Structure):
    _fields_ = [("max_corr_dist", C.c_double), ("max_iters", C.c_int), ("reserved", C.c_int),
                ("transformation_epsilon", C.c_double), ("euclidean_fitness_epsilon", C.c_double), ("prev_mse", C.c_double)]


class IcpResult(C.Structure):
    _fields_ = [("final_transform", C.c_float * 16), ("converged", C.c_int), ("iters", C.c_int), ("state", C.c_int),
                ("n_corr_last", C.c_int), ("fitness", C.c_double), ("prev_mse", C.c_double)]

    def as_dict(self):
        return dict(T=np.array(list(self.final_transform), np.float32).reshape(4, 4), converged=bool(self.converged),
                    iters=self.iters, state=self.state, n_corr_last=self.n_corr_last, fitness=self.fitness, prev_mse=self.prev_mse)


class NdtParams(C.Structure):
    _fields_ = [("resolution", C.c_double), ("step_size", C.c_double), ("transformation_epsilon", C.c_double),
                ("outlier_ratio", C.c_double), ("min_covar_eigvalue_mult", C.c_double), ("max_iters", C.c_int),
                ("min_points_per_voxel", C.c_int), ("line_search", C.c_int), ("reserved", C.c_int)]


class NdtInfo(C.Structure):
    _fields_ = [("dims", C.c_int * 3), ("n_voxels", C.c_int), ("n_valid", C.c_int), ("reserved", C.c_int)]


class NdtTargetJob(C.Structure):
    """lisreg_ndt_target_job"""
    _fields_ = [("slot", C.c_int), ("n", C.c_int), ("cloud", C.c_void_p), ("status", C.c_int), ("info", NdtInfo)]


NDT_TARGET_BATCH_MAX = 1024
NDT_TARGET_BATCH_MAX_POINTS = 1 << 27


class NdtResult(C.Structure):
    _fields_ = [("final_transform", C.c_float * 16), ("p", C.c_double * 6), ("converged", C.c_int), ("iters", C.c_int),
                ("n_evals", C.c_int), ("reserved", C.c_int), ("n_pairs_last", C.c_longlong), ("score", C.c_double),
                ("trans_probability", C.c_double)]

    def as_dict(self):
        return dict(T=np.array(list(self.final_transform), np.float32).reshape(4, 4), p=np.array(list(self.p)),
                    converged=bool(self.converged), iters=self.iters, n_evals=self.n_evals, n_pairs_last=self.n_pairs_last,
                    score=self.score, trans_probability=self.trans_probability)


class VgicpParams(C.Structure):
    _fields_ = [("resolution", C.c_double), ("transformation_epsilon", C.c_double), ("rotation_epsilon", C.c_double),
                ("lm_init_lambda_factor", C.c_double), ("plane_epsilon", C.c_double), ("k_correspondences", C.c_int),
                ("max_iters", C.c_int), ("lm_max_iterations", C.c_int), ("reserved", C.c_int)]

    # neighbor_search (§7w) is the struct's last int, whose member is named `reserved` in include/lisreg.h and here
    @property
    def neighbor_search(self) -> int:
        """0 or VGICP_DIRECT1, VGICP_DIRECT7, VGICP_DIRECT27: the voxel neighbourhood of an alignment"""
        return self.reserved

    @neighbor_search.setter
    def neighbor_search(self, mode: int):
        self.reserved = int(mode)


VGICP_DIRECT1, VGICP_DIRECT7, VGICP_DIRECT27 = 1, 7, 27


class VgicpInfo(C.Structure):
    _fields_ = [("dims", C.c_int * 3), ("n_voxels", C.c_int), ("n_points", C.c_int)]


class VgicpTargetJob(C.Structure):
    """lisreg_vgicp_target_job"""
    _fields_ = [("slot", C.c_int), ("n", C.c_int), ("cloud", C.c_void_p), ("status", C.c_int), ("info", VgicpInfo)]


VGICP_TARGET_BATCH_MAX = 1024
VGICP_TARGET_BATCH_MAX_POINTS = 1 << 27


class VgicpResult(C.Structure):
    _fields_ = [("final_transform", C.c_double * 16), ("converged", C.c_int), ("iters", C.c_int), ("n_evals", C.c_int),
                ("n_rejected", C.c_int), ("n_pairs_last", C.c_longlong), ("error", C.c_double), ("lambda_", C.c_double)]

    def as_dict(self):
        return dict(T=np.array(list(self.final_transform), np.float64).reshape(4, 4), converged=bool(self.converged), iters=self.iters,
                    n_evals=self.n_evals, n_rejected=self.n_rejected, n_pairs_last=self.n_pairs_last, error=self.error,
                    lam=self.lambda_)


class FgicpParams(C.Structure):
    _fields_ = [("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double), ("rotation_epsilon", C.c_double),
                ("lm_init_lambda_factor", C.c_double), ("plane_epsilon", C.c_double), ("k_correspondences", C.c_int),
                ("max_iters", C.c_int), ("lm_max_iterations", C.c_int), ("reserved", C.c_int)]


class FgicpInfo(C.Structure):
    _fields_ = [("grid_dims", C.c_int * 3), ("n_points", C.c_int)]


class FgicpTargetJob(C.Structure):
    """lisreg_fgicp_target_job"""
    _fields_ = [("slot", C.c_int), ("n", C.c_int), ("cloud", C.c_void_p), ("cell_edge", C.c_float), ("status", C.c_int),
                ("info", FgicpInfo)]


FGICP_TARGET_BATCH_MAX = 1024
FGICP_TARGET_BATCH_MAX_POINTS = 1 << 27


class FgicpResult(VgicpResult):
    """the fields of VgicpResult, in the same order"""


class GicpParams(C.Structure):
    """lisreg_gicp_params"""
    _fields_ = [("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double), ("rotation_epsilon", C.c_double),
                ("gicp_epsilon", C.c_double), ("rho", C.c_double), ("sigma", C.c_double), ("tau1", C.c_double), ("tau2", C.c_double),
                ("tau3", C.c_double), ("step_size", C.c_double), ("gradient_tol", C.c_double), ("k_correspondences", C.c_int),
                ("max_iters", C.c_int), ("max_inner_iters", C.c_int), ("order", C.c_int)]


class GicpResult(C.Structure):
    """lisreg_gicp_result"""
    _fields_ = [("final_transform", C.c_double * 16), ("converged", C.c_int), ("iters", C.c_int), ("inner_iters", C.c_int),
                ("n_evals", C.c_int), ("n_rounds", C.c_int), ("inner_exit", C.c_int), ("n_pairs_last", C.c_longlong),
                ("error", C.c_double), ("last_delta", C.c_double)]

    def as_dict(self):
        return dict(T=np.array(list(self.final_transform), np.float64).reshape(4, 4), converged=bool(self.converged), iters=self.iters,
                    inner_iters=self.inner_iters, n_evals=self.n_evals, n_rounds=self.n_rounds, inner_exit=self.inner_exit,
                    n_pairs_last=self.n_pairs_last, error=self.error, last_delta=self.last_delta)


class FgicpItemC(C.Structure):
    """lisreg_fgicp_item"""
    _fields_ = [("source", C.c_int), ("slot", C.c_int), ("guess", C.POINTER(C.c_float))]


class FgicpBatchInfo(C.Structure):
    _fields_ = [("best", C.c_int), ("n_rounds", C.c_int), ("n_sources_staged", C.c_int), ("reserved", C.c_int)]


class FgicpItem:
    """one alignment of a batch: sources[source] against the FastGICP target in `slot` from `guess` (4x4 or None = identity)"""

    def __init__(self, source: int, slot: int, guess=None):
        self.source, self.slot = int(source), int(slot)
        self.guess = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(16).copy()


class VgicpItemC(FgicpItemC):
    """lisreg_vgicp_item: the fields of lisreg_fgicp_item, in the same order"""


class VgicpBatchInfo(FgicpBatchInfo):
    """lisreg_vgicp_batch_info: the fields of lisreg_fgicp_batch_info, in the same order"""


class VgicpItem(FgicpItem):
    """one alignment of a batch: sources[source] against the VGICP target in `slot` from `guess` (4x4 or None = identity)"""


class NdtItemC(FgicpItemC):
    """lisreg_ndt_item: the fields of lisreg_fgicp_item, in the same order"""


class NdtBatchInfo(FgicpBatchInfo):
    """lisreg_ndt_batch_info: the fields of lisreg_fgicp_batch_info, in the same order"""


class NdtItem(FgicpItem):
    """one alignment of a batch: sources[source] against the NDT target in `slot` from `guess` (4x4 or None = identity)"""


class GicpItemC(FgicpItemC):
    """lisreg_gicp_item: the fields of lisreg_fgicp_item, in the same order"""


class GicpBatchInfo(FgicpBatchInfo):
    """lisreg_gicp_batch_info: the fields of lisreg_fgicp_batch_info, in the same order"""


class GicpItem(FgicpItem):
    """one alignment of a batch: sources[source] against the FastGICP target in `slot` (PCL's GICP, §7r) from `guess` (4x4 or None = identity)"""


class GuessInput(C.Structure):
    _fields_ = [("odom_available", C.c_int), ("imu_available", C.c_int),
                ("imu_roll_init", C.c_float), ("imu_pitch_init", C.c_float), ("imu_yaw_init", C.c_float),
                ("initial_guess_x", C.c_float), ("initial_guess_y", C.c_float), ("initial_guess_z", C.c_float),
                ("initial_guess_roll", C.c_float), ("initial_guess_pitch", C.c_float), ("initial_guess_yaw", C.c_float)]


class GuessState(C.Structure):
    _fields_ = [("first_trans_available", C.c_int), ("last_imu_pre_trans_available", C.c_int), ("first", C.c_int), ("reserved", C.c_int),
                ("last_imu_transformation", C.c_float * 12), ("last_imu_pre_transformation", C.c_float * 12),
                ("last_transform_tobe_mapped", C.c_float * 6)]


class IcpItem(C.Structure):
    _fields_ = [("source", C.c_void_p), ("n", C.c_int), ("slot", C.c_int), ("guess", C.POINTER(C.c_float))]


LOOPDET_MAX_DB = 16
LOOPDET_NO_SHIFT = -2 ** 31


class LoopdetParams(C.Structure):
    _fields_ = [("skip_neighbour_distance", C.c_double), ("inflation_covariance", C.c_double), ("distance_threshold", C.c_double)]


class LoopdetFrame(C.Structure):
    _fields_ = [("corner", C.c_void_p), ("n_corner", C.c_int), ("surf", C.c_void_p), ("n_surf", C.c_int),
                ("semantic", C.c_void_p), ("n_semantic", C.c_int), ("odom", C.c_float * 12)]


class LoopdetResult(C.Structure):
    _fields_ = [("current_frame_id", C.c_int), ("n_candidates", C.c_int), ("matched_frame_id", C.c_int), ("reserved", C.c_int),
                ("matched_transform", C.c_float * 16), ("score", C.c_double)]

    def as_dict(self):
        return dict(current_frame_id=self.current_frame_id, n_candidates=self.n_candidates, matched_frame_id=self.matched_frame_id,
                    matched_transform=np.array(list(self.matched_transform), np.float32).reshape(4, 4), score=self.score)


class LoopdetCandidate(C.Structure):
    _fields_ = [("history_id", C.c_int), ("yaw_shift", C.c_int), ("yaw_angle", C.c_float), ("icp_state", C.c_int),
                ("icp_iters", C.c_int), ("icp_n_corr", C.c_int), ("transform", C.c_float * 16), ("score_shift", C.c_int),
                ("reserved", C.c_int), ("score", C.c_double)]

    def as_dict(self):
        return dict(history_id=self.history_id, yaw_shift=self.yaw_shift, yaw_angle=self.yaw_angle, icp_state=self.icp_state,
                    icp_iters=self.icp_iters, icp_n_corr=self.icp_n_corr,
                    transform=np.array(list(self.transform), np.float32).reshape(4, 4), score_shift=self.score_shift, score=self.score)


# the seven loopDetection selectors (lis_slam/Using{ISC,SC,EPSC,SEPSC,FEPSC,SSC,Pose}Flag), bit = kind index, in push order
LOOP_ISC, LOOP_SC, LOOP_EPSC, LOOP_SEPSC, LOOP_FEPSC, LOOP_SSC, LOOP_POSE = (1 << k for k in range(7))
LOOP_KIND_NAMES = ("isc", "sc", "epsc", "sepsc", "fepsc", "ssc", "pose")
LOOP_KINDS = {n: 1 << k for k, n in enumerate(LOOP_KIND_NAMES)}
LOOP_LABEL_THRESHOLD = 0.79


def loop_kinds(kinds) -> int:
    """a LISREG_LOOP_* mask from an int or an iterable of names ("isc", ..., "pose")."""
    if isinstance(kinds, (int, np.integer)):
        return int(kinds)
    return sum(LOOP_KINDS[k.lower()] for k in kinds)


class LoopdetMatch(C.Structure):
    _fields_ = [("kind", C.c_int), ("history_id", C.c_int), ("transform", C.c_float * 16), ("score", C.c_double)]

    def as_dict(self):
        return dict(kind=self.kind, kind_name=LOOP_KIND_NAMES[self.kind.bit_length() - 1], history_id=self.history_id,
                    transform=np.array(list(self.transform), np.float32).reshape(4, 4), score=self.score)


class LoopdetKindScores(C.Structure):
    _fields_ = [("history_id", C.c_int), ("shift", C.c_int * 7), ("score", C.c_double * 7)]

    def as_dict(self):
        return dict(history_id=self.history_id, shift=np.array(list(self.shift), np.int32), score=np.array(list(self.score), np.float64))


def loopdet_default_params() -> LoopdetParams:
    p = LoopdetParams()
    lib().lisreg_loopdet_default_params(C.byref(p))
    return p


class Deskew(C.Structure):
    _fields_ = [("enabled", C.c_int), ("imu_pointer_cur", C.c_int), ("imu_time", C.POINTER(C.c_double)),
                ("imu_rot_x", C.POINTER(C.c_double)), ("imu_rot_y", C.POINTER(C.c_double)), ("imu_rot_z", C.POINTER(C.c_double)),
                ("time_scan_cur", C.c_double), ("time_device", C.POINTER(C.c_float))]


def make_deskew(imu_time, rot_x, rot_y, rot_z, time_scan_cur, enabled=True, time_device_ptr=0):
    """lisreg_deskew from the integrated IMU tables (imuTime / imuRotX,Y,Z of imuDeskewInfo); keeps the arrays alive."""
    arrs = [np.ascontiguousarray(a, np.float64) for a in (imu_time, rot_x, rot_y, rot_z)]
    d = Deskew()
    d.enabled = 1 if enabled else 0
    d.imu_pointer_cur = len(arrs[0]) - 1
    d.imu_time, d.imu_rot_x, d.imu_rot_y, d.imu_rot_z = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs]
    d.time_scan_cur = float(time_scan_cur)
    d.time_device = C.cast(C.c_void_p(time_device_ptr), C.POINTER(C.c_float)) if time_device_ptr else None
    d._keep = arrs
    return d


class IcpGnResult(C.Structure):
    _fields_ = [("final_transform", C.c_float * 16), ("steps_applied", C.c_int), ("n_corr_last", C.c_int),
                ("fitness", C.c_float), ("reserved", C.c_int)]

    def as_dict(self):
        return dict(T=np.array(list(self.final_transform), np.float32).reshape(4, 4), steps_applied=self.steps_applied,
                    n_corr_last=self.n_corr_last, fitness=self.fitness)


class IcpGnItemC(C.Structure):
    _fields_ = [("source", C.c_int), ("slot", C.c_int), ("predict_pose", C.POINTER(C.c_float))]


class IcpGnBatchInfo(C.Structure):
    _fields_ = [("best", C.c_int), ("n_sources_staged", C.c_int), ("n_syncs", C.c_int), ("reserved", C.c_int)]


class IcpGnItem:
    """one candidate of icp_gn_match_batch: the index of its source, its map-index slot and its predict_pose (None: identity)"""

    def __init__(self, source: int, slot: int, predict_pose=None):
        self.source, self.slot, self.predict_pose = source, slot, predict_pose


class Params(C.Structure):
    _fields_ = [("max_iters", C.c_int), ("fixed_iters", C.c_int), ("knn_sq_thresh", C.c_float),
                ("conv_deg", C.c_float), ("conv_cm", C.c_float), ("min_corr", C.c_int),
                ("eig_thresh", C.c_float), ("edge_min", C.c_int), ("surf_min", C.c_int),
                ("line_ratio", C.c_float), ("plane_tol", C.c_float), ("accept_s", C.c_float),
                ("use_label_weight", C.c_int), ("label_score", C.c_float * 32),
                ("emulate_matp_shadow", C.c_int), ("skip_empty_target", C.c_int), ("use_imu_blend", C.c_int),
                ("imu_rpy_weight", C.c_float), ("rotation_tol", C.c_float), ("z_tol", C.c_float)]


class Imu(C.Structure):
    _fields_ = [("imu_available", C.c_int), ("imu_roll_init", C.c_float), ("imu_pitch_init", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("iters", C.c_int), ("deltaR", C.c_float), ("deltaT", C.c_float), ("degenerate", C.c_int),
                ("n_corr_last", C.c_int), ("status", C.c_int)]


class Item(C.Structure):
    _fields_ = [("src_corner", C.c_void_p), ("n_corner", C.c_int), ("src_surf", C.c_void_p), ("n_surf", C.c_int),
                ("stride_bytes", C.c_int), ("fmt", C.c_int), ("target", C.c_int), ("degenerate_in", C.c_int),
                ("imu", Imu)]


class LocalMapParams(C.Structure):
    _fields_ = [("max_num_pts", C.c_int), ("dynamic_removal_on", C.c_int), ("dynamic_removal_center_radius", C.c_float),
                ("dynamic_dist_thre_min", C.c_float), ("dynamic_dist_thre_max", C.c_float), ("near_dist_thre", C.c_float),
                ("leaf", C.c_float * 5), ("crop_box", C.c_float * 6), ("crop_pad", C.c_float)]


class KeyframesInfo(C.Structure):
    _fields_ = [("n_keyframes", C.c_int), ("n_target_corner", C.c_int), ("n_target_surf", C.c_int)]


class LocalMapInfo(C.Structure):
    _fields_ = [("n", C.c_int * 5), ("feature_point_num", C.c_int), ("bound", C.c_double * 6), ("crop", C.c_double * 6),
                ("n_target_corner", C.c_int), ("n_target_surf", C.c_int)]


class SubmapInfo(C.Structure):
    _fields_ = [("n", C.c_int * 5), ("feature_point_num", C.c_int), ("local_bound", C.c_double * 6), ("bound", C.c_double * 6)]


class SubmapExtractOut(C.Structure):
    _fields_ = [("isect", C.c_double * 6), ("isect_local", C.c_double * 6), ("n_target_corner", C.c_int), ("n_target_surf", C.c_int),
                ("src_corner", C.c_void_p), ("n_src_corner", C.c_int), ("src_surf", C.c_void_p), ("n_src_surf", C.c_int)]


LOCALMAP_CLASSES = ("dynamic", "pole", "ground", "building", "outlier")      # class order of localMap_t (subMap.h:742-753)
CLS_DYNAMIC, CLS_POLE, CLS_GROUND, CLS_BUILDING, CLS_OUTLIER, CLS_ALL = 1, 2, 4, 8, 16, 31      # bit k = class k (lisreg_submap_gather)


class GatherParams(C.Structure):
    _fields_ = [("class_mask", C.c_uint), ("out_fmt", C.c_int), ("chunk_points", C.c_int)]


class FeatureParams(C.Structure):
    _fields_ = [("n_scan", C.c_int), ("horizon_scan", C.c_int), ("downsample_rate", C.c_int), ("min_range", C.c_float),
                ("max_range", C.c_float), ("edge_threshold", C.c_float), ("surf_threshold", C.c_float)]


class FeatureOut(C.Structure):
    _fields_ = [(f, t) for name in ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")
                for f, t in ((name, C.c_void_p), ("cap_" + name, C.c_int), ("n_" + name, C.c_int))]


VOXEL_BATCH_MAX = 1024


class VoxelJob(C.Structure):
    """lisreg_voxel_job: one cloud of lisreg_voxel_downsample_batch (n_out and status are written back)."""
    _fields_ = [("in_", C.c_void_p), ("n", C.c_int), ("leaf", C.c_float), ("out", C.c_void_p), ("out_capacity", C.c_int),
                ("n_out", C.c_int), ("status", C.c_int)]


class PretreatParams(C.Structure):
    _fields_ = [("n_scan", C.c_int), ("min_range", C.c_float), ("max_range", C.c_float), ("scan_period", C.c_double)]


class PretreatOut(C.Structure):
    _fields_ = [("cloud", C.c_void_p), ("capacity", C.c_int), ("n", C.c_int), ("time_device", C.c_void_p),
                ("intensity_device", C.c_void_p), ("start_ori", C.c_float), ("end_ori", C.c_float), ("half_index", C.c_int)]

    def as_dict(self):
        return dict(n=self.n, start_ori=np.float32(self.start_ori), end_ori=np.float32(self.end_ori), half_index=self.half_index)


class Motion(C.Structure):
    """lisreg_motion: DistortionAdjust::SetMotionInfo's arguments"""
    _fields_ = [("scan_period", C.c_float), ("linear_velocity", C.c_double * 3), ("angular_velocity", C.c_double * 3)]


class AdjustOut(C.Structure):
    _fields_ = [("cloud", C.c_void_p), ("capacity", C.c_int), ("n", C.c_int), ("time_device", C.c_void_p)]


def make_motion(linear_velocity=(0.0, 0.0, 0.0), angular_velocity=(0.0, 0.0, 0.0), scan_period: float | None = None) -> Motion:
    """lisreg_default_motion (scan period 0.1f, zero rates) with the given velocities"""
    m = Motion()
    rc = lib().lisreg_default_motion(C.byref(m))
    if rc:
        raise LisregError(rc, "lisreg_default_motion")
    if scan_period is not None:
        m.scan_period = scan_period
    m.linear_velocity[:] = [float(v) for v in linear_velocity]
    m.angular_velocity[:] = [float(v) for v in angular_velocity]
    return m


class RangenetParams(C.Structure):
    _fields_ = [("img_h", C.c_int), ("img_w", C.c_int), ("fov_up", C.c_double), ("fov_down", C.c_double), ("means", C.c_float * 5),
                ("stds", C.c_float * 5), ("n_classes", C.c_int)]


class RangenetOut(C.Structure):
    _fields_ = [("tensor", C.c_void_p), ("invalid_mask", C.c_void_p), ("pixel_index", C.c_void_p), ("n_valid", C.c_int)]


class RangenetKnnParams(C.Structure):
    _fields_ = [("knn", C.c_int), ("search", C.c_int), ("sigma", C.c_float), ("cutoff", C.c_float), ("no_vote_label", C.c_int)]


class SemanticOut(C.Structure):
    _fields_ = [("cloud", C.c_void_p * 5), ("cap", C.c_int * 5), ("n", C.c_int * 5)]


SEMANTIC_BATCH_MAX = 256
CONCAT_BATCH_MAX = 1024
SEMANTIC_BATCH_TILE = 1024         # kSbTile (csrc/lisreg_semantic_batch_plan.hpp): points of one tile of lisreg_semantic_split_batch


class SemanticJob(C.Structure):
    """lisreg_semantic_job: one frame of lisreg_semantic_split_batch (out.n and status are written back)."""
    _fields_ = [("in_", C.c_void_p), ("n", C.c_int), ("out", SemanticOut), ("status", C.c_int)]


class ConcatJob(C.Structure):
    """lisreg_concat_job: one job of lisreg_concat_device_batch (n_out is written back)."""
    _fields_ = [("in_", C.c_void_p * 8), ("n", C.c_int * 8), ("k", C.c_int), ("out", C.c_void_p), ("out_capacity", C.c_int), ("n_out", C.c_int)]


class LisregError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"lisreg error {code}: {msg}")
        self.code = code


def build(verbose: bool = False) -> str:
    """Compile liblisreg.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", CSRC] + ([] if verbose else ["-s"]))
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built — run `make -C {CSRC}` (there is no fallback path)")
        L = C.CDLL(LIB_PATH)
        vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)
        L.lisreg_device_count.restype = C.c_int
        L.lisreg_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.lisreg_destroy.argtypes = [vp]
        L.lisreg_destroy.restype = None
        L.lisreg_last_error.argtypes = [vp]
        L.lisreg_last_error.restype = C.c_char_p
        L.lisreg_set_stream.argtypes = [vp, vp]
        L.lisreg_get_stream.argtypes = [vp]
        L.lisreg_get_stream.restype = vp
        L.lisreg_default_params.argtypes = [C.c_int, C.POINTER(Params)]
        L.lisreg_set_target.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int]
        L.lisreg_set_target_slot.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int]
        L.lisreg_target_from_classes.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int,
                                                 C.c_int, C.c_int]
        L.lisreg_align.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(Params),
                                   C.POINTER(Imu), fp, C.POINTER(Stats)]
        L.lisreg_align_batch.argtypes = [vp, C.c_int, C.POINTER(Item), C.POINTER(Params), fp, C.POINTER(Stats)]
        L.lisreg_batch_prepare.argtypes = [vp, C.c_int, C.POINTER(Item), C.POINTER(Params), fp]
        L.lisreg_stage_host_items.argtypes = [vp, C.c_int, C.POINTER(Item), C.POINTER(Item)]
        L.lisreg_batch_run.argtypes = [vp]
        L.lisreg_batch_fetch.argtypes = [vp, fp, C.POINTER(Stats)]
        L.lisreg_batch_result_device.argtypes = [vp]
        L.lisreg_batch_result_device.restype = vp
        L.lisreg_set_option.argtypes = [vp, C.c_char_p, C.c_int]
        L.lisreg_upload_cloud.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
        L.lisreg_concat_device.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), vp, C.POINTER(C.c_int)]
        L.lisreg_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
        L.lisreg_get_neighbors.argtypes = [vp, C.POINTER(C.c_int), C.c_int]
        L.lisreg_get_partial_rows.argtypes = [vp, ip, ip, C.POINTER(C.c_double), C.c_int, fp, ip, C.c_int]
        if hasattr(L, "lisreg_test_fit_models"): L.lisreg_test_fit_models.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(Params), C.c_int, C.POINTER(C.c_float)]
        if hasattr(L, "lisreg_test_solve_steps"): L.lisreg_test_solve_steps.argtypes = [vp, C.c_int, C.c_int, ip, C.POINTER(C.c_double), fp, ip, ip, ip, C.POINTER(Imu), C.POINTER(Params), fp, fp, fp]
        L.lisreg_get_target_index.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.lisreg_get_target_graph.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]
        L.lisreg_get_target_cell_rows.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]
        L.lisreg_get_counters.argtypes = [vp, C.POINTER(C.c_ulonglong), C.c_int]
        L.lisreg_get_trace.argtypes = [vp, fp, C.c_int]
        L.lisreg_set_profiling.argtypes = [vp, C.c_int]
        L.lisreg_get_timing.argtypes = [vp, C.POINTER(C.c_double)]
        L.lisreg_pose_to_matrix.argtypes = [fp, fp]
        L.lisreg_pose_to_matrix.restype = None
        L.lisreg_transform_update.argtypes = [C.POINTER(Params), C.POINTER(Imu), fp]
        L.lisreg_transform_update.restype = None
        L.lisreg_comm_unique_id.argtypes = [C.POINTER(C.c_ubyte)]
        L.lisreg_comm_init.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_ubyte)]
        L.lisreg_gather_results.argtypes = [vp, vp, C.c_int, vp]
        L.lisreg_comm_destroy.argtypes = [vp]
        L.lisreg_comm_destroy.restype = None
        L.lisreg_voxel_downsample_multi.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int,
                                                    C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.lisreg_voxel_downsample.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp, C.c_int, ip]
        L.lisreg_voxel_downsample_batch.argtypes = [vp, C.c_int, C.POINTER(VoxelJob), C.c_int]
        L.lisreg_transform_cloud.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, fp, vp]
        L.lisreg_extract_features.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(FeatureParams), C.POINTER(FeatureOut)]
        L.lisreg_default_feature_params.argtypes = [C.POINTER(FeatureParams)]
        L.lisreg_extract_features_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(FeatureParams),
                                                    C.POINTER(FeatureOut)]
        L.lisreg_extract_features_deskew.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(FeatureParams), C.POINTER(Deskew),
                                                     C.POINTER(FeatureOut)]
        L.lisreg_default_pretreat_params.argtypes = [C.POINTER(PretreatParams)]
        L.lisreg_pretreat.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PretreatParams), C.POINTER(PretreatOut)]
        L.lisreg_pretreat_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(PretreatParams),
                                            C.POINTER(PretreatOut)]
        L.lisreg_extract_features_deskew_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(FeatureParams),
                                                           C.POINTER(Deskew), C.POINTER(FeatureOut)]
        L.lisreg_default_motion.argtypes = [C.POINTER(Motion)]
        L.lisreg_adjust_cloud.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(Motion), C.POINTER(AdjustOut)]
        L.lisreg_adjust_cloud_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(Motion),
                                                C.POINTER(AdjustOut)]
        L.lisreg_default_rangenet_params.argtypes = [C.POINTER(RangenetParams)]
        L.lisreg_rangenet_project.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(RangenetParams), C.POINTER(RangenetOut)]
        L.lisreg_rangenet_project_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(RangenetParams),
                                                    C.POINTER(RangenetOut)]
        L.lisreg_rangenet_label.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(RangenetParams), vp, vp]
        L.lisreg_rangenet_label_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(RangenetParams),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.lisreg_default_rangenet_knn_params.argtypes = [C.POINTER(RangenetKnnParams)]
        L.lisreg_rangenet_knn_weights.argtypes = [C.POINTER(RangenetKnnParams), fp]
        L.lisreg_rangenet_knn_weights.restype = None
        L.lisreg_rangenet_label_knn.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(RangenetParams), C.POINTER(RangenetKnnParams), vp, vp]
        L.lisreg_rangenet_label_knn_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(RangenetParams),
                                                      C.POINTER(RangenetKnnParams), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.lisreg_semantic_split.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(SemanticOut)]
        L.lisreg_semantic_split_batch.argtypes = [vp, C.c_int, C.POINTER(SemanticJob), C.POINTER(C.c_uint32)]
        L.lisreg_concat_device_batch.argtypes = [vp, C.c_int, C.POINTER(ConcatJob)]
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        L.lisreg_map_index_set.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int]
        L.lisreg_map_index_set_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int]
        L.lisreg_nearest.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]
        L.lisreg_get_map_grid.argtypes = [vp, C.c_int, ip, C.POINTER(C.c_float)]
        L.lisreg_test_nn1.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_float, C.c_int, ip, ip, C.POINTER(C.c_float)]
        L.lisreg_test_scan.argtypes = [vp, ip, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]
        L.lisreg_dynamic_filter.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                            C.c_float, vp, ip]
        L.lisreg_bbx_filter.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, dp, C.c_int, vp, ip]
        L.lisreg_cloud_bounds.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, dp]
        L.lisreg_localmap_default_params.argtypes = [C.POINTER(LocalMapParams)]
        L.lisreg_localmap_reset.argtypes = [vp, C.c_int]
        L.lisreg_keyframes_reset.argtypes = [vp, C.c_int]
        L.lisreg_keyframes_push.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(KeyframesInfo)]
        L.lisreg_keyframes_target.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(KeyframesInfo)]
        L.lisreg_localmap_insert.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, fp,
                                             C.POINTER(LocalMapParams), C.POINTER(LocalMapInfo)]
        L.lisreg_localmap_extract.argtypes = [vp, C.c_int, fp, C.POINTER(LocalMapParams), C.c_int, C.POINTER(LocalMapInfo)]
        L.lisreg_localmap_get.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, ip]
        L.lisreg_submap_insert.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, fp, fp,
                                           C.POINTER(LocalMapParams), C.POINTER(SubmapInfo)]
        L.lisreg_submap_extract.argtypes = [vp, C.c_int, C.c_int, fp, fp, C.c_float, C.c_float, C.c_float, C.c_int, C.POINTER(SubmapExtractOut)]
        L.lisreg_submap_crop_boxes.argtypes = [C.POINTER(C.c_double), fp, C.POINTER(C.c_double), fp, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.lisreg_submap_crop_boxes.restype = None
        llp = C.POINTER(C.c_longlong)
        L.lisreg_default_gather_params.argtypes = [C.POINTER(GatherParams)]
        L.lisreg_submap_gather_count.argtypes = [vp, C.c_int, ip, C.c_uint, llp, llp]
        L.lisreg_submap_gather.argtypes = [vp, C.c_int, ip, fp, C.POINTER(GatherParams), vp, C.c_longlong, llp, llp]
        L.lisreg_predict_pose.argtypes = [fp, fp, fp]
        L.lisreg_predict_pose.restype = None
        L.lisreg_guess_state_init.argtypes = [C.POINTER(GuessState)]
        L.lisreg_guess_state_init.restype = None
        L.lisreg_update_initial_guess.argtypes = [C.c_int, C.c_int, C.POINTER(GuessInput), C.POINTER(GuessState), fp, fp]
        L.lisreg_update_initial_guess.restype = None
        L.lisreg_icp_default_params.argtypes = [C.c_int, C.POINTER(IcpParams)]
        L.lisreg_icp_gn_match.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_float, fp, C.POINTER(IcpGnResult), vp]
        L.lisreg_icp_gn_match_batch.argtypes = [vp, C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int, C.POINTER(IcpGnItemC), C.c_int, C.c_uint, C.c_float,
                                                C.POINTER(IcpGnResult), C.POINTER(IcpGnBatchInfo)]
        L.lisreg_icp_align.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(IcpParams), fp, C.POINTER(IcpResult), vp]
        L.lisreg_icp_align_batch.argtypes = [vp, C.POINTER(IcpItem), C.c_int, C.c_int, C.c_int, C.POINTER(IcpParams), C.c_int, C.POINTER(IcpResult)]
        u8p = C.POINTER(C.c_uint8)
        L.lisreg_loopdet_default_params.argtypes = [C.POINTER(LoopdetParams)]
        L.lisreg_loopdet_reset.argtypes = [vp, C.c_int]
        L.lisreg_loopdet_detect.argtypes = [vp, C.c_int, C.POINTER(LoopdetFrame), C.c_int, C.c_int, C.c_int, C.POINTER(LoopdetParams),
                                            C.POINTER(LoopdetResult)]
        L.lisreg_loopdet_candidates.argtypes = [vp, C.c_int, C.c_int, C.POINTER(LoopdetCandidate), C.c_int, ip]
        L.lisreg_loopdet_get.argtypes = [vp, C.c_int, C.c_int, u8p, fp]
        L.lisreg_loop_descriptor.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, fp, u8p, u8p, u8p, fp]
        L.lisreg_loopdet_configure.argtypes = [vp, C.c_int, C.c_uint, C.c_double]
        L.lisreg_loopdet_matches.argtypes = [vp, C.c_int, C.c_int, C.POINTER(LoopdetMatch), C.c_int, ip]
        L.lisreg_loopdet_candidate_scores.argtypes = [vp, C.c_int, C.c_int, C.POINTER(LoopdetKindScores), C.c_int, ip]
        L.lisreg_loopdet_get_descriptor.argtypes = [vp, C.c_int, C.c_int, C.c_uint, u8p]
        L.lisreg_loop_descriptor_kind.argtypes = [vp, C.c_uint, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, fp, u8p]
        dbl = C.POINTER(C.c_double)
        L.lisreg_ndt_default_params.argtypes = [C.c_int, C.POINTER(NdtParams)]
        L.lisreg_ndt_set_target.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(NdtParams), C.POINTER(NdtInfo)]
        L.lisreg_ndt_align.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(NdtParams), fp, C.POINTER(NdtResult), vp]
        L.lisreg_ndt_get_voxels.argtypes = [vp, C.c_int, ip, ip, dbl, dbl, C.c_int, ip]
        L.lisreg_ndt_derivatives.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(NdtParams), dbl, C.c_int, dbl,
                                             C.POINTER(C.c_longlong)]
        L.lisreg_ndt_align_batch.argtypes = [vp, C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int, C.POINTER(NdtItemC), C.c_int,
                                             C.POINTER(NdtParams), C.POINTER(NdtResult), dbl, C.POINTER(NdtBatchInfo)]
        L.lisreg_vgicp_default_params.argtypes = [C.c_int, C.POINTER(VgicpParams)]
        L.lisreg_vgicp_set_target.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(VgicpParams), C.POINTER(VgicpInfo)]
        L.lisreg_vgicp_align.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(VgicpParams), fp, C.POINTER(VgicpResult), vp]
        L.lisreg_vgicp_covariances.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, dbl, ip, C.c_float]
        L.lisreg_vgicp_get_voxels.argtypes = [vp, C.c_int, ip, ip, dbl, dbl, C.c_int, ip]
        L.lisreg_vgicp_linearize.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(VgicpParams), dbl, C.c_int, dbl,
                                             C.POINTER(C.c_longlong)]
        L.lisreg_vgicp_align_batch.argtypes = [vp, C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int, C.POINTER(VgicpItemC), C.c_int,
                                               C.POINTER(VgicpParams), C.POINTER(VgicpResult), dbl, C.POINTER(VgicpBatchInfo)]
        L.lisreg_ndt_set_target_batch.argtypes = [vp, C.c_int, C.POINTER(NdtTargetJob), C.POINTER(NdtParams)]
        L.lisreg_ndt_get_target.argtypes = [vp, C.c_int, C.POINTER(NdtInfo), ip, ip, dbl, fp, ip, ip, ip, fp, ip, ip, ip, ip, dbl,
                                            C.c_int, C.c_int, C.c_int, C.c_int]
        L.lisreg_ndt_target_batch_counts.argtypes = [vp, ip, ip]
        L.lisreg_vgicp_set_target_batch.argtypes = [vp, C.c_int, C.POINTER(VgicpTargetJob), C.POINTER(VgicpParams)]
        L.lisreg_vgicp_get_target.argtypes = [vp, C.c_int, C.POINTER(VgicpInfo), ip, ip, dbl, fp, ip, fp, ip, ip, C.c_int, C.c_int, C.c_int]
        L.lisreg_vgicp_target_batch_counts.argtypes = [vp, ip, ip]
        L.lisreg_fgicp_default_params.argtypes = [C.c_int, C.POINTER(FgicpParams)]
        L.lisreg_fgicp_set_target.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(FgicpParams), C.POINTER(FgicpInfo), C.c_float]
        L.lisreg_fgicp_set_target_batch.argtypes = [vp, C.c_int, C.POINTER(FgicpTargetJob), C.POINTER(FgicpParams)]
        L.lisreg_fgicp_get_target.argtypes = [vp, C.c_int, C.POINTER(FgicpInfo), fp, fp, ip, ip, dbl, C.c_int, C.c_int]
        L.lisreg_fgicp_grid_geometry.argtypes = [fp, C.c_int, C.c_float, ip, fp]
        L.lisreg_fgicp_target_batch_counts.argtypes = [vp, ip, ip]
        L.lisreg_fgicp_align.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(FgicpParams), fp, C.POINTER(FgicpResult), vp]
        L.lisreg_fgicp_correspondences.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(FgicpParams), dbl, ip, dbl]
        L.lisreg_fgicp_align_batch.argtypes = [vp, C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int, C.POINTER(FgicpItemC), C.c_int,
                                               C.POINTER(FgicpParams), C.POINTER(FgicpResult), dbl, C.POINTER(FgicpBatchInfo)]
        L.lisreg_fgicp_linearize.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(FgicpParams), dbl, dbl, C.c_int, dbl,
                                             C.POINTER(C.c_longlong)]
        L.lisreg_gicp_default_params.argtypes = [C.c_int, C.POINTER(GicpParams)]
        L.lisreg_gicp_align.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(GicpParams), fp, C.POINTER(GicpResult), vp]
        L.lisreg_gicp_moments.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(GicpParams), dbl, dbl]
        L.lisreg_gicp_inner.argtypes = [dbl, dbl, dbl, C.POINTER(GicpParams), dbl, ip, dbl]
        L.lisreg_gicp_align_batch.argtypes = [vp, C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int, C.POINTER(GicpItemC), C.c_int,
                                              C.POINTER(GicpParams), C.POINTER(GicpResult), dbl, C.POINTER(GicpBatchInfo)]
        _lib = L
    return _lib


def _default_params(struct, fn_name: str, kind: int, overrides: dict):
    """the library's defaults of one verifier's parameter struct, then the caller's overrides (an unknown name raises AttributeError)"""
    p = struct()
    if getattr(lib(), fn_name)(kind, C.byref(p)):
        raise LisregError(ERR_ARG, fn_name)
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def fgicp_grid_geometry(bb, n_points: int, cell_edge: float = 0.0):
    """lisreg_fgicp_grid_geometry: (dims [3], cell, inv_cell) of the search grid over the finite box bb [6]; needs no device"""
    bb = np.ascontiguousarray(bb, np.float32).reshape(6)
    dims = (C.c_int * 3)()
    cell = (C.c_float * 2)()
    rc = lib().lisreg_fgicp_grid_geometry(bb.ctypes.data_as(C.POINTER(C.c_float)), int(n_points), float(cell_edge), dims, cell)
    if rc != OK:
        raise LisregError(rc, "lisreg_fgicp_grid_geometry: bad arguments")
    return list(dims), np.float32(cell[0]), np.float32(cell[1])


def fgicp_default_params(kind: int = 0, **overrides) -> FgicpParams:
    return _default_params(FgicpParams, "lisreg_fgicp_default_params", kind, overrides)


def gicp_default_params(kind: int = 0, **overrides) -> GicpParams:
    return _default_params(GicpParams, "lisreg_gicp_default_params", kind, overrides)


def gicp_inner(moments, centre, x0, params: GicpParams) -> dict:
    """lisreg_gicp_inner: the inner BFGS of one outer iteration of PCL's GICP from its 74 moments, the centre they are taken about and
    the outer iterate x0 = (tx, ty, tz, roll, pitch, yaw).  Needs no GPU.  Returns dict(x [6], f, iters, n_f, n_df, exit)."""
    dp = C.POINTER(C.c_double)
    m, c, x0 = (np.ascontiguousarray(a, np.float64).ravel() for a in (moments, centre, x0))
    if m.size != 74 or c.size != 3 or x0.size != 6:
        raise ValueError("gicp_inner: moments [74], centre [3], x0 [6]")
    x, cnt, f = np.zeros(6), np.zeros(4, np.int32), C.c_double(0.0)
    rc = lib().lisreg_gicp_inner(m.ctypes.data_as(dp), c.ctypes.data_as(dp), x0.ctypes.data_as(dp), C.byref(params), x.ctypes.data_as(dp),
                                 cnt.ctypes.data_as(C.POINTER(C.c_int)), C.byref(f))
    if rc:
        raise LisregError(rc, "lisreg_gicp_inner")
    return dict(x=x, f=f.value, iters=int(cnt[0]), n_f=int(cnt[1]), n_df=int(cnt[2]), exit=int(cnt[3]))


def vgicp_default_params(kind: int = 0, **overrides) -> VgicpParams:
    return _default_params(VgicpParams, "lisreg_vgicp_default_params", kind, overrides)


def ndt_default_params(kind: int = 0, **overrides) -> NdtParams:
    return _default_params(NdtParams, "lisreg_ndt_default_params", kind, overrides)


def localmap_default_params() -> LocalMapParams:
    p = LocalMapParams()
    if lib().lisreg_localmap_default_params(C.byref(p)):
        raise LisregError(ERR_ARG, "lisreg_localmap_default_params")
    return p


def predict_pose(T_last, T_cur) -> np.ndarray:
    a = np.ascontiguousarray(T_last, np.float32); b = np.ascontiguousarray(T_cur, np.float32)
    out = np.zeros(6, np.float32)
    f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    lib().lisreg_predict_pose(f(a), f(b), f(out))
    return out


class InitialGuess:
    """updateInitialGuess with its function-local statics (lisreg_update_initial_guess): variant 0 = odomEstimationNode.cpp:297-419,
    1 = subMapOptmizationNode.cpp:896-1032.  update(T, ...) returns (T_new, transPredictionMapped or None)."""

    def __init__(self, variant: int = 0, use_imu_heading_initialization: bool = False):
        self.variant, self.heading = variant, use_imu_heading_initialization
        self.state = GuessState()
        lib().lisreg_guess_state_init(C.byref(self.state))

    def update(self, T, odom_available=False, imu_available=False, imu_rpy=(0.0, 0.0, 0.0), initial_guess=(0.0,) * 6):
        """initial_guess = (x, y, z, roll, pitch, yaw) of cloudInfo.initialGuess*"""
        inp = GuessInput(1 if odom_available else 0, 1 if imu_available else 0, *[float(v) for v in imu_rpy], *[float(v) for v in initial_guess])
        T = np.array(T, np.float32)
        # "not assigned" is told by a bit pattern the library cannot produce (a NaN with a payload of its own), not by NaN-ness: a prediction
        # that really IS NaN (a NaN pose propagated through the increment) comes back as what it is
        sentinel = np.uint32(0x7FC0DEAD)
        pred = np.full(6, sentinel, np.uint32).view(np.float32)
        f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        lib().lisreg_update_initial_guess(self.variant, 1 if self.heading else 0, C.byref(inp), C.byref(self.state), f(T), f(pred))
        return T, (None if (pred.view(np.uint32) == sentinel).all() else pred)


def _info_dict(info: LocalMapInfo) -> dict:
    return dict(n=list(info.n), feature_point_num=info.feature_point_num, bound=np.array(list(info.bound)),
                crop=np.array(list(info.crop)), n_target_corner=info.n_target_corner, n_target_surf=info.n_target_surf)


def icp_default_params(kind: int = 0) -> IcpParams:
    p = IcpParams()
    if lib().lisreg_icp_default_params(kind, C.byref(p)):
        raise LisregError(ERR_ARG, "lisreg_icp_default_params")
    return p


def default_params(variant: int = VARIANT_ODOM) -> Params:
    p = Params()
    rc = lib().lisreg_default_params(variant, C.byref(p))
    if rc:
        raise LisregError(rc, "lisreg_default_params")
    return p


def pose_to_matrix(T) -> np.ndarray:
    T = np.ascontiguousarray(T, np.float32)
    M = np.zeros(12, np.float32)
    lib().lisreg_pose_to_matrix(T.ctypes.data_as(C.POINTER(C.c_float)), M.ctypes.data_as(C.POINTER(C.c_float)))
    return M.reshape(3, 4)


def transform_update(params: Params, imu: Imu | None, T) -> np.ndarray:
    T = np.array(T, np.float32)
    lib().lisreg_transform_update(C.byref(params), C.byref(imu) if imu is not None else None,
                                  T.ctypes.data_as(C.POINTER(C.c_float)))
    return T


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and len(a) else None


def _fmt_of(cloud) -> int:
    return FMT_XYZIL if (cloud.dtype.names and "label" in cloud.dtype.names) else FMT_XYZI


def stats_dict(s: Stats) -> dict:
    return dict(iters=s.iters, deltaR=s.deltaR, deltaT=s.deltaT, degenerate=s.degenerate,
                n_corr_last=s.n_corr_last, status=s.status)


class Context:
    """One lisreg_ctx (single-threaded; one per caller, like the three reference node classes)."""

    def __init__(self, device: int = 0):
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.lisreg_create(device, C.byref(h))
        if rc:
            raise LisregError(rc, self._L.lisreg_last_error(None).decode())
        self._h = h
        self._keep = []

    def close(self):
        if self._h:
            self._L.lisreg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, allow=(OK,)):
        if rc not in allow:
            raise LisregError(rc, self._L.lisreg_last_error(self._h).decode())
        return rc

    def last_error(self) -> str:
        """lisreg_last_error: the text of the context's last failure (a call that returns OK may leave one: a failed job of a batch)"""
        return self._L.lisreg_last_error(self._h).decode()

    @property
    def stream(self) -> int:
        return self._L.lisreg_get_stream(self._h) or 0

    def set_stream(self, hip_stream: int | None):
        self._chk(self._L.lisreg_set_stream(self._h, C.c_void_p(hip_stream) if hip_stream else None))

    def set_option(self, name: str, value: int):
        self._chk(self._L.lisreg_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int(0)
        self._chk(self._L.lisreg_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def neighbors(self, n_elems: int) -> np.ndarray:
        """[6, n_elems]: rows 0-4 original target indices of every source point's neighbours in the last GN iteration run
        (-1: none), row 5 = 1 where the point contributed a correspondence."""
        out = np.full((6, n_elems), -1, np.int32)
        self._chk(self._L.lisreg_get_neighbors(self._h, out.ctypes.data_as(C.POINTER(C.c_int)), n_elems))
        return out

    def partial_rows(self, n_elems: int | None = None) -> dict:
        """Test hook (lisreg_get_partial_rows): blocks[n_blocks, 4] (item, kind, first batch position, count) and rows[n_blocks, 28]
        (float64) as the last executed GN iteration left them; with n_elems (the batch's source point count; eight lanes per query
        only) also coef[n_elems, 4] and coef_ok[n_elems]."""
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        nb = C.c_int(-1)
        self._chk(self._L.lisreg_get_partial_rows(self._h, C.byref(nb), None, None, 0, None, None, 0))
        n = nb.value
        out = dict(blocks=np.full((n, 4), -1, np.int32), rows=np.full((n, 28), np.nan, np.float64))
        coef = coef_ok = None
        if n_elems is not None:
            out["coef"] = coef = np.full((n_elems, 4), np.nan, np.float32)
            out["coef_ok"] = coef_ok = np.full(n_elems, -1, np.int32)
        self._chk(self._L.lisreg_get_partial_rows(self._h, C.byref(nb), out["blocks"].ctypes.data_as(ip),
                                                  out["rows"].ctypes.data_as(C.POINTER(C.c_double)), n,
                                                  coef.ctypes.data_as(fp) if coef is not None else None,
                                                  coef_ok.ctypes.data_as(ip) if coef_ok is not None else None,
                                                  n_elems if n_elems is not None else 0))
        assert nb.value == n
        return out

    def test_fit_models(self, kind: int, neighbours: np.ndarray, queries: np.ndarray, params, exact: bool = False) -> np.ndarray:
        """Test hook: the device functions of the residual models (kind 1 = surfOptimization's body, 0 = cornerOptimization's, 2 = its eigen-solver alone) on
        neighbours[n, 5, 3] / queries[n, 3]; returns float32[n, 10] as include/lisreg.h describes."""
        nb = np.ascontiguousarray(neighbours, np.float32).reshape(-1, 15)
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
        assert nb.shape[0] == q.shape[0]
        out = np.zeros((nb.shape[0], 10), np.float32)
        fp = C.POINTER(C.c_float)
        self._chk(self._L.lisreg_test_fit_models(self._h, int(kind), nb.shape[0], nb.ctypes.data_as(fp), q.ctypes.data_as(fp), C.byref(params),
                                                 1 if exact else 0, out.ctypes.data_as(fp)))
        return out

    def test_solve_steps(self, n_rows, rows, T_init, params, degenerate_in=None, n_sc=None, n_ss=None, imu=None) -> dict:
        """Test hook (lisreg_test_solve_steps): the production solve / finalize kernels on caller-given normal equations.  n_rows[n]:
        partial rows per item (back to back); rows[n_steps, sum(n_rows), 28] float64; T_init[n, 6]; imu: a list of Imu (or None per
        item).  Returns dict(trace[n, n_steps, 56], state[n, n_steps, 56], results[n, 12]) as include/lisreg.h describes."""
        n_rows = np.ascontiguousarray(n_rows, np.int32).ravel()
        n = len(n_rows); total = int(n_rows.sum())
        rows = np.ascontiguousarray(rows, np.float64)
        assert rows.ndim == 3 and rows.shape[1:] == (total, 28), rows.shape
        n_steps = rows.shape[0]
        T0 = np.ascontiguousarray(T_init, np.float32).reshape(n, 6)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        opt = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).reshape(n)
        deg, sc, ss = opt(degenerate_in), opt(n_sc), opt(n_ss)
        iptr = lambda a: None if a is None else a.ctypes.data_as(ip)
        imu_arr = None
        if imu is not None:
            imu_arr = (Imu * max(n, 1))()
            for i, m in enumerate(imu):
                if m is not None:
                    imu_arr[i] = m
        trace = np.zeros((n, n_steps, TRACE_STRIDE), np.float32)
        state = np.zeros((n, n_steps, SOLVE_STATE_STRIDE), np.float32)
        results = np.zeros((n, RESULT_SIZE), np.float32)
        self._chk(self._L.lisreg_test_solve_steps(self._h, n, n_steps, n_rows.ctypes.data_as(ip), rows.ctypes.data_as(C.POINTER(C.c_double)),
                                                  T0.ctypes.data_as(fp), iptr(deg), iptr(sc), iptr(ss), imu_arr, C.byref(params),
                                                  trace.ctypes.data_as(fp), state.ctypes.data_as(fp), results.ctypes.data_as(fp)))
        return dict(trace=trace, state=state, results=results)

    def front_end(self) -> int:
        """search front-end of the prepared batch (1 cell walk, 3 k-NN graph scan, ...)."""
        return self.get_option("front_end")

    def set_profiling_paused(self, paused: bool):
        """stop (or resume) recording HIP events without discarding the ones already recorded; batch_fetch collects them."""
        self._chk(self._L.lisreg_set_profiling(self._h, 0 if paused else 1))

    # -- target ------------------------------------------------------------------------------------------
    def set_target(self, corner: np.ndarray, surf: np.ndarray, slot: int = 0):
        """corner/surf: numpy arrays of PCL point structs (itemsize = stride)."""
        corner = np.ascontiguousarray(corner); surf = np.ascontiguousarray(surf)
        self._chk(self._L.lisreg_set_target_slot(self._h, slot, _vp(corner), len(corner), _vp(surf), len(surf),
                                                 corner.dtype.itemsize, _fmt_of(corner)))

    def set_target_device(self, corner_ptr: int, n_corner: int, surf_ptr: int, n_surf: int, slot: int = 0):
        self._chk(self._L.lisreg_set_target_slot(self._h, slot, C.c_void_p(corner_ptr), n_corner,
                                                 C.c_void_p(surf_ptr), n_surf, 16, FMT_DEVICE))

    def target_from_classes(self, pole, ground, building, dynamic, slot: int = 0):
        arrs = [np.ascontiguousarray(a) for a in (pole, ground, building, dynamic)]
        self._chk(self._L.lisreg_target_from_classes(self._h, slot, _vp(arrs[0]), len(arrs[0]), _vp(arrs[1]),
                                                     len(arrs[1]), _vp(arrs[2]), len(arrs[2]), _vp(arrs[3]),
                                                     len(arrs[3]), arrs[0].dtype.itemsize, _fmt_of(arrs[0])))

    # -- single registration ---------------------------------------------------------------------------------
    def align(self, src_corner: np.ndarray, src_surf: np.ndarray, T_init, params: Params, imu: Imu | None = None):
        """lisreg_align.  Returns (T, stats dict, trace[n,56])."""
        sc = np.ascontiguousarray(src_corner); ss = np.ascontiguousarray(src_surf)
        T = np.array(T_init, np.float32).copy()
        st = Stats()
        rc = self._L.lisreg_align(self._h, _vp(sc), len(sc), _vp(ss), len(ss), sc.dtype.itemsize, _fmt_of(sc),
                                  C.byref(params), C.byref(imu) if imu is not None else None,
                                  T.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
        self._chk(rc, allow=(OK, NOT_ENOUGH_FEATURES, TOO_FEW_CORRESPONDENCES))
        bound = params.fixed_iters if params.fixed_iters > 0 else params.max_iters
        buf = np.zeros((max(bound, 1), TRACE_STRIDE), np.float32)
        n = self._L.lisreg_get_trace(self._h, buf.ctypes.data_as(C.POINTER(C.c_float)), max(bound, 1))
        d = stats_dict(st)
        if rc == NOT_ENOUGH_FEATURES:
            d["status"] = NOT_ENOUGH_FEATURES
        return T, d, buf[:n]

    # -- batches ---------------------------------------------------------------------------------------------
    def align_batch(self, items: list[dict], T_init: np.ndarray, params: Params):
        """items: dicts with src_corner, src_surf (PCL struct arrays), optional target, degenerate_in, imu."""
        n = len(items)
        arr = (Item * max(n, 1))()
        keep = []
        for i, it in enumerate(items):
            sc = np.ascontiguousarray(it["src_corner"]); ss = np.ascontiguousarray(it["src_surf"])
            keep += [sc, ss]
            arr[i].src_corner = _vp(sc); arr[i].n_corner = len(sc)
            arr[i].src_surf = _vp(ss); arr[i].n_surf = len(ss)
            arr[i].stride_bytes = sc.dtype.itemsize; arr[i].fmt = _fmt_of(sc)
            arr[i].target = it.get("target", 0); arr[i].degenerate_in = it.get("degenerate_in", 0)
            if it.get("imu") is not None:
                arr[i].imu = it["imu"]
        T = np.ascontiguousarray(T_init, np.float32).reshape(n, 6).copy()
        st = (Stats * max(n, 1))()
        self._chk(self._L.lisreg_align_batch(self._h, n, arr, C.byref(params),
                                             T.ctypes.data_as(C.POINTER(C.c_float)), st))
        return T, [stats_dict(st[i]) for i in range(n)]

    def batch_prepare_device(self, items: list[dict], T_init: np.ndarray, params: Params):
        """items: dicts with corner_ptr, n_corner, surf_ptr, n_surf (device pointers to 16-B records), target."""
        n = len(items)
        arr = (Item * max(n, 1))()
        for i, it in enumerate(items):
            arr[i].src_corner = C.c_void_p(it["corner_ptr"]) if it["n_corner"] else None
            arr[i].n_corner = it["n_corner"]
            arr[i].src_surf = C.c_void_p(it["surf_ptr"]) if it["n_surf"] else None
            arr[i].n_surf = it["n_surf"]
            arr[i].stride_bytes = 16; arr[i].fmt = FMT_DEVICE
            arr[i].target = it.get("target", 0); arr[i].degenerate_in = it.get("degenerate_in", 0)
            if it.get("imu") is not None:
                arr[i].imu = it["imu"]
        T = np.ascontiguousarray(T_init, np.float32).reshape(n, 6)
        self._n_items = n
        self._chk(self._L.lisreg_batch_prepare(self._h, n, arr, C.byref(params),
                                               T.ctypes.data_as(C.POINTER(C.c_float))))

    def batch_run(self):
        self._chk(self._L.lisreg_batch_run(self._h))

    def batch_fetch(self):
        n = self._n_items
        T = np.zeros((n, 6), np.float32)
        st = (Stats * max(n, 1))()
        self._chk(self._L.lisreg_batch_fetch(self._h, T.ctypes.data_as(C.POINTER(C.c_float)), st))
        return T, [stats_dict(st[i]) for i in range(n)]

    @property
    def result_device_ptr(self) -> int:
        return self._L.lisreg_batch_result_device(self._h) or 0

    def counters(self) -> np.ndarray:
        out = (C.c_ulonglong * 64)()
        self._chk(self._L.lisreg_get_counters(self._h, out, 64))
        return np.array(out[:], np.int64).reshape(32, 2)

    def target_index(self, slot: int = 0, kind: int = 1) -> dict:
        """Diagnostics: the device search index of a target (see lisreg_get_target_index)."""
        dims = (C.c_int * 5)(); geom = (C.c_float * 4)()
        self._chk(self._L.lisreg_get_target_index(self._h, slot, kind, dims, geom, None, 0, None, 0))
        n, nx, ny, nz, nc = [int(v) for v in dims]
        pts = np.zeros((max(n, 1), 4), np.float32); cs = np.zeros(nc + 1, np.int32)
        self._chk(self._L.lisreg_get_target_index(self._h, slot, kind, dims, geom, pts.ctypes.data, n, cs.ctypes.data, nc + 1))
        return dict(n=n, nx=nx, ny=ny, nz=nz, n_cells=nc, origin=np.array(geom[:3], np.float32), cell=float(geom[3]),
                    sorted=pts[:n], cell_start=cs)

    def target_graph(self, slot: int = 0, kind: int = 1) -> dict:
        """Diagnostics: the k-NN graph of a target (see lisreg_get_target_graph): ids [n, k] (sorted positions, -1 padded),
        xyz [n, k, 3], rho2 [n], count [n]."""
        n = self.target_index(slot, kind)["n"]
        k = C.c_int()
        self._chk(self._L.lisreg_get_target_graph(self._h, slot, kind, C.byref(k), None, None, 0))
        rows = np.zeros((max(n, 1), k.value, 4), np.float32); meta = np.zeros((max(n, 1), 2), np.float32)
        self._chk(self._L.lisreg_get_target_graph(self._h, slot, kind, C.byref(k), rows.ctypes.data_as(C.POINTER(C.c_float)),
                                                  meta.ctypes.data_as(C.POINTER(C.c_float)), n))
        return dict(k=k.value, ids=rows[:n, :, 3].copy().view(np.int32), xyz=rows[:n, :, :3], rho2=meta[:n, 0],
                    count=meta[:n, 1].copy().view(np.int32))

    def target_cell_rows(self, slot: int = 0, kind: int = 1) -> dict:
        """Diagnostics: the cell rows of a target (see lisreg_get_target_cell_rows): table [n_cells], ids [rows, k] (sorted positions,
        -1 padded), xyz [rows, k, 3], rho2 [rows], count [rows]."""
        n_rows, k = C.c_int(), C.c_int()
        # (the first call builds the rows if need be — which re-makes the target's grid with its two-cell margin: read the geometry after it)
        self._chk(self._L.lisreg_get_target_cell_rows(self._h, slot, kind, C.byref(n_rows), C.byref(k), None, 0, None, None, 0))
        nc = self.target_index(slot, kind)["n_cells"]
        table = np.zeros(max(nc, 1), np.int32)
        rows = np.zeros((max(n_rows.value, 1), k.value, 4), np.float32); meta = np.zeros((max(n_rows.value, 1), 2), np.float32)
        self._chk(self._L.lisreg_get_target_cell_rows(self._h, slot, kind, C.byref(n_rows), C.byref(k), table.ctypes.data_as(C.POINTER(C.c_int)), nc,
                                                      rows.ctypes.data_as(C.POINTER(C.c_float)), meta.ctypes.data_as(C.POINTER(C.c_float)), n_rows.value))
        r = n_rows.value
        return dict(k=k.value, n_rows=r, table=table[:nc], ids=rows[:r, :, 3].copy().view(np.int32), xyz=rows[:r, :, :3], rho2=meta[:r, 0],
                    count=meta[:r, 1].copy().view(np.int32))

    def raw_counters(self):
        out = (C.c_ulonglong * 128)()
        self._chk(self._L.lisreg_get_counters(self._h, out, 128))
        return [int(v) for v in out]

    def wave_counters(self) -> np.ndarray:
        """Graph front-end only: per GN iteration (wavefronts with at least one lane in the cell walk, wavefronts)."""
        out = (C.c_ulonglong * 128)()
        self._chk(self._L.lisreg_get_counters(self._h, out, 128))
        raw = np.array(out[64:96], np.uint64)
        return np.stack([(raw >> np.uint64(32)).astype(np.int64), (raw & np.uint64(0xffffffff)).astype(np.int64)], 1)

    # -- §8 f-1 -------------------------------------------------------------------------------------------
    def voxel_downsample(self, cloud: np.ndarray, leaf: float):
        """pcl::VoxelGrid replacement on a PCL struct array.  Returns (status, downsampled array)."""
        cloud = np.ascontiguousarray(cloud)
        out = np.zeros_like(cloud)
        n_out = C.c_int(0)
        rc = self._L.lisreg_voxel_downsample(self._h, _vp(cloud), len(cloud), cloud.dtype.itemsize, _fmt_of(cloud), leaf,
                                             out.ctypes.data_as(C.c_void_p), len(out), C.byref(n_out))
        self._chk(rc, allow=(OK, LEAF_TOO_SMALL))
        return rc, out[: n_out.value]

    def voxel_downsample_device(self, in_ptr: int, n: int, leaf: float, out_ptr: int, capacity: int, intensity: bool = False):
        """Device records in, device records out.  intensity=True: the payload is a float (PointXYZI clouds) and is averaged;
        otherwise it is a label and the voxel takes the majority."""
        n_out = C.c_int(0)
        rc = self._L.lisreg_voxel_downsample(self._h, C.c_void_p(in_ptr), n, 16, FMT_DEVICE_XYZI if intensity else FMT_DEVICE, leaf, C.c_void_p(out_ptr),
                                             capacity, C.byref(n_out))
        self._chk(rc, allow=(OK, LEAF_TOO_SMALL))
        return rc, n_out.value

    def voxel_downsample_multi_device(self, in_ptrs, counts, leafs, out_ptrs, capacities, intensity: bool = False):
        """K device clouds through ONE launch sequence (lisreg_voxel_downsample_multi); returns the K output counts."""
        k = len(in_ptrs)
        ins = (C.c_void_p * k)(*[C.c_void_p(int(p)) if c else None for p, c in zip(in_ptrs, counts)])
        outs = (C.c_void_p * k)(*[C.c_void_p(int(p)) if c else None for p, c in zip(out_ptrs, counts)])
        cnt = (C.c_int * k)(*[int(x) for x in counts]); cap = (C.c_int * k)(*[int(x) for x in capacities])
        lf = (C.c_float * k)(*[float(x) for x in leafs]); no = (C.c_int * k)()
        self._chk(self._L.lisreg_voxel_downsample_multi(self._h, k, ins, cnt, lf, FMT_DEVICE_XYZI if intensity else FMT_DEVICE, outs, cap, no))
        return [int(x) for x in no]

    def voxel_downsample_batch_device(self, in_ptrs, counts, leafs, out_ptrs, capacities, intensity: bool = False):
        """Up to VOXEL_BATCH_MAX device clouds through one launch sequence and one host synchronisation
        (lisreg_voxel_downsample_batch).  Returns (n_out, status): two lists with, per cloud, what voxel_downsample_device gives for
        it alone — status OK, LEAF_TOO_SMALL (the input was copied) or ERR_ARG (n_out = the count needed when the capacity was too
        small, 0 for a cloud with an infinite coordinate; nothing written).  Bad arguments raise."""
        k = len(in_ptrs)
        jobs = (VoxelJob * max(k, 1))()
        for s in range(k):
            jobs[s] = VoxelJob(int(in_ptrs[s]) or None, int(counts[s]), float(leafs[s]), int(out_ptrs[s]) or None, int(capacities[s]), 0, 0)
        self._chk(self._L.lisreg_voxel_downsample_batch(self._h, k, jobs, FMT_DEVICE_XYZI if intensity else FMT_DEVICE))
        return [int(jobs[s].n_out) for s in range(k)], [int(jobs[s].status) for s in range(k)]

    def transform_cloud(self, cloud: np.ndarray, T):
        cloud = np.ascontiguousarray(cloud)
        out = np.zeros_like(cloud)
        Tf = np.ascontiguousarray(T, np.float32)
        self._chk(self._L.lisreg_transform_cloud(self._h, _vp(cloud), len(cloud), cloud.dtype.itemsize, _fmt_of(cloud),
                                                 Tf.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.c_void_p)))
        return out

    def transform_cloud_device(self, in_ptr: int, n: int, T, out_ptr: int):
        Tf = np.ascontiguousarray(T, np.float32)
        self._chk(self._L.lisreg_transform_cloud(self._h, C.c_void_p(in_ptr), n, 16, FMT_DEVICE,
                                                 Tf.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(out_ptr)))

    # -- §8 f-2 -------------------------------------------------------------------------------------------
    def extract_features(self, cloud: np.ndarray, params: "FeatureParams", deskew: "Deskew | None" = None) -> dict:
        """LaserProcessing replacement on a PointXYZIRT struct array: the five clouds of cloud_info (optionally IMU-de-skewed)."""
        cloud = np.ascontiguousarray(cloud)
        cap = params.n_scan * params.horizon_scan
        names = ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")
        bufs = {k: np.zeros(cap, cloud.dtype) for k in names}
        fo = FeatureOut()
        for k in names:
            setattr(fo, k, bufs[k].ctypes.data_as(C.c_void_p)); setattr(fo, "cap_" + k, cap)
        self._chk(self._L.lisreg_extract_features_deskew(self._h, _vp(cloud), len(cloud), cloud.dtype.itemsize, FMT_XYZIRT,
                                                         C.byref(params), C.byref(deskew) if deskew is not None else None, C.byref(fo)))
        return {k: bufs[k][: getattr(fo, "n_" + k)] for k in names}

    def extract_features_device(self, in_ptr: int, n: int, params: "FeatureParams", out_ptrs: dict, cap: int, deskew=None) -> dict:
        fo = FeatureOut()
        for k, ptr in out_ptrs.items():
            setattr(fo, k, C.c_void_p(ptr)); setattr(fo, "cap_" + k, cap)
        self._chk(self._L.lisreg_extract_features_deskew(self._h, C.c_void_p(in_ptr), n, 16, FMT_DEVICE, C.byref(params),
                                                         C.byref(deskew) if deskew is not None else None, C.byref(fo)))
        return {k: getattr(fo, "n_" + k) for k in ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")}

    def extract_features_batch_device(self, in_ptrs, counts, params: "FeatureParams", out_ptrs: list, cap: int) -> list:
        """lisreg_extract_features_batch: in_ptrs / counts per sweep (device records), out_ptrs = one dict of five device buffers
        per sweep (capacity `cap` points each).  Returns the per-sweep count dicts."""
        S = len(in_ptrs)
        ptrs = (C.c_void_p * S)(*[C.c_void_p(int(p)) if n else None for p, n in zip(in_ptrs, counts)])
        ns = (C.c_int * S)(*[int(x) for x in counts])
        fos = (FeatureOut * S)()
        for s in range(S):
            for k, ptr in out_ptrs[s].items():
                setattr(fos[s], k, C.c_void_p(ptr)); setattr(fos[s], "cap_" + k, cap)
        self._chk(self._L.lisreg_extract_features_batch(self._h, S, ptrs, ns, C.byref(params), fos))
        return [{k: getattr(fos[s], "n_" + k) for k in ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")} for s in range(S)]

    def extract_features_deskew_batch_device(self, in_ptrs, counts, params: "FeatureParams", deskews, out_ptrs: list, cap: int) -> list:
        """lisreg_extract_features_deskew_batch: as extract_features_batch_device, with one Deskew (make_deskew with time_device_ptr; or
        None: that sweep is not de-skewed) per sweep, or deskews = None for the plain batch.  Returns the per-sweep count dicts."""
        S = len(in_ptrs)
        ptrs = (C.c_void_p * S)(*[C.c_void_p(int(p)) if n else None for p, n in zip(in_ptrs, counts)])
        ns = (C.c_int * S)(*[int(x) for x in counts])
        fos = (FeatureOut * S)()
        for s in range(S):
            for k, ptr in out_ptrs[s].items():
                setattr(fos[s], k, C.c_void_p(ptr)); setattr(fos[s], "cap_" + k, cap)
        dks = None
        if deskews is not None:
            assert len(deskews) == S
            dks = (Deskew * S)()
            for s, d in enumerate(deskews):
                if d is not None:
                    C.memmove(C.byref(dks[s]), C.byref(d), C.sizeof(Deskew))          # the tables stay alive with the caller's Deskew
        self._chk(self._L.lisreg_extract_features_deskew_batch(self._h, S, ptrs, ns, C.byref(params), dks, fos))
        return [{k: getattr(fos[s], "n_" + k) for k in ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")} for s in range(S)]

    # -- constant-velocity motion compensation (DistortionAdjust) -------------------------------------------
    def adjust_cloud(self, cloud: np.ndarray, motion: "Motion", capacity: int | None = None) -> np.ndarray:
        """DistortionAdjust::AdjustCloud on a PointXYZIRT struct array: points 1 .. n - 1 under the motion, as structs of the same dtype."""
        cloud = np.ascontiguousarray(cloud)
        n = len(cloud)
        cap = max(n - 1, 0) if capacity is None else capacity
        out = np.zeros(max(cap, 1), cloud.dtype)
        ao = AdjustOut()
        ao.cloud, ao.capacity = out.ctypes.data_as(C.c_void_p), cap
        self._chk(self._L.lisreg_adjust_cloud(self._h, _vp(cloud) if n else None, n, cloud.dtype.itemsize, FMT_XYZIRT, None, C.byref(motion),
                                              C.byref(ao)))
        return out[: ao.n]

    def adjust_cloud_device(self, in_ptr: int, n: int, time_ptr: int, motion: "Motion", out_ptr: int, out_time_ptr: int, cap: int) -> int:
        """lisreg_adjust_cloud on device records (ring in the payload) and their device times; returns the number of points written."""
        ao = AdjustOut()
        ao.cloud, ao.capacity, ao.time_device = C.c_void_p(out_ptr), cap, C.c_void_p(out_time_ptr)
        self._chk(self._L.lisreg_adjust_cloud(self._h, C.c_void_p(in_ptr) if n else None, n, 16, FMT_DEVICE, C.c_void_p(time_ptr) if n else None,
                                              C.byref(motion), C.byref(ao)))
        return ao.n

    def adjust_cloud_batch_device(self, in_ptrs, counts, time_ptrs, motions, out_ptrs, out_time_ptrs, cap) -> list:
        """lisreg_adjust_cloud_batch: per sweep device records, device times, a Motion and two output buffers of `cap` points (an int, or
        one per sweep).  Returns the per-sweep counts."""
        S = len(in_ptrs)
        caps = [int(cap)] * S if np.isscalar(cap) else [int(x) for x in cap]
        ptrs = (C.c_void_p * S)(*[C.c_void_p(int(p)) if n else None for p, n in zip(in_ptrs, counts)])
        tps = (C.c_void_p * S)(*[C.c_void_p(int(p)) if n else None for p, n in zip(time_ptrs, counts)])
        ns = (C.c_int * S)(*[int(x) for x in counts])
        ms = (Motion * S)()
        aos = (AdjustOut * S)()
        for s in range(S):
            C.memmove(C.byref(ms[s]), C.byref(motions[s]), C.sizeof(Motion))
            aos[s].cloud, aos[s].capacity, aos[s].time_device = C.c_void_p(int(out_ptrs[s])), caps[s], C.c_void_p(int(out_time_ptrs[s]))
        self._chk(self._L.lisreg_adjust_cloud_batch(self._h, S, ptrs, ns, tps, ms, aos))
        return [aos[s].n for s in range(S)]

    # -- laser pretreatment: ring and time of a raw sweep ---------------------------------------------------
    def pretreat(self, raw: np.ndarray, params: "PretreatParams", capacity: int | None = None, info: dict | None = None) -> np.ndarray:
        """LaserPretreatment::Pretreatment on a host sweep: an (n, 4) float32 array (x y z intensity, the packed 16-byte layout of KITTI's
        velodyne files) or a PCL struct array with the intensity at byte 16.  Returns the kept points as PointXYZIRT structs; `info`, when
        given, receives n, start_ori, end_ori and half_index."""
        from .synth import XYZIRT_DTYPE
        raw = np.ascontiguousarray(raw)
        if raw.dtype.names:
            fmt, n, stride = FMT_XYZI, len(raw), raw.dtype.itemsize
        else:
            raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 4)
            fmt, n, stride = FMT_XYZI_PACKED, len(raw), 16
        cap = n if capacity is None else capacity
        out = np.zeros(max(cap, 1), XYZIRT_DTYPE)
        po = PretreatOut()
        po.cloud, po.capacity = out.ctypes.data_as(C.c_void_p), cap
        rc = self._L.lisreg_pretreat(self._h, _vp(raw) if n else None, n, stride, fmt, C.byref(params), C.byref(po))
        if info is not None:
            info.update(po.as_dict())
        self._chk(rc)
        return out[: po.n]

    def pretreat_device(self, in_ptr: int, n: int, params: "PretreatParams", out_ptr: int, time_ptr: int, cap: int,
                        intensity_ptr: int | None = None) -> dict:
        """lisreg_pretreat on device records whose payload is the float intensity (a KITTI sweep copied to HBM as it is): ring records to
        out_ptr, times to time_ptr, intensities to intensity_ptr when given (`cap` points each).  Returns n, start_ori, end_ori, half_index."""
        po = PretreatOut()
        po.cloud, po.capacity, po.time_device = C.c_void_p(out_ptr), cap, C.c_void_p(time_ptr)
        po.intensity_device = C.c_void_p(intensity_ptr) if intensity_ptr else None
        self._chk(self._L.lisreg_pretreat(self._h, C.c_void_p(in_ptr), n, 16, FMT_DEVICE_XYZI, C.byref(params), C.byref(po)))
        return po.as_dict()

    def pretreat_batch_device(self, in_ptrs, counts, params: "PretreatParams", out_ptrs, time_ptrs, cap: int, intensity_ptrs=None) -> list:
        """lisreg_pretreat_batch: per sweep a device input, a record buffer and a time buffer (optionally an intensity buffer) of `cap`
        points.  Returns the per-sweep result dicts."""
        S = len(in_ptrs)
        ptrs = (C.c_void_p * S)(*[C.c_void_p(int(p)) if n else None for p, n in zip(in_ptrs, counts)])
        ns = (C.c_int * S)(*[int(x) for x in counts])
        pos = (PretreatOut * S)()
        for s in range(S):
            pos[s].cloud, pos[s].capacity, pos[s].time_device = C.c_void_p(int(out_ptrs[s])), cap, C.c_void_p(int(time_ptrs[s]))
            pos[s].intensity_device = C.c_void_p(int(intensity_ptrs[s])) if intensity_ptrs else None
        self._chk(self._L.lisreg_pretreat_batch(self._h, S, ptrs, ns, C.byref(params), pos))
        return [pos[s].as_dict() for s in range(S)]

    # -- RangeNet++ around the network: range-image projection and point labelling ---------------------------
    def rangenet_project(self, raw: np.ndarray, params: "RangenetParams", tensor_ptr: int, mask_ptr: int, pixel_ptr: int) -> int:
        """lisreg_rangenet_project on a host sweep: an (n, 4) float32 array (x y z intensity, packed 16-byte records) or a PCL struct
        array with the intensity at byte 16.  The outputs are the caller's device buffers.  Returns the number of valid pixels."""
        raw = np.ascontiguousarray(raw)
        if raw.dtype.names:
            fmt, n, stride = FMT_XYZI, len(raw), raw.dtype.itemsize
        else:
            raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 4)
            fmt, n, stride = FMT_XYZI_PACKED, len(raw), 16
        ro = RangenetOut(C.c_void_p(tensor_ptr), C.c_void_p(mask_ptr), C.c_void_p(pixel_ptr), 0)
        self._chk(self._L.lisreg_rangenet_project(self._h, _vp(raw) if n else None, n, stride, fmt, C.byref(params), C.byref(ro)))
        return ro.n_valid

    def rangenet_project_device(self, in_ptr: int, n: int, params: "RangenetParams", tensor_ptr: int, mask_ptr: int, pixel_ptr: int) -> int:
        """lisreg_rangenet_project on device records whose payload is the float intensity: the 5 x H x W float tensor to tensor_ptr (a
        torch tensor's data_ptr() will do), the H x W invalid mask (bytes) to mask_ptr, the per-point int32 pixel index to pixel_ptr;
        all complete when the call returns.  Returns the number of valid pixels."""
        ro = RangenetOut(C.c_void_p(tensor_ptr), C.c_void_p(mask_ptr), C.c_void_p(pixel_ptr), 0)
        self._chk(self._L.lisreg_rangenet_project(self._h, C.c_void_p(in_ptr) if n else None, n, 16, FMT_DEVICE_XYZI, C.byref(params), C.byref(ro)))
        return ro.n_valid

    def rangenet_project_batch_device(self, in_ptrs, counts, params: "RangenetParams", tensor_ptr: int, mask_ptrs, pixel_ptrs) -> list:
        """lisreg_rangenet_project_batch: sweep s writes plane block s of the (S, 5, H, W) float tensor at tensor_ptr, its own mask and
        its own pixel index.  Returns the per-sweep valid-pixel counts."""
        S = len(in_ptrs)
        ptrs = (C.c_void_p * S)(*[C.c_void_p(int(p)) if n else None for p, n in zip(in_ptrs, counts)])
        ns = (C.c_int * S)(*[int(x) for x in counts])
        ros = (RangenetOut * S)()
        plane = 5 * params.img_h * params.img_w * 4
        for s in range(S):
            ros[s].tensor, ros[s].invalid_mask, ros[s].pixel_index = C.c_void_p(int(tensor_ptr) + s * plane), C.c_void_p(int(mask_ptrs[s])), C.c_void_p(int(pixel_ptrs[s]))
        self._chk(self._L.lisreg_rangenet_project_batch(self._h, S, ptrs, ns, C.byref(params), ros))
        return [int(ros[s].n_valid) for s in range(S)]

    def rangenet_label_device(self, in_ptr: int, n: int, pixel_ptr: int, mask_ptr: int, logits_ptr: int, params: "RangenetParams",
                              out_ptr: int, image_ptr: int | None = None):
        """lisreg_rangenet_label: logits_ptr is the network's n_classes x H x W float output in HBM; out_ptr receives n device records
        (x y z bit for bit, label in the payload — what semantic_split_device takes), image_ptr the H x W label image when given."""
        self._chk(self._L.lisreg_rangenet_label(self._h, C.c_void_p(in_ptr) if n else None, n, FMT_DEVICE_XYZI, C.c_void_p(pixel_ptr) if n else None,
                                                C.c_void_p(mask_ptr), C.c_void_p(logits_ptr), C.byref(params), C.c_void_p(out_ptr) if n else None,
                                                C.c_void_p(image_ptr) if image_ptr else None))

    def rangenet_label_batch_device(self, in_ptrs, counts, pixel_ptrs, mask_ptrs, logits_ptrs, params: "RangenetParams", out_ptrs, image_ptrs=None):
        """lisreg_rangenet_label_batch: the per-sweep buffers of rangenet_label_device, one launch sequence."""
        S = len(in_ptrs)

        def arr(ps, gate=None):
            return (C.c_void_p * S)(*[C.c_void_p(int(p)) if (p and (gate is None or gate[k])) else None for k, p in enumerate(ps)])
        ns = (C.c_int * S)(*[int(x) for x in counts])
        self._chk(self._L.lisreg_rangenet_label_batch(self._h, S, arr(in_ptrs, counts), ns, arr(pixel_ptrs, counts), arr(mask_ptrs), arr(logits_ptrs),
                                                      C.byref(params), arr(out_ptrs, counts), arr(image_ptrs) if image_ptrs else None))

    def rangenet_label_knn_device(self, in_ptr: int, n: int, pixel_ptr: int, mask_ptr: int, logits_ptr: int, params: "RangenetParams",
                                  knn_params: "RangenetKnnParams", out_ptr: int, image_ptr: int | None = None, fmt: int = FMT_DEVICE_XYZI):
        """lisreg_rangenet_label_knn: rangenet_label_device followed by the kNN clean-up of RangeNet++ (a vote among the knn cells of a
        search x search window nearest in range); image_ptr receives the per-pixel argmax image, as in the plain call."""
        self._chk(self._L.lisreg_rangenet_label_knn(self._h, C.c_void_p(in_ptr) if n else None, n, fmt, C.c_void_p(pixel_ptr) if n else None,
                                                    C.c_void_p(mask_ptr), C.c_void_p(logits_ptr), C.byref(params), C.byref(knn_params),
                                                    C.c_void_p(out_ptr) if n else None, C.c_void_p(image_ptr) if image_ptr else None))

    def rangenet_label_knn_batch_device(self, in_ptrs, counts, pixel_ptrs, mask_ptrs, logits_ptrs, params: "RangenetParams",
                                        knn_params: "RangenetKnnParams", out_ptrs, image_ptrs=None):
        """lisreg_rangenet_label_knn_batch: the per-sweep buffers of rangenet_label_knn_device, one launch sequence."""
        S = len(in_ptrs)

        def arr(ps, gate=None):
            return (C.c_void_p * S)(*[C.c_void_p(int(p)) if (p and (gate is None or gate[k])) else None for k, p in enumerate(ps)])
        ns = (C.c_int * S)(*[int(x) for x in counts])
        self._chk(self._L.lisreg_rangenet_label_knn_batch(self._h, S, arr(in_ptrs, counts), ns, arr(pixel_ptrs, counts), arr(mask_ptrs),
                                                          arr(logits_ptrs), C.byref(params), C.byref(knn_params), arr(out_ptrs, counts),
                                                          arr(image_ptrs) if image_ptrs else None))

    def concat_device(self, in_ptrs, counts, out_ptr: int) -> int:
        """lisreg_concat_device: K device clouds end to end into out_ptr (stream-ordered, no wait).  Returns the total count."""
        k = len(in_ptrs)
        p = (C.c_void_p * k)(*[C.c_void_p(int(x)) for x in in_ptrs])
        n = (C.c_int * k)(*[int(x) for x in counts])
        tot = C.c_int(0)
        self._chk(self._L.lisreg_concat_device(self._h, k, p, n, C.c_void_p(int(out_ptr)), C.byref(tot)))
        return tot.value

    def upload_cloud(self, cloud: np.ndarray, dev_ptr: int) -> int:
        """lisreg_upload_cloud: a host PCL struct array (x, y, z at 0 / 4 / 8; the uint16 at byte 20 — label or ring — becomes the
        payload when the dtype has one) into a device buffer of len(cloud) 16-byte records.  Returns the count."""
        cloud = np.ascontiguousarray(cloud)
        if not cloud.dtype.names:                                    # a raw sweep: (n, 4) float32 x y z intensity, the records as they are
            cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
            self._chk(self._L.lisreg_upload_cloud(self._h, cloud.ctypes.data_as(C.c_void_p), len(cloud), 16, FMT_XYZI_PACKED, C.c_void_p(dev_ptr)))
            return len(cloud)
        names = cloud.dtype.names or ()
        has16 = any(cloud.dtype.fields[k][1] == 20 and cloud.dtype.fields[k][0].itemsize == 2 for k in names)
        self._chk(self._L.lisreg_upload_cloud(self._h, cloud.ctypes.data_as(C.c_void_p), len(cloud), cloud.dtype.itemsize,
                                              FMT_XYZIL if has16 else FMT_XYZI, C.c_void_p(dev_ptr)))
        return len(cloud)

    def semantic_split_device(self, in_ptr: int, n: int, out_ptrs, cap: int, using_label=None) -> list:
        """categoryMapping on device records (label in the payload): out_ptrs = five device buffers of `cap` records
        (dynamic, ground, building, pole, outlier).  Returns the five counts."""
        so = SemanticOut()
        for k in range(5):
            so.cloud[k] = int(out_ptrs[k]); so.cap[k] = cap
        m = (C.c_uint32 * 32)(*using_label) if using_label is not None else None
        self._chk(self._L.lisreg_semantic_split(self._h, C.c_void_p(in_ptr), n, 16, FMT_DEVICE, m, C.byref(so)))
        return [int(so.n[k]) for k in range(5)]

    def semantic_split_batch_device(self, in_ptrs, counts, out_ptrs, caps, using_label=None):
        """lisreg_semantic_split_batch: categoryMapping for up to SEMANTIC_BATCH_MAX labelled device clouds in three launches and one
        host synchronisation.  out_ptrs[frame][5]: device buffers (dynamic, ground, building, pole, outlier), 0 = that class is counted
        and not written; caps[frame][5] their capacities in records.  Returns (counts [frame][5], status [frame]): per frame what
        semantic_split_device gives for it alone, status OK or ERR_ARG (a capacity below its class count: the counts needed, nothing
        written).  Bad arguments raise."""
        k = len(in_ptrs)
        jobs = (SemanticJob * max(k, 1))()
        for s in range(k):
            jobs[s].in_ = int(in_ptrs[s]) or None
            jobs[s].n = int(counts[s])
            for q in range(5):
                jobs[s].out.cloud[q] = int(out_ptrs[s][q]) or None
                jobs[s].out.cap[q] = int(caps[s][q])
        m = (C.c_uint32 * 32)(*using_label) if using_label is not None else None
        self._chk(self._L.lisreg_semantic_split_batch(self._h, k, jobs, m))
        return [[int(jobs[s].out.n[q]) for q in range(5)] for s in range(k)], [int(jobs[s].status) for s in range(k)]

    def concat_device_batch(self, in_ptrs, counts, out_ptrs, capacities) -> list:
        """lisreg_concat_device_batch: up to CONCAT_BATCH_MAX jobs in one launch.  in_ptrs[job] / counts[job]: up to 8 device clouds
        (0 for an empty one) that go end to end into out_ptrs[job] (capacities[job] records).  Returns the totals."""
        k = len(in_ptrs)
        jobs = (ConcatJob * max(k, 1))()
        for s in range(k):
            jobs[s].k = len(in_ptrs[s])                      # more than 8: the library refuses the job by name
            for q in range(min(len(in_ptrs[s]), 8)):
                jobs[s].in_[q] = int(in_ptrs[s][q]) or None
                jobs[s].n[q] = int(counts[s][q])
            jobs[s].out = int(out_ptrs[s]) or None
            jobs[s].out_capacity = int(capacities[s])
        self._chk(self._L.lisreg_concat_device_batch(self._h, k, jobs))
        return [int(jobs[s].n_out) for s in range(k)]

    def align_device(self, corner_ptr: int, n_corner: int, surf_ptr: int, n_surf: int, T_init, params: Params, imu: Imu | None = None):
        """lisreg_align on device-resident source records.  Returns (T, stats dict)."""
        T = np.array(T_init, np.float32).copy()
        st = Stats()
        rc = self._L.lisreg_align(self._h, C.c_void_p(corner_ptr) if n_corner else None, n_corner, C.c_void_p(surf_ptr) if n_surf else None,
                                  n_surf, 16, FMT_DEVICE, C.byref(params), C.byref(imu) if imu is not None else None,
                                  T.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
        self._chk(rc, allow=(OK, NOT_ENOUGH_FEATURES, TOO_FEW_CORRESPONDENCES))
        d = stats_dict(st)
        if rc == NOT_ENOUGH_FEATURES:
            d["status"] = NOT_ENOUGH_FEATURES
        return T, d

    def semantic_split(self, cloud: np.ndarray, using_label=None) -> list:
        """categoryMapping replacement: [dynamic, ground, building, pole, outlier] from a PointXYZIL struct array."""
        cloud = np.ascontiguousarray(cloud)
        bufs = [np.zeros(len(cloud), cloud.dtype) for _ in range(5)]
        so = SemanticOut()
        for k in range(5):
            so.cloud[k] = bufs[k].ctypes.data_as(C.c_void_p).value if len(cloud) else None
            so.cap[k] = len(cloud)
        m = (C.c_uint32 * 32)(*using_label) if using_label is not None else None
        self._chk(self._L.lisreg_semantic_split(self._h, _vp(cloud), len(cloud), cloud.dtype.itemsize, FMT_XYZIL, m, C.byref(so)))
        return [bufs[k][: so.n[k]] for k in range(5)]

    # -- the odometry node's key-frame target, device-resident ------------------------------------------------
    def keyframes_reset(self, ring_id: int = 0):
        self._chk(self._L.lisreg_keyframes_reset(self._h, ring_id))

    def keyframes_push(self, ring_id: int, corner: np.ndarray, surf: np.ndarray, pose, max_keep: int = 19) -> dict:
        corner = np.ascontiguousarray(corner); surf = np.ascontiguousarray(surf)
        T = np.ascontiguousarray(pose, np.float32)
        info = KeyframesInfo()
        self._chk(self._L.lisreg_keyframes_push(self._h, ring_id, _vp(corner), len(corner), _vp(surf), len(surf), corner.dtype.itemsize,
                                                _fmt_of(corner), T.ctypes.data_as(C.POINTER(C.c_float)), max_keep, C.byref(info)))
        return dict(n_keyframes=info.n_keyframes)

    def keyframes_push_device(self, ring_id: int, corner_ptr: int, n_corner: int, surf_ptr: int, n_surf: int, pose, max_keep: int = 19,
                              label_payload: bool = False) -> dict:
        T = np.ascontiguousarray(pose, np.float32)
        info = KeyframesInfo()
        self._chk(self._L.lisreg_keyframes_push(self._h, ring_id, C.c_void_p(corner_ptr) if n_corner else None, n_corner,
                                                C.c_void_p(surf_ptr) if n_surf else None, n_surf, 16, FMT_DEVICE if label_payload else FMT_DEVICE_XYZI,
                                                T.ctypes.data_as(C.POINTER(C.c_float)), max_keep, C.byref(info)))
        return dict(n_keyframes=info.n_keyframes)

    def keyframes_target(self, ring_id: int, corner_leaf: float, surf_leaf: float, target_slot: int = 0) -> dict:
        info = KeyframesInfo()
        self._chk(self._L.lisreg_keyframes_target(self._h, ring_id, corner_leaf, surf_leaf, target_slot, C.byref(info)))
        return dict(n_keyframes=info.n_keyframes, n_target_corner=info.n_target_corner, n_target_surf=info.n_target_surf)

    # -- §8 f-3: device-resident sliding local map -----------------------------------------------------------
    def localmap_reset(self, map_id: int = 0):
        self._chk(self._L.lisreg_localmap_reset(self._h, map_id))

    def localmap_insert(self, map_id: int, clouds, pose, params: LocalMapParams) -> dict:
        """clouds: five PCL PointXYZIL struct arrays in LOCALMAP_CLASSES order (sensor frame, un-downsampled)."""
        arrs = [np.ascontiguousarray(a) for a in clouds]
        ptrs = (C.c_void_p * 5)(*[a.ctypes.data if len(a) else None for a in arrs])
        cnt = (C.c_int * 5)(*[len(a) for a in arrs])
        T = np.ascontiguousarray(pose, np.float32)
        info = LocalMapInfo()
        self._chk(self._L.lisreg_localmap_insert(self._h, map_id, ptrs, cnt, arrs[0].dtype.itemsize, _fmt_of(arrs[0]),
                                                 T.ctypes.data_as(C.POINTER(C.c_float)), C.byref(params), C.byref(info)))
        return _info_dict(info)

    def localmap_insert_device(self, map_id: int, ptrs, counts, pose, params: LocalMapParams) -> dict:
        p = (C.c_void_p * 5)(*[C.c_void_p(int(x)) if c else None for x, c in zip(ptrs, counts)])
        cnt = (C.c_int * 5)(*[int(x) for x in counts])
        T = np.ascontiguousarray(pose, np.float32)
        info = LocalMapInfo()
        self._chk(self._L.lisreg_localmap_insert(self._h, map_id, p, cnt, 16, FMT_DEVICE,
                                                 T.ctypes.data_as(C.POINTER(C.c_float)), C.byref(params), C.byref(info)))
        return _info_dict(info)

    def localmap_extract(self, map_id: int, cur_pose, params: LocalMapParams, target_slot: int = 0) -> dict:
        T = np.ascontiguousarray(cur_pose, np.float32)
        info = LocalMapInfo()
        self._chk(self._L.lisreg_localmap_extract(self._h, map_id, T.ctypes.data_as(C.POINTER(C.c_float)), C.byref(params),
                                                  target_slot, C.byref(info)))
        return _info_dict(info)

    # -- copy #3: submap_t + insert_submap + extractSubMapCloud (device-resident) ------------------------------------
    def submap_insert(self, map_id: int, clouds, relative_pose, submap_pose, params: LocalMapParams) -> dict:
        """clouds: the key frame's five DOWN-sampled class clouds (LOCALMAP_CLASSES order); relative_pose None = fisrt_submap."""
        arrs = [np.ascontiguousarray(a) for a in clouds]
        ptrs = (C.c_void_p * 5)(*[a.ctypes.data if len(a) else None for a in arrs])
        cnt = (C.c_int * 5)(*[len(a) for a in arrs])
        Tr = None if relative_pose is None else np.ascontiguousarray(relative_pose, np.float32)
        Ts = np.ascontiguousarray(submap_pose, np.float32)
        info = SubmapInfo()
        fp = C.POINTER(C.c_float)
        self._chk(self._L.lisreg_submap_insert(self._h, map_id, ptrs, cnt, arrs[0].dtype.itemsize, _fmt_of(arrs[0]),
                                               Tr.ctypes.data_as(fp) if Tr is not None else None, Ts.ctypes.data_as(fp), C.byref(params), C.byref(info)))
        return dict(n=list(info.n), feature_point_num=info.feature_point_num, local_bound=np.array(info.local_bound[:], np.float64),
                    bound=np.array(info.bound[:], np.float64))

    def submap_extract(self, pre_id: int, cur_id: int, pre_pose, cur_pose, pad: float = 10.0, corner_leaf: float = 0.2,
                       surf_leaf: float = 0.5, target_slot: int = 0) -> dict:
        Tp = np.ascontiguousarray(pre_pose, np.float32); Tc = np.ascontiguousarray(cur_pose, np.float32)
        out = SubmapExtractOut()
        fp = C.POINTER(C.c_float)
        self._chk(self._L.lisreg_submap_extract(self._h, pre_id, cur_id, Tp.ctypes.data_as(fp), Tc.ctypes.data_as(fp), pad, corner_leaf,
                                                surf_leaf, target_slot, C.byref(out)))
        return dict(isect=np.array(out.isect[:], np.float64), isect_local=np.array(out.isect_local[:], np.float64),
                    n_target_corner=out.n_target_corner, n_target_surf=out.n_target_surf,
                    src_corner_ptr=out.src_corner or 0, n_src_corner=out.n_src_corner, src_surf_ptr=out.src_surf or 0, n_src_surf=out.n_src_surf)

    def submap_insert_device(self, map_id: int, ptrs, counts, relative_pose, submap_pose, params: LocalMapParams) -> dict:
        """submap_insert for five clouds of device records (payload = label bits); relative_pose None = fisrt_submap."""
        p = (C.c_void_p * 5)(*[C.c_void_p(int(x)) if c else None for x, c in zip(ptrs, counts)])
        cnt = (C.c_int * 5)(*[int(x) for x in counts])
        Tr = None if relative_pose is None else np.ascontiguousarray(relative_pose, np.float32)
        Ts = np.ascontiguousarray(submap_pose, np.float32)
        info = SubmapInfo()
        fp = C.POINTER(C.c_float)
        self._chk(self._L.lisreg_submap_insert(self._h, map_id, p, cnt, 16, FMT_DEVICE, Tr.ctypes.data_as(fp) if Tr is not None else None,
                                               Ts.ctypes.data_as(fp), C.byref(params), C.byref(info)))
        return dict(n=list(info.n), feature_point_num=info.feature_point_num, local_bound=np.array(info.local_bound[:], np.float64),
                    bound=np.array(info.bound[:], np.float64))

    # -- the global map: chosen classes of a list of resident submaps, each under its own pose, as one cloud ------------------------
    @staticmethod
    def _gather_list(map_ids, poses):
        ids = np.ascontiguousarray(map_ids, np.int32).ravel()
        T = None
        if poses is not None:
            T = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
            if len(T) != len(ids):
                raise ValueError("submap_gather: one pose per listed map")
        return ids, T

    def submap_gather_count(self, map_ids, class_mask: int = CLS_ALL):
        """(points the gather would write, int64 segment starts [len(map_ids) * 5 + 1]); segment 5 * i + k = class k of map_ids[i]."""
        ids, _ = self._gather_list(map_ids, None)
        n = C.c_longlong(0)
        off = np.zeros(len(ids) * 5 + 1, np.int64)
        self._chk(self._L.lisreg_submap_gather_count(self._h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int)), class_mask, C.byref(n),
                                                     off.ctypes.data_as(C.POINTER(C.c_longlong))))
        return n.value, off

    def submap_gather_device(self, map_ids, poses, out_ptr: int, capacity_points: int, class_mask: int = CLS_ALL, out_fmt: int = FMT_DEVICE,
                             chunk_points: int = 0):
        """The gather into caller memory (a device pointer: one launch on the context's stream, not waited for; a host address: chunked,
        complete on return).  poses: [len(map_ids), 6] or None (records copied bit for bit).  Returns (points written, segment starts)."""
        ids, T = self._gather_list(map_ids, poses)
        prm = GatherParams(class_mask, out_fmt, chunk_points)
        n = C.c_longlong(0)
        off = np.zeros(len(ids) * 5 + 1, np.int64)
        self._chk(self._L.lisreg_submap_gather(self._h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int)),
                                               T.ctypes.data_as(C.POINTER(C.c_float)) if T is not None else None, C.byref(prm),
                                               C.c_void_p(int(out_ptr)) if out_ptr else None, capacity_points, C.byref(n),
                                               off.ctypes.data_as(C.POINTER(C.c_longlong))))
        return n.value, off

    def submap_gather(self, map_ids, poses=None, class_mask: int = CLS_ALL, out_fmt: int = FMT_DEVICE, chunk_points: int = 0):
        """The gather into a new host array: [n, 4] float32 records (x, y, z, label bits) for FMT_DEVICE, 32-byte PointXYZIL structs
        (intensity 0) for FMT_XYZIL.  Returns (cloud, segment starts)."""
        n, _ = self.submap_gather_count(map_ids, class_mask)
        if out_fmt == FMT_XYZIL:
            from .synth import PCL_DTYPE
            out = np.zeros(max(n, 1), PCL_DTYPE)
        else:
            out = np.zeros((max(n, 1), 4), np.float32)
        m, off = self.submap_gather_device(map_ids, poses, out.ctypes.data, n, class_mask, out_fmt, chunk_points)
        return out[:m], off

    def localmap_get(self, map_id: int, cls: int) -> np.ndarray:
        """[n, 4] float32 records (x, y, z, label bits) of class cls (0-4) or of the corner / surf target (5 / 6)."""
        n = C.c_int(0)
        self._L.lisreg_localmap_get(self._h, map_id, cls, None, 0, C.byref(n))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        self._chk(self._L.lisreg_localmap_get(self._h, map_id, cls, out.ctypes.data_as(C.c_void_p), max(n.value, 1), C.byref(n)))
        return out[: n.value]

    # -- §8 f-3 -------------------------------------------------------------------------------------------
    def map_index_set(self, slot: int, cloud: np.ndarray):
        cloud = np.ascontiguousarray(cloud)
        self._chk(self._L.lisreg_map_index_set(self._h, slot, _vp(cloud), len(cloud), cloud.dtype.itemsize, _fmt_of(cloud)))

    def map_index_set_batch(self, slots, clouds):
        """lisreg_map_index_set_batch: clouds = host PCL-struct arrays (one dtype), or (device_ptr, n) tuples"""
        k = len(slots)
        sl = (C.c_int * max(k, 1))(*[int(v) for v in slots])
        ptrs = (C.c_void_p * max(k, 1))(); cnt = (C.c_int * max(k, 1))()
        keep, fmt, stride = [], FMT_DEVICE, 16
        for i, cl in enumerate(clouds):
            if isinstance(cl, tuple):
                ptrs[i], cnt[i] = C.c_void_p(cl[0]), cl[1]
            else:
                cl = np.ascontiguousarray(cl); keep.append(cl)
                ptrs[i], cnt[i] = C.c_void_p(cl.ctypes.data if len(cl) else 0), len(cl)
                fmt, stride = _fmt_of(cl), cl.dtype.itemsize
        self._chk(self._L.lisreg_map_index_set_batch(self._h, k, sl, ptrs, cnt, stride, fmt))

    def map_index_set_device(self, slot: int, ptr: int, n: int):
        self._chk(self._L.lisreg_map_index_set(self._h, slot, C.c_void_p(ptr), n, 16, FMT_DEVICE))

    def nearest(self, slot: int, query: np.ndarray, max_dist: float = 1e18):
        """k = 1 search: (idx [n] int32, -1 beyond max_dist; squared distance [n] float32)."""
        query = np.ascontiguousarray(query)
        idx = np.zeros(len(query), np.int32)
        sqd = np.zeros(len(query), np.float32)
        self._chk(self._L.lisreg_nearest(self._h, slot, _vp(query), len(query), query.dtype.itemsize, _fmt_of(query),
                                         max_dist, idx.ctypes.data_as(C.c_void_p), sqd.ctypes.data_as(C.c_void_p)))
        return idx, sqd

    def map_grid(self, slot: int) -> dict:
        """Diagnostics (lisreg_get_map_grid): dict(n, dims=(nx, ny, nz), n_cells, o=float32[3], cell) of the map index of `slot`."""
        d = np.zeros(5, np.int32); g = np.zeros(4, np.float32)
        self._chk(self._L.lisreg_get_map_grid(self._h, int(slot), d.ctypes.data_as(C.POINTER(C.c_int)), g.ctypes.data_as(C.POINTER(C.c_float))))
        return dict(n=int(d[0]), dims=(int(d[1]), int(d[2]), int(d[3])), n_cells=int(d[4]), o=g[:3].copy(), cell=g[3])

    def test_nn1(self, slot: int, queries: np.ndarray, max_dist: float, form: int, seeds=None):
        """Test hook (lisreg_test_nn1): ONE form of the k = 1 search per query — form 1, 4, 8: nn1_search<Q>, 0: nn1_search_flat — on
        queries[n, 3]; seeds[n] (or None): original map indices, -1 none, -2 the cell seed of ICP's first iteration.  Returns
        (idx [n] int32 original index or -1, squared distance [n] float32)."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
        n = q.shape[0]
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray(seeds, np.int32).ravel()
            assert len(sd) == n
        idx = np.zeros(n, np.int32)
        sqd = np.zeros(n, np.float32)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        self._chk(self._L.lisreg_test_nn1(self._h, int(slot), q.ctypes.data_as(fp), n, float(max_dist), int(form),
                                          None if sd is None else sd.ctypes.data_as(ip), idx.ctypes.data_as(ip), sqd.ctypes.data_as(fp)))
        return idx, sqd

    def test_scan(self, in0, in1=None, in_offset: int = 0, out_offset: int = 0, in_place: bool = False):
        """Test hook (lisreg_test_scan): the exclusive scan as production dispatches it.  in1 None: out0 [n0 + 1] int32 of in0 (out0[n0] =
        the total).  Otherwise the pair form of the cell rows: (out0, out1), None for a half with n = 0 (off, as in production).  The
        offsets (0 to 3 ints off a 16-byte aligned device address) choose the vector or the scalar path; in_place: out = in."""
        a = [np.ascontiguousarray(in0, np.int32).ravel(), None if in1 is None else np.ascontiguousarray(in1, np.int32).ravel()]
        ip = C.POINTER(C.c_int)
        # (an empty array still hands over a pointer: in1 != NULL is what selects the pair form)
        src = [None if v is None else (v if len(v) else np.zeros(1, np.int32)) for v in a]
        out = [None if v is None else np.full(len(v) + 1, -1, np.int32) for v in a]
        self._chk(self._L.lisreg_test_scan(self._h, src[0].ctypes.data_as(ip), len(a[0]), None if a[1] is None else src[1].ctypes.data_as(ip),
                                           0 if a[1] is None else len(a[1]), int(in_offset), int(out_offset), 1 if in_place else 0,
                                           out[0].ctypes.data_as(ip), None if a[1] is None else out[1].ctypes.data_as(ip)))
        if in1 is None:
            return out[0]
        return tuple(o if len(v) else None for o, v in zip(out, a))

    def nearest_device(self, slot: int, q_ptr: int, n: int, max_dist: float, idx_ptr: int, sqd_ptr: int):
        self._chk(self._L.lisreg_nearest(self._h, slot, C.c_void_p(q_ptr), n, 16, FMT_DEVICE, max_dist,
                                         C.c_void_p(idx_ptr), C.c_void_p(sqd_ptr)))

    def dynamic_filter(self, slot: int, cloud: np.ndarray, center_radius: float, dist_thre_min: float = 3.4028234663852886e38,
                       dist_thre_max: float = 3.4028234663852886e38, near_dist_thre: float = 0.0):
        """map_scan_feature_pts_distance_removal: (filtered cloud, applied) — applied False where the reference returns false."""
        cloud = np.ascontiguousarray(cloud)
        out = np.zeros_like(cloud)
        m = C.c_int(0)
        rc = self._chk(self._L.lisreg_dynamic_filter(self._h, slot, _vp(cloud), len(cloud), cloud.dtype.itemsize, _fmt_of(cloud),
                                                     center_radius, dist_thre_min, dist_thre_max, near_dist_thre,
                                                     out.ctypes.data_as(C.c_void_p), C.byref(m)),
                       allow=(OK, NOT_ENOUGH_FEATURES))
        return out[: m.value], rc == OK

    def dynamic_filter_device(self, slot: int, in_ptr: int, n: int, center_radius: float, dist_thre_min: float,
                              dist_thre_max: float, near_dist_thre: float, out_ptr: int) -> int:
        m = C.c_int(0)
        self._chk(self._L.lisreg_dynamic_filter(self._h, slot, C.c_void_p(in_ptr), n, 16, FMT_DEVICE, center_radius,
                                                dist_thre_min, dist_thre_max, near_dist_thre, C.c_void_p(out_ptr), C.byref(m)),
                  allow=(OK, NOT_ENOUGH_FEATURES))
        return m.value

    def bbx_filter(self, cloud: np.ndarray, bounds, delete_box: bool = False) -> np.ndarray:
        """bounds = (min_x, min_y, min_z, max_x, max_y, max_z)"""
        cloud = np.ascontiguousarray(cloud)
        out = np.zeros_like(cloud)
        m = C.c_int(0)
        b = (C.c_double * 6)(*[float(v) for v in bounds])
        self._chk(self._L.lisreg_bbx_filter(self._h, _vp(cloud), len(cloud), cloud.dtype.itemsize, _fmt_of(cloud), b,
                                            1 if delete_box else 0, out.ctypes.data_as(C.c_void_p), C.byref(m)))
        return out[: m.value]

    def bbx_filter_device(self, in_ptr: int, n: int, bounds, delete_box: bool, out_ptr: int) -> int:
        m = C.c_int(0)
        b = (C.c_double * 6)(*[float(v) for v in bounds])
        self._chk(self._L.lisreg_bbx_filter(self._h, C.c_void_p(in_ptr), n, 16, FMT_DEVICE, b, 1 if delete_box else 0,
                                            C.c_void_p(out_ptr), C.byref(m)))
        return m.value

    def cloud_bounds(self, cloud: np.ndarray) -> np.ndarray:
        cloud = np.ascontiguousarray(cloud)
        b = (C.c_double * 6)()
        self._chk(self._L.lisreg_cloud_bounds(self._h, _vp(cloud), len(cloud), cloud.dtype.itemsize, _fmt_of(cloud), b))
        return np.array(list(b))

    # -- §8 f-4 -------------------------------------------------------------------------------------------
    def icp_align(self, slot: int, source: np.ndarray, params: "IcpParams", guess=None, want_aligned: bool = False):
        """pcl::IterativeClosestPoint::align against the map index in `slot`; returns the result dict (+ 'aligned')."""
        source = np.ascontiguousarray(source)
        res = IcpResult()
        g = None if guess is None else np.ascontiguousarray(guess, np.float32).ravel().ctypes.data_as(C.POINTER(C.c_float))
        out = np.zeros_like(source) if want_aligned else None
        self._chk(self._L.lisreg_icp_align(self._h, slot, _vp(source), len(source), source.dtype.itemsize, _fmt_of(source),
                                           C.byref(params), g, C.byref(res), _vp(out) if want_aligned else None))
        d = res.as_dict()
        if want_aligned:
            d["aligned"] = out
        return d

    def icp_align_batch(self, items, params: "IcpParams", chain_prev_mse: bool = False):
        """lisreg_icp_align_batch: items = [(slot, source, guess or None), ...] — host PCL-struct arrays (one dtype for the batch), or
        (slot, (device_ptr, n), guess) tuples for LISREG_FMT_DEVICE records.  Returns the list of result dicts, one per item."""
        n = len(items)
        arr = (IcpItem * max(n, 1))()
        keep = []
        fmt, stride = None, 16
        for k, (slot, source, guess) in enumerate(items):
            if isinstance(source, tuple):
                ptr, cnt = source
                arr[k].source = C.c_void_p(ptr); arr[k].n = cnt
                f, st = FMT_DEVICE, 16
            else:
                source = np.ascontiguousarray(source)
                keep.append(source)
                arr[k].source = C.c_void_p(source.ctypes.data if len(source) else 0); arr[k].n = len(source)
                f, st = _fmt_of(source), source.dtype.itemsize
            if fmt is None:
                fmt, stride = f, st
            elif (fmt, stride) != (f, st):
                raise ValueError("icp_align_batch: one point format per batch")
            arr[k].slot = slot
            if guess is not None:
                g = np.ascontiguousarray(guess, np.float32).ravel()
                keep.append(g)
                arr[k].guess = g.ctypes.data_as(C.POINTER(C.c_float))
        res = (IcpResult * max(n, 1))()
        self._chk(self._L.lisreg_icp_align_batch(self._h, arr, n, stride, FMT_DEVICE if fmt is None else fmt, C.byref(params),
                                                 1 if chain_prev_mse else 0, res))
        return [res[k].as_dict() for k in range(n)]

    # ---- FEPSC loop-closure candidate detection (EPSCGeneration::loopDetection) ----
    @staticmethod
    def _loop_clouds(clouds):
        """(corner, surf, semantic): host PCL struct arrays (one itemsize), or (device_ptr, n) tuples of LISREG_FMT_DEVICE records."""
        ptrs, ns, fmt, stride = [], [], None, 32
        for cl in clouds:
            if isinstance(cl, tuple):
                ptrs.append(C.c_void_p(cl[0])); ns.append(int(cl[1])); f, st = FMT_DEVICE, 16
            else:
                ptrs.append(C.c_void_p(cl.ctypes.data if len(cl) else 0)); ns.append(len(cl)); f, st = FMT_XYZIL, cl.dtype.itemsize
            if fmt is None:
                fmt, stride = f, st
            elif (fmt, stride) != (f, st):
                raise ValueError("loop detection: one point format per call")
        return ptrs, ns, fmt, stride

    def loopdet_reset(self, db_id: int = 0):
        """lisreg_loopdet_reset: forget every frame of database db_id."""
        self._chk(self._L.lisreg_loopdet_reset(self._h, db_id))

    def loopdet_detect(self, frames, db_id: int = 0, params: "LoopdetParams" = None):
        """lisreg_loopdet_detect: frames = [(corner, surf, semantic, odom), ...] with odom a row-major 3 x 4 (or 4 x 4) matrix.
        Returns one result dict per frame."""
        n = len(frames)
        arr = (LoopdetFrame * max(n, 1))()
        keep, fmt, stride = [], FMT_XYZIL, 32
        for k, (corner, surf, semantic, odom) in enumerate(frames):
            clouds = [c if isinstance(c, tuple) else np.ascontiguousarray(c) for c in (corner, surf, semantic)]
            keep.extend(clouds)
            (p0, p1, p2), (n0, n1, n2), f, st = self._loop_clouds(clouds)
            if k == 0:
                fmt, stride = f, st
            elif (fmt, stride) != (f, st):
                raise ValueError("loopdet_detect: one point format per call")
            arr[k].corner, arr[k].n_corner, arr[k].surf, arr[k].n_surf, arr[k].semantic, arr[k].n_semantic = p0, n0, p1, n1, p2, n2
            o = np.asarray(odom, np.float32).reshape(-1, 4)[:3].ravel()
            for i in range(12):
                arr[k].odom[i] = float(o[i])
        res = (LoopdetResult * max(n, 1))()
        self._chk(self._L.lisreg_loopdet_detect(self._h, db_id, arr, n, stride, fmt, C.byref(params) if params is not None else None, res))
        return [res[k].as_dict() for k in range(n)]

    def loopdet_candidates(self, k: int, db_id: int = 0):
        """lisreg_loopdet_candidates: every gated candidate of frame k of the last detect call, in history order."""
        cnt = C.c_int(0)
        self._chk(self._L.lisreg_loopdet_candidates(self._h, db_id, k, None, 0, C.byref(cnt)))
        out = (LoopdetCandidate * max(cnt.value, 1))()
        self._chk(self._L.lisreg_loopdet_candidates(self._h, db_id, k, out, cnt.value, C.byref(cnt)))
        return [out[j].as_dict() for j in range(cnt.value)]

    def loopdet_get(self, frame_id: int, db_id: int = 0):
        """lisreg_loopdet_get: (FEPSC uint8 [20, 80], projection float32 [360, 4]) stored for frame_id."""
        d = np.zeros((20, 80), np.uint8)
        pr = np.zeros((360, 4), np.float32)
        self._chk(self._L.lisreg_loopdet_get(self._h, db_id, frame_id, d.ctypes.data_as(C.POINTER(C.c_uint8)), pr.ctypes.data_as(C.POINTER(C.c_float))))
        return d, pr

    def loop_descriptor(self, corner, surf, semantic, M=None):
        """lisreg_loop_descriptor: dict of fepsc / epsc / sepsc (uint8 [20, 80]) and projection (float32 [360, 4]) under M."""
        clouds = [c if isinstance(c, tuple) else np.ascontiguousarray(c) for c in (corner, surf, semantic)]
        (p0, p1, p2), (n0, n1, n2), fmt, stride = self._loop_clouds(clouds)
        m = None if M is None else np.ascontiguousarray(M, np.float32).ravel()
        out = {k: np.zeros((20, 80), np.uint8) for k in ("fepsc", "epsc", "sepsc")}
        out["projection"] = np.zeros((360, 4), np.float32)
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        self._chk(self._L.lisreg_loop_descriptor(self._h, p0, n0, p1, n1, p2, n2, stride, fmt, None if m is None else m.ctypes.data_as(C.POINTER(C.c_float)),
                                                 u8(out["fepsc"]), u8(out["epsc"]), u8(out["sepsc"]), out["projection"].ctypes.data_as(C.POINTER(C.c_float))))
        return out

    # ---- the other loopDetection selectors (ISC, SC, EPSC, SEPSC, SSC, Pose) ----
    def loopdet_configure(self, kinds, db_id: int = 0, label_threshold: float = LOOP_LABEL_THRESHOLD):
        """lisreg_loopdet_configure: the kinds (a LOOP_* mask or names) of an empty database, and SSC's threshold."""
        self._chk(self._L.lisreg_loopdet_configure(self._h, db_id, loop_kinds(kinds), label_threshold))

    def loopdet_matches(self, k: int, db_id: int = 0):
        """lisreg_loopdet_matches: the matched list of frame k of the last detect call (matched_frame_id / _transform), push order."""
        cnt = C.c_int(0)
        out = (LoopdetMatch * 7)()
        self._chk(self._L.lisreg_loopdet_matches(self._h, db_id, k, out, 7, C.byref(cnt)))
        return [out[j].as_dict() for j in range(cnt.value)]

    def loopdet_candidate_scores(self, k: int, db_id: int = 0):
        """lisreg_loopdet_candidate_scores: per gated candidate of frame k, the score (and shift) of every kind, by kind index."""
        cnt = C.c_int(0)
        self._chk(self._L.lisreg_loopdet_candidate_scores(self._h, db_id, k, None, 0, C.byref(cnt)))
        out = (LoopdetKindScores * max(cnt.value, 1))()
        self._chk(self._L.lisreg_loopdet_candidate_scores(self._h, db_id, k, out, cnt.value, C.byref(cnt)))
        return [out[j].as_dict() for j in range(cnt.value)]

    def loopdet_get_descriptor(self, frame_id: int, kind, db_id: int = 0):
        """lisreg_loopdet_get_descriptor: the stored uint8 [20, 80] descriptor of one enabled kind of frame_id."""
        d = np.zeros((20, 80), np.uint8)
        self._chk(self._L.lisreg_loopdet_get_descriptor(self._h, db_id, frame_id, loop_kinds([kind] if isinstance(kind, str) else kind),
                                                        d.ctypes.data_as(C.POINTER(C.c_uint8))))
        return d

    def loop_descriptor_kind(self, kind, corner, surf, semantic, M=None):
        """lisreg_loop_descriptor_kind: one kind's uint8 [20, 80] descriptor of the clouds moved by M."""
        clouds = [c if isinstance(c, tuple) else np.ascontiguousarray(c) for c in (corner, surf, semantic)]
        (p0, p1, p2), (n0, n1, n2), fmt, stride = self._loop_clouds(clouds)
        m = None if M is None else np.ascontiguousarray(M, np.float32).ravel()
        d = np.zeros((20, 80), np.uint8)
        self._chk(self._L.lisreg_loop_descriptor_kind(self._h, loop_kinds([kind] if isinstance(kind, str) else kind), p0, n0, p1, n1, p2, n2,
                                                      stride, fmt, None if m is None else m.ctypes.data_as(C.POINTER(C.c_float)),
                                                      d.ctypes.data_as(C.POINTER(C.c_uint8))))
        return d

    def icp_gn_match(self, slot: int, source: np.ndarray, max_iterations: int, max_correspond_distance: float, predict_pose,
                     want_transformed: bool = False):
        """OptimizedICPGN::Match + GetFitnessScore against the map index in `slot`."""
        source = np.ascontiguousarray(source)
        res = IcpGnResult()
        g = np.ascontiguousarray(predict_pose, np.float32).ravel()
        out = np.zeros_like(source) if want_transformed else None
        self._chk(self._L.lisreg_icp_gn_match(self._h, slot, _vp(source), len(source), source.dtype.itemsize, _fmt_of(source),
                                              max_iterations, max_correspond_distance, g.ctypes.data_as(C.POINTER(C.c_float)),
                                              C.byref(res), _vp(out) if want_transformed else None))
        d = dict(T=np.array(list(res.final_transform), np.float32).reshape(4, 4), steps_applied=res.steps_applied,
                 n_corr_last=res.n_corr_last, fitness=res.fitness)
        if want_transformed:
            d["transformed"] = out
        return d

    def icp_gn_match_batch(self, sources, items, max_iterations: int, max_correspond_distance: float):
        """lisreg_icp_gn_match_batch: sources = a list of clouds (all host PCL-struct arrays of one dtype, or all (device_ptr, n); None
        for a source no item names), items = a list of IcpGnItem.  Returns (results, info): per item icp_gn_match's dict plus
        'bytes', the 80 bytes of its lisreg_icpgn_result; info = dict(best, n_sources_staged, n_syncs)."""
        args = [(None, 0, None, None, None) if s is None else self._cloud_args(s) for s in sources]
        layouts = {(a[2], a[3]) for a in args if a[2] is not None}
        if len(layouts) > 1:
            raise ValueError("icp_gn_match_batch: the sources of one call share one layout")
        stride, fmt = layouts.pop() if layouts else (16, FMT_DEVICE)
        ptrs = (C.c_void_p * max(len(args), 1))(*[a[0] for a in args])
        ns = (C.c_int * max(len(args), 1))(*[a[1] for a in args])
        its = (IcpGnItemC * max(len(items), 1))()
        keep = []
        for k, it in enumerate(items):
            its[k].source, its[k].slot = it.source, it.slot
            if it.predict_pose is not None:
                g = np.ascontiguousarray(it.predict_pose, np.float32).ravel()
                keep.append(g)
                its[k].predict_pose = g.ctypes.data_as(C.POINTER(C.c_float))
        res = (IcpGnResult * max(len(items), 1))()
        info = IcpGnBatchInfo()
        self._chk(self._L.lisreg_icp_gn_match_batch(self._h, ptrs, ns, len(args), stride, fmt, its, len(items), max_iterations,
                                                    max_correspond_distance, res, C.byref(info)))
        return ([dict(res[k].as_dict(), bytes=bytes(res[k])) for k in range(len(items))],
                dict(best=info.best, n_sources_staged=info.n_sources_staged, n_syncs=info.n_syncs))

    def icp_align_device(self, slot: int, src_ptr: int, n: int, params: "IcpParams", guess=None, out_ptr: int = 0):
        res = IcpResult()
        g = None if guess is None else np.ascontiguousarray(guess, np.float32).ravel().ctypes.data_as(C.POINTER(C.c_float))
        self._chk(self._L.lisreg_icp_align(self._h, slot, C.c_void_p(src_ptr), n, 16, FMT_DEVICE, C.byref(params), g,
                                           C.byref(res), C.c_void_p(out_ptr) if out_ptr else None))
        return res.as_dict()

    # -- §7j: NDT registration ---------------------------------------------------------------------------
    @staticmethod
    def _cloud_args(cloud):
        """(pointer, n, stride, fmt) of a host PCL-struct array or of a (device_ptr, n) tuple of 16-byte records"""
        if isinstance(cloud, tuple):
            return C.c_void_p(cloud[0]), int(cloud[1]), 16, FMT_DEVICE, None
        cloud = np.ascontiguousarray(cloud)
        return _vp(cloud), len(cloud), cloud.dtype.itemsize, _fmt_of(cloud), cloud

    def ndt_set_target(self, slot: int, cloud, params: "NdtParams") -> dict:
        """setInputTarget + setResolution; cloud = host PCL-struct array or (device_ptr, n)"""
        ptr, n, stride, fmt, _keep = self._cloud_args(cloud)
        info = NdtInfo()
        self._chk(self._L.lisreg_ndt_set_target(self._h, slot, ptr, n, stride, fmt, C.byref(params), C.byref(info)))
        return dict(dims=list(info.dims), n_voxels=info.n_voxels, n_valid=info.n_valid)

    def _align(self, fn, result_type, slot, source, params, guess, want_aligned, out_ptr) -> dict:
        """one alignment of a verifier through `fn`; returns the result dict (+ 'aligned')."""
        ptr, n, stride, fmt, keep = self._cloud_args(source)
        res = result_type()
        g = None if guess is None else np.ascontiguousarray(guess, np.float32).ravel().ctypes.data_as(C.POINTER(C.c_float))
        out = np.zeros_like(keep) if (want_aligned and keep is not None) else None
        o = C.c_void_p(out_ptr) if out_ptr else (_vp(out) if out is not None else None)
        self._chk(fn(self._h, slot, ptr, n, stride, fmt, C.byref(params), g, C.byref(res), o))
        d = res.as_dict()
        if out is not None:
            d["aligned"] = out
        return d

    def _get_voxels(self, fn, slot: int, last_key: str) -> dict:
        """the voxels `fn` reports for a slot: cell_ids, counts, means [m, 3] and the [m, 6] array named last_key"""
        m = C.c_int(0)
        self._chk(fn(self._h, slot, None, None, None, None, 0, C.byref(m)))
        cap = max(m.value, 1)
        ids, cnt = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        means, sym = np.zeros((cap, 3)), np.zeros((cap, 6))
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        self._chk(fn(self._h, slot, ids.ctypes.data_as(ip), cnt.ctypes.data_as(ip), means.ctypes.data_as(dp), sym.ctypes.data_as(dp), cap,
                     C.byref(m)))
        k = m.value
        return {"cell_ids": ids[:k], "counts": cnt[:k], "means": means[:k], last_key: sym[:k]}

    def _sums_at(self, fn, slot, source, params, poses, with_hessian):
        """one evaluation through `fn` at `poses` (float64 arrays, None: a NULL pointer): (out [28]; pairs)"""
        ptr, n, stride, fmt, _keep = self._cloud_args(source)
        dp = C.POINTER(C.c_double)
        poses = [None if a is None else np.ascontiguousarray(a, np.float64).ravel() for a in poses]
        out = np.zeros(28)
        pairs = C.c_longlong(0)
        self._chk(fn(self._h, slot, ptr, n, stride, fmt, C.byref(params), *[None if a is None else a.ctypes.data_as(dp) for a in poses],
                     1 if with_hessian else 0, out.ctypes.data_as(dp), C.byref(pairs)))
        return out, pairs.value

    def ndt_align(self, slot: int, source, params: "NdtParams", guess=None, want_aligned: bool = False, out_ptr: int = 0) -> dict:
        """pcl::NormalDistributionsTransform::align against the NDT target in `slot`; returns the result dict (+ 'aligned')."""
        return self._align(self._L.lisreg_ndt_align, NdtResult, slot, source, params, guess, want_aligned, out_ptr)

    def ndt_get_voxels(self, slot: int) -> dict:
        """the valid voxels of an NDT target in ascending cell order: cell_ids, counts, means [m, 3], icov6 [m, 6]"""
        return self._get_voxels(self._L.lisreg_ndt_get_voxels, slot, "icov6")

    def ndt_derivatives(self, slot: int, source, params: "NdtParams", p, with_hessian: bool = True):
        """one evaluation at p = (tx, ty, tz, a, b, c): (out [28] = score, gradient, Hessian upper triangle; pairs)"""
        return self._sums_at(self._L.lisreg_ndt_derivatives, slot, source, params, [p], with_hessian)

    def ndt_set_target_batch(self, jobs, params: "NdtParams"):
        """lisreg_ndt_set_target_batch (§7v): jobs = a list of (slot, (device_ptr, n)).  Returns a list of dicts, one per job: status,
        dims, n_voxels, n_valid (a failed job: status = ERR_ARG; last_error() names the first)."""
        arr = (NdtTargetJob * max(len(jobs), 1))()
        for k, job in enumerate(jobs):
            arr[k].slot, arr[k].cloud, arr[k].n = int(job[0]), job[1][0], int(job[1][1])
        self._chk(self._L.lisreg_ndt_set_target_batch(self._h, len(jobs), arr, C.byref(params)))
        return [dict(status=arr[k].status, dims=list(arr[k].info.dims), n_voxels=arr[k].info.n_voxels, n_valid=arr[k].info.n_valid)
                for k in range(len(jobs))]

    def ndt_target_batch_counts(self):
        """(enqueues, synchronisations) of the last ndt_set_target_batch of this context"""
        e, s = C.c_int(0), C.c_int(0)
        self._chk(self._L.lisreg_ndt_target_batch_counts(self._h, C.byref(e), C.byref(s)))
        return e.value, s.value

    def ndt_get_target(self, slot: int) -> dict:
        """lisreg_ndt_get_target: the slot as it stands — dims, n_voxels (occupied), n_valid, n_points, n_records, min_b [3], resolution,
        geom [11] (the search grid's origin, cell, 1 / cell, the bounding box), grid_dims [3], sorted [m, 4] float32 (the fourth word =
        index among the finite points, as bits), cell_start [grid cells + 1], table [voxel cells], and of every voxel record, valid or
        not: record_cells, record_flags, records [n_records, 10]"""
        info = NdtInfo()
        dims, min_b, res = (C.c_int * 3)(), (C.c_int * 3)(), C.c_double(0)
        geom = np.zeros(11, np.float32)
        gp = geom.ctypes.data_as(C.POINTER(C.c_float))
        gd = (C.c_int * 3)()
        m_, nv_ = C.c_int(0), C.c_int(0)
        self._chk(self._L.lisreg_ndt_get_target(self._h, slot, C.byref(info), dims, min_b, C.byref(res), gp, gd, C.byref(m_), C.byref(nv_),
                                                None, None, None, None, None, None, 0, 0, 0, 0))
        m, nv, cells, n_table = m_.value, nv_.value, gd[0] * gd[1] * gd[2], dims[0] * dims[1] * dims[2]
        srt = np.zeros((m, 4), np.float32)
        cs, tab = np.zeros(cells + 1, np.int32), np.zeros(n_table, np.int32)
        rc, rf, rec = np.zeros(nv, np.int32), np.zeros(nv, np.int32), np.zeros((nv, 10))
        ip = C.POINTER(C.c_int)
        self._chk(self._L.lisreg_ndt_get_target(self._h, slot, C.byref(info), dims, min_b, C.byref(res), gp, gd, C.byref(m_), C.byref(nv_),
                                                srt.ctypes.data_as(C.POINTER(C.c_float)), cs.ctypes.data_as(ip), tab.ctypes.data_as(ip),
                                                rc.ctypes.data_as(ip), rf.ctypes.data_as(ip), rec.ctypes.data_as(C.POINTER(C.c_double)),
                                                m, cells + 1, n_table, nv))
        return dict(dims=list(dims), n_voxels=info.n_voxels, n_valid=info.n_valid, n_points=m, n_records=nv, min_b=list(min_b),
                    resolution=res.value, geom=geom, grid_dims=list(gd), sorted=srt, cell_start=cs, table=tab, record_cells=rc,
                    record_flags=rf, records=rec)

    # -- §7k: VGICP registration -------------------------------------------------------------------------
    def vgicp_set_target(self, slot: int, cloud, params: "VgicpParams") -> dict:
        """distributions + voxel statistics of the target; cloud = host PCL-struct array or (device_ptr, n)"""
        ptr, n, stride, fmt, _keep = self._cloud_args(cloud)
        info = VgicpInfo()
        self._chk(self._L.lisreg_vgicp_set_target(self._h, slot, ptr, n, stride, fmt, C.byref(params), C.byref(info)))
        return dict(dims=list(info.dims), n_voxels=info.n_voxels, n_points=info.n_points)

    def vgicp_align(self, slot: int, source, params: "VgicpParams", guess=None, want_aligned: bool = False, out_ptr: int = 0) -> dict:
        """FastVGICP::align against the VGICP target in `slot`; returns the result dict (+ 'aligned')."""
        return self._align(self._L.lisreg_vgicp_align, VgicpResult, slot, source, params, guess, want_aligned, out_ptr)

    def vgicp_covariances(self, cloud, k: int = 20, want_neighbours: bool = True, cell_edge: float = 0.0):
        """(cov6 [n, 6] with NaN rows for NaN points, neighbours [n, k] or None) of every point's distribution"""
        ptr, n, stride, fmt, _keep = self._cloud_args(cloud)
        cov = np.zeros((max(n, 1), 6))
        nbr = np.zeros((max(n, 1), max(k, 1)), np.int32) if want_neighbours else None
        self._chk(self._L.lisreg_vgicp_covariances(self._h, ptr, n, stride, fmt, k, cov.ctypes.data_as(C.POINTER(C.c_double)),
                                                   nbr.ctypes.data_as(C.POINTER(C.c_int)) if want_neighbours else None, cell_edge))
        return cov[:n], (nbr[:n] if want_neighbours else None)

    def vgicp_get_voxels(self, slot: int) -> dict:
        """the voxels of a VGICP target in ascending cell order: cell_ids, counts, means [m, 3], cov6 [m, 6]"""
        return self._get_voxels(self._L.lisreg_vgicp_get_voxels, slot, "cov6")

    def vgicp_linearize(self, slot: int, source, params: "VgicpParams", T, with_hessian: bool = True):
        """one linearisation at T (4x4): (out [28] = error, b, H upper triangle; pairs)"""
        return self._sums_at(self._L.lisreg_vgicp_linearize, slot, source, params, [np.reshape(T, 16)], with_hessian)

    def vgicp_set_target_batch(self, jobs, params: "VgicpParams"):
        """lisreg_vgicp_set_target_batch (§7u): jobs = a list of (slot, (device_ptr, n)).  Returns a list of dicts, one per job: status,
        dims, n_voxels, n_points (a failed job: status = ERR_ARG; last_error() names the first)."""
        arr = (VgicpTargetJob * max(len(jobs), 1))()
        for k, job in enumerate(jobs):
            arr[k].slot, arr[k].cloud, arr[k].n = int(job[0]), job[1][0], int(job[1][1])
        self._chk(self._L.lisreg_vgicp_set_target_batch(self._h, len(jobs), arr, C.byref(params)))
        return [dict(status=arr[k].status, dims=list(arr[k].info.dims), n_voxels=arr[k].info.n_voxels, n_points=arr[k].info.n_points)
                for k in range(len(jobs))]

    def vgicp_target_batch_counts(self):
        """(enqueues, synchronisations) of the last vgicp_set_target_batch of this context"""
        e, s = C.c_int(0), C.c_int(0)
        self._chk(self._L.lisreg_vgicp_target_batch_counts(self._h, C.byref(e), C.byref(s)))
        return e.value, s.value

    def vgicp_get_target(self, slot: int) -> dict:
        """lisreg_vgicp_get_target: the slot as it stands — dims, n_voxels, n_points, min_b [3], resolution, geom [11] (the search grid's
        origin, cell, 1 / cell, the bounding box), grid_dims [3], sorted [m, 4] float32 (the fourth word = index among the finite points, as bits),
        cell_start [grid cells + 1], table [voxel cells]"""
        info = VgicpInfo()
        dims, min_b, res = (C.c_int * 3)(), (C.c_int * 3)(), C.c_double(0)
        geom = np.zeros(11, np.float32)
        gp = geom.ctypes.data_as(C.POINTER(C.c_float))
        gd = (C.c_int * 3)()
        self._chk(self._L.lisreg_vgicp_get_target(self._h, slot, C.byref(info), dims, min_b, C.byref(res), gp, gd, None, None, None, 0, 0, 0))
        m, cells, n_table = info.n_points, gd[0] * gd[1] * gd[2], dims[0] * dims[1] * dims[2]
        srt = np.zeros((m, 4), np.float32)
        cs, tab = np.zeros(cells + 1, np.int32), np.zeros(n_table, np.int32)
        ip = C.POINTER(C.c_int)
        self._chk(self._L.lisreg_vgicp_get_target(self._h, slot, C.byref(info), dims, min_b, C.byref(res), gp, gd,
                                                  srt.ctypes.data_as(C.POINTER(C.c_float)), cs.ctypes.data_as(ip), tab.ctypes.data_as(ip),
                                                  m, cells + 1, n_table))
        return dict(dims=list(dims), n_voxels=info.n_voxels, n_points=m, min_b=list(min_b), resolution=res.value, geom=geom,
                    grid_dims=list(gd), sorted=srt, cell_start=cs, table=tab)

    # -- §7l: FastGICP registration ----------------------------------------------------------------------
    def fgicp_set_target(self, slot: int, cloud, params: "FgicpParams", cell_edge: float = 0.0) -> dict:
        """distributions + search grid of the target; cloud = host PCL-struct array or (device_ptr, n)"""
        ptr, n, stride, fmt, _keep = self._cloud_args(cloud)
        info = FgicpInfo()
        self._chk(self._L.lisreg_fgicp_set_target(self._h, slot, ptr, n, stride, fmt, C.byref(params), C.byref(info), cell_edge))
        return dict(grid_dims=list(info.grid_dims), n_points=info.n_points)

    def fgicp_set_target_batch(self, jobs, params: "FgicpParams"):
        """lisreg_fgicp_set_target_batch (§7t): jobs = a list of (slot, (device_ptr, n)) or (slot, (device_ptr, n), cell_edge).  Returns
        a list of dicts, one per job: status, grid_dims, n_points (a failed job: status = ERR_ARG; last_error() names the first)."""
        arr = (FgicpTargetJob * max(len(jobs), 1))()
        for k, job in enumerate(jobs):
            arr[k].slot, arr[k].cloud, arr[k].n = int(job[0]), job[1][0], int(job[1][1])
            arr[k].cell_edge = float(job[2]) if len(job) > 2 else 0.0
        self._chk(self._L.lisreg_fgicp_set_target_batch(self._h, len(jobs), arr, C.byref(params)))
        return [dict(status=arr[k].status, grid_dims=list(arr[k].info.grid_dims), n_points=arr[k].info.n_points) for k in range(len(jobs))]

    def fgicp_target_batch_counts(self):
        """(enqueues, synchronisations) of the last fgicp_set_target_batch of this context"""
        e, s = C.c_int(0), C.c_int(0)
        self._chk(self._L.lisreg_fgicp_target_batch_counts(self._h, C.byref(e), C.byref(s)))
        return e.value, s.value

    def fgicp_get_target(self, slot: int) -> dict:
        """lisreg_fgicp_get_target: the slot as it stands — grid_dims, n_points, geom [11] (origin, cell, 1 / cell, bounding box),
        sorted [m, 4] float32 (the fourth word = index among the finite points, as bits), cell_start [cells + 1], orig [m], cov6 [m, 6]"""
        info = FgicpInfo()
        geom = np.zeros(11, np.float32)
        gp = geom.ctypes.data_as(C.POINTER(C.c_float))
        self._chk(self._L.lisreg_fgicp_get_target(self._h, slot, C.byref(info), gp, None, None, None, None, 0, 0))
        m, cells = info.n_points, info.grid_dims[0] * info.grid_dims[1] * info.grid_dims[2]
        srt = np.zeros((m, 4), np.float32)
        cs, orig, cov = np.zeros(cells + 1, np.int32), np.zeros(m, np.int32), np.zeros((m, 6))
        ip = C.POINTER(C.c_int)
        self._chk(self._L.lisreg_fgicp_get_target(self._h, slot, C.byref(info), gp, srt.ctypes.data_as(C.POINTER(C.c_float)),
                                                  cs.ctypes.data_as(ip), orig.ctypes.data_as(ip), cov.ctypes.data_as(C.POINTER(C.c_double)),
                                                  m, cells + 1))
        return dict(grid_dims=list(info.grid_dims), n_points=m, geom=geom, sorted=srt, cell_start=cs, orig=orig, cov6=cov)

    def fgicp_align(self, slot: int, source, params: "FgicpParams", guess=None, want_aligned: bool = False, out_ptr: int = 0) -> dict:
        """FastGICP::align against the FastGICP target in `slot`; returns the result dict (+ 'aligned')."""
        return self._align(self._L.lisreg_fgicp_align, FgicpResult, slot, source, params, guess, want_aligned, out_ptr)

    def fgicp_correspondences(self, slot: int, source, params: "FgicpParams", T, want_sqdist: bool = True):
        """the search at T (4x4): (index [n] in the caller's target cloud, -1 none; squared distance [n], NaN where -1, or None)"""
        ptr, n, stride, fmt, _keep = self._cloud_args(source)
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        idx = np.zeros(max(n, 1), np.int32)
        sq = np.zeros(max(n, 1)) if want_sqdist else None
        dp = C.POINTER(C.c_double)
        self._chk(self._L.lisreg_fgicp_correspondences(self._h, slot, ptr, n, stride, fmt, C.byref(params), T.ctypes.data_as(dp),
                                                       idx.ctypes.data_as(C.POINTER(C.c_int)), sq.ctypes.data_as(dp) if want_sqdist else None))
        return idx[:n], (sq[:n] if want_sqdist else None)

    def fgicp_linearize(self, slot: int, source, params: "FgicpParams", T_pairs, with_hessian: bool = True, T_eval=None):
        """pairs and M from a search at T_pairs, the sums at T_eval (None: T_pairs): (out [28] = error, b, H upper triangle; pairs)"""
        return self._sums_at(self._L.lisreg_fgicp_linearize, slot, source, params,
                             [np.reshape(T_pairs, 16), None if T_eval is None else np.reshape(T_eval, 16)], with_hessian)

    # -- §7q: PCL's GICP registration (the target is a FastGICP slot) ------------------------------------------
    def gicp_align(self, slot: int, source, params: "GicpParams", guess=None, want_aligned: bool = False, out_ptr: int = 0) -> dict:
        """pcl::GeneralizedIterativeClosestPoint::align against the FastGICP target in `slot`; returns the result dict (+ 'aligned')."""
        return self._align(self._L.lisreg_gicp_align, GicpResult, slot, source, params, guess, want_aligned, out_ptr)

    def gicp_moments(self, slot: int, source, params: "GicpParams", T):
        """one round at T (4x4): the 74 moments of the pairs found at T (c0, g [12], S [60], pairs)"""
        ptr, n, stride, fmt, _keep = self._cloud_args(source)
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        out = np.zeros(74)
        dp = C.POINTER(C.c_double)
        self._chk(self._L.lisreg_gicp_moments(self._h, slot, ptr, n, stride, fmt, C.byref(params), T.ctypes.data_as(dp), out.ctypes.data_as(dp)))
        return out

    def _gicp_align_batch(self, fn, item_type, result_type, info_type, who, sources, items, params, want_fitness):
        """one batch call of a verifier through `fn`; returns (results: a list of the single call's dicts, fitness [n_items] or None,
        info dict).  A source given as None goes down as a NULL pointer of no points (for a source no item names)."""
        args = [(None, 0, None, None, None) if s is None else self._cloud_args(s) for s in sources]
        layouts = {(a[2], a[3]) for a in args if a[2] is not None}
        if len(layouts) > 1:
            raise ValueError(who + ": the sources of one call share one layout")
        stride, fmt = layouts.pop() if layouts else (16, FMT_DEVICE)
        ptrs = (C.c_void_p * max(len(args), 1))(*[a[0] for a in args])
        ns = (C.c_int * max(len(args), 1))(*[a[1] for a in args])
        its = (item_type * max(len(items), 1))()
        for k, it in enumerate(items):
            its[k].source, its[k].slot = it.source, it.slot
            its[k].guess = None if it.guess is None else it.guess.ctypes.data_as(C.POINTER(C.c_float))
        res = (result_type * max(len(items), 1))()
        fit = np.zeros(max(len(items), 1)) if want_fitness else None
        info = info_type()
        self._chk(fn(self._h, ptrs, ns, len(args), stride, fmt, its, len(items), C.byref(params), res,
                     fit.ctypes.data_as(C.POINTER(C.c_double)) if want_fitness else None, C.byref(info)))
        return ([res[k].as_dict() for k in range(len(items))], fit[:len(items)] if want_fitness else None,
                dict(best=info.best, n_rounds=info.n_rounds, n_sources_staged=info.n_sources_staged))

    def fgicp_align_batch(self, sources, items, params: "FgicpParams", want_fitness: bool = True):
        """lisreg_fgicp_align_batch: sources = a list of clouds (all host PCL-struct arrays of one dtype, or all (device_ptr, n)),
        items = a list of FgicpItem.  Returns (results: a list of fgicp_align's dicts, fitness [n_items] or None, info dict)."""
        return self._gicp_align_batch(self._L.lisreg_fgicp_align_batch, FgicpItemC, FgicpResult, FgicpBatchInfo, "fgicp_align_batch",
                                      sources, items, params, want_fitness)

    def vgicp_align_batch(self, sources, items, params: "VgicpParams", want_fitness: bool = True):
        """lisreg_vgicp_align_batch: sources = a list of clouds (all host PCL-struct arrays of one dtype, or all (device_ptr, n)),
        items = a list of VgicpItem.  Returns (results: a list of vgicp_align's dicts, fitness [n_items] or None, info dict)."""
        return self._gicp_align_batch(self._L.lisreg_vgicp_align_batch, VgicpItemC, VgicpResult, VgicpBatchInfo, "vgicp_align_batch",
                                      sources, items, params, want_fitness)

    def ndt_align_batch(self, sources, items, params: "NdtParams", want_fitness: bool = True):
        """lisreg_ndt_align_batch (§7o): sources = a list of clouds (all host PCL-struct arrays of one dtype, or all (device_ptr, n); None
        for a source no item names), items = a list of NdtItem.  Returns (results: a list of ndt_align's dicts, fitness [n_items] or
        None, info dict)."""
        return self._gicp_align_batch(self._L.lisreg_ndt_align_batch, NdtItemC, NdtResult, NdtBatchInfo, "ndt_align_batch",
                                      sources, items, params, want_fitness)

    def gicp_align_batch(self, sources, items, params: "GicpParams", want_fitness: bool = True):
        """lisreg_gicp_align_batch (§7r): sources = a list of clouds (all host PCL-struct arrays of one dtype, or all (device_ptr, n); None
        for a source no item names), items = a list of GicpItem naming FastGICP slots.  Returns (results: a list of gicp_align's dicts,
        fitness [n_items] or None, info dict)."""
        return self._gicp_align_batch(self._L.lisreg_gicp_align_batch, GicpItemC, GicpResult, GicpBatchInfo, "gicp_align_batch",
                                      sources, items, params, want_fitness)

    def set_profiling(self, on: bool):
        self._chk(self._L.lisreg_set_profiling(self._h, 1 if on else 0))

    def timing(self) -> dict:
        out = (C.c_double * 5)()
        self._chk(self._L.lisreg_get_timing(self._h, out))
        return dict(assoc_ms=out[0], assoc_launches=int(out[1]), solve_ms=out[2], solve_launches=int(out[3]),
                    index_ms=out[4])


def pack_device_records(cloud: np.ndarray) -> np.ndarray:
    """PCL struct array -> contiguous [n,4] float32 view of lisreg_dpoint records (payload = label bits)."""
    n = len(cloud)
    out = np.zeros((n, 4), np.float32)
    out[:, 0], out[:, 1], out[:, 2] = cloud["x"], cloud["y"], cloud["z"]
    if cloud.dtype.names and "label" in cloud.dtype.names:
        out[:, 3] = cloud["label"].astype(np.uint32).view(np.float32)
    return out


_HIP = None


def hip_runtime():
    """The HIP runtime liblisreg.so is bound to — the copy ALREADY in the process (soname libamdhip64.so.7: the system's, or the one a
    PyTorch wheel brought along if torch was imported first), never a second one opened by file name."""
    global _HIP
    if _HIP is None:
        lib()
        for name in ("libamdhip64.so.7", "libamdhip64.so"):
            try:
                _HIP = C.CDLL(name, mode=os.RTLD_NOW | os.RTLD_NOLOAD)
                break
            except OSError:
                continue
        if _HIP is None:
            _HIP = C.CDLL("libamdhip64.so")
    return _HIP


class PinnedArray:
    """Page-locked host memory (hipHostMalloc through the library's own HIP runtime) viewed as a numpy array: what a caller's pinned
    clouds look like to the feeder's copy engine (lisreg_stage_host_items), without torch in the process."""

    def __init__(self, host: np.ndarray):
        self._hip = hip_runtime()
        host = np.ascontiguousarray(host)
        p = C.c_void_p()
        if self._hip.hipHostMalloc(C.byref(p), C.c_size_t(max(host.nbytes, 64)), C.c_uint(0)) != 0:
            raise MemoryError("hipHostMalloc failed")
        self.ptr = p.value
        self.nbytes = host.nbytes
        self.array = np.frombuffer((C.c_ubyte * max(host.nbytes, 1)).from_address(self.ptr), dtype=np.uint8, count=host.nbytes)
        self.array[:] = host.view(np.uint8).reshape(-1)

    def free(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._hip.hipHostFree(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceArray:
    """Minimal device buffer through the SAME HIP runtime liblisreg.so uses (hipMalloc/hipMemcpy via ctypes), for
    callers that hand device-resident clouds to the library without torch."""

    def __init__(self, host: np.ndarray):
        self._hip = hip_runtime()
        host = np.ascontiguousarray(host)
        self.nbytes = host.nbytes
        self.shape = host.shape
        p = C.c_void_p()
        if self._hip.hipMalloc(C.byref(p), C.c_size_t(max(self.nbytes, 16))) != 0:
            raise MemoryError("hipMalloc failed")
        self.ptr = p.value
        if self.nbytes and self._hip.hipMemcpy(C.c_void_p(self.ptr), host.ctypes.data_as(C.c_void_p),
                                               C.c_size_t(self.nbytes), 1) != 0:
            raise RuntimeError("hipMemcpy H2D failed")

    def upload(self, host: np.ndarray, offset_bytes: int = 0):
        """H2D into this buffer (it must be large enough)."""
        host = np.ascontiguousarray(host)
        assert offset_bytes + host.nbytes <= max(self.nbytes, 16)
        if host.nbytes and self._hip.hipMemcpy(C.c_void_p(self.ptr + offset_bytes), host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) != 0:
            raise RuntimeError("hipMemcpy H2D failed")

    def copy_from_device(self, src_ptr: int, nbytes: int, offset_bytes: int = 0):
        assert offset_bytes + nbytes <= max(self.nbytes, 16)
        if nbytes and self._hip.hipMemcpy(C.c_void_p(self.ptr + offset_bytes), C.c_void_p(src_ptr), C.c_size_t(nbytes), 3) != 0:
            raise RuntimeError("hipMemcpy D2D failed")

    def download(self, n_rows: int) -> np.ndarray:
        out = np.zeros((n_rows,) + tuple(self.shape[1:]), np.float32)
        if out.nbytes and self._hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), C.c_size_t(out.nbytes), 2) != 0:
            raise RuntimeError("hipMemcpy D2H failed")
        return out

    def free(self):
        if getattr(self, "ptr", None):
            self._hip.hipFree(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def comm_unique_id() -> bytes:
    buf = (C.c_ubyte * 128)()
    rc = lib().lisreg_comm_unique_id(buf)
    if rc:
        raise LisregError(rc, lib().lisreg_last_error(None).decode())
    return bytes(buf)


def _ctx_comm_init(self, rank: int, nranks: int, uid: bytes):
    buf = (C.c_ubyte * 128).from_buffer_copy(uid)
    self._chk(self._L.lisreg_comm_init(self._h, rank, nranks, buf))


def _ctx_gather_results(self, local_ptr: int, n_local: int, out_ptr: int):
    self._chk(self._L.lisreg_gather_results(self._h, C.c_void_p(local_ptr), n_local, C.c_void_p(out_ptr)))


def _ctx_comm_destroy(self):
    self._L.lisreg_comm_destroy(self._h)


def device_count() -> int:
    return int(lib().lisreg_device_count())


Context.comm_init = _ctx_comm_init
Context.gather_results = _ctx_gather_results
Context.comm_destroy = _ctx_comm_destroy


def device_to_host(ptr: int, shape, dtype=np.float32) -> np.ndarray:
    """Blocking D2H copy through the library's HIP runtime (tests only)."""
    out = np.zeros(shape, dtype)
    hip = hip_runtime()
    hip.hipDeviceSynchronize()
    if hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) != 0:
        raise RuntimeError("hipMemcpy D2H failed")
    return out


def default_pretreat_params(n_scan: int | None = None) -> PretreatParams:
    p = PretreatParams()
    rc = lib().lisreg_default_pretreat_params(C.byref(p))
    if rc:
        raise LisregError(rc, "lisreg_default_pretreat_params")
    if n_scan is not None:
        p.n_scan = n_scan
    return p


def default_rangenet_params(img_h: int | None = None, img_w: int | None = None) -> RangenetParams:
    """lisreg_default_rangenet_params: 64 x 2048, fov 3 / -25 degrees, means 0, stds 1 (the real ones are the model's), 20 classes"""
    p = RangenetParams()
    rc = lib().lisreg_default_rangenet_params(C.byref(p))
    if rc != OK:
        raise LisregError(rc, "lisreg_default_rangenet_params")
    if img_h is not None:
        p.img_h = img_h
    if img_w is not None:
        p.img_w = img_w
    return p


def default_rangenet_knn_params() -> RangenetKnnParams:
    """lisreg_default_rangenet_knn_params: knn 5, search 5, sigma 1, cutoff 1 (the model's own are the `post: KNN: params:` block of its
    arch_cfg.yaml), no_vote_label 0"""
    p = RangenetKnnParams()
    rc = lib().lisreg_default_rangenet_knn_params(C.byref(p))
    if rc != OK:
        raise LisregError(rc, "lisreg_default_rangenet_knn_params")
    return p


def rangenet_knn_weights(knn_params: RangenetKnnParams) -> np.ndarray:
    """lisreg_rangenet_knn_weights: the search * search float32 window weights (host only, no device needed)"""
    if knn_params.search not in (1, 3, 5, 7) or not (0.0 < knn_params.sigma < float("inf")):
        raise LisregError(ERR_ARG, "rangenet_knn_weights: search must be 1, 3, 5 or 7 and sigma finite and > 0")
    out = np.zeros(knn_params.search ** 2, np.float32)
    lib().lisreg_rangenet_knn_weights(C.byref(knn_params), out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def default_feature_params() -> FeatureParams:
    p = FeatureParams()
    rc = lib().lisreg_default_feature_params(C.byref(p))
    if rc:
        raise LisregError(rc, "lisreg_default_feature_params")
    return p
