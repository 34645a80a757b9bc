"""ctypes binding of libmfhip.so (include/mfhip.h).

The HIP library is THE implementation of the voxel / refinement ops: there is no
Python or CPU fallback.  If the shared object is missing (or a tensor is not on a
HIP device) the ops raise -- loudly -- instead of computing something else.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MF_LIBMFHIP=<file name in this directory>: a differently built copy of the same library (tools/stamps_*.py use
# libmfhip_dbg.so = `make ICC_DEBUG=1 OUT=../libmfhip_dbg.so OBJDIR=_obj_dbg`: per-phase time stamps in the ICC kernels)
SO_PATH = os.path.join(_HERE, os.path.basename(os.environ.get("MF_LIBMFHIP", "libmfhip.so")))
_lib = None

_p = ctypes.c_void_p
_i = ctypes.c_int32  # C int and int32_t: the same type on every ABI this library is built for
_i64 = ctypes.c_int64
_f = ctypes.c_float
_d = ctypes.c_double


class IccBatch(ctypes.Structure):
    """mfIccBatch (include/mfhip.h)."""

    _fields_ = [
        ("pts4", _p), ("obj_off", _p), ("scene_off", _p), ("obj_scene", _p),
        ("pitch", _p), ("origin", _p), ("grid_target", _p), ("grid_ne", _p),
        ("n_objects", _i), ("n_scenes", _i), ("n_points", _i), ("dim", _i), ("max_scene_objects", _i),
        ("voxel_threshold", _f), ("sdf_offset", _f), ("grid_ne_binary", _i), ("flags", _i),
    ]


class OccTree(ctypes.Structure):
    """mfOccTree (include/mfhip.h)."""

    _fields_ = [
        ("logodds", _p), ("bits", _p), ("lo", _i * 3), ("dim", _i * 3),
        ("resolution", _d), ("res_factor", _d),
    ]


class IcpRegBatch(ctypes.Structure):
    """mfIcpRegBatch (include/mfhip.h)."""

    _fields_ = [(n, _p) for n in (
        "src", "src_off", "src_cnt", "tgt", "tgt_off", "tgt_cnt", "grid_off", "grid_dim", "grid_origin", "grid_start",
        "grid_idx", "transform_init", "active", "cur", "corr", "transform", "transformation", "fitness", "inlier_rmse",
        "n_iter", "hist_transform", "hist_fitness", "hist_rmse")] + [
        ("max_corr_dist", _d), ("cell", _d), ("n_objects", _i), ("max_iter", _i), ("mode", _i), ("reserved", _i)]


class MeshSdfBatch(ctypes.Structure):
    """mfMeshSdfBatch (include/mfhip.h)."""

    _fields_ = [(n, _p) for n in (
        "vertices", "v_off", "faces", "f_off", "face_rec", "points", "q_off", "blk_off", "grid_origin", "grid_h",
        "dist", "face", "winding", "sdf", "occupancy")] + [
        ("n_meshes", _i), ("n_blocks", _i), ("grid_dim", _i), ("reserved", _i)]


class RenderBatch(ctypes.Structure):
    """mfRenderBatch (include/mfhip.h)."""

    _fields_ = [(n, _p) for n in (
        "vertices", "v_off", "faces", "f_off", "item_mesh", "item_T", "item_target", "item_id", "item_rec_off",
        "workspace", "depth", "instance", "face", "count")] + [
        (n, _d) for n in ("fx", "fy", "cx", "cy", "near")] + [
        (n, _i) for n in ("n_meshes", "n_items", "n_targets", "height", "width", "reserved")]


class OccRegBatch(ctypes.Structure):
    """mfOccRegBatch (include/mfhip.h)."""

    _fields_ = [(n, _p) for n in (
        "points", "pts_off", "pitch", "origin", "dims", "threshold", "grid_occ", "grid_unocc", "grid_off", "active",
        "host_pts_off", "host_pitch", "host_dims", "host_threshold")] + [
        (n, _i) for n in ("n_objects", "n_points_total", "max_voxels", "reserved")]


_SIGNATURES = {
    "mf_version": ([], _i),
    "mf_last_error_string": ([], ctypes.c_char_p),
    "mf_average_voxelization_3d_fwd": ([_p, _p, _p, _i64, _i, _i, _i, _i, _i, _f, _f, _f, _f, _p, _p, _p, _p, _p, _p], _i),
    "mf_average_voxelization_3d_bwd": ([_p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _f, _f, _f, _f, _p, _p], _i),
    "mf_max_voxelization_3d_fwd": ([_p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _f, _f, _f, _f, _p, _p, _p, _p, _p], _i),
    "mf_max_voxelization_3d_bwd": ([_p, _p, _i64, _i, _i, _i, _i, _i, _p, _p], _i),
    "mf_interpolate_voxel_grid_fwd": ([_p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _p, _i, _p], _i),
    "mf_interpolate_voxel_grid_bwd": ([_p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _p, _i, _p], _i),
    "mf_occupancy_grid_3d_fwd": ([_p, _i64, _f, _f, _f, _f, _i, _i, _i, _f, _p, _p, _p], _i),
    "mf_occupancy_grid_3d_bwd": ([_p, _p, _i64, _f, _f, _f, _f, _i, _i, _i, _f, _p, _p, _p], _i),
    "mf_truncated_distance_function_fwd": ([_p, _i64, _f, _f, _f, _f, _i, _i, _i, _f, _p, _p, _p], _i),
    "mf_truncated_distance_function_bwd": ([_p, _p, _p, _i64, _f, _f, _f, _f, _i, _i, _i, _f, _p, _p], _i),
    "mf_pseudo_occupancy_weights": ([_p, _p, _p, _i, _i, _i, _i, _f, _f, _p, _p, _p, _p, _p], _i),
    "mf_nn": ([_p, _i64, _p, _i64, _p, _p, _p], _i),
    "mf_icp_loss_grad": ([_p, _i64, _p, _i64, _p, _f, _p, _p], _i),
    "mf_icp_refine": ([_p, _p, _p, _p, _i, _i, _f, _p, _p, _p, _p, _i, _i, _f, _f, _p, _p, _p], _i),
    "mf_icc_workspace_bytes": ([ctypes.POINTER(IccBatch)], _i64),
    "mf_icc_iteration_launches": ([ctypes.POINTER(IccBatch)], _i),
    "mf_icc_plan": ([ctypes.POINTER(IccBatch), _p, _i], _i),
    "mf_icc_launch_stage": ([ctypes.POINTER(IccBatch), _p, _p, _p, _i, _p], _i),
    "mf_icc_prepare": ([ctypes.POINTER(IccBatch), _p, _p], _i),
    "mf_icc_loss_grad": ([ctypes.POINTER(IccBatch), _p, _p, _p, _p, _p, _p, _p], _i),
    "mf_icc_refine": ([ctypes.POINTER(IccBatch), _p, _p, _p, _p, _i, _i, _f, _f, _p, _p, _p, _p], _i),
    "mf_icc_observer_bytes": ([_i, _i], _i64),
    "mf_icc_refine_converge": ([ctypes.POINTER(IccBatch), _p, _p, _p, _p, _i, _i, _f, _f, _d, _i, _i, _p, _p, _p, _p, _p,
                                _p], _i),
    "mf_icc_debug_stamps": ([_p, _i], _i),
    "mf_sparse_conv3d_workspace_bytes": ([_i] * 5 + [_i64], _i64),
    "mf_sparse_conv3d_k4s2_points_fwd": ([_p, _p, _p, _i64, _f, _f, _f, _f, _p, _p, _p, _p, _p] + [_i] * 6 + [_p], _i),
    "mf_sparse_conv3d_pack_weights": ([_p, _i, _i, _i, _i, _p, _p], _i),
    "mf_sparse_conv3d_k4s2_fwd": ([_p, _p, _p, _p, _p, _p, _p] + [_i] * 6 + [_p], _i),
    "mf_pack_points_sdf": ([_p, _p, _i64, _p, _p], _i),
    "mf_average_distance_fwd": ([_p, _p, _p, _p, _i, _i, _i, _p, _p, _p], _i),
    "mf_average_distance_bwd": ([_p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p], _i),
    "mf_conv3d_k4s2_pack_weights": ([_p, _i, _i, _i, _i, _p, _p], _i),
    "mf_conv3d_k4s2_default_split": ([_i] * 4, _i),
    "mf_conv3d_k4s2_workspace_bytes": ([_i] * 4, _i64),
    "mf_conv3d_k4s2_fwd": ([_p, _p, _p, _p, _p, _p] + [_i] * 6 + [_p], _i),
    "mf_to_channels_last": ([_p, _p, _i, _i, _i64, _p], _i),
    "mf_sparse_conv3d_k4s2_points_cl_fwd": ([_p, _i64, _p, _p, _i64, _f, _f, _f, _f, _p, _p, _p, _p, _p] + [_i] * 6 + [_p], _i),
    "mf_interpolate_voxel_grid_cl_fwd": ([_p, _p, _p, _i64, _i, _i, _i, _i, _i, _p, _i64, _p], _i),
    "mf_occupancy_convs_fwd": ([_p] * 7 + [_i] * 2 + [_p], _i),
    "mf_occupancy_convs_split_fwd": ([_p] * 8 + [_i] * 2 + [_p], _i),
    "mf_linear_fwd": ([_p, _i64, _i, _p, _i64, _i, _p, _i64, _p, _i64] + [_i] * 7 + [_p], _i),
    "mf_cast_rows_bf16": ([_p, _i64, _p, _i64, _i64, _i, _p], _i),
    "mf_relu_mask_bf16": ([_p, _p, _p, _p, _i64, _p], _i),
    "mf_linear_bf16": ([_p, _i64, _i, _p, _i64, _i, _p, _i64, _p, _i64] + [_i] * 8 + [_p], _i),
    "mf_linear_wgrad_bf16": ([_p, _i64, _i, _p, _i64, _i, _p, _i64, _i, _p] + [_i] * 5 + [_p], _i),
    "mf_conv3d_k4s2_pack_bf16": ([_p] + [_i] * 4 + [_p, _p, _p], _i),
    "mf_conv3d_k4s2_bf16_fwd": ([_p, _p, _p, _p] + [_i] * 6 + [_p], _i),
    "mf_conv3d_k4s2_bf16_dgrad": ([_p, _p, _p] + [_i] * 6 + [_p], _i),
    "mf_conv3d_k4s2_bf16_wgrad_workspace_bytes": ([_i] * 3, _i64),
    "mf_conv3d_k4s2_bf16_wgrad_default_split": ([_i] * 4, _i),
    "mf_conv3d_k4s2_bf16_wgrad": ([_p, _p, _p, _p] + [_i] * 7 + [_p], _i),
    "mf_conv3d_bf16_pack": ([_p] + [_i] * 5 + [_p, _p, _p, _p], _i),
    "mf_conv3d_bf16_fwd": ([_p, _p, _p, _p] + [_i] * 11 + [_p], _i),
    "mf_conv3d_bf16_fwd_workspace_bytes": ([_i] * 8, _i64),
    "mf_conv3d_bf16_fwd_ws": ([_p, _p, _p, _p, _p, _i64] + [_i] * 11 + [_p], _i),
    "mf_conv2d_split_pack": ([_p] + [_i] * 3 + [_p, _p], _i),
    "mf_conv2d_split_workspace_bytes": ([_i] * 8, _i64),
    "mf_conv2d_split_fwd": ([_p, _p, _p, _p, _i, _p, _i, _p, _i, _p, _i, _i, _p, _i64] + [_i] * 8 + [_p], _i),
    "mf_conv3d_k4s2_split_pack": ([_p] + [_i] * 4 + [_p, _p], _i),
    "mf_conv3d_k4s2_split_workspace_bytes": ([_i] * 4, _i64),
    "mf_conv3d_k4s2_split_fwd": ([_p, _p, _p, _i, _p, _i, _p, _i, _i, _p, _i64] + [_i] * 4 + [_p], _i),
    "mf_linear_split_pack": ([_p, _i64] + [_i] * 6 + [_p, _p], _i),
    "mf_linear_split_workspace_bytes": ([_i64, _i, _i], _i64),
    "mf_linear_split_fwd": ([_p, _i, _p, _p, _i, _p, _i, _p, _i, _i, _p, _i64] + [_i] * 3 + [_p], _i),
    "mf_sparse_conv3d_k4s2_points_cl_split_fwd": ([_p, _i64, _p, _p, _i64, _f, _f, _f, _f, _p, _p, _p, _p, _p, _p] + [_i] * 6 + [_p], _i),
    "mf_interpolate_voxel_grid_cl_split_fwd": ([_p, _p, _p, _i64, _i, _i, _i, _i, _i, _p, _i64, _i64, _p], _i),
    "mf_conv3d_k3_narrow_bf16_pack_elems": ([_i], _i64),
    "mf_conv3d_k3_narrow_bf16_pack": ([_p] + [_i] * 5 + [_p, _p], _i),
    "mf_conv3d_k3_narrow_bf16": ([_p, _p, _p, _p] + [_i] * 6 + [_p], _i),
    "mf_conv3d_bf16_wgrad_workspace_bytes": ([_i] * 4, _i64),
    "mf_wgrad_split": ([_i64, _i64, _i64], _i),
    "mf_linear_wgrad_bf16_default_split": ([_i64, _i, _i, _i], _i),
    "mf_conv3d_bf16_wgrad_default_split": ([_i] * 5, _i),
    "mf_conv3d_bf16_wgrad": ([_p, _p, _p, _p] + [_i] * 11 + [_p], _i),
    "mf_sparse_conv3_bf16_max_rows": ([_i64], _i64),
    "mf_sparse_conv3_bf16_workspace_bytes": ([_i64, _i, _i], _i64),
    "mf_sparse_conv3_bf16_tables": ([_p, _i64, _i, _i, _p], _i),
    "mf_sparse_conv3_bf16_index": ([_p, _p, _i64, _i, _i, _p, _p], _i),
    "mf_sparse_conv3_bf16_pack": ([_p, _i, _i, _i, _i, _p, _p, _p], _i),
    "mf_sparse_conv3_bf16_unpack_dw": ([_p, _i, _i, _i, _i, _p, _p], _i),
    "mf_sparse_conv3_bf16_reduce": ([_p, _p, _p, _p, _i64, _i, _i, _i, _i, _p, _p], _i),
    "mf_sparse_conv3_bf16_gather_dy": ([_p, _p, _i64, _i, _i, _i, _p, _p], _i),
    "mf_linear_bf16_tiles": ([_p, _i, _p, _i64, _i, _p, _p, _i, _i, _i, _i, _i, _p], _i),
    "mf_linear_wgrad_bf16_ranges": ([_p, _i, _p, _i, _p, _i64, _i, _p, _i, _i, _i, _p], _i),
    "mf_conv3d_k4s2_bf16_pack_cols": ([_p, _i, _i, _i, _i, _p, _p], _i),
    "mf_conv3d_k4s2_bf16_col2im": ([_p, _i, _i, _i, _p, _p], _i),
    "mf_average_voxelization_rows_bf16_fwd": ([_p, _i64, _p, _p, _i64, _i, _i, _i, _p, _p, _p, _p, _p, _i64, _p], _i),
    "mf_average_voxelization_rows_bf16_bwd": ([_p, _i64, _p, _p, _p, _p, _i64, _i, _i, _i, _p, _i64, _p], _i),
    "mf_average_voxelization_cl_bf16_fwd": ([_p, _i64, _p, _p, _i64, _i, _i, _i, _p, _i64, _p, _p, _p, _p], _i),
    "mf_average_voxelization_cl_bf16_bwd": ([_p, _i64, _p, _p, _p, _i64, _i, _i, _i, _p, _i64, _p], _i),
    "mf_interpolate_voxel_grid_cl_bf16_fwd": ([_p, _p, _p, _i64, _i, _i, _i, _i, _i, _p, _i64, _p], _i),
    "mf_interpolate_voxel_grid_cl_bf16_bwd": ([_p, _i64, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _p, _i, _p], _i),
    "mf_upsample_bilinear_cl_fwd": ([_p, _p] + [_i] * 7 + [_p], _i),
    "mf_upsample_bilinear_cl_split_fwd": ([_p, _p] + [_i] * 8 + [_p], _i),
    "mf_upsample2x_tapsum_fwd": ([_p, _p, _p, _i, _p, _i, _p] + [_i] * 6 + [_p], _i),
    "mf_split_bf16": ([_p, _i64, _i64, _i64, _i64] + [_i] * 4 + [_p, _i, _i, _p], _i),
    "mf_maxpool3s2_split_fwd": ([_p, _i64, _i64, _i64, _i64] + [_i] * 4 + [_p, _p, _p], _i),
    "mf_upsample_bilinear_cl_bwd": ([_p, _p] + [_i] * 7 + [_p], _i),
    "mf_upsample_bilinear_cf_fwd": ([_p, _p, _i64] + [_i] * 5 + [_p], _i),
    "mf_upsample_bilinear_cf_bwd": ([_p, _p, _i64] + [_i] * 5 + [_p], _i),
    "mf_prelu_fwd": ([_p, _p, _p, _i64, _i, _p], _i),
    "mf_rgb_normalize": ([_p, _i, _p, _p, _p, _i64, _p], _i),
    "mf_bn_act_fwd": ([_p, _p, _p, _p, _p, _p, _f, _p, _i64, _i, _i64, _i, _i, _i, _p], _i),
    "mf_backbone2d_last_path": ([], _i),
    "mf_prelu_bwd_workspace_floats": ([_i64], _i64),
    "mf_prelu_bwd": ([_p, _p, _p, _p, _p, _p, _i64, _i, _p], _i),
    "mf_gemm_bf16_last_tile": ([], _i),
    "mf_gemm_bf16_nt_plan": ([_i, _i64, _i, _i, _i, _i, _i64, _i, _i, _p, _p], _i),
    "mf_gemm_bf16_tn_plan": ([_i, _i, _i, _i64, _i, _i, _i, _i, _p, _p, _p], _i),
    "mf_psp_tail_rows_bf16_fwd": ([_p, _p, _i, _i, _i, _i, _p, _p], _i),
    "mf_psp_tail_rows_bf16_bwd": ([_p, _p, _i, _i, _i, _i, _p, _p, _p], _i),
    "mf_confidence_loss_fwd": ([_p, _p, _i, _i, _f, _p, _p, _p], _i),
    "mf_confidence_loss_bwd": ([_p, _p, _p, _p, _i, _i, _f, _p, _p, _p], _i),
    "mf_pose_epilogue_train_fwd": ([_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p], _i),
    "mf_pose_epilogue_train_bwd": ([_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p], _i),
    "mf_transformation_matrix_fwd": ([_p, _p, _i64, _p, _p], _i),
    "mf_transformation_matrix_bwd": ([_p, _p, _i64, _p, _p, _p], _i),
    "mf_point_prep": ([_p, _p, _p, _p, _i, _i, _i, _f, _p, _p, _p, _p, _p], _i),
    "mf_pose_epilogue": ([_p, _i64, _i, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p], _i),
    "mf_psp_tail_fwd": ([_p, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p] + [_i] * 4 + [_p, _p], _i),
    "mf_valid_pixel_order": ([_p, _i, _i, _p, _p, _p], _i),
    "mf_instance_stats": ([_p, _p, _i, _i, _p, _i, _p, _p], _i),
    "mf_instance_crops": ([_p, _p, _p, _i, _i, _d, _d, _d, _d, _p, _p, _i, _i, _i, _p, _p, _p, _p], _i),
    "mf_occmap_regrid": ([ctypes.POINTER(OccTree), ctypes.POINTER(OccTree), _p], _i),
    "mf_occmap_bounds": ([_p, _p, _i64, _p, _i, _p, _i, _p, _p], _i),
    "mf_occmap_raycast": ([_p, _p, _i64, _p, _i, _p, _f, _f, _f, _p, _p], _i),
    "mf_occmap_count_hits": ([_p, _i64, _p, _i, _p, _p], _i),
    "mf_occmap_apply": ([_p, _i, _i64, _i, _p], _i),
    "mf_occmap_extract": ([_p, _i, _p, _p, _p] + [_i] * 4 + [_p] * 6, _i),
    "mf_occtrack_workspace_bytes": ([_i] * 3, _i64),
    "mf_occtrack_stats_elems": ([_i, _i], _i64),
    "mf_occtrack_transform": ([_p, _p, _i64, _p, _p], _i),
    "mf_occtrack_render": ([_p, _p, _p, _f, _f, _f, _p, _p, _i, _i, _i, _p, _p, _p, _p], _i),
    "mf_occtrack_overlap": ([_p, _p, _i, _i, _p, _i, _p, _i, _p, _p], _i),
    "mf_occtrack_assign": ([_p, _p] + [_i] * 7 + [_d, _d] + [_p] * 5, _i),
    "mf_occtrack_relabel": ([_p, _p, _i, _i, _p, _i, _p, _i] + [_p] * 5, _i),
    "mf_occtrack_clean": ([_p] + [_i] * 4 + [_p, _p, _p], _i),
    "mf_occtrack_merge": ([_p, _p, _i, _i, _p, _i, _p, _p, _p], _i),
    "mf_occserver_bounds": ([_p, _p, _i, _i, _p, _i, _p, _i, _i, _p, _p], _i),
    "mf_occserver_stats": ([_p, _p, _i, _i, _p, _i, _p, _p], _i),
    "mf_occserver_raycast": ([_p, _p, _i, _i, _p, _i, _p, _i, _f, _f, _f, _p, _p], _i),
    "mf_occserver_apply": ([_p, _i, _i64, _f, _f, _f, _f, _p], _i),
    "mf_occserver_publish": ([_p, _i, _p, _i] + [_p] * 5 + [_d, _i, _i, _i] + [_p] * 5, _i),
    "mf_icpreg_workspace_bytes": ([_i64, _i64, _i64], _i64),
    "mf_icpreg_bounds": ([_p, _p, _i, _d, _p, _p, _p], _i),
    "mf_icpreg_prepare": ([_p, _p, _i, _d, _p, _p, _p, _i64, _p, _p, _i64, _d, _i64] + [_p] * 7, _i),
    "mf_icpreg_run": ([ctypes.POINTER(IcpRegBatch), _p], _i),
    "mf_meshsdf_workspace_bytes": ([_i64], _i64),
    "mf_meshsdf_prepare": ([ctypes.POINTER(MeshSdfBatch), _i64, _p], _i),
    "mf_meshsdf_query": ([ctypes.POINTER(MeshSdfBatch), _p], _i),
    "mf_render_workspace_bytes": ([_i64] * 4, _i64),
    "mf_render_setup": ([_p, _i64, _p], _i),  # (mfRenderBatch by reference: ctypes.byref(RenderBatch))
    "mf_render_raster": ([_p, _i64, _p], _i),
    "mf_render_resolve": ([_p, _i64, _p], _i),
    "mf_full_grids": ([_p] * 5 + [_i, _i64, _i, _p, _p, _p], _i),
    "mf_pick_occlusion": ([_p, _p, _i, _i, _i, _p, _p, _p, _p], _i),
    "mf_pick_normals": ([_p, _p, _i, _i, _i, _p, _p], _i),
    "mf_pick_grasp": ([_p, _p, _p, _p, _i, _i, _i, _d, _d, _d, _d, _p, _p, _p, _p], _i),
    "mf_average_distance_f64_workspace_bytes": ([_i, _i], _i64),
    "mf_average_distance_f64": ([_p] * 5 + [_i] * 4 + [_p] * 4, _i),
    "mf_augment_workspace_bytes": ([_i, _i], _i64),
    "mf_augment_mask": ([_p, _p, _i, _p, _i, _i, _i64] + [_p] * 9, _i),
    "mf_augment_rgb": ([_p, _p, _i, _i, _p, _p, _p], _i),
    "mf_augment_pcd": ([_p, _i, _p, _i, _i, _i64, _p, _p], _i),
    "mf_pcdnet_workspace_offsets": ([_i, _i, _i, _p], _i),
    "mf_pcdnet_workspace_bytes": ([_i, _i, _i], _i64),
    "mf_pcdnet_stem": ([_p] * 8 + [_i] * 3 + [_p, _p, _i, _p, _i, _i, _p], _i),
    "mf_pcdnet_pool": ([_p, _i64, _i, _i, _i, _p, _p], _i),
    "mf_pcdnet_bias_relu_split": ([_p, _i64, _p, _i, _i, _i, _i, _p, _i64, _p], _i),
    "mf_occreg_workspace_bytes": ([_i64, _i64, _i64], _i64),
    "mf_occreg_loss_grad": ([_p] * 8, _i),  # (mfOccRegBatch by reference: ctypes.byref(OccRegBatch))
    "mf_occreg_refine": ([_p] * 5 + [_i, _i, _f, _f] + [_p] * 4, _i),
    "mf_gridmesh_workspace_bytes": ([_i64, _i64], _i64),
    "mf_gridmesh_count": ([_p, _p, _p, _i, _p, _p, _p], _i),
    "mf_gridmesh_emit": ([_p] * 5 + [_i, _p, _p, _i64, _i64, _p, _p, _p], _i),
    "mf_gridmesh_adjacency": ([_p, _p, _i, _i64, _i64, _p, _p, _p], _i),
    "mf_gridmesh_smooth": ([_p, _p, _p, _i64, _d, _d, _i, _p, _p], _i),
    "mf_gridmesh_label": ([_p, _p, _p, _i, _i, _p, _p], _i),
    "mf_occserver_map_grids": ([_p, _i, _p, _p, _p, _i, _i, _p, _p, _p], _i),
    "mf_camtrack_workspace_bytes": ([_i] * 5, _i64),
    "mf_camtrack_prepare": ([_p] + [_i] * 4 + [_d] * 5 + [_p, _p], _i),
    "mf_camtrack_align": ([_p, _p] + [_i] * 4 + [_d] * 4 + [_p, _p, _p, _d, _d, _i] + [_p] * 6, _i),
    "mf_tsdf_integrate": ([_p] + [_i] * 3 + [_d] * 6 + [_p, _i, _i] + [_d] * 4 + [_p, _p, _p], _i),
    "mf_tsdf_raycast": ([_p] + [_i] * 3 + [_d] * 7 + [_i] * 3 + [_d] * 4 + [_p] * 4, _i),
    "mf_tsdfmesh_workspace_bytes": ([_i] * 3, _i64),
    "mf_tsdfmesh_count": ([_p] + [_i] * 3 + [_d, _p, _p, _p], _i),
    "mf_tsdfmesh_emit": ([_p] + [_i] * 3 + [_d] * 5 + [_p, _i64, _i64] + [_p] * 4, _i),
    "mf_tsdf_integrate_labels": ([_p, _p] + [_i] * 3 + [_d] * 6 + [_p, _i, _i] + [_d] * 4 + [_p, _p, _i, _p, _p], _i),
    "mf_tsdf_label_image": ([_p] + [_i] * 3 + [_d] * 4 + [_p, _i, _i] + [_d] * 4 + [_p, _i, _p, _p], _i),
    "mf_tsdf_instance_stats": ([_p, _p] + [_i] * 3 + [_d, _i, _p, _i, _p, _p], _i),
    "mf_tsdf_publish_grids": ([_p, _p] + [_i] * 3 + [_d] * 4 + [_p] * 5 + [_d, _i, _d, _d] + [_i] * 3 + [_p] * 5, _i),
    "mf_tsdf_summary_bytes": ([_i] * 4, _i64),
    "mf_tsdf_block_summary": ([_p] + [_i] * 4 + [_p, _p], _i),
    "mf_tsdf_render": ([_p] + [_i] * 3 + [_d] * 7 + [_i] * 3 + [_d] * 4 + [_p, _p, _i, _p, _i] + [_p] * 5, _i),
    "mf_tsdf_integrate_colors": ([_p] + [_i] * 3 + [_d] * 6 + [_p, _p, _i, _i] + [_d] * 4 + [_p, _p, _p], _i),
    "mf_tsdf_color_image": ([_p] + [_i] * 3 + [_d] * 4 + [_p, _i, _i] + [_d] * 4 + [_p, _p, _p], _i),
    "mf_tsdf_sample_colors": ([_p] + [_i] * 3 + [_d] * 4 + [_p, _i64, _p, _p], _i),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def bind(handle, partial=False):
    """Set ``argtypes`` / ``restype`` of every ``_SIGNATURES`` entry on a ``ctypes.CDLL`` and return it.  A missing
    symbol raises, unless ``partial``: a library built from a few of the csrc files binds the ones it has."""
    for name, (argtypes, restype) in _SIGNATURES.items():
        fn = getattr(handle, name, None) if partial else getattr(handle, name)  # AttributeError: symbol absent
        if fn is not None:
            fn.argtypes, fn.restype = argtypes, restype
    return handle


def lib():
    """Load libmfhip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                f"{SO_PATH} is missing: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
                "morefusion_amd/csrc`). morefusion_amd has no CPU fallback."
            )
        handle = bind(ctypes.CDLL(SO_PATH))
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().mf_last_error_string().decode()
        raise RuntimeError(f"{what} failed ({code}): {msg}")


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def require_gpu(*tensors):
    """Every tensor on the GPU, and on the CURRENT device: the kernels are launched on the current
    device's stream (``stream_ptr``), so a tensor of another GPU would be dereferenced by the wrong
    device (one process may drive several GPUs: select the device with ``torch.cuda.device``)."""
    cur = None
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"expected torch.Tensor, got {type(t)}")
        if not t.is_cuda:
            raise RuntimeError(
                "morefusion_amd voxel/refinement ops run on the MI355X only: got a "
                f"{t.device} tensor (there is no CPU fallback; move inputs to 'cuda')."
            )
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise RuntimeError(
                f"tensor on {t.device} but the current device is cuda:{cur}: run the op under "
                f"`with torch.cuda.device({t.device.index}):` (kernels launch on the current device's stream)")


def ptr(t):
    return None if t is None else t.data_ptr()


def f32c(t):
    return t.detach().to(torch.float32).contiguous()


def i32c(t):
    return t.detach().to(torch.int32).contiguous()


def as_float3(origin):
    if isinstance(origin, torch.Tensor):
        origin = origin.detach().cpu().tolist()
    o = [float(x) for x in origin]
    if len(o) != 3:
        raise ValueError("origin must have 3 elements")
    return o
