"""ctypes binding of the C-ABI in include/ga_surfel.h (libga_mi355.so, built in-tree by csrc/Makefile).

There is NO fallback: if the HIP library is missing or does not export a declared symbol this module raises, and
every product entry point that needs it fails loudly (the oracle under oracle/ is test infrastructure, never a
substitute).
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libga_mi355.so")

GA_OK = 0
GA_STATUS_NUM_RENDERED, GA_STATUS_OVERFLOW, GA_STATUS_MAX_TILE, GA_STATUS_WORDS = 0, 1, 2, 16
GA_STATUS_SEG_WORK = 9
GA_SURFEL_FLAG_STATS, GA_SURFEL_FLAG_WORKSPACE_CLEAN, GA_SURFEL_FLAG_SPLIT_WALK, GA_SURFEL_FLAG_BG_IN_BLEND = 1, 2, 4, 8
GA_SEG_EPOCH_WORD = 96   # csrc/surfel_common.h: kSegEpochWord
GA_SURFEL_RECORD_FLOATS = 24
GA_SURFEL_STAGE_EVENTS = 5
_ERR = {-1: "GA_ERR_NULL_ARG", -2: "GA_ERR_BAD_SHAPE", -3: "GA_ERR_WORKSPACE", -4: "GA_ERR_LAUNCH", -5: "GA_ERR_BAD_FLAGS"}
GA_SURFEL_STORE_PLAIN, GA_SURFEL_STORE_WRITE_THROUGH, GA_SURFEL_STORE_NONTEMPORAL = 0, 1, 2


def store_flags(pre: int = 0, fill: int = 0, sort: int = 0, blend: int = 0) -> int:
    """include/ga_surfel.h: GA_SURFEL_STORE_FLAGS -- the store-policy field of GaSurfelForwardArgs.flags (bits 4..11, two per site)"""
    return ((pre & 3) | ((fill & 3) << 2) | ((sort & 3) << 4) | ((blend & 3) << 6)) << 4


GA_SURFEL_STORE_DEFAULT = store_flags(0, 0, 0, 0)   # include/ga_surfel.h: the measured choice (profiles/store_policy_ab.txt)



class GaSurfelForwardArgs(ctypes.Structure):
    _fields_ = [
        ("num_points", ctypes.c_int32), ("num_views", ctypes.c_int32),
        ("image_height", ctypes.c_int32), ("image_width", ctypes.c_int32),
        ("scale_modifier", ctypes.c_float), ("flags", ctypes.c_int32),
        ("means3D", ctypes.c_void_p), ("opacities", ctypes.c_void_p), ("colors", ctypes.c_void_p),
        ("scales", ctypes.c_void_p), ("rotations", ctypes.c_void_p),
        ("viewmatrix", ctypes.c_void_p), ("projmatrix", ctypes.c_void_p), ("bg", ctypes.c_void_p),
        ("out_color", ctypes.c_void_p), ("out_others", ctypes.c_void_p), ("radii", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t), ("capacity", ctypes.c_int64),
        ("stage_events", ctypes.POINTER(ctypes.c_void_p)), ("seg_capacity", ctypes.c_int64),
        ("seg_T", ctypes.c_void_p), ("seg_T_floats", ctypes.c_int64),
    ]


class GaSurfelWorkspaceLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in (
        "status", "seg_sync", "tile_count", "tile_start", "tile_cursor", "tile_order", "run_table", "rect", "depth", "record", "keys",
        "point_list", "seg_table", "seg_scratch", "view_total", "total_bytes")]


class GaSurfelBackwardArgs(ctypes.Structure):
    """include/ga_surfel.h: GaSurfelBackwardArgs"""
    _fields_ = [("fwd", GaSurfelForwardArgs), ("grad_color", ctypes.c_void_p), ("grad_others", ctypes.c_void_p),
                ("scratch", ctypes.c_void_p), ("scratch_bytes", ctypes.c_size_t), ("grad_means3D", ctypes.c_void_p),
                ("grad_opacities", ctypes.c_void_p), ("grad_colors", ctypes.c_void_p), ("grad_scales", ctypes.c_void_p),
                ("grad_rotations", ctypes.c_void_p)]


class GaSurfelPostArgs(ctypes.Structure):
    """include/ga_surfel.h: GaSurfelPostArgs"""
    _fields_ = [("num_views", ctypes.c_int32), ("image_height", ctypes.c_int32), ("image_width", ctypes.c_int32),
                ("color", ctypes.c_void_p), ("allmap", ctypes.c_void_p), ("viewmatrix", ctypes.c_void_p),
                ("image", ctypes.c_void_p), ("rend_normal", ctypes.c_void_p), ("depth", ctypes.c_void_p)]


class GaTsdfVolume(ctypes.Structure):
    """include/ga_tsdf.h: GaTsdfVolume"""
    _fields_ = [("units", ctypes.c_int32 * 3), ("unit0", ctypes.c_int32 * 3), ("voxel_length", ctypes.c_double),
                ("sdf_trunc", ctypes.c_double), ("tsdf", ctypes.c_void_p), ("weight", ctypes.c_void_p),
                ("color", ctypes.c_void_p), ("touched", ctypes.c_void_p), ("allocated", ctypes.c_void_p)]


class GaTsdfFrame(ctypes.Structure):
    """include/ga_tsdf.h: GaTsdfFrame"""
    _fields_ = [("height", ctypes.c_int32), ("width", ctypes.c_int32), ("rgb", ctypes.c_void_p), ("depth", ctypes.c_void_p),
                ("alpha", ctypes.c_void_p), ("alpha_thres", ctypes.c_float), ("depth_trunc", ctypes.c_float),
                ("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double),
                ("extrinsic", ctypes.c_double * 16), ("pose", ctypes.c_double * 16), ("depth_sampling_stride", ctypes.c_int32)]


class GaFpsArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaFpsArgs"""
    _fields_ = [("batch", ctypes.c_int32), ("num_points", ctypes.c_int32), ("num_samples", ctypes.c_int32),
                ("points", ctypes.c_void_p), ("lengths", ctypes.c_void_p), ("start_idx", ctypes.c_void_p),
                ("out_idx", ctypes.c_void_p), ("out_points", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
                ("workspace_bytes", ctypes.c_size_t)]


class GaFpsPlan(ctypes.Structure):
    """include/ga_pointcloud.h: GaFpsPlan"""
    _fields_ = [("variant", ctypes.c_int32), ("threads", ctypes.c_int32), ("points_per_lane", ctypes.c_int32)]


class GaNearestArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaNearestArgs"""
    _fields_ = [("batch", ctypes.c_int32), ("num_query", ctypes.c_int32), ("num_target", ctypes.c_int32),
                ("query", ctypes.c_void_p), ("target", ctypes.c_void_p), ("query_lengths", ctypes.c_void_p),
                ("target_lengths", ctypes.c_void_p), ("out_dist2", ctypes.c_void_p), ("out_idx", ctypes.c_void_p)]


class GaKnnArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaKnnArgs"""
    _fields_ = [("batch", ctypes.c_int32), ("num_query", ctypes.c_int32), ("num_target", ctypes.c_int32), ("k", ctypes.c_int32),
                ("query", ctypes.c_void_p), ("target", ctypes.c_void_p), ("query_lengths", ctypes.c_void_p),
                ("target_lengths", ctypes.c_void_p), ("out_dist2", ctypes.c_void_p), ("out_idx", ctypes.c_void_p)]


class GaKnnPlan(ctypes.Structure):
    """include/ga_pointcloud.h: GaKnnPlan"""
    _fields_ = [("k_slots", ctypes.c_int32), ("threads", ctypes.c_int32), ("tile", ctypes.c_int32), ("grid_x", ctypes.c_int32),
                ("grid_y", ctypes.c_int32)]


class GaKnnBackwardArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaKnnBackwardArgs"""
    _fields_ = [("batch", ctypes.c_int32), ("num_query", ctypes.c_int32), ("num_target", ctypes.c_int32), ("k", ctypes.c_int32),
                ("query", ctypes.c_void_p), ("target", ctypes.c_void_p), ("query_lengths", ctypes.c_void_p),
                ("target_lengths", ctypes.c_void_p), ("idx", ctypes.c_void_p), ("grad_dist2", ctypes.c_void_p),
                ("grad_query", ctypes.c_void_p), ("grad_target", ctypes.c_void_p)]


class GaNormalsArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaNormalsArgs"""
    _fields_ = [("batch", ctypes.c_int32), ("num_points", ctypes.c_int32), ("k", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("points", ctypes.c_void_p), ("lengths", ctypes.c_void_p), ("idx", ctypes.c_void_p), ("viewpoint", ctypes.c_void_p),
                ("normal", ctypes.c_void_p), ("tangent", ctypes.c_void_p), ("eigenvalues", ctypes.c_void_p)]


class GaNormalsPlan(ctypes.Structure):
    """include/ga_pointcloud.h: GaNormalsPlan"""
    _fields_ = [("threads", ctypes.c_int32), ("grid_x", ctypes.c_int32), ("grid_y", ctypes.c_int32), ("sweeps", ctypes.c_int32)]


class GaSurfelInitArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaSurfelInitArgs"""
    _fields_ = [("batch", ctypes.c_int32), ("num_points", ctypes.c_int32), ("k", ctypes.c_int32), ("opacity", ctypes.c_float),
                ("scale_factor", ctypes.c_float), ("reserved", ctypes.c_int32),
                ("points", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("tangent", ctypes.c_void_p), ("dist2", ctypes.c_void_p),
                ("lengths", ctypes.c_void_p), ("eigenvalues", ctypes.c_void_p), ("colors", ctypes.c_void_p),
                ("gaussians", ctypes.c_void_p)]


class GaUnprojectArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaUnprojectArgs"""
    _fields_ = [(n, ctypes.c_int32) for n in ("num_views", "height", "width", "depth_kind", "color_kind", "erode", "drop_zero",
                                              "pixel_stride", "capacity")] + \
               [(n, ctypes.c_float) for n in ("depth_min", "depth_max", "mask_threshold", "clip")] + [("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("depth", "mask", "color", "normal", "cameras", "points", "colors", "normals", "source",
                                               "count", "view_counts", "workspace")] + [("workspace_bytes", ctypes.c_size_t)]


_PC_FILTER_CLOUD = ("in_count", "points", "colors", "normals", "source")
_PC_FILTER_OUT = ("out_points", "out_colors", "out_normals", "out_source", "kept_rows", "count", "view_counts")


class GaFilterViewsArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaFilterViewsArgs"""
    _fields_ = [(n, ctypes.c_int32) for n in ("rows", "capacity", "num_views", "height", "width", "depth_kind", "window", "min_support",
                                              "max_conflicts", "carve")] + \
               [(n, ctypes.c_float) for n in ("depth_min", "depth_max", "mask_threshold", "tol_abs", "tol_rel")] + \
               [("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in _PC_FILTER_CLOUD + ("depth", "mask", "cameras") + _PC_FILTER_OUT +
                ("support", "conflicts", "workspace")] + [("workspace_bytes", ctypes.c_size_t)]


class GaVoxelThinArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaVoxelThinArgs"""
    _fields_ = [(n, ctypes.c_int32) for n in ("rows", "capacity", "keep", "num_views", "view_pixels", "flags")] + \
               [("origin", ctypes.c_float * 3), ("voxel_size", ctypes.c_float), ("table_slots", ctypes.c_int64)] + \
               [(n, ctypes.c_void_p) for n in _PC_FILTER_CLOUD + _PC_FILTER_OUT + ("multiplicity", "dropped", "workspace")] + \
               [("workspace_bytes", ctypes.c_size_t)]


class GaAlignArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaAlignArgs"""
    _fields_ = [(n, ctypes.c_int32) for n in ("batch", "num_points", "estimate_scale", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("x", "y", "weights", "lengths", "transform", "rmse", "status", "workspace")] + \
               [("workspace_bytes", ctypes.c_size_t)]


class GaIcpArgs(ctypes.Structure):
    """include/ga_pointcloud.h: GaIcpArgs"""
    _fields_ = [(n, ctypes.c_int32) for n in ("batch", "num_points", "num_target", "max_iterations", "estimate_scale", "reserved")] + \
               [("relative_rmse_thr", ctypes.c_float), ("max_distance", ctypes.c_float)] + \
               [(n, ctypes.c_void_p) for n in ("x", "y", "weights", "x_lengths", "y_lengths", "init_transform", "transform", "rmse",
                                               "status", "iterations", "history", "xt", "idx", "dist2", "workspace")] + \
               [("workspace_bytes", ctypes.c_size_t)]


class GaAlignPlan(ctypes.Structure):
    """include/ga_pointcloud.h: GaAlignPlan"""
    _fields_ = [(n, ctypes.c_int32) for n in ("threads", "tile", "grid_x", "solve_threads", "sweeps", "terms")]


class GaMeshSampleArgs(ctypes.Structure):
    """include/ga_mesh.h: GaMeshSampleArgs"""
    _fields_ = [(n, ctypes.c_int32) for n in ("num_vertices", "num_faces", "num_samples", "reserved")] + [("seed", ctypes.c_uint64)] + \
               [(n, ctypes.c_void_p) for n in ("seed_words", "vertices", "faces", "vertex_colors", "points", "face", "bary", "normals",
                                               "colors", "workspace")] + [("workspace_bytes", ctypes.c_size_t)]


class GaMeshSamplePlan(ctypes.Structure):
    """include/ga_mesh.h: GaMeshSamplePlan"""
    _fields_ = [(n, ctypes.c_int32) for n in ("threads", "faces_per_group", "sums_per_trip", "num_groups")] + \
               [("workspace_bytes", ctypes.c_size_t)]


class GaMeshPointDistanceArgs(ctypes.Structure):
    """include/ga_mesh.h: GaMeshPointDistanceArgs"""
    _fields_ = [(n, ctypes.c_int32) for n in ("num_points", "num_vertices", "num_faces", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("points", "count", "vertices", "faces", "dist2", "face", "closest", "bary", "workspace")] + \
               [("workspace_bytes", ctypes.c_size_t)]


class GaMeshPointDistancePlan(ctypes.Structure):
    """include/ga_mesh.h: GaMeshPointDistancePlan"""
    _fields_ = [(n, ctypes.c_int32) for n in ("threads", "tile", "tiles_per_chunk", "num_chunks")] + [("workspace_bytes", ctypes.c_size_t)]


class GaPhotoLossArgs(ctypes.Structure):
    """include/ga_loss.h: GaPhotoLossArgs"""
    _fields_ = [("num_images", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32), ("img1", ctypes.c_void_p), ("img2", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("ssim_map", ctypes.c_void_p), ("grad_out", ctypes.c_void_p), ("grad_img1", ctypes.c_void_p),
                ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]


class GaPhotoLossPlan(ctypes.Structure):
    """include/ga_loss.h: GaPhotoLossPlan"""
    _fields_ = [("tile_w", ctypes.c_int32), ("tile_h", ctypes.c_int32), ("threads", ctypes.c_int32), ("tiles_x", ctypes.c_int32),
                ("tiles_y", ctypes.c_int32), ("lds_bytes", ctypes.c_int32), ("grid_x", ctypes.c_int64), ("num_partials", ctypes.c_int64)]


class GaGeoLossArgs(ctypes.Structure):
    """include/ga_loss.h: GaGeoLossArgs"""
    _fields_ = [("num_views", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("tanfov", ctypes.c_double), ("view", ctypes.c_void_p), ("rend_normal", ctypes.c_void_p), ("depth", ctypes.c_void_p),
                ("alpha", ctypes.c_void_p), ("dist", ctypes.c_void_p), ("target_normal", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("surf_normal_out", ctypes.c_void_p), ("grad_out", ctypes.c_void_p),
                ("grad_rend_normal", ctypes.c_void_p), ("grad_depth", ctypes.c_void_p), ("grad_dist", ctypes.c_void_p),
                ("grad_alpha", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]


class GaGeoLossPlan(ctypes.Structure):
    """include/ga_loss.h: GaGeoLossPlan"""
    _fields_ = [("tile_w", ctypes.c_int32), ("tile_h", ctypes.c_int32), ("threads", ctypes.c_int32), ("tiles_x", ctypes.c_int32),
                ("tiles_y", ctypes.c_int32), ("lds_bytes", ctypes.c_int32), ("lds_bytes_backward", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("grid_x", ctypes.c_int64), ("num_partials", ctypes.c_int64)]


class GaFitPlan(ctypes.Structure):
    """include/ga_fit.h: GaFitPlan"""
    _fields_ = [(n, ctypes.c_int32) for n in ("threads", "pack_vec", "grid_activate", "grid_adam", "grid_pack_x", "grid_pack_y")] + \
               [(n, ctypes.c_size_t) for n in ("means", "opacities", "colors", "scales", "rotations", "inv_norm", "workspace_bytes")]


class GaFitActivateArgs(ctypes.Structure):
    """include/ga_fit.h: GaFitActivateArgs"""
    _fields_ = [("num_points", ctypes.c_int32), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("raw", "means", "opacities", "colors", "scales", "rotations", "inv_norm")]


class GaFitPackArgs(ctypes.Structure):
    """include/ga_fit.h: GaFitPackArgs"""
    _fields_ = [(n, ctypes.c_int32) for n in ("num_views", "height", "width", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("color", "allmap", "view", "g_image", "g_rend_normal", "g_depth", "g_dist", "g_alpha",
                                               "g_color", "g_allmap")]


class GaFitAdamArgs(ctypes.Structure):
    """include/ga_fit.h: GaFitAdamArgs"""
    _fields_ = [(n, ctypes.c_int32) for n in ("num_points", "num_views", "flags", "max_steps")] + \
               [(n, ctypes.c_void_p) for n in ("g_means", "g_opacities", "g_colors", "g_scales", "g_rotations", "opacities", "colors",
                                               "scales", "rotations", "inv_norm", "raw", "m", "v", "radii", "table", "counter")] + \
               [(n, ctypes.c_float) for n in ("beta1", "one_minus_beta1", "beta2", "one_minus_beta2", "eps")] + \
               [("reserved", ctypes.c_int32), ("raw_grad", ctypes.c_void_p)]


class GaFitAdvanceArgs(ctypes.Structure):
    """include/ga_fit.h: GaFitAdvanceArgs"""
    _fields_ = [("num_views", ctypes.c_int32), ("max_steps", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("counter", "photo_out", "geo_out", "w_photo", "w_geo", "history")] + \
               [("ssim_bias", ctypes.c_float), ("reserved", ctypes.c_int32), ("status", ctypes.c_void_p), ("seen", ctypes.c_void_p)]


class GaFitSelectArgs(ctypes.Structure):
    """include/ga_fit.h: GaFitSelectArgs"""
    _fields_ = [(n, ctypes.c_int32) for n in ("pool_views", "batch_views", "height", "width", "max_steps", "flags")] + \
               [(n, ctypes.c_void_p) for n in ("schedule", "counter", "pool_view", "pool_proj", "pool_targets", "pool_mask", "pool_normal",
                                               "view", "proj", "targets", "mask", "normal", "selected")]


class GaFitAccumulateArgs(ctypes.Structure):
    """include/ga_densify.h: GaFitAccumulateArgs"""
    _fields_ = [("num_points", ctypes.c_int32), ("num_views", ctypes.c_int32), ("tanfov", ctypes.c_float), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("g_means", "means", "radii", "view", "grad_accum", "denom", "max_radius")]


class GaDensifyArgs(ctypes.Structure):
    """include/ga_densify.h: GaDensifyArgs"""
    _fields_ = [("num_points", ctypes.c_int32), ("flags", ctypes.c_int32), ("round", ctypes.c_uint32), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_float) for n in ("grad_threshold", "min_opacity", "percent_dense", "extent", "max_screen_size")] + \
               [("reserved2", ctypes.c_int32), ("seed", ctypes.c_uint64)] + \
               [(n, ctypes.c_void_p) for n in ("raw", "m", "v", "opacities", "scales", "rotations", "grad_accum", "denom", "max_radius",
                                               "out_raw", "out_m", "out_v", "parent", "noise_out", "out_counts", "workspace")] + \
               [("workspace_bytes", ctypes.c_size_t)]


class GaFitResetOpacityArgs(ctypes.Structure):
    """include/ga_densify.h: GaFitResetOpacityArgs"""
    _fields_ = [("num_points", ctypes.c_int32), ("logit_cap", ctypes.c_float), ("raw", ctypes.c_void_p), ("m", ctypes.c_void_p),
                ("v", ctypes.c_void_p)]


GA_DENSIFY_PRUNE_ONLY, GA_DENSIFY_COUNTS = 1, 8
GA_FIT_PARAMS, GA_FIT_GROUPS, GA_FIT_TABLE_COLS, GA_FIT_HISTORY_COLS, GA_FIT_VISIBLE_ONLY = 13, 5, 8, 8, 1
GA_FIT_SELECT_U8_TARGETS = 1
GA_FPS_VARIANT_REGISTER, GA_FPS_VARIANT_STREAMING = 0, 1
GA_PHOTO_LOSS_SAVE = 1
GA_GEO_LOSS_TARGET, GA_GEO_LOSS_NORMALS = 1, 2
GA_PC_KNN_MAX_K = 32
GA_PC_NORMALS_SWEEPS, GA_PC_NORMALS_MIN_K, GA_PC_SURFEL_MIN_K, GA_PC_SURFEL_FLOATS = 5, 3, 4, 13
GA_PC_DEPTH_Z, GA_PC_DEPTH_RAY, GA_PC_COLOR_F32, GA_PC_COLOR_U8 = 0, 1, 0, 1
GA_PC_UNPROJECT_THREADS, GA_PC_UNPROJECT_TILE_PIXELS, GA_PC_UNPROJECT_MAX_WIDTH, GA_PC_UNPROJECT_MAX_ERODE = 256, 1024, 4096, 4
GA_PC_CAMERA_FLOATS = 21
GA_PC_FILTER_THREADS, GA_PC_FILTER_BAND_ROWS, GA_PC_FILTER_MAX_ROWS = 256, 1024, 1 << 30
GA_PC_VOXEL_FIRST, GA_PC_VOXEL_CENTER, GA_PC_VOXEL_MAX_INDEX, GA_PC_VOXEL_WAVE_MERGE = 0, 1, (1 << 20) - 1, 1
GA_PC_ALIGN_SWEEPS, GA_PC_ALIGN_TERMS, GA_PC_TRANSFORM_FLOATS, GA_PC_ALIGN_HISTORY_FLOATS = 6, 19, 13, 14
GA_PC_ALIGN_RUNNING, GA_PC_ALIGN_CONVERGED, GA_PC_ALIGN_DEGENERATE, GA_PC_ICP_MAX_ITERATIONS = 0, 1, 2, 10000
GA_MESH_THREADS, GA_MESH_PHILOX_STREAM, GA_MESH_MAX_FACES, GA_MESH_MAX_ROWS = 256, 0x4853454D, 1 << 27, 1 << 29

EXPORTS = ("ga_surfel_version", "ga_surfel_workspace_layout", "ga_surfel_workspace_layout2", "ga_surfel_forward", "ga_surfel_postprocess",
           "ga_surfel_backward", "ga_surfel_backward_scratch_bytes", "ga_surfel_store_policy",
           "ga_tsdf_integrate", "ga_tsdf_mesh_scratch_bytes", "ga_tsdf_mesh_count", "ga_tsdf_mesh_emit", "ga_mesh_write_obj", "ga_mesh_cluster_labels",
           "ga_pc_fps", "ga_pc_fps_plan", "ga_pc_fps_workspace_bytes", "ga_pc_nearest",
           "ga_pc_knn", "ga_pc_knn_plan", "ga_pc_knn_backward", "ga_pc_normals", "ga_pc_normals_plan", "ga_pc_surfel_init",
           "ga_pc_unproject", "ga_pc_unproject_workspace_bytes",
           "ga_pc_filter_views", "ga_pc_filter_views_workspace_bytes", "ga_pc_voxel_thin", "ga_pc_voxel_thin_workspace_bytes",
           "ga_pc_align_plan", "ga_pc_align_workspace_bytes", "ga_pc_align_points", "ga_pc_icp",
           "ga_mesh_sample_plan", "ga_mesh_sample", "ga_mesh_point_distance_plan", "ga_mesh_point_distance",
           "ga_photo_loss_plan", "ga_photo_loss_workspace_bytes", "ga_photo_loss_forward", "ga_photo_loss_backward",
           "ga_geo_loss_plan", "ga_geo_loss_workspace_bytes", "ga_geo_loss_forward", "ga_geo_loss_backward",
           "ga_fit_plan", "ga_fit_activate", "ga_fit_pack_grads", "ga_fit_adam", "ga_fit_advance", "ga_fit_select_views",
           "ga_fit_accumulate", "ga_densify_workspace_bytes", "ga_densify", "ga_fit_reset_opacity")

_lib = None


def build(verbose: bool = False) -> str:
    """Compile every HIP translation unit for gfx950 (hipcc cross-compiles without a GPU) into LIB_PATH."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")] + ([] if verbose else ["-s"])
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the MI355X HIP library has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C gaussiananything_amd/csrc`). "
                "There is no CPU fallback for the product path.")
        # torch first: the library's libamdhip64 dependency must resolve to the HIP runtime PyTorch has loaded (its streams and
        # allocations are handed to the kernels); loaded the other way round -- e.g. build() and then smoke() in one process --
        # the process ends up with the launches failing (GA_ERR_LAUNCH)
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name in EXPORTS:
            if not hasattr(L, name):
                raise RuntimeError(f"{LIB_PATH} does not export {name}")
        L.ga_surfel_version.restype = ctypes.c_char_p
        L.ga_surfel_workspace_layout.restype = ctypes.c_int
        L.ga_surfel_workspace_layout.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_int64,
                                                                       ctypes.POINTER(GaSurfelWorkspaceLayout)]
        L.ga_surfel_workspace_layout2.restype = ctypes.c_int
        L.ga_surfel_workspace_layout2.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_int64, ctypes.c_int64,
                                                                        ctypes.POINTER(GaSurfelWorkspaceLayout)]
        L.ga_surfel_forward.restype = ctypes.c_int
        L.ga_surfel_forward.argtypes = [ctypes.POINTER(GaSurfelForwardArgs), ctypes.c_void_p]
        L.ga_surfel_store_policy.restype = ctypes.c_int
        L.ga_surfel_store_policy.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32 * 4)]
        L.ga_surfel_backward.restype = ctypes.c_int
        L.ga_surfel_backward.argtypes = [ctypes.POINTER(GaSurfelBackwardArgs), ctypes.c_void_p]
        L.ga_surfel_backward_scratch_bytes.restype = ctypes.c_size_t
        L.ga_surfel_backward_scratch_bytes.argtypes = [ctypes.POINTER(GaSurfelForwardArgs)]
        L.ga_surfel_postprocess.restype = ctypes.c_int
        L.ga_surfel_postprocess.argtypes = [ctypes.POINTER(GaSurfelPostArgs), ctypes.c_void_p]
        L.ga_tsdf_integrate.restype = ctypes.c_int
        L.ga_tsdf_integrate.argtypes = [ctypes.POINTER(GaTsdfVolume), ctypes.POINTER(GaTsdfFrame), ctypes.c_void_p]
        L.ga_tsdf_mesh_scratch_bytes.restype = ctypes.c_size_t
        L.ga_tsdf_mesh_scratch_bytes.argtypes = [ctypes.POINTER(GaTsdfVolume)]
        L.ga_tsdf_mesh_count.restype = ctypes.c_int
        L.ga_tsdf_mesh_count.argtypes = [ctypes.POINTER(GaTsdfVolume), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        L.ga_mesh_cluster_labels.restype = ctypes.c_int
        L.ga_mesh_cluster_labels.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        L.ga_mesh_write_obj.restype = ctypes.c_int
        L.ga_mesh_write_obj.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
        L.ga_tsdf_mesh_emit.restype = ctypes.c_int
        L.ga_tsdf_mesh_emit.argtypes = [ctypes.POINTER(GaTsdfVolume), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int64,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ga_pc_fps.restype = ctypes.c_int
        L.ga_pc_fps.argtypes = [ctypes.POINTER(GaFpsArgs), ctypes.c_void_p]
        L.ga_pc_fps_plan.restype = ctypes.c_int
        L.ga_pc_fps_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(GaFpsPlan)]
        L.ga_pc_fps_workspace_bytes.restype = ctypes.c_size_t
        L.ga_pc_fps_workspace_bytes.argtypes = [ctypes.c_int32] * 3
        L.ga_pc_nearest.restype = ctypes.c_int
        L.ga_pc_nearest.argtypes = [ctypes.POINTER(GaNearestArgs), ctypes.c_void_p]
        L.ga_pc_knn.restype = ctypes.c_int
        L.ga_pc_knn.argtypes = [ctypes.POINTER(GaKnnArgs), ctypes.c_void_p]
        L.ga_pc_knn_plan.restype = ctypes.c_int
        L.ga_pc_knn_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(GaKnnPlan)]
        L.ga_pc_knn_backward.restype = ctypes.c_int
        L.ga_pc_knn_backward.argtypes = [ctypes.POINTER(GaKnnBackwardArgs), ctypes.c_void_p]
        L.ga_pc_normals.restype = ctypes.c_int
        L.ga_pc_normals.argtypes = [ctypes.POINTER(GaNormalsArgs), ctypes.c_void_p]
        L.ga_pc_normals_plan.restype = ctypes.c_int
        L.ga_pc_normals_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(GaNormalsPlan)]
        L.ga_pc_surfel_init.restype = ctypes.c_int
        L.ga_pc_surfel_init.argtypes = [ctypes.POINTER(GaSurfelInitArgs), ctypes.c_void_p]
        L.ga_pc_unproject.restype = ctypes.c_int
        L.ga_pc_unproject.argtypes = [ctypes.POINTER(GaUnprojectArgs), ctypes.c_void_p]
        L.ga_pc_unproject_workspace_bytes.restype = ctypes.c_size_t
        L.ga_pc_unproject_workspace_bytes.argtypes = [ctypes.c_int32] * 3
        L.ga_pc_filter_views.restype = ctypes.c_int
        L.ga_pc_filter_views.argtypes = [ctypes.POINTER(GaFilterViewsArgs), ctypes.c_void_p]
        L.ga_pc_filter_views_workspace_bytes.restype = ctypes.c_size_t
        L.ga_pc_filter_views_workspace_bytes.argtypes = [ctypes.c_int32]
        L.ga_pc_voxel_thin.restype = ctypes.c_int
        L.ga_pc_voxel_thin.argtypes = [ctypes.POINTER(GaVoxelThinArgs), ctypes.c_void_p]
        L.ga_pc_voxel_thin_workspace_bytes.restype = ctypes.c_size_t
        L.ga_pc_voxel_thin_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int64]
        L.ga_pc_align_plan.restype = ctypes.c_int
        L.ga_pc_align_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(GaAlignPlan)]
        L.ga_pc_align_workspace_bytes.restype = ctypes.c_size_t
        L.ga_pc_align_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32]
        L.ga_pc_align_points.restype = ctypes.c_int
        L.ga_pc_align_points.argtypes = [ctypes.POINTER(GaAlignArgs), ctypes.c_void_p]
        L.ga_pc_icp.restype = ctypes.c_int
        L.ga_pc_icp.argtypes = [ctypes.POINTER(GaIcpArgs), ctypes.c_void_p]
        L.ga_mesh_sample_plan.restype = ctypes.c_int
        L.ga_mesh_sample_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(GaMeshSamplePlan)]
        L.ga_mesh_sample.restype = ctypes.c_int
        L.ga_mesh_sample.argtypes = [ctypes.POINTER(GaMeshSampleArgs), ctypes.c_void_p]
        L.ga_mesh_point_distance_plan.restype = ctypes.c_int
        L.ga_mesh_point_distance_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(GaMeshPointDistancePlan)]
        L.ga_mesh_point_distance.restype = ctypes.c_int
        L.ga_mesh_point_distance.argtypes = [ctypes.POINTER(GaMeshPointDistanceArgs), ctypes.c_void_p]
        L.ga_photo_loss_plan.restype = ctypes.c_int
        L.ga_photo_loss_plan.argtypes = [ctypes.c_int32] * 4 + [ctypes.POINTER(GaPhotoLossPlan)]
        L.ga_photo_loss_workspace_bytes.restype = ctypes.c_size_t
        L.ga_photo_loss_workspace_bytes.argtypes = [ctypes.c_int32] * 5
        L.ga_photo_loss_forward.restype = ctypes.c_int
        L.ga_photo_loss_forward.argtypes = [ctypes.POINTER(GaPhotoLossArgs), ctypes.c_void_p]
        L.ga_photo_loss_backward.restype = ctypes.c_int
        L.ga_photo_loss_backward.argtypes = [ctypes.POINTER(GaPhotoLossArgs), ctypes.c_void_p]
        L.ga_geo_loss_plan.restype = ctypes.c_int
        L.ga_geo_loss_plan.argtypes = [ctypes.c_int32] * 3 + [ctypes.POINTER(GaGeoLossPlan)]
        L.ga_geo_loss_workspace_bytes.restype = ctypes.c_size_t
        L.ga_geo_loss_workspace_bytes.argtypes = [ctypes.c_int32] * 3
        L.ga_geo_loss_forward.restype = ctypes.c_int
        L.ga_geo_loss_forward.argtypes = [ctypes.POINTER(GaGeoLossArgs), ctypes.c_void_p]
        L.ga_geo_loss_backward.restype = ctypes.c_int
        L.ga_geo_loss_backward.argtypes = [ctypes.POINTER(GaGeoLossArgs), ctypes.c_void_p]
        L.ga_fit_plan.restype = ctypes.c_int
        L.ga_fit_plan.argtypes = [ctypes.c_int32] * 4 + [ctypes.POINTER(GaFitPlan)]
        for name, struct in (("ga_fit_activate", GaFitActivateArgs), ("ga_fit_pack_grads", GaFitPackArgs), ("ga_fit_adam", GaFitAdamArgs),
                             ("ga_fit_advance", GaFitAdvanceArgs), ("ga_fit_select_views", GaFitSelectArgs),
                             ("ga_fit_accumulate", GaFitAccumulateArgs),
                             ("ga_densify", GaDensifyArgs), ("ga_fit_reset_opacity", GaFitResetOpacityArgs)):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = [ctypes.POINTER(struct), ctypes.c_void_p]
        L.ga_densify_workspace_bytes.restype = ctypes.c_size_t
        L.ga_densify_workspace_bytes.argtypes = [ctypes.c_int32]
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != GA_OK:
        raise RuntimeError(f"{what} failed: {_ERR.get(rc, rc)}")
