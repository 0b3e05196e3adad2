"""ctypes binding of libnof.so (the C ABI declared in include/nof.h).

torch is imported first so that its bundled HIP runtime (soname
libamdhip64.so.7) is the one libnof.so binds to: one runtime, one set of
streams. There is no CPU fallback anywhere behind this module — a missing or
unloadable library raises immediately.
"""
import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL load, see module doc)

_HERE = os.path.dirname(os.path.abspath(__file__))
# NOF_LIB: the timing-ablation build (scripts/ablate.py) only
LIB_PATH = os.environ.get("NOF_LIB") or os.path.join(_HERE, "libnof.so")
_LIB = None

_p = ctypes.c_void_p
_u32 = ctypes.c_uint32
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_f32 = ctypes.c_float
_int = ctypes.c_int

_SIGNATURES = {
    "nof_last_error": ([], ctypes.c_char_p),
    "nof_version": ([], ctypes.c_char_p),
    "nof_level_params": ([_u32, _f32, _u32, _p, _p], None),
    "nof_grid_encode_forward": ([_p, _p, _p, _p, _u32, _u32, _u32, _u32, _f32, _u32, _int, _p, _u32, _int, _int, _p],
                                _int),
    "nof_grid_encode_backward": ([_p, _p, _p, _p, _p, _u32, _u32, _u32, _u32, _f32, _u32, _int, _p, _p, _u32, _int,
                                  _int, _p], _int),
    "nof_sample_rays_uniform_occupied_voxels": ([_p, _p, _p, _i32, _i32, _i32, _p, _p], _int),
    "nof_postprocess_octree_ray_tracing": ([_p, _p, _p, _p, _i64, _i64, _i32, _p, _p], _int),
    "nof_ray_color_to_texture_uv": ([_p, _p, _p, _p, _p, _p, _i64, _p], _int),
    "nof_octree_ray_trace": ([_p, _i32, _p, _p, _i32, _i32, _p, _p, _p], _int),
    "nof_step_schedule": ([_p, _p, _p, _p], _int),
    "nof_trace_rays": ([_p, _p, _i32, _p, _p, _i32, _i32, _f32, _f32, _f32, _p, _p, _p, _p, _p, _p], _int),
    "nof_trace_rays_epoch": ([_p, _p, _p, _i32, _p, _p, _i32, _i32, _f32, _f32, _f32, _p, _p, _p, _p, _p, _p], _int),
    "nof_sample_batch": ([_p, _i32, _i32, _u32, _p, _p, _p], _int),
    "nof_pack_mlp": ([_p, _p, _i32, _i32, _p, _p, _int, _p], _int),
    "nof_field_step": ([_p, _p], _int),
    "nof_field_desc_size": ([], ctypes.c_size_t),
    "nof_quad_mirror": ([_p, _p], _int),
    "nof_render_workspace_bytes": ([_i32, _i32], ctypes.c_size_t),
    "nof_render_rays": ([_p, _p, _p], _int),
    "nof_render_view_workspace_bytes": ([_i32, _i32], ctypes.c_size_t),
    "nof_render_view": ([_p, _p, _p, _p], _int),
    "nof_field_workspace_bytes": ([_i32, _i32, _i32], ctypes.c_size_t),
    "nof_field_workspace_offsets": ([_i32, _i32, _i32, _p, _i32], _int),
    "nof_field_timing": ([_i32], _int),
    "nof_pose_forward": ([_p, _p, _i32, _f32, _f32, _p, _p, _p], _int),
    "nof_step_prologue": ([_p, _p, _p, _p, _p, _i32, _f32, _f32, _p, _p, _p, _p, _i32, _i32, _p, _p, _int, _p], _int),
    "nof_query_sdf": ([_p, _i32, _p, ctypes.c_uint32, _p, _p, _i32, _i32, _p, ctypes.c_int64, _p, _p, _p, _i32, _i32,
                       _i32, _p, _i32, _p, _p], _int),
    "nof_query_field": ([_p, _i32, _p, _u32, _p, _p, _i32, _i32, _p, _i64, _p, _i32, _i32, _i32, _p, _p, _p, _p], _int),
    "nof_pose_backward": ([_p, _p, _i32, _p, _i32, _p, _p, _p], _int),
    "nof_field_timing_collect": ([_p, _i32, _p], _int),
    "nof_level_table": ([_u32, _f32, _u32, _p, _p], None),
    "nof_unscale_check": ([_p, _i64, _p, _p, _p, _i64, _i64, _i64, _p], _int),
    "nof_adam_active_bytes": ([_i64], ctypes.c_size_t),
    "nof_adam_step": ([_p, _p, _p, _p, _i64, _i64, ctypes.c_double, ctypes.c_double, _f32, _f32, _f32, _p, _p, _p,
                       _i64, _p, _p, _p, _p, _p], _int),
    "nof_scaler_update": ([_p, _p, _p, _p, _f32, _f32, _i32, _int, _p], _int),
    "nof_to_half": ([_p, _p, _i64, _p], _int),
    "nof_grad16_to_f32": ([_p, _p, _i64, _p], _int),
    "nof_ray_pool_workspace_bytes": ([_i32, _i32, _i32], ctypes.c_size_t),
    "nof_make_frame_rays": ([_p, _p], _int),
    "nof_point_grid_workspace_bytes": ([_i64], ctypes.c_size_t),
    "nof_point_grid_build": ([_p, _i32, _p, _p, ctypes.c_double, _p, _p, _p, _p, _p], _int),
    "nof_knn_mean_dist": ([_p, _i32, _i32, _p, _p], _int),
    "nof_dbscan_workspace_bytes": ([_i32, _i64], ctypes.c_size_t),
    "nof_raster_faces": ([_p, _p, _i64, _p, _p, _i32, _i32, ctypes.c_double, ctypes.c_double, _p, _p], _int),
    "nof_texture_hits": ([_p, _i32, _i32, _p, _f32, _p, _p, _p, _p, _p, _p, _p], _int),
    "nof_texture_accumulate": ([_p, _p, _i64, _p, _i32, _i32, _p, _p, _p, _p], _int),
    "nof_vertex_color_accumulate": ([_p, _i32, _i32, _p, _f32, _p, _p, _p, _p, _p, _i64, ctypes.c_double, _p, _p, _p, _p,
                                     _p], _int),
    "nof_render_mesh_workspace_bytes": ([_i32, _i64, _i32, _i32], ctypes.c_size_t),
    "nof_render_mesh": ([_p, _p], _int),
    "nof_segment_mean": ([_p, _i32, _p, _p, _i32, _p, _p], _int),
    "nof_dbscan": ([_p, _i32, ctypes.c_double, _i32, _p, _p, _p, _p, _p], _int),
    "nof_marching_cubes_blocks": ([_i32, _i32, _i32, _p], _int),
    "nof_marching_cubes_count": ([_p, _i32, _i32, _i32, _f32, _p, _p, _p, _p, _p], _int),
    "nof_marching_cubes_emit": ([_p, _i32, _i32, _i32, _f32, _p, _p, _p, _i64, _i64, _p, _p, _p], _int),
    "nof_mesh_components": ([_p, _i64, _i64, _p, _p, _p], _int),
    "nof_mesh_laplacian_step": ([_p, _p, _p, _i64, ctypes.c_double, _p, _p], _int),
    "nof_mesh_volume_workspace_bytes": ([_i64], ctypes.c_size_t),
    "nof_mesh_volume": ([_p, _p, _i64, _p, _p, _p], _int),
    "nof_mesh_scale_to_volume": ([_p, _i64, _p, _p, _p, _p], _int),
    "nof_mesh_vertex_normals": ([_p, _p, _p, _p, _i64, _p, _p], _int),
    "nof_nearest_points": ([_p, _i32, _p, _i32, _p, _p, _p, _i32, _p, _p, ctypes.c_double, ctypes.c_double, _p, _p,
                            _p], _int),
    "nof_nearest_workspace_bytes": ([_i32], ctypes.c_size_t),
    "nof_correspondence_moments": ([_p, _i32, _p, _p, _i32, _p, _p, _p, _p, _p], _int),
    "nof_ransac_workspace_bytes": ([_i32, _i64, _i32], ctypes.c_size_t),
    "nof_ransac_pairs": ([_p, _p], _int),
    "nof_pose_graph_workspace_bytes": ([_i32, _i32, _i64, _i32, _i32], ctypes.c_size_t),
    "nof_pose_graph_optimize": ([_p, _p], _int),
    "nof_frame_erode": ([_p, _p], _int),
    "nof_frame_bilateral": ([_p, _p], _int),
    "nof_frame_geometry": ([_p, _p], _int),
    "nof_frame_lift_matches": ([_p, _p], _int),
    "nof_frame_covisibility": ([_p, _p], _int),
    "nof_match_workspace_bytes": ([_i32, _i32, _i32], ctypes.c_size_t),
    "nof_match_descriptors": ([_p, _p], _int),
    "nof_feature_transformer_workspace_bytes": ([_i32, _i32, _i32, _i32], ctypes.c_size_t),
    "nof_feature_transformer": ([_p, _p], _int),
    "nof_fine_windows": ([_p, _p], _int),
    "nof_fine_expectation": ([_p, _p], _int),
}


class FieldDesc(ctypes.Structure):
    """Mirror of nof_field_desc (include/nof.h), in the header's order and sections."""
    _fields_ = [# batch inputs and scalars
                ("rays", _p), ("tf", _p), ("intervals", _p), ("totals", _p), ("t_rand", _p), ("seed", _u32),
                ("R", _i32), ("Kmax", _i32), ("N_oct", _i32), ("N_dep", _i32), ("S", _i32), ("perturb", _i32),
                ("near_sc", _f32), ("far_sc", _f32), ("trunc", _f32), ("neg_trunc_ratio", _f32), ("sdf_lambda", _f32),
                ("fs_sdf", _f32), ("first_frame_weight", _f32), ("rgb_weight", _f32), ("fs_weight", _f32),
                ("empty_weight", _f32), ("trunc_weight", _f32), ("fs_rgb_weight", _f32), ("skip_pose_grad", _i32),
                ("loss_scale", _p), ("step_params", _p),
                # parameters
                ("table", _p), ("levels", _p), ("L", _u32), ("C", _u32), ("D", _u32), ("table_dtype", _i32),
                ("mlp_dtype", _i32), ("n_ff", _i32), ("frags", _p), ("bias", _p), ("ff", _p),
                # outputs
                ("grad_table", _p), ("grad_table16", _p), ("grad_mlp", _p), ("grad_ff", _p), ("ray_grad", _p),
                ("loss_acc", _p),
                # debug outputs
                ("dbg_z", _p), ("dbg_raw", _p), ("dbg_valid", _p), ("dbg_rgb", _p),
                # workspace
                ("workspace", _p), ("table_quads", _p), ("table_rows", _i64), ("quads_prebuilt", _i32),
                # shape knobs
                ("count_atomics", _i32), ("ablate", _i32), ("scatter_slots", _i32), ("scatter_levels_per_wave", _i32), ("bwd_flush", _i32),
                ("compact_per_block", _i32), ("encode_group", _i32), ("quads_min_rays", _i32), ("xcd_order", _i32)]


class RenderOut(ctypes.Structure):
    """Mirror of nof_render_out (include/nof.h): the outputs of nof_render_rays."""
    _fields_ = [("rgb", _p), ("depth", _p), ("z", _p), ("sdf", _p), ("valid", _p), ("workspace", _p)]


class ViewDesc(ctypes.Structure):
    """Mirror of nof_view_desc (include/nof.h): the camera and march settings of nof_render_view."""
    _fields_ = [("c2w", _f32 * 16), ("K", _f32 * 9), ("H", _i32), ("W", _i32), ("pixels", _p), ("n", _i32),
                ("pixel0", _i32), ("step", _f32), ("max_steps", _i32), ("n_refine", _i32), ("frame_id", _i32),
                ("n_frames", _i32), ("occ_n", _i32), ("occ", _p)]


class ViewOut(ctypes.Structure):
    """Mirror of nof_view_out (include/nof.h): the outputs of nof_render_view."""
    _fields_ = [("t", _p), ("depth", _p), ("normal", _p), ("rgb", _p), ("hit", _p), ("index", _p), ("tiles", _p),
                ("workspace", _p)]


MESH_COLOUR_FLAT, MESH_COLOUR_VERTEX, MESH_COLOUR_TEXTURE = 0, 1, 2   # NOF_MESH_COLOUR_*


class MeshRenderDesc(ctypes.Structure):
    """Mirror of nof_mesh_render_desc (include/nof.h): the mesh, poses, camera and outputs of nof_render_mesh."""
    _d = ctypes.c_double
    _fields_ = [("vertices", _p), ("faces", _p), ("n_vertices", _i64), ("n_faces", _i64), ("colors", _p),
                ("normals", _p), ("uv", _p), ("texture", _p), ("tex_h", _i32), ("tex_w", _i32), ("ob_in_cam", _p),
                ("K", _p), ("B", _i32), ("H", _i32), ("W", _i32), ("znear", _d), ("zfar", _d), ("colour_mode", _i32),
                ("shade", _i32), ("base_rgb", ctypes.c_uint8 * 4), ("small_max_pixels", _i32), ("workspace", _p),
                ("depth", _p), ("face", _p), ("rgb", _p), ("normal", _p)]


class RansacDesc(ctypes.Structure):
    """Mirror of nof_ransac_desc (include/nof.h): the correspondences, settings and outputs of nof_ransac_pairs."""
    _d = ctypes.c_double
    _fields_ = [("pts_a", _p), ("pts_b", _p), ("normals_a", _p), ("normals_b", _p), ("conf", _p), ("pair_start", _p),
                ("max_trans_sq", _p), ("min_trace", _p), ("M", _i64), ("P", _i32), ("n_trials", _i32), ("seed", _u32),
                ("min_inliers", _i32), ("inlier_dist_sq", _d), ("cos_normal", _d), ("workspace", _p),
                ("workspace_bytes", ctypes.c_size_t), ("best_trial", _p), ("score", _p), ("pose", _p),
                ("n_inliers", _p), ("inlier", _p), ("sums", _p), ("trial_idx", _p), ("trial_pose", _p),
                ("trial_live", _p), ("trial_score", _p)]


class PoseGraphDesc(ctypes.Structure):
    """Mirror of nof_pose_graph_desc (include/nof.h): the poses, both terms, settings and outputs of
    nof_pose_graph_optimize."""
    _d = ctypes.c_double
    _fields_ = [("poses", _p), ("fixed", _p), ("N", _i32), ("n_outer", _i32), ("n_inner", _i32), ("P", _i32),
                ("M", _i64), ("pair_frames", _p), ("pts_a", _p), ("pts_b", _p), ("pair_start", _p), ("weight", _p),
                ("points", _p), ("normals", _p), ("H", _i32), ("W", _i32), ("radius", _i32), ("reserved", _i32),
                ("fx", _d), ("fy", _d), ("cx", _d), ("cy", _d), ("robust_delta", _d), ("w_sparse", _d),
                ("w_dense", _d), ("dist_thresh", _d), ("normal_thresh", _d), ("depth_min", _d), ("depth_max", _d),
                ("min_trace", _d), ("workspace", _p), ("workspace_bytes", ctypes.c_size_t), ("poses_out", _p),
                ("history", _p), ("iter_poses", _p), ("dbg_A", _p), ("dbg_g", _p), ("dbg_delta", _p),
                ("dense_index", _p)]


class FrameErodeDesc(ctypes.Structure):
    """Mirror of nof_frame_erode_desc (include/nof.h)."""
    _d = ctypes.c_double
    _fields_ = [("in_", _p), ("out", _p), ("N", _i32), ("H", _i32), ("W", _i32), ("radius", _i32), ("depth_min", _d),
                ("zfar", _d), ("diff", _d), ("ratio", _d)]


class FrameBilateralDesc(ctypes.Structure):
    """Mirror of nof_frame_bilateral_desc (include/nof.h)."""
    _d = ctypes.c_double
    _fields_ = [("in_", _p), ("out", _p), ("N", _i32), ("H", _i32), ("W", _i32), ("radius", _i32), ("depth_min", _d),
                ("zfar", _d), ("two_sigma_d_sq", _d), ("two_sigma_r_sq", _d), ("band", _d)]


class FrameGeometryDesc(ctypes.Structure):
    """Mirror of nof_frame_geometry_desc (include/nof.h)."""
    _d = ctypes.c_double
    _fields_ = [("depth_in", _p), ("K", _p), ("mask", _p), ("N", _i32), ("H", _i32), ("W", _i32), ("reserved", _i32),
                ("depth_min", _d), ("z_diff", _d), ("sin_edge", _d), ("depth", _p), ("points", _p), ("normals", _p),
                ("n_valid", _p)]


class FrameLiftDesc(ctypes.Structure):
    """Mirror of nof_frame_lift_desc (include/nof.h)."""
    _d = ctypes.c_double
    _fields_ = [("points", _p), ("normals", _p), ("N", _i32), ("H", _i32), ("W", _i32), ("P", _i32), ("M", _i64),
                ("pair_frames", _p), ("pair_start", _p), ("uv_a", _p), ("uv_b", _p), ("poses", _p), ("depth_min", _d),
                ("max_dist", _d), ("cos_normal", _d), ("gate_dist", _i32), ("gate_normal", _i32), ("pts_a", _p),
                ("pts_b", _p), ("normals_a", _p), ("normals_b", _p), ("valid", _p)]


class FrameCovisDesc(ctypes.Structure):
    """Mirror of nof_frame_covis_desc (include/nof.h)."""
    _d = ctypes.c_double
    _fields_ = [("points", _p), ("normals", _p), ("N", _i32), ("H", _i32), ("W", _i32), ("Q", _i32), ("pairs", _p),
                ("T", _p), ("stride", _i32), ("reserved", _i32), ("depth_min", _d), ("cos_visible", _d), ("counts", _p)]


class MatchDesc(ctypes.Structure):
    """Mirror of nof_match_desc (include/nof.h): the descriptors, settings and outputs of nof_match_descriptors."""
    _fields_ = [("desc_a", _p), ("desc_b", _p), ("valid_a", _p), ("valid_b", _p), ("P", _i32), ("L", _i32), ("S", _i32),
                ("C", _i32), ("h0", _i32), ("w0", _i32), ("h1", _i32), ("w1", _i32), ("border_rm", _i32),
                ("reserved", _i32), ("temperature", _f32), ("thr", _f32), ("workspace", _p),
                ("workspace_bytes", ctypes.c_size_t), ("j_of_i", _p), ("conf", _p), ("n_matches", _p), ("row_max", _p),
                ("row_sum", _p), ("col_max", _p), ("col_sum", _p)]


FT_SELF, FT_CROSS, FT_MAX_LAYERS = 0, 1, 16   # NOF_FT_*


class FeatureTransformerDesc(ctypes.Structure):
    """Mirror of nof_feature_transformer_desc (include/nof.h): the streams, masks, layers and weights of
    nof_feature_transformer."""
    _fields_ = [("feat_a", _p), ("feat_b", _p), ("mask_a", _p), ("mask_b", _p), ("P", _i32), ("L", _i32), ("S", _i32),
                ("C", _i32), ("n_layers", _i32), ("layer_kind", _i32 * FT_MAX_LAYERS), ("reserved", _i32),
                ("weights", _p), ("weights_bytes", ctypes.c_size_t), ("workspace", _p),
                ("workspace_bytes", ctypes.c_size_t)]


class FineWindowsDesc(ctypes.Structure):
    """Mirror of nof_fine_windows_desc (include/nof.h): the maps, matches, weights and outputs of nof_fine_windows."""
    _fields_ = [("fine_a", _p), ("fine_b", _p), ("coarse_a", _p), ("coarse_b", _p), ("frames_a", _p), ("frames_b", _p),
                ("pair", _p), ("i", _p), ("j", _p), ("M", _i32), ("P", _i32), ("N_a", _i32), ("N_b", _i32), ("h0", _i32),
                ("w0", _i32), ("h1", _i32), ("w1", _i32), ("stride", _i32), ("reserved", _i32), ("weights", _p),
                ("weights_bytes", ctypes.c_size_t), ("context", _p), ("win_a", _p), ("win_b", _p)]


class FineExpectationDesc(ctypes.Structure):
    """Mirror of nof_fine_expectation_desc (include/nof.h)."""
    _fields_ = [("win_a", _p), ("win_b", _p), ("pair", _p), ("i", _p), ("j", _p), ("M", _i32), ("P", _i32), ("L", _i32),
                ("S", _i32), ("expec", _p)]


class StepParams(ctypes.Structure):
    """Mirror of nof_step_params (include/nof.h): the device step block."""
    _fields_ = [("lr0", ctypes.c_double), ("lr1", ctypes.c_double), ("trunc", _f32), ("seed", _u32),
                ("batch_seed", _u32), ("step", _i32)]


class ScheduleDesc(ctypes.Structure):
    """Mirror of nof_schedule_desc (include/nof.h)."""
    _d = ctypes.c_double
    _fields_ = [("lrate", _d), ("lrate_pose", _d), ("decay_rate", _d), ("trunc", _d), ("trunc_start", _d),
                ("sc_factor", _d), ("trunc_decay", _i32), ("n_step", _i32), ("seed_base", _u32),
                ("batch_seed_base", _u32)]


class RayPoolDesc(ctypes.Structure):
    """Mirror of nof_ray_pool_desc (include/nof.h)."""
    _d = ctypes.c_double
    _fields_ = [("rgb", _p), ("depth", _p), ("mask", _p), ("occ_mask", _p), ("cam_in_world", _p), ("F", _i32),
                ("H", _i32), ("W", _i32), ("first_frame_id", _i32), ("dilate_first", _i32), ("dilate_other", _i32),
                ("fx", _f32), ("fy", _f32), ("cx", _f32), ("cy", _f32), ("near_sc", _f32), ("far_sc", _f32),
                ("far_sc64", _d), ("bbox", _d * 6), ("occ", _p), ("occ_n", _i32), ("cell_start", _p),
                ("cell_points", _p), ("grid_origin", _d * 3), ("grid_dims", _i32 * 3), ("grid_cell", _d),
                ("grid_radius", _d), ("workspace", _p), ("rays", _p), ("n_out", _p)]


def declared_symbols():
    return list(_SIGNATURES)


def check_field_desc_layout(L, struct=FieldDesc):
    """Raise unless library L was built from the nof_field_desc that `struct` mirrors: a library
    from another header (NOF_LIB, a stale libnof_prev.so / libnof_ablate.so) would read the
    descriptor's pointers from the wrong offsets."""
    fn = getattr(L, "nof_field_desc_size", None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} does not export nof_field_desc_size: it predates this binding's "
                           f"nof_field_desc ({ctypes.sizeof(struct)} bytes) — rebuild it")
    fn.argtypes, fn.restype = _SIGNATURES["nof_field_desc_size"]
    if fn() != ctypes.sizeof(struct):
        raise RuntimeError(f"{LIB_PATH}: nof_field_desc is {fn()} bytes in the library, {ctypes.sizeof(struct)} "
                           "in this binding — rebuild the library from the current include/nof.h")


def lib():
    """Load libnof.so once; raise if it is missing (no fallback) or built from another
    nof_field_desc than FieldDesc mirrors."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m bundlesdf_amd.build` "
                               "(the HIP path has no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        check_field_desc_layout(L)
        for name, (args, res) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _LIB = L
    return _LIB


def check(rc, what=""):
    if rc != 0:
        msg = lib().nof_last_error().decode(errors="replace")
        raise RuntimeError(f"{what}: {msg}" if what else msg)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream_of(t):
    """Current HIP stream of tensor t's device (graph-capture safe)."""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def require_device(t, name):
    if not (t.is_cuda):
        raise RuntimeError(f"{name} must be a CUDA tensor")


def require_contiguous(t, name):
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")
