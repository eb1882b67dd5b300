"""ctypes binding of libdfusion_hip.so (include/dfusion_hip.h).

There is deliberately NO fallback: if the library is missing or a call fails, the caller
gets an exception.  Build with `python -m dynamicfusion_body_amd.build`.
"""
import ctypes
import os
import re

_PKG = os.path.dirname(os.path.abspath(__file__))
# DFH_LIB_PATH: an alternative build of the SAME library (kernel experiments, tools/build_variant.sh) -- not a fallback
LIB_PATH = os.environ.get("DFH_LIB_PATH") or os.path.join(_PKG, "libdfusion_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "dfusion_hip.h")

F32, F64 = 0, 1
ABI_VERSION = 8

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int_p = ctypes.POINTER(ctypes.c_int)
_vp = ctypes.c_void_p
_int = ctypes.c_int
_dbl = ctypes.c_double


class Problem(ctypes.Structure):
    """dfh_gn_problem (include/dfusion_hip.h): what the solver owns."""
    _fields_ = [("sample_pos", _vp), ("sample_nrm", _vp), ("nbr", _vp), ("weights", _vp), ("corr", _vp), ("valid", _vp),
                ("n_samples", _int), ("knn", _int),
                ("node_dq", _vp), ("node_pos", _vp), ("node_w", _vp), ("node_nbr", _vp), ("n_nodes", _int),
                ("lw_dq", _dbl * 8), ("rw", _dbl), ("huber_delta", _dbl),
                ("row_ptr", _vp), ("col", _vp), ("n_blocks", _int), ("vals", _vp), ("rhs", _vp), ("cost_count", _vp),
                ("blk_upper", _vp), ("n_upper", _int),
                ("run_id", _vp), ("n_rows", _int), ("partial", _vp), ("blk_ptr", _vp), ("blk_ent", _vp), ("node_ptr", _vp),
                ("node_ent", _vp),
                ("partial_reg", _vp), ("rblk_ptr", _vp), ("rblk_ent", _vp), ("rnode_ptr", _vp), ("rnode_ent", _vp)]


class Frame(ctypes.Structure):
    """dfh_gn_frame: the live frame the data term is associated against (always a packed views table)."""
    _fields_ = [("views", _vp), ("n_views", _int), ("depth_dtype", _int), ("H", _int), ("W", _int),
                ("K", _dbl * 9), ("Kinv", _dbl * 9), ("scale", _dbl), ("center", _dbl * 3), ("half", _dbl), ("max_dist", _dbl)]


class SolveParams(ctypes.Structure):
    """dfh_gn_solve_params: one dfh_gn_solve call's schedule."""
    _fields_ = [("pcg_iters", _int), ("lm_abs", _dbl), ("lm_rel", _dbl), ("x_out", _vp), ("pcg_workspace", _vp),
                ("pcg_workspace_bytes", ctypes.c_size_t), ("step", _dbl), ("n_iters", _int), ("n_global", _int),
                ("global_lm", _dbl), ("global_xi_out", _vp), ("global_scratch", _vp), ("global_scratch_bytes", ctypes.c_size_t)]


class Slab(ctypes.Structure):
    """dfh_slab: planes [x0, x1) of a res grid."""
    _fields_ = [("res", _int * 3), ("x0", _int), ("x1", _int)]


class Volume(ctypes.Structure):
    """dfh_volume: the TSDF / weight pair on a slab."""
    _fields_ = [("tsdf", _vp), ("tsdf_w", _vp), ("dtype", _int), ("slab", Slab)]


class Live(ctypes.Structure):
    """dfh_live: the whole live volume."""
    _fields_ = [("data", _vp), ("dtype", _int), ("res", _int * 3)]


class VolumeTerm(ctypes.Structure):
    """dfh_gn_volume_term: the live TSDF volume the data term is associated against, and the term's settings."""
    _fields_ = [("live", Live), ("value_to_vox", _dbl), ("band", _dbl), ("max_dist", _dbl), ("min_grad", _dbl)]


class DepthViews(ctypes.Structure):
    """dfh_depth_views: n_views depth maps of one size through one camera (depth, lw: host arrays the caller keeps alive)."""
    _fields_ = [("n_views", _int), ("depth", ctypes.POINTER(_vp)), ("depth_dtype", _int), ("H", _int), ("W", _int),
                ("K", _dbl * 9), ("Kinv", _dbl * 9), ("lw", _c_double_p), ("scale", _dbl), ("center", _dbl * 3), ("tsdf_res", _int)]


class Nodes(ctypes.Structure):
    """dfh_nodes: the deformation graph's nodes as K3 reads them."""
    _fields_ = [("pos", _vp), ("dq", _vp), ("w", _vp), ("n_nodes", _int), ("knn", _int)]


class ColorVolume(ctypes.Structure):
    """dfh_color_volume: the float32 (r, g, b, wc) packs of a slab."""
    _fields_ = [("rgbw", _vp), ("slab", Slab)]


class DepthPrepParams(ctypes.Structure):
    """dfh_depth_prep_params: the maps, camera, filter tables and thresholds of one dfh_depth_prep call (depth: a host array the
    caller keeps alive; spatial, range_lut: device float32)."""
    _fields_ = [("n_views", _int), ("depth", ctypes.POINTER(_vp)), ("depth_dtype", _int), ("H", _int), ("W", _int),
                ("Kinv", _dbl * 9), ("radius", _int), ("spatial", _vp), ("range_lut", _vp), ("n_lut", _int),
                ("range_scale", _dbl), ("max_jump", _dbl), ("min_cos", _dbl), ("mask", _int)]


class NormalGate(ctypes.Structure):
    """dfh_gn_normal_gate: the live normal maps ((V, H, W, 3) float32, device) and the smallest compatible cosine."""
    _fields_ = [("normals", _vp), ("min_cos", _dbl)]


class Landmarks(ctypes.Structure):
    """dfh_gn_landmarks: the point-to-point landmark term -- landmarks sorted by node tuple, their plan and the term's settings."""
    _fields_ = [("pos", _vp), ("nbr", _vp), ("weights", _vp), ("target", _vp), ("valid", _vp), ("conf", _vp), ("n", _int),
                ("weight", _dbl), ("huber_delta", _dbl), ("max_dist", _dbl),
                ("run_id", _vp), ("n_rows", _int), ("partial", _vp), ("blk_ptr", _vp), ("blk_ent", _vp), ("node_ptr", _vp),
                ("node_ent", _vp), ("active_out", _vp)]


class Photometric(ctypes.Structure):
    """dfh_gn_photometric: the colour-consistency term -- samples sorted by node tuple with reference intensities, the views' colour
    images (a host array of device pointers), their plan and the term's settings."""
    _fields_ = [("pos", _vp), ("nbr", _vp), ("weights", _vp), ("ref", _vp), ("valid", _vp), ("conf", _vp), ("n", _int),
                ("weight", _dbl), ("huber_delta", _dbl), ("max_diff", _dbl), ("band_sd", _dbl), ("color", _vp),
                ("run_id", _vp), ("n_rows", _int), ("partial", _vp), ("blk_ptr", _vp), ("blk_ent", _vp), ("node_ptr", _vp),
                ("node_ent", _vp), ("active_out", _vp), ("view_out", _vp), ("resid_out", _vp)]


class RGBDView(ctypes.Structure):
    """dfh_rgbd_view: one view's calibration for dfh_rgbd_ingest -- raw depth camera, colour camera, depth -> colour transform."""
    _fields_ = [("fd", _dbl * 4), ("kd", _dbl * 5), ("fc", _dbl * 4), ("kc", _dbl * 5), ("T_dc", _dbl * 12)]


class RGBDIngestParams(ctypes.Structure):
    """dfh_rgbd_ingest_params: the raw maps and images (host arrays of device pointers the caller keeps alive), the output
    pinhole, the decode range, the occlusion test's settings and the views' calibration (a host array)."""
    _fields_ = [("n_views", _int), ("raw_depth", ctypes.POINTER(_vp)), ("raw_color", ctypes.POINTER(_vp)),
                ("Hd", _int), ("Wd", _int), ("Hc", _int), ("Wc", _int), ("C", _int),
                ("fx", _dbl), ("fy", _dbl), ("cx", _dbl), ("cy", _dbl), ("depth_scale", _dbl), ("z_min", _dbl), ("z_max", _dbl),
                ("occl_tol", _dbl), ("max_splat", _int), ("sample", _int), ("views", ctypes.POINTER(RGBDView))]


class RaycastParams(ctypes.Structure):
    """dfh_raycast_params: the volume (and colour volume), the views (lw, wl: host arrays the caller keeps alive), the march's
    settings, the brick table and the device outputs of one dfh_raycast call."""
    _fields_ = [("vol", ctypes.POINTER(Volume)), ("colors", ctypes.POINTER(ColorVolume)), ("n_views", _int), ("H", _int), ("W", _int),
                ("K", _dbl * 9), ("Kinv", _dbl * 9), ("lw", _c_double_p), ("wl", _c_double_p),
                ("scale", _dbl), ("center", _dbl * 3), ("half", _dbl), ("z_near", _dbl), ("z_far", _dbl), ("step", _dbl),
                ("min_weight", _dbl), ("refine", _int), ("max_steps", _int), ("table", _vp), ("table_bytes", ctypes.c_size_t),
                ("depth", _vp), ("normals", _vp), ("color", _vp), ("hit", _vp)]


class IcpTrackParams(ctypes.Structure):
    """dfh_icp_track_params: the live and model maps of one pyramid level (device float32), the level's camera, the poses T
    (device, in and out), the gates, the solve's guards and the device outputs of one dfh_icp_track call."""
    _fields_ = [("n_views", _int), ("H", _int), ("W", _int), ("live_depth", _vp), ("live_normals", _vp), ("model_depth", _vp),
                ("model_normals", _vp), ("K", _dbl * 9), ("Kinv", _dbl * 9), ("T", _vp), ("max_dist", _dbl), ("min_cos", _dbl),
                ("huber", _dbl), ("lm_rel", _dbl), ("n_iters", _int), ("min_count", _int), ("max_rot", _dbl), ("max_trans", _dbl),
                ("stats", _vp), ("rows", _vp), ("scratch", _vp), ("scratch_bytes", ctypes.c_size_t)]


class MeshSdfLayout(ctypes.Structure):
    """dfh_mesh_sdf_layout: the cell table's geometry and size, filled by dfh_mesh_sdf_plan."""
    _fields_ = [("lo", _dbl * 3), ("hi", _dbl * 3), ("cell", _dbl), ("maxabs", _dbl), ("dims", _int * 3),
                ("n_verts", ctypes.c_long), ("n_faces", ctypes.c_long), ("n_entries", ctypes.c_long), ("bytes", ctypes.c_size_t)]


class MeshSdf(ctypes.Structure):
    """dfh_mesh_sdf: a mesh on the device with its pseudonormal tables and its cell table."""
    _fields_ = [("verts", _vp), ("faces", _vp), ("keep", _vp), ("face_normals", _vp), ("edge_normals", _vp), ("vertex_normals", _vp),
                ("n_verts", ctypes.c_long), ("n_faces", ctypes.c_long), ("table", _vp), ("table_bytes", ctypes.c_size_t),
                ("layout", MeshSdfLayout)]


class MeshSdfGridParams(ctypes.Structure):
    """dfh_mesh_sdf_grid_params: the grid, the band and the device outputs of one dfh_mesh_sdf_grid call."""
    _fields_ = [("origin", _dbl * 3), ("spacing", _dbl * 3), ("shape", _int * 3), ("band", _dbl), ("orientation", _int), ("dtype", _int),
                ("value", _vp), ("status", _vp), ("closest", _vp), ("face", _vp)]


_problem_p = ctypes.POINTER(Problem)
_frame_p = ctypes.POINTER(Frame)
_slab_p = ctypes.POINTER(Slab)
_volume_p = ctypes.POINTER(Volume)
_term_p = ctypes.POINTER(VolumeTerm)
_gate_p = ctypes.POINTER(NormalGate)
_landmarks_p = ctypes.POINTER(Landmarks)
_photo_p = ctypes.POINTER(Photometric)
STRUCTS = {"dfh_gn_problem": Problem, "dfh_gn_frame": Frame, "dfh_gn_solve_params": SolveParams, "dfh_slab": Slab,
           "dfh_volume": Volume, "dfh_live": Live, "dfh_depth_views": DepthViews, "dfh_nodes": Nodes,
           "dfh_gn_volume_term": VolumeTerm, "dfh_depth_prep_params": DepthPrepParams,
           "dfh_gn_normal_gate": NormalGate, "dfh_gn_landmarks": Landmarks, "dfh_color_volume": ColorVolume,
           "dfh_gn_photometric": Photometric, "dfh_rgbd_view": RGBDView, "dfh_rgbd_ingest_params": RGBDIngestParams,
           "dfh_raycast_params": RaycastParams, "dfh_icp_track_params": IcpTrackParams,
           "dfh_mesh_sdf_layout": MeshSdfLayout, "dfh_mesh_sdf": MeshSdf, "dfh_mesh_sdf_grid_params": MeshSdfGridParams}

_SIGNATURES = {
    "dfh_version": (_int, []),
    "dfh_last_error": (ctypes.c_char_p, []),
    "dfh_stream_synchronize": (_int, [_vp]),
    "dfh_set_option": (_int, [ctypes.c_char_p, ctypes.c_long]),
    "dfh_get_option": (ctypes.c_long, [ctypes.c_char_p]),
    "dfh_integrate_workspace_bytes": (ctypes.c_size_t, [_int, _int, _int, _slab_p]),
    "dfh_integrate_multi_workspace_bytes": (ctypes.c_size_t, [_int]),
    "dfh_integrate_depth": (_int, [_volume_p, ctypes.POINTER(DepthViews), _dbl, _dbl, _c_double_p, _vp, ctypes.c_size_t, _vp]),
    "dfh_integrate_depth_path": (_int, [_int, _slab_p, _int, _int, _int]),
    "dfh_integrate_depth_ocl": (_int, [_volume_p, _vp, _int, _int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.c_float, ctypes.c_float, _vp]),
    "dfh_fuse_volume_rigid": (_int, [_volume_p, ctypes.POINTER(Live), _c_double_p, _dbl, _dbl, _vp]),
    "dfh_dqb_workspace_bytes": (ctypes.c_size_t, [_slab_p]),
    "dfh_dqb_workspace_bytes_cached": (ctypes.c_size_t, [_slab_p, _int, _int, _int]),
    "dfh_fuse_volume_dqb": (_int, [_volume_p, ctypes.POINTER(Live), ctypes.POINTER(Nodes), _c_double_p, _dbl, _dbl, _vp, ctypes.c_size_t, _int, _vp]),
    "dfh_integrate_depth_dqb": (_int, [_volume_p, ctypes.POINTER(DepthViews), ctypes.POINTER(Nodes), _c_double_p, _dbl, _dbl, _int, _vp,
                                      ctypes.c_size_t, _int, _vp]),
    "dfh_residual_rigid": (_int, [_vp, _vp, _vp, _int, _c_double_p, _vp, _vp]),
    "dfh_gn_build_rigid": (_int, [_vp, _vp, _vp, _vp, _int, _c_double_p, _vp, _vp]),
    "dfh_residual_data": (_int, [_vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _int, _c_double_p, _vp, _vp]),
    "dfh_residual_reg": (_int, [_vp, _int, _int, _vp, _vp, _vp, _dbl, _vp, _vp]),
    "dfh_warp_points": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _int, _c_double_p, _vp, _vp, _vp]),
    "dfh_closest_correspondences": (_int, [_vp, _vp, _int, _vp, _int, _int, _dbl, _vp, _vp, _vp, _vp]),
    "dfh_nearest_points": (_int, [_vp, _int, _vp, _int, _vp, _vp, _vp]),
    "dfh_graph_unsupported": (_int, [_vp, _int, _vp, _int, _vp, _vp, _int, _vp, _vp]),
    "dfh_dq_blend_points": (_int, [_vp, _int, _vp, _int, _vp, _vp, _vp, _int, _vp, _vp]),
    "dfh_radius_sample_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long]),
    "dfh_radius_sample": (_int, [_vp, ctypes.c_long, _dbl, _vp, ctypes.c_long, ctypes.POINTER(ctypes.c_long), _c_int_p, _vp,
                                 ctypes.c_size_t, _vp]),
    "dfh_sample_knn": (_int, [_vp, _int, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    "dfh_dqb_skip_layout": (_int, [_slab_p, _c_int_p, _int, _int, ctypes.POINTER(ctypes.c_size_t)]),
    "dfh_dqb_build_candidates": (_int, [_slab_p, _vp, _int, _int, _vp, ctypes.c_size_t, _vp]),
    "dfh_sample_knn_bricks": (_int, [_vp, _int, _vp, _vp, _int, _int, _slab_p, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "dfh_permute_samples": (_int, [_vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dfh_gn_partial_doubles": (ctypes.c_size_t, [_int]),
    "dfh_gn_views_bytes": (ctypes.c_size_t, [_int, _int, _int, _int]),
    "dfh_gn_pack_views": (_int, [_vp, _int, ctypes.POINTER(ctypes.c_void_p), _int, _int, _int, _c_double_p, _vp]),
    "dfh_gn_associate": (_int, [_problem_p, _frame_p, _vp]),
    "dfh_gn_associate_volume": (_int, [_problem_p, _term_p, _vp]),
    "dfh_gn_build": (_int, [_problem_p, _frame_p, _vp]),
    "dfh_gn_build_volume": (_int, [_problem_p, _term_p, _vp]),
    "dfh_gn_solve": (_int, [_problem_p, _frame_p, ctypes.POINTER(SolveParams), _vp]),
    "dfh_gn_solve_volume": (_int, [_problem_p, _term_p, ctypes.POINTER(SolveParams), _vp]),
    "dfh_gn_associate_gated": (_int, [_problem_p, _frame_p, _gate_p, _vp]),
    "dfh_gn_build_gated": (_int, [_problem_p, _frame_p, _gate_p, _vp]),
    "dfh_gn_solve_gated": (_int, [_problem_p, _frame_p, _gate_p, ctypes.POINTER(SolveParams), _vp]),
    "dfh_gn_add_landmarks": (_int, [_problem_p, _landmarks_p, _vp]),
    "dfh_gn_solve_landmarks": (_int, [_problem_p, _frame_p, _landmarks_p, ctypes.POINTER(SolveParams), _vp]),
    "dfh_gn_add_photometric": (_int, [_problem_p, _frame_p, _photo_p, _vp]),
    "dfh_gn_solve_photometric": (_int, [_problem_p, _frame_p, _landmarks_p, _photo_p, ctypes.POINTER(SolveParams), _vp]),
    "dfh_gn_global_sampled_gated": (_int, [_problem_p, _frame_p, _gate_p, _int, _dbl, _int, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_gn_pack_upper": (_int, [_vp, _vp, _vp, _vp, _int, _int, _int, _vp, _vp]),
    "dfh_gn_unpack_upper": (_int, [_vp, _vp, _vp, _vp, _int, _int, _int, _vp, _vp]),
    "dfh_gn_sort_workspace_bytes": (ctypes.c_size_t, [_int]),
    "dfh_gn_sort_samples": (_int, [_vp, _vp, _vp, _vp, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_gn_tile_samples": (_int, []),
    "dfh_gn_plan_count": (_int, [_vp, _int, _int, _vp, _vp, _vp]),
    "dfh_gn_plan_workspace_bytes": (ctypes.c_size_t, [_int, _int]),
    "dfh_gn_plan_build": (_int, [_vp, _int, _int, _int, _vp, _int, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                 ctypes.c_size_t, _vp]),
    "dfh_pcg_workspace_bytes": (ctypes.c_size_t, [_int, _int]),
    "dfh_pcg_solve": (_int, [_vp, _vp, _vp, _vp, _int, _int, _dbl, _dbl, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_pcg_solve_update": (_int, [_vp, _vp, _vp, _vp, _int, _int, _dbl, _dbl, _vp, _vp, ctypes.c_size_t, _vp, _dbl, _vp]),
    "dfh_pcg_set_mode": (_int, [_int]),
    "dfh_pcg_path": (_int, [_int]),
    "dfh_pcg_status": (_int, [_vp, ctypes.POINTER(ctypes.c_long)]),
    "dfh_pcg_status_peek": (_int, [_vp, ctypes.POINTER(ctypes.c_long)]),
    "dfh_apply_twist": (_int, [_vp, _vp, _int, _dbl, _vp]),
    "dfh_relax_twists": (_int, [_vp, _int, _dbl, _vp]),
    "dfh_gn_global_sampled_bytes": (ctypes.c_size_t, [_int, _int]),
    "dfh_gn_global_sampled": (_int, [_problem_p, _frame_p, _int, _dbl, _int, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_gn_global_sampled_volume": (_int, [_problem_p, _term_p, _int, _dbl, _int, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_gn_global_apply": (_int, [_vp, _dbl, _int, _vp, _vp, _vp]),
    "dfh_gn_global_step_bytes": (ctypes.c_size_t, []),
    "dfh_gn_global_step": (_int, [_vp, _int, _vp, _int, _dbl, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_surface_workspace_bytes": (ctypes.c_size_t, [_c_int_p]),
    "dfh_surface_count": (_int, [_vp, _vp, _int, _c_int_p, _dbl, _vp, ctypes.c_size_t, _vp, _vp]),
    "dfh_surface_emit": (_int, [_vp, _vp, _int, _c_int_p, _int, _dbl, _vp, _vp, _vp, ctypes.c_long, _vp]),
    "dfh_mc_workspace_bytes": (ctypes.c_size_t, [_c_int_p, _int]),
    "dfh_mc_count": (_int, [_vp, _int, _c_int_p, _int, _dbl, _vp, ctypes.c_size_t, _vp, _vp]),
    "dfh_mc_emit": (_int, [_vp, _int, _c_int_p, _int, _dbl, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp, ctypes.c_long, ctypes.c_long,
                           ctypes.c_long, _vp]),
    "dfh_mc_reorder_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long, ctypes.c_long]),
    "dfh_mc_reorder": (_int, [_vp, _vp, _vp, _vp, ctypes.c_long, ctypes.c_long, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_render_workspace_bytes": (ctypes.c_size_t, [_int, _int, _int, ctypes.c_long]),
    "dfh_render_raster": (_int, [_vp, ctypes.c_long, _vp, ctypes.c_long, _int, _c_double_p, _c_double_p, _int, _int, _dbl, _c_double_p,
                                 _dbl, _dbl, _vp, ctypes.c_size_t, _vp]),
    "dfh_render_resolve": (_int, [_vp, _vp, ctypes.c_long, _vp, ctypes.c_long, _int, _c_double_p, _c_double_p, _int, _int, _dbl,
                                  _c_double_p, _dbl, _dbl, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp]),
    "dfh_render_samples_workspace_bytes": (ctypes.c_size_t, [_int, _int, _int, _int]),
    "dfh_render_samples_count": (_int, [_int, _int, _int, ctypes.c_long, _int, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, _vp]),
    "dfh_render_samples_emit": (_int, [_vp, _vp, _vp, ctypes.c_long, _vp, ctypes.c_long, _int, _c_double_p, _c_double_p, _int, _int, _dbl,
                                       _c_double_p, _dbl, _dbl, _int, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, _vp, _vp,
                                       ctypes.c_long, _vp]),
    "dfh_depth_prep": (_int, [ctypes.POINTER(DepthPrepParams), _vp, _vp, _vp]),
    "dfh_depth_prep_tile": (_int, [_c_int_p]),
    "dfh_nearest_descriptors_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long, ctypes.c_long, _int]),
    "dfh_nearest_descriptors_path": (_int, [ctypes.c_long, ctypes.c_long, _int]),
    "dfh_nearest_descriptors": (_int, [_vp, ctypes.c_long, _vp, ctypes.c_long, _int, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_nearest_descriptors_tile": (_int, [_c_int_p]),
    "dfh_render_vertex_ids": (_int, [_vp, ctypes.c_long, _vp, ctypes.c_long, _int, _c_double_p, _c_double_p, _int, _int, _dbl, _c_double_p,
                                     _dbl, _dbl, _vp, ctypes.c_size_t, _dbl, _dbl, _vp, _vp, _vp]),
    "dfh_pool_features_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long, ctypes.c_long]),
    "dfh_pool_features": (_int, [_vp, _vp, ctypes.c_long, _int, ctypes.c_long, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_pool_features_tile": (_int, [_c_int_p]),
    "dfh_integrate_color": (_int, [ctypes.POINTER(ColorVolume), _volume_p, ctypes.POINTER(DepthViews), ctypes.POINTER(_vp),
                                   ctypes.POINTER(Nodes), _c_double_p, _dbl, _dbl, _dbl, _dbl, _vp, ctypes.c_size_t, _int, _vp]),
    "dfh_sample_colors": (_int, [ctypes.POINTER(ColorVolume), _vp, ctypes.c_long, _vp, _vp, _vp]),
    "dfh_rgbd_ingest": (_int, [ctypes.POINTER(RGBDIngestParams), _vp, _vp, _vp, _vp, _vp]),
    "dfh_rgbd_ingest_workspace_bytes": (ctypes.c_size_t, [_int, _int, _int]),
    "dfh_rgbd_ingest_tile": (_int, [_c_int_p]),
    "dfh_raycast_table_bytes": (ctypes.c_size_t, [_slab_p]),
    "dfh_raycast_table": (_int, [_volume_p, _vp, _vp]),
    "dfh_raycast": (_int, [ctypes.POINTER(RaycastParams), _vp]),
    "dfh_depth_halve": (_int, [ctypes.POINTER(_vp), _int, _int, _int, _int, _dbl, _vp, _vp]),
    "dfh_icp_track_bytes": (ctypes.c_size_t, [_int]),
    "dfh_icp_track": (_int, [ctypes.POINTER(IcpTrackParams), _vp]),
    "dfh_mesh_sdf_chunk": (_int, []),
    "dfh_mesh_sdf_plan": (_int, [_vp, ctypes.c_long, _vp, _vp, ctypes.c_long, _dbl, ctypes.POINTER(MeshSdfLayout)]),
    "dfh_mesh_sdf_build": (_int, [ctypes.POINTER(MeshSdf), _vp]),
    "dfh_mesh_sdf_points": (_int, [ctypes.POINTER(MeshSdf), _vp, ctypes.c_long, _dbl, _int, _vp, _vp, _vp, _vp]),
    "dfh_mesh_sdf_grid": (_int, [ctypes.POINTER(MeshSdf), ctypes.POINTER(MeshSdfGridParams), _vp]),
    "dfh_mesh_components_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long, ctypes.c_long]),
    "dfh_mesh_components": (_int, [_vp, ctypes.c_long, ctypes.c_long, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_long), _vp, ctypes.c_size_t, _vp]),
    "dfh_mesh_component_table": (_int, [_vp, _int, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp, _vp, ctypes.c_long, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp, ctypes.c_size_t, _vp]),
    "dfh_mesh_compact": (_int, [_vp, ctypes.c_long, ctypes.c_long, _vp, _vp, _vp, ctypes.c_long, _int, _vp, _vp, _vp,
                                ctypes.POINTER(ctypes.c_long), _vp, ctypes.c_size_t, _vp]),
    "dfh_mesh_simplify_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long, ctypes.c_long]),
    "dfh_mesh_simplify_keys": (_int, [_vp, _int, ctypes.c_long, _vp, ctypes.c_long, _dbl, _c_double_p, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_mesh_simplify_group": (_int, [_vp, _vp, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_long), _vp,
                                       ctypes.c_size_t, _vp]),
    "dfh_mesh_simplify_clusters": (_int, [_vp, _int, ctypes.c_long, _vp, ctypes.c_long, _dbl, _c_double_p, _int, _dbl, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, ctypes.c_long, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_mesh_simplify_attr": (_int, [_vp, _int, ctypes.c_long, ctypes.c_long, _vp, _vp, _vp, ctypes.c_long, _vp, _vp]),
    "dfh_mesh_simplify_faces": (_int, [_vp, ctypes.c_long, ctypes.c_long, _vp, ctypes.c_long, _int, _vp, _vp, _vp, _vp, _vp,
                                       ctypes.POINTER(ctypes.c_long), _vp, ctypes.c_size_t, _vp]),
    "dfh_mesh_smooth_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long, ctypes.c_long]),
    "dfh_mesh_smooth_prepare": (_int, [_vp, _int, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp, _int, _vp, _vp, ctypes.c_size_t, _vp]),
    "dfh_mesh_smooth_run": (_int, [_vp, _int, ctypes.c_long, ctypes.c_long, ctypes.c_long, _int, _int, _int, _int, _dbl, _dbl, _vp, _vp,
                                   ctypes.c_size_t, _vp]),
    "dfh_mesh_vertex_normals": (_int, [_vp, _int, ctypes.c_long, ctypes.c_long, _dbl, _vp, _vp, ctypes.c_size_t, _vp]),
}

_lib = None


class DfhError(RuntimeError):
    pass


class DfhTimeout(DfhError):
    """A persistent kernel gave up waiting in a grid barrier (DFH_E_TIMEOUT)."""


def declared_symbols(header=HEADER_PATH):
    """Every function the public header declares (used by the symbol-export test)."""
    txt = open(header).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dfh_[a-z0-9_]+)\s*\(", txt)))


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DfhError("%s not found: the HIP library is the only implementation of this path "
                       "(no CPU fallback). Build it with `python -m dynamicfusion_body_amd.build`." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    v = lib.dfh_version()
    if v != ABI_VERSION:
        raise DfhError("libdfusion_hip.so ABI version %d != expected %d (rebuild)" % (v, ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().dfh_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError("%s: %s" % (what, msg))
        if rc == -4:
            raise DfhTimeout("%s: %s" % (what, msg))
        raise DfhError("%s failed (%d): %s" % (what, rc, msg))


_options_touched = set()


def set_option(name, value):
    """A development switch of the library (include/dfusion_hip.h: dfh_set_option); value None = unset (-1)."""
    check(load().dfh_set_option(name.encode(), -1 if value is None else int(value)), "dfh_set_option")
    _options_touched.add(name)


def reset_options():
    """Every switch changed through set_option() back to unset (tests call this between cases)."""
    for name in sorted(_options_touched):
        check(load().dfh_set_option(name.encode(), -1), "dfh_set_option")
    _options_touched.clear()


def get_option(name):
    return int(load().dfh_get_option(name.encode()))


def opt_on(name):
    """True when a development switch is set (> 0).  The Python layer's own A/B switches (py_*) live in the library's option
    table too: DFH_OPTIONS="py_no_side_stream=1" or set_option(); no call path reads the environment."""
    return load().dfh_get_option(name.encode()) > 0


_darr_cache = {}


def darr(values, n):
    """n doubles as a ctypes array.  The same small numpy arrays (intrinsics, poses) are passed on every launch of a frame:
    conversions are remembered by content (a few entries; the returned arrays are read-only by convention)."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
    if a.size != n:
        raise ValueError("expected %d values, got %d" % (n, a.size))
    key = a.tobytes()
    hit = _darr_cache.get(key)
    if hit is None:
        if len(_darr_cache) > 256:
            _darr_cache.clear()
        hit = _darr_cache[key] = (ctypes.c_double * n).from_buffer_copy(key)
    return hit


def iarr(values):
    vals = [int(v) for v in values]
    return (ctypes.c_int * len(vals))(*vals)


def slab(res, x_range=None):
    """dfh_slab: planes `x_range` (default: all) of a `res` grid."""
    x0, x1 = (0, res[0]) if x_range is None else x_range
    return Slab(iarr(res), int(x0), int(x1))
