"""ctypes binding of libgem_hip.so (include/gem_hip.h).

There is no CPU fallback: if the HIP library has not been built (`python -c "import
__graft_entry__ as g; g.build()"`) importing the compute path raises, and every entry point that
returns non-zero raises `GemError` with `gem_last_error()`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GEM_HIP_LIB: developer override to A/B two builds of the library on the same box
LIB_PATH = os.environ.get("GEM_HIP_LIB") or os.path.join(_HERE, "_lib", "libgem_hip.so")

GEM_MAX_HIDDEN, GEM_MAX_POLY, GEM_MAX_JOINTS = 8, 16, 16
STAGE_LOCAL, STAGE_GLOBAL = 0, 1
PRECISION = {"f32": 0, "bf16x3": 1, "bf16": 2}


class GemError(RuntimeError):
    pass


class GemConfig(C.Structure):
    _fields_ = [("seq_len", C.c_int32), ("n_joints", C.c_int32), ("latent_dim", C.c_int32), ("n_hidden", C.c_int32),
                ("hidden", C.c_int32 * GEM_MAX_HIDDEN), ("heat_h", C.c_int32), ("heat_w", C.c_int32),
                ("n_poly", C.c_int32), ("poly", C.c_double * GEM_MAX_POLY), ("cx", C.c_double), ("cy", C.c_double),
                ("parents", C.c_int32 * GEM_MAX_JOINTS), ("max_windows", C.c_int32), ("device", C.c_int32)]


class GemEnergyWeights(C.Structure):
    _fields_ = [("w3d", C.c_double), ("smooth", C.c_double), ("bone", C.c_double), ("vae", C.c_double),
                ("reproj", C.c_double)]


class GemLbfgsOpts(C.Structure):
    _fields_ = [("lr", C.c_double), ("max_iter", C.c_int32), ("max_eval", C.c_int32), ("history", C.c_int32),
                ("reserved", C.c_int32), ("tol_grad", C.c_double), ("tol_change", C.c_double), ("c1", C.c_double),
                ("c2", C.c_double), ("ls_tol_change", C.c_double)]


class GemTrainOpts(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("kld_weight", C.c_double), ("bn_momentum", C.c_double), ("recon_sum", C.c_int32), ("reserved", C.c_int32)]


class GemPickleArray(C.Structure):
    _fields_ = [("offset", C.c_int64), ("nbytes", C.c_int64), ("dtype", C.c_int32), ("ndim", C.c_int32), ("fortran", C.c_int32),
                ("key", C.c_int32), ("shape", C.c_int64 * 4)]


DT_F32, DT_F64 = 0, 1
PICKLE_UNSUPPORTED = 2


class GemMatArray(C.Structure):
    _fields_ = [("offset", C.c_int64), ("nbytes", C.c_int64), ("next", C.c_int64), ("start", C.c_int64), ("bare", C.c_int32),
                ("compressed", C.c_int32), ("mat_class", C.c_int32), ("storage", C.c_int32), ("ndim", C.c_int32),
                ("reserved", C.c_int32), ("dims", C.c_int64 * 4)]


class GemView(C.Structure):
    _fields_ = [("right", C.c_double * 3), ("down", C.c_double * 3), ("forward", C.c_double * 3), ("centre", C.c_double * 3),
                ("half_width", C.c_double), ("width", C.c_int32), ("height", C.c_int32)]


class GemCameraView(C.Structure):
    _fields_ = [("size", C.c_int32), ("joint_mask", C.c_uint32), ("rgb_heat", C.c_uint32), ("reserved", C.c_uint32),
                ("joint_radius", C.c_double), ("line_radius", C.c_double)]


class GemLiveBuffers(C.Structure):
    _fields_ = [("ring_pose", C.c_void_p), ("ring_cams", C.c_void_p), ("ring_times", C.c_void_p), ("ring_heat", C.c_void_p),
                ("state", C.c_void_p)]


LIVE_WINDOW, LIVE_STRIDE, LIVE_RING, LIVE_PUSH_MAX, LIVE_STATE_DOUBLES = 10, 8, 32, 8, 320
LIVE_DENSE_SLOTS, LIVE_DENSE_DOUBLES = 16, 1664          # include/gem_live_dense.h

MAT_UNSUPPORTED, MAT_NOT_FOUND = 2, 3
MAT_HEAT_F64, MAT_DEPTH_F32 = 1, 2
MI_SINGLE, MI_DOUBLE = 7, 9


class GemScaleReport(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("scale", "s0", "s_ref", "g0", "pairs", "inliers", "informative", "residual_rms", "path_length",
                                          "stance_right", "stance_left", "status", "lag", "tau", "min_pairs", "n_chunks")]


SCALE_CANDIDATES, SCALE_TILE, SCALE_REPORT_DOUBLES = 513, 256, 16
SCALE_NO_PAIRS, SCALE_TOO_FEW, SCALE_BAD_SCALE = 2, 3, 4


class GemDriftReport(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("status", "n_knots", "knot", "stiffness", "inliers", "informative", "residual_rms", "scale_min",
                                          "scale_max", "scale_mean", "metric_length", "slam_length", "lam", "first_id", "bad_pivot", "informed")]


DRIFT_MAX_KNOTS, DRIFT_REPORT_DOUBLES, DRIFT_NOT_SOLVED = 2048, 16, 5


class GemBoneDepthOpts(C.Structure):
    _fields_ = [("bone", C.c_double * GEM_MAX_JOINTS), ("dbar", C.c_double * GEM_MAX_JOINTS), ("neck_depth", C.c_double), ("w_n", C.c_double),
                ("w_m", C.c_double), ("iters", C.c_int32), ("reserved", C.c_int32)]


class GemGroundRecord(C.Structure):
    _fields_ = [("status", C.c_double), ("source", C.c_double), ("n", C.c_double * 3), ("d", C.c_double), ("u0", C.c_double * 3),
                ("tilt_cos", C.c_double)] + \
               [(k, C.c_double) for k in ("points", "inliers", "rms", "spread", "extent", "contact_right", "contact_left", "skate", "penetration",
                                          "lift_max", "skate_pairs", "frames", "lag")] + [("crt", C.c_double * 13), ("reserved", C.c_double * 12)]


GROUND_RECORD_DOUBLES, GROUND_LDS_FRAMES = 48, 1024
GROUND_NO_BODY, GROUND_BAD_SEQUENCE = 2, 3
GROUND_SOURCES = ("plane", "body_normal", "body")


class GemFootLockRecord(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("status", "runs_right", "runs_left", "pinned_right", "pinned_left", "changed", "lengthened", "unreachable",
                                          "delta_max", "delta_mean", "knee_max", "stretch_max", "slide_before", "slide_after", "slide_pairs",
                                          "frames")] + [("reserved", C.c_double * 8)]


FOOT_LOCK_RECORD_DOUBLES = 24
FOOT_LOCK_NO_CONTACT, FOOT_LOCK_BAD_GROUND, FOOT_LOCK_BAD_SEQUENCE = 2, 3, 4


class GemBridgeRecord(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("status", "frames", "lost", "gaps", "systems", "longest_gap", "offset_max", "angle_max",
                                          "translation_max")] + [("reserved", C.c_double * 7)]


BRIDGE_RECORD_DOUBLES, BRIDGE_MAX_GAP, BRIDGE_MAX_SPAN = 16, 64, 127
BRIDGE_NOT_SOLVED = 2
GLTF_LAYOUT = 40


class GemWindowStats(C.Structure):
    _fields_ = [("n_iter", C.c_int32), ("func_evals", C.c_int32), ("final_loss", C.c_float), ("status", C.c_int32)]


class GemLbfgsDebugState(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("phase", "n_iter", "evals", "ls_iter", "ls_evals", "hist_count", "hist_start", "low", "high",
                                          "insuf", "nan_seen", "pad_nonzero")] + \
               [(k, C.c_double) for k in ("t", "loss", "gtd", "d_norm", "H_diag")]


class GemGemmDebugArgs(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("route", "epi", "M", "T", "a_rows", "family", "out_bf16", "allow_split", "defer", "reserved")] + \
               [(k, C.c_void_p) for k in ("d_A", "d_aux", "d_C", "d_rows", "d_row_map")]


# name -> (restype, argtypes); every symbol include/gem_hip.h declares
_P = C.c_void_p
SIGNATURES = {
    "gem_last_error": (C.c_char_p, []),
    "gem_version": (C.c_int, []),
    "gem_create": (C.c_int, [C.POINTER(GemConfig), C.POINTER(_P)]),
    "gem_destroy": (None, [_P]),
    "gem_set_precision": (C.c_int, [_P, C.c_int]),
    "gem_load_vae": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "gem_mean_bone_length": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "gem_encode": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    "gem_decode": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P]),
    "gem_energy_grad": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.POINTER(GemEnergyWeights), _P, _P, _P, _P, _P]),
    "gem_optimize_stage": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.POINTER(GemEnergyWeights),
                                     C.POINTER(GemLbfgsOpts), _P, _P, _P]),
    "gem_optimize_windows": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.POINTER(GemEnergyWeights),
                                       C.POINTER(GemEnergyWeights), C.POINTER(GemLbfgsOpts), _P, _P, _P, _P]),
    "gem_set_texel_cache": (C.c_int, [_P, C.c_int]),
    "gem_graph_enable": (C.c_int, [_P, C.c_int]),
    "gem_graph_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gem_read_trace": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "gem_lbfgs_debug_begin": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "gem_lbfgs_debug_advance": (C.c_int, [_P, C.c_int, C.POINTER(GemLbfgsOpts), _P, _P, C.c_int, _P]),
    "gem_lbfgs_debug_read": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "gem_gemm_debug_layer_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(_P)]),
    "gem_gemm_debug_layer_destroy": (C.c_int, [_P, _P]),
    "gem_gemm_debug_run": (C.c_int, [_P, _P, C.POINTER(GemGemmDebugArgs), C.c_char_p, C.c_int, C.POINTER(C.c_int32), _P]),
    "gem_merge_windows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "gem_calculate_errors": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_double), _P, _P]),
    "gem_calculate_errors_chunks": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.POINTER(C.c_double), _P, _P]),
    "gem_sequence_quality": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "gem_skeleton_mesh_layout": (C.c_int, [C.POINTER(C.c_int64)]),
    "gem_skeleton_mesh_constant": (C.c_int, [_P, _P]),
    "gem_sequence_align": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "gem_skeleton_mesh": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P]),
    "gem_render_layout": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "gem_skeleton_capsules": (C.c_int, [_P, C.c_int64, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "gem_render_capsules": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int, C.POINTER(GemView), _P, C.c_int64, _P, _P, _P]),
    "gem_project_sequence": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P]),
    "gem_render_camera": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.POINTER(GemCameraView), _P, C.c_int64, _P, _P, _P]),
    "gem_lift_skeleton": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "gem_set_lanes": (C.c_int, [_P, C.c_int]),
    "gem_pickle_scan": (C.c_int, [_P, C.c_int64, C.POINTER(C.c_char_p), C.c_int, C.POINTER(GemPickleArray), C.c_int64, C.POINTER(C.c_int64)]),
    "gem_pickle_gather_f64": (C.c_int, [_P, C.c_int64, C.POINTER(GemPickleArray), C.c_int64, _P]),
    "gem_heat_gather": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "gem_chunk_open": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(_P)]),
    "gem_chunk_close": (None, [_P]),
    "gem_chunk_bytes": (C.c_int64, [_P]),
    "gem_chunk_count": (C.c_int64, [_P, C.c_int]),
    "gem_chunk_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    "gem_chunk_offsets": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "gem_chunk_gather_f64": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "gem_file_stage": (C.c_int, [C.c_char_p, C.c_int, _P, _P, C.c_int64, C.c_int64, C.POINTER(C.c_int64), _P]),
    "gem_mat_scan": (C.c_int, [_P, C.c_int64, C.c_char_p, C.POINTER(GemMatArray)]),
    "gem_files_sizes": (C.c_int, [C.POINTER(C.c_char_p), C.c_int64, _P]),
    "gem_mat_read": (C.c_int, [C.POINTER(C.c_char_p), C.c_int64, _P, _P, C.c_char_p, _P, C.c_int64, C.POINTER(GemMatArray), _P]),
    "gem_mat_frames": (C.c_int, [_P, C.c_int64, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "gem_prepare_global": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, _P]),
    "gem_profile_enable": (C.c_int, [_P, C.c_int]),
    "gem_profile_read": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "gem_profile_kernels": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_int]),
    "gem_trainer_create": (C.c_int, [C.POINTER(GemConfig), C.POINTER(_P)]),
    "gem_trainer_destroy": (None, [_P]),
    "gem_trainer_sizes": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gem_trainer_upload": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "gem_trainer_download": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "gem_trainer_set_step": (C.c_int, [_P, C.c_int64]),
    "gem_trainer_step": (C.c_int, [_P, C.c_int, _P, _P, C.POINTER(GemTrainOpts), C.c_int, _P, _P]),
    "gem_trainer_arena": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "gem_trainer_apply": (C.c_int, [_P, C.POINTER(GemTrainOpts), C.c_double, _P]),
    "gem_trainer_route": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "gem_trainer_layer_output": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P), C.POINTER(C.c_int)]),
    "gem_motion_cameras": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "gem_motion_windows": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int64, C.c_int, C.c_int, _P, C.c_int64, _P, _P]),
    "gem_latent_paths": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P]),
    "gem_latent_report": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "gem_live_push": (C.c_int, [_P, C.POINTER(GemLiveBuffers), C.c_int64, C.c_int, C.c_int64, _P, _P, _P, _P, _P]),
    "gem_live_window": (C.c_int, [_P, C.POINTER(GemLiveBuffers), C.c_int64, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "gem_live_emit": (C.c_int, [_P, C.POINTER(GemLiveBuffers), C.c_int64, C.c_int, _P, _P, _P, C.POINTER(C.c_double), _P, _P]),
    "gem_one_euro": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_double), _P, _P]),
    "gem_bvh_layout": (C.c_int, [C.POINTER(C.c_int64)]),
    "gem_bvh_tables": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gem_bvh_rest": (C.c_int, [_P, C.c_int64, _P, _P, _P]),
    "gem_bvh_channels": (C.c_int, [_P, C.c_int64, _P, _P, C.c_double, _P, _P]),
    "gem_format_fields": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P]),
    "gem_gltf_layout": (C.c_int, [C.c_int64, C.POINTER(C.c_int64)]),
    "gem_gltf_animation": (C.c_int, [_P, C.c_int64, _P, C.c_double, _P, _P, _P]),
    "gem_gltf_rest_mesh": (C.c_int, [_P, _P, _P, _P]),
    "gem_jpeg_header": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int64]),
    "gem_jpeg_bound": (C.c_int64, [C.c_int, C.c_int]),
    "gem_jpeg_encode": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, _P, C.c_int64, _P, _P, _P]),
    "gem_keypoint_heatmaps": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P]),
    "gem_lift_keypoints": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_double), C.c_int, _P, _P, _P, _P, _P]),
    "gem_fill_missing": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "gem_bone_depths": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_double), C.c_int, C.POINTER(GemBoneDepthOpts), _P, _P, _P, _P]),
    "gem_heatmap_peaks": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, _P]),
    "gem_slam_scale_work": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "gem_slam_scale": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int), _P, _P, _P, C.c_int64, C.c_int, C.c_double, C.c_int, _P,
                                 C.c_int64, _P, _P, _P, _P]),
    "gem_slam_drift_work": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "gem_slam_drift": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int), _P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_double,
                                 C.c_int, C.c_int, C.c_double, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gem_ground_plane_work": (C.c_int64, [_P, C.c_int, _P]),
    "gem_ground_plane": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, _P, C.c_int64, _P, _P]),
    "gem_similarity_compose": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "gem_foot_lock_work": (C.c_int64, [_P, C.c_int, _P]),
    "gem_foot_lock": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, _P, C.c_int64, _P, _P]),
    "gem_slam_bridge_work": (C.c_int64, [C.c_int64]),
    "gem_slam_bridge": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int64, _P, _P, _P, _P, _P, C.c_int64, _P, _P]),
    "gem_merge_cover": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int64, _P, _P, _P, _P, _P]),
}

# every symbol include/gem_live_dense.h declares (the header gem_hip.h includes for dense live mode)
DENSE_SIGNATURES = {
    "gem_live_window_at": (C.c_int, [_P, C.POINTER(GemLiveBuffers), C.c_int64, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "gem_live_emit_dense": (C.c_int, [_P, C.POINTER(GemLiveBuffers), _P, C.c_int, C.c_int64, C.c_int, _P, _P, _P, C.POINTER(C.c_double), _P, _P]),
    "gem_merge_dense": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
}

_lib = None


def load_library(path=None):
    """dlopen the HIP library and bind every declared symbol; raises GemError if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise GemError("HIP library %s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback for the optimiser)" % p)
    # PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64; it must be the HIP runtime of the
    # process (device pointers and streams come from torch), so make sure it is loaded first: the
    # DT_NEEDED entry of libgem_hip.so then binds to that copy by soname.
    import torch  # noqa: F401
    lib = C.CDLL(p)
    for name, (res, args) in list(SIGNATURES.items()) + list(DENSE_SIGNATURES.items()):
        fn = getattr(lib, name)           # AttributeError here = header and library out of sync
        fn.restype, fn.argtypes = res, args
    if path is None:
        _lib = lib
    return lib


def check(rc, lib=None):
    if rc != 0:
        msg = (lib or load_library()).gem_last_error()
        raise GemError(msg.decode() if msg else "libgem_hip call failed")


def default_lbfgs_opts(lr=2.0, max_iter=25, tol_change=1e-6):
    """torch.optim.LBFGS defaults as instantiated at optimizer.py:261-262."""
    return GemLbfgsOpts(lr=float(lr), max_iter=int(max_iter), max_eval=int(max_iter) * 5 // 4, history=100, reserved=0,
                        tol_grad=1e-7, tol_change=float(tol_change), c1=1e-4, c2=0.9, ls_tol_change=1e-9)
