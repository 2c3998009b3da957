"""ctypes binding of the HIP engine (librope_hip.so, ABI in include/rope_s3d.h).

This module is the only way the Python host code reaches the GPU.  There is no CPU
fallback: if the shared library is missing or no HIP device is usable, construction
raises `EngineUnavailable`.
"""
import ctypes as C
import os

import numpy as np

from .build import LIB_PATH
from .robot import RobotModel

LOSS_DEPTH, LOSS_FULL, LOSS_LOOKUP, LOSS_TSWEEP, LOSS_CAMFULL = 0, 1, 2, 3, 4
SUM_WORDS = 23
AGREE_WORDS = 28                 # ROPE_AGREE_WORDS (include/rope_s3d.h): the words rope_frame_agreement writes per frame
SHADE_MAX_NOISE_Q = 1023         # ROPE_SHADE_MAX_NOISE_Q
NEQ_WORDS = 32                   # ROPE_NEQ_WORDS: the doubles rope_pose_normal_equations writes per frame
BNEQ_WORDS = 96                  # ROPE_BNEQ_WORDS: the doubles rope_bundle_normal_equations writes per frame
RESID_WORDS = 258                # ROPE_RESID_WORDS: the uint32 rope_residual_histogram writes per frame: 256 bins, beyond the clip, not both
ROBUST_KINDS = {'huber': 1, 'tukey': 2}     # ROPE_ROBUST_HUBER, ROPE_ROBUST_TUKEY
SIL_MAX_RADIUS = 16              # ROPE_SIL_MAX_RADIUS: the largest truncation of rope_mask_distance's field, pixels
# rope_shade_params (include/rope_s3d.h), 64 bytes a record
SHADE_DTYPE = np.dtype([('light', '<f4', 3), ('ambient', '<f4'), ('gain', '<f4', 3), ('bg_depth', '<f4'), ('noise_q', '<i4'), ('bg_index', '<i4'),
                        ('albedo', 'u1', (6, 3)), ('bg_colour', 'u1', 3), ('reserved', 'u1', 3)])
Q32 = 4294967296.0
TQ_MAX = (1 << 39) - 1

ABI_SYMBOLS = (
    'rope_create', 'rope_destroy', 'rope_last_error', 'rope_set_robot', 'rope_set_camera', 'rope_set_target',
    'rope_candidates_upload', 'rope_eval_resident', 'rope_sync', 'rope_results_download', 'rope_eval',
    'rope_lookup_build', 'rope_lookup_score', 'rope_render', 'rope_render_batch', 'rope_render_masks', 'rope_trace_contours', 'rope_coverage', 'rope_debug_mvp', 'rope_profile_eval', 'rope_set_strategy', 'rope_geometry_cache_stats', 'rope_fragment_store_stats', 'rope_fragment_store_pairs', 'rope_set_fragment_budget',
    'rope_set_frames', 'rope_eval_views', 'rope_predict', 'rope_set_robot_mesh', 'rope_partition_mesh', 'rope_pack_target', 'rope_downsample_even',
    'rope_seg_nms', 'rope_seg_roi_align', 'rope_seg_bias_act', 'rope_seg_mask_overlaps',
    'rope_seg_rpn_targets', 'rope_seg_roi_targets', 'rope_seg_roi_align_float', 'rope_seg_roi_align_backward',
    'rope_set_target_tsweep', 'rope_set_targets', 'rope_stage_targets', 'rope_commit_targets', 'rope_eval_targets', 'rope_lookup_score_targets', 'rope_predict_batch',
    'rope_prepare_synthetic', 'rope_host_alloc', 'rope_host_free', 'rope_build_id', 'rope_camera_matrix', 'rope_lookup_grid', 'rope_crop_divisions',
    'rope_prepare_segmented', 'rope_stage_targets_segmented', 'rope_debug_targets', 'rope_resident_targets',
    'rope_render_batch_device', 'rope_stage_targets_synthetic', 'rope_hole_thresholds', 'rope_depth_holes', 'rope_frame_agreement',
    'rope_depth_decimated_shape', 'rope_depth_decimate', 'rope_depth_spatial', 'rope_depth_temporal', 'rope_depth_align',
    'rope_shade_frames', 'rope_pose_normal_equations', 'rope_pose_normal_workspace', 'rope_camera_normal_equations',
    'rope_bundle_normal_equations', 'rope_bundle_normal_workspace',
    'rope_residual_histogram', 'rope_bundle_normal_equations_robust', 'rope_bundle_normal_workspace_robust',
    'rope_mask_distance', 'rope_silhouette_normal_equations', 'rope_silhouette_normal_workspace',
    'rope_render_nearest', 'rope_silhouette_normal_equations_reverse',
    'rope_joint_axes', 'rope_levenberg_step', 'rope_formal_variance', 'rope_refine_poses', 'rope_refine_workspace',
    'rope_camera_twists', 'rope_bundle_pool', 'rope_bundle_schur_workspace', 'rope_bundle_schur_step', 'rope_bundle_schur_variance',
    'rope_bundle_columns_step', 'rope_bundle_columns_variance', 'rope_refine_bundle', 'rope_refine_bundle_workspace')

TARGET_TILE_W, TARGET_TILE_H = 64, 32      # ROPE_TARGET_TILE_W / _H (csrc/rope_kernels.h): the output tile of rope_stage_targets_segmented's kernel


STAGE_LOOKUP, STAGE_DESCENT, STAGE_SFLIP, STAGE_ISWEEP, STAGE_TSWEEP = 0, 1, 2, 3, 4


class StageDesc(C.Structure):
    """rope_stage (include/rope_s3d.h)."""
    _fields_ = [('kind', C.c_int32), ('to_render', C.c_int32), ('count', C.c_int32), ('joints', C.c_uint32),
                ('init_rate', C.c_double * 6), ('rate_reduction', C.c_double), ('early_stop', C.c_double), ('range', C.c_double)]


EvalHook = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int32)     # rope_eval_hook


class PredictArgs(C.Structure):
    """rope_predict_args (include/rope_s3d.h)."""
    _fields_ = [('stages', C.POINTER(StageDesc)), ('n_stages', C.c_int32), ('speculate', C.c_int32),
                ('limits', C.c_void_p), ('camera_pose', C.c_void_p), ('min_ang_inc', C.c_void_p),
                ('lookup_angles', C.c_void_p), ('n_lookup', C.c_int32), ('use_table', C.c_int32), ('lookup_crop', C.c_void_p),
                ('lookup_angles_live', C.c_void_p), ('on_eval', EvalHook), ('on_eval_user', C.c_void_p)]


class EngineUnavailable(RuntimeError):
    pass


class EngineError(RuntimeError):
    pass


_lib = None


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch ships its own copy of libamdhip64 (SONAME libamdhip64.so.7, found through its RPATH);
    librope_hip.so asks the loader for libamdhip64.so.7 and, loaded first, gets the system copy — a later `import torch` (the
    segmentation stage: Predictor._load_segmenter imports maskrcnn after the engine exists) then brings a SECOND runtime into the
    process, torch finds no GPU, and the rope_seg_* kernels would be handed streams and pointers of a runtime that is not theirs.
    So when torch is installed and not yet loaded, its copy is mapped first: the loader then satisfies librope_hip.so — and
    torch's own libraries later — with that one copy.  Nothing of torch is imported here."""
    import sys
    if 'torch' in sys.modules or os.environ.get('ROPE_SYSTEM_HIP_RUNTIME'):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
        if spec is None or not spec.submodule_search_locations:
            return
        lib = os.path.join(list(spec.submodule_search_locations)[0], 'lib', 'libamdhip64.so')
        if os.path.exists(lib):
            C.CDLL(lib, mode=C.RTLD_GLOBAL)
    except (ImportError, OSError, ValueError):
        pass                                             # no torch, or a torch without its own runtime: the system copy serves everyone


def load_library(path: str = None):
    """dlopen librope_hip.so and declare the prototypes.  Does not touch the GPU."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get('ROPE_HIP_LIB', LIB_PATH)
    if not os.path.exists(path):
        raise EngineUnavailable(f"{path} not found: build it with `python -m rope_s3d_amd.build` "
                                "(hipcc, gfx950); the engine has no CPU fallback")
    _share_torch_hip_runtime()
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise EngineUnavailable(f"cannot load {path}: {e}") from e
    vp, i32, dbl = C.c_void_p, C.c_int, C.c_double
    lib.rope_create.argtypes = [C.POINTER(vp), i32]
    lib.rope_destroy.argtypes = [vp]
    lib.rope_destroy.restype = None
    lib.rope_last_error.argtypes = [vp]
    lib.rope_last_error.restype = C.c_char_p
    lib.rope_set_robot.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp]
    lib.rope_set_camera.argtypes = [vp, vp, i32, i32, dbl, dbl]
    lib.rope_set_target.argtypes = [vp, vp, vp, vp]
    lib.rope_candidates_upload.argtypes = [vp, vp, i32]
    lib.rope_eval_resident.argtypes = [vp, i32, i32, vp]
    lib.rope_sync.argtypes = [vp]
    lib.rope_results_download.argtypes = [vp, vp, vp, vp, vp]
    lib.rope_eval.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.rope_lookup_build.argtypes = [vp, vp, i32, i32, vp]
    lib.rope_lookup_score.argtypes = [vp, vp, vp, vp]
    lib.rope_render.argtypes = [vp, vp, i32, vp, vp]
    lib.rope_render_batch.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    lib.rope_render_masks.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp]
    lib.rope_trace_contours.argtypes = [vp, i32, i32, i32, vp, i32, vp, i32, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.rope_coverage.argtypes = [vp, vp, i32, i32, vp]
    lib.rope_debug_mvp.argtypes = [vp, vp, i32, i32]
    lib.rope_profile_eval.argtypes = [vp, i32, i32, vp, i32, vp]
    lib.rope_set_strategy.argtypes = [vp, i32]
    lib.rope_geometry_cache_stats.argtypes = [vp, vp, vp]
    lib.rope_fragment_store_stats.argtypes = [vp, vp, vp, vp, vp]
    lib.rope_set_fragment_budget.argtypes = [vp, C.c_uint64]
    lib.rope_fragment_store_pairs.argtypes = [vp, vp]
    if hasattr(lib, 'rope_debug_skip'):                 # librope_hip_profile.so only (ROPE_HIP_LIB=...)
        lib.rope_debug_skip.argtypes = [vp, i32]
        lib.rope_debug_clock.argtypes = [vp, vp]
        lib.rope_debug_bounds.argtypes = [vp, vp]
    lib.rope_predict.argtypes = [vp, C.POINTER(PredictArgs), vp, vp, C.POINTER(C.c_int64)]
    lib.rope_set_robot_mesh.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp]
    lib.rope_partition_mesh.argtypes = [vp, i32, vp, i32, i32, i32, vp, vp]
    lib.rope_pack_target.argtypes = [vp, vp, C.c_int64, vp]
    lib.rope_downsample_even.argtypes = [vp, i32, i32, i32, C.c_int64, i32, i32, vp]
    lib.rope_seg_nms.argtypes = [vp, vp, vp, i32, i32, C.c_float, i32, vp, vp, vp]
    lib.rope_seg_roi_align.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp]
    lib.rope_seg_rpn_targets.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.rope_seg_roi_targets.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, vp, C.c_float, vp, vp, vp, vp, vp]
    lib.rope_seg_roi_align_float.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp]
    lib.rope_seg_roi_align_backward.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp]
    lib.rope_seg_bias_act.argtypes = [vp, vp, vp, C.c_int64, i32, C.c_int64, i32, vp]
    lib.rope_seg_mask_overlaps.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp, vp]
    lib.rope_frame_agreement.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.c_float, vp, vp]
    lib.rope_depth_decimated_shape.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.rope_depth_decimate.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    lib.rope_depth_spatial.argtypes = [vp, i32, i32, i32, C.c_float, i32, i32, vp]
    lib.rope_depth_temporal.argtypes = [vp, i32, i32, i32, C.c_float, i32, i32, vp, vp, vp]
    lib.rope_depth_align.argtypes = [vp, i32, i32, i32, vp, vp, vp, dbl, i32, i32, vp, vp, vp]
    lib.rope_shade_frames.argtypes = [vp, vp, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp, i32, C.c_uint32,
                                      C.c_uint64, vp, vp, vp]
    lib.rope_pose_normal_equations.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, vp, i32, C.c_float,
                                               vp, vp, vp]
    lib.rope_camera_normal_equations.argtypes = list(lib.rope_pose_normal_equations.argtypes)
    lib.rope_pose_normal_workspace.argtypes = [i32, i32, i32]
    lib.rope_pose_normal_workspace.restype = C.c_size_t
    lib.rope_bundle_normal_equations.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, vp, i32, vp, i32,
                                                 C.c_float, vp, vp, vp]
    lib.rope_bundle_normal_workspace.argtypes = [i32, i32, i32]
    lib.rope_bundle_normal_workspace.restype = C.c_size_t
    lib.rope_residual_histogram.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.c_float, vp, vp]
    lib.rope_bundle_normal_equations_robust.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, vp, i32, vp,
                                                        i32, C.c_float, i32, C.c_float, vp, vp, vp]
    lib.rope_bundle_normal_workspace_robust.argtypes = [i32, i32, i32]
    lib.rope_bundle_normal_workspace_robust.restype = C.c_size_t
    lib.rope_mask_distance.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    lib.rope_silhouette_normal_equations.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, vp, i32, vp, i32,
                                                     i32, vp, vp, vp]
    lib.rope_silhouette_normal_workspace.argtypes = [i32, i32, i32]
    lib.rope_silhouette_normal_workspace.restype = C.c_size_t
    lib.rope_render_nearest.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
    lib.rope_silhouette_normal_equations_reverse.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, vp, i32,
                                                             vp, i32, i32, vp, vp, vp]
    lib.rope_joint_axes.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    lib.rope_levenberg_step.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    lib.rope_formal_variance.argtypes = [vp, i32, i32, vp, vp]
    lib.rope_refine_poses.argtypes = [vp, vp, vp, i32, vp, C.c_float, C.c_float, C.c_float, C.c_float, i32, vp, C.c_float, i32, dbl,
                                      vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rope_refine_workspace.argtypes = [vp, i32]
    lib.rope_refine_workspace.restype = C.c_size_t
    lib.rope_camera_twists.argtypes = [vp, vp, vp, vp]
    lib.rope_bundle_pool.argtypes = [vp, i32, vp, vp]
    lib.rope_bundle_schur_workspace.argtypes = [i32]
    lib.rope_bundle_schur_workspace.restype = C.c_size_t
    lib.rope_bundle_schur_step.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.rope_bundle_schur_variance.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    lib.rope_bundle_columns_step.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.rope_bundle_columns_variance.argtypes = [vp, i32, vp, vp]
    lib.rope_refine_bundle.argtypes = [vp, i32, vp, vp, vp, i32, dbl, dbl, dbl, dbl, dbl, dbl, i32, i32, vp, C.c_float, i32, dbl, vp,
                                       vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rope_refine_bundle_workspace.argtypes = [vp, i32]
    lib.rope_refine_bundle_workspace.restype = C.c_size_t
    lib.rope_set_frames.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.rope_eval_views.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.rope_set_target_tsweep.argtypes = [vp, vp]
    lib.rope_set_targets.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.rope_stage_targets.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.rope_commit_targets.argtypes = [vp]
    lib.rope_stage_targets_segmented.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, vp, i32, i32, vp]
    lib.rope_debug_targets.argtypes = [vp, vp, vp, vp, vp]
    lib.rope_resident_targets.argtypes = [vp]
    lib.rope_render_batch_device.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.rope_stage_targets_synthetic.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp]
    lib.rope_hole_thresholds.argtypes = [dbl, dbl, i32, vp, C.POINTER(i32)]
    lib.rope_depth_holes.argtypes = [vp, i32, i32, i32, C.c_uint32, C.c_uint64, vp, vp, i32, i32, vp]
    lib.rope_eval_targets.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    lib.rope_lookup_score_targets.argtypes = [vp, vp, vp, vp]
    lib.rope_predict_batch.argtypes = [vp, C.POINTER(PredictArgs), i32, vp, vp, C.POINTER(C.c_int64)]
    lib.rope_camera_matrix.argtypes = [vp, dbl, dbl, dbl, dbl, i32, i32, dbl, dbl, vp]
    lib.rope_crop_divisions.argtypes = [C.c_int64, i32, vp]
    lib.rope_prepare_segmented.argtypes = [vp, i32, C.c_int64, i32, i32, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp]
    lib.rope_lookup_grid.argtypes = [vp, vp, vp, C.c_int64]
    lib.rope_lookup_grid.restype = C.c_int64
    lib.rope_build_id.argtypes = []
    lib.rope_build_id.restype = C.c_char_p
    lib.rope_host_alloc.argtypes = [C.c_size_t]
    lib.rope_host_alloc.restype = C.c_void_p
    lib.rope_host_free.argtypes = [vp]
    lib.rope_host_free.restype = None
    lib.rope_prepare_synthetic.argtypes = [vp, C.c_int64, vp, i32, C.c_int64, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp]
    _lib = lib
    return lib


def _dp(t):
    """A torch tensor's storage as a void pointer."""
    return C.c_void_p(t.data_ptr())


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def pack_target(depth: np.ndarray, mask_bits: np.ndarray = None) -> np.ndarray:
    """Target depth (metres) + per-link mask bits -> the uint64 plane rope_set_target takes.

    bits 0..38: depth in Q32 metres (round half even, clipped to [0, 2^39-1]; NaN and
    negatives count as "no depth" = 0); bits 40..47: bit l set where link l's mask is true.
    """
    d = np.asarray(depth, np.float64)
    if _lib is not None or os.path.exists(os.environ.get('ROPE_HIP_LIB', LIB_PATH)):       # one pass in the library (host code, no GPU)
        d = np.ascontiguousarray(d)
        bits = None if mask_bits is None else np.ascontiguousarray(mask_bits, np.uint8)
        out = np.empty(d.shape, np.uint64)
        if load_library().rope_pack_target(_p(d), _p(bits), d.size, _p(out)) == 0:
            return out
    q = np.rint(np.where(np.isfinite(d) & (d > 0), d, 0.0) * Q32)
    q = np.minimum(q, float(TQ_MAX)).astype(np.uint64)
    if mask_bits is not None:
        q |= np.asarray(mask_bits, np.uint64) << np.uint64(40)
    return np.ascontiguousarray(q)


def trace_contours(mask: np.ndarray, bit: int, box=None, min_points: int = 0) -> list:
    """rope_trace_contours (host only, thread-safe, no GPU): the borders of bit `bit` of an (H, W) uint8 plane as
    cv2.findContours(RETR_TREE, CHAIN_APPROX_SIMPLE) finds them, outer and hole borders in raster-scan order, each an (k, 2)
    int32 array of (x, y) points.  box (r0, r1, c0, c1) must enclose every set pixel of the bit (all -1 = none set) or be
    None for the whole plane; contours of fewer than min_points points are left out."""
    lib = load_library()
    mask = np.ascontiguousarray(mask, np.uint8)
    if mask.ndim != 2:
        raise ValueError(f"trace_contours: need one (H, W) plane, got {mask.shape}")
    box_arr = None if box is None else np.ascontiguousarray(box, np.int32).reshape(4)
    H, W = mask.shape
    n_pts, n_con = C.c_int(0), C.c_int(0)
    pts, starts = np.empty((1024, 2), np.int32), np.empty(65, np.int32)
    while True:
        rc = lib.rope_trace_contours(_p(mask), H, W, int(bit), _p(box_arr), int(min_points), _p(pts), len(pts), _p(starts),
                                     len(starts), C.byref(n_pts), C.byref(n_con))
        if rc != -3:                                    # ROPE_E_NOMEM: the sizes it needs are in n_pts / n_con
            break
        pts, starts = np.empty((max(n_pts.value, 1), 2), np.int32), np.empty(n_con.value + 1, np.int32)
    if rc != 0:
        raise EngineError(f"rope_trace_contours failed ({rc}): bad plane, bit or box")
    return [pts[starts[i]:starts[i + 1]].copy() for i in range(n_con.value)]


def build_id() -> str:
    """rope_build_id of the loaded library: the hash of the sources it was built from."""
    return load_library().rope_build_id().decode()


def camera_twists(pose6):
    """rope_camera_twists (host only, no GPU): [x, y, z, a3, a4, a5] -> (Rwc (3, 3), tc (3,), twists (6, 6)): the kernels' camera
    axes X_c = Rwc (X_w - tc) as rope_refine_poses derives them, and refinement.camera_twists with a written operation order."""
    pose = np.ascontiguousarray(pose6, np.float64).reshape(6)
    Rwc, tc, tw = np.empty((3, 3)), np.empty(3), np.empty((6, 6))
    if load_library().rope_camera_twists(_p(pose), _p(Rwc), _p(tc), _p(tw)) != 0:
        raise ValueError(f"camera pose: six finite numbers, got {pose}")
    return Rwc, tc, tw


def pinned_empty(shape, dtype) -> np.ndarray:
    """np.empty in page-locked host memory (rope_host_alloc): planes handed to set_target(s) from it reach the device in one
    transfer.  Falls back to ordinary memory when the runtime refuses.  The memory lives as long as the array (or any view of it)."""
    import weakref
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    lib = load_library()
    ptr = lib.rope_host_alloc(n) if n else None
    if not ptr:
        return np.empty(shape, dtype)
    buf = (C.c_ubyte * n).from_address(ptr)
    weakref.finalize(buf, lib.rope_host_free, C.c_void_p(ptr))
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def prepare_synthetic(color: np.ndarray, depth: np.ndarray, f: int, link_blue, n_lookup_links: int, tq: np.ndarray, lookup_f32: np.ndarray,
                      flags: np.ndarray, tgt_depth: np.ndarray = None) -> bool:
    """rope_prepare_synthetic: one frame of the synthetic path into the given output arrays (host code, interpreter lock released).
    False when the arrays' layout is not one the library takes (the caller then goes the numpy way)."""
    if color.dtype != np.uint8 or color.ndim != 3 or color.shape[2] != 3 or color.strides[2] != 1 or color.strides[1] != 3 or color.strides[0] < 0:
        return False
    kind = {np.dtype(np.float32): 1, np.dtype(np.float64): 2}.get(depth.dtype)
    if kind is None or depth.ndim != 2 or depth.shape != color.shape[:2] or depth.strides[1] != depth.itemsize or depth.strides[0] < 0:
        return False
    H0, W0 = depth.shape
    if f < 1 or (f > 1 and f % 2) or H0 % f or W0 % f:
        return False
    for a, dt in ((tq, np.uint64), (lookup_f32, np.float32), (flags, np.uint8)) + (((tgt_depth, np.float64),) if tgt_depth is not None else ()):
        assert a.dtype == dt and a.flags.c_contiguous
    assert tq.shape == (H0 // f, W0 // f) == lookup_f32.shape and flags.size >= 8
    lb = np.ascontiguousarray(link_blue, np.int32)
    rc = load_library().rope_prepare_synthetic(C.c_void_p(color.ctypes.data), color.strides[0], C.c_void_p(depth.ctypes.data), kind, depth.strides[0],
                                               H0, W0, int(f), _p(lb), len(lb), int(n_lookup_links), _p(tq), _p(lookup_f32), _p(tgt_depth), _p(flags))
    return rc == 0


def prepare_segmented(depth: np.ndarray, f: int, masks: np.ndarray, link_of, n_links: int, n_lookup_links: int, tq: np.ndarray,
                      lookup_f32: np.ndarray, flags: np.ndarray, tgt_depth: np.ndarray = None) -> bool:
    """rope_prepare_segmented: one frame of the segmentation path (instance masks (H, W, K) bool + the link of every instance) into
    the given output arrays.  False when the layout is not one the library takes."""
    kind = {np.dtype(np.float32): 1, np.dtype(np.float64): 2}.get(depth.dtype)
    if kind is None or depth.ndim != 2 or depth.strides[1] != depth.itemsize or depth.strides[0] < 0:
        return False
    H0, W0 = depth.shape
    if f < 1 or (f > 1 and f % 2) or H0 % f or W0 % f:
        return False
    m = np.ascontiguousarray(masks).view(np.uint8) if masks.dtype == bool else np.ascontiguousarray(masks, np.uint8)
    if m.ndim != 3 or m.shape[:2] != (H0 // f, W0 // f):
        return False
    lo = np.ascontiguousarray(link_of, np.int32)
    if len(lo) != m.shape[2]:
        return False
    assert tq.shape == (H0 // f, W0 // f) == lookup_f32.shape and tq.flags.c_contiguous and lookup_f32.flags.c_contiguous and flags.size >= 8
    rc = load_library().rope_prepare_segmented(C.c_void_p(depth.ctypes.data), kind, depth.strides[0], H0, W0, int(f), _p(m), m.shape[2], _p(lo),
                                               int(n_links), int(n_lookup_links), _p(tq), _p(lookup_f32), _p(tgt_depth), _p(flags))
    return rc == 0


def hole_thresholds(std: float = .22, thresh_factor: float = 1, max_size: int = 25):
    """rope_hole_thresholds (host code, no GPU): the dilation sizes d = np.arange(3, max_size, 3) of NoiseMaker.holes and, per size,
    T = floor(P(|N(0, std)| >= 1 - thresh_factor / d) * 2^32), the threshold its seed bits are drawn against.
    -> (d int32 (n,), T uint32 (n,))."""
    lib = load_library()
    n = C.c_int(0)
    if lib.rope_hole_thresholds(float(std), float(thresh_factor), int(max_size), None, C.byref(n)) != 0:
        raise EngineError(f"rope_hole_thresholds: std {std} must be positive and max_size {max_size} at most 33")
    T = np.zeros(n.value, np.uint32)
    if lib.rope_hole_thresholds(float(std), float(thresh_factor), int(max_size), _p(T), C.byref(n)) != 0:
        raise EngineError("rope_hole_thresholds failed")
    return np.arange(3, 3 * n.value + 1, 3, dtype=np.int32), T


class Engine:
    """One engine context on one GPU: robot + camera + current target, batched evaluation."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        rc = self._lib.rope_create(C.byref(self._ctx), int(device))
        if rc != 0:
            msg = self._lib.rope_last_error(None).decode()
            self._ctx = C.c_void_p()
            raise EngineUnavailable(f"rope_create(device={device}) failed ({rc}): {msg}")
        self.device = device
        self.W = self.H = 0
        self.n_links = 0
        self.n_candidates = 0
        self._strategy = 0            # last value given to rope_set_strategy (the ROPE_STRATEGY environment default is the library's own)

    def close(self):
        if getattr(self, '_ctx', None) is not None and self._ctx.value:
            self._lib.rope_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise EngineError(f"{what} failed ({rc}): {self._lib.rope_last_error(self._ctx).decode()}")

    # -- static state -------------------------------------------------------------------------
    def set_robot(self, robot: RobotModel):
        m = robot.meshlets
        hdr = np.ascontiguousarray(m.header, np.uint32)
        verts = np.ascontiguousarray(m.verts, np.float32)
        tris = np.ascontiguousarray(m.tris, np.uint32)
        first = np.ascontiguousarray(m.link_first, np.int32)
        jf = np.ascontiguousarray(robot.joint_fixed, np.float64)
        ja = np.ascontiguousarray(robot.joint_axes, np.float64)
        self._check(self._lib.rope_set_robot(self._ctx, _p(hdr), len(hdr), _p(verts), len(verts), _p(tris), len(tris),
                                             _p(first), len(first) - 1, _p(jf), _p(ja)), 'rope_set_robot')
        self.n_links = len(first) - 1

    def set_robot_mesh(self, robot: RobotModel):
        """rope_set_robot_mesh: plain vertex / index arrays in, the library builds the meshlets (what a C host calls)."""
        verts, faces = np.ascontiguousarray(robot.verts, np.float32), np.ascontiguousarray(robot.faces, np.int32)
        vo, to = np.ascontiguousarray(robot.vtx_off, np.int32), np.ascontiguousarray(robot.tri_off, np.int32)
        jf, ja = np.ascontiguousarray(robot.joint_fixed, np.float64), np.ascontiguousarray(robot.joint_axes, np.float64)
        self._check(self._lib.rope_set_robot_mesh(self._ctx, _p(verts), _p(faces), _p(vo), _p(to), len(vo) - 1, _p(jf), _p(ja)),
                    'rope_set_robot_mesh')
        self.n_links = len(vo) - 1

    def set_camera(self, PV: np.ndarray, W: int, H: int, znear: float, zfar: float):
        PV = np.ascontiguousarray(PV, np.float64)
        assert PV.shape == (4, 4)
        self._check(self._lib.rope_set_camera(self._ctx, _p(PV), int(W), int(H), float(znear), float(zfar)), 'rope_set_camera')
        self.W, self.H = int(W), int(H)

    def set_target(self, tq: np.ndarray, t32: np.ndarray = None, link_flags=None):
        tq = np.ascontiguousarray(tq, np.uint64)
        if tq.shape != (self.H, self.W):
            raise ValueError(f"target plane must be {(self.H, self.W)}, got {tq.shape}")
        if t32 is not None:
            t32 = np.ascontiguousarray(t32, np.float32)
            if t32.shape != (self.H, self.W):
                raise ValueError("float32 target plane has the wrong shape")
        lf = np.zeros(8, np.uint8)
        if link_flags is not None:
            lf[:len(link_flags)] = link_flags
        self._check(self._lib.rope_set_target(self._ctx, _p(tq), _p(t32), _p(lf)), 'rope_set_target')

    def set_target_tsweep(self, t32_full: np.ndarray = None):
        """The float32 plane ROPE_LOSS_TSWEEP reads (the whole target depth) when it is not the lookup plane; None: the one plane."""
        if t32_full is not None:
            t32_full = np.ascontiguousarray(t32_full, np.float32)
            if t32_full.shape != (self.H, self.W):
                raise ValueError("float32 target plane has the wrong shape")
        self._check(self._lib.rope_set_target_tsweep(self._ctx, _p(t32_full)), 'rope_set_target_tsweep')

    # -- many frames at once --------------------------------------------------------------------
    def _target_planes(self, tq, t32, link_flags, t32_tsweep):
        tq = np.ascontiguousarray(tq, np.uint64)
        n = len(tq)
        if tq.shape != (n, self.H, self.W):
            raise ValueError(f"target planes must be {(n, self.H, self.W)}, got {tq.shape}")
        planes = []
        for a in (t32, t32_tsweep):
            if a is not None:
                a = np.ascontiguousarray(a, np.float32)
                if a.shape != tq.shape:
                    raise ValueError("float32 target planes have the wrong shape")
            planes.append(a)
        lf = np.zeros((n, 8), np.uint8)
        if link_flags is not None:
            lf[:] = np.asarray(link_flags, np.uint8).reshape(n, 8)
        return n, tq, planes[0], planes[1], lf

    def set_targets(self, tq: np.ndarray, t32: np.ndarray = None, link_flags: np.ndarray = None, t32_tsweep: np.ndarray = None):
        """The targets of N frames resident at once (rope_set_targets): tq (N,H,W) uint64, t32 / t32_tsweep (N,H,W) float32 or None,
        link_flags (N,8) uint8."""
        n, tq, t32, ts, lf = self._target_planes(tq, t32, link_flags, t32_tsweep)
        self._check(self._lib.rope_set_targets(self._ctx, n, _p(tq), _p(t32), _p(ts), _p(lf)), 'rope_set_targets')
        self.n_targets = n

    def stage_targets(self, tq: np.ndarray, t32: np.ndarray = None, link_flags: np.ndarray = None, t32_tsweep: np.ndarray = None):
        """set_targets into the context's second set of planes, on a stream of its own (rope_stage_targets): returns with the copies
        on their way while the resident targets stay in use — from this thread or another.  The arrays must stay alive and
        untouched until commit_targets() (they are kept here); page-locked ones (pinned_empty) make the copy asynchronous."""
        n, tq, t32, ts, lf = self._target_planes(tq, t32, link_flags, t32_tsweep)
        self._staged = (n, tq, t32, ts, lf)
        rc = self._lib.rope_stage_targets(self._ctx, n, _p(tq), _p(t32), _p(ts), _p(lf))
        if rc:
            self._staged = None
            raise RuntimeError(f"rope_stage_targets failed ({rc})")

    def commit_targets(self):
        """The staged targets become the resident ones (rope_commit_targets)."""
        self._check(self._lib.rope_commit_targets(self._ctx), 'rope_commit_targets')
        self.n_targets = self._staged[0] if getattr(self, '_staged', None) else 0
        self._staged = None

    def stage_targets_segmented(self, depth_t, masks_t, inst_first, link_of, n_lookup: int, n_total: int, slot0: int = 0,
                                want_tsweep: bool = False):
        """rope_stage_targets_segmented: slots slot0 .. slot0 + B - 1 of a staged set of n_total frames, built on the device from
        torch tensors that are there already — depth_t (B, H, W) float32 / float64, masks_t (K_total, H, W) bool or uint8 (instance
        planes, frame-major; None when K_total == 0) — by kernels on torch's current stream, with no wait for them: they run behind
        whatever produced the masks.  inst_first: B + 1 plane offsets, link_of: K_total link indices (-1: none of the rendered links).
        The tensors are kept alive until commit_targets()."""
        import torch
        kind = {torch.float32: 1, torch.float64: 2}.get(depth_t.dtype)
        if kind is None or depth_t.dim() != 3 or tuple(depth_t.shape[1:]) != (self.H, self.W) or not depth_t.is_contiguous():
            raise ValueError(f"depth planes must be contiguous (B, {self.H}, {self.W}) float32 / float64, got {tuple(depth_t.shape)} {depth_t.dtype}")
        if depth_t.device.type != 'cuda' or depth_t.device.index != self.device:
            raise ValueError(f"depth planes must be on cuda:{self.device}, got {depth_t.device}")
        first = np.ascontiguousarray(inst_first, np.int32).reshape(-1)
        links = np.ascontiguousarray(link_of, np.int32).reshape(-1)
        if len(first) != depth_t.shape[0] + 1 or (len(first) and len(links) != first[-1]):
            raise ValueError("inst_first holds one offset per frame and one more; link_of one entry per instance plane")
        masks_ptr = None
        if masks_t is not None and masks_t.numel():
            if masks_t.dtype not in (torch.bool, torch.uint8) or masks_t.dim() != 3 or tuple(masks_t.shape[1:]) != (self.H, self.W) \
                    or not masks_t.is_contiguous() or masks_t.device != depth_t.device or masks_t.shape[0] < len(links):
                raise ValueError(f"instance planes must be contiguous (K, {self.H}, {self.W}) bool / uint8 beside the depth, K >= {len(links)}")
            masks_ptr = C.c_void_p(masks_t.data_ptr())
        if slot0 == 0 or getattr(self, '_staged', None) is None or not isinstance(self._staged[1], list):
            self._staged = (int(n_total), [])
        self._staged[1].append((depth_t, masks_t))
        rc = self._lib.rope_stage_targets_segmented(self._ctx, int(n_total), int(slot0), int(depth_t.shape[0]), C.c_void_p(depth_t.data_ptr()), kind,
                                                    masks_ptr, _p(first), _p(links) if len(links) else None, int(n_lookup), int(bool(want_tsweep)),
                                                    C.c_void_p(torch.cuda.current_stream(depth_t.device).cuda_stream))
        if rc:
            raise EngineError(f"rope_stage_targets_segmented failed ({rc})")

    def stage_targets_synthetic(self, depth_t, ids_t, f: int, blue_of_id, link_blue, n_lookup: int, n_total: int, slot0: int = 0,
                                want_tsweep: bool = False):
        """rope_stage_targets_synthetic: slots slot0 .. slot0 + B - 1 of a staged set of n_total frames, built on the device from
        full-size renders that are there already — depth_t (B, H0, W0) float32 and ids_t (B, H0, W0) uint8 torch tensors
        (render_batch_device), H0 / f x W0 / f this engine's image size — by kernels on torch's current stream: per frame what
        prepare_synthetic gives for the colour plane blue_of_id[ids].  blue_of_id: 256 channel-0 values, link_blue: one per link.
        The tensors are kept alive until commit_targets()."""
        import torch
        if depth_t.dtype != torch.float32 or ids_t.dtype != torch.uint8 or depth_t.dim() != 3 or depth_t.shape != ids_t.shape \
                or not depth_t.is_contiguous() or not ids_t.is_contiguous():
            raise ValueError(f"need contiguous (B, H0, W0) float32 depth and uint8 id planes, got {tuple(depth_t.shape)} {depth_t.dtype} and "
                             f"{tuple(ids_t.shape)} {ids_t.dtype}")
        if depth_t.device.type != 'cuda' or depth_t.device.index != self.device or ids_t.device != depth_t.device:
            raise ValueError(f"the planes must be on cuda:{self.device}, got {depth_t.device} and {ids_t.device}")
        lut = np.ascontiguousarray(blue_of_id, np.uint8).reshape(-1)
        lb = np.ascontiguousarray(link_blue, np.int32).reshape(-1)
        if len(lut) != 256:
            raise ValueError("blue_of_id holds one channel-0 value per id: 256 bytes")
        if slot0 == 0 or getattr(self, '_staged', None) is None or not isinstance(self._staged[1], list):
            self._staged = (int(n_total), [])
        self._staged[1].append((depth_t, ids_t))
        rc = self._lib.rope_stage_targets_synthetic(self._ctx, int(n_total), int(slot0), int(depth_t.shape[0]), C.c_void_p(depth_t.data_ptr()),
                                                    C.c_void_p(ids_t.data_ptr()), int(depth_t.shape[1]), int(depth_t.shape[2]), int(f), _p(lut), _p(lb),
                                                    len(lb), int(n_lookup), int(bool(want_tsweep)),
                                                    C.c_void_p(torch.cuda.current_stream(depth_t.device).cuda_stream))
        if rc:
            raise EngineError(f"rope_stage_targets_synthetic failed ({rc})")

    def depth_holes(self, depth_t, seed: int, frame0: int = 0, std: float = .22, thresh_factor: float = 1, max_size: int = 25,
                    connection_factor: int = 20):
        """rope_depth_holes: NoiseMaker.holes' holes punched into depth_t, (N, H, W) or (H, W) float32 on this engine's device, in
        place, by a kernel on torch's current stream.  Plane m takes the bits of frame frame0 + m of the 64-bit `seed`: the holes
        of a frame do not depend on how a run is cut into calls.  The distribution is the reference's, the stream its own
        (tests/holes_ref.py is the same contract in numpy)."""
        import torch
        if depth_t.dtype != torch.float32 or depth_t.dim() not in (2, 3) or not depth_t.is_contiguous():
            raise ValueError(f"depth planes must be contiguous (N, H, W) float32, got {tuple(depth_t.shape)} {depth_t.dtype}")
        if depth_t.device.type != 'cuda' or depth_t.device.index != self.device:
            raise ValueError(f"depth planes must be on cuda:{self.device}, got {depth_t.device}")
        d, T = hole_thresholds(std, thresh_factor, max_size)
        H, W = depth_t.shape[-2:]
        N = depth_t.shape[0] if depth_t.dim() == 3 else 1
        if N == 0:
            return depth_t
        with torch.cuda.device(depth_t.device):
            rc = self._lib.rope_depth_holes(C.c_void_p(depth_t.data_ptr()), int(N), int(H), int(W), int(frame0) & 0xFFFFFFFF,
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, _p(T), _p(d), len(d), int(connection_factor),
                                            C.c_void_p(torch.cuda.current_stream(depth_t.device).cuda_stream))
        if rc:
            raise EngineError(f"rope_depth_holes failed ({rc}): N <= 65535 planes, dilations and connection_factor at most 32")
        return depth_t

    def _planes(self, named):
        """named: (name, tensor, torch dtype by name, or a tuple of names) per plane stack.  Every one a contiguous (N, H, W) tensor of
        its dtype on this engine's device and of the first one's shape, or ValueError -> (N, H, W)."""
        import torch
        shape = None
        for name, t, dt in named:
            dts, text = (dt, ' or '.join(dt)) if isinstance(dt, tuple) else ((dt,), f"torch.{dt}")
            if not isinstance(t, torch.Tensor) or t.dtype not in [getattr(torch, d) for d in dts] or t.dim() != 3 or not t.is_contiguous():
                raise ValueError(f"{name}: a contiguous (N, H, W) {text} tensor")
            if t.device.type != 'cuda' or t.device.index != self.device:
                raise ValueError(f"{name} must be on cuda:{self.device}, got {t.device}")
            if shape is None:
                shape = tuple(t.shape)
            elif tuple(t.shape) != shape:
                raise ValueError(f"{name}: shape {tuple(t.shape)}, the renders are {shape}")
        return shape

    def shade_frames(self, depth_t, ids_t, params, intr, n_links: int, backgrounds=None, frame0: int = 0, seed: int = 0, depth_out=True,
                     out=None):
        """rope_shade_frames: the N renders depth_t (N, H, W) float32 / ids_t (N, H, W) uint8 (render_batch_device's, on this engine's
        device) lit, painted, laid over their backgrounds and given sensor noise, by kernels on torch's current stream; nothing is
        waited for.  params: N records of SHADE_DTYPE (simulation/shading.py makes them); intr: (fx, fy, cx, cy); backgrounds:
        (n_bg, H, W, 3) uint8 on the device, or None when every bg_index is -1.  Plane m draws the noise of frame frame0 + m of the
        64-bit seed.  depth_out: True = a new tensor, False = none, or the tensor to write (depth_t itself is allowed).  out: the
        (N, H, W, 3) uint8 tensor to write the pictures to (any alignment), a new one when None.
        -> (bgr (N, H, W, 3) uint8, depth with bg_depth behind the robot (N, H, W) float32 or None).
        The arithmetic is the contract of include/rope_s3d.h; tests/shade_ref.py restates it in numpy."""
        import torch
        N, H, W = self._planes((('depth', depth_t, 'float32'), ('ids', ids_t, 'uint8')))
        dev = depth_t.device
        params = np.ascontiguousarray(params, SHADE_DTYPE).reshape(-1)
        if len(params) != N:
            raise ValueError(f"{len(params)} parameter records for {N} frames")
        n_bg = 0
        if backgrounds is not None:
            if backgrounds.dtype != torch.uint8 or backgrounds.device != dev or not backgrounds.is_contiguous() or \
                    tuple(backgrounds.shape[1:]) != (H, W, 3):
                raise ValueError(f"backgrounds: a contiguous (n_bg, {H}, {W}, 3) uint8 tensor on {dev}")
            n_bg = int(backgrounds.shape[0])
        fx, fy, cx, cy = (float(v) for v in intr)
        with torch.cuda.device(dev):
            bgr = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev) if out is None else out
            if bgr.dtype != torch.uint8 or tuple(bgr.shape) != (N, H, W, 3) or not bgr.is_contiguous() or bgr.device != dev:
                raise ValueError(f"out: a contiguous ({N}, {H}, {W}, 3) uint8 tensor on {dev}")
            if depth_out is True:
                depth_out = torch.empty_like(depth_t)
            elif depth_out is False:
                depth_out = None
            elif depth_out.dtype != torch.float32 or depth_out.shape != depth_t.shape or not depth_out.is_contiguous() or depth_out.device != dev:
                raise ValueError("depth_out: a contiguous float32 tensor of the depth planes' shape, on their device")
            rc = self._lib.rope_shade_frames(C.c_void_p(depth_t.data_ptr()), C.c_void_p(ids_t.data_ptr()), int(N), int(H), int(W), int(n_links),
                                             fx, fy, cx, cy, _p(params), C.c_void_p(backgrounds.data_ptr()) if n_bg else None, n_bg,
                                             int(frame0) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(bgr.data_ptr()),
                                             C.c_void_p(depth_out.data_ptr()) if depth_out is not None else None,
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc == -1:
            raise ValueError(f"rope_shade_frames refused its arguments: {N} frames of {H} x {W}, n_links {n_links} (1 .. 6), noise_q in "
                             f"0 .. {SHADE_MAX_NOISE_Q}, bg_index in -1 .. {n_bg - 1}")
        if rc:
            raise EngineError(f"rope_shade_frames failed ({rc})")
        return bgr, depth_out

    def frame_agreement(self, render_depth, render_ids, frame_depth, n_links: int, tol: float) -> np.ndarray:
        """rope_frame_agreement: N renders against the N recorded depth maps of their frames -> (N, 28) uint64, per frame
        [0] valid pixels of the recording, [1] rendered pixels, [2] the sum of |q(R) - q(T)| (q = floor(x 2^32)) over the pixels both
        rendered and valid, [3] pixels whose id is neither a link's nor the background's, [4 + 4 l ..] link l: rendered, both, close
        (within tol metres), front (the recording nearer by more than tol).  render_depth / frame_depth (N, H, W) float32 and
        render_ids (N, H, W) uint8 are torch tensors on this engine's device (render_batch_device's); the kernel runs on torch's
        current stream and the sums are waited for here."""
        import torch
        N, H, W = self._planes((('render_depth', render_depth, 'float32'), ('render_ids', render_ids, 'uint8'), ('frame_depth', frame_depth, 'float32')))
        if N == 0:
            return np.zeros((0, AGREE_WORDS), np.uint64)
        dev = render_depth.device
        with torch.cuda.device(dev):
            sums = torch.empty((N, AGREE_WORDS), dtype=torch.int64, device=dev)
            rc = self._lib.rope_frame_agreement(C.c_void_p(render_depth.data_ptr()), C.c_void_p(render_ids.data_ptr()),
                                                C.c_void_p(frame_depth.data_ptr()), int(N), int(H), int(W), int(n_links), float(tol),
                                                C.c_void_p(sums.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            if rc == -1:
                raise ValueError(f"rope_frame_agreement refused its arguments: {N} frames of {H} x {W} (at most 2^24 pixels), "
                                 f"n_links {n_links} (1 .. 6), tol {tol} (finite, not negative)")
            if rc:
                raise EngineError(f"rope_frame_agreement failed ({rc})")
            return sums.cpu().numpy().view(np.uint64)

    def pose_normal_equations(self, render_depth, render_ids, frame_depth, joints, n_links: int, clip: float, intr) -> np.ndarray:
        """rope_pose_normal_equations: N renders at N poses against the N depth frames -> (N, 32) float64, per frame [0] the pixels
        both rendered and measured, [1] the sum over them of min(r^2, clip^2) with r = render - frame, [2] the inliers (on a moving
        link, |r| <= clip, a normal, not grazing), [3] their sum of r^2, [4..9] J^T r, [10..30] the upper triangle of J^T J row by
        row, [31] 0; J is the derivative of the rendered depth with respect to the joint angles (include/rope_s3d.h).
        render_depth / frame_depth (N, H, W) float32 and render_ids (N, H, W) uint8 are torch tensors on this engine's device
        (render_batch_device's); joints (N, n_joints, 6) float64, a numpy array or a tensor: unit axis and a point on the axis per
        joint, in camera axes (x right, y down, z forward); intr: (fx, fy, cx, cy).  The kernels run on torch's current stream and
        the sums are waited for here.  The same planes give the same bytes from run to run and however a batch is cut."""
        return self._normal_equations('rope_pose_normal_equations', self._lib.rope_pose_normal_workspace, NEQ_WORDS, render_depth, render_ids,
                                      ('frame_depth', frame_depth, 'float32'), [('joints', joints, 'axis and a point on it per joint')],
                                      n_links, float(clip), f"clip {clip} (finite, positive)", intr)

    def camera_normal_equations(self, render_depth, render_ids, frame_depth, twists, n_links: int, clip: float, intr) -> np.ndarray:
        """rope_camera_normal_equations: pose_normal_equations with respect to the camera pose -> (N, 32) float64 with the same
        words.  twists (N, n_cols, 6) float64, a numpy array or a tensor: per column its angular part w and its linear part v in
        camera axes; a surface point P moves by w x P + v per unit of the column, and EVERY drawn link moves with every column,
        link 0 too (prediction/refinement.py: camera_twists).  Columns from n_cols on are exactly zero in [4..30].  Everything
        else — the planes, intr, the stream, determinism, the empty batch — is pose_normal_equations'."""
        return self._normal_equations('rope_camera_normal_equations', self._lib.rope_pose_normal_workspace, NEQ_WORDS, render_depth, render_ids,
                                      ('frame_depth', frame_depth, 'float32'), [('twists', twists, 'angular and linear part per column')],
                                      n_links, float(clip), f"clip {clip} (finite, positive)", intr)

    def bundle_normal_equations(self, render_depth, render_ids, frame_depth, joint_axes, twists, n_links: int, clip: float, intr) -> np.ndarray:
        """rope_bundle_normal_equations: the joints' and the camera's columns in ONE system of twelve slots -> (N, 96) float64, per
        frame [0] .. [3] as camera_normal_equations', [4 + c] J_c^T r, [16..93] the upper triangle of J^T J row by row over the
        twelve slots, [94], [95] 0; slot j < 6 is joint j (pose_normal_equations' column), slot 6 + k camera column k
        (camera_normal_equations'), and every drawn link is an inlier, the base too (include/rope_s3d.h).  joint_axes
        (N, n_joints, 6) and twists (N, n_cols, 6) float64 as those two calls take them; either may be None (no such columns), not
        both.  Everything else — the planes, intr, the stream, determinism, the empty batch — is pose_normal_equations'."""
        return self._normal_equations('rope_bundle_normal_equations', self._lib.rope_bundle_normal_workspace, BNEQ_WORDS, render_depth, render_ids,
                                      ('frame_depth', frame_depth, 'float32'), self._two_blocks(joint_axes, twists), n_links, float(clip),
                                      f"clip {clip} (finite, positive)", intr)

    def bundle_normal_equations_robust(self, render_depth, render_ids, frame_depth, joint_axes, twists, n_links: int, clip: float, intr, kind: str,
                                       scale: float) -> np.ndarray:
        """rope_bundle_normal_equations_robust: bundle_normal_equations with a Huber or Tukey weight w per inlier at the scale `scale`
        metres (finite, 0 < scale <= clip) -> (N, 96) float64 in the same layout and slots: [1] the sum of the robust cost, [3] the sum
        of w r^2, [4 + c] of w J_c r, [16..93] of w J_a J_b; Tukey's inliers end at the scale, Huber's at clip (include/rope_s3d.h).
        kind: 'huber' or 'tukey'.  Huber at scale == clip gives bundle_normal_equations' bytes.  Everything else — the planes, the
        columns, intr, the stream, determinism, the empty batch — is bundle_normal_equations'."""
        if kind not in ROBUST_KINDS:
            raise ValueError(f"kind: 'huber' or 'tukey', got {kind!r}")
        return self._normal_equations('rope_bundle_normal_equations_robust', self._lib.rope_bundle_normal_workspace_robust, BNEQ_WORDS, render_depth,
                                      render_ids, ('frame_depth', frame_depth, 'float32'), self._two_blocks(joint_axes, twists), n_links,
                                      (float(clip), ROBUST_KINDS[kind], float(scale)),
                                      f"clip {clip} (finite, positive), scale {scale} (finite, positive, at most clip)", intr)

    def residual_histogram(self, render_depth, render_ids, frame_depth, n_links: int, clip: float) -> np.ndarray:
        """rope_residual_histogram: N renders against the N depth frames -> (N, 258) uint32, per frame [b < 256] the pixels both
        rendered and measured with |r| <= clip in bin min(255, int(|r| 256 / clip)), [256] those beyond clip (a NaN too), [257] the
        pixels that are not both; a frame's words add up to H W (include/rope_s3d.h).  The planes are bundle_normal_equations'.
        Integer adds alone: the words depend neither on order nor on how a batch is cut.  Runs on torch's current stream and the
        counts are waited for here."""
        import torch
        N, H, W = self._planes((('render_depth', render_depth, 'float32'), ('render_ids', render_ids, 'uint8'), ('frame_depth', frame_depth, 'float32')))
        if N == 0:
            return np.zeros((0, RESID_WORDS), np.uint32)
        dev = render_depth.device
        with torch.cuda.device(dev):
            hist = torch.empty((N, RESID_WORDS), dtype=torch.int32, device=dev)
            rc = self._lib.rope_residual_histogram(_dp(render_depth), _dp(render_ids), _dp(frame_depth), int(N), int(H), int(W), int(n_links),
                                                   float(clip), _dp(hist), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            if rc == -1:
                raise ValueError(f"rope_residual_histogram refused its arguments: {N} frames of {H} x {W} (at most 2^24 pixels), "
                                 f"n_links {n_links} (1 .. 6), clip {clip} (finite, positive)")
            if rc:
                raise EngineError(f"rope_residual_histogram failed ({rc})")
            return hist.cpu().numpy().view(np.uint32)

    def mask_distance(self, mask_t, radius: int):
        """rope_mask_distance: N masks -> (N, H, W) int32 on the device, the truncated signed squared distance of every pixel to
        its mask's boundary: -m inside the mask, +m outside, m the least dx^2 + dy^2 to a pixel of the other state within radius
        pixels and inside the image, radius^2 + 1 where there is none (include/rope_s3d.h).  mask_t (N, H, W) bool or uint8, a
        contiguous torch tensor on this engine's device, non-zero = robot; radius 1 .. 16.  The kernel runs on torch's current
        stream and nothing is waited for."""
        import torch
        N, H, W = self._planes([('mask', mask_t, ('uint8', 'bool'))])
        radius = self._radius(radius)
        dev = mask_t.device
        with torch.cuda.device(dev):
            sd2 = torch.empty((N, H, W), dtype=torch.int32, device=dev)
            if N == 0:
                return sd2
            rc = self._lib.rope_mask_distance(_dp(mask_t), int(N), int(H), int(W), radius, _dp(sd2), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc == -1:
            raise ValueError(f"rope_mask_distance refused its arguments: {N} planes of {H} x {W} (fewer than 2^31 pixels), radius {radius}")
        if rc:
            raise EngineError(f"rope_mask_distance failed ({rc})")
        return sd2

    def silhouette_normal_equations(self, render_depth, render_ids, sd2, joint_axes, twists, n_links: int, radius: int, intr) -> np.ndarray:
        """rope_silhouette_normal_equations: the outline of N renders against the distance fields of the N frames' masks -> (N, 96)
        float64 in bundle_normal_equations' layout and slots, per frame [0] the contour pixels of the render, [1] their sum of e^2
        (e the signed distance of the pixel's outer edge to the mask's boundary, pixels, truncated at radius), [2] the contour
        pixels within radius of the boundary, [3] their sum of e^2, [4 + c] J_c^T e, [16..93] the upper triangle of J^T J, [94],
        [95] 0 (include/rope_s3d.h).  sd2 (N, H, W) int32: mask_distance's of the same radius.  One-directional: the render's
        outline is measured against the mask.  Everything else — the renders, joint_axes, twists, intr, the stream, determinism,
        the empty batch — is bundle_normal_equations'."""
        return self._normal_equations('rope_silhouette_normal_equations', self._lib.rope_silhouette_normal_workspace, BNEQ_WORDS, render_depth,
                                      render_ids, ('sd2', sd2, 'int32'), self._two_blocks(joint_axes, twists), n_links, self._radius(radius),
                                      f"radius {radius}", intr)

    def render_nearest(self, render_ids, n_links: int, radius: int):
        """rope_render_nearest: N id planes of a render -> (N, H, W) int16 on the device, per pixel the nearest pixel of the other
        state (rendered, id < n_links, or not) within radius pixels and inside the image as (dy + 16) 33 + (dx + 16), of several at
        the least distance the first in raster order; -1 where there is none (include/rope_s3d.h).  It is mask_distance's field of
        the render's coverage, sd = -+(dx^2 + dy^2), and where that distance is reached.  render_ids (N, H, W) uint8, a contiguous
        torch tensor on this engine's device (render_batch_device's); n_links 1 .. 255; radius 1 .. 16.  The kernel runs on torch's
        current stream and nothing is waited for."""
        import torch
        N, H, W = self._planes([('render_ids', render_ids, 'uint8')])
        radius = self._radius(radius)
        dev = render_ids.device
        with torch.cuda.device(dev):
            near = torch.empty((N, H, W), dtype=torch.int16, device=dev)
            if N == 0:
                return near
            rc = self._lib.rope_render_nearest(_dp(render_ids), int(N), int(H), int(W), int(n_links), radius, _dp(near),
                                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc == -1:
            raise ValueError(f"rope_render_nearest refused its arguments: {N} planes of {H} x {W} (fewer than 2^31 pixels), n_links {n_links} "
                             f"(1 .. 255), radius {radius}")
        if rc:
            raise EngineError(f"rope_render_nearest failed ({rc})")
        return near

    def silhouette_normal_equations_reverse(self, mask, near, render_depth, render_ids, joint_axes, twists, n_links: int, radius: int,
                                            intr) -> np.ndarray:
        """rope_silhouette_normal_equations_reverse: the outline of the N frames' MASKS against the nearest-pixel fields of the N
        renders -> (N, 96) float64 in silhouette_normal_equations' layout, slots and units, so that the two directions' words add:
        [0] the contour pixels of the mask, [1] their sum of e^2, [2] those within radius of the render's boundary, [3] their sum
        of e^2, [4 + c] J_c^T e, [16..93] the upper triangle of J^T J, [94], [95] 0; a column's J is taken at the rendered pixel
        that carries the boundary the mask pixel sees (include/rope_s3d.h).  mask (N, H, W) uint8 or bool, non-zero = robot; near
        (N, H, W) int16: render_nearest's of render_ids at the same n_links and radius.  Everything else — the renders, joint_axes,
        twists, intr, the stream, determinism, the empty batch — is silhouette_normal_equations'."""
        return self._normal_equations('rope_silhouette_normal_equations_reverse', self._lib.rope_silhouette_normal_workspace, BNEQ_WORDS,
                                      render_depth, render_ids, None, self._two_blocks(joint_axes, twists), n_links, self._radius(radius),
                                      f"radius {radius}", intr, lead=(('mask', mask, ('uint8', 'bool')), ('near', near, 'int16')))

    @staticmethod
    def _radius(radius) -> int:
        if int(radius) != radius or not 1 <= int(radius) <= SIL_MAX_RADIUS:
            raise ValueError(f"radius: a whole number in 1 .. {SIL_MAX_RADIUS}, got {radius}")
        return int(radius)

    @staticmethod
    def _two_blocks(joint_axes, twists):
        return [('joint_axes', joint_axes, 'axis and a point on it per joint'), ('twists', twists, 'angular and linear part per column')]

    def _normal_equations(self, entry: str, workspace, width: int, render_depth, render_ids, third, blocks, n_links: int, scalar, scalar_text: str,
                          intr, lead=()) -> np.ndarray:
        """The checks, the buffers and the call behind the normal-equation entries.  workspace: the entry's scratch query;
        width: the words a frame gets (32 or 96); third: (name, tensor, dtype) of the planes the renders are held against, handed
        over after the renders — or None for an entry that takes its planes BEFORE the renders, lead: such (name, tensor, dtype); blocks:
        one or two (name, columns, what they are), columns (N, n, 6) float64 or None — not all None; scalar: what the entry takes
        after the columns (clip or radius; a tuple where it takes several), checked and converted by the caller, and scalar_text its part of
        the refusal."""
        import torch
        third = () if third is None else (third,)
        N, H, W = self._planes((('render_depth', render_depth, 'float32'), ('render_ids', render_ids, 'uint8'), *third, *lead))
        dev = render_depth.device
        if all(c is None for _, c, _ in blocks):
            raise ValueError(f"{' and '.join(name for name, _, _ in blocks)}: at least one of them" if len(blocks) > 1 else f"{blocks[0][0]}: not None")
        cols = []
        for name, c, what in blocks:
            if c is not None and not isinstance(c, torch.Tensor):
                c = torch.from_numpy(np.ascontiguousarray(c, np.float64))
            if c is not None and (c.dtype != torch.float64 or c.dim() != 3 or c.shape[0] != N or c.shape[2] != 6):
                raise ValueError(f"{name}: ({N}, n, 6) float64 — {what}, got {tuple(c.shape)} {c.dtype}")
            cols.append(c)
        counts = [0 if c is None else int(c.shape[1]) for c in cols]
        if N == 0:
            return np.zeros((0, width), np.float64)
        fx, fy, cx, cy = (float(v) for v in intr)
        with torch.cuda.device(dev):
            cols = [None if c is None or n == 0 else c.to(dev).contiguous() for c, n in zip(cols, counts)]
            out = torch.empty((N, width), dtype=torch.float64, device=dev)
            work = torch.empty(max(1, workspace(int(N), int(H), int(W)) // 8), dtype=torch.float64, device=dev)
            rc = getattr(self._lib, entry)(*(_dp(t) for _, t, _ in lead), _dp(render_depth), _dp(render_ids), *(_dp(t) for _, t, _ in third),
                                           int(N), int(H), int(W), int(n_links), fx, fy, cx, cy,
                                           *(a for c, n in zip(cols, counts) for a in (None if c is None else _dp(c), n)),
                                           *(scalar if isinstance(scalar, tuple) else (scalar,)), _dp(out), _dp(work),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            if rc == -1:
                columns = f"{counts[0]} {blocks[0][0]} (1 .. 6)" if len(blocks) == 1 else \
                    f"{counts[0]} joints and {counts[1]} twists (0 .. 6 each, not both 0)"
                raise ValueError(f"{entry} refused its arguments: {N} frames of {H} x {W} (at most 2^24 pixels), n_links {n_links} (1 .. 6), "
                                 f"{columns}, {scalar_text}, intrinsics {(fx, fy, cx, cy)}")
            if rc:
                raise EngineError(f"{entry} failed ({rc})")
            return out.cpu().numpy()

    # -- the native polish (csrc/rope_polish.hip) ----------------------------------------------------
    def _polish_tensor(self, name: str, t, cols, N=None):
        """A float64 numpy array or tensor -> a contiguous float64 tensor (N, cols) (or (N,) for cols None) on this engine's device,
        checked the way _normal_equations checks its columns."""
        import torch
        if not isinstance(t, torch.Tensor):
            t = torch.from_numpy(np.ascontiguousarray(t, np.float64))
        shape = tuple(t.shape)
        if t.dtype != torch.float64 or t.dim() != (1 if cols is None else 2) or (cols is not None and shape[1] != cols) or \
                (N is not None and shape[0] != N):
            raise ValueError(f"{name}: ({'N' if N is None else N}{'' if cols is None else f', {cols}'}) float64, got {shape} {t.dtype}")
        if t.device.type == 'cuda' and t.device.index != self.device:
            raise ValueError(f"{name} must be on cuda:{self.device} or on the host, got {t.device}")
        return t.to(torch.device('cuda', self.device)).contiguous()

    @staticmethod
    def _active_mask(active_mask) -> int:
        if isinstance(active_mask, bool) or int(active_mask) != active_mask or not 0 <= int(active_mask) <= 63:
            raise ValueError(f"active_mask: bit j set = joint j is refined, 0 .. 63, got {active_mask!r}")
        return int(active_mask)

    @staticmethod
    def _limits(limits) -> np.ndarray:
        limits = np.ascontiguousarray(limits, np.float64)
        if limits.shape != (6, 2) or not np.isfinite(limits).all() or (limits[:, 0] > limits[:, 1]).any():
            raise ValueError("limits: (6, 2) finite [lo, hi] per joint with lo <= hi")
        return limits

    def joint_axes_device(self, q, Rwc, tc):
        """rope_joint_axes: (N, 6) angles, a float64 numpy array or tensor -> (N, 6, 6) float64 tensor on this engine's device: per
        joint its unit axis and a point on it in the camera axes X_c = Rwc (X_w - tc), by the chain the renders are drawn with
        (include/rope_s3d.h) — what pose_normal_equations takes as `joints`.  Rwc (3, 3) and tc (3,) are host float64.  The kernel
        runs on torch's current stream and nothing is waited for."""
        import torch
        q_t = self._polish_tensor('q', q, 6)
        Rwc, tc = np.ascontiguousarray(Rwc, np.float64), np.ascontiguousarray(tc, np.float64)
        if Rwc.shape != (3, 3) or tc.shape != (3,) or not (np.isfinite(Rwc).all() and np.isfinite(tc).all()):
            raise ValueError("Rwc: (3, 3) and tc: (3,), finite float64")
        N = q_t.shape[0]
        dev = q_t.device
        with torch.cuda.device(dev):
            out = torch.empty((N, 6, 6), dtype=torch.float64, device=dev)
            if N == 0:
                return out
            self._check(self._lib.rope_joint_axes(self._ctx, C.c_void_p(q_t.data_ptr()), int(N), _p(Rwc), _p(tc), C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), 'rope_joint_axes')
        return out

    def levenberg_step(self, words, q, lam, active_mask: int, limits):
        """rope_levenberg_step: per frame (A + lam diag A) d = -g on the joints of active_mask with a positive diagonal, by Gaussian
        elimination with partial pivoting, and trial = clip(q + d, limits) -> (N, 6) float64 tensor on the device; d = 0 for a
        frame with no such joint, a singular system or a solution that is not finite (include/rope_s3d.h).  words (N, 32), q (N, 6),
        lam (N,): float64 numpy arrays or tensors; limits (6, 2).  Runs on torch's current stream; nothing is waited for."""
        import torch
        words_t = self._polish_tensor('words', words, NEQ_WORDS)
        N = words_t.shape[0]
        q_t, lam_t = self._polish_tensor('q', q, 6, N), self._polish_tensor('lam', lam, None, N)
        mask, limits = self._active_mask(active_mask), self._limits(limits)
        dev = words_t.device
        with torch.cuda.device(dev):
            trial = torch.empty((N, 6), dtype=torch.float64, device=dev)
            if N == 0:
                return trial
            rc = self._lib.rope_levenberg_step(C.c_void_p(words_t.data_ptr()), C.c_void_p(q_t.data_ptr()), C.c_void_p(lam_t.data_ptr()), int(N), mask,
                                               _p(limits), C.c_void_p(trial.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc:
            raise EngineError(f"rope_levenberg_step failed ({rc})")
        return trial

    def formal_variance(self, words, active_mask: int):
        """rope_formal_variance: per frame s^2 diag(A^-1) on the joints of active_mask with a positive diagonal, s^2 = [3] / ([2] - p)
        -> (N, 6) float64 tensor on the device: the SQUARE of refinement.formal_sigma — nan outside active_mask, inf where the
        frame does not pin the joints down (include/rope_s3d.h).  Runs on torch's current stream; nothing is waited for."""
        import torch
        words_t = self._polish_tensor('words', words, NEQ_WORDS)
        mask = self._active_mask(active_mask)
        N = words_t.shape[0]
        dev = words_t.device
        with torch.cuda.device(dev):
            var = torch.empty((N, 6), dtype=torch.float64, device=dev)
            if N == 0:
                return var
            rc = self._lib.rope_formal_variance(C.c_void_p(words_t.data_ptr()), int(N), mask, C.c_void_p(var.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc:
            raise EngineError(f"rope_formal_variance failed ({rc})")
        return var

    def refine_workspace(self, n_frames: int) -> int:
        """rope_refine_workspace: the bytes of device scratch refine_poses needs for n_frames frames of the camera's size; 0 for a
        batch one call does not take."""
        return int(self._lib.rope_refine_workspace(self._ctx, int(n_frames)))

    def refine_poses(self, q, frame_depth, camera_pose, intr, active_mask: int, limits, clip: float, iterations: int, damping: float,
                     want_words: bool = False):
        """rope_refine_poses: PoseRefiner.refine's loop inside the library — render, joint axes, normal equations, Levenberg steps
        kept only when the cost falls, formal variances — with the systems and the solves on the device.
        q (N, 6) host angles; frame_depth (N, H, W) float32 tensor on this engine's device, H x W the camera's; camera_pose
        [x, y, z, a3, a4, a5]; intr (fx, fy, cx, cy); active_mask bit j = joint j; limits (6, 2).
        -> dict(angles (N, 6), var (N, 6) — formal_sigma squared —, cost_before, cost_after, inliers (N,) float64, steps (N,) int32
        [, words (N, 32) the final systems]).  Runs on the context's stream, after torch's current stream has finished with the
        frames, and is complete on return.  Like render_batch_device it takes the per-candidate buffers."""
        mask, limits = self._active_mask(active_mask), self._limits(limits)
        fx, fy, cx, cy = (float(v) for v in intr)

        def outputs(N):
            out = dict(angles=np.empty((N, 6)), var=np.empty((N, 6)), cost_before=np.empty(N), cost_after=np.empty(N), inliers=np.empty(N),
                       steps=np.empty(N, np.int32))
            if want_words:
                out['words'] = np.empty((N, NEQ_WORDS))
            return out

        return self._native_refine('rope_refine_poses', self.refine_workspace, q, frame_depth, camera_pose, iterations, damping, 0, outputs,
                                   lambda q, pose, depth, N, work, o: self._lib.rope_refine_poses(
                                       self._ctx, q, depth, N, pose, fx, fy, cx, cy, mask, _p(limits), float(clip), int(iterations), float(damping), work,
                                       _p(o['angles']), _p(o['var']), _p(o['cost_before']), _p(o['cost_after']), _p(o['steps']), _p(o['inliers']),
                                       _p(o.get('words'))))

    def _native_refine(self, entry: str, workspace, q, frame_depth, camera_pose, iterations, damping, min_frames: int, outputs, call):
        """What refine_poses and refine_bundle share: the checks of the poses, the frames and the loop's arguments, outputs(N) ->
        the dict of host arrays the entry fills, the scratch, and call(q, pose, frames, N, scratch, outputs) -> the entry's code
        once torch's current stream has finished with the frames.  Fewer than min_frames frames are refused; an empty batch
        that is not returns its empty outputs without a call."""
        import torch
        q = np.ascontiguousarray(q, np.float64).reshape(-1, 6)
        N = len(q)
        self._planes([('frame_depth', frame_depth, 'float32')])
        if N < min_frames or tuple(frame_depth.shape) != (N, self.H, self.W):
            raise ValueError(f"frame_depth: ({N}, {self.H}, {self.W}) as the poses and the camera{f', N >= {min_frames}' if min_frames else ''}, "
                             f"got {tuple(frame_depth.shape)}")
        pose = np.ascontiguousarray(camera_pose, np.float64).reshape(6)
        if int(iterations) != iterations or iterations < 0 or not (np.isfinite(damping) and damping >= 0):
            raise ValueError("iterations and damping must not be negative")
        out = outputs(N)
        if N == 0:
            return out
        nbytes = workspace(N)
        if nbytes == 0:
            raise ValueError(f"{entry} takes no batch of {N} frames of {self.H} x {self.W} in one call")
        dev = frame_depth.device
        with torch.cuda.device(dev):
            work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
            torch.cuda.current_stream(dev).synchronize()            # the frames are ready, and `work` is no longer anyone else's
            rc = call(_p(q), _p(pose), _dp(frame_depth), int(N), _dp(work), out)
        if rc == -1:
            raise ValueError(f"{entry} refused its arguments: {self._lib.rope_last_error(self._ctx).decode()}")
        self._check(rc, entry)
        return out

    # -- the native camera and bundle polish (csrc/rope_bundle_polish.hip) ----------------------------
    def _bundle_call(self, name: str, N: int, outs, call):
        """The launch the bundle exports share: outputs allocated on the device, the call on torch's current stream."""
        import torch
        dev = torch.device('cuda', self.device)
        with torch.cuda.device(dev):
            tensors = [torch.empty(shape, dtype=torch.float64, device=dev) for shape in outs]
            if N > 0:
                work = torch.empty(max(1, self._lib.rope_bundle_schur_workspace(int(N)) // 8), dtype=torch.float64, device=dev)
                rc = call(_dp(work), [_dp(t) for t in tensors],
                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
                if rc:
                    raise EngineError(f"{name} failed ({rc})")
        return tensors

    def bundle_pool(self, words):
        """rope_bundle_pool: (N, 96) words -> (96,) float64 tensor on the device, the frames added in frame order, bit-equal to
        refinement.pool_bundle.  Runs on torch's current stream; nothing is waited for."""
        import torch
        w = self._polish_tensor('words', words, BNEQ_WORDS)
        if w.shape[0] == 0:
            return torch.zeros(BNEQ_WORDS, dtype=torch.float64, device=w.device)
        return self._bundle_call('rope_bundle_pool', w.shape[0], [(BNEQ_WORDS,)],
                                 lambda work, o, s: self._lib.rope_bundle_pool(_dp(w), int(w.shape[0]), o[0], s))[0]

    def bundle_schur_step(self, words, pooled, q, pose, lam: float, joint_mask: int, camera_mask: int, limits):
        """rope_bundle_schur_step: refinement.schur_step on the device, then pose + dc and clip(q + dq) -> (trial_q (N, 6),
        trial_pose (6,)) float64 tensors on the device (include/rope_s3d.h).  words (N, 96), pooled (96,), q (N, 6), pose (6,): float64
        numpy arrays or tensors; lam ONE damping; limits (6, 2).  Runs on torch's current stream; nothing is waited for."""
        import torch
        w = self._polish_tensor('words', words, BNEQ_WORDS)
        N = w.shape[0]
        p_t, q_t, pose_t = self._polish_tensor('pooled', pooled, None, BNEQ_WORDS), self._polish_tensor('q', q, 6, N), self._polish_tensor('pose', pose, None, 6)
        lam_t = torch.tensor([float(lam)], dtype=torch.float64, device=w.device)
        jm, cm, limits = self._active_mask(joint_mask), self._active_mask(camera_mask), self._limits(limits)
        out = self._bundle_call('rope_bundle_schur_step', N, [(N, 6), (6,)], lambda work, o, s: self._lib.rope_bundle_schur_step(
            _dp(w), _dp(p_t), _dp(q_t), _dp(pose_t), _dp(lam_t), int(N), jm, cm, _p(limits), work, o[0], o[1], s))
        return out[0], out[1]

    def bundle_schur_variance(self, words, pooled, joint_mask: int, camera_mask: int):
        """rope_bundle_schur_variance: the SQUARE of refinement.schur_sigma -> (var_q (N, 6), var_pose (6,)) float64 tensors on the
        device: nan for what is not refined, inf where the views do not pin an unknown down.  Nothing is waited for."""
        w = self._polish_tensor('words', words, BNEQ_WORDS)
        N = w.shape[0]
        p_t = self._polish_tensor('pooled', pooled, None, BNEQ_WORDS)
        jm, cm = self._active_mask(joint_mask), self._active_mask(camera_mask)
        out = self._bundle_call('rope_bundle_schur_variance', N, [(N, 6), (6,)], lambda work, o, s: self._lib.rope_bundle_schur_variance(
            _dp(w), _dp(p_t), int(N), jm, cm, work, o[0], o[1], s))
        return out[0], out[1]

    @staticmethod
    def _slot_mask(slot_mask) -> int:
        if isinstance(slot_mask, bool) or int(slot_mask) != slot_mask or not 0 <= int(slot_mask) <= 4095:
            raise ValueError(f"slot_mask: bit c set = slot c is refined, 0 .. 4095, got {slot_mask!r}")
        return int(slot_mask)

    def bundle_columns_step(self, pooled, lam: float, slot_mask: int, pose, off, q0, limits):
        """rope_bundle_columns_step: refinement.bundle_columns_step on the device and what follows it -> (trial_pose (6,),
        trial_off (6,), trial_q (N, 6)) float64 tensors on the device: pose + d[6:], off + d[:6], clip(q0 + trial_off)."""
        import torch
        p_t = self._polish_tensor('pooled', pooled, None, BNEQ_WORDS)
        q_t = self._polish_tensor('q0', q0, 6)
        N = q_t.shape[0]
        pose_t, off_t = self._polish_tensor('pose', pose, None, 6), self._polish_tensor('off', off, None, 6)
        lam_t = torch.tensor([float(lam)], dtype=torch.float64, device=p_t.device)
        sm, limits = self._slot_mask(slot_mask), self._limits(limits)
        out = self._bundle_call('rope_bundle_columns_step', N, [(6,), (6,), (N, 6)], lambda work, o, s: self._lib.rope_bundle_columns_step(
            _dp(p_t), _dp(lam_t), sm, _dp(pose_t), _dp(off_t), _dp(q_t), int(N), _p(limits), o[0], o[1], o[2], s))
        return out[0], out[1], out[2]

    def bundle_columns_variance(self, pooled, slot_mask: int):
        """rope_bundle_columns_variance: the SQUARE of refinement.bundle_columns_sigma -> (12,) float64 tensor on the device."""
        p_t = self._polish_tensor('pooled', pooled, None, BNEQ_WORDS)
        sm = self._slot_mask(slot_mask)
        return self._bundle_call('rope_bundle_columns_variance', 1, [(12,)], lambda work, o, s: self._lib.rope_bundle_columns_variance(
            _dp(p_t), sm, o[0], s))[0]

    def refine_bundle_workspace(self, n_frames: int) -> int:
        """rope_refine_bundle_workspace: the bytes of device scratch refine_bundle needs for n_frames frames; 0 for a batch one
        call does not take."""
        return int(self._lib.rope_refine_bundle_workspace(self._ctx, int(n_frames)))

    def refine_bundle(self, mode: str, camera_pose, q, frame_depth, intr, znear: float, zfar: float, joint_mask: int, camera_mask: int,
                      limits, clip: float, iterations: int, damping: float, want_words: bool = False):
        """rope_refine_bundle: BundleRefiner.refine's depth loop inside the library — render, joint axes, twists, bundle normal
        equations, pool, the Schur ('frame') or twelve-column ('offset') Levenberg step kept only when the pooled cost falls, the
        formal variances — with everything but the render's rows on the device (include/rope_s3d.h).
        camera_pose (6,) and q (N, 6) host; frame_depth (N, H, W) float32 tensor on this engine's device, H x W the camera's; intr
        (fx, fy, cx, cy); znear, zfar those of set_camera.
        -> dict(pose (6,), angles (N, 6), offsets (6,) — nan in 'frame' mode —, var_pose (6,), var_joints ((N, 6) 'frame', (6,)
        'offset'), cost_before, cost_after, inliers (float), steps (int), frame_cost (N,) [, words (N, 96)]).  Complete on return."""
        if mode not in ('frame', 'offset'):
            raise ValueError(f"mode: 'frame' or 'offset', got {mode!r}")
        jm, cm, limits = self._active_mask(joint_mask), self._active_mask(camera_mask), self._limits(limits)
        if jm == 0 and cm == 0:
            raise ValueError("joint_mask and camera_mask: not both 0")
        frame_mode = mode == 'frame'
        fx, fy, cx, cy = (float(v) for v in intr)

        def outputs(N):
            o = dict(pose=np.empty(6), angles=np.empty((N, 6)), offsets=np.empty(6), var_pose=np.empty(6),
                     var_joints=np.empty((N, 6) if frame_mode else 6), costs=np.empty(3), steps=np.zeros(1, np.int32), frame_cost=np.empty(N))
            if want_words:
                o['words'] = np.empty((N, BNEQ_WORDS))
            return o

        o = self._native_refine('rope_refine_bundle', self.refine_bundle_workspace, q, frame_depth, camera_pose, iterations, damping, 1, outputs,
                                lambda q, pose, depth, N, work, o: self._lib.rope_refine_bundle(
                                    self._ctx, 0 if frame_mode else 1, pose, q, depth, N, fx, fy, cx, cy, float(znear), float(zfar), jm, cm, _p(limits),
                                    float(clip), int(iterations), float(damping), work, _p(o['pose']), _p(o['angles']), _p(o['offsets']),
                                    _p(o['var_pose']), _p(o['var_joints']), _p(o['costs']), _p(o['steps']), _p(o['frame_cost']), _p(o.get('words'))))
        costs = o.pop('costs')
        o.update(cost_before=float(costs[0]), cost_after=float(costs[1]), inliers=float(costs[2]), steps=int(o['steps'][0]))
        return o

    def debug_targets(self, want_tsweep: bool = False):
        """rope_debug_targets: the resident set back on the host -> (tq (N,H,W) uint64, t32 (N,H,W) float32, tsweep planes or None,
        flags (N,8) uint8), for tests."""
        n = self.n_targets
        tq, t32 = np.empty((n, self.H, self.W), np.uint64), np.empty((n, self.H, self.W), np.float32)
        ts = np.empty((n, self.H, self.W), np.float32) if want_tsweep else None
        flags = np.empty((n, 8), np.uint8)
        self._check(self._lib.rope_debug_targets(self._ctx, _p(tq), _p(t32), _p(ts), _p(flags)), 'rope_debug_targets')
        return tq, t32, ts, flags

    def resident_depth(self) -> np.ndarray:
        """The whole-depth float32 planes of the resident set (the ones ROPE_LOSS_TSWEEP reads; a set staged with want_tsweep has
        them) -> (N, H, W) float32 on the host: rope_debug_targets asked for that one plane stack and nothing else."""
        ts = np.empty((self.n_targets, self.H, self.W), np.float32)
        self._check(self._lib.rope_debug_targets(self._ctx, None, None, _p(ts), None), 'rope_debug_targets')
        return ts

    def eval_targets(self, cand, frame_of, n_render: int, loss: int, crop=None) -> np.ndarray:
        """Row i of `cand` scored against the resident target frame_of[i] -> errors (R,)."""
        cand = np.ascontiguousarray(cand, np.float64).reshape(-1, 6)
        fo = np.ascontiguousarray(frame_of, np.int32).reshape(-1)
        if len(fo) != len(cand):
            raise ValueError("one frame index per row")
        crop_a = np.ascontiguousarray(crop, np.int32) if crop is not None else None
        err = np.empty(len(cand), np.float64)
        self._check(self._lib.rope_eval_targets(self._ctx, _p(cand), _p(fo), len(cand), int(n_render), int(loss), _p(crop_a), _p(err)), 'rope_eval_targets')
        return err

    def lookup_score_targets(self, want_scores: bool = False):
        """The stored table against every resident target -> (scores (N, rows) or None, first-argmin row per frame, its score per frame)."""
        n = self.n_targets
        scores = np.empty((n, self._table_rows), np.float64) if want_scores else None
        bi, be = np.empty(n, np.int32), np.empty(n, np.float64)
        self._check(self._lib.rope_lookup_score_targets(self._ctx, _p(bi), _p(be), _p(scores)), 'rope_lookup_score_targets')
        return scores, bi, be

    def _predict_args(self, stages, limits, camera_pose, min_ang_inc, lookup_angles, lookup_crop, use_table, speculate, lookup_live):
        arr = stages if isinstance(stages, C.Array) else (StageDesc * len(stages))(*stages)
        limits = np.ascontiguousarray(limits, np.float64).reshape(6, 2)
        cam = np.ascontiguousarray(camera_pose, np.float64).reshape(6)
        inc = np.ascontiguousarray(min_ang_inc, np.float64).reshape(6)
        grid = np.ascontiguousarray(lookup_angles, np.float64).reshape(-1, 6) if lookup_angles is not None else None
        crop = np.ascontiguousarray(lookup_crop, np.int32).reshape(4) if lookup_crop is not None else None
        if lookup_live is not None:                  # the reference's table aliasing: edited in place by the library
            if grid is None or lookup_live.shape != grid.shape or lookup_live.dtype != np.float64 or not lookup_live.flags.c_contiguous:
                raise ValueError("lookup_live must be a C-contiguous float64 array of the grid's shape")
        a = PredictArgs(arr, len(arr), int(speculate), _p(limits), _p(cam), _p(inc), _p(grid), 0 if grid is None else len(grid),
                        1 if use_table else 0, _p(crop), _p(lookup_live))
        return a, (arr, limits, cam, inc, grid, crop, lookup_live)          # the arrays the struct points into stay alive with the tuple

    def predict_batch(self, stages, limits, camera_pose, min_ang_inc, lookup_angles=None, lookup_crop=None, use_table=False,
                      speculate: int = 3):
        """rope_predict_batch: the stage machine over all resident targets in lockstep.
        -> (angles (N, 6), trace (N, n_stages, 6), candidate poses evaluated)."""
        a, keep = self._predict_args(stages, limits, camera_pose, min_ang_inc, lookup_angles, lookup_crop, use_table, speculate, None)
        n = self.n_targets
        out, trace, cnt = np.empty((n, 6)), np.empty((n, a.n_stages, 6)), C.c_int64()
        self._check(self._lib.rope_predict_batch(self._ctx, C.byref(a), n, _p(out), _p(trace), C.byref(cnt)), 'rope_predict_batch')
        return out, trace, int(cnt.value)

    # -- evaluation ---------------------------------------------------------------------------
    def upload_candidates(self, cand: np.ndarray):
        cand = np.ascontiguousarray(cand, np.float64).reshape(-1, 6)
        self._check(self._lib.rope_candidates_upload(self._ctx, _p(cand), len(cand)), 'rope_candidates_upload')
        self.n_candidates = len(cand)

    def eval_resident(self, n_render: int, loss: int, crop=None):
        crop_a = np.ascontiguousarray(crop, np.int32) if crop is not None else None
        self._check(self._lib.rope_eval_resident(self._ctx, int(n_render), int(loss), _p(crop_a)), 'rope_eval_resident')

    def sync(self):
        self._check(self._lib.rope_sync(self._ctx), 'rope_sync')

    def download(self, want_err=True, want_sums=False):
        n = self.n_candidates
        err = np.empty(n, np.float64) if want_err else None
        sums = np.empty((n, SUM_WORDS), np.uint64) if want_sums else None
        bi, be = C.c_int32(), C.c_double()
        self._check(self._lib.rope_results_download(self._ctx, _p(err), _p(sums), C.byref(bi), C.byref(be)), 'rope_results_download')
        return err, sums, int(bi.value), float(be.value)

    MAX_BATCH = 65535          # candidates per launch (grid y dimension)

    def eval(self, cand, n_render: int, loss: int, crop=None, want_sums=False):
        """-> (err (C,), sums or None, first-argmin index, its error).  Any number of candidates: batches beyond
        65 535 rows are evaluated in several launches and merged (first index of the smallest error, NaN never wins)."""
        cand = np.ascontiguousarray(cand, np.float64).reshape(-1, 6)
        if len(cand) <= self.MAX_BATCH:
            # one call across the boundary: upload + enqueue + sync + download (rope_eval)
            n = len(cand)
            err = np.empty(n, np.float64)
            sums = np.empty((n, SUM_WORDS), np.uint64) if want_sums else None
            crop_a = np.ascontiguousarray(crop, np.int32) if crop is not None else None
            bi, be = C.c_int32(), C.c_double()
            self._check(self._lib.rope_eval(self._ctx, _p(cand), n, int(n_render), int(loss), _p(crop_a), _p(err), _p(sums),
                                            C.byref(bi), C.byref(be)), 'rope_eval')
            self.n_candidates = n
            return err, sums, int(bi.value), float(be.value)
        errs, sums, best, best_err = [], [], -1, np.nan
        for lo in range(0, len(cand), self.MAX_BATCH):
            e, s, bi, be = self.eval(cand[lo:lo + self.MAX_BATCH], n_render, loss, crop, want_sums)
            errs.append(e)
            sums.append(s)
            if best < 0 or be < best_err or (np.isnan(best_err) and not np.isnan(be)):
                best, best_err = lo + bi, be
        self.n_candidates = min(len(cand) - (len(cand) - 1) // self.MAX_BATCH * self.MAX_BATCH, self.MAX_BATCH)
        return np.concatenate(errs), (np.concatenate(sums) if want_sums else None), best, best_err

    def lookup_build(self, cand, n_render: int, crop):
        """Render the pose grid once into an HBM-resident table of cropped sqrt-depth images."""
        cand = np.ascontiguousarray(cand, np.float64).reshape(-1, 6)
        crop_a = np.ascontiguousarray(crop, np.int32)
        self._check(self._lib.rope_lookup_build(self._ctx, _p(cand), len(cand), int(n_render), _p(crop_a)), 'rope_lookup_build')
        self.n_candidates = len(cand)
        self._table_rows = len(cand)

    def lookup_score(self, want_scores: bool = False):
        """-> (scores or None, first-argmin row, its score) of the stored table against the current target."""
        scores = np.empty(self._table_rows, np.float64) if want_scores else None
        bi, be = C.c_int32(), C.c_double()
        self._check(self._lib.rope_lookup_score(self._ctx, _p(scores), C.byref(bi), C.byref(be)), 'rope_lookup_score')
        return scores, int(bi.value), float(be.value)

    def predict(self, stages, limits, camera_pose, min_ang_inc, lookup_angles=None, lookup_crop=None, use_table=False,
                speculate: int = 3, lookup_live: np.ndarray = None, on_eval=None):
        """rope_predict: the whole stage machine of one frame in one call.  `stages` = StageDesc array (or list).  `on_eval`:
        callable(stage index, n_render, rows (R, 6)) after every scored batch of a stage, handed a copy of the rows (on_eval of
        rope_predict_args; it must not use this engine).  -> (angles (6,), trace (n_stages, 6), candidate poses evaluated)."""
        a, keep = self._predict_args(stages, limits, camera_pose, min_ang_inc, lookup_angles, lookup_crop, use_table, speculate, lookup_live)
        if on_eval is not None:
            hook = EvalHook(lambda _, stage, n_render, rows, n: on_eval(stage, n_render, np.ctypeslib.as_array(rows, (n, 6)).copy()))
            a.on_eval = hook                            # `hook` lives until the call returns
        out, trace, n = np.empty(6), np.empty((a.n_stages, 6)), C.c_int64()
        self._check(self._lib.rope_predict(self._ctx, C.byref(a), _p(out), _p(trace), C.byref(n)), 'rope_predict')
        return out, trace, int(n.value)

    def render(self, q, n_render: int = 6):
        """-> (depth float32 HxW metres, link id uint8 HxW with 255 = background)."""
        q = np.ascontiguousarray(q, np.float64).reshape(6)
        depth = np.empty((self.H, self.W), np.float32)
        ids = np.empty((self.H, self.W), np.uint8)
        self._check(self._lib.rope_render(self._ctx, _p(q), int(n_render), _p(depth), _p(ids)), 'rope_render')
        return depth, ids

    def render_batch(self, q, n_render: int = 6, PV=None, crop=None, depth: bool = True, ids: bool = True):
        """rope_render_batch: N poses in one device batch.  q (N, 6); PV (N, 4, 4) per-pose P·V or None = the camera of
        set_camera (which stays the context's camera); crop (r0, r1, c0, c1) inclusive or None = whole frame.
        -> (depth (N, h, w) float32 metres | None, ids (N, h, w) uint8, 255 = background | None), h x w the crop."""
        q = np.ascontiguousarray(q, np.float64).reshape(-1, 6)
        N = len(q)
        if PV is not None:
            PV = np.ascontiguousarray(PV, np.float64).reshape(-1, 16)
            if len(PV) != N:
                raise ValueError(f"render_batch: {len(PV)} view matrices for {N} poses")
        crop_arr = None
        h, w = self.H, self.W
        if crop is not None:
            crop_arr = np.ascontiguousarray(crop, np.int32).reshape(4)
            h, w = int(crop_arr[1]) - int(crop_arr[0]) + 1, int(crop_arr[3]) - int(crop_arr[2]) + 1
        if N and (h < 1 or w < 1):
            raise ValueError(f"render_batch: empty crop {tuple(crop_arr)}")
        d = np.empty((N, max(h, 0), max(w, 0)), np.float32) if depth else None
        i = np.empty((N, max(h, 0), max(w, 0)), np.uint8) if ids else None
        if N == 0:
            return d, i
        self._check(self._lib.rope_render_batch(self._ctx, _p(q), _p(PV), N, int(n_render), _p(crop_arr), _p(d), _p(i)), 'rope_render_batch')
        return d, i

    def render_batch_device(self, q, n_render: int = 6, PV=None):
        """rope_render_batch_device: render_batch for the whole frame with the planes left on the GPU
        -> (depth (N, H, W) float32, ids (N, H, W) uint8) torch tensors on this engine's device, complete on return."""
        import torch
        q = np.ascontiguousarray(q, np.float64).reshape(-1, 6)
        N = len(q)
        if PV is not None:
            PV = np.ascontiguousarray(PV, np.float64).reshape(-1, 16)
            if len(PV) != N:
                raise ValueError(f"render_batch_device: {len(PV)} view matrices for {N} poses")
        device = torch.device('cuda', self.device)
        d = torch.empty((N, self.H, self.W), dtype=torch.float32, device=device)
        i = torch.empty((N, self.H, self.W), dtype=torch.uint8, device=device)
        if N == 0:
            return d, i
        # fresh tensors may be memory that earlier work has not finished with: torch's allocator hands a freed block back to the
        # stream it was allocated on, in that stream's order, so that stream alone is waited for (the context draws on its own)
        torch.cuda.current_stream(device).synchronize()
        self._check(self._lib.rope_render_batch_device(self._ctx, _p(q), _p(PV), N, int(n_render), C.c_void_p(d.data_ptr()),
                                                       C.c_void_p(i.data_ptr())), 'rope_render_batch_device')
        return d, i

    def render_masks(self, q, n_render: int, label_of_link, pad: int, PV=None):
        """rope_render_masks: N poses to label bit planes, each label dilated by a pad x pad window (cv2.dilate's anchor), in
        device batches.  label_of_link: n_render bits (0..7, 255 = none); PV (N, 4, 4) per-pose P·V or None = the camera of
        set_camera.  -> (masks (N, H, W) uint8, boxes (N, 8, 4) int32 {r0, r1, c0, c1} per label bit, -1 when empty)."""
        q = np.ascontiguousarray(q, np.float64).reshape(-1, 6)
        N = len(q)
        lab = np.ascontiguousarray(label_of_link, np.uint8).reshape(-1)
        if len(lab) != int(n_render):
            raise ValueError(f"render_masks: {len(lab)} labels for {n_render} links")
        if PV is not None:
            PV = np.ascontiguousarray(PV, np.float64).reshape(-1, 16)
            if len(PV) != N:
                raise ValueError(f"render_masks: {len(PV)} view matrices for {N} poses")
        masks = np.empty((N, self.H, self.W), np.uint8)
        boxes = np.empty((N, 8, 4), np.int32)
        if N == 0:
            return masks, boxes
        self._check(self._lib.rope_render_masks(self._ctx, _p(q), _p(PV), N, int(n_render), _p(lab), int(pad), _p(masks), _p(boxes)),
                    'rope_render_masks')
        return masks, boxes

    @staticmethod
    def trace_contours(mask: np.ndarray, bit: int, box=None, min_points: int = 0) -> list:
        """engine.trace_contours: host code, no context needed."""
        return trace_contours(mask, bit, box, min_points)

    def coverage(self, cand, n_render: int) -> np.ndarray:
        cand = np.ascontiguousarray(cand, np.float64).reshape(-1, 6)
        cover = np.empty((self.H, self.W), np.uint8)
        self._check(self._lib.rope_coverage(self._ctx, _p(cand), len(cand), int(n_render), _p(cover)), 'rope_coverage')
        self.n_candidates = len(cand)
        return cover

    # -- camera-pose path ------------------------------------------------------------------------
    def set_frames(self, q, tq, t32=None, link_planes=None):
        """N frames: joint vectors (N,6), uint64 depth planes (N,H,W), optional float32 planes (N,H,W) and per-link
        planes (N,6,H,W) — the targets every candidate camera is scored against (rope_set_frames)."""
        q = np.ascontiguousarray(q, np.float64).reshape(-1, 6)
        n = len(q)
        tq = np.ascontiguousarray(tq, np.uint64)
        if tq.shape != (n, self.H, self.W):
            raise ValueError(f"frame planes must be {(n, self.H, self.W)}, got {tq.shape}")
        if t32 is not None:
            t32 = np.ascontiguousarray(t32, np.float32)
            if t32.shape != tq.shape:
                raise ValueError("float32 frame planes have the wrong shape")
        if link_planes is not None:
            link_planes = np.ascontiguousarray(link_planes, np.uint64)
            if link_planes.shape != (n, 6, self.H, self.W):
                raise ValueError("link planes must be (N, 6, H, W)")
        self._check(self._lib.rope_set_frames(self._ctx, n, _p(q), _p(tq), _p(t32), _p(link_planes)), 'rope_set_frames')
        self.n_frames = n

    def eval_views(self, PV, n_render: int, loss: int) -> np.ndarray:
        """K candidate cameras (K,4,4 P·V) x the resident frames -> (K, N, 23) exact integer sums."""
        PV = np.ascontiguousarray(PV, np.float64).reshape(-1, 4, 4)
        sums = np.empty((len(PV), self.n_frames, SUM_WORDS), np.uint64)
        self._check(self._lib.rope_eval_views(self._ctx, _p(PV), len(PV), int(n_render), int(loss), _p(sums)), 'rope_eval_views')
        self.n_candidates = len(PV) * self.n_frames
        return sums

    def debug_mvp(self, C_: int, n_render: int) -> np.ndarray:
        out = np.empty((C_, n_render, 16), np.float32)
        self._check(self._lib.rope_debug_mvp(self._ctx, _p(out), int(C_), int(n_render)), 'rope_debug_mvp')
        return out

    NO_LAYERS, NO_SPLIT, NO_PARENTS, NO_QUEUE, CLIP_KERNELS, SEPARATE_GEOMETRY, NO_GEOMETRY_CACHE, NO_KEPT_FRAGMENTS = 1, 2, 4, 8, 16, 32, 64, 128

    def set_strategy(self, flags: int):
        """rope_set_strategy: launch structure only (shared layers / small-batch split / second sharing level off);
        results are bit-identical for every value."""
        self._check(self._lib.rope_set_strategy(self._ctx, int(flags)), 'rope_set_strategy')
        self._strategy = int(flags)

    def geometry_cache_stats(self):
        """rope_geometry_cache_stats -> (hits, misses): large layered passes that ran on the geometry the pass before left / built it."""
        hits, misses = C.c_uint64(), C.c_uint64()
        self._check(self._lib.rope_geometry_cache_stats(self._ctx, C.byref(hits), C.byref(misses)), 'rope_geometry_cache_stats')
        return int(hits.value), int(misses.value)

    def fragment_store_stats(self):
        """rope_fragment_store_stats -> (builds, passes_served, bytes, groups): fragment stores built and passes scored from one so
        far; size of the store held now (0, 0: none)."""
        v = [C.c_uint64() for _ in range(4)]
        self._check(self._lib.rope_fragment_store_stats(self._ctx, *(C.byref(x) for x in v)), 'rope_fragment_store_stats')
        return tuple(int(x.value) for x in v)

    def fragment_store_pairs(self) -> int:
        """rope_fragment_store_pairs: (row, tile) pairs of the store held now that keep any group."""
        v = C.c_uint64()
        self._check(self._lib.rope_fragment_store_pairs(self._ctx, C.byref(v)), 'rope_fragment_store_pairs')
        return int(v.value)

    def set_fragment_budget(self, mib: float = None):
        """rope_set_fragment_budget: most memory a grid's kept fragments may take, in MiB; None: the lookup table's default
        (simulation.lookup.DEFAULT_LOOKUP_VRAM_MIB x GPU_MEMORY_ALLOWED_FOR_LOOKUP)."""
        if mib is None:
            from .constants import GPU_MEMORY_ALLOWED_FOR_LOOKUP
            from .simulation.lookup import DEFAULT_LOOKUP_VRAM_MIB
            mib = DEFAULT_LOOKUP_VRAM_MIB * GPU_MEMORY_ALLOWED_FOR_LOOKUP
        self._check(self._lib.rope_set_fragment_budget(self._ctx, int(mib * (1 << 20))), 'rope_set_fragment_budget')

    def debug_skip(self, mask: int):
        """Kernel-phase ablation; only the profiling build of the library has it (tools/build_variants.py profile)."""
        if not hasattr(self._lib, 'rope_debug_skip'):
            raise EngineError("rope_debug_skip: not in this library; build librope_hip_profile.so and point ROPE_HIP_LIB at it")
        self._check(self._lib.rope_debug_skip(self._ctx, int(mask)), 'rope_debug_skip')

    def debug_clock(self):
        """Profiling build only: (shader clock in GHz during the last scoring launch of a large batch, that launch's length in ms),
        from s_memtime / s_memrealtime stamps of its workgroups."""
        if not hasattr(self._lib, 'rope_debug_clock'):
            raise EngineError("rope_debug_clock: not in this library; build librope_hip_profile.so and point ROPE_HIP_LIB at it")
        out = np.zeros(2)
        self._check(self._lib.rope_debug_clock(self._ctx, _p(out)), 'rope_debug_clock')
        return float(out[0]), float(out[1])

    def debug_bounds(self) -> int:
        """Profiling build only: indices into the raster kernels' shared arrays / queue segments found out of range so far."""
        if not hasattr(self._lib, 'rope_debug_bounds'):
            raise EngineError("rope_debug_bounds: not in this library; build librope_hip_profile.so and point ROPE_HIP_LIB at it")
        v = C.c_int()
        self._check(self._lib.rope_debug_bounds(self._ctx, C.byref(v)), 'rope_debug_bounds')
        return int(v.value)

    def profile_eval(self, n_render: int, loss: int, crop=None, reps: int = 10):
        """-> dict of average milliseconds per pass (HIP events on the engine stream): fk (+bounds), layer (shared
        upstream links), score (per-candidate raster + loss), finalize (+argmin), total; raster = layer + score."""
        crop_a = np.ascontiguousarray(crop, np.int32) if crop is not None else None
        ms = np.zeros(5, np.float32)
        self._check(self._lib.rope_profile_eval(self._ctx, int(n_render), int(loss), _p(crop_a), int(reps), _p(ms)), 'rope_profile_eval')
        return {'fk': float(ms[0]), 'layer': float(ms[1]), 'score': float(ms[2]), 'raster': float(ms[1] + ms[2]),
                'finalize': float(ms[3]), 'total': float(ms[4])}
