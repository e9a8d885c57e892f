"""ctypes binding of das3r_amd/libdas3r_hip.so (C-ABI: include/das3r_raster.h).

The product path has NO fallback: if the HIP library is missing or a call fails, a RuntimeError is raised.
PyTorch is used only for device memory (allocations handed to the library through the allocator callbacks)
and for the current HIP stream.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdas3r_hip.so")
ABI_VERSION = 16
NO_BACKWARD_IN_FLAG = 8   # das3r_raster_saved.flags bit 3 on the way in to das3r_raster_forward: no backward pass will follow
ANTIALIAS_FLAG = 16       # das3r_raster_saved.flags bit 4: an antialiased forward (asked for on the way in, set again on the way out)
ERR_INVALID_ARG = -1      # DAS3R_ERR_INVALID_ARG
AUX_MAX_CHANNELS = 8     # DAS3R_AUX_MAX_CHANNELS: channels per das3r_raster_aux_forward / _adjoint call

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)


class RasterArgs(C.Structure):
    _fields_ = [("P", C.c_int32), ("sh_degree", C.c_int32), ("M", C.c_int32), ("image_width", C.c_int32),
                ("image_height", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
                ("bg", C.c_void_p), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p),
                ("prefiltered", C.c_int32), ("debug", C.c_int32), ("capacity_hint", C.c_int64)]


class PreTransform(C.Structure):
    """include/das3r_raster.h das3r_pretransform (ABI 14): raw model parameters + pose, taken by the rasterizer's own kernels."""
    _fields_ = [("xyz", C.c_void_p), ("rot", C.c_void_p), ("scaling", C.c_void_p), ("opacity_raw", C.c_void_p), ("conf_flat", C.c_void_p),
                ("mask_index", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p), ("Lq", C.c_void_p)]


class RasterIn(C.Structure):
    _fields_ = [("means3D", C.c_void_p), ("opacities", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
                ("scales", C.c_void_p), ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p), ("pre", C.POINTER(PreTransform))]


class RasterOut(C.Structure):
    _fields_ = [("out_color", C.c_void_p), ("radii", C.c_void_p), ("out_invdepth", C.c_void_p)]   # ABI 16: + out_invdepth ([H, W] or NULL)


class RasterSaved(C.Structure):
    _fields_ = [("geom", C.c_void_p), ("binning", C.c_void_p), ("img", C.c_void_p), ("num_rendered", C.c_int64), ("capacity", C.c_int64),
                ("check_word", C.c_void_p), ("check_tag", C.c_uint32), ("flags", C.c_uint32)]


class AdamSlot(C.Structure):
    """include/das3r_raster.h das3r_adam_slot (ABI 11)."""
    _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("step_size", C.c_float), ("bc2_sqrt", C.c_float)]


class Chain(C.Structure):
    """include/das3r_raster.h das3r_chain (ABI 14): the rasterizer's backward goes on through the pose pre-transform and the Adam step."""
    _fields_ = [("g_conf_flat", C.c_void_p), ("g_small", C.c_void_p), ("slots", C.POINTER(AdamSlot)), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float)]


class RasterGrads(C.Structure):
    _fields_ = [("dL_dmeans2D", C.c_void_p), ("dL_dopacities", C.c_void_p), ("dL_dmeans3D", C.c_void_p),
                ("dL_dshs", C.c_void_p), ("dL_dcolors_precomp", C.c_void_p), ("dL_dscales", C.c_void_p),
                ("dL_drotations", C.c_void_p), ("dL_dcov3D", C.c_void_p), ("scratch", C.c_void_p), ("chain", C.POINTER(Chain))]


class PruneTensor(C.Structure):
    """include/das3r_raster.h das3r_prune_tensor: one row-major tensor of das3r_prune_compact."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int64)]


class PathPolicyState(C.Structure):
    """include/das3r_raster.h das3r_path_policy_state: what the forwards of a shape have learnt (csrc/path_policy.h Verdict + Resume)."""
    _fields_ = [("P", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("last_I", C.c_int64), ("peak_I", C.c_int64), ("radix_left", C.c_int32),
                ("backoff", C.c_int32), ("gen", C.c_uint32), ("seg_extra", C.c_int32), ("last_seg", C.c_int32), ("fine", C.c_int32),
                ("forwards", C.c_uint32), ("clean", C.c_uint32), ("longest", C.c_uint32), ("resume_valid", C.c_int32), ("resume_fine", C.c_int32),
                ("resume_forwards", C.c_uint32)]


class PathPolicyInputs(C.Structure):
    """include/das3r_raster.h das3r_path_policy_inputs: what a forward's plan reads besides the state."""
    _fields_ = [("P", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("ntiles", C.c_int32), ("tbits", C.c_int32), ("tile_passes", C.c_int32),
                ("too_long", C.c_uint32), ("want_bits", C.c_uint32), ("forced", C.c_int32), ("onesweep", C.c_int32), ("capacity_hint", C.c_int64),
                ("capacity_exact", C.c_int32)]


class PathPolicyPlan(C.Structure):
    """include/das3r_raster.h das3r_path_policy_plan."""
    _fields_ = [("local", C.c_int32), ("seg", C.c_int32), ("seg_bits", C.c_int32), ("seg_passes", C.c_int32), ("speculate", C.c_int32),
                ("decide_fine", C.c_int32), ("gen", C.c_uint32), ("cells", C.c_int32), ("cap", C.c_int64)]


class Switches(C.Structure):
    """include/das3r_raster.h das3r_switches: the DAS3R_* switches as parsed (csrc/kernel_choice.h Switches)."""
    _fields_ = [(n, C.c_int32) for n in
                ("sort_ipl", "sort_classic", "rect_upstream", "verbose", "binning", "capacity_exact", "fused_emit_off", "no_sh_stage", "render_fwd",
                 "render_bwd", "render_bwd_mb", "render_bwd_atomic", "render_bwd_pix", "render_bwd_occ", "render_bwd_strips", "tile_chunk",
                 "scan_items", "deterministic", "tile_lpt_off", "bwd_reduce_set", "bwd_reduce_shfl", "ablate_set", "ablate", "tickets",
                 "bwd_pad_lds", "fwd_pad_lds", "bwd_buckets", "fwd_no_prefetch", "split_colour", "tile_strip")]


class BwdChoice(C.Structure):
    """include/das3r_raster.h das3r_bwd_choice."""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "mb", "slices", "pix", "occ", "strips", "atomic_flush")]


class FwdChoice(C.Structure):
    """include/das3r_raster.h das3r_fwd_choice."""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "quad_lanes", "row_private", "tile_lpt")]


class PreprocessBackwardInputs(C.Structure):
    """include/das3r_raster.h das3r_preprocess_backward_inputs (csrc/preprocess_choice.h PreprocessBackwardInputs)."""
    _fields_ = [(n, C.c_int32) for n in ("has_sh", "has_cov", "M", "sh_degree", "shs_aligned16", "dL_dshs_aligned16", "no_sh_stage", "jac_saved",
                                         "chained", "quad_rows", "depth", "aa")]


class PreprocessForm(C.Structure):
    """include/das3r_raster.h das3r_preprocess_form: preprocess_backward_kernel's nine template arguments + base_index, sh_rows_staged."""
    _fields_ = [(n, C.c_int32) for n in ("has_sh", "has_cov", "stage_in", "stage_out", "deg0", "chain", "depth", "jac", "aa", "base_index",
                                         "sh_rows_staged")]


PRUNE_GROUP_ROWS = 1024   # DAS3R_PRUNE_GROUP_ROWS
TSDF_MAX_VIEWS = 16       # DAS3R_TSDF_MAX_VIEWS: views per launch of das3r_tsdf_integrate (more are taken in chunks)
TSDF_MAX_VOXELS = 1 << 28 # DAS3R_TSDF_MAX_VOXELS


def prune_count_words(P):
    """DAS3R_PRUNE_COUNT_WORDS(P): int32 words of das3r_prune_select's `count` (word 0 = kept rows, the rest scratch)."""
    return 1 + (int(P) + PRUNE_GROUP_ROWS - 1) // PRUNE_GROUP_ROWS


class RasterLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in
                ("geom_bytes", "binning_bytes", "img_bytes", "depth_key", "xy", "conic_opacity", "rgbd", "splat_stride", "clamped",
                 "tiles_touched", "sorted_idx", "offsets", "point_list", "final_T", "n_contrib", "ranges")]


# every symbol include/das3r_raster.h declares
EXPORTS = ("das3r_raster_forward", "das3r_raster_backward", "das3r_raster_backward_depth", "das3r_raster_backward_depth_scratch_bytes", "das3r_raster_check", "das3r_raster_backward_scratch_bytes", "das3r_mark_visible", "das3r_knn3_workspace_bytes",
           "das3r_knn3_mean_dist2", "das3r_raster_get_layout", "das3r_abi_version", "das3r_last_error", "das3r_reload_switches", "das3r_get_stats",
           "das3r_raster_forget_shapes", "das3r_raster_learning",
           "das3r_profile_enable", "das3r_profile_report", "das3r_pretransform_forward", "das3r_pretransform_backward", "das3r_pose_matrices", "das3r_pose_chain",
           "das3r_adam_step", "das3r_adam_step_gated", "das3r_photometric_blocks", "das3r_photometric_forward", "das3r_photometric_backward",
           "das3r_has_experiments", "das3r_pair_counters", "das3r_debug_poison_lds", "das3r_debug_inject_fault", "das3r_debug_mutate",
           "das3r_pose_matrices_qt", "das3r_pose_chain_qt", "das3r_photometric_finish", "das3r_pretransform_backward_adam", "das3r_pretransform_pose_sums",
           "das3r_raster_count_live_pairs", "das3r_photometric_backward_finish", "das3r_pose_chain_qt_rearm", "das3r_ssim_map_forward", "das3r_ssim_map_backward",
           "das3r_split_colour_rule", "das3r_split_colour_switch", "das3r_depth_l1_blocks", "das3r_depth_l1", "das3r_prune_select", "das3r_prune_compact",
           "das3r_photometric_forward_exposure", "das3r_photometric_backward_finish_exposure", "das3r_exposure_grad_finish",
           "das3r_raster_aux_forward", "das3r_raster_aux_scratch_bytes", "das3r_raster_aux_adjoint",
           "das3r_raster_aux_backward_scratch_bytes", "das3r_raster_aux_backward",
           "das3r_raster_distortion_forward", "das3r_raster_distortion_backward_scratch_bytes", "das3r_raster_distortion_backward",
           "das3r_raster_median_forward", "das3r_raster_median_scratch_bytes", "das3r_raster_median_adjoint",
           "das3r_gaussian_normals_forward", "das3r_gaussian_normals_backward", "das3r_normal_consistency_forward", "das3r_normal_consistency_backward",
           "das3r_thin_workspace_bytes", "das3r_thin_voxels", "das3r_raster_focal_workspace_bytes", "das3r_raster_backward_focal",
           "das3r_tsdf_integrate", "das3r_tsdf_extract_workspace_bytes", "das3r_tsdf_extract_count", "das3r_tsdf_extract_emit",
           "das3r_debug_tsdf_integrate_host", "das3r_debug_tsdf_extract_host", "das3r_debug_tsdf_swap_table",
           "das3r_mesh_components_workspace_bytes", "das3r_mesh_components", "das3r_mesh_filter_select", "das3r_mesh_filter_faces",
           "das3r_debug_mesh_components_host",
           "das3r_debug_path_policy_fresh", "das3r_debug_path_policy_plan", "das3r_debug_path_policy_count", "das3r_debug_path_policy_skew",
           "das3r_debug_path_policy_hint", "das3r_debug_path_policy_forget", "das3r_debug_path_policy_resume", "das3r_debug_seg_dbits",
           "das3r_debug_parse_switches", "das3r_debug_choose_backward", "das3r_debug_choose_forward", "das3r_debug_has_invdepth_form",
           "das3r_debug_kernel_name", "das3r_debug_choose_preprocess_backward", "das3r_debug_preprocess_backward_name")

_lib = None


def load():
    """Load libdas3r_hip.so (once).  Raises RuntimeError — never falls back — when it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"das3r_amd: HIP library not found at {LIB_PATH}. Build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or `make -C das3r_amd/csrc`. There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(L, name):
            raise RuntimeError(f"das3r_amd: {LIB_PATH} does not export {name}; rebuild it")
    L.das3r_abi_version.restype = C.c_int
    if L.das3r_abi_version() != ABI_VERSION:
        raise RuntimeError("das3r_amd: ABI version mismatch between the Python host layer and libdas3r_hip.so; rebuild")
    L.das3r_last_error.restype = C.c_char_p
    L.das3r_raster_forward.restype = C.c_int64
    L.das3r_raster_forward.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterIn), C.POINTER(RasterOut), ALLOC_FN, ALLOC_FN,
                                       ALLOC_FN, C.c_void_p, C.POINTER(RasterSaved), C.c_void_p]
    L.das3r_raster_backward.restype = C.c_int
    L.das3r_raster_backward.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterIn), C.POINTER(RasterSaved), C.c_void_p,
                                        C.POINTER(RasterGrads), C.c_void_p]
    L.das3r_raster_backward_scratch_bytes.restype = C.c_size_t
    L.das3r_raster_backward_depth.restype = C.c_int   # ABI 16
    L.das3r_raster_backward_depth.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterIn), C.POINTER(RasterSaved), C.c_void_p, C.c_void_p,
                                              C.POINTER(RasterGrads), C.c_void_p]
    L.das3r_raster_backward_depth_scratch_bytes.restype = C.c_size_t
    L.das3r_raster_backward_depth_scratch_bytes.argtypes = [C.c_int64]
    L.das3r_raster_backward_scratch_bytes.argtypes = [C.c_int64]
    L.das3r_raster_check.restype = C.c_int
    L.das3r_raster_check.argtypes = [C.POINTER(RasterSaved), C.c_void_p]
    L.das3r_raster_count_live_pairs.restype = C.c_int   # measurement aid (ABI 12)
    L.das3r_raster_count_live_pairs.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterSaved), C.POINTER(C.c_uint64), C.c_void_p]
    L.das3r_mark_visible.restype = C.c_int
    L.das3r_mark_visible.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_knn3_workspace_bytes.restype = C.c_size_t
    L.das3r_knn3_workspace_bytes.argtypes = [C.c_int32]
    L.das3r_knn3_mean_dist2.restype = C.c_int
    L.das3r_knn3_mean_dist2.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_pose_matrices.restype = C.c_int
    L.das3r_pose_matrices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_pose_chain.restype = C.c_int
    L.das3r_pose_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_pretransform_forward.restype = C.c_int
    L.das3r_pretransform_forward.argtypes = [C.c_int32] + [C.c_void_p] * 13 + [C.c_void_p]
    L.das3r_pretransform_backward.restype = C.c_int
    L.das3r_pretransform_backward.argtypes = [C.c_int32] + [C.c_void_p] * 18 + [C.c_void_p]
    L.das3r_pretransform_backward_adam.restype = C.c_int
    L.das3r_pretransform_backward_adam.argtypes = [C.c_int32] + [C.c_void_p] * 10 + [C.POINTER(AdamSlot), C.c_float, C.c_float, C.c_float, C.c_void_p]
    L.das3r_pretransform_pose_sums.restype = C.c_int
    L.das3r_pretransform_pose_sums.argtypes = [C.c_int32] + [C.c_void_p] * 7 + [C.c_void_p]
    L.das3r_photometric_blocks.restype = C.c_int64
    L.das3r_photometric_blocks.argtypes = [C.c_int32, C.c_int32]
    L.das3r_photometric_forward.restype = C.c_int
    L.das3r_photometric_forward.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_photometric_backward.restype = C.c_int
    L.das3r_photometric_backward.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_pose_matrices_qt.restype = C.c_int
    L.das3r_pose_matrices_qt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_pose_chain_qt.restype = C.c_int
    L.das3r_pose_chain_qt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_pose_chain_qt_rearm.restype = C.c_int
    L.das3r_pose_chain_qt_rearm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_ssim_map_forward.restype = C.c_int
    L.das3r_ssim_map_forward.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_ssim_map_backward.restype = C.c_int
    L.das3r_ssim_map_backward.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_photometric_backward_finish.restype = C.c_int
    L.das3r_photometric_backward_finish.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_photometric_forward_exposure.restype = C.c_int   # per-frame exposure compensation (additive under ABI 16)
    L.das3r_photometric_forward_exposure.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]
    L.das3r_photometric_backward_finish_exposure.restype = C.c_int
    L.das3r_photometric_backward_finish_exposure.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 9
    L.das3r_exposure_grad_finish.restype = C.c_int
    L.das3r_exposure_grad_finish.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_depth_l1_blocks.restype = C.c_int64
    L.das3r_depth_l1_blocks.argtypes = [C.c_int32, C.c_int32]
    L.das3r_depth_l1.restype = C.c_int
    L.das3r_depth_l1.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    L.das3r_prune_select.restype = C.c_int
    L.das3r_prune_select.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    L.das3r_prune_compact.restype = C.c_int
    L.das3r_prune_compact.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(PruneTensor), C.c_void_p]
    L.das3r_thin_workspace_bytes.restype = C.c_size_t   # voxel thinning (additive under ABI 16)
    L.das3r_thin_workspace_bytes.argtypes = [C.c_int32]
    L.das3r_thin_voxels.restype = C.c_int
    L.das3r_thin_voxels.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    i3, f3 = C.POINTER(C.c_int32), C.POINTER(C.c_float)   # TSDF fusion and mesh extraction (additive under ABI 16)
    integrate = [i3, f3, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, f3, f3, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                 C.c_void_p, C.c_float, C.c_float]
    L.das3r_tsdf_integrate.restype = C.c_int
    L.das3r_tsdf_integrate.argtypes = integrate + [C.c_void_p]
    L.das3r_debug_tsdf_integrate_host.restype = C.c_int
    L.das3r_debug_tsdf_integrate_host.argtypes = integrate
    L.das3r_tsdf_extract_workspace_bytes.restype = C.c_size_t
    L.das3r_tsdf_extract_workspace_bytes.argtypes = [i3]
    L.das3r_tsdf_extract_count.restype = C.c_int
    L.das3r_tsdf_extract_count.argtypes = [i3, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_tsdf_extract_emit.restype = C.c_int
    L.das3r_tsdf_extract_emit.argtypes = [i3, f3, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_debug_tsdf_extract_host.restype = C.c_int
    L.das3r_debug_tsdf_extract_host.argtypes = [i3, f3, C.c_float] + [C.c_void_p] * 9
    L.das3r_debug_tsdf_swap_table.restype = None
    L.das3r_debug_tsdf_swap_table.argtypes = [C.POINTER(C.c_uint32)]
    L.das3r_mesh_components_workspace_bytes.restype = C.c_size_t   # mesh clean-up: components, selection, face remap (additive under ABI 16)
    L.das3r_mesh_components_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.das3r_mesh_components.restype = C.c_int
    L.das3r_mesh_components.argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [i3, C.c_void_p, C.c_void_p]
    L.das3r_mesh_filter_select.restype = C.c_int
    L.das3r_mesh_filter_select.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, i3,
                                           C.c_void_p, C.c_void_p]
    L.das3r_mesh_filter_faces.restype = C.c_int
    L.das3r_mesh_filter_faces.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 4 + [C.c_void_p]
    L.das3r_debug_mesh_components_host.restype = C.c_int
    L.das3r_debug_mesh_components_host.argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * 5
    L.das3r_raster_focal_workspace_bytes.restype = C.c_size_t   # focal gradients beside a backward pass (additive under ABI 16)
    L.das3r_raster_focal_workspace_bytes.argtypes = [C.c_int32]
    L.das3r_raster_backward_focal.restype = C.c_int
    L.das3r_raster_backward_focal.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterIn), C.POINTER(RasterSaved), C.c_void_p, C.c_void_p,
                                              C.POINTER(RasterGrads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_raster_aux_forward.restype = C.c_int   # extra per-Gaussian channels over a forward's lists (additive under ABI 16)
    L.das3r_raster_aux_forward.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterSaved), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_raster_aux_scratch_bytes.restype = C.c_size_t
    L.das3r_raster_aux_scratch_bytes.argtypes = [C.c_int64, C.c_int32]
    L.das3r_raster_aux_adjoint.restype = C.c_int
    L.das3r_raster_aux_adjoint.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterSaved), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                           C.c_void_p]
    L.das3r_raster_aux_backward_scratch_bytes.restype = C.c_size_t   # aux channels / coverage: gradients to the geometry (additive under ABI 16)
    L.das3r_raster_aux_backward_scratch_bytes.argtypes = [C.c_int64, C.c_int32]
    L.das3r_raster_aux_backward.restype = C.c_int
    L.das3r_raster_aux_backward.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterIn), C.POINTER(RasterSaved), C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.POINTER(RasterGrads), C.c_void_p]
    L.das3r_raster_distortion_forward.restype = C.c_int   # the ray-distortion term over a forward's lists (additive under ABI 16)
    L.das3r_raster_distortion_forward.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterSaved), C.c_void_p, C.c_void_p, C.c_void_p]
    L.das3r_raster_distortion_backward_scratch_bytes.restype = C.c_size_t
    L.das3r_raster_distortion_backward_scratch_bytes.argtypes = [C.c_int64, C.c_int32]
    L.das3r_raster_distortion_backward.restype = C.c_int
    L.das3r_raster_distortion_backward.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterIn), C.POINTER(RasterSaved), C.c_void_p, C.c_void_p,
                                                   C.POINTER(RasterGrads), C.c_void_p]
    L.das3r_raster_median_forward.restype = C.c_int   # median depth and surface hits over a forward's lists (additive under ABI 16)
    L.das3r_raster_median_forward.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterSaved), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
    L.das3r_raster_median_scratch_bytes.restype = C.c_size_t
    L.das3r_raster_median_scratch_bytes.argtypes = [C.c_int64]
    L.das3r_raster_median_adjoint.restype = C.c_int
    L.das3r_raster_median_adjoint.argtypes = [C.POINTER(RasterArgs), C.POINTER(RasterSaved), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_void_p, C.c_void_p]
    L.das3r_gaussian_normals_forward.restype = C.c_int   # the normal-consistency regulariser's per-Gaussian and image kernels (additive under ABI 16)
    L.das3r_gaussian_normals_forward.argtypes = [C.POINTER(RasterArgs)] + [C.c_void_p] * 5 + [C.c_void_p]
    L.das3r_gaussian_normals_backward.restype = C.c_int
    L.das3r_gaussian_normals_backward.argtypes = [C.POINTER(RasterArgs)] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]
    L.das3r_normal_consistency_forward.restype = C.c_int
    L.das3r_normal_consistency_forward.argtypes = [C.c_int32, C.c_int32, C.c_float, C.c_float] + [C.c_void_p] * 6 + [C.c_void_p]
    L.das3r_normal_consistency_backward.restype = C.c_int
    L.das3r_normal_consistency_backward.argtypes = [C.c_int32, C.c_int32, C.c_float, C.c_float] + [C.c_void_p] * 7 + [C.c_void_p]
    L.das3r_photometric_finish.restype = C.c_int
    L.das3r_photometric_finish.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    L.das3r_adam_step_gated.restype = C.c_int
    L.das3r_adam_step_gated.argtypes = [C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    L.das3r_adam_step.restype = C.c_int
    L.das3r_adam_step.argtypes = [C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p]
    ps = C.POINTER(PathPolicyState)   # the binning-path policy on a caller's own state (additive under ABI 16; host-only)
    L.das3r_debug_path_policy_fresh.restype = None
    L.das3r_debug_path_policy_fresh.argtypes = [ps, C.c_uint32]
    L.das3r_debug_path_policy_plan.restype = None
    L.das3r_debug_path_policy_plan.argtypes = [ps, C.POINTER(PathPolicyInputs), C.POINTER(PathPolicyPlan)]
    L.das3r_debug_path_policy_count.restype = C.c_int
    L.das3r_debug_path_policy_count.argtypes = [ps, C.POINTER(PathPolicyInputs), C.POINTER(PathPolicyPlan), C.c_int64]
    L.das3r_debug_path_policy_skew.restype = C.c_int
    L.das3r_debug_path_policy_skew.argtypes = [ps, C.c_uint32, C.c_uint32, C.c_int64, C.c_int32]
    L.das3r_debug_path_policy_hint.restype = C.c_uint32
    L.das3r_debug_path_policy_hint.argtypes = [ps]
    L.das3r_debug_path_policy_forget.restype = None
    L.das3r_debug_path_policy_forget.argtypes = [ps]
    L.das3r_debug_path_policy_resume.restype = None
    L.das3r_debug_path_policy_resume.argtypes = [ps, C.c_uint32, C.c_uint32]
    L.das3r_debug_seg_dbits.restype = C.c_int
    L.das3r_debug_seg_dbits.argtypes = [C.c_int32, C.c_int32]
    sw = C.POINTER(Switches)   # the switches and the compositing-kernel choice on a caller's own values (additive under ABI 16; host-only)
    L.das3r_debug_parse_switches.restype = None
    L.das3r_debug_parse_switches.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int32, C.c_int32, sw]
    L.das3r_debug_choose_backward.restype = None
    L.das3r_debug_choose_backward.argtypes = [sw, C.c_int64, C.c_int32, C.c_uint32, C.POINTER(BwdChoice)]
    L.das3r_debug_choose_forward.restype = None
    L.das3r_debug_choose_forward.argtypes = [sw, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(FwdChoice)]
    L.das3r_debug_has_invdepth_form.restype = C.c_int
    L.das3r_debug_has_invdepth_form.argtypes = [C.c_int32, C.c_int32]
    L.das3r_debug_kernel_name.restype = C.c_char_p
    L.das3r_debug_kernel_name.argtypes = [C.c_int32, C.c_int32]
    L.das3r_debug_choose_preprocess_backward.restype = C.c_int   # the per-Gaussian backward's form (additive under ABI 16; host-only)
    L.das3r_debug_choose_preprocess_backward.argtypes = [C.POINTER(PreprocessBackwardInputs), C.POINTER(PreprocessForm)]
    L.das3r_debug_preprocess_backward_name.restype = C.c_char_p
    L.das3r_debug_preprocess_backward_name.argtypes = [C.POINTER(PreprocessForm)]
    L.das3r_raster_get_layout.restype = C.c_int
    L.das3r_raster_get_layout.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(RasterLayout)]
    _lib = L
    return L


def reload_switches():
    """Have the library read its DAS3R_* experiment switches from the environment again (it reads them once, at first use)."""
    L = load()
    L.das3r_reload_switches.restype = None
    L.das3r_reload_switches.argtypes = []
    L.das3r_reload_switches()


def split_colour_rule(has_sh, sh_degree, P, binning_path, forced=None, no_backward=False):
    """include/das3r_raster.h das3r_split_colour_rule: does a forward of this shape take the split preprocess?  binning_path: 0 global
    depth sort, 1 local order / segmented, 2 fused emission; forced=None: what DAS3R_SPLIT_COLOUR says (as last read); no_backward: an
    evaluation forward (das3r_raster_saved.flags bit 3 on the way in)."""
    L = load()
    L.das3r_split_colour_rule.restype = C.c_int
    L.das3r_split_colour_rule.argtypes = [C.c_int32] * 6
    L.das3r_split_colour_switch.restype = C.c_int
    L.das3r_split_colour_switch.argtypes = []
    if forced is None:
        forced = L.das3r_split_colour_switch()
    return bool(L.das3r_split_colour_rule(int(bool(has_sh)), int(sh_degree), int(P), int(binning_path), int(bool(no_backward)), int(forced)))


def split_colour_switch():
    """-1 / 0 / 1: DAS3R_SPLIT_COLOUR = "0" / unset / "1", as the library last read it (reload_switches)."""
    L = load()
    L.das3r_split_colour_switch.restype = C.c_int
    L.das3r_split_colour_switch.argtypes = []
    return int(L.das3r_split_colour_switch())


def has_experiments():
    """True when the library was built with `make EXPERIMENTS=1` (superseded kernels behind DAS3R_RENDER_BWD=mfma | stream,
    DAS3R_SORT=classic)."""
    L = load()
    L.das3r_has_experiments.restype = C.c_int
    L.das3r_has_experiments.argtypes = []
    return bool(L.das3r_has_experiments())


def inject_fault(bits):
    """Test aid: OR `bits` into the binning self-check word of every forward from now on; 0 switches it off (include/das3r_raster.h)."""
    L = load()
    L.das3r_debug_inject_fault.restype = None
    L.das3r_debug_inject_fault.argtypes = [C.c_uint32]
    L.das3r_debug_inject_fault(int(bits))


def forget_shapes():
    """The calling thread's library state on the current device forgets what it has learnt about shapes (include/das3r_raster.h
    das3r_raster_forget_shapes): a job that must end bit-identical whatever its thread ran before calls this first."""
    L = load()
    L.das3r_raster_forget_shapes.restype = C.c_int
    L.das3r_raster_forget_shapes.argtypes = []
    check(L.das3r_raster_forget_shapes(), "das3r_raster_forget_shapes")


def learning(state=None):
    """include/das3r_raster.h das3r_raster_learning: state=None reads (forward kernel, forwards so far) of the calling thread's current shape;
    a tuple hands it to the next shape the thread meets (a resumed job)."""
    L = load()
    L.das3r_raster_learning.restype = C.c_int
    L.das3r_raster_learning.argtypes = [C.c_int32, C.POINTER(C.c_uint32)]
    buf = (C.c_uint32 * 2)(*(state if state is not None else (0, 0)))
    check(L.das3r_raster_learning(0 if state is None else 1, buf), "das3r_raster_learning")
    return int(buf[0]), int(buf[1])


def mutate(what):
    """Test aid: 1 = the block-walk backward evaluates exp(power) (1 + 1e-4), 0 = off (include/das3r_raster.h das3r_debug_mutate)."""
    L = load()
    L.das3r_debug_mutate.restype = None
    L.das3r_debug_mutate.argtypes = [C.c_uint32]
    L.das3r_debug_mutate(int(what))


def poison_lds(pattern=0x7FC00000):
    """Test aid: fill the LDS of every CU with `pattern` on torch's current stream (include/das3r_raster.h)."""
    import torch
    L = load()
    L.das3r_debug_poison_lds.restype = C.c_int
    L.das3r_debug_poison_lds.argtypes = [C.c_uint32, C.c_void_p]
    check(L.das3r_debug_poison_lds(int(pattern), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "das3r_debug_poison_lds")


def pair_counters(enable):
    """enable=True: zero the compositing kernels' pair counters and start counting; enable=False: stop and return
    dict(fwd_pairs, bwd_pairs, fwd_wave_iterations, bwd_wave_iterations)."""
    L = load()
    L.das3r_pair_counters.restype = C.c_int
    L.das3r_pair_counters.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
    if enable:
        check(L.das3r_pair_counters(1, None), "das3r_pair_counters")
        return None
    out = (C.c_uint64 * 4)()
    check(L.das3r_pair_counters(0, out), "das3r_pair_counters")
    return dict(fwd_pairs=int(out[0]), bwd_pairs=int(out[1]), fwd_wave_iterations=int(out[2]), bwd_wave_iterations=int(out[3]))


def stats():
    """-> dict(forwards, checks_examined, rescued_polls, failed_checks): the library's process-wide counters."""
    L = load()
    out = (C.c_uint64 * 4)()
    L.das3r_get_stats.restype = None
    L.das3r_get_stats.argtypes = [C.POINTER(C.c_uint64)]
    L.das3r_get_stats(out)
    return dict(forwards=int(out[0]), checks_examined=int(out[1]), rescued_polls=int(out[2]), failed_checks=int(out[3]))


def profile_enable(on):
    L = load()
    L.das3r_profile_enable.restype = None
    L.das3r_profile_enable.argtypes = [C.c_int]
    L.das3r_profile_enable(int(bool(on)))


def profile_report(raw=False):
    """-> {kernel name: (launches, total_ms)}; clears the records.  Template arguments are stripped from names unless `raw` (the
    names are the launch sites' own text, e.g. "render_backward_blk_kernel<MBV, PIX, 0, OCC, true>": the instantiation's LAST flag)."""
    L = load()
    L.das3r_profile_report.restype = C.c_int
    L.das3r_profile_report.argtypes = [C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    check(L.das3r_profile_report(buf, len(buf)), "das3r_profile_report")
    out = {}
    for line in buf.value.decode().splitlines():
        name, n, ms = line.rsplit(" ", 2)
        name = name.strip("() ")
        if not raw:
            name = name.split("<")[0]
        c, t = out.get(name, (0, 0.0))
        out[name] = (c + int(n), t + float(ms))
    return out


def splat_field(geom, L, name, P):
    """[P, 4] float32 view of one field ("xy" / "conic_opacity" / "rgbd") of the per-Gaussian 64-byte records in `geom`."""
    import torch
    nbytes = (P - 1) * L["splat_stride"] + 16 if P > 0 else 0
    fl = geom[L[name]:L[name] + nbytes].view(torch.float32)
    return torch.as_strided(fl, (P, 4), (L["splat_stride"] // 4, 1))


def last_error():
    return load().das3r_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc < 0:
        raise RuntimeError(f"{what} failed (status {rc}): {last_error()}")
    return rc


def layout(P, capacity, W, H):
    out = RasterLayout()
    check(load().das3r_raster_get_layout(int(P), int(capacity), int(W), int(H), C.byref(out)), "das3r_raster_get_layout")
    return {n: getattr(out, n) for n, _ in RasterLayout._fields_}
