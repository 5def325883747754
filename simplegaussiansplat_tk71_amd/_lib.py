"""ctypes binding of libgrouped_cumprod_hip.so (the C ABI of include/grouped_cumprod_hip.h).

There is NO fallback: if the library is missing or does not load, importing the
ops raises.  The reference has the same property — `import grouped_cumprod`
fails when its extension is not built (reference: gs_model.py:8).
"""
import ctypes
import os

from . import _build
from ._build import LIB_PATH

_c_void_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_sz = ctypes.c_size_t
_i32 = ctypes.c_int32

# name -> (restype, argtypes); must list every symbol include/grouped_cumprod_hip.h declares
SIGNATURES = {
    "gcp_abi_version": (ctypes.c_int, []),
    "gcp_source_hash": (ctypes.c_char_p, []),
    "gcp_last_hip_error": (ctypes.c_int, []),
    "gcp_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "gcp_workspace_bytes": (_sz, [_i64]),
    "gcp_workspace_init": (ctypes.c_int, [_c_void_p, _sz, _c_void_p]),
    "gcp_cumprod_forward": (ctypes.c_int, [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _sz, _c_void_p]),
    "gcp_cumsum_forward": (ctypes.c_int, [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _sz, _c_void_p]),
    "gcp_cumsum_reverse": (ctypes.c_int, [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _sz, _c_void_p]),
    "gcp_cumprod_forward_indexed": (ctypes.c_int, [_c_void_p] * 4 + [_i64, _c_void_p, _sz, _c_void_p]),
    "gcp_cumsum_forward_indexed": (ctypes.c_int, [_c_void_p] * 4 + [_i64, _c_void_p, _sz, _c_void_p]),
    "gcp_cumsum_reverse_indexed": (ctypes.c_int, [_c_void_p] * 4 + [_i64, _c_void_p, _sz, _c_void_p]),
    "gcp_cumprod_forward_carry": (ctypes.c_int, [_c_void_p] * 4 + [_i64, _i64, _c_void_p, _sz, _c_void_p]),
    "gcp_cumsum_forward_carry": (ctypes.c_int, [_c_void_p] * 4 + [_i64, _i64, _c_void_p, _sz, _c_void_p]),
    "gcp_cumsum_reverse_carry": (ctypes.c_int, [_c_void_p] * 4 + [_i64, _i64, _c_void_p, _sz, _c_void_p]),
    "gcp_cumprod_backward": (
        ctypes.c_int,
        [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _c_void_p, _sz, _c_void_p],
    ),
    "gcp_cumprod_backward_given": (
        ctypes.c_int,
        [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _c_void_p, _sz, _c_void_p],
    ),
    "gcp_check_groups": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i64, ctypes.POINTER(_i64), _c_void_p]),
    "gcp_check_permutation": (ctypes.c_int, [_c_void_p, _i64, ctypes.POINTER(_i64), _c_void_p]),
    "gcp_check_group_ids": (ctypes.c_int, [_c_void_p, _i64, _i64, ctypes.POINTER(_i64), _c_void_p]),
    "gcp_set_validate_operands": (ctypes.c_int, [ctypes.c_int]),
    "gcp_tile_elems": (ctypes.c_int, []),
    "gcp_last_fallback_tiles": (ctypes.c_int, [_c_void_p, _c_void_p, ctypes.POINTER(_i64)]),
    "gcp_last_lookback_tiles": (ctypes.c_int, [_c_void_p, _c_void_p, ctypes.POINTER(_i64)]),
    "gcp_set_lookback_wait_us": (ctypes.c_int, [_i64]),
    # rows f1 / f2 (gcp_bin.hip, gcp_blend.hip) and what serves rows a5 / a6 around them (gcp_sort.hip, gcp_compact.hip, gcp_walk.hip)
    "gcp_tile_grid": (ctypes.c_int, [_i32, _i32, ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "gcp_scan_i32_workspace_bytes": (_sz, [_i64]),
    "gcp_exclusive_scan_i32": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _c_void_p, _sz, _c_void_p]),
    "gcp_bin_tiles_count": (
        ctypes.c_int,
        [_c_void_p, _c_void_p, _i64, _i32, _i32, _c_void_p, ctypes.POINTER(_i64), _c_void_p, _sz, _c_void_p],
    ),
    "gcp_bin_workspace_bytes": (_sz, [_i64, _i64]),
    "gcp_bin_tiles_fill": (
        ctypes.c_int,
        [_c_void_p, _c_void_p, _i64, _i32, _i32, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p],
    ),
    "gcp_bin_tiles": (
        ctypes.c_int,
        [_c_void_p, _c_void_p, _i64, _i32, _i32, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p],
    ),
    "gcp_blend_checkpoint_floats": (_sz, [_i64, _i32, _i32]),
    "gcp_blend_forward": (
        ctypes.c_int,
        [_c_void_p] * 6 + [_i64, _i32, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p],
    ),
    "gcp_blend_backward_workspace_bytes": (_sz, [_i64]),
    "gcp_blend_backward": (
        ctypes.c_int,
        [_c_void_p] * 6 + [_i64, _i32, _i32, _c_void_p, _i64] + [_c_void_p] * 8 + [_c_void_p, _sz, _c_void_p],
    ),
    "gcp_blend_forward_depth": (ctypes.c_int, [_c_void_p] * 8 + [_i64, _i32, _i32] + [_c_void_p] * 7),
    "gcp_blend_backward_depth_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "gcp_blend_backward_depth": (ctypes.c_int, [_c_void_p] * 8 + [_i64, _i32, _i32, _c_void_p, _i64] + [_c_void_p] * 13 + [_sz, _c_void_p]),
    "gcp_gather_f32": (ctypes.c_int, [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p]),
    "gcp_unsort_finish": (ctypes.c_int, [_c_void_p] * 5 + [_i64, _i32, _c_void_p]),
    "gcp_sort_workspace_bytes": (_sz, [_i64]),
    "gcp_sort_pairs_u32": (ctypes.c_int, [_c_void_p, _i64, _i32, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_sort_rects": (ctypes.c_int, [_c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_rects_key_range": (ctypes.c_int, [_c_void_p, _i64, _c_void_p, _c_void_p]),
    "gcp_compact_workspace_bytes": (_sz, [_i64]),
    "gcp_compact_finish": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i64, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_pairs_finish_prepare": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _c_void_p]),
    "gcp_pairs_finish_boxes": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i32, _i32] + [_c_void_p] * 6 + [_i64, _i32, _c_void_p, _i32, _c_void_p]),
    "gcp_compact_kept_workspace_bytes": (_sz, [_i64]),
    "gcp_compact_kept_count": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i64, _i64, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_compact_kept_write": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i64, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_rects_cut_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i64]),
    "gcp_rects_cut": (ctypes.c_int, [_c_void_p, _i32, _i64, _i64, _i64, _i32, _i64] + [_c_void_p] * 6 + [_sz, _c_void_p]),
    "gcp_pixels_range": (ctypes.c_int, [_c_void_p, _i32, _i64, _c_void_p, _c_void_p]),
    "gcp_pixels_min_workspace_bytes": (_sz, [_i32, _i32]),
    "gcp_pixels_min": (ctypes.c_int, [_c_void_p, _i32, _c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_rects_rows_workspace_bytes": (_sz, [_i64]),
    "gcp_rects_rows_capacity": (_i64, [_i64]),
    "gcp_rects_rows": (ctypes.c_int, [_c_void_p, _i64, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_rects_rows_i64": (ctypes.c_int, [_c_void_p, _i64, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_rows_rectangles_workspace_bytes": (_sz, [_i64]),
    "gcp_rows_rectangles": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_rectangle_boxes": (ctypes.c_int, [_c_void_p, _c_void_p, _c_void_p, _i64, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "gcp_pairs_scan_boxes": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i32, _i32] + [_c_void_p] * 5 + [_i64, _i32, _c_void_p, _c_void_p]),
    "gcp_box_sizes": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p]),
    "gcp_expand_rects": (ctypes.c_int, [_c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _c_void_p, _c_void_p, _c_void_p]),
    "gcp_pixel_lists_count": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i32, _i32] + [_c_void_p] * 5),
    "gcp_pixel_lists_fill": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i32, _i32] + [_c_void_p] * 8),
    "gcp_project_forward": (ctypes.c_int, [_c_void_p] * 7 + [_i64, _i32, _i32, _i32, _i32, ctypes.c_float] + [_c_void_p] * 5),
    "gcp_project_gather": (ctypes.c_int, [_c_void_p, _c_void_p, _i64] + [_c_void_p] * 11),
    "gcp_adam_step": (ctypes.c_int, [_c_void_p] * 4 + [_i64] + [ctypes.c_double] * 4 + [_i64, _c_void_p]),
    # n_tensors, host arrays (param, grad, exp_avg, exp_avg_sq, rows, width, step), device lr, scal, visible, betas, eps, stream
    "gcp_adam_step_multi": (ctypes.c_int, [_i32] + [_c_void_p] * 10 + [ctypes.c_double] * 3 + [_c_void_p]),
    "gcp_ssim_blocks": (_i64, [_i64, _i32, _i32]),
    "gcp_ssim_l1_forward": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i32, _i32, _c_void_p, ctypes.c_float, ctypes.c_float]
                            + [_c_void_p] * 5),
    "gcp_ssim_l1_backward": (ctypes.c_int, [_c_void_p] * 5 + [_i64, _i32, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    # img, ref, images, channels, height, width, host window, c1, c2, GCP_METRICS_* flags, partial, out (double), stream
    "gcp_image_metrics": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _c_void_p, ctypes.c_float, ctypes.c_float, _i32]
                          + [_c_void_p] * 3),
    # per-camera exposure (device float[images][3][4] after img, ref; three channels implied): the loss forward and backward
    # (..., scales, grad_img or NULL, partial_e, grad_exposure or NULL, stream) and the metrics on the compensated render
    "gcp_exposure_blocks": (_i64, [_i64, _i32, _i32]),
    "gcp_ssim_l1_forward_exposure": (ctypes.c_int, [_c_void_p] * 3 + [_i64, _i32, _i32, _c_void_p, ctypes.c_float, ctypes.c_float]
                                     + [_c_void_p] * 5),
    "gcp_ssim_l1_backward_exposure": (ctypes.c_int, [_c_void_p] * 6 + [_i64, _i32, _i32] + [_c_void_p] * 6),
    "gcp_image_metrics_exposure": (ctypes.c_int, [_c_void_p] * 3 + [_i64, _i32, _i32, _c_void_p, ctypes.c_float, ctypes.c_float, _i32]
                                   + [_c_void_p] * 3),
    "gcp_project_backward": (ctypes.c_int, [_c_void_p] * 7 + [_i64, _i32, _i32] + [_c_void_p] * 10),
    "gcp_project_gather_depth": (ctypes.c_int, [_c_void_p, _c_void_p, _i64] + [_c_void_p] * 12),
    "gcp_project_backward_depth": (ctypes.c_int, [_c_void_p] * 7 + [_i64, _i32, _i32] + [_c_void_p] * 11),
    # the same with the SH direction's frame chosen (0 camera, 1 world); the backward's grad_depth may be NULL
    "gcp_project_forward_sh": (ctypes.c_int, [_c_void_p] * 7 + [_i64, _i32, _i32, _i32, _i32, _i32, ctypes.c_float] + [_c_void_p] * 5),
    "gcp_project_backward_sh": (ctypes.c_int, [_c_void_p] * 7 + [_i64, _i32, _i32, _i32] + [_c_void_p] * 11),
    # float centres, covariance dilation, colour clamp (gcp_splat.hip): cov_eps, mean_offset, clamp_colour after box_clamp;
    # the gather's depth and keep may be NULL; the backward takes cov_eps, clamp_colour and grad_mean_xy (may be NULL) before the outputs
    "gcp_splat_forward": (ctypes.c_int, [_c_void_p] * 7 + [_i64, _i32, _i32, _i32, _i32, _i32] + [ctypes.c_float] * 3 + [_i32] + [_c_void_p] * 5),
    "gcp_splat_gather": (ctypes.c_int, [_c_void_p, _c_void_p, _i64] + [_c_void_p] * 12),
    "gcp_splat_backward": (ctypes.c_int, [_c_void_p] * 7 + [_i64, _i32, _i32, _i32] + [_c_void_p] * 5 + [ctypes.c_float, _i32] + [_c_void_p] * 7),
    # the same two with a set of GCP_SPLAT_* flags (SPLAT_CLAMP_COLOUR, SPLAT_ANTIALIAS below) where clamp_colour stands
    "gcp_splat_forward_flags": (ctypes.c_int, [_c_void_p] * 7 + [_i64, _i32, _i32, _i32, _i32, _i32] + [ctypes.c_float] * 3 + [_i32] + [_c_void_p] * 5),
    "gcp_splat_backward_flags": (ctypes.c_int, [_c_void_p] * 7 + [_i64, _i32, _i32, _i32] + [_c_void_p] * 5 + [ctypes.c_float, _i32] + [_c_void_p] * 7),
    # density control on the device (gcp_densify.hip): statistic, plan (count, action, offset), row list, row gather, split samples
    "gcp_densify_accumulate": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, ctypes.c_float, ctypes.c_float, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p]),
    "gcp_densify_plan_workspace_bytes": (_sz, [_i64]),
    "gcp_densify_plan": (ctypes.c_int, [_c_void_p] * 4 + [_i64] + [ctypes.c_float] * 4 + [_i32] + [_c_void_p] * 4 + [_sz, _c_void_p]),
    "gcp_densify_fill": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i64, _c_void_p, _c_void_p, _c_void_p]),
    "gcp_densify_rows": (ctypes.c_int, [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p]),
    "gcp_densify_split": (ctypes.c_int, [_c_void_p] * 6 + [_i64, _i64, _i32, ctypes.c_uint32, ctypes.c_uint32] + [_c_void_p] * 3),
    # MCMC density control (gcp_mcmc.hip): weights and their prefix sum, draw (src_row, times, kind), relocated values, position noise
    "gcp_mcmc_workspace_bytes": (_sz, [_i64]),
    "gcp_mcmc_weights": (ctypes.c_int, [_c_void_p, _i64, ctypes.c_float, _i32, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_mcmc_draw": (ctypes.c_int, [_c_void_p, _i64, _i64, ctypes.c_uint32, ctypes.c_uint32] + [_c_void_p] * 4),
    "gcp_mcmc_values": (ctypes.c_int, [_c_void_p] * 4 + [_i64, _i64, ctypes.c_float] + [_c_void_p] * 3),
    "gcp_mcmc_noise": (ctypes.c_int, [_c_void_p] * 4 + [_i64] + [ctypes.c_float] * 3 + [ctypes.c_uint32, ctypes.c_uint32, _c_void_p]),
    # per-Gaussian contribution from the blend (gcp_contrib.hip): max and sum of the colour weight over each Gaussian's box
    "gcp_blend_contrib_workspace_bytes": (_sz, [_i64]),
    "gcp_blend_contrib": (ctypes.c_int, [_c_void_p] * 5 + [_i64, _i32, _i32, _c_void_p, _i64] + [_c_void_p] * 5 + [_sz, _c_void_p]),
    # absolute screen-space gradient (gcp_absgrad.hip): the backward's inputs, then absgrad [N,2], ws, ws_bytes, stream
    "gcp_blend_absgrad_workspace_bytes": (_sz, [_i64]),
    "gcp_blend_absgrad": (ctypes.c_int, [_c_void_p] * 6 + [_i64, _i32, _i32, _c_void_p, _i64] + [_c_void_p] * 6 + [_sz, _c_void_p]),
    "gcp_blend_absgrad_depth": (ctypes.c_int, [_c_void_p] * 8 + [_i64, _i32, _i32, _c_void_p, _i64] + [_c_void_p] * 8 + [_sz, _c_void_p]),
    # depth distortion (gcp_distort.hip): forward -> dist, A_n, sum w (z_L - z) maps; backward: those, t_ckpt and grad_dist -> four gradients
    "gcp_blend_distort_forward": (ctypes.c_int, [_c_void_p] * 6 + [_i64, _i32, _i32] + [_c_void_p] * 6),
    "gcp_blend_distort_backward_workspace_bytes": (_sz, [_i64]),
    "gcp_blend_distort_backward": (ctypes.c_int, [_c_void_p] * 6 + [_i64, _i32, _i32, _c_void_p, _i64] + [_c_void_p] * 11 + [_sz, _c_void_p]),
    # median depth (gcp_median.hip): forward -> median f32 and index i32 maps; backward: boxes, bins, index and grad_median -> grad_depth
    "gcp_blend_median_forward": (ctypes.c_int, [_c_void_p] * 6 + [_i64, _i32, _i32] + [_c_void_p] * 5),
    "gcp_blend_median_backward_workspace_bytes": (_sz, [_i64]),
    "gcp_blend_median_backward": (ctypes.c_int, [_c_void_p] * 2 + [_i64, _i32, _i32, _c_void_p, _i64] + [_c_void_p] * 5 + [_sz, _c_void_p]),
    # the 3-D smoothing filter (gcp_filter3d.hip): rate (mean, P, K, wh, n, cameras, near, margin -> rate); apply (log scale, opacity,
    # filter, n -> the filtered two); its backward (the three inputs, the two upstream gradients, n -> the two gradients); stream last
    "gcp_filter3d_rate": (ctypes.c_int, [_c_void_p] * 4 + [_i64, _i64, ctypes.c_float, ctypes.c_float, _c_void_p, _c_void_p]),
    "gcp_filter3d_apply": (ctypes.c_int, [_c_void_p] * 3 + [_i64] + [_c_void_p] * 3),
    "gcp_filter3d_apply_backward": (ctypes.c_int, [_c_void_p] * 5 + [_i64] + [_c_void_p] * 3),
    # lens distortion (gcp_undistort.hip): src (u8 [n,H,W,3] / f32 [n,3,H,W]), lenses f32[n][LENS_WORDS], images, height, width,
    # dst f32[n,3,H,W], stream
    "gcp_undistort_u8": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p]),
    "gcp_undistort_f32": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p]),
    # normals (gcp_normal.hip): per-Gaussian normals (q, log scale, mean, P, index, n, m -> normal, aux; its backward: q, P, index,
    # aux, g_normal, n, m -> g_q) and the depth-normal consistency loss (depth, alpha, normal, K, images, height, width, alpha_min
    # -> e_map or NULL, depth_normal or NULL, partial; its backward: ... alpha_min, scale -> g_depth, g_alpha, g_normal); stream last
    "gcp_normals_forward": (ctypes.c_int, [_c_void_p] * 5 + [_i64, _i64] + [_c_void_p] * 3),
    "gcp_normals_backward": (ctypes.c_int, [_c_void_p] * 5 + [_i64, _i64] + [_c_void_p] * 2),
    "gcp_normal_consistency_blocks": (_i64, [_i64, _i32, _i32]),
    "gcp_normal_consistency_forward": (ctypes.c_int, [_c_void_p] * 4 + [_i64, _i32, _i32, ctypes.c_float] + [_c_void_p] * 4),
    "gcp_normal_consistency_backward": (ctypes.c_int, [_c_void_p] * 4 + [_i64, _i32, _i32, ctypes.c_float] + [_c_void_p] * 5),
    # mesh extraction (gcp_tsdf.hip): TSDF integration (tsdf, weight, rgb or NULL, nx, ny, nz, origin x y z, voxel, trunc, depth,
    # alpha, image or NULL, P, K, cameras, height, width, alpha_min, depth_max, stream) and marching tetrahedra: count (tsdf,
    # weight or NULL, nx, ny, nz, iso, ws, ws_bytes -> host int64[2] vertices, faces) and write (tsdf, rgb or NULL, nx, ny, nz,
    # origin x y z, voxel, iso, ws, ws_bytes, vertices, faces -> vertices, faces, colours or NULL); stream last
    "gcp_tsdf_integrate": (ctypes.c_int, [_c_void_p] * 3 + [_i32] * 3 + [ctypes.c_float] * 5 + [_c_void_p] * 5 + [_i64, _i32, _i32]
                           + [ctypes.c_float] * 2 + [_c_void_p]),
    "gcp_mesh_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "gcp_mesh_count": (ctypes.c_int, [_c_void_p, _c_void_p, _i32, _i32, _i32, ctypes.c_float, _c_void_p, _sz, ctypes.POINTER(_i64), _c_void_p]),
    "gcp_mesh_write": (ctypes.c_int, [_c_void_p, _c_void_p, _i32, _i32, _i32] + [ctypes.c_float] * 5 + [_c_void_p, _sz, _i64, _i64]
                       + [_c_void_p] * 4),
    # mesh cleaning and vertex normals (gcp_meshclean.hip): components (faces, F, V -> label, size, status or NULL; ws, ws_bytes),
    # select (faces, F, V, keep_largest, min_faces, ws, ws_bytes -> host int64[2] V', F'), compact (faces, F, V, vertices, colours or
    # NULL, normals or NULL, ws, ws_bytes, V', F' -> vertices, faces, colours or NULL, normals or NULL), normals (vertices, faces, V, F
    # -> normals; ws, ws_bytes); stream last
    "gcp_mesh_components_workspace_bytes": (_sz, [_i64, _i64]),
    "gcp_mesh_components": (ctypes.c_int, [_c_void_p, _i64, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p]),
    "gcp_mesh_clean_workspace_bytes": (_sz, [_i64, _i64]),
    "gcp_mesh_select": (ctypes.c_int, [_c_void_p, _i64, _i64, _i64, _i64, _c_void_p, _sz, ctypes.POINTER(_i64), _c_void_p]),
    "gcp_mesh_compact": (ctypes.c_int, [_c_void_p, _i64, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _sz, _i64, _i64] + [_c_void_p] * 5),
    "gcp_mesh_vertex_normals_workspace_bytes": (_sz, [_i64, _i64]),
    "gcp_mesh_vertex_normals": (ctypes.c_int, [_c_void_p, _c_void_p, _i64, _i64, _c_void_p, _c_void_p, _sz, _c_void_p]),
    # exact k nearest neighbours inside one cloud (gcp_knn.hip): xyz, n, k -> index i32[n,k], dist2 f32[n,k]; ws, ws_bytes, stream
    "gcp_knn_workspace_bytes": (_sz, [_i64]),
    "gcp_knn": (ctypes.c_int, [_c_void_p, _i64, _i32, _c_void_p, _c_void_p, _c_void_p, _sz, _c_void_p]),
}

ABI_VERSION = 4
SPLAT_CLAMP_COLOUR, SPLAT_ANTIALIAS = 1, 2  # GCP_SPLAT_* of the header
METRICS_CLAMP = 1  # GCP_METRICS_CLAMP
LENS_WORDS, LENS_KINDS = 20, ("pinhole", "polynomial", "fisheye")  # GCP_LENS_WORDS; GCP_LENS_* = the index of the kind

_lib = None


def load():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("GCP_LIBRARY", LIB_PATH)
    if path == LIB_PATH and os.path.exists(path) and _build.is_stale():
        # a binary older than the sources of this checkout: rebuild where hipcc exists, refuse otherwise
        try:
            _build.build_hip_library(force=True)
        except RuntimeError as e:
            raise ImportError(f"{path} was built from other sources than this checkout's and cannot be rebuilt: {e}") from e
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python setup.py build_ext --inplace` "
            "(or __graft_entry__.build()). There is no CPU fallback."
        )
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    got = lib.gcp_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"{path}: ABI version {got}, binding expects {ABI_VERSION}")
    _lib = lib
    return lib


def check(status, what):
    """Turn a GCP_* status into the RuntimeError the reference's callers would see."""
    if status == 0:
        return
    lib = load()
    msg = lib.gcp_status_string(status).decode()
    if status == 3:
        msg += f" (hipError {lib.gcp_last_hip_error()})"
    raise RuntimeError(f"{what}: {msg}")
