"""ctypes binding of include/sbbseg.h -- the thin layer between the Python host and the HIP library.

There is deliberately no fallback: if libsbbseg.so is missing or a call fails, a RuntimeError is
raised (the reference's callers expect ordinary Python exceptions, main.py:2061-2157)."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsbbseg.so")

PREC_BF16, PREC_F32, PREC_F16, PREC_F16X3 = 0, 1, 2, 3
PRECISIONS = {"bf16": PREC_BF16, "f32": PREC_F32, "f16": PREC_F16, "f16x3": PREC_F16X3}
INPUT_C8, INPUT_PAIRS = 0, 1

EXPORTS = [
    "sbbseg_last_error", "sbbseg_abi_version", "sbbseg_device_count", "sbbseg_create", "sbbseg_destroy",
    "sbbseg_model_load", "sbbseg_model_load_file", "sbbseg_debug_plan_summary",
    "sbbseg_set_stream", "sbbseg_set_lanes", "sbbseg_set_label_channels", "sbbseg_set_dedupe", "sbbseg_set_ksplit", "sbbseg_synchronize", "sbbseg_set_input", "sbbseg_input_form", "sbbseg_add_tensor",
    "sbbseg_add_conv", "sbbseg_add_maxpool", "sbbseg_add_tail", "sbbseg_add_head", "sbbseg_finalize", "sbbseg_model_info",
    "sbbseg_num_ops", "sbbseg_op_info", "sbbseg_op_issued_flops", "sbbseg_device_bytes", "sbbseg_predict", "sbbseg_segment_page",
    "sbbseg_segment_page_dev", "sbbseg_segment_pages_dev", "sbbseg_segment_page_scaled", "sbbseg_segment_page_otsu", "sbbseg_segment_crop", "sbbseg_segment_crop_dev", "sbbseg_debug_largest_contour", "sbbseg_debug_counter", "sbbseg_comm_unique_id", "sbbseg_comm_init", "sbbseg_comm_info", "sbbseg_comm_destroy", "sbbseg_allgather_labels_dev", "sbbseg_otsu_dev",
    "sbbseg_segment_tile_range_bin_dev", "sbbseg_segment_whole", "sbbseg_segment_whole_scaled", "sbbseg_tile_grid", "sbbseg_nearest_map", "sbbseg_segment_tiles_dev",
    "sbbseg_segment_tile_range_dev", "sbbseg_stitch_dev", "sbbseg_debug_ingest", "sbbseg_debug_read_tensor",
    "sbbseg_debug_set_conv_variant", "sbbseg_debug_inject_alloc_failure",
    "sbbseg_morph_dev", "sbbseg_morph", "sbbseg_page_box_dev", "sbbseg_extract_page_box", "sbbseg_extract_page_box_dev",
    "sbbseg_deskew_side", "sbbseg_rotation_matrix", "sbbseg_deskew_profiles_dev", "sbbseg_deskew_profiles",
    "sbbseg_segment_pages",
    "sbbseg_profile_enable", "sbbseg_profile_reset", "sbbseg_profile_get",
    "sbbseg_debug_largest_contour_area2", "sbbseg_text_regions_present_dev", "sbbseg_run_page", "sbbseg_device_alloc", "sbbseg_device_free", "sbbseg_upload", "sbbseg_download", "sbbseg_download_labels",
    "sbbseg_set_owned_regions", "sbbseg_owned_region_info", "sbbseg_op_executed", "sbbseg_debug_owned_range", "sbbseg_debug_region_rows",
    "sbbseg_debug_poison_activations",
    "sbbseg_text_region_boxes_dev", "sbbseg_text_region_boxes", "sbbseg_region_deskew_profiles_dev", "sbbseg_region_deskew_profiles",
    "sbbseg_profile_statistics_host", "sbbseg_profile_statistics_dev", "sbbseg_deskew_sweep_angles", "sbbseg_region_deskew_slopes_dev", "sbbseg_region_deskew_slopes",
    "sbbseg_region_line_masks_dev", "sbbseg_region_line_masks", "sbbseg_region_line_masks_host", "sbbseg_region_line_table",
    "sbbseg_line_split_host", "sbbseg_line_split_dev", "sbbseg_region_line_boxes_dev", "sbbseg_region_line_boxes",
    "sbbseg_segment_views_dev", "sbbseg_segment_views", "sbbseg_debug_axis_owner",
    "sbbseg_debug_op_launch", "sbbseg_debug_tensor_period_mismatches",
    "sbbseg_segment_whole_views_dev", "sbbseg_extract_page_boxes_dev", "sbbseg_run_pages",
    "sbbseg_run_pages_planes", "sbbseg_planes_deskew_slopes_dev", "sbbseg_planes_line_masks_dev", "sbbseg_planes_line_boxes_dev",
    "sbbseg_text_region_contours_dev", "sbbseg_text_region_contours", "sbbseg_text_region_contours_read", "sbbseg_mask_contours_host",
    "sbbseg_debug_mask_contours_dev", "sbbseg_debug_set_contour_lds_limit", "sbbseg_debug_contour_launches", "sbbseg_debug_set_contour_host_step_bound",
    "sbbseg_debug_profile_statistics", "sbbseg_debug_soft_arith",
    "sbbseg_contour_moments_dev", "sbbseg_contour_moments_host", "sbbseg_region_order_dev", "sbbseg_region_order", "sbbseg_region_order_host",
    "sbbseg_debug_row_sums", "sbbseg_debug_order_launches",
    "sbbseg_region_line_extents_dev", "sbbseg_region_line_extents_read", "sbbseg_region_line_extents_host", "sbbseg_region_line_extent_weights",
    "sbbseg_debug_mask_border_winner_dev", "sbbseg_debug_mask_border_winner_host", "sbbseg_debug_set_extent_lds_limit", "sbbseg_debug_extent_launches",
]


class ConvSrc(C.Structure):
    _fields_ = [("tensor", C.c_int32), ("channels", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
                ("stride_y", C.c_int32), ("stride_x", C.c_int32), ("pad_top", C.c_int32), ("pad_left", C.c_int32),
                ("up_shift", C.c_int32), ("off_y", C.c_int32), ("off_x", C.c_int32)]


class RunInfo(C.Structure):
    """sbbseg_run_info (include/sbbseg.h)"""
    _fields_ = [("box_xywh", C.c_int32 * 4), ("box_pixels", C.c_int64), ("otsu_threshold", C.c_int32), ("regions_ok", C.c_int32),
                ("text_present", C.c_int32), ("textlines_ok", C.c_int32)]


class View(C.Structure):
    """sbbseg_view (include/sbbseg.h)"""
    _fields_ = [("page", C.c_void_p), ("Hs", C.c_int32), ("Ws", C.c_int32), ("Hp", C.c_int32), ("Wp", C.c_int32), ("cx", C.c_int32),
                ("cy", C.c_int32), ("cw", C.c_int32), ("ch", C.c_int32), ("binarise", C.c_int32), ("labels", C.c_void_p),
                ("threshold", C.c_void_p)]


class WholeView(C.Structure):
    """sbbseg_whole_view (include/sbbseg.h)"""
    _fields_ = [("page", C.c_void_p), ("stored_h", C.c_int32), ("stored_w", C.c_int32), ("page_h", C.c_int32), ("page_w", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("labels", C.c_void_p)]


class RunPageIO(C.Structure):
    """sbbseg_run_page_io (include/sbbseg.h)"""
    _fields_ = [("page", C.c_void_p), ("Hp", C.c_int32), ("Wp", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32),
                ("page_mask_out", C.c_void_p), ("regions_out", C.c_void_p), ("textlines_out", C.c_void_p), ("info", RunInfo),
                ("status", C.c_int32)]


class Plane(C.Structure):
    """sbbseg_plane (include/sbbseg.h)"""
    _fields_ = [("d_hw", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32)]


class ConvDesc(C.Structure):
    _fields_ = [("n_src", C.c_int32), ("src", ConvSrc * 2), ("cout", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("out_stride_y", C.c_int32), ("out_stride_x", C.c_int32), ("out_off_y", C.c_int32), ("out_off_x", C.c_int32),
                ("out_tensor", C.c_int32), ("relu", C.c_int32), ("residual_tensor", C.c_int32),
                ("raw_out_tensor", C.c_int32), ("head_classes", C.c_int32), ("algorithmic_macs", C.c_double)]


_lib = None


def load_library(path: Optional[str] = None):
    """Load libsbbseg.so (no GPU needed for loading).  Raises if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not found: build it with `python -m sbb_textline_detection_amd._build` "
                           "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(p)
    lib.sbbseg_last_error.restype = C.c_char_p
    vp, i32, f32p = C.c_void_p, C.c_int, C.POINTER(C.c_float)
    sigs = {
        "sbbseg_abi_version": [],
        "sbbseg_device_count": [C.POINTER(C.c_int)],
        "sbbseg_create": [i32, i32, C.POINTER(vp)],
        "sbbseg_destroy": [vp],
        "sbbseg_model_load": [vp, C.c_size_t, i32, i32, i32, i32, C.POINTER(vp)],
        "sbbseg_model_load_file": [C.c_char_p, i32, i32, i32, i32, C.POINTER(vp)],
        "sbbseg_debug_plan_summary": [vp, C.c_size_t, i32, i32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)],
        "sbbseg_set_stream": [vp, vp],
        "sbbseg_synchronize": [vp],
        "sbbseg_set_lanes": [vp, i32],
        "sbbseg_set_label_channels": [vp, i32],
        "sbbseg_set_dedupe": [vp, i32],
        "sbbseg_set_ksplit": [vp, i32],
        "sbbseg_set_input": [vp, i32, i32, i32],
        "sbbseg_input_form": [vp, i32, i32, C.POINTER(C.c_int)],
        "sbbseg_add_tensor": [vp, i32, i32, i32, C.POINTER(C.c_int)],
        "sbbseg_add_conv": [vp, C.POINTER(ConvDesc)] + [vp] * 9,
        "sbbseg_add_maxpool": [vp, i32, i32, i32, i32, vp, vp, i32],
        "sbbseg_add_head": [vp, i32, i32, i32, vp, vp, vp],
        "sbbseg_add_tail": [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, C.c_double],
        "sbbseg_finalize": [vp, i32],
        "sbbseg_model_info": [vp] + [C.POINTER(C.c_int)] * 4,
        "sbbseg_num_ops": [vp, C.POINTER(C.c_int)],
        "sbbseg_op_info": [vp, i32, C.c_char_p, i32, C.POINTER(C.c_double), C.POINTER(C.c_double)],
        "sbbseg_op_issued_flops": [vp, i32, C.POINTER(C.c_double)],
        "sbbseg_device_bytes": [vp, C.POINTER(C.c_size_t)],
        "sbbseg_predict": [vp, vp, i32, vp],
        "sbbseg_segment_page": [vp, vp, i32, i32, vp],
        "sbbseg_segment_page_dev": [vp, vp, i32, i32, vp],
        "sbbseg_segment_pages_dev": [vp, i32, vp, i32, i32, vp],
        "sbbseg_segment_page_scaled": [vp, vp, i32, i32, i32, i32, vp],
        "sbbseg_segment_page_otsu": [vp, vp, i32, i32, i32, i32, vp, C.POINTER(C.c_int)],
        "sbbseg_debug_largest_contour": [vp, i32, i32, vp, C.POINTER(C.c_int64)],
        "sbbseg_debug_counter": [vp, i32, C.POINTER(C.c_int64)],
        "sbbseg_comm_unique_id": [C.c_char_p],
        "sbbseg_comm_init": [vp, i32, i32, C.c_char_p],
        "sbbseg_comm_info": [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "sbbseg_comm_destroy": [vp],
        "sbbseg_allgather_labels_dev": [vp, vp, C.c_size_t, vp],
        "sbbseg_segment_crop": [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, C.POINTER(C.c_int)],
        "sbbseg_segment_crop_dev": [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp],
        "sbbseg_segment_views_dev": [vp, i32, C.POINTER(View)],
        "sbbseg_segment_views": [vp, i32, C.POINTER(View), vp],
        "sbbseg_debug_axis_owner": [i32, i32, i32, i32, vp],
        "sbbseg_segment_whole_views_dev": [vp, i32, C.POINTER(WholeView)],
        "sbbseg_extract_page_boxes_dev": [vp, i32, C.POINTER(WholeView), vp, vp],
        "sbbseg_run_pages": [vp, vp, vp, i32, C.POINTER(RunPageIO), i32],
        "sbbseg_otsu_dev": [vp, vp, i32, i32, vp],
        "sbbseg_segment_tile_range_bin_dev": [vp, vp, i32, i32, i32, i32, vp, vp],
        "sbbseg_segment_whole": [vp, vp, i32, i32, i32, i32, vp],
        "sbbseg_segment_whole_scaled": [vp, vp, i32, i32, i32, i32, i32, i32, vp],
        "sbbseg_tile_grid": [i32, i32, i32, i32, vp, i32, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "sbbseg_nearest_map": [i32, i32, vp],
        "sbbseg_segment_tiles_dev": [vp, vp, i32, i32, vp, i32, vp],
        "sbbseg_segment_tile_range_dev": [vp, vp, i32, i32, i32, i32, vp],
        "sbbseg_stitch_dev": [vp, vp, i32, i32, vp],
        "sbbseg_debug_ingest": [vp, vp, i32, i32, vp, i32, i32, vp, C.c_size_t],
        "sbbseg_debug_read_tensor": [vp, i32, i32, vp, C.c_size_t],
        "sbbseg_debug_set_conv_variant": [vp, i32],
        "sbbseg_morph_dev": [vp, vp, i32, i32, i32, i32, i32, vp],
        "sbbseg_morph": [vp, vp, i32, i32, i32, i32, i32, vp],
        "sbbseg_page_box_dev": [vp, vp, i32, i32, vp, C.POINTER(C.c_int64)],
        "sbbseg_extract_page_box": [vp, vp, i32, i32, i32, i32, vp, vp, C.POINTER(C.c_int64)],
        "sbbseg_extract_page_box_dev": [vp, vp, i32, i32, i32, i32, vp, vp, C.POINTER(C.c_int64)],
        "sbbseg_segment_pages": [vp, i32, vp, i32, i32, vp],
        "sbbseg_deskew_side": [i32, i32, C.POINTER(C.c_int)],
        "sbbseg_rotation_matrix": [C.c_double, C.c_double, C.c_double, vp],
        "sbbseg_deskew_profiles_dev": [vp, vp, i32, i32, vp, vp, i32, vp],
        "sbbseg_deskew_profiles": [vp, vp, i32, i32, vp, vp, i32, vp],
        "sbbseg_debug_inject_alloc_failure": [i32],
        "sbbseg_profile_enable": [vp, i32],
        "sbbseg_profile_reset": [vp],
        "sbbseg_profile_get": [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
        "sbbseg_text_regions_present_dev": [vp, vp, i32, i32, i32, C.c_double, C.POINTER(C.c_int)],
        "sbbseg_debug_largest_contour_area2": [vp, i32, i32, C.POINTER(C.c_int64)],
        "sbbseg_run_page": [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(RunInfo)],
        "sbbseg_device_alloc": [vp, C.c_size_t, C.POINTER(vp)],
        "sbbseg_device_free": [vp, vp],
        "sbbseg_upload": [vp, vp, vp, C.c_size_t],
        "sbbseg_download": [vp, vp, vp, C.c_size_t],
        "sbbseg_download_labels": [vp, vp, vp, C.c_size_t, i32],
        "sbbseg_set_owned_regions": [vp, i32],
        "sbbseg_owned_region_info": [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "sbbseg_op_executed": [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double)],
        "sbbseg_debug_owned_range": [i32, i32, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "sbbseg_debug_region_rows": [i32, i32, i32, i32, i32, i32, vp, vp],
        "sbbseg_debug_poison_activations": [vp, i32],
        "sbbseg_debug_op_launch": [vp, i32, vp, i32],
        "sbbseg_debug_tensor_period_mismatches": [vp, i32, i32, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
        "sbbseg_text_region_boxes_dev": [vp, vp, i32, i32, i32, C.c_double, C.c_double, vp, i32, C.POINTER(C.c_int)],
        "sbbseg_text_region_boxes": [vp, vp, i32, i32, i32, C.c_double, C.c_double, vp, i32, C.POINTER(C.c_int)],
        "sbbseg_region_deskew_profiles_dev": [vp, vp, i32, i32, vp, i32, i32, vp, i32, vp, vp],
        "sbbseg_region_deskew_profiles": [vp, vp, i32, i32, vp, i32, i32, vp, i32, vp, vp],
        "sbbseg_profile_statistics_host": [vp, vp, i32, i32, vp, i32, C.c_double, vp, vp, vp, vp],
        "sbbseg_profile_statistics_dev": [vp, vp, vp, i32, i32, vp, i32, C.c_double, vp, vp, vp],
        "sbbseg_deskew_sweep_angles": [i32, vp, i32, C.POINTER(C.c_int)],
        "sbbseg_region_deskew_slopes_dev": [vp, vp, i32, i32, vp, i32, i32, vp, i32, vp],
        "sbbseg_region_deskew_slopes": [vp, vp, i32, i32, vp, i32, i32, vp, i32, vp],
        "sbbseg_region_line_masks_dev": [vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
        "sbbseg_region_line_masks": [vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
        "sbbseg_region_line_masks_host": [vp, i32, i32, i32, C.c_double, vp, vp, vp],
        "sbbseg_region_line_table": [vp, i32],
        "sbbseg_line_split_host": [vp, vp, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp],
        "sbbseg_line_split_dev": [vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp],
        "sbbseg_region_line_boxes_dev": [vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp],
        "sbbseg_region_line_boxes": [vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp],
        "sbbseg_run_pages_planes": [vp, i32, C.POINTER(Plane), C.POINTER(Plane)],
        "sbbseg_planes_deskew_slopes_dev": [vp, C.POINTER(Plane), i32, vp, vp, i32, i32, vp, i32, vp],
        "sbbseg_planes_line_masks_dev": [vp, C.POINTER(Plane), i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
        "sbbseg_planes_line_boxes_dev": [vp, C.POINTER(Plane), i32, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp],
        "sbbseg_text_region_contours_dev": [vp, vp, i32, i32, i32, C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int64)],
        "sbbseg_text_region_contours": [vp, vp, i32, i32, i32, C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int64)],
        "sbbseg_text_region_contours_read": [vp, vp, vp, vp, i32, vp, C.c_int64],
        "sbbseg_mask_contours_host": [vp, i32, i32, vp, vp, vp, i32, vp, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int64)],
        "sbbseg_debug_mask_contours_dev": [vp, vp, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int64)],
        "sbbseg_debug_set_contour_lds_limit": [vp, i32],
        "sbbseg_debug_contour_launches": [vp, C.POINTER(C.c_int64)],
        "sbbseg_debug_set_contour_host_step_bound": [C.c_int64],
        "sbbseg_debug_profile_statistics": [vp, vp, vp, i32, i32, vp, i32, C.c_double, vp, vp, vp, vp, vp],
        "sbbseg_debug_soft_arith": [vp, i32, vp, vp, C.c_int64, vp],
        "sbbseg_contour_moments_dev": [vp, vp, vp, i32, vp, vp, vp],
        "sbbseg_contour_moments_host": [vp, vp, i32, vp, vp, vp],
        "sbbseg_region_order_dev": [vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, C.POINTER(C.c_int)],
        "sbbseg_region_order": [vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, C.POINTER(C.c_int)],
        "sbbseg_region_order_host": [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, C.POINTER(C.c_int)],
        "sbbseg_debug_row_sums": [vp, vp, i32, i32, vp],
        "sbbseg_debug_order_launches": [vp, C.POINTER(C.c_int64)],
        "sbbseg_region_line_extents_dev": [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "sbbseg_region_line_extents_read": [vp, i32, vp, vp, i32],
        "sbbseg_region_line_extents_host": [vp, i32, vp, C.c_double, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32],
        "sbbseg_region_line_extent_weights": [vp, i32],
        "sbbseg_debug_mask_border_winner_dev": [vp, vp, vp, i32, vp],
        "sbbseg_debug_mask_border_winner_host": [vp, i32, i32, vp, vp, i32],
        "sbbseg_debug_set_extent_lds_limit": [vp, i32],
        "sbbseg_debug_extent_launches": [vp, C.POINTER(C.c_int64)],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    if lib.sbbseg_abi_version() != 5:
        raise RuntimeError("libsbbseg ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def check(rc: int, what: str = "libsbbseg"):
    if rc != 0:
        msg = load_library().sbbseg_last_error()
        raise RuntimeError(f"{what}: {msg.decode('utf-8', 'replace') if msg else 'unknown error'}")


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# sbbseg_debug_op_launch: SBBSEG_LAUNCH_* family numbers and the order of the record's ints (include/sbbseg.h)
LAUNCH_FAMILIES = ("none", "conv_igemm", "conv_naive_f32", "conv_splitk", "stem", "stem_pool", "direct64", "bottleneck", "bottleneck_pq",
                   "block_x3", "expand_reduce", "conv3_expand_reduce", "dec_halo", "tail", "maxpool", "head")
LAUNCH_FIELDS = ("family", "BP", "BC", "stages", "fast_gather", "tile_map", "cls_minor", "table", "n_tiles", "grid", "res_epilogue",
                 "persistent", "residual")
LINE_SIGMA_MAX = 128                                             # largest sigma of the line splitter's device table (csrc/line_split.h)
LINES_OK, LINES_NONE, LINES_SIGMA_TOO_LARGE = 0, 1, 2


class Context:
    """Owns one sbbseg_ctx (one GPU, one plan)."""

    def __init__(self, device: int = 0, precision: int = PREC_BF16, _handle=None):
        self.lib = load_library()
        if _handle is None:
            h = C.c_void_p()
            check(self.lib.sbbseg_create(device, precision, C.byref(h)), "sbbseg_create")
        else:
            h = _handle
        self.h = h
        self.device, self.precision = device, precision
        self.tensor_ids = []

    @classmethod
    def from_sbbw(cls, source, device: int, precision: int, max_batch: int, flags: int = 0) -> "Context":
        """One-call load through the library's own graph reader + planner (sbbseg_model_load[_file]): ``source`` is a path or the
        container's bytes.  The handle comes back finalized."""
        lib = load_library()
        h = C.c_void_p()
        if isinstance(source, (bytes, bytearray, memoryview)):
            buf = bytes(source)
            check(lib.sbbseg_model_load(buf, len(buf), device, precision, int(max_batch), int(flags), C.byref(h)), "sbbseg_model_load")
        else:
            check(lib.sbbseg_model_load_file(os.fsencode(source), device, precision, int(max_batch), int(flags), C.byref(h)), "sbbseg_model_load_file")
        return cls(device, precision, _handle=h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.sbbseg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plan upload ---------------------------------------------------------------------------
    def load_plan(self, plan, max_batch: int):
        lib, h = self.lib, self.h
        check(lib.sbbseg_set_input(h, plan.in_h, plan.in_w, 3))
        ids = []
        for t in plan.tensors:
            tid = C.c_int(-1)
            if t.kind == "input_c8":
                check(lib.sbbseg_input_form(h, INPUT_C8, 0, C.byref(tid)))
            elif t.kind == "input_pairs":
                check(lib.sbbseg_input_form(h, INPUT_PAIRS, t.pad, C.byref(tid)))
            elif t.kind == "unused":
                pass                                   # e.g. the last conv's output when the head is fused
            else:
                check(lib.sbbseg_add_tensor(h, t.H, t.W, t.C, C.byref(tid)))
            ids.append(tid.value)
        self.tensor_ids = ids
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        for s in plan.steps:
            if s.kind == "conv":
                d = ConvDesc()
                d.n_src = len(s.srcs)
                keep = []
                for k, g in enumerate(s.srcs):
                    d.src[k] = ConvSrc(ids[g.tensor], g.channels, g.kh, g.kw, g.stride_y, g.stride_x, g.pad_top,
                                       g.pad_left, g.shift, g.off_y, g.off_x)
                    keep.append(f32(g.w))
                d.cout, d.out_h, d.out_w = s.cout, s.out_h, s.out_w
                d.out_stride_y, d.out_stride_x = s.out_stride
                d.out_off_y, d.out_off_x = s.out_off
                d.out_tensor = ids[s.out] if s.out >= 0 else -1
                d.relu = int(s.relu)
                d.residual_tensor = ids[s.residual] if s.residual >= 0 else -1
                d.raw_out_tensor = ids[s.raw_out] if s.raw_out >= 0 else -1
                d.head_classes = s.head.classes if s.head is not None else 0
                d.algorithmic_macs = float(s.algorithmic_macs)
                sc, sh, rs, rb = f32(s.scale), f32(s.shift), f32(s.raw_scale), f32(s.raw_shift)
                hw = hs = hb = None
                if s.head is not None:
                    hw, hs, hb = f32(s.head.w), f32(s.head.scale), f32(s.head.shift)
                check(lib.sbbseg_add_conv(h, C.byref(d), _ptr(keep[0]), _ptr(keep[1]) if len(keep) > 1 else None,
                                          _ptr(sc), _ptr(sh), _ptr(rs), _ptr(rb), _ptr(hw), _ptr(hs), _ptr(hb)),
                      f"sbbseg_add_conv({s.name})")
            elif s.kind == "tail":
                arrs = [f32(s.w_src0), f32(s.w_img), f32(s.scale), f32(s.shift), f32(s.head.w), f32(s.head.scale), f32(s.head.shift)]
                check(lib.sbbseg_add_tail(h, ids[s.src0], ids[s.img], _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), _ptr(arrs[3]),
                                          s.head.classes, _ptr(arrs[4]), _ptr(arrs[5]), _ptr(arrs[6]), float(s.algorithmic_macs)),
                      f"sbbseg_add_tail({s.name})")
            elif s.kind == "maxpool":
                ps, pb = f32(s.pre_scale), f32(s.pre_shift)
                check(lib.sbbseg_add_maxpool(h, ids[s.src], ids[s.dst], s.k, s.stride, _ptr(ps), _ptr(pb), int(s.pre_relu)),
                      f"sbbseg_add_maxpool({s.name})")
            elif s.kind == "head":
                w = np.ascontiguousarray(s.w, np.float32)
                sc, sh = np.ascontiguousarray(s.scale, np.float32), np.ascontiguousarray(s.shift, np.float32)
                check(lib.sbbseg_add_head(h, ids[s.src], s.cin, s.classes, _ptr(w), _ptr(sc), _ptr(sh)),
                      f"sbbseg_add_head({s.name})")
            else:
                raise RuntimeError(f"unknown plan step {s.kind}")
        check(lib.sbbseg_finalize(h, int(max_batch)), "sbbseg_finalize")

    # -- queries -------------------------------------------------------------------------------
    def model_info(self):
        v = [C.c_int() for _ in range(4)]
        check(self.lib.sbbseg_model_info(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)          # H, W, classes, max_batch

    def ops(self):
        n = C.c_int()
        check(self.lib.sbbseg_num_ops(self.h, C.byref(n)))
        out = []
        for i in range(n.value):
            buf = C.create_string_buffer(128)
            fl, by = C.c_double(), C.c_double()
            check(self.lib.sbbseg_op_info(self.h, i, buf, 128, C.byref(fl), C.byref(by)))
            iss = C.c_double()
            check(self.lib.sbbseg_op_issued_flops(self.h, i, C.byref(iss)))
            out.append({"index": i, "name": buf.value.decode(), "flops": fl.value, "issued_flops": iss.value, "min_bytes": by.value})
        return out

    def device_bytes(self) -> int:
        b = C.c_size_t()
        check(self.lib.sbbseg_device_bytes(self.h, C.byref(b)))
        return b.value

    def set_stream(self, stream_ptr: int):
        """Run on the caller's HIP stream (0 = the legacy default stream); -1 = the handle's own stream."""
        check(self.lib.sbbseg_set_stream(self.h, C.c_void_p(stream_ptr if stream_ptr >= 0 else 2 ** 64 - 1)))

    def synchronize(self):
        check(self.lib.sbbseg_synchronize(self.h))

    def set_lanes(self, lanes: int):
        """1 = one stream; 2 (default) = chunks of >= 16 tiles run as two concurrent halves (see sbbseg.h)."""
        check(self.lib.sbbseg_set_lanes(self.h, int(lanes)), "sbbseg_set_lanes")

    def set_dedupe(self, on: bool):
        """Fused page paths compute a repeated clamped tile once (default on; same label map).  See sbbseg.h."""
        check(self.lib.sbbseg_set_dedupe(self.h, int(bool(on))), "sbbseg_set_dedupe")

    def set_ksplit(self, on: bool):
        """Whole-image branch: split the K range of one-patch launches over the idle CUs (default on; see sbbseg.h)."""
        check(self.lib.sbbseg_set_ksplit(self.h, int(bool(on))), "sbbseg_set_ksplit")

    def set_owned_regions(self, mode: int):
        """Decoder launches over the region the page stitch keeps of every tile (+ halo) only: 0 = off, 1 = fused page paths
        (default), 2 = the tile-range entry points too (their tile labels are then defined on the owned regions only).  See sbbseg.h."""
        check(self.lib.sbbseg_set_owned_regions(self.h, int(mode)), "sbbseg_set_owned_regions")

    def owned_region_levels(self) -> int:
        """Decoder levels this plan runs as owned-region launches (0: everything is computed whole)."""
        return self.owned_region_info()[1]

    def owned_region_info(self):
        """(mode in force, decoder levels the plan runs as owned-region launches)."""
        mode, levels = C.c_int(0), C.c_int(0)
        check(self.lib.sbbseg_owned_region_info(self.h, C.byref(mode), C.byref(levels)), "sbbseg_owned_region_info")
        return int(mode.value), int(levels.value)

    def poison_activations(self, byte_value: int = 0xFF):
        """Test hook: fill every activation buffer, the tile-label scratch and the split-K workspace of the whole-image branch (where
        one has been allocated) with a byte (0xFF = NaN in every 16-bit format and in fp32)."""
        check(self.lib.sbbseg_debug_poison_activations(self.h, int(byte_value)), "sbbseg_debug_poison_activations")

    def op_launch(self, op: int) -> dict:
        """Test hook: what the last launch of plan op `op` used -- {field of LAUNCH_FIELDS: int}, "family" as its name of
        LAUNCH_FAMILIES ("none": the op launched nothing, it is fused into another op's launch)."""
        rec = np.zeros(len(LAUNCH_FIELDS), np.int32)
        check(self.lib.sbbseg_debug_op_launch(self.h, int(op), _ptr(rec), rec.size), "sbbseg_debug_op_launch")
        out = {k: int(v) for k, v in zip(LAUNCH_FIELDS, rec)}
        out["family"] = LAUNCH_FAMILIES[out["family"]]
        return out

    def tensor_period_mismatches(self, plan_tensor: int, n: int, period: int):
        """Test hook: (bytes in which stored patch i differs from patch i - period over period <= i < n, offset of the first one from
        the start of patch `period` or -1), compared on the device over the whole patch stride."""
        if not self.tensor_ids and getattr(self, "ids_provider", None) is not None:
            self.ids_provider()
        cnt, first = C.c_int64(0), C.c_int64(-1)
        check(self.lib.sbbseg_debug_tensor_period_mismatches(self.h, self.tensor_ids[plan_tensor], int(n), int(period), C.byref(cnt), C.byref(first)),
              "sbbseg_debug_tensor_period_mismatches")
        return int(cnt.value), int(first.value)

    def forwards(self) -> int:
        """Patches run through the plan on this handle so far."""
        v = C.c_int64(0)
        check(self.lib.sbbseg_debug_counter(self.h, 1, C.byref(v)), "sbbseg_debug_counter")
        return int(v.value)

    def _label_out(self, h: int, w: int, channels: int) -> np.ndarray:
        """Output array for a host label map: one plane, or the reference's 3 identical channels (replicated on the
        device: numpy needs ~12 ms to do that for a 3500x2500 page, more than the whole forward pass)."""
        if channels not in (1, 3):
            raise ValueError("channels must be 1 or 3")
        check(self.lib.sbbseg_set_label_channels(self.h, channels), "sbbseg_set_label_channels")
        return np.empty((h, w) if channels == 1 else (h, w, 3), np.uint8)

    # -- execution -----------------------------------------------------------------------------
    def predict(self, x: np.ndarray) -> np.ndarray:
        H, W, classes, _ = self.model_info()
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 4 or x.shape[1:] != (H, W, 3):
            raise ValueError(f"predict expects [n,{H},{W},3], got {x.shape}")
        out = np.empty((x.shape[0], H, W, classes), np.float32)
        check(self.lib.sbbseg_predict(self.h, _ptr(x), x.shape[0], _ptr(out)), "sbbseg_predict")
        return out

    def segment_page(self, page: np.ndarray, channels: int = 1) -> np.ndarray:
        page = np.ascontiguousarray(page, np.uint8)
        if page.ndim != 3 or page.shape[2] != 3:
            raise ValueError(f"page must be uint8 [H,W,3], got {page.shape}")
        out = self._label_out(page.shape[0], page.shape[1], channels)
        check(self.lib.sbbseg_segment_page(self.h, _ptr(page), page.shape[0], page.shape[1], _ptr(out)), "sbbseg_segment_page")
        return out

    def segment_page_scaled(self, page: np.ndarray, out_h: int, out_w: int, channels: int = 1) -> np.ndarray:
        page = np.ascontiguousarray(page, np.uint8)
        out = self._label_out(out_h, out_w, channels)
        check(self.lib.sbbseg_segment_page_scaled(self.h, _ptr(page), page.shape[0], page.shape[1], out_h, out_w, _ptr(out)),
              "sbbseg_segment_page_scaled")
        return out

    def segment_page_otsu(self, page: np.ndarray, out_h: int = 0, out_w: int = 0, channels: int = 1):
        """extract_text_regions (main.py:439-447) in one call: (optional nearest rescale to out_h x out_w) +
        otsu_copy + do_prediction(patches=True).  Returns (labels uint8 [out_h, out_w], Otsu threshold)."""
        page = np.ascontiguousarray(page, np.uint8)
        if page.ndim != 3 or page.shape[2] != 3:
            raise ValueError(f"page must be uint8 [H,W,3], got {page.shape}")
        out_h, out_w = (out_h or page.shape[0]), (out_w or page.shape[1])
        out = self._label_out(out_h, out_w, channels)
        thr = C.c_int(0)
        check(self.lib.sbbseg_segment_page_otsu(self.h, _ptr(page), page.shape[0], page.shape[1], out_h, out_w, _ptr(out),
                                                C.byref(thr)), "sbbseg_segment_page_otsu")
        return out, int(thr.value)

    def segment_crop(self, page: np.ndarray, scaled_h: int, scaled_w: int, box, binarise: bool = False, channels: int = 1):
        """A patch stage on extract_page's cropped page (main.py:2061-2102): ``page`` = the stored image, ``scaled_*`` its size
        after get_image_and_scales, ``box`` = (x, y, w, h) on the upscaled page.  Returns (labels [h][w] (x3), Otsu threshold or
        None); ``binarise`` = the layout stage's otsu_copy on the crop."""
        page = np.ascontiguousarray(page, np.uint8)
        x, y, w, h = (int(v) for v in box)
        out = self._label_out(h, w, channels)
        thr = C.c_int(0)
        check(self.lib.sbbseg_segment_crop(self.h, _ptr(page), page.shape[0], page.shape[1], int(scaled_h), int(scaled_w), x, y, w, h,
                                           1 if binarise else 0, _ptr(out), C.byref(thr)), "sbbseg_segment_crop")
        return out, (int(thr.value) if binarise else None)

    def segment_crop_dev(self, d_page: int, Hs: int, Ws: int, scaled_h: int, scaled_w: int, box, binarise: bool, d_labels: int, d_threshold: int = 0):
        x, y, w, h = (int(v) for v in box)
        check(self.lib.sbbseg_segment_crop_dev(self.h, C.c_void_p(d_page), Hs, Ws, int(scaled_h), int(scaled_w), x, y, w, h,
                                               1 if binarise else 0, C.c_void_p(d_labels), C.c_void_p(d_threshold or None)), "sbbseg_segment_crop_dev")

    def segment_views_dev(self, views):
        """Many crops in one call, tiles pooled across them (sbbseg_segment_views_dev).  ``views``: a sequence of
        (d_page, Hs, Ws, scaled_h, scaled_w, box, binarise, d_labels[, d_threshold]) -- the arguments of :meth:`segment_crop_dev`, per view."""
        arr = (View * max(len(views), 1))()
        for k, v in enumerate(views):
            d_page, Hs, Ws, Hp, Wp, box, binarise, d_labels = v[:8]
            x, y, w, h = (int(q) for q in box)
            arr[k] = View(int(d_page) or None, int(Hs), int(Ws), int(Hp), int(Wp), x, y, w, h, 1 if binarise else 0, int(d_labels) or None,
                          (int(v[8]) if len(v) > 8 else 0) or None)
        check(self.lib.sbbseg_segment_views_dev(self.h, len(views), arr), "sbbseg_segment_views_dev")

    def segment_views(self, views, channels: int = 1):
        """The host form: ``views`` = a sequence of (page, scaled_h, scaled_w, box, binarise) as :meth:`segment_crop` takes them; views that
        pass the same array object share one upload.  Returns [(labels [h][w] (x3), Otsu threshold or None), ...]."""
        if channels not in (1, 3):
            raise ValueError("channels must be 1 or 3")
        check(self.lib.sbbseg_set_label_channels(self.h, channels), "sbbseg_set_label_channels")
        arr = (View * max(len(views), 1))()
        pages, outs = {}, []
        for k, (page, Hp, Wp, box, binarise) in enumerate(views):
            pg = pages.setdefault(id(page), np.ascontiguousarray(page, np.uint8))
            if pg.ndim != 3 or pg.shape[2] != 3:
                raise ValueError(f"view {k}: page must be uint8 [H,W,3], got {pg.shape}")
            x, y, w, h = (int(q) for q in box)
            if w < 1 or h < 1:
                raise ValueError(f"view {k}: empty box {tuple(box)}")
            outs.append(np.empty((h, w) if channels == 1 else (h, w, 3), np.uint8))
            arr[k] = View(pg.ctypes.data, pg.shape[0], pg.shape[1], int(Hp), int(Wp), x, y, w, h, 1 if binarise else 0, outs[k].ctypes.data, None)
        thr = np.zeros(max(len(views), 1), np.int32)
        check(self.lib.sbbseg_segment_views(self.h, len(views), arr, _ptr(thr)), "sbbseg_segment_views")
        return [(outs[k], int(thr[k]) if views[k][4] else None) for k in range(len(views))]

    def views_launches(self) -> int:
        """Ingest + region-table + stitch kernels :meth:`segment_views_dev` has queued on this handle so far (sbbseg_debug_counter 3)."""
        return self.debug_counter(3)

    def debug_counter(self, which: int) -> int:
        v = C.c_int64(0)
        check(self.lib.sbbseg_debug_counter(self.h, int(which), C.byref(v)), "sbbseg_debug_counter")
        return int(v.value)

    # -- the sharded path's collective on RCCL, inside the library (no torch.distributed needed) ------------------
    def comm_init(self, rank: int, world: int, unique_id: bytes):
        """Join the communicator `unique_id` (from :func:`comm_unique_id` on rank 0) as `rank` of `world`; collective."""
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        check(self.lib.sbbseg_comm_init(self.h, int(rank), int(world), C.create_string_buffer(bytes(unique_id), 128)), "sbbseg_comm_init")

    def comm_info(self):
        r, w = C.c_int(0), C.c_int(0)
        check(self.lib.sbbseg_comm_info(self.h, C.byref(r), C.byref(w)), "sbbseg_comm_info")
        return int(r.value), int(w.value)

    def comm_destroy(self):
        check(self.lib.sbbseg_comm_destroy(self.h), "sbbseg_comm_destroy")

    def allgather_labels_dev(self, d_send: int, bytes_per_rank: int, d_recv: int):
        """All-gather of u8 label maps over RCCL on the handle's stream: d_recv = [world][bytes_per_rank]."""
        check(self.lib.sbbseg_allgather_labels_dev(self.h, C.c_void_p(d_send), int(bytes_per_rank), C.c_void_p(d_recv)), "sbbseg_allgather_labels_dev")

    def otsu_dev(self, d_page: int, Hp: int, Wp: int, d_threshold: int):
        check(self.lib.sbbseg_otsu_dev(self.h, C.c_void_p(d_page), Hp, Wp, C.c_void_p(d_threshold)), "sbbseg_otsu_dev")

    def segment_tile_range_bin_dev(self, d_page: int, Hp: int, Wp: int, first: int, n: int, d_threshold: int, d_tile_labels: int):
        check(self.lib.sbbseg_segment_tile_range_bin_dev(self.h, C.c_void_p(d_page), Hp, Wp, first, n, C.c_void_p(d_threshold),
                                                         C.c_void_p(d_tile_labels)), "sbbseg_segment_tile_range_bin_dev")

    def segment_whole(self, page: np.ndarray, out_h: int, out_w: int, channels: int = 1) -> np.ndarray:
        page = np.ascontiguousarray(page, np.uint8)
        out = self._label_out(out_h, out_w, channels)
        check(self.lib.sbbseg_segment_whole(self.h, _ptr(page), page.shape[0], page.shape[1], out_h, out_w, _ptr(out)),
              "sbbseg_segment_whole")
        return out

    def segment_whole_scaled(self, page: np.ndarray, scaled_h: int, scaled_w: int, out_h: int, out_w: int, channels: int = 1) -> np.ndarray:
        """Whole-image branch on the stored page as if it had first been nearest-upscaled to scaled_h x scaled_w."""
        page = np.ascontiguousarray(page, np.uint8)
        out = self._label_out(out_h, out_w, channels)
        check(self.lib.sbbseg_segment_whole_scaled(self.h, _ptr(page), page.shape[0], page.shape[1], scaled_h, scaled_w, out_h, out_w,
                                                   _ptr(out)), "sbbseg_segment_whole_scaled")
        return out

    @staticmethod
    def _whole_views(views):
        arr = (WholeView * max(len(views), 1))()
        for k, (d_page, stored_h, stored_w, page_h, page_w, out_h, out_w, d_labels) in enumerate(views):
            arr[k] = WholeView(int(d_page) or None, int(stored_h), int(stored_w), int(page_h), int(page_w), int(out_h), int(out_w), int(d_labels) or None)
        return arr

    def segment_whole_views_dev(self, views):
        """The whole-image branch for many pages in shared launches (sbbseg_segment_whole_views_dev).  ``views``: a sequence of
        (d_page, stored_h, stored_w, page_h, page_w, out_h, out_w, d_labels) -- device pointers, the stored page's size, its size after
        get_image_and_scales, and the size of the label plane to write."""
        check(self.lib.sbbseg_segment_whole_views_dev(self.h, len(views), self._whole_views(views)), "sbbseg_segment_whole_views_dev")

    def extract_page_boxes_dev(self, views):
        """Border model + page box for many pages (sbbseg_extract_page_boxes_dev).  ``views`` as :meth:`segment_whole_views_dev` takes
        them, out size == page size, d_labels = 0: the mask stays in library scratch.  Returns [((x, y, w, h), pixels), ...]; an empty
        mask gives ((0, 0, 0, 0), 0)."""
        n = len(views)
        boxes = np.zeros((max(n, 1), 4), np.int32)
        px = np.zeros(max(n, 1), np.int64)
        check(self.lib.sbbseg_extract_page_boxes_dev(self.h, n, self._whole_views(views), _ptr(boxes), _ptr(px)), "sbbseg_extract_page_boxes_dev")
        return [(tuple(int(v) for v in boxes[k]), int(px[k])) for k in range(n)]

    def whole_launches(self) -> int:
        """Ingest + label-resize kernels the whole-views calls have queued on this handle so far (sbbseg_debug_counter 4)."""
        return self.debug_counter(4)

    def segment_page_dev(self, d_page: int, Hp: int, Wp: int, d_labels: int):
        check(self.lib.sbbseg_segment_page_dev(self.h, C.c_void_p(d_page), Hp, Wp, C.c_void_p(d_labels)), "sbbseg_segment_page_dev")

    def segment_pages_dev(self, d_pages, Hp: int, Wp: int, d_labels):
        """Equally sized pages (device pointers) -> their label maps (device pointers), tiles pooled across pages."""
        n = len(d_pages)
        if n != len(d_labels) or n == 0:
            raise ValueError("need as many label buffers as pages (at least one)")
        pa = (C.c_void_p * n)(*[C.c_void_p(int(v)) for v in d_pages])
        la = (C.c_void_p * n)(*[C.c_void_p(int(v)) for v in d_labels])
        check(self.lib.sbbseg_segment_pages_dev(self.h, n, pa, Hp, Wp, la), "sbbseg_segment_pages_dev")

    def segment_tile_range_dev(self, d_page: int, Hp: int, Wp: int, first: int, n: int, d_tile_labels: int):
        check(self.lib.sbbseg_segment_tile_range_dev(self.h, C.c_void_p(d_page), Hp, Wp, first, n, C.c_void_p(d_tile_labels)),
              "sbbseg_segment_tile_range_dev")

    def segment_tiles_dev(self, d_page: int, Hp: int, Wp: int, tile_xy: np.ndarray, d_tile_labels: int):
        xy = np.ascontiguousarray(tile_xy, np.int32)
        check(self.lib.sbbseg_segment_tiles_dev(self.h, C.c_void_p(d_page), Hp, Wp, _ptr(xy), xy.shape[0], C.c_void_p(d_tile_labels)),
              "sbbseg_segment_tiles_dev")

    def stitch_dev(self, d_tile_labels: int, Hp: int, Wp: int, d_labels: int):
        check(self.lib.sbbseg_stitch_dev(self.h, C.c_void_p(d_tile_labels), Hp, Wp, C.c_void_p(d_labels)), "sbbseg_stitch_dev")

    def debug_ingest(self, page: np.ndarray, tile_xy: np.ndarray, form: int, shape) -> np.ndarray:
        page = np.ascontiguousarray(page, np.uint8)
        xy = np.ascontiguousarray(tile_xy, np.int32)
        out = np.empty((xy.shape[0],) + tuple(shape), np.float32)
        check(self.lib.sbbseg_debug_ingest(self.h, _ptr(page), page.shape[0], page.shape[1], _ptr(xy), xy.shape[0], form,
                                           _ptr(out), out.size), "sbbseg_debug_ingest")
        return out

    def debug_read_tensor(self, plan_tensor: int, n: int, shape) -> np.ndarray:
        if not self.tensor_ids and getattr(self, "ids_provider", None) is not None:
            self.ids_provider()                       # natively planned handle: ids re-derived from the mirror plan (model.py)
        out = np.empty((n,) + tuple(shape), np.float32)
        check(self.lib.sbbseg_debug_read_tensor(self.h, self.tensor_ids[plan_tensor], n, _ptr(out), out.size),
              "sbbseg_debug_read_tensor")
        return out

    # -- stage glue ---------------------------------------------------------------
    def morph(self, plane: np.ndarray, op: int, ksize: int = 5, iterations: int = 1) -> np.ndarray:
        """cv2.erode (op 0) / cv2.dilate (op 1) of a uint8 plane [H,W] with a ksize x ksize kernel of ones, on the device."""
        plane = np.ascontiguousarray(plane, np.uint8)
        if plane.ndim != 2:
            raise ValueError("morph expects a uint8 plane [H, W]")
        out = np.empty_like(plane)
        check(self.lib.sbbseg_morph(self.h, _ptr(plane), plane.shape[0], plane.shape[1], int(op), int(ksize), int(iterations), _ptr(out)),
              "sbbseg_morph")
        return out

    def morph_dev(self, d_src: int, H: int, W: int, op: int, ksize: int, iterations: int, d_dst: int):
        check(self.lib.sbbseg_morph_dev(self.h, C.c_void_p(d_src), H, W, int(op), int(ksize), int(iterations), C.c_void_p(d_dst)), "sbbseg_morph_dev")

    # -- device buffers (callers without torch: stages.InferenceStages.run) ------------------------------------------
    def device_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        check(self.lib.sbbseg_device_alloc(self.h, int(nbytes), C.byref(p)), "sbbseg_device_alloc")
        return int(p.value)

    def device_free(self, d_ptr: int):
        if d_ptr and getattr(self, "h", None):
            check(self.lib.sbbseg_device_free(self.h, C.c_void_p(d_ptr)), "sbbseg_device_free")

    def upload(self, d_dst: int, a: np.ndarray):
        a = np.ascontiguousarray(a)
        check(self.lib.sbbseg_upload(self.h, C.c_void_p(d_dst), _ptr(a), a.nbytes), "sbbseg_upload")

    def download(self, d_src: int, shape, dtype=np.uint8) -> np.ndarray:
        out = np.empty(shape, dtype)
        check(self.lib.sbbseg_download(self.h, _ptr(out), C.c_void_p(d_src), out.nbytes), "sbbseg_download")
        return out

    def download_labels(self, d_labels: int, h: int, w: int, channels: int = 1) -> np.ndarray:
        out = np.empty((h, w, 3) if channels == 3 else (h, w), np.uint8)
        check(self.lib.sbbseg_download_labels(self.h, _ptr(out), C.c_void_p(d_labels), h * w, channels), "sbbseg_download_labels")
        return out

    def text_regions_present_dev(self, d_regions: int, H: int, W: int, label: int = 1, min_area: float = 0.00001) -> bool:
        """get_text_region_contours_and_boxes' `len(contours) > 0` (main.py:456-480, 2083-2096) on a device label plane."""
        present = C.c_int(0)
        check(self.lib.sbbseg_text_regions_present_dev(self.h, C.c_void_p(d_regions), H, W, label, float(min_area), C.byref(present)),
              "sbbseg_text_regions_present_dev")
        return bool(present.value)

    def text_regions_present(self, regions: np.ndarray, label: int = 1, min_area: float = 0.00001) -> bool:
        plane = np.ascontiguousarray(regions[:, :, 0] if regions.ndim == 3 else regions, np.uint8)
        return self.text_regions_present_dev(self.stage(plane), plane.shape[0], plane.shape[1], label, min_area)

    def stage(self, plane: np.ndarray) -> int:
        """Upload a host plane into the staging buffer cached on the Context (grown on demand, released with the handle:
        sbbseg_device_free synchronises the device); returns the device pointer, valid until the next stage()."""
        cap = getattr(self, "_gate_cap", 0)
        if cap < plane.nbytes:
            if cap:
                self.device_free(self._gate_buf)
            self._gate_buf, self._gate_cap = self.device_alloc(plane.nbytes), plane.nbytes
        self.upload(self._gate_buf, plane)
        return self._gate_buf

    def text_region_boxes_dev(self, d_regions: int, H: int, W: int, label: int = 1, min_area: float = 0.00001, max_area: float = 1.0):
        """get_text_region_contours_and_boxes' ``self.boxes`` (main.py:456-480) from a device label plane: a list of [x, y, w, h].
        Order [EXT, unpinned]: first pixel in raster order, descending (see sbbseg.h)."""
        return self._boxes_call(self.lib.sbbseg_text_region_boxes_dev, C.c_void_p(d_regions), H, W, label, min_area, max_area)

    def text_region_boxes(self, regions: np.ndarray, label: int = 1, min_area: float = 0.00001, max_area: float = 1.0):
        """The same from a host label map ([H, W] or [H, W, 3]: all channels must equal ``label``, main.py:458)."""
        regions = np.asarray(regions)
        if regions.ndim == 3:
            plane = np.where(np.all(regions == label, axis=-1), label, (label + 1) & 255).astype(np.uint8)      # any value but the label
        else:
            plane = np.ascontiguousarray(regions, np.uint8)
        return self._boxes_call(self.lib.sbbseg_text_region_boxes, _ptr(plane), plane.shape[0], plane.shape[1], label, min_area, max_area)

    def _boxes_call(self, fn, src, H, W, label, min_area, max_area):
        n = C.c_int(0)
        cap = 64
        while True:                                             # a second call only when there are more boxes than the first guess
            boxes = np.zeros((cap, 4), np.int32)
            check(fn(self.h, src, int(H), int(W), int(label), float(min_area), float(max_area), _ptr(boxes), cap, C.byref(n)), "sbbseg_text_region_boxes")
            if n.value <= cap:
                return [[int(v) for v in b] for b in boxes[:n.value]]
            cap = n.value

    def text_region_contours_dev(self, d_regions: int, H: int, W: int, label: int = 1, min_area: float = 0.00001, max_area: float = 1.0):
        """get_text_region_contours_and_boxes (main.py:456-481) from a device label plane, traced on the device: ``(boxes, contours)`` --
        ``self.boxes`` as :meth:`text_region_boxes_dev` gives it and, per box, the contour's CHAIN_APPROX_SIMPLE points as an int32
        [N, 2] array of (x, y).  Order [EXT, unpinned]: first pixel in raster order, descending.  The tables stay on the device
        (:meth:`contour_tables` reads them as they are)."""
        n, npts = C.c_int(0), C.c_int64(0)
        check(self.lib.sbbseg_text_region_contours_dev(self.h, C.c_void_p(d_regions), int(H), int(W), int(label), float(min_area), float(max_area),
                                                       C.byref(n), C.byref(npts)), "sbbseg_text_region_contours_dev")
        return contours_from_tables(*self.contour_tables(n.value, npts.value))

    def text_region_contours(self, regions: np.ndarray, label: int = 1, min_area: float = 0.00001, max_area: float = 1.0):
        """The same from a host label map ([H, W] or [H, W, 3]: all channels must equal ``label``, main.py:458)."""
        regions = np.asarray(regions)
        if regions.ndim == 3:
            plane = np.where(np.all(regions == label, axis=-1), label, (label + 1) & 255).astype(np.uint8)      # any value but the label
        else:
            plane = np.ascontiguousarray(regions, np.uint8)
        n, npts = C.c_int(0), C.c_int64(0)
        check(self.lib.sbbseg_text_region_contours(self.h, _ptr(plane), plane.shape[0], plane.shape[1], int(label), float(min_area), float(max_area),
                                                   C.byref(n), C.byref(npts)), "sbbseg_text_region_contours")
        return contours_from_tables(*self.contour_tables(n.value, npts.value))

    def debug_mask_contours_dev(self, d_mask: int, H: int, W: int):
        """The device tracer on a raw device mask (!= 0): every 8-connected component, no morphology, no filter; ``(boxes, contours)``."""
        n, npts = C.c_int(0), C.c_int64(0)
        check(self.lib.sbbseg_debug_mask_contours_dev(self.h, C.c_void_p(d_mask), int(H), int(W), C.byref(n), C.byref(npts)),
              "sbbseg_debug_mask_contours_dev")
        return contours_from_tables(*self.contour_tables(n.value, npts.value))

    def contour_tables(self, n_contours: int, n_points: int):
        """The handle's last contour result as the library keeps it: (boxes int32 [n, 4], area2 int64 [n], point_off int64 [n + 1],
        points int32 [points, 2]).  Arrays smaller than the result are an error that writes nothing."""
        boxes, area2 = np.zeros((n_contours, 4), np.int32), np.zeros(n_contours, np.int64)
        off, pts = np.zeros(n_contours + 1, np.int64), np.zeros((n_points, 2), np.int32)
        check(self.lib.sbbseg_text_region_contours_read(self.h, _ptr(boxes), _ptr(area2), _ptr(off), int(n_contours), _ptr(pts), int(n_points)),
              "sbbseg_text_region_contours_read")
        return boxes, area2, off, pts

    def set_contour_lds_limit(self, nbytes: int):
        """Test hook: contours whose bit map exceeds ``nbytes`` are traced on the label plane in global memory (default 65536)."""
        check(self.lib.sbbseg_debug_set_contour_lds_limit(self.h, int(nbytes)), "sbbseg_debug_set_contour_lds_limit")

    def contour_launches(self) -> int:
        """Tracer and packing kernels the contour calls have queued on this handle so far."""
        v = C.c_int64(0)
        check(self.lib.sbbseg_debug_contour_launches(self.h, C.byref(v)), "sbbseg_debug_contour_launches")
        return int(v.value)

    def contour_moments_dev(self, contours=None, n: int = 0):
        """cv2.moments' m00, m10, m01 and the centroids of main.py:1835-1836 per contour, on the device (``sbbseg_contour_moments_dev``):
        (moments float64 [n, 3], centroids float64 [n, 2], serial int32 [n]).  ``contours``: a list of int (x, y) point arrays ([N, 2] or
        the reference's [N, 1, 2] rings), or None for the ``n`` contours of the handle's resident contour result, read in place."""
        pts, off, n = (None, None, int(n)) if contours is None else pack_contours(contours)
        moments, centroids, serial = np.zeros((n, 3), np.float64), np.zeros((n, 2), np.float64), np.zeros(n, np.int32)
        check(self.lib.sbbseg_contour_moments_dev(self.h, _ptr(pts), _ptr(off), n, _ptr(moments), _ptr(centroids), _ptr(serial)),
              "sbbseg_contour_moments_dev")
        return moments, centroids, serial

    def _region_order_call(self, fn, what, src, H, W, contours, n):
        pts, off, n = (None, None, int(n)) if contours is None else pack_contours(contours)
        out = _region_order_buffers(H, n)
        ne = C.c_int(0)
        check(fn(self.h, src, int(H), int(W), _ptr(order_weights()), _ptr(pts), _ptr(off), n, *[_ptr(a) for a in out], out[-1].shape[0], C.byref(ne)), what)
        return _region_order_record(out, ne.value)

    def region_order_dev(self, d_textlines: int, H: int, W: int, contours=None, n: int = 0):
        """order_of_regions (main.py:1802-1889) for a textline plane in device memory (``sbbseg_region_order_dev``): the record of
        :func:`host_region_order`.  ``contours`` None: the ``n`` contours of the handle's resident contour result, read in place -- nothing
        but the record's few ints and doubles crosses the bus.  The plane may belong to another handle on the same device."""
        return self._region_order_call(self.lib.sbbseg_region_order_dev, "sbbseg_region_order_dev", C.c_void_p(d_textlines), H, W, contours, n)

    def region_order(self, textlines: np.ndarray, contours=None, n: int = 0):
        """The same from a host plane (uint8 [H, W]), uploaded once."""
        plane = np.ascontiguousarray(textlines, np.uint8)
        return self._region_order_call(self.lib.sbbseg_region_order, "sbbseg_region_order", _ptr(plane), plane.shape[0], plane.shape[1], contours, n)

    def debug_row_sums(self, plane: np.ndarray) -> np.ndarray:
        """``plane.sum(axis=1)`` of a uint8 [H, W] plane by the reading order's row-sum kernel: int32 [H]."""
        plane = np.ascontiguousarray(plane, np.uint8)
        out = np.zeros(plane.shape[0], np.int32)
        check(self.lib.sbbseg_debug_row_sums(self.h, _ptr(plane), plane.shape[0], plane.shape[1], _ptr(out)), "sbbseg_debug_row_sums")
        return out

    def order_launches(self) -> int:
        """Kernels the reading-order calls have queued on this handle so far."""
        v = C.c_int64(0)
        check(self.lib.sbbseg_debug_order_launches(self.h, C.byref(v)), "sbbseg_debug_order_launches")
        return int(v.value)

    def region_line_extents_raw(self, boxes, slopes, records, contours=None, fill: int = 0):
        """``sbbseg_region_line_extents_dev`` as the library packs it: (line_off int64 [n + 1], extent int32 [total, 2], corners and
        corners_rot int32 [total, 4, 2], rec int32 [n, 8]).  ``fill``: what ``extent`` and the line slots beyond every record's count hold
        before the call (tests: the call writes nothing there)."""
        boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        slopes = np.ascontiguousarray(slopes, np.float64).reshape(-1)
        n = boxes.shape[0]
        if slopes.shape[0] != n or len(records) != n:
            raise ValueError("one slope and one record per box: %d boxes, %d slopes, %d records" % (n, slopes.shape[0], len(records)))
        pts, off, nc = (None, None, n) if contours is None else pack_contours(contours)
        if nc != n:
            raise ValueError("one ring per box: %d boxes, %d rings" % (n, nc))
        rots = np.array([line_rotation_terms(int(b[2]), int(b[3]), float(s)) for b, s in zip(boxes, slopes)], np.float64).reshape(n, 6)
        info, line_off, lines, corners, corners_rot = _extent_tables(boxes, slopes, records, fill)
        extent, rec = np.full((lines.shape[0], 2), fill, np.int32), np.zeros((n, EXTENT_REC_INTS), np.int32)
        check(self.lib.sbbseg_region_line_extents_dev(self.h, _ptr(pts), _ptr(off), n, _ptr(boxes), _ptr(slopes), _ptr(rots), _ptr(info), _ptr(line_off),
                                                      _ptr(lines), _ptr(extent), _ptr(corners), _ptr(corners_rot), _ptr(rec)),
              "sbbseg_region_line_extents_dev")
        return line_off, extent, corners, corners_rot, rec

    def region_line_extents_dev(self, boxes, slopes, records, contours=None):
        """The x extent of every text line from its region's filled, rotated contour (``sbbseg_region_line_extents_dev``; the contour half
        of textline_contours_postprocessing, main.py:1492-1511, and cv2.pointPolygonTest inside seperate_lines).  ``records``: the line
        records of ``region_line_boxes_dev`` for ``boxes`` / ``slopes``; ``contours``: one ring per box (int (x, y) points in page
        coordinates, [N, 2] or [N, 1, 2]), or None for the handle's resident contour result, read in place.  Returns the records with
        ``boxes`` / ``boxes_rot`` rewritten where the reference takes x_min / x_max (branches 0, 3, 4 of the horizontal splitter), plus
        ``extent`` int32 [lines, 2] and ``contour`` = the region's record of :func:`host_region_line_extents`.  A region without any border
        in its rotated contour has status LINES_NONE and no lines, as the reference's bare except leaves it."""
        if len(records) == 0:
            return []
        return _extent_records(records, *self.region_line_extents_raw(boxes, slopes, records, contours))

    def region_line_extents_read(self, region: int, w: int, h: int, n_points: int):
        """(threshrot uint8 [h, w] of 0 / 255, the winner's points int32 [n_points, 2]) of region ``region`` of the handle's last extent or
        border-winner call."""
        thresh, winner = np.zeros((int(h), int(w)), np.uint8), np.zeros((max(int(n_points), 1), 2), np.int32)
        check(self.lib.sbbseg_region_line_extents_read(self.h, int(region), _ptr(thresh), _ptr(winner), winner.shape[0]), "sbbseg_region_line_extents_read")
        return thresh, winner[:int(n_points)].copy()

    def debug_mask_border_winner(self, masks):
        """The border scan of the extent step alone on raw masks (``sbbseg_debug_mask_border_winner_dev``): per mask the record of
        :func:`host_mask_border_winner`."""
        masks = [np.ascontiguousarray(np.asarray(m) != 0, np.uint8) for m in masks]
        n = len(masks)
        if n == 0:
            return []
        wh = np.ascontiguousarray([[m.shape[1], m.shape[0]] for m in masks], np.int32)
        packed = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in masks]), np.uint8)
        rec = np.zeros((n, EXTENT_REC_INTS), np.int32)
        check(self.lib.sbbseg_debug_mask_border_winner_dev(self.h, _ptr(packed), _ptr(wh), n, _ptr(rec)), "sbbseg_debug_mask_border_winner_dev")
        out = []
        for r in range(n):
            d = _extent_rec(rec[r])
            d["winner"] = self.region_line_extents_read(r, wh[r, 0], wh[r, 1], d["points"])[1]
            out.append(d)
        return out

    def set_extent_lds_limit(self, nbytes: int):
        """Test hook: regions whose three bit maps exceed ``nbytes`` are scanned on a global workspace (default 61440)."""
        check(self.lib.sbbseg_debug_set_extent_lds_limit(self.h, int(nbytes)), "sbbseg_debug_set_extent_lds_limit")

    def extent_launches(self) -> int:
        """Kernels the extent calls have queued on this handle so far."""
        v = C.c_int64(0)
        check(self.lib.sbbseg_debug_extent_launches(self.h, C.byref(v)), "sbbseg_debug_extent_launches")
        return int(v.value)

    def _region_profiles_call(self, fn, src, H, W, boxes, angles_deg, erode_iterations):
        boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        angles_deg = np.ascontiguousarray(angles_deg, np.float64).reshape(-1)
        n, na = boxes.shape[0], angles_deg.shape[0]
        offsets = region_deskew_offsets(boxes, na, H, W)
        if n == 0:
            return []
        counts = np.empty(int(offsets[-1]), np.int32)
        check(fn(self.h, src, int(H), int(W), _ptr(boxes), n, int(erode_iterations), _ptr(angles_deg), na, _ptr(counts), _ptr(offsets)),
              "sbbseg_region_deskew_profiles")
        return [counts[offsets[r]:offsets[r + 1]].reshape(na, -1) for r in range(n)]

    def region_deskew_profiles_dev(self, d_textlines: int, H: int, W: int, boxes, angles_deg, erode_iterations: int = 2):
        """Row profiles of the deskew sweep for every box of a device textline plane, one call: a list of int32 [n_angles][S_r]."""
        return self._region_profiles_call(self.lib.sbbseg_region_deskew_profiles_dev, C.c_void_p(d_textlines), H, W, boxes, angles_deg, erode_iterations)

    def region_deskew_profiles(self, textlines: np.ndarray, boxes, angles_deg, erode_iterations: int = 2):
        """The same from a host textline map uint8 [H, W] (uploaded once per call): per box, bit for bit
        ``deskew_profiles(cv2.erode(crop, 5x5, iterations), angles)``."""
        plane = np.ascontiguousarray(textlines, np.uint8)
        if plane.ndim != 2:
            raise ValueError("region_deskew_profiles expects a uint8 plane [H, W]")
        return self._region_profiles_call(self.lib.sbbseg_region_deskew_profiles, _ptr(plane), plane.shape[0], plane.shape[1], boxes, angles_deg,
                                          erode_iterations)

    def profile_statistics_dev(self, d_counts: int, offsets, n_angles: int, weights=None, multiplier: float = 20.3):
        """The 1-D statistic of the deskew search for every (region, angle) profile of a sweep whose packed int32 counts are in device memory,
        and the winner per region: (spread float64 [n_regions, n_angles], state uint8 [n_regions, n_angles], winner int32 [n_regions]) --
        see sbbseg.h.  ``weights``: ``gaussian_weights(sigma)``; None = the library's table for sigma = 2."""
        offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        n = offsets.shape[0] - 1
        w = None if weights is None else np.ascontiguousarray(weights, np.float64).reshape(-1)
        spread, state, winner = np.zeros((n, n_angles), np.float64), np.zeros((n, n_angles), np.uint8), np.zeros(n, np.int32)
        check(self.lib.sbbseg_profile_statistics_dev(self.h, C.c_void_p(d_counts), _ptr(offsets), n, int(n_angles), _ptr(w), 0 if w is None else w.shape[0] - 1,
                                                     float(multiplier), _ptr(spread), _ptr(state), _ptr(winner)), "sbbseg_profile_statistics_dev")
        return spread, state, winner

    def _slopes_call(self, fn, src, H, W, boxes, erode_iterations, weights, box_plane=None):
        """``box_plane`` given: the pooled form, ``src`` = the Plane array, ``H`` = its length (``W`` unused)."""
        boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        w = None if weights is None else np.ascontiguousarray(weights, np.float64).reshape(-1)
        slopes = np.zeros(boxes.shape[0], np.float64)
        front = (src, int(H), int(W), _ptr(boxes)) if box_plane is None else (src, int(H), _ptr(boxes), _ptr(box_plane))
        check(fn(self.h, *front, boxes.shape[0], int(erode_iterations), _ptr(w), 0 if w is None else w.shape[0] - 1, _ptr(slopes)),
              "sbbseg_region_deskew_slopes")
        return [float(v) for v in slopes]

    def region_deskew_slopes_dev(self, d_textlines: int, H: int, W: int, boxes, erode_iterations: int = 2, weights=None):
        """The slope half of do_work_of_slopes (main.py:1728-1748) for every box of a device textline plane: a list of float.  Sweeps,
        statistic and angle selection run on the device; only the winners are copied back (sbbseg.h)."""
        return self._slopes_call(self.lib.sbbseg_region_deskew_slopes_dev, C.c_void_p(d_textlines), H, W, boxes, erode_iterations, weights)

    def region_deskew_slopes(self, textlines: np.ndarray, boxes, erode_iterations: int = 2, weights=None):
        """The same from a host textline map uint8 [H, W] (uploaded once per call)."""
        plane = np.ascontiguousarray(textlines, np.uint8)
        if plane.ndim != 2:
            raise ValueError("region_deskew_slopes expects a uint8 plane [H, W]")
        return self._slopes_call(self.lib.sbbseg_region_deskew_slopes, _ptr(plane), plane.shape[0], plane.shape[1], boxes, erode_iterations, weights)

    def _line_masks_call(self, fn, src, H, W, boxes, slopes, erode_iterations, masks, box_plane=None):
        boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        slopes = np.ascontiguousarray(slopes, np.float64).reshape(-1)
        n = boxes.shape[0]
        if slopes.shape[0] != n:
            raise ValueError("one slope per box: %d boxes, %d slopes" % (n, slopes.shape[0]))
        if n == 0:
            return []
        w, h = boxes[:, 2].astype(np.int64).clip(0), boxes[:, 3].astype(np.int64).clip(0)
        out_masks = np.empty(int((w * h).sum()), np.uint8) if masks else None
        rows, cols = np.empty(int(h.sum()), np.int32), np.empty(int(w.sum()), np.int32)
        mo, ro, co = (np.zeros(n + 1, np.int64) for _ in range(3))
        front = (src, int(H), int(W), _ptr(boxes)) if box_plane is None else (src, int(H), _ptr(boxes), _ptr(box_plane))
        check(fn(self.h, *front, n, int(erode_iterations), _ptr(slopes), _ptr(out_masks), _ptr(rows), _ptr(cols),
                 _ptr(mo), _ptr(ro), _ptr(co)), "sbbseg_region_line_masks")
        return [(out_masks[mo[r]:mo[r + 1]].reshape(int(h[r]), int(w[r])) if masks else None,
                 rows[ro[r]:ro[r + 1]].astype(np.int64), cols[co[r]:co[r + 1]].astype(np.int64)) for r in range(n)]

    def region_line_masks_dev(self, d_textlines: int, H: int, W: int, boxes, slopes, erode_iterations: int = 2, masks: bool = True):
        """The deskewed text-line mask of every box of a device textline plane (textline_contours_postprocessing up to ``dst``,
        main.py:1472-1487) and its projections, one call: a list of (dst uint8 [h, w] of 0 / 1, or None with ``masks=False``; row sums
        int64 [h]; column sums int64 [w]) -- see sbbseg.h."""
        return self._line_masks_call(self.lib.sbbseg_region_line_masks_dev, C.c_void_p(d_textlines), H, W, boxes, slopes, erode_iterations, masks)

    def region_line_masks(self, textlines: np.ndarray, boxes, slopes, erode_iterations: int = 2, masks: bool = True):
        """The same from a host textline map uint8 [H, W] (uploaded once per call)."""
        plane = np.ascontiguousarray(textlines, np.uint8)
        if plane.ndim != 2:
            raise ValueError("region_line_masks expects a uint8 plane [H, W]")
        return self._line_masks_call(self.lib.sbbseg_region_line_masks, _ptr(plane), plane.shape[0], plane.shape[1], boxes, slopes, erode_iterations, masks)

    def line_split_dev(self, d_profiles: int, offsets, others, verticals, rots, sigma_max: int = LINE_SIGMA_MAX):
        """The text lines of every region from its projection (``seperate_lines`` / ``seperate_lines_vertical`` after ``img_patch.sum``,
        main.py:516-1457) for packed int32 profiles in device memory, one call: a list of line records (``line_split_host``).  The x
        extent of every line is the reference's fallback (0, w); ``region_line_extents_dev`` cuts the lines to the contour (sbbseg.h).  A region whose sigma_gaus exceeds
        the device's table is finished by the host twin with that sigma's weights."""
        offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        n = offsets.shape[0] - 1
        geom = _line_geom(np.diff(offsets), others, verticals)
        rots = np.ascontiguousarray(rots, np.float64).reshape(n, 6)
        w, w_off = line_weight_table(sigma_max)
        out = _line_split_buffers(geom)
        if n:
            check(self.lib.sbbseg_line_split_dev(self.h, C.c_void_p(d_profiles), _ptr(offsets), n, _ptr(geom), _ptr(rots), _ptr(w), _ptr(w_off), int(sigma_max),
                                                 *[_ptr(a) for a in out]), "sbbseg_line_split_dev")
        records = _line_records(*out)
        for r, rec in enumerate(records):
            if rec["status"] == LINES_SIGMA_TOO_LARGE:
                prof = self.download(d_profiles + 4 * int(offsets[r]), (int(geom[r, 0]),), np.int32)
                records[r] = line_split_host([prof], [geom[r, 1]], [geom[r, 2]], [rots[r]], sigma_max)[0]
        return records

    def _line_boxes_call(self, fn, src, d_src, H, W, boxes, slopes, erode_iterations, sigma_max, box_plane=None):
        """``d_src(r)``: (device pointer, H, W) of the plane of box r, for the one-box fallback."""
        boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        slopes = np.ascontiguousarray(slopes, np.float64).reshape(-1)
        n = boxes.shape[0]
        if slopes.shape[0] != n:
            raise ValueError("one slope per box: %d boxes, %d slopes" % (n, slopes.shape[0]))
        if n == 0:
            return []
        vertical = np.abs(slopes) > 45
        geom = _line_geom(np.where(vertical, boxes[:, 2], boxes[:, 3]).clip(1), np.where(vertical, boxes[:, 3], boxes[:, 2]), vertical)
        rots = np.array([line_rotation_terms(int(b[2]), int(b[3]), float(s)) for b, s in zip(boxes, slopes)], np.float64).reshape(n, 6)
        w, w_off = line_weight_table(sigma_max)
        out = _line_split_buffers(geom)
        front = (src, int(H), int(W), _ptr(boxes)) if box_plane is None else (src, int(H), _ptr(boxes), _ptr(box_plane))
        check(fn(self.h, *front, n, int(erode_iterations), _ptr(slopes), _ptr(rots), _ptr(w), _ptr(w_off), int(sigma_max),
                 *[_ptr(a) for a in out]), "sbbseg_region_line_boxes")
        records = _line_records(*out)
        for r, rec in enumerate(records):
            if rec["status"] == LINES_SIGMA_TOO_LARGE:          # the profile of this one box, then the host twin with its sigma's weights
                _m, rows, cols = self.region_line_masks_dev(*d_src(r), [boxes[r]], [slopes[r]], erode_iterations, False)[0]
                records[r] = line_split_host([cols if vertical[r] else rows], [geom[r, 1]], [geom[r, 2]], [rots[r]], sigma_max)[0]
        return records

    def region_line_boxes_dev(self, d_textlines: int, H: int, W: int, boxes, slopes, erode_iterations: int = 2, sigma_max: int = LINE_SIGMA_MAX):
        """``region_line_masks_dev`` and then the line splitter of every box on its own profile (row sums, or column sums for
        ``abs(slope) > 45``, main.py:1514), the profiles staying on the device: a list of line records (``line_split_host``) -- see
        sbbseg.h.  The x extent of every line is the reference's fallback (0, w); ``region_line_extents_dev`` cuts the lines to the contour."""
        return self._line_boxes_call(self.lib.sbbseg_region_line_boxes_dev, C.c_void_p(d_textlines), lambda r: (d_textlines, H, W), H, W, boxes, slopes,
                                     erode_iterations, sigma_max)

    def region_line_boxes(self, textlines: np.ndarray, boxes, slopes, erode_iterations: int = 2, sigma_max: int = LINE_SIGMA_MAX):
        """The same from a host textline map uint8 [H, W] (uploaded once per call)."""
        plane = np.ascontiguousarray(textlines, np.uint8)
        if plane.ndim != 2:
            raise ValueError("region_line_boxes expects a uint8 plane [H, W]")
        return self._line_boxes_call(self.lib.sbbseg_region_line_boxes, _ptr(plane), lambda r: (self.stage(plane), plane.shape[0], plane.shape[1]),
                                     plane.shape[0], plane.shape[1], boxes, slopes, erode_iterations, sigma_max)

    # -- the per-box calls for boxes on many planes (the resident textline planes of many pages: run_pages_planes) -------------
    def planes_deskew_slopes_dev(self, planes, boxes_per_plane, erode_iterations: int = 2, weights=None):
        """``region_deskew_slopes_dev`` for the boxes of MANY device planes in one call (``sbbseg_planes_deskew_slopes_dev``): ``planes`` =
        [(device pointer, H, W)], ``boxes_per_plane`` = one box list per plane.  Returns one list of float per plane; every slope is bit
        for bit what the one-plane call gives for that box on that plane, and the launches do not grow with the planes."""
        arr, n_planes, boxes, box_plane, counts = _pool_planes(planes, boxes_per_plane)
        out = self._slopes_call(self.lib.sbbseg_planes_deskew_slopes_dev, arr, n_planes, 0, boxes, erode_iterations, weights, box_plane)
        return _unpool(out, counts)

    def planes_line_masks_dev(self, planes, boxes_per_plane, slopes_per_plane, erode_iterations: int = 2, masks: bool = True):
        """``region_line_masks_dev`` for the boxes of many device planes in one call (``sbbseg_planes_line_masks_dev``): one list of
        (dst or None, row sums, column sums) per plane."""
        arr, n_planes, boxes, box_plane, counts = _pool_planes(planes, boxes_per_plane, slopes_per_plane)
        slopes = [float(v) for sl in slopes_per_plane for v in sl]
        return _unpool(self._line_masks_call(self.lib.sbbseg_planes_line_masks_dev, arr, n_planes, 0, boxes, slopes, erode_iterations, masks, box_plane), counts)

    def planes_line_boxes_dev(self, planes, boxes_per_plane, slopes_per_plane, erode_iterations: int = 2, sigma_max: int = LINE_SIGMA_MAX):
        """``region_line_boxes_dev`` for the boxes of many device planes in one call (``sbbseg_planes_line_boxes_dev``): one list of line
        records per plane.  A box whose sigma exceeds the device's table is finished by the host twin from a one-box call on its plane."""
        arr, n_planes, boxes, box_plane, counts = _pool_planes(planes, boxes_per_plane, slopes_per_plane)
        slopes = [float(v) for sl in slopes_per_plane for v in sl]
        planes = [(int(d or 0), int(H), int(W)) for d, H, W in planes]
        return _unpool(self._line_boxes_call(self.lib.sbbseg_planes_line_boxes_dev, arr, lambda r: planes[int(box_plane[r])], n_planes, 0, boxes, slopes,
                                             erode_iterations, sigma_max, box_plane), counts)

    def slope_sweep_launches(self) -> int:
        """Kernels the deskew slope sweeps have queued on this handle so far (sbbseg_debug_counter 5)."""
        return self.debug_counter(5)

    def line_mask_launches(self) -> int:
        """Kernels the line-mask and line-split calls have queued on this handle so far (sbbseg_debug_counter 2)."""
        v = C.c_int64(0)
        check(self.lib.sbbseg_debug_counter(self.h, 2, C.byref(v)), "sbbseg_debug_counter")
        return int(v.value)

    def page_box_dev(self, d_mask: int, H: int, W: int):
        """((x, y, w, h), pixels) of the largest component of the dilated mask (main.py:394-404); pixels == 0: empty mask."""
        box = np.zeros(4, np.int32)
        px = C.c_int64(0)
        check(self.lib.sbbseg_page_box_dev(self.h, C.c_void_p(d_mask), H, W, _ptr(box), C.byref(px)), "sbbseg_page_box_dev")
        return tuple(int(v) for v in box), int(px.value)

    def host_contour_calls(self) -> int:
        v = C.c_int64(0)
        check(self.lib.sbbseg_debug_counter(self.h, 0, C.byref(v)), "sbbseg_debug_counter")
        return int(v.value)

    def extract_page_box(self, page: np.ndarray, scaled_h: int, scaled_w: int, channels: int = 1, want_mask: bool = True):
        """Border model on the page as upscaled to scaled_h x scaled_w + the page box, one call: (mask, (x, y, w, h), pixels).
        want_mask=False: the mask (a local of the reference's extract_page) stays on the device; returns (None, box, pixels)."""
        page = np.ascontiguousarray(page, np.uint8)
        mask = self._label_out(scaled_h, scaled_w, channels) if want_mask else None
        box = np.zeros(4, np.int32)
        px = C.c_int64(0)
        check(self.lib.sbbseg_extract_page_box(self.h, _ptr(page), page.shape[0], page.shape[1], scaled_h, scaled_w,
                                               _ptr(mask) if want_mask else None, _ptr(box), C.byref(px)), "sbbseg_extract_page_box")
        return mask, tuple(int(v) for v in box), int(px.value)

    def extract_page_box_dev(self, d_page: int, Hp: int, Wp: int, scaled_h: int, scaled_w: int, d_mask: int = 0):
        """The same on a page that is already on the device (pointer); d_mask = device buffer of scaled_h x scaled_w labels or 0.
        Returns ((x, y, w, h), pixels)."""
        box = np.zeros(4, np.int32)
        px = C.c_int64(0)
        check(self.lib.sbbseg_extract_page_box_dev(self.h, C.c_void_p(d_page), Hp, Wp, scaled_h, scaled_w, C.c_void_p(d_mask) if d_mask else None,
                                                   _ptr(box), C.byref(px)), "sbbseg_extract_page_box_dev")
        return tuple(int(v) for v in box), int(px.value)

    def segment_pages(self, pages, channels: int = 1):
        """do_prediction(patches=True) for a list of HOST pages of one size, upload / compute / download pipelined:
        list of uint8 label maps ([Hp][Wp], or [Hp][Wp][3] with channels=3)."""
        pages = [np.ascontiguousarray(p_, np.uint8) for p_ in pages]
        Hp, Wp = pages[0].shape[:2]
        if any(p_.shape != (Hp, Wp, 3) for p_ in pages):
            raise ValueError("segment_pages: all pages must be uint8 [Hp][Wp][3] of one size")
        outs = [self._label_out(Hp, Wp, channels) for _ in pages]
        n = len(pages)
        pin = (C.c_void_p * n)(*[p_.ctypes.data for p_ in pages])
        pout = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        check(self.lib.sbbseg_segment_pages(self.h, n, pin, Hp, Wp, pout), "sbbseg_segment_pages")
        return outs

    def deskew_profiles(self, mask: np.ndarray, angles_deg=None, matrices=None) -> np.ndarray:
        """Rotate-and-project of the deskew search: int32 [n_angles][side] row counts of the rotated, binarised region mask."""
        mask = np.ascontiguousarray(mask, np.uint8)
        H, W = mask.shape
        side = deskew_side(H, W)
        if matrices is not None:
            matrices = np.ascontiguousarray(matrices, np.float64).reshape(-1, 6)
            n = matrices.shape[0]
        else:
            angles_deg = np.ascontiguousarray(angles_deg, np.float64).reshape(-1)
            n = angles_deg.shape[0]
        counts = np.zeros((n, side), np.int32)
        check(self.lib.sbbseg_deskew_profiles(self.h, _ptr(mask), H, W, _ptr(matrices) if matrices is not None else None,
                                              _ptr(angles_deg) if matrices is None else None, n, _ptr(counts)), "sbbseg_deskew_profiles")
        return counts

    def set_conv_variant(self, variant: int):
        check(self.lib.sbbseg_debug_set_conv_variant(self.h, int(variant)))

    # -- profiling -----------------------------------------------------------------------------
    def profile_enable(self, on: bool):
        check(self.lib.sbbseg_profile_enable(self.h, int(on)))

    def profile_reset(self):
        check(self.lib.sbbseg_profile_reset(self.h))

    def profile(self):
        out = []
        for i, op in enumerate(self.ops()):
            ms, ln, pt = C.c_double(), C.c_int64(), C.c_int64()
            check(self.lib.sbbseg_profile_get(self.h, i, C.byref(ms), C.byref(ln), C.byref(pt)))
            ex, tex = C.c_double(), C.c_double()
            check(self.lib.sbbseg_op_executed(self.h, i, C.byref(ex), C.byref(tex)))
            # exec_patches: whole-patch equivalents of the work launched since profile_reset (owned-region launches count the share of
            # the output grid they walk); timed_exec_patches: the same over the launches total_ms covers
            op.update(total_ms=ms.value, launches=ln.value, patches=pt.value, exec_patches=ex.value, timed_exec_patches=tex.value)
            out.append(op)
        return out


def host_largest_contour(mask: np.ndarray):
    """((x, y, w, h), pixels) by the library's exact HOST ranking (contour tracing) on an already dilated u8 mask; no GPU."""
    mask = np.ascontiguousarray(mask, np.uint8)
    box = np.zeros(4, np.int32)
    px = C.c_int64(0)
    check(load_library().sbbseg_debug_largest_contour(_ptr(mask), mask.shape[0], mask.shape[1], _ptr(box), C.byref(px)), "sbbseg_debug_largest_contour")
    return tuple(int(v) for v in box), int(px.value)


def contours_from_tables(boxes, area2, point_off, points):
    """(boxes, contours) of the contour calls from the library's tables: [[x, y, w, h], ...] and one int32 [N, 2] array per contour."""
    return ([[int(v) for v in b] for b in boxes], [points[int(point_off[k]):int(point_off[k + 1])].copy() for k in range(len(boxes))])


def mask_contours_host_tables(mask: np.ndarray):
    """The library's HOST tracer (no GPU) on a raw u8 mask (!= 0): the contour of every 8-connected component, by descending first pixel,
    as the tables of :meth:`Context.contour_tables`."""
    mask = np.ascontiguousarray(mask, np.uint8)
    lib = load_library()
    n, npts = C.c_int(0), C.c_int64(0)
    check(lib.sbbseg_mask_contours_host(_ptr(mask), mask.shape[0], mask.shape[1], None, None, None, 0, None, 0, C.byref(n), C.byref(npts)),
          "sbbseg_mask_contours_host")
    boxes, area2 = np.zeros((n.value, 4), np.int32), np.zeros(n.value, np.int64)
    off, pts = np.zeros(n.value + 1, np.int64), np.zeros((max(npts.value, 1), 2), np.int32)
    check(lib.sbbseg_mask_contours_host(_ptr(mask), mask.shape[0], mask.shape[1], _ptr(boxes), _ptr(area2), _ptr(off), n.value, _ptr(pts), npts.value,
                                        C.byref(n), C.byref(npts)), "sbbseg_mask_contours_host")
    return boxes, area2, off, pts[:npts.value]


def mask_contours_host(mask: np.ndarray):
    """``(boxes, contours)`` of :func:`mask_contours_host_tables`."""
    return contours_from_tables(*mask_contours_host_tables(mask))


def set_contour_host_step_bound(steps: int):
    """Test hook (process-global): the host tracer gives up after ``steps`` steps per contour; 0 restores 8 x box pixels + 8."""
    check(load_library().sbbseg_debug_set_contour_host_step_bound(int(steps)), "sbbseg_debug_set_contour_host_step_bound")


def _pool_planes(planes, boxes_per_plane, slopes_per_plane=None):
    """(Plane array, number of planes, boxes int32 [n, 4], box_plane int32 [n], boxes per plane) of the pooled per-box calls; boxes in plane order."""
    planes, boxes_per_plane = list(planes), [np.asarray(b, np.int64).reshape(-1, 4) for b in boxes_per_plane]
    if len(boxes_per_plane) != len(planes):
        raise ValueError("one box list per plane: %d planes, %d lists" % (len(planes), len(boxes_per_plane)))
    counts = [b.shape[0] for b in boxes_per_plane]
    if slopes_per_plane is not None and [len(sl) for sl in slopes_per_plane] != counts:
        raise ValueError("one slope per box on every plane")
    arr = (Plane * max(len(planes), 1))()
    for k, (d, H, W) in enumerate(planes):
        arr[k].d_hw, arr[k].H, arr[k].W = int(d) if d else None, int(H), int(W)
    boxes = np.ascontiguousarray(np.concatenate(boxes_per_plane) if planes else np.zeros((0, 4)), np.int32).reshape(-1, 4)
    box_plane = np.ascontiguousarray(np.repeat(np.arange(len(planes)), np.asarray(counts, np.int64)), np.int32)
    return arr, len(planes), boxes, box_plane, counts


def _unpool(flat, counts):
    out, at = [], 0
    for n in counts:
        out.append(list(flat[at:at + n]))
        at += n
    return out


def group_pages_for_lines(boxes_per_page, n_angles: int = 80, max_area: int = (1 << 31) - 1, max_counts: int = (1 << 31) - 1):
    """Greedy grouping of consecutive pages so that every pooled per-box call stays under the library's limits ("too much work for one
    call ... split the boxes"): the sum of the box areas of a group stays <= ``max_area`` and the sum of ``n_angles * S`` (S = the deskew
    square's side, int(1.4 * max(h, w)); 80 angles in the first sweep, the larger one) stays <= ``max_counts``.  Returns a list of lists
    of page indices, in order, every page in exactly one group and no group empty; a single page beyond a limit gets a group of its own
    (the library then says so).  Pure Python."""
    groups, area, counts = [], 0, 0
    for k, boxes in enumerate(boxes_per_page):
        a = sum(int(b[2]) * int(b[3]) for b in boxes)
        c = sum(int(n_angles) * int(max(int(b[2]), int(b[3])) * 1.4) for b in boxes)
        if groups and area + a <= max_area and counts + c <= max_counts:
            groups[-1].append(k)
            area, counts = area + a, counts + c
        else:
            groups.append([k])
            area, counts = a, c
    return groups


def run_pages_planes(layout: "Context"):
    """What the last :func:`run_pages` with ``layout`` as its layout handle left on the device (``sbbseg_run_pages_planes``): two lists, one
    entry per page, of (device pointer, h, w) -- the cleaned layout plane and the textline plane of the page box; the pointer is 0 where
    that page has none.  Valid until the next run_page / run_pages on those handles.  Raises after a failed or absent run_pages."""
    n = getattr(layout, "_run_pages_n", None) or 1
    regions, textlines = (Plane * n)(), (Plane * n)()
    check(layout.lib.sbbseg_run_pages_planes(layout.h, n, regions, textlines), "sbbseg_run_pages_planes")
    return ([(int(p.d_hw or 0), int(p.H), int(p.W)) for p in regions], [(int(p.d_hw or 0), int(p.H), int(p.W)) for p in textlines])


def run_page(border: "Context", layout: "Context", textline: "Context", page: np.ndarray, scaled_h: int, scaled_w: int,
             channels: int = 3, want_mask: bool = True):
    """The model-running part of run() (main.py:2056-2107) in one library call (``sbbseg_run_page``): the page is uploaded once and
    stays on the device for the border, layout and textline stages.  Returns (page mask or None, regions or None, textlines or None,
    RunInfo); regions / textlines are cut to the page box (h x w [x channels]).  An empty border mask raises like main.py:401."""
    page = np.ascontiguousarray(page, np.uint8)
    pix = scaled_h * scaled_w
    mask = np.empty((scaled_h, scaled_w, 3) if channels == 3 else (scaled_h, scaled_w), np.uint8) if want_mask else None
    regions = np.empty(pix * channels, np.uint8)
    lines = np.empty(pix, np.uint8)
    info = RunInfo()
    rc = border.lib.sbbseg_run_page(border.h, layout.h, textline.h, _ptr(page), page.shape[0], page.shape[1], scaled_h, scaled_w, channels,
                                    _ptr(mask), _ptr(regions), _ptr(lines), C.byref(info))
    if rc != 0:
        msg = (border.lib.sbbseg_last_error() or b"").decode("utf-8", "replace")
        if "empty sequence" in msg:
            raise ValueError("attempt to get argmax of an empty sequence")          # what main.py:401 raises
        raise RuntimeError("sbbseg_run_page: " + msg)
    w, h = int(info.box_xywh[2]), int(info.box_xywh[3])
    r = regions[:h * w * channels].reshape((h, w, 3) if channels == 3 else (h, w)).copy() if info.regions_ok else None
    t = lines[:h * w].reshape(h, w).copy() if info.textlines_ok else None
    return mask, r, t, info


def run_pages(border: "Context", layout: "Context", textline: "Context", pages, channels: int = 3, want_mask: bool = True):
    """:func:`run_page` for many pages in one resident, pooled library call (``sbbseg_run_pages``).  ``pages``: a sequence of
    (stored page uint8 [H, W, 3], scaled_h, scaled_w).  Returns one (page mask or None, regions or None, textlines or None, RunInfo,
    status) per page; status 1 = the border model found no page there (what makes :func:`run_page` raise): its arrays are None."""
    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    n = len(pages)
    io = (RunPageIO * max(n, 1))()
    keep = []
    for k, (page, scaled_h, scaled_w) in enumerate(pages):
        page = np.ascontiguousarray(page, np.uint8)
        if page.ndim != 3 or page.shape[2] != 3:
            raise ValueError(f"page {k}: must be uint8 [H,W,3], got {page.shape}")
        scaled_h, scaled_w = int(scaled_h), int(scaled_w)
        pix = scaled_h * scaled_w
        mask = np.empty((scaled_h, scaled_w, 3) if channels == 3 else (scaled_h, scaled_w), np.uint8) if want_mask else None
        regions = np.empty(pix * channels, np.uint8)
        lines = np.empty(pix, np.uint8)
        keep.append((page, mask, regions, lines))
        io[k].page, io[k].Hp, io[k].Wp, io[k].Hs, io[k].Ws = page.ctypes.data, page.shape[0], page.shape[1], scaled_h, scaled_w
        io[k].page_mask_out = mask.ctypes.data if want_mask else None
        io[k].regions_out, io[k].textlines_out = regions.ctypes.data, lines.ctypes.data
    layout._run_pages_n = None
    check(border.lib.sbbseg_run_pages(border.h, layout.h, textline.h, n, io, channels), "sbbseg_run_pages")
    layout._run_pages_n = n                                     # (run_pages_planes asks for as many)
    out = []
    for k, (_, mask, regions, lines) in enumerate(keep):
        info = RunInfo.from_buffer_copy(io[k].info)
        if io[k].status != 0:
            out.append((None, None, None, info, int(io[k].status)))
            continue
        w, h = int(info.box_xywh[2]), int(info.box_xywh[3])
        r = regions[:h * w * channels].reshape((h, w, 3) if channels == 3 else (h, w)).copy() if info.regions_ok else None
        t = lines[:h * w].reshape(h, w).copy() if info.textlines_ok else None
        out.append((mask, r, t, info, 0))
    return out


def owned_range(extent: int, tile: int, margin: int, n_tiles: int, t: int):
    """[lo, hi) in tile coordinates of what the page stitch keeps of tile t of an axis (closed form of the owned-region launches; no GPU)."""
    lib = load_library()
    lo, hi = C.c_int(0), C.c_int(0)
    check(lib.sbbseg_debug_owned_range(int(extent), int(tile), int(margin), int(n_tiles), int(t), C.byref(lo), C.byref(hi)), "sbbseg_debug_owned_range")
    return int(lo.value), int(hi.value)


def region_rows(extent: int, tile: int, margin: int, n_tiles: int, t: int, level_sizes):
    """Rows [lo, hi) every decoder level must produce for tile t of an axis: one pair per level, level 0 = the network output (no GPU)."""
    lib = load_library()
    sizes = np.ascontiguousarray(level_sizes, dtype=np.int32)
    out = np.zeros((len(sizes), 2), dtype=np.int32)
    check(lib.sbbseg_debug_region_rows(int(extent), int(tile), int(margin), int(n_tiles), int(t), len(sizes), _ptr(sizes), _ptr(out)),
          "sbbseg_debug_region_rows")
    return out


def host_axis_owner(extent: int, tile: int, margin: int, n_tiles: int) -> np.ndarray:
    """int32 [extent]: (tile << 16) | offset inside it of the tile that owns each coordinate of an axis -- the closed form the stitch of
    segment_views evaluates per pixel; no GPU."""
    own = np.zeros(int(extent), np.int32)
    check(load_library().sbbseg_debug_axis_owner(int(extent), int(tile), int(margin), int(n_tiles), _ptr(own)), "sbbseg_debug_axis_owner")
    return own


def host_largest_contour_area2(mask: np.ndarray) -> int:
    """TWICE the largest outer-contour area (cv2.contourArea) of a u8 mask by the library's HOST tracer; no GPU."""
    mask = np.ascontiguousarray(mask, np.uint8)
    a2 = C.c_int64(0)
    check(load_library().sbbseg_debug_largest_contour_area2(_ptr(mask), mask.shape[0], mask.shape[1], C.byref(a2)), "sbbseg_debug_largest_contour_area2")
    return int(a2.value)


def comm_unique_id() -> bytes:
    """128 opaque bytes naming a new RCCL communicator (rank 0 calls this and ships them to every rank)."""
    buf = C.create_string_buffer(128)
    check(load_library().sbbseg_comm_unique_id(buf), "sbbseg_comm_unique_id")
    return buf.raw


def tile_grid(Hp: int, Wp: int, H: int, W: int):
    """(tile_xy int32 [n,2], nxf, nyf) from the library's restatement of main.py:246-281."""
    lib = load_library()
    nx, ny = C.c_int(), C.c_int()
    check(lib.sbbseg_tile_grid(Hp, Wp, H, W, None, 0, C.byref(nx), C.byref(ny)), "sbbseg_tile_grid")
    xy = np.empty((nx.value * ny.value, 2), np.int32)
    check(lib.sbbseg_tile_grid(Hp, Wp, H, W, _ptr(xy), xy.shape[0], None, None), "sbbseg_tile_grid")
    return xy, nx.value, ny.value


def deskew_side(H: int, W: int) -> int:
    """Side of the zero square the deskew search centres a region mask on: int(1.4 * max(H, W)) (main.py:1613)."""
    side = C.c_int(0)
    check(load_library().sbbseg_deskew_side(int(H), int(W), C.byref(side)), "sbbseg_deskew_side")
    return int(side.value)


def region_deskew_offsets(boxes, n_angles: int, H: int, W: int) -> np.ndarray:
    """int64 [n_boxes + 1]: where region r's [n_angles][S_r] counts start in the packed buffer of sbbseg_region_deskew_profiles (the
    last entry is the total).  Validates the boxes against the H x W plane; no GPU and no handle needed."""
    boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    offsets = np.zeros(boxes.shape[0] + 1, np.int64)
    check(load_library().sbbseg_region_deskew_profiles_dev(None, None, int(H), int(W), _ptr(boxes), boxes.shape[0], 0, None, int(n_angles), None,
                                                           _ptr(offsets)), "sbbseg_region_deskew_profiles")
    return offsets


def gaussian_weights(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """The half kernel weights[0 .. radius] of ``scipy.ndimage.gaussian_filter1d(., sigma)``, computed exactly as scipy's
    ``_gaussian_kernel1d`` does (numpy's exp, divided by its numpy sum): what the library's profile statistic takes from its caller."""
    sd = float(sigma)
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:], np.float64)


def profile_statistics_host(counts, offsets, n_angles: int, weights=None, multiplier: float = 20.3, want_smooth: bool = False):
    """``Context.profile_statistics_dev`` on the CPU (serial, no handle, no GPU): the same bits.  ``counts``: packed int32 host array.
    With ``want_smooth`` a fourth value: the smoothed profiles, packed like ``counts``."""
    counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
    offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
    n = offsets.shape[0] - 1
    w = None if weights is None else np.ascontiguousarray(weights, np.float64).reshape(-1)
    spread, state, winner = np.zeros((n, n_angles), np.float64), np.zeros((n, n_angles), np.uint8), np.zeros(n, np.int32)
    smooth = np.zeros(counts.shape[0], np.float64) if want_smooth else None
    check(load_library().sbbseg_profile_statistics_host(_ptr(counts), _ptr(offsets), n, int(n_angles), _ptr(w), 0 if w is None else w.shape[0] - 1,
                                                        float(multiplier), _ptr(spread), _ptr(state), _ptr(winner), _ptr(smooth)),
          "sbbseg_profile_statistics_host")
    return (spread, state, winner, smooth) if want_smooth else (spread, state, winner)


def debug_profile_statistics(ctx, counts, offsets, n_angles: int, weights=None, multiplier: float = 20.3):
    """(spread, state, winner, smooth, below) of sbbseg_debug_profile_statistics from packed int32 HOST counts: ``ctx`` None = the serial host
    twin, a ``Context`` = the product's kernels.  ``smooth``: z packed like ``counts``; ``below`` float64 [n_regions, n_angles]."""
    counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
    offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
    n = offsets.shape[0] - 1
    w = None if weights is None else np.ascontiguousarray(weights, np.float64).reshape(-1)
    spread, state, winner = np.zeros((n, n_angles), np.float64), np.zeros((n, n_angles), np.uint8), np.zeros(n, np.int32)
    smooth, below = np.zeros(counts.shape[0], np.float64), np.zeros((n, n_angles), np.float64)
    check(load_library().sbbseg_debug_profile_statistics(None if ctx is None else ctx.h, _ptr(counts), _ptr(offsets), n, int(n_angles), _ptr(w),
                                                         0 if w is None else w.shape[0] - 1, float(multiplier), _ptr(spread), _ptr(state), _ptr(winner),
                                                         _ptr(smooth), _ptr(below)), "sbbseg_debug_profile_statistics")
    return spread, state, winner, smooth, below


def debug_soft_arith(ctx, op: int, a, b=None) -> np.ndarray:
    """csrc/profile_stat.h's soft_div(a, b) (``op`` 0) or soft_sqrt(a) (``op`` 1) element by element: ``ctx`` None = on the host, a ``Context`` =
    one kernel.  float64 in, float64 out (compare bit patterns)."""
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    b = None if b is None else np.ascontiguousarray(b, np.float64).reshape(-1)
    if op == 0 and (b is None or b.shape != a.shape):
        raise ValueError("debug_soft_arith: the divide takes two arrays of one length")
    out = np.zeros(a.shape[0], np.float64)
    check(load_library().sbbseg_debug_soft_arith(None if ctx is None else ctx.h, int(op), _ptr(a), _ptr(b), a.shape[0], _ptr(out)),
          "sbbseg_debug_soft_arith")
    return out


_LINE_TABLES = {}


def line_weight_table(sigma_max: int = LINE_SIGMA_MAX):
    """(weights float64, offsets int64 [sigma_max]): ``gaussian_weights(sigma)`` for sigma = 2 .. sigma_max one after the other (4 sigma +
    1 values each, from offsets[sigma - 2]): what the line splitter takes from its caller.  Built once per sigma_max."""
    sigma_max = int(sigma_max)
    if sigma_max not in _LINE_TABLES:
        halves = [gaussian_weights(s) for s in range(2, sigma_max + 1)]
        offsets = np.concatenate([[0], np.cumsum([h.shape[0] for h in halves])]).astype(np.int64)
        _LINE_TABLES[sigma_max] = (np.ascontiguousarray(np.concatenate(halves), np.float64), offsets)
    return _LINE_TABLES[sigma_max]

ORDER_SIGMA = 8                                                  # order_of_regions' sigma_gaus (main.py:1814; csrc/order.h)


def order_weights() -> np.ndarray:
    """The 33 doubles the reading-order calls take from their caller: the sigma 8 slice of :func:`line_weight_table`."""
    w, off = line_weight_table()
    return np.ascontiguousarray(w[int(off[ORDER_SIGMA - 2]):int(off[ORDER_SIGMA - 1])])


def pack_contours(contours):
    """(points int32 [total, 2], point_off int64 [n + 1], n) of a list of int (x, y) point arrays ([N, 2], or [N, 1, 2] rings)."""
    arrays = [np.asarray(c).reshape(-1, 2) for c in contours]
    for a in arrays:
        if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
            raise ValueError("contour coordinates must fit 32 bits")
    off = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrays])]).astype(np.int64)
    pts = np.ascontiguousarray(np.concatenate(arrays) if arrays else np.zeros((0, 2)), np.int32).reshape(-1, 2)
    if pts.shape[0] == 0:
        pts = np.zeros((1, 2), np.int32)                         # (a pointer to pass; no point of it is read)
    return pts, off, len(arrays)


def _region_order_buffers(H: int, n: int):
    return (np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 2), np.float64),
            np.zeros((int(H) + 80) // 2 + 2, np.int32))


def _region_order_record(out, n_edges: int):
    sorted_index, order, band, centroids, edges = out
    return dict(sorted_index=sorted_index, order=order, band=band, centroids=centroids, edges=edges[:n_edges].copy())


def host_region_order(textline_mask: np.ndarray, contours):
    """``Context.region_order_dev`` on the CPU (serial, no handle, no GPU): the same bits.  A record: ``edges`` int32 (the band edges, [0] +
    peaks_neg + [H], unclamped), ``centroids`` float64 [n, 2] (cx, cy), ``band`` int32 [n] (-1: in no band), ``sorted_index`` int32 [n]
    (the regions by band, cx, index; those of band -1 last) and ``order`` int32 [n] (position in that list; -1 for band -1)."""
    mask = np.asarray(textline_mask)
    sums = np.ascontiguousarray(mask.sum(axis=1, dtype=np.int64), np.int32)
    pts, off, n = pack_contours(contours)
    out = _region_order_buffers(mask.shape[0], n)
    ne = C.c_int(0)
    check(load_library().sbbseg_region_order_host(_ptr(sums), mask.shape[0], _ptr(order_weights()), _ptr(pts), _ptr(off), n, *[_ptr(a) for a in out],
                                                  out[-1].shape[0], C.byref(ne)), "sbbseg_region_order_host")
    return _region_order_record(out, ne.value)


def host_contour_moments(contours):
    """``Context.contour_moments_dev`` on the CPU (the literal serial float64 loop): (moments [n, 3], centroids [n, 2], serial [n])."""
    pts, off, n = pack_contours(contours)
    moments, centroids, serial = np.zeros((n, 3), np.float64), np.zeros((n, 2), np.float64), np.zeros(n, np.int32)
    check(load_library().sbbseg_contour_moments_host(_ptr(pts), _ptr(off), n, _ptr(moments), _ptr(centroids), _ptr(serial)),
          "sbbseg_contour_moments_host")
    return moments, centroids, serial


def line_rotation_terms(w: int, h: int, slope: float):
    """[cos, -sin, sin, cos, x_d, y_d] of seperate_lines (main.py:517-524) for a dst of h x w, or of seperate_lines_vertical
    (main.py:996-1005: thetha + 90 first) when ``abs(slope) > 45``: numpy's cos / sin and the library's getRotationMatrix2D."""
    thetha = float(slope) + 90 if abs(float(slope)) > 45 else float(slope)
    M = rotation_matrix(w // 2, h // 2, -thetha)
    t = thetha / 180. * np.pi
    return [float(np.cos(t)), float(-np.sin(t)), float(np.sin(t)), float(np.cos(t)), float(M[0, 2]), float(M[1, 2])]


def _line_geom(lengths, others, verticals) -> np.ndarray:
    return np.ascontiguousarray(np.stack([np.asarray(lengths, np.int64), np.asarray(others, np.int64), np.asarray(verticals, np.int64)], axis=1)
                                if len(lengths) else np.zeros((0, 3)), np.int32)


def _line_split_buffers(geom: np.ndarray):
    """(info, line_off, lines, corners, corners_rot) sized by the capacities sbbseg.h documents."""
    total = int(((geom[:, 0].astype(np.int64) + 40) // 2).sum())
    return (np.zeros((geom.shape[0], 5), np.int32), np.zeros(geom.shape[0] + 1, np.int64), np.zeros((total, 3), np.int32),
            np.zeros((total, 4, 2), np.int32), np.zeros((total, 4, 2), np.int32))


def _line_records(info, line_off, lines, corners, corners_rot):
    out = []
    for r in range(info.shape[0]):
        at, n = int(line_off[r]), int(info[r, 4])
        out.append({"status": int(info[r, 0]), "sigma": int(info[r, 1]), "raised": bool(info[r, 2]), "branch": int(info[r, 3]),
                    "peaks": lines[at:at + n, 0].copy(), "point_up": lines[at:at + n, 1].copy(), "point_down": lines[at:at + n, 2].copy(),
                    "boxes": corners[at:at + n].copy(), "boxes_rot": corners_rot[at:at + n].copy()})
    return out


def line_split_host_raw(profiles, others, verticals, rots, sigma_max: int = LINE_SIGMA_MAX, extra_sigma: int = 0):
    """``sbbseg_line_split_host`` as the library packs it: (info int32 [n, 5], line_off int64 [n + 1], lines [total, 3], corners
    [total, 4, 2], corners_rot [total, 4, 2]).  ``extra_sigma``: one further sigma whose weights are computed on the spot."""
    profiles = [np.ascontiguousarray(p, np.int32).reshape(-1) for p in profiles]
    n = len(profiles)
    offsets = np.concatenate([[0], np.cumsum([p.shape[0] for p in profiles])]).astype(np.int64)
    packed = np.ascontiguousarray(np.concatenate(profiles) if n else np.zeros(0), np.int32)
    geom = _line_geom([p.shape[0] for p in profiles], others, verticals)
    rots = np.ascontiguousarray(rots, np.float64).reshape(n, 6)
    w, w_off = line_weight_table(sigma_max)
    extra = gaussian_weights(extra_sigma) if extra_sigma else None
    out = _line_split_buffers(geom)
    check(load_library().sbbseg_line_split_host(_ptr(packed), _ptr(offsets), n, _ptr(geom), _ptr(rots), _ptr(w), _ptr(w_off), int(sigma_max), _ptr(extra),
                                                int(extra_sigma), *[_ptr(a) for a in out]), "sbbseg_line_split_host")
    return out


def line_split_host(profiles, others, verticals, rots, sigma_max: int = LINE_SIGMA_MAX):
    """``Context.line_split_dev`` on the CPU (serial, no handle, no GPU): the same bits.  ``profiles``: one int array per region (row sums
    of dst, or column sums for the vertical splitter); ``others``: the other extent of dst; ``rots``: ``line_rotation_terms``.  Returns
    one record per region: status (LINES_OK, or LINES_NONE where the reference returns []), sigma (sigma_gaus), raised (the first
    estimate's ``try`` raised), branch (0 .. 4: main.py:744, 822, 825, 864, 919; -1 not reached), peaks, point_up, point_down (int32
    [lines]), boxes and boxes_rot (int32 [lines, 4, 2]: main.py:817-820 and 812-815).  The x extent is the reference's fallback (0, w);
    ``host_region_line_extents`` cuts the lines to the contour.  A region whose sigma_gaus is beyond the table is run again with that sigma's weights."""
    raw = line_split_host_raw(profiles, others, verticals, rots, sigma_max)
    records = _line_records(*raw)
    for r, rec in enumerate(records):
        if rec["status"] == LINES_SIGMA_TOO_LARGE:
            one = line_split_host_raw([profiles[r]], [others[r]], [verticals[r]], [np.asarray(rots, np.float64).reshape(-1, 6)[r]], sigma_max, rec["sigma"])
            records[r] = _line_records(*one)[0]
    return records


EXTENT_OK, EXTENT_NONE, EXTENT_REC_INTS = 0, 1, 8


def _extent_rec(rec) -> dict:
    return {"status": int(rec[0]), "borders": int(rec[1]), "points": int(rec[2]), "is_hole": bool(rec[3]), "tie": bool(rec[4]),
            "start": (int(rec[5]), int(rec[6])), "holes": int(rec[7])}


def _extent_tables(boxes, slopes, records, fill: int = 0):
    """Line records back in the packed form of ``sbbseg_region_line_boxes_dev``: (info, line_off, lines, corners, corners_rot); slots
    beyond a record's count hold ``fill``."""
    vertical = np.abs(slopes) > 45
    geom = _line_geom(np.where(vertical, boxes[:, 2], boxes[:, 3]).clip(1), np.where(vertical, boxes[:, 3], boxes[:, 2]), vertical)
    info, line_off, lines, corners, corners_rot = _line_split_buffers(geom)
    line_off[1:] = np.cumsum((geom[:, 0].astype(np.int64) + 40) // 2)
    for a in (lines, corners, corners_rot):
        a[...] = fill
    for r, rec in enumerate(records):
        at, cnt = int(line_off[r]), len(rec["peaks"])
        info[r] = (rec["status"], rec["sigma"], int(rec["raised"]), rec["branch"], cnt)
        lines[at:at + cnt, 0], lines[at:at + cnt, 1], lines[at:at + cnt, 2] = rec["peaks"], rec["point_up"], rec["point_down"]
        corners[at:at + cnt], corners_rot[at:at + cnt] = rec["boxes"], rec["boxes_rot"]
    return info, line_off, lines, corners, corners_rot


def _extent_records(records, line_off, extent, corners, corners_rot, rec):
    out = []
    for r, old in enumerate(records):
        at, cnt = int(line_off[r]), len(old["peaks"])
        new = dict(old, boxes=corners[at:at + cnt].copy(), boxes_rot=corners_rot[at:at + cnt].copy(), extent=extent[at:at + cnt].copy(),
                   contour=_extent_rec(rec[r]))
        if new["contour"]["status"] == EXTENT_NONE:              # np.argmax([]) raised: the bare except returns [] (main.py:1520)
            new.update(status=LINES_NONE, peaks=old["peaks"][:0], point_up=old["point_up"][:0], point_down=old["point_down"][:0],
                       boxes=new["boxes"][:0], boxes_rot=new["boxes_rot"][:0], extent=new["extent"][:0])
        out.append(new)
    return out


def host_region_line_extents(contour, box, slope: float, record, want_masks: bool = False):
    """``Context.region_line_extents_dev`` for ONE region on the CPU (serial, no handle, no GPU; the same statements, csrc/line_extent.h).
    Returns the record with ``boxes`` / ``boxes_rot`` rewritten, ``extent`` int32 [lines, 2] and ``contour`` = {status (EXTENT_OK /
    EXTENT_NONE), borders, points, is_hole, tie, start, holes} of the border that wins np.argmax in the rotated contour image;
    ``want_masks`` adds ``threshrot`` (uint8 [h, w] of 0 / 255) and ``winner`` (int32 [points, 2]) to ``contour``."""
    box = np.ascontiguousarray(box, np.int32).reshape(4)
    ring = np.ascontiguousarray(np.asarray(contour).reshape(-1, 2), np.int32)
    w, h = int(box[2]), int(box[3])
    slopes = np.array([float(slope)], np.float64)
    info, line_off, lines, corners, corners_rot = _extent_tables(box.reshape(1, 4), slopes, [record])
    rot = np.array(line_rotation_terms(w, h, float(slope)), np.float64)
    cnt = len(record["peaks"])
    extent, rec = np.zeros((lines.shape[0], 2), np.int32), np.zeros((1, EXTENT_REC_INTS), np.int32)
    thresh = np.zeros((max(h, 1), max(w, 1)), np.uint8)
    winner = np.zeros((4 * (max(h, 1) * max(w, 1)) + 8, 2), np.int32)
    check(load_library().sbbseg_region_line_extents_host(_ptr(ring), ring.shape[0], _ptr(box), float(slope), _ptr(rot), int(record["branch"]), _ptr(lines),
                                                         cnt if record["status"] == LINES_OK else 0, _ptr(extent), _ptr(corners), _ptr(corners_rot),
                                                         _ptr(rec), _ptr(thresh), _ptr(winner), winner.shape[0]), "sbbseg_region_line_extents_host")
    out = _extent_records([record], line_off, extent, corners, corners_rot, rec)[0]
    if want_masks:
        out["contour"].update(threshrot=thresh, winner=winner[:out["contour"]["points"]].copy())
    return out


def host_mask_border_winner(mask: np.ndarray) -> dict:
    """The serial border scan of the extent step on a raw mask (!= 0): {status, borders, points, is_hole, tie, start, holes, winner}."""
    m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    rec, winner = np.zeros(EXTENT_REC_INTS, np.int32), np.zeros((4 * m.size + 8, 2), np.int32)
    check(load_library().sbbseg_debug_mask_border_winner_host(_ptr(m), m.shape[1], m.shape[0], _ptr(rec), _ptr(winner), winner.shape[0]),
          "sbbseg_debug_mask_border_winner_host")
    d = _extent_rec(rec)
    d["winner"] = winner[:d["points"]].copy()
    return d


def region_line_extent_weights() -> np.ndarray:
    """int64 [32][32][4][4]: the float32 bicubic products of the contour rotation times 2^34, indexed [ay][ax][row][column] (sbbseg.h)."""
    out = np.empty(32 * 32 * 16, np.int64)
    check(load_library().sbbseg_region_line_extent_weights(_ptr(out), out.shape[0]), "sbbseg_region_line_extent_weights")
    return out.reshape(32, 32, 4, 4)


def host_region_line_mask(crop: np.ndarray, slope: float, erode_iterations: int = 2, mask: bool = True):
    """``Context.region_line_masks_dev`` for ONE box on the CPU (no handle, no GPU; the same statements, csrc/line_mask.h): ``crop`` is the
    textline plane cut to the box.  Returns (dst uint8 [h, w] or None, row sums int64 [h], column sums int64 [w])."""
    crop = np.ascontiguousarray(crop, np.uint8)
    if crop.ndim != 2:
        raise ValueError("host_region_line_mask expects a uint8 crop [h, w]")
    h, w = crop.shape
    dst = np.empty((h, w), np.uint8) if mask else None
    rows, cols = np.empty(h, np.int32), np.empty(w, np.int32)
    check(load_library().sbbseg_region_line_masks_host(_ptr(crop), h, w, int(erode_iterations), float(slope), _ptr(dst), _ptr(rows), _ptr(cols)),
          "sbbseg_region_line_masks_host")
    return dst, rows.astype(np.int64), cols.astype(np.int64)


def region_line_table() -> np.ndarray:
    """int16 [32][32][4][4]: the fixed-point bicubic weights of the line-mask rotation, indexed [ay][ax][row][column] (sbbseg.h)."""
    out = np.empty(32 * 32 * 16, np.int16)
    check(load_library().sbbseg_region_line_table(_ptr(out), out.shape[0]), "sbbseg_region_line_table")
    return out.reshape(32, 32, 4, 4)


def deskew_sweep_angles(sweep: int) -> np.ndarray:
    """The library's angles of return_deskew_slope's sweep 0 (80 in [-25, 25]) or 1 (30 in [-90, -50]): np.linspace's values."""
    n = C.c_int(0)
    out = np.zeros(80, np.float64)
    check(load_library().sbbseg_deskew_sweep_angles(int(sweep), _ptr(out), 80, C.byref(n)), "sbbseg_deskew_sweep_angles")
    return out[:n.value].copy()


def rotation_matrix(cx: float, cy: float, angle_deg: float) -> np.ndarray:
    """cv2.getRotationMatrix2D((cx, cy), angle, 1.0) as the library computes it: float64 [2][3]."""
    m = np.zeros(6, np.float64)
    check(load_library().sbbseg_rotation_matrix(float(cx), float(cy), float(angle_deg), _ptr(m)), "sbbseg_rotation_matrix")
    return m.reshape(2, 3)


def nearest_map(src_len: int, dst_len: int) -> np.ndarray:
    """int32 [dst_len]: the library's cv2.INTER_NEAREST index rule (sbbseg_nearest_map)."""
    out = np.empty(dst_len, np.int32)
    check(load_library().sbbseg_nearest_map(int(src_len), int(dst_len), _ptr(out)), "sbbseg_nearest_map")
    return out


def native_plan_summary(sbbw_bytes: bytes, precision: int, flags: int = 0) -> str:
    """Text summary of the plan the library's own planner builds from a .sbbw container (no GPU needed; test hook)."""
    lib = load_library()
    need = C.c_size_t(0)
    check(lib.sbbseg_debug_plan_summary(sbbw_bytes, len(sbbw_bytes), precision, flags, None, 0, C.byref(need)), "sbbseg_debug_plan_summary")
    buf = C.create_string_buffer(need.value)
    check(lib.sbbseg_debug_plan_summary(sbbw_bytes, len(sbbw_bytes), precision, flags, buf, need.value, None), "sbbseg_debug_plan_summary")
    return buf.value.decode()
