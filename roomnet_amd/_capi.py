"""ctypes binding of libroomnet_hip.so (C ABI in include/roomnet_hip.h).

There is deliberately no CPU fallback: if the HIP library is missing or cannot be
loaded, importing the product path fails loudly with ``RoomNetLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .graph import BN_EPSILON, Graph

RN_OK = 0
RN_DTYPE_F32, RN_DTYPE_BF16, RN_DTYPE_F16 = 0, 1, 2
RN_FLAG_TAPS = 1
RN_FLAG_STAGE_LAUNCHES = 2      # 16-bit handles: one launch per conv stage (no cross-stage fusion)
RN_FLAG_GENERIC_KERNELS = 4     # 16-bit handles: generic stage kernel everywhere (diagnostic cross-check)
RN_FLAG_PAIR_32X32 = 8          # 16-bit handles: the fused stage pair on the round-2 32x32x16 kernel (comparison arm)
RN_FLAG_COMPUTE_FROZEN = 16     # convolve the provably constant channels too (comparison arm of the frozen-channel folding)
RN_FLAG_NO_DITHER = 32          # 16-bit handles: plain rounding of weights and stores (comparison arm of the round-6 dither)
RN_FLAG_BATCH_STATS = 64        # float32 handles: every BN normalises with the moments of the batch being fed (training=True forward)
RN_MAX_STAGES = 16
RN_MAX_DENSE = 8
RN_NAME_LEN = 32

DTYPES = {"f32": RN_DTYPE_F32, "fp32": RN_DTYPE_F32, "float32": RN_DTYPE_F32,
          "bf16": RN_DTYPE_BF16, "bfloat16": RN_DTYPE_BF16,
          "f16": RN_DTYPE_F16, "fp16": RN_DTYPE_F16, "float16": RN_DTYPE_F16}

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libroomnet_hip.so")
# the test / A-B library: the product library's objects + the round-2 comparison kernels behind RN_FLAG_PAIR_32X32
AB_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libroomnet_hip_ab.so")

# every symbol include/roomnet_hip.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = (
    "rn_create", "rn_destroy", "rn_last_error", "rn_device_count", "rn_version",
    "rn_forward_u8", "rn_submit_u8", "rn_collect", "rn_forward_f32", "rn_forward_u8_device", "rn_forward_f32_device", "rn_sync",
    "rn_set_stream", "rn_set_stream_null", "rn_node_count", "rn_node_info_get", "rn_tap", "rn_set_profiling", "rn_timing",
    "rn_dominant_stage", "rn_stage_launch", "rn_device_malloc", "rn_device_free", "rn_memcpy_h2d", "rn_memcpy_d2h",
    "rn_crop_resize_u8_device", "rn_crop_resize_batch_u8_device", "rn_classify_images_u8", "rn_host_alloc", "rn_host_free", "rn_frozen_info", "rn_const_info",
    "rn_group_create", "rn_group_destroy", "rn_group_size", "rn_group_handle", "rn_group_forward_u8",
    "rn_group_forward_u8_device", "rn_group_result_buffer", "rn_group_sync", "rn_group_plan",
    "rn_band_plan", "rn_f32m_plan",
    "rn_grad_cam_u8", "rn_grad_cam_f32", "rn_grad_cam_u8_device",
    "rn_bn_count", "rn_bn_info", "rn_bn_batch_stats",
    "rn_features_shape", "rn_features_u8", "rn_features_u8_device",
    "rn_features_depth_shape", "rn_features_depth_u8", "rn_features_depth_u8_device",
    "rn_ft_create", "rn_ft_create_depth", "rn_ft_depth", "rn_ft_destroy", "rn_ft_run", "rn_ft_eval", "rn_ft_var_count", "rn_ft_var_info", "rn_ft_read",
    "rn_ft_step_count", "rn_ft_last_run_ms", "rn_ft_upload", "rn_ft_free",
    "rn_ft_set_dropout", "rn_ft_dropout", "rn_ft_dropout_mask",
    "rn_ft_val_points", "rn_ft_run_validated", "rn_ft_best",
    "rn_view_draw", "rn_views_create", "rn_views_destroy", "rn_views_batch_device", "rn_ft_run_views",
    "rn_jpeg_probe", "rn_jpeg_coeff_count", "rn_jpeg_entropy_decode", "rn_jpeg_decode_batch_device", "rn_classify_jpegs",
    "rn_jpeg_last_decode_ms",
    "rn_jpeg_scan_probe", "rn_jpeg_huffman_model", "rn_jpeg_huffman_batch_device", "rn_jpeg_huffman_batch", "rn_classify_jpeg_files",
    "rn_jpeg_last_huffman_ms", "rn_jpeg_last_huffman_rounds",
    "rn_jpeg_probe_oriented", "rn_jpeg_scan_probe_oriented", "rn_jpeg_oriented_size",
    "rn_jpeg_encode_info", "rn_jpeg_encoded_bound", "rn_jpeg_entropy_encode", "rn_jpeg_overlay_batch_device",
    "rn_jpeg_encode_batch_device", "rn_jpeg_last_encode_ms",
    "rn_jpeg_encode_headers", "rn_jpeg_huffenc_model", "rn_jpeg_huffenc_batch", "rn_jpeg_encode_files_device", "rn_jpeg_last_huffenc_ms",
    "rn_cam_overlay_batch_device", "rn_cam_last_overlay_ms",
    "rn_occlusion_plan", "rn_occlusion_masks_device", "rn_occlusion_u8_device", "rn_occlusion_u8", "rn_occlusion_last_ms",
    "rn_faith_plan", "rn_faith_rank_model", "rn_faith_ranks_device", "rn_faith_masks_device", "rn_faith_u8_device", "rn_faith_u8",
    "rn_faith_last_ms",
)

# what rn_ft_read returns of a trained variable (include/roomnet_hip.h: fine-tuning)
RN_FT_PARAM, RN_FT_GRAD, RN_FT_ADAM_M, RN_FT_ADAM_V = 0, 1, 2, 3
RN_FT_BEST = 4                           # the master parameters as they were at the best validation point

# rn_views_batch_device / rn_ft_run_views flags (include/roomnet_hip.h: fine-tuning on fresh random views)
RN_VIEW_CROP, RN_VIEW_FLIP, RN_VIEW_SITE = 1, 2, 254

# the layers rn_grad_cam_* explains (include/roomnet_hip.h: grad-CAM)
GRAD_CAM_LAYERS = ("s6.bn", "s7.bn")


class RoomNetLibraryError(RuntimeError):
    """libroomnet_hip.so is missing / unloadable, or a call into it failed."""


_fp = C.POINTER(C.c_float)


class rn_conv_stage(C.Structure):
    _fields_ = [("cin", C.c_int32), ("cout", C.c_int32), ("pool_k", C.c_int32), ("pool_s", C.c_int32),
                ("skip_stage", C.c_int32),
                ("kernel", _fp), ("gamma", _fp), ("beta", _fp), ("mean", _fp), ("variance", _fp),
                ("gamma2", _fp), ("beta2", _fp), ("mean2", _fp), ("variance2", _fp)]


class rn_dense_layer(C.Structure):
    _fields_ = [("nin", C.c_int32), ("nout", C.c_int32), ("kernel", _fp), ("bias", _fp),
                ("gamma", _fp), ("beta", _fp), ("mean", _fp), ("variance", _fp)]


class rn_weights(C.Structure):
    _fields_ = [("im_side", C.c_int32), ("num_classes", C.c_int32), ("n_stages", C.c_int32),
                ("n_dense", C.c_int32), ("bn_epsilon", C.c_float),
                ("stages", C.POINTER(rn_conv_stage)), ("dense", C.POINTER(rn_dense_layer))]


class rn_f32m_stage_plan(C.Structure):
    _fields_ = [(name, C.c_int) for name in ("kind", "variant", "live_cin", "frozen_couts", "npt", "ringcols", "lds", "n_colblocks", "n_ctg", "threads")]


class rn_stage_ms(C.Structure):
    _fields_ = [("n_stages", C.c_int32), ("preprocess_ms", C.c_float),
                ("stage_ms", C.c_float * RN_MAX_STAGES), ("head_ms", C.c_float), ("total_ms", C.c_float)]


class rn_node_info(C.Structure):
    _fields_ = [("name", C.c_char * RN_NAME_LEN), ("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32)]


class rn_ft_config(C.Structure):
    _fields_ = [("learn_rate", C.c_float), ("decay_rate", C.c_float), ("num_steps", C.c_int32), ("start_step", C.c_int32),
                ("l2_coeff", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float)]


RN_JPEG_REASON_LEN = 48


class rn_view(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("side", C.c_int32), ("fliplr", C.c_int32), ("flipud", C.c_int32)]


class rn_view_source(C.Structure):
    _fields_ = [("d_bgr", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32)]


class rn_jpeg_info(C.Structure):
    """What ``rn_jpeg_probe`` reads from a JPEG file's headers (include/roomnet_hip.h: baseline JPEG files)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hsamp", C.c_int32), ("vsamp", C.c_int32),
                ("restart_interval", C.c_int32), ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3),
                ("supported", C.c_int32), ("qt", (C.c_uint16 * 64) * 3), ("reason", C.c_char * RN_JPEG_REASON_LEN)]


def jpeg_oriented_shape(info) -> Tuple[int, int]:
    """``(height, width)`` of the image the pixel stage writes for a supported ``rn_jpeg_info``: the stored size, swapped when
    ``supported`` is an EXIF orientation of 5..8 (``rn_jpeg_oriented_size``)."""
    h, w = int(info.height), int(info.width)
    return (w, h) if int(info.supported) >= 5 else (h, w)


class rn_jpeg_image(C.Structure):
    _fields_ = [("info", rn_jpeg_info), ("coeffs", C.c_void_p)]


class rn_jpeg_hufftab(C.Structure):
    _fields_ = [("look", C.c_uint16 * 512), ("maxcode", C.c_int32 * 18), ("valoff", C.c_int32 * 17), ("vals", C.c_uint8 * 256)]


class rn_jpeg_scan(C.Structure):
    """What ``rn_jpeg_scan_probe`` adds to ``rn_jpeg_info``: the scan's byte range and the components' Huffman lookup tables."""
    _fields_ = [("scan_begin", C.c_uint64), ("scan_len", C.c_uint64), ("dc", rn_jpeg_hufftab * 3), ("ac", rn_jpeg_hufftab * 3)]


class rn_jpeg_file(C.Structure):
    _fields_ = [("info", rn_jpeg_info), ("scan", rn_jpeg_scan), ("bytes", C.c_void_p)]


# the status of an image after the GPU Huffman pass (include/roomnet_hip.h)
(RN_JPEG_ST_OK, RN_JPEG_ST_INVALID_CODE, RN_JPEG_ST_RUN_PAST_BLOCK, RN_JPEG_ST_TRUNCATED, RN_JPEG_ST_RESTART, RN_JPEG_ST_COEF_LIMIT,
 RN_JPEG_ST_NOT_SYNCED, RN_JPEG_ST_TOO_LARGE) = range(8)
RN_JPEG_SUBSEQ_BYTES = 128

RN_JPEG_MAX_OVERLAYS = 8


class rn_jpeg_overlay(C.Structure):
    """One rasterised text line for ``rn_jpeg_overlay_batch_device`` / ``rn_jpeg_encode_batch_device``: its box inside the image, its
    colour and the host address of its float32 ``[h, w]`` coverage (``hershey.coverage``)."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("color_bgr", C.c_uint8 * 3),
                ("coverage", C.c_void_p)]


class rn_jpeg_source(C.Structure):
    _fields_ = [("d_bgr", C.c_void_p), ("info", rn_jpeg_info), ("overlays", C.POINTER(rn_jpeg_overlay)), ("n_overlays", C.c_int32),
                ("coeffs", C.c_void_p)]


class rn_cam_target(C.Structure):
    """One image of ``rn_cam_overlay_batch_device``: a BGR image in device memory and the device map to draw on its crop window."""
    _fields_ = [("d_bgr", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("d_cam", C.c_void_p), ("cam_h", C.c_int32),
                ("cam_w", C.c_int32)]


_lib: Optional[C.CDLL] = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load libroomnet_hip.so and declare its prototypes.  Raises if unavailable."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("ROOMNET_HIP_LIB", LIB_PATH)
    if not os.path.isfile(p):
        raise RoomNetLibraryError(
            "libroomnet_hip.so not found at %r -- build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or roomnet_amd/csrc/build.sh" % p)
    try:
        lib = C.CDLL(p)
    except OSError as e:
        raise RoomNetLibraryError("cannot load %r: %s" % (p, e)) from e
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.rn_create.argtypes = [C.POINTER(rn_weights), i32, i32, i32, C.c_uint, C.POINTER(vp)]
    lib.rn_create.restype = i32
    lib.rn_destroy.argtypes = [vp]
    lib.rn_destroy.restype = None
    lib.rn_last_error.argtypes = []
    lib.rn_last_error.restype = C.c_char_p
    lib.rn_version.argtypes = []
    lib.rn_version.restype = C.c_char_p
    lib.rn_device_count.argtypes = []
    lib.rn_device_count.restype = i32
    for name in ("rn_forward_u8", "rn_forward_f32", "rn_forward_u8_device", "rn_forward_f32_device"):
        fn = getattr(lib, name)
        fn.argtypes = [vp, vp, i32, vp, vp]
        fn.restype = i32
    lib.rn_submit_u8.argtypes = [vp, vp, i32, i32]
    lib.rn_submit_u8.restype = i32
    lib.rn_collect.argtypes = [vp, i32, vp, vp]
    lib.rn_collect.restype = i32
    lib.rn_sync.argtypes = [vp]
    lib.rn_sync.restype = i32
    lib.rn_set_stream.argtypes = [vp, vp]
    lib.rn_set_stream.restype = i32
    lib.rn_set_stream_null.argtypes = [vp]
    lib.rn_set_stream_null.restype = i32
    lib.rn_node_count.argtypes = [vp]
    lib.rn_node_count.restype = i32
    lib.rn_node_info_get.argtypes = [vp, i32, C.POINTER(rn_node_info)]
    lib.rn_node_info_get.restype = i32
    lib.rn_tap.argtypes = [vp, i32, vp, sz, C.POINTER(sz)]
    lib.rn_tap.restype = i32
    lib.rn_set_profiling.argtypes = [vp, i32]
    lib.rn_set_profiling.restype = i32
    lib.rn_timing.argtypes = [vp, C.POINTER(rn_stage_ms)]
    lib.rn_timing.restype = i32
    lib.rn_dominant_stage.argtypes = [vp]
    lib.rn_dominant_stage.restype = i32
    lib.rn_stage_launch.argtypes = [vp, i32]
    lib.rn_stage_launch.restype = i32
    lib.rn_device_malloc.argtypes = [vp, sz, C.POINTER(vp)]
    lib.rn_device_malloc.restype = i32
    lib.rn_device_free.argtypes = [vp, vp]
    lib.rn_device_free.restype = i32
    lib.rn_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    lib.rn_memcpy_h2d.restype = i32
    if hasattr(lib, "rn_const_info"):
        lib.rn_const_info.argtypes = [vp, C.POINTER(C.c_int)]
        lib.rn_const_info.restype = i32
    if hasattr(lib, "rn_frozen_info"):
        lib.rn_frozen_info.argtypes = [vp, C.POINTER(C.c_int)]
        lib.rn_frozen_info.restype = i32
    if hasattr(lib, "rn_host_alloc"):           # (absent from the older libraries tools/gpu_var.sh loads through ROOMNET_HIP_LIB as A/B arms)
        lib.rn_host_alloc.argtypes = [sz, C.POINTER(vp)]
        lib.rn_host_alloc.restype = i32
        lib.rn_host_free.argtypes = [vp]
        lib.rn_host_free.restype = i32
    lib.rn_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    lib.rn_memcpy_d2h.restype = i32
    lib.rn_crop_resize_u8_device.argtypes = [vp, vp, i32, i32, vp, i32]
    lib.rn_crop_resize_u8_device.restype = i32
    if hasattr(lib, "rn_crop_resize_batch_u8_device"):
        lib.rn_crop_resize_batch_u8_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int), i32, vp]
        lib.rn_crop_resize_batch_u8_device.restype = i32
    lib.rn_classify_images_u8.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int), i32, vp, vp]
    lib.rn_classify_images_u8.restype = i32
    lib.rn_group_create.argtypes = [C.POINTER(rn_weights), i32, C.POINTER(C.c_int), i32, i32, C.c_uint, C.POINTER(vp)]
    lib.rn_group_create.restype = i32
    lib.rn_group_destroy.argtypes = [vp]
    lib.rn_group_destroy.restype = None
    lib.rn_group_size.argtypes = [vp]
    lib.rn_group_size.restype = i32
    lib.rn_group_handle.argtypes = [vp, i32]
    lib.rn_group_handle.restype = vp
    lib.rn_group_forward_u8.argtypes = [vp, vp, i32, vp, vp]
    lib.rn_group_forward_u8.restype = i32
    lib.rn_group_forward_u8_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int)]
    lib.rn_group_forward_u8_device.restype = i32
    lib.rn_group_result_buffer.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz)]
    lib.rn_group_result_buffer.restype = i32
    lib.rn_group_sync.argtypes = [vp]
    lib.rn_group_sync.restype = i32
    if hasattr(lib, "rn_group_plan"):
        lib.rn_group_plan.argtypes = [i32, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(sz)]
        lib.rn_group_plan.restype = i32
    if hasattr(lib, "rn_f32m_plan"):
        lib.rn_f32m_plan.argtypes = [i32] * 9 + [C.POINTER(rn_f32m_stage_plan)]
        lib.rn_f32m_plan.restype = i32
    if hasattr(lib, "rn_band_plan"):
        lib.rn_band_plan.argtypes = [i32] * 8 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.rn_band_plan.restype = i32
    if hasattr(lib, "rn_grad_cam_u8"):
        for name in ("rn_grad_cam_u8", "rn_grad_cam_f32", "rn_grad_cam_u8_device"):
            fn = getattr(lib, name)
            fn.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp]
            fn.restype = i32
    if hasattr(lib, "rn_bn_count"):
        lib.rn_bn_count.argtypes = [vp]
        lib.rn_bn_count.restype = i32
        lib.rn_bn_info.argtypes = [vp, i32, C.POINTER(rn_node_info)]
        lib.rn_bn_info.restype = i32
        lib.rn_bn_batch_stats.argtypes = [vp, i32, vp, vp, C.POINTER(C.c_int64)]
        lib.rn_bn_batch_stats.restype = i32
    if hasattr(lib, "rn_ft_create"):
        lib.rn_features_shape.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.rn_features_shape.restype = i32
        lib.rn_features_u8.argtypes = [vp, vp, i32, vp]
        lib.rn_features_u8.restype = i32
        lib.rn_features_u8_device.argtypes = [vp, vp, i32, vp]
        lib.rn_features_u8_device.restype = i32
        lib.rn_ft_create.argtypes = [C.POINTER(rn_weights), i32, i32, C.POINTER(rn_ft_config), C.POINTER(vp)]
        lib.rn_ft_create.restype = i32
        lib.rn_ft_destroy.argtypes = [vp]
        lib.rn_ft_destroy.restype = None
        lib.rn_ft_run.argtypes = [vp, vp, vp, C.c_int64, vp, i32, i32, vp]
        lib.rn_ft_run.restype = i32
        lib.rn_ft_eval.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp]
        lib.rn_ft_eval.restype = i32
        lib.rn_ft_var_count.argtypes = [vp]
        lib.rn_ft_var_count.restype = i32
        lib.rn_ft_var_info.argtypes = [vp, i32, C.c_char_p, sz, C.POINTER(C.c_int64)]
        lib.rn_ft_var_info.restype = i32
        lib.rn_ft_read.argtypes = [vp, i32, i32, vp, sz]
        lib.rn_ft_read.restype = i32
        lib.rn_ft_step_count.argtypes = [vp]
        lib.rn_ft_step_count.restype = C.c_int64
        lib.rn_ft_last_run_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.rn_ft_last_run_ms.restype = i32
        lib.rn_ft_upload.argtypes = [vp, vp, sz, C.POINTER(vp)]
        lib.rn_ft_upload.restype = i32
        lib.rn_ft_free.argtypes = [vp, vp]
        lib.rn_ft_free.restype = i32
    if hasattr(lib, "rn_ft_create_depth"):
        lib.rn_features_depth_shape.argtypes = [vp, i32, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.rn_features_depth_shape.restype = i32
        lib.rn_features_depth_u8.argtypes = [vp, i32, vp, i32, vp]
        lib.rn_features_depth_u8.restype = i32
        lib.rn_features_depth_u8_device.argtypes = [vp, i32, vp, i32, vp]
        lib.rn_features_depth_u8_device.restype = i32
        lib.rn_ft_create_depth.argtypes = [C.POINTER(rn_weights), i32, i32, C.POINTER(rn_ft_config), i32, C.POINTER(vp)]
        lib.rn_ft_create_depth.restype = i32
        lib.rn_ft_depth.argtypes = [vp]
        lib.rn_ft_depth.restype = i32
    if hasattr(lib, "rn_ft_set_dropout"):
        lib.rn_ft_set_dropout.argtypes = [vp, C.c_float, C.c_uint64]
        lib.rn_ft_set_dropout.restype = i32
        lib.rn_ft_dropout.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        lib.rn_ft_dropout.restype = i32
        lib.rn_ft_dropout_mask.argtypes = [vp, i32, C.c_int64, i32, C.c_int64, vp]
        lib.rn_ft_dropout_mask.restype = i32
    if hasattr(lib, "rn_ft_run_validated"):
        lib.rn_ft_val_points.argtypes = [vp, i32, i32, vp, i32]
        lib.rn_ft_val_points.restype = i32
        lib.rn_ft_run_validated.argtypes = [vp, vp, vp, C.c_int64, vp, i32, i32, vp, vp, vp, C.c_int64, i32, vp, vp]
        lib.rn_ft_run_validated.restype = i32
        lib.rn_ft_best.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.rn_ft_best.restype = i32
    if hasattr(lib, "rn_ft_run_views"):
        lib.rn_view_draw.argtypes = [C.c_uint64, C.c_int64, i32, i32, i32, C.c_uint, C.POINTER(rn_view)]
        lib.rn_view_draw.restype = i32
        lib.rn_views_create.argtypes = [vp, C.POINTER(rn_view_source), C.c_int64, C.POINTER(vp)]
        lib.rn_views_create.restype = i32
        lib.rn_views_destroy.argtypes = [vp]
        lib.rn_views_destroy.restype = None
        lib.rn_views_batch_device.argtypes = [vp, vp, vp, C.c_int64, i32, C.c_uint64, C.c_int64, C.c_uint, vp]
        lib.rn_views_batch_device.restype = i32
        lib.rn_ft_run_views.argtypes = [vp, vp, vp, vp, C.c_int64, vp, i32, i32, C.c_uint64, C.c_uint, vp, vp, vp, C.c_int64, i32, vp, vp]
        lib.rn_ft_run_views.restype = i32
    if hasattr(lib, "rn_jpeg_probe"):
        lib.rn_jpeg_probe.argtypes = [C.c_char_p, sz, C.POINTER(rn_jpeg_info)]
        lib.rn_jpeg_probe.restype = i32
        lib.rn_jpeg_coeff_count.argtypes = [C.POINTER(rn_jpeg_info)]
        lib.rn_jpeg_coeff_count.restype = sz
        lib.rn_jpeg_entropy_decode.argtypes = [C.c_char_p, sz, C.POINTER(rn_jpeg_info), vp, sz]
        lib.rn_jpeg_entropy_decode.restype = i32
        lib.rn_jpeg_decode_batch_device.argtypes = [vp, C.POINTER(rn_jpeg_image), i32, C.POINTER(vp)]
        lib.rn_jpeg_decode_batch_device.restype = i32
        lib.rn_classify_jpegs.argtypes = [vp, C.POINTER(rn_jpeg_image), i32, vp, vp]
        lib.rn_classify_jpegs.restype = i32
        lib.rn_jpeg_last_decode_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.rn_jpeg_last_decode_ms.restype = i32
    if hasattr(lib, "rn_jpeg_scan_probe"):
        lib.rn_jpeg_scan_probe.argtypes = [vp, sz, C.POINTER(rn_jpeg_scan)]
        lib.rn_jpeg_scan_probe.restype = i32
        lib.rn_jpeg_huffman_model.argtypes = [C.c_char_p, sz, C.POINTER(rn_jpeg_info), vp, sz, i32, C.POINTER(i32)]
        lib.rn_jpeg_huffman_model.restype = i32
        for name in ("rn_jpeg_huffman_batch_device", "rn_jpeg_huffman_batch"):
            getattr(lib, name).argtypes = [vp, C.POINTER(rn_jpeg_file), i32, C.POINTER(vp), vp]
            getattr(lib, name).restype = i32
        lib.rn_classify_jpeg_files.argtypes = [vp, C.POINTER(rn_jpeg_file), i32, vp, vp, vp]
        lib.rn_classify_jpeg_files.restype = i32
        lib.rn_jpeg_last_huffman_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.rn_jpeg_last_huffman_ms.restype = i32
        lib.rn_jpeg_last_huffman_rounds.argtypes = [vp, i32, vp, vp]
        lib.rn_jpeg_last_huffman_rounds.restype = i32
    if hasattr(lib, "rn_jpeg_probe_oriented"):
        lib.rn_jpeg_probe_oriented.argtypes = [C.c_char_p, sz, C.POINTER(rn_jpeg_info)]
        lib.rn_jpeg_probe_oriented.restype = i32
        lib.rn_jpeg_scan_probe_oriented.argtypes = [vp, sz, C.POINTER(rn_jpeg_scan)]
        lib.rn_jpeg_scan_probe_oriented.restype = i32
        lib.rn_jpeg_oriented_size.argtypes = [C.POINTER(rn_jpeg_info), C.POINTER(i32), C.POINTER(i32)]
        lib.rn_jpeg_oriented_size.restype = i32
    if hasattr(lib, "rn_jpeg_encode_info"):
        lib.rn_jpeg_encode_info.argtypes = [i32, i32, i32, C.POINTER(rn_jpeg_info)]
        lib.rn_jpeg_encode_info.restype = i32
        lib.rn_jpeg_encoded_bound.argtypes = [C.POINTER(rn_jpeg_info)]
        lib.rn_jpeg_encoded_bound.restype = sz
        lib.rn_jpeg_entropy_encode.argtypes = [C.POINTER(rn_jpeg_info), vp, vp, sz, C.POINTER(sz)]
        lib.rn_jpeg_entropy_encode.restype = i32
        for name in ("rn_jpeg_overlay_batch_device", "rn_jpeg_encode_batch_device"):
            getattr(lib, name).argtypes = [vp, C.POINTER(rn_jpeg_source), i32]
            getattr(lib, name).restype = i32
        lib.rn_jpeg_last_encode_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.rn_jpeg_last_encode_ms.restype = i32
    if hasattr(lib, "rn_jpeg_huffenc_model"):
        lib.rn_jpeg_encode_headers.argtypes = [C.POINTER(rn_jpeg_info), vp, sz, C.POINTER(sz)]
        lib.rn_jpeg_encode_headers.restype = i32
        lib.rn_jpeg_huffenc_model.argtypes = [C.POINTER(rn_jpeg_info), vp, vp, sz, C.POINTER(sz), C.POINTER(i32)]
        lib.rn_jpeg_huffenc_model.restype = i32
        lib.rn_jpeg_huffenc_batch.argtypes = [vp, C.POINTER(rn_jpeg_info), C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), vp]
        lib.rn_jpeg_huffenc_batch.restype = i32
        lib.rn_jpeg_encode_files_device.argtypes = [vp, C.POINTER(rn_jpeg_source), i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), vp]
        lib.rn_jpeg_encode_files_device.restype = i32
        lib.rn_jpeg_last_huffenc_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.rn_jpeg_last_huffenc_ms.restype = i32
    if hasattr(lib, "rn_cam_overlay_batch_device"):
        lib.rn_cam_overlay_batch_device.argtypes = [vp, C.POINTER(rn_cam_target), i32, C.c_double]
        lib.rn_cam_overlay_batch_device.restype = i32
        lib.rn_cam_last_overlay_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.rn_cam_last_overlay_ms.restype = i32
    if hasattr(lib, "rn_occlusion_plan"):
        lib.rn_occlusion_plan.argtypes = [i32] * 5 + [C.POINTER(C.c_int)] * 3
        lib.rn_occlusion_plan.restype = i32
        lib.rn_occlusion_masks_device.argtypes = [vp, vp, i32, i32, i32, vp, i32, i32, vp]
        lib.rn_occlusion_masks_device.restype = i32
        for name in ("rn_occlusion_u8_device", "rn_occlusion_u8"):
            fn = getattr(lib, name)
            fn.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
            fn.restype = i32
        lib.rn_occlusion_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.rn_occlusion_last_ms.restype = i32
    if hasattr(lib, "rn_faith_plan"):
        lib.rn_faith_plan.argtypes = [i32] * 5 + [C.POINTER(C.c_int)] * 2
        lib.rn_faith_plan.restype = i32
        lib.rn_faith_rank_model.argtypes = [vp, i32, i32, vp]
        lib.rn_faith_rank_model.restype = i32
        lib.rn_faith_ranks_device.argtypes = [vp, vp, i32, vp]
        lib.rn_faith_ranks_device.restype = i32
        lib.rn_faith_masks_device.argtypes = [vp, vp, vp, i32, i32, i32, vp, i32, i32, vp]
        lib.rn_faith_masks_device.restype = i32
        for name in ("rn_faith_u8_device", "rn_faith_u8"):
            fn = getattr(lib, name)
            fn.argtypes = [vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
            fn.restype = i32
        lib.rn_faith_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.rn_faith_last_ms.restype = i32
    if path is None:
        _lib = lib
    return lib


def _check(lib: C.CDLL, rc: int, what: str) -> None:
    if rc != RN_OK:
        msg = lib.rn_last_error()
        text = msg.decode("utf-8", "replace") if msg else ""
        if rc in (-1, -5):
            raise ValueError("%s failed (%d): %s" % (what, rc, text))
        raise RoomNetLibraryError("%s failed (%d): %s" % (what, rc, text))


def device_count() -> int:
    return int(load_library().rn_device_count())


class _Packed:
    """Keeps the float32 arrays alive while the C structs point into them."""

    def __init__(self, graph: Graph, weights: Dict[str, np.ndarray]):
        self.keep: List[np.ndarray] = []
        self.stages = (rn_conv_stage * len(graph.stages))()
        self.dense = (rn_dense_layer * len(graph.dense))()

        def ptr(name: str, shape: Tuple[int, ...]):
            if name not in weights:
                raise KeyError("tensor %r not found in checkpoint" % name)
            a = np.ascontiguousarray(weights[name], dtype=np.float32)
            if tuple(a.shape) != tuple(shape):
                raise ValueError("tensor %r has shape %s, the graph needs %s"
                                 % (name, tuple(a.shape), tuple(shape)))
            self.keep.append(a)
            return a.ctypes.data_as(_fp)

        for i, s in enumerate(graph.stages):
            st = self.stages[i]
            st.cin, st.cout, st.pool_k, st.pool_s, st.skip_stage = s.cin, s.cout, s.pool_k, s.pool_s, s.skip_stage
            st.kernel = ptr(s.conv_name + "/kernel", (3, 3, s.cin, s.cout))
            st.gamma = ptr(s.bn_name + "/gamma", (s.cout,))
            st.beta = ptr(s.bn_name + "/beta", (s.cout,))
            st.mean = ptr(s.bn_name + "/moving_mean", (s.cout,))
            st.variance = ptr(s.bn_name + "/moving_variance", (s.cout,))
            if s.residual:
                st.gamma2 = ptr(s.bn2_name + "/gamma", (s.cout,))
                st.beta2 = ptr(s.bn2_name + "/beta", (s.cout,))
                st.mean2 = ptr(s.bn2_name + "/moving_mean", (s.cout,))
                st.variance2 = ptr(s.bn2_name + "/moving_variance", (s.cout,))
        for i, d in enumerate(graph.dense):
            dl = self.dense[i]
            dl.nin, dl.nout = d.nin, d.nout
            dl.kernel = ptr(d.name + "/kernel", (d.nin, d.nout))
            if d.biased:
                dl.bias = ptr(d.name + "/bias", (d.nout,))
            if d.bn_name:
                dl.gamma = ptr(d.bn_name + "/gamma", (d.nout,))
                dl.beta = ptr(d.bn_name + "/beta", (d.nout,))
                dl.mean = ptr(d.bn_name + "/moving_mean", (d.nout,))
                dl.variance = ptr(d.bn_name + "/moving_variance", (d.nout,))
        self.w = rn_weights()
        self.w.im_side = graph.im_side
        self.w.num_classes = graph.num_classes
        self.w.n_stages = len(graph.stages)
        self.w.n_dense = len(graph.dense)
        self.w.bn_epsilon = BN_EPSILON
        self.w.stages = C.cast(self.stages, C.POINTER(rn_conv_stage))
        self.w.dense = C.cast(self.dense, C.POINTER(rn_dense_layer))


class Engine:
    """One rn_handle: a model instance bound to one GPU and one stream."""

    def __init__(self, graph: Graph, weights: Dict[str, np.ndarray], device: int = 0, dtype="f32",
                 max_batch: int = 64, taps: bool = False, lib_path: Optional[str] = None,
                 stage_launches: bool = False, generic_kernels: bool = False, pair32: bool = False,
                 compute_frozen: bool = False, no_dither: bool = False, batch_stats: bool = False):
        if pair32 and lib_path is None and "ROOMNET_HIP_LIB" not in os.environ:
            lib_path = AB_LIB_PATH           # (the round-2 comparison kernels are not in the product library)
        self.lib = load_library(lib_path)
        self.graph = graph
        self.dtype = DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
        self.max_batch = int(max_batch)
        self.device = int(device)
        packed = _Packed(graph, weights)
        h = C.c_void_p()
        rc = self.lib.rn_create(C.byref(packed.w), self.device, self.dtype, self.max_batch,
                                (RN_FLAG_TAPS if taps else 0) | (RN_FLAG_STAGE_LAUNCHES if stage_launches else 0)
                                | (RN_FLAG_GENERIC_KERNELS if generic_kernels else 0)
                                | (RN_FLAG_PAIR_32X32 if pair32 else 0)
                                | (RN_FLAG_COMPUTE_FROZEN if compute_frozen else 0)
                                | (RN_FLAG_NO_DITHER if no_dither else 0)
                                | (RN_FLAG_BATCH_STATS if batch_stats else 0), C.byref(h))
        _check(self.lib, rc, "rn_create")
        self._h = h
        self._nodes: Optional[Dict[str, Tuple[int, Tuple[int, int, int]]]] = None

    # -- lifetime
    def close(self) -> None:
        if getattr(self, "_h", None):
            for p in (getattr(self, "_jpeg_dst", 0), getattr(self, "_jpeg_src", 0), getattr(self, "_jpeg_res", 0),
                      getattr(self, "_cam_maps", 0), getattr(self, "_occ_maps", 0), getattr(self, "_occ_drops", 0)):
                # (jpegs_to_batch's / classify_resident's / explain_resident's / occlusion_resident's device buffers)
                if p:
                    self.lib.rn_device_free(self._h, C.c_void_p(p))
            self._jpeg_dst = self._jpeg_src = self._jpeg_src_cap = self._jpeg_res = self._cam_maps = 0
            self._occ_maps = self._occ_drops = self._occ_drops_cap = 0
            self.lib.rn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise RoomNetLibraryError("engine is closed")
        return self._h

    # -- forward
    def forward_u8(self, im_bgr_u8: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        s = self.graph.im_side
        im = np.ascontiguousarray(im_bgr_u8, dtype=np.uint8)
        if im.ndim != 4 or im.shape[1:] != (s, s, 3):
            raise ValueError("expected a [N,%d,%d,3] uint8 batch, got %s" % (s, s, im.shape))
        n = im.shape[0]
        probs = np.empty((n, self.graph.num_classes), np.float32)
        ids = np.empty((n,), np.int64)
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            rc = self.lib.rn_forward_u8(self.handle, im[i:i + m].ctypes.data, m, probs[i:i + m].ctypes.data,
                                        ids[i:i + m].ctypes.data)
            _check(self.lib, rc, "rn_forward_u8")
        return ids, probs

    def classify_images(self, images) -> Tuple[np.ndarray, np.ndarray]:
        """``images``: sequence of BGR uint8 HWC arrays of any (individual) size.  Centre crop + INTER_LINEAR resize
        run on the GPU (``rn_classify_images_u8``); returns ``(ids [n], probs [n, C])``."""
        ims = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        for im in ims:
            if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError("expected HWC uint8 images with 3 channels, got %s" % (im.shape,))
        n = len(ims)
        probs = np.empty((n, self.graph.num_classes), np.float32)
        ids = np.empty((n,), np.int64)
        for i in range(0, n, self.max_batch):
            chunk = ims[i:i + self.max_batch]
            m = len(chunk)
            ptrs = (C.c_void_p * m)(*[im.ctypes.data for im in chunk])
            hs = (C.c_int * m)(*[im.shape[0] for im in chunk])
            ws = (C.c_int * m)(*[im.shape[1] for im in chunk])
            rc = self.lib.rn_classify_images_u8(self.handle, ptrs, hs, ws, m, probs[i:i + m].ctypes.data,
                                                ids[i:i + m].ctypes.data)
            _check(self.lib, rc, "rn_classify_images_u8")
        return ids, probs

    @staticmethod
    def _jpeg_images(items):
        """``[(rn_jpeg_info, coefficient address or int16 array)]`` -> the C array ``rn_jpeg_image[n]`` (the arrays stay the caller's)."""
        arr = (rn_jpeg_image * len(items))()
        for k, (info, coeffs) in enumerate(items):
            arr[k].info = info
            arr[k].coeffs = coeffs.ctypes.data if isinstance(coeffs, np.ndarray) else int(coeffs)
        return arr

    def classify_jpegs(self, items) -> Tuple[np.ndarray, np.ndarray]:
        """``items``: ``[(rn_jpeg_info, coeffs)]`` of supported baseline JPEG files as ``jpegdec.probe`` / ``entropy_decode`` give
        them (``coeffs``: an int16 array or the address of one, e.g. inside a ``PinnedArray``).  Pixel stage, centre crop, resize
        and forward pass on the GPU (``rn_classify_jpegs``); returns ``(ids [n], probs [n, C])``, bit-identical to
        ``classify_images`` of the decoded files."""
        items = list(items)
        n = len(items)
        probs = np.empty((n, self.graph.num_classes), np.float32)
        ids = np.empty((n,), np.int64)
        for i in range(0, n, self.max_batch):
            arr = self._jpeg_images(items[i:i + self.max_batch])
            m = len(arr)
            _check(self.lib, self.lib.rn_classify_jpegs(self.handle, arr, m, probs[i:i + m].ctypes.data, ids[i:i + m].ctypes.data),
                   "rn_classify_jpegs")
        return ids, probs

    @staticmethod
    def _jpeg_files(items):
        """``[(rn_jpeg_info, rn_jpeg_scan, scan bytes)]`` -> the C array ``rn_jpeg_file[n]``; the scan bytes are a uint8 array that
        holds exactly them, or the address of their first one (the buffers stay the caller's)."""
        arr = (rn_jpeg_file * max(len(items), 1))()
        for k, (info, scan, data) in enumerate(items):
            arr[k].info = info
            arr[k].scan = scan
            arr[k].bytes = data.ctypes.data if isinstance(data, np.ndarray) else int(data)
        return arr

    def jpeg_huffman_batch(self, items):
        """One ``rn_jpeg_huffman_batch`` call over ``items`` (as ``_jpeg_files`` takes them, at most ``max_batch``): the Huffman pass
        on the GPU.  Returns ``(status int32 [n], [int16 coefficient array per image])``; the array of an image whose status is not
        0 is left as zeros."""
        items = list(items)
        n = len(items)
        arr = self._jpeg_files(items)
        outs = [np.zeros(max(1, sum(int(info.blocks_w[c]) * int(info.blocks_h[c]) * 64 for c in range(min(max(info.ncomp, 0), 3)))),
                         np.int16) for info, _s, _d in items]
        ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        status = np.full((max(n, 1),), -1, np.int32)
        _check(self.lib, self.lib.rn_jpeg_huffman_batch(self.handle, arr, n, ptrs, status.ctypes.data), "rn_jpeg_huffman_batch")
        return status[:n], outs

    def classify_jpeg_files(self, items) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``items``: ``[(rn_jpeg_info, rn_jpeg_scan, scan bytes)]`` of supported baseline JPEG files as ``jpegdec.load_file_bytes``
        gives them.  Huffman pass, pixel stage, centre crop, resize and forward pass on the GPU (``rn_classify_jpeg_files``);
        returns ``(ids [n], probs [n, C], status [n])``: where ``status`` is 0 the results are bit-identical to ``classify_jpegs``,
        elsewhere the id is -1 and the file is one for the host's Huffman pass."""
        items = list(items)
        n = len(items)
        probs = np.empty((n, self.graph.num_classes), np.float32)
        ids = np.empty((n,), np.int64)
        status = np.empty((n,), np.int32)
        for i in range(0, n, self.max_batch):
            chunk = items[i:i + self.max_batch]
            m = len(chunk)
            _check(self.lib, self.lib.rn_classify_jpeg_files(self.handle, self._jpeg_files(chunk), m, probs[i:i + m].ctypes.data,
                                                             ids[i:i + m].ctypes.data, status[i:i + m].ctypes.data),
                   "rn_classify_jpeg_files")
        return ids, probs, status

    def jpeg_last_huffman_ms(self) -> float:
        """Device time of the last batch's Huffman launches (``rn_jpeg_last_huffman_ms``)."""
        ms = C.c_float(0.0)
        _check(self.lib, self.lib.rn_jpeg_last_huffman_ms(self.handle, C.byref(ms)), "rn_jpeg_last_huffman_ms")
        return float(ms.value)

    def jpeg_last_huffman_rounds(self, n: int) -> Tuple[np.ndarray, np.ndarray]:
        """Synchronisation rounds of the last Huffman batch's ``n`` images: ``(inside groups, across groups)``."""
        inside, across = np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(self.lib, self.lib.rn_jpeg_last_huffman_rounds(self.handle, n, inside.ctypes.data, across.ctypes.data),
               "rn_jpeg_last_huffman_rounds")
        return inside, across

    def jpeg_decode_batch(self, items, repeat: int = 1):
        """One ``rn_jpeg_decode_batch_device`` call over ``items`` (as ``classify_jpegs`` takes them, at most ``max_batch``): the
        list of decoded BGR uint8 ``[h, w, 3]`` images, read back (parity tests, timing; ``repeat`` > 1 issues the call that often)."""
        items = list(items)
        n = len(items)
        arr = self._jpeg_images(items)
        shapes = [jpeg_oriented_shape(info) + (3,) for info, _c in items]
        d_out = [self.device_malloc(max(1, h * w * 3)) for h, w, _ in shapes]
        try:
            ptrs = (C.c_void_p * max(n, 1))(*d_out)
            for _ in range(max(1, repeat)):
                _check(self.lib, self.lib.rn_jpeg_decode_batch_device(self.handle, arr, n, ptrs), "rn_jpeg_decode_batch_device")
            self.sync()
            outs = []
            for d, shape in zip(d_out, shapes):
                a = np.empty(shape, np.uint8)
                self.d2h(a, d)
                outs.append(a)
            return outs
        finally:
            for d in d_out:
                self.device_free(d)

    def _stage_resident(self, jpegs, images):
        """``jpegs`` ``[(rn_jpeg_info, coeffs)]`` decoded (``rn_jpeg_decode_batch_device``) and ``images`` (BGR uint8 HWC arrays)
        uploaded into a device buffer this engine keeps and grows, then ONE crop + resize launch
        (``rn_crop_resize_batch_u8_device``) into ``self._jpeg_dst``.  Returns ``(addresses, shapes)`` of the full-size images,
        jpegs first; they stay valid until the next call.  Asynchronous; at most ``max_batch`` files."""
        shapes = [jpeg_oriented_shape(info) for info, _c in jpegs] + [im.shape[:2] for im in images]
        m, s = len(shapes), self.graph.im_side
        if not getattr(self, "_jpeg_dst", 0):
            self._jpeg_dst, self._jpeg_src, self._jpeg_src_cap = self.device_malloc(self.max_batch * s * s * 3), 0, 0
        sizes = [(h * w * 3 + 15) & ~15 for h, w in shapes]
        if sum(sizes) > self._jpeg_src_cap:
            self.sync()
            if self._jpeg_src:
                self.device_free(self._jpeg_src)
            self._jpeg_src_cap = sum(sizes) + sum(sizes) // 4
            self._jpeg_src = self.device_malloc(self._jpeg_src_cap)
        addrs = [self._jpeg_src + int(o) for o in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
        ptrs = (C.c_void_p * m)(*addrs)
        if jpegs:
            _check(self.lib, self.lib.rn_jpeg_decode_batch_device(self.handle, self._jpeg_images(jpegs), len(jpegs), ptrs),
                   "rn_jpeg_decode_batch_device")
        for a, im in zip(addrs[len(jpegs):], images):
            self.h2d(a, im)
        hs = (C.c_int * m)(*[h for h, _w in shapes])
        ws = (C.c_int * m)(*[w for _h, w in shapes])
        _check(self.lib, self.lib.rn_crop_resize_batch_u8_device(self.handle, ptrs, hs, ws, m, C.c_void_p(self._jpeg_dst)),
               "rn_crop_resize_batch_u8_device")
        return addrs, shapes

    def jpegs_to_batch(self, items) -> np.ndarray:
        """``items`` as ``classify_jpegs`` takes them -> their centre-cropped, resized images, uint8 BGR ``[n, S, S, 3]`` on the
        host: pixel stage (``rn_jpeg_decode_batch_device``) into a device buffer this engine keeps and grows, ONE crop + resize
        launch (``rn_crop_resize_batch_u8_device``), and only the ``S x S`` results come back."""
        items = list(items)
        s = self.graph.im_side
        out = np.empty((len(items), s, s, 3), np.uint8)
        for i in range(0, len(items), self.max_batch):
            chunk = items[i:i + self.max_batch]
            self._stage_resident(chunk, [])
            self.sync()
            self.d2h(out[i:i + len(chunk)], self._jpeg_dst)
        return out

    def classify_resident(self, jpegs, images):
        """Classify a chunk and KEEP its full-size images on the device: ``jpegs`` are decoded there and ``images`` uploaded
        (``_stage_resident``), then ``rn_forward_u8_device`` on the cropped, resized batch -- the launches of ``classify_jpegs`` /
        ``classify_images``, so the same bits.  Returns ``(ids, probs, addresses, shapes)``, jpegs first; the addresses stay valid
        until the next ``classify_resident`` / ``jpegs_to_batch`` call (``jpeg_encode_batch`` takes them).  At most ``max_batch``."""
        jpegs, images = list(jpegs), [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        m, nc = len(jpegs) + len(images), self.graph.num_classes
        if not 1 <= m <= self.max_batch:
            raise ValueError("classify_resident: %d files (1..%d)" % (m, self.max_batch))
        addrs, shapes = self._stage_resident(jpegs, images)
        if not getattr(self, "_jpeg_res", 0):
            self._jpeg_res = self.device_malloc(self.max_batch * (nc * 4 + 8))
        d_probs, d_ids = self._jpeg_res, self._jpeg_res + self.max_batch * nc * 4
        self.forward_u8_device(self._jpeg_dst, m, d_probs, d_ids)
        self.sync()
        probs, ids = np.empty((m, nc), np.float32), np.empty((m,), np.int64)
        self.d2h(probs, d_probs)
        self.d2h(ids, d_ids)
        return ids, probs, addrs, shapes

    def explain_resident(self, jpegs, images, layer, class_ids=None):
        """``classify_resident`` with the evidence: the chunk is staged the same way, then ``rn_grad_cam_u8_device`` runs on the
        cropped, resized batch instead of the forward pass and its maps STAY on the device.  ``class_ids``: int per file or None
        (each file's argmax).  Returns ``(ids, probs, addresses, shapes, d_cams, (mh, mw))``: ``ids`` / ``probs`` are
        ``classify_resident``'s bits (the grad-CAM contract), ``d_cams[k]`` the device address of file k's float32 ``[mh, mw]`` map,
        valid like the image addresses until the next ``explain_resident`` (``cam_overlay_batch`` takes both)."""
        if layer not in GRAD_CAM_LAYERS:
            raise ValueError("grad_cam: layer must be one of %s, got %r" % (GRAD_CAM_LAYERS, layer))
        jpegs, images = list(jpegs), [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        m, nc = len(jpegs) + len(images), self.graph.num_classes
        if not 1 <= m <= self.max_batch:
            raise ValueError("explain_resident: %d files (1..%d)" % (m, self.max_batch))
        addrs, shapes = self._stage_resident(jpegs, images)
        if not getattr(self, "_jpeg_res", 0):
            self._jpeg_res = self.device_malloc(self.max_batch * (nc * 4 + 8))
        per_map = max(h * w for _id, (h, w, _c) in (self.nodes()[name] for name in GRAD_CAM_LAYERS)) * 4
        if not getattr(self, "_cam_maps", 0):
            self._cam_maps = self.device_malloc(self.max_batch * (per_map + 4))         # the maps, then the class ids
        d_probs, d_ids = self._jpeg_res, self._jpeg_res + self.max_batch * nc * 4
        d_cls = None
        if class_ids is not None:
            d_cls = self._cam_maps + self.max_batch * per_map
            self.h2d(d_cls, np.ascontiguousarray(np.broadcast_to(np.asarray(class_ids), (m,)), dtype=np.int32))
        self.grad_cam_u8_device(self._jpeg_dst, m, d_cls, layer, self._cam_maps, None, d_probs, d_ids)
        self.sync()
        probs, ids = np.empty((m, nc), np.float32), np.empty((m,), np.int64)
        self.d2h(probs, d_probs)
        self.d2h(ids, d_ids)
        mh, mw, _c = self.nodes()[layer][1]
        return ids, probs, addrs, shapes, [self._cam_maps + k * mh * mw * 4 for k in range(m)], (mh, mw)

    def occlusion_resident(self, jpegs, images, patch: int = 32, stride: int = 16, fill="mean", class_ids=None):
        """``explain_resident`` with occlusion-sensitivity maps: the chunk is staged the same way, then ``rn_occlusion_u8_device`` runs
        on the cropped, resized batch -- pass 0, the masked passes, the pixel map -- and the maps STAY on the device.  Returns
        ``(ids, probs, addresses, shapes, d_maps, (S, S))``: ``ids`` / ``probs`` are ``classify_resident``'s bits, ``d_maps[k]`` the
        device address of file k's float32 ``[S, S]`` map, valid like the image addresses until the next ``occlusion_resident``
        (``cam_overlay_batch`` takes both)."""
        jpegs, images = list(jpegs), [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        m, nc, s = len(jpegs) + len(images), self.graph.num_classes, self.graph.im_side
        if not 1 <= m <= self.max_batch:
            raise ValueError("occlusion_resident: %d files (1..%d)" % (m, self.max_batch))
        _g, n_windows, _c = self.occlusion_plan(m, patch, stride)
        self._occlusion_fill(fill)               # (a bad fill is refused before anything is staged)
        addrs, shapes = self._stage_resident(jpegs, images)
        if not getattr(self, "_jpeg_res", 0):
            self._jpeg_res = self.device_malloc(self.max_batch * (nc * 4 + 8))
        if not getattr(self, "_occ_maps", 0):
            self._occ_maps, self._occ_drops, self._occ_drops_cap = self.device_malloc(self.max_batch * (s * s * 4 + 4)), 0, 0    # the maps, then the class ids
        if n_windows > self._occ_drops_cap:
            self.sync()
            if self._occ_drops:
                self.device_free(self._occ_drops)
            self._occ_drops_cap = n_windows + n_windows // 4
            self._occ_drops = self.device_malloc(self._occ_drops_cap * 4)
        d_probs, d_ids = self._jpeg_res, self._jpeg_res + self.max_batch * nc * 4
        d_cls = None
        if class_ids is not None:
            d_cls = self._occ_maps + self.max_batch * s * s * 4
            self.h2d(d_cls, np.ascontiguousarray(np.broadcast_to(np.asarray(class_ids), (m,)), dtype=np.int32))
        self.occlusion_u8_device(self._jpeg_dst, m, d_cls, patch, stride, fill, self._occ_drops, self._occ_maps, d_probs, d_ids)
        self.sync()
        probs, ids = np.empty((m, nc), np.float32), np.empty((m,), np.int64)
        self.d2h(probs, d_probs)
        self.d2h(ids, d_ids)
        return ids, probs, addrs, shapes, [self._occ_maps + k * s * s * 4 for k in range(m)], (s, s)

    def cam_overlay_batch(self, items, weight: float = 0.5) -> None:
        """``rn_cam_overlay_batch_device`` over ``items`` ``[(device image address, (height, width), device map address, (mh, mw))]``
        (at most ``max_batch``): each map is drawn as a heat map on its image's crop window, in place -- the bytes of
        ``cam.overlay_image``.  Asynchronous, ordered in front of a following ``jpeg_overlay_batch`` / ``jpeg_encode_batch``."""
        arr = (rn_cam_target * max(len(items), 1))()
        for k, (d_bgr, (h, w), d_cam, (mh, mw)) in enumerate(items):
            arr[k].d_bgr, arr[k].height, arr[k].width = int(d_bgr), int(h), int(w)
            arr[k].d_cam, arr[k].cam_h, arr[k].cam_w = int(d_cam), int(mh), int(mw)
        _check(self.lib, self.lib.rn_cam_overlay_batch_device(self.handle, arr, len(items), float(weight)), "rn_cam_overlay_batch_device")

    def cam_last_overlay_ms(self) -> float:
        """Device time of the last heat-map batch's two launches (``rn_cam_last_overlay_ms``)."""
        ms = C.c_float(0)
        _check(self.lib, self.lib.rn_cam_last_overlay_ms(self.handle, C.byref(ms)), "rn_cam_last_overlay_ms")
        return float(ms.value)

    def jpeg_last_decode_ms(self) -> float:
        """Device time of the last JPEG batch's pixel stage (``rn_jpeg_last_decode_ms``)."""
        ms = C.c_float(0)
        _check(self.lib, self.lib.rn_jpeg_last_decode_ms(self.handle, C.byref(ms)), "rn_jpeg_last_decode_ms")
        return float(ms.value)

    @staticmethod
    def _jpeg_sources(items):
        """``[(device image address, rn_jpeg_info of jpegenc.encode_info, overlays, coefficient address / int16 array / None)]``
        with ``overlays`` a list of ``(x, y, coverage float32 [h, w], color_bgr)`` -> ``(rn_jpeg_source[n], what it points into)``."""
        arr = (rn_jpeg_source * max(len(items), 1))()
        keep = []
        for k, (d_bgr, info, overlays, coeffs) in enumerate(items):
            ovs = (rn_jpeg_overlay * max(len(overlays), 1))()
            for j, (x, y, cov, color) in enumerate(overlays):
                cov = np.ascontiguousarray(cov, dtype=np.float32)
                ovs[j].x, ovs[j].y, ovs[j].h, ovs[j].w = int(x), int(y), int(cov.shape[0]), int(cov.shape[1])
                ovs[j].color_bgr[:] = [int(c) for c in color]
                ovs[j].coverage = cov.ctypes.data
                keep.append(cov)
            keep.append(ovs)
            arr[k].d_bgr = int(d_bgr)
            arr[k].info = info
            arr[k].overlays = C.cast(ovs, C.POINTER(rn_jpeg_overlay))
            arr[k].n_overlays = len(overlays)
            arr[k].coeffs = 0 if coeffs is None else (coeffs.ctypes.data if isinstance(coeffs, np.ndarray) else int(coeffs))
        return arr, keep

    def jpeg_overlay_batch(self, items) -> None:
        """``rn_jpeg_overlay_batch_device`` over ``items`` (as ``_jpeg_sources`` takes them, at most ``max_batch``): the overlays are
        drawn into the device images, in order.  Asynchronous; the coverages are copied before it returns."""
        arr, _keep = self._jpeg_sources(items)
        _check(self.lib, self.lib.rn_jpeg_overlay_batch_device(self.handle, arr, len(items)), "rn_jpeg_overlay_batch_device")

    def jpeg_encode_batch(self, items) -> None:
        """``rn_jpeg_encode_batch_device`` over ``items``: overlays, then the pixel stage of the JPEG encode; each image's quantised
        coefficients arrive in its coefficient buffer (``jpegenc.entropy_encode`` writes the file from them).  ``sync()`` before
        reading them."""
        arr, _keep = self._jpeg_sources(items)
        _check(self.lib, self.lib.rn_jpeg_encode_batch_device(self.handle, arr, len(items)), "rn_jpeg_encode_batch_device")

    def jpeg_last_encode_ms(self) -> float:
        """Device time of the last encoded batch's launches (``rn_jpeg_last_encode_ms``)."""
        ms = C.c_float(0)
        _check(self.lib, self.lib.rn_jpeg_last_encode_ms(self.handle, C.byref(ms)), "rn_jpeg_last_encode_ms")
        return float(ms.value)

    @staticmethod
    def _file_buffers(bufs, caps):
        """uint8 arrays (or ``PinnedArray``s) -> ``(pointers, caps, lens)`` C arrays; ``caps``: bytes announced per buffer
        (default: all of each)."""
        arrays = [b.array if isinstance(b, PinnedArray) else b for b in bufs]
        for a in arrays:
            assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
        n = max(len(arrays), 1)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrays])
        sizes = (C.c_size_t * n)(*[a.size if caps is None else int(caps[k]) for k, a in enumerate(arrays)])
        return ptrs, sizes, (C.c_size_t * n)()

    def jpeg_huffenc_batch(self, items, bufs=None, caps=None):
        """``rn_jpeg_huffenc_batch`` over ``items`` ``[(rn_jpeg_info of jpegenc.encode_info, int16 coefficient array)]`` (at most
        ``max_batch``): the Huffman pass of the output file on the GPU, on arbitrary coefficients.  ``bufs``: uint8 arrays the
        files are written into (default: new arrays of ``jpegenc.encoded_bound`` bytes), ``caps`` the bytes announced of each.
        Returns ``(files, lens, status)``: ``files[k]`` is ``bytes`` where ``status[k]`` is 0 (``RN_JPEG_ENC_ST_OK``: the file
        ``jpegenc.entropy_encode`` writes), else None.  Synchronous."""
        n = len(items)
        infos = (rn_jpeg_info * max(n, 1))(*[info for info, _c in items])
        coeffs = [np.ascontiguousarray(c, dtype=np.int16) for _i, c in items]
        cptr = (C.c_void_p * max(n, 1))(*[c.ctypes.data for c in coeffs])
        if bufs is None:
            bufs = [np.empty(max(int(self.lib.rn_jpeg_encoded_bound(C.byref(info))), 1), np.uint8) for info, _c in items]
        ptrs, sizes, lens = self._file_buffers(bufs, caps)
        status = np.zeros(max(n, 1), np.int32)
        _check(self.lib, self.lib.rn_jpeg_huffenc_batch(self.handle, infos, cptr, n, ptrs, sizes, lens, status.ctypes.data), "rn_jpeg_huffenc_batch")
        arrays = [b.array if isinstance(b, PinnedArray) else b for b in bufs]
        files = [arrays[k][:lens[k]].tobytes() if status[k] == 0 else None for k in range(n)]
        return files, [int(lens[k]) for k in range(n)], status[:n]

    def jpeg_encode_files(self, items, bufs, caps=None):
        """``rn_jpeg_encode_files_device`` over ``items`` (as ``_jpeg_sources`` takes them; the coefficient entry is ignored): the
        overlays, the encode's pixel stage and the Huffman pass on the GPU; file k arrives in ``bufs[k]`` -- page-locked
        ``PinnedArray``s (or uint8 arrays); ``jpegenc.encoded_bound(info)`` bytes always suffice, a file that needs more than
        its buffer gets status ``RN_JPEG_ENC_ST_CAP`` and its needed size in ``lens[k]``.  Returns ``(lens, status)``: where
        ``status[k]`` is 0, ``bufs[k][:lens[k]]`` is the file ``jpegenc.entropy_encode`` writes for the image.  Synchronous."""
        arr, _keep = self._jpeg_sources([(a, info, ov, None) for a, info, ov, *_rest in items])
        ptrs, sizes, lens = self._file_buffers(bufs, caps)
        status = np.zeros(max(len(items), 1), np.int32)
        _check(self.lib, self.lib.rn_jpeg_encode_files_device(self.handle, arr, len(items), ptrs, sizes, lens, status.ctypes.data),
               "rn_jpeg_encode_files_device")
        return [int(lens[k]) for k in range(len(items))], status[:len(items)]

    def jpeg_last_huffenc_ms(self) -> float:
        """Device time of the last batch's Huffman-encode launches (``rn_jpeg_last_huffenc_ms``)."""
        ms = C.c_float(0)
        _check(self.lib, self.lib.rn_jpeg_last_huffenc_ms(self.handle, C.byref(ms)), "rn_jpeg_last_huffenc_ms")
        return float(ms.value)

    def crop_resize(self, im_bgr_u8: np.ndarray) -> np.ndarray:
        """One image through the device crop + resize; returns the ``[S, S, 3]`` uint8 result (parity tests)."""
        im = np.ascontiguousarray(im_bgr_u8, dtype=np.uint8)
        s = self.graph.im_side
        d_src = self.device_malloc(im.nbytes)
        d_dst = self.device_malloc(self.max_batch * s * s * 3)
        try:
            self.h2d(d_src, im)
            rc = self.lib.rn_crop_resize_u8_device(self.handle, C.c_void_p(d_src), im.shape[0], im.shape[1],
                                                   C.c_void_p(d_dst), 0)
            _check(self.lib, rc, "rn_crop_resize_u8_device")
            out = np.empty((s, s, 3), np.uint8)
            self.d2h(out, d_dst)
            return out
        finally:
            self.device_free(d_src)
            self.device_free(d_dst)

    def crop_resize_batch(self, ims, repeat: int = 1) -> np.ndarray:
        """A list of images (any sizes, <= max_batch of them) through the BATCHED device crop + resize -- one launch for all of them
        (``rn_crop_resize_batch_u8_device``); returns the ``[n, S, S, 3]`` uint8 results.  ``repeat`` > 1 launches it that often
        (profiling / timing of the one kernel)."""
        ims = [np.ascontiguousarray(im, dtype=np.uint8) for im in ims]
        n, s = len(ims), self.graph.im_side
        d_srcs = [self.device_malloc(im.nbytes) for im in ims]
        d_dst = self.device_malloc(self.max_batch * s * s * 3)
        try:
            for d, im in zip(d_srcs, ims):
                self.h2d(d, im)
            ptrs = (C.c_void_p * n)(*d_srcs)
            hs = (C.c_int * n)(*[im.shape[0] for im in ims])
            ws = (C.c_int * n)(*[im.shape[1] for im in ims])
            for _ in range(max(1, repeat)):
                _check(self.lib, self.lib.rn_crop_resize_batch_u8_device(self.handle, ptrs, hs, ws, n, C.c_void_p(d_dst)),
                       "rn_crop_resize_batch_u8_device")
            self.sync()
            out = np.empty((n, s, s, 3), np.uint8)
            self.d2h(out, d_dst)
            return out
        finally:
            for d in d_srcs:
                self.device_free(d)
            self.device_free(d_dst)

    # -- training views (include/roomnet_hip.h: fine-tuning on fresh random views)
    def views_create(self, images) -> "Views":
        """A list of whole BGR uint8 photographs of any size, uploaded ONCE into one device allocation, and the table
        ``rn_views_create`` makes of them: the resident training set of ``views_batch`` and ``Trainer.run_views``.  A failed
        allocation raises ``RoomNetLibraryError`` naming the bytes the set needs.  ``views_destroy`` (or ``Views.close``) frees both."""
        ims = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        for i, im in enumerate(ims):
            if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError("views_create: image %d is not a BGR [H, W, 3] array (shape %s)" % (i, im.shape))
        if not ims:
            raise ValueError("views_create: no image")
        offsets, total = [], 0
        for im in ims:
            offsets.append(total)
            total += (im.nbytes + 255) & ~255
        try:
            d_pixels = self.device_malloc(total)
        except RoomNetLibraryError as e:
            raise RoomNetLibraryError("views_create: the %d photographs need %d bytes of device memory: %s" % (len(ims), total, e)) from None
        v = C.c_void_p()
        try:
            srcs = (rn_view_source * len(ims))()
            for k, (im, off) in enumerate(zip(ims, offsets)):
                self.h2d(d_pixels + off, im)
                srcs[k] = rn_view_source(d_pixels + off, im.shape[0], im.shape[1])
            _check(self.lib, self.lib.rn_views_create(self.handle, srcs, len(ims), C.byref(v)), "rn_views_create")
        except Exception:
            self.device_free(d_pixels)
            raise
        return Views(self, v, d_pixels, [im.shape[:2] for im in ims], total)

    def views_destroy(self, views: "Views") -> None:
        views.close()

    def views_batch(self, views: "Views", index, step: int, seed: int = 0, crop: bool = True, flip: bool = True, repeat: int = 1) -> np.ndarray:
        """The views of one minibatch, made on the GPU in one launch (``rn_views_batch_device``): slot ``b`` is the view of item
        ``index[b]`` at global step ``step``; returns uint8 ``[n, S, S, 3]`` (``finetune.make_view`` of ``finetune.view_draw`` states
        the same bytes).  ``repeat`` > 1 launches it that often back to back, without a synchronisation in between."""
        index = np.ascontiguousarray(index, np.int32).reshape(-1)
        n, s = int(index.size), self.graph.im_side
        if index.size and (index.min() < 0 or index.max() >= views.n_items):
            raise ValueError("views_batch: an index outside [0, %d)" % views.n_items)
        flags = (RN_VIEW_CROP if crop else 0) | (RN_VIEW_FLIP if flip else 0)
        d_index = self.device_malloc(max(index.nbytes, 4))
        d_dst = self.device_malloc(self.max_batch * s * s * 3)
        try:
            if n:
                self.h2d(d_index, index)
            for _ in range(max(1, int(repeat))):
                _check(self.lib, self.lib.rn_views_batch_device(self.handle, views.handle, C.c_void_p(d_index), 0, n,
                                                                C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(step), flags,
                                                                C.c_void_p(d_dst)), "rn_views_batch_device")
            self.sync()
            out = np.empty((n, s, s, 3), np.uint8)
            self.d2h(out, d_dst)
            return out
        finally:
            self.device_free(d_index)
            self.device_free(d_dst)

    def forward_f32(self, x_rgb: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        s = self.graph.im_side
        x = np.ascontiguousarray(x_rgb, dtype=np.float32)
        if x.ndim != 4 or x.shape[1:] != (s, s, 3):
            raise ValueError("expected a [N,%d,%d,3] float32 batch, got %s" % (s, s, x.shape))
        n = x.shape[0]
        probs = np.empty((n, self.graph.num_classes), np.float32)
        ids = np.empty((n,), np.int64)
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            rc = self.lib.rn_forward_f32(self.handle, x[i:i + m].ctypes.data, m, probs[i:i + m].ctypes.data,
                                         ids[i:i + m].ctypes.data)
            _check(self.lib, rc, "rn_forward_f32")
        return ids, probs

    def forward_u8_device(self, d_bgr: int, n: int, d_probs: int, d_ids: int) -> None:
        """Asynchronous: raw device pointers (e.g. ``tensor.data_ptr()``)."""
        rc = self.lib.rn_forward_u8_device(self.handle, C.c_void_p(d_bgr), n, C.c_void_p(d_probs),
                                           C.c_void_p(d_ids))
        _check(self.lib, rc, "rn_forward_u8_device")

    def grad_cam(self, x: np.ndarray, class_ids=None, layer: str = "s6.bn", with_alpha: bool = False):
        """Grad-CAM maps of a batch (``rn_grad_cam_u8`` for uint8 BGR ``[N,S,S,3]``, ``rn_grad_cam_f32`` for a pre-processed
        float RGB batch on float32 handles).  ``class_ids``: int per image or None (each image's argmax); ``layer``: "s6.bn" or
        "s7.bn".  Returns ``(cam [N,h,w] float32, ids [N] int64, probs [N,C] float32)`` and, with ``with_alpha``, ``alpha [N,c]``
        last.  Score, gradient rules and layers: include/roomnet_hip.h, grad-CAM."""
        if layer not in GRAD_CAM_LAYERS:
            raise ValueError("grad_cam: layer must be one of %s, got %r" % (GRAD_CAM_LAYERS, layer))
        s = self.graph.im_side
        x = np.asarray(x)
        if x.ndim != 4 or x.shape[1:] != (s, s, 3):
            raise ValueError("expected a [N,%d,%d,3] batch, got %s" % (s, s, x.shape))
        u8 = x.dtype == np.uint8
        x = np.ascontiguousarray(x, dtype=np.uint8 if u8 else np.float32)
        fn = self.lib.rn_grad_cam_u8 if u8 else self.lib.rn_grad_cam_f32
        nid, (h, w, c) = self.nodes()[layer]
        n = x.shape[0]
        cls = None
        if class_ids is not None:
            cls = np.ascontiguousarray(np.broadcast_to(np.asarray(class_ids), (n,)), dtype=np.int32)
        cam = np.empty((n, h, w), np.float32)
        alpha = np.empty((n, c), np.float32)
        probs = np.empty((n, self.graph.num_classes), np.float32)
        ids = np.empty((n,), np.int64)
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            rc = fn(self.handle, x[i:i + m].ctypes.data, m, None if cls is None else cls[i:i + m].ctypes.data, nid,
                    cam[i:i + m].ctypes.data, alpha[i:i + m].ctypes.data if with_alpha else None, probs[i:i + m].ctypes.data,
                    ids[i:i + m].ctypes.data)
            _check(self.lib, rc, "rn_grad_cam")
        if with_alpha:
            return cam, ids, probs, alpha
        return cam, ids, probs

    def grad_cam_u8_device(self, d_bgr: int, n: int, d_class_ids: Optional[int], layer: str, d_cam: int, d_alpha: Optional[int],
                           d_probs: int, d_ids: int) -> None:
        """Asynchronous ``rn_grad_cam_u8_device`` on raw device pointers."""
        if layer not in GRAD_CAM_LAYERS:
            raise ValueError("grad_cam: layer must be one of %s, got %r" % (GRAD_CAM_LAYERS, layer))
        rc = self.lib.rn_grad_cam_u8_device(self.handle, C.c_void_p(d_bgr), n, C.c_void_p(d_class_ids) if d_class_ids else None,
                                            self.nodes()[layer][0], C.c_void_p(d_cam), C.c_void_p(d_alpha) if d_alpha else None,
                                            C.c_void_p(d_probs), C.c_void_p(d_ids))
        _check(self.lib, rc, "rn_grad_cam_u8_device")

    # -- occlusion-sensitivity maps (include/roomnet_hip.h; roomnet_amd/occlusion.py is the NumPy statement)
    @staticmethod
    def _occlusion_fill(fill):
        """``"mean"`` -> None (the library computes the per-image means), a BGR triple -> three bytes."""
        if isinstance(fill, str):
            if fill != "mean":
                raise ValueError("occlusion: fill must be 'mean' or a BGR triple, got %r" % (fill,))
            return None
        f = np.asarray(fill)
        if f.shape != (3,) or (f < 0).any() or (f > 255).any():
            raise ValueError("occlusion: fill must be 'mean' or a BGR triple of 0..255, got %r" % (fill,))
        return (C.c_uint8 * 3)(*[int(v) for v in f])

    def occlusion_plan(self, n: int, patch: int, stride: int) -> Tuple[int, int, int]:
        """``rn_occlusion_plan`` for this engine's side and ``max_batch``: ``(G, n_windows, n_chunks)``."""
        return occlusion_plan(self.graph.im_side, patch, stride, n, self.max_batch, lib=self.lib)

    def occlusion_masks_device(self, d_bgr: int, n: int, patch: int, stride: int, fill, first: int, count: int, d_out: int) -> None:
        """Asynchronous ``rn_occlusion_masks_device`` on raw device pointers: the masked images ``[first, first + count)``."""
        rc = self.lib.rn_occlusion_masks_device(self.handle, C.c_void_p(d_bgr), n, patch, stride, self._occlusion_fill(fill), first, count,
                                                C.c_void_p(d_out))
        _check(self.lib, rc, "rn_occlusion_masks_device")

    def occlusion_u8_device(self, d_bgr: int, n: int, d_class_ids: Optional[int], patch: int, stride: int, fill, d_drop: int,
                            d_map: Optional[int], d_probs: int, d_ids: int) -> None:
        """Asynchronous ``rn_occlusion_u8_device`` on raw device pointers."""
        rc = self.lib.rn_occlusion_u8_device(self.handle, C.c_void_p(d_bgr), n, C.c_void_p(d_class_ids) if d_class_ids else None, patch,
                                             stride, self._occlusion_fill(fill), C.c_void_p(d_drop), C.c_void_p(d_map) if d_map else None,
                                             C.c_void_p(d_probs), C.c_void_p(d_ids))
        _check(self.lib, rc, "rn_occlusion_u8_device")

    def occlusion_u8(self, im_bgr_u8: np.ndarray, class_ids=None, patch: int = 32, stride: int = 16, fill="mean", with_map: bool = True):
        """Occlusion-sensitivity maps of a uint8 BGR ``[N,S,S,3]`` batch (``rn_occlusion_u8`` per ``max_batch`` images).  Returns
        ``(maps [N,S,S] float32 or None, drops [N,G,G] float32, ids [N] int64, probs [N,C] float32)``."""
        s = self.graph.im_side
        im = np.ascontiguousarray(im_bgr_u8, dtype=np.uint8)
        if im.ndim != 4 or im.shape[1:] != (s, s, 3):
            raise ValueError("expected a [N,%d,%d,3] uint8 batch, got %s" % (s, s, im.shape))
        n = im.shape[0]
        g = self.occlusion_plan(min(n, self.max_batch), patch, stride)[0]         # (refuses an empty batch and a bad grid)
        fill_c = self._occlusion_fill(fill)
        cls = None
        if class_ids is not None:
            cls = np.ascontiguousarray(np.broadcast_to(np.asarray(class_ids), (n,)), dtype=np.int32)
        maps = np.empty((n, s, s), np.float32) if with_map else None
        drops = np.empty((n, g, g), np.float32)
        probs = np.empty((n, self.graph.num_classes), np.float32)
        ids = np.empty((n,), np.int64)
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            rc = self.lib.rn_occlusion_u8(self.handle, im[i:i + m].ctypes.data, m, None if cls is None else cls[i:i + m].ctypes.data,
                                          patch, stride, fill_c, drops[i:i + m].ctypes.data, maps[i:i + m].ctypes.data if with_map else None,
                                          probs[i:i + m].ctypes.data, ids[i:i + m].ctypes.data)
            _check(self.lib, rc, "rn_occlusion_u8")
        return maps, drops, ids, probs

    def occlusion_last_ms(self) -> float:
        """Device time of the last occlusion call, pass 0 to the map (``rn_occlusion_last_ms``)."""
        ms = C.c_float(0)
        _check(self.lib, self.lib.rn_occlusion_last_ms(self.handle, C.byref(ms)), "rn_occlusion_last_ms")
        return float(ms.value)

    # -- deletion / insertion curves of a heat map (include/roomnet_hip.h; roomnet_amd/faithfulness.py is the NumPy statement)
    def faith_plan(self, n: int, steps: int, modes=3) -> Tuple[int, int]:
        """``rn_faith_plan`` for this engine's side and ``max_batch``: ``(n_passes, n_chunks)``."""
        from .faithfulness import mode_mask
        return faith_plan(self.graph.im_side, steps, modes if isinstance(modes, int) else mode_mask(modes), n, self.max_batch, lib=self.lib)

    def faith_ranks_device(self, d_map: int, n: int, d_rank: int) -> None:
        """Asynchronous ``rn_faith_ranks_device`` on raw device pointers: ``[n,S,S]`` float32 maps -> ``[n,S,S]`` uint32 ranks."""
        _check(self.lib, self.lib.rn_faith_ranks_device(self.handle, C.c_void_p(d_map), n, C.c_void_p(d_rank)), "rn_faith_ranks_device")

    def faith_masks_device(self, d_bgr: int, d_map: int, n: int, steps: int, modes, fill, first: int, count: int, d_out: int) -> None:
        """Asynchronous ``rn_faith_masks_device`` on raw device pointers: the masked images of the passes ``[first, first + count)``."""
        from .faithfulness import mode_mask
        rc = self.lib.rn_faith_masks_device(self.handle, C.c_void_p(d_bgr), C.c_void_p(d_map), n, steps, mode_mask(modes),
                                            self._occlusion_fill(fill), first, count, C.c_void_p(d_out))
        _check(self.lib, rc, "rn_faith_masks_device")

    def faith_u8_device(self, d_bgr: int, d_map: int, n: int, d_class_ids: Optional[int], steps: int, modes, fill, d_curve: int,
                        d_auc: int, d_probs: int, d_ids: int) -> None:
        """Asynchronous ``rn_faith_u8_device`` on raw device pointers."""
        from .faithfulness import mode_mask
        rc = self.lib.rn_faith_u8_device(self.handle, C.c_void_p(d_bgr), C.c_void_p(d_map), n, C.c_void_p(d_class_ids) if d_class_ids else None,
                                         steps, mode_mask(modes), self._occlusion_fill(fill), C.c_void_p(d_curve), C.c_void_p(d_auc),
                                         C.c_void_p(d_probs), C.c_void_p(d_ids))
        _check(self.lib, rc, "rn_faith_u8_device")

    def faith_u8(self, im_bgr_u8: np.ndarray, maps: np.ndarray, class_ids=None, steps: int = 32, modes=3, fill="mean"):
        """Deletion / insertion curves of ``[N,S,S]`` float32 maps on a uint8 BGR ``[N,S,S,3]`` batch (``rn_faith_u8`` per ``max_batch``
        images).  Returns ``(curves [N,M,J+1] float32, aucs [N,M] float32, ids [N] int64, probs [N,C] float32)``."""
        from .faithfulness import mode_mask, mode_slots
        s = self.graph.im_side
        im = np.ascontiguousarray(im_bgr_u8, dtype=np.uint8)
        if im.ndim != 4 or im.shape[1:] != (s, s, 3):
            raise ValueError("expected a [N,%d,%d,3] uint8 batch, got %s" % (s, s, im.shape))
        n = im.shape[0]
        maps = np.ascontiguousarray(maps, dtype=np.float32)
        if maps.shape != (n, s, s):
            raise ValueError("expected [%d,%d,%d] float32 maps, got %s" % (n, s, s, maps.shape))
        mask, m_curves = mode_mask(modes), len(mode_slots(modes))
        self.faith_plan(min(n, self.max_batch), steps, mask)          # (refuses an empty batch and bad steps)
        fill_c = self._occlusion_fill(fill)
        cls = None
        if class_ids is not None:
            cls = np.ascontiguousarray(np.broadcast_to(np.asarray(class_ids), (n,)), dtype=np.int32)
        curves = np.empty((n, m_curves, steps + 1), np.float32)
        aucs = np.empty((n, m_curves), np.float32)
        probs = np.empty((n, self.graph.num_classes), np.float32)
        ids = np.empty((n,), np.int64)
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            rc = self.lib.rn_faith_u8(self.handle, im[i:i + m].ctypes.data, maps[i:i + m].ctypes.data, m,
                                      None if cls is None else cls[i:i + m].ctypes.data, steps, mask, fill_c, curves[i:i + m].ctypes.data,
                                      aucs[i:i + m].ctypes.data, probs[i:i + m].ctypes.data, ids[i:i + m].ctypes.data)
            _check(self.lib, rc, "rn_faith_u8")
        return curves, aucs, ids, probs

    def faith_last_ms(self) -> float:
        """Device time of the last faithfulness call, or of the last ``faith_ranks_device``'s rank launch (``rn_faith_last_ms``)."""
        ms = C.c_float(0)
        _check(self.lib, self.lib.rn_faith_last_ms(self.handle, C.byref(ms)), "rn_faith_last_ms")
        return float(ms.value)

    def features_shape(self, depth: int = 2) -> Tuple[int, int, int]:
        """Per-image shape of the fine-tuning feature of a trainer of ``depth``: ``s7.bn`` at depth 2 (``rn_features_shape``),
        ``s6.bn`` at depth 3 (``rn_features_depth_shape``)."""
        side, ch = C.c_int(0), C.c_int(0)
        if depth == 2:
            _check(self.lib, self.lib.rn_features_shape(self.handle, C.byref(side), C.byref(ch)), "rn_features_shape")
        else:
            _check(self.lib, self.lib.rn_features_depth_shape(self.handle, int(depth), C.byref(side), C.byref(ch)),
                   "rn_features_depth_shape")
        return side.value, side.value, ch.value

    def features_u8(self, im_bgr_u8: np.ndarray, depth: int = 2) -> np.ndarray:
        """The feature a ``Trainer`` of ``depth`` trains on, of a uint8 BGR ``[N,S,S,3]`` batch, widened to float32: ``s7.bn``
        ``[N, side, side, 16]`` at depth 2 (``rn_features_u8``; 28 KB per image at 224), ``s6.bn`` ``[N, side, side, 128]`` at
        depth 3 (``rn_features_depth_u8``; 1.08 MB per image at 224)."""
        s = self.graph.im_side
        im = np.ascontiguousarray(im_bgr_u8, dtype=np.uint8)
        if im.ndim != 4 or im.shape[1:] != (s, s, 3):
            raise ValueError("expected a [N,%d,%d,3] uint8 batch, got %s" % (s, s, im.shape))
        n = im.shape[0]
        out = np.empty((n,) + self.features_shape(depth), np.float32)
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            if depth == 2:
                _check(self.lib, self.lib.rn_features_u8(self.handle, im[i:i + m].ctypes.data, m, out[i:i + m].ctypes.data),
                       "rn_features_u8")
            else:
                _check(self.lib, self.lib.rn_features_depth_u8(self.handle, int(depth), im[i:i + m].ctypes.data, m,
                                                               out[i:i + m].ctypes.data), "rn_features_depth_u8")
        return out

    def features_u8_device(self, d_bgr: int, n: int, d_feat: int, depth: int = 2) -> None:
        """Asynchronous ``rn_features_u8_device`` (depth 3: ``rn_features_depth_u8_device``) on raw device pointers."""
        if depth == 2:
            _check(self.lib, self.lib.rn_features_u8_device(self.handle, C.c_void_p(d_bgr), n, C.c_void_p(d_feat)),
                   "rn_features_u8_device")
        else:
            _check(self.lib, self.lib.rn_features_depth_u8_device(self.handle, int(depth), C.c_void_p(d_bgr), n, C.c_void_p(d_feat)),
                   "rn_features_depth_u8_device")

    def sync(self) -> None:
        _check(self.lib, self.lib.rn_sync(self.handle), "rn_sync")

    def submit_u8(self, bgr_nhwc: np.ndarray, slot: int) -> None:
        """Upload + enqueue one batch (<= max_batch images) into pipeline slot 0 or 1 (``rn_submit_u8``)."""
        s = self.graph.im_side
        x = np.ascontiguousarray(bgr_nhwc, dtype=np.uint8)
        if x.ndim != 4 or x.shape[1:] != (s, s, 3):
            raise ValueError("expected uint8 [n,%d,%d,3], got %s" % (s, s, x.shape))
        _check(self.lib, self.lib.rn_submit_u8(self.handle, x.ctypes.data, x.shape[0], slot), "rn_submit_u8")
        self._slot_n = getattr(self, "_slot_n", {})
        self._slot_n[slot] = x.shape[0]

    def collect(self, slot: int) -> Tuple[np.ndarray, np.ndarray]:
        """Wait for the batch in `slot` and return ``(ids, probs)`` (``rn_collect``)."""
        n = getattr(self, "_slot_n", {}).get(slot, 0)
        probs = np.empty((max(n, 1), self.graph.num_classes), np.float32)
        ids = np.empty((max(n, 1),), np.int64)
        _check(self.lib, self.lib.rn_collect(self.handle, slot, probs.ctypes.data, ids.ctypes.data), "rn_collect")
        return ids[:n], probs[:n]

    def set_stream(self, hip_stream: Optional[int]) -> None:
        """Run on the given hipStream_t handle; ``None`` restores the engine's own (non-blocking) stream; ``0`` selects
        the HIP null stream (what ``torch.cuda.current_stream().cuda_stream`` is when no stream context is active)."""
        if hip_stream is None:
            _check(self.lib, self.lib.rn_set_stream(self.handle, C.c_void_p(0)), "rn_set_stream")
        elif hip_stream == 0:
            _check(self.lib, self.lib.rn_set_stream_null(self.handle), "rn_set_stream_null")
        else:
            _check(self.lib, self.lib.rn_set_stream(self.handle, C.c_void_p(hip_stream)), "rn_set_stream")

    # -- device memory helpers
    def device_malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _check(self.lib, self.lib.rn_device_malloc(self.handle, nbytes, C.byref(p)), "rn_device_malloc")
        return int(p.value)

    def device_free(self, ptr: int) -> None:
        _check(self.lib, self.lib.rn_device_free(self.handle, C.c_void_p(ptr)), "rn_device_free")

    def h2d(self, d_dst: int, src: np.ndarray) -> None:
        a = np.ascontiguousarray(src)
        _check(self.lib, self.lib.rn_memcpy_h2d(self.handle, C.c_void_p(d_dst), a.ctypes.data, a.nbytes),
               "rn_memcpy_h2d")

    def d2h(self, dst: np.ndarray, d_src: int) -> None:
        assert dst.flags["C_CONTIGUOUS"]
        _check(self.lib, self.lib.rn_memcpy_d2h(self.handle, dst.ctypes.data, C.c_void_p(d_src), dst.nbytes),
               "rn_memcpy_d2h")

    # -- introspection
    def nodes(self) -> Dict[str, Tuple[int, Tuple[int, int, int]]]:
        if self._nodes is None:
            out = {}
            for i in range(self.lib.rn_node_count(self.handle)):
                info = rn_node_info()
                _check(self.lib, self.lib.rn_node_info_get(self.handle, i, C.byref(info)), "rn_node_info_get")
                out[info.name.decode()] = (i, (info.h, info.w, info.c))
            self._nodes = out
        return self._nodes

    def tap(self, name: str, n: int) -> np.ndarray:
        nid, (h, w, c) = self.nodes()[name]
        out = np.empty((n, h, w, c), np.float32)
        got = C.c_size_t()
        _check(self.lib, self.lib.rn_tap(self.handle, nid, out.ctypes.data, out.size, C.byref(got)), "rn_tap")
        if got.value != out.size:
            raise RoomNetLibraryError("rn_tap(%s): expected %d elements, library has %d" % (name, out.size, got.value))
        if h == 1 and w == 1:
            return out.reshape(n, c)
        return out

    def frozen_info(self) -> Dict[str, int]:
        """What rn_create folded on this handle (``rn_frozen_info``): channels of the first 32 -> 32 stage's output (16-bit
        handles: the fused pair's on-chip tensor) that are provably constant and not convolved / not contracted by the next
        stage, how many were proven, the residual stage whose frozen first-BN channels are folded and how many of its 16-cout
        quarters still run their convolution."""
        info = (C.c_int * 4)(0, 0, -1, 4)
        if hasattr(self.lib, "rn_frozen_info"):      # (older libraries loaded as A/B arms fold nothing)
            _check(self.lib, self.lib.rn_frozen_info(self.handle, info), "rn_frozen_info")
        return {"pair_channels_not_convolved": info[0], "pair_channels_proven_frozen": info[1], "residual_stage_folded": info[2],
                "residual_stage_live_quarters": info[3]}

    def const_info(self) -> Dict[str, int]:
        """Constant channels nobody computes on this handle (``rn_const_info``): the conv stage whose last 16 output channels
        are constants in the handle's 16-bit store (written once at rn_create), how many of its channels were proven so, how
        many are folded, and how many input channels the stage behind it still contracts."""
        info = (C.c_int * 4)(-1, 0, 0, 0)
        if hasattr(self.lib, "rn_const_info"):       # (older libraries loaded as A/B arms fold nothing)
            _check(self.lib, self.lib.rn_const_info(self.handle, info), "rn_const_info")
        return {"stage": info[0], "channels_proven_constant": info[1], "channels_not_convolved": info[2],
                "next_stage_input_channels": info[3]}

    def bn_batch_stats(self) -> Dict[str, Tuple[np.ndarray, np.ndarray, int]]:
        """The batch moments of the last forward call on a ``batch_stats`` engine (``rn_bn_batch_stats``):
        ``{bn_variable_prefix: (mean float32[c], var_biased float32[c], count)}`` in the reference's variable order
        ``batch_normalization``, ``batch_normalization_1``, ... (count = n * h * w of the BN's input; n for the dense BNs)."""
        n = self.lib.rn_bn_count(self.handle)
        _check(self.lib, min(n, 0), "rn_bn_count")
        out = {}
        for i in range(n):
            info = rn_node_info()
            _check(self.lib, self.lib.rn_bn_info(self.handle, i, C.byref(info)), "rn_bn_info")
            mean, var = np.empty(info.c, np.float32), np.empty(info.c, np.float32)
            count = C.c_int64(0)
            _check(self.lib, self.lib.rn_bn_batch_stats(self.handle, i, mean.ctypes.data, var.ctypes.data, C.byref(count)),
                   "rn_bn_batch_stats")
            out["batch_normalization" if i == 0 else "batch_normalization_%d" % i] = (mean, var, int(count.value))
        return out

    def bn_nodes(self) -> List[str]:
        """Output node of every BN of a ``batch_stats`` engine, in the order of ``bn_batch_stats`` (``rn_bn_info``)."""
        n = self.lib.rn_bn_count(self.handle)
        _check(self.lib, min(n, 0), "rn_bn_count")
        names = []
        for i in range(n):
            info = rn_node_info()
            _check(self.lib, self.lib.rn_bn_info(self.handle, i, C.byref(info)), "rn_bn_info")
            names.append(info.name.decode())
        return names

    def set_profiling(self, enable: bool) -> None:
        _check(self.lib, self.lib.rn_set_profiling(self.handle, 1 if enable else 0), "rn_set_profiling")

    def timing(self) -> Dict[str, object]:
        t = rn_stage_ms()
        _check(self.lib, self.lib.rn_timing(self.handle, C.byref(t)), "rn_timing")
        return {"preprocess_ms": t.preprocess_ms, "stage_ms": [t.stage_ms[i] for i in range(t.n_stages)],
                "head_ms": t.head_ms, "total_ms": t.total_ms}

    def dominant_stage(self) -> int:
        return int(self.lib.rn_dominant_stage(self.handle))

    def launch_groups(self):
        """Conv stages grouped by launch: [[0], [1], [2, 3], [4], ...] when stages 2 and 3 run as one kernel.  A group's
        time is reported under its last stage in `timing()["stage_ms"]`."""
        groups = {}
        for i in range(len(self.graph.stages)):
            rep = int(self.lib.rn_stage_launch(self.handle, i))
            if rep < 0:
                raise RoomNetLibraryError(self.lib.rn_last_error().decode())
            groups.setdefault(rep, []).append(i)
        return [groups[k] for k in sorted(groups)]


class Views:
    """A resident training set of ``Engine.views_create``: the photographs' pixels in one device allocation and the ``rn_views``
    table over them.  ``shapes``: ``(height, width)`` of every photograph; ``nbytes``: the size of the pixel allocation."""

    def __init__(self, engine: "Engine", handle: C.c_void_p, d_pixels: int, shapes, nbytes: int):
        self.engine, self._v, self.d_pixels, self.shapes, self.nbytes = engine, handle, d_pixels, list(shapes), int(nbytes)
        self.n_items = len(self.shapes)

    @property
    def handle(self) -> C.c_void_p:
        if not self._v:
            raise RoomNetLibraryError("the views are closed")
        return self._v

    def close(self) -> None:
        if getattr(self, "_v", None):
            self.engine.lib.rn_views_destroy(self._v)
            self._v = None
            if getattr(self.engine, "_h", None):
                self.engine.device_free(self.d_pixels)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Trainer:
    """One rn_ft: float32 master copies of the last two conv stages and the dense head, Adam slots and the step counter on one
    GPU (include/roomnet_hip.h: fine-tuning).  Trains on features that stay resident in device memory: ``upload`` the
    ``[n_items, side, side, 16]`` float32 features of ``Engine.features_u8`` and the int32 labels once, then ``run``.
    ``depth=3`` (``rn_ft_create_depth``) trains the whole last conv block, stage 7 included, on the ``[n_items, side, side, 128]``
    features of ``Engine.features_u8(..., depth=3)``: 1.08 MB per image at 224 against 28 KB at depth 2.
    ``dropout_rate`` in ``[0, 1)`` and ``dropout_seed`` (``rn_ft_set_dropout``) switch on dropout at every site at or behind the cached
    feature (``finetune.dropout_sites``); the dropout behind the frozen stages upstream of the cache cannot be applied to cached
    features.  ``eval`` never drops."""

    def __init__(self, graph: Graph, weights: Dict[str, np.ndarray], device: int = 0, max_batch: int = 64, learn_rate: float = 1e-4,
                 num_steps: int = 10000, start_step: int = 0, l2_coeff: float = 1e-2, decay_rate: float = 0.068,
                 beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8, lib_path: Optional[str] = None,
                 depth: int = 2, dropout_rate: float = 0.0, dropout_seed: int = 0):
        self.lib = load_library(lib_path)
        self.graph = graph
        self.depth = int(depth)
        self.max_batch = int(max_batch)
        packed = _Packed(graph, weights)
        cfg = rn_ft_config(learn_rate, decay_rate, int(num_steps), int(start_step), l2_coeff, beta1, beta2, epsilon)
        h = C.c_void_p()
        self._h = None
        if self.depth == 2:
            _check(self.lib, self.lib.rn_ft_create(C.byref(packed.w), int(device), self.max_batch, C.byref(cfg), C.byref(h)),
                   "rn_ft_create")
        else:
            _check(self.lib, self.lib.rn_ft_create_depth(C.byref(packed.w), int(device), self.max_batch, C.byref(cfg), self.depth,
                                                         C.byref(h)), "rn_ft_create_depth")
        self._h = h
        self._vars: Optional[List[Tuple[str, int]]] = None
        if dropout_rate or dropout_seed:
            try:
                self.set_dropout(dropout_rate, dropout_seed)
            except Exception:
                self.close()
                raise

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.rn_ft_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise RoomNetLibraryError("trainer is closed")
        return self._h

    def upload(self, a: np.ndarray) -> int:
        """Copy an array into device memory the trainer owns (``rn_ft_upload``); returns the device pointer."""
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        _check(self.lib, self.lib.rn_ft_upload(self.handle, a.ctypes.data, a.nbytes, C.byref(p)), "rn_ft_upload")
        return int(p.value)

    def free(self, d_ptr: int) -> None:
        _check(self.lib, self.lib.rn_ft_free(self.handle, C.c_void_p(d_ptr)), "rn_ft_free")

    def run(self, d_feats: int, d_labels: int, n_items: int, d_index: int, batch: int, steps: int) -> np.ndarray:
        """``steps`` Adam steps on device-resident features, labels and ``[steps, batch]`` int32 indices (``rn_ft_run``); returns each
        step's loss (before its update) as float32 ``[steps]``."""
        losses = np.empty((max(int(steps), 1),), np.float32)
        _check(self.lib, self.lib.rn_ft_run(self.handle, C.c_void_p(d_feats), C.c_void_p(d_labels), int(n_items), C.c_void_p(d_index),
                                            int(batch), int(steps), losses.ctypes.data), "rn_ft_run")
        return losses[:steps]

    def run_host(self, feats: np.ndarray, labels, index, batch: Optional[int] = None) -> np.ndarray:
        """``run`` for host arrays: uploads them, runs ``index.shape[0]`` steps, frees them."""
        feats = np.ascontiguousarray(feats, np.float32)
        index = np.ascontiguousarray(index, np.int32)
        if index.ndim == 1:
            index = index.reshape(-1, int(batch))
        d = [self.upload(feats), self.upload(np.ascontiguousarray(labels, np.int32)), self.upload(index)]
        try:
            return self.run(d[0], d[1], feats.shape[0], d[2], index.shape[1], index.shape[0])
        finally:
            for p in d:
                self.free(p)

    def val_points(self, steps: int, val_every: int) -> np.ndarray:
        """The global steps at which ``run_validated(..., steps, ..., val_every)`` would validate from the trainer's current step
        (``rn_ft_val_points``; ``finetune.validation_steps`` states the same): int64 ``[points]``."""
        n = self.lib.rn_ft_val_points(self.handle, int(steps), int(val_every), None, 0)
        _check(self.lib, min(n, 0), "rn_ft_val_points")
        out = np.empty((n,), np.int64)
        _check(self.lib, min(self.lib.rn_ft_val_points(self.handle, int(steps), int(val_every), out.ctypes.data, n), 0),
               "rn_ft_val_points")
        return out

    def run_validated(self, d_feats: int, d_labels: int, n_items: int, d_index: int, batch: int, steps: int, d_val_feats: int,
                      d_val_labels: int, n_val: int, val_every: int):
        """``run`` with the device-resident validation set ``d_val_feats`` / ``d_val_labels`` evaluated on the GPU every
        ``val_every`` global steps and after the last step, inside the run's one synchronisation (``rn_ft_run_validated``).
        Returns ``(losses float32 [steps], point_steps int64 [points], val_losses float32 [points], confusion int32 [points, C, C])``;
        confusion: row = label, column = predicted class.  The best point so far is kept on the trainer (``best``,
        ``read(RN_FT_BEST)``)."""
        nc = self.graph.num_classes
        points = self.val_points(steps, val_every)
        losses = np.empty((int(steps),), np.float32)
        val_losses = np.empty((points.size,), np.float32)
        confusion = np.empty((points.size, nc, nc), np.int32)
        _check(self.lib, self.lib.rn_ft_run_validated(
            self.handle, C.c_void_p(d_feats), C.c_void_p(d_labels), int(n_items), C.c_void_p(d_index), int(batch), int(steps),
            losses.ctypes.data, C.c_void_p(d_val_feats), C.c_void_p(d_val_labels), int(n_val), int(val_every), val_losses.ctypes.data,
            confusion.ctypes.data), "rn_ft_run_validated")
        return losses, points, val_losses, confusion

    def run_views(self, engine: "Engine", views: "Views", d_labels: int, d_index: int, batch: int, steps: int, seed: int = 0,
                  crop: bool = True, flip: bool = True, d_val_feats: Optional[int] = None, d_val_labels: Optional[int] = None,
                  n_val: int = 0, val_every: Optional[int] = None):
        """``steps`` Adam steps on fresh views (``rn_ft_run_views``): every step ``engine`` makes the minibatch's views of the resident
        photographs ``views`` at the trainer's global step (``seed``, ``crop``, ``flip``: ``finetune.view_draw``) and runs its trunk
        into a feature slot the trainer reads.  ``d_labels`` ``[n_items]`` and ``d_index`` ``[steps, batch]`` are device int32 (e.g.
        of ``upload``).  ``engine``'s weights being this trainer's frozen trunk is the caller's contract.  Returns the losses, or with
        ``val_every`` (and the cached validation features ``d_val_feats``, ``d_val_labels``, ``n_val``) what ``run_validated``
        returns."""
        flags = (RN_VIEW_CROP if crop else 0) | (RN_VIEW_FLIP if flip else 0)
        losses = np.empty((max(int(steps), 1),), np.float32)
        head = (self.handle, engine.handle, views.handle, C.c_void_p(d_labels), int(views.n_items), C.c_void_p(d_index), int(batch),
                int(steps), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), flags, losses.ctypes.data)
        if val_every is None:
            _check(self.lib, self.lib.rn_ft_run_views(*head, None, None, 0, 0, None, None), "rn_ft_run_views")
            return losses[:steps]
        nc = self.graph.num_classes
        points = self.val_points(steps, val_every)
        val_losses = np.empty((points.size,), np.float32)
        confusion = np.empty((points.size, nc, nc), np.int32)
        _check(self.lib, self.lib.rn_ft_run_views(*head, C.c_void_p(d_val_feats), C.c_void_p(d_val_labels), int(n_val), int(val_every),
                                                  val_losses.ctypes.data, confusion.ctypes.data), "rn_ft_run_views")
        return losses[:steps], points, val_losses, confusion

    def best(self) -> Tuple[int, int, int]:
        """``(step, correct, n_val)`` of the best validation point so far on this trainer (``rn_ft_best``): the earliest point with
        the most correct predictions.  Raises ``RoomNetLibraryError`` before any point has been taken."""
        step, correct, n_val = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _check(self.lib, self.lib.rn_ft_best(self.handle, C.byref(step), C.byref(correct), C.byref(n_val)), "rn_ft_best")
        return int(step.value), int(correct.value), int(n_val.value)

    def eval(self, d_feats: int, n: int, d_labels: Optional[int] = None):
        """Forward only from the current parameters (``rn_ft_eval``): ``(mean_loss or None, probs [n, C], ids [n])``."""
        probs = np.empty((n, self.graph.num_classes), np.float32)
        ids = np.empty((n,), np.int64)
        loss = C.c_float(0)
        _check(self.lib, self.lib.rn_ft_eval(self.handle, C.c_void_p(d_feats), C.c_void_p(d_labels) if d_labels else None, int(n),
                                             C.byref(loss) if d_labels else None, probs.ctypes.data, ids.ctypes.data), "rn_ft_eval")
        return (float(loss.value) if d_labels else None), probs, ids

    def eval_host(self, feats: np.ndarray, labels=None):
        feats = np.ascontiguousarray(feats, np.float32)
        d = [self.upload(feats)] + ([self.upload(np.ascontiguousarray(labels, np.int32))] if labels is not None else [])
        try:
            return self.eval(d[0], feats.shape[0], d[1] if labels is not None else None)
        finally:
            for p in d:
                self.free(p)

    def variables(self) -> List[Tuple[str, int]]:
        """``[(checkpoint name, element count)]`` of the trained variables, in the trainer's order (``rn_ft_var_info``)."""
        if self._vars is None:
            n = self.lib.rn_ft_var_count(self.handle)
            _check(self.lib, min(n, 0), "rn_ft_var_count")
            out = []
            for i in range(n):
                name, cnt = C.create_string_buffer(64), C.c_int64(0)
                _check(self.lib, self.lib.rn_ft_var_info(self.handle, i, name, 64, C.byref(cnt)), "rn_ft_var_info")
                out.append((name.value.decode(), int(cnt.value)))
            self._vars = out
        return self._vars

    def read(self, what: int = RN_FT_PARAM) -> Dict[str, np.ndarray]:
        """Every trained variable's parameters, last gradient or Adam slot, or (``RN_FT_BEST``) its parameters at the best validation
        point (``rn_ft_read``), in its checkpoint shape."""
        shapes = self.graph.variable_shapes()
        out = {}
        for i, (name, cnt) in enumerate(self.variables()):
            a = np.empty((cnt,), np.float32)
            _check(self.lib, self.lib.rn_ft_read(self.handle, int(what), i, a.ctypes.data, a.size), "rn_ft_read")
            out[name] = a.reshape(shapes[name])
        return out

    def step_count(self) -> int:
        return int(self.lib.rn_ft_step_count(self.handle))

    def set_dropout(self, rate: float, seed: int = 0) -> None:
        """Dropout from the next ``run`` on (``rn_ft_set_dropout``): ``rate`` in ``[0, 1)``, 0 switches it off; ``seed``: 64 bits."""
        _check(self.lib, self.lib.rn_ft_set_dropout(self.handle, C.c_float(rate), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)),
               "rn_ft_set_dropout")

    def dropout(self) -> Tuple[float, int]:
        """``(rate, seed)`` as set (``rn_ft_dropout``); ``(0.0, 0)`` on a new trainer."""
        rate, seed = C.c_float(0), C.c_uint64(0)
        _check(self.lib, self.lib.rn_ft_dropout(self.handle, C.byref(rate), C.byref(seed)), "rn_ft_dropout")
        return float(rate.value), int(seed.value)

    def dropout_mask(self, site: int, step: int, slot: int, count: int) -> np.ndarray:
        """The keep mask (uint8 ``[count]``, 0 or 1) that global step ``step`` would use for the first ``count`` elements of ``site``
        in minibatch slot ``slot``, computed on the device (``rn_ft_dropout_mask``); ``finetune.dropout_keep`` states the same."""
        keep = np.empty((max(int(count), 1),), np.uint8)
        _check(self.lib, self.lib.rn_ft_dropout_mask(self.handle, int(site), int(step), int(slot), int(count), keep.ctypes.data),
               "rn_ft_dropout_mask")
        return keep[:count]

    def last_run_ms(self) -> float:
        """Device time of the last ``run``'s step loop (``rn_ft_last_run_ms``)."""
        ms = C.c_float(0)
        _check(self.lib, self.lib.rn_ft_last_run_ms(self.handle, C.byref(ms)), "rn_ft_last_run_ms")
        return float(ms.value)


class PinnedArray:
    """A NumPy array over page-locked host memory (``rn_host_alloc``): uploads out of it are asynchronous DMAs, so the
    two-slot pipeline (``Engine.submit_u8`` / ``collect``) hides them behind the previous batch's kernels.  Fill
    ``.array`` in place; ``close()`` (or garbage collection) frees the memory -- do not use ``.array`` afterwards."""

    def __init__(self, shape, dtype=np.uint8, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        _check(self.lib, self.lib.rn_host_alloc(max(nbytes, 1), C.byref(p)), "rn_host_alloc")
        self._p = p
        buf = (C.c_uint8 * max(nbytes, 1)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self) -> None:
        if self._p:
            self.array = None
            self.lib.rn_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def group_plan(n: int, ndev: int, max_batch_per_device: int, num_classes: int = 6, lib_path: Optional[str] = None):
    """``rn_group_plan``: (counts, offsets, slot_bytes) of an n-image call on ndev devices -- no GPU needed."""
    lib = load_library(lib_path)
    counts, offsets, slot = (C.c_int * ndev)(), (C.c_int * ndev)(), C.c_size_t(0)
    _check(lib, lib.rn_group_plan(n, ndev, max_batch_per_device, num_classes, counts, offsets, C.byref(slot)), "rn_group_plan")
    return list(counts), list(offsets), int(slot.value)


def occlusion_plan(side: int, patch: int, stride: int, n: int, max_batch: int, lib: Optional[C.CDLL] = None) -> Tuple[int, int, int]:
    """``rn_occlusion_plan``: (G, n_windows, n_chunks) of an n-image occlusion call -- no GPU needed."""
    lib = lib or load_library()
    g, nw, nc = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib, lib.rn_occlusion_plan(side, patch, stride, n, max_batch, C.byref(g), C.byref(nw), C.byref(nc)), "rn_occlusion_plan")
    return int(g.value), int(nw.value), int(nc.value)


def faith_plan(side: int, steps: int, modes, n: int, max_batch: int, lib: Optional[C.CDLL] = None) -> Tuple[int, int]:
    """``rn_faith_plan``: (n_passes, n_chunks) of an n-image deletion / insertion call -- no GPU needed.  ``modes``: the bit mask
    (1 deletion, 2 insertion, 3 both)."""
    lib = lib or load_library()
    npass, nc = C.c_int(0), C.c_int(0)
    _check(lib, lib.rn_faith_plan(side, steps, int(modes), n, max_batch, C.byref(npass), C.byref(nc)), "rn_faith_plan")
    return int(npass.value), int(nc.value)


def faith_rank_model(maps: np.ndarray, lib: Optional[C.CDLL] = None) -> np.ndarray:
    """``rn_faith_rank_model``: the ranks of ``[n, npix]`` float32 maps by the rank kernel's own steps on the host -- no GPU needed."""
    lib = lib or load_library()
    maps = np.ascontiguousarray(maps, dtype=np.float32)
    if maps.ndim != 2:
        raise ValueError("faith_rank_model: expected [n, npix] maps, got %s" % (maps.shape,))
    rank = np.empty(maps.shape, np.uint32)
    _check(lib, lib.rn_faith_rank_model(maps.ctypes.data, maps.shape[0], maps.shape[1], rank.ctypes.data), "rn_faith_rank_model")
    return rank


# launch families of rn_band_plan (include/roomnet_hip.h: RN_BANDS_*)
BAND_FAMILIES = {"stage0": 0, "generic": 1, "pair": 2, "conv16": 3, "conv16p": 4, "rowreg": 5, "rw": 6, "f32m": 7}


def band_plan(family, n: int, n_cu: int, out_side: int, n_colblocks: int, wgs_per_cu: int = 1, pool_k: int = 0, pool_s: int = 1,
              lib_path: Optional[str] = None) -> Tuple[int, int]:
    """``rn_band_plan``: (rows_per_band, n_bands) the forward pass chooses for a launch of ``family`` -- no GPU needed."""
    lib = load_library(lib_path)
    fam = BAND_FAMILIES[family] if isinstance(family, str) else int(family)
    rows, bands = C.c_int(0), C.c_int(0)
    _check(lib, lib.rn_band_plan(fam, n, n_cu, out_side, n_colblocks, wgs_per_cu, pool_k, pool_s, C.byref(rows), C.byref(bands)), "rn_band_plan")
    return int(rows.value), int(bands.value)


# kernel kinds of rn_f32m_plan (include/roomnet_hip.h: RN_F32M_*)
F32M_KINDS = ("off", "wide", "m16")


def f32m_plan(cin: int, cout: int, pool_k: int, pool_s: int, residual: bool, in_side: int, out_side: int, live_cin: Optional[int] = None,
              frozen_couts: int = 0, lib_path: Optional[str] = None) -> Dict[str, object]:
    """``rn_f32m_plan``: what a float32 handle decides for a conv stage of this shape (kernel kind, variant, launch geometry,
    dynamic LDS) -- no GPU needed."""
    lib = load_library(lib_path)
    p = rn_f32m_stage_plan()
    _check(lib, lib.rn_f32m_plan(cin, cout, pool_k, pool_s, int(residual), in_side, out_side, cin if live_cin is None else live_cin, frozen_couts,
                                 C.byref(p)), "rn_f32m_plan")
    out = {name: int(getattr(p, name)) for name, _ in rn_f32m_stage_plan._fields_}
    out["kind"] = F32M_KINDS[out["kind"]]
    return out


class Group:
    """One rn_group: the model replicated on several GPUs of this process, batches sharded contiguously, one RCCL
    all-gather of the packed results (the C ABI's multi-GPU entry, include/roomnet_hip.h)."""

    def __init__(self, graph: Graph, weights: Dict[str, np.ndarray], devices: Sequence[int], dtype="bf16",
                 max_batch_per_device: int = 64, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        self.graph = graph
        self.devices = [int(d) for d in devices]
        self.cap = int(max_batch_per_device)
        packed = _Packed(graph, weights)
        dt = DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
        devs = (C.c_int * len(self.devices))(*self.devices)
        g = C.c_void_p()
        rc = self.lib.rn_group_create(C.byref(packed.w), len(self.devices), devs, dt, self.cap, 0, C.byref(g))
        _check(self.lib, rc, "rn_group_create")
        self._g = g

    def forward_u8(self, bgr_nhwc: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        s = self.graph.im_side
        x = np.ascontiguousarray(bgr_nhwc, dtype=np.uint8)
        if x.ndim != 4 or x.shape[1:] != (s, s, 3):
            raise ValueError("expected uint8 [n,%d,%d,3], got %s" % (s, s, x.shape))
        n = x.shape[0]
        probs = np.empty((n, self.graph.num_classes), np.float32)
        ids = np.empty((n,), np.int64)
        step = self.cap * len(self.devices)
        for i in range(0, n, step):
            m = min(step, n - i)
            rc = self.lib.rn_group_forward_u8(self._g, x[i:i + m].ctypes.data, m, probs[i:i + m].ctypes.data,
                                              ids[i:i + m].ctypes.data)
            _check(self.lib, rc, "rn_group_forward_u8")
        return ids, probs

    def close(self) -> None:
        if self._g:
            self.lib.rn_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
