"""ctypes binding of libmi355vision.so (include/mi355vision.h) -- the only way the Python layer computes.

There is deliberately no CPU or PyTorch fallback: if the library is missing, cannot be loaded, or is
handed a tensor that does not live on a HIP device, the call raises.  PyTorch is used for device
memory, streams and dtype plumbing only.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import sys
from pathlib import Path
from typing import Optional, Sequence

import torch

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("MI355VISION_LIB", _HERE / "lib" / "libmi355vision.so"))

BORDER_VALID, BORDER_REFLECT, BORDER_ZERO = 0, 1, 2
BORDERS = {"valid": BORDER_VALID, "reflect": BORDER_REFLECT, "zero": BORDER_ZERO, "zeros": BORDER_ZERO}
MAX_HOST_TAPS_2D = 121
MAX_TAPS_1D = 63

# every symbol include/mi355vision.h declares: (name, restype, argtypes)
_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
SYMBOLS = {
    "mv_abi_version": (_i, []),
    "mv_last_error": (C.c_char_p, []),
    "mv_last_kernel": (C.c_char_p, []),
    "mv_build_id": (C.c_char_p, []),
    "mv_device_count": (_i, []),
    "mv_depthwise_conv2d_f32": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _i, _i, _i, _vp]),
    "mv_depthwise_conv2d_u8": (_i, [_vp, _vp, _vp, _i, _i64, _i, _i, _i, _i, _i, _vp]),
    "mv_gaussian_blur_f32": (_i, [_vp, _vp, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_gaussian_blur_u8": (_i, [_vp, _vp, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_gaussian_blur_u8_workspace_bytes": (_i64, [_i64, _i, _i, _i, _i]),
    "mv_gaussian_blur_u8_ws": (_i, [_vp, _vp, _i64, _i, _i, _fp, _i, _fp, _i, _vp, _i64, _vp]),
    "mv_separable_blur_f32": (_i, [_vp, _vp, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_gaussian_blur_f16": (_i, [_vp, _vp, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_gaussian_blur_bf16": (_i, [_vp, _vp, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_gaussian_blur_f64": (_i, [_vp, _vp, _i64, _i, _i, C.POINTER(C.c_double), _i, C.POINTER(C.c_double), _i, _vp]),
    "mv_depthwise_conv2d_f64": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _vp]),
    "mv_sharpness_f64": (_i, [_vp, _vp, _i64, _i, _i, _d, _i, _vp]),
    "mv_gaussian_blur_f32_v": (_i, [_vp, _vp, _i, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_gaussian_blur_u8_v": (_i, [_vp, _vp, _i, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_separable_blur_f32_v": (_i, [_vp, _vp, _i, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_separable_blur_u8_v": (_i, [_vp, _vp, _i, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_sharpness_f32_v": (_i, [_vp, _vp, _i, _i64, _i, _i, _d, _i, C.c_float, _i, _vp]),
    "mv_sharpness_u8_v": (_i, [_vp, _vp, _i, _i64, _i, _i, _d, _i, _vp]),
    "mv_conv1x1_k_slices": (_i, [_i64, _i, _i, _i, _i, C.POINTER(C.c_int)]),
    "mv_separable_blur_u8": (_i, [_vp, _vp, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_sobel_f32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "mv_gaussian_sobel_f32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _fp, _i, _fp, _i, _vp]),
    "mv_sharpness_f32": (_i, [_vp, _vp, _i64, _i, _i, _d, _i, C.c_float, _i, _vp]),
    "mv_sharpness_u8": (_i, [_vp, _vp, _i64, _i, _i, _d, _i, _vp]),
    "mv_conv3x3_bias_relu_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _vp]),
    "mv_to_float_normalize_u8": (_i, [_vp, _vp, _i64, _i, _i64, _fp, _fp, _vp]),
    "mv_normalize_f32": (_i, [_vp, _vp, _i64, _i, _i64, _fp, _fp, _vp]),
    "mv_conv3x3_bias_relu_u8norm_f32": (_i, [_vp, _fp, _fp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "mv_linear_bias_relu_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "mv_linear_k_slices": (_i, [_i64, _i, _i, C.POINTER(C.c_int)]),
    "mv_linear_workspace_bytes": (_i64, [_i64, _i, _i]),
    "mv_linear_bias_relu_ws_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _i64, _vp]),
    "mv_conv_norm_act_f32": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "mv_conv1x1_upsample_add_f32": (_i, [_vp] * 7 + [_i64] + [_i] * 8 + [_vp]),
    "mv_inverted_residual_k_slices": (_i, [_i64, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int)]),
    "mv_inverted_residual_workspace_bytes": (_i64, [_i64, _i, _i, _i, _i, _i, _i]),
    "mv_inverted_residual_f32": (_i, [_vp] * 10 + [_i, _vp, _i64] + [_i] * 7 + [_vp, _i64, _vp]),
    "mv_fold_batchnorm": (None, [_fp, _fp, _fp, _fp, C.c_double, _i, _fp, _fp]),
    "mv_deform_conv2d_workspace_bytes": (_i64, [_i64] + [_i] * 11),
    "mv_conv3x3_k_slices": (_i, [_i64, _i, _i, _i, _i, _vp]),
    "mv_conv3x3_workspace_bytes": (_i64, [_i64, _i, _i, _i, _i]),
    "mv_conv3x3_bias_relu_ws_f32": (_i, [_vp] * 4 + [_i64] + [_i] * 5 + [_vp, _i64, _vp]),
    "mv_deform_conv2d_needs_workspace": (_i, [_i64] + [_i] * 14),
    "mv_deform_conv2d_f32": (_i, [_vp] * 6 + [_i64] + [_i] * 15 + [_vp, _i64, _vp]),
    "mv_conv2d_needs_workspace": (_i, [_i64] + [_i] * 13),
    "mv_conv2d_bias_act_f32": (_i, [_vp] * 4 + [_i64] + [_i] * 14 + [_vp, _i64, _vp]),
    "mv_maxpool2d_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "mv_conv2d_affine_act_f32": (_i, [_vp] * 7 + [_i64] + [_i] * 15 + [_vp, _i64, _vp]),
    "mv_maxpool2d_pad_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _vp]),
    "mv_maxpool2d_ceil_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _vp]),
    "mv_resize_workspace_bytes": (_i64, [_i64, _i, _i, _i, _i, _i, _i, _i, _i]),
    "mv_resize_bilinear_aa_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
    "mv_resize_bilinear_aa_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
    "mv_preset_classification_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _vp, _i64, _vp]),
    "mv_preset_classification_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _vp, _i64, _vp]),
    "mv_maxpool2x2_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp]),
    "mv_adaptive_avgpool_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "mv_elastic_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _i64, _i64, _i64, _i, _fp, _vp]),
    "mv_elastic_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _i64, _i64, _i64, _i, _fp, _vp]),
    "mv_warp_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _fp, _i, _i, _i, _fp, _vp]),
    "mv_warp_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _fp, _i, _i, _i, _fp, _vp]),
    "mv_color_workspace_bytes": (_i64, [_i64, _i, _i, _i]),
    "mv_color_chain_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_double), _i, _i, _vp, _i64, _vp]),
    "mv_color_chain_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_double), _i, _i, _vp, _i64, _vp]),
    "mv_rgb_to_grayscale_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "mv_rgb_to_grayscale_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "mv_pointwise_f32": (_i, [_vp, _vp, _i64, _i, _d, _vp]),
    "mv_pointwise_u8": (_i, [_vp, _vp, _i64, _i, _d, _vp]),
    "mv_autocontrast_workspace_bytes": (_i64, [_i64, _i, _i, _i]),
    "mv_autocontrast_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _vp]),
    "mv_autocontrast_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _vp]),
    "mv_equalize_workspace_bytes": (_i64, [_i64, _i, _i, _i]),
    "mv_equalize_f32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _vp]),
    "mv_equalize_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i64, _vp]),
    "mv_resized_crop_u8": (_i, [_vp, _vp, _i64] + [_i] * 10 + [_vp, _i64, _vp]),
    "mv_resized_crop_f32": (_i, [_vp, _vp, _i64] + [_i] * 10 + [_vp, _i64, _vp]),
    "mv_resized_crop_preset_u8": (_i, [_vp, _vp, _i64] + [_i] * 12 + [_fp, _fp, _vp, _i64, _vp]),
    "mv_resized_crop_preset_f32": (_i, [_vp, _vp, _i64] + [_i] * 12 + [_fp, _fp, _vp, _i64, _vp]),
    "mv_pad_crop_flip": (_i, [_vp, _vp, _i64] + [_i] * 11 + [_vp, _vp]),
    "mv_erase": (_i, [_vp, _vp, _i64] + [_i] * 8 + [_vp, _i, _vp]),
    "mv_mixup_f32": (_i, [_vp, _vp, _i64, _i64, _d, _vp]),
    "mv_mixup_f16": (_i, [_vp, _vp, _i64, _i64, _d, _vp]),
    "mv_mixup_f64": (_i, [_vp, _vp, _i64, _i64, _d, _vp]),
    "mv_cutmix": (_i, [_vp, _vp, _i64, _i64] + [_i] * 7 + [_vp]),
    "mv_mixup_labels_i64": (_i, [_vp, _vp, _i64, _i, _d, _vp]),
    "mv_nms_workspace_bytes": (_i64, [_i64]),
    "mv_nms_f32": (_i, [_vp, _vp, _i64, _d, _vp, _vp, _vp, _i64, _vp]),
    "mv_roi_align_f32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _i64, _i, _i, _d, _i, _i, _vp]),
    "mv_roi_pool_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i64, _i, _i, _d, _vp]),
    "mv_ps_roi_pool_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i64, _i, _i, _d, _vp]),
    "mv_ps_roi_align_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i64, _i, _i, _d, _i, _vp]),
    "mv_multiscale_roi_align_f32": (_i, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), _i, _vp, _vp, _vp, _i64, _i,
                                         _i64, _i, _i, _i, _i, _vp]),
    "mv_box_iou_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _vp]),
    "mv_masks_to_boxes_workspace_bytes": (_i64, [_i64]),
    "mv_masks_to_boxes_u8": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _i64, _vp]),
    "mv_masks_to_boxes_f32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _i64, _vp]),
    "mv_rpn_topk_workspace_bytes": (_i64, [_i64, _ip, _ip, _ip, _i, _i]),
    "mv_rpn_topk_f32": (_i, [_vp, _ip, _ip, _ip, C.POINTER(C.c_int64), _i, _i64, _i, _vp, _vp, _i64, _vp]),
    "mv_rpn_decode_f32": (_i, [_vp, _vp, _ip, _ip, _ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ip, _ip, _i, _vp, _vp, _vp, _i64, _i64]
                          + [_d] * 7 + [_vp] * 5),
    "mv_box_decode_f32": (_i, [_vp, _vp, _vp, _i64, _i] + [_d] * 5 + [_vp]),
    "mv_retinanet_topk_chunk": (_i, []),
    "mv_retinanet_topk_workspace_bytes": (_i64, [_i64, _ip, _ip, _ip, _i, _i, _i]),
    "mv_retinanet_topk_f32": (_i, [_vp, _ip, _ip, _ip, C.POINTER(C.c_int64), _i, _i, _i64, _i, _d, _vp, _vp, _i64, _vp]),
    "mv_retinanet_decode_f32": (_i, [_vp, _vp, _ip, _ip, _ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ip, _ip, _i, _i, _vp, _vp, _vp,
                                     _i64, _i64] + [_d] * 5 + [_vp] * 5),
    "mv_fcos_topk_f32": (_i, [_vp, _vp, _ip, _ip, _ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i, _i, _i64, _i, _d, _vp, _vp, _i64, _vp]),
    "mv_fcos_decode_f32": (_i, [_vp, _vp, _vp, _ip, _ip, _ip] + [C.POINTER(C.c_int64)] * 3 + [_ip, _ip, _i, _i, _vp, _vp, _vp, _i64, _i64]
                           + [_vp] * 5),
    "mv_ssd_scores_f32": (_i, [_vp, _ip, _ip, _ip, C.POINTER(C.c_int64), _i, _i, _i64, _vp, _vp]),
    "mv_ssd_topk_f32": (_i, [_vp, _i64, _i, _i64, _i, _d, _vp, _vp]),
    "mv_ssd_decode_f32": (_i, [_vp, _vp, _ip, _ip, _ip, C.POINTER(C.c_int64), _i, _i, _vp, _fp, _fp, _i, _i, _vp, _vp, _i64, _i64] + [_d] * 5
                          + [_vp] * 5),
    "mv_group_norm_chunk": (_i, []),
    "mv_group_norm_workspace_bytes": (_i64, [_i64, _i, _i, _i, _i]),
    "mv_group_norm_act_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i64, _i64, _d, _i, _vp, _i64, _vp]),
    "mv_l2_normalize_scale_f32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _i64, _i64, _d, _vp]),
    "mv_roi_detections_f32": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i, _i64] + [_d] * 7 + [_vp] * 5),
    "mv_interpolate_bilinear_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "mv_detection_batch_f32": (_i, [_vp, _ip, _ip, _ip, _ip, _i64, _i, _fp, _fp, _vp, _i, _i, _vp]),
    "mv_interpolate_argmax_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _vp]),
    "mv_paste_masks_f32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "mv_mask_probs_f32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "mv_conv_transpose2x2_bias_act_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _vp]),
    "mv_conv_transpose4x4s2_bias_act_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _vp]),
    "mv_heatmaps_to_keypoints_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "mv_dwconv_norm_act_f32": (_i, [_vp] * 7 + [_i64] + [_i] * 7 + [_vp]),
    "mv_global_avgpool_f64sum_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i64, _vp]),
    "mv_linear_act_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "mv_se_scale_f32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "mv_conv1x1_scaled_f32": (_i, [_vp] * 8 + [_i64] + [_i] * 6 + [_vp]),
    "mv_dwconv_dilated_norm_act_f32": (_i, [_vp] * 7 + [_i64] + [_i] * 8 + [_vp]),
    "mv_conv1x1_gated_upsample_f32": (_i, [_vp] * 6 + [_i64] + [_i] * 6 + [_vp]),
    "mv_dwconv3x3_conv1x1_f32": (_i, [_vp] * 11 + [_i64] + [_i] * 9 + [_vp]),
    "mv_dwconv7x7_bias_f32": (_i, [_vp] * 4 + [_i64, _i, _i, _i, _vp]),
    "mv_layer_norm2d_stats_f32": (_i, [_vp] * 3 + [_i64, _i, _i, _i, _d, _vp]),
    "mv_layer_norm2d_f32": (_i, [_vp] * 4 + [_i64, _i, _i, _i, _d, _vp]),
    "mv_conv1x1_ln_gelu_f32": (_i, [_vp] * 8 + [_i64] + [_i] * 5 + [_vp]),
}

_lib: Optional[C.CDLL] = None


class Mi355VisionError(RuntimeError):
    """The native library is missing / failed, or was asked to run off-device."""


def _open(path: Path) -> C.CDLL:
    if not path.exists():
        raise Mi355VisionError(
            f"{path} not found: build it with `python cpu-vision_amd/_build.py` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(str(path))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.mv_abi_version() != 1:
        raise Mi355VisionError(f"ABI version mismatch: library reports {lib.mv_abi_version()}, binding expects 1")
    return lib


def load() -> C.CDLL:
    """Load libmi355vision.so (once).  Raises if it is not built: there is no fallback path."""
    global _lib
    if _lib is None:
        _lib = _open(LIB_PATH)
    return _lib


TUNING_LIB_PATH = _HERE / "lib" / "libmi355vision_tuning.so"


class tuning_library:
    """Context manager for tools/ and for the tests that force an alternative kernel: inside it every call of the
    package goes to the -DMV_TUNING build of the same sources, the only build that reads MV_* environment knobs
    (the product library has no environment lookup at all)."""

    def __init__(self, path: Optional[Path] = None):
        self._path = Path(path) if path else TUNING_LIB_PATH
        self._saved = None

    def __enter__(self) -> C.CDLL:
        global _lib
        self._saved = _lib
        _lib = _open(self._path)
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self._saved
        return False


def last_kernel() -> str:
    """The kernel instantiation the calling thread's last entry point launched (mv_last_kernel)."""
    return load().mv_last_kernel().decode()


def build_id() -> str:
    return load().mv_build_id().decode()


def _raise(rc: int):
    msg = load().mv_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError(msg)
    raise Mi355VisionError(f"libmi355vision error {rc}: {msg}")


def check(rc: int):
    if rc != 0:
        _raise(rc)


def require_device(t: torch.Tensor, what: str = "input") -> None:
    if not t.is_cuda:
        raise Mi355VisionError(
            f"{what} lives on '{t.device}': mi355vision kernels run on the MI355X only and there is no CPU "
            "fallback -- move the tensor to a HIP device (tensor.cuda()).")


def require_f32_u8(image: torch.Tensor, name: str, allow_bool: bool = False) -> None:
    """The dtype gate of the image ops whose kernels exist for float32 and uint8 storage (launch_image_op)."""
    dtype = image.dtype
    if not (dtype is torch.uint8 or dtype is torch.float32 or (allow_bool and dtype is torch.bool)):
        raise NotImplementedError(f"{name}: {image.dtype} images are not on the MI355X path (float32 and uint8 are)")


def max_value(dtype: torch.dtype) -> int:
    """transforms/_functional_tensor.py:41-57"""
    return {torch.uint8: 255, torch.int8: 127, torch.int16: 32767, torch.uint16: 65535, torch.int32: 2147483647,
            torch.int64: 9223372036854775807}.get(dtype, 1)


class _ForwardOnly(torch.autograd.Function):
    """Marks the output of a forward-only kernel: it takes part in autograd (so that nothing downstream silently trains on
    missing gradients) and raises as soon as a backward pass reaches it."""

    @staticmethod
    def forward(ctx, out, what, *deps):
        ctx.what = what
        return out.view_as(out)

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError(
            f"{ctx.what} is forward-only on the MI355X (inference / data-augmentation path): there is no backward kernel. "
            "Run it under torch.no_grad() or on tensors that do not require grad.")


def forward_only(out: torch.Tensor, what: str, *deps) -> torch.Tensor:
    """`out` was computed by a forward-only kernel from `deps`.  When autograd is recording and any of them requires grad,
    return a result whose backward raises (the reference would compute gradients here); otherwise `out` itself."""
    if torch.is_grad_enabled() and any(isinstance(d, torch.Tensor) and d.requires_grad for d in deps):
        return _ForwardOnly.apply(out, what, *[d for d in deps if isinstance(d, torch.Tensor)])
    return out


class _DeviceOf:
    """`with torch.cuda.device(t.device)` only when t is not on the current device (the context manager costs
    ~10 us of host time per call, which matters for launch-bound per-frame use)."""

    __slots__ = ("_ctx",)

    def __init__(self, t: torch.Tensor):
        idx = t.device.index
        self._ctx = None if (idx is None or idx == torch.cuda.current_device()) else torch.cuda.device(t.device)

    def __enter__(self):
        if self._ctx is not None:
            self._ctx.__enter__()

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)
        return False


def on_device_of(t: torch.Tensor) -> _DeviceOf:
    return _DeviceOf(t)


def stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def launch(fn, on: torch.Tensor, *args) -> None:
    """fn(*args, stream) on `on`'s device and its current stream; a non-zero status raises."""
    with on_device_of(on):
        check(fn(*args, stream_ptr(on)))


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def workspace(nbytes: int, device):
    """(buffer, pointer, nbytes) of a uint8 device buffer for a *_ws entry point, (None, None, 0) when it needs none.  The
    caller holds `buffer` until the launch is queued."""
    if not nbytes:
        return None, None, 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws, ws.data_ptr(), nbytes


def columns_workspace_bytes(n: int, per_image: int, cap: int) -> int:
    """Bytes of the im2col columns workspace for a batch of n: whole images, as many as stay below `cap`, one at the least (the
    library then runs the batch in passes of as many images as the workspace holds)."""
    return max(1, min(n, cap // max(per_image, 1))) * per_image


def f32_on(t: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    """An optional tensor as a detached contiguous float32 tensor on `device` (a layer's bias, folded norm, residual ...).
    A tensor that already is one comes back itself: a new tensor object per call is measurable at batch 1."""
    if t is None or (t.device == device and t.dtype == torch.float32 and t.is_contiguous()):
        return t
    return t.detach().to(device, torch.float32).contiguous()


@functools.lru_cache(maxsize=256)
def _uploaded_table(values: tuple, shape: tuple, dtype: torch.dtype, device: str) -> torch.Tensor:
    return torch.tensor(values, dtype=dtype).reshape(shape).to(device)


def table_on(t: torch.Tensor, device, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """A small table a wrapper takes from the host or the device -- cell anchors, image sizes, default-box pairs, a filter's taps --
    as a contiguous `dtype` tensor on `device`, read-only.  One that lies on a device is used as it is (moved, if it lies on
    another).  A host table is uploaded once per distinct contents, shape, dtype and device and cached, as _geometry.py and
    _color.py cache their tables: an upload per call synchronises the stream and cannot be captured into a graph (the first call
    with new contents still uploads: a warm-up outside the capture, as graphs.capture makes)."""
    t = t.detach()
    if t.device.type != "cpu":
        return t.to(device, dtype).contiguous()
    return _uploaded_table(tuple(t.reshape(-1).tolist()), tuple(t.shape), dtype, str(device))


def require_f32_layer(name: str, x: torch.Tensor, weight: torch.Tensor) -> None:
    """The CNN layers compute in float32 only."""
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError(f"{name} computes in float32. Got input {x.dtype}, weight {weight.dtype}")


def launch_xy(fn, image: torch.Tensor, args, *, out_shape=None, out_dtype=None, pair: bool = False):
    """ONE call of fn(x, y, *args, stream) -- the filters, the pools and the preset steps: x the contiguous image, y a fresh
    output of x's shape and dtype unless `out_shape` / `out_dtype` say otherwise.  pair: fn(x, y0, y1, *args, stream) with two
    such outputs, returned as a tuple.  The caller has checked its arguments; a device tensor whose pointer is in `args` lives
    on the image's device, and the caller keeps it alive over this call."""
    require_device(image)
    x = image.contiguous()
    # each case's cheapest binding of the same allocation, as in launch_image_op
    if out_shape is None and out_dtype is None:
        y = torch.empty_like(x)
    else:
        y = torch.empty(out_shape or x.shape, dtype=out_dtype or x.dtype, device=x.device)
    if pair:
        y1 = torch.empty(y.shape, dtype=y.dtype, device=y.device)
        launch(fn, x, x.data_ptr(), y.data_ptr(), y1.data_ptr(), *args)
        return y, y1
    launch(fn, x, x.data_ptr(), y.data_ptr(), *args)
    return y


def launch_frames(fn, frames, args):
    """ONE call of a mv_*_v entry point, fn(xs, ys, n, *args, stream), over separately allocated, equally shaped frames on one
    device (host tables of their pointers); returns views of one output batch."""
    f0 = frames[0]
    xs = [f.contiguous() for f in frames]
    out = torch.empty((len(xs),) + tuple(f0.shape), dtype=f0.dtype, device=f0.device)
    ys = [out[i] for i in range(len(xs))]
    launch(fn, f0, pointer_table(xs), pointer_table(ys), len(xs), *args)
    return ys


def launch_image_op(name: str, image: torch.Tensor, args, *, out_shape=None, workspace=None, allow_bool: bool = False,
                    what: Optional[str] = None, deps=()) -> torch.Tensor:
    """ONE call of mv_<name>_u8 / mv_<name>_f32 (chosen by the storage type) on a non-empty float32 / uint8 image:
    fn(x, y, *args[, workspace, workspace_bytes], stream), x the contiguous image and y a fresh output of `out_shape` (default:
    x's shape).  The caller has checked its arguments and the dtype (require_f32_u8).

      args        the tuple of what the entry point takes between y and the workspace / stream; a device tensor whose pointer is
                  in it lives on the image's device, and the caller keeps it alive over this call
      workspace   (base, dims): a device buffer of mv_<base>_workspace_bytes(*dims, is_u8) bytes, passed with its size
      allow_bool  bool images are computed as float32 and come back through the reference's integer tail, round_().to(bool)
      what, deps  float32 results are forward-only (forward_only) under the name `what` (default: `name`), computed from
                  the image and `deps`

    The filters, the pools and the preset steps, which widen other dtypes or return pairs, go through launch_xy, lists of frames
    through launch_frames; the CNN layers, with several input tensors each, prepare those with f32_on / ptr / workspace and
    call launch."""
    require_device(image)
    lib = load()
    u8 = image.dtype is torch.uint8
    as_f32 = allow_bool and image.dtype is torch.bool
    with on_device_of(image):
        x = image.to(torch.float32).contiguous() if as_f32 else image.contiguous()
        # each case's cheapest binding of the same allocation: torch.empty(shape, dtype=, device=) costs 1-2 us more host time
        y = torch.empty_like(x, memory_format=torch.contiguous_format) if out_shape is None else x.new_empty(out_shape)
        if workspace is not None:
            base, dims = workspace
            ws_bytes = int(getattr(lib, f"mv_{base}_workspace_bytes")(*dims, int(u8)))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
            args += (ws.data_ptr(), ws_bytes)
        fn = getattr(lib, f"mv_{name}_u8" if u8 else f"mv_{name}_f32")
        check(fn(x.data_ptr(), y.data_ptr(), *args, stream_ptr(x)))
    if as_f32:
        return y.round_().to(torch.bool)
    if u8:
        return y
    return forward_only(y, what or name, image, *deps)


def switch(name: str):
    """The value, now, of one of the module-level switches of `functional` (INTEGER_BLUR_*, BATCH_INVARIANT_SUMMATION,
    CONV2D_*): the one place where they are defined and set.  The modules behind `functional` read them through here at call
    time -- a `from .functional import X` would freeze the default, and `functional` imports those modules."""
    return getattr(sys.modules[__package__ + ".functional"], name)


def taps(values: Sequence[float]):
    arr = (C.c_float * len(values))(*[float(v) for v in values])
    return arr


def pointer_table(tensors):
    """HOST array of device pointers (void*[n]) for the mv_*_v entry points."""
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def taps64_from_tensor(t: torch.Tensor):
    """Host double array from a (CPU, fp64) tensor of taps -- bit-preserving."""
    flat = t.detach().to("cpu", torch.float64).contiguous().reshape(-1)
    arr = (C.c_double * flat.numel())()
    C.memmove(arr, flat.data_ptr(), flat.numel() * 8)
    return arr


def taps_from_tensor(t: torch.Tensor):
    """Host float array from a (CPU, fp32) tensor of taps -- bit-preserving."""
    flat = t.detach().to("cpu", torch.float32).contiguous().reshape(-1)
    arr = (C.c_float * flat.numel())()
    C.memmove(arr, flat.data_ptr(), flat.numel() * 4)
    return arr
