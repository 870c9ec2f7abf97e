"""Functional API of the hot path -- same names, signatures, defaults, validation and error text as the
reference's torchvision.transforms.v2.functional for this path, computed by libmi355vision.so.

This module is the one namespace the package, the tests and tools/ use: it defines the module-level switches below and
re-exports, under the same names and as the same objects (private helpers included), what the modules behind it define --
split as the reference splits transforms/v2/functional/, plus the layers, which the reference keeps elsewhere:
  _filters    gaussian_blur / adjust_sharpness and their _image / PIL / _video kernels and *_frames list forms
              (_misc.py:75-181, _color.py:218-288), the Gaussian taps (_get_gaussian_kernel1d / 2d, _misc.py:86-99), and the new
              operators on the same primitive (BASELINE cfg1/cfg3; the reference has no box / separable / Sobel):
              depthwise_conv2d, box_filter, separable_gaussian_blur, sobel, gaussian_sobel
  _layers     the CNN layers (models/vgg.py:81-85, ops/misc.py:68-128, models/mobilenetv2.py:39-63): conv2d_bias_relu,
              conv2d_bias_act, conv2d_affine_act, max_pool2d*, adaptive_avg_pool2d, linear_bias_relu, conv_norm_act,
              conv1x1_upsample_add (FPN's top-down merge), conv1x1_gated_upsample (LRASPP's head), dwconv_pointwise (SSDlite's
              depthwise-separable block), inverted_residual, dwconv7x7 and conv1x1_gelu (ConvNeXt's block: depthwise 7x7 + bias; the
              per-pixel Linear with the LayerNorm in its loads and GELU in its epilogue),
              fold_batchnorm, normalized_conv2d_bias_relu, the *_k_slices queries
  _misc       resize / center_crop / to_dtype / normalize and their kernels, to_float_normalize
  _geometry   elastic / affine / rotate / perspective and their _image / _mask / _video kernels
  _color      adjust_brightness / adjust_contrast / adjust_saturation / adjust_hue, rgb_to_grayscale,
              invert / posterize / solarize / autocontrast / equalize and their _image / _video kernels
  _crop       pad / crop / flips / resized_crop / erase and their kernels
  _mix        mixup_image / cutmix_image / mixup_labels
  _detection  rpn_topk / rpn_decode / box_decode (models/detection/rpn.py filter_proposals up to the nms, _utils.py
              BoxCoder.decode_single), roi_detections (roi_heads.py postprocess_detections up to the per-image filters),
              retinanet_topk / retinanet_decode (retinanet.py postprocess_detections up to the nms)
              fcos_topk / fcos_decode (fcos.py postprocess_detections up to the nms: the centerness score, BoxLinearCoder.decode)
              ssd_scores / ssd_topk / ssd_decode (ssd.py postprocess_detections up to the nms: softmax, per-class top-k, default boxes)
  _norm       group_norm_act (torch.nn.functional.group_norm + ReLU: the FCOS towers' norm), group_norm_chunk, l2_normalize_scale
              (weight * F.normalize over the channels: SSD's conv4_3), layer_norm2d / layer_norm2d_stats (LayerNorm over the channels of
              an NCHW map: ConvNeXt's LayerNorm2d)
  _se         global_avg_pool / linear_act / se_scale and squeeze_excitation_gate / squeeze_excitation (ops/misc.py SqueezeExcitation;
              MobileNetV3's Linear -> Hardswish); the gate folded into the projection is conv_norm_act(..., input_scale=gate)
  _interp     interpolate (torch.nn.functional.interpolate, plain bilinear) and detection_batch, the fused normalize + resize +
              batch_images in front of a detection model (models/detection/transform.py)
  _mask       paste_masks_in_image / mask_probs (roi_heads.py paste_masks_in_image, maskrcnn_inference) and
              conv_transpose2d_bias_act, ConvTranspose2d(kernel 2, stride 2) + bias + activation (mask_rcnn.py conv5_mask)
  _keypoint   heatmaps_to_keypoints (roi_heads.py) and conv_transpose2d_bias_act's kernel 4, stride 2, padding 1 geometry
              (keypoint_rcnn.py kps_score_lowres) with its conv_transpose4x4_relayout
  _segment    interpolate_argmax, interpolate(...).argmax(1) as one launch that writes only the labels (segmentation.py labels)
The switches (INTEGER_BLUR_*, BATCH_INVARIANT_SUMMATION, CONV2D_*) are set on this module only; the code behind it reads them
here at call time (_lib.switch).

Tensors must live on a HIP device; there is no CPU fallback (see _lib.py).  Host-side work is what the reference also does on
the host: argument checking, the handful of Gaussian taps, reshapes.
"""
from __future__ import annotations

# same objects: everything the modules behind this one define is reached through it
from ._color import (_add_alpha_fuses, adjust_brightness, adjust_brightness_image, adjust_brightness_video,  # noqa: F401
                     adjust_contrast, adjust_contrast_image, adjust_contrast_video, adjust_hue, adjust_hue_image,
                     adjust_hue_video, adjust_saturation, adjust_saturation_image, adjust_saturation_video,
                     autocontrast, autocontrast_image, autocontrast_video, _blend_form, _check_color_channels,
                     _check_color_factor, _color_chain, color_jitter_image, _COLOR_OPS, equalize, equalize_image,
                     equalize_video, invert, invert_image, invert_video, _plane_op, _POINT_OPS, _pointwise,
                     posterize, posterize_image, posterize_video, rgb_to_grayscale, rgb_to_grayscale_image,
                     solarize, solarize_image, solarize_video)
from ._crop import (axis_index_map, crop, crop_image, crop_mask, crop_video, erase, erase_image, erase_video, hflip,  # noqa: F401
                    horizontal_flip, horizontal_flip_image, horizontal_flip_mask, horizontal_flip_video, pad, pad_crop,
                    pad_crop_image, pad_image, pad_mask, PAD_MODES, pad_video, _parse_pad_padding, resized_crop,
                    resized_crop_flip_normalize, resized_crop_image, resized_crop_video, vertical_flip,
                    vertical_flip_image, vertical_flip_mask, vertical_flip_video, vflip)
from ._mix import cutmix_image, mixup_image, mixup_labels  # noqa: F401
from ._geometry import (affine, _affine_coeffs, affine_image, affine_mask, _affine_parse_args, affine_video,  # noqa: F401
                        _assert_grid_transform_inputs, _blocked_bmm_fuses, _BMM_NAIVE_LIMIT,
                        _compute_affine_output_size, elastic, _elastic_bounding_boxes_dispatch, _elastic_fill,
                        elastic_image, _elastic_image_pil, elastic_mask, _ELASTIC_MODES, elastic_transform,
                        elastic_video, _get_inverse_affine_matrix, _get_perspective_coeffs, _grid_order,
                        _identity_grid_vectors, _interpolation_name, _nearest_on_mask, perspective,
                        _perspective_coefficients, _perspective_grid_coeffs, perspective_image, perspective_mask,
                        perspective_video, _PIL_INTERPOLATION, rotate, rotate_image, rotate_mask, rotate_video,
                        _warp, _WARP_KINDS)
from ._detection import (BBOX_XFORM_CLIP, box_decode, fcos_decode, fcos_topk, MAX_ROI_CLASSES, MAX_RPN_LEVELS,  # noqa: F401
                         MAX_RPN_TOPK, retinanet_decode, retinanet_topk, retinanet_topk_chunk, roi_detections, rpn_decode, rpn_topk,
                         ssd_decode, ssd_scores, ssd_topk)
from ._filters import (_adjust_sharpness_image_pil, adjust_sharpness, adjust_sharpness_frames, adjust_sharpness_image,  # noqa: F401
                       adjust_sharpness_video, _blur_with_taps, _border, box_filter, _check_gaussian_args, _compute_dtype,
                       depthwise_conv2d, _DIRECT_2D_MAX_TAPS, _filter_f32_u8, _frames_call, gaussian_blur,
                       gaussian_blur_frames, gaussian_blur_image, _gaussian_blur_image_pil, gaussian_blur_video,
                       gaussian_sobel, _get_gaussian_kernel1d, _get_gaussian_kernel2d, _host_taps, _pair_f32, _planes,
                       _same_frames, separable_gaussian_blur, _sharpness, sobel, _taps_dtype, _use_separable)
from ._interp import detection_batch, interpolate, interpolate_output_size, MAX_NORMALIZE_CHANNELS  # noqa: F401
from ._layers import (_ACT_CODES, adaptive_avg_pool2d, _AFFINE_CODES, conv1x1_gated_upsample, conv1x1_gelu, conv1x1_k_slices,  # noqa: F401
                      conv1x1_upsample_add, dwconv7x7,
                      conv2d_affine_act, conv2d_bias_act, conv2d_bias_relu,
                      conv3x3_k_slices, conv_norm_act, _CONV_WORKSPACE_BYTES, dwconv_pointwise, fold_batchnorm, inverted_residual,
                      inverted_residual_k_slices, _inverted_residual_workspace_bytes, linear_bias_relu, linear_k_slices,
                      max_pool2d, max_pool2d_2x2, normalized_conv2d_bias_relu)
from ._keypoint import conv_transpose4x4_relayout, heatmaps_to_keypoints, MAX_HEATMAP_ELEMENTS  # noqa: F401
from ._lib import max_value as _max_value  # noqa: F401
from ._mask import conv_transpose2d_bias_act, conv_transpose2x2_relayout, mask_probs, paste_masks_in_image  # noqa: F401
from ._misc import (center_crop, center_crop_image, _mean_std, normalize, normalize_image, resize, resize_image,  # noqa: F401
                    resize_video, to_dtype, to_dtype_image, _to_dtype_tensor_dispatch, to_float_normalize)
from ._norm import group_norm_act, group_norm_chunk, l2_normalize_scale, layer_norm2d, layer_norm2d_stats  # noqa: F401
from ._se import global_avg_pool, linear_act, se_scale, squeeze_excitation, squeeze_excitation_gate  # noqa: F401
from ._segment import interpolate_argmax, LABEL_DTYPES  # noqa: F401
from ._registry import _get_kernel, _register_kernel_internal  # noqa: F401

# uint8 images with a kernel side above 3.  True (default) = ONE 2-D pass, the reference's own formulation
# (_misc.py:147-163: pad -> conv2d with the outer-product kernel -> round_()): equal to the reference's outputs on every pixel of
# the committed fixtures (93 144 uint8 pixels, tests/golden/gaussian_blur.npz) and on 37.7 M random pixels against the
# reference's call sequence on torch-CPU (3x3 ... 23x23: 0 differing pixels).  False = the fp32 separable pair + one round_():
# kx + ky instead of kx * ky taps (5x5 1.8x, 7x7 2.4x, 23x23 28x faster on 32 x 4K uint8) but another association of the sum --
# on the same data it differs from the reference by 1 LSB in 1 of the 93 144 fixture pixels and in 0.0006-0.0036 % of the
# random ones (exact rounding ties; the reference's own test allows atol = 1).  Integer results are the reference's by
# default; the fast form is an opt-in (DESIGN.md section 4 has the table).
INTEGER_BLUR_EXACT_2D = True
# With INTEGER_BLUR_EXACT_2D: True = get those integers through mv_gaussian_blur_u8_ws -- the separable pair for every pixel
# plus the 2-D chain for the 1-4 % of lane-rows whose value lies within the two forms' (proved) error bound of a rounding tie:
# the same bits as the 2-D pass, 1.5-20x faster (csrc/tiefix_u8.hip).  False = run the plain 2-D pass.
INTEGER_BLUR_EXACT_FAST = True
# The 3x3 convolutions and the Linear layers of the CNNs run K in slices when a launch is too small to fill the chip
# (conv3x3_k_slices / linear_k_slices).  The slice plan depends on the workgroup count and therefore on the BATCH SIZE: the
# same image can differ in its last bits between batch 1 and batch 8 (<= 1e-6 relative; each plan is stated by the library
# and restated by the oracle).  True = every such call keeps the single ascending chain per output, whatever the batch:
# batch-invariant bits, at the small-batch speed of the unsliced kernels.  A fused InvertedResidual block whose plan has several
# slices (mv_inverted_residual_k_slices) then runs as three launches.  (MobileNet's pointwise convs slice K inside the
# workgroup, mv_conv1x1_k_slices: that plan is part of the kernel and is not switched by this flag.)
BATCH_INVARIANT_SUMMATION = False
# True: conv2d_bias_act brings the columns workspace even when the library does not ask for it (the tuning build's MV_CONV_COLUMNS
# then runs the im2col + GEMM form: what the tests and tools compare the implicit kernel with)
CONV2D_COLUMNS_WORKSPACE = False
# True: launches of a handful of workgroups (batch 1) bring the optional columns workspace (mv_conv2d_needs_workspace() == 2): the
# columns form cuts smaller tiles there (AlexNet batch 1: 0.37 -> 0.28 ms)
CONV2D_SMALL_LAUNCH_WORKSPACE = True
