"""The mask branch of Mask R-CNN behind the mask head: paste_masks_in_image and mask_probs (models/detection/roi_heads.py
paste_masks_in_image / maskrcnn_inference) and conv_transpose2d_bias_act, nn.ConvTranspose2d(kernel 2, stride 2) + bias + activation
(mask_rcnn.py's conv5_mask; the kernel 4, stride 2, padding 1 geometry of Keypoint R-CNN goes on to _keypoint.py) -- ONE launch each
(csrc/mask.hip, the pixel-shuffle instance of csrc/convnorm.hip's pointwise kernel; arithmetic in mi355vision.h, mv_paste_masks_f32
and below).

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._keypoint import conv_transpose4x4s2
from ._layers import _ACT_CODES


def paste_masks_in_image(masks: torch.Tensor, boxes: torch.Tensor, img_shape: Sequence[int], padding: int = 1) -> torch.Tensor:
    """roi_heads.py paste_masks_in_image: masks (R, 1, M, M) float32 and boxes (R, 4) float32 on the device -> (R, 1, H, W) float32,
    mask r resized into its box expanded by (M + 2 padding) / M and truncated to integers, zeros elsewhere.  ONE launch writes the
    result once; the boxes are read on the device, nothing is read back.  Numerics and domain: mi355vision.h, mv_paste_masks_f32
    (a box with a non-finite or huge coordinate gives a zero plane; a box wholly outside the image gives zeros where the reference
    raises or wraps around)."""
    if masks.dim() != 4 or masks.shape[1] != 1 or masks.shape[2] != masks.shape[3]:
        raise ValueError(f"paste_masks_in_image: masks are expected to have the shape [R, 1, M, M], got {list(masks.shape)}")
    if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.shape[0] != masks.shape[0]:
        raise ValueError(f"paste_masks_in_image: boxes are expected to have the shape [{masks.shape[0]}, 4], got {list(boxes.shape)}")
    if masks.dtype != torch.float32 or boxes.dtype != torch.float32:
        raise TypeError(f"paste_masks_in_image computes in float32. Got masks {masks.dtype}, boxes {boxes.dtype}")
    if len(img_shape) != 2:
        raise ValueError(f"paste_masks_in_image: img_shape is expected to be (height, width), got {tuple(img_shape)}")
    im_h, im_w = int(img_shape[0]), int(img_shape[1])
    padding = int(padding)
    r, m = int(masks.shape[0]), int(masks.shape[2])
    if m < 1 or im_h < 1 or im_w < 1 or padding < 0:
        raise ValueError(f"paste_masks_in_image: masks of side {m}, an image of ({im_h}, {im_w}) and padding {padding}: the sizes should "
                         "be positive and the padding non-negative")
    _lib.require_device(masks, "masks")
    _lib.require_device(boxes, "boxes")
    if boxes.device != masks.device:
        raise ValueError("paste_masks_in_image: masks and boxes must live on one device")
    if r == 0:
        return masks.new_empty((0, 1, im_h, im_w))
    mc, bc = masks.detach().contiguous(), boxes.detach().contiguous()
    out = torch.empty((r, 1, im_h, im_w), dtype=torch.float32, device=masks.device)
    _lib.launch(_lib.load().mv_paste_masks_f32, mc, mc.data_ptr(), bc.data_ptr(), out.data_ptr(), r, m, padding, im_h, im_w)
    return _lib.forward_only(out, "paste_masks_in_image", masks, boxes)


def mask_probs(mask_logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """roi_heads.py maskrcnn_inference before the split: mask_logits (R, C, Mh, Mw) float32 and labels (R,) int64 on the device ->
    (R, 1, Mh, Mw) = sigmoid(mask_logits[r, labels[r]]), ONE launch that reads only the selected planes (the reference runs the
    sigmoid over all C planes, then indexes).  A label outside [0, C) gives a zero plane (the reference raises; the labels are not
    read back).  Numerics: mi355vision.h, mv_mask_probs_f32."""
    if mask_logits.dim() != 4:
        raise ValueError(f"mask_probs: mask_logits are expected to have the shape [R, C, Mh, Mw], got {list(mask_logits.shape)}")
    if labels.dim() != 1 or labels.shape[0] != mask_logits.shape[0]:
        raise ValueError(f"mask_probs: labels are expected to have the shape [{mask_logits.shape[0]}], got {list(labels.shape)}")
    if mask_logits.dtype != torch.float32:
        raise TypeError(f"mask_probs computes in float32. Got {mask_logits.dtype}")
    if labels.dtype != torch.int64:
        raise TypeError(f"mask_probs: labels are expected to be int64. Got {labels.dtype}")
    r, c, mh, mw = (int(s) for s in mask_logits.shape)
    if c < 1 or mh < 1 or mw < 1:
        raise ValueError(f"mask_probs: mask_logits of shape {list(mask_logits.shape)}: classes and sizes should be positive")
    _lib.require_device(mask_logits, "mask_logits")
    _lib.require_device(labels, "labels")
    if labels.device != mask_logits.device:
        raise ValueError("mask_probs: mask_logits and labels must live on one device")
    if r == 0:
        return mask_logits.new_empty((0, 1, mh, mw))
    xc, lc = mask_logits.detach().contiguous(), labels.contiguous()
    out = torch.empty((r, 1, mh, mw), dtype=torch.float32, device=mask_logits.device)
    _lib.launch(_lib.load().mv_mask_probs_f32, xc, xc.data_ptr(), lc.data_ptr(), out.data_ptr(), r, c, mh, mw)
    return _lib.forward_only(out, "mask_probs", mask_logits)


def _pair(v) -> Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def conv_transpose2x2_relayout(weight: torch.Tensor, bias: Optional[torch.Tensor], device) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """torch's ConvTranspose2d weight (cin, cout, 2, 2) and bias (cout) as what mv_conv_transpose2x2_bias_act_f32 takes: the weight
    (4 cout, cin), row 4 co + 2 dy + dx = weight[:, co, dy, dx], and the bias with every entry repeated four times -- float32,
    contiguous, on `device`.  A module calls this once per parameter version (MaskRCNNPredictor.relaid)."""
    cin, cout = int(weight.shape[0]), int(weight.shape[1])
    with torch.no_grad():
        w4 = weight.detach().to(device, torch.float32).permute(1, 2, 3, 0).reshape(4 * cout, cin).contiguous()
        b4 = None if bias is None else bias.detach().to(device, torch.float32).repeat_interleave(4).contiguous()
    return w4, b4


def conv_transpose2d_bias_act(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, activation: Optional[str] = None,
                              stride=2, padding=0, output_padding=0, groups: int = 1, dilation=1,
                              relaid: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None) -> torch.Tensor:
    """nn.ConvTranspose2d + bias + activation (None / "relu" / "relu6") as ONE launch, x (N, Cin, H, W) and torch's weight (Cin, Cout,
    k, k) -> (N, Cout, 2 H, 2 W), in exactly two geometries:
      kernel 2, stride 2, padding 0   the four taps never overlap, so this is a pointwise conv with 4 Cout channels whose store is a
                                      pixel shuffle; the summation order is the one conv1x1_k_slices(N, Cin, H, W, 4 Cout) states;
      kernel 4, stride 2, padding 1   every output phase (py, px) is a 2x2 convolution of the input, so this is the implicit-GEMM
                                      conv2d_bias_act(x, w2, bias4, padding=1) with 4 Cout channels whose store keeps each phase's
                                      window positions (_keypoint.py); the summation order is conv2d_bias_act's single chain.
    Any other geometry raises NotImplementedError naming the argument.  `relaid`: the result of conv_transpose2x2_relayout /
    conv_transpose4x4_relayout for this weight and bias, when the caller caches it."""
    if x.ndim != 4 or weight.ndim != 4:
        raise RuntimeError(f"Expected 4D input and weight. Got {tuple(x.shape)} and {tuple(weight.shape)}")
    four = weight.ndim == 4 and tuple(weight.shape[2:]) == (4, 4)
    for name, value, want in (("stride", _pair(stride), (2, 2)), ("padding", _pair(padding), (1, 1) if four else (0, 0)),
                              ("output_padding", _pair(output_padding), (0, 0)), ("dilation", _pair(dilation), (1, 1))):
        if value != want:
            raise NotImplementedError(f"conv_transpose2d_bias_act: {name}={value} is not on the MI355X path ({name}={want} is)")
    if groups != 1:
        raise NotImplementedError(f"conv_transpose2d_bias_act: groups={groups} is not on the MI355X path (groups=1 is)")
    if not four and tuple(weight.shape[2:]) != (2, 2):
        raise NotImplementedError(f"conv_transpose2d_bias_act: kernel_size={tuple(weight.shape[2:])} is not on the MI355X path "
                                  "(kernel_size=(2, 2) with padding 0 and (4, 4) with padding 1 are)")
    if activation not in (None, "none", "relu", "relu6"):
        raise NotImplementedError(f"conv_transpose2d_bias_act: activation={activation!r} is not on the MI355X path (None, 'relu' and "
                                  "'relu6' are)")
    n, cin, h, w = (int(d) for d in x.shape)
    cout = int(weight.shape[1])
    if int(weight.shape[0]) != cin:
        raise RuntimeError(f"weight {tuple(weight.shape)} does not fit {cin} input channels")
    if bias is not None and bias.numel() != cout:
        raise RuntimeError(f"bias has {bias.numel()} elements for {cout} output channels")
    if h < 1 or w < 1:
        raise RuntimeError(f"conv_transpose2d_bias_act: an input of shape {tuple(x.shape)} has no pixels")
    _lib.require_f32_layer("conv_transpose2d_bias_act", x, weight)
    _lib.require_device(x)
    if four:
        y = conv_transpose4x4s2(x, weight, bias, _ACT_CODES[activation], relaid)
        return _lib.forward_only(y, "conv_transpose2d_bias_act", x, weight, bias)
    w4, b4 = relaid if relaid is not None else conv_transpose2x2_relayout(weight, bias, x.device)
    y = torch.empty((n, cout, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    if n == 0:
        return y
    xc = x.contiguous()
    _lib.launch(_lib.load().mv_conv_transpose2x2_bias_act_f32, xc, xc.data_ptr(), w4.data_ptr(), _lib.ptr(b4), y.data_ptr(), n, cin, h, w,
                cout, _ACT_CODES[activation])
    return _lib.forward_only(y, "conv_transpose2d_bias_act", x, weight, bias)
