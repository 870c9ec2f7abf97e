"""models/detection/transform.py: GeneralizedRCNNTransform, the normalisation and batching in front of a detection model and the
box rescaling behind it.

`forward` computes the resized sizes on the host (`resized_size`) and makes ONE launch, F.detection_batch: normalize, the reference's
non-antialiased bilinear `interpolate` and the zero-padded batch in one pass over the pixels.  The pieces stay
callable on their own and give the same bits: `normalize` is the package's F.normalize, `resize` is F.interpolate at the size
`resized_size` gives (device tensors only), `batch_images` is the reference's new_full + copy_ on the device; `postprocess` /
`resize_boxes` is the reference's float32 composition, and a prediction with "masks" (Mask R-CNN) has them pasted into the original
image by ONE F.paste_masks_in_image launch per image, on the rescaled boxes as in the reference.  With the reference's private keyword `_skip_resize=True` (the reference
honours it in training mode only; here it also stands for inference on images that already have their final size) `forward` runs
those pieces one by one and does not resize.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import nn, Tensor

from . import functional as F
from .image_list import ImageList

__all__ = ["GeneralizedRCNNTransform", "resize_boxes", "resized_size"]


def resized_size(h: int, w: int, min_size: int, max_size: int, fixed_size: Optional[Tuple[int, int]] = None) -> Tuple[int, int]:
    """(oh, ow) of the reference's _resize_image_and_masks (transform.py:24-75) for an (h, w) image at inference.  With `fixed_size`
    = (width, height) it is (fixed_size[1], fixed_size[0]).  Otherwise the reference's EAGER branch: scale_factor = min(min_size /
    min(h, w), max_size / max(h, w)) in Python floats, then interpolate's recompute_scale_factor=True rule, floor(float(in) *
    scale_factor) per axis.  The reference's scripted / tracing branch computes the scale in float32 tensors and gives another size
    for some shapes (201 x 201 at 800 / 1333: 800 x 800 here, 799 x 799 there); the library implements the eager branch only."""
    if fixed_size is not None:
        return int(fixed_size[1]), int(fixed_size[0])
    scale_factor = min(float(min_size) / float(min(h, w)), float(max_size) / float(max(h, w)))
    oh, ow = F.interpolate_output_size((h, w), scale_factor=scale_factor)
    return oh, ow


class GeneralizedRCNNTransform(nn.Module):
    """transform.py:78-285.  forward(images, targets=None) -> (ImageList, targets): normalise each (C, H, W) image, resize it so that
    its shorter side is min_size unless the longer one would exceed max_size (or to `fixed_size`), pad them into one batch whose
    sides are multiples of `size_divisible`; image_sizes are the resized sizes."""

    def __init__(self, min_size: int, max_size: int, image_mean: List[float], image_std: List[float], size_divisible: int = 32,
                 fixed_size: Optional[Tuple[int, int]] = None, **kwargs: Any):
        super().__init__()
        if not isinstance(min_size, (list, tuple)):
            min_size = (min_size,)
        self.min_size = min_size
        self.max_size = max_size
        self.image_mean = image_mean
        self.image_std = image_std
        self.size_divisible = size_divisible
        self.fixed_size = fixed_size
        self._skip_resize = kwargs.pop("_skip_resize", False)
        self.eval()

    def forward(self, images: List[Tensor], targets: Optional[List[Dict[str, Tensor]]] = None) -> Tuple[ImageList, Optional[List[Dict[str, Tensor]]]]:
        if self.training or targets is not None:
            raise RuntimeError("the MI355X GeneralizedRCNNTransform is inference only: call .eval() and pass no targets")
        images = [img for img in images]
        if not self._skip_resize:
            return self._forward_fused(images), targets
        for i in range(len(images)):
            image = images[i]
            if image.dim() != 3:
                raise ValueError(f"images is expected to be a list of 3d tensors of shape [C, H, W], got {image.shape}")
            image = self.normalize(image)
            image = self.resize(image)
            images[i] = image

        image_sizes = [img.shape[-2:] for img in images]
        images = self.batch_images(images, size_divisible=self.size_divisible)
        image_sizes_list: List[Tuple[int, int]] = []
        for image_size in image_sizes:
            torch._assert(len(image_size) == 2, f"Input tensors expected to have in the last two elements H and W, instead got {image_size}")
            image_sizes_list.append((image_size[0], image_size[1]))

        image_list = ImageList(images, image_sizes_list)
        return image_list, targets

    def _forward_fused(self, images: List[Tensor]) -> ImageList:
        """normalize -> resize -> batch_images of every image as one F.detection_batch launch: the same checks, the same bits."""
        for image in images:
            if image.dim() != 3:
                raise ValueError(f"images is expected to be a list of 3d tensors of shape [C, H, W], got {image.shape}")
            self._check_dtype(image)
        sizes = [resized_size(int(img.shape[-2]), int(img.shape[-1]), self.min_size[-1], self.max_size, self.fixed_size) for img in images]
        batch = F.detection_batch(images, sizes, list(self.image_mean), list(self.image_std), self.size_divisible)
        return ImageList(batch, sizes)

    def _check_dtype(self, image: Tensor) -> None:
        if not image.is_floating_point():
            raise TypeError(f"Expected input images to be of floating type (in range [0, 1]), but found type {image.dtype} instead")
        if image.dtype != torch.float32:
            raise TypeError(f"GeneralizedRCNNTransform computes in float32. Got {image.dtype}")

    def normalize(self, image: Tensor) -> Tensor:
        self._check_dtype(image)
        return F.normalize(image, list(self.image_mean), list(self.image_std))

    def resize(self, image: Tensor) -> Tensor:
        """_resize_image_and_masks for inference, the eager branch (resized_size), on a (C, H, W) float32 device tensor."""
        if self._skip_resize:
            return image
        if not image.is_cuda:
            raise NotImplementedError("GeneralizedRCNNTransform.resize: the non-antialiased bilinear interpolate runs on the device only "
                                      f"(F.interpolate); the image lives on '{image.device}'")
        size = resized_size(int(image.shape[-2]), int(image.shape[-1]), self.min_size[-1], self.max_size, self.fixed_size)
        return F.interpolate(image[None], size=list(size), mode="bilinear", align_corners=False)[0]

    def max_by_axis(self, the_list: List[List[int]]) -> List[int]:
        maxes = the_list[0]
        for sublist in the_list[1:]:
            for index, item in enumerate(sublist):
                maxes[index] = max(maxes[index], item)
        return maxes

    def batch_images(self, images: List[Tensor], size_divisible: int = 32) -> Tensor:
        max_size = self.max_by_axis([list(img.shape) for img in images])
        stride = float(size_divisible)
        max_size = list(max_size)
        max_size[1] = int(math.ceil(float(max_size[1]) / stride) * stride)
        max_size[2] = int(math.ceil(float(max_size[2]) / stride) * stride)

        batch_shape = [len(images)] + max_size
        batched_imgs = images[0].new_full(batch_shape, 0)
        for i in range(batched_imgs.shape[0]):
            img = images[i]
            batched_imgs[i, : img.shape[0], : img.shape[1], : img.shape[2]].copy_(img)

        return batched_imgs

    def postprocess(self, result: List[Dict[str, Tensor]], image_shapes: List[Tuple[int, int]],
                    original_image_sizes: List[Tuple[int, int]]) -> List[Dict[str, Tensor]]:
        if self.training:
            return result
        for i, (pred, im_s, o_im_s) in enumerate(zip(result, image_shapes, original_image_sizes)):
            boxes = pred["boxes"]
            boxes = resize_boxes(boxes, im_s, o_im_s)
            result[i]["boxes"] = boxes
            if "masks" in pred:
                masks = pred["masks"]
                masks = F.paste_masks_in_image(masks, boxes, o_im_s)
                result[i]["masks"] = masks
            if "keypoints" in pred:
                keypoints = pred["keypoints"]
                keypoints = resize_keypoints(keypoints, im_s, o_im_s)
                result[i]["keypoints"] = keypoints
        return result

    def __repr__(self) -> str:
        format_string = f"{self.__class__.__name__}("
        _indent = "\n    "
        format_string += f"{_indent}Normalize(mean={self.image_mean}, std={self.image_std})"
        format_string += f"{_indent}Resize(min_size={self.min_size}, max_size={self.max_size}, mode='bilinear')"
        format_string += "\n)"
        return format_string


def resize_keypoints(keypoints: Tensor, original_size: List[int], new_size: List[int]) -> Tensor:
    """transform.py:284-298, the eager branch: a torch composition, as resize_boxes"""
    ratios = [
        torch.tensor(s, dtype=torch.float32, device=keypoints.device) / torch.tensor(s_orig, dtype=torch.float32, device=keypoints.device)
        for s, s_orig in zip(new_size, original_size)
    ]
    ratio_h, ratio_w = ratios
    resized_data = keypoints.clone()
    resized_data[..., 0] *= ratio_w
    resized_data[..., 1] *= ratio_h
    return resized_data


def resize_boxes(boxes: Tensor, original_size: List[int], new_size: List[int]) -> Tensor:
    """transform.py:301-313"""
    ratios = [
        torch.tensor(s, dtype=torch.float32, device=boxes.device) / torch.tensor(s_orig, dtype=torch.float32, device=boxes.device)
        for s, s_orig in zip(new_size, original_size)
    ]
    ratio_height, ratio_width = ratios
    xmin, ymin, xmax, ymax = boxes.unbind(1)

    xmin = xmin * ratio_width
    xmax = xmax * ratio_width
    ymin = ymin * ratio_height
    ymax = ymax * ratio_height
    return torch.stack((xmin, ymin, xmax, ymax), dim=1)
