"""interpolate, torch.nn.functional.interpolate for the one mode a detection model's transform uses (bilinear, align_corners=False,
antialias=False), and detection_batch, that transform's normalize -> resize -> batch_images as ONE launch (csrc/interp.hip;
arithmetic in mi355vision.h, mv_interpolate_bilinear_f32 and mv_detection_batch_f32).

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._misc import _mean_std

MAX_NORMALIZE_CHANNELS = 16  # mean / std travel in the kernel arguments


def interpolate_output_size(in_size: Sequence[int], size=None, scale_factor=None) -> List[int]:
    """The (oh, ow) torch.nn.functional.interpolate computes for a 4-D input: `size` itself, or with scale_factor and
    recompute_scale_factor=True floor(float(in) * scale_factor) per axis in Python doubles."""
    if size is not None and scale_factor is not None:
        raise ValueError("only one of size or scale_factor should be defined")
    if size is None and scale_factor is None:
        raise ValueError("either size or scale_factor should be defined")
    if size is not None:
        out = [int(s) for s in size] if isinstance(size, (list, tuple)) else [int(size)] * 2
        if len(out) != 2:
            raise ValueError(f"Input and output must have the same number of spatial dimensions, but got input with spatial dimensions of "
                             f"{list(in_size)} and output size of {list(size)}. Please provide input tensor in (N, C, d1, d2, ...,dK) format "
                             "and output size in (o1, o2, ...,oK) format.")
        return out
    factors = [float(f) for f in scale_factor] if isinstance(scale_factor, (list, tuple)) else [float(scale_factor)] * 2
    if len(factors) != 2:
        raise ValueError(f"Input and scale_factor must have the same number of spatial dimensions, but got input with spatial dimensions of "
                         f"{list(in_size)} and scale_factor of shape {list(scale_factor)}. Please provide input tensor in (N, C, d1, d2, ...,dK) "
                         "format and scale_factor in (s1, s2, ...,sK) format.")
    return [int(math.floor(float(i) * f)) for i, f in zip(in_size, factors)]


def checked_interpolate_shape(name: str, input: torch.Tensor, size, scale_factor, mode: str, align_corners: Optional[bool],
                              recompute_scale_factor: Optional[bool], antialias: bool) -> Tuple[int, int, int, int, int, int]:
    """The domain of `interpolate`, shared with interpolate_argmax: (n, c, h, w, oh, ow) of a 4-D float32 tensor for
    mode="bilinear", align_corners=False, antialias=False; everything else raises, naming the argument."""
    if mode != "bilinear":
        raise NotImplementedError(f"{name}: mode={mode!r} is not on the MI355X path (mode='bilinear' is)")
    if align_corners:
        raise NotImplementedError(f"{name}: align_corners=True is not on the MI355X path (align_corners=False is)")
    if antialias:
        raise NotImplementedError(f"{name}: antialias=True is not on this entry (F.resize is the antialiased bilinear resize)")
    if input.dim() != 4:
        raise NotImplementedError(f"{name}: input of {input.dim()} dimensions is not on the MI355X path (4-D (N, C, H, W) is)")
    if input.dtype != torch.float32:
        raise NotImplementedError(f"{name}: input of dtype {input.dtype} is not on the MI355X path (float32 is)")
    if scale_factor is not None and size is None and not recompute_scale_factor:
        raise NotImplementedError(f"{name}: scale_factor without recompute_scale_factor=True is not on the MI355X path (the kernel's "
                                  "scale is in / out)")
    n, c, h, w = (int(s) for s in input.shape)
    oh, ow = interpolate_output_size((h, w), size, scale_factor)
    if recompute_scale_factor and size is not None:
        raise ValueError("recompute_scale_factor is not meaningful with an explicit size.")
    if h < 1 or w < 1 or oh < 1 or ow < 1:
        raise ValueError(f"Input and output sizes should be greater than 0, but got input (H: {h}, W: {w}) output (H: {oh}, W: {ow})")
    return n, c, h, w, oh, ow


def interpolate(input: torch.Tensor, size=None, scale_factor=None, mode: str = "bilinear", align_corners: Optional[bool] = False,
                recompute_scale_factor: Optional[bool] = None, antialias: bool = False) -> torch.Tensor:
    """torch.nn.functional.interpolate on a 4-D float32 device tensor for mode="bilinear", align_corners=False, antialias=False, the
    size given by `size=` or by `scale_factor=` with recompute_scale_factor=True.  Everything else raises NotImplementedError naming
    the argument (the antialiased bilinear resize is F.resize).  Numerics: mi355vision.h, mv_interpolate_bilinear_f32."""
    n, c, h, w, oh, ow = checked_interpolate_shape("interpolate", input, size, scale_factor, mode, align_corners, recompute_scale_factor,
                                                   antialias)
    _lib.require_device(input)
    if n * c == 0:
        return input.new_empty((n, c, oh, ow))
    y = _lib.launch_xy(_lib.load().mv_interpolate_bilinear_f32, input, (n * c, h, w, oh, ow), out_shape=(n, c, oh, ow))
    return _lib.forward_only(y, "interpolate", input)


def _ints(values):
    return (C.c_int * len(values))(*[int(v) for v in values])


def detection_batch(images: Sequence[torch.Tensor], sizes: Sequence[Tuple[int, int]], mean, std, size_divisible: int = 32) -> torch.Tensor:
    """GeneralizedRCNNTransform's front end as ONE launch: image i, a (C, h_i, w_i) float32 device tensor allocated on its own, is
    normalised with (mean, std), resized to sizes[i] = (oh_i, ow_i) with `interpolate`'s arithmetic and written into the zero-padded
    batch (N, C, Hp, Wp), Hp and Wp the greatest oh_i and ow_i rounded up to multiples of `size_divisible` (batch_images).  The bits
    are those of normalize -> interpolate -> batch_images.  Numerics: mi355vision.h, mv_detection_batch_f32."""
    images = list(images)
    if not images:
        raise ValueError("detection_batch: an empty list of images")
    if len(sizes) != len(images):
        raise ValueError(f"detection_batch: {len(images)} images and {len(sizes)} sizes")
    first = images[0]
    for image in images:
        if image.dim() != 3:
            raise ValueError(f"images is expected to be a list of 3d tensors of shape [C, H, W], got {image.shape}")
        if image.dtype != torch.float32:
            raise TypeError(f"detection_batch computes in float32. Got {image.dtype}")
        _lib.require_device(image)
        if image.device != first.device or image.shape[0] != first.shape[0]:
            raise ValueError("detection_batch: the images must live on one device and have the same number of channels")
    c = int(first.shape[0])
    if isinstance(std, (tuple, list)) and not all(std):
        raise ValueError("std evaluated to zero, leading to division by zero.")
    if not 1 <= c <= MAX_NORMALIZE_CHANNELS:
        raise NotImplementedError(f"detection_batch: {c} channels are not on the MI355X path (1 to {MAX_NORMALIZE_CHANNELS} are)")
    m, s = _mean_std(mean, std, c)
    sizes = [(int(oh), int(ow)) for oh, ow in sizes]
    stride = float(size_divisible)  # batch_images
    hp = int(math.ceil(float(max(oh for oh, _ in sizes)) / stride) * stride)
    wp = int(math.ceil(float(max(ow for _, ow in sizes)) / stride) * stride)
    xs = [image.contiguous() for image in images]
    out = torch.empty((len(xs), c, hp, wp), dtype=torch.float32, device=first.device)
    _lib.launch(_lib.load().mv_detection_batch_f32, first, _lib.pointer_table(xs), _ints([x.shape[1] for x in xs]),
                _ints([x.shape[2] for x in xs]), _ints([oh for oh, _ in sizes]), _ints([ow for _, ow in sizes]), len(xs), c, m, s,
                out.data_ptr(), hp, wp)
    return _lib.forward_only(out, "detection_batch", *images)
