"""interpolate_argmax, the labels of a segmentation model: torch.nn.functional.interpolate(mode="bilinear", align_corners=False) of the
logits and the argmax over the classes as ONE launch that writes only the labels (csrc/segment.hip; arithmetic in mi355vision.h,
mv_interpolate_argmax_f32).

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._interp import checked_interpolate_shape

LABEL_DTYPES = {torch.int64: 8, torch.uint8: 1}  # bytes per label


def interpolate_argmax(input: torch.Tensor, size=None, scale_factor=None, *, recompute_scale_factor: Optional[bool] = None,
                       dtype: torch.dtype = torch.int64, mode: str = "bilinear", align_corners: Optional[bool] = False,
                       antialias: bool = False) -> torch.Tensor:
    """interpolate(input, size, scale_factor, ...).argmax(dim=1) bit for bit, (N, C, H, W) float32 -> (N, OH, OW) of `dtype` (int64 or
    uint8, the latter for C <= 256), without the upsampled tensor in memory: the taps and weights of an output pixel are computed once
    for its C planes.  The order is torch.argmax's (the lowest index among equal maxima, -0.0 == +0.0; a NaN is greater than every
    number, the first one wins) on exactly `interpolate`'s float32 values.  Domain and argument errors are `interpolate`'s."""
    if dtype not in LABEL_DTYPES:
        raise NotImplementedError(f"interpolate_argmax: labels of dtype {dtype} are not on the MI355X path (int64 and uint8 are)")
    n, c, h, w, oh, ow = checked_interpolate_shape("interpolate_argmax", input, size, scale_factor, mode, align_corners,
                                                   recompute_scale_factor, antialias)
    if c == 0:
        raise IndexError("argmax(): Expected reduction dim 1 to have non-zero size.")
    if dtype is torch.uint8 and c > 256:
        raise ValueError(f"interpolate_argmax: {c} classes do not fit a uint8 label (up to 256 do); use dtype=torch.int64")
    _lib.require_device(input)
    if n == 0:
        return torch.empty((0, oh, ow), dtype=dtype, device=input.device)
    return _lib.launch_xy(_lib.load().mv_interpolate_argmax_f32, input.detach(), (n, c, h, w, oh, ow, LABEL_DTYPES[dtype]),
                          out_shape=(n, oh, ow), out_dtype=dtype)
