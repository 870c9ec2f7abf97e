"""The steps before the path: resize, center_crop, to_dtype and normalize of the reference's transforms/v2/functional
(_geometry.py:172-262, 1811-1880, _misc.py:19-67, 222-330) for what the presets use, and to_float_normalize, the fused tail of
the ImageClassification preset.  The launches go through _lib.launch_xy.

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import _lib, tv_tensors
from ._registry import _get_kernel, _register_kernel_internal


# --------------------------------------------------------------------------------------------- the step before the path (8f.2)
def _mean_std(mean, std, c: int):
    m = [float(v) for v in (mean if isinstance(mean, (list, tuple)) else [mean])]
    s = [float(v) for v in (std if isinstance(std, (list, tuple)) else [std])]
    if len(m) == 1:
        m = m * c
    if len(s) == 1:
        s = s * c
    if len(m) != c or len(s) != c:
        raise RuntimeError(f"The size of mean/std ({len(m)}/{len(s)}) must match the number of channels ({c})")
    # ATen narrows the Python doubles to the tensor dtype: torch.as_tensor(mean, dtype=float32) (_misc.py:56-57)
    return _lib.taps(m), _lib.taps(s)


# --------------------------------------------------------------------------------------------- resize / center_crop (v2 surface)
def resize(inpt: torch.Tensor, size: Optional[List[int]], interpolation="bilinear", max_size: Optional[int] = None,
           antialias: Optional[bool] = True) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py:172-186."""
    kernel = _get_kernel(resize, type(inpt))
    return kernel(inpt, size=size, interpolation=interpolation, max_size=max_size, antialias=antialias)


@_register_kernel_internal(resize, torch.Tensor)
@_register_kernel_internal(resize, tv_tensors.Image)
def resize_image(image: torch.Tensor, size: Optional[List[int]], interpolation="bilinear", max_size: Optional[int] = None,
                 antialias: Optional[bool] = True) -> torch.Tensor:
    """resize_image (_geometry.py:189-262) for what the presets use: bilinear with antialias.  On a device tensor the
    reference casts uint8 to float32, interpolates, rounds and narrows (:222-254) -- the v1 tensor path's arithmetic
    (_functional_tensor.py:441-474), which mv_resize_bilinear_aa_* reproduces bit for bit."""
    from . import functional_v1
    if size is None:
        if not isinstance(max_size, int):
            raise ValueError(f"max_size must be an integer when size is None, but got {max_size} instead.")
        h, w = int(image.shape[-2]), int(image.shape[-1])  # _geometry.py:117-121: the longer edge becomes max_size
        size = [max_size, int(max_size * w / h)] if h >= w else [int(max_size * h / w), max_size]
        max_size = None
    return functional_v1.resize(image, size, interpolation, max_size, antialias)


@_register_kernel_internal(resize, tv_tensors.Video)
def resize_video(video: torch.Tensor, size: Optional[List[int]], interpolation="bilinear", max_size: Optional[int] = None,
                 antialias: Optional[bool] = True) -> torch.Tensor:
    return resize_image(video, size, interpolation=interpolation, max_size=max_size, antialias=antialias)


def center_crop(inpt: torch.Tensor, output_size: List[int]) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py:1811-1824."""
    kernel = _get_kernel(center_crop, type(inpt))
    return kernel(inpt, output_size=output_size)


@_register_kernel_internal(center_crop, torch.Tensor)
@_register_kernel_internal(center_crop, tv_tensors.Image)
@_register_kernel_internal(center_crop, tv_tensors.Video)
def center_crop_image(image: torch.Tensor, output_size: List[int]) -> torch.Tensor:
    """center_crop_image (_geometry.py:1860-1880): a view when the box lies inside the image, zero padding otherwise."""
    from . import functional_v1
    return functional_v1.center_crop(image, output_size)


def to_dtype(inpt: torch.Tensor, dtype: torch.dtype = torch.float, scale: bool = False) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_misc.py:222-231."""
    kernel = _get_kernel(to_dtype, type(inpt))
    return kernel(inpt, dtype=dtype, scale=scale)


@_register_kernel_internal(to_dtype, torch.Tensor)
@_register_kernel_internal(to_dtype, tv_tensors.Image)
def to_dtype_image(image: torch.Tensor, dtype: torch.dtype = torch.float, scale: bool = False) -> torch.Tensor:
    """to_dtype_image (_misc.py:250-309) for the conversion the inference preset makes: uint8 -> float32 with
    scale=True (image.to(float32).mul_(1/255)) as one kernel.  Same-dtype and scale=False requests are the plain
    casts the reference does; other scaled conversions are outside SURVEY.md section 8 and raise."""
    if image.dtype == dtype:
        return image
    if not scale:
        return image.to(dtype)
    if image.dtype == torch.uint8 and dtype == torch.float32:
        if image.numel() == 0:
            return image.to(dtype)
        _lib.require_device(image)
        return _lib.launch_xy(_lib.load().mv_to_float_normalize_u8, image, (1, 1, image.numel(), None, None), out_dtype=torch.float32)
    raise NotImplementedError(f"scaled conversion {image.dtype} -> {dtype} is not on the MI355X hot path (uint8 -> float32 is)")


@_register_kernel_internal(to_dtype, tv_tensors.BoundingBoxes, tv_tensor_wrapper=False)
@_register_kernel_internal(to_dtype, tv_tensors.Mask, tv_tensor_wrapper=False)
def _to_dtype_tensor_dispatch(inpt: torch.Tensor, dtype: torch.dtype, scale: bool = False) -> torch.Tensor:
    """_misc.py:326-330: masks and boxes are only cast (values are never rescaled)."""
    return inpt.to(dtype)


def normalize(inpt: torch.Tensor, mean: List[float], std: List[float], inplace: bool = False) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_misc.py:19-32."""
    kernel = _get_kernel(normalize, type(inpt))
    return kernel(inpt, mean=mean, std=std, inplace=inplace)


@_register_kernel_internal(normalize, torch.Tensor)
@_register_kernel_internal(normalize, tv_tensors.Image)
def normalize_image(image: torch.Tensor, mean: List[float], std: List[float], inplace: bool = False) -> torch.Tensor:
    """normalize_image (_misc.py:35-67): (image - mean[c]) / std[c] on (..., C, H, W) float images."""
    if not image.is_floating_point():
        raise TypeError(f"Input tensor should be a float tensor. Got {image.dtype}.")
    if image.ndim < 3:
        raise ValueError(f"Expected tensor to be a tensor image of size (..., C, H, W). Got {image.shape}.")
    if isinstance(std, (tuple, list)):
        divzero = not all(std)
    elif isinstance(std, (int, float)):
        divzero = std == 0
    else:
        divzero = False
    if divzero:
        raise ValueError("std evaluated to zero, leading to division by zero.")
    if image.numel() == 0:
        return image
    _lib.require_device(image)
    c = int(image.shape[-3])
    m, s = _mean_std(mean, std, c)
    n = int(image.numel() // (c * image.shape[-1] * image.shape[-2]))
    hw = int(image.shape[-1] * image.shape[-2])
    y = _lib.launch_xy(_lib.load().mv_normalize_f32, image.to(torch.float32), (n, c, hw, m, s))
    y = y if image.dtype == torch.float32 else y.to(image.dtype)
    if inplace:
        image.copy_(y)
        return image
    return y


def to_float_normalize(image: torch.Tensor, mean: List[float], std: List[float]) -> torch.Tensor:
    """normalize(to_dtype(image, float32, scale=True), mean, std) -- the tail of the ImageClassification preset
    (transforms/_presets.py:58-60) -- as ONE pass over a uint8 (..., C, H, W) image: 1 B read + 4 B written."""
    if image.dtype != torch.uint8:
        raise TypeError(f"to_float_normalize expects a uint8 image. Got {image.dtype}")
    if image.ndim < 3:
        raise ValueError(f"Expected tensor to be a tensor image of size (..., C, H, W). Got {image.shape}.")
    if isinstance(std, (tuple, list)) and not all(std):
        raise ValueError("std evaluated to zero, leading to division by zero.")
    _lib.require_device(image)
    c = int(image.shape[-3])
    m, s = _mean_std(mean, std, c)
    hw = int(image.shape[-1] * image.shape[-2])
    n = int(image.numel() // max(c * hw, 1))
    return _lib.launch_xy(_lib.load().mv_to_float_normalize_u8, image, (n, c, hw, m, s), out_dtype=torch.float32)

