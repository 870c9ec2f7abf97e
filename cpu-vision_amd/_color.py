"""The colour ops of the v2 surface -- the reference's transforms/v2/functional/_color.py adjust_brightness / contrast /
saturation / hue, rgb_to_grayscale, invert, posterize, solarize, autocontrast and equalize with their _image / _video kernels:
argument checks and special cases here, with the reference's error text; the pixels go through csrc/color.hip and
csrc/autoaug.hip, one call per op or per ColorJitter chain (DESIGN.md sections 3.15 and 3.16).

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Sequence, Tuple

import torch

from . import _lib, _pil, tv_tensors
from ._registry import _get_kernel, _register_image_and_video, _register_kernel_internal, _unsupported

# --------------------------------------------------------------------------------------------- colour (v2 surface)
# transforms/v2/functional/_color.py: argument checks and special cases here, with the reference's error text; the pixel
# arithmetic is one chain of ops per call in k_color (csrc/color.hip).
_COLOR_OPS = {"brightness": 0, "contrast": 1, "saturation": 2, "hue": 3}


@functools.lru_cache(maxsize=None)
def _add_alpha_fuses() -> bool:
    """Whether this host's `a.add_(b, alpha=s)` on float32 rounds as fma(b, s, a) (True: ATen's vectorised kernel on a host
    with FMA) or as a + b * s (False).  The reference's grey value and its `_blend` are such adds, so their rounding is probed
    once, on 4096 random pairs, and passed to the kernel as its blend form."""
    g = torch.Generator().manual_seed(0)
    a = torch.rand(4096, generator=g) * 255.0
    b = torch.rand(4096, generator=g) * 255.0
    got = a.clone().add_(b, alpha=0.587)
    plain = a + b * torch.tensor(0.587, dtype=torch.float32)  # two separately rounded ops
    return not torch.equal(got, plain)


def _blend_form() -> int:
    return 1 if _add_alpha_fuses() else 0


def _check_color_channels(image: torch.Tensor) -> int:
    c = image.shape[-3]
    if c not in [1, 3]:
        raise TypeError(f"Input image tensor permitted channel values are 1 or 3, but found {c}")
    return int(c)


def _check_color_factor(name: str, factor: float) -> None:
    if name == "hue":
        if not (-0.5 <= factor <= 0.5):
            raise ValueError(f"hue_factor ({factor}) is not in [-0.5, 0.5].")
    elif factor < 0:
        raise ValueError(f"{name}_factor ({factor}) is not non-negative.")


def _color_chain(image: torch.Tensor, ops: Sequence[Tuple[str, float]]) -> torch.Tensor:
    """The ops, in order, on a non-empty float32 / uint8 (..., C, H, W) image with C in {1, 3}: ONE mv_color_chain_* call (a
    chain with contrast runs its mean reduction on the stream first).  The caller has checked the arguments and dropped
    saturation and hue from 1-channel chains."""
    c, h, w = (int(s) for s in image.shape[-3:])
    images = image.numel() // (c * h * w)
    n = len(ops)
    codes = (C.c_int * n)(*[_COLOR_OPS[name] for name, _ in ops])
    factors = (C.c_double * n)(*[float(f) for _, f in ops])
    args = (images, c, h, w, codes, factors, n, _blend_form())
    what = "adjust_" + ops[0][0] if n == 1 else "color_jitter"
    if any(name == "contrast" for name, _ in ops):  # the mean reduction's buffer
        return _lib.launch_image_op("color_chain", image, args, workspace=("color", (images, h, w)), what=what)
    return _lib.launch_image_op("color_chain", image, args + (None, 0), what=what)


def adjust_brightness(inpt: torch.Tensor, brightness_factor: float) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py `adjust_brightness`."""
    kernel = _get_kernel(adjust_brightness, type(inpt))
    return kernel(inpt, brightness_factor=brightness_factor)


@_register_image_and_video(adjust_brightness)
def adjust_brightness_image(image: torch.Tensor, brightness_factor: float) -> torch.Tensor:
    """adjust_brightness_image (_color.py): image.mul(factor).clamp_(0, bound), truncated back to uint8."""
    _check_color_factor("brightness", brightness_factor)
    _check_color_channels(image)
    _lib.require_f32_u8(image, "adjust_brightness")
    if image.dtype == torch.uint8 and isinstance(brightness_factor, int) and brightness_factor > 1:
        # image.mul(int) stays uint8 in the reference and wraps modulo 256 before the clamp
        raise NotImplementedError(f"adjust_brightness: an integer factor ({brightness_factor}) on a uint8 image multiplies "
                                  "modulo 256 in the reference, which is not on the MI355X path; pass a float factor")
    if image.numel() == 0:
        return torch.empty_like(image)
    return _color_chain(image, [("brightness", brightness_factor)])


adjust_brightness_video = adjust_brightness_image


def adjust_saturation(inpt: torch.Tensor, saturation_factor: float) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py `adjust_saturation`."""
    kernel = _get_kernel(adjust_saturation, type(inpt))
    return kernel(inpt, saturation_factor=saturation_factor)


@_register_image_and_video(adjust_saturation)
def adjust_saturation_image(image: torch.Tensor, saturation_factor: float) -> torch.Tensor:
    """adjust_saturation_image (_color.py): _blend with the per-pixel grey value (floored for uint8); 1-channel images are
    returned as they are."""
    _check_color_factor("saturation", saturation_factor)
    c = _check_color_channels(image)
    if c == 1:  # the reference matches PIL here
        return image
    _lib.require_f32_u8(image, "adjust_saturation")
    if image.numel() == 0:
        return torch.empty_like(image)
    return _color_chain(image, [("saturation", saturation_factor)])


adjust_saturation_video = adjust_saturation_image


def adjust_contrast(inpt: torch.Tensor, contrast_factor: float) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py `adjust_contrast`."""
    kernel = _get_kernel(adjust_contrast, type(inpt))
    return kernel(inpt, contrast_factor=contrast_factor)


@_register_image_and_video(adjust_contrast)
def adjust_contrast_image(image: torch.Tensor, contrast_factor: float) -> torch.Tensor:
    """adjust_contrast_image (_color.py): _blend with the mean of the grey image over dims (-3, -2, -1) -- per image, per
    frame of a video; a 1-channel image is its own grey image."""
    _check_color_factor("contrast", contrast_factor)
    _check_color_channels(image)
    _lib.require_f32_u8(image, "adjust_contrast")
    if image.numel() == 0:
        return torch.empty_like(image)
    return _color_chain(image, [("contrast", contrast_factor)])


adjust_contrast_video = adjust_contrast_image


def adjust_hue(inpt: torch.Tensor, hue_factor: float) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py `adjust_hue`."""
    kernel = _get_kernel(adjust_hue, type(inpt))
    return kernel(inpt, hue_factor=hue_factor)


@_register_image_and_video(adjust_hue)
def adjust_hue_image(image: torch.Tensor, hue_factor: float) -> torch.Tensor:
    """adjust_hue_image (_color.py): _rgb_to_hsv, h = (h + hue_factor) mod 1, _hsv_to_rgb, with uint8 scaled in and out as
    to_dtype_image(scale=True) does; 1-channel and empty images are returned as they are."""
    _check_color_factor("hue", hue_factor)
    c = _check_color_channels(image)
    if c == 1:  # the reference matches PIL here
        return image
    if image.numel() == 0:
        return image
    _lib.require_f32_u8(image, "adjust_hue")
    return _color_chain(image, [("hue", hue_factor)])


adjust_hue_video = adjust_hue_image


def color_jitter_image(image: torch.Tensor, ops: Sequence[Tuple[str, float]]) -> torch.Tensor:
    """The reference's loop of single `adjust_*_image` calls (v2.ColorJitter._transform) over (name, factor) pairs, as ONE
    mv_color_chain_* call on a non-empty float32 / uint8 image on the device: the same bits as the loop.  Names are
    "brightness", "contrast", "saturation" and "hue"."""
    for name, factor in ops:
        if name not in _COLOR_OPS:
            raise ValueError(f"unknown colour op {name!r}")
        _check_color_factor(name, factor)
    if not ops:
        return image
    c = _check_color_channels(image)
    if c == 1:  # saturation and hue return 1-channel images unchanged
        ops = [(name, f) for name, f in ops if name in ("brightness", "contrast")]
        if not ops:
            return image
    _lib.require_f32_u8(image, "ColorJitter")
    if image.numel() == 0:
        raise ValueError("color_jitter_image: empty images take the reference's loop of single calls")
    return _color_chain(image, list(ops))


def rgb_to_grayscale(inpt: torch.Tensor, num_output_channels: int = 1) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py `rgb_to_grayscale`."""
    kernel = _get_kernel(rgb_to_grayscale, type(inpt))
    return kernel(inpt, num_output_channels=num_output_channels)


@_register_kernel_internal(rgb_to_grayscale, torch.Tensor)
@_register_kernel_internal(rgb_to_grayscale, tv_tensors.Image)
def rgb_to_grayscale_image(image: torch.Tensor, num_output_channels: int = 1) -> torch.Tensor:
    """rgb_to_grayscale_image (_color.py): the grey value r * 0.2989 + g * 0.587 + b * 0.114 (truncated for uint8) in 1 or 3
    planes; a 1-channel image is cloned or repeated."""
    if num_output_channels not in (1, 3):
        raise ValueError(f"num_output_channels must be 1 or 3, got {num_output_channels}.")
    c = _check_color_channels(image)
    if c == 1:
        if num_output_channels == 1:
            return image.clone()
        s = [1] * image.ndim
        s[-3] = 3
        return image.repeat(s)
    _lib.require_f32_u8(image, "rgb_to_grayscale")
    h, w = (int(d) for d in image.shape[-2:])
    out_shape = tuple(image.shape[:-3]) + (num_output_channels, h, w)
    if image.numel() == 0:
        return torch.empty(out_shape, dtype=image.dtype, device=image.device)
    images = image.numel() // (3 * h * w)
    return _lib.launch_image_op("rgb_to_grayscale", image, (images, h, w, num_output_channels, _blend_form()),
                                out_shape=out_shape)


if _pil.PIL is not None:
    for _f in (adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue, rgb_to_grayscale):
        _unsupported(_f, _pil.PIL.Image.Image, "PIL images go through Pillow's ImageEnhance in the reference, whose results "
                                               "the tensor formula does not reproduce; convert with pil_to_tensor and move the "
                                               "tensor to the MI355X")
    del _f


# --------------------------------------------------------------------------------------------- automatic-augmentation ops
# transforms/v2/functional/_color.py invert / posterize / solarize / autocontrast / equalize: what AutoAugment, RandAugment and
# TrivialAugmentWide call besides the geometric and F.adjust_* ops.  Argument checks here, with the reference's error text;
# the pixels go through csrc/autoaug.hip.  Nothing is read back to the host.
_POINT_OPS = {"invert": 0, "posterize": 1, "solarize": 2}


def _pointwise(image: torch.Tensor, op: str, param: float = 0.0) -> torch.Tensor:
    """One mv_pointwise_* call over every element of a non-empty float32 / uint8 image."""
    return _lib.launch_image_op("pointwise", image, (image.numel(), _POINT_OPS[op], float(param)), what=op)


def _plane_op(image: torch.Tensor, name: str) -> torch.Tensor:
    """mv_autocontrast_* / mv_equalize_* on the (H, W) planes of a non-empty float32 / uint8 image, with its workspace."""
    h, w = (int(d) for d in image.shape[-2:])
    planes = image.numel() // (h * w)
    return _lib.launch_image_op(name, image, (planes, h, w), workspace=(name, (planes, h, w)))


def invert(inpt: torch.Tensor) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py `invert`."""
    kernel = _get_kernel(invert, type(inpt))
    return kernel(inpt)


@_register_image_and_video(invert)
def invert_image(image: torch.Tensor) -> torch.Tensor:
    """invert_image (_color.py): float 1.0 - x, uint8 bitwise_not; any number of channels."""
    _lib.require_f32_u8(image, "invert")
    if image.numel() == 0:
        return torch.empty_like(image)
    return _pointwise(image, "invert")


invert_video = invert_image


def posterize(inpt: torch.Tensor, bits: int) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py `posterize`."""
    kernel = _get_kernel(posterize, type(inpt))
    return kernel(inpt, bits=bits)


@_register_image_and_video(posterize)
def posterize_image(image: torch.Tensor, bits: int) -> torch.Tensor:
    """posterize_image (_color.py): float x.mul(2^bits).floor_().clamp_(0, 2^bits - 1).mul_(2^-bits); uint8 keeps the top
    `bits` bits, and bits >= 8 returns the image itself."""
    if not isinstance(bits, int) or not 0 <= bits <= 8:
        raise TypeError(f"bits must be a positive integer in the range [0, 8], got {bits} instead.")
    _lib.require_f32_u8(image, "posterize")
    if image.dtype == torch.uint8 and bits >= 8:
        return image
    if image.numel() == 0:
        return torch.empty_like(image)
    return _pointwise(image, "posterize", bits)


posterize_video = posterize_image


def solarize(inpt: torch.Tensor, threshold: float) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py `solarize`."""
    kernel = _get_kernel(solarize, type(inpt))
    return kernel(inpt, threshold=threshold)


@_register_image_and_video(solarize)
def solarize_image(image: torch.Tensor, threshold: float) -> torch.Tensor:
    """solarize_image (_color.py): torch.where(image >= threshold, invert(image), image).  The comparison is torch's: a
    float threshold is rounded to float32 (a uint8 image is promoted to float32 against it); an integer threshold against a
    uint8 image is first wrapped to uint8."""
    _lib.require_f32_u8(image, "solarize")
    if threshold > _lib.max_value(image.dtype):
        raise TypeError(f"Threshold should be less or equal the maximum value of the dtype, but got {threshold}")
    if image.numel() == 0:
        return torch.empty_like(image)
    if image.dtype == torch.uint8 and isinstance(threshold, int) and not isinstance(threshold, bool):
        threshold = threshold % 256
    return _pointwise(image, "solarize", float(threshold))


solarize_video = solarize_image


def autocontrast(inpt: torch.Tensor) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py `autocontrast`."""
    kernel = _get_kernel(autocontrast, type(inpt))
    return kernel(inpt)


@_register_image_and_video(autocontrast)
def autocontrast_image(image: torch.Tensor) -> torch.Tensor:
    """autocontrast_image (_color.py): per (image, channel) plane, (x - min) / ((max - min) * (1 / bound)) clamped to
    [0, bound] (uint8 truncated), min = 0 and scale 1 on flat planes; a NaN makes its float plane NaN.  Empty images are
    returned as they are."""
    _check_color_channels(image)
    _lib.require_f32_u8(image, "autocontrast")
    if image.numel() == 0:
        return image
    return _plane_op(image, "autocontrast")


autocontrast_video = autocontrast_image


def equalize(inpt: torch.Tensor) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py `equalize`."""
    kernel = _get_kernel(equalize, type(inpt))
    return kernel(inpt)


@_register_image_and_video(equalize)
def equalize_image(image: torch.Tensor) -> torch.Tensor:
    """equalize_image (_color.py): per (H, W) plane, the 256-bin histogram of the uint8 image (float32: of
    to_dtype(scale=True)), PIL's LUT, planes with step == 0 unequalised; float32 comes back as the uint8 result / 255, so it
    is always quantised to 256 levels.  Float values outside [0, 1] (and NaN), where the reference's float -> uint8 cast is
    undefined, are saturated: below 0 and NaN bin as 0, above 1 as 255.  Empty images are returned as they are."""
    _lib.require_f32_u8(image, "equalize")
    if image.numel() == 0:
        return image
    return _plane_op(image, "equalize")


equalize_video = equalize_image


if _pil.PIL is not None:
    for _f in (invert, posterize, solarize, autocontrast, equalize):
        _unsupported(_f, _pil.PIL.Image.Image, "PIL images go through Pillow's ImageOps in the reference, which this library "
                                               "does not reproduce; convert with pil_to_tensor and move the tensor to the MI355X")
    del _f
