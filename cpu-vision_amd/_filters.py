"""The filters: gaussian_blur and adjust_sharpness of the reference's transforms/v2/functional (_misc.py:75-181,
_color.py:218-288) with their _image / PIL / _video kernels and list-of-frames forms, and the operators on the same primitive
that the reference does not have -- depthwise_conv2d, box_filter, separable_gaussian_blur, sobel, gaussian_sobel.  Every launch
goes through _lib.launch_xy (lists of frames: _lib.launch_frames).

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it; the
INTEGER_BLUR_* switches live there and are read through _lib.switch.
"""
from __future__ import annotations

import functools
import math
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _lib, _pil, tv_tensors
from ._lib import max_value as _max_value
from ._registry import _get_kernel, _register_kernel_internal

# direct 2-D evaluation (the reference's own formulation) up to this many taps; larger float kernels
# run as the fused separable pair (same result to ~1e-7 relative, see DESIGN.md "Numerics")
_DIRECT_2D_MAX_TAPS = 49


# --------------------------------------------------------------------------------------------- taps
def _get_gaussian_kernel1d(kernel_size: int, sigma: float, dtype: torch.dtype = torch.float32,
                           device: Union[str, torch.device] = "cpu") -> torch.Tensor:
    """_misc.py:86-90 -- the same torch ops, so on the host the taps are bit-identical to the reference's."""
    lim = (kernel_size - 1) / (2.0 * math.sqrt(2.0))
    x = torch.linspace(-lim, lim, steps=kernel_size, dtype=dtype, device=device)
    return torch.softmax(x.div(sigma).pow(2).neg(), dim=0)


def _get_gaussian_kernel2d(kernel_size: List[int], sigma: List[float], dtype: torch.dtype = torch.float32,
                           device: Union[str, torch.device] = "cpu") -> torch.Tensor:
    """_misc.py:93-99: kernel_size / sigma are (x, y); the result has shape (ky, kx)."""
    kernel1d_x = _get_gaussian_kernel1d(kernel_size[0], sigma[0], dtype, device)
    kernel1d_y = _get_gaussian_kernel1d(kernel_size[1], sigma[1], dtype, device)
    return kernel1d_y.unsqueeze(-1) * kernel1d_x


@functools.lru_cache(maxsize=256)
def _host_taps(kernel_size: int, sigma: float, v1: bool = False, dtype: torch.dtype = torch.float32):
    """(tensor, ctypes array) of one 1-D Gaussian, cached: a DataLoader calls the same (k, sigma) over and
    over, and building the taps with five torch ops costs more host time than launching the kernel.
    dtype float64: the taps of a float64 image, which the reference builds in the image's dtype (_misc.py:141)."""
    if v1:
        from . import functional_v1
        t = functional_v1._get_gaussian_kernel1d(kernel_size, sigma, dtype)
    else:
        t = _get_gaussian_kernel1d(kernel_size, sigma, dtype)
    return t, (_lib.taps64_from_tensor(t) if dtype == torch.float64 else _lib.taps_from_tensor(t))


def _taps_dtype(image: torch.Tensor) -> torch.dtype:
    return torch.float64 if image.dtype == torch.float64 else torch.float32


# --------------------------------------------------------------------------------------------- plumbing
def _planes(image: torch.Tensor) -> Tuple[int, int, int]:
    h, w = image.shape[-2:]
    planes = 1
    for d in image.shape[:-2]:
        planes *= int(d)
    return planes, int(h), int(w)


def _compute_dtype(image: torch.Tensor) -> str:
    if image.dtype == torch.float32:
        return "f32"
    if image.dtype == torch.uint8:
        return "u8"
    return "float" if image.is_floating_point() else "int"


def _filter_f32_u8(image: torch.Tensor, fn_f32, fn_u8, args, out_shape=None) -> torch.Tensor:
    """Run a filter whose kernels exist for fp32 and uint8 storage: fn_*(x, y, *args, stream), fn_u8 None if there is none.

    fp16 / bf16 are computed in fp32 and narrowed back (the reference computes in the input dtype; fp32 accumulation
    is at least as accurate).  float64 reaches this helper only for the operators that have no float64 kernel
    (box / Sobel / the generic primitive with a float32 weight); gaussian_blur and adjust_sharpness compute float64
    images in float64 (mv_gaussian_blur_f64 / mv_sharpness_f64).
    Other integer dtypes follow the reference's integer recipe: .to(float32) -> filter -> round_() -> .to(dtype).
    """
    _lib.require_device(image)
    kind = _compute_dtype(image)
    if kind == "u8" and fn_u8 is not None:
        return _lib.launch_xy(fn_u8, image, args, out_shape=out_shape, out_dtype=torch.uint8)
    y = _lib.launch_xy(fn_f32, image if kind == "f32" else image.to(torch.float32), args, out_shape=out_shape,
                       out_dtype=torch.float32)
    if kind == "f32":
        return y
    if kind == "float":
        return y.to(image.dtype)
    return y.round_().to(image.dtype)


def _border(border: str) -> int:
    try:
        return _lib.BORDERS[border]
    except KeyError:
        raise ValueError(f"border should be one of {sorted(_lib.BORDERS)}. Got {border!r}") from None


# --------------------------------------------------------------------------------------------- gaussian_blur
def gaussian_blur(inpt: torch.Tensor, kernel_size: List[int], sigma: Optional[List[float]] = None) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_misc.py:75-83."""
    kernel = _get_kernel(gaussian_blur, type(inpt))
    return kernel(inpt, kernel_size=kernel_size, sigma=sigma)


def _check_gaussian_args(kernel_size, sigma):
    """Argument normalisation of gaussian_blur_image, _misc.py:108-133 (same messages)."""
    if isinstance(kernel_size, int):
        kernel_size = [kernel_size, kernel_size]
    elif len(kernel_size) != 2:
        raise ValueError(f"If kernel_size is a sequence its length should be 2. Got {len(kernel_size)}")
    for ksize in kernel_size:
        if ksize % 2 == 0 or ksize < 0:
            raise ValueError(f"kernel_size should have odd and positive integers. Got {kernel_size}")

    if sigma is None:
        sigma = [ksize * 0.15 + 0.35 for ksize in kernel_size]
    else:
        if isinstance(sigma, (list, tuple)):
            length = len(sigma)
            if length == 1:
                s = sigma[0]
                sigma = [s, s]
            elif length != 2:
                raise ValueError(f"If sigma is a sequence, its length should be 2. Got {length}")
        elif isinstance(sigma, (int, float)):
            s = float(sigma)
            sigma = [s, s]
        else:
            raise TypeError(f"sigma should be either float or sequence of floats. Got {type(sigma)}")
    for s in sigma:
        if s <= 0.0:
            raise ValueError(f"sigma should have positive values. Got {sigma}")
    return list(kernel_size), list(sigma)


def _blur_with_taps(image: torch.Tensor, taps_x, taps_y, separable: bool) -> torch.Tensor:
    """pad(reflect) + depthwise conv with the outer-product kernel (or its separable factorisation).
    taps_* are (tensor, ctypes array) pairs from _host_taps."""
    (k1d_x, tx), (k1d_y, ty) = taps_x, taps_y
    kx, ky = k1d_x.numel(), k1d_y.numel()
    h, w = image.shape[-2:]
    if kx // 2 >= w or ky // 2 >= h:
        # ATen's reflection_pad2d message, raised here before any launch
        raise RuntimeError(
            f"Argument #4: Padding size should be less than the corresponding input dimension, but got: padding "
            f"({kx // 2}, {kx // 2}) at dimension 3 of input {list(image.shape)}"
            if kx // 2 >= w else
            f"Argument #6: Padding size should be less than the corresponding input dimension, but got: padding "
            f"({ky // 2}, {ky // 2}) at dimension 2 of input {list(image.shape)}")
    lib = _lib.load()
    planes, h, w = _planes(image)
    args = (planes, h, w, tx, kx, ty, ky)
    huge = max(kx, ky) > _lib.MAX_TAPS_1D
    if huge:  # beyond the 63-tap kernels (ElasticTransform with sigma >= 8): the reference's own single 2-D pass, taps on the device
        k2 = (k1d_y.unsqueeze(-1) * k1d_x).to(image.device).contiguous()
    if image.dtype == torch.float64:
        # float64 images are computed in float64 like the reference's (taps, outer product and accumulation), one 2-D pass
        assert k1d_x.dtype == torch.float64 and k1d_y.dtype == torch.float64
        if huge:
            return _lib.launch_xy(lib.mv_depthwise_conv2d_f64, image, (k2.data_ptr(), planes, h, w, ky, kx, _lib.BORDER_REFLECT))
        return _lib.launch_xy(lib.mv_gaussian_blur_f64, image, args)
    if huge:
        return _filter_f32_u8(image, lib.mv_depthwise_conv2d_f32, lib.mv_depthwise_conv2d_u8,
                              (k2.data_ptr(), 1, planes, h, w, ky, kx, _lib.BORDER_REFLECT))
    if image.dtype in (torch.float16, torch.bfloat16) and not separable:
        # half-precision storage, 2-D pass: fp32 arithmetic inside the tile kernel, one rounding on store -- the same bits as
        # .to(float32) -> filter -> .to(dtype), without the two conversion passes over the image
        return _lib.launch_xy(lib.mv_gaussian_blur_f16 if image.dtype == torch.float16 else lib.mv_gaussian_blur_bf16, image, args)
    if image.dtype != torch.uint8:
        return _filter_f32_u8(image, lib.mv_separable_blur_f32 if separable else lib.mv_gaussian_blur_f32, None, args)
    # large kernels on uint8 storage (SimCLR-style GaussianBlur(23)): the separable pair in fp32, then round_()
    big = separable and max(kx, ky) <= 63 and w >= 8
    if not big and _lib.switch("INTEGER_BLUR_EXACT_2D") and _lib.switch("INTEGER_BLUR_EXACT_FAST"):
        # the reference's integers at the separable pair's cost (mv_gaussian_blur_u8_ws): the pair everywhere, the 2-D chain
        # only for the lane-rows within its error bound of a rounding tie
        _lib.require_device(image)
        ws, ws_ptr, nbytes = _lib.workspace(int(lib.mv_gaussian_blur_u8_workspace_bytes(planes, h, w, kx, ky)), image.device)
        if nbytes:
            return _lib.launch_xy(lib.mv_gaussian_blur_u8_ws, image, args + (ws_ptr, nbytes), out_dtype=torch.uint8)
    return _filter_f32_u8(image, None, lib.mv_separable_blur_u8 if big else lib.mv_gaussian_blur_u8, args)


def _use_separable(kx: int, ky: int, image: torch.Tensor) -> bool:
    """Which formulation gaussian_blur_image runs.  The reference's is one 2-D pass with the outer-product kernel; the
    separable pair (row pass, then column pass, both fp32) agrees with it to <= 2e-7 relative and costs kx + ky instead of
    kx * ky taps.
      float images   2-D while both sides are <= 5 (the templated tile kernels: 3x3, 5x5, 3x5, 5x3, HBM-bound anyway);
                     separable beyond -- 7x7 runs 1.56 -> 1.15 ms and unequal sizes such as (7, 3) or (5, 9), which only had
                     the run-time-size tile kernel, 2.4-3.8 -> 1.1-1.3 ms on 32 x 4K frames.  Widths with W % 4 != 0 keep
                     the 2-D pass while both sides are <= 7 (templated tile kernel, 3.5 TB/s): k_sepfast needs 16-byte
                     rows and the LDS fallback behind it runs at 1.6 TB/s (k_sepstream, sides above 7, takes any width)
      uint8          the reference's single 2-D pass by default (INTEGER_BLUR_EXACT_2D = True: bit-for-bit the reference's
                     integers).  With INTEGER_BLUR_EXACT_2D = False: 2-D for 3x3 (HBM-bound already) and for images narrower
                     than 16 pixels, the fp32 separable pair + one round_() for every larger kernel -- 5x5 / 7x7 are
                     VALU-bound as one 25- / 49-tap chain (0.54 / 0.96 ms on 32 x 4K uint8) and need 10 / 14 taps as a pair;
                     the pair differs from the 2-D sum only at exact rounding ties (~1e-5 of the pixels by 1 LSB, inside the
                     reference's own atol = 1, test_transforms_v2.py:3309)
      other integers always the 2-D pass."""
    if image.is_floating_point():
        if kx <= 5 and ky <= 5:
            return False
        if image.dtype in (torch.float16, torch.bfloat16) and kx <= 11 and ky <= 11:
            return False  # half-precision storage runs fused in the 2-D tile kernel (no fp32 copies of the image)
        odd_width = image.ndim >= 1 and image.shape[-1] % 4 != 0
        return not (odd_width and kx <= 7 and ky <= 7)
    if image.dtype != torch.uint8 or _lib.switch("INTEGER_BLUR_EXACT_2D"):
        return False
    wide = image.ndim >= 1 and image.shape[-1] >= 16  # the 16-pixel-per-lane kernels
    return kx > 7 or ky > 7 or ((kx > 3 or ky > 3) and wide)


@_register_kernel_internal(gaussian_blur, torch.Tensor)
@_register_kernel_internal(gaussian_blur, tv_tensors.Image)
def gaussian_blur_image(image: torch.Tensor, kernel_size: List[int], sigma: Optional[List[float]] = None) -> torch.Tensor:
    """gaussian_blur_image (_misc.py:102-165): (..., C, H, W) of any dtype -> same shape and dtype.

    Differences from the reference, all below its own test tolerance: the reflect border is resolved inside
    the kernel (no padded copy), fp16 / bf16 images accumulate in fp32 (float64 images in float64, float32 in float32,
    like the reference), and larger float32 kernels run as the fused separable pair (`_use_separable`).
    """
    kernel_size, sigma = _check_gaussian_args(kernel_size, sigma)
    if image.numel() == 0:
        return image
    image.shape[-3]  # noqa: B018 -- (..., C, H, W) required, IndexError like the reference otherwise
    k1d_x = _host_taps(kernel_size[0], float(sigma[0]), False, _taps_dtype(image))
    k1d_y = _host_taps(kernel_size[1], float(sigma[1]), False, _taps_dtype(image))
    separable = _use_separable(kernel_size[0], kernel_size[1], image)
    return _blur_with_taps(image, k1d_x, k1d_y, separable)


def _gaussian_blur_image_pil(image, kernel_size: List[int], sigma: Optional[List[float]] = None):
    """_gaussian_blur_image_pil (_misc.py:169-174): pil_to_tensor -> gaussian_blur_image -> to_pil_image(mode=image.mode).
    The tensor goes to the current HIP device for the kernel and comes back (PCIe both ways: a DataLoader that decodes to
    PIL should convert once and keep the batch on the device -- see DESIGN.md "Host buffers")."""
    t_img = _pil.pil_to_tensor(image)
    output = gaussian_blur_image(t_img.to(_pil.device_for_host_inputs()), kernel_size=kernel_size, sigma=sigma)
    return _pil.to_pil_image(output.cpu(), mode=image.mode)


if _pil.PIL is not None:
    _register_kernel_internal(gaussian_blur, _pil.PIL.Image.Image)(_gaussian_blur_image_pil)


@_register_kernel_internal(gaussian_blur, tv_tensors.Video)
def gaussian_blur_video(video: torch.Tensor, kernel_size: List[int], sigma: Optional[List[float]] = None) -> torch.Tensor:
    return gaussian_blur_image(video, kernel_size, sigma)


# --------------------------------------------------------------------------------------------- adjust_sharpness
def adjust_sharpness(inpt: torch.Tensor, sharpness_factor: float) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_color.py:218-226."""
    kernel = _get_kernel(adjust_sharpness, type(inpt))
    return kernel(inpt, sharpness_factor=sharpness_factor)


def _sharpness(image: torch.Tensor, sharpness_factor: float, v1: bool) -> torch.Tensor:
    lib = _lib.load()
    _lib.require_device(image)
    planes, h, w = _planes(image)
    f = float(sharpness_factor)
    if image.dtype == torch.uint8:
        return _lib.launch_xy(lib.mv_sharpness_u8, image, (planes, h, w, f, int(v1)))
    if image.dtype == torch.float64:  # computed in float64 like the reference (kernel dtype = image dtype, _color.py:246)
        return _lib.launch_xy(lib.mv_sharpness_f64, image, (planes, h, w, f, int(v1)))
    y = _lib.launch_xy(lib.mv_sharpness_f32, image.to(torch.float32),
                       (planes, h, w, f, int(v1), float(_max_value(image.dtype)), int(not image.is_floating_point())))
    return y if image.dtype == torch.float32 else y.to(image.dtype)


@_register_kernel_internal(adjust_sharpness, torch.Tensor)
@_register_kernel_internal(adjust_sharpness, tv_tensors.Image)
def adjust_sharpness_image(image: torch.Tensor, sharpness_factor: float) -> torch.Tensor:
    """adjust_sharpness_image (_color.py:229-280): valid 3x3 smoothing, in-place blend, clamp -- one kernel."""
    num_channels, height, width = image.shape[-3:]
    if num_channels not in (1, 3):
        raise TypeError(f"Input image tensor can have 1 or 3 channels, but found {num_channels}")
    if sharpness_factor < 0:
        raise ValueError(f"sharpness_factor ({sharpness_factor}) is not non-negative.")
    if image.numel() == 0 or height <= 2 or width <= 2:
        return image
    return _sharpness(image, sharpness_factor, v1=False)


def _adjust_sharpness_image_pil(image, sharpness_factor: float):
    """The reference registers PIL's own ImageEnhance.Sharpness here (_color.py:283 -> _functional_pil.py:113-121): SMOOTH
    filter, blend with the original, alpha band kept.  The uint8 tensor kernel reproduces PIL's result exactly
    (tests/golden: PIL-exact vectors), so the PIL entry is that kernel around a conversion; an alpha band passes through."""
    if not _pil.is_pil_image(image):
        raise TypeError(f"img should be PIL Image. Got {type(image)}")
    t = _pil.pil_to_tensor(image)
    if image.mode in ("LA", "RGBA"):
        color, alpha = t[:-1], t[-1:]
    else:
        color, alpha = t, None
    if color.shape[0] not in (1, 3) or color.dtype != torch.uint8:
        raise TypeError(f"adjust_sharpness on a PIL image supports modes L, LA, RGB and RGBA, got {image.mode}")
    out = adjust_sharpness_image(color.contiguous().to(_pil.device_for_host_inputs()), sharpness_factor).cpu()
    if alpha is not None:
        out = torch.cat([out, alpha], 0)
    return _pil.to_pil_image(out, mode=image.mode)


if _pil.PIL is not None:
    _register_kernel_internal(adjust_sharpness, _pil.PIL.Image.Image)(_adjust_sharpness_image_pil)


@_register_kernel_internal(adjust_sharpness, tv_tensors.Video)
def adjust_sharpness_video(video: torch.Tensor, sharpness_factor: float) -> torch.Tensor:
    return adjust_sharpness_image(video, sharpness_factor=sharpness_factor)


# --------------------------------------------------------------------------------------------- lists of frames, one launch
def _same_frames(frames: Sequence[torch.Tensor]) -> bool:
    f0 = frames[0]
    return all(isinstance(f, torch.Tensor) and f.is_cuda and f.device == f0.device and f.dtype == f0.dtype
               and f.shape == f0.shape for f in frames)


def _frames_call(frames: Sequence[torch.Tensor], fn_name: str, args_of):
    """Run one mv_*_v launch over separately allocated, equally shaped frames; returns views of one output batch."""
    return _lib.launch_frames(getattr(_lib.load(), fn_name), frames, (*_planes(frames[0]), *args_of()))


def gaussian_blur_frames(frames: Sequence[torch.Tensor], kernel_size: List[int], sigma: Optional[List[float]] = None
                         ) -> List[torch.Tensor]:
    """gaussian_blur_image over a LIST of separately allocated frames (what a DataLoader hands to a transform,
    transforms/v2/_transform.py:40-55).  Equally shaped float32 / uint8 frames on one device go through ONE launch
    (mv_gaussian_blur_*_v / mv_separable_blur_*_v, whichever formulation gaussian_blur_image runs for that size: per-frame
    base pointers in the kernel arguments, no copy of the frames); anything else is a loop over gaussian_blur_image.
    Results equal the per-frame calls bit for bit."""
    frames = list(frames)
    if not frames:
        return []
    kernel_size, sigma = _check_gaussian_args(kernel_size, sigma)
    f0 = frames[0]
    kx, ky = kernel_size
    batched = (len(frames) > 1 and _same_frames(frames) and f0.dtype in (torch.float32, torch.uint8) and f0.ndim >= 3
               and f0.numel() > 0 and kx // 2 < f0.shape[-1] and ky // 2 < f0.shape[-2] and max(kx, ky) <= _lib.MAX_TAPS_1D)
    separable = batched and _use_separable(kx, ky, f0)
    if separable and f0.dtype == torch.uint8 and f0.shape[-1] < (8 if max(kx, ky) > 7 else 16):
        batched = False  # (gaussian_blur_image takes the 2-D pass there)
    if batched and not separable and max(kx, ky) > 11:
        batched = False
    if not batched:
        return [gaussian_blur_image(f, kernel_size, sigma) for f in frames]
    (_, tx), (_, ty) = _host_taps(kx, float(sigma[0])), _host_taps(ky, float(sigma[1]))
    name = ("mv_separable_blur_" if separable else "mv_gaussian_blur_") + ("f32_v" if f0.dtype == torch.float32 else "u8_v")
    return _frames_call(frames, name, lambda: (tx, kx, ty, ky))


def adjust_sharpness_frames(frames: Sequence[torch.Tensor], sharpness_factor: float) -> List[torch.Tensor]:
    """adjust_sharpness_image over a list of separately allocated frames: one launch for equally shaped float32 / uint8
    frames (mv_sharpness_*_v), a loop otherwise."""
    frames = list(frames)
    if not frames:
        return []
    f0 = frames[0]
    batched = (len(frames) > 1 and _same_frames(frames) and f0.dtype in (torch.float32, torch.uint8) and f0.ndim >= 3
               and f0.shape[-3] in (1, 3) and f0.numel() > 0 and f0.shape[-1] > 2 and f0.shape[-2] > 2 and sharpness_factor >= 0)
    if not batched:
        return [adjust_sharpness_image(f, sharpness_factor) for f in frames]
    f = float(sharpness_factor)
    if f0.dtype == torch.uint8:
        return _frames_call(frames, "mv_sharpness_u8_v", lambda: (f, 0))
    return _frames_call(frames, "mv_sharpness_f32_v", lambda: (f, 0, 1.0, 0))


# --------------------------------------------------------------------------------------------- the primitive, exposed
def depthwise_conv2d(image: torch.Tensor, weight: torch.Tensor, border: str = "reflect") -> torch.Tensor:
    """[pad(border)] + conv2d(image, weight.expand(C,1,ky,kx), groups=C): the primitive every filter of the
    reference is built on (_misc.py:153-155).  `weight` is a (ky, kx) tensor (host or device)."""
    if weight.ndim != 2:
        raise ValueError(f"weight should be a 2-D (ky, kx) tensor. Got shape {tuple(weight.shape)}")
    ky, kx = int(weight.shape[0]), int(weight.shape[1])
    if ky % 2 == 0 or kx % 2 == 0:
        raise ValueError(f"kernel size must be odd and positive, got ({ky}, {kx})")
    b = _border(border)
    if image.numel() == 0:
        return image
    lib = _lib.load()
    planes, h, w = _planes(image)
    if b == _lib.BORDER_VALID:
        if ky > h or kx > w:
            raise ValueError(f"valid conv: kernel ({ky}, {kx}) larger than image ({h}, {w})")
        out_shape = tuple(image.shape[:-2]) + (h - ky + 1, w - kx + 1)
    else:
        out_shape = None
    if image.dtype == torch.float64:
        # a float64 image is filtered in float64, like conv2d of a float64 tensor (the weight is widened exactly if it is float32)
        _lib.require_device(image)
        wd = _lib.table_on(weight, image.device, torch.float64)
        return _lib.launch_xy(lib.mv_depthwise_conv2d_f64, image, (wd.data_ptr(), planes, h, w, ky, kx, b), out_shape=out_shape,
                              out_dtype=torch.float64)
    on_device = ky * kx > _lib.MAX_HOST_TAPS_2D
    if on_device:
        wt = _lib.table_on(weight, image.device, torch.float32)
        wp = wt.data_ptr()
    else:
        wp = _lib.taps_from_tensor(weight)
    return _filter_f32_u8(image, lib.mv_depthwise_conv2d_f32, lib.mv_depthwise_conv2d_u8,
                          (wp, int(on_device), planes, h, w, ky, kx, b), out_shape)


def box_filter(image: torch.Tensor, kernel_size: Union[int, Sequence[int]] = 3, border: str = "reflect") -> torch.Tensor:
    """k x k mean filter (BASELINE cfg1): the primitive with w = 1/(kx*ky)."""
    if isinstance(kernel_size, int):
        kernel_size = [kernel_size, kernel_size]
    kx, ky = kernel_size
    w = torch.full((ky, kx), 1.0 / float(kx * ky), dtype=torch.float32)
    return depthwise_conv2d(image, w, border)


def separable_gaussian_blur(image: torch.Tensor, kernel_size: List[int], sigma: Optional[List[float]] = None) -> torch.Tensor:
    """Gaussian blur as the fused (1 x kx) then (ky x 1) pair of the primitive (BASELINE cfg3); float images."""
    kernel_size, sigma = _check_gaussian_args(kernel_size, sigma)
    if image.numel() == 0:
        return image
    k1d_x = _host_taps(kernel_size[0], float(sigma[0]))
    k1d_y = _host_taps(kernel_size[1], float(sigma[1]))
    if not image.is_floating_point():
        raise TypeError(f"separable_gaussian_blur expects a floating point image. Got {image.dtype}")
    return _blur_with_taps(image, k1d_x, k1d_y, separable=True)


def _pair_f32(image: torch.Tensor, fn, args, out_shape=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fn(x, gx, gy, *args, stream) on a floating image, computed in float32 and narrowed back."""
    _lib.require_device(image)
    if not image.is_floating_point():
        raise TypeError(f"expected a floating point image. Got {image.dtype}")
    gx, gy = _lib.launch_xy(fn, image.to(torch.float32), args, out_shape=out_shape, out_dtype=torch.float32, pair=True)
    if image.dtype != torch.float32:
        gx, gy = gx.to(image.dtype), gy.to(image.dtype)
    return gx, gy


def sobel(image: torch.Tensor, border: str = "reflect") -> Tuple[torch.Tensor, torch.Tensor]:
    """(gx, gy): the primitive with taps [[-1,0,1],[-2,0,2],[-1,0,1]] and its transpose (cross-correlation)."""
    b = _border(border)
    lib = _lib.load()
    planes, h, w = _planes(image)
    if image.numel() == 0:
        return image, image
    out_shape = tuple(image.shape[:-2]) + (h - 2, w - 2) if b == _lib.BORDER_VALID else None
    return _pair_f32(image, lib.mv_sobel_f32, (planes, h, w, b), out_shape)


def gaussian_sobel(image: torch.Tensor, kernel_size: List[int], sigma: Optional[List[float]] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """BASELINE cfg3 as one kernel: separable Gaussian (reflect) then Sobel (reflect) of the blurred image."""
    kernel_size, sigma = _check_gaussian_args(kernel_size, sigma)
    if image.numel() == 0:
        return image, image
    (k1d_x, tx), (k1d_y, ty) = _host_taps(kernel_size[0], float(sigma[0])), _host_taps(kernel_size[1], float(sigma[1]))
    planes, h, w = _planes(image)
    return _pair_f32(image, _lib.load().mv_gaussian_sobel_f32, (planes, h, w, tx, k1d_x.numel(), ty, k1d_y.numel()))
