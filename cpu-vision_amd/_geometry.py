"""The grid transforms of the v2 surface -- the reference's transforms/v2/functional/_geometry.py elastic / affine / rotate /
perspective with their _image / _mask / _video kernels: argument checks and host math here, with the reference's error text;
the resampling is one launch of csrc/elastic.hip or csrc/warp.hip per call (DESIGN.md sections 3.13 and 3.14).

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it.
"""
from __future__ import annotations

import functools
import math
import numbers
from typing import List, Optional, Tuple

import torch

from . import _lib, _pil, tv_tensors
from ._registry import _get_kernel, _register_image_and_video, _register_kernel_internal, _register_mask, _unsupported


# --------------------------------------------------------------------------------------------- elastic (v2 surface)
def elastic(inpt: torch.Tensor, displacement: torch.Tensor, interpolation="bilinear", fill=None) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py `elastic`: resample `inpt` at identity grid + displacement."""
    kernel = _get_kernel(elastic, type(inpt))
    return kernel(inpt, displacement=displacement, interpolation=interpolation, fill=fill)


elastic_transform = elastic

# Pillow's integer constants (transforms/functional.py `_interpolation_modes_from_int`)
_PIL_INTERPOLATION = {0: "nearest", 2: "bilinear", 3: "bicubic", 4: "box", 5: "hamming", 1: "lanczos"}
_ELASTIC_MODES = {"bilinear": 0, "nearest": 1}


def _interpolation_name(interpolation) -> str:
    """_check_interpolation (_geometry.py): an InterpolationMode, its string value or a Pillow integer constant -> the mode's
    string value."""
    if isinstance(interpolation, int) and not isinstance(interpolation, bool):
        if interpolation not in _PIL_INTERPOLATION:
            raise ValueError(f"Interpolation mode {interpolation} is not supported.")
        return _PIL_INTERPOLATION[interpolation]
    name = getattr(interpolation, "value", interpolation)
    if not isinstance(name, str):
        raise ValueError(f"Argument interpolation should be an `InterpolationMode` or a corresponding Pillow integer constant, "
                         f"but got {interpolation}.")
    return name


@functools.lru_cache(maxsize=64)
def _identity_grid_vectors(h: int, w: int, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two linspace vectors of the reference's `_create_identity_grid`, computed by torch on the host exactly as the
    reference computes them (ATen's vectorised arange: its bits are not the closed form start + i * step) and kept on the
    device: W + H floats per frame size."""
    bx = torch.linspace((-w + 1) / w, (w - 1) / w, w, dtype=torch.float32)
    by = torch.linspace((-h + 1) / h, (h - 1) / h, h, dtype=torch.float32)
    return bx.to(device), by.to(device)


def _elastic_fill(fill, c: int):
    """(host float array, channels) of the fill blend, or (None, 1).  The reference builds
    torch.tensor(fill_list, dtype=float32).view(1, -1, 1, 1) and broadcasts it against C channels."""
    if fill is None:
        return None, 1
    values = [float(v) for v in fill] if isinstance(fill, (tuple, list)) else [float(fill)]
    if len(values) not in (1, c):
        raise RuntimeError(f"The size of tensor a ({c}) must match the size of tensor b ({len(values)}) at non-singleton "
                           "dimension 1: fill needs one value or one per channel")
    return _lib.taps(values), len(values)


@_register_image_and_video(elastic)
def elastic_image(image: torch.Tensor, displacement: torch.Tensor, interpolation="bilinear", fill=None) -> torch.Tensor:
    """elastic_image (_geometry.py) on (..., C, H, W) float32 / uint8 images: grid_sample(image, identity grid +
    displacement, mode, padding_mode="zeros", align_corners=False) with the fill blend of the reference's ones-mask, as ONE
    launch (mv_elastic_*) over every plane -- the reference's per-pixel arithmetic, bit for bit.
    The identity grid is never materialised: the kernel adds the displacement to the two cached linspace vectors."""
    if not isinstance(displacement, torch.Tensor):
        raise TypeError("Argument displacement should be a Tensor")
    mode = _interpolation_name(interpolation)
    if image.ndim < 3:
        raise ValueError(f"Expected tensor to be a tensor image of size (..., C, H, W). Got {tuple(image.shape)}.")
    h, w = int(image.shape[-2]), int(image.shape[-1])
    expected_shape = (1, h, w, 2)
    if expected_shape != displacement.shape:
        raise ValueError(f"Argument displacement shape should be {expected_shape}, but given {displacement.shape}")
    if mode not in _ELASTIC_MODES:
        raise NotImplementedError(f"elastic: interpolation {mode!r} is not on the MI355X path (bilinear and nearest are)")
    _lib.require_f32_u8(image, "elastic", allow_bool=True)
    c = int(image.shape[-3])
    fill_arr, fill_channels = _elastic_fill(fill, c)
    if image.numel() == 0:
        return image
    _lib.require_device(image)
    _lib.require_device(displacement, "displacement")
    planes = image.numel() // (h * w)
    bx, by = _identity_grid_vectors(h, w, image.device)
    d = displacement.detach().to(dtype=torch.float32, device=image.device)  # the reference's .to(dtype, device): no copy when it fits
    args = (planes, fill_channels, h, w, bx.data_ptr(), by.data_ptr(), d.data_ptr(), d.stride(1), d.stride(2), d.stride(3),
            _ELASTIC_MODES[mode], fill_arr)
    return _lib.launch_image_op("elastic", image, args, allow_bool=True, deps=(displacement,))


def _elastic_image_pil(image, displacement: torch.Tensor, interpolation="bilinear", fill=None):
    """_elastic_image_pil (_geometry.py): pil_to_tensor -> elastic_image -> to_pil_image(mode=image.mode), the tensor on the
    current HIP device for the kernel."""
    t_img = _pil.pil_to_tensor(image)
    output = elastic_image(t_img.to(_pil.device_for_host_inputs()), displacement=displacement, interpolation=interpolation,
                           fill=fill)
    return _pil.to_pil_image(output.cpu(), mode=image.mode)


if _pil.PIL is not None:
    _register_kernel_internal(elastic, _pil.PIL.Image.Image)(_elastic_image_pil)


def _nearest_on_mask(image_kernel, mask: torch.Tensor, *args, **kwargs) -> torch.Tensor:
    """The `*_mask` kernels of _geometry.py: the image kernel with nearest interpolation, a channel dimension added below
    3-D."""
    needs_squeeze = mask.ndim < 3
    if needs_squeeze:
        mask = mask.unsqueeze(0)
    output = image_kernel(mask, *args, interpolation="nearest", **kwargs)
    return output.squeeze(0) if needs_squeeze else output


@_register_mask(elastic)
def elastic_mask(mask: torch.Tensor, displacement: torch.Tensor, fill=None) -> torch.Tensor:
    return _nearest_on_mask(elastic_image, mask, displacement=displacement, fill=fill)


@_register_kernel_internal(elastic, tv_tensors.BoundingBoxes, tv_tensor_wrapper=False)
def _elastic_bounding_boxes_dispatch(inpt: torch.Tensor, displacement: torch.Tensor, **kwargs) -> torch.Tensor:
    """Boxes are not warped here: passed through, they would come back unmoved -- silently wrong -- so they raise."""
    raise NotImplementedError("elastic: warping BoundingBoxes (elastic_bounding_boxes) is not implemented on the MI355X path")


elastic_video = elastic_image


# --------------------------------------------------------------------------------------------- affine / rotate / perspective
# (v2 surface).  The host math below is the reference's, with its own ops on the CPU (transforms/functional.py
# _get_inverse_affine_matrix / _get_perspective_coeffs, v2/functional/_geometry.py _affine_parse_args /
# _compute_affine_output_size / _perspective_coefficients / _assert_grid_transform_inputs / _affine_grid / _perspective_grid);
# the grid itself is computed per pixel by k_warp (csrc/warp.hip).
_WARP_KINDS = {"affine": 0, "perspective": 1}
# ATen's bmm takes its naive loop -- plain sums, no fma -- below this many multiply-adds (contraction 3 x oh*ow x 2); above
# it the rounding is the BLAS kernel's (_blocked_bmm_fuses)
_BMM_NAIVE_LIMIT = 400


def _affine_parse_args(angle, translate, scale, shear, center=None):
    """_affine_parse_args (_geometry.py); the interpolation is checked by the caller."""
    if not isinstance(angle, (int, float)):
        raise TypeError("Argument angle should be int or float")
    if not isinstance(translate, (list, tuple)):
        raise TypeError("Argument translate should be a sequence")
    if len(translate) != 2:
        raise ValueError("Argument translate should be a sequence of length 2")
    if scale <= 0.0:
        raise ValueError("Argument scale should be positive")
    if not isinstance(shear, (numbers.Number, (list, tuple))):
        raise TypeError("Shear should be either a single value or a sequence of two values")
    if isinstance(angle, int):
        angle = float(angle)
    if isinstance(translate, tuple):
        translate = list(translate)
    if isinstance(shear, numbers.Number):
        shear = [shear, 0.0]
    if isinstance(shear, tuple):
        shear = list(shear)
    if len(shear) == 1:
        shear = [shear[0], shear[0]]
    if len(shear) != 2:
        raise ValueError(f"Shear should be a sequence containing two values. Got {shear}")
    if center is not None:
        if not isinstance(center, (list, tuple)):
            raise TypeError("Argument center should be a sequence")
        center = [float(c) for c in center]
    return angle, translate, shear, center


def _get_inverse_affine_matrix(center: List[float], angle: float, translate: List[float], scale: float,
                               shear: List[float]) -> List[float]:
    """transforms/functional.py `_get_inverse_affine_matrix` (inverted=True): RSS^-1 * C^-1 * T^-1, then C."""
    rot = math.radians(angle)
    sx = math.radians(shear[0])
    sy = math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    matrix = [d, -b, 0.0, -c, a, 0.0]
    matrix = [x / scale for x in matrix]
    matrix[2] += matrix[0] * (-cx - tx) + matrix[1] * (-cy - ty)
    matrix[5] += matrix[3] * (-cx - tx) + matrix[4] * (-cy - ty)
    matrix[2] += cx
    matrix[5] += cy
    return matrix


def _compute_affine_output_size(matrix: List[float], w: int, h: int) -> Tuple[int, int]:
    """_compute_affine_output_size (_geometry.py, tensor form): the (w, h) of rotate's `expand` canvas."""
    half_w = 0.5 * w
    half_h = 0.5 * h
    pts = torch.tensor([[-half_w, -half_h, 1.0], [-half_w, half_h, 1.0], [half_w, half_h, 1.0], [half_w, -half_h, 1.0]])
    theta = torch.tensor(matrix, dtype=torch.float).view(2, 3)
    new_pts = torch.matmul(pts, theta.T)
    min_vals, max_vals = new_pts.aminmax(dim=0)
    halfs = torch.tensor((half_w, half_h))
    min_vals.add_(halfs)
    max_vals.add_(halfs)
    tol = 1e-4  # truncate to 1e-4 so that ceil does not turn X.00000000001 into X + 1
    inv_tol = 1.0 / tol
    cmax = max_vals.mul_(inv_tol).trunc_().mul_(tol).ceil_()
    cmin = min_vals.mul_(inv_tol).trunc_().mul_(tol).floor_()
    size = cmax.sub_(cmin)
    return int(size[0]), int(size[1])


def _get_perspective_coeffs(startpoints: List[List[int]], endpoints: List[List[int]]) -> List[float]:
    """transforms/functional.py `_get_perspective_coeffs`: the 8 coefficients mapping endpoints to startpoints, by least
    squares in float64, rounded to float32."""
    if len(startpoints) != 4 or len(endpoints) != 4:
        raise ValueError(
            f"Please provide exactly four corners, got {len(startpoints)} startpoints and {len(endpoints)} endpoints.")
    a_matrix = torch.zeros(2 * len(startpoints), 8, dtype=torch.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a_matrix[2 * i, :] = torch.tensor([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]])
        a_matrix[2 * i + 1, :] = torch.tensor([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]])
    b_matrix = torch.tensor(startpoints, dtype=torch.float64).view(8)
    res = torch.linalg.lstsq(a_matrix, b_matrix, driver="gels").solution.to(torch.float32)
    return res.tolist()


def _perspective_coefficients(startpoints, endpoints, coefficients) -> List[float]:
    """_perspective_coefficients (_geometry.py)."""
    if coefficients is not None:
        if startpoints is not None and endpoints is not None:
            raise ValueError("The startpoints/endpoints and the coefficients shouldn't be defined concurrently.")
        elif len(coefficients) != 8:
            raise ValueError("Argument coefficients should have 8 float values")
        return coefficients
    elif startpoints is not None and endpoints is not None:
        return _get_perspective_coeffs(startpoints, endpoints)
    raise ValueError("Either the startpoints/endpoints or the coefficients must have non `None` values.")


def _assert_grid_transform_inputs(image: torch.Tensor, matrix: Optional[List[float]], interpolation: str, fill,
                                  supported_interpolation_modes: List[str], coeffs: Optional[List[float]] = None) -> None:
    """_assert_grid_transform_inputs (_geometry.py)."""
    if matrix is not None:
        if not isinstance(matrix, list):
            raise TypeError("Argument matrix should be a list")
        elif len(matrix) != 6:
            raise ValueError("Argument matrix should have 6 float values")
    if coeffs is not None and len(coeffs) != 8:
        raise ValueError("Argument coeffs should have 8 float values")
    if fill is not None:
        if isinstance(fill, (tuple, list)):
            length = len(fill)
            num_channels = image.shape[-3]
            if length > 1 and length != num_channels:
                raise ValueError("The number of elements in 'fill' cannot broadcast to match the number of "
                                 f"channels of the image: {length} != {num_channels}")
        elif not isinstance(fill, (int, float)):
            raise ValueError("Argument fill should be either int, float, tuple or list")
    if interpolation not in supported_interpolation_modes:
        raise ValueError(f"Interpolation mode '{interpolation}' is unsupported with Tensor input")


def _affine_coeffs(matrix: List[float], w: int, h: int) -> List[float]:
    """The 8 kernel coefficients of `_affine_grid`: rescaled_theta = theta.transpose(1, 2).div_([0.5 * w, 0.5 * h]) in
    float32 with torch, column x then column y (the denominator's two are unused)."""
    theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
    rescaled = theta.transpose(1, 2).div_(torch.tensor([0.5 * w, 0.5 * h], dtype=torch.float32))
    return rescaled[0].t().reshape(6).tolist() + [0.0, 0.0]


def _perspective_grid_coeffs(coeffs: List[float], ow: int, oh: int) -> List[float]:
    """The 8 kernel coefficients of `_perspective_grid`: theta1 rescaled by (0.5 * ow, 0.5 * oh) in float32, then theta2's
    (coeffs[6], coeffs[7]) as float32."""
    theta1 = torch.tensor([[[coeffs[0], coeffs[1], coeffs[2]], [coeffs[3], coeffs[4], coeffs[5]]]], dtype=torch.float32)
    rescaled = theta1.transpose(1, 2).div_(torch.tensor([0.5 * ow, 0.5 * oh], dtype=torch.float32))
    theta2 = torch.tensor([coeffs[6], coeffs[7]], dtype=torch.float32)
    return rescaled[0].t().reshape(6).tolist() + theta2.tolist()


@functools.lru_cache(maxsize=None)
def _blocked_bmm_fuses() -> bool:
    """Whether this host's CPU bmm, past ATen's naive loop, rounds the grid as fma(y, b, x * a) + c (True) or as the plain
    sum (x * a + y * b) + c (False).  The BLAS kernel behind it differs between CPUs of one torch build (both forms have been
    seen on AVX-512 hosts), so the reference's rounding is probed once, on a 64 x 64 rotation grid."""
    n = 64
    matrix = _get_inverse_affine_matrix([0.0, 0.0], 30.0, [0.0, 0.0], 1.0, [0.0, 0.0])
    theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
    rt = theta.transpose(1, 2).div_(torch.tensor([0.5 * n, 0.5 * n], dtype=torch.float32))[0]
    v = torch.linspace((1.0 - n) * 0.5, (n - 1.0) * 0.5, steps=n)
    base = torch.stack([v.expand(n, n), v.unsqueeze(-1).expand(n, n), torch.ones(n, n)], -1).reshape(1, n * n, 3)
    got = base.bmm(rt.unsqueeze(0))[0]
    x, y = base[0, :, :1], base[0, :, 1:2]
    plain = (x * rt[0] + y * rt[1]) + rt[2]  # separate elementwise ops: each rounded once
    return not torch.equal(got, plain)


def _grid_order(oh: int, ow: int) -> int:
    """1: the grid carries the fma chain (this host's blocked CPU bmm fuses); 0: plain sums (ATen's naive small-bmm loop,
    or a blocked bmm that does not fuse)."""
    return 0 if oh * ow * 3 * 2 < _BMM_NAIVE_LIMIT or not _blocked_bmm_fuses() else 1


def _warp(image: torch.Tensor, oh: int, ow: int, coeffs: List[float], kind: str, mode: str, fill) -> torch.Tensor:
    """`_apply_grid_transform` of the (..., C, H, W) image at the k_warp grid given by the 8 float32 `coeffs`: ONE launch
    (mv_warp_*) over every plane.  The caller has run `_assert_grid_transform_inputs`."""
    _lib.require_f32_u8(image, kind, allow_bool=True)
    c, ih, iw = (int(s) for s in image.shape[-3:])
    out_shape = tuple(image.shape[:-2]) + (oh, ow)
    fill_arr, fill_channels = _elastic_fill(fill, c)
    if image.numel() == 0:
        return image.reshape(out_shape)
    planes = image.numel() // (ih * iw)
    args = (planes, fill_channels, ih, iw, oh, ow, _lib.taps(coeffs), _WARP_KINDS[kind], _grid_order(oh, ow),
            _ELASTIC_MODES[mode], fill_arr)
    return _lib.launch_image_op("warp", image, args, out_shape=out_shape, allow_bool=True, what=kind)


def affine(inpt: torch.Tensor, angle, translate, scale, shear, interpolation="nearest", fill=None,
           center: Optional[List[float]] = None) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py `affine`."""
    kernel = _get_kernel(affine, type(inpt))
    return kernel(inpt, angle=angle, translate=translate, scale=scale, shear=shear, interpolation=interpolation, fill=fill,
                  center=center)


@_register_image_and_video(affine)
def affine_image(image: torch.Tensor, angle, translate, scale, shear, interpolation="nearest", fill=None,
                 center: Optional[List[float]] = None) -> torch.Tensor:
    """affine_image (_geometry.py) on (..., C, H, W) float32 / uint8 / bool images: the inverse affine matrix about the image
    centre (or `center`), then grid_sample at its grid with the fill blend, in one mv_warp_* launch."""
    mode = _interpolation_name(interpolation)
    angle, translate, shear, center = _affine_parse_args(angle, translate, scale, shear, center)
    height, width = image.shape[-2:]
    center_f = [0.0, 0.0]
    if center is not None:  # pixel coordinates, shifted so that (0, 0) is the image centre
        center_f = [(c - s * 0.5) for c, s in zip(center, [width, height])]
    translate_f = [float(t) for t in translate]
    matrix = _get_inverse_affine_matrix(center_f, angle, translate_f, scale, shear)
    _assert_grid_transform_inputs(image, matrix, mode, fill, ["nearest", "bilinear"])
    return _warp(image, height, width, _affine_coeffs(matrix, width, height), "affine", mode, fill)


affine_video = affine_image


@_register_mask(affine)
def affine_mask(mask: torch.Tensor, angle, translate, scale, shear, fill=None,
                center: Optional[List[float]] = None) -> torch.Tensor:
    return _nearest_on_mask(affine_image, mask, angle, translate, scale, shear, fill=fill, center=center)


def rotate(inpt: torch.Tensor, angle: float, interpolation="nearest", expand: bool = False,
           center: Optional[List[float]] = None, fill=None) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py `rotate`."""
    kernel = _get_kernel(rotate, type(inpt))
    return kernel(inpt, angle=angle, interpolation=interpolation, expand=expand, fill=fill, center=center)


@_register_image_and_video(rotate)
def rotate_image(image: torch.Tensor, angle: float, interpolation="nearest", expand: bool = False,
                 center: Optional[List[float]] = None, fill=None) -> torch.Tensor:
    """rotate_image (_geometry.py): the inverse affine matrix of -angle about the centre; `expand` sizes the output to the
    rotated frame (_compute_affine_output_size), whose grid is still normalised by the input size."""
    mode = _interpolation_name(interpolation)
    shape = image.shape
    num_channels, height, width = shape[-3:]
    center_f = [0.0, 0.0]
    if center is not None:
        center_f = [(c - s * 0.5) for c, s in zip(center, [width, height])]
    # rotate and affine turn in opposite directions: -angle
    matrix = _get_inverse_affine_matrix(center_f, -angle, [0.0, 0.0], 1.0, [0.0, 0.0])
    if image.numel() > 0:
        image = image.reshape(-1, num_channels, height, width)
        _assert_grid_transform_inputs(image, matrix, mode, fill, ["nearest", "bilinear"])
        ow, oh = _compute_affine_output_size(matrix, width, height) if expand else (width, height)
        output = _warp(image, oh, ow, _affine_coeffs(matrix, width, height), "affine", mode, fill)
        new_height, new_width = output.shape[-2:]
    else:
        output = image
        new_width, new_height = _compute_affine_output_size(matrix, width, height) if expand else (width, height)
    return output.reshape(shape[:-3] + (num_channels, new_height, new_width))


rotate_video = rotate_image


@_register_mask(rotate)
def rotate_mask(mask: torch.Tensor, angle: float, expand: bool = False, center: Optional[List[float]] = None,
                fill=None) -> torch.Tensor:
    return _nearest_on_mask(rotate_image, mask, angle, expand=expand, fill=fill, center=center)


def perspective(inpt: torch.Tensor, startpoints: Optional[List[List[int]]], endpoints: Optional[List[List[int]]],
                interpolation="bilinear", fill=None, coefficients: Optional[List[float]] = None) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py `perspective`."""
    kernel = _get_kernel(perspective, type(inpt))
    return kernel(inpt, startpoints=startpoints, endpoints=endpoints, interpolation=interpolation, fill=fill,
                  coefficients=coefficients)


@_register_image_and_video(perspective)
def perspective_image(image: torch.Tensor, startpoints: Optional[List[List[int]]], endpoints: Optional[List[List[int]]],
                      interpolation="bilinear", fill=None, coefficients: Optional[List[float]] = None) -> torch.Tensor:
    """perspective_image (_geometry.py): the 8 perspective coefficients (given, or solved from the corners), then
    grid_sample at `_perspective_grid` with the fill blend, in one mv_warp_* launch."""
    perspective_coeffs = _perspective_coefficients(startpoints, endpoints, coefficients)
    mode = _interpolation_name(interpolation)
    if image.numel() == 0:
        return image
    _assert_grid_transform_inputs(image, matrix=None, interpolation=mode, fill=fill,
                                  supported_interpolation_modes=["nearest", "bilinear"], coeffs=perspective_coeffs)
    oh, ow = image.shape[-2:]
    return _warp(image, oh, ow, _perspective_grid_coeffs(perspective_coeffs, ow, oh), "perspective", mode, fill)


perspective_video = perspective_image


@_register_mask(perspective)
def perspective_mask(mask: torch.Tensor, startpoints: Optional[List[List[int]]], endpoints: Optional[List[List[int]]],
                     fill=None, coefficients: Optional[List[float]] = None) -> torch.Tensor:
    return _nearest_on_mask(perspective_image, mask, startpoints, endpoints, fill=fill, coefficients=coefficients)


for _f in (affine, rotate, perspective):
    _unsupported(_f, tv_tensors.BoundingBoxes, "BoundingBoxes are not transformed on the MI355X path (the local BoundingBoxes "
                                               "carries no format or canvas size)")
    if _pil.PIL is not None:
        _unsupported(_f, _pil.PIL.Image.Image, "PIL images are resampled by Pillow's own C code in the reference, not by "
                                               "grid_sample; convert with pil_to_tensor and move the tensor to the MI355X")
del _f
