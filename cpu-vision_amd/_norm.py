"""torch.nn.functional.group_norm (+ ReLU) over mv_group_norm_act_f32 (csrc/groupnorm.hip): the `GroupNorm -> ReLU` of the FCOS towers
and of the v2 detection heads; weight * torch.nn.functional.normalize over mv_l2_normalize_scale_f32 (csrc/l2norm.hip): SSD's
rescaling of conv4_3; LayerNorm over the channels of an NCHW map and its statistics over mv_layer_norm2d_f32 /
mv_layer_norm2d_stats_f32 (csrc/layernorm.hip): ConvNeXt's LayerNorm2d and the norm of its blocks.  float32, forward-only; the argument checks
fire before a device is needed.  Every name here is re-exported by `functional`.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _lib
from ._detection import _dense_images


def group_norm_chunk() -> int:
    """The elements of a group's slab one workgroup of group_norm_act sums (mv_group_norm_chunk)."""
    return int(_lib.load().mv_group_norm_chunk())


def group_norm_act(x: torch.Tensor, num_groups: int, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                   eps: float = 1e-5, relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.nn.functional.group_norm(x, num_groups, weight, bias, eps) and, with relu=True, the ReLU behind it, as TWO launches (the
    groups' float64 sums chunk by chunk, then the normalisation), whatever the batch and the size: x (N, C, H, W) float32 -> (N, C, H, W).
    A channel slice of a wider contiguous tensor is read as it is.  out: `x` itself for the in-place form (then x is dense NCHW).
    The arithmetic is stated in mi355vision.h (mv_group_norm_act_f32); a group's result depends on its own values only."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise RuntimeError("group_norm_act: x should be a 4-D tensor (N, C, H, W)")
    if x.dtype != torch.float32:
        raise TypeError(f"group_norm_act computes in float32. Got x {x.dtype}")
    n, c, h, w = (int(d) for d in x.shape)
    if not isinstance(num_groups, int) or isinstance(num_groups, bool) or num_groups < 1:
        raise ValueError(f"group_norm_act: num_groups must be a positive int, got {num_groups!r}")
    if c % num_groups:
        raise RuntimeError(f"Expected number of channels in input to be divisible by num_groups, but got input of shape {list(x.shape)} "
                           f"and num_groups={num_groups}")
    for name, p in (("weight", weight), ("bias", bias)):
        if p is not None and (not isinstance(p, torch.Tensor) or tuple(p.shape) != (c,)):
            raise RuntimeError(f"group_norm_act: {name} should have shape ({c},), got "
                               f"{tuple(p.shape) if isinstance(p, torch.Tensor) else type(p).__name__}")
        if p is not None and p.dtype != torch.float32:
            raise TypeError(f"group_norm_act computes in float32. Got {name} {p.dtype}")
    eps = float(eps)
    if not (eps > 0 and math.isfinite(eps)):
        raise ValueError(f"group_norm_act: eps must be positive and finite, got {eps!r}")
    if out is not None and out is not x:
        raise ValueError("group_norm_act: out is x itself (in place) or None")
    _lib.require_device(x, "x")
    lib = _lib.load()
    with _lib.on_device_of(x):
        xs = _dense_images(x)
        if out is not None:
            if xs.data_ptr() != x.data_ptr():  # _dense_images made a copy
                raise ValueError("group_norm_act: the in-place form needs dense images")
            y = xs
        else:
            y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        if n and c and h and w:
            gamma, beta = _lib.f32_on(weight, x.device), _lib.f32_on(bias, x.device)
            image = c * h * w
            nbytes = int(lib.mv_group_norm_workspace_bytes(n, c, h, w, num_groups))
            if not nbytes:
                raise _lib.Mi355VisionError(f"group_norm_act: {tuple(x.shape)} in {num_groups} groups is more than one call takes")
            buf, ws_ptr, nbytes = _lib.workspace(nbytes, x.device)
            x_stride = int(xs.stride(0)) if n > 1 else image
            _lib.launch(lib.mv_group_norm_act_f32, xs, xs.data_ptr(), y.data_ptr(), _lib.ptr(gamma), _lib.ptr(beta), n, c, h, w, num_groups,
                        x_stride, x_stride if out is not None else image, eps, int(bool(relu)), ws_ptr, nbytes)
    if out is not None:
        return x
    return _lib.forward_only(y, "group_norm_act", x, weight, bias)


def _check_layer_norm2d(name: str, x: torch.Tensor, weight, bias, eps) -> float:
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise RuntimeError(f"{name}: x should be a 4-D tensor (N, C, H, W)")
    if x.dtype != torch.float32:
        raise TypeError(f"{name} computes in float32. Got x {x.dtype}")
    c = int(x.shape[1])
    if c == 0:
        raise RuntimeError(f"{name}: no channels to normalise over in input of shape {list(x.shape)}")
    for what, p in (("weight", weight), ("bias", bias)):
        if p is not None and (not isinstance(p, torch.Tensor) or tuple(p.shape) != (c,)):
            raise RuntimeError(f"{name}: {what} should have shape ({c},), got "
                               f"{tuple(p.shape) if isinstance(p, torch.Tensor) else type(p).__name__}")
        if p is not None and p.dtype != torch.float32:
            raise TypeError(f"{name} computes in float32. Got {what} {p.dtype}")
    eps = float(eps)
    if not (eps >= 0 and math.isfinite(eps)):
        raise ValueError(f"{name}: eps must be non-negative and finite, got {eps!r}")
    return eps


def layer_norm2d_stats(x: torch.Tensor, eps: float = 1e-6) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, rstd), each (N, H, W) float32, of every pixel's C values of x (N, C, H, W): the statistics of layer_norm2d as ONE launch,
    for conv1x1_gelu(..., norm=(mean, rstd, weight, bias)), which normalises in its loads.  float64 sums in the order
    mv_layer_norm2d_stats_f32 states; a pixel's pair depends on its own C values, C and eps only."""
    eps = _check_layer_norm2d("layer_norm2d_stats", x, None, None, eps)
    n, c, h, w = (int(d) for d in x.shape)
    _lib.require_device(x, "x")
    lib = _lib.load()
    with _lib.on_device_of(x):
        xc = x.contiguous()
        mean = torch.empty((n, h, w), dtype=torch.float32, device=x.device)
        rstd = torch.empty((n, h, w), dtype=torch.float32, device=x.device)
        if n and h and w:
            _lib.launch(lib.mv_layer_norm2d_stats_f32, xc, xc.data_ptr(), mean.data_ptr(), rstd.data_ptr(), n, c, h, w, eps)
    return mean, rstd


def layer_norm2d(x: torch.Tensor, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                 eps: float = 1e-6) -> torch.Tensor:
    """models/convnext.py LayerNorm2d -- permute(0, 2, 3, 1), torch.nn.functional.layer_norm over C, permute back -- as ONE launch on
    x (N, C, H, W) float32, weight / bias (C,) or None.  The arithmetic is stated in mi355vision.h (mv_layer_norm2d_f32): float64
    statistics, four float32 roundings per element; a pixel's result depends on its own C values, C, the terms and eps only."""
    eps = _check_layer_norm2d("layer_norm2d", x, weight, bias, eps)
    n, c, h, w = (int(d) for d in x.shape)
    _lib.require_device(x, "x")
    lib = _lib.load()
    with _lib.on_device_of(x):
        xc = x.contiguous()
        y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        if n and h and w:
            gamma, beta = _lib.f32_on(weight, x.device), _lib.f32_on(bias, x.device)
            _lib.launch(lib.mv_layer_norm2d_f32, xc, xc.data_ptr(), _lib.ptr(gamma), _lib.ptr(beta), y.data_ptr(), n, c, h, w, eps)
    return _lib.forward_only(y, "layer_norm2d", x, weight, bias)


def l2_normalize_scale(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-12, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """weight.view(1, -1, 1, 1) * torch.nn.functional.normalize(x, p=2, dim=1, eps=eps) as ONE launch: x (N, C, H, W) float32 ->
    (N, C, H, W), weight (C,).  A channel slice of a wider contiguous tensor is read as it is.  out: `x` itself for the in-place form
    (then x is dense NCHW).  The arithmetic is stated in mi355vision.h (mv_l2_normalize_scale_f32): the squares are summed in float64,
    and a pixel's result depends on its own C values only."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise RuntimeError("l2_normalize_scale: x should be a 4-D tensor (N, C, H, W)")
    if x.dtype != torch.float32:
        raise TypeError(f"l2_normalize_scale computes in float32. Got x {x.dtype}")
    n, c, h, w = (int(d) for d in x.shape)
    if not isinstance(weight, torch.Tensor) or tuple(weight.shape) != (c,):
        raise RuntimeError(f"l2_normalize_scale: weight should have shape ({c},), got "
                           f"{tuple(weight.shape) if isinstance(weight, torch.Tensor) else type(weight).__name__}")
    if weight.dtype != torch.float32:
        raise TypeError(f"l2_normalize_scale computes in float32. Got weight {weight.dtype}")
    eps = float(eps)
    if not (eps > 0 and math.isfinite(eps)):
        raise ValueError(f"l2_normalize_scale: eps must be positive and finite, got {eps!r}")
    if out is not None and out is not x:
        raise ValueError("l2_normalize_scale: out is x itself (in place) or None")
    _lib.require_device(x, "x")
    lib = _lib.load()
    with _lib.on_device_of(x):
        xs = _dense_images(x)
        if out is not None:
            if xs.data_ptr() != x.data_ptr():  # _dense_images made a copy
                raise ValueError("l2_normalize_scale: the in-place form needs dense images")
            y = xs
        else:
            y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        if n and c and h and w:
            scale = _lib.f32_on(weight, x.device)
            image = c * h * w
            x_stride = int(xs.stride(0)) if n > 1 else image
            _lib.launch(lib.mv_l2_normalize_scale_f32, xs, xs.data_ptr(), y.data_ptr(), scale.data_ptr(), n, c, h, w, x_stride,
                        x_stride if out is not None else image, eps)
    if out is not None:
        return x
    return _lib.forward_only(y, "l2_normalize_scale", x, weight)
