"""Squeeze-excitation (ops/misc.py SqueezeExcitation) and the dense layer with an activation over csrc/se.hip: global_avg_pool
(mv_global_avgpool_f64sum_f32), linear_act (mv_linear_act_f32), se_scale (mv_se_scale_f32) and the two compositions
squeeze_excitation_gate / squeeze_excitation.  float32, forward-only; the argument checks fire before a device is needed.  The
summation orders are stated in mi355vision.h.  Every name here is re-exported by `functional`; the gate folded into the projection
conv is conv_norm_act(..., input_scale=gate) of _layers.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._detection import _dense_images

_LINEAR_ACT_CODES = {None: 0, "none": 0, "relu": 1, "hardswish": 3, "hardsigmoid": 5, "sigmoid": 6}


def global_avg_pool(x: torch.Tensor) -> torch.Tensor:
    """The mean of every (image, channel) plane: x (N, C, H, W) float32 -> (N, C), one wave per plane, summed in float64 in the
    order mv_global_avgpool_f64sum_f32 states.  A channel slice of a wider contiguous tensor is read as it is.  (adaptive_avg_pool2d
    keeps its float32 chain.)"""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise RuntimeError("global_avg_pool: x should be a 4-D tensor (N, C, H, W)")
    if x.dtype != torch.float32:
        raise TypeError(f"global_avg_pool computes in float32. Got x {x.dtype}")
    n, c, h, w = (int(d) for d in x.shape)
    if c == 0 or h == 0 or w == 0:
        raise RuntimeError(f"global_avg_pool: empty planes in input of shape {list(x.shape)}")
    _lib.require_device(x, "x")
    lib = _lib.load()
    with _lib.on_device_of(x):
        xs = _dense_images(x)
        y = torch.empty((n, c), dtype=torch.float32, device=x.device)
        if n:
            _lib.launch(lib.mv_global_avgpool_f64sum_f32, xs, xs.data_ptr(), y.data_ptr(), n, c, h, w,
                        int(xs.stride(0)) if n > 1 else c * h * w)
    return _lib.forward_only(y, "global_avg_pool", x)


def linear_act(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, activation: Optional[str] = None) -> torch.Tensor:
    """activation(x @ weight.T + bias): x (N, K), weight (M, K) as nn.Linear stores it or (M, K, 1, 1) as the 1x1 nn.Conv2d of a
    SqueezeExcitation does; activation None | "relu" | "hardswish" | "hardsigmoid" | "sigmoid".  One wave per output, float64 sums in
    the order mv_linear_act_f32 states: a row's result does not depend on N.  The squeeze layers and MobileNetV3's
    Linear -> Hardswish."""
    if activation not in _LINEAR_ACT_CODES:
        raise ValueError(f"unknown activation {activation!r}")
    if weight.ndim == 4 and tuple(weight.shape[2:]) == (1, 1):
        weight = weight.reshape(weight.shape[0], weight.shape[1])
    if x.ndim != 2 or weight.ndim != 2 or weight.shape[1] != x.shape[1]:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(x.shape)} and {tuple(weight.t().shape)})")
    n, k = (int(d) for d in x.shape)
    m = int(weight.shape[0])
    if bias is not None and tuple(bias.shape) != (m,):
        raise RuntimeError(f"bias should have shape ({m},). Got {tuple(bias.shape)}")
    _lib.require_device(x)
    _lib.require_device(weight, "weight")
    _lib.require_f32_layer("linear_act", x, weight)
    lib = _lib.load()
    xc, wc, bc = x.contiguous(), weight.detach().contiguous(), _lib.f32_on(bias, x.device)
    y = torch.empty((n, m), dtype=torch.float32, device=x.device)
    _lib.launch(lib.mv_linear_act_f32, xc, xc.data_ptr(), wc.data_ptr(), _lib.ptr(bc), y.data_ptr(), n, k, m, _LINEAR_ACT_CODES[activation])
    return _lib.forward_only(y, "linear_act", x, weight, bias)


def _check_gate(x: torch.Tensor, gate: torch.Tensor, name: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise RuntimeError(f"{name}: x should be a 4-D tensor (N, C, H, W)")
    shape = tuple(int(d) for d in x.shape[:2])
    if not isinstance(gate, torch.Tensor) or tuple(gate.shape) not in (shape, shape + (1, 1)):
        raise RuntimeError(f"{name}: the gate should have shape {shape} or {shape + (1, 1)}, got "
                           f"{tuple(gate.shape) if isinstance(gate, torch.Tensor) else type(gate).__name__}")
    if x.dtype != torch.float32 or gate.dtype != torch.float32:
        raise TypeError(f"{name} computes in float32. Got x {x.dtype}, gate {gate.dtype}")


def se_scale(x: torch.Tensor, gate: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gate[:, :, None, None] * x as one launch: x (N, C, H, W) float32, gate (N, C) or (N, C, 1, 1).  out: `x` itself for the
    in-place form (then x is contiguous)."""
    _check_gate(x, gate, "se_scale")
    if out is not None and out is not x:
        raise ValueError("se_scale: out is x itself (in place) or None")
    if out is not None and not x.is_contiguous():
        raise ValueError("se_scale: the in-place form needs a contiguous x")
    _lib.require_device(x, "x")
    _lib.require_device(gate, "gate")
    n, c, h, w = (int(d) for d in x.shape)
    lib = _lib.load()
    xc, gc = x.contiguous(), gate.detach().contiguous()
    y = xc if out is not None else torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    if n and c and h and w:
        _lib.launch(lib.mv_se_scale_f32, xc, xc.data_ptr(), gc.data_ptr(), y.data_ptr(), n, c, h, w)
    if out is not None:
        return x
    return _lib.forward_only(y, "se_scale", x, gate)


def squeeze_excitation_gate(x: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor],
                            activation: str = "relu", scale_activation: str = "sigmoid") -> torch.Tensor:
    """SqueezeExcitation._scale as three launches: scale_activation(fc2(activation(fc1(avgpool(x))))) -> (N, C)."""
    return linear_act(linear_act(global_avg_pool(x), w1, b1, activation), w2, b2, scale_activation)


def squeeze_excitation(x: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor],
                       activation: str = "relu", scale_activation: str = "sigmoid") -> torch.Tensor:
    """SqueezeExcitation.forward: squeeze_excitation_gate(x, ...) * x, four launches."""
    return se_scale(x, squeeze_excitation_gate(x, w1, b1, w2, b2, activation, scale_activation))
