"""The CNN layers behind nn.py, mobilenet.py and presets.py -- none of them a transforms.v2.functional function: conv2d_bias_relu
(models/vgg.py:81-85, ops/misc.py:97-119), max_pool2d*, conv2d_bias_act, conv2d_affine_act (models/resnet.py), adaptive_avg_pool2d,
linear_bias_relu, conv_norm_act / dwconv_pointwise / inverted_residual / fold_batchnorm (ops/misc.py:68-128, models/mobilenetv2.py:39-63), normalized_conv2d_bias_relu and the
*_k_slices queries.  All compute in float32 and are forward-only.  The pools launch through _lib.launch_xy; the layers with
several input tensors prepare them with _lib.f32_on / ptr / workspace and call _lib.launch.

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it; the
BATCH_INVARIANT_SUMMATION and CONV2D_* switches live there and are read through _lib.switch.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._filters import _planes
from ._misc import _mean_std


# --------------------------------------------------------------------------------------------- first CNN layer
def conv2d_bias_relu(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = True,
                     out: Optional[torch.Tensor] = None, sliced_k: Optional[bool] = None) -> torch.Tensor:
    """relu(conv2d(x, weight, bias, padding=1)) for 3x3 kernels -- nn.Conv2d(cin, cout, 3, padding=1) + nn.ReLU
    (models/vgg.py:81-85) on the fp32 MFMA.  x (N, Cin, H, W) fp32, weight (Cout, Cin, 3, 3).
    sliced_k: None = `not BATCH_INVARIANT_SUMMATION`; True lets small launches sum K in slices across workgroups (the order
    conv3x3_k_slices states: it depends on the batch size); False keeps one chain per output for every batch size."""
    if sliced_k is None:
        sliced_k = not _lib.switch("BATCH_INVARIANT_SUMMATION")
    if x.ndim != 4:
        raise ValueError(f"Expected 4D (N, C, H, W) input. Got {x.ndim}D")
    if weight.ndim != 4 or weight.shape[2:] != (3, 3):
        raise ValueError(f"weight should have shape (Cout, Cin, 3, 3). Got {tuple(weight.shape)}")
    n, cin, h, w = (int(d) for d in x.shape)
    cout = int(weight.shape[0])
    if int(weight.shape[1]) != cin:
        raise RuntimeError(f"Given groups=1, weight of size {list(weight.shape)}, expected input{list(x.shape)} "
                           f"to have {int(weight.shape[1])} channels, but got {cin} channels instead")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f"bias should have shape ({cout},). Got {tuple(bias.shape)}")
    _lib.require_device(x)
    _lib.require_device(weight, "weight")
    _lib.require_f32_layer("conv2d_bias_relu", x, weight)
    lib = _lib.load()
    xc, wc, bc = x.contiguous(), weight.detach().contiguous(), _lib.f32_on(bias, x.device)
    if out is None:
        out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, cout, h, w) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of shape (N, Cout, H, W)")
    args = (xc.data_ptr(), wc.data_ptr(), _lib.ptr(bc), out.data_ptr(), n, cin, h, w, cout, int(relu))
    # launches too small to fill the chip with one chain per output run K in slices across workgroups (conv3x3_k_slices
    # states the order); their raw sums pass through a workspace
    ws, ws_ptr, nbytes = _lib.workspace(int(lib.mv_conv3x3_workspace_bytes(n, cin, h, w, cout)) if sliced_k else 0, x.device)
    if nbytes:
        _lib.launch(lib.mv_conv3x3_bias_relu_ws_f32, xc, *args, ws_ptr, nbytes)
    else:
        _lib.launch(lib.mv_conv3x3_bias_relu_f32, xc, *args)
    return _lib.forward_only(out, "conv2d_bias_relu", x, weight, bias)


def conv3x3_k_slices(n: int, cin: int, h: int, w: int, cout: int) -> Tuple[int, int]:
    """(slices, slice_channels) of the summation order conv2d_bias_relu uses for a 3x3 conv of this shape
    (mv_conv3x3_k_slices): 1 slice = one ascending (channel, ky, kx) chain per output; more = chains over slices of
    slice_channels input channels, added in ascending order, then bias and ReLU (host logic, no GPU needed)."""
    sc = C.c_int(0)
    s = int(_lib.load().mv_conv3x3_k_slices(int(n), int(cin), int(h), int(w), int(cout), C.byref(sc)))
    return s, int(sc.value)


# --------------------------------------------------------------------------------------------- rest of the small CNN (8f.1)
def max_pool2d_2x2(x: torch.Tensor) -> torch.Tensor:
    """nn.MaxPool2d(kernel_size=2, stride=2) (models/vgg.py:78-79) on (..., H, W) fp32."""
    _lib.require_device(x)
    if x.dtype != torch.float32:
        raise TypeError(f"max_pool2d_2x2 computes in float32. Got {x.dtype}")
    planes, h, w = _planes(x)
    return _lib.launch_xy(_lib.load().mv_maxpool2x2_f32, x, (planes, h, w), out_shape=tuple(x.shape[:-2]) + (h // 2, w // 2),
                          out_dtype=torch.float32)


def max_pool2d(x: torch.Tensor, kernel_size: int, stride: Optional[int] = None, padding: int = 0, *, ceil_mode: bool = False) -> torch.Tensor:
    """nn.MaxPool2d(kernel_size, stride, padding), dilation 1 on (..., H, W): without padding AlexNet's 3, 2
    (models/alexnet.py:24); with padding (0 < padding <= kernel_size // 2: ResNet's stem, 3, 2, 1; models/resnet.py:201) the padded
    positions never win and NaN propagates as in torch's CPU kernel (mv_maxpool2d_pad_f32).  ceil_mode=True (SSD's third VGG pool,
    75 -> 38): the output side is ceil((in + 2 padding - kernel_size) / stride) + 1, less one when the last window would start in the
    right padding; windows are clipped to the input (mv_maxpool2d_ceil_f32)."""
    if ceil_mode:
        return _max_pool2d_ceil(x, int(kernel_size), int(kernel_size if stride is None else stride), int(padding))
    stride = kernel_size if stride is None else stride
    if padding != 0:
        return _max_pool2d_padded(x, int(kernel_size), int(stride), int(padding))
    if (kernel_size, stride) == (2, 2):
        return max_pool2d_2x2(x)
    _lib.require_device(x)
    if x.dtype != torch.float32:
        raise TypeError(f"max_pool2d computes in float32. Got {x.dtype}")
    planes, h, w = _planes(x)
    if kernel_size > h or kernel_size > w:
        raise RuntimeError(f"max_pool2d: kernel {kernel_size} exceeds the {h}x{w} input")
    out_shape = tuple(x.shape[:-2]) + ((h - kernel_size) // stride + 1, (w - kernel_size) // stride + 1)
    return _lib.launch_xy(_lib.load().mv_maxpool2d_f32, x, (planes, h, w, kernel_size, stride), out_shape=out_shape,
                          out_dtype=torch.float32)


def _max_pool2d_padded(x: torch.Tensor, kernel_size: int, stride: int, padding: int) -> torch.Tensor:
    _lib.require_device(x)
    if x.dtype != torch.float32:
        raise TypeError(f"max_pool2d computes in float32. Got {x.dtype}")
    if padding < 0 or padding > kernel_size // 2:
        raise RuntimeError(f"pad should be at most half of effective kernel size, but got pad={padding}, kernel_size={kernel_size}")
    planes, h, w = _planes(x)
    if h + 2 * padding < kernel_size or w + 2 * padding < kernel_size:
        raise RuntimeError(f"max_pool2d: kernel {kernel_size} exceeds the {h}x{w} input padded by {padding}")
    out_shape = tuple(x.shape[:-2]) + ((h + 2 * padding - kernel_size) // stride + 1, (w + 2 * padding - kernel_size) // stride + 1)
    return _lib.launch_xy(_lib.load().mv_maxpool2d_pad_f32, x, (planes, h, w, kernel_size, stride, padding), out_shape=out_shape,
                          out_dtype=torch.float32)


def _ceil_pool_out(size: int, kernel_size: int, stride: int, padding: int) -> int:
    """torch's pooling_output_shape with ceil_mode=True."""
    o = -((size + 2 * padding - kernel_size) // -stride) + 1
    return o - 1 if (o - 1) * stride >= size + padding else o


def _max_pool2d_ceil(x: torch.Tensor, kernel_size: int, stride: int, padding: int) -> torch.Tensor:
    if x.dtype != torch.float32:
        raise TypeError(f"max_pool2d computes in float32. Got {x.dtype}")
    if kernel_size <= 0 or stride <= 0:
        raise RuntimeError(f"max_pool2d: kernel_size and stride must be positive, got {kernel_size}, {stride}")
    if padding < 0 or padding > kernel_size // 2:
        raise RuntimeError(f"pad should be at most half of effective kernel size, but got pad={padding}, kernel_size={kernel_size}")
    planes, h, w = _planes(x)
    if h + 2 * padding < kernel_size or w + 2 * padding < kernel_size:
        raise RuntimeError(f"max_pool2d: kernel {kernel_size} exceeds the {h}x{w} input padded by {padding}")
    _lib.require_device(x)
    out_shape = tuple(x.shape[:-2]) + (_ceil_pool_out(h, kernel_size, stride, padding), _ceil_pool_out(w, kernel_size, stride, padding))
    return _lib.launch_xy(_lib.load().mv_maxpool2d_ceil_f32, x, (planes, h, w, kernel_size, stride, padding), out_shape=out_shape,
                          out_dtype=torch.float32)


_CONV_WORKSPACE_BYTES = 1 << 30


def conv2d_bias_act(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, stride=1, padding=0, dilation=1,
                    groups: int = 1, activation: Optional[str] = None) -> torch.Tensor:
    """Any nn.Conv2d [+ ReLU ...] of the small CNNs that the specialised kernels do not cover (AlexNet's 11x11 stride 4 and
    5x5: models/alexnet.py:22-33): implicit GEMM on the fp32 MFMA (mv_conv2d_bias_act_f32) -- the im2col columns are gathered
    from the input chunk by chunk into LDS and never reach HBM; no workspace unless mv_conv2d_needs_workspace() asks for one."""
    return _conv2d("conv2d_bias_act", x, weight, bias, None, None, None, stride, padding, dilation, groups, None, activation)


def adaptive_avg_pool2d(x: torch.Tensor, output_size: Sequence[int]) -> torch.Tensor:
    """nn.AdaptiveAvgPool2d(output_size) (models/vgg.py:41) on (..., H, W) fp32."""
    _lib.require_device(x)
    if x.dtype != torch.float32:
        raise TypeError(f"adaptive_avg_pool2d computes in float32. Got {x.dtype}")
    oh, ow = (int(output_size[0]), int(output_size[1]))
    planes, h, w = _planes(x)
    return _lib.launch_xy(_lib.load().mv_adaptive_avgpool_f32, x, (planes, h, w, oh, ow), out_shape=tuple(x.shape[:-2]) + (oh, ow),
                          out_dtype=torch.float32)


def linear_k_slices(n: int, k: int, m: int) -> Tuple[int, int]:
    """(slices, slice_len) of the K slicing linear_bias_relu uses for an (n, k) x (m, k) problem: 1 slice = the single
    ascending-k chain; more = partial chains over contiguous slices of slice_len, added in ascending order (host logic, no
    GPU needed)."""
    sl = C.c_int(0)
    s = int(_lib.load().mv_linear_k_slices(int(n), int(k), int(m), C.byref(sl)))
    return s, int(sl.value)


def conv1x1_k_slices(n: int, cin: int, h: int, w: int, cout: int) -> Tuple[int, int]:
    """(slices, slice_len) of the summation order conv_norm_act uses for a pointwise conv of this shape
    (mv_conv1x1_k_slices): 1 slice = one ascending-channel chain per output; more = chains over contiguous channel slices of
    slice_len, added in ascending order (host logic, no GPU needed)."""
    sl = C.c_int(0)
    s = int(_lib.load().mv_conv1x1_k_slices(int(n), int(cin), int(h), int(w), int(cout), C.byref(sl)))
    return s, int(sl.value)


def linear_bias_relu(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False,
                     sliced_k: Optional[bool] = None) -> torch.Tensor:
    """relu?(x @ weight.T + bias): nn.Linear [+ nn.ReLU] of the classifier (models/vgg.py:42-50); x (N, K) fp32,
    weight (M, K) as nn.Linear stores it.  Inference-size batches run K in slices over the whole chip (see
    linear_k_slices; the plan depends on the batch size); sliced_k=False forces the single ascending-k chain, None =
    `not BATCH_INVARIANT_SUMMATION`."""
    if sliced_k is None:
        sliced_k = not _lib.switch("BATCH_INVARIANT_SUMMATION")
    if x.ndim != 2 or weight.ndim != 2 or weight.shape[1] != x.shape[1]:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(x.shape)} and {tuple(weight.t().shape)})")
    _lib.require_device(x)
    _lib.require_device(weight, "weight")
    _lib.require_f32_layer("linear_bias_relu", x, weight)
    n, k = (int(d) for d in x.shape)
    m = int(weight.shape[0])
    lib = _lib.load()
    xc, wc, bc = x.contiguous(), weight.detach().contiguous(), _lib.f32_on(bias, x.device)
    y = torch.empty((n, m), dtype=torch.float32, device=x.device)
    args = (xc.data_ptr(), wc.data_ptr(), _lib.ptr(bc), y.data_ptr(), n, k, m, int(relu))
    ws, ws_ptr, nbytes = _lib.workspace(int(lib.mv_linear_workspace_bytes(n, k, m)) if sliced_k else 0, x.device)
    if nbytes:
        _lib.launch(lib.mv_linear_bias_relu_ws_f32, xc, *args, ws_ptr, nbytes)
    else:
        _lib.launch(lib.mv_linear_bias_relu_f32, xc, *args)
    return _lib.forward_only(y, "linear_bias_relu", x, weight, bias)


# --------------------------------------------------------------------------------------------- Conv2dNormActivation (8f.3)
_ACT_CODES = {None: 0, "none": 0, "relu": 1, "relu6": 2, "hardswish": 3, "silu": 4}
_AFFINE_CODES = {None: 0, "none": 0, "mul_add": 1, "fma": 2}


def fold_batchnorm(weight, bias, running_mean, running_var, eps: float = 1e-5):
    """nn.BatchNorm2d in eval mode as per-channel (alpha, beta) with y = fma(x, alpha, beta): ATen batch_norm_cpu's
    own steps (alpha = (1 / sqrt(var + eps)) * weight, beta = fma(-mean, alpha, bias)), evaluated on the host by
    mv_fold_batchnorm.  Returns CPU float32 tensors."""
    lib = _lib.load()
    mean = running_mean.detach().to("cpu", torch.float32).contiguous()
    var = running_var.detach().to("cpu", torch.float32).contiguous()
    c = mean.numel()
    w = None if weight is None else weight.detach().to("cpu", torch.float32).contiguous()
    b = None if bias is None else bias.detach().to("cpu", torch.float32).contiguous()
    alpha, beta = torch.empty(c, dtype=torch.float32), torch.empty(c, dtype=torch.float32)
    fp = C.POINTER(C.c_float)
    ptr = lambda t: None if t is None else C.cast(t.data_ptr(), fp)  # noqa: E731
    lib.mv_fold_batchnorm(ptr(w), ptr(b), ptr(mean), ptr(var), float(eps), c, ptr(alpha), ptr(beta))
    return alpha, beta


def _check_epilogue_terms(out_shape, bias, alpha, beta, residual) -> None:
    """conv_norm_act's and conv2d_affine_act's epilogue tensors: a residual shaped like the output, per-channel terms of cout
    elements."""
    if residual is not None and tuple(residual.shape) != out_shape:
        raise RuntimeError(f"residual of shape {tuple(residual.shape)} does not match the output {out_shape}")
    for t, name in ((bias, "bias"), (alpha, "alpha"), (beta, "beta")):
        if t is not None and t.numel() != out_shape[1]:
            raise RuntimeError(f"{name} has {t.numel()} elements for {out_shape[1]} output channels")


def conv_norm_act(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  alpha: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                  residual: Optional[torch.Tensor] = None, stride: int = 1, groups: int = 1, affine: Optional[str] = None,
                  activation: Optional[str] = None, *, input_scale: Optional[torch.Tensor] = None, dilation: int = 1) -> torch.Tensor:
    """One Conv2dNormActivation block (ops/misc.py:68-128) as one kernel: conv2d(padding=(k-1)//2) -> + bias ->
    folded norm (`affine`: "mul_add" = FrozenBatchNorm2d, "fma" = BatchNorm2d eval) -> + residual -> activation.
    Covers the MobileNet family's shapes: dense 3x3 with cin <= 4 (stem), depthwise 3x3 and 5x5 (groups = C),
    pointwise 1x1; stride 1 or 2.
    input_scale (pointwise only): a squeeze-excitation gate (N, Cin) or (N, Cin, 1, 1) multiplied into the conv's loads
    (mv_conv1x1_scaled_f32) -- the same bits as conv_norm_act(se_scale(x, input_scale), ...) without that tensor in memory.
    dilation (depthwise 5x5 at stride 1 only): 2 is the dilated block of MobileNetV3 as a segmentation backbone, padding 4
    (mv_dwconv_dilated_norm_act_f32); every other dilated geometry raises NotImplementedError."""
    if x.ndim != 4 or weight.ndim != 4:
        raise RuntimeError(f"Expected 4D input and weight. Got {tuple(x.shape)} and {tuple(weight.shape)}")
    if not isinstance(dilation, int) or isinstance(dilation, bool) or dilation < 1:
        raise ValueError(f"dilation should be a positive int, got {dilation!r}")
    if dilation != 1 and not (dilation == 2 and stride == 1 and tuple(weight.shape[1:]) == (1, 5, 5)
                              and groups == int(x.shape[1]) == int(weight.shape[0])):
        raise NotImplementedError(f"conv_norm_act: dilation {dilation} with weight {tuple(weight.shape)}, groups={groups}, stride={stride}; the "
                                  "one dilated geometry is depthwise 5x5 at dilation 2 and stride 1 (every other conv runs at dilation 1)")
    _lib.require_device(x)
    _lib.require_device(weight, "weight")
    _lib.require_f32_layer("conv_norm_act", x, weight)
    n, cin, h, w = (int(d) for d in x.shape)
    cout, cg, kh, kw = (int(d) for d in weight.shape)
    if groups == 1 and (kh, kw) == (3, 3) and cg == cin and cin <= 4:
        kind = 0
    elif groups == cin and cg == 1 and cout == cin and (kh, kw) == (3, 3):
        kind = 1
    elif groups == 1 and (kh, kw) == (1, 1) and cg == cin:
        kind = 2
    elif groups == cin and cg == 1 and cout == cin and (kh, kw) == (5, 5):
        kind = 3  # mv_dwconv_norm_act_f32
    else:
        raise NotImplementedError(
            f"conv_norm_act covers dense 3x3 with cin <= 4, depthwise 3x3 and 5x5 and pointwise 1x1; got weight {tuple(weight.shape)}, "
            f"groups={groups} on {cin} input channels")
    if input_scale is not None:
        if kind != 2:
            raise NotImplementedError("input_scale: pointwise (1x1) weights only")
        if not isinstance(input_scale, torch.Tensor) or tuple(input_scale.shape) not in ((n, cin), (n, cin, 1, 1)):
            raise RuntimeError(f"input_scale should have shape ({n}, {cin}) or ({n}, {cin}, 1, 1), got "
                               f"{tuple(input_scale.shape) if isinstance(input_scale, torch.Tensor) else type(input_scale).__name__}")
    if kind == 2 and stride != 1:
        raise NotImplementedError("pointwise convolution with stride != 1")
    if activation not in _ACT_CODES or affine not in _AFFINE_CODES:
        raise ValueError(f"unknown activation {activation!r} / affine {affine!r}")
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    lib = _lib.load()
    xc, wc = x.contiguous(), weight.detach().contiguous()
    bc, ac, btc, rc = (_lib.f32_on(t, x.device) for t in (bias, alpha, beta, residual))
    _check_epilogue_terms((n, cout, oh, ow), bc, ac, btc, rc)
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x.device)
    p = _lib.ptr
    if input_scale is not None:
        gc = _lib.f32_on(input_scale, x.device)
        _lib.launch(lib.mv_conv1x1_scaled_f32, xc, xc.data_ptr(), gc.data_ptr(), wc.data_ptr(), p(bc), p(ac), p(btc), p(rc), y.data_ptr(),
                    n, cin, h, w, cout, _AFFINE_CODES[affine], _ACT_CODES[activation])
    elif kind == 3:
        _lib.launch(lib.mv_dwconv_dilated_norm_act_f32, xc, xc.data_ptr(), wc.data_ptr(), p(bc), p(ac), p(btc), p(rc), y.data_ptr(),
                    n, cin, h, w, kh, stride, dilation, _AFFINE_CODES[affine], _ACT_CODES[activation])
    else:
        _lib.launch(lib.mv_conv_norm_act_f32, xc, kind, xc.data_ptr(), wc.data_ptr(), p(bc), p(ac), p(btc), p(rc), y.data_ptr(),
                    n, cin, h, w, cout, stride, _AFFINE_CODES[affine], _ACT_CODES[activation])
    return _lib.forward_only(y, "conv_norm_act", x, weight, bias, alpha, beta, residual, input_scale)


def dwconv7x7(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.Conv2d(C, C, 7, padding=3, groups=C) of a ConvNeXt block (models/convnext.py CNBlock.block[0]) as ONE launch
    (mv_dwconv7x7_bias_f32, k_dwpc7x7): x (N, C, H, W) float32, weight (C, 1, 7, 7), bias (C,) or None -> (N, C, H, W).  One fmaf
    chain per output in (ky, kx) order from +0, the padding taps through the chain as zeros, then `+ bias`: the oracle's bits."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or x.ndim != 4 or weight.ndim != 4:
        raise RuntimeError("dwconv7x7: expected a 4-D input (N, C, H, W) and a 4-D weight (C, 1, 7, 7)")
    n, c, h, w = (int(d) for d in x.shape)
    if tuple(weight.shape) != (c, 1, 7, 7):
        raise RuntimeError(f"dwconv7x7: weight should have shape ({c}, 1, 7, 7), got {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (c,):
        raise RuntimeError(f"dwconv7x7: bias should have shape ({c},), got {tuple(bias.shape)}")
    _lib.require_f32_layer("dwconv7x7", x, weight)
    _lib.require_device(x)
    _lib.require_device(weight, "weight")
    lib = _lib.load()
    xc, wc, bc = x.contiguous(), weight.detach().contiguous(), _lib.f32_on(bias, x.device)
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    if n and c and h and w:
        _lib.launch(lib.mv_dwconv7x7_bias_f32, xc, xc.data_ptr(), wc.data_ptr(), _lib.ptr(bc), y.data_ptr(), n, c, h, w)
    return _lib.forward_only(y, "dwconv7x7", x, weight, bias)


def conv1x1_gelu(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, norm=None, gelu: bool = True) -> torch.Tensor:
    """The per-pixel nn.Linear(Cin, Cout) [+ nn.GELU()] of a ConvNeXt block on the NCHW map, as the pointwise MFMA kernel
    (mv_conv1x1_ln_gelu_f32, k_conv1x1_ln): x (N, Cin, H, W) float32, weight (Cout, Cin) as nn.Linear stores it or (Cout, Cin, 1, 1),
    bias (Cout,) or None -> (N, Cout, H, W).  Summation order: conv1x1_k_slices; then `+ bias`; then the exact (erf) GELU stated in
    mi355vision.h, or nothing with gelu=False.
    norm: None, or (mean, rstd, ln_weight, ln_bias) -- layer_norm2d_stats(x, eps)'s pair (N, H, W) and the LayerNorm's terms (Cin,) or
    None: the LayerNorm over the channels is applied in the conv's loads, the same bits as conv1x1_gelu(layer_norm2d(x, ln_weight,
    ln_bias, eps), weight, bias) without that tensor in memory."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or x.ndim != 4:
        raise RuntimeError("conv1x1_gelu: expected a 4-D input (N, C, H, W)")
    if weight.ndim == 4 and tuple(weight.shape[2:]) == (1, 1):
        weight = weight.reshape(weight.shape[0], weight.shape[1])
    n, cin, h, w = (int(d) for d in x.shape)
    if weight.ndim != 2 or int(weight.shape[1]) != cin:
        raise RuntimeError(f"conv1x1_gelu: weight should have shape (Cout, {cin}) or (Cout, {cin}, 1, 1), got {tuple(weight.shape)}")
    cout = int(weight.shape[0])
    if cin == 0 or cout == 0:
        raise RuntimeError(f"conv1x1_gelu: no channels (weight {tuple(weight.shape)})")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise RuntimeError(f"conv1x1_gelu: bias should have shape ({cout},), got {tuple(bias.shape)}")
    mean = rstd = ln_w = ln_b = None
    if norm is not None:
        if not isinstance(norm, (tuple, list)) or len(norm) != 4:
            raise ValueError("conv1x1_gelu: norm is (mean, rstd, ln_weight, ln_bias) or None")
        mean, rstd, ln_w, ln_b = norm
        for what, t in (("mean", mean), ("rstd", rstd)):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (n, h, w):
                raise RuntimeError(f"conv1x1_gelu: norm's {what} should have shape ({n}, {h}, {w}), got "
                                   f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            if t.dtype != torch.float32:
                raise TypeError(f"conv1x1_gelu computes in float32. Got {what} {t.dtype}")
        for what, t in (("ln_weight", ln_w), ("ln_bias", ln_b)):
            if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (cin,)):
                raise RuntimeError(f"conv1x1_gelu: norm's {what} should have shape ({cin},), got "
                                   f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    _lib.require_f32_layer("conv1x1_gelu", x, weight)
    _lib.require_device(x)
    _lib.require_device(weight, "weight")
    lib = _lib.load()
    xc, wc, bc = x.contiguous(), weight.detach().contiguous(), _lib.f32_on(bias, x.device)
    mc, rc, lw, lb = (_lib.f32_on(t, x.device) for t in (mean, rstd, ln_w, ln_b))
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    p = _lib.ptr
    if n and h and w:
        _lib.launch(lib.mv_conv1x1_ln_gelu_f32, xc, xc.data_ptr(), p(mc), p(rc), p(lw), p(lb), wc.data_ptr(), p(bc), y.data_ptr(),
                    n, cin, h, w, cout, int(bool(gelu)))
    return _lib.forward_only(y, "conv1x1_gelu", x, weight, bias, ln_w, ln_b)


def conv1x1_upsample_add(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                         alpha: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                         top: Optional[torch.Tensor] = None, affine: Optional[str] = None,
                         activation: Optional[str] = None) -> torch.Tensor:
    """FeaturePyramidNetwork's top-down merge (ops/feature_pyramid_network.py:  inner_block(x) + F.interpolate(last_inner,
    size=feat_shape, mode="nearest")) as ONE launch (mv_conv1x1_upsample_add_f32): conv_norm_act's pointwise kernel, whose
    epilogue reads `top` (N, Cout, any H', W') at torch's nearest source index of each output pixel where conv_norm_act reads a
    residual -- no upsampled map and no separate sum in memory.  Same bits as conv_norm_act(..., residual=interpolate(top,
    size=x.shape[-2:], mode="nearest")); summation order: conv1x1_k_slices.  `top` is required (conv_norm_act is the call
    without one)."""
    if x.ndim != 4 or weight.ndim != 4:
        raise RuntimeError(f"Expected 4D input and weight. Got {tuple(x.shape)} and {tuple(weight.shape)}")
    if top is None:
        raise ValueError("conv1x1_upsample_add needs `top`; conv_norm_act is the pointwise conv without a top-down map")
    n, cin, h, w = (int(d) for d in x.shape)
    cout, cg, kh, kw = (int(d) for d in weight.shape)
    if (kh, kw) != (1, 1) or cg != cin:
        raise NotImplementedError(f"conv1x1_upsample_add covers pointwise 1x1 convs; got weight {tuple(weight.shape)} on {cin} input channels")
    if activation not in _ACT_CODES or affine not in _AFFINE_CODES:
        raise ValueError(f"unknown activation {activation!r} / affine {affine!r}")
    if _AFFINE_CODES[affine] != 0 and (alpha is None or beta is None):
        raise ValueError(f"affine={affine!r} needs alpha and beta")
    if top.ndim != 4 or int(top.shape[0]) != n or int(top.shape[1]) != cout or top.shape[2] < 1 or top.shape[3] < 1:
        raise RuntimeError(f"top of shape {tuple(top.shape)} does not match the output's batch and channels ({n}, {cout})")
    _check_epilogue_terms((n, cout, h, w), bias, alpha, beta, None)
    _lib.require_device(x)
    _lib.require_device(weight, "weight")
    _lib.require_device(top, "top")
    _lib.require_f32_layer("conv1x1_upsample_add", x, weight)
    lib = _lib.load()
    xc, wc = x.contiguous(), weight.detach().contiguous()
    bc, ac, btc, tc = (_lib.f32_on(t, x.device) for t in (bias, alpha, beta, top))
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    p = _lib.ptr
    _lib.launch(lib.mv_conv1x1_upsample_add_f32, xc, xc.data_ptr(), wc.data_ptr(), p(bc), p(ac), p(btc), tc.data_ptr(), y.data_ptr(),
                n, cin, h, w, cout, int(tc.shape[2]), int(tc.shape[3]), _AFFINE_CODES[affine], _ACT_CODES[activation])
    return _lib.forward_only(y, "conv1x1_upsample_add", x, weight, bias, alpha, beta, top)


def conv1x1_gated_upsample(x: torch.Tensor, gate: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                           residual: Optional[torch.Tensor] = None, size=None) -> torch.Tensor:
    """LRASPPHead's tail (models/segmentation/lraspp.py: low_classifier(low) + high_classifier(interpolate(cbr(high) * scale(high),
    size=low.shape[-2:]))) as ONE launch (mv_conv1x1_gated_upsample_f32): the pointwise conv `weight` (Cout, Cin, 1, 1) + `bias` over
    the bilinear (align_corners=False) resize to `size` of x (N, Cin, h, w) scaled by gate (N, Cin) or (N, Cin, 1, 1), plus `residual`
    (N, Cout, *size).  The gate product and the four-tap blend happen in the kernel's loads: neither the gated nor the resized tensor
    reaches memory.  The same bits as conv_norm_act(interpolate(se_scale(x, gate), size=size), weight, bias, residual=residual);
    summation order: conv1x1_k_slices(N, Cin, *size, Cout)."""
    from ._interp import checked_interpolate_shape
    if x.ndim != 4 or weight.ndim != 4:
        raise RuntimeError(f"Expected 4D input and weight. Got {tuple(x.shape)} and {tuple(weight.shape)}")
    n, cin, h, w = (int(d) for d in x.shape)
    cout, cg, kh, kw = (int(d) for d in weight.shape)
    if (kh, kw) != (1, 1) or cg != cin:
        raise NotImplementedError(f"conv1x1_gated_upsample covers pointwise 1x1 convs; got weight {tuple(weight.shape)} on {cin} input channels")
    if not isinstance(gate, torch.Tensor) or tuple(gate.shape) not in ((n, cin), (n, cin, 1, 1)):
        raise RuntimeError(f"input_scale should have shape ({n}, {cin}) or ({n}, {cin}, 1, 1), got "
                           f"{tuple(gate.shape) if isinstance(gate, torch.Tensor) else type(gate).__name__}")
    oh, ow = checked_interpolate_shape("conv1x1_gated_upsample", x, size, None, "bilinear", False, None, False)[4:]
    _lib.require_device(x)
    _lib.require_device(weight, "weight")
    _lib.require_f32_layer("conv1x1_gated_upsample", x, weight)
    lib = _lib.load()
    xc, wc = x.contiguous(), weight.detach().contiguous()
    gc, bc, rc = (_lib.f32_on(t, x.device) for t in (gate, bias, residual))
    _check_epilogue_terms((n, cout, oh, ow), bc, None, None, rc)
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x.device)
    p = _lib.ptr
    _lib.launch(lib.mv_conv1x1_gated_upsample_f32, xc, xc.data_ptr(), gc.data_ptr(), wc.data_ptr(), p(bc), p(rc), y.data_ptr(),
                n, cin, h, w, oh, ow, cout)
    return _lib.forward_only(y, "conv1x1_gated_upsample", x, gate, weight, bias, residual)


def dwconv_pointwise(x: torch.Tensor, dw_weight: torch.Tensor, dw_bias: Optional[torch.Tensor] = None,
                     dw_alpha: Optional[torch.Tensor] = None, dw_beta: Optional[torch.Tensor] = None,
                     weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                     alpha: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                     residual: Optional[torch.Tensor] = None, *, stride: int = 1, dw_affine: Optional[str] = None,
                     dw_activation: Optional[str] = None, affine: Optional[str] = None, activation: Optional[str] = None) -> torch.Tensor:
    """A depthwise-separable block (models/detection/ssdlite.py _prediction_block, the back half of _extra_block) as ONE launch
    (mv_dwconv3x3_conv1x1_f32): depthwise 3x3 (padding 1, `stride` 1 or 2) `dw_weight` (C, 1, 3, 3) -> + dw_bias -> folded norm
    (`dw_affine`) -> `dw_activation`, then the pointwise conv `weight` (Cout, C, 1, 1) with conv_norm_act's whole epilogue (bias, alpha /
    beta under `affine`, residual (N, Cout, oh, ow), `activation`).  The depthwise stage is computed in the pointwise kernel's loads: the
    hidden tensor never reaches memory.  The same bits as
        conv_norm_act(conv_norm_act(x, dw_weight, dw_bias, dw_alpha, dw_beta, stride=stride, groups=C, affine=dw_affine,
                                    activation=dw_activation),
                      weight, bias, alpha, beta, residual, affine=affine, activation=activation);
    summation order of the pointwise stage: conv1x1_k_slices(N, C, oh, ow, Cout)."""
    if weight is None:
        raise ValueError("dwconv_pointwise needs the pointwise `weight`; conv_norm_act is the depthwise conv alone")
    if x.ndim != 4 or dw_weight.ndim != 4 or weight.ndim != 4:
        raise RuntimeError(f"Expected 4D input and weights. Got {tuple(x.shape)}, {tuple(dw_weight.shape)} and {tuple(weight.shape)}")
    n, cin, h, w = (int(d) for d in x.shape)
    if tuple(dw_weight.shape) != (cin, 1, 3, 3):
        raise NotImplementedError(f"dwconv_pointwise covers depthwise 3x3 convs: dw_weight should have shape ({cin}, 1, 3, 3), got "
                                  f"{tuple(dw_weight.shape)}")
    cout, cg, kh, kw = (int(d) for d in weight.shape)
    if (kh, kw) != (1, 1) or cg != cin:
        raise NotImplementedError(f"dwconv_pointwise covers pointwise 1x1 convs; got weight {tuple(weight.shape)} on {cin} input channels")
    if stride not in (1, 2):
        raise ValueError(f"stride should be 1 or 2, got {stride!r}")
    if activation not in _ACT_CODES or affine not in _AFFINE_CODES:
        raise ValueError(f"unknown activation {activation!r} / affine {affine!r}")
    if dw_activation not in _ACT_CODES or dw_affine not in _AFFINE_CODES:
        raise ValueError(f"unknown dw_activation {dw_activation!r} / dw_affine {dw_affine!r}")
    if _AFFINE_CODES[dw_affine] != 0 and (dw_alpha is None or dw_beta is None):
        raise ValueError(f"dw_affine={dw_affine!r} needs dw_alpha and dw_beta")
    if _AFFINE_CODES[affine] != 0 and (alpha is None or beta is None):
        raise ValueError(f"affine={affine!r} needs alpha and beta")
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    for t, name in ((dw_bias, "dw_bias"), (dw_alpha, "dw_alpha"), (dw_beta, "dw_beta")):
        if t is not None and t.numel() != cin:
            raise RuntimeError(f"{name} has {t.numel()} elements for {cin} depthwise channels")
    _check_epilogue_terms((n, cout, oh, ow), bias, alpha, beta, residual)
    _lib.require_device(x)
    _lib.require_device(dw_weight, "dw_weight")
    _lib.require_device(weight, "weight")
    _lib.require_f32_layer("dwconv_pointwise", x, dw_weight)
    _lib.require_f32_layer("dwconv_pointwise", x, weight)
    lib = _lib.load()
    xc, dwc, wc = x.contiguous(), dw_weight.detach().contiguous(), weight.detach().contiguous()
    dbc, dac, dbtc, bc, ac, btc, rc = (_lib.f32_on(t, x.device) for t in (dw_bias, dw_alpha, dw_beta, bias, alpha, beta, residual))
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x.device)
    p = _lib.ptr
    _lib.launch(lib.mv_dwconv3x3_conv1x1_f32, xc, xc.data_ptr(), dwc.data_ptr(), p(dbc), p(dac), p(dbtc), wc.data_ptr(), p(bc), p(ac), p(btc),
                p(rc), y.data_ptr(), n, cin, h, w, cout, int(stride), _AFFINE_CODES[dw_affine], _ACT_CODES[dw_activation],
                _AFFINE_CODES[affine], _ACT_CODES[activation])
    return _lib.forward_only(y, "dwconv_pointwise", x, dw_weight, dw_bias, dw_alpha, dw_beta, weight, bias, alpha, beta, residual)


def conv2d_affine_act(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                      alpha: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                      residual: Optional[torch.Tensor] = None, stride=1, padding=0, dilation=1, groups: int = 1,
                      affine: Optional[str] = None, activation: Optional[str] = None) -> torch.Tensor:
    """Any nn.Conv2d -> + bias -> folded norm (`affine`: "mul_add" = FrozenBatchNorm2d, "fma" = BatchNorm2d eval) -> + residual ->
    activation as ONE launch (mv_conv2d_affine_act_f32): conv2d_bias_act's implicit GEMM -- any kernel size, stride, padding,
    dilation, groups; one ascending (c, ky, kx) chain per output -- with conv_norm_act's epilogue.  ResNet's 7x7 stride-2 stem,
    its 3x3 convs and its 1x1 stride-2 downsample (models/resnet.py); 1x1 convs at stride 1 are conv_norm_act's."""
    return _conv2d("conv2d_affine_act", x, weight, bias, alpha, beta, residual, stride, padding, dilation, groups, affine, activation)


def _conv2d(name: str, x, weight, bias, alpha, beta, residual, stride, padding, dilation, groups, affine, activation) -> torch.Tensor:
    """The body of conv2d_bias_act and conv2d_affine_act (`name`): checks, the columns workspace when mv_conv2d_needs_workspace() or
    a switch asks for one, ONE launch of mv_<name>_f32.  mv_conv2d_bias_act_f32 takes no alpha, beta, residual or affine code:
    conv2d_bias_act passes None for them, and its bias's length is not checked (a known gap)."""
    full = name == "conv2d_affine_act"
    if x.ndim != 4 or weight.ndim != 4:
        raise RuntimeError(f"Expected 4D input and weight. Got {tuple(x.shape)} and {tuple(weight.shape)}")
    _lib.require_device(x)
    _lib.require_device(weight, "weight")
    _lib.require_f32_layer(name, x, weight)
    pair = lambda v: (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))  # noqa: E731
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(padding), pair(dilation)
    n, cin, h, w = (int(d) for d in x.shape)
    cout, cg, kh, kw = (int(d) for d in weight.shape)
    if groups <= 0 or cg * groups != cin or cout % groups:
        raise RuntimeError(f"weight {tuple(weight.shape)} does not fit {cin} input channels in {groups} groups")
    if activation not in _ACT_CODES or affine not in _AFFINE_CODES:
        raise ValueError(f"unknown activation {activation!r} / affine {affine!r}" if full else f"unknown activation {activation!r}")
    if _AFFINE_CODES[affine] != 0 and (alpha is None or beta is None):
        raise ValueError(f"affine={affine!r} needs alpha and beta")
    oh, ow = (h + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (w + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    if oh <= 0 or ow <= 0:
        raise RuntimeError(f"Calculated output size too small - out_h: {oh} out_w: {ow}")
    lib = _lib.load()
    xc, wc = x.contiguous(), weight.detach().contiguous()
    bc, ac, btc, rc = (_lib.f32_on(t, x.device) for t in (bias, alpha, beta, residual))
    if full:
        _check_epilogue_terms((n, cout, oh, ow), bc, ac, btc, rc)
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x.device)
    if n == 0:
        return y
    nbytes = 0
    need = int(lib.mv_conv2d_needs_workspace(n, cin, cout, h, w, kh, kw, sh, sw, ph, pw, dh, dw, groups))
    if need == 1 or (need == 2 and _lib.switch("CONV2D_SMALL_LAUNCH_WORKSPACE")) or _lib.switch("CONV2D_COLUMNS_WORKSPACE"):
        per_image = int(lib.mv_deform_conv2d_workspace_bytes(1, cin, h, w, kh, kw, sh, sw, ph, pw, dh, dw))
        nbytes = _lib.columns_workspace_bytes(n, per_image, _CONV_WORKSPACE_BYTES)
    ws, ws_ptr, nbytes = _lib.workspace(nbytes, x.device)
    p = _lib.ptr
    terms, codes = ((p(bc), p(ac), p(btc), p(rc)), (_AFFINE_CODES[affine], _ACT_CODES[activation])) if full else ((p(bc),), (_ACT_CODES[activation],))
    _lib.launch(getattr(lib, "mv_" + name + "_f32"), xc, xc.data_ptr(), wc.data_ptr(), *terms, y.data_ptr(), n, cin, h, w, cout, kh, kw,
                sh, sw, ph, pw, dh, dw, groups, *codes, ws_ptr, nbytes)
    return _lib.forward_only(y, name, x, weight, bias, alpha, beta, residual)


def inverted_residual_k_slices(n: int, cin: int, hidden: int, cout: int, h: int, w: int, stride: int) -> Tuple[int, int]:
    """(slices, slice_len) of the fused InvertedResidual kernel for this shape (mv_inverted_residual_k_slices; host logic, no GPU):
    slices == 0 -> no fused kernel (the block runs as three conv_norm_act launches); otherwise the projection sums `slices`
    chains over `slice_len` hidden channels each, ascending from +0, added in ascending order."""
    sl = C.c_int(0)
    s = int(_lib.load().mv_inverted_residual_k_slices(int(n), int(cin), int(hidden), int(cout), int(h), int(w), int(stride), C.byref(sl)))
    return s, int(sl.value)


@functools.lru_cache(maxsize=512)
def _inverted_residual_workspace_bytes(lib_id: int, n: int, cin: int, hidden: int, cout: int, h: int, w: int, stride: int) -> int:
    """mv_inverted_residual_workspace_bytes, remembered per shape and loaded library (a pure function of both)."""
    return int(_lib.load().mv_inverted_residual_workspace_bytes(n, cin, hidden, cout, h, w, stride))


def inverted_residual(x: torch.Tensor, w_expand: torch.Tensor, a1: torch.Tensor, b1: torch.Tensor, w_dw: torch.Tensor, a2: torch.Tensor,
                      b2: torch.Tensor, w_project: torch.Tensor, a3: torch.Tensor, b3: torch.Tensor, residual: bool, stride: int = 1,
                      affine: str = "fma") -> torch.Tensor:
    """A whole InvertedResidual block (models/mobilenetv2.py:39-63) as one kernel: [1x1 expand + norm + ReLU6 ->] 3x3 depthwise
    (stride) + norm + ReLU6 -> 1x1 project + norm [-> + x]; the hidden tensor stays on the CU (csrc/invres.hip).  Shapes
    without a fused kernel raise Mi355VisionError (ask inverted_residual_k_slices first).  All tensors fp32 on the device;
    a*, b*: the folded norms of the three convolutions (`affine`: "fma" = BatchNorm2d eval, "mul_add" = FrozenBatchNorm2d)."""
    _lib.require_device(x)
    if x.ndim != 4 or x.dtype != torch.float32:
        raise TypeError(f"inverted_residual expects a float32 (N, C, H, W) tensor. Got {x.dtype} {tuple(x.shape)}")
    n, cin, h, w = (int(d) for d in x.shape)
    hidden, cout = int(w_dw.shape[0]), int(w_project.shape[0])
    if w_expand is None:  # a block without expansion (expand_ratio 1): the depthwise conv runs on x itself
        if hidden != cin or a1 is not None or b1 is not None:
            raise RuntimeError(f"a block without expansion has hidden == cin and no a1 / b1 (hidden {hidden}, cin {cin})")
    elif tuple(w_expand.shape[:2]) != (hidden, cin):
        raise RuntimeError(f"weights {tuple(w_expand.shape)}, {tuple(w_dw.shape)}, {tuple(w_project.shape)} do not form a block on {cin} channels")
    if tuple(w_dw.shape) != (hidden, 1, 3, 3) or tuple(w_project.shape[:2]) != (cout, hidden):
        raise RuntimeError(f"weights {tuple(w_dw.shape)}, {tuple(w_project.shape)} do not form a block on {cin} channels")
    if affine not in ("fma", "mul_add"):
        raise ValueError(f"affine should be 'fma' or 'mul_add'. Got {affine!r}")
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    lib = _lib.load()
    xc = x.contiguous()
    ts = [_lib.f32_on(t, x.device) for t in (w_expand, a1, b1, w_dw, a2, b2, w_project, a3, b3)]
    for t, c, name in ((ts[1], hidden, "a1"), (ts[2], hidden, "b1"), (ts[4], hidden, "a2"), (ts[5], hidden, "b2"), (ts[7], cout, "a3"), (ts[8], cout, "b3")):
        if t is not None and t.numel() != c:
            raise RuntimeError(f"{name} has {t.numel()} elements for {c} channels")
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x.device)
    ws, ws_ptr, nbytes = _lib.workspace(_inverted_residual_workspace_bytes(id(lib), n, cin, hidden, cout, h, w, stride), x.device)
    _lib.launch(lib.mv_inverted_residual_f32, xc, xc.data_ptr(), *[_lib.ptr(t) for t in ts], int(bool(residual)), y.data_ptr(), n, cin,
                hidden, cout, h, w, stride, _AFFINE_CODES[affine], ws_ptr, nbytes)
    return _lib.forward_only(y, "inverted_residual", x, *([] if w_expand is None else [w_expand]), w_dw, w_project)

def normalized_conv2d_bias_relu(image_u8: torch.Tensor, mean: List[float], std: List[float], weight: torch.Tensor,
                                bias: Optional[torch.Tensor] = None, relu: bool = True) -> torch.Tensor:
    """relu(conv2d(normalize(to_dtype(image_u8, float32, scale=True), mean, std), weight, bias, padding=1)) with the
    conversion and normalisation fused into the conv's load: the uint8 (N, 3, H, W) batch is read once (1 B/element)
    and no fp32 copy of it is ever written."""
    if image_u8.dtype != torch.uint8 or image_u8.ndim != 4 or image_u8.shape[1] != 3:
        raise TypeError(f"expected a uint8 (N, 3, H, W) batch. Got {image_u8.dtype} {tuple(image_u8.shape)}")
    if weight.ndim != 4 or tuple(weight.shape[1:]) != (3, 3, 3):
        raise ValueError(f"weight should have shape (Cout, 3, 3, 3). Got {tuple(weight.shape)}")
    _lib.require_device(image_u8)
    _lib.require_device(weight, "weight")
    n, _, h, w = (int(d) for d in image_u8.shape)
    cout = int(weight.shape[0])
    m, s = _mean_std(mean, std, 3)
    lib = _lib.load()
    xc, wc, bc = image_u8.contiguous(), weight.detach().to(torch.float32).contiguous(), _lib.f32_on(bias, image_u8.device)
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=image_u8.device)
    _lib.launch(lib.mv_conv3x3_bias_relu_u8norm_f32, xc, xc.data_ptr(), m, s, wc.data_ptr(), _lib.ptr(bc), y.data_ptr(), n, h, w,
                cout, int(relu))
    return _lib.forward_only(y, "normalized_conv2d_bias_relu", weight, bias)
