"""ConvNeXt (tiny, small, base, large) on the MI355X kernels.

Mirrors models/convnext.py of the reference: LayerNorm2d, CNBlock, CNBlockConfig, ConvNeXt and the four builders, with the reference's
constructor arguments, argument errors and module tree (torch's own nn.Conv2d / nn.LayerNorm / nn.Linear / nn.GELU serve as PARAMETER
CONTAINERS, built in the reference's order, so its state dicts load as they are and a seeded construction consumes torch's RNG like
the reference's).  StochasticDepth and Permute (ops/stochastic_depth.py, ops/misc.py) live here and are re-exported by `ops`.  Only
`forward` differs:

  * a CNBlock is FOUR launches, or five: F.dwconv7x7 (depthwise 7x7 + bias), F.layer_norm2d_stats (a pixel's mean and rstd over the
    channels), F.conv1x1_gelu(..., norm=...) (Linear(C, 4C) as the pointwise MFMA kernel with the LayerNorm in its loads and GELU in its
    epilogue: neither the permuted nor the normalised tensor reaches memory) and F.conv_norm_act(..., alpha=layer_scale,
    residual=input) (Linear(4C, C), `layer_scale *` and `+= input` in the epilogue).  `_use_fused(dim, pixels)` says per launch whether
    the norm runs in the loads or as its own launch (F.layer_norm2d, then F.conv1x1_gelu without `norm`: five launches, the same bits);
  * the stem and the downsample layers are F.conv2d_affine_act with bias (4x4 stride 4, 2x2 stride 2) and F.layer_norm2d;
  * the head is F.global_avg_pool, F.layer_norm2d on the (N, C, 1, 1) map and F.linear_bias_relu(relu=False).

Inference only: the device forward raises in training mode (StochasticDepth is then the identity it is in eval mode), and -- the
project's convention, not the reference's -- `ConvNeXt.__init__` ends in `self.eval()`.  No weight files, as for the other builders.
"""
from __future__ import annotations

from functools import partial
from typing import Any, Callable, List, Optional, Sequence

import torch
from torch import nn

from . import functional as F
from ._lib import forward_only

__all__ = ["LayerNorm2d", "CNBlock", "CNBlockConfig", "ConvNeXt", "StochasticDepth", "Permute", "stochastic_depth", "convnext_tiny",
           "convnext_small", "convnext_base", "convnext_large"]


def stochastic_depth(input: torch.Tensor, p: float, mode: str, training: bool = True) -> torch.Tensor:
    """ops/stochastic_depth.py stochastic_depth: the reference's torch composition (a training-time op; the identity otherwise)."""
    if p < 0.0 or p > 1.0:
        raise ValueError(f"drop probability has to be between 0 and 1, but got {p}")
    if mode not in ["batch", "row"]:
        raise ValueError(f"mode has to be either 'batch' or 'row', but got {mode}")
    if not training or p == 0.0:
        return input
    survival_rate = 1.0 - p
    if mode == "row":
        size = [input.shape[0]] + [1] * (input.ndim - 1)
    else:
        size = [1] * input.ndim
    noise = torch.empty(size, dtype=input.dtype, device=input.device)
    noise = noise.bernoulli_(survival_rate)
    if survival_rate > 0.0:
        noise.div_(survival_rate)
    return input * noise


class StochasticDepth(nn.Module):
    """ops/stochastic_depth.py StochasticDepth: the identity in eval mode."""

    def __init__(self, p: float, mode: str) -> None:
        super().__init__()
        self.p = p
        self.mode = mode

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return stochastic_depth(input, self.p, self.mode, self.training)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(p={self.p}, mode={self.mode})"


class Permute(nn.Module):
    """ops/misc.py Permute: torch.permute(x, dims) (a view)."""

    def __init__(self, dims: List[int]):
        super().__init__()
        self.dims = dims

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.permute(x, self.dims)


class LayerNorm2d(nn.LayerNorm):
    """models/convnext.py LayerNorm2d: LayerNorm over the channels of an NCHW map, ONE launch (F.layer_norm2d)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if len(self.normalized_shape) != 1:
            raise NotImplementedError("LayerNorm2d normalises over the channel dimension alone")
        return F.layer_norm2d(x, self.weight, self.bias, self.eps)


def _use_fused(dim: int, pixels: int) -> bool:
    """Whether a block of width `dim` on `pixels` = N H W pixels normalises in the loads of its first pointwise conv (four launches) or
    in a launch of its own (five).  The same bits either way; decided by measurement (profiles/perf_convnext.log): the
    four-launch form won on the small launches of the two deep stages (384 x 14 x 14 and 768 x 7 x 7 at batch 1: 0.086 against 0.092 ms
    and 0.147 against 0.158 ms per block) and lost everywhere else (96 and 192 channels at batch 1, every stage at batch 64), where the
    pointwise kernel is bound by its loads' arithmetic and not by launches."""
    return dim >= 384 and pixels <= 1024


_ZEROS: dict = {}


def _zeros(dim: int, device: torch.device) -> torch.Tensor:
    """The `+ 0` of the "mul_add" epilogue of a block's projection: one tensor per (width, device), made on first use -- the module
    keeps the reference's parameters and buffers and nothing else."""
    key = (dim, device)
    if key not in _ZEROS:
        _ZEROS[key] = torch.zeros(dim, dtype=torch.float32, device=device)
    return _ZEROS[key]


class CNBlock(nn.Module):
    """models/convnext.py CNBlock: depthwise 7x7 -> LayerNorm -> Linear(C, 4C) -> GELU -> Linear(4C, C), `layer_scale *`, `+ input`."""

    def __init__(self, dim, layer_scale: float, stochastic_depth_prob: float, norm_layer: Optional[Callable[..., nn.Module]] = None) -> None:
        super().__init__()
        if norm_layer is None:
            norm_layer = partial(nn.LayerNorm, eps=1e-6)
        self.block = nn.Sequential(
            nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True),
            Permute([0, 2, 3, 1]),
            norm_layer(dim),
            nn.Linear(in_features=dim, out_features=4 * dim, bias=True),
            nn.GELU(),
            nn.Linear(in_features=4 * dim, out_features=dim, bias=True),
            Permute([0, 3, 1, 2]),
        )
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)
        self.stochastic_depth = StochasticDepth(stochastic_depth_prob, "row")

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise RuntimeError("the MI355X CNBlock is inference only: call .eval()")
        conv, norm, fc1, fc2 = self.block[0], self.block[2], self.block[3], self.block[5]
        if not isinstance(norm, nn.LayerNorm) or len(norm.normalized_shape) != 1:
            raise NotImplementedError("CNBlock runs nn.LayerNorm over the channels; got " + type(norm).__name__)
        dim = conv.out_channels
        with torch.no_grad():
            h = F.dwconv7x7(input, conv.weight, conv.bias)
            if _use_fused(dim, int(input.shape[0]) * int(input.shape[2]) * int(input.shape[3])):
                mean, rstd = F.layer_norm2d_stats(h, norm.eps)
                h = F.conv1x1_gelu(h, fc1.weight, fc1.bias, norm=(mean, rstd, norm.weight, norm.bias))
            else:
                h = F.conv1x1_gelu(F.layer_norm2d(h, norm.weight, norm.bias, norm.eps), fc1.weight, fc1.bias)
            # input + fl(fl(acc + b2) * layer_scale): the reference's `layer_scale * block(x)`, then `+= input`
            out = F.conv_norm_act(h, fc2.weight.view(dim, 4 * dim, 1, 1), fc2.bias, alpha=self.layer_scale.reshape(dim),
                                  beta=_zeros(dim, input.device), residual=input, affine="mul_add")
        return forward_only(out, "CNBlock.forward", input, conv.weight, fc1.weight, fc2.weight, self.layer_scale)


class CNBlockConfig:
    """models/convnext.py CNBlockConfig: one stage -- its width, the next stage's width (None: the last), its number of blocks."""

    def __init__(self, input_channels: int, out_channels: Optional[int], num_layers: int) -> None:
        self.input_channels = input_channels
        self.out_channels = out_channels
        self.num_layers = num_layers

    def __repr__(self) -> str:
        s = self.__class__.__name__ + "("
        s += "input_channels={input_channels}"
        s += ", out_channels={out_channels}"
        s += ", num_layers={num_layers}"
        s += ")"
        return s.format(**self.__dict__)


class _Stem(nn.Sequential):
    """Conv2dNormActivation(3, c0, kernel_size=4, stride=4, padding=0, norm_layer, activation_layer=None, bias=True): children "0" (the
    conv) and "1" (the norm), the conv with its bias as one launch and the norm as another."""

    def __init__(self, in_channels: int, out_channels: int, norm_layer: Callable[..., nn.Module]) -> None:
        super().__init__(nn.Conv2d(in_channels, out_channels, kernel_size=4, stride=4, padding=0, bias=True), norm_layer(out_channels))
        self.out_channels = out_channels

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self[1](_conv_bias(self[0], x))


class _Downsample(nn.Sequential):
    """Sequential(norm_layer(cin), Conv2d(cin, cout, kernel_size=2, stride=2)): two launches."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _conv_bias(self[1], self[0](x))


def _conv_bias(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    return F.conv2d_affine_act(x, conv.weight, conv.bias, stride=conv.stride, padding=conv.padding)


class ConvNeXt(nn.Module):
    """models/convnext.py ConvNeXt."""

    def __init__(self, block_setting: List[CNBlockConfig], stochastic_depth_prob: float = 0.0, layer_scale: float = 1e-6,
                 num_classes: int = 1000, block: Optional[Callable[..., nn.Module]] = None,
                 norm_layer: Optional[Callable[..., nn.Module]] = None, **kwargs: Any) -> None:
        super().__init__()
        if not block_setting:
            raise ValueError("The block_setting should not be empty")
        elif not (isinstance(block_setting, Sequence) and all([isinstance(s, CNBlockConfig) for s in block_setting])):
            raise TypeError("The block_setting should be List[CNBlockConfig]")
        if block is None:
            block = CNBlock
        if norm_layer is None:
            norm_layer = partial(LayerNorm2d, eps=1e-6)
        layers: List[nn.Module] = []
        firstconv_output_channels = block_setting[0].input_channels
        layers.append(_Stem(3, firstconv_output_channels, norm_layer))
        total_stage_blocks = sum(cnf.num_layers for cnf in block_setting)
        stage_block_id = 0
        for cnf in block_setting:
            stage: List[nn.Module] = []
            for _ in range(cnf.num_layers):
                sd_prob = stochastic_depth_prob * stage_block_id / (total_stage_blocks - 1.0)
                stage.append(block(cnf.input_channels, layer_scale, sd_prob))
                stage_block_id += 1
            layers.append(nn.Sequential(*stage))
            if cnf.out_channels is not None:
                layers.append(_Downsample(norm_layer(cnf.input_channels),
                                          nn.Conv2d(cnf.input_channels, cnf.out_channels, kernel_size=2, stride=2)))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        lastblock = block_setting[-1]
        lastconv_output_channels = lastblock.out_channels if lastblock.out_channels is not None else lastblock.input_channels
        self.classifier = nn.Sequential(norm_layer(lastconv_output_channels), nn.Flatten(1), nn.Linear(lastconv_output_channels, num_classes))
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        self.eval()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise RuntimeError("the MI355X ConvNeXt is inference only: call .eval()")
        inp = x
        norm, fc = self.classifier[0], self.classifier[2]
        with torch.no_grad():  # no autograd bookkeeping per layer; the result is marked once (its backward raises)
            x = self.features(x)
            n, c = int(x.shape[0]), int(x.shape[1])
            x = F.global_avg_pool(x).view(n, c, 1, 1)  # avgpool
            x = norm(x).view(n, c)                     # LayerNorm2d on the (N, C, 1, 1) map, Flatten(1)
            x = F.linear_bias_relu(x, fc.weight, fc.bias, relu=False)
        return forward_only(x, "ConvNeXt.forward", inp, fc.weight)


def _convnext(block_setting: List[CNBlockConfig], stochastic_depth_prob: float, **kwargs: Any) -> ConvNeXt:
    return ConvNeXt(block_setting, stochastic_depth_prob=stochastic_depth_prob, **kwargs)


def convnext_tiny(**kwargs: Any) -> ConvNeXt:
    block_setting = [CNBlockConfig(96, 192, 3), CNBlockConfig(192, 384, 3), CNBlockConfig(384, 768, 9), CNBlockConfig(768, None, 3)]
    return _convnext(block_setting, kwargs.pop("stochastic_depth_prob", 0.1), **kwargs)


def convnext_small(**kwargs: Any) -> ConvNeXt:
    block_setting = [CNBlockConfig(96, 192, 3), CNBlockConfig(192, 384, 3), CNBlockConfig(384, 768, 27), CNBlockConfig(768, None, 3)]
    return _convnext(block_setting, kwargs.pop("stochastic_depth_prob", 0.4), **kwargs)


def convnext_base(**kwargs: Any) -> ConvNeXt:
    block_setting = [CNBlockConfig(128, 256, 3), CNBlockConfig(256, 512, 3), CNBlockConfig(512, 1024, 27), CNBlockConfig(1024, None, 3)]
    return _convnext(block_setting, kwargs.pop("stochastic_depth_prob", 0.5), **kwargs)


def convnext_large(**kwargs: Any) -> ConvNeXt:
    block_setting = [CNBlockConfig(192, 384, 3), CNBlockConfig(384, 768, 3), CNBlockConfig(768, 1536, 27), CNBlockConfig(1536, None, 3)]
    return _convnext(block_setting, kwargs.pop("stochastic_depth_prob", 0.5), **kwargs)
