"""MobileNetV3 (large and small) on the MI355X kernels.

Mirrors models/mobilenetv3.py of the reference: InvertedResidualConfig, InvertedResidual, MobileNetV3, _mobilenet_v3_conf and the two
builders, with the reference's constructor arguments and module tree (torch's own nn.Conv2d / nn.BatchNorm2d / nn.Linear / activations
serve as PARAMETER CONTAINERS, built in the reference's order, so its state dicts load as they are and a seeded construction consumes
torch's RNG like the reference's).  Only `forward` differs:

  * every conv -> norm -> activation block is ONE launch (mobilenet.Conv2dNormActivation; the 5x5 depthwise convs run k_dwpc5x5);
  * a block with squeeze-excitation is expand, depthwise, F.global_avg_pool, F.linear_act twice, and the projection conv with the gate
    multiplied into its loads (F.conv_norm_act(..., input_scale=gate)) and the residual in its epilogue: the gated tensor never
    reaches memory;
  * the classifier is F.global_avg_pool, F.linear_act(..., "hardswish") and F.linear_bias_relu.

Inference only (norms in eval mode).  dilated=True builds the reference's tree, whose last three blocks hold a depthwise 5x5 conv at
dilation 2, padding 4 and stride 1 (k_dwpc5x5<1, 2>, F.conv_norm_act(..., dilation=2)).  Here a dilated MobileNetV3 is a SEGMENTATION
BACKBONE: its `.features` run, every block with the launches it has undilated, and that is all the reference's segmentation builders
(lraspp_mobilenet_v3_large, deeplabv3_mobilenet_v3_large: segmentation.py) call.  Its classification forward raises
NotImplementedError, before any launch; lifting that is a later change.
"""
from __future__ import annotations

from functools import partial
from typing import Any, Callable, List, Optional, Sequence

import torch
from torch import nn

from . import functional as F
from ._lib import forward_only
from .mobilenet import Conv2dNormActivation, SqueezeExcitation, _make_divisible

__all__ = ["InvertedResidualConfig", "InvertedResidual", "MobileNetV3", "mobilenet_v3_large", "mobilenet_v3_small"]


class InvertedResidualConfig:
    """models/mobilenetv3.py InvertedResidualConfig: one row of the MobileNetV3 paper's tables 1 and 2."""

    def __init__(self, input_channels: int, kernel: int, expanded_channels: int, out_channels: int, use_se: bool, activation: str,
                 stride: int, dilation: int, width_mult: float):
        self.input_channels = self.adjust_channels(input_channels, width_mult)
        self.kernel = kernel
        self.expanded_channels = self.adjust_channels(expanded_channels, width_mult)
        self.out_channels = self.adjust_channels(out_channels, width_mult)
        self.use_se = use_se
        self.use_hs = activation == "HS"
        self.stride = stride
        self.dilation = dilation

    @staticmethod
    def adjust_channels(channels: int, width_mult: float):
        return _make_divisible(channels * width_mult, 8)


class InvertedResidual(nn.Module):
    """models/mobilenetv3.py InvertedResidual: [1x1 expand] -> k x k depthwise -> [squeeze-excitation] -> 1x1 project [+ x]."""

    def __init__(self, cnf: InvertedResidualConfig, norm_layer: Callable[..., nn.Module],
                 se_layer: Callable[..., nn.Module] = partial(SqueezeExcitation, scale_activation=nn.Hardsigmoid)):
        super().__init__()
        if not (1 <= cnf.stride <= 2):
            raise ValueError("illegal stride value")
        self.use_res_connect = cnf.stride == 1 and cnf.input_channels == cnf.out_channels
        layers: List[nn.Module] = []
        activation_layer = nn.Hardswish if cnf.use_hs else nn.ReLU
        if cnf.expanded_channels != cnf.input_channels:
            layers.append(Conv2dNormActivation(cnf.input_channels, cnf.expanded_channels, kernel_size=1, norm_layer=norm_layer,
                                               activation_layer=activation_layer))
        stride = 1 if cnf.dilation > 1 else cnf.stride
        layers.append(Conv2dNormActivation(cnf.expanded_channels, cnf.expanded_channels, kernel_size=cnf.kernel, stride=stride,
                                           dilation=cnf.dilation, groups=cnf.expanded_channels, norm_layer=norm_layer,
                                           activation_layer=activation_layer))
        if cnf.use_se:
            squeeze_channels = _make_divisible(cnf.expanded_channels // 4, 8)
            layers.append(se_layer(cnf.expanded_channels, squeeze_channels))
        layers.append(Conv2dNormActivation(cnf.expanded_channels, cnf.out_channels, kernel_size=1, norm_layer=norm_layer,
                                           activation_layer=None))
        self.block = nn.Sequential(*layers)
        self.out_channels = cnf.out_channels
        self._is_cn = cnf.stride > 1
        self._dilated = cnf.dilation > 1

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return _run_block(self.block, input, input if self.use_res_connect else None)


def _run_block(layers, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The layers of an InvertedResidual's `block` (or a tail of them: SSDlite splits the C4 block behind its expansion) on the kernels:
    one launch per Conv2dNormActivation, the squeeze-excitation's gate multiplied into the projection's loads, `residual` in its
    epilogue."""
    layers = list(layers)
    y, gate = x, None
    for layer in layers[:-1]:
        if isinstance(layer, SqueezeExcitation):
            gate = layer._gate(y)  # multiplied into the projection's loads below
        else:
            y = layer(y)
    project = layers[-1]
    alpha, beta, mode = project._fold.get(project[1] if project._has_norm else None, y.device)
    return F.conv_norm_act(y, project[0].weight, project[0].bias, alpha, beta, residual, stride=1, groups=1, affine=mode, activation=None,
                           input_scale=gate)


class MobileNetV3(nn.Module):
    """models/mobilenetv3.py MobileNetV3."""

    def __init__(self, inverted_residual_setting: List[InvertedResidualConfig], last_channel: int, num_classes: int = 1000,
                 block: Optional[Callable[..., nn.Module]] = None, norm_layer: Optional[Callable[..., nn.Module]] = None,
                 dropout: float = 0.2, **kwargs: Any) -> None:
        super().__init__()
        if not inverted_residual_setting:
            raise ValueError("The inverted_residual_setting should not be empty")
        elif not (isinstance(inverted_residual_setting, Sequence)
                  and all(isinstance(s, InvertedResidualConfig) for s in inverted_residual_setting)):
            raise TypeError("The inverted_residual_setting should be List[InvertedResidualConfig]")
        if block is None:
            block = InvertedResidual
        if norm_layer is None:
            norm_layer = partial(nn.BatchNorm2d, eps=0.001, momentum=0.01)
        layers: List[nn.Module] = []
        firstconv_output_channels = inverted_residual_setting[0].input_channels
        layers.append(Conv2dNormActivation(3, firstconv_output_channels, kernel_size=3, stride=2, norm_layer=norm_layer,
                                           activation_layer=nn.Hardswish))
        for cnf in inverted_residual_setting:
            layers.append(block(cnf, norm_layer))
        lastconv_input_channels = inverted_residual_setting[-1].out_channels
        lastconv_output_channels = 6 * lastconv_input_channels
        layers.append(Conv2dNormActivation(lastconv_input_channels, lastconv_output_channels, kernel_size=1, norm_layer=norm_layer,
                                           activation_layer=nn.Hardswish))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Linear(lastconv_output_channels, last_channel), nn.Hardswish(inplace=True),
                                        nn.Dropout(p=dropout, inplace=True), nn.Linear(last_channel, num_classes))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)
        self.eval()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise RuntimeError("the MI355X MobileNetV3 is inference only: call .eval()")
        if any(getattr(m, "_dilated", False) for m in self.features):
            raise NotImplementedError("a dilated MobileNetV3 is a segmentation backbone here: its .features run (lraspp_mobilenet_v3_large, "
                                      "deeplabv3_mobilenet_v3_large), its classification forward does not")
        inp = x
        fc1, fc2 = self.classifier[0], self.classifier[3]  # Dropout is the identity in eval mode
        with torch.no_grad():  # no autograd bookkeeping per layer; the result is marked once (its backward raises)
            x = self.features(x)
            x = F.global_avg_pool(x)  # avgpool + flatten
            x = F.linear_act(x, fc1.weight, fc1.bias, "hardswish")
            x = F.linear_bias_relu(x, fc2.weight, fc2.bias, relu=False)
        return forward_only(x, "MobileNetV3.forward", inp, fc1.weight, fc2.weight)


def _mobilenet_v3_conf(arch: str, width_mult: float = 1.0, reduced_tail: bool = False, dilated: bool = False, **kwargs: Any):
    reduce_divider = 2 if reduced_tail else 1
    dilation = 2 if dilated else 1
    bneck_conf = partial(InvertedResidualConfig, width_mult=width_mult)
    adjust_channels = partial(InvertedResidualConfig.adjust_channels, width_mult=width_mult)
    if arch == "mobilenet_v3_large":
        inverted_residual_setting = [
            bneck_conf(16, 3, 16, 16, False, "RE", 1, 1),
            bneck_conf(16, 3, 64, 24, False, "RE", 2, 1),  # C1
            bneck_conf(24, 3, 72, 24, False, "RE", 1, 1),
            bneck_conf(24, 5, 72, 40, True, "RE", 2, 1),  # C2
            bneck_conf(40, 5, 120, 40, True, "RE", 1, 1),
            bneck_conf(40, 5, 120, 40, True, "RE", 1, 1),
            bneck_conf(40, 3, 240, 80, False, "HS", 2, 1),  # C3
            bneck_conf(80, 3, 200, 80, False, "HS", 1, 1),
            bneck_conf(80, 3, 184, 80, False, "HS", 1, 1),
            bneck_conf(80, 3, 184, 80, False, "HS", 1, 1),
            bneck_conf(80, 3, 480, 112, True, "HS", 1, 1),
            bneck_conf(112, 3, 672, 112, True, "HS", 1, 1),
            bneck_conf(112, 5, 672, 160 // reduce_divider, True, "HS", 2, dilation),  # C4
            bneck_conf(160 // reduce_divider, 5, 960 // reduce_divider, 160 // reduce_divider, True, "HS", 1, dilation),
            bneck_conf(160 // reduce_divider, 5, 960 // reduce_divider, 160 // reduce_divider, True, "HS", 1, dilation),
        ]
        last_channel = adjust_channels(1280 // reduce_divider)  # C5
    elif arch == "mobilenet_v3_small":
        inverted_residual_setting = [
            bneck_conf(16, 3, 16, 16, True, "RE", 2, 1),  # C1
            bneck_conf(16, 3, 72, 24, False, "RE", 2, 1),  # C2
            bneck_conf(24, 3, 88, 24, False, "RE", 1, 1),
            bneck_conf(24, 5, 96, 40, True, "HS", 2, 1),  # C3
            bneck_conf(40, 5, 240, 40, True, "HS", 1, 1),
            bneck_conf(40, 5, 240, 40, True, "HS", 1, 1),
            bneck_conf(40, 5, 120, 48, True, "HS", 1, 1),
            bneck_conf(48, 5, 144, 48, True, "HS", 1, 1),
            bneck_conf(48, 5, 288, 96 // reduce_divider, True, "HS", 2, dilation),  # C4
            bneck_conf(96 // reduce_divider, 5, 576 // reduce_divider, 96 // reduce_divider, True, "HS", 1, dilation),
            bneck_conf(96 // reduce_divider, 5, 576 // reduce_divider, 96 // reduce_divider, True, "HS", 1, dilation),
        ]
        last_channel = adjust_channels(1024 // reduce_divider)  # C5
    else:
        raise ValueError(f"Unsupported model type {arch}")
    return inverted_residual_setting, last_channel


def mobilenet_v3_large(num_classes: int = 1000, **kwargs: Any) -> MobileNetV3:
    setting, last_channel = _mobilenet_v3_conf("mobilenet_v3_large", **kwargs)
    return MobileNetV3(setting, last_channel, num_classes=num_classes,
                       **{k: v for k, v in kwargs.items() if k not in ("width_mult", "reduced_tail", "dilated")})


def mobilenet_v3_small(num_classes: int = 1000, **kwargs: Any) -> MobileNetV3:
    setting, last_channel = _mobilenet_v3_conf("mobilenet_v3_small", **kwargs)
    return MobileNetV3(setting, last_channel, num_classes=num_classes,
                       **{k: v for k, v in kwargs.items() if k not in ("width_mult", "reduced_tail", "dilated")})
