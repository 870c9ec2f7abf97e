"""ResNet-18/34/50/101/152 and the wide variants on the MI355X kernels: every conv -> norm [-> + identity] [-> ReLU] is ONE launch.

Mirrors models/resnet.py:22-282 of the reference the way mobilenet.py mirrors models/mobilenetv2.py: same constructor arguments,
same module tree with the reference's names (conv1, bn1, layer1.0.conv1, layer1.0.downsample.0, ..., fc).  torch's own
nn.Conv2d / nn.BatchNorm2d / nn.ReLU / nn.MaxPool2d / nn.AdaptiveAvgPool2d / nn.Linear serve as PARAMETER CONTAINERS built in
the reference's order, so the reference's state dicts load as they are and a seeded construction consumes torch's RNG exactly
like the reference's.  Only `forward` differs; the containers' own forward is never called.  Inference only: norms are
nn.BatchNorm2d in eval mode (folded as one fmaf: affine "fma") or mobilenet.FrozenBatchNorm2d ("mul_add"), cached per layer.

Launches: BasicBlock 2 (+ 1 with a downsample), Bottleneck 3 (+ 1).  The downsample conv carries its norm and no activation;
the block's last conv carries `residual=identity` and the ReLU in its epilogue.  1x1 convs at stride 1 run the pointwise kernel
(F.conv_norm_act: its summation order is stated by F.conv1x1_k_slices), everything else -- the 7x7 stride-2 stem, the 3x3 convs
at any stride / dilation / groups, the 1x1 stride-2 downsample -- the implicit GEMM with the full epilogue
(F.conv2d_affine_act: one ascending (c, ky, kx) chain per output).

One deliberate superset of the reference: BasicBlock accepts dilation > 1 (both 3x3 convs then take dilation = padding =
`dilation`, as Bottleneck's conv2 does), where the reference raises NotImplementedError; resnet18 / 34 therefore take
replace_stride_with_dilation too.  The resnext* builders are not provided (`groups` is accepted and runs one launch per group,
untuned).
"""
from __future__ import annotations

from typing import Callable, List, Optional, Type, Union

import torch
from torch import nn

from . import _lib
from . import functional as F
from .mobilenet import FrozenBatchNorm2d, _FoldedNorm

__all__ = ["ResNet", "BasicBlock", "Bottleneck", "conv3x3", "conv1x1", "resnet18", "resnet34", "resnet50", "resnet101",
           "resnet152", "wide_resnet50_2", "wide_resnet101_2"]


def conv3x3(in_planes: int, out_planes: int, stride: int = 1, groups: int = 1, dilation: int = 1) -> nn.Conv2d:
    """3x3 convolution with padding (resnet.py:38-50)."""
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=dilation, groups=groups, bias=False,
                     dilation=dilation)


def conv1x1(in_planes: int, out_planes: int, stride: int = 1) -> nn.Conv2d:
    """1x1 convolution (resnet.py:53-55)."""
    return nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


def _checked_norm(norm: nn.Module) -> nn.Module:
    if not isinstance(norm, (nn.BatchNorm2d, FrozenBatchNorm2d)):
        raise NotImplementedError(f"norm layer {type(norm).__name__}: BatchNorm2d (eval) and FrozenBatchNorm2d fold into the conv")
    return norm


def fused_conv_norm(x: torch.Tensor, conv: nn.Conv2d, norm: nn.Module, cache: _FoldedNorm, relu: bool,
                    residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv -> folded norm -> (+ residual) -> ReLU? as one launch; the modules only hold the parameters."""
    alpha, beta, mode = cache.get(norm, x.device)
    act = "relu" if relu else None
    if conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.dilation == (1, 1) and conv.padding == (0, 0) and conv.groups == 1:
        return F.conv_norm_act(x, conv.weight, conv.bias, alpha, beta, residual, stride=1, groups=1, affine=mode, activation=act)
    return F.conv2d_affine_act(x, conv.weight, conv.bias, alpha, beta, residual, stride=conv.stride, padding=conv.padding,
                               dilation=conv.dilation, groups=conv.groups, affine=mode, activation=act)


class _Block(nn.Module):
    """What the two block types share: the downsample branch and the inference-only check."""

    def _identity(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise RuntimeError("the MI355X ResNet blocks are inference only: call .eval()")
        if self.downsample is None:
            return x
        return fused_conv_norm(x, self.downsample[0], self.downsample[1], self._fold_down, relu=False)


class BasicBlock(_Block):
    """resnet.py:58-105: 3x3 + norm + ReLU -> 3x3 + norm (+ identity) + ReLU: two launches, three with a downsample."""
    expansion: int = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None, groups: int = 1,
                 base_width: int = 64, dilation: int = 1, norm_layer: Optional[Callable[..., nn.Module]] = None) -> None:
        super().__init__()
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        if groups != 1 or base_width != 64:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        # both self.conv1 and self.downsample layers downsample the input when stride != 1
        self.conv1 = conv3x3(inplanes, planes, stride, dilation=dilation)
        self.bn1 = _checked_norm(norm_layer(planes))
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes, dilation=dilation)
        self.bn2 = _checked_norm(norm_layer(planes))
        self.downsample = downsample
        self.stride = stride
        self._fold1, self._fold2, self._fold_down = _FoldedNorm(), _FoldedNorm(), _FoldedNorm()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        identity = self._identity(x)
        out = fused_conv_norm(x, self.conv1, self.bn1, self._fold1, relu=True)
        return fused_conv_norm(out, self.conv2, self.bn2, self._fold2, relu=True, residual=identity)


class Bottleneck(_Block):
    """resnet.py:108-163 (the stride sits on the 3x3 conv: ResNet V1.5): 1x1 + norm + ReLU -> 3x3 + norm + ReLU -> 1x1 + norm
    (+ identity) + ReLU: three launches, four with a downsample."""
    expansion: int = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None, groups: int = 1,
                 base_width: int = 64, dilation: int = 1, norm_layer: Optional[Callable[..., nn.Module]] = None) -> None:
        super().__init__()
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        width = int(planes * (base_width / 64.0)) * groups
        # both self.conv2 and self.downsample layers downsample the input when stride != 1
        self.conv1 = conv1x1(inplanes, width)
        self.bn1 = _checked_norm(norm_layer(width))
        self.conv2 = conv3x3(width, width, stride, groups, dilation)
        self.bn2 = _checked_norm(norm_layer(width))
        self.conv3 = conv1x1(width, planes * self.expansion)
        self.bn3 = _checked_norm(norm_layer(planes * self.expansion))
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride
        self._fold1, self._fold2, self._fold3, self._fold_down = _FoldedNorm(), _FoldedNorm(), _FoldedNorm(), _FoldedNorm()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        identity = self._identity(x)
        out = fused_conv_norm(x, self.conv1, self.bn1, self._fold1, relu=True)
        out = fused_conv_norm(out, self.conv2, self.bn2, self._fold2, relu=True)
        return fused_conv_norm(out, self.conv3, self.bn3, self._fold3, relu=True, residual=identity)


class ResNet(nn.Module):
    """models/resnet.py:166-282."""

    def __init__(self, block: Type[Union[BasicBlock, Bottleneck]], layers: List[int], num_classes: int = 1000,
                 zero_init_residual: bool = False, groups: int = 1, width_per_group: int = 64,
                 replace_stride_with_dilation: Optional[List[bool]] = None,
                 norm_layer: Optional[Callable[..., nn.Module]] = None) -> None:
        super().__init__()
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        self._norm_layer = norm_layer
        self.inplanes = 64
        self.dilation = 1
        if replace_stride_with_dilation is None:
            # each element in the tuple indicates if we should replace the 2x2 stride with a dilated convolution instead
            replace_stride_with_dilation = [False, False, False]
        if len(replace_stride_with_dilation) != 3:
            raise ValueError("replace_stride_with_dilation should be None "
                             f"or a 3-element tuple, got {replace_stride_with_dilation}")
        self.groups = groups
        self.base_width = width_per_group
        self.conv1 = nn.Conv2d(3, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = _checked_norm(norm_layer(self.inplanes))
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2, dilate=replace_stride_with_dilation[0])
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2, dilate=replace_stride_with_dilation[1])
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2, dilate=replace_stride_with_dilation[2])
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)

        for m in self.modules():  # resnet.py:208-213
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        # Zero-initialize the last BN in each residual branch, so that the residual branch starts with zeros, and each
        # residual block behaves like an identity (resnet.py:215-223)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck) and m.bn3.weight is not None:
                    nn.init.constant_(m.bn3.weight, 0)
                elif isinstance(m, BasicBlock) and m.bn2.weight is not None:
                    nn.init.constant_(m.bn2.weight, 0)
        self._fold = _FoldedNorm()
        self.eval()

    def _make_layer(self, block: Type[Union[BasicBlock, Bottleneck]], planes: int, blocks: int, stride: int = 1,
                    dilate: bool = False) -> nn.Sequential:
        norm_layer = self._norm_layer
        downsample = None
        previous_dilation = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride),
                                       _checked_norm(norm_layer(planes * block.expansion)))
        layers = [block(self.inplanes, planes, stride, downsample, self.groups, self.base_width, previous_dilation, norm_layer)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, groups=self.groups, base_width=self.base_width, dilation=self.dilation,
                                norm_layer=norm_layer))
        return nn.Sequential(*layers)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise RuntimeError("the MI355X ResNet is inference only: call .eval()")
        inp = x
        with torch.no_grad():  # no autograd bookkeeping per layer; the result is marked once (its backward raises)
            x = fused_conv_norm(x, self.conv1, self.bn1, self._fold, relu=True)
            mp = self.maxpool
            x = F.max_pool2d(x, mp.kernel_size, mp.stride, mp.padding)
            x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
            x = F.adaptive_avg_pool2d(x, (1, 1))
            x = torch.flatten(x, 1)
            x = F.linear_bias_relu(x, self.fc.weight, self.fc.bias, relu=False)
        return _lib.forward_only(x, "ResNet.forward", inp, self.fc.weight)


def _resnet(block, layers: List[int], **kwargs) -> ResNet:
    return ResNet(block, layers, **kwargs)


def resnet18(**kwargs) -> ResNet:
    return _resnet(BasicBlock, [2, 2, 2, 2], **kwargs)


def resnet34(**kwargs) -> ResNet:
    return _resnet(BasicBlock, [3, 4, 6, 3], **kwargs)


def resnet50(**kwargs) -> ResNet:
    return _resnet(Bottleneck, [3, 4, 6, 3], **kwargs)


def resnet101(**kwargs) -> ResNet:
    return _resnet(Bottleneck, [3, 4, 23, 3], **kwargs)


def resnet152(**kwargs) -> ResNet:
    return _resnet(Bottleneck, [3, 8, 36, 3], **kwargs)


def wide_resnet50_2(**kwargs) -> ResNet:
    """The bottleneck's 3x3 convs are twice as wide (width_per_group = 128); the outer 1x1 channels are ResNet-50's."""
    kwargs["width_per_group"] = 64 * 2
    return _resnet(Bottleneck, [3, 4, 6, 3], **kwargs)


def wide_resnet101_2(**kwargs) -> ResNet:
    kwargs["width_per_group"] = 64 * 2
    return _resnet(Bottleneck, [3, 4, 23, 3], **kwargs)
