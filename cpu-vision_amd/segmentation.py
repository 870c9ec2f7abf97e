"""FCN, DeepLabV3 and LRASPP on the ResNet and MobileNetV3 backbones, on the MI355X kernels: all of models/segmentation.

Mirrors models/segmentation/_utils.py (_SimpleSegmentationModel), fcn.py (FCN, FCNHead, fcn_resnet50 / 101), deeplabv3.py
(DeepLabV3, DeepLabHead, ASPP, ASPPConv, ASPPPooling, deeplabv3_resnet50 / 101, deeplabv3_mobilenet_v3_large) and lraspp.py (LRASPP,
LRASPPHead, lraspp_mobilenet_v3_large) of the reference: the same module tree, constructor
arguments and state-dict keys, torch's own nn.Conv2d / nn.BatchNorm2d / nn.ReLU / nn.Dropout / nn.AdaptiveAvgPool2d as PARAMETER
CONTAINERS built in the reference's order, so its state dicts load as they are and a seeded construction consumes torch's RNG like
the reference's.  Only `forward` differs; the containers' own forward is never called.  Inference only (Dropout is the identity).

Launches: a 1x1 conv -> norm -> ReLU is ONE (resnet.fused_conv_norm, the pointwise kernel, whose sum is K-sliced); a 3x3 conv -> norm
-> ReLU of a head is the implicit GEMM (padding = dilation = rate for the atrous ones) summed in slices of 128 input channels, one
launch per slice (sliced_conv_norm_relu: one launch up to 128 channels; one float32 chain over 256 - 2048 channels misses the
project's accuracy condition); the last 1x1 conv of a head is F.conv_norm_act with its bias.  With s = ceil(cin / 128): FCNHead
s + 1.  ASPP 1 + len(rates) * s + 3 (F.global_avg_pool, the 1x1 conv on the (N, C, 1, 1) map, F.interpolate back to the feature
size), torch.cat, 1 for the projection; DeepLabHead that + 2 + 1.  The model adds one F.interpolate per returned head.

Beyond the reference: `labels(x)` = forward(x)["out"].argmax(1) bit for bit, the resize and the argmax as ONE launch
(F.interpolate_argmax) that writes only the labels, and without running the aux head.

The two mobile models run on mobilenet_v3_large(dilated=True).features through IntermediateLayerGetter (children "0" ... "16"; the
last three blocks' depthwise 5x5 convs at dilation 2 are k_dwpc5x5<1, 2>).  LRASPPHead is FIVE launches: cbr (the pointwise kernel),
F.global_avg_pool, F.linear_act(..., "sigmoid") for the gate, low_classifier, and F.conv1x1_gated_upsample -- high_classifier over the
resized gated map with low_classifier's output as its residual; neither the gated nor the upsampled tensor reaches memory
(DESIGN.md 3.34).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Dict, Optional, Sequence

import torch
from torch import nn

from . import _lib, mobilenetv3, resnet
from . import functional as F
from .backbone_utils import IntermediateLayerGetter
from .mobilenet import _FoldedNorm, _ParameterCache, _tensor_versions

__all__ = ["FCN", "FCNHead", "DeepLabV3", "DeepLabHead", "ASPP", "ASPPConv", "ASPPPooling", "fcn_resnet50", "fcn_resnet101",
           "deeplabv3_resnet50", "deeplabv3_resnet101", "LRASPP", "LRASPPHead", "lraspp_mobilenet_v3_large",
           "deeplabv3_mobilenet_v3_large"]


def _inference_only(module: nn.Module) -> None:
    if module.training:
        raise RuntimeError(f"the MI355X {type(module).__name__} is inference only: call .eval()")


SLICE_CHANNELS = 128  # input channels per summation slice of a head's 3x3 conv: chains of 9 x 128 = 1152 terms


class _SlicedConv(_ParameterCache):
    """What a head's 3x3 conv + norm + ReLU needs per call, recomputed when the tensors change: the folded norm, a zero shift and
    the weight cut into contiguous slices of SLICE_CHANNELS input channels."""

    def __init__(self):
        self.fold, self.key, self.weights, self.zero, self.beta = _FoldedNorm(), None, None, None, None

    def reset(self) -> None:
        self.key = None
        self.fold.reset()

    def get(self, conv: nn.Conv2d, norm: nn.Module, device):
        alpha, beta, mode = self.fold.get(norm, device)
        key = _tensor_versions(conv.weight)
        if key != self.key:
            w = conv.weight.detach()
            self.weights = [w[:, c:c + SLICE_CHANNELS].contiguous() for c in range(0, w.shape[1], SLICE_CHANNELS)]
            self.key = key
        if beta is not self.beta:  # the zero shift follows the folded norm (its device and length), not the conv's weight
            self.beta, self.zero = beta, torch.zeros_like(beta)
        return alpha, beta, mode, self.weights, self.zero


def sliced_conv_norm_relu(x: torch.Tensor, conv: nn.Conv2d, norm: nn.Module, cache: _SlicedConv) -> torch.Tensor:
    """A head's 3x3 conv (no bias) -> folded norm -> ReLU, summed in slices of SLICE_CHANNELS input channels: one
    F.conv2d_affine_act launch per slice g, p_0 = fma(alpha, s_0, beta), p_g = fma(alpha, s_g, 0) + p_(g-1) through the residual
    term, ReLU in the last -- s_g the one ascending (c, ky, kx) chain over the slice's channels.  With up to 128 channels it is the
    one launch of resnet.fused_conv_norm.  The heads read 256 - 2048 channels: one float32 chain of 9 x 2048 terms per output is
    measurably less accurate than torch's blocked GEMM sums and misses the project's accuracy condition; chains
    of 1152 terms meet it.  The sliced sum inside one launch is the implicit-GEMM kernel's next step."""
    alpha, beta, mode, weights, zero = cache.get(conv, norm, x.device)
    if conv.bias is not None or conv.groups != 1 or conv.stride != (1, 1):
        raise NotImplementedError(f"{conv}: the segmentation heads' 3x3 convs have no bias, one group and stride 1")
    y = None
    for g, w in enumerate(weights):
        xs = x if len(weights) == 1 else x[:, g * SLICE_CHANNELS:g * SLICE_CHANNELS + w.shape[1]]
        y = F.conv2d_affine_act(xs, w, None, alpha, beta if g == 0 else zero, y, stride=1, padding=conv.padding, dilation=conv.dilation,
                                groups=1, affine=mode, activation="relu" if g == len(weights) - 1 else None)
    return y


def _classify(x: torch.Tensor, conv: nn.Conv2d) -> torch.Tensor:
    """The last 1x1 conv of a head, with its bias."""
    return F.conv_norm_act(x, conv.weight, conv.bias, None, None, None, stride=1, groups=1, affine=None, activation=None)


class _Labels:
    """labels(x) of a segmentation model, on its `_out_logits(x)`: the "out" head's logits before the final resize."""

    def labels(self, x: torch.Tensor, dtype: torch.dtype = torch.int64) -> torch.Tensor:
        """forward(x)["out"].argmax(1) bit for bit as (N, H, W) of `dtype` (int64, or uint8 for up to 256 classes): the resize and the
        argmax are one launch (F.interpolate_argmax), the upsampled logits never reach memory and the aux head does not run."""
        _inference_only(self)
        with torch.no_grad():
            return F.interpolate_argmax(self._out_logits(x), size=x.shape[-2:], dtype=dtype)


class _SimpleSegmentationModel(_Labels, nn.Module):
    """models/segmentation/_utils.py: backbone -> classifier (-> aux_classifier) -> resize to the input."""
    __constants__ = ["aux_classifier"]

    def __init__(self, backbone: nn.Module, classifier: nn.Module, aux_classifier: Optional[nn.Module] = None) -> None:
        super().__init__()
        self.backbone = backbone
        self.classifier = classifier
        self.aux_classifier = aux_classifier
        self.eval()

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        _inference_only(self)
        input_shape = x.shape[-2:]
        result = OrderedDict()
        with torch.no_grad():  # no autograd bookkeeping per layer; the results are marked once (their backward raises)
            features = self.backbone(x)
            y = self.classifier(features["out"])
            result["out"] = F.interpolate(y, size=input_shape, mode="bilinear", align_corners=False)
            if self.aux_classifier is not None:
                y = self.aux_classifier(features["aux"])
                result["aux"] = F.interpolate(y, size=input_shape, mode="bilinear", align_corners=False)
        dep = next((p for p in self.parameters() if p.requires_grad), None)
        return OrderedDict((k, _lib.forward_only(v, f"{type(self).__name__}.forward", x, dep)) for k, v in result.items())

    def _out_logits(self, x: torch.Tensor) -> torch.Tensor:
        return self.classifier(self.backbone(x)["out"])


class FCN(_SimpleSegmentationModel):
    """models/segmentation/fcn.py FCN: a backbone returning "out" (and "aux"), an FCNHead on each."""


class FCNHead(nn.Sequential):
    """fcn.py FCNHead: 3x3 conv + norm + ReLU (sliced_conv_norm_relu), Dropout(0.1) (identity), 1x1 conv with bias."""

    def __init__(self, in_channels: int, channels: int) -> None:
        inter_channels = in_channels // 4
        super().__init__(nn.Conv2d(in_channels, inter_channels, 3, padding=1, bias=False), nn.BatchNorm2d(inter_channels), nn.ReLU(),
                         nn.Dropout(0.1), nn.Conv2d(inter_channels, channels, 1))
        self._fold = _SlicedConv()
        self.eval()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _inference_only(self)
        return _classify(sliced_conv_norm_relu(x, self[0], self[1], self._fold), self[4])


class DeepLabV3(_SimpleSegmentationModel):
    """models/segmentation/deeplabv3.py DeepLabV3: a backbone returning "out" (and "aux"), a DeepLabHead (and an FCNHead)."""


class _ConvNormReLU(nn.Sequential):
    """conv, norm, ReLU[, Dropout] as containers (the reference's plain nn.Sequential of them): one launch."""

    def __init__(self, *layers: nn.Module) -> None:
        super().__init__(*layers)
        self._fold = _FoldedNorm()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return resnet.fused_conv_norm(x, self[0], self[1], self._fold, relu=True)


class ASPPConv(_ConvNormReLU):
    """deeplabv3.py ASPPConv: the atrous 3x3 conv (padding = dilation = rate) + norm + ReLU (sliced_conv_norm_relu)."""

    def __init__(self, in_channels: int, out_channels: int, dilation: int) -> None:
        super().__init__(nn.Conv2d(in_channels, out_channels, 3, padding=dilation, dilation=dilation, bias=False),
                         nn.BatchNorm2d(out_channels), nn.ReLU())
        self._fold = _SlicedConv()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return sliced_conv_norm_relu(x, self[0], self[1], self._fold)


class ASPPPooling(nn.Sequential):
    """deeplabv3.py ASPPPooling: global average pool -> 1x1 conv + norm + ReLU -> bilinear resize back to the feature size.  The
    pool is F.global_avg_pool (float64 sums).  The resize stays an F.interpolate launch: with a 1x1 source both taps of an axis read
    the one value v, but fma(w0, v, w1 * v) is not v for every weight pair, and an infinity becomes NaN, as in the reference."""

    def __init__(self, in_channels: int, out_channels: int) -> None:
        super().__init__(nn.AdaptiveAvgPool2d(1), nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels),
                         nn.ReLU())
        self._fold = _FoldedNorm()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        size = x.shape[-2:]
        pooled = F.global_avg_pool(x)
        y = resnet.fused_conv_norm(pooled.view(pooled.shape[0], pooled.shape[1], 1, 1), self[1], self[2], self._fold, relu=True)
        return F.interpolate(y, size=size, mode="bilinear", align_corners=False)


class ASPP(nn.Module):
    """deeplabv3.py ASPP: a 1x1 branch, one atrous branch per rate and the pooling branch, concatenated and projected."""

    def __init__(self, in_channels: int, atrous_rates: Sequence[int], out_channels: int = 256) -> None:
        super().__init__()
        modules = [_ConvNormReLU(nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU())]
        rates = tuple(atrous_rates)
        for rate in rates:
            modules.append(ASPPConv(in_channels, out_channels, rate))
        modules.append(ASPPPooling(in_channels, out_channels))
        self.convs = nn.ModuleList(modules)
        self.project = _ConvNormReLU(nn.Conv2d(len(self.convs) * out_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels),
                                     nn.ReLU(), nn.Dropout(0.5))
        self.eval()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _inference_only(self)
        return self.project(torch.cat([conv(x) for conv in self.convs], dim=1))


class DeepLabHead(nn.Sequential):
    """deeplabv3.py DeepLabHead: ASPP -> 3x3 conv + norm + ReLU (sliced_conv_norm_relu: two launches) -> 1x1 conv with bias."""

    def __init__(self, in_channels: int, num_classes: int, atrous_rates: Sequence[int] = (12, 24, 36)) -> None:
        super().__init__(ASPP(in_channels, atrous_rates), nn.Conv2d(256, 256, 3, padding=1, bias=False), nn.BatchNorm2d(256), nn.ReLU(),
                         nn.Conv2d(256, num_classes, 1))
        self._fold = _SlicedConv()
        self.eval()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _inference_only(self)
        return _classify(sliced_conv_norm_relu(self[0](x), self[1], self[2], self._fold), self[4])


def _segmentation_resnet(name: str, model, head, depth: str, weights, num_classes: Optional[int], aux_loss: Optional[bool],
                         weights_backbone) -> _SimpleSegmentationModel:
    if weights is not None or weights_backbone is not None:
        raise ValueError(f"{name}: the package ships no weight files, weights and weights_backbone must be None; "
                         "load a state dict with load_state_dict")
    if num_classes is None:
        num_classes = 21
    backbone = resnet.__dict__[depth](replace_stride_with_dilation=[False, True, True])
    return_layers = {"layer4": "out"}
    if aux_loss:
        return_layers["layer3"] = "aux"
    body = IntermediateLayerGetter(backbone, return_layers=return_layers)
    aux_classifier = FCNHead(1024, num_classes) if aux_loss else None
    return model(body, head(2048, num_classes), aux_classifier)


class LRASPPHead(nn.Module):
    """lraspp.py LRASPPHead: low_classifier(low) + high_classifier(interpolate(cbr(high) * scale(high), size=low.shape[-2:])) as five
    launches: cbr is the pointwise kernel; the gate scale(high) is F.global_avg_pool and F.linear_act(..., "sigmoid") (float64 sums,
    as a squeeze-excitation's); low_classifier with its bias; then F.conv1x1_gated_upsample: high_classifier over the resized gated
    map, the gate product and the four-tap blend in its loads, low_classifier's output as its residual."""

    def __init__(self, low_channels: int, high_channels: int, num_classes: int, inter_channels: int) -> None:
        super().__init__()
        self.cbr = nn.Sequential(nn.Conv2d(high_channels, inter_channels, 1, bias=False), nn.BatchNorm2d(inter_channels),
                                 nn.ReLU(inplace=True))
        self.scale = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(high_channels, inter_channels, 1, bias=False), nn.Sigmoid())
        self.low_classifier = nn.Conv2d(low_channels, num_classes, 1)
        self.high_classifier = nn.Conv2d(inter_channels, num_classes, 1)
        self._fold = _FoldedNorm()
        self.eval()

    def forward(self, input: Dict[str, torch.Tensor]) -> torch.Tensor:
        _inference_only(self)
        low, high = input["low"], input["high"]
        x = resnet.fused_conv_norm(high, self.cbr[0], self.cbr[1], self._fold, relu=True)
        gate = F.linear_act(F.global_avg_pool(high), self.scale[1].weight, None, "sigmoid")
        return F.conv1x1_gated_upsample(x, gate, self.high_classifier.weight, self.high_classifier.bias,
                                        _classify(low, self.low_classifier), size=low.shape[-2:])


class LRASPP(_Labels, nn.Module):
    """lraspp.py LRASPP: a backbone returning "low" and "high", an LRASPPHead, the resize to the input."""

    def __init__(self, backbone: nn.Module, low_channels: int, high_channels: int, num_classes: int, inter_channels: int = 128) -> None:
        super().__init__()
        self.backbone = backbone
        self.classifier = LRASPPHead(low_channels, high_channels, num_classes, inter_channels)
        self.eval()

    def _out_logits(self, x: torch.Tensor) -> torch.Tensor:
        return self.classifier(self.backbone(x))

    def forward(self, input: torch.Tensor) -> Dict[str, torch.Tensor]:
        _inference_only(self)
        with torch.no_grad():  # no autograd bookkeeping per layer; the result is marked once (its backward raises)
            out = F.interpolate(self._out_logits(input), size=input.shape[-2:], mode="bilinear", align_corners=False)
        dep = next((p for p in self.parameters() if p.requires_grad), None)
        return OrderedDict(out=_lib.forward_only(out, "LRASPP.forward", input, dep))


def _mobilenet_v3_stages(name: str, weights, weights_backbone):
    """mobilenet_v3_large(dilated=True).features and the reference's stage_indices on it: [0, 2, 4, 7, 13, 16]."""
    if weights is not None or weights_backbone is not None:
        raise ValueError(f"{name}: the package ships no weight files, weights and weights_backbone must be None; "
                         "load a state dict with load_state_dict")
    backbone = mobilenetv3.mobilenet_v3_large(dilated=True).features
    stage_indices = [0] + [i for i, b in enumerate(backbone) if getattr(b, "_is_cn", False)] + [len(backbone) - 1]
    return backbone, stage_indices


def lraspp_mobilenet_v3_large(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                              weights_backbone: Optional[Any] = None, **kwargs: Any) -> LRASPP:
    """lraspp.py lraspp_mobilenet_v3_large: LRASPP on the dilated MobileNetV3-large: "low" = stage_indices[-4] (features.4: 40 channels,
    stride 8), "high" = the last feature (960 channels, stride 16), 21 classes unless `num_classes` says otherwise.  Weights as for
    fcn_resnet50."""
    if kwargs.pop("aux_loss", False):
        raise NotImplementedError("This model does not use auxiliary loss")
    backbone, stage_indices = _mobilenet_v3_stages("lraspp_mobilenet_v3_large", weights, weights_backbone)
    if num_classes is None:
        num_classes = 21
    low_pos, high_pos = stage_indices[-4], stage_indices[-1]
    low_channels, high_channels = backbone[low_pos].out_channels, backbone[high_pos].out_channels
    body = IntermediateLayerGetter(backbone, return_layers={str(low_pos): "low", str(high_pos): "high"})
    return LRASPP(body, low_channels, high_channels, num_classes)


def deeplabv3_mobilenet_v3_large(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                                 aux_loss: Optional[bool] = None, weights_backbone: Optional[Any] = None, **kwargs: Any) -> DeepLabV3:
    """deeplabv3.py deeplabv3_mobilenet_v3_large: DeepLabV3 (DeepLabHead(960)) on the dilated MobileNetV3-large's last feature, an
    FCNHead(40) on features.4 as "aux" when `aux_loss`, 21 classes unless `num_classes` says otherwise.  Weights as for fcn_resnet50."""
    backbone, stage_indices = _mobilenet_v3_stages("deeplabv3_mobilenet_v3_large", weights, weights_backbone)
    if num_classes is None:
        num_classes = 21
    out_pos, aux_pos = stage_indices[-1], stage_indices[-4]
    out_inplanes, aux_inplanes = backbone[out_pos].out_channels, backbone[aux_pos].out_channels
    return_layers = {str(out_pos): "out"}
    if aux_loss:
        return_layers[str(aux_pos)] = "aux"
    body = IntermediateLayerGetter(backbone, return_layers=return_layers)
    aux_classifier = FCNHead(aux_inplanes, num_classes) if aux_loss else None  # before the head, as the reference draws
    return DeepLabV3(body, DeepLabHead(out_inplanes, num_classes), aux_classifier)


def fcn_resnet50(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                 aux_loss: Optional[bool] = None, weights_backbone: Optional[Any] = None, **kwargs: Any) -> FCN:
    """fcn.py fcn_resnet50: an FCN on ResNet-50 with layer3 and layer4 dilated (output stride 8), 21 classes unless `num_classes` says
    otherwise, an FCNHead(1024) on layer3 as "aux" when `aux_loss`.

    The package ships no weight files: `weights` and `weights_backbone` must be None; load a state dict of the reference's model with
    load_state_dict (the keys are the reference's)."""
    return _segmentation_resnet("fcn_resnet50", FCN, FCNHead, "resnet50", weights, num_classes, aux_loss, weights_backbone)


def fcn_resnet101(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                  aux_loss: Optional[bool] = None, weights_backbone: Optional[Any] = None, **kwargs: Any) -> FCN:
    """fcn.py fcn_resnet101: fcn_resnet50 on ResNet-101."""
    return _segmentation_resnet("fcn_resnet101", FCN, FCNHead, "resnet101", weights, num_classes, aux_loss, weights_backbone)


def deeplabv3_resnet50(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                       aux_loss: Optional[bool] = None, weights_backbone: Optional[Any] = None, **kwargs: Any) -> DeepLabV3:
    """deeplabv3.py deeplabv3_resnet50: DeepLabV3 (ASPP rates 12, 24, 36) on ResNet-50 with layer3 and layer4 dilated, 21 classes unless
    `num_classes` says otherwise, an FCNHead(1024) on layer3 as "aux" when `aux_loss`.  Weights as for fcn_resnet50."""
    return _segmentation_resnet("deeplabv3_resnet50", DeepLabV3, DeepLabHead, "resnet50", weights, num_classes, aux_loss, weights_backbone)


def deeplabv3_resnet101(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                        aux_loss: Optional[bool] = None, weights_backbone: Optional[Any] = None, **kwargs: Any) -> DeepLabV3:
    """deeplabv3.py deeplabv3_resnet101: deeplabv3_resnet50 on ResNet-101."""
    return _segmentation_resnet("deeplabv3_resnet101", DeepLabV3, DeepLabHead, "resnet101", weights, num_classes, aux_loss, weights_backbone)
