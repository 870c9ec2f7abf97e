"""SSDlite inference on the MI355X kernels: models/detection/ssdlite.py of the reference -- SSDLiteHead, SSDLiteClassificationHead,
SSDLiteRegressionHead, SSDLiteFeatureExtractorMobileNet and the ssdlite320_mobilenet_v3_large builder -- with the same classes,
constructor arguments, defaults, argument errors, child names (backbone.features.{0,1}.*, backbone.extra.{i}.{0,1,2}.*,
head.classification_head.module_list.{i}.{0.0, 0.1, 1}, head.regression_head.module_list.{i}.*), state-dict keys and initialisation
order.  Only `forward` differs.  Everything SSDlite shares with SSD300 is ssd.py's: SSD, SSDScoringHead, the post-processing.

SSDlite's compute pattern is the depthwise-separable block, depthwise 3x3 + norm + ReLU6 followed by a 1x1 conv, on maps of 20 x 20
cells and smaller where every launch is latency.  Such a block is ONE F.dwconv_pointwise launch (mv_dwconv3x3_conv1x1_f32,
k_conv1x1_dw): the depthwise stage is computed in the loads of the pointwise MFMA kernel and the hidden tensor never reaches memory.
  * a prediction block (6 levels x 2 heads): one launch, the depthwise norm folded, the 1x1 conv's bias in the epilogue (at 320 x 320:
    4 of the 12 blocks; the other 8 are two launches each, see below);
  * an extra block: the first 1x1 through Conv2dNormActivation.forward, then one launch for the stride-2 depthwise conv and the last
    1x1 with its folded norm and ReLU6;
  * the back half of the C4 block (depthwise 5x5 stride 2, squeeze-excitation, projection) runs as mobilenetv3.InvertedResidual does,
    the gate in the projection's loads.
Where the fused launch was measured slower than the two launches it replaces, the block runs as those two launches: `_use_fused`
states the rule once (the bits are the same either way; DESIGN.md 3.35 has what was measured).

Inference only, float32 only.  There are no weight files.
"""
from __future__ import annotations

import warnings
from collections import OrderedDict
from functools import partial
from typing import Any, Callable, Dict, List, Optional

import torch
from torch import nn, Tensor

from . import _lib
from . import functional as F
from .anchor_utils import DefaultBoxGenerator
from .backbone_utils import _validate_trainable_layers
from .mobilenet import _ACTIVATIONS, Conv2dNormActivation
from .mobilenetv3 import _run_block, mobilenet_v3_large
from .ssd import SSD, SSDScoringHead, _retrieve_out_channels

__all__ = ["SSDLiteHead", "SSDLiteClassificationHead", "SSDLiteRegressionHead", "SSDLiteFeatureExtractorMobileNet",
           "ssdlite320_mobilenet_v3_large"]


# Building blocks of SSDlite as described in section 6.2 of MobileNetV2 paper
def _prediction_block(in_channels: int, out_channels: int, kernel_size: int, norm_layer: Callable[..., nn.Module]) -> nn.Sequential:
    return nn.Sequential(
        # 3x3 depthwise with stride 1 and padding 1
        Conv2dNormActivation(in_channels, in_channels, kernel_size=kernel_size, groups=in_channels, norm_layer=norm_layer,
                             activation_layer=nn.ReLU6),
        # 1x1 projetion to output channels
        nn.Conv2d(in_channels, out_channels, 1),
    )


def _extra_block(in_channels: int, out_channels: int, norm_layer: Callable[..., nn.Module]) -> nn.Sequential:
    activation = nn.ReLU6
    intermediate_channels = out_channels // 2
    return nn.Sequential(
        # 1x1 projection to half output channels
        Conv2dNormActivation(in_channels, intermediate_channels, kernel_size=1, norm_layer=norm_layer, activation_layer=activation),
        # 3x3 depthwise with stride 2 and padding 1
        Conv2dNormActivation(intermediate_channels, intermediate_channels, kernel_size=3, stride=2, groups=intermediate_channels,
                             norm_layer=norm_layer, activation_layer=activation),
        # 1x1 projetion to output channels
        Conv2dNormActivation(intermediate_channels, out_channels, kernel_size=1, norm_layer=norm_layer, activation_layer=activation),
    )


def _normal_init(conv: nn.Module):
    for layer in conv.modules():
        if isinstance(layer, nn.Conv2d):
            torch.nn.init.normal_(layer.weight, mean=0.0, std=0.03)
            if layer.bias is not None:
                torch.nn.init.constant_(layer.bias, 0.0)


def _use_fused(cin: int, cout: int) -> bool:
    """The dispatch rule of a depthwise-separable block (cin depthwise channels, cout outputs of the 1x1 conv), from the per-site times
    of tools/perf_ssdlite.py at batch 1 and batch 32 (profiles/perf_ssdlite.json): one F.dwconv_pointwise launch wins by a
    third where the block is a launch's latency -- up to 128 channels, or up to 256 with more than 64 outputs: the three coarsest
    classification levels, the coarsest regression level and all four extra blocks of ssdlite320.  It loses by more than the same-code
    spread where the depthwise stage is real work that every block of output channels recomputes and every K chunk waits for: more
    than 256 channels (the K-by-4 sliced instances: the 20 x 20, 10 x 10 and 5 x 5 levels), and 256 channels into at most 64 outputs
    (four X units per thread).  Those blocks run as the two launches.  The result has the same bits either way."""
    return cin <= 128 or (cin <= 256 and cout > 64)


def _separable(x: Tensor, depthwise: Conv2dNormActivation, pointwise: nn.Module, fused: Optional[bool] = None) -> Tensor:
    """A depthwise 3x3 Conv2dNormActivation followed by a 1x1 conv -- an nn.Conv2d with its bias, or a Conv2dNormActivation with its
    norm and activation -- as ONE F.dwconv_pointwise launch, or as the two F.conv_norm_act launches where `_use_fused` says so
    (fused: True / False overrides the rule: tools/perf_ssdlite.py).  The modules only hold the parameters."""
    dw = depthwise[0]
    if fused is None:
        fused = _use_fused(dw.in_channels, pointwise.out_channels)
    if not fused:
        hidden = depthwise(x)
        return F.conv_norm_act(hidden, pointwise.weight, pointwise.bias) if isinstance(pointwise, nn.Conv2d) else pointwise(hidden)
    if not (dw.kernel_size == (3, 3) and dw.padding == (1, 1) and dw.dilation == (1, 1) and dw.padding_mode == "zeros"
            and dw.groups == dw.in_channels == dw.out_channels and dw.stride in ((1, 1), (2, 2))):
        raise NotImplementedError(f"{dw}: the MI355X depthwise-separable block covers depthwise 3x3 convs, padding 1, stride 1 or 2")
    if isinstance(pointwise, Conv2dNormActivation):
        pw, pw_norm, pw_act, fold = pointwise[0], (pointwise[1] if pointwise._has_norm else None), \
            (pointwise[-1] if pointwise._has_act else None), pointwise._fold
    else:
        pw, pw_norm, pw_act, fold = pointwise, None, None, None
    if not (isinstance(pw, nn.Conv2d) and pw.kernel_size == (1, 1) and pw.stride == (1, 1) and pw.padding == (0, 0) and pw.groups == 1):
        raise NotImplementedError(f"{pw}: the MI355X depthwise-separable block ends in a 1x1 conv at stride 1")
    dw_act = depthwise[-1] if depthwise._has_act else None
    for act in (dw_act, pw_act):
        if act is not None and type(act) not in _ACTIVATIONS:
            raise NotImplementedError(f"activation {type(act).__name__}")
    dw_alpha, dw_beta, dw_mode = depthwise._fold.get(depthwise[1] if depthwise._has_norm else None, x.device)
    alpha, beta, mode = fold.get(pw_norm, x.device) if fold is not None else (None, None, None)
    return F.dwconv_pointwise(x, dw.weight, dw.bias, dw_alpha, dw_beta, pw.weight, pw.bias, alpha, beta, None, stride=dw.stride[0],
                              dw_affine=dw_mode, dw_activation=None if dw_act is None else _ACTIVATIONS[type(dw_act)], affine=mode,
                              activation=None if pw_act is None else _ACTIVATIONS[type(pw_act)])


class _SSDLiteScoringHead(SSDScoringHead):
    """SSDScoringHead over prediction blocks: module_list[idx](x) is one F.dwconv_pointwise launch, or two launches (`_use_fused`)."""

    def _get_result_from_module_list(self, x: Tensor, idx: int) -> Tensor:
        num_blocks = len(self.module_list)
        if idx < 0:
            idx += num_blocks
        block = self.module_list[idx]
        return _separable(x, block[0], block[1])

    def forward(self, x: List[Tensor]) -> List[Tensor]:
        """SSDScoringHead.forward with the autograd dependencies gathered once: a prediction block has six parameters and three
        modules where SSD's has two and one, and walking them once per level cost as much host time as the head's launches."""
        if self.training:
            raise RuntimeError(f"the MI355X {type(self).__name__} is inference only: call .eval()")
        with torch.no_grad():
            out = [self._get_result_from_module_list(features, i) for i, features in enumerate(x)]
        if not torch.is_grad_enabled():
            return out  # forward_only would return every map as it is
        deps = (*x, *self.parameters())
        return [_lib.forward_only(v, f"{type(self).__name__}.forward", *deps) for v in out]


class SSDLiteHead(nn.Module):
    """ssdlite.py SSDLiteHead.  forward(x: List[Tensor]) -> {"bbox_regression", "cls_logits"}: the per-level NCHW maps, as SSDHead's."""

    def __init__(self, in_channels: List[int], num_anchors: List[int], num_classes: int, norm_layer: Callable[..., nn.Module]):
        super().__init__()
        self.classification_head = SSDLiteClassificationHead(in_channels, num_anchors, num_classes, norm_layer)
        self.regression_head = SSDLiteRegressionHead(in_channels, num_anchors, norm_layer)
        self.eval()

    def forward(self, x: List[Tensor]) -> Dict[str, List[Tensor]]:
        return {
            "bbox_regression": self.regression_head(x),
            "cls_logits": self.classification_head(x),
        }


class SSDLiteClassificationHead(_SSDLiteScoringHead):
    def __init__(self, in_channels: List[int], num_anchors: List[int], num_classes: int, norm_layer: Callable[..., nn.Module]):
        cls_logits = nn.ModuleList()
        for channels, anchors in zip(in_channels, num_anchors):
            cls_logits.append(_prediction_block(channels, num_classes * anchors, 3, norm_layer))
        _normal_init(cls_logits)
        super().__init__(cls_logits, num_classes)


class SSDLiteRegressionHead(_SSDLiteScoringHead):
    def __init__(self, in_channels: List[int], num_anchors: List[int], norm_layer: Callable[..., nn.Module]):
        bbox_reg = nn.ModuleList()
        for channels, anchors in zip(in_channels, num_anchors):
            bbox_reg.append(_prediction_block(channels, 4 * anchors, 3, norm_layer))
        _normal_init(bbox_reg)
        super().__init__(bbox_reg, 4)


class SSDLiteFeatureExtractorMobileNet(nn.Module):
    """ssdlite.py SSDLiteFeatureExtractorMobileNet.  forward(x) -> OrderedDict "0" ... "5": the C4 expansion's output, the backbone's
    last map, then the four extra blocks' outputs."""

    def __init__(self, backbone: nn.Module, c4_pos: int, norm_layer: Callable[..., nn.Module], width_mult: float = 1.0,
                 min_depth: int = 16):
        super().__init__()

        if backbone[c4_pos].use_res_connect:
            raise ValueError("backbone[c4_pos].use_res_connect should be False")

        self.features = nn.Sequential(
            # As described in section 6.3 of MobileNetV3 paper
            nn.Sequential(*backbone[:c4_pos], backbone[c4_pos].block[0]),  # from start until C4 expansion layer
            nn.Sequential(backbone[c4_pos].block[1:], *backbone[c4_pos + 1:]),  # from C4 depthwise until end
        )

        get_depth = lambda d: max(min_depth, int(d * width_mult))  # noqa: E731
        extra = nn.ModuleList(
            [
                _extra_block(backbone[-1].out_channels, get_depth(512), norm_layer),
                _extra_block(get_depth(512), get_depth(256), norm_layer),
                _extra_block(get_depth(256), get_depth(256), norm_layer),
                _extra_block(get_depth(256), get_depth(128), norm_layer),
            ]
        )
        _normal_init(extra)

        self.extra = extra
        self.eval()

    def _module_out_channels(self) -> List[int]:
        """The channels of the six maps, read off the modules (ssd._retrieve_out_channels: the probing forward needs the MI355X)."""
        return [int(self.features[0][-1].out_channels), int(self.features[1][-1].out_channels)] + \
            [int(block[-1].out_channels) for block in self.extra]

    def forward(self, x: Tensor) -> Dict[str, Tensor]:
        if self.training:
            raise RuntimeError("the MI355X SSDLiteFeatureExtractorMobileNet is inference only: call .eval()")
        inp = x
        with torch.no_grad():
            # Get feature maps from backbone and extras
            output = []
            x = self.features[0](x)
            output.append(x)
            tail = list(self.features[1])
            x = _run_block(tail[0], x)  # the back half of the C4 block: depthwise 5x5, the gate, the projection (never a residual)
            for block in tail[1:]:
                x = block(x)
            output.append(x)

            for block in self.extra:
                x = _separable(block[0](x), block[1], block[2])
                output.append(x)
        deps = (inp, *self.parameters())
        return OrderedDict([(str(i), _lib.forward_only(v, "SSDLiteFeatureExtractorMobileNet.forward", *deps)) for i, v in enumerate(output)])


def _mobilenet_extractor(backbone: nn.Module, trainable_layers: int, norm_layer: Callable[..., nn.Module]):
    backbone = backbone.features
    # Gather the indices of blocks which are strided. These are the locations of C1, ..., Cn-1 blocks.
    # The first and last layer are always included because they are the C0 (conv1) and Cn.
    stage_indices = [0] + [i for i, b in enumerate(backbone) if getattr(b, "_is_cn", False)] + [len(backbone) - 1]
    num_stages = len(stage_indices)

    # find the index of the layer from which we won't freeze
    torch._assert(
        0 <= trainable_layers <= num_stages,
        f"trainable_layers should be in the range [0, {num_stages}]. Instead got {trainable_layers}",
    )
    freeze_before = len(backbone) if trainable_layers == 0 else stage_indices[num_stages - trainable_layers]

    for b in backbone[:freeze_before]:
        for parameter in b.parameters():
            parameter.requires_grad_(False)

    return SSDLiteFeatureExtractorMobileNet(backbone, stage_indices[-2], norm_layer)


def ssdlite320_mobilenet_v3_large(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                                  weights_backbone: Optional[Any] = None, trainable_backbone_layers: Optional[int] = None,
                                  norm_layer: Optional[Callable[..., nn.Module]] = None, **kwargs: Any) -> SSD:
    """ssdlite.py ssdlite320_mobilenet_v3_large: SSDlite at 320 x 320 on MobileNetV3-Large with the reduced tail (the whole MobileNetV3
    is constructed first, as the reference does, so a seeded construction draws from the RNG in the reference's order), 91 classes
    unless `num_classes` says otherwise.

    The package ships no weight files: `weights` and `weights_backbone` must be None; load a state dict of the reference's model
    with load_state_dict (the keys are the reference's)."""
    if weights is not None or weights_backbone is not None:
        raise ValueError("ssdlite320_mobilenet_v3_large: the package ships no weight files, weights and weights_backbone must be None; "
                         "load a state dict with load_state_dict")

    if "size" in kwargs:
        warnings.warn("The size of the model is already fixed; ignoring the parameter.")
        kwargs.pop("size")

    if num_classes is None:
        num_classes = 91

    trainable_backbone_layers = _validate_trainable_layers(False, trainable_backbone_layers, 6, 6)

    if norm_layer is None:
        norm_layer = partial(nn.BatchNorm2d, eps=0.001, momentum=0.03)

    # the reduced tail: no pretrained backbone is selected
    backbone = mobilenet_v3_large(norm_layer=norm_layer, reduced_tail=True)
    # Change the default initialization scheme if not pretrained
    _normal_init(backbone)
    backbone = _mobilenet_extractor(
        backbone,
        trainable_backbone_layers,
        norm_layer,
    )

    size = (320, 320)
    anchor_generator = DefaultBoxGenerator([[2, 3] for _ in range(6)], min_ratio=0.2, max_ratio=0.95)
    out_channels = _retrieve_out_channels(backbone, size)
    num_anchors = anchor_generator.num_anchors_per_location()
    if len(out_channels) != len(anchor_generator.aspect_ratios):
        raise ValueError(
            f"The length of the output channels from the backbone {len(out_channels)} do not match the length of the anchor generator aspect ratios {len(anchor_generator.aspect_ratios)}"
        )

    defaults = {
        "score_thresh": 0.001,
        "nms_thresh": 0.55,
        "detections_per_img": 300,
        "topk_candidates": 300,
        # Rescale the input in a way compatible to the backbone:
        # The following mean/std rescale the data from [0, 1] to [-1, 1]
        "image_mean": [0.5, 0.5, 0.5],
        "image_std": [0.5, 0.5, 0.5],
    }
    kwargs: Any = {**defaults, **kwargs}
    model = SSD(
        backbone,
        anchor_generator,
        size,
        num_classes,
        head=SSDLiteHead(out_channels, num_anchors, num_classes, norm_layer),
        **kwargs,
    )
    return model
