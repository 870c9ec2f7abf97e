"""References for the SSDlite tests (a helper module, not a test file and not a conftest).  Imports nothing from the package.

A plain-torch replica of the reference's models/detection/ssdlite.py (torchvision is not importable in the test environment) on top of
tests/_ssd_ref.py (SSD, SSDScoringHead, DefaultBoxGenerator, retrieve_out_channels and the restated post-processing) and
tests/_mobilenetv3_ref.py (the MobileNetV3 replica): the same constructor arguments, child names, construction order and
initialisation, plain nn.Conv2d / nn.BatchNorm2d, and torch's own forward, which runs on the CPU.
"""
import warnings
from collections import OrderedDict
from functools import partial

import torch
from torch import nn

from tests import _mobilenetv3_ref as MR
from tests import _ssd_ref as R
from tests._mobilenetv3_ref import TConv2dNormActivation


def _prediction_block(in_channels, out_channels, kernel_size, norm_layer):
    return nn.Sequential(
        TConv2dNormActivation(in_channels, in_channels, kernel_size=kernel_size, groups=in_channels, norm_layer=norm_layer,
                              activation_layer=nn.ReLU6),
        nn.Conv2d(in_channels, out_channels, 1),
    )


def _extra_block(in_channels, out_channels, norm_layer):
    activation = nn.ReLU6
    intermediate_channels = out_channels // 2
    return nn.Sequential(
        TConv2dNormActivation(in_channels, intermediate_channels, kernel_size=1, norm_layer=norm_layer, activation_layer=activation),
        TConv2dNormActivation(intermediate_channels, intermediate_channels, kernel_size=3, stride=2, groups=intermediate_channels,
                              norm_layer=norm_layer, activation_layer=activation),
        TConv2dNormActivation(intermediate_channels, out_channels, kernel_size=1, norm_layer=norm_layer, activation_layer=activation),
    )


def _normal_init(conv):
    for layer in conv.modules():
        if isinstance(layer, nn.Conv2d):
            torch.nn.init.normal_(layer.weight, mean=0.0, std=0.03)
            if layer.bias is not None:
                torch.nn.init.constant_(layer.bias, 0.0)


class SSDLiteClassificationHead(R.SSDScoringHead):
    def __init__(self, in_channels, num_anchors, num_classes, norm_layer):
        cls_logits = nn.ModuleList()
        for channels, anchors in zip(in_channels, num_anchors):
            cls_logits.append(_prediction_block(channels, num_classes * anchors, 3, norm_layer))
        _normal_init(cls_logits)
        super().__init__(cls_logits, num_classes)


class SSDLiteRegressionHead(R.SSDScoringHead):
    def __init__(self, in_channels, num_anchors, norm_layer):
        bbox_reg = nn.ModuleList()
        for channels, anchors in zip(in_channels, num_anchors):
            bbox_reg.append(_prediction_block(channels, 4 * anchors, 3, norm_layer))
        _normal_init(bbox_reg)
        super().__init__(bbox_reg, 4)


class SSDLiteHead(nn.Module):
    def __init__(self, in_channels, num_anchors, num_classes, norm_layer):
        super().__init__()
        self.classification_head = SSDLiteClassificationHead(in_channels, num_anchors, num_classes, norm_layer)
        self.regression_head = SSDLiteRegressionHead(in_channels, num_anchors, norm_layer)

    def forward(self, x):
        return {"bbox_regression": self.regression_head(x), "cls_logits": self.classification_head(x)}


class SSDLiteFeatureExtractorMobileNet(nn.Module):
    def __init__(self, backbone, c4_pos, norm_layer, width_mult=1.0, min_depth=16):
        super().__init__()
        if backbone[c4_pos].use_res_connect:
            raise ValueError("backbone[c4_pos].use_res_connect should be False")
        self.features = nn.Sequential(
            nn.Sequential(*backbone[:c4_pos], backbone[c4_pos].block[0]),
            nn.Sequential(backbone[c4_pos].block[1:], *backbone[c4_pos + 1:]),
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

    def forward(self, x):
        output = []
        for block in self.features:
            x = block(x)
            output.append(x)
        for block in self.extra:
            x = block(x)
            output.append(x)
        return OrderedDict([(str(i), v) for i, v in enumerate(output)])


def _mobilenet_extractor(backbone, trainable_layers, norm_layer):
    backbone = backbone.features
    stage_indices = [0] + [i for i, b in enumerate(backbone) if getattr(b, "_is_cn", False)] + [len(backbone) - 1]
    num_stages = len(stage_indices)
    if not 0 <= trainable_layers <= num_stages:
        raise ValueError(f"trainable_layers should be in the range [0, {num_stages}], instead got {trainable_layers}")
    freeze_before = len(backbone) if trainable_layers == 0 else stage_indices[num_stages - trainable_layers]
    for b in backbone[:freeze_before]:
        for parameter in b.parameters():
            parameter.requires_grad_(False)
    return SSDLiteFeatureExtractorMobileNet(backbone, stage_indices[-2], norm_layer)


def default_norm_layer():
    return partial(nn.BatchNorm2d, eps=0.001, momentum=0.03)


def mobilenet_v3_large(width_mult=1.0, momentum=0.03):
    """The MobileNetV3-Large replica with the reduced tail; its norms get the momentum SSDlite's norm_layer sets (the replica's
    constructor fixes eps = 0.001, which is SSDlite's too; neither enters a state dict or an eval-mode forward)."""
    m = MR.replica("mobilenet_v3_large", width_mult=width_mult, reduced_tail=True)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.momentum = momentum
    return m


def ssdlite_generator():
    return R.DefaultBoxGenerator([[2, 3] for _ in range(6)], min_ratio=0.2, max_ratio=0.95)


def ssdlite320_mobilenet_v3_large(*, weights=None, progress=True, num_classes=None, weights_backbone=None, trainable_backbone_layers=None,
                                  norm_layer=None, **kwargs):
    if "size" in kwargs:
        warnings.warn("The size of the model is already fixed; ignoring the parameter.")
        kwargs.pop("size")
    if num_classes is None:
        num_classes = 91
    trainable_backbone_layers = 6  # _validate_trainable_layers without weights
    if norm_layer is None:
        norm_layer = default_norm_layer()
    backbone = mobilenet_v3_large()
    _normal_init(backbone)
    backbone = _mobilenet_extractor(backbone, trainable_backbone_layers, norm_layer)
    size = (320, 320)
    anchor_generator = ssdlite_generator()
    out_channels = R.retrieve_out_channels(backbone, size)
    num_anchors = anchor_generator.num_anchors_per_location()
    if len(out_channels) != len(anchor_generator.aspect_ratios):
        raise ValueError(
            f"The length of the output channels from the backbone {len(out_channels)} do not match the length of the anchor generator aspect ratios {len(anchor_generator.aspect_ratios)}"
        )
    defaults = {"score_thresh": 0.001, "nms_thresh": 0.55, "detections_per_img": 300, "topk_candidates": 300,
                "image_mean": [0.5, 0.5, 0.5], "image_std": [0.5, 0.5, 0.5]}
    kwargs = {**defaults, **kwargs}
    return R.SSD(backbone, anchor_generator, size, num_classes, head=SSDLiteHead(out_channels, num_anchors, num_classes, norm_layer), **kwargs)
