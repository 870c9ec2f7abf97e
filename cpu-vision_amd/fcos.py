"""FCOS inference on the MI355X kernels: models/detection/fcos.py of the reference -- FCOSClassificationHead, FCOSRegressionHead,
FCOSHead, FCOS and the fcos_resnet50_fpn builder -- with the same classes, constructor arguments, defaults, argument errors, child
names (backbone, anchor_generator, head.classification_head.conv.{3 i} / conv.{3 i + 1} / cls_logits, head.regression_head.conv.{..} /
bbox_reg / bbox_ctrness, transform), state-dict keys and initialisation order.  Only `forward` differs.

Every tower block `Conv2d 3x3 -> GroupNorm -> ReLU` is one F.conv2d_bias_relu(relu=False) launch and one F.group_norm_act(relu=True)
call (two launches: the groups' float64 sums, then the normalisation with the ReLU).  The heads keep their per-level NCHW maps, as
RetinaNet's do here: F.fcos_topk thresholds sqrt(sigmoid(cls) * sigmoid(centerness)) and selects on the maps where they lie, and
F.fcos_decode decodes the selected candidates only with BoxLinearCoder's linear decode -- two calls for the whole batch and all
levels, then per image the boolean indexing by `valid`, ops.batched_nms and the slice.  retinanet.concat_layout gives the reference's
(N, sum HW, last) layout of any of the three maps to anyone who asks.

Inference only, float32 only; norm_layer may be nn.GroupNorm with any group count (with or without affine).  The training half of the
reference (center sampling, the matcher, the gIoU and centerness losses, BoxLinearCoder.encode) is not built; there are no weight
files, as in retinanet.py.
"""
from __future__ import annotations

import math
from functools import partial
from typing import Any, Callable, Dict, List, Optional, Tuple

import torch
from torch import nn, Tensor

from . import _lib
from . import functional as F
from . import resnet
from ._one_stage import OneStageDetector, pyramid_strides
from .anchor_utils import AnchorGenerator
from .backbone_utils import _resnet_fpn_extractor, _validate_trainable_layers
from .fpn import LastLevelP6P7
from .mobilenet import FrozenBatchNorm2d
from .transform import GeneralizedRCNNTransform

__all__ = ["FCOS", "FCOSHead", "FCOSClassificationHead", "FCOSRegressionHead", "BoxLinearCoder", "fcos_resnet50_fpn"]


class BoxLinearCoder:
    """_utils.py BoxLinearCoder, the decode half (F.fcos_decode computes it for normalize_by_size=True; `encode` is training only)."""

    def __init__(self, normalize_by_size: bool = True) -> None:
        self.normalize_by_size = normalize_by_size


def _tower_blocks(in_channels: int, num_convs: int, norm_layer, name: str) -> nn.Sequential:
    """The reference's flat Sequential [Conv2d 3x3, norm_layer(C), ReLU] * num_convs; anything but nn.GroupNorm is not built."""
    conv = []
    for _ in range(num_convs):
        conv.append(nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1))
        norm = norm_layer(in_channels)
        if not isinstance(norm, nn.GroupNorm):
            raise NotImplementedError(f"the MI355X {name} is built with nn.GroupNorm towers only, norm_layer made {type(norm).__name__}")
        conv.append(norm)
        conv.append(nn.ReLU())
    return nn.Sequential(*conv)


def _tower(conv: nn.Sequential, t: Tensor) -> Tensor:
    """The conv + GroupNorm + ReLU blocks: per block one conv launch, then the norm with the ReLU (two launches)."""
    layers = list(conv)
    for i in range(0, len(layers), 3):
        c, norm = layers[i], layers[i + 1]
        t = F.conv2d_bias_relu(t, c.weight, c.bias, relu=False)
        t = F.group_norm_act(t, norm.num_groups, norm.weight, norm.bias, norm.eps, relu=True)
    return t


class FCOSClassificationHead(nn.Module):
    """fcos.py FCOSClassificationHead.  forward(x: List[Tensor]) -> per level the NCHW map (N, A * K, H, W) of cls_logits."""

    def __init__(self, in_channels: int, num_anchors: int, num_classes: int, num_convs: int = 4, prior_probability: float = 0.01,
                 norm_layer: Optional[Callable[..., nn.Module]] = None) -> None:
        super().__init__()

        self.num_classes = num_classes
        self.num_anchors = num_anchors

        if norm_layer is None:
            norm_layer = partial(nn.GroupNorm, 32)

        self.conv = _tower_blocks(in_channels, num_convs, norm_layer, "FCOSClassificationHead")

        for layer in self.conv.children():
            if isinstance(layer, nn.Conv2d):
                torch.nn.init.normal_(layer.weight, std=0.01)
                torch.nn.init.constant_(layer.bias, 0)

        self.cls_logits = nn.Conv2d(in_channels, num_anchors * num_classes, kernel_size=3, stride=1, padding=1)
        torch.nn.init.normal_(self.cls_logits.weight, std=0.01)
        torch.nn.init.constant_(self.cls_logits.bias, -math.log((1 - prior_probability) / prior_probability))
        self.eval()

    def level(self, x: Tensor) -> Tensor:
        t = _tower(self.conv, x)
        return F.conv2d_bias_relu(t, self.cls_logits.weight, self.cls_logits.bias, relu=False)

    def forward(self, x: List[Tensor]) -> List[Tensor]:
        if self.training:
            raise RuntimeError("the MI355X FCOSClassificationHead is inference only: call .eval()")
        with torch.no_grad():
            out = [self.level(features) for features in x]
        return [_lib.forward_only(v, "FCOSClassificationHead.forward", *x, *self.parameters()) for v in out]


class FCOSRegressionHead(nn.Module):
    """fcos.py FCOSRegressionHead.  forward(x: List[Tensor]) -> (per level relu(bbox_reg) (N, 4 A, H, W), per level bbox_ctrness
    (N, A, H, W)); the ReLU is the conv launch's own."""

    def __init__(self, in_channels: int, num_anchors: int, num_convs: int = 4,
                 norm_layer: Optional[Callable[..., nn.Module]] = None):
        super().__init__()

        if norm_layer is None:
            norm_layer = partial(nn.GroupNorm, 32)

        self.conv = _tower_blocks(in_channels, num_convs, norm_layer, "FCOSRegressionHead")

        self.bbox_reg = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=3, stride=1, padding=1)
        self.bbox_ctrness = nn.Conv2d(in_channels, num_anchors * 1, kernel_size=3, stride=1, padding=1)
        for layer in [self.bbox_reg, self.bbox_ctrness]:
            torch.nn.init.normal_(layer.weight, std=0.01)
            torch.nn.init.zeros_(layer.bias)

        for layer in self.conv.children():
            if isinstance(layer, nn.Conv2d):
                torch.nn.init.normal_(layer.weight, std=0.01)
                torch.nn.init.zeros_(layer.bias)
        self.eval()

    def level(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        t = _tower(self.conv, x)
        return (F.conv2d_bias_relu(t, self.bbox_reg.weight, self.bbox_reg.bias, relu=True),
                F.conv2d_bias_relu(t, self.bbox_ctrness.weight, self.bbox_ctrness.bias, relu=False))

    def forward(self, x: List[Tensor]) -> Tuple[List[Tensor], List[Tensor]]:
        if self.training:
            raise RuntimeError("the MI355X FCOSRegressionHead is inference only: call .eval()")
        with torch.no_grad():
            out = [self.level(features) for features in x]
        deps = (*x, *self.parameters())
        return ([_lib.forward_only(r, "FCOSRegressionHead.forward", *deps) for r, _ in out],
                [_lib.forward_only(c, "FCOSRegressionHead.forward", *deps) for _, c in out])


class FCOSHead(nn.Module):
    """fcos.py FCOSHead.  forward(x: List[Tensor]) -> {"cls_logits", "bbox_regression", "bbox_ctrness"}: the per-level NCHW maps
    (N, A K, H, W), (N, 4 A, H, W) and (N, A, H, W) the kernels read; retinanet.concat_layout(maps, K / 4 / 1) gives the reference's."""

    __annotations__ = {
        "box_coder": BoxLinearCoder,
    }

    def __init__(self, in_channels: int, num_anchors: int, num_classes: int, num_convs: Optional[int] = 4) -> None:
        super().__init__()
        self.box_coder = BoxLinearCoder(normalize_by_size=True)
        self.classification_head = FCOSClassificationHead(in_channels, num_anchors, num_classes, num_convs)
        self.regression_head = FCOSRegressionHead(in_channels, num_anchors, num_convs)
        self.eval()

    def forward(self, x: List[Tensor]) -> Dict[str, List[Tensor]]:
        if self.training:
            raise RuntimeError("the MI355X FCOSHead is inference only: call .eval()")
        cls_logits = self.classification_head(x)
        bbox_regression, bbox_ctrness = self.regression_head(x)
        return {"cls_logits": cls_logits, "bbox_regression": bbox_regression, "bbox_ctrness": bbox_ctrness}


class FCOS(OneStageDetector):
    """fcos.py FCOS.  forward(images: List[Tensor (C, H, W) float32 in 0..1]) -> List[{boxes (N, 4) as (x1, y1, x2, y2), scores (N,),
    labels (N,) int64}], the boxes in the coordinates of the images as given.  `**kwargs` go to GeneralizedRCNNTransform.
    center_sampling_radius is the training half's and only kept."""

    __annotations__ = {
        "box_coder": BoxLinearCoder,
    }
    _name = "FCOS"

    def __init__(self, backbone: nn.Module, num_classes: int,
                 # transform parameters
                 min_size: int = 800, max_size: int = 1333, image_mean: Optional[List[float]] = None, image_std: Optional[List[float]] = None,
                 # Anchor parameters
                 anchor_generator: Optional[AnchorGenerator] = None, head: Optional[nn.Module] = None, center_sampling_radius: float = 1.5,
                 score_thresh: float = 0.2, nms_thresh: float = 0.6, detections_per_img: int = 100, topk_candidates: int = 1000, **kwargs):
        super().__init__()

        if not hasattr(backbone, "out_channels"):
            raise ValueError(
                "backbone should contain an attribute out_channels "
                "specifying the number of output channels (assumed to be the "
                "same for all the levels)"
            )
        self.backbone = backbone

        if not isinstance(anchor_generator, (AnchorGenerator, type(None))):
            raise TypeError(f"anchor_generator should be of type AnchorGenerator or None instead of {type(anchor_generator)}")
        if topk_candidates > F.MAX_RPN_TOPK:
            raise ValueError(f"the MI355X FCOS selects up to {F.MAX_RPN_TOPK} candidates per level, got topk_candidates={topk_candidates}")

        if anchor_generator is None:
            anchor_sizes = ((8,), (16,), (32,), (64,), (128,))  # equal to strides of multi-level feature map
            aspect_ratios = ((1.0,),) * len(anchor_sizes)  # set only one anchor
            anchor_generator = AnchorGenerator(anchor_sizes, aspect_ratios)
        self.anchor_generator = anchor_generator
        if self.anchor_generator.num_anchors_per_location()[0] != 1:
            raise ValueError(
                f"anchor_generator.num_anchors_per_location()[0] should be 1 instead of {anchor_generator.num_anchors_per_location()[0]}"
            )

        if head is None:
            head = FCOSHead(backbone.out_channels, anchor_generator.num_anchors_per_location()[0], num_classes)
        self.head = head

        self.box_coder = BoxLinearCoder(normalize_by_size=True)

        if image_mean is None:
            image_mean = [0.485, 0.456, 0.406]
        if image_std is None:
            image_std = [0.229, 0.224, 0.225]
        self.transform = GeneralizedRCNNTransform(min_size, max_size, image_mean, image_std, **kwargs)

        self.center_sampling_radius = center_sampling_radius
        self.score_thresh = score_thresh
        self.nms_thresh = nms_thresh
        self.detections_per_img = detections_per_img
        self.topk_candidates = topk_candidates

        # used only on torchscript mode
        self._has_warned = False
        self.eval()

    def candidates(self, head_outputs: Dict[str, List[Tensor]], padded_size, image_shapes) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
        """postprocess_detections up to the nms for the whole batch and all levels, two calls: (idx, boxes, scores, labels, valid)."""
        cls, reg, ctr = head_outputs["cls_logits"], head_outputs["bbox_regression"], head_outputs["bbox_ctrness"]
        cell_anchors = self.anchor_generator.cell_anchors
        strides = pyramid_strides(cell_anchors, cls, padded_size)
        num_classes = int(cls[0].shape[1])
        idx = F.fcos_topk(cls, ctr, num_classes, self.topk_candidates, self.score_thresh)
        boxes, scores, labels, valid = F.fcos_decode(cls, ctr, reg, idx, cell_anchors, strides, image_shapes, num_classes)
        return idx, boxes, scores, labels, valid

    def postprocess_detections(self, head_outputs: Dict[str, List[Tensor]], padded_size, image_shapes) -> List[Dict[str, Tensor]]:
        """fcos.py postprocess_detections on the head's per-level NCHW maps: `candidates`, then per image the boolean indexing by
        `valid`, ops.batched_nms over the labels and the slice."""
        return self._nms_tail(*self.candidates(head_outputs, padded_size, image_shapes)[1:])

    def _detect(self, head_outputs, features, images):
        return self.postprocess_detections(head_outputs, images.tensors.shape[-2:], images.image_sizes)


def fcos_resnet50_fpn(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                      weights_backbone: Optional[Any] = None, trainable_backbone_layers: Optional[int] = None, **kwargs: Any) -> FCOS:
    """fcos.py fcos_resnet50_fpn: FCOS with a ResNet-50-FPN backbone on layer2 .. layer4 plus P6 and P7 made from P5
    (FrozenBatchNorm2d folded into the convs), 91 classes unless `num_classes` says otherwise.

    The package ships no weight files: `weights` and `weights_backbone` must be None; load a state dict of the reference's model
    with load_state_dict (the keys are the reference's)."""
    if weights is not None or weights_backbone is not None:
        raise ValueError("fcos_resnet50_fpn: the package ships no weight files, weights and weights_backbone must be None; "
                         "load a state dict with load_state_dict")
    if num_classes is None:
        num_classes = 91

    is_trained = False
    trainable_backbone_layers = _validate_trainable_layers(is_trained, trainable_backbone_layers, 5, 3)

    backbone = resnet.resnet50(norm_layer=FrozenBatchNorm2d)
    backbone = _resnet_fpn_extractor(backbone, trainable_backbone_layers, returned_layers=[2, 3, 4], extra_blocks=LastLevelP6P7(256, 256))
    model = FCOS(backbone, num_classes, **kwargs)
    return model
