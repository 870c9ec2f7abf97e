"""RetinaNet inference on the MI355X kernels: models/detection/retinanet.py of the reference -- RetinaNetClassificationHead,
RetinaNetRegressionHead, RetinaNetHead, RetinaNet and the retinanet_resnet50_fpn builder -- with the same classes, constructor
arguments, defaults, argument errors, child names (backbone, anchor_generator, head.classification_head.conv.{i}.0 / cls_logits,
head.regression_head.conv.{i}.0 / bbox_reg, transform), state-dict keys (with the version-1 key renaming) and initialisation
order.  Only `forward` differs.

The heads keep their per-level NCHW maps: the reference permutes and concatenates every (anchor, class) logit into (N, HWA, K)
before it looks at one of them, F.retinanet_topk thresholds and selects on the maps where they lie, one (image, level) spread over
many workgroups, and F.retinanet_decode decodes the selected candidates only -- two calls for the whole batch and all levels, then
per image the boolean indexing by `valid`, ops.batched_nms and the slice.  `concat_layout` gives the reference's layout to anyone
who asks.

Each 3x3 conv (+ ReLU) of the towers is one F.conv2d_bias_relu launch.  The first layers of the two towers read the same
feature map: RetinaNetHead runs them as ONE launch over their concatenated (2 C, C, 3, 3) weight wherever that launch sums in the
order the two separate ones would (F.conv3x3_k_slices is the same for C and 2 C output channels), and passes the halves on as
channel slices.  Inference only, float32 only, norm_layer=None only (GroupNorm belongs to the v2 builder); there are no weight
files, as in faster_rcnn.py.
"""
from __future__ import annotations

import math
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
from .mobilenet import _ParameterCache, _tensor_versions, Conv2dNormActivation, FrozenBatchNorm2d
from .rpn import BoxCoder
from .transform import GeneralizedRCNNTransform

__all__ = ["RetinaNet", "RetinaNetHead", "RetinaNetClassificationHead", "RetinaNetRegressionHead", "retinanet_resnet50_fpn",
           "concat_layout"]


def _v1_to_v2_weights(state_dict, prefix):
    for i in range(4):
        for type in ["weight", "bias"]:
            old_key = f"{prefix}conv.{2*i}.{type}"
            new_key = f"{prefix}conv.{i}.0.{type}"
            if old_key in state_dict:
                state_dict[new_key] = state_dict.pop(old_key)


def _default_anchorgen():
    anchor_sizes = tuple((x, int(x * 2 ** (1.0 / 3)), int(x * 2 ** (2.0 / 3))) for x in [32, 64, 128, 256, 512])
    aspect_ratios = ((0.5, 1.0, 2.0),) * len(anchor_sizes)
    anchor_generator = AnchorGenerator(anchor_sizes, aspect_ratios)
    return anchor_generator


def concat_layout(maps: List[Tensor], last: int) -> Tensor:
    """The reference's layout of a head's per-level NCHW maps (N, A * last, H, W): view(N, -1, last, H, W).permute(0, 3, 4, 1, 2)
    .reshape(N, -1, last) per level, concatenated -> (N, sum HWA, last), as torch compositions (RetinaNet itself never builds it)."""
    out = []
    for m in maps:
        N, _, H, W = m.shape
        m = m.contiguous().view(N, -1, last, H, W)
        m = m.permute(0, 3, 4, 1, 2)
        out.append(m.reshape(N, -1, last))  # Size=(N, HWA, last)
    return torch.cat(out, dim=1)


def _no_norm(norm_layer, name):
    if norm_layer is not None:
        raise NotImplementedError(f"the MI355X {name} is built with norm_layer=None only (GroupNorm heads belong to retinanet_resnet50_fpn_v2)")


def _tower(conv: nn.Sequential, t: Tensor, first: Optional[Tensor] = None) -> Tensor:
    """The four conv + ReLU blocks, one launch each; `first`: the output of block 0, already computed."""
    for i, block in enumerate(conv):
        t = first if i == 0 and first is not None else F.conv2d_bias_relu(t, block[0].weight, block[0].bias, relu=True)
    return t


class RetinaNetClassificationHead(nn.Module):
    """retinanet.py:63-170.  forward(x: List[Tensor]) -> per level the NCHW map (N, A * K, H, W) of cls_logits (channel a K + c)."""

    _version = 2

    def __init__(self, in_channels, num_anchors, num_classes, prior_probability=0.01,
                 norm_layer: Optional[Callable[..., nn.Module]] = None):
        super().__init__()
        _no_norm(norm_layer, "RetinaNetClassificationHead")

        conv = []
        for _ in range(4):
            conv.append(Conv2dNormActivation(in_channels, in_channels, norm_layer=norm_layer))
        self.conv = nn.Sequential(*conv)

        for layer in self.conv.modules():
            if isinstance(layer, nn.Conv2d):
                torch.nn.init.normal_(layer.weight, std=0.01)
                if layer.bias is not None:
                    torch.nn.init.constant_(layer.bias, 0)

        self.cls_logits = nn.Conv2d(in_channels, num_anchors * num_classes, kernel_size=3, stride=1, padding=1)
        torch.nn.init.normal_(self.cls_logits.weight, std=0.01)
        torch.nn.init.constant_(self.cls_logits.bias, -math.log((1 - prior_probability) / prior_probability))

        self.num_classes = num_classes
        self.num_anchors = num_anchors
        self.eval()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)

        if version is None or version < 2:
            _v1_to_v2_weights(state_dict, prefix)

        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def level(self, x: Tensor, first: Optional[Tensor] = None) -> Tensor:
        t = _tower(self.conv, x, first)
        return F.conv2d_bias_relu(t, self.cls_logits.weight, self.cls_logits.bias, relu=False)

    def forward(self, x: List[Tensor]) -> List[Tensor]:
        if self.training:
            raise RuntimeError("the MI355X RetinaNetClassificationHead is inference only: call .eval()")
        with torch.no_grad():
            out = [self.level(features) for features in x]
        return [_lib.forward_only(v, "RetinaNetClassificationHead.forward", *x, *self.parameters()) for v in out]


class RetinaNetRegressionHead(nn.Module):
    """retinanet.py:173-288.  forward(x: List[Tensor]) -> per level the NCHW map (N, 4 A, H, W) of bbox_reg (channel 4 a + q)."""

    _version = 2

    __annotations__ = {
        "box_coder": BoxCoder,
    }

    def __init__(self, in_channels, num_anchors, norm_layer: Optional[Callable[..., nn.Module]] = None):
        super().__init__()
        _no_norm(norm_layer, "RetinaNetRegressionHead")

        conv = []
        for _ in range(4):
            conv.append(Conv2dNormActivation(in_channels, in_channels, norm_layer=norm_layer))
        self.conv = nn.Sequential(*conv)

        self.bbox_reg = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=3, stride=1, padding=1)
        torch.nn.init.normal_(self.bbox_reg.weight, std=0.01)
        torch.nn.init.zeros_(self.bbox_reg.bias)

        for layer in self.conv.modules():
            if isinstance(layer, nn.Conv2d):
                torch.nn.init.normal_(layer.weight, std=0.01)
                if layer.bias is not None:
                    torch.nn.init.zeros_(layer.bias)

        self.box_coder = BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
        self._loss_type = "l1"
        self.eval()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)

        if version is None or version < 2:
            _v1_to_v2_weights(state_dict, prefix)

        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def level(self, x: Tensor, first: Optional[Tensor] = None) -> Tensor:
        t = _tower(self.conv, x, first)
        return F.conv2d_bias_relu(t, self.bbox_reg.weight, self.bbox_reg.bias, relu=False)

    def forward(self, x: List[Tensor]) -> List[Tensor]:
        if self.training:
            raise RuntimeError("the MI355X RetinaNetRegressionHead is inference only: call .eval()")
        with torch.no_grad():
            out = [self.level(features) for features in x]
        return [_lib.forward_only(v, "RetinaNetRegressionHead.forward", *x, *self.parameters()) for v in out]


class RetinaNetHead(nn.Module):
    """retinanet.py:34-60.  forward(x: List[Tensor]) -> {"cls_logits": [...], "bbox_regression": [...]}: the per-level NCHW maps
    (N, A K, H, W) and (N, 4 A, H, W) the kernels read; concat_layout(maps, K) / concat_layout(maps, 4) give the reference's
    (N, sum HWA, K) / (N, sum HWA, 4)."""

    def __init__(self, in_channels, num_anchors, num_classes, norm_layer: Optional[Callable[..., nn.Module]] = None):
        super().__init__()
        self.classification_head = RetinaNetClassificationHead(in_channels, num_anchors, num_classes, norm_layer=norm_layer)
        self.regression_head = RetinaNetRegressionHead(in_channels, num_anchors, norm_layer=norm_layer)
        self._joint = _ParameterCache()
        self.eval()

    def joint_first_layer(self, device) -> Tuple[Tensor, Tensor]:
        """(weight (2 C, C, 3, 3), bias (2 C)) of the two towers' first convs as one conv on `device`, rebuilt when a parameter
        changes (the cache of RPNHead.joint_pointwise)."""
        c, r = self.classification_head.conv[0][0], self.regression_head.conv[0][0]
        key = _tensor_versions(c.weight, c.bias, r.weight, r.bias) + (str(device),)

        def joint():
            with torch.no_grad():
                return (torch.cat([c.weight, r.weight]).to(device, torch.float32).contiguous(),
                        torch.cat([c.bias, r.bias]).to(device, torch.float32).contiguous())
        return self._joint.lookup(key, joint)

    @staticmethod
    def joint_sums_alike(x: Tensor) -> bool:
        """Whether one launch with 2 C output channels sums as the launches with C do (host logic): always when the summation is
        batch invariant (one chain per output), else when the K slices of the two shapes agree."""
        if _lib.switch("BATCH_INVARIANT_SUMMATION"):
            return True
        n, c, h, w = (int(d) for d in x.shape)
        return F.conv3x3_k_slices(n, c, h, w, 2 * c) == F.conv3x3_k_slices(n, c, h, w, c)

    def forward(self, x: List[Tensor]) -> Dict[str, List[Tensor]]:
        if self.training:
            raise RuntimeError("the MI355X RetinaNetHead is inference only: call .eval()")
        cls, reg = [], []
        with torch.no_grad():
            for features in x:
                first_c = first_r = None
                if self.joint_sums_alike(features):
                    w, b = self.joint_first_layer(features.device)
                    both = F.conv2d_bias_relu(features, w, b, relu=True)
                    c = w.shape[1]
                    first_c, first_r = both[:, :c], both[:, c:]
                cls.append(self.classification_head.level(features, first_c))
                reg.append(self.regression_head.level(features, first_r))
        deps = (*x, *self.parameters())
        return {"cls_logits": [_lib.forward_only(v, "RetinaNetHead.forward", *deps) for v in cls],
                "bbox_regression": [_lib.forward_only(v, "RetinaNetHead.forward", *deps) for v in reg]}


class RetinaNet(OneStageDetector):
    """retinanet.py:291-669.  forward(images: List[Tensor (C, H, W) float32 in 0..1]) -> List[{boxes (N, 4) as (x1, y1, x2, y2),
    scores (N,), labels (N,) int64}], the boxes in the coordinates of the images as given.  The images may have any sizes: the
    transform resizes them to min_size / max_size (transform.py).  `**kwargs` go to GeneralizedRCNNTransform (`_skip_resize=True`
    for images that already have their final size).  The
    matcher and the losses of the reference are training-only and not built; `proposal_matcher` is kept as given."""

    __annotations__ = {
        "box_coder": BoxCoder,
    }
    _name = "RetinaNet"

    def __init__(self, backbone, num_classes,
                 # transform parameters
                 min_size=800, max_size=1333, image_mean=None, image_std=None,
                 # Anchor parameters
                 anchor_generator=None, head=None, proposal_matcher=None, score_thresh=0.05, nms_thresh=0.5, detections_per_img=300,
                 fg_iou_thresh=0.5, bg_iou_thresh=0.4, topk_candidates=1000, **kwargs):
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
            raise ValueError(f"the MI355X RetinaNet selects up to {F.MAX_RPN_TOPK} candidates per level, got topk_candidates={topk_candidates}")

        if anchor_generator is None:
            anchor_generator = _default_anchorgen()
        self.anchor_generator = anchor_generator

        if head is None:
            head = RetinaNetHead(backbone.out_channels, anchor_generator.num_anchors_per_location()[0], num_classes)
        self.head = head

        self.proposal_matcher = proposal_matcher  # training only: there is no Matcher in the library
        self.fg_iou_thresh, self.bg_iou_thresh = fg_iou_thresh, bg_iou_thresh

        self.box_coder = BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))

        if image_mean is None:
            image_mean = [0.485, 0.456, 0.406]
        if image_std is None:
            image_std = [0.229, 0.224, 0.225]
        self.transform = GeneralizedRCNNTransform(min_size, max_size, image_mean, image_std, **kwargs)

        self.score_thresh = score_thresh
        self.nms_thresh = nms_thresh
        self.detections_per_img = detections_per_img
        self.topk_candidates = topk_candidates

        # used only on torchscript mode
        self._has_warned = False
        self.eval()

    def candidates(self, head_outputs: Dict[str, List[Tensor]], padded_size, image_shapes) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
        """postprocess_detections up to the nms for the whole batch and all levels, two calls: (idx, boxes, scores, labels, valid)."""
        cls, reg = head_outputs["cls_logits"], head_outputs["bbox_regression"]
        cell_anchors = self.anchor_generator.cell_anchors
        strides = pyramid_strides(cell_anchors, cls, padded_size)
        num_classes = int(cls[0].shape[1]) // int(cell_anchors[0].shape[0])
        idx = F.retinanet_topk(cls, num_classes, self.topk_candidates, self.score_thresh)
        boxes, scores, labels, valid = F.retinanet_decode(cls, reg, idx, cell_anchors, strides, image_shapes, num_classes,
                                                          self.box_coder.weights, self.box_coder.bbox_xform_clip)
        return idx, boxes, scores, labels, valid

    def postprocess_detections(self, head_outputs: Dict[str, List[Tensor]], padded_size, image_shapes) -> List[Dict[str, Tensor]]:
        """retinanet.py:494-560 on the head's per-level NCHW maps: `candidates`, then per image the boolean indexing by `valid` (the
        one read-back besides the nms's count), ops.batched_nms over the labels and the slice."""
        return self._nms_tail(*self.candidates(head_outputs, padded_size, image_shapes)[1:])

    def _detect(self, head_outputs, features, images):
        return self.postprocess_detections(head_outputs, images.tensors.shape[-2:], images.image_sizes)


def retinanet_resnet50_fpn(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                           weights_backbone: Optional[Any] = None, trainable_backbone_layers: Optional[int] = None,
                           **kwargs: Any) -> RetinaNet:
    """retinanet.py:729-826: RetinaNet with a ResNet-50-FPN backbone on layer2 .. layer4 plus P6 and P7 (FrozenBatchNorm2d folded
    into the convs), 91 classes unless `num_classes` says otherwise.

    The package ships no weight files: `weights` and `weights_backbone` must be None; load a state dict of the reference's model
    with load_state_dict (the keys are the reference's)."""
    if weights is not None or weights_backbone is not None:
        raise ValueError("retinanet_resnet50_fpn: the package ships no weight files, weights and weights_backbone must be None; "
                         "load a state dict with load_state_dict")
    if num_classes is None:
        num_classes = 91

    is_trained = False
    trainable_backbone_layers = _validate_trainable_layers(is_trained, trainable_backbone_layers, 5, 3)

    backbone = resnet.resnet50(norm_layer=FrozenBatchNorm2d)
    # skip P2 because it generates too many anchors (according to their paper)
    backbone = _resnet_fpn_extractor(backbone, trainable_backbone_layers, returned_layers=[2, 3, 4], extra_blocks=LastLevelP6P7(256, 256))
    anchor_generator = _default_anchorgen()
    model = RetinaNet(backbone, num_classes, anchor_generator=anchor_generator, **kwargs)
    return model
