"""RegionProposalNetwork inference on the MI355X kernels: head -> top-k on the head's own NCHW maps -> decode of the selected
candidates only -> nms.

Mirrors models/detection/rpn.py and _utils.py::BoxCoder of the reference the way fpn.py mirrors ops/feature_pyramid_network.py:
same classes, constructor arguments, child names (head.conv.0.0, head.cls_logits, head.bbox_pred), state-dict keys (with the
version-1 key renaming) and initialisation order.  Only `forward` differs.  The reference materialises every anchor of every
level, permutes and concatenates every logit and delta, decodes every anchor and then takes the top k per level and gathers;
here F.rpn_topk selects per (image, level) first and F.rpn_decode builds the anchor of each selected candidate in registers,
decodes, clips, applies the sigmoid and flags the valid ones -- two launches after the head, whatever the number of levels.

RPNHead: each 3x3 conv + ReLU is one launch (the MFMA 3x3 of F.conv2d_bias_relu); cls_logits and bbox_pred run as ONE pointwise
F.conv_norm_act over their concatenated weight (5 A output channels, the hidden map read once) and come back as channel slices of
that tensor: conv_depth + 1 launches per level.

Numerics: every float operation of decode_single, the clipping and the sigmoid is the reference's float32 operation, rounded once;
exp is the correctly rounded float32 exp where torch's CPU exp is a 1-ulp routine.  Inference only, float32 only.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn, Tensor

from . import _lib
from . import functional as F
from . import ops as box_ops
from .anchor_utils import AnchorGenerator
from .image_list import ImageList
from .mobilenet import _ParameterCache, _tensor_versions, Conv2dNormActivation

__all__ = ["BoxCoder", "RPNHead", "RegionProposalNetwork", "concat_box_prediction_layers", "permute_and_flatten"]


class BoxCoder:
    """_utils.py:127-233, the decoding half: `encode` / `encode_single` are training-only and not here."""

    def __init__(self, weights: Tuple[float, float, float, float], bbox_xform_clip: float = math.log(1000.0 / 16)) -> None:
        self.weights = weights
        self.bbox_xform_clip = bbox_xform_clip

    def decode(self, rel_codes: Tensor, boxes: List[Tensor]) -> Tensor:
        torch._assert(isinstance(boxes, (list, tuple)), "This function expects boxes of type list or tuple.")
        torch._assert(isinstance(rel_codes, torch.Tensor), "This function expects rel_codes of type torch.Tensor.")
        boxes_per_image = [b.size(0) for b in boxes]
        concat_boxes = torch.cat(boxes, dim=0)
        box_sum = 0
        for val in boxes_per_image:
            box_sum += val
        if box_sum > 0:
            rel_codes = rel_codes.reshape(box_sum, -1)
        pred_boxes = self.decode_single(rel_codes, concat_boxes)
        if box_sum > 0:
            pred_boxes = pred_boxes.reshape(box_sum, -1, 4)
        return pred_boxes

    def decode_single(self, rel_codes: Tensor, boxes: Tensor) -> Tensor:
        """From a set of original boxes and encoded relative box offsets, get the decoded boxes: one launch (F.box_decode)."""
        return F.box_decode(boxes.to(rel_codes.dtype), rel_codes, self.weights, self.bbox_xform_clip)


class RPNHead(nn.Module):
    """rpn.py:15-79.  forward(x: List[Tensor]) -> (logits, bbox_reg), per level (N, A, H, W) and (N, 4 A, H, W): channel slices of
    ONE (N, 5 A, H, W) tensor per level."""

    _version = 2

    def __init__(self, in_channels: int, num_anchors: int, conv_depth=1) -> None:
        super().__init__()
        convs = []
        for _ in range(conv_depth):
            convs.append(Conv2dNormActivation(in_channels, in_channels, kernel_size=3, norm_layer=None))
        self.conv = nn.Sequential(*convs)
        self.cls_logits = nn.Conv2d(in_channels, num_anchors, kernel_size=1, stride=1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=1, stride=1)

        for layer in self.modules():
            if isinstance(layer, torch.nn.Conv2d):
                torch.nn.init.normal_(layer.weight, std=0.01)  # type: ignore[arg-type]
                if layer.bias is not None:
                    torch.nn.init.constant_(layer.bias, 0)  # type: ignore[arg-type]
        self._joint = _ParameterCache()
        self.eval()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)

        if version is None or version < 2:
            for type in ["weight", "bias"]:
                old_key = f"{prefix}conv.{type}"
                new_key = f"{prefix}conv.0.0.{type}"
                if old_key in state_dict:
                    state_dict[new_key] = state_dict.pop(old_key)

        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def joint_pointwise(self, device) -> Tuple[Tensor, Tensor]:
        """(weight (5 A, C, 1, 1), bias (5 A)) of cls_logits and bbox_pred as one conv on `device`, rebuilt when a parameter changes
        (the cache of resnet.py / fpn.py's folded norms)."""
        tensors = (self.cls_logits.weight, self.cls_logits.bias, self.bbox_pred.weight, self.bbox_pred.bias)
        key = _tensor_versions(*tensors) + (str(device),)

        def joint():
            with torch.no_grad():
                return (torch.cat([self.cls_logits.weight, self.bbox_pred.weight]).to(device, torch.float32).contiguous(),
                        torch.cat([self.cls_logits.bias, self.bbox_pred.bias]).to(device, torch.float32).contiguous())
        return self._joint.lookup(key, joint)

    def forward(self, x: List[Tensor]) -> Tuple[List[Tensor], List[Tensor]]:
        if self.training:
            raise RuntimeError("the MI355X RPNHead is inference only: call .eval()")
        logits = []
        bbox_reg = []
        a = self.cls_logits.out_channels
        deps = (*x, self.cls_logits.weight)
        with torch.no_grad():  # no autograd bookkeeping per launch; the results are marked once (their backward raises)
            for feature in x:
                t = feature
                for block in self.conv:
                    t = block(t)
                w, b = self.joint_pointwise(t.device)
                both = F.conv_norm_act(t, w, b)
                logits.append(both[:, :a])
                bbox_reg.append(both[:, a:])
        return ([_lib.forward_only(v, "RPNHead.forward", *deps) for v in logits],
                [_lib.forward_only(v, "RPNHead.forward", *deps) for v in bbox_reg])


def permute_and_flatten(layer: Tensor, N: int, A: int, C: int, H: int, W: int) -> Tensor:
    """rpn.py:82-86"""
    layer = layer.view(N, -1, C, H, W)
    layer = layer.permute(0, 3, 4, 1, 2)
    layer = layer.reshape(N, -1, C)
    return layer


def concat_box_prediction_layers(box_cls: List[Tensor], box_regression: List[Tensor]) -> Tuple[Tensor, Tensor]:
    """rpn.py:89-110: the reference's (y, x, a) layout of all levels, as torch compositions (the RPN itself never builds it)."""
    box_cls_flattened = []
    box_regression_flattened = []
    # for each feature level, permute the outputs to make them be in the
    # same format as the labels. Note that the labels are computed for
    # all feature levels concatenated, so we keep the same representation
    # for the objectness and the box_regression
    for box_cls_per_level, box_regression_per_level in zip(box_cls, box_regression):
        N, AxC, H, W = box_cls_per_level.shape
        Ax4 = box_regression_per_level.shape[1]
        A = Ax4 // 4
        C = AxC // A
        box_cls_per_level = permute_and_flatten(box_cls_per_level.contiguous(), N, A, C, H, W)
        box_cls_flattened.append(box_cls_per_level)

        box_regression_per_level = permute_and_flatten(box_regression_per_level.contiguous(), N, A, 4, H, W)
        box_regression_flattened.append(box_regression_per_level)
    # concatenate on the first dimension (representing the feature levels), to
    # take into account the way the labels were generated (with all feature maps
    # being concatenated as well)
    box_cls = torch.cat(box_cls_flattened, dim=1).flatten(0, -2)
    box_regression = torch.cat(box_regression_flattened, dim=1).reshape(-1, 4)
    return box_cls, box_regression


def filter_proposals_detailed(objectness: List[Tensor], pred_bbox_deltas: List[Tensor], cell_anchors: List[Tensor],
                              strides: List[Tuple[int, int]], image_shapes: List[Tuple[int, int]], box_coder: BoxCoder, pre_nms_top_n: int,
                              post_nms_top_n: int, nms_thresh: float, min_size: float = 1e-3,
                              score_thresh: float = 0.0) -> Tuple[List[Tensor], List[Tensor]]:
    """rpn.py filter_proposals on the head's per-level NCHW outputs -> (boxes, scores) per image: F.rpn_topk, F.rpn_decode, then per
    image the boolean indexing by `valid` (the one read-back besides the nms's count), ops.batched_nms and the slice."""
    idx = F.rpn_topk(objectness, pre_nms_top_n)
    boxes, scores, levels, valid = F.rpn_decode(objectness, pred_bbox_deltas, idx, cell_anchors, strides, image_shapes, box_coder.weights,
                                                box_coder.bbox_xform_clip, min_size, score_thresh)
    final_boxes, final_scores = [], []
    for b, s, lvl, v in zip(boxes, scores, levels, valid):
        b, s, lvl = b[v], s[v], lvl[v]
        # non-maximum suppression, independently done per level
        keep = box_ops.batched_nms(b, s, lvl, nms_thresh)
        # keep only topk scoring predictions
        keep = keep[:post_nms_top_n]
        final_boxes.append(b[keep])
        final_scores.append(s[keep])
    return final_boxes, final_scores


class RegionProposalNetwork(nn.Module):
    """rpn.py:113-388, inference: forward(images, features) -> (boxes per image, {}).  The matcher, the sampler and the losses of
    the reference are training-only and not built; their constructor arguments are kept."""

    __annotations__ = {"box_coder": BoxCoder}

    def __init__(self, anchor_generator: AnchorGenerator, head: nn.Module,
                 # Faster-RCNN Training
                 fg_iou_thresh: float, bg_iou_thresh: float, batch_size_per_image: int, positive_fraction: float,
                 # Faster-RCNN Inference
                 pre_nms_top_n: Dict[str, int], post_nms_top_n: Dict[str, int], nms_thresh: float, score_thresh: float = 0.0) -> None:
        super().__init__()
        self.anchor_generator = anchor_generator
        self.head = head
        self.box_coder = BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
        # used during training (kept as given: the matcher and the sampler are not built)
        self.fg_iou_thresh, self.bg_iou_thresh = fg_iou_thresh, bg_iou_thresh
        self.batch_size_per_image, self.positive_fraction = batch_size_per_image, positive_fraction
        # used during testing
        self._pre_nms_top_n = pre_nms_top_n
        self._post_nms_top_n = post_nms_top_n
        self.nms_thresh = nms_thresh
        self.score_thresh = score_thresh
        self.min_size = 1e-3
        self.eval()

    def pre_nms_top_n(self) -> int:
        if self.training:
            return self._pre_nms_top_n["training"]
        return self._pre_nms_top_n["testing"]

    def post_nms_top_n(self) -> int:
        if self.training:
            return self._post_nms_top_n["training"]
        return self._post_nms_top_n["testing"]

    def filter_proposals_detailed(self, images: ImageList, features: Dict[str, Tensor]) -> Tuple[List[Tensor], List[Tensor]]:
        """(boxes, scores) per image: `forward` with the scores the reference's filter_proposals also computes."""
        if self.training:
            raise RuntimeError("the MI355X RegionProposalNetwork is inference only: call .eval()")
        # RPN uses all feature maps that are available
        features = list(features.values())
        for f in features:
            if f.dtype != torch.float32:
                raise TypeError(f"RegionProposalNetwork computes in float32. Got features {f.dtype}")
        with torch.no_grad():
            objectness, pred_bbox_deltas = self.head(features)
            image_size = images.tensors.shape[-2:]
            strides = [(int(image_size[0]) // int(o.shape[-2]), int(image_size[1]) // int(o.shape[-1])) for o in objectness]
            cell_anchors = self.anchor_generator.cell_anchors
            torch._assert(len(cell_anchors) == len(objectness),
                          "Anchors should be Tuple[Tuple[int]] because each feature "
                          "map could potentially have different sizes and aspect ratios. "
                          "There needs to be a match between the number of "
                          "feature maps passed and the number of sizes / aspect ratios specified.")
            boxes, scores = filter_proposals_detailed(objectness, pred_bbox_deltas, cell_anchors, strides, images.image_sizes, self.box_coder,
                                                      self.pre_nms_top_n(), self.post_nms_top_n(), self.nms_thresh, self.min_size,
                                                      self.score_thresh)
        deps = (*features, *self.head.parameters())
        return ([_lib.forward_only(b, "RegionProposalNetwork.forward", *deps) for b in boxes],
                [_lib.forward_only(s, "RegionProposalNetwork.forward", *deps) for s in scores])

    def forward(self, images: ImageList, features: Dict[str, Tensor],
                targets: Optional[List[Dict[str, Tensor]]] = None) -> Tuple[List[Tensor], Dict[str, Tensor]]:
        if self.training or targets is not None:
            raise RuntimeError("the MI355X RegionProposalNetwork is inference only: call .eval() and pass no targets")
        boxes, _ = self.filter_proposals_detailed(images, features)
        return boxes, {}
