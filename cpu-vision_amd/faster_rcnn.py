"""Faster R-CNN inference on the MI355X kernels: models/detection/faster_rcnn.py of the reference -- FasterRCNN, TwoMLPHead,
FastRCNNPredictor and the fasterrcnn_resnet50_fpn builder -- with the same classes, constructor arguments, defaults, argument errors,
child names (transform, backbone, rpn, roi_heads.box_roi_pool / box_head.fc6 / fc7 / box_predictor.cls_score / bbox_pred), state-dict
keys and construction order.  Only `forward` differs.

TwoMLPHead is two F.linear_bias_relu launches (linear + bias + ReLU each).  FastRCNNPredictor runs cls_score and bbox_pred as ONE
F.linear_bias_relu over their concatenated (5 C, K) weight -- the hidden vector read once -- and returns the two results as column
slices of that one tensor, which F.roi_detections takes by their row strides (RPNHead does the same with its two 1x1 convs).
Inference only, float32 only; there are no weight files, as in resnet.py.
"""
from __future__ import annotations

from typing import Any, Optional, Tuple

import torch
from torch import nn, Tensor

from . import _lib
from . import functional as F
from . import resnet
from .anchor_utils import AnchorGenerator
from .backbone_utils import _resnet_fpn_extractor, _validate_trainable_layers
from .generalized_rcnn import GeneralizedRCNN
from .mobilenet import _ParameterCache, _tensor_versions, FrozenBatchNorm2d
from .ops import MultiScaleRoIAlign
from .roi_heads import RoIHeads
from .rpn import RegionProposalNetwork, RPNHead
from .transform import GeneralizedRCNNTransform

__all__ = ["FasterRCNN", "TwoMLPHead", "FastRCNNPredictor", "fasterrcnn_resnet50_fpn"]


def _default_anchorgen():
    anchor_sizes = ((32,), (64,), (128,), (256,), (512,))
    aspect_ratios = ((0.5, 1.0, 2.0),) * len(anchor_sizes)
    return AnchorGenerator(anchor_sizes, aspect_ratios)


class FasterRCNN(GeneralizedRCNN):
    """faster_rcnn.py:44-297.  forward(images: List[Tensor (C, H, W) float32 in 0..1]) -> List[{boxes (N, 4) as (x1, y1, x2, y2),
    labels (N,) int64, scores (N,)}], the boxes in the coordinates of the images as given.  The images may have any sizes: the
    transform resizes them to min_size / max_size (transform.py).  `**kwargs` go to GeneralizedRCNNTransform (`_skip_resize=True`
    for images that already have their final size)."""

    def __init__(self, backbone, num_classes=None,
                 # transform parameters
                 min_size=800, max_size=1333, image_mean=None, image_std=None,
                 # RPN parameters
                 rpn_anchor_generator=None, rpn_head=None, rpn_pre_nms_top_n_train=2000, rpn_pre_nms_top_n_test=1000,
                 rpn_post_nms_top_n_train=2000, rpn_post_nms_top_n_test=1000, rpn_nms_thresh=0.7, rpn_fg_iou_thresh=0.7,
                 rpn_bg_iou_thresh=0.3, rpn_batch_size_per_image=256, rpn_positive_fraction=0.5, rpn_score_thresh=0.0,
                 # Box parameters
                 box_roi_pool=None, box_head=None, box_predictor=None, box_score_thresh=0.05, box_nms_thresh=0.5,
                 box_detections_per_img=100, box_fg_iou_thresh=0.5, box_bg_iou_thresh=0.5, box_batch_size_per_image=512,
                 box_positive_fraction=0.25, bbox_reg_weights=None, **kwargs):

        if not hasattr(backbone, "out_channels"):
            raise ValueError(
                "backbone should contain an attribute out_channels "
                "specifying the number of output channels (assumed to be the "
                "same for all the levels)"
            )

        if not isinstance(rpn_anchor_generator, (AnchorGenerator, type(None))):
            raise TypeError(f"rpn_anchor_generator should be of type AnchorGenerator or None instead of {type(rpn_anchor_generator)}")
        if not isinstance(box_roi_pool, (MultiScaleRoIAlign, type(None))):
            raise TypeError(f"box_roi_pool should be of type MultiScaleRoIAlign or None instead of {type(box_roi_pool)}")

        if num_classes is not None:
            if box_predictor is not None:
                raise ValueError("num_classes should be None when box_predictor is specified")
        else:
            if box_predictor is None:
                raise ValueError("num_classes should not be None when box_predictor is not specified")

        out_channels = backbone.out_channels

        if rpn_anchor_generator is None:
            rpn_anchor_generator = _default_anchorgen()
        if rpn_head is None:
            rpn_head = RPNHead(out_channels, rpn_anchor_generator.num_anchors_per_location()[0])

        rpn_pre_nms_top_n = dict(training=rpn_pre_nms_top_n_train, testing=rpn_pre_nms_top_n_test)
        rpn_post_nms_top_n = dict(training=rpn_post_nms_top_n_train, testing=rpn_post_nms_top_n_test)

        rpn = RegionProposalNetwork(rpn_anchor_generator, rpn_head, rpn_fg_iou_thresh, rpn_bg_iou_thresh, rpn_batch_size_per_image,
                                    rpn_positive_fraction, rpn_pre_nms_top_n, rpn_post_nms_top_n, rpn_nms_thresh,
                                    score_thresh=rpn_score_thresh)

        if box_roi_pool is None:
            box_roi_pool = MultiScaleRoIAlign(featmap_names=["0", "1", "2", "3"], output_size=7, sampling_ratio=2)

        if box_head is None:
            resolution = box_roi_pool.output_size[0]
            representation_size = 1024
            box_head = TwoMLPHead(out_channels * resolution**2, representation_size)

        if box_predictor is None:
            representation_size = 1024
            box_predictor = FastRCNNPredictor(representation_size, num_classes)

        roi_heads = RoIHeads(
            # Box
            box_roi_pool, box_head, box_predictor, box_fg_iou_thresh, box_bg_iou_thresh, box_batch_size_per_image, box_positive_fraction,
            bbox_reg_weights, box_score_thresh, box_nms_thresh, box_detections_per_img)

        if image_mean is None:
            image_mean = [0.485, 0.456, 0.406]
        if image_std is None:
            image_std = [0.229, 0.224, 0.225]
        transform = GeneralizedRCNNTransform(min_size, max_size, image_mean, image_std, **kwargs)

        super().__init__(backbone, rpn, roi_heads, transform)


class TwoMLPHead(nn.Module):
    """faster_rcnn.py:300-323: flatten -> fc6 + ReLU -> fc7 + ReLU, two launches."""

    def __init__(self, in_channels, representation_size):
        super().__init__()

        self.fc6 = nn.Linear(in_channels, representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)
        self.eval()

    def forward(self, x: Tensor) -> Tensor:
        if self.training:
            raise RuntimeError("the MI355X TwoMLPHead is inference only: call .eval()")
        inp = x
        with torch.no_grad():
            x = x.flatten(start_dim=1)

            x = F.linear_bias_relu(x, self.fc6.weight, self.fc6.bias, relu=True)
            x = F.linear_bias_relu(x, self.fc7.weight, self.fc7.bias, relu=True)

        return _lib.forward_only(x, "TwoMLPHead.forward", inp, *self.parameters())


class FastRCNNPredictor(nn.Module):
    """faster_rcnn.py:326-350.  forward(x) -> (scores (R, C), bbox_deltas (R, 4 C)): column slices of ONE (R, 5 C) tensor."""

    def __init__(self, in_channels, num_classes):
        super().__init__()
        self.cls_score = nn.Linear(in_channels, num_classes)
        self.bbox_pred = nn.Linear(in_channels, num_classes * 4)
        self._joint = _ParameterCache()
        self.eval()

    def joint_linear(self, device) -> Tuple[Tensor, Tensor]:
        """(weight (5 C, K), bias (5 C)) of cls_score and bbox_pred as one linear layer on `device`, rebuilt when a parameter changes
        (the cache of RPNHead.joint_pointwise)."""
        tensors = (self.cls_score.weight, self.cls_score.bias, self.bbox_pred.weight, self.bbox_pred.bias)
        key = _tensor_versions(*tensors) + (str(device),)

        def joint():
            with torch.no_grad():
                return (torch.cat([self.cls_score.weight, self.bbox_pred.weight]).to(device, torch.float32).contiguous(),
                        torch.cat([self.cls_score.bias, self.bbox_pred.bias]).to(device, torch.float32).contiguous())
        return self._joint.lookup(key, joint)

    def forward(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        if self.training:
            raise RuntimeError("the MI355X FastRCNNPredictor is inference only: call .eval()")
        if x.dim() == 4:
            torch._assert(
                list(x.shape[2:]) == [1, 1],
                f"x has the wrong shape, expecting the last two dimensions to be [1,1] instead of {list(x.shape[2:])}",
            )
        inp = x
        c = self.cls_score.out_features
        with torch.no_grad():
            x = x.flatten(start_dim=1)
            w, b = self.joint_linear(x.device)
            both = F.linear_bias_relu(x, w, b, relu=False)
        deps = (inp, *self.parameters())
        scores = _lib.forward_only(both[:, :c], "FastRCNNPredictor.forward", *deps)
        bbox_deltas = _lib.forward_only(both[:, c:], "FastRCNNPredictor.forward", *deps)

        return scores, bbox_deltas


def fasterrcnn_resnet50_fpn(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                            weights_backbone: Optional[Any] = None, trainable_backbone_layers: Optional[int] = None,
                            **kwargs: Any) -> FasterRCNN:
    """faster_rcnn.py:459-571: Faster R-CNN with a ResNet-50-FPN backbone (FrozenBatchNorm2d folded into the convs), 91 classes
    unless `num_classes` says otherwise.

    The package ships no weight files: `weights` and `weights_backbone` must be None; load a state dict of the reference's model
    with load_state_dict (the keys are the reference's)."""
    if weights is not None or weights_backbone is not None:
        raise ValueError("fasterrcnn_resnet50_fpn: the package ships no weight files, weights and weights_backbone must be None; "
                         "load a state dict with load_state_dict")
    if num_classes is None:
        num_classes = 91

    is_trained = False
    trainable_backbone_layers = _validate_trainable_layers(is_trained, trainable_backbone_layers, 5, 3)

    backbone = resnet.resnet50(norm_layer=FrozenBatchNorm2d)
    backbone = _resnet_fpn_extractor(backbone, trainable_backbone_layers)
    model = FasterRCNN(backbone, num_classes=num_classes, **kwargs)
    return model
