"""Mask R-CNN inference on the MI355X kernels: models/detection/mask_rcnn.py of the reference -- MaskRCNN, MaskRCNNHeads,
MaskRCNNPredictor and the maskrcnn_resnet50_fpn builder -- with the same classes, constructor arguments, defaults, argument errors,
child names (roi_heads.mask_roi_pool / mask_head.{i}.0 / mask_predictor.conv5_mask / relu / mask_fcn_logits), state-dict keys and
construction order.  Only `forward` differs.

MaskRCNNHeads is the package's Conv2dNormActivation per layer (3x3 conv + bias + ReLU, one launch each).  MaskRCNNPredictor is
F.conv_transpose2d_bias_act (ConvTranspose2d(2, 2) + bias + ReLU, ONE launch: the pointwise MFMA kernel with a pixel-shuffle store)
then the pointwise mask_fcn_logits.  RoIHeads.forward runs the branch and F.mask_probs (roi_heads.py); the transform's postprocess
pastes the masks into the image with F.paste_masks_in_image (transform.py).  DESIGN.md 3.28.
Inference only, float32 only; there are no weight files, as in faster_rcnn.py.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Callable, Optional, Tuple

import torch
from torch import nn, Tensor

from . import _lib
from . import functional as F
from . import resnet
from .backbone_utils import _resnet_fpn_extractor, _validate_trainable_layers
from .faster_rcnn import FasterRCNN
from .mobilenet import _ParameterCache, _tensor_versions, Conv2dNormActivation, FrozenBatchNorm2d
from .ops import MultiScaleRoIAlign

__all__ = ["MaskRCNN", "MaskRCNNHeads", "MaskRCNNPredictor", "maskrcnn_resnet50_fpn"]


class MaskRCNN(FasterRCNN):
    """mask_rcnn.py:24-260.  forward(images) -> List[{boxes, labels, scores, masks (N, 1, H, W) float32 in 0..1}], the masks pasted
    into the images as given (not thresholded, as in the reference)."""

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
                 box_positive_fraction=0.25, bbox_reg_weights=None,
                 # Mask parameters
                 mask_roi_pool=None, mask_head=None, mask_predictor=None, **kwargs):

        if not isinstance(mask_roi_pool, (MultiScaleRoIAlign, type(None))):
            raise TypeError(f"mask_roi_pool should be of type MultiScaleRoIAlign or None instead of {type(mask_roi_pool)}")

        if num_classes is not None:
            if mask_predictor is not None:
                raise ValueError("num_classes should be None when mask_predictor is specified")

        out_channels = backbone.out_channels

        if mask_roi_pool is None:
            mask_roi_pool = MultiScaleRoIAlign(featmap_names=["0", "1", "2", "3"], output_size=14, sampling_ratio=2)

        if mask_head is None:
            mask_layers = (256, 256, 256, 256)
            mask_dilation = 1
            mask_head = MaskRCNNHeads(out_channels, mask_layers, mask_dilation)

        if mask_predictor is None:
            mask_predictor_in_channels = 256  # == mask_layers[-1]
            mask_dim_reduced = 256
            mask_predictor = MaskRCNNPredictor(mask_predictor_in_channels, mask_dim_reduced, num_classes)

        super().__init__(
            backbone, num_classes,
            # transform parameters
            min_size, max_size, image_mean, image_std,
            # RPN-specific parameters
            rpn_anchor_generator, rpn_head, rpn_pre_nms_top_n_train, rpn_pre_nms_top_n_test, rpn_post_nms_top_n_train,
            rpn_post_nms_top_n_test, rpn_nms_thresh, rpn_fg_iou_thresh, rpn_bg_iou_thresh, rpn_batch_size_per_image,
            rpn_positive_fraction, rpn_score_thresh,
            # Box parameters
            box_roi_pool, box_head, box_predictor, box_score_thresh, box_nms_thresh, box_detections_per_img, box_fg_iou_thresh,
            box_bg_iou_thresh, box_batch_size_per_image, box_positive_fraction, bbox_reg_weights, **kwargs)

        self.roi_heads.mask_roi_pool = mask_roi_pool
        self.roi_heads.mask_head = mask_head
        self.roi_heads.mask_predictor = mask_predictor


class MaskRCNNHeads(nn.Sequential):
    """mask_rcnn.py:263-315: `layers` Conv2dNormActivation(3x3, stride 1, padding = dilation) blocks, one launch each.  The package's
    Conv2dNormActivation covers dilation 1 and, without a norm layer, conv + bias + ReLU; a head built with dilation != 1 or with a
    norm_layer raises NotImplementedError from its forward (nothing is computed another way)."""

    _version = 2

    def __init__(self, in_channels, layers, dilation, norm_layer: Optional[Callable[..., nn.Module]] = None):
        blocks = []
        next_feature = in_channels
        for layer_features in layers:
            blocks.append(Conv2dNormActivation(next_feature, layer_features, kernel_size=3, stride=1, padding=dilation,
                                               dilation=dilation, norm_layer=norm_layer))
            next_feature = layer_features

        super().__init__(*blocks)
        for layer in self.modules():
            if isinstance(layer, nn.Conv2d):
                nn.init.kaiming_normal_(layer.weight, mode="fan_out", nonlinearity="relu")
                if layer.bias is not None:
                    nn.init.zeros_(layer.bias)
        self.eval()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)

        if version is None or version < 2:
            num_blocks = len(self)
            for i in range(num_blocks):
                for type in ["weight", "bias"]:
                    old_key = f"{prefix}mask_fcn{i+1}.{type}"
                    new_key = f"{prefix}{i}.0.{type}"
                    if old_key in state_dict:
                        state_dict[new_key] = state_dict.pop(old_key)

        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x: Tensor) -> Tensor:
        if self.training:
            raise RuntimeError("the MI355X MaskRCNNHeads is inference only: call .eval()")
        inp = x
        with torch.no_grad():
            for block in self:
                x = block(x)
        return _lib.forward_only(x, "MaskRCNNHeads.forward", inp, *self.parameters())


class MaskRCNNPredictor(nn.Sequential):
    """mask_rcnn.py:318-334: conv5_mask (ConvTranspose2d(2, 2)) + ReLU as ONE launch, then mask_fcn_logits (1x1 conv) as one."""

    def __init__(self, in_channels, dim_reduced, num_classes):
        super().__init__(
            OrderedDict(
                [
                    ("conv5_mask", nn.ConvTranspose2d(in_channels, dim_reduced, 2, 2, 0)),
                    ("relu", nn.ReLU(inplace=True)),
                    ("mask_fcn_logits", nn.Conv2d(dim_reduced, num_classes, 1, 1, 0)),
                ]
            )
        )

        for name, param in self.named_parameters():
            if "weight" in name:
                nn.init.kaiming_normal_(param, mode="fan_out", nonlinearity="relu")
            # elif "bias" in name:
            #     nn.init.constant_(param, 0)
        self._relaid = _ParameterCache()
        self.eval()

    def relaid(self, device) -> Tuple[Tensor, Optional[Tensor]]:
        """conv5_mask's weight as (4 Cout, Cin) and its bias repeated four times on `device` (F.conv_transpose2x2_relayout), rebuilt
        when a parameter changes (the cache of FastRCNNPredictor.joint_linear)."""
        conv = self.conv5_mask
        key = _tensor_versions(conv.weight, conv.bias) + (str(device),)
        return self._relaid.lookup(key, lambda: F.conv_transpose2x2_relayout(conv.weight, conv.bias, device))

    def forward(self, x: Tensor) -> Tensor:
        if self.training:
            raise RuntimeError("the MI355X MaskRCNNPredictor is inference only: call .eval()")
        inp = x
        conv, logits = self.conv5_mask, self.mask_fcn_logits
        with torch.no_grad():
            x = F.conv_transpose2d_bias_act(x, conv.weight, conv.bias, "relu", stride=conv.stride, padding=conv.padding,
                                            output_padding=conv.output_padding, groups=conv.groups, dilation=conv.dilation,
                                            relaid=self.relaid(x.device))
            x = F.conv_norm_act(x, logits.weight, logits.bias)
        return _lib.forward_only(x, "MaskRCNNPredictor.forward", inp, *self.parameters())


def maskrcnn_resnet50_fpn(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                          weights_backbone: Optional[Any] = None, trainable_backbone_layers: Optional[int] = None,
                          **kwargs: Any) -> MaskRCNN:
    """mask_rcnn.py:398-493: Mask R-CNN with a ResNet-50-FPN backbone (FrozenBatchNorm2d folded into the convs), 91 classes unless
    `num_classes` says otherwise.

    The package ships no weight files: `weights` and `weights_backbone` must be None; load a state dict of the reference's model
    with load_state_dict (the keys are the reference's)."""
    if weights is not None or weights_backbone is not None:
        raise ValueError("maskrcnn_resnet50_fpn: the package ships no weight files, weights and weights_backbone must be None; "
                         "load a state dict with load_state_dict")
    if num_classes is None:
        num_classes = 91

    is_trained = False
    trainable_backbone_layers = _validate_trainable_layers(is_trained, trainable_backbone_layers, 5, 3)

    backbone = resnet.resnet50(norm_layer=FrozenBatchNorm2d)
    backbone = _resnet_fpn_extractor(backbone, trainable_backbone_layers)
    model = MaskRCNN(backbone, num_classes=num_classes, **kwargs)
    return model
