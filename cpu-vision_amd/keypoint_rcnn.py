"""Keypoint R-CNN inference on the MI355X kernels: models/detection/keypoint_rcnn.py of the reference -- KeypointRCNN,
KeypointRCNNHeads, KeypointRCNNPredictor and the keypointrcnn_resnet50_fpn builder -- with the same classes, constructor arguments,
defaults, argument errors, child names (roi_heads.keypoint_roi_pool / keypoint_head.{0, 2, ..., 14} / keypoint_predictor.
kps_score_lowres), state-dict keys and construction order.  Only `forward` differs.

KeypointRCNNHeads runs every Conv2d + ReLU pair as one 3x3 MFMA launch.  KeypointRCNNPredictor is F.conv_transpose2d_bias_act
(ConvTranspose2d(4, stride 2, padding 1) + bias, ONE launch: the implicit-GEMM kernel with the transposed store) then the x2
bilinear F.interpolate.  RoIHeads.forward runs the branch and F.heatmaps_to_keypoints, one launch for the whole batch
(roi_heads.py); the transform's postprocess rescales the keypoints (transform.py).  DESIGN.md 3.29.
Inference only, float32 only; there are no weight files, as in faster_rcnn.py.
"""
from __future__ import annotations

from typing import Any, Optional, Tuple

import torch
from torch import nn, Tensor

from . import _lib
from . import functional as F
from . import resnet
from .backbone_utils import _resnet_fpn_extractor, _validate_trainable_layers
from .faster_rcnn import FasterRCNN
from .mobilenet import _ParameterCache, _tensor_versions, FrozenBatchNorm2d
from .ops import MultiScaleRoIAlign
from .roi_heads import check_keypoint_modules

__all__ = ["KeypointRCNN", "KeypointRCNNHeads", "KeypointRCNNPredictor", "keypointrcnn_resnet50_fpn"]


class KeypointRCNN(FasterRCNN):
    """keypoint_rcnn.py:22-249.  forward(images) -> List[{boxes, labels, scores, keypoints (N, K, 3) rows (x, y, visibility = 1) in
    the coordinates of the images as given, keypoints_scores (N, K)}]."""

    def __init__(self, backbone, num_classes=None,
                 # transform parameters
                 min_size=None, max_size=1333, image_mean=None, image_std=None,
                 # RPN parameters
                 rpn_anchor_generator=None, rpn_head=None, rpn_pre_nms_top_n_train=2000, rpn_pre_nms_top_n_test=1000,
                 rpn_post_nms_top_n_train=2000, rpn_post_nms_top_n_test=1000, rpn_nms_thresh=0.7, rpn_fg_iou_thresh=0.7,
                 rpn_bg_iou_thresh=0.3, rpn_batch_size_per_image=256, rpn_positive_fraction=0.5, rpn_score_thresh=0.0,
                 # Box parameters
                 box_roi_pool=None, box_head=None, box_predictor=None, box_score_thresh=0.05, box_nms_thresh=0.5,
                 box_detections_per_img=100, box_fg_iou_thresh=0.5, box_bg_iou_thresh=0.5, box_batch_size_per_image=512,
                 box_positive_fraction=0.25, bbox_reg_weights=None,
                 # keypoint parameters
                 keypoint_roi_pool=None, keypoint_head=None, keypoint_predictor=None, num_keypoints=None, **kwargs):

        if not isinstance(keypoint_roi_pool, (MultiScaleRoIAlign, type(None))):
            raise TypeError(f"keypoint_roi_pool should be of type MultiScaleRoIAlign or None instead of {type(keypoint_roi_pool)}")
        if min_size is None:
            min_size = (640, 672, 704, 736, 768, 800)

        if num_keypoints is not None:
            if keypoint_predictor is not None:
                raise ValueError("num_keypoints should be None when keypoint_predictor is specified")
        else:
            num_keypoints = 17

        out_channels = backbone.out_channels

        if keypoint_roi_pool is None:
            keypoint_roi_pool = MultiScaleRoIAlign(featmap_names=["0", "1", "2", "3"], output_size=14, sampling_ratio=2)

        if keypoint_head is None:
            keypoint_layers = tuple(512 for _ in range(8))
            keypoint_head = KeypointRCNNHeads(out_channels, keypoint_layers)

        if keypoint_predictor is None:
            keypoint_dim_reduced = 512  # == keypoint_layers[-1]
            keypoint_predictor = KeypointRCNNPredictor(keypoint_dim_reduced, num_keypoints)

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

        check_keypoint_modules(keypoint_roi_pool, keypoint_head, keypoint_predictor)
        self.roi_heads.keypoint_roi_pool = keypoint_roi_pool
        self.roi_heads.keypoint_head = keypoint_head
        self.roi_heads.keypoint_predictor = keypoint_predictor


class KeypointRCNNHeads(nn.Sequential):
    """keypoint_rcnn.py:252-267: [Conv2d(3x3, padding 1), ReLU(inplace)] per entry of `layers` (children 0, 1, ..., the convs at the
    even indices); forward runs every pair as ONE launch (F.conv2d_bias_relu, the 3x3 MFMA kernel)."""

    def __init__(self, in_channels, layers):
        d = []
        next_feature = in_channels
        for out_channels in layers:
            d.append(nn.Conv2d(next_feature, out_channels, 3, stride=1, padding=1))
            d.append(nn.ReLU(inplace=True))
            next_feature = out_channels
        super().__init__(*d)
        for m in self.children():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                nn.init.constant_(m.bias, 0)
        self.eval()

    def forward(self, x: Tensor) -> Tensor:
        if self.training:
            raise RuntimeError("the MI355X KeypointRCNNHeads is inference only: call .eval()")
        inp = x
        layers = list(self)
        if len(layers) % 2 or not all(isinstance(c, nn.Conv2d) and isinstance(a, nn.ReLU) for c, a in zip(layers[::2], layers[1::2])):
            raise NotImplementedError("KeypointRCNNHeads: the MI355X path runs [Conv2d, ReLU] pairs only")
        with torch.no_grad():
            for conv in layers[::2]:
                x = F.conv2d_bias_relu(x, conv.weight, conv.bias)
        return _lib.forward_only(x, "KeypointRCNNHeads.forward", inp, *self.parameters())


class KeypointRCNNPredictor(nn.Module):
    """keypoint_rcnn.py:270-291: kps_score_lowres (ConvTranspose2d(4, stride 2, padding 1)) + bias as ONE launch, then the x2 bilinear
    interpolate as one."""

    def __init__(self, in_channels, num_keypoints):
        super().__init__()
        input_features = in_channels
        deconv_kernel = 4
        self.kps_score_lowres = nn.ConvTranspose2d(input_features, num_keypoints, deconv_kernel, stride=2,
                                                   padding=deconv_kernel // 2 - 1)
        nn.init.kaiming_normal_(self.kps_score_lowres.weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.kps_score_lowres.bias, 0)
        self.up_scale = 2
        self.out_channels = num_keypoints
        self._relaid = _ParameterCache()
        self.eval()

    def relaid(self, device) -> Tuple[Tensor, Optional[Tensor]]:
        """kps_score_lowres's weight as the (4 Cout, Cin, 2, 2) weight of the equivalent 2x2 convolution and its bias repeated four
        times on `device` (F.conv_transpose4x4_relayout), rebuilt when a parameter changes (the cache of MaskRCNNPredictor.relaid)."""
        conv = self.kps_score_lowres
        key = _tensor_versions(conv.weight, conv.bias) + (str(device),)
        return self._relaid.lookup(key, lambda: F.conv_transpose4x4_relayout(conv.weight, conv.bias, device))

    def forward(self, x: Tensor) -> Tensor:
        if self.training:
            raise RuntimeError("the MI355X KeypointRCNNPredictor is inference only: call .eval()")
        inp = x
        conv = self.kps_score_lowres
        with torch.no_grad():
            x = F.conv_transpose2d_bias_act(x, conv.weight, conv.bias, None, stride=conv.stride, padding=conv.padding,
                                            output_padding=conv.output_padding, groups=conv.groups, dilation=conv.dilation,
                                            relaid=self.relaid(x.device))
            # the reference calls interpolate(scale_factor=2.0, recompute_scale_factor=False): torch then takes 1 / 2.0 as the axis
            # scale, and 0.5 == float32(h) / float32(2 h) exactly, which is the scale of size=[2 h, 2 w] -- the same call
            size = [int(x.shape[-2]) * int(self.up_scale), int(x.shape[-1]) * int(self.up_scale)]
            x = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
        return _lib.forward_only(x, "KeypointRCNNPredictor.forward", inp, *self.parameters())


def keypointrcnn_resnet50_fpn(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                              num_keypoints: Optional[int] = None, weights_backbone: Optional[Any] = None,
                              trainable_backbone_layers: Optional[int] = None, **kwargs: Any) -> KeypointRCNN:
    """keypoint_rcnn.py:356-474: Keypoint R-CNN with a ResNet-50-FPN backbone (FrozenBatchNorm2d folded into the convs), 2 classes
    and 17 keypoints unless `num_classes` / `num_keypoints` say otherwise.

    The package ships no weight files: `weights` and `weights_backbone` must be None; load a state dict of the reference's model
    with load_state_dict (the keys are the reference's)."""
    if weights is not None or weights_backbone is not None:
        raise ValueError("keypointrcnn_resnet50_fpn: the package ships no weight files, weights and weights_backbone must be None; "
                         "load a state dict with load_state_dict")
    if num_classes is None:
        num_classes = 2
    if num_keypoints is None:
        num_keypoints = 17

    is_trained = False
    trainable_backbone_layers = _validate_trainable_layers(is_trained, trainable_backbone_layers, 5, 3)

    backbone = resnet.resnet50(norm_layer=FrozenBatchNorm2d)
    backbone = _resnet_fpn_extractor(backbone, trainable_backbone_layers)
    model = KeypointRCNN(backbone, num_classes, num_keypoints=num_keypoints, **kwargs)
    return model
