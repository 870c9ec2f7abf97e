"""References for the RetinaNet tests (a helper module, not a test file and not a conftest).  Imports nothing from the package.

(a) A plain-torch replica of the reference's models/detection/retinanet.py (torchvision is not importable in the test
    environment), written from the reference's source like tests/_rpn_ref.py: RetinaNetClassificationHead, RetinaNetRegressionHead,
    RetinaNetHead and RetinaNet with the same constructor arguments, child names, construction order and initialisation, torch's own
    convs, torch.sigmoid and torch.topk.  AnchorGenerator, BoxCoder, Conv2dNormActivation, batched_nms and `same` are those of
    tests/_rpn_ref.py.
(b) The restatement the library is compared with bit for bit (`Numerics`, as in tests/_rpn_ref.py):
      sigmoid(v)  -> 1 / (1 + E(-v)) in float32, E the correctly rounded float32 exp             (sigmoid_cr)
      `> thresh`  -> the strict comparison with (float32)thresh, which is what torch's float32 tensor > python float does
      topk        -> the first k of torch.sort(stable=True, descending=True): equal SCORES by ascending flat index
      exp(v)      -> the correctly rounded float32 exp in decode_single
    and, for the two kernels' own outputs, `select` / `decode`: the fixed-shape (N, Ktot) form with -1 padding that
    mv_retinanet_topk_f32 / mv_retinanet_decode_f32 write.
"""
import math
from collections import OrderedDict

import torch
from torch import nn

from tests._rpn_ref import (AnchorGenerator, BoxCoder, Conv2dNormActivation, Numerics, REPLICA, RESTATEMENT, batched_nms,  # noqa: F401
                            clip_boxes_to_image, same, sigmoid_cr, topk_stable)


# ------------------------------------------------------------------------------------------------ (a) the torch replica
def _v1_to_v2_weights(state_dict, prefix):
    for i in range(4):
        for type in ["weight", "bias"]:
            old_key = f"{prefix}conv.{2*i}.{type}"
            new_key = f"{prefix}conv.{i}.0.{type}"
            if old_key in state_dict:
                state_dict[new_key] = state_dict.pop(old_key)


def permute_level(m, last):
    """(N, A * last, H, W) -> (N, HWA, last): the reference's view / permute / reshape of one level."""
    N, _, H, W = m.shape
    return m.view(N, -1, last, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, last)


class RetinaNetClassificationHead(nn.Module):
    _version = 2

    def __init__(self, in_channels, num_anchors, num_classes, prior_probability=0.01, norm_layer=None):
        super().__init__()
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

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:
            _v1_to_v2_weights(state_dict, prefix)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def maps(self, x):
        return [self.cls_logits(self.conv(features)) for features in x]

    def forward(self, x):
        return torch.cat([permute_level(m, self.num_classes) for m in self.maps(x)], dim=1)


class RetinaNetRegressionHead(nn.Module):
    _version = 2

    def __init__(self, in_channels, num_anchors, norm_layer=None):
        super().__init__()
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

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:
            _v1_to_v2_weights(state_dict, prefix)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def maps(self, x):
        return [self.bbox_reg(self.conv(features)) for features in x]

    def forward(self, x):
        return torch.cat([permute_level(m, 4) for m in self.maps(x)], dim=1)


class RetinaNetHead(nn.Module):
    def __init__(self, in_channels, num_anchors, num_classes, norm_layer=None):
        super().__init__()
        self.classification_head = RetinaNetClassificationHead(in_channels, num_anchors, num_classes, norm_layer=norm_layer)
        self.regression_head = RetinaNetRegressionHead(in_channels, num_anchors, norm_layer=norm_layer)

    def forward(self, x):
        return {"cls_logits": self.classification_head(x), "bbox_regression": self.regression_head(x)}


def default_anchorgen():
    anchor_sizes = tuple((x, int(x * 2 ** (1.0 / 3)), int(x * 2 ** (2.0 / 3))) for x in [32, 64, 128, 256, 512])
    aspect_ratios = ((0.5, 1.0, 2.0),) * len(anchor_sizes)
    return AnchorGenerator(anchor_sizes, aspect_ratios)


class Transform(nn.Module):
    """GeneralizedRCNNTransform without the resize (the library's _skip_resize=True): normalize, batch to a multiple of 32,
    rescale the boxes back (the identity without a resize)."""

    def __init__(self, image_mean, image_std, size_divisible=32):
        super().__init__()
        self.image_mean, self.image_std, self.size_divisible = image_mean, image_std, size_divisible

    def forward(self, images):
        from tests._rpn_ref import ImageList
        mean, std = torch.as_tensor(self.image_mean)[:, None, None], torch.as_tensor(self.image_std)[:, None, None]
        images = [(img - mean) / std for img in images]
        sizes = [tuple(int(d) for d in img.shape[-2:]) for img in images]
        h, w = (int(math.ceil(max(s[i] for s in sizes) / self.size_divisible) * self.size_divisible) for i in (0, 1))
        batch = images[0].new_zeros((len(images), images[0].shape[0], h, w))
        for i, img in enumerate(images):
            batch[i, :, :img.shape[1], :img.shape[2]].copy_(img)
        return ImageList(batch, sizes)


class RetinaNet(nn.Module):
    """retinanet.py:291-669, the inference path; `numerics` picks (a) or (b)."""

    def __init__(self, backbone, num_classes, min_size=800, max_size=1333, image_mean=None, image_std=None, anchor_generator=None, head=None,
                 proposal_matcher=None, score_thresh=0.05, nms_thresh=0.5, detections_per_img=300, fg_iou_thresh=0.5, bg_iou_thresh=0.4,
                 topk_candidates=1000, numerics=REPLICA):
        super().__init__()
        if not hasattr(backbone, "out_channels"):
            raise ValueError("backbone should contain an attribute out_channels specifying the number of output channels (assumed to be the "
                             "same for all the levels)")
        self.backbone = backbone
        if not isinstance(anchor_generator, (AnchorGenerator, type(None))):
            raise TypeError(f"anchor_generator should be of type AnchorGenerator or None instead of {type(anchor_generator)}")
        if anchor_generator is None:
            anchor_generator = default_anchorgen()
        self.anchor_generator = anchor_generator
        if head is None:
            head = RetinaNetHead(backbone.out_channels, anchor_generator.num_anchors_per_location()[0], num_classes)
        self.head = head
        self.proposal_matcher = proposal_matcher
        self.numerics = numerics
        self.box_coder = BoxCoder(weights=(1.0, 1.0, 1.0, 1.0), numerics=numerics)
        if image_mean is None:
            image_mean = [0.485, 0.456, 0.406]
        if image_std is None:
            image_std = [0.229, 0.224, 0.225]
        self.transform = Transform(image_mean, image_std)
        self.score_thresh = score_thresh
        self.nms_thresh = nms_thresh
        self.detections_per_img = detections_per_img
        self.topk_candidates = topk_candidates

    def postprocess_detections(self, head_outputs, anchors, image_shapes, detailed=False):
        """head_outputs / anchors: per level lists, as the reference splits them.  detailed: also the per-image candidates before
        the nms (flat indices into the concatenated (anchor, class) layout, boxes, scores, labels)."""
        class_logits = head_outputs["cls_logits"]
        box_regression = head_outputs["bbox_regression"]
        num_images = len(image_shapes)
        detections, candidates = [], []
        for index in range(num_images):
            box_regression_per_image = [br[index] for br in box_regression]
            logits_per_image = [cl[index] for cl in class_logits]
            anchors_per_image, image_shape = anchors[index], image_shapes[index]
            image_boxes, image_scores, image_labels, image_flat = [], [], [], []
            start = 0
            for box_regression_per_level, logits_per_level, anchors_per_level in zip(box_regression_per_image, logits_per_image, anchors_per_image):
                num_classes = logits_per_level.shape[-1]
                # remove low scoring boxes
                scores_per_level = self.numerics.sigmoid(logits_per_level).flatten()
                keep_idxs = scores_per_level > self.score_thresh  # float32 tensor > python float: compared in float32
                scores_per_level = scores_per_level[keep_idxs]
                topk_idxs = torch.where(keep_idxs)[0]
                # keep only topk scoring predictions
                num_topk = min(topk_idxs.size(0), self.topk_candidates)
                idxs = self.numerics.topk(scores_per_level[None], num_topk)[0]
                scores_per_level = scores_per_level[idxs]
                topk_idxs = topk_idxs[idxs]
                anchor_idxs = torch.div(topk_idxs, num_classes, rounding_mode="floor")
                labels_per_level = topk_idxs % num_classes
                boxes_per_level = self.box_coder.decode_single(box_regression_per_level[anchor_idxs], anchors_per_level[anchor_idxs])
                boxes_per_level = clip_boxes_to_image(boxes_per_level, image_shape)
                image_boxes.append(boxes_per_level)
                image_scores.append(scores_per_level)
                image_labels.append(labels_per_level)
                image_flat.append(topk_idxs + start * num_classes)
                start += logits_per_level.shape[0]
            image_boxes = torch.cat(image_boxes, dim=0)
            image_scores = torch.cat(image_scores, dim=0)
            image_labels = torch.cat(image_labels, dim=0)
            candidates.append({"idx": torch.cat(image_flat), "boxes": image_boxes, "scores": image_scores, "labels": image_labels})
            # non-maximum suppression
            keep = batched_nms(image_boxes, image_scores, image_labels, self.nms_thresh)
            keep = keep[: self.detections_per_img]
            detections.append({"boxes": image_boxes[keep], "scores": image_scores[keep], "labels": image_labels[keep]})
        return (detections, candidates) if detailed else detections

    def from_head_maps(self, images, cls_maps, reg_maps, detailed=False):
        """forward from the heads' per-level NCHW maps on (CPU tensors)."""
        num_classes = cls_maps[0].shape[1] // (reg_maps[0].shape[1] // 4)
        anchors = self.anchor_generator(images, cls_maps)
        per_level = [int(m.shape[2] * m.shape[3] * (m.shape[1] // 4)) for m in reg_maps]
        head_outputs = {"cls_logits": [permute_level(m, num_classes) for m in cls_maps], "bbox_regression": [permute_level(m, 4) for m in reg_maps]}
        split_anchors = [list(a.split(per_level)) for a in anchors]
        return self.postprocess_detections(head_outputs, split_anchors, images.image_sizes, detailed)

    def forward(self, images):
        images = self.transform(images)
        features = self.backbone(images.tensors)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        features = list(features.values())
        cls_maps, reg_maps = self.head.classification_head.maps(features), self.head.regression_head.maps(features)
        return self.from_head_maps(images, cls_maps, reg_maps)


# ------------------------------------------------------------------------------------------------ (b) what the two kernels write
def select(cls_maps, num_classes, k, score_thresh):
    """mv_retinanet_topk_f32: (N, Ktot) int32, per (image, level) the flat indices of the min(k, passing) greatest scores in stable
    descending order, then -1."""
    thresh = torch.tensor(score_thresh, dtype=torch.float32)
    out, start = [], 0
    for m in cls_maps:
        flat = permute_level(m, num_classes).flatten(1)  # (N, HWA K)
        s = sigmoid_cr(flat)
        passing = s > thresh  # strict, float32; a NaN does not pass
        seg = min(k, flat.shape[1])
        order = torch.sort(torch.where(passing, s, torch.full_like(s, -1.0)), dim=1, stable=True, descending=True)[1][:, :seg]
        taken = torch.arange(seg)[None, :] < passing.sum(1, keepdim=True)
        out.append(torch.where(taken, order + start, torch.full_like(order, -1)))
        start += flat.shape[1]
    return torch.cat(out, 1).to(torch.int32)


def decode(cls_maps, reg_maps, idx, anchors, image_sizes, num_classes, weights=(1.0, 1.0, 1.0, 1.0), clip=math.log(1000.0 / 16)):
    """mv_retinanet_decode_f32 for idx (N, K): boxes (N, K, 4), scores (N, K), labels (N, K) int64, valid (N, K) bool; anchors: per
    image the (total, 4) anchors of all levels."""
    coder = BoxCoder(weights, clip, numerics=RESTATEMENT)
    cls = torch.cat([permute_level(m, num_classes) for m in cls_maps], 1)  # (N, total, K)
    reg = torch.cat([permute_level(m, 4) for m in reg_maps], 1)
    total = cls.shape[1]
    boxes, scores, labels, valid = [], [], [], []
    for i in range(idx.shape[0]):
        f = idx[i].long()
        ok = (f >= 0) & (f < total * num_classes)
        g = torch.where(ok, f, torch.zeros_like(f))
        a, c = torch.div(g, num_classes, rounding_mode="floor"), g % num_classes
        b = coder.decode_single(reg[i][a], anchors[i][a]).reshape(-1, 4)
        b = clip_boxes_to_image(b, image_sizes[i])
        s = sigmoid_cr(cls[i][a, c])
        boxes.append(torch.where(ok[:, None], b, torch.zeros_like(b)))
        scores.append(torch.where(ok, s, torch.zeros_like(s)))
        labels.append(torch.where(ok, c, torch.zeros_like(c)))
        valid.append(ok)
    return torch.stack(boxes), torch.stack(scores), torch.stack(labels), torch.stack(valid)
