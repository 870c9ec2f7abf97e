"""References for the FCOS tests (a helper module, not a test file and not a conftest).  Imports nothing from the package.

(a) A plain-torch replica of the reference's models/detection/fcos.py and _utils.py::BoxLinearCoder.decode (torchvision is not
    importable in the test environment), like tests/_retinanet_ref.py: FCOSClassificationHead, FCOSRegressionHead, FCOSHead and FCOS
    with the same constructor arguments, child names, construction order and initialisation, torch's own convs, nn.GroupNorm,
    torch.sigmoid, torch.sqrt and torch.topk.  AnchorGenerator, batched_nms, Transform and `same` are those of tests/_rpn_ref.py and
    tests/_retinanet_ref.py.
(b) The restatement the library is compared with bit for bit:
      group_norm_act  -> `group_norm`: mv_group_norm_act_f32's stated order of the float64 sums (numpy reshapes and adds) and its
                         float32 chain, one rounding per operation
      score           -> sqrt_cr(sigmoid_cr(cls) * sigmoid_cr(ctr)) in float32 (`score`): sigmoid_cr as in tests/_rpn_ref.py, sqrt_cr the
                         correctly rounded float32 square root (torch.sqrt on float32 is a 1-ulp vector routine on the CPU)
      `> thresh`, topk-> the strict float32 comparison and the first k of the stable descending sort, as tests/_retinanet_ref.py
      decode          -> BoxLinearCoder.decode operation by operation on max(r, 0) (`linear_decode`)
    and, for the two kernels' own outputs, `select` / `decode`: the fixed-shape (N, Ktot) form with -1 padding.
"""
import math
from collections import OrderedDict
from functools import partial

import numpy as np
import torch
from torch import nn

from tests._retinanet_ref import Transform, permute_level
from tests._rpn_ref import (AnchorGenerator, Numerics, REPLICA, RESTATEMENT, batched_nms, clip_boxes_to_image, same,  # noqa: F401
                            sigmoid_cr)

GN_CHUNK = 4096  # mv_group_norm_chunk(): the tests assert that the library reports this


# ------------------------------------------------------------------------------------------------ (b) GroupNorm
def _fold(a):
    """(..., 64) -> (...): a[l] += a[l ^ 32], then ^ 16, 8, 4, 2, 1 -- lane 0's value."""
    for half in (32, 16, 8, 4, 2, 1):
        a = a.reshape(a.shape[:-1] + (2, half))
        a = a[..., 0, :] + a[..., 1, :]
    return a[..., 0]


def group_sums(slabs):
    """slabs (S, m) float32 -> (sum x, sum x^2) float64 (S,) in the order mv_group_norm_act_f32 states."""
    s_, m = slabs.shape
    chunks = -(-m // GN_CHUNK)
    pad = np.zeros((s_, chunks * GN_CHUNK), dtype=np.float64)
    pad[:, :m] = slabs
    v = pad.reshape(s_, chunks, 4, 256, 4)  # element 1024 u + 4 t + q of a chunk at [u, t, q]
    s, s2 = np.zeros((s_, chunks, 256)), np.zeros((s_, chunks, 256))
    for u in range(4):
        for q in range(4):
            d = v[:, :, u, :, q]
            s = s + d
            s2 = s2 + d * d
    out = []
    for a in (s, s2):
        w = _fold(a.reshape(s_, chunks, 4, 64))  # (S, chunks, 4 waves)
        c = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
        total = np.zeros(s_)
        for j in range(chunks):
            total = total + c[:, j]
        out.append(total)
    return out[0], out[1]


def group_norm(x, num_groups, weight=None, bias=None, eps=1e-5, relu=False):
    """mv_group_norm_act_f32 restated: x (N, C, H, W) float32 tensor -> tensor."""
    n, c, h, w = x.shape
    xs = x.detach().contiguous().numpy()
    m = (c // num_groups) * h * w
    with np.errstate(all="ignore"):
        slabs = xs.reshape(n * num_groups, m)
        S, S2 = group_sums(slabs)
        dm = np.float64(m)
        mean = S / dm
        var = S2 / dm - mean * mean
        var = np.where(var < 0, 0.0, var)
        rstd = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
        mean32, rstd32 = mean.astype(np.float32)[:, None], rstd.astype(np.float32)[:, None]
        y = ((slabs - mean32) * rstd32).astype(np.float32).reshape(n, c, h * w)
        assert y.dtype == np.float32
        if weight is not None:
            y = y * weight.detach().numpy().astype(np.float32)[None, :, None]
        if bias is not None:
            y = y + bias.detach().numpy().astype(np.float32)[None, :, None]
        if relu:
            y = np.where(y < 0, np.float32(0), y)
    assert y.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(y.reshape(n, c, h, w)))


# ------------------------------------------------------------------------------------------------ (a) the torch replica
class BoxLinearCoder:
    def __init__(self, normalize_by_size=True):
        self.normalize_by_size = normalize_by_size

    def decode(self, rel_codes, boxes):
        boxes = boxes.to(dtype=rel_codes.dtype)
        ctr_x = 0.5 * (boxes[..., 0] + boxes[..., 2])
        ctr_y = 0.5 * (boxes[..., 1] + boxes[..., 3])
        if self.normalize_by_size:
            boxes_w = boxes[..., 2] - boxes[..., 0]
            boxes_h = boxes[..., 3] - boxes[..., 1]
            list_box_size = torch.stack((boxes_w, boxes_h, boxes_w, boxes_h), dim=-1)
            rel_codes = rel_codes * list_box_size
        pred_boxes1 = ctr_x - rel_codes[..., 0]
        pred_boxes2 = ctr_y - rel_codes[..., 1]
        pred_boxes3 = ctr_x + rel_codes[..., 2]
        pred_boxes4 = ctr_y + rel_codes[..., 3]
        return torch.stack((pred_boxes1, pred_boxes2, pred_boxes3, pred_boxes4), dim=-1)


class FCOSClassificationHead(nn.Module):
    def __init__(self, in_channels, num_anchors, num_classes, num_convs=4, prior_probability=0.01, norm_layer=None):
        super().__init__()
        self.num_classes = num_classes
        self.num_anchors = num_anchors
        if norm_layer is None:
            norm_layer = partial(nn.GroupNorm, 32)
        conv = []
        for _ in range(num_convs):
            conv.append(nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1))
            conv.append(norm_layer(in_channels))
            conv.append(nn.ReLU())
        self.conv = nn.Sequential(*conv)
        for layer in self.conv.children():
            if isinstance(layer, nn.Conv2d):
                torch.nn.init.normal_(layer.weight, std=0.01)
                torch.nn.init.constant_(layer.bias, 0)
        self.cls_logits = nn.Conv2d(in_channels, num_anchors * num_classes, kernel_size=3, stride=1, padding=1)
        torch.nn.init.normal_(self.cls_logits.weight, std=0.01)
        torch.nn.init.constant_(self.cls_logits.bias, -math.log((1 - prior_probability) / prior_probability))

    def maps(self, x):
        return [self.cls_logits(self.conv(features)) for features in x]

    def forward(self, x):
        return torch.cat([permute_level(m, self.num_classes) for m in self.maps(x)], dim=1)


class FCOSRegressionHead(nn.Module):
    def __init__(self, in_channels, num_anchors, num_convs=4, norm_layer=None):
        super().__init__()
        if norm_layer is None:
            norm_layer = partial(nn.GroupNorm, 32)
        conv = []
        for _ in range(num_convs):
            conv.append(nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1))
            conv.append(norm_layer(in_channels))
            conv.append(nn.ReLU())
        self.conv = nn.Sequential(*conv)
        self.bbox_reg = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=3, stride=1, padding=1)
        self.bbox_ctrness = nn.Conv2d(in_channels, num_anchors * 1, kernel_size=3, stride=1, padding=1)
        for layer in [self.bbox_reg, self.bbox_ctrness]:
            torch.nn.init.normal_(layer.weight, std=0.01)
            torch.nn.init.zeros_(layer.bias)
        for layer in self.conv.children():
            if isinstance(layer, nn.Conv2d):
                torch.nn.init.normal_(layer.weight, std=0.01)
                torch.nn.init.zeros_(layer.bias)

    def maps(self, x):
        reg, ctr = [], []
        for features in x:
            t = self.conv(features)
            reg.append(nn.functional.relu(self.bbox_reg(t)))
            ctr.append(self.bbox_ctrness(t))
        return reg, ctr

    def forward(self, x):
        reg, ctr = self.maps(x)
        return torch.cat([permute_level(m, 4) for m in reg], dim=1), torch.cat([permute_level(m, 1) for m in ctr], dim=1)


class FCOSHead(nn.Module):
    def __init__(self, in_channels, num_anchors, num_classes, num_convs=4):
        super().__init__()
        self.box_coder = BoxLinearCoder(normalize_by_size=True)
        self.classification_head = FCOSClassificationHead(in_channels, num_anchors, num_classes, num_convs)
        self.regression_head = FCOSRegressionHead(in_channels, num_anchors, num_convs)

    def forward(self, x):
        cls_logits = self.classification_head(x)
        bbox_regression, bbox_ctrness = self.regression_head(x)
        return {"cls_logits": cls_logits, "bbox_regression": bbox_regression, "bbox_ctrness": bbox_ctrness}


def default_anchorgen():
    return AnchorGenerator(((8,), (16,), (32,), (64,), (128,)), ((1.0,),) * 5)


class FCOS(nn.Module):
    """fcos.py FCOS, the inference path; `numerics` picks (a) or (b) for the sigmoid and the topk."""

    def __init__(self, backbone, num_classes, min_size=800, max_size=1333, image_mean=None, image_std=None, anchor_generator=None, head=None,
                 center_sampling_radius=1.5, score_thresh=0.2, nms_thresh=0.6, detections_per_img=100, topk_candidates=1000,
                 numerics=REPLICA):
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
        if self.anchor_generator.num_anchors_per_location()[0] != 1:
            raise ValueError(f"anchor_generator.num_anchors_per_location()[0] should be 1 instead of "
                             f"{anchor_generator.num_anchors_per_location()[0]}")
        if head is None:
            head = FCOSHead(backbone.out_channels, anchor_generator.num_anchors_per_location()[0], num_classes)
        self.head = head
        self.numerics = numerics
        self.box_coder = BoxLinearCoder(normalize_by_size=True)
        if image_mean is None:
            image_mean = [0.485, 0.456, 0.406]
        if image_std is None:
            image_std = [0.229, 0.224, 0.225]
        self.transform = Transform(image_mean, image_std)
        self.center_sampling_radius = center_sampling_radius
        self.score_thresh = score_thresh
        self.nms_thresh = nms_thresh
        self.detections_per_img = detections_per_img
        self.topk_candidates = topk_candidates

    def postprocess_detections(self, head_outputs, anchors, image_shapes, detailed=False):
        """head_outputs / anchors: per level lists, as the reference splits them."""
        class_logits = head_outputs["cls_logits"]
        box_regression = head_outputs["bbox_regression"]
        box_ctrness = head_outputs["bbox_ctrness"]
        num_images = len(image_shapes)
        detections, candidates = [], []
        for index in range(num_images):
            box_regression_per_image = [br[index] for br in box_regression]
            logits_per_image = [cl[index] for cl in class_logits]
            box_ctrness_per_image = [bc[index] for bc in box_ctrness]
            anchors_per_image, image_shape = anchors[index], image_shapes[index]
            image_boxes, image_scores, image_labels, image_flat = [], [], [], []
            start = 0
            for box_regression_per_level, logits_per_level, box_ctrness_per_level, anchors_per_level in zip(
                    box_regression_per_image, logits_per_image, box_ctrness_per_image, anchors_per_image):
                num_classes = logits_per_level.shape[-1]
                # remove low scoring boxes
                sqrt = torch.sqrt if self.numerics is REPLICA else sqrt_cr
                scores_per_level = sqrt(self.numerics.sigmoid(logits_per_level) * self.numerics.sigmoid(box_ctrness_per_level)).flatten()
                keep_idxs = scores_per_level > self.score_thresh
                scores_per_level = scores_per_level[keep_idxs]
                topk_idxs = torch.where(keep_idxs)[0]
                # keep only topk scoring predictions
                num_topk = min(topk_idxs.size(0), self.topk_candidates)
                idxs = self.numerics.topk(scores_per_level[None], num_topk)[0]
                scores_per_level = scores_per_level[idxs]
                topk_idxs = topk_idxs[idxs]
                anchor_idxs = torch.div(topk_idxs, num_classes, rounding_mode="floor")
                labels_per_level = topk_idxs % num_classes
                boxes_per_level = self.box_coder.decode(box_regression_per_level[anchor_idxs], anchors_per_level[anchor_idxs])
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

    def from_head_maps(self, images, cls_maps, reg_maps, ctr_maps, detailed=False):
        """forward from the heads' per-level NCHW maps on (CPU tensors); reg_maps are rectified (the head's ReLU)."""
        num_classes = cls_maps[0].shape[1]
        anchors = self.anchor_generator(images, cls_maps)
        per_level = [int(m.shape[2] * m.shape[3]) for m in cls_maps]
        head_outputs = {"cls_logits": [permute_level(m, num_classes) for m in cls_maps], "bbox_regression": [permute_level(m, 4) for m in reg_maps],
                        "bbox_ctrness": [permute_level(m, 1) for m in ctr_maps]}
        split_anchors = [list(a.split(per_level)) for a in anchors]
        return self.postprocess_detections(head_outputs, split_anchors, images.image_sizes, detailed)

    def forward(self, images):
        images = self.transform(images)
        features = self.backbone(images.tensors)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        features = list(features.values())
        cls_maps = self.head.classification_head.maps(features)
        reg_maps, ctr_maps = self.head.regression_head.maps(features)
        return self.from_head_maps(images, cls_maps, reg_maps, ctr_maps)


# ------------------------------------------------------------------------------------------------ (b) what the two kernels write
def sqrt_cr(v):
    """The correctly rounded float32 square root, through float64 (53 >= 2 * 24 + 2 bits: the second rounding is innocuous).  torch's
    CPU float32 sqrt is a vector routine that misses it by one ulp on about a sixth of the scores, like its exp (tests/_rpn_ref.py)."""
    return torch.sqrt(v.double()).to(v.dtype)


def score(cls, ctr):
    """sqrt_cr(fl(sigmoid_cr(cls) * sigmoid_cr(ctr))) in float32, ctr broadcast over the classes."""
    return sqrt_cr(sigmoid_cr(cls) * sigmoid_cr(ctr))


def level_scores(cls_map, ctr_map, num_classes):
    """(N, K, H, W), (N, 1, H, W) -> (N, HW K): the scores in the flat order position * K + class."""
    return score(permute_level(cls_map, num_classes), permute_level(ctr_map, 1)).flatten(1)


def select(cls_maps, ctr_maps, num_classes, k, score_thresh):
    """mv_fcos_topk_f32: (N, Ktot) int32, per (image, level) the flat indices of the min(k, passing) greatest scores in stable
    descending order, then -1."""
    thresh = torch.tensor(score_thresh, dtype=torch.float32)
    out, start = [], 0
    for m, c in zip(cls_maps, ctr_maps):
        s = level_scores(m, c, num_classes)
        passing = s > thresh  # strict, float32; a NaN does not pass
        seg = min(k, s.shape[1])
        order = torch.sort(torch.where(passing, s, torch.full_like(s, -1.0)), dim=1, stable=True, descending=True)[1][:, :seg]
        taken = torch.arange(seg)[None, :] < passing.sum(1, keepdim=True)
        out.append(torch.where(taken, order + start, torch.full_like(order, -1)))
        start += s.shape[1]
    return torch.cat(out, 1).to(torch.int32)


def linear_decode(r, anchors):
    """BoxLinearCoder(normalize_by_size=True).decode of max(r, 0), operation by operation: r, anchors (M, 4) float32."""
    r = torch.where(r < 0, torch.zeros_like(r), r)  # a NaN stays
    x1, y1, x2, y2 = anchors.unbind(1)
    half = torch.tensor(0.5)
    cx, cy = half * (x1 + x2), half * (y1 + y2)
    w, h = x2 - x1, y2 - y1
    return torch.stack((cx - r[:, 0] * w, cy - r[:, 1] * h, cx + r[:, 2] * w, cy + r[:, 3] * h), dim=1)


def decode(cls_maps, ctr_maps, reg_maps, idx, anchors, image_sizes, num_classes):
    """mv_fcos_decode_f32 for idx (N, K): boxes (N, K, 4), scores (N, K), labels (N, K) int64, valid (N, K) bool; anchors: per image
    the (total, 4) anchors of all levels."""
    cls = torch.cat([permute_level(m, num_classes) for m in cls_maps], 1)  # (N, total, K)
    ctr = torch.cat([permute_level(m, 1) for m in ctr_maps], 1)[..., 0]   # (N, total)
    reg = torch.cat([permute_level(m, 4) for m in reg_maps], 1)
    total = cls.shape[1]
    boxes, scores, labels, valid = [], [], [], []
    for i in range(idx.shape[0]):
        f = idx[i].long()
        ok = (f >= 0) & (f < total * num_classes)
        g = torch.where(ok, f, torch.zeros_like(f))
        a, c = torch.div(g, num_classes, rounding_mode="floor"), g % num_classes
        b = clip_boxes_to_image(linear_decode(reg[i][a], anchors[i][a]), image_sizes[i])
        s = score(cls[i][a, c], ctr[i][a])
        boxes.append(torch.where(ok[:, None], b, torch.zeros_like(b)))
        scores.append(torch.where(ok, s, torch.zeros_like(s)))
        labels.append(torch.where(ok, c, torch.zeros_like(c)))
        valid.append(ok)
    return torch.stack(boxes), torch.stack(scores), torch.stack(labels), torch.stack(valid)
