"""References for the RoIHeads / Faster R-CNN tests (a helper module, not a test file and not a conftest).  Imports nothing from the
package.

(a) A plain-torch replica of the reference's models/detection/roi_heads.py (inference path), faster_rcnn.py, generalized_rcnn.py and
    transform.py (torchvision is not importable in the test environment), written from the reference's source like
    tests/_rpn_ref.py, on whose replicas (AnchorGenerator, RPNHead, RegionProposalNetwork, BoxCoder, clip_boxes_to_image,
    batched_nms) and tests/_fpn_ref.py's backbones it is built: the same classes, constructor arguments, child names, construction
    order and initialisation, with torch's own forward, torch.softmax and torch.exp.  Its pooler is ops/poolers.py's per-level loop
    over tests/_detect_ref.roi_align_ref (tests/_boxes_ref.multiscale_ref).
(b) The restatement the library is compared with bit for bit: (a) with exactly two substitutions (`Numerics`),
      exp(v)      -> torch.exp(v.double()).float()     the correctly rounded float32 exp (tests/_rpn_ref.exp_cr)
      softmax(x)  -> m = max_j x_j; e_j = E(x_j - m); s = ((e_0 + e_1) + e_2) + ... as a Python loop over the columns, one float32
                     add each, the background included; e_j / s
    torch's CPU softmax uses a 1-ulp vector exp and a summation order that depends on the vector width, so no kernel can reproduce
    (a) bit for bit; (b) is what mi355vision.h states (mv_roi_detections_f32).
"""
import math
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from tests import _boxes_ref as B
from tests import _fpn_ref as FP
from tests import _resnet_ref as R
from tests import _rpn_ref as P

BoxCoder, clip_boxes_to_image, batched_nms, same = P.BoxCoder, P.clip_boxes_to_image, P.batched_nms, P.same


# ------------------------------------------------------------------------------------------------ the two substitutions
def softmax_torch(x):
    return torch.softmax(x, -1)


def softmax_chain(x):
    """max, E, ONE ascending float32 chain over the columns, the divide."""
    m = x.max(dim=1, keepdim=True)[0]
    e = P.exp_cr(x - m)
    s = e[:, 0].clone()
    for j in range(1, x.shape[1]):
        s = s + e[:, j]
    return e / s[:, None]


class Numerics:
    def __init__(self, exp, softmax, rpn):
        self.exp, self.softmax, self.rpn = exp, softmax, rpn


REPLICA = Numerics(torch.exp, softmax_torch, P.REPLICA)
RESTATEMENT = Numerics(P.exp_cr, softmax_chain, P.RESTATEMENT)


# ------------------------------------------------------------------------------------------------ the torch replica
class MultiScaleRoIAlign(nn.Module):
    """ops/poolers.py MultiScaleRoIAlign on CPU tensors: the per-level loop over roi_align_ref."""

    def __init__(self, featmap_names, output_size, sampling_ratio, *, canonical_scale=224, canonical_level=4):
        super().__init__()
        if isinstance(output_size, int):
            output_size = (output_size, output_size)
        self.featmap_names = featmap_names
        self.sampling_ratio = sampling_ratio
        self.output_size = tuple(output_size)
        self.scales = None
        self.k_min = self.k_max = None
        self.canonical_scale = canonical_scale
        self.canonical_level = canonical_level

    def setup_scales(self, features, image_shapes):
        max_x = max(s[0] for s in image_shapes)
        max_y = max(s[1] for s in image_shapes)
        # _infer_scale: the first axis decides
        self.scales = [2 ** float(torch.tensor(float(f.shape[-2]) / float(max_x)).log2().round()) for f in features]
        del max_y
        self.k_min = int(-torch.log2(torch.tensor(self.scales[0], dtype=torch.float32)).item())
        self.k_max = int(-torch.log2(torch.tensor(self.scales[-1], dtype=torch.float32)).item())

    def levels(self, boxes):
        area = torch.cat([(b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) for b in boxes])
        s = torch.sqrt(area)
        target = torch.floor(self.canonical_level + torch.log2(s / self.canonical_scale) + torch.tensor(1e-6, dtype=s.dtype))
        target = torch.clamp(target, min=self.k_min, max=self.k_max)
        return (target.to(torch.int64) - self.k_min).to(torch.int64)

    def forward(self, x, boxes, image_shapes):
        feats = [v for k, v in x.items() if k in self.featmap_names]
        if self.scales is None:
            self.setup_scales(feats, image_shapes)
        rois = torch.cat([torch.cat([torch.full_like(b[:, :1], i), b], 1) for i, b in enumerate(boxes)])
        if len(feats) == 1:
            from tests import _detect_ref as D
            out = D.roi_align_ref(feats[0].detach().numpy(), rois.detach().numpy(), self.output_size, self.scales[0], self.sampling_ratio, False)
        else:
            out = B.multiscale_ref([f.detach().numpy() for f in feats], rois.detach().numpy(), self.levels(boxes).detach().numpy(), self.scales, self.output_size,
                                   self.sampling_ratio)
        return torch.from_numpy(out)


class TwoMLPHead(nn.Module):
    def __init__(self, in_channels, representation_size):
        super().__init__()
        self.fc6 = nn.Linear(in_channels, representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)

    def forward(self, x):
        x = x.flatten(start_dim=1)
        x = nn.functional.relu(self.fc6(x))
        x = nn.functional.relu(self.fc7(x))
        return x


class FastRCNNPredictor(nn.Module):
    def __init__(self, in_channels, num_classes):
        super().__init__()
        self.cls_score = nn.Linear(in_channels, num_classes)
        self.bbox_pred = nn.Linear(in_channels, num_classes * 4)

    def forward(self, x):
        if x.dim() == 4:
            torch._assert(list(x.shape[2:]) == [1, 1],
                          f"x has the wrong shape, expecting the last two dimensions to be [1,1] instead of {list(x.shape[2:])}")
        x = x.flatten(start_dim=1)
        scores = self.cls_score(x)
        bbox_deltas = self.bbox_pred(x)
        return scores, bbox_deltas


def remove_small_boxes(boxes, min_size):
    return P.remove_small_boxes(boxes, min_size)


class RoIHeads(nn.Module):
    """roi_heads.py:496-876, the inference path of the box branch (no matcher, sampler or losses); `numerics` picks (a) or (b)."""

    def __init__(self, box_roi_pool, box_head, box_predictor, fg_iou_thresh, bg_iou_thresh, batch_size_per_image, positive_fraction,
                 bbox_reg_weights, score_thresh, nms_thresh, detections_per_img, mask_roi_pool=None, mask_head=None, mask_predictor=None,
                 keypoint_roi_pool=None, keypoint_head=None, keypoint_predictor=None, numerics=REPLICA):
        super().__init__()
        self.numerics = numerics
        if bbox_reg_weights is None:
            bbox_reg_weights = (10.0, 10.0, 5.0, 5.0)
        self.box_coder = BoxCoder(bbox_reg_weights, numerics=numerics)
        self.box_roi_pool = box_roi_pool
        self.box_head = box_head
        self.box_predictor = box_predictor
        self.score_thresh = score_thresh
        self.nms_thresh = nms_thresh
        self.detections_per_img = detections_per_img
        self.mask_roi_pool, self.mask_head, self.mask_predictor = mask_roi_pool, mask_head, mask_predictor
        self.keypoint_roi_pool, self.keypoint_head, self.keypoint_predictor = keypoint_roi_pool, keypoint_head, keypoint_predictor

    def dense(self, class_logits, box_regression, proposals, image_shapes, min_size=1e-2):
        """postprocess_detections up to the filters -> boxes (R, C - 1, 4), scores (R, C - 1), labels (R, C - 1), valid (R, C - 1):
        what mv_roi_detections_f32 writes."""
        num_classes = class_logits.shape[-1]
        boxes_per_image = [b.shape[0] for b in proposals]
        pred_boxes = self.box_coder.decode(box_regression, proposals)
        pred_scores = self.numerics.softmax(class_logits)
        all_boxes, all_scores, all_labels, all_valid = [], [], [], []
        for boxes, scores, image_shape in zip(pred_boxes.split(boxes_per_image, 0), pred_scores.split(boxes_per_image, 0), image_shapes):
            boxes = clip_boxes_to_image(boxes, image_shape)
            labels = torch.arange(num_classes, device=class_logits.device)
            labels = labels.view(1, -1).expand_as(scores)
            # remove predictions with the background label
            boxes, scores, labels = boxes[:, 1:], scores[:, 1:], labels[:, 1:]
            ws, hs = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
            all_valid.append((scores > self.score_thresh) & (ws >= min_size) & (hs >= min_size))
            all_boxes.append(boxes), all_scores.append(scores), all_labels.append(labels)
        return torch.cat(all_boxes), torch.cat(all_scores), torch.cat(all_labels), torch.cat(all_valid)

    def postprocess_detections(self, class_logits, box_regression, proposals, image_shapes):
        num_classes = class_logits.shape[-1]
        boxes_per_image = [boxes_in_image.shape[0] for boxes_in_image in proposals]
        pred_boxes = self.box_coder.decode(box_regression, proposals)
        pred_scores = self.numerics.softmax(class_logits)
        pred_boxes_list = pred_boxes.split(boxes_per_image, 0)
        pred_scores_list = pred_scores.split(boxes_per_image, 0)
        all_boxes, all_scores, all_labels = [], [], []
        for boxes, scores, image_shape in zip(pred_boxes_list, pred_scores_list, image_shapes):
            boxes = clip_boxes_to_image(boxes, image_shape)
            # create labels for each prediction
            labels = torch.arange(num_classes, device=class_logits.device)
            labels = labels.view(1, -1).expand_as(scores)
            # remove predictions with the background label
            boxes = boxes[:, 1:]
            scores = scores[:, 1:]
            labels = labels[:, 1:]
            # batch everything, by making every class prediction be a separate instance
            boxes = boxes.reshape(-1, 4)
            scores = scores.reshape(-1)
            labels = labels.reshape(-1)
            # remove low scoring boxes
            inds = torch.where(scores > self.score_thresh)[0]
            boxes, scores, labels = boxes[inds], scores[inds], labels[inds]
            # remove empty boxes
            keep = remove_small_boxes(boxes, min_size=1e-2)
            boxes, scores, labels = boxes[keep], scores[keep], labels[keep]
            # non-maximum suppression, independently done per class
            keep = batched_nms(boxes, scores, labels, self.nms_thresh)
            # keep only topk scoring predictions
            keep = keep[:self.detections_per_img]
            boxes, scores, labels = boxes[keep], scores[keep], labels[keep]
            all_boxes.append(boxes)
            all_scores.append(scores)
            all_labels.append(labels)
        return all_boxes, all_scores, all_labels

    def forward(self, features, proposals, image_shapes, targets=None):
        box_features = self.box_roi_pool(features, proposals, image_shapes)
        box_features = self.box_head(box_features)
        class_logits, box_regression = self.box_predictor(box_features)
        result = []
        boxes, scores, labels = self.postprocess_detections(class_logits, box_regression, proposals, image_shapes)
        for i in range(len(boxes)):
            result.append({"boxes": boxes[i], "labels": labels[i], "scores": scores[i]})
        return result, {}


def resize_boxes(boxes, original_size, new_size):
    ratios = [torch.tensor(s, dtype=torch.float32, device=boxes.device) / torch.tensor(s_orig, dtype=torch.float32, device=boxes.device)
              for s, s_orig in zip(new_size, original_size)]
    ratio_height, ratio_width = ratios
    xmin, ymin, xmax, ymax = boxes.unbind(1)
    xmin = xmin * ratio_width
    xmax = xmax * ratio_width
    ymin = ymin * ratio_height
    ymax = ymax * ratio_height
    return torch.stack((xmin, ymin, xmax, ymax), dim=1)


class GeneralizedRCNNTransform(nn.Module):
    """transform.py:78-285 for inference.  `_skip_resize` skips the resize in either mode (the reference: in training mode only),
    which is how the library takes it; without it the reference's non-antialiased bilinear interpolate runs."""

    def __init__(self, min_size, max_size, image_mean, image_std, size_divisible=32, fixed_size=None, **kwargs):
        super().__init__()
        if not isinstance(min_size, (list, tuple)):
            min_size = (min_size,)
        self.min_size = min_size
        self.max_size = max_size
        self.image_mean = image_mean
        self.image_std = image_std
        self.size_divisible = size_divisible
        self.fixed_size = fixed_size
        self._skip_resize = kwargs.pop("_skip_resize", False)

    def forward(self, images, targets=None):
        images = [img for img in images]
        for i in range(len(images)):
            image = images[i]
            if image.dim() != 3:
                raise ValueError(f"images is expected to be a list of 3d tensors of shape [C, H, W], got {image.shape}")
            image = self.normalize(image)
            image = self.resize(image)
            images[i] = image
        image_sizes = [img.shape[-2:] for img in images]
        images = self.batch_images(images, size_divisible=self.size_divisible)
        image_sizes_list = []
        for image_size in image_sizes:
            torch._assert(len(image_size) == 2, f"Input tensors expected to have in the last two elements H and W, instead got {image_size}")
            image_sizes_list.append((image_size[0], image_size[1]))
        return P.ImageList(images, image_sizes_list), targets

    def normalize(self, image):
        if not image.is_floating_point():
            raise TypeError(f"Expected input images to be of floating type (in range [0, 1]), but found type {image.dtype} instead")
        dtype, device = image.dtype, image.device
        mean = torch.as_tensor(self.image_mean, dtype=dtype, device=device)
        std = torch.as_tensor(self.image_std, dtype=dtype, device=device)
        return (image - mean[:, None, None]) / std[:, None, None]

    def resize(self, image):
        if self._skip_resize:
            return image
        size = self.min_size[-1]
        if self.fixed_size is not None:
            return nn.functional.interpolate(image[None], size=[self.fixed_size[1], self.fixed_size[0]], mode="bilinear", align_corners=False)[0]
        im_shape = torch.tensor(image.shape[-2:])
        min_size = torch.min(im_shape).to(dtype=torch.float32)
        max_size = torch.max(im_shape).to(dtype=torch.float32)
        scale_factor = torch.min(size / min_size, self.max_size / max_size).item()
        return nn.functional.interpolate(image[None], scale_factor=scale_factor, mode="bilinear", recompute_scale_factor=True,
                                         align_corners=False)[0]

    def max_by_axis(self, the_list):
        maxes = the_list[0]
        for sublist in the_list[1:]:
            for index, item in enumerate(sublist):
                maxes[index] = max(maxes[index], item)
        return maxes

    def batch_images(self, images, size_divisible=32):
        max_size = self.max_by_axis([list(img.shape) for img in images])
        stride = float(size_divisible)
        max_size = list(max_size)
        max_size[1] = int(math.ceil(float(max_size[1]) / stride) * stride)
        max_size[2] = int(math.ceil(float(max_size[2]) / stride) * stride)
        batch_shape = [len(images)] + max_size
        batched_imgs = images[0].new_full(batch_shape, 0)
        for i in range(batched_imgs.shape[0]):
            img = images[i]
            batched_imgs[i, : img.shape[0], : img.shape[1], : img.shape[2]].copy_(img)
        return batched_imgs

    def postprocess(self, result, image_shapes, original_image_sizes):
        if self.training:
            return result
        for i, (pred, im_s, o_im_s) in enumerate(zip(result, image_shapes, original_image_sizes)):
            boxes = pred["boxes"]
            boxes = resize_boxes(boxes, im_s, o_im_s)
            result[i]["boxes"] = boxes
        return result


class GeneralizedRCNN(nn.Module):
    def __init__(self, backbone, rpn, roi_heads, transform):
        super().__init__()
        self.transform = transform
        self.backbone = backbone
        self.rpn = rpn
        self.roi_heads = roi_heads
        self._has_warned = False

    def forward(self, images, targets=None):
        original_image_sizes = []
        for img in images:
            val = img.shape[-2:]
            torch._assert(len(val) == 2, f"expecting the last two dimensions of the Tensor to be H and W instead got {img.shape[-2:]}")
            original_image_sizes.append((val[0], val[1]))
        images, targets = self.transform(images, targets)
        features = self.backbone(images.tensors)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        proposals, _ = self.rpn(images, features, targets)
        detections, _ = self.roi_heads(features, proposals, images.image_sizes, targets)
        return self.transform.postprocess(detections, images.image_sizes, original_image_sizes)


def _default_anchorgen():
    anchor_sizes = ((32,), (64,), (128,), (256,), (512,))
    aspect_ratios = ((0.5, 1.0, 2.0),) * len(anchor_sizes)
    return P.AnchorGenerator(anchor_sizes, aspect_ratios)


class FasterRCNN(GeneralizedRCNN):
    def __init__(self, backbone, num_classes=None, min_size=800, max_size=1333, image_mean=None, image_std=None, rpn_anchor_generator=None,
                 rpn_head=None, rpn_pre_nms_top_n_train=2000, rpn_pre_nms_top_n_test=1000, rpn_post_nms_top_n_train=2000,
                 rpn_post_nms_top_n_test=1000, rpn_nms_thresh=0.7, rpn_fg_iou_thresh=0.7, rpn_bg_iou_thresh=0.3,
                 rpn_batch_size_per_image=256, rpn_positive_fraction=0.5, rpn_score_thresh=0.0, box_roi_pool=None, box_head=None,
                 box_predictor=None, box_score_thresh=0.05, box_nms_thresh=0.5, box_detections_per_img=100, box_fg_iou_thresh=0.5,
                 box_bg_iou_thresh=0.5, box_batch_size_per_image=512, box_positive_fraction=0.25, bbox_reg_weights=None, numerics=REPLICA,
                 **kwargs):
        if not hasattr(backbone, "out_channels"):
            raise ValueError("backbone should contain an attribute out_channels "
                             "specifying the number of output channels (assumed to be the "
                             "same for all the levels)")
        if not isinstance(rpn_anchor_generator, (P.AnchorGenerator, type(None))):
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
            rpn_head = P.RPNHead(out_channels, rpn_anchor_generator.num_anchors_per_location()[0])
        rpn_pre_nms_top_n = dict(training=rpn_pre_nms_top_n_train, testing=rpn_pre_nms_top_n_test)
        rpn_post_nms_top_n = dict(training=rpn_post_nms_top_n_train, testing=rpn_post_nms_top_n_test)
        rpn = P.RegionProposalNetwork(rpn_anchor_generator, rpn_head, rpn_fg_iou_thresh, rpn_bg_iou_thresh, rpn_batch_size_per_image,
                                      rpn_positive_fraction, rpn_pre_nms_top_n, rpn_post_nms_top_n, rpn_nms_thresh,
                                      score_thresh=rpn_score_thresh, numerics=numerics.rpn)
        if box_roi_pool is None:
            box_roi_pool = MultiScaleRoIAlign(featmap_names=["0", "1", "2", "3"], output_size=7, sampling_ratio=2)
        if box_head is None:
            resolution = box_roi_pool.output_size[0]
            representation_size = 1024
            box_head = TwoMLPHead(out_channels * resolution**2, representation_size)
        if box_predictor is None:
            representation_size = 1024
            box_predictor = FastRCNNPredictor(representation_size, num_classes)
        roi_heads = RoIHeads(box_roi_pool, box_head, box_predictor, box_fg_iou_thresh, box_bg_iou_thresh, box_batch_size_per_image,
                             box_positive_fraction, bbox_reg_weights, box_score_thresh, box_nms_thresh, box_detections_per_img,
                             numerics=numerics)
        if image_mean is None:
            image_mean = [0.485, 0.456, 0.406]
        if image_std is None:
            image_std = [0.229, 0.224, 0.225]
        transform = GeneralizedRCNNTransform(min_size, max_size, image_mean, image_std, **kwargs)
        super().__init__(backbone, rpn, roi_heads, transform)


def fasterrcnn_resnet50_fpn(*, weights=None, progress=True, num_classes=None, weights_backbone=None, trainable_backbone_layers=None,
                            **kwargs):
    """faster_rcnn.py:459-571 without weight files, on a FrozenBatchNorm2d backbone (what the library builds)."""
    assert weights is None and weights_backbone is None
    if num_classes is None:
        num_classes = 91
    backbone = R.resnet50(norm_layer=FP.FrozenBatchNorm2d)
    backbone = FP._resnet_fpn_extractor(backbone, 5 if trainable_backbone_layers is None else trainable_backbone_layers)
    return FasterRCNN(backbone, num_classes=num_classes, **kwargs)


# ------------------------------------------------------------------------------------------------ helpers of the tests
def score_bound(classes):
    """The relative distance allowed between torch's CPU softmax and the restatement, which differ in a 1-ulp-or-better exp, in the
    order of the sum and in how they normalise (derived in tests/test_roi_heads_host.py): (2 C + 7) 2^-24."""
    return (2 * classes + 7) * 2.0 ** -24


def np_same(got, want, what=""):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want), err_msg=what)
