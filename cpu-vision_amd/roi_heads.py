"""RoIHeads inference on the MI355X kernels: pooler -> box head -> box predictor -> postprocess_detections.

Mirrors models/detection/roi_heads.py of the reference the way rpn.py mirrors models/detection/rpn.py: the same class, constructor
arguments, child names (box_roi_pool, box_head, box_predictor) and state-dict keys.  Only `forward` differs.  The reference's
postprocess_detections runs a softmax, BoxCoder.decode over every class, clip_boxes_to_image, three slices that drop the background
column, three reshapes and two filter passes per image; here F.roi_detections does all of it for the whole batch in ONE launch and
writes dense (R, C - 1) boxes / scores / labels with a validity flag.  What is left per image is what rpn.filter_proposals_detailed
also does: the boolean indexing by `valid` (one read-back), ops.batched_nms and the slice.

Numerics: DESIGN.md 3.25 and mi355vision.h mv_roi_detections_f32 -- every float operation is the reference's float32 operation,
rounded once; exp is the correctly rounded float32 exp and the softmax sum is one ascending chain.  Inference only, float32 only:
the matcher, the sampler and the losses of the reference are not built.

With mask modules (mask_rcnn.py: this package's MultiScaleRoIAlign, MaskRCNNHeads and MaskRCNNPredictor) `forward` runs the
reference's mask branch on the detected boxes and adds "masks" (N_i, 1, M, M) to every result: pooler -> mask head -> predictor ->
F.mask_probs, which reads only the predicted label's plane of every roi.

With keypoint modules (keypoint_rcnn.py: this package's MultiScaleRoIAlign, KeypointRCNNHeads and KeypointRCNNPredictor, all three
or none) `forward` then runs the reference's keypoint branch on the detected boxes and adds "keypoints" (N_i, K, 3) and
"keypoints_scores" (N_i, K): pooler -> keypoint head -> predictor -> ONE F.heatmaps_to_keypoints launch on the concatenated boxes of
the whole batch, where the reference loops over the detections with a bicubic interpolate and two read-backs each.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
from torch import nn, Tensor

from . import _lib
from . import functional as F
from . import ops as box_ops
from .rpn import BoxCoder

__all__ = ["RoIHeads", "postprocess_detections_detailed", "check_keypoint_modules"]


def postprocess_detections_detailed(class_logits: Tensor, box_regression: Tensor, proposals: List[Tensor], image_shapes: List[Tuple[int, int]],
                                    box_coder: BoxCoder, score_thresh: float, nms_thresh: float, detections_per_img: int,
                                    min_size: float = 1e-2) -> Tuple[List[Tensor], List[Tensor], List[Tensor]]:
    """roi_heads.py postprocess_detections -> (boxes, scores, labels) per image: one F.roi_detections call for the whole batch, then
    per image the boolean indexing by `valid` (the one read-back besides the nms's count), ops.batched_nms per class and the slice."""
    boxes_per_image = [int(boxes_in_image.shape[0]) for boxes_in_image in proposals]
    rois = box_ops._convert_to_roi_format([p.to(class_logits.dtype) for p in proposals])
    boxes, scores, labels, valid = F.roi_detections(class_logits, box_regression, rois, image_shapes, box_coder.weights,
                                                    box_coder.bbox_xform_clip, score_thresh, min_size)
    all_boxes, all_scores, all_labels = [], [], []
    for b, s, lab, v in zip(boxes.split(boxes_per_image, 0), scores.split(boxes_per_image, 0), labels.split(boxes_per_image, 0),
                            valid.split(boxes_per_image, 0)):
        # batch everything, by making every class prediction be a separate instance; low scores and empty boxes are `valid`'s zeros
        b, s, lab = b[v], s[v], lab[v]
        # non-maximum suppression, independently done per class
        keep = box_ops.batched_nms(b, s, lab, nms_thresh)
        # keep only topk scoring predictions
        keep = keep[:detections_per_img]
        all_boxes.append(b[keep])
        all_scores.append(s[keep])
        all_labels.append(lab[keep])
    return all_boxes, all_scores, all_labels


def check_keypoint_modules(keypoint_roi_pool, keypoint_head, keypoint_predictor) -> None:
    """The keypoint modules RoIHeads runs: this package's MultiScaleRoIAlign, KeypointRCNNHeads and KeypointRCNNPredictor, all three
    or none.  Anything else raises NotImplementedError naming the argument -- another object would compute on another path, and one
    module without the others would silently run no keypoint branch (as it does in the reference)."""
    from .keypoint_rcnn import KeypointRCNNHeads, KeypointRCNNPredictor  # keypoint_rcnn imports faster_rcnn, which imports this module

    given = (("keypoint_roi_pool", keypoint_roi_pool, box_ops.MultiScaleRoIAlign), ("keypoint_head", keypoint_head, KeypointRCNNHeads),
             ("keypoint_predictor", keypoint_predictor, KeypointRCNNPredictor))
    for name, module, kind in given:
        if module is not None and not isinstance(module, kind):
            raise NotImplementedError(f"RoIHeads: {name} is a {type(module).__name__}, and the keypoint branch on the MI355X path runs "
                                      f"this package's {kind.__name__} only")
    missing = [name for name, module, _ in given if module is None]
    if 0 < len(missing) < 3:
        present = [name for name, module, _ in given if module is not None]
        raise NotImplementedError(f"RoIHeads: {', '.join(present)} given without {', '.join(missing)}: the keypoint branch on the MI355X "
                                  "path takes its three modules together")


class RoIHeads(nn.Module):
    """roi_heads.py:496-876, inference: forward(features, proposals, image_shapes) -> ([{boxes, labels, scores[, masks][, keypoints,
    keypoints_scores]}] per image, {}).  The training arguments are kept as given; the mask modules must be this package's
    (mask_rcnn.py) and the keypoint modules this package's, all three together (keypoint_rcnn.py); any other object raises
    NotImplementedError."""

    __annotations__ = {"box_coder": BoxCoder}

    def __init__(self, box_roi_pool, box_head, box_predictor,
                 # Faster R-CNN training
                 fg_iou_thresh, bg_iou_thresh, batch_size_per_image, positive_fraction, bbox_reg_weights,
                 # Faster R-CNN inference
                 score_thresh, nms_thresh, detections_per_img,
                 # Mask
                 mask_roi_pool=None, mask_head=None, mask_predictor=None, keypoint_roi_pool=None, keypoint_head=None,
                 keypoint_predictor=None):
        super().__init__()
        from .mask_rcnn import MaskRCNNHeads, MaskRCNNPredictor  # mask_rcnn imports faster_rcnn, which imports this module

        for name, module, kind in (("mask_roi_pool", mask_roi_pool, box_ops.MultiScaleRoIAlign), ("mask_head", mask_head, MaskRCNNHeads),
                                   ("mask_predictor", mask_predictor, MaskRCNNPredictor)):
            if module is not None and not isinstance(module, kind):
                raise NotImplementedError(f"RoIHeads: {name} is a {type(module).__name__}, and the mask branch on the MI355X path runs "
                                          f"this package's {kind.__name__} only")
        check_keypoint_modules(keypoint_roi_pool, keypoint_head, keypoint_predictor)
        self.box_similarity = box_ops.box_iou
        # used during training (kept as given: the matcher and the sampler are not built)
        self.fg_iou_thresh, self.bg_iou_thresh = fg_iou_thresh, bg_iou_thresh
        self.batch_size_per_image, self.positive_fraction = batch_size_per_image, positive_fraction

        if bbox_reg_weights is None:
            bbox_reg_weights = (10.0, 10.0, 5.0, 5.0)
        self.box_coder = BoxCoder(bbox_reg_weights)

        self.box_roi_pool = box_roi_pool
        self.box_head = box_head
        self.box_predictor = box_predictor

        self.score_thresh = score_thresh
        self.nms_thresh = nms_thresh
        self.detections_per_img = detections_per_img

        self.mask_roi_pool = mask_roi_pool
        self.mask_head = mask_head
        self.mask_predictor = mask_predictor

        self.keypoint_roi_pool = keypoint_roi_pool
        self.keypoint_head = keypoint_head
        self.keypoint_predictor = keypoint_predictor
        self.eval()

    def has_mask(self):
        if self.mask_roi_pool is None:
            return False
        if self.mask_head is None:
            return False
        if self.mask_predictor is None:
            return False
        return True

    def has_keypoint(self):
        if self.keypoint_roi_pool is None:
            return False
        if self.keypoint_head is None:
            return False
        if self.keypoint_predictor is None:
            return False
        return True

    def postprocess_detections(self, class_logits: Tensor, box_regression: Tensor, proposals: List[Tensor],
                               image_shapes: List[Tuple[int, int]]) -> Tuple[List[Tensor], List[Tensor], List[Tensor]]:
        return postprocess_detections_detailed(class_logits, box_regression, proposals, image_shapes, self.box_coder, self.score_thresh,
                                               self.nms_thresh, self.detections_per_img)

    def forward(self, features: Dict[str, Tensor], proposals: List[Tensor], image_shapes: List[Tuple[int, int]],
                targets: Optional[List[Dict[str, Tensor]]] = None) -> Tuple[List[Dict[str, Tensor]], Dict[str, Tensor]]:
        if self.training or targets is not None:
            raise RuntimeError("the MI355X RoIHeads is inference only: call .eval() and pass no targets")
        for f in features.values():
            if f.dtype != torch.float32:
                raise TypeError(f"RoIHeads computes in float32. Got features {f.dtype}")
        with torch.no_grad():  # no autograd bookkeeping per launch; the results are marked once (their backward raises)
            box_features = self.box_roi_pool(features, proposals, image_shapes)
            box_features = self.box_head(box_features)
            class_logits, box_regression = self.box_predictor(box_features)
            boxes, scores, labels = self.postprocess_detections(class_logits, box_regression, proposals, image_shapes)
        deps = (*features.values(), *proposals, *self.box_head.parameters(), *self.box_predictor.parameters())
        result: List[Dict[str, Tensor]] = []
        for i in range(len(boxes)):
            result.append({"boxes": _lib.forward_only(boxes[i], "RoIHeads.forward", *deps), "labels": labels[i],
                           "scores": _lib.forward_only(scores[i], "RoIHeads.forward", *deps)})
        if self.has_mask():
            mask_deps = (*deps, *self.mask_head.parameters(), *self.mask_predictor.parameters())
            for r, probs in zip(result, self.mask_branch(features, boxes, labels, image_shapes)):
                r["masks"] = _lib.forward_only(probs, "RoIHeads.forward", *mask_deps)
        if self.has_keypoint():
            check_keypoint_modules(self.keypoint_roi_pool, self.keypoint_head, self.keypoint_predictor)
            kp_deps = (*deps, *self.keypoint_head.parameters(), *self.keypoint_predictor.parameters())
            for r, (kps, kp_scores) in zip(result, self.keypoint_branch(features, boxes, image_shapes)):
                r["keypoints"] = _lib.forward_only(kps, "RoIHeads.forward", *kp_deps)
                r["keypoints_scores"] = _lib.forward_only(kp_scores, "RoIHeads.forward", *kp_deps)
        return result, {}

    def mask_branch(self, features: Dict[str, Tensor], boxes: List[Tensor], labels: List[Tensor],
                    image_shapes: List[Tuple[int, int]]) -> List[Tensor]:
        """roi_heads.py:815-850, inference: mask_roi_pool on the detected boxes -> mask_head -> mask_predictor -> F.mask_probs on the
        concatenated labels (maskrcnn_inference: one gather + sigmoid launch), split per image into (N_i, 1, M, M).  Without a
        detection in the whole batch nothing is launched and every image gets an empty tensor."""
        boxes_per_image = [int(b.shape[0]) for b in boxes]
        with torch.no_grad():
            if sum(boxes_per_image) == 0:
                # MaskRCNNHeads keeps the pooled size, MaskRCNNPredictor's ConvTranspose2d(2, 2) doubles it
                mh, mw = (2 * int(s) for s in self.mask_roi_pool.output_size)
                return [b.new_empty((0, 1, mh, mw)) for b in boxes]
            mask_features = self.mask_roi_pool(features, [b.detach() for b in boxes], image_shapes)
            mask_features = self.mask_head(mask_features)
            mask_logits = self.mask_predictor(mask_features)
            probs = F.mask_probs(mask_logits, torch.cat(labels))
        return list(probs.split(boxes_per_image, dim=0))

    def keypoint_branch(self, features: Dict[str, Tensor], boxes: List[Tensor],
                        image_shapes: List[Tuple[int, int]]) -> List[Tuple[Tensor, Tensor]]:
        """roi_heads.py:852-874, inference: keypoint_roi_pool on the detected boxes -> keypoint_head -> keypoint_predictor -> ONE
        F.heatmaps_to_keypoints call on the concatenated boxes (keypointrcnn_inference calls it per image, and it loops over the
        detections), split per image into ((N_i, K, 3), (N_i, K)).  Without a detection in the whole batch nothing is launched and
        every image gets empty tensors."""
        boxes_per_image = [int(b.shape[0]) for b in boxes]
        with torch.no_grad():
            if sum(boxes_per_image) == 0:
                k = int(self.keypoint_predictor.out_channels)
                return [(b.new_empty((0, k, 3)), b.new_empty((0, k))) for b in boxes]
            rois = [b.detach() for b in boxes]
            keypoint_features = self.keypoint_roi_pool(features, rois, image_shapes)
            keypoint_features = self.keypoint_head(keypoint_features)
            keypoint_logits = self.keypoint_predictor(keypoint_features)
            xy, scores = F.heatmaps_to_keypoints(keypoint_logits, torch.cat(rois))
        return list(zip(xy.split(boxes_per_image, dim=0), scores.split(boxes_per_image, dim=0)))
