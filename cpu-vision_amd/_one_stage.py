"""What the one-stage detectors RetinaNet (retinanet.py), FCOS (fcos.py) and SSD (ssd.py; ssdlite.py builds an SSD) share: `forward`,
`eager_outputs` and the per-image tail behind a model's `candidates` (boolean indexing by `valid`, ops.batched_nms, the slice), stated
once in OneStageDetector.  A subclass keeps its `__init__` (nothing is constructed here: the submodules, their order and the RNG draws
are the reference's), its `candidates`, its `postprocess_detections` with the reference's signature and `_detect`, the hook through
which `forward` reaches it.  `pyramid_strides` is the start of RetinaNet's and FCOS's `candidates`.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn, Tensor

from . import _lib
from . import ops as box_ops


def pyramid_strides(cell_anchors, maps: List[Tensor], padded_size) -> List[Tuple[int, int]]:
    """One set of cell anchors per map (the reference's _assert), then (stride_h, stride_w) of every map in the padded batch."""
    torch._assert(len(cell_anchors) == len(maps),
                  "Anchors should be Tuple[Tuple[int]] because each feature "
                  "map could potentially have different sizes and aspect ratios. "
                  "There needs to be a match between the number of "
                  "feature maps passed and the number of sizes / aspect ratios specified.")
    return [(int(padded_size[0]) // int(m.shape[-2]), int(padded_size[1]) // int(m.shape[-1])) for m in maps]


class OneStageDetector(nn.Module):
    """forward(images: List[Tensor (C, H, W) float32 in 0..1]) -> List[{boxes, scores, labels}] over self.transform, self.backbone,
    self.head and the subclass's `_detect`.  `_name` is the class's word in the messages: an attribute, so a subclass of a detector
    speaks as its parent does."""

    _name = "OneStageDetector"

    def eager_outputs(self, losses, detections):
        if self.training:
            return losses

        return detections

    def _nms_tail(self, boxes: Tensor, scores: Tensor, labels: Tensor, valid: Tensor) -> List[Dict[str, Tensor]]:
        """Per image the boolean indexing by `valid` (the one read-back besides the nms's count), ops.batched_nms over the labels
        and the slice to detections_per_img."""
        detections: List[Dict[str, Tensor]] = []
        for b, s, lab, v in zip(boxes, scores, labels, valid):
            b, s, lab = b[v], s[v], lab[v]
            # non-maximum suppression
            keep = box_ops.batched_nms(b, s, lab, self.nms_thresh)
            keep = keep[: self.detections_per_img]
            detections.append({"boxes": b[keep], "scores": s[keep], "labels": lab[keep]})
        return detections

    def _detect(self, head_outputs: Dict[str, List[Tensor]], features: List[Tensor], images) -> List[Dict[str, Tensor]]:
        """The subclass's postprocess_detections, with the arguments it takes."""
        raise NotImplementedError

    def forward(self, images: List[Tensor], targets: Optional[List[Dict[str, Tensor]]] = None) -> List[Dict[str, Tensor]]:
        if self.training or targets is not None:
            raise RuntimeError(f"the MI355X {self._name} is inference only: call .eval() and pass no targets")

        # get the original image sizes
        original_image_sizes: List[Tuple[int, int]] = []
        for img in images:
            val = img.shape[-2:]
            torch._assert(len(val) == 2, f"expecting the last two dimensions of the Tensor to be H and W instead got {img.shape[-2:]}")
            original_image_sizes.append((val[0], val[1]))

        # transform the input
        images, targets = self.transform(images, targets)

        # get the features from the backbone
        features = self.backbone(images.tensors)
        if isinstance(features, Tensor):
            features = OrderedDict([("0", features)])

        features = list(features.values())
        for f in features:
            if f.dtype != torch.float32:
                raise TypeError(f"{self._name} computes in float32. Got features {f.dtype}")

        with torch.no_grad():
            # compute the heads' outputs using the features, then the detections
            head_outputs = self.head(features)
            detections = self._detect(head_outputs, features, images)
        deps = (*features, *self.head.parameters())
        where = f"{self._name}.forward"
        detections = [{"boxes": _lib.forward_only(d["boxes"], where, *deps), "scores": _lib.forward_only(d["scores"], where, *deps),
                       "labels": d["labels"]} for d in detections]
        detections = self.transform.postprocess(detections, images.image_sizes, original_image_sizes)

        return self.eager_outputs({}, detections)
