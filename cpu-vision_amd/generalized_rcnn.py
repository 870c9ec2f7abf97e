"""models/detection/generalized_rcnn.py: GeneralizedRCNN, the transform -> backbone -> rpn -> roi_heads -> postprocess pipeline.
Inference only: eval mode returns the detections; training mode and targets raise."""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn, Tensor

__all__ = ["GeneralizedRCNN"]


class GeneralizedRCNN(nn.Module):
    """generalized_rcnn.py:14-118.  forward(images: List[Tensor (C, H, W)]) -> List[{boxes, labels, scores}], the boxes in the
    coordinates of the images as they were passed."""

    def __init__(self, backbone: nn.Module, rpn: nn.Module, roi_heads: nn.Module, transform: nn.Module) -> None:
        super().__init__()
        self.transform = transform
        self.backbone = backbone
        self.rpn = rpn
        self.roi_heads = roi_heads
        # used only on torchscript mode
        self._has_warned = False
        self.eval()

    def eager_outputs(self, losses, detections):
        if self.training:
            return losses

        return detections

    def forward(self, images: List[Tensor], targets: Optional[List[Dict[str, Tensor]]] = None) -> List[Dict[str, Tensor]]:
        if self.training or targets is not None:
            raise RuntimeError("the MI355X GeneralizedRCNN is inference only: call .eval() and pass no targets")

        original_image_sizes: List[Tuple[int, int]] = []
        for img in images:
            val = img.shape[-2:]
            torch._assert(len(val) == 2, f"expecting the last two dimensions of the Tensor to be H and W instead got {img.shape[-2:]}")
            original_image_sizes.append((val[0], val[1]))

        images, targets = self.transform(images, targets)
        features = self.backbone(images.tensors)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        proposals, proposal_losses = self.rpn(images, features, targets)
        detections, detector_losses = self.roi_heads(features, proposals, images.image_sizes, targets)
        detections = self.transform.postprocess(detections, images.image_sizes, original_image_sizes)  # type: ignore[operator]

        losses = {}
        losses.update(detector_losses)
        losses.update(proposal_losses)
        return self.eager_outputs(losses, detections)
