"""models/detection/image_list.py: ImageList, a batch of images of possibly different sizes padded into one tensor."""
from __future__ import annotations

from typing import List, Tuple

import torch
from torch import Tensor

__all__ = ["ImageList"]


class ImageList:
    """image_list.py:7-25.  tensors: the padded batch; image_sizes: the (h, w) of every image before padding."""

    def __init__(self, tensors: Tensor, image_sizes: List[Tuple[int, int]]) -> None:
        self.tensors = tensors
        self.image_sizes = image_sizes

    def to(self, device: torch.device) -> "ImageList":
        cast_tensor = self.tensors.to(device)
        return ImageList(cast_tensor, self.image_sizes)
