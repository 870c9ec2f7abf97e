"""MixUp / CutMix on a collated batch -- the data movement and arithmetic of the reference's transforms/v2/_augment.py
`_BaseMixUpCutMix`, `MixUp` and `CutMix`, which has no functional form: `mixup_image`, `cutmix_image` and `mixup_labels` are
project extensions in the manner of `resized_crop_flip_normalize`.  Sample b of the batch is paired with sample b - 1 (the
reference's `roll(1, 0)`); each call is ONE launch of csrc/batchmix.hip (mv_mixup_* / mv_cutmix / mv_mixup_labels_i64;
DESIGN.md section 3.18), and there is no CPU path.

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _lib

_MIXUP_ENTRIES = {torch.float32: "mv_mixup_f32", torch.float16: "mv_mixup_f16", torch.float64: "mv_mixup_f64"}


def _mixup_rows(batch: torch.Tensor, lam: float, what: str) -> torch.Tensor:
    """fl(fl(batch.roll(1, 0) * (1 - lam)) + fl(batch * lam)) over the leading dimension of a floating (B, ...) tensor."""
    if batch.ndim < 1:
        raise ValueError(f"{what}: expected a batch with a leading batch dimension, got a 0-d tensor")
    if not batch.is_floating_point():
        raise TypeError(f"{what}: mixing needs a floating point batch, got {batch.dtype}; convert first, e.g. with "
                        "to_dtype(batch, torch.float32, scale=True)")
    if batch.dtype not in _MIXUP_ENTRIES:
        raise NotImplementedError(f"{what}: {batch.dtype} is not on the MI355X path (float32, float16 and float64 are)")
    _lib.require_device(batch)
    lib = _lib.load()
    with _lib.on_device_of(batch):
        x = batch.contiguous()
        y = torch.empty_like(x, memory_format=torch.contiguous_format)
        n = int(x.shape[0])
        if x.numel():
            _lib.check(getattr(lib, _MIXUP_ENTRIES[x.dtype])(x.data_ptr(), y.data_ptr(), n, x.numel() // n, float(lam),
                                                            _lib.stream_ptr(x)))
    return _lib.forward_only(y, what, batch)


def mixup_image(batch: torch.Tensor, lam: float) -> torch.Tensor:
    """MixUp._transform on a (B, ...) float32 / float16 / float64 batch: batch.roll(1, 0).mul_(1.0 - lam).add_(batch.mul(lam)),
    bit for bit, reading the batch once.  Integer batches raise TypeError (the reference's mul_ raises there)."""
    return _mixup_rows(batch, lam, "mixup_image")


def cutmix_image(batch: torch.Tensor, box: Sequence[int]) -> torch.Tensor:
    """CutMix._transform on a (B, ..., H, W) batch of any 1 / 2 / 4 / 8-byte dtype: a copy of the batch whose box
    `box = (x1, y1, x2, y2)` -- columns [x1, x2), rows [y1, y2), inside the image -- comes from batch.roll(1, 0)."""
    if batch.ndim < 3:
        raise ValueError(f"cutmix_image: expected a batch of shape (B, ..., H, W), got {tuple(batch.shape)}")
    x1, y1, x2, y2 = (int(v) for v in box)
    h, w = int(batch.shape[-2]), int(batch.shape[-1])
    if not (0 <= x1 <= x2 <= w and 0 <= y1 <= y2 <= h):
        raise ValueError(f"cutmix_image: the box (x1={x1}, y1={y1}, x2={x2}, y2={y2}) must lie inside the ({h}, {w}) image")
    if batch.element_size() not in (1, 2, 4, 8) or batch.is_complex():
        raise NotImplementedError(f"cutmix_image: {batch.dtype} images are not on the MI355X path")
    _lib.require_device(batch)
    lib = _lib.load()
    with _lib.on_device_of(batch):
        x = batch.contiguous()
        y = torch.empty_like(x, memory_format=torch.contiguous_format)
        n = int(x.shape[0])
        if x.numel():
            _lib.check(lib.mv_cutmix(x.data_ptr(), y.data_ptr(), n, x.numel() // (n * h * w), x.element_size(), h, w, x1, y1, x2, y2,
                                     _lib.stream_ptr(x)))
    return _lib.forward_only(y, "cutmix_image", batch) if batch.is_floating_point() else y


def mixup_labels(labels: torch.Tensor, lam: float, num_classes: Optional[int] = None) -> torch.Tensor:
    """_BaseMixUpCutMix._mixup_label: index labels (B,) int64 become one_hot(labels, num_classes).float(), probability labels
    (B, K) are cast with .float() unless floating, then label.roll(1, 0).mul_(1.0 - lam).add_(label.mul(lam)).  Index labels take
    one launch that never materialises the one-hot tensor.

    The reference's one_hot raises on a label outside [0, num_classes), which needs a device-to-host read.  Here such a label is
    not reported: it matches no class, so its share of the two rows it takes part in is zeros."""
    if labels.ndim not in (1, 2):
        raise ValueError("labels should be index based with shape (batch_size,) or probability based with shape (batch_size, "
                         f"num_classes), but got a tensor of shape {labels.shape} instead.")
    if labels.ndim == 2:
        return _mixup_rows(labels if labels.is_floating_point() else labels.float(), lam, "mixup_labels")
    if num_classes is None:
        raise ValueError("num_classes must be passed if the labels are index-based (1D)")
    if labels.dtype != torch.int64:
        raise RuntimeError("one_hot is only applicable to index tensor of type LongTensor.")
    if int(num_classes) <= 0:
        raise ValueError(f"num_classes should be positive, got {num_classes}")
    _lib.require_device(labels)
    lib = _lib.load()
    with _lib.on_device_of(labels):
        x = labels.contiguous()
        y = torch.empty((int(x.shape[0]), int(num_classes)), dtype=torch.float32, device=x.device)
        if y.numel():
            _lib.check(lib.mv_mixup_labels_i64(x.data_ptr(), y.data_ptr(), int(x.shape[0]), int(num_classes), float(lam),
                                               _lib.stream_ptr(x)))
    return y
