"""The functional entries of the detection heads (models/detection/rpn.py, roi_heads.py, retinanet.py, _utils.py BoxCoder): rpn_topk,
rpn_decode and box_decode over mv_rpn_topk_f32 / mv_rpn_decode_f32 / mv_box_decode_f32 (csrc/rpn.hip), roi_detections over
mv_roi_detections_f32 (csrc/roi_heads.hip), retinanet_topk and retinanet_decode over mv_retinanet_topk_f32 / mv_retinanet_decode_f32
(csrc/retinanet.hip), fcos_topk and fcos_decode over mv_fcos_topk_f32 / mv_fcos_decode_f32 (the same file: fcos.py's centerness score and
BoxLinearCoder.decode), ssd_scores, ssd_topk and ssd_decode over mv_ssd_scores_f32 / mv_ssd_topk_f32 / mv_ssd_decode_f32 (csrc/ssd.hip:
ssd.py's softmax, per-class top-k and default boxes).  float32, forward-only; the argument checks fire before a device is needed.  Every name
here is re-exported by `functional`.

Stated once: the checks of per-level maps (_level_maps, _class_maps, _fcos_maps), of k, idx, strides and the four weights (_check_*);
the pyramid top-k and decode of the rpn and retinanet (_topk, _decode); a decode entry's four outputs and its return (_candidate_outputs,
_candidates).  fcos_topk and fcos_decode keep bodies of their own: routed through _topk / _decode they measured slower.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib

MAX_RPN_LEVELS = 8   # kMaxRpnLevels
MAX_RPN_TOPK = 4096  # kRpnMaxK
MAX_ROI_CLASSES = 2048  # kRoiMaxClasses
BBOX_XFORM_CLIP = math.log(1000.0 / 16)


def _level_maps(name: str, maps: Sequence[torch.Tensor], what: str, per_anchor: int, anchors: Optional[List[int]] = None):
    """The checks of a list of per-level NCHW maps ((n, per_anchor * A_l, H_l, W_l) float32) -> [(n, A_l, H_l, W_l)]."""
    if not isinstance(maps, (list, tuple)) or not maps:
        raise TypeError(f"{name}: {what} should be a non-empty list of tensors, one per level")
    if len(maps) > MAX_RPN_LEVELS:
        raise _lib.Mi355VisionError(f"{name}: up to {MAX_RPN_LEVELS} levels per call, got {len(maps)}")
    shapes = []
    for l, m in enumerate(maps):
        if not isinstance(m, torch.Tensor) or m.dim() != 4:
            raise RuntimeError(f"{name}: {what}[{l}] should be a 4-D tensor (N, C, H, W)")
        if m.dtype != torch.float32:
            raise TypeError(f"{name} computes in float32. Got {what}[{l}] {m.dtype}")
        n, c, h, w = (int(d) for d in m.shape)
        if n != int(maps[0].shape[0]):
            raise RuntimeError(f"{name}: {what}[{l}] holds {n} images, {what}[0] holds {int(maps[0].shape[0])}")
        if c < 1 or h < 1 or w < 1 or c % per_anchor:
            raise RuntimeError(f"{name}: bad shape {tuple(m.shape)} of {what}[{l}]")
        if anchors is not None and c != per_anchor * anchors[l]:
            raise RuntimeError(f"{name}: {what}[{l}] has {c} channels for {anchors[l]} anchors per location")
        shapes.append((n, c // per_anchor, h, w))
    if sum(a * h * w for _, a, h, w in shapes) >= 2 ** 31:
        raise _lib.Mi355VisionError(f"{name}: the anchors of all levels exceed the 32-bit index")
    return shapes


def _dense_images(m: torch.Tensor) -> torch.Tensor:
    """The map itself when each of its images is dense (a channel slice of a wider contiguous tensor is), else a contiguous copy."""
    m = m.detach()
    _, c, h, w = m.shape
    if m.stride(3) == 1 and m.stride(2) == w and m.stride(1) == h * w and (m.shape[0] == 1 or m.stride(0) >= c * h * w):
        return m
    return m.contiguous()


def _tables(shapes):
    num = len(shapes)
    return ((C.c_int * num)(*[s[2] for s in shapes]), (C.c_int * num)(*[s[3] for s in shapes]), (C.c_int * num)(*[s[1] for s in shapes]))


def _img_strides(maps):
    return (C.c_int64 * len(maps))(*[int(m.stride(0)) if m.shape[0] > 1 else int(m[0].numel()) for m in maps])


def _image_sizes(name: str, image_sizes, fits, rows: str) -> torch.Tensor:
    """image_sizes (rows (h, w): a list, or an (N, 2) tensor) as a tensor; `fits(sizes)` is the caller's rule for the rows, `rows`
    its words in the message."""
    sizes = image_sizes if isinstance(image_sizes, torch.Tensor) else torch.tensor([[float(s[0]), float(s[1])] for s in image_sizes],
                                                                                 dtype=torch.float32).reshape(-1, 2)
    if not fits(sizes):
        raise RuntimeError(f"{name}: image_sizes should hold {rows} (height, width), got {tuple(sizes.shape)}")
    return sizes


def _check_k(name: str, k, reject_bool: bool = False) -> None:
    if not isinstance(k, int) or (reject_bool and isinstance(k, bool)) or k < 1:
        raise ValueError(f"{name}: k must be a positive int, got {k!r}")
    if k > MAX_RPN_TOPK:
        raise _lib.Mi355VisionError(f"{name}: k up to {MAX_RPN_TOPK}, got {k}")


def _check_idx(name: str, idx, n: int, cols: str = "K") -> None:
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.dtype != torch.int32 or int(idx.shape[0]) != n:
        raise RuntimeError(f"{name}: idx should be an int32 tensor of shape ({n}, {cols})")


def _check_strides(name: str, strides, num: int) -> None:
    if len(strides) != num or any(len(s) != 2 or int(s[0]) < 0 or int(s[1]) < 0 for s in strides):
        raise RuntimeError(f"{name}: strides should hold one non-negative (stride_h, stride_w) per level, got {strides!r}")


def _check_weights(name: str, weights) -> None:
    if len(weights) != 4:
        raise ValueError(f"{name}: four weights (wx, wy, ww, wh), got {weights!r}")


def _candidate_outputs(shape: Tuple[int, int], device):
    """The four outputs of a decode entry, uninitialised: boxes (*shape, 4) and scores float32, the int64 output, valid uint8."""
    return (torch.empty((*shape, 4), dtype=torch.float32, device=device), torch.empty(shape, dtype=torch.float32, device=device),
            torch.empty(shape, dtype=torch.int64, device=device), torch.empty(shape, dtype=torch.uint8, device=device))


def _candidates(name: str, deps, boxes, scores, third, valid):
    """What a decode entry returns: boxes and scores forward-only in `deps`, the int64 output, valid as bool."""
    return _lib.forward_only(boxes, name, *deps), _lib.forward_only(scores, name, *deps), third, valid.view(torch.bool)


def _topk(name: str, logits, shapes, k, classes: Optional[int] = None, score_thresh=None) -> torch.Tensor:
    """What rpn_topk and retinanet_topk share behind the checks of their maps: the checks of k, the workspace of
    mv_<name>_workspace_bytes and the launch of mv_<name>_f32.  classes and score_thresh: retinanet's, arguments of its entries only."""
    _check_k(name, k)
    per_anchor = 1 if classes is None else classes
    classes, thresh = (() if classes is None else (classes,)), (() if score_thresh is None else (float(score_thresh),))
    for m in logits:
        _lib.require_device(m, "logits")
    lib = _lib.load()
    l0, n = logits[0], shapes[0][0]
    total = sum(min(k, a * h * w * per_anchor) for _, a, h, w in shapes)
    with _lib.on_device_of(l0):
        maps = [_dense_images(m) for m in logits]
        idx = torch.empty((n, total), dtype=torch.int32, device=l0.device)
        if n:
            hs, ws, as_ = _tables(shapes)
            nbytes = int(getattr(lib, f"mv_{name}_workspace_bytes")(n, hs, ws, as_, len(maps), *classes, k))
            if not nbytes:
                raise _lib.Mi355VisionError(f"{name}: {n} images are more than one call takes")
            buf, ws_ptr, nbytes = _lib.workspace(nbytes, l0.device)
            _lib.launch(getattr(lib, f"mv_{name}_f32"), l0, _lib.pointer_table(maps), hs, ws, as_, _img_strides(maps), len(maps), *classes, n, k,
                        *thresh, idx.data_ptr(), ws_ptr, nbytes)
    return idx


def _decode(name: str, logits, shapes, deltas, idx, cell_anchors, strides, image_sizes, weights, clip, classes=(), filters=()):
    """What rpn_decode and retinanet_decode share behind the checks of their logits: the checks of the other arguments, the staging
    and the launch of mv_<name>_f32 -> boxes, scores, the entry's int64 output, valid.  classes: (num_classes,) for retinanet's
    entry; filters: (min_size, score_thresh) for the rpn's."""
    anchors = [a for _, a, _, _ in shapes]
    dshapes = _level_maps(name, deltas, "deltas", 4, anchors) if isinstance(deltas, (list, tuple)) and len(deltas) == len(logits) else None
    if dshapes is None or any(d[2:] != s[2:] or d[0] != s[0] for d, s in zip(dshapes, shapes)):
        raise RuntimeError(f"{name}: deltas should hold one map per level of logits, of the same batch and size with 4 channels per anchor")
    num, n = len(shapes), shapes[0][0]
    _check_idx(name, idx, n)
    if not isinstance(cell_anchors, (list, tuple)) or len(cell_anchors) != num or \
            any(tuple(c.shape) != (a, 4) for c, a in zip(cell_anchors, anchors)):
        raise RuntimeError(f"{name}: cell_anchors should hold one (A, 4) tensor per level, A = {anchors}")
    _check_strides(name, strides, num)
    _check_weights(name, weights)
    sizes = _image_sizes(name, image_sizes, lambda t: tuple(t.shape) == (n, 2), f"{n} rows")
    for m in (*logits, *deltas, idx):
        _lib.require_device(m, f"{name} input")
    lib = _lib.load()
    l0, k = logits[0], int(idx.shape[1])
    with _lib.on_device_of(l0):
        lmaps, dmaps = [_dense_images(m) for m in logits], [_dense_images(m) for m in deltas]
        base = torch.cat([_lib.table_on(c, l0.device) for c in cell_anchors]).contiguous()
        sizes = _lib.table_on(sizes, l0.device)
        ix = idx.contiguous()
        boxes, scores, third, valid = _candidate_outputs((n, k), l0.device)
        if n and k:
            hs, ws, as_ = _tables(shapes)
            sh = (C.c_int * num)(*[int(s[0]) for s in strides])
            sw = (C.c_int * num)(*[int(s[1]) for s in strides])
            _lib.launch(getattr(lib, f"mv_{name}_f32"), l0, _lib.pointer_table(lmaps), _lib.pointer_table(dmaps), hs, ws, as_,
                        _img_strides(lmaps), _img_strides(dmaps), sh, sw, num, *classes, base.data_ptr(), sizes.data_ptr(), ix.data_ptr(), n, k,
                        *[float(w) for w in weights], float(clip), *[float(f) for f in filters], boxes.data_ptr(), scores.data_ptr(),
                        third.data_ptr(), valid.data_ptr())
    return _candidates(name, (*logits, *deltas), boxes, scores, third, valid)


def rpn_topk(logits: List[torch.Tensor], k: int) -> torch.Tensor:
    """filter_proposals' per-level top-k (rpn.py) on the head's own NCHW logits, ONE launch: logits[l] (N, A_l, H_l, W_l) -> idx
    (N, K) int32, K = sum_l min(k, A_l H_l W_l): per image, level after level, the indices into the reference's concatenated
    (y, x, a) layout of the level's greatest logits in stable descending order (equal logits by ascending index, NaN greatest)."""
    return _topk("rpn_topk", logits, _level_maps("rpn_topk", logits, "logits", 1), k)


def rpn_decode(logits: List[torch.Tensor], deltas: List[torch.Tensor], idx: torch.Tensor, cell_anchors: List[torch.Tensor],
               strides: Sequence[Tuple[int, int]], image_sizes, weights: Tuple[float, float, float, float] = (1.0, 1.0, 1.0, 1.0),
               bbox_xform_clip: float = BBOX_XFORM_CLIP, min_size: float = 1e-3,
               score_thresh: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The rest of filter_proposals before the nms for the candidates idx (N, K) of rpn_topk, ONE launch, one lane per candidate:
    its anchor from cell_anchors[l] (A_l, 4) and strides[l] = (stride_h, stride_w), BoxCoder.decode_single with `weights`,
    clip_boxes_to_image with image_sizes (N rows (h, w): a list, or an (N, 2) tensor), sigmoid -> boxes (N, K, 4), scores (N, K),
    levels (N, K) int64, valid (N, K) bool = both sides >= min_size and score >= score_thresh."""
    shapes = _level_maps("rpn_decode", logits, "logits", 1)
    return _decode("rpn_decode", logits, shapes, deltas, idx, cell_anchors, strides, image_sizes, weights, bbox_xform_clip,
                   filters=(min_size, score_thresh))


def _class_maps(name: str, logits, num_classes):
    """The checks of RetinaNet's per-level class maps ((n, A_l * num_classes, H_l, W_l) float32) -> [(n, A_l, H_l, W_l)]."""
    if not isinstance(num_classes, int) or isinstance(num_classes, bool) or num_classes < 1:
        raise ValueError(f"{name}: num_classes must be a positive int, got {num_classes!r}")
    shapes = _level_maps(name, logits, "logits", num_classes)
    if sum(a * h * w for _, a, h, w in shapes) * num_classes >= 2 ** 31:
        raise _lib.Mi355VisionError(f"{name}: the anchors of all levels x {num_classes} classes exceed the 32-bit index")
    return shapes


def retinanet_topk(logits: List[torch.Tensor], num_classes: int, k: int, score_thresh: float) -> torch.Tensor:
    """postprocess_detections' sigmoid, `> score_thresh` and per-level topk (retinanet.py) on the head's own NCHW class maps:
    logits[l] (N, A_l * num_classes, H_l, W_l) -> idx (N, Ktot) int32, Ktot = sum_l min(k, A_l H_l W_l num_classes): per image, level
    after level, the flat indices ((y, x, a) anchor index of the concatenated layout) * num_classes + class of the level's
    min(k, passing) greatest scores in stable descending order (equal scores by ascending flat index), then -1.  One (image, level)
    is spread over many workgroups; nothing is read back."""
    return _topk("retinanet_topk", logits, _class_maps("retinanet_topk", logits, num_classes), k, num_classes, score_thresh)


def retinanet_decode(logits: List[torch.Tensor], deltas: List[torch.Tensor], idx: torch.Tensor, cell_anchors: List[torch.Tensor],
                     strides: Sequence[Tuple[int, int]], image_sizes, num_classes: int,
                     weights: Tuple[float, float, float, float] = (1.0, 1.0, 1.0, 1.0),
                     clip: float = BBOX_XFORM_CLIP) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The rest of postprocess_detections before the nms for the candidates idx (N, K) of retinanet_topk, ONE launch, one lane per
    candidate: anchor idx // num_classes from cell_anchors[l] (A_l, 4) and strides[l] = (stride_h, stride_w), label idx % num_classes,
    BoxCoder.decode_single with `weights` and `clip`, clip_boxes_to_image with image_sizes (N rows (h, w): a list, or an (N, 2)
    tensor), the sigmoid -> boxes (N, K, 4), scores (N, K), labels (N, K) int64, valid (N, K) bool (False, with zeros, for the -1
    padding and any other index outside the pyramid)."""
    shapes = _class_maps("retinanet_decode", logits, num_classes)
    return _decode("retinanet_decode", logits, shapes, deltas, idx, cell_anchors, strides, image_sizes, weights, clip, classes=(num_classes,))


def retinanet_topk_chunk() -> int:
    """The elements of an (image, level) class map one stage-1 workgroup of retinanet_topk reads (mv_retinanet_topk_chunk)."""
    return int(_lib.load().mv_retinanet_topk_chunk())


def _fcos_maps(name: str, cls_logits, ctrness, num_classes):
    """The checks of FCOS's per-level class maps (n, num_classes, H_l, W_l) and centerness maps (n, 1, H_l, W_l): one anchor per
    location -> the shapes [(n, 1, H_l, W_l)]."""
    shapes = _class_maps(name, cls_logits, num_classes)
    if any(a != 1 for _, a, _, _ in shapes):
        raise RuntimeError(f"{name}: one anchor per location: cls_logits[l] should have {num_classes} channels, got "
                           f"{[int(m.shape[1]) for m in cls_logits]}")
    cshapes = _level_maps(name, ctrness, "ctrness", 1) if isinstance(ctrness, (list, tuple)) and len(ctrness) == len(cls_logits) else None
    if cshapes is None or cshapes != shapes:
        raise RuntimeError(f"{name}: ctrness should hold one map per level of cls_logits, of the same batch and size with one channel")
    return shapes


def fcos_topk(cls_logits: List[torch.Tensor], ctrness: List[torch.Tensor], num_classes: int, k: int, score_thresh: float) -> torch.Tensor:
    """FCOS.postprocess_detections' score sqrt(sigmoid(cls) * sigmoid(centerness)), `> score_thresh` and per-level topk (fcos.py) on the
    head's own NCHW maps: cls_logits[l] (N, num_classes, H_l, W_l), ctrness[l] (N, 1, H_l, W_l) -> idx (N, Ktot) int32,
    Ktot = sum_l min(k, H_l W_l num_classes), as retinanet_topk: per image, level after level, the flat indices position * num_classes +
    class (offset by the positions of the levels before) of the min(k, passing) greatest scores in stable descending order, then -1."""
    shapes = _fcos_maps("fcos_topk", cls_logits, ctrness, num_classes)
    _check_k("fcos_topk", k)
    for m in (*cls_logits, *ctrness):
        _lib.require_device(m, "fcos_topk input")
    lib = _lib.load()
    l0, n = cls_logits[0], shapes[0][0]
    total = sum(min(k, h * w * num_classes) for _, _, h, w in shapes)
    with _lib.on_device_of(l0):
        maps, cmaps = [_dense_images(m) for m in cls_logits], [_dense_images(m) for m in ctrness]
        idx = torch.empty((n, total), dtype=torch.int32, device=l0.device)
        if n:
            hs, ws, as_ = _tables(shapes)
            nbytes = int(lib.mv_retinanet_topk_workspace_bytes(n, hs, ws, as_, len(maps), num_classes, k))
            if not nbytes:
                raise _lib.Mi355VisionError(f"fcos_topk: {n} images are more than one call takes")
            buf, ws_ptr, nbytes = _lib.workspace(nbytes, l0.device)
            _lib.launch(lib.mv_fcos_topk_f32, l0, _lib.pointer_table(maps), _lib.pointer_table(cmaps), hs, ws, as_, _img_strides(maps),
                        _img_strides(cmaps), len(maps), num_classes, n, k, float(score_thresh), idx.data_ptr(), ws_ptr, nbytes)
    return idx


def fcos_decode(cls_logits: List[torch.Tensor], ctrness: List[torch.Tensor], bbox_regression: List[torch.Tensor], idx: torch.Tensor,
                cell_anchors: List[torch.Tensor], strides: Sequence[Tuple[int, int]], image_sizes,
                num_classes: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The rest of FCOS.postprocess_detections before the nms for the candidates idx (N, K) of fcos_topk, ONE launch, one lane per
    candidate: the anchor of position idx // num_classes from cell_anchors[l] (1, 4) and strides[l], label idx % num_classes,
    BoxLinearCoder(normalize_by_size=True).decode with max(bbox_regression, 0) (the head's ReLU), clip_boxes_to_image, the score
    recomputed -> boxes (N, K, 4), scores (N, K), labels (N, K) int64, valid (N, K) bool (False, with zeros, for the -1 padding and any
    other index outside the pyramid)."""
    name = "fcos_decode"
    shapes = _fcos_maps(name, cls_logits, ctrness, num_classes)
    dshapes = _level_maps(name, bbox_regression, "bbox_regression", 4, [1] * len(shapes)) \
        if isinstance(bbox_regression, (list, tuple)) and len(bbox_regression) == len(cls_logits) else None
    if dshapes is None or dshapes != shapes:
        raise RuntimeError(f"{name}: bbox_regression should hold one map per level of cls_logits, of the same batch and size with 4 channels")
    num, n = len(shapes), shapes[0][0]
    _check_idx(name, idx, n)
    if not isinstance(cell_anchors, (list, tuple)) or len(cell_anchors) != num or any(tuple(c.shape) != (1, 4) for c in cell_anchors):
        raise RuntimeError(f"{name}: cell_anchors should hold one (1, 4) tensor per level")
    _check_strides(name, strides, num)
    sizes = _image_sizes(name, image_sizes, lambda t: tuple(t.shape) == (n, 2), f"{n} rows")
    for m in (*cls_logits, *ctrness, *bbox_regression, idx):
        _lib.require_device(m, f"{name} input")
    lib = _lib.load()
    l0, k = cls_logits[0], int(idx.shape[1])
    with _lib.on_device_of(l0):
        lmaps, cmaps, dmaps = ([_dense_images(m) for m in maps] for maps in (cls_logits, ctrness, bbox_regression))
        base = torch.cat([_lib.table_on(c, l0.device) for c in cell_anchors]).contiguous()
        sizes = _lib.table_on(sizes, l0.device)
        ix = idx.contiguous()
        boxes, scores, labels, valid = _candidate_outputs((n, k), l0.device)
        if n and k:
            hs, ws, as_ = _tables(shapes)
            sh = (C.c_int * num)(*[int(s[0]) for s in strides])
            sw = (C.c_int * num)(*[int(s[1]) for s in strides])
            _lib.launch(lib.mv_fcos_decode_f32, l0, _lib.pointer_table(lmaps), _lib.pointer_table(cmaps), _lib.pointer_table(dmaps), hs, ws, as_,
                        _img_strides(lmaps), _img_strides(cmaps), _img_strides(dmaps), sh, sw, num, num_classes, base.data_ptr(),
                        sizes.data_ptr(), ix.data_ptr(), n, k, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), valid.data_ptr())
    return _candidates(name, (*cls_logits, *ctrness, *bbox_regression), boxes, scores, labels, valid)


def ssd_scores(cls_logits: List[torch.Tensor], num_classes: int) -> torch.Tensor:
    """SSD.postprocess_detections' softmax (ssd.py) on the head's own NCHW class maps, ONE launch for all levels and images:
    cls_logits[l] (N, A_l * num_classes, H_l, W_l) -> scores (N, num_classes, V) float32, CLASS-MAJOR: scores[i, c, v] is the softmax
    over the classes of anchor v = start_l + (y W_l + x) A_l + a of the reference's concatenated layout (channel a * num_classes + c).
    Maximum and exponentials as roi_detections', the sum one ascending float64 chain (mi355vision.h, mv_ssd_scores_f32)."""
    shapes = _class_maps("ssd_scores", cls_logits, num_classes)
    if num_classes < 2:
        raise ValueError(f"ssd_scores: at least 2 classes (the background and one more), got {num_classes}")
    for m in cls_logits:
        _lib.require_device(m, "ssd_scores input")
    lib = _lib.load()
    l0, n = cls_logits[0], shapes[0][0]
    total = sum(a * h * w for _, a, h, w in shapes)
    with _lib.on_device_of(l0):
        maps = [_dense_images(m) for m in cls_logits]
        scores = torch.empty((n, num_classes, total), dtype=torch.float32, device=l0.device)
        if n:
            hs, ws, as_ = _tables(shapes)
            _lib.launch(lib.mv_ssd_scores_f32, l0, _lib.pointer_table(maps), hs, ws, as_, _img_strides(maps), len(maps), num_classes, n,
                        scores.data_ptr())
    return _lib.forward_only(scores, "ssd_scores", *cls_logits)


def ssd_topk(scores: torch.Tensor, k: int, score_thresh: float) -> torch.Tensor:
    """SSD.postprocess_detections' loop over the labels (ssd.py) as ONE launch, one workgroup per (image, class >= 1): scores
    (N, K, V) of ssd_scores -> idx (N, (K - 1) * k) int32.  Segment (c - 1) * k holds the flat indices v * K + c of the
    min(k, passing) anchors with the greatest scores[i, c, v] > score_thresh in stable descending order (equal scores by ascending
    anchor), then -1.  Nothing is read back."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 3:
        raise RuntimeError("ssd_topk: scores should be a 3-D tensor (N, K, V)")
    if scores.dtype != torch.float32:
        raise TypeError(f"ssd_topk computes in float32. Got scores {scores.dtype}")
    n, classes, v = (int(d) for d in scores.shape)
    if classes < 2:
        raise ValueError(f"ssd_topk: at least 2 classes (the background and one more), got {classes}")
    _check_k("ssd_topk", k, reject_bool=True)
    if v * classes >= 2 ** 31:
        raise _lib.Mi355VisionError(f"ssd_topk: {v} anchors x {classes} classes exceed the 32-bit index")
    _lib.require_device(scores, "scores")
    lib = _lib.load()
    with _lib.on_device_of(scores):
        sc = scores.detach().contiguous()
        idx = torch.empty((n, (classes - 1) * k), dtype=torch.int32, device=scores.device)
        if n:
            _lib.launch(lib.mv_ssd_topk_f32, sc, sc.data_ptr(), n, classes, v, k, float(score_thresh), idx.data_ptr())
    return idx


def ssd_decode(scores: torch.Tensor, bbox_regression: List[torch.Tensor], idx: torch.Tensor, wh_pairs: List[torch.Tensor],
               steps: Optional[Sequence[float]], batch_size: Tuple[int, int], image_sizes,
               weights: Tuple[float, float, float, float] = (10.0, 10.0, 5.0, 5.0), clip: bool = True,
               bbox_xform_clip: float = BBOX_XFORM_CLIP) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The rest of SSD.postprocess_detections before the nms for the candidates idx (N, M) of ssd_topk, ONE launch, one lane per
    candidate: anchor idx // K and label idx % K; the default box of DefaultBoxGenerator built in registers from wh_pairs[l]
    ((A_l, 2): the generator's _wh_pairs, clamped to [0, 1] here when `clip`), steps (the generator's, or None: the grid's own size)
    and batch_size = (H, W) of the batch tensor; BoxCoder.decode_single with bbox_regression[l] (N, 4 A_l, H_l, W_l) and `weights`,
    clip_boxes_to_image with image_sizes (N rows (h, w): a list, or an (N, 2) tensor), the score from the matrix -> boxes (N, M, 4),
    scores (N, M), labels (N, M) int64, valid (N, M) bool (False, with zeros, for the -1 padding and any other index outside the
    pyramid)."""
    name = "ssd_decode"
    if not isinstance(wh_pairs, (list, tuple)) or not wh_pairs or \
            any(not isinstance(p, torch.Tensor) or p.dim() != 2 or p.shape[1] != 2 or p.shape[0] < 1 for p in wh_pairs):
        raise RuntimeError(f"{name}: wh_pairs should hold one (A, 2) tensor per level")
    anchors = [int(p.shape[0]) for p in wh_pairs]
    dshapes = _level_maps(name, bbox_regression, "bbox_regression", 4, anchors) \
        if isinstance(bbox_regression, (list, tuple)) and len(bbox_regression) == len(wh_pairs) else None
    if dshapes is None:
        raise RuntimeError(f"{name}: bbox_regression should hold one map per level of wh_pairs, with 4 channels per anchor")
    num, n = len(dshapes), dshapes[0][0]
    total = sum(a * h * w for _, a, h, w in dshapes)
    if not isinstance(scores, torch.Tensor) or scores.dim() != 3 or int(scores.shape[0]) != n or int(scores.shape[2]) != total:
        raise RuntimeError(f"{name}: scores should have shape ({n}, K, {total})")
    if scores.dtype != torch.float32:
        raise TypeError(f"{name} computes in float32. Got scores {scores.dtype}")
    classes = int(scores.shape[1])
    if classes < 2:
        raise ValueError(f"{name}: at least 2 classes (the background and one more), got {classes}")
    if total * classes >= 2 ** 31:
        raise _lib.Mi355VisionError(f"{name}: the anchors of all levels x {classes} classes exceed the 32-bit index")
    _check_idx(name, idx, n, "M")
    if steps is not None and (len(steps) != num or any(not float(s) > 0 for s in steps)):
        raise ValueError(f"{name}: steps should hold one positive step per level, got {steps!r}")
    if len(batch_size) != 2 or int(batch_size[0]) < 1 or int(batch_size[1]) < 1:
        raise ValueError(f"{name}: batch_size should be the (height, width) of the batch tensor, got {batch_size!r}")
    _check_weights(name, weights)
    sizes = _image_sizes(name, image_sizes, lambda t: tuple(t.shape) == (n, 2), f"{n} rows")
    for m in (scores, *bbox_regression, idx):
        _lib.require_device(m, f"{name} input")
    lib = _lib.load()
    d0 = bbox_regression[0]
    m_ = int(idx.shape[1])
    bh, bw = int(batch_size[0]), int(batch_size[1])
    with _lib.on_device_of(d0):
        dmaps = [_dense_images(m) for m in bbox_regression]
        pairs = torch.cat([p.detach().to(torch.float32) for p in wh_pairs])
        if clip:
            pairs = pairs.clamp(min=0, max=1)
        pairs = _lib.table_on(pairs, d0.device)
        sc = scores.detach().contiguous()
        sizes = _lib.table_on(sizes, d0.device)
        ix = idx.contiguous()
        out = _candidate_outputs((n, m_), d0.device)
        if n and m_:
            hs, ws, as_ = _tables(dshapes)
            # the reference divides a float32 tensor by the Python double image side / step (or by the grid's int side)
            x_f = (C.c_float * num)(*[bw / steps[l] if steps is not None else float(dshapes[l][3]) for l in range(num)])
            y_f = (C.c_float * num)(*[bh / steps[l] if steps is not None else float(dshapes[l][2]) for l in range(num)])
            _lib.launch(lib.mv_ssd_decode_f32, d0, sc.data_ptr(), _lib.pointer_table(dmaps), hs, ws, as_, _img_strides(dmaps), num, classes,
                        pairs.data_ptr(), x_f, y_f, bh, bw, sizes.data_ptr(), ix.data_ptr(), n, m_, *[float(w) for w in weights],
                        float(bbox_xform_clip), *[o.data_ptr() for o in out])
    return _candidates(name, (scores, *bbox_regression), *out)


def box_decode(boxes: torch.Tensor, rel_codes: torch.Tensor, weights: Tuple[float, float, float, float],
               bbox_xform_clip: float = BBOX_XFORM_CLIP) -> torch.Tensor:
    """BoxCoder.decode_single (_utils.py): boxes (M, 4) and rel_codes (M, 4 C) -> (M, 4 C), one lane per (box, class)."""
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.size(1) != 4:
        raise RuntimeError("box_decode: boxes should have shape (M, 4)")
    if not isinstance(rel_codes, torch.Tensor) or rel_codes.dim() != 2 or rel_codes.size(0) != boxes.size(0) or rel_codes.size(1) % 4 or \
            (rel_codes.size(1) == 0 and rel_codes.size(0) > 0):
        raise RuntimeError(f"box_decode: rel_codes should have shape ({boxes.size(0)}, 4 C), got {tuple(rel_codes.shape)}")
    if boxes.dtype != torch.float32 or rel_codes.dtype != torch.float32:
        raise TypeError(f"box_decode computes in float32. Got boxes {boxes.dtype}, rel_codes {rel_codes.dtype}")
    _check_weights("box_decode", weights)
    _lib.require_device(rel_codes, "rel_codes")
    _lib.require_device(boxes, "boxes")
    lib = _lib.load()
    m, c4 = int(rel_codes.size(0)), int(rel_codes.size(1))
    with _lib.on_device_of(rel_codes):
        b, r = boxes.detach().to(rel_codes.device).contiguous(), rel_codes.detach().contiguous()
        out = torch.empty((m, c4), dtype=torch.float32, device=rel_codes.device)
        if m:
            _lib.launch(lib.mv_box_decode_f32, r, b.data_ptr(), r.data_ptr(), out.data_ptr(), m, c4 // 4, *[float(w) for w in weights],
                        float(bbox_xform_clip))
    return _lib.forward_only(out, "box_decode", boxes, rel_codes)


def _rows(m: torch.Tensor) -> torch.Tensor:
    """The matrix itself when its rows are dense (a column slice of a wider contiguous tensor is), else a contiguous copy."""
    m = m.detach()
    if m.stride(1) == 1 and (m.shape[0] <= 1 or m.stride(0) >= m.shape[1]):
        return m
    return m.contiguous()


def roi_detections(class_logits: torch.Tensor, box_regression: torch.Tensor, rois: torch.Tensor, image_sizes,
                   weights: Tuple[float, float, float, float] = (10.0, 10.0, 5.0, 5.0), bbox_xform_clip: float = BBOX_XFORM_CLIP,
                   score_thresh: float = 0.05, min_size: float = 1e-2) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """RoIHeads.postprocess_detections (roi_heads.py) up to the per-image filters, ONE launch, one wave per roi: softmax of
    class_logits (R, C), BoxCoder.decode_single of rois[:, 1:5] with box_regression (R, 4 C) and `weights`, clip_boxes_to_image with
    image_sizes (N rows (h, w): a list, or an (N, 2) tensor) of image rois[:, 0], the background class dropped -> boxes (R, C - 1, 4),
    scores (R, C - 1), labels (R, C - 1) int64 (column j - 1 holds class j), valid (R, C - 1) bool = score > score_thresh and both
    sides >= min_size.  class_logits and box_regression may be column slices of one tensor: they are passed by their row strides."""
    if not isinstance(class_logits, torch.Tensor) or class_logits.dim() != 2:
        raise RuntimeError("roi_detections: class_logits should have shape (R, C)")
    r, c = int(class_logits.shape[0]), int(class_logits.shape[1])
    if not isinstance(box_regression, torch.Tensor) or tuple(box_regression.shape) != (r, 4 * c):
        raise RuntimeError(f"roi_detections: box_regression should have shape ({r}, {4 * c}), got "
                           f"{tuple(box_regression.shape) if isinstance(box_regression, torch.Tensor) else type(box_regression).__name__}")
    if not isinstance(rois, torch.Tensor) or tuple(rois.shape) != (r, 5):
        raise RuntimeError(f"roi_detections: rois should have shape ({r}, 5): (image index, x1, y1, x2, y2)")
    if class_logits.dtype != torch.float32 or box_regression.dtype != torch.float32 or rois.dtype != torch.float32:
        raise TypeError(f"roi_detections computes in float32. Got class_logits {class_logits.dtype}, box_regression {box_regression.dtype}, "
                        f"rois {rois.dtype}")
    if c < 2:
        raise ValueError(f"roi_detections: at least 2 classes (the background and one more), got {c}")
    if c > MAX_ROI_CLASSES:
        raise _lib.Mi355VisionError(f"roi_detections: up to {MAX_ROI_CLASSES} classes, got {c}")
    if r * c >= 2 ** 31:
        raise _lib.Mi355VisionError(f"roi_detections: {r} rois x {c} classes exceed the 32-bit index")
    _check_weights("roi_detections", weights)
    sizes = _image_sizes("roi_detections", image_sizes, lambda t: t.dim() == 2 and t.shape[1] == 2 and (r == 0 or t.shape[0] >= 1),
                         "at least one row")
    for m in (class_logits, box_regression, rois):
        _lib.require_device(m, "roi_detections input")
    lib = _lib.load()
    dev = class_logits.device
    with _lib.on_device_of(class_logits):
        lg, dl = _rows(class_logits), _rows(box_regression)
        rs = rois.detach().to(dev).contiguous()
        sizes = _lib.table_on(sizes, dev)
        out = _candidate_outputs((r, c - 1), dev)
        if r:
            _lib.launch(lib.mv_roi_detections_f32, lg, lg.data_ptr(), int(lg.stride(0)) if r > 1 else c, dl.data_ptr(),
                        int(dl.stride(0)) if r > 1 else 4 * c, rs.data_ptr(), sizes.data_ptr(), r, c, int(sizes.shape[0]),
                        *[float(w) for w in weights], float(bbox_xform_clip), float(score_thresh), float(min_size),
                        *[o.data_ptr() for o in out])
    return _candidates("roi_detections", (class_logits, box_regression, rois), *out)
