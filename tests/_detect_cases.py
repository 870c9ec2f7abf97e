"""The cases tests/test_detect_host.py, test_gpu_detect.py and test_gpu_detect_guard.py share, and their references
(tests/_detect_ref.py), each computed once per process and never modified (the arrays are read-only)."""
import functools
import itertools

import numpy as np

from tests import _detect_ref as R

# nms: sizes across the 64-box tile and the word boundaries; thresholds; box families (R.make_boxes)
NMS_SIZES = (0, 1, 2, 63, 64, 65, 130, 1000)
NMS_THRESHOLDS = (0.0, 0.5, 1.0)
NMS_KINDS = ("clustered", "identical", "disjoint", "ties", "degenerate")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def nms_case(kind, n):
    """(boxes, scores) of `kind` with n boxes, clear of every threshold in NMS_THRESHOLDS (R.tie_margin_ok)."""
    if n == 0:
        return _frozen(np.zeros((0, 4), np.float32), np.zeros((0,), np.float32))
    boxes, scores, _ = R.boxes_with_margin(kind, n, NMS_THRESHOLDS, seed=n)
    return _frozen(boxes, scores)


@functools.lru_cache(maxsize=None)
def nms_reference(kind, n, thr):
    boxes, scores = nms_case(kind, n)
    return _frozen(R.nms_ref(boxes, scores, thr))[0]


# roi_align: (output_size, sampling_ratio, aligned, spatial_scale)
ROI_CONFIGS = tuple(itertools.product(((1, 1), (2, 3), (7, 7)), (-1, 1, 2), (False, True), (1.0, 0.25)))
ROI_SHAPES = {"main": (2, 5, 13, 17), "tiny": (1, 3, 1, 1)}


@functools.lru_cache(maxsize=None)
def roi_input(shape):
    n, c, h, w = ROI_SHAPES[shape]
    g = np.random.default_rng(17 + h)
    return _frozen((g.random((n, c, h, w)) * 2 - 1).astype(np.float32))[0]


@functools.lru_cache(maxsize=None)
def roi_rois(shape, spatial_scale, extra=0):
    n, _, h, w = ROI_SHAPES[shape]
    return _frozen(R.roi_cases(h, w, spatial_scale, batch=n, extra=extra, seed=3))[0]


@functools.lru_cache(maxsize=None)
def roi_reference(shape, cfg, extra=0):
    """-> (float32 restatement, float64 evaluation, rois) for ROI_SHAPES[shape] under cfg."""
    out, ratio, aligned, scale = cfg
    x, rois = roi_input(shape), roi_rois(shape, scale, extra)
    f32 = R.roi_align_ref(x, rois, out, scale, ratio, aligned, np.float32)
    f64 = R.roi_align_ref(x, rois, out, scale, ratio, aligned, np.float64)
    return _frozen(f32, f64) + (rois,)
