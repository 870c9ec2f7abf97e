"""The cases tests/test_roipool_host.py, test_gpu_roipool.py and test_gpu_roipool_guard.py share, and their references
(tests/_roipool_ref.py), each computed once per process and never modified (the arrays are read-only).  The rois are those of the
roi_align tests (tests/_detect_ref.roi_cases through tests/_detect_cases.roi_rois)."""
import functools
import itertools

import numpy as np

from tests import _roipool_ref as P
from tests._detect_cases import ROI_SHAPES, _frozen, roi_rois

OUTPUTS = ((1, 1), (2, 3), (7, 7))
SCALES = (1.0, 0.25)
RATIOS = (-1, 1, 2)
# (output_size, spatial_scale) for the two pooling ops; (output_size, spatial_scale, sampling_ratio) for ps_roi_align
POOL_CONFIGS = tuple(itertools.product(OUTPUTS, SCALES))
PS_ALIGN_CONFIGS = tuple(itertools.product(OUTPUTS, SCALES, RATIOS))
SHAPES = ("main", "tiny")
OPS = ("roi_pool", "ps_roi_pool", "ps_roi_align")
# rows of R.roi_cases: the roi of zero size and the one of negative size
DEGENERATE_ROIS = (10, 11)


def input_shape(op, shape, out):
    """(n, c, h, w): ROI_SHAPES for roi_pool; c = 2 PH PW on the 13 x 17 map and PH PW on the 1 x 1 map for the position-sensitive ops."""
    n, c, h, w = ROI_SHAPES[shape]
    if op != "roi_pool":
        c = (2 if shape == "main" else 1) * out[0] * out[1]
    return n, c, h, w


@functools.lru_cache(maxsize=None)
def pool_input(op, shape, out):
    n, c, h, w = input_shape(op, shape, out)
    g = np.random.default_rng(29 + h + c)
    return _frozen((g.random((n, c, h, w)) * 2 - 1).astype(np.float32))[0]  # in [-1, 1)


@functools.lru_cache(maxsize=None)
def pool_reference(op, shape, cfg, extra=0):
    """-> ((y, second) in float32, (y, second) in float64, rois) of `op` on SHAPES[shape] under cfg."""
    out, scale = cfg[0], cfg[1]
    x, rois = pool_input(op, shape, out), roi_rois(shape, scale, extra)
    if op == "roi_pool":
        f32, f64 = (P.roi_pool_ref(x, rois, out, scale, t) for t in (np.float32, np.float64))
    elif op == "ps_roi_pool":
        f32, f64 = (P.ps_roi_pool_ref(x, rois, out, scale, t) for t in (np.float32, np.float64))
    else:
        f32, f64 = (P.ps_roi_align_ref(x, rois, out, scale, cfg[2], t) for t in (np.float32, np.float64))
    return _frozen(*f32), _frozen(*f64), rois


def same_as_aligned_roi_align(y, mapping, full, ratio, what):
    """Asserts the relation the shared bin sampler (csrc/mv_roi.h) embodies: ps_roi_align's float32 output `y` is, bit for bit,
    the output `full` of roi_align(aligned=True) on the same map and rois, gathered along channels by `mapping`.  Excluded are only
    the elements of the DEGENERATE_ROIS rows that ps_roi_align makes NaN with an adaptive grid (ratio <= 0): there the divisor
    differs by contract, the bare grid_h * grid_w against roi_align's max(.., 1).  The zero-size roi is such a row at every output
    size."""
    y, full = np.ascontiguousarray(y), np.ascontiguousarray(full)
    assert y.dtype == full.dtype == np.float32 and full.shape[1] == y.shape[1] * y.shape[2] * y.shape[3], what
    gathered = np.ascontiguousarray(np.take_along_axis(full, mapping.astype(np.int64), axis=1))
    excluded = np.zeros(y.shape, bool)
    if ratio <= 0:
        excluded[list(DEGENERATE_ROIS)] = np.isnan(y[list(DEGENERATE_ROIS)])
        assert excluded[DEGENERATE_ROIS[0]].all(), f"{what}: the zero-size roi is not NaN throughout"
    assert np.isnan(y[excluded]).all()
    differ = (y.view(np.uint32) != gathered.view(np.uint32)) & ~excluded
    assert not differ.any(), f"{what}: {int(differ.sum())} of {y.size} elements differ, in rois {np.flatnonzero(differ.any((1, 2, 3))).tolist()}"


def configs(op):
    return PS_ALIGN_CONFIGS if op == "ps_roi_align" else POOL_CONFIGS
