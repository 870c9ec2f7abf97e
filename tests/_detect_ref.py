"""References for ops.nms / ops.roi_align: the reference's CPU kernels (csrc/ops/cpu/nms_kernel.cpp, roi_align_kernel.cpp with
roi_align_common.h) restated in numpy, one rounded operation at a time.  Imports nothing from the package.

float32 numpy scalars and arrays round every elementwise operation once and never fuse a multiply with an add, which is what the
reference's scalar loops do in a CPU build.  The loops run element by element over boxes (nms) and over rois, bins and samples
(roi_align); the only vector axis is one over which the reference performs the same independent scalar operation (the candidate
boxes j of one kept box i; the channels of one sample), so the rounding of every element is that of the scalar loop.

  nms_ref(boxes, scores, thr)                         kept indices, int64, in score order (scores without NaN)
  roi_align_ref(x, rois, out, scale, ratio, aligned, dtype)   dtype np.float32 (the restatement) or np.float64 (the yardstick)
  iou_matrix64 / tie_margin_ok / make_boxes           the input condition of the nms tests
  roi_cases(...)                                      the rois of the roi_align tests
"""
import numpy as np

F32 = np.float32


def nms_ref(boxes, scores, iou_threshold):
    """nms_kernel_impl<float>: greedy loop over the stable descending score order; `ovr > iou_threshold` compares the float32
    quotient with the double threshold."""
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=F32)
    n = boxes.shape[0]
    if n == 0:
        return np.zeros((0,), dtype=np.int64)
    x1, y1, x2, y2 = (boxes[:, i].copy() for i in range(4))
    areas = (x2 - x1) * (y2 - y1)
    order = np.argsort(-scores, kind="stable")  # descending, equal scores in index order
    suppressed = np.zeros(n, dtype=bool)
    keep = []
    thr = np.float64(iou_threshold)
    zero = F32(0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _i in range(n):
            i = order[_i]
            if suppressed[i]:
                continue
            keep.append(i)
            js = order[_i + 1:]
            xx1, yy1 = np.maximum(x1[i], x1[js]), np.maximum(y1[i], y1[js])
            xx2, yy2 = np.minimum(x2[i], x2[js]), np.minimum(y2[i], y2[js])
            w, h = np.maximum(zero, xx2 - xx1), np.maximum(zero, yy2 - yy1)
            inter = w * h
            ovr = inter / (areas[i] + areas[js] - inter)
            assert ovr.dtype == F32
            suppressed[js[ovr.astype(np.float64) > thr]] = True
    return np.asarray(keep, dtype=np.int64)


def iou_matrix64(boxes):
    """(iou, inter) of every pair in float64."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(0.0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
    h = np.maximum(0.0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area[:, None] + area[None, :] - inter), inter


def tie_margin_ok(boxes, iou_threshold, margin=1e-6):
    """The input condition of the nms tests: no pair's IoU lies within `margin` of the threshold.  Two kinds of pair have an IoU
    that no evaluation order can move and are exempt: an empty intersection (inter == 0 exactly, IoU 0 or 0 / 0) and two
    identical boxes of positive area (a / ((a + a) - a) == 1 exactly) -- without them thresholds 0 and 1 could not be tested on
    disjoint or identical boxes at all."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    iou, inter = iou_matrix64(b)
    same = (b[:, None, :] == b[None, :, :]).all(-1)
    exact = (inter == 0) | same | ~np.isfinite(iou)
    np.fill_diagonal(exact, True)
    return not bool((~exact & (np.abs(iou - iou_threshold) <= margin)).any())


def make_boxes(kind, n, seed):
    """(boxes (n, 4) float32, scores (n) float32) of one family:
      clustered   boxes jittered around n // 8 + 1 centres, so that many are suppressed
      identical   one box n times
      disjoint    a grid of boxes with gaps
      ties        clustered, with scores drawn from 4 values only (the stable order decides)
      degenerate  clustered, every third box of zero width, height or both"""
    g = np.random.default_rng(seed)
    if kind == "identical":
        return np.tile(np.array([[10.0, 20.0, 50.0, 80.0]], dtype=F32), (n, 1)), g.random(n).astype(F32)
    if kind == "disjoint":
        idx = np.arange(n)
        x, y = (idx % 32) * 12.0, (idx // 32) * 12.0
        return np.stack([x, y, x + 10.0, y + 10.0], 1).astype(F32), g.random(n).astype(F32)
    centres = g.random((n // 8 + 1, 2)) * 200.0
    c = centres[g.integers(0, len(centres), n)] + g.normal(0.0, 4.0, (n, 2))
    wh = 20.0 + g.random((n, 2)) * 30.0
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F32)
    scores = g.random(n).astype(F32)
    if kind == "ties":
        scores = (g.integers(0, 4, n) * 0.25).astype(F32)
    elif kind == "degenerate":
        for i in range(0, n, 3):
            if i % 2 == 0:
                boxes[i, 2] = boxes[i, 0]
            if i % 9 != 0:
                boxes[i, 3] = boxes[i, 1]
    else:
        assert kind == "clustered", kind
    return boxes, scores


def boxes_with_margin(kind, n, thresholds, seed=0, max_seeds=20):
    """make_boxes at the first seed >= `seed` whose boxes satisfy tie_margin_ok for every threshold -> (boxes, scores, seed)."""
    for s in range(seed, seed + max_seeds):
        boxes, scores = make_boxes(kind, n, s)
        if all(tie_margin_ok(boxes, t) for t in thresholds):
            return boxes, scores, s
    raise AssertionError(f"no seed in [{seed}, {seed + max_seeds}) gives {kind} boxes clear of the thresholds {thresholds}")


def roi_align_ref(x, rois, output_size, spatial_scale, sampling_ratio, aligned, dtype=F32):
    """roi_align_forward_kernel_impl<T> with pre_calc_for_bilinear_interpolate folded in, T = dtype."""
    T = dtype
    x = np.asarray(x, dtype=T)
    rois = np.asarray(rois, dtype=T).reshape(-1, 5)
    n, c, height, width = x.shape
    ph_n, pw_n = output_size
    out = np.zeros((rois.shape[0], c, ph_n, pw_n), dtype=T)
    scale, half, one, zero = T(spatial_scale), T(0.5), T(1), T(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(rois.shape[0]):
            roi = rois[k]
            b = int(roi[0])
            if not 0 <= b < n:
                continue  # mv_roi_align_f32 writes zeros for a batch index outside the input (the reference would read outside it)
            offset = half if aligned else zero
            start_w, start_h = roi[1] * scale - offset, roi[2] * scale - offset
            end_w, end_h = roi[3] * scale - offset, roi[4] * scale - offset
            roi_w, roi_h = end_w - start_w, end_h - start_h
            if not aligned:
                roi_w, roi_h = max(roi_w, one), max(roi_h, one)
            bin_h, bin_w = roi_h / T(ph_n), roi_w / T(pw_n)
            grid_h = sampling_ratio if sampling_ratio > 0 else int(np.ceil(roi_h / T(ph_n)))
            grid_w = sampling_ratio if sampling_ratio > 0 else int(np.ceil(roi_w / T(pw_n)))
            count = T(max(grid_h * grid_w, 1))
            planes = x[b].reshape(c, -1)
            for ph in range(ph_n):
                for pw in range(pw_n):
                    val = np.zeros(c, dtype=T)
                    for iy in range(grid_h):
                        yy = start_h + T(ph) * bin_h + (T(iy) + half) * bin_h / T(grid_h)
                        for ix in range(grid_w):
                            xx = start_w + T(pw) * bin_w + (T(ix) + half) * bin_w / T(grid_w)
                            y, xq = yy, xx
                            if y < -1.0 or y > height or xq < -1.0 or xq > width:
                                w1 = w2 = w3 = w4 = zero
                                p1 = p2 = p3 = p4 = 0
                            else:
                                y, xq = (zero if y <= 0 else y), (zero if xq <= 0 else xq)
                                y_low, x_low = int(y), int(xq)
                                if y_low >= height - 1:
                                    y_high = y_low = height - 1
                                    y = T(y_low)
                                else:
                                    y_high = y_low + 1
                                if x_low >= width - 1:
                                    x_high = x_low = width - 1
                                    xq = T(x_low)
                                else:
                                    x_high = x_low + 1
                                ly, lx = y - T(y_low), xq - T(x_low)
                                hy, hx = one - ly, one - lx
                                w1, w2, w3, w4 = hy * hx, hy * lx, ly * hx, ly * lx
                                p1, p2 = y_low * width + x_low, y_low * width + x_high
                                p3, p4 = y_high * width + x_low, y_high * width + x_high
                            s = w1 * planes[:, p1] + w2 * planes[:, p2] + w3 * planes[:, p3] + w4 * planes[:, p4]
                            assert s.dtype == T
                            val = val + s
                    out[k, :, ph, pw] = val / count
    return out


def convert_boxes_to_roi_format_ref(boxes):
    """ops/_utils.py convert_boxes_to_roi_format on numpy arrays: (L_i, 4) per image -> (K, 5) with the image index in front."""
    rows = [np.concatenate([np.full((len(b), 1), i, dtype=b.dtype), b], 1) for i, b in enumerate(boxes)]
    return np.concatenate(rows, 0)


def roi_cases(h, w, spatial_scale, batch=2, extra=0, seed=0):
    """(k, 5) float32 rois in INPUT-IMAGE coordinates (map coordinates / spatial_scale) for an (h, w) map: inside, touching each
    border, fully outside on each side, zero and negative size, larger than the map, batch indices 0 .. batch - 1; `extra` more
    random ones."""
    s = 1.0 / spatial_scale
    W, H = float(w), float(h)
    base = [
        (0, 2.3, 1.7, 9.6, 8.2),                # inside
        (batch - 1, 3.0, 2.0, 11.0, 10.0),      # inside, integer corners, the last image
        (0, 0.0, 1.5, 5.5, 6.5),                # touches the left border
        (batch - 1, 4.5, 0.0, 9.5, 4.0),        # the top
        (0, W - 6.0, 2.0, W, 7.0),              # the right
        (batch - 1, 2.0, H - 5.0, 8.0, H),      # the bottom
        (0, 0.0, 0.0, W, H),                    # the whole map
        (batch - 1, -30.0, -30.0, -12.0, -15.0),  # fully outside, up and left
        (0, W + 4.0, H + 3.0, W + 20.0, H + 9.0),  # fully outside, down and right
        (0, -0.7, -0.9, 3.2, 2.8),              # straddles the corner: samples in (-1, 0)
        (batch - 1, 5.0, 5.0, 5.0, 5.0),        # zero size
        (0, 9.0, 8.0, 4.0, 3.0),                # negative size
        (batch - 1, -8.0, -6.25, W + 9.0, H + 7.5),  # larger than the map (no sample of the tested grids exactly on a border)
        (0, 6.25, 4.75, 6.75, 12.0),            # thin
    ]
    rois = np.array(base, dtype=np.float64)
    if extra:
        g = np.random.default_rng(seed)
        p = np.stack([g.random(extra) * (W + 4) - 2, g.random(extra) * (H + 4) - 2], 1)
        q = p + np.stack([g.random(extra) * W * 0.6, g.random(extra) * H * 0.6], 1)
        more = np.concatenate([g.integers(0, batch, (extra, 1)).astype(np.float64), p, q], 1)
        rois = np.concatenate([rois, more], 0)
    rois[:, 1:] *= s
    return rois.astype(F32)
