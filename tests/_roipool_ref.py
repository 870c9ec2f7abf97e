"""References for ops.roi_pool / ps_roi_pool / ps_roi_align: the reference's CPU kernels (csrc/ops/cpu/roi_pool_kernel.cpp,
ps_roi_pool_kernel.cpp, ps_roi_align_kernel.cpp) restated in numpy scalars, one rounded operation at a time, as
tests/_detect_ref.py restates roi_align.  Imports nothing from the package.

`dtype` is np.float32 (the restatement) or np.float64 (the yardstick).  The loops run roi by roi, bin by bin and element by
element; the only vector axis is the channels, over which the reference performs the same independent scalar operation.

  roi_pool_ref(x, rois, out, scale, dtype)              -> (y, argmax int32)
  ps_roi_pool_ref(x, rois, out, scale, dtype)           -> (y, channel_mapping int32)
  ps_roi_align_ref(x, rois, out, scale, ratio, dtype)   -> (y, channel_mapping int32)
  pool_windows(rois, out, scale, h, w, dtype, ps)       (k, PH, PW, 4) int64: hstart, hend, wstart, wend of every bin
  adaptive_grids(rois, out, scale, dtype)               (k, 2) int64: grid_h, grid_w of ps_roi_align with sampling_ratio <= 0

A roi whose batch index does not truncate into [0, n) (or is NaN) gives zeros and -1 (roi_pool) or the mapping, as the entry
points do (the reference would read outside the input)."""
import math

import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
CORNER_LIMIT = float(2 ** 29)


def roundf(p):
    """C's roundf (half away from zero) of a float32 or float64 scalar: the value widened to a Python float, then
    copysign(floor(|p| + 0.5), p).  Exact for a float32 p: |p| + 0.5 is representable in double whenever it has a fraction.
    (np.round would round half to even.)"""
    p = float(p)
    if math.isnan(p):
        return p
    if math.isinf(p):
        return p
    return math.copysign(math.floor(abs(p) + 0.5), p)


def rounded_corner(v, scale, T):
    """(int)roundf(v * scale) with the entry points' guard: NaN -> 0, the rounded value clamped to +-2^29."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = roundf(T(v) * T(scale))
    if math.isnan(r):
        return 0
    return int(min(max(r, -CORNER_LIMIT), CORNER_LIMIT))


def _batch_index(bf, n):
    """-> b, or None when !(bf > -1 && bf < n)."""
    bf = float(bf)
    if not (bf > -1.0 and bf < n):
        return None
    return int(bf)


def _clamp(v, hi):
    return min(max(v, 0), hi)


def _window(roi, out, scale, h, w, T, ps, ph, pw):
    ph_n, pw_n = out
    start_w, start_h = rounded_corner(roi[1], scale, T), rounded_corner(roi[2], scale, T)
    end_w, end_h = rounded_corner(roi[3], scale, T), rounded_corner(roi[4], scale, T)
    if ps:
        roi_w, roi_h = max(end_w - start_w, 1), max(end_h - start_h, 1)
    else:
        roi_w, roi_h = max(end_w - start_w + 1, 1), max(end_h - start_h + 1, 1)
    bin_h, bin_w = T(roi_h) / T(ph_n), T(roi_w) / T(pw_n)
    if ps:
        hstart, hend = math.floor(T(ph) * bin_h + T(start_h)), math.ceil(T(ph + 1) * bin_h + T(start_h))
        wstart, wend = math.floor(T(pw) * bin_w + T(start_w)), math.ceil(T(pw + 1) * bin_w + T(start_w))
    else:
        hstart, hend = math.floor(T(ph) * bin_h) + start_h, math.ceil(T(ph + 1) * bin_h) + start_h
        wstart, wend = math.floor(T(pw) * bin_w) + start_w, math.ceil(T(pw + 1) * bin_w) + start_w
    return _clamp(hstart, h), _clamp(hend, h), _clamp(wstart, w), _clamp(wend, w)


def pool_windows(rois, output_size, spatial_scale, h, w, dtype=F32, ps=False):
    """The clamped window of every bin of every roi, computed in `dtype`."""
    rois = np.asarray(rois, dtype=dtype).reshape(-1, 5)
    ph_n, pw_n = output_size
    win = np.zeros((rois.shape[0], ph_n, pw_n, 4), dtype=np.int64)
    for k in range(rois.shape[0]):
        for ph in range(ph_n):
            for pw in range(pw_n):
                win[k, ph, pw] = _window(rois[k], output_size, spatial_scale, h, w, dtype, ps, ph, pw)
    return win


def roi_pool_ref(x, rois, output_size, spatial_scale, dtype=F32):
    """roi_pool_forward_kernel_impl<T>, T = dtype."""
    T = dtype
    x = np.asarray(x, dtype=T)
    rois = np.asarray(rois, dtype=T).reshape(-1, 5)
    n, c, height, width = x.shape
    ph_n, pw_n = output_size
    out = np.zeros((rois.shape[0], c, ph_n, pw_n), dtype=T)
    argmax = np.full((rois.shape[0], c, ph_n, pw_n), -1, dtype=np.int32)
    for k in range(rois.shape[0]):
        b = _batch_index(rois[k, 0], n)
        if b is None:
            continue
        planes = x[b].reshape(c, -1)
        for ph in range(ph_n):
            for pw in range(pw_n):
                hstart, hend, wstart, wend = _window(rois[k], output_size, spatial_scale, height, width, T, False, ph, pw)
                empty = hend <= hstart or wend <= wstart
                maxval = np.full(c, 0.0 if empty else -FLT_MAX, dtype=T)
                maxidx = np.full(c, -1, dtype=np.int32)
                for hh in range(hstart, hend):
                    for ww in range(wstart, wend):
                        v = planes[:, hh * width + ww]
                        take = v > maxval  # strict, and False for a NaN
                        maxval = np.where(take, v, maxval)
                        maxidx = np.where(take, np.int32(hh * width + ww), maxidx)
                out[k, :, ph, pw] = maxval
                argmax[k, :, ph, pw] = maxidx
    return out, argmax


def _mapping(k, c_out, ph_n, pw_n):
    co, ph, pw = np.meshgrid(np.arange(c_out), np.arange(ph_n), np.arange(pw_n), indexing="ij")
    m = ((co * ph_n + ph) * pw_n + pw).astype(np.int32)
    return np.broadcast_to(m, (k, c_out, ph_n, pw_n)).copy()


def ps_roi_pool_ref(x, rois, output_size, spatial_scale, dtype=F32):
    """ps_roi_pool_forward_kernel_impl<T>, T = dtype."""
    T = dtype
    x = np.asarray(x, dtype=T)
    rois = np.asarray(rois, dtype=T).reshape(-1, 5)
    n, c, height, width = x.shape
    ph_n, pw_n = output_size
    assert c % (ph_n * pw_n) == 0
    c_out = c // (ph_n * pw_n)
    out = np.zeros((rois.shape[0], c_out, ph_n, pw_n), dtype=T)
    mapping = _mapping(rois.shape[0], c_out, ph_n, pw_n)
    for k in range(rois.shape[0]):
        b = _batch_index(rois[k, 0], n)
        if b is None:
            continue
        planes = x[b].reshape(c, -1)
        for ph in range(ph_n):
            for pw in range(pw_n):
                hstart, hend, wstart, wend = _window(rois[k], output_size, spatial_scale, height, width, T, True, ph, pw)
                if hend <= hstart or wend <= wstart:
                    continue
                c_in = mapping[k, :, ph, pw]
                s = np.zeros(c_out, dtype=T)
                for hh in range(hstart, hend):
                    for ww in range(wstart, wend):
                        s = s + planes[c_in, hh * width + ww]
                assert s.dtype == T
                out[k, :, ph, pw] = s / T((hend - hstart) * (wend - wstart))
    return out, mapping


def _grid(roi_size, pooled, T):
    return int(np.ceil(roi_size / T(pooled)))


def adaptive_grids(rois, output_size, spatial_scale, dtype=F32):
    T = dtype
    rois = np.asarray(rois, dtype=T).reshape(-1, 5)
    scale, half = T(spatial_scale), T(0.5)
    g = np.zeros((rois.shape[0], 2), dtype=np.int64)
    for k, roi in enumerate(rois):
        roi_w = (roi[3] * scale - half) - (roi[1] * scale - half)
        roi_h = (roi[4] * scale - half) - (roi[2] * scale - half)
        g[k] = _grid(roi_h, output_size[0], T), _grid(roi_w, output_size[1], T)
    return g


def ps_roi_align_ref(x, rois, output_size, spatial_scale, sampling_ratio, dtype=F32):
    """ps_roi_align_forward_kernel_impl<T>, T = dtype, with the bilinear sample of tests/_detect_ref.roi_align_ref."""
    T = dtype
    x = np.asarray(x, dtype=T)
    rois = np.asarray(rois, dtype=T).reshape(-1, 5)
    n, c, height, width = x.shape
    ph_n, pw_n = output_size
    assert c % (ph_n * pw_n) == 0
    c_out = c // (ph_n * pw_n)
    out = np.zeros((rois.shape[0], c_out, ph_n, pw_n), dtype=T)
    mapping = _mapping(rois.shape[0], c_out, ph_n, pw_n)
    scale, half, one, zero = T(spatial_scale), T(0.5), T(1), T(0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(rois.shape[0]):
            roi = rois[k]
            b = _batch_index(roi[0], n)
            if b is None:
                continue
            start_w, start_h = roi[1] * scale - half, roi[2] * scale - half
            end_w, end_h = roi[3] * scale - half, roi[4] * scale - half
            roi_w, roi_h = end_w - start_w, end_h - start_h
            bin_h, bin_w = roi_h / T(ph_n), roi_w / T(pw_n)
            grid_h = sampling_ratio if sampling_ratio > 0 else _grid(roi_h, ph_n, T)
            grid_w = sampling_ratio if sampling_ratio > 0 else _grid(roi_w, pw_n, T)
            count = T(grid_h * grid_w)
            planes = x[b].reshape(c, -1)
            for ph in range(ph_n):
                hstart = T(ph) * bin_h + start_h
                for pw in range(pw_n):
                    wstart = T(pw) * bin_w + start_w
                    c_in = mapping[k, :, ph, pw]
                    val = np.zeros(c_out, dtype=T)
                    for iy in range(grid_h):
                        yy = hstart + (T(iy) + half) * bin_h / T(grid_h)
                        for ix in range(grid_w):
                            xx = wstart + (T(ix) + half) * bin_w / T(grid_w)
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
                            s = w1 * planes[c_in, p1] + w2 * planes[c_in, p2] + w3 * planes[c_in, p3] + w4 * planes[c_in, p4]
                            assert s.dtype == T
                            val = val + s
                    out[k, :, ph, pw] = val / count  # count 0: 0 / 0 = NaN, as the reference's loop
    return out, mapping
