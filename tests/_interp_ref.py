"""The oracle of F.interpolate / F.detection_batch and of the detection transform's size rule: the formula that
include/mi355vision.h states for mv_interpolate_bilinear_f32, restated in numpy float32.

A float32 fma is computed as the float64 product (exact: 24 + 24 bits) plus the addend, rounded to float32.  The float64 sum is
itself rounded, so it is first rounded TO ODD (the error of the sum from TwoSum; 53 >= 24 + 2 bits): the float32 rounding of that is
the correctly rounded fma in every case, not only almost always.

  axis_taps(n_in, n_out)             i0, i1, w0, w1 of every output index of one axis
  interpolate(x, oh, ow, rows=None)  (..., h, w) float32 -> (..., oh, ow), or only the output rows `rows`
  fma32_torch(a, b, c)               the same fma with torch ops, on any device
  normalize(x, mean, std)            torch float32 sub / div, as the reference's transform
  detection_batch(images, sizes, mean, std, size_divisible)   normalize -> interpolate -> zero-padded batch
  resized_size / scripted_resized_size    the reference's eager and scripted size rules
"""
import math

import numpy as np
import torch

F32 = np.float32


def fma32(a, b, c):
    """round_to_float32(a * b + c) for float32 arrays, one rounding."""
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)  # exact
        c = np.broadcast_to(np.asarray(c, dtype=F32).astype(np.float64), p.shape)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)  # TwoSum: p + c == s + err exactly
        bits = s.copy().view(np.int64)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
        away = (err > 0) == (s > 0)  # the exact sum lies farther from zero than s
        bits[fix & away] += 1
        bits[fix & ~away] -= 1
        return bits.view(np.float64).astype(F32)


def axis_taps(n_in, n_out):
    s = F32(n_in) / F32(n_out)
    d = np.arange(n_out, dtype=F32)
    src = np.maximum(fma32(np.full(n_out, s, F32), d + F32(0.5), F32(-0.5)), F32(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = np.clip(src - i0.astype(F32), F32(0), F32(1)).astype(F32)
    return i0, i1, (F32(1) - lam).astype(F32), lam


def interpolate(x, oh, ow, rows=None):
    """rows: a slice or index array of output rows to compute (default: all oh)."""
    x = np.asarray(x, dtype=F32)
    h, w = x.shape[-2:]
    y0, y1, wy0, wy1 = axis_taps(h, oh)
    if rows is not None:
        y0, y1, wy0, wy1 = y0[rows], y1[rows], wy0[rows], wy1[rows]
    x0, x1, wx0, wx1 = axis_taps(w, ow)
    top, bot = x[..., y0, :], x[..., y1, :]
    with np.errstate(all="ignore"):
        t = fma32(wx0, top[..., x0], wx1 * top[..., x1])
        u = fma32(wx0, bot[..., x0], wx1 * bot[..., x1])
        wy0, wy1 = wy0[:, None], wy1[:, None]
        return fma32(np.broadcast_to(wy0, t.shape), t, wy1 * u)


def fma32_torch(a, b, c):
    """fma32 on float32 torch tensors of any device, with torch's float64 ops (each one IEEE operation): for references too large
    for the host."""
    p = a.double() * b.double()
    c = c.double().expand_as(p)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.clone().view(torch.int64)
    fix = torch.isfinite(s) & torch.isfinite(err) & (err != 0) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)
    bits += (fix & away).to(torch.int64) - (fix & ~away).to(torch.int64)
    return bits.view(torch.float64).float()


def normalize(x, mean, std):
    """(x - mean[c]) / std[c] on a (C, H, W) float32 torch tensor, as the reference's GeneralizedRCNNTransform.normalize."""
    m = torch.as_tensor(mean, dtype=torch.float32)
    s = torch.as_tensor(std, dtype=torch.float32)
    return (x - m[:, None, None]) / s[:, None, None]


def padded_side(v, size_divisible):
    return int(math.ceil(float(v) / float(size_divisible)) * float(size_divisible))


def detection_batch(images, sizes, mean, std, size_divisible=32):
    """images: (C, h, w) float32 CPU tensors -> the (N, C, Hp, Wp) float32 batch as a torch tensor."""
    resized = [interpolate(normalize(img, mean, std).numpy(), oh, ow) for img, (oh, ow) in zip(images, sizes)]
    hp = padded_side(max(r.shape[1] for r in resized), size_divisible)
    wp = padded_side(max(r.shape[2] for r in resized), size_divisible)
    out = np.zeros((len(resized), resized[0].shape[0], hp, wp), dtype=F32)
    for i, r in enumerate(resized):
        out[i, :, :r.shape[1], :r.shape[2]] = r
    return torch.from_numpy(out)


def resized_size(h, w, min_size, max_size, fixed_size=None):
    """The reference's eager branch (transform.py:24-75 at inference): the scale in Python floats, then floor(float(in) * scale)."""
    if fixed_size is not None:
        return fixed_size[1], fixed_size[0]
    scale = min(float(min_size) / float(min(h, w)), float(max_size) / float(max(h, w)))
    return int(math.floor(float(h) * scale)), int(math.floor(float(w) * scale))


def scripted_resized_size(h, w, min_size, max_size):
    """The reference's scripted / tracing branch (and tests/_roi_heads_ref.py): the scale in float32 tensors."""
    shape = torch.tensor([h, w])
    lo, hi = torch.min(shape).to(torch.float32), torch.max(shape).to(torch.float32)
    scale = torch.min(min_size / lo, max_size / hi).item()
    return int(math.floor(float(h) * scale)), int(math.floor(float(w) * scale))


def bits(t):
    """float32 values as int32, so that NaN compares equal to itself and -0.0 differs from +0.0."""
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32)
