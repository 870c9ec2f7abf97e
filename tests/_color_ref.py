"""The reference's colour ops restated with torch ops on the host CPU, and an exact host emulation of the library's formulas.

Reference: torchvision 0.20, transforms/v2/functional/_color.py (`_blend`, `_rgb_to_grayscale_image`, `adjust_*_image`,
`_rgb_to_hsv`, `_hsv_to_rgb`) and transforms/v2/functional/_misc.py `to_dtype_image` (uint8 <-> float32 with scale=True),
plus ColorJitter._transform's loop.  Only float32 and uint8 images are exercised.

Emulation: csrc/color.hip's arithmetic in numpy float32, one rounding per operation; the explicit fma of the kernel is
computed in float64 and rounded once to float32 (a product of two float32 values is exact in float64)."""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------------ the reference
def _max_value(dtype):
    return 255 if dtype == torch.uint8 else 1.0


def ref_blend(image1, image2, ratio):
    ratio = float(ratio)
    fp = image1.is_floating_point()
    bound = _max_value(image1.dtype)
    output = image1.mul(ratio).add_(image2, alpha=(1.0 - ratio)).clamp_(0, bound)
    return output if fp else output.to(image1.dtype)


def ref_rgb_to_grayscale(image, num_output_channels=1, preserve_dtype=True):
    if image.shape[-3] == 1 and num_output_channels == 1:
        return image.clone()
    if image.shape[-3] == 1 and num_output_channels == 3:
        s = [1] * len(image.shape)
        s[-3] = 3
        return image.repeat(s)
    r, g, b = image.unbind(dim=-3)
    l_img = r.mul(0.2989).add_(g, alpha=0.587).add_(b, alpha=0.114)
    l_img = l_img.unsqueeze(dim=-3)
    if preserve_dtype:
        l_img = l_img.to(image.dtype)
    if num_output_channels == 3:
        l_img = l_img.expand(image.shape)
    return l_img


def ref_brightness(image, f):
    fp = image.is_floating_point()
    output = image.mul(f).clamp_(0, _max_value(image.dtype))
    return output if fp else output.to(image.dtype)


def ref_saturation(image, f):
    if image.shape[-3] == 1:
        return image
    grayscale_image = ref_rgb_to_grayscale(image, num_output_channels=1, preserve_dtype=False)
    if not image.is_floating_point():
        grayscale_image = grayscale_image.floor_()
    return ref_blend(image, grayscale_image, f)


def ref_contrast_mean(image):
    fp = image.is_floating_point()
    if image.shape[-3] == 3:
        grayscale_image = ref_rgb_to_grayscale(image, num_output_channels=1, preserve_dtype=False)
        if not fp:
            grayscale_image = grayscale_image.floor_()
    else:
        grayscale_image = image if fp else image.to(torch.float32)
    return torch.mean(grayscale_image, dim=(-3, -2, -1), keepdim=True)


def ref_contrast(image, f, mean=None):
    """adjust_contrast_image; `mean` replaces the reference's torch.mean (float32: the library's correctly rounded mean)."""
    return ref_blend(image, ref_contrast_mean(image) if mean is None else mean, f)


def _rgb_to_hsv(image):
    r, g, _ = image.unbind(dim=-3)
    minc, maxc = torch.aminmax(image, dim=-3)
    eqc = maxc == minc
    channels_range = maxc - minc
    ones = torch.ones_like(maxc)
    s = channels_range / torch.where(eqc, ones, maxc)
    channels_range_divisor = torch.where(eqc, ones, channels_range).unsqueeze_(dim=-3)
    rc, gc, bc = ((maxc.unsqueeze(dim=-3) - image) / channels_range_divisor).unbind(dim=-3)
    mask_maxc_neq_r = maxc != r
    mask_maxc_eq_g = maxc == g
    hg = rc.add(2.0).sub_(bc).mul_(mask_maxc_eq_g & mask_maxc_neq_r)
    hr = bc.sub_(gc).mul_(~mask_maxc_neq_r)
    hb = gc.add_(4.0).sub_(rc).mul_(mask_maxc_neq_r.logical_and_(mask_maxc_eq_g.logical_not_()))
    h = hr.add_(hg).add_(hb)
    h = h.mul_(1.0 / 6.0).add_(1.0).fmod_(1.0)
    return torch.stack((h, s, maxc), dim=-3)


def _hsv_to_rgb(img):
    h, s, v = img.unbind(dim=-3)
    h6 = h.mul(6)
    i = torch.floor(h6)
    f = h6.sub_(i)
    i = i.to(dtype=torch.int32)
    sxf = s * f
    one_minus_s = 1.0 - s
    q = (1.0 - sxf).mul_(v).clamp_(0.0, 1.0)
    t = sxf.add_(one_minus_s).mul_(v).clamp_(0.0, 1.0)
    p = one_minus_s.mul_(v).clamp_(0.0, 1.0)
    i.remainder_(6)
    vpqt = torch.stack((v, p, q, t), dim=-3)
    select = torch.tensor([[0, 2, 1, 1, 3, 0], [3, 0, 0, 2, 1, 1], [1, 1, 3, 0, 0, 2]], dtype=torch.long)
    select = select.to(device=img.device, non_blocking=True)
    select = select[:, i]
    if select.ndim > 3:
        select = select.moveaxis(0, -3)
    return vpqt.gather(-3, select)


def ref_hue(image, f):
    if image.shape[-3] == 1 or image.numel() == 0:
        return image
    orig_dtype = image.dtype
    if orig_dtype == torch.uint8:
        image = image.to(torch.float32).mul_(1.0 / 255)
    image = _rgb_to_hsv(image)
    h, s, v = image.unbind(dim=-3)
    h.add_(f).remainder_(1.0)
    image = torch.stack((h, s, v), dim=-3)
    image_hue_adj = _hsv_to_rgb(image)
    if orig_dtype == torch.uint8:
        return image_hue_adj.mul(255.0 + 1.0 - 1e-3).to(torch.uint8)
    return image_hue_adj


REF_OPS = {"brightness": ref_brightness, "contrast": ref_contrast, "saturation": ref_saturation, "hue": ref_hue}


def ref_chain(image, ops):
    """ColorJitter._transform's loop of single calls."""
    for name, f in ops:
        image = REF_OPS[name](image, f)
    return image


# ------------------------------------------------------------------------------------------------------ the emulation
F32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F32)


def emu_grey(r, g, b, form=1):
    if form:
        return _fma(b, F32(0.114), _fma(g, F32(0.587), r * F32(0.2989)))
    return (r * F32(0.2989) + g * F32(0.587)) + b * F32(0.114)


def _clamp(v, hi):
    v = np.where(v <= 0, F32(0), v)
    return np.where(v >= hi, F32(hi), v).astype(F32)


def emu_blend(x, y, f, u8, form=1):
    t = x * F32(f)
    a = F32(1.0 - float(f))
    v = _fma(y, a, t) if form else t + y * a
    v = _clamp(v, 255 if u8 else 1)
    return np.trunc(v).astype(F32) if u8 else v


def emu_hue(x, f, u8):
    r, g, b = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    if u8:
        r, g, b = r * F32(1 / 255), g * F32(1 / 255), b * F32(1 / 255)
    maxc = np.maximum(np.maximum(r, g), b)
    minc = np.minimum(np.minimum(r, g), b)
    eqc = maxc == minc
    rng = maxc - minc
    s = rng / np.where(eqc, F32(1), maxc)
    div = np.where(eqc, F32(1), rng)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    neq_r, eq_g = maxc != r, maxc == g
    hg = ((rc + F32(2)) - bc) * (eq_g & neq_r).astype(F32)
    hr = (bc - gc) * (~neq_r).astype(F32)
    hb = ((gc + F32(4)) - rc) * (neq_r & ~eq_g).astype(F32)
    h = (hr + hg) + hb
    h = np.fmod(h * F32(1.0 / 6.0) + F32(1), F32(1))
    h = np.fmod(h + F32(f), F32(1))
    h = np.where((h != 0) & (h < 0), h + F32(1), h)
    v = maxc
    h6 = h * F32(6)
    fi = np.floor(h6)
    fr = h6 - fi
    i = fi.astype(np.int32) % 6
    sxf, oms = s * fr, F32(1) - s
    q = _clamp((F32(1) - sxf) * v, 1)
    t = _clamp((sxf + oms) * v, 1)
    p = _clamp(oms * v, 1)
    ro = np.select([i == 0, i == 1, i == 2, i == 3, i == 4], [v, q, p, p, t], v)
    go = np.select([i == 0, i == 1, i == 2, i == 3, i == 4], [t, v, v, q, p], p)
    bo = np.select([i == 0, i == 1, i == 2, i == 3, i == 4], [p, p, t, v, v], q)
    out = np.stack([ro, go, bo], axis=-3).astype(F32)
    if u8:
        out = (out * F32(255.999)).astype(np.int32).astype(np.uint8).astype(F32)
    return out


def emu_mean(x, u8, form=1):
    """The library's per-image mean of the grey image of x (..., C, H, W): uint8 (float)S / (float)N of the exact integer
    sum; float32 the correctly rounded mean."""
    if x.shape[-3] == 3:
        grey = emu_grey(x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :], form)
        if u8:
            grey = np.floor(grey)
    else:
        grey = x[..., 0, :, :]
    n = grey.shape[-1] * grey.shape[-2]
    flat = grey.reshape(-1, n)
    if u8:
        s = flat.astype(np.int64).sum(axis=1)
        means = s.astype(F32) / F32(n)
    else:
        import math
        means = np.array([math.fsum(row.astype(np.float64).tolist()) / n for row in flat]).astype(F32)
    return means.reshape(grey.shape[:-2] + (1, 1, 1))


def emu_chain(image, ops, form=1):
    """The library's chain on a CPU float32 / uint8 torch tensor (..., C, H, W): a torch tensor of the input's dtype."""
    u8 = image.dtype == torch.uint8
    x = image.numpy().astype(F32)
    c = x.shape[-3]
    for name, f in ops:
        if name == "brightness":
            v = _clamp(x * F32(f), 255 if u8 else 1)
            x = np.trunc(v).astype(F32) if u8 else v
        elif name == "contrast":
            x = emu_blend(x, emu_mean(x, u8, form), f, u8, form)
        elif name == "saturation" and c == 3:
            grey = emu_grey(x[..., 0:1, :, :], x[..., 1:2, :, :], x[..., 2:3, :, :], form)
            if u8:
                grey = np.floor(grey)
            x = emu_blend(x, grey, f, u8, form)
        elif name == "hue" and c == 3:
            x = emu_hue(x, f, u8)
    return torch.from_numpy(x.astype(np.uint8) if u8 else x)


def emu_grayscale(image, num_output_channels, form=1):
    u8 = image.dtype == torch.uint8
    x = image.numpy().astype(F32)
    grey = emu_grey(x[..., 0:1, :, :], x[..., 1:2, :, :], x[..., 2:3, :, :], form)
    grey = np.repeat(grey, num_output_channels, axis=-3)
    return torch.from_numpy(np.trunc(grey).astype(np.uint8) if u8 else grey)


def check_contrast_reference(image, f, got, form=1):
    """The contrast rule: the reference's blend against the library's mean equals, per element, either the fused form (the
    library's) or the plain form, and no more than 64 elements per CPU thread take the plain one."""
    u8 = image.dtype == torch.uint8
    x = image.numpy().astype(F32)
    mean = emu_mean(x, u8, form)
    ref = ref_contrast(image, f, mean=torch.from_numpy(mean)).numpy()
    fused = emu_blend(x, mean, f, u8, 1)
    plain = emu_blend(x, mean, f, u8, 0)
    if u8:
        fused, plain = fused.astype(np.uint8), plain.astype(np.uint8)
    assert np.all((ref == fused) | (ref == plain)), "the reference's contrast blend is neither the fused nor the plain form"
    n_plain = int(np.count_nonzero(ref != fused))
    assert n_plain <= 64 * torch.get_num_threads(), n_plain
    assert torch.equal(got, torch.from_numpy(fused)), "library output != the fused contrast form"
    return n_plain
