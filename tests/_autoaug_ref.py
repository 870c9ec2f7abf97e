"""torchvision 0.20's v2 automatic-augmentation colour ops (transforms/v2/functional/_color.py invert_image, posterize_image,
solarize_image, autocontrast_image, equalize_image) and the parameter draws of v2/_auto_augment.py's AutoAugment, RandAugment
and TrivialAugmentWide, restated with the same torch ops on the CPU; plus exact host emulations of the kernels' own
arithmetic (csrc/autoaug.hip) for the host tests."""
import math

import numpy as np
import torch


def _bound(dtype):
    return 255 if dtype == torch.uint8 else 1.0


# ---- the reference's kernels --------------------------------------------------------------------------------------------
def ref_invert(x):
    if x.is_floating_point():
        return 1.0 - x
    return x.bitwise_not()


def ref_posterize(x, bits):
    if x.is_floating_point():
        levels = 1 << bits
        return x.mul(levels).floor_().clamp_(0, levels - 1).mul_(1.0 / levels)
    if bits >= 8:
        return x
    mask = ((1 << bits) - 1) << (8 - bits)
    return x & mask


def ref_solarize(x, threshold):
    return torch.where(x >= threshold, ref_invert(x), x)


def ref_autocontrast(x):
    bound = _bound(x.dtype)
    fp = x.is_floating_point()
    float_image = x if fp else x.to(torch.float32)
    minimum = float_image.amin(dim=(-2, -1), keepdim=True)
    maximum = float_image.amax(dim=(-2, -1), keepdim=True)
    eq_idxs = maximum == minimum
    inv_scale = maximum.sub_(minimum).mul_(1.0 / bound)
    minimum[eq_idxs] = 0.0
    inv_scale[eq_idxs] = 1.0
    diff = float_image.sub(minimum) if fp else float_image.sub_(minimum)
    return diff.div_(inv_scale).clamp_(0, bound).to(x.dtype)


def ref_to_uint8(x):
    """to_dtype_image(x, uint8, scale=True)."""
    if x.dtype == torch.uint8:
        return x
    return x.mul(255 + 1.0 - 1e-3).to(torch.uint8)


def ref_equalize(x):
    """equalize_image; float inputs must lie in [0, 1] (the reference's float -> uint8 cast is undefined outside)."""
    output_dtype = x.dtype
    image = ref_to_uint8(x)
    batch_shape = image.shape[:-2]
    flat_image = image.flatten(start_dim=-2).to(torch.long)
    hist = flat_image.new_zeros(batch_shape + (256,), dtype=torch.int32)
    hist.scatter_add_(dim=-1, index=flat_image, src=hist.new_ones(1).expand_as(flat_image))
    cum_hist = hist.cumsum(dim=-1)
    index = cum_hist.argmax(dim=-1, keepdim=True)
    num_non_max_pixels = flat_image.shape[-1] - hist.gather(dim=-1, index=index)
    step = num_non_max_pixels.div_(255, rounding_mode="floor")
    valid_equalization = step.ne(0)
    step.clamp_(min=1)
    cum_hist = cum_hist[..., :-1]
    cum_hist.add_(step // 2).div_(step, rounding_mode="floor").clamp_(0, 255)
    lut = cum_hist.to(torch.uint8)
    lut = torch.cat([lut.new_zeros(1).expand(batch_shape + (1,)), lut], dim=-1)
    equalized_image = lut.gather(dim=-1, index=flat_image).view_as(image)
    output = torch.where(valid_equalization.unsqueeze(-1), equalized_image, image)
    if output_dtype == torch.uint8:
        return output
    return output.to(torch.float32).mul_(1.0 / 255)


def ref_equalize_saturated(x):
    """The library's choice for float inputs outside [0, 1] and NaN: saturate to [0, 1] first (NaN as 0)."""
    if x.dtype == torch.uint8:
        return ref_equalize(x)
    return ref_equalize(torch.nan_to_num(x, nan=0.0).clamp(0.0, 1.0))


REF_OPS = {
    "invert": lambda x: ref_invert(x),
    "posterize": ref_posterize,
    "solarize": ref_solarize,
    "autocontrast": lambda x: ref_autocontrast(x),
    "equalize": lambda x: ref_equalize_saturated(x),
}


# ---- host emulations of the kernels' arithmetic -------------------------------------------------------------------------
def emu_autocontrast_u8(values, mn, mx):
    """k_autocontrast on uint8 values of a plane whose min / max are mn < mx (float32 throughout, numpy)."""
    f32 = np.float32
    lo = f32(mn)
    inv = f32(f32(mx) - f32(mn)) * f32(1.0 / 255.0)
    r = (np.asarray(values, dtype=f32) - lo) / inv
    r = np.where(r <= 0, f32(0), r)
    r = np.where(r >= 255, f32(255), r)
    return np.trunc(r).astype(np.uint8)


def emu_equalize_lut(hist):
    """k_equalize's LUT from a plane's 256-bin histogram (integers): (lut, valid)."""
    hist = [int(h) for h in hist]
    n = sum(hist)
    top = max(k for k in range(256) if hist[k])
    step = (n - hist[top]) // 255
    if step == 0:
        return list(range(256)), False
    lut, cum = [0] * 256, 0
    for k in range(1, 256):
        cum += hist[k - 1]
        lut[k] = min((cum + step // 2) // step, 255)
    return lut, True


# ---- the policies' parameter draws --------------------------------------------------------------------------------------
def _lin(a, b):
    return lambda num_bins, height, width: torch.linspace(a, b, num_bins)


def _post(levels):
    return lambda num_bins, height, width: (8 - (torch.arange(num_bins) / ((num_bins - 1) / levels))).round().int()


def _nil(num_bins, height, width):
    return None


_AA_SPACE = {
    "ShearX": (_lin(0.0, 0.3), True),
    "ShearY": (_lin(0.0, 0.3), True),
    "TranslateX": (lambda num_bins, height, width: torch.linspace(0.0, 150.0 / 331.0 * width, num_bins), True),
    "TranslateY": (lambda num_bins, height, width: torch.linspace(0.0, 150.0 / 331.0 * height, num_bins), True),
    "Rotate": (_lin(0.0, 30.0), True),
    "Brightness": (_lin(0.0, 0.9), True),
    "Color": (_lin(0.0, 0.9), True),
    "Contrast": (_lin(0.0, 0.9), True),
    "Sharpness": (_lin(0.0, 0.9), True),
    "Posterize": (_post(4), False),
    "Solarize": (_lin(1.0, 0.0), False),
    "AutoContrast": (_nil, False),
    "Equalize": (_nil, False),
    "Invert": (_nil, False),
}
RA_SPACE = {"Identity": (_nil, False)}
RA_SPACE.update({k: v for k, v in _AA_SPACE.items() if k != "Invert"})
TA_SPACE = {
    "Identity": (_nil, False),
    "ShearX": (_lin(0.0, 0.99), True),
    "ShearY": (_lin(0.0, 0.99), True),
    "TranslateX": (_lin(0.0, 32.0), True),
    "TranslateY": (_lin(0.0, 32.0), True),
    "Rotate": (_lin(0.0, 135.0), True),
    "Brightness": (_lin(0.0, 0.99), True),
    "Color": (_lin(0.0, 0.99), True),
    "Contrast": (_lin(0.0, 0.99), True),
    "Sharpness": (_lin(0.0, 0.99), True),
    "Posterize": (_post(6), False),
    "Solarize": (_lin(1.0, 0.0), False),
    "AutoContrast": (_nil, False),
    "Equalize": (_nil, False),
}


def _random_item(dct):
    keys = tuple(dct.keys())
    key = keys[int(torch.randint(len(keys), ()))]
    return key, dct[key]


def ref_autoaugment_draws(policies, height, width):
    """AutoAugment.forward's draws: [(transform_id, magnitude)] of the ops it applies."""
    out = []
    policy = policies[int(torch.randint(len(policies), ()))]
    for transform_id, probability, magnitude_idx in policy:
        if not torch.rand(()) <= probability:
            continue
        magnitudes_fn, signed = _AA_SPACE[transform_id]
        magnitudes = magnitudes_fn(10, height, width)
        if magnitudes is not None:
            magnitude = float(magnitudes[magnitude_idx])
            if signed and torch.rand(()) <= 0.5:
                magnitude *= -1
        else:
            magnitude = 0.0
        out.append((transform_id, magnitude))
    return out


def ref_randaugment_draws(num_ops, magnitude_bin, num_bins, height, width):
    out = []
    for _ in range(num_ops):
        transform_id, (magnitudes_fn, signed) = _random_item(RA_SPACE)
        magnitudes = magnitudes_fn(num_bins, height, width)
        if magnitudes is not None:
            magnitude = float(magnitudes[magnitude_bin])
            if signed and torch.rand(()) <= 0.5:
                magnitude *= -1
        else:
            magnitude = 0.0
        out.append((transform_id, magnitude))
    return out


def ref_trivialaugment_draws(num_bins, height, width):
    transform_id, (magnitudes_fn, signed) = _random_item(TA_SPACE)
    magnitudes = magnitudes_fn(num_bins, height, width)
    if magnitudes is not None:
        magnitude = float(magnitudes[int(torch.randint(num_bins, ()))])
        if signed and torch.rand(()) <= 0.5:
            magnitude *= -1
    else:
        magnitude = 0.0
    return [(transform_id, magnitude)]


def ref_apply(image, transform_id, magnitude):
    """_apply_image_or_video_transform for the ops that need no geometry or blend (the CPU transcription of a draw);
    None for the others."""
    if transform_id == "Identity":
        return image
    if transform_id == "Posterize":
        return ref_posterize(image, int(magnitude))
    if transform_id == "Solarize":
        return ref_solarize(image, _bound(image.dtype) * magnitude)
    if transform_id == "AutoContrast":
        return ref_autocontrast(image)
    if transform_id == "Equalize":
        return ref_equalize(image)
    if transform_id == "Invert":
        return ref_invert(image)
    return None


def shear_degrees(magnitude):
    return math.degrees(math.atan(magnitude))
