"""torchvision 0.20's pad / crop / flip / resized_crop / erase and the parameter draws of RandomCrop, RandomResizedCrop and
RandomErasing, restated with torch CPU ops (transforms/v2/functional/_geometry.py, _augment.py, v2/_geometry.py, v2/_augment.py,
_functional_tensor.py `_pad_symmetric`).  Nothing here imports the package under test."""
import math

import torch
from torch.nn.functional import interpolate, pad as torch_pad


def parse_pad_padding(padding):
    if isinstance(padding, int):
        l = r = t = b = padding
    elif len(padding) == 1:
        l = r = t = b = padding[0]
    elif len(padding) == 2:
        l = r = padding[0]
        t = b = padding[1]
    elif len(padding) == 4:
        l, t, r, b = padding
    else:
        raise ValueError(f"Padding must be an int or a 1, 2, or 4 element tuple, not a {len(padding)} element tuple")
    return [l, r, t, b]


def pad_symmetric(img, padding):
    """_functional_tensor.py `_pad_symmetric`: negative entries crop first."""
    if padding[0] < 0 or padding[1] < 0 or padding[2] < 0 or padding[3] < 0:
        neg_min_padding = [-min(x, 0) for x in padding]
        crop_left, crop_right, crop_top, crop_bottom = neg_min_padding
        img = img[..., crop_top:img.shape[-2] - crop_bottom, crop_left:img.shape[-1] - crop_right]
        padding = [max(x, 0) for x in padding]
    in_sizes = img.size()
    _x_indices = [i for i in range(in_sizes[-1])]
    left_indices = [i for i in range(padding[0] - 1, -1, -1)]
    right_indices = [-(i + 1) for i in range(padding[1])]
    x_indices = torch.tensor(left_indices + _x_indices + right_indices)
    _y_indices = [i for i in range(in_sizes[-2])]
    top_indices = [i for i in range(padding[2] - 1, -1, -1)]
    bottom_indices = [-(i + 1) for i in range(padding[3])]
    y_indices = torch.tensor(top_indices + _y_indices + bottom_indices)
    ndim = img.ndim
    if ndim == 3:
        return img[:, y_indices[:, None], x_indices[None, :]]
    return img[:, :, y_indices[:, None], x_indices[None, :]]


def _pad_with_scalar_fill(image, torch_padding, fill, padding_mode):
    shape = image.shape
    c, h, w = shape[-3:]
    image = image.reshape(-1, c, h, w)
    if padding_mode == "edge":
        padding_mode = "replicate"
    if padding_mode == "constant":
        image = torch_pad(image, torch_padding, mode=padding_mode, value=float(fill))
    elif padding_mode in ("reflect", "replicate"):
        dtype = image.dtype
        if not image.is_floating_point():
            image = image.to(torch.float32)  # the identity for integers of up to 16 bits and bool
        image = torch_pad(image, torch_padding, mode=padding_mode).to(dtype)
    else:
        image = pad_symmetric(image, torch_padding)
    return image.reshape(shape[:-3] + image.shape[-3:])


def pad_image(image, padding, fill=None, padding_mode="constant"):
    torch_padding = parse_pad_padding(padding)
    if fill is None:
        fill = 0
    if isinstance(fill, (int, float)):
        return _pad_with_scalar_fill(image, torch_padding, fill, padding_mode)
    if len(fill) == 1:
        return _pad_with_scalar_fill(image, torch_padding, fill[0], padding_mode)
    if padding_mode != "constant":
        raise ValueError(f"Padding mode '{padding_mode}' is not supported if fill is not scalar")
    output = _pad_with_scalar_fill(image, torch_padding, 0, "constant")
    left, right, top, bottom = torch_padding
    fill = torch.tensor(fill, dtype=image.dtype).reshape(-1, 1, 1)
    if top > 0:
        output[..., :top, :] = fill
    if left > 0:
        output[..., :, :left] = fill
    if bottom > 0:
        output[..., -bottom:, :] = fill
    if right > 0:
        output[..., :, -right:] = fill
    return output


def pad_mask(mask, padding, fill=None, padding_mode="constant"):
    squeeze = mask.ndim < 3
    out = pad_image(mask.unsqueeze(0) if squeeze else mask, padding, 0 if fill is None else fill, padding_mode)
    return out.squeeze(0) if squeeze else out


def crop_image(image, top, left, height, width):
    """crop_image: the part of the box inside the image, zero-padded to (height, width)."""
    h, w = image.shape[-2:]
    out = image.new_zeros(tuple(image.shape[:-2]) + (height, width))
    y0, y1, x0, x1 = max(top, 0), min(top + height, h), max(left, 0), min(left + width, w)
    if y1 > y0 and x1 > x0:
        out[..., y0 - top:y1 - top, x0 - left:x1 - left] = image[..., y0:y1, x0:x1]
    return out


def resize_image(image, size):
    """resize_image for bilinear + antialias with the device-tensor convention: uint8 is cast to float32, interpolated,
    rounded and narrowed."""
    if tuple(image.shape[-2:]) == tuple(size):
        return image
    shape = image.shape
    x = image.reshape((-1,) + tuple(shape[-3:]))
    u8 = x.dtype == torch.uint8
    y = interpolate(x.to(torch.float32) if u8 else x, size=list(size), mode="bilinear", align_corners=False, antialias=True)
    if u8:
        y = y.round_().clamp_(0, 255).to(torch.uint8)
    return y.reshape(tuple(shape[:-2]) + tuple(size))


def resized_crop_image(image, top, left, height, width, size):
    return resize_image(crop_image(image, top, left, height, width), size)


def erase_image(image, i, j, h, w, v):
    image = image.clone()
    image[..., i:i + h, j:j + w] = v
    return image


def to_float_normalize(image, mean, std):
    """normalize_image(to_dtype_image(image, float32, scale=True)): v2 scales uint8 by `.to(float32).mul_(1.0 / 255)`."""
    x = image.to(torch.float32).mul_(1.0 / 255) if image.dtype == torch.uint8 else image
    m = torch.as_tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(-1, 1, 1)
    return x.sub(m).div_(s)


# ---- the parameter draws (host RNG calls in the reference's order) ------------------------------------------------------------
def random_crop_params(h, w, size, padding=None, pad_if_needed=False):
    ph, pw = h, w
    if padding is not None:
        pl, pr, pt, pb = parse_pad_padding(padding)
        ph += pt + pb
        pw += pl + pr
    else:
        pl = pr = pt = pb = 0
    ch, cw = size
    if pad_if_needed:
        if ph < ch:
            diff = ch - ph
            pt += diff
            pb += diff
            ph += 2 * diff
        if pw < cw:
            diff = cw - pw
            pl += diff
            pr += diff
            pw += 2 * diff
    if ph < ch or pw < cw:
        raise ValueError(f"Required crop size {(ch, cw)} is larger than {'padded ' if padding is not None else ''}input image "
                         f"size {(ph, pw)}.")
    pad = [pl, pt, pr, pb]
    vert, top = (True, int(torch.randint(0, ph - ch + 1, size=()))) if ph > ch else (False, 0)
    horz, left = (True, int(torch.randint(0, pw - cw + 1, size=()))) if pw > cw else (False, 0)
    return dict(needs_crop=vert or horz, top=top, left=left, height=ch, width=cw, needs_pad=any(pad), padding=pad)


def random_resized_crop_params(height, width, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """-> (params, True when one of the 10 tries fitted)."""
    area = height * width
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = torch.randint(0, height - h + 1, size=(1,)).item()
            j = torch.randint(0, width - w + 1, size=(1,)).item()
            return dict(top=i, left=j, height=h, width=w), True
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return dict(top=(height - h) // 2, left=(width - w) // 2, height=h, width=w), False


def random_erasing_params(img_c, img_h, img_w, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=(0.0,)):
    """`value`: a list of floats or None ("random") -> (params, True when one of the 10 tries fitted)."""
    area = img_h * img_w
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        erase_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        h = int(round(math.sqrt(erase_area * aspect_ratio)))
        w = int(round(math.sqrt(erase_area / aspect_ratio)))
        if not (h < img_h and w < img_w):
            continue
        if value is None:
            v = torch.empty([img_c, h, w], dtype=torch.float32).normal_()
        else:
            v = torch.tensor(list(value))[:, None, None]
        i = torch.randint(0, img_h - h + 1, size=(1,)).item()
        j = torch.randint(0, img_w - w + 1, size=(1,)).item()
        return dict(i=i, j=j, h=h, w=w, v=v), True
    return dict(i=0, j=0, h=img_h, w=img_w, v=None), False
