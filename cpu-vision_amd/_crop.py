"""pad / crop / flip / resized_crop / erase of the v2 surface -- the reference's transforms/v2/functional/_geometry.py
(horizontal_flip, vertical_flip, pad, crop, resized_crop) and _augment.py (erase) with their _image / _mask / _video kernels:
argument checks and host math here, with the reference's error text; the data movement is one launch of the gather kernel of
csrc/crop.hip (mv_pad_crop_flip / mv_erase), and resized_crop is the resize kernels reading through a source window
(mv_resized_crop_*).

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib, _pil, tv_tensors
from ._registry import _get_kernel, _register_kernel_internal, _unsupported

PAD_MODES = {"constant": 0, "edge": 1, "reflect": 2, "symmetric": 3}
_IMAGE_TYPES = (tv_tensors.Image, torch.Tensor, tv_tensors.Video)
_MAX_FILL_CHANNELS = 4


# --------------------------------------------------------------------------------------------- the kernel's index map
def axis_index_map(n: int, before: int, after: int, mode: str, flip: bool = False) -> List[int]:
    """The gather kernel's map of ONE axis, written once on the host: for each of the n + before + after output positions the
    source index it takes, or -1 for the fill.  `before` / `after` are the paddings of the two ends (negative: cropping).
    It is csrc/crop.hip `gather_index` term for term; the launchers call it through `_check_axis` to validate, and the tests
    hold it against torch.nn.functional.pad and _pad_symmetric."""
    _check_axis(n, before, after, mode)
    out = n + before + after
    code = PAD_MODES[mode]
    res = []
    for o in range(max(out, 0)):
        p = (out - 1 - o if flip else o) - before
        if not 0 <= p < n:
            if code == 0:
                p = -1
            else:
                if code == 2:
                    p = -p if p < 0 else 2 * (n - 1) - p
                elif code == 3:
                    p = -1 - p if p < 0 else 2 * n - 1 - p
                p = min(max(p, 0), n - 1)
        res.append(p)
    return res


def _check_axis(n: int, before: int, after: int, mode: str) -> None:
    """What one reflection can reach: reflect padding must be smaller than the side (ATen's rule), symmetric padding at most
    the side."""
    if mode not in PAD_MODES:
        raise ValueError(f"`padding_mode` should be either `'constant'`, `'edge'`, `'reflect'` or `'symmetric'`, "
                         f"but got `'{mode}'`.")
    if mode == "constant" or n + before + after <= 0:
        return
    if n <= 0:
        raise ValueError(f"Padding mode '{mode}' needs a non-empty image")
    if mode == "reflect" and not (before < n and after < n):
        raise ValueError(f"Padding size should be less than the corresponding input dimension, but got: padding ({before}, "
                         f"{after}) at a dimension of size {n}")
    if mode == "symmetric" and not (before <= n and after <= n):
        raise ValueError(f"Symmetric padding ({before}, {after}) exceeds a dimension of size {n}")


def _parse_pad_padding(padding) -> List[int]:
    """_parse_pad_padding (_geometry.py): `padding` in the order (left, top, right, bottom) -> [left, right, top, bottom]."""
    if isinstance(padding, int):
        pad_left = pad_right = pad_top = pad_bottom = padding
    elif isinstance(padding, (tuple, list)):
        if len(padding) == 1:
            pad_left = pad_right = pad_top = pad_bottom = padding[0]
        elif len(padding) == 2:
            pad_left = pad_right = padding[0]
            pad_top = pad_bottom = padding[1]
        elif len(padding) == 4:
            pad_left, pad_top, pad_right, pad_bottom = padding
        else:
            raise ValueError(f"Padding must be an int or a 1, 2, or 4 element tuple, not a {len(padding)} element tuple")
    else:
        raise TypeError(f"`padding` should be an integer or tuple or list of integers, but got {padding}")
    return [int(pad_left), int(pad_right), int(pad_top), int(pad_bottom)]


def _fill_elements(dtype: torch.dtype, fill, channels: int) -> torch.Tensor:
    """The constant fill as host elements of the image's dtype, made by the reference's own conversions: a scalar goes through
    torch's constant pad of a one-element tensor (`value=float(fill)`), a vector through torch.tensor(fill, dtype=...)."""
    if isinstance(fill, (int, float)):
        return torch.nn.functional.pad(torch.zeros(1, dtype=dtype), [0, 1], mode="constant", value=float(fill))[1:]
    if len(fill) != channels:
        raise ValueError(f"The number of elements in 'fill' cannot broadcast to match the number of channels of the image: "
                         f"{len(fill)} != {channels}")
    if channels > _MAX_FILL_CHANNELS:
        raise NotImplementedError(f"pad: a per-channel fill on {channels} channels is not on the MI355X path (up to "
                                  f"{_MAX_FILL_CHANNELS} channels are; a scalar fill works for any channel count)")
    return torch.tensor(fill, dtype=dtype)


def _host_bytes(t: torch.Tensor):
    raw = t.contiguous().view(torch.uint8).numpy().tobytes()
    return C.create_string_buffer(raw, len(raw))


def _gather(image: torch.Tensor, oh: int, ow: int, top: int, left: int, mode: str = "constant", flip_h: bool = False,
            flip_v: bool = False, fill=0, what: str = "pad") -> torch.Tensor:
    """ONE launch of the gather kernel (mv_pad_crop_flip) over every (H, W) plane of `image`: output pixel (y, x) takes source
    pixel (map(y), map(x)) with the per-axis map of `axis_index_map` at offsets (top, left) in source coordinates."""
    h, w = int(image.shape[-2]), int(image.shape[-1])
    lead = tuple(image.shape[:-2])
    _check_axis(h, -top, oh - h + top, mode)
    _check_axis(w, -left, ow - w + left, mode)
    channels = int(image.shape[-3]) if image.ndim >= 3 else 1
    elems = _fill_elements(image.dtype, fill if fill is not None else 0, channels) if mode == "constant" else None
    planes = 1
    for d in lead:
        planes *= int(d)
    if planes == 0 or oh <= 0 or ow <= 0:
        return image.new_empty(lead + (max(oh, 0), max(ow, 0)))
    _lib.require_device(image)
    if image.element_size() not in (1, 2, 4, 8) or image.is_complex():
        raise NotImplementedError(f"{what}: {image.dtype} images are not on the MI355X path")
    lib = _lib.load()
    with _lib.on_device_of(image):
        x = image.contiguous()
        y = x.new_empty(lead + (oh, ow))
        n_fill = int(elems.numel()) if elems is not None else 1
        buf = _host_bytes(elems) if elems is not None else None
        _lib.check(lib.mv_pad_crop_flip(x.data_ptr(), y.data_ptr(), planes, n_fill, x.element_size(), h, w, oh, ow, top, left,
                                        PAD_MODES[mode], int(flip_h), int(flip_v), buf, _lib.stream_ptr(x)))
    return _lib.forward_only(y, what, image) if image.is_floating_point() else y


def _register_image_mask_video(functional):
    def decorator(kernel):
        for input_type in _IMAGE_TYPES + (tv_tensors.Mask,):
            _register_kernel_internal(functional, input_type)(kernel)
        return kernel

    return decorator


def _no_boxes_no_pil(functional, pil_reason: str) -> None:
    _unsupported(functional, tv_tensors.BoundingBoxes, "BoundingBoxes are not transformed on the MI355X path (the local "
                                                       "BoundingBoxes carries no format or canvas size)")
    if _pil.PIL is not None:
        _unsupported(functional, _pil.PIL.Image.Image, pil_reason)


_PIL_REASON = "PIL images are handled by Pillow's own C code in the reference; convert with pil_to_tensor and move the tensor " \
              "to the MI355X"


# --------------------------------------------------------------------------------------------- flips
def horizontal_flip(inpt: torch.Tensor) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py `horizontal_flip`."""
    kernel = _get_kernel(horizontal_flip, type(inpt))
    return kernel(inpt)


@_register_image_mask_video(horizontal_flip)
def horizontal_flip_image(image: torch.Tensor) -> torch.Tensor:
    """horizontal_flip_image (_geometry.py): image.flip(-1), a fresh tensor, in one gather launch."""
    if image.ndim < 1:
        raise IndexError("Dimension out of range (expected to be in range of [-1, 0], but got -1)")
    if image.ndim == 1:
        return _gather(image.unsqueeze(0), 1, int(image.shape[-1]), 0, 0, flip_h=True, what="horizontal_flip").squeeze(0)
    return _gather(image, int(image.shape[-2]), int(image.shape[-1]), 0, 0, flip_h=True, what="horizontal_flip")


horizontal_flip_mask = horizontal_flip_video = horizontal_flip_image
hflip = horizontal_flip


def vertical_flip(inpt: torch.Tensor) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py `vertical_flip`."""
    kernel = _get_kernel(vertical_flip, type(inpt))
    return kernel(inpt)


@_register_image_mask_video(vertical_flip)
def vertical_flip_image(image: torch.Tensor) -> torch.Tensor:
    """vertical_flip_image (_geometry.py): image.flip(-2), a fresh tensor, in one gather launch."""
    if image.ndim < 2:
        raise IndexError(f"Dimension out of range (expected to be in range of [-{max(image.ndim, 1)}, {max(image.ndim, 1) - 1}], "
                         "but got -2)")
    return _gather(image, int(image.shape[-2]), int(image.shape[-1]), 0, 0, flip_v=True, what="vertical_flip")


vertical_flip_mask = vertical_flip_video = vertical_flip_image
vflip = vertical_flip


# --------------------------------------------------------------------------------------------- pad
def pad(inpt: torch.Tensor, padding: List[int], fill=None, padding_mode: str = "constant") -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py `pad`."""
    kernel = _get_kernel(pad, type(inpt))
    return kernel(inpt, padding=padding, fill=fill, padding_mode=padding_mode)


def _scalar_or_vector_fill(fill, padding_mode: str):
    """pad_image's three branches: None -> 0, a number or a 1-element sequence -> scalar, C values -> constant mode only."""
    if fill is None:
        return 0
    if isinstance(fill, (int, float)):
        return fill
    if len(fill) == 1:
        return fill[0]
    if padding_mode != "constant":
        raise ValueError(f"Padding mode '{padding_mode}' is not supported if fill is not scalar")
    return list(fill)


def _pad_offsets(image: torch.Tensor, torch_padding: List[int], padding_mode: str, name: str):
    """(oh, ow) of the padded image after the reference's own checks of what its padding routines accept."""
    left, right, top, bottom = torch_padding
    h, w = int(image.shape[-2]), int(image.shape[-1])
    if padding_mode in ("edge", "reflect") and image.dtype in (torch.int32, torch.int64):
        # the reference pads integer images as float32 and casts back: the identity up to 16 bits only
        raise NotImplementedError(f"{name}: {padding_mode} padding of {image.dtype} images goes through float32 in the reference "
                                  "and is not on the MI355X path (constant and symmetric are)")
    if padding_mode == "symmetric":  # _pad_symmetric crops first and mirrors what is left
        for n, before, after in ((w, left, right), (h, top, bottom)):
            kept = n + min(before, 0) + min(after, 0)
            if max(before, 0) > kept or max(after, 0) > kept:
                raise ValueError(f"Symmetric padding ({before}, {after}) exceeds the cropped dimension of size {kept}")
    return h + top + bottom, w + left + right


def pad_image(image: torch.Tensor, padding: List[int], fill=None, padding_mode: str = "constant") -> torch.Tensor:
    """pad_image (_geometry.py) on (..., C, H, W) tensors of any 1 / 2 / 4 / 8-byte dtype: _pad_with_scalar_fill /
    _pad_with_vector_fill / _pad_symmetric as ONE launch of the gather kernel."""
    torch_padding = _parse_pad_padding(padding)
    if padding_mode not in PAD_MODES:
        raise ValueError(f"`padding_mode` should be either `'constant'`, `'edge'`, `'reflect'` or `'symmetric'`, "
                         f"but got `'{padding_mode}'`.")
    fill = _scalar_or_vector_fill(fill, padding_mode)
    if image.ndim < 3:
        raise ValueError(f"Expected tensor to be a tensor image of size (..., C, H, W). Got {tuple(image.shape)}.")
    oh, ow = _pad_offsets(image, torch_padding, padding_mode, "pad")
    if oh < 0 or ow < 0:
        raise RuntimeError(f"The input size {tuple(image.shape[-2:])}, plus negative padding {torch_padding} resulted in a "
                           "negative output size, which is invalid.")
    return _gather(image, oh, ow, -torch_padding[2], -torch_padding[0], padding_mode, fill=fill, what="pad")


for _t in _IMAGE_TYPES:
    _register_kernel_internal(pad, _t)(pad_image)
pad_video = pad_image


@_register_kernel_internal(pad, tv_tensors.Mask)
def pad_mask(mask: torch.Tensor, padding: List[int], fill=None, padding_mode: str = "constant") -> torch.Tensor:
    """pad_mask (_geometry.py): fill None -> 0, a scalar fill only; 2-D masks gain a channel for the call."""
    if fill is None:
        fill = 0
    if isinstance(fill, (tuple, list)):
        raise ValueError("Non-scalar fill value is not supported")
    needs_squeeze = mask.ndim < 3
    if needs_squeeze:
        mask = mask.unsqueeze(0)
    output = pad_image(mask, padding=padding, fill=fill, padding_mode=padding_mode)
    return output.squeeze(0) if needs_squeeze else output


# --------------------------------------------------------------------------------------------- crop
def crop(inpt: torch.Tensor, top: int, left: int, height: int, width: int) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py `crop`."""
    kernel = _get_kernel(crop, type(inpt))
    return kernel(inpt, top=top, left=left, height=height, width=width)


@_register_image_mask_video(crop)
def crop_image(image: torch.Tensor, top: int, left: int, height: int, width: int) -> torch.Tensor:
    """crop_image (_geometry.py): a view when the box lies inside the image; a box that reaches outside is the part inside,
    zero-padded -- one gather launch at offset (top, left) with a zero fill."""
    h, w = int(image.shape[-2]), int(image.shape[-1])
    top, left, height, width = int(top), int(left), int(height), int(width)
    right, bottom = left + width, top + height
    if (left < 0 or top < 0 or right > w or bottom > h) and height > 0 and width > 0:
        return _gather(image, height, width, top, left, "constant", fill=0, what="crop")
    return image[..., top:bottom, left:right]


crop_mask = crop_video = crop_image


def pad_crop(inpt: torch.Tensor, padding: List[int], top: int, left: int, height: int, width: int, fill=None,
             padding_mode: str = "constant") -> torch.Tensor:
    """crop(pad(inpt, padding, fill, padding_mode), top, left, height, width) for a box inside the padded image -- RandomCrop
    with padding -- as ONE launch: the two steps compose into one offset per axis."""
    kernel = _get_kernel(pad_crop, type(inpt))
    return kernel(inpt, padding=padding, top=top, left=left, height=height, width=width, fill=fill, padding_mode=padding_mode)


@_register_image_mask_video(pad_crop)
def pad_crop_image(image: torch.Tensor, padding: List[int], top: int, left: int, height: int, width: int, fill=None,
                   padding_mode: str = "constant") -> torch.Tensor:
    pl, pr, pt, pb = _parse_pad_padding(padding)
    if padding_mode not in PAD_MODES:
        raise ValueError(f"`padding_mode` should be either `'constant'`, `'edge'`, `'reflect'` or `'symmetric'`, "
                         f"but got `'{padding_mode}'`.")
    fill = _scalar_or_vector_fill(fill, padding_mode)
    needs_squeeze = image.ndim < 3
    if needs_squeeze:
        image = image.unsqueeze(0)
    ph, pw = _pad_offsets(image, [pl, pr, pt, pb], padding_mode, "pad_crop")
    h, w = int(image.shape[-2]), int(image.shape[-1])
    _check_axis(h, pt, pb, padding_mode)
    _check_axis(w, pl, pr, padding_mode)
    if top < 0 or left < 0 or top + height > ph or left + width > pw or height <= 0 or width <= 0:
        out = crop_image(pad_image(image, [pl, pt, pr, pb], fill=fill, padding_mode=padding_mode), top, left, height, width)
    else:
        out = _gather(image, int(height), int(width), int(top) - pt, int(left) - pl, padding_mode, fill=fill, what="pad_crop")
    return out.squeeze(0) if needs_squeeze else out


# --------------------------------------------------------------------------------------------- resized_crop
def resized_crop(inpt: torch.Tensor, top: int, left: int, height: int, width: int, size: List[int],
                 interpolation="bilinear", antialias: Optional[bool] = True) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_geometry.py `resized_crop`."""
    kernel = _get_kernel(resized_crop, type(inpt))
    return kernel(inpt, top=top, left=left, height=height, width=width, size=size, interpolation=interpolation,
                  antialias=antialias)


def _resized_crop_launch(image: torch.Tensor, top: int, left: int, height: int, width: int, oh: int, ow: int, flip_h: bool,
                         flip_v: bool, preset=None) -> torch.Tensor:
    """mv_resized_crop_* / mv_resized_crop_preset_*: the resize kernels read the (height, width) window at (top, left) of the
    image in place -- zeros where it reaches outside -- and mirror the output in their final store."""
    _lib.require_device(image)
    if image.dtype not in (torch.uint8, torch.float32):
        raise NotImplementedError(f"resize runs on uint8 and float32 images. Got {image.dtype}")
    lib = _lib.load()
    h, w = int(image.shape[-2]), int(image.shape[-1])
    lead = tuple(image.shape[:-2])
    planes = 1
    for d in lead:
        planes *= int(d)
    u8 = image.dtype == torch.uint8
    with _lib.on_device_of(image):
        x = image.contiguous()
        y = torch.empty(lead + (oh, ow), dtype=torch.float32 if preset is not None else image.dtype, device=image.device)
        if planes == 0:
            return y
        nbytes = int(lib.mv_resize_workspace_bytes(planes, height, width, oh, ow, 0, 0, oh, ow))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=image.device) if nbytes else None
        tail = (None if ws is None else ws.data_ptr(), nbytes, _lib.stream_ptr(x))
        geometry = (h, w, int(top), int(left), int(height), int(width), oh, ow, int(flip_h), int(flip_v))
        if preset is None:
            fn = lib.mv_resized_crop_u8 if u8 else lib.mv_resized_crop_f32
            _lib.check(fn(x.data_ptr(), y.data_ptr(), planes, *geometry, *tail))
        else:
            mean, std = preset
            c = int(image.shape[-3])
            fn = lib.mv_resized_crop_preset_u8 if u8 else lib.mv_resized_crop_preset_f32
            # v2_scale = 1: to_dtype(scale=True) multiplies by 1 / 255, where the v1 preset divides by 255
            _lib.check(fn(x.data_ptr(), y.data_ptr(), planes // c, c, *geometry, 1, mean, std, *tail))
    return y if u8 and preset is None else _lib.forward_only(y, "resized_crop", image)


def _resized_crop_size(image: torch.Tensor, height: int, width: int, size, interpolation, antialias) -> Tuple[int, int]:
    from . import functional_v1
    interpolation = getattr(interpolation, "value", interpolation)
    size = functional_v1._check_resize_args(image, size, interpolation, None, antialias)
    if height <= 0 or width <= 0:
        raise ValueError(f"resized_crop: the crop box must be non-empty, got height={height}, width={width}")
    oh, ow = functional_v1._compute_resized_output_size((int(height), int(width)), size, None)
    return int(oh), int(ow)


@_register_kernel_internal(resized_crop, tv_tensors.Image)
@_register_kernel_internal(resized_crop, torch.Tensor)
@_register_kernel_internal(resized_crop, tv_tensors.Video)
def resized_crop_image(image: torch.Tensor, top: int, left: int, height: int, width: int, size: List[int],
                       interpolation="bilinear", antialias: Optional[bool] = True) -> torch.Tensor:
    """resized_crop_image (_geometry.py) = resize_image(crop_image(image, top, left, height, width), size) for bilinear with
    antialias, without a copy of the crop: one launch (scale factors up to 7) or two.  uint8 follows `resize_image`: float32,
    interpolate, round_(), narrow."""
    oh, ow = _resized_crop_size(image, height, width, size, interpolation, antialias)
    if (oh, ow) == (int(height), int(width)):  # resize_image hands an image of the requested size back as it is
        return crop_image(image, top, left, height, width)
    return _resized_crop_launch(image, top, left, height, width, oh, ow, False, False)


resized_crop_video = resized_crop_image


@_register_kernel_internal(resized_crop, tv_tensors.Mask, tv_tensor_wrapper=False)
def _resized_crop_mask_dispatch(inpt, *args, **kwargs):
    raise NotImplementedError("resized_crop: masks are resized with nearest interpolation in the reference, which is not on the "
                              "MI355X path (antialiased bilinear is)")


def resized_crop_flip_normalize(image: torch.Tensor, top: int, left: int, height: int, width: int, size: List[int], flip: bool,
                                mean: Sequence[float], std: Sequence[float]) -> torch.Tensor:
    """normalize(to_dtype(hflip-if-`flip`(resized_crop(image, ...)), float32, scale=True), mean, std) -- the head of the
    classification training recipe -- in the ONE launch of the resize: window on the loads, flip and the preset tail on the
    store.  uint8 or float32 (..., C <= 4, H, W) images; float32 images are not rescaled, as to_dtype does not."""
    from .functional import _mean_std
    if image.ndim < 3:
        raise ValueError(f"Expected tensor to be a tensor image of size (..., C, H, W). Got {tuple(image.shape)}.")
    if isinstance(std, (tuple, list)) and not all(std):
        raise ValueError("std evaluated to zero, leading to division by zero.")
    oh, ow = _resized_crop_size(image, height, width, size, "bilinear", True)
    c = int(image.shape[-3])
    if c > 4:
        raise NotImplementedError(f"resized_crop_flip_normalize: up to 4 channels, got {c}")
    return _resized_crop_launch(image, top, left, height, width, oh, ow, bool(flip), False, preset=_mean_std(mean, std, c))


# --------------------------------------------------------------------------------------------- erase
def erase(inpt: torch.Tensor, i: int, j: int, h: int, w: int, v: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """Dispatcher, as transforms/v2/functional/_augment.py `erase`."""
    kernel = _get_kernel(erase, type(inpt))
    return kernel(inpt, i=i, j=j, h=h, w=w, v=v, inplace=inplace)


@_register_kernel_internal(erase, tv_tensors.Image)
@_register_kernel_internal(erase, torch.Tensor)
@_register_kernel_internal(erase, tv_tensors.Video)
def erase_image(image: torch.Tensor, i: int, j: int, h: int, w: int, v: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """erase_image (_augment.py): image.clone() unless `inplace`, then image[..., i:i+h, j:j+w] = v with v broadcastable
    (C, 1, 1) or (C, h, w), converted to the image's dtype as the assignment converts it.  Out of place it is one gather
    launch that never reads the pixels under the box; in place only the box is written."""
    if not isinstance(v, torch.Tensor):
        raise TypeError(f"Argument v should be a Tensor, got {type(v)}")
    if image.ndim < 3:
        raise ValueError(f"Expected tensor to be a tensor image of size (..., C, H, W). Got {tuple(image.shape)}.")
    c, ih, iw = (int(s) for s in image.shape[-3:])
    i0, i1, _ = slice(int(i), int(i) + int(h)).indices(ih)  # the box the slice assignment really covers
    j0, j1, _ = slice(int(j), int(j) + int(w)).indices(iw)
    bh, bw = max(i1 - i0, 0), max(j1 - j0, 0)
    if v.ndim > 3:
        raise NotImplementedError("erase: v broadcastable over (C, h, w) is on the MI355X path; it has more dimensions")
    vb = v.detach().to(image.dtype)  # on v's own device: the conversion the slice assignment makes
    while vb.ndim < 3:
        vb = vb.unsqueeze(0)
    per_pixel = tuple(vb.shape[-2:]) != (1, 1)
    try:
        vb = vb.expand(c, bh, bw) if per_pixel else vb.expand(c, 1, 1)
    except RuntimeError as e:
        raise RuntimeError(f"erase: v of shape {tuple(v.shape)} does not broadcast to ({c}, {bh}, {bw})") from e
    if image.numel() == 0:
        return image if inplace else image.clone()
    _lib.require_device(image)
    if image.element_size() not in (1, 2, 4, 8) or image.is_complex():
        raise NotImplementedError(f"erase: {image.dtype} images are not on the MI355X path")
    if inplace and not image.is_contiguous():
        raise NotImplementedError("erase: inplace=True needs a contiguous image on the MI355X path")
    lib = _lib.load()
    planes = image.numel() // (ih * iw)
    with _lib.on_device_of(image):
        x = image if inplace else image.contiguous()
        y = x if inplace else torch.empty_like(x, memory_format=torch.contiguous_format)
        vd = vb.to(image.device).contiguous()
        _lib.check(lib.mv_erase(x.data_ptr(), y.data_ptr(), planes, c, x.element_size(), ih, iw, i0, j0, bh, bw, vd.data_ptr(),
                                int(per_pixel), _lib.stream_ptr(x)))
    if inplace or not image.is_floating_point():
        return y
    return _lib.forward_only(y, "erase", image, v)


erase_video = erase_image

for _f in (horizontal_flip, vertical_flip, pad, crop, pad_crop, resized_crop, erase):
    _no_boxes_no_pil(_f, _PIL_REASON)
del _f, _t
