"""Transform classes that call the hot path -- mirrors of the reference's callers:

  Transform.forward / _call_kernel        transforms/v2/_transform.py:17-87
  GaussianBlur (v2)                       transforms/v2/_misc.py:168-205
  RandomAdjustSharpness (v2)              transforms/v2/_color.py:356-376 (+ _RandomApplyTransform, _transform.py:~150-190)
  GaussianBlurV1                          transforms/transforms.py:1753-1812
  ElasticTransform                        transforms/v2/_geometry.py:1003-1085 (noise field -> gaussian_blur -> displacement
                                          -> F.elastic)
  RandomRotation / RandomAffine / RandomPerspective   transforms/v2/_geometry.py (-> F.rotate / F.affine / F.perspective)
  ColorJitter / Grayscale / RandomGrayscale           transforms/v2/_color.py (-> F.adjust_* / F.rgb_to_grayscale)
  RandomInvert / RandomPosterize / RandomSolarize / RandomAutocontrast / RandomEqualize   transforms/v2/_color.py
  AutoAugment / RandAugment / TrivialAugmentWide      transforms/v2/_auto_augment.py (-> F.affine / rotate / adjust_* /
                                                      posterize / solarize / autocontrast / equalize / invert)
  Resize / CenterCrop / ToDtype / Normalize / Compose   v2/_geometry.py:76-193, v2/_misc.py:134-304, v2/_container.py:10-64
  RandomHorizontalFlip / RandomVerticalFlip / Pad / RandomCrop / RandomResizedCrop   transforms/v2/_geometry.py
  RandomErasing                           transforms/v2/_augment.py (-> F.erase)
  MixUp / CutMix                          transforms/v2/_augment.py (-> F.mixup_image / F.cutmix_image / F.mixup_labels)
  RandomApply / RandomChoice / RandomOrder   transforms/v2/_container.py

Parameter sampling stays on the host RNG exactly like the reference (torch.empty(1).uniform_ / torch.rand(1)).
"""
from __future__ import annotations

import collections.abc
import math
import numbers
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import nn
from torch.utils._pytree import tree_flatten, tree_unflatten

from . import _pil
from . import functional as F
from . import functional_v1 as F1
from . import tv_tensors
from ._registry import _get_kernel, is_pure_tensor

_PIL_TYPES = (_pil.PIL.Image.Image,) if _pil.PIL is not None else ()


import enum as _enum


class InterpolationMode(_enum.Enum):
    """transforms/functional.py:21-35."""

    NEAREST = "nearest"
    NEAREST_EXACT = "nearest-exact"
    BILINEAR = "bilinear"
    BICUBIC = "bicubic"
    BOX = "box"
    HAMMING = "hamming"
    LANCZOS = "lanczos"


def _setup_size(size, error_msg):
    """transforms/transforms.py `_setup_size`"""
    if isinstance(size, numbers.Number):
        return int(size), int(size)
    if isinstance(size, Sequence) and len(size) == 1:
        return size[0], size[0]
    if len(size) != 2:
        raise ValueError(error_msg)
    return size


def _setup_number_or_seq(arg, name: str) -> Sequence[float]:
    """transforms/v2/_utils.py:21-38"""
    if not isinstance(arg, (int, float, Sequence)):
        raise TypeError(f"{name} should be a number or a sequence of numbers. Got {type(arg)}")
    if isinstance(arg, Sequence) and len(arg) not in (1, 2):
        raise ValueError(f"If {name} is a sequence its length should be 1 or 2. Got {len(arg)}")
    if isinstance(arg, Sequence):
        for element in arg:
            if not isinstance(element, (int, float)):
                raise ValueError(f"{name} should be a sequence of numbers. Got {type(element)}")
    if isinstance(arg, (int, float)):
        arg = [float(arg), float(arg)]
    elif isinstance(arg, Sequence):
        arg = [float(arg[0]), float(arg[0])] if len(arg) == 1 else [float(arg[0]), float(arg[1])]
    return arg


def query_size(flat_inputs: List[Any]):
    """transforms/v2/_utils.py:175-196: the one (H, W) of the images / videos / masks / boxes of a sample."""
    sizes = set()
    for inpt in flat_inputs:
        if isinstance(inpt, tv_tensors.BoundingBoxes) and hasattr(inpt, "canvas_size"):
            sizes.add(tuple(inpt.canvas_size))
        elif isinstance(inpt, torch.Tensor):
            if inpt.ndim < 2:
                raise TypeError(f"Input tensor should have at least two dimensions, but got {inpt.ndim}")
            sizes.add(tuple(inpt.shape[-2:]))
        elif isinstance(inpt, _PIL_TYPES):
            sizes.add((inpt.size[1], inpt.size[0]))
    if not sizes:
        raise TypeError("No image, video, mask or bounding box was found in the sample")
    if len(sizes) > 1:
        raise ValueError(f"Found multiple HxW dimensions in the sample: {sorted(sizes)}")
    h, w = sizes.pop()
    return int(h), int(w)


def query_chw(flat_inputs: List[Any]) -> Tuple[int, int, int]:
    """transforms/v2/_utils.py `query_chw`: the one (C, H, W) of the images and videos of a sample."""
    chws = set()
    for inpt in flat_inputs:
        if isinstance(inpt, (tv_tensors.Image, tv_tensors.Video)) or is_pure_tensor(inpt):
            chw = list(inpt.shape[-3:])
            if len(chw) == 2:
                chw.insert(0, 1)
            elif len(chw) != 3:
                raise TypeError(f"Input tensor should have at least two dimensions, but got {len(chw)}")
            chws.add(tuple(int(d) for d in chw))
        elif isinstance(inpt, _PIL_TYPES):
            chws.add((len(inpt.getbands()), inpt.size[1], inpt.size[0]))
    if not chws:
        raise TypeError("No image or video was found in the sample")
    if len(chws) > 1:
        raise ValueError(f"Found multiple CxHxW dimensions in the sample: {', '.join(str(c) for c in sorted(chws))}")
    c, h, w = chws.pop()
    return c, h, w


class Transform(nn.Module):
    _transformed_types = (torch.Tensor,) + _PIL_TYPES

    def _check_inputs(self, flat_inputs: List[Any]) -> None:
        pass

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        return dict()

    def _call_kernel(self, functional: Callable, inpt: Any, *args: Any, **kwargs: Any) -> Any:
        kernel = _get_kernel(functional, type(inpt), allow_passthrough=True)
        return kernel(inpt, *args, **kwargs)

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        raise NotImplementedError

    def forward(self, *inputs: Any) -> Any:
        flat_inputs, spec = tree_flatten(inputs if len(inputs) > 1 else inputs[0])
        self._check_inputs(flat_inputs)
        needs = self._needs_transform_list(flat_inputs)
        params = self._get_params([i for i, n in zip(flat_inputs, needs) if n])
        flat_outputs = self._transform_all(flat_inputs, needs, params)
        return tree_unflatten(flat_outputs, spec)

    def _transform_many(self, inpts: List[Any], params: Dict[str, Any]):
        """Hook: transform several plain image tensors of one sample with the same params in one call (None = no batched
        form; GaussianBlur / RandomAdjustSharpness route a list of frames through one mv_*_v launch)."""
        return None

    def _transform_all(self, flat_inputs: List[Any], needs: List[bool], params: Dict[str, Any]) -> List[Any]:
        idx = [k for k, (i, n) in enumerate(zip(flat_inputs, needs))
               if n and type(i) in (torch.Tensor, tv_tensors.Image) and i.is_cuda]
        outs = {}
        if len(idx) > 1:
            many = self._transform_many([flat_inputs[k].as_subclass(torch.Tensor) for k in idx], params)
            if many is not None:
                for k, o in zip(idx, many):
                    like = flat_inputs[k]
                    outs[k] = tv_tensors.wrap(o, like=like) if isinstance(like, tv_tensors.TVTensor) else o
        return [outs[k] if k in outs else (self._transform(i, params) if n else i)
                for k, (i, n) in enumerate(zip(flat_inputs, needs))]

    def extra_repr(self) -> str:
        """v2/_transform.py:89-99: the public, plainly typed attributes."""
        import enum
        extra = []
        for name, value in self.__dict__.items():
            if name.startswith("_") or name == "training":
                continue
            if not isinstance(value, (bool, int, float, str, tuple, list, enum.Enum)):
                continue
            extra.append(f"{name}={value}")
        return ", ".join(extra)

    def _needs_transform_list(self, flat_inputs: List[Any]) -> List[bool]:
        # the reference's pure-tensor heuristic (_transform.py:57-87): with an explicit Image/Video in the
        # sample pure tensors pass through; otherwise only the first pure tensor is treated as the image
        has_explicit = any(isinstance(i, (tv_tensors.Image, tv_tensors.Video) + _PIL_TYPES) for i in flat_inputs)
        transform_pure_tensor = not has_explicit
        out = []
        for inpt in flat_inputs:
            needs = isinstance(inpt, self._transformed_types)
            if needs and is_pure_tensor(inpt):
                if transform_pure_tensor:
                    transform_pure_tensor = False
                else:
                    needs = False
            out.append(needs)
        return out


class _RandomApplyTransform(Transform):
    def __init__(self, p: float = 0.5) -> None:
        if not (0.0 <= p <= 1.0):
            raise ValueError("`p` should be a floating point value in the interval [0.0, 1.0].")
        super().__init__()
        self.p = p

    def forward(self, *inputs: Any) -> Any:
        inputs = inputs if len(inputs) > 1 else inputs[0]
        flat_inputs, spec = tree_flatten(inputs)
        self._check_inputs(flat_inputs)
        if torch.rand(1) >= self.p:
            return inputs
        needs = self._needs_transform_list(flat_inputs)
        params = self._get_params([i for i, n in zip(flat_inputs, needs) if n])
        flat_outputs = self._transform_all(flat_inputs, needs, params)
        return tree_unflatten(flat_outputs, spec)


class GaussianBlur(Transform):
    """v2.GaussianBlur(kernel_size, sigma=(0.1, 2.0)) -- transforms/v2/_misc.py:168-205."""

    def __init__(self, kernel_size: Union[int, Sequence[int]], sigma: Union[int, float, Sequence[float]] = (0.1, 2.0)) -> None:
        super().__init__()
        self.kernel_size = _setup_size(kernel_size, "Kernel size should be a tuple/list of two integers")
        for ks in self.kernel_size:
            if ks <= 0 or ks % 2 == 0:
                raise ValueError("Kernel size value should be an odd and positive number.")
        self.sigma = _setup_number_or_seq(sigma, "sigma")
        if not 0.0 < self.sigma[0] <= self.sigma[1]:
            raise ValueError(f"sigma values should be positive and of the form (min, max). Got {self.sigma}")

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        sigma = torch.empty(1).uniform_(self.sigma[0], self.sigma[1]).item()
        return dict(sigma=[sigma, sigma])

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.gaussian_blur, inpt, self.kernel_size, **params)

    def _transform_many(self, inpts: List[Any], params: Dict[str, Any]):
        return F.gaussian_blur_frames(inpts, list(self.kernel_size), **params)


class RandomAdjustSharpness(_RandomApplyTransform):
    """v2.RandomAdjustSharpness(sharpness_factor, p=0.5) -- transforms/v2/_color.py:356-376."""

    def __init__(self, sharpness_factor: float, p: float = 0.5) -> None:
        super().__init__(p=p)
        self.sharpness_factor = sharpness_factor

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.adjust_sharpness, inpt, sharpness_factor=self.sharpness_factor)

    def _transform_many(self, inpts: List[Any], params: Dict[str, Any]):
        if any(i.shape[-3] not in (1, 3) for i in inpts):
            return None  # the per-image kernel raises the reference's TypeError
        return F.adjust_sharpness_frames(inpts, self.sharpness_factor)


# ---- the classification preset's steps as v2 transforms (row f2): Resize -> CenterCrop -> ToDtype(float32, scale=True) ->
#      Normalize, composable with the blur / sharpness transforms above ---------------------------------------------------
class Resize(Transform):
    """v2.Resize(size, interpolation=BILINEAR, max_size=None, antialias=True) -- transforms/v2/_geometry.py:76-168.
    Bilinear with antialias (what every classification preset uses) runs on the MI355X resize kernels."""

    def __init__(self, size, interpolation=InterpolationMode.BILINEAR, max_size=None, antialias=True) -> None:
        super().__init__()
        if isinstance(size, int):
            size = [size]
        elif isinstance(size, Sequence) and len(size) in {1, 2}:
            size = list(size)
        elif size is None:
            if not isinstance(max_size, int):
                raise ValueError(f"max_size must be an integer when size is None, but got {max_size} instead.")
        else:
            raise ValueError(f"size can be an integer, a sequence of one or two integers, or None, but got {size} instead.")
        self.size = size
        self.interpolation = interpolation
        self.max_size = max_size
        self.antialias = antialias

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.resize, inpt, self.size, interpolation=self.interpolation, max_size=self.max_size,
                                 antialias=self.antialias)


class CenterCrop(Transform):
    """v2.CenterCrop(size) -- transforms/v2/_geometry.py:171-193."""

    def __init__(self, size) -> None:
        super().__init__()
        self.size = _setup_size(size, "Please provide only two dimensions (h, w) for size.")

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.center_crop, inpt, output_size=list(self.size))


class ToDtype(Transform):
    """v2.ToDtype(dtype, scale=False) -- transforms/v2/_misc.py:208-304 (a torch.dtype or a {type: dtype, "others": ...} dict)."""

    def __init__(self, dtype, scale: bool = False) -> None:
        super().__init__()
        if not isinstance(dtype, (dict, torch.dtype)):
            raise ValueError(f"dtype must be a dict or a torch.dtype, got {type(dtype)} instead")
        self.dtype = dtype
        self.scale = scale

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        if isinstance(self.dtype, torch.dtype):
            if not is_pure_tensor(inpt) and not isinstance(inpt, (tv_tensors.Image, tv_tensors.Video)):
                return inpt
            dtype = self.dtype
        elif type(inpt) in self.dtype:
            dtype = self.dtype[type(inpt)]
        elif "others" in self.dtype:
            dtype = self.dtype["others"]
        else:
            raise ValueError(f"No dtype was specified for type {type(inpt)}. "
                             "If you only need to convert the dtype of images or videos, you can just pass e.g. dtype=torch.float32. "
                             "If you're passing a dict as dtype, "
                             'you can use "others" as a catch-all key '
                             'e.g. dtype={tv_tensors.Mask: torch.int64, "others": None} to pass-through the rest of the inputs.')
        if dtype is None:
            return inpt
        return self._call_kernel(F.to_dtype, inpt, dtype=dtype, scale=self.scale)


class Normalize(Transform):
    """v2.Normalize(mean, std, inplace=False) -- transforms/v2/_misc.py:134-165."""

    def __init__(self, mean: Sequence[float], std: Sequence[float], inplace: bool = False) -> None:
        super().__init__()
        self.mean = list(mean)
        self.std = list(std)
        self.inplace = inplace

    def _check_inputs(self, flat_inputs: List[Any]) -> None:
        if any(isinstance(i, _PIL_TYPES) for i in flat_inputs):
            raise TypeError(f"{type(self).__name__}() does not support PIL images.")

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.normalize, inpt, mean=self.mean, std=self.std, inplace=self.inplace)


class Compose(Transform):
    """v2.Compose(transforms) -- transforms/v2/_container.py:10-64."""

    def __init__(self, transforms: Sequence[Callable]) -> None:
        super().__init__()
        if not isinstance(transforms, Sequence):
            raise TypeError("Argument transforms should be a sequence of callables")
        elif not transforms:
            raise ValueError("Pass at least one transform")
        self.transforms = transforms

    def forward(self, *inputs: Any) -> Any:
        needs_unpacking = len(inputs) > 1
        for transform in self.transforms:
            outputs = transform(*inputs)
            inputs = outputs if needs_unpacking else (outputs,)
        return outputs

    def extra_repr(self) -> str:
        return "\n".join(f"    {t}" for t in self.transforms)


def _check_fill_arg(fill) -> None:
    """transforms/v2/_utils.py `_check_fill_arg`."""
    if isinstance(fill, dict):
        for value in fill.values():
            _check_fill_arg(value)
    elif fill is not None and not isinstance(fill, (numbers.Number, tuple, list)):
        raise TypeError("Got inappropriate fill arg, only Numbers, tuples, lists and dicts are allowed.")


def _convert_fill_arg(fill):
    """transforms/v2/_utils.py `_convert_fill_arg`: fill = 0 is not fill = None (None skips the blend)."""
    if fill is None:
        return fill
    if not isinstance(fill, (int, float)):
        fill = [float(v) for v in list(fill)]
    return fill


def _setup_fill_arg(fill):
    """transforms/v2/_utils.py `_setup_fill_arg`: a {type: fill} dict, or one fill for every type."""
    _check_fill_arg(fill)
    if isinstance(fill, dict):
        for k, v in fill.items():
            fill[k] = _convert_fill_arg(v)
        return fill
    return {"others": _convert_fill_arg(fill)}


def _get_fill(fill_dict, inpt_type):
    """transforms/v2/_utils.py `_get_fill` (a dict with neither the type nor "others" gives None, as the reference's does)."""
    if inpt_type in fill_dict:
        return fill_dict[inpt_type]
    if "others" in fill_dict:
        return fill_dict["others"]
    return None


_PIL_INTERPOLATION_MODES = {0: InterpolationMode.NEAREST, 2: InterpolationMode.BILINEAR, 3: InterpolationMode.BICUBIC,
                            4: InterpolationMode.BOX, 5: InterpolationMode.HAMMING, 1: InterpolationMode.LANCZOS}


def _check_interpolation(interpolation) -> InterpolationMode:
    """transforms/v2/functional/_geometry.py `_check_interpolation`: an InterpolationMode or a Pillow integer constant; its
    string value ("bilinear") is accepted as well."""
    if isinstance(interpolation, int) and not isinstance(interpolation, bool):
        if interpolation not in _PIL_INTERPOLATION_MODES:
            raise ValueError(f"Interpolation mode {interpolation} is not supported.")
        return _PIL_INTERPOLATION_MODES[interpolation]
    if isinstance(interpolation, str):
        try:
            return InterpolationMode(interpolation)
        except ValueError:
            pass
    elif isinstance(interpolation, InterpolationMode):
        return interpolation
    raise ValueError(f"Argument interpolation should be an `InterpolationMode` or a corresponding Pillow integer constant, "
                     f"but got {interpolation}.")


class ElasticTransform(Transform):
    """v2.ElasticTransform(alpha=50.0, sigma=5.0, interpolation=BILINEAR, fill=0) -- transforms/v2/_geometry.py:1003-1085.

    `_get_params` (row a9): a U(-1, 1) noise field per axis, blurred with a Gaussian of `k = int(8 * sigma + 1) | 1` taps per
    side, scaled by `alpha / size`.  The noise is drawn from the HOST generator with the reference's calls in the reference's
    order (`torch.rand([1, 1, H, W]) * 2 - 1`, dx then dy), so a seeded pipeline samples the same displacement field; the
    blur -- 41 x 41 taps at the default sigma = 5 -- runs on the MI355X and the field stays there.

    `_transform` applies the field with `F.elastic` (one mv_elastic_* launch per image, video or mask: grid_sample at
    identity grid + displacement and the fill blend, the reference's bits).  `fill` is the reference's: a number, a
    sequence, None (no blend) or a {type: fill} dict; masks are resampled with nearest; BoundingBoxes raise (not warped)."""

    def __init__(self, alpha: Union[float, Sequence[float]] = 50.0, sigma: Union[float, Sequence[float]] = 5.0,
                 interpolation: Union[InterpolationMode, str, int] = InterpolationMode.BILINEAR, fill=0) -> None:
        super().__init__()
        self.alpha = _setup_number_or_seq(alpha, "alpha")
        self.sigma = _setup_number_or_seq(sigma, "sigma")
        self.interpolation = _check_interpolation(interpolation)
        self.fill = fill
        self._fill = _setup_fill_arg(fill)

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        size = list(query_size(flat_inputs))
        device = _pil.device_for_host_inputs()

        dx = torch.rand([1, 1] + size) * 2 - 1
        if self.sigma[0] > 0.0:
            kx = int(8 * self.sigma[0] + 1)
            # if kernel size is even we have to make it odd
            if kx % 2 == 0:
                kx += 1
            dx = self._call_kernel(F.gaussian_blur, dx.to(device), [kx, kx], list(self.sigma))
        dx = dx.to(device) * self.alpha[0] / size[0]

        dy = torch.rand([1, 1] + size) * 2 - 1
        if self.sigma[1] > 0.0:
            ky = int(8 * self.sigma[1] + 1)
            if ky % 2 == 0:
                ky += 1
            dy = self._call_kernel(F.gaussian_blur, dy.to(device), [ky, ky], list(self.sigma))
        dy = dy.to(device) * self.alpha[1] / size[1]
        displacement = torch.concat([dx, dy], 1).permute([0, 2, 3, 1])  # 1 x H x W x 2
        return dict(displacement=displacement)

    def get_params(self, *inputs: Any) -> Dict[str, Any]:
        """Sample the displacement field for a sample (public form of `_get_params`)."""
        flat_inputs, _ = tree_flatten(inputs if len(inputs) > 1 else inputs[0])
        return self._get_params(flat_inputs)

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        if "displacement" not in params:
            raise NotImplementedError(
                "ElasticTransform: the params hold no displacement field to resample with grid_sample (F.elastic); use "
                "forward() or get_params(sample).")
        fill = _get_fill(self._fill, type(inpt))
        return self._call_kernel(F.elastic, inpt, **params, fill=fill, interpolation=self.interpolation)


def _check_sequence_input(x, name: str, req_sizes) -> None:
    """transforms/v2/_utils.py `_check_sequence_input`."""
    msg = req_sizes[0] if len(req_sizes) < 2 else " or ".join([str(s) for s in req_sizes])
    if not isinstance(x, Sequence):
        raise TypeError(f"{name} should be a sequence of length {msg}.")
    if len(x) not in req_sizes:
        raise ValueError(f"{name} should be a sequence of length {msg}.")


def _setup_angle(x, name: str, req_sizes=(2,)) -> List[float]:
    """transforms/v2/_utils.py `_setup_angle`: a number d gives [-d, d]."""
    if isinstance(x, numbers.Number):
        if x < 0:
            raise ValueError(f"If {name} is a single number, it must be positive.")
        x = [-x, x]
    else:
        _check_sequence_input(x, name, req_sizes)
    return [float(d) for d in x]


class RandomRotation(Transform):
    """v2.RandomRotation(degrees, interpolation=NEAREST, expand=False, center=None, fill=0) -- transforms/v2/_geometry.py.

    The angle is drawn from the host generator as the reference draws it (`torch.empty(1).uniform_`); `F.rotate` resamples
    images, videos and masks (nearest) in one mv_warp_* launch each.  The default fill = 0 runs the fill blend, which for
    bilinear is not the same as fill=None."""

    def __init__(self, degrees: Union[numbers.Number, Sequence], interpolation=InterpolationMode.NEAREST, expand: bool = False,
                 center: Optional[List[float]] = None, fill=0) -> None:
        super().__init__()
        self.degrees = _setup_angle(degrees, name="degrees", req_sizes=(2,))
        self.interpolation = _check_interpolation(interpolation)
        self.expand = expand
        self.fill = fill
        self._fill = _setup_fill_arg(fill)
        if center is not None:
            _check_sequence_input(center, "center", req_sizes=(2,))
        self.center = center

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        angle = torch.empty(1).uniform_(self.degrees[0], self.degrees[1]).item()
        return dict(angle=angle)

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        fill = _get_fill(self._fill, type(inpt))
        return self._call_kernel(F.rotate, inpt, **params, interpolation=self.interpolation, expand=self.expand,
                                 center=self.center, fill=fill)


class RandomAffine(Transform):
    """v2.RandomAffine(degrees, translate=None, scale=None, shear=None, interpolation=NEAREST, fill=0, center=None) --
    transforms/v2/_geometry.py.  `_get_params` draws angle, translation, scale and shear from the host generator with the
    reference's calls in the reference's order; `F.affine` resamples in one mv_warp_* launch per image, video or mask."""

    def __init__(self, degrees: Union[numbers.Number, Sequence], translate: Optional[Sequence[float]] = None,
                 scale: Optional[Sequence[float]] = None, shear: Optional[Union[int, float, Sequence[float]]] = None,
                 interpolation=InterpolationMode.NEAREST, fill=0, center: Optional[List[float]] = None) -> None:
        super().__init__()
        self.degrees = _setup_angle(degrees, name="degrees", req_sizes=(2,))
        if translate is not None:
            _check_sequence_input(translate, "translate", req_sizes=(2,))
            for t in translate:
                if not (0.0 <= t <= 1.0):
                    raise ValueError("translation values should be between 0 and 1")
        self.translate = translate
        if scale is not None:
            _check_sequence_input(scale, "scale", req_sizes=(2,))
            for s in scale:
                if s <= 0:
                    raise ValueError("scale values should be positive")
        self.scale = scale
        if shear is not None:
            self.shear = _setup_angle(shear, name="shear", req_sizes=(2, 4))
        else:
            self.shear = shear
        self.interpolation = _check_interpolation(interpolation)
        self.fill = fill
        self._fill = _setup_fill_arg(fill)
        if center is not None:
            _check_sequence_input(center, "center", req_sizes=(2,))
        self.center = center

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        height, width = query_size(flat_inputs)
        angle = torch.empty(1).uniform_(self.degrees[0], self.degrees[1]).item()
        if self.translate is not None:
            max_dx = float(self.translate[0] * width)
            max_dy = float(self.translate[1] * height)
            tx = int(round(torch.empty(1).uniform_(-max_dx, max_dx).item()))
            ty = int(round(torch.empty(1).uniform_(-max_dy, max_dy).item()))
            translate = (tx, ty)
        else:
            translate = (0, 0)
        if self.scale is not None:
            scale = torch.empty(1).uniform_(self.scale[0], self.scale[1]).item()
        else:
            scale = 1.0
        shear_x = shear_y = 0.0
        if self.shear is not None:
            shear_x = torch.empty(1).uniform_(self.shear[0], self.shear[1]).item()
            if len(self.shear) == 4:
                shear_y = torch.empty(1).uniform_(self.shear[2], self.shear[3]).item()
        shear = (shear_x, shear_y)
        return dict(angle=angle, translate=translate, scale=scale, shear=shear)

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        fill = _get_fill(self._fill, type(inpt))
        return self._call_kernel(F.affine, inpt, **params, interpolation=self.interpolation, fill=fill, center=self.center)


class RandomPerspective(_RandomApplyTransform):
    """v2.RandomPerspective(distortion_scale=0.5, p=0.5, interpolation=BILINEAR, fill=0) -- transforms/v2/_geometry.py.
    `_get_params` draws the four displaced corners with the reference's `torch.randint` calls in its order and solves the 8
    coefficients on the host (float64 least squares); `F.perspective` resamples in one mv_warp_* launch."""

    def __init__(self, distortion_scale: float = 0.5, p: float = 0.5, interpolation=InterpolationMode.BILINEAR,
                 fill=0) -> None:
        super().__init__(p=p)
        if not (0 <= distortion_scale <= 1):
            raise ValueError("Argument distortion_scale value should be between 0 and 1")
        self.distortion_scale = distortion_scale
        self.interpolation = _check_interpolation(interpolation)
        self.fill = fill
        self._fill = _setup_fill_arg(fill)

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        height, width = query_size(flat_inputs)
        distortion_scale = self.distortion_scale
        half_height = height // 2
        half_width = width // 2
        bound_height = int(distortion_scale * half_height) + 1
        bound_width = int(distortion_scale * half_width) + 1
        topleft = [
            int(torch.randint(0, bound_width, size=(1,))),
            int(torch.randint(0, bound_height, size=(1,))),
        ]
        topright = [
            int(torch.randint(width - bound_width, width, size=(1,))),
            int(torch.randint(0, bound_height, size=(1,))),
        ]
        botright = [
            int(torch.randint(width - bound_width, width, size=(1,))),
            int(torch.randint(height - bound_height, height, size=(1,))),
        ]
        botleft = [
            int(torch.randint(0, bound_width, size=(1,))),
            int(torch.randint(height - bound_height, height, size=(1,))),
        ]
        startpoints = [[0, 0], [width - 1, 0], [width - 1, height - 1], [0, height - 1]]
        endpoints = [topleft, topright, botright, botleft]
        perspective_coeffs = F._get_perspective_coeffs(startpoints, endpoints)
        return dict(coefficients=perspective_coeffs)

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        fill = _get_fill(self._fill, type(inpt))
        return self._call_kernel(F.perspective, inpt, startpoints=None, endpoints=None, fill=fill,
                                 interpolation=self.interpolation, **params)


_COLOR_JITTER_OPS = ("brightness", "contrast", "saturation", "hue")


class ColorJitter(Transform):
    """v2.ColorJitter(brightness=None, contrast=None, saturation=None, hue=None) -- transforms/v2/_color.py.

    `_get_params` draws with the reference's host RNG calls in its order: torch.randperm(4), then one
    torch.empty(1).uniform_ per configured factor (brightness, contrast, saturation, hue).  A float32 / uint8 tensor, Image or
    Video on the device goes through the whole chain in ONE call (F.color_jitter_image: one pass, two with contrast); any
    other input takes the reference's loop of single F.adjust_* calls.  Both give the same bits."""

    def __init__(self, brightness=None, contrast=None, saturation=None, hue=None) -> None:
        super().__init__()
        self.brightness = self._check_input(brightness, "brightness")
        self.contrast = self._check_input(contrast, "contrast")
        self.saturation = self._check_input(saturation, "saturation")
        self.hue = self._check_input(hue, "hue", center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)

    def _check_input(self, value, name: str, center: float = 1.0, bound: Tuple[float, float] = (0, float("inf")),
                     clip_first_on_zero: bool = True) -> Optional[Tuple[float, float]]:
        if value is None:
            return None
        if isinstance(value, (int, float)):
            if value < 0:
                raise ValueError(f"If {name} is a single number, it must be non negative.")
            value = [center - value, center + value]
            if clip_first_on_zero:
                value[0] = max(value[0], 0.0)
        elif isinstance(value, collections.abc.Sequence) and len(value) == 2:
            value = [float(v) for v in value]
        else:
            raise TypeError(f"{name}={value} should be a single number or a sequence with length 2.")
        if not bound[0] <= value[0] <= value[1] <= bound[1]:
            raise ValueError(f"{name} values should be between {bound}, but got {value}.")
        return None if value[0] == value[1] == center else (float(value[0]), float(value[1]))

    @staticmethod
    def _generate_value(left: float, right: float) -> float:
        return torch.empty(1).uniform_(left, right).item()

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        fn_idx = torch.randperm(4)
        b = None if self.brightness is None else self._generate_value(self.brightness[0], self.brightness[1])
        c = None if self.contrast is None else self._generate_value(self.contrast[0], self.contrast[1])
        s = None if self.saturation is None else self._generate_value(self.saturation[0], self.saturation[1])
        h = None if self.hue is None else self._generate_value(self.hue[0], self.hue[1])
        return dict(fn_idx=fn_idx, brightness_factor=b, contrast_factor=c, saturation_factor=s, hue_factor=h)

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        ops = []
        for fn_id in params["fn_idx"]:
            name = _COLOR_JITTER_OPS[int(fn_id)]
            factor = params[name + "_factor"]
            if factor is not None:
                ops.append((name, factor))
        if (ops and type(inpt) in (torch.Tensor, tv_tensors.Image, tv_tensors.Video) and inpt.is_cuda
                and inpt.dtype in (torch.float32, torch.uint8) and inpt.numel() > 0):
            plain = inpt.as_subclass(torch.Tensor)
            out = F.color_jitter_image(plain, ops)
            if out is plain:
                return inpt  # saturation and hue alone leave a 1-channel image as it is
            return tv_tensors.wrap(out, like=inpt) if isinstance(inpt, tv_tensors.TVTensor) else out
        output = inpt
        for name, factor in ops:
            functional = getattr(F, "adjust_" + name)
            output = self._call_kernel(functional, output, **{name + "_factor": factor})
        return output


class Grayscale(Transform):
    """v2.Grayscale(num_output_channels=1) -- transforms/v2/_color.py (-> F.rgb_to_grayscale; masks, boxes and videos pass
    through, as in the reference)."""

    def __init__(self, num_output_channels: int = 1) -> None:
        super().__init__()
        self.num_output_channels = num_output_channels

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.rgb_to_grayscale, inpt, num_output_channels=self.num_output_channels)


class RandomGrayscale(_RandomApplyTransform):
    """v2.RandomGrayscale(p=0.1) -- transforms/v2/_color.py: grey with as many channels as the input has."""

    def __init__(self, p: float = 0.1) -> None:
        super().__init__(p=p)

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        num_input_channels, *_ = query_chw(flat_inputs)
        return dict(num_input_channels=num_input_channels)

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.rgb_to_grayscale, inpt, num_output_channels=params["num_input_channels"])


class RandomInvert(_RandomApplyTransform):
    """v2.RandomInvert(p=0.5) -- transforms/v2/_color.py (-> F.invert)."""

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.invert, inpt)


class RandomPosterize(_RandomApplyTransform):
    """v2.RandomPosterize(bits, p=0.5) -- transforms/v2/_color.py (-> F.posterize)."""

    def __init__(self, bits: int, p: float = 0.5) -> None:
        super().__init__(p=p)
        self.bits = bits

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.posterize, inpt, bits=self.bits)


class RandomSolarize(_RandomApplyTransform):
    """v2.RandomSolarize(threshold, p=0.5) -- transforms/v2/_color.py (-> F.solarize)."""

    def __init__(self, threshold: float, p: float = 0.5) -> None:
        super().__init__(p=p)
        self.threshold = threshold

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.solarize, inpt, threshold=self.threshold)


class RandomAutocontrast(_RandomApplyTransform):
    """v2.RandomAutocontrast(p=0.5) -- transforms/v2/_color.py (-> F.autocontrast)."""

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.autocontrast, inpt)


class RandomEqualize(_RandomApplyTransform):
    """v2.RandomEqualize(p=0.5) -- transforms/v2/_color.py (-> F.equalize)."""

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.equalize, inpt)


class AutoAugmentPolicy(_enum.Enum):
    """transforms/autoaugment.py `AutoAugmentPolicy`: the policies learned on these datasets."""

    IMAGENET = "imagenet"
    CIFAR10 = "cifar10"
    SVHN = "svhn"


class _AutoAugmentBase(Transform):
    """transforms/v2/_auto_augment.py `_AutoAugmentBase`: one image or video per sample, ops applied one by one through the
    F.* dispatchers.  The draws are the reference's host RNG calls in its order; PIL images raise NotImplementedError before
    any draw."""

    _AUGMENTATION_SPACE: Dict[str, Tuple[Callable[[int, int, int], Optional[torch.Tensor]], bool]] = {}

    def __init__(self, *, interpolation=InterpolationMode.NEAREST, fill=None) -> None:
        super().__init__()
        self.interpolation = _check_interpolation(interpolation)
        self.fill = fill
        self._fill = _setup_fill_arg(fill)

    def _get_random_item(self, dct: Dict[str, Any]) -> Tuple[str, Any]:
        keys = tuple(dct.keys())
        key = keys[int(torch.randint(len(keys), ()))]
        return key, dct[key]

    def _flatten_and_extract_image_or_video(self, inputs: Any, unsupported_types=(tv_tensors.BoundingBoxes, tv_tensors.Mask)):
        flat_inputs, spec = tree_flatten(inputs if len(inputs) > 1 else inputs[0])
        needs_transform_list = self._needs_transform_list(flat_inputs)
        image_or_videos = []
        for idx, (inpt, needs_transform) in enumerate(zip(flat_inputs, needs_transform_list)):
            if needs_transform and (isinstance(inpt, (tv_tensors.Image, tv_tensors.Video) + _PIL_TYPES)
                                    or is_pure_tensor(inpt)):
                image_or_videos.append((idx, inpt))
            elif isinstance(inpt, unsupported_types):
                raise TypeError(f"Inputs of type {type(inpt).__name__} are not supported by {type(self).__name__}()")
        if not image_or_videos:
            raise TypeError("Found no image in the sample.")
        if len(image_or_videos) > 1:
            raise TypeError(f"Auto augment transformations are only properly defined for a single image or video, "
                            f"but found {len(image_or_videos)}.")
        idx, image_or_video = image_or_videos[0]
        if isinstance(image_or_video, _PIL_TYPES):
            raise NotImplementedError(f"{type(self).__name__}: PIL images go through Pillow's ImageOps / ImageEnhance in "
                                      "the reference, which this library does not reproduce; convert with pil_to_tensor")
        return (flat_inputs, spec, idx), image_or_video

    def _unflatten_and_insert_image_or_video(self, flat_inputs_with_spec, image_or_video: Any) -> Any:
        flat_inputs, spec, idx = flat_inputs_with_spec
        flat_inputs[idx] = image_or_video
        return tree_unflatten(flat_inputs, spec)

    def _apply_image_or_video_transform(self, image: Any, transform_id: str, magnitude: float, interpolation, fill) -> Any:
        fill_ = _get_fill(fill, type(image))
        if transform_id == "Identity":
            return image
        elif transform_id == "ShearX":
            # tan of the shear angle is the magnitude (the official AutoAugment's (1, level, 0, 0, 1, 0))
            return F.affine(image, angle=0.0, translate=[0, 0], scale=1.0, shear=[math.degrees(math.atan(magnitude)), 0.0],
                            interpolation=interpolation, fill=fill_, center=[0, 0])
        elif transform_id == "ShearY":
            return F.affine(image, angle=0.0, translate=[0, 0], scale=1.0, shear=[0.0, math.degrees(math.atan(magnitude))],
                            interpolation=interpolation, fill=fill_, center=[0, 0])
        elif transform_id == "TranslateX":
            return F.affine(image, angle=0.0, translate=[int(magnitude), 0], scale=1.0, interpolation=interpolation,
                            shear=[0.0, 0.0], fill=fill_)
        elif transform_id == "TranslateY":
            return F.affine(image, angle=0.0, translate=[0, int(magnitude)], scale=1.0, interpolation=interpolation,
                            shear=[0.0, 0.0], fill=fill_)
        elif transform_id == "Rotate":
            return F.rotate(image, angle=magnitude, interpolation=interpolation, fill=fill_)
        elif transform_id == "Brightness":
            return F.adjust_brightness(image, brightness_factor=1.0 + magnitude)
        elif transform_id == "Color":
            return F.adjust_saturation(image, saturation_factor=1.0 + magnitude)
        elif transform_id == "Contrast":
            return F.adjust_contrast(image, contrast_factor=1.0 + magnitude)
        elif transform_id == "Sharpness":
            return F.adjust_sharpness(image, sharpness_factor=1.0 + magnitude)
        elif transform_id == "Posterize":
            return F.posterize(image, bits=int(magnitude))
        elif transform_id == "Solarize":
            bound = F._max_value(image.dtype)
            return F.solarize(image, threshold=bound * magnitude)
        elif transform_id == "AutoContrast":
            return F.autocontrast(image)
        elif transform_id == "Equalize":
            return F.equalize(image)
        elif transform_id == "Invert":
            return F.invert(image)
        else:
            raise ValueError(f"No transform available for {transform_id}")

    def _apply(self, image_or_video: Any, transform_id: str, magnitude: float) -> Any:
        return self._apply_image_or_video_transform(image_or_video, transform_id, magnitude,
                                                    interpolation=self.interpolation, fill=self._fill)

    @staticmethod
    def _size(image_or_video: Any) -> Tuple[int, int]:
        h, w = image_or_video.shape[-2:]
        return int(h), int(w)


def _linspace(start: float, end: float):
    return lambda num_bins, height, width: torch.linspace(start, end, num_bins)


def _posterize_bits(levels: int):
    return lambda num_bins, height, width: (8 - (torch.arange(num_bins) / ((num_bins - 1) / levels))).round().int()


def _none(num_bins, height, width):
    return None


class AutoAugment(_AutoAugmentBase):
    """v2.AutoAugment(policy=IMAGENET, interpolation=NEAREST, fill=None) -- transforms/v2/_auto_augment.py: one of the
    policy's 25 sub-policies per sample (torch.randint), each of its two ops applied when torch.rand(()) <= its probability,
    signed magnitudes negated when torch.rand(()) <= 0.5."""

    _AUGMENTATION_SPACE = {
        "ShearX": (_linspace(0.0, 0.3), True),
        "ShearY": (_linspace(0.0, 0.3), True),
        "TranslateX": (lambda num_bins, height, width: torch.linspace(0.0, 150.0 / 331.0 * width, num_bins), True),
        "TranslateY": (lambda num_bins, height, width: torch.linspace(0.0, 150.0 / 331.0 * height, num_bins), True),
        "Rotate": (_linspace(0.0, 30.0), True),
        "Brightness": (_linspace(0.0, 0.9), True),
        "Color": (_linspace(0.0, 0.9), True),
        "Contrast": (_linspace(0.0, 0.9), True),
        "Sharpness": (_linspace(0.0, 0.9), True),
        "Posterize": (_posterize_bits(4), False),
        "Solarize": (_linspace(1.0, 0.0), False),
        "AutoContrast": (_none, False),
        "Equalize": (_none, False),
        "Invert": (_none, False),
    }

    def __init__(self, policy: AutoAugmentPolicy = AutoAugmentPolicy.IMAGENET, interpolation=InterpolationMode.NEAREST,
                 fill=None) -> None:
        super().__init__(interpolation=interpolation, fill=fill)
        self.policy = policy
        self._policies = self._get_policies(policy)

    def _get_policies(self, policy: AutoAugmentPolicy):
        if policy == AutoAugmentPolicy.IMAGENET:
            return [
                (("Posterize", 0.4, 8), ("Rotate", 0.6, 9)),
                (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)),
                (("Equalize", 0.8, None), ("Equalize", 0.6, None)),
                (("Posterize", 0.6, 7), ("Posterize", 0.6, 6)),
                (("Equalize", 0.4, None), ("Solarize", 0.2, 4)),
                (("Equalize", 0.4, None), ("Rotate", 0.8, 8)),
                (("Solarize", 0.6, 3), ("Equalize", 0.6, None)),
                (("Posterize", 0.8, 5), ("Equalize", 1.0, None)),
                (("Rotate", 0.2, 3), ("Solarize", 0.6, 8)),
                (("Equalize", 0.6, None), ("Posterize", 0.4, 6)),
                (("Rotate", 0.8, 8), ("Color", 0.4, 0)),
                (("Rotate", 0.4, 9), ("Equalize", 0.6, None)),
                (("Equalize", 0.0, None), ("Equalize", 0.8, None)),
                (("Invert", 0.6, None), ("Equalize", 1.0, None)),
                (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
                (("Rotate", 0.8, 8), ("Color", 1.0, 2)),
                (("Color", 0.8, 8), ("Solarize", 0.8, 7)),
                (("Sharpness", 0.4, 7), ("Invert", 0.6, None)),
                (("ShearX", 0.6, 5), ("Equalize", 1.0, None)),
                (("Color", 0.4, 0), ("Equalize", 0.6, None)),
                (("Equalize", 0.4, None), ("Solarize", 0.2, 4)),
                (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)),
                (("Invert", 0.6, None), ("Equalize", 1.0, None)),
                (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
                (("Equalize", 0.8, None), ("Equalize", 0.6, None)),
            ]
        elif policy == AutoAugmentPolicy.CIFAR10:
            return [
                (("Invert", 0.1, None), ("Contrast", 0.2, 6)),
                (("Rotate", 0.7, 2), ("TranslateX", 0.3, 9)),
                (("Sharpness", 0.8, 1), ("Sharpness", 0.9, 3)),
                (("ShearY", 0.5, 8), ("TranslateY", 0.7, 9)),
                (("AutoContrast", 0.5, None), ("Equalize", 0.9, None)),
                (("ShearY", 0.2, 7), ("Posterize", 0.3, 7)),
                (("Color", 0.4, 3), ("Brightness", 0.6, 7)),
                (("Sharpness", 0.3, 9), ("Brightness", 0.7, 9)),
                (("Equalize", 0.6, None), ("Equalize", 0.5, None)),
                (("Contrast", 0.6, 7), ("Sharpness", 0.6, 5)),
                (("Color", 0.7, 7), ("TranslateX", 0.5, 8)),
                (("Equalize", 0.3, None), ("AutoContrast", 0.4, None)),
                (("TranslateY", 0.4, 3), ("Sharpness", 0.2, 6)),
                (("Brightness", 0.9, 6), ("Color", 0.2, 8)),
                (("Solarize", 0.5, 2), ("Invert", 0.0, None)),
                (("Equalize", 0.2, None), ("AutoContrast", 0.6, None)),
                (("Equalize", 0.2, None), ("Equalize", 0.6, None)),
                (("Color", 0.9, 9), ("Equalize", 0.6, None)),
                (("AutoContrast", 0.8, None), ("Solarize", 0.2, 8)),
                (("Brightness", 0.1, 3), ("Color", 0.7, 0)),
                (("Solarize", 0.4, 5), ("AutoContrast", 0.9, None)),
                (("TranslateY", 0.9, 9), ("TranslateY", 0.7, 9)),
                (("AutoContrast", 0.9, None), ("Solarize", 0.8, 3)),
                (("Equalize", 0.8, None), ("Invert", 0.1, None)),
                (("TranslateY", 0.7, 9), ("AutoContrast", 0.9, None)),
            ]
        elif policy == AutoAugmentPolicy.SVHN:
            return [
                (("ShearX", 0.9, 4), ("Invert", 0.2, None)),
                (("ShearY", 0.9, 8), ("Invert", 0.7, None)),
                (("Equalize", 0.6, None), ("Solarize", 0.6, 6)),
                (("Invert", 0.9, None), ("Equalize", 0.6, None)),
                (("Equalize", 0.6, None), ("Rotate", 0.9, 3)),
                (("ShearX", 0.9, 4), ("AutoContrast", 0.8, None)),
                (("ShearY", 0.9, 8), ("Invert", 0.4, None)),
                (("ShearY", 0.9, 5), ("Solarize", 0.2, 6)),
                (("Invert", 0.9, None), ("AutoContrast", 0.8, None)),
                (("Equalize", 0.6, None), ("Rotate", 0.9, 3)),
                (("ShearX", 0.9, 4), ("Solarize", 0.3, 3)),
                (("ShearY", 0.8, 8), ("Invert", 0.7, None)),
                (("Equalize", 0.9, None), ("TranslateY", 0.6, 6)),
                (("Invert", 0.9, None), ("Equalize", 0.6, None)),
                (("Contrast", 0.3, 3), ("Rotate", 0.8, 4)),
                (("Invert", 0.8, None), ("TranslateY", 0.0, 2)),
                (("ShearY", 0.7, 6), ("Solarize", 0.4, 8)),
                (("Invert", 0.6, None), ("Rotate", 0.8, 4)),
                (("ShearY", 0.3, 7), ("TranslateX", 0.9, 3)),
                (("ShearX", 0.1, 6), ("Invert", 0.6, None)),
                (("Solarize", 0.7, 2), ("TranslateY", 0.6, 7)),
                (("ShearY", 0.8, 4), ("Invert", 0.8, None)),
                (("ShearX", 0.7, 9), ("TranslateY", 0.8, 3)),
                (("ShearY", 0.8, 5), ("AutoContrast", 0.7, None)),
                (("ShearX", 0.7, 2), ("Invert", 0.1, None)),
            ]
        else:
            raise ValueError(f"The provided policy {policy} is not recognized.")

    def forward(self, *inputs: Any) -> Any:
        flat_inputs_with_spec, image_or_video = self._flatten_and_extract_image_or_video(inputs)
        height, width = self._size(image_or_video)
        policy = self._policies[int(torch.randint(len(self._policies), ()))]
        for transform_id, probability, magnitude_idx in policy:
            if not torch.rand(()) <= probability:
                continue
            magnitudes_fn, signed = self._AUGMENTATION_SPACE[transform_id]
            magnitudes = magnitudes_fn(10, height, width)
            if magnitudes is not None:
                magnitude = float(magnitudes[magnitude_idx])
                if signed and torch.rand(()) <= 0.5:
                    magnitude *= -1
            else:
                magnitude = 0.0
            image_or_video = self._apply(image_or_video, transform_id, magnitude)
        return self._unflatten_and_insert_image_or_video(flat_inputs_with_spec, image_or_video)


class RandAugment(_AutoAugmentBase):
    """v2.RandAugment(num_ops=2, magnitude=9, num_magnitude_bins=31, interpolation=NEAREST, fill=None) --
    transforms/v2/_auto_augment.py: num_ops ops drawn uniformly from the space (torch.randint), each at the fixed magnitude
    bin, signed magnitudes negated when torch.rand(()) <= 0.5."""

    _AUGMENTATION_SPACE = {
        "Identity": (_none, False),
        "ShearX": (_linspace(0.0, 0.3), True),
        "ShearY": (_linspace(0.0, 0.3), True),
        "TranslateX": (lambda num_bins, height, width: torch.linspace(0.0, 150.0 / 331.0 * width, num_bins), True),
        "TranslateY": (lambda num_bins, height, width: torch.linspace(0.0, 150.0 / 331.0 * height, num_bins), True),
        "Rotate": (_linspace(0.0, 30.0), True),
        "Brightness": (_linspace(0.0, 0.9), True),
        "Color": (_linspace(0.0, 0.9), True),
        "Contrast": (_linspace(0.0, 0.9), True),
        "Sharpness": (_linspace(0.0, 0.9), True),
        "Posterize": (_posterize_bits(4), False),
        "Solarize": (_linspace(1.0, 0.0), False),
        "AutoContrast": (_none, False),
        "Equalize": (_none, False),
    }

    def __init__(self, num_ops: int = 2, magnitude: int = 9, num_magnitude_bins: int = 31,
                 interpolation=InterpolationMode.NEAREST, fill=None) -> None:
        super().__init__(interpolation=interpolation, fill=fill)
        self.num_ops = num_ops
        self.magnitude = magnitude
        self.num_magnitude_bins = num_magnitude_bins

    def forward(self, *inputs: Any) -> Any:
        flat_inputs_with_spec, image_or_video = self._flatten_and_extract_image_or_video(inputs)
        height, width = self._size(image_or_video)
        for _ in range(self.num_ops):
            transform_id, (magnitudes_fn, signed) = self._get_random_item(self._AUGMENTATION_SPACE)
            magnitudes = magnitudes_fn(self.num_magnitude_bins, height, width)
            if magnitudes is not None:
                magnitude = float(magnitudes[self.magnitude])
                if signed and torch.rand(()) <= 0.5:
                    magnitude *= -1
            else:
                magnitude = 0.0
            image_or_video = self._apply(image_or_video, transform_id, magnitude)
        return self._unflatten_and_insert_image_or_video(flat_inputs_with_spec, image_or_video)


class TrivialAugmentWide(_AutoAugmentBase):
    """v2.TrivialAugmentWide(num_magnitude_bins=31, interpolation=NEAREST, fill=None) -- transforms/v2/_auto_augment.py: one
    op drawn uniformly from the space (torch.randint), a magnitude bin drawn uniformly (torch.randint, only for ops with
    magnitudes), signed magnitudes negated when torch.rand(()) <= 0.5."""

    _AUGMENTATION_SPACE = {
        "Identity": (_none, False),
        "ShearX": (_linspace(0.0, 0.99), True),
        "ShearY": (_linspace(0.0, 0.99), True),
        "TranslateX": (_linspace(0.0, 32.0), True),
        "TranslateY": (_linspace(0.0, 32.0), True),
        "Rotate": (_linspace(0.0, 135.0), True),
        "Brightness": (_linspace(0.0, 0.99), True),
        "Color": (_linspace(0.0, 0.99), True),
        "Contrast": (_linspace(0.0, 0.99), True),
        "Sharpness": (_linspace(0.0, 0.99), True),
        "Posterize": (_posterize_bits(6), False),
        "Solarize": (_linspace(1.0, 0.0), False),
        "AutoContrast": (_none, False),
        "Equalize": (_none, False),
    }

    def __init__(self, num_magnitude_bins: int = 31, interpolation=InterpolationMode.NEAREST, fill=None) -> None:
        super().__init__(interpolation=interpolation, fill=fill)
        self.num_magnitude_bins = num_magnitude_bins

    def forward(self, *inputs: Any) -> Any:
        flat_inputs_with_spec, image_or_video = self._flatten_and_extract_image_or_video(inputs)
        height, width = self._size(image_or_video)
        transform_id, (magnitudes_fn, signed) = self._get_random_item(self._AUGMENTATION_SPACE)
        magnitudes = magnitudes_fn(self.num_magnitude_bins, height, width)
        if magnitudes is not None:
            magnitude = float(magnitudes[int(torch.randint(self.num_magnitude_bins, ()))])
            if signed and torch.rand(()) <= 0.5:
                magnitude *= -1
        else:
            magnitude = 0.0
        image_or_video = self._apply(image_or_video, transform_id, magnitude)
        return self._unflatten_and_insert_image_or_video(flat_inputs_with_spec, image_or_video)


# ---- the training recipes' geometry: flips, Pad, RandomCrop, RandomResizedCrop, RandomErasing (v2/_geometry.py, v2/_augment.py).
#      The host RNG calls are the reference's, in its order.
def _check_padding_arg(padding) -> None:
    """transforms/v2/_utils.py `_check_padding_arg`."""
    if not isinstance(padding, (numbers.Number, tuple, list)):
        raise TypeError("Got inappropriate padding arg")
    if isinstance(padding, (tuple, list)) and len(padding) not in [1, 2, 4]:
        raise ValueError(f"Padding must be an int or a 1, 2, or 4 element tuple, not a {len(padding)} element tuple")


def _check_padding_mode_arg(padding_mode) -> None:
    """transforms/v2/_utils.py `_check_padding_mode_arg`."""
    if padding_mode not in ["constant", "edge", "reflect", "symmetric"]:
        raise ValueError("Padding mode should be either constant, edge, reflect or symmetric")


class RandomHorizontalFlip(_RandomApplyTransform):
    """v2.RandomHorizontalFlip(p=0.5) -- transforms/v2/_geometry.py."""

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.horizontal_flip, inpt)


class RandomVerticalFlip(_RandomApplyTransform):
    """v2.RandomVerticalFlip(p=0.5) -- transforms/v2/_geometry.py."""

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.vertical_flip, inpt)


class Pad(Transform):
    """v2.Pad(padding, fill=0, padding_mode="constant") -- transforms/v2/_geometry.py."""

    def __init__(self, padding, fill=0, padding_mode: str = "constant") -> None:
        super().__init__()
        _check_padding_arg(padding)
        _check_padding_mode_arg(padding_mode)
        if not isinstance(padding, int):
            padding = list(padding)
        self.padding = padding
        self.fill = fill
        self._fill = _setup_fill_arg(fill)
        self.padding_mode = padding_mode

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        fill = _get_fill(self._fill, type(inpt))
        return self._call_kernel(F.pad, inpt, padding=self.padding, fill=fill, padding_mode=self.padding_mode)


class RandomCrop(Transform):
    """v2.RandomCrop(size, padding=None, pad_if_needed=False, fill=0, padding_mode="constant") -- transforms/v2/_geometry.py.
    When a sample is both padded and cropped the two steps run as ONE gather launch (F.pad_crop)."""

    def __init__(self, size, padding=None, pad_if_needed: bool = False, fill=0, padding_mode: str = "constant") -> None:
        super().__init__()
        self.size = _setup_size(size, "Please provide only two dimensions (h, w) for size.")
        if pad_if_needed or padding is not None:
            if padding is not None:
                _check_padding_arg(padding)
            _check_padding_mode_arg(padding_mode)
        self.padding = F._parse_pad_padding(padding) if padding else None
        self.pad_if_needed = pad_if_needed
        self.fill = fill
        self._fill = _setup_fill_arg(fill)
        self.padding_mode = padding_mode

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        padded_height, padded_width = query_size(flat_inputs)
        if self.padding is not None:
            pad_left, pad_right, pad_top, pad_bottom = self.padding
            padded_height += pad_top + pad_bottom
            padded_width += pad_left + pad_right
        else:
            pad_left = pad_right = pad_top = pad_bottom = 0
        cropped_height, cropped_width = self.size
        if self.pad_if_needed:
            if padded_height < cropped_height:
                diff = cropped_height - padded_height
                pad_top += diff
                pad_bottom += diff
                padded_height += 2 * diff
            if padded_width < cropped_width:
                diff = cropped_width - padded_width
                pad_left += diff
                pad_right += diff
                padded_width += 2 * diff
        if padded_height < cropped_height or padded_width < cropped_width:
            raise ValueError(f"Required crop size {(cropped_height, cropped_width)} is larger than "
                             f"{'padded ' if self.padding is not None else ''}input image size {(padded_height, padded_width)}.")
        padding = [pad_left, pad_top, pad_right, pad_bottom]  # F.pad's order
        needs_pad = any(padding)
        needs_vert_crop, top = ((True, int(torch.randint(0, padded_height - cropped_height + 1, size=())))
                                if padded_height > cropped_height else (False, 0))
        needs_horz_crop, left = ((True, int(torch.randint(0, padded_width - cropped_width + 1, size=())))
                                 if padded_width > cropped_width else (False, 0))
        return dict(needs_crop=needs_vert_crop or needs_horz_crop, top=top, left=left, height=cropped_height,
                    width=cropped_width, needs_pad=needs_pad, padding=padding)

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        box = dict(top=params["top"], left=params["left"], height=params["height"], width=params["width"])
        if params["needs_pad"]:
            fill = _get_fill(self._fill, type(inpt))
            if params["needs_crop"]:
                return self._call_kernel(F.pad_crop, inpt, padding=params["padding"], fill=fill, padding_mode=self.padding_mode,
                                         **box)
            return self._call_kernel(F.pad, inpt, padding=params["padding"], fill=fill, padding_mode=self.padding_mode)
        if params["needs_crop"]:
            return self._call_kernel(F.crop, inpt, **box)
        return inpt


def _check_scale_ratio(scale, ratio) -> None:
    import warnings
    if not isinstance(scale, Sequence):
        raise TypeError("Scale should be a sequence")
    if not isinstance(ratio, Sequence):
        raise TypeError("Ratio should be a sequence")
    if (scale[0] > scale[1]) or (ratio[0] > ratio[1]):
        warnings.warn("Scale and ratio should be of kind (min, max)")


class RandomResizedCrop(Transform):
    """v2.RandomResizedCrop(size, scale=(0.08, 1.0), ratio=(3/4, 4/3), interpolation=BILINEAR, antialias=True) --
    transforms/v2/_geometry.py; the crop and the resize are one launch (F.resized_crop)."""

    def __init__(self, size, scale: Tuple[float, float] = (0.08, 1.0), ratio: Tuple[float, float] = (3.0 / 4.0, 4.0 / 3.0),
                 interpolation=InterpolationMode.BILINEAR, antialias: Optional[bool] = True) -> None:
        super().__init__()
        self.size = _setup_size(size, "Please provide only two dimensions (h, w) for size.")
        _check_scale_ratio(scale, ratio)
        self.scale = scale
        self.ratio = ratio
        self.interpolation = interpolation
        self.antialias = antialias
        self._log_ratio = torch.log(torch.tensor(self.ratio))

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        height, width = query_size(flat_inputs)
        area = height * width
        log_ratio = self._log_ratio
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(self.scale[0], self.scale[1]).item()
            aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if 0 < w <= width and 0 < h <= height:
                i = torch.randint(0, height - h + 1, size=(1,)).item()
                j = torch.randint(0, width - w + 1, size=(1,)).item()
                break
        else:  # the central crop
            in_ratio = float(width) / float(height)
            if in_ratio < min(self.ratio):
                w = width
                h = int(round(w / min(self.ratio)))
            elif in_ratio > max(self.ratio):
                h = height
                w = int(round(h * max(self.ratio)))
            else:
                w = width
                h = height
            i = (height - h) // 2
            j = (width - w) // 2
        return dict(top=i, left=j, height=h, width=w)

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        return self._call_kernel(F.resized_crop, inpt, **params, size=list(self.size), interpolation=self.interpolation,
                                 antialias=self.antialias)


class RandomErasing(_RandomApplyTransform):
    """v2.RandomErasing(p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0.0, inplace=False) -- transforms/v2/_augment.py.
    The "random" values are drawn on the host, as the reference draws them, and copied to the device."""

    def __init__(self, p: float = 0.5, scale: Tuple[float, float] = (0.02, 0.33), ratio: Tuple[float, float] = (0.3, 3.3),
                 value=0.0, inplace: bool = False) -> None:
        super().__init__(p=p)
        if not isinstance(value, (numbers.Number, str, tuple, list)):
            raise TypeError("Argument value should be either a number or str or a sequence")
        if isinstance(value, str) and value != "random":
            raise ValueError("If value is str, it should be 'random'")
        _check_scale_ratio(scale, ratio)
        if scale[0] < 0 or scale[1] > 1:
            raise ValueError("Scale should be between 0 and 1")
        self.scale = scale
        self.ratio = ratio
        if isinstance(value, (int, float)):
            self.value = [float(value)]
        elif isinstance(value, str):
            self.value = None
        elif isinstance(value, (list, tuple)):
            self.value = [float(v) for v in value]
        else:
            self.value = value
        self.inplace = inplace
        self._log_ratio = torch.log(torch.tensor(self.ratio))

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        img_c, img_h, img_w = query_chw(flat_inputs)
        if self.value is not None and not (len(self.value) in (1, img_c)):
            raise ValueError(f"If value is a sequence, it should have either a single value or {img_c} (number of inpt channels)")
        area = img_h * img_w
        log_ratio = self._log_ratio
        for _ in range(10):
            erase_area = area * torch.empty(1).uniform_(self.scale[0], self.scale[1]).item()
            aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
            h = int(round(math.sqrt(erase_area * aspect_ratio)))
            w = int(round(math.sqrt(erase_area / aspect_ratio)))
            if not (h < img_h and w < img_w):
                continue
            if self.value is None:
                v = torch.empty([img_c, h, w], dtype=torch.float32).normal_()
            else:
                v = torch.tensor(self.value)[:, None, None]
            i = torch.randint(0, img_h - h + 1, size=(1,)).item()
            j = torch.randint(0, img_w - w + 1, size=(1,)).item()
            break
        else:
            i, j, h, w, v = 0, 0, img_h, img_w, None
        return dict(i=i, j=j, h=h, w=w, v=v)

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        if params["v"] is not None:
            inpt = self._call_kernel(F.erase, inpt, **params, inplace=self.inplace)
        return inpt


def _find_labels_default_heuristic(inputs: Any) -> torch.Tensor:
    """transforms/v2/_utils.py `_find_labels_default_heuristic`: the second item of a tuple or list sample, itself the labels
    or a dict that holds them under "label" / "labels" (any letter case)."""
    if isinstance(inputs, (tuple, list)):
        inputs = inputs[1]
    if is_pure_tensor(inputs):
        return inputs
    if not isinstance(inputs, collections.abc.Mapping):
        raise ValueError("When using the default labels_getter, the input passed to forward must be a dictionary or a two-tuple "
                         f"whose second item is a dictionary or a tensor, but got {inputs} instead.")
    candidate_key = next((key for key in inputs.keys() if key.lower() in ("label", "labels")), None)
    if candidate_key is None:
        raise ValueError("Could not infer where the labels are in the sample. Try passing a callable as the labels_getter "
                         "parameter? If there are no labels in the sample by design, pass labels_getter=None.")
    return inputs[candidate_key]


def _parse_labels_getter(labels_getter: Union[str, Callable[[Any], Any], None]) -> Callable[[Any], Any]:
    """transforms/v2/_utils.py `_parse_labels_getter`."""
    if labels_getter == "default":
        return _find_labels_default_heuristic
    if callable(labels_getter):
        return labels_getter
    if labels_getter is None:
        return lambda _: None
    raise ValueError(f"labels_getter should either be 'default', a callable, or None, but got {labels_getter}.")


class _BaseMixUpCutMix(Transform):
    """transforms/v2/_augment.py `_BaseMixUpCutMix`: a batch-level transform of (images, labels) after collation.  Sample b is
    mixed with sample b - 1; the labels become (B, num_classes) float probabilities."""

    def __init__(self, *, alpha: float = 1.0, num_classes: Optional[int] = None, labels_getter="default") -> None:
        super().__init__()
        self.alpha = float(alpha)
        self._dist = torch.distributions.Beta(torch.tensor([alpha]), torch.tensor([alpha]))
        self.num_classes = num_classes
        self._labels_getter = _parse_labels_getter(labels_getter)

    def forward(self, *inputs: Any) -> Any:
        inputs = inputs if len(inputs) > 1 else inputs[0]
        flat_inputs, spec = tree_flatten(inputs)
        needs = self._needs_transform_list(flat_inputs)
        if any(isinstance(i, _PIL_TYPES + (tv_tensors.BoundingBoxes, tv_tensors.Mask)) for i in flat_inputs):
            raise ValueError(f"{type(self).__name__}() does not support PIL images, bounding boxes and masks.")
        labels = self._labels_getter(inputs)
        if not isinstance(labels, torch.Tensor):
            raise ValueError(f"The labels must be a tensor, but got {type(labels)} instead.")
        if labels.ndim not in (1, 2):
            raise ValueError("labels should be index based with shape (batch_size,) or probability based with shape (batch_size, "
                             f"num_classes), but got a tensor of shape {labels.shape} instead.")
        if labels.ndim == 2 and self.num_classes is not None and labels.shape[-1] != self.num_classes:
            raise ValueError("When passing 2D labels, the number of elements in last dimension must match num_classes: "
                             f"{labels.shape[-1]} != {self.num_classes}. You can Leave num_classes to None.")
        if labels.ndim == 1 and self.num_classes is None:
            raise ValueError("num_classes must be passed if the labels are index-based (1D)")
        params = {"labels": labels, "batch_size": labels.shape[0],
                  **self._get_params([i for i, n in zip(flat_inputs, needs) if n])}
        # the labels are transformed by identity, not by the pure-tensor heuristic; _get_params above does not see them
        needs[next(k for k, i in enumerate(flat_inputs) if i is labels)] = True
        flat_outputs = [self._transform(i, params) if n else i for i, n in zip(flat_inputs, needs)]
        return tree_unflatten(flat_outputs, spec)

    def _check_image_or_video(self, inpt: torch.Tensor, *, batch_size: int) -> None:
        expected_num_dims = 5 if isinstance(inpt, tv_tensors.Video) else 4
        if inpt.ndim != expected_num_dims:
            raise ValueError(f"Expected a batched input with {expected_num_dims} dims, but got {inpt.ndim} dimensions instead.")
        if inpt.shape[0] != batch_size:
            raise ValueError("The batch size of the image or video does not match the batch size of the labels: "
                             f"{inpt.shape[0]} != {batch_size}.")

    def _mixup_label(self, label: torch.Tensor, *, lam: float) -> torch.Tensor:
        return F.mixup_labels(label.as_subclass(torch.Tensor), lam, num_classes=self.num_classes)

    def _mix(self, image: torch.Tensor, params: Dict[str, Any]) -> torch.Tensor:
        raise NotImplementedError

    def _transform(self, inpt: Any, params: Dict[str, Any]) -> Any:
        if inpt is params["labels"]:
            return self._mixup_label(inpt, lam=params["lam"])
        if isinstance(inpt, (tv_tensors.Image, tv_tensors.Video)) or is_pure_tensor(inpt):
            self._check_image_or_video(inpt, batch_size=params["batch_size"])
            output = self._mix(inpt.as_subclass(torch.Tensor), params)
            if isinstance(inpt, (tv_tensors.Image, tv_tensors.Video)):
                output = tv_tensors.wrap(output, like=inpt)
            return output
        return inpt


class MixUp(_BaseMixUpCutMix):
    """v2.MixUp(*, alpha=1.0, num_classes=None, labels_getter="default") -- transforms/v2/_augment.py: images and labels become
    lam * x[b] + (1 - lam) * x[b - 1] with lam ~ Beta(alpha, alpha) drawn on the host; one launch for the images that reads the
    batch once, one for the labels.  Integer images raise TypeError (the reference's mul_ raises): convert with ToDtype first."""

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        return dict(lam=float(self._dist.sample(())))

    def _mix(self, image: torch.Tensor, params: Dict[str, Any]) -> torch.Tensor:
        return F.mixup_image(image, params["lam"])


class CutMix(_BaseMixUpCutMix):
    """v2.CutMix(*, alpha=1.0, num_classes=None, labels_getter="default") -- transforms/v2/_augment.py: a box of every image is
    replaced by the same box of the previous image of the batch, and the labels are mixed by the share of the area that is left.
    The box is drawn on the host with the reference's calls in the reference's order."""

    def _get_params(self, flat_inputs: List[Any]) -> Dict[str, Any]:
        lam = float(self._dist.sample(()))
        H, W = query_size(flat_inputs)
        r_x = torch.randint(W, size=(1,))
        r_y = torch.randint(H, size=(1,))
        r = 0.5 * math.sqrt(1.0 - lam)
        r_w_half = int(r * W)
        r_h_half = int(r * H)
        x1 = int(torch.clamp(r_x - r_w_half, min=0))
        y1 = int(torch.clamp(r_y - r_h_half, min=0))
        x2 = int(torch.clamp(r_x + r_w_half, max=W))
        y2 = int(torch.clamp(r_y + r_h_half, max=H))
        box = (x1, y1, x2, y2)
        lam_adjusted = float(1.0 - (x2 - x1) * (y2 - y1) / (W * H))
        return dict(box=box, lam=lam_adjusted)

    def _mix(self, image: torch.Tensor, params: Dict[str, Any]) -> torch.Tensor:
        return F.cutmix_image(image, params["box"])


def _thread_through(transforms, order, inputs: Tuple[Any, ...]) -> Any:
    """Compose.forward's loop over transforms[k] for k in `order`: multi-argument outputs are fed back as *inputs.  An empty
    `order` hands the inputs back, where the reference's loop leaves `outputs` unbound and raises UnboundLocalError."""
    needs_unpacking = len(inputs) > 1
    outputs = inputs if needs_unpacking else inputs[0]
    for k in order:
        outputs = transforms[k](*inputs)
        inputs = outputs if needs_unpacking else (outputs,)
    return outputs


class RandomApply(Transform):
    """v2.RandomApply(transforms, p=0.5) -- transforms/v2/_container.py: all of `transforms` in turn, or none of them."""

    def __init__(self, transforms: Union[Sequence[Callable], nn.ModuleList], p: float = 0.5) -> None:
        super().__init__()
        if not isinstance(transforms, (Sequence, nn.ModuleList)):
            raise TypeError("Argument transforms should be a sequence of callables or a `nn.ModuleList`")
        self.transforms = transforms
        if not (0.0 <= p <= 1.0):
            raise ValueError("`p` should be a floating point value in the interval [0.0, 1.0].")
        self.p = p

    def forward(self, *inputs: Any) -> Any:
        if torch.rand(1) >= self.p:
            return inputs if len(inputs) > 1 else inputs[0]
        return _thread_through(self.transforms, range(len(self.transforms)), inputs)

    def extra_repr(self) -> str:
        return "\n".join(f"    {t}" for t in self.transforms)


class RandomChoice(Transform):
    """v2.RandomChoice(transforms, p=None) -- transforms/v2/_container.py: one of `transforms`, drawn with torch.multinomial
    from the weights `p` (default: equal), which are stored normalised."""

    def __init__(self, transforms: Sequence[Callable], p: Optional[List[float]] = None) -> None:
        if not isinstance(transforms, Sequence):
            raise TypeError("Argument transforms should be a sequence of callables")
        if p is None:
            p = [1] * len(transforms)
        elif len(p) != len(transforms):
            raise ValueError(f"Length of p doesn't match the number of transforms: {len(p)} != {len(transforms)}")
        super().__init__()
        self.transforms = transforms
        total = sum(p)
        self.p = [prob / total for prob in p]

    def forward(self, *inputs: Any) -> Any:
        idx = int(torch.multinomial(torch.tensor(self.p), 1))
        return self.transforms[idx](*inputs)


class RandomOrder(Transform):
    """v2.RandomOrder(transforms) -- transforms/v2/_container.py: all of `transforms`, in the order of one torch.randperm."""

    def __init__(self, transforms: Sequence[Callable]) -> None:
        if not isinstance(transforms, Sequence):
            raise TypeError("Argument transforms should be a sequence of callables")
        super().__init__()
        self.transforms = transforms

    def forward(self, *inputs: Any) -> Any:
        return _thread_through(self.transforms, [int(k) for k in torch.randperm(len(self.transforms))], inputs)


class GaussianBlurV1(nn.Module):
    """transforms.GaussianBlur (v1) -- transforms/transforms.py:1753-1812."""

    def __init__(self, kernel_size, sigma=(0.1, 2.0)):
        super().__init__()
        self.kernel_size = _setup_size(kernel_size, "Kernel size should be a tuple/list of two integers")
        for ks in self.kernel_size:
            if ks <= 0 or ks % 2 == 0:
                raise ValueError("Kernel size value should be an odd and positive number.")
        if isinstance(sigma, numbers.Number):
            if sigma <= 0:
                raise ValueError("If sigma is a single number, it must be positive.")
            sigma = (sigma, sigma)
        elif isinstance(sigma, Sequence) and len(sigma) == 2:
            if not 0.0 < sigma[0] <= sigma[1]:
                raise ValueError("sigma values should be positive and of the form (min, max).")
        else:
            raise ValueError("sigma should be a single number or a list/tuple with length 2.")
        self.sigma = sigma

    @staticmethod
    def get_params(sigma_min: float, sigma_max: float) -> float:
        return torch.empty(1).uniform_(sigma_min, sigma_max).item()

    def forward(self, img: torch.Tensor) -> torch.Tensor:
        sigma = self.get_params(self.sigma[0], self.sigma[1])
        return F1.gaussian_blur(img, list(self.kernel_size), [sigma, sigma])

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(kernel_size={self.kernel_size}, sigma={self.sigma})"
