"""Capture cases (data only, nothing here touches a device): small calls of the public `functional` / `ops` wrappers that
tests/test_gpu_capture.py runs inside a HIP graph and tests/test_capture_cases_host.py runs on CPU tensors with the launches recorded.

Two tables.  cases(): one call per form of every wrapper that can be captured.  For the layer, RoI, paste and keypoint families it
is a call on the tensors of a tests/_fuzz_cases.py case: per family and per form of the call (FORMS: the part of the geometry that
selects another kernel, entry point or epilogue) the smallest case whose tensors total at most MAX_BYTES and whose CPU reference
depends on its data.  For the wrappers those sweeps do not run -- the image filters in every storage type and as lists of frames, the
colour, crop, mix, warp and resize ops, the remaining layers, the detectors' top-k, score and decode entries chained as the detectors
chain them -- it is a case written by hand (HAND).  inputs(case, second=False / True) are a case's tensors from two data seeds; every
array changes with the seed -- weights, biases, norm terms, boxes, labels, gates, cell anchors and image sizes, not only x.
NOT_CAPTURABLE: {entry point: reason} for the wrappers that read a result back.  NO_WRAPPER: the one entry point no
wrapper calls.  The names the cases call and the two tables together are every stream-taking entry point of include/mi355vision.h: the
census of the host test and of the GPU test (captured_entry_points)."""
import contextlib
import dataclasses
import re
from pathlib import Path

import numpy as np
import torch

from cpu_vision_amd import functional as F
from cpu_vision_amd import ops
from tests import _fuzz_cases as FC
from tests._util import philox_f32

MAX_BYTES = 1 << 20
SEED_STEP = 7  # the second data seed of a case
HEADER = Path(__file__).resolve().parent.parent / "include" / "mi355vision.h"


def stream_entry_points():
    """Every mv_* function of include/mi355vision.h whose declaration ends in the stream parameter."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return {m.group(1) for m in re.finditer(r"\b(mv_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
            if re.search(r"\bstream\s*$", m.group(2).split(",")[-1].strip())}


class Recorder:
    """Stands in for the loaded library (swapped in as _lib.tuning_library swaps it): a stream-taking entry point is noted when it
    is CALLED -- fetching the attribute alone records nothing -- and then runs (launch=True) or reports success without running; the
    rest (host queries of workspace sizes and K slices, mv_last_kernel) is the library's."""

    def __init__(self, real, launch=False):
        self._real, self._launch, self._stream, self.names = real, launch, stream_entry_points(), []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._stream:
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args) if self._launch else 0
        return call


def captured_entry_points():
    """The entry points the cases have to call between them: every stream-taking one but those of the two tables below."""
    return stream_entry_points() - set(NOT_CAPTURABLE) - set(NO_WRAPPER)


# ---- the calls ------------------------------------------------------------------------------------------------------------------------
def _epilogue(t):
    return t["bias"], t["alpha"], t["beta"]


@contextlib.contextmanager
def _switch(name, value):
    old = getattr(F, name)
    setattr(F, name, value)
    try:
        yield
    finally:
        setattr(F, name, old)


def _conv2d(g, t):
    with _switch("CONV2D_SMALL_LAUNCH_WORKSPACE", g["columns"]):
        return F.conv2d_affine_act(t["x"], t["w"], *_epilogue(t), t["res"], stride=g["stride"], padding=g["padding"], dilation=g["dilation"],
                                   groups=g["groups"], affine=g["affine"], activation=g["act"])


def _roi(g, t):
    out = (g["ph"], g["pw"])
    if g["op"] == "roi_align":
        return ops.roi_align(t["x"], t["rois"], out, g["scale"], g["ratio"], g["aligned"])
    if g["op"] == "ps_roi_align":
        return ops.ps_roi_align(t["x"], t["rois"], out, g["scale"], g["ratio"])
    return getattr(ops, g["op"])(t["x"], t["rois"], out, g["scale"])


CALLS = {
    "dw5x5": lambda g, t: F.conv_norm_act(t["x"], t["w"], *_epilogue(t), t["res"], stride=g["stride"], groups=g["c"], affine=g["affine"],
                                          activation=g["act"], dilation=g["dilation"]),
    "pw_scaled": lambda g, t: F.conv_norm_act(t["x"], t["w"], *_epilogue(t), t["res"], affine=g["affine"], activation=g["act"],
                                              input_scale=t["gate"]),
    "se": lambda g, t: (F.global_avg_pool(t["x"]), F.se_scale(t["x"], t["gate"]), F.linear_act(t["xl"], t["wl"], t["bl"], g["act"]),
                        F.squeeze_excitation_gate(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], g["gate_act"], g["scale_act"])),
    "conv2d": _conv2d,
    "maxpool": lambda g, t: F.max_pool2d(t["x"], g["k"], g["stride"], g["padding"], ceil_mode=g["ceil_mode"]),
    "convt": lambda g, t: F.conv_transpose2d_bias_act(t["x"], t["w"], t["bias"], g["act"], padding=0 if g["k"] == 2 else 1),
    "groupnorm": lambda g, t: F.group_norm_act(t["x"], g["groups"], t["weight"], t["bias"], g["eps"], relu=g["relu"]),
    "l2norm": lambda g, t: F.l2_normalize_scale(t["x"], t["weight"], g["eps"]),
    "lateral": lambda g, t: F.conv1x1_upsample_add(t["x"], t["w"], *_epilogue(t), t["top"], affine=g["affine"], activation=g["act"]),
    "interp": lambda g, t: F.interpolate(t["x"], size=(g["oh"], g["ow"])),
    "argmax": lambda g, t: tuple(F.interpolate_argmax(t["x"], size=(g["oh"], g["ow"]), dtype=d) for d in (torch.int64, torch.uint8)),
    "gated_up": lambda g, t: F.conv1x1_gated_upsample(t["x"], t["gate"], t["w"], t["bias"], t["res"], size=(g["oh"], g["ow"])),
    "roi": _roi,
    "paste": lambda g, t: F.paste_masks_in_image(t["masks"], t["boxes"], (g["h"], g["w"]), g["padding"]),
    "keypoints": lambda g, t: F.heatmaps_to_keypoints(t["maps"], t["rois"]),
}

# family: the part of a case's geometry that selects another kernel, entry point or epilogue form
FORMS = {
    "dw5x5": lambda g: (g["stride"], g["dilation"]),
    "pw_scaled": lambda g: (F.conv1x1_k_slices(g["n"], g["cin"], g["h"], g["w"], g["cout"])[0] > 1, g["res"]),
    "se": lambda g: (g["h"] * g["w"] % 4 == 0,),
    "conv2d": lambda g: (g["columns"], g["groups"] > 1, g["dilation"] > 1, (g["kh"], g["kw"]) == (1, 1)),
    "maxpool": lambda g: (g["ceil_mode"], g["padding"] > 0, (g["k"], g["stride"]) == (2, 2)),
    "convt": lambda g: (g["k"], g["w"] % 2 == 0),
    "groupnorm": lambda g: (g["relu"], g["h"] * g["w"] % 4 == 0),
    "l2norm": lambda g: (),
    "lateral": lambda g: (g["affine"], g["bias"]),
    "interp": lambda g: (g["ow"] % 4 == 0,),
    "argmax": lambda g: (g["ow"] % 4 == 0,),
    "gated_up": lambda g: (F.conv1x1_k_slices(g["n"], g["cin"], g["oh"], g["ow"], g["cout"])[0] > 1,),
    "roi": lambda g: (g["op"], g.get("aligned"), g.get("ratio", 0) > 0),
    "paste": lambda g: (g["w"] % 4 == 0,),
    "keypoints": lambda g: (),
}


# ---- cases written by hand: the wrappers the sweeps of tests/_fuzz_cases.py do not run ------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Hand:
    """A case with no generator behind it: make(seed) -> its inputs, fn(tensors) -> its call.  No CPU reference is computed for
    these (the families' own tests do that); the host test asserts that the two seeds' inputs differ, the GPU test that the two
    eager results do."""
    id: str
    seed: int
    make: object
    fn: object
    family: str = "hand"


F32 = np.float32
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
_IMG = (2, 3, 40, 56)


def _f(seed, shape, lo=-1.0, hi=1.0):
    return (philox_f32(seed, shape) * F32(hi - lo) + F32(lo)).astype(F32)


def _u8(seed, shape):
    return np.random.Generator(np.random.Philox(seed)).integers(0, 256, shape, dtype=np.uint8)


def _boxes(seed, n, size=40.0):
    a = _f(seed, (n, 4), 0.0, size)
    return np.concatenate([np.minimum(a[:, :2], a[:, 2:]), np.maximum(a[:, :2], a[:, 2:]) + 1], 1).astype(F32)


def _epi(s, c):
    return dict(bias=_f(s + 2, (c,)), alpha=_f(s + 3, (c,), 0.5, 1.5), beta=_f(s + 4, (c,)))


# a pyramid of two levels, (5, 7) at stride 8 and (3, 4) at stride 16, for two images
_GRIDS, _STRIDES = ((5, 7), (3, 4)), [(8, 8), (16, 16)]


def _cells(seed, anchors):
    """(anchors, 4) cell anchors per level, their size a little different from seed to seed."""
    base = np.array([[-4.0, -4, 4, 4], [-8, -4, 8, 4], [-4, -8, 4, 8]], F32)[:anchors]
    return [(base * F32(k * (1 + (seed % 5) / 8))).astype(F32) for k in (1, 2)]


_SIZE_LIST = [(40, 56), (37, 50)]  # image sizes as the detector classes pass them


def _host_cells(anchors):
    return [torch.from_numpy(c) for c in _cells(0, anchors)]


def _ssd_pairs():
    from cpu_vision_amd.anchor_utils import DefaultBoxGenerator
    return DefaultBoxGenerator([[2], [2, 3]])._wh_pairs


def _sizes(seed):
    """(2, 2) image sizes (h, w), different from seed to seed (SEED_STEP is no multiple of 5)."""
    return (np.array([[40, 56], [37, 50]], F32) + F32(seed % 5)).astype(F32)


def _levels(seed, channels, lo, hi):
    return [_f(seed + i, (2, channels, h, w), lo, hi) for i, (h, w) in enumerate(_GRIDS)]


def _preset():
    from cpu_vision_amd.presets import ImageClassification
    return ImageClassification(crop_size=16, resize_size=20)


def _frames(seed, dtype):
    """Three separately allocated frames."""
    return [_u8(seed + i, (3, 24, 32)) if dtype is np.uint8 else _f(seed + i, (3, 24, 32), 0.0, 1.0) for i in range(3)]


def _pair_blur(blur, x):
    """A uint8 blur as the float32 separable pair: the switch that leaves the reference's exact integers."""
    with _switch("INTEGER_BLUR_EXACT_2D", False):
        return blur(x, [9, 9], [1.7, 1.7])


HAND = {
    "conv_norm_act[stem 3x3 s2]": (lambda s: dict(x=_f(s, (2, 3, 9, 11)), w=_f(s + 1, (8, 3, 3, 3), -0.4, 0.4), **_epi(s, 8)),
                                   lambda t: F.conv_norm_act(t["x"], t["w"], t["bias"], t["alpha"], t["beta"], None, stride=2, affine="fma",
                                                             activation="relu6")),
    "conv_norm_act[depthwise 3x3]": (lambda s: dict(x=_f(s, (2, 6, 9, 11)), w=_f(s + 1, (6, 1, 3, 3), -0.4, 0.4), **_epi(s, 6)),
                                     lambda t: F.conv_norm_act(t["x"], t["w"], t["bias"], t["alpha"], t["beta"], None, groups=6, affine="mul_add",
                                                               activation="hardswish")),
    "conv_norm_act[pointwise + residual]": (lambda s: dict(x=_f(s, (2, 5, 7, 9)), w=_f(s + 1, (9, 5, 1, 1)), res=_f(s + 5, (2, 9, 7, 9)), **_epi(s, 9)),
                                            lambda t: F.conv_norm_act(t["x"], t["w"], t["bias"], t["alpha"], t["beta"], t["res"], affine="fma")),
    "linear_bias_relu": (lambda s: dict(x=_f(s, (3, 20)), w=_f(s + 1, (7, 20)), b=_f(s + 2, (7,))),
                         lambda t: F.linear_bias_relu(t["x"], t["w"], t["b"], relu=True)),
    "linear_bias_relu[sliced K]": (lambda s: dict(x=_f(s, (1, 4096)), w=_f(s + 1, (24, 4096), -0.05, 0.05), b=_f(s + 2, (24,))),
                                   lambda t: F.linear_bias_relu(t["x"], t["w"], t["b"], relu=False)),
    "adaptive_avg_pool2d": (lambda s: dict(x=_f(s, (2, 5, 9, 7))), lambda t: F.adaptive_avg_pool2d(t["x"], (1, 1))),
    "conv2d_bias_relu[cin 3]": (lambda s: dict(x=_f(s, (2, 3, 10, 12)), w=_f(s + 1, (16, 3, 3, 3), -0.3, 0.3), b=_f(s + 2, (16,))),
                                lambda t: F.conv2d_bias_relu(t["x"], t["w"], t["b"])),
    "conv2d_bias_relu[K chunks]": (lambda s: dict(x=_f(s, (1, 16, 14, 14)), w=_f(s + 1, (32, 16, 3, 3), -0.2, 0.2)),
                                   lambda t: F.conv2d_bias_relu(t["x"], t["w"], None)),
    "conv2d_bias_act[5x5 s2]": (lambda s: dict(x=_f(s, (2, 3, 11, 13)), w=_f(s + 1, (8, 3, 5, 5), -0.2, 0.2), b=_f(s + 2, (8,))),
                                lambda t: F.conv2d_bias_act(t["x"], t["w"], t["b"], stride=2, padding=2, activation="relu")),
    "dwconv_pointwise": (lambda s: dict(x=_f(s, (2, 35, 7, 6)), wdw=_f(s + 1, (35, 1, 3, 3)), a=_f(s + 2, (35,), 0.5, 1.5), b=_f(s + 3, (35,)),
                                        wpw=_f(s + 4, (9, 35, 1, 1)), bpw=_f(s + 5, (9,))),
                         lambda t: F.dwconv_pointwise(t["x"], t["wdw"], None, t["a"], t["b"], t["wpw"], t["bpw"], stride=2, dw_affine="fma",
                                                      dw_activation="relu6")),
    "dwconv7x7": (lambda s: dict(x=_f(s, (2, 8, 9, 11)), w=_f(s + 1, (8, 1, 7, 7), -0.2, 0.2), b=_f(s + 2, (8,))),
                  lambda t: F.dwconv7x7(t["x"], t["w"], t["b"])),
    "layer_norm2d": (lambda s: dict(x=_f(s, (2, 8, 5, 7)), w=_f(s + 1, (8,), 0.5, 1.5), b=_f(s + 2, (8,))),
                     lambda t: F.layer_norm2d(t["x"], t["w"], t["b"])),
    "conv1x1_gelu[norm in the loads]": (lambda s: dict(x=_f(s, (2, 8, 5, 7)), nw=_f(s + 1, (8,), 0.5, 1.5), nb=_f(s + 2, (8,)),
                                                       w=_f(s + 3, (32, 8)), b=_f(s + 4, (32,))),
                                        lambda t: F.conv1x1_gelu(t["x"], t["w"], t["b"], norm=(*F.layer_norm2d_stats(t["x"]), t["nw"], t["nb"]))),
    "sobel": (lambda s: dict(x=_f(s, (2, 3, 16, 20))), lambda t: F.sobel(t["x"])),
    "gaussian_sobel": (lambda s: dict(x=_f(s, (2, 3, 16, 20))), lambda t: F.gaussian_sobel(t["x"], [5, 5], [1.1, 1.1])),
    "gaussian_blur[f32 3x3]": (lambda s: dict(x=_f(s, _IMG)), lambda t: F.gaussian_blur(t["x"], [3, 3])),
    "gaussian_blur[f32 5x5]": (lambda s: dict(x=_f(s, _IMG)), lambda t: F.gaussian_blur(t["x"], [5, 5], [1.1, 1.1])),
    "gaussian_blur[u8 3x3]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.gaussian_blur(t["x"], [3, 3])),
    "gaussian_blur[u8 9x9]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.gaussian_blur(t["x"], [9, 9], [1.7, 1.7])),
    "separable_gaussian_blur": (lambda s: dict(x=_f(s, _IMG)), lambda t: F.separable_gaussian_blur(t["x"], [5, 5], [1.1, 1.1])),
    "box_filter[f32]": (lambda s: dict(x=_f(s, _IMG)), lambda t: F.box_filter(t["x"], 3)),
    "box_filter[u8]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.box_filter(t["x"], 3)),
    "adjust_sharpness[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)), lambda t: F.adjust_sharpness(t["x"], 1.5)),
    "adjust_sharpness[u8]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.adjust_sharpness(t["x"], 0.5)),
    "to_float_normalize": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.to_float_normalize(t["x"], MEAN, STD)),
    "normalize": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)), lambda t: F.normalize(t["x"], MEAN, STD)),
    "resize[u8]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.resize(t["x"], [24])),
    "resize[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)), lambda t: F.resize(t["x"], [24])),
    "pad": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.pad(t["x"], [3, 5], fill=[1, 2, 3])),
    "horizontal_flip": (lambda s: dict(x=_f(s, _IMG)), lambda t: F.horizontal_flip(t["x"])),
    "erase": (lambda s: dict(x=_u8(s, _IMG), v=_u8(s + 1, (3, 1, 1))), lambda t: F.erase(t["x"], 5, 7, 20, 30, t["v"])),
    "resized_crop[u8]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.resized_crop(t["x"], 2, -3, 30, 40, [16, 16])),
    "resized_crop[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)), lambda t: F.resized_crop(t["x"], 2, 3, 30, 40, [16, 16])),
    "resized_crop_flip_normalize[u8]": (lambda s: dict(x=_u8(s, _IMG)),
                                        lambda t: F.resized_crop_flip_normalize(t["x"], 2, 3, 30, 40, [16, 16], True, MEAN, STD)),
    "color_jitter[u8]": (lambda s: dict(x=_u8(s, _IMG)),
                         lambda t: F.color_jitter_image(t["x"], [("brightness", 1.2), ("contrast", 0.8), ("saturation", 1.3), ("hue", 0.1)])),
    "color_jitter[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)),
                          lambda t: F.color_jitter_image(t["x"], [("brightness", 1.2), ("saturation", 1.3), ("hue", -0.2)])),
    "rgb_to_grayscale[u8]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.rgb_to_grayscale(t["x"], 3)),
    "rgb_to_grayscale[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)), lambda t: F.rgb_to_grayscale(t["x"])),
    "solarize[u8]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.solarize(t["x"], 100)),
    "invert[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)), lambda t: F.invert(t["x"])),
    "autocontrast[u8]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.autocontrast(t["x"])),
    "autocontrast[f32]": (lambda s: dict(x=_f(s, _IMG, 0.1, 0.9)), lambda t: F.autocontrast(t["x"])),
    "equalize[u8]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.equalize(t["x"])),
    "mixup_image[f32]": (lambda s: dict(x=_f(s, (4, 3, 8, 10))), lambda t: F.mixup_image(t["x"], 0.3)),
    "cutmix_image": (lambda s: dict(x=_u8(s, (4, 3, 8, 10))), lambda t: F.cutmix_image(t["x"], (2, 1, 7, 6))),
    "mixup_labels": (lambda s: dict(y=np.random.Generator(np.random.Philox(s)).permutation(8)[:4].astype(np.int64)),
                     lambda t: F.mixup_labels(t["y"], 0.3, 8)),
    "mask_probs": (lambda s: dict(x=_f(s, (3, 4, 7, 7), -3, 3), labels=((np.arange(3) + s) % 4).astype(np.int64)),
                   lambda t: F.mask_probs(t["x"], t["labels"])),
    "box_iou": (lambda s: dict(a=_boxes(s, 5), b=_boxes(s + 1, 7)), lambda t: ops.box_iou(t["a"], t["b"])),
    "box_decode": (lambda s: dict(boxes=_boxes(s, 6), codes=_f(s + 1, (6, 8))), lambda t: F.box_decode(t["boxes"], t["codes"], (10.0, 10.0, 5.0, 5.0))),
    "rpn_topk": (lambda s: dict(maps=[_f(s, (2, 3, 5, 7), -4, 4), _f(s + 1, (2, 3, 3, 4), -4, 4)]), lambda t: F.rpn_topk(t["maps"], 5)),
    "retinanet_topk": (lambda s: dict(maps=[_f(s, (2, 6, 5, 7), -4, 4), _f(s + 1, (2, 6, 3, 4), -4, 4)]),
                       lambda t: F.retinanet_topk(t["maps"], 3, 5, 0.05)),
    "fcos_topk": (lambda s: dict(maps=[_f(s, (2, 3, 5, 7), -4, 4), _f(s + 1, (2, 3, 3, 4), -4, 4)],
                                 ctrs=[_f(s + 2, (2, 1, 5, 7), -4, 4), _f(s + 3, (2, 1, 3, 4), -4, 4)]),
                  lambda t: F.fcos_topk(t["maps"], t["ctrs"], 3, 5, 0.05)),
    "ssd_scores + ssd_topk": (lambda s: dict(maps=[_f(s, (2, 20, 5, 4), -2, 2), _f(s + 1, (2, 30, 3, 3), -2, 2)]),
                              lambda t: (lambda sc: (sc, F.ssd_topk(sc, 9, 0.05)))(F.ssd_scores(t["maps"], 5))),
    # top-k and decode as the detectors chain them: the decode reads the indices the top-k has just written
    # the cell anchors, SSD's (w, h) pairs and the image sizes as device tensors, inputs like the maps ...
    "rpn_topk + rpn_decode": (lambda s: dict(maps=_levels(s, 3, -4, 4), deltas=_levels(s + 2, 12, -0.5, 0.5), cells=_cells(s, 3), sizes=_sizes(s)),
                              lambda t: F.rpn_decode(t["maps"], t["deltas"], F.rpn_topk(t["maps"], 5), t["cells"], _STRIDES, t["sizes"])),
    "retinanet_topk + retinanet_decode": (lambda s: dict(maps=_levels(s, 6, -4, 4), deltas=_levels(s + 2, 8, -0.5, 0.5), cells=_cells(s, 2),
                                                         sizes=_sizes(s)),
                                          lambda t: F.retinanet_decode(t["maps"], t["deltas"], F.retinanet_topk(t["maps"], 3, 5, 0.05), t["cells"],
                                                                       _STRIDES, t["sizes"], 3)),
    "fcos_topk + fcos_decode": (lambda s: dict(maps=_levels(s, 3, -4, 4), ctrs=_levels(s + 2, 1, -4, 4), deltas=_levels(s + 4, 4, 0.0, 3.0),
                                               cells=_cells(s, 1), sizes=_sizes(s)),
                                lambda t: F.fcos_decode(t["maps"], t["ctrs"], t["deltas"], F.fcos_topk(t["maps"], t["ctrs"], 3, 5, 0.05), t["cells"],
                                                        _STRIDES, t["sizes"], 3)),
    "ssd_scores + ssd_topk + ssd_decode": (lambda s: dict(maps=[_f(s, (2, 20, 5, 4), -2, 2), _f(s + 1, (2, 30, 3, 3), -2, 2)],
                                                          deltas=[_f(s + 2, (2, 16, 5, 4)), _f(s + 3, (2, 24, 3, 3))],
                                                          pairs=[_f(s + 4, (4, 2), 0.1, 0.9), _f(s + 5, (6, 2), 0.1, 0.9)], sizes=_sizes(s)),
                                           lambda t: (lambda sc: F.ssd_decode(sc, t["deltas"], F.ssd_topk(sc, 9, 0.05), t["pairs"], None, (40, 32),
                                                                              t["sizes"]))(F.ssd_scores(t["maps"], 5))),
    # ... and the detectors' own form: cell anchors and pairs as host tensors, image sizes as a list (uploaded once, then cached)
    "rpn_topk + rpn_decode[host tables]": (lambda s: dict(maps=_levels(s, 3, -4, 4), deltas=_levels(s + 2, 12, -0.5, 0.5)),
                                           lambda t: F.rpn_decode(t["maps"], t["deltas"], F.rpn_topk(t["maps"], 5), _host_cells(3), _STRIDES,
                                                                  _SIZE_LIST)),
    "retinanet_topk + retinanet_decode[host tables]": (lambda s: dict(maps=_levels(s, 6, -4, 4), deltas=_levels(s + 2, 8, -0.5, 0.5)),
                                                       lambda t: F.retinanet_decode(t["maps"], t["deltas"], F.retinanet_topk(t["maps"], 3, 5, 0.05),
                                                                                    _host_cells(2), _STRIDES, _SIZE_LIST, 3)),
    "fcos_topk + fcos_decode[host tables]": (lambda s: dict(maps=_levels(s, 3, -4, 4), ctrs=_levels(s + 2, 1, -4, 4),
                                                            deltas=_levels(s + 4, 4, 0.0, 3.0)),
                                             lambda t: F.fcos_decode(t["maps"], t["ctrs"], t["deltas"], F.fcos_topk(t["maps"], t["ctrs"], 3, 5, 0.05),
                                                                     _host_cells(1), _STRIDES, _SIZE_LIST, 3)),
    "ssd_scores + ssd_topk + ssd_decode[host tables]": (lambda s: dict(maps=[_f(s, (2, 20, 5, 4), -2, 2), _f(s + 1, (2, 30, 3, 3), -2, 2)],
                                                                       deltas=[_f(s + 2, (2, 16, 5, 4)), _f(s + 3, (2, 24, 3, 3))]),
                                                        lambda t: (lambda sc: F.ssd_decode(sc, t["deltas"], F.ssd_topk(sc, 9, 0.05), _ssd_pairs(), None,
                                                                                           (40, 32), [(40, 32), (37, 30)]))(F.ssd_scores(t["maps"], 5))),
    "roi_detections[host sizes]": (lambda s: dict(logits=_f(s, (6, 5), -3, 3), deltas=_f(s + 1, (6, 20)),
                                                  rois=np.concatenate([(np.arange(6)[:, None] % 2).astype(F32), _boxes(s + 2, 6)], 1)),
                                   lambda t: F.roi_detections(t["logits"], t["deltas"], t["rois"], _SIZE_LIST)),
    "roi_detections": (lambda s: dict(logits=_f(s, (6, 5), -3, 3), deltas=_f(s + 1, (6, 20)),
                                      rois=np.concatenate([(np.arange(6)[:, None] % 2).astype(F32), _boxes(s + 2, 6)], 1), sizes=_sizes(s)),
                       lambda t: F.roi_detections(t["logits"], t["deltas"], t["rois"], t["sizes"])),
    "multiscale_roi_align": (lambda s: dict(f0=_f(s, (2, 4, 16, 16)), f1=_f(s + 1, (2, 4, 8, 8)), b0=_boxes(s + 2, 3, 50.0), b1=_boxes(s + 3, 2, 50.0)),
                             lambda t: ops.MultiScaleRoIAlign(["0", "1"], 3, 2)({"0": t["f0"], "1": t["f1"]}, [t["b0"], t["b1"]], [(64, 64), (64, 64)])),
    "mask_probs + paste": (lambda s: dict(x=_f(s, (3, 4, 7, 7), -3, 3), labels=((np.arange(3) + s) % 4).astype(np.int64), boxes=_boxes(s + 1, 3, 30.0)),
                           lambda t: F.paste_masks_in_image(F.mask_probs(t["x"], t["labels"]), t["boxes"], (40, 44), 1)),
    "detection_batch": (lambda s: dict(images=[_f(s, (3, 20, 24), 0.0, 1.0), _f(s + 1, (3, 18, 30), 0.0, 1.0)]),
                        lambda t: F.detection_batch(t["images"], [(32, 38), (29, 48)], MEAN, STD)),
    # the other forms of the layers
    "conv2d_bias_relu[sliced K, workspace]": (lambda s: dict(x=_f(s, (1, 128, 7, 7)), w=_f(s + 1, (64, 128, 3, 3), -0.1, 0.1), b=_f(s + 2, (64,))),
                                              lambda t: F.conv2d_bias_relu(t["x"], t["w"], t["b"], sliced_k=True)),
    "normalized_conv2d_bias_relu": (lambda s: dict(x=_u8(s, (2, 3, 10, 12)), w=_f(s + 1, (8, 3, 3, 3), -0.3, 0.3), b=_f(s + 2, (8,))),
                                    lambda t: F.normalized_conv2d_bias_relu(t["x"], MEAN, STD, t["w"], t["b"])),
    "deform_conv2d": (lambda s: dict(x=_f(s, (1, 4, 8, 8)), offset=_f(s + 1, (1, 18, 8, 8), -1.5, 1.5), w=_f(s + 2, (6, 4, 3, 3), -0.3, 0.3),
                                     b=_f(s + 3, (6,)), mask=_f(s + 4, (1, 9, 8, 8), 0.0, 1.0)),
                      lambda t: ops.deform_conv2d(t["x"], t["offset"], t["w"], t["b"], padding=(1, 1), mask=t["mask"])),
    "inverted_residual": (lambda s: dict(x=_f(s, (1, 64, 14, 14)), we=_f(s + 1, (384, 64, 1, 1), -0.2, 0.2), a1=_f(s + 2, (384,), 0.5, 1.5),
                                         b1=_f(s + 3, (384,)), wd=_f(s + 4, (384, 1, 3, 3), -0.4, 0.4), a2=_f(s + 5, (384,), 0.5, 1.5),
                                         b2=_f(s + 6, (384,)), wp=_f(s + 7, (64, 384, 1, 1), -0.1, 0.1), a3=_f(s + 8, (64,), 0.5, 1.5),
                                         b3=_f(s + 9, (64,))),
                          lambda t: F.inverted_residual(t["x"], t["we"], t["a1"], t["b1"], t["wd"], t["a2"], t["b2"], t["wp"], t["a3"], t["b3"], True)),
    # the other storage types and the lists of frames of the filters
    "gaussian_blur[f64]": (lambda s: dict(x=_f(s, (2, 3, 20, 24)).astype(np.float64)), lambda t: F.gaussian_blur(t["x"], [3, 3])),
    "gaussian_blur[f16]": (lambda s: dict(x=_f(s, (2, 3, 20, 24), 0.0, 1.0).astype(np.float16)), lambda t: F.gaussian_blur(t["x"], [3, 3])),
    "gaussian_blur[bf16]": (lambda s: dict(x=_f(s, (2, 3, 20, 24), 0.0, 1.0)), lambda t: F.gaussian_blur(t["x"].to(torch.bfloat16), [3, 3])),
    "gaussian_blur[u8 5x5]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.gaussian_blur(t["x"], [5, 5], [1.1, 1.1])),
    "gaussian_blur[u8 21x21]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.gaussian_blur(t["x"], [21, 21], [3.0, 3.0])),
    "adjust_sharpness[f64]": (lambda s: dict(x=_f(s, (2, 3, 20, 24), 0.0, 1.0).astype(np.float64)), lambda t: F.adjust_sharpness(t["x"], 1.5)),
    "box_filter[f64]": (lambda s: dict(x=_f(s, (2, 3, 20, 24)).astype(np.float64)), lambda t: F.box_filter(t["x"], 3)),
    "depthwise_conv2d[f64]": (lambda s: dict(x=_f(s, (2, 3, 20, 24)).astype(np.float64), w=_f(s + 1, (3, 3)).astype(np.float64)),
                              lambda t: F.depthwise_conv2d(t["x"], t["w"])),
    "gaussian_blur_frames[f32 3x3]": (lambda s: dict(frames=_frames(s, F32)), lambda t: tuple(F.gaussian_blur_frames(t["frames"], [3, 3]))),
    "gaussian_blur_frames[f32 9x9]": (lambda s: dict(frames=_frames(s, F32)), lambda t: tuple(F.gaussian_blur_frames(t["frames"], [9, 9], [1.7, 1.7]))),
    "gaussian_blur_frames[u8 3x3]": (lambda s: dict(frames=_frames(s, np.uint8)), lambda t: tuple(F.gaussian_blur_frames(t["frames"], [3, 3]))),
    "gaussian_blur_frames[u8 9x9]": (lambda s: dict(frames=_frames(s, np.uint8)), lambda t: tuple(F.gaussian_blur_frames(t["frames"], [9, 9], [1.7, 1.7]))),
    "gaussian_blur[u8 9x9, separable pair]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: _pair_blur(F.gaussian_blur, t["x"])),
    "gaussian_blur_frames[u8 9x9, separable pair]": (lambda s: dict(frames=_frames(s, np.uint8)),
                                                     lambda t: tuple(_pair_blur(F.gaussian_blur_frames, t["frames"]))),
    "adjust_sharpness_frames[f32]": (lambda s: dict(frames=_frames(s, F32)), lambda t: tuple(F.adjust_sharpness_frames(t["frames"], 1.5))),
    "adjust_sharpness_frames[u8]": (lambda s: dict(frames=_frames(s, np.uint8)), lambda t: tuple(F.adjust_sharpness_frames(t["frames"], 0.5))),
    # the other storage types of the image ops
    "equalize[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)), lambda t: F.equalize(t["x"])),
    "resized_crop_flip_normalize[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)),
                                         lambda t: F.resized_crop_flip_normalize(t["x"], 2, 3, 30, 40, [16, 16], False, MEAN, STD)),
    "mixup_image[f16]": (lambda s: dict(x=_f(s, (4, 3, 8, 10)).astype(np.float16)), lambda t: F.mixup_image(t["x"], 0.3)),
    "mixup_image[f64]": (lambda s: dict(x=_f(s, (4, 3, 8, 10)).astype(np.float64)), lambda t: F.mixup_image(t["x"], 0.3)),
    "image_classification_preset[u8]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: _preset()(t["x"])),
    "image_classification_preset[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)), lambda t: _preset()(t["x"])),
    "elastic[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0), d=_f(s + 1, (1, 40, 56, 2), -0.1, 0.1)), lambda t: F.elastic(t["x"], t["d"])),
    "elastic[u8]": (lambda s: dict(x=_u8(s, _IMG), d=_f(s + 1, (1, 40, 56, 2), -0.1, 0.1)), lambda t: F.elastic(t["x"], t["d"], fill=[1, 2, 3])),
    "rotate[f32]": (lambda s: dict(x=_f(s, _IMG, 0.0, 1.0)), lambda t: F.rotate(t["x"], 30.0, interpolation="bilinear")),
    "affine[u8]": (lambda s: dict(x=_u8(s, _IMG)), lambda t: F.affine(t["x"], 10.0, [3, -2], 1.1, [5.0, 0.0], fill=[1, 2, 3])),
}

# The one stream-taking entry point no wrapper of the package calls any more: conv_norm_act launches mv_dwconv_dilated_norm_act_f32 at
# dilation 1 for the depthwise 5x5.  It stays in the header as a stable ABI; tests/test_gpu_lraspp.py compares the two
# entries at the C ABI.  No capture case: a case would restate a private calling convention.
NO_WRAPPER = {"mv_dwconv_norm_act_f32": "kept in the C ABI for its callers outside the package; conv_norm_act calls mv_dwconv_dilated_norm_act_f32"}

# Stream-taking entry points whose wrapper cannot be captured, with the host read that says why.  The detectors (Faster / Mask /
# Keypoint R-CNN, RetinaNet, FCOS, SSD, SSDlite) end in ops.batched_nms and are not captured for the first reason.
NOT_CAPTURABLE = {
    "mv_nms_f32": "the wrapper returns a data-dependent shape: ops.py, _nms_impl, `return keep[:int(count.item())]` reads the count back",
    "mv_masks_to_boxes_u8": "the wrapper returns a host value: ops.py, masks_to_boxes, `if int(flag.item())` reads the empty-mask flag back "
                            "and raises on it",
    "mv_masks_to_boxes_f32": "the wrapper returns a host value: ops.py, masks_to_boxes, `if int(flag.item())` reads the empty-mask flag back "
                             "and raises on it",
}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _usable(case, d):
    arrs = [v for v in d.values() if isinstance(v, np.ndarray)]
    return all(a.size for a in arrs) and FC.nbytes(d) <= MAX_BYTES  # an empty batch or roi list launches nothing


def _arrays(v):
    return [np.asarray(a) for a in (v.values() if isinstance(v, dict) else v if isinstance(v, (tuple, list)) else (v,))]


def references_differ(case):
    """Whether the CPU references of the case's two data seeds differ: a case whose output does not depend on its data (one class
    to take the argmax over, a ReLU that clears everything) would show nothing when its inputs are refreshed."""
    r1 = _arrays(FC.reference(case, inputs(case)))
    r2 = _arrays(FC.reference(seeded(case, True), inputs(case, second=True)))
    return any(not np.array_equal(a, b, equal_nan=True) for a, b in zip(r1, r2))


def _select(family):
    """Per form the smallest usable case whose two seeds give different references."""
    by_form = {}
    for case in FC.cases(family):
        d = FC.inputs(case)
        if _usable(case, d):
            by_form.setdefault(FORMS[family](case.g), []).append((FC.nbytes(d), case.id, case))
    chosen = [next((case for _, _, case in sorted(found) if references_differ(case)), None) for found in by_form.values()]
    assert all(c is not None for c in chosen), f"{family}: a form without a case whose output depends on its data"
    return sorted(chosen, key=lambda c: c.id)


_CASES = {}


def cases():
    """{id: the case} of every capture case: a tests/_fuzz_cases.py case, or a Hand."""
    if not _CASES:
        for family in CALLS:
            for case in _select(family):
                _CASES[f"{family}[{case.sweep}#{case.index}]"] = case
        for i, (name, (make, fn)) in enumerate(HAND.items()):
            _CASES[name] = Hand(name, 5000 + 20 * i, make, fn)
    return _CASES


def seeded(case, second):
    """The case itself, or the same geometry with the second data seed."""
    if not second:
        return case
    return dataclasses.replace(case, geom=tuple((k, v + SEED_STEP if k == "seed" else v) for k, v in case.geom))


def inputs(case, second=False):
    """{name: numpy array, list of arrays or None} of a case from its first or second data seed."""
    if isinstance(case, Hand):
        return case.make(case.seed + (SEED_STEP if second else 0))
    return FC.inputs(seeded(case, second))


def _tensor(v, device):
    if isinstance(v, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(v)).to(device)
    return [_tensor(a, device) for a in v] if isinstance(v, list) else v


def tensors(d, device="cpu"):
    return {k: _tensor(v, device) for k, v in d.items()}


def arrays(d):
    """Every numpy array of a case's inputs, the entries of lists included, as (name, array)."""
    out = []
    for k, v in d.items():
        out.extend([(k, v)] if isinstance(v, np.ndarray) else [(f"{k}[{i}]", a) for i, a in enumerate(v)] if isinstance(v, list) else [])
    return out


def refresh(t, second):
    """Overwrite every tensor of t in place with the one of `second`."""
    for k, v in t.items():
        for dst, src in zip(v if isinstance(v, list) else [v], second[k] if isinstance(v, list) else [second[k]]):
            if isinstance(dst, torch.Tensor):
                dst.copy_(src)


def call(case, t):
    """The case's call on the tensors t: a tensor or a tuple of tensors."""
    return case.fn(t) if isinstance(case, Hand) else CALLS[case.family](case.g, t)
