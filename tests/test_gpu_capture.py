"""Calls of single entry points and whole forwards inside a HIP graph.

Entry points: every case of tests/_capture_cases.py (one call per form of every wrapper that can be captured) is computed eagerly on
the default stream, warmed up on a side stream, captured on one stream and replayed; the replay must equal the eager result.  Then
EVERY device input of the case -- weights, biases, norm terms, boxes, gates, not only x -- is overwritten in place with the data of a
second seed, and another replay must equal the eager call on the new contents.  A recording proxy around the library
(_capture_cases.Recorder) notes the mv_* names called under capture; the last test of the section asserts that they, together with _capture_cases.NOT_CAPTURABLE and NO_WRAPPER, are the 111 stream-taking entry points of the
header.

Whole forwards: tiny models of every family that came after MobileNetV2 (whose capture test is in
tests/test_gpu_mobilenet.py): graphs.capture(forward, x), then replays on new inputs, each equal to the eager forward bit for bit with
NaN in equal places.

The reference is the eager path: eager bits are what every other GPU test compares with the oracle, stage by stage.  This file adds
capture and stream invariance only -- a launch or memset on the null stream, a host read of device data, a per-call upload or an
allocation outside the graph's pool raises during the capture; a value baked on the host from an input's contents shows in the second
replay.  The detectors end in NMS, whose output shape depends on the data: they are not captured.  The parameters stay as they are
after the capture (the graph holds pointers to the cached folds; see graphs.py)."""
from collections import OrderedDict
from functools import partial

import numpy as np
import pytest
import torch
from torch import nn

import cpu_vision_amd as mv
from cpu_vision_amd import functional as F
from cpu_vision_amd import _lib, graphs, mobilenetv3, resnet, segmentation
from cpu_vision_amd.convnext import CNBlockConfig, ConvNeXt
from tests import _capture_cases as CC
from tests import _convnext_ref as CR
from tests import _mobilenetv3_ref as MR

pytestmark = pytest.mark.gpu

N = 2  # batch


def _x(seed, side):
    return torch.from_numpy(np.random.Generator(np.random.Philox(seed)).standard_normal((N, 3, side, side)).astype(np.float32)).cuda()


# ---- the models -----------------------------------------------------------------------------------------------------------------------
class _Trunk(nn.Module):
    """The children of a ResNet with a few channels -- a stem, a BasicBlock stage, a Bottleneck stage with a strided downsample -- for
    IntermediateLayerGetter, which runs them.  dilate: the Bottleneck stage at dilation 2 in place of its stride (a segmentation
    trunk)."""

    def __init__(self, dilate: bool = False) -> None:
        super().__init__()
        self.conv1 = nn.Conv2d(3, 8, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(8)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = nn.Sequential(resnet.BasicBlock(8, 8), resnet.BasicBlock(8, 8))
        down = nn.Sequential(resnet.conv1x1(8, 16, 1 if dilate else 2), nn.BatchNorm2d(16))
        self.layer2 = nn.Sequential(resnet.Bottleneck(8, 4, 1 if dilate else 2, down), resnet.Bottleneck(16, 4, dilation=2 if dilate else 1))


class _TinyResNet(nn.Module):
    """ResNet.forward on the trunk: the stages, the average pool, the classifier."""

    def __init__(self) -> None:
        super().__init__()
        self.body = mv.IntermediateLayerGetter(_Trunk(), {"layer2": "out"})
        self.fc = nn.Linear(16, 5)

    def forward(self, x):
        y = F.adaptive_avg_pool2d(self.body(x)["out"], (1, 1))
        return F.linear_bias_relu(torch.flatten(y, 1), self.fc.weight, self.fc.bias, relu=False)


_ROW = partial(mobilenetv3.InvertedResidualConfig, width_mult=1.0)


def _mobilenet_v3(dilated: bool):
    """A stride-2 3x3 block, then two 5x5 blocks with squeeze-excitation (the second with the residual); dilated: the 5x5 blocks at
    dilation 2, as the segmentation backbones have them."""
    d = 2 if dilated else 1
    rows = [_ROW(8, 3, 16, 8, False, "RE", 2, 1), _ROW(8, 5, 24, 16, True, "HS", 2, d), _ROW(16, 5, 32, 16, True, "HS", 1, d)]
    return mobilenetv3.MobileNetV3(rows, last_channel=24, num_classes=5)


def _segmentation_trunk(aux):
    return mv.IntermediateLayerGetter(_Trunk(dilate=True), {"layer2": "out", **({"layer1": "aux"} if aux else {})})


def _make(name):
    if name == "resnet":
        return _TinyResNet()
    if name == "mobilenet_v3":
        return _mobilenet_v3(dilated=False)
    if name == "convnext":
        return ConvNeXt([CNBlockConfig(*r) for r in CR.NET_ROWS], num_classes=7)
    if name == "resnet_fpn_backbone":
        return mv.BackboneWithFPN(_Trunk(), {"layer1": "0", "layer2": "1"}, [8, 16], 8)
    if name == "fcn":
        return segmentation.FCN(_segmentation_trunk(True), segmentation.FCNHead(16, 4), segmentation.FCNHead(8, 4))
    if name == "deeplabv3":
        return segmentation.DeepLabV3(_segmentation_trunk(True), segmentation.DeepLabHead(16, 4, (2, 3)), segmentation.FCNHead(8, 4))
    if name == "lraspp":
        body = mv.IntermediateLayerGetter(_mobilenet_v3(dilated=True).features, {"1": "low", "4": "high"})
        return segmentation.LRASPP(body, 8, 96, 4, inter_channels=16)
    raise KeyError(name)


def _model(name, seed):
    torch.manual_seed(seed)
    model = _make(name).eval()
    if name == "convnext":
        CR.perturb(model, seed + 1)
        CR.scale_weights(model, 6.0)
    else:
        MR.perturb(model, seed + 1)
    return model.cuda()


def _flat(out):
    if isinstance(out, torch.Tensor):
        return [("", out)]
    return list(out.items()) if isinstance(out, (dict, OrderedDict)) else [(str(i), v) for i, v in enumerate(out)]


def _clone(out):
    return [(k, v.clone()) for k, v in _flat(out)]


def _same(got, want, what):
    got, want = _flat(got), want
    assert [k for k, _ in got] == [k for k, _ in want], what
    for (k, g), (_, w) in zip(got, want):
        if g.dtype is torch.bfloat16:  # numpy has no bfloat16: the bits (a blur of finite values has no NaN)
            g, w = g.view(torch.int16), w.view(torch.int16)
        MR.same(g, w, f"{what} {k}")


def _differ(a, b):
    return any(not torch.equal(u, v) for (_, u), (_, v) in zip(a, b))


def _captured_equals_eager(fn, side, seed, what):
    x1, x2, x3 = _x(seed, side), _x(seed + 1, side), _x(seed + 2, side)
    with torch.no_grad():
        want = [_clone(fn(x)) for x in (x1, x2, x3)]
        assert _differ(want[0], want[1]) and _differ(want[1], want[2]), f"{what}: the inputs do not reach the output"
        cap = graphs.capture(fn, x1)
        for k in (0, 1, 2, 0):
            _same(cap((x1, x2, x3)[k]), want[k], f"{what}: replay on input {k}")
    return want


# ---- single entry points ------------------------------------------------------------------------------------------------------------------
SEEN = {}  # case id -> (the kernel of the eager call on the second seed's data, the mv_* names called under capture)


def _capture_case(name, monkeypatch):
    case = CC.cases()[name]
    t = CC.tensors(CC.inputs(case), "cuda")
    second = CC.tensors(CC.inputs(case, second=True), "cuda")
    eager0 = _clone(CC.call(case, t))  # 1. eager, default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # 2. warm-up outside the capture
        CC.call(case, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    rec = CC.Recorder(_lib.load(), launch=True)
    monkeypatch.setattr(_lib, "_lib", rec)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # 3. one stream, no parallel branches
        out = CC.call(case, t)
    monkeypatch.undo()
    graph.replay()  # 4.
    torch.cuda.synchronize()
    _same(out, eager0, f"{name}: first replay")
    CC.refresh(t, second)  # 5. every device input, in place
    graph.replay()  # 6.
    torch.cuda.synchronize()
    want = _clone(CC.call(case, t))
    kernel = _lib.last_kernel()
    _same(out, want, f"{name}: replay on the second seed's data [{kernel}]")
    assert _differ(want, eager0), f"{name}: the second seed's data give the first result"
    assert rec.names and set(rec.names) <= CC.captured_entry_points(), (name, rec.names)
    SEEN[name] = (kernel, tuple(rec.names))


@pytest.mark.parametrize("name", list(CC.cases()))
def test_entry_point_in_a_captured_graph(name, monkeypatch):
    _capture_case(name, monkeypatch)


def test_captures_reach_every_stream_taking_entry_point(monkeypatch):
    """The census of tests/test_capture_cases_host.py on the device: the names called under capture, together with the not-capturable
    table, are the stream-taking entry points of the header (the cases that have not run in this process run here)."""
    for name in CC.cases():
        if name not in SEEN:
            _capture_case(name, monkeypatch)
    called = {n for _, names in SEEN.values() for n in names}
    assert not called & (set(CC.NOT_CAPTURABLE) | set(CC.NO_WRAPPER))
    assert called | set(CC.NOT_CAPTURABLE) | set(CC.NO_WRAPPER) == CC.stream_entry_points()
    assert all(kernel.startswith("k_") for kernel, _ in SEEN.values()), SEEN


# ---- forwards -------------------------------------------------------------------------------------------------------------------------
FORWARDS = {"resnet": 64, "mobilenet_v3": 64, "convnext": 64, "resnet_fpn_backbone": 64, "fcn": 48, "deeplabv3": 33, "lraspp": 40}


@pytest.mark.parametrize("name", list(FORWARDS))
def test_forward_in_a_captured_graph(name):
    model = _model(name, 9700 + len(name))
    want = _captured_equals_eager(model, FORWARDS[name], 9800 + len(name), name)
    keys = [k for k, _ in want[0]]
    assert keys == {"resnet_fpn_backbone": ["0", "1", "pool"], "fcn": ["out", "aux"], "deeplabv3": ["out", "aux"], "lraspp": ["out"]}.get(name, [""])


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
@pytest.mark.parametrize("name", ["fcn", "deeplabv3", "lraspp"])
def test_fused_labels_in_a_captured_graph(name, dtype):
    model = _model(name, 9700 + len(name))
    side = FORWARDS[name]
    last = model.classifier.high_classifier if name == "lraspp" else model.classifier[4]
    with torch.no_grad():  # the random biases otherwise decide the argmax everywhere: every class the same mean logit on one input
        last.bias -= model(_x(9900, side))["out"].mean(dim=(0, 2, 3))
    want = _captured_equals_eager(partial(model.labels, dtype=dtype), side, 9800 + len(name), f"{name} labels {dtype}")
    for _, labels in want[0]:
        assert labels.dtype == dtype and labels.shape == (N, side, side) and len(labels.unique()) > 1
