"""FCN / DeepLabV3 and F.interpolate_argmax without a device: the module trees, state-dict keys, shapes and seeded initialisation of
the four builders against the plain-torch replica (tests/_segmentation_ref.py), the argument errors, the refusals of
mv_interpolate_argmax_f32 with host pointers (they come before any launch), and the non-vacuity of the helper and its fixtures:
its interpolate_argmax against torch's CPU interpolate(...).argmax(1), ties in the tie fixture, NaN in the NaN fixture."""
import numpy as np
import pytest
import torch

import cpu_vision_amd as mv
from cpu_vision_amd import _lib, resnet, segmentation
from cpu_vision_amd import functional as F
from tests import _interp_ref as IR
from tests import _segmentation_ref as R

BUILDERS = ["fcn_resnet50", "fcn_resnet101", "deeplabv3_resnet50", "deeplabv3_resnet101"]


# ---- trees, keys, shapes, seeded initialisation ----------------------------------------------------------------------------------------
def _tree(model):
    """(name, what kind of parameter container) of every module; the fused wrappers stand where the reference has a Sequential."""
    kinds = (torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.ReLU, torch.nn.Dropout, torch.nn.AdaptiveAvgPool2d, torch.nn.MaxPool2d,
             torch.nn.ModuleList)
    return [(name, next((k.__name__ for k in kinds if isinstance(m, k)), "container")) for name, m in model.named_modules()]


@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("name", BUILDERS)
def test_builders_match_the_replica(name, aux):
    torch.manual_seed(5)
    got = getattr(mv, name)(num_classes=3, aux_loss=aux)
    torch.manual_seed(5)
    want = R.replica(name, num_classes=3, aux_loss=aux)
    assert _tree(got) == _tree(want)
    gs, ws = got.state_dict(), want.state_dict()
    assert list(gs) == list(ws)
    for k in gs:
        assert gs[k].shape == ws[k].shape and gs[k].dtype == ws[k].dtype, k
        assert torch.equal(gs[k], ws[k]), k  # the same draws from torch's RNG in the same order
    assert (got.aux_classifier is not None) == aux and not got.training
    assert type(got).__name__ == ("FCN" if name.startswith("fcn") else "DeepLabV3")
    assert gs["classifier.4.weight" if name.startswith("fcn") else "classifier.4.weight"].shape[0] == 3
    want.load_state_dict(gs)  # the keys are the reference's in both directions
    got.load_state_dict(ws)


def test_builder_defaults_and_names():
    m = mv.fcn_resnet50()
    assert m.classifier[4].out_channels == 21 and m.aux_classifier is None
    assert list(m.backbone.return_layers.items()) == [("layer4", "out")]
    d = mv.deeplabv3_resnet50(aux_loss=True)
    assert d.classifier[4].out_channels == 21 and d.aux_classifier[0].in_channels == 1024
    assert [c[0].dilation[0] for c in list(d.classifier[0].convs)[1:4]] == [12, 24, 36]
    assert d.backbone["layer3"][1].conv2.dilation == (2, 2) and d.backbone["layer4"][1].conv2.dilation == (4, 4)
    for name in ("FCN", "FCNHead", "DeepLabV3", "DeepLabHead", "ASPP", "ASPPConv", "ASPPPooling", *BUILDERS):
        assert getattr(mv, name) is getattr(segmentation, name) and name in segmentation.__all__
    assert F.interpolate_argmax.__module__.endswith("_segment")
    assert segmentation.SLICE_CHANNELS == R.SLICE_CHANNELS == 128  # the helper restates the heads' summation slices


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------
def test_builder_and_module_argument_errors():
    for name in BUILDERS:
        with pytest.raises(ValueError, match="ships no weight files"):
            getattr(mv, name)(weights="DEFAULT")
        with pytest.raises(ValueError, match="ships no weight files"):
            getattr(mv, name)(weights_backbone="IMAGENET1K_V1")
    with pytest.raises(ValueError, match="return_layers are not present"):
        mv.IntermediateLayerGetter(resnet.resnet18(), {"layer5": "out"})
    with pytest.raises(ValueError, match="3-element tuple"):
        resnet.resnet18(replace_stride_with_dilation=[False, True])
    x = torch.zeros(1, 3, 16, 16)
    model = segmentation.FCN(mv.IntermediateLayerGetter(resnet.resnet18(), {"layer4": "out"}), mv.FCNHead(512, 3))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        model(x)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        model.labels(x)
    model.train()
    with pytest.raises(RuntimeError, match="inference only"):
        model(x)
    with pytest.raises(RuntimeError, match="inference only"):
        model.labels(x)
    for head, shape in ((mv.FCNHead(16, 3), (1, 16, 4, 4)), (mv.ASPP(8, (1, 2), 8), (1, 8, 4, 4)), (mv.DeepLabHead(8, 3, (1,)), (1, 8, 4, 4))):
        with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
            head(torch.zeros(shape))
        with pytest.raises(RuntimeError, match="inference only"):
            head.train()(torch.zeros(shape))


def test_interpolate_argmax_argument_errors():
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(NotImplementedError, match="mode='nearest'"):
        F.interpolate_argmax(x, size=(8, 8), mode="nearest")
    with pytest.raises(NotImplementedError, match="align_corners=True"):
        F.interpolate_argmax(x, size=(8, 8), align_corners=True)
    with pytest.raises(NotImplementedError, match="antialias=True"):
        F.interpolate_argmax(x, size=(8, 8), antialias=True)
    with pytest.raises(NotImplementedError, match="3 dimensions"):
        F.interpolate_argmax(x[0], size=(8, 8))
    with pytest.raises(NotImplementedError, match="float64"):
        F.interpolate_argmax(x.double(), size=(8, 8))
    with pytest.raises(NotImplementedError, match="int32"):
        F.interpolate_argmax(x, size=(8, 8), dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="recompute_scale_factor=True"):
        F.interpolate_argmax(x, scale_factor=2.0)
    with pytest.raises(ValueError, match="only one of size or scale_factor"):
        F.interpolate_argmax(x, size=(8, 8), scale_factor=2.0)
    with pytest.raises(ValueError, match="either size or scale_factor"):
        F.interpolate_argmax(x)
    with pytest.raises(ValueError, match="greater than 0"):
        F.interpolate_argmax(x, size=(0, 8))
    with pytest.raises(ValueError, match="uint8 label"):
        F.interpolate_argmax(torch.zeros(1, 257, 2, 2), size=(3, 3), dtype=torch.uint8)
    with pytest.raises(IndexError, match="non-zero size"):
        F.interpolate_argmax(torch.zeros(1, 0, 2, 2), size=(3, 3))
    with pytest.raises(IndexError):
        torch.zeros(1, 0, 3, 3).argmax(1)  # what the message restates
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.interpolate_argmax(x, size=(8, 8))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.interpolate_argmax(torch.zeros(1, 256, 2, 2), size=(3, 3), dtype=torch.uint8)


# ---- the entry point refuses before any launch ---------------------------------------------------------------------------------------------
def test_interpolate_argmax_abi_refusals_without_a_device():
    lib = _lib.load()
    x = np.zeros((2, 3, 4, 4), np.float32)
    y = np.zeros((2, 8, 8), np.int64)
    xp, yp = x.ctypes.data, y.ctypes.data

    def call(**o):
        a = {**dict(x=xp, y=yp, n=2, c=3, h=4, w=4, oh=8, ow=8, out_bytes=8), **o}
        return lib.mv_interpolate_argmax_f32(a["x"], a["y"], a["n"], a["c"], a["h"], a["w"], a["oh"], a["ow"], a["out_bytes"], None)
    for over, text in ((dict(c=0), "bad shape"), (dict(c=-2), "bad shape"), (dict(h=0), "bad shape"), (dict(w=-1), "bad shape"),
                       (dict(oh=0), "bad shape"), (dict(ow=0), "bad shape"), (dict(n=-1), "bad shape"), (dict(out_bytes=4), "out_bytes"),
                       (dict(out_bytes=0), "out_bytes"), (dict(out_bytes=1, c=257), "uint8 label"), (dict(x=None), "null pointer"),
                       (dict(y=None), "null pointer"), (dict(y=yp + 1), "8-byte aligned"), (dict(y=xp), "must not overlap"),
                       (dict(y=xp + 64), "must not overlap")):
        assert call(**over) == -1 and text in lib.mv_last_error().decode(), (over, lib.mv_last_error())
    assert call(n=0, x=None, y=None) == 0
    assert call(n=0, x=None, y=None, out_bytes=1, c=256) == 0
    assert call(n=0, c=0) == -1  # the shape is checked before the empty batch returns
    assert call(n=2 ** 31, oh=1, ow=1, y=xp + 2 ** 50) == -2 and "launch grid" in lib.mv_last_error().decode()
    assert call(h=2 ** 15, w=2 ** 15, y=xp + 2 ** 50) == -2 and "32-bit byte offset" in lib.mv_last_error().decode()
    assert call(n=2 ** 40, oh=2 ** 20, ow=2 ** 20, y=xp + 2 ** 50) == -1 and "address space" in lib.mv_last_error().decode()
    assert not y.any()


# ---- non-vacuity of the helper and its fixtures ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.fixtures()))
def test_helper_equals_torch_cpu(name):
    x, (oh, ow) = R.fixtures()[name]
    want = torch.nn.functional.interpolate(torch.from_numpy(x), size=(oh, ow), mode="bilinear", align_corners=False).argmax(1)
    got = R.interpolate_argmax(x, oh, ow)
    assert got.dtype == np.int64 and got.shape == (x.shape[0], oh, ow)
    assert np.array_equal(got, want.numpy())


def test_argmax_rule_is_torch_argmax():
    nan, inf = np.nan, np.inf
    v = np.array([[[0.0, -0.0, 1.0, nan, 2.0, -inf, inf, nan], [-0.0, 0.0, 1.0, 5.0, nan, -inf, inf, nan],
                   [0.0, 0.0, 2.0, nan, nan, -inf, nan, 1.0]]], np.float32).reshape(1, 3, 1, 8)
    want = torch.from_numpy(v).argmax(1).numpy()
    assert np.array_equal(R.argmax_rule(v), want)
    assert want.reshape(-1).tolist() == [0, 0, 2, 0, 1, 0, 2, 0]


def test_the_tie_fixture_has_ties():
    x = R.fixture_ties()
    v = IR.interpolate(x, 23, 31)
    top = v.max(axis=1, keepdims=True)
    share = float(((v == top).sum(axis=1) >= 2).mean())
    print(f"tie fixture: {share:.1%} of the output pixels have their maximum attained by two or more classes")
    assert share >= 0.10
    labels = R.interpolate_argmax(x, 23, 31)
    assert (labels == 1).any() and not (labels == 3).any()  # the copy never wins against the original
    z = R.fixture_signed_zeros()
    vz = IR.interpolate(z, 9, 11)
    assert np.signbit(vz[0, 1]).all() and not np.signbit(vz[0, 2]).any() and (vz[0, 0] < 0).all()
    assert (R.interpolate_argmax(z, 9, 11) == 1).all()


def test_the_special_fixture_has_nan_in_two_classes_and_in_none():
    x = R.fixture_special()
    v = IR.interpolate(x, 13, 17)
    nans = np.isnan(v).sum(axis=1)
    assert (nans >= 2).any() and (nans == 0).any() and (nans == 1).any()
    assert np.isposinf(v).any() and np.isneginf(v).any()
    labels = R.interpolate_argmax(x, 13, 17)
    two = nans[0] >= 2
    assert (labels[0][two] == 1).all()  # the first NaN of classes 1 and 3
    x255, (oh, ow) = R.fixtures()["class_255"]
    assert R.interpolate_argmax(x255, oh, ow)[0, 2, 2] == 255


def test_pooling_branch_differs_from_a_broadcast():
    """Why ASPPPooling keeps its interpolate: from a 1x1 source both taps read the one value v, and fma(w0, v, w1 * v) with
    w0 + w1 == 1 is not v for every weight pair."""
    v = np.random.Generator(np.random.Philox(3)).standard_normal((2, 8, 1, 1), dtype=np.float32)
    resized = IR.interpolate(v, 5, 7)
    assert (resized != np.broadcast_to(v, resized.shape)).any()
    torch_resized = torch.nn.functional.interpolate(torch.from_numpy(v), size=(5, 7), mode="bilinear", align_corners=False)
    assert not torch.equal(torch_resized, torch.from_numpy(v).expand(2, 8, 5, 7))
    inf = IR.interpolate(np.full((1, 1, 1, 1), np.inf, np.float32), 3, 3)
    assert np.isnan(inf).any()  # a zero weight times inf
