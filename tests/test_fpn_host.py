"""FPN without a GPU: the refusals of mv_conv1x1_upsample_add_f32 (they return before any launch), the Python checks of
F.conv1x1_upsample_add that fire before a device is needed, and the module trees of cpu_vision_amd.fpn / backbone_utils against
the torch.nn replica of the reference (tests/_fpn_ref.py): state-dict keys and shapes, seeded parameters, both load directions,
the version-1 key renaming, and what each constructor refuses."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch
from torch import nn

import cpu_vision_amd as mv
from cpu_vision_amd import _lib, backbone_utils, fpn, ops, resnet
from cpu_vision_amd import functional as F
from cpu_vision_amd.mobilenet import FrozenBatchNorm2d
from tests import _fpn_ref as P

INVALID, UNSUPPORTED = -1, -2  # MV_ERR_INVALID_ARGUMENT, MV_ERR_UNSUPPORTED


def _ptr(a):
    if a is None or isinstance(a, int):
        return a
    return a.ctypes.data_as(C.c_void_p)


def _call(lib, x, w, top, y, bias=None, alpha=None, beta=None, n=1, cin=4, h=5, wd=7, cout=8, top_h=3, top_w=4, affine=0, act=0):
    return lib.mv_conv1x1_upsample_add_f32(_ptr(x), _ptr(w), _ptr(bias), _ptr(alpha), _ptr(beta), _ptr(top), _ptr(y), n, cin, h, wd, cout,
                                           top_h, top_w, affine, act, None)


def test_abi_refusals_without_a_device():
    """Host pointers are enough: every refusal comes before the first launch, with a negative status and a message, and writes
    nothing."""
    lib = _lib.load()
    x, w = np.zeros((1, 4, 5, 7), np.float32), np.zeros((8, 4), np.float32)
    top, y = np.zeros((1, 8, 3, 4), np.float32), np.full((1, 8, 5, 7), -7.25, np.float32)
    a = np.ones(8, np.float32)
    kernel_before = lib.mv_last_kernel()

    def refused(rc, text, status=INVALID):
        assert rc == status and text in lib.mv_last_error().decode(), (rc, lib.mv_last_error())
        assert lib.mv_last_kernel() == kernel_before  # no launch was attempted

    refused(_call(lib, None, w, top, y), "null pointer")
    refused(_call(lib, x, None, top, y), "null pointer")
    refused(_call(lib, x, w, None, y), "null pointer")
    refused(_call(lib, x, w, top, None), "null pointer")
    refused(_call(lib, x, w, top, y, top_h=0), "bad top size (0, 4)")
    refused(_call(lib, x, w, top, y, top_w=0), "bad top size (3, 0)")
    refused(_call(lib, x, w, top, y, top_h=-2), "bad top size (-2, 4)")
    for affine in (1, 2):
        refused(_call(lib, x, w, top, y, alpha=None, beta=a, affine=affine), "affine without alpha / beta")
        refused(_call(lib, x, w, top, y, alpha=a, beta=None, affine=affine), "affine without alpha / beta")
    refused(_call(lib, x, w, top, y, affine=3), "bad affine (3) / activation (0) code")
    refused(_call(lib, x, w, top, y, affine=-1), "bad affine (-1) / activation (0) code")
    refused(_call(lib, x, w, top, y, act=5), "bad affine (0) / activation (5) code")
    refused(_call(lib, x, w, top, y, act=-1), "bad affine (0) / activation (-1) code")
    refused(_call(lib, x, w, top, x[:, :4], cout=4), "output must not overlap input, weight or top")
    refused(_call(lib, x, w, top, w, h=1, wd=4, cout=1, cin=4), "output must not overlap input, weight or top")
    refused(_call(lib, x, w, top, top, h=3, wd=4), "output must not overlap input, weight or top")
    refused(_call(lib, x, w, top, top.reshape(-1)[95:], h=1, wd=1, top_h=3, top_w=4), "output must not overlap input, weight or top")  # the last element
    refused(_call(lib, x, w, top, y, cin=0), "bad conv shape")
    refused(_call(lib, x, w, top, y, h=0), "bad conv shape")
    refused(_call(lib, x, w, top, y, n=-1), "bad conv shape")
    # sizes beyond one launch; the "pointers" are far-apart integers that nothing dereferences
    far = dict(x=1 << 40, w=2 << 40, top=3 << 40, y=4 << 40)
    refused(_call(lib, **far, n=65536, cin=1, cout=1, h=1, wd=1, top_h=1, top_w=1), "too large for one launch", UNSUPPORTED)
    refused(_call(lib, **far, n=1, cin=1, cout=1, h=65536, wd=32768, top_h=1, top_w=1), "plane too large", UNSUPPORTED)
    refused(_call(lib, **far, n=1, cin=1, cout=1, h=2, wd=2, top_h=65536, top_w=32768), "top plane too large", UNSUPPORTED)
    # a plane within 1024 pixels of 2^31: the last workgroup's int pixel indices would pass 2^31
    refused(_call(lib, **far, n=1, cin=1, cout=1, h=1, wd=2 ** 31 - 1024, top_h=1, top_w=1), "plane too large", UNSUPPORTED)
    assert np.all(y == -7.25)

    # n == 0: a successful no-op that looks at no pointer -- but after the shape and code checks
    assert _call(lib, None, None, None, None, n=0) == 0
    assert _call(lib, x, w, top, y, n=0, affine=2) == 0
    assert _call(lib, None, None, None, None, n=0, top_h=0) == INVALID
    assert _call(lib, None, None, None, None, n=0, act=7) == INVALID
    assert lib.mv_last_kernel() == kernel_before and np.all(y == -7.25)


def test_python_checks_without_a_device():
    x, w, top = torch.zeros(2, 4, 5, 7), torch.zeros(8, 4, 1, 1), torch.zeros(2, 8, 3, 4)
    v = torch.ones(8)
    with pytest.raises(ValueError, match="needs `top`"):
        F.conv1x1_upsample_add(x, w)
    with pytest.raises(RuntimeError, match="does not match the output's batch and channels"):
        F.conv1x1_upsample_add(x, w, top=top[:1])
    with pytest.raises(RuntimeError, match="does not match the output's batch and channels"):
        F.conv1x1_upsample_add(x, w, top=torch.zeros(2, 7, 3, 4))
    with pytest.raises(RuntimeError, match="does not match the output's batch and channels"):
        F.conv1x1_upsample_add(x, w, top=torch.zeros(2, 8, 0, 4))
    with pytest.raises(RuntimeError, match="does not match the output's batch and channels"):
        F.conv1x1_upsample_add(x, w, top=torch.zeros(16, 3, 4))
    with pytest.raises(NotImplementedError, match="pointwise 1x1"):
        F.conv1x1_upsample_add(x, torch.zeros(8, 4, 3, 3), top=top)
    with pytest.raises(NotImplementedError, match="pointwise 1x1"):
        F.conv1x1_upsample_add(x, torch.zeros(8, 2, 1, 1), top=top)
    with pytest.raises(RuntimeError, match="Expected 4D"):
        F.conv1x1_upsample_add(x[0], w, top=top)
    with pytest.raises(ValueError, match="unknown"):
        F.conv1x1_upsample_add(x, w, top=top, activation="gelu")
    with pytest.raises(ValueError, match="unknown"):
        F.conv1x1_upsample_add(x, w, top=top, alpha=v, beta=v, affine="group")
    with pytest.raises(ValueError, match="needs alpha and beta"):
        F.conv1x1_upsample_add(x, w, top=top, affine="fma")
    with pytest.raises(RuntimeError, match="alpha has 4 elements for 8 output channels"):
        F.conv1x1_upsample_add(x, w, top=top, alpha=v[:4], beta=v, affine="fma")
    with pytest.raises(RuntimeError, match="bias has 3 elements for 8 output channels"):
        F.conv1x1_upsample_add(x, w, bias=v[:3], top=top)
    with pytest.raises(Exception, match="(?i)gpu|device|cuda"):  # and no CPU fall-back
        F.conv1x1_upsample_add(x, w, top=top)


def test_the_names_are_exported():
    for name in ("ExtraFPNBlock", "FeaturePyramidNetwork", "LastLevelMaxPool", "LastLevelP6P7"):
        assert getattr(ops, name) is getattr(fpn, name) is getattr(mv, name)
    for name in ("IntermediateLayerGetter", "BackboneWithFPN", "resnet_fpn_backbone"):
        assert getattr(mv, name) is getattr(backbone_utils, name)
    assert F.conv1x1_upsample_add is mv.functional.conv1x1_upsample_add


def _same_tree(ours, theirs):
    a, b = ours.state_dict(), theirs.state_dict()
    assert list(a) == list(b)
    assert [tuple(v.shape) for v in a.values()] == [tuple(v.shape) for v in b.values()]
    return a


@pytest.mark.parametrize("norm", [None, nn.BatchNorm2d, "frozen"], ids=["no norm", "BatchNorm2d", "FrozenBatchNorm2d"])
def test_fpn_state_dict_has_the_replicas_keys_and_shapes(norm):
    ours = fpn.FeaturePyramidNetwork([64, 128, 256, 512], 256, norm_layer=FrozenBatchNorm2d if norm == "frozen" else norm)
    theirs = P.FeaturePyramidNetwork([64, 128, 256, 512], 256, norm_layer=P.FrozenBatchNorm2d if norm == "frozen" else norm)
    sd = _same_tree(ours, theirs)
    assert tuple(sd["inner_blocks.3.0.weight"].shape) == (256, 512, 1, 1) and tuple(sd["layer_blocks.0.0.weight"].shape) == (256, 256, 3, 3)
    assert ("inner_blocks.0.0.bias" in sd) == (norm is None) and ("layer_blocks.2.1.running_var" in sd) == (norm is not None)
    assert not ours.training and ours._version == 2 == theirs._version
    ours = fpn.FeaturePyramidNetwork([8, 16], 16, extra_blocks=fpn.LastLevelP6P7(16, 16))
    sd = _same_tree(ours, P.FeaturePyramidNetwork([8, 16], 16, extra_blocks=P.LastLevelP6P7(16, 16)))
    assert "extra_blocks.p6.weight" in sd and "extra_blocks.p7.bias" in sd and ours.extra_blocks.use_P5
    assert not fpn.LastLevelP6P7(32, 16).use_P5 and list(fpn.LastLevelMaxPool().state_dict()) == []


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_backbone_state_dict_has_the_replicas_keys_and_shapes(name):
    ours, theirs = mv.resnet_fpn_backbone(backbone_name=name), P.resnet_fpn_backbone(backbone_name=name)
    sd = _same_tree(ours, theirs)
    wide = 4 if name == "resnet50" else 1
    assert tuple(sd["fpn.inner_blocks.0.0.weight"].shape) == (256, 64 * wide, 1, 1)
    assert tuple(sd["fpn.inner_blocks.3.0.weight"].shape) == (256, 512 * wide, 1, 1)
    assert "body.layer4.1.conv2.weight" in sd and "body.bn1.running_mean" in sd and not any(k.startswith("body.fc") for k in sd)
    assert ours.out_channels == 256 and isinstance(ours.fpn.extra_blocks, fpn.LastLevelMaxPool) and not ours.training
    assert isinstance(ours.body, backbone_utils.IntermediateLayerGetter) and list(ours.body) == list(theirs.body)
    assert ours.body.return_layers == theirs.body.return_layers == {"layer1": "0", "layer2": "1", "layer3": "2", "layer4": "3"}
    assert isinstance(ours.body["bn1"], FrozenBatchNorm2d)
    # the reference's freezing: trainable_layers = 3 leaves layer2 .. layer4 trainable
    frozen = lambda m: [k for k, p in m.named_parameters() if not p.requires_grad]  # noqa: E731
    assert frozen(ours) == frozen(theirs) and "body.conv1.weight" in frozen(ours) and "body.layer2.0.conv1.weight" not in frozen(ours)
    for layers in (0, 5):
        assert frozen(mv.resnet_fpn_backbone(backbone_name="resnet18", trainable_layers=layers, norm_layer=nn.BatchNorm2d)) == \
            frozen(P.resnet_fpn_backbone(backbone_name="resnet18", trainable_layers=layers, norm_layer=nn.BatchNorm2d))
    part = _same_tree(mv.resnet_fpn_backbone(backbone_name=name, returned_layers=[2, 3, 4], extra_blocks=fpn.LastLevelP6P7(256, 256)),
                      P.resnet_fpn_backbone(backbone_name=name, returned_layers=[2, 3, 4], extra_blocks=P.LastLevelP6P7(256, 256)))
    assert tuple(part["fpn.inner_blocks.0.0.weight"].shape) == (256, 128 * wide, 1, 1) and "fpn.inner_blocks.3.0.weight" not in part


BUILDERS = {
    "fpn": lambda M: M.FeaturePyramidNetwork([8, 16, 32], 16),
    "fpn, BatchNorm2d, P6P7": lambda M: M.FeaturePyramidNetwork([8, 16, 32], 16, extra_blocks=M.LastLevelP6P7(32, 16), norm_layer=nn.BatchNorm2d),
    "resnet18 backbone": lambda M: M.resnet_fpn_backbone(backbone_name="resnet18"),
    "resnet50 backbone, P6P7": lambda M: M.resnet_fpn_backbone(backbone_name="resnet50", returned_layers=[2, 3, 4],
                                                                extra_blocks=M.LastLevelP6P7(256, 256)),
}


class _Ours:
    FeaturePyramidNetwork, LastLevelP6P7, resnet_fpn_backbone = fpn.FeaturePyramidNetwork, fpn.LastLevelP6P7, staticmethod(backbone_utils.resnet_fpn_backbone)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_seeded_construction_consumes_the_rng_like_the_replica(name):
    torch.manual_seed(4321)
    ours = BUILDERS[name](_Ours)
    after_ours = torch.rand(4)
    torch.manual_seed(4321)
    theirs = BUILDERS[name](P)
    after_theirs = torch.rand(4)
    assert torch.equal(after_ours, after_theirs)
    for (k, a), b in zip(ours.state_dict().items(), theirs.state_dict().values()):
        assert torch.equal(a, b), k
    convs = [m for m in ours.modules() if isinstance(m, nn.Conv2d) and m.bias is not None]
    assert convs and all(float(m.bias.detach().abs().max()) == 0.0 for m in convs)  # kaiming_uniform_(a=1) and zero bias
    P.randomize(theirs, 9)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    for (k, a), b in zip(ours.state_dict().items(), theirs.state_dict().values()):
        assert torch.equal(a, b), k
    P.randomize(ours, 10)
    theirs.load_state_dict(ours.state_dict(), strict=True)


def test_version_1_state_dict_loads_through_the_key_renaming():
    torch.manual_seed(5)
    src = fpn.FeaturePyramidNetwork([8, 16], 16)
    sd = src.state_dict()
    v1 = OrderedDict((k.replace(".0.weight", ".weight").replace(".0.bias", ".bias"), v) for k, v in sd.items())
    assert "inner_blocks.0.weight" in v1 and "layer_blocks.1.bias" in v1 and "inner_blocks.0.0.weight" not in v1
    assert not hasattr(v1, "_metadata")  # no version recorded: version 1
    for cls in (fpn.FeaturePyramidNetwork, P.FeaturePyramidNetwork):
        dst = cls([8, 16], 16)
        dst.load_state_dict(OrderedDict(v1), strict=True)
        for k, v in dst.state_dict().items():
            assert torch.equal(v, sd[k]), k
    # inside a larger model too (the prefix is part of the keys)
    holder = nn.Module()
    holder.fpn = fpn.FeaturePyramidNetwork([8, 16], 16)
    holder.load_state_dict(OrderedDict(("fpn." + k, v) for k, v in v1.items()), strict=True)
    assert torch.equal(holder.fpn.inner_blocks[1][0].weight, src.inner_blocks[1][0].weight)


def _raises_like_the_replica(make):
    with pytest.raises(Exception) as theirs:
        make(P)
    with pytest.raises(type(theirs.value)) as ours:
        make(_OursAll)
    assert str(ours.value) == str(theirs.value)
    return str(ours.value)


class _OursAll(_Ours):
    ExtraFPNBlock, LastLevelMaxPool = fpn.ExtraFPNBlock, fpn.LastLevelMaxPool
    IntermediateLayerGetter, BackboneWithFPN = backbone_utils.IntermediateLayerGetter, backbone_utils.BackboneWithFPN
    R = resnet  # the replica module reaches its ResNet as P.R too


def test_constructors_refuse_what_the_replica_refuses():
    assert "in_channels=0" in _raises_like_the_replica(lambda M: M.FeaturePyramidNetwork([8, 0, 16], 16))
    assert "should be of type ExtraFPNBlock" in _raises_like_the_replica(lambda M: M.FeaturePyramidNetwork([8], 16, extra_blocks=nn.Identity()))
    assert "return_layers are not present in model" in _raises_like_the_replica(
        lambda M: M.IntermediateLayerGetter(M.R.resnet18(), {"layer1": "0", "layer9": "1"}))
    for layers in (-1, 6):
        assert "range [0,5]" in _raises_like_the_replica(lambda M: M.resnet_fpn_backbone(backbone_name="resnet18", trainable_layers=layers))
    for returned in ([0, 1], [3, 5], [-1]):
        assert "range [1,4]" in _raises_like_the_replica(lambda M: M.resnet_fpn_backbone(backbone_name="resnet18", returned_layers=returned))
    assert backbone_utils._validate_trainable_layers(True, None, 5, 3) == 3 and backbone_utils._validate_trainable_layers(True, 2, 5, 3) == 2
    with pytest.warns(UserWarning, match="has no effect"):
        assert backbone_utils._validate_trainable_layers(False, 2, 5, 3) == 5
    with pytest.raises(ValueError, match=r"range \[0,5\], got 6"):
        backbone_utils._validate_trainable_layers(True, 6, 5, 3)


def test_the_getter_refuses_children_it_cannot_run_fused():
    class Plain(nn.Module):
        def __init__(self, middle):
            super().__init__()
            self.conv1, self.bn1, self.relu = nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8), nn.ReLU()
            self.middle = middle
            self.layer1 = nn.Sequential(resnet.BasicBlock(8, 8))

    ok = backbone_utils.IntermediateLayerGetter(Plain(nn.MaxPool2d(2, 2)), {"layer1": "out"})
    assert list(ok) == ["conv1", "bn1", "relu", "middle", "layer1"] and not ok.training
    for middle, text in ((nn.Dropout(), "Dropout"), (nn.Linear(8, 8), "Linear"), (nn.Sequential(nn.Conv2d(8, 8, 1)), "Sequential"),
                         (nn.GroupNorm(2, 8), "GroupNorm")):
        with pytest.raises(NotImplementedError, match=text):
            backbone_utils.IntermediateLayerGetter(Plain(middle), {"layer1": "out"})
    with pytest.raises(NotImplementedError, match="followed|follows"):  # a conv without its norm
        backbone_utils.IntermediateLayerGetter(Plain(nn.Conv2d(8, 8, 1)), {"layer1": "out"})
    with pytest.raises(NotImplementedError, match="one launch"):  # the middle of a fused run cannot be returned
        backbone_utils.IntermediateLayerGetter(Plain(nn.MaxPool2d(2, 2)), {"bn1": "stem", "layer1": "out"})
    # a child the forward never reaches is not looked at
    m = Plain(nn.MaxPool2d(2, 2))
    m.head = nn.Linear(8, 2)
    assert list(backbone_utils.IntermediateLayerGetter(m, {"relu": "stem"})) == ["conv1", "bn1", "relu"]


def test_training_mode_raises():
    x = OrderedDict(a=torch.zeros(1, 8, 4, 4))
    with pytest.raises(RuntimeError, match="inference only"):
        fpn.FeaturePyramidNetwork([8], 8).train()(x)
    with pytest.raises(RuntimeError, match="inference only"):
        mv.resnet_fpn_backbone(backbone_name="resnet18").train()(torch.zeros(1, 3, 32, 32))


def test_the_float_source_index_is_torchs_and_not_the_integer_rule():
    """The index rule the header states, restated in numpy float32, against torch's CPU interpolate for every in <= 69, out <= 139;
    and the integer rule o * in / out differs from it (65 -> 110 among others), which is why the kernel multiplies floats."""
    differs = 0
    for n_in in range(1, 70):
        src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
        for n_out in range(1, 140):
            want = nn.functional.interpolate(src, size=(1, n_out), mode="nearest").reshape(-1).to(torch.int64).numpy()
            scale = np.float32(n_in) / np.float32(n_out)
            got = np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)
            assert np.array_equal(got, want), (n_in, n_out)
            differs += int(not np.array_equal(np.arange(n_out) * n_in // n_out, want))
    assert differs > 0
    o = np.arange(110)
    want = nn.functional.interpolate(torch.arange(65, dtype=torch.float32).reshape(1, 1, 1, 65), size=(1, 110), mode="nearest").reshape(-1).numpy()
    assert not np.array_equal(o * 65 // 110, want)
