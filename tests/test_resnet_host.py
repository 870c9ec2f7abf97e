"""ResNet without a GPU: the two new ABI entries' refusals (they return before any launch), the module tree of cpu_vision_amd.resnet
against the torch.nn replica of the reference (tests/_resnet_ref.py) -- state-dict keys and shapes, seeded parameters, strides and
dilations -- the plain-Python checks, and the oracle composition of a whole network against the replica in float64."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

from cpu_vision_amd import _lib, resnet
from cpu_vision_amd import functional as F
from cpu_vision_amd.mobilenet import FrozenBatchNorm2d
from tests import _resnet_ref as R

INVALID = -1  # MV_ERR_INVALID_ARGUMENT


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _conv(lib, x, w, y, alpha=None, beta=None, res=None, n=1, cin=4, h=6, wd=6, cout=8, k=3, stride=1, pad=1, groups=1, affine=0, act=0):
    return lib.mv_conv2d_affine_act_f32(_ptr(x), _ptr(w), None, _ptr(alpha), _ptr(beta), _ptr(res), _ptr(y), n, cin, h, wd, cout, k, k,
                                        stride, stride, pad, pad, 1, 1, groups, affine, act, None, 0, None)


def test_abi_refusals_without_a_device():
    """Host pointers are enough: every refusal comes before the first launch, with a negative status and a message."""
    lib = _lib.load()
    x, w, y = np.zeros((1, 4, 6, 6), np.float32), np.zeros((8, 4, 3, 3), np.float32), np.full((1, 8, 6, 6), -7.25, np.float32)
    a = np.ones(8, np.float32)

    def refused(rc, text):
        assert rc == INVALID and text in lib.mv_last_error().decode(), (rc, lib.mv_last_error())

    for affine in (1, 2):
        refused(_conv(lib, x, w, y, None, a, affine=affine), "affine without alpha / beta")
        refused(_conv(lib, x, w, y, a, None, affine=affine), "affine without alpha / beta")
    refused(_conv(lib, x, w, y, res=y), "must not overlap")
    refused(_conv(lib, x, w, y, res=y.reshape(-1)[4:]), "must not overlap")  # a partial overlap too
    refused(_conv(lib, x, w, x[:, :4]), "must not overlap")
    refused(_conv(lib, x, w, y, h=2, wd=2, pad=0), "output size too small")
    refused(_conv(lib, x, w, y, affine=3), "bad affine")
    refused(_conv(lib, x, w, y, act=9), "bad affine")
    refused(_conv(lib, x, w, y, groups=3), "must divide")
    assert _conv(lib, x, w, y, n=0) == 0  # empty work: a successful no-op
    assert np.all(y == -7.25)

    px, py = np.zeros((2, 5, 5), np.float32), np.full((2, 5, 5), -7.25, np.float32)
    pool = lambda h, wd, k, s, p, planes=2: lib.mv_maxpool2d_pad_f32(_ptr(px), _ptr(py), planes, h, wd, k, s, p, None)  # noqa: E731
    refused(pool(5, 5, 3, 2, 2), "pad should be at most half")
    refused(pool(5, 5, 2, 2, 2), "pad should be at most half")
    refused(pool(5, 5, 3, 2, -1), "pad should be at most half")
    refused(pool(1, 5, 4, 1, 1), "Output size is too small")  # 1 + 2 - 4 < 0
    refused(pool(5, 5, 3, 0, 1), "bad pooling shape")
    assert lib.mv_maxpool2d_pad_f32(_ptr(px), _ptr(px), 2, 5, 5, 3, 2, 1, None) == INVALID
    assert pool(5, 5, 3, 2, 1, planes=0) == 0
    assert np.all(py == -7.25)


def test_python_checks_without_a_device():
    x = torch.zeros(1, 4, 6, 6)
    with pytest.raises(Exception, match="(?i)gpu|device|cuda"):
        F.max_pool2d(x, 3, 2, padding=1)
    with pytest.raises(Exception, match="(?i)gpu|device|cuda"):
        F.conv2d_affine_act(x, torch.zeros(8, 4, 3, 3), padding=1)


BUILDERS = [("resnet18", {}), ("resnet50", {}), ("wide_resnet50_2", {})]


@pytest.mark.parametrize("name,kw", BUILDERS)
def test_state_dict_has_the_replicas_keys_and_shapes(name, kw):
    ours, theirs = getattr(resnet, name)(num_classes=10, **kw).state_dict(), getattr(R, name)(num_classes=10, **kw).state_dict()
    assert list(ours) == list(theirs)
    assert [tuple(v.shape) for v in ours.values()] == [tuple(v.shape) for v in theirs.values()]
    assert "layer1.0.conv1.weight" in ours and "fc.bias" in ours and ("layer2.0.downsample.0.weight" in ours)


def test_replica_parameter_counts():
    count = lambda m: sum(p.numel() for p in m.parameters())  # noqa: E731
    assert count(R.resnet18()) == 11689512 and count(R.resnet50()) == 25557032
    assert count(resnet.resnet18()) == 11689512 and count(resnet.resnet50()) == 25557032


@pytest.mark.parametrize("name,kw", [("resnet18", {}), ("resnet50", {"zero_init_residual": True}), ("wide_resnet50_2", {})])
def test_seeded_construction_consumes_the_rng_like_the_replica(name, kw):
    torch.manual_seed(1234)
    ours = getattr(resnet, name)(num_classes=10, **kw)
    after_ours = torch.rand(4)
    torch.manual_seed(1234)
    theirs = getattr(R, name)(num_classes=10, **kw)
    after_theirs = torch.rand(4)
    assert torch.equal(after_ours, after_theirs)
    for (k, a), b in zip(ours.state_dict().items(), theirs.state_dict().values()):
        assert torch.equal(a, b), k
    theirs.load_state_dict(ours.state_dict(), strict=True)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    if kw.get("zero_init_residual"):
        assert float(ours.layer1[0].bn3.weight.detach().abs().max()) == 0.0 and float(ours.layer1[0].bn2.weight.detach().min()) == 1.0


def test_frozen_norm_state_dict_loads_from_batchnorm():
    frozen = resnet.resnet18(num_classes=10, norm_layer=FrozenBatchNorm2d)
    frozen.load_state_dict(R.resnet18(num_classes=10).state_dict(), strict=True)  # num_batches_tracked is dropped, as in the reference
    assert isinstance(frozen.layer2[0].downsample[1], FrozenBatchNorm2d)


def test_training_mode_and_unknown_norms_raise():
    m = resnet.resnet18(num_classes=10)
    assert not m.training  # built in eval mode, like mobilenet.MobileNetV2
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m(torch.zeros(1, 3, 32, 32))
    blk = resnet.BasicBlock(8, 8)
    with pytest.raises(RuntimeError, match="inference only"):
        blk(torch.zeros(1, 8, 4, 4))
    with pytest.raises(RuntimeError, match="inference only"):
        resnet.Bottleneck(8, 2).train()(torch.zeros(1, 8, 4, 4))
    with pytest.raises(NotImplementedError, match="GroupNorm"):
        resnet.resnet18(norm_layer=lambda c: nn.GroupNorm(2, c))
    with pytest.raises(NotImplementedError, match="Identity"):
        resnet.Bottleneck(8, 2, norm_layer=lambda c: nn.Identity())
    with pytest.raises(ValueError, match="groups=1 and base_width=64"):
        resnet.BasicBlock(8, 8, groups=2)
    with pytest.raises(ValueError, match="replace_stride_with_dilation"):
        resnet.resnet50(replace_stride_with_dilation=[True])


def test_block_repr_is_the_module_tree():
    assert repr(resnet.BasicBlock(8, 8)) == repr(R.BasicBlock(8, 8))
    down = lambda mod: nn.Sequential(mod.conv1x1(8, 16, 2), nn.BatchNorm2d(16))  # noqa: E731
    assert repr(resnet.Bottleneck(8, 4, 2, down(resnet))) == repr(R.Bottleneck(8, 4, 2, down(R)))
    text = repr(resnet.BasicBlock(8, 8, norm_layer=FrozenBatchNorm2d))
    assert "(bn1): FrozenBatchNorm2d(8, eps=1e-05)" in text and "_fold" not in text


def test_replace_stride_with_dilation_gives_the_references_geometry():
    geometry = lambda m: [(k, c.stride, c.dilation, c.padding) for k, c in m.named_modules() if isinstance(c, nn.Conv2d)]  # noqa: E731
    for rswd in ([False, True, True], [True, False, True], [False, False, True]):
        ours, theirs = resnet.resnet50(num_classes=10, replace_stride_with_dilation=rswd), R.resnet50(num_classes=10, replace_stride_with_dilation=rswd)
        assert geometry(ours) == geometry(theirs)
    m = resnet.resnet50(num_classes=10, replace_stride_with_dilation=[False, True, True])
    assert m.layer3[0].conv2.stride == (1, 1) and m.layer3[0].conv2.dilation == (1, 1) and m.layer3[0].downsample[0].stride == (1, 1)
    assert m.layer3[1].conv2.dilation == (2, 2) and m.layer4[0].conv2.dilation == (2, 2) and m.layer4[1].conv2.dilation == (4, 4)
    assert m.layer4[1].conv2.padding == (4, 4)
    # the stated superset of the reference: a dilated BasicBlock (the reference raises NotImplementedError there)
    m18 = resnet.resnet18(num_classes=10, replace_stride_with_dilation=[False, False, True])
    assert m18.layer4[1].conv1.dilation == (2, 2) and m18.layer4[1].conv2.padding == (2, 2) and m18.layer4[0].conv1.stride == (1, 1)


def test_zero_stuffed_kernel_is_the_dilated_conv():
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(1, 3, 9, 8, generator=g), torch.randn(4, 3, 3, 3, generator=g)
    stuffed = torch.from_numpy(R.zero_stuffed(w.numpy(), 2))
    assert stuffed.shape == (4, 3, 5, 5)
    torch.testing.assert_close(torch.nn.functional.conv2d(x, stuffed, padding=2), torch.nn.functional.conv2d(x, w, padding=2, dilation=2),
                               rtol=1e-5, atol=1e-5)


# The oracle is one float32 chain per output in ascending (c, ky, kx) order; torch's CPU forward is float32 too, in its GEMM's
# order.  Both are compared with the replica in float64; the oracle may be off by torch-float32's own error times this margin
# (two float32 summation orders of the same sums: their errors are of one size, neither is "the" float32 answer).
MARGIN = 4.0


def test_oracle_composition_against_float64():
    torch.manual_seed(7)
    model = R.resnet18(num_classes=10).eval()
    R.randomize_norms(model, 11)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)) * 2 - 1
    with torch.no_grad():
        f32 = model(x).numpy().astype(np.float64)
        f64 = model.double()(x.double()).numpy()
        model.float()
    orc = R.oracle_resnet(model, x.numpy()).astype(np.float64)
    scale = float(np.abs(f64).max())
    err_torch, err_oracle = float(np.abs(f32 - f64).max()) / scale, float(np.abs(orc - f64).max()) / scale
    print(f"max |error| / max |logit| against float64: torch float32 {err_torch:.3e}, oracle {err_oracle:.3e}, margin {MARGIN}")
    assert err_torch > 0 and err_oracle <= MARGIN * err_torch, (err_oracle, err_torch)
