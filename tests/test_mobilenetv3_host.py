"""MobileNetV3 without a GPU: the module trees, state-dict keys, parameter counts and seeded initialisation against the torch replica
(tests/_mobilenetv3_ref.py), the argument errors, the host-side refusals of the five new ABI entries (host pointers: nothing is
launched), and the numerics of the stated squeeze-excitation gate against torch's float32 ops and a float64 evaluation."""
import numpy as np
import pytest
import torch
from torch import nn

from cpu_vision_amd import _lib
from cpu_vision_amd import functional as F
from cpu_vision_amd import ops
from cpu_vision_amd.mobilenet import SqueezeExcitation
from cpu_vision_amd.mobilenetv3 import (InvertedResidual, InvertedResidualConfig, MobileNetV3, _mobilenet_v3_conf, mobilenet_v3_large,
                                        mobilenet_v3_small)
from tests import _mobilenetv3_ref as R

BUILDERS = {"mobilenet_v3_large": mobilenet_v3_large, "mobilenet_v3_small": mobilenet_v3_small}


def _tree(m):
    return [(name, type(c).__name__.lstrip("T") if type(c).__module__ == R.__name__ else type(c).__name__) for name, c in m.named_modules()]


@pytest.mark.parametrize("arch,params,entries", [("mobilenet_v3_large", 5483032, 312), ("mobilenet_v3_small", 2542856, 244)])
def test_tree_keys_counts_and_seeded_init_equal_the_replica(arch, params, entries):
    torch.manual_seed(11)
    ours = BUILDERS[arch]()
    torch.manual_seed(11)
    theirs = R.replica(arch)
    assert _tree(ours) == _tree(theirs)
    assert sum(p.numel() for p in ours.parameters()) == params
    sd, td = ours.state_dict(), theirs.state_dict()
    assert list(sd) == list(td) and len(sd) == entries
    for k in sd:
        assert torch.equal(sd[k], td[k]), k
    R.perturb(theirs, 3)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    assert not ours.training
    for blk, want in zip(ours.features[1:-1], theirs.features[1:-1]):
        assert (blk.use_res_connect, blk.out_channels, blk._is_cn) == (want.use_res_connect, want.out_channels, want._is_cn)


def test_se_shapes_and_block_children():
    shapes = lambda m: [(b.fc1.in_channels, b.fc1.out_channels) for b in m.modules() if isinstance(b, SqueezeExcitation)]  # noqa: E731
    assert shapes(mobilenet_v3_large()) == [(72, 24), (120, 32), (120, 32), (480, 120), (672, 168), (672, 168), (960, 240), (960, 240)]
    assert shapes(mobilenet_v3_small()) == [(16, 8), (96, 24), (240, 64), (240, 64), (120, 32), (144, 40), (288, 72), (576, 144), (576, 144)]
    se = SqueezeExcitation(16, 8)
    assert [n for n, _ in se.named_children()] == ["avgpool", "fc1", "fc2", "activation", "scale_activation"]
    assert ops.SqueezeExcitation is SqueezeExcitation
    blk = mobilenet_v3_large().features[4]  # 24 -> 72 -> 40, 5x5 stride 2, SE
    assert [type(c).__name__ for c in blk.block] == ["Conv2dNormActivation", "Conv2dNormActivation", "SqueezeExcitation", "Conv2dNormActivation"]
    assert blk.block[1][0].kernel_size == (5, 5) and blk.block[1][0].stride == (2, 2) and type(blk.block[2].scale_activation) is nn.Hardsigmoid
    assert type(mobilenet_v3_large().features[1].block[0][2]) is nn.ReLU and len(mobilenet_v3_large().features[1].block) == 2


@pytest.mark.parametrize("arch", list(BUILDERS))
def test_width_mult_and_reduced_tail_channels(arch):
    for kw in (dict(width_mult=0.75), dict(reduced_tail=True), dict(width_mult=0.75, reduced_tail=True, dilated=True)):
        torch.manual_seed(2)
        ours = BUILDERS[arch](num_classes=5, **kw)
        torch.manual_seed(2)
        theirs = R.replica(arch, num_classes=5, **kw)
        assert [(k, tuple(v.shape)) for k, v in ours.state_dict().items()] == [(k, tuple(v.shape)) for k, v in theirs.state_dict().items()]
        convs = lambda m: [(c.kernel_size, c.stride, c.padding, c.dilation, c.groups) for c in m.modules() if isinstance(c, nn.Conv2d)]  # noqa: E731
        assert convs(ours) == convs(theirs)
    setting, last = _mobilenet_v3_conf(arch, width_mult=0.75)
    assert last == InvertedResidualConfig.adjust_channels(1280 if arch.endswith("large") else 1024, 0.75)
    setting, last = _mobilenet_v3_conf(arch, reduced_tail=True)
    assert (setting[-1].out_channels, last) == ((80, 640) if arch.endswith("large") else (48, 512))


def test_argument_errors():
    with pytest.raises(ValueError, match="Unsupported model type mobilenet_v3_tiny"):
        _mobilenet_v3_conf("mobilenet_v3_tiny")
    with pytest.raises(ValueError, match="The inverted_residual_setting should not be empty"):
        MobileNetV3([], 1280)
    with pytest.raises(TypeError, match=r"The inverted_residual_setting should be List\[InvertedResidualConfig\]"):
        MobileNetV3([[16, 3, 16, 16]], 1280)
    with pytest.raises(ValueError, match="illegal stride value"):
        InvertedResidual(InvertedResidualConfig(16, 3, 16, 16, False, "RE", 3, 1, 1.0), nn.BatchNorm2d)
    with pytest.raises(NotImplementedError):
        SqueezeExcitation(16, 8, activation=nn.SiLU)
    with pytest.raises(NotImplementedError):
        SqueezeExcitation(16, 8, scale_activation=nn.Tanh)
    assert InvertedResidualConfig.adjust_channels(100, 0.75) == 72 and InvertedResidualConfig(16, 3, 16, 16, False, "HS", 1, 1, 1.0).use_hs
    m = mobilenet_v3_small(num_classes=3)
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()(torch.zeros(1, 3, 32, 32))
    with pytest.raises(_lib.Mi355VisionError):  # no CPU fallback
        m.eval()(torch.zeros(1, 3, 32, 32))


def test_functional_argument_errors():
    x = torch.zeros(2, 8, 4, 4)
    with pytest.raises(ValueError, match="unknown activation"):
        F.linear_act(torch.zeros(2, 8), torch.zeros(3, 8), None, "tanh")
    with pytest.raises(RuntimeError, match="cannot be multiplied"):
        F.linear_act(torch.zeros(2, 8), torch.zeros(3, 7))
    with pytest.raises(RuntimeError, match="bias should have shape"):
        F.linear_act(torch.zeros(2, 8), torch.zeros(3, 8), torch.zeros(4))
    with pytest.raises(TypeError):
        F.global_avg_pool(x.double())
    with pytest.raises(RuntimeError):
        F.global_avg_pool(x[0])
    with pytest.raises(RuntimeError, match="gate should have shape"):
        F.se_scale(x, torch.zeros(2, 7))
    with pytest.raises(ValueError, match="out is x itself"):
        F.se_scale(x, torch.zeros(2, 8), out=torch.zeros(2, 8, 4, 4))
    for call in (lambda: F.global_avg_pool(x), lambda: F.se_scale(x, torch.zeros(2, 8)), lambda: F.linear_act(torch.zeros(2, 8), torch.zeros(3, 8)),
                 lambda: F.conv_norm_act(x, torch.zeros(8, 1, 5, 5), groups=8)):
        with pytest.raises(_lib.Mi355VisionError):  # no CPU fallback
            call()


def _refused(rc, text, code=-1):
    msg = _lib.load().mv_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_abi_refusals_without_a_device():
    """Every call is refused (or is the n == 0 no-op) before a launch: the pointers are host integers that are never dereferenced."""
    lib = _lib.load()
    X, W, Y, G = 1 << 40, 2 << 40, 3 << 40, 4 << 40  # far enough apart for every shape below
    dw = lambda **o: lib.mv_dwconv_norm_act_f32(*[{**dict(x=X, w=W, b=None, al=None, be=None, r=None, y=Y, n=1, c=4, h=6, wd=6, k=5, s=1, af=0, act=0), **o}[k]  # noqa: E731
                                                  for k in ("x", "w", "b", "al", "be", "r", "y", "n", "c", "h", "wd", "k", "s", "af", "act")], None)
    _refused(dw(k=7), "kernel 3 or 5", -2)
    _refused(dw(k=4), "kernel 3 or 5", -2)
    _refused(dw(k=1), "kernel 3 or 5", -2)
    _refused(dw(n=-1), "bad conv shape")
    _refused(dw(c=0), "bad conv shape")
    _refused(dw(s=3), "stride should be 1 or 2")
    _refused(dw(act=5), "activation")
    _refused(dw(af=3), "affine")
    _refused(dw(x=None), "null pointer")
    _refused(dw(y=None), "null pointer")
    _refused(dw(af=2), "affine without alpha / beta")
    _refused(dw(y=X), "alias")
    _refused(dw(k=3, s=3), "stride should be 1 or 2")  # k = 3 is mv_conv_norm_act_f32's own refusal
    _refused(dw(k=3, x=None), "null pointer")
    assert dw(n=0) == 0 and dw(n=0, k=3) == 0 and dw(n=0, x=None, y=None) == 0

    sc = lambda **o: lib.mv_conv1x1_scaled_f32(*[{**dict(x=X, g=G, w=W, b=None, al=None, be=None, r=None, y=Y, n=1, ci=4, h=6, wd=6, co=5, af=0, act=0), **o}[k]  # noqa: E731
                                                 for k in ("x", "g", "w", "b", "al", "be", "r", "y", "n", "ci", "h", "wd", "co", "af", "act")], None)
    _refused(sc(g=None), "null pointer")
    _refused(sc(w=None), "null pointer")
    _refused(sc(co=0), "bad conv shape")
    _refused(sc(act=7), "activation")
    _refused(sc(af=1), "affine without alpha / beta")
    _refused(sc(y=X + 16), "must not overlap")
    _refused(sc(y=G), "must not overlap")
    _refused(sc(r=Y + 4), "must not overlap")
    _refused(sc(n=65536), "too large", -2)
    assert sc(n=0) == 0

    pool = lambda **o: lib.mv_global_avgpool_f64sum_f32(*[{**dict(x=X, y=Y, n=2, c=3, h=4, wd=5, xs=60), **o}[k] for k in ("x", "y", "n", "c", "h", "wd", "xs")], None)  # noqa: E731
    _refused(pool(xs=59), "image stride")
    _refused(pool(h=0), "bad shape")
    _refused(pool(n=-2), "bad shape")
    _refused(pool(x=None), "null pointer")
    _refused(pool(x=X + 2), "4-byte aligned")
    _refused(pool(y=X + 8), "must not overlap")
    _refused(pool(h=65536, wd=65536, xs=2 ** 40), "32-bit index", -2)
    assert pool(n=0) == 0

    lin = lambda **o: lib.mv_linear_act_f32(*[{**dict(x=X, w=W, b=None, y=Y, n=2, k=8, m=3, act=0), **o}[k] for k in ("x", "w", "b", "y", "n", "k", "m", "act")], None)  # noqa: E731
    _refused(lin(act=2), "activation code")  # ReLU6 is not a linear_act activation
    _refused(lin(act=4), "activation code")
    _refused(lin(act=7), "activation code")
    _refused(lin(k=0), "bad linear shape")
    _refused(lin(w=None), "null pointer")
    _refused(lin(y=X), "must not overlap")
    _refused(lin(b=Y + 4), "must not overlap")
    _refused(lin(n=65536), "launch grid", -2)
    assert lin(n=0) == 0

    scale = lambda **o: lib.mv_se_scale_f32(*[{**dict(x=X, g=G, y=Y, n=2, c=3, h=4, wd=5), **o}[k] for k in ("x", "g", "y", "n", "c", "h", "wd")], None)  # noqa: E731
    _refused(scale(g=None), "null pointer")
    _refused(scale(c=0), "bad shape")
    _refused(scale(y=X + 4), "y must be x itself")
    _refused(scale(y=G), "must not overlap gate")
    _refused(scale(y=Y + 1), "4-byte aligned")
    _refused(scale(h=65536, wd=65536), "32-bit index", -2)
    assert scale(n=0) == 0


def test_restatements_on_small_hand_cases():
    """The restated orders against direct float64 evaluations on inputs where every order gives the same float32 (small integers)."""
    x = np.arange(2 * 3 * 5 * 7, dtype=np.float32).reshape(2, 3, 5, 7) % 13 - 6
    np.testing.assert_array_equal(R.global_avg_pool(x), (x.astype(np.float64).mean((2, 3))).astype(np.float32))
    w = (np.arange(4 * 70, dtype=np.float32).reshape(4, 70) % 7) - 3
    a = (np.arange(3 * 70, dtype=np.float32).reshape(3, 70) % 5) - 2
    b = np.array([0.5, -1.0, 2.0, 100.0], np.float32)
    np.testing.assert_array_equal(R.linear_act(a, w, b), (a.astype(np.float64) @ w.astype(np.float64).T + b).astype(np.float32))
    v = torch.tensor([-np.inf, -4.0, -3.0, -1.5, -0.0, 0.0, 0.7, 3.0, 5.0, np.inf, np.nan], dtype=torch.float32)
    for name, fn in (("relu", torch.relu), ("hardswish", nn.functional.hardswish), ("hardsigmoid", nn.functional.hardsigmoid)):
        R.same(R.ACTIVATIONS[name](v.numpy()), fn(v).numpy(), name)
    s, t = R.act_sigmoid(v.numpy()), torch.sigmoid(v).numpy()
    assert np.isnan(s[-1]) and s[0] == 0 and s[-2] == 1 and np.abs(s[:-1].astype(np.float64) - t[:-1]).max() <= 2.0 ** -23
    g = torch.Generator().manual_seed(8)
    big = torch.randn(100000, generator=g) * 4
    R.same(R.act_hardswish(big.numpy()), nn.functional.hardswish(big).numpy(), "hardswish on 1e5 values")
    R.same(R.act_hardsigmoid(big.numpy()), nn.functional.hardsigmoid(big).numpy(), "hardsigmoid on 1e5 values")


GATE_CASES = [(72, 24, 28), (960, 240, 7), (16, 8, 56), (3, 8, 1), (130, 40, 5)]


@pytest.mark.parametrize("c,sq,side", GATE_CASES)
def test_gate_restatement_is_at_least_as_accurate_as_torch(c, sq, side):
    """The project's condition: max |restatement - f64| <= 2 max |torch f32 - f64| + 2^-22 max |f64|, with at least 40 % of the gate
    strictly inside (0, 1) so that the clamp does not hide the sums.  Measured with these seeds (restatement / torch float32 in units of
    2^-24 max|f64|, share inside): (72, 24, 28) 1.17 / 2.85, 94 %; (960, 240, 7) 2.21 / 17.66, 46 %; (16, 8, 56) 1.48 / 1.48, 100 %;
    (3, 8, 1) 1.10 / 0.75, 100 %; (130, 40, 5) 1.25 / 6.14, 86 %."""
    g = torch.Generator().manual_seed(1000 + c)
    se = R.TSqueezeExcitation(c, sq, scale_activation=nn.Hardsigmoid)
    with torch.no_grad():
        for conv in (se.fc1, se.fc2):
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.3)
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=g))
    x = torch.randn((2, c, side, side), generator=g)
    with torch.no_grad():
        t32 = se._scale(x).reshape(2, c)
        f64 = se.double()._scale(x.double()).reshape(2, c)
    se.float()
    got = torch.from_numpy(R.se_gate_of(se, x.numpy()))
    scale = float(f64.abs().max())
    e_re, e_t = float((got.double() - f64).abs().max()), float((t32.double() - f64).abs().max())
    inside = float(((f64 > 0) & (f64 < 1)).double().mean())
    print(f"gate ({c}, {sq}, {side}): restatement {e_re / scale * 2 ** 24:.2f}, torch {e_t / scale * 2 ** 24:.2f} (x 2^-24 max|f64|), "
          f"{inside * 100:.0f} % inside (0, 1)")
    assert inside >= 0.40
    assert e_re <= 2 * e_t + 2.0 ** -22 * scale
