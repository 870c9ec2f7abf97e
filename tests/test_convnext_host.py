"""ConvNeXt without a GPU: the module trees, state-dict keys, parameter counts and seeded initialisation against the torch replica
(tests/_convnext_ref.py), the argument errors, the host-side refusals of the four new ABI entries (host pointers: nothing is
launched), the restated LayerNorm and GELU against torch's float32 ops and a float64 evaluation, the distance of every GELU argument
of the GPU tests from a float32 rounding tie of erf, and the reach of the GPU tests' shape lists."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from cpu_vision_amd import _lib
from cpu_vision_amd import functional as F
from cpu_vision_amd import ops
from cpu_vision_amd.convnext import (CNBlock, CNBlockConfig, ConvNeXt, LayerNorm2d, Permute, StochasticDepth, convnext_base, convnext_large,
                                     convnext_small, convnext_tiny)
from tests import _convnext_ref as R

BUILDERS = {"convnext_tiny": convnext_tiny, "convnext_small": convnext_small, "convnext_base": convnext_base, "convnext_large": convnext_large}


def _tree(m):
    return [(name, type(c).__name__.lstrip("T") if type(c).__module__ == R.__name__ else type(c).__name__.lstrip("_")) for name, c in m.named_modules()]


def _same_tree(ours, theirs):
    """The same names in the same order, the same class for every module the reference names (the stem and the downsample pairs are
    nn.Sequential subclasses here and plain nn.Sequential in the replica, as Conv2dNormActivation is one in the reference)."""
    a, b = _tree(ours), _tree(theirs)
    assert [n for n, _ in a] == [n for n, _ in b]
    for (name, ca), (_, cb) in zip(a, b):
        assert ca == cb or {ca, cb} <= {"Sequential", "Stem", "Downsample"}, (name, ca, cb)


def test_tree_keys_counts_and_seeded_init_equal_the_replica():
    torch.manual_seed(11)
    ours = convnext_tiny()
    torch.manual_seed(11)
    theirs = R.replica("convnext_tiny")
    _same_tree(ours, theirs)
    assert sum(p.numel() for p in ours.parameters()) == 28589128  # the reference's documented parameter count
    sd, td = ours.state_dict(), theirs.state_dict()
    assert list(sd) == list(td)
    for k in ("features.1.0.layer_scale", "features.1.0.block.0.weight", "features.1.0.block.2.weight", "features.1.0.block.3.weight",
              "features.1.0.block.5.bias", "features.2.0.weight", "features.2.1.weight", "features.0.0.weight", "features.0.1.bias",
              "classifier.0.weight", "classifier.2.weight"):
        assert k in sd, k
    for k in sd:
        assert torch.equal(sd[k], td[k]), k
    assert float(sd["features.1.0.layer_scale"].unique()) == float(np.float32(1e-6)) and tuple(sd["features.1.0.layer_scale"].shape) == (96, 1, 1)
    R.perturb(theirs, 3)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    assert not ours.training
    probs = [b.stochastic_depth.p for stage in ours.features for b in stage if isinstance(b, CNBlock)]
    assert len(probs) == 18 and probs[0] == 0.0 and probs[-1] == pytest.approx(0.1) and probs == sorted(probs)
    assert probs == [b.stochastic_depth.p for stage in theirs.features for b in stage if isinstance(b, R.TCNBlock)]


def test_custom_block_setting_equals_the_replica():
    torch.manual_seed(5)
    ours = ConvNeXt([CNBlockConfig(*r) for r in R.NET_ROWS], stochastic_depth_prob=0.3, layer_scale=0.5, num_classes=7)
    torch.manual_seed(5)
    theirs = R.replica(R.NET_ROWS, stochastic_depth_prob=0.3, layer_scale=0.5, num_classes=7)
    _same_tree(ours, theirs)
    sd, td = ours.state_dict(), theirs.state_dict()
    assert list(sd) == list(td)
    for k in sd:
        assert torch.equal(sd[k], td[k]), k
    assert [type(m).__name__ for m in ours.features] == ["_Stem", "Sequential", "_Downsample", "Sequential", "_Downsample", "Sequential"]
    assert [len(m) for m in ours.features] == [2, 1, 2, 2, 2, 1]
    assert ours.classifier[2].in_features == 24 and isinstance(ours.classifier[0], LayerNorm2d) and ours.classifier[0].eps == 1e-6
    assert [n for n, _ in ours.named_buffers()] == [n for n, _ in theirs.named_buffers()] == []
    assert repr(CNBlockConfig(8, None, 2)) == "CNBlockConfig(input_channels=8, out_channels=None, num_layers=2)"


@pytest.mark.parametrize("arch,params", [("convnext_small", 50223688), ("convnext_base", 88591464), ("convnext_large", 197767336)])
def test_the_other_builders_have_the_references_shapes(arch, params):
    rows, sd_prob = R.SETTINGS[arch]
    torch.manual_seed(1)
    ours = BUILDERS[arch]()
    assert sum(p.numel() for p in ours.parameters()) == params
    blocks = [b for stage in ours.features for b in stage if isinstance(b, CNBlock)]
    assert len(blocks) == sum(r[2] for r in rows) and blocks[-1].stochastic_depth.p == pytest.approx(sd_prob)
    assert [s[0].block[0].out_channels for s in ours.features if isinstance(s[0], CNBlock)] == [r[0] for r in rows]


def test_argument_errors_and_the_small_modules():
    with pytest.raises(ValueError, match="The block_setting should not be empty"):
        ConvNeXt([])
    with pytest.raises(TypeError, match=r"The block_setting should be List\[CNBlockConfig\]"):
        ConvNeXt([(8, 16, 1)])
    with pytest.raises(ValueError, match="drop probability has to be between 0 and 1"):
        StochasticDepth(1.5, "row")(torch.zeros(2, 3))
    with pytest.raises(ValueError, match="mode has to be either 'batch' or 'row'"):
        StochasticDepth(0.5, "col")(torch.zeros(2, 3))
    assert ops.StochasticDepth is StochasticDepth and ops.Permute is Permute
    x = torch.arange(24.0).view(2, 3, 4)
    sd = StochasticDepth(0.5, "row")
    assert sd.eval()(x) is x and StochasticDepth(0.0, "row").train()(x) is x and repr(sd) == "StochasticDepth(p=0.5, mode=row)"
    torch.manual_seed(0)
    out = sd.train()(torch.ones(64, 3))
    assert set(out.unique().tolist()) == {0.0, 2.0} and bool((out == out[:, :1]).all())  # whole rows, scaled by 1 / survival
    assert bool((StochasticDepth(1.0, "batch").train()(x) == 0).all())
    assert torch.equal(Permute([0, 2, 1])(x), x.permute(0, 2, 1))
    m = ConvNeXt([CNBlockConfig(*r) for r in R.NET_ROWS], num_classes=3)
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="inference only"):
        CNBlock(8, 1e-6, 0.0)(torch.zeros(1, 8, 4, 4))
    with pytest.raises(_lib.Mi355VisionError):  # no CPU fallback
        m.eval()(torch.zeros(1, 3, 32, 32))
    with pytest.raises(_lib.Mi355VisionError):
        LayerNorm2d(8)(torch.zeros(1, 8, 4, 4))


def test_functional_argument_errors():
    x = torch.zeros(2, 8, 4, 4)
    with pytest.raises(RuntimeError, match=r"weight should have shape \(8, 1, 7, 7\)"):
        F.dwconv7x7(x, torch.zeros(8, 1, 5, 5))
    with pytest.raises(RuntimeError, match="bias should have shape"):
        F.dwconv7x7(x, torch.zeros(8, 1, 7, 7), torch.zeros(7))
    with pytest.raises(TypeError):
        F.dwconv7x7(x.double(), torch.zeros(8, 1, 7, 7))
    with pytest.raises(RuntimeError, match="4-D"):
        F.layer_norm2d(x[0])
    with pytest.raises(TypeError):
        F.layer_norm2d(x.half())
    with pytest.raises(RuntimeError, match=r"weight should have shape \(8,\)"):
        F.layer_norm2d(x, torch.zeros(7))
    with pytest.raises(RuntimeError, match=r"bias should have shape \(8,\)"):
        F.layer_norm2d(x, None, torch.zeros(8, 1))
    for eps in (-1e-6, math.nan, math.inf):
        with pytest.raises(ValueError, match="eps must be non-negative and finite"):
            F.layer_norm2d(x, eps=eps)
        with pytest.raises(ValueError, match="eps must be non-negative and finite"):
            F.layer_norm2d_stats(x, eps)
    with pytest.raises(RuntimeError, match="no channels"):
        F.layer_norm2d_stats(torch.zeros(2, 0, 4, 4))
    w = torch.zeros(5, 8)
    with pytest.raises(RuntimeError, match="weight should have shape"):
        F.conv1x1_gelu(x, torch.zeros(5, 7))
    with pytest.raises(RuntimeError, match="weight should have shape"):
        F.conv1x1_gelu(x, torch.zeros(5, 8, 3, 3))
    with pytest.raises(RuntimeError, match="bias should have shape"):
        F.conv1x1_gelu(x, w, torch.zeros(8))
    with pytest.raises(ValueError, match="norm is"):
        F.conv1x1_gelu(x, w, norm=(torch.zeros(2, 4, 4),))
    with pytest.raises(RuntimeError, match="mean should have shape"):
        F.conv1x1_gelu(x, w, norm=(torch.zeros(2, 4), torch.zeros(2, 4, 4), None, None))
    with pytest.raises(RuntimeError, match="rstd should have shape"):
        F.conv1x1_gelu(x, w, norm=(torch.zeros(2, 4, 4), None, None, None))
    with pytest.raises(RuntimeError, match="ln_weight should have shape"):
        F.conv1x1_gelu(x, w, norm=(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), torch.zeros(5), None))
    with pytest.raises(TypeError):
        F.conv1x1_gelu(x, w.double())
    stats = (torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), None, None)
    for call in (lambda: F.dwconv7x7(x, torch.zeros(8, 1, 7, 7)), lambda: F.layer_norm2d(x), lambda: F.layer_norm2d_stats(x),
                 lambda: F.conv1x1_gelu(x, w), lambda: F.conv1x1_gelu(x, w.view(5, 8, 1, 1), norm=stats, gelu=False)):
        with pytest.raises(_lib.Mi355VisionError):  # no CPU fallback
            call()
    # the existing surface: GELU is no activation code of the other entry points (their refusal of 7x7 weights needs a device:
    # tests/test_gpu_convnext.py)
    assert "gelu" not in F._ACT_CODES and max(F._ACT_CODES.values()) == 4
    with pytest.raises(ValueError, match="unknown activation"):
        F.conv1x1_upsample_add(x, torch.zeros(5, 8, 1, 1), top=x, activation="gelu")


def _refused(rc, text, code=-1):
    msg = _lib.load().mv_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_abi_refusals_without_a_device():
    """Every call is refused (or is the empty no-op) before a launch: the pointers are host integers that are never dereferenced."""
    lib = _lib.load()
    X, W, Y, M, S, B = 1 << 40, 2 << 40, 3 << 40, 4 << 40, 5 << 40, 6 << 40  # far enough apart for every shape below
    dw = lambda **o: lib.mv_dwconv7x7_bias_f32(*[{**dict(x=X, w=W, b=None, y=Y, n=1, c=4, h=6, wd=6), **o}[k]  # noqa: E731
                                                 for k in ("x", "w", "b", "y", "n", "c", "h", "wd")], None)
    _refused(dw(n=-1), "negative size")
    _refused(dw(h=-3), "negative size")
    _refused(dw(x=None), "null pointer")
    _refused(dw(w=None), "null pointer")
    _refused(dw(y=None), "null pointer")
    _refused(dw(y=X), "must not overlap")
    _refused(dw(y=X + 64), "must not overlap")
    _refused(dw(y=W + 4), "must not overlap")
    _refused(dw(b=Y + 8), "must not overlap")
    _refused(dw(x=X + 2), "4-byte aligned")
    _refused(dw(h=65536, wd=65536), "32-bit index", -2)
    _refused(dw(n=1 << 40, h=64, wd=64), "launch grid", -2)
    assert dw(n=0) == 0 and dw(c=0, x=None) == 0 and dw(h=0, y=None) == 0

    st = lambda **o: lib.mv_layer_norm2d_stats_f32(*[{**dict(x=X, m=M, s=S, n=2, c=3, h=4, wd=5, eps=1e-6), **o}[k]  # noqa: E731
                                                     for k in ("x", "m", "s", "n", "c", "h", "wd", "eps")], None)
    _refused(st(c=-1), "negative size")
    _refused(st(eps=-1.0), "eps must be non-negative")
    _refused(st(eps=math.nan), "eps must be non-negative")
    _refused(st(eps=1e39), "eps must be non-negative")
    _refused(st(c=0), "no channels")
    _refused(st(x=None), "null pointer")
    _refused(st(m=None), "null pointer")
    _refused(st(s=None), "null pointer")
    _refused(st(m=X + 8), "must not overlap")
    _refused(st(s=M + 4), "must not overlap")
    _refused(st(s=S + 1), "4-byte aligned")
    _refused(st(c=70000, h=256, wd=256), "32-bit index", -2)
    assert st(n=0) == 0 and st(h=0, x=None) == 0 and st(eps=0.0, n=0) == 0

    ln = lambda **o: lib.mv_layer_norm2d_f32(*[{**dict(x=X, w=None, b=None, y=Y, n=2, c=3, h=4, wd=5, eps=1e-6), **o}[k]  # noqa: E731
                                               for k in ("x", "w", "b", "y", "n", "c", "h", "wd", "eps")], None)
    _refused(ln(n=-2), "negative size")
    _refused(ln(eps=-1e-9), "eps must be non-negative")
    _refused(ln(c=0), "no channels")
    _refused(ln(x=None), "null pointer")
    _refused(ln(y=None), "null pointer")
    _refused(ln(y=X), "must not overlap")
    _refused(ln(w=Y + 4), "must not overlap")
    _refused(ln(b=Y + 4 * 119), "must not overlap")
    _refused(ln(w=W + 3), "4-byte aligned")
    _refused(ln(n=1 << 33, c=1, h=1, wd=1), "launch grid", -2)
    assert ln(n=0) == 0 and ln(wd=0, y=None) == 0

    pw = lambda **o: lib.mv_conv1x1_ln_gelu_f32(*[{**dict(x=X, m=None, s=None, lw=None, lb=None, w=W, b=None, y=Y, n=1, ci=4, h=6, wd=6, co=5, g=1), **o}[k]  # noqa: E731
                                                  for k in ("x", "m", "s", "lw", "lb", "w", "b", "y", "n", "ci", "h", "wd", "co", "g")], None)
    _refused(pw(ci=0), "bad conv shape")
    _refused(pw(co=0), "bad conv shape")
    _refused(pw(n=-1), "bad conv shape")
    _refused(pw(g=2), "gelu should be 0 or 1")
    _refused(pw(g=7), "gelu should be 0 or 1")
    _refused(pw(m=M), "mean and rstd come together")
    _refused(pw(s=S), "mean and rstd come together")
    _refused(pw(lw=B), "LayerNorm terms without mean and rstd")
    _refused(pw(lb=B), "LayerNorm terms without mean and rstd")
    _refused(pw(x=None), "null pointer")
    _refused(pw(w=None), "null pointer")
    _refused(pw(y=None), "null pointer")
    _refused(pw(y=X + 16), "must not overlap")
    _refused(pw(y=W), "must not overlap")
    _refused(pw(b=Y + 4), "must not overlap")
    _refused(pw(m=M, s=Y + 8), "must not overlap")
    _refused(pw(m=Y, s=S), "must not overlap")
    _refused(pw(m=M, s=S, lw=Y + 12), "must not overlap")
    _refused(pw(m=M, s=S, lb=Y), "must not overlap")
    _refused(pw(x=X + 2), "4-byte aligned")
    _refused(pw(w=W + 1), "4-byte aligned")
    _refused(pw(m=M + 2, s=S), "4-byte aligned")
    _refused(pw(b=B + 3), "4-byte aligned")
    _refused(pw(n=65536), "too large", -2)
    assert pw(n=0) == 0 and pw(h=0, x=None) == 0 and pw(n=0, m=M, s=S, lw=B) == 0


# ------------------------------------------------------------------------------------------------------------- the restatements
def test_layer_norm_restatement_on_hand_cases():
    """Small integers, where every summation order gives the same float64 sums."""
    x = (np.arange(2 * 5 * 3 * 4, dtype=np.float32).reshape(2, 5, 3, 4) * 7 % 11) - 5
    mean, rstd = R.layer_norm2d_stats(x, 1e-6)
    xd = x.astype(np.float64)
    m, v = xd.mean(1), xd.var(1)
    np.testing.assert_array_equal(mean, m.astype(np.float32))
    np.testing.assert_allclose(rstd.astype(np.float64), 1 / np.sqrt(v + np.float64(np.float32(1e-6))), rtol=2.0 ** -23, atol=0)
    one = R.layer_norm2d_stats(np.full((1, 1, 2, 2), 3.5, np.float32), 1e-6)
    assert (one[0] == 3.5).all() and (one[1] == np.float32(1 / math.sqrt(np.float64(np.float32(1e-6))))).all()
    mean0, rstd0 = R.layer_norm2d_stats(np.full((1, 4, 1, 1), 2.0, np.float32), 0.0)
    assert mean0[0, 0, 0] == 2 and np.isinf(rstd0[0, 0, 0])
    assert np.isnan(R.layer_norm2d(np.full((1, 4, 1, 1), 2.0, np.float32), eps=0.0)).all()  # 0 * inf


@pytest.mark.parametrize("c,offset", [(1, 0.0), (2, 0.0), (63, 0.5), (96, 0.0), (257, 3.0), (768, -1.0)])
def test_layer_norm_restatement_against_float64_and_torch(c, offset):
    """|restatement - f64| stays within the bound the four float32 roundings give.  With u = 2^-24, m and r the exact mean and rstd,
    A = |x - m| r and M = |m| r: mean rounds to float32 (u |m|), the subtraction rounds (u |x - mean|): u (M + A) after scaling by r;
    rstd's rounding and the product's add 2 u A; the product with w adds u |w| A on |w| times that; the sum with b adds u |y|.  In all
    u (|w| (M + 4 A) + |y|), with (1 + 2^-20) for the second-order terms and 2^-45 max|y| for the float64 evaluation itself.  And the
    restatement is at least as accurate as torch's float32 layer_norm on the same inputs: its largest error is no larger.  Both errors
    are printed."""
    g = torch.Generator().manual_seed(900 + c)
    x = torch.randn((2, c, 5, 7), generator=g) + offset
    w, b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    eps = 1e-6
    xd = x.double().permute(0, 2, 3, 1)
    f64 = nn.functional.layer_norm(xd, (c,), w.double(), b.double(), eps).permute(0, 3, 1, 2)
    t32 = nn.functional.layer_norm(x.permute(0, 2, 3, 1), (c,), w, b, eps).permute(0, 3, 1, 2)
    got = torch.from_numpy(R.layer_norm2d(x.numpy(), w.numpy(), b.numpy(), eps)).double()
    m = x.double().mean(1, keepdim=True)
    r = 1 / torch.sqrt(x.double().var(1, unbiased=False, keepdim=True) + eps)
    a, mm = (x.double() - m).abs() * r, m.abs() * r
    u = 2.0 ** -24
    bound = (1 + 2.0 ** -20) * u * (w.double().abs().view(1, c, 1, 1) * (mm + 4 * a) + f64.abs()) + 2.0 ** -45 * float(f64.abs().max())
    err = (got - f64).abs()
    scale = float(f64.abs().max())
    e_re, e_t = float(err.max()), float((t32.double() - f64).abs().max())
    print(f"layer_norm c={c}: restatement {e_re / scale * 2 ** 24:.2f}, torch float32 {e_t / scale * 2 ** 24:.2f} (x 2^-24 max|f64|); "
          f"largest share of the bound {float((err / bound).max()):.2f}")
    assert bool((err <= bound).all())
    assert e_re <= e_t + 2.0 ** -45 * scale  # at least as accurate as torch's float32 result; the slack is the float64 evaluation's own


def test_gelu_restatement_against_float64_and_torch():
    g = torch.Generator().manual_seed(77)
    v = torch.cat([torch.randn(200000, generator=g) * 2, torch.linspace(-9, 9, 4001), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 50.0, -50.0])])
    f64 = nn.functional.gelu(v.double())
    t32 = nn.functional.gelu(v)
    got = torch.from_numpy(R.gelu(v.numpy())).double()
    scale = float(f64.abs().max())
    e_re, e_t = float((got - f64).abs().max()), float((t32.double() - f64).abs().max())
    # the bound of the formula's roundings, u = 2^-24, h = 0.5 v (exact), E = erf(t): t's rounding moves E by at most |t| erf'(t) u, E's own
    # by u |E|, fl(1 + E) by u |1 + E|, the product by u |y|: |error| <= u (|h| (|t| erf'(t) + |E| + |1 + E|) + |y|); 1e-45 covers a
    # subnormal float32 product.  (For v < 0 the sum 1 + E cancels: the bound is absolute, not relative.)
    vd = v.double()
    t = vd * float(R.INV_SQRT2)
    e = torch.erf(t)
    bound = (1 + 2.0 ** -20) * 2.0 ** -24 * ((0.5 * vd).abs() * (t.abs() * 2 / math.sqrt(math.pi) * torch.exp(-t * t) + e.abs() + (1 + e).abs())
                                             + f64.abs()) + 1e-45
    err = (got - f64).abs()
    print(f"gelu: restatement {e_re / scale * 2 ** 24:.3f}, torch float32 {e_t / scale * 2 ** 24:.3f} (x 2^-24 max|f64|); largest share of "
          f"the bound {float((err / bound).max()):.2f}")
    assert e_re <= e_t + 2.0 ** -45 * scale  # at least as accurate as torch's float32 gelu; the slack is the float64 evaluation's own
    assert bool((err <= bound).all())
    sp = R.gelu(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32))
    assert np.isnan(sp[0]) and sp[1] == np.inf and np.isnan(sp[2]) and sp[3] == 0 and sp[4] == 0 and np.signbit(sp[4])
    assert torch.isnan(nn.functional.gelu(torch.tensor([-np.inf]))).all()  # the formula's -inf * 0, here as in torch


def test_erf_libraries_agree_and_the_margin_on_normal_values():
    """math.erf and torch.erf in float64 differ by at most an ulp and in no float32 bit on 4 x 10^5 normal(0, 2) values, and erf stays
    at least 8 float64 ulps from a float32 rounding midpoint there."""
    g = torch.Generator().manual_seed(12)
    t = (torch.randn(400000, generator=g) * 2).numpy()
    a = np.array([math.erf(float(v)) for v in t.astype(np.float64)])
    b = torch.erf(torch.from_numpy(t.astype(np.float64))).numpy()
    assert np.abs(a - b).max() <= np.spacing(np.abs(a)).max() and (np.abs(a - b) <= np.spacing(np.abs(a))).all()
    np.testing.assert_array_equal(a.astype(np.float32), b.astype(np.float32))
    margin = R.erf_margin_ulps(t)
    print(f"erf margin on normal(0, 2): {margin.min():.0f} float64 ulps over {margin.size} values")
    assert margin.min() >= 8


# ------------------------------------------------------------------------------------------------------------- the GPU tests' cases
def _pw_arguments(i, shape, large):
    """The values GELU is applied to in test_gpu_convnext's conv1x1_gelu case i, with and without the norm (a large case: on the sampled
    pixels it is compared on)."""
    n, cin, cout, h, w = shape
    x, wt, b, lw, lb = R.pw_case(i, shape)
    slice_len = None
    if large:
        assert R.pw_plan(n, cin, h * w, cout)[2] == 1
        x, slice_len = x.reshape(n, cin, 1, h * w)[:, :, :, R.sample_pixels(h * w, i)], 0
    pre = []
    R.conv1x1_gelu(x, wt, b, pre=pre, slice_len=slice_len)
    R.conv1x1_gelu(x, wt, b, norm=R.layer_norm2d_stats(x, 1e-6) + (lw, lb), pre=pre, slice_len=slice_len)
    return pre


def _assert_margin(values, what):
    margin = R.erf_margin_ulps(np.concatenate([R.gelu_arguments(v).reshape(-1) for v in values]))
    assert margin.size and margin.min() >= 8, (what, margin.min())
    return margin.min()


def test_no_gpu_case_is_decided_by_a_libms_last_bit():
    """For every GELU argument the bit-for-bit GPU cases produce, taken from the reference: erf in float64 lies at least 8 float64 ulps
    from a float32 rounding midpoint, so a libm whose erf is within a few ulps gives the same float32.  (A seed that fails this is
    changed; the margin is not.)"""
    lo = []
    for i, shape in enumerate(R.PW_SMALL):
        lo.append(_assert_margin(_pw_arguments(i, shape, False), shape))
    for i, shape in enumerate(R.PW_LARGE):
        lo.append(_assert_margin(_pw_arguments(len(R.PW_SMALL) + i, shape, True), shape))
    for shape in R.GUARD_PW_CASES:  # tests/test_gpu_convnext_guard.py
        x, wt, b, lw, lb = R.pw_case(R.GUARD_SEED, shape)
        pre = []
        R.conv1x1_gelu(x, wt, b, pre=pre)
        R.conv1x1_gelu(x, wt, b, norm=R.layer_norm2d_stats(x, 1e-6) + (lw, lb), pre=pre)
        lo.append(_assert_margin(pre, ("guard", shape)))
    lo.append(_assert_margin([R.SPECIAL_GELU_VALUES], "special values"))
    for dim, h, w in R.BLOCK_CASES:
        _, cpu = R.block_pair(dim, 40 + dim, CNBlock)
        pre = []
        R.block_stages(cpu, R.block_input(dim, h, w, 50 + dim), pre)
        lo.append(_assert_margin(pre, ("block", dim)))
    _, cpu = R.net_pair(R.NET_ROWS, 31, lambda **kw: ConvNeXt([CNBlockConfig(*r) for r in R.NET_ROWS], **kw))
    pre = []
    R.forward_stages(cpu, R.block_input(3, 64, 64, 800), pre)
    lo.append(_assert_margin(pre, "custom network"))
    _, cpu = R.net_pair("convnext_tiny", 33, convnext_tiny)
    pre = []
    R.forward_stages(cpu, R.block_input(3, 32, 32, 801)[:1], pre)
    lo.append(_assert_margin(pre, "convnext_tiny"))
    print(f"smallest erf margin over the GPU cases: {min(lo):.0f} float64 ulps")


def test_the_gpu_shape_lists_reach_every_instance_and_edge():
    plans = {shape: R.pw_plan(shape[0], shape[1], shape[3] * shape[4], shape[2]) for shape in R.PW_SMALL + R.PW_LARGE}
    assert set(plans.values()) == R.LN_INSTANCES
    assert {R.pw_plan(*s[:2], s[3] * s[4], s[2]) for s in R.PW_LARGE} == {(2, 1, 1), (2, 2, 1), (2, 4, 1), (4, 2, 1), (4, 4, 1)}
    for (n, cin, cout, h, w), (nt, mw, ks) in plans.items():
        slices, _ = F.conv1x1_k_slices(n, cin, h, w, cout)  # the restated plan and the library's agree on the K slices
        assert slices == (1 if ks == 1 else -(-(-(-cin // 32)) // (-(-(-(-cin // 32)) // ks)))), (n, cin, cout, h, w, slices, ks)
    # H W one below, at and one above a multiple of the pixels of a workgroup, for every one of the 14 instances
    for nt, mw, ks in R.LN_INSTANCES:
        pxb = R.pixels_per_workgroup(nt, mw)
        rem = {s[3] * s[4] % pxb for s, p in plans.items() if p == (nt, mw, ks) and s[3] * s[4] >= pxb - 1}
        assert rem >= {pxb - 1, 0, 1}, (nt, mw, ks, sorted(rem))
    for shape in R.PW_LARGE:  # the sample a large case is compared on holds the plane's last pixels
        hw = shape[3] * shape[4]
        assert set(range(hw - 300, hw)) <= set(R.sample_pixels(hw, 7).tolist())
    assert {s[1] for s in R.PW_SMALL} >= {31, 32, 33, 96} and {s[2] for s in R.PW_SMALL} >= {31, 32, 33, 127, 128, 129}
    assert any(s[0] == 2 for s in R.PW_SMALL)
    for shapes in (R.PW_SMALL, R.PW_LARGE):  # planes of whole quads (16-byte loads and stores) and others
        assert {s[3] * s[4] % 4 == 0 for s in shapes} == {True, False}
    # the depthwise strips: 8 rows, 4 in short launches (tests/test_gpu_convnext.py takes heights around both under each)
    assert R.dw7x7_plan(1, 3, 9, 9)[0] == 4 and R.dw7x7_plan(4, 65, 9, 260)[0] == 8
    for dim, h, w in R.BLOCK_CASES:
        assert R.pw_plan(2, dim, h * w, 4 * dim)[2] == 1
    assert R.pw_plan(2, 384, 49, 96)[2] == 4  # the dim-96 block's projection sums K in slices
