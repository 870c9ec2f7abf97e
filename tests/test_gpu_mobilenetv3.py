"""MobileNetV3 on the GPU (`-m gpu`): the 5x5 depthwise kernel, the squeeze-excitation kernels, the gated projection, the modules and
the two networks.  Every comparison is bit for bit -- NaN in equal places, == elsewhere -- against oracle/ref.py (the convs) and the
restatements of tests/_mobilenetv3_ref.py (the float64-summed pool and dense layer); the networks' logits are also held to the
project's accuracy condition against a float64 evaluation."""
import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd.mobilenet import SqueezeExcitation  # noqa: E402
from cpu_vision_amd.mobilenetv3 import (InvertedResidual, InvertedResidualConfig, mobilenet_v3_large,  # noqa: E402
                                        mobilenet_v3_small)
from oracle import ref  # noqa: E402
from tests import _mobilenetv3_ref as R  # noqa: E402

NAN, INF = float("nan"), float("inf")
ACTS = [None, "relu", "relu6", "hardswish", "silu"]
AFFINE = {None: 0, "mul_add": 1, "fma": 2}


def _rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def _randn(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _offset_by_4_bytes(a):
    """The array on the device, starting 4 bytes past a 16-byte boundary."""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------------------------- depthwise 5x5
def _dw(x, w, stride, bias=None, alpha=None, beta=None, res=None, affine=None, act=None, xd=None):
    got = F.conv_norm_act(_cuda(x) if xd is None else xd, _cuda(w), _cuda(bias), _cuda(alpha), _cuda(beta), _cuda(res), stride=stride,
                          groups=x.shape[1], affine=affine, activation=act)
    want = ref.conv2d_affine_act(x, w, bias, alpha, beta, res, stride, (w.shape[-1] - 1) // 2, x.shape[1], AFFINE[affine], act)
    return got, want


SIZES = [(1, 1), (2, 3), (4, 4), (5, 5), (7, 7), (9, 6), (14, 14), (28, 28), (33, 31), (6, 64), (3, 260)]


@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise5x5_sizes_channels_batches(stride):
    """Maps smaller than the window, odd and even sizes at stride 2, one thread group and several per row, rows of whole quads."""
    rng = _rng(100 + stride)
    for h, w in SIZES:
        for c in (1, 3, 65):
            for n in (1, 2):
                x, wt = _randn(rng, (n, c, h, w)), _randn(rng, (c, 1, 5, 5), 0.3)
                got, want = _dw(x, wt, stride)
                assert _lib.last_kernel().startswith(f"k_dwpc5x5<s{stride},"), _lib.last_kernel()
                R.same(got, want, f"dw5x5 s{stride} {(n, c, h, w)}")


@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise5x5_heights_around_the_strip_lengths(stride):
    """A thread's strip is 8 output rows, 4 in launches of fewer than 16384 threads: output heights 3, 4, 5 and 7, 8, 9 under both."""
    rng = _rng(110 + stride)
    for oh in (3, 4, 5, 7, 8, 9):
        for h in ({oh} if stride == 1 else {2 * oh - 1, 2 * oh}):
            for (n, c, w), rows in (((1, 3, 9), 4), ((4, 65, 260 * stride), 8)):
                x, wt = _randn(rng, (n, c, h, w)), _randn(rng, (c, 1, 5, 5), 0.3)
                got, want = _dw(x, wt, stride)
                assert _lib.last_kernel() == f"k_dwpc5x5<s{stride},rows{rows}>", (_lib.last_kernel(), n, c, h, w)
                R.same(got, want, f"dw5x5 s{stride} {(n, c, h, w)}")


@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise5x5_x_at_a_4_byte_offset_gives_the_same_bits(stride):
    rng = _rng(120 + stride)
    for shape in ((2, 3, 28, 28), (1, 5, 8, 64), (1, 2, 14, 14)):
        x, wt = _randn(rng, shape), _randn(rng, (shape[1], 1, 5, 5), 0.3)
        aligned, want = _dw(x, wt, stride)
        shifted, _ = _dw(x, wt, stride, xd=_offset_by_4_bytes(x))
        R.same(aligned, want, f"aligned {shape}")
        assert torch.equal(aligned, shifted)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("affine", [None, "mul_add", "fma"])
def test_depthwise5x5_epilogue(stride, affine):
    rng = _rng(130 + stride)
    n, c, h, w = 2, 7, 9, 11
    x, wt = _randn(rng, (n, c, h, w)), _randn(rng, (c, 1, 5, 5), 0.3)
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    alpha, beta = (None, None) if affine is None else (_randn(rng, c) + 1.5, _randn(rng, c))
    for act in ACTS:
        for bias in (None, _randn(rng, c)):
            for res in (None, _randn(rng, (n, c, oh, ow))):
                got, want = _dw(x, wt, stride, bias, alpha, beta, res, affine, act)
                if act == "silu":  # expf: last-ulp differences from the CPU's (convnorm.hip)
                    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-6, atol=1e-7)
                else:
                    R.same(got, want, f"dw5x5 epilogue s{stride} {affine} {act} bias={bias is not None} res={res is not None}")


def test_depthwise_entry_empty_batch_kernel_3_and_refusals():
    rng = _rng(140)
    assert tuple(F.conv_norm_act(torch.empty((0, 4, 6, 6), device="cuda"), _cuda(_randn(rng, (4, 1, 5, 5))), groups=4, stride=2).shape) == (0, 4, 3, 3)
    lib = _lib.load()
    x, w3 = _cuda(_randn(rng, (2, 5, 9, 7))), _cuda(_randn(rng, (5, 1, 3, 3)))
    for stride in (1, 2):
        want = F.conv_norm_act(x, w3, groups=5, stride=stride, activation="hardswish")
        name = _lib.last_kernel()
        y = torch.full_like(want, -7.25)
        rc = lib.mv_dwconv_norm_act_f32(x.data_ptr(), w3.data_ptr(), None, None, None, None, y.data_ptr(), 2, 5, 9, 7, 3, stride, 0, 3, _lib.stream_ptr(x))
        assert rc == 0 and _lib.last_kernel() == name and torch.equal(y, want)
    with pytest.raises(NotImplementedError, match="depthwise 3x3 and 5x5"):
        F.conv_norm_act(x, _cuda(_randn(rng, (5, 1, 7, 7))), groups=5)
    with pytest.raises(NotImplementedError, match="input_scale: pointwise"):
        F.conv_norm_act(x, _cuda(_randn(rng, (5, 1, 5, 5))), groups=5, input_scale=torch.ones(2, 5, device="cuda"))
    with pytest.raises(RuntimeError, match="input_scale should have shape"):
        F.conv_norm_act(x, _cuda(_randn(rng, (4, 5, 1, 1))), input_scale=torch.ones(2, 4, device="cuda"))


def test_conv_norm_act_accepts_depthwise_5x5_weights():
    """On the code before the feature this call raises NotImplementedError."""
    rng = _rng(150)
    x, wt = _randn(rng, (1, 8, 14, 14)), _randn(rng, (8, 1, 5, 5), 0.3)
    got, want = _dw(x, wt, 1, act="hardswish")
    R.same(got, want, "conv_norm_act on (c, 1, 5, 5)")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("value", [NAN, INF])
def test_depthwise5x5_special_value_reaches_its_windows_only(stride, value):
    rng = _rng(160)
    n, c, h, w = 1, 2, 13, 14
    x, wt = _randn(rng, (n, c, h, w)), _randn(rng, (c, 1, 5, 5), 0.3) + 0.01
    iy, ix = 6, 9
    x[0, 1, iy, ix] = value
    got, want = _dw(x, wt, stride)
    R.same(got, want, "special value")
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    mask = np.zeros((n, c, oh, ow), bool)
    for oy in range(oh):
        for ox in range(ow):
            mask[0, 1, oy, ox] = abs(oy * stride - iy) <= 2 and abs(ox * stride - ix) <= 2
    assert mask.sum() == (25 if stride == 1 else 6)
    np.testing.assert_array_equal(~np.isfinite(got.cpu().numpy()), mask)


# ------------------------------------------------------------------------------------------------------------- global_avg_pool
PLANES = {1: (1, 1), 3: (1, 3), 4: (2, 2), 49: (7, 7), 255: (15, 17), 256: (16, 16), 257: (1, 257), 784: (28, 28), 3136: (56, 56), 5000: (50, 100)}


def test_global_avg_pool_against_the_restatement():
    rng = _rng(200)
    for hw, (h, w) in PLANES.items():
        for c in (1, 3, 72):
            for n in (1, 3):
                x = _randn(rng, (n, c, h, w)) + 0.5
                got = F.global_avg_pool(_cuda(x))
                assert _lib.last_kernel() == "k_se_pool" and tuple(got.shape) == (n, c)
                R.same(got, R.global_avg_pool(x), f"pool {(n, c, h, w)}")
    assert tuple(F.global_avg_pool(torch.empty((0, 3, 4, 4), device="cuda")).shape) == (0, 3)


def test_global_avg_pool_slices_offsets_and_positions():
    rng = _rng(210)
    wide = _randn(rng, (3, 9, 7, 7))
    wd = _cuda(wide)
    got = F.global_avg_pool(wd[:, 2:7])  # a channel slice, read where it lies
    R.same(got, R.global_avg_pool(wide[:, 2:7]), "channel slice")
    for shape in ((2, 3, 16, 16), (1, 2, 50, 100), (2, 5, 7, 7)):
        x = _randn(rng, shape)
        a, b = F.global_avg_pool(_cuda(x)), F.global_avg_pool(_offset_by_4_bytes(x))  # 16-byte loads, then 4-byte loads
        assert torch.equal(a, b)
        R.same(a, R.global_avg_pool(x), f"offset {shape}")
    # one plane's result at two positions in the tensor and at two batch sizes
    plane = _randn(rng, (28, 28))
    x1, x2 = _randn(rng, (1, 4, 28, 28)), _randn(rng, (3, 6, 28, 28))
    x1[0, 1], x2[2, 5] = plane, plane
    a, b = F.global_avg_pool(_cuda(x1)), F.global_avg_pool(_cuda(x2))
    assert a[0, 1].item() == b[2, 5].item() == R.global_avg_pool(plane[None, None])[0, 0]


def test_global_avg_pool_special_values_stay_in_their_plane():
    rng = _rng(220)
    x = _randn(rng, (2, 4, 9, 9))
    x[0, 1, 3, 3], x[1, 0, 0, 0], x[1, 2, 8, 8], x[1, 3, 1, 1], x[1, 3, 5, 5] = NAN, INF, -INF, INF, -INF
    got = F.global_avg_pool(_cuda(x))
    want = R.global_avg_pool(x)
    R.same(got, want, "special values")
    g = got.cpu().numpy()
    assert np.isnan(g[0, 1]) and g[1, 0] == INF and g[1, 2] == -INF and np.isnan(g[1, 3])
    assert np.isfinite(np.delete(g.reshape(-1), [1, 4, 6, 7])).all()


# ------------------------------------------------------------------------------------------------------------- linear_act
LIN_ACTS = [None, "relu", "hardswish", "hardsigmoid", "sigmoid"]


@pytest.mark.parametrize("k,m", [(1, 1), (3, 8), (63, 5), (64, 64), (65, 7), (72, 24), (960, 240), (240, 960), (576, 1024)])
def test_linear_act_against_the_restatement(k, m):
    rng = _rng(300 + k + m)
    w, b = _randn(rng, (m, k), 0.3), _randn(rng, m)
    x33 = _randn(rng, (33, k))
    pre = {True: R.linear_act(x33, w, b), False: R.linear_act(x33, w, None)}
    for n in (1, 2, 5, 33):  # 33 rows cross any tile of images; rows of a smaller batch are the first rows of the larger
        for act in LIN_ACTS:
            for with_bias in (True, False):
                got = F.linear_act(_cuda(x33[:n]), _cuda(w), _cuda(b) if with_bias else None, act)
                assert _lib.last_kernel() == "k_linear_act"
                R.same(got, R.ACTIVATIONS[act](pre[with_bias][:n]), f"linear_act k={k} m={m} n={n} {act} bias={with_bias}")
    # a row's result does not depend on its index, and (M, K, 1, 1) weights are the same weights
    got = F.linear_act(_cuda(x33[::-1].copy()), _cuda(w.reshape(m, k, 1, 1)), _cuda(b), "hardsigmoid")
    R.same(got, R.act_hardsigmoid(pre[True])[::-1].copy(), "reversed rows, 4-D weight")
    assert tuple(F.linear_act(torch.empty((0, k), device="cuda"), _cuda(w)).shape) == (0, m)


def test_linear_act_special_values():
    """K = 1 and w = 1: the pre-activation values are x itself.  NaN gives NaN under every activation; +-inf as torch's CPU functions."""
    v = torch.tensor([NAN, -INF, INF, -3.0, -0.0, 0.0, 3.0, 7.5, -1e30, 1e30], dtype=torch.float32)
    one = torch.ones((1, 1), device="cuda")
    out = {a: F.linear_act(v.view(-1, 1).cuda(), one, None, a).cpu().view(-1) for a in LIN_ACTS}
    for a in LIN_ACTS:
        assert torch.isnan(out[a][0]), a
        R.same(out[a], torch.from_numpy(R.ACTIVATIONS[a](v.numpy())), str(a))
    R.same(out["relu"], torch.relu(v), "relu")
    R.same(out["hardswish"], nn.functional.hardswish(v), "hardswish")  # hardswish(-inf) is NaN
    R.same(out["hardsigmoid"], nn.functional.hardsigmoid(v), "hardsigmoid")
    assert torch.isnan(out["hardswish"][1]) and out["hardsigmoid"][1] == 0 and out["hardsigmoid"][2] == 1
    sig = torch.sigmoid(v)
    assert out["sigmoid"][1] == sig[1] == 0 and out["sigmoid"][2] == sig[2] == 1
    # a NaN among finite terms, and an infinity of each sign in one row (inf - inf)
    x = torch.ones((2, 70))
    x[0, 66], x[1, 3], x[1, 69] = NAN, INF, -INF
    for a in LIN_ACTS:
        assert bool(torch.isnan(F.linear_act(x.cuda(), torch.ones((3, 70), device="cuda"), None, a)).all()), a


# ------------------------------------------------------------------------------------------------------------- se_scale, gated projection
def test_se_scale_against_numpy_and_in_place():
    rng = _rng(400)
    for shape in ((1, 1, 1, 1), (2, 3, 5, 7), (3, 16, 9, 7), (2, 72, 28, 28), (1, 5, 1, 260)):
        x, g = _randn(rng, shape), _randn(rng, shape[:2])
        want = R.se_scale(x, g)
        got = F.se_scale(_cuda(x), _cuda(g))
        assert _lib.last_kernel() == ("k_se_scale<vec16>" if (shape[2] * shape[3]) % 4 == 0 else "k_se_scale<scalar>")
        R.same(got, want, f"se_scale {shape}")
        R.same(F.se_scale(_cuda(x), _cuda(g.reshape(shape[:2] + (1, 1)))), want, "4-D gate")
        xd = _cuda(x)
        assert F.se_scale(xd, _cuda(g), out=xd) is xd
        R.same(xd, want, f"in place {shape}")
        shifted = _offset_by_4_bytes(x)
        R.same(F.se_scale(shifted, _cuda(g)), want, f"offset {shape}")
    x, g = _randn(rng, (2, 4, 3, 3)), _randn(rng, (2, 4))
    g[0, 1], g[1, 0], g[1, 3] = NAN, INF, 0.0
    R.same(F.se_scale(_cuda(x), _cuda(g)), R.se_scale(x, g), "special gate")


PW_SHAPES = [(1, 1, (1, 1)), (3, 5, (1, 7)), (33, 31, (7, 7)), (72, 40, (28, 28)), (960, 160, (7, 7)), (672, 112, (14, 14)), (40, 24, (3, 11))]


@pytest.mark.parametrize("cin,cout,hw", PW_SHAPES)
def test_scaled_projection_equals_the_unfused_form_and_the_oracle(cin, cout, hw):
    """A short last K chunk (33, 72, 40 channels), partial pixel tiles (1, 7, 49, 33 pixels), several K slices (960 and 672 channels on
    small maps) and single chains."""
    rng = _rng(500 + cin)
    h, w = hw
    for n in (1, 3):
        slices, sl = F.conv1x1_k_slices(n, cin, h, w, cout)
        if (cin, n) in ((960, 1), (672, 1)):
            assert slices > 1, (slices, sl)
        if cin <= 72:
            assert slices == 1
        x, g = _randn(rng, (n, cin, h, w)), (np.abs(_randn(rng, (n, cin))) % 1.0).astype(np.float32)
        wt = _randn(rng, (cout, cin, 1, 1), 0.2)
        alpha, beta = _randn(rng, cout) + 1.5, _randn(rng, cout)
        scaled = R.se_scale(x, g)
        xd, gd, wd = _cuda(x), _cuda(g), _cuda(wt)
        for affine in ("fma", "mul_add"):
            for res in (None, _randn(rng, (n, cout, h, w))):
                got = F.conv_norm_act(xd, wd, None, _cuda(alpha), _cuda(beta), _cuda(res), affine=affine, input_scale=gd)
                assert _lib.last_kernel().startswith("k_conv1x1_sc<"), _lib.last_kernel()
                unfused = F.conv_norm_act(F.se_scale(xd, gd), wd, None, _cuda(alpha), _cuda(beta), _cuda(res), affine=affine)
                assert _lib.last_kernel().startswith("k_conv1x1<"), _lib.last_kernel()
                what = f"scaled projection {(n, cin, cout, h, w)} {affine} res={res is not None}"
                assert torch.equal(got, unfused), what
                want = ref.conv2d_affine_act(scaled, wt, None, alpha, beta, res, 1, 0, 1, AFFINE[affine], None, slice_len=sl if slices > 1 else 0)
                R.same(got, want, what)
        R.same(F.conv_norm_act(xd, wd, _cuda(beta), activation="relu", input_scale=gd.view(n, cin, 1, 1)),
               ref.conv2d_affine_act(scaled, wt, beta, None, None, None, 1, 0, 1, 0, "relu", slice_len=sl if slices > 1 else 0), "bias, ReLU, 4-D gate")


def test_scaled_projection_special_gates_and_the_plain_path_unchanged():
    rng = _rng(520)
    n, cin, cout, h, w = 2, 40, 24, 3, 11
    x, g, wt = _randn(rng, (n, cin, h, w)), np.abs(_randn(rng, (n, cin))), _randn(rng, (cout, cin, 1, 1), 0.2)
    g[0, 3], g[0, 39], g[1, 0], g[1, 17] = 0.0, NAN, INF, -INF
    xd, gd, wd = _cuda(x), _cuda(g), _cuda(wt)
    got = F.conv_norm_act(xd, wd, input_scale=gd)
    unfused = F.conv_norm_act(F.se_scale(xd, gd), wd)
    R.same(got, unfused, "special gates")
    assert bool(torch.isnan(got[0]).all()) and not bool(torch.isfinite(got[1]).any())
    g[0, 39], g[1, 17] = 2.0, 1.0  # image 0 finite (one channel gated off), image 1 a single +inf
    gd = _cuda(g)
    got = F.conv_norm_act(xd, wd, input_scale=gd)
    R.same(got, F.conv_norm_act(F.se_scale(xd, gd), wd), "zero and inf gates")
    assert bool(torch.isfinite(got[0]).all()) and not bool(torch.isfinite(got[1]).any())
    # without a gate the existing instances run, under the names they had
    for (ci, co, hh, ww), name in (((72, 40, 28, 28), "k_conv1x1<1,2>"), ((960, 160, 7, 7), "k_conv1x1<1,4,ks4>"), ((16, 64, 32, 32), "k_conv1x1<1,1>")):
        F.conv_norm_act(_cuda(_randn(rng, (1, ci, hh, ww))), _cuda(_randn(rng, (co, ci, 1, 1))), input_scale=None)
        assert _lib.last_kernel() == name, (_lib.last_kernel(), name)


# ------------------------------------------------------------------------------------------------------------- modules
@pytest.mark.parametrize("scale", [nn.Hardsigmoid, nn.Sigmoid])
def test_squeeze_excitation_module(scale):
    torch.manual_seed(5)
    se = SqueezeExcitation(16, 8, scale_activation=scale)
    with torch.no_grad():
        se.fc1.bias.normal_()
        se.fc2.bias.normal_()
    x = _randn(_rng(600), (3, 16, 9, 7))
    gate = R.se_gate_of(se, x)
    dev = SqueezeExcitation(16, 8, scale_activation=scale)
    dev.load_state_dict(se.state_dict())
    dev = dev.cuda()
    with torch.no_grad():
        sc = dev._scale(_cuda(x))
        assert tuple(sc.shape) == (3, 16, 1, 1)
        R.same(sc.view(3, 16), gate, "SqueezeExcitation._scale")
        R.same(dev(_cuda(x)), R.se_scale(x, gate), "SqueezeExcitation.forward")
    assert ((gate > 0) & (gate < 1)).mean() > 0.4


BLOCKS = [(16, 3, 16, 16, False, "RE", 1), (16, 3, 64, 24, False, "RE", 2), (24, 5, 72, 24, True, "RE", 1), (24, 5, 96, 40, True, "HS", 2),
          (16, 3, 16, 16, True, "RE", 2), (24, 3, 88, 24, False, "HS", 1), (24, 5, 24, 24, True, "HS", 1)]


@pytest.mark.parametrize("row", BLOCKS)
def test_inverted_residual_stage_by_stage(row):
    """With and without expansion, with and without squeeze-excitation, 3x3 and 5x5, stride 1 and 2, with and without the residual, ReLU
    and Hardswish: every launch of the block's forward against the reference forward."""
    cin, k, exp, cout, se, act, stride = row
    norm = lambda c: nn.BatchNorm2d(c, eps=0.001, momentum=0.01)  # noqa: E731
    torch.manual_seed(7)
    cpu = InvertedResidual(InvertedResidualConfig(cin, k, exp, cout, se, act, stride, 1, 1.0), norm).eval()
    R.perturb(cpu, 17)
    dev = InvertedResidual(InvertedResidualConfig(cin, k, exp, cout, se, act, stride, 1, 1.0), norm).eval()
    dev.load_state_dict(cpu.state_dict())
    dev = dev.cuda()
    x = _randn(_rng(700 + cin + exp), (2, cin, 14, 14))
    want = R.block_stages(cpu, x)
    assert len(want) == len(cpu.block)
    with torch.no_grad():
        y, stages = _cuda(x), []
        for layer in list(dev.block)[:-1]:
            if isinstance(layer, SqueezeExcitation):
                stages.append(layer._gate(y))
            else:
                y = layer(y)
                stages.append(y)
        stages.append(dev(_cuda(x)))
        assert _lib.last_kernel().startswith("k_conv1x1_sc<" if se else "k_conv1x1<"), _lib.last_kernel()
    for i, (g, wnt) in enumerate(zip(stages, want)):
        R.same(g, wnt, f"block {row} stage {i}")
    assert cpu.use_res_connect == (stride == 1 and cin == cout)


def _pair(builder, arch, seed, **kw):
    torch.manual_seed(seed)
    rep = R.replica(arch, num_classes=7, **kw).eval()
    R.perturb(rep, seed + 1)
    cpu = builder(num_classes=7, **kw)
    cpu.load_state_dict(rep.state_dict(), strict=True)
    dev = builder(num_classes=7, **kw)
    dev.load_state_dict(rep.state_dict(), strict=True)
    return rep, cpu, dev.cuda()


def _run_with_stages(dev, x):
    outs = []
    hooks = [m.register_forward_hook(lambda _m, _i, o: outs.append(o)) for m in dev.features]
    with torch.no_grad():
        logits = dev(_cuda(x))
    for hk in hooks:
        hk.remove()
    return outs, logits


@pytest.mark.parametrize("arch,builder", [("mobilenet_v3_small", mobilenet_v3_small), ("mobilenet_v3_large", mobilenet_v3_large)])
def test_network_stage_by_stage_and_accuracy(arch, builder):
    """Every stage and the logits bit for bit against the stage-by-stage reference forward; the logits against float64 within the
    project's condition: the library's error <= 2 x the float32 replica's error + 2^-22 max |f64|.  Measured, in units of 2^-24 max |f64|:
    small 0.95 (library) / 1.12 (replica), large 1.20 / 1.51."""
    rep, cpu, dev = _pair(builder, arch, 31)
    x = _randn(_rng(800), (2, 3, 64, 64))
    feats, want = R.forward_stages(cpu, x)
    outs, logits = _run_with_stages(dev, x)
    assert len(outs) == len(feats)
    for i, (g, wnt) in enumerate(zip(outs, feats)):
        R.same(g, wnt, f"{arch} features[{i}]")
    R.same(logits, want, f"{arch} logits")
    with torch.no_grad():
        t32 = rep(torch.from_numpy(x))
        f64 = rep.double()(torch.from_numpy(x).double())
    scale = float(f64.abs().max())
    e_lib, e_t = float((logits.cpu().double() - f64).abs().max()), float((t32.double() - f64).abs().max())
    print(f"{arch} logits: library {e_lib / scale * 2 ** 24:.2f}, torch float32 replica {e_t / scale * 2 ** 24:.2f} (x 2^-24 max|f64| = {scale:.3g})")
    assert e_lib <= 2 * e_t + 2.0 ** -22 * scale


def test_network_width_mult():
    rep, cpu, dev = _pair(mobilenet_v3_small, "mobilenet_v3_small", 41, width_mult=0.75)
    x = _randn(_rng(810), (1, 3, 64, 64))
    feats, want = R.forward_stages(cpu, x)
    outs, logits = _run_with_stages(dev, x)
    R.same(outs[-1], feats[-1], "width 0.75 features")
    R.same(logits, want, "width 0.75 logits")
    dil = mobilenet_v3_small(num_classes=3, dilated=True).cuda()
    with pytest.raises(NotImplementedError):
        dil(_cuda(x))
