"""ResNet on the GPU (`-m gpu`): F.conv2d_affine_act (k_conv_igemm_full and the columns form), F.max_pool2d with padding, the blocks
and whole networks of cpu_vision_amd.resnet -- bit for bit against the oracle composition of tests/_resnet_ref.py
(np.testing.assert_array_equal: NaN in equal places, == elsewhere) unless a test says otherwise."""
import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _layers, _lib, resnet  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd.mobilenet import FrozenBatchNorm2d  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _resnet_ref as R  # noqa: E402
from tests._boxes_ref import kernel_constant  # noqa: E402
from tests._util import philox_f32  # noqa: E402

TILE = kernel_constant("kIgTile", "conv_igemm.hip")  # the workgroup tile is TILE * {1, 2, 3} channels x TILE * {1, 2, 4} pixels
AFFINES = (None, "mul_add", "fma")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _data(seed, n, cin, h, w, cout, kh, kw, groups=1):
    x = philox_f32(seed, (n, cin, h, w)) * 2 - 1
    wt = (philox_f32(seed + 1, (cout, cin // groups, kh, kw)) - 0.5) * 0.5
    a, b = philox_f32(seed + 2, (cout,)) + 0.5, philox_f32(seed + 3, (cout,)) - 0.5
    bias = philox_f32(seed + 4, (cout,)) - 0.5
    return x, wt, a, b, bias


def _both(x, wt, bias=None, a=None, b=None, res=None, stride=1, padding=0, dilation=1, groups=1, affine=None, act=None, on_dev=None):
    """(GPU result, oracle result) of one call; on_dev: already uploaded (x, weight)."""
    dx, dw = on_dev if on_dev is not None else (dev(x), dev(wt))
    use = affine is not None
    got = host(F.conv2d_affine_act(dx, dw, dev(bias), dev(a) if use else None, dev(b) if use else None, dev(res), stride=stride,
                                   padding=padding, dilation=dilation, groups=groups, affine=affine, activation=act))
    want = R.oracle_conv(x, wt, bias, a if use else None, b if use else None, res, stride, padding, dilation, groups, R.AFFINE[affine], act)
    return got, want


def _out_shape(x, wt, stride, padding, dilation):
    span = lambda k: dilation * (k - 1) + 1  # noqa: E731
    return (x.shape[0], wt.shape[0], (x.shape[2] + 2 * padding - span(wt.shape[2])) // stride + 1,
            (x.shape[3] + 2 * padding - span(wt.shape[3])) // stride + 1)


# ---- geometries --------------------------------------------------------------------------------------------------------------
GEOMETRIES = {
    # name: (n, cin, h, w, cout, k, stride, padding, dilation, groups, affine, residual, act)
    "stem 7x7 s2 p3, K = 147": (2, 3, 33, 37, 64, 7, 2, 3, 1, 1, "fma", False, "relu"),
    "3x3 s1 p1 + residual + relu": (2, 64, 9, 11, 64, 3, 1, 1, 1, 1, "fma", True, "relu"),
    "3x3 s2 p1": (2, 64, 15, 15, 128, 3, 2, 1, 1, 1, "mul_add", False, "relu"),
    "1x1 s2 fma, no activation": (2, 64, 15, 14, 128, 1, 2, 0, 1, 1, "fma", False, None),
    "3x3 dilation 2 padding 2": (2, 16, 13, 12, 24, 3, 1, 2, 2, 1, "fma", True, "relu"),
    "groups = 2": (2, 16, 10, 9, 36, 3, 1, 1, 1, 2, "mul_add", True, "relu"),
    "groups = 2, stride 2, dilation 2": (2, 8, 12, 13, 10, 3, 2, 2, 2, 2, "fma", False, None),
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("small_launch_workspace", [False, True], ids=["implicit", "columns"])
def test_geometries(name, small_launch_workspace, monkeypatch):
    """Each geometry in the implicit form and (all of them are launches of a handful of workgroups) in the columns form."""
    monkeypatch.setattr(F, "CONV2D_SMALL_LAUNCH_WORKSPACE", small_launch_workspace)
    n, cin, h, w, cout, k, stride, padding, dilation, groups, affine, residual, act = GEOMETRIES[name]
    x, wt, a, b, _ = _data(3100 + cout + h, n, cin, h, w, cout, k, k, groups)
    res = philox_f32(3105, _out_shape(x, wt, stride, padding, dilation)) - 0.5 if residual else None
    got, want = _both(x, wt, None, a, b, res, stride, padding, dilation, groups, affine, act)
    assert _lib.last_kernel().startswith("k_conv1x1" if small_launch_workspace else "k_conv_igemm_full"), _lib.last_kernel()
    np.testing.assert_array_equal(got, want, err_msg=name)  # (the dilated cases: by value, +0 == -0, see tests/_resnet_ref.py)


# ---- tile and store edges ------------------------------------------------------------------------------------------------------
# oh * ow at the pixel tiles (TILE, 2 TILE, 4 TILE) - 1, + 0, + 1: the tile sizes themselves have HW % 4 == 0 (16-byte stores and
# residual loads), their neighbours not (scalar path)
def _factor(hw):
    for d in range(int(hw ** 0.5), 0, -1):
        if hw % d == 0:
            return d, hw // d


PIXELS = [t * TILE + e for t in (1, 2, 4) for e in (-1, 0, 1)]


@pytest.mark.parametrize("cout", [63, 64, 65, 129, 193])
def test_tile_and_store_edges(cout, monkeypatch):
    """cout at the channel tiles +- 1 x every pixel-tile edge x affine x residual x activation, in the implicit kernel."""
    monkeypatch.setattr(F, "CONV2D_SMALL_LAUNCH_WORKSPACE", False)
    assert {p % 4 == 0 for p in PIXELS} == {True, False}
    for hw in PIXELS:
        h, w = _factor(hw)
        x, wt, a, b, bias = _data(3200 + hw, 2, 3, h, w, cout, 3, 3)
        res = philox_f32(3206 + hw, (2, cout, h, w)) - 0.5
        on_dev = (dev(x), dev(wt))
        for affine in AFFINES:
            for r in (None, res):
                for act in (None, "relu"):
                    got, want = _both(x, wt, bias if affine is None else None, a, b, r, 1, 1, 1, 1, affine, act, on_dev=on_dev)
                    kernel = _lib.last_kernel()
                    assert kernel.startswith("k_conv_igemm_full" if (affine or r is not None) else "k_conv_igemm<"), kernel
                    np.testing.assert_array_equal(got, want, err_msg=f"cout {cout} hw {h}x{w} {affine} res={r is not None} {act} [{kernel}]")


# ---- every instance the launcher can pick runs the full epilogue -----------------------------------------------------------------
INSTANCES = {
    # (channels, pixels) of the workgroup tile: (n, cin, h, w, cout)
    (64, 256): (2, 64, 65, 65, 64),   # HW = 4225 > 4096
    (64, 128): (8, 4, 64, 64, 64),    # 8 x 32 = 256 workgroups of 128 pixels
    (64, 64): (2, 8, 9, 9, 40),
    (128, 128): (4, 8, 91, 91, 128),  # 4 x 65 = 260 workgroups
    (128, 64): (2, 8, 9, 9, 128),
    (192, 128): (4, 4, 91, 91, 192),
    (192, 64): (2, 8, 9, 9, 192),
}


@pytest.mark.parametrize("tile", list(INSTANCES), ids=str)
def test_every_instance_runs_the_full_epilogue(tile, monkeypatch):
    monkeypatch.setattr(F, "CONV2D_SMALL_LAUNCH_WORKSPACE", False)
    n, cin, h, w, cout = INSTANCES[tile]
    x, wt, a, b, _ = _data(3300 + cout + h, n, cin, h, w, cout, 3, 3)
    res = philox_f32(3307, (n, cout, h, w)) - 0.5
    got, want = _both(x, wt, None, a, b, res, 1, 1, 1, 1, "fma", "relu")
    assert _lib.last_kernel() == "k_conv_igemm_full<%dch,%dpx,implicit 3x3>" % tile, _lib.last_kernel()
    np.testing.assert_array_equal(got, want)


def test_existing_entry_keeps_its_instances(monkeypatch):
    """F.conv2d_bias_act and the new entry without norm and residual run the bias + activation instances, same bits."""
    monkeypatch.setattr(F, "CONV2D_SMALL_LAUNCH_WORKSPACE", False)
    x, wt, _, _, bias = _data(3400, 2, 5, 9, 11, 70, 3, 3)
    old = host(F.conv2d_bias_act(dev(x), dev(wt), dev(bias), stride=1, padding=1, activation="relu"))
    assert _lib.last_kernel() == "k_conv_igemm<128ch,64px,implicit 3x3>"
    new = host(F.conv2d_affine_act(dev(x), dev(wt), dev(bias), padding=1, activation="relu"))
    assert _lib.last_kernel() == "k_conv_igemm<128ch,64px,implicit 3x3>"
    np.testing.assert_array_equal(old, new)
    np.testing.assert_array_equal(new, ref.conv2d_affine_act(x, wt, bias, None, None, None, 1, 1, 1, 0, "relu"))


# ---- non-finite values, the two forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small_launch_workspace", [False, True], ids=["implicit", "columns"])
def test_nan_and_inf_come_out_where_the_oracle_puts_them(small_launch_workspace, monkeypatch):
    monkeypatch.setattr(F, "CONV2D_SMALL_LAUNCH_WORKSPACE", small_launch_workspace)
    x, wt, a, b, _ = _data(3500, 2, 6, 10, 12, 20, 3, 3)
    res = philox_f32(3506, (2, 20, 10, 12)) - 0.5
    x[0, 1, 0, 0], x[0, 2, 9, 11], x[1, 5, 4, 6], x[1, 0, 5, 5] = np.nan, np.inf, -np.inf, np.inf
    res[0, 3, 7, 7], res[1, 19, 9, 11], res[1, 2, 0, 0] = np.nan, np.inf, -np.inf
    for affine in AFFINES:
        for act in (None, "relu"):
            got, want = _both(x, wt, None, a, b, res, 1, 1, 1, 1, affine, act)
            assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
            np.testing.assert_array_equal(got, want, err_msg=f"{affine} {act}")


def _with_and_without_the_optional_workspace(monkeypatch, n, cin, h, w, cout, groups, affines):
    assert _lib.load().mv_conv2d_needs_workspace(n, cin, cout, h, w, 3, 3, 1, 1, 1, 1, 1, 1, groups) == 2
    x, wt, a, b, _ = _data(3600, n, cin, h, w, cout, 3, 3, groups)
    res = philox_f32(3606, (n, cout, h, w)) - 0.5
    out = {}
    for flag, kernel in ((False, "k_conv_igemm_full"), (True, "k_conv1x1")):
        monkeypatch.setattr(F, "CONV2D_SMALL_LAUNCH_WORKSPACE", flag)
        for affine in affines:
            got, want = _both(x, wt, None, a, b, res, 1, 1, 1, groups, affine, "relu")
            assert _lib.last_kernel().startswith(kernel), _lib.last_kernel()
            np.testing.assert_array_equal(got, want, err_msg=f"{affine} workspace={flag}")
            out[flag, affine] = got
    for affine in affines:
        np.testing.assert_array_equal(out[False, affine], out[True, affine])


def test_with_and_without_the_optional_workspace_same_bits(monkeypatch):
    _with_and_without_the_optional_workspace(monkeypatch, 1, 64, 14, 14, 64, 1, AFFINES)


def test_grouped_columns_form_in_several_passes_with_a_residual(monkeypatch):
    """Two weight groups, and a workspace of exactly one image's columns: three passes, in which the residual (like y) advances
    per pass and per group at once."""
    n, cin, h, w, cout = 3, 4, 5, 5, 6
    per_image = _lib.load().mv_deform_conv2d_workspace_bytes(1, cin, h, w, 3, 3, 1, 1, 1, 1, 1, 1)
    assert per_image == cin * 9 * h * w * 4
    monkeypatch.setattr(_layers, "_CONV_WORKSPACE_BYTES", per_image)
    _with_and_without_the_optional_workspace(monkeypatch, n, cin, h, w, cout, 2, ("fma",))


def test_python_checks():
    x, wt = torch.zeros(1, 4, 6, 6, device="cuda"), torch.zeros(8, 4, 3, 3, device="cuda")
    v = torch.ones(8, device="cuda")
    with pytest.raises(ValueError, match="needs alpha and beta"):
        F.conv2d_affine_act(x, wt, affine="fma")
    with pytest.raises(ValueError, match="unknown"):
        F.conv2d_affine_act(x, wt, alpha=v, beta=v, affine="group")
    with pytest.raises(RuntimeError, match="residual of shape"):
        F.conv2d_affine_act(x, wt, residual=torch.zeros(1, 8, 6, 6, device="cuda"))  # the output is 4 x 4 without padding
    with pytest.raises(RuntimeError, match="elements for 8 output channels"):
        F.conv2d_affine_act(x, wt, alpha=v[:4], beta=v, affine="fma")
    with pytest.raises(RuntimeError, match="does not fit"):
        F.conv2d_affine_act(x, wt, groups=2)
    with pytest.raises(RuntimeError, match="output size too small"):
        F.conv2d_affine_act(x, torch.zeros(8, 4, 7, 7, device="cuda"))
    assert F.conv2d_affine_act(x[:0], wt, padding=1).shape == (0, 8, 6, 6)
    y = F.conv2d_affine_act(x.requires_grad_(), wt, padding=1)
    with pytest.raises(Exception):
        y.sum().backward()
    with pytest.raises(RuntimeError, match="pad should be at most half"):
        F.max_pool2d(x.detach(), 3, 2, padding=2)


# ---- the padded pool ------------------------------------------------------------------------------------------------------------------
def _pool_input(seed, shape):
    x = philox_f32(seed, shape) * 4 - 2
    flat = x.reshape(-1)
    flat[::7] = -np.abs(flat[::7]) - 1.0
    return x


POOLS = [((2, 3, 7, 7), 3, 2, 1), ((2, 3, 8, 9), 3, 2, 1), ((2, 3, 17, 33), 3, 2, 1), ((2, 3, 8, 9), 3, 1, 1), ((2, 3, 17, 33), 5, 2, 2),
         ((3, 9, 1), 3, 2, 1), ((3, 1, 9), 3, 2, 1), ((1, 1, 1), 3, 2, 1), ((2, 2, 6, 6), 2, 2, 1), ((4, 64, 32, 32), 3, 2, 1)]


@pytest.mark.parametrize("shape,k,stride,pad", POOLS, ids=str)
def test_padded_max_pool_equals_torch_cpu(shape, k, stride, pad):
    x = _pool_input(3700 + shape[-1], shape)
    variants = {"mixed": x, "all negative": -np.abs(x) - 0.5}
    special = x.copy()
    sf = special.reshape(-1)
    sf[0], sf[-1], sf[sf.size // 2] = np.nan, np.nan, np.nan
    sf[1::5] = -np.inf
    sf[3::11] = np.inf
    variants["nan and inf"] = special
    variants["all -inf"] = np.full(shape, -np.inf, np.float32)
    for name, v in variants.items():
        got = host(F.max_pool2d(dev(v), k, stride, pad))
        assert _lib.last_kernel() == "k_maxpool2d_pad"
        np.testing.assert_array_equal(got, R.padded_max_pool(v, k, stride, pad), err_msg=name)


def test_max_pool_without_padding_is_todays():
    x = _pool_input(3800, (2, 3, 13, 15))
    for args, kw in (((3, 2), {}), ((3, 2), {"padding": 0}), ((3, 2, 0), {})):
        got = host(F.max_pool2d(dev(x), *args, **kw))
        assert _lib.last_kernel() == "k_maxpool2d"
        np.testing.assert_array_equal(got, ref.maxpool2d(x, 3, 2))
    np.testing.assert_array_equal(host(F.max_pool2d(dev(x), 2, padding=0)), ref.maxpool2x2(x))


# ---- blocks -----------------------------------------------------------------------------------------------------------------------------
def _down(inplanes, planes, stride, norm):
    return nn.Sequential(resnet.conv1x1(inplanes, planes, stride), norm(planes))


BLOCKS = {
    "basic": lambda norm: resnet.BasicBlock(16, 16, norm_layer=norm),
    "basic, stride-2 downsample": lambda norm: resnet.BasicBlock(16, 24, 2, _down(16, 24, 2, norm), norm_layer=norm),
    "basic, dilation 2": lambda norm: resnet.BasicBlock(16, 16, dilation=2, norm_layer=norm),
    "bottleneck": lambda norm: resnet.Bottleneck(32, 8, norm_layer=norm),
    "bottleneck, stride-2 downsample": lambda norm: resnet.Bottleneck(16, 8, 2, _down(16, 32, 2, norm), norm_layer=norm),
    "bottleneck, dilation 2": lambda norm: resnet.Bottleneck(32, 8, dilation=2, norm_layer=norm),
    "bottleneck, groups 2 width 128": lambda norm: resnet.Bottleneck(32, 8, groups=2, base_width=128, norm_layer=norm),
}


@pytest.mark.parametrize("norm", [nn.BatchNorm2d, FrozenBatchNorm2d], ids=["BatchNorm2d", "FrozenBatchNorm2d"])
@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_equal_the_oracle_composition(name, norm):
    torch.manual_seed(41)
    block = BLOCKS[name](norm).eval()
    R.randomize_norms(block, 43)
    x = philox_f32(3900, (2, block.conv1.in_channels, 13, 11)) * 2 - 1
    want = R.oracle_block(block, x)
    launches = []
    got = host(_counting(block.cuda(), dev(x), launches))
    per_conv = 2 + (1 if hasattr(block, "conv3") else 0) + (1 if block.downsample is not None else 0)
    groups = block.conv2.groups
    assert len(launches) == per_conv, launches  # one library call per conv (a grouped conv launches once per group inside its call)
    assert groups in (1, 2)
    np.testing.assert_array_equal(got, want, err_msg=name)
    assert (got >= 0).all() and (got > 0).any()


def _counting(module, x, launches):
    """module(x), recording the library calls made through F.conv2d_affine_act / F.conv_norm_act."""
    originals = {n: getattr(F, n) for n in ("conv2d_affine_act", "conv_norm_act")}

    def wrap(n):
        def call(*a, **k):
            launches.append(n)
            return originals[n](*a, **k)
        return call
    try:
        for n in originals:
            setattr(F, n, wrap(n))
        return module(x)
    finally:
        for n, f in originals.items():
            setattr(F, n, f)


# ---- whole networks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_whole_network_equals_the_oracle_composition(name):
    torch.manual_seed(51)
    replica = getattr(R, name)(num_classes=10).eval()
    R.randomize_norms(replica, 53)
    model = getattr(resnet, name)(num_classes=10)
    model.load_state_dict(replica.state_dict(), strict=True)
    model = model.cuda()
    x = philox_f32(4000, (2, 3, 64, 64)) * 2 - 1
    for batch in (x, x[:1]):
        got = host(model(dev(batch)))
        want = R.oracle_resnet(replica, batch)
        assert got.shape == (batch.shape[0], 10) and np.isfinite(want).all() and np.abs(want).max() > 1e-3
        np.testing.assert_array_equal(got, want, err_msg=f"{name} batch {batch.shape[0]}")
    with torch.no_grad():  # and the network is the reference's: torch's own float32 forward on the CPU, to float32 accuracy
        np.testing.assert_allclose(got, replica(torch.from_numpy(x[:1])).numpy(), rtol=1e-3, atol=1e-4 * float(np.abs(want).max()))
