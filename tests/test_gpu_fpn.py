"""FPN on the GPU (`-m gpu`): F.conv1x1_upsample_add (k_conv1x1_up: the pointwise kernel whose epilogue reads the coarser map at
torch's nearest source index), cpu_vision_amd.fpn and backbone_utils.  Every value is compared bit for bit
(np.testing.assert_array_equal: NaN in equal places, == elsewhere) with the CPU oracle fed with
R = torch.nn.functional.interpolate(top_cpu, size, mode="nearest") as an ordinary residual (tests/_fpn_ref.py); max_pool2d(1, 2) and
relu, which the oracle does not have, are torch's on the CPU."""
from collections import OrderedDict
from functools import lru_cache

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import _lib, fpn, ops  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd.mobilenet import FrozenBatchNorm2d  # noqa: E402
from tests import _fpn_ref as P  # noqa: E402
from tests._util import philox_f32  # noqa: E402

AFFINES = (None, "mul_add", "fma")
CODE = {None: 0, "mul_add": 1, "fma": 2}
ACTS = (None, "relu")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _data(seed, n, cin, h, w, cout, top_hw):
    """x, weight, alpha, beta, bias, top: `n` distinct images everywhere (a wrong image stride on top shows)."""
    x = philox_f32(seed, (n, cin, h, w)) * 2 - 1
    wt = (philox_f32(seed + 1, (cout, cin, 1, 1)) - 0.5) * 0.5
    a, b = philox_f32(seed + 2, (cout,)) + 0.5, philox_f32(seed + 3, (cout,)) - 0.5
    bias = philox_f32(seed + 4, (cout,)) - 0.5
    top = philox_f32(seed + 5, (n, cout) + tuple(top_hw)) * 2 - 1
    return x, wt, a, b, bias, top


def _epilogues(x, wt, a, b, bias, top, what):
    """Every affine x activation of one shape on the GPU against the oracle; the conv bias is present except in the "fma" case (the
    kernel's fast epilogue is the one without a bias).  Returns the kernels that ran."""
    dx, dw, dtop = dev(x), dev(wt), dev(top)
    kernels = set()
    for affine in AFFINES:
        use, bs = affine is not None, (None if affine == "fma" else bias)
        for act in ACTS:
            got = host(F.conv1x1_upsample_add(dx, dw, dev(bs), dev(a) if use else None, dev(b) if use else None, dtop, affine=affine,
                                              activation=act))
            kernels.add(_lib.last_kernel())
            want = P.oracle_lateral(x, wt, bs, a if use else None, b if use else None, top, CODE[affine], act)
            np.testing.assert_array_equal(got, want, err_msg=f"{what} affine={affine} act={act} [{_lib.last_kernel()}]")
    return kernels


# ---- the kernel against the oracle -------------------------------------------------------------------------------------------------
def _integer_rule_differs(n_in, n_out):
    """torch's CPU nearest index for n_in -> n_out is not the integer o * n_in // n_out."""
    want = nn.functional.interpolate(torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in), size=(1, n_out), mode="nearest")
    return not np.array_equal(np.arange(n_out) * n_in // n_out, want.reshape(-1).numpy().astype(np.int64))


@lru_cache(maxsize=None)
def _float_rule_pair(upsampling):
    """The smallest (out, in), out <= 140, at which the float rule differs from the integer one (a CPU search); upsampling: among
    the pairs with in < out, FPN's direction."""
    for n_out in range(1, 141):
        for n_in in range(1, n_out if upsampling else 141):
            if _integer_rule_differs(n_in, n_out):
                return n_in, n_out
    raise AssertionError("no (in, out) pair with out <= 140 separates the float rule from the integer rule")


COUTS, CINS = (31, 32, 33, 65, 129), (3, 32, 33)
OUTPUTS = ((1, 1), (5, 7), (8, 8), (9, 13), (25, 25))


def _top_sizes(h, w):
    sizes = {"equal": (h, w), "1x1": (1, 1), "larger than the output": (h + 3, 2 * w + 1), "ceil-half": ((h + 1) // 2, (w + 1) // 2)}
    if h % 2 == 0 and w % 2 == 0:
        sizes["exactly half"] = (h // 2, w // 2)
    return sizes


def _kernel_cases():
    """(h, w) x top size, with cout and cin dealt round-robin: 5 and 3 are coprime, so every (cout, cin) pair occurs."""
    cases, i = [], 0
    for h, w in OUTPUTS:
        for kind, top_hw in _top_sizes(h, w).items():
            cases.append((f"{h}x{w} top {kind} {top_hw[0]}x{top_hw[1]}", h, w, top_hw, COUTS[i % 5], CINS[i % 3]))
            i += 1
    assert {(c[4], c[5]) for c in cases} == {(co, ci) for co in COUTS for ci in CINS}
    assert ((25, 25), (13, 13)) in {((c[1], c[2]), c[3]) for c in cases} and ((9, 13), (5, 7)) in {((c[1], c[2]), c[3]) for c in cases}
    assert ((5, 7), (3, 4)) in {((c[1], c[2]), c[3]) for c in cases} and ((8, 8), (4, 4)) in {((c[1], c[2]), c[3]) for c in cases}
    return cases


KERNEL_CASES = _kernel_cases()


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_kernel_equals_the_oracle(case):
    what, h, w, top_hw, cout, cin = case
    x, wt, a, b, bias, top = _data(5100 + 7 * h + w + cout, 2, cin, h, w, cout, top_hw)
    kernels = _epilogues(x, wt, a, b, bias, top, f"{what} cout {cout} cin {cin}")
    assert all(k.startswith("k_conv1x1_up<") for k in kernels), kernels


@pytest.mark.parametrize("upsampling", [False, True], ids=["smallest pair", "smallest upsampling pair"])
@pytest.mark.parametrize("axis", ["rows", "columns"])
def test_source_index_is_the_float_rule_where_the_integer_rule_differs(axis, upsampling):
    n_in, n_out = _float_rule_pair(upsampling)
    assert _integer_rule_differs(n_in, n_out) and n_out <= 140
    (h, top_h), (w, top_w) = ((n_out, n_in), (7, 4)) if axis == "rows" else ((5, 3), (n_out, n_in))
    x, wt, a, b, bias, top = _data(5200, 2, 3, h, w, 33, (top_h, top_w))
    _epilogues(x, wt, a, b, bias, top, f"{top_h}x{top_w} -> {h}x{w}")


# ---- K slices inside the workgroup ---------------------------------------------------------------------------------------------------
def test_k_slice_instances_equal_the_sliced_oracle():
    """FPN's small levels (long K, a handful of workgroups) fall into the K-slice plan: one shape the library puts in 2 slices and
    one it puts in 4, against the oracle in that order."""
    seen = {}
    for cin in (256, 512):
        slices, sl = F.conv1x1_k_slices(1, cin, 7, 7, 256)
        x, wt, a, b, bias, top = _data(5300 + cin, 1, cin, 7, 7, 256, (4, 4))
        kernels = _epilogues(x, wt, a, b, bias, top, f"cin {cin}: {slices} slices of {sl}")
        assert kernels == {f"k_conv1x1_up<1,4,ks{slices}>"}, kernels
        seen[slices] = sl
    assert set(seen) == {2, 4}, seen


# ---- every instance the plan can pick has the gather ---------------------------------------------------------------------------------
# (n, cin, h, w, cout, top size): reached by shape, as the pointwise kernel's own tests reach them -- one K chunk -> <1,1>; cout
# <= 32 / <= 64 / more -> MW 1 / 2 / 4; more than 8192 wave tiles (32 channels x 32 pixels) -> NT 2, more than 32768 -> NT 4
# (MW 1 stays at 2); few workgroups and >= 6 / >= 12 chunks of 32 channels -> 2 / 4 K slices
INSTANCES = {
    "k_conv1x1_up<1,1>": (2, 3, 9, 13, 40, (5, 7)),
    "k_conv1x1_up<1,2>": (2, 33, 9, 13, 64, (5, 7)),
    "k_conv1x1_up<1,4>": (2, 33, 9, 13, 65, (5, 7)),
    "k_conv1x1_up<2,1>": (2, 33, 364, 364, 32, (183, 183)),
    "k_conv1x1_up<2,2>": (2, 33, 258, 258, 33, (129, 130)),
    "k_conv1x1_up<2,4>": (2, 33, 210, 210, 65, (106, 105)),
    "k_conv1x1_up<4,2>": (2, 33, 513, 513, 33, (257, 257)),
    "k_conv1x1_up<4,4>": (2, 33, 364, 364, 97, (182, 183)),
    "k_conv1x1_up<1,1,ks2>": (1, 192, 7, 7, 32, (4, 4)),
    "k_conv1x1_up<1,1,ks4>": (1, 384, 7, 7, 31, (4, 4)),
    "k_conv1x1_up<1,2,ks2>": (1, 192, 7, 7, 64, (4, 4)),
    "k_conv1x1_up<1,2,ks4>": (1, 384, 7, 7, 33, (4, 4)),
    "k_conv1x1_up<1,4,ks2>": (1, 192, 5, 7, 65, (3, 4)),
    "k_conv1x1_up<1,4,ks4>": (1, 384, 5, 7, 129, (3, 4)),
}


@pytest.mark.parametrize("kernel", list(INSTANCES))
def test_every_instance_gathers(kernel):
    """The large maps (NT 2 and 4 need tens of thousands of wave tiles) are compared with the oracle on the first and last
    channel of every 32-channel tile, and in all channels with the existing path on the GPU, F.conv_norm_act with the
    upsampled map as its residual -- which the pointwise kernel's own tests hold to the oracle."""
    n, cin, h, w, cout, top_hw = INSTANCES[kernel]
    x, wt, a, b, bias, top = _data(5400 + cout + h, n, cin, h, w, cout, top_hw)
    large = h * w > 4096
    channels = sorted({c for c in range(cout) if c % 32 in (0, 31)} | {cout - 1}) if large else None
    dx, dw, da, db, dtop = dev(x), dev(wt), dev(a), dev(b), dev(top)
    got = F.conv1x1_upsample_add(dx, dw, None, da, db, dtop, affine="fma", activation="relu")
    assert _lib.last_kernel() == kernel, _lib.last_kernel()
    sel = slice(None) if channels is None else np.asarray(channels)
    slices, sl = F.conv1x1_k_slices(n, cin, h, w, cout)
    want = P.oracle_lateral(x, np.ascontiguousarray(wt[sel]), None, a[sel], b[sel], np.ascontiguousarray(top[:, sel]), 2, "relu",
                            slice_len=sl if slices > 1 else 0)
    np.testing.assert_array_equal(host(got)[:, sel], want, err_msg=kernel)
    old = F.conv_norm_act(dx, dw, None, da, db, residual=nn.functional.interpolate(dtop, size=(h, w), mode="nearest"), affine="fma",
                          activation="relu")
    assert _lib.last_kernel() == kernel.replace("_up<", "<"), _lib.last_kernel()  # the same plan without the gather
    assert torch.equal(got, old), kernel


def test_nt4_through_the_long_k_rule():
    """128 channels on 2 x 184 x 184 with a long K (cin = 512: the launcher's wide-tile rule) is an NT = 4 launch too; all
    channels against the existing path, three against the oracle."""
    n, cin, h, w, cout = 2, 512, 184, 184, 128
    x, wt, a, b, bias, top = _data(5450, n, cin, h, w, cout, (92, 92))
    dx, dw, dbias, dtop = dev(x), dev(wt), dev(bias), dev(top)
    got = F.conv1x1_upsample_add(dx, dw, dbias, None, None, dtop)
    assert _lib.last_kernel() == "k_conv1x1_up<4,4>", _lib.last_kernel()
    old = F.conv_norm_act(dx, dw, dbias, residual=nn.functional.interpolate(dtop, size=(h, w), mode="nearest"))
    assert torch.equal(got, old)
    sel = np.asarray([0, 63, 127])
    want = P.oracle_lateral(x, np.ascontiguousarray(wt[sel]), bias[sel], None, None, np.ascontiguousarray(top[:, sel]), 0, None, slice_len=0)
    np.testing.assert_array_equal(host(got)[:, sel], want)


# ---- special values ------------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_come_out_where_the_oracle_puts_them():
    x, wt, a, b, bias, top = _data(5500, 2, 6, 9, 13, 33, (5, 7))
    x[0, 1, 0, 0], x[0, 2, 8, 12], x[1, 5, 4, 6], x[1, 0, 5, 5] = np.nan, np.inf, -np.inf, np.inf
    top[0, 3, 2, 2], top[1, 32, 4, 6], top[1, 2, 0, 0], top[0, 0, 4, 0] = np.nan, np.inf, -np.inf, np.inf
    _epilogues(x, wt, a, b, bias, top, "special values")
    want = P.oracle_lateral(x, wt, bias, None, None, top, 0, None)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()


# ---- equality with the existing path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 33, 9, 13, 65, (5, 7)), (2, 3, 8, 8, 31, (4, 4)), (2, 32, 25, 25, 129, (13, 13)), (1, 256, 7, 7, 256, (4, 4)),
                                   (2, 33, 5, 7, 33, (9, 11)), (2, 8, 6, 10, 16, (6, 10)), (2, 8, 6, 10, 16, (1, 1))], ids=str)
def test_same_bits_as_conv_norm_act_on_the_upsampled_map(shape):
    n, cin, h, w, cout, top_hw = shape
    x, wt, a, b, bias, top = _data(5600 + cout, n, cin, h, w, cout, top_hw)
    dx, dw, dtop = dev(x), dev(wt), dev(top)
    up = nn.functional.interpolate(dtop, size=(h, w), mode="nearest")
    np.testing.assert_array_equal(host(up), P.nearest(top, (h, w)))  # torch's GPU index is its CPU index
    for affine in AFFINES:
        use, bs = affine is not None, (None if affine == "fma" else bias)
        for act in ACTS:
            args = (dx, dw, dev(bs), dev(a) if use else None, dev(b) if use else None)
            new = F.conv1x1_upsample_add(*args, dtop, affine=affine, activation=act)
            old = F.conv_norm_act(*args, residual=up, affine=affine, activation=act)
            assert torch.equal(new, old), (shape, affine, act)


def test_python_checks_on_the_device():
    x, wt, top = torch.zeros(2, 4, 5, 7, device="cuda"), torch.zeros(8, 4, 1, 1, device="cuda"), torch.zeros(2, 8, 3, 4, device="cuda")
    assert F.conv1x1_upsample_add(x[:0], wt, top=top[:0]).shape == (0, 8, 5, 7)
    with pytest.raises(Exception, match="(?i)gpu|device|cuda"):
        F.conv1x1_upsample_add(x, wt, top=top.cpu())
    with pytest.raises(TypeError, match="float32"):
        F.conv1x1_upsample_add(x.double(), wt.double(), top=top)
    y = F.conv1x1_upsample_add(x, wt, top=top.requires_grad_())
    with pytest.raises(RuntimeError, match="forward-only"):
        y.sum().backward()
    strided = torch.zeros(2, 8, 3, 8, device="cuda")[..., ::2]  # a non-contiguous top is made contiguous, not misread
    strided.copy_(torch.rand(2, 8, 3, 4))
    assert torch.equal(F.conv1x1_upsample_add(x, wt, top=strided), nn.functional.interpolate(strided, size=(5, 7), mode="nearest"))


# ---- F.max_pool2d(kernel 1, stride 2): LastLevelMaxPool's call -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 3, 4), (2, 3, 1, 1), (1, 2, 8, 8), (3, 5, 7), (2, 16, 25, 26)], ids=str)
def test_max_pool_kernel_1_stride_2_equals_torch_cpu(shape):
    x = philox_f32(5700 + shape[-1], shape) * 4 - 2
    x.reshape(-1)[::5] = np.nan
    x.reshape(-1)[1::7] = -np.inf
    got = host(F.max_pool2d(dev(x), 1, 2, 0))
    assert _lib.last_kernel() == "k_maxpool2d"
    np.testing.assert_array_equal(got, nn.functional.max_pool2d(torch.from_numpy(x), kernel_size=1, stride=2, padding=0).numpy())


# ---- the modules ---------------------------------------------------------------------------------------------------------------------
COUNTED = ("conv_norm_act", "conv1x1_upsample_add", "conv2d_bias_relu", "conv2d_affine_act", "conv2d_bias_act", "max_pool2d")


def _counting(module, x, launches):
    """module(x), recording the library calls made through the functional layer (tests/test_gpu_resnet.py::_counting)."""
    originals = {n: getattr(F, n) for n in COUNTED}

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


NORMS = {"no norm": None, "FrozenBatchNorm2d": FrozenBatchNorm2d, "BatchNorm2d": nn.BatchNorm2d}
EXTRAS = {
    "no extra block": (lambda: None, [], 0),
    "LastLevelMaxPool": (fpn.LastLevelMaxPool, ["pool"], 1),
    "LastLevelP6P7 on P5": (lambda: fpn.LastLevelP6P7(16, 16), ["p6", "p7"], 2),
    "LastLevelP6P7 on C5": (lambda: fpn.LastLevelP6P7(32, 16), ["p6", "p7"], 2),
}
MAPS = OrderedDict([("feat0", (8, 9, 13)), ("feat2", (16, 5, 7)), ("feat3", (32, 3, 4))])


@lru_cache(maxsize=None)
def _feature_maps():
    return OrderedDict((k, philox_f32(5800 + i, (2,) + s) * 2 - 1) for i, (k, s) in enumerate(MAPS.items()))


@pytest.mark.parametrize("extra", list(EXTRAS))
@pytest.mark.parametrize("norm", list(NORMS))
def test_fpn_equals_the_oracle_composition(norm, extra):
    make_extra, extra_names, extra_launches = EXTRAS[extra]
    torch.manual_seed(61)
    model = fpn.FeaturePyramidNetwork([8, 16, 32], 16, extra_blocks=make_extra(), norm_layer=NORMS[norm])
    P.randomize(model, 63)
    feats = _feature_maps()
    want = P.oracle_fpn(model, feats)
    launches = []
    got = _counting(model.cuda(), OrderedDict((k, dev(v)) for k, v in feats.items()), launches)
    assert isinstance(got, OrderedDict) and list(got) == list(want) == list(MAPS) + extra_names
    for k in want:
        np.testing.assert_array_equal(host(got[k]), want[k], err_msg=f"{norm}, {extra}: level {k}")
    levels = len(MAPS)
    assert len(launches) == 2 * levels + extra_launches, launches
    assert launches.count("conv1x1_upsample_add") == levels - 1 and launches[0] == "conv_norm_act"
    assert launches.count("conv2d_bias_relu" if norm == "no norm" else "conv2d_affine_act") >= levels
    assert tuple(got["feat0"].shape) == (2, 16, 9, 13) and tuple(got[list(got)[-1]].shape[:2]) == (2, 16)
    assert all(np.abs(v).max() > 1e-3 for v in want.values())


def test_fpn_is_the_references_network():
    """torch's own float32 forward of the replica on the CPU, to float32 accuracy: the composition is the reference's."""
    torch.manual_seed(65)
    replica = P.FeaturePyramidNetwork([8, 16, 32], 16, extra_blocks=P.LastLevelMaxPool(), norm_layer=nn.BatchNorm2d).eval()
    P.randomize(replica, 67)
    model = fpn.FeaturePyramidNetwork([8, 16, 32], 16, extra_blocks=fpn.LastLevelMaxPool(), norm_layer=nn.BatchNorm2d)
    model.load_state_dict(replica.state_dict(), strict=True)
    feats = _feature_maps()
    with torch.no_grad():
        want = replica(OrderedDict((k, torch.from_numpy(v)) for k, v in feats.items()))
    got = model.cuda()(OrderedDict((k, dev(v)) for k, v in feats.items()))
    assert list(got) == list(want)
    for k in want:
        np.testing.assert_allclose(host(got[k]), want[k].numpy(), rtol=1e-4, atol=1e-5 * float(want[k].abs().max()), err_msg=k)


# ---- backbones -----------------------------------------------------------------------------------------------------------------------
IMAGE = (2, 3, 72, 104)  # levels 18 x 26, 9 x 13, 5 x 7, 3 x 4 and the pool 2 x 2: no merge is an exact 2x


def _backbone_pair(name, **kw):
    """(the library's backbone with the replica's parameters, still on the CPU; the input batch)."""
    torch.manual_seed(71)
    replica_kw = dict(kw)
    if "extra_blocks" in kw:
        replica_kw["extra_blocks"] = P.LastLevelP6P7(256, 256)
    replica = P.resnet_fpn_backbone(backbone_name=name, **replica_kw).eval()
    P.randomize(replica, 73)
    model = mv.resnet_fpn_backbone(backbone_name=name, **kw)
    model.load_state_dict(replica.state_dict(), strict=True)
    return model, philox_f32(5900, IMAGE) * 2 - 1


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_backbone_equals_the_oracle_composition(name):
    model, x = _backbone_pair(name)
    want = P.oracle_backbone(model, x)
    model = model.cuda()
    got = model(dev(x))
    assert list(got) == list(want) == ["0", "1", "2", "3", "pool"]
    assert [tuple(v.shape) for v in got.values()] == [(2, 256, 18, 26), (2, 256, 9, 13), (2, 256, 5, 7), (2, 256, 3, 4), (2, 256, 2, 2)]
    for k in want:
        assert np.isfinite(want[k]).all() and np.abs(want[k]).max() > 1e-3
        np.testing.assert_array_equal(host(got[k]), want[k], err_msg=f"{name}: level {k}")
    if name != "resnet18":
        return
    # and the pyramid feeds the pooler: the same call on the oracle's pyramid moved to the GPU
    boxes = [torch.tensor([[3.0, 4.0, 60.0, 50.0], [10.5, 2.25, 100.0, 70.0], [40.0, 30.0, 47.0, 39.0]], device="cuda"),
             torch.tensor([[0.0, 0.0, 104.0, 72.0], [55.0, 11.0, 80.5, 33.0]], device="cuda")]
    sizes = [(72, 104), (72, 104)]
    pooler = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    ours = pooler(got, boxes, sizes)
    theirs = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)(OrderedDict((k, dev(v)) for k, v in want.items()), boxes, sizes)
    assert tuple(ours.shape) == (5, 256, 7, 7) and torch.equal(ours, theirs) and float(ours.detach().abs().max()) > 1e-3


def test_backbone_with_three_returned_layers_and_p6p7():
    model, x = _backbone_pair("resnet18", returned_layers=[2, 3, 4], extra_blocks=fpn.LastLevelP6P7(256, 256))
    want = P.oracle_backbone(model, x)
    got = model.cuda()(dev(x))
    assert list(got) == list(want) == ["0", "1", "2", "p6", "p7"]
    assert [tuple(v.shape[-2:]) for v in got.values()] == [(9, 13), (5, 7), (3, 4), (2, 2), (1, 1)]
    for k in want:
        np.testing.assert_array_equal(host(got[k]), want[k], err_msg=f"level {k}")
