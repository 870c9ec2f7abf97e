"""LRASPP and DeepLabV3-MobileNetV3 on the GPU (`-m gpu`), bit for bit against tests/_lraspp_ref.py:

  * the depthwise 5x5 conv at dilation 2 (k_dwpc5x5<1, 2>) against the oracle on the zero-stuffed kernel (the host tests show that oracle
    equal to the oracle's own dilated conv): maps down to 1 x 1, ragged widths, several strips of each row parity, both sides of the
    short-launch rule, the epilogue cross, NaN / Inf at one pixel, and dilation 1 of the new entry being the old entry;
  * F.conv1x1_gated_upsample against its restatement and against the library's own unfused composition;
  * LRASPPHead stage by stage, the dilated MobileNetV3s' features element by element, and the whole models stage by stage, their
    labels(), and the project's accuracy condition against the float64 evaluation of the torch replica.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from tests import _lraspp_ref as R  # noqa: E402
from tests import _mobilenetv3_ref as MR  # noqa: E402

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
ACTS = [None, "relu", "relu6", "hardswish", "silu"]
AFFINE = {None: 0, "mul_add": 1, "fma": 2}
DTYPES = [torch.int64, torch.uint8]


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dw(x, w, bias=None, alpha=None, beta=None, res=None, affine=None, act=None):
    return F.conv_norm_act(_cuda(x), _cuda(w), _cuda(bias), _cuda(alpha), _cuda(beta), _cuda(res), stride=1, groups=x.shape[1],
                           affine=affine, activation=act, dilation=2)


# ---- the dilated depthwise conv ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.DW_SHAPES + [R.DW_LONG], ids=str)
def test_dilated_depthwise_equals_the_oracle(shape):
    x, w, bias, alpha, beta, res = R.dw_inputs(shape)
    got = _dw(x, w, None, alpha, beta, res, "fma", "hardswish")
    n, c, h, wd = shape
    # the launcher's strip rule, restated: 8 rows per parity unless that leaves fewer than 16384 threads
    threads = n * c * 2 * -(-h // 16) * -(-wd // 4)
    assert _lib.last_kernel() == f"k_dwpc5x5<s1,d2,rows{8 if threads >= 16384 else 4}>", _lib.last_kernel()
    assert (shape == R.DW_LONG) == (threads >= 16384)
    R.same(got, R.dw_dilated(x, w, None, alpha, beta, res, 2, "hardswish"), f"dilated dw {shape}")
    R.same(_dw(x, w), R.dw_dilated(x, w), f"dilated dw {shape}, no epilogue")
    if shape == (1, 1, 19, 5):
        assert -(-h // 8) == 3  # three row blocks: a column has three strips of each parity


def test_dilated_depthwise_does_not_depend_on_alignment_or_batch():
    shape = (3, 2, 13, 14)
    x, w, bias, alpha, beta, res = R.dw_inputs(shape)
    want = R.dw_dilated(x, w, bias, alpha, beta, res, 1, "relu")
    R.same(_dw(x, w, bias, alpha, beta, res, "mul_add", "relu"), want, "whole batch")
    for i in range(3):  # an image alone, read at a 4-byte offset from the batch's allocation
        xd = _cuda(x)[i:i + 1]
        got = F.conv_norm_act(xd, _cuda(w), _cuda(bias), _cuda(alpha), _cuda(beta), _cuda(res[i:i + 1]), stride=1, groups=2, affine="mul_add",
                              activation="relu", dilation=2)
        R.same(got, want[i:i + 1], f"image {i} alone")
    flat = torch.zeros(x.size + 1, device=DEV)
    flat[1:] = _cuda(x).flatten()
    got = F.conv_norm_act(flat[1:].view(shape), _cuda(w), _cuda(bias), _cuda(alpha), _cuda(beta), _cuda(res), stride=1, groups=2,
                          affine="mul_add", activation="relu", dilation=2)
    R.same(got, want, "x at a 4-byte offset")


@pytest.mark.parametrize("affine", [None, "mul_add", "fma"])
def test_dilated_depthwise_epilogue_cross(affine):
    shape = (2, 3, 9, 6)
    x, w, bias, alpha, beta, res = R.dw_inputs(shape, seed=1)
    if affine is None:
        alpha = beta = None
    for act in ACTS:
        for b in (None, bias):
            for r in (None, res):
                got, want = _dw(x, w, b, alpha, beta, r, affine, act), R.dw_dilated(x, w, b, alpha, beta, r, AFFINE[affine], act)
                if act == "silu":  # expf: last-ulp differences from the CPU's (the tolerance of tests/test_gpu_mobilenetv3.py)
                    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-6, atol=1e-7)
                else:
                    R.same(got, want, f"dilated dw epilogue {affine} {act} bias={b is not None} res={r is not None}")


@pytest.mark.parametrize("value", [NAN, INF, -INF], ids=["nan", "inf", "-inf"])
def test_a_nan_or_inf_pixel_reaches_its_25_outputs(value):
    shape = (1, 2, 13, 14)
    x, w = R.dw_inputs(shape, seed=2)[:2]
    assert (w != 0).all()
    x[0, 1, 6, 7] = value
    got = _dw(x, w).cpu().numpy()
    want = R.dw_dilated_select(x, w)
    MR.same(got, want, f"dilated dw with {value}")
    hit = ~np.isfinite(got)
    expect = np.zeros(shape, bool)
    for dy in (-4, -2, 0, 2, 4):
        for dx in (-4, -2, 0, 2, 4):
            expect[0, 1, 6 + dy, 7 + dx] = True
    assert np.array_equal(hit, expect) and hit.sum() == 25


def test_dilation_1_of_the_new_entry_is_the_old_entry():
    lib = _lib.load()
    for shape, k, stride in (((2, 3, 9, 7), 5, 1), ((2, 3, 9, 7), 5, 2), ((1, 4, 7, 9), 3, 1), ((1, 4, 7, 9), 3, 2)):
        n, c, h, w = shape
        g = R.rng(7100 + k + stride)
        x, wt = _cuda(g.standard_normal(shape, dtype=np.float32)), _cuda(g.standard_normal((c, 1, k, k), dtype=np.float32))
        al, be = _cuda(g.random(c, dtype=np.float32) + 0.5), _cuda(g.standard_normal(c, dtype=np.float32))
        oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
        y_old, y_new = torch.zeros(n, c, oh, ow, device=DEV), torch.zeros(n, c, oh, ow, device=DEV)
        s = _lib.stream_ptr(x)
        rc = lib.mv_dwconv_norm_act_f32(x.data_ptr(), wt.data_ptr(), None, al.data_ptr(), be.data_ptr(), None, y_old.data_ptr(), n, c, h, w, k,
                                        stride, 2, 3, s)
        assert rc == 0, lib.mv_last_error()
        old_kernel = _lib.last_kernel()
        rc = lib.mv_dwconv_dilated_norm_act_f32(x.data_ptr(), wt.data_ptr(), None, al.data_ptr(), be.data_ptr(), None, y_new.data_ptr(), n, c,
                                                h, w, k, stride, 1, 2, 3, s)
        assert rc == 0, lib.mv_last_error()
        assert _lib.last_kernel() == old_kernel and "d2" not in old_kernel
        MR.same(y_new, y_old, f"dilation 1, kernel {k}, stride {stride}")
        assert bool(y_old.any())


# ---- the fused head launch ---------------------------------------------------------------------------------------------------------------
def _gu(x, gate, w, bias, res, size):
    return F.conv1x1_gated_upsample(_cuda(x), _cuda(gate), _cuda(w), _cuda(bias), _cuda(res), size=size)


def _unfused(x, gate, w, bias, res, size):
    return F.conv_norm_act(F.interpolate(F.se_scale(_cuda(x), _cuda(gate)), size=size), _cuda(w), _cuda(bias), residual=_cuda(res))


@pytest.mark.parametrize("case", R.GU_CASES, ids=str)
def test_gated_upsample_equals_the_restatement_and_the_composition(case):
    (n, cin, h, wd), (oh, ow), cout = case
    x, gate, w, bias, res = R.gu_inputs(case)
    slices = F.conv1x1_k_slices(n, cin, oh, ow, cout)[0]
    if case == R.GU_CASES[R.GU_SLICED]:
        assert slices > 1
    for b in (bias, None):
        for r in (res, None):
            got = _gu(x, gate, w, b, r, (oh, ow))
            assert _lib.last_kernel().startswith("k_conv1x1_gu<"), _lib.last_kernel()
            assert ("ks" in _lib.last_kernel()) == (slices > 1)
            assert tuple(got.shape) == (n, cout, oh, ow)
            what = f"gated upsample {case} bias={b is not None} res={r is not None}"
            R.same(got, R.gated_upsample(x, gate, w, b, r, oh, ow), what)
            R.same(got, _unfused(x, gate, w, b, r, (oh, ow)), what + " vs the composition")
    got = _gu(x, gate.reshape(n, cin, 1, 1), w, bias, res, (oh, ow))  # the gate as (N, C, 1, 1)
    R.same(got, R.gated_upsample(x, gate, w, bias, res, oh, ow), "gate (N, C, 1, 1)")


def test_gated_upsample_with_nan_and_inf():
    case = ((2, 5, 3, 4), (5, 7), 3)
    x, gate, w, bias, res = R.gu_inputs(case, seed=1)
    x[0, 1, 1, 2], x[0, 3, 0, 0], x[1, 2, 2, 3] = NAN, INF, -INF
    got = _gu(x, gate, w, bias, res, (5, 7))
    R.same(got, _unfused(x, gate, w, bias, res, (5, 7)), "x with NaN and +-Inf vs the composition")
    R.same(got, R.gated_upsample(x, gate, w, bias, res, 5, 7), "x with NaN and +-Inf")
    assert bool(torch.isnan(got).any()) and bool(torch.isfinite(got).any())
    x = R.gu_inputs(case, seed=1)[0]
    gate[0, 0], gate[0, 2], gate[1, 4] = 0.0, INF, NAN
    got = _gu(x, gate, w, bias, res, (5, 7))
    R.same(got, _unfused(x, gate, w, bias, res, (5, 7)), "gate with 0, Inf and NaN vs the composition")
    R.same(got, R.gated_upsample(x, gate, w, bias, res, 5, 7), "gate with 0, Inf and NaN")
    assert bool(torch.isnan(got[1]).all())


# ---- modules -------------------------------------------------------------------------------------------------------------------------------
def _hooked(dev, modules, x):
    outs = {}
    hooks = [m.register_forward_hook(lambda m_, _i, o: outs.__setitem__(id(m_), o)) for m in modules]
    with torch.no_grad():
        y = dev(x)
    for hk in hooks:
        hk.remove()
    return outs, y


def test_lraspp_head_stage_by_stage():
    torch.manual_seed(300)
    cpu = mv.LRASPPHead(4, 8, 3, 6)
    MR.perturb(cpu, 301)
    dev = mv.LRASPPHead(4, 8, 3, 6)
    dev.load_state_dict(cpu.state_dict())
    dev = dev.to(DEV)
    low, high = R.rng(302).standard_normal((2, 4, 9, 11), dtype=np.float32), R.rng(303).standard_normal((2, 8, 5, 6), dtype=np.float32)
    cbr, pooled, gate, lowc, out = R.lraspp_head_stages(cpu, low, high)
    with torch.no_grad():
        got = dev({"low": _cuda(low), "high": _cuda(high)})
        assert _lib.last_kernel().startswith("k_conv1x1_gu<"), _lib.last_kernel()
        g_pool = F.global_avg_pool(_cuda(high))
        g_gate = F.linear_act(g_pool, dev.scale[1].weight, None, "sigmoid")
        g_cbr = mv.resnet.fused_conv_norm(_cuda(high), dev.cbr[0], dev.cbr[1], dev._fold, relu=True)
        g_low = F.conv_norm_act(_cuda(low), dev.low_classifier.weight, dev.low_classifier.bias)
    for g, wnt, what in ((g_cbr, cbr, "cbr"), (g_pool, pooled, "pool"), (g_gate, gate, "gate"), (g_low, lowc, "low classifier"), (got, out, "output")):
        R.same(g, wnt, "LRASPPHead " + what)
    assert tuple(got.shape) == (2, 3, 9, 11)


@pytest.mark.parametrize("arch", ["mobilenet_v3_small", "mobilenet_v3_large"])
def test_dilated_features_element_by_element(arch):
    torch.manual_seed(310)
    cpu = getattr(mv, arch)(num_classes=3, dilated=True)
    MR.perturb(cpu, 311)
    dev = getattr(mv, arch)(num_classes=3, dilated=True)
    dev.load_state_dict(cpu.state_dict())
    dev = dev.to(DEV)
    x = R.rng(312).standard_normal((1, 3, 64, 64), dtype=np.float32)
    want = R.features_stages(cpu.features, x)
    outs, y = _hooked(dev.features, list(dev.features), _cuda(x))
    assert len(outs) == len(want) == len(dev.features)
    dilated = 0
    for i, (m, wnt) in enumerate(zip(dev.features, want)):
        R.same(outs[id(m)], wnt, f"{arch} features.{i}")
        dilated += bool(getattr(m, "_dilated", False))
    assert dilated == 3 and tuple(y.shape[-2:]) == (4, 4)  # output stride 16
    with pytest.raises(NotImplementedError, match="segmentation backbone"):
        dev(_cuda(x))


MODELS = {"lraspp": ("lraspp_mobilenet_v3_large", {}, (1, 3, 40, 56)), "lraspp-33": ("lraspp_mobilenet_v3_large", {}, (1, 3, 33, 33)),
          "deeplabv3": ("deeplabv3_mobilenet_v3_large", {"aux_loss": True}, (1, 3, 33, 33))}
_CASES = {}


def _case(which):
    """One model, input, stage-by-stage reference and hooked device forward per `which`, computed once for the tests below."""
    if which not in _CASES:
        name, kw, shape = MODELS[which]
        torch.manual_seed(400)
        rep = R.replica(name, num_classes=3, **kw)
        x = R.rng(401).standard_normal(shape, dtype=np.float32)
        R.perturb(rep, 402, x)
        cpu, dev = getattr(mv, name)(num_classes=3, **kw), getattr(mv, name)(num_classes=3, **kw)
        cpu.load_state_dict(rep.state_dict())
        dev.load_state_dict(rep.state_dict())
        dev = dev.to(DEV)
        mods = [dev.backbone, dev.classifier] + ([dev.aux_classifier] if kw else [])
        outs, got = _hooked(dev, mods, _cuda(x))
        _CASES[which] = dict(rep=rep, dev=dev, x=x, want=R.model_stages(cpu, x), outs=outs, got=got)
    return _CASES[which]


@pytest.mark.parametrize("which", list(MODELS))
def test_model_stage_by_stage_and_labels(which):
    """Backbone features, the heads' outputs and the resized logits bit for bit against the stage-by-stage reference; labels(x) ==
    forward(x)["out"].argmax(1) for both dtypes; a model in training mode raises."""
    c = _case(which)
    dev, want, outs, got, shape = c["dev"], c["want"], c["outs"], c["got"], MODELS[which][2]
    feats = outs[id(dev.backbone)]
    assert set(feats) == set(want["features"])
    for k in feats:
        R.same(feats[k], want["features"][k], f"{which} backbone {k}")
    R.same(outs[id(dev.classifier)], want["out_stages"][-1], f"{which} classifier")
    keys = ["out"] + (["aux"] if "aux" in want else [])
    assert list(got) == keys
    if "aux" in want:
        R.same(outs[id(dev.aux_classifier)], want["aux_stages"][-1], f"{which} aux classifier")
    for k in keys:
        assert tuple(got[k].shape) == (shape[0], 3) + shape[2:]
        R.same(got[k], want[k], f"{which} {k}")
    xd = _cuda(c["x"])
    composed = got["out"].argmax(1)
    for dtype in DTYPES:
        labels = dev.labels(xd, dtype=dtype)
        assert labels.dtype == dtype and tuple(labels.shape) == (shape[0],) + shape[2:]
        assert _lib.last_kernel().startswith("k_interp_argmax<"), _lib.last_kernel()
        assert torch.equal(labels.to(torch.int64), composed)
    assert len(torch.unique(composed)) > 1  # not one class everywhere
    dev.train()
    try:
        with pytest.raises(RuntimeError, match="inference only"):
            dev(xd)
        with pytest.raises(RuntimeError, match="inference only"):
            dev.labels(xd)
    finally:
        dev.eval()


@pytest.mark.parametrize("which", list(MODELS))
def test_model_accuracy_condition(which):
    """Every output against the float64 evaluation of the torch replica within the project's condition (tests/test_gpu_mobilenetv3.py):
    the library's max error <= 2 x the float32 replica's + 2^-22 max |f64|.

    Measured on an MI355X host, in units of 2^-24 max |f64| (library / float32 replica; bound): lraspp at 40 x 56 out 40.95 / 233.77
    (471.5), at 33 x 33 out 43.64 / 153.08 (310.2); deeplabv3 out 21.11 / 24.87 (53.7), aux 12.49 / 10.03 (24.1).  The state's last
    biases are moved so that every class has the same mean logit (tests/_lraspp_ref.perturb), which makes max |f64| small (0.04 - 0.1)
    and the figures of both sides large."""
    c = _case(which)
    x = torch.from_numpy(c["x"])
    with torch.no_grad():
        t32 = c["rep"](x)
        f64 = copy.deepcopy(c["rep"]).double()(x.double())
    inside = []
    for k in t32:
        scale = float(f64[k].abs().max())
        e_lib, e_t = float((c["got"][k].cpu().double() - f64[k]).abs().max()), float((t32[k].double() - f64[k]).abs().max())
        print(f"{which} {k}: library {e_lib / scale * 2 ** 24:.2f}, torch float32 replica {e_t / scale * 2 ** 24:.2f} "
              f"(x 2^-24 max|f64| = {scale:.3g})")
        inside.append(e_lib <= 2 * e_t + 2.0 ** -22 * scale)
    assert all(inside), inside
