"""SSDlite on the GPU (`-m gpu`): F.dwconv_pointwise (csrc/convnorm.hip, k_conv1x1_dw) against the two F.conv_norm_act launches it
replaces by bit pattern and against the composition of the CPU oracle, a seeded sweep, special values, SSDLiteHead,
SSDLiteFeatureExtractorMobileNet and ssdlite320_mobilenet_v3_large stage by stage (the references of tests/_ssd_ref.py and
tests/_ssdlite_ref.py on the CPU)."""
import functools
import itertools
import re

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd import ssdlite as SL  # noqa: E402
from cpu_vision_amd.anchor_utils import DefaultBoxGenerator  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _fuzz_cases as FC  # noqa: E402
from tests import _mobilenetv3_ref as MR  # noqa: E402
from tests import _ssd_ref as R  # noqa: E402
from tests import _ssdlite_ref as RL  # noqa: E402
from tests._util import philox_f32  # noqa: E402

NAN, INF = float("nan"), float("inf")
AFF = {None: 0, "mul_add": 1, "fma": 2}
ACTS = (None, "relu", "relu6", "hardswish")
TILE = 32  # the side of the MFMA tile: pixels and channels per wave tile


def _randn(seed, shape, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------ the plan, restated on the host
KPK = FC.constant("kPK", "convnorm.hip")
COUT_STEPS = FC.pointwise_cout_steps()  # (32, 64): up to these the workgroup has 1 and 2 channel tiles (MW), 4 above


@functools.lru_cache(maxsize=None)
def _plan_numbers():
    """The thresholds of pw_plan in convnorm.hip: (wave tiles up to which NT = 1, up to which NT = 2, the workgroups up to which K is
    sliced, the chunks from which KS = 2 and KS = 4)."""
    src = (FC.CSRC / "convnorm.hip").read_text()
    a = re.search(r"p\.nt = wave_tiles <= (\d+) \? 1 : \(\(wave_tiles <= (\d+) \|\| p\.mw == 1\) \? 2 : 4\)", src)
    b = re.search(r"if \(p\.nt == 1 && workgroups <= (\d+) && chunks >= (\d+)\) p\.ks = chunks >= (\d+) \? 4 : 2;", src)
    assert a and b, "the pointwise plan was not found in convnorm.hip"
    return tuple(int(v) for v in a.groups() + b.groups())


def _plan(n, cin, hw, cout):
    """(NT, MW, KS) of pw_plan; every run asserts that the launched instance is the one stated here."""
    nt1, nt2, max_wg, ks2, ks4 = _plan_numbers()
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    mw = 1 if cout <= COUT_STEPS[0] else (2 if cout <= COUT_STEPS[1] else 4)
    wave_tiles = cdiv(cout, TILE) * cdiv(hw, TILE) * n
    nt = 1 if wave_tiles <= nt1 else (2 if (wave_tiles <= nt2 or mw == 1) else 4)
    if cin >= 512 and mw == 4:  # long K: wider pixel tiles while two workgroups per CU remain
        mb = cdiv(cout, 4 * TILE)
        if mb * cdiv(hw, 4 * TILE) * n >= 512:
            nt = 4
        elif mb * cdiv(hw, 2 * TILE) * n >= 512:
            nt = 2
    chunks = cdiv(cin, KPK)
    if chunks == 1:
        mw, nt = 1, 1
    pxb = (4 // mw) * nt * TILE
    workgroups = cdiv(cout, mw * TILE) * cdiv(hw, pxb) * n
    ks = 1
    if nt == 1 and workgroups <= max_wg and chunks >= ks2:
        ks = 4 if chunks >= ks4 else 2
    return nt, mw, ks


def _instance(n, cin, h, w, cout, stride):
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    nt, mw, ks = _plan(n, cin, oh * ow, cout)
    return f"k_conv1x1_dw<1,{mw},ks{ks}>" if ks > 1 else f"k_conv1x1_dw<{nt},{mw}>"


# what convnorm.hip instantiates: NT generic at KS = 1 (MW = 1 has no NT = 4), NT = 1 at KS = 2 and 4
INSTANCES = {f"k_conv1x1_dw<{nt},{mw}>" for nt, mw in ((1, 1), (2, 1), (1, 2), (2, 2), (4, 2), (1, 4), (2, 4), (4, 4))} | \
    {f"k_conv1x1_dw<1,{mw},ks{ks}>" for mw in (1, 2, 4) for ks in (2, 4)}


# ------------------------------------------------------------------------------------------------ one case: data, the three results
def _terms(seed, c, affine, bias):
    """(bias, alpha, beta) of one stage."""
    b = _randn(seed, (c,), 0.5) if bias else None
    if affine is None:
        return b, None, None
    return b, _randn(seed + 1, (c,), 0.3) + 1.2, _randn(seed + 2, (c,), 0.4)


def _data(seed, n, cin, h, w, cout, stride, dw_bias, dw_affine, bias, affine, residual):
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    d = {"x": _randn(seed, (n, cin, h, w)), "dw": _randn(seed + 1, (cin, 1, 3, 3), 0.4), "w": _randn(seed + 2, (cout, cin, 1, 1), 1.0 / (cin ** 0.5))}
    d["dw_bias"], d["dw_alpha"], d["dw_beta"] = _terms(seed + 10, cin, dw_affine, dw_bias)
    d["bias"], d["alpha"], d["beta"] = _terms(seed + 20, cout, affine, bias)
    d["res"] = _randn(seed + 30, (n, cout, oh, ow)) if residual else None
    return d


def _cuda(d):
    return {k: None if v is None else v.cuda() for k, v in d.items()}


def _fused(g, stride, dw_affine, dw_act, affine, act):
    return F.dwconv_pointwise(g["x"], g["dw"], g["dw_bias"], g["dw_alpha"], g["dw_beta"], g["w"], g["bias"], g["alpha"], g["beta"], g["res"],
                              stride=stride, dw_affine=dw_affine, dw_activation=dw_act, affine=affine, activation=act)


def _composed(g, stride, dw_affine, dw_act, affine, act):
    """The two launches the fused call replaces."""
    hidden = F.conv_norm_act(g["x"], g["dw"], g["dw_bias"], g["dw_alpha"], g["dw_beta"], stride=stride, groups=int(g["x"].shape[1]),
                             affine=dw_affine, activation=dw_act)
    return F.conv_norm_act(hidden, g["w"], g["bias"], g["alpha"], g["beta"], g["res"], affine=affine, activation=act)


def _np(t):
    return None if t is None else t.numpy()


def _oracle(d, stride, dw_affine, dw_act, affine, act, plan_n=None):
    """The oracle's composition: the depthwise stage, then the pointwise stage in the order F.conv1x1_k_slices states (for a batch of
    plan_n images when `d` holds only some of them)."""
    n, cin, h, w = d["x"].shape
    cout = d["w"].shape[0]
    hidden = ref.conv2d_affine_act(_np(d["x"]), _np(d["dw"]), _np(d["dw_bias"]), _np(d["dw_alpha"]), _np(d["dw_beta"]), None, stride, 1, cin,
                                   AFF[dw_affine], dw_act)
    oh, ow = hidden.shape[2:]
    slices, sl = F.conv1x1_k_slices(plan_n or n, cin, oh, ow, cout)
    return ref.conv2d_affine_act(hidden, _np(d["w"]), _np(d["bias"]), _np(d["alpha"]), _np(d["beta"]), _np(d["res"]), 1, 0, 1, AFF[affine], act,
                                 slice_len=sl if slices > 1 else 0)


def _same_bits(got, want, what):
    a, b = got.detach().contiguous().view(torch.int32), want.detach().contiguous().view(torch.int32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not torch.equal(a, b):
        bad = (a != b).reshape(-1)
        first = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits, first at flat index {first}: "
                             f"{got.reshape(-1)[first].item()!r} against {want.reshape(-1)[first].item()!r}")


def _run(shape, seed, epi, oracle=True):
    """One shape with one epilogue (dw_bias, dw_affine, dw_act, bias, affine, residual, act): the launched instance, the composition by
    bit pattern, the oracle's composition."""
    n, cin, h, w, cout, stride = shape
    dw_bias, dw_affine, dw_act, bias, affine, residual, act = epi
    d = _data(seed, n, cin, h, w, cout, stride, dw_bias, dw_affine, bias, affine, residual)
    g = _cuda(d)
    got = _fused(g, stride, dw_affine, dw_act, affine, act)
    name = _lib.last_kernel()
    what = f"{shape} {epi}"
    assert name == _instance(*shape) and name in INSTANCES, (what, name, _instance(*shape))
    _same_bits(got, _composed(g, stride, dw_affine, dw_act, affine, act), what + " against the composition")
    if oracle:
        R.same(got, torch.from_numpy(_oracle(d, stride, dw_affine, dw_act, affine, act)), what + " against the oracle")
    return name


# ------------------------------------------------------------------------------------------------ 1. shapes
def _boundary_shapes():
    """(n, cin, h, w, cout, stride): the smallest shapes that can go wrong."""
    nt1, nt2, max_wg, ks2, ks4 = _plan_numbers()
    shapes = [(1, 1, 1, 1, 1, 1), (2, 3, 2, 2, 5, 2), (1, 31, 3, 3, 24, 2), (2, 33, 5, 5, 33, 1), (1, 64, 3, 5, 65, 1), (1, 40, 7, 6, 24, 2)]
    shapes += [(1, 5, 1, 31, 7, 1), (1, 5, 4, 8, 7, 1), (1, 5, 3, 11, 7, 1)]  # a plane of 31, 32 and 33 output pixels
    # below, at and above each pixel-block size PXB = (4 / MW) NT 32 of the NT = 1 instances (cin > kPK: MW follows cout), at stride 1 and,
    # for the plane AT the size, also as the output of a stride-2 conv
    for mw, cout in ((1, 24), (2, 40), (4, 72)):
        pxb = (4 // mw) * TILE
        for hw in FC.around(pxb):
            shapes.append((1, KPK + 2, 1, hw, cout, 1))
        shapes.append((1, KPK + 2, 7, 2 * (pxb // 4) - 1, cout, 2))  # 4 x pxb / 4 output pixels
    # below, at and above each channel-block size MW 32
    for cb in (COUT_STEPS[0], COUT_STEPS[1], 4 * TILE):
        for cout in FC.around(cb):
            shapes.append((1, KPK + 1, 3, 4, cout, 1))
    # below, at and above the chunk length, and two whole chunks
    for cin in FC.around(KPK, 2 * KPK):
        shapes.append((2, cin, 4, 3, 9, 1))
    # cin just below and at the plan's thresholds for KS = 2 and KS = 4, for every MW
    for chunks in (ks2, ks4):
        for cout in (24, 40, 72):
            shapes += [(1, (chunks - 1) * KPK, 3, 3, cout, 1), (1, (chunks - 1) * KPK + 1, 5, 4, cout, 2)]
    # the three real head shapes
    shapes += [(1, 672, 20, 20, 546, 1), (1, 480, 10, 10, 24, 1), (1, 128, 1, 1, 546, 1)]
    return shapes


def _large_plan_shapes():
    """One shape per NT = 2 and NT = 4 plan (and per MW): the fewest channels that leave the single-chunk rule (kPK + 1), the plane
    just long enough for the plan's wave-tile thresholds at n = 2; the largest tensor is 91 MB."""
    nt1, nt2 = _plan_numbers()[:2]
    shapes = []
    for cout, above in ((9, nt1), (COUT_STEPS[0] + 1, nt1), (COUT_STEPS[1] + 1, nt1), (COUT_STEPS[0] + 1, nt2), (COUT_STEPS[1] + 1, nt2)):
        ctiles = -(-cout // TILE)
        ptiles = above // (2 * ctiles) + 1  # 2 images
        shapes.append((2, KPK + 1, ptiles, TILE, cout, 1))
    return shapes


BOUNDARY = _boundary_shapes()
LARGE = _large_plan_shapes()
# bias x affine x activation of the depthwise stage, bias x affine x residual x activation of the pointwise stage: dealt round-robin over
# the shapes (the full product runs on one small shape below)
EPILOGUES = [e for e in itertools.product((False, True), (None, "mul_add", "fma"), ACTS, (False, True), (None, "mul_add", "fma"), (False, True), ACTS)]


def _epilogue(i):
    return EPILOGUES[(i * 131 + 7) % len(EPILOGUES)]  # 131 is coprime to the 1152 classes: consecutive shapes get unrelated classes


def test_every_instantiated_kernel_is_reached():
    """The plan evaluated on the host for every shape of this file (each run asserts that the launched kernel is that instance)."""
    reached = {_instance(*s) for s in BOUNDARY + LARGE}
    assert reached == INSTANCES, (sorted(INSTANCES - reached), sorted(reached - INSTANCES))
    assert _instance(1, 672, 20, 20, 546, 1) == "k_conv1x1_dw<1,4,ks4>"
    assert {_instance(*s) for s in LARGE} == {"k_conv1x1_dw<2,1>", "k_conv1x1_dw<2,2>", "k_conv1x1_dw<2,4>", "k_conv1x1_dw<4,2>", "k_conv1x1_dw<4,4>"}
    assert all(4 * max(s[0] * s[1] * s[2] * s[3], s[0] * s[4] * s[2] * s[3]) < 200e6 for s in LARGE)


@pytest.mark.parametrize("i", range(len(BOUNDARY)), ids=lambda i: "x".join(str(v) for v in BOUNDARY[i]))
def test_fused_equals_the_composition_and_the_oracle(i):
    _run(BOUNDARY[i], 3000 + 40 * i, _epilogue(i))
    # the block as SSDlite uses it: a folded BatchNorm2d and ReLU6 on the depthwise stage, the 1x1 conv's bias
    _run(BOUNDARY[i], 3020 + 40 * i, (False, "fma", "relu6", True, None, False, None))


@pytest.mark.parametrize("i", range(len(LARGE)), ids=lambda i: "x".join(str(v) for v in LARGE[i]))
def test_large_plans(i):
    """The NT = 2 and NT = 4 instances: the composition on the whole batch, the oracle on the first and the last image."""
    shape = LARGE[i]
    n, cin, h, w, cout, stride = shape
    epi = (True, "fma", "relu6", True, "mul_add", True, "relu") if i % 2 else (False, "mul_add", "hardswish", True, "fma", True, None)
    dw_bias, dw_affine, dw_act, bias, affine, residual, act = epi
    d = _data(5000 + i, n, cin, h, w, cout, stride, dw_bias, dw_affine, bias, affine, residual)
    g = _cuda(d)
    got = _fused(g, stride, dw_affine, dw_act, affine, act)
    assert _lib.last_kernel() == _instance(*shape)
    _same_bits(got, _composed(g, stride, dw_affine, dw_act, affine, act), f"{shape} against the composition")
    got = got.cpu()
    for img in (0, n - 1):
        one = {k: (v[img:img + 1] if k in ("x", "res") and v is not None else v) for k, v in d.items()}
        R.same(got[img:img + 1], torch.from_numpy(_oracle(one, stride, dw_affine, dw_act, affine, act, plan_n=n)), f"{shape} image {img} against the oracle")


def test_every_epilogue_on_one_small_shape():
    """Each affine code and each of none / relu / relu6 / hardswish on either stage (144 combinations), the biases and the residual
    alternating, on 2 x 35 x 5 x 4 -> 37 at both strides."""
    for j, (dw_affine, dw_act, affine, act) in enumerate(itertools.product((None, "mul_add", "fma"), ACTS, (None, "mul_add", "fma"), ACTS)):
        epi = (bool(j & 1), dw_affine, dw_act, bool(j & 2), affine, bool(j & 4), act)
        _run((2, 35, 5, 4, 37, 1 + (j >> 3) % 2), 6000 + j, epi)


# ------------------------------------------------------------------------------------------------ 2. a seeded sweep
def test_seeded_sweep_against_the_composition():
    rng = np.random.default_rng(7100)
    sizes = sorted({1, 2, 3, 5, 7, 8} | set(FC.around(KPK // 4)) | set(FC.around(KPK // 2)))
    chans = sorted({1, 2, 3, 7} | set(FC.around(KPK, 2 * KPK)) | set(FC.around(COUT_STEPS[0], COUT_STEPS[1])) | {_plan_numbers()[3] * KPK - KPK + 1})
    ran, seen = 0, set()
    for j in range(40):
        shape = (int(rng.integers(1, 4)), int(rng.choice(chans)), int(rng.choice(sizes)), int(rng.choice(sizes)), int(rng.choice(chans)),
                 1 + j % 2)
        seen.add(_run(shape, 7200 + j, _epilogue(500 + 37 * j), oracle=False))
        ran += 1
    assert ran == 40 and len(seen) >= 4, (ran, seen)


# ------------------------------------------------------------------------------------------------ 3. special values
def _window_pixels(h, w, stride, iy, ix):
    """The output pixels whose 3 x 3 window (padding 1) contains input pixel (iy, ix), from the geometry alone."""
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    hit = torch.zeros(oh, ow, dtype=torch.bool)
    for oy in range(oh):
        for ox in range(ow):
            if abs(oy * stride - iy) <= 1 and abs(ox * stride - ix) <= 1:
                hit[oy, ox] = True
    return hit


@pytest.mark.parametrize("stride", [1, 2])
def test_special_values(stride):
    n, cin, h, w, cout = 2, 37, 7, 6, 41
    epi = dict(dw_affine="fma", dw_act=None, affine=None, act=None)
    d = _data(8000 + stride, n, cin, h, w, cout, stride, True, "fma", True, None, True)
    clean = _fused(_cuda(d), stride, **epi).cpu()
    assert bool(torch.isfinite(clean).all())

    def check(key, index, value, what):
        e = {k: (None if v is None else v.clone()) for k, v in d.items()}
        e[key][index] = value
        g = _cuda(e)
        got = _fused(g, stride, **epi)
        _same_bits(got, _composed(g, stride, **epi), what)
        return got.cpu()

    # a single NaN, +Inf and a subnormal in x: only the output pixels whose window holds it change, in its image
    for value, name in ((NAN, "NaN"), (INF, "+Inf"), (1e-41, "a subnormal")):
        for img, k, iy, ix in ((1, 5, 0, 0), (0, 36, 3, 2), (1, 20, h - 1, w - 1)):
            got = check("x", (img, k, iy, ix), value, f"{name} in x at {(img, k, iy, ix)}")
            hit = torch.zeros(n, *clean.shape[2:], dtype=torch.bool)
            hit[img] = _window_pixels(h, w, stride, iy, ix)
            changed = (got.view(torch.int32) != clean.view(torch.int32))
            assert not bool(changed[~hit[:, None].expand_as(changed)].any()), f"{name}: a pixel outside the window changed"
            if name != "a subnormal":
                assert torch.equal(~torch.isfinite(got), hit[:, None].expand_as(got)), f"{name}: the non-finite outputs are not the window's pixels"
            assert int(hit.sum()) >= 1
    # a NaN and an Inf in one depthwise weight of channel k: every pixel of the plane, the border pixels through their padding taps
    for value, name in ((NAN, "NaN"), (INF, "Inf")):
        for tap in ((0, 0), (1, 1), (2, 1)):
            got = check("dw", (9, 0) + tap, value, f"{name} in a depthwise weight, tap {tap}")
            assert not bool(torch.isfinite(got).any()), f"{name} in the depthwise weight {tap} left a finite output"
    # a NaN in one pointwise weight: its output channel, nothing else
    got = check("w", (17, 30, 0, 0), NAN, "NaN in a pointwise weight")
    assert bool(torch.isnan(got[:, 17]).all())
    keep = [c for c in range(cout) if c != 17]
    assert torch.equal(got[:, keep].view(torch.int32), clean[:, keep].view(torch.int32))


# ------------------------------------------------------------------------------------------------ the modules
COUNTED = ("dwconv_pointwise", "conv_norm_act", "conv2d_bias_relu", "conv2d_bias_act", "squeeze_excitation_gate", "se_scale", "squeeze_excitation")


def _counting(fn, names):
    """fn() with every call of a functional entry point recorded by name, as tests/test_gpu_ssd.py does."""
    wrapped = {}
    for name in COUNTED:
        orig = getattr(F, name)
        wrapped[name] = orig

        def make(orig=orig, name=name):
            @functools.wraps(orig)
            def call(*a, **kw):
                names.append(name)
                return orig(*a, **kw)
            return call
        setattr(F, name, make())
    try:
        return fn()
    finally:
        for name, orig in wrapped.items():
            setattr(F, name, orig)


def _folded(bn, device="cuda"):
    a, b = F.fold_batchnorm(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    return a.to(device), b.to(device)


def _prediction_by_hand(block, x):
    """A prediction block as the layer calls written out."""
    cna, conv = block[0], block[1]
    a, b = _folded(cna[1])
    return F.dwconv_pointwise(x, cna[0].weight, None, a, b, conv.weight, conv.bias, dw_affine="fma", dw_activation="relu6")


def _prediction_composed(block, x):
    cna, conv = block[0], block[1]
    a, b = _folded(cna[1])
    hidden = F.conv_norm_act(x, cna[0].weight, None, a, b, groups=cna[0].in_channels, affine="fma", activation="relu6")
    return F.conv_norm_act(hidden, conv.weight, conv.bias)


def _randomize(module, seed, std=0.2):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * std)
    MR.perturb(module, seed + 1)


def test_head_on_three_tiny_levels():
    """SSDLiteHead on 8, 16 and 24 channels, grids (5, 4), (3, 3), (1, 1), a batch of two: one fused launch per (level, head), every
    map equal to the layer calls written out and to the two-launch composition, permuted() against the replica's output."""
    chans, grids, anchors, classes = [8, 16, 24], [(5, 4), (3, 3), (1, 1)], [4, 6, 4], 3
    norm = RL.default_norm_layer()
    head = mv.SSDLiteHead(chans, anchors, classes, norm)
    _randomize(head, 8100)
    xs = [torch.from_numpy(philox_f32(8110 + i, (2, c, h, w)) * 2 - 1) for i, (c, (h, w)) in enumerate(zip(chans, grids))]
    state = {k: v.clone() for k, v in head.state_dict().items()}
    head = head.cuda()
    dx = [x.cuda() for x in xs]
    launches = []
    out = _counting(lambda: head(dx), launches)
    assert launches == ["dwconv_pointwise"] * 6 and list(out) == ["bbox_regression", "cls_logits"]
    for name, sub, cols in (("cls_logits", head.classification_head, classes), ("bbox_regression", head.regression_head, 4)):
        assert [tuple(m.shape) for m in out[name]] == [(2, a * cols, h, w) for a, (h, w) in zip(anchors, grids)]
        for l, block in enumerate(sub.module_list):
            _same_bits(out[name][l], _prediction_by_hand(block, dx[l]), f"{name} level {l}: the layer call")
            _same_bits(out[name][l], _prediction_composed(block, dx[l]), f"{name} level {l}: the composition")
        replica = RL.SSDLiteClassificationHead(chans, anchors, classes, norm) if cols == classes else RL.SSDLiteRegressionHead(chans, anchors, norm)
        prefix = "classification_head." if cols == classes else "regression_head."
        replica.load_state_dict({k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}, strict=True)
        replica.eval()
        perm = sub.permuted(out[name]).detach().cpu()
        with torch.no_grad():
            theirs = replica(xs)
        assert perm.shape == theirs.shape == (2, sum(a * h * w for a, (h, w) in zip(anchors, grids)), cols)
        assert float((perm - theirs).abs().max()) <= 1e-4 * max(1.0, float(theirs.abs().max()))
    # norm_layer=None: the blocks carry conv biases instead
    plain = mv.SSDLiteRegressionHead([8], [4], None)
    _randomize(plain, 8150)
    plain = plain.cuda()
    blk = plain.module_list[0]
    assert blk[0][0].bias is not None and len(blk[0]) == 2
    want = F.conv_norm_act(F.conv_norm_act(dx[0], blk[0][0].weight, blk[0][0].bias, groups=8, activation="relu6"), blk[1].weight, blk[1].bias)
    _same_bits(plain([dx[0]])[0], want, "norm_layer=None")


def _c(n=1):
    return ["conv_norm_act"] * n


G_, D_ = ["squeeze_excitation_gate"], ["dwconv_pointwise"]
# MobileNetV3-Large by its table: a block is [expand] + depthwise + [gate] + projection
FEATURES0 = _c() + _c(2) + _c(3) + _c(3) + 3 * (_c(2) + G_ + _c()) + 4 * _c(3) + 2 * (_c(2) + G_ + _c()) + _c()
FEATURES1 = _c() + G_ + _c() + 2 * (_c(2) + G_ + _c()) + _c()
EXTRA = 4 * (_c() + D_)


def _extractor_by_hand(bb, x):
    """The six maps as the library calls written out: the blocks in front of C4 through their modules, the C4 expansion, the back half
    of the C4 block with the gate as the projection's input_scale, the rest of the backbone, the extra blocks."""
    maps = []
    t = x
    for m in list(bb.features[0])[:-1]:
        t = m(t)
    exp = bb.features[0][-1]
    t = F.conv_norm_act(t, exp[0].weight, None, *_folded(exp[1]), affine="fma", activation="hardswish")
    maps.append(t)
    dw, se, proj = list(bb.features[1][0])
    t = F.conv_norm_act(t, dw[0].weight, None, *_folded(dw[1]), stride=2, groups=dw[0].in_channels, affine="fma", activation="hardswish")
    gate = F.squeeze_excitation_gate(t, se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias, "relu", "hardsigmoid")
    t = F.conv_norm_act(t, proj[0].weight, None, *_folded(proj[1]), affine="fma", input_scale=gate)
    for m in list(bb.features[1])[1:]:
        t = m(t)
    maps.append(t)
    for block in bb.extra:
        t = F.conv_norm_act(t, block[0][0].weight, None, *_folded(block[0][1]), affine="fma", activation="relu6")
        a1, b1 = _folded(block[1][1])
        a2, b2 = _folded(block[2][1])
        t = F.dwconv_pointwise(t, block[1][0].weight, None, a1, b1, block[2][0].weight, None, a2, b2, stride=2, dw_affine="fma",
                               dw_activation="relu6", affine="fma", activation="relu6")
        maps.append(t)
    return maps


# How the seed and the spread of the class-head biases were chosen: with the replica (tests/_ssdlite_ref.py) on the CPU, loaded with this
# model's state dict, and the restated post-processing of tests/_ssd_ref.py, torch.manual_seed 9000 .. 9002 and N(0, s) biases for
# s in (0.5, 1, 2) were tried on the two test images.  Every pair qualified: 1200 candidates per image, 440 to 600 detections behind the
# nms (so the cut at detections_per_img = 300 is exercised), three or four classes among the 300 kept.  The first seed with the middle
# spread is used.  The norms' statistics are perturbed (tests/_mobilenetv3_ref.perturb) so that the folded terms differ from 1 and 0.
MODEL_SEED, BIAS_SEED, BIAS_STD = 9000, 9001, 1.0


def build_ssdlite320():
    torch.manual_seed(MODEL_SEED)
    model = mv.ssdlite320_mobilenet_v3_large(num_classes=5)
    MR.perturb(model, MODEL_SEED + 2)
    g = torch.Generator().manual_seed(BIAS_SEED)
    with torch.no_grad():
        for block in model.head.classification_head.module_list:
            block[1].bias.copy_(torch.randn(block[1].bias.shape, generator=g) * BIAS_STD)
    return model


def _images():
    return [torch.from_numpy(philox_f32(9020, (3, 240, 320))), torch.from_numpy(philox_f32(9021, (3, 333, 250)))]


@pytest.fixture(scope="module")
def ssdlite320():
    return build_ssdlite320().cuda()


def test_extractor_at_320(ssdlite320):
    bb = ssdlite320.backbone
    x = torch.from_numpy(philox_f32(9010, (1, 3, 320, 320)) * 2 - 1).cuda()
    launches = []
    out = _counting(lambda: bb(x), launches)
    assert list(out) == ["0", "1", "2", "3", "4", "5"]
    assert [tuple(v.shape) for v in out.values()] == [(1, 672, 20, 20), (1, 480, 10, 10), (1, 512, 5, 5), (1, 256, 3, 3), (1, 256, 2, 2), (1, 128, 1, 1)]
    assert launches == FEATURES0 + FEATURES1 + EXTRA and "se_scale" not in launches
    for i, want in enumerate(_extractor_by_hand(bb, x)):
        _same_bits(out[str(i)], want, f"map {i}")
    assert float(out["5"].detach().abs().max()) > 0 and bool(torch.isfinite(out["5"]).all())


def _check_model(model, imgs, size_hw, classes, originals, min_det):
    """Stage by stage, every reference fed the library's own output of the stage before (tests/test_gpu_ssd.py::test_ssd300_stage_by_stage)."""
    dimgs = [i.cuda() for i in imgs]
    n = len(imgs)
    images, _ = model.transform(dimgs, None)
    assert images.image_sizes == [size_hw] * n and tuple(images.tensors.shape) == (n, 3) + size_hw
    feats = list(model.backbone(images.tensors).values())
    launches = []
    head_out = _counting(lambda: model.head(feats), launches)
    # the dispatch rule of ssdlite._use_fused, restated: one fused launch up to 128 channels, or up to 256 with more than 64 outputs; the
    # two-launch composition elsewhere.  The regression head runs first
    want_launches = []
    for cols in (4, classes):
        for f in feats:
            cin, cout = int(f.shape[1]), 6 * cols
            want_launches += D_ if cin <= 128 or (cin <= 256 and cout > 64) else _c(2)
    assert launches == want_launches and launches.count("dwconv_pointwise") >= 2
    for name, sub in (("cls_logits", model.head.classification_head), ("bbox_regression", model.head.regression_head)):
        for l, block in enumerate(sub.module_list):  # the same bits whichever way a block was dispatched
            _same_bits(head_out[name][l], _prediction_by_hand(block, feats[l]), f"{name} level {l}: the fused call")
            _same_bits(head_out[name][l], _prediction_composed(block, feats[l]), f"{name} level {l}: the composition")
    cl, rg = ([m.detach().cpu() for m in head_out[name]] for name in ("cls_logits", "bbox_regression"))
    grids = [tuple(f.shape[-2:]) for f in feats]
    assert [tuple(m.shape) for m in cl] == [(n, 6 * classes) + g for g in grids]
    idx, boxes, scores, labels, valid = model.candidates(head_out, feats, images)
    sc = R.scores(cl, classes)
    k = model.topk_candidates
    want_idx = R.select(sc, k, model.score_thresh)
    assert idx.shape == (n, (classes - 1) * k) and torch.equal(idx.cpu(), want_idx)
    gen = model.anchor_generator
    dboxes = R.default_boxes(gen, grids, size_hw)
    assert torch.equal(dboxes, gen(R.ImageList(images.tensors.cpu(), images.image_sizes), cl)[0])
    wb, wsc, wl, wv = R.decode(sc, rg, want_idx, dboxes, images.image_sizes)
    R.same(boxes, wb, "boxes"), R.same(scores, wsc, "scores")
    assert torch.equal(labels.cpu(), wl) and torch.equal(valid.cpu(), wv)
    got = model(dimgs)
    for i, original in enumerate(originals):
        b, s, lab = wb[i][wv[i]], wsc[i][wv[i]], wl[i][wv[i]]
        keep = R.batched_nms(b, s, lab, model.nms_thresh)[:model.detections_per_img]
        want_boxes = R.RH.resize_boxes(b[keep], size_hw, original)
        print(f"image {i}: {int(wv[i].sum())} candidates, {len(keep)} detections, classes {sorted(set(lab[keep].tolist()))}")
        assert min_det <= len(keep) <= model.detections_per_img and len(set(lab[keep].tolist())) >= 2, "the comparison shows nothing"
        R.same(got[i]["boxes"], want_boxes, f"boxes of image {i}")
        R.same(got[i]["scores"], s[keep], f"scores of image {i}")
        assert torch.equal(got[i]["labels"].cpu(), lab[keep])
        gb = got[i]["boxes"].detach()
        assert float(gb.min()) >= 0 and float(gb[:, 0::2].max()) <= original[1] + 1e-3 and float(gb[:, 1::2].max()) <= original[0] + 1e-3
    return dboxes


def test_ssdlite320_stage_by_stage(ssdlite320):
    """ssdlite320_mobilenet_v3_large(num_classes=5) on two raw images of different sizes."""
    assert ssdlite320.detections_per_img == 300
    dboxes = _check_model(ssdlite320, _images(), (320, 320), 5, [(240, 320), (333, 250)], 10)
    assert dboxes.shape == (3234, 4)
    # at 91 classes the rule gives: regression 5 x two launches + 1 fused, classification 3 x two launches + 3 fused
    assert [SL._use_fused(c, 24) for c in (672, 480, 512, 256, 256, 128)] == [False] * 5 + [True]
    assert [SL._use_fused(c, 546) for c in (672, 480, 512, 256, 256, 128)] == [False] * 3 + [True] * 3
    assert all(SL._use_fused(c // 2, c) for c in (512, 256, 256, 128))  # the extra blocks


def test_small_non_square_model():
    """A width_mult = 0.25 extractor at a fixed size of 96 x 128, three images, 4 classes: maps of 6 x 8, 3 x 4, 2 x 2 and three of
    1 x 1, so the stride-2 depthwise conv runs on 2 -> 1 and 1 -> 1."""
    torch.manual_seed(9500)
    norm = RL.default_norm_layer()
    backbone = mv.mobilenet_v3_large(width_mult=0.25, reduced_tail=True, norm_layer=norm)
    SL._normal_init(backbone)
    extractor = mv.SSDLiteFeatureExtractorMobileNet(backbone.features, 13, norm, width_mult=0.25)
    gen = DefaultBoxGenerator([[2, 3] for _ in range(6)], min_ratio=0.2, max_ratio=0.95)
    channels = extractor._module_out_channels()
    model = mv.SSD(extractor, gen, (128, 96), 4, head=mv.SSDLiteHead(channels, gen.num_anchors_per_location(), 4, norm), image_mean=[0.5] * 3,
                   image_std=[0.5] * 3, score_thresh=0.05, nms_thresh=0.55, topk_candidates=30, detections_per_img=25)
    MR.perturb(model, 9501)
    g = torch.Generator().manual_seed(9502)
    with torch.no_grad():
        for block in model.head.classification_head.module_list:
            block[1].bias.copy_(torch.randn(block[1].bias.shape, generator=g))
    model = model.cuda()
    imgs = [torch.from_numpy(philox_f32(9510, (3, 100, 130))), torch.from_numpy(philox_f32(9511, (3, 96, 128))), torch.from_numpy(philox_f32(9512, (3, 40, 150)))]
    feats = model.backbone(model.transform([i.cuda() for i in imgs], None)[0].tensors)
    assert [tuple(f.shape[-2:]) for f in feats.values()] == [(6, 8), (3, 4), (2, 2), (1, 1), (1, 1), (1, 1)]
    _check_model(model, imgs, (96, 128), 4, [(100, 130), (96, 128), (40, 150)], 3)
