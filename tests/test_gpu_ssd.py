"""SSD on the GPU (`-m gpu`): F.l2_normalize_scale (csrc/l2norm.hip), F.max_pool2d(ceil_mode=True) (csrc/cnn_ops.hip), F.ssd_scores,
F.ssd_topk, F.ssd_decode (csrc/ssd.hip), SSDHead, SSDFeatureExtractorVGG and SSD.  The kernels are compared bit for bit (NaN in equal
places, == elsewhere) with the restatement (b) of tests/_ssd_ref.py on the CPU, the pool with torch's CPU max_pool2d (a maximum is
exact), the head with the CPU oracle conv."""
import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd.anchor_utils import DefaultBoxGenerator  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _ssd_ref as R  # noqa: E402
from tests._util import oracle_conv3x3, philox_f32  # noqa: E402

NAN, INF = float("nan"), float("inf")


def _randn(seed, shape, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------ l2_normalize_scale
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (38, 38)])
@pytest.mark.parametrize("c", [1, 3, 64, 512, 513])
def test_l2_normalize_scale_equals_the_restatement(c, hw):
    x = _randn(100 + c, (2, c) + hw, 3.0)
    w = _randn(200 + c, (c,)) * 2 + 20
    got = F.l2_normalize_scale(x.cuda(), w.cuda())
    assert _lib.last_kernel() == "k_l2_normalize_scale"
    R.same(got, R.l2_normalize_scale(x, w), f"C={c} {hw}")


def test_l2_normalize_scale_strided_and_in_place():
    c = 37
    wide = _randn(301, (3, c + 5, 5, 7))
    w = _randn(302, (c,)) + 4
    x = wide[:, 2:c + 2]
    want = R.l2_normalize_scale(x, w)
    dwide = wide.cuda()
    R.same(F.l2_normalize_scale(dwide[:, 2:c + 2], w.cuda()), want, "a channel slice")
    assert torch.equal(dwide.cpu(), wide), "the input changed"
    dense = x.contiguous().cuda()
    assert F.l2_normalize_scale(dense, w.cuda(), out=dense) is dense
    R.same(dense, want, "in place")
    view = dwide[:, 2:c + 2]
    assert F.l2_normalize_scale(view, w.cuda(), out=view) is view
    expect = wide.clone()
    expect[:, 2:c + 2] = want
    R.same(dwide, expect, "in place on a channel slice: the other channels keep their values")
    R.same(F.l2_normalize_scale(x.permute(0, 1, 3, 2).cuda(), w.cuda()), R.l2_normalize_scale(x.permute(0, 1, 3, 2).contiguous(), w),
           "a transposed view is copied")
    assert F.l2_normalize_scale(torch.zeros((0, 4, 3, 3), device="cuda"), torch.ones(4, device="cuda")).shape == (0, 4, 3, 3)
    R.same(F.l2_normalize_scale(x[:1].cuda(), w.cuda(), eps=2.5), R.l2_normalize_scale(x[:1], w, eps=2.5), "a large eps clamps")


def test_l2_normalize_scale_special_values_stay_in_their_pixel():
    x = _randn(310, (2, 64, 5, 5))
    x[0, :, 2, 3] = 0.0              # an all-zero pixel: 0, not NaN
    x[0, 7, 1, 1] = NAN
    x[1, 9, 0, 4], x[1, 20, 4, 0] = INF, -INF
    w = _randn(311, (64,)) + 3
    got = F.l2_normalize_scale(x.cuda(), w.cuda()).cpu()
    R.same(got, R.l2_normalize_scale(x, w), "special values")
    assert float(got[0, :, 2, 3].abs().max()) == 0.0
    bad = torch.isnan(got).any(dim=1)
    want_bad = torch.zeros(2, 5, 5, dtype=torch.bool)
    want_bad[0, 1, 1] = want_bad[1, 0, 4] = want_bad[1, 4, 0] = True
    assert torch.equal(bad, want_bad)
    assert bool(torch.isnan(got[0, :, 1, 1]).all())                                      # a NaN: the whole pixel
    assert float(got[1, 8, 0, 4]) == 0.0 and bool(torch.isnan(got[1, 9, 0, 4]))          # an infinity: x / inf = 0, inf / inf = NaN


def test_l2_normalize_scale_depends_on_the_pixel_alone():
    c = 512
    pixel = _randn(320, (c,), 2.0)
    w = _randn(321, (c,)) + 20
    small = _randn(322, (1, c, 5, 7))
    small[0, :, 0, 0] = pixel
    small[0, :, 4, 6] = pixel
    big = _randn(323, (3, c, 38, 38))
    big[2, :, 17, 21] = pixel
    odd = torch.empty(3 * c * 38 * 38 + 1, device="cuda")[1:].view(3, c, 38, 38)  # 4 bytes past a 16-byte boundary
    odd.copy_(big)
    assert odd.data_ptr() % 16 == 4
    a = F.l2_normalize_scale(small.cuda(), w.cuda())
    b = F.l2_normalize_scale(big.cuda(), w.cuda())
    d = F.l2_normalize_scale(odd, w.cuda())
    want = R.l2_normalize_scale(pixel.view(1, c, 1, 1), w).view(c)
    for got, what in ((a[0, :, 0, 0], "first"), (a[0, :, 4, 6], "last"), (b[2, :, 17, 21], "batch of 3"), (d[2, :, 17, 21], "misaligned")):
        R.same(got, want, what)
    assert torch.equal(b, d)


# ------------------------------------------------------------------------------------------------ max_pool2d(ceil_mode=True)
POOL_CASES = [((75, 75), 2, 2, 0, (38, 38)), ((3, 3), 2, 2, 1, (2, 2)), ((4, 4), 2, 2, 1, (3, 3)), ((5, 5), 3, 2, 1, (3, 3)),
              ((7, 10), 3, 2, 1, (4, 6)), ((9, 4), 2, 2, 0, (5, 2)), ((19, 19), 3, 1, 1, (19, 19)), ((6, 11), 3, 3, 0, (2, 4)),
              ((10, 13), 5, 4, 2, (3, 4))]


@pytest.mark.parametrize("size,k,s,p,out", POOL_CASES)
def test_max_pool2d_ceil_mode_equals_torch(size, k, s, p, out):
    x = _randn(400 + size[0] * 16 + k, (2, 3) + size)
    x[0, 1, size[0] // 2, size[1] // 2] = NAN
    x[1, 2] = -INF
    x[1, 0, -1, -1] = INF
    want = nn.functional.max_pool2d(x, k, s, p, ceil_mode=True)
    assert tuple(want.shape[-2:]) == out
    got = F.max_pool2d(x.cuda(), k, s, p, ceil_mode=True)
    assert _lib.last_kernel() == "k_maxpool2d_pad<ceil>"
    R.same(got, want, f"{size} k={k} s={s} p={p}")
    assert bool(torch.isnan(got).any()) and bool((got[1, 2] == -INF).all())


def test_max_pool2d_floor_mode_is_the_existing_call():
    x = _randn(450, (2, 3, 9, 11)).cuda()
    for args in ((3, 2, 1), (2, 2, 0), (3, 2, 0), (3, 1, 1)):
        a = F.max_pool2d(x, *args, ceil_mode=False)
        ka = _lib.last_kernel()
        b = F.max_pool2d(x, *args)
        assert ka == _lib.last_kernel() != "k_maxpool2d_pad<ceil>" and torch.equal(a, b)
    # where both modes give the same size they give the same values
    assert torch.equal(F.max_pool2d(x, 3, 2, 1, ceil_mode=True), F.max_pool2d(x, 3, 2, 1))


# ------------------------------------------------------------------------------------------------ ssd_scores
SCORE_GRIDS = {"tiny": [((1, 1), 4), ((3, 3), 6), ((5, 4), 4)], "ssd": [((38, 38), 4), ((3, 3), 6)]}


def _class_maps(seed, grids, classes, n=2, pad=0, scale=2.0):
    """Per-level maps (n, A K, H, W); pad > 0: channel slices of wider tensors, so that the image stride exceeds the map."""
    maps = []
    for i, ((h, w), a) in enumerate(grids):
        wide = _randn(seed + i, (n, a * classes + pad, h, w), scale)
        maps.append(wide[:, :a * classes] if pad else wide)
    return maps


def _to_device(m):
    """A map on the device with the strides it has on the host (`.cuda()` alone would make a channel slice dense)."""
    base = m._base if m._base is not None else m
    return torch.as_strided(base.cuda(), m.shape, m.stride(), m.storage_offset())


@pytest.mark.parametrize("grids", list(SCORE_GRIDS))
@pytest.mark.parametrize("classes", [2, 21, 91])
def test_ssd_scores_equal_the_restatement(classes, grids):
    maps = _class_maps(500 + classes, SCORE_GRIDS[grids], classes, pad=3)
    m0 = maps[0]
    m0[0, 0:classes, 0, 0] = 1.5         # anchor 0 of position 0: equal logits -> 1 / K each
    m0[1, classes + 1, 0, 0] = NAN      # anchor 1 of position 0 of image 1: a NaN row
    maps[1][0, 2, 1, 1] = INF            # +inf: the row is NaN, as torch's
    maps[1][1, 3, 2, 2] = -INF           # -inf: a zero score
    dmaps = [_to_device(m) for m in maps]
    assert all(d.stride(0) > d[0].numel() for d in dmaps)
    got = F.ssd_scores(dmaps, classes)
    assert _lib.last_kernel() == f"k_ssd_scores<levels{len(maps)},classes{classes}>"
    want = R.scores(maps, classes)
    assert got.shape == want.shape == (2, classes, sum(h * w * a for (h, w), a in SCORE_GRIDS[grids])) and got.is_contiguous()
    R.same(got, want, f"K={classes} {grids}")
    got = got.cpu()
    assert float((got[0, :, 0] - 1.0 / classes).abs().max()) < 1e-7  # equal logits
    assert bool(torch.isnan(got[1, :, 1]).all()) and not bool(torch.isnan(got[1, :, 0]).any())
    (h0, w0), a0 = SCORE_GRIDS[grids][0]
    v_inf = a0 * h0 * w0 + (1 * 3 + 1) * 6 + 2 // classes  # level 1 (3 x 3, A = 6), position (1, 1), the anchor of channel 2
    assert bool(torch.isnan(got[0, :, v_inf]).all()) and not bool(torch.isnan(got[0, :, v_inf + 6]).any())
    torch_sm = torch.softmax(torch.cat([R.permute_level(m, classes) for m in maps], dim=1), -1).permute(0, 2, 1)
    ok = ~torch.isnan(want)
    assert float((got[ok] - torch_sm[ok]).abs().max()) <= R.RH.score_bound(classes)  # scores <= 1: the relative bound, absolutely


# ------------------------------------------------------------------------------------------------ ssd_topk
def _scores(seed, n, classes, v, ties=True):
    p = torch.softmax(_randn(seed, (n, v, classes), 2.0), -1).permute(0, 2, 1).contiguous()
    if ties:
        p.view(-1)[::7] = 0.25
    return p


TOPK_CASES = {
    "V < k": (lambda: _scores(600, 2, 4, 10), 16, 0.05),
    "ssd300": (lambda: _scores(601, 2, 3, 8732), 400, 0.01),
    "k = 1": (lambda: _scores(602, 2, 5, 300), 1, 0.01),
    "all equal": (lambda: torch.full((2, 3, 700), 0.5), 50, 0.1),
    "nothing passes": (lambda: _scores(603, 1, 3, 200), 7, 1.5),
    "everything passes": (lambda: _scores(604, 2, 3, 5000), 4096, -1.0),
    "zeros pass a negative threshold": (lambda: torch.zeros((1, 2, 100)), 8, -0.5),
    "equal to the threshold fails": (lambda: _scores(605, 2, 3, 900), 300, 0.25),
    "more ties than k": (lambda: _scores(606, 1, 2, 4000).clamp_(max=0.3), 33, 0.1),
}


@pytest.mark.parametrize("name", list(TOPK_CASES))
def test_ssd_topk_equals_the_restatement(name):
    make, k, thresh = TOPK_CASES[name]
    sc = make()
    n, classes, v = sc.shape
    got = F.ssd_topk(sc.cuda(), k, thresh)
    assert _lib.last_kernel() == f"k_ssd_topk<classes{classes},k{k}>"
    want = R.select(sc, k, thresh)
    assert got.shape == (n, (classes - 1) * k) and got.dtype == torch.int32
    assert torch.equal(got.cpu(), want), name
    if name == "all equal":
        assert torch.equal(want[0, :50], (torch.arange(50) * 3 + 1).int()) and torch.equal(want[0, 50:], (torch.arange(50) * 3 + 2).int())
    if name == "nothing passes":
        assert bool((want == -1).all())
    if name == "equal to the threshold fails":
        sel = want[want >= 0].long()
        assert bool((sc.permute(0, 2, 1).reshape(n, -1)[0][want[0][want[0] >= 0].long()] > 0.25).all()) and sel.numel() > 0
        assert bool((sc == 0.25).any())
    if name == "V < k":
        assert bool((want.view(n, classes - 1, k)[:, :, 10:] == -1).all())


def test_ssd_topk_nan_scores_and_the_background_row():
    sc = _scores(610, 2, 4, 500)
    sc[:, 0] = 0.99                # the background: never selected
    sc[0, 2, ::3] = NAN            # a NaN fails the comparison
    sc[1, 3] = NAN
    got = F.ssd_topk(sc.cuda(), 64, 0.05).cpu()
    assert torch.equal(got, R.select(sc, 64, 0.05))
    assert bool((got[1, 128:] == -1).all()) and bool((got[got >= 0] % 4 != 0).all())
    f = got[0, 64:128]
    assert bool((((f[f >= 0] // 4) % 3) != 0).all())


# ------------------------------------------------------------------------------------------------ ssd_decode
DEC_GRIDS = [(5, 4), (3, 3), (1, 1)]
DEC_RATIOS = [[2], [2, 3], [2]]
DEC_IMAGE = (40, 32)
DEC_SIZES = [(40, 32), (37, 30)]


def _decode_case(seed, classes, gen, delta_scale):
    anchors = gen.num_anchors_per_location()
    cls = [_randn(seed + i, (2, a * classes, h, w), 2.0) for i, ((h, w), a) in enumerate(zip(DEC_GRIDS, anchors))]
    reg = [_randn(seed + 10 + i, (2, a * 4, h, w), delta_scale) for i, ((h, w), a) in enumerate(zip(DEC_GRIDS, anchors))]
    sc = R.scores(cls, classes)
    return cls, reg, sc


@pytest.mark.parametrize("clip,steps,scales", [(True, None, None), (True, [7, 13, 29], None), (False, None, [0.5, 1.2, 1.7, 2.0]),
                                               (False, [8, 16, 40], [0.5, 1.2, 1.7, 2.0])])
def test_ssd_decode_equals_the_restatement(clip, steps, scales):
    classes, k = 6, 9
    gen = DefaultBoxGenerator(DEC_RATIOS, steps=steps, scales=scales, clip=clip)
    if not clip:
        assert float(torch.cat(gen._wh_pairs).max()) > 1
    _, reg, sc = _decode_case(700, classes, gen, 6.0)  # wide deltas: boxes leave the image on every side
    reg[0][0, 2, 1, 1], reg[1][1, 4 + 3, 0, 2] = 50.0, 45.0  # dw, dh above log(1000 / 16) * 5
    reg[2][0, 1, 0, 0] = NAN
    idx = R.select(sc, k, 0.05)
    v = sc.shape[2]
    idx[0, 3], idx[1, 0], idx[1, 7], idx[0, 11] = -1, v * classes, v * classes + 5, -7  # outside the pyramid
    want = R.decode(sc, reg, idx, R.default_boxes(gen, DEC_GRIDS, DEC_IMAGE), DEC_SIZES)
    got = F.ssd_decode(sc.cuda(), [m.cuda() for m in reg], idx.cuda(), gen._wh_pairs, gen.steps, DEC_IMAGE, DEC_SIZES, clip=gen.clip)
    assert _lib.last_kernel() == "k_ssd_decode<levels3>"
    for g, w, what in zip(got, want, ("boxes", "scores", "labels", "valid")):
        R.same(g, w, what)
    b, ok = want[0], want[3]
    assert not bool(ok[0, 3]) and not bool(ok[1, 0]) and not bool(ok[1, 7]) and not bool(ok[0, 11]) and float(b[0, 3].abs().max()) == 0
    bb = b[ok]
    bb = bb[~torch.isnan(bb).any(1)]
    assert bool((bb[:, 0] == 0).any()) and bool((bb[:, 1] == 0).any()) and bool((bb[:, 2] == 32).any() or (bb[:, 2] == 30).any()) and \
        bool((bb[:, 3] == 40).any() or (bb[:, 3] == 37).any()), "a box should be clipped on every side"


def test_ssd_decode_clamps_dw_at_the_clip():
    """One candidate whose dw is far above log(1000 / 16): its width is exp(clip) times the default box's, not more."""
    classes = 2
    gen = DefaultBoxGenerator([[2]], clip=True)
    reg = [torch.zeros(1, 16, 1, 1)]
    reg[0][0, 2] = 500.0
    sc = torch.full((1, 2, 4), 0.5)
    idx = torch.tensor([[0 * 2 + 1]], dtype=torch.int32)
    big = (4000, 4000)
    boxes, scores, labels, valid = F.ssd_decode(sc.cuda(), [reg[0].cuda()], idx.cuda(), gen._wh_pairs, None, (100, 100), [big])
    want = R.decode(sc, reg, idx, R.default_boxes(gen, [(1, 1)], (100, 100)), [big])
    R.same(boxes, want[0], "boxes")
    assert float(boxes[0, 0, 0]) == 0.0 and abs(float(boxes[0, 0, 2]) - (50 + 62.5 * 15.0 / 2)) < 1e-2 and bool(valid[0, 0]) and int(labels[0, 0]) == 1 and float(scores[0, 0]) == 0.5


# ------------------------------------------------------------------------------------------------ the modules
def _counting(fn, names):
    """fn() with every launch's kernel recorded (the entry points of the functional namespace, by name)."""
    import functools
    wrapped = {}
    for name in ("conv2d_bias_relu", "conv2d_bias_act", "max_pool2d", "l2_normalize_scale", "ssd_scores", "ssd_topk", "ssd_decode"):
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


def _randomize(module, seed, std=0.05):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * std)


def test_head_equals_the_layer_calls_and_the_oracle():
    """SSDHead on three tiny levels of 8 channels, a batch of two: one launch per (level, head), the layer-by-layer calls and the CPU
    oracle conv bit for bit, and permuted() against the reference's layout."""
    grids, anchors, classes = [(5, 4), (3, 3), (1, 1)], [4, 6, 4], 3
    head = mv.SSDHead([8, 8, 8], anchors, classes)
    _randomize(head, 800, 0.2)
    xs = [torch.from_numpy(philox_f32(810 + i, (2, 8, h, w)) * 2 - 1) for i, (h, w) in enumerate(grids)]
    head = head.cuda()
    dx = [x.cuda() for x in xs]
    launches = []
    out = _counting(lambda: head(dx), launches)
    assert launches == ["conv2d_bias_relu"] * 6 and list(out) == ["bbox_regression", "cls_logits"]
    for name, sub, cols in (("cls_logits", head.classification_head, classes), ("bbox_regression", head.regression_head, 4)):
        assert [tuple(m.shape) for m in out[name]] == [(2, a * cols, h, w) for a, (h, w) in zip(anchors, grids)]
        for l, conv in enumerate(sub.module_list):
            assert torch.equal(out[name][l], F.conv2d_bias_relu(dx[l], conv.weight, conv.bias, relu=False))
            want = oracle_conv3x3(ref, xs[l].numpy(), conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy(), relu=False)
            np.testing.assert_array_equal(out[name][l].detach().cpu().numpy(), want, err_msg=f"{name} level {l}")
        replica = (R.SSDClassificationHead([8, 8, 8], anchors, classes) if cols == classes else R.SSDRegressionHead([8, 8, 8], anchors))
        replica.load_state_dict({k: v.cpu() for k, v in sub.state_dict().items()}, strict=True)
        perm = sub.permuted(out[name]).detach().cpu()
        with torch.no_grad():
            theirs = replica(xs)
        assert perm.shape == theirs.shape == (2, sum(a * h * w for a, (h, w) in zip(anchors, grids)), cols)
        assert float((perm - theirs).abs().max()) <= 1e-4 * max(1.0, float(theirs.abs().max()))


def _by_hand(mods, x):
    """The library calls of a Conv2d / ReLU / MaxPool2d run, written out."""
    mods = list(mods)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Sequential):
            x = _by_hand(m, x)
        elif isinstance(m, nn.MaxPool2d):
            x = F.max_pool2d(x, m.kernel_size, m.stride, m.padding, ceil_mode=m.ceil_mode)
        elif isinstance(m, nn.Conv2d):
            if m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.dilation == (1, 1):
                x = F.conv2d_bias_relu(x, m.weight, m.bias, relu=True)
            else:
                x = F.conv2d_bias_act(x, m.weight, m.bias, stride=m.stride, padding=m.padding, dilation=m.dilation, activation="relu")
            i += 1  # the ReLU behind it
        i += 1
    return x


@pytest.fixture(scope="module")
def ssd300():
    torch.manual_seed(900)
    model = mv.ssd300_vgg16(num_classes=5)
    g = torch.Generator().manual_seed(901)
    with torch.no_grad():  # wider class logits than xavier gives on rescaled features, so that the scores spread
        for conv in model.head.classification_head.module_list:
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=g))
    return model.cuda()


def test_feature_extractor_stage_by_stage(ssd300):
    """SSDFeatureExtractorVGG at 300 x 300, N = 1: the six maps' sizes, the launch list, and every stage equal to the same library
    calls written out by hand."""
    bb = ssd300.backbone
    x = torch.from_numpy(philox_f32(910, (1, 3, 300, 300)) * 255 - 120).cuda()
    launches = []
    out = _counting(lambda: bb(x), launches)
    assert list(out) == ["0", "1", "2", "3", "4", "5"]
    assert [tuple(v.shape) for v in out.values()] == [(1, 512, 38, 38), (1, 1024, 19, 19), (1, 512, 10, 10), (1, 256, 5, 5), (1, 256, 3, 3),
                                                      (1, 256, 1, 1)]
    conv, act, pool = "conv2d_bias_relu", "conv2d_bias_act", "max_pool2d"
    assert launches == [conv, conv, pool, conv, conv, pool, conv, conv, conv, pool, conv, conv, conv, "l2_normalize_scale",
                        pool, conv, conv, conv, pool, act, act] + [act, act] * 4
    t = _by_hand(bb.features[:16], x)
    assert tuple(t.shape) == (1, 256, 75, 75)
    t = F.max_pool2d(t, 2, 2, 0, ceil_mode=True)
    assert tuple(t.shape) == (1, 256, 38, 38)
    t = _by_hand(bb.features[17:], t)
    assert torch.equal(out["0"], F.l2_normalize_scale(t, bb.scale_weight))
    R.same(out["0"][:, :, :3, :3], R.l2_normalize_scale(t[:, :, :3, :3].cpu(), bb.scale_weight.detach().cpu()), "conv4_3 rescaled")
    for i, block in enumerate(bb.extra):
        t = _by_hand(block, t)
        assert torch.equal(out[str(i + 1)], t), f"extra block {i}"
    assert float(out["5"].detach().abs().max()) > 0


def test_ssd300_stage_by_stage(ssd300):
    """ssd300_vgg16(num_classes=5) on two raw images of different sizes; every stage's reference is fed the library's own output of
    the stage before: the transform, the candidates bit for bit against the restatement, the detections = batched_nms of them, the
    boxes in the original coordinates, at most detections_per_img."""
    model = ssd300
    imgs = [torch.from_numpy(philox_f32(920, (3, 240, 320))), torch.from_numpy(philox_f32(921, (3, 333, 250)))]
    dimgs = [i.cuda() for i in imgs]
    images, _ = model.transform(dimgs, None)
    assert images.image_sizes == [(300, 300), (300, 300)] and tuple(images.tensors.shape) == (2, 3, 300, 300)
    theirs, _ = R.GeneralizedRCNNTransform(300, 300, model.transform.image_mean, model.transform.image_std, size_divisible=1,
                                           fixed_size=(300, 300))(imgs)
    assert float((images.tensors.cpu() - theirs.tensors).abs().max()) <= 1e-3 * 255
    feats = list(model.backbone(images.tensors).values())
    head_out = model.head(feats)
    cl, rg = ([m.detach().cpu() for m in head_out[name]] for name in ("cls_logits", "bbox_regression"))
    assert [tuple(m.shape) for m in cl] == [(2, a * 5, s, s) for a, s in zip((4, 6, 6, 6, 4, 4), (38, 19, 10, 5, 3, 1))]
    launches = []
    idx, boxes, scores, labels, valid = _counting(lambda: model.candidates(head_out, feats, images), launches)
    assert launches == ["ssd_scores", "ssd_topk", "ssd_decode"]
    sc = R.scores(cl, 5)
    want_idx = R.select(sc, 400, 0.01)
    assert idx.shape == (2, 1600) and torch.equal(idx.cpu(), want_idx)
    gen = model.anchor_generator
    grids = [tuple(m.shape[-2:]) for m in cl]
    dboxes = R.default_boxes(gen, grids, (300, 300))
    cpu_images = R.ImageList(images.tensors.cpu(), images.image_sizes)
    assert torch.equal(dboxes, gen(cpu_images, cl)[0]) and dboxes.shape == (8732, 4)
    wb, wsc, wl, wv = R.decode(sc, rg, want_idx, dboxes, images.image_sizes)
    R.same(boxes, wb, "boxes"), R.same(scores, wsc, "scores")
    assert torch.equal(labels.cpu(), wl) and torch.equal(valid.cpu(), wv)
    got = model(dimgs)
    for i, original in enumerate([(240, 320), (333, 250)]):
        b, s, lab = wb[i][wv[i]], wsc[i][wv[i]], wl[i][wv[i]]
        keep = R.batched_nms(b, s, lab, model.nms_thresh)[:model.detections_per_img]
        want_boxes = R.RH.resize_boxes(b[keep], (300, 300), original)
        n = len(keep)
        print(f"image {i}: {int(wv[i].sum())} candidates, {n} detections, classes {sorted(set(lab[keep].tolist()))}")
        assert 10 <= n <= model.detections_per_img == 200 and len(set(lab[keep].tolist())) >= 2, "the comparison shows nothing"
        R.same(got[i]["boxes"], want_boxes, f"boxes of image {i}")
        R.same(got[i]["scores"], s[keep], f"scores of image {i}")
        assert torch.equal(got[i]["labels"].cpu(), lab[keep])
        gb = got[i]["boxes"].detach()
        assert float(gb[:, 0::2].max()) <= original[1] + 1e-3 and float(gb[:, 1::2].max()) <= original[0] + 1e-3


class _SmallBackbone(nn.Module):
    """Two levels from three convs on the library's kernels, with out_channels."""

    def __init__(self):
        super().__init__()
        self.a, self.b, self.c = nn.Conv2d(3, 8, 3, padding=1), nn.Conv2d(8, 16, 3, padding=1), nn.Conv2d(16, 24, 3, padding=1)
        self.out_channels = [16, 24]

    def forward(self, x):
        from collections import OrderedDict
        x = F.max_pool2d(F.conv2d_bias_relu(x, self.a.weight, self.a.bias), 2, 2, 0, ceil_mode=True)
        x = F.max_pool2d(F.conv2d_bias_relu(x, self.b.weight, self.b.bias), 2, 2, 0, ceil_mode=True)
        y = F.max_pool2d(F.conv2d_bias_relu(x, self.c.weight, self.c.bias), 3, 2, 1, ceil_mode=True)
        return OrderedDict([("0", x), ("1", y)])


def test_small_two_level_ssd():
    """A 2-level SSD on a hand-made backbone exposing out_channels, a 45 x 37 fixed size (odd grids through the ceil-mode pools), no
    steps: the candidates against the restatement and the detections against batched_nms of them."""
    torch.manual_seed(950)
    gen = DefaultBoxGenerator([[2], [2, 3]], min_ratio=0.2, max_ratio=0.9)
    model = mv.SSD(_SmallBackbone(), gen, (37, 45), 4, image_mean=[0.5, 0.5, 0.5], image_std=[0.25, 0.25, 0.25], score_thresh=0.2, topk_candidates=30,
                   detections_per_img=25)
    _randomize(model.head, 951, 0.3)
    model = model.cuda()
    imgs = [torch.from_numpy(philox_f32(952, (3, 50, 41))), torch.from_numpy(philox_f32(953, (3, 45, 37))), torch.from_numpy(philox_f32(954, (3, 20, 64)))]
    dimgs = [i.cuda() for i in imgs]
    images, _ = model.transform(dimgs, None)
    assert tuple(images.tensors.shape) == (3, 3, 45, 37)
    feats = list(model.backbone(images.tensors).values())
    assert [tuple(f.shape) for f in feats] == [(3, 16, 12, 10), (3, 24, 7, 6)]
    head_out = model.head(feats)
    cl, rg = ([m.detach().cpu() for m in head_out[name]] for name in ("cls_logits", "bbox_regression"))
    idx, boxes, scores, labels, valid = model.candidates(head_out, feats, images)
    sc = R.scores(cl, 4)
    want_idx = R.select(sc, 30, 0.2)
    assert torch.equal(idx.cpu(), want_idx)
    dboxes = R.default_boxes(gen, [(12, 10), (7, 6)], (45, 37))
    assert torch.equal(dboxes, gen(R.ImageList(images.tensors.cpu(), images.image_sizes), cl)[0])
    wb, wsc, wl, wv = R.decode(sc, rg, want_idx, dboxes, images.image_sizes)
    R.same(boxes, wb, "boxes"), R.same(scores, wsc, "scores")
    assert torch.equal(labels.cpu(), wl) and torch.equal(valid.cpu(), wv)
    got = model(dimgs)
    for i, original in enumerate([(50, 41), (45, 37), (20, 64)]):
        b, s, lab = wb[i][wv[i]], wsc[i][wv[i]], wl[i][wv[i]]
        keep = R.batched_nms(b, s, lab, model.nms_thresh)[:25]
        assert 3 <= len(keep) <= 25
        R.same(got[i]["boxes"], R.RH.resize_boxes(b[keep], (45, 37), original), f"boxes of image {i}")
        R.same(got[i]["scores"], s[keep], f"scores of image {i}")
        assert torch.equal(got[i]["labels"].cpu(), lab[keep])
