"""FCOS on the GPU (`-m gpu`): F.group_norm_act (csrc/groupnorm.hip), F.fcos_topk, F.fcos_decode (csrc/retinanet.hip), FCOSHead and
FCOS.  The three kernels are compared bit for bit (NaN in equal places, == elsewhere) with the restatement (b) of tests/_fcos_ref.py
on the CPU, the head with the CPU oracle conv composed with the GroupNorm restatement."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _fcos_ref as R  # noqa: E402
from tests import _fpn_ref as PF  # noqa: E402
from tests import _rpn_ref as P  # noqa: E402
from tests._util import oracle_conv3x3, philox_f32  # noqa: E402
from tests.test_gpu_retinanet import _pattern, FIVE, HEAD_GRIDS, PATTERNS, T_LOGIT  # noqa: E402

THRESH = 0.2
NAN, INF = float("nan"), float("inf")


def _bits_equal(got, want, what=""):
    """Bit for bit but for the NaNs' payloads: NaN in equal places, the same int32 patterns elsewhere (-0 is not +0)."""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    a, b = got.view(torch.int32)[~nan], want.view(torch.int32)[~nan]
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {b.numel()} elements differ"


# ---- group_norm_act ---------------------------------------------------------------------------------------------------------------------
def _gn_check(x, groups, weight=None, bias=None, eps=1e-5, what="", dx=None):
    dx = x.cuda() if dx is None else dx
    dw, db = (None if p is None else p.cuda() for p in (weight, bias))
    out = {}
    for relu in (False, True):
        got = F.group_norm_act(dx, groups, dw, db, eps, relu=relu)
        assert _lib.last_kernel().startswith("k_gn_apply<") and _lib.last_kernel().endswith(f"relu{int(relu)}>")
        _bits_equal(got, R.group_norm(x, groups, weight, bias, eps, relu), f"{what} relu={relu}")
        out[relu] = got
    return out


def _affine(c, g):
    return torch.randn(c, generator=g) + 1, torch.randn(c, generator=g)


GN_SHAPES = [((1, 4, 3, 3), 2),      # m = 18: less than a wave
             ((2, 6, 5, 7), 3),      # m = 70: no multiple of 4
             ((2, 8, 5, 7), 8),      # G = C
             ((2, 8, 5, 7), 1),      # G = 1
             ((2, 256, 13, 17), 32),  # the head's form
             ((3, 12, 4, 4), 3)]     # m = 64, slabs on 16 bytes: the dwordx4 form


@pytest.mark.parametrize("shape,groups", GN_SHAPES)
def test_group_norm_equals_the_restatement(shape, groups):
    g = torch.Generator().manual_seed(9000 + shape[1] * 10 + groups)
    x = torch.randn(shape, generator=g) * 2 + 0.3
    w, b = _affine(shape[1], g)
    _gn_check(x, groups, w, b, what=f"{shape} G={groups}")
    _gn_check(x, groups, what=f"{shape} G={groups} no affine")
    _gn_check(x, groups, w, None, eps=1e-3, what=f"{shape} G={groups} weight only")
    _gn_check(x, groups, None, b, what=f"{shape} G={groups} bias only")


def test_group_norm_around_the_statistics_chunk():
    """Slabs of exactly one chunk, one chunk + 1, two chunks - 1 and 2 chunks + 4 elements, sized by the library's accessor: the
    scalar and the dwordx4 form (m % 4 == 0), one and several partials per slab."""
    c = F.group_norm_chunk()
    assert c == R.GN_CHUNK == _lib.load().mv_group_norm_chunk()
    g = torch.Generator().manual_seed(9010)
    forms = set()
    for m in (c, c + 1, 2 * c - 1, 2 * c + 4):
        x = torch.randn((2, 4, 1, m // 2 if m % 2 == 0 else m), generator=g) * 3 + 1
        groups = 2 if m % 2 == 0 else 4  # two channels per group, or one
        assert (4 // groups) * x.shape[3] == m
        w, b = _affine(4, g)
        _gn_check(x, groups, w, b, what=f"m={m}")
        forms.add(_lib.last_kernel().split("<")[1].split(",")[0])
    assert forms == {"vec", "scalar"}


def test_group_norm_channel_slice_and_in_place():
    g = torch.Generator().manual_seed(9020)
    big = torch.randn((3, 32, 5, 7), generator=g)
    w, b = _affine(16, g)
    dbig = big.cuda()
    view = dbig[:, 8:24]
    assert not view.is_contiguous()
    _gn_check(big[:, 8:24].contiguous(), 4, w, b, what="channel slice", dx=view)
    assert torch.equal(dbig.cpu(), big), "the input is left alone"
    # exactly in place
    x = torch.randn((2, 6, 5, 7), generator=g)
    dx = x.cuda()
    ptr = dx.data_ptr()
    got = F.group_norm_act(dx, 3, w[:6].cuda(), b[:6].cuda(), relu=True, out=dx)
    assert got is dx and dx.data_ptr() == ptr
    _bits_equal(dx, R.group_norm(x, 3, w[:6], b[:6], relu=True), "in place")
    sparse = view[:, :, :, ::2]
    with pytest.raises(ValueError, match="dense images"):
        F.group_norm_act(sparse, 4, out=sparse)


def test_group_norm_degenerate_values():
    g = torch.Generator().manual_seed(9030)
    w, b = _affine(6, g)
    # a constant slab: var = 0, rstd = 1 / sqrt(eps), x - mean = 0 -> the output is beta (and 0 * gamma = +-0)
    x = torch.randn((2, 6, 5, 7), generator=g)
    x[0, 2:4] = 3.25
    out = _gn_check(x, 3, w, b, what="constant slab")
    assert torch.equal(out[False][0, 2:4].cpu(), b[2:4, None, None].expand(2, 5, 7))
    # mean 1000, std 1: E[x^2] - mean^2 in float64
    x = torch.randn((2, 6, 5, 7), generator=g) + 1000
    out = _gn_check(x, 3, w, b, what="mean 1000")
    f64 = torch.nn.functional.group_norm(x.double(), 3, w.double(), b.double(), 1e-5)
    assert float((out[False].cpu().double() - f64).abs().max()) <= 1e-4 * float(f64.abs().max())


def test_group_norm_nan_and_inf_stay_in_their_slab():
    g = torch.Generator().manual_seed(9040)
    base = torch.randn((3, 6, 5, 7), generator=g)
    w, b = _affine(6, g)
    clean = _gn_check(base, 3, w, b, what="clean")[False].cpu()
    for value in (NAN, INF, -INF):
        x = base.clone()
        x[1, 2, 3, 4] = value  # image 1, group 1
        got = _gn_check(x, 3, w, b, what=f"{value}")[False].cpu()
        poisoned = torch.zeros_like(x, dtype=torch.bool)
        poisoned[1, 2:4] = True
        assert bool(torch.isnan(got[poisoned]).all()), "the whole slab is NaN"
        assert torch.equal(got[~poisoned], clean[~poisoned]), "and no other slab changed"


def test_group_norm_does_not_depend_on_the_position():
    """The same slab values at image 0 / group 0 and at image 2 / the last group, in a batch of 3 and alone, aligned and not."""
    g = torch.Generator().manual_seed(9050)
    for shape, groups in (((3, 6, 5, 7), 3), ((3, 8, 2, 4 * 1100), 4)):  # m = 70 (scalar), m = 17600 (vec, five chunks)
        n, c, h, w_ = shape
        cpg = c // groups
        x = torch.randn(shape, generator=g) * 2 + 0.5
        slab = torch.randn((cpg, h, w_), generator=g) * 3 - 1
        x[0, :cpg] = slab
        x[2, c - cpg:] = slab
        w, b = torch.randn(cpg, generator=g).repeat(groups), torch.randn(cpg, generator=g).repeat(groups)
        got = F.group_norm_act(x.cuda(), groups, w.cuda(), b.cuda(), relu=True).cpu()
        _bits_equal(got[0, :cpg], got[2, c - cpg:], f"{shape}")
        alone = F.group_norm_act(slab[None].cuda(), 1, w[:cpg].cuda(), b[:cpg].cuda(), relu=True).cpu()
        _bits_equal(alone[0], got[0, :cpg], f"{shape} alone")
        # one float further: the slab is no longer on 16 bytes
        flat = torch.zeros(slab.numel() + 1, device="cuda")
        flat[1:] = slab.flatten().cuda()
        off = F.group_norm_act(flat[1:].view(1, cpg, h, w_), 1, w[:cpg].cuda(), b[:cpg].cuda(), relu=True).cpu()
        _bits_equal(off[0], got[0, :cpg], f"{shape} misaligned")


# ---- fcos_topk --------------------------------------------------------------------------------------------------------------------------
def _check(cls, ctr, classes, k, thresh=THRESH, what=""):
    got = F.fcos_topk([m.cuda() for m in cls], [m.cuda() for m in ctr], classes, k, thresh)
    assert _lib.last_kernel() == f"k_retinanet_rank<fcos,levels{len(cls)},k{k}>"
    want = R.select(cls, ctr, classes, k, thresh)
    assert got.dtype == torch.int32 and tuple(got.shape) == tuple(want.shape), what
    assert torch.equal(got.cpu(), want), f"{what} k={k}: {int((got.cpu() != want).sum())} of {want.numel()} indices differ"
    return want


@pytest.mark.parametrize("classes", [1, 5, 91])
def test_topk_grid(classes):
    g = torch.Generator().manual_seed(9100 + classes)
    cls = [torch.randn((2, classes, h, w), generator=g) * 3 for h, w in FIVE]
    ctr = [torch.randn((2, 1, h, w), generator=g) * 2 for h, w in FIVE]
    for k in (1, 7, 1000, 4096):
        want = _check(cls, ctr, classes, k, what=f"K={classes}")
    assert bool((want >= 0).any()) and bool((want == -1).any())
    # channel slices of wider tensors: the image strides are larger than the maps
    wide = [torch.cat([m, c, torch.full_like(c, 30.0)], 1).cuda() for m, c in zip(cls, ctr)]
    got = F.fcos_topk([w[:, :classes] for w in wide], [w[:, classes:classes + 1] for w in wide], classes, 1000, THRESH)
    assert torch.equal(got.cpu(), R.select(cls, ctr, classes, 1000, THRESH))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_topk_patterns(pattern):
    """The logit patterns of tests/test_gpu_retinanet.py on the class map with a random centerness map, and on the centerness map
    with a random class map."""
    g = torch.Generator().manual_seed(9200 + PATTERNS.index(pattern))
    classes = 5
    for on_ctr in (False, True):
        cls = [(torch.randn((2, classes, h, w), generator=g) * 3) if on_ctr else _pattern(pattern, (2, classes, h, w), g) for h, w in FIVE]
        ctr = [_pattern(pattern, (2, 1, h, w), g) if on_ctr else torch.randn((2, 1, h, w), generator=g) for h, w in FIVE]
        thresh = float(R.score(torch.tensor(T_LOGIT), torch.tensor(T_LOGIT))) if pattern == "at the threshold" else THRESH
        for k in (7, 1000):
            want = _check(cls, ctr, classes, k, thresh, what=f"{pattern} on_ctr={on_ctr}")
        if pattern == "zeros nan inf":  # a NaN in either map never passes
            s = R.level_scores(cls[0], ctr[0], classes)
            taken = want[0, :min(1000, s.shape[1])]
            taken = taken[taken >= 0].long()
            assert bool(torch.isnan(s).any()) and not bool(torch.isnan(s[0][taken]).any())


def test_topk_all_equal_none_passing_exactly_k():
    classes, h, w = 5, 7, 9
    n0 = classes * h * w
    # all scores equal and passing: ascending flat index
    cls, ctr = [torch.full((2, classes, h, w), 0.5)], [torch.full((2, 1, h, w), 0.25)]
    for k in (7, 100, 1000):
        want = _check(cls, ctr, classes, k, what="all equal")
        assert torch.equal(want, torch.arange(min(k, n0), dtype=torch.int32)[None].expand(2, -1))
    # the shipped initialisation: every score near sqrt(0.01 * 0.5), none passes
    cls, ctr = [torch.full((2, classes, h, w), -math.log(99.0))], [torch.zeros((2, 1, h, w))]
    assert bool((_check(cls, ctr, classes, 100, what="none passing") == -1).all())
    # exactly 7 passing
    cls, ctr = [torch.full((1, classes, h, w), -10.0)], [torch.zeros((1, 1, h, w))]
    flat_pos = [5, 17, 100, 101, 250, 300, 314]
    for j, f in enumerate(flat_pos):  # flat f = pos * K + c -> channel c at pos
        cls[0].view(-1)[(f % classes) * h * w + f // classes] = 1.0 + (j % 3)
    assert int((R.level_scores(cls[0], ctr[0], classes) > THRESH).sum()) == 7
    for k in (6, 7, 8, 1000):
        want = _check(cls, ctr, classes, k, what="exactly 7 passing")
        assert int((want >= 0).sum()) == min(k, 7) and want.shape[1] == min(k, n0)
    assert F.fcos_topk([cls[0].cuda()], [ctr[0].cuda()], classes, 8, THRESH).cpu()[0].tolist() == [100, 300, 17, 250, 5, 101, 314, -1]
    # the centerness decides: equal class logits, the order is the centerness's
    cls, ctr = [torch.full((1, 2, 2, 3), 1.0)], [torch.tensor([0.5, -1.0, 2.0, 0.0, 3.0, -9.0]).reshape(1, 1, 2, 3)]
    assert F.fcos_topk([cls[0].cuda()], [ctr[0].cuda()], 2, 12, THRESH).cpu()[0].tolist() == [8, 9, 4, 5, 0, 1, 6, 7, 2, 3, -1, -1]


def test_topk_across_the_stage_1_chunks():
    """One level of C - 1, C + 1 and 3 C + 1 candidates for the stage-1 chunk C, and one of K = 5 classes of more than 3 C whose
    flat order is not its memory order.  Few distinct values: runs of equal scores cover every chunk boundary."""
    c = F.retinanet_topk_chunk()
    g = torch.Generator().manual_seed(9300)
    for classes, h, w in ((1, 1, c - 1), (1, 1, c + 1), (1, 1, 3 * c + 1), (5, 1, 3 * c // 5 + 7)):
        cls = torch.tensor([-4.0, 0.5, 0.75, 3.0])[torch.randint(0, 4, (2, classes, h, w), generator=g)]
        ctr = torch.tensor([-1.0, 0.0, 2.0])[torch.randint(0, 3, (2, 1, h, w), generator=g)]
        for edge in range(c, classes * h * w, c):
            cls.flatten(1)[:, edge - 2:edge + 2] = 0.75
        for k in (7, 1000, 4096):
            want = _check([cls], [ctr], classes, k, what=f"{(classes, h, w)}")
            assert int((want >= 0).sum()) == 2 * min(k, classes * h * w)


# ---- fcos_decode ------------------------------------------------------------------------------------------------------------------------
PADDED, SIZES = (104, 136), [(104, 136), (97, 120)]
STRIDES = [(PADDED[0] // h, PADDED[1] // w) for h, w in FIVE]


def _decode_inputs(seed, classes=5):
    g = torch.Generator().manual_seed(seed)
    cls = [torch.randn((2, classes, h, w), generator=g) * 3 for h, w in FIVE]
    ctr = [torch.randn((2, 1, h, w), generator=g) * 2 for h, w in FIVE]
    reg = [torch.randn((2, 4, h, w), generator=g) * 1.5 for h, w in FIVE]  # half of them negative: rectified by the kernel
    for d in reg[:3]:
        f = d.view(2, 4, -1)
        f[0, 0, 1], f[1, 3, 2], f[0, 2, 3] = NAN, NAN, INF
        f[1, 1, 0], f[0, 3, 4] = -INF, 40.0
    return cls, ctr, reg


def test_decode_equals_the_restatement():
    classes = 5
    cls, ctr, reg = _decode_inputs(9400)
    ag = R.default_anchorgen()
    anchors = ag(P.ImageList(torch.zeros(2, 3, *PADDED), SIZES), cls)
    total = anchors[0].shape[0]
    d = [[m.cuda() for m in maps] for maps in (cls, ctr, reg)]
    sel = F.fcos_topk(d[0], d[1], classes, 1000, THRESH)
    assert torch.equal(sel.cpu(), R.select(cls, ctr, classes, 1000, THRESH))
    hand = torch.tensor([[-1, total * classes, 2 ** 31 - 1, 0, total * classes - 1, 7, -5, 1234],
                         [3, -1, total * classes + 1, 2 ** 30, 44, total * classes - 2, 1, -2 ** 31]], dtype=torch.int32)
    idx = torch.cat([sel.cpu(), hand], 1)
    boxes, scores, labels, valid = F.fcos_decode(d[0], d[1], d[2], idx.cuda(), ag.cell_anchors, STRIDES, SIZES, classes)
    assert _lib.last_kernel() == "k_fcos_decode<levels5>"
    wb, wsc, wl, wv = R.decode(cls, ctr, reg, idx, anchors, SIZES, classes)
    _bits_equal(boxes, wb, "boxes"), _bits_equal(scores, wsc, "scores")
    assert labels.dtype == torch.int64 and torch.equal(labels.cpu(), wl)
    assert valid.dtype == torch.bool and torch.equal(valid.cpu(), wv)
    # what the comparison covers
    ok = (idx >= 0) & (idx.long() < total * classes)
    assert torch.equal(wv, ok) and hand.shape[1] - int(ok[0, -8:].sum()) == 4
    assert float(wb[~ok].abs().max()) == 0 and float(wsc[~ok].abs().max()) == 0 and int(wl[~ok].abs().max()) == 0
    assert torch.equal(wl[ok], idx[ok].long() % classes) and bool(torch.isnan(wb).any())
    for i, (ih, iw) in enumerate(SIZES):  # boxes clipped on every side of both images
        b = wb[i][ok[i]]
        assert bool((b[:, 0] == 0).any()) and bool((b[:, 1] == 0).any()) and bool((b[:, 2] == iw).any()) and bool((b[:, 3] == ih).any())
    # the kernel rectifies: the rectified maps give the same bits, and negative distances alone give the anchors' centres
    rect = F.fcos_decode(d[0], d[1], [torch.relu(m) for m in d[2]], idx.cuda(), ag.cell_anchors, STRIDES, SIZES, classes)
    _bits_equal(rect[0], wb, "rectified maps")
    assert any(bool((m < 0).any()) for m in reg)
    neg = F.fcos_decode(d[0], d[1], [-torch.rand_like(m) for m in d[2]], sel, ag.cell_anchors, STRIDES, [(4096, 4096)] * 2, classes)
    for i in range(2):
        f = sel[i].cpu().long()
        a = anchors[i][f[f >= 0] // classes]
        centre = torch.stack([0.5 * (a[:, 0] + a[:, 2]), 0.5 * (a[:, 1] + a[:, 3])] * 2, 1).clamp(min=0)
        assert torch.equal(neg[0][i].cpu()[f >= 0], centre)


# ---- the head ---------------------------------------------------------------------------------------------------------------------------
def _randomize(module, seed, std=0.03):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * std + (1.0 if p.dim() == 1 and p.numel() == 256 else 0.0))


def _counting(call, launches, names=("conv2d_bias_relu", "group_norm_act", "fcos_topk", "fcos_decode")):
    originals = {n: getattr(F, n) for n in names}

    def wrap(n):
        def wrapped(*a, **k):
            launches.append(n)
            return originals[n](*a, **k)
        return wrapped
    try:
        for n in originals:
            setattr(F, n, wrap(n))
        return call()
    finally:
        for n, f in originals.items():
            setattr(F, n, f)


LEVEL_LAUNCHES = ["conv2d_bias_relu", "group_norm_act"] * 4 + ["conv2d_bias_relu"] + \
                 ["conv2d_bias_relu", "group_norm_act"] * 4 + ["conv2d_bias_relu"] * 2  # the class tower, then the regression tower


def test_head_equals_the_oracle_composition():
    """FCOSHead(256, 1, 5) on the five levels of a 128 x 160 batch of two: the launch list, the layer-by-layer composition of
    F.conv2d_bias_relu and F.group_norm_act, and the CPU oracle conv composed with the GroupNorm restatement, bit for bit."""
    head = mv.FCOSHead(256, 1, 5)
    _randomize(head, 9500)
    xs = [philox_f32(9510 + i, (2, 256, h, w)) * 2 - 1 for i, (h, w) in enumerate(HEAD_GRIDS)]
    head = head.cuda()
    dxs = [torch.from_numpy(x).cuda() for x in xs]
    launches = []
    out = _counting(lambda: head(dxs), launches)
    # per head all levels: the class head's five levels, then the regression head's
    per_cls, per_reg = LEVEL_LAUNCHES[:9], LEVEL_LAUNCHES[9:]
    assert launches == per_cls * 5 + per_reg * 5, launches
    ch, rh = head.classification_head, head.regression_head
    finals = ((ch.conv, ch.cls_logits, False, "cls_logits", 5), (rh.conv, rh.bbox_reg, True, "bbox_regression", 4),
              (rh.conv, rh.bbox_ctrness, False, "bbox_ctrness", 1))
    for l, x in enumerate(dxs):
        for tower, last, relu, name, channels in finals:
            t = x
            layers = list(tower)
            for i in range(0, 12, 3):
                t = F.conv2d_bias_relu(t, layers[i].weight, layers[i].bias, relu=False)
                t = F.group_norm_act(t, 32, layers[i + 1].weight, layers[i + 1].bias, 1e-5, relu=True)
            want = F.conv2d_bias_relu(t, last.weight, last.bias, relu=relu)
            got = out[name][l]
            assert tuple(got.shape) == (2, channels) + HEAD_GRIDS[l]
            assert torch.equal(got.detach(), want.detach()), f"level {l} {name}"
            assert float(got.detach().abs().max()) > 1e-3
    assert all(float(m.detach().min()) >= 0 for m in out["bbox_regression"]) and any(float(m.detach().min()) < 0 for m in out["bbox_ctrness"])
    cpu = lambda p: p.detach().cpu()  # noqa: E731
    for l in range(5):
        for tower, last, relu, name, _ in finals:
            t = xs[l]
            layers = list(tower)
            for i in range(0, 12, 3):
                t = oracle_conv3x3(ref, t, cpu(layers[i].weight).numpy(), cpu(layers[i].bias).numpy(), relu=False)
                t = R.group_norm(torch.from_numpy(np.ascontiguousarray(t)), 32, cpu(layers[i + 1].weight), cpu(layers[i + 1].bias), 1e-5, relu=True).numpy()
            want = oracle_conv3x3(ref, t, cpu(last.weight).numpy(), cpu(last.bias).numpy(), relu=relu)
            np.testing.assert_array_equal(out[name][l].detach().cpu().numpy(), want, err_msg=f"level {l} {name}")
    # the reference's layout for anyone who asks
    cat = mv.retinanet.concat_layout(out["bbox_ctrness"], 1)
    assert tuple(cat.shape) == (2, sum(h * w for h, w in HEAD_GRIDS), 1) and cat[1, 3 * 20 + 4, 0] == out["bbox_ctrness"][0][1, 0, 3, 4]


# ---- the whole model --------------------------------------------------------------------------------------------------------------------
def test_fcos_end_to_end_stage_by_stage():
    """resnet18 FPN on layer2 .. layer4 + P6 / P7, 5 classes, two images; every stage's reference is fed the library's own output of
    the stage before.  cls_logits is re-initialised with a wider weight (std 0.02) and a bias of -3.5 so that detections exist: the
    shipped initialisation puts every score near sqrt(0.01 * 0.5) = 0.07, below the threshold 0.2.  The constants were chosen on the
    replica's own head on the CPU (72 and 57 detections in 4 classes there)."""
    torch.manual_seed(9900)
    replica_bb = PF.resnet_fpn_backbone(backbone_name="resnet18", returned_layers=[2, 3, 4], extra_blocks=PF.LastLevelP6P7(256, 256)).eval()
    PF.randomize(replica_bb, 9901)
    backbone = mv.resnet_fpn_backbone(backbone_name="resnet18", returned_layers=[2, 3, 4], extra_blocks=mv.LastLevelP6P7(256, 256))
    backbone.load_state_dict(replica_bb.state_dict(), strict=True)
    model = mv.FCOS(backbone, 5, topk_candidates=100, _skip_resize=True)
    g = torch.Generator().manual_seed(9902)
    with torch.no_grad():
        for p in model.head.parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * 0.03)
        c = model.head.classification_head.cls_logits
        c.weight.copy_(torch.randn(c.weight.shape, generator=g) * 0.02)
        c.bias.fill_(-3.5)
    model = model.cuda()
    imgs = [torch.from_numpy(philox_f32(9904, (3, 128, 160))), torch.from_numpy(philox_f32(9905, (3, 120, 150)))]
    dimgs = [i.cuda() for i in imgs]

    images, _ = model.transform(dimgs, None)
    assert images.image_sizes == [(128, 160), (120, 150)] and tuple(images.tensors.shape) == (2, 3, 128, 160)
    feats = model.backbone(images.tensors)
    assert list(feats) == ["0", "1", "2", "p6", "p7"] and [tuple(f.shape[2:]) for f in feats.values()] == list(HEAD_GRIDS)
    # head maps
    launches = []
    head_out = _counting(lambda: model.head(list(feats.values())), launches)
    assert launches == LEVEL_LAUNCHES[:9] * 5 + LEVEL_LAUNCHES[9:] * 5
    cl, rg, ct = ([m.detach().cpu() for m in head_out[name]] for name in ("cls_logits", "bbox_regression", "bbox_ctrness"))
    assert [tuple(m.shape) for m in cl] == [(2, 5) + s for s in HEAD_GRIDS] and [tuple(m.shape) for m in rg] == [(2, 4) + s for s in HEAD_GRIDS]
    assert [tuple(m.shape) for m in ct] == [(2, 1) + s for s in HEAD_GRIDS]
    # the head is close to the replica's float32 head on the library's features
    replica = R.FCOSHead(256, 1, 5).eval()
    replica.load_state_dict({k: v.cpu() for k, v in model.head.state_dict().items()}, strict=True)
    with torch.no_grad():
        want_cl = replica.classification_head.maps([f.detach().cpu() for f in feats.values()])
    for a, b in zip(cl, want_cl):
        assert float((a - b).abs().max()) <= 1e-3 * max(1.0, float(b.abs().max()))
    # idx and the decoded candidates, bit for bit
    launches.clear()
    idx, boxes, scores, labels, valid = _counting(lambda: model.candidates(head_out, images.tensors.shape[-2:], images.image_sizes), launches)
    assert launches == ["fcos_topk", "fcos_decode"]
    want_idx = R.select(cl, ct, 5, 100, 0.2)
    assert torch.equal(idx.cpu(), want_idx)
    cpu_images = P.ImageList(images.tensors.cpu(), images.image_sizes)
    anchors = R.default_anchorgen()(cpu_images, cl)
    wb, wsc, wl, wv = R.decode(cl, ct, rg, want_idx, anchors, images.image_sizes, 5)
    _bits_equal(boxes, wb, "boxes"), _bits_equal(scores, wsc, "scores")
    assert torch.equal(labels.cpu(), wl) and torch.equal(valid.cpu(), wv)
    # nms and the rescaled boxes: the restatement's FCOS on the library's head maps
    want = R.FCOS(replica_bb, 5, topk_candidates=100, numerics=P.RESTATEMENT).eval().from_head_maps(cpu_images, cl, rg, ct)
    got = model(dimgs)
    for i in range(2):
        n = len(want[i]["boxes"])
        print(f"image {i}: {n} detections, classes {sorted(set(want[i]['labels'].tolist()))}, {int(wv[i].sum())} candidates")
        assert 10 <= n < model.detections_per_img == 100 and len(set(want[i]["labels"].tolist())) >= 2, "the comparison shows nothing"
        P.same(got[i]["boxes"], want[i]["boxes"], f"boxes of image {i}")
        P.same(got[i]["scores"], want[i]["scores"], f"scores of image {i}")
        assert torch.equal(got[i]["labels"].cpu(), want[i]["labels"])


# ---- image stride past 2^31 -------------------------------------------------------------------------------------------------------------
def test_image_stride_past_2_to_31_elements():
    """n = 2 images 2^31 + 64 elements apart in one allocation of about 8 GiB holding the class and the centerness maps: image 1's
    result equals the same maps run alone, so the map offsets of both kernels are 64-bit."""
    classes, h, w = 6, 5, 7
    stride = 2 ** 31 + 64
    numel, hw = classes * h * w, h * w
    g = torch.Generator().manual_seed(9700)
    m = torch.randn((2, classes, h, w), generator=g) * 3
    c = torch.randn((2, 1, h, w), generator=g) * 2
    d = torch.randn((2, 4, h, w), generator=g)
    try:
        big = torch.empty(stride + numel + hw, dtype=torch.float32, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.fail("8 GiB of device memory are not available")
    for i in range(2):
        big[i * stride:i * stride + numel] = m[i].flatten().cuda()
        big[i * stride + numel:i * stride + numel + hw] = c[i].flatten().cuda()
    view = torch.as_strided(big, (2, classes, h, w), (stride, hw, w, 1))
    cview = torch.as_strided(big, (2, 1, h, w), (stride, hw, w, 1), numel)
    idx = F.fcos_topk([view], [cview], classes, 50, THRESH)
    alone = F.fcos_topk([m[1:].cuda()], [c[1:].cuda()], classes, 50, THRESH)
    assert torch.equal(idx[1], alone[0]) and torch.equal(idx.cpu(), R.select([m], [c], classes, 50, THRESH))
    cell = [torch.tensor([[-4.0, -4, 4, 4]])]
    got = F.fcos_decode([view], [cview], [d.cuda()], idx, cell, [(8, 8)], [(40, 56), (33, 50)], classes)
    want = F.fcos_decode([m[1:].cuda()], [c[1:].cuda()], [d[1:].cuda()], alone, cell, [(8, 8)], [(33, 50)], classes)
    for gt, wt in zip(got, want):
        P.same(gt[1], wt[0])
    assert bool(got[3][1].any())
    del big, view, cview
    torch.cuda.empty_cache()
