"""RetinaNet on the GPU (`-m gpu`): F.retinanet_topk, F.retinanet_decode (csrc/retinanet.hip), RetinaNetHead and RetinaNet.  The
two kernels are compared bit for bit (NaN in equal places, == elsewhere) with the restatement (b) of tests/_retinanet_ref.py on
the CPU, the head with the CPU oracle in the summation order the library states."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _fpn_ref as PF  # noqa: E402
from tests import _retinanet_ref as R  # noqa: E402
from tests import _rpn_ref as P  # noqa: E402
from tests._util import oracle_conv3x3, philox_f32  # noqa: E402

CLIP = math.log(1000.0 / 16)
THRESH = 0.05
LEVEL_SETS = [((1, 1),), ((2, 3), (1, 1)), ((13, 17), (7, 9), (4, 5), (2, 3), (1, 1))]
FIVE = LEVEL_SETS[2]
KS = (1, 7, 1000, 4096)


def bits(patterns):
    return patterns.to(torch.int32).view(torch.float32)


def _check(maps, classes, k, thresh=THRESH, dmaps=None, what=""):
    got = F.retinanet_topk(dmaps if dmaps is not None else [m.cuda() for m in maps], classes, k, thresh)
    want = R.select(maps, classes, k, thresh)
    assert got.dtype == torch.int32 and tuple(got.shape) == tuple(want.shape), what
    assert torch.equal(got.cpu(), want), f"{what} k={k}: {int((got.cpu() != want).sum())} of {want.numel()} indices differ"
    return want


# ---- top-k: the grid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,classes", [(1, 1), (3, 2), (9, 5), (9, 91)])
def test_topk_grid(a, classes):
    g = torch.Generator().manual_seed(9100 + a * 100 + classes)
    for levels in LEVEL_SETS:
        maps = [torch.randn((2, a * classes, h, w), generator=g) * 3 for h, w in levels]  # two images with different data
        # channel slices of a wider tensor: the image stride is larger than the map
        wide = [torch.cat([m, torch.full((2, 3) + tuple(m.shape[2:]), 30.0)], 1).cuda() for m in maps]
        sliced = [w[:, :m.shape[1]] for w, m in zip(wide, maps)]
        assert all(s.stride(0) == m[0].numel() + 3 * m.shape[2] * m.shape[3] for s, m in zip(sliced, maps))
        for k in KS:
            want = _check(maps, classes, k, dmaps=sliced, what=f"A={a} K={classes} {levels} sliced")
            assert _lib.last_kernel() == f"k_retinanet_rank<levels{len(levels)},k{k}>"
            assert torch.equal(F.retinanet_topk([m.cuda() for m in maps], classes, k, THRESH).cpu(), want)


# ---- top-k: chunk crossing ------------------------------------------------------------------------------------------------------------
def test_topk_across_the_stage_1_chunks():
    """One level of exactly C, C - 1, C + 1 and 3 C + 1 candidates for the stage-1 chunk size C the library reports, and a (3, 2)
    level of more than 3 C whose flat order is not its memory order.  Four distinct logits: runs of equal scores cover every chunk
    boundary, and far more than k candidates pass."""
    c = F.retinanet_topk_chunk()
    assert c == _lib.load().mv_retinanet_topk_chunk() and c >= 1024
    g = torch.Generator().manual_seed(9200)
    shapes = [(1, 1, 1, c), (1, 1, 1, c - 1), (1, 1, 1, c + 1), (1, 1, 1, 3 * c + 1), (3, 2, 1, 3 * c // 6 + 1)]
    for a, classes, h, w in shapes:
        m = torch.tensor([-4.0, 0.5, 0.75, 3.0])[torch.randint(0, 4, (2, a * classes, h, w), generator=g)]
        flat = R.permute_level(m, classes).flatten(1)
        for edge in range(c, a * classes * h * w, c):  # equal scores on both sides of every boundary, in memory order
            mem = m.flatten(1)
            mem[:, edge - 2:edge + 2] = 0.75
        for k in (7, 1000, 4096):
            want = _check([m], classes, k, what=f"{(a, classes, h, w)}")
            assert int((want >= 0).sum()) == 2 * min(k, flat.shape[1])
    # all equal and all passing: the first k flat indices, in order, whichever chunks they lie in
    for a, classes, h, w in shapes[3:]:
        m = torch.full((1, a * classes, h, w), 0.25)
        for k in (1000, 4096):
            assert F.retinanet_topk([m.cuda()], classes, k, THRESH).cpu()[0].tolist() == list(range(k))


# ---- top-k: logit patterns ------------------------------------------------------------------------------------------------------------
T_LOGIT = -1.25
T_SCORE = float(R.sigmoid_cr(torch.tensor(T_LOGIT)))  # a threshold that IS a score: the float32 value, passed exactly


def _pattern(name, shape, g):
    n = int(np.prod(shape))
    if name == "normal":
        v = torch.randn(n, generator=g) * 3
    elif name == "all equal":
        v = torch.full((n,), 0.5)
    elif name == "all below":
        v = torch.full((n,), -math.log(99.0))  # the shipped cls_logits bias with zero weights: score 0.01
    elif name == "all above":
        v = torch.full((n,), 20.0)
    elif name == "equal scores":
        v = torch.tensor([18.0, 20.0, 25.0, 88.0])[torch.randint(0, 4, (n,), generator=g)]
    elif name == "at the threshold":
        x = torch.tensor(T_LOGIT)
        near = [x]
        for _ in range(3):
            near = [torch.nextafter(near[0], torch.tensor(-9.0))] + near + [torch.nextafter(near[-1], torch.tensor(9.0))]
        v = torch.stack(near)[torch.randint(0, 7, (n,), generator=g)]
    elif name == "zeros nan inf":
        v = torch.randn(n, generator=g)
        r = torch.rand(n, generator=g)
        v[r < 0.1] = float("nan")
        v[(r >= 0.1) & (r < 0.2)] = float("inf")
        v[(r >= 0.2) & (r < 0.3)] = float("-inf")
        v[(r >= 0.3) & (r < 0.4)] = 0.0
        v[(r >= 0.4) & (r < 0.5)] = -0.0
        v = torch.where((r >= 0.5) & (r < 0.55), bits(torch.tensor([0xFFC00001])), v)  # a NaN with the sign bit and a payload
    else:
        raise AssertionError(name)
    return v.reshape(shape)


PATTERNS = ["normal", "all equal", "all below", "all above", "equal scores", "at the threshold", "zeros nan inf"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_topk_patterns(pattern):
    g = torch.Generator().manual_seed(9300 + PATTERNS.index(pattern))
    thresh = T_SCORE if pattern == "at the threshold" else THRESH
    for a, classes in ((3, 2), (9, 5)):
        maps = [_pattern(pattern, (2, a * classes, h, w), g) for h, w in FIVE]
        for k in (7, 1000):
            want = _check(maps, classes, k, thresh, what=pattern)
        n0 = a * classes * 13 * 17
        seg = want[:, :min(1000, n0)]
        if pattern == "all below":
            assert bool((want == -1).all())
        if pattern in ("all equal", "all above", "equal scores"):  # one score: ascending flat index, whatever the logits
            assert torch.equal(seg, torch.arange(seg.shape[1], dtype=torch.int32)[None].expand(2, -1))
        if pattern == "equal scores":
            assert bool((R.sigmoid_cr(maps[0]) == 1.0).all()) and len(torch.unique(maps[0])) == 4
        if pattern == "at the threshold":
            s = R.sigmoid_cr(maps[0])
            t = torch.tensor(T_SCORE)
            assert bool((s == t).any()) and bool((s < t).any()) and bool((s > t).any()), "scores on both sides of and at the threshold"
            assert int((want[:, :min(1000, n0)] >= 0).sum()) == min(int((s[0] > t).sum()), 1000) + min(int((s[1] > t).sum()), 1000)
        if pattern == "zeros nan inf":
            flat = R.permute_level(maps[0], classes).flatten(1)
            taken = seg[0][seg[0] >= 0].long()
            assert not bool(torch.isnan(flat[0][taken]).any()) and bool(torch.isnan(flat).any())
            assert bool((flat[0][taken[:5]] == float("inf")).all())  # score 1 first; -inf has the score 0 and does not pass
        if pattern == "normal":
            assert bool((want[:, -1000:] == -1).any()) and bool((want[:, :7] >= 0).all())  # small levels are padded


def test_topk_exactly_k_and_fewer_than_k_passing():
    a, classes, h, w = 3, 2, 7, 9
    m = torch.full((1, a * classes, h, w), -10.0)
    flat_pos = [5, 17, 100, 101, 250, 300, 377]
    mem = m.view(-1)
    for j, f in enumerate(flat_pos):  # flat f = (pos * A + a) * K + c -> channel a K + c at pos
        pos, ch = f // (a * classes), f % (a * classes)
        mem[ch * h * w + pos] = 1.0 + (j % 3)
    assert int((R.sigmoid_cr(m) > THRESH).sum()) == 7
    for k in (6, 7, 8, 1000):
        want = _check([m], classes, k, what="exactly 7 passing")
        assert int((want >= 0).sum()) == min(k, 7) and want.shape[1] == min(k, a * classes * h * w)
    assert F.retinanet_topk([m.cuda()], classes, 8, THRESH).cpu()[0].tolist() == [100, 300, 17, 250, 5, 101, 377, -1]


# ---- decode ---------------------------------------------------------------------------------------------------------------------------
PADDED, SIZES = (104, 136), [(104, 136), (97, 120)]
STRIDES = [(PADDED[0] // h, PADDED[1] // w) for h, w in FIVE]
ANCHOR_SIZES = ((8, 10, 13), (16, 20, 25), (32, 40, 50), (64, 80, 101), (128, 161, 203))


def _anchorgen():
    return P.AnchorGenerator(ANCHOR_SIZES, ((0.5, 1.0, 2.0),) * 5)


def _decode_inputs(seed, a=9, classes=5):
    g = torch.Generator().manual_seed(seed)
    cl = [torch.randn((2, a * classes, h, w), generator=g) * 3 for h, w in FIVE]
    dl = [torch.randn((2, 4 * a, h, w), generator=g) for h, w in FIVE]
    clip32 = torch.tensor(CLIP, dtype=torch.float32)
    for d in dl[:3]:
        f = d.view(2, a, 4, -1)  # (image, anchor, coordinate, position)
        f[0, 0, 2, 1] = 9.0                                           # dw above the clip
        f[0, 1, 3, 2] = clip32                                        # dh = clip exactly
        f[1, 2, 2, 0] = torch.nextafter(clip32, torch.tensor(9.0))    # and the float above it
        f[0, 2, 0, 3], f[1, 0, 3, 1], f[1, 1, 1, 2] = float("nan"), float("nan"), float("nan")
        f[0, 0, 0, 4], f[0, 1, 2, 4], f[1, 0, 3, 3] = float("inf"), float("inf"), float("-inf")
        f[1, 2, 1, 4], f[0, 2, 2, 0] = float("-inf"), float("-inf")
    return cl, dl


def test_decode_equals_the_restatement():
    a, classes = 9, 5
    cl, dl = _decode_inputs(9400)
    ag = _anchorgen()
    images = P.ImageList(torch.zeros(2, 3, *PADDED), SIZES)
    anchors = ag(images, cl)
    total = anchors[0].shape[0]
    dcl, ddl = [m.cuda() for m in cl], [m.cuda() for m in dl]
    sel = F.retinanet_topk(dcl, classes, 1000, THRESH)
    assert torch.equal(sel.cpu(), R.select(cl, classes, 1000, THRESH))
    hand = torch.tensor([[-1, total * classes, 2 ** 31 - 1, 0, total * classes - 1, 7, -5, 12345],
                         [3, -1, total * classes + 1, 2 ** 30, 44, total * classes - 2, 1, -2 ** 31]], dtype=torch.int32)
    idx = torch.cat([sel.cpu(), hand], 1)
    boxes, scores, labels, valid = F.retinanet_decode(dcl, ddl, idx.cuda(), ag.cell_anchors, STRIDES, SIZES, classes, (1.0, 1.0, 1.0, 1.0), CLIP)
    assert _lib.last_kernel() == "k_retinanet_decode<levels5>"
    wb, wsc, wl, wv = R.decode(cl, dl, idx, anchors, SIZES, classes)
    P.same(boxes, wb, "boxes"), P.same(scores, wsc, "scores")
    assert labels.dtype == torch.int64 and torch.equal(labels.cpu(), wl)
    assert valid.dtype == torch.bool and torch.equal(valid.cpu(), wv)
    # what the comparison covers
    ok = (idx >= 0) & (idx.long() < total * classes)
    assert torch.equal(wv, ok) and hand.shape[1] - int(ok[0, -8:].sum()) == 4
    assert float(wb[~ok].abs().max()) == 0 and float(wsc[~ok].abs().max()) == 0 and int(wl[~ok].abs().max()) == 0
    assert torch.equal(wl[ok], idx[ok].long() % classes)
    assert bool(torch.isnan(wb).any())
    for i, (ih, iw) in enumerate(SIZES):  # boxes clipped at both borders of both images
        b = wb[i][ok[i]]
        assert bool((b[:, 0] == 0).any()) and bool((b[:, 1] == 0).any()) and bool((b[:, 2] == iw).any()) and bool((b[:, 3] == ih).any())
    # other weights and clip
    w2 = (10.0, 10.0, 5.0, 5.0)
    got = F.retinanet_decode(dcl, ddl, sel, ag.cell_anchors, STRIDES, SIZES, classes, w2, 2.0)
    want = R.decode(cl, dl, sel.cpu(), anchors, SIZES, classes, w2, 2.0)
    P.same(got[0], want[0], "boxes, weights (10, 10, 5, 5)"), P.same(got[1], want[1])


def test_decode_anchor_and_label_follow_the_flat_index():
    """Zero deltas: decode_single is the identity on integer anchors, so box j is anchor idx // K clipped; label idx % K."""
    a, classes = 9, 5
    cl, _ = _decode_inputs(9401)
    dl = [torch.zeros(2, 4 * a, h, w) for h, w in FIVE]
    ag = _anchorgen()
    anchors = ag(P.ImageList(torch.zeros(2, 3, *PADDED), SIZES), cl)
    dcl = [m.cuda() for m in cl]
    idx = F.retinanet_topk(dcl, classes, 300, 0.5)
    big = [(4096, 4096), (4096, 4096)]
    boxes, scores, labels, valid = F.retinanet_decode(dcl, [d.cuda() for d in dl], idx, ag.cell_anchors, STRIDES, big, classes)
    flat_cls = torch.cat([R.permute_level(m, classes) for m in cl], 1)
    for i in range(2):
        f = idx[i].cpu().long()
        v = f >= 0
        assert torch.equal(valid[i].cpu(), v) and bool(v.any()) and bool((~v).any())
        assert torch.equal(boxes[i].cpu()[v], P.clip_boxes_to_image(anchors[i][f[v] // classes], big[i]))
        assert torch.equal(labels[i].cpu()[v], f[v] % classes)
        P.same(scores[i].cpu()[v], R.sigmoid_cr(flat_cls[i][f[v] // classes, f[v] % classes]))


# ---- the head -------------------------------------------------------------------------------------------------------------------------
HEAD_GRIDS = ((16, 20), (8, 10), (4, 5), (2, 3), (1, 2))  # a 128 x 160 batch at strides 8 .. 128


def _randomize(module, seed, std=0.03):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * std)


def _counting(call, launches, names=("conv2d_bias_relu", "retinanet_topk", "retinanet_decode")):
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


def test_head_equals_the_oracle_composition_and_two_separate_first_layers():
    """RetinaNetHead(256, 9, 5) on the five levels of a 128 x 160 batch of two.  Every level's maps equal, bit for bit, the CPU
    oracle composition in the summation order the library states, and the layer-by-layer composition of F.conv2d_bias_relu with the
    two towers' first layers as two SEPARATE launches."""
    head = mv.RetinaNetHead(256, 9, 5)
    _randomize(head, 9500)
    xs = [philox_f32(9510 + i, (2, 256, h, w)) * 2 - 1 for i, (h, w) in enumerate(HEAD_GRIDS)]
    head = head.cuda()
    dxs = [torch.from_numpy(x).cuda() for x in xs]
    launches = []
    out = _counting(lambda: head(dxs), launches)
    joint = [head.joint_sums_alike(x) for x in dxs]
    assert launches == ["conv2d_bias_relu"] * sum(9 if j else 10 for j in joint), launches
    assert any(joint), "no level takes the joint first layer"
    ch, rh = head.classification_head, head.regression_head
    for l, x in enumerate(dxs):
        for tower, last, got in ((ch.conv, ch.cls_logits, out["cls_logits"][l]), (rh.conv, rh.bbox_reg, out["bbox_regression"][l])):
            t = x
            for block in tower:
                t = F.conv2d_bias_relu(t, block[0].weight, block[0].bias, relu=True)
            want = F.conv2d_bias_relu(t, last.weight, last.bias, relu=False)
            assert tuple(got.shape) == (2, last.out_channels) + HEAD_GRIDS[l]
            assert torch.equal(got.detach(), want.detach()), f"level {l}: joint {joint[l]}"
            assert float(got.detach().abs().max()) > 1e-3
    for l in range(5):
        for tower, last, got in ((ch.conv, ch.cls_logits, out["cls_logits"][l]), (rh.conv, rh.bbox_reg, out["bbox_regression"][l])):
            t = xs[l]
            for block in tower:
                t = oracle_conv3x3(ref, t, block[0].weight.detach().cpu().numpy(), block[0].bias.detach().cpu().numpy(), relu=True)
            want = oracle_conv3x3(ref, t, last.weight.detach().cpu().numpy(), last.bias.detach().cpu().numpy(), relu=False)
            np.testing.assert_array_equal(got.detach().cpu().numpy(), want)
    # the reference's layout for anyone who asks
    cat = mv.retinanet.concat_layout(out["cls_logits"], 5)
    assert tuple(cat.shape) == (2, 9 * sum(h * w for h, w in HEAD_GRIDS), 5)
    assert cat[1, (3 * 20 + 4) * 9 + 7, 2] == out["cls_logits"][0][1, 7 * 5 + 2, 3, 4]


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
def test_retinanet_end_to_end_stage_by_stage():
    """resnet18 FPN on layer2 .. layer4 + P6 / P7, 5 classes, two images; every stage's reference is fed the library's own output of
    the stage before.  cls_logits is re-initialised with a wider weight (std 0.02) and a bias of -2.2 so that detections exist (the shipped
    bias -log 99 with std 0.01 puts every score near 0.01, below the threshold)."""
    torch.manual_seed(9600)
    replica_bb = PF.resnet_fpn_backbone(backbone_name="resnet18", returned_layers=[2, 3, 4], extra_blocks=PF.LastLevelP6P7(256, 256)).eval()
    PF.randomize(replica_bb, 9601)
    backbone = mv.resnet_fpn_backbone(backbone_name="resnet18", returned_layers=[2, 3, 4], extra_blocks=mv.LastLevelP6P7(256, 256))
    backbone.load_state_dict(replica_bb.state_dict(), strict=True)
    model = mv.RetinaNet(backbone, 5, topk_candidates=100, _skip_resize=True)
    _randomize(model.head, 9602, 0.02)
    g = torch.Generator().manual_seed(9603)
    with torch.no_grad():
        c = model.head.classification_head.cls_logits
        c.weight.copy_(torch.randn(c.weight.shape, generator=g) * 0.02)
        c.bias.fill_(-2.2)
    model = model.cuda()
    imgs = [torch.from_numpy(philox_f32(9604, (3, 128, 160))), torch.from_numpy(philox_f32(9605, (3, 120, 150)))]
    dimgs = [i.cuda() for i in imgs]

    # ImageList
    images, _ = model.transform(dimgs, None)
    ref_images = R.Transform(model.transform.image_mean, model.transform.image_std)(imgs)
    assert images.image_sizes == ref_images.image_sizes == [(128, 160), (120, 150)] and tuple(images.tensors.shape) == (2, 3, 128, 160)
    np.testing.assert_allclose(images.tensors.cpu().numpy(), ref_images.tensors.numpy(), rtol=0, atol=4e-7 * 3)
    # features: five levels at strides 8 .. 128, close to the replica's float32 forward
    feats = model.backbone(images.tensors)
    assert list(feats) == ["0", "1", "2", "p6", "p7"] and [tuple(f.shape[2:]) for f in feats.values()] == list(HEAD_GRIDS)
    with torch.no_grad():
        ref_feats = replica_bb(images.tensors.cpu())
    for name in feats:
        scale = float(ref_feats[name].abs().max())
        assert float((feats[name].detach().cpu() - ref_feats[name]).abs().max()) <= 1e-3 * scale, name
    # head maps
    launches = []
    head_out = _counting(lambda: model.head(list(feats.values())), launches)
    cl, dl = [m.detach().cpu() for m in head_out["cls_logits"]], [m.detach().cpu() for m in head_out["bbox_regression"]]
    assert [tuple(m.shape) for m in cl] == [(2, 45) + s for s in HEAD_GRIDS] and [tuple(m.shape) for m in dl] == [(2, 36) + s for s in HEAD_GRIDS]
    # idx and the decoded candidates, bit for bit
    launches.clear()
    idx, boxes, scores, labels, valid = _counting(lambda: model.candidates(head_out, images.tensors.shape[-2:], images.image_sizes), launches)
    assert launches == ["retinanet_topk", "retinanet_decode"]
    want_idx = R.select(cl, 5, 100, 0.05)
    assert torch.equal(idx.cpu(), want_idx)
    ag = R.default_anchorgen()
    anchors = ag(P.ImageList(images.tensors.cpu(), images.image_sizes), cl)
    wb, wsc, wl, wv = R.decode(cl, dl, want_idx, anchors, images.image_sizes, 5)
    P.same(boxes, wb, "boxes"), P.same(scores, wsc, "scores")
    assert torch.equal(labels.cpu(), wl) and torch.equal(valid.cpu(), wv)
    # nms and the rescaled boxes: the restatement's RetinaNet on the library's head maps
    want = R.RetinaNet(replica_bb, 5, topk_candidates=100,
                       numerics=P.RESTATEMENT).eval().from_head_maps(P.ImageList(images.tensors.cpu(), images.image_sizes), cl, dl)
    got = model(dimgs)
    for i in range(2):
        n = len(want[i]["boxes"])
        print(f"image {i}: {n} detections, classes {sorted(set(want[i]['labels'].tolist()))}, {int(wv[i].sum())} candidates")
        assert 10 <= n < model.detections_per_img == 300 and len(set(want[i]["labels"].tolist())) >= 2, "the comparison shows nothing"
        P.same(got[i]["boxes"], want[i]["boxes"], f"boxes of image {i}")
        P.same(got[i]["scores"], want[i]["scores"], f"scores of image {i}")
        assert torch.equal(got[i]["labels"].cpu(), want[i]["labels"])


# ---- image stride past 2^31 -----------------------------------------------------------------------------------------------------------
def test_image_stride_past_2_to_31_elements():
    """n = 2 images 2^31 + 64 elements apart in one allocation of about 8 GiB, of which only the two maps are written: image 1's
    result equals the same map run alone, so the map offsets are 64-bit."""
    a, classes, h, w = 3, 2, 5, 7
    stride = 2 ** 31 + 64
    numel = a * classes * h * w
    g = torch.Generator().manual_seed(9700)
    m = torch.randn((2, a * classes, h, w), generator=g) * 3
    d = torch.randn((2, 4 * a, h, w), generator=g)
    try:
        big = torch.empty(stride + numel, dtype=torch.float32, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.fail("8 GiB of device memory are not available")
    big[:numel] = m[0].flatten().cuda()
    big[stride:stride + numel] = m[1].flatten().cuda()
    view = torch.as_strided(big, (2, a * classes, h, w), (stride, h * w, w, 1))
    idx = F.retinanet_topk([view], classes, 50, THRESH)
    alone = F.retinanet_topk([m[1:].cuda()], classes, 50, THRESH)
    assert torch.equal(idx[1], alone[0]) and torch.equal(idx.cpu(), R.select([m], classes, 50, THRESH))
    cell = [torch.tensor([[-8.0, -8, 8, 8], [-4, -8, 4, 8], [-8, -4, 8, 4]])]
    got = F.retinanet_decode([view], [d.cuda()], idx, cell, [(8, 8)], [(40, 56), (33, 50)], classes)
    want = F.retinanet_decode([m[1:].cuda()], [d[1:].cuda()], alone, cell, [(8, 8)], [(33, 50)], classes)
    for gt, wt in zip(got, want):
        P.same(gt[1], wt[0])
    del big, view
    torch.cuda.empty_cache()
