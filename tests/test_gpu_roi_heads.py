"""RoIHeads and Faster R-CNN on the GPU (`-m gpu`): F.roi_detections (csrc/roi_heads.hip), TwoMLPHead, FastRCNNPredictor,
RoIHeads.forward and FasterRCNN.forward.  The detections are compared bit for bit (NaN in equal places, == elsewhere) with the
restatement (b) of tests/_roi_heads_ref.py on the CPU, the linear layers with the CPU oracle in the summation order the library states."""
import functools
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
from tests import _roi_heads_ref as H  # noqa: E402
from tests import _rpn_ref as P  # noqa: E402
from tests._util import philox_f32  # noqa: E402

CLIP = math.log(1000.0 / 16)
SIZES = [(64, 96), (61, 90)]
NAN, INF = float("nan"), float("inf")


# ---- F.roi_detections -------------------------------------------------------------------------------------------------------------------
def detection_case(r, c, seed=0):
    """class_logits (r, c), box_regression (r, 4 c), proposals of the two images of SIZES.  Row i of the logits follows pattern
    (i + c) % 8: N(0, 3^2) | all equal | one class at +80 over the rest near -25 (E underflows to 0 and to denormals) | +-0 | a NaN |
    a +inf | all -inf | N(0, 3^2).  The deltas hold NaN, +-inf and codes beyond the clip; the rois lie inside, across and outside
    the images and on the clip boundary."""
    g = torch.Generator().manual_seed(8700 + 1000 * seed + 7 * r + c)
    logits = torch.randn((r, c), generator=g) * 3
    for i in range(r):
        kind = (i + c) % 8
        if kind == 1:
            logits[i] = 0.75
        elif kind == 2:
            logits[i] = torch.randn(c, generator=g) * 3 - 25
            logits[i, (i * 5 + 1) % c] = 80.0
        elif kind == 3:
            logits[i] = torch.tensor([0.0, -0.0])[torch.randint(0, 2, (c,), generator=g)]
        elif kind == 4:
            logits[i, (i * 3) % c] = NAN
        elif kind == 5:
            logits[i, (i * 3 + 1) % c] = INF
        elif kind == 6:
            logits[i] = -INF
    deltas = torch.randn((r, 4 * c), generator=g) * 2
    u = torch.rand((r, 4 * c), generator=g)
    deltas[u < 0.02] = NAN
    deltas[(u >= 0.02) & (u < 0.03)] = INF
    deltas[(u >= 0.03) & (u < 0.04)] = -INF
    deltas[(u >= 0.04) & (u < 0.08)] = 30.0   # / 5 beyond the clip
    deltas[(u >= 0.08) & (u < 0.10)] = 100.0  # / 1 and / 5 beyond the clip
    p = torch.rand((r, 2), generator=g) * torch.tensor([110.0, 80.0]) - 12
    boxes = torch.cat([p, p + 2 + torch.rand((r, 2), generator=g) * 50], 1)
    split = (r + 1) // 2
    for i in range(r):
        h, w = SIZES[0] if i < split else SIZES[1]
        if i % 7 == 3:
            boxes[i, 2], boxes[i, 3] = float(w), float(h)      # on the clip boundary
        if i % 11 == 5:
            boxes[i] = torch.tensor([w + 3.0, h + 2.0, w + 30.0, h + 40.0])  # outside the image
    return logits, deltas, [boxes[:split], boxes[split:]]


@functools.lru_cache(maxsize=None)
def detection_want(r, c, weights, score_thresh, min_size):
    logits, deltas, proposals = detection_case(r, c)
    heads = H.RoIHeads(None, None, None, 0.5, 0.5, 512, 0.25, weights, score_thresh, 0.5, 100, numerics=H.RESTATEMENT)
    return heads.dense(logits, deltas, proposals, SIZES, min_size)


def _rois(proposals):
    return torch.cat([torch.cat([torch.full_like(b[:, :1], float(i)), b], 1) for i, b in enumerate(proposals)])


def _check(got, want, what):
    for name, g, w in zip(("boxes", "scores", "labels", "valid"), got, want):
        P.same(g, w, f"{what} {name}")


@pytest.mark.parametrize("weights", [(10.0, 10.0, 5.0, 5.0), (1.0, 1.0, 1.0, 1.0)], ids=["w10-5", "w1"])
@pytest.mark.parametrize("r", [1, 63, 257])
@pytest.mark.parametrize("c", [2, 3, 64, 65, 91, 129, 257])
def test_roi_detections_equals_the_restatement(c, r, weights):
    logits, deltas, proposals = detection_case(r, c)
    want = detection_want(r, c, weights, 0.05, 1e-2)
    rois = _rois(proposals).cuda()
    # contiguous inputs
    got = F.roi_detections(logits.cuda(), deltas.cuda(), rois, SIZES, weights, CLIP, 0.05, 1e-2)
    assert _lib.last_kernel() == f"k_roi_detections<classes{c}>"
    assert got[0].shape == (r, c - 1, 4) and got[2].dtype == torch.int64 and got[3].dtype == torch.bool
    _check(got, want, f"contiguous r={r} c={c}")
    # the two as column slices of one (r, 5 c) tensor, as FastRCNNPredictor returns them: no copy, the same results
    both = torch.cat([logits, deltas], 1).cuda()
    sliced = F.roi_detections(both[:, :c], both[:, c:], rois, torch.tensor(SIZES, dtype=torch.float32).cuda(), weights, CLIP, 0.05, 1e-2)
    _check(sliced, want, f"sliced r={r} c={c}")
    for g, s in zip(got, sliced):
        P.same(s, g.cpu())
    if r > 1:
        assert bool(want[3].any()) and not bool(want[3].all()) and bool(torch.isnan(want[1]).any())


def test_roi_detections_at_the_thresholds():
    """C = 2 and equal logits: the score is 0.5 exactly, and the test is strict.  Zero deltas return the roi; a roi from x1 = 95.5
    across the right edge of a 96-wide image is clipped to a side of exactly 0.5, and the size test is not strict."""
    logits = torch.tensor([[1.25, 1.25], [0.0, -0.0], [3.0, 3.0]])
    deltas = torch.zeros(3, 8)
    proposals = [torch.tensor([[4.0, 4.0, 20.0, 30.0], [95.5, 2.0, 200.0, 8.0], [10.0, 63.5, 30.0, 90.0]])]
    rois = _rois(proposals).cuda()
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    for thresh, min_size, valid in ((0.5, 1e-2, [0, 0, 0]), (below, 1e-2, [1, 1, 1]), (below, 0.5, [1, 1, 1]), (below, above, [1, 0, 0]),
                                    (0.05, 0.5, [1, 1, 1])):
        heads = H.RoIHeads(None, None, None, 0.5, 0.5, 512, 0.25, None, thresh, 0.5, 100, numerics=H.RESTATEMENT)
        want = heads.dense(logits, deltas, proposals, SIZES[:1], min_size)
        assert want[3].reshape(-1).tolist() == [bool(v) for v in valid], (thresh, min_size)
        got = F.roi_detections(logits.cuda(), deltas.cuda(), rois, SIZES[:1], (10.0, 10.0, 5.0, 5.0), CLIP, thresh, min_size)
        _check(got, want, f"thresh={thresh} min_size={min_size}")
    assert bool((want[1] == 0.5).all())
    assert want[0][1, 0].tolist() == [95.5, 2.0, 96.0, 8.0] and want[0][2, 0].tolist() == [10.0, 63.5, 30.0, 64.0]


def test_roi_detections_image_index_outside_the_batch_gives_zeros():
    r, c = 63, 5
    logits, deltas, proposals = detection_case(r, c, seed=1)
    want = [w.clone() for w in H.RoIHeads(None, None, None, 0.5, 0.5, 512, 0.25, None, 0.05, 0.5, 100, numerics=H.RESTATEMENT)
            .dense(logits, deltas, proposals, SIZES)]
    rois = _rois(proposals)
    bad = {4: 2.0, 9: -1.0, 40: 2.0, 41: -1.0, 62: 1e9, 17: NAN}
    for i, v in bad.items():
        rois[i, 0] = v
        for w in want:
            w[i] = 0
    got = F.roi_detections(logits.cuda(), deltas.cuda(), rois.cuda(), SIZES)
    _check(got, want, "bad image index")
    assert bool(want[3].any())
    empty = F.roi_detections(torch.zeros((0, c), device="cuda"), torch.zeros((0, 4 * c), device="cuda"), torch.zeros((0, 5), device="cuda"), SIZES)
    assert empty[0].shape == (0, c - 1, 4) and empty[1].shape == (0, c - 1) and empty[3].dtype == torch.bool


def test_roi_detections_softmax_is_as_close_to_float64_as_the_reference():
    """The yardstick of DESIGN 3.24: against the float64 softmax the kernel may be at most twice as far as torch's own float32."""
    g = torch.Generator().manual_seed(8790)
    r, c = 257, 91
    logits = torch.randn((r, c), generator=g) * 3
    deltas = torch.zeros(r, 4 * c)
    proposals = [torch.tensor([[4.0, 4.0, 20.0, 30.0]]).repeat(r, 1)]
    exact = torch.softmax(logits.double(), -1)[:, 1:]
    replica = torch.softmax(logits, -1)[:, 1:].double()
    got = F.roi_detections(logits.cuda(), deltas.cuda(), _rois(proposals).cuda(), SIZES[:1])[1].cpu().double()
    err, ref_err = float((got - exact).abs().max()), float((replica - exact).abs().max())
    print(f"max |kernel - float64| = {err:.3e}, max |torch float32 - float64| = {ref_err:.3e}")
    assert err <= 2 * ref_err


def test_roi_detections_rows_more_than_2_31_elements_apart():
    """The row strides are 64-bit: three rows of one (3, 5 C) view whose rows start 2^31 + 8 elements apart (an uninitialised 17 GB
    buffer of which 15 C floats are written), so the second row lies past element 2^31 and byte 2^32, the third past element 2^32."""
    c, stride = 5, 2 ** 31 + 8
    logits, deltas, proposals = detection_case(3, c, seed=2)
    logits[1] = torch.tensor([0.5, 2.0, -1.0, 0.25, 1.5])  # rows 0 and 2 follow detection_case's patterns, this one is finite
    want = H.RoIHeads(None, None, None, 0.5, 0.5, 512, 0.25, None, 0.05, 0.5, 100, numerics=H.RESTATEMENT).dense(logits, deltas, proposals, SIZES)
    buf = torch.empty(2 * stride + 5 * c, dtype=torch.float32, device="cuda")
    both = torch.as_strided(buf, (3, 5 * c), (stride, 1))
    both.copy_(torch.cat([logits, deltas], 1))
    assert both[2, 0].data_ptr() - buf.data_ptr() == 8 * stride > 2 ** 34
    got = F.roi_detections(both[:, :c], both[:, c:], _rois(proposals).cuda(), SIZES)
    _check(got, want, "rows 2^31 + 8 elements apart")
    assert bool(want[3][1].any())


# ---- the box head and the predictor ---------------------------------------------------------------------------------------------------------
def _counting(call, launches, names=("linear_bias_relu", "roi_detections", "conv_norm_act", "conv2d_bias_relu", "rpn_topk", "rpn_decode")):
    """call(), recording the library calls made through the functional layer (tests/test_gpu_rpn.py::_counting)."""
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


def _oracle_linear(x, w, b, relu):
    n, k, m = x.shape[0], x.shape[1], w.shape[0]
    slices, slice_len = F.linear_k_slices(n, k, m)
    return ref.linear_bias_relu(x, w, b, relu=relu, slice_len=slice_len if slices > 1 else 0)


def _randomize(module, seed, std):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * std)


def oracle_predictor(pred, x):
    """(scores, bbox_deltas) of a CPU-resident FastRCNNPredictor on a numpy (R, K): ONE linear over the concatenated weight."""
    w = torch.cat([pred.cls_score.weight, pred.bbox_pred.weight]).detach().numpy()
    b = torch.cat([pred.cls_score.bias, pred.bbox_pred.bias]).detach().numpy()
    both = _oracle_linear(x, w, b, False)
    c = pred.cls_score.out_features
    return both[:, :c], both[:, c:]


def oracle_head(head, x):
    t = _oracle_linear(np.ascontiguousarray(x.reshape(x.shape[0], -1)), head.fc6.weight.detach().numpy(), head.fc6.bias.detach().numpy(), True)
    return _oracle_linear(t, head.fc7.weight.detach().numpy(), head.fc7.bias.detach().numpy(), True)


def test_predictor_equals_the_oracle_composition_in_one_launch():
    r, k, c = 37, 1024, 5
    pred = mv.FastRCNNPredictor(k, c)
    _randomize(pred, 8800, 0.05)
    x = philox_f32(8801, (r, k)) * 2 - 1
    want_scores, want_deltas = oracle_predictor(pred, x)
    pred = pred.cuda()
    launches = []
    scores, deltas = _counting(lambda: pred(torch.from_numpy(x).cuda()), launches)
    assert launches == ["linear_bias_relu"]
    assert tuple(scores.shape) == (r, c) and tuple(deltas.shape) == (r, 4 * c) and scores.stride(0) == 5 * c and deltas.stride(0) == 5 * c
    assert scores.untyped_storage().data_ptr() == deltas.untyped_storage().data_ptr(), "the two outputs are views of one tensor"
    np.testing.assert_array_equal(scores.detach().cpu().numpy(), want_scores)
    np.testing.assert_array_equal(deltas.detach().cpu().numpy(), want_deltas)
    assert np.abs(want_scores).max() > 1e-2
    four_d = pred(torch.from_numpy(x).cuda().reshape(r, k, 1, 1))  # the reference's flatten
    np.testing.assert_array_equal(four_d[0].detach().cpu().numpy(), want_scores)


def test_two_mlp_head_equals_the_oracle_composition():
    head = mv.TwoMLPHead(256 * 7 * 7, 1024)
    _randomize(head, 8810, 0.02)
    x = philox_f32(8811, (37, 256, 7, 7)) * 2 - 1
    want = oracle_head(head, x)
    head = head.cuda()
    launches = []
    got = _counting(lambda: head(torch.from_numpy(x).cuda()), launches)
    assert launches == ["linear_bias_relu"] * 2
    np.testing.assert_array_equal(got.detach().cpu().numpy(), want)
    assert (want > 0).mean() > 0.1 and (want == 0).mean() > 0.1


# ---- RoIHeads.forward and FasterRCNN.forward, stage by stage ----------------------------------------------------------------------------------
WHOLE_SEED = 0
MODEL_KW = dict(num_classes=5, rpn_pre_nms_top_n_test=200, rpn_post_nms_top_n_test=50, box_score_thresh=0.05, box_detections_per_img=20,
                _skip_resize=True)


def whole_setup(seed=WHOLE_SEED):
    """(library model, replica model in the restatement's numerics, images), on the CPU with equal parameters."""
    torch.manual_seed(8900 + seed)
    replica = H.FasterRCNN(PF.resnet_fpn_backbone(backbone_name="resnet18"), numerics=H.RESTATEMENT, **MODEL_KW).eval()
    PF.randomize(replica.backbone, 8901 + seed)
    _randomize(replica.rpn.head, 8902 + seed, 0.03)
    _randomize(replica.roi_heads.box_head, 8903 + seed, 0.02)
    _randomize(replica.roi_heads.box_predictor, 8904 + seed, 0.04)  # 0.1 saturates the scores near 1
    model = mv.FasterRCNN(mv.resnet_fpn_backbone(backbone_name="resnet18"), **MODEL_KW)
    model.load_state_dict(replica.state_dict(), strict=True)
    images = [torch.from_numpy(philox_f32(8905 + seed, (3, 128, 160))), torch.from_numpy(philox_f32(8906 + seed, (3, 120, 150)))]
    return model, replica, images


@torch.no_grad()
def test_faster_rcnn_stage_by_stage():
    """Each stage's reference takes the library's own output of the stage before, so that a last-bit difference upstream cannot
    cascade: images -> ImageList, proposals, pooled features, box head, predictor, detections, the boxes rescaled."""
    model, replica, images = whole_setup()
    model = model.cuda()
    dev_images = [im.cuda() for im in images]
    # images -> ImageList
    il, _ = model.transform(dev_images)
    want_il, _ = replica.transform(images)
    assert isinstance(il, mv.ImageList) and [tuple(s) for s in il.image_sizes] == [tuple(s) for s in want_il.image_sizes] == [(128, 160), (120, 150)]
    P.same(il.tensors, want_il.tensors, "ImageList.tensors")
    assert tuple(il.tensors.shape) == (2, 3, 128, 160)
    # backbone and rpn head: the library's; proposals against the restatement on the head's outputs
    feats = model.backbone(il.tensors)
    objectness, deltas = model.rpn.head(list(feats.values()))
    proposals, _ = model.rpn(il, feats)
    ref_il = P.ImageList(il.tensors.cpu(), il.image_sizes)
    want_props, _ = replica.rpn.from_head_outputs(ref_il, [o.cpu().contiguous() for o in objectness], [d.cpu().contiguous() for d in deltas])
    for i in range(2):
        assert 0 < len(want_props[i]) <= 50
        P.same(proposals[i], want_props[i], f"proposals of image {i}")
    # pooled features
    heads = model.roi_heads
    cpu_feats = {k: v.cpu() for k, v in feats.items()}
    cpu_props = [p.cpu() for p in proposals]
    pooled = heads.box_roi_pool(feats, proposals, il.image_sizes)
    want_pooled = replica.roi_heads.box_roi_pool(cpu_feats, cpu_props, il.image_sizes)
    assert tuple(pooled.shape) == (sum(len(p) for p in proposals), 256, 7, 7)
    P.same(pooled, want_pooled, "pooled features")
    # box head, predictor
    hidden = heads.box_head(pooled)
    np.testing.assert_array_equal(hidden.detach().cpu().numpy(), oracle_head(replica.roi_heads.box_head, pooled.detach().cpu().numpy()))
    class_logits, box_regression = heads.box_predictor(hidden)
    want_logits, want_reg = oracle_predictor(replica.roi_heads.box_predictor, hidden.detach().cpu().numpy())
    np.testing.assert_array_equal(class_logits.detach().cpu().numpy(), want_logits)
    np.testing.assert_array_equal(box_regression.detach().cpu().numpy(), want_reg)
    # detections: the restatement's postprocess_detections on the library's logits, deltas and proposals
    launches = []
    boxes, scores, labels = _counting(lambda: heads.postprocess_detections(class_logits, box_regression, proposals, il.image_sizes), launches)
    assert launches == ["roi_detections"]
    want = replica.roi_heads.postprocess_detections(class_logits.cpu().contiguous(), box_regression.cpu().contiguous(), cpu_props, il.image_sizes)
    seen = set()
    for i in range(2):
        assert 0 < len(want[0][i]) <= 20, "every image returns detections"
        P.same(boxes[i], want[0][i], f"detection boxes of image {i}")
        P.same(scores[i], want[1][i], f"detection scores of image {i}")
        P.same(labels[i], want[2][i], f"detection labels of image {i}")
        seen |= set(want[2][i].tolist())
    assert len(seen) > 1 and 0 not in seen, "the detections are not all in one class"
    # RoIHeads.forward: pooler, head, predictor, detections in that order, and nothing else
    launches = []
    result, losses = _counting(lambda: heads(feats, proposals, il.image_sizes), launches)
    assert launches == ["linear_bias_relu"] * 3 + ["roi_detections"] and losses == {}
    for i in range(2):
        assert list(result[i]) == ["boxes", "labels", "scores"]
        P.same(result[i]["boxes"], want[0][i]), P.same(result[i]["scores"], want[1][i]), P.same(result[i]["labels"], want[2][i])
    # the whole model: the same detections, the boxes through transform.postprocess (here the identity scale, still computed)
    out = model(dev_images)
    want_out = replica.transform.postprocess([{"boxes": b, "labels": lab, "scores": s} for b, s, lab in zip(*want)], il.image_sizes,
                                             [(128, 160), (120, 150)])
    assert len(out) == 2
    for got, w in zip(out, want_out):
        P.same(got["boxes"], w["boxes"]), P.same(got["scores"], w["scores"]), P.same(got["labels"], w["labels"])
        assert got["labels"].dtype == torch.int64 and got["boxes"].is_cuda
    # rescaling to other original sizes is the reference's float32 composition
    rescaled = model.transform.postprocess([{"boxes": b.clone()} for b in boxes], il.image_sizes, [(256, 200), (77, 150)])
    want_rescaled = replica.transform.postprocess([{"boxes": b.clone()} for b in want[0]], il.image_sizes, [(256, 200), (77, 150)])
    for got, w in zip(rescaled, want_rescaled):
        P.same(got["boxes"], w["boxes"])
