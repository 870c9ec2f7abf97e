"""The mask branch of Mask R-CNN without a GPU: the two references of tests/_mask_ref.py against each other (the integer boxes bit for
bit, the pasted values within the bound of DESIGN.md 3.27 and bit for bit where torch vectorises), the pixel-shuffled oracle of the
transposed conv against torch, MaskRCNNHeads / MaskRCNNPredictor / MaskRCNN / maskrcnn_resnet50_fpn against the replica (state,
version-1 keys, initialisation, argument errors), every refusal of the three C entries with host pointers (refusals come before any
launch and write nothing) and the Python-side checks, which fire before a device is needed."""
import numpy as np
import pytest
import torch

import cpu_vision_amd as mv
from cpu_vision_amd import _lib, mask_rcnn
from cpu_vision_amd import functional as F
from tests import _fpn_ref as FP
from tests import _mask_ref as M
from tests import _roi_heads_ref as H

INVALID, UNSUPPORTED = -1, -2
SENT = -7.25


# ---- the restatement against the replica ---------------------------------------------------------------------------------------------------
def test_scale_is_the_float32_of_the_double_quotient():
    assert float(np.float32(float(28 + 2) / 28)) == 1.0714285373687744


@pytest.mark.parametrize("m,padding", [(28, 1), (14, 1), (1, 1), (28, 0), (7, 3)])
def test_integer_boxes_equal_the_replicas_bit_for_bit(m, padding):
    """A few thousand seeded boxes: inside, negative, fractional, degenerate (zero size), inverted, and halves that truncate through
    negative fractions.  The replica multiplies a float32 tensor by the Python float `scale`; the restatement multiplies by
    float32(scale): equal integers pin that claim."""
    g = torch.Generator().manual_seed(9600 + m + padding)
    p = torch.rand((4000, 2), generator=g) * 300 - 60
    size = torch.rand((4000, 2), generator=g) * 200 - 20  # some inverted
    boxes = torch.cat([p, p + size], 1)
    boxes[::7] = boxes[::7].round()
    boxes[::11, 2:] = boxes[::11, :2]  # degenerate
    boxes[::13] = boxes[::13] * 0.01   # around zero: -0.x truncates to 0
    want = M.expand_boxes(boxes.clone(), float(m + 2 * padding) / m).to(dtype=torch.int64).numpy()
    got, ok = M.expanded_boxes(boxes.numpy(), m, padding)
    assert bool(ok.all())
    np.testing.assert_array_equal(got, want)
    assert (got < 0).any() and (got[:, 2] < got[:, 0]).any() and (got[:, 2] == got[:, 0]).any()
    lo = M.expand_boxes(boxes.clone(), float(m + 2 * padding) / m)
    assert bool(((lo > -1) & (lo < 0)).any()), "no coordinate truncates through a negative fraction"


def test_boxes_outside_the_domain_are_flagged():
    _, zero_plane = M.paste_boxes(37, 53)
    ints, ok = M.expanded_boxes(zero_plane, 28, 1)
    assert not ok.any() and not ints.any()
    edge = np.array([[0.0, 0.0, 2.0 ** 30 - 128, 4.0]], np.float32)  # expands past 2^30
    assert not M.expanded_boxes(edge, 28, 1)[1][0] and M.expanded_boxes(edge * np.float32(0.5), 28, 1)[1][0]


@pytest.mark.parametrize("m,padding", [(28, 1), (14, 1), (1, 1), (28, 0), (14, 0), (1, 0)])
@pytest.mark.parametrize("h,w", M.PASTE_IMAGES)
def test_paste_restatement_against_the_replica(h, w, m, padding):
    """Every roi of the paste tests that the reference accepts.  The non-zero supports are equal (the integer geometry), the values lie
    within (6 + 8 (M + 2 p)) 2^-24 max|x|, and they are bit-equal where torch's CPU interpolate vectorises: a resized mask of more than
    3 264 elements from a source of at least 14 x 14 (from a 3 x 3 source torch 2.10 was seen to take another loop above that size
    too, one ulp away, so those rois are held to the bound only)."""
    boxes, _ = M.paste_boxes(h, w)
    masks = M.paste_masks(9610 + m, len(boxes), m)
    want = M.paste_masks_in_image(masks, torch.from_numpy(boxes), (h, w), padding).numpy()
    got = M.paste(masks.numpy(), boxes, h, w, padding)
    assert got.shape == want.shape == (len(boxes), 1, h, w)
    ints, _ = M.expanded_boxes(boxes, m, padding)
    bound = M.paste_bound(m, padding, float(masks.max()))
    exact = 0
    for i, (bx0, by0, bx1, by1) in enumerate(ints.tolist()):
        inside = np.zeros((h, w), bool)
        inside[max(by0, 0):max(min(by1 + 1, h), 0), max(bx0, 0):max(min(bx1 + 1, w), 0)] = True
        assert not got[i, 0][~inside].any() and not want[i, 0][~inside].any(), f"roi {i} wrote outside its box"
        worst = float(np.abs(got[i].astype(np.float64) - want[i]).max())
        assert worst <= bound, (i, worst, bound)
        resized = max(bx1 - bx0 + 1, 1) * max(by1 - by0 + 1, 1)
        if resized > M.TORCH_VECTORISED_ABOVE and m + 2 * padding >= 14:
            np.testing.assert_array_equal(got[i].view(np.int32), want[i].view(np.int32), err_msg=f"roi {i}, {resized} elements")
            exact += 1
    assert (want != 0).any() and (want == 0).any()
    if m + 2 * padding >= 14:
        assert exact >= 1, "no roi of the case reaches torch's vectorised loop"


def test_paste_of_no_mask_and_padding_zero_identity():
    assert M.paste(np.zeros((0, 1, 28, 28), np.float32), np.zeros((0, 4), np.float32), 5, 7).shape == (0, 1, 5, 7)
    assert tuple(M.paste_masks_in_image(torch.zeros(0, 1, 28, 28), torch.zeros(0, 4), (5, 7)).shape) == (0, 1, 5, 7)
    # padding 0 and a box of the mask's own size: src == d on both axes, the paste is the mask
    mask = M.paste_masks(9620, 1, 14).numpy()
    out = M.paste(mask, np.array([[3.0, 2.0, 16.0, 15.0]], np.float32), 20, 24, padding=0)
    np.testing.assert_array_equal(out[0, 0, 2:16, 3:17], mask[0, 0])


def test_mask_probs_restatement_against_the_replica():
    g = torch.Generator().manual_seed(9630)
    logits = torch.randn((7, 5, 6, 6), generator=g) * 4
    labels = torch.tensor([0, 4, 1, 2, 3, 4, 0])
    want = torch.cat(M.maskrcnn_inference(logits, [labels[:3], labels[3:]]))
    got = M.mask_probs(logits, labels)
    assert got.shape == want.shape == (7, 1, 6, 6)
    # torch.sigmoid is within an ulp or two of the correctly rounded chain; the exponent of a probability is at most 0
    assert float((got - want).abs().max()) <= 4 * 2.0 ** -24
    assert not M.mask_probs(logits, torch.tensor([5, -1, 0, 0, 0, 0, 0]))[:2].any()


# ---- the oracle of the transposed conv against torch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cin,h,w,cout", [(3, 40, 7, 7, 5), (1, 3, 5, 9, 1), (2, 32, 14, 14, 24)])
@pytest.mark.parametrize("bias", [True, False])
def test_pixel_shuffled_oracle_equals_torch_conv_transpose2d(n, cin, h, w, cout, bias):
    g = torch.Generator().manual_seed(9640 + cin)
    x = torch.rand((n, cin, h, w), generator=g) * 2 - 1
    wt = torch.randn((cin, cout, 2, 2), generator=g) * 0.2
    b = torch.randn((cout,), generator=g) if bias else None
    want = torch.relu(torch.nn.functional.conv_transpose2d(x, wt, b, stride=2)).numpy()
    got = M.oracle_conv_transpose(x.numpy(), wt.numpy(), None if b is None else b.numpy(), "relu", slice_len=0)
    assert got.shape == want.shape == (n, cout, 2 * h, 2 * w)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()))
    assert (want > 0).any() and (want == 0).any()
    w4, b4 = M.relaid(wt.numpy(), None if b is None else b.numpy())
    lw4, lb4 = F.conv_transpose2x2_relayout(wt, b, torch.device("cpu"))
    np.testing.assert_array_equal(lw4.numpy(), w4)
    assert (b4 is None and lb4 is None) or np.array_equal(lb4.numpy(), b4)
    np.testing.assert_array_equal(w4[4 * (cout - 1) + 2 * 1 + 0], wt.numpy()[:, cout - 1, 1, 0])


# ---- structure: state, version-1 keys, initialisation --------------------------------------------------------------------------------------
def _same_state(ours, theirs, keys=None):
    sd, ref_sd = ours.state_dict(), theirs.state_dict()
    assert list(sd) == list(ref_sd)
    if keys is not None:
        assert list(sd) == keys
    for k in sd:
        assert sd[k].shape == ref_sd[k].shape and torch.equal(sd[k], ref_sd[k]), k
    ours.load_state_dict(ref_sd, strict=True)
    theirs.load_state_dict(sd, strict=True)


def _seeded(make_ours, make_theirs, seed):
    torch.manual_seed(seed)
    ours = make_ours()
    after = torch.rand(1)
    torch.manual_seed(seed)
    theirs = make_theirs()
    assert torch.equal(after, torch.rand(1)), "the constructor leaves the RNG where the reference leaves it"
    return ours, theirs


def test_mask_heads_state_init_and_version_1_keys():
    ours, theirs = _seeded(lambda: mv.MaskRCNNHeads(8, (6, 4), 1), lambda: M.MaskRCNNHeads(8, (6, 4), 1), 9650)
    _same_state(ours, theirs, ["0.0.weight", "0.0.bias", "1.0.weight", "1.0.bias"])
    assert not ours.training and mv.MaskRCNNHeads._version == 2
    assert not ours[0][0].bias.any() and float(ours[0][0].weight.detach().std()) > 0
    assert ours.state_dict()._metadata[""]["version"] == 2
    old = {"mask_fcn1.weight": torch.full((6, 8, 3, 3), 0.5), "mask_fcn1.bias": torch.full((6,), 0.25),
           "mask_fcn2.weight": torch.full((4, 6, 3, 3), -0.5), "mask_fcn2.bias": torch.full((4,), -0.25)}
    for module in (ours, theirs):
        module.load_state_dict(dict(old), strict=True)  # a plain dict has no metadata: version None
    _same_state(ours, theirs)
    assert bool((ours[1][0].weight == -0.5).all()) and bool((ours[0][0].bias == 0.25).all())
    # inside a parent: the prefix is honoured
    parent = torch.nn.Module()
    parent.mask_head = mv.MaskRCNNHeads(8, (6,), 1)
    parent.load_state_dict({"mask_head.mask_fcn1.weight": old["mask_fcn1.weight"], "mask_head.mask_fcn1.bias": old["mask_fcn1.bias"]}, strict=True)
    assert bool((parent.mask_head[0][0].weight == 0.5).all())
    with pytest.raises(RuntimeError, match="inference only"):
        mv.MaskRCNNHeads(4, (4,), 1).train()(torch.zeros(1, 4, 6, 6))
    with pytest.raises(NotImplementedError, match="dilation 1"):
        mv.MaskRCNNHeads(4, (4,), 2)(torch.zeros(1, 4, 6, 6))  # never reaches a kernel of another geometry


def test_mask_predictor_state_init_and_relayout_cache():
    ours, theirs = _seeded(lambda: mv.MaskRCNNPredictor(8, 6, 3), lambda: M.MaskRCNNPredictor(8, 6, 3), 9651)
    _same_state(ours, theirs, ["conv5_mask.weight", "conv5_mask.bias", "mask_fcn_logits.weight", "mask_fcn_logits.bias"])
    assert [n for n, _ in ours.named_children()] == ["conv5_mask", "relu", "mask_fcn_logits"]
    assert ours.conv5_mask.weight.shape == (8, 6, 2, 2) and ours.mask_fcn_logits.weight.shape == (3, 6, 1, 1) and not ours.training
    w4, b4 = ours.relaid(torch.device("cpu"))
    assert w4.shape == (24, 8) and b4.shape == (24,)
    assert torch.equal(w4[4 * 2 + 2 * 1 + 0], ours.conv5_mask.weight[:, 2, 1, 0]) and torch.equal(b4[8:12], ours.conv5_mask.bias[2].expand(4))
    assert ours.relaid(torch.device("cpu"))[0] is w4
    with torch.no_grad():
        ours.conv5_mask.bias.add_(1.0)
    assert torch.equal(ours.relaid(torch.device("cpu"))[1][::4], ours.conv5_mask.bias)
    with pytest.raises(RuntimeError, match="inference only"):
        mv.MaskRCNNPredictor(4, 4, 2).train()(torch.zeros(1, 4, 6, 6))


def test_mask_rcnn_state_equals_the_replica_on_a_resnet18_fpn():
    ours, theirs = _seeded(lambda: mv.MaskRCNN(mv.resnet_fpn_backbone(backbone_name="resnet18"), num_classes=5, _skip_resize=True),
                           lambda: M.MaskRCNN(FP.resnet_fpn_backbone(backbone_name="resnet18"), num_classes=5, _skip_resize=True), 9652)
    _same_state(ours, theirs)
    keys = list(ours.state_dict())
    assert keys[-12:] == [f"roi_heads.mask_head.{i}.0.{t}" for i in range(4) for t in ("weight", "bias")] + \
        [f"roi_heads.mask_predictor.{n}.{t}" for n in ("conv5_mask", "mask_fcn_logits") for t in ("weight", "bias")]
    heads = ours.roi_heads
    assert isinstance(ours, mv.FasterRCNN) and heads.has_mask() and not heads.has_keypoint() and not ours.training
    assert isinstance(heads.mask_roi_pool, mv.MultiScaleRoIAlign) and heads.mask_roi_pool.output_size == (14, 14)
    assert isinstance(heads.mask_head, mv.MaskRCNNHeads) and len(heads.mask_head) == 4 and heads.mask_head[3][0].out_channels == 256
    assert isinstance(heads.mask_predictor, mv.MaskRCNNPredictor) and heads.mask_predictor.mask_fcn_logits.out_channels == 5
    assert [n for n, _ in heads.named_children()] == [n for n, _ in theirs.roi_heads.named_children()]
    assert mask_rcnn.MaskRCNN is mv.MaskRCNN and mv.mask_rcnn.maskrcnn_resnet50_fpn is mv.maskrcnn_resnet50_fpn


def test_maskrcnn_resnet50_fpn_state_equals_the_replica():
    ours, theirs = _seeded(lambda: mv.maskrcnn_resnet50_fpn(num_classes=3), lambda: M.maskrcnn_resnet50_fpn(num_classes=3), 9653)
    _same_state(ours, theirs)
    assert ours.roi_heads.mask_predictor.mask_fcn_logits.out_channels == 3
    assert type(ours.backbone.body["bn1"]).__name__ == "FrozenBatchNorm2d"
    with pytest.raises(ValueError, match="no weight files"):
        mv.maskrcnn_resnet50_fpn(weights="DEFAULT")
    with pytest.raises(ValueError, match="no weight files"):
        mv.maskrcnn_resnet50_fpn(weights_backbone="IMAGENET1K_V1")
    with pytest.raises(TypeError):
        mv.maskrcnn_resnet50_fpn(None)  # keyword-only, as the reference


def test_mask_rcnn_argument_errors_are_the_references():
    backbone = mv.resnet_fpn_backbone(backbone_name="resnet18")
    with pytest.raises(TypeError, match="mask_roi_pool should be of type MultiScaleRoIAlign or None instead of <class 'str'>"):
        mv.MaskRCNN(backbone, num_classes=3, mask_roi_pool="pool")
    with pytest.raises(ValueError, match="num_classes should be None when mask_predictor is specified"):
        mv.MaskRCNN(backbone, num_classes=3, mask_predictor=mv.MaskRCNNPredictor(256, 256, 3))
    ref_backbone = FP.resnet_fpn_backbone(backbone_name="resnet18")
    for kw_ours, kw_theirs in ((dict(num_classes=3, mask_roi_pool=3), dict(num_classes=3, mask_roi_pool=3)),
                               (dict(num_classes=3, mask_predictor=mv.MaskRCNNPredictor(8, 8, 3)), dict(num_classes=3, mask_predictor=M.MaskRCNNPredictor(8, 8, 3))),
                               (dict(), dict()),  # FasterRCNN's own: num_classes should not be None ...
                               (dict(num_classes=3, rpn_anchor_generator=3), dict(num_classes=3, rpn_anchor_generator=3))):
        with pytest.raises((ValueError, TypeError)) as ours:
            mv.MaskRCNN(backbone, **kw_ours)
        with pytest.raises((ValueError, TypeError)) as theirs:
            M.MaskRCNN(ref_backbone, **kw_theirs)
        assert type(ours.value) is type(theirs.value) and str(ours.value) == str(theirs.value)
    custom = mv.MaskRCNN(backbone, box_predictor=mv.FastRCNNPredictor(1024, 7), mask_predictor=mv.MaskRCNNPredictor(256, 32, 7),
                         mask_roi_pool=mv.MultiScaleRoIAlign(["0", "1"], 7, 2), mask_head=mv.MaskRCNNHeads(256, (64, 256), 1), _skip_resize=True)
    assert custom.roi_heads.mask_roi_pool.output_size == (7, 7) and len(custom.roi_heads.mask_head) == 2


def test_roi_heads_accepts_only_this_packages_mask_modules():
    args = dict(box_roi_pool=mv.MultiScaleRoIAlign(["0", "1"], 2, 2), box_head=mv.TwoMLPHead(16 * 4, 32), box_predictor=mv.FastRCNNPredictor(32, 5),
                fg_iou_thresh=0.5, bg_iou_thresh=0.5, batch_size_per_image=512, positive_fraction=0.25, bbox_reg_weights=None, score_thresh=0.05,
                nms_thresh=0.5, detections_per_img=100)
    heads = mv.RoIHeads(**args, mask_roi_pool=mv.MultiScaleRoIAlign(["0", "1"], 4, 2), mask_head=mv.MaskRCNNHeads(16, (8,), 1),
                        mask_predictor=mv.MaskRCNNPredictor(8, 8, 5))
    assert heads.has_mask()
    for name, module in (("mask_roi_pool", H.MultiScaleRoIAlign(["0"], 4, 2)), ("mask_head", M.MaskRCNNHeads(16, (8,), 1)),
                         ("mask_predictor", M.MaskRCNNPredictor(8, 8, 5)), ("mask_head", torch.nn.Identity())):
        with pytest.raises(NotImplementedError, match=name):
            mv.RoIHeads(**args, **{name: module})
    for name in ("keypoint_roi_pool", "keypoint_head", "keypoint_predictor"):
        with pytest.raises(NotImplementedError, match=name):
            mv.RoIHeads(**args, **{name: mv.MultiScaleRoIAlign(["0"], 4, 2)})


# ---- the C entries: refusals with host pointers -----------------------------------------------------------------------------------------
def test_paste_masks_refusals_write_nothing():
    lib = _lib.load()
    masks, boxes = np.zeros((2, 4, 4), np.float32), np.zeros((2, 4), np.float32)
    y = np.full((2, 6, 8), SENT, np.float32)
    mp, bp, yp = masks.ctypes.data, boxes.ctypes.data, y.ctypes.data

    def call(**o):
        a = {**dict(masks=mp, boxes=bp, y=yp, r=2, m=4, padding=1, h=6, w=8), **o}
        return lib.mv_paste_masks_f32(a["masks"], a["boxes"], a["y"], a["r"], a["m"], a["padding"], a["h"], a["w"], None)
    cases = [(dict(masks=None), INVALID, "null pointer"), (dict(boxes=None), INVALID, "null pointer"), (dict(y=None), INVALID, "null pointer"),
             (dict(m=0), INVALID, "bad shape"), (dict(h=0), INVALID, "bad shape"), (dict(w=-2), INVALID, "bad shape"), (dict(r=-1), INVALID, "bad shape"),
             (dict(padding=-1), INVALID, "bad shape"), (dict(padding=2 ** 30), INVALID, "exceeds the index range"),
             (dict(y=mp), INVALID, "must not overlap"), (dict(y=bp + 16), INVALID, "must not overlap"), (dict(masks=yp + 4 * 95), INVALID, "must not overlap"),
             (dict(r=2 ** 45), INVALID, "exceed the address space"), (dict(r=2 ** 31, h=16, w=4, y=yp + 2 ** 50), UNSUPPORTED, "exceed the launch grid")]
    for over, status, text in cases:
        rc = call(**over)
        assert rc == status and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    assert call(r=0, masks=None, boxes=None, y=None) == 0
    assert call(r=0, m=0) == INVALID
    assert bool((y == SENT).all()) and not masks.any() and not boxes.any(), "a refused call wrote"


def test_mask_probs_refusals_write_nothing():
    lib = _lib.load()
    logits, labels = np.zeros((2, 3, 4, 4), np.float32), np.zeros(3, np.int64)
    y = np.full((2, 4, 4), SENT, np.float32)
    xp, lp, yp = logits.ctypes.data, labels.ctypes.data, y.ctypes.data

    def call(**o):
        a = {**dict(x=xp, labels=lp, y=yp, r=2, c=3, mh=4, mw=4), **o}
        return lib.mv_mask_probs_f32(a["x"], a["labels"], a["y"], a["r"], a["c"], a["mh"], a["mw"], None)
    cases = [(dict(x=None), INVALID, "null pointer"), (dict(labels=None), INVALID, "null pointer"), (dict(y=None), INVALID, "null pointer"),
             (dict(c=0), INVALID, "bad shape"), (dict(mh=0), INVALID, "bad shape"), (dict(mw=-1), INVALID, "bad shape"), (dict(r=-1), INVALID, "bad shape"),
             (dict(labels=lp + 4), INVALID, "8-byte aligned"), (dict(y=xp + 64), INVALID, "must not overlap"), (dict(y=lp), INVALID, "must not overlap"),
             (dict(r=2 ** 44), INVALID, "exceed the address space"), (dict(r=2 ** 36, c=1, y=yp + 2 ** 50), UNSUPPORTED, "exceed the launch grid")]
    for over, status, text in cases:
        rc = call(**over)
        assert rc == status and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    assert call(r=0, x=None, labels=None, y=None) == 0
    assert bool((y == SENT).all()), "a refused call wrote"


def test_conv_transpose_refusals_write_nothing():
    lib = _lib.load()
    x, w4, b4 = np.zeros((2, 3, 4, 5), np.float32), np.zeros((8, 3), np.float32), np.zeros(8, np.float32)
    y = np.full((2, 2, 8, 10), SENT, np.float32)
    xp, wp, bp, yp = x.ctypes.data, w4.ctypes.data, b4.ctypes.data, y.ctypes.data

    def call(**o):
        a = {**dict(x=xp, w=wp, b=bp, y=yp, n=2, cin=3, h=4, wd=5, cout=2, act=1), **o}
        return lib.mv_conv_transpose2x2_bias_act_f32(a["x"], a["w"], a["b"], a["y"], a["n"], a["cin"], a["h"], a["wd"], a["cout"], a["act"], None)
    cases = [(dict(x=None), INVALID, "null pointer"), (dict(w=None), INVALID, "null pointer"), (dict(y=None), INVALID, "null pointer"),
             (dict(n=-1), INVALID, "bad shape"), (dict(cin=0), INVALID, "bad shape"), (dict(cout=0), INVALID, "bad shape"), (dict(h=0), INVALID, "bad shape"),
             (dict(wd=-1), INVALID, "bad shape"), (dict(act=3), INVALID, "bad activation code"), (dict(act=-1), INVALID, "bad activation code"),
             (dict(cout=2 ** 30), UNSUPPORTED, "exceeds the index range"), (dict(y=xp), INVALID, "must not overlap"),
             (dict(y=wp + 32), INVALID, "must not overlap"), (dict(y=bp), INVALID, "must not overlap"), (dict(x=yp + 4 * 319), INVALID, "must not overlap"),
             (dict(n=2 ** 45), INVALID, "exceed the address space")]
    for over, status, text in cases:
        rc = call(**over)
        assert rc == status and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    assert call(n=0, x=None, w=None, y=None, b=None) == 0
    assert bool((y == SENT).all()), "a refused call wrote"


# ---- the Python checks fire before a device is needed -----------------------------------------------------------------------------------
def test_functional_checks_and_messages():
    masks, boxes = torch.zeros(3, 1, 28, 28), torch.zeros(3, 4)
    with pytest.raises(ValueError, match=r"shape \[R, 1, M, M\]"):
        F.paste_masks_in_image(torch.zeros(3, 28, 28), boxes, (8, 8))
    with pytest.raises(ValueError, match=r"shape \[R, 1, M, M\]"):
        F.paste_masks_in_image(torch.zeros(3, 1, 28, 14), boxes, (8, 8))
    with pytest.raises(ValueError, match=r"shape \[3, 4\]"):
        F.paste_masks_in_image(masks, torch.zeros(2, 4), (8, 8))
    with pytest.raises(TypeError, match="float32"):
        F.paste_masks_in_image(masks.double(), boxes, (8, 8))
    with pytest.raises(TypeError, match="float32"):
        F.paste_masks_in_image(masks, boxes.to(torch.int64), (8, 8))
    with pytest.raises(ValueError, match="padding non-negative"):
        F.paste_masks_in_image(masks, boxes, (8, 8), padding=-1)
    with pytest.raises(ValueError, match="sizes should be positive"):
        F.paste_masks_in_image(masks, boxes, (0, 8))
    with pytest.raises(ValueError, match="height, width"):
        F.paste_masks_in_image(masks, boxes, (8, 8, 3))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.paste_masks_in_image(masks, boxes, (8, 8))
    logits, labels = torch.zeros(3, 5, 4, 4), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"shape \[R, C, Mh, Mw\]"):
        F.mask_probs(torch.zeros(3, 5, 4), labels)
    with pytest.raises(ValueError, match=r"shape \[3\]"):
        F.mask_probs(logits, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError, match="float32"):
        F.mask_probs(logits.half(), labels)
    with pytest.raises(TypeError, match="int64"):
        F.mask_probs(logits, labels.to(torch.int32))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.mask_probs(logits, labels)
    x, w = torch.zeros(1, 4, 6, 6), torch.zeros(4, 3, 2, 2)
    for kw, name in ((dict(stride=1), "stride"), (dict(stride=(2, 1)), "stride"), (dict(padding=1), "padding"), (dict(output_padding=1), "output_padding"),
                     (dict(groups=2), "groups"), (dict(dilation=2), "dilation"), (dict(activation="silu"), "activation")):
        with pytest.raises(NotImplementedError, match=name):
            F.conv_transpose2d_bias_act(x, w, None, **kw)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        F.conv_transpose2d_bias_act(x, torch.zeros(4, 3, 3, 3))
    with pytest.raises(RuntimeError, match="does not fit 4 input channels"):
        F.conv_transpose2d_bias_act(x, torch.zeros(5, 3, 2, 2))
    with pytest.raises(RuntimeError, match="bias has 2 elements"):
        F.conv_transpose2d_bias_act(x, w, torch.zeros(2))
    with pytest.raises(RuntimeError, match="4D input and weight"):
        F.conv_transpose2d_bias_act(x[0], w)
    with pytest.raises(TypeError, match="float32"):
        F.conv_transpose2d_bias_act(x.double(), w.double())
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.conv_transpose2d_bias_act(x, w)
    assert F.paste_masks_in_image is mv.functional.paste_masks_in_image and mv._mask.mask_probs is F.mask_probs


def test_postprocess_without_masks_is_unchanged_and_masks_go_to_the_library():
    t = mv.GeneralizedRCNNTransform(800, 1333, [0.0] * 3, [1.0] * 3, _skip_resize=True)
    boxes = torch.tensor([[1.0, 2.0, 9.0, 8.0]])
    out = t.postprocess([{"boxes": boxes.clone()}], [(16, 16)], [(32, 32)])
    assert list(out[0]) == ["boxes"] and torch.equal(out[0]["boxes"], boxes * 2)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):  # the masks are pasted by the library, never by torch
        t.postprocess([{"boxes": boxes.clone(), "masks": torch.zeros(1, 1, 28, 28)}], [(16, 16)], [(32, 32)])
