"""RoIHeads / Faster R-CNN without a GPU: the two references of tests/_roi_heads_ref.py against each other, TwoMLPHead /
FastRCNNPredictor / RoIHeads / FasterRCNN / fasterrcnn_resnet50_fpn against the replica (state, initialisation), every refusal of
mv_roi_detections_f32 with host pointers (refusals come before any launch), the Python-side checks, the inference-only and argument
errors, and the transform's batching and box rescaling (plain torch: they run on the CPU) against the replica."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cpu_vision_amd as mv
from cpu_vision_amd import _lib, faster_rcnn, roi_heads, transform
from cpu_vision_amd import functional as F
from tests import _fpn_ref as FP
from tests import _roi_heads_ref as H
from tests import _rpn_ref as P

CLIP = math.log(1000.0 / 16)
SIZES = [(64, 96), (61, 90)]


def _inputs(seed, r, c, scale=3.0):
    """class_logits (r, c), box_regression (r, 4 c), proposals of two images: boxes inside and partly outside 64 x 96."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((r, c), generator=g) * scale
    deltas = torch.randn((r, 4 * c), generator=g) * 2
    p = torch.rand((r, 2), generator=g) * torch.tensor([80.0, 50.0]) - 5
    boxes = torch.cat([p, p + 4 + torch.rand((r, 2), generator=g) * 40], 1)
    split = r // 2
    return logits, deltas, [boxes[:split], boxes[split:]]


def _heads(numerics, score_thresh=0.05, weights=None, detections=100):
    return H.RoIHeads(None, None, None, 0.5, 0.5, 512, 0.25, weights, score_thresh, 0.5, detections, numerics=numerics).eval()


# ---- replica (a) against restatement (b) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [2, 5, 91, 257])
def test_replica_and_restatement_scores_agree_within_the_rounding_bound(classes):
    """With u = 2^-24 (half an ulp, relative) both sides compute the same m and the same x_j - m.  To first order:
      numerator     e_j: torch's vector exp is within 1 ulp (2 u), the correctly rounded one within u                        3 u
      denominator   the same two exp errors, carried through a sum of positive numbers (a weighted mean of them)            3 u
                    the C - 1 float32 additions of each sum, in whatever order: (C - 1) u each                        2 (C - 1) u
      normalisation the restatement divides (u); torch multiplies by the rounded reciprocal (2 u)                            3 u
    together (2 C + 7) 2^-24 relative -- one u more than a count with a division on both sides, because torch's CPU softmax
    normalises with `1 / sum` and a product."""
    logits, _, _ = _inputs(100 + classes, 257, classes)
    a, b = H.softmax_torch(logits), H.softmax_chain(logits)
    bound = H.score_bound(classes)
    assert bound == (2 * classes + 7) * 2.0 ** -24
    rel = ((a - b).abs() / b).max()
    print(f"C = {classes}: max relative distance {float(rel) / 2.0 ** -24:.2f} x 2^-24, bound {2 * classes + 7} x 2^-24")
    assert bool(((a - b).abs() <= bound * b).all())
    assert bool((b.sum(1) - 1).abs().max() < 1e-5)


def test_replica_and_restatement_boxes_agree_up_to_one_ulp_of_exp():
    """test_rpn_host's rule, with the box head's weights: bit-equal where torch.exp is the correctly rounded exp for dw and dh."""
    _, deltas, proposals = _inputs(7, 200, 5)
    a, b = _heads(H.REPLICA), _heads(H.RESTATEMENT)
    pa, pb = a.box_coder.decode(deltas, proposals).reshape(-1, 4), b.box_coder.decode(deltas, proposals).reshape(-1, 4)
    d = deltas.reshape(-1, 4)[:, 2:] / 5.0
    d = torch.clamp(d, max=CLIP)
    exact = (torch.exp(d) == P.exp_cr(d)).all(-1)
    assert exact.float().mean() > 0.9, "more than 10 % of the boxes excluded"
    np.testing.assert_array_equal(pa[exact].numpy(), pb[exact].numpy())
    # elsewhere: tests/test_rpn_host.py's bound (one ulp of exp moves the half side by side * 2^-23, the final sum rounds on each side)
    side, mag = (pb[:, 2:] - pb[:, :2]).abs().max(-1)[0], pb.abs().max(-1)[0]
    bound = ((side + mag * 2.0 ** -22) * 2.0 ** -23 + mag * 2.0 ** -23)[:, None]
    assert bool(((pa - pb).abs() <= bound)[~exact].all())


def test_detection_sets_are_equal_away_from_the_threshold():
    classes, thresh = 6, 0.05
    logits, deltas, proposals = _inputs(11, 120, classes)
    a, b = _heads(H.REPLICA, thresh), _heads(H.RESTATEMENT, thresh)
    da, db = a.dense(logits, deltas, proposals, SIZES), b.dense(logits, deltas, proposals, SIZES)
    # the inputs: no score within the rounding bound of the threshold, no side within a coordinate's rounding of min_size
    bound = H.score_bound(classes)
    assert bool(((db[1] - thresh).abs() > 2 * bound * thresh).all())
    ws, hs = db[0][..., 2] - db[0][..., 0], db[0][..., 3] - db[0][..., 1]
    assert bool(((ws - 1e-2).abs() > 1e-3).all()) and bool(((hs - 1e-2).abs() > 1e-3).all())
    assert torch.equal(da[3], db[3]) and torch.equal(da[2], db[2])
    assert 0.05 < float(db[3].float().mean()) < 0.95, "the threshold should split the scores"
    ra, rb = a.postprocess_detections(logits, deltas, proposals, SIZES), b.postprocess_detections(logits, deltas, proposals, SIZES)
    for la, lb, ba, bb in zip(ra[2], rb[2], ra[0], rb[0]):
        assert torch.equal(la, lb) and len(la) > 0
        assert bool(((ba - bb).abs() <= 1e-4).all())


def test_the_score_test_is_strict_and_in_float32_as_torch_is():
    """C = 2 and equal logits give 0.5 exactly on both sides; torch.where(scores > thresh) drops it, and compares in float32."""
    logits = torch.tensor([[1.25, 1.25], [0.0, -0.0]])
    deltas = torch.zeros(2, 8)
    proposals = [torch.tensor([[4.0, 4.0, 20.0, 30.0], [1.0, 2.0, 9.0, 8.0]])]
    for numerics in (H.REPLICA, H.RESTATEMENT):
        at = _heads(numerics, 0.5)
        boxes, scores, labels, valid = at.dense(logits, deltas, proposals, SIZES[:1])
        assert bool((scores == 0.5).all()) and not bool(valid.any())
        assert [len(s) for s in at.postprocess_detections(logits, deltas, proposals, SIZES[:1])[1]] == [0]
        below = _heads(numerics, float(np.nextafter(np.float32(0.5), np.float32(0))))
        assert bool(below.dense(logits, deltas, proposals, SIZES[:1])[3].all())
        assert [len(s) for s in below.postprocess_detections(logits, deltas, proposals, SIZES[:1])[1]] == [2]
    # the threshold is taken as (float): float32(0.05) is above the double 0.05, and torch does not call it greater
    assert not bool((torch.tensor([0.05], dtype=torch.float32) > 0.05).item())
    assert float(np.float32(0.05)) > 0.05


# ---- structure: state, initialisation, loads ----------------------------------------------------------------------------------------------
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


def test_two_mlp_head_and_predictor_state_equal_the_replica():
    ours, theirs = _seeded(lambda: mv.TwoMLPHead(16 * 4, 32), lambda: H.TwoMLPHead(16 * 4, 32), 3)
    _same_state(ours, theirs, ["fc6.weight", "fc6.bias", "fc7.weight", "fc7.bias"])
    ours, theirs = _seeded(lambda: mv.FastRCNNPredictor(32, 5), lambda: H.FastRCNNPredictor(32, 5), 4)
    _same_state(ours, theirs, ["cls_score.weight", "cls_score.bias", "bbox_pred.weight", "bbox_pred.bias"])
    assert ours.cls_score.weight.shape == (5, 32) and ours.bbox_pred.weight.shape == (20, 32)
    assert not ours.training


def test_predictor_joint_weight_follows_the_parameters():
    pred = mv.FastRCNNPredictor(8, 3)
    w, b = pred.joint_linear(torch.device("cpu"))
    assert w.shape == (15, 8) and b.shape == (15,)
    assert torch.equal(w[:3], pred.cls_score.weight) and torch.equal(w[3:], pred.bbox_pred.weight)
    assert pred.joint_linear(torch.device("cpu"))[0] is w
    with torch.no_grad():
        pred.bbox_pred.bias.add_(1.0)
    w2, b2 = pred.joint_linear(torch.device("cpu"))
    assert torch.equal(b2[3:], pred.bbox_pred.bias) and torch.equal(b2[:3], pred.cls_score.bias)
    with pytest.raises(AssertionError, match="x has the wrong shape"):
        pred(torch.zeros(2, 2, 2, 2))


def _lib_heads(**kw):
    args = dict(box_roi_pool=mv.MultiScaleRoIAlign(["0", "1"], 2, 2), box_head=mv.TwoMLPHead(16 * 4, 32), box_predictor=mv.FastRCNNPredictor(32, 5),
                fg_iou_thresh=0.5, bg_iou_thresh=0.5, batch_size_per_image=512, positive_fraction=0.25, bbox_reg_weights=None, score_thresh=0.05,
                nms_thresh=0.5, detections_per_img=100)
    args.update(kw)
    return mv.RoIHeads(**args)


def test_roi_heads_state_and_attributes():
    ours, theirs = _seeded(_lib_heads, lambda: H.RoIHeads(H.MultiScaleRoIAlign(["0", "1"], 2, 2), H.TwoMLPHead(16 * 4, 32), H.FastRCNNPredictor(32, 5),
                                                           0.5, 0.5, 512, 0.25, None, 0.05, 0.5, 100), 5)
    _same_state(ours, theirs, ["box_head.fc6.weight", "box_head.fc6.bias", "box_head.fc7.weight", "box_head.fc7.bias",
                               "box_predictor.cls_score.weight", "box_predictor.cls_score.bias", "box_predictor.bbox_pred.weight",
                               "box_predictor.bbox_pred.bias"])
    assert ours.box_coder.weights == (10.0, 10.0, 5.0, 5.0) and ours.box_coder.bbox_xform_clip == CLIP
    assert _lib_heads(bbox_reg_weights=(1.0, 2.0, 3.0, 4.0)).box_coder.weights == (1.0, 2.0, 3.0, 4.0)
    assert (ours.score_thresh, ours.nms_thresh, ours.detections_per_img) == (0.05, 0.5, 100)
    assert (ours.fg_iou_thresh, ours.bg_iou_thresh, ours.batch_size_per_image, ours.positive_fraction) == (0.5, 0.5, 512, 0.25)
    assert not ours.has_mask() and not ours.has_keypoint() and not ours.training


def test_faster_rcnn_state_equals_the_replica_on_a_resnet18_fpn():
    ours, theirs = _seeded(lambda: mv.FasterRCNN(mv.resnet_fpn_backbone(backbone_name="resnet18"), num_classes=5, _skip_resize=True),
                           lambda: H.FasterRCNN(FP.resnet_fpn_backbone(backbone_name="resnet18"), num_classes=5, _skip_resize=True), 6)
    _same_state(ours, theirs)
    assert [n for n, _ in ours.named_children()] == [n for n, _ in theirs.named_children()] == ["transform", "backbone", "rpn", "roi_heads"]
    assert isinstance(ours.rpn, mv.RegionProposalNetwork) and isinstance(ours.roi_heads, mv.RoIHeads)
    assert isinstance(ours.roi_heads.box_roi_pool, mv.MultiScaleRoIAlign) and ours.roi_heads.box_roi_pool.output_size == (7, 7)
    assert ours.roi_heads.box_head.fc6.in_features == 256 * 49 and ours.roi_heads.box_predictor.cls_score.out_features == 5
    assert ours.rpn.pre_nms_top_n() == 1000 and ours.rpn.post_nms_top_n() == 1000 and ours.rpn.nms_thresh == 0.7
    assert ours.transform.min_size == (800,) and ours.transform.max_size == 1333 and ours.transform._skip_resize is True
    assert ours.transform.image_mean == [0.485, 0.456, 0.406] and ours.transform.image_std == [0.229, 0.224, 0.225]
    assert not ours.training


def test_fasterrcnn_resnet50_fpn_state_equals_the_replica():
    ours, theirs = _seeded(lambda: mv.fasterrcnn_resnet50_fpn(num_classes=3), lambda: H.fasterrcnn_resnet50_fpn(num_classes=3), 8)
    _same_state(ours, theirs)
    assert "backbone.body.layer4.2.bn3.running_var" in ours.state_dict() and "backbone.fpn.layer_blocks.3.0.weight" in ours.state_dict()
    assert ours.roi_heads.box_predictor.bbox_pred.out_features == 12
    assert type(ours.backbone.body["bn1"]).__name__ == "FrozenBatchNorm2d"
    with pytest.raises(ValueError, match="no weight files"):
        mv.fasterrcnn_resnet50_fpn(weights="DEFAULT")
    with pytest.raises(ValueError, match="no weight files"):
        mv.fasterrcnn_resnet50_fpn(weights_backbone="IMAGENET1K_V1")
    with pytest.raises(TypeError):
        mv.fasterrcnn_resnet50_fpn(None)  # keyword-only, as the reference


# ---- the C entry: refusals with host pointers ---------------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -2
SENT = -7.25


class _Call:
    """r = 3 rois, 4 classes, one image, everything in host memory: valid arguments that single tests spoil."""

    def __init__(self):
        self.logits, self.deltas = np.zeros(3 * 4 + 8, np.float32), np.zeros(3 * 16 + 8, np.float32)
        self.rois, self.sizes = np.zeros(15, np.float32), np.array([20.0, 28.0], np.float32)
        self.boxes, self.scores = np.full(36, SENT, np.float32), np.full(9, SENT, np.float32)
        self.labels, self.valid = np.full(9, 0x5AA5C33C, np.int64), np.full(9, 0xA5, np.uint8)
        self.kw = dict(logits=self.logits.ctypes.data, ls=4, deltas=self.deltas.ctypes.data, ds=16, rois=self.rois.ctypes.data,
                       sizes=self.sizes.ctypes.data, r=3, c=4, n=1, boxes=self.boxes.ctypes.data, scores=self.scores.ctypes.data,
                       labels=self.labels.ctypes.data, valid=self.valid.ctypes.data)

    def call(self, **over):
        a = {**self.kw, **over}
        lib = _lib.load()
        rc = lib.mv_roi_detections_f32(a["logits"], a["ls"], a["deltas"], a["ds"], a["rois"], a["sizes"], a["r"], a["c"], a["n"], 10.0, 10.0, 5.0,
                                       5.0, CLIP, 0.05, 1e-2, a["boxes"], a["scores"], a["labels"], a["valid"], None)
        assert bool((self.boxes == SENT).all()) and bool((self.scores == SENT).all()) and bool((self.labels == 0x5AA5C33C).all()) and \
            bool((self.valid == 0xA5).all()), "a refused call wrote"
        return rc, lib.mv_last_error().decode()


def test_roi_detections_refusals():
    d = _Call()
    cases = [(dict(**{name: None}), INVALID, "null pointer") for name in ("logits", "deltas", "rois", "sizes", "boxes", "scores", "labels", "valid")]
    cases += [
        (dict(c=1), INVALID, "at least 2 classes"),
        (dict(c=0), INVALID, "at least 2 classes"),
        (dict(c=2049, ls=2049, ds=4 * 2049), UNSUPPORTED, "up to 2048 classes"),
        (dict(ls=3), INVALID, "row strides"),
        (dict(ds=15), INVALID, "row strides"),
        (dict(r=-1), INVALID, "bad shape"),
        (dict(n=-1), INVALID, "bad shape"),
        (dict(n=0), INVALID, "no image"),
        (dict(r=1 << 29), UNSUPPORTED, "32-bit index"),
        (dict(r=(1 << 31) // 4), UNSUPPORTED, "32-bit index"),
        (dict(labels=d.labels.ctypes.data + 4), INVALID, "8-byte aligned"),
        (dict(boxes=d.deltas.ctypes.data), INVALID, "must not overlap"),
        (dict(scores=d.logits.ctypes.data + 4 * 11), INVALID, "must not overlap"),
        (dict(scores=d.boxes.ctypes.data + 4 * 35), INVALID, "must not overlap"),
        (dict(valid=d.rois.ctypes.data + 59), INVALID, "must not overlap"),
        (dict(labels=d.sizes.ctypes.data), INVALID, "must not overlap"),
        (dict(valid=d.labels.ctypes.data + 71), INVALID, "must not overlap"),
        # the strides count: rows 2 elements apart reach 4 elements past a (3, 4) block
        (dict(ls=6, scores=d.logits.ctypes.data + 4 * 15), INVALID, "must not overlap"),
    ]
    for over, status, text in cases:
        rc, msg = d.call(**over)
        assert rc == status and text in msg, (list(over), rc, msg)
    # R == 0 is a no-op that touches no pointer; the shape checks still come first
    assert d.call(r=0, logits=None, deltas=None, rois=None, sizes=None, boxes=None, scores=None, labels=None, valid=None, n=0)[0] == 0
    assert d.call(r=0, c=1)[0] == INVALID
    assert F.MAX_ROI_CLASSES == 2048


# ---- the Python checks fire before a device is needed ---------------------------------------------------------------------------------
def test_functional_checks_and_messages():
    logits, deltas, rois = torch.zeros(3, 4), torch.zeros(3, 16), torch.zeros(3, 5)
    sizes = [(20, 28)]
    with pytest.raises(RuntimeError, match=r"class_logits should have shape \(R, C\)"):
        F.roi_detections(torch.zeros(3), deltas, rois, sizes)
    with pytest.raises(RuntimeError, match=r"box_regression should have shape \(3, 16\)"):
        F.roi_detections(logits, torch.zeros(3, 12), rois, sizes)
    with pytest.raises(RuntimeError, match=r"rois should have shape \(3, 5\)"):
        F.roi_detections(logits, deltas, torch.zeros(3, 4), sizes)
    with pytest.raises(TypeError, match="float32"):
        F.roi_detections(logits.double(), deltas, rois, sizes)
    with pytest.raises(TypeError, match="float32"):
        F.roi_detections(logits, deltas, rois.half(), sizes)
    with pytest.raises(ValueError, match="at least 2 classes"):
        F.roi_detections(torch.zeros(3, 1), torch.zeros(3, 4), rois, sizes)
    with pytest.raises(_lib.Mi355VisionError, match="up to 2048 classes"):
        F.roi_detections(torch.zeros(1, 2049), torch.zeros(1, 4 * 2049), torch.zeros(1, 5), sizes)
    with pytest.raises(ValueError, match="four weights"):
        F.roi_detections(logits, deltas, rois, sizes, weights=(1.0, 1.0))
    with pytest.raises(RuntimeError, match="image_sizes should hold"):
        F.roi_detections(logits, deltas, rois, [])
    with pytest.raises(RuntimeError, match="image_sizes should hold"):
        F.roi_detections(logits, deltas, rois, torch.zeros(2, 3))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.roi_detections(logits, deltas, rois, sizes)
    assert mv.roi_heads.RoIHeads is mv.RoIHeads and mv.faster_rcnn.FasterRCNN is mv.FasterRCNN
    assert mv.transform.GeneralizedRCNNTransform is mv.GeneralizedRCNNTransform and mv.generalized_rcnn.GeneralizedRCNN is mv.GeneralizedRCNN


# ---- inference only; the branches that are not built ----------------------------------------------------------------------------------------
def test_not_implemented_and_inference_only_paths():
    for name in ("mask_roi_pool", "mask_head", "mask_predictor", "keypoint_roi_pool", "keypoint_head", "keypoint_predictor"):
        with pytest.raises(NotImplementedError, match=name):
            _lib_heads(**{name: torch.nn.Identity()})
    heads = _lib_heads()
    feats = {"0": torch.zeros(1, 16, 8, 8), "1": torch.zeros(1, 16, 4, 4)}
    props = [torch.tensor([[1.0, 1.0, 9.0, 9.0]])]
    with pytest.raises(RuntimeError, match="inference only"):
        heads(feats, props, [(32, 32)], targets=[{}])
    heads.train()
    with pytest.raises(RuntimeError, match="inference only"):
        heads(feats, props, [(32, 32)])
    heads.eval()
    with pytest.raises(TypeError, match="float32"):
        heads({k: v.double() for k, v in feats.items()}, props, [(32, 32)])
    with pytest.raises(RuntimeError, match="inference only"):
        mv.TwoMLPHead(4, 4).train()(torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match="inference only"):
        mv.FastRCNNPredictor(4, 2).train()(torch.zeros(1, 4))
    # the transform: no resize in the library yet
    t = mv.GeneralizedRCNNTransform(800, 1333, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    assert t._skip_resize is False and t.min_size == (800,) and t.size_divisible == 32 and t.fixed_size is None
    with pytest.raises(NotImplementedError, match="non-antialiased bilinear"):
        t.resize(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="list of 3d tensors"):
        t([torch.zeros(1, 3, 8, 8)])
    with pytest.raises(TypeError, match="floating type"):
        t([torch.zeros(3, 8, 8, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match="inference only"):
        t([torch.zeros(3, 8, 8)], targets=[{}])
    skip = mv.GeneralizedRCNNTransform((640, 800), 1333, [0.5] * 3, [0.25] * 3, size_divisible=16, fixed_size=(4, 4), _skip_resize=True)
    assert skip._skip_resize is True and skip.min_size == (640, 800) and skip.size_divisible == 16 and skip.fixed_size == (4, 4)
    image = torch.zeros(3, 8, 8)
    assert skip.resize(image) is image
    assert "Normalize(mean=[0.5, 0.5, 0.5], std=[0.25, 0.25, 0.25])" in repr(skip) and "Resize(min_size=(640, 800), max_size=1333, mode='bilinear')" in repr(skip)
    model = mv.FasterRCNN(mv.resnet_fpn_backbone(backbone_name="resnet18"), num_classes=3, _skip_resize=True)
    with pytest.raises(RuntimeError, match="inference only"):
        model([torch.zeros(3, 32, 32)], targets=[{}])
    with pytest.raises(RuntimeError, match="inference only"):
        model.train()([torch.zeros(3, 32, 32)])


def test_faster_rcnn_argument_errors_are_the_references():
    backbone = mv.resnet_fpn_backbone(backbone_name="resnet18")
    with pytest.raises(ValueError, match="backbone should contain an attribute out_channels"):
        mv.FasterRCNN(torch.nn.Identity(), num_classes=3)
    with pytest.raises(TypeError, match="rpn_anchor_generator should be of type AnchorGenerator or None instead of <class 'int'>"):
        mv.FasterRCNN(backbone, num_classes=3, rpn_anchor_generator=3)
    with pytest.raises(TypeError, match="box_roi_pool should be of type MultiScaleRoIAlign or None instead of <class 'str'>"):
        mv.FasterRCNN(backbone, num_classes=3, box_roi_pool="pool")
    with pytest.raises(ValueError, match="num_classes should be None when box_predictor is specified"):
        mv.FasterRCNN(backbone, num_classes=3, box_predictor=mv.FastRCNNPredictor(1024, 3))
    with pytest.raises(ValueError, match="num_classes should not be None when box_predictor is not specified"):
        mv.FasterRCNN(backbone)
    for make, other in ((lambda **kw: mv.FasterRCNN(backbone, **kw), lambda **kw: H.FasterRCNN(FP.resnet_fpn_backbone(backbone_name="resnet18"), **kw)),):
        for kw in (dict(), dict(num_classes=3, rpn_anchor_generator=3), dict(num_classes=3, box_predictor=H.FastRCNNPredictor(8, 3))):
            with pytest.raises((ValueError, TypeError)) as ours:
                make(**kw)
            with pytest.raises((ValueError, TypeError)) as theirs:
                other(**kw)
            assert type(ours.value) is type(theirs.value) and str(ours.value) == str(theirs.value)
    custom = mv.FasterRCNN(backbone, box_predictor=mv.FastRCNNPredictor(1024, 7), rpn_anchor_generator=mv.AnchorGenerator(((16, 32),) * 5, ((1.0,),) * 5),
                           box_detections_per_img=9, box_score_thresh=0.3, box_nms_thresh=0.4, bbox_reg_weights=(1.0, 1.0, 1.0, 1.0),
                           rpn_pre_nms_top_n_test=77, size_divisible=64, _skip_resize=True)
    assert custom.rpn.head.cls_logits.out_channels == 2 and custom.rpn.pre_nms_top_n() == 77 and custom.transform.size_divisible == 64
    assert (custom.roi_heads.detections_per_img, custom.roi_heads.score_thresh, custom.roi_heads.nms_thresh) == (9, 0.3, 0.4)
    assert custom.roi_heads.box_coder.weights == (1.0, 1.0, 1.0, 1.0)


# ---- the transform's torch halves on the CPU -------------------------------------------------------------------------------------------------
def test_batch_images_and_postprocess_equal_the_replica():
    g = torch.Generator().manual_seed(21)
    images = [torch.rand((3, 30, 45), generator=g), torch.rand((3, 33, 40), generator=g), torch.rand((3, 17, 64), generator=g)]
    for div in (32, 16, 1):
        ours = mv.GeneralizedRCNNTransform(800, 1333, [0.0] * 3, [1.0] * 3, size_divisible=div, _skip_resize=True)
        theirs = H.GeneralizedRCNNTransform(800, 1333, [0.0] * 3, [1.0] * 3, size_divisible=div, _skip_resize=True).eval()
        got, want = ours.batch_images(images, div), theirs.batch_images(images, div)
        assert got.shape == want.shape and torch.equal(got, want)
        assert got.shape[-2] % div == 0 and got.shape[-1] % div == 0 and bool((got[0, :, 30:] == 0).all())
    boxes = [torch.rand((5, 4), generator=g) * 100, torch.rand((0, 4), generator=g), torch.rand((2, 4), generator=g) * 50]
    shapes, originals = [(30, 45), (33, 40), (17, 64)], [(60, 91), (33, 40), (100, 7)]

    def result():
        return [{"boxes": b.clone(), "labels": torch.zeros(len(b), dtype=torch.int64), "scores": torch.ones(len(b))} for b in boxes]
    got, want = ours.postprocess(result(), shapes, originals), theirs.postprocess(result(), shapes, originals)
    for gd, wd, b in zip(got, want, boxes):
        assert torch.equal(gd["boxes"], wd["boxes"]) and gd["boxes"].shape == b.shape
    assert torch.equal(transform.resize_boxes(boxes[0], (30, 45), (60, 91)), H.resize_boxes(boxes[0], (30, 45), (60, 91)))
    assert torch.equal(got[1]["boxes"], boxes[1]) and not torch.equal(got[0]["boxes"], boxes[0])
    assert roi_heads.postprocess_detections_detailed is not None and faster_rcnn.TwoMLPHead is mv.TwoMLPHead
