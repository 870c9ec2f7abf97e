"""The keypoint branch of Keypoint R-CNN without a GPU: KeypointRCNNHeads / KeypointRCNNPredictor / KeypointRCNN /
keypointrcnn_resnet50_fpn against the replica of tests/_keypoint_ref.py (state, initialisation, argument errors), what RoIHeads accepts
as keypoint modules, the relaid transposed conv against torch, the restatement of heatmaps_to_keypoints against the replica (values
within the bound of DESIGN.md 3.29, positions exactly where the replica's own top-two gap exceeds twice that bound), every refusal of
the two C entries with host pointers (refusals come before any launch and write nothing) and the Python-side checks, which fire
before a device is needed."""
import numpy as np
import pytest
import torch

import cpu_vision_amd as mv
from cpu_vision_amd import _lib, keypoint_rcnn
from cpu_vision_amd import functional as F
from tests import _fpn_ref as FP
from tests import _keypoint_ref as KR
from tests import _roi_heads_ref as H

INVALID, UNSUPPORTED = -1, -2
SENT = -7.25


# ---- structure: state, initialisation, argument errors ---------------------------------------------------------------------------------------
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


def test_keypoint_heads_state_and_init():
    ours, theirs = _seeded(lambda: mv.KeypointRCNNHeads(8, (6, 4, 5)), lambda: KR.KeypointRCNNHeads(8, (6, 4, 5)), 9800)
    _same_state(ours, theirs, [f"{i}.{t}" for i in (0, 2, 4) for t in ("weight", "bias")])
    assert [type(m).__name__ for m in ours] == ["Conv2d", "ReLU"] * 3 and not ours.training
    assert not ours[0].bias.any() and float(ours[0].weight.detach().std()) > 0 and ours[4].weight.shape == (5, 4, 3, 3)
    with pytest.raises(RuntimeError, match="inference only"):
        mv.KeypointRCNNHeads(4, (4,)).train()(torch.zeros(1, 4, 6, 6))


def test_keypoint_predictor_state_init_and_relayout_cache():
    ours, theirs = _seeded(lambda: mv.KeypointRCNNPredictor(8, 3), lambda: KR.KeypointRCNNPredictor(8, 3), 9801)
    _same_state(ours, theirs, ["kps_score_lowres.weight", "kps_score_lowres.bias"])
    conv = ours.kps_score_lowres
    assert [n for n, _ in ours.named_children()] == ["kps_score_lowres"] and (ours.up_scale, ours.out_channels) == (2, 3)
    assert conv.weight.shape == (8, 3, 4, 4) and (conv.stride, conv.padding, conv.output_padding) == ((2, 2), (1, 1), (0, 0))
    assert not conv.bias.any() and not ours.training
    w2, b4 = ours.relaid(torch.device("cpu"))
    assert w2.shape == (12, 8, 2, 2) and b4.shape == (12,)
    # row 4 co + 2 py + px, tap (ty, tx) = weight[:, co, 3 - py - 2 ty, 3 - px - 2 tx]
    assert torch.equal(w2[4 * 2 + 2 * 1 + 0, :, 1, 0], conv.weight[:, 2, 0, 3]) and torch.equal(w2[0, :, 0, 0], conv.weight[:, 0, 3, 3])
    assert ours.relaid(torch.device("cpu"))[0] is w2
    with torch.no_grad():
        conv.bias.add_(1.0)
    assert torch.equal(ours.relaid(torch.device("cpu"))[1][::4], conv.bias)
    with pytest.raises(RuntimeError, match="inference only"):
        mv.KeypointRCNNPredictor(4, 2).train()(torch.zeros(1, 4, 6, 6))


def test_keypoint_rcnn_state_equals_the_replica_on_a_resnet18_fpn():
    ours, theirs = _seeded(lambda: mv.KeypointRCNN(mv.resnet_fpn_backbone(backbone_name="resnet18"), num_classes=2, _skip_resize=True),
                           lambda: KR.KeypointRCNN(FP.resnet_fpn_backbone(backbone_name="resnet18"), num_classes=2, _skip_resize=True), 9802)
    _same_state(ours, theirs)
    keys = list(ours.state_dict())
    assert keys[-18:] == [f"roi_heads.keypoint_head.{i}.{t}" for i in range(0, 16, 2) for t in ("weight", "bias")] + \
        [f"roi_heads.keypoint_predictor.kps_score_lowres.{t}" for t in ("weight", "bias")]
    heads = ours.roi_heads
    assert isinstance(ours, mv.FasterRCNN) and heads.has_keypoint() and not heads.has_mask() and not ours.training
    assert isinstance(heads.keypoint_roi_pool, mv.MultiScaleRoIAlign) and heads.keypoint_roi_pool.output_size == (14, 14)
    assert isinstance(heads.keypoint_head, mv.KeypointRCNNHeads) and len(heads.keypoint_head) == 16 and heads.keypoint_head[14].out_channels == 512
    assert isinstance(heads.keypoint_predictor, mv.KeypointRCNNPredictor) and heads.keypoint_predictor.kps_score_lowres.out_channels == 17
    assert [n for n, _ in heads.named_children()] == [n for n, _ in theirs.roi_heads.named_children()]
    assert tuple(ours.transform.min_size) == tuple(theirs.transform.min_size) == (640, 672, 704, 736, 768, 800)
    assert keypoint_rcnn.KeypointRCNN is mv.KeypointRCNN and mv.keypoint_rcnn.keypointrcnn_resnet50_fpn is mv.keypointrcnn_resnet50_fpn


def test_keypointrcnn_resnet50_fpn_state_equals_the_replica():
    ours, theirs = _seeded(lambda: mv.keypointrcnn_resnet50_fpn(num_keypoints=5), lambda: KR.keypointrcnn_resnet50_fpn(num_keypoints=5), 9803)
    _same_state(ours, theirs)
    assert ours.roi_heads.keypoint_predictor.kps_score_lowres.out_channels == 5 and ours.roi_heads.box_predictor.cls_score.out_features == 2
    assert type(ours.backbone.body["bn1"]).__name__ == "FrozenBatchNorm2d"
    with pytest.raises(ValueError, match="no weight files"):
        mv.keypointrcnn_resnet50_fpn(weights="DEFAULT")
    with pytest.raises(ValueError, match="no weight files"):
        mv.keypointrcnn_resnet50_fpn(weights_backbone="IMAGENET1K_V1")
    with pytest.raises(TypeError):
        mv.keypointrcnn_resnet50_fpn(None)  # keyword-only, as the reference


def test_keypoint_rcnn_argument_errors_are_the_references():
    backbone = mv.resnet_fpn_backbone(backbone_name="resnet18")
    with pytest.raises(TypeError, match="keypoint_roi_pool should be of type MultiScaleRoIAlign or None instead of <class 'str'>"):
        mv.KeypointRCNN(backbone, num_classes=2, keypoint_roi_pool="pool")
    with pytest.raises(ValueError, match="num_keypoints should be None when keypoint_predictor is specified"):
        mv.KeypointRCNN(backbone, num_classes=2, num_keypoints=17, keypoint_predictor=mv.KeypointRCNNPredictor(512, 17))
    ref_backbone = FP.resnet_fpn_backbone(backbone_name="resnet18")
    for kw_ours, kw_theirs in ((dict(num_classes=2, keypoint_roi_pool=3), dict(num_classes=2, keypoint_roi_pool=3)),
                               (dict(num_classes=2, num_keypoints=4, keypoint_predictor=mv.KeypointRCNNPredictor(8, 4)),
                                dict(num_classes=2, num_keypoints=4, keypoint_predictor=KR.KeypointRCNNPredictor(8, 4))),
                               (dict(), dict()),  # FasterRCNN's own: num_classes should not be None ...
                               (dict(num_classes=2, rpn_anchor_generator=3), dict(num_classes=2, rpn_anchor_generator=3))):
        with pytest.raises((ValueError, TypeError)) as ours:
            mv.KeypointRCNN(backbone, **kw_ours)
        with pytest.raises((ValueError, TypeError)) as theirs:
            KR.KeypointRCNN(ref_backbone, **kw_theirs)
        assert type(ours.value) is type(theirs.value) and str(ours.value) == str(theirs.value)
    custom = mv.KeypointRCNN(backbone, num_classes=2, keypoint_predictor=mv.KeypointRCNNPredictor(64, 4),
                             keypoint_roi_pool=mv.MultiScaleRoIAlign(["0", "1"], 7, 2), keypoint_head=mv.KeypointRCNNHeads(256, (32, 64)),
                             _skip_resize=True)
    assert custom.roi_heads.keypoint_roi_pool.output_size == (7, 7) and len(custom.roi_heads.keypoint_head) == 4
    with pytest.raises(NotImplementedError, match="keypoint_head"):
        mv.KeypointRCNN(backbone, num_classes=2, keypoint_head=KR.KeypointRCNNHeads(256, (32,)))


def test_roi_heads_accepts_only_this_packages_keypoint_modules_all_three():
    args = dict(box_roi_pool=mv.MultiScaleRoIAlign(["0", "1"], 2, 2), box_head=mv.TwoMLPHead(16 * 4, 32), box_predictor=mv.FastRCNNPredictor(32, 5),
                fg_iou_thresh=0.5, bg_iou_thresh=0.5, batch_size_per_image=512, positive_fraction=0.25, bbox_reg_weights=None, score_thresh=0.05,
                nms_thresh=0.5, detections_per_img=100)
    ours = dict(keypoint_roi_pool=mv.MultiScaleRoIAlign(["0", "1"], 4, 2), keypoint_head=mv.KeypointRCNNHeads(16, (8,)),
                keypoint_predictor=mv.KeypointRCNNPredictor(8, 3))
    heads = mv.RoIHeads(**args, **ours)
    assert heads.has_keypoint() and not heads.has_mask()
    assert [n for n, _ in heads.named_children()][-3:] == ["keypoint_roi_pool", "keypoint_head", "keypoint_predictor"]
    for name, module in (("keypoint_roi_pool", H.MultiScaleRoIAlign(["0"], 4, 2)), ("keypoint_head", KR.KeypointRCNNHeads(16, (8,))),
                         ("keypoint_predictor", KR.KeypointRCNNPredictor(8, 3)), ("keypoint_head", torch.nn.Identity()),
                         ("keypoint_predictor", mv.MaskRCNNPredictor(8, 8, 3))):
        with pytest.raises(NotImplementedError, match=name):
            mv.RoIHeads(**args, **{**ours, name: module})
    for name in ours:  # one module, or two, without the rest: stricter than the reference, which would run no keypoint branch
        with pytest.raises(NotImplementedError, match=f"{name} given without"):
            mv.RoIHeads(**args, **{name: ours[name]})
        with pytest.raises(NotImplementedError, match=f"without {name}"):
            mv.RoIHeads(**args, **{k: v for k, v in ours.items() if k != name})
    heads.keypoint_head = torch.nn.Identity()  # assigned after construction: refused by forward, before anything runs
    feats = {"0": torch.zeros(1, 16, 8, 8), "1": torch.zeros(1, 16, 4, 4)}
    with pytest.raises((NotImplementedError, _lib.Mi355VisionError)):
        heads(feats, [torch.tensor([[1.0, 1.0, 9.0, 9.0]])], [(32, 32)])


def test_postprocess_rescales_the_keypoints_as_the_replica():
    g = torch.Generator().manual_seed(9804)
    kps = torch.rand((5, 3, 3), generator=g) * 100
    kps[..., 2] = 1
    boxes = torch.rand((5, 4), generator=g) * 100
    t = mv.GeneralizedRCNNTransform(64, 128, [0.0] * 3, [1.0] * 3)
    out = t.postprocess([{"boxes": boxes.clone(), "keypoints": kps.clone(), "keypoints_scores": torch.ones(5, 3)}], [(120, 150)], [(77, 201)])
    want = KR.resize_keypoints(kps, (120, 150), (77, 201))
    assert torch.equal(out[0]["keypoints"], want) and list(out[0]) == ["boxes", "keypoints", "keypoints_scores"]
    assert torch.equal(want[..., 2], kps[..., 2]) and not torch.equal(want[..., 0], kps[..., 0])


# ---- the relaid transposed conv against torch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cin,h,w,cout", [(2, 8, 5, 7, 3), (1, 4, 1, 1, 1), (1, 24, 14, 14, 17)])
@pytest.mark.parametrize("bias", [True, False])
def test_relaid_composition_equals_torch_conv_transpose2d(n, cin, h, w, cout, bias):
    g = torch.Generator().manual_seed(9810 + cin)
    x = torch.rand((n, cin, h, w), generator=g) * 2 - 1
    wt = torch.randn((cin, cout, 4, 4), generator=g) * 0.2
    b = torch.randn((cout,), generator=g) if bias else None
    want = torch.relu(torch.nn.functional.conv_transpose2d(x, wt, b, stride=2, padding=1)).numpy()
    got = KR.oracle_conv_transpose4(x.numpy(), wt.numpy(), None if b is None else b.numpy(), "relu")
    assert got.shape == want.shape == (n, cout, 2 * h, 2 * w)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()))
    assert (want > 0).any() and (want == 0).any()
    w2, b4 = KR.relaid4(wt.numpy(), None if b is None else b.numpy())
    lw2, lb4 = F.conv_transpose4x4_relayout(wt, b, torch.device("cpu"))
    np.testing.assert_array_equal(lw2.numpy(), w2)
    assert (b4 is None and lb4 is None) or np.array_equal(lb4.numpy(), b4)
    np.testing.assert_array_equal(w2[4 * (cout - 1) + 2 * 1 + 0, :, 0, 1], wt.numpy()[:, cout - 1, 2, 1])


# ---- the restatement of heatmaps_to_keypoints against the replica -----------------------------------------------------------------------------
def _bump_maps(seed, r, k, mh, mw):
    """One dominant, lopsided bump per heatmap (the peak, a weaker right and a weaker lower neighbour) on small noise."""
    g = torch.Generator().manual_seed(seed)
    maps = torch.randn((r, k, mh, mw), generator=g) * 0.05
    py = torch.randint(0, mh, (r, k), generator=g)
    px = torch.randint(0, mw, (r, k), generator=g)
    side = torch.rand((r, k, 2), generator=g) * 0.4 + 0.2
    for i in range(r):
        for j in range(k):
            y, x = int(py[i, j]), int(px[i, j])
            maps[i, j, y, x] += 8.0
            maps[i, j, y, min(x + 1, mw - 1)] += 8.0 * float(side[i, j, 0])
            maps[i, j, min(y + 1, mh - 1), x] += 8.0 * float(side[i, j, 1])
    return maps


def test_restatement_against_the_replica_within_the_bound():
    """Largest deviation seen on the CPU (torch 2.10): values 9.5e-6 against the bound 1.69e-3 at max|x| = 12.6 (the bound is dominated
    by its weight term, which assumes the worst slope on every tap); 4 of 408 (roi, keypoint) pairs excluded, the cap being 8."""
    g = torch.Generator().manual_seed(9820)
    r, k = 24, 17
    xy0 = torch.rand((r, 2), generator=g) * 300 - 20
    size = torch.rand((r, 2), generator=g) * 270 + 30
    rois = torch.cat([xy0, xy0 + size], 1)
    rois[0] = torch.tensor([3.0, 5.0, 59.0, 61.0])      # identity
    rois[1] = torch.tensor([-7.5, 2.25, 12.5, 35.25])   # downsampling, negative offset
    rois[2] = torch.tensor([10.0, 10.0, 9.0, 50.0])     # inverted: the width clamps to 1
    rois[3] = torch.tensor([0.0, 0.0, 130.6, 199.2])    # fractional: ceil
    maps = _bump_maps(9821, r, k, 56, 56)
    want_xy, want_scores = KR.heatmaps_to_keypoints(maps, rois)
    got_xy, got_scores, roi_maps = KR.keypoints(maps.numpy(), rois.numpy(), with_maps=True)
    bound = KR.bicubic_bound(56, 56, float(maps.abs().max()))
    worst, excluded = 0.0, 0
    for i in range(r):
        _, _, _, rw, rh = KR.roi_geometry(rois[i].numpy())
        theirs = torch.nn.functional.interpolate(maps[i][:, None], size=(rh, rw), mode="bicubic", align_corners=False)[:, 0].numpy()
        worst = max(worst, float(np.abs(roi_maps[i].astype(np.float64) - theirs).max()))
        top2 = np.sort(theirs.reshape(k, -1), axis=1)[:, -2:] if rw * rh > 1 else np.stack([np.full(k, -np.inf), theirs.reshape(k)], 1)
        for j in range(k):
            if float(top2[j, 1]) - float(top2[j, 0]) > 2 * bound:
                np.testing.assert_array_equal(got_xy[i, j], want_xy[i, j].numpy(), err_msg=f"roi {i} keypoint {j}")
            else:
                excluded += 1
    print(f"bicubic: worst |restatement - torch| = {worst:.3e}, bound {bound:.3e}; excluded {excluded} of {r * k}")
    assert worst <= bound, (worst, bound)
    assert float(np.abs(got_scores - want_scores.numpy()).max()) <= bound
    assert excluded <= 0.02 * r * k, (excluded, r * k)
    assert (got_xy[..., 2] == 1).all() and got_xy.shape == (r, k, 3) and got_scores.shape == (r, k)


def test_restatement_domain_and_first_maximum():
    maps = np.zeros((4, 2, 4, 7), np.float32)
    maps[:, 1] = 2.5  # a constant plane: the first index wins
    maps[0, 0, 1, 2] = maps[0, 0, 3, 5] = 9.0
    rois = np.array([[2.0, 3.0, 9.0, 7.0], [np.nan, 0.0, 5.0, 5.0], [0.0, 0.0, 40000.0, 5.0], [0.0, -np.inf, 5.0, 5.0]], np.float32)
    xy, scores = KR.keypoints(maps, rois)
    assert not xy[1:].any() and not scores[1:].any(), "rois outside the domain give zero rows"
    np.testing.assert_array_equal(xy[0, 0], np.array([2.0 + 2.5, 3.0 + 1.5, 1.0], np.float32))  # 7 x 4 -> 7 x 4: the identity
    np.testing.assert_array_equal(xy[0, 1], np.array([2.5, 3.5, 1.0], np.float32))
    assert scores[0, 0] == 9.0 and scores[0, 1] == 2.5
    edge = np.array([[0.0, 0.0, 32768.0, 1.0]], np.float32)
    assert KR.roi_geometry(edge[0])[0] and not KR.roi_geometry(np.array([0.0, 0.0, 32768.5, 1.0], np.float32))[0]


# ---- the C entries: refusals with host pointers --------------------------------------------------------------------------------------------------
def test_heatmaps_to_keypoints_refusals_write_nothing():
    lib = _lib.load()
    maps, rois = np.zeros((2, 3, 4, 5), np.float32), np.zeros((2, 4), np.float32)
    xy, sc = np.full((2, 3, 3), SENT, np.float32), np.full((2, 3), SENT, np.float32)
    mp, rp, xp, sp = maps.ctypes.data, rois.ctypes.data, xy.ctypes.data, sc.ctypes.data

    def call(**o):
        a = {**dict(maps=mp, rois=rp, xy=xp, sc=sp, r=2, k=3, mh=4, mw=5), **o}
        return lib.mv_heatmaps_to_keypoints_f32(a["maps"], a["rois"], a["xy"], a["sc"], a["r"], a["k"], a["mh"], a["mw"], None)
    cases = [(dict(maps=None), INVALID, "null pointer"), (dict(rois=None), INVALID, "null pointer"), (dict(xy=None), INVALID, "null pointer"),
             (dict(sc=None), INVALID, "null pointer"), (dict(k=0), INVALID, "bad shape"), (dict(mh=0), INVALID, "bad shape"),
             (dict(mw=-1), INVALID, "bad shape"), (dict(r=-1), INVALID, "bad shape"), (dict(mh=129, mw=128), UNSUPPORTED, "exceed 16384 elements"),
             (dict(xy=mp), INVALID, "must not overlap"), (dict(sc=rp + 16), INVALID, "must not overlap"), (dict(sc=xp + 8), INVALID, "must not overlap"),
             (dict(maps=xp + 4 * 17), INVALID, "must not overlap"), (dict(r=2 ** 45), INVALID, "exceed the address space"),
             (dict(r=2 ** 31, k=1, mh=1, mw=1, xy=xp + 2 ** 50, sc=sp + 2 ** 52), INVALID, "exceed the launch grid")]
    for over, status, text in cases:
        rc = call(**over)
        assert rc == status and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    assert call(r=0, maps=None, rois=None, xy=None, sc=None) == 0
    assert call(r=0, k=0) == INVALID and call(mh=128, mw=128, maps=None) == INVALID  # 16384 elements pass the size check
    assert bool((xy == SENT).all()) and bool((sc == SENT).all()) and not maps.any() and not rois.any(), "a refused call wrote"


def test_conv_transpose4x4s2_refusals_write_nothing():
    lib = _lib.load()
    x, w2, b4 = np.zeros((2, 3, 4, 5), np.float32), np.zeros((8, 3, 2, 2), np.float32), np.zeros(8, np.float32)
    y = np.full((2, 2, 8, 10), SENT, np.float32)
    xp, wp, bp, yp = x.ctypes.data, w2.ctypes.data, b4.ctypes.data, y.ctypes.data

    def call(**o):
        a = {**dict(x=xp, w=wp, b=bp, y=yp, n=2, cin=3, h=4, wd=5, cout=2, act=1), **o}
        return lib.mv_conv_transpose4x4s2_bias_act_f32(a["x"], a["w"], a["b"], a["y"], a["n"], a["cin"], a["h"], a["wd"], a["cout"], a["act"], None)
    cases = [(dict(x=None), INVALID, "null pointer"), (dict(w=None), INVALID, "null pointer"), (dict(y=None), INVALID, "null pointer"),
             (dict(n=-1), INVALID, "bad shape"), (dict(cin=0), INVALID, "bad shape"), (dict(cout=0), INVALID, "bad shape"), (dict(h=0), INVALID, "bad shape"),
             (dict(wd=-1), INVALID, "bad shape"), (dict(act=3), INVALID, "bad activation code"), (dict(act=-1), INVALID, "bad activation code"),
             (dict(cout=2 ** 30), UNSUPPORTED, "index range"), (dict(cin=16384), UNSUPPORTED, "index range"), (dict(wd=4095), UNSUPPORTED, "index range"),
             (dict(h=1023, wd=1023), UNSUPPORTED, "index range"), (dict(n=65536), UNSUPPORTED, "index range"),
             (dict(y=xp), INVALID, "must not overlap"), (dict(y=wp + 32), INVALID, "must not overlap"), (dict(y=bp), INVALID, "must not overlap"),
             (dict(x=yp + 4 * 319), INVALID, "must not overlap")]
    for over, status, text in cases:
        rc = call(**over)
        assert rc == status and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    assert call(n=0, x=None, w=None, y=None, b=None) == 0
    assert bool((y == SENT).all()), "a refused call wrote"


# ---- the Python checks fire before a device is needed ----------------------------------------------------------------------------------------
def test_functional_checks_and_messages():
    maps, rois = torch.zeros(3, 2, 8, 8), torch.zeros(3, 4)
    with pytest.raises(ValueError, match=r"shape \[R, K, Mh, Mw\]"):
        F.heatmaps_to_keypoints(torch.zeros(3, 8, 8), rois)
    with pytest.raises(ValueError, match=r"shape \[3, 4\]"):
        F.heatmaps_to_keypoints(maps, torch.zeros(2, 4))
    with pytest.raises(TypeError, match="float32"):
        F.heatmaps_to_keypoints(maps.double(), rois)
    with pytest.raises(TypeError, match="float32"):
        F.heatmaps_to_keypoints(maps, rois.to(torch.int64))
    with pytest.raises(ValueError, match="should be positive"):
        F.heatmaps_to_keypoints(torch.zeros(3, 0, 8, 8), rois)
    with pytest.raises(NotImplementedError, match="16384 elements"):
        F.heatmaps_to_keypoints(torch.zeros(3, 1, 129, 128), rois)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.heatmaps_to_keypoints(maps, rois)
    x, w = torch.zeros(1, 4, 6, 6), torch.zeros(4, 3, 4, 4)
    for kw, name in ((dict(padding=1, stride=1), "stride"), (dict(padding=0), "padding"), (dict(), "padding"), (dict(padding=(1, 0)), "padding"),
                     (dict(padding=1, output_padding=1), "output_padding"), (dict(padding=1, groups=2), "groups"),
                     (dict(padding=1, dilation=2), "dilation"), (dict(padding=1, activation="silu"), "activation")):
        with pytest.raises(NotImplementedError, match=name):
            F.conv_transpose2d_bias_act(x, w, None, **kw)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        F.conv_transpose2d_bias_act(x, torch.zeros(4, 3, 4, 2))
    with pytest.raises(RuntimeError, match="does not fit 4 input channels"):
        F.conv_transpose2d_bias_act(x, torch.zeros(5, 3, 4, 4), padding=1)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.conv_transpose2d_bias_act(x, w, None, padding=1)
    assert F.heatmaps_to_keypoints is mv.functional.heatmaps_to_keypoints and "mv_heatmaps_to_keypoints_f32" in _lib.SYMBOLS
