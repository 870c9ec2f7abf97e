"""FCOS without a GPU: the module tree, state and seeded initialisation against the replica of tests/_fcos_ref.py, defaults and
argument errors, the paths that are not built, the refusals of mv_group_norm_act_f32 / mv_fcos_topk_f32 / mv_fcos_decode_f32 with
host pointers (refusals come before any launch), the Python-side checks, the GroupNorm restatement against torch's GroupNorm and
the two references of tests/_fcos_ref.py against each other."""
import math
from functools import partial

import numpy as np
import pytest
import torch

import cpu_vision_amd as mv
from cpu_vision_amd import _lib, fcos
from cpu_vision_amd import functional as F
from tests import _fcos_ref as R
from tests import _fpn_ref as PF
from tests import _rpn_ref as P
from tests._util import c_i64s as _i64s, c_ints as _ints, c_ptrs as _ptrs

INVALID, UNSUPPORTED = -1, -2
SENT = -7.25


def _equal_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k
    a.load_state_dict(sb, strict=True)
    b.load_state_dict(sa, strict=True)


def _seeded(make_lib, make_ref, seed):
    torch.manual_seed(seed)
    lib = make_lib()
    after = torch.rand(1)
    torch.manual_seed(seed)
    ref = make_ref()
    assert torch.equal(after, torch.rand(1)), "the constructor leaves the RNG where the reference leaves it"
    _equal_state(lib, ref)
    return lib, ref


# ---- module tree, state, seeded initialisation ------------------------------------------------------------------------------------------
def _tower_keys(num_convs=4):
    return [f"conv.{3 * i + j}.{t}" for i in range(num_convs) for j in (0, 1) for t in ("weight", "bias")]


def test_classification_head_equals_the_replica():
    head, _ = _seeded(lambda: mv.FCOSClassificationHead(64, 1, 5), lambda: R.FCOSClassificationHead(64, 1, 5), 41)
    assert list(head.state_dict()) == _tower_keys() + ["cls_logits.weight", "cls_logits.bias"]
    assert [type(m).__name__ for m in head.conv] == ["Conv2d", "GroupNorm", "ReLU"] * 4
    assert head.conv[1].num_groups == 32 and head.conv[1].eps == 1e-5 and head.conv[1].affine
    assert head.num_classes == 5 and head.num_anchors == 1 and not head.training
    assert torch.equal(head.cls_logits.bias, torch.full((5,), -math.log(99.0)))
    other, _ = _seeded(lambda: mv.FCOSClassificationHead(8, 1, 3, num_convs=2, prior_probability=0.25, norm_layer=partial(torch.nn.GroupNorm, 4)),
                       lambda: R.FCOSClassificationHead(8, 1, 3, num_convs=2, prior_probability=0.25, norm_layer=partial(torch.nn.GroupNorm, 4)), 42)
    assert list(other.state_dict()) == _tower_keys(2) + ["cls_logits.weight", "cls_logits.bias"]
    assert torch.equal(other.cls_logits.bias, torch.full((3,), -math.log(3.0)))


def test_regression_head_equals_the_replica():
    head, _ = _seeded(lambda: mv.FCOSRegressionHead(64, 1), lambda: R.FCOSRegressionHead(64, 1), 43)
    assert list(head.state_dict()) == _tower_keys() + ["bbox_reg.weight", "bbox_reg.bias", "bbox_ctrness.weight", "bbox_ctrness.bias"]
    assert head.bbox_reg.weight.shape == (4, 64, 3, 3) and head.bbox_ctrness.weight.shape == (1, 64, 3, 3)
    assert bool((head.bbox_reg.bias == 0).all()) and bool((head.bbox_ctrness.bias == 0).all())
    # the predictors are initialised BEFORE the tower: with one seed the classification head's tower differs
    torch.manual_seed(43)
    c = mv.FCOSClassificationHead(64, 1, 5)
    assert not torch.equal(c.conv[0].weight, head.conv[0].weight)


def test_head_equals_the_replica():
    head, _ = _seeded(lambda: mv.FCOSHead(32, 1, 5), lambda: R.FCOSHead(32, 1, 5), 44)
    assert [n for n, _ in head.named_children()] == ["classification_head", "regression_head"]
    assert head.box_coder.normalize_by_size is True
    two, _ = _seeded(lambda: mv.FCOSHead(32, 1, 5, num_convs=2), lambda: R.FCOSHead(32, 1, 5, num_convs=2), 45)
    assert len(two.classification_head.conv) == 6 and len(two.regression_head.conv) == 6


def _backbones():
    kw = dict(backbone_name="resnet18", returned_layers=[2, 3, 4])
    return (lambda: mv.resnet_fpn_backbone(extra_blocks=mv.LastLevelP6P7(256, 256), **kw),
            lambda: PF.resnet_fpn_backbone(extra_blocks=PF.LastLevelP6P7(256, 256), **kw))


def test_fcos_on_a_resnet18_fpn_equals_the_replica():
    lib_bb, ref_bb = _backbones()
    model, ref = _seeded(lambda: mv.FCOS(lib_bb(), 5), lambda: R.FCOS(ref_bb(), 5), 46)
    assert [n for n, _ in model.named_children()] == ["backbone", "anchor_generator", "head", "transform"]
    assert not model.training
    assert (model.score_thresh, model.nms_thresh, model.detections_per_img, model.topk_candidates, model.center_sampling_radius) == \
        (0.2, 0.6, 100, 1000, 1.5)
    assert model.box_coder.normalize_by_size is True
    assert model.transform.image_mean == [0.485, 0.456, 0.406] and model.transform.image_std == [0.229, 0.224, 0.225]
    assert model.transform.min_size == (800,) and model.transform.max_size == 1333
    ag = model.anchor_generator
    assert ag.sizes == ((8,), (16,), (32,), (64,), (128,)) and ag.aspect_ratios == ((1.0,),) * 5 and ag.num_anchors_per_location() == [1] * 5
    assert all(torch.equal(a, b) for a, b in zip(ag.cell_anchors, R.default_anchorgen().cell_anchors))
    assert "head.classification_head.conv.9.weight" in model.state_dict() and "head.regression_head.bbox_ctrness.bias" in model.state_dict()


def test_fcos_resnet50_fpn_builder():
    torch.manual_seed(47)
    model = mv.fcos_resnet50_fpn()
    after = torch.rand(1)
    torch.manual_seed(47)
    ref = R.FCOS(PF._resnet_fpn_extractor(PF.R.resnet50(norm_layer=PF.FrozenBatchNorm2d), 3, returned_layers=[2, 3, 4],
                                          extra_blocks=PF.LastLevelP6P7(256, 256)), 91)
    assert torch.equal(after, torch.rand(1))
    _equal_state(model, ref)
    assert model.head.classification_head.cls_logits.out_channels == 91 and model.backbone.out_channels == 256
    assert isinstance(model.backbone.fpn.extra_blocks, mv.LastLevelP6P7) and list(model.backbone.body.keys())[-1] == "layer4"
    assert mv.fcos_resnet50_fpn(num_classes=7, topk_candidates=50).head.classification_head.num_classes == 7
    for kw in (dict(weights="DEFAULT"), dict(weights_backbone="IMAGENET1K_V1")):
        with pytest.raises(ValueError, match="ships no weight files"):
            mv.fcos_resnet50_fpn(**kw)
    assert mv.fcos.FCOS is mv.FCOS and F.fcos_topk is mv.functional.fcos_topk and F.group_norm_act is mv.functional.group_norm_act


# ---- argument errors, inference only ----------------------------------------------------------------------------------------------------
def test_argument_errors():
    lib_bb, _ = _backbones()
    with pytest.raises(ValueError, match="backbone should contain an attribute out_channels"):
        mv.FCOS(torch.nn.Identity(), 5)
    with pytest.raises(TypeError, match="anchor_generator should be of type AnchorGenerator or None instead of <class 'int'>"):
        mv.FCOS(lib_bb(), 5, anchor_generator=3)
    with pytest.raises(ValueError, match=r"anchor_generator.num_anchors_per_location\(\)\[0\] should be 1 instead of 3"):
        mv.FCOS(lib_bb(), 5, anchor_generator=mv.AnchorGenerator(((8,),) * 5, ((0.5, 1.0, 2.0),) * 5))
    with pytest.raises(ValueError, match="selects up to 4096 candidates per level, got topk_candidates=5000"):
        mv.FCOS(lib_bb(), 5, topk_candidates=5000)
    for make in (lambda n: mv.FCOSClassificationHead(8, 1, 4, norm_layer=n), lambda n: mv.FCOSRegressionHead(8, 1, norm_layer=n)):
        with pytest.raises(NotImplementedError, match="nn.GroupNorm towers only, norm_layer made BatchNorm2d"):
            make(torch.nn.BatchNorm2d)
        with pytest.raises(ValueError, match="must be divisible by num_groups"):
            make(partial(torch.nn.GroupNorm, 3))  # nn.GroupNorm's own
        assert not make(partial(torch.nn.GroupNorm, 2, affine=False)).conv[1].affine


def test_inference_only():
    lib_bb, _ = _backbones()
    model = mv.FCOS(lib_bb(), 5)
    imgs = [torch.zeros(3, 32, 32)]
    with pytest.raises(RuntimeError, match="inference only"):
        model(imgs, [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64)}])
    model.train()
    with pytest.raises(RuntimeError, match="inference only"):
        model(imgs)
    feats = [torch.zeros(1, 32, 4, 4)]
    for head in (mv.FCOSHead(32, 1, 3), mv.FCOSClassificationHead(32, 1, 3), mv.FCOSRegressionHead(32, 1)):
        with pytest.raises(RuntimeError, match="inference only"):
            head.train()(feats)
        with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
            head.eval()(feats)


# ---- the C ABI refuses before any launch ------------------------------------------------------------------------------------------------
class _Gn:
    """mv_group_norm_act_f32 on host buffers: x (2, 6, 5, 7), 3 groups, one chunk per slab -> a workspace of 2 * 3 * 16 bytes."""

    def __init__(self):
        self.x, self.y = np.zeros(2 * 210 + 8, np.float32), np.full(2 * 210 + 8, SENT, np.float32)
        self.w, self.b = np.ones(6, np.float32), np.zeros(6, np.float32)
        self.ws = np.full(96 // 8 + 4, SENT, np.float64)
        self.ws_ptr = (self.ws.ctypes.data + 15) // 16 * 16
        self.kw = dict(x=self.x.ctypes.data, y=self.y.ctypes.data, w=self.w.ctypes.data, b=self.b.ctypes.data, n=2, c=6, h=5, wd=7, g=3, xs=210,
                       ys=210, eps=1e-5, relu=1, wsp=self.ws_ptr, nbytes=96)

    def call(self, **over):
        a = {**self.kw, **over}
        lib = _lib.load()
        rc = lib.mv_group_norm_act_f32(a["x"], a["y"], a["w"], a["b"], a["n"], a["c"], a["h"], a["wd"], a["g"], a["xs"], a["ys"], a["eps"], a["relu"],
                                       a["wsp"], a["nbytes"], None)
        assert bool((self.y == SENT).all()) and bool((self.ws == SENT).all()), "a refused call wrote"
        return rc, lib.mv_last_error().decode()


def test_group_norm_workspace_and_chunk():
    lib = _lib.load()
    chunk = lib.mv_group_norm_chunk()
    assert chunk == F.group_norm_chunk() == R.GN_CHUNK
    bytes_ = lambda n, c, h, w, g: int(lib.mv_group_norm_workspace_bytes(n, c, h, w, g))  # noqa: E731
    assert bytes_(2, 6, 5, 7, 3) == 2 * 3 * 16
    assert bytes_(1, 2, 1, chunk, 2) == 2 * 16 and bytes_(1, 2, 1, chunk + 1, 2) == 4 * 16 and bytes_(1, 2, 1, 2 * chunk - 1, 1) == 4 * 16
    assert bytes_(1, 256, 100, 168, 32) == 32 * 33 * 16  # P3 of 800 x 1344: 134 400 elements per group
    assert bytes_(1, 6, 5, 7, 4) == 0 and bytes_(1, 6, 5, 7, 0) == 0 and bytes_(0, 6, 5, 7, 3) == 0 and bytes_(-1, 6, 5, 7, 3) == 0


def test_group_norm_refusals():
    t = _Gn()
    big = 1 << 15
    cases = [
        (dict(g=4), INVALID, "6 channels are not divisible by 4 groups"),
        (dict(g=0), INVALID, "groups must be positive"),
        (dict(g=-3), INVALID, "groups must be positive"),
        (dict(eps=0.0), INVALID, "eps must be positive"),
        (dict(eps=-1e-5), INVALID, "eps must be positive"),
        (dict(eps=float("nan")), INVALID, "eps must be positive"),
        (dict(eps=float("inf")), INVALID, "eps must be positive"),
        (dict(eps=1e-60), INVALID, "eps must be positive"),  # 0 as a float32
        (dict(n=-1), INVALID, "negative size"),
        (dict(h=-5), INVALID, "negative size"),
        (dict(c=2, g=1, h=big, wd=big), UNSUPPORTED, "32-bit index"),
        (dict(xs=209), INVALID, "image strides"),
        (dict(ys=209), INVALID, "image strides"),
        (dict(x=None), INVALID, "null pointer"),
        (dict(y=None), INVALID, "null pointer"),
        (dict(x=t.x.ctypes.data + 2), INVALID, "4-byte aligned"),
        (dict(y=t.x.ctypes.data + 4), INVALID, "y must be x itself"),          # a partial overlap
        (dict(y=t.x.ctypes.data, ys=214), INVALID, "y must be x itself"),      # the same pointer, another stride
        (dict(wsp=None), INVALID, "needs a workspace"),
        (dict(nbytes=95), INVALID, "workspace of 95 bytes, need 96"),
        (dict(wsp=t.ws_ptr + 8), INVALID, "16-byte aligned"),
        (dict(wsp=(t.x.ctypes.data + 15) // 16 * 16), INVALID, "must not overlap"),
        (dict(y=t.w.ctypes.data), INVALID, "must not overlap"),
    ]
    for over, status, text in cases:
        rc, msg = t.call(**over)
        assert rc == status and text in msg, (over, rc, msg)
    # empty work is a no-op that touches no pointer
    for over in (dict(n=0), dict(c=0, g=3), dict(h=0), dict(wd=0)):
        assert t.call(x=None, y=None, wsp=None, nbytes=0, **over)[0] == 0, over


class _Fcos:
    """The two FCOS entries on host buffers: one level (5, 7), 2 classes, one image."""

    def __init__(self):
        self.cls, self.ctr, self.reg = np.zeros(70, np.float32), np.zeros(35, np.float32), np.zeros(140, np.float32)
        self.base, self.sizes = np.zeros(4, np.float32), np.array([20.0, 28.0], np.float32)
        self.idx = np.full(4, 0x5AA5C33C, np.int32)
        self.need = int(_lib.load().mv_retinanet_topk_workspace_bytes(1, _ints(5), _ints(7), _ints(1), 1, 2, 4))
        self.ws = np.full(self.need // 8 + 4, SENT, np.float64)
        self.ws_ptr = (self.ws.ctypes.data + 15) // 16 * 16
        self.boxes, self.scores = np.full(16, SENT, np.float32), np.full(4, SENT, np.float32)
        self.labels, self.valid = np.full(4, 0x5AA5C33C, np.int64), np.full(4, 0xA5, np.uint8)
        self.kw = dict(cls=_ptrs(self.cls), ctr=_ptrs(self.ctr), reg=_ptrs(self.reg), hs=_ints(5), ws=_ints(7), as_=_ints(1), ls=_i64s(70),
                       cs=_i64s(35), ds=_i64s(140), sh=_ints(4), sw=_ints(4), levels=1, classes=2, n=1, k=4, idx=self.idx.ctypes.data,
                       wsp=self.ws_ptr, nbytes=self.need, base=self.base.ctypes.data, sizes=self.sizes.ctypes.data,
                       boxes=self.boxes.ctypes.data, scores=self.scores.ctypes.data, lb=self.labels.ctypes.data, valid=self.valid.ctypes.data)

    def _clean(self):
        assert bool((self.idx == 0x5AA5C33C).all()) and bool((self.ws == SENT).all()) and bool((self.boxes == SENT).all()) and \
            bool((self.scores == SENT).all()) and bool((self.labels == 0x5AA5C33C).all()) and bool((self.valid == 0xA5).all()), "a refused call wrote"

    def topk(self, **over):
        a = {**self.kw, **over}
        lib = _lib.load()
        rc = lib.mv_fcos_topk_f32(a["cls"], a["ctr"], a["hs"], a["ws"], a["as_"], a["ls"], a["cs"], a["levels"], a["classes"], a["n"], a["k"], 0.2,
                                  a["idx"], a["wsp"], a["nbytes"], None)
        self._clean()
        return rc, lib.mv_last_error().decode()

    def decode(self, **over):
        a = {**self.kw, **over}
        lib = _lib.load()
        rc = lib.mv_fcos_decode_f32(a["cls"], a["ctr"], a["reg"], a["hs"], a["ws"], a["as_"], a["ls"], a["cs"], a["ds"], a["sh"], a["sw"], a["levels"],
                                    a["classes"], a["base"], a["sizes"], a["idx"], a["n"], a["k"], a["boxes"], a["scores"], a["lb"], a["valid"],
                                    None)
        self._clean()
        return rc, lib.mv_last_error().decode()


def test_fcos_entries_refuse_as_retinanets_and_check_the_centerness():
    t = _Fcos()
    shared = [
        (dict(cls=None), INVALID, "null pointer"),
        (dict(ctr=None), INVALID, "null pointer"),
        (dict(cs=None), INVALID, "null pointer"),
        (dict(ctr=_ptrs(None)), INVALID, "null pointer (level 0)"),
        (dict(as_=_ints(3)), INVALID, "one anchor per location, level 0 has 3"),
        (dict(cs=_i64s(34)), INVALID, "image stride 34 of the centerness of level 0, its map has 35 elements"),
        (dict(levels=0), INVALID, "1 to 8 levels"),
        (dict(levels=9), UNSUPPORTED, "1 to 8 levels"),
        (dict(hs=_ints(0)), INVALID, "bad shape"),
        (dict(classes=0), INVALID, "classes must be positive"),
        (dict(hs=_ints(1 << 10), ws=_ints(1 << 10), classes=1 << 11), UNSUPPORTED, "32-bit index"),
    ]
    topk = shared + [
        (dict(k=0), INVALID, "k must be positive"),
        (dict(k=4097), UNSUPPORTED, "k up to 4096"),
        (dict(n=-1), INVALID, "bad image count"),
        (dict(ls=_i64s(69)), INVALID, "image stride"),
        (dict(wsp=None), INVALID, "needs a workspace"),
        (dict(nbytes=t.need - 1), INVALID, f"workspace of {t.need - 1} bytes, need {t.need}"),
        (dict(wsp=t.ws_ptr + 4), INVALID, "16-byte aligned"),
        (dict(idx=t.ctr.ctypes.data + 8), INVALID, "must not overlap"),  # idx on the centerness map
        (dict(wsp=(t.ctr.ctypes.data + 15) // 16 * 16, nbytes=t.need), INVALID, "must not overlap"),
    ]
    for over, status, text in topk:
        rc, msg = t.topk(**over)
        assert rc == status and text in msg and msg.startswith("fcos_topk:"), (list(over), rc, msg)
    assert t.topk(n=0, cls=None, ctr=None, idx=None, wsp=None, nbytes=0)[0] == 0
    decode = shared + [
        (dict(reg=None), INVALID, "null pointer"),
        (dict(sh=_ints(-4)), INVALID, "bad strides"),
        (dict(k=-1), INVALID, "bad shape"),
        (dict(ds=_i64s(139)), INVALID, "image strides"),
        (dict(lb=t.labels.ctypes.data + 4), INVALID, "8-byte aligned"),
        (dict(boxes=t.ctr.ctypes.data), INVALID, "must not overlap"),  # an output on the centerness map
        (dict(scores=t.reg.ctypes.data), INVALID, "must not overlap"),
        (dict(valid=None), INVALID, "null pointer"),
    ]
    for over, status, text in decode:
        rc, msg = t.decode(**over)
        assert rc == status and text in msg and msg.startswith("fcos_decode:"), (list(over), rc, msg)
    assert t.decode(n=0, cls=None, boxes=None)[0] == 0 and t.decode(k=0, idx=None, boxes=None, scores=None, lb=None, valid=None)[0] == 0


# ---- the Python checks fire before a device is needed ---------------------------------------------------------------------------------
def test_functional_checks_and_messages():
    x = torch.zeros(2, 6, 5, 7)
    with pytest.raises(RuntimeError, match="4-D tensor"):
        F.group_norm_act(x[0], 3)
    with pytest.raises(TypeError, match="float32"):
        F.group_norm_act(x.double(), 3)
    with pytest.raises(ValueError, match="num_groups must be a positive int"):
        F.group_norm_act(x, 0)
    with pytest.raises(RuntimeError, match="divisible by num_groups"):
        F.group_norm_act(x, 4)
    with pytest.raises(RuntimeError, match=r"weight should have shape \(6,\)"):
        F.group_norm_act(x, 3, torch.ones(5))
    with pytest.raises(TypeError, match="bias torch.float64"):
        F.group_norm_act(x, 3, None, torch.ones(6).double())
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps must be positive and finite"):
            F.group_norm_act(x, 3, eps=eps)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.group_norm_act(x, 3)
    g = torch.Generator().manual_seed(48)
    grids = ((4, 6), (2, 3))
    cl = [torch.randn((2, 3, h, w), generator=g) for h, w in grids]
    ct = [torch.randn((2, 1, h, w), generator=g) for h, w in grids]
    rg = [torch.randn((2, 4, h, w), generator=g) for h, w in grids]
    with pytest.raises(RuntimeError, match="one anchor per location"):
        F.fcos_topk([torch.zeros(2, 6, 4, 6)], [ct[0]], 3, 4, 0.2)
    with pytest.raises(RuntimeError, match="ctrness should hold one map per level"):
        F.fcos_topk(cl, ct[:1], 3, 4, 0.2)
    with pytest.raises(RuntimeError, match="ctrness should hold one map per level"):
        F.fcos_topk(cl, [c[:1] for c in ct], 3, 4, 0.2)  # another batch
    with pytest.raises(RuntimeError, match="ctrness should hold one map per level"):
        F.fcos_topk(cl, [ct[0], torch.zeros(2, 2, 2, 3)], 3, 4, 0.2)  # two channels
    with pytest.raises(ValueError, match="k must be a positive int"):
        F.fcos_topk(cl, ct, 3, 0, 0.2)
    with pytest.raises(_lib.Mi355VisionError, match="k up to 4096"):
        F.fcos_topk(cl, ct, 3, 4097, 0.2)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.fcos_topk(cl, ct, 3, 4, 0.2)
    idx = torch.zeros((2, 8), dtype=torch.int32)
    cells, strides, sizes = [torch.zeros(1, 4)] * 2, [(4, 4), (8, 8)], [(16, 24), (15, 20)]
    with pytest.raises(RuntimeError, match="bbox_regression should hold one map per level"):
        F.fcos_decode(cl, ct, rg[:1], idx, cells, strides, sizes, 3)
    with pytest.raises(RuntimeError, match="int32 tensor of shape"):
        F.fcos_decode(cl, ct, rg, idx.long(), cells, strides, sizes, 3)
    with pytest.raises(RuntimeError, match="cell_anchors should hold one"):
        F.fcos_decode(cl, ct, rg, idx, [torch.zeros(3, 4)] * 2, strides, sizes, 3)
    with pytest.raises(RuntimeError, match="strides should hold"):
        F.fcos_decode(cl, ct, rg, idx, cells, [(4, 4), (-1, 8)], sizes, 3)
    with pytest.raises(RuntimeError, match="image_sizes should hold 2 rows"):
        F.fcos_decode(cl, ct, rg, idx, cells, strides, sizes[:1], 3)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.fcos_decode(cl, ct, rg, idx, cells, strides, sizes, 3)


# ---- the GroupNorm restatement against torch ------------------------------------------------------------------------------------------
GN_INPUTS = [((2, 256, 13, 17), 32, 0.0, 1.0), ((1, 256, 100, 168), 32, 0.3, 2.0), ((2, 6, 5, 7), 3, 1000.0, 1.0), ((1, 8, 3, 3), 2, -5.0, 0.01)]


@pytest.mark.parametrize("case", range(4))
def test_group_norm_restatement_is_as_close_to_float64_as_torch(case):
    """max|restatement - f64| <= 2 max|torch float32 - f64| + 2^-22 max|f64| on the four inputs of DESIGN.md 3.30, torch's GroupNorm in
    float64 the reference: five float32 roundings of the stated chain against torch's different but equally long chain."""
    shape, groups, mu, sd = GN_INPUTS[case]
    g = torch.Generator().manual_seed(100 + case)
    x = torch.randn(shape, generator=g) * sd + mu
    w, b = torch.randn(shape[1], generator=g), torch.randn(shape[1], generator=g)
    got = R.group_norm(x, groups, w, b, 1e-5)
    f32 = torch.nn.functional.group_norm(x, groups, w, b, 1e-5)
    f64 = torch.nn.functional.group_norm(x.double(), groups, w.double(), b.double(), 1e-5)
    scale = float(f64.abs().max())
    err, err32 = float((got.double() - f64).abs().max()), float((f32.double() - f64).abs().max())
    print(f"{shape} G {groups} N({mu}, {sd}): restatement {err / scale:.3g}, torch float32 {err32 / scale:.3g} of max|f64|")
    assert err <= 2 * err32 + 2.0 ** -22 * scale
    # the ReLU and the absence of the affine parameters
    plain = R.group_norm(x, groups, None, None, 1e-5, relu=True)
    f64 = torch.relu(torch.nn.functional.group_norm(x.double(), groups, None, None, 1e-5))
    f32 = torch.relu(torch.nn.functional.group_norm(x, groups, None, None, 1e-5))
    assert float((plain.double() - f64).abs().max()) <= 2 * float((f32.double() - f64).abs().max()) + 2.0 ** -22 * float(f64.abs().max())
    assert float(plain.min()) == 0


def test_group_norm_restatement_sums_in_the_stated_order():
    """The stated order on a slab of two chunks - 1 elements against a literal loop over threads, lanes and chunks."""
    c = R.GN_CHUNK
    g = torch.Generator().manual_seed(49)
    slab = (torch.randn(2 * c - 1, generator=g) * 3 + 1).numpy()
    S, S2 = R.group_sums(slab[None])
    total, total2 = 0.0, 0.0
    for ch in range(2):
        part = np.zeros(c)
        seg = slab[ch * c:(ch + 1) * c]
        part[:seg.size] = seg
        lanes = []
        for t in range(256):
            s = s2 = np.float64(0)
            for u in range(4):
                for q in range(4):
                    d = np.float64(part[1024 * u + 4 * t + q])
                    s, s2 = s + d, s2 + d * d
            lanes.append((s, s2))
        waves = []
        for v in range(4):
            a = list(lanes[64 * v:64 * v + 64])
            for mask in (32, 16, 8, 4, 2, 1):
                a = [(a[l][0] + a[l ^ mask][0], a[l][1] + a[l ^ mask][1]) for l in range(64)]
            waves.append(a[0])
        cs, cs2 = waves[0]
        for v in range(1, 4):
            cs, cs2 = cs + waves[v][0], cs2 + waves[v][1]
        total, total2 = total + cs, total2 + cs2
    assert S[0] == total and S2[0] == total2


# ---- replica (a) against restatement (b) ------------------------------------------------------------------------------------------------
GRIDS = ((8, 10), (4, 5), (2, 3))
K, THRESH, TOPK = 4, 0.3, 60


def test_replica_and_restatement_select_and_decode_alike():
    """Random maps: the index sets of the replica's torch ops and of the restatement are equal but for candidates whose restated score
    lies within 2 ulp of the threshold or of the level's k-th score (at most 1 % are set aside, asserted); the boxes of the common
    candidates are equal bit for bit (the linear decode has no transcendental), their scores within 2 ulp."""
    g = torch.Generator().manual_seed(51)
    cls_maps = [torch.randn((2, K, h, w), generator=g) * 2 for h, w in GRIDS]
    ctr_maps = [torch.randn((2, 1, h, w), generator=g) for h, w in GRIDS]
    reg_maps = [torch.relu(torch.randn((2, 4, h, w), generator=g) * 1.5) for h, w in GRIDS]

    def make(numerics):
        ag = P.AnchorGenerator(((8,), (16,), (32,)), ((1.0,),) * 3)
        bb = torch.nn.Identity()
        bb.out_channels = 32
        return R.FCOS(bb, K, anchor_generator=ag, score_thresh=THRESH, topk_candidates=TOPK, detections_per_img=30, numerics=numerics).eval()
    images = P.ImageList(torch.zeros(2, 3, 64, 80), [(64, 80), (60, 75)])
    (det_a, cand_a), (det_b, cand_b) = (make(n).from_head_maps(images, cls_maps, reg_maps, ctr_maps, detailed=True) for n in (P.REPLICA, P.RESTATEMENT))
    want_idx = R.select(cls_maps, ctr_maps, K, TOPK, THRESH)
    thresh = torch.tensor(THRESH, dtype=torch.float32)
    total = aside = 0
    for i in range(2):
        assert torch.equal(cand_b[i]["idx"], want_idx[i][want_idx[i] >= 0].long())
        assert len(cand_b[i]["idx"]) > TOPK, "more than one level contributes"
        # the candidates near the threshold or near the k-th score of their level, by the restated scores
        near, start = set(), 0
        for m, c in zip(cls_maps, ctr_maps):
            s = R.level_scores(m, c, K)[i]
            passing = torch.sort(s[s > thresh], descending=True)[0]
            marks = [(thresh, 0)] + ([(passing[TOPK - 1], 1)] if len(passing) > TOPK else [])
            for mark, itself in marks:  # the k-th score is a score: it is near when ANOTHER score lies within 2 ulp of it
                close = (P.ulp_distance(s, mark.expand_as(s)) <= 2).nonzero().flatten()
                if len(close) > itself:
                    near |= {int(f) + start for f in close}
            start += s.numel()
        a_set, b_set = set(cand_a[i]["idx"].tolist()), set(cand_b[i]["idx"].tolist())
        assert (a_set ^ b_set) <= near, "the two index sets differ away from the threshold and the k-th score"
        total, aside = total + len(a_set | b_set), aside + len((a_set | b_set) & near)
        common = sorted((a_set & b_set) - near)
        pos_a = {int(f): j for j, f in enumerate(cand_a[i]["idx"].tolist())}
        pos_b = {int(f): j for j, f in enumerate(cand_b[i]["idx"].tolist())}
        ja, jb = torch.tensor([pos_a[f] for f in common]), torch.tensor([pos_b[f] for f in common])
        P.same(cand_a[i]["boxes"][ja], cand_b[i]["boxes"][jb], "boxes")
        assert torch.equal(cand_a[i]["labels"][ja], cand_b[i]["labels"][jb])
        assert int(P.ulp_distance(cand_a[i]["scores"][ja], cand_b[i]["scores"][jb]).max()) <= 2
        assert 0 < len(det_b[i]["boxes"]) <= 30
    assert aside <= 0.01 * total, f"{aside} of {total} candidates set aside"
    # the fixed-shape form the kernels write agrees with the per-image form
    anchors = make(P.RESTATEMENT).anchor_generator(images, cls_maps)
    boxes, scores, labels, valid = R.decode(cls_maps, ctr_maps, reg_maps, want_idx, anchors, images.image_sizes, K)
    for i in range(2):
        v = valid[i]
        assert torch.equal(v, want_idx[i] >= 0) and bool((~v).any())
        P.same(boxes[i][v], cand_b[i]["boxes"]), P.same(scores[i][v], cand_b[i]["scores"])
        assert torch.equal(labels[i][v], cand_b[i]["labels"])
        assert float(boxes[i][~v].abs().max()) == 0 and float(scores[i][~v].abs().max()) == 0
    # the decode rectifies: a negative distance is a zero distance
    neg = [-m for m in reg_maps]
    b_neg = R.decode(cls_maps, ctr_maps, neg, want_idx, anchors, images.image_sizes, K)[0]
    b_zero = R.decode(cls_maps, ctr_maps, [torch.zeros_like(m) for m in reg_maps], want_idx, anchors, images.image_sizes, K)[0]
    P.same(b_neg, b_zero)
