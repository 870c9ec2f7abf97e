"""RetinaNet without a GPU: the module tree, state and seeded initialisation against the replica of tests/_retinanet_ref.py, the
version-1 key renaming, defaults and argument errors, the paths that are not built, every refusal of mv_retinanet_topk_f32 /
mv_retinanet_decode_f32 with host pointers (refusals come before any launch), the Python-side checks, and the two references of
tests/_retinanet_ref.py against each other."""
import math

import numpy as np
import pytest
import torch

import cpu_vision_amd as mv
from cpu_vision_amd import _lib, retinanet
from cpu_vision_amd import functional as F
from tests import _fpn_ref as PF
from tests import _retinanet_ref as R
from tests import _rpn_ref as P
from tests import test_rpn_host as RH  # its fixtures and refusal tables, for the comparison of the two families
from tests._util import c_i64s as _i64s, c_ints as _ints, c_ptrs as _ptrs


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
def test_classification_head_equals_the_replica():
    head, _ = _seeded(lambda: mv.RetinaNetClassificationHead(16, 3, 5), lambda: R.RetinaNetClassificationHead(16, 3, 5), 21)
    keys = [f"conv.{i}.0.{t}" for i in range(4) for t in ("weight", "bias")] + ["cls_logits.weight", "cls_logits.bias"]
    assert list(head.state_dict()) == keys
    assert head.num_classes == 5 and head.num_anchors == 3 and head._version == 2 and not head.training
    assert head.cls_logits.weight.shape == (15, 16, 3, 3)
    assert torch.equal(head.cls_logits.bias, torch.full((15,), -math.log(99.0)))
    assert all(bool((head.conv[i][0].bias == 0).all()) for i in range(4))
    other = mv.RetinaNetClassificationHead(8, 2, 3, prior_probability=0.25)
    assert torch.equal(other.cls_logits.bias, torch.full((6,), -math.log(3.0)))


def test_regression_head_equals_the_replica():
    head, _ = _seeded(lambda: mv.RetinaNetRegressionHead(16, 3), lambda: R.RetinaNetRegressionHead(16, 3), 22)
    keys = [f"conv.{i}.0.{t}" for i in range(4) for t in ("weight", "bias")] + ["bbox_reg.weight", "bbox_reg.bias"]
    assert list(head.state_dict()) == keys
    assert head.bbox_reg.weight.shape == (12, 16, 3, 3) and bool((head.bbox_reg.bias == 0).all())
    assert head.box_coder.weights == (1.0, 1.0, 1.0, 1.0) and head._loss_type == "l1" and head._version == 2


def test_the_two_init_orders_differ():
    """The classification head initialises the tower and then the predictor, the regression head the predictor and then the tower:
    with one seed the towers of the two heads therefore differ, and each equals the replica's (the tests above)."""
    torch.manual_seed(5)
    c = mv.RetinaNetClassificationHead(8, 3, 4)
    torch.manual_seed(5)
    r = mv.RetinaNetRegressionHead(8, 3)
    assert not torch.equal(c.conv[0][0].weight, r.conv[0][0].weight)


def test_head_equals_the_replica():
    head, _ = _seeded(lambda: mv.RetinaNetHead(16, 3, 5), lambda: R.RetinaNetHead(16, 3, 5), 23)
    assert [n for n, _ in head.named_children()] == ["classification_head", "regression_head"]


def _backbones():
    kw = dict(backbone_name="resnet18", returned_layers=[2, 3, 4])
    return (lambda: mv.resnet_fpn_backbone(extra_blocks=mv.LastLevelP6P7(256, 256), **kw),
            lambda: PF.resnet_fpn_backbone(extra_blocks=PF.LastLevelP6P7(256, 256), **kw))


def test_retinanet_on_a_resnet18_fpn_equals_the_replica():
    lib_bb, ref_bb = _backbones()
    model, ref = _seeded(lambda: mv.RetinaNet(lib_bb(), 5), lambda: R.RetinaNet(ref_bb(), 5), 24)
    assert [n for n, _ in model.named_children()] == ["backbone", "anchor_generator", "head", "transform"]
    assert not model.training and model.proposal_matcher is None
    assert (model.score_thresh, model.nms_thresh, model.detections_per_img, model.topk_candidates) == (0.05, 0.5, 300, 1000)
    assert model.box_coder.weights == (1.0, 1.0, 1.0, 1.0) and model.box_coder.bbox_xform_clip == math.log(1000.0 / 16)
    assert model.transform.image_mean == [0.485, 0.456, 0.406] and model.transform.image_std == [0.229, 0.224, 0.225]
    assert model.transform.min_size == (800,) and model.transform.max_size == 1333
    assert model.head.classification_head.cls_logits.out_channels == 9 * 5
    assert "head.classification_head.conv.3.0.weight" in model.state_dict() and "backbone.fpn.extra_blocks.p7.weight" in model.state_dict()
    matcher = object()
    assert mv.RetinaNet(lib_bb(), 2, proposal_matcher=matcher).proposal_matcher is matcher


def test_default_anchor_sizes():
    sizes = ((32, 40, 50), (64, 80, 101), (128, 161, 203), (256, 322, 406), (512, 645, 812))
    ag = retinanet._default_anchorgen()
    assert ag.sizes == sizes and ag.aspect_ratios == ((0.5, 1.0, 2.0),) * 5 and ag.num_anchors_per_location() == [9] * 5
    ref = R.default_anchorgen()
    assert ref.sizes == sizes and all(torch.equal(a, b) for a, b in zip(ag.cell_anchors, ref.cell_anchors))
    lib_bb, _ = _backbones()
    assert mv.RetinaNet(lib_bb(), 3).anchor_generator.sizes == sizes


def test_retinanet_resnet50_fpn_builder():
    torch.manual_seed(25)
    model = mv.retinanet_resnet50_fpn()
    after = torch.rand(1)
    torch.manual_seed(25)
    ref = R.RetinaNet(PF._resnet_fpn_extractor(PF.R.resnet50(norm_layer=PF.FrozenBatchNorm2d), 3, returned_layers=[2, 3, 4],
                                               extra_blocks=PF.LastLevelP6P7(256, 256)), 91, anchor_generator=R.default_anchorgen())
    assert torch.equal(after, torch.rand(1))
    _equal_state(model, ref)
    assert model.head.classification_head.cls_logits.out_channels == 9 * 91 and model.head.classification_head.num_classes == 91
    assert list(model.backbone.body.keys())[-1] == "layer4" and model.backbone.out_channels == 256
    assert isinstance(model.backbone.fpn.extra_blocks, mv.LastLevelP6P7)
    assert mv.retinanet_resnet50_fpn(num_classes=7, topk_candidates=50).head.classification_head.num_classes == 7
    for kw in (dict(weights="DEFAULT"), dict(weights_backbone="IMAGENET1K_V1")):
        with pytest.raises(ValueError, match="ships no weight files"):
            mv.retinanet_resnet50_fpn(**kw)
    assert not hasattr(mv, "retinanet_resnet50_fpn_v2")


@pytest.mark.parametrize("cls", ["classification", "regression"])
def test_heads_load_a_version_1_state_dict(cls):
    def make(mod):
        return mod.RetinaNetClassificationHead(8, 3, 4) if cls == "classification" else mod.RetinaNetRegressionHead(8, 3)
    torch.manual_seed(3)
    src = make(mv)
    old = {}
    for k, v in src.state_dict().items():
        parts = k.split(".")
        old[f"conv.{2 * int(parts[1])}.{parts[3]}" if parts[0] == "conv" else k] = v.clone()
    assert "conv.6.weight" in old and "conv.3.0.weight" not in old
    dst, ref = make(mv), make(R)
    dst.load_state_dict(dict(old), strict=True)  # a plain dict carries no version metadata: version None
    ref.load_state_dict(dict(old), strict=True)
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v) and torch.equal(ref.state_dict()[k], v)
    # through the whole head, with the prefix
    whole = mv.RetinaNetHead(8, 3, 4)
    sd = whole.state_dict()
    name = f"{cls}_head."
    v1 = {k: v for k, v in sd.items() if not k.startswith(name)}
    v1.update({name + k: v for k, v in old.items()})
    whole.load_state_dict(v1, strict=True)
    assert torch.equal(whole.state_dict()[name + "conv.3.0.weight"], old["conv.6.weight"])


# ---- argument errors, the paths that are not built ---------------------------------------------------------------------------------------
def test_argument_errors():
    lib_bb, _ = _backbones()
    with pytest.raises(ValueError) as e:
        mv.RetinaNet(torch.nn.Identity(), 5)
    assert str(e.value) == ("backbone should contain an attribute out_channels specifying the number of output channels (assumed to be the "
                            "same for all the levels)")
    with pytest.raises(TypeError) as e:
        mv.RetinaNet(lib_bb(), 5, anchor_generator=3)
    assert str(e.value) == "anchor_generator should be of type AnchorGenerator or None instead of <class 'int'>"
    with pytest.raises(ValueError, match="4096"):
        mv.RetinaNet(lib_bb(), 5, topk_candidates=4097)
    assert mv.RetinaNet(lib_bb(), 5, topk_candidates=4096).topk_candidates == 4096


def test_inference_only_and_norm_layer():
    lib_bb, _ = _backbones()
    model = mv.RetinaNet(lib_bb(), 5, _skip_resize=True)
    img = [torch.zeros(3, 32, 32)]
    with pytest.raises(RuntimeError, match="inference only"):
        model.train()(img)
    model.eval()
    with pytest.raises(RuntimeError, match="inference only"):
        model(img, targets=[{}])
    x = [torch.zeros(1, 8, 4, 4)]
    for head in (mv.RetinaNetHead(8, 3, 4), mv.RetinaNetClassificationHead(8, 3, 4), mv.RetinaNetRegressionHead(8, 3)):
        with pytest.raises(RuntimeError, match="inference only"):
            head.train()(x)
    for make in (lambda n: mv.RetinaNetHead(8, 3, 4, norm_layer=n), lambda n: mv.RetinaNetClassificationHead(8, 3, 4, norm_layer=n),
                 lambda n: mv.RetinaNetRegressionHead(8, 3, norm_layer=n)):
        with pytest.raises(NotImplementedError, match="norm_layer=None"):
            make(lambda c: torch.nn.GroupNorm(4, c))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        mv.RetinaNetHead(8, 3, 4)(x)


def test_joint_first_layer_follows_the_parameters():
    head = mv.RetinaNetHead(8, 3, 4)
    w, b = head.joint_first_layer(torch.device("cpu"))
    c, r = head.classification_head.conv[0][0], head.regression_head.conv[0][0]
    assert w.shape == (16, 8, 3, 3) and b.shape == (16,)
    assert torch.equal(w[:8], c.weight) and torch.equal(w[8:], r.weight)
    assert head.joint_first_layer(torch.device("cpu"))[0] is w
    with torch.no_grad():
        r.bias.add_(1.0)
    w2, b2 = head.joint_first_layer(torch.device("cpu"))
    assert bool((b2[8:] == 1).all()) and bool((b2[:8] == 0).all())


def test_concat_layout_equals_the_replica():
    g = torch.Generator().manual_seed(6)
    maps = [torch.randn((2, 3 * 5, h, w), generator=g) for h, w in ((4, 6), (2, 3))]
    got = retinanet.concat_layout(maps, 5)
    assert torch.equal(got, torch.cat([R.permute_level(m, 5) for m in maps], 1)) and got.shape == (2, 3 * (24 + 6), 5)
    y, x, a, c = 1, 2, 1, 3
    assert got[1, 3 * 24 + (y * 3 + x) * 3 + a, c] == maps[1][1, a * 5 + c, y, x]


# ---- the C entries: refusals with host pointers -----------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -2
SENT = -7.25


class _Topk:
    """One level (1, 3 * classes, 5, 7), k = 4, everything in host memory: valid arguments that single tests spoil."""

    def __init__(self, classes=2):
        self.numel = 105 * classes
        self.need = int(_lib.load().mv_retinanet_topk_workspace_bytes(1, _ints(5), _ints(7), _ints(3), 1, classes, 4))
        self.logits = np.zeros(self.numel, np.float32)
        self.idx = np.full(4, 0x5AA5C33C, np.int32)
        self.ws = np.full(self.need + 16, 0xA5, np.uint8)
        self.ws_ptr = self.ws.ctypes.data + (-self.ws.ctypes.data) % 16
        self.kw = dict(logits=_ptrs(self.logits), hs=_ints(5), ws=_ints(7), as_=_ints(3), strides=_i64s(self.numel), levels=1, classes=classes,
                       n=1, k=4, thresh=0.05, idx=self.idx.ctypes.data, wsp=self.ws_ptr, nbytes=self.need)

    def call(self, **over):
        a = {**self.kw, **over}
        rc = _lib.load().mv_retinanet_topk_f32(a["logits"], a["hs"], a["ws"], a["as_"], a["strides"], a["levels"], a["classes"], a["n"], a["k"],
                                               a["thresh"], a["idx"], a["wsp"], a["nbytes"], None)
        assert bool((self.idx == 0x5AA5C33C).all()) and bool((self.ws == 0xA5).all()), "a refused call wrote"
        return rc, _lib.load().mv_last_error().decode()


def test_topk_workspace_and_chunk():
    lib = _lib.load()
    chunk = lib.mv_retinanet_topk_chunk()
    assert chunk == F.retinanet_topk_chunk() and chunk >= 1024 and chunk % 1024 == 0
    one = lambda n, k, h=5: int(lib.mv_retinanet_topk_workspace_bytes(n, _ints(h), _ints(7), _ints(3), 1, 2, k))  # noqa: E731
    assert one(1, 4) == 16 + 4 * 8                    # the counts rounded up to 16 bytes, one chunk of min(k, chunk) keys
    assert one(5, 4) == 32 + 5 * 4 * 8
    assert one(1, 4, h=chunk) == 16 + 42 * 4 * 8      # 42 chunks: 3 * 2 * 7 maps of `chunk` elements
    assert one(1, 4, h=chunk + 1) == 16 + 43 * 4 * 8
    assert one(1, 4097) == 0 and one(0, 4) == 0 and one(1, 0) == 0
    assert int(lib.mv_retinanet_topk_workspace_bytes(1, _ints(5), _ints(7), _ints(3), 1, 0, 4)) == 0
    assert int(lib.mv_retinanet_topk_workspace_bytes(1, _ints(5), _ints(7), _ints(3), 9, 2, 4)) == 0


def _topk_cases(t):
    """(spoiled arguments, status, part of the message), written on the fixture t (test_rpn_host._topk_cases)."""
    return [
        (dict(logits=None), INVALID, "null pointer"),
        (dict(logits=_ptrs(None)), INVALID, "null pointer (level 0)"),
        (dict(idx=None), INVALID, "null pointer"),
        (dict(hs=None), INVALID, "null level table"),
        (dict(strides=None), INVALID, "null pointer"),
        (dict(levels=0), INVALID, "1 to 8 levels"),
        (dict(levels=9), UNSUPPORTED, "1 to 8 levels"),
        (dict(hs=_ints(0)), INVALID, "bad shape"),
        (dict(ws=_ints(-7)), INVALID, "bad shape"),
        (dict(as_=_ints(0)), INVALID, "bad shape"),
        (dict(classes=0), INVALID, "classes must be positive"),
        (dict(classes=-3), INVALID, "classes must be positive"),
        (dict(k=0), INVALID, "k must be positive"),
        (dict(k=4097, nbytes=1 << 20), UNSUPPORTED, "k up to 4096"),
        (dict(n=-1), INVALID, "bad image count"),
        (dict(strides=_i64s(t.numel - 1)), INVALID, "image stride"),
        (dict(hs=_ints(1 << 15), ws=_ints(1 << 15), as_=_ints(2)), UNSUPPORTED, "32-bit index"),
        (dict(hs=_ints(1 << 10), ws=_ints(1 << 10), classes=1 << 10), UNSUPPORTED, "32-bit index"),
        (dict(wsp=None), INVALID, "needs a workspace"),
        (dict(nbytes=t.need - 1), INVALID, f"workspace of {t.need - 1} bytes, need {t.need}"),
        (dict(wsp=t.ws_ptr + 4), INVALID, "16-byte aligned"),
        (dict(idx=t.logits.ctypes.data + 4 * 50), INVALID, "must not overlap"),
        (dict(wsp=(t.logits.ctypes.data + 15) // 16 * 16), INVALID, "must not overlap"),
    ]


def test_topk_refusals():
    t = _Topk()
    for over, status, text in _topk_cases(t):
        rc, msg = t.call(**over)
        assert rc == status and text in msg, (over.keys(), rc, msg)
    assert t.call(n=0, logits=None, idx=None, wsp=None, nbytes=0)[0] == 0


class _Decode:
    out64 = "lb"  # the key of the int64 output in `kw`

    def __init__(self, classes=2):
        self.numel = 105 * classes  # the elements of the logit map
        self.logits, self.deltas = np.zeros(self.numel, np.float32), np.zeros(420, np.float32)
        self.base, self.sizes = np.zeros(12, np.float32), np.array([20.0, 28.0], np.float32)
        self.idx = np.zeros(4, np.int32)
        self.boxes, self.scores = np.full(16, SENT, np.float32), np.full(4, SENT, np.float32)
        self.labels, self.valid = np.full(4, 0x5AA5C33C, np.int64), np.full(4, 0xA5, np.uint8)
        self.kw = dict(logits=_ptrs(self.logits), deltas=_ptrs(self.deltas), hs=_ints(5), ws=_ints(7), as_=_ints(3), ls=_i64s(self.numel),
                       ds=_i64s(420), sh=_ints(4), sw=_ints(4), levels=1, classes=classes, base=self.base.ctypes.data, sizes=self.sizes.ctypes.data,
                       idx=self.idx.ctypes.data, n=1, k=4, boxes=self.boxes.ctypes.data, scores=self.scores.ctypes.data,
                       lb=self.labels.ctypes.data, valid=self.valid.ctypes.data)

    def call(self, **over):
        a = {**self.kw, **over}
        rc = _lib.load().mv_retinanet_decode_f32(a["logits"], a["deltas"], a["hs"], a["ws"], a["as_"], a["ls"], a["ds"], a["sh"], a["sw"],
                                                 a["levels"], a["classes"], a["base"], a["sizes"], a["idx"], a["n"], a["k"], 1.0, 1.0, 1.0, 1.0,
                                                 math.log(1000.0 / 16), a["boxes"], a["scores"], a["lb"], a["valid"], None)
        assert bool((self.boxes == SENT).all()) and bool((self.scores == SENT).all()) and bool((self.labels == 0x5AA5C33C).all()) and \
            bool((self.valid == 0xA5).all()), "a refused call wrote"
        return rc, _lib.load().mv_last_error().decode()


def _decode_cases(d):
    """As _topk_cases, for the fixture d of a decode entry."""
    cases = [(dict(**{name: None}), INVALID, "null") for name in ("logits", "deltas", "hs", "ws", "as_", "ls", "ds", "sh", "sw", "base", "sizes",
                                                                  "idx", "boxes", "scores", d.out64, "valid")]
    return cases + [
        (dict(deltas=_ptrs(None)), INVALID, "null pointer (level 0)"),
        (dict(levels=0), INVALID, "1 to 8 levels"),
        (dict(levels=9), UNSUPPORTED, "1 to 8 levels"),
        (dict(hs=_ints(0)), INVALID, "bad shape"),
        (dict(as_=_ints(-1)), INVALID, "bad shape"),
        (dict(classes=0), INVALID, "classes must be positive"),
        (dict(sh=_ints(-4)), INVALID, "bad strides"),
        (dict(n=-1), INVALID, "bad shape"),
        (dict(k=-1), INVALID, "bad shape"),
        (dict(ls=_i64s(d.numel - 1)), INVALID, "image strides"),
        (dict(ds=_i64s(419)), INVALID, "image strides"),
        (dict(hs=_ints(1 << 10), ws=_ints(1 << 10), classes=1 << 10), UNSUPPORTED, "32-bit index"),
        ({d.out64: d.kw[d.out64] + 4}, INVALID, "8-byte aligned"),
        (dict(boxes=d.deltas.ctypes.data), INVALID, "must not overlap"),
        (dict(scores=d.logits.ctypes.data + 4 * (d.numel - 1)), INVALID, "must not overlap"),
        (dict(scores=d.boxes.ctypes.data + 4 * 15), INVALID, "must not overlap"),
        (dict(valid=d.idx.ctypes.data), INVALID, "must not overlap"),
        ({d.out64: d.base.ctypes.data}, INVALID, "must not overlap"),
    ]


def test_decode_refusals():
    d = _Decode()
    for over, status, text in _decode_cases(d):
        rc, msg = d.call(**over)
        assert rc == status and text in msg, (list(over), rc, msg)
    assert d.call(n=0, logits=None, boxes=None)[0] == 0
    assert d.call(k=0, idx=None, boxes=None, scores=None, lb=None, valid=None)[0] == 0


def test_rpn_entries_refuse_as_the_one_class_retinanet_entries():
    """The rpn entries and the retinanet entries with classes = 1 answer every spoiled call alike: the same status, and the same
    message once `retinanet_` reads `rpn_` and `labels must` reads `levels must`.  The spoils are every case of the four refusal
    tables (this file's and test_rpn_host's) that does not set `classes`, each written on the fixture it runs on (105 logits here),
    and an image count and a candidate count past the launch grid.  The size of the workspace is each entry's own (32 bytes
    against 48 here), so the one message that prints it is compared with the sizes of its own fixture written in."""
    lib = _lib.load()
    assert int(lib.mv_retinanet_topk_workspace_bytes(1, _ints(5), _ints(7), _ints(3), 1, 1, 4)) > 0
    assert int(lib.mv_rpn_topk_workspace_bytes(1, _ints(5), _ints(7), _ints(3), 1, 4)) == 32
    grid = "exceed the launch grid"
    pairs = [(RH._Topk(), _Topk(classes=1), (RH._topk_cases, _topk_cases), (dict(n=70000), UNSUPPORTED, grid)),
             (RH._Decode(), _Decode(classes=1), (RH._decode_cases, _decode_cases), (dict(n=1 << 33, k=1 << 33), UNSUPPORTED, grid))]
    for rpn, ret, tables, extra in pairs:
        spoils = lambda fixture: [c for table in tables for c in table(fixture) if "classes" not in c[0]] + [extra]  # noqa: E731
        on_rpn, on_ret = spoils(rpn), spoils(ret)
        assert len(on_rpn) == len(on_ret) >= 40
        for (over_rpn, status, text), (over_ret, _, _) in zip(on_rpn, on_ret):
            rc_rpn, msg_rpn = rpn.call(**over_rpn)
            rc_ret, msg_ret = ret.call(**over_ret)
            msg_ret = msg_ret.replace("retinanet_", "rpn_").replace("labels must", "levels must")
            if "nbytes" in over_ret and "k" not in over_ret:
                assert f"workspace of {ret.need - 1} bytes, need {ret.need} " in msg_ret
                msg_ret = msg_ret.replace(f"of {ret.need - 1} bytes, need {ret.need} ", f"of {rpn.need - 1} bytes, need {rpn.need} ")
            assert rc_rpn == rc_ret == status and msg_rpn == msg_ret and text in msg_rpn, (list(over_rpn), rc_rpn, msg_rpn, rc_ret, msg_ret)


# ---- the Python checks fire before a device is needed ---------------------------------------------------------------------------------
def _random_maps(seed, n=2, a=3, k=2, grids=((4, 6), (2, 3))):
    g = torch.Generator().manual_seed(seed)
    return ([torch.randn((n, a * k, h, w), generator=g) * 3 for h, w in grids], [torch.randn((n, 4 * a, h, w), generator=g) for h, w in grids])


def test_functional_checks_and_messages():
    cl, dl = _random_maps(9)
    with pytest.raises(TypeError, match="non-empty list"):
        F.retinanet_topk([], 2, 4, 0.05)
    with pytest.raises(_lib.Mi355VisionError, match="up to 8 levels"):
        F.retinanet_topk([cl[0]] * 9, 2, 4, 0.05)
    with pytest.raises(RuntimeError, match="4-D tensor"):
        F.retinanet_topk([cl[0][0]], 2, 4, 0.05)
    with pytest.raises(TypeError, match="float32"):
        F.retinanet_topk([cl[0].double()], 2, 4, 0.05)
    with pytest.raises(RuntimeError, match="bad shape"):
        F.retinanet_topk(cl, 4, 4, 0.05)  # 6 channels are no multiple of 4 classes
    with pytest.raises(ValueError, match="num_classes must be a positive int"):
        F.retinanet_topk(cl, 0, 4, 0.05)
    with pytest.raises(ValueError, match="k must be a positive int"):
        F.retinanet_topk(cl, 2, 0, 0.05)
    with pytest.raises(_lib.Mi355VisionError, match="k up to 4096"):
        F.retinanet_topk(cl, 2, 4097, 0.05)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.retinanet_topk(cl, 2, 4, 0.05)
    idx = torch.zeros((2, 8), dtype=torch.int32)
    cells = [torch.zeros(3, 4)] * 2
    strides, sizes = [(4, 4), (8, 8)], [(16, 24), (15, 20)]
    with pytest.raises(RuntimeError, match="one map per level"):
        F.retinanet_decode(cl, dl[:1], idx, cells, strides, sizes, 2)
    with pytest.raises(RuntimeError, match="channels for 3 anchors"):
        F.retinanet_decode(cl, [dl[0][:, :8], dl[1]], idx, cells, strides, sizes, 2)
    with pytest.raises(RuntimeError, match="int32 tensor of shape"):
        F.retinanet_decode(cl, dl, idx.long(), cells, strides, sizes, 2)
    with pytest.raises(RuntimeError, match="cell_anchors should hold"):
        F.retinanet_decode(cl, dl, idx, cells[:1], strides, sizes, 2)
    with pytest.raises(RuntimeError, match="strides should hold"):
        F.retinanet_decode(cl, dl, idx, cells, [(4, 4), (-1, 8)], sizes, 2)
    with pytest.raises(RuntimeError, match="image_sizes should hold 2 rows"):
        F.retinanet_decode(cl, dl, idx, cells, strides, sizes[:1], 2)
    with pytest.raises(ValueError, match="four weights"):
        F.retinanet_decode(cl, dl, idx, cells, strides, sizes, 2, weights=(1.0, 1.0))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.retinanet_decode(cl, dl, idx, cells, strides, sizes, 2)
    assert mv.retinanet.RetinaNet is mv.RetinaNet and F.retinanet_topk is mv.functional.retinanet_topk


# ---- replica (a) against restatement (b) ------------------------------------------------------------------------------------------------
GRIDS = ((8, 10), (4, 5), (2, 3))
A, K, THRESH, TOPK = 3, 4, 0.35, 60  # 0.35: no grid point of the three levels lies within 1e-3 of logit(0.35) (asserted below)


def _grid_logits(seed):
    """Per level a seeded permutation of an evenly spaced grid on [-6, 6] with at most 4000 points."""
    g = torch.Generator().manual_seed(seed)
    maps = []
    for h, w in GRIDS:
        n = 2 * A * K * h * w
        assert n <= 4000
        grid = torch.linspace(-6.0, 6.0, n, dtype=torch.float64).float()
        maps.append(grid[torch.randperm(n, generator=g)].reshape(2, A * K, h, w))
    return maps


def test_replica_and_restatement_select_the_same_candidates():
    cls_maps = _grid_logits(31)
    g = torch.Generator().manual_seed(32)
    reg_maps = [torch.randn((2, 4 * A, h, w), generator=g) * 0.5 for h, w in GRIDS]
    # the margins the comparison rests on, asserted on the data
    logit_t = math.log(THRESH / (1 - THRESH))
    for m in cls_maps:
        assert float((m.double() - logit_t).abs().min()) > 1e-3, "a grid point within 1e-3 of logit(score_thresh)"
        s = torch.sort(R.sigmoid_cr(m.flatten()))[0]
        gap = (s[1:] - s[:-1]).min()
        ulp = torch.finfo(torch.float32).eps  # the ulp of scores in [0.5, 1), the greatest below 1
        assert float(gap) >= 50 * ulp, "neighbouring scores closer than 50 ulp: sigmoid's last bit could reorder them"
        assert int(P.ulp_distance(torch.sigmoid(m), R.sigmoid_cr(m)).max()) <= 2
        spacing = 12.0 / (m.numel() - 1)
        assert float(gap) >= 0.9 * spacing * math.exp(-6.0) / (1 + math.exp(-6.0)) ** 2  # sigma'(6) times the grid's spacing

    def make(numerics):
        ag = P.AnchorGenerator(((16, 20, 25), (32, 40, 50), (64, 80, 101)), ((1.0,),) * 3)
        bb = torch.nn.Identity()
        bb.out_channels = 8
        return R.RetinaNet(bb, K, anchor_generator=ag, score_thresh=THRESH, topk_candidates=TOPK, detections_per_img=30, numerics=numerics).eval()
    images = P.ImageList(torch.zeros(2, 3, 64, 80), [(64, 80), (60, 75)])
    (det_a, cand_a), (det_b, cand_b) = (make(n).from_head_maps(images, cls_maps, reg_maps, detailed=True) for n in (P.REPLICA, P.RESTATEMENT))
    want_idx = R.select(cls_maps, K, TOPK, THRESH)
    for i in range(2):
        assert torch.equal(cand_a[i]["idx"], cand_b[i]["idx"]), "tie-free and with margins: topk's order is the stable order"
        assert torch.equal(cand_b[i]["idx"], want_idx[i][want_idx[i] >= 0].long())
        assert len(cand_b[i]["idx"]) > TOPK, "more than one level contributes"
        # boxes by test_rpn_host's rule: bit-equal where torch.exp is correctly rounded for dw and dh, else within the bound there
        pa, pb = cand_a[i]["boxes"], cand_b[i]["boxes"]
        side, mag = (pb[:, 2:] - pb[:, :2]).abs().max(-1)[0], pb.abs().max(-1)[0]
        bound = ((side + mag * 2.0 ** -22) * 2.0 ** -23 + mag * 2.0 ** -23)[:, None]
        assert bool(((pa - pb).abs() <= bound).all())
        assert float((pa == pb).float().mean()) > 0.9
        assert torch.equal(cand_a[i]["labels"], cand_b[i]["labels"])
        # the final detections as sets: the kept candidates are the same
        key = lambda d: sorted(zip(d["labels"].tolist(), [round(float(s), 5) for s in d["scores"]]))  # noqa: E731
        assert key(det_a[i]) == key(det_b[i]) and 0 < len(det_b[i]["boxes"]) <= 30
    # and the fixed-shape form the kernels write agrees with the per-image form
    anchors = make(P.RESTATEMENT).anchor_generator(images, cls_maps)
    boxes, scores, labels, valid = R.decode(cls_maps, reg_maps, want_idx, anchors, images.image_sizes, K)
    for i in range(2):
        v = valid[i]
        assert torch.equal(v, want_idx[i] >= 0) and bool((~v).any())
        P.same(boxes[i][v], cand_b[i]["boxes"]), P.same(scores[i][v], cand_b[i]["scores"])
        assert torch.equal(labels[i][v], cand_b[i]["labels"])
        assert float(boxes[i][~v].abs().max()) == 0 and float(scores[i][~v].abs().max()) == 0
