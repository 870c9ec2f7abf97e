"""RPN without a GPU: the two references of tests/_rpn_ref.py against each other, AnchorGenerator / RPNHead / RegionProposalNetwork
against the replica (values, state, initialisation), every refusal of mv_rpn_topk_f32 / mv_rpn_decode_f32 / mv_box_decode_f32 with
host pointers (refusals come before any launch), and the Python-side checks."""
import math

import numpy as np
import pytest
import torch

import cpu_vision_amd as mv
from cpu_vision_amd import _lib, anchor_utils, image_list, rpn
from cpu_vision_amd import functional as F
from tests import _rpn_ref as P
from tests._util import c_i64s as _i64s, c_ints as _ints, c_ptrs as _ptrs


# ---- replica (a) against restatement (b) ----------------------------------------------------------------------------------------------
def _random_head_outputs(seed, n=2, a=3, grids=((16, 24), (8, 12), (5, 7))):
    g = torch.Generator().manual_seed(seed)
    ob = [torch.randn((n, a, h, w), generator=g) * 3 for h, w in grids]
    dl = [torch.randn((n, 4 * a, h, w), generator=g) for h, w in grids]
    return ob, dl


def _rpn_pair(pre=50, post=20, score_thresh=0.0):
    def make(numerics):
        ag = P.AnchorGenerator(((32,), (64,), (128,)), ((0.5, 1.0, 2.0),) * 3)
        return P.RegionProposalNetwork(ag, P.RPNHead(8, 3), 0.7, 0.3, 256, 0.5, {"training": 2000, "testing": pre}, {"training": 2000, "testing": post},
                                       0.7, score_thresh, numerics=numerics).eval()
    return make(P.REPLICA), make(P.RESTATEMENT)


def test_replica_and_restatement_agree_up_to_one_ulp_of_exp():
    """Every anchor of three levels decoded by both references, and the sigmoid of every logit."""
    ob, dl = _random_head_outputs(1)
    images = P.ImageList(torch.zeros(2, 3, 64, 96), [(64, 96), (61, 90)])
    a, b = _rpn_pair()
    anchors = a.anchor_generator(images, ob)
    logits, deltas = P.concat_box_prediction_layers(ob, dl)
    pa, pb = a.box_coder.decode(deltas, anchors).reshape(-1, 4), b.box_coder.decode(deltas, anchors).reshape(-1, 4)
    # where torch.exp is the correctly rounded exp for the box's dw and dh the coordinates are bit-equal
    d = torch.clamp(deltas[:, 2:], max=math.log(1000.0 / 16))
    exact = (torch.exp(d) == P.exp_cr(d)).all(-1)
    print(f"torch.exp is correctly rounded for both sides of {float(exact.float().mean()):.4f} of {exact.numel()} boxes")
    assert exact.float().mean() > 0.9, "more than 10 % of the boxes excluded"
    np.testing.assert_array_equal(pa[exact].numpy(), pb[exact].numpy())
    # elsewhere within what one ulp of exp moves a coordinate: exp and its product with the anchor's side differ by at most
    # 2^-23 + 2^-23 relative, so the half side by side * 2^-23; the final sum or difference rounds on each side by at most half an
    # ulp of the coordinate, |c| * 2^-24 each.  `side` is the restatement's own x2 - x1, itself within |c| * 2^-22 of the side
    side, mag = (pb[:, 2:] - pb[:, :2]).abs().max(-1)[0], pb.abs().max(-1)[0]
    bound = ((side + mag * 2.0 ** -22) * 2.0 ** -23 + mag * 2.0 ** -23)[:, None]
    assert bool(((pa - pb).abs() <= bound)[~exact].all())
    sa, sb = torch.sigmoid(logits), P.sigmoid_cr(logits)
    dist = P.ulp_distance(sa, sb)
    print(f"sigmoid: {float((dist > 0).float().mean()):.4f} of {dist.numel()} scores differ, by at most {int(dist.max())} ulp")
    assert int(dist.max()) <= 2


def test_selected_index_sets_are_equal_on_tie_free_logits():
    ob, dl = _random_head_outputs(2)
    images = P.ImageList(torch.zeros(2, 3, 64, 96), [(64, 96), (61, 90)])
    a, b = _rpn_pair(pre=50)
    ia, ib = a.from_head_outputs(images, ob, dl, detailed=True)["idx"], b.from_head_outputs(images, ob, dl, detailed=True)["idx"]
    assert torch.equal(ia, ib)  # tie-free: topk's order is the stable order


# ---- AnchorGenerator ----------------------------------------------------------------------------------------------------------------
def test_anchor_generator_default_values():
    ag = mv.AnchorGenerator()
    assert ag.sizes == ((128, 256, 512),) and ag.aspect_ratios == ((0.5, 1.0, 2.0),)
    want = torch.tensor([[-91., -45., 91., 45.], [-181., -91., 181., 91.], [-362., -181., 362., 181.], [-64., -64., 64., 64.],
                         [-128., -128., 128., 128.], [-256., -256., 256., 256.], [-45., -91., 45., 91.], [-91., -181., 91., 181.],
                         [-181., -362., 181., 362.]])
    assert len(ag.cell_anchors) == 1 and torch.equal(ag.cell_anchors[0], want)
    assert ag.num_anchors_per_location() == [9]


def test_anchor_generator_equals_the_replica_on_fpn_sizes_and_unequal_strides():
    lib_ag, ref_ag = mv.AnchorGenerator(P.FPN_SIZES, P.FPN_RATIOS), P.AnchorGenerator(P.FPN_SIZES, P.FPN_RATIOS)
    assert lib_ag.num_anchors_per_location() == [3] * 5
    for got, want in zip(lib_ag.cell_anchors, ref_ag.cell_anchors):
        assert torch.equal(got, want)
    assert torch.equal(lib_ag.cell_anchors[0], torch.tensor([[-23., -11., 23., 11.], [-16., -16., 16., 16.], [-11., -23., 11., 23.]]))
    # padded batch 64 x 96 over grids 16 x 24, 8 x 12, 5 x 7, 2 x 3, 1 x 1: strides (4, 4), (8, 8), (12, 13), (32, 32), (64, 96)
    maps = [torch.zeros(2, 4, h, w) for h, w in ((16, 24), (8, 12), (5, 7), (2, 3), (1, 1))]
    tensors = torch.zeros(2, 3, 64, 96)
    got = lib_ag(image_list.ImageList(tensors, [(64, 96), (61, 90)]), maps)
    want = ref_ag(P.ImageList(tensors, [(64, 96), (61, 90)]), maps)
    assert len(got) == 2 and got[0].shape == (3 * (16 * 24 + 8 * 12 + 35 + 6 + 1), 4)
    for g, w in zip(got, want):
        assert torch.equal(g, w) and g.dtype == torch.float32
    # anchor i = (y W + x) A + a of level 2 (strides 12, 13)
    start, (y, x, a) = 3 * (16 * 24 + 8 * 12), (3, 5, 2)
    b = lib_ag.cell_anchors[2][a]
    assert torch.equal(got[0][start + (y * 7 + x) * 3 + a], torch.tensor([x * 13 + b[0], y * 12 + b[1], x * 13 + b[2], y * 12 + b[3]]))


def test_anchor_generator_argument_normalisation_and_asserts():
    ag = mv.AnchorGenerator(sizes=(32, 64), aspect_ratios=(0.5, 1.0))
    assert ag.sizes == ((32,), (64,)) and ag.aspect_ratios == ((0.5, 1.0), (0.5, 1.0))
    ref = P.AnchorGenerator(sizes=(32, 64), aspect_ratios=(0.5, 1.0))
    assert all(torch.equal(g, w) for g, w in zip(ag.cell_anchors, ref.cell_anchors))
    with pytest.raises(AssertionError, match="Anchors should be Tuple"):
        ag.grid_anchors([(2, 2)], [[torch.tensor(4), torch.tensor(4)]])
    with pytest.raises(AssertionError, match="Anchors should be Tuple"):
        ag(image_list.ImageList(torch.zeros(1, 3, 8, 8), [(8, 8)]), [torch.zeros(1, 2, 2, 2)])
    ag.cell_anchors = None
    with pytest.raises(AssertionError, match="cell_anchors should not be None"):
        ag.grid_anchors([(2, 2)], [[torch.tensor(4), torch.tensor(4)]])


def test_image_list():
    t = torch.zeros(2, 3, 4, 5)
    il = mv.ImageList(t, [(4, 5), (3, 4)])
    moved = il.to(torch.device("cpu"))
    assert isinstance(moved, mv.ImageList) and moved.image_sizes == [(4, 5), (3, 4)] and moved.tensors.shape == t.shape


# ---- RPNHead / RegionProposalNetwork: state and initialisation -----------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
def test_head_state_and_seeded_construction_equal_the_replica(depth):
    torch.manual_seed(7)
    head = rpn.RPNHead(16, 3, conv_depth=depth)
    after = torch.rand(1)
    torch.manual_seed(7)
    ref = P.RPNHead(16, 3, conv_depth=depth)
    ref_after = torch.rand(1)
    assert torch.equal(after, ref_after), "the constructor leaves the RNG where the reference leaves it"
    sd, ref_sd = head.state_dict(), ref.state_dict()
    assert list(sd) == list(ref_sd)
    for k in sd:
        assert sd[k].shape == ref_sd[k].shape and torch.equal(sd[k], ref_sd[k]), k
    assert "conv.0.0.weight" in sd and sd["cls_logits.weight"].shape == (3, 16, 1, 1) and sd["bbox_pred.weight"].shape == (12, 16, 1, 1)
    assert sd["_metadata"][""]["version"] == 2 if "_metadata" in sd else head._version == 2
    assert not head.training
    head.load_state_dict(ref_sd, strict=True)
    ref.load_state_dict(sd, strict=True)


def test_head_loads_a_version_1_state_dict():
    torch.manual_seed(3)
    src = rpn.RPNHead(8, 3)
    old = {("conv." + k[len("conv.0.0."):] if k.startswith("conv.0.0.") else k): v.clone() for k, v in src.state_dict().items()}
    assert "conv.weight" in old and "conv.0.0.weight" not in old
    dst, ref = rpn.RPNHead(8, 3), P.RPNHead(8, 3)
    dst.load_state_dict(dict(old), strict=True)   # a plain dict carries no version metadata: version None
    ref.load_state_dict(dict(old), strict=True)
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v) and torch.equal(ref.state_dict()[k], v)


def _lib_rpn(head=None, **kw):
    ag = mv.AnchorGenerator(P.FPN_SIZES, P.FPN_RATIOS)
    head = head or rpn.RPNHead(16, 3)
    return mv.RegionProposalNetwork(ag, head, 0.7, 0.3, 256, 0.5, {"training": 2000, "testing": 1000}, {"training": 2000, "testing": 300}, 0.7, **kw)


def test_rpn_state_constructor_and_top_n():
    torch.manual_seed(11)
    m = _lib_rpn()
    after = torch.rand(1)
    torch.manual_seed(11)
    ref = P.RegionProposalNetwork(P.AnchorGenerator(P.FPN_SIZES, P.FPN_RATIOS), P.RPNHead(16, 3), 0.7, 0.3, 256, 0.5,
                                  {"training": 2000, "testing": 1000}, {"training": 2000, "testing": 300}, 0.7)
    assert torch.equal(after, torch.rand(1))
    sd, ref_sd = m.state_dict(), ref.state_dict()
    assert list(sd) == list(ref_sd) == ["head.conv.0.0.weight", "head.conv.0.0.bias", "head.cls_logits.weight", "head.cls_logits.bias",
                                         "head.bbox_pred.weight", "head.bbox_pred.bias"]
    assert all(torch.equal(sd[k], ref_sd[k]) for k in sd)
    m.load_state_dict(ref_sd, strict=True)
    ref.load_state_dict(sd, strict=True)
    assert m.pre_nms_top_n() == 1000 and m.post_nms_top_n() == 300 and m.min_size == 1e-3 and m.score_thresh == 0.0
    assert m.box_coder.weights == (1.0, 1.0, 1.0, 1.0) and m.box_coder.bbox_xform_clip == math.log(1000.0 / 16)
    m.train()
    assert m.pre_nms_top_n() == 2000 and m.post_nms_top_n() == 2000
    feats = {"0": torch.zeros(1, 16, 4, 4)}
    with pytest.raises(RuntimeError, match="inference only"):
        m(mv.ImageList(torch.zeros(1, 3, 16, 16), [(16, 16)]), feats)
    m.eval()
    with pytest.raises(RuntimeError, match="inference only"):
        m(mv.ImageList(torch.zeros(1, 3, 16, 16), [(16, 16)]), feats, targets=[{}])
    with pytest.raises(TypeError, match="float32"):
        m(mv.ImageList(torch.zeros(1, 3, 16, 16), [(16, 16)]), {"0": torch.zeros(1, 16, 4, 4, dtype=torch.float64)})
    with pytest.raises(RuntimeError, match="inference only"):
        rpn.RPNHead(8, 3).train()([torch.zeros(1, 8, 4, 4)])


def test_joint_pointwise_weight_follows_the_parameters():
    head = rpn.RPNHead(8, 3)
    w, b = head.joint_pointwise(torch.device("cpu"))
    assert w.shape == (15, 8, 1, 1) and b.shape == (15,)
    assert torch.equal(w[:3], head.cls_logits.weight) and torch.equal(w[3:], head.bbox_pred.weight)
    assert head.joint_pointwise(torch.device("cpu"))[0] is w
    with torch.no_grad():
        head.bbox_pred.bias.add_(1.0)
    w2, b2 = head.joint_pointwise(torch.device("cpu"))
    assert torch.equal(b2[3:], head.bbox_pred.bias) and bool((b2[3:] == 1).all())


def test_concat_box_prediction_layers_equals_the_replica():
    ob, dl = _random_head_outputs(5)
    got, want = rpn.concat_box_prediction_layers(ob, dl), P.concat_box_prediction_layers(ob, dl)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # flat index (y W + x) A + a: logit channel a, delta q channel 4 a + q
    n_l0, (y, x, a) = 3 * 16 * 24, (2, 5, 1)
    i = n_l0 + (y * 12 + x) * 3 + a
    total = sum(o[0].numel() for o in ob)
    assert got[0][total + i, 0] == ob[1][1, a, y, x] and got[1][total + i, 2] == dl[1][1, 4 * a + 2, y, x]


# ---- the C entries: refusals with host pointers -----------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -2
SENT = -7.25


class _Topk:
    """One level (1, 3, 5, 7), k = 4, everything in host memory: valid arguments that single tests spoil."""

    def __init__(self):
        self.numel, self.need = 105, 32  # the elements of the map, the bytes of the workspace
        self.logits = np.zeros(105, np.float32)
        self.idx = np.full(4, 0x5AA5C33C, np.int32)
        self.ws = np.full(32 + 16, 0xA5, np.uint8)
        off = (-self.ws.ctypes.data) % 16
        self.ws_ptr = self.ws.ctypes.data + off
        self.kw = dict(logits=_ptrs(self.logits), hs=_ints(5), ws=_ints(7), as_=_ints(3), strides=_i64s(105), levels=1, n=1, k=4,
                       idx=self.idx.ctypes.data, wsp=self.ws_ptr, nbytes=32)

    def call(self, **over):
        a = {**self.kw, **over}
        rc = _lib.load().mv_rpn_topk_f32(a["logits"], a["hs"], a["ws"], a["as_"], a["strides"], a["levels"], a["n"], a["k"], a["idx"], a["wsp"],
                                         a["nbytes"], None)
        assert bool((self.idx == 0x5AA5C33C).all()) and bool((self.ws == 0xA5).all()), "a refused call wrote"
        return rc, _lib.load().mv_last_error().decode()


def _topk_cases(t):
    """(spoiled arguments, status, part of the message), written on the fixture t: test_retinanet_host runs them on its own too."""
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
        (dict(k=0), INVALID, "k must be positive"),
        (dict(k=4097, nbytes=1 << 20), UNSUPPORTED, "k up to 4096"),
        (dict(n=-1), INVALID, "bad image count"),
        (dict(strides=_i64s(t.numel - 1)), INVALID, "image stride"),
        (dict(hs=_ints(1 << 15), ws=_ints(1 << 15), as_=_ints(2)), UNSUPPORTED, "32-bit index"),
        (dict(wsp=None), INVALID, "needs a workspace"),
        (dict(nbytes=t.need - 1), INVALID, f"workspace of {t.need - 1} bytes, need {t.need}"),
        (dict(wsp=t.ws_ptr + 4), INVALID, "16-byte aligned"),
        (dict(idx=t.logits.ctypes.data + 4 * 50), INVALID, "must not overlap"),
        (dict(wsp=(t.logits.ctypes.data + 15) // 16 * 16), INVALID, "must not overlap"),
    ]


def test_topk_refusals():
    t = _Topk()
    lib = _lib.load()
    assert lib.mv_rpn_topk_workspace_bytes(1, _ints(5), _ints(7), _ints(3), 1, 4) == 32
    assert lib.mv_rpn_topk_workspace_bytes(2, _ints(5, 1), _ints(7, 1), _ints(3, 1), 2, 4) == 2 * 5 * 8
    assert lib.mv_rpn_topk_workspace_bytes(1, _ints(5), _ints(7), _ints(3), 1, 1000) == 848  # 105 candidates of 8 bytes, rounded up to 16
    assert lib.mv_rpn_topk_workspace_bytes(1, _ints(5), _ints(7), _ints(3), 1, 4097) == 0
    assert lib.mv_rpn_topk_workspace_bytes(1, _ints(5), _ints(7), _ints(3), 9, 4) == 0
    for over, status, text in _topk_cases(t):
        rc, msg = t.call(**over)
        assert rc == status and text in msg, (over.keys(), rc, msg)
    assert t.call(n=0, logits=None, idx=None, wsp=None, nbytes=0)[0] == 0


class _Decode:
    numel, out64 = 105, "lv"  # the elements of the logit map; the key of the int64 output in `kw`

    def __init__(self):
        self.logits, self.deltas = np.zeros(105, np.float32), np.zeros(420, np.float32)
        self.base, self.sizes = np.zeros(12, np.float32), np.array([20.0, 28.0], np.float32)
        self.idx = np.zeros(4, np.int32)
        self.boxes, self.scores = np.full(16, SENT, np.float32), np.full(4, SENT, np.float32)
        self.levels, self.valid = np.full(4, 0x5AA5C33C, np.int64), np.full(4, 0xA5, np.uint8)
        self.kw = dict(logits=_ptrs(self.logits), deltas=_ptrs(self.deltas), hs=_ints(5), ws=_ints(7), as_=_ints(3), ls=_i64s(105), ds=_i64s(420),
                       sh=_ints(4), sw=_ints(4), levels=1, base=self.base.ctypes.data, sizes=self.sizes.ctypes.data, idx=self.idx.ctypes.data, n=1,
                       k=4, boxes=self.boxes.ctypes.data, scores=self.scores.ctypes.data, lv=self.levels.ctypes.data, valid=self.valid.ctypes.data)

    def call(self, **over):
        a = {**self.kw, **over}
        rc = _lib.load().mv_rpn_decode_f32(a["logits"], a["deltas"], a["hs"], a["ws"], a["as_"], a["ls"], a["ds"], a["sh"], a["sw"], a["levels"],
                                           a["base"], a["sizes"], a["idx"], a["n"], a["k"], 1.0, 1.0, 1.0, 1.0, math.log(1000.0 / 16), 1e-3, 0.0,
                                           a["boxes"], a["scores"], a["lv"], a["valid"], None)
        assert bool((self.boxes == SENT).all()) and bool((self.scores == SENT).all()) and bool((self.levels == 0x5AA5C33C).all()) and \
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
        (dict(sh=_ints(-4)), INVALID, "bad strides"),
        (dict(n=-1), INVALID, "bad shape"),
        (dict(k=-1), INVALID, "bad shape"),
        (dict(ls=_i64s(d.numel - 1)), INVALID, "image strides"),
        (dict(ds=_i64s(419)), INVALID, "image strides"),
        (dict(hs=_ints(1 << 15), ws=_ints(1 << 15), as_=_ints(2)), UNSUPPORTED, "32-bit index"),
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
    assert d.call(k=0, idx=None, boxes=None, scores=None, lv=None, valid=None)[0] == 0


def test_box_decode_refusals():
    lib = _lib.load()
    boxes, codes, out = np.zeros(8, np.float32), np.zeros(16, np.float32), np.full(16, SENT, np.float32)
    clip = math.log(1000.0 / 16)

    def call(b, c, o, m=2, classes=2):
        rc = lib.mv_box_decode_f32(b, c, o, m, classes, 10.0, 10.0, 5.0, 5.0, clip, None)
        assert bool((out == SENT).all()), "a refused call wrote"
        return rc, lib.mv_last_error().decode()

    pb, pc, po = boxes.ctypes.data, codes.ctypes.data, out.ctypes.data
    for args, status, text in [((None, pc, po), INVALID, "null pointer"), ((pb, None, po), INVALID, "null pointer"), ((pb, pc, None), INVALID, "null pointer"),
                               ((pb, pc, po, -1), INVALID, "bad shape"), ((pb, pc, po, 2, 0), INVALID, "bad shape"),
                               ((pb, pc, pc), INVALID, "must not overlap"), ((pb, pc, pb + 4), INVALID, "must not overlap"),
                               ((pb, pc, pc + 4 * 15), INVALID, "must not overlap"), ((pb, pc, po, 1 << 40, 1 << 20), UNSUPPORTED, "launch grid")]:
        rc, msg = call(*args)
        assert rc == status and text in msg, (args, rc, msg)
    assert call(None, None, None, 0)[0] == 0


# ---- the Python checks fire before a device is needed ---------------------------------------------------------------------------------
def test_functional_checks_and_messages():
    ob, dl = _random_head_outputs(9)
    with pytest.raises(TypeError, match="non-empty list"):
        F.rpn_topk([], 4)
    with pytest.raises(TypeError, match="non-empty list"):
        F.rpn_topk(ob[0], 4)
    with pytest.raises(_lib.Mi355VisionError, match="up to 8 levels"):
        F.rpn_topk([ob[0]] * 9, 4)
    with pytest.raises(RuntimeError, match="4-D tensor"):
        F.rpn_topk([ob[0][0]], 4)
    with pytest.raises(TypeError, match="float32"):
        F.rpn_topk([ob[0].double()], 4)
    with pytest.raises(RuntimeError, match="holds 1 images"):
        F.rpn_topk([ob[0], ob[1][:1]], 4)
    with pytest.raises(ValueError, match="positive int"):
        F.rpn_topk(ob, 0)
    with pytest.raises(_lib.Mi355VisionError, match="k up to 4096"):
        F.rpn_topk(ob, 4097)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.rpn_topk(ob, 4)
    idx = torch.zeros((2, 12), dtype=torch.int32)
    cells = [torch.zeros(3, 4)] * 3
    strides = [(4, 4), (8, 8), (12, 13)]
    sizes = [(64, 96), (61, 90)]
    with pytest.raises(RuntimeError, match="one map per level"):
        F.rpn_decode(ob, dl[:2], idx, cells, strides, sizes)
    with pytest.raises(RuntimeError, match="channels for 3 anchors"):
        F.rpn_decode(ob, [dl[0][:, :8], dl[1], dl[2]], idx, cells, strides, sizes)
    with pytest.raises(RuntimeError, match="int32 tensor of shape"):
        F.rpn_decode(ob, dl, idx.long(), cells, strides, sizes)
    with pytest.raises(RuntimeError, match="cell_anchors should hold"):
        F.rpn_decode(ob, dl, idx, cells[:2], strides, sizes)
    with pytest.raises(RuntimeError, match="strides should hold"):
        F.rpn_decode(ob, dl, idx, cells, [(4, 4), (8, 8), (-1, 13)], sizes)
    with pytest.raises(RuntimeError, match="image_sizes should hold 2 rows"):
        F.rpn_decode(ob, dl, idx, cells, strides, sizes[:1])
    with pytest.raises(ValueError, match="four weights"):
        F.rpn_decode(ob, dl, idx, cells, strides, sizes, weights=(1.0, 1.0))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.rpn_decode(ob, dl, idx, cells, strides, sizes)
    with pytest.raises(RuntimeError, match=r"boxes should have shape \(M, 4\)"):
        F.box_decode(torch.zeros(3, 5), torch.zeros(3, 4), (1, 1, 1, 1))
    with pytest.raises(RuntimeError, match="rel_codes should have shape"):
        F.box_decode(torch.zeros(3, 4), torch.zeros(3, 6), (1, 1, 1, 1))
    with pytest.raises(TypeError, match="float32"):
        F.box_decode(torch.zeros(3, 4), torch.zeros(3, 4).double(), (1, 1, 1, 1))
    with pytest.raises(ValueError, match="four weights"):
        F.box_decode(torch.zeros(3, 4), torch.zeros(3, 4), (1, 1, 1))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.box_decode(torch.zeros(3, 4), torch.zeros(3, 4), (1, 1, 1, 1))
    coder = rpn.BoxCoder((10.0, 10.0, 5.0, 5.0))
    with pytest.raises(AssertionError, match="boxes of type list or tuple"):
        coder.decode(torch.zeros(3, 4), torch.zeros(3, 4))
    with pytest.raises(AssertionError, match="rel_codes of type torch.Tensor"):
        coder.decode([0.0], [torch.zeros(3, 4)])
    assert not hasattr(coder, "encode")
    assert F.MAX_RPN_LEVELS == 8 and F.MAX_RPN_TOPK == 4096 and F.BBOX_XFORM_CLIP == math.log(1000.0 / 16)
    assert mv.rpn.RegionProposalNetwork is mv.RegionProposalNetwork and mv.anchor_utils.AnchorGenerator is anchor_utils.AnchorGenerator
