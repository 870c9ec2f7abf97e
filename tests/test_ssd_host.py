"""SSD without a device: the module tree and the seeded initialisation of ssd300_vgg16 against the replica (tests/_ssd_ref.py), every
argument error, DefaultBoxGenerator against the replica and the restated float32 chain bit for bit, the host-side refusals of the new
ABI entries (with host pointers: nothing is launched), and the numerics of the two stated arithmetics -- the float64-summed L2 norm and
the softmax with a float64 sum -- against torch's float32 ops and a float64 evaluation, with the selection that follows from them."""
import ctypes as C
import warnings
from collections import OrderedDict

import pytest
import torch
from torch import nn

import cpu_vision_amd as mv
from cpu_vision_amd import _lib
from cpu_vision_amd import functional as F
from cpu_vision_amd import ssd as S
from cpu_vision_amd.anchor_utils import DefaultBoxGenerator
from tests import _ssd_ref as R


# ------------------------------------------------------------------------------------------------ the module tree
@pytest.fixture(scope="module")
def models():
    torch.manual_seed(7)
    mine = mv.ssd300_vgg16(num_classes=5)
    torch.manual_seed(7)
    ref = R.ssd300_vgg16(num_classes=5)
    return mine, ref


def test_state_dict_keys_and_seeded_init(models):
    mine, ref = models
    a, b = mine.state_dict(), ref.state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    keys = set(a)
    want = {"backbone.scale_weight"}
    want |= {f"backbone.features.{i}.{p}" for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21) for p in ("weight", "bias")}
    want |= {f"backbone.extra.0.{i}.{p}" for i in (1, 3, 5) for p in ("weight", "bias")}
    want |= {f"backbone.extra.0.7.{i}.{p}" for i in (1, 3) for p in ("weight", "bias")}
    want |= {f"backbone.extra.{b_}.{i}.{p}" for b_ in (1, 2, 3, 4) for i in (0, 2) for p in ("weight", "bias")}
    want |= {f"head.{h}.module_list.{i}.{p}" for h in ("classification_head", "regression_head") for i in range(6) for p in ("weight", "bias")}
    assert keys == want
    assert torch.equal(a["backbone.scale_weight"], torch.full((512,), 20.0))
    assert [n for n, _ in mine.named_children()] == ["backbone", "anchor_generator", "head", "transform"]
    assert [n for n, _ in mine.head.named_children()] == ["classification_head", "regression_head"]
    assert all(p.requires_grad for p in mine.parameters())  # five trainable layers: nothing frozen
    assert mine.backbone.features[16].ceil_mode is True and [m.ceil_mode for m in mine.backbone.features if isinstance(m, nn.MaxPool2d)] == \
        [False, False, True]
    assert mine.head.classification_head.num_columns == 5 and mine.head.regression_head.num_columns == 4
    assert [c.out_channels for c in mine.head.classification_head.module_list] == [20, 30, 30, 30, 20, 20]
    assert [c.out_channels for c in mine.head.regression_head.module_list] == [16, 24, 24, 24, 16, 16]


def test_defaults_and_attributes(models):
    mine, ref = models
    assert mine.box_coder.weights == (10.0, 10.0, 5.0, 5.0)
    assert (mine.score_thresh, mine.nms_thresh, mine.detections_per_img, mine.topk_candidates) == (0.01, 0.45, 200, 400)
    assert mine.neg_to_pos_ratio == ref.neg_to_pos_ratio == 3.0 and mine.iou_thresh == 0.5
    t = mine.transform
    assert t.fixed_size == (300, 300) and t.size_divisible == 1 and t.min_size == (300,) and t.max_size == 300
    assert t.image_mean == [0.48235, 0.45882, 0.40784] and t.image_std == [1.0 / 255.0] * 3
    g = mine.anchor_generator
    assert g.steps == [8, 16, 32, 64, 100, 300] and g.clip is True and g.num_anchors_per_location() == [4, 6, 6, 6, 4, 4]
    assert not mine.training and not mine.backbone.training and not mine.head.training
    assert S._retrieve_out_channels(mine.backbone, (300, 300)) == R.SSD300_OUT_CHANNELS


def test_argument_errors(models):
    mine, _ = models
    with pytest.raises(ValueError, match="no weight files"):
        mv.ssd300_vgg16(weights="DEFAULT")
    with pytest.raises(ValueError, match="no weight files"):
        mv.ssd300_vgg16(weights_backbone="DEFAULT")
    with pytest.raises(ValueError, match="aspect_ratios and steps should have the same length"):
        DefaultBoxGenerator([[2], [2, 3]], steps=[8])
    backbone = mine.backbone
    with pytest.raises(ValueError, match=r"output channels from the backbone \(6\) do not match .* aspect ratios \(2\)"):
        S.SSD(backbone, DefaultBoxGenerator([[2], [2]]), (300, 300), 3)
    with pytest.raises(ValueError, match="up to 4096 candidates"):
        S.SSD(backbone, R.ssd300_generator(), (300, 300), 3, topk_candidates=5000)
    with pytest.raises(AssertionError, match=r"trainable_layers should be in the range \[0, 5\]"):
        S._vgg_extractor(mv.nn.VGG("D", init_weights=False), False, 6)
    x = [torch.rand(3, 20, 30)]
    with pytest.raises(RuntimeError, match="inference only"):
        mine(x, targets=[{}])
    mine.train()
    try:
        with pytest.raises(RuntimeError, match="inference only"):
            mine(x)
    finally:
        mine.eval()
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):  # no fallback: a CPU tensor is refused
        mine(x)
    with pytest.raises(RuntimeError, match="inference only"):
        mine.head.classification_head.train()([torch.zeros(1, 512, 3, 3)])
    mine.head.eval()


def test_size_keyword_is_ignored_with_a_warning():
    torch.manual_seed(1)
    with pytest.warns(UserWarning, match="The size of the model is already fixed; ignoring the parameter."):
        m = mv.ssd300_vgg16(num_classes=2, size=(512, 512))
    assert m.transform.fixed_size == (300, 300)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = mv.ssd300_vgg16(num_classes=2, trainable_backbone_layers=2)  # without weights: falls back to 5, as the reference
    assert all(p.requires_grad for p in m.parameters())


def test_vgg_extractor_freezes_and_highres():
    vgg = mv.nn.VGG("D", init_weights=False)
    ext = S._vgg_extractor(vgg, True, 2)
    frozen = [n for n, p in ext.named_parameters() if not p.requires_grad]
    assert frozen == [f"features.{i}.{p}" for i in (0, 2, 5, 7, 10, 12, 14) for p in ("weight", "bias")]  # before stage_indices[3] = 16
    assert len(ext.extra) == 6 and ext.extra[5][2].kernel_size == (4, 4)
    assert S._retrieve_out_channels(ext, (512, 512)) == [512, 1024, 512, 256, 256, 256, 256]
    ext0 = S._vgg_extractor(mv.nn.VGG("D", init_weights=False), False, 0)
    assert not any(p.requires_grad for n, p in ext0.named_parameters() if n.startswith("features") or n.startswith("extra.0.") and ".7." not in n)


class _Small(nn.Module):
    """A two-level CPU backbone without out_channels: SSD probes it with a forward on zeros, as the reference does."""

    def __init__(self):
        super().__init__()
        self.a, self.b = nn.Conv2d(3, 8, 3, stride=4, padding=1), nn.Conv2d(8, 12, 3, stride=2, padding=1)

    def forward(self, x):
        x = self.a(x)
        return OrderedDict([("0", x), ("1", self.b(x))])


def test_out_channels_attribute_and_probing_forward():
    gen = DefaultBoxGenerator([[2], [2, 3]])
    m = S.SSD(_Small(), gen, (32, 24), 3)
    assert [c.in_channels for c in m.head.classification_head.module_list] == [8, 12]
    b = _Small()
    b.out_channels = [8, 12]
    m = S.SSD(b, gen, (32, 24), 3)
    assert [c.out_channels for c in m.head.regression_head.module_list] == [16, 24]


# ------------------------------------------------------------------------------------------------ DefaultBoxGenerator
SSD300 = dict(aspect_ratios=[[2], [2, 3], [2, 3], [2, 3], [2], [2]], scales=[0.07, 0.15, 0.33, 0.51, 0.69, 0.87, 1.05],
              steps=[8, 16, 32, 64, 100, 300])
BOX_CONFIGS = {
    "ssd300": (SSD300, (300, 300), [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1)]),
    "steps": (dict(aspect_ratios=[[2], [2, 3], [2]], steps=[7, 13, 29]), (61, 47), [(9, 7), (5, 4), (3, 2)]),
    "no_steps": (dict(aspect_ratios=[[2], [2, 3], [2]]), (61, 47), [(9, 7), (5, 4), (3, 2)]),
}


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("name", list(BOX_CONFIGS))
def test_default_boxes_equal_the_replica_and_the_restated_chain(name, clip):
    kw, image, grids = BOX_CONFIGS[name]
    mine, ref = DefaultBoxGenerator(clip=clip, **kw), R.DefaultBoxGenerator(clip=clip, **kw)
    assert mine.scales == ref.scales and mine.num_anchors_per_location() == ref.num_anchors_per_location()
    for a, b in zip(mine._wh_pairs, ref._wh_pairs):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    maps = [torch.zeros(2, 1, h, w) for h, w in grids]
    images = R.ImageList(torch.zeros(2, 3, *image), [image, (image[0] - 3, image[1] - 5)])
    got, want = mine(images, maps), ref(images, maps)
    assert len(got) == 2 and torch.equal(got[0], got[1])
    total = sum(h * w * a for (h, w), a in zip(grids, mine.num_anchors_per_location()))
    assert got[0].shape == (total, 4) and got[0].dtype == torch.float32
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[0], R.default_boxes(mine, grids, image))
    if name == "ssd300":
        assert total == 8732
    if not clip and name == "ssd300":
        assert float(torch.cat(mine._wh_pairs).max()) > 1  # 1.05 sqrt(2): the unclipped pair


def test_default_scales():
    g = DefaultBoxGenerator([[2], [2], [2]])
    assert g.scales == [0.15 + 0.75 * k / 2.0 for k in range(3)] + [1.0]
    assert DefaultBoxGenerator([[2, 3]], min_ratio=0.2, max_ratio=0.8).scales == [0.2, 0.8]
    assert "DefaultBoxGenerator(aspect_ratios=[[2], [2], [2]], clip=True" in repr(g)


# ------------------------------------------------------------------------------------------------ host-side refusals
def _ints(v):
    return (C.c_int * len(v))(*v)


def _i64s(v):
    return (C.c_int64 * len(v))(*v)


def _refused(rc, text, code=-1):
    msg = _lib.load().mv_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_l2_normalize_scale_refusals():
    lib = _lib.load()
    call = lambda x=64, y=4096, wt=8192, n=2, c=3, h=4, w=5, xs=60, ys=60, eps=1e-12: lib.mv_l2_normalize_scale_f32(  # noqa: E731
        x, y, wt, n, c, h, w, xs, ys, eps, None)
    _refused(call(n=-1), "negative size")
    _refused(call(c=-3), "negative size")
    _refused(call(eps=0.0), "eps must be positive")
    _refused(call(eps=float("nan")), "eps must be positive")
    _refused(call(eps=float("inf")), "eps must be positive")
    _refused(call(eps=1e-50), "eps must be positive")  # 0 as a float32
    _refused(call(xs=59), "image strides")
    _refused(call(ys=59), "image strides")
    _refused(call(x=None), "null pointer")
    _refused(call(y=None), "null pointer")
    _refused(call(wt=None), "null pointer")
    _refused(call(x=66), "4-byte aligned")
    _refused(call(y=4097), "4-byte aligned")
    _refused(call(y=64 + 16), "y must be x itself")
    _refused(call(y=64, ys=64, xs=60), "y must be x itself")  # the same pointer with another stride
    _refused(call(y=8192 - 64), "must not overlap weight")
    _refused(call(c=1 << 20, h=1 << 6, w=1 << 6), "32-bit index", code=-2)
    _refused(call(n=1 << 31, c=1, h=1, w=1), "launch grid", code=-2)
    assert call(n=0, x=None, y=None, wt=None) == 0 and call(c=0, x=None, y=None, wt=None) == 0 and call(w=0, x=None, y=None, wt=None) == 0
    for name, args in (("x", (torch.zeros(3, 4, 4), torch.ones(4))), ("weight", (torch.zeros(1, 3, 4, 4), torch.ones(4)))):
        with pytest.raises(RuntimeError, match=name):
            F.l2_normalize_scale(*args)
    with pytest.raises(TypeError, match="float32"):
        F.l2_normalize_scale(torch.zeros(1, 3, 4, 4, dtype=torch.float64), torch.ones(3))
    with pytest.raises(ValueError, match="eps must be positive"):
        F.l2_normalize_scale(torch.zeros(1, 3, 4, 4), torch.ones(3), eps=0.0)
    with pytest.raises(ValueError, match="out is x itself"):
        F.l2_normalize_scale(torch.zeros(1, 3, 4, 4), torch.ones(3), out=torch.zeros(1, 3, 4, 4))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.l2_normalize_scale(torch.zeros(1, 3, 4, 4), torch.ones(3))


def test_max_pool2d_ceil_refusals():
    lib = _lib.load()
    call = lambda x=64, y=4096, planes=2, h=5, w=5, k=3, s=2, p=1: lib.mv_maxpool2d_ceil_f32(x, y, planes, h, w, k, s, p, None)  # noqa: E731
    _refused(call(planes=-1), "bad pooling shape")
    _refused(call(s=0), "bad pooling shape")
    _refused(call(p=2), "pad should be at most half")
    _refused(call(p=-1), "pad should be at most half")
    _refused(call(h=2, k=5, p=1), "Output size is too small")
    _refused(call(x=None), "null pointer")
    _refused(call(y=64), "alias")
    assert call(planes=0, x=None, y=None) == 0
    with pytest.raises(RuntimeError, match="pad should be at most half"):
        F.max_pool2d(torch.zeros(1, 5, 5), 2, 2, 2, ceil_mode=True)
    with pytest.raises(TypeError, match="float32"):
        F.max_pool2d(torch.zeros(1, 5, 5, dtype=torch.float64), 2, 2, 0, ceil_mode=True)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.max_pool2d(torch.zeros(1, 5, 5), 2, 2, 0, ceil_mode=True)
    with pytest.raises(TypeError):
        F.max_pool2d(torch.zeros(1, 5, 5), 2, 2, 0, True)  # keyword-only
    from cpu_vision_amd._layers import _ceil_pool_out
    assert [_ceil_pool_out(*a) for a in ((75, 2, 2, 0), (3, 2, 2, 1), (4, 2, 2, 1), (5, 3, 2, 1), (300, 2, 2, 0))] == [38, 2, 3, 3, 150]
    x = torch.zeros(1, 1, 7, 9)
    for k, s, p in ((2, 2, 0), (2, 2, 1), (3, 2, 1), (3, 1, 1), (3, 3, 0), (5, 4, 2)):
        want = nn.functional.max_pool2d(x, k, s, p, ceil_mode=True).shape[-2:]
        assert (_ceil_pool_out(7, k, s, p), _ceil_pool_out(9, k, s, p)) == tuple(want), (k, s, p)


def test_ssd_scores_refusals():
    lib = _lib.load()
    hs, ws, as_ = _ints([3, 2]), _ints([4, 2]), _ints([4, 6])
    maps = (C.c_void_p * 2)(4096, 65536)

    def call(logits=maps, hs=hs, ws=ws, as_=as_, strides=(3 * 4 * 4 * 5, 2 * 2 * 6 * 5), levels=2, classes=5, n=2, scores=1 << 20):
        return lib.mv_ssd_scores_f32(logits, hs, ws, as_, _i64s(list(strides)), levels, classes, n, scores, None)
    _refused(call(n=-1), "bad image count")
    _refused(call(levels=0), "1 to 8 levels")
    _refused(call(levels=9), "1 to 8 levels", code=-2)
    _refused(call(hs=None), "null level table")
    _refused(call(hs=_ints([0, 2])), "bad shape")
    _refused(call(classes=0), "classes must be positive")
    _refused(call(classes=1), "at least 2 classes")
    _refused(call(classes=1 << 27), "32-bit index", code=-2)
    _refused(call(n=65536), "launch grid", code=-2)
    _refused(call(logits=None), "null pointer")
    _refused(call(scores=None), "null pointer")
    _refused(call(logits=(C.c_void_p * 2)(4096, None)), "null pointer (level 1)")
    _refused(call(logits=(C.c_void_p * 2)(4098, 65536)), "4-byte aligned")
    _refused(call(scores=(1 << 20) + 2), "4-byte aligned")
    _refused(call(strides=(239, 120)), "image stride 239 of level 0")
    _refused(call(scores=4096 + 64), "must not overlap")
    assert call(n=0, logits=None, scores=None) == 0
    with pytest.raises(TypeError, match="non-empty list"):
        F.ssd_scores([], 3)
    with pytest.raises(RuntimeError, match="bad shape"):
        F.ssd_scores([torch.zeros(1, 7, 2, 2)], 3)
    with pytest.raises(ValueError, match="at least 2 classes"):
        F.ssd_scores([torch.zeros(1, 4, 2, 2)], 1)
    with pytest.raises(TypeError, match="float32"):
        F.ssd_scores([torch.zeros(1, 6, 2, 2, dtype=torch.float16)], 3)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.ssd_scores([torch.zeros(1, 6, 2, 2)], 3)


def test_ssd_topk_refusals():
    lib = _lib.load()
    call = lambda scores=4096, n=2, classes=5, v=100, k=7, thresh=0.01, idx=1 << 20: lib.mv_ssd_topk_f32(  # noqa: E731
        scores, n, classes, v, k, thresh, idx, None)
    _refused(call(n=-1), "bad shape")
    _refused(call(v=-1), "bad shape")
    _refused(call(k=0), "k must be positive")
    _refused(call(classes=1), "at least 2 classes")
    _refused(call(v=1 << 30, classes=3), "32-bit index", code=-2)
    _refused(call(k=4097), "k up to 4096", code=-2)
    _refused(call(n=65536), "launch grid", code=-2)
    _refused(call(scores=None), "null pointer")
    _refused(call(idx=None), "null pointer")
    _refused(call(scores=4098), "4-byte aligned")
    _refused(call(idx=(1 << 20) + 1), "4-byte aligned")
    _refused(call(idx=4096 + 400), "must not overlap")
    assert call(n=0, scores=None, idx=None) == 0
    with pytest.raises(RuntimeError, match="3-D"):
        F.ssd_topk(torch.zeros(2, 5), 3, 0.1)
    with pytest.raises(ValueError, match="k must be a positive int"):
        F.ssd_topk(torch.zeros(1, 3, 5), 0, 0.1)
    with pytest.raises(_lib.Mi355VisionError, match="k up to 4096"):
        F.ssd_topk(torch.zeros(1, 3, 5), 4097, 0.1)
    with pytest.raises(ValueError, match="at least 2 classes"):
        F.ssd_topk(torch.zeros(1, 1, 5), 2, 0.1)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.ssd_topk(torch.zeros(1, 3, 5), 2, 0.1)


def test_ssd_decode_refusals():
    lib = _lib.load()
    hs, ws, as_ = _ints([3, 2]), _ints([4, 2]), _ints([4, 6])
    maps = (C.c_void_p * 2)(4096, 65536)
    xf = (C.c_float * 2)(4.0, 2.0)
    base = dict(scores=1 << 20, deltas=maps, hs=hs, strides=(192, 96), levels=2, classes=5, wh=1 << 21, xf=xf, yf=xf, bh=30, bw=40,
                sizes=1 << 22, idx=1 << 23, n=2, k=9, boxes=1 << 24, out=1 << 25, labels=1 << 26, valid=1 << 27)

    def call(**over):
        a = {**base, **over}
        return lib.mv_ssd_decode_f32(a["scores"], a["deltas"], a["hs"], ws, as_, _i64s(list(a["strides"])), a["levels"], a["classes"], a["wh"], a["xf"],
                                     a["yf"], a["bh"], a["bw"], a["sizes"], a["idx"], a["n"], a["k"], 10.0, 10.0, 5.0, 5.0, 4.135, a["boxes"], a["out"],
                                     a["labels"], a["valid"], None)
    _refused(call(n=-1), "bad shape")
    _refused(call(k=-1), "bad shape")
    _refused(call(levels=9), "1 to 8 levels", code=-2)
    _refused(call(hs=None), "null level table")
    _refused(call(classes=1), "at least 2 classes")
    _refused(call(xf=None), "null level table")
    _refused(call(xf=(C.c_float * 2)(4.0, 0.0)), "bad grid divisors")
    _refused(call(yf=(C.c_float * 2)(float("nan"), 1.0)), "bad grid divisors")
    _refused(call(bh=0), "bad batch size")
    _refused(call(n=1 << 31, k=1 << 20), "launch grid", code=-2)
    for name in ("scores", "deltas", "wh", "sizes", "idx", "boxes", "out", "labels", "valid"):
        _refused(call(**{name: None}), "null pointer")
    _refused(call(deltas=(C.c_void_p * 2)(None, 65536)), "null pointer (level 0)")
    _refused(call(labels=(1 << 26) + 4), "8-byte aligned")
    _refused(call(idx=(1 << 23) + 2), "idx must be 4-byte aligned")
    _refused(call(boxes=(1 << 24) + 1), "4-byte aligned")
    _refused(call(strides=(191, 96)), "image stride 191 of level 0")
    _refused(call(out=(1 << 24) + 64), "must not overlap")
    _refused(call(boxes=(1 << 23) + 8), "must not overlap")
    assert call(n=0, scores=None, boxes=None) == 0 and call(k=0, idx=None, boxes=None) == 0
    pairs = [torch.ones(4, 2), torch.ones(6, 2)]
    reg = [torch.zeros(2, 16, 3, 4), torch.zeros(2, 24, 2, 2)]
    sc, idx = torch.zeros(2, 5, 72), torch.zeros(2, 9, dtype=torch.int32)
    ok = dict(scores=sc, bbox_regression=reg, idx=idx, wh_pairs=pairs, steps=None, batch_size=(30, 40), image_sizes=[(30, 40), (28, 33)])
    for over, exc, text in ((dict(wh_pairs=[torch.ones(4, 3)] * 2), RuntimeError, "wh_pairs"), (dict(bbox_regression=reg[:1]), RuntimeError, "one map per level"),
                            (dict(bbox_regression=[reg[0], torch.zeros(2, 20, 2, 2)]), RuntimeError, "channels for 6 anchors"),
                            (dict(scores=sc[:, :, :70]), RuntimeError, "scores should have shape"), (dict(scores=sc.double()), TypeError, "float32"),
                            (dict(scores=sc[:, :1]), ValueError, "at least 2 classes"), (dict(idx=idx.long()), RuntimeError, "int32"),
                            (dict(steps=[8]), ValueError, "steps"), (dict(steps=[8, 0]), ValueError, "steps"), (dict(batch_size=(0, 4)), ValueError, "batch_size"),
                            (dict(weights=(1.0, 1.0)), ValueError, "four weights"), (dict(image_sizes=[(30, 40)]), RuntimeError, "image_sizes"),
                            (dict(), _lib.Mi355VisionError, "no CPU")):
        with pytest.raises(exc, match=text):
            F.ssd_decode(**{**ok, **over})


# ------------------------------------------------------------------------------------------------ numerics of the stated arithmetics
def _l2_inputs():
    g = torch.Generator().manual_seed(9100)
    a = torch.randn((2, 512, 9, 7), generator=g)
    b = torch.randn((1, 3, 4, 4), generator=g) + 100.0
    c = torch.randn((1, 64, 5, 5), generator=g)
    c[0, :, 2, 3] = 0.0
    return {"N(0,1) C=512": a, "N(100,1) C=3": b, "C=64, a zero pixel": c}


@pytest.mark.parametrize("name", list(_l2_inputs()))
def test_l2_norm_restatement_is_at_least_as_accurate_as_torch(name):
    """The condition is the project's form: max |restatement - f64| <= 2 max |torch f32 - f64| + 2^-22 max |f64|.  Measured on these
    inputs (restatement / torch in units of 2^-24 max |f64|, then the greatest ulp distance of the two): 1.99 / 4.10, 7;  1.65 / 1.32, 2;
    1.15 / 2.17, 4.  Ulp equality with torch is not asserted: torch's float32 sum is the less accurate one."""
    x = _l2_inputs()[name]
    w = torch.randn(x.shape[1], generator=torch.Generator().manual_seed(5)) * 3 + 20
    got = R.l2_normalize_scale(x, w)
    t32 = w.view(1, -1, 1, 1) * nn.functional.normalize(x)
    f64 = w.double().view(1, -1, 1, 1) * nn.functional.normalize(x.double())
    scale = float(f64.abs().max())
    e_re, e_t = float((got.double() - f64).abs().max()), float((t32.double() - f64).abs().max())
    print(f"l2 norm {name}: restatement {e_re / scale * 2 ** 24:.2f}, torch {e_t / scale * 2 ** 24:.2f} (x 2^-24 max|f64|), "
          f"max ulp distance restatement / torch {int(R.ulp_distance(got, t32)[(got != 0) & (t32 != 0)].max())}")
    assert e_re <= 2 * e_t + 2.0 ** -22 * scale
    if "zero" in name:
        assert torch.equal(got[0, :, 2, 3], torch.zeros(64)) and not bool(torch.isnan(got).any())


@pytest.mark.parametrize("classes,sigma", [(2, 1.0), (21, 1.0), (91, 1.0), (91, 4.0)])
def test_softmax_restatement_is_at_least_as_accurate_as_torch(classes, sigma):
    """The same form of condition for mv_ssd_scores_f32's softmax (float32 exponentials, one float64 chain, the float64 division) against
    torch.softmax and float64.  D, the greatest ulp distance between the two float32 results on these inputs, is printed; DESIGN
    3.31 records the figures.  The float32 chain of k_roi_detections (tests/_roi_heads_ref.softmax_chain) is printed beside it: at
    K = 91, sigma = 4 its error is 13.15 x 2^-24 max|f64| against 2 x 4.00 + 4 = 12.0 allowed, which is why this kernel sums in float64."""
    g = torch.Generator().manual_seed(9200 + classes)
    x = torch.randn((4000, classes), generator=g) * sigma
    got, t32, f64 = R.softmax_f64sum(x), torch.softmax(x, -1), torch.softmax(x.double(), -1)
    scale = float(f64.abs().max())
    e_re, e_t = float((got.double() - f64).abs().max()), float((t32.double() - f64).abs().max())
    d = int(R.ulp_distance(got, t32).max())
    e_chain = float((R.RH.softmax_chain(x).double() - f64).abs().max())
    print(f"softmax K={classes} sigma={sigma}: restatement {e_re / scale * 2 ** 24:.2f}, torch {e_t / scale * 2 ** 24:.2f}, a float32 chain "
          f"{e_chain / scale * 2 ** 24:.2f} (x 2^-24 max|f64|), D = {d} ulp")
    assert e_re <= 2 * e_t + 2.0 ** -22 * scale


# ------------------------------------------------------------------------------------------------ selection: replica against restatement
GRIDS = [(5, 4), (3, 3), (1, 1)]
RATIOS = [[2], [2, 3], [2]]
IMAGE = (40, 32)
SIZES = [(40, 32), (37, 30)]


def _maps(classes, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    anchors = [4, 6, 4]
    cls = [torch.randn((2, a * classes, h, w), generator=g) * scale for a, (h, w) in zip(anchors, GRIDS)]
    reg = [torch.randn((2, a * 4, h, w), generator=g) for a, (h, w) in zip(anchors, GRIDS)]
    return cls, reg


@pytest.mark.parametrize("classes,k,thresh", [(2, 30, 0.3), (21, 12, 0.05), (91, 5, 0.02)])
def test_selection_replica_against_restatement(classes, k, thresh):
    """The replica (torch.softmax, torch.exp, torch.topk, the loop over the labels) and the restatement select the same anchors per
    (image, class), apart from candidates whose restated score lies within D ulp (the measured distance of the two softmaxes on these
    inputs) of the threshold or of the k-th score: at most 1 % of the candidates, which the restatement's own count of such scores
    stays under.  Boxes of common candidates differ by the two exps only: exp enters as fl(E(dw) w) / 2 on either side of the
    centre, a 1-ulp difference of E moves a corner by at most 2^-23 of the box's half side plus one rounding of the corner, and the
    boxes are clipped to an image of at most 40 pixels with sides below 2^8 before the clip for these deltas: 2^-14 in absolute terms
    is a generous bound of it (the measured maximum is printed).  Measured: K = 2 / 21 / 91: D = 2 / 4 / 4 ulp, 60 / 480 / 900 candidates,
    none set aside, no restated score at a boundary, box differences up to 1.9e-6."""
    cls, reg = _maps(classes, 9300 + classes)
    gen = R.DefaultBoxGenerator(RATIOS)
    images = R.ImageList(torch.zeros(2, 3, *IMAGE), SIZES)
    anchors = gen(images, cls)
    rep = R.SSD(None, gen, IMAGE, classes, head=nn.Identity(), score_thresh=thresh, topk_candidates=k)
    head_outputs = {"cls_logits": torch.cat([R.permute_level(m, classes) for m in cls], dim=1),
                    "bbox_regression": torch.cat([R.permute_level(m, 4) for m in reg], dim=1)}
    replica = rep.candidates(head_outputs, anchors, SIZES)
    sc = R.scores(cls, classes)
    d = int(R.ulp_distance(sc, R.scores(cls, classes, softmax=R.RH.softmax_torch)).max())
    idx = R.select(sc, k, thresh)
    boxes, _, labels, valid = R.decode(sc, reg, idx, R.default_boxes(gen, GRIDS, IMAGE), SIZES)
    t32 = torch.tensor(thresh, dtype=torch.float32)
    total = aside = near = 0
    worst = 0.0
    for i in range(2):
        rb, rs, rl, ra = replica[i]
        for c in range(1, classes):
            seg = idx[i, (c - 1) * k:c * k]
            # (the lambda below is called within this iteration only)
            mine = {int(f) // classes: j for j, f in enumerate(seg.tolist()) if f >= 0}
            theirs = {int(a): j for j, a in enumerate(ra[rl == c].tolist())}
            row = sc[i, c]
            last = sorted(mine, key=lambda a: mine[a])[-1] if len(mine) == k else None  # the k-th: a boundary when the segment is full
            edge = lambda a: int(R.ulp_distance(row[a], t32)) <= d or (last is not None and int(R.ulp_distance(row[a], row[last])) <= d)  # noqa: E731
            total += len(mine)
            near += sum(1 for a in range(row.numel()) if a != last and edge(a))
            for a in set(mine) ^ set(theirs):
                assert edge(a), f"image {i} class {c} anchor {a}: selected by one side only, and not at a boundary"
                aside += 1
            rbox = rb[rl == c]
            for a in set(mine) & set(theirs):
                worst = max(worst, float((boxes[i, (c - 1) * k + mine[a]] - rbox[theirs[a]]).abs().max()))
    print(f"selection K={classes}: D = {d} ulp, {total} candidates, {aside} set aside, {near} restated scores at a boundary, "
          f"max box difference {worst:.3g}")
    assert total > 50 and near <= 0.01 * total and aside <= 0.01 * total
    assert worst <= 2.0 ** -14
    assert bool(valid.any()) and bool((labels[valid] >= 1).all())
