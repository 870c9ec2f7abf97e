"""SSDlite without a device: the module tree and the seeded initialisation of ssdlite320_mobilenet_v3_large against the replica
(tests/_ssdlite_ref.py) and against the keys and shapes the reference's model is known to have, the defaults, every argument error,
the freezing, the channels read off the modules against the replica's probing forward, the default boxes, and the refusals of
F.dwconv_pointwise and mv_dwconv3x3_conv1x1_f32 that need no device (host pointers: nothing is launched)."""
import warnings
from functools import partial

import pytest
import torch
from torch import nn

import cpu_vision_amd as mv
from cpu_vision_amd import _lib
from cpu_vision_amd import functional as F
from cpu_vision_amd import ssd as S
from cpu_vision_amd import ssdlite as SL
from cpu_vision_amd.anchor_utils import DefaultBoxGenerator
from tests import _ssd_ref as R
from tests import _ssdlite_ref as RL

K = 5
LITERAL_SHAPES = {
    "backbone.features.0.13.0.weight": (672, 112, 1, 1),
    "backbone.features.1.0.1.0.weight": (672, 1, 5, 5),
    "backbone.features.1.0.3.0.weight": (80, 672, 1, 1),
    "backbone.features.1.3.0.weight": (480, 80, 1, 1),
    "backbone.extra.0.0.0.weight": (256, 480, 1, 1),
    "backbone.extra.0.1.0.weight": (256, 1, 3, 3),
    "backbone.extra.0.2.0.weight": (512, 256, 1, 1),
    "head.classification_head.module_list.0.0.0.weight": (672, 1, 3, 3),
    "head.classification_head.module_list.0.1.weight": (6 * K, 672, 1, 1),
    "head.classification_head.module_list.0.1.bias": (6 * K,),
}


@pytest.fixture(scope="module")
def models():
    torch.manual_seed(11)
    mine = mv.ssdlite320_mobilenet_v3_large(num_classes=K)
    torch.manual_seed(11)
    ref = RL.ssdlite320_mobilenet_v3_large(num_classes=K)
    return mine, ref


# ------------------------------------------------------------------------------------------------ the module tree
def test_state_dict_keys_and_seeded_init(models):
    mine, ref = models
    a, b = mine.state_dict(), ref.state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    for k, shape in LITERAL_SHAPES.items():
        assert k in a and tuple(a[k].shape) == shape, k
    assert "backbone.features.1.0.2.fc1.weight" in a
    assert [n for n, _ in mine.named_children()] == ["backbone", "anchor_generator", "head", "transform"]
    assert [n for n, _ in mine.backbone.named_children()] == ["features", "extra"]
    assert [n for n, _ in mine.head.named_children()] == ["classification_head", "regression_head"]
    assert len(mine.backbone.features) == 2 and len(mine.backbone.features[0]) == 14 and len(mine.backbone.extra) == 4
    assert mine.head.classification_head.num_columns == K and mine.head.regression_head.num_columns == 4
    assert [b_[1].out_channels for b_ in mine.head.classification_head.module_list] == [6 * K] * 6
    assert [b_[1].out_channels for b_ in mine.head.regression_head.module_list] == [24] * 6
    assert [b_[0][0].in_channels for b_ in mine.head.regression_head.module_list] == [672, 480, 512, 256, 256, 128]
    # _normal_init: every conv N(0, 0.03), every conv bias 0; the norms keep MobileNetV3's ones and zeros
    w = a["backbone.extra.1.2.0.weight"]
    assert abs(float(w.std()) - 0.03) < 0.003 and abs(float(w.mean())) < 0.003
    assert float(a["head.classification_head.module_list.3.1.bias"].abs().max()) == 0.0
    assert torch.equal(a["backbone.features.0.0.1.weight"], torch.ones(16))
    bn = mine.head.regression_head.module_list[0][0][1]
    assert isinstance(bn, nn.BatchNorm2d) and bn.eps == 0.001 and bn.momentum == 0.03


def test_defaults_and_attributes(models):
    mine, ref = models
    assert (mine.score_thresh, mine.nms_thresh, mine.detections_per_img, mine.topk_candidates) == (0.001, 0.55, 300, 300)
    assert (ref.score_thresh, ref.nms_thresh, ref.detections_per_img, ref.topk_candidates) == (0.001, 0.55, 300, 300)
    t = mine.transform
    assert t.fixed_size == (320, 320) and t.size_divisible == 1 and t.image_mean == [0.5] * 3 and t.image_std == [0.5] * 3
    g = mine.anchor_generator
    assert g.steps is None and g.clip is True and g.num_anchors_per_location() == [6] * 6
    assert g.scales == RL.ssdlite_generator().scales and g.scales[0] == 0.2 and abs(g.scales[5] - 0.95) < 1e-12 and g.scales[6] == 1.0
    assert not mine.training and not mine.backbone.training and not mine.head.training
    assert mv.ssdlite320_mobilenet_v3_large.__kwdefaults__ == {"weights": None, "progress": True, "num_classes": None, "weights_backbone": None,
                                                               "trainable_backbone_layers": None, "norm_layer": None}
    assert all(p.requires_grad for p in mine.parameters())  # six trainable layers: nothing frozen
    m91 = SL.SSDLiteHead([16], [6], 91, partial(nn.BatchNorm2d, eps=0.001))
    assert m91.classification_head.module_list[0][1].out_channels == 546


def test_argument_errors(models, monkeypatch):
    mine, _ = models
    with pytest.raises(ValueError, match="no weight files"):
        mv.ssdlite320_mobilenet_v3_large(weights="DEFAULT")
    with pytest.raises(ValueError, match="no weight files"):
        mv.ssdlite320_mobilenet_v3_large(weights_backbone="DEFAULT")
    norm = RL.default_norm_layer()
    with pytest.raises(AssertionError, match=r"trainable_layers should be in the range \[0, 6\]. Instead got 7"):
        SL._mobilenet_extractor(mv.mobilenet_v3_large(reduced_tail=True), 7, norm)
    with pytest.raises(AssertionError, match=r"trainable_layers should be in the range \[0, 6\]. Instead got -1"):
        SL._mobilenet_extractor(mv.mobilenet_v3_large(reduced_tail=True), -1, norm)
    feats = mv.mobilenet_v3_large(reduced_tail=True).features
    assert feats[14].use_res_connect and not feats[13].use_res_connect
    with pytest.raises(ValueError, match=r"backbone\[c4_pos\].use_res_connect should be False"):
        mv.SSDLiteFeatureExtractorMobileNet(feats, 14, norm)
    # the channels / aspect-ratio mismatch: SSD's own check through the channels read off the modules, and the builder's
    with pytest.raises(ValueError, match=r"output channels from the backbone \(6\) do not match .* aspect ratios \(5\)"):
        S.SSD(mine.backbone, DefaultBoxGenerator([[2, 3]] * 5), (320, 320), 3)
    monkeypatch.setattr(SL, "DefaultBoxGenerator", lambda ratios, **kw: DefaultBoxGenerator(ratios[:4], **kw))
    with pytest.raises(ValueError, match="output channels from the backbone 6 do not match the length of the anchor generator aspect ratios 4"):
        mv.ssdlite320_mobilenet_v3_large(num_classes=2)
    monkeypatch.undo()
    x = [torch.rand(3, 20, 30)]
    with pytest.raises(RuntimeError, match="inference only"):
        mine(x, targets=[{}])
    mine.train()
    try:
        with pytest.raises(RuntimeError, match="inference only"):
            mine(x)
        with pytest.raises(RuntimeError, match="inference only"):
            mine.backbone(torch.zeros(1, 3, 32, 32))
        with pytest.raises(RuntimeError, match="inference only"):
            mine.head.classification_head([torch.zeros(1, 672, 3, 3)])
    finally:
        mine.eval()
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):  # no fallback: a CPU tensor is refused
        mine(x)


def test_size_keyword_is_ignored_with_a_warning():
    torch.manual_seed(1)
    with pytest.warns(UserWarning, match="The size of the model is already fixed; ignoring the parameter."):
        m = mv.ssdlite320_mobilenet_v3_large(num_classes=2, size=(512, 512))
    assert m.transform.fixed_size == (320, 320)
    with pytest.warns(UserWarning, match="falling back to trainable_backbone_layers=6"):
        m = mv.ssdlite320_mobilenet_v3_large(num_classes=2, trainable_backbone_layers=9)  # without weights: falls back to 6, as the reference
    assert all(p.requires_grad for p in m.parameters())


@pytest.mark.parametrize("layers,first_trainable", [(0, None), (3, 7), (6, 0)])
def test_mobilenet_extractor_freezes(layers, first_trainable):
    """stage_indices of MobileNetV3-Large are [0, 2, 4, 7, 13, 16]: everything before stage_indices[6 - layers] is frozen, everything
    (of the backbone's own features) when layers == 0; the extra blocks are never frozen; c4_pos is 13."""
    feats = mv.mobilenet_v3_large(reduced_tail=True)
    assert [0] + [i for i, b in enumerate(feats.features) if getattr(b, "_is_cn", False)] + [len(feats.features) - 1] == [0, 2, 4, 7, 13, 16]
    params = [[p for p in b.parameters()] for b in feats.features]
    ext = SL._mobilenet_extractor(feats, layers, RL.default_norm_layer())
    for i, ps in enumerate(params):
        frozen = first_trainable is None or i < first_trainable
        assert all(p.requires_grad != frozen for p in ps), (layers, i)
    assert all(p.requires_grad for p in ext.extra.parameters())
    assert len(ext.features[0]) == 14 and ext.features[0][13] is feats.features[13].block[0]
    replica = RL._mobilenet_extractor(RL.mobilenet_v3_large(), layers, RL.default_norm_layer())
    assert [n for n, p in ext.named_parameters() if not p.requires_grad] == [n for n, p in replica.named_parameters() if not p.requires_grad]


def test_out_channels_read_off_the_modules_equal_the_probing_forward(models):
    mine, ref = models
    assert S._retrieve_out_channels(mine.backbone, (320, 320)) == R.retrieve_out_channels(ref.backbone, (320, 320)) == [672, 480, 512, 256, 256, 128]
    with torch.no_grad():
        shapes = [tuple(v.shape) for v in ref.backbone.eval()(torch.zeros(1, 3, 320, 320)).values()]
    assert shapes == [(1, 672, 20, 20), (1, 480, 10, 10), (1, 512, 5, 5), (1, 256, 3, 3), (1, 256, 2, 2), (1, 128, 1, 1)]
    norm = RL.default_norm_layer()
    small = mv.SSDLiteFeatureExtractorMobileNet(mv.mobilenet_v3_large(width_mult=0.25, reduced_tail=True).features, 13, norm, width_mult=0.25)
    small_ref = RL.SSDLiteFeatureExtractorMobileNet(RL.mobilenet_v3_large(width_mult=0.25).features, 13, norm, width_mult=0.25)
    got = S._retrieve_out_channels(small, (128, 96))
    assert got == R.retrieve_out_channels(small_ref, (128, 96))
    assert got[2:] == [128, 64, 64, 32] and small.extra[3][0].out_channels == 16  # min_depth engages: int(128 * 0.25) // 2 = 16
    tiny = mv.SSDLiteFeatureExtractorMobileNet(mv.mobilenet_v3_large(width_mult=0.25, reduced_tail=True).features, 13, norm, width_mult=0.05)
    tiny_ref = RL.SSDLiteFeatureExtractorMobileNet(RL.mobilenet_v3_large(width_mult=0.25).features, 13, norm, width_mult=0.05)
    assert S._retrieve_out_channels(tiny, (128, 96)) == R.retrieve_out_channels(tiny_ref, (128, 96))
    assert S._retrieve_out_channels(tiny, (128, 96))[2:] == [25, 16, 16, 16]
    assert list(small.state_dict()) == list(small_ref.state_dict())


def test_default_boxes_at_320(models):
    mine, ref = models
    grids = [(20, 20), (10, 10), (5, 5), (3, 3), (2, 2), (1, 1)]
    maps = [torch.zeros(1, 1, h, w) for h, w in grids]
    images = R.ImageList(torch.zeros(1, 3, 320, 320), [(320, 320)])
    got, want = mine.anchor_generator(images, maps)[0], ref.anchor_generator(images, maps)[0]
    assert got.shape == (3234, 4) and torch.equal(got, want)
    assert torch.equal(got, R.default_boxes(mine.anchor_generator, grids, (320, 320)))


# ------------------------------------------------------------------------------------------------ host-side refusals
def _refused(rc, text, code=-1):
    msg = _lib.load().mv_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_dwconv3x3_conv1x1_refusals():
    lib = _lib.load()
    MB = 1 << 20
    base = dict(x=1 * MB, w_dw=2 * MB, bias_dw=None, alpha_dw=3 * MB, beta_dw=4 * MB, w=5 * MB, bias=6 * MB, alpha=None, beta=None, res=7 * MB,
                y=8 * MB, n=2, cin=8, h=5, wd=7, cout=12, stride=1, affine_dw=2, act_dw=2, affine=0, act=0)

    def call(**over):
        a = {**base, **over}
        return lib.mv_dwconv3x3_conv1x1_f32(a["x"], a["w_dw"], a["bias_dw"], a["alpha_dw"], a["beta_dw"], a["w"], a["bias"], a["alpha"], a["beta"],
                                            a["res"], a["y"], a["n"], a["cin"], a["h"], a["wd"], a["cout"], a["stride"], a["affine_dw"], a["act_dw"],
                                            a["affine"], a["act"], None)
    _refused(call(n=-1), "bad conv shape")
    _refused(call(cin=0), "bad conv shape")
    _refused(call(cout=0), "bad conv shape")
    _refused(call(h=0), "bad conv shape")
    _refused(call(wd=-2), "bad conv shape")
    _refused(call(stride=0), "stride should be 1 or 2 instead of 0")
    _refused(call(stride=3), "stride should be 1 or 2 instead of 3")
    _refused(call(affine_dw=3), "bad depthwise affine (3)")
    _refused(call(act_dw=5), "bad depthwise affine (2) / activation (5)")
    _refused(call(affine=-1), "bad affine (-1)")
    _refused(call(act=7), "activation (7)")
    for name in ("x", "w_dw", "w", "y"):
        _refused(call(**{name: None}), "null pointer")
    _refused(call(alpha_dw=None), "depthwise affine without alpha / beta")
    _refused(call(beta_dw=None), "depthwise affine without alpha / beta")
    _refused(call(affine=1), "affine without alpha / beta")
    _refused(call(affine=2, alpha=9 * MB), "affine without alpha / beta")
    ny = 2 * 12 * 5 * 7 * 4
    _refused(call(y=1 * MB), "must not overlap")                        # x itself
    _refused(call(y=1 * MB + 2 * 8 * 5 * 7 * 4 - 4), "must not overlap")  # the last element of x
    _refused(call(y=2 * MB - ny + 4), "must not overlap")               # the first element of w_dw
    _refused(call(y=3 * MB + 28), "must not overlap")                   # alpha_dw
    _refused(call(y=4 * MB - 8), "must not overlap")                    # beta_dw
    _refused(call(y=5 * MB + 4 * 95), "must not overlap")               # the last element of w
    _refused(call(y=6 * MB + 44), "must not overlap")                   # bias
    _refused(call(y=7 * MB + 16), "must not overlap")                   # the residual
    _refused(call(res=8 * MB), "must not overlap")                      # the residual is no in-place operand
    _refused(call(affine=2, alpha=8 * MB + 64, beta=9 * MB), "must not overlap")
    _refused(call(cin=1 << 16, h=1 << 8, wd=1 << 7), "32-bit index", code=-2)
    # what the pointwise conv refuses: a batch beyond the launch grid, a plane beyond the pixel index (far pointers: no overlap)
    far = dict(x=1 << 40, w_dw=2 << 40, alpha_dw=3 << 40, beta_dw=4 << 40, w=5 << 40, bias=6 << 40, res=7 << 40, y=8 << 40)
    _refused(call(n=65536, **far), "too large for one launch", code=-2)
    _refused(call(n=1, cin=1, h=512, wd=(1 << 22) - 1, **far), "plane too large", code=-2)  # 2^31 - 512 pixels: inside the int range
    assert call(n=0, x=None, w_dw=None, w=None, y=None) == 0


def test_dwconv_pointwise_refusals():
    x, dw, w = torch.zeros(2, 8, 5, 7), torch.zeros(8, 1, 3, 3), torch.zeros(12, 8, 1, 1)
    ones8, ones12 = torch.ones(8), torch.ones(12)
    with pytest.raises(ValueError, match="needs the pointwise"):
        F.dwconv_pointwise(x, dw)
    with pytest.raises(RuntimeError, match="Expected 4D"):
        F.dwconv_pointwise(x[0], dw, weight=w)
    with pytest.raises(RuntimeError, match="Expected 4D"):
        F.dwconv_pointwise(x, dw, weight=w[:, :, 0, 0])
    for bad in (torch.zeros(8, 1, 5, 5), torch.zeros(7, 1, 3, 3), torch.zeros(8, 8, 3, 3)):
        with pytest.raises(NotImplementedError, match=r"dw_weight should have shape \(8, 1, 3, 3\)"):
            F.dwconv_pointwise(x, bad, weight=w)
    for bad in (torch.zeros(12, 8, 3, 3), torch.zeros(12, 7, 1, 1)):
        with pytest.raises(NotImplementedError, match="pointwise 1x1"):
            F.dwconv_pointwise(x, dw, weight=bad)
    for stride in (0, 3, 1.5):
        with pytest.raises(ValueError, match="stride should be 1 or 2"):
            F.dwconv_pointwise(x, dw, weight=w, stride=stride)
    with pytest.raises(ValueError, match="unknown activation 'gelu'"):
        F.dwconv_pointwise(x, dw, weight=w, activation="gelu")
    with pytest.raises(ValueError, match="affine 'bn'"):
        F.dwconv_pointwise(x, dw, weight=w, affine="bn")
    with pytest.raises(ValueError, match="unknown dw_activation 'tanh'"):
        F.dwconv_pointwise(x, dw, weight=w, dw_activation="tanh")
    with pytest.raises(ValueError, match="dw_affine 'x'"):
        F.dwconv_pointwise(x, dw, weight=w, dw_affine="x")
    with pytest.raises(ValueError, match="dw_affine='fma' needs dw_alpha and dw_beta"):
        F.dwconv_pointwise(x, dw, None, ones8, None, w, dw_affine="fma")
    with pytest.raises(ValueError, match="affine='mul_add' needs alpha and beta"):
        F.dwconv_pointwise(x, dw, weight=w, beta=ones12, affine="mul_add")
    with pytest.raises(RuntimeError, match="dw_bias has 12 elements for 8 depthwise channels"):
        F.dwconv_pointwise(x, dw, ones12, weight=w)
    with pytest.raises(RuntimeError, match="dw_alpha has 12 elements"):
        F.dwconv_pointwise(x, dw, None, ones12, ones8, w, dw_affine="fma")
    with pytest.raises(RuntimeError, match="bias has 8 elements for 12 output channels"):
        F.dwconv_pointwise(x, dw, weight=w, bias=ones8)
    with pytest.raises(RuntimeError, match=r"residual of shape \(2, 12, 5, 7\) does not match the output \(2, 12, 3, 4\)"):
        F.dwconv_pointwise(x, dw, weight=w, residual=torch.zeros(2, 12, 5, 7), stride=2)
    with pytest.raises(TypeError):
        F.dwconv_pointwise(x, dw, None, None, None, w, None, None, None, None, 2)  # stride and the codes are keyword-only
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.dwconv_pointwise(x, dw, weight=w)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        mv.SSDLiteHead([8], [6], 3, RL.default_norm_layer())([x])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert F.dwconv_pointwise is mv.functional.dwconv_pointwise
