"""LRASPP and DeepLabV3-MobileNetV3 without a GPU: trees, state-dict keys and seeded initialisation of the two builders against the
torch replicas of tests/_lraspp_ref.py, argument errors, the refusals of mv_dwconv_dilated_norm_act_f32 and
mv_conv1x1_gated_upsample_f32 (they return before any launch), what stays pinned (dense dilated convs, the dilated classification
forward), and the checks of the GPU tests' own oracles: the zero-stuffed form of the dilated depthwise conv against the oracle's
dilated conv, and the stage-by-stage forward against torch's float32 forward."""
import numpy as np
import pytest
import torch

import cpu_vision_amd as mv
from cpu_vision_amd import _lib, mobilenet, segmentation
from cpu_vision_amd import functional as F
from tests import _lraspp_ref as R

BUILDERS = [("lraspp_mobilenet_v3_large", {}), ("deeplabv3_mobilenet_v3_large", {}), ("deeplabv3_mobilenet_v3_large", {"aux_loss": True})]


def _tree(m):
    return [(n, type(c).__name__.lstrip("T")) for n, c in m.named_modules() if isinstance(c, (torch.nn.Conv2d, torch.nn.BatchNorm2d,
                                                                                             torch.nn.Linear))]


@pytest.mark.parametrize("name,kw", BUILDERS, ids=["lraspp", "deeplabv3", "deeplabv3-aux"])
def test_builders_match_the_replicas(name, kw):
    torch.manual_seed(11)
    got = getattr(mv, name)(num_classes=5, **kw)
    torch.manual_seed(11)
    want = R.replica(name, num_classes=5, **kw)
    gs, ws = got.state_dict(), want.state_dict()
    assert list(gs) == list(ws)
    for k in gs:
        assert gs[k].shape == ws[k].shape and torch.equal(gs[k], ws[k]), k  # the same draws in the same order
    assert _tree(got) == _tree(want)
    assert not got.training
    got.load_state_dict(ws)
    assert getattr(segmentation, name) is getattr(mv, name) and name in segmentation.__all__
    if name.startswith("lraspp"):
        assert isinstance(got, mv.LRASPP) and isinstance(got.classifier, mv.LRASPPHead)
        assert got.backbone.return_layers == {"4": "low", "16": "high"}
        assert got.classifier.low_classifier.in_channels == 40 and got.classifier.cbr[0].in_channels == 960
        assert got.classifier.cbr[0].out_channels == 128 and got.classifier.high_classifier.out_channels == 5
    else:
        assert isinstance(got, mv.DeepLabV3) and (got.aux_classifier is not None) == bool(kw)
        assert got.classifier[0].convs[0][0].in_channels == 960


def test_stage_indices_and_defaults():
    feats = mv.mobilenet_v3_large(dilated=True).features
    idx = [0] + [i for i, b in enumerate(feats) if getattr(b, "_is_cn", False)] + [len(feats) - 1]
    assert idx == R.STAGE_INDICES == R.stage_indices(R.MR.replica("mobilenet_v3_large", dilated=True).features)
    m = mv.lraspp_mobilenet_v3_large()
    assert m.classifier.high_classifier.out_channels == 21 and m.backbone.return_layers == {"4": "low", "16": "high"}
    assert list(m.backbone) == [str(i) for i in range(17)]
    d = mv.deeplabv3_mobilenet_v3_large(aux_loss=True)
    assert d.classifier[4].out_channels == 21 and d.backbone.return_layers == {"16": "out", "4": "aux"}
    assert d.aux_classifier[0].in_channels == 40


def test_argument_errors():
    for build in (mv.lraspp_mobilenet_v3_large, mv.deeplabv3_mobilenet_v3_large):
        with pytest.raises(ValueError, match="ships no weight files"):
            build(weights="DEFAULT")
        with pytest.raises(ValueError, match="ships no weight files"):
            build(weights_backbone="IMAGENET1K_V1")
    with pytest.raises(NotImplementedError, match="This model does not use auxiliary loss"):
        mv.lraspp_mobilenet_v3_large(aux_loss=True)
    mv.lraspp_mobilenet_v3_large(aux_loss=False, num_classes=2)
    x = torch.zeros(1, 3, 32, 32)
    for m in (mv.lraspp_mobilenet_v3_large(num_classes=2), mv.LRASPPHead(4, 8, 3, 6)):
        m.train()
        with pytest.raises(RuntimeError, match="inference only"):
            m(x if isinstance(m, mv.LRASPP) else {"low": x, "high": x})
    m = mv.lraspp_mobilenet_v3_large(num_classes=2).train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.labels(x)
    xs = torch.zeros(1, 8, 6, 6)
    for w, kw in ((torch.zeros(8, 1, 3, 3), dict(groups=8)), (torch.zeros(4, 8, 1, 1), {}), (torch.zeros(8, 1, 5, 5), dict(groups=8, stride=2))):
        with pytest.raises(NotImplementedError, match="dilation 2"):
            F.conv_norm_act(xs, w, dilation=2, **kw)
    with pytest.raises(NotImplementedError, match="dilation 3"):
        F.conv_norm_act(xs, torch.zeros(8, 1, 5, 5), groups=8, dilation=3)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="dilation"):
            F.conv_norm_act(xs, torch.zeros(8, 1, 5, 5), groups=8, dilation=bad)
    with pytest.raises(NotImplementedError, match="dilation 2"):
        F.conv_norm_act(xs, torch.zeros(8, 1, 7, 7), groups=8, dilation=2)
    with pytest.raises(_lib.Mi355VisionError):  # no CPU fallback
        F.conv_norm_act(xs, torch.zeros(8, 1, 5, 5), groups=8, dilation=2)
    g, w = torch.zeros(1, 8), torch.zeros(3, 8, 1, 1)
    with pytest.raises(_lib.Mi355VisionError):
        F.conv1x1_gated_upsample(xs, g, w, size=(9, 9))
    with pytest.raises(RuntimeError, match="input_scale should have shape"):
        F.conv1x1_gated_upsample(xs, torch.zeros(1, 7), w, size=(9, 9))
    with pytest.raises(NotImplementedError, match="pointwise 1x1"):
        F.conv1x1_gated_upsample(xs, g, torch.zeros(3, 8, 3, 3), size=(9, 9))
    with pytest.raises(ValueError, match="either size or scale_factor"):
        F.conv1x1_gated_upsample(xs, g, w)
    with pytest.raises(ValueError, match="greater than 0"):
        F.conv1x1_gated_upsample(xs, g, w, size=(0, 4))
    with pytest.raises(RuntimeError, match="Expected 4D"):
        F.conv1x1_gated_upsample(xs[0], g, w, size=(9, 9))


def _refused(rc, text, code=-1):
    msg = _lib.load().mv_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_abi_refusals_without_a_device():
    """Every call is refused (or is the n == 0 no-op) before a launch: the pointers are host integers that are never dereferenced."""
    lib = _lib.load()
    X, W, Y, G = 1 << 40, 2 << 40, 3 << 40, 4 << 40  # far enough apart for every shape below
    keys = ("x", "w", "b", "al", "be", "r", "y", "n", "c", "h", "wd", "k", "s", "d", "af", "act")
    base = dict(x=X, w=W, b=None, al=None, be=None, r=None, y=Y, n=1, c=4, h=6, wd=6, k=5, s=1, d=2, af=0, act=0)
    dw = lambda **o: lib.mv_dwconv_dilated_norm_act_f32(*[{**base, **o}[k] for k in keys], None)  # noqa: E731
    _refused(dw(d=0), "dilation should be at least 1")
    _refused(dw(d=-2), "dilation should be at least 1")
    _refused(dw(k=3), "kernel 5, dilation 2, stride 1", -2)
    _refused(dw(s=2), "kernel 5, dilation 2, stride 1", -2)
    _refused(dw(d=3), "kernel 5, dilation 2, stride 1", -2)
    _refused(dw(k=7), "kernel 5, dilation 2, stride 1", -2)
    _refused(dw(n=-1), "bad conv shape")
    _refused(dw(h=0), "bad conv shape")
    _refused(dw(s=3), "stride should be 1 or 2")
    _refused(dw(act=5), "activation")
    _refused(dw(x=None), "null pointer")
    _refused(dw(w=None), "null pointer")
    _refused(dw(af=2), "affine without alpha / beta")
    _refused(dw(y=X), "alias")
    assert dw(n=0) == 0 and dw(n=0, x=None, y=None) == 0
    # dilation 1 is mv_dwconv_norm_act_f32: its refusals, texts and order (tests/test_mobilenetv3_host.py)
    for o, text, code in ((dict(k=7), "kernel 3 or 5", -2), (dict(k=4), "kernel 3 or 5", -2), (dict(n=-1), "bad conv shape", -1),
                          (dict(c=0), "bad conv shape", -1), (dict(s=3), "stride should be 1 or 2", -1), (dict(act=5), "activation", -1),
                          (dict(af=3), "affine", -1), (dict(x=None), "null pointer", -1), (dict(af=2), "affine without alpha / beta", -1),
                          (dict(y=X), "alias", -1), (dict(k=3, s=3), "stride should be 1 or 2", -1), (dict(k=3, x=None), "null pointer", -1),
                          (dict(k=7, n=-1), "bad conv shape", -1), (dict(k=7, s=3), "stride should be 1 or 2", -1)):
        rc_new = dw(d=1, **o)
        new = lib.mv_last_error().decode()
        a = {**base, **o}
        rc_old = lib.mv_dwconv_norm_act_f32(*[a[k] for k in keys if k != "d"], None)
        assert rc_new == rc_old == code and new == lib.mv_last_error().decode() and text in new, (o, rc_new, rc_old, new)
    assert dw(d=1, n=0) == 0 and dw(d=1, n=0, k=3) == 0

    gk = ("x", "g", "w", "b", "r", "y", "n", "ci", "h", "wd", "oh", "ow", "co")
    gb = dict(x=X, g=G, w=W, b=None, r=None, y=Y, n=1, ci=4, h=6, wd=6, oh=9, ow=11, co=5)
    gu = lambda **o: lib.mv_conv1x1_gated_upsample_f32(*[{**gb, **o}[k] for k in gk], None)  # noqa: E731
    for k in ("x", "g", "w", "y"):
        _refused(gu(**{k: None}), "null pointer")
    for k in ("ci", "co", "h", "wd", "oh", "ow"):
        _refused(gu(**{k: 0}), "bad conv shape")
    _refused(gu(n=-1), "bad conv shape")
    _refused(gu(y=X + 16), "must not overlap")
    _refused(gu(y=G), "must not overlap")
    _refused(gu(y=W + 4), "must not overlap")
    _refused(gu(r=Y + 4), "must not overlap")
    _refused(gu(r=Y - 4), "must not overlap")
    _refused(gu(n=65536), "too large", -2)
    _refused(gu(oh=65536, ow=65536), "too large", -2)
    _refused(gu(h=65536, wd=65536), "too large", -2)
    assert gu(n=0) == 0 and gu(n=0, x=None, g=None, w=None, y=None) == 0


def test_what_stays_pinned():
    conv = torch.nn.Conv2d(4, 4, 3, padding=2, dilation=2)  # a dense dilated conv
    with pytest.raises(NotImplementedError, match="dilation 1"):
        mobilenet.fused_conv_block(torch.zeros(1, 4, 8, 8), conv, None, None, mobilenet._FoldedNorm())
    for bad in (torch.nn.Conv2d(4, 4, 3, padding=2, dilation=2, groups=4), torch.nn.Conv2d(4, 4, 5, padding=4, dilation=2, groups=2),
                torch.nn.Conv2d(4, 4, 5, padding=2, dilation=2, groups=4), torch.nn.Conv2d(4, 4, 5, padding=4, dilation=2, groups=4, stride=2)):
        with pytest.raises(NotImplementedError, match="dilation 1"):
            mobilenet.fused_conv_block(torch.zeros(1, 4, 8, 8), bad, None, None, mobilenet._FoldedNorm())
    for build in (mv.mobilenet_v3_small, mv.mobilenet_v3_large):
        with pytest.raises(NotImplementedError, match="segmentation backbone"):  # before any launch: not Mi355VisionError
            build(num_classes=3, dilated=True)(torch.zeros(1, 3, 32, 32))
    with pytest.raises(_lib.Mi355VisionError):  # the undilated forward reaches the library
        mv.mobilenet_v3_small(num_classes=3)(torch.zeros(1, 3, 32, 32))


@pytest.mark.parametrize("shape", R.DW_SHAPES + [R.DW_LONG], ids=str)
def test_the_stuffed_oracle_is_the_dilated_conv(shape):
    """The GPU tests' oracle (the zero-stuffed 9 x 9 kernel through ref.conv2d_affine_act) equals the oracle's own dilated conv
    (padding by select) bit for bit on the finite test inputs."""
    x, w = R.dw_inputs(shape)[:2]
    got, want = R.dw_dilated(x, w), R.dw_dilated_select(x, w)
    assert got.shape == want.shape == shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    t = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), None, 1, 4, 2, shape[1]).numpy()
    assert np.abs(got - t).max() <= 1e-5 * max(1.0, np.abs(t).max())


def test_stage_by_stage_forward_against_torch():
    """The stage-by-stage CPU forward of the replica against torch's own float32 forward, and the resized logits of a seeded replica
    not being one class everywhere."""
    torch.manual_seed(21)
    rep = R.replica("lraspp_mobilenet_v3_large", num_classes=3)
    x = R.rng(23).standard_normal((1, 3, 33, 33), dtype=np.float32)
    R.perturb(rep, 22, x)
    want = R.model_stages(rep, x)
    with torch.no_grad():
        feats = rep.backbone(torch.from_numpy(x))
        out = rep(torch.from_numpy(x))["out"].numpy()
    for k in ("low", "high"):
        t = feats[k].numpy()
        assert want["features"][k].shape == t.shape
        assert np.abs(want["features"][k] - t).max() <= 1e-4 * np.abs(t).max(), k
    assert want["out"].shape == out.shape == (1, 3, 33, 33)
    assert np.abs(want["out"] - out).max() <= 1e-4 * np.abs(out).max()
    assert len(np.unique(want["out"].argmax(1))) > 1


def test_gated_upsample_restatement_against_torch():
    for case in R.GU_CASES:
        x, gate, w, bias, res = R.gu_inputs(case)
        (n, cin, h, wd), (oh, ow), cout = case
        got = R.gated_upsample(x, gate, w, bias, res, oh, ow)
        u = torch.nn.functional.interpolate(torch.from_numpy(x).double() * torch.from_numpy(gate).double()[:, :, None, None], size=(oh, ow),
                                            mode="bilinear", align_corners=False)
        t = (torch.nn.functional.conv2d(u, torch.from_numpy(w).double(), torch.from_numpy(bias).double()) + torch.from_numpy(res).double()).numpy()
        assert got.shape == t.shape and np.abs(got - t).max() <= 1e-5 * max(1.0, np.abs(t).max()), case
    (n, cin, h, wd), (oh, ow), cout = R.GU_CASES[R.GU_SLICED]
    assert F.conv1x1_k_slices(n, cin, oh, ow, cout)[0] > 1  # the K-sliced plan
