"""What the LRASPP / DeepLabV3-MobileNetV3 tests compare with (a helper module, not a conftest):

  * a plain-torch replica of the reference's models/segmentation/lraspp.py (LRASPPHead, LRASPP, lraspp_mobilenet_v3_large) and of
    deeplabv3_mobilenet_v3_large, written from the reference's published structure over tests/_mobilenetv3_ref.replica(...,
    dilated=True), tests/_fpn_ref.IntermediateLayerGetter and tests/_segmentation_ref's heads: the same constructor arguments, children,
    names and construction order, and torch's own forward;
  * the oracle of the dilated depthwise conv (kernel 5, dilation 2, padding 4, stride 1): oracle.ref.conv2d_affine_act on the kernel
    zero-stuffed to 9 x 9 -- for finite data the extra fmaf(0, x, acc) terms change no bit -- and, for NaN / Inf inputs,
    ref.conv2d_bias_act(dilation=2, groups=c), which pads by select and has no epilogue (the stuffed form would spread a NaN over the
    whole 9 x 9 window).  tests/test_lraspp_host.py asserts the two equal on the finite test inputs;
  * the restatement of F.conv1x1_gated_upsample: tests/_interp_ref.interpolate of tests/_mobilenetv3_ref.se_scale(x, gate), through
    ref.conv2d_affine_act in the order F.conv1x1_k_slices(n, cin, oh, ow, cout) states, with the residual;
  * stage-by-stage numpy forwards of a MobileNetV3's `features` (the dilated blocks through the oracle above; tests/_util.
    oracle_conv_block passes conv.padding with the 5 x 5 weight and cannot run them), of an LRASPPHead and of the whole models.
"""
from collections import OrderedDict

import numpy as np
import torch
from torch import nn
from torch.nn import functional as TF

from tests import _interp_ref as IR
from tests import _mobilenetv3_ref as MR
from tests import _resnet_ref as RR
from tests import _segmentation_ref as GR
from tests._fpn_ref import IntermediateLayerGetter

F32 = np.float32
STAGE_INDICES = [0, 2, 4, 7, 13, 16]


# ------------------------------------------------------------------------------------------------------------- torch replica
class TLRASPPHead(nn.Module):
    def __init__(self, low_channels, high_channels, num_classes, inter_channels):
        super().__init__()
        self.cbr = nn.Sequential(nn.Conv2d(high_channels, inter_channels, 1, bias=False), nn.BatchNorm2d(inter_channels),
                                 nn.ReLU(inplace=True))
        self.scale = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(high_channels, inter_channels, 1, bias=False), nn.Sigmoid())
        self.low_classifier = nn.Conv2d(low_channels, num_classes, 1)
        self.high_classifier = nn.Conv2d(inter_channels, num_classes, 1)

    def forward(self, input):
        low, high = input["low"], input["high"]
        x = self.cbr(high) * self.scale(high)
        x = TF.interpolate(x, size=low.shape[-2:], mode="bilinear", align_corners=False)
        return self.low_classifier(low) + self.high_classifier(x)


class TLRASPP(nn.Module):
    def __init__(self, backbone, low_channels, high_channels, num_classes, inter_channels=128):
        super().__init__()
        self.backbone = backbone
        self.classifier = TLRASPPHead(low_channels, high_channels, num_classes, inter_channels)

    def forward(self, input):
        out = self.classifier(self.backbone(input))
        return OrderedDict(out=TF.interpolate(out, size=input.shape[-2:], mode="bilinear", align_corners=False))


def stage_indices(features):
    return [0] + [i for i, b in enumerate(features) if getattr(b, "_is_cn", False)] + [len(features) - 1]


def replica(name, num_classes=21, aux_loss=None):
    """The torch replica of lraspp_mobilenet_v3_large / deeplabv3_mobilenet_v3_large (no weights), built in the reference's order."""
    backbone = MR.replica("mobilenet_v3_large", dilated=True).features
    idx = stage_indices(backbone)
    if name == "lraspp_mobilenet_v3_large":
        low, high = idx[-4], idx[-1]
        body = IntermediateLayerGetter(backbone, return_layers={str(low): "low", str(high): "high"})
        return TLRASPP(body, backbone[low].out_channels, backbone[high].out_channels, num_classes).eval()
    assert name == "deeplabv3_mobilenet_v3_large"
    out_pos, aux_pos = idx[-1], idx[-4]
    return_layers = {str(out_pos): "out"}
    if aux_loss:
        return_layers[str(aux_pos)] = "aux"
    body = IntermediateLayerGetter(backbone, return_layers=return_layers)
    aux = GR.TFCNHead(backbone[aux_pos].out_channels, num_classes) if aux_loss else None
    return GR.TDeepLabV3(body, GR.TDeepLabHead(backbone[out_pos].out_channels, num_classes), aux).eval()


# ------------------------------------------------------------------------------------------------------------- the dilated depthwise conv
def stuffed(w):
    """(c, 1, 5, 5) -> (c, 1, 9, 9): the taps at the even positions, zeros between them."""
    w = np.asarray(w, F32)
    st = np.zeros((w.shape[0], 1, 9, 9), F32)
    st[:, :, ::2, ::2] = w
    return st


def dw_dilated(x, w, bias=None, alpha=None, beta=None, res=None, affine=0, act=None):
    """Depthwise 5x5, dilation 2, padding 4, stride 1 + the epilogue, for FINITE data: the oracle on the zero-stuffed kernel."""
    from oracle import ref
    x = np.ascontiguousarray(x, F32)
    return ref.conv2d_affine_act(x, stuffed(w), bias, alpha, beta, res, 1, 4, x.shape[1], affine, act)


def dw_dilated_select(x, w):
    """The same conv without an epilogue, padding by select: the reference for NaN / Inf inputs."""
    from oracle import ref
    x = np.ascontiguousarray(x, F32)
    return ref.conv2d_bias_act(x, np.ascontiguousarray(w, F32), None, (1, 1), (4, 4), (2, 2), x.shape[1], None)


def is_dilated_dw(conv):
    return conv.groups == conv.in_channels == conv.out_channels and conv.kernel_size == (5, 5) and conv.dilation == (2, 2) and \
        conv.padding == (4, 4) and conv.stride == (1, 1)


def conv_block(block, x, residual=None):
    """One conv -> norm [-> activation] block of a MobileNetV3 (the library's or the replica's) through the oracle."""
    conv = block[0]
    if conv.dilation == (1, 1):
        return MR._conv_block(block, x, residual)
    assert is_dilated_dw(conv) and conv.bias is None, conv
    a, b, code = RR.folded(block[1])
    act = MR._ACT_NAMES[type(block[2])] if len(block) > 2 else None
    return dw_dilated(x, conv.weight.detach().numpy(), None, a, b, residual, code, act)


def block_stages(block, x):
    """tests/_mobilenetv3_ref.block_stages with the dilated depthwise conv: expand?, depthwise, gate? (N, C), the block's output."""
    out, y, gate = [], x, None
    layers = list(block.block)
    for layer in layers[:-1]:
        if hasattr(layer, "fc1"):
            gate = MR.se_gate_of(layer, y)
            out.append(gate)
        else:
            y = conv_block(layer, y)
            out.append(y)
    if gate is not None:
        y = MR.se_scale(y, gate)
    out.append(conv_block(layers[-1], y, x if block.use_res_connect else None))
    return out


def features_stages(features, x):
    """The output of every element of a MobileNetV3's `features` (any iterable of its children) on a numpy batch."""
    feats, y = [], np.ascontiguousarray(x, F32)
    for layer in features:
        y = block_stages(layer, y)[-1] if hasattr(layer, "block") else conv_block(layer, y)
        feats.append(y)
    return feats


def backbone_features(body, x):
    """{returned name: feature} of an IntermediateLayerGetter over a MobileNetV3's features (children "0", "1", ...), in call order."""
    returned = {str(k): v for k, v in body.return_layers.items()}
    feats = features_stages(body.values(), x)
    return OrderedDict((returned[name], f) for name, f in zip(body.keys(), feats) if name in returned)


# ------------------------------------------------------------------------------------------------------------- the fused head launch
def gated_upsample(x, gate, w, bias, res, oh, ow):
    """F.conv1x1_gated_upsample restated: resize(se_scale(x, gate)) -> the pointwise conv in the stated order -> + bias -> res + v."""
    from cpu_vision_amd import functional as F
    from oracle import ref
    u = np.ascontiguousarray(IR.interpolate(MR.se_scale(np.asarray(x, F32), gate), oh, ow))
    w = np.ascontiguousarray(np.asarray(w, F32).reshape(w.shape[0], -1, 1, 1))
    slices, sl = F.conv1x1_k_slices(u.shape[0], u.shape[1], oh, ow, w.shape[0])
    with np.errstate(all="ignore"):
        return ref.conv2d_affine_act(u, w, bias, None, None, res, 1, 0, 1, 0, None, slice_len=sl if slices > 1 else 0)


def _p(t):
    return None if t is None else t.detach().numpy()


def lraspp_head_stages(head, low, high):
    """[cbr, pooled (N, high), gate (N, inter), low_classifier(low), the head's output] of an LRASPPHead: its five launches."""
    low, high = np.ascontiguousarray(low, F32), np.ascontiguousarray(high, F32)
    cbr = RR.oracle_conv_norm(high, head.cbr[0], head.cbr[1], relu=True)
    pooled = MR.global_avg_pool(high)
    gate = MR.linear_act(pooled, _p(head.scale[1].weight), None, "sigmoid")
    lowc = GR.classify(low, head.low_classifier)
    out = gated_upsample(cbr, gate, _p(head.high_classifier.weight), _p(head.high_classifier.bias), lowc, low.shape[2], low.shape[3])
    return [cbr, pooled, gate, lowc, out]


def model_stages(model, x):
    """A whole LRASPP or DeepLabV3-MobileNetV3 with CPU-resident parameters on a numpy batch: {"features", "out_stages", "out" and,
    with an aux head, "aux_stages", "aux"}."""
    h, w = x.shape[-2:]
    feats = backbone_features(model.backbone, x)
    if hasattr(model.classifier, "cbr"):
        res = {"features": feats, "out_stages": lraspp_head_stages(model.classifier, feats["low"], feats["high"])}
    else:
        res = {"features": feats, "out_stages": GR.head_stages(model.classifier, feats["out"])}
    res["out"] = IR.interpolate(res["out_stages"][-1], h, w)
    if getattr(model, "aux_classifier", None) is not None:
        res["aux_stages"] = GR.head_stages(model.aux_classifier, feats["aux"])
        res["aux"] = IR.interpolate(res["aux_stages"][-1], h, w)
    return res


# ------------------------------------------------------------------------------------------------------------- shared test inputs
# (n, c, h, w) of the dilated depthwise tests.  (1, 1, 19, 5): three row blocks at the short-launch strip (4 rows per parity, 8 per
# block) -- a column has three strips of each row parity, the last block ragged
DW_SHAPES = [(1, 1, 1, 1), (2, 3, 2, 3), (1, 2, 5, 7), (1, 3, 9, 6), (1, 2, 9, 9), (1, 2, 13, 14), (1, 3, 33, 33), (1, 2, 6, 64),
             (1, 1, 7, 65), (1, 1, 19, 5)]
# the launcher halves the strip below kDw5ShortLaunch = 16384 threads: 2 x 128 planes x 2 parities x ceil(16 / 16) x 32 quads = 16384
# threads at 8 rows per parity keeps the full strip; the shapes above all take the short one
DW_LONG = (2, 128, 16, 128)

# (n, cin, h, w), (oh, ow), cout of the fused head launch
GU_CASES = [((1, 1, 1, 1), (1, 1), 1), ((2, 5, 3, 4), (5, 7), 3), ((1, 33, 9, 9), (17, 19), 33), ((1, 8, 6, 6), (6, 6), 4),
            ((1, 8, 7, 9), (4, 5), 4), ((1, 192, 3, 3), (5, 5), 21), ((1, 128, 3, 3), (5, 5), 21)]
GU_SLICED = 5  # index of the K-sliced case


def rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def dw_inputs(shape, seed=0):
    """x, w (c, 1, 5, 5), bias, alpha, beta, residual of one depthwise case: finite, seeded by the shape."""
    n, c, h, w = shape
    g = rng(7000 + seed + 131 * c + 17 * h + w)
    x = g.standard_normal(shape, dtype=F32)
    wt = (g.standard_normal((c, 1, 5, 5), dtype=F32) * F32(0.3)).astype(F32)
    bias, beta = g.standard_normal(c, dtype=F32), g.standard_normal(c, dtype=F32)
    alpha = (g.random(c, dtype=F32) + F32(0.5)).astype(F32)
    res = g.standard_normal(shape, dtype=F32)
    return x, wt, bias, alpha, beta, res


def gu_inputs(case, seed=0):
    """x, gate (n, cin), w (cout, cin, 1, 1), bias, residual (n, cout, oh, ow) of one fused-head case."""
    (n, cin, h, w), (oh, ow), cout = case
    g = rng(8000 + seed + 131 * cin + 17 * h + oh)
    x = g.standard_normal((n, cin, h, w), dtype=F32)
    gate = g.random((n, cin), dtype=F32)
    wt = (g.standard_normal((cout, cin, 1, 1), dtype=F32) * F32(0.3)).astype(F32)
    return x, gate, wt, g.standard_normal(cout, dtype=F32), g.standard_normal((n, cout, oh, ow), dtype=F32)


def perturb(rep, seed, x):
    """tests/_mobilenetv3_ref.perturb on a torch replica, then every head's last bias moved so that each class has the same mean
    logit on the batch x: the random biases otherwise decide the argmax everywhere (measured: one class on every pixel for ten
    seeds), and a labels() test on such a state would show nothing.  Chosen on the replica alone."""
    MR.perturb(rep, seed)
    last = [rep.classifier.high_classifier] if hasattr(rep.classifier, "cbr") else [rep.classifier[4]]
    keys = ["out"]
    if getattr(rep, "aux_classifier", None) is not None:
        last.append(rep.aux_classifier[4])
        keys.append("aux")
    with torch.no_grad():
        out = rep(torch.from_numpy(np.ascontiguousarray(x, F32)))
        for conv, k in zip(last, keys):
            conv.bias -= out[k].mean(dim=(0, 2, 3))


same = MR.same
