"""What the segmentation tests compare with (a helper module, not a conftest):

  * a plain-torch replica of the reference's models/segmentation/_utils.py, fcn.py and deeplabv3.py (ResNet backbones), written from
    the reference's published structure over tests/_resnet_ref.ResNet and tests/_fpn_ref.IntermediateLayerGetter: the same constructor
    arguments, children, names and construction order, and torch's own forward -- for trees, state-dict keys, seeded initialisation
    and the float32 / float64 evaluations of the accuracy condition;
  * a stage-by-stage numpy forward of the heads and of a whole model: tests/_resnet_ref.oracle_conv for every conv + norm + ReLU (the
    pointwise ones in the order F.conv1x1_k_slices states), tests/_mobilenetv3_ref.global_avg_pool for the pool,
    tests/_interp_ref.interpolate for both resizes;
  * interpolate_argmax: tests/_interp_ref.interpolate, then the first-maximum / first-NaN rule written out, and the fixtures of
    F.interpolate_argmax shared by the host and the GPU tests.

An atrous 3x3 conv whose rate reaches the map's larger side reads, for every output pixel, only its centre tap inside the map; the
oracle then runs that tap alone (a 1x1 conv, the single ascending chain over the channels): the dropped taps add x * 0 = +-0 to the
chain, which changes no finite sum, so the comparison is by value (+0 == -0), as for tests/_resnet_ref's zero-stuffed kernels.
"""
from collections import OrderedDict

import numpy as np
import torch
from torch import nn
from torch.nn import functional as TF

from tests import _interp_ref as IR
from tests import _mobilenetv3_ref as MR
from tests import _resnet_ref as RR
from tests._fpn_ref import IntermediateLayerGetter

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------- torch replica
class TSimpleSegmentationModel(nn.Module):
    def __init__(self, backbone, classifier, aux_classifier=None):
        super().__init__()
        self.backbone = backbone
        self.classifier = classifier
        self.aux_classifier = aux_classifier

    def forward(self, x):
        input_shape = x.shape[-2:]
        features = self.backbone(x)
        result = OrderedDict()
        result["out"] = TF.interpolate(self.classifier(features["out"]), size=input_shape, mode="bilinear", align_corners=False)
        if self.aux_classifier is not None:
            result["aux"] = TF.interpolate(self.aux_classifier(features["aux"]), size=input_shape, mode="bilinear", align_corners=False)
        return result


class TFCN(TSimpleSegmentationModel):
    pass


class TDeepLabV3(TSimpleSegmentationModel):
    pass


class TFCNHead(nn.Sequential):
    def __init__(self, in_channels, channels):
        inter = in_channels // 4
        super().__init__(nn.Conv2d(in_channels, inter, 3, padding=1, bias=False), nn.BatchNorm2d(inter), nn.ReLU(), nn.Dropout(0.1),
                         nn.Conv2d(inter, channels, 1))


class TASPPConv(nn.Sequential):
    def __init__(self, in_channels, out_channels, dilation):
        super().__init__(nn.Conv2d(in_channels, out_channels, 3, padding=dilation, dilation=dilation, bias=False),
                         nn.BatchNorm2d(out_channels), nn.ReLU())


class TASPPPooling(nn.Sequential):
    def __init__(self, in_channels, out_channels):
        super().__init__(nn.AdaptiveAvgPool2d(1), nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels),
                         nn.ReLU())

    def forward(self, x):
        size = x.shape[-2:]
        for mod in self:
            x = mod(x)
        return TF.interpolate(x, size=size, mode="bilinear", align_corners=False)


class TASPP(nn.Module):
    def __init__(self, in_channels, atrous_rates, out_channels=256):
        super().__init__()
        modules = [nn.Sequential(nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU())]
        for rate in tuple(atrous_rates):
            modules.append(TASPPConv(in_channels, out_channels, rate))
        modules.append(TASPPPooling(in_channels, out_channels))
        self.convs = nn.ModuleList(modules)
        self.project = nn.Sequential(nn.Conv2d(len(self.convs) * out_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels),
                                     nn.ReLU(), nn.Dropout(0.5))

    def forward(self, x):
        return self.project(torch.cat([conv(x) for conv in self.convs], dim=1))


class TDeepLabHead(nn.Sequential):
    def __init__(self, in_channels, num_classes, atrous_rates=(12, 24, 36)):
        super().__init__(TASPP(in_channels, atrous_rates), nn.Conv2d(256, 256, 3, padding=1, bias=False), nn.BatchNorm2d(256), nn.ReLU(),
                         nn.Conv2d(256, num_classes, 1))


def resnet101(**kw):
    return RR.ResNet(RR.Bottleneck, [3, 4, 23, 3], **kw)


_BUILDERS = {"fcn_resnet50": (TFCN, TFCNHead, RR.resnet50), "fcn_resnet101": (TFCN, TFCNHead, resnet101),
             "deeplabv3_resnet50": (TDeepLabV3, TDeepLabHead, RR.resnet50), "deeplabv3_resnet101": (TDeepLabV3, TDeepLabHead, resnet101)}


def replica(name, num_classes=21, aux_loss=None):
    """The torch replica of fcn_resnet50 / 101 and deeplabv3_resnet50 / 101 (no weights): the aux head is built before the classifier,
    as the reference's _fcn_resnet / _deeplabv3_resnet do."""
    model, head, resnet = _BUILDERS[name]
    backbone = resnet(replace_stride_with_dilation=[False, True, True])
    return_layers = {"layer4": "out"}
    if aux_loss:
        return_layers["layer3"] = "aux"
    body = IntermediateLayerGetter(backbone, return_layers=return_layers)
    aux = TFCNHead(1024, num_classes) if aux_loss else None
    return model(body, head(2048, num_classes), aux).eval()


# ------------------------------------------------------------------------------------------------------------- stage-by-stage forward
def _p(t):
    return t.detach().numpy()


SLICE_CHANNELS = 128  # segmentation.SLICE_CHANNELS, restated


def conv_norm_relu(x, conv, norm):
    """conv -> folded norm -> ReLU through the oracle.  A 1x1 conv: the pointwise order.  A head's 3x3 conv: the stated sliced sum
    (segmentation.sliced_conv_norm_relu) -- per slice g of 128 input channels one ascending (c, ky, kx) chain s_g,
    p_0 = fma(alpha, s_0, beta), p_g = fma(alpha, s_g, 0) + p_(g-1), ReLU on the last; an atrous conv out of the map's reach as its
    centre tap (module docstring)."""
    x = np.ascontiguousarray(x, F32)
    if conv.kernel_size != (3, 3):
        return RR.oracle_conv_norm(x, conv, norm, relu=True)
    d, cin = conv.dilation[0], x.shape[1]
    assert conv.padding == (d, d) and conv.stride == (1, 1) and conv.groups == 1 and conv.bias is None
    centre = d > 1 and d >= max(x.shape[2], x.shape[3])
    a, b, code = RR.folded(norm)
    w, p = _p(conv.weight), None
    for c0 in range(0, cin, SLICE_CHANNELS):
        ws = w[:, c0:c0 + SLICE_CHANNELS, 1:2, 1:2] if centre else w[:, c0:c0 + SLICE_CHANNELS]
        p = RR.oracle_conv(np.ascontiguousarray(x[:, c0:c0 + SLICE_CHANNELS]), np.ascontiguousarray(ws), None, a,
                           b if c0 == 0 else np.zeros_like(b), p, 1, 0 if centre else d, 1 if centre else d, 1, code,
                           "relu" if c0 + SLICE_CHANNELS >= cin else None)
    return p


def classify(x, conv):
    """The last 1x1 conv of a head with its bias, in the pointwise order."""
    return RR.oracle_conv(x, _p(conv.weight), _p(conv.bias), pointwise_order=True)


def fcn_head_stages(head, x):
    """[conv + norm + ReLU, logits] of an FCNHead (the library's or the replica's: the same children)."""
    mid = conv_norm_relu(x, head[0], head[1])
    return [mid, classify(mid, head[4])]


def aspp_pooling_stages(mod, x):
    """[pooled (N, C), conv + norm + ReLU on the (N, C, 1, 1) map, the resize to the feature size] of an ASPPPooling."""
    x = np.asarray(x, F32)
    pooled = MR.global_avg_pool(x)
    y = conv_norm_relu(pooled.reshape(pooled.shape[0], pooled.shape[1], 1, 1), mod[1], mod[2])
    return [pooled, y, IR.interpolate(y, x.shape[2], x.shape[3])]


def aspp_stages(aspp, x):
    """[every branch's output ..., the projection] of an ASPP."""
    branches = [conv_norm_relu(x, conv[0], conv[1]) for conv in list(aspp.convs)[:-1]]
    branches.append(aspp_pooling_stages(aspp.convs[-1], x)[-1])
    cat = np.ascontiguousarray(np.concatenate(branches, axis=1))
    return branches + [conv_norm_relu(cat, aspp.project[0], aspp.project[1])]


def deeplab_head_stages(head, x):
    """[ASPP's output, conv + norm + ReLU, logits] of a DeepLabHead."""
    y = aspp_stages(head[0], x)[-1]
    mid = conv_norm_relu(y, head[1], head[2])
    return [y, mid, classify(mid, head[4])]


def head_stages(head, x):
    return deeplab_head_stages(head, x) if hasattr(head[0], "convs") else fcn_head_stages(head, x)


def backbone_features(body, x):
    """{"out": layer4, "aux": layer3 (when returned)} of an IntermediateLayerGetter over a ResNet through the oracle."""
    a = RR.oracle_conv_norm(np.ascontiguousarray(x, F32), body["conv1"], body["bn1"], relu=True)
    mp = body["maxpool"]
    a = RR.padded_max_pool(a, mp.kernel_size, mp.stride, mp.padding)
    out = OrderedDict()
    returned = {str(k): v for k, v in body.return_layers.items()}
    for name in ("layer1", "layer2", "layer3", "layer4"):
        for block in body[name]:
            a = RR.oracle_block(block, a)
        if name in returned:
            out[returned[name]] = a
    return out


def model_stages(model, x):
    """A whole _SimpleSegmentationModel with CPU-resident parameters on a numpy batch: {"features": {...}, "out_stages": [...],
    "out": resized logits, and "aux_stages" / "aux" with an aux head}."""
    h, w = x.shape[-2:]
    feats = backbone_features(model.backbone, x)
    res = {"features": feats, "out_stages": head_stages(model.classifier, feats["out"])}
    res["out"] = IR.interpolate(res["out_stages"][-1], h, w)
    if model.aux_classifier is not None:
        res["aux_stages"] = head_stages(model.aux_classifier, feats["aux"])
        res["aux"] = IR.interpolate(res["aux_stages"][-1], h, w)
    return res


# ------------------------------------------------------------------------------------------------------------- interpolate_argmax
def argmax_rule(v):
    """torch.argmax over axis 1 written out: ascending classes, a later class wins only when it is greater or is the first NaN."""
    v = np.asarray(v, F32)
    best, arg = v[:, 0].copy(), np.zeros(v[:, 0].shape, np.int64)
    for k in range(1, v.shape[1]):
        vk = v[:, k]
        with np.errstate(invalid="ignore"):
            take = (vk > best) | (np.isnan(vk) & ~np.isnan(best))
        best, arg = np.where(take, vk, best), np.where(take, k, arg)
    return arg


def interpolate_argmax(x, oh, ow):
    """(N, C, H, W) float32 -> (N, oh, ow) int64: the stated bilinear values, then the rule."""
    return argmax_rule(IR.interpolate(x, oh, ow))


def _rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def _randn(seed, shape):
    return _rng(seed).standard_normal(shape, dtype=F32)


def fixture_class255():
    """(1, 256, 2, 2) -> (3, 3) with class 255 the maximum at source pixel (1, 1), which output pixel (2, 2) reads alone."""
    x = _randn(7, (1, 256, 2, 2))
    x[0, 255, 1, 1] = 9.0
    return x


def fixture_ties():
    """(2, 5, 7, 9) -> (23, 31), seed 0, plane 3 a copy of plane 1: wherever plane 1 is the maximum two classes attain it."""
    x = _randn(0, (2, 5, 7, 9))
    x[:, 3] = x[:, 1]
    return x


def fixture_signed_zeros():
    """(1, 3, 4, 5) -> (9, 11): a negative plane, a -0.0 plane and a +0.0 plane: -0.0 == +0.0 is a tie and class 1 wins everywhere."""
    x = np.zeros((1, 3, 4, 5), F32)
    x[0, 0] = -np.abs(_randn(1, (4, 5))) - F32(0.5)
    x[0, 1] = F32(-0.0)
    return x


def fixture_special():
    """(2, 4, 6, 7) -> (13, 17) with NaN in two classes of one source pixel, a lone NaN, +Inf and -Inf."""
    x = _randn(2, (2, 4, 6, 7))
    x[0, 1, 2, 3] = x[0, 3, 2, 3] = np.nan
    x[1, 2, 5, 6] = np.nan
    x[0, 2, 4, 1] = np.inf
    x[1, 0, 1, 1] = -np.inf
    x[1, 3, 3, 0] = np.inf
    return x


# name -> (input, (oh, ow)); every case runs with both label dtypes
def fixtures():
    return OrderedDict([
        ("ragged", (_randn(10, (2, 5, 7, 9)), (23, 31))),              # ragged width, non-integer scales
        ("x8_vector", (_randn(11, (1, 21, 9, 9)), (72, 72))),          # x8, the vector store path
        ("one_class", (_randn(12, (1, 1, 4, 4)), (8, 8))),             # C = 1: all zeros
        ("source_1x1", (_randn(13, (3, 2, 1, 1)), (5, 6))),
        ("downscale", (_randn(14, (1, 4, 12, 10)), (5, 4))),
        ("two_column_blocks", (_randn(15, (1, 3, 3, 40)), (6, 523))),  # more than one column block, ragged tail
        ("class_255", (fixture_class255(), (3, 3))),
        ("ties", (fixture_ties(), (23, 31))),
        ("signed_zeros", (fixture_signed_zeros(), (9, 11))),
        ("special", (fixture_special(), (13, 17))),
    ])


def perturb(model, seed):
    """tests/_mobilenetv3_ref.perturb: seeded norm statistics, affine terms and biases."""
    MR.perturb(model, seed)


same = MR.same
