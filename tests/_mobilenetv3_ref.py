"""What the MobileNetV3 tests compare with (a helper module, not a conftest):

  * a plain-torch replica of the reference's modules (ops/misc.py SqueezeExcitation and Conv2dNormActivation, models/mobilenetv3.py
    InvertedResidualConfig / InvertedResidual / MobileNetV3 / _mobilenet_v3_conf), written from the reference's published structure:
    the same constructor arguments, children, names and initialisation, and torch's own forward -- for trees, state-dict keys,
    seeded initialisation and the float32 / float64 evaluations of the accuracy conditions;
  * numpy restatements of the arithmetic mi355vision.h states for mv_global_avgpool_f64sum_f32, mv_linear_act_f32 (with its five
    activations) and mv_se_scale_f32: float64 additions in the stated order, one cast;
  * forward_stages: a whole network stage by stage, every conv through oracle.ref.conv2d_affine_act (in the summation order
    F.conv1x1_k_slices states for the pointwise ones), the projection of a squeeze-excitation block fed the restated se_scale.
"""
from functools import partial

import numpy as np
import torch
from torch import nn

LANES = 64


# ------------------------------------------------------------------------------------------------------------- torch replica
def make_divisible(v, divisor=8, min_value=None):
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


class TConv2dNormActivation(nn.Sequential):
    def __init__(self, cin, cout, kernel_size=3, stride=1, groups=1, norm_layer=nn.BatchNorm2d, activation_layer=nn.ReLU, dilation=1):
        padding = (kernel_size - 1) // 2 * dilation
        layers = [nn.Conv2d(cin, cout, kernel_size, stride, padding, dilation=dilation, groups=groups, bias=norm_layer is None)]
        if norm_layer is not None:
            layers.append(norm_layer(cout))
        if activation_layer is not None:
            layers.append(activation_layer(inplace=True))
        super().__init__(*layers)
        self.out_channels = cout


class TSqueezeExcitation(nn.Module):
    def __init__(self, input_channels, squeeze_channels, activation=nn.ReLU, scale_activation=nn.Sigmoid):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(input_channels, squeeze_channels, 1)
        self.fc2 = nn.Conv2d(squeeze_channels, input_channels, 1)
        self.activation = activation()
        self.scale_activation = scale_activation()

    def _scale(self, x):
        return self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(x)))))

    def forward(self, x):
        return self._scale(x) * x


class TConfig:
    def __init__(self, input_channels, kernel, expanded_channels, out_channels, use_se, activation, stride, dilation, width_mult):
        adj = lambda c: make_divisible(c * width_mult, 8)  # noqa: E731
        self.input_channels, self.kernel, self.expanded_channels, self.out_channels = adj(input_channels), kernel, adj(expanded_channels), adj(out_channels)
        self.use_se, self.use_hs, self.stride, self.dilation = use_se, activation == "HS", stride, dilation


class TInvertedResidual(nn.Module):
    def __init__(self, cnf, norm_layer, se_layer=partial(TSqueezeExcitation, scale_activation=nn.Hardsigmoid)):
        super().__init__()
        if not (1 <= cnf.stride <= 2):
            raise ValueError("illegal stride value")
        self.use_res_connect = cnf.stride == 1 and cnf.input_channels == cnf.out_channels
        act = nn.Hardswish if cnf.use_hs else nn.ReLU
        layers = []
        if cnf.expanded_channels != cnf.input_channels:
            layers.append(TConv2dNormActivation(cnf.input_channels, cnf.expanded_channels, kernel_size=1, norm_layer=norm_layer, activation_layer=act))
        layers.append(TConv2dNormActivation(cnf.expanded_channels, cnf.expanded_channels, kernel_size=cnf.kernel,
                                            stride=1 if cnf.dilation > 1 else cnf.stride, dilation=cnf.dilation, groups=cnf.expanded_channels,
                                            norm_layer=norm_layer, activation_layer=act))
        if cnf.use_se:
            layers.append(se_layer(cnf.expanded_channels, make_divisible(cnf.expanded_channels // 4, 8)))
        layers.append(TConv2dNormActivation(cnf.expanded_channels, cnf.out_channels, kernel_size=1, norm_layer=norm_layer, activation_layer=None))
        self.block = nn.Sequential(*layers)
        self.out_channels = cnf.out_channels
        self._is_cn = cnf.stride > 1

    def forward(self, x):
        y = self.block(x)
        return x + y if self.use_res_connect else y


class TMobileNetV3(nn.Module):
    def __init__(self, setting, last_channel, num_classes=1000, dropout=0.2):
        super().__init__()
        norm_layer = partial(nn.BatchNorm2d, eps=0.001, momentum=0.01)
        layers = [TConv2dNormActivation(3, setting[0].input_channels, kernel_size=3, stride=2, norm_layer=norm_layer, activation_layer=nn.Hardswish)]
        layers += [TInvertedResidual(c, norm_layer) for c in setting]
        cl = setting[-1].out_channels
        layers.append(TConv2dNormActivation(cl, 6 * cl, kernel_size=1, norm_layer=norm_layer, activation_layer=nn.Hardswish))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Linear(6 * cl, last_channel), nn.Hardswish(inplace=True), nn.Dropout(p=dropout, inplace=True),
                                        nn.Linear(last_channel, num_classes))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        return self.classifier(torch.flatten(self.avgpool(self.features(x)), 1))


# rows (in, k, exp, out, se, act, stride, dilated?) with r = the reduced tail's divider applied to the marked entries
_LARGE = [(16, 3, 16, 16, 0, "RE", 1, 0), (16, 3, 64, 24, 0, "RE", 2, 0), (24, 3, 72, 24, 0, "RE", 1, 0), (24, 5, 72, 40, 1, "RE", 2, 0),
          (40, 5, 120, 40, 1, "RE", 1, 0), (40, 5, 120, 40, 1, "RE", 1, 0), (40, 3, 240, 80, 0, "HS", 2, 0), (80, 3, 200, 80, 0, "HS", 1, 0),
          (80, 3, 184, 80, 0, "HS", 1, 0), (80, 3, 184, 80, 0, "HS", 1, 0), (80, 3, 480, 112, 1, "HS", 1, 0), (112, 3, 672, 112, 1, "HS", 1, 0),
          (112, 5, 672, -160, 1, "HS", 2, 1), (-160, 5, -960, -160, 1, "HS", 1, 1), (-160, 5, -960, -160, 1, "HS", 1, 1)]
_SMALL = [(16, 3, 16, 16, 1, "RE", 2, 0), (16, 3, 72, 24, 0, "RE", 2, 0), (24, 3, 88, 24, 0, "RE", 1, 0), (24, 5, 96, 40, 1, "HS", 2, 0),
          (40, 5, 240, 40, 1, "HS", 1, 0), (40, 5, 240, 40, 1, "HS", 1, 0), (40, 5, 120, 48, 1, "HS", 1, 0), (48, 5, 144, 48, 1, "HS", 1, 0),
          (48, 5, 288, -96, 1, "HS", 2, 1), (-96, 5, -576, -96, 1, "HS", 1, 1), (-96, 5, -576, -96, 1, "HS", 1, 1)]


def replica(arch, num_classes=1000, width_mult=1.0, reduced_tail=False, dilated=False):
    """The torch replica of mobilenet_v3_large / mobilenet_v3_small (a negative table entry is divided by the reduced tail's 2)."""
    r, d = (2 if reduced_tail else 1), (2 if dilated else 1)
    rows, last = {"mobilenet_v3_large": (_LARGE, 1280), "mobilenet_v3_small": (_SMALL, 1024)}[arch]
    red = lambda c: c if c > 0 else -c // r  # noqa: E731
    setting = [TConfig(red(i), k, red(e), red(o), bool(se), act, s, d if dil else 1, width_mult) for i, k, e, o, se, act, s, dil in rows]
    return TMobileNetV3(setting, make_divisible(last // r * width_mult, 8), num_classes=num_classes)


def perturb(model, seed):
    """Seeded values away from the initialisation for every norm's statistics and affine terms and every bias (in module order)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
                m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) * 0.4 - 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 1.5 + 0.4)
            elif isinstance(m, (nn.Conv2d, nn.Linear)) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)


# ------------------------------------------------------------------------------------------------------------- restatements
def _tree(s):
    """S[l] += S[l + off] for l < off, off = 32 .. 1, on the last axis (64 lanes) of a float64 array; returns S[0]."""
    s = s.copy()
    off = LANES // 2
    while off >= 1:
        s[..., :off] = s[..., :off] + s[..., off:2 * off]
        off //= 2
    return s[..., 0]


def global_avg_pool(x):
    """mv_global_avgpool_f64sum_f32: element p of a plane belongs to lane (p / 4) mod 64; a lane adds its elements in ascending p to
    0.0 in float64; the tree; (float)(S / P).  (Adding the +0.0 that pads a lane's last round changes no float64 sum.)"""
    x = np.asarray(x, np.float32)
    n, c, h, w = x.shape
    p = h * w
    rounds = -(-p // (4 * LANES))
    flat = np.zeros((n * c, rounds * 4 * LANES), np.float64)
    flat[:, :p] = x.reshape(n * c, p)
    q = flat.reshape(n * c, rounds, LANES, 4)
    s = np.zeros((n * c, LANES), np.float64)
    with np.errstate(all="ignore"):
        for r in range(rounds):
            for i in range(4):
                s = s + q[:, r, :, i]
        return (_tree(s) / np.float64(p)).astype(np.float32).reshape(n, c)


def act_relu(v):
    return np.where(v < 0, np.float32(0), v).astype(np.float32)  # a NaN stays


def _t(v):
    t = (v + np.float32(3)).astype(np.float32)
    return np.where(np.isnan(t), t, np.minimum(np.maximum(t, np.float32(0)), np.float32(6))).astype(np.float32)


def act_hardswish(v):
    with np.errstate(all="ignore"):
        return ((v * _t(v)).astype(np.float32) / np.float32(6)).astype(np.float32)


def act_hardsigmoid(v):
    with np.errstate(all="ignore"):
        return (_t(v) / np.float32(6)).astype(np.float32)


def act_sigmoid(v):
    with np.errstate(all="ignore"):
        e = np.exp(-v.astype(np.float64)).astype(np.float32)  # the correctly rounded float32 exp
        return (np.float32(1) / (np.float32(1) + e).astype(np.float32)).astype(np.float32)


ACTIVATIONS = {None: lambda v: v, "relu": act_relu, "hardswish": act_hardswish, "hardsigmoid": act_hardsigmoid, "sigmoid": act_sigmoid}


def linear_act(x, w, b=None, activation=None):
    """mv_linear_act_f32: lane l adds the exact float64 products x[i][k] w[j][k], k = l, l + 64, ..., in ascending k to 0.0; the tree;
    (float)(S + (double)b[j]); the activation."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    w = w.reshape(w.shape[0], -1)
    n, k = x.shape
    m = w.shape[0]
    rounds = -(-k // LANES)
    xp, wp = np.zeros((n, rounds * LANES), np.float64), np.zeros((m, rounds * LANES), np.float64)
    xp[:, :k], wp[:, :k] = x, w
    out = np.empty((n, m), np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            s = np.zeros((m, LANES), np.float64)
            for r in range(rounds):
                s = s + wp[:, r * LANES:(r + 1) * LANES] * xp[i, r * LANES:(r + 1) * LANES]
            tot = _tree(s)
            if b is not None:
                tot = tot + np.asarray(b, np.float32).astype(np.float64)
            out[i] = tot.astype(np.float32)
    return ACTIVATIONS[activation](out)


def se_scale(x, gate):
    with np.errstate(all="ignore"):
        return (np.asarray(gate, np.float32).reshape(x.shape[0], x.shape[1], 1, 1) * np.asarray(x, np.float32)).astype(np.float32)


def squeeze_excitation_gate(x, w1, b1, w2, b2, activation="relu", scale_activation="sigmoid"):
    return linear_act(linear_act(global_avg_pool(x), w1, b1, activation), w2, b2, scale_activation)


def se_gate_of(se, x):
    """The restated gate of a SqueezeExcitation module (the library's or the replica's: the same children) on a numpy x."""
    scale = {nn.Hardsigmoid: "hardsigmoid", nn.Sigmoid: "sigmoid"}[type(se.scale_activation)]
    p = lambda t: t.detach().numpy()  # noqa: E731
    return squeeze_excitation_gate(x, p(se.fc1.weight), p(se.fc1.bias), p(se.fc2.weight), p(se.fc2.bias), "relu", scale)


# ------------------------------------------------------------------------------------------------------------- stage-by-stage forward
_ACT_NAMES = {nn.ReLU: "relu", nn.Hardswish: "hardswish", nn.ReLU6: "relu6"}


def _conv_block(block, x, residual=None):
    from oracle import ref
    from tests._util import oracle_conv_block
    conv, norm = block[0], block[1]
    act = _ACT_NAMES[type(block[2])] if len(block) > 2 else None
    return oracle_conv_block(ref, x, conv, norm, act, residual)


def block_stages(block, x):
    """One InvertedResidual (the library's or the replica's) on a numpy x: the list of what each launch of the library's forward
    produces -- expand?, depthwise, gate? (N, C), the block's output."""
    out, y, gate = [], x, None
    layers = list(block.block)
    for layer in layers[:-1]:
        if hasattr(layer, "fc1"):
            gate = se_gate_of(layer, y)
            out.append(gate)
        else:
            y = _conv_block(layer, y)
            out.append(y)
    if gate is not None:
        y = se_scale(y, gate)
    out.append(_conv_block(layers[-1], y, x if block.use_res_connect else None))
    return out


def forward_stages(model, x):
    """(the output of every element of model.features, the logits) of a CPU-resident MobileNetV3 on a numpy batch."""
    from oracle import ref
    from cpu_vision_amd import functional as F
    feats, y = [], np.asarray(x, np.float32)
    for layer in model.features:
        y = block_stages(layer, y)[-1] if hasattr(layer, "block") else _conv_block(layer, y)
        feats.append(y)
    fc1, fc2 = model.classifier[0], model.classifier[3]
    p = lambda t: t.detach().numpy()  # noqa: E731
    z = linear_act(global_avg_pool(y), p(fc1.weight), p(fc1.bias), "hardswish")
    slices, sl = F.linear_k_slices(z.shape[0], z.shape[1], fc2.out_features)
    logits = ref.linear_bias_relu(z, p(fc2.weight), p(fc2.bias), relu=False, **({"slice_len": sl} if slices > 1 else {}))
    return feats, logits


def same(got, want, what=""):
    """NaN in equal places, == elsewhere, same shape; `got` a tensor (any device) or an array."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(got, want, err_msg=what)
