"""What the ConvNeXt tests compare with (a helper module, not a conftest):

  * a plain-torch replica of the reference's modules (models/convnext.py LayerNorm2d / CNBlock / CNBlockConfig / ConvNeXt, ops/misc.py
    Permute, ops/stochastic_depth.py StochasticDepth), written from the reference's published structure: the same constructor arguments,
    children, names and initialisation, and torch's own forward -- for trees, state-dict keys, seeded initialisation and the float32 /
    float64 evaluations of the accuracy conditions;
  * numpy restatements of the arithmetic mi355vision.h states for mv_layer_norm2d_stats_f32 / mv_layer_norm2d_f32 (float64 sums in the
    stated order: 16 channel groups, ascending inside a group, the groups added in ascending order; four float32 roundings) and for
    the GELU of mv_conv1x1_ln_gelu_f32 (math.erf on the float64 of t, one cast);
  * forward_stages: a whole network stage by stage, every conv through oracle.ref.conv2d_affine_act (in the summation order
    F.conv1x1_k_slices states for the pointwise ones).
"""
import math
from functools import partial

import numpy as np
import torch
from torch import nn

from tests._mobilenetv3_ref import global_avg_pool, same  # noqa: F401  (the float64-summed pool; NaN-aware equality)

LN_GROUPS = 16  # channel q belongs to group q % 16 (layernorm.hip)


# ------------------------------------------------------------------------------------------------------------- torch replica
class TPermute(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.dims = dims

    def forward(self, x):
        return torch.permute(x, self.dims)


class TStochasticDepth(nn.Module):
    def __init__(self, p, mode):
        super().__init__()
        self.p, self.mode = p, mode

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        survival = 1.0 - self.p
        size = [x.shape[0]] + [1] * (x.ndim - 1) if self.mode == "row" else [1] * x.ndim
        noise = torch.empty(size, dtype=x.dtype, device=x.device).bernoulli_(survival)
        if survival > 0.0:
            noise.div_(survival)
        return x * noise


class TLayerNorm2d(nn.LayerNorm):
    def forward(self, x):
        x = x.permute(0, 2, 3, 1)
        x = nn.functional.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
        return x.permute(0, 3, 1, 2)


class TCNBlock(nn.Module):
    def __init__(self, dim, layer_scale, stochastic_depth_prob, norm_layer=None):
        super().__init__()
        if norm_layer is None:
            norm_layer = partial(nn.LayerNorm, eps=1e-6)
        self.block = nn.Sequential(nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True), TPermute([0, 2, 3, 1]), norm_layer(dim),
                                   nn.Linear(dim, 4 * dim, bias=True), nn.GELU(), nn.Linear(4 * dim, dim, bias=True), TPermute([0, 3, 1, 2]))
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)
        self.stochastic_depth = TStochasticDepth(stochastic_depth_prob, "row")

    def forward(self, input):
        result = self.layer_scale * self.block(input)
        result = self.stochastic_depth(result)
        result += input
        return result


class TCNBlockConfig:
    def __init__(self, input_channels, out_channels, num_layers):
        self.input_channels, self.out_channels, self.num_layers = input_channels, out_channels, num_layers


class TConvNeXt(nn.Module):
    def __init__(self, block_setting, stochastic_depth_prob=0.0, layer_scale=1e-6, num_classes=1000, block=None, norm_layer=None):
        super().__init__()
        if not block_setting:
            raise ValueError("The block_setting should not be empty")
        elif not (isinstance(block_setting, (list, tuple)) and all(isinstance(s, TCNBlockConfig) for s in block_setting)):
            raise TypeError("The block_setting should be List[CNBlockConfig]")
        block = TCNBlock if block is None else block
        norm_layer = partial(TLayerNorm2d, eps=1e-6) if norm_layer is None else norm_layer
        c0 = block_setting[0].input_channels
        layers = [nn.Sequential(nn.Conv2d(3, c0, kernel_size=4, stride=4, padding=0, bias=True), norm_layer(c0))]
        total = sum(cnf.num_layers for cnf in block_setting)
        block_id = 0
        for cnf in block_setting:
            stage = []
            for _ in range(cnf.num_layers):
                stage.append(block(cnf.input_channels, layer_scale, stochastic_depth_prob * block_id / (total - 1.0)))
                block_id += 1
            layers.append(nn.Sequential(*stage))
            if cnf.out_channels is not None:
                layers.append(nn.Sequential(norm_layer(cnf.input_channels), nn.Conv2d(cnf.input_channels, cnf.out_channels, kernel_size=2, stride=2)))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        last = block_setting[-1]
        c_last = last.out_channels if last.out_channels is not None else last.input_channels
        self.classifier = nn.Sequential(norm_layer(c_last), nn.Flatten(1), nn.Linear(c_last, num_classes))
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, x):
        return self.classifier(self.avgpool(self.features(x)))


SETTINGS = {"convnext_tiny": ([(96, 192, 3), (192, 384, 3), (384, 768, 9), (768, None, 3)], 0.1),
            "convnext_small": ([(96, 192, 3), (192, 384, 3), (384, 768, 27), (768, None, 3)], 0.4),
            "convnext_base": ([(128, 256, 3), (256, 512, 3), (512, 1024, 27), (1024, None, 3)], 0.5),
            "convnext_large": ([(192, 384, 3), (384, 768, 3), (768, 1536, 27), (1536, None, 3)], 0.5)}


def replica(arch_or_rows, **kwargs):
    """The torch replica of a builder ("convnext_tiny" ...) or of a custom list of (input_channels, out_channels, num_layers) rows."""
    if isinstance(arch_or_rows, str):
        rows, sd = SETTINGS[arch_or_rows]
        kwargs.setdefault("stochastic_depth_prob", sd)
    else:
        rows = arch_or_rows
    return TConvNeXt([TCNBlockConfig(*r) for r in rows], **kwargs)


def perturb(model, seed, layer_scale=None):
    """Seeded values away from the initialisation for every LayerNorm's terms, every bias and every layer_scale (in module order), on
    the library's model or the replica (the same state-dict keys).  layer_scale: a fixed value instead of seeded ones around 0.5."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
            elif isinstance(m, (nn.Conv2d, nn.Linear)):
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
            if hasattr(m, "layer_scale"):
                ls = torch.rand(m.layer_scale.shape, generator=g) * 0.5 + 0.25
                m.layer_scale.copy_(ls if layer_scale is None else torch.full_like(ls, layer_scale))


def scale_weights(model, factor):
    """Every conv's and dense layer's weight times `factor`: trunc_normal_(std=0.02) leaves the branch of a block a few hundred times
    smaller than its input, and a test of the branch wants it to weigh as much."""
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                m.weight.mul_(factor)


# ------------------------------------------------------------------------------------------------------------- restatements
def _fold(v):
    """(n, c, h, w) float64 -> (n, h, w): group g adds its channels q = g, g + 16, ... in ascending order to 0.0; the 16 partial sums
    are added in ascending g to 0.0."""
    n, c, h, w = v.shape
    part = np.zeros((LN_GROUPS, n, h, w), np.float64)
    for q in range(c):
        part[q % LN_GROUPS] = part[q % LN_GROUPS] + v[:, q]
    s = np.zeros((n, h, w), np.float64)
    for g in range(LN_GROUPS):
        s = s + part[g]
    return s


def layer_norm2d_stats(x, eps):
    """mv_layer_norm2d_stats_f32: (mean, rstd), each (n, h, w) float32."""
    x = np.asarray(x, np.float32)
    c = np.float64(x.shape[1])
    xd = x.astype(np.float64)
    with np.errstate(all="ignore"):
        m = _fold(xd) / c
        d = xd - m[:, None]
        q = _fold(d * d)
        rstd = np.float64(1.0) / np.sqrt(q / c + np.float64(np.float32(eps)))
    return m.astype(np.float32), rstd.astype(np.float32)


def layer_norm2d_apply(x, mean, rstd, weight=None, bias=None):
    """fl(fl(fl(fl(x - mean) rstd) w) + b): four float32 roundings, the last two dropped without the term."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        y = ((x - mean[:, None]).astype(np.float32) * rstd[:, None]).astype(np.float32)
        if weight is not None:
            y = (y * np.asarray(weight, np.float32).reshape(1, -1, 1, 1)).astype(np.float32)
        if bias is not None:
            y = (y + np.asarray(bias, np.float32).reshape(1, -1, 1, 1)).astype(np.float32)
    return y


def layer_norm2d(x, weight=None, bias=None, eps=1e-6):
    """mv_layer_norm2d_f32 on (n, c, h, w)."""
    mean, rstd = layer_norm2d_stats(x, eps)
    return layer_norm2d_apply(x, mean, rstd, weight, bias)


_erf = np.frompyfunc(math.erf, 1, 1)
INV_SQRT2 = np.float32(0.70710678118654752440)


def gelu_arguments(v):
    """t = fl(v * 0.70710678f), the float32 values whose erf the GELU takes."""
    with np.errstate(all="ignore"):
        return (np.asarray(v, np.float32) * INV_SQRT2).astype(np.float32)


def gelu(v):
    """fl(fl(0.5 v) fl(1 + E)), E = (float)erf((double)t)."""
    v = np.asarray(v, np.float32)
    t = gelu_arguments(v)
    e = _erf(t.astype(np.float64)).astype(np.float64).astype(np.float32).reshape(v.shape)
    with np.errstate(all="ignore"):
        return ((np.float32(0.5) * v).astype(np.float32) * (np.float32(1) + e).astype(np.float32)).astype(np.float32)


def pointwise(x, w, b=None, alpha=None, beta=None, res=None, affine=0, slice_len=None):
    """The pointwise conv in the summation order F.conv1x1_k_slices states for its shape (slice_len: of another shape, whose pixels
    these are a sample of), through the oracle."""
    from oracle import ref
    from cpu_vision_amd import functional as F
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    if slice_len is None:
        slices, sl = F.conv1x1_k_slices(n, cin, h, wd, cout)
        slice_len = sl if slices > 1 else 0
    return ref.conv2d_affine_act(x, w.reshape(cout, cin, 1, 1), b, alpha, beta, res, 1, 0, 1, affine, None, slice_len=slice_len)


def conv1x1_gelu(x, w, b=None, norm=None, gelu_on=True, pre=None, slice_len=None):
    """F.conv1x1_gelu: norm = (mean, rstd, ln_w, ln_b) or None.  pre: a list that receives the value GELU is applied to."""
    z = np.asarray(x, np.float32) if norm is None else layer_norm2d_apply(x, *norm)
    v = pointwise(z, w, b, slice_len=slice_len)
    if pre is not None:
        pre.append(v)
    return gelu(v) if gelu_on else v


# ------------------------------------------------------------------------------------------------------------- stage-by-stage forward
def _p(t):
    return None if t is None else t.detach().cpu().numpy()


def block_stages(block, x, pre=None):
    """One CNBlock (the library's or the replica's) on a numpy x: what each launch of the library's forward produces -- the depthwise
    conv, (mean, rstd), Linear + GELU, the block's output."""
    from oracle import ref
    conv, norm, fc1, fc2 = block.block[0], block.block[2], block.block[3], block.block[5]
    dim = conv.out_channels
    h = ref.conv2d_affine_act(x, _p(conv.weight), _p(conv.bias), None, None, None, 1, 3, dim, 0, None)
    stats = layer_norm2d_stats(h, norm.eps)
    g = conv1x1_gelu(h, _p(fc1.weight), _p(fc1.bias), norm=stats + (_p(norm.weight), _p(norm.bias)), pre=pre)
    out = pointwise(g, _p(fc2.weight), _p(fc2.bias), _p(block.layer_scale).reshape(dim), np.zeros(dim, np.float32), x, affine=1)
    return [h, stats, g, out]


def _ln_module(m, x):
    return layer_norm2d(x, _p(m.weight), _p(m.bias), m.eps)


def _conv_module(conv, x):
    from oracle import ref
    return ref.conv2d_affine_act(x, _p(conv.weight), _p(conv.bias), None, None, None, conv.stride[0], conv.padding[0], 1, 0, None)


def forward_stages(model, x, pre=None):
    """(the output of every element of model.features, the logits) of a CPU-resident ConvNeXt on a numpy batch.  pre: a list that
    receives every value a GELU is applied to."""
    from oracle import ref
    from cpu_vision_amd import functional as F
    feats, y = [], np.asarray(x, np.float32)
    for i, layer in enumerate(model.features):
        if i == 0:
            y = _ln_module(layer[1], _conv_module(layer[0], y))
        elif isinstance(layer[0], nn.LayerNorm):
            y = _conv_module(layer[1], _ln_module(layer[0], y))
        else:
            for blk in layer:
                y = block_stages(blk, y, pre)[-1]
        feats.append(y)
    norm, fc = model.classifier[0], model.classifier[2]
    z = global_avg_pool(y)
    z = _ln_module(norm, z[:, :, None, None])[:, :, 0, 0]
    slices, sl = F.linear_k_slices(z.shape[0], z.shape[1], fc.out_features)
    logits = ref.linear_bias_relu(z, _p(fc.weight), _p(fc.bias), relu=False, **({"slice_len": sl} if slices > 1 else {}))
    return feats, logits


# ------------------------------------------------------------------------------------------------------------- the GPU tests' shapes
def dw7x7_plan(n, c, h, w):
    """(rows of a strip, threads) of launch_dwpc7x7, restated from dw7x7.hip with its two constants."""
    from tests._fuzz_cases import constant
    rows, short = constant("kDw7Rows"), constant("kDw7ShortLaunch")
    gx = (w + 3) // 4
    if n * c * -(-h // rows) * gx < short:
        rows //= 2
    return rows, n * c * -(-h // rows) * gx


def pw_plan(n, cin, hw, cout):
    """(NT, MW, KS) of the pointwise kernel for a shape, restated from convnorm.hip's pw_plan."""
    mw = 1 if cout <= 32 else (2 if cout <= 64 else 4)
    wave_tiles = -(-cout // 32) * -(-hw // 32) * n
    nt = 1 if wave_tiles <= 8192 else (2 if (wave_tiles <= 32768 or mw == 1) else 4)
    if cin >= 512 and mw == 4:
        mb = -(-cout // 128)
        if mb * -(-hw // 128) * n >= 512:
            nt = 4
        elif mb * -(-hw // 64) * n >= 512:
            nt = 2
    chunks = -(-cin // 32)
    if chunks == 1:
        mw, nt = 1, 1
    pxb = (4 // mw) * nt * 32
    workgroups = -(-cout // (mw * 32)) * -(-hw // pxb) * n
    ks = 1
    if nt == 1 and workgroups <= 640 and chunks >= 6:
        ks = 4 if chunks >= 12 else 2
    return nt, mw, ks


def ln_kernel_name(n, cin, hw, cout, norm):
    nt, mw, ks = pw_plan(n, cin, hw, cout)
    loads = "norm" if norm else "plain"
    return f"k_conv1x1_ln<1,{mw},ks{ks},{loads}>" if ks > 1 else f"k_conv1x1_ln<{nt},{mw},{loads}>"


def pixels_per_workgroup(nt, mw):
    return (4 // mw) * nt * 32


# (n, cin, cout, h, w): the 32-row chunk (cin 31, 32, 33, 96) x cout around 32, 64 and the widest channel tile (128) ...
PW_SMALL = [(1, cin, cout, 7, 9) for cin in (31, 32, 33, 96) for cout in (31, 32, 33, 63, 64, 65, 127, 128, 129)]
# ... H W one below, at and one above the pixels of a workgroup of the three one-tile instances (128, 64, 32), batch 2 ...
PW_SMALL += [(2, 33, cout, 1, pxb + d) for cout, pxb in ((32, 128), (64, 64), (128, 32)) for d in (-1, 0, 1)]
# ... one pixel; the K-slice instances (6 and 13 chunks on few workgroups) for each channel-tile count ...
PW_SMALL += [(1, 33, 40, 1, 1), (2, 3, 5, 1, 7)]
PW_SMALL += [(n, cin, cout, 5, 5) for cin in (192, 416) for cout, n in ((32, 1), (64, 2), (128, 1))]
# ... the same three pixel counts for the six K-slice instances ...
PW_SMALL += [(1, cin, cout, 1, pxb + d) for cin in (192, 416) for cout, pxb in ((32, 128), (64, 64), (128, 32)) for d in (-1, 0, 1)]
# ... and the instances with two and four pixel tiles per wave, which only large launches reach: compared on a sample of pixels that
# holds the last 300 of the plane.  H W = k PXB - 1, k PXB, k PXB + 1 with PXB the instance's pixels per workgroup (256, 128, 64, 256, 128)
PW_LARGE = [(1, 33, 32, 520, 513), (1, 33, 64, 363, 365), (2, 33, 128, 182, 181), (2, 33, 64, 517, 513), (2, 33, 128, 365, 363)]
PW_LARGE += [(n, 33, cout, 1, k * pxb + d) for n, cout, k, pxb in ((1, 32, 1025, 256), (1, 64, 1025, 128), (2, 128, 513, 64), (2, 64, 1025, 256),
                                                                  (2, 128, 1025, 128)) for d in (-1, 0, 1)]
LN_INSTANCES = {(1, 1, 1), (1, 2, 1), (1, 4, 1), (2, 1, 1), (2, 2, 1), (2, 4, 1), (4, 2, 1), (4, 4, 1), (1, 1, 2), (1, 2, 2), (1, 4, 2), (1, 1, 4),
                (1, 2, 4), (1, 4, 4)}


def pw_case(i, shape):
    """The seeded inputs of one conv1x1_gelu case: x, w, b, ln_w, ln_b."""
    n, cin, cout, h, w = shape
    g = np.random.Generator(np.random.Philox(7000 + i))
    f = lambda shp, s=1.0: (g.standard_normal(shp) * s).astype(np.float32)  # noqa: E731
    return f((n, cin, h, w)) + np.float32(0.25), f((cout, cin), 2.0 / math.sqrt(cin)), f(cout), f(cin) + np.float32(1.5), f(cin)


def sample_pixels(hw, seed=0):
    """Pixel indices a large case is compared on: both ends of the plane and 300 seeded ones."""
    g = np.random.Generator(np.random.Philox(seed))
    idx = np.concatenate([np.arange(min(300, hw)), np.arange(max(hw - 300, 0), hw), g.integers(0, hw, 300)])
    return np.unique(idx)


# tests/test_gpu_convnext_guard.py's shapes (inputs: pw_case(GUARD_SEED, shape)) and the values of the special-value test of
# tests/test_gpu_convnext.py: they too are compared bit for bit through GELU
GUARD_PW_CASES = [(1, 1, 1, 1, 1), (2, 3, 5, 1, 7), (1, 33, 31, 3, 5), (2, 40, 65, 1, 33), (1, 192, 33, 3, 3), (1, 416, 70, 1, 5)]
GUARD_SEED = 99
SPECIAL_GELU_VALUES = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 1e-30, 30.0, -30.0], np.float32)

BLOCK_CASES = [(8, 9, 11), (96, 7, 7)]  # (dim, h, w)
NET_ROWS = [(8, 16, 1), (16, 24, 2), (24, None, 1)]


def block_pair(dim, seed, builder, layer_scale=None, weight_factor=8.0):
    """(replica, the library's CNBlock on the CPU with the same perturbed state)."""
    torch.manual_seed(seed)
    rep = TCNBlock(dim, 1e-6, 0.0).eval()
    perturb(rep, seed + 1, layer_scale)
    scale_weights(rep, weight_factor)
    cpu = builder(dim, 1e-6, 0.0).eval()
    cpu.load_state_dict(rep.state_dict(), strict=True)
    return rep, cpu


def net_pair(arch_or_rows, seed, builder, **kw):
    torch.manual_seed(seed)
    rep = replica(arch_or_rows, num_classes=7, **kw).eval()
    perturb(rep, seed + 1)
    scale_weights(rep, 6.0)
    cpu = builder(num_classes=7, **kw)
    cpu.load_state_dict(rep.state_dict(), strict=True)
    return rep, cpu


def block_input(dim, h, w, seed):
    return (np.random.Generator(np.random.Philox(seed)).standard_normal((2, dim, h, w))).astype(np.float32)


def erf_margin_ulps(t):
    """For float32 GELU arguments t: the distance of erf((double)t) from the nearest float32 rounding midpoint, in float64 ulps of the
    value; NaN arguments and saturated |erf| == 1 values are left out."""
    t = np.asarray(t, np.float32).reshape(-1)
    t = t[~np.isnan(t)]
    e = torch.erf(torch.from_numpy(t.astype(np.float64))).numpy()
    e = e[np.abs(e) != 1.0]
    f = e.astype(np.float32)
    up, down = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
    mid_up, mid_down = (f.astype(np.float64) + up.astype(np.float64)) / 2, (f.astype(np.float64) + down.astype(np.float64)) / 2
    dist = np.minimum(np.abs(e - mid_up), np.abs(e - mid_down))
    return dist / np.spacing(np.abs(e))
