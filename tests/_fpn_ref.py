"""References for the FPN tests (a helper module, not a test file and not a conftest).

1. A plain torch.nn replica of the reference's ops/feature_pyramid_network.py, models/_utils.py::IntermediateLayerGetter and
   models/detection/backbone_utils.py (torchvision is not importable in the test environment), written from the reference's
   source like tests/_resnet_ref.py, on whose ResNet replica the backbones are built: the same classes, constructor arguments,
   child names, construction order and initialisation, with torch's own forward.
2. The oracle composition of a pyramid: oracle.ref.conv2d_affine_act per conv -- the lateral 1x1 convs in the summation order
   F.conv1x1_k_slices states, with R = torch.nn.functional.interpolate(top, size, mode="nearest") (torch on the CPU) as an ordinary
   residual; the 3x3 output convs in the order F.conv3x3_k_slices states without a norm (the MFMA 3x3) and as the single chain
   with one -- and torch on the CPU for max_pool2d(1, 2) and relu, which the oracle does not have.
"""
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from oracle import ref
from tests import _resnet_ref as R
from tests._util import oracle_conv3x3


# ------------------------------------------------------------------------------------------------ the torch.nn replica
class FrozenBatchNorm2d(nn.Module):
    """ops/misc.py:13-65."""

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        key = prefix + "num_batches_tracked"
        if key in state_dict:
            del state_dict[key]
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x):
        w, b = self.weight.reshape(1, -1, 1, 1), self.bias.reshape(1, -1, 1, 1)
        rv, rm = self.running_var.reshape(1, -1, 1, 1), self.running_mean.reshape(1, -1, 1, 1)
        scale = w * (rv + self.eps).rsqrt()
        bias = b - rm * scale
        return x * scale + bias


class Conv2dNormActivation(nn.Sequential):
    """ops/misc.py:68-172 (the arguments the FPN uses)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=None, groups=1, norm_layer=nn.BatchNorm2d,
                 activation_layer=nn.ReLU, dilation=1, inplace=True, bias=None):
        if padding is None:
            padding = (kernel_size - 1) // 2 * dilation
        if bias is None:
            bias = norm_layer is None
        layers = [nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, dilation=dilation, groups=groups, bias=bias)]
        if norm_layer is not None:
            layers.append(norm_layer(out_channels))
        if activation_layer is not None:
            params = {} if inplace is None else {"inplace": inplace}
            layers.append(activation_layer(**params))
        super().__init__(*layers)
        self.out_channels = out_channels


class ExtraFPNBlock(nn.Module):
    def forward(self, results, x, names):
        pass


class FeaturePyramidNetwork(nn.Module):
    _version = 2

    def __init__(self, in_channels_list, out_channels, extra_blocks=None, norm_layer=None):
        super().__init__()
        self.inner_blocks = nn.ModuleList()
        self.layer_blocks = nn.ModuleList()
        for in_channels in in_channels_list:
            if in_channels == 0:
                raise ValueError("in_channels=0 is currently not supported")
            inner_block_module = Conv2dNormActivation(in_channels, out_channels, kernel_size=1, padding=0, norm_layer=norm_layer,
                                                      activation_layer=None)
            layer_block_module = Conv2dNormActivation(out_channels, out_channels, kernel_size=3, norm_layer=norm_layer,
                                                      activation_layer=None)
            self.inner_blocks.append(inner_block_module)
            self.layer_blocks.append(layer_block_module)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        if extra_blocks is not None:
            if not isinstance(extra_blocks, ExtraFPNBlock):
                raise TypeError(f"extra_blocks should be of type ExtraFPNBlock not {type(extra_blocks)}")
        self.extra_blocks = extra_blocks

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:
            num_blocks = len(self.inner_blocks)
            for block in ["inner_blocks", "layer_blocks"]:
                for i in range(num_blocks):
                    for type in ["weight", "bias"]:
                        old_key = f"{prefix}{block}.{i}.{type}"
                        new_key = f"{prefix}{block}.{i}.0.{type}"
                        if old_key in state_dict:
                            state_dict[new_key] = state_dict.pop(old_key)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x):
        names = list(x.keys())
        x = list(x.values())
        last_inner = self.inner_blocks[-1](x[-1])
        results = [self.layer_blocks[-1](last_inner)]
        for idx in range(len(x) - 2, -1, -1):
            inner_lateral = self.inner_blocks[idx](x[idx])
            feat_shape = inner_lateral.shape[-2:]
            inner_top_down = nn.functional.interpolate(last_inner, size=feat_shape, mode="nearest")
            last_inner = inner_lateral + inner_top_down
            results.insert(0, self.layer_blocks[idx](last_inner))
        if self.extra_blocks is not None:
            results, names = self.extra_blocks(results, x, names)
        return OrderedDict([(k, v) for k, v in zip(names, results)])


class LastLevelMaxPool(ExtraFPNBlock):
    def forward(self, x, y, names):
        names.append("pool")
        x.append(nn.functional.max_pool2d(x[-1], kernel_size=1, stride=2, padding=0))
        return x, names


class LastLevelP6P7(ExtraFPNBlock):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.p6 = nn.Conv2d(in_channels, out_channels, 3, 2, 1)
        self.p7 = nn.Conv2d(out_channels, out_channels, 3, 2, 1)
        for module in [self.p6, self.p7]:
            nn.init.kaiming_uniform_(module.weight, a=1)
            nn.init.constant_(module.bias, 0)
        self.use_P5 = in_channels == out_channels

    def forward(self, p, c, names):
        p5, c5 = p[-1], c[-1]
        x = p5 if self.use_P5 else c5
        p6 = self.p6(x)
        p7 = self.p7(nn.functional.relu(p6))
        p.extend([p6, p7])
        names.extend(["p6", "p7"])
        return p, names


class IntermediateLayerGetter(nn.ModuleDict):
    _version = 2

    def __init__(self, model, return_layers):
        if not set(return_layers).issubset([name for name, _ in model.named_children()]):
            raise ValueError("return_layers are not present in model")
        orig_return_layers = return_layers
        return_layers = {str(k): str(v) for k, v in return_layers.items()}
        layers = OrderedDict()
        for name, module in model.named_children():
            layers[name] = module
            if name in return_layers:
                del return_layers[name]
            if not return_layers:
                break
        super().__init__(layers)
        self.return_layers = orig_return_layers

    def forward(self, x):
        out = OrderedDict()
        for name, module in self.items():
            x = module(x)
            if name in self.return_layers:
                out[self.return_layers[name]] = x
        return out


class BackboneWithFPN(nn.Module):
    def __init__(self, backbone, return_layers, in_channels_list, out_channels, extra_blocks=None, norm_layer=None):
        super().__init__()
        if extra_blocks is None:
            extra_blocks = LastLevelMaxPool()
        self.body = IntermediateLayerGetter(backbone, return_layers=return_layers)
        self.fpn = FeaturePyramidNetwork(in_channels_list=in_channels_list, out_channels=out_channels, extra_blocks=extra_blocks,
                                         norm_layer=norm_layer)
        self.out_channels = out_channels

    def forward(self, x):
        return self.fpn(self.body(x))


def resnet_fpn_backbone(*, backbone_name, norm_layer=FrozenBatchNorm2d, trainable_layers=3, returned_layers=None, extra_blocks=None):
    """backbone_utils.py:62-114 without `weights` (no weight files)."""
    backbone = getattr(R, backbone_name)(norm_layer=norm_layer)
    return _resnet_fpn_extractor(backbone, trainable_layers, returned_layers, extra_blocks)


def _resnet_fpn_extractor(backbone, trainable_layers, returned_layers=None, extra_blocks=None, norm_layer=None):
    if trainable_layers < 0 or trainable_layers > 5:
        raise ValueError(f"Trainable layers should be in the range [0,5], got {trainable_layers}")
    layers_to_train = ["layer4", "layer3", "layer2", "layer1", "conv1"][:trainable_layers]
    if trainable_layers == 5:
        layers_to_train.append("bn1")
    for name, parameter in backbone.named_parameters():
        if all([not name.startswith(layer) for layer in layers_to_train]):
            parameter.requires_grad_(False)
    if extra_blocks is None:
        extra_blocks = LastLevelMaxPool()
    if returned_layers is None:
        returned_layers = [1, 2, 3, 4]
    if min(returned_layers) <= 0 or max(returned_layers) >= 5:
        raise ValueError(f"Each returned layer should be in the range [1,4]. Got {returned_layers}")
    return_layers = {f"layer{k}": str(v) for v, k in enumerate(returned_layers)}
    in_channels_stage2 = backbone.inplanes // 8
    in_channels_list = [in_channels_stage2 * 2 ** (i - 1) for i in returned_layers]
    out_channels = 256
    return BackboneWithFPN(backbone, return_layers, in_channels_list, out_channels, extra_blocks=extra_blocks, norm_layer=norm_layer)


# ------------------------------------------------------------------------------------------------ the oracle composition
def nearest(top, size):
    """torch's CPU F.interpolate(top, size=size, mode="nearest") on numpy arrays: the reference of the source index."""
    return nn.functional.interpolate(torch.from_numpy(np.ascontiguousarray(top)), size=tuple(size), mode="nearest").numpy()


def folded(norm):
    """(alpha, beta, affine code) of a norm container or None; FrozenBatchNorm2d of either the replica or the library."""
    if norm is None:
        return None, None, 0
    return R.folded(norm)


def oracle_lateral(x, w, bias, alpha, beta, top, affine, act, slice_len=None):
    """The fused lateral: the pointwise conv in the order the library states for the shape, the upsampled `top` as its residual."""
    from cpu_vision_amd import functional as F
    n, cin, h, wd = x.shape
    if slice_len is None:
        slices, sl = F.conv1x1_k_slices(n, cin, h, wd, w.shape[0])
        slice_len = sl if slices > 1 else 0
    res = None if top is None else nearest(top, (h, wd))
    return ref.conv2d_affine_act(x, np.ascontiguousarray(w.reshape(w.shape[0], cin, 1, 1)), bias, alpha, beta, res, 1, 0, 1, affine, act,
                                 slice_len=slice_len)


def _block_parts(block):
    conv = block[0]
    norm = block[1] if len(block) > 1 else None
    bias = None if conv.bias is None else conv.bias.detach().numpy()
    return conv.weight.detach().numpy(), bias, folded(norm)


def oracle_fpn(fpn, feats):
    """A FeaturePyramidNetwork (CPU-resident; the library's or the replica's: same children) on an OrderedDict of numpy maps ->
    OrderedDict of numpy levels, level by level as the reference's forward."""
    names, x = list(feats.keys()), [np.ascontiguousarray(v, np.float32) for v in feats.values()]

    def inner(idx, top):
        w, bias, (a, b, code) = _block_parts(fpn.inner_blocks[idx])
        return oracle_lateral(x[idx], w, bias, a, b, top, code, None)

    def layer(idx, v):
        w, bias, (a, b, code) = _block_parts(fpn.layer_blocks[idx])
        if code == 0:
            return oracle_conv3x3(ref, v, w, bias, relu=False)
        return ref.conv2d_affine_act(v, w, bias, a, b, None, 1, 1, 1, code, None, slice_len=0)

    last_inner = inner(-1, None)
    results = [layer(-1, last_inner)]
    for idx in range(len(x) - 2, -1, -1):
        last_inner = inner(idx, last_inner)
        results.insert(0, layer(idx, last_inner))
    extra = fpn.extra_blocks
    if extra is not None and hasattr(extra, "p6"):
        src = results[-1] if extra.use_P5 else x[-1]
        conv = lambda m, v: ref.conv2d_affine_act(v, m.weight.detach().numpy(), m.bias.detach().numpy(), None, None, None, 2, 1, 1, 0, None,  # noqa: E731
                                                  slice_len=0)
        p6 = conv(extra.p6, src)
        p7 = conv(extra.p7, torch.relu(torch.from_numpy(p6)).numpy())
        results, names = results + [p6, p7], names + ["p6", "p7"]
    elif extra is not None:
        pool = nn.functional.max_pool2d(torch.from_numpy(results[-1]), kernel_size=1, stride=2, padding=0).numpy()
        results, names = results + [pool], names + ["pool"]
    return OrderedDict(zip(names, results))


def oracle_body(body, x):
    """The IntermediateLayerGetter of a ResNet (conv1, bn1, relu, maxpool, layer1 ...) through the oracle -> OrderedDict."""
    a = R.oracle_conv_norm(np.ascontiguousarray(x, np.float32), body["conv1"], body["bn1"], relu=True)
    mp = body["maxpool"]
    a = R.padded_max_pool(a, mp.kernel_size, mp.stride, mp.padding)
    out = OrderedDict()
    for name in ("layer1", "layer2", "layer3", "layer4"):
        if name not in body:
            break
        for block in body[name]:
            a = R.oracle_block(block, a)
        if name in body.return_layers:
            out[body.return_layers[name]] = a
    return out


def oracle_backbone(model, x):
    return oracle_fpn(model.fpn, oracle_body(model.body, x))


def randomize(model, seed):
    """Non-trivial norms (R.randomize_norms) and conv biases (the FPN initialises them to zero, which would hide a dropped bias)."""
    R.randomize_norms(model, seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.Conv2d) and m.bias is not None:
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
