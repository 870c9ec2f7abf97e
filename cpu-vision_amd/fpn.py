"""FeaturePyramidNetwork on the MI355X kernels: every lateral conv and its top-down merge is ONE launch.

Mirrors ops/feature_pyramid_network.py of the reference the way resnet.py mirrors models/resnet.py: same classes, constructor
arguments, child names (inner_blocks.i.0, layer_blocks.i.0, extra_blocks.p6 ...), state-dict keys (with the version-1 key
renaming) and initialisation order; the package's Conv2dNormActivation (torch's own nn.Conv2d and norm as PARAMETER CONTAINERS)
holds the parameters.  Only `forward` differs.  The reference computes per level

    last_inner = inner_block(x[idx]) + F.interpolate(last_inner, size=feat_shape, mode="nearest")

-- three passes over the largest maps of the network.  Here the lateral 1x1 conv reads the coarser map through torch's nearest
source index in its own epilogue (F.conv1x1_upsample_add: k_conv1x1_up), so neither the upsampled map nor a separate sum ever
exists.  A pyramid of L levels is exactly 2 L launches plus the extra block's: the coarsest lateral is F.conv_norm_act, every
other lateral one F.conv1x1_upsample_add, every 3x3 output conv F.conv2d_bias_relu(relu=False) (the MFMA 3x3; order:
F.conv3x3_k_slices) without a norm and F.conv2d_affine_act with one.  Inference only: norms are nn.BatchNorm2d in eval mode or
FrozenBatchNorm2d, folded into the conv.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _lib
from . import functional as F
from .mobilenet import Conv2dNormActivation

__all__ = ["ExtraFPNBlock", "FeaturePyramidNetwork", "LastLevelMaxPool", "LastLevelP6P7"]


class ExtraFPNBlock(nn.Module):
    """feature_pyramid_network.py:11-32: base class of the extra block.  forward(results, x, names) takes the FPN's outputs, the
    original feature maps and their names and returns the extended (results, names)."""

    def forward(self, results: List[torch.Tensor], x: List[torch.Tensor], names: List[str]) -> Tuple[List[torch.Tensor], List[str]]:
        pass


class FeaturePyramidNetwork(nn.Module):
    """feature_pyramid_network.py:35-201.  forward takes an OrderedDict of feature maps in increasing depth order and returns
    an OrderedDict of the pyramid's levels, highest resolution first, under the same names (plus the extra block's)."""

    _version = 2

    def __init__(self, in_channels_list: List[int], out_channels: int, extra_blocks: Optional[ExtraFPNBlock] = None,
                 norm_layer: Optional[Callable[..., nn.Module]] = None):
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

        # initialize parameters now to avoid modifying the initialization of top_blocks
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

        if extra_blocks is not None:
            if not isinstance(extra_blocks, ExtraFPNBlock):
                raise TypeError(f"extra_blocks should be of type ExtraFPNBlock not {type(extra_blocks)}")
        self.extra_blocks = extra_blocks
        self.eval()

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

    def get_result_from_inner_blocks(self, x: torch.Tensor, idx: int, top: Optional[torch.Tensor] = None) -> torch.Tensor:
        """inner_blocks[idx](x) [+ interpolate(top, size=x.shape[-2:], mode="nearest")], one launch either way."""
        block = self.inner_blocks[idx]
        if top is None:
            return block(x)
        conv = block[0]
        alpha, beta, mode = block._fold.get(block[1] if block._has_norm else None, x.device)
        return F.conv1x1_upsample_add(x, conv.weight, conv.bias, alpha, beta, top, affine=mode)

    def get_result_from_layer_blocks(self, x: torch.Tensor, idx: int) -> torch.Tensor:
        """layer_blocks[idx](x): without a norm the block's own path (the MFMA 3x3 of F.conv2d_bias_relu), with one the implicit
        GEMM with the full epilogue -- Conv2dNormActivation itself has no dense 3x3 with a norm beyond the stem's cin <= 4."""
        block = self.layer_blocks[idx]
        if not block._has_norm:
            return block(x)
        conv = block[0]
        alpha, beta, mode = block._fold.get(block[1], x.device)
        return F.conv2d_affine_act(x, conv.weight, conv.bias, alpha, beta, None, stride=1, padding=1, affine=mode)

    def forward(self, x: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        if self.training:
            raise RuntimeError("the MI355X FeaturePyramidNetwork is inference only: call .eval()")
        # unpack OrderedDict into two lists for easier handling
        names = list(x.keys())
        x = list(x.values())
        with torch.no_grad():  # no autograd bookkeeping per launch; the results are marked once (their backward raises)
            last_inner = self.get_result_from_inner_blocks(x[-1], -1)
            results = [self.get_result_from_layer_blocks(last_inner, -1)]
            for idx in range(len(x) - 2, -1, -1):
                last_inner = self.get_result_from_inner_blocks(x[idx], idx, top=last_inner)
                results.insert(0, self.get_result_from_layer_blocks(last_inner, idx))
            if self.extra_blocks is not None:
                results, names = self.extra_blocks(results, x, names)
        deps = (*x, self.inner_blocks[0][0].weight)
        # make it back an OrderedDict
        return OrderedDict([(k, _lib.forward_only(v, "FeaturePyramidNetwork.forward", *deps)) for k, v in zip(names, results)])


class LastLevelMaxPool(ExtraFPNBlock):
    """feature_pyramid_network.py:204-219: max_pool2d(kernel 1, stride 2) on top of the last feature map."""

    def forward(self, x: List[torch.Tensor], y: List[torch.Tensor], names: List[str]) -> Tuple[List[torch.Tensor], List[str]]:
        names.append("pool")
        # Use max pooling to simulate stride 2 subsampling
        x.append(F.max_pool2d(x[-1], 1, 2, 0))
        return x, names


class LastLevelP6P7(ExtraFPNBlock):
    """feature_pyramid_network.py:222-250: the two extra 3x3 stride-2 levels of RetinaNet, one launch each; the ReLU between
    them is applied to P6's copy only (P6 itself is returned without it, as in the reference)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.p6 = nn.Conv2d(in_channels, out_channels, 3, 2, 1)
        self.p7 = nn.Conv2d(out_channels, out_channels, 3, 2, 1)
        for module in [self.p6, self.p7]:
            nn.init.kaiming_uniform_(module.weight, a=1)
            nn.init.constant_(module.bias, 0)
        self.use_P5 = in_channels == out_channels

    def forward(self, p: List[torch.Tensor], c: List[torch.Tensor], names: List[str]) -> Tuple[List[torch.Tensor], List[str]]:
        p5, c5 = p[-1], c[-1]
        x = p5 if self.use_P5 else c5
        p6 = F.conv2d_affine_act(x, self.p6.weight, self.p6.bias, stride=2, padding=1)
        p7 = F.conv2d_affine_act(torch.relu(p6), self.p7.weight, self.p7.bias, stride=2, padding=1)
        p.extend([p6, p7])
        names.extend(["p6", "p7"])
        return p, names
