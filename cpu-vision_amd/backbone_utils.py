"""IntermediateLayerGetter, BackboneWithFPN and resnet_fpn_backbone on the MI355X kernels.

Mirrors models/_utils.py:13-75 (IntermediateLayerGetter) and models/detection/backbone_utils.py (BackboneWithFPN,
resnet_fpn_backbone, _resnet_fpn_extractor, _validate_trainable_layers) of the reference: same classes, arguments, child names
(body.conv1 ... body.layer4, fpn.inner_blocks ...), state-dict keys and messages.  In this package the parameter containers' own
forward is never called, so the getter does not call its children one by one: it runs the fused path the models run --
a Conv2d, norm[, ReLU] run of children is ONE resnet.fused_conv_norm launch, MaxPool2d is F.max_pool2d, a Sequential of the
package's blocks is called as it is, and so is a block on its own (the children "0" ... "16" of a MobileNetV3's `features`, the
backbone of LRASPP and deeplabv3_mobilenet_v3_large).  A model with any other child is refused at construction.  Inference only.
"""
from __future__ import annotations

import warnings
from collections import OrderedDict
from typing import Callable, Dict, List, Optional

import torch
from torch import nn

from . import _lib, mobilenetv3, resnet
from . import functional as F
from .fpn import ExtraFPNBlock, FeaturePyramidNetwork, LastLevelMaxPool
from .mobilenet import Conv2dNormActivation, FrozenBatchNorm2d, InvertedResidual, _FoldedNorm

__all__ = ["IntermediateLayerGetter", "BackboneWithFPN", "resnet_fpn_backbone"]

_NORMS = (nn.BatchNorm2d, FrozenBatchNorm2d)
_BLOCKS = (resnet.BasicBlock, resnet.Bottleneck, Conv2dNormActivation, InvertedResidual, mobilenetv3.InvertedResidual)


def _fused_plan(children: "OrderedDict[str, nn.Module]", returned) -> list:
    """The children as steps of the fused path: ("conv", conv name, norm name, ReLU name or None, cache, name the result carries),
    ("pool", name) or ("call", name).  A name in `returned` must be the last child of its step."""
    names, plan, i = list(children), [], 0
    while i < len(names):
        name, m = names[i], children[names[i]]
        if isinstance(m, nn.Conv2d):
            norm = children[names[i + 1]] if i + 1 < len(names) else None
            if not isinstance(norm, _NORMS):
                raise NotImplementedError(f"child {name!r}: a Conv2d runs fused with the BatchNorm2d / FrozenBatchNorm2d child that follows it; "
                                          f"found {type(norm).__name__}")
            relu = names[i + 2] if i + 2 < len(names) and isinstance(children[names[i + 2]], nn.ReLU) else None
            run = names[i:i + (3 if relu else 2)]
            if any(n in returned for n in run[:-1]):
                raise NotImplementedError(f"children {run} run as one launch: only {run[-1]!r} can be returned")
            plan.append(("conv", name, names[i + 1], relu, _FoldedNorm(), run[-1]))
            i += len(run)
            continue
        if isinstance(m, nn.MaxPool2d):
            if m.dilation != 1 or m.ceil_mode or m.return_indices:
                raise NotImplementedError(f"child {name!r}: {m}")
            plan.append(("pool", name))
        elif isinstance(m, nn.Sequential) and len(m) > 0 and all(isinstance(b, _BLOCKS) for b in m):
            plan.append(("call", name))
        elif isinstance(m, _BLOCKS):
            plan.append(("call", name))
        else:
            raise NotImplementedError(f"child {name!r} ({type(m).__name__}) has no fused path: IntermediateLayerGetter runs Conv2d + norm "
                                      "[+ ReLU], MaxPool2d and Sequentials of this package's blocks")
        i += 1
    return plan


class IntermediateLayerGetter(nn.ModuleDict):
    """models/_utils.py:13-75: the children of `model` up to the last one named in `return_layers` (child name -> output name);
    forward returns an OrderedDict of the named activations.  As in the reference the children must be used in registration
    order and only direct children can be returned."""

    _version = 2
    __annotations__ = {
        "return_layers": Dict[str, str],
    }

    def __init__(self, model: nn.Module, return_layers: Dict[str, str]) -> None:
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

        plan = _fused_plan(layers, {str(k) for k in orig_return_layers})
        super().__init__(layers)
        self.return_layers = orig_return_layers
        self._plan = plan
        self.eval()

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        if self.training:
            raise RuntimeError("the MI355X IntermediateLayerGetter is inference only: call .eval()")
        inp, out = x, OrderedDict()
        returned = {str(k): v for k, v in self.return_layers.items()}
        with torch.no_grad():  # no autograd bookkeeping per layer; the results are marked once (their backward raises)
            for step in self._plan:
                if step[0] == "conv":
                    _, conv, norm, relu, cache, name = step
                    x = resnet.fused_conv_norm(x, self[conv], self[norm], cache, relu=relu is not None)
                elif step[0] == "pool":
                    name = step[1]
                    mp = self[name]
                    x = F.max_pool2d(x, mp.kernel_size, mp.stride, mp.padding)
                else:
                    name = step[1]
                    x = self[name](x)
                if name in returned:
                    out[returned[name]] = x
        dep = next((p for p in self.parameters() if p.requires_grad), None)
        return OrderedDict((k, _lib.forward_only(v, "IntermediateLayerGetter.forward", inp, dep)) for k, v in out.items())


class BackboneWithFPN(nn.Module):
    """detection/backbone_utils.py:14-59: a FeaturePyramidNetwork on top of the returned layers of a backbone.  `.body` is the
    IntermediateLayerGetter, `.fpn` the pyramid (extra block LastLevelMaxPool unless one is given), `.out_channels` its width."""

    def __init__(self, backbone: nn.Module, return_layers: Dict[str, str], in_channels_list: List[int], out_channels: int,
                 extra_blocks: Optional[ExtraFPNBlock] = None, norm_layer: Optional[Callable[..., nn.Module]] = None) -> None:
        super().__init__()
        if extra_blocks is None:
            extra_blocks = LastLevelMaxPool()
        self.body = IntermediateLayerGetter(backbone, return_layers=return_layers)
        self.fpn = FeaturePyramidNetwork(in_channels_list=in_channels_list, out_channels=out_channels, extra_blocks=extra_blocks,
                                         norm_layer=norm_layer)
        self.out_channels = out_channels
        self.eval()

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        x = self.body(x)
        x = self.fpn(x)
        return x


def resnet_fpn_backbone(*, backbone_name: str, norm_layer: Callable[..., nn.Module] = FrozenBatchNorm2d, trainable_layers: int = 3,
                        returned_layers: Optional[List[int]] = None, extra_blocks: Optional[ExtraFPNBlock] = None) -> BackboneWithFPN:
    """detection/backbone_utils.py:62-114: a ResNet of this package (resnet18 ... wide_resnet101_2) with a FeaturePyramidNetwork
    of 256 channels on top of layer1..layer4 (or `returned_layers`, each in 1..4).

    There is no `weights` argument: the package ships no weight files.  Load a state dict of the reference's backbone
    (body.* / fpn.* keys) with load_state_dict.  `trainable_layers` (0..5) freezes the rest with requires_grad_(False) as the
    reference does, although the library is forward only: an output computed from a tensor that still requires grad raises in
    backward."""
    backbone = resnet.__dict__[backbone_name](norm_layer=norm_layer)
    return _resnet_fpn_extractor(backbone, trainable_layers, returned_layers, extra_blocks)


def _resnet_fpn_extractor(backbone: resnet.ResNet, trainable_layers: int, returned_layers: Optional[List[int]] = None,
                          extra_blocks: Optional[ExtraFPNBlock] = None,
                          norm_layer: Optional[Callable[..., nn.Module]] = None) -> BackboneWithFPN:
    # select layers that won't be frozen
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


def _validate_trainable_layers(is_trained: bool, trainable_backbone_layers: Optional[int], max_value: int, default_value: int) -> int:
    # don't freeze any layers if pretrained model or backbone is not used
    if not is_trained:
        if trainable_backbone_layers is not None:
            warnings.warn(
                "Changing trainable_backbone_layers has no effect if "
                "neither pretrained nor pretrained_backbone have been set to True, "
                f"falling back to trainable_backbone_layers={max_value} so that all layers are trainable"
            )
        trainable_backbone_layers = max_value

    # by default freeze first blocks
    if trainable_backbone_layers is None:
        trainable_backbone_layers = default_value
    if trainable_backbone_layers < 0 or trainable_backbone_layers > max_value:
        raise ValueError(
            f"Trainable backbone layers should be in the range [0,{max_value}], got {trainable_backbone_layers} "
        )
    return trainable_backbone_layers
