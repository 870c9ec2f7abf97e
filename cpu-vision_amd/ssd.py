"""SSD inference on the MI355X kernels: models/detection/ssd.py of the reference -- SSDScoringHead, SSDClassificationHead,
SSDRegressionHead, SSDHead, SSDFeatureExtractorVGG, SSD and the ssd300_vgg16 builder -- with the same classes, constructor arguments,
defaults, argument errors, child names (backbone.scale_weight / features.{i} / extra.0.{1,3,5} / extra.0.7.{1,3} / extra.{1..}.{0,2},
anchor_generator, head.classification_head.module_list.{i}, head.regression_head.module_list.{i}, transform), state-dict keys and
initialisation order.  Only `forward` differs.

The extractor walks its containers on the kernels: every Conv2d 3x3 + ReLU is one F.conv2d_bias_relu launch, the dilated fc6, the
stride-2, 1x1 and 4x4 convs go through F.conv2d_bias_act, the pools through F.max_pool2d (the third with ceil_mode=True: 75 -> 38),
and conv4_3's rescaling is one F.l2_normalize_scale launch.  The heads keep their per-level NCHW maps, as RetinaNet's do here: one
F.conv2d_bias_relu(relu=False) launch per (level, head).  F.ssd_scores takes the softmax of every anchor into a class-major matrix,
F.ssd_topk thresholds and selects per class on its rows, F.ssd_decode builds the default boxes of the selected candidates in
registers and decodes them -- three calls for the whole batch in place of the reference's loop over the labels; then per image the
boolean indexing by `valid`, ops.batched_nms and the slice.

Inference only, float32 only.  The training half of the reference (SSDMatcher, hard-negative mining, the losses, BoxCoder.encode) is
not built: `iou_thresh` is stored in place of the reference's `proposal_matcher`.  There are no weight files.
"""
from __future__ import annotations

import warnings
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import nn, Tensor

from . import _lib
from . import functional as F
from ._one_stage import OneStageDetector
from .anchor_utils import DefaultBoxGenerator
from .backbone_utils import _validate_trainable_layers
from .image_list import ImageList
from .nn import VGG
from .rpn import BoxCoder
from .transform import GeneralizedRCNNTransform

__all__ = ["SSD", "SSDHead", "SSDScoringHead", "SSDClassificationHead", "SSDRegressionHead", "SSDFeatureExtractorVGG", "ssd300_vgg16"]


def _xavier_init(conv: nn.Module):
    for layer in conv.modules():
        if isinstance(layer, nn.Conv2d):
            torch.nn.init.xavier_uniform_(layer.weight)
            if layer.bias is not None:
                torch.nn.init.constant_(layer.bias, 0.0)


class SSDHead(nn.Module):
    """ssd.py SSDHead.  forward(x: List[Tensor]) -> {"bbox_regression", "cls_logits"}: the per-level NCHW maps (N, 4 A, H, W) and
    (N, A K, H, W) the kernels read; permuted() of either head gives the reference's layout."""

    def __init__(self, in_channels: List[int], num_anchors: List[int], num_classes: int):
        super().__init__()
        self.classification_head = SSDClassificationHead(in_channels, num_anchors, num_classes)
        self.regression_head = SSDRegressionHead(in_channels, num_anchors)
        self.eval()

    def forward(self, x: List[Tensor]) -> Dict[str, List[Tensor]]:
        return {
            "bbox_regression": self.regression_head(x),
            "cls_logits": self.classification_head(x),
        }


class SSDScoringHead(nn.Module):
    """ssd.py SSDScoringHead: one Conv2d(ch, num_columns * A, 3, padding=1) per level.  forward(x: List[Tensor]) -> per level the NCHW
    map (N, A * num_columns, H, W): channel a * num_columns + c at (y, x) is column c of anchor (y W + x) A + a, which is what the
    reference's view(N, -1, num_columns, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, num_columns) yields; permuted() builds that."""

    def __init__(self, module_list: nn.ModuleList, num_columns: int):
        super().__init__()
        self.module_list = module_list
        self.num_columns = num_columns
        self.eval()

    def _get_result_from_module_list(self, x: Tensor, idx: int) -> Tensor:
        """module_list[idx](x) on the kernels: one launch."""
        num_blocks = len(self.module_list)
        if idx < 0:
            idx += num_blocks
        conv = self.module_list[idx]
        return F.conv2d_bias_relu(x, conv.weight, conv.bias, relu=False)

    def forward(self, x: List[Tensor]) -> List[Tensor]:
        if self.training:
            raise RuntimeError(f"the MI355X {type(self).__name__} is inference only: call .eval()")
        with torch.no_grad():
            out = [self._get_result_from_module_list(features, i) for i, features in enumerate(x)]
        return [_lib.forward_only(v, f"{type(self).__name__}.forward", *x, *self.parameters()) for v in out]

    def permuted(self, maps: List[Tensor]) -> Tensor:
        """The reference's forward output (N, sum HWA, num_columns) of this head's per-level maps, as torch compositions."""
        all_results = []
        for results in maps:
            # Permute output from (N, A * K, H, W) to (N, HWA, K).
            N, _, H, W = results.shape
            results = results.contiguous().view(N, -1, self.num_columns, H, W)
            results = results.permute(0, 3, 4, 1, 2)
            results = results.reshape(N, -1, self.num_columns)  # Size=(N, HWA, K)
            all_results.append(results)
        return torch.cat(all_results, dim=1)


class SSDClassificationHead(SSDScoringHead):
    def __init__(self, in_channels: List[int], num_anchors: List[int], num_classes: int):
        cls_logits = nn.ModuleList()
        for channels, anchors in zip(in_channels, num_anchors):
            cls_logits.append(nn.Conv2d(channels, num_classes * anchors, kernel_size=3, padding=1))
        _xavier_init(cls_logits)
        super().__init__(cls_logits, num_classes)


class SSDRegressionHead(SSDScoringHead):
    def __init__(self, in_channels: List[int], num_anchors: List[int]):
        bbox_reg = nn.ModuleList()
        for channels, anchors in zip(in_channels, num_anchors):
            bbox_reg.append(nn.Conv2d(channels, 4 * anchors, kernel_size=3, padding=1))
        _xavier_init(bbox_reg)
        super().__init__(bbox_reg, 4)


def _single(v) -> int:
    return int(v if isinstance(v, int) else v[0])


def _walk(mods, x: Tensor) -> Tensor:
    """A reference-style run of Conv2d / ReLU / MaxPool2d modules and nn.Sequentials of them on the kernels: every conv with the
    ReLU behind it is one launch, every pool one launch (its own ceil_mode honoured)."""
    mods = list(mods)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Sequential):
            x = _walk(m, x)
            i += 1
        elif isinstance(m, nn.Conv2d):
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            if m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.dilation == (1, 1) and m.groups == 1:
                x = F.conv2d_bias_relu(x, m.weight, m.bias, relu=relu)
            else:
                x = F.conv2d_bias_act(x, m.weight, m.bias, stride=m.stride, padding=m.padding, dilation=m.dilation, groups=m.groups,
                                      activation="relu" if relu else None)
            i += 2 if relu else 1
        elif isinstance(m, nn.MaxPool2d):
            if _single(m.dilation) != 1:
                raise NotImplementedError("a dilated MaxPool2d is not on the MI355X path")
            x = F.max_pool2d(x, _single(m.kernel_size), _single(m.stride), _single(m.padding), ceil_mode=bool(m.ceil_mode))
            i += 1
        else:
            raise NotImplementedError(f"{type(m).__name__} is not on the MI355X SSD path")
    return x


class SSDFeatureExtractorVGG(nn.Module):
    """ssd.py SSDFeatureExtractorVGG.  forward(x) -> OrderedDict "0", "1", ...: conv4_3 rescaled (F.l2_normalize_scale), fc7, then the
    extra blocks' outputs."""

    def __init__(self, backbone: nn.Module, highres: bool):
        super().__init__()

        _, _, maxpool3_pos, maxpool4_pos, _ = (i for i, layer in enumerate(backbone) if isinstance(layer, nn.MaxPool2d))

        # Patch ceil_mode for maxpool3 to get the same WxH output sizes as the paper
        backbone[maxpool3_pos].ceil_mode = True

        # parameters used for L2 regularization + rescaling
        self.scale_weight = nn.Parameter(torch.ones(512) * 20)

        # Multiple Feature maps - page 4, Fig 2 of SSD paper
        self.features = nn.Sequential(*backbone[:maxpool4_pos])  # until conv4_3

        # SSD300 case - page 4, Fig 2 of SSD paper
        extra = nn.ModuleList(
            [
                nn.Sequential(
                    nn.Conv2d(1024, 256, kernel_size=1),
                    nn.ReLU(inplace=True),
                    nn.Conv2d(256, 512, kernel_size=3, padding=1, stride=2),  # conv8_2
                    nn.ReLU(inplace=True),
                ),
                nn.Sequential(
                    nn.Conv2d(512, 128, kernel_size=1),
                    nn.ReLU(inplace=True),
                    nn.Conv2d(128, 256, kernel_size=3, padding=1, stride=2),  # conv9_2
                    nn.ReLU(inplace=True),
                ),
                nn.Sequential(
                    nn.Conv2d(256, 128, kernel_size=1),
                    nn.ReLU(inplace=True),
                    nn.Conv2d(128, 256, kernel_size=3),  # conv10_2
                    nn.ReLU(inplace=True),
                ),
                nn.Sequential(
                    nn.Conv2d(256, 128, kernel_size=1),
                    nn.ReLU(inplace=True),
                    nn.Conv2d(128, 256, kernel_size=3),  # conv11_2
                    nn.ReLU(inplace=True),
                ),
            ]
        )
        if highres:
            # Additional layers for the SSD512 case. See page 11, footernote 5.
            extra.append(
                nn.Sequential(
                    nn.Conv2d(256, 128, kernel_size=1),
                    nn.ReLU(inplace=True),
                    nn.Conv2d(128, 256, kernel_size=4),  # conv12_2
                    nn.ReLU(inplace=True),
                )
            )
        _xavier_init(extra)

        fc = nn.Sequential(
            nn.MaxPool2d(kernel_size=3, stride=1, padding=1, ceil_mode=False),  # add modified maxpool5
            nn.Conv2d(in_channels=512, out_channels=1024, kernel_size=3, padding=6, dilation=6),  # FC6 with atrous
            nn.ReLU(inplace=True),
            nn.Conv2d(in_channels=1024, out_channels=1024, kernel_size=1),  # FC7
            nn.ReLU(inplace=True),
        )
        _xavier_init(fc)
        extra.insert(
            0,
            nn.Sequential(
                *backbone[maxpool4_pos:-1],  # until conv5_3, skip maxpool5
                fc,
            ),
        )
        self.extra = extra
        self.eval()

    def forward(self, x: Tensor) -> Dict[str, Tensor]:
        if self.training:
            raise RuntimeError("the MI355X SSDFeatureExtractorVGG is inference only: call .eval()")
        inp = x
        with torch.no_grad():
            # L2 regularization + Rescaling of 1st block's feature map
            x = _walk(self.features, x)
            rescaled = F.l2_normalize_scale(x, self.scale_weight)
            output = [rescaled]

            # Calculating Feature maps for the rest blocks
            for block in self.extra:
                x = _walk(block, x)
                output.append(x)
        deps = (inp, *self.parameters())
        return OrderedDict([(str(i), _lib.forward_only(v, "SSDFeatureExtractorVGG.forward", *deps)) for i, v in enumerate(output)])


def _vgg_extractor(backbone: VGG, highres: bool, trainable_layers: int):
    backbone = backbone.features
    # Gather the indices of maxpools. These are the locations of output blocks.
    stage_indices = [0] + [i for i, b in enumerate(backbone) if isinstance(b, nn.MaxPool2d)][:-1]
    num_stages = len(stage_indices)

    # find the index of the layer from which we won't freeze
    torch._assert(
        0 <= trainable_layers <= num_stages,
        f"trainable_layers should be in the range [0, {num_stages}]. Instead got {trainable_layers}",
    )
    freeze_before = len(backbone) if trainable_layers == 0 else stage_indices[num_stages - trainable_layers]

    for b in backbone[:freeze_before]:
        for parameter in b.parameters():
            parameter.requires_grad_(False)

    return SSDFeatureExtractorVGG(backbone, highres)


def _retrieve_out_channels(model: nn.Module, size: Tuple[int, int]) -> List[int]:
    """_utils.py retrieve_out_channels.  This package's SSDFeatureExtractorVGG is read off its modules (512 for conv4_3, then the last
    conv of every `extra` block): its forward needs the MI355X.  Any other backbone gets the reference's probing forward on zeros, on
    the backbone's own device.  An extractor of this package that states its channels itself (`_module_out_channels`: SSDlite's) is
    asked."""
    if hasattr(model, "_module_out_channels"):
        return model._module_out_channels()
    if isinstance(model, SSDFeatureExtractorVGG):
        out_channels = [int(model.scale_weight.numel())]
        for block in model.extra:
            out_channels.append([m for m in block.modules() if isinstance(m, nn.Conv2d)][-1].out_channels)
        return out_channels

    in_training = model.training
    model.eval()

    with torch.no_grad():
        # Use dummy data to retrieve the feature map sizes to avoid hard-coding their values
        device = next(model.parameters()).device
        tmp_img = torch.zeros((1, 3, size[1], size[0]), device=device)
        features = model(tmp_img)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        out_channels = [x.size(1) for x in features.values()]

    if in_training:
        model.train()

    return out_channels


class SSD(OneStageDetector):
    """ssd.py SSD.  forward(images: List[Tensor (C, H, W) float32 in 0..1]) -> List[{boxes (N, 4) as (x1, y1, x2, y2), scores (N,),
    labels (N,) int64}], the boxes in the coordinates of the images as given.  `**kwargs` go to GeneralizedRCNNTransform.  iou_thresh
    and positive_fraction are the training half's and only kept (iou_thresh, neg_to_pos_ratio)."""

    __annotations__ = {
        "box_coder": BoxCoder,
    }
    _name = "SSD"

    def __init__(self, backbone: nn.Module, anchor_generator: DefaultBoxGenerator, size: Tuple[int, int], num_classes: int,
                 image_mean: Optional[List[float]] = None, image_std: Optional[List[float]] = None, head: Optional[nn.Module] = None,
                 score_thresh: float = 0.01, nms_thresh: float = 0.45, detections_per_img: int = 200, iou_thresh: float = 0.5,
                 topk_candidates: int = 400, positive_fraction: float = 0.25, **kwargs: Any):
        super().__init__()

        self.backbone = backbone

        self.anchor_generator = anchor_generator

        self.box_coder = BoxCoder(weights=(10.0, 10.0, 5.0, 5.0))

        if topk_candidates > F.MAX_RPN_TOPK:
            raise ValueError(f"the MI355X SSD selects up to {F.MAX_RPN_TOPK} candidates per class, got topk_candidates={topk_candidates}")

        if head is None:
            if hasattr(backbone, "out_channels"):
                out_channels = backbone.out_channels
            else:
                out_channels = _retrieve_out_channels(backbone, size)

            if len(out_channels) != len(anchor_generator.aspect_ratios):
                raise ValueError(
                    f"The length of the output channels from the backbone ({len(out_channels)}) do not match the length of the anchor generator aspect ratios ({len(anchor_generator.aspect_ratios)})"
                )

            num_anchors = self.anchor_generator.num_anchors_per_location()
            head = SSDHead(out_channels, num_anchors, num_classes)
        self.head = head

        self.iou_thresh = iou_thresh  # the reference's proposal_matcher = SSDMatcher(iou_thresh) is training only

        if image_mean is None:
            image_mean = [0.485, 0.456, 0.406]
        if image_std is None:
            image_std = [0.229, 0.224, 0.225]
        self.transform = GeneralizedRCNNTransform(
            min(size), max(size), image_mean, image_std, size_divisible=1, fixed_size=size, **kwargs
        )

        self.score_thresh = score_thresh
        self.nms_thresh = nms_thresh
        self.detections_per_img = detections_per_img
        self.topk_candidates = topk_candidates
        self.neg_to_pos_ratio = (1.0 - positive_fraction) / positive_fraction

        # used only on torchscript mode
        self._has_warned = False
        self.eval()

    def candidates(self, head_outputs: Dict[str, List[Tensor]], features: List[Tensor],
                   images: ImageList) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
        """postprocess_detections up to the nms for the whole batch, three calls: (idx, boxes, scores, labels, valid), one row of
        (K - 1) * topk_candidates candidates per image, class after class."""
        cls, reg = head_outputs["cls_logits"], head_outputs["bbox_regression"]
        gen = self.anchor_generator
        torch._assert(len(gen._wh_pairs) == len(cls) == len(features), "the anchor generator and the head should have one entry per feature map")
        anchors = gen.num_anchors_per_location()
        num_classes = int(cls[0].shape[1]) // anchors[0]
        scores = F.ssd_scores(cls, num_classes)
        idx = F.ssd_topk(scores, self.topk_candidates, self.score_thresh)
        boxes, cand_scores, labels, valid = F.ssd_decode(scores, reg, idx, gen._wh_pairs, gen.steps, tuple(images.tensors.shape[-2:]),
                                                         images.image_sizes, self.box_coder.weights, gen.clip, self.box_coder.bbox_xform_clip)
        return idx, boxes, cand_scores, labels, valid

    def postprocess_detections(self, head_outputs: Dict[str, List[Tensor]], features: List[Tensor],
                               images: ImageList) -> List[Dict[str, Tensor]]:
        """ssd.py postprocess_detections on the head's per-level NCHW maps: `candidates`, then per image the boolean indexing by
        `valid`, ops.batched_nms over the labels and the slice."""
        return self._nms_tail(*self.candidates(head_outputs, features, images)[1:])

    def _detect(self, head_outputs, features, images):
        return self.postprocess_detections(head_outputs, features, images)


def ssd300_vgg16(*, weights: Optional[Any] = None, progress: bool = True, num_classes: Optional[int] = None,
                 weights_backbone: Optional[Any] = None, trainable_backbone_layers: Optional[int] = None, **kwargs: Any) -> SSD:
    """ssd.py ssd300_vgg16: SSD300 on VGG16's features (the whole VGG16 is constructed first, as the reference does, so a seeded
    construction draws from the RNG in the reference's order), 91 classes unless `num_classes` says otherwise.

    The package ships no weight files: `weights` and `weights_backbone` must be None; load a state dict of the reference's model
    with load_state_dict (the keys are the reference's)."""
    if weights is not None or weights_backbone is not None:
        raise ValueError("ssd300_vgg16: the package ships no weight files, weights and weights_backbone must be None; "
                         "load a state dict with load_state_dict")

    if "size" in kwargs:
        warnings.warn("The size of the model is already fixed; ignoring the parameter.")
        kwargs.pop("size")

    if num_classes is None:
        num_classes = 91

    trainable_backbone_layers = _validate_trainable_layers(False, trainable_backbone_layers, 5, 4)

    # Use custom backbones more appropriate for SSD
    backbone = VGG("D")
    backbone = _vgg_extractor(backbone, False, trainable_backbone_layers)
    anchor_generator = DefaultBoxGenerator(
        [[2], [2, 3], [2, 3], [2, 3], [2], [2]],
        scales=[0.07, 0.15, 0.33, 0.51, 0.69, 0.87, 1.05],
        steps=[8, 16, 32, 64, 100, 300],
    )

    defaults = {
        # Rescale the input in a way compatible to the backbone
        "image_mean": [0.48235, 0.45882, 0.40784],
        "image_std": [1.0 / 255.0, 1.0 / 255.0, 1.0 / 255.0],  # undo the 0-1 scaling of toTensor
    }
    kwargs: Any = {**defaults, **kwargs}
    model = SSD(backbone, anchor_generator, (300, 300), num_classes, **kwargs)
    return model
