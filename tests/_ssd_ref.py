"""References for the SSD tests (a helper module, not a test file and not a conftest).  Imports nothing from the package.

(a) A plain-torch replica of the reference's models/detection/ssd.py, anchor_utils.py::DefaultBoxGenerator and models/vgg.py
    (torchvision is not importable in the test environment), like tests/_fcos_ref.py: the same constructor arguments, child names,
    construction order and initialisation, torch's own convs and pools, torch.softmax, torch.exp and torch.topk, and the
    reference's Python loop over the labels.  BoxCoder, clip_boxes_to_image, batched_nms, ImageList and `same` are those of
    tests/_rpn_ref.py, the transform that of tests/_roi_heads_ref.py.
(b) The restatement the library is compared with bit for bit:
      l2_normalize_scale -> `l2_normalize_scale`: mv_l2_normalize_scale_f32's stated order of the float64 sum of squares (16 channel
                            groups c = g, g + 16, ..., each an ascending chain, then the groups in ascending order), the float32
                            square root of it, clamp_min and the division and multiplication, one rounding each
      softmax            -> `softmax_f64sum` / `scores`: max, the correctly rounded float32 exp, one ascending FLOAT64 chain over the
                            classes, the float64 division rounded to float32, for every anchor, class-major (N, K, V)
      default boxes      -> `default_boxes`: DefaultBoxGenerator's float32 chain in numpy
      `> thresh`, topk   -> `select`: the strict float32 comparison and the first k of the stable descending sort per class
      decode             -> `decode`: BoxCoder.decode_single with the correctly rounded exp on the restated default boxes, the clamp
"""
import math
import warnings
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from tests import _roi_heads_ref as RH
from tests import _rpn_ref as P
from tests._roi_heads_ref import GeneralizedRCNNTransform
from tests._rpn_ref import ImageList, batched_nms, clip_boxes_to_image, same, ulp_distance  # noqa: F401

REPLICA, RESTATEMENT = RH.REPLICA, RH.RESTATEMENT
L2_GROUPS = 16  # the channel groups of mv_l2_normalize_scale_f32's sum


# ------------------------------------------------------------------------------------------------ (b) the L2 norm
def l2_normalize_scale(x, weight, eps=1e-12):
    """mv_l2_normalize_scale_f32 restated: x (N, C, H, W) float32 tensor, weight (C,) -> tensor."""
    xs = x.detach().contiguous().numpy()
    n, c, h, w = xs.shape
    with np.errstate(all="ignore"):
        d = xs.astype(np.float64)
        sq = d * d
        total = np.zeros((n, h, w))
        for g in range(L2_GROUPS):
            s = np.zeros((n, h, w))
            for ch in range(g, c, L2_GROUPS):
                s = s + sq[:, ch]
            total = total + s
        nrm = np.sqrt(total).astype(np.float32)
        eps32 = np.float32(eps)
        div = np.where(nrm < eps32, eps32, nrm)  # clamp_min: a NaN stays
        q = xs / div[:, None]
        assert q.dtype == np.float32
        y = weight.detach().numpy().astype(np.float32)[None, :, None, None] * q
    assert y.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(y))


# ------------------------------------------------------------------------------------------------ (a) the torch replica
class DefaultBoxGenerator(nn.Module):
    def __init__(self, aspect_ratios, min_ratio=0.15, max_ratio=0.9, scales=None, steps=None, clip=True):
        super().__init__()
        if steps is not None and len(aspect_ratios) != len(steps):
            raise ValueError("aspect_ratios and steps should have the same length")
        self.aspect_ratios = aspect_ratios
        self.steps = steps
        self.clip = clip
        num_outputs = len(aspect_ratios)
        if scales is None:
            if num_outputs > 1:
                range_ratio = max_ratio - min_ratio
                self.scales = [min_ratio + range_ratio * k / (num_outputs - 1.0) for k in range(num_outputs)]
                self.scales.append(1.0)
            else:
                self.scales = [min_ratio, max_ratio]
        else:
            self.scales = scales
        self._wh_pairs = self._generate_wh_pairs(num_outputs)

    def _generate_wh_pairs(self, num_outputs, dtype=torch.float32, device=torch.device("cpu")):
        _wh_pairs = []
        for k in range(num_outputs):
            s_k = self.scales[k]
            s_prime_k = math.sqrt(self.scales[k] * self.scales[k + 1])
            wh_pairs = [[s_k, s_k], [s_prime_k, s_prime_k]]
            for ar in self.aspect_ratios[k]:
                sq_ar = math.sqrt(ar)
                w = self.scales[k] * sq_ar
                h = self.scales[k] / sq_ar
                wh_pairs.extend([[w, h], [h, w]])
            _wh_pairs.append(torch.as_tensor(wh_pairs, dtype=dtype, device=device))
        return _wh_pairs

    def num_anchors_per_location(self):
        return [2 + 2 * len(r) for r in self.aspect_ratios]

    def _grid_default_boxes(self, grid_sizes, image_size, dtype=torch.float32):
        default_boxes = []
        for k, f_k in enumerate(grid_sizes):
            if self.steps is not None:
                x_f_k = image_size[1] / self.steps[k]
                y_f_k = image_size[0] / self.steps[k]
            else:
                y_f_k, x_f_k = f_k
            shifts_x = ((torch.arange(0, f_k[1]) + 0.5) / x_f_k).to(dtype=dtype)
            shifts_y = ((torch.arange(0, f_k[0]) + 0.5) / y_f_k).to(dtype=dtype)
            shift_y, shift_x = torch.meshgrid(shifts_y, shifts_x, indexing="ij")
            shift_x = shift_x.reshape(-1)
            shift_y = shift_y.reshape(-1)
            shifts = torch.stack((shift_x, shift_y) * len(self._wh_pairs[k]), dim=-1).reshape(-1, 2)
            _wh_pair = self._wh_pairs[k].clamp(min=0, max=1) if self.clip else self._wh_pairs[k]
            wh_pairs = _wh_pair.repeat((f_k[0] * f_k[1]), 1)
            default_box = torch.cat((shifts, wh_pairs), dim=1)
            default_boxes.append(default_box)
        return torch.cat(default_boxes, dim=0)

    def forward(self, image_list, feature_maps):
        grid_sizes = [feature_map.shape[-2:] for feature_map in feature_maps]
        image_size = image_list.tensors.shape[-2:]
        dtype, device = feature_maps[0].dtype, feature_maps[0].device
        default_boxes = self._grid_default_boxes(grid_sizes, image_size, dtype=dtype)
        default_boxes = default_boxes.to(device)
        dboxes = []
        x_y_size = torch.tensor([image_size[1], image_size[0]], device=default_boxes.device)
        for _ in image_list.image_sizes:
            dboxes_in_image = default_boxes
            dboxes_in_image = torch.cat(
                [
                    (dboxes_in_image[:, :2] - 0.5 * dboxes_in_image[:, 2:]) * x_y_size,
                    (dboxes_in_image[:, :2] + 0.5 * dboxes_in_image[:, 2:]) * x_y_size,
                ],
                -1,
            )
            dboxes.append(dboxes_in_image)
        return dboxes


def _xavier_init(conv):
    for layer in conv.modules():
        if isinstance(layer, nn.Conv2d):
            torch.nn.init.xavier_uniform_(layer.weight)
            if layer.bias is not None:
                torch.nn.init.constant_(layer.bias, 0.0)


class SSDScoringHead(nn.Module):
    def __init__(self, module_list, num_columns):
        super().__init__()
        self.module_list = module_list
        self.num_columns = num_columns

    def _get_result_from_module_list(self, x, idx):
        num_blocks = len(self.module_list)
        if idx < 0:
            idx += num_blocks
        out = x
        for i, module in enumerate(self.module_list):
            if i == idx:
                out = module(x)
        return out

    def maps(self, x):
        return [self._get_result_from_module_list(features, i) for i, features in enumerate(x)]

    def forward(self, x):
        all_results = []
        for i, features in enumerate(x):
            results = self._get_result_from_module_list(features, i)
            N, _, H, W = results.shape
            results = results.view(N, -1, self.num_columns, H, W)
            results = results.permute(0, 3, 4, 1, 2)
            results = results.reshape(N, -1, self.num_columns)
            all_results.append(results)
        return torch.cat(all_results, dim=1)


class SSDClassificationHead(SSDScoringHead):
    def __init__(self, in_channels, num_anchors, num_classes):
        cls_logits = nn.ModuleList()
        for channels, anchors in zip(in_channels, num_anchors):
            cls_logits.append(nn.Conv2d(channels, num_classes * anchors, kernel_size=3, padding=1))
        _xavier_init(cls_logits)
        super().__init__(cls_logits, num_classes)


class SSDRegressionHead(SSDScoringHead):
    def __init__(self, in_channels, num_anchors):
        bbox_reg = nn.ModuleList()
        for channels, anchors in zip(in_channels, num_anchors):
            bbox_reg.append(nn.Conv2d(channels, 4 * anchors, kernel_size=3, padding=1))
        _xavier_init(bbox_reg)
        super().__init__(bbox_reg, 4)


class SSDHead(nn.Module):
    def __init__(self, in_channels, num_anchors, num_classes):
        super().__init__()
        self.classification_head = SSDClassificationHead(in_channels, num_anchors, num_classes)
        self.regression_head = SSDRegressionHead(in_channels, num_anchors)

    def forward(self, x):
        return {"bbox_regression": self.regression_head(x), "cls_logits": self.classification_head(x)}


VGG16_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]


class VGG(nn.Module):
    """models/vgg.py VGG with make_layers(cfg, batch_norm=False): the whole model, as ssd300_vgg16 constructs it before it keeps the
    features (the classifier's draws are part of the seeded sequence)."""

    def __init__(self, cfg=VGG16_CFG, num_classes=1000, init_weights=True, dropout=0.5):
        super().__init__()
        layers, in_channels = [], 3
        for v in cfg:
            if v == "M":
                layers += [nn.MaxPool2d(kernel_size=2, stride=2)]
            else:
                layers += [nn.Conv2d(in_channels, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                in_channels = v
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d((7, 7))
        self.classifier = nn.Sequential(
            nn.Linear(512 * 7 * 7, 4096), nn.ReLU(True), nn.Dropout(p=dropout),
            nn.Linear(4096, 4096), nn.ReLU(True), nn.Dropout(p=dropout),
            nn.Linear(4096, num_classes),
        )
        if init_weights:
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
                elif isinstance(m, nn.Linear):
                    nn.init.normal_(m.weight, 0, 0.01)
                    nn.init.constant_(m.bias, 0)


class SSDFeatureExtractorVGG(nn.Module):
    def __init__(self, backbone, highres):
        super().__init__()
        _, _, maxpool3_pos, maxpool4_pos, _ = (i for i, layer in enumerate(backbone) if isinstance(layer, nn.MaxPool2d))
        backbone[maxpool3_pos].ceil_mode = True
        self.scale_weight = nn.Parameter(torch.ones(512) * 20)
        self.features = nn.Sequential(*backbone[:maxpool4_pos])
        extra = nn.ModuleList(
            [
                nn.Sequential(nn.Conv2d(1024, 256, kernel_size=1), nn.ReLU(inplace=True),
                              nn.Conv2d(256, 512, kernel_size=3, padding=1, stride=2), nn.ReLU(inplace=True)),
                nn.Sequential(nn.Conv2d(512, 128, kernel_size=1), nn.ReLU(inplace=True),
                              nn.Conv2d(128, 256, kernel_size=3, padding=1, stride=2), nn.ReLU(inplace=True)),
                nn.Sequential(nn.Conv2d(256, 128, kernel_size=1), nn.ReLU(inplace=True),
                              nn.Conv2d(128, 256, kernel_size=3), nn.ReLU(inplace=True)),
                nn.Sequential(nn.Conv2d(256, 128, kernel_size=1), nn.ReLU(inplace=True),
                              nn.Conv2d(128, 256, kernel_size=3), nn.ReLU(inplace=True)),
            ]
        )
        if highres:
            extra.append(nn.Sequential(nn.Conv2d(256, 128, kernel_size=1), nn.ReLU(inplace=True),
                                       nn.Conv2d(128, 256, kernel_size=4), nn.ReLU(inplace=True)))
        _xavier_init(extra)
        fc = nn.Sequential(
            nn.MaxPool2d(kernel_size=3, stride=1, padding=1, ceil_mode=False),
            nn.Conv2d(in_channels=512, out_channels=1024, kernel_size=3, padding=6, dilation=6),
            nn.ReLU(inplace=True),
            nn.Conv2d(in_channels=1024, out_channels=1024, kernel_size=1),
            nn.ReLU(inplace=True),
        )
        _xavier_init(fc)
        extra.insert(0, nn.Sequential(*backbone[maxpool4_pos:-1], fc))
        self.extra = extra

    def forward(self, x):
        x = self.features(x)
        rescaled = self.scale_weight.view(1, -1, 1, 1) * nn.functional.normalize(x)
        output = [rescaled]
        for block in self.extra:
            x = block(x)
            output.append(x)
        return OrderedDict([(str(i), v) for i, v in enumerate(output)])


def _vgg_extractor(backbone, highres, trainable_layers):
    backbone = backbone.features
    stage_indices = [0] + [i for i, b in enumerate(backbone) if isinstance(b, nn.MaxPool2d)][:-1]
    num_stages = len(stage_indices)
    torch._assert(0 <= trainable_layers <= num_stages,
                  f"trainable_layers should be in the range [0, {num_stages}]. Instead got {trainable_layers}")
    freeze_before = len(backbone) if trainable_layers == 0 else stage_indices[num_stages - trainable_layers]
    for b in backbone[:freeze_before]:
        for parameter in b.parameters():
            parameter.requires_grad_(False)
    return SSDFeatureExtractorVGG(backbone, highres)


def retrieve_out_channels(model, size):
    in_training = model.training
    model.eval()
    with torch.no_grad():
        device = next(model.parameters()).device
        tmp_img = torch.zeros((1, 3, size[1], size[0]), device=device)
        features = model(tmp_img)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        out_channels = [x.size(1) for x in features.values()]
    if in_training:
        model.train()
    return out_channels


def _topk_min(input, orig_kval, axis):
    return min(orig_kval, input.size(axis))


class SSD(nn.Module):
    """ssd.py SSD, the inference path.  out_channels: what the reference finds with a forward on zeros (retrieve_out_channels), given
    by the caller where that forward is too slow for a test (VGG16 at 300 x 300 on the CPU).  `numerics` picks (a) or (b)."""

    def __init__(self, backbone, anchor_generator, size, num_classes, image_mean=None, image_std=None, head=None, score_thresh=0.01,
                 nms_thresh=0.45, detections_per_img=200, iou_thresh=0.5, topk_candidates=400, positive_fraction=0.25, out_channels=None,
                 numerics=REPLICA, **kwargs):
        super().__init__()
        self.backbone = backbone
        self.anchor_generator = anchor_generator
        self.numerics = numerics
        self.box_coder = P.BoxCoder(weights=(10.0, 10.0, 5.0, 5.0), numerics=numerics.rpn)
        if head is None:
            if hasattr(backbone, "out_channels"):
                out_channels = backbone.out_channels
            elif out_channels is None:
                out_channels = retrieve_out_channels(backbone, size)
            if len(out_channels) != len(anchor_generator.aspect_ratios):
                raise ValueError(
                    f"The length of the output channels from the backbone ({len(out_channels)}) do not match the length of the anchor generator aspect ratios ({len(anchor_generator.aspect_ratios)})"
                )
            num_anchors = self.anchor_generator.num_anchors_per_location()
            head = SSDHead(out_channels, num_anchors, num_classes)
        self.head = head
        self.iou_thresh = iou_thresh
        if image_mean is None:
            image_mean = [0.485, 0.456, 0.406]
        if image_std is None:
            image_std = [0.229, 0.224, 0.225]
        self.transform = GeneralizedRCNNTransform(min(size), max(size), image_mean, image_std, size_divisible=1, fixed_size=size, **kwargs)
        self.score_thresh = score_thresh
        self.nms_thresh = nms_thresh
        self.detections_per_img = detections_per_img
        self.topk_candidates = topk_candidates
        self.neg_to_pos_ratio = (1.0 - positive_fraction) / positive_fraction

    def candidates(self, head_outputs, image_anchors, image_shapes):
        """postprocess_detections up to the nms: per image (boxes, scores, labels, anchors) -- `anchors` the anchor index of every
        candidate, which the reference does not keep."""
        bbox_regression = head_outputs["bbox_regression"]
        logits = head_outputs["cls_logits"]
        pred_scores = self.numerics.softmax(logits.reshape(-1, logits.shape[-1])).reshape(logits.shape)
        num_classes = pred_scores.size(-1)
        device = pred_scores.device
        out = []
        for boxes, scores, anchors, image_shape in zip(bbox_regression, pred_scores, image_anchors, image_shapes):
            boxes = self.box_coder.decode_single(boxes, anchors)
            boxes = clip_boxes_to_image(boxes, image_shape)
            image_boxes, image_scores, image_labels, image_anchor_idx = [], [], [], []
            for label in range(1, num_classes):
                score = scores[:, label]
                keep_idxs = score > self.score_thresh
                score = score[keep_idxs]
                box = boxes[keep_idxs]
                # keep only topk scoring predictions
                num_topk = _topk_min(score, self.topk_candidates, 0)
                idxs = self.numerics.rpn.topk(score[None], num_topk)[0]
                score = score[idxs]
                box = box[idxs]
                image_boxes.append(box)
                image_scores.append(score)
                image_labels.append(torch.full_like(score, fill_value=label, dtype=torch.int64, device=device))
                image_anchor_idx.append(torch.where(keep_idxs)[0][idxs])
            out.append((torch.cat(image_boxes, dim=0), torch.cat(image_scores, dim=0), torch.cat(image_labels, dim=0),
                        torch.cat(image_anchor_idx, dim=0)))
        return out

    def postprocess_detections(self, head_outputs, image_anchors, image_shapes):
        detections = []
        for image_boxes, image_scores, image_labels, _ in self.candidates(head_outputs, image_anchors, image_shapes):
            keep = batched_nms(image_boxes, image_scores, image_labels, self.nms_thresh)
            keep = keep[: self.detections_per_img]
            detections.append({"boxes": image_boxes[keep], "scores": image_scores[keep], "labels": image_labels[keep]})
        return detections

    def forward(self, images, targets=None):
        original_image_sizes = []
        for img in images:
            val = img.shape[-2:]
            original_image_sizes.append((val[0], val[1]))
        images, targets = self.transform(images, targets)
        features = self.backbone(images.tensors)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        features = list(features.values())
        head_outputs = self.head(features)
        anchors = self.anchor_generator(images, features)
        detections = self.postprocess_detections(head_outputs, anchors, images.image_sizes)
        return self.transform.postprocess(detections, images.image_sizes, original_image_sizes)


SSD300_OUT_CHANNELS = [512, 1024, 512, 256, 256, 256]  # what retrieve_out_channels finds for SSDFeatureExtractorVGG(highres=False)


def ssd300_generator(clip=True):
    return DefaultBoxGenerator([[2], [2, 3], [2, 3], [2, 3], [2], [2]], scales=[0.07, 0.15, 0.33, 0.51, 0.69, 0.87, 1.05],
                               steps=[8, 16, 32, 64, 100, 300], clip=clip)


def ssd300_vgg16(*, weights=None, progress=True, num_classes=None, weights_backbone=None, trainable_backbone_layers=None, **kwargs):
    if "size" in kwargs:
        warnings.warn("The size of the model is already fixed; ignoring the parameter.")
        kwargs.pop("size")
    if num_classes is None:
        num_classes = 91
    trainable_backbone_layers = 5  # _validate_trainable_layers without weights
    backbone = VGG()
    backbone = _vgg_extractor(backbone, False, trainable_backbone_layers)
    anchor_generator = ssd300_generator()
    defaults = {"image_mean": [0.48235, 0.45882, 0.40784], "image_std": [1.0 / 255.0, 1.0 / 255.0, 1.0 / 255.0]}
    kwargs = {**defaults, **kwargs}
    return SSD(backbone, anchor_generator, (300, 300), num_classes, out_channels=SSD300_OUT_CHANNELS, **kwargs)


# ------------------------------------------------------------------------------------------------ (b) the post-processing
def permute_level(m, last):
    N, _, H, W = m.shape
    return m.contiguous().view(N, -1, last, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, last)


def softmax_f64sum(x):
    """mv_ssd_scores_f32's softmax of the rows of x (R, K): max, E in float32, ONE ascending float64 chain, the float64 division."""
    m = x.max(dim=1, keepdim=True)[0]
    e = P.exp_cr(x - m)
    s = torch.zeros(x.shape[0], dtype=torch.float64)
    for j in range(x.shape[1]):
        s = s + e[:, j].double()
    return (e.double() / s[:, None]).float()


def scores(cls_maps, num_classes, softmax=softmax_f64sum):
    """mv_ssd_scores_f32 restated: per-level maps (N, A K, H, W) -> (N, K, V) class-major."""
    logits = torch.cat([permute_level(m, num_classes) for m in cls_maps], dim=1)  # (N, V, K)
    n, v, k = logits.shape
    with np.errstate(all="ignore"):
        p = softmax(logits.reshape(-1, k)).reshape(n, v, k)
    return p.permute(0, 2, 1).contiguous()


def default_boxes(gen, grid_sizes, image_size):
    """DefaultBoxGenerator's float32 chain in numpy: (V, 4) float32 tensor for the grids [(H_l, W_l)] and the batch's (H, W)."""
    f32 = np.float32
    h_img, w_img = int(image_size[0]), int(image_size[1])
    out = []
    for l, (gh, gw) in enumerate(grid_sizes):
        x_f = f32(w_img / gen.steps[l]) if gen.steps is not None else f32(gw)
        y_f = f32(h_img / gen.steps[l]) if gen.steps is not None else f32(gh)
        pairs = gen._wh_pairs[l].numpy().astype(f32)
        if gen.clip:
            pairs = np.clip(pairs, f32(0), f32(1))
        a = pairs.shape[0]
        cx = (np.arange(gw).astype(f32) + f32(0.5)) / x_f
        cy = (np.arange(gh).astype(f32) + f32(0.5)) / y_f
        cx = np.broadcast_to(cx[None, :, None], (gh, gw, a))
        cy = np.broadcast_to(cy[:, None, None], (gh, gw, a))
        hw_, hh_ = f32(0.5) * pairs[:, 0], f32(0.5) * pairs[:, 1]
        box = np.stack([(cx - hw_) * f32(w_img), (cy - hh_) * f32(h_img), (cx + hw_) * f32(w_img), (cy + hh_) * f32(h_img)], axis=-1)
        assert box.dtype == f32
        out.append(box.reshape(-1, 4))
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(out)))


def select(score_matrix, k, score_thresh):
    """mv_ssd_topk_f32 restated: (N, K, V) -> idx (N, (K - 1) k) int32."""
    n, classes, v = score_matrix.shape
    thresh = torch.tensor(score_thresh, dtype=torch.float32)
    idx = torch.full((n, (classes - 1) * k), -1, dtype=torch.int32)
    for i in range(n):
        for c in range(1, classes):
            row = score_matrix[i, c]
            cand = torch.where(row > thresh)[0]
            order = torch.sort(row[cand], stable=True, descending=True)[1][:k]
            f = cand[order] * classes + c
            idx[i, (c - 1) * k:(c - 1) * k + f.numel()] = f.to(torch.int32)
    return idx


def decode(score_matrix, reg_maps, idx, dboxes, image_sizes, weights=(10.0, 10.0, 5.0, 5.0), clip=math.log(1000.0 / 16)):
    """mv_ssd_decode_f32 restated -> boxes (N, M, 4), scores (N, M), labels (N, M) int64, valid (N, M) bool."""
    n, classes, v = score_matrix.shape
    reg = torch.cat([permute_level(m, 4) for m in reg_maps], dim=1)  # (N, V, 4)
    coder = P.BoxCoder(weights, clip, numerics=P.RESTATEMENT)
    m_ = idx.shape[1]
    boxes, sc = torch.zeros((n, m_, 4)), torch.zeros((n, m_))
    labels, valid = torch.zeros((n, m_), dtype=torch.int64), torch.zeros((n, m_), dtype=torch.bool)
    for i in range(n):
        f = idx[i].to(torch.int64)
        ok = (f >= 0) & (torch.div(f, classes, rounding_mode="floor") < v)
        fa = f[ok]
        a, c = torch.div(fa, classes, rounding_mode="floor"), fa % classes
        with np.errstate(all="ignore"):
            b = coder.decode_single(reg[i][a], dboxes[a])
        b = clip_boxes_to_image(b, image_sizes[i])
        boxes[i][ok], sc[i][ok], labels[i][ok], valid[i][ok] = b, score_matrix[i, c, a], c, True
    return boxes, sc, labels, valid
