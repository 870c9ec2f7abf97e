"""The references of the keypoint branch of Keypoint R-CNN.

(a) The torch replica of the reference's models/detection/keypoint_rcnn.py and of the keypoint parts of roi_heads.py / transform.py
    (torchvision 0.20), written from its source as tests/_roi_heads_ref.py and tests/_mask_ref.py were: heatmaps_to_keypoints,
    keypointrcnn_inference, resize_keypoints, KeypointRCNNHeads, KeypointRCNNPredictor, KeypointRCNN on tests/_roi_heads_ref.py's
    FasterRCNN, keypointrcnn_resnet50_fpn.
(b) The numpy float32 restatements of what include/mi355vision.h states:
      cubic_taps / bicubic          the library's bicubic resize (mv_heatmaps_to_keypoints_f32), every operation rounded once, the
                                    source coordinate's fma through tests/_interp_ref.py's fma32
      keypoints(maps, rois)         mv_heatmaps_to_keypoints_f32: (xy (R, K, 3), scores (R, K))
      relaid4 / gather_phases / oracle_conv_transpose4   mv_conv_transpose4x4s2_bias_act_f32: the relayout, oracle/ref.py's conv with
                                    padding 1 on the relaid weight, the strided gather of the four phases
      bicubic_bound(in_h, in_w, max_abs)   the bound of |restatement - torch's CPU bicubic| derived in DESIGN.md 3.29
"""
import math

import numpy as np
import torch
from torch import nn

from oracle import ref
from tests import _fpn_ref as FP
from tests import _interp_ref as IR
from tests import _mask_ref as M
from tests import _resnet_ref as R
from tests import _roi_heads_ref as H

F32 = np.float32


# ------------------------------------------------------------------------------------------------ (a) the torch replica: roi_heads.py
def heatmaps_to_keypoints(maps, rois):
    offset_x = rois[:, 0]
    offset_y = rois[:, 1]

    widths = rois[:, 2] - rois[:, 0]
    heights = rois[:, 3] - rois[:, 1]
    widths = widths.clamp(min=1)
    heights = heights.clamp(min=1)
    widths_ceil = widths.ceil()
    heights_ceil = heights.ceil()

    num_keypoints = maps.shape[1]

    xy_preds = torch.zeros((len(rois), 3, num_keypoints), dtype=torch.float32, device=maps.device)
    end_scores = torch.zeros((len(rois), num_keypoints), dtype=torch.float32, device=maps.device)
    for i in range(len(rois)):
        roi_map_width = int(widths_ceil[i].item())
        roi_map_height = int(heights_ceil[i].item())
        width_correction = widths[i] / roi_map_width
        height_correction = heights[i] / roi_map_height
        roi_map = torch.nn.functional.interpolate(maps[i][:, None], size=(roi_map_height, roi_map_width), mode="bicubic",
                                                  align_corners=False)[:, 0]
        w = roi_map.shape[2]
        pos = roi_map.reshape(num_keypoints, -1).argmax(dim=1)

        x_int = pos % w
        y_int = torch.div(pos - x_int, w, rounding_mode="floor")
        x = (x_int.float() + 0.5) * width_correction
        y = (y_int.float() + 0.5) * height_correction
        xy_preds[i, 0, :] = x + offset_x[i]
        xy_preds[i, 1, :] = y + offset_y[i]
        xy_preds[i, 2, :] = 1
        end_scores[i, :] = roi_map[torch.arange(num_keypoints, device=roi_map.device), y_int, x_int]

    return xy_preds.permute(0, 2, 1), end_scores


def keypointrcnn_inference(x, boxes):
    kp_probs = []
    kp_scores = []

    boxes_per_image = [box.size(0) for box in boxes]
    x2 = x.split(boxes_per_image, dim=0)

    for xx, bb in zip(x2, boxes):
        kp_prob, scores = heatmaps_to_keypoints(xx, bb)
        kp_probs.append(kp_prob)
        kp_scores.append(scores)

    return kp_probs, kp_scores


def resize_keypoints(keypoints, original_size, new_size):
    ratios = [
        torch.tensor(s, dtype=torch.float32, device=keypoints.device) / torch.tensor(s_orig, dtype=torch.float32, device=keypoints.device)
        for s, s_orig in zip(new_size, original_size)
    ]
    ratio_h, ratio_w = ratios
    resized_data = keypoints.clone()
    resized_data[..., 0] *= ratio_w
    resized_data[..., 1] *= ratio_h
    return resized_data


# ------------------------------------------------------------------------------------------------ (a) the torch replica: keypoint_rcnn.py
class KeypointRCNNHeads(nn.Sequential):
    def __init__(self, in_channels, layers):
        d = []
        next_feature = in_channels
        for out_channels in layers:
            d.append(nn.Conv2d(next_feature, out_channels, 3, stride=1, padding=1))
            d.append(nn.ReLU(inplace=True))
            next_feature = out_channels
        super().__init__(*d)
        for m in self.children():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                nn.init.constant_(m.bias, 0)


class KeypointRCNNPredictor(nn.Module):
    def __init__(self, in_channels, num_keypoints):
        super().__init__()
        input_features = in_channels
        deconv_kernel = 4
        self.kps_score_lowres = nn.ConvTranspose2d(input_features, num_keypoints, deconv_kernel, stride=2, padding=deconv_kernel // 2 - 1)
        nn.init.kaiming_normal_(self.kps_score_lowres.weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.kps_score_lowres.bias, 0)
        self.up_scale = 2
        self.out_channels = num_keypoints

    def forward(self, x):
        x = self.kps_score_lowres(x)
        return torch.nn.functional.interpolate(x, scale_factor=float(self.up_scale), mode="bilinear", align_corners=False,
                                               recompute_scale_factor=False)


class KeypointRCNN(H.FasterRCNN):
    def __init__(self, backbone, num_classes=None, min_size=None, max_size=1333, image_mean=None, image_std=None, rpn_anchor_generator=None,
                 rpn_head=None, rpn_pre_nms_top_n_train=2000, rpn_pre_nms_top_n_test=1000, rpn_post_nms_top_n_train=2000,
                 rpn_post_nms_top_n_test=1000, rpn_nms_thresh=0.7, rpn_fg_iou_thresh=0.7, rpn_bg_iou_thresh=0.3,
                 rpn_batch_size_per_image=256, rpn_positive_fraction=0.5, rpn_score_thresh=0.0, box_roi_pool=None, box_head=None,
                 box_predictor=None, box_score_thresh=0.05, box_nms_thresh=0.5, box_detections_per_img=100, box_fg_iou_thresh=0.5,
                 box_bg_iou_thresh=0.5, box_batch_size_per_image=512, box_positive_fraction=0.25, bbox_reg_weights=None,
                 keypoint_roi_pool=None, keypoint_head=None, keypoint_predictor=None, num_keypoints=None, **kwargs):
        if not isinstance(keypoint_roi_pool, (H.MultiScaleRoIAlign, type(None))):
            raise TypeError(f"keypoint_roi_pool should be of type MultiScaleRoIAlign or None instead of {type(keypoint_roi_pool)}")
        if min_size is None:
            min_size = (640, 672, 704, 736, 768, 800)

        if num_keypoints is not None:
            if keypoint_predictor is not None:
                raise ValueError("num_keypoints should be None when keypoint_predictor is specified")
        else:
            num_keypoints = 17

        out_channels = backbone.out_channels

        if keypoint_roi_pool is None:
            keypoint_roi_pool = H.MultiScaleRoIAlign(featmap_names=["0", "1", "2", "3"], output_size=14, sampling_ratio=2)

        if keypoint_head is None:
            keypoint_layers = tuple(512 for _ in range(8))
            keypoint_head = KeypointRCNNHeads(out_channels, keypoint_layers)

        if keypoint_predictor is None:
            keypoint_dim_reduced = 512  # == keypoint_layers[-1]
            keypoint_predictor = KeypointRCNNPredictor(keypoint_dim_reduced, num_keypoints)

        super().__init__(backbone, num_classes, min_size, max_size, image_mean, image_std, rpn_anchor_generator, rpn_head,
                         rpn_pre_nms_top_n_train, rpn_pre_nms_top_n_test, rpn_post_nms_top_n_train, rpn_post_nms_top_n_test, rpn_nms_thresh,
                         rpn_fg_iou_thresh, rpn_bg_iou_thresh, rpn_batch_size_per_image, rpn_positive_fraction, rpn_score_thresh,
                         box_roi_pool, box_head, box_predictor, box_score_thresh, box_nms_thresh, box_detections_per_img, box_fg_iou_thresh,
                         box_bg_iou_thresh, box_batch_size_per_image, box_positive_fraction, bbox_reg_weights, **kwargs)

        self.roi_heads.keypoint_roi_pool = keypoint_roi_pool
        self.roi_heads.keypoint_head = keypoint_head
        self.roi_heads.keypoint_predictor = keypoint_predictor


def keypointrcnn_resnet50_fpn(*, weights=None, progress=True, num_classes=None, num_keypoints=None, weights_backbone=None,
                              trainable_backbone_layers=None, **kwargs):
    """keypoint_rcnn.py:356-474 without weight files, on a FrozenBatchNorm2d backbone (what the library builds)."""
    assert weights is None and weights_backbone is None
    if num_classes is None:
        num_classes = 2
    if num_keypoints is None:
        num_keypoints = 17
    backbone = R.resnet50(norm_layer=FP.FrozenBatchNorm2d)
    backbone = FP._resnet_fpn_extractor(backbone, 5 if trainable_backbone_layers is None else trainable_backbone_layers)
    return KeypointRCNN(backbone, num_classes, num_keypoints=num_keypoints, **kwargs)


# ------------------------------------------------------------------------------------------------ (b) the restatement: bicubic, keypoints
A = F32(-0.75)
MAX_ROI_SIDE = 1 << 15


def _c1(x):  # ((A + 2) x - (A + 3)) x x + 1, left to right
    return ((F32(1.25) * x - F32(2.25)) * x * x + F32(1)).astype(F32)


def _c2(x):  # ((A x - 5 A) x + 8 A) x - 4 A, left to right
    return (((A * x - F32(-3.75)) * x + F32(-6)) * x - F32(-3)).astype(F32)


def cubic_taps(n_in, n_out):
    """(idx (n_out, 4) clamped source indices, w (n_out, 4) float32 weights, i0 (n_out,)) of one axis."""
    s = F32(n_in) / F32(n_out)
    d = np.arange(n_out, dtype=F32)
    real = IR.fma32(np.full(n_out, s, F32), d + F32(0.5), F32(-0.5))
    i0 = np.minimum(np.floor(real).astype(np.int64), n_in - 1)
    t = np.clip(real - i0.astype(F32), F32(0), F32(1)).astype(F32)
    u = (F32(1) - t).astype(F32)
    w = np.stack([_c2(t + F32(1)), _c1(t), _c1(u), _c2(u + F32(1))], axis=1).astype(F32)
    idx = np.clip(i0[:, None] - 1 + np.arange(4)[None, :], 0, n_in - 1)
    return idx, w, i0


def _dot4(w, v):
    """w (..., 4) and v (..., 4) float32 -> ((w0 v0 + w1 v1) + w2 v2) + w3 v3, every product and sum rounded once."""
    with np.errstate(all="ignore"):
        p = (w * v).astype(F32)
        return (((p[..., 0] + p[..., 1]).astype(F32) + p[..., 2]).astype(F32) + p[..., 3]).astype(F32)


def bicubic(x, oh, ow):
    """(..., h, w) float32 -> (..., oh, ow): sum_i wy_i (sum_j wx_j x[y_i, x_j]), the inner sum first."""
    x = np.asarray(x, dtype=F32)
    h, w = x.shape[-2:]
    yi, wy, _ = cubic_taps(h, oh)
    xi, wx, _ = cubic_taps(w, ow)
    u = _dot4(wx, x[..., :, xi])                           # (..., h, ow)
    cols = np.moveaxis(u[..., yi, :], -2, -1)              # (..., oh, ow, 4)
    return _dot4(wy[:, None, :], cols)


def roi_geometry(roi):
    """One roi (4,) float32 -> (ok, bw, bh, rw, rh) in the library's arithmetic."""
    x1, y1, x2, y2 = (F32(v) for v in roi)
    with np.errstate(all="ignore"):
        bw, bh = np.maximum(F32(x2 - x1), F32(1)), np.maximum(F32(y2 - y1), F32(1))
    ok = bool(np.isfinite([x1, y1, x2, y2]).all() and bw <= MAX_ROI_SIDE and bh <= MAX_ROI_SIDE)
    if not ok:
        return False, bw, bh, 0, 0
    return True, bw, bh, int(math.ceil(float(bw))), int(math.ceil(float(bh)))


def keypoints(maps, rois, with_maps=False):
    """mv_heatmaps_to_keypoints_f32 on numpy maps (R, K, Mh, Mw) and rois (R, 4) -> (xy (R, K, 3), scores (R, K))[, the roi maps]."""
    maps, rois = np.asarray(maps, dtype=F32), np.asarray(rois, dtype=F32)
    r, k = maps.shape[:2]
    xy, scores, kept = np.zeros((r, k, 3), F32), np.zeros((r, k), F32), []
    for i in range(r):
        ok, bw, bh, rw, rh = roi_geometry(rois[i])
        if not ok:
            kept.append(None)
            continue
        roi_map = bicubic(maps[i], rh, rw)
        kept.append(roi_map)
        flat = roi_map.reshape(k, -1)
        pos = flat.argmax(1)  # numpy's argmax: a NaN is the maximum, the first one wins; else the first maximum
        xi, yi = pos % rw, pos // rw
        cx, cy = F32(bw / F32(rw)), F32(bh / F32(rh))
        xy[i, :, 0] = ((xi.astype(F32) + F32(0.5)) * cx).astype(F32) + rois[i, 0]
        xy[i, :, 1] = ((yi.astype(F32) + F32(0.5)) * cy).astype(F32) + rois[i, 1]
        xy[i, :, 2] = 1
        scores[i] = flat[np.arange(k), pos]
    return (xy, scores, kept) if with_maps else (xy, scores)


def bicubic_bound(in_h, in_w, max_abs):
    """|restatement - torch's CPU bicubic| <= this, u = 2^-24, S = 1.375 the largest sum of |weights| of an axis:
      arithmetic   each side evaluates 20 products and 6 sums on a path of 8 roundings: 2 * 8 u S^2 max|x|
      weights      the source coordinate: one rounding here (fma), two in a multiply-subtract, so t differs by <= 1.5 ulp(in);
                   a weight's slope is <= 1.35, and a weight is 5-6 operations on intermediates below 6: <= 36 u per side, so two
                   weights differ by E = 1.35 * 1.5 ulp(in) + 72 u, and the 2-D weights' sum by <= S * 4 E per axis."""
    u, s = 2.0 ** -24, 1.375
    total = 16 * u * s * s
    for n in (in_h, in_w):
        ulp_in = 2.0 ** (math.floor(math.log2(max(n, 1))) - 23)
        total += s * 4 * (1.35 * 1.5 * ulp_in + 72 * u)
    return total * float(max_abs)


# ------------------------------------------------------------------------------------------------ (b) the oracle: transposed conv, modules
def relaid4(weight, bias):
    """torch's ConvTranspose2d weight (cin, cout, 4, 4) -> w2 (4 cout, cin, 2, 2), w2[4 co + 2 py + px, ci, ty, tx] =
    weight[ci, co, 3 - py - 2 ty, 3 - px - 2 tx]; the bias repeated four times."""
    w = np.asarray(weight, dtype=F32)
    cin, cout = w.shape[:2]
    w2 = np.empty((cout, 2, 2, cin, 2, 2), F32)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    w2[:, py, px, :, ty, tx] = w[:, :, 3 - py - 2 * ty, 3 - px - 2 * tx].T
    b4 = None if bias is None else np.ascontiguousarray(np.repeat(np.asarray(bias, dtype=F32), 4))
    return np.ascontiguousarray(w2.reshape(4 * cout, cin, 2, 2)), b4


def gather_phases(y4):
    """(n, 4 cout, h + 1, w + 1), channel 4 co + 2 py + px -> (n, cout, 2 h, 2 w): phase (py, px) keeps position (m + py, n + px).
    numpy or torch."""
    n, c4, h1, w1 = y4.shape
    h, w = h1 - 1, w1 - 1
    y = (torch.empty if isinstance(y4, torch.Tensor) else np.empty)((n, c4 // 4, 2 * h, 2 * w), dtype=y4.dtype,
                                                                     **({"device": y4.device} if isinstance(y4, torch.Tensor) else {}))
    for py in range(2):
        for px in range(2):
            y[:, :, py::2, px::2] = y4[:, 2 * py + px::4, py:py + h, px:px + w]
    return y


def oracle_conv_transpose4(x, weight, bias, act):
    """ConvTranspose2d(4, stride 2, padding 1) + bias + act ("relu" / None) of a numpy x (n, cin, h, w) and torch-layout weight
    (cin, cout, 4, 4): oracle/ref.py's conv (one ascending chain per output, + bias, activation) on the relaid weight, gathered."""
    x = np.ascontiguousarray(x, dtype=F32)
    w2, b4 = relaid4(weight, bias)
    return gather_phases(ref.conv2d_affine_act(x, w2, b4, None, None, None, 1, 1, 1, 0, act))


def oracle_heads(heads, x):
    """A CPU-resident KeypointRCNNHeads (the library's or the replica's: same children) on a numpy x."""
    x = np.ascontiguousarray(x, dtype=F32)
    for conv in list(heads)[::2]:
        assert conv.padding == (1, 1) and conv.kernel_size == (3, 3)
        x = M.oracle_conv3x3(x, conv.weight.detach().numpy(), conv.bias.detach().numpy(), relu=True)
    return x


def oracle_predictor(pred, x):
    """A CPU-resident KeypointRCNNPredictor on a numpy x -> (the ConvTranspose2d output, the x2 bilinear upsample of it)."""
    conv = pred.kps_score_lowres
    low = oracle_conv_transpose4(x, conv.weight.detach().numpy(), conv.bias.detach().numpy(), None)
    return low, IR.interpolate(low, 2 * low.shape[-2], 2 * low.shape[-1])
