"""References for the Mask R-CNN tests (a helper module, not a test file and not a conftest).

(a) A plain-torch replica of the reference's mask path (torchvision is not importable in the test environment), written from the
    reference's source like tests/_roi_heads_ref.py: roi_heads.py's expand_boxes, expand_masks, paste_mask_in_image,
    paste_masks_in_image and maskrcnn_inference, and mask_rcnn.py's MaskRCNNHeads, MaskRCNNPredictor, MaskRCNN and
    maskrcnn_resnet50_fpn on tests/_roi_heads_ref.py's FasterRCNN -- the same classes, constructor arguments, child names,
    construction order and initialisation, with torch's own forward.
(b) The restatement the library is compared with bit for bit, what include/mi355vision.h states:
      expanded_boxes / paste    mv_paste_masks_f32 in numpy float32, on tests/_interp_ref.interpolate
      mask_probs                mv_mask_probs_f32 on tests/_rpn_ref.sigmoid_cr
      oracle_conv_transpose     mv_conv_transpose2x2_bias_act_f32: oracle/ref.py's pointwise conv on the weight relaid to (4 cout, cin)
                                in the summation order F.conv1x1_k_slices states (the call tests/_fpn_ref.oracle_lateral makes), then a
                                numpy pixel shuffle
      oracle_heads / oracle_predictor   the modules as compositions of the oracle's layers
"""
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from oracle import ref
from tests import _fpn_ref as FP
from tests import _interp_ref as IR
from tests import _resnet_ref as R
from tests import _roi_heads_ref as H
from tests import _rpn_ref as P

F32 = np.float32


# ------------------------------------------------------------------------------------------------ (a) the torch replica: roi_heads.py
def expand_boxes(boxes, scale):
    w_half = (boxes[:, 2] - boxes[:, 0]) * 0.5
    h_half = (boxes[:, 3] - boxes[:, 1]) * 0.5
    x_c = (boxes[:, 2] + boxes[:, 0]) * 0.5
    y_c = (boxes[:, 3] + boxes[:, 1]) * 0.5

    w_half *= scale
    h_half *= scale

    boxes_exp = torch.zeros_like(boxes)
    boxes_exp[:, 0] = x_c - w_half
    boxes_exp[:, 2] = x_c + w_half
    boxes_exp[:, 1] = y_c - h_half
    boxes_exp[:, 3] = y_c + h_half
    return boxes_exp


def expand_masks(mask, padding):
    M = mask.shape[-1]
    scale = float(M + 2 * padding) / M
    padded_mask = nn.functional.pad(mask, (padding,) * 4)
    return padded_mask, scale


def paste_mask_in_image(mask, box, im_h, im_w):
    TO_REMOVE = 1
    w = int(box[2] - box[0] + TO_REMOVE)
    h = int(box[3] - box[1] + TO_REMOVE)
    w = max(w, 1)
    h = max(h, 1)

    # Set shape to [batchxCxHxW]
    mask = mask.expand((1, 1, -1, -1))

    # Resize mask
    mask = nn.functional.interpolate(mask, size=(h, w), mode="bilinear", align_corners=False)
    mask = mask[0][0]

    im_mask = torch.zeros((im_h, im_w), dtype=mask.dtype, device=mask.device)
    x_0 = max(box[0], 0)
    x_1 = min(box[2] + 1, im_w)
    y_0 = max(box[1], 0)
    y_1 = min(box[3] + 1, im_h)

    im_mask[y_0:y_1, x_0:x_1] = mask[(y_0 - box[1]):(y_1 - box[1]), (x_0 - box[0]):(x_1 - box[0])]
    return im_mask


def paste_masks_in_image(masks, boxes, img_shape, padding=1):
    masks, scale = expand_masks(masks, padding=padding)
    boxes = expand_boxes(boxes, scale).to(dtype=torch.int64)
    im_h, im_w = img_shape

    res = [paste_mask_in_image(m[0], b, im_h, im_w) for m, b in zip(masks, boxes)]
    if len(res) > 0:
        ret = torch.stack(res, dim=0)[:, None]
    else:
        ret = masks.new_empty((0, 1, im_h, im_w))
    return ret


def maskrcnn_inference(x, labels):
    mask_prob = x.sigmoid()

    # select masks corresponding to the predicted classes
    num_masks = x.shape[0]
    boxes_per_image = [label.shape[0] for label in labels]
    labels = torch.cat(labels)
    index = torch.arange(num_masks, device=labels.device)
    mask_prob = mask_prob[index, labels][:, None]
    mask_prob = mask_prob.split(boxes_per_image, dim=0)

    return mask_prob


# ------------------------------------------------------------------------------------------------ (a) the torch replica: mask_rcnn.py
class Conv2dNormActivation(nn.Sequential):
    """ops/misc.py Conv2dNormActivation as MaskRCNNHeads uses it: [Conv2d, norm?, ReLU(inplace)]."""

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


class MaskRCNNHeads(nn.Sequential):
    _version = 2

    def __init__(self, in_channels, layers, dilation, norm_layer=None):
        blocks = []
        next_feature = in_channels
        for layer_features in layers:
            blocks.append(Conv2dNormActivation(next_feature, layer_features, kernel_size=3, stride=1, padding=dilation, dilation=dilation,
                                               norm_layer=norm_layer))
            next_feature = layer_features

        super().__init__(*blocks)
        for layer in self.modules():
            if isinstance(layer, nn.Conv2d):
                nn.init.kaiming_normal_(layer.weight, mode="fan_out", nonlinearity="relu")
                if layer.bias is not None:
                    nn.init.zeros_(layer.bias)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)

        if version is None or version < 2:
            num_blocks = len(self)
            for i in range(num_blocks):
                for type in ["weight", "bias"]:
                    old_key = f"{prefix}mask_fcn{i+1}.{type}"
                    new_key = f"{prefix}{i}.0.{type}"
                    if old_key in state_dict:
                        state_dict[new_key] = state_dict.pop(old_key)

        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


class MaskRCNNPredictor(nn.Sequential):
    def __init__(self, in_channels, dim_reduced, num_classes):
        super().__init__(
            OrderedDict(
                [
                    ("conv5_mask", nn.ConvTranspose2d(in_channels, dim_reduced, 2, 2, 0)),
                    ("relu", nn.ReLU(inplace=True)),
                    ("mask_fcn_logits", nn.Conv2d(dim_reduced, num_classes, 1, 1, 0)),
                ]
            )
        )

        for name, param in self.named_parameters():
            if "weight" in name:
                nn.init.kaiming_normal_(param, mode="fan_out", nonlinearity="relu")


class MaskRCNN(H.FasterRCNN):
    def __init__(self, backbone, num_classes=None, min_size=800, max_size=1333, image_mean=None, image_std=None, rpn_anchor_generator=None,
                 rpn_head=None, rpn_pre_nms_top_n_train=2000, rpn_pre_nms_top_n_test=1000, rpn_post_nms_top_n_train=2000,
                 rpn_post_nms_top_n_test=1000, rpn_nms_thresh=0.7, rpn_fg_iou_thresh=0.7, rpn_bg_iou_thresh=0.3,
                 rpn_batch_size_per_image=256, rpn_positive_fraction=0.5, rpn_score_thresh=0.0, box_roi_pool=None, box_head=None,
                 box_predictor=None, box_score_thresh=0.05, box_nms_thresh=0.5, box_detections_per_img=100, box_fg_iou_thresh=0.5,
                 box_bg_iou_thresh=0.5, box_batch_size_per_image=512, box_positive_fraction=0.25, bbox_reg_weights=None,
                 mask_roi_pool=None, mask_head=None, mask_predictor=None, **kwargs):
        if not isinstance(mask_roi_pool, (H.MultiScaleRoIAlign, type(None))):
            raise TypeError(f"mask_roi_pool should be of type MultiScaleRoIAlign or None instead of {type(mask_roi_pool)}")

        if num_classes is not None:
            if mask_predictor is not None:
                raise ValueError("num_classes should be None when mask_predictor is specified")

        out_channels = backbone.out_channels

        if mask_roi_pool is None:
            mask_roi_pool = H.MultiScaleRoIAlign(featmap_names=["0", "1", "2", "3"], output_size=14, sampling_ratio=2)

        if mask_head is None:
            mask_layers = (256, 256, 256, 256)
            mask_dilation = 1
            mask_head = MaskRCNNHeads(out_channels, mask_layers, mask_dilation)

        if mask_predictor is None:
            mask_predictor_in_channels = 256  # == mask_layers[-1]
            mask_dim_reduced = 256
            mask_predictor = MaskRCNNPredictor(mask_predictor_in_channels, mask_dim_reduced, num_classes)

        super().__init__(backbone, num_classes, min_size, max_size, image_mean, image_std, rpn_anchor_generator, rpn_head,
                         rpn_pre_nms_top_n_train, rpn_pre_nms_top_n_test, rpn_post_nms_top_n_train, rpn_post_nms_top_n_test, rpn_nms_thresh,
                         rpn_fg_iou_thresh, rpn_bg_iou_thresh, rpn_batch_size_per_image, rpn_positive_fraction, rpn_score_thresh,
                         box_roi_pool, box_head, box_predictor, box_score_thresh, box_nms_thresh, box_detections_per_img, box_fg_iou_thresh,
                         box_bg_iou_thresh, box_batch_size_per_image, box_positive_fraction, bbox_reg_weights, **kwargs)

        self.roi_heads.mask_roi_pool = mask_roi_pool
        self.roi_heads.mask_head = mask_head
        self.roi_heads.mask_predictor = mask_predictor


def maskrcnn_resnet50_fpn(*, weights=None, progress=True, num_classes=None, weights_backbone=None, trainable_backbone_layers=None, **kwargs):
    """mask_rcnn.py:398-493 without weight files, on a FrozenBatchNorm2d backbone (what the library builds)."""
    assert weights is None and weights_backbone is None
    if num_classes is None:
        num_classes = 91
    backbone = R.resnet50(norm_layer=FP.FrozenBatchNorm2d)
    backbone = FP._resnet_fpn_extractor(backbone, 5 if trainable_backbone_layers is None else trainable_backbone_layers)
    return MaskRCNN(backbone, num_classes=num_classes, **kwargs)


# ------------------------------------------------------------------------------------------------ (b) the restatement: paste
LIMIT = F32(2.0 ** 30)


def expanded_boxes(boxes, m, padding):
    """boxes (R, 4) float32 -> ((R, 4) int64 rows (bx0, by0, bx1, by1), ok (R,)): expand_boxes in float32, one rounding per operation,
    the scale float32((double)(m + 2 padding) / m), then the truncation toward zero.  ok is False where an expanded coordinate is not
    finite or reaches 2^30 in magnitude (the integers are 0 there): the roi writes a zero plane."""
    b = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    scale = F32(float(m + 2 * padding) / m)
    with np.errstate(all="ignore"):
        wh = ((b[:, 2] - b[:, 0]) * F32(0.5)).astype(F32)
        hh = ((b[:, 3] - b[:, 1]) * F32(0.5)).astype(F32)
        xc = ((b[:, 2] + b[:, 0]) * F32(0.5)).astype(F32)
        yc = ((b[:, 3] + b[:, 1]) * F32(0.5)).astype(F32)
        wh, hh = (wh * scale).astype(F32), (hh * scale).astype(F32)
        e = np.stack([xc - wh, yc - hh, xc + wh, yc + hh], 1).astype(F32)
        ok = (np.abs(e) < LIMIT).all(1)  # a NaN fails the comparison
        ints = np.trunc(np.where(ok[:, None], e, F32(0))).astype(np.int64)
    return ints, ok


def padded(mask, padding):
    m = np.asarray(mask, dtype=F32)
    return np.pad(m, [(0, 0)] * (m.ndim - 2) + [(padding, padding)] * 2)


def paste(masks, boxes, im_h, im_w, padding=1):
    """masks (R, 1, M, M), boxes (R, 4) -> (R, 1, im_h, im_w) float32: the rule of mv_paste_masks_f32."""
    masks = np.asarray(masks, dtype=F32)
    r, m = masks.shape[0], masks.shape[-1]
    ints, ok = expanded_boxes(boxes, m, padding)
    out = np.zeros((r, 1, im_h, im_w), dtype=F32)
    for i in range(r):
        if not ok[i]:
            continue
        bx0, by0, bx1, by1 = (int(v) for v in ints[i])
        w, h = max(bx1 - bx0 + 1, 1), max(by1 - by0 + 1, 1)
        x0, x1, y0, y1 = max(bx0, 0), min(bx1 + 1, im_w), max(by0, 0), min(by1 + 1, im_h)
        if x0 >= x1 or y0 >= y1:
            continue
        cols = np.arange(x0 - bx0, x1 - bx0)
        rows = np.arange(y0 - by0, y1 - by0)
        resized = interpolate_window(padded(masks[i, 0], padding), h, w, rows, cols)
        out[i, 0, y0:y1, x0:x1] = resized
    return out


def interpolate_window(x, oh, ow, rows, cols):
    """tests/_interp_ref.interpolate of the 2-D x to (oh, ow), only the output rows `rows` and columns `cols` (a box larger than the
    image is never resized whole)."""
    h, w = x.shape
    y0, y1, wy0, wy1 = (a[rows] for a in IR.axis_taps(h, oh))
    x0, x1, wx0, wx1 = (a[cols] for a in IR.axis_taps(w, ow))
    top, bot = x[y0, :], x[y1, :]
    with np.errstate(all="ignore"):
        t = IR.fma32(np.broadcast_to(wx0, top[:, x0].shape), top[:, x0], wx1 * top[:, x1])
        u = IR.fma32(np.broadcast_to(wx0, bot[:, x0].shape), bot[:, x0], wx1 * bot[:, x1])
        return IR.fma32(np.broadcast_to(wy0[:, None], t.shape), t, wy1[:, None] * u)


def paste_bound(m, padding, max_abs=1.0):
    """|replica - restatement| allowed where torch takes its non-vectorised loops: (6 + 8 (M + 2 p)) 2^-24 max|x|."""
    return (6 + 8 * (m + 2 * padding)) * 2.0 ** -24 * max_abs


TORCH_VECTORISED_ABOVE = 3264  # elements of the resized mask above which torch 2.10's CPU interpolate takes its vectorised loop


NAN, INF = float("nan"), float("inf")
PASTE_IMAGES = [(37, 53), (40, 56), (37, 601), (40, 600)]  # scalar stores, 16-byte stores, and both again with three column blocks per row


def paste_boxes(h, w):
    """The rois of the paste tests for an (h, w) image -> (finite (K, 4), zero-plane (3, 4)) float32 boxes.  `finite` are boxes the
    reference accepts: well inside; sticking out on the left, the top, the right, the bottom; larger than the image; a 1 x 1 box;
    x1 == x2 == w; inverted; one whose truncation goes through a negative fraction (-0.5.. -> 0, a floor would give -1); one almost as
    wide as the image (several column blocks of the kernel when w > 256).  `zero-plane` are a NaN, an infinite and a huge box."""
    finite = np.array([[10.3, 8.2, 30.7, 25.9], [-7.5, 10.0, 12.0, 20.0], [10.0, -6.2, 25.0, 9.0], [w - 10.5, 5.0, w + 8.3, 20.0],
                       [5.0, h - 9.2, 22.0, h + 6.6], [-20.0, -15.0, w + 25.0, h + 18.0], [12.4, 13.4, 12.6, 13.6],
                       [float(w), 5.0, float(w), 20.0], [30.0, 25.0, 20.0, 10.0], [-0.1, 3.0, 12.0, 18.0], [3.2, 1.0, w - 2.7, h - 1.5]], dtype=F32)
    zero_plane = np.array([[NAN, 3.0, 10.0, 12.0], [2.0, -INF, 9.0, 8.0], [0.0, 1.0, 3.0e9, 9.0]], dtype=F32)
    return finite, zero_plane


def paste_masks(seed, r, m):
    """(r, 1, m, m) float32 in [0, 1] with exact zeros and ones among them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((r, 1, m, m), generator=g)
    u = torch.rand((r, 1, m, m), generator=g)
    x[u < 0.1] = 0.0
    x[u > 0.9] = 1.0
    return x


# ------------------------------------------------------------------------------------------------ (b) the restatement: probabilities
def mask_probs(logits, labels):
    """logits (R, C, Mh, Mw) float32 torch tensor, labels (R,) int64 -> (R, 1, Mh, Mw): sigmoid_cr of the selected plane, a zero plane
    for a label outside [0, C)."""
    r, c = logits.shape[:2]
    out = torch.zeros((r, 1) + tuple(logits.shape[2:]), dtype=torch.float32)
    for i in range(r):
        lab = int(labels[i])
        if 0 <= lab < c:
            out[i, 0] = P.sigmoid_cr(logits[i, lab].contiguous())
    return out


# ------------------------------------------------------------------------------------------------ (b) the oracle: transposed conv, modules
def relaid(weight, bias):
    """torch's ConvTranspose2d weight (cin, cout, 2, 2) -> (4 cout, cin), row 4 co + 2 dy + dx; the bias repeated four times."""
    w = np.asarray(weight, dtype=F32)
    cin, cout = w.shape[:2]
    w4 = np.ascontiguousarray(w.transpose(1, 2, 3, 0).reshape(4 * cout, cin))
    b4 = None if bias is None else np.ascontiguousarray(np.repeat(np.asarray(bias, dtype=F32), 4))
    return w4, b4


def pixel_shuffle(y4):
    """(n, 4 cout, h, w) with channel 4 co + 2 dy + dx -> (n, cout, 2 h, 2 w)."""
    n, c4, h, w = y4.shape
    y = y4.reshape(n, c4 // 4, 2, 2, h, w).transpose(0, 1, 4, 2, 5, 3)
    return np.ascontiguousarray(y.reshape(n, c4 // 4, 2 * h, 2 * w))


def oracle_conv_transpose(x, weight, bias, act, slice_len=None):
    """ConvTranspose2d(2, 2) + bias + act ("relu" / None) of a numpy x (n, cin, h, w) and torch-layout weight (cin, cout, 2, 2).
    slice_len: None = the order F.conv1x1_k_slices(n, cin, h, w, 4 cout) states; 0 = one ascending chain."""
    x = np.ascontiguousarray(x, dtype=F32)
    n, cin, h, wd = x.shape
    w4, b4 = relaid(weight, bias)
    if slice_len is None:
        from cpu_vision_amd import functional as F
        slices, sl = F.conv1x1_k_slices(n, cin, h, wd, w4.shape[0])
        slice_len = sl if slices > 1 else 0
    y4 = ref.conv2d_affine_act(x, np.ascontiguousarray(w4.reshape(w4.shape[0], cin, 1, 1)), b4, None, None, None, 1, 0, 1, 0, act,
                               slice_len=slice_len)
    return pixel_shuffle(y4)


def oracle_conv3x3(x, w, b, relu=True):
    """F.conv2d_bias_relu's oracle in the order F.conv3x3_k_slices states for the shape."""
    from cpu_vision_amd import functional as F
    n, cin, h, wd = x.shape
    slices, sc = F.conv3x3_k_slices(n, cin, h, wd, w.shape[0])
    return ref.conv3x3_bias_relu(x, w, b, relu=relu, slice_channels=sc if slices > 1 else 0)


def oracle_heads(heads, x):
    """A CPU-resident MaskRCNNHeads (the library's or the replica's: same children; no norm, dilation 1) on a numpy x."""
    x = np.ascontiguousarray(x, dtype=F32)
    for block in heads:
        conv = block[0]
        assert len(block) == 2 and conv.dilation == (1, 1) and conv.padding == (1, 1)
        x = oracle_conv3x3(x, conv.weight.detach().numpy(), conv.bias.detach().numpy(), relu=True)
    return x


def oracle_pointwise(x, w, b):
    from cpu_vision_amd import functional as F
    n, cin, h, wd = x.shape
    slices, sl = F.conv1x1_k_slices(n, cin, h, wd, w.shape[0])
    return ref.conv2d_affine_act(x, np.ascontiguousarray(w.reshape(w.shape[0], cin, 1, 1)), b, None, None, None, 1, 0, 1, 0, None,
                                 slice_len=sl if slices > 1 else 0)


def oracle_predictor(pred, x):
    """A CPU-resident MaskRCNNPredictor on a numpy x -> (the ConvTranspose2d + ReLU output, the logits)."""
    conv, logits = pred.conv5_mask, pred.mask_fcn_logits
    up = oracle_conv_transpose(x, conv.weight.detach().numpy(), conv.bias.detach().numpy(), "relu")
    return up, oracle_pointwise(up, logits.weight.detach().numpy(), logits.bias.detach().numpy())
