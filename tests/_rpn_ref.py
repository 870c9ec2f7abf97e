"""References for the RPN tests (a helper module, not a test file and not a conftest).  Imports nothing from the package.

(a) A plain-torch replica of the reference's models/detection/image_list.py, anchor_utils.py, _utils.py::BoxCoder (decode half) and
    rpn.py (torchvision is not importable in the test environment), written from the reference's source like tests/_fpn_ref.py:
    the same classes, constructor arguments, child names, construction order and initialisation, with torch's own forward,
    torch.topk, torch.exp and torch.sigmoid.  Its nms is tests/_detect_ref.py's restatement of the reference's CPU kernel under
    the coordinate trick of batched_nms, with the same float32 `boxes + offsets` arithmetic.
(b) The restatement the library is compared with bit for bit: (a) with three substitutions (`Numerics`),
      exp(v)      -> torch.exp(v.double()).float()          the correctly rounded float32 exp
      sigmoid(v)  -> 1 / (1 + E(-v)) in float32
      topk        -> the first k of torch.sort(stable=True, descending=True)
    torch's CPU exp is a 1-ulp vector routine (and its one-element path disagrees with its vector path on sigmoid), so no kernel can
    reproduce (a) bit for bit; (b) is what mi355vision.h states.
"""
import math

import numpy as np
import torch
from torch import nn

from tests import _detect_ref as D


# ------------------------------------------------------------------------------------------------ the three substitutions
def exp_cr(v):
    """The correctly rounded float32 exp (float64 inputs: torch's own)."""
    return torch.exp(v.double()).to(v.dtype)


def sigmoid_cr(v):
    one = torch.ones((), dtype=v.dtype, device=v.device)
    return one / (one + exp_cr(-v))


def topk_torch(ob, k):
    return ob.topk(k, dim=1)[1]


def topk_stable(ob, k):
    return torch.sort(ob, dim=1, stable=True, descending=True)[1][:, :k]


class Numerics:
    def __init__(self, exp, sigmoid, topk):
        self.exp, self.sigmoid, self.topk = exp, sigmoid, topk


REPLICA = Numerics(torch.exp, torch.sigmoid, topk_torch)
RESTATEMENT = Numerics(exp_cr, sigmoid_cr, topk_stable)


# ------------------------------------------------------------------------------------------------ the torch replica
class ImageList:
    def __init__(self, tensors, image_sizes):
        self.tensors = tensors
        self.image_sizes = image_sizes

    def to(self, device):
        return ImageList(self.tensors.to(device), self.image_sizes)


class AnchorGenerator(nn.Module):
    def __init__(self, sizes=((128, 256, 512),), aspect_ratios=((0.5, 1.0, 2.0),)):
        super().__init__()
        if not isinstance(sizes[0], (list, tuple)):
            sizes = tuple((s,) for s in sizes)
        if not isinstance(aspect_ratios[0], (list, tuple)):
            aspect_ratios = (aspect_ratios,) * len(sizes)
        self.sizes = sizes
        self.aspect_ratios = aspect_ratios
        self.cell_anchors = [self.generate_anchors(size, aspect_ratio) for size, aspect_ratio in zip(sizes, aspect_ratios)]

    def generate_anchors(self, scales, aspect_ratios, dtype=torch.float32, device=torch.device("cpu")):
        scales = torch.as_tensor(scales, dtype=dtype, device=device)
        aspect_ratios = torch.as_tensor(aspect_ratios, dtype=dtype, device=device)
        h_ratios = torch.sqrt(aspect_ratios)
        w_ratios = 1 / h_ratios
        ws = (w_ratios[:, None] * scales[None, :]).view(-1)
        hs = (h_ratios[:, None] * scales[None, :]).view(-1)
        base_anchors = torch.stack([-ws, -hs, ws, hs], dim=1) / 2
        return base_anchors.round()

    def set_cell_anchors(self, dtype, device):
        self.cell_anchors = [cell_anchor.to(dtype=dtype, device=device) for cell_anchor in self.cell_anchors]

    def num_anchors_per_location(self):
        return [len(s) * len(a) for s, a in zip(self.sizes, self.aspect_ratios)]

    def grid_anchors(self, grid_sizes, strides):
        anchors = []
        cell_anchors = self.cell_anchors
        torch._assert(cell_anchors is not None, "cell_anchors should not be None")
        torch._assert(
            len(grid_sizes) == len(strides) == len(cell_anchors),
            "Anchors should be Tuple[Tuple[int]] because each feature "
            "map could potentially have different sizes and aspect ratios. "
            "There needs to be a match between the number of "
            "feature maps passed and the number of sizes / aspect ratios specified.",
        )
        for size, stride, base_anchors in zip(grid_sizes, strides, cell_anchors):
            grid_height, grid_width = size
            stride_height, stride_width = stride
            device = base_anchors.device
            shifts_x = torch.arange(0, grid_width, dtype=torch.int32, device=device) * stride_width
            shifts_y = torch.arange(0, grid_height, dtype=torch.int32, device=device) * stride_height
            shift_y, shift_x = torch.meshgrid(shifts_y, shifts_x, indexing="ij")
            shift_x = shift_x.reshape(-1)
            shift_y = shift_y.reshape(-1)
            shifts = torch.stack((shift_x, shift_y, shift_x, shift_y), dim=1)
            anchors.append((shifts.view(-1, 1, 4) + base_anchors.view(1, -1, 4)).reshape(-1, 4))
        return anchors

    def forward(self, image_list, feature_maps):
        grid_sizes = [feature_map.shape[-2:] for feature_map in feature_maps]
        image_size = image_list.tensors.shape[-2:]
        dtype, device = feature_maps[0].dtype, feature_maps[0].device
        strides = [[torch.empty((), dtype=torch.int64, device=device).fill_(image_size[0] // g[0]),
                    torch.empty((), dtype=torch.int64, device=device).fill_(image_size[1] // g[1])] for g in grid_sizes]
        self.set_cell_anchors(dtype, device)
        anchors_over_all_feature_maps = self.grid_anchors(grid_sizes, strides)
        anchors = []
        for _ in range(len(image_list.image_sizes)):
            anchors.append([a for a in anchors_over_all_feature_maps])
        return [torch.cat(anchors_per_image) for anchors_per_image in anchors]


class BoxCoder:
    def __init__(self, weights, bbox_xform_clip=math.log(1000.0 / 16), numerics=REPLICA):
        self.weights = weights
        self.bbox_xform_clip = bbox_xform_clip
        self.numerics = numerics

    def decode(self, rel_codes, boxes):
        torch._assert(isinstance(boxes, (list, tuple)), "This function expects boxes of type list or tuple.")
        torch._assert(isinstance(rel_codes, torch.Tensor), "This function expects rel_codes of type torch.Tensor.")
        boxes_per_image = [b.size(0) for b in boxes]
        concat_boxes = torch.cat(boxes, dim=0)
        box_sum = 0
        for val in boxes_per_image:
            box_sum += val
        if box_sum > 0:
            rel_codes = rel_codes.reshape(box_sum, -1)
        pred_boxes = self.decode_single(rel_codes, concat_boxes)
        if box_sum > 0:
            pred_boxes = pred_boxes.reshape(box_sum, -1, 4)
        return pred_boxes

    def decode_single(self, rel_codes, boxes):
        boxes = boxes.to(rel_codes.dtype)
        widths = boxes[:, 2] - boxes[:, 0]
        heights = boxes[:, 3] - boxes[:, 1]
        ctr_x = boxes[:, 0] + 0.5 * widths
        ctr_y = boxes[:, 1] + 0.5 * heights
        wx, wy, ww, wh = self.weights
        dx = rel_codes[:, 0::4] / wx
        dy = rel_codes[:, 1::4] / wy
        dw = rel_codes[:, 2::4] / ww
        dh = rel_codes[:, 3::4] / wh
        # Prevent sending too large values into torch.exp()
        dw = torch.clamp(dw, max=self.bbox_xform_clip)
        dh = torch.clamp(dh, max=self.bbox_xform_clip)
        pred_ctr_x = dx * widths[:, None] + ctr_x[:, None]
        pred_ctr_y = dy * heights[:, None] + ctr_y[:, None]
        pred_w = self.numerics.exp(dw) * widths[:, None]
        pred_h = self.numerics.exp(dh) * heights[:, None]
        # Distance from center to box's corner.
        c_to_c_h = torch.tensor(0.5, dtype=pred_ctr_y.dtype, device=pred_h.device) * pred_h
        c_to_c_w = torch.tensor(0.5, dtype=pred_ctr_x.dtype, device=pred_w.device) * pred_w
        pred_boxes1 = pred_ctr_x - c_to_c_w
        pred_boxes2 = pred_ctr_y - c_to_c_h
        pred_boxes3 = pred_ctr_x + c_to_c_w
        pred_boxes4 = pred_ctr_y + c_to_c_h
        return torch.stack((pred_boxes1, pred_boxes2, pred_boxes3, pred_boxes4), dim=2).flatten(1)


class Conv2dNormActivation(nn.Sequential):
    """ops/misc.py:68-172 as the head uses it: conv with a bias + ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size=3, norm_layer=None):
        assert norm_layer is None
        super().__init__(nn.Conv2d(in_channels, out_channels, kernel_size, 1, (kernel_size - 1) // 2, bias=True), nn.ReLU(inplace=True))
        self.out_channels = out_channels


class RPNHead(nn.Module):
    _version = 2

    def __init__(self, in_channels, num_anchors, conv_depth=1):
        super().__init__()
        convs = []
        for _ in range(conv_depth):
            convs.append(Conv2dNormActivation(in_channels, in_channels, kernel_size=3, norm_layer=None))
        self.conv = nn.Sequential(*convs)
        self.cls_logits = nn.Conv2d(in_channels, num_anchors, kernel_size=1, stride=1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=1, stride=1)
        for layer in self.modules():
            if isinstance(layer, torch.nn.Conv2d):
                torch.nn.init.normal_(layer.weight, std=0.01)
                if layer.bias is not None:
                    torch.nn.init.constant_(layer.bias, 0)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:
            for type in ["weight", "bias"]:
                old_key = f"{prefix}conv.{type}"
                new_key = f"{prefix}conv.0.0.{type}"
                if old_key in state_dict:
                    state_dict[new_key] = state_dict.pop(old_key)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x):
        logits = []
        bbox_reg = []
        for feature in x:
            t = self.conv(feature)
            logits.append(self.cls_logits(t))
            bbox_reg.append(self.bbox_pred(t))
        return logits, bbox_reg


def permute_and_flatten(layer, N, A, C, H, W):
    layer = layer.view(N, -1, C, H, W)
    layer = layer.permute(0, 3, 4, 1, 2)
    layer = layer.reshape(N, -1, C)
    return layer


def concat_box_prediction_layers(box_cls, box_regression):
    box_cls_flattened = []
    box_regression_flattened = []
    for box_cls_per_level, box_regression_per_level in zip(box_cls, box_regression):
        N, AxC, H, W = box_cls_per_level.shape
        Ax4 = box_regression_per_level.shape[1]
        A = Ax4 // 4
        C = AxC // A
        box_cls_flattened.append(permute_and_flatten(box_cls_per_level, N, A, C, H, W))
        box_regression_flattened.append(permute_and_flatten(box_regression_per_level, N, A, 4, H, W))
    box_cls = torch.cat(box_cls_flattened, dim=1).flatten(0, -2)
    box_regression = torch.cat(box_regression_flattened, dim=1).reshape(-1, 4)
    return box_cls, box_regression


def clip_boxes_to_image(boxes, size):
    dim = boxes.dim()
    boxes_x = boxes[..., 0::2]
    boxes_y = boxes[..., 1::2]
    height, width = size
    boxes_x = boxes_x.clamp(min=0, max=width)
    boxes_y = boxes_y.clamp(min=0, max=height)
    clipped_boxes = torch.stack((boxes_x, boxes_y), dim=dim)
    return clipped_boxes.reshape(boxes.shape)


def remove_small_boxes(boxes, min_size):
    ws, hs = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    keep = (ws >= min_size) & (hs >= min_size)
    return torch.where(keep)[0]


def batched_nms(boxes, scores, idxs, iou_threshold):
    """ops/boxes.py _batched_nms_coordinate_trick with tests/_detect_ref.nms_ref as the kernel."""
    if boxes.numel() == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    max_coordinate = boxes.max()
    offsets = idxs.to(boxes) * (max_coordinate + torch.tensor(1).to(boxes))
    boxes_for_nms = boxes + offsets[:, None]
    return nms(boxes_for_nms, scores, iou_threshold)


def nms(boxes, scores, iou_threshold):
    """The nms under batched_nms: the reference's CPU kernel restated (tests/_detect_ref.py).  tools/perf_rpn.py, which runs the
    replica on a GPU, puts a torch composition in its place."""
    return torch.from_numpy(D.nms_ref(boxes.numpy(), scores.numpy(), iou_threshold))


class RegionProposalNetwork(nn.Module):
    """rpn.py:113-388, the inference path (no matcher, sampler or losses); `numerics` picks (a) or (b)."""

    def __init__(self, anchor_generator, head, fg_iou_thresh, bg_iou_thresh, batch_size_per_image, positive_fraction, pre_nms_top_n,
                 post_nms_top_n, nms_thresh, score_thresh=0.0, numerics=REPLICA):
        super().__init__()
        self.anchor_generator = anchor_generator
        self.head = head
        self.numerics = numerics
        self.box_coder = BoxCoder(weights=(1.0, 1.0, 1.0, 1.0), numerics=numerics)
        self._pre_nms_top_n = pre_nms_top_n
        self._post_nms_top_n = post_nms_top_n
        self.nms_thresh = nms_thresh
        self.score_thresh = score_thresh
        self.min_size = 1e-3

    def pre_nms_top_n(self):
        return self._pre_nms_top_n["training" if self.training else "testing"]

    def post_nms_top_n(self):
        return self._post_nms_top_n["training" if self.training else "testing"]

    def _get_top_n_idx(self, objectness, num_anchors_per_level):
        r = []
        offset = 0
        for ob in objectness.split(num_anchors_per_level, 1):
            num_anchors = ob.shape[1]
            pre_nms_top_n = min(self.pre_nms_top_n(), num_anchors)
            top_n_idx = self.numerics.topk(ob, pre_nms_top_n)
            r.append(top_n_idx + offset)
            offset += num_anchors
        return torch.cat(r, dim=1)

    def select(self, proposals, objectness, image_shapes, num_anchors_per_level):
        """filter_proposals up to the per-image filters -> dict of idx (N, K), boxes (N, K, 4) clipped, scores (N, K), levels (N, K),
        valid (N, K): what mv_rpn_topk_f32 + mv_rpn_decode_f32 write."""
        num_images = proposals.shape[0]
        objectness = objectness.detach().reshape(num_images, -1)
        device = proposals.device
        levels = [torch.full((n,), idx, dtype=torch.int64, device=device) for idx, n in enumerate(num_anchors_per_level)]
        levels = torch.cat(levels, 0).reshape(1, -1).expand_as(objectness)
        top_n_idx = self._get_top_n_idx(objectness, num_anchors_per_level)
        batch_idx = torch.arange(num_images, device=device)[:, None]
        objectness = objectness[batch_idx, top_n_idx]
        levels = levels[batch_idx, top_n_idx]
        proposals = proposals[batch_idx, top_n_idx]
        scores = self.numerics.sigmoid(objectness)
        boxes = torch.stack([clip_boxes_to_image(b, s) for b, s in zip(proposals, image_shapes)])
        ws, hs = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
        valid = (ws >= self.min_size) & (hs >= self.min_size) & (scores >= self.score_thresh)
        return {"idx": top_n_idx, "boxes": boxes, "scores": scores, "levels": levels, "valid": valid}

    def filter_proposals(self, proposals, objectness, image_shapes, num_anchors_per_level):
        s = self.select(proposals, objectness, image_shapes, num_anchors_per_level)
        final_boxes, final_scores = [], []
        for boxes, scores, lvl in zip(s["boxes"], s["scores"], s["levels"]):
            # remove small boxes
            keep = remove_small_boxes(boxes, self.min_size)
            boxes, scores, lvl = boxes[keep], scores[keep], lvl[keep]
            # remove low scoring boxes
            keep = torch.where(scores >= self.score_thresh)[0]
            boxes, scores, lvl = boxes[keep], scores[keep], lvl[keep]
            # non-maximum suppression, independently done per level
            keep = batched_nms(boxes, scores, lvl, self.nms_thresh)
            # keep only topk scoring predictions
            keep = keep[:self.post_nms_top_n()]
            final_boxes.append(boxes[keep])
            final_scores.append(scores[keep])
        return final_boxes, final_scores

    def from_head_outputs(self, images, objectness, pred_bbox_deltas, detailed=False):
        """forward from the head's per-level outputs on (CPU tensors) -> (boxes, scores), or select()'s dict."""
        anchors = self.anchor_generator(images, objectness)
        num_images = len(anchors)
        num_anchors_per_level = [int(o[0].numel()) for o in objectness]
        objectness, pred_bbox_deltas = concat_box_prediction_layers(objectness, pred_bbox_deltas)
        proposals = self.box_coder.decode(pred_bbox_deltas.detach(), anchors)
        proposals = proposals.view(num_images, -1, 4)
        if detailed:
            return self.select(proposals, objectness, images.image_sizes, num_anchors_per_level)
        return self.filter_proposals(proposals, objectness, images.image_sizes, num_anchors_per_level)

    def forward(self, images, features, targets=None):
        features = list(features.values())
        objectness, pred_bbox_deltas = self.head(features)
        boxes, _ = self.from_head_outputs(images, objectness, pred_bbox_deltas)
        return boxes, {}


# ------------------------------------------------------------------------------------------------ helpers of the tests
FPN_SIZES = ((32,), (64,), (128,), (256,), (512,))
FPN_RATIOS = ((0.5, 1.0, 2.0),) * 5


def ulp_distance(a, b):
    """|a - b| in units of the last place of float32 tensors of equal sign (integer distance of the bit patterns)."""
    ia, ib = a.contiguous().view(torch.int32).to(torch.int64), b.contiguous().view(torch.int32).to(torch.int64)
    return (ia - ib).abs()


def same(got, want, what=""):
    """NaN in equal places, == elsewhere (-0 equals +0), same shape and dtype."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(got.numpy(), want.numpy(), err_msg=what)
