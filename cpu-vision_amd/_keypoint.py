"""The keypoint branch of Keypoint R-CNN behind the keypoint head: heatmaps_to_keypoints (models/detection/roi_heads.py) as ONE launch
(csrc/keypoint.hip) and the ConvTranspose2d(kernel 4, stride 2, padding 1) geometry of conv_transpose2d_bias_act (keypoint_rcnn.py's
kps_score_lowres; csrc/conv_igemm.hip's transposed store).  Arithmetic in mi355vision.h, mv_heatmaps_to_keypoints_f32 and
mv_conv_transpose4x4s2_bias_act_f32.

Every name here is re-exported by `functional`, which is where the rest of the package, the tests and tools/ find it.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

MAX_HEATMAP_ELEMENTS = 16384  # mv_heatmaps_to_keypoints_f32 stages a heatmap in LDS


def heatmaps_to_keypoints(maps: torch.Tensor, rois: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """roi_heads.py heatmaps_to_keypoints: maps (R, K, Mh, Mw) float32 and rois (R, 4) float32 on the device -> (xy_preds (R, K, 3),
    end_scores (R, K)): per roi and keypoint the first maximum of the heatmap resized (bicubic) to the roi's (ceil(h), ceil(w)),
    as image coordinates (x, y, 1) and its value.  ONE launch; the resized maps are never materialised, the rois are read on the
    device and nothing is read back.  Numerics and domain: mi355vision.h, mv_heatmaps_to_keypoints_f32 (a roi with a non-finite
    coordinate or a side above 2^15 gives a zero row where the reference fails)."""
    if maps.dim() != 4:
        raise ValueError(f"heatmaps_to_keypoints: maps are expected to have the shape [R, K, Mh, Mw], got {list(maps.shape)}")
    if rois.dim() != 2 or rois.shape[1] != 4 or rois.shape[0] != maps.shape[0]:
        raise ValueError(f"heatmaps_to_keypoints: rois are expected to have the shape [{maps.shape[0]}, 4], got {list(rois.shape)}")
    if maps.dtype != torch.float32 or rois.dtype != torch.float32:
        raise TypeError(f"heatmaps_to_keypoints computes in float32. Got maps {maps.dtype}, rois {rois.dtype}")
    r, k, mh, mw = (int(s) for s in maps.shape)
    if k < 1 or mh < 1 or mw < 1:
        raise ValueError(f"heatmaps_to_keypoints: maps of shape {list(maps.shape)}: keypoints and sizes should be positive")
    if mh * mw > MAX_HEATMAP_ELEMENTS:
        raise NotImplementedError(f"heatmaps_to_keypoints: heatmaps of ({mh}, {mw}) are not on the MI355X path (up to "
                                  f"{MAX_HEATMAP_ELEMENTS} elements are)")
    _lib.require_device(maps, "maps")
    _lib.require_device(rois, "rois")
    if rois.device != maps.device:
        raise ValueError("heatmaps_to_keypoints: maps and rois must live on one device")
    xy = torch.empty((r, k, 3), dtype=torch.float32, device=maps.device)
    scores = torch.empty((r, k), dtype=torch.float32, device=maps.device)
    if r == 0:
        return xy, scores
    mc, rc = maps.detach().contiguous(), rois.detach().contiguous()
    _lib.launch(_lib.load().mv_heatmaps_to_keypoints_f32, mc, mc.data_ptr(), rc.data_ptr(), xy.data_ptr(), scores.data_ptr(), r, k, mh, mw)
    return _lib.forward_only(xy, "heatmaps_to_keypoints", maps, rois), _lib.forward_only(scores, "heatmaps_to_keypoints", maps, rois)


def conv_transpose4x4_relayout(weight: torch.Tensor, bias: Optional[torch.Tensor], device) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """torch's ConvTranspose2d weight (cin, cout, 4, 4) and bias (cout) as what mv_conv_transpose4x4s2_bias_act_f32 takes: the weight
    of the equivalent 2x2 convolution, (4 cout, cin, 2, 2) with w2[4 co + 2 py + px, ci, ty, tx] = weight[ci, co, 3 - py - 2 ty,
    3 - px - 2 tx], and the bias with every entry repeated four times -- float32, contiguous, on `device`.  A module calls this once
    per parameter version (KeypointRCNNPredictor.relaid)."""
    cin, cout = int(weight.shape[0]), int(weight.shape[1])
    with torch.no_grad():
        w = weight.detach().to(device, torch.float32)
        w2 = torch.empty((cout, 2, 2, cin, 2, 2), dtype=torch.float32, device=w.device)
        for py in range(2):
            for px in range(2):
                for ty in range(2):
                    for tx in range(2):
                        w2[:, py, px, :, ty, tx] = w[:, :, 3 - py - 2 * ty, 3 - px - 2 * tx].t()
        w2 = w2.reshape(4 * cout, cin, 2, 2).contiguous()
        b4 = None if bias is None else bias.detach().to(device, torch.float32).repeat_interleave(4).contiguous()
    return w2, b4


def conv_transpose4x4s2(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act_code: int,
                        relaid: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]]) -> torch.Tensor:
    """The launch of conv_transpose2d_bias_act (which has checked the arguments) for kernel 4, stride 2, padding 1."""
    n, cin, h, w = (int(d) for d in x.shape)
    cout = int(weight.shape[1])
    w2, b4 = relaid if relaid is not None else conv_transpose4x4_relayout(weight, bias, x.device)
    y = torch.empty((n, cout, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    if n == 0:
        return y
    xc = x.contiguous()
    _lib.launch(_lib.load().mv_conv_transpose4x4s2_bias_act_f32, xc, xc.data_ptr(), w2.data_ptr(), _lib.ptr(b4), y.data_ptr(), n, cin, h, w,
                cout, act_code)
    return y
