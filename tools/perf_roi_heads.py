#!/usr/bin/env python3
"""RoIHeads inference on one MI355X against the torch replica of the reference (tests/_roi_heads_ref.py) on the same GPU, fp32.

Shapes: ResNet-50-FPN on an 800 x 800 image -- four 256-channel levels of 200, 100, 50 and 25 pixels a side -- 1000 proposals per
image, 91 classes, box_score_thresh 0.05, nms 0.5, 100 detections per image, at batch 1 and batch 8.  Rows:

  pooler          MultiScaleRoIAlign, one launch | the reference's per-level loop (torch.where, gather, roi_align, scatter); BOTH sides
                  run the package's ops.roi_align kernel (torch has none of its own: the comparison is of the loop around it)
  TwoMLPHead      two F.linear_bias_relu launches | nn.Linear + relu twice
  predictor       cls_score and bbox_pred as one linear launch | two nn.Linear
  roi_detections  F.roi_detections, one launch | softmax, BoxCoder.decode, clip, the three slices and reshapes, the score and
                  small-box filters per image (the replica's postprocess_detections up to the nms)
  forward         RoIHeads.forward | the replica's forward; BOTH sides run the package's ops.nms and ops.roi_align

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON.

  python tools/perf_roi_heads.py [--batches 1 8] [--iters 5] [--out profiles/perf_roi_heads.json]
"""
import argparse
import json
import sys
from collections import OrderedDict
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd import ops  # noqa: E402
from tests import _roi_heads_ref as H  # noqa: E402  (the torch replica of the reference's modules)
from tests import _rpn_ref as P  # noqa: E402
from tools.perf_detect import alternate  # noqa: E402

SIDES = [200, 100, 50, 25]
IMAGE, PROPOSALS, CLASSES = 800, 1000, 91
THRESH, NMS, DETECTIONS = 0.05, 0.5, 100


class LoopPooler(torch.nn.Module):
    """ops/poolers.py _multiscale_roi_align: the reference's loop over the levels around the package's roi_align."""

    def __init__(self, pooler):
        super().__init__()
        self.pooler = pooler

    def forward(self, x, boxes, image_shapes):
        feats = [v for k, v in x.items() if k in self.pooler.featmap_names]
        rois = ops._convert_to_roi_format(boxes)
        levels = self.pooler.map_levels(boxes)
        result = torch.zeros((len(rois), feats[0].shape[1]) + self.pooler.output_size, dtype=feats[0].dtype, device=feats[0].device)
        for level, (feature, scale) in enumerate(zip(feats, self.pooler.scales)):
            idx = torch.where(levels == level)[0]
            result[idx] = ops.roi_align(feature, rois[idx], self.pooler.output_size, scale, self.pooler.sampling_ratio)
        return result


def replica_filters(heads, class_logits, box_regression, proposals, image_shapes):
    """The replica's postprocess_detections up to the nms."""
    num_classes = class_logits.shape[-1]
    boxes_per_image = [len(p) for p in proposals]
    pred_boxes = heads.box_coder.decode(box_regression, proposals)
    pred_scores = torch.softmax(class_logits, -1)
    out = []
    for boxes, scores, image_shape in zip(pred_boxes.split(boxes_per_image, 0), pred_scores.split(boxes_per_image, 0), image_shapes):
        boxes = P.clip_boxes_to_image(boxes, image_shape)
        labels = torch.arange(num_classes, device=boxes.device).view(1, -1).expand_as(scores)
        boxes, scores, labels = boxes[:, 1:].reshape(-1, 4), scores[:, 1:].reshape(-1), labels[:, 1:].reshape(-1)
        inds = torch.where(scores > heads.score_thresh)[0]
        boxes, scores, labels = boxes[inds], scores[inds], labels[inds]
        keep = P.remove_small_boxes(boxes, 1e-2)
        out.append((boxes[keep], scores[keep], labels[keep]))
    return out


def build_pair():
    torch.manual_seed(0)
    replica_head, replica_pred = H.TwoMLPHead(256 * 49, 1024).eval(), H.FastRCNNPredictor(1024, CLASSES).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in replica_pred.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    head, pred = mv.TwoMLPHead(256 * 49, 1024), mv.FastRCNNPredictor(1024, CLASSES)
    head.load_state_dict(replica_head.state_dict(), strict=True)
    pred.load_state_dict(replica_pred.state_dict(), strict=True)
    pooler = mv.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    args = (0.5, 0.5, 512, 0.25, None, THRESH, NMS, DETECTIONS)
    ours = mv.RoIHeads(pooler, head, pred, *args).cuda()
    replica = H.RoIHeads(LoopPooler(pooler), replica_head, replica_pred, *args).cuda().eval()
    return ours, replica


def rows_for(n, iters):
    ours, replica = build_pair()
    g = torch.Generator().manual_seed(2 + n)
    feats = OrderedDict((str(i), torch.rand((n, 256, s, s), device="cuda") * 2 - 1) for i, s in enumerate(SIDES))
    feats["pool"] = torch.zeros((n, 256, 13, 13), device="cuda")
    sizes = [(IMAGE, IMAGE - 16 * (i % 2)) for i in range(n)]
    proposals = []
    for _ in range(n):  # sides of 16 .. 512 pixels, log-uniform: every level gets its share
        side = 16 * 2 ** (torch.rand((PROPOSALS, 2), generator=g) * 5)
        p = torch.rand((PROPOSALS, 2), generator=g) * (IMAGE - side).clamp(min=1)
        proposals.append(torch.cat([p, (p + side).clamp(max=IMAGE)], 1).cuda())
    P.nms = ops.nms  # the replica's nms is a numpy restatement: both sides run the package's kernel
    with torch.no_grad():
        pooled = ours.box_roi_pool(feats, proposals, sizes)
        pooled_t = replica.box_roi_pool(feats, proposals, sizes)
        ms, ms_t = alternate([lambda: ours.box_roi_pool(feats, proposals, sizes), lambda: replica.box_roi_pool(feats, proposals, sizes)], iters)
        yield dict(what=f"pooler {n * PROPOSALS} rois", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_multiscale_roi_align",
                   max_abs_diff_vs_torch=float((pooled - pooled_t).abs().max()))
        hidden, hidden_t = ours.box_head(pooled), replica.box_head(pooled)
        ms, ms_t = alternate([lambda: ours.box_head(pooled), lambda: replica.box_head(pooled)], iters)
        yield dict(what="TwoMLPHead 12544 -> 1024 -> 1024", batch=n, ours_ms=ms, torch_ms=ms_t,
                   max_abs_diff_vs_torch=float((hidden - hidden_t).abs().max()))
        # class logits of a few units, as a trained model's: a few classes per roi pass the threshold (random weights leave none)
        scale = 2.0 / float(ours.box_predictor(hidden)[0].std())
        for module in (ours.box_predictor, replica.box_predictor):
            module.cls_score.weight.mul_(scale), module.cls_score.bias.mul_(scale)
        logits, reg = ours.box_predictor(hidden)
        logits_t, reg_t = replica.box_predictor(hidden)
        ms, ms_t = alternate([lambda: ours.box_predictor(hidden), lambda: replica.box_predictor(hidden)], iters)
        yield dict(what=f"predictor 1024 -> {5 * CLASSES}", batch=n, ours_ms=ms, torch_ms=ms_t,
                   max_abs_diff_vs_torch=max(float((logits - logits_t).abs().max()), float((reg - reg_t).abs().max())))
        rois = ops._convert_to_roi_format(proposals)
        coder = ours.box_coder
        detect = lambda: F.roi_detections(logits, reg, rois, sizes, coder.weights, coder.bbox_xform_clip, THRESH, 1e-2)  # noqa: E731
        boxes, scores, labels, valid = detect()
        kept_t = replica_filters(replica, logits_t, reg_t, proposals, sizes)
        ms, ms_t = alternate([detect, lambda: replica_filters(replica, logits_t, reg_t, proposals, sizes)], iters)
        yield dict(what=f"roi_detections {n * PROPOSALS} rois x {CLASSES} classes", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_roi_detections",
                   valid=int(valid.sum()), torch_kept=sum(len(k[0]) for k in kept_t),
                   max_score_diff_vs_torch=float((scores - torch.softmax(logits_t, -1)[:, 1:]).abs().max()))
        got, _ = ours(feats, proposals, sizes)
        want, _ = replica(feats, proposals, sizes)
        ms, ms_t = alternate([lambda: ours(feats, proposals, sizes), lambda: replica(feats, proposals, sizes)], max(1, iters // 2))
        yield dict(what="RoIHeads.forward", batch=n, ours_ms=ms, torch_ms=ms_t, detections=[len(d["boxes"]) for d in got],
                   torch_detections=[len(d["boxes"]) for d in want])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="profiles/perf_roi_heads.json")
    a = ap.parse_args()
    rows = []
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for n in a.batches:
        for row in rows_for(n, a.iters):
            rows.append(row)  # the series is kept row by row: a later shape that runs out of time loses nothing
            Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=7, rows=rows), indent=1) + "\n")
            print(f"batch {row['batch']} {row['what']}: {row['ours_ms']:8.3f} ms | {row['torch_ms']:8.3f} ms ({row['torch_ms'] / row['ours_ms']:5.2f}x)",
                  flush=True)


if __name__ == "__main__":
    main()
