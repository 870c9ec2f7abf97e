#!/usr/bin/env python3
"""FCOS inference on one MI355X against torch and the torch replica of the reference (tests/_fcos_ref.py) on the same GPU, fp32.

Shapes: ResNet-50-FPN (layer2 .. layer4 + P6, P7) on an 800 x 1344 input -- five 256-channel levels of 100 x 168, 50 x 84, 25 x 42,
13 x 21 and 7 x 11 -- one anchor, 91 classes, GroupNorm(32, 256), score_thresh 0.2, 1000 candidates per level, nms 0.6, 100 detections
per image, at batch 1 and batch 8.  Rows, every reference fed the library's own outputs of the stage before:

  group_norm_act    F.group_norm_act(relu=True) per level | torch.nn.functional.group_norm + relu.  GB/s: the 3 x 4 bytes per element the
                    two-launch form moves (x read twice, y written once) over the time
  head              FCOSHead.forward (NCHW maps) | the replica's head (torch convs, nn.GroupNorm, permuted and concatenated)
  candidates        F.fcos_topk + F.fcos_decode, all levels and images in two calls | the replica's postprocess_detections up to the nms
                    per image and level (sigmoids, sqrt, `> thresh`, torch.where, topk, gathers, BoxLinearCoder.decode, clip)
  forward           FCOS.forward | the replica's forward; BOTH sides run the package's backbone and ops.nms

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON.

  python tools/perf_fcos.py [--batches 1 8] [--iters 5] [--out profiles/perf_fcos.json]
"""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
os.environ.setdefault("MI355VISION_LIB", str(ROOT / "cpu-vision_amd" / "lib" / "libmi355vision_tuning.so"))
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd import ops  # noqa: E402
from tests import _fcos_ref as R  # noqa: E402  (the torch replica of the reference's modules)
from tests import _rpn_ref as P  # noqa: E402
from tools.perf_detect import alternate  # noqa: E402

GRIDS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
PADDED = (800, 1344)
CLASSES, TOPK, THRESH, PASSING = 91, 1000, 0.2, 3000


def replica_candidates(model, cls, reg, ctr, anchors, sizes):
    """The replica's postprocess_detections up to the nms on the NCHW maps."""
    head_outputs = {"cls_logits": [R.permute_level(m, CLASSES) for m in cls], "bbox_regression": [R.permute_level(m, 4) for m in reg],
                    "bbox_ctrness": [R.permute_level(m, 1) for m in ctr]}
    saved = model.nms_thresh
    model.nms_thresh = 2.0  # nothing is suppressed: the nms is not part of this row
    try:
        return model.postprocess_detections(head_outputs, anchors, sizes)
    finally:
        model.nms_thresh = saved


def rows_for(n, iters):
    g = torch.Generator(device="cuda").manual_seed(5 + n)
    with torch.no_grad():
        gamma, beta = torch.rand(256, device="cuda", generator=g) + 0.5, torch.randn(256, device="cuda", generator=g) * 0.1
        for h, w in GRIDS:
            x = torch.randn((n, 256, h, w), device="cuda", generator=g) * 2 + 0.3
            ours = lambda: F.group_norm_act(x, 32, gamma, beta, 1e-5, relu=True)  # noqa: E731
            theirs = lambda: torch.relu(torch.nn.functional.group_norm(x, 32, gamma, beta, 1e-5))  # noqa: E731
            diff = float((ours() - theirs()).abs().max())
            ms, ms_t = alternate([ours, theirs], iters)
            yield dict(what=f"group_norm_act relu 256 x {h} x {w}, 32 groups", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_gn_stats + k_gn_apply",
                       gb_per_s=12.0 * x.numel() / (ms * 1e-3) / 1e9, max_abs_diff_vs_torch=diff)
        # the head and the whole model
        torch.manual_seed(0)
        model = mv.fcos_resnet50_fpn(_skip_resize=True)
        gen = torch.Generator().manual_seed(1)
        for p in model.head.parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.03)
        model = model.cuda()
        replica_head = R.FCOSHead(256, 1, CLASSES).eval()
        replica_head.load_state_dict(model.head.state_dict(), strict=True)
        replica_head = replica_head.cuda()
        feats = [torch.rand((n, 256, h, w), device="cuda", generator=g) * 2 - 1 for h, w in GRIDS]
        out = model.head(feats)
        out_t = replica_head(feats)
        diff = float((mv.retinanet.concat_layout(out["cls_logits"], CLASSES) - out_t["cls_logits"]).abs().max())
        ms, ms_t = alternate([lambda: model.head(feats), lambda: replica_head(feats)], max(1, iters // 2))
        yield dict(what="FCOSHead 256 channels, 5 levels", batch=n, ours_ms=ms, torch_ms=ms_t, max_abs_diff_vs_torch=diff)
        # candidates: class logits N(-6, std_l^2), the centerness N(0, 1): 3000 (P7) to 21 000 (P3) candidates per level pass (stored)
        normal = torch.distributions.Normal(0.0, 1.0)
        stds = [4.6 / float(normal.icdf(torch.tensor(1.0 - PASSING / (CLASSES * h * w)))) for h, w in GRIDS]
        cls = [torch.randn((n, CLASSES, h, w), device="cuda", generator=g) * sd - 6 for (h, w), sd in zip(GRIDS, stds)]
        ctr = [torch.randn((n, 1, h, w), device="cuda", generator=g) for h, w in GRIDS]
        reg = [torch.rand((n, 4, h, w), device="cuda", generator=g) * 2 for h, w in GRIDS]
        sizes = [(800, 1333 - 16 * (i % 2)) for i in range(n)]
        strides = [(PADDED[0] // h, PADDED[1] // w) for h, w in GRIDS]
        ag = R.default_anchorgen()
        cells = [c.cuda() for c in ag.cell_anchors]
        anchors_flat = ag(P.ImageList(torch.zeros((n, 3) + PADDED, device="cuda"), sizes), cls)
        anchors = [list(a.split([h * w for h, w in GRIDS])) for a in anchors_flat]
        P.nms = ops.nms  # the replica's nms is a numpy restatement: both sides run the package's kernel
        replica = R.FCOS(model.backbone, CLASSES, head=replica_head, anchor_generator=ag).eval()

        def ours():
            idx = F.fcos_topk(cls, ctr, CLASSES, TOPK, THRESH)
            return idx, F.fcos_decode(cls, ctr, reg, idx, cells, strides, sizes, CLASSES)
        idx, (_, _, _, valid) = ours()
        theirs = lambda: replica_candidates(replica, cls, reg, ctr, anchors, sizes)  # noqa: E731
        passing = [int((R.level_scores(m[:1], c[:1], CLASSES) > THRESH).sum()) for m, c in zip(cls, ctr)]
        ms, ms_t = alternate([ours, theirs], iters)
        yield dict(what=f"candidates: fcos_topk + fcos_decode, {idx.shape[1]} per image", batch=n, ours_ms=ms, torch_ms=ms_t,
                   kernel="k_retinanet_chunks<fcos> + k_retinanet_rank + k_fcos_decode", passing=passing, valid=int(valid.sum()))
        del replica.transform
        replica.transform = lambda images: model.transform(images, None)[0]
        images = [torch.rand((3,) + s, device="cuda", generator=g) for s in sizes]
        # a trained model's scores: the bias is shifted so that about 3000 candidates of level 0 pass at a centerness of 0
        level0 = model.head(list(model.backbone(model.transform(images, None)[0].tensors).values()))["cls_logits"][0][0].flatten()
        q = float(level0.kthvalue(level0.numel() - PASSING)[0])
        for head in (model.head.classification_head, replica_head.classification_head):
            head.cls_logits.bias.add_(-2.44 - q)
        got, want = model(images), replica(images)
        ms, ms_t = alternate([lambda: model(images), lambda: replica(images)], max(1, iters // 2))
        yield dict(what="FCOS.forward resnet50 fpn", batch=n, ours_ms=ms, torch_ms=ms_t, detections=[len(d["boxes"]) for d in got],
                   torch_detections=[len(d["boxes"]) for d in want])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="profiles/perf_fcos.json")
    a = ap.parse_args()
    rows = []
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for n in a.batches:
        for row in rows_for(n, a.iters):
            rows.append(row)  # the series is kept row by row: a later shape that runs out of time loses nothing
            Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=7, rows=rows), indent=1) + "\n")
            extra = f" {row['gb_per_s']:7.0f} GB/s" if "gb_per_s" in row else ""
            print(f"batch {row['batch']} {row['what']}: {row['ours_ms']:8.3f} ms | {row['torch_ms']:8.3f} ms ({row['torch_ms'] / row['ours_ms']:5.2f}x){extra}",
                  flush=True)


if __name__ == "__main__":
    main()
