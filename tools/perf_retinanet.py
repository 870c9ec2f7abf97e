#!/usr/bin/env python3
"""RetinaNet inference on one MI355X against the torch replica of the reference (tests/_retinanet_ref.py) on the same GPU, fp32.

Shapes: ResNet-50-FPN (layer2 .. layer4 + P6, P7) on an 800 x 1333 image -- five 256-channel levels of 100 x 167, 50 x 84, 25 x 42,
13 x 21 and 7 x 11 -- 9 anchors, 91 classes, score_thresh 0.05, 1000 candidates per level, nms 0.5, 300 detections per image, at
batch 1 and batch 8.  The class logits of level l are N(-6, std_l^2) with std_l chosen so that about 3000 candidates of every level
pass the threshold (the counts are printed and stored).  Rows, every reference fed the library's own outputs of the stage before:

  retinanet_topk    F.retinanet_topk, all levels and images in one call | per image and level: permute + reshape of the map,
                    sigmoid, `> thresh`, torch.where, topk (the replica's postprocess_detections up to the decode)
  level 0 alone     F.retinanet_topk on level 0 only, stage 1 + stage 2 (many workgroups per image) | the library's own stage 2
                    run directly on the map, ONE workgroup per (image, level) (MV_RETINANET_ONE_WORKGROUP=1, a knob of the
                    -DMV_TUNING library, which is the library this tool loads); the two index tensors are compared
  retinanet_decode  F.retinanet_decode | the replica's divide, modulo, gathers, decode_single and clip on its own anchors
  head              RetinaNetHead.forward (NCHW maps) | the replica's head (torch convs, permuted and concatenated)
  forward           RetinaNet.forward | the replica's forward; BOTH sides run the package's backbone and ops.nms

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON.

  python tools/perf_retinanet.py [--batches 1 8] [--iters 5] [--out profiles/perf_retinanet.json]
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
from tests import _retinanet_ref as R  # noqa: E402  (the torch replica of the reference's modules)
from tests import _rpn_ref as P  # noqa: E402
from tools.perf_detect import alternate  # noqa: E402

GRIDS = [(100, 167), (50, 84), (25, 42), (13, 21), (7, 11)]
PADDED = (800, 1344)
ANCHORS, CLASSES, TOPK, THRESH, PASSING = 9, 91, 1000, 0.05, 3000


def replica_select(cls_maps):
    """The replica's postprocess_detections up to the decode -> per image and level (flat indices, scores)."""
    out = []
    flat = [R.permute_level(m, CLASSES) for m in cls_maps]
    for i in range(cls_maps[0].shape[0]):
        per_level = []
        for level in flat:
            scores = torch.sigmoid(level[i]).flatten()
            keep = scores > THRESH
            scores = scores[keep]
            idxs = torch.where(keep)[0]
            scores, order = scores.topk(min(idxs.size(0), TOPK))
            per_level.append((idxs[order], scores))
        out.append(per_level)
    return out


def replica_decode(coder, selected, reg_maps, anchors, sizes):
    flat = [R.permute_level(m, 4) for m in reg_maps]
    out = []
    for i, per_level in enumerate(selected):
        boxes = []
        for (idxs, _), reg, anc in zip(per_level, flat, anchors[i]):
            a = torch.div(idxs, CLASSES, rounding_mode="floor")
            labels = idxs % CLASSES  # noqa: F841
            boxes.append(P.clip_boxes_to_image(coder.decode_single(reg[i][a], anc[a]), sizes[i]))
        out.append(torch.cat(boxes))
    return out


def rows_for(n, iters):
    g = torch.Generator(device="cuda").manual_seed(3 + n)
    # N(-6, std_l^2) with std_l such that about 3000 candidates of level l pass the threshold (logit(0.05) = -2.944)
    normal = torch.distributions.Normal(0.0, 1.0)
    stds = [3.056 / float(normal.icdf(torch.tensor(1.0 - PASSING / (ANCHORS * CLASSES * h * w)))) for h, w in GRIDS]
    cls = [torch.randn((n, ANCHORS * CLASSES, h, w), device="cuda", generator=g) * sd - 6 for (h, w), sd in zip(GRIDS, stds)]
    reg = [torch.randn((n, 4 * ANCHORS, h, w), device="cuda", generator=g) * 0.5 for h, w in GRIDS]
    sizes = [(800, 1333 - 16 * (i % 2)) for i in range(n)]
    strides = [(PADDED[0] // h, PADDED[1] // w) for h, w in GRIDS]
    ag = R.default_anchorgen()
    passing = [[int((torch.sigmoid(m[i]) > THRESH).sum()) for m in cls] for i in range(n)]
    print(f"batch {n}: candidates passing {THRESH} per level, image 0: {passing[0]}", flush=True)
    with torch.no_grad():
        topk = lambda: F.retinanet_topk(cls, CLASSES, TOPK, THRESH)  # noqa: E731
        idx = topk()
        sel = replica_select(cls)
        same = all(set(idx[i][idx[i] >= 0].tolist()) ==
                   set(torch.cat([f + s * CLASSES for (f, _), s in zip(sel[i], _starts())]).tolist()) for i in range(min(n, 2)))
        ms, ms_t = alternate([topk, lambda: replica_select(cls)], iters)
        yield dict(what="retinanet_topk 5 levels", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_retinanet_chunks + k_retinanet_rank",
                   passing=passing[0], same_index_sets_as_torch=same)
        one = lambda: F.retinanet_topk(cls[:1], CLASSES, TOPK, THRESH)  # noqa: E731

        def single():  # the knob is read at every launch
            os.environ["MV_RETINANET_ONE_WORKGROUP"] = "1"
            try:
                return F.retinanet_topk(cls[:1], CLASSES, TOPK, THRESH)
            finally:
                del os.environ["MV_RETINANET_ONE_WORKGROUP"]
        equal = bool(torch.equal(one(), single()))
        ms, ms_t = alternate([one, single], max(1, iters // 2))
        yield dict(what="level 0 alone: stage 1 + stage 2 | stage 2 on the map, one workgroup per image", batch=n, ours_ms=ms, torch_ms=ms_t,
                   equal_indices=equal)
        anchors_flat = ag(P.ImageList(torch.zeros((n, 3) + PADDED, device="cuda"), sizes), cls)
        per_level = [ANCHORS * h * w for h, w in GRIDS]
        anchors = [list(a.split(per_level)) for a in anchors_flat]
        coder = P.BoxCoder((1.0, 1.0, 1.0, 1.0))
        cells = [c.cuda() for c in ag.cell_anchors]
        decode = lambda: F.retinanet_decode(cls, reg, idx, cells, strides, sizes, CLASSES)  # noqa: E731
        boxes, scores, labels, valid = decode()
        ms, ms_t = alternate([decode, lambda: replica_decode(coder, sel, reg, anchors, sizes)], iters)
        yield dict(what=f"retinanet_decode {idx.shape[1]} candidates per image", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_retinanet_decode",
                   valid=int(valid.sum()))
        # the head and the whole model
        torch.manual_seed(0)
        model = mv.retinanet_resnet50_fpn(_skip_resize=True)
        gen = torch.Generator().manual_seed(1)
        for p in model.head.parameters():  # std 0.03 keeps the towers' activations at the scale of their input (0.01 shrinks them)
            p.copy_(torch.randn(p.shape, generator=gen) * 0.03)
        model = model.cuda()
        replica_head = R.RetinaNetHead(256, ANCHORS, CLASSES).eval()
        replica_head.load_state_dict(model.head.state_dict(), strict=True)
        replica_head = replica_head.cuda()
        feats = [torch.rand((n, 256, h, w), device="cuda", generator=g) * 2 - 1 for h, w in GRIDS]
        out = model.head(feats)
        out_t = replica_head(feats)
        diff = float((mv.retinanet.concat_layout(out["cls_logits"], CLASSES) - out_t["cls_logits"]).abs().max())
        ms, ms_t = alternate([lambda: model.head(feats), lambda: replica_head(feats)], max(1, iters // 2))
        yield dict(what="RetinaNetHead 256 channels, 5 levels", batch=n, ours_ms=ms, torch_ms=ms_t, max_abs_diff_vs_torch=diff)
        P.nms = ops.nms  # the replica's nms is a numpy restatement: both sides run the package's kernel
        replica = R.RetinaNet(model.backbone, CLASSES, head=replica_head, anchor_generator=ag).eval()
        del replica.transform
        replica.transform = lambda images: model.transform(images, None)[0]
        images = [torch.rand((3,) + s, device="cuda", generator=g) for s in sizes]
        # a trained model's scores: the bias is shifted so that about 3000 candidates of level 0 pass
        level0 = model.head(list(model.backbone(model.transform(images, None)[0].tensors).values()))["cls_logits"][0][0].flatten()
        q = float(level0.kthvalue(level0.numel() - PASSING)[0])
        for head in (model.head.classification_head, replica_head.classification_head):
            head.cls_logits.bias.add_(-2.944 - q)
        got, want = model(images), replica(images)
        ms, ms_t = alternate([lambda: model(images), lambda: replica(images)], max(1, iters // 2))
        yield dict(what="RetinaNet.forward resnet50 fpn", batch=n, ours_ms=ms, torch_ms=ms_t, detections=[len(d["boxes"]) for d in got],
                   torch_detections=[len(d["boxes"]) for d in want])


def _starts():
    s, out = 0, []
    for h, w in GRIDS:
        out.append(s)
        s += ANCHORS * h * w
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="profiles/perf_retinanet.json")
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
