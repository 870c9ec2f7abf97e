#!/usr/bin/env python3
"""SSD inference on one MI355X against torch and the torch replica of the reference (tests/_ssd_ref.py) on the same GPU, fp32.

Shapes: ssd300_vgg16 -- six levels of 38, 19, 10, 5, 3 and 1 cells with 4, 6, 6, 6, 4, 4 default boxes (8 732 anchors), 91 classes,
score_thresh 0.01, 400 candidates per class, nms 0.45, 200 detections per image, at batch 1 and batch 8.  Rows, every reference fed
the library's own outputs of the stage before:

  l2_normalize_scale  F.l2_normalize_scale at (N, 512, 38, 38) | weight.view(1, -1, 1, 1) * torch.nn.functional.normalize(x).  GB/s: the
                      3 x 4 bytes per element the kernel moves (x read twice, the second time out of L2, y written once) over the time
  candidates          SSD.candidates: F.ssd_scores + F.ssd_topk + F.ssd_decode, all levels and images in three calls | the replica's
                      postprocess_detections up to the nms (softmax, decode and clip of all anchors, the loop over the 90 labels with
                      `> thresh`, topk and gathers)
  forward             SSD.forward | the replica's forward (torch convs and pools, its own transform); BOTH sides run the package's nms

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON.

  python tools/perf_ssd.py [--batches 1 8] [--iters 5] [--out profiles/perf_ssd.json]
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
from tests import _rpn_ref as P  # noqa: E402
from tests import _ssd_ref as R  # noqa: E402  (the torch replica of the reference's modules)
from tools.perf_detect import alternate  # noqa: E402

GRIDS = [38, 19, 10, 5, 3, 1]
ANCHORS = [4, 6, 6, 6, 4, 4]
CLASSES = 91


def rows_for(n, iters):
    g = torch.Generator(device="cuda").manual_seed(5 + n)
    with torch.no_grad():
        x = torch.randn((n, 512, 38, 38), device="cuda", generator=g).relu_() * 30
        w = torch.full((512,), 20.0, device="cuda")
        ours = lambda: F.l2_normalize_scale(x, w)  # noqa: E731
        theirs = lambda: w.view(1, -1, 1, 1) * torch.nn.functional.normalize(x)  # noqa: E731
        diff = float((ours() - theirs()).abs().max())
        ms, ms_t = alternate([ours, theirs], iters)
        yield dict(what="l2_normalize_scale 512 x 38 x 38", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_l2_normalize_scale",
                   gb_per_s=12.0 * x.numel() / (ms * 1e-3) / 1e9, max_abs_diff_vs_torch=diff)

        torch.manual_seed(0)
        model = mv.ssd300_vgg16()
        replica = R.ssd300_vgg16()
        replica.load_state_dict(model.state_dict(), strict=True)
        model, replica = model.cuda(), replica.eval().cuda()
        P.nms = ops.nms  # the replica's nms is a numpy restatement: both sides run the package's kernel
        # candidates: logits N(0, 2^2) with the background 4 higher, so that a few per cent of the (anchor, class) scores pass 0.01
        cls = [torch.randn((n, a * CLASSES, s, s), device="cuda", generator=g) * 2 for a, s in zip(ANCHORS, GRIDS)]
        for m, a in zip(cls, ANCHORS):
            m[:, 0::CLASSES] += 4
        reg = [torch.randn((n, a * 4, s, s), device="cuda", generator=g) for a, s in zip(ANCHORS, GRIDS)]
        images = R.ImageList(torch.zeros((n, 3, 300, 300), device="cuda"), [(300, 300)] * n)
        head_out = {"cls_logits": cls, "bbox_regression": reg}
        anchors = replica.anchor_generator(images, cls)
        permuted = {"cls_logits": torch.cat([R.permute_level(m, CLASSES) for m in cls], dim=1),
                    "bbox_regression": torch.cat([R.permute_level(m, 4) for m in reg], dim=1)}
        ours = lambda: model.candidates(head_out, cls, images)  # noqa: E731
        theirs = lambda: replica.candidates(permuted, anchors, images.image_sizes)  # noqa: E731
        idx, _, _, _, valid = ours()
        ms, ms_t = alternate([ours, theirs], iters)
        yield dict(what=f"candidates: ssd_scores + ssd_topk + ssd_decode, {idx.shape[1]} per image", batch=n, ours_ms=ms, torch_ms=ms_t,
                   kernel="k_ssd_scores + k_ssd_topk + k_ssd_decode", valid=int(valid.sum()))
        imgs = [torch.rand((3, 480, 640 - 16 * (i % 2)), device="cuda", generator=g) for i in range(n)]
        got, want = model(imgs), replica(imgs)
        ms, ms_t = alternate([lambda: model(imgs), lambda: replica(imgs)], max(1, iters // 2))
        yield dict(what="SSD.forward ssd300_vgg16", batch=n, ours_ms=ms, torch_ms=ms_t, detections=[len(d["boxes"]) for d in got],
                   torch_detections=[len(d["boxes"]) for d in want])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="profiles/perf_ssd.json")
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
