#!/usr/bin/env python3
"""The keypoint branch of Keypoint R-CNN on one MI355X, fp32: each fused launch against its pieces, and the whole model.

  (a) keypoints F.heatmaps_to_keypoints of R = 100 and of R = 20 rois with K = 17 heatmaps of 56 x 56 (boxes as a detector returns
                them in an 800 x 1216 image: 30 .. 300 pixels a side), ONE launch (k_heatmaps_to_keypoints), against
                  torch     the reference's loop over the detections (tests/_keypoint_ref.py's replica: two read-backs, a bicubic
                            interpolate, an argmax and a gather per roi) with torch on the same GPU
  (b) convT     F.conv_transpose2d_bias_act, kernel 4 / stride 2 / padding 1, at (100, 512, 14, 14) -> (100, 17, 28, 28), ONE launch
                (k_conv_igemm_tr), against
                  unfused   the library's own composition: F.conv2d_bias_act of the relaid weight with padding 1 (68 channels on the
                            15 x 15 window positions) plus torch's strided gather of the four phases
                  torch     torch.nn.functional.conv_transpose2d
  (c) model     keypointrcnn_resnet50_fpn forward at batch 2 (480 x 640 and 427 x 640 images, random weights), and the same model
                without its keypoint branch (the roi_heads' keypoint modules removed): the difference is the share of the branch

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON, the printed lines to the log next to it.

  python tools/perf_keypoint_rcnn.py [--iters 50] [--only keypoints convT model] [--out profiles/perf_keypoint_rcnn.json]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from tests import _keypoint_ref as KR  # noqa: E402
from tools.perf_detect import alternate  # noqa: E402
from tools.perf_mask_rcnn import detector_boxes  # noqa: E402


def keypoints_row(r, k, h, w, iters):
    g = torch.Generator(device="cuda").manual_seed(r)
    maps = torch.randn((r, k, 56, 56), device="cuda", generator=g)
    boxes = detector_boxes(r, h, w, g)

    def fused():
        return F.heatmaps_to_keypoints(maps, boxes)

    def with_torch():
        return KR.heatmaps_to_keypoints(maps, boxes)

    xy, scores = fused()
    kernel = _lib.last_kernel()
    txy, tscores = with_torch()
    same_position = float(((xy[..., :2] - txy[..., :2]).abs().amax(-1) <= 1e-3).float().mean())
    err = float((scores - tscores).abs().max())
    ms = alternate([fused, with_torch], iters)
    outputs = float((torch.clamp(boxes[:, 2] - boxes[:, 0], min=1).ceil() * torch.clamp(boxes[:, 3] - boxes[:, 1], min=1).ceil()).sum()) * k
    return dict(what="keypoints", rois=r, keypoints=k, image=[h, w], kernel=kernel, fused_ms=ms[0], torch_ms=ms[1], resized_elements=outputs,
                fused_elements_per_s=outputs / (ms[0] * 1e-3), same_position_share=same_position, max_abs_score_diff_vs_torch=err)


def conv_transpose_row(n, cin, hw, cout, iters):
    g = torch.Generator(device="cuda").manual_seed(cin)
    x = torch.rand((n, cin, hw, hw), device="cuda", generator=g) * 2 - 1
    wt = (torch.rand((cin, cout, 4, 4), device="cuda", generator=g) * 2 - 1) * (1.0 / cin ** 0.5)
    b = torch.rand((cout,), device="cuda", generator=g) * 2 - 1
    relaid = F.conv_transpose4x4_relayout(wt, b, x.device)

    def fused():
        return F.conv_transpose2d_bias_act(x, wt, b, None, padding=1, relaid=relaid)

    def unfused():
        return KR.gather_phases(F.conv2d_bias_act(x, relaid[0], relaid[1], padding=1))

    def with_torch():
        return torch.nn.functional.conv_transpose2d(x, wt, b, stride=2, padding=1)

    out = fused()
    kernel = _lib.last_kernel()
    same = bool(torch.equal(out, unfused()))
    unfused_kernel = _lib.last_kernel()
    err = float((out - with_torch()).abs().max())
    ms = alternate([fused, unfused, with_torch], iters)
    flops = 2.0 * n * (2 * hw) * (2 * hw) * cin * 4 * cout  # every output sums 4 taps of cin channels
    nbytes = 4 * (x.numel() + out.numel() + wt.numel())
    return dict(what="convT", shape=[n, cin, hw, hw, cout], kernel=kernel, unfused_kernel=unfused_kernel, fused_ms=ms[0], unfused_ms=ms[1],
                torch_ms=ms[2], flops=flops, fused_flops_per_s=flops / (ms[0] * 1e-3), algorithmic_bytes=nbytes,
                fused_bytes_per_s=nbytes / (ms[0] * 1e-3), fused_equals_unfused=same, max_abs_diff_vs_torch=err)


def model_row(iters):
    torch.manual_seed(0)
    model = mv.keypointrcnn_resnet50_fpn(box_score_thresh=0.0).cuda()  # random weights: keep every detection, 100 per image
    g = torch.Generator(device="cuda").manual_seed(1)
    images = [torch.rand((3, 480, 640), device="cuda", generator=g), torch.rand((3, 427, 640), device="cuda", generator=g)]
    heads = model.roi_heads
    modules = (heads.keypoint_roi_pool, heads.keypoint_head, heads.keypoint_predictor)

    def with_keypoints():
        heads.keypoint_roi_pool, heads.keypoint_head, heads.keypoint_predictor = modules
        with torch.no_grad():
            return model(images)

    def boxes_only():
        heads.keypoint_roi_pool = heads.keypoint_head = heads.keypoint_predictor = None
        with torch.no_grad():
            return model(images)

    out = with_keypoints()
    counts = [int(o["boxes"].shape[0]) for o in out]
    ms = alternate([with_keypoints, boxes_only], iters)
    heads.keypoint_roi_pool, heads.keypoint_head, heads.keypoint_predictor = modules
    return dict(what="model", model="keypointrcnn_resnet50_fpn", batch=2, images=[[480, 640], [427, 640]], detections=counts,
                keypoints_shape=[list(o["keypoints"].shape) for o in out], forward_ms=ms[0], without_keypoint_branch_ms=ms[1],
                keypoint_branch_share=(ms[0] - ms[1]) / ms[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", nargs="+", default=["keypoints", "convT", "model"])
    ap.add_argument("--out", default="profiles/perf_keypoint_rcnn.json")
    a = ap.parse_args()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rows, lines = [], []

    def done(row, line):
        rows.append(row)
        lines.append(line)
        out.write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=7, rows=rows), indent=1) + "\n")
        out.with_suffix(".log").write_text("\n".join(lines) + "\n")
        print(line, flush=True)

    if "keypoints" in a.only:
        for r in (100, 20):
            row = keypoints_row(r, 17, 800, 1216, max(a.iters // 10, 2))
            done(row, f"keypoints R={r} K=17 in 800x1216 ({row['kernel']}): fused {row['fused_ms']:.4f} ms ({row['fused_elements_per_s'] / 1e9:.1f} G "
                      f"resized elements/s of {row['resized_elements'] / 1e6:.1f} M) | torch loop {row['torch_ms']:.3f} ms ({row['torch_ms'] / row['fused_ms']:.0f}x); "
                      f"same position {100 * row['same_position_share']:.1f} %, max |score - torch| {row['max_abs_score_diff_vs_torch']:.2e}")
    if "convT" in a.only:
        row = conv_transpose_row(100, 512, 14, 17, a.iters)
        done(row, f"convT {row['shape']} ({row['kernel']}): fused {row['fused_ms']:.4f} ms ({row['fused_flops_per_s'] / 1e12:.1f} TFLOP/s, "
                  f"{row['fused_bytes_per_s'] / 1e12:.2f} TB/s) | conv + gather ({row['unfused_kernel']}) {row['unfused_ms']:.4f} ms "
                  f"({row['unfused_ms'] / row['fused_ms']:.2f}x) | torch {row['torch_ms']:.4f} ms ({row['torch_ms'] / row['fused_ms']:.2f}x); "
                  f"fused == unfused: {row['fused_equals_unfused']}, max |fused - torch| {row['max_abs_diff_vs_torch']:.2e}")
    if "model" in a.only:
        row = model_row(max(a.iters // 10, 2))
        done(row, f"keypointrcnn_resnet50_fpn batch 2, detections {row['detections']}: forward {row['forward_ms']:.2f} ms | without the keypoint "
                  f"branch {row['without_keypoint_branch_ms']:.2f} ms | keypoint branch {100 * row['keypoint_branch_share']:.0f} % of the forward")


if __name__ == "__main__":
    main()
