#!/usr/bin/env python3
"""The mask branch of Mask R-CNN on one MI355X, fp32: each fused launch against its pieces, and the whole model.

  (a) paste     F.paste_masks_in_image of R = 100 masks into 800 x 1216 and of R = 20 into 480 x 640 (28 x 28 masks, boxes as a
                detector returns them: inside the image, 30 .. 300 pixels a side), ONE launch (k_paste_masks), against
                  unfused   the library's own composition: per mask F.interpolate of the zero-padded mask, then torch's zeros, slice
                            copy and stack (the integer boxes read back once, as the reference reads them)
                  torch     the reference's paste_masks_in_image (tests/_mask_ref.py's replica) with torch on the same GPU
                and the bytes the algorithm needs -- the result written once, the masks and boxes read once -- over the fused time
  (b) convT     F.conv_transpose2d_bias_act at (100, 256, 14, 14) -> (100, 256, 28, 28), ONE launch (k_conv1x1_ct), against
                  unfused   the pointwise conv on the relaid weight (F.conv_norm_act, 1024 channels) plus torch's pixel-shuffle copy
                  torch     torch.nn.functional.conv_transpose2d + relu
  (c) probs     F.mask_probs at (100, 91, 28, 28), ONE launch (k_mask_probs), against torch's sigmoid()[index, labels]
  (d) model     maskrcnn_resnet50_fpn forward at batch 2 (480 x 640 and 427 x 640 images, random weights), and the same model without
                its mask branch (the roi_heads' mask modules removed): the difference is the share of the mask branch

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON, the printed lines to the log next to it.

  python tools/perf_mask_rcnn.py [--iters 50] [--only paste convT probs model] [--out profiles/perf_mask_rcnn.json]
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
from tests import _mask_ref as M  # noqa: E402
from tools.perf_detect import alternate  # noqa: E402

COPY_BYTES_PER_S = 6.3e12  # what a device-to-device copy reaches on this GPU


def detector_boxes(r, h, w, g):
    side = 30 + torch.rand((r, 2), device="cuda", generator=g) * 270
    side = torch.minimum(side, torch.tensor([w - 2.0, h - 2.0], device="cuda"))
    corner = torch.rand((r, 2), device="cuda", generator=g) * (torch.tensor([float(w), float(h)], device="cuda") - side)
    return torch.cat([corner, corner + side], 1).contiguous()


def paste_row(r, h, w, iters):
    g = torch.Generator(device="cuda").manual_seed(r)
    masks = torch.rand((r, 1, 28, 28), device="cuda", generator=g)
    boxes = detector_boxes(r, h, w, g)

    def fused():
        return F.paste_masks_in_image(masks, boxes, (h, w))

    def unfused():
        padded, scale = M.expand_masks(masks, 1)
        ints = M.expand_boxes(boxes, scale).to(torch.int64).tolist()  # one read-back
        res = []
        for i, (bx0, by0, bx1, by1) in enumerate(ints):
            bw, bh = max(bx1 - bx0 + 1, 1), max(by1 - by0 + 1, 1)
            resized = F.interpolate(padded[i:i + 1], size=[bh, bw])[0, 0]
            image = torch.zeros((h, w), device="cuda")
            x0, x1, y0, y1 = max(bx0, 0), min(bx1 + 1, w), max(by0, 0), min(by1 + 1, h)
            image[y0:y1, x0:x1] = resized[y0 - by0:y1 - by0, x0 - bx0:x1 - bx0]
            res.append(image)
        return torch.stack(res, 0)[:, None]

    def with_torch():
        return M.paste_masks_in_image(masks, boxes, (h, w))

    out = fused()
    kernel = _lib.last_kernel()
    same = bool(torch.equal(out, unfused()))
    err = float((out - with_torch()).abs().max())
    ms = alternate([fused, unfused, with_torch], iters)
    nbytes = 4 * (out.numel() + masks.numel() + boxes.numel())
    rate = nbytes / (ms[0] * 1e-3)
    return dict(what="paste", rois=r, image=[h, w], kernel=kernel, fused_ms=ms[0], unfused_ms=ms[1], torch_ms=ms[2], algorithmic_bytes=nbytes,
                fused_bytes_per_s=rate, share_of_copy_rate=rate / COPY_BYTES_PER_S, fused_equals_unfused=same, max_abs_diff_vs_torch=err,
                box_area_share=float(((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).mean()) / (h * w))


def conv_transpose_row(n, cin, hw, cout, iters):
    g = torch.Generator(device="cuda").manual_seed(cin)
    x = torch.rand((n, cin, hw, hw), device="cuda", generator=g) * 2 - 1
    wt = (torch.rand((cin, cout, 2, 2), device="cuda", generator=g) * 2 - 1) * (2.0 / cin ** 0.5)
    b = torch.rand((cout,), device="cuda", generator=g) * 2 - 1
    relaid = F.conv_transpose2x2_relayout(wt, b, x.device)
    w4 = relaid[0].reshape(4 * cout, cin, 1, 1)

    def fused():
        return F.conv_transpose2d_bias_act(x, wt, b, "relu", relaid=relaid)

    def unfused():
        y4 = F.conv_norm_act(x, w4, relaid[1], activation="relu")
        return y4.view(n, cout, 2, 2, hw, hw).permute(0, 1, 4, 2, 5, 3).reshape(n, cout, 2 * hw, 2 * hw)

    def with_torch():
        return torch.relu_(torch.nn.functional.conv_transpose2d(x, wt, b, stride=2))

    out = fused()
    kernel = _lib.last_kernel()
    same = bool(torch.equal(out, unfused()))
    err = float((out - with_torch()).abs().max())
    ms = alternate([fused, unfused, with_torch], iters)
    flops = 2.0 * n * hw * hw * cin * 4 * cout
    nbytes = 4 * (x.numel() + out.numel() + wt.numel())
    return dict(what="convT", shape=[n, cin, hw, hw, cout], kernel=kernel, k_slices=list(F.conv1x1_k_slices(n, cin, hw, hw, 4 * cout)), fused_ms=ms[0],
                unfused_ms=ms[1], torch_ms=ms[2], flops=flops, fused_flops_per_s=flops / (ms[0] * 1e-3), algorithmic_bytes=nbytes,
                fused_bytes_per_s=nbytes / (ms[0] * 1e-3), fused_equals_unfused=same, max_abs_diff_vs_torch=err)


def probs_row(r, c, m, iters):
    g = torch.Generator(device="cuda").manual_seed(c)
    logits = torch.randn((r, c, m, m), device="cuda", generator=g) * 3
    labels = torch.randint(1, c, (r,), device="cuda", generator=g)
    index = torch.arange(r, device="cuda")

    def fused():
        return F.mask_probs(logits, labels)

    def with_torch():
        return logits.sigmoid()[index, labels][:, None]

    out = fused()
    kernel = _lib.last_kernel()
    err = float((out - with_torch()).abs().max())
    ms = alternate([fused, with_torch], iters)
    return dict(what="probs", shape=[r, c, m, m], kernel=kernel, fused_ms=ms[0], torch_ms=ms[1], max_abs_diff_vs_torch=err)


def model_row(iters):
    torch.manual_seed(0)
    model = mv.maskrcnn_resnet50_fpn(num_classes=91, box_score_thresh=0.0).cuda()  # random weights: keep every detection, 100 per image
    g = torch.Generator(device="cuda").manual_seed(1)
    images = [torch.rand((3, 480, 640), device="cuda", generator=g), torch.rand((3, 427, 640), device="cuda", generator=g)]
    heads = model.roi_heads
    mask_modules = (heads.mask_roi_pool, heads.mask_head, heads.mask_predictor)

    def with_masks():
        heads.mask_roi_pool, heads.mask_head, heads.mask_predictor = mask_modules
        with torch.no_grad():
            return model(images)

    def boxes_only():
        heads.mask_roi_pool = heads.mask_head = heads.mask_predictor = None
        with torch.no_grad():
            return model(images)

    out = with_masks()
    counts = [int(o["boxes"].shape[0]) for o in out]
    ms = alternate([with_masks, boxes_only], iters)
    heads.mask_roi_pool, heads.mask_head, heads.mask_predictor = mask_modules
    return dict(what="model", model="maskrcnn_resnet50_fpn", batch=2, images=[[480, 640], [427, 640]], detections=counts,
                masks_shape=[list(o["masks"].shape) for o in out], forward_ms=ms[0], without_mask_branch_ms=ms[1],
                mask_branch_share=(ms[0] - ms[1]) / ms[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", nargs="+", default=["paste", "convT", "probs", "model"])
    ap.add_argument("--out", default="profiles/perf_mask_rcnn.json")
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

    if "paste" in a.only:
        for r, h, w in ((100, 800, 1216), (20, 480, 640)):
            row = paste_row(r, h, w, max(a.iters // 5, 2))
            done(row, f"paste R={r} into {h}x{w} ({row['kernel']}): fused {row['fused_ms']:.4f} ms ({row['fused_bytes_per_s'] / 1e12:.2f} TB/s of "
                      f"{row['algorithmic_bytes'] / 1e6:.1f} MB, {100 * row['share_of_copy_rate']:.0f} % of the copy rate) | unfused {row['unfused_ms']:.4f} ms "
                      f"({row['unfused_ms'] / row['fused_ms']:.1f}x) | torch {row['torch_ms']:.4f} ms ({row['torch_ms'] / row['fused_ms']:.1f}x); "
                      f"fused == unfused: {row['fused_equals_unfused']}, max |fused - torch| {row['max_abs_diff_vs_torch']:.2e}")
    if "convT" in a.only:
        row = conv_transpose_row(100, 256, 14, 256, a.iters)
        done(row, f"convT {row['shape']} ({row['kernel']}, k slices {row['k_slices']}): fused {row['fused_ms']:.4f} ms ({row['fused_flops_per_s'] / 1e12:.1f} "
                  f"TFLOP/s, {row['fused_bytes_per_s'] / 1e12:.2f} TB/s) | pointwise + shuffle copy {row['unfused_ms']:.4f} ms "
                  f"({row['unfused_ms'] / row['fused_ms']:.2f}x) | torch {row['torch_ms']:.4f} ms ({row['torch_ms'] / row['fused_ms']:.2f}x); "
                  f"fused == unfused: {row['fused_equals_unfused']}, max |fused - torch| {row['max_abs_diff_vs_torch']:.2e}")
    if "probs" in a.only:
        row = probs_row(100, 91, 28, a.iters)
        done(row, f"probs {row['shape']} ({row['kernel']}): fused {row['fused_ms']:.4f} ms | torch sigmoid + index {row['torch_ms']:.4f} ms "
                  f"({row['torch_ms'] / row['fused_ms']:.1f}x); max |fused - torch| {row['max_abs_diff_vs_torch']:.2e}")
    if "model" in a.only:
        row = model_row(max(a.iters // 10, 2))
        done(row, f"maskrcnn_resnet50_fpn batch 2, detections {row['detections']}: forward {row['forward_ms']:.2f} ms | without the mask branch "
                  f"{row['without_mask_branch_ms']:.2f} ms | mask branch {100 * row['mask_branch_share']:.0f} % of the forward")


if __name__ == "__main__":
    main()
