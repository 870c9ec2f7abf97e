#!/usr/bin/env python3
"""The detection transform's front end (normalize -> resize -> batch) on one MI355X, fp32: the fused launch against its pieces.

Batches of 2 and 8 COCO-shaped float32 images (480 x 640, 427 x 640, 640 x 480, 500 x 375 in turn), each allocated on its own,
resized to 800 / 1333 and padded to multiples of 32.  Rows, per batch:

  fused      F.detection_batch: ONE launch (k_interp_batch<norm>) from the images to the padded batch
  unfused    the library's own pieces: F.normalize and F.interpolate per image, then new_full + copy_ (batch_images)
  torch      the same four steps with torch on the same GPU: sub / div, nn.functional.interpolate, new_full, copy_

and the bytes the algorithm needs -- every source image read once, the batch written once -- over the fused time, as bytes / s.

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON.

  python tools/perf_det_transform.py [--batches 2 8] [--iters 200] [--out profiles/perf_det_transform.json]
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
from cpu_vision_amd.transform import resized_size  # noqa: E402
from tools.perf_detect import alternate  # noqa: E402

SHAPES = [(480, 640), (427, 640), (640, 480), (500, 375)]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
MIN_SIZE, MAX_SIZE, DIVISIBLE = 800, 1333, 32


def row_for(n, iters):
    g = torch.Generator(device="cuda").manual_seed(n)
    shapes = [SHAPES[i % len(SHAPES)] for i in range(n)]
    images = [torch.rand((3, h, w), device="cuda", generator=g) for h, w in shapes]
    sizes = [resized_size(h, w, MIN_SIZE, MAX_SIZE) for h, w in shapes]
    transform = mv.GeneralizedRCNNTransform(MIN_SIZE, MAX_SIZE, MEAN, STD, size_divisible=DIVISIBLE, _skip_resize=True)
    mean_t = torch.tensor(MEAN, device="cuda")[:, None, None]
    std_t = torch.tensor(STD, device="cuda")[:, None, None]

    def fused():
        return F.detection_batch(images, sizes, MEAN, STD, DIVISIBLE)

    def unfused():
        return transform.batch_images([F.interpolate(F.normalize(im, MEAN, STD)[None], size=list(s))[0] for im, s in zip(images, sizes)], DIVISIBLE)

    def with_torch():
        resized = [torch.nn.functional.interpolate(((im - mean_t) / std_t)[None], size=list(s), mode="bilinear", align_corners=False)[0]
                   for im, s in zip(images, sizes)]
        return transform.batch_images(resized, DIVISIBLE)

    batch = fused()
    kernel = _lib.last_kernel()
    same = bool(torch.equal(batch, unfused()))
    err = float((batch - with_torch()).abs().max())
    ms = alternate([fused, unfused, with_torch], iters)
    nbytes = 4 * (sum(3 * h * w for h, w in shapes) + batch.numel())
    return dict(batch=n, shapes=shapes, sizes=sizes, batch_shape=list(batch.shape), kernel=kernel, fused_ms=ms[0], unfused_ms=ms[1], torch_ms=ms[2],
                algorithmic_bytes=nbytes, fused_bytes_per_s=nbytes / (ms[0] * 1e-3), fused_equals_unfused=same, max_abs_diff_vs_torch=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[2, 8])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="profiles/perf_det_transform.json")
    a = ap.parse_args()
    rows = []
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for n in a.batches:
        row = row_for(n, a.iters)
        rows.append(row)
        Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=7, rows=rows), indent=1) + "\n")
        print(f"batch {n} {row['batch_shape']}: fused {row['fused_ms']:.4f} ms ({row['fused_bytes_per_s'] / 1e12:.2f} TB/s of {row['algorithmic_bytes'] / 1e6:.1f} MB)"
              f" | unfused {row['unfused_ms']:.4f} ms ({row['unfused_ms'] / row['fused_ms']:.2f}x) | torch {row['torch_ms']:.4f} ms"
              f" ({row['torch_ms'] / row['fused_ms']:.2f}x); fused == unfused: {row['fused_equals_unfused']}, max |fused - torch| {row['max_abs_diff_vs_torch']:.2e}",
              flush=True)


if __name__ == "__main__":
    main()
