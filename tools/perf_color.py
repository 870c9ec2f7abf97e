#!/usr/bin/env python3
"""The colour ops and ColorJitter on one MI355X: time per call (HIP events, median of 7 rounds of `--iters` back-to-back calls
after a warm-up), algorithmic bytes, TB/s and the fraction of the 8 TB/s HBM peak, and the speed-up over the reference's ops
composed with torch on the same GPU (tests/_color_ref.py's restatement, run on the device).

  python tools/perf_color.py [--iters 5]

Cases: 32 x 3 x 1080p and 256 x 3 x 224^2, uint8 and float32; brightness, contrast, saturation, hue (fixed factors) and the
fused ColorJitter chain hue -> contrast -> brightness -> saturation.  Algorithmic bytes = input + output, plus one more input
read when contrast is in the chain (its mean pass).  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run
of this script."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from cpu_vision_amd import _lib, functional as F  # noqa: E402
from tests import _color_ref as R  # noqa: E402
from tools.perf_vgg import timeit  # noqa: E402

PEAK_TBS = 8.0
JITTER = [("hue", 0.08), ("contrast", 1.3), ("brightness", 0.8), ("saturation", 1.2)]
CASES = [("brightness", [("brightness", 1.3)]), ("contrast", [("contrast", 1.3)]), ("saturation", [("saturation", 0.7)]),
         ("hue", [("hue", 0.1)]), ("ColorJitter", JITTER)]


def row(what, ms, nbytes, kernel=""):
    tbs = nbytes / (ms * 1e-3) / 1e12
    print(f"{what:44s} {ms:8.3f} ms  {nbytes / 1e9:6.3f} GB  {tbs:5.2f} TB/s  {tbs / PEAK_TBS * 100:5.1f} % of 8 TB/s  {kernel}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="back-to-back calls per timed round")
    args = ap.parse_args()
    torch.manual_seed(0)
    for n, h, w in ((32, 1080, 1920), (256, 224, 224)):
        for dtype in (torch.uint8, torch.float32):
            shape = (n, 3, h, w)
            img = (torch.rand(shape, device="cuda") if dtype == torch.float32
                   else torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda"))
            tag = f"{n}x3x{h}x{w} {str(dtype).replace('torch.', '')}"
            for name, ops in CASES:
                nbytes = img.numel() * img.element_size() * (3 if any(o == "contrast" for o, _ in ops) else 2)

                def ours():
                    for _ in range(args.iters):
                        F.color_jitter_image(img, ops)

                def composed():
                    for _ in range(args.iters):
                        R.ref_chain(img, ops)

                ms_ours = timeit(ours, 7) / args.iters
                kernel = _lib.last_kernel()
                ms_ref = timeit(composed, 7) / args.iters
                row(f"{name} {tag}", ms_ours, nbytes, kernel)
                row("  torch composition", ms_ref, nbytes)
                print(f"{'':44s} speed-up over the torch composition: {ms_ref / ms_ours:.2f}x", flush=True)
            del img
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
