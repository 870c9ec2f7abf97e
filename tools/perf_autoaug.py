#!/usr/bin/env python3
"""The automatic-augmentation colour ops and the policies on one MI355X: time per call (HIP events, median of 7 rounds of
`--iters` back-to-back calls after a warm-up), algorithmic bytes, TB/s and the fraction of the 8 TB/s HBM peak, and the
speed-up over the reference's ops composed with torch on the same GPU (tests/_autoaug_ref.py's restatement, run on the
device).

  python tools/perf_autoaug.py [--iters 5] [--seeds 16]

Cases: 32 x 3 x 1080p and 256 x 3 x 224^2, uint8 and float32; invert, posterize(4), solarize(0.5 of the bound),
autocontrast, equalize on random images and equalize on constant images (every pixel in one histogram bin); then
TrivialAugmentWide and RandAugment per call over a fixed set of seeds (the same draws for both sides: the reference side
applies the library's draws with the torch composition where it has one, the library's own op otherwise).  Algorithmic
bytes = input + output, plus one more input read for autocontrast and equalize.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from cpu_vision_amd import _lib, functional as F, transforms  # noqa: E402
from tests import _autoaug_ref as R  # noqa: E402
from tools.perf_vgg import timeit  # noqa: E402

PEAK_TBS = 8.0


def row(what, ms, nbytes, kernel=""):
    tbs = nbytes / (ms * 1e-3) / 1e12
    print(f"{what:44s} {ms:8.3f} ms  {nbytes / 1e9:6.3f} GB  {tbs:5.2f} TB/s  {tbs / PEAK_TBS * 100:5.1f} % of 8 TB/s  {kernel}",
          flush=True)


def compare(what, ours, ref, nbytes, iters, calls=1):
    """`ours` / `ref` make `calls` calls each; rows are per call (nbytes: of one call)."""
    def run_ours():
        for _ in range(iters):
            ours()

    def run_ref():
        for _ in range(iters):
            ref()

    ms_ours = timeit(run_ours, 7) / iters / calls
    kernel = _lib.last_kernel()
    ms_ref = timeit(run_ref, 7) / iters / calls
    row(what, ms_ours, nbytes, kernel)
    row("  torch composition", ms_ref, nbytes)
    print(f"{'':44s} speed-up over the torch composition: {ms_ref / ms_ours:.2f}x", flush=True)


def policy_case(t, img, seeds, tag, iters):
    """Per call of the policy over `seeds` (re-seeded before every call, so both sides apply the same draws)."""
    draws = []
    rec = t._apply_image_or_video_transform

    def record(image, transform_id, magnitude, interpolation, fill):
        draws[-1].append((transform_id, magnitude))
        return image

    t._apply_image_or_video_transform = record
    for s in seeds:
        draws.append([])
        torch.manual_seed(s)
        t(img)
    t._apply_image_or_video_transform = rec
    del t._apply_image_or_video_transform

    def ours():
        for s in seeds:
            torch.manual_seed(s)
            t(img)

    def ref():
        for calls in draws:
            x = img
            for op, m in calls:
                y = R.ref_apply(x, op, m)
                x = y if y is not None else t._apply_image_or_video_transform(x, op, m, t.interpolation, t._fill)

    n = len(seeds)
    compare(f"{type(t).__name__} {tag} (per call)", ours, ref, img.numel() * img.element_size() * 2, iters, calls=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="back-to-back calls per timed round")
    ap.add_argument("--seeds", type=int, default=16, help="policy calls per round")
    args = ap.parse_args()
    torch.manual_seed(0)
    for n, h, w in ((32, 1080, 1920), (256, 224, 224)):
        for dtype in (torch.uint8, torch.float32):
            shape = (n, 3, h, w)
            img = (torch.rand(shape, device="cuda") if dtype == torch.float32
                   else torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda"))
            flat = torch.full(shape, 0.3 if dtype == torch.float32 else 77, dtype=dtype, device="cuda")
            bound = 1.0 if dtype == torch.float32 else 255
            tag = f"{n}x3x{h}x{w} {str(dtype).replace('torch.', '')}"
            size = img.numel() * img.element_size()
            cases = [
                ("invert", lambda x: F.invert(x), R.ref_invert, 2),
                ("posterize", lambda x: F.posterize(x, 4), lambda x: R.ref_posterize(x, 4), 2),
                ("solarize", lambda x: F.solarize(x, 0.5 * bound), lambda x: R.ref_solarize(x, 0.5 * bound), 2),
                ("autocontrast", lambda x: F.autocontrast(x), R.ref_autocontrast, 3),
                ("equalize", lambda x: F.equalize(x), R.ref_equalize, 3),
            ]
            for name, ours, ref, k in cases:
                compare(f"{name} {tag}", lambda: ours(img), lambda: ref(img), size * k, args.iters)
            compare(f"equalize constant {tag}", lambda: F.equalize(flat), lambda: R.ref_equalize(flat), size * 3, args.iters)
            seeds = list(range(args.seeds))
            x1 = img[0]
            policy_case(transforms.TrivialAugmentWide(), x1, seeds, f"3x{h}x{w} {str(dtype).replace('torch.', '')}", 1)
            policy_case(transforms.RandAugment(), x1, seeds, f"3x{h}x{w} {str(dtype).replace('torch.', '')}", 1)
            del img, flat
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
