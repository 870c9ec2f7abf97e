#!/usr/bin/env python3
"""F.elastic on one MI355X: time per call (HIP events, median of 7 rounds of 5 back-to-back calls), algorithmic bytes, TB/s and
the fraction of the 8 TB/s HBM peak, for the kernel and for the reference's ops composed with torch on the same GPU (identity
grid + add + cat of the ones-mask + grid_sample + fill blend + round).

  python tools/perf_elastic.py [--iters 5]

Algorithmic bytes = planes * H * W * (in + out element size) + 8 * H * W (the fp32 (1, H, W, 2) field, read once)."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from cpu_vision_amd import _lib, functional as F, transforms  # noqa: E402
from tools.perf_vgg import timeit  # noqa: E402

PEAK_TBS = 8.0


def torch_composition(img, disp, fill):
    """The reference's _create_identity_grid + _apply_grid_transform, as torch ops on the image's device."""
    h, w = img.shape[-2:]
    dt = img.dtype if img.is_floating_point() else torch.float32
    g = torch.empty(1, h, w, 2, dtype=dt, device=img.device)
    g[..., 0].copy_(torch.linspace((-w + 1) / w, (w - 1) / w, w, dtype=dt, device=img.device))
    g[..., 1].copy_(torch.linspace((-h + 1) / h, (h - 1) / h, h, dtype=dt, device=img.device).unsqueeze_(-1))
    g = g.add_(disp.to(dt))
    c = img.shape[-3]
    x = img.reshape(-1, c, h, w)
    n = x.shape[0]
    fp = img.dtype == dt
    fi = x if fp else x.to(dt)
    fi = torch.cat((fi, torch.ones(n, 1, h, w, dtype=dt, device=img.device)), 1)
    fi = torch.nn.functional.grid_sample(fi, g.expand(n, -1, -1, -1), mode="bilinear", padding_mode="zeros", align_corners=False)
    fi, m = torch.tensor_split(fi, indices=(-1,), dim=-3)
    f_img = torch.tensor([float(fill)], dtype=dt, device=img.device).view(1, -1, 1, 1)
    fi = fi.sub_(f_img).mul_(m.expand_as(fi)).add_(f_img)
    return (fi.round_().to(img.dtype) if not fp else fi).reshape(img.shape)


def row(what, ms, nbytes, kernel=""):
    tbs = nbytes / (ms * 1e-3) / 1e12
    print(f"{what:44s} {ms:8.3f} ms  {nbytes / 1e9:6.3f} GB  {tbs:5.2f} TB/s  {tbs / PEAK_TBS * 100:5.1f} % of 8 TB/s  {kernel}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="back-to-back calls per timed round")
    args = ap.parse_args()
    torch.manual_seed(0)
    cases = [((32, 3, 1080, 1920), torch.float32), ((32, 3, 1080, 1920), torch.uint8), ((3, 224, 224), torch.uint8)]
    for shape, dtype in cases:
        h, w = shape[-2:]
        img = (torch.rand(shape, device="cuda") if dtype == torch.float32
               else torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda"))
        disp = transforms.ElasticTransform(alpha=50.0, sigma=5.0).get_params(img)["displacement"]
        planes = img.numel() // (h * w)
        nbytes = planes * h * w * 2 * img.element_size() + 8 * h * w
        tag = f"{'x'.join(map(str, shape))} {str(dtype).replace('torch.', '')}"

        def ours():
            for _ in range(args.iters):
                F.elastic(img, disp, fill=0)

        def composed():
            for _ in range(args.iters):
                torch_composition(img, disp, 0)

        ms_ours = timeit(ours, 7) / args.iters
        kernel = _lib.last_kernel()
        ms_ref = timeit(composed, 7) / args.iters
        row(f"F.elastic {tag}", ms_ours, nbytes, kernel)
        row(f"torch composition {tag}", ms_ref, nbytes)
        print(f"{'':44s} speed-up over the torch composition: {ms_ref / ms_ours:.2f}x", flush=True)
        del img, disp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
