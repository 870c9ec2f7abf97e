#!/usr/bin/env python3
"""F.rotate / F.affine / F.perspective on one MI355X: time per call (HIP events, median of 7 rounds of 5 back-to-back calls),
algorithmic bytes, TB/s and the fraction of the 8 TB/s HBM peak, for the kernel and for the reference's ops composed with torch
on the same GPU (base grid + bmm + cat of the ones-mask + grid_sample + fill blend + round).

  python tools/perf_warp.py [--iters 5] [--layouts]

--layouts also times both k_warp layouts (row segment / 2-D block) per case through the -DMV_TUNING library
(MV_WARP_LAYOUT=row|block).  Algorithmic bytes = planes * (H * W * in + OH * OW * out element size): no grid is read."""
import argparse
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from cpu_vision_amd import _lib, functional as F  # noqa: E402
from tools.perf_vgg import timeit  # noqa: E402

PEAK_TBS = 8.0


def torch_composition(img, coeffs, kind, fill):
    """The reference's _affine_grid / _perspective_grid + _apply_grid_transform (bilinear), as torch ops on the image's
    device.  `coeffs` is the 2 x 3 inverse affine matrix or the 8 perspective coefficients."""
    dev = img.device
    h, w = img.shape[-2:]
    base = torch.empty(1, h, w, 3, dtype=torch.float32, device=dev)
    if kind == "affine":
        base[..., 0].copy_(torch.linspace((1.0 - w) * 0.5, (w - 1.0) * 0.5, steps=w, device=dev))
        base[..., 1].copy_(torch.linspace((1.0 - h) * 0.5, (h - 1.0) * 0.5, steps=h, device=dev).unsqueeze_(-1))
        base[..., 2].fill_(1)
        theta = torch.tensor(coeffs, dtype=torch.float32, device=dev).reshape(1, 2, 3)
        rt = theta.transpose(1, 2).div_(torch.tensor([0.5 * w, 0.5 * h], dtype=torch.float32, device=dev))
        grid = base.view(1, h * w, 3).bmm(rt).view(1, h, w, 2)
    else:
        base[..., 0].copy_(torch.linspace(0.5, w - 0.5, steps=w, device=dev))
        base[..., 1].copy_(torch.linspace(0.5, h - 0.5, steps=h, device=dev).unsqueeze_(-1))
        base[..., 2].fill_(1)
        c = coeffs
        t1 = torch.tensor([[[c[0], c[1], c[2]], [c[3], c[4], c[5]]]], dtype=torch.float32, device=dev)
        t2 = torch.tensor([[[c[6], c[7], 1.0], [c[6], c[7], 1.0]]], dtype=torch.float32, device=dev)
        rt1 = t1.transpose(1, 2).div_(torch.tensor([0.5 * w, 0.5 * h], dtype=torch.float32, device=dev))
        g1 = base.view(1, h * w, 3).bmm(rt1)
        g2 = base.view(1, h * w, 3).bmm(t2.transpose(1, 2))
        grid = g1.div_(g2).sub_(1.0).view(1, h, w, 2)
    ch = img.shape[-3]
    x = img.reshape(-1, ch, h, w)
    n = x.shape[0]
    fp = img.dtype == torch.float32
    fi = x if fp else x.to(torch.float32)
    fi = torch.cat((fi, torch.ones(n, 1, h, w, dtype=torch.float32, device=dev)), 1)
    fi = torch.nn.functional.grid_sample(fi, grid.expand(n, -1, -1, -1), mode="bilinear", padding_mode="zeros",
                                         align_corners=False)
    fi, m = torch.tensor_split(fi, indices=(-1,), dim=-3)
    f_img = torch.tensor([float(fill)], dtype=torch.float32, device=dev).view(1, -1, 1, 1)
    fi = fi.sub_(f_img).mul_(m.expand_as(fi)).add_(f_img)
    return (fi.round_().to(img.dtype) if not fp else fi).reshape(img.shape)


def row(what, ms, nbytes, kernel=""):
    tbs = nbytes / (ms * 1e-3) / 1e12
    print(f"{what:52s} {ms:8.3f} ms  {nbytes / 1e9:6.3f} GB  {tbs:5.2f} TB/s  {tbs / PEAK_TBS * 100:5.1f} % of 8 TB/s  {kernel}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="back-to-back calls per timed round")
    ap.add_argument("--layouts", action="store_true", help="also time both k_warp layouts (tuning library)")
    args = ap.parse_args()
    h, w = 1080, 1920
    start = [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]]
    end = [[96, 40], [w - 150, 12], [w - 30, h - 90], [60, h - 20]]
    pcoeffs = F._get_perspective_coeffs(start, end)

    def rot(a):
        return (f"rotate {a}", lambda x: F.rotate(x, a, interpolation="bilinear", fill=0), "affine",
                F._get_inverse_affine_matrix([0.0, 0.0], -a, [0.0, 0.0], 1.0, [0.0, 0.0]))

    ops = [rot(0.0), rot(30.0), rot(45.0), rot(90.0),
           ("affine scale 0.8 shear (12, 5)", lambda x: F.affine(x, 10.0, [20, -10], 0.8, [12.0, 5.0], interpolation="bilinear",
                                                                 fill=0), "affine",
            F._get_inverse_affine_matrix([0.0, 0.0], 10.0, [20.0, -10.0], 0.8, [12.0, 5.0])),
           ("perspective", lambda x: F.perspective(x, start, end, fill=0), "perspective", pcoeffs)]
    torch.manual_seed(0)
    for dtype in (torch.float32, torch.uint8):
        shape = (32, 3, h, w)
        img = (torch.rand(shape, device="cuda") if dtype == torch.float32
               else torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda"))
        planes = img.numel() // (h * w)
        nbytes = planes * h * w * 2 * img.element_size()
        tag = f"32x3x1080x1920 {str(dtype).replace('torch.', '')}"
        for name, fn, kind, coeffs in ops:
            def ours():
                for _ in range(args.iters):
                    fn(img)

            def composed():
                for _ in range(args.iters):
                    torch_composition(img, coeffs, kind, 0)

            ms_ours = timeit(ours, 7) / args.iters
            kernel = _lib.last_kernel()
            ms_ref = timeit(composed, 7) / args.iters
            row(f"{name} {tag}", ms_ours, nbytes, kernel)
            row(f"  torch composition", ms_ref, nbytes)
            print(f"{'':52s} speed-up over the torch composition: {ms_ref / ms_ours:.2f}x", flush=True)
            if args.layouts:
                with _lib.tuning_library():
                    for layout in ("row", "block"):
                        os.environ["MV_WARP_LAYOUT"] = layout
                        ms = timeit(ours, 7) / args.iters
                        row(f"  layout {layout}", ms, nbytes, _lib.last_kernel())
                    del os.environ["MV_WARP_LAYOUT"]
        del img
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
