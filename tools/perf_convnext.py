#!/usr/bin/env python3
"""ConvNeXt inference on one MI355X against the torch replica of the reference (tests/_convnext_ref.py) on the same GPU, fp32.

Rows, per batch (1 and 64 by default), for one block of each of convnext_tiny's four stages at 224 x 224 (96 @ 56 x 56, 192 @ 28 x 28,
384 @ 14 x 14, 768 @ 7 x 7):

  dwconv7x7         F.dwconv7x7 (k_dwpc7x7) | torch's conv2d(groups=C).  GB/s: the input read once and the output written once
  ln stats / ln     F.layer_norm2d_stats and F.layer_norm2d (k_layer_norm2d) | the replica's permute + layer_norm + permute.  GB/s: the
                    input read once (and the output written once)
  linear + gelu     F.conv1x1_gelu with the norm in its loads (k_conv1x1_ln<..,norm>) | the same launch with gelu=False (what the
                    float64 erf costs the epilogue) | the plain loads on a materialised input (k_conv1x1_ln<..,plain>) | torch's
                    linear + gelu on the NHWC tensor
  projection        F.conv_norm_act(..., alpha=layer_scale, residual=input) (k_conv1x1) | torch's linear, scale and add
  block             CNBlock.forward with the norm in the loads (four launches) | materialised (five) | the replica's block
  accuracy          the block's error against the float64 replica, in units of 2^-24 max|f64|, beside the float32 replica's: the second
                    Linear sums 4C products per output in the order F.conv1x1_k_slices states for the shape
  forward           convnext_tiny at 224 x 224, four-launch blocks | five-launch blocks | the replica's forward

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON.

  python tools/perf_convnext.py [--batches 1 64] [--iters 10] [--out profiles/perf_convnext.json]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import convnext as CN  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from tests import _convnext_ref as R  # noqa: E402
from tools.perf_detect import alternate  # noqa: E402

STAGES = [(96, 56), (192, 28), (384, 14), (768, 7)]


def _block_pair(dim, seed):
    rep, cpu = R.block_pair(dim, seed, CN.CNBlock, layer_scale=1.0, weight_factor=4.0 if dim >= 384 else 8.0)
    dev = CN.CNBlock(dim, 1e-6, 0.0)
    dev.load_state_dict(cpu.state_dict(), strict=True)
    return rep, dev.cuda().eval()


def _with_fusion(flag, fn):
    def run():
        saved = CN._use_fused
        CN._use_fused = lambda dim, pixels: flag
        try:
            return fn()
        finally:
            CN._use_fused = saved
    return run


def rows_for(n, iters, stages, forward):
    g = torch.Generator(device="cuda").manual_seed(7 + n)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
    with torch.no_grad():
        for dim, side in stages:
            shape = f"{dim} x {side} x {side}"
            rep, blk = _block_pair(dim, 20 + dim)
            conv, norm, fc1, fc2 = blk.block[0], blk.block[2], blk.block[3], blk.block[5]
            x = rnd(n, dim, side, side)
            ms, ms_t = alternate([lambda: F.dwconv7x7(x, conv.weight, conv.bias), lambda: nn.functional.conv2d(x, conv.weight, conv.bias, 1, 3, 1, dim)], iters)
            h = F.dwconv7x7(x, conv.weight, conv.bias)
            yield dict(what=f"dwconv7x7 {shape}", batch=n, ours_ms=ms, torch_ms=ms_t, kernel=_lib.last_kernel(), gb_per_s=8.0 * x.numel() / (ms * 1e-3) / 1e9)
            t_ln = lambda: nn.functional.layer_norm(h.permute(0, 2, 3, 1), (dim,), norm.weight, norm.bias, norm.eps).permute(0, 3, 1, 2)  # noqa: E731
            ms_s, ms, ms_t = alternate([lambda: F.layer_norm2d_stats(h, norm.eps), lambda: F.layer_norm2d(h, norm.weight, norm.bias, norm.eps), t_ln], iters)
            yield dict(what=f"layer_norm2d_stats {shape}", batch=n, ours_ms=ms_s, torch_ms=ms_t, kernel="k_layer_norm2d<stats>", gb_per_s=4.0 * h.numel() / (ms_s * 1e-3) / 1e9)
            yield dict(what=f"layer_norm2d {shape}", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_layer_norm2d<apply>", gb_per_s=8.0 * h.numel() / (ms * 1e-3) / 1e9,
                       max_abs_diff_vs_torch=float((F.layer_norm2d(h, norm.weight, norm.bias, norm.eps) - t_ln()).abs().max()))
            mean, rstd = F.layer_norm2d_stats(h, norm.eps)
            z = F.layer_norm2d(h, norm.weight, norm.bias, norm.eps)
            stats = (mean, rstd, norm.weight, norm.bias)
            z_nhwc = z.permute(0, 2, 3, 1).contiguous()
            fused = lambda: F.conv1x1_gelu(h, fc1.weight, fc1.bias, norm=stats)  # noqa: E731
            y = fused()
            name = _lib.last_kernel()
            same = bool(torch.equal(y, F.conv1x1_gelu(z, fc1.weight, fc1.bias)))
            diff = float((y - nn.functional.gelu(nn.functional.linear(z_nhwc, fc1.weight, fc1.bias)).permute(0, 3, 1, 2)).abs().max())
            ms, ms_n, ms_p, ms_t = alternate([fused, lambda: F.conv1x1_gelu(h, fc1.weight, fc1.bias, norm=stats, gelu=False),
                                              lambda: F.conv1x1_gelu(z, fc1.weight, fc1.bias),
                                              lambda: nn.functional.gelu(nn.functional.linear(z_nhwc, fc1.weight, fc1.bias))], iters)
            yield dict(what=f"linear + gelu {shape} -> {4 * dim}", batch=n, ours_ms=ms, no_gelu_ms=ms_n, plain_loads_ms=ms_p, torch_ms=ms_t, kernel=name,
                       fused_equals_unfused=same, max_abs_diff_vs_torch=diff)
            w2, ls, zero = fc2.weight.view(dim, 4 * dim, 1, 1), blk.layer_scale.reshape(dim), CN._zeros(dim, x.device)
            y_nhwc, x_nhwc = y.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
            ms, ms_t = alternate([lambda: F.conv_norm_act(y, w2, fc2.bias, alpha=ls, beta=zero, residual=x, affine="mul_add"),
                                  lambda: x_nhwc + ls * nn.functional.linear(y_nhwc, fc2.weight, fc2.bias)], iters)
            F.conv_norm_act(y, w2, fc2.bias, alpha=ls, beta=zero, residual=x, affine="mul_add")
            yield dict(what=f"projection {4 * dim} -> {shape} (+ scale, + input)", batch=n, ours_ms=ms, torch_ms=ms_t, kernel=_lib.last_kernel(),
                       k_slices=list(F.conv1x1_k_slices(n, 4 * dim, side, side, dim)))
            rep_dev = rep.cuda()
            four, five = _with_fusion(True, lambda: blk(x)), _with_fusion(False, lambda: blk(x))
            same = bool(torch.equal(four(), five()))
            ms, ms_u, ms_t = alternate([four, five, lambda: rep_dev(x)], iters)
            yield dict(what=f"block {shape}: four launches | five | replica", batch=n, ours_ms=ms, unfused_ms=ms_u, torch_ms=ms_t, fused_equals_unfused=same)
            got, t32 = four().cpu().double(), rep_dev(x).cpu().double()
            f64 = rep.cpu().double()(x.cpu().double())
            rep.float()
            scale = float(f64.abs().max())
            yield dict(what=f"accuracy block {shape}", batch=n, library_err=float((got - f64).abs().max()) / scale * 2 ** 24,
                       torch_err=float((t32 - f64).abs().max()) / scale * 2 ** 24, k_slices=list(F.conv1x1_k_slices(n, 4 * dim, side, side, dim)))
        if forward:
            torch.manual_seed(0)
            rep = R.replica("convnext_tiny").eval()
            R.perturb(rep, 1)
            R.scale_weights(rep, 4.0)
            model = CN.convnext_tiny()
            model.load_state_dict(rep.state_dict(), strict=True)
            model, rep = model.cuda(), rep.cuda()
            img = rnd(n, 3, 224, 224)
            four, five = _with_fusion(True, lambda: model(img)), _with_fusion(False, lambda: model(img))
            out, want = four(), rep(img)
            ms, ms_u, ms_t = alternate([four, five, lambda: rep(img)], max(1, iters // 2))
            yield dict(what="convnext_tiny forward 224 x 224: four-launch blocks | five | replica", batch=n, ours_ms=ms, unfused_ms=ms_u, torch_ms=ms_t,
                       fused_equals_unfused=bool(torch.equal(out, five())), max_abs_diff_vs_torch=float((out - want).abs().max()),
                       max_abs_logit=float(want.abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 64])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--stages", nargs="+", type=int, default=[0, 1, 2, 3])
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default="profiles/perf_convnext.json")
    a = ap.parse_args()
    rows = []
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for n in a.batches:
        for row in rows_for(n, a.iters, [STAGES[i] for i in a.stages], not a.no_forward):
            rows.append(row)  # the series is kept row by row: a later shape that runs out of time loses nothing
            Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=7, rows=rows), indent=1) + "\n")
            if "library_err" in row:
                print(f"batch {row['batch']} {row['what']}: library {row['library_err']:.2f}, torch float32 replica {row['torch_err']:.2f} "
                      f"(x 2^-24 max|f64|), K slices {row['k_slices']}", flush=True)
                continue
            extra = f" {row['gb_per_s']:7.0f} GB/s" if "gb_per_s" in row else ""
            mid = "".join(f" | {k[:-3]} {row[k]:8.3f} ms" for k in ("no_gelu_ms", "plain_loads_ms", "unfused_ms") if k in row)
            print(f"batch {row['batch']} {row['what']}: {row['ours_ms']:8.3f} ms{mid} | torch {row['torch_ms']:8.3f} ms "
                  f"({row['torch_ms'] / row['ours_ms']:5.2f}x){extra} {row.get('kernel', '')}", flush=True)


if __name__ == "__main__":
    main()
