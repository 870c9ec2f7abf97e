#!/usr/bin/env python3
"""MobileNetV3 inference on one MI355X against the torch replica of the reference (tests/_mobilenetv3_ref.py) on the same GPU, fp32.

Rows, per batch (1 and 64 by default):

  dw5x5             F.conv_norm_act on the 5x5 depthwise layers of mobilenet_v3_large at 224 x 224 (k_dwpc5x5) | torch's conv2d + batch_norm +
                    activation.  GB/s: the input read once and the output written once (4 B each per element) over the time
  global_avg_pool   F.global_avg_pool on the squeeze-excitation inputs (k_se_pool) | x.mean((2, 3)).  GB/s: the input read once
  linear_act        F.linear_act on fc1 / fc2 of the largest SE layer and on the classifier's Linear -> Hardswish (k_linear_act) | torch's
                    linear + activation.  GB/s: weight and x read once, y written once
  se_scale          F.se_scale (k_se_scale) | gate * x.  GB/s: x read, y written
  SE block          pool + two linear_act + the projection with input_scale (as the model runs it) | the unfused form, F.se_scale + the
                    plain projection | the replica's six torch ops + conv + batch_norm
  pointwise         the plain projection of the same shapes, which shares k_conv1x1's source with the gated instances (for the record
                    against profiles/perf_mobilenet*.json of earlier commits)
  forward           mobilenet_v3_large / mobilenet_v3_small at 224 x 224 | the replica's forward

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON.

  python tools/perf_mobilenetv3.py [--batches 1 64] [--iters 10] [--out profiles/perf_mobilenetv3.json]
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
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd.mobilenetv3 import mobilenet_v3_large, mobilenet_v3_small  # noqa: E402
from tests import _mobilenetv3_ref as R  # noqa: E402
from tools.perf_detect import alternate  # noqa: E402

# (channels, input side, stride, activation) of mobilenet_v3_large's 5x5 depthwise layers at 224 x 224, then (C, squeeze, side, cout) of
# its squeeze-excitation blocks (the side is the map the SE layer sees)
DW5 = [(72, 56, 2, "relu"), (120, 28, 1, "relu"), (672, 14, 2, "hardswish"), (960, 7, 1, "hardswish")]
SE = [(72, 24, 28, 40), (120, 32, 28, 40), (480, 120, 14, 112), (672, 168, 14, 112), (672, 168, 7, 160), (960, 240, 7, 160)]
TORCH_ACT = {"relu": torch.relu, "hardswish": nn.functional.hardswish, "hardsigmoid": nn.functional.hardsigmoid}


def rows_for(n, iters):
    g = torch.Generator(device="cuda").manual_seed(7 + n)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
    with torch.no_grad():
        for c, side, stride, act in DW5:
            x, w = rnd(n, c, side, side), rnd(c, 1, 5, 5) * 0.2
            a, b = rnd(c).abs() + 0.5, rnd(c)
            zeros, ones = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
            ours = lambda: F.conv_norm_act(x, w, None, a, b, stride=stride, groups=c, affine="fma", activation=act)  # noqa: E731
            theirs = lambda: TORCH_ACT[act](nn.functional.batch_norm(nn.functional.conv2d(x, w, None, stride, 2, 1, c), zeros, ones, a, b, False, 0.0, 1e-12))  # noqa: E731
            y = ours()
            name = _lib.last_kernel()
            diff = float((y - theirs()).abs().max())
            ms, ms_t = alternate([ours, theirs], iters)
            yield dict(what=f"dw5x5 {c} x {side} x {side} s{stride} {act}", batch=n, ours_ms=ms, torch_ms=ms_t, kernel=name,
                       gb_per_s=4.0 * (x.numel() + y.numel()) / (ms * 1e-3) / 1e9, max_abs_diff_vs_torch=diff)
        for c, sq, side, cout in SE:
            x = rnd(n, c, side, side)
            w1, b1, w2, b2 = rnd(sq, c, 1, 1) * 0.1, rnd(sq), rnd(c, sq, 1, 1) * 0.1, rnd(c)
            wp, a, b = rnd(cout, c, 1, 1) * 0.1, rnd(cout).abs() + 0.5, rnd(cout)
            zeros, ones = torch.zeros(cout, device="cuda"), torch.ones(cout, device="cuda")
            shape = f"{c} x {side} x {side}"
            ms, ms_t = alternate([lambda: F.global_avg_pool(x), lambda: x.mean((2, 3))], iters)
            yield dict(what=f"global_avg_pool {shape}", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_se_pool", gb_per_s=4.0 * x.numel() / (ms * 1e-3) / 1e9)
            pooled = F.global_avg_pool(x)
            hidden = F.linear_act(pooled, w1, b1, "relu")
            gate = F.linear_act(hidden, w2, b2, "hardsigmoid")
            for label, inp, w, bias, act in (("fc1 + ReLU", pooled, w1, b1, "relu"), ("fc2 + Hardsigmoid", hidden, w2, b2, "hardsigmoid")):
                w2d = w.reshape(w.shape[0], -1)
                ms, ms_t = alternate([lambda: F.linear_act(inp, w, bias, act), lambda: TORCH_ACT[act](nn.functional.linear(inp, w2d, bias))], iters)
                yield dict(what=f"linear_act {label} {w2d.shape[1]} -> {w2d.shape[0]}", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_linear_act",
                           gb_per_s=4.0 * (w2d.numel() + inp.numel() + n * w2d.shape[0]) / (ms * 1e-3) / 1e9)
            ms, ms_t = alternate([lambda: F.se_scale(x, gate), lambda: gate.view(n, c, 1, 1) * x], iters)
            yield dict(what=f"se_scale {shape}", batch=n, ours_ms=ms, torch_ms=ms_t, kernel=_lib.last_kernel(), gb_per_s=8.0 * x.numel() / (ms * 1e-3) / 1e9)

            def fused():
                gt = F.squeeze_excitation_gate(x, w1, b1, w2, b2, "relu", "hardsigmoid")
                return F.conv_norm_act(x, wp, None, a, b, affine="fma", input_scale=gt)

            def unfused():
                return F.conv_norm_act(F.squeeze_excitation(x, w1, b1, w2, b2, "relu", "hardsigmoid"), wp, None, a, b, affine="fma")

            def replica():
                s = nn.functional.hardsigmoid(nn.functional.conv2d(torch.relu(nn.functional.conv2d(nn.functional.adaptive_avg_pool2d(x, 1), w1, b1)), w2, b2))
                return nn.functional.batch_norm(nn.functional.conv2d(s * x, wp), zeros, ones, a, b, False, 0.0, 1e-12)

            same = bool(torch.equal(fused(), unfused()))
            name = _lib.last_kernel()
            diff = float((fused() - replica()).abs().max())
            ms, ms_u, ms_t = alternate([fused, unfused, replica], iters)
            yield dict(what=f"SE block {shape} -> {cout}: gate + gated projection", batch=n, ours_ms=ms, unfused_ms=ms_u, torch_ms=ms_t,
                       fused_equals_unfused=same, max_abs_diff_vs_torch=diff)
            ms, ms_t = alternate([lambda: F.conv_norm_act(x, wp, None, a, b, affine="fma"),
                                  lambda: nn.functional.batch_norm(nn.functional.conv2d(x, wp), zeros, ones, a, b, False, 0.0, 1e-12)], iters)
            yield dict(what=f"pointwise {shape} -> {cout} (no gate)", batch=n, ours_ms=ms, torch_ms=ms_t, kernel=name)
        x, w, bias = rnd(n, 960), rnd(1280, 960) * 0.05, rnd(1280)
        ms, ms_t = alternate([lambda: F.linear_act(x, w, bias, "hardswish"), lambda: nn.functional.hardswish(nn.functional.linear(x, w, bias))], iters)
        yield dict(what="linear_act classifier 960 -> 1280 + Hardswish", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_linear_act",
                   gb_per_s=4.0 * (w.numel() + x.numel() + n * 1280) / (ms * 1e-3) / 1e9)
        for arch, builder in (("mobilenet_v3_large", mobilenet_v3_large), ("mobilenet_v3_small", mobilenet_v3_small)):
            torch.manual_seed(0)
            rep = R.replica(arch).eval()
            R.perturb(rep, 1)
            model = builder()
            model.load_state_dict(rep.state_dict(), strict=True)
            model, rep = model.cuda(), rep.cuda()
            img = rnd(n, 3, 224, 224)
            diff = float((model(img) - rep(img)).abs().max())
            ms, ms_t = alternate([lambda: model(img), lambda: rep(img)], max(1, iters // 2))
            yield dict(what=f"{arch} forward 224 x 224", batch=n, ours_ms=ms, torch_ms=ms_t, max_abs_diff_vs_torch=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 64])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="profiles/perf_mobilenetv3.json")
    a = ap.parse_args()
    rows = []
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for n in a.batches:
        for row in rows_for(n, a.iters):
            rows.append(row)  # the series is kept row by row: a later shape that runs out of time loses nothing
            Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=7, rows=rows), indent=1) + "\n")
            extra = f" {row['gb_per_s']:7.0f} GB/s" if "gb_per_s" in row else ""
            mid = f" | unfused {row['unfused_ms']:8.3f} ms" if "unfused_ms" in row else ""
            print(f"batch {row['batch']} {row['what']}: {row['ours_ms']:8.3f} ms{mid} | torch {row['torch_ms']:8.3f} ms "
                  f"({row['torch_ms'] / row['ours_ms']:5.2f}x){extra}", flush=True)


if __name__ == "__main__":
    main()
