#!/usr/bin/env python3
"""FCN / DeepLabV3 inference and the fused upsample + argmax on one MI355X against torch on the same GPU, fp32.

Rows:

  interpolate_argmax   F.interpolate_argmax (k_interp_argmax) on (n, 21, 65, 65) -> 520 x 520 for n = 1 and 8, int64 and uint8 labels |
                       the library's F.interpolate(...).argmax(1) | torch's interpolate(...).argmax(1) (uint8: + .to(torch.uint8)).
                       GB/s: the bytes the fused form needs, the source read once and the labels written once, over its time; the
                       composition moves 84 + 84 + 8 bytes per output pixel
  forward              fcn_resnet50 / deeplabv3_resnet50 at 1 x 3 x 520 x 520 | the torch replica's forward (tests/_segmentation_ref.py)
  labels               model.labels(x) | model(x)["out"].argmax(1) of the library | the replica's
  dilated depthwise    (--only mobile) F.conv_norm_act(dilation=2) + BatchNorm2d fold + Hardswish (k_dwpc5x5<1, 2>) on n x 672 | 960 x 33 x 33,
                       n = 1 and 8 | the undilated k_dwpc5x5 on the same shape (the memory-traffic yardstick) | torch's conv2d(groups=c,
                       dilation=2) + batch_norm + hardswish
  LRASPP head launch   F.conv1x1_gated_upsample on n x 128 x 33 x 33 -> 65 x 65, 21 classes | the library's unfused composition (F.se_scale,
                       F.interpolate, F.conv_norm_act: 3 launches, two more tensors written: bytes_not_written) | the same in torch
  mobile models        lraspp_mobilenet_v3_large / deeplabv3_mobilenet_v3_large forward and labels at 520 x 520, batch 1 and 8 | the torch
                       replica (tests/_lraspp_ref.py)

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON.

  python tools/perf_segmentation.py [--iters 20] [--only all|resnet|mobile] [--out profiles/perf_segmentation.json]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
from torch import nn  # noqa: E402

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from tests import _lraspp_ref as LR  # noqa: E402
from tests import _segmentation_ref as R  # noqa: E402
from tools.perf_detect import alternate  # noqa: E402

CLASSES, FEATURE, IMAGE = 21, 65, 520


def rows_for(iters):
    g = torch.Generator(device="cuda").manual_seed(11)
    with torch.no_grad():
        for n in (1, 8):
            x = torch.randn((n, CLASSES, FEATURE, FEATURE), device="cuda", generator=g)
            for dtype in (torch.int64, torch.uint8):
                fused = lambda: F.interpolate_argmax(x, size=(IMAGE, IMAGE), dtype=dtype)  # noqa: E731
                composed = lambda: F.interpolate(x, size=(IMAGE, IMAGE)).argmax(1).to(dtype)  # noqa: E731
                theirs = lambda: nn.functional.interpolate(x, size=(IMAGE, IMAGE), mode="bilinear", align_corners=False).argmax(1).to(dtype)  # noqa: E731
                y = fused()
                name = _lib.last_kernel()
                same = bool(torch.equal(y, composed()))
                agree = float((y == theirs()).float().mean())
                ms, ms_c, ms_t = alternate([fused, composed, theirs], iters)
                needed = 4.0 * x.numel() + y.numel() * y.element_size()
                yield dict(what=f"interpolate_argmax {CLASSES} x {FEATURE} x {FEATURE} -> {IMAGE} x {IMAGE} {str(dtype)[6:]}", batch=n, ours_ms=ms,
                           composed_ms=ms_c, torch_ms=ms_t, kernel=name, gb_per_s=needed / (ms * 1e-3) / 1e9, fused_equals_composed=same,
                           labels_equal_to_torch=agree)
        for arch in ("fcn_resnet50", "deeplabv3_resnet50"):
            torch.manual_seed(0)
            rep = R.replica(arch)
            R.perturb(rep, 1)
            model = getattr(mv, arch)()
            model.load_state_dict(rep.state_dict(), strict=True)
            model, rep = model.cuda(), rep.cuda()
            img = torch.randn((1, 3, IMAGE, IMAGE), device="cuda", generator=g)
            out, out_t = model(img)["out"], rep(img)["out"]
            diff = float((out - out_t).abs().max())
            ms, ms_t = alternate([lambda: model(img), lambda: rep(img)], max(1, iters // 4))
            yield dict(what=f"{arch} forward {IMAGE} x {IMAGE}", batch=1, ours_ms=ms, torch_ms=ms_t, max_abs_diff_vs_torch=diff,
                       max_abs=float(out_t.abs().max()))
            same = bool(torch.equal(model.labels(img), out.argmax(1)))
            ms, ms_c, ms_t = alternate([lambda: model.labels(img), lambda: model(img)["out"].argmax(1), lambda: rep(img)["out"].argmax(1)],
                                       max(1, iters // 4))
            yield dict(what=f"{arch} labels {IMAGE} x {IMAGE}", batch=1, ours_ms=ms, composed_ms=ms_c, torch_ms=ms_t, fused_equals_composed=same)


def mobile_rows_for(iters):
    g = torch.Generator(device="cuda").manual_seed(12)
    tf = nn.functional
    with torch.no_grad():
        for c in (672, 960):
            for n in (1, 8):
                x = torch.randn((n, c, 33, 33), device="cuda", generator=g)
                w = torch.randn((c, 1, 5, 5), device="cuda", generator=g) * 0.2
                bn = [torch.rand(c, device="cuda", generator=g) + 0.5 for _ in range(4)]  # weight, bias, mean, var
                alpha, beta = F.fold_batchnorm(bn[0].cpu(), bn[1].cpu(), bn[2].cpu(), bn[3].cpu(), 1e-3)
                alpha, beta = alpha.cuda(), beta.cuda()
                ours = lambda: F.conv_norm_act(x, w, None, alpha, beta, groups=c, affine="fma", activation="hardswish", dilation=2)  # noqa: E731
                undilated = lambda: F.conv_norm_act(x, w, None, alpha, beta, groups=c, affine="fma", activation="hardswish")  # noqa: E731
                theirs = lambda: tf.hardswish(tf.batch_norm(tf.conv2d(x, w, None, 1, 4, 2, c), bn[2], bn[3], bn[0], bn[1], False, 0.0, 1e-3))  # noqa: E731
                y = ours()
                name = _lib.last_kernel()
                diff = float((y - theirs()).abs().max())
                ms, ms_u, ms_t = alternate([ours, undilated, theirs], iters)
                yield dict(what=f"depthwise 5x5 dilation 2 + norm + hardswish {c} x 33 x 33", batch=n, ours_ms=ms, undilated_ms=ms_u, torch_ms=ms_t,
                           kernel=name, gb_per_s=8.0 * x.numel() / (ms * 1e-3) / 1e9, max_abs_diff_vs_torch=diff)
        for n in (1, 8):
            x = torch.randn((n, 128, 33, 33), device="cuda", generator=g)
            gate, w = torch.rand((n, 128), device="cuda", generator=g), torch.randn((CLASSES, 128, 1, 1), device="cuda", generator=g) * 0.1
            bias, res = torch.randn(CLASSES, device="cuda", generator=g), torch.randn((n, CLASSES, FEATURE, FEATURE), device="cuda", generator=g)
            fused = lambda: F.conv1x1_gated_upsample(x, gate, w, bias, res, size=(FEATURE, FEATURE))  # noqa: E731
            composed = lambda: F.conv_norm_act(F.interpolate(F.se_scale(x, gate), size=(FEATURE, FEATURE)), w, bias, residual=res)  # noqa: E731
            theirs = lambda: res + tf.conv2d(tf.interpolate(x * gate[:, :, None, None], size=(FEATURE, FEATURE), mode="bilinear",  # noqa: E731
                                                            align_corners=False), w, bias)
            y = fused()
            name = _lib.last_kernel()
            same = bool(torch.equal(y, composed()))
            ms, ms_c, ms_t = alternate([fused, composed, theirs], iters)
            yield dict(what=f"LRASPP head launch 128 x 33 x 33 -> {FEATURE} x {FEATURE}, {CLASSES} classes", batch=n, ours_ms=ms, composed_ms=ms_c,
                       torch_ms=ms_t, kernel=name, launches=1, composed_launches=3, fused_equals_composed=same,
                       bytes_not_written=4 * (x.numel() + n * 128 * FEATURE * FEATURE))
        for arch in ("lraspp_mobilenet_v3_large", "deeplabv3_mobilenet_v3_large"):
            torch.manual_seed(0)
            rep = LR.replica(arch)
            LR.MR.perturb(rep, 1)
            model = getattr(mv, arch)()
            model.load_state_dict(rep.state_dict(), strict=True)
            model, rep = model.cuda(), rep.cuda()
            for n in (1, 8):
                img = torch.randn((n, 3, IMAGE, IMAGE), device="cuda", generator=g)
                out, out_t = model(img)["out"], rep(img)["out"]
                diff = float((out - out_t).abs().max())
                ms, ms_t = alternate([lambda: model(img), lambda: rep(img)], max(1, iters // 4))
                yield dict(what=f"{arch} forward {IMAGE} x {IMAGE}", batch=n, ours_ms=ms, torch_ms=ms_t, max_abs_diff_vs_torch=diff,
                           max_abs=float(out_t.abs().max()))
                same = bool(torch.equal(model.labels(img), out.argmax(1)))
                ms, ms_c, ms_t = alternate([lambda: model.labels(img), lambda: model(img)["out"].argmax(1), lambda: rep(img)["out"].argmax(1)],
                                           max(1, iters // 4))
                yield dict(what=f"{arch} labels {IMAGE} x {IMAGE}", batch=n, ours_ms=ms, composed_ms=ms_c, torch_ms=ms_t, fused_equals_composed=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=["all", "resnet", "mobile"], default="all")
    ap.add_argument("--out", default="profiles/perf_segmentation.json")
    a = ap.parse_args()
    rows = []
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    import itertools
    series = [rows_for(a.iters)] * (a.only != "mobile") + [mobile_rows_for(a.iters)] * (a.only != "resnet")
    for row in itertools.chain(*series):
        rows.append(row)  # the series is kept row by row: a later shape that runs out of time loses nothing
        Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=7, rows=rows), indent=1) + "\n")
        extra = f" {row['gb_per_s']:7.0f} GB/s" if "gb_per_s" in row else ""
        mid = f" | composed {row['composed_ms']:8.3f} ms" if "composed_ms" in row else ""
        mid += f" | undilated {row['undilated_ms']:8.3f} ms" if "undilated_ms" in row else ""
        print(f"batch {row['batch']} {row['what']}: {row['ours_ms']:8.3f} ms{mid} | torch {row['torch_ms']:8.3f} ms "
              f"({row['torch_ms'] / row['ours_ms']:5.2f}x){extra}", flush=True)


if __name__ == "__main__":
    main()
