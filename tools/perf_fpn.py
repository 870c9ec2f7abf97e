#!/usr/bin/env python3
"""FeaturePyramidNetwork's top-down merge on one MI355X: the fused lateral (F.conv1x1_upsample_add: 1x1 conv + nearest upsample +
add in one launch) against the two ways to compute the same thing without it, on the same GPU, fp32:

  (a) composed  what the library offered before: F.conv_norm_act for the lateral, then torch's interpolate and add on the GPU;
  (b) torch     torch.nn's forward of the reference's module (nn.Conv2d, F.interpolate, +).

Shapes: every merging lateral of ResNet-50-FPN on an 800 x 800 image (256 -> 256 @ 200 x 200, 512 -> 256 @ 100 x 100, 1024 -> 256 @
50 x 50), then the whole FeaturePyramidNetwork([256, 512, 1024, 2048], 256) with LastLevelMaxPool, then one whole
resnet_fpn_backbone("resnet50") forward, at batch 1 and batch 8.

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  GB/s: the bytes the fused launch has to move (x, w, top once, y once) over its time; the roof is
8 TB/s of HBM.  All medians go to `--out` as JSON.

  python tools/perf_fpn.py [--batches 1 8] [--iters 5] [--out profiles/perf_fpn.json]
"""
import argparse
import json
import sys
from collections import OrderedDict
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
from torch import nn  # noqa: E402

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from tests import _fpn_ref as P  # noqa: E402  (the torch.nn replica of the reference's modules)
from tools.perf_detect import alternate  # noqa: E402

HBM_GBS = 8000.0
LATERALS = [(256, 200), (512, 100), (1024, 50)]  # (cin, side) of the merging levels; the top map is half the side


def lateral_rows(n, iters):
    rows = []
    for cin, side in LATERALS:
        x = torch.rand((n, cin, side, side), device="cuda") * 2 - 1
        top = torch.rand((n, 256, side // 2, side // 2), device="cuda") * 2 - 1
        conv = nn.Conv2d(cin, 256, 1).cuda()
        w, b = conv.weight.detach(), conv.bias.detach()
        fused = lambda: F.conv1x1_upsample_add(x, w, b, top=top)  # noqa: E731
        composed = lambda: F.conv_norm_act(x, w, b) + nn.functional.interpolate(top, size=(side, side), mode="nearest")  # noqa: E731
        plain = lambda: conv(x) + nn.functional.interpolate(top, size=(side, side), mode="nearest")  # noqa: E731
        with torch.no_grad():
            y = fused()
            kernel = _lib.last_kernel()
            assert torch.equal(y, composed()), "the fused lateral and the composition differ"
            err = float((y - plain()).abs().max())
            ms, ms_a, ms_b = alternate([fused, composed, plain], iters)
        nbytes = 4.0 * (x.numel() + w.numel() + top.numel() + y.numel())
        rows.append(dict(what=f"lateral {cin}->256 @{side}x{side}", batch=n, kernel=kernel, fused_ms=ms, composed_ms=ms_a, torch_ms=ms_b,
                         fused_gbs=nbytes / ms / 1e6, max_abs_diff_vs_torch=err))
    return rows


def fpn_row(n, iters):
    torch.manual_seed(0)
    replica = P.FeaturePyramidNetwork([256, 512, 1024, 2048], 256, extra_blocks=P.LastLevelMaxPool()).cuda().eval()
    ours = mv.FeaturePyramidNetwork([256, 512, 1024, 2048], 256, extra_blocks=mv.LastLevelMaxPool())
    ours.load_state_dict(replica.state_dict(), strict=True)
    ours = ours.cuda()
    feats = OrderedDict((str(i), torch.rand((n, c, s, s), device="cuda") * 2 - 1) for i, (c, s) in enumerate([(256, 200), (512, 100), (1024, 50), (2048, 25)]))

    def composed():  # the parent's pieces: every conv one library launch, interpolate and add torch's
        x = list(feats.values())
        last = ours.get_result_from_inner_blocks(x[-1], -1)
        out = [ours.get_result_from_layer_blocks(last, -1)]
        for i in range(len(x) - 2, -1, -1):
            lat = ours.get_result_from_inner_blocks(x[i], i)
            last = lat + nn.functional.interpolate(last, size=lat.shape[-2:], mode="nearest")
            out.insert(0, ours.get_result_from_layer_blocks(last, i))
        out.append(F.max_pool2d(out[-1], 1, 2, 0))
        return out
    with torch.no_grad():
        got, want = ours(feats), replica(feats)
        assert all(torch.equal(g, c) for g, c in zip(got.values(), composed())), "the fused pyramid and the composition differ"
        err = max(float((got[k] - want[k]).abs().max()) for k in want)
        ms, ms_a, ms_b = alternate([lambda: ours(feats), composed, lambda: replica(feats)], iters)
    return dict(what="FeaturePyramidNetwork([256, 512, 1024, 2048], 256) + pool @800x800", batch=n, fused_ms=ms, composed_ms=ms_a, torch_ms=ms_b,
                max_abs_diff_vs_torch=err)


def backbone_row(n, iters):
    torch.manual_seed(0)
    replica = P.resnet_fpn_backbone(backbone_name="resnet50").cuda().eval()
    ours = mv.resnet_fpn_backbone(backbone_name="resnet50")
    ours.load_state_dict(replica.state_dict(), strict=True)
    ours = ours.cuda()
    x = torch.rand((n, 3, 800, 800), device="cuda")
    with torch.no_grad():
        got, want = ours(x), replica(x)
        err = max(float((got[k] - want[k]).abs().max()) / float(want[k].abs().max()) for k in want)
        ms, ms_b = alternate([lambda: ours(x), lambda: replica(x)], iters)
    return dict(what='resnet_fpn_backbone("resnet50") @800x800', batch=n, fused_ms=ms, torch_ms=ms_b, max_rel_diff_vs_torch=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="profiles/perf_fpn.json")
    a = ap.parse_args()
    rows = []
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)

    def report(row):  # the series is kept row by row: a later shape that runs out of time loses nothing
        rows.append(row)
        Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=7, rows=rows), indent=1) + "\n")
        tail = "" if "composed_ms" not in row else f" | (a) composed {row['composed_ms']:8.3f} ms ({row['composed_ms'] / row['fused_ms']:5.2f}x)"
        gbs = "" if "fused_gbs" not in row else f"  {row['fused_gbs']:7.1f} GB/s ({row['fused_gbs'] / HBM_GBS * 100:4.1f}% HBM) [{row['kernel']}]"
        print(f"batch {row['batch']} {row['what']}: fused {row['fused_ms']:8.3f} ms{tail} | (b) torch {row['torch_ms']:8.3f} ms "
              f"({row['torch_ms'] / row['fused_ms']:5.2f}x){gbs}", flush=True)

    for n in a.batches:
        for row in lateral_rows(n, a.iters):
            report(row)
        report(fpn_row(n, a.iters))
        report(backbone_row(n, max(1, a.iters // 2)))


if __name__ == "__main__":
    main()
