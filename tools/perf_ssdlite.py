#!/usr/bin/env python3
"""SSDlite inference on one MI355X: the fused depthwise-separable launch (F.dwconv_pointwise, k_conv1x1_dw) against the composition of
existing calls it replaces, and the whole model against the torch replica of the reference (tests/_ssdlite_ref.py) on the same GPU, fp32.

Shapes: ssdlite320_mobilenet_v3_large -- six maps of 672 x 20^2, 480 x 10^2, 512 x 5^2, 256 x 3^2, 256 x 2^2 and 128 x 1^2, 6 default
boxes per cell (3 234 anchors), 91 classes -- at batch 1 and batch 32.  Rows:

  head site        one prediction block (level, head): F.dwconv_pointwise | F.conv_norm_act (depthwise) + F.conv_norm_act (1x1)
  head, all fused  SSDLiteHead.forward with every prediction block fused, 12 launches | with every block as two launches, 24
  head             SSDLiteHead.forward as it dispatches (ssdlite._use_fused: fused where that won) | the same 24 launches
  extra site       the back half of one extra block (stride-2 depthwise + 1x1, both with norm and ReLU6): fused | composed
  extra blocks     the four extra blocks: 4 x (1x1 + fused) | 4 x (1x1 + depthwise + 1x1)
  forward          SSD.forward | the replica's forward (torch convs, its own transform); BOTH sides run the package's nms

Every fused | composed row also times the fused side a second time in the same rounds: `spread_ms` is the difference of the two medians
of the same code, the yardstick for calling a difference a loss.  Times are HIP events, the median over 7 rounds of `--iters` calls after
a warm-up, the sides taking turns round by round (tools/perf_detect.alternate).  All medians go to `--out` as JSON.

  python tools/perf_ssdlite.py [--batches 1 32] [--iters 20] [--out profiles/perf_ssdlite.json]
"""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
os.environ.setdefault("MI355VISION_LIB", str(ROOT / "cpu-vision_amd" / "lib" / "libmi355vision_tuning.so"))
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd import ops  # noqa: E402
from cpu_vision_amd import ssdlite as SLM  # noqa: E402
from cpu_vision_amd.ssdlite import _separable  # noqa: E402
from tests import _rpn_ref as P  # noqa: E402
from tests import _ssdlite_ref as RL  # noqa: E402  (the torch replica of the reference's modules)
from tools.perf_detect import alternate  # noqa: E402

MAPS = [(672, 20), (480, 10), (512, 5), (256, 3), (256, 2), (128, 1)]


def _composed(x, depthwise, pointwise):
    """What _separable replaces, as existing calls: the depthwise Conv2dNormActivation, then the 1x1 conv (an nn.Conv2d with its bias or
    a Conv2dNormActivation)."""
    hidden = depthwise(x)
    if isinstance(pointwise, torch.nn.Conv2d):
        return F.conv_norm_act(hidden, pointwise.weight, pointwise.bias)
    return pointwise(hidden)


def _pair(what, n, fused, composed, iters, **extra):
    same = bool(torch.equal(fused().view(torch.int32), composed().view(torch.int32))) if extra.pop("compare", True) else None
    a, c, b = alternate([fused, composed, fused], iters)
    return dict(what=what, batch=n, fused_ms=min(a, b), composed_ms=c, spread_ms=abs(a - b), same_bits=same, **extra)


def rows_for(n, iters):
    g = torch.Generator(device="cuda").manual_seed(5 + n)
    with torch.no_grad():
        torch.manual_seed(0)
        model = mv.ssdlite320_mobilenet_v3_large()
        replica = RL.ssdlite320_mobilenet_v3_large()
        replica.load_state_dict(model.state_dict(), strict=True)
        model, replica = model.cuda(), replica.eval().cuda()
        P.nms = ops.nms  # the replica's nms is a numpy restatement: both sides run the package's kernel
        feats = [torch.randn((n, c, s, s), device="cuda", generator=g).relu_() for c, s in MAPS]
        head = model.head
        for name, sub in (("cls", head.classification_head), ("reg", head.regression_head)):
            for level, (block, x) in enumerate(zip(sub.module_list, feats)):
                fused = lambda block=block, x=x: _separable(x, block[0], block[1], True)  # noqa: E731
                composed = lambda block=block, x=x: _composed(x, block[0], block[1])  # noqa: E731
                fused()
                yield _pair(f"head site {name} level {level}: {tuple(x.shape[1:])} -> {block[1].out_channels}", n, fused, composed, iters,
                            kernel=_lib.last_kernel())
        def head_with(rule):  # SSDLiteHead.forward with the dispatch rule replaced: the same module plumbing on either side
            def run():
                kept = SLM._use_fused
                SLM._use_fused = rule or kept
                try:
                    return head(feats)
                finally:
                    SLM._use_fused = kept
            return run
        composed = head_with(lambda cin, cout: False)
        yield _pair("head, all fused: 12 launches | 24 launches", n, head_with(lambda cin, cout: True), composed, iters, compare=False)
        yield _pair("head as dispatched (SSDLiteHead.forward) | 24 launches", n, head_with(None), composed, iters, compare=False)

        extra = model.backbone.extra
        mids = []
        x = feats[1]
        for i, block in enumerate(extra):
            mid = block[0](x)
            mids.append(mid)
            fused = lambda block=block, mid=mid: _separable(mid, block[1], block[2], True)  # noqa: E731
            composed = lambda block=block, mid=mid: _composed(mid, block[1], block[2])  # noqa: E731
            x = fused()
            yield _pair(f"extra site {i}: {tuple(mid.shape[1:])} -> {block[2].out_channels} at stride 2", n, fused, composed, iters,
                        kernel=_lib.last_kernel())

        def run_extra(sep):
            t = feats[1]
            for block in extra:
                t = sep(block[0](t), block[1], block[2])
            return t
        yield _pair("extra blocks: 4 x (1x1 + fused) | 4 x (1x1 + depthwise + 1x1)", n, lambda: run_extra(lambda t, a, b: _separable(t, a, b, True)), lambda: run_extra(_composed),
                    iters)

        imgs = [torch.rand((3, 480, 640 - 16 * (i % 2)), device="cuda", generator=g) for i in range(n)]
        got, want = model(imgs), replica(imgs)
        ms, ms_t = alternate([lambda: model(imgs), lambda: replica(imgs)], max(1, iters // 4))
        yield dict(what="SSD.forward ssdlite320_mobilenet_v3_large", batch=n, ours_ms=ms, torch_ms=ms_t, detections=[len(d["boxes"]) for d in got][:4],
                   torch_detections=[len(d["boxes"]) for d in want][:4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 32])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="profiles/perf_ssdlite.json")
    a = ap.parse_args()
    rows = []
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for n in a.batches:
        for row in rows_for(n, a.iters):
            rows.append(row)  # the series is kept row by row: a later shape that runs out of time loses nothing
            Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=7, rows=rows), indent=1) + "\n")
            if "fused_ms" in row:
                print(f"batch {row['batch']} {row['what']}: fused {row['fused_ms']:7.4f} ms | composed {row['composed_ms']:7.4f} ms "
                      f"({row['composed_ms'] / row['fused_ms']:5.2f}x), same-code spread {row['spread_ms']:.4f} ms {row.get('kernel', '')}", flush=True)
            else:
                print(f"batch {row['batch']} {row['what']}: {row['ours_ms']:8.3f} ms | {row['torch_ms']:8.3f} ms "
                      f"({row['torch_ms'] / row['ours_ms']:5.2f}x)", flush=True)


if __name__ == "__main__":
    main()
