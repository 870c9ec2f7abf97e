#!/usr/bin/env python3
"""RegionProposalNetwork inference on one MI355X against the torch replica of the reference (tests/_rpn_ref.py) on the same GPU, fp32.

Shapes: ResNet-50-FPN on an 800 x 800 image -- five 256-channel levels of 200, 100, 50, 25 and 13 pixels a side, 3 anchors per
location (159 882 anchors per image), pre_nms_top_n 1000, post_nms_top_n 1000, nms 0.7 -- at batch 1 and batch 8.  Rows:

  head @side     RPNHead on one level: conv3x3 + ReLU, then cls_logits and bbox_pred as one pointwise launch | nn.Conv2d x 3
  topk           F.rpn_topk on the head's NCHW logits | permute + reshape + cat of every logit, torch.topk per level
  decode         F.rpn_decode of the 4 507 selected candidates | every anchor generated and decoded, then gather, sigmoid, clip
  topk + decode  the two together | the replica's path up to the per-image filters
  forward        RegionProposalNetwork.forward | the replica's forward; BOTH sides run the package's ops.nms (torch has no nms of its
                 own: the comparison is of everything before it)
  exp            the decode arithmetic on flat arrays with E = (float)exp((double)v), the library's, against expf (tools/micro/
                 rpn_decode_exp.hip, built on first use): what the exactness costs.  Not a library kernel.

Times are HIP events, the median over 7 rounds of `--iters` calls after a warm-up, the sides taking turns round by round
(tools/perf_detect.alternate).  All medians go to `--out` as JSON.

  python tools/perf_rpn.py [--batches 1 8] [--iters 5] [--out profiles/perf_rpn.json]
"""
import argparse
import ctypes as C
import json
import subprocess
import sys
from collections import OrderedDict
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd import _lib, ops  # noqa: E402
from tests import _rpn_ref as P  # noqa: E402  (the torch replica of the reference's modules)
from tools.perf_detect import alternate  # noqa: E402

SIDES = [200, 100, 50, 25, 13]
IMAGE = 800
PRE, POST, NMS = 1000, 1000, 0.7


def build_pair():
    torch.manual_seed(0)
    replica_head = P.RPNHead(256, 3).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # the init's std of 0.01 leaves every proposal on its anchor
        for p in replica_head.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.03)
    head = mv.RPNHead(256, 3)
    head.load_state_dict(replica_head.state_dict(), strict=True)
    top_n = ({"training": 2000, "testing": PRE}, {"training": 2000, "testing": POST})
    ours = mv.RegionProposalNetwork(mv.AnchorGenerator(P.FPN_SIZES, P.FPN_RATIOS), head, 0.7, 0.3, 256, 0.5, *top_n, NMS).cuda()
    replica = P.RegionProposalNetwork(P.AnchorGenerator(P.FPN_SIZES, P.FPN_RATIOS), replica_head, 0.7, 0.3, 256, 0.5, *top_n, NMS).cuda().eval()
    return ours, replica


def rows_for(n, iters):
    ours, replica = build_pair()
    feats = OrderedDict((str(i), torch.rand((n, 256, s, s), device="cuda") * 2 - 1) for i, s in enumerate(SIDES))
    sizes = [(IMAGE, IMAGE - 16 * (i % 2)) for i in range(n)]
    images, ref_images = mv.ImageList(torch.zeros((n, 3, IMAGE, IMAGE), device="cuda"), sizes), P.ImageList(torch.zeros((n, 3, IMAGE, IMAGE), device="cuda"), sizes)
    with torch.no_grad():
        for name, x in feats.items():
            side = x.shape[-1]
            ms, ms_t = alternate([lambda: ours.head([x]), lambda: replica.head([x])], iters)
            (lg,), (bb,) = ours.head([x])
            (lg_t,), (bb_t,) = replica.head([x])
            err = max(float((lg - lg_t).abs().max()), float((bb - bb_t).abs().max()))
            yield dict(what=f"head @{side}x{side}", batch=n, ours_ms=ms, torch_ms=ms_t, max_abs_diff_vs_torch=err)
        ob, dl = ours.head(list(feats.values()))
        ob_t, dl_t = [o.contiguous() for o in ob], [d.contiguous() for d in dl]  # the replica on the same numbers
        strides = [(IMAGE // s, IMAGE // s) for s in SIDES]
        cells = ours.anchor_generator.cell_anchors
        per_level = [int(o[0].numel()) for o in ob]

        def torch_topk():
            flat, _ = P.concat_box_prediction_layers(ob_t, dl_t)
            return replica._get_top_n_idx(flat.reshape(n, -1), per_level)

        def torch_decode(idx):
            anchors = replica.anchor_generator(ref_images, ob_t)
            flat, deltas = P.concat_box_prediction_layers(ob_t, dl_t)
            proposals = replica.box_coder.decode(deltas, anchors).view(n, -1, 4)
            batch = torch.arange(n, device="cuda")[:, None]
            scores = torch.sigmoid(flat.reshape(n, -1)[batch, idx])
            return torch.stack([P.clip_boxes_to_image(b, s) for b, s in zip(proposals[batch, idx], sizes)]), scores

        idx = F.rpn_topk(ob, PRE)
        idx_t = torch_topk()
        same_sets = bool(torch.equal(idx.long().sort(1)[0], idx_t.sort(1)[0]))
        ms, ms_t = alternate([lambda: F.rpn_topk(ob, PRE), torch_topk], iters)
        yield dict(what=f"topk {PRE} per level of {sum(per_level)} anchors", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_rpn_topk",
                   same_index_sets=same_sets)
        decode = lambda: F.rpn_decode(ob, dl, idx, cells, strides, sizes)  # noqa: E731
        boxes, scores, _, _ = decode()
        boxes_t, scores_t = torch_decode(idx.long())
        err = float((boxes - boxes_t).abs().max())
        ms, ms_t = alternate([decode, lambda: torch_decode(idx_t)], iters)
        yield dict(what=f"decode {idx.shape[1]} candidates", batch=n, ours_ms=ms, torch_ms=ms_t, kernel="k_rpn_decode",
                   max_abs_diff_vs_torch=err, max_score_diff_vs_torch=float((scores - scores_t).abs().max()))
        ms, ms_t = alternate([lambda: F.rpn_decode(ob, dl, F.rpn_topk(ob, PRE), cells, strides, sizes),
                              lambda: replica.from_head_outputs(ref_images, ob_t, dl_t, detailed=True)], iters)
        yield dict(what="topk + decode", batch=n, ours_ms=ms, torch_ms=ms_t)
        P.nms = ops.nms  # the replica's nms is a numpy restatement: both sides run the package's kernel
        got, _ = ours(images, feats)
        want, _ = replica(ref_images, feats)
        ms, ms_t = alternate([lambda: ours(images, feats), lambda: replica(ref_images, feats)], max(1, iters // 2))
        yield dict(what="RegionProposalNetwork.forward", batch=n, ours_ms=ms, torch_ms=ms_t, proposals=[len(b) for b in got],
                   torch_proposals=[len(b) for b in want])
        yield exp_row(n, idx.shape[1], iters)


def exp_row(n, k, iters):
    """The decode arithmetic with the library's exp and with expf, on n * k candidates."""
    src = ROOT / "tools" / "micro" / "rpn_decode_exp.hip"
    so = src.with_name("librpn_decode_exp.so")
    if not so.exists() or so.stat().st_mtime < src.stat().st_mtime:
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    fn = C.CDLL(str(so)).rpn_decode_exp
    fn.restype, fn.argtypes = C.c_int, [C.c_int] + [C.c_void_p] * 5 + [C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_void_p]
    count = n * k
    p = torch.rand((count, 2), device="cuda") * 700
    anchors = torch.cat([p, p + 32 + torch.rand((count, 2), device="cuda") * 400], 1).contiguous()
    deltas, logits = torch.randn((count, 4), device="cuda"), torch.randn(count, device="cuda") * 3
    out = [(torch.empty((count, 4), device="cuda"), torch.empty(count, device="cuda")) for _ in range(2)]

    def run(expf):
        b, s = out[expf]
        rc = fn(expf, anchors.data_ptr(), deltas.data_ptr(), logits.data_ptr(), b.data_ptr(), s.data_ptr(), count, F.BBOX_XFORM_CLIP, float(IMAGE),
                float(IMAGE), _lib.stream_ptr(anchors))
        assert rc == 0, rc
    ms, ms_f = alternate([lambda: run(0), lambda: run(1)], iters * 4)
    differ = float((out[0][0] != out[1][0]).any(1).float().mean())
    return dict(what=f"decode arithmetic on {count} candidates: (float)exp((double)v) | expf", batch=n, ours_ms=ms, torch_ms=ms_f,
                boxes_that_differ=differ, max_abs_diff=float((out[0][0] - out[1][0]).abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="profiles/perf_rpn.json")
    a = ap.parse_args()
    rows = []
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for n in a.batches:
        for row in rows_for(n, a.iters):
            rows.append(row)  # the series is kept row by row: a later shape that runs out of time loses nothing
            Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=7, rows=rows), indent=1) + "\n")
            print(f"batch {row['batch']} {row['what']}: {row['ours_ms']:8.3f} ms | {row['torch_ms']:8.3f} ms ({row['torch_ms'] / row['ours_ms']:5.2f}x)",
                  flush=True)


if __name__ == "__main__":
    main()
