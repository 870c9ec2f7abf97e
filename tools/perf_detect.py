#!/usr/bin/env python3
"""ops.nms, ops.roi_align, ops.roi_pool, ops.ps_roi_pool and ops.ps_roi_align on one MI355X: time per call (HIP events, median of 7 rounds of `--iters` back-to-back calls after a
warm-up, the two sides of a comparison alternating round by round) against the same op on the same GPU -- torchvision's own
when that package is importable, otherwise a restatement in torch ops:

  nms        sort + the (n, n) IoU matrix + the greedy walk over its rows as a host loop that reads each decision back -- what a
             user without a native kernel writes.  The walk costs a host round trip per kept box, so its time is mostly that.
  roi_align  the reference's own pure-torch formulation (ops/roi_align.py _roi_align: masked gathers over a (K, C, PH, PW, IY, IX)
             index space) for a fixed sampling_ratio.

  box_iou / generalized_box_iou / distance_box_iou   the reference's chain of broadcast torch ops (ops/boxes.py) on the same GPU.
  masks_to_boxes      the reference's loop, a torch.where per mask (one host round trip each).
  MultiScaleRoIAlign  the reference's per-level loop (torch.where, gather, roi_align, scatter) built from ops.roi_align: the same
                      kernel arithmetic, so the difference is the syncs, gathers and scatters.

  python tools/perf_detect.py [--iters 5] [--pooling-only] [--boxes-only]

Cases: nms at 1 000 / 4 000 / 20 000 clustered boxes (threshold 0.5); roi_align at 1 000 rois x 256
channels x 7 x 7 on a 2 x 256 x 200 x 304 map (spatial_scale 0.25, sampling_ratio 2, aligned), with the bytes it must move
(the output once; the map's touched part at most once) against the 8 TB/s HBM peak; roi_pool / ps_roi_pool / ps_roi_align at
1 000 rois x 7 x 7 on a 2 x 256 x 50 x 68 map (spatial_scale 0.25; 245 = 5 x 49 channels for the position-sensitive ops;
ps_roi_align with sampling_ratio 2) against torchvision's op on the GPU where that package is importable -- otherwise the op's
own time and the bytes it moves are printed, without a baseline."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from cpu_vision_amd import _lib, ops  # noqa: E402

try:
    import torchvision.ops as tv_ops
except Exception:
    tv_ops = None

PEAK_TBS = 8.0


def alternate(fns, iters, rounds=7):
    """Median ms per call of each fn, the fns taking turns round by round."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / iters)
    return [sorted(t)[len(t) // 2] for t in ts]


def boxes(n, seed=0):
    """Clusters of jittered boxes, 8 per centre on average, as a detector's raw output has them."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.rand((n // 8 + 1, 2), device="cuda", generator=g) * 1000
    c = centres[torch.randint(0, n // 8 + 1, (n,), device="cuda", generator=g)] + torch.randn((n, 2), device="cuda", generator=g) * 4
    wh = 20 + torch.rand((n, 2), device="cuda", generator=g) * 30
    return torch.cat([c - wh / 2, c + wh / 2], 1).contiguous(), torch.rand(n, device="cuda", generator=g)


def torch_nms(b, s, thr):
    order = torch.sort(s, stable=True, descending=True).indices
    b = b[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt, rb = torch.max(b[:, None, :2], b[None, :, :2]), torch.min(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    over = (inter / (area[:, None] + area[None, :] - inter) > thr).triu(1)
    removed = torch.zeros(len(b), dtype=torch.bool, device=b.device)
    keep = []
    for i in range(len(b)):
        if not removed[i]:  # one read-back per box
            keep.append(i)
            removed |= over[i]
    return order[torch.tensor(keep, device=b.device)]


def torch_roi_align(x, rois, scale, ph_n, pw_n, ratio, aligned):
    """ops/roi_align.py _roi_align for ratio > 0, in torch ops on the device."""
    _, c, h, w = x.shape
    off = 0.5 if aligned else 0.0
    idx = rois[:, 0].long()
    sw, sh, ew, eh = (rois[:, i] * scale - off for i in (1, 2, 3, 4))
    rw, rh = ew - sw, eh - sh
    if not aligned:
        rw, rh = rw.clamp(min=1.0), rh.clamp(min=1.0)
    bh, bw = rh / ph_n, rw / pw_n
    ar = lambda n: torch.arange(n, device=x.device, dtype=x.dtype)  # noqa: E731
    y = sh[:, None, None] + ar(ph_n)[None, :, None] * bh[:, None, None] + (ar(ratio)[None, None, :] + 0.5) * (bh[:, None, None] / ratio)
    xs = sw[:, None, None] + ar(pw_n)[None, :, None] * bw[:, None, None] + (ar(ratio)[None, None, :] + 0.5) * (bw[:, None, None] / ratio)

    def axis(v, size):
        outside = (v < -1.0) | (v > size)
        v = v.clamp(min=0)
        lo = v.long().clamp(max=size - 1)
        hi = (lo + 1).clamp(max=size - 1)
        v = torch.where(lo >= size - 1, lo.to(v.dtype), v)
        frac = v - lo
        return lo, hi, frac, 1 - frac, outside

    yl, yh, ly, hy, yo = axis(y, h)  # (K, PH, IY)
    xl, xh, lx, hx, xo = axis(xs, w)  # (K, PW, IX)

    def tap(yi, xi):  # (K, C, PH, PW, IY, IX)
        return x[idx[:, None, None, None, None, None], ar(c).long()[None, :, None, None, None, None], yi[:, None, :, None, :, None],
                 xi[:, None, None, :, None, :]]

    def wgt(a, b):
        return a[:, None, :, None, :, None] * b[:, None, None, :, None, :]

    val = wgt(hy, hx) * tap(yl, xl) + wgt(hy, lx) * tap(yl, xh) + wgt(ly, hx) * tap(yh, xl) + wgt(ly, lx) * tap(yh, xh)
    val = val.masked_fill(yo[:, None, :, None, :, None] | xo[:, None, None, :, None, :], 0)
    return val.sum((-1, -2)) / (ratio * ratio)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pooling-only", action="store_true", help="only the roi_pool / ps_roi_pool / ps_roi_align rows")
    ap.add_argument("--boxes-only", action="store_true", help="only the box_iou family / masks_to_boxes / MultiScaleRoIAlign rows")
    args = ap.parse_args()
    it = args.iters
    if args.pooling_only:
        return pooling_rows(it)
    if args.boxes_only:
        return boxes_rows(it)
    print(f"baseline: {'torchvision.ops on the GPU' if tv_ops is not None else 'torch-op restatements (no torchvision on this machine)'}")
    for n in (1000, 4000, 20000):
        b, s = boxes(n)
        ours = lambda: ops.nms(b, s, 0.5)  # noqa: E731
        if tv_ops is not None:
            ref, ref_name = (lambda: tv_ops.nms(b, s, 0.5)), "torchvision.ops.nms"
        else:
            ref, ref_name = (lambda: torch_nms(b, s, 0.5)), "torch: sort + IoU matrix + host walk"
        kept = ours()
        same = kept.tolist() == ref().tolist()
        if n > 4000 and tv_ops is None:  # the host walk takes seconds at this size: one call, not a series
            ms = alternate([ours], it)[0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ref()
            e1.record()
            torch.cuda.synchronize()
            ms_ref = e0.elapsed_time(e1)
        else:
            ms, ms_ref = alternate([ours, ref], it)
        print(f"nms n={n:6d} thr=0.5 kept={len(kept):6d}  {ms:9.4f} ms   {ref_name}: {ms_ref:10.4f} ms -> {ms_ref / ms:.1f}x   "
              f"same indices: {same}   {_lib.last_kernel()}", flush=True)

    x = torch.rand((2, 256, 200, 304), device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.rand((1000, 2), device="cuda", generator=g) * torch.tensor([1216.0 - 64, 800.0 - 64], device="cuda")
    wh = 32 + torch.rand((1000, 2), device="cuda", generator=g) * 300
    rois = torch.cat([torch.randint(0, 2, (1000, 1), device="cuda", generator=g).float(), p, p + wh], 1)
    ours = lambda: ops.roi_align(x, rois, 7, 0.25, 2, True)  # noqa: E731
    if tv_ops is not None:
        ref, ref_name = (lambda: tv_ops.roi_align(x, rois, 7, 0.25, 2, True)), "torchvision.ops.roi_align"
    else:
        ref, ref_name = (lambda: torch_roi_align(x, rois, 0.25, 7, 7, 2, True)), "torch: the reference's _roi_align in torch ops"
    err = (ours() - ref()).abs().max().item()
    ms, ms_ref = alternate([ours, ref], it)
    out_bytes = 1000 * 256 * 49 * 4
    taps = 1000 * 256 * 49 * 4 * 4 * 4  # every tap as its own 4-byte read: what the lanes request (mostly from L2)
    print(f"roi_align 1000 rois x 256 ch x 7x7 on 2x256x200x304  {ms:9.4f} ms   output {out_bytes / 1e6:.1f} MB = "
          f"{out_bytes / (ms * 1e-3) / 1e12:.3f} TB/s ({out_bytes / (ms * 1e-3) / 1e12 / PEAK_TBS * 100:.1f} % of 8 TB/s), tap requests "
          f"{taps / 1e9:.2f} GB = {taps / (ms * 1e-3) / 1e12:.2f} TB/s   {_lib.last_kernel()}")
    print(f"  {ref_name}: {ms_ref:9.4f} ms -> {ms_ref / ms:.1f}x   max |difference| {err:.2e}", flush=True)

    pooling_rows(it)
    boxes_rows(it)


def _torch_inter_union(b1, b2):
    area1, area2 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1]), (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    lt, rb = torch.max(b1[:, None, :2], b2[:, :2]), torch.min(b1[:, None, 2:], b2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter, area1[:, None] + area2 - inter


def torch_box_iou(b1, b2):
    inter, union = _torch_inter_union(b1, b2)
    return inter / union


def torch_generalized_box_iou(b1, b2):
    inter, union = _torch_inter_union(b1, b2)
    iou = inter / union
    lti, rbi = torch.min(b1[:, None, :2], b2[:, :2]), torch.max(b1[:, None, 2:], b2[:, 2:])
    whi = (rbi - lti).clamp(min=0)
    areai = whi[:, :, 0] * whi[:, :, 1]
    return iou - (areai - union) / areai


def torch_distance_box_iou(b1, b2, eps=1e-7):
    iou = torch_box_iou(b1, b2)
    lti, rbi = torch.min(b1[:, None, :2], b2[:, :2]), torch.max(b1[:, None, 2:], b2[:, 2:])
    whi = (rbi - lti).clamp(min=0)
    diag = (whi[:, :, 0] ** 2) + (whi[:, :, 1] ** 2) + eps
    xp, yp = (b1[:, 0] + b1[:, 2]) / 2, (b1[:, 1] + b1[:, 3]) / 2
    xg, yg = (b2[:, 0] + b2[:, 2]) / 2, (b2[:, 1] + b2[:, 3]) / 2
    return iou - (((xp[:, None] - xg[None, :]) ** 2) + ((yp[:, None] - yg[None, :]) ** 2)) / diag


def torch_masks_to_boxes(masks):
    out = torch.zeros((masks.shape[0], 4), device=masks.device, dtype=torch.float)
    for index, mask in enumerate(masks):
        y, x = torch.where(mask != 0)
        out[index, 0], out[index, 1], out[index, 2], out[index, 3] = torch.min(x), torch.min(y), torch.max(x), torch.max(y)
    return out


def per_level_roi_align(feats, rois, levels, scales, size, ratio):
    result = torch.zeros((len(rois), feats[0].shape[1]) + size, dtype=feats[0].dtype, device=feats[0].device)
    for level, (f, scale) in enumerate(zip(feats, scales)):
        idx = torch.where(levels == level)[0]
        result[idx] = ops.roi_align(f, rois[idx], size, scale, ratio)
    return result


def boxes_rows(it):
    """The pairwise IoU family at 100 000 x 128 (anchors against ground truth) and 4 096 x 4 096, masks_to_boxes on 100 bool masks
    of 800 x 1216, MultiScaleRoIAlign with 1 000 rois x 256 channels x 7 x 7 on the strides 4 .. 32 of a 2 x 800 x 1216 batch."""
    for n, m in ((100000, 128), (4096, 4096)):
        b1, b2 = boxes(n, seed=3)[0], boxes(m, seed=4)[0]
        for name, ref in (("box_iou", torch_box_iou), ("generalized_box_iou", torch_generalized_box_iou),
                          ("distance_box_iou", torch_distance_box_iou)):
            fn = getattr(ops, name)
            same = torch.equal(fn(b1, b2).nan_to_num(), ref(b1, b2).nan_to_num())
            ms, ms_ref = alternate([lambda: fn(b1, b2), lambda: ref(b1, b2)], it)
            out_bytes = n * m * 4
            print(f"{name} {n} x {m}  {ms:9.4f} ms   output {out_bytes / 1e6:.1f} MB = {out_bytes / (ms * 1e-3) / 1e12:.3f} TB/s "
                  f"({out_bytes / (ms * 1e-3) / 1e12 / PEAK_TBS * 100:.1f} % of 8 TB/s)   torch ops on the GPU: {ms_ref:9.4f} ms -> "
                  f"{ms_ref / ms:.1f}x   same values: {same}   {_lib.last_kernel()}", flush=True)

    g = torch.Generator(device="cuda").manual_seed(5)
    masks = torch.zeros((100, 800, 1216), dtype=torch.bool, device="cuda")
    corners = torch.randint(0, 400, (100, 2), device="cuda", generator=g).tolist()
    for i, (y0, x0) in enumerate(corners):
        masks[i, y0:y0 + 300, x0:x0 + 500] = torch.rand((300, 500), device="cuda", generator=g) < 0.5
    same = torch.equal(ops.masks_to_boxes(masks), torch_masks_to_boxes(masks))
    ms, ms_ref = alternate([lambda: ops.masks_to_boxes(masks), lambda: torch_masks_to_boxes(masks)], it)
    print(f"masks_to_boxes 100 x 800 x 1216 bool  {ms:9.4f} ms   masks {masks.numel() / 1e6:.1f} MB = "
          f"{masks.numel() / (ms * 1e-3) / 1e12:.3f} TB/s   the reference's loop on the GPU: {ms_ref:9.4f} ms -> {ms_ref / ms:.1f}x   "
          f"same values: {same}   {_lib.last_kernel()}", flush=True)

    feats = [torch.rand((2, 256, 800 // s, 1216 // s), device="cuda") for s in (4, 8, 16, 32)]
    scales = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    p = torch.rand((1000, 2), device="cuda", generator=g) * torch.tensor([1216.0 - 64, 800.0 - 64], device="cuda")
    wh = 16 * 2 ** (torch.rand((1000, 2), device="cuda", generator=g) * 5)  # sides 16 .. 512: every level takes its share
    rois = torch.cat([torch.randint(0, 2, (1000, 1), device="cuda", generator=g).float(), p, p + wh], 1)
    levels = ops.LevelMapper(2, 5)([rois[:, 1:]])
    counts = torch.bincount(levels, minlength=4).tolist()
    ours = lambda: ops._multiscale_roi_align_impl(feats, rois, levels, scales, 7, 7, 2)  # noqa: E731
    ref = lambda: per_level_roi_align(feats, rois, levels, scales, (7, 7), 2)  # noqa: E731
    fused = ours()
    kernel = _lib.last_kernel()
    same = torch.equal(fused, ref())
    ms, ms_ref = alternate([ours, ref], it)
    print(f"MultiScaleRoIAlign 1000 rois {counts} x 256 ch x 7x7 on 4 maps of 2x800x1216  {ms:9.4f} ms   per-level loop of "
          f"ops.roi_align: {ms_ref:9.4f} ms -> {ms_ref / ms:.1f}x   same bits: {same}   {kernel}", flush=True)


def pooling_rows(it):
    """roi_pool / ps_roi_pool / ps_roi_align: 1 000 rois, 7 x 7 outputs, a 256-channel 50 x 68 map (the channel count rounded to a
    multiple of 49 for the position-sensitive ops)."""
    g = torch.Generator(device="cuda").manual_seed(2)
    p = torch.rand((1000, 2), device="cuda", generator=g) * torch.tensor([272.0 - 32, 200.0 - 32], device="cuda")
    wh = 16 + torch.rand((1000, 2), device="cuda", generator=g) * 120
    rois = torch.cat([torch.randint(0, 2, (1000, 1), device="cuda", generator=g).float(), p, p + wh], 1)
    for name, c, tail in (("roi_pool", 256, ()), ("ps_roi_pool", 245, ()), ("ps_roi_align", 245, (2,))):
        x = torch.rand((2, c, 50, 68), device="cuda")
        ours = lambda: getattr(ops, name)(x, rois, 7, 0.25, *tail)  # noqa: E731
        c_out = c if name == "roi_pool" else c // 49
        out_bytes = 1000 * c_out * 49 * (4 + 4)  # both outputs
        in_bytes = x.numel() * 4  # the map at most once from HBM (it fits the L2s)
        if tv_ops is not None:
            ref = lambda: getattr(tv_ops, name)(x, rois, 7, 0.25, *tail)  # noqa: E731
            same = torch.equal(ours().nan_to_num(), ref().nan_to_num())
            ms, ms_ref = alternate([ours, ref], it)
            against = f"torchvision.ops.{name}: {ms_ref:9.4f} ms -> {ms_ref / ms:.1f}x   same values: {same}"
        else:
            ms = alternate([ours], it)[0]
            against = "no baseline (torchvision cannot be imported)"
        print(f"{name} 1000 rois x {c_out} ch x 7x7 on 2x{c}x50x68  {ms:9.4f} ms   outputs {out_bytes / 1e6:.2f} MB + map "
              f"{in_bytes / 1e6:.2f} MB = {(out_bytes + in_bytes) / (ms * 1e-3) / 1e12:.4f} TB/s   {against}   {_lib.last_kernel()}",
              flush=True)


if __name__ == "__main__":
    main()
