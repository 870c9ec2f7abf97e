"""Guard-band runs of mv_roi_detections_f32 at the C ABI (`-m gpu`), with the helpers of tests/_guard.py: the strided inputs sit
inside a buffer whose other elements are NaN (poison for a softmax and for a decode: a read outside a row changes the result), the
four outputs in buffers of sentinels that must come back untouched outside the output and written whole inside it, and refused calls
write nothing.  The expected values are the restatement's (tests/_roi_heads_ref.py)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests.test_gpu_roi_heads import detection_case, detection_want, SIZES, _rois  # noqa: E402

NAN = float("nan")
DEV = "cuda"
CLIP = math.log(1000.0 / 16)
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1), (0, 2), (3, 3)]  # (inputs, outputs), in elements
R, C = 63, 65


def _outputs(off):
    return {"boxes": G.guarded((R, C - 1, 4), torch.float32, DEV, off), "scores": G.guarded((R, C - 1), torch.float32, DEV, off + 1),
            "labels": G.guarded((R, C - 1), torch.int64, DEV, off), "valid": G.guarded((R, C - 1), torch.uint8, DEV, off)}


@pytest.mark.parametrize("layout", ["contiguous", "sliced"])
def test_roi_detections_inside_guards(layout):
    lib = _lib.load()
    logits, deltas, proposals = detection_case(R, C)
    want = detection_want(R, C, WEIGHTS, 0.05, 1e-2)
    rois, sizes = _rois(proposals), torch.tensor(SIZES, dtype=torch.float32)
    for off_in, off_out in OFFSETS:
        if layout == "contiguous":
            lb, lv = G.guarded(logits, torch.float32, DEV, off_in, sentinel=NAN)
            db, dv = G.guarded(deltas, torch.float32, DEV, off_in + 1, sentinel=NAN)
            ins = [(lb, lv), (db, dv)]
            lp, ls, dp, ds = lv.data_ptr(), C, dv.data_ptr(), 4 * C
        else:
            # rows of 5 C + 3 elements: C logits, 4 C deltas, three NaN that belong to neither
            both = torch.cat([logits, deltas, torch.full((R, 3), NAN)], 1)
            bb, bv = G.guarded(both, torch.float32, DEV, off_in, sentinel=NAN)
            ins = [(bb, bv)]
            lp, ls, dp, ds = bv.data_ptr(), 5 * C + 3, bv.data_ptr() + 4 * C, 5 * C + 3
        ins += [G.guarded(rois, torch.float32, DEV, off_in, sentinel=NAN), G.guarded(sizes, torch.float32, DEV, off_in + 2, sentinel=NAN)]
        before = [b.cpu() for b, _ in ins]
        outs = _outputs(off_out)
        rc = lib.mv_roi_detections_f32(lp, ls, dp, ds, ins[-2][1].data_ptr(), ins[-1][1].data_ptr(), R, C, 2, *WEIGHTS, CLIP, 0.05, 1e-2,
                                       outs["boxes"][1].data_ptr(), outs["scores"][1].data_ptr(), outs["labels"][1].data_ptr(),
                                       outs["valid"][1].data_ptr(), _lib.stream_ptr(outs["boxes"][1]))
        assert rc == 0, lib.mv_last_error()
        what = f"roi_detections {layout} offsets=({off_in}, {off_out})"
        G.assert_same(outs["boxes"][1], want[0], what + " boxes")
        G.assert_same(outs["scores"][1], want[1], what + " scores")
        G.assert_same(outs["labels"][1], want[2].contiguous(), what + " labels")
        G.assert_same(outs["valid"][1], want[3].to(torch.uint8), what + " valid")
        for name, (buf, view) in outs.items():
            G.assert_guards_intact(buf, view, what=f"{what} {name}")
        for (b, _), was in zip(ins, before):
            G.assert_unchanged(b, was, what + " input")


def test_refused_calls_write_nothing():
    lib = _lib.load()
    logits, deltas, proposals = detection_case(R, C)
    (lb, lv), (db, dv) = G.guarded(logits, torch.float32, DEV, 0, sentinel=NAN), G.guarded(deltas, torch.float32, DEV, 0, sentinel=NAN)
    (rb, rv), (sb, sv) = G.guarded(_rois(proposals), torch.float32, DEV, 0), G.guarded(torch.tensor(SIZES, dtype=torch.float32), torch.float32, DEV, 0)
    outs = _outputs(0)
    ptr = {k: v.data_ptr() for k, (_, v) in outs.items()}
    everything = [lb, db, rb, sb] + [b for b, _ in outs.values()]
    before = [b.cpu() for b in everything]
    base = dict(lp=lv.data_ptr(), ls=C, dp=dv.data_ptr(), ds=4 * C, c=C, n=2, **ptr)
    for over, text in ((dict(c=1), "at least 2 classes"), (dict(c=2049, ls=2049, ds=4 * 2049), "up to 2048 classes"), (dict(ls=C - 1), "row strides"),
                       (dict(ds=4 * C - 1), "row strides"), (dict(n=0), "no image"), (dict(labels=ptr["labels"] + 4), "8-byte aligned"),
                       (dict(boxes=dv.data_ptr() + 16), "must not overlap"), (dict(scores=ptr["boxes"] + 64), "must not overlap"),
                       (dict(valid=lv.data_ptr() + 3), "must not overlap"), (dict(scores=None), "null pointer"), (dict(lp=None), "null pointer")):
        a = {**base, **over}
        rc = lib.mv_roi_detections_f32(a["lp"], a["ls"], a["dp"], a["ds"], rv.data_ptr(), sv.data_ptr(), R, a["c"], a["n"], *WEIGHTS, CLIP, 0.05, 1e-2,
                                       a["boxes"], a["scores"], a["labels"], a["valid"], _lib.stream_ptr(lv))
        assert rc < 0 and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    torch.cuda.synchronize()
    for buf, was in zip(everything, before):
        G.assert_unchanged(buf, was, "refused roi_detections")
