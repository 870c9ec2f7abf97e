"""Guard-band runs of mv_retinanet_topk_f32 and mv_retinanet_decode_f32 at the C ABI (`-m gpu`), with the helpers of
tests/_guard.py, as tests/test_gpu_rpn_guard.py: every input sits at element offsets 0 - 3 of a buffer whose other elements are
30.0 for the top-k (the score 1: a logit read outside a map would be selected first; a NaN would pass unnoticed, it never passes
the threshold) and NaN for the decode (a read outside a map changes the result), every output in a buffer of sentinels that must
come back untouched outside the output and written whole inside it, the workspace is exactly mv_retinanet_topk_workspace_bytes
long, and refused calls write nothing.  The expected values are the restatement's (tests/_retinanet_ref.py).  (A, K) = (9, 5) on
the five-level set of tests/test_gpu_retinanet.py."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _retinanet_ref as R  # noqa: E402
from tests import _rpn_ref as P  # noqa: E402
from tests.test_gpu_retinanet import _anchorgen, _decode_inputs, PADDED, SIZES, STRIDES, THRESH  # noqa: E402

NAN = float("nan")
DEV = "cuda"
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1)]  # (inputs, outputs), in elements
A, K = 9, 5


def _ints(v):
    return (C.c_int * len(v))(*v)


def _i64s(v):
    return (C.c_int64 * len(v))(*v)


def _tables(maps, per_anchor):
    return _ints([m.shape[2] for m in maps]), _ints([m.shape[3] for m in maps]), _ints([m.shape[1] // per_anchor for m in maps])


@pytest.mark.parametrize("k", [7, 300])
def test_topk_inside_guards(k):
    lib = _lib.load()
    cl, _ = _decode_inputs(9800)
    for m in cl:
        m.view(-1)[::11] = 0.25  # ties
    want = R.select(cl, K, k, THRESH)
    hs, ws, as_ = _tables(cl, K)
    nbytes = int(lib.mv_retinanet_topk_workspace_bytes(2, hs, ws, as_, 5, K, k))
    assert nbytes > 0 and nbytes % 16 == 0
    for off_in, off_out in OFFSETS:
        ins = [G.guarded(m, torch.float32, DEV, off_in + i, sentinel=30.0) for i, m in enumerate(cl)]
        before = [b.cpu() for b, _ in ins]
        ibuf, idx = G.guarded(tuple(want.shape), torch.int32, DEV, off_out)
        wbuf, wsp = G.guarded_workspace(nbytes, DEV)
        views = [v for _, v in ins]
        rc = lib.mv_retinanet_topk_f32(_lib.pointer_table(views), hs, ws, as_, _i64s([v[0].numel() for v in views]), 5, K, 2, k, THRESH,
                                       idx.data_ptr(), wsp.data_ptr(), nbytes, _lib.stream_ptr(idx))
        assert rc == 0, lib.mv_last_error()
        what = f"retinanet_topk k={k} offsets=({off_in}, {off_out})"
        G.assert_same(idx, want, what)
        G.assert_guards_intact(ibuf, idx, what=what + " idx")
        G.assert_guards_intact(wbuf, wsp, what=what + " workspace")
        for (b, _), was in zip(ins, before):
            G.assert_unchanged(b, was, what + " input")


@pytest.mark.parametrize("weights", [(1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)], ids=["w1", "w10-5"])
def test_decode_inside_guards(weights):
    lib = _lib.load()
    cl, dl = _decode_inputs(9810)
    ag = _anchorgen()
    anchors = ag(P.ImageList(torch.zeros(2, 3, *PADDED), SIZES), cl)
    idx = R.select(cl, K, 300, THRESH)
    idx[0, 5], idx[1, 9] = -1, anchors[0].shape[0] * K  # outside the pyramid
    want = dict(zip(("boxes", "scores", "labels", "valid"), R.decode(cl, dl, idx, anchors, SIZES, K, weights)))
    k = idx.shape[1]
    base = torch.cat(ag.cell_anchors)
    sizes = torch.tensor(SIZES, dtype=torch.float32)
    hs, ws, as_ = _tables(cl, K)
    sh, sw = _ints([s[0] for s in STRIDES]), _ints([s[1] for s in STRIDES])
    for off_in, off_out in OFFSETS:
        ins = {name: [G.guarded(t, torch.float32, DEV, off_in + i, sentinel=NAN) for i, t in enumerate(ts)]
               for name, ts in (("cl", cl), ("dl", dl), ("misc", [base, sizes]))}
        ins["idx"] = [G.guarded(idx, torch.int32, DEV, off_in)]
        before = {name: [b.cpu() for b, _ in pairs] for name, pairs in ins.items()}
        outs = {"boxes": G.guarded((2, k, 4), torch.float32, DEV, off_out), "scores": G.guarded((2, k), torch.float32, DEV, off_out + 1),
                "labels": G.guarded((2, k), torch.int64, DEV, off_out), "valid": G.guarded((2, k), torch.uint8, DEV, off_out)}
        clv, dlv = [v for _, v in ins["cl"]], [v for _, v in ins["dl"]]
        rc = lib.mv_retinanet_decode_f32(_lib.pointer_table(clv), _lib.pointer_table(dlv), hs, ws, as_, _i64s([v[0].numel() for v in clv]),
                                         _i64s([v[0].numel() for v in dlv]), sh, sw, 5, K, ins["misc"][0][1].data_ptr(),
                                         ins["misc"][1][1].data_ptr(), ins["idx"][0][1].data_ptr(), 2, k, *weights, math.log(1000.0 / 16),
                                         outs["boxes"][1].data_ptr(), outs["scores"][1].data_ptr(), outs["labels"][1].data_ptr(),
                                         outs["valid"][1].data_ptr(), _lib.stream_ptr(clv[0]))
        assert rc == 0, lib.mv_last_error()
        what = f"retinanet_decode offsets=({off_in}, {off_out})"
        G.assert_same(outs["boxes"][1], want["boxes"], what + " boxes")
        G.assert_same(outs["scores"][1], want["scores"], what + " scores")
        G.assert_same(outs["labels"][1], want["labels"], what + " labels")
        G.assert_same(outs["valid"][1], want["valid"].to(torch.uint8), what + " valid")
        for name, (buf, view) in outs.items():
            G.assert_guards_intact(buf, view, what=f"{what} {name}")
        for name, pairs in ins.items():
            for (b, _), was in zip(pairs, before[name]):
                G.assert_unchanged(b, was, f"{what} input {name}")


def test_refused_calls_write_nothing():
    lib = _lib.load()
    g = torch.Generator().manual_seed(9830)
    m = torch.randn((2, 6, 5, 7), generator=g)
    (mb, mv_), (ibuf, idx) = G.guarded(m, torch.float32, DEV, 0, sentinel=NAN), G.guarded((2, 7), torch.int32, DEV, 0)
    hs, ws, as_ = _tables([m], 2)
    nbytes = int(lib.mv_retinanet_topk_workspace_bytes(2, hs, ws, as_, 1, 2, 7))
    wbuf, wsp = G.guarded_workspace(nbytes, DEV)
    ws_before, idx_before = wbuf.cpu(), ibuf.cpu()
    args = lambda **o: ({**dict(k=7, stride=210, nb=nbytes, wp=wsp.data_ptr(), ip=idx.data_ptr(), classes=2), **o})  # noqa: E731
    for over, text in ((dict(k=0), "k must be positive"), (dict(k=4097), "k up to 4096"), (dict(stride=209), "image stride"),
                       (dict(nb=nbytes - 1), "workspace of"), (dict(wp=wsp.data_ptr() + 8), "16-byte aligned"),
                       (dict(ip=mv_.data_ptr() + 8), "must not overlap"), (dict(classes=0), "classes must be positive")):
        a = args(**over)
        rc = lib.mv_retinanet_topk_f32(_lib.pointer_table([mv_]), hs, ws, as_, _i64s([a["stride"]]), 1, a["classes"], 2, a["k"], THRESH, a["ip"],
                                       a["wp"], a["nb"], _lib.stream_ptr(idx))
        assert rc < 0 and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    torch.cuda.synchronize()
    G.assert_unchanged(wbuf, ws_before, "refused retinanet_topk: workspace")
    G.assert_unchanged(ibuf, idx_before, "refused retinanet_topk: idx")
    G.assert_unchanged(mb, G.guarded(m, torch.float32, "cpu", 0, sentinel=NAN)[0], "refused retinanet_topk: logits")
    # retinanet_decode: labels misaligned, an output on top of an input, a null output
    d = torch.zeros((2, 12, 5, 7))
    (db, dv) = G.guarded(d, torch.float32, DEV, 0)
    outs = [G.guarded(s, t, DEV, 0) for s, t in (((2, 7, 4), torch.float32), ((2, 7), torch.float32), ((2, 7), torch.int64), ((2, 7), torch.uint8))]
    base, sizes = torch.zeros((3, 4), device=DEV), torch.tensor([[20.0, 28.0]] * 2, device=DEV)
    good = torch.zeros((2, 7), dtype=torch.int32, device=DEV)
    before = [b.cpu() for b, _ in outs] + [db.cpu()]
    ptr = [v.data_ptr() for _, v in outs]
    for o, text in (({2: ptr[2] + 4}, "8-byte aligned"), ({0: dv.data_ptr()}, "must not overlap"), ({3: ptr[0] + 5}, "must not overlap"), ({1: None}, "null pointer")):
        p = [o.get(i, ptr[i]) for i in range(4)]
        rc = lib.mv_retinanet_decode_f32(_lib.pointer_table([mv_]), _lib.pointer_table([dv]), hs, ws, as_, _i64s([210]), _i64s([420]), _ints([4]),
                                         _ints([4]), 1, 2, base.data_ptr(), sizes.data_ptr(), good.data_ptr(), 2, 7, 1.0, 1.0, 1.0, 1.0, 4.0, p[0],
                                         p[1], p[2], p[3], _lib.stream_ptr(good))
        assert rc == -1 and text in lib.mv_last_error().decode(), (o, lib.mv_last_error())
    torch.cuda.synchronize()
    for (buf, _), was in zip(outs + [(db, dv)], before):
        G.assert_unchanged(buf, was, "refused retinanet_decode")
