"""Guard-band runs of mv_rpn_topk_f32, mv_rpn_decode_f32 and mv_box_decode_f32 at the C ABI (`-m gpu`), with the helpers of
tests/_guard.py: every input sits at element offsets 0 - 3 of a buffer whose other elements are NaN (the greatest top-k key, and
poison for a decode: a read outside a map changes the result), every output in a buffer of sentinels that must come back
untouched outside the output and written whole inside it, the workspace is exactly mv_rpn_topk_workspace_bytes long, and refused
calls write nothing.  The expected values are the restatement's (tests/_rpn_ref.py)."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _rpn_ref as P  # noqa: E402
from tests.test_gpu_rpn import _decode_inputs, _restatement, _topk_want, SIZES, STRIDES  # noqa: E402

NAN = float("nan")
DEV = "cuda"
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1), (0, 2), (3, 3)]  # (inputs, outputs), in elements


def _ints(v):
    return (C.c_int * len(v))(*v)


def _i64s(v):
    return (C.c_int64 * len(v))(*v)


def _ptrs(tensors):
    return _lib.pointer_table(tensors)


def _stream(t):
    return _lib.stream_ptr(t)


def _tables(maps, per_anchor=1):
    return _ints([m.shape[2] for m in maps]), _ints([m.shape[3] for m in maps]), _ints([m.shape[1] // per_anchor for m in maps])


@pytest.mark.parametrize("k", [7, 300])
def test_topk_inside_guards(k):
    lib = _lib.load()
    g = torch.Generator().manual_seed(8600)
    maps = [torch.randn((2, a, h, w), generator=g) for a, h, w in ((3, 5, 7), (1, 1, 257), (5, 5, 41))]
    for m in maps:
        m.view(-1)[::11] = 0.25  # ties
    want = _topk_want(maps, k)
    hs, ws, as_ = _tables(maps)
    nbytes = int(lib.mv_rpn_topk_workspace_bytes(2, hs, ws, as_, 3, k))
    assert nbytes == (2 * want.shape[1] * 8 + 15) // 16 * 16
    for off_in, off_out in OFFSETS:
        ins = [G.guarded(m, torch.float32, DEV, off_in + i, sentinel=NAN) for i, m in enumerate(maps)]
        before = [b.cpu() for b, _ in ins]
        ibuf, idx = G.guarded(tuple(want.shape), torch.int32, DEV, off_out)
        wbuf, wsp = G.guarded_workspace(nbytes, DEV)
        views = [v for _, v in ins]
        rc = lib.mv_rpn_topk_f32(_ptrs(views), hs, ws, as_, _i64s([v[0].numel() for v in views]), 3, 2, k, idx.data_ptr(), wsp.data_ptr(), nbytes,
                                 _stream(idx))
        assert rc == 0, lib.mv_last_error()
        what = f"rpn_topk k={k} offsets=({off_in}, {off_out})"
        G.assert_same(idx, want, what)
        G.assert_guards_intact(ibuf, idx, what=what + " idx")
        G.assert_guards_intact(wbuf, wsp, what=what + " workspace")
        for (b, _), was in zip(ins, before):
            G.assert_unchanged(b, was, what + " input")


@pytest.mark.parametrize("weights", [(1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)], ids=["w1", "w10-5"])
def test_decode_inside_guards(weights):
    lib = _lib.load()
    ob, dl = _decode_inputs(8610)
    m = _restatement(0.5, weights)
    want = m.from_head_outputs(P.ImageList(torch.zeros(2, 3, 64, 96), SIZES), ob, dl, detailed=True)
    k = want["idx"].shape[1]
    base = torch.cat(m.anchor_generator.cell_anchors)
    sizes = torch.tensor(SIZES, dtype=torch.float32)
    hs, ws, as_ = _tables(ob)
    sh, sw = _ints([s[0] for s in STRIDES]), _ints([s[1] for s in STRIDES])
    for off_in, off_out in OFFSETS:
        ins = {name: [G.guarded(t, torch.float32, DEV, off_in + i, sentinel=NAN) for i, t in enumerate(ts)]
               for name, ts in (("ob", ob), ("dl", dl), ("misc", [base, sizes]))}
        ins["idx"] = [G.guarded(want["idx"].to(torch.int32), torch.int32, DEV, off_in)]
        before = {name: [b.cpu() for b, _ in pairs] for name, pairs in ins.items()}
        outs = {"boxes": G.guarded((2, k, 4), torch.float32, DEV, off_out), "scores": G.guarded((2, k), torch.float32, DEV, off_out + 1),
                "levels": G.guarded((2, k), torch.int64, DEV, off_out), "valid": G.guarded((2, k), torch.uint8, DEV, off_out)}
        obv, dlv = [v for _, v in ins["ob"]], [v for _, v in ins["dl"]]
        rc = lib.mv_rpn_decode_f32(_ptrs(obv), _ptrs(dlv), hs, ws, as_, _i64s([v[0].numel() for v in obv]), _i64s([v[0].numel() for v in dlv]), sh, sw,
                                   3, ins["misc"][0][1].data_ptr(), ins["misc"][1][1].data_ptr(), ins["idx"][0][1].data_ptr(), 2, k, *weights,
                                   math.log(1000.0 / 16), 1e-3, 0.5, outs["boxes"][1].data_ptr(), outs["scores"][1].data_ptr(),
                                   outs["levels"][1].data_ptr(), outs["valid"][1].data_ptr(), _stream(obv[0]))
        assert rc == 0, lib.mv_last_error()
        what = f"rpn_decode offsets=({off_in}, {off_out})"
        G.assert_same(outs["boxes"][1], want["boxes"], what + " boxes")
        G.assert_same(outs["scores"][1], want["scores"], what + " scores")
        G.assert_same(outs["levels"][1], want["levels"], what + " levels")
        G.assert_same(outs["valid"][1], want["valid"].to(torch.uint8), what + " valid")
        for name, (buf, view) in outs.items():
            G.assert_guards_intact(buf, view, what=f"{what} {name}")
        for name, pairs in ins.items():
            for (b, _), was in zip(pairs, before[name]):
                G.assert_unchanged(b, was, f"{what} input {name}")


@pytest.mark.parametrize("m,classes", [(1, 1), (65, 2), (63, 91)])
def test_box_decode_inside_guards(m, classes):
    lib = _lib.load()
    g = torch.Generator().manual_seed(8620 + m)
    p = torch.rand((m, 2), generator=g) * 300
    boxes = torch.cat([p, p + torch.rand((m, 2), generator=g) * 200], 1)
    codes = torch.randn((m, 4 * classes), generator=g) * 4
    coder = P.BoxCoder((10.0, 10.0, 5.0, 5.0), numerics=P.RESTATEMENT)
    want = coder.decode_single(codes, boxes)
    for off_in, off_out in OFFSETS:
        (bb, bv), (cb, cv) = G.guarded(boxes, torch.float32, DEV, off_in, sentinel=NAN), G.guarded(codes, torch.float32, DEV, off_in + 1, sentinel=NAN)
        before = bb.cpu(), cb.cpu()
        obuf, out = G.guarded((m, 4 * classes), torch.float32, DEV, off_out)
        rc = lib.mv_box_decode_f32(bv.data_ptr(), cv.data_ptr(), out.data_ptr(), m, classes, 10.0, 10.0, 5.0, 5.0, math.log(1000.0 / 16), _stream(out))
        assert rc == 0, lib.mv_last_error()
        what = f"box_decode m={m} classes={classes} offsets=({off_in}, {off_out})"
        G.assert_same(out, want, what)
        G.assert_guards_intact(obuf, out, what=what)
        G.assert_unchanged(bb, before[0], what + " boxes")
        G.assert_unchanged(cb, before[1], what + " rel_codes")


def test_refused_calls_write_nothing():
    lib = _lib.load()
    g = torch.Generator().manual_seed(8630)
    m = torch.randn((2, 3, 5, 7), generator=g)
    (mb, mv_), (ibuf, idx) = G.guarded(m, torch.float32, DEV, 0, sentinel=NAN), G.guarded((2, 7), torch.int32, DEV, 0)
    hs, ws, as_ = _tables([m])
    nbytes = int(lib.mv_rpn_topk_workspace_bytes(2, hs, ws, as_, 1, 7))
    wbuf, wsp = G.guarded_workspace(nbytes, DEV)
    ws_before, idx_before = wbuf.cpu(), ibuf.cpu()
    args = lambda **o: ({**dict(k=7, stride=105, nb=nbytes, wp=wsp.data_ptr(), ip=idx.data_ptr()), **o})  # noqa: E731
    for over, text in ((dict(k=0), "k must be positive"), (dict(k=4097), "k up to 4096"), (dict(stride=104), "image stride"), (dict(nb=nbytes - 1), "workspace of"),
                       (dict(wp=wsp.data_ptr() + 8), "16-byte aligned"), (dict(ip=mv_.data_ptr() + 8), "must not overlap")):
        a = args(**over)
        rc = lib.mv_rpn_topk_f32(_ptrs([mv_]), hs, ws, as_, _i64s([a["stride"]]), 1, 2, a["k"], a["ip"], a["wp"], a["nb"], _stream(idx))
        assert rc < 0 and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    torch.cuda.synchronize()
    G.assert_unchanged(wbuf, ws_before, "refused rpn_topk: workspace")
    G.assert_unchanged(ibuf, idx_before, "refused rpn_topk: idx")
    G.assert_unchanged(mb, G.guarded(m, torch.float32, "cpu", 0, sentinel=NAN)[0], "refused rpn_topk: logits")
    # box_decode: the output overlapping an input, and a bad class count
    boxes, codes = torch.rand((5, 4), generator=g), torch.randn((5, 8), generator=g)
    (bb, bv), (cb, cv), (obuf, out) = (G.guarded(boxes, torch.float32, DEV, 1), G.guarded(codes, torch.float32, DEV, 2),
                                       G.guarded((5, 8), torch.float32, DEV, 3))
    before = bb.cpu(), cb.cpu(), obuf.cpu()
    for o, classes, text in ((cv.data_ptr() + 4, 2, "must not overlap"), (out.data_ptr(), 0, "bad shape"), (None, 2, "null pointer")):
        rc = lib.mv_box_decode_f32(bv.data_ptr(), cv.data_ptr(), o, 5, classes, 1.0, 1.0, 1.0, 1.0, 4.0, _stream(out))
        assert rc == -1 and text in lib.mv_last_error().decode()
    torch.cuda.synchronize()
    for buf, was in zip((bb, cb, obuf), before):
        G.assert_unchanged(buf, was, "refused box_decode")
    # rpn_decode: levels misaligned, an output on top of an input
    d = torch.zeros((2, 12, 5, 7))
    (db, dv) = G.guarded(d, torch.float32, DEV, 0)
    outs = [G.guarded(s, t, DEV, 0) for s, t in (((2, 7, 4), torch.float32), ((2, 7), torch.float32), ((2, 7), torch.int64), ((2, 7), torch.uint8))]
    base, sizes = torch.zeros((3, 4), device=DEV), torch.tensor([[20.0, 28.0]] * 2, device=DEV)
    idx.zero_()
    before = [b.cpu() for b, _ in outs] + [db.cpu()]
    ptr = [v.data_ptr() for _, v in outs]
    for o, text in (({2: ptr[2] + 4}, "8-byte aligned"), ({0: dv.data_ptr()}, "must not overlap"), ({3: ptr[0] + 5}, "must not overlap"), ({1: None}, "null pointer")):
        p = [o.get(i, ptr[i]) for i in range(4)]
        rc = lib.mv_rpn_decode_f32(_ptrs([mv_]), _ptrs([dv]), hs, ws, as_, _i64s([105]), _i64s([420]), _ints([4]), _ints([4]), 1, base.data_ptr(),
                                   sizes.data_ptr(), idx.data_ptr(), 2, 7, 1.0, 1.0, 1.0, 1.0, 4.0, 1e-3, 0.0, p[0], p[1], p[2], p[3], _stream(idx))
        assert rc == -1 and text in lib.mv_last_error().decode(), (o, lib.mv_last_error())
    torch.cuda.synchronize()
    for (buf, _), was in zip(outs + [(db, dv)], before):
        G.assert_unchanged(buf, was, "refused rpn_decode")
