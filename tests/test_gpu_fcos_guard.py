"""Guard-band runs of mv_group_norm_act_f32, mv_fcos_topk_f32 and mv_fcos_decode_f32 at the C ABI (`-m gpu`), with the helpers of
tests/_guard.py, as tests/test_gpu_retinanet_guard.py: every input sits at element offsets 0 - 3 of a buffer whose other elements
are NaN (a read outside a tensor changes the result; for the top-k 30.0, the score 1, which would be selected first), every output
in a buffer of sentinels that must come back untouched outside the output and written whole inside it -- the -1 tail of idx and the
zero rows of invalid candidates included -- the workspaces are exactly as long as the library asks, and refused calls write
nothing.  The expected values are the restatement's (tests/_fcos_ref.py)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _fcos_ref as R  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _rpn_ref as P  # noqa: E402
from tests.test_gpu_fcos import _decode_inputs, PADDED, SIZES, STRIDES, THRESH  # noqa: E402

NAN = float("nan")
DEV = "cuda"
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1)]  # (inputs, outputs), in elements
K = 5


def _ints(v):
    return (C.c_int * len(v))(*v)


def _i64s(v):
    return (C.c_int64 * len(v))(*v)


# (shape, groups): m = 70 (odd sizes, the scalar form), m = 64 (the dwordx4 form where the offsets leave it aligned), two chunks + 3
GN_CASES = [((2, 6, 5, 7), 3), ((3, 12, 4, 4), 3), ((2, 3, 1, 2 * 4096 + 3), 3)]


@pytest.mark.parametrize("shape,groups", GN_CASES)
def test_group_norm_inside_guards(shape, groups):
    lib = _lib.load()
    n, c, h, w = shape
    g = torch.Generator().manual_seed(9800 + c)
    x = torch.randn(shape, generator=g) * 2 + 0.5
    gamma, beta = torch.randn(c, generator=g) + 1, torch.randn(c, generator=g)
    nbytes = int(lib.mv_group_norm_workspace_bytes(n, c, h, w, groups))
    assert nbytes == n * groups * -(-(c // groups * h * w) // 4096) * 16
    for relu, (off_in, off_out) in zip((0, 1, 0, 1), OFFSETS):
        want = R.group_norm(x, groups, gamma, beta, 1e-5, bool(relu))
        ins = [G.guarded(t, torch.float32, DEV, off_in + i, sentinel=NAN) for i, t in enumerate((x, gamma, beta))]
        before = [b.cpu() for b, _ in ins]
        ybuf, y = G.guarded(shape, torch.float32, DEV, off_out)  # off_out > 0: the output starts mid-allocation, off 16 bytes
        wbuf, wsp = G.guarded_workspace(nbytes, DEV)
        rc = lib.mv_group_norm_act_f32(ins[0][1].data_ptr(), y.data_ptr(), ins[1][1].data_ptr(), ins[2][1].data_ptr(), n, c, h, w, groups,
                                       c * h * w, c * h * w, 1e-5, relu, wsp.data_ptr(), nbytes, _lib.stream_ptr(y))
        assert rc == 0, lib.mv_last_error()
        what = f"group_norm_act {shape} relu={relu} offsets=({off_in}, {off_out})"
        G.assert_same(y, want, what)
        G.assert_guards_intact(ybuf, y, what=what + " y")
        G.assert_guards_intact(wbuf, wsp, what=what + " workspace")
        for (b, _), was in zip(ins, before):
            G.assert_unchanged(b, was, what + " input")
    # in place, the images a channel slice apart: the channels between the images keep their sentinel
    wide = torch.full((n, c + 2, h, w), -7.25)
    wide[:, :c] = x
    buf, view = G.guarded(wide, torch.float32, DEV, 1)
    wbuf, wsp = G.guarded_workspace(nbytes, DEV)
    rc = lib.mv_group_norm_act_f32(view.data_ptr(), view.data_ptr(), None, None, n, c, h, w, groups, (c + 2) * h * w, (c + 2) * h * w, 1e-5, 0,
                                   wsp.data_ptr(), nbytes, _lib.stream_ptr(view))
    assert rc == 0, lib.mv_last_error()
    wide[:, :c] = R.group_norm(x, groups)
    G.assert_same(view, wide, "in place on a channel slice")
    G.assert_guards_intact(buf, view, what="in place")
    G.assert_guards_intact(wbuf, wsp, what="in place workspace")


def _tables(maps):
    return _ints([m.shape[2] for m in maps]), _ints([m.shape[3] for m in maps]), _ints([1] * len(maps))


@pytest.mark.parametrize("k", [7, 300])
def test_topk_inside_guards(k):
    lib = _lib.load()
    cls, ctr, _ = _decode_inputs(9810)
    for m in cls:
        m.view(-1)[::11] = 0.25  # ties
    want = R.select(cls, ctr, K, k, THRESH)
    assert bool((want == -1).any()) and bool((want >= 0).any())
    hs, ws, as_ = _tables(cls)
    nbytes = int(lib.mv_retinanet_topk_workspace_bytes(2, hs, ws, as_, 5, K, k))
    assert nbytes > 0 and nbytes % 16 == 0
    for off_in, off_out in OFFSETS:
        ins = [G.guarded(m, torch.float32, DEV, off_in + i, sentinel=30.0) for i, m in enumerate(cls + ctr)]
        before = [b.cpu() for b, _ in ins]
        ibuf, idx = G.guarded(tuple(want.shape), torch.int32, DEV, off_out)
        wbuf, wsp = G.guarded_workspace(nbytes, DEV)
        clv, ctv = [v for _, v in ins[:5]], [v for _, v in ins[5:]]
        rc = lib.mv_fcos_topk_f32(_lib.pointer_table(clv), _lib.pointer_table(ctv), hs, ws, as_, _i64s([v[0].numel() for v in clv]),
                                  _i64s([v[0].numel() for v in ctv]), 5, K, 2, k, THRESH, idx.data_ptr(), wsp.data_ptr(), nbytes,
                                  _lib.stream_ptr(idx))
        assert rc == 0, lib.mv_last_error()
        what = f"fcos_topk k={k} offsets=({off_in}, {off_out})"
        G.assert_same(idx, want, what)
        G.assert_guards_intact(ibuf, idx, what=what + " idx")
        G.assert_guards_intact(wbuf, wsp, what=what + " workspace")
        for (b, _), was in zip(ins, before):
            G.assert_unchanged(b, was, what + " input")


def test_decode_inside_guards():
    lib = _lib.load()
    cls, ctr, reg = _decode_inputs(9820)
    ag = R.default_anchorgen()
    anchors = ag(P.ImageList(torch.zeros(2, 3, *PADDED), SIZES), cls)
    idx = R.select(cls, ctr, K, 300, THRESH)
    idx[0, 5], idx[1, 9] = -1, anchors[0].shape[0] * K  # outside the pyramid
    want = dict(zip(("boxes", "scores", "labels", "valid"), R.decode(cls, ctr, reg, idx, anchors, SIZES, K)))
    assert bool((~want["valid"]).any())
    k = idx.shape[1]
    base = torch.cat(ag.cell_anchors)
    sizes = torch.tensor(SIZES, dtype=torch.float32)
    hs, ws, as_ = _tables(cls)
    sh, sw = _ints([s[0] for s in STRIDES]), _ints([s[1] for s in STRIDES])
    for off_in, off_out in OFFSETS:
        ins = {name: [G.guarded(t, torch.float32, DEV, off_in + i, sentinel=NAN) for i, t in enumerate(ts)]
               for name, ts in (("cls", cls), ("ctr", ctr), ("reg", reg), ("misc", [base, sizes]))}
        ins["idx"] = [G.guarded(idx, torch.int32, DEV, off_in)]
        before = {name: [b.cpu() for b, _ in pairs] for name, pairs in ins.items()}
        outs = {"boxes": G.guarded((2, k, 4), torch.float32, DEV, off_out), "scores": G.guarded((2, k), torch.float32, DEV, off_out + 1),
                "labels": G.guarded((2, k), torch.int64, DEV, off_out), "valid": G.guarded((2, k), torch.uint8, DEV, off_out)}
        v = {name: [t for _, t in pairs] for name, pairs in ins.items()}
        strides = lambda ts: _i64s([t[0].numel() for t in ts])  # noqa: E731
        rc = lib.mv_fcos_decode_f32(_lib.pointer_table(v["cls"]), _lib.pointer_table(v["ctr"]), _lib.pointer_table(v["reg"]), hs, ws, as_,
                                    strides(v["cls"]), strides(v["ctr"]), strides(v["reg"]), sh, sw, 5, K, v["misc"][0].data_ptr(),
                                    v["misc"][1].data_ptr(), v["idx"][0].data_ptr(), 2, k, outs["boxes"][1].data_ptr(),
                                    outs["scores"][1].data_ptr(), outs["labels"][1].data_ptr(), outs["valid"][1].data_ptr(),
                                    _lib.stream_ptr(v["cls"][0]))
        assert rc == 0, lib.mv_last_error()
        what = f"fcos_decode offsets=({off_in}, {off_out})"
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
    x = torch.randn((2, 6, 5, 7), generator=g)
    (xb, xv), (yb, yv) = G.guarded(x, torch.float32, DEV, 0, sentinel=NAN), G.guarded((2, 6, 5, 7), torch.float32, DEV, 0)
    wbuf, wsp = G.guarded_workspace(96, DEV)
    before = [b.cpu() for b in (xb, yb, wbuf)]
    args = lambda **o: ({**dict(y=yv.data_ptr(), groups=3, eps=1e-5, nb=96, wp=wsp.data_ptr(), ys=210), **o})  # noqa: E731
    for over, text in ((dict(groups=4), "not divisible"), (dict(groups=0), "groups must be positive"), (dict(eps=0.0), "eps must be positive"),
                       (dict(eps=float("inf")), "eps must be positive"), (dict(nb=95), "workspace of"), (dict(wp=wsp.data_ptr() + 8), "16-byte aligned"),
                       (dict(y=xv.data_ptr() + 16), "y must be x itself"), (dict(ys=209), "image strides")):
        a = args(**over)
        rc = lib.mv_group_norm_act_f32(xv.data_ptr(), a["y"], None, None, 2, 6, 5, 7, a["groups"], 210, a["ys"], a["eps"], 1, a["wp"], a["nb"],
                                       _lib.stream_ptr(xv))
        assert rc < 0 and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    torch.cuda.synchronize()
    for buf, was, name in zip((xb, yb, wbuf), before, ("x", "y", "workspace")):
        G.assert_unchanged(buf, was, f"refused group_norm_act: {name}")
    # fcos_topk: the centerness map too short, two anchors, idx on the centerness map
    m, c = torch.randn((2, 3, 5, 7), generator=g), torch.randn((2, 1, 5, 7), generator=g)
    (mb, mv_), (cb, cv), (ibuf, idx) = (G.guarded(m, torch.float32, DEV, 0, sentinel=NAN), G.guarded(c, torch.float32, DEV, 0, sentinel=NAN),
                                        G.guarded((2, 7), torch.int32, DEV, 0))
    hs, ws = _ints([5]), _ints([7])
    nbytes = int(lib.mv_retinanet_topk_workspace_bytes(2, hs, ws, _ints([1]), 1, 3, 7))
    wbuf, wsp = G.guarded_workspace(nbytes, DEV)
    before = [b.cpu() for b in (mb, cb, ibuf, wbuf)]
    for over, text in ((dict(cs=34), "of the centerness"), (dict(a=3), "one anchor per location"), (dict(ip=cv.data_ptr() + 8), "must not overlap"),
                       (dict(nb=nbytes - 1), "workspace of")):
        a = {**dict(cs=35, a=1, ip=idx.data_ptr(), nb=nbytes), **over}
        rc = lib.mv_fcos_topk_f32(_lib.pointer_table([mv_]), _lib.pointer_table([cv]), hs, ws, _ints([a["a"]]), _i64s([105]), _i64s([a["cs"]]), 1, 3, 2, 7,
                                  THRESH, a["ip"], wsp.data_ptr(), a["nb"], _lib.stream_ptr(idx))
        assert rc < 0 and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    torch.cuda.synchronize()
    for buf, was in zip((mb, cb, ibuf, wbuf), before):
        G.assert_unchanged(buf, was, "refused fcos_topk")
