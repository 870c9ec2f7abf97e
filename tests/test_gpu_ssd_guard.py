"""Guard-band runs of mv_l2_normalize_scale_f32, mv_maxpool2d_ceil_f32, mv_ssd_scores_f32, mv_ssd_topk_f32 and mv_ssd_decode_f32 at the
C ABI (`-m gpu`), with the helpers of tests/_guard.py, as tests/test_gpu_fcos_guard.py: every input sits at element offsets 0 - 3 of a
buffer whose other elements are NaN (a read outside a tensor changes the result; for the pool +inf, which would win, for the top-k
0.99, which would be selected first), every output in a buffer of sentinels that must come back untouched outside the output and
written whole inside it -- the -1 tail of idx and the zero rows of invalid candidates included -- and refused calls write nothing.
The expected values are the restatement's (tests/_ssd_ref.py) and, for the pool, torch's."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd.anchor_utils import DefaultBoxGenerator  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _ssd_ref as R  # noqa: E402

NAN, INF = float("nan"), float("inf")
DEV = "cuda"
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1)]  # (inputs, outputs), in elements
GRIDS, ANCHORS, RATIOS = [(5, 4), (3, 3), (1, 1)], [4, 6, 4], [[2], [2, 3], [2]]
K = 5


def _ints(v):
    return (C.c_int * len(v))(*v)


def _i64s(v):
    return (C.c_int64 * len(v))(*v)


def _randn(seed, shape, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# C = 37 on 5 x 7 (odd sizes, three blocks of 16 pixels, the last ragged), C = 1, and 2 x 2 pixels of 513 channels
@pytest.mark.parametrize("shape", [(2, 37, 5, 7), (3, 1, 1, 19), (2, 513, 2, 2)])
def test_l2_normalize_scale_inside_guards(shape):
    lib = _lib.load()
    n, c, h, w = shape
    x, wt = _randn(9000 + c, shape, 2.0), _randn(9001 + c, (c,)) + 3
    want = R.l2_normalize_scale(x, wt)
    for off_in, off_out in OFFSETS:
        ins = [G.guarded(t, torch.float32, DEV, off_in + i, sentinel=NAN) for i, t in enumerate((x, wt))]
        before = [b.cpu() for b, _ in ins]
        ybuf, y = G.guarded(shape, torch.float32, DEV, off_out)
        rc = lib.mv_l2_normalize_scale_f32(ins[0][1].data_ptr(), y.data_ptr(), ins[1][1].data_ptr(), n, c, h, w, c * h * w, c * h * w, 1e-12,
                                           _lib.stream_ptr(y))
        assert rc == 0, lib.mv_last_error()
        what = f"l2_normalize_scale {shape} offsets=({off_in}, {off_out})"
        G.assert_same(y, want, what)
        G.assert_guards_intact(ybuf, y, what=what + " y")
        for (b, _), was in zip(ins, before):
            G.assert_unchanged(b, was, what + " input")
    # in place, the images a channel slice apart: the channels between the images keep their sentinel
    wide = torch.full((n, c + 2, h, w), -7.25)
    wide[:, :c] = x
    buf, view = G.guarded(wide, torch.float32, DEV, 1)
    wbuf, wv = G.guarded(wt, torch.float32, DEV, 0, sentinel=NAN)
    rc = lib.mv_l2_normalize_scale_f32(view.data_ptr(), view.data_ptr(), wv.data_ptr(), n, c, h, w, (c + 2) * h * w, (c + 2) * h * w, 1e-12,
                                       _lib.stream_ptr(view))
    assert rc == 0, lib.mv_last_error()
    wide[:, :c] = want
    G.assert_same(view, wide, "in place on a channel slice")
    G.assert_guards_intact(buf, view, what="in place")


@pytest.mark.parametrize("size,k,s,p", [((75, 75), 2, 2, 0), ((5, 7), 3, 2, 1), ((3, 4), 2, 2, 1), ((9, 5), 5, 4, 2)])
def test_max_pool2d_ceil_inside_guards(size, k, s, p):
    lib = _lib.load()
    x = _randn(9100 + size[0], (3,) + size)
    want = torch.nn.functional.max_pool2d(x[None], k, s, p, ceil_mode=True)[0]
    for off_in, off_out in OFFSETS:
        xb, xv = G.guarded(x, torch.float32, DEV, off_in, sentinel=INF)  # a window past the plane would pick the guard up
        was = xb.cpu()
        ybuf, y = G.guarded(tuple(want.shape), torch.float32, DEV, off_out)
        rc = lib.mv_maxpool2d_ceil_f32(xv.data_ptr(), y.data_ptr(), 3, size[0], size[1], k, s, p, _lib.stream_ptr(y))
        assert rc == 0, lib.mv_last_error()
        what = f"max_pool2d ceil {size} k={k} s={s} p={p} offsets=({off_in}, {off_out})"
        G.assert_same(y, want, what)
        G.assert_guards_intact(ybuf, y, what=what + " y")
        G.assert_unchanged(xb, was, what + " input")


def _maps(seed, per_anchor, scale):
    return [_randn(seed + i, (2, a * per_anchor, h, w), scale) for i, ((h, w), a) in enumerate(zip(GRIDS, ANCHORS))]


def _tables():
    return _ints([g[0] for g in GRIDS]), _ints([g[1] for g in GRIDS]), _ints(ANCHORS)


def test_ssd_scores_inside_guards():
    lib = _lib.load()
    cls = _maps(9200, K, 2.0)
    want = R.scores(cls, K)
    hs, ws, as_ = _tables()
    for off_in, off_out in OFFSETS:
        ins = [G.guarded(m, torch.float32, DEV, off_in + i, sentinel=NAN) for i, m in enumerate(cls)]
        before = [b.cpu() for b, _ in ins]
        sbuf, sc = G.guarded(tuple(want.shape), torch.float32, DEV, off_out)
        views = [v for _, v in ins]
        rc = lib.mv_ssd_scores_f32(_lib.pointer_table(views), hs, ws, as_, _i64s([v[0].numel() for v in views]), 3, K, 2, sc.data_ptr(),
                                   _lib.stream_ptr(sc))
        assert rc == 0, lib.mv_last_error()
        what = f"ssd_scores offsets=({off_in}, {off_out})"
        G.assert_same(sc, want, what)
        G.assert_guards_intact(sbuf, sc, what=what + " scores")
        for (b, _), was in zip(ins, before):
            G.assert_unchanged(b, was, what + " input")


@pytest.mark.parametrize("k", [7, 300])
def test_ssd_topk_inside_guards(k):
    lib = _lib.load()
    sc = R.scores(_maps(9300, K, 2.0), K)
    sc.view(-1)[::11] = 0.25  # ties
    v = sc.shape[2]
    want = R.select(sc, k, 0.1)
    assert bool((want >= 0).any()) and (k == 7 or bool((want == -1).any()))  # k = 300 > V: every segment ends in -1
    for off_in, off_out in OFFSETS:
        sbuf, sv = G.guarded(sc, torch.float32, DEV, off_in, sentinel=0.99)
        was = sbuf.cpu()
        ibuf, idx = G.guarded(tuple(want.shape), torch.int32, DEV, off_out)
        rc = lib.mv_ssd_topk_f32(sv.data_ptr(), 2, K, v, k, 0.1, idx.data_ptr(), _lib.stream_ptr(idx))
        assert rc == 0, lib.mv_last_error()
        what = f"ssd_topk k={k} offsets=({off_in}, {off_out})"
        G.assert_same(idx, want, what)
        G.assert_guards_intact(ibuf, idx, what=what + " idx")
        G.assert_unchanged(sbuf, was, what + " input")


SIZES = [(40, 32), (37, 30)]


def test_ssd_decode_inside_guards():
    lib = _lib.load()
    gen = DefaultBoxGenerator(RATIOS, steps=[7, 13, 29])
    sc, reg = R.scores(_maps(9400, K, 2.0), K), _maps(9410, 4, 3.0)
    v = sc.shape[2]
    idx = R.select(sc, 9, 0.05)
    idx[0, 5], idx[1, 9] = -1, v * K  # outside the pyramid
    want = dict(zip(("boxes", "scores", "labels", "valid"), R.decode(sc, reg, idx, R.default_boxes(gen, GRIDS, (40, 32)), SIZES)))
    assert bool((~want["valid"]).any()) and bool(want["valid"].any())
    m = idx.shape[1]
    pairs = torch.cat(gen._wh_pairs).clamp(min=0, max=1)
    sizes = torch.tensor(SIZES, dtype=torch.float32)
    hs, ws, as_ = _tables()
    xf = (C.c_float * 3)(*[32 / s for s in gen.steps])
    yf = (C.c_float * 3)(*[40 / s for s in gen.steps])
    for off_in, off_out in OFFSETS:
        ins = {name: [G.guarded(t, torch.float32, DEV, off_in + i, sentinel=NAN) for i, t in enumerate(ts)]
               for name, ts in (("reg", reg), ("misc", [sc, pairs, sizes]))}
        ins["idx"] = [G.guarded(idx, torch.int32, DEV, off_in)]
        before = {name: [b.cpu() for b, _ in ps] for name, ps in ins.items()}
        outs = {"boxes": G.guarded((2, m, 4), torch.float32, DEV, off_out), "scores": G.guarded((2, m), torch.float32, DEV, off_out + 1),
                "labels": G.guarded((2, m), torch.int64, DEV, off_out), "valid": G.guarded((2, m), torch.uint8, DEV, off_out)}
        vw = {name: [t for _, t in ps] for name, ps in ins.items()}
        rc = lib.mv_ssd_decode_f32(vw["misc"][0].data_ptr(), _lib.pointer_table(vw["reg"]), hs, ws, as_, _i64s([t[0].numel() for t in vw["reg"]]),
                                   3, K, vw["misc"][1].data_ptr(), xf, yf, 40, 32, vw["misc"][2].data_ptr(), vw["idx"][0].data_ptr(), 2, m, 10.0, 10.0,
                                   5.0, 5.0, math.log(1000.0 / 16), outs["boxes"][1].data_ptr(), outs["scores"][1].data_ptr(),
                                   outs["labels"][1].data_ptr(), outs["valid"][1].data_ptr(), _lib.stream_ptr(vw["reg"][0]))
        assert rc == 0, lib.mv_last_error()
        what = f"ssd_decode offsets=({off_in}, {off_out})"
        G.assert_same(outs["boxes"][1], want["boxes"], what + " boxes")
        G.assert_same(outs["scores"][1], want["scores"], what + " scores")
        G.assert_same(outs["labels"][1], want["labels"], what + " labels")
        G.assert_same(outs["valid"][1], want["valid"].to(torch.uint8), what + " valid")
        for name, (buf, view) in outs.items():
            G.assert_guards_intact(buf, view, what=f"{what} {name}")
        for name, ps in ins.items():
            for (b, _), was in zip(ps, before[name]):
                G.assert_unchanged(b, was, f"{what} input {name}")


def test_refused_calls_write_nothing():
    lib = _lib.load()
    x = _randn(9500, (2, 6, 5, 7))
    (xb, xv), (yb, yv), (wb, wv) = (G.guarded(x, torch.float32, DEV, 0, sentinel=NAN), G.guarded((2, 6, 5, 7), torch.float32, DEV, 0),
                                    G.guarded(torch.ones(6), torch.float32, DEV, 0))
    before = [b.cpu() for b in (xb, yb, wb)]
    for over, text in ((dict(eps=0.0), "eps must be positive"), (dict(eps=INF), "eps must be positive"), (dict(y=xv.data_ptr() + 16), "y must be x itself"),
                       (dict(ys=209), "image strides"), (dict(y=yv.data_ptr() + 2), "4-byte aligned"), (dict(w=None), "null pointer")):
        a = {**dict(y=yv.data_ptr(), eps=1e-12, ys=210, w=wv.data_ptr()), **over}
        rc = lib.mv_l2_normalize_scale_f32(xv.data_ptr(), a["y"], a["w"], 2, 6, 5, 7, 210, a["ys"], a["eps"], _lib.stream_ptr(xv))
        assert rc < 0 and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    rc = lib.mv_maxpool2d_ceil_f32(xv.data_ptr(), yv.data_ptr(), 12, 5, 7, 2, 2, 2, _lib.stream_ptr(xv))
    assert rc < 0 and "pad should be" in lib.mv_last_error().decode()
    torch.cuda.synchronize()
    for buf, was, name in zip((xb, yb, wb), before, ("x", "y", "weight")):
        G.assert_unchanged(buf, was, f"refused l2_normalize_scale / max_pool2d: {name}")
    # ssd_scores: a short image stride, one class, scores on the map; ssd_topk: k too large, idx on the scores
    m = _randn(9510, (2, 12, 5, 7))
    (mb, mv_), (sb, sv), (ib, iv) = (G.guarded(m, torch.float32, DEV, 0, sentinel=NAN), G.guarded((2, 3, 140), torch.float32, DEV, 0),
                                     G.guarded((2, 14), torch.int32, DEV, 0))
    before = [b.cpu() for b in (mb, sb, ib)]
    hs, ws, as_ = _ints([5]), _ints([7]), _ints([4])
    for over, text in ((dict(stride=419), "image stride"), (dict(classes=1, a=12), "at least 2 classes"), (dict(out=mv_.data_ptr() + 64), "must not overlap")):
        a = {**dict(stride=420, classes=3, a=4, out=sv.data_ptr()), **over}
        rc = lib.mv_ssd_scores_f32(_lib.pointer_table([mv_]), hs, ws, _ints([a["a"]]), _i64s([a["stride"]]), 1, a["classes"], 2, a["out"],
                                   _lib.stream_ptr(sv))
        assert rc < 0 and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    for over, text in ((dict(k=4097), "k up to 4096"), (dict(k=0), "k must be positive"), (dict(idx=sv.data_ptr() + 32), "must not overlap")):
        a = {**dict(k=7, idx=iv.data_ptr()), **over}
        rc = lib.mv_ssd_topk_f32(sv.data_ptr(), 2, 3, 140, a["k"], 0.1, a["idx"], _lib.stream_ptr(sv))
        assert rc < 0 and text in lib.mv_last_error().decode(), (over, rc, lib.mv_last_error())
    torch.cuda.synchronize()
    for buf, was in zip((mb, sb, ib), before):
        G.assert_unchanged(buf, was, "refused ssd_scores / ssd_topk")
