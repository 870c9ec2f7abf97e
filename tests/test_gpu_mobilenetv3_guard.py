"""Guard-band runs of mv_dwconv_norm_act_f32, mv_global_avgpool_f64sum_f32, mv_linear_act_f32, mv_se_scale_f32 and
mv_conv1x1_scaled_f32 at the C ABI (`-m gpu`), with the helpers of tests/_guard.py, as tests/test_gpu_ssd_guard.py: every input sits at
element offsets 0 - 3 of a buffer whose other elements are NaN (a read outside a tensor changes the result), every output in a buffer
of sentinels that must come back untouched outside the output and written whole inside it, and refused calls write nothing.  The
shapes are the smallest of tests/test_gpu_mobilenetv3.py; the expected values are the oracle's and the restatements'."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _mobilenetv3_ref as R  # noqa: E402

NAN = float("nan")
DEV = "cuda"
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1)]  # (inputs, outputs), in elements


def _randn(seed, shape, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _inputs(tensors, off):
    ins = [G.guarded(t, torch.float32, DEV, off + i, sentinel=NAN) for i, t in enumerate(tensors)]
    return ins, [b.cpu() for b, _ in ins]


def _check(ybuf, y, want, ins, before, what):
    G.assert_same(y, torch.from_numpy(np.asarray(want)), what)
    G.assert_guards_intact(ybuf, y, what=what + " y")
    for (b, _), was in zip(ins, before):
        G.assert_unchanged(b, was, what + " input")


@pytest.mark.parametrize("shape,stride", [((1, 1, 1, 1), 1), ((2, 3, 2, 3), 1), ((2, 3, 5, 5), 2), ((1, 3, 9, 6), 1), ((1, 2, 7, 7), 2), ((1, 2, 6, 64), 1)])
def test_depthwise5x5_inside_guards(shape, stride):
    lib = _lib.load()
    n, c, h, w = shape
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    x, wt, al, be, res = (_randn(9600 + h, shape), _randn(9601, (c, 1, 5, 5), 0.3), _randn(9602, (c,)) + 1.5, _randn(9603, (c,)),
                          _randn(9604, (n, c, oh, ow)))
    want = ref.conv2d_affine_act(x.numpy(), wt.numpy(), None, al.numpy(), be.numpy(), res.numpy(), stride, 2, c, 2, "hardswish")
    for off_in, off_out in OFFSETS:
        ins, before = _inputs((x, wt, al, be, res), off_in)
        ybuf, y = G.guarded((n, c, oh, ow), torch.float32, DEV, off_out)
        v = [t for _, t in ins]
        rc = lib.mv_dwconv_norm_act_f32(v[0].data_ptr(), v[1].data_ptr(), None, v[2].data_ptr(), v[3].data_ptr(), v[4].data_ptr(), y.data_ptr(),
                                        n, c, h, w, 5, stride, 2, 3, _lib.stream_ptr(y))
        assert rc == 0, lib.mv_last_error()
        _check(ybuf, y, want, ins, before, f"dwconv 5x5 {shape} s{stride} offsets=({off_in}, {off_out})")


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 3, 1, 3), (2, 3, 7, 7), (1, 2, 1, 257)])
def test_global_avgpool_and_se_scale_inside_guards(shape):
    lib = _lib.load()
    n, c, h, w = shape
    x, g = _randn(9700 + w, shape), _randn(9701, (n, c))
    for off_in, off_out in OFFSETS:
        ins, before = _inputs((x, g), off_in)
        ybuf, y = G.guarded((n, c), torch.float32, DEV, off_out)
        rc = lib.mv_global_avgpool_f64sum_f32(ins[0][1].data_ptr(), y.data_ptr(), n, c, h, w, c * h * w, _lib.stream_ptr(y))
        assert rc == 0, lib.mv_last_error()
        _check(ybuf, y, R.global_avg_pool(x.numpy()), ins, before, f"global_avgpool {shape} offsets=({off_in}, {off_out})")
        ybuf, y = G.guarded(shape, torch.float32, DEV, off_out)
        rc = lib.mv_se_scale_f32(ins[0][1].data_ptr(), ins[1][1].data_ptr(), y.data_ptr(), n, c, h, w, _lib.stream_ptr(y))
        assert rc == 0, lib.mv_last_error()
        _check(ybuf, y, R.se_scale(x.numpy(), g.numpy()), ins, before, f"se_scale {shape} offsets=({off_in}, {off_out})")
        # in place: y == x, the guards of x keep their NaN
        xbuf, xv = G.guarded(x, torch.float32, DEV, off_out, sentinel=NAN)
        rc = lib.mv_se_scale_f32(xv.data_ptr(), ins[1][1].data_ptr(), xv.data_ptr(), n, c, h, w, _lib.stream_ptr(xv))
        assert rc == 0, lib.mv_last_error()
        G.assert_same(xv, torch.from_numpy(R.se_scale(x.numpy(), g.numpy())), "se_scale in place")
        G.assert_guards_intact(xbuf, xv, sentinel=NAN, what="se_scale in place")
    # the pool on a channel slice: the channels between the images are NaN and are not read
    wide = torch.full((n, c + 2, h, w), NAN)
    wide[:, :c] = x
    wbuf, wv = G.guarded(wide, torch.float32, DEV, 1, sentinel=NAN)
    ybuf, y = G.guarded((n, c), torch.float32, DEV, 0)
    rc = lib.mv_global_avgpool_f64sum_f32(wv.data_ptr(), y.data_ptr(), n, c, h, w, (c + 2) * h * w, _lib.stream_ptr(y))
    assert rc == 0, lib.mv_last_error()
    G.assert_same(y, torch.from_numpy(R.global_avg_pool(x.numpy())), "pool on a channel slice")
    G.assert_guards_intact(ybuf, y, what="pool on a channel slice")


@pytest.mark.parametrize("n,k,m,act,name", [(1, 1, 1, 0, None), (2, 3, 8, 1, "relu"), (5, 63, 5, 3, "hardswish"), (2, 65, 7, 5, "hardsigmoid"), (3, 64, 64, 6, "sigmoid")])
def test_linear_act_inside_guards(n, k, m, act, name):
    lib = _lib.load()
    x, w, b = _randn(9800 + k, (n, k)), _randn(9801, (m, k), 0.3), _randn(9802, (m,))
    want = R.linear_act(x.numpy(), w.numpy(), b.numpy(), name)
    for off_in, off_out in OFFSETS:
        ins, before = _inputs((x, w, b), off_in)
        ybuf, y = G.guarded((n, m), torch.float32, DEV, off_out)
        rc = lib.mv_linear_act_f32(ins[0][1].data_ptr(), ins[1][1].data_ptr(), ins[2][1].data_ptr(), y.data_ptr(), n, k, m, act, _lib.stream_ptr(y))
        assert rc == 0, lib.mv_last_error()
        _check(ybuf, y, want, ins, before, f"linear_act {(n, k, m)} {name} offsets=({off_in}, {off_out})")


@pytest.mark.parametrize("n,cin,cout,h,w", [(1, 1, 1, 1, 1), (3, 3, 5, 1, 7), (1, 33, 31, 7, 7), (2, 40, 24, 3, 11), (1, 960, 160, 7, 7)])
def test_scaled_projection_inside_guards(n, cin, cout, h, w):
    from cpu_vision_amd import functional as F
    lib = _lib.load()
    x, g, wt = _randn(9900 + cin, (n, cin, h, w)), _randn(9901, (n, cin)).abs(), _randn(9902, (cout, cin, 1, 1), 0.2)
    al, be, res = _randn(9903, (cout,)) + 1.5, _randn(9904, (cout,)), _randn(9905, (n, cout, h, w))
    slices, sl = F.conv1x1_k_slices(n, cin, h, w, cout)
    want = ref.conv2d_affine_act(R.se_scale(x.numpy(), g.numpy()), wt.numpy(), None, al.numpy(), be.numpy(), res.numpy(), 1, 0, 1, 2, None,
                                 slice_len=sl if slices > 1 else 0)
    for off_in, off_out in OFFSETS:
        ins, before = _inputs((x, g, wt, al, be, res), off_in)
        ybuf, y = G.guarded((n, cout, h, w), torch.float32, DEV, off_out)
        v = [t.data_ptr() for _, t in ins]
        rc = lib.mv_conv1x1_scaled_f32(v[0], v[1], v[2], None, v[3], v[4], v[5], y.data_ptr(), n, cin, h, w, cout, 2, 0, _lib.stream_ptr(y))
        assert rc == 0, lib.mv_last_error()
        _check(ybuf, y, want, ins, before, f"conv1x1_scaled {(n, cin, cout, h, w)} offsets=({off_in}, {off_out})")


def test_refused_calls_write_nothing():
    lib = _lib.load()
    x = _randn(9950, (2, 4, 5, 7))
    (xb, xv), (yb, yv), (gb, gv), (wb, wv) = (G.guarded(x, torch.float32, DEV, 0, sentinel=NAN), G.guarded((2, 4, 5, 7), torch.float32, DEV, 0),
                                              G.guarded(torch.ones(2, 4), torch.float32, DEV, 0), G.guarded(torch.ones(4, 25), torch.float32, DEV, 0))
    before = [b.cpu() for b in (xb, yb, gb, wb)]
    s = _lib.stream_ptr(xv)
    X, Y, Gp, W = xv.data_ptr(), yv.data_ptr(), gv.data_ptr(), wv.data_ptr()
    for call, text in ((lambda: lib.mv_dwconv_norm_act_f32(X, W, None, None, None, None, Y, 2, 4, 5, 7, 7, 1, 0, 0, s), "kernel 3 or 5"),
                     (lambda: lib.mv_dwconv_norm_act_f32(X, W, None, None, None, None, Y, 2, 4, 5, 7, 5, 3, 0, 0, s), "stride should be"),
                     (lambda: lib.mv_dwconv_norm_act_f32(X, W, None, None, None, None, X, 2, 4, 5, 7, 5, 1, 0, 0, s), "alias"),
                     (lambda: lib.mv_global_avgpool_f64sum_f32(X, Y, 2, 4, 5, 7, 139, s), "image stride"),
                     (lambda: lib.mv_global_avgpool_f64sum_f32(X, X + 16, 2, 4, 5, 7, 140, s), "must not overlap"),
                     (lambda: lib.mv_linear_act_f32(X, W, None, Y, 2, 25, 4, 2, s), "activation code"),
                     (lambda: lib.mv_linear_act_f32(X, W, None, X + 8, 2, 25, 4, 0, s), "must not overlap"),
                     (lambda: lib.mv_se_scale_f32(X, Gp, X + 16, 2, 4, 5, 7, s), "y must be x itself"),
                     (lambda: lib.mv_se_scale_f32(X, None, Y, 2, 4, 5, 7, s), "null pointer"),
                     (lambda: lib.mv_conv1x1_scaled_f32(X, Gp, W, None, None, None, None, X + 32, 2, 4, 5, 7, 4, 0, 0, s), "must not overlap"),
                     (lambda: lib.mv_conv1x1_scaled_f32(X, None, W, None, None, None, None, Y, 2, 4, 5, 7, 4, 0, 0, s), "null pointer"),
                     (lambda: lib.mv_conv1x1_scaled_f32(X, Gp, W, None, None, None, None, Y, 2, 4, 5, 7, 4, 1, 0, s), "affine without")):
        rc = call()
        assert rc < 0 and text in lib.mv_last_error().decode(), (rc, text, lib.mv_last_error())
    torch.cuda.synchronize()
    for buf, was, name in zip((xb, yb, gb, wb), before, ("x", "y", "gate", "w")):
        G.assert_unchanged(buf, was, f"refused calls: {name}")
