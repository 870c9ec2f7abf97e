"""Guard-band runs of mv_dwconv3x3_conv1x1_f32 at the C ABI (`-m gpu`), with the helpers of tests/_guard.py, as
tests/test_gpu_mobilenetv3_guard.py: every input sits at element offsets 0 - 3 of a buffer whose other elements are NaN (a read outside
a tensor changes the result), the output in a buffer of sentinels that must come back untouched outside it and written whole inside
it, and refused calls write nothing.  The expected values are the composition of the CPU oracle in the stated summation order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _guard as G  # noqa: E402

NAN = float("nan")
DEV = "cuda"
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1)]  # (inputs, outputs), in elements
SHAPES = [(1, 1, 1, 1, 1, 1), (2, 3, 2, 2, 5, 2), (1, 31, 3, 3, 24, 2), (2, 33, 5, 5, 33, 1), (1, 64, 3, 5, 65, 1), (1, 40, 7, 6, 24, 2),
          (1, 672, 4, 4, 130, 1)]


def _randn(seed, shape, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_dwconv3x3_conv1x1_inside_guards(shape):
    lib = _lib.load()
    n, cin, h, w, cout, stride = shape
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    x, wdw, wpw = _randn(9600 + cin, (n, cin, h, w)), _randn(9601, (cin, 1, 3, 3), 0.4), _randn(9602, (cout, cin, 1, 1), cin ** -0.5)
    bdw, adw, btdw = _randn(9603, (cin,), 0.5), _randn(9604, (cin,), 0.3) + 1.2, _randn(9605, (cin,), 0.4)
    b, a, bt, res = _randn(9606, (cout,), 0.5), _randn(9607, (cout,), 0.3) + 1.2, _randn(9608, (cout,), 0.4), _randn(9609, (n, cout, oh, ow))
    hidden = ref.conv2d_affine_act(x.numpy(), wdw.numpy(), bdw.numpy(), adw.numpy(), btdw.numpy(), None, stride, 1, cin, 2, "relu6")
    slices, sl = F.conv1x1_k_slices(n, cin, oh, ow, cout)
    want = ref.conv2d_affine_act(hidden, wpw.numpy(), b.numpy(), a.numpy(), bt.numpy(), res.numpy(), 1, 0, 1, 1, "hardswish",
                                 slice_len=sl if slices > 1 else 0)
    for off_in, off_out in OFFSETS:
        ins = [G.guarded(t, torch.float32, DEV, off_in + i, sentinel=NAN) for i, t in enumerate((x, wdw, bdw, adw, btdw, wpw, b, a, bt, res))]
        before = [buf.cpu() for buf, _ in ins]
        ybuf, y = G.guarded((n, cout, oh, ow), torch.float32, DEV, off_out)
        v = [t.data_ptr() for _, t in ins]
        rc = lib.mv_dwconv3x3_conv1x1_f32(*v, y.data_ptr(), n, cin, h, w, cout, stride, 2, 2, 1, 3, _lib.stream_ptr(y))
        assert rc == 0, lib.mv_last_error()
        what = f"dwconv3x3_conv1x1 {shape} offsets=({off_in}, {off_out})"
        assert _lib.last_kernel().startswith("k_conv1x1_dw<"), what
        G.assert_same(y, torch.from_numpy(np.asarray(want)), what)
        G.assert_guards_intact(ybuf, y, what=what + " y")
        for (buf, _), was in zip(ins, before):
            G.assert_unchanged(buf, was, what + " input")


def test_null_epilogue_terms_inside_guards():
    """Every optional pointer null: no bias, no affine, no residual, no activation on either stage."""
    lib = _lib.load()
    n, cin, h, w, cout, stride = 2, 33, 5, 5, 33, 2
    x, wdw, wpw = _randn(9650, (n, cin, h, w)), _randn(9651, (cin, 1, 3, 3), 0.4), _randn(9652, (cout, cin, 1, 1), cin ** -0.5)
    hidden = ref.conv2d_affine_act(x.numpy(), wdw.numpy(), None, None, None, None, stride, 1, cin, 0, None)
    want = ref.conv2d_affine_act(hidden, wpw.numpy(), None, None, None, None, 1, 0, 1, 0, None)
    ins = [G.guarded(t, torch.float32, DEV, 1 + i, sentinel=NAN) for i, t in enumerate((x, wdw, wpw))]
    ybuf, y = G.guarded((n, cout, 3, 3), torch.float32, DEV, 3)
    rc = lib.mv_dwconv3x3_conv1x1_f32(ins[0][1].data_ptr(), ins[1][1].data_ptr(), None, None, None, ins[2][1].data_ptr(), None, None, None, None,
                                      y.data_ptr(), n, cin, h, w, cout, stride, 0, 0, 0, 0, _lib.stream_ptr(y))
    assert rc == 0, lib.mv_last_error()
    G.assert_same(y, torch.from_numpy(np.asarray(want)), "null terms")
    G.assert_guards_intact(ybuf, y, what="null terms y")


def test_refused_calls_write_nothing():
    lib = _lib.load()
    n, cin, h, w, cout = 2, 4, 5, 7, 6
    x = _randn(9950, (n, cin, h, w))
    (xb, xv), (yb, yv), (db, dv), (wb, wv), (tb, tv) = (G.guarded(x, torch.float32, DEV, 0, sentinel=NAN), G.guarded((n, cout, h, w), torch.float32, DEV, 0),
                                                        G.guarded(torch.ones(cin, 9), torch.float32, DEV, 0), G.guarded(torch.ones(cout, cin), torch.float32, DEV, 0),
                                                        G.guarded(torch.ones(8), torch.float32, DEV, 0))
    bufs = (xb, yb, db, wb, tb)
    before = [b.cpu() for b in bufs]
    s = _lib.stream_ptr(xv)
    X, Y, D, W, T = xv.data_ptr(), yv.data_ptr(), dv.data_ptr(), wv.data_ptr(), tv.data_ptr()

    def call(x=X, w_dw=D, bias_dw=None, alpha_dw=None, beta_dw=None, w_=W, bias=None, alpha=None, beta=None, res=None, y=Y, n_=n, cin_=cin, h_=h,
             wd=w, cout_=cout, stride=1, affine_dw=0, act_dw=0, affine=0, act=0):
        return lib.mv_dwconv3x3_conv1x1_f32(x, w_dw, bias_dw, alpha_dw, beta_dw, w_, bias, alpha, beta, res, y, n_, cin_, h_, wd, cout_, stride,
                                            affine_dw, act_dw, affine, act, s)
    refusals = [(dict(x=None), "null pointer"), (dict(w_dw=None), "null pointer"), (dict(w_=None), "null pointer"), (dict(y=None), "null pointer"),
                (dict(stride=0), "stride should be 1 or 2"), (dict(stride=3), "stride should be 1 or 2"), (dict(n_=-1), "bad conv shape"),
                (dict(cin_=0), "bad conv shape"), (dict(cout_=0), "bad conv shape"), (dict(h_=0), "bad conv shape"),
                (dict(affine_dw=1), "depthwise affine without alpha / beta"), (dict(affine_dw=2, alpha_dw=T), "depthwise affine without alpha / beta"),
                (dict(affine=2), "affine without alpha / beta"), (dict(affine=1, beta=T), "affine without alpha / beta"),
                (dict(affine_dw=3), "bad depthwise affine"), (dict(act_dw=5), "bad depthwise affine"), (dict(affine=3), "bad affine"), (dict(act=-1), "bad affine"),
                (dict(y=X), "must not overlap"), (dict(y=X + 4 * (n * cin * h * w - 1)), "must not overlap"), (dict(y=D), "must not overlap"),
                (dict(y=W), "must not overlap"), (dict(res=Y), "must not overlap"), (dict(res=Y + 8), "must not overlap"),
                (dict(bias=Y + 16), "must not overlap"), (dict(bias_dw=Y + 4 * n * cout * h * w - 4), "must not overlap"),
                (dict(affine_dw=2, alpha_dw=Y, beta_dw=T), "must not overlap"), (dict(affine=1, alpha=T, beta=Y + 32), "must not overlap"),
                (dict(cin_=1 << 16, h_=1 << 8, wd=1 << 7), "32-bit index")]
    for over, text in refusals:
        rc = call(**over)
        assert rc < 0 and text in lib.mv_last_error().decode(), (over, rc, text, lib.mv_last_error())
    assert call(n_=0, x=None, w_dw=None, w_=None, y=None) == 0
    torch.cuda.synchronize()
    for buf, was, name in zip(bufs, before, ("x", "y", "w_dw", "w", "terms")):
        G.assert_unchanged(buf, was, f"refused calls: {name}")
