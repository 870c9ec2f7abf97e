"""Guard-band runs of mv_dwconv7x7_bias_f32, mv_layer_norm2d_stats_f32, mv_layer_norm2d_f32 and mv_conv1x1_ln_gelu_f32 at the C ABI
(`-m gpu`), with the helpers of tests/_guard.py, as tests/test_gpu_layer_guard_bands.py: every input sits at element offsets 0 - 3 of a
buffer whose other elements are NaN (a read outside a tensor changes the result), every output in a buffer of sentinels that must come
back untouched outside the output and written whole inside it, and refused calls write nothing.  Edge shapes: widths that are no
multiple of 4, one pixel, one channel, cout no multiple of 32; the expected values are those of tests/_convnext_ref.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _convnext_ref as R  # noqa: E402
from tests import _guard as G  # noqa: E402

NAN = float("nan")
DEV = "cuda"
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1)]  # (inputs, outputs), in elements


def _randn(seed, *shapes):
    g = np.random.Generator(np.random.Philox(seed))
    return [g.standard_normal(s).astype(np.float32) for s in shapes]


def _inputs(arrays, off):
    ins = [G.guarded(torch.from_numpy(np.ascontiguousarray(a)), torch.float32, DEV, off + i, sentinel=NAN) for i, a in enumerate(arrays)]
    return ins, [b.cpu() for b, _ in ins]


def _check(outs, wants, ins, before, what):
    for (ybuf, y), want in zip(outs, wants):
        G.assert_same(y, torch.from_numpy(np.asarray(want)), what)
        G.assert_guards_intact(ybuf, y, what=what + " output")
    for (b, _), was in zip(ins, before):
        G.assert_unchanged(b, was, what + " input")


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 2, 9, 13), (1, 1, 7, 65), (2, 1, 3, 4)], ids=str)
def test_depthwise7x7_inside_guards(shape):
    lib = _lib.load()
    n, c, h, w = shape
    x, wt, bias = _randn(3, shape, (c, 1, 7, 7), (c,))
    want = ref.conv2d_affine_act(x, wt, bias, None, None, None, 1, 3, c, 0, None)
    for off_in, off_out in OFFSETS:
        ins, before = _inputs((x, wt, bias), off_in)
        out = G.guarded(shape, torch.float32, DEV, off_out)
        v = [t.data_ptr() for _, t in ins]
        rc = lib.mv_dwconv7x7_bias_f32(v[0], v[1], v[2], out[1].data_ptr(), n, c, h, w, _lib.stream_ptr(out[1]))
        assert rc == 0, lib.mv_last_error()
        assert _lib.last_kernel().startswith("k_dwpc7x7<"), _lib.last_kernel()
        _check([out], [want], ins, before, f"dwconv7x7 {shape} offsets=({off_in}, {off_out})")


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 1, 1), (1, 5, 3, 5), (2, 17, 1, 17), (1, 33, 4, 4)], ids=str)
def test_layer_norm_and_stats_inside_guards(shape):
    lib = _lib.load()
    n, c, h, w = shape
    x, g, b = _randn(4, shape, (c,), (c,))
    mean, rstd = R.layer_norm2d_stats(x, 1e-6)
    want = R.layer_norm2d_apply(x, mean, rstd, g, b)
    for off_in, off_out in OFFSETS:
        ins, before = _inputs((x, g, b), off_in)
        v = [t.data_ptr() for _, t in ins]
        m, r = G.guarded((n, h, w), torch.float32, DEV, off_out), G.guarded((n, h, w), torch.float32, DEV, off_out + 1)
        rc = lib.mv_layer_norm2d_stats_f32(v[0], m[1].data_ptr(), r[1].data_ptr(), n, c, h, w, 1e-6, _lib.stream_ptr(m[1]))
        assert rc == 0 and _lib.last_kernel() == "k_layer_norm2d<stats>", lib.mv_last_error()
        _check([m, r], [mean, rstd], ins, before, f"layer_norm2d_stats {shape} offsets=({off_in}, {off_out})")
        out = G.guarded(shape, torch.float32, DEV, off_out)
        rc = lib.mv_layer_norm2d_f32(v[0], v[1], v[2], out[1].data_ptr(), n, c, h, w, 1e-6, _lib.stream_ptr(out[1]))
        assert rc == 0 and _lib.last_kernel() == "k_layer_norm2d<apply>", lib.mv_last_error()
        _check([out], [want], ins, before, f"layer_norm2d {shape} offsets=({off_in}, {off_out})")


@pytest.mark.parametrize("case", R.GUARD_PW_CASES, ids=str)
def test_conv1x1_ln_gelu_inside_guards(case):
    """One pixel and one channel, widths that are no multiple of 4, cout that is no multiple of 32, one chain and K slices."""
    lib = _lib.load()
    n, cin, cout, h, w = case
    x, wt, bias, lw, lb = R.pw_case(R.GUARD_SEED, case)
    mean, rstd = R.layer_norm2d_stats(x, 1e-6)
    want_norm = R.conv1x1_gelu(x, wt, bias, norm=(mean, rstd, lw, lb))
    want_plain = R.conv1x1_gelu(x, wt, bias)
    for off_in, off_out in OFFSETS:
        ins, before = _inputs((x, mean, rstd, lw, lb, wt, bias), off_in)
        v = [t.data_ptr() for _, t in ins]
        out = G.guarded((n, cout, h, w), torch.float32, DEV, off_out)
        rc = lib.mv_conv1x1_ln_gelu_f32(v[0], v[1], v[2], v[3], v[4], v[5], v[6], out[1].data_ptr(), n, cin, h, w, cout, 1, _lib.stream_ptr(out[1]))
        assert rc == 0, lib.mv_last_error()
        assert _lib.last_kernel() == R.ln_kernel_name(n, cin, h * w, cout, True), _lib.last_kernel()
        _check([out], [want_norm], ins, before, f"conv1x1_ln_gelu {case} offsets=({off_in}, {off_out})")
        out = G.guarded((n, cout, h, w), torch.float32, DEV, off_out)
        rc = lib.mv_conv1x1_ln_gelu_f32(v[0], None, None, None, None, v[5], v[6], out[1].data_ptr(), n, cin, h, w, cout, 1, _lib.stream_ptr(out[1]))
        assert rc == 0, lib.mv_last_error()
        assert _lib.last_kernel() == R.ln_kernel_name(n, cin, h * w, cout, False), _lib.last_kernel()
        _check([out], [want_plain], ins, before, f"conv1x1_ln_gelu without norm {case} offsets=({off_in}, {off_out})")


def test_refused_calls_write_nothing():
    lib = _lib.load()
    x = torch.randn((2, 4, 5, 7), generator=torch.Generator().manual_seed(9970))
    pairs = (G.guarded(x, torch.float32, DEV, 0, sentinel=NAN), G.guarded((2, 4, 5, 7), torch.float32, DEV, 0),
             G.guarded(torch.ones(2, 5, 7), torch.float32, DEV, 0), G.guarded(torch.ones(2, 5, 7), torch.float32, DEV, 0),
             G.guarded(torch.ones(4, 49), torch.float32, DEV, 0))
    (xb, xv), (yb, yv), (mb, mv), (sb, sv), (wb, wv) = pairs
    before = [b.cpu() for b, _ in pairs]
    s = _lib.stream_ptr(xv)
    X, Y, M, S, W = (v.data_ptr() for _, v in pairs)
    dw, st, ln, pw = lib.mv_dwconv7x7_bias_f32, lib.mv_layer_norm2d_stats_f32, lib.mv_layer_norm2d_f32, lib.mv_conv1x1_ln_gelu_f32
    for call, text in ((lambda: dw(X, W, None, X, 2, 4, 5, 7, s), "must not overlap"),
                       (lambda: dw(X, None, None, Y, 2, 4, 5, 7, s), "null pointer"),
                       (lambda: dw(X, W, None, Y, 2, 4, -5, 7, s), "negative size"),
                       (lambda: st(X, M, M, 2, 4, 5, 7, 1e-6, s), "must not overlap"),
                       (lambda: st(X, M, S, 2, 4, 5, 7, -1.0, s), "eps must be non-negative"),
                       (lambda: st(X, None, S, 2, 4, 5, 7, 1e-6, s), "null pointer"),
                       (lambda: ln(X, None, None, X, 2, 4, 5, 7, 1e-6, s), "must not overlap"),
                       (lambda: ln(X, Y + 16, None, Y, 2, 4, 5, 7, 1e-6, s), "must not overlap"),
                       (lambda: ln(X, None, None, Y, 2, 0, 5, 7, 1e-6, s), "no channels"),
                       (lambda: pw(X, M, None, None, None, W, None, Y, 2, 4, 5, 7, 4, 1, s), "mean and rstd come together"),
                       (lambda: pw(X, None, None, W, None, W, None, Y, 2, 4, 5, 7, 4, 1, s), "LayerNorm terms without"),
                       (lambda: pw(X, M, S, None, None, W, None, Y, 2, 4, 5, 7, 4, 3, s), "gelu should be 0 or 1"),
                       (lambda: pw(X, Y + 8, S, None, None, W, None, Y, 2, 4, 5, 7, 4, 1, s), "must not overlap"),
                       (lambda: pw(X, M, S, None, None, W, None, X + 32, 2, 4, 5, 7, 4, 1, s), "must not overlap")):
        rc = call()
        assert rc < 0 and text in lib.mv_last_error().decode(), (rc, text, lib.mv_last_error())
    torch.cuda.synchronize()
    for (buf, _), was, name in zip(pairs, before, ("x", "y", "mean", "rstd", "w")):
        G.assert_unchanged(buf, was, f"refused calls: {name}")
