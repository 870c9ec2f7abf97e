"""Guard-band runs of mv_heatmaps_to_keypoints_f32 and mv_conv_transpose4x4s2_bias_act_f32 at the C ABI (`-m gpu`), with the helpers
of tests/_guard.py: every input sits at element offsets 0 - 3 of a buffer whose other elements are NaN (a read outside an input
changes the result: a NaN beats every number in the keypoint kernel, and poisons a sum in the conv), the outputs in buffers of
sentinels that must come back untouched outside the output and written whole inside it (the zero rows of the keypoints included: the
sentinel is not 0), and refused calls write nothing.  The expected values are those of tests/_keypoint_ref.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _keypoint_ref as KR  # noqa: E402
from tests._util import philox_f32  # noqa: E402

NAN, INF = float("nan"), float("inf")
DEV = "cuda"
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1), (0, 2), (3, 3)]  # (inputs, outputs), in elements


def _stream(t):
    return _lib.stream_ptr(t)


@pytest.mark.parametrize("k,mh,mw", [(3, 56, 56), (2, 4, 7), (1, 5, 3)])
def test_heatmaps_to_keypoints_inside_guards(k, mh, mw):
    lib = _lib.load()
    # the last roi and the first: upsampling whose windows clamp at every edge of the map; zero rows in between and at the end
    rois = torch.tensor([[0.0, 0.0, 200.0, 131.0], [NAN, 0.0, 1.0, 1.0], [-3.5, 2.0, 16.5, 35.0], [2.0, 2.0, 2.0 + mw, 2.0 + mh],
                         [1.0, 1.0, 601.0, 10.0], [0.0, 0.0, INF, 4.0]])
    r = len(rois)
    maps = torch.from_numpy(philox_f32(9900 + k + mh, (r, k, mh, mw)) * 4 - 2)
    maps[0, 0, 0, 0] = maps[4, k - 1, mh - 1, mw - 1] = 9.0  # maxima at the first and the last element of the maps
    want_xy, want_scores = (torch.from_numpy(a) for a in KR.keypoints(maps.numpy(), rois.numpy()))
    assert float(G.FLOAT_SENTINEL) != 0.0 and not want_xy[1].any() and not want_xy[5].any() and want_scores[0, 0] > 8
    for off_in, off_out in OFFSETS:
        mb, mv_ = G.guarded(maps, torch.float32, DEV, off_in, sentinel=NAN)
        rb, rv = G.guarded(rois, torch.float32, DEV, (off_in + 1) % 4, sentinel=NAN)
        before = mb.cpu(), rb.cpu()
        xb, xv = G.guarded((r, k, 3), torch.float32, DEV, off_out)
        sb, sv = G.guarded((r, k), torch.float32, DEV, (off_out + 1) % 4)
        rc = lib.mv_heatmaps_to_keypoints_f32(mv_.data_ptr(), rv.data_ptr(), xv.data_ptr(), sv.data_ptr(), r, k, mh, mw, _stream(xv))
        assert rc == 0, lib.mv_last_error()
        what = f"heatmaps_to_keypoints k={k} ({mh}, {mw}) offsets=({off_in}, {off_out})"
        assert _lib.last_kernel() == "k_heatmaps_to_keypoints", (what, _lib.last_kernel())
        G.assert_same(xv, want_xy, what + " xy")  # no sentinel is left inside: `want` holds none
        G.assert_same(sv, want_scores, what + " scores")
        assert not bool((xv == G.FLOAT_SENTINEL).any()) and not bool((sv == G.FLOAT_SENTINEL).any()), what
        G.assert_guards_intact(xb, xv, what=what + " xy")
        G.assert_guards_intact(sb, sv, what=what + " scores")
        G.assert_unchanged(mb, before[0], what + " maps")
        G.assert_unchanged(rb, before[1], what + " rois")


@pytest.mark.parametrize("n,cin,h,w,cout", [(2, 8, 5, 7, 3), (1, 256, 14, 14, 17), (1, 4, 1, 1, 1), (3, 6, 9, 4, 20)])
def test_conv_transpose4x4s2_inside_guards(n, cin, h, w, cout):
    lib = _lib.load()
    x = philox_f32(9910 + cin, (n, cin, h, w)) * 2 - 1
    wt = (philox_f32(9911 + cin, (cin, cout, 4, 4)) * 2 - 1) * np.float32(2.0 / np.sqrt(cin))
    b = philox_f32(9912 + cin, (cout,)) * 2 - 1
    w2, b4 = KR.relaid4(wt, b)
    want = torch.from_numpy(KR.oracle_conv_transpose4(x, wt, b, "relu"))
    for off_in, off_out in OFFSETS:
        xb, xv = G.guarded(torch.from_numpy(x), torch.float32, DEV, off_in, sentinel=NAN)
        wb, wv = G.guarded(torch.from_numpy(w2), torch.float32, DEV, (off_in + 1) % 4, sentinel=NAN)
        bb, bv = G.guarded(torch.from_numpy(b4), torch.float32, DEV, (off_in + 2) % 4, sentinel=NAN)
        before = xb.cpu(), wb.cpu(), bb.cpu()
        yb, yv = G.guarded((n, cout, 2 * h, 2 * w), torch.float32, DEV, off_out)
        rc = lib.mv_conv_transpose4x4s2_bias_act_f32(xv.data_ptr(), wv.data_ptr(), bv.data_ptr(), yv.data_ptr(), n, cin, h, w, cout, 1, _stream(yv))
        assert rc == 0, lib.mv_last_error()
        what = f"conv_transpose4x4s2 {(n, cin, h, w, cout)} offsets=({off_in}, {off_out})"
        assert _lib.last_kernel().startswith("k_conv_igemm_tr<"), (what, _lib.last_kernel())
        G.assert_same(yv, want, what)
        assert not bool((yv == G.FLOAT_SENTINEL).any()), what
        G.assert_guards_intact(yb, yv, what=what)
        for buf, was, name in zip((xb, wb, bb), before, ("x", "w2", "bias4")):
            G.assert_unchanged(buf, was, f"{what} {name}")


def test_refused_calls_write_nothing():
    lib = _lib.load()
    maps, rois = torch.from_numpy(philox_f32(9920, (2, 2, 2, 4))), torch.tensor([[1.0, 1.0, 5.0, 4.0], [0.0, 2.0, 7.0, 5.0]])
    (mb, mv_), (rb, rv) = G.guarded(maps, torch.float32, DEV, 1, sentinel=NAN), G.guarded(rois, torch.float32, DEV, 2, sentinel=NAN)
    xb, xv = G.guarded((2, 2, 3), torch.float32, DEV, 2)
    sb, sv = G.guarded((64,), torch.float32, DEV, 1)
    before = [t.cpu() for t in (mb, rb, xb, sb)]
    m, b, xy, sc = mv_.data_ptr(), rv.data_ptr(), xv.data_ptr(), sv.data_ptr()
    s = _stream(xv)
    for args, status, text in (((m, b, None, sc, 2, 2, 2, 4), -1, "null pointer"), ((m, b, xy, None, 2, 2, 2, 4), -1, "null pointer"),
                               ((None, b, xy, sc, 2, 2, 2, 4), -1, "null pointer"), ((m, b, xy, sc, 2, 0, 2, 4), -1, "bad shape"),
                               ((m, b, xy, sc, -2, 2, 2, 4), -1, "bad shape"), ((m, b, xy, sc, 2, 2, 129, 128), -2, "exceed 16384 elements"),
                               ((m, b, m + 8, sc, 2, 2, 2, 4), -1, "must not overlap"), ((m, b, xy, xy + 16, 2, 2, 2, 4), -1, "must not overlap"),
                               ((m, sc + 8, xy, sc, 2, 2, 2, 4), -1, "must not overlap")):
        rc = lib.mv_heatmaps_to_keypoints_f32(*args, s)
        assert rc == status and text in lib.mv_last_error().decode(), (args, rc, lib.mv_last_error())
    # x (1, 2, 2, 2) and w2 (4, 2, 2, 2) in the 32 floats of `maps`' buffer from m on, bias4 in `rois`, y (1, 1, 4, 4) in `scores`
    w = m + 32
    for args, status, text in (((m, w, b, None, 1, 2, 2, 2, 1, 1), -1, "null pointer"), ((m, None, b, sc, 1, 2, 2, 2, 1, 1), -1, "null pointer"),
                               ((m, w, b, sc, 1, 2, 2, 2, 1, 4), -1, "bad activation code"), ((m, w, b, sc, 1, 2, 0, 2, 1, 1), -1, "bad shape"),
                               ((m, w, b, sc, 1, 16384, 2, 2, 1, 1), -2, "index range"), ((m, w, b, m + 16, 1, 2, 2, 2, 1, 1), -1, "must not overlap"),
                               ((m, w, sc + 32, sc, 1, 2, 2, 2, 1, 1), -1, "must not overlap")):
        rc = lib.mv_conv_transpose4x4s2_bias_act_f32(*args, s)
        assert rc == status and text in lib.mv_last_error().decode(), (args, rc, lib.mv_last_error())
    torch.cuda.synchronize()
    for buf, was, name in zip((mb, rb, xb, sb), before, ("maps", "rois", "xy", "scores")):
        G.assert_unchanged(buf, was, "refused calls: " + name)
