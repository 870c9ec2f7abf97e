"""Guard-band runs of mv_paste_masks_f32, mv_mask_probs_f32 and mv_conv_transpose2x2_bias_act_f32 at the C ABI (`-m gpu`), with the
helpers of tests/_guard.py: every input sits at element offsets 0 - 3 of a buffer whose other elements are NaN (a read outside an
input changes the result), the output in a buffer of sentinels that must come back untouched outside the output and written whole
inside it (the zeros of the paste included: the sentinel is not 0), both store variants are asserted by kernel name, and refused
calls write nothing.  The expected values are those of tests/_mask_ref.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _mask_ref as M  # noqa: E402
from tests._util import philox_f32  # noqa: E402

NAN = float("nan")
DEV = "cuda"
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1), (0, 2), (3, 3)]  # (inputs, output), in elements


def _stream(t):
    return _lib.stream_ptr(t)


@pytest.mark.parametrize("h,w,m,padding", [(37, 53, 28, 1), (40, 56, 28, 1), (9, 600, 14, 0), (11, 301, 1, 2)])
def test_paste_masks_inside_guards(h, w, m, padding):
    lib = _lib.load()
    finite, zero_plane = M.paste_boxes(max(h, 37), w)
    boxes_np = np.concatenate([finite, zero_plane])
    if h < 37:  # the short images: boxes that reach them, the reference's domain does not matter here
        boxes_np[:, 1::2] *= np.float32(h / 37.0)
    masks, boxes = M.paste_masks(9800 + m, len(boxes_np), m), torch.from_numpy(boxes_np)
    r = len(boxes_np)
    want = torch.from_numpy(M.paste(masks.numpy(), boxes_np, h, w, padding)).reshape(r, h, w)
    assert float(G.FLOAT_SENTINEL) != 0.0 and (want == 0).any() and (want != 0).any()  # the zeros must be written, not left
    seen = set()
    for off_in, off_out in OFFSETS:
        mb, mv_ = G.guarded(masks.reshape(r, m, m), torch.float32, DEV, off_in, sentinel=NAN)
        bb, bv = G.guarded(boxes, torch.float32, DEV, (off_in + 1) % 4, sentinel=NAN)
        before = mb.cpu(), bb.cpu()
        yb, yv = G.guarded((r, h, w), torch.float32, DEV, off_out)
        rc = lib.mv_paste_masks_f32(mv_.data_ptr(), bv.data_ptr(), yv.data_ptr(), r, m, padding, h, w, _stream(yv))
        assert rc == 0, lib.mv_last_error()
        what = f"paste_masks {h}x{w} m={m} padding={padding} offsets=({off_in}, {off_out})"
        vec = w % 4 == 0 and yv.data_ptr() % 16 == 0
        assert _lib.last_kernel() == f"k_paste_masks<{'vec16' if vec else 'scalar'}>", (what, _lib.last_kernel())
        seen.add(vec)
        G.assert_same(yv, want, what)  # no sentinel is left inside: `want` holds none
        assert not bool((yv == G.FLOAT_SENTINEL).any()), what
        G.assert_guards_intact(yb, yv, what=what)
        G.assert_unchanged(mb, before[0], what + " masks")
        G.assert_unchanged(bb, before[1], what + " boxes")
    assert seen == ({True, False} if w % 4 == 0 else {False})


@pytest.mark.parametrize("r,c,mh,mw", [(5, 3, 28, 28), (3, 2, 5, 7)])
def test_mask_probs_inside_guards(r, c, mh, mw):
    lib = _lib.load()
    logits = torch.from_numpy(philox_f32(9810 + r, (r, c, mh, mw)) * 12 - 6)
    labels = torch.tensor([0, c - 1, c, 1, -1][:r])
    want = M.mask_probs(logits, labels).reshape(r, mh, mw)
    assert not want[2].any() and want[0].all()
    for off_in, off_out in OFFSETS:
        xb, xv = G.guarded(logits, torch.float32, DEV, off_in, sentinel=NAN)
        lb, lv = G.guarded(labels, torch.int64, DEV, off_in % 2, sentinel=2 ** 40)  # a guard read as a label would select no plane
        before = xb.cpu(), lb.cpu()
        yb, yv = G.guarded((r, mh, mw), torch.float32, DEV, off_out)
        rc = lib.mv_mask_probs_f32(xv.data_ptr(), lv.data_ptr(), yv.data_ptr(), r, c, mh, mw, _stream(yv))
        assert rc == 0, lib.mv_last_error()
        what = f"mask_probs {(r, c, mh, mw)} offsets=({off_in}, {off_out})"
        assert _lib.last_kernel() == "k_mask_probs", what
        G.assert_same(yv, want, what)
        assert not bool((yv == G.FLOAT_SENTINEL).any()), what
        G.assert_guards_intact(yb, yv, what=what)
        G.assert_unchanged(xb, before[0], what + " logits")
        G.assert_unchanged(lb, before[1], what + " labels")


@pytest.mark.parametrize("n,cin,h,w,cout", [(3, 40, 7, 7, 5), (2, 32, 14, 14, 24), (1, 256, 14, 14, 16), (1, 3, 5, 9, 1)])
def test_conv_transpose_inside_guards(n, cin, h, w, cout):
    lib = _lib.load()
    x = philox_f32(9820 + cin, (n, cin, h, w)) * 2 - 1
    wt = (philox_f32(9821 + cin, (cin, cout, 2, 2)) * 2 - 1) * np.float32(2.0 / np.sqrt(cin))
    b = philox_f32(9822 + cin, (cout,)) * 2 - 1
    w4, b4 = M.relaid(wt, b)
    want = torch.from_numpy(M.oracle_conv_transpose(x, wt, b, "relu"))
    seen = set()
    for off_in, off_out in OFFSETS:
        xb, xv = G.guarded(torch.from_numpy(x), torch.float32, DEV, off_in, sentinel=NAN)
        wb, wv = G.guarded(torch.from_numpy(w4), torch.float32, DEV, (off_in + 1) % 4, sentinel=NAN)
        bb, bv = G.guarded(torch.from_numpy(b4), torch.float32, DEV, (off_in + 2) % 4, sentinel=NAN)
        before = xb.cpu(), wb.cpu(), bb.cpu()
        yb, yv = G.guarded((n, cout, 2 * h, 2 * w), torch.float32, DEV, off_out)
        rc = lib.mv_conv_transpose2x2_bias_act_f32(xv.data_ptr(), wv.data_ptr(), bv.data_ptr(), yv.data_ptr(), n, cin, h, w, cout, 1, _stream(yv))
        assert rc == 0, lib.mv_last_error()
        what = f"conv_transpose {(n, cin, h, w, cout)} offsets=({off_in}, {off_out})"
        vec = w % 2 == 0 and yv.data_ptr() % 16 == 0
        kernel = _lib.last_kernel()
        assert kernel.startswith("k_conv1x1_ct<") and kernel.endswith(",vec16>" if vec else ",scalar>"), (what, kernel)
        seen.add(vec)
        G.assert_same(yv, want, what)
        assert not bool((yv == G.FLOAT_SENTINEL).any()), what
        G.assert_guards_intact(yb, yv, what=what)
        for buf, was, name in zip((xb, wb, bb), before, ("x", "w4", "bias4")):
            G.assert_unchanged(buf, was, f"{what} {name}")
    assert seen == ({True, False} if w % 2 == 0 else {False})


def test_refused_calls_write_nothing():
    lib = _lib.load()
    masks, boxes = M.paste_masks(9830, 2, 4).reshape(2, 4, 4), torch.tensor([[1.0, 1.0, 5.0, 4.0], [0.0, 2.0, 7.0, 5.0]])
    (mb, mv_), (bb, bv) = G.guarded(masks, torch.float32, DEV, 1, sentinel=NAN), G.guarded(boxes, torch.float32, DEV, 2, sentinel=NAN)
    labels = torch.tensor([0, 1])
    lb, lv = G.guarded(labels, torch.int64, DEV, 1)
    yb, yv = G.guarded((2, 6, 8), torch.float32, DEV, 2)
    before = [t.cpu() for t in (mb, bb, lb, yb)]
    m, b, lab, y = mv_.data_ptr(), bv.data_ptr(), lv.data_ptr(), yv.data_ptr()
    s = _stream(yv)
    for args, status, text in (((m, b, None, 2, 4, 1, 6, 8), -1, "null pointer"), ((None, b, y, 2, 4, 1, 6, 8), -1, "null pointer"),
                               ((m, b, y, 2, 0, 1, 6, 8), -1, "bad shape"), ((m, b, y, 2, 4, -1, 6, 8), -1, "bad shape"),
                               ((m, b, y, -2, 4, 1, 6, 8), -1, "bad shape"), ((m, b, m + 8, 2, 4, 1, 6, 8), -1, "must not overlap"),
                               ((m, y + 4 * 95, y, 2, 4, 1, 6, 8), -1, "must not overlap")):
        rc = lib.mv_paste_masks_f32(*args, s)
        assert rc == status and text in lib.mv_last_error().decode(), (args, rc, lib.mv_last_error())
    # (2, 2, 2, 2) logits in the 32 floats of `masks`, (2, 2, 2) probabilities in `y`
    for args, status, text in (((m, lab, None, 2, 2, 2, 2), -1, "null pointer"), ((m, None, y, 2, 2, 2, 2), -1, "null pointer"),
                               ((m, lab, y, 2, 0, 2, 2), -1, "bad shape"), ((m, lab + 4, y, 2, 2, 2, 2), -1, "8-byte aligned"),
                               ((m, lab, m + 60, 2, 2, 2, 2), -1, "must not overlap")):
        rc = lib.mv_mask_probs_f32(*args, s)
        assert rc == status and text in lib.mv_last_error().decode(), (args, rc, lib.mv_last_error())
    # x (1, 2, 2, 2) and w4 (4, 2) in `masks`, bias4 in `boxes`, y (1, 1, 4, 4) in `y`
    for args, status, text in (((m, m + 32, b, None, 1, 2, 2, 2, 1, 1), -1, "null pointer"), ((m, None, b, y, 1, 2, 2, 2, 1, 1), -1, "null pointer"),
                               ((m, m + 32, b, y, 1, 2, 2, 2, 1, 4), -1, "bad activation code"), ((m, m + 32, b, y, 1, 2, 0, 2, 1, 1), -1, "bad shape"),
                               ((m, m + 32, b, m + 16, 1, 2, 2, 2, 1, 1), -1, "must not overlap"), ((m, m + 32, y + 32, y, 1, 2, 2, 2, 1, 1), -1, "must not overlap")):
        rc = lib.mv_conv_transpose2x2_bias_act_f32(*args, s)
        assert rc == status and text in lib.mv_last_error().decode(), (args, rc, lib.mv_last_error())
    torch.cuda.synchronize()
    for buf, was, name in zip((mb, bb, lb, yb), before, ("masks", "boxes", "labels", "output")):
        G.assert_unchanged(buf, was, "refused calls: " + name)
