"""Guard-band runs of mv_interpolate_bilinear_f32 and mv_detection_batch_f32 at the C ABI (`-m gpu`), with the helpers of
tests/_guard.py: every input sits at element offsets 0 - 3 of a buffer whose other elements are NaN (a read outside an image changes
the result), the output in a buffer of sentinels that must come back untouched outside the output and written whole inside it (the
padding of the batch included: the sentinel is not 0), and refused calls write nothing.  The expected values are the oracle's
(tests/_interp_ref.py)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _interp_ref as R  # noqa: E402
from tests._util import philox_f32  # noqa: E402

NAN = float("nan")
DEV = "cuda"
OFFSETS = [(0, 0), (1, 0), (2, 3), (3, 1), (0, 2), (3, 3)]  # (inputs, output), in elements
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _ints(v):
    return (C.c_int * len(v))(*v)


def _stream(t):
    return _lib.stream_ptr(t)


@pytest.mark.parametrize("h,w,oh,ow", [(5, 7, 9, 13), (23, 31, 7, 5), (6, 10, 11, 260), (9, 9, 9, 12)])
def test_interpolate_inside_guards(h, w, oh, ow):
    lib = _lib.load()
    x = torch.from_numpy(philox_f32(9400 + h, (3, h, w)) * 2 - 1)
    want = torch.from_numpy(R.interpolate(x.numpy(), oh, ow))
    for off_in, off_out in OFFSETS:
        xb, xv = G.guarded(x, torch.float32, DEV, off_in, sentinel=NAN)
        before = xb.cpu()
        yb, yv = G.guarded((3, oh, ow), torch.float32, DEV, off_out)
        rc = lib.mv_interpolate_bilinear_f32(xv.data_ptr(), yv.data_ptr(), 3, h, w, oh, ow, _stream(yv))
        assert rc == 0, lib.mv_last_error()
        what = f"interpolate {h}x{w} -> {oh}x{ow} offsets=({off_in}, {off_out})"
        vec = ow % 4 == 0 and yv.data_ptr() % 16 == 0
        assert _lib.last_kernel() == f"k_interp_batch<plain,{'vec16' if vec else 'scalar'}>", (what, _lib.last_kernel())
        G.assert_same(yv, want, what)
        G.assert_guards_intact(yb, yv, what=what)
        G.assert_unchanged(xb, before, what + " input")


@pytest.mark.parametrize("div", [32, 3])
def test_detection_batch_inside_guards(div):
    lib = _lib.load()
    shapes = [(40, 56), (50, 37), (33, 33)]
    sizes = [R.resized_size(h, w, 64, 96) for h, w in shapes]
    images = [torch.from_numpy(philox_f32(9410 + i, (3, h, w))) for i, (h, w) in enumerate(shapes)]
    want = R.detection_batch(images, sizes, MEAN, STD, div)
    n, c, hp, wp = want.shape
    assert float(G.FLOAT_SENTINEL) != 0.0 and (want == 0).any()  # the padding must be written, not left
    mean, std = _lib.taps(MEAN), _lib.taps(STD)
    for off_in, off_out in OFFSETS:
        ins = [G.guarded(im, torch.float32, DEV, (off_in + i) % 4, sentinel=NAN) for i, im in enumerate(images)]
        before = [b.cpu() for b, _ in ins]
        yb, yv = G.guarded((n, c, hp, wp), torch.float32, DEV, off_out)
        rc = lib.mv_detection_batch_f32(_lib.pointer_table([v for _, v in ins]), _ints([h for h, _ in shapes]), _ints([w for _, w in shapes]),
                                        _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes]), n, c, mean, std, yv.data_ptr(), hp, wp,
                                        _stream(yv))
        assert rc == 0, lib.mv_last_error()
        what = f"detection_batch div={div} offsets=({off_in}, {off_out})"
        G.assert_same(yv, want, what)  # no sentinel is left inside: `want` holds none
        assert not bool((yv == G.FLOAT_SENTINEL).any()), what
        G.assert_guards_intact(yb, yv, what=what)
        for (b, _), was in zip(ins, before):
            G.assert_unchanged(b, was, what + " input")


def test_refused_calls_write_nothing():
    lib = _lib.load()
    x = torch.from_numpy(philox_f32(9420, (3, 6, 8)))
    (xb, xv), (yb, yv) = G.guarded(x, torch.float32, DEV, 1, sentinel=NAN), G.guarded((3, 12, 16), torch.float32, DEV, 2)
    before = xb.cpu(), yb.cpu()
    for args, text in (((xv.data_ptr(), None, 3, 6, 8, 12, 16), "null pointer"), ((None, yv.data_ptr(), 3, 6, 8, 12, 16), "null pointer"),
                       ((xv.data_ptr(), yv.data_ptr(), 3, 6, 8, 0, 16), "bad shape"), ((xv.data_ptr(), yv.data_ptr(), -1, 6, 8, 12, 16), "bad shape"),
                       ((xv.data_ptr(), xv.data_ptr() + 8, 3, 6, 8, 12, 16), "must not overlap")):
        rc = lib.mv_interpolate_bilinear_f32(*args, _stream(yv))
        assert rc == -1 and text in lib.mv_last_error().decode(), (args, lib.mv_last_error())
    mean, std, zero = _lib.taps(MEAN), _lib.taps(STD), _lib.taps([0.2, 0.0, 0.2])
    tables = dict(hs=[6], ws=[8], ohs=[12], ows=[16])

    def batch(y=yv.data_ptr(), xs=(xv,), c=3, m=mean, s=std, hp=12, wp=16, **over):
        t = {**tables, **over}
        return lib.mv_detection_batch_f32(_lib.pointer_table(list(xs)), _ints(t["hs"]), _ints(t["ws"]), _ints(t["ohs"]), _ints(t["ows"]), len(xs), c, m, s,
                                          y, hp, wp, _stream(yv))
    for kw, rc_want, text in ((dict(y=None), -1, "null pointer"), (dict(m=None), -1, "null pointer"), (dict(s=zero), -1, "std evaluated to zero"),
                              (dict(c=17), -2, "up to 16 channels"), (dict(ohs=[13]), -1, "does not fit the batch"), (dict(ws=[0]), -1, "bad size"),
                              (dict(y=xv.data_ptr() + 16), -1, "must not overlap"), (dict(wp=0), -1, "bad shape")):
        rc = batch(**kw)
        assert rc == rc_want and text in lib.mv_last_error().decode(), (kw, rc, lib.mv_last_error())
    torch.cuda.synchronize()
    G.assert_unchanged(xb, before[0], "refused calls: input")
    G.assert_unchanged(yb, before[1], "refused calls: output")
