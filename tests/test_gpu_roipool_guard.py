"""Guard-band runs of mv_roi_pool_f32, mv_ps_roi_pool_f32 and mv_ps_roi_align_f32 at the C ABI (`-m gpu`), with the helpers of
tests/_guard.py as tests/test_gpu_detect_guard.py uses them: k = 65 rois, a 7 x 7 output, spatial_scale 0.25 on the 13 x 17 map.
BOTH outputs lie in sentinel-filled buffers at element offsets 0 - 3 and the inputs inside NaN guards (a stray read would change
the result).  Every case asserts that both results equal the restatement (tests/_roipool_ref.py; the outputs are pre-filled with
the sentinel, so equality proves that every element was written), that nothing outside the outputs changed and that the inputs
are untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests._roipool_cases import OPS, input_shape, pool_input, pool_reference  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F32, I32 = torch.float32, torch.int32


class _OnDevice:
    device = torch.device(DEV)


def _stream():
    return _lib.stream_ptr(_OnDevice)


@pytest.mark.parametrize("op", OPS)
def test_both_outputs_inside_guard_bands(op):
    lib = _lib.load()
    entry = getattr(lib, f"mv_{op}_f32")
    cfg = ((7, 7), 0.25) + ((-1,) if op == "ps_roi_align" else ())
    (y32, s32), _, rois = pool_reference(op, "main", cfg, extra=51)
    x = pool_input(op, "main", (7, 7))
    n, c, h, w = input_shape(op, "main", (7, 7))
    assert x.shape == (n, c, h, w) and (h, w) == (13, 17)
    k = len(rois)
    assert k == 65
    want_y, want_s = torch.from_numpy(y32.copy()), torch.from_numpy(s32.copy())
    tail = (-1,) if op == "ps_roi_align" else ()
    for off in range(4):
        what = f"{op} k={k} 7x7 offset={off}"
        xbuf, xv = G.guarded(torch.from_numpy(x.copy()), F32, DEV, 3 - off, sentinel=NAN)
        rbuf, rv = G.guarded(torch.from_numpy(rois.copy()), F32, DEV, (off + 2) % 4, sentinel=NAN)
        x_before, r_before = xbuf.cpu(), rbuf.cpu()
        ybuf, yv = G.guarded(tuple(y32.shape), F32, DEV, off)
        sbuf, sv = G.guarded(tuple(s32.shape), I32, DEV, (off + 1) % 4)
        _lib.check(entry(xv.data_ptr(), rv.data_ptr(), yv.data_ptr(), sv.data_ptr(), n, c, h, w, k, 7, 7, 0.25, *tail, _stream()))
        torch.cuda.synchronize()
        tag = f"{what} [{_lib.last_kernel()}]"
        G.assert_guards_intact(ybuf, yv, what=tag + ": output")
        G.assert_guards_intact(sbuf, sv, what=tag + ": second output")
        G.assert_same(yv, want_y, tag)
        G.assert_same(sv, want_s, tag + ": second output")
        G.assert_unchanged(xbuf, x_before, tag + ": input")
        G.assert_unchanged(rbuf, r_before, tag + ": rois")
