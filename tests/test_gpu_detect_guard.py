"""Guard-band runs of mv_nms_f32 and mv_roi_align_f32 at the C ABI (`-m gpu`), with the helpers of tests/_guard.py as
tests/test_gpu_guard_bands.py uses them: inputs, outputs and the nms workspace each lie inside a sentinel-filled buffer, the
outputs at element offsets 0 - 3, at the ragged sizes n = 65 and 130 (nms) and k = 65 with a 7 x 7 output (roi_align).  Every
case asserts that the result equals the reference (tests/_detect_ref.py), that nothing outside the outputs and the workspace
changed, that the inputs (NaN around them: a stray read would change the result) are untouched, and -- nms -- that the result
does not depend on what the workspace held (0xFF, then 0x00) and that keep_out is written up to the count and no further."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests._detect_cases import nms_case, nms_reference, roi_input, roi_reference  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F32, I64 = torch.float32, torch.int64


class _OnDevice:
    device = torch.device(DEV)


def _stream():
    return _lib.stream_ptr(_OnDevice)


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("kind", ["clustered", "ties"])
def test_nms(kind, n):
    lib = _lib.load()
    boxes, scores = nms_case(kind, n)
    want = torch.from_numpy(nms_reference(kind, n, 0.5).copy())
    ws_bytes = int(lib.mv_nms_workspace_bytes(n))
    assert ws_bytes > 0
    sentinel = G.sentinel_for(I64)
    for off in range(4):
        what = f"nms {kind} n={n} offset={off}"
        bbuf, bv = G.guarded(torch.from_numpy(boxes.copy()), F32, DEV, off, sentinel=NAN)
        sbuf, sv = G.guarded(torch.from_numpy(scores.copy()), F32, DEV, 3 - off, sentinel=NAN)
        b_before, s_before = bbuf.cpu(), sbuf.cpu()
        results = []
        for garbage in (0xFF, 0x00):
            tag = f"{what} workspace={garbage:#04x}"
            kbuf, kv = G.guarded((n,), I64, DEV, off)
            cbuf, cv = G.guarded((1,), I64, DEV, (off + 1) % 4)
            wbuf, ws = G.guarded_workspace(ws_bytes, DEV, garbage)
            _lib.check(lib.mv_nms_f32(bv.data_ptr(), sv.data_ptr(), n, 0.5, kv.data_ptr(), cv.data_ptr(), ws.data_ptr(), ws_bytes, _stream()))
            torch.cuda.synchronize()
            tag = f"{tag} [{_lib.last_kernel()}]"
            G.assert_guards_intact(kbuf, kv, what=tag + ": keep_out")
            G.assert_guards_intact(cbuf, cv, what=tag + ": keep_count_out")
            G.assert_guards_intact(wbuf, ws, what=tag + ": workspace")
            G.assert_unchanged(bbuf, b_before, tag + ": boxes")
            G.assert_unchanged(sbuf, s_before, tag + ": scores")
            count = int(cv.item())
            assert count == want.numel(), (tag, count, want.numel())
            G.assert_same(kv[:count], want, tag)
            assert bool((kv[count:].cpu() == sentinel).all()), tag + ": keep_out was written past the count"
            results.append(kv.cpu())
        G.assert_unchanged(results[1], results[0], what + ": the result depends on the workspace's content")


def test_roi_align():
    lib = _lib.load()
    cfg = ((7, 7), -1, True, 0.25)
    f32, _, rois = roi_reference("main", cfg, extra=51)
    x = roi_input("main")
    n, c, h, w = x.shape
    k = len(rois)
    assert k == 65
    want = torch.from_numpy(f32.copy())
    for off in range(4):
        what = f"roi_align k={k} 7x7 offset={off}"
        xbuf, xv = G.guarded(torch.from_numpy(x.copy()), F32, DEV, 3 - off, sentinel=NAN)
        rbuf, rv = G.guarded(torch.from_numpy(rois.copy()), F32, DEV, (off + 2) % 4, sentinel=NAN)
        x_before, r_before = xbuf.cpu(), rbuf.cpu()
        ybuf, yv = G.guarded((k, c, 7, 7), F32, DEV, off)
        _lib.check(lib.mv_roi_align_f32(xv.data_ptr(), rv.data_ptr(), yv.data_ptr(), n, c, h, w, k, 7, 7, 0.25, -1, 1, _stream()))
        torch.cuda.synchronize()
        tag = f"{what} [{_lib.last_kernel()}]"
        G.assert_guards_intact(ybuf, yv, what=tag + ": output")
        G.assert_same(yv, want, tag)
        G.assert_unchanged(xbuf, x_before, tag + ": input")
        G.assert_unchanged(rbuf, r_before, tag + ": rois")
