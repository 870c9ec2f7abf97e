"""Guard-band runs of mv_box_iou_f32, mv_masks_to_boxes_u8 / _f32 and mv_multiscale_roi_align_f32 at the C ABI (`-m gpu`), with the
helpers of tests/_guard.py as tests/test_gpu_detect_guard.py uses them: every tensor lies inside a sentinel-filled buffer, each in
turn at element offsets 0 - 3 (an output of box_iou at an odd offset cannot take 16-byte stores: both store paths run, and
mv_last_kernel says which), the masks_to_boxes workspace is sized exactly and holds 0xFF, then 0x00.  Every case asserts that the
result equals the reference, that nothing outside the outputs and the workspace changed, that the inputs (NaN around the float
ones: a stray read would change the result) are untouched, and that a refused call writes nothing."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _boxes_ref as B  # noqa: E402
from tests import _guard as G  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


class _OnDevice:
    device = torch.device(DEV)


def _stream():
    return _lib.stream_ptr(_OnDevice)


def _untouched(buf, view, what):
    """An output that a refused call must not have written: the view still holds the sentinel, as its guards do."""
    G.assert_guards_intact(buf, view, what=what)
    want = G._fill(view.numel(), view.dtype, G.sentinel_for(view.dtype)).view(view.shape)
    G.assert_unchanged(view, want, what + ": written by a refused call")


@pytest.mark.parametrize("mode", [0, 1, 2], ids=B.MODES)
@pytest.mark.parametrize("shape", [(65, 260), (33, 257)], ids=str)
def test_box_iou(shape, mode):
    lib = _lib.load()
    n, m = shape
    b1, b2 = B.pair_case(n, m)
    want = torch.from_numpy(B.pair_reference(B.MODES[mode], n, m).copy())
    kernels = set()
    for off in range(4):
        what = f"{B.MODES[mode]} {shape} offset={off}"
        abuf, av = G.guarded(torch.from_numpy(b1.copy()), F32, DEV, 3 - off, sentinel=NAN)
        bbuf, bv = G.guarded(torch.from_numpy(b2.copy()), F32, DEV, (off + 2) % 4, sentinel=NAN)
        a_before, b_before = abuf.cpu(), bbuf.cpu()
        obuf, ov = G.guarded((n, m), F32, DEV, G.ALIGNED + off)
        assert (ov.data_ptr() % 16 == 0) == (off == 0)
        _lib.check(lib.mv_box_iou_f32(av.data_ptr(), bv.data_ptr(), ov.data_ptr(), n, m, mode, _stream()))
        torch.cuda.synchronize()
        kernel = _lib.last_kernel()
        assert kernel.endswith("vec16>" if (off == 0 and m % 4 == 0) else "scalar>"), (what, kernel)
        kernels.add(kernel)
        tag = f"{what} [{kernel}]"
        G.assert_guards_intact(obuf, ov, what=tag + ": output")
        G.assert_same(ov, want, tag)
        G.assert_unchanged(abuf, a_before, tag + ": boxes1")
        G.assert_unchanged(bbuf, b_before, tag + ": boxes2")
    assert len(kernels) == (2 if m % 4 == 0 else 1)  # both store paths ran, on the same values

    obuf, ov = G.guarded((n, m), F32, DEV, G.ALIGNED)
    for rc, args in ((-1, (av.data_ptr(), bv.data_ptr(), ov.data_ptr(), n, m, 3)), (-1, (av.data_ptr(), bv.data_ptr(), ov.data_ptr(), -n, m, mode)),
                     (-1, (None, bv.data_ptr(), ov.data_ptr(), n, m, mode)), (-1, (ov.data_ptr(), bv.data_ptr(), ov.data_ptr(), n, m, mode)),
                     (0, (av.data_ptr(), bv.data_ptr(), ov.data_ptr(), n, 0, mode)), (0, (av.data_ptr(), bv.data_ptr(), ov.data_ptr(), 0, m, mode))):
        assert lib.mv_box_iou_f32(*args, _stream()) == rc, args
    torch.cuda.synchronize()
    _untouched(obuf, ov, f"{B.MODES[mode]} {shape}")


@pytest.mark.parametrize("dtype", [U8, F32], ids=str)
def test_masks_to_boxes(dtype):
    lib = _lib.load()
    fn = lib.mv_masks_to_boxes_f32 if dtype == F32 else lib.mv_masks_to_boxes_u8
    n, h, w = 3, 2 * B.kernel_constant("kMtbChunkRows") + 5, 131  # rows start at every alignment; three chunks per mask
    ws_bytes = int(lib.mv_masks_to_boxes_workspace_bytes(n))
    assert ws_bytes == 16 * n
    for empty in (False, True):
        masks = torch.from_numpy(B.mask_case(n, h, w, seed=3)).to(dtype)
        if empty:
            masks[1] = 0
        want = torch.zeros((n, 4)) if empty else B.masks_to_boxes_ref(masks)
        if empty:
            want[0], want[2] = B.masks_to_boxes_ref(masks[0:1])[0], B.masks_to_boxes_ref(masks[2:3])[0]
        for off in range(4):
            what = f"masks_to_boxes {dtype} empty={empty} offset={off}"
            mbuf, mv = G.guarded(masks, dtype, DEV, off, sentinel=NAN if dtype == F32 else 0xA5)  # set elements around the masks
            m_before = mbuf.cpu()
            results = []
            for garbage in (0xFF, 0x00):
                tag = f"{what} workspace={garbage:#04x}"
                bbuf, bv = G.guarded((n, 4), F32, DEV, 3 - off)
                fbuf, fv = G.guarded((1,), I32, DEV, (off + 1) % 4)
                fv.zero_()
                wbuf, ws = G.guarded_workspace(ws_bytes, DEV, garbage)
                _lib.check(fn(mv.data_ptr(), bv.data_ptr(), fv.data_ptr(), n, h, w, ws.data_ptr(), ws_bytes, _stream()))
                torch.cuda.synchronize()
                tag = f"{tag} [{_lib.last_kernel()}]"
                G.assert_guards_intact(bbuf, bv, what=tag + ": boxes")
                G.assert_guards_intact(fbuf, fv, what=tag + ": empty_flag")
                G.assert_guards_intact(wbuf, ws, what=tag + ": workspace")
                G.assert_unchanged(mbuf, m_before, tag + ": masks")
                G.assert_same(bv, want, tag)
                assert int(fv.item()) == int(empty), tag
                results.append(bv.cpu())
            G.assert_unchanged(results[1], results[0], what + ": the result depends on the workspace's content")

    bbuf, bv = G.guarded((n, 4), F32, DEV, 0)
    fbuf, fv = G.guarded((1,), I32, DEV, 0)
    wbuf, ws = G.guarded_workspace(ws_bytes, DEV, 0xFF)
    w_before = wbuf.cpu()
    p = (mv.data_ptr(), bv.data_ptr(), fv.data_ptr())
    for rc, args in ((-1, p + (n, h, w, ws.data_ptr(), ws_bytes - 1)), (-1, p + (n, h, w, None, 0)), (-1, p + (n, -h, w, ws.data_ptr(), ws_bytes)),
                     (-1, p + (n, h, w, ws.data_ptr() + 4, ws_bytes)), (-1, (mv.data_ptr(), bv.data_ptr(), None, n, h, w, ws.data_ptr(), ws_bytes)),
                     (0, p + (0, h, w, ws.data_ptr(), ws_bytes))):
        assert fn(*args, _stream()) == rc, args
    torch.cuda.synchronize()
    _untouched(bbuf, bv, "masks_to_boxes boxes")
    _untouched(fbuf, fv, "masks_to_boxes empty_flag")
    G.assert_unchanged(wbuf, w_before, "masks_to_boxes: the workspace was written by a refused call")


def test_multiscale_roi_align():
    lib = _lib.load()
    feats = B.fpn_features()
    boxes = B.fpn_boxes(per_level=4)
    rois = np.concatenate([np.concatenate([np.full((len(b), 1), i, np.float32), b], 1) for i, b in enumerate(boxes)], 0)
    from cpu_vision_amd import ops
    levels = ops.LevelMapper(2, 5, canonical_scale=B.CANONICAL_SCALE, canonical_level=B.CANONICAL_LEVEL)(
        [torch.from_numpy(b.copy()) for b in boxes])
    levels[3] = 7  # outside the maps: zeros
    assert sorted(set(levels.tolist())) == [0, 1, 2, 3, 7]
    scales = [0.25, 0.125, 0.0625, 0.03125]
    k, (n, c) = len(rois), feats[0].shape[:2]
    want = torch.from_numpy(B.multiscale_ref(feats, rois, levels.numpy(), scales, (7, 7), 2))
    assert not bool(want[3].any())
    hs = (ctypes.c_int * 4)(*[f.shape[2] for f in feats])
    ws = (ctypes.c_int * 4)(*[f.shape[3] for f in feats])
    sc = (ctypes.c_double * 4)(*scales)
    for off in range(4):
        what = f"multiscale_roi_align k={k} 7x7 offset={off}"
        maps = [G.guarded(torch.from_numpy(f.copy()), F32, DEV, (off + i) % 4, sentinel=NAN) for i, f in enumerate(feats)]
        rbuf, rv = G.guarded(torch.from_numpy(rois.copy()), F32, DEV, (off + 2) % 4, sentinel=NAN)
        lbuf, lv = G.guarded(levels, I64, DEV, off, sentinel=1)  # a stray read of a level would pick another map
        before = [buf.cpu() for buf, _ in maps] + [rbuf.cpu(), lbuf.cpu()]
        ybuf, yv = G.guarded((k, c, 7, 7), F32, DEV, off)
        xs = _lib.pointer_table([view for _, view in maps])
        _lib.check(lib.mv_multiscale_roi_align_f32(xs, hs, ws, sc, 4, rv.data_ptr(), lv.data_ptr(), yv.data_ptr(), n, c, k, 7, 7, 2, 0, _stream()))
        torch.cuda.synchronize()
        tag = f"{what} [{_lib.last_kernel()}]"
        G.assert_guards_intact(ybuf, yv, what=tag + ": output")
        G.assert_same(yv, want, tag)
        for (buf, _), was, name in zip(maps + [(rbuf, rv), (lbuf, lv)], before, ["map 0", "map 1", "map 2", "map 3", "rois", "levels"]):
            G.assert_unchanged(buf, was, f"{tag}: {name}")

    ybuf, yv = G.guarded((k, c, 7, 7), F32, DEV, 0)
    common = (rv.data_ptr(), lv.data_ptr(), yv.data_ptr(), n, c)
    for rc, args in ((-2, (xs, hs, ws, sc, 9) + common + (k, 7, 7, 2, 0)), (-1, (xs, hs, ws, sc, 4) + common + (-k, 7, 7, 2, 0)),
                     (-1, (None, hs, ws, sc, 4) + common + (k, 7, 7, 2, 0)), (-1, (xs, hs, ws, sc, 4, yv.data_ptr(), lv.data_ptr(), yv.data_ptr(), n, c, k, 7, 7, 2, 0)),
                     (0, (xs, hs, ws, sc, 4) + common + (0, 7, 7, 2, 0)), (0, (xs, hs, ws, sc, 4) + common + (k, 0, 7, 2, 0))):
        assert lib.mv_multiscale_roi_align_f32(*args, _stream()) == rc, args
    torch.cuda.synchronize()
    _untouched(ybuf, yv, "multiscale_roi_align output")
