"""ops.nms / batched_nms / roi_align on the MI355X (`-m gpu`) against tests/_detect_ref.py, the reference's CPU kernels restated
in numpy (and against torchvision's own CPU ops where that package is importable; nothing here requires it).

nms returns exactly the reference's index list: the IoU is one chain of float32 operations without any freedom of order, and
the inputs (tests/_detect_cases.py) hold no pair whose IoU lies within 1e-6 of a tested threshold (R.tie_margin_ok).
roi_align is bit-for-bit the float32 restatement (separately rounded products and sums, samples in ascending (iy, ix) order);
independently every case asserts  max|kernel - float64| <= 2 max|float32 restatement - float64|  on the same inputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, ops  # noqa: E402
from tests import _detect_ref as R  # noqa: E402
from tests._detect_cases import (NMS_KINDS, NMS_SIZES, NMS_THRESHOLDS, ROI_CONFIGS, nms_case, nms_reference, roi_input,  # noqa: E402
                                 roi_reference)

try:
    import torchvision.ops as tv_ops
except Exception:  # not installed, or built against another torch
    tv_ops = None

DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _nms(boxes, scores, thr):
    b, s = _dev(boxes), _dev(scores)
    b0, s0 = b.clone(), s.clone()
    keep = ops.nms(b, s, thr)
    assert keep.dtype == torch.int64 and keep.device.type == "cuda" and keep.ndim == 1
    assert torch.equal(b, b0) and torch.equal(s, s0), "nms changed its inputs"
    return keep.cpu().numpy()


# ---- nms ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", NMS_KINDS)
@pytest.mark.parametrize("n", NMS_SIZES)
def test_nms_equals_the_reference(kind, n):
    boxes, scores = nms_case(kind, n)
    for thr in NMS_THRESHOLDS:
        want = nms_reference(kind, n, thr)
        got = _nms(boxes, scores, thr)
        assert got.tolist() == want.tolist(), f"{kind} n={n} iou_threshold={thr}: {len(got)} kept, reference {len(want)}"
        if tv_ops is not None and n:
            tv = tv_ops.nms(torch.from_numpy(np.array(boxes)), torch.from_numpy(np.array(scores)), thr)
            assert got.tolist() == tv.tolist(), f"{kind} n={n} iou_threshold={thr}: differs from torchvision's CPU nms"
    if n > 2 and kind == "clustered":
        assert len(nms_reference(kind, n, 0.5)) < n, "the clustered boxes suppress nothing: the case tests no suppression"
    if n > 1 and kind == "identical":
        assert len(nms_reference(kind, n, 0.5)) == 1 and len(nms_reference(kind, n, 1.0)) == n
    if kind == "disjoint":
        assert len(nms_reference(kind, n, 0.0)) == n


@pytest.mark.parametrize("n", [65, 130, 1000])
def test_nms_is_invariant_under_a_permutation_of_its_input(n):
    boxes, _ = nms_case("clustered", n)
    g = np.random.default_rng(n)
    scores = g.permutation(n).astype(np.float32) / n  # distinct: the order does not depend on the input positions
    perm = g.permutation(n)
    keep = _nms(boxes, scores, 0.5)
    keep_p = perm[_nms(boxes[perm], scores[perm], 0.5)]
    assert keep.tolist() == R.nms_ref(boxes, scores, 0.5).tolist()
    assert sorted(keep_p.tolist()) == sorted(keep.tolist())
    assert keep_p.tolist() == keep.tolist()  # and, the scores being distinct, in the same order


def test_nms_orders_equal_scores_by_index():
    boxes, _ = nms_case("disjoint", 130)
    scores = np.zeros(130, dtype=np.float32)
    scores[70:] = -0.0  # -0 == +0: still one group of equal scores
    assert _nms(boxes, scores, 0.5).tolist() == list(range(130))
    scores[::2] = 1.0
    assert _nms(boxes, scores, 0.5).tolist() == list(range(0, 130, 2)) + list(range(1, 130, 2))


def test_nms_on_a_side_stream_and_from_views():
    boxes, scores = nms_case("clustered", 130)
    want = nms_reference("clustered", 130, 0.5).tolist()
    side = torch.cuda.Stream()
    b, s = _dev(boxes), _dev(scores)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        keep = ops.nms(b, s, 0.5)
    side.synchronize()
    assert keep.cpu().tolist() == want
    wide = torch.zeros((130, 6), device=DEV)
    wide[:, 1:5] = b
    assert ops.nms(wide[:, 1:5], s, 0.5).cpu().tolist() == want  # a non-contiguous view of the boxes


def test_nms_registered_operator_and_dtype_gate():
    ops.register_torchvision_op()
    boxes, scores = nms_case("clustered", 65)
    keep = torch.ops.torchvision.nms(_dev(boxes), _dev(scores), 0.5)
    assert keep.cpu().tolist() == nms_reference("clustered", 65, 0.5).tolist()
    with pytest.raises(NotImplementedError):
        ops.nms(_dev(boxes).double(), _dev(scores).double(), 0.5)
    with pytest.raises(_lib.Mi355VisionError):
        ops.nms(_dev(boxes), torch.from_numpy(np.array(scores)), 0.5)


# ---- batched_nms -------------------------------------------------------------------------------------------------------------------
def test_batched_nms_equals_per_class_nms_merged_by_score():
    n, classes = 200, 3
    boxes, scores = nms_case("clustered", n)
    # coordinates on a grid of 1 / 4: boxes + idxs * (max + 1) is then exact in float32, so the moved boxes of one class have
    # the float32 IoUs of the unmoved ones and the per-class reference applies bit for bit
    boxes = (np.round(boxes * 4) / 4).astype(np.float32)
    assert R.tie_margin_ok(boxes, 0.5)
    idxs = np.random.default_rng(5).integers(0, classes, n)
    kept = np.concatenate([np.flatnonzero(idxs == c)[R.nms_ref(boxes[idxs == c], scores[idxs == c], 0.5)] for c in range(classes)])
    want = kept[np.lexsort((kept, -scores[kept]))]
    b, s, i = _dev(boxes), _dev(scores), _dev(idxs)
    b0, s0, i0 = b.clone(), s.clone(), i.clone()
    got = ops.batched_nms(b, s, i, 0.5)
    assert got.dtype == torch.int64 and got.cpu().tolist() == want.tolist()
    assert torch.equal(b, b0) and torch.equal(s, s0) and torch.equal(i, i0)
    assert len(want) > len(R.nms_ref(boxes, scores, 0.5)), "the classes keep nothing apart: the case does not test them"
    empty = ops.batched_nms(b[:0], s[:0], i[:0], 0.5)
    assert empty.dtype == torch.int64 and empty.shape == (0,) and empty.device.type == "cuda"


# ---- roi_align ---------------------------------------------------------------------------------------------------------------------
def _check_roi(got, f32, f64, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == f32.shape, (what, got.shape, f32.shape)
    err = float(np.abs(got.astype(np.float64) - f64).max()) if got.size else 0.0
    ref_err = float(np.abs(f32.astype(np.float64) - f64).max()) if got.size else 0.0
    print(f"{what}: max|kernel - f64| = {err:.3e}, max|float32 restatement - f64| = {ref_err:.3e}, "
          f"{int((got != f32).sum())} of {got.size} elements differ from the restatement")
    assert err <= 2 * ref_err, f"{what}: error {err:.3e} against float64 exceeds twice the restatement's own {ref_err:.3e}"
    assert np.array_equal(got, f32), f"{what}: {int((got != f32).sum())} of {got.size} elements differ from the float32 restatement"


def _roi_align(x, rois, cfg):
    out, ratio, aligned, scale = cfg
    x0 = x.clone()
    r0 = [r.clone() for r in rois] if isinstance(rois, list) else rois.clone()
    y = ops.roi_align(x, rois, out, scale, ratio, aligned)
    assert torch.equal(x, x0), "roi_align changed its input"
    assert all(torch.equal(a, b) for a, b in zip(rois, r0)) if isinstance(rois, list) else torch.equal(rois, r0)
    return y


@pytest.mark.parametrize("cfg", ROI_CONFIGS, ids=str)
def test_roi_align_equals_the_float32_restatement(cfg):
    for shape in ("main", "tiny"):
        f32, f64, rois = roi_reference(shape, cfg)
        x = _dev(roi_input(shape))
        got = _roi_align(x, _dev(rois), cfg)
        _check_roi(got, f32, f64, f"roi_align {shape} {cfg}")
        if tv_ops is not None:
            out, ratio, aligned, scale = cfg
            tv = tv_ops.roi_align(torch.from_numpy(np.array(roi_input(shape))), torch.from_numpy(np.array(rois)), out, scale, ratio, aligned)
            assert np.array_equal(got.cpu().numpy(), tv.numpy()), f"roi_align {shape} {cfg}: differs from torchvision's CPU roi_align"


@pytest.mark.parametrize("k", [0, 1, 65])
def test_roi_align_roi_counts(k):
    cfg = ((7, 7), -1, True, 0.25)
    f32, f64, rois = roi_reference("main", cfg, extra=51)
    assert len(rois) == 65
    x = _dev(roi_input("main"))
    got = _roi_align(x, _dev(rois[:k]).reshape(k, 5), cfg)
    _check_roi(got, f32[:k], f64[:k], f"roi_align k={k}")


def test_roi_align_list_of_boxes_int_output_size_and_module():
    cfg = ((2, 3), 2, False, 1.0)
    x = _dev(roi_input("main"))
    per_image = [np.array([[2.3, 1.7, 9.6, 8.2], [0.0, 0.0, 17.0, 13.0]], np.float32), np.array([[4.5, 0.0, 9.5, 4.0]], np.float32)]
    rois = R.convert_boxes_to_roi_format_ref(per_image)
    args = (roi_input("main"), rois, cfg[0], cfg[3], cfg[1], cfg[2])
    got = _roi_align(x, [_dev(b) for b in per_image], cfg)
    _check_roi(got, R.roi_align_ref(*args, np.float32), R.roi_align_ref(*args, np.float64), "roi_align list of boxes")
    sq = (roi_input("main"), rois, (3, 3), 0.5, -1, True)
    got = ops.RoIAlign(3, 0.5, -1, aligned=True)(x, _dev(rois))
    _check_roi(got, R.roi_align_ref(*sq, np.float32), R.roi_align_ref(*sq, np.float64), "RoIAlign(3)")


def test_roi_align_batch_index_outside_the_input_gives_zeros():
    x = _dev(roi_input("main"))
    rois = _dev(np.array([[2, 1, 1, 9, 9], [-1, 1, 1, 9, 9], [1e9, 1, 1, 9, 9], [float("nan"), 1, 1, 9, 9], [1, 1, 1, 9, 9]], np.float32))
    y = ops.roi_align(x, rois, (2, 2)).cpu()
    assert torch.equal(y[:4], torch.zeros(4, 5, 2, 2)) and bool((y[4] != 0).any())


def test_roi_align_float16_is_the_float32_result_narrowed():
    cfg = ((7, 7), 2, True, 0.25)
    _, _, rois = roi_reference("main", cfg)
    xh, rh = _dev(roi_input("main")).half(), _dev(rois).half()
    got = _roi_align(xh, rh, cfg)
    want = ops.roi_align(xh.float(), rh.float(), cfg[0], cfg[3], cfg[1], cfg[2]).half()
    assert got.dtype == torch.float16 and torch.equal(got, want)
    with pytest.raises(NotImplementedError):
        ops.roi_align(xh.double(), rh.double(), 2)


def test_roi_align_side_stream_registered_operator_and_backward():
    cfg = ((2, 3), -1, False, 1.0)
    f32, f64, rois = roi_reference("main", cfg)
    x, r = _dev(roi_input("main")), _dev(rois)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = ops.roi_align(x, r, cfg[0], cfg[3], cfg[1], cfg[2])
    side.synchronize()
    _check_roi(got, f32, f64, "roi_align on a side stream")
    ops.register_torchvision_op()
    got = torch.ops.torchvision.roi_align(x, r, 1.0, 2, 3, -1, False)
    _check_roi(got, f32, f64, "torch.ops.torchvision.roi_align")
    for call in (lambda t: ops.roi_align(t, r, (2, 3)), lambda t: torch.ops.torchvision.roi_align(t, r, 1.0, 2, 3, -1, False)):
        xg = x.clone().requires_grad_(True)
        y = call(xg)
        assert y.requires_grad
        with pytest.raises(RuntimeError, match="forward-only"):
            y.sum().backward()
