"""ops.nms / batched_nms / roi_align without a GPU: argument checks and their messages, the C ABI's host-side validation, the
box-list conversion, and the references of tests/_detect_ref.py themselves (the float32 restatement against its float64 form on
the shapes tests/test_gpu_detect.py runs; the tie-margin generator)."""
import numpy as np
import pytest
import torch

from cpu_vision_amd import _lib, ops
from tests import _detect_ref as R
from tests._detect_cases import NMS_KINDS, NMS_SIZES, NMS_THRESHOLDS, ROI_CONFIGS, roi_reference


def test_nms_checks_ranks_before_anything_else():
    b, s = torch.zeros(3, 4), torch.zeros(3)
    with pytest.raises(RuntimeError, match="boxes should be a 2d tensor, got 1D"):
        ops.nms(torch.zeros(12), s, 0.5)
    with pytest.raises(RuntimeError, match="boxes should have 4 elements in dimension 1, got 5"):
        ops.nms(torch.zeros(3, 5), s, 0.5)
    with pytest.raises(RuntimeError, match="scores should be a 1d tensor, got 2D"):
        ops.nms(b, torch.zeros(3, 1), 0.5)
    with pytest.raises(RuntimeError, match="boxes and scores should have same number of elements in dimension 0, got 3 and 2"):
        ops.nms(b, torch.zeros(2), 0.5)


def test_cpu_tensors_raise():
    b, s = torch.zeros(3, 4), torch.zeros(3)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        ops.nms(b, s, 0.5)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        ops.batched_nms(b, s, torch.zeros(3, dtype=torch.int64), 0.5)
    x = torch.zeros(1, 2, 4, 4)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        ops.roi_align(x, torch.zeros(1, 5), 2)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        ops.roi_align(x, [torch.zeros(1, 4)], (2, 3))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        ops.RoIAlign(2, 1.0, -1)(x, torch.zeros(1, 5))


def test_roi_align_checks_boxes_and_input():
    x = torch.zeros(1, 2, 4, 4)
    with pytest.raises(AssertionError, match=r"The boxes tensor shape is not correct as Tensor\[K, 5\]"):
        ops.roi_align(x, torch.zeros(3, 4), 2)
    with pytest.raises(AssertionError, match=r"The shape of the tensor in the boxes list is not correct as List\[Tensor\[L, 4\]\]"):
        ops.roi_align(x, [torch.zeros(3, 4), torch.zeros(2, 5)], 2)
    with pytest.raises(AssertionError, match=r"boxes is expected to be a Tensor\[L, 5\] or a List\[Tensor\[K, 4\]\]"):
        ops.roi_align(x, 7, 2)
    with pytest.raises(RuntimeError, match="4-D input"):
        ops.roi_align(torch.zeros(2, 4, 4), torch.zeros(1, 5), 2)
    with pytest.raises(RuntimeError, match=r"rois must have shape as Tensor\[K, 5\]"):
        ops._roi_align_impl(x, torch.zeros(1, 4), 1.0, 2, 2, -1, False)


def test_roi_align_output_size_int_and_pair_list_and_tensor(monkeypatch):
    """What reaches the operator: an int becomes a pair, a list of boxes the (K, 5) tensor."""
    seen = []

    def fake(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, aligned):
        seen.append((tuple(rois.shape), spatial_scale, pooled_height, pooled_width, sampling_ratio, aligned))
        return torch.zeros(rois.shape[0], input.shape[1], pooled_height, pooled_width)

    monkeypatch.setattr(ops, "_roi_align_impl", fake)
    x = torch.zeros(2, 3, 8, 8)
    assert ops.roi_align(x, torch.zeros(4, 5), 3).shape == (4, 3, 3, 3)
    assert ops.roi_align(x, [torch.zeros(1, 4), torch.zeros(2, 4)], (2, 5), 0.25, 2, True).shape == (3, 3, 2, 5)
    assert ops.RoIAlign((7, 6), 0.5, 1)(x, torch.zeros(1, 5)).shape == (1, 3, 7, 6)
    assert seen == [((4, 5), 1.0, 3, 3, -1, False), ((3, 5), 0.25, 2, 5, 2, True), ((1, 5), 0.5, 7, 6, 1, False)]
    assert repr(ops.RoIAlign(7, 0.25, 2, True)) == "RoIAlign(output_size=7, spatial_scale=0.25, sampling_ratio=2, aligned=True)"


def test_dtype_gates(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda t, what="input": None)
    with pytest.raises(NotImplementedError, match="float32"):
        ops.nms(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), 0.5)
    with pytest.raises(NotImplementedError, match="float64"):
        ops.roi_align(torch.zeros(1, 1, 2, 2, dtype=torch.float64), torch.zeros(1, 5, dtype=torch.float64), 1)
    with pytest.raises(RuntimeError, match="to have the same type"):
        ops.roi_align(torch.zeros(1, 1, 2, 2), torch.zeros(1, 5, dtype=torch.float16), 1)


def test_convert_boxes_to_roi_format_against_a_restatement():
    g = torch.Generator().manual_seed(0)
    boxes = [torch.rand((n, 4), generator=g) for n in (3, 0, 1, 5)]
    got = ops.convert_boxes_to_roi_format(boxes)
    want = R.convert_boxes_to_roi_format_ref([b.numpy() for b in boxes])
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    one = ops.convert_boxes_to_roi_format(boxes[:1])
    assert np.array_equal(one.numpy(), R.convert_boxes_to_roi_format_ref([boxes[0].numpy()]))


def test_abi_validates_on_the_host():
    """Every rejection happens before a launch; n == 0 / k == 0 succeed without one."""
    lib = _lib.load()
    assert lib.mv_nms_workspace_bytes(0) == 0 and lib.mv_nms_workspace_bytes(-3) == 0
    assert lib.mv_nms_workspace_bytes(65) == (16 * 65 + 8 * 65 * 2 + 4 * 65 + 15) // 16 * 16
    assert lib.mv_nms_workspace_bytes(64 * 4096 + 1) == 0
    assert lib.mv_nms_f32(None, None, 0, 0.5, None, None, None, 0, None) == 0
    assert lib.mv_nms_f32(16, 32, -1, 0.5, 64, 128, 256, 1 << 20, None) == -1 and b"bad box count" in lib.mv_last_error()
    assert lib.mv_nms_f32(16, 32, 10, 0.5, None, 128, 256, 1 << 20, None) == -1 and b"null pointer" in lib.mv_last_error()
    assert lib.mv_nms_f32(16, 32, 10, 0.5, 64, 128, None, 0, None) == -1 and b"needs a workspace" in lib.mv_last_error()
    need = lib.mv_nms_workspace_bytes(10)
    assert lib.mv_nms_f32(16, 32, 10, 0.5, 64, 128, 256, need - 1, None) == -1 and b"mv_nms_workspace_bytes" in lib.mv_last_error()
    assert lib.mv_nms_f32(16, 32, 10, 0.5, 64, 128, 264, need, None) == -1 and b"16-byte aligned" in lib.mv_last_error()
    assert lib.mv_nms_f32(16, 32, 10, 0.5, 68, 128, 256, need, None) == -1 and b"8-byte aligned" in lib.mv_last_error()
    assert lib.mv_nms_f32(16, 32, 64 * 4096 + 1, 0.5, 64, 128, 256, 1 << 40, None) == -2 and b"boxes per call" in lib.mv_last_error()

    assert lib.mv_roi_align_f32(None, None, None, 2, 3, 8, 8, 0, 7, 7, 1.0, -1, 0, None) == 0
    assert lib.mv_roi_align_f32(None, None, None, 2, 3, 8, 8, 5, 0, 7, 1.0, -1, 0, None) == 0
    assert lib.mv_roi_align_f32(16, 32, 64, 2, 3, 8, 8, -1, 7, 7, 1.0, -1, 0, None) == -1 and b"bad shape" in lib.mv_last_error()
    assert lib.mv_roi_align_f32(16, 32, 64, 2, 3, 8, -8, 1, 7, 7, 1.0, -1, 0, None) == -1 and b"bad shape" in lib.mv_last_error()
    assert lib.mv_roi_align_f32(16, 32, 64, 2, 3, 0, 8, 1, 7, 7, 1.0, -1, 0, None) == -1 and b"empty" in lib.mv_last_error()
    assert lib.mv_roi_align_f32(16, 32, None, 2, 3, 8, 8, 1, 7, 7, 1.0, -1, 0, None) == -1 and b"null pointer" in lib.mv_last_error()
    assert lib.mv_roi_align_f32(16, 32, 16, 2, 3, 8, 8, 1, 7, 7, 1.0, -1, 0, None) == -1 and b"alias" in lib.mv_last_error()
    assert lib.mv_roi_align_f32(16, 32, 64, 2, 3, 65536, 65536, 1, 7, 7, 1.0, -1, 0, None) == -2 and b"plane index" in lib.mv_last_error()
    assert lib.mv_roi_align_f32(16, 32, 64, 2, 1 << 20, 8, 8, 1 << 40, 7, 7, 1.0, -1, 0, None) == -2 and b"launch grid" in lib.mv_last_error()


def test_nms_reference_on_hand_made_boxes():
    boxes = np.array([[0, 0, 10, 10], [1, 1, 11, 11], [20, 20, 30, 30], [0, 0, 10, 10], [5, 5, 5, 9]], dtype=np.float32)
    scores = np.array([0.5, 0.9, 0.5, 0.9, 0.1], dtype=np.float32)
    # order: 1, 3 (equal scores, index order), 0, 2, 4; IoU(1, 3) = 81 / 119 = 0.68, IoU(3, 0) = 1
    assert R.nms_ref(boxes, scores, 0.5).tolist() == [1, 2, 4]
    assert R.nms_ref(boxes, scores, 0.7).tolist() == [1, 3, 2, 4]
    assert R.nms_ref(boxes, scores, 1.0).tolist() == [1, 3, 0, 2, 4]
    assert R.nms_ref(boxes, scores, 0.0).tolist() == [1, 2, 4]
    assert R.nms_ref(boxes[:0], scores[:0], 0.5).tolist() == []


@pytest.mark.parametrize("kind", NMS_KINDS)
def test_tie_margin_generator_terminates_within_a_few_seeds(kind):
    for n in NMS_SIZES:
        if n == 0:
            continue
        boxes, scores, seed = R.boxes_with_margin(kind, n, NMS_THRESHOLDS, seed=n, max_seeds=5)
        assert boxes.shape == (n, 4) and scores.shape == (n,) and boxes.dtype == np.float32 and seed < n + 5


def test_tie_margin_flags_a_pair_at_the_threshold():
    boxes = np.array([[0, 0, 2, 1], [1, 0, 3, 1]], dtype=np.float32)  # IoU 1 / 3
    assert not R.tie_margin_ok(boxes, 1 / 3) and R.tie_margin_ok(boxes, 0.5) and R.tie_margin_ok(boxes, 0.0)


@pytest.mark.parametrize("cfg", ROI_CONFIGS, ids=str)
def test_float32_and_float64_references_agree(cfg):
    for shape in ("main", "tiny"):
        f32, f64, _ = roi_reference(shape, cfg)
        assert f32.dtype == np.float32 and f64.dtype == np.float64 and f32.shape == f64.shape
        assert np.abs(f32.astype(np.float64) - f64).max() <= 1e-5
