"""ops.box_iou / generalized_box_iou / distance_box_iou, masks_to_boxes, MultiScaleRoIAlign and the thin box functions without a GPU:
the references of tests/_boxes_ref.py against each other, argument checks and dtype gates with their messages, the C ABI's
host-side validation, the torch compositions against hand-computed values, and the pooler's Python (LevelMapper, _infer_scale,
_setup_scales, _filter_input, repr)."""
import numpy as np
import pytest
import torch

from cpu_vision_amd import _lib, ops
from tests import _boxes_ref as B


@pytest.mark.parametrize("mode", B.MODES)
def test_numpy_and_torch_restatements_agree_bit_for_bit(mode):
    for n, m in ((257, 131), (32, 32), (1, 1)):
        b1, b2 = B.pair_case(n, m)
        want = B.pair_reference(mode, n, m)
        got = B.pairwise_np(mode, b1, b2)
        assert want.dtype == np.float32 and want.shape == (n, m)
        assert B.same_values(got, want)
    assert np.isnan(B.pair_reference(mode, 32, 32)).any() and np.isfinite(B.pair_reference(mode, 32, 32)).any()


def test_reference_on_hand_made_boxes():
    b1 = torch.tensor([[0.0, 0.0, 2.0, 2.0], [0.0, 0.0, 1.0, 1.0], [5.0, 5.0, 5.0, 5.0]])
    b2 = torch.tensor([[1.0, 1.0, 3.0, 3.0], [0.0, 0.0, 2.0, 2.0], [4.0, 0.0, 6.0, 2.0], [5.0, 5.0, 5.0, 5.0]])
    iou = B.box_iou(b1, b2)
    assert iou[0, 1] == 1.0 and iou[0, 2] == 0.0 and iou[0, 0] == np.float32(1) / np.float32(7)
    assert torch.isnan(iou[2, 3]) and iou[1, 1] == 0.25
    giou = B.generalized_box_iou(b1, b2)
    assert giou[0, 1] == 1.0 and giou[0, 0] == np.float32(1) / np.float32(7) - np.float32(2) / np.float32(9)
    assert giou[0, 2] == np.float32(0) - np.float32(4) / np.float32(12)  # disjoint: the gap's share of the enclosing box
    diou = B.distance_box_iou(b1, b2)
    want = np.float32(1) / np.float32(7) - np.float32(2) / (np.float32(18) + np.float32(1e-7))
    assert diou[0, 0] == want and diou[0, 1] == 1.0


def test_pairwise_argument_checks(monkeypatch):
    good = torch.zeros(3, 4)
    for fn in (ops.box_iou, ops.generalized_box_iou, ops.distance_box_iou):
        with pytest.raises(RuntimeError, match="boxes1 should be a 2d tensor, got 1D"):
            fn(torch.zeros(12), good)
        with pytest.raises(RuntimeError, match="boxes2 should have 4 elements in dimension 1, got 5"):
            fn(good, torch.zeros(3, 5))
        with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
            fn(good, good)
    monkeypatch.setattr(_lib, "require_device", lambda t, what="input": None)
    for fn in (ops.box_iou, ops.generalized_box_iou, ops.distance_box_iou):
        with pytest.raises(NotImplementedError, match="float16"):
            fn(good.half(), good.half())
        with pytest.raises(NotImplementedError, match="int64"):
            fn(good, good.long())
        with pytest.raises(NotImplementedError, match="float64"):
            fn(good.double(), good)
    with pytest.raises(NotImplementedError, match="eps"):
        ops.distance_box_iou(good, good, eps=1e-6)


def test_masks_to_boxes_checks(monkeypatch):
    empty = ops.masks_to_boxes(torch.zeros((0, 5, 7), dtype=torch.bool))  # as the reference: no device, no launch
    assert empty.shape == (0, 4) and empty.dtype == torch.float32
    assert ops.masks_to_boxes(torch.zeros((3, 0, 7))).shape == (0, 4)
    with pytest.raises(RuntimeError, match="3d tensor"):
        ops.masks_to_boxes(torch.ones(5, 7))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        ops.masks_to_boxes(torch.ones(1, 5, 7))
    monkeypatch.setattr(_lib, "require_device", lambda t, what="input": None)
    for dtype in (torch.float16, torch.int32, torch.float64):
        with pytest.raises(NotImplementedError, match=str(dtype)):
            ops.masks_to_boxes(torch.ones((1, 5, 7), dtype=dtype))


def test_masks_to_boxes_reference_on_a_hand_made_mask():
    m = torch.zeros((2, 4, 6))
    m[0, 1, 2] = m[0, 3, 4] = 1.0
    m[1, 0, 5] = float("nan")
    m[1, 2, 0] = -0.0
    assert B.masks_to_boxes_ref(m).tolist() == [[2.0, 1.0, 4.0, 3.0], [5.0, 0.0, 5.0, 0.0]]
    with pytest.raises(RuntimeError):
        B.masks_to_boxes_ref(torch.zeros((1, 3, 3)))


def test_abi_validates_on_the_host():
    """Every rejection happens before a launch; empty work succeeds without touching a pointer."""
    lib = _lib.load()
    err = lib.mv_last_error
    for mode in (0, 1, 2):
        assert lib.mv_box_iou_f32(None, None, None, 0, 5, mode, None) == 0
        assert lib.mv_box_iou_f32(None, None, None, 5, 0, mode, None) == 0
    assert lib.mv_box_iou_f32(16, 32, 64, -1, 5, 0, None) == -1 and b"bad shape" in err()
    assert lib.mv_box_iou_f32(16, 32, 64, 5, -5, 0, None) == -1 and b"bad shape" in err()
    assert lib.mv_box_iou_f32(16, 32, 64, 5, 5, 3, None) == -1 and b"unknown mode" in err()
    assert lib.mv_box_iou_f32(16, 32, 64, 5, 5, -1, None) == -1 and b"unknown mode" in err()
    assert lib.mv_box_iou_f32(None, 32, 64, 5, 5, 0, None) == -1 and b"null pointer" in err()
    assert lib.mv_box_iou_f32(16, 32, None, 5, 5, 0, None) == -1 and b"null pointer" in err()
    assert lib.mv_box_iou_f32(16, 32, 16, 5, 5, 0, None) == -1 and b"alias" in err()
    assert lib.mv_box_iou_f32(16, 32, 32, 5, 5, 0, None) == -1 and b"alias" in err()
    assert lib.mv_box_iou_f32(16, 32, 64, 1 << 40, 1 << 40, 0, None) == -2 and b"launch grid" in err()
    assert lib.mv_box_iou_f32(16, 32, 64, 1 << 31, 1 << 20, 0, None) == -2 and b"launch grid" in err()

    assert lib.mv_masks_to_boxes_workspace_bytes(0) == 0 and lib.mv_masks_to_boxes_workspace_bytes(-2) == 0
    assert lib.mv_masks_to_boxes_workspace_bytes(5) == 80
    for fn in (lib.mv_masks_to_boxes_u8, lib.mv_masks_to_boxes_f32):
        assert fn(None, None, None, 0, 8, 8, None, 0, None) == 0
        assert fn(16, 32, 64, -1, 8, 8, 256, 1 << 20, None) == -1 and b"bad shape" in err()
        assert fn(16, 32, 64, 2, 8, -8, 256, 1 << 20, None) == -1 and b"bad shape" in err()
        assert fn(None, 32, 64, 2, 8, 8, 256, 1 << 20, None) == -1 and b"null pointer" in err()
        assert fn(16, 32, None, 2, 8, 8, 256, 1 << 20, None) == -1 and b"null pointer" in err()
        assert fn(16, 16, 64, 2, 8, 8, 256, 1 << 20, None) == -1 and b"alias" in err()
        assert fn(16, 32, 66, 2, 8, 8, 256, 1 << 20, None) == -1 and b"4-byte aligned" in err()
        assert fn(16, 32, 64, 2, 8, 8, None, 0, None) == -1 and b"needs a workspace" in err()
        assert fn(16, 32, 64, 2, 8, 8, 256, 31, None) == -1 and b"mv_masks_to_boxes_workspace_bytes" in err()
        assert fn(16, 32, 64, 2, 8, 8, 264, 32, None) == -1 and b"16-byte aligned" in err()
        assert fn(16, 32, 64, 1 << 30, 1 << 20, 8, 256, 1 << 40, None) == -2 and b"launch grid" in err()
        # one workgroup of 256 threads per (mask, 32-row chunk), fewer than 2^32 threads in all: at most 2^24 - 1 workgroups
        assert fn(16, 32, 64, 1, 2 ** 31 - 16, 1, 256, 1 << 20, None) == -2 and b"launch grid" in err()
        assert fn(16, 32, 64, 1, 32 * (2 ** 24 - 1) + 1, 1, 256, 1 << 20, None) == -2 and b"launch grid" in err()
        assert fn(16, 32, 64, 1 << 24, 32, 8, 256, 1 << 40, None) == -2 and b"launch grid" in err()

    I, D = _lib.C.c_int, _lib.C.c_double
    xs = (_lib.C.c_void_p * 2)(1024, 2048)
    hs, ws, sc = (I * 2)(8, 4), (I * 2)(8, 4), (D * 2)(0.25, 0.125)
    f = lib.mv_multiscale_roi_align_f32
    assert f(None, None, None, None, 2, None, None, None, 2, 3, 0, 7, 7, 2, 0, None) == 0
    assert f(None, None, None, None, 2, None, None, None, 2, 3, 5, 7, 0, 2, 0, None) == 0
    assert f(xs, hs, ws, sc, 2, 16, 32, 64, 2, 3, -1, 7, 7, 2, 0, None) == -1 and b"bad shape" in err()
    assert f(xs, hs, ws, sc, -1, 16, 32, 64, 2, 3, 1, 7, 7, 2, 0, None) == -1 and b"bad shape" in err()
    assert f(xs, hs, ws, sc, 9, 16, 32, 64, 2, 3, 1, 7, 7, 2, 0, None) == -2 and b"feature maps per call" in err()
    assert f(None, hs, ws, sc, 2, 16, 32, 64, 2, 3, 1, 7, 7, 2, 0, None) == -1 and b"null level table" in err()
    assert f(xs, (I * 2)(8, 0), ws, sc, 2, 16, 32, 64, 2, 3, 1, 7, 7, 2, 0, None) == -1 and b"empty" in err()
    assert f(xs, (I * 2)(8, -4), ws, sc, 2, 16, 32, 64, 2, 3, 1, 7, 7, 2, 0, None) == -1 and b"bad shape" in err()
    assert f(xs, (I * 2)(8, 65536), (I * 2)(8, 65536), sc, 2, 16, 32, 64, 2, 3, 1, 7, 7, 2, 0, None) == -2 and b"plane index" in err()
    assert f(xs, hs, ws, sc, 2, 16, 32, 64, 2, 1 << 20, 1 << 40, 7, 7, 2, 0, None) == -2 and b"launch grid" in err()
    assert f(xs, hs, ws, sc, 2, 16, None, 64, 2, 3, 1, 7, 7, 2, 0, None) == -1 and b"null pointer" in err()
    assert f(xs, hs, ws, sc, 2, 16, 32, None, 2, 3, 1, 7, 7, 2, 0, None) == -1 and b"null pointer" in err()
    assert f((_lib.C.c_void_p * 2)(1024, None), hs, ws, sc, 2, 16, 32, 64, 2, 3, 1, 7, 7, 2, 0, None) == -1 and b"feature map 1" in err()
    assert f(xs, hs, ws, sc, 2, 16, 32, 16, 2, 3, 1, 7, 7, 2, 0, None) == -1 and b"alias" in err()
    assert f(xs, hs, ws, sc, 2, 16, 32, 2048, 2, 3, 1, 7, 7, 2, 0, None) == -1 and b"alias" in err()
    assert f(xs, hs, ws, sc, 2, 16, 36, 64, 2, 3, 1, 7, 7, 2, 0, None) == -1 and b"8-byte aligned" in err()


# ---- the thin compositions against hand-computed values ----------------------------------------------------------------------------
def test_box_area():
    b = torch.tensor([[0.0, 0.0, 2.0, 3.0], [1.0, 1.0, 1.0, 5.0], [4.0, 4.0, 2.0, 5.0]])
    assert ops.box_area(b).tolist() == [6.0, 0.0, -2.0]
    assert ops.box_area(b.half()).dtype == torch.float32  # _upcast
    assert ops.box_area(torch.tensor([[0, 0, 200, 200]], dtype=torch.uint8)).tolist() == [40000]
    b.requires_grad_(True)
    ops.box_area(b).sum().backward()  # a torch composition: it stays differentiable
    assert b.grad is not None


def test_box_convert():
    xyxy = torch.tensor([[1.0, 2.0, 4.0, 8.0], [0.0, 0.0, 3.0, 1.0]])
    xywh = torch.tensor([[1.0, 2.0, 3.0, 6.0], [0.0, 0.0, 3.0, 1.0]])
    cxcywh = torch.tensor([[2.5, 5.0, 3.0, 6.0], [1.5, 0.5, 3.0, 1.0]])
    assert torch.equal(ops.box_convert(xyxy, "xyxy", "xywh"), xywh)
    assert torch.equal(ops.box_convert(xyxy, "xyxy", "cxcywh"), cxcywh)
    assert torch.equal(ops.box_convert(xywh, "xywh", "xyxy"), xyxy)
    assert torch.equal(ops.box_convert(cxcywh, "cxcywh", "xyxy"), xyxy)
    assert torch.equal(ops.box_convert(xywh, "xywh", "cxcywh"), cxcywh)  # through xyxy
    assert torch.equal(ops.box_convert(ops.box_convert(xywh, "xywh", "cxcywh"), "cxcywh", "xywh"), xywh)  # and back
    same = ops.box_convert(xyxy, "xyxy", "xyxy")
    assert torch.equal(same, xyxy) and same.data_ptr() != xyxy.data_ptr()  # clone()
    for bad in (("xyxy", "xxyy"), ("cxcywhr", "xyxy"), ("XYXY", "xywh")):
        with pytest.raises(ValueError, match="Unsupported Bounding Box Conversions for given in_fmt and out_fmt"):
            ops.box_convert(xyxy, *bad)
    assert ops.box_convert(torch.zeros(2, 3, 4), "xyxy", "cxcywh").shape == (2, 3, 4)


def test_clip_boxes_to_image():
    b = torch.tensor([[-1.0, -2.0, 30.0, 40.0], [5.0, 6.0, 7.0, 8.0], [25.0, 12.0, 19.5, 9.5]])
    got = ops.clip_boxes_to_image(b, (10, 20))  # (height, width): x to [0, 20], y to [0, 10]
    assert got.tolist() == [[0.0, 0.0, 20.0, 10.0], [5.0, 6.0, 7.0, 8.0], [20.0, 10.0, 19.5, 9.5]]
    batched = ops.clip_boxes_to_image(b.reshape(1, 3, 4).repeat(2, 1, 1), (10, 20))
    assert batched.shape == (2, 3, 4) and torch.equal(batched[1], got)


def test_remove_small_boxes():
    b = torch.tensor([[0.0, 0.0, 2.0, 2.0], [0.0, 0.0, 1.5, 3.0], [1.0, 1.0, 3.0, 3.5], [0.0, 0.0, 2.0, 1.99], [3.0, 3.0, 9.0, 9.0]])
    keep = ops.remove_small_boxes(b, 2.0)  # a side exactly min_size stays
    assert keep.dtype == torch.int64 and keep.tolist() == [0, 2, 4]
    assert ops.remove_small_boxes(b, 10.0).tolist() == []


# ---- ops/poolers.py ------------------------------------------------------------------------------------------------------------------
def test_level_mapper_on_canonical_sizes_where_eps_decides():
    mapper = ops.initLevelMapper(2, 5)
    assert isinstance(mapper, ops.LevelMapper) and (mapper.s0, mapper.lvl0, mapper.eps) == (224, 4, 1e-6)
    sides = [224.0 * 2.0 ** j for j in (-3, -2, -1, 0, 1, 2)]
    boxes = torch.tensor([[10.0, 20.0, 10.0 + s, 20.0 + s] for s in sides])
    levels = mapper([boxes[:2], boxes[2:]])
    assert levels.dtype == torch.int64
    assert levels.tolist() == [0, 0, 1, 2, 3, 3]  # lvl0 + j, clamped to [2, 5], minus k_min
    just_below = torch.tensor([[0.0, 0.0, 223.9, 223.9], [0.0, 0.0, 447.0, 447.0], [0.0, 0.0, 1.0, 1.0]])
    assert mapper([just_below]).tolist() == [1, 2, 0]
    other = ops.LevelMapper(2, 5, canonical_scale=32, canonical_level=4)
    assert other([torch.tensor([[0.0, 0.0, 32.0, 32.0], [0.0, 0.0, 20.0, 20.0], [0.0, 0.0, 100.0, 50.0]])]).tolist() == [2, 1, 3]


def test_levels_of_the_gpu_cases_cover_what_they_claim():
    mapper = ops.LevelMapper(2, 5, canonical_scale=B.CANONICAL_SCALE, canonical_level=B.CANONICAL_LEVEL)
    all_four = mapper([torch.from_numpy(b.copy()) for b in B.fpn_boxes()])
    assert sorted(set(all_four.tolist())) == [0, 1, 2, 3] and len(all_four) == 24
    without = mapper([torch.from_numpy(b.copy()) for b in B.fpn_boxes(skip_level=3)])
    assert sorted(set(without.tolist())) == [0, 2, 3]


def test_infer_scale_and_setup_scales():
    assert ops._infer_scale(torch.zeros(1, 1, 32, 40), [128, 160]) == 0.25
    # ceil-divided FPN maps of a 127 x 159 image: 32/127, 16/127, 8/127, 4/127 are no powers of two
    for size, want in ((32, 0.25), (16, 0.125), (8, 0.0625), (4, 0.03125)):
        assert ops._infer_scale(torch.zeros(1, 1, size, size + 8), [127, 159]) == want
    assert ops._infer_scale(torch.zeros(1, 1, 50, 7), [200, 999]) == 0.25  # the first axis decides
    feats = [torch.zeros(s) for s in B.FPN_SHAPES]
    scales, mapper = ops._setup_scales(feats, [(100, 160), (128, 90)], 56, 3)  # the maxima per axis: (128, 160)
    assert scales == [0.25, 0.125, 0.0625, 0.03125]
    assert (mapper.k_min, mapper.k_max, mapper.s0, mapper.lvl0) == (2, 5, 56, 3)
    with pytest.raises(ValueError, match="images list should not be empty"):
        ops._setup_scales(feats, [], 224, 4)


def test_filter_input_and_module_state_and_repr():
    x = {"a": torch.zeros(1), "b": torch.ones(1), "pool": torch.zeros(2), "c": torch.full((1,), 2.0)}
    assert [float(t.sum()) for t in ops._filter_input(x, ["c", "a"])] == [0.0, 2.0]  # the dict's order, not the list's
    m = ops.MultiScaleRoIAlign(["feat1", "feat3"], 3, 2)
    assert repr(m) == "MultiScaleRoIAlign(featmap_names=['feat1', 'feat3'], output_size=(3, 3), sampling_ratio=2)"
    assert m.scales is None and m.map_levels is None and (m.canonical_scale, m.canonical_level) == (224, 4)
    m = ops.MultiScaleRoIAlign(["0"], (7, 5), 0, canonical_scale=56, canonical_level=3)
    assert m.output_size == (7, 5) and (m.canonical_scale, m.canonical_level) == (56, 3)
    with pytest.raises(TypeError):
        ops.MultiScaleRoIAlign(["0"], 7, 2, 224)  # keyword-only, as in the reference
    with pytest.raises(ValueError, match="scales and mapper should not be None"):
        ops._multiscale_roi_align([torch.zeros(1, 1, 2, 2)], [torch.zeros(1, 4)], (2, 2), 2, None, None)


def test_multiscale_argument_checks(monkeypatch):
    feats = [torch.zeros(s) for s in B.FPN_SHAPES]
    rois, levels = torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64)
    scales = [0.25, 0.125, 0.0625, 0.03125]
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        ops._multiscale_roi_align_impl(feats, rois, levels, scales, 7, 7, 2)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        ops.MultiScaleRoIAlign(["0", "1"], 7, 2)({"0": feats[0], "1": feats[1]}, [torch.zeros(2, 4)], [B.IMAGE])
    monkeypatch.setattr(_lib, "require_device", lambda t, what="input": None)
    with pytest.raises(RuntimeError, match="4 feature maps for 3 scales"):
        ops._multiscale_roi_align_impl(feats, rois, levels, scales[:3], 7, 7, 2)
    with pytest.raises(_lib.Mi355VisionError, match="up to 8 feature maps"):
        ops._multiscale_roi_align_impl(feats[:1] * 9, rois, levels, [0.25] * 9, 7, 7, 2)
    with pytest.raises(RuntimeError, match="must agree in batch size, channels and dtype"):
        ops._multiscale_roi_align_impl(feats[:1] + [torch.zeros(2, 4, 16, 20)], rois, levels, scales[:2], 7, 7, 2)
    with pytest.raises(RuntimeError, match=r"rois must have shape as Tensor\[K, 5\]"):
        ops._multiscale_roi_align_impl(feats, torch.zeros(3, 4), levels, scales, 7, 7, 2)
    with pytest.raises(RuntimeError, match="levels must be a tensor of 3 integers"):
        ops._multiscale_roi_align_impl(feats, rois, levels[:2], scales, 7, 7, 2)
    with pytest.raises(RuntimeError, match="levels must be a tensor of 3 integers"):
        ops._multiscale_roi_align_impl(feats, rois, levels.float(), scales, 7, 7, 2)
    with pytest.raises(RuntimeError, match="to have the same type"):
        ops._multiscale_roi_align_impl(feats, rois.half(), levels, scales, 7, 7, 2)
    with pytest.raises(NotImplementedError, match="float64"):
        ops._multiscale_roi_align_impl([f.double() for f in feats], rois.double(), levels, scales, 7, 7, 2)
    with pytest.raises(RuntimeError, match="must not be negative"):
        ops._multiscale_roi_align_impl(feats, rois, levels, scales, -1, 7, 2)


def test_multiscale_reference_scatters_by_level():
    feats = B.fpn_features()
    rois = np.array([[0, 4, 4, 40, 36], [1, 10, 8, 100, 90], [0, 2, 2, 12, 14]], dtype=np.float32)
    levels = np.array([1, 3, 0])
    scales = [0.25, 0.125, 0.0625, 0.03125]
    got = B.multiscale_ref(feats, rois, levels, scales, (2, 3), 2)
    for i, lv in enumerate(levels):
        want = B.R.roi_align_ref(feats[lv], rois[i:i + 1], (2, 3), scales[lv], 2, False)
        assert np.array_equal(got[i:i + 1], want)
    assert B.kernel_constant("kMaxRoiLevels", "mv_common.h") == ops.MAX_ROI_LEVELS
