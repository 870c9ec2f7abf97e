"""ops.box_iou / generalized_box_iou / distance_box_iou, ops.masks_to_boxes and ops.MultiScaleRoIAlign on the GPU (`-m gpu`) against
the references of tests/_boxes_ref.py: the reference's expressions evaluated by torch on the CPU (equal as values: NaN in the same
places, == elsewhere), the reference's masks_to_boxes loop, and for the pooler both the per-level composition with ops.roi_align on
the GPU (bit for bit) and the numpy restatement roi_align_ref scattered by the CPU's levels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, ops  # noqa: E402
from tests import _boxes_ref as B  # noqa: E402

DEV = "cuda"
STRIP, COLS, WAVE_ROWS = B.kernel_constant("kIouStrip"), B.kernel_constant("kIouCols"), B.kernel_constant("kIouWaveRows")
CHUNK_ROWS = B.kernel_constant("kMtbChunkRows")
# (N, M): the listed shapes, then the row strip, the wave's row group and the column tile at constant - 1, constant, constant + 1
PAIR_SHAPES = [(1, 1), (3, 5), (64, 64), (65, 257), (257, 3), (5, 1024), (0, 5), (5, 0),
               (STRIP - 1, COLS - 1), (STRIP, COLS), (STRIP + 1, COLS + 1), (WAVE_ROWS + 1, COLS + 4), (WAVE_ROWS - 1, 2 * COLS + 4)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=str)
@pytest.mark.parametrize("mode", B.MODES)
def test_pairwise_equals_the_cpu_expression(mode, shape):
    n, m = shape
    b1, b2 = B.pair_case(n, m)
    d1, d2 = torch.from_numpy(b1.copy()).to(DEV), torch.from_numpy(b2.copy()).to(DEV)
    got = getattr(ops, mode)(d1, d2)
    assert got.shape == (n, m) and got.dtype == torch.float32 and got.device.type == "cuda"
    if n and m:
        assert _lib.last_kernel() == "k_box_iou<%s,%s>" % ({"box_iou": "iou", "generalized_box_iou": "giou", "distance_box_iou": "diou"}[mode],
                                                          "vec16" if m % 4 == 0 else "scalar")
    want = B.pair_reference(mode, n, m)
    assert B.same_values(got.cpu().numpy(), want), f"{mode} {shape}: differs from the CPU expression [{_lib.last_kernel()}]"
    assert np.array_equal(_bits(d1).numpy(), b1.view(np.int32)) and np.array_equal(_bits(d2).numpy(), b2.view(np.int32)), "inputs changed"


def test_pairwise_special_boxes_are_in_the_cases():
    """What the cases hold (tests/_boxes_ref.SPECIALS), on the CPU reference the GPU is compared with: identical boxes give exactly 1,
    touching and disjoint boxes 0, two zero-area boxes NaN, NaN and inf coordinates NaN / a finite value."""
    ref = B.pair_reference("box_iou", 64, 64)
    assert ref[7, 7] == 1.0 and ref[7, 23] == 1.0           # identical
    assert ref[7, 9] == 0.0 and ref[7, 11] == 0.0           # touching, disjoint
    assert np.isnan(ref[3, 3]) and np.isnan(ref[13, 0])     # 0 / 0; a NaN coordinate
    assert ref[5, 7] == 0.0                                 # negative size against a box that covers it
    assert np.isfinite(ref[15, 0]) or np.isnan(ref[15, 0])  # an infinite coordinate: whatever IEEE gives, the GPU must give it too
    gen = B.pair_reference("generalized_box_iou", 64, 64)
    assert gen[7, 7] == 1.0 and gen[7, 11] < 0 and np.isnan(gen[15, 15])  # inf - inf in the enclosing box
    dist = B.pair_reference("distance_box_iou", 64, 64)
    assert dist[7, 7] == 1.0 and dist[7, 11] < 0
    b1, b2 = B.pair_case(64, 64)
    got = ops.box_iou(torch.from_numpy(b1.copy()).to(DEV), torch.from_numpy(b2.copy()).to(DEV)).cpu().numpy()
    assert got[7, 7] == 1.0 and np.isnan(got[3, 3]) and got[7, 9] == 0.0


def test_pairwise_views_dtype_gates_and_backward():
    b1, b2 = B.pair_case(65, 257)
    wide = torch.zeros((65, 6), device=DEV)
    wide[:, 1:5] = torch.from_numpy(b1.copy()).to(DEV)
    d2 = torch.from_numpy(b2.copy()).to(DEV)
    got = ops.generalized_box_iou(wide[:, 1:5], d2)  # a non-contiguous view
    assert B.same_values(got.cpu().numpy(), B.pair_reference("generalized_box_iou", 65, 257))
    for fn in (ops.box_iou, ops.generalized_box_iou, ops.distance_box_iou):
        with pytest.raises(NotImplementedError, match="float16"):
            fn(d2.half(), d2.half())
        with pytest.raises(NotImplementedError, match="int32"):
            fn(d2.int(), d2)
        g = d2.clone().requires_grad_(True)
        out = fn(g, d2)
        assert out.requires_grad
        with pytest.raises(RuntimeError, match="forward-only"):
            out.nan_to_num().sum().backward()
        with torch.no_grad():
            assert not fn(g, d2).requires_grad


# ---- masks_to_boxes ------------------------------------------------------------------------------------------------------------------
MASK_SHAPES = [(1, 1, 1), (3, 5, 7), (4, 37, 131), (2, 64, 256), (3, 2 * CHUNK_ROWS + 3, 50), (2, CHUNK_ROWS + 1, 16)]


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.float32], ids=str)
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=str)
def test_masks_to_boxes_equals_the_reference_loop(shape, dtype):
    for seed in range(4):  # the single pixel of mask 0 in each corner
        cpu = torch.from_numpy(B.mask_case(*shape, seed=seed)).to(dtype)
        dev = cpu.to(DEV)
        before = dev.clone()
        got = ops.masks_to_boxes(dev)
        assert got.dtype == torch.float32 and got.shape == (shape[0], 4)
        assert torch.equal(got.cpu(), B.masks_to_boxes_ref(cpu)), f"{shape} {dtype} seed {seed} [{_lib.last_kernel()}]"
        assert torch.equal(dev, before)
    assert ("f32" if dtype == torch.float32 else "u8") in _lib.last_kernel()


def test_masks_to_boxes_float_nan_is_set_and_negative_zero_is_clear():
    m = torch.zeros((2, 9, 21))
    m[0, 4, 5] = float("nan")
    m[0, 2, 17] = -0.0
    m[0, 7, 1] = -0.0
    m[1, 8, 20] = -3.5
    m[1, 0, 0] = 1e-45  # a denormal is not zero
    m[1, 5, 5] = float("inf")
    want = B.masks_to_boxes_ref(m)
    assert want.tolist() == [[5.0, 4.0, 5.0, 4.0], [0.0, 0.0, 20.0, 8.0]]
    assert torch.equal(ops.masks_to_boxes(m.to(DEV)).cpu(), want)


def test_masks_to_boxes_views_empty_batch_and_an_empty_mask():
    big = torch.zeros((4, 37, 131), dtype=torch.uint8, device=DEV)
    big[:, 3:30, 5:120] = torch.from_numpy(B.mask_case(4, 27, 115)).to(DEV)
    view = big[:, 3:30, 5:120]  # not contiguous
    assert torch.equal(ops.masks_to_boxes(view).cpu(), B.masks_to_boxes_ref(view.cpu()))
    assert ops.masks_to_boxes(torch.zeros((0, 5, 7), dtype=torch.bool, device=DEV)).shape == (0, 4)
    assert ops.masks_to_boxes(torch.zeros((0, 5, 7), dtype=torch.bool, device=DEV)).device.type == "cuda"
    for dtype in (torch.bool, torch.uint8, torch.float32):
        batch = torch.from_numpy(B.mask_case(3, 40, 33)).to(dtype).to(DEV)
        batch[2] = 0
        with pytest.raises(RuntimeError, match="no non-zero element"):
            ops.masks_to_boxes(batch)
    with pytest.raises(NotImplementedError, match="int64"):
        ops.masks_to_boxes(torch.ones((1, 3, 3), dtype=torch.int64, device=DEV))


# ---- MultiScaleRoIAlign --------------------------------------------------------------------------------------------------------------
SCALES = [0.25, 0.125, 0.0625, 0.03125]
NAMES = ["p2", "p3", "p4", "p5"]


def _features(dtype=torch.float32):
    return [torch.from_numpy(f.copy()).to(DEV, dtype) for f in B.fpn_features()]


def _cpu_levels(boxes):
    mapper = ops.LevelMapper(2, 5, canonical_scale=B.CANONICAL_SCALE, canonical_level=B.CANONICAL_LEVEL)
    return mapper([torch.from_numpy(b.copy()) for b in boxes])


def _per_level_on_the_gpu(feats, rois, levels, output_size, sampling_ratio):
    """The reference's loop with ops.roi_align: what the fused launch must equal bit for bit."""
    result = torch.zeros((len(rois), feats[0].shape[1]) + tuple(output_size), dtype=feats[0].dtype, device=DEV)
    for level, (f, scale) in enumerate(zip(feats, SCALES)):
        idx = torch.where(levels == level)[0]
        result[idx] = ops.roi_align(f, rois[idx], output_size, scale, sampling_ratio)
    return result


@pytest.mark.parametrize("skip_level", [None, 3], ids=["all-levels", "empty-level"])
@pytest.mark.parametrize("sampling_ratio", [2, 0])
@pytest.mark.parametrize("output_size", [7, (2, 3)], ids=str)
def test_multiscale_equals_the_per_level_loop(output_size, sampling_ratio, skip_level):
    boxes = B.fpn_boxes(skip_level=skip_level)
    cpu_levels = _cpu_levels(boxes)
    assert sorted(set(cpu_levels.tolist())) == ([0, 1, 2, 3] if skip_level is None else [0, 2, 3])
    dev_boxes = [torch.from_numpy(b.copy()).to(DEV) for b in boxes]
    mapper = ops.LevelMapper(2, 5, canonical_scale=B.CANONICAL_SCALE, canonical_level=B.CANONICAL_LEVEL)
    dev_levels = mapper(dev_boxes)
    assert dev_levels.device.type == "cuda" and torch.equal(dev_levels.cpu(), cpu_levels)  # no roi is near a level boundary
    feats = _features()
    size = (output_size, output_size) if isinstance(output_size, int) else output_size
    rois = ops._convert_to_roi_format(dev_boxes)
    want_gpu = _per_level_on_the_gpu(feats, rois, dev_levels, size, sampling_ratio)
    want_np = B.multiscale_ref(B.fpn_features(), rois.cpu().numpy(), cpu_levels.numpy(), SCALES, size, sampling_ratio)
    explicit = ops._multiscale_roi_align_impl(feats, rois, dev_levels, SCALES, size[0], size[1], sampling_ratio)
    assert _lib.last_kernel().startswith("k_multiscale_roi_align<levels4,legacy,")
    module = ops.MultiScaleRoIAlign(NAMES, output_size, sampling_ratio, canonical_scale=B.CANONICAL_SCALE, canonical_level=B.CANONICAL_LEVEL)
    x = dict(zip(NAMES, feats))
    x["pool"] = torch.zeros((2, 3, 2, 3), device=DEV)  # not in featmap_names
    end_to_end = module(x, dev_boxes, [B.IMAGE, (100, 150)])
    assert module.scales == SCALES and (module.map_levels.k_min, module.map_levels.k_max) == (2, 5)
    for name, got in (("explicit levels", explicit), ("module", end_to_end)):
        assert got.shape == (len(rois), 3) + size and got.dtype == torch.float32
        assert torch.equal(_bits(got), _bits(want_gpu)), f"{name}: differs from the per-level ops.roi_align"
        assert np.array_equal(got.cpu().numpy(), want_np), f"{name}: differs from roi_align_ref scattered by level"


def test_multiscale_level_outside_the_maps_gives_zeros():
    boxes = B.fpn_boxes()
    dev_boxes = [torch.from_numpy(b.copy()).to(DEV) for b in boxes]
    rois = ops._convert_to_roi_format(dev_boxes)
    levels = _cpu_levels(boxes).to(DEV)
    levels[0], levels[5], levels[7] = -1, 4, 1 << 40
    got = ops._multiscale_roi_align_impl(_features(), rois, levels, SCALES, 7, 7, 2)
    inside = (levels >= 0) & (levels < 4)
    want = _per_level_on_the_gpu(_features(), rois, levels, (7, 7), 2)
    assert not bool(got[~inside].any()) and torch.equal(_bits(got), _bits(want)) and bool(got[inside].any())


def test_multiscale_no_rois_single_map_float16_and_backward():
    feats = _features()
    module = ops.MultiScaleRoIAlign(NAMES, 7, 2, canonical_scale=B.CANONICAL_SCALE, canonical_level=B.CANONICAL_LEVEL)
    x = dict(zip(NAMES, feats))
    none = module(x, [torch.zeros((0, 4), device=DEV), torch.zeros((0, 4), device=DEV)], [B.IMAGE, B.IMAGE])
    assert none.shape == (0, 3, 7, 7) and none.dtype == torch.float32

    boxes = B.fpn_boxes()
    dev_boxes = [torch.from_numpy(b.copy()).to(DEV) for b in boxes]
    single = ops.MultiScaleRoIAlign(["p3"], (2, 3), 2)(x, dev_boxes, [B.IMAGE, B.IMAGE])  # one map: plain roi_align
    assert _lib.last_kernel().startswith("k_roi_align<")
    want = ops.roi_align(feats[1], dev_boxes, (2, 3), 0.125, 2)
    assert torch.equal(_bits(single), _bits(want))

    half_boxes = [b.half() for b in dev_boxes]
    half = module(dict(zip(NAMES, _features(torch.float16))), half_boxes, [B.IMAGE, B.IMAGE])
    assert half.dtype == torch.float16
    f32_feats = [f.float() for f in _features(torch.float16)]
    wide = ops._multiscale_roi_align_impl(f32_feats, ops._convert_to_roi_format([b.float() for b in half_boxes]),
                                          _cpu_levels([b.cpu().numpy() for b in half_boxes]).to(DEV), SCALES, 7, 7, 2)
    assert torch.equal(half, wide.half())  # computed in float32, narrowed once

    g = feats[0].clone().requires_grad_(True)
    out = module({**x, "p2": g}, dev_boxes, [B.IMAGE, B.IMAGE])
    with pytest.raises(RuntimeError, match="forward-only"):
        out.sum().backward()
    with pytest.raises(NotImplementedError, match="float64"):
        module({k: v.double() for k, v in x.items()}, [b.double() for b in dev_boxes], [B.IMAGE, B.IMAGE])
