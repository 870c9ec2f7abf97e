"""ops.roi_pool / ps_roi_pool / ps_roi_align on the MI355X (`-m gpu`) against tests/_roipool_ref.py, the reference's CPU kernels
restated in numpy (and against torchvision's own CPU ops where that package is importable; nothing here requires it).

Both outputs of every op are bit-for-bit the float32 restatement (NaN in equal places for ps_roi_align); independently the two
averaging ops assert  max|kernel - float64| <= 2 max|float32 restatement - float64|  over the non-NaN elements of the same inputs
(tests/test_roipool_host.py asserts that the windows are the same in both precisions and mostly not empty)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, ops  # noqa: E402
from tests import _detect_ref as R  # noqa: E402
from tests import _roipool_ref as P  # noqa: E402
from tests._detect_cases import roi_rois  # noqa: E402
from tests._roipool_cases import OPS, configs, pool_input, pool_reference, same_as_aligned_roi_align  # noqa: E402

try:
    import torchvision.ops as tv_ops
except Exception:  # not installed, or built against another torch
    tv_ops = None

DEV = "cuda"
MULTIPLE = "input channels must be a multiple of pooling height \\* pooling width"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _impl(op, x, rois, cfg):
    """The operator's pair (output, second) through ops._<op>_impl."""
    out, scale = cfg[0], cfg[1]
    return getattr(ops, f"_{op}_impl")(x, rois, float(scale), out[0], out[1], *cfg[2:])


def _public(op, x, rois, cfg):
    return getattr(ops, op)(x, rois, cfg[0], cfg[1], *cfg[2:])


def _check(op, got, f32, f64, what):
    """got, f32, f64: (output, second).  Prints the error figures before it asserts, as test_gpu_detect._check_roi does."""
    y, second = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert got[1].dtype == torch.int32 and got[1].device.type == "cuda", (what, got[1].dtype, got[1].device)
    assert y.dtype == np.float32 and y.shape == f32[0].shape and second.shape == f32[1].shape, (what, y.shape, f32[0].shape)
    assert np.array_equal(np.isnan(y), np.isnan(f32[0])), f"{what}: NaN in other places than in the restatement"
    ok = ~np.isnan(f64[0])
    err = float(np.abs(y.astype(np.float64) - f64[0])[ok].max()) if ok.any() else 0.0
    ref_err = float(np.abs(f32[0].astype(np.float64) - f64[0])[ok].max()) if ok.any() else 0.0
    differ = int((~np.isclose(y, f32[0], rtol=0, atol=0, equal_nan=True)).sum())
    print(f"{what}: max|kernel - f64| = {err:.3e}, max|float32 restatement - f64| = {ref_err:.3e}, {differ} of {y.size} elements and "
          f"{int((second != f32[1]).sum())} of the second output differ from the restatement, {int((~ok).sum())} NaN")
    if op != "roi_pool":
        assert err <= 2 * ref_err, f"{what}: error {err:.3e} against float64 exceeds twice the restatement's own {ref_err:.3e}"
    assert np.array_equal(y, f32[0], equal_nan=True), f"{what}: {differ} of {y.size} elements differ from the float32 restatement"
    assert np.array_equal(second, f32[1]), f"{what}: the second output differs from the restatement"


def _tv(op, x, rois, cfg):
    fn = getattr(tv_ops, op)
    return fn(torch.from_numpy(np.array(x)), torch.from_numpy(np.array(rois)), cfg[0], cfg[1], *cfg[2:]).numpy()


@pytest.mark.parametrize("op", OPS)
def test_equals_the_float32_restatement(op):
    for cfg in configs(op):
        for shape in ("main", "tiny"):
            f32, f64, rois = pool_reference(op, shape, cfg)
            x, r = _dev(pool_input(op, shape, cfg[0])), _dev(rois)
            x0, r0 = x.clone(), r.clone()
            got = _impl(op, x, r, cfg)
            assert torch.equal(x, x0) and torch.equal(r, r0), f"{op} changed its inputs"
            _check(op, got, f32, f64, f"{op} {shape} {cfg}")
            if tv_ops is not None:
                assert np.array_equal(got[0].cpu().numpy(), _tv(op, pool_input(op, shape, cfg[0]), rois, cfg), equal_nan=True), \
                    f"{op} {shape} {cfg}: differs from torchvision's CPU op"


@pytest.mark.parametrize("ratio", (-1, 2))
@pytest.mark.parametrize("scale", (1.0, 0.25))
@pytest.mark.parametrize("out", ((2, 3), (7, 7)), ids=str)
def test_ps_roi_align_is_aligned_roi_align_gathered_by_channel_mapping(out, scale, ratio):
    """k_ps_roi_align and k_roi_align sum a bin with the same device function: on the same map their outputs are the same bits."""
    x, r = _dev(pool_input("ps_roi_align", "main", out)), _dev(roi_rois("main", scale))
    y, mapping = ops._ps_roi_align_impl(x, r, float(scale), out[0], out[1], ratio)
    assert torch.equal(ops.ps_roi_align(x, r, out, scale, ratio).nan_to_num(7.0), y.nan_to_num(7.0))
    full = ops.roi_align(x, r, out, scale, ratio, aligned=True)
    same_as_aligned_roi_align(y.cpu().numpy(), mapping.cpu().numpy(), full.cpu().numpy(), ratio, f"ps_roi_align {(out, scale, ratio)}")


@pytest.mark.parametrize("op", OPS)
def test_roi_counts(op):
    cfg = ((7, 7), 0.25) + ((-1,) if op == "ps_roi_align" else ())
    f32, f64, rois = pool_reference(op, "main", cfg, extra=51)
    assert len(rois) == 65
    x = _dev(pool_input(op, "main", cfg[0]))
    for k in (0, 1, 65):
        got = _impl(op, x, _dev(rois[:k]).reshape(k, 5), cfg)
        _check(op, got, tuple(a[:k] for a in f32), tuple(a[:k] for a in f64), f"{op} k={k}")
        y = _public(op, x, _dev(rois[:k]).reshape(k, 5), cfg)
        assert torch.equal(y.isnan(), got[0].isnan()) and torch.equal(y.nan_to_num(7.0), got[0].nan_to_num(7.0))


def _args(op, x, rois, out, scale, ratio=None):
    return (x, rois, out, scale) + ((ratio,) if op == "ps_roi_align" else ())


@pytest.mark.parametrize("op", OPS)
def test_list_of_boxes_int_output_size_and_module(op):
    ref = getattr(P, op + "_ref")
    x_np = pool_input(op, "main", (2, 3))
    x = _dev(x_np)
    per_image = [np.array([[2.3, 1.7, 9.6, 8.2], [0.0, 0.0, 17.0, 13.0]], np.float32), np.array([[4.5, 0.0, 9.5, 4.0]], np.float32)]
    rois = R.convert_boxes_to_roi_format_ref(per_image)
    tail = (2,) if op == "ps_roi_align" else ()
    got = getattr(ops, op)(x, [_dev(b) for b in per_image], (2, 3), 1.0, *tail)
    want = ref(*_args(op, x_np, rois, (2, 3), 1.0, 2))[0]
    assert np.array_equal(got.cpu().numpy(), want), f"{op}: a list of boxes"
    x_np = pool_input(op, "main", (3, 3))  # 18 channels for the 3 x 3 bins of the position-sensitive ops
    x = _dev(x_np)
    module = {"roi_pool": lambda: ops.RoIPool(3, 0.5), "ps_roi_pool": lambda: ops.PSRoIPool(3, 0.5),
              "ps_roi_align": lambda: ops.PSRoIAlign(3, 0.5, -1)}[op]()
    doubled = rois * np.array([1, 2, 2, 2, 2], np.float32)
    got = module(x, _dev(doubled))
    want = ref(*_args(op, x_np, doubled, (3, 3), 0.5, -1))[0]
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), f"{op}: the module with an int output_size"


@pytest.mark.parametrize("op", OPS)
def test_batch_index_outside_the_input_gives_zeros(op):
    x = _dev(pool_input(op, "main", (2, 2)))
    rois = _dev(np.array([[2, 1, 1, 9, 9], [-1, 1, 1, 9, 9], [1e9, 1, 1, 9, 9], [float("nan"), 1, 1, 9, 9], [1, 1, 1, 9, 9]], np.float32))
    cfg = ((2, 2), 1.0) + ((2,) if op == "ps_roi_align" else ())
    y, second = (t.cpu() for t in _impl(op, x, rois, cfg))
    assert torch.equal(y[:4], torch.zeros_like(y[:4])) and bool((y[4] != 0).all())
    if op == "roi_pool":
        assert bool((second[:4] == -1).all()) and bool((second[4] >= 0).all())
    else:
        assert all(torch.equal(second[i], second[4]) for i in range(4)) and second[4].flatten().tolist() == list(range(x.shape[1]))


@pytest.mark.parametrize("op", OPS)
def test_float16_is_the_float32_result_narrowed_and_float64_raises(op):
    cfg = ((7, 7), 0.25) + ((2,) if op == "ps_roi_align" else ())
    _, _, rois = pool_reference(op, "main", cfg)
    xh, rh = _dev(pool_input(op, "main", cfg[0])).half(), _dev(rois).half()
    got, second = _impl(op, xh, rh, cfg)
    want, second32 = _impl(op, xh.float(), rh.float(), cfg)
    assert got.dtype == torch.float16 and torch.equal(got, want.half()) and second.dtype == torch.int32 and torch.equal(second, second32)
    assert _public(op, xh, rh, cfg).dtype == torch.float16
    with pytest.raises(NotImplementedError):
        _public(op, xh.double(), rh.double(), cfg)
    with pytest.raises(_lib.Mi355VisionError):
        _public(op, xh.float(), rh.float().cpu(), cfg)


@pytest.mark.parametrize("op", OPS)
def test_side_stream_views_registered_operator_and_backward(op):
    cfg = ((2, 3), 1.0) + ((-1,) if op == "ps_roi_align" else ())
    f32, f64, rois = pool_reference(op, "main", cfg)
    x, r = _dev(pool_input(op, "main", cfg[0])), _dev(rois)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = _impl(op, x, r, cfg)
    side.synchronize()
    _check(op, got, f32, f64, f"{op} on a side stream")
    wide = torch.zeros((len(rois), 7), device=DEV)
    wide[:, 1:6] = r
    view = wide[:, 1:6]
    assert not view.is_contiguous()
    _check(op, _impl(op, x, view, cfg), f32, f64, f"{op} with rois as a non-contiguous view")
    ops.register_torchvision_op()
    registered = getattr(torch.ops.torchvision, op)
    tail = (-1,) if op == "ps_roi_align" else ()
    pair = registered(x, r, 1.0, 2, 3, *tail)
    assert isinstance(pair, (tuple, list)) and len(pair) == 2
    _check(op, pair, f32, f64, f"torch.ops.torchvision.{op}")
    for call in (lambda t: getattr(ops, op)(t, r, (2, 3), 1.0, *tail), lambda t: registered(t, r, 1.0, 2, 3, *tail)[0]):
        xg = x.clone().requires_grad_(True)
        y = call(xg)
        assert y.requires_grad
        with pytest.raises(RuntimeError, match="forward-only"):
            y.nan_to_num().sum().backward()
    second = registered(x.clone().requires_grad_(True), r, 1.0, 2, 3, *tail)[1]
    assert second.dtype == torch.int32 and not second.requires_grad


@pytest.mark.parametrize("op", ["ps_roi_pool", "ps_roi_align"])
def test_a_channel_count_that_is_no_multiple_raises(op):
    x, r = torch.zeros((1, 7, 4, 4), device=DEV), torch.zeros((1, 5), device=DEV)
    with pytest.raises(RuntimeError, match=MULTIPLE):
        getattr(ops, op)(x, r, (2, 3))
    ops.register_torchvision_op()
    tail = (-1,) if op == "ps_roi_align" else ()
    with pytest.raises(RuntimeError, match=MULTIPLE):
        getattr(torch.ops.torchvision, op)(x, r, 1.0, 2, 3, *tail)
