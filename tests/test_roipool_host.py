"""ops.roi_pool / ps_roi_pool / ps_roi_align without a GPU: argument checks and their messages, what reaches the operators, the
reprs, the C ABI's host-side validation, and the references of tests/_roipool_ref.py themselves -- on hand-checkable inputs, and
the float32 restatement against its float64 form on the shapes tests/test_gpu_roipool.py runs."""
import numpy as np
import pytest
import torch

from cpu_vision_amd import _lib, ops
from tests import _detect_ref as R
from tests import _roipool_ref as P
from tests._detect_cases import roi_rois
from tests._roipool_cases import (DEGENERATE_ROIS, OPS, OUTPUTS, POOL_CONFIGS, PS_ALIGN_CONFIGS, SCALES, SHAPES, input_shape,
                                  pool_input, pool_reference, same_as_aligned_roi_align)

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
PUBLIC = {"roi_pool": ops.roi_pool, "ps_roi_pool": ops.ps_roi_pool, "ps_roi_align": ops.ps_roi_align}
MULTIPLE = "input channels must be a multiple of pooling height \\* pooling width"


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_checks_boxes_and_input(op):
    fn, x = PUBLIC[op], torch.zeros(1, 4, 4, 4)
    with pytest.raises(AssertionError, match=r"The boxes tensor shape is not correct as Tensor\[K, 5\]"):
        fn(x, torch.zeros(3, 4), 2)
    with pytest.raises(AssertionError, match=r"The shape of the tensor in the boxes list is not correct as List\[Tensor\[L, 4\]\]"):
        fn(x, [torch.zeros(3, 4), torch.zeros(2, 5)], 2)
    with pytest.raises(AssertionError, match=r"boxes is expected to be a Tensor\[L, 5\] or a List\[Tensor\[K, 4\]\]"):
        fn(x, 7, 2)
    with pytest.raises(RuntimeError, match="4-D input"):
        fn(torch.zeros(4, 4, 4), torch.zeros(1, 5), 2)
    impl = getattr(ops, f"_{op}_impl")
    tail = (-1,) if op == "ps_roi_align" else ()
    with pytest.raises(RuntimeError, match=r"rois must have shape as Tensor\[K, 5\]"):
        impl(x, torch.zeros(1, 4), 1.0, 2, 2, *tail)
    with pytest.raises(RuntimeError, match=r"rois must have shape as Tensor\[K, 5\]"):
        impl(x, torch.zeros(5), 1.0, 2, 2, *tail)


@pytest.mark.parametrize("op", OPS)
def test_cpu_tensors_raise(op):
    fn, x = PUBLIC[op], torch.zeros(1, 4, 4, 4)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        fn(x, torch.zeros(1, 5), 2)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        fn(x, [torch.zeros(1, 4)], (2, 2))
    module = {"roi_pool": ops.RoIPool(2, 1.0), "ps_roi_pool": ops.PSRoIPool(2, 1.0), "ps_roi_align": ops.PSRoIAlign(2, 1.0, -1)}[op]
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        module(x, torch.zeros(1, 5))


@pytest.mark.parametrize("op", OPS)
def test_dtype_gates_and_channel_multiple(op, monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda t, what="input": None)
    fn = PUBLIC[op]
    with pytest.raises(NotImplementedError, match="float64"):
        fn(torch.zeros(1, 4, 2, 2, dtype=torch.float64), torch.zeros(1, 5, dtype=torch.float64), 1)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        fn(torch.zeros(1, 4, 2, 2, dtype=torch.bfloat16), torch.zeros(1, 5, dtype=torch.bfloat16), 1)
    with pytest.raises(RuntimeError, match="to have the same type"):
        fn(torch.zeros(1, 4, 2, 2), torch.zeros(1, 5, dtype=torch.float16), 1)
    if op != "roi_pool":
        with pytest.raises(RuntimeError, match=MULTIPLE):
            fn(torch.zeros(1, 5, 4, 4), torch.zeros(1, 5), 2)
        with pytest.raises(RuntimeError, match=MULTIPLE):
            fn(torch.zeros(1, 7, 4, 4), torch.zeros(1, 5), (2, 3))


def test_output_size_int_and_pair_list_and_tensor(monkeypatch):
    """What reaches each operator: an int becomes a pair, a list of boxes the (K, 5) tensor; the public function returns the first
    tensor of the pair."""
    seen = []

    def fake(name):
        def impl(input, rois, spatial_scale, pooled_height, pooled_width, *tail):
            seen.append((name, tuple(rois.shape), spatial_scale, pooled_height, pooled_width) + tail)
            shape = (rois.shape[0], input.shape[1], pooled_height, pooled_width)
            return torch.zeros(shape), torch.ones(shape, dtype=torch.int32)
        return impl

    for op in OPS:
        monkeypatch.setattr(ops, f"_{op}_impl", fake(op))
    x = torch.zeros(2, 3, 8, 8)
    boxes = [torch.zeros(1, 4), torch.zeros(2, 4)]
    for op in ("roi_pool", "ps_roi_pool"):
        fn = PUBLIC[op]
        y = fn(x, torch.zeros(4, 5), 3)
        assert isinstance(y, torch.Tensor) and y.shape == (4, 3, 3, 3) and y.dtype == torch.float32
        assert fn(x, boxes, (2, 5), 0.25).shape == (3, 3, 2, 5)
    assert ops.RoIPool((7, 6), 0.5)(x, torch.zeros(1, 5)).shape == (1, 3, 7, 6)
    assert ops.PSRoIPool(4, 0.125)(x, boxes).shape == (3, 3, 4, 4)
    assert ops.ps_roi_align(x, torch.zeros(4, 5), 3).shape == (4, 3, 3, 3)
    assert ops.ps_roi_align(x, boxes, (2, 5), 0.25, 2).shape == (3, 3, 2, 5)
    assert ops.PSRoIAlign((7, 6), 0.5, 1)(x, torch.zeros(1, 5)).shape == (1, 3, 7, 6)
    assert seen == [("roi_pool", (4, 5), 1.0, 3, 3), ("roi_pool", (3, 5), 0.25, 2, 5),
                    ("ps_roi_pool", (4, 5), 1.0, 3, 3), ("ps_roi_pool", (3, 5), 0.25, 2, 5),
                    ("roi_pool", (1, 5), 0.5, 7, 6), ("ps_roi_pool", (3, 5), 0.125, 4, 4),
                    ("ps_roi_align", (4, 5), 1.0, 3, 3, -1), ("ps_roi_align", (3, 5), 0.25, 2, 5, 2),
                    ("ps_roi_align", (1, 5), 0.5, 7, 6, 1)]
    assert all(type(v) is float for s in seen for v in s[2:3]) and all(type(v) is int for s in seen for v in s[3:])


def test_reprs_and_exports():
    assert repr(ops.RoIPool(7, 0.25)) == "RoIPool(output_size=7, spatial_scale=0.25)"
    assert repr(ops.PSRoIPool((3, 2), 1.0)) == "PSRoIPool(output_size=(3, 2), spatial_scale=1.0)"
    assert repr(ops.PSRoIAlign(7, 0.0625, 2)) == "PSRoIAlign(output_size=7, spatial_scale=0.0625, sampling_ratio=2)"
    for schema, name in ((ops._ROI_POOL_SCHEMA, "roi_pool"), (ops._PS_ROI_POOL_SCHEMA, "ps_roi_pool"),
                         (ops._PS_ROI_ALIGN_SCHEMA, "ps_roi_align")):
        assert schema.startswith(name + "(Tensor input, Tensor rois, float spatial_scale, SymInt pooled_height, SymInt pooled_width")
        assert schema.endswith("-> (Tensor, Tensor)")
    assert "int sampling_ratio" in ops._PS_ROI_ALIGN_SCHEMA and "sampling_ratio" not in ops._PS_ROI_POOL_SCHEMA


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ("roi_align",) + OPS)
def test_abi_validates_on_the_host(op):
    """Every rejection happens before a launch (the pointers are made up); k == 0, c == 0 and a zero output side succeed without one.
    The four entry points share one set of checks; roi_align has no second output, so `second` is not passed on."""
    lib = _lib.load()
    fn = getattr(lib, f"mv_{op}_f32")
    ps = op in ("ps_roi_pool", "ps_roi_align")
    pair = op != "roi_align"
    tail = {"roi_align": (-1, 0, None), "ps_roi_align": (-1, None)}.get(op, (None,))
    c = 98 if ps else 3  # 2 * 7 * 7

    def call(x=16, rois=32, y=64, second=128, n=2, c=c, h=8, w=8, k=1, ph=7, pw=7):
        return fn(x, rois, y, *((second,) if pair else ()), n, c, h, w, k, ph, pw, 1.0, *tail)

    assert call(None, None, None, None, k=0) == 0
    assert call(None, None, None, None, c=0) == 0
    assert call(None, None, None, None, ph=0) == 0 and call(None, None, None, None, pw=0) == 0
    for bad in (dict(k=-1), dict(h=-8), dict(n=-1), dict(c=-1), dict(w=-1), dict(ph=-1), dict(pw=-7)):
        assert call(**bad) == -1 and b"bad shape" in lib.mv_last_error(), bad
        assert (op + ":").encode() in lib.mv_last_error()
    assert call(h=0) == -1 and b"empty" in lib.mv_last_error()
    assert call(w=0) == -1 and b"empty" in lib.mv_last_error()
    assert call(h=65536, w=65536) == -2 and b"plane index" in lib.mv_last_error()
    assert call(c=(1 << 20) * (49 if ps else 1), k=1 << 40) == -2 and b"launch grid" in lib.mv_last_error()
    for null in (dict(x=None), dict(rois=None), dict(y=None)) + ((dict(second=None),) if pair else ()):
        assert call(**null) == -1 and b"null pointer" in lib.mv_last_error(), null
    message = b"output must not alias input or the other output" if pair else b"output must not alias input"
    for alias in (dict(y=16), dict(y=32)) + ((dict(second=16), dict(second=32), dict(second=64)) if pair else ()):
        assert call(**alias) == -1 and lib.mv_last_error() == message, alias
    if ps:
        for c_bad in (97, 99, 1, 48):
            assert call(c=c_bad) == -1 and b"input channels must be a multiple of pooling height * pooling width" in lib.mv_last_error()
        assert call(None, None, None, None, c=97, k=0) == 0  # nothing to do comes first
        assert call(c=6, ph=2, pw=3, y=None) == -1 and b"null pointer" in lib.mv_last_error()  # a multiple passes that check


# ---- the restatements on hand-checkable inputs ---------------------------------------------------------------------------------------
def _plane(h, w, seed=0, c=1, n=1):
    return (np.random.default_rng(seed).random((n, c, h, w)) * 2 - 1).astype(F32)


def test_roundf_is_half_away_from_zero():
    assert [P.roundf(F32(v)) for v in (0.5, 1.5, 2.5, -0.5, -2.5, 2.4999, -0.49, 0.0)] == [1, 2, 3, -1, -3, 2, -0.0, 0]
    assert P.rounded_corner(F32(10.0), 0.25, F32) == 3 and P.rounded_corner(F32(-10.0), 0.25, F32) == -3  # 2.5 -> 3: not half-to-even
    assert P.rounded_corner(F32("nan"), 1.0, F32) == 0
    assert P.rounded_corner(F32(3e38), 10.0, F32) == 2 ** 29 and P.rounded_corner(F32(-1e30), 1.0, F32) == -2 ** 29


def test_roi_pool_of_the_whole_map():
    h, w = 5, 7
    x = _plane(h, w, c=3)
    whole = np.array([[0, 0, 0, w - 1, h - 1]], F32)
    y, arg = P.roi_pool_ref(x, whole, (1, 1), 1.0)
    flat = x[0].reshape(3, -1)
    assert np.array_equal(y[0, :, 0, 0], flat.max(1)) and np.array_equal(arg[0, :, 0, 0], flat.argmax(1)) and arg.dtype == np.int32
    y, arg = P.roi_pool_ref(x, whole, (h, w), 1.0)
    assert np.array_equal(y[0], x[0])
    assert np.array_equal(arg[0], np.broadcast_to(np.arange(h * w, dtype=np.int32).reshape(h, w), (3, h, w)))


def test_roi_pool_ties_outside_and_nan():
    h, w = 6, 9
    x = np.full((1, 2, h, w), 0.25, F32)
    rois = np.array([[0, 1, 1, 7, 4]], F32)
    y, arg = P.roi_pool_ref(x, rois, (2, 3), 1.0)
    win = P.pool_windows(rois, (2, 3), 1.0, h, w)
    assert np.all(y == F32(0.25))
    assert np.array_equal(arg[0, 0], (win[0, :, :, 0] * w + win[0, :, :, 2]).astype(np.int32))  # the first of equal values wins
    assert win[0, 0, 0].tolist() == [1, 3, 1, 4] and win[0, 1, 2].tolist() == [3, 5, 5, 8]  # 4 rows in 2 bins, 7 columns in 3
    outside = np.array([[0, -30, -30, -12, -15], [0, w + 4, h + 3, w + 20, h + 9]], F32)
    y, arg = P.roi_pool_ref(_plane(h, w), outside, (2, 2), 1.0)
    assert np.all(y == 0) and np.all(arg == -1)
    x = _plane(h, w)
    x[0, 0, 1:3, 1:3] = np.nan
    y, arg = P.roi_pool_ref(x, np.array([[0, 1, 1, 2, 2]], F32), (1, 1), 1.0)
    assert y[0, 0, 0, 0] == -FLT_MAX and arg[0, 0, 0, 0] == -1
    y, arg = P.roi_pool_ref(x, np.array([[0, 1, 1, 3, 2]], F32), (1, 1), 1.0)  # one more column: NaNs are passed over
    assert y[0, 0, 0, 0] == max(x[0, 0, 1, 3], x[0, 0, 2, 3]) and arg[0, 0, 0, 0] in (1 * w + 3, 2 * w + 3)


def test_batch_index_outside_the_input():
    x = _plane(4, 4, c=4, n=2)
    rois = np.array([[2, 0, 0, 3, 3], [-1, 0, 0, 3, 3], [1e9, 0, 0, 3, 3], [np.nan, 0, 0, 3, 3], [-0.5, 0, 0, 3, 3], [1.9, 0, 0, 3, 3]], F32)
    y, arg = P.roi_pool_ref(x, rois, (2, 2), 1.0)
    assert np.all(y[:4] == 0) and np.all(arg[:4] == -1) and np.all(arg[4:] >= 0)
    assert np.array_equal(y[4], P.roi_pool_ref(x[:1], np.array([[0, 0, 0, 3, 3]], F32), (2, 2), 1.0)[0][0])  # -0.5 truncates to 0
    assert np.array_equal(y[5], P.roi_pool_ref(x[1:], np.array([[0, 0, 0, 3, 3]], F32), (2, 2), 1.0)[0][0])  # 1.9 to 1
    for ref in (lambda: P.ps_roi_pool_ref(x, rois, (2, 2), 1.0), lambda: P.ps_roi_align_ref(x, rois, (2, 2), 1.0, 2)):
        y, mapping = ref()
        assert np.all(y[:4] == 0) and np.all(y[4:] != 0) and np.array_equal(mapping[0], mapping[5])


def test_ps_roi_pool_mean_of_the_whole_map_and_mapping():
    h, w = 13, 17
    x = _plane(h, w, c=6)
    y, mapping = P.ps_roi_pool_ref(x, np.array([[0, 0, 0, w, h]], F32), (1, 1), 1.0)
    assert y.shape == (1, 6, 1, 1) and mapping.dtype == np.int32 and mapping[0, :, 0, 0].tolist() == list(range(6))
    mean64 = x[0].astype(np.float64).reshape(6, -1).mean(1)
    bound = h * w * 2.0 ** -24 * float(np.abs(x).max())
    assert np.abs(y[0, :, 0, 0].astype(np.float64) - mean64).max() <= bound
    x = _plane(h, w, c=2 * 2 * 3)
    _, mapping = P.ps_roi_pool_ref(x, np.array([[0, 1, 1, 9, 9], [0, 2, 2, 5, 5]], F32), (2, 3), 1.0)
    _, mapping_a = P.ps_roi_align_ref(x, np.array([[0, 1, 1, 9, 9], [0, 2, 2, 5, 5]], F32), (2, 3), 1.0, 1)
    want = np.array([[[(co * 2 + ph) * 3 + pw for pw in range(3)] for ph in range(2)] for co in range(2)], np.int32)
    assert np.array_equal(mapping, np.stack([want, want])) and np.array_equal(mapping_a, mapping)
    # each output reads ITS channel: a plane of constant value v_c gives v_c at the bins mapped to it
    const = np.broadcast_to(np.arange(12, dtype=F32).reshape(1, 12, 1, 1), (1, 12, h, w)).copy()
    y, _ = P.ps_roi_pool_ref(const, np.array([[0, 1, 1, 9, 9]], F32), (2, 3), 1.0)
    assert np.array_equal(y[0], want.astype(F32))
    y, _ = P.ps_roi_align_ref(const, np.array([[0, 1, 1, 9, 9]], F32), (2, 3), 1.0, 2)
    assert np.array_equal(y[0], want.astype(F32))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("out", OUTPUTS, ids=str)
def test_ps_roi_align_is_nan_exactly_where_the_adaptive_grid_has_no_sample_count(out, scale):
    """count = grid_h * grid_w without a max(.., 1): 0 / 0 = NaN where the product is 0.  Exactly the zero-size and the
    negative-size roi have an empty adaptive grid; the zero-size roi's product is 0 at every output size, the negative-size one's
    (size -5 x -5 on the map) whenever ceil(-5 / pooled) is 0 on an axis -- at 7 x 7 both are NaN, as every other output is not --
    and with sampling_ratio > 0 both are finite."""
    rois = roi_rois("main", scale, 51)
    assert len(rois) == 65
    grids = P.adaptive_grids(rois, out, scale)
    assert tuple(np.flatnonzero((grids <= 0).any(1))) == DEGENERATE_ROIS
    assert grids[DEGENERATE_ROIS[0]].tolist() == [0, 0]
    assert grids[DEGENERATE_ROIS[1]].tolist() == [int(np.ceil(-5 / out[0])), int(np.ceil(-5 / out[1]))]
    (y, _), (y64, _), _ = pool_reference("ps_roi_align", "main", (out, scale, -1), 51)
    nan_rois = np.flatnonzero(grids.prod(1) == 0)
    if out == (7, 7):
        assert tuple(nan_rois) == DEGENERATE_ROIS
    for arr in (y, y64):
        isnan = np.isnan(arr)
        assert np.array_equal(np.flatnonzero(isnan.any((1, 2, 3))), nan_rois) and np.array_equal(isnan.all((1, 2, 3)), isnan.any((1, 2, 3)))
        assert np.all(arr[[r for r in DEGENERATE_ROIS if r not in nan_rois]] == 0)
    for ratio in (1, 2):
        (y, _), _, _ = pool_reference("ps_roi_align", "main", (out, scale, ratio), 51)
        assert np.isfinite(y).all()


@pytest.mark.parametrize("cfg", PS_ALIGN_CONFIGS, ids=str)
def test_ps_roi_align_is_aligned_roi_align_gathered_by_channel_mapping(cfg):
    """The two restatements agree bit for bit wherever the divisor is the same: what lets the kernels share one bin sampler."""
    out, scale, ratio = cfg
    (y, mapping), _, rois = pool_reference("ps_roi_align", "main", cfg)
    full = R.roi_align_ref(pool_input("ps_roi_align", "main", out), rois, out, scale, ratio, True)
    same_as_aligned_roi_align(y, mapping, full, ratio, f"ps_roi_align_ref {cfg}")


# ---- the conditions under which the float64 yardstick means something ----------------------------------------------------------------
@pytest.mark.parametrize("cfg", POOL_CONFIGS, ids=str)
def test_windows_are_identical_in_float32_and_float64_and_mostly_not_empty(cfg):
    out, scale = cfg
    _, _, h, w = input_shape("roi_pool", "main", out)
    rois = roi_rois("main", scale, 51)
    assert len(rois) == 65
    expected_empty = {(1, 1): (11, 11), (2, 3): (110, 104), (7, 7): (1156, 1024)}[out]
    for ps, want_empty in zip((False, True), expected_empty):
        w32, w64 = P.pool_windows(rois, out, scale, h, w, np.float32, ps), P.pool_windows(rois, out, scale, h, w, np.float64, ps)
        assert np.array_equal(w32, w64), f"{'ps_roi_pool' if ps else 'roi_pool'} {cfg}: windows differ between float32 and float64"
        empty = (w32[..., 1] <= w32[..., 0]) | (w32[..., 3] <= w32[..., 2])
        assert empty.size == 65 * out[0] * out[1]
        assert int(empty.sum()) == want_empty, (cfg, ps, int(empty.sum()))
        assert 2 * int(empty.sum()) <= empty.size, f"{cfg}: more than half of the bins are empty"


@pytest.mark.parametrize("op", OPS)
def test_float32_and_float64_references_agree(op):
    cfgs = PS_ALIGN_CONFIGS if op == "ps_roi_align" else POOL_CONFIGS
    for cfg in cfgs:
        for shape in SHAPES:
            (y32, s32), (y64, s64), rois = pool_reference(op, shape, cfg)
            n, c, h, w = input_shape(op, shape, cfg[0])
            c_out = c if op == "roi_pool" else c // (cfg[0][0] * cfg[0][1])
            assert y32.dtype == np.float32 and y64.dtype == np.float64 and y32.shape == y64.shape == (len(rois), c_out) + cfg[0]
            assert s32.dtype == s64.dtype == np.int32 and np.array_equal(s32, s64), (op, cfg, shape)
            assert np.array_equal(np.isnan(y32), np.isnan(y64)), (op, cfg, shape)
            ok = ~np.isnan(y64)
            if op == "roi_pool":
                assert np.array_equal(y32[ok].astype(np.float64), y64[ok])  # a maximum of the same elements: no rounding at all
            else:
                assert np.abs(y32[ok].astype(np.float64) - y64[ok]).max() <= 1e-5, (op, cfg, shape)
