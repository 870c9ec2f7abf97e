"""Kernels at element offsets past 2^31 and byte offsets past 2^31 and 2^32 ("Large offsets").

Every case fills its big input on the device, runs ONE launch into an output pre-filled with NaN (or with a value the op cannot
produce), and asserts
  * the oracle / reference of the op's small-shape test, bit for bit, on the first rows, the last rows and the rows on both sides
    of every boundary the input or the output crosses (tests/_large.py states the flat offsets and asserts they straddle);
  * that no sentinel is left and that the WHOLE output equals the same op run band by band on slices whose offsets all stay below
    2^31 bytes -- a size-independence property, which is what finds a store that wrapped to a place the sampled rows do not see;
  * the kernel that served it, where the case exists for one.
The shapes are the smallest that cross the boundary in question; no test holds more than 24 GiB of device memory (the fixture
below asserts it) and the host touches a few MB."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, _misc, ops  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _boxes_ref as B  # noqa: E402
from tests import _large as L  # noqa: E402
from tests import _mix_ref as MR  # noqa: E402
from tests import _resnet_ref as RR  # noqa: E402
from tests._util import philox_f32  # noqa: E402

NAN = float("nan")
CAP = 24 * 2 ** 30


@pytest.fixture(autouse=True)
def device_memory_cap():
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak <= CAP, f"the test held {peak / 2 ** 30:.1f} GiB of device memory"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nans(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def equal_on_device(got, want):
    """Bit-for-bit as values on the device, without a NaN in `got` (the sentinel)."""
    return not bool(torch.isnan(got).any()) and torch.equal(got, want)


# ---- ops whose output rows depend on a few input rows of the same plane -----------------------------------------------------------
def rowwise_case(x, y, planes, rin, win, rout, wout, scale, cut, small, oracle, band, need=()):
    """x viewed as (planes, rin, win) -> y viewed as (planes, rout, wout), already computed by one launch into a NaN-filled y.
    small(rows of one plane, on the device) -> its output rows (the same op, a launch of its own); oracle(the same, numpy)."""
    xv, yv = x.view(planes, rin, win), y.view(planes, rout, wout)
    picks = L.pick_rows(planes, rin, win, x.element_size(), rout, wout, y.element_size(), scale)
    what = L.assert_crossings_straddled(picks, cut, planes, rin, win, x.element_size(), rout, wout, y.element_size(), need)
    for p, runs in picks.items():
        for a, b in runs:
            lo, hi, drop, _ = cut(a, b, rin)
            want = oracle(xv[p, lo:hi].cpu().numpy())[drop:drop + (b - a)]
            np.testing.assert_array_equal(yv[p, a:b].cpu().numpy(), want, err_msg=f"plane {p} rows [{a}, {b}); {what}")
    for p in range(planes):
        for a in range(0, rout, band):
            b = min(a + band, rout)
            lo, hi, drop, _ = cut(a, b, rin)
            assert (hi - lo) * win * x.element_size() < L.B31 and (b - a + drop) * wout * y.element_size() < L.B31
            assert equal_on_device(yv[p, a:b], small(xv[p, lo:hi])[drop:drop + (b - a)]), f"plane {p} rows [{a}, {b}) differ from the band's own launch"


# ---- conv2d_bias_relu: k_conv3x3 (pipelined and KS == 0), k_conv3x3_c3, k_conv3x3_gen ----------------------------------------------
def conv3x3_case(cin, cout, h, w, relu, kernel, band, seed, need=()):
    x = L.fill(torch.empty((1, cin, h, w), device="cuda"), seed)
    wt = (philox_f32(seed + 1, (cout, cin, 3, 3)) - 0.5) * 0.5
    bias = philox_f32(seed + 2, (cout,)) + 0.5  # most outputs are positive: a ReLU zero would hide a misplaced store
    wd, bd = dev(wt), dev(bias)
    assert F.conv3x3_k_slices(1, cin, h, w, cout)[0] == 1  # one ascending chain per output at this size
    y = nans((1, cout, h, w))
    F.conv2d_bias_relu(x, wd, bd, relu=relu, out=y)
    name = _lib.last_kernel()
    assert name == kernel if kernel.startswith("k_conv3x3<") else kernel in name, name
    # the rows to compare: first, last, and around every boundary of the input (cin, h, w) and of the output (cout, h, w)
    rows = {0, 1, h - 2, h - 1}
    xc, yc = L.crossings(x.numel(), 4), L.crossings(y.numel(), 4)
    for e in list(xc.values()) + list(yc.values()):
        rows.update(L.rows_near(e, w, h))
    out_ranges, in_ranges = [], []
    for a, b in L.strips(rows):
        lo, hi, drop, first = L.cut_conv3(a, b, h)
        out_ranges += L.plane_ranges(range(cout), h, w, a, b)
        in_ranges += L.plane_ranges(range(cin), h, w, first, hi)
    for name, e in yc.items():
        L.assert_straddles(out_ranges, e, "output " + name)
    for name, e in xc.items():
        L.assert_straddles(in_ranges, e, "input " + name)
    crossed = ["output " + k for k in yc] + ["input " + k for k in xc]
    assert all(k in crossed for k in need), (need, crossed)
    what = f"output {L.describe(out_ranges, 4)}; input {L.describe(in_ranges, 4)}; crossed {crossed}"
    for a, b in L.strips(rows):
        lo, hi, drop, _ = L.cut_conv3(a, b, h)
        want = ref.conv3x3_bias_relu(x[:, :, lo:hi].cpu().numpy(), wt, bias, relu=relu)[:, :, drop:drop + (b - a)]
        np.testing.assert_array_equal(y[:, :, a:b].cpu().numpy(), want, err_msg=f"rows [{a}, {b}); {what}")
    for a in range(0, h, band):
        b = min(a + band, h)
        lo, hi, drop, _ = L.cut_conv3(a, b, h)
        assert max(cin, cout) * (hi - lo) * w * 4 < L.B31
        yb = F.conv2d_bias_relu(x[:, :, lo:hi].contiguous(), wd, bd, relu=relu, sliced_k=False)
        assert equal_on_device(y[:, :, a:b], yb[:, :, drop:drop + (b - a)]), f"rows [{a}, {b}) differ from the band's own launch"


@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("w", [14720, 14730], ids=["w%32==0", "w%4!=0"])
def test_conv3x3_first_generation_kernel_with_20_planes_past_4_gib(cin, w):
    """k_conv3x3 at cout 8 (the hf == 1 lanes store channels 4 .. 7) with 20 * h * w >= 2^32: the pipelined epilogue's 32-bit lane
    offset (4 * hf planes + one plane, in bytes) would wrap -- at w = 14720 for rows >= 14065 of channels 4 .. 7, whose stores would
    land in channels 0 .. 3 and leave 4 .. 7 unwritten -- so launch_conv3x3 sends these planes to the KS == 0 instantiation."""
    h = 14720
    assert 20 * h * w >= 2 ** 32 > 16 * h * w
    conv3x3_case(cin, 8, h, w, relu=(w % 32 == 0), kernel="k_conv3x3<ks0>", band=2048, seed=100 + cin + w, need=("output byte 2^32",))


def test_conv3x3_pipelined_epilogue_at_its_largest_lane_offset():
    """The largest plane the pipelined epilogue still takes: lane offsets up to 20 * h * w - 4 bytes, just below 2^32."""
    h, w = 14716, 14592  # w = 57 x 256: every tile inside the row, the unpredicated (FULLW) form
    assert 2 ** 32 - 2 ** 18 < 20 * h * w < 2 ** 32 and w % 256 == 0
    conv3x3_case(3, 8, h, w, relu=False, kernel="k_conv3x3<ks14,fullw>", band=2048, seed=120, need=("output byte 2^31",))


@pytest.mark.parametrize("w,kernel", [(4092, "k_conv3x3_c3"), (4096, "k_conv3x3<ks14,fullw>")], ids=["below 2^32", "at 2^32"])
def test_conv3x3_c3_window(w, kernel):
    """cin 3, cout 64: an image whose output is just below 2^32 bytes is k_conv3x3_c3's largest; at exactly 2^32 it leaves c3."""
    h = 4096
    assert (64 * h * w * 4 < 2 ** 32) == (kernel == "k_conv3x3_c3") and 64 * h * (w + 4) * 4 >= 2 ** 32
    conv3x3_case(3, 64, h, w, relu=True, kernel=kernel, band=1024, seed=130 + w, need=("output byte 2^31",))


@pytest.mark.parametrize("h,kernel", [(33026, "k_conv3x3_gen"), (33027, "k_conv3x3<ks0>")], ids=["below 2^32", "past 2^32"])
def test_conv3x3_gen_window(h, kernel):
    """cin 8, cout 60, w 508: (cout + 4) * h * w * 4 just below 2^32 is k_conv3x3_gen's largest image (one chain per output: the
    plan does not slice K at this size, asserted in conv3x3_case); one row more goes to k_conv3x3 (KS == 0)."""
    w = 508
    assert ((60 + 4) * h * w * 4 < 2 ** 32) == (kernel == "k_conv3x3_gen") and 2 ** 32 - 2 ** 18 < 64 * 33026 * w * 4
    conv3x3_case(8, 60, h, w, relu=(h % 2 == 0), kernel=kernel, band=4096, seed=140 + h, need=("output byte 2^31",))


# ---- pools -----------------------------------------------------------------------------------------------------------------------------
def _pool(entry, x, y, *args):
    _lib.launch(getattr(_lib.load(), entry), x, x.data_ptr(), y.data_ptr(), *args)


def test_maxpool2x2_input_past_2_31_elements():
    p, h, w = 3, 26760, 26760
    assert p * h * w > 2 ** 31 and w % 8 == 0
    x = L.fill(torch.empty((p, h, w), device="cuda"), 200)
    y = nans((p, h // 2, w // 2))
    _pool("mv_maxpool2x2_f32", x, y, p, h, w)
    assert _lib.last_kernel() == "k_maxpool2x2"
    rowwise_case(x, y, p, h, w, h // 2, w // 2, 2, L.cut_pool2, lambda xs: F.max_pool2d_2x2(xs[None])[0],
                 lambda a: ref.maxpool2x2(a[None])[0], band=8192, need=("input element 2^31", "output byte 2^31"))


def test_max_pool2d_k3_s2_input_past_2_31_elements():
    p, h, w = 3, 26761, 26763
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    assert p * h * w > 2 ** 31
    x = L.fill(torch.empty((p, h, w), device="cuda"), 201)
    y = nans((p, oh, ow))
    _pool("mv_maxpool2d_f32", x, y, p, h, w, 3, 2)
    assert _lib.last_kernel() == "k_maxpool2d"
    rowwise_case(x, y, p, h, w, oh, ow, 2, L.cut_pool3s2, lambda xs: F.max_pool2d(xs[None], 3, 2)[0],
                 lambda a: ref.maxpool2d(a[None], 3, 2)[0], band=8192, need=("input element 2^31", "output byte 2^31"))


def test_padded_max_pool_3_2_1_input_past_2_31_elements():
    p, h, w = 3, 26761, 26760
    oh, ow = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    assert p * h * w > 2 ** 31
    x = L.fill(torch.empty((p, h, w), device="cuda"), 202)
    y = nans((p, oh, ow))
    _pool("mv_maxpool2d_pad_f32", x, y, p, h, w, 3, 2, 1)
    assert _lib.last_kernel() == "k_maxpool2d_pad"
    rowwise_case(x, y, p, h, w, oh, ow, 2, L.cut_pool3s2p1, lambda xs: F.max_pool2d(xs[None], 3, 2, 1)[0],
                 lambda a: RR.padded_max_pool(a[None], 3, 2, 1)[0], band=8192, need=("input element 2^31", "output byte 2^31"))


@pytest.mark.parametrize("h,w,oh,ow,kernel", [(33, 31, 7, 7, "k_adaptive_avgpool"), (7, 7, 1, 1, "k_global_avgpool_small")])
def test_adaptive_avg_pool_input_past_2_31_elements(h, w, oh, ow, kernel):
    planes = 2 ** 31 // (h * w) + 3
    x = L.fill(torch.empty((planes, h, w), device="cuda"), 203)
    y = nans((planes, oh, ow))
    _pool("mv_adaptive_avgpool_f32", x, y, planes, h, w, oh, ow)
    assert _lib.last_kernel() == kernel
    # a "row" is a whole plane here: output plane i reads input plane i
    rowwise_case(x, y, 1, planes, h * w, planes, oh * ow, 1, L.cut_same,
                 lambda xs: F.adaptive_avg_pool2d(xs.view(-1, h, w), (oh, ow)).view(-1, oh * ow),
                 lambda a: ref.adaptive_avgpool(a.reshape(-1, h, w), oh, ow).reshape(-1, oh * ow), band=2 ** 30 // (h * w * 4),
                 need=("input element 2^31",))


@pytest.mark.parametrize("shape,out", [((2, 70000, 1), (40000, 1)), ((1, 3, 70000), (2, 40000)), ((1, 50000, 50000 // 7), (46000, 3))], ids=str)
def test_adaptive_avg_pool_window_products_past_2_31(shape, out):
    """Not a large tensor: the window bounds floor(o * in / out) and ceil((o + 1) * in / out) have products past 2^31 as soon as
    out * in >= 2^31 (70000 -> 40000 is 280 KB); as 32-bit products they turned negative and the kernel read before its input."""
    assert max(out[0] * shape[1], out[1] * shape[2]) >= 2 ** 31
    x = philox_f32(205, shape)
    got = F.adaptive_avg_pool2d(dev(x), out)
    assert _lib.last_kernel() == "k_adaptive_avgpool"
    np.testing.assert_array_equal(got.cpu().numpy(), ref.adaptive_avgpool(x, *out))
    # torch's CPU op as a second witness of the windows (the oracle had the same 32-bit products).  It does not state its order of
    # summation: a window of N elements in [0, 1) summed in two orders differs by at most 2 (N - 1) 2^-24 N (each of the N - 1
    # additions of each sum rounds a partial sum < N), i.e. 2 (N - 1) 2^-24 after the division, plus one rounding of the quotient;
    # a window of at most two elements has one order only and must be equal.  A wrong window is off by ~1 / sqrt(N), far outside.
    want = torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(x), out).numpy()
    win = min(-(-shape[1] // out[0]) + 1, shape[1]) * min(-(-shape[2] // out[1]) + 1, shape[2])  # ceil(in / out) + 1 per axis at the most
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"adaptive_avg_pool {shape} -> {out}: window <= {win} elements, max |kernel - torch CPU| = {err:.3e}")
    assert err <= (0.0 if win <= 2 else 2 * (win - 1) * 2.0 ** -24 + 2.0 ** -24)


# ---- to_float_normalize (uint8) and normalize (float32) ---------------------------------------------------------------------------------
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@pytest.mark.parametrize("tail", [0, 3], ids=["hw%4==0", "hw%4!=0"])
def test_to_float_normalize_u8_one_plane_past_2_31_elements(tail):
    hw = 2 ** 31 + 3 * 4096 + tail
    x = L.fill(torch.empty((1, 1, 1, hw), dtype=torch.uint8, device="cuda"), 210, 0, 256)
    y = nans((1, 1, 1, hw))
    m, s = _misc._mean_std([0.45], [0.225], 1)
    _lib.launch(_lib.load().mv_to_float_normalize_u8, x, x.data_ptr(), y.data_ptr(), 1, 1, hw, m, s)
    assert _lib.last_kernel() == "k_to_float_normalize"
    # rows of 4096 elements (the kernel's chunk); the ragged end is compared on its own below
    rows = hw // 4096
    rowwise_case(x.view(-1)[:rows * 4096], y.view(-1)[:rows * 4096], 1, rows, 4096, rows, 4096, 1, L.cut_same,
                 lambda xs: F.to_float_normalize(xs.view(1, 1, -1), [0.45], [0.225]).view(-1, 4096),
                 lambda a: ref.to_float_normalize(a.reshape(1, 1, 1, -1), [0.45], [0.225]).reshape(-1, 4096), band=1 << 16,
                 need=("input element 2^31", "input byte 2^31", "output element 2^31", "output byte 2^32"))
    end = slice(rows * 4096 - 4096, hw)
    np.testing.assert_array_equal(y.view(-1)[end].cpu().numpy(),
                                  ref.to_float_normalize(x.view(-1)[end].cpu().numpy().reshape(1, 1, 1, -1), [0.45], [0.225]).reshape(-1))


def test_normalize_f32_batch_past_2_31_elements():
    hw = 2500
    n = 2 ** 31 // (3 * hw) + 3
    x = L.fill(torch.empty((n, 3, 50, 50), device="cuda"), 211, 0.0, 1.0)
    y = nans((n, 3, 50, 50))
    m, s = _misc._mean_std(MEAN, STD, 3)
    _lib.launch(_lib.load().mv_normalize_f32, x, x.data_ptr(), y.data_ptr(), n, 3, hw, m, s)
    assert _lib.last_kernel() == "k_to_float_normalize"
    # a "row" is one image (3 planes)
    rowwise_case(x, y, 1, n, 3 * hw, n, 3 * hw, 1, L.cut_same,
                 lambda xs: F.normalize(xs.view(-1, 3, 50, 50), MEAN, STD).view(-1, 3 * hw),
                 lambda a: ref.to_float_normalize(a.reshape(-1, 3, 50, 50), MEAN, STD).reshape(-1, 3 * hw), band=1 << 15,
                 need=("input element 2^31", "output element 2^31"))


# ---- linear_bias_relu --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(4, 132), (132, 4)], ids=["n*m past 2^31", "n*k past 2^31"])
def test_linear_past_2_31_elements(k, m):
    """Neither shape is K-sliced (mv_linear_k_slices: the grid is far past 512 workgroups), so the workspace entry point runs the
    same single chain as the plain one: its whole output must equal the plain entry point's, which is the one checked in bands."""
    n = 2 ** 31 // 132 + 37
    assert n * max(k, m) > 2 ** 31 and F.linear_k_slices(n, k, m)[0] == 1
    x = L.fill(torch.empty((n, k), device="cuda"), 220)
    wt = philox_f32(221, (m, k)) - 0.5
    bias = philox_f32(222, (m,)) - 0.25
    wd, bd = dev(wt), dev(bias)
    lib = _lib.load()
    args = (x.data_ptr(), wd.data_ptr(), bd.data_ptr())
    y = nans((n, m))
    _lib.launch(lib.mv_linear_bias_relu_f32, x, *args, y.data_ptr(), n, k, m, 1)
    assert _lib.last_kernel() == "k_linear", _lib.last_kernel()
    rowwise_case(x, y, 1, n, k, n, m, 1, L.cut_same, lambda xs: F.linear_bias_relu(xs, wd, bd, relu=True, sliced_k=False),
                 lambda a: ref.linear_bias_relu(a, wt, bias, relu=True), band=1 << 21,
                 need=("output element 2^31",) if m > k else ("input element 2^31",))
    y2 = nans((n, m))
    _lib.launch(lib.mv_linear_bias_relu_ws_f32, x, *args, y2.data_ptr(), n, k, m, 1, None, 0)
    assert _lib.last_kernel() == "k_linear" and torch.equal(y2, y)


# ---- mixup / cutmix / mixup_labels: y[b] = mix(x[b - 1], x[b]) ------------------------------------------------------------------------------
LAM = 0.3


def _mix_launch(x, y, batch, elems, kernel):
    entry = {torch.float32: "mv_mixup_f32", torch.float16: "mv_mixup_f16", torch.float64: "mv_mixup_f64"}[x.dtype]
    _lib.launch(getattr(_lib.load(), entry), x, x.data_ptr(), y.data_ptr(), batch, elems, LAM)
    assert _lib.last_kernel().startswith(kernel), _lib.last_kernel()


def _column_picks(batch, elems, itemsize, seg):
    """Column segments [a, b) of a (batch, elems) tensor (input and output alike): the first, the last, and those around every
    boundary the tensor crosses; asserts that they straddle."""
    cols = [(0, seg), (elems - seg, elems)]
    cross = L.crossings(batch * elems, itemsize)
    for e in cross.values():
        c = e % elems
        if c == 0:
            continue  # the boundary falls between two samples: the first and last segments hold its two sides
        cols.append((max(c - seg, 0), min(c + seg, elems)))
    ranges = [(b * elems + a, b * elems + z) for b in range(batch) for a, z in cols]
    for name, e in cross.items():
        L.assert_straddles(ranges, e, name)
    return cols, cross, L.describe(ranges, itemsize)


def wide_sample_case(x, y, small, reference, seg, band, need):
    """x, y (batch, elems) with few, huge samples: columns are independent, so segments and bands are column ranges."""
    batch, elems = x.shape
    cols, cross, what = _column_picks(batch, elems, x.element_size(), seg)
    assert all(k in cross for k in need), (need, list(cross))
    for a, b in cols:
        assert torch.equal(y[:, a:b].cpu(), reference(x[:, a:b].cpu())), f"columns [{a}, {b}); {what}"
    for a in range(0, elems, band):
        b = min(a + band, elems)
        assert batch * (b - a) * x.element_size() < L.B31
        assert torch.equal(y[:, a:b], small(x[:, a:b].contiguous())), f"columns [{a}, {b}) differ from the band's own launch"


def many_samples_case(x, y, small, reference, need, sentinel_free):
    """x (batch, ...) -> y (batch, ...) with many small samples: output sample b reads input samples b - 1 (the last one for b = 0)
    and b, so a cut of samples [a, b) is run on samples a - 1 .. b - 1 and its first output dropped."""
    batch = x.shape[0]
    xe, ye = x[0].numel(), y[0].numel()
    picks = L.pick_rows(1, batch, xe, x.element_size(), batch, ye, y.element_size())
    cut = lambda a, b, rin: (a - 1, b, 1, max(a - 1, 0))  # noqa: E731  (sample -1 is the last one)
    out_ranges, in_ranges = L.compared_ranges(picks, cut, batch, xe, batch, ye)
    in_ranges.append(((batch - 1) * xe, batch * xe))  # read by output sample 0
    cross = []
    for side, ranges, numel, item in (("input", in_ranges, x.numel(), x.element_size()), ("output", out_ranges, y.numel(), y.element_size())):
        for name, e in L.crossings(numel, item).items():
            L.assert_straddles(ranges, e, f"{side} {name}")
            cross.append(f"{side} {name}")
    assert all(k in cross for k in need), (need, cross)

    def take(a, b):
        return torch.cat([x[a - 1:] if a == 0 else x[a - 1:a], x[a:b]])

    for a, b in picks[0]:
        assert torch.equal(y[a:b].cpu(), reference(take(a, b).cpu())[1:]), f"samples [{a}, {b}); crossed {cross}"
    band = 2 ** 30 // max(xe * x.element_size(), ye * y.element_size())  # samples per band: 1 GiB of the larger side
    for a in range(0, batch, band):
        b = min(a + band, batch)
        assert (b - a + 1) * max(xe * x.element_size(), ye * y.element_size()) < L.B31
        assert sentinel_free(y[a:b]) and torch.equal(y[a:b], small(take(a, b))[1:]), f"samples [{a}, {b}) differ from the band's own launch"


def _no_nan(t):
    return not bool(torch.isnan(t).any())


def test_mixup_f16_roll_one_sample_past_2_31_elements():
    elems = 2 ** 31 + 8 * 1000 + 6  # the last 16-byte group of a sample is anchored at its end
    x = L.fill(torch.empty((2, elems), dtype=torch.float16, device="cuda"), 230)
    y = nans((2, elems), torch.float16)
    _mix_launch(x, y, 2, elems, "k_mixup_roll<f16")
    assert _no_nan(y)
    wide_sample_case(x, y, lambda xs: F.mixup_image(xs, LAM), lambda xs: MR.mixup_image(xs, LAM), 4096, 1 << 28,
                     ("element 2^31", "byte 2^31", "byte 2^32"))


@pytest.mark.parametrize("dtype,name", [(torch.float16, "f16"), (torch.float32, "f32")], ids=["f16", "f32"])
def test_mixup_flat_one_sample_past_2_31_elements(dtype, name):
    """A batch of ONE sample past 2^31 elements (a batch of one mixes the sample with itself: no walk, k_mixup_flat): two tensors of
    2^31 elements fit the cap for float32 too; with two such samples (the walk, above) only float16 does."""
    elems = 2 ** 31 + 8 * 1000 + 6
    x = L.fill(torch.empty((1, elems), dtype=dtype, device="cuda"), 231)
    y = nans((1, elems), dtype)
    _mix_launch(x, y, 1, elems, f"k_mixup_flat<{name}")
    assert _no_nan(y)
    wide_sample_case(x, y, lambda xs: F.mixup_image(xs, LAM), lambda xs: MR.mixup_image(xs, LAM), 4096, 1 << 27,
                     ("element 2^31", "byte 2^31", "byte 2^32"))


@pytest.mark.parametrize("dtype,elems,kernel", [(torch.float32, 1001, "k_mixup_roll<f32"), (torch.float32, 101, "k_mixup_flat<f32"),
                                                (torch.float64, 1001, "k_mixup_roll<f64")], ids=["f32 roll", "f32 flat", "f64 roll"])
def test_mixup_many_samples_past_2_31_elements(dtype, elems, kernel):
    """float64: two tensors of 2^31 doubles are 32 GiB, past the cap; the batch is 2^30 elements, which crosses byte 2^31 and 2^32
    (and 2^33) but not element 2^31."""
    total = 2 ** 31 if dtype == torch.float32 else 2 ** 30
    batch = total // elems + 5
    x = L.fill(torch.empty((batch, elems), dtype=dtype, device="cuda"), 232)
    y = nans((batch, elems), dtype)
    _mix_launch(x, y, batch, elems, kernel)
    need = ("input element 2^31", "output element 2^31") if dtype == torch.float32 else ("input byte 2^32", "output byte 2^32")
    many_samples_case(x, y, lambda xs: F.mixup_image(xs, LAM), lambda xs: MR.mixup_image(xs, LAM), need, _no_nan)


BOX = (100, 37, 901, 1000)  # x1, y1, x2, y2


@pytest.mark.parametrize("dtype,batch", [(torch.uint8, 2), (torch.int16, 2), (torch.int32, 1)], ids=["1 byte", "2 bytes", "4 bytes, batch 1"])
def test_cutmix_one_sample_past_2_31_elements(dtype, batch):
    """The 64-bit branch of k_cutmix (G.elems > 0x7fffffff).  With 4-byte elements two samples past 2^31 elements, in and out, are
    32 GiB -- past the cap -- so that element size runs with a batch of one (the sample is its own partner; the addressing is the
    same) and, with many small samples, in test_cutmix_many_samples."""
    h, w = 1000, 1001  # 16-byte groups straddle rows and box edges
    planes = 2 ** 31 // (h * w) + 2
    elems = planes * h * w
    assert elems > 0x7fffffff
    x = L.fill(torch.empty((batch, planes, h, w), dtype=dtype, device="cuda"), 240, 0, 255)  # never 255: the sentinel
    y = torch.full_like(x, 255)
    _lib.launch(_lib.load().mv_cutmix, x, x.data_ptr(), y.data_ptr(), batch, planes, x.element_size(), h, w, *BOX)
    assert _lib.last_kernel() == f"k_cutmix<b{x.element_size()}>"
    assert not bool((y == 255).any())
    # the planes on both sides of every boundary the (batch, elems) tensors cross, the first and the last: whole planes, so that
    # the box keeps its place in every cut
    cols, cross, what = _column_picks(batch, elems, x.element_size(), 1)
    assert all(k in cross for k in ("element 2^31", "byte 2^31", "byte 2^32")), list(cross)
    for a, b in cols:
        p0, p1 = a // (h * w), (b - 1) // (h * w) + 1
        assert torch.equal(y[:, p0:p1].cpu(), MR.cutmix_image(x[:, p0:p1].cpu(), BOX)), f"planes [{p0}, {p1}); {what}"
    band = 2 ** 29 // (batch * h * w * x.element_size())
    for p0 in range(0, planes, band):
        p1 = min(p0 + band, planes)
        assert batch * (p1 - p0) * h * w * x.element_size() < L.B31
        assert torch.equal(y[:, p0:p1], F.cutmix_image(x[:, p0:p1].contiguous(), BOX)), f"planes [{p0}, {p1}) differ from the band's own launch"


def test_cutmix_many_samples_past_2_31_elements():
    h, w = 32, 33
    box = (5, 3, 30, 29)
    batch = 2 ** 31 // (3 * h * w) + 5
    x = L.fill(torch.empty((batch, 3, h, w), device="cuda"), 241)
    y = nans((batch, 3, h, w))
    _lib.launch(_lib.load().mv_cutmix, x, x.data_ptr(), y.data_ptr(), batch, 3, 4, h, w, *box)
    assert _lib.last_kernel() == "k_cutmix<b4>"
    many_samples_case(x, y, lambda xs: F.cutmix_image(xs, box), lambda xs: MR.cutmix_image(xs, box),
                      ("input element 2^31", "output element 2^31"), _no_nan)


def test_mixup_labels_outputs_past_2_31():
    classes = 1000
    batch = 2 ** 31 // classes + 5
    labels = L.fill(torch.empty((batch,), dtype=torch.int64, device="cuda"), 250, 0, classes)
    y = nans((batch, classes))
    _lib.launch(_lib.load().mv_mixup_labels_i64, labels, labels.data_ptr(), y.data_ptr(), batch, classes, LAM)
    assert _lib.last_kernel() == "k_mixup_labels<vec>"
    many_samples_case(labels, y, lambda xs: F.mixup_labels(xs, LAM, classes), lambda xs: MR.mixup_label(xs, LAM, classes),
                      ("output element 2^31", "output byte 2^32"), _no_nan)


# ---- box_iou family, masks_to_boxes ------------------------------------------------------------------------------------------------------
def _boxes(n, seed):
    """(n, 4) random boxes of positive area in a 100 x 100 field, on the device: every pair's value is finite."""
    p = L.fill(torch.empty((n, 2), device="cuda"), seed, 0.0, 80.0)
    wh = L.fill(torch.empty((n, 2), device="cuda"), seed + 1, 1.0, 41.0)
    return torch.cat([p, p + wh], 1).contiguous()


@pytest.mark.parametrize("m", [46342, 46344], ids=["scalar", "vec16"])
@pytest.mark.parametrize("mode", ["box_iou", "generalized_box_iou", "distance_box_iou"])  # the three the library has (no complete_box_iou)
def test_box_iou_pairs_past_2_31(mode, m):
    n = 46342
    assert n * m > 2 ** 31
    b1, b2 = _boxes(n, 260), _boxes(m, 262)
    b2_cpu = b2.cpu()
    y = nans((n, m))
    _lib.launch(_lib.load().mv_box_iou_f32, b1, b1.data_ptr(), b2.data_ptr(), y.data_ptr(), n, m, ops._IOU_MODES[mode])
    assert ("vec16" if m % 4 == 0 else "scalar") in _lib.last_kernel()
    fn = getattr(ops, mode)
    rowwise_case(b1, y, 1, n, 4, n, m, 1, L.cut_same, lambda xs: fn(xs, b2),
                 lambda a: B.TORCH_REF[mode](torch.from_numpy(a), b2_cpu).numpy(), band=8192,
                 need=("output element 2^31", "output byte 2^31", "output byte 2^32"))
    cols = [0, 1, m // 2, m - 2, m - 1]  # sampled columns, every row
    want = B.TORCH_REF[mode](b1.cpu(), b2_cpu[cols])
    assert torch.equal(y[:, cols].cpu(), want)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_masks_to_boxes_masks_past_2_31_elements(dtype):
    h, w = 255, 257
    n = 2 ** 31 // (h * w) + 3
    assert n * h * w > 2 ** 31
    masks = torch.zeros((n, h, w), dtype=dtype, device="cuda")
    # two set pixels per mask, different for every mask
    i = torch.arange(n, device="cuda")
    ya, xa, yb, xb = (i * 7) % h, (i * 13) % w, (i * 31 + 5) % h, (i * 17 + 3) % w
    masks[i, ya, xa] = 1
    masks[i, yb, xb] = 200
    boxes = nans((n, 4))
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    lib = _lib.load()
    ws, ws_ptr, nbytes = _lib.workspace(int(lib.mv_masks_to_boxes_workspace_bytes(n)), masks.device)
    entry = lib.mv_masks_to_boxes_u8 if dtype == torch.uint8 else lib.mv_masks_to_boxes_f32
    _lib.launch(entry, masks, masks.data_ptr(), boxes.data_ptr(), flag.data_ptr(), n, h, w, ws_ptr, nbytes)
    assert int(flag.item()) == 0 and "k_mtb_reduce" in _lib.last_kernel()
    rowwise_case(masks, boxes, 1, n, h * w, n, 4, 1, L.cut_same, lambda xs: ops.masks_to_boxes(xs.view(-1, h, w)),
                 lambda a: B.masks_to_boxes_ref(torch.from_numpy(a.reshape(-1, h, w))).numpy(), band=4096,
                 need=("input element 2^31",))
    want = torch.stack([torch.minimum(xa, xb), torch.minimum(ya, yb), torch.maximum(xa, xb), torch.maximum(ya, yb)], 1).float()
    assert torch.equal(boxes, want)


# ---- roi_align / roi_pool / ps_roi_pool / ps_roi_align / multiscale_roi_align: feature maps past 2^31 elements ------------------------------
ROI_C, ROI_H, ROI_W = 12, 30, 50  # 12 channels: a multiple of the 2 x 3 bins of the position-sensitive ops


def _roi_images(n, per_image):
    """The images whose rois are compared: the first, the last, and the one that holds flat element 2^31 with its neighbours."""
    mid = 2 ** 31 // per_image
    assert mid * per_image < 2 ** 31 - 1 and 2 ** 31 < (mid + 1) * per_image < n * per_image  # elements 2^31 - 1 and 2^31 lie inside image `mid`
    return [0, mid - 1, mid, mid + 1, n - 1]


def _rois_on(images):
    """Per image: the whole map (every element of every channel is read by the pooling ops), a box in the middle, one over the
    bottom right corner.  (K, 5) float32 rows [image, x1, y1, x2, y2] in the input's scale (spatial_scale 0.5)."""
    boxes = [(0.0, 0.0, 2.0 * ROI_W, 2.0 * ROI_H), (21.3, 9.8, 70.1, 44.4), (60.5, 30.25, 110.0, 70.0)]
    return np.array([[float(b), *box] for b in images for box in boxes], np.float32)


@pytest.mark.parametrize("op", ["roi_align", "roi_pool", "ps_roi_pool", "ps_roi_align"])
def test_roi_ops_feature_map_past_2_31_elements(op):
    from tests import _detect_ref as DR
    from tests import _roipool_ref as P
    per_image = ROI_C * ROI_H * ROI_W
    n = 2 ** 31 // per_image + 3
    assert n < 2 ** 24  # the image index travels as a float32
    x = L.fill(torch.empty((n, ROI_C, ROI_H, ROI_W), device="cuda"), 300)
    images = _roi_images(n, per_image)
    rois = _rois_on(images)
    local = rois.copy()
    local[:, 0] = np.repeat(np.arange(len(images)), 3)  # the same rois on the cut x[images]
    cut = x[images]
    if op == "roi_align":
        run = lambda t, r: ops.roi_align(t, r, (2, 3), 0.5, 2, True)  # noqa: E731
        want = DR.roi_align_ref(cut.cpu().numpy(), local, (2, 3), 0.5, 2, True, np.float32)
    elif op == "ps_roi_align":
        run = lambda t, r: ops.ps_roi_align(t, r, (2, 3), 0.5, 2)  # noqa: E731
        want = P.ps_roi_align_ref(cut.cpu().numpy(), local, (2, 3), 0.5, 2)[0]
    else:
        run = lambda t, r: getattr(ops, op)(t, r, (2, 3), 0.5)  # noqa: E731
        want = getattr(P, op + "_ref")(cut.cpu().numpy(), local, (2, 3), 0.5)[0]
    # the big launch through the C entry, into a NaN-filled output
    rd = dev(rois)
    c_out = ROI_C if op in ("roi_align", "roi_pool") else ROI_C // 6
    got = nans((len(rois), c_out, 2, 3))
    shape = (n, ROI_C, ROI_H, ROI_W, len(rois), 2, 3, 0.5)
    lib = _lib.load()
    if op == "roi_align":
        _lib.launch(lib.mv_roi_align_f32, x, x.data_ptr(), rd.data_ptr(), got.data_ptr(), *shape, 2, 1)
    else:
        second = torch.full(got.shape, -7, dtype=torch.int32, device="cuda")
        _lib.launch(getattr(lib, f"mv_{op}_f32"), x, x.data_ptr(), rd.data_ptr(), got.data_ptr(), second.data_ptr(), *shape,
                    *((2,) if op == "ps_roi_align" else ()))
        assert not bool((second == -7).any())
    assert _lib.last_kernel().startswith("k_" + op), _lib.last_kernel()
    assert _no_nan(got) and got.shape == want.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)  # every channel, the last one included
    assert torch.equal(got, run(cut, dev(local))), "differs from the launch on the cut images"


def test_multiscale_roi_align_level_past_2_31_elements():
    per_image = ROI_C * ROI_H * ROI_W
    n = 2 ** 31 // per_image + 3
    feats = [L.fill(torch.empty((n, ROI_C, ROI_H, ROI_W), device="cuda"), 310),
             L.fill(torch.empty((n, ROI_C, ROI_H // 2, ROI_W // 2), device="cuda"), 311)]
    scales = [0.5, 0.25]
    images = _roi_images(n, per_image)
    rois = _rois_on(images)
    levels = np.tile(np.array([0, 1, 0], np.int64), len(images))  # the whole-map roi of every image on the big level
    local = rois.copy()
    local[:, 0] = np.repeat(np.arange(len(images)), 3)
    cuts = [f[images] for f in feats]
    got = ops._multiscale_roi_align_impl(feats, dev(rois), dev(levels), scales, 2, 3, 2)
    assert _lib.last_kernel().startswith("k_multiscale_roi_align<levels2"), _lib.last_kernel()
    want = B.multiscale_ref([c.cpu().numpy() for c in cuts], local, levels, scales, (2, 3), 2)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, ops._multiscale_roi_align_impl(cuts, dev(local), dev(levels), scales, 2, 3, 2))


def test_roi_align_output_past_2_31_elements():
    from tests import _detect_ref as DR
    c, h, w, ph, pw = 64, 20, 30, 7, 7
    k = 2 ** 31 // (c * ph * pw) + 3
    feat = L.fill(torch.empty((2, c, h, w), device="cuda"), 320)
    feat_np = feat.cpu().numpy()
    p = L.fill(torch.empty((k, 2), device="cuda"), 321, 0.0, 40.0)
    wh = L.fill(torch.empty((k, 2), device="cuda"), 322, 1.0, 30.0)
    img = (torch.arange(k, device="cuda") % 2).float()[:, None]
    rois = torch.cat([img, p, p + wh], 1).contiguous()
    y = nans((k, c, ph, pw))
    _lib.launch(_lib.load().mv_roi_align_f32, feat, feat.data_ptr(), rois.data_ptr(), y.data_ptr(), 2, c, h, w, k, ph, pw, 0.5, 2, 0)
    assert _lib.last_kernel() == "k_roi_align<legacy,fixed>"
    rowwise_case(rois, y, 1, k, 5, k, c * ph * pw, 1, L.cut_same,
                 lambda rs: ops.roi_align(feat, rs, (ph, pw), 0.5, 2, False).view(-1, c * ph * pw),
                 lambda a: DR.roi_align_ref(feat_np, a, (ph, pw), 0.5, 2, False, np.float32).reshape(-1, c * ph * pw),
                 band=2 ** 30 // (c * ph * pw * 4), need=("output element 2^31", "output byte 2^32"))


# ---- conv_norm_act (pointwise, depthwise, small-cin 3x3) and conv1x1_upsample_add: batch 2, every tensor past 2^31 elements --------------
def conv_rows_case(n, cin, cout, h, w, y, small, oracle, halo, band, need, even=False):
    """x (n, cin, h, w) -> y (n, cout, h, w), stride 1, already computed into a NaN-filled y.  small(lo, hi) / oracle(lo, hi): the op
    on input rows [lo, hi) of every image -- a launch of its own on the device / the oracle on the host.  halo: input rows an
    output row reads above and below.  even: cuts start on even rows and have even length (a 2x nearest upsample keeps its place)."""
    rows = {0, 1, h - 2, h - 1}
    xc, yc = L.crossings(n * cin * h * w, 4), L.crossings(n * cout * h * w, 4)
    for e in list(xc.values()) + list(yc.values()):
        rows.update(L.rows_near(e, w, h))
    if even:
        rows = {r & ~1 for r in rows} | {r | 1 for r in rows}
    cut = (lambda a, b: (max(a - halo, 0), min(b + halo, h)))
    out_ranges, in_ranges = [], []
    for a, b in L.strips(rows):
        lo, hi = cut(a, b)
        out_ranges += L.plane_ranges(range(n * cout), h, w, a, b)
        in_ranges += L.plane_ranges(range(n * cin), h, w, lo, hi)
    for name, e in yc.items():
        L.assert_straddles(out_ranges, e, "output " + name)
    for name, e in xc.items():
        L.assert_straddles(in_ranges, e, "input " + name)
    crossed = ["output " + k for k in yc] + ["input " + k for k in xc]
    assert all(k in crossed for k in need), (need, crossed)
    what = f"output {L.describe(out_ranges, 4)}; input {L.describe(in_ranges, 4)}; crossed {crossed}"
    for a, b in L.strips(rows):
        lo, hi = cut(a, b)
        want = oracle(lo, hi)[:, :, a - lo:a - lo + (b - a)]
        np.testing.assert_array_equal(y[:, :, a:b].cpu().numpy(), want, err_msg=f"rows [{a}, {b}); {what}")
    for a in range(0, h, band):
        b = min(a + band, h)
        lo, hi = cut(a, b)
        assert n * max(cin, cout) * (hi - lo) * w * 4 < L.B31
        assert equal_on_device(y[:, :, a:b], small(lo, hi)[:, :, a - lo:a - lo + (b - a)]), f"rows [{a}, {b}) differ from the band's own launch"


CNA_H = CNA_W = 11586  # 2 x 8 x 11586^2 > 2^31


def _cna_terms(cout, seed):
    alpha = philox_f32(seed, (cout,)) + 0.5
    beta = philox_f32(seed + 1, (cout,)) - 0.5
    return alpha, beta


@pytest.mark.parametrize("kind", ["pointwise", "depthwise"])
def test_conv_norm_act_8_channels_past_2_31_elements(kind):
    """The residual is the input itself (a third tensor of 2^31 floats would pass the memory cap): both are only read."""
    n, c, h, w = 2, 8, CNA_H, CNA_W
    assert n * c * h * w > 2 ** 31
    x = L.fill(torch.empty((n, c, h, w), device="cuda"), 400)
    if kind == "pointwise":
        wt, groups, halo, kernel = philox_f32(401, (c, c, 1, 1)) - 0.5, 1, 0, "k_conv1x1<"
        assert F.conv1x1_k_slices(n, c, h, w, c)[0] == 1
    else:
        wt, groups, halo, kernel = philox_f32(402, (c, 1, 3, 3)) - 0.5, c, 1, "k_dwpc3x3"
    alpha, beta = _cna_terms(c, 403)
    wd, ad, bd = dev(wt), dev(alpha), dev(beta)
    y = nans((n, c, h, w))
    p = _lib.ptr
    _lib.launch(_lib.load().mv_conv_norm_act_f32, x, 2 if kind == "pointwise" else 1, x.data_ptr(), wd.data_ptr(), None, p(ad), p(bd),
                x.data_ptr(), y.data_ptr(), n, c, h, w, c, 1, 2, 2)  # affine fma, ReLU6
    assert _lib.last_kernel().startswith(kernel), _lib.last_kernel()

    def small(lo, hi):
        xs = x[:, :, lo:hi].contiguous()  # stride 1, padding (k - 1) / 2: the cut's output has the cut's rows, and so has its residual
        return F.conv_norm_act(xs, wd, None, ad, bd, residual=xs, groups=groups, affine="fma", activation="relu6")

    def oracle(lo, hi):
        xs = x[:, :, lo:hi].cpu().numpy()
        return ref.conv2d_affine_act(xs, wt, None, alpha, beta, xs, 1, halo, groups, 2, "relu6")

    conv_rows_case(n, c, c, h, w, y, small, oracle, halo, 2048, ("input element 2^31", "output element 2^31"))


def test_conv_norm_act_small_cin_3x3_output_past_2_31_elements():
    n, cin, cout, h, w = 2, 4, 8, CNA_H, CNA_W
    x = L.fill(torch.empty((n, cin, h, w), device="cuda"), 410)
    res = L.fill(torch.empty((n, cout, h, w), device="cuda"), 411)
    wt = (philox_f32(412, (cout, cin, 3, 3)) - 0.5) * 0.5
    bias = philox_f32(413, (cout,)) - 0.5
    alpha, beta = _cna_terms(cout, 414)
    wd, bsd, ad, bd = dev(wt), dev(bias), dev(alpha), dev(beta)
    y = nans((n, cout, h, w))
    p = _lib.ptr
    _lib.launch(_lib.load().mv_conv_norm_act_f32, x, 0, x.data_ptr(), wd.data_ptr(), p(bsd), p(ad), p(bd), res.data_ptr(), y.data_ptr(),
                n, cin, h, w, cout, 1, 1, 3)  # affine mul_add, hardswish
    assert _lib.last_kernel() == "k_conv3x3_smallcin", _lib.last_kernel()

    def small(lo, hi):
        return F.conv_norm_act(x[:, :, lo:hi].contiguous(), wd, bsd, ad, bd, residual=res[:, :, lo:hi].contiguous(), affine="mul_add",
                               activation="hardswish")

    def oracle(lo, hi):
        return ref.conv2d_affine_act(x[:, :, lo:hi].cpu().numpy(), wt, bias, alpha, beta, res[:, :, lo:hi].cpu().numpy(), 1, 1, 1, 1, "hardswish")

    conv_rows_case(n, cin, cout, h, w, y, small, oracle, 1, 1024, ("output element 2^31", "input byte 2^32"))


def test_conv1x1_upsample_add_past_2_31_elements():
    from tests import _fpn_ref as FR
    n, c, h, w = 2, 8, CNA_H, CNA_W
    th, tw = h // 2, w // 2
    assert h % 2 == 0 and w % 2 == 0
    x = L.fill(torch.empty((n, c, h, w), device="cuda"), 420)
    top = L.fill(torch.empty((n, c, th, tw), device="cuda"), 421)
    wt = philox_f32(422, (c, c)) - 0.5
    bias = philox_f32(423, (c,)) - 0.5
    wd, bsd = dev(wt.reshape(c, c, 1, 1)), dev(bias)
    assert F.conv1x1_k_slices(n, c, h, w, c)[0] == 1
    y = nans((n, c, h, w))
    _lib.launch(_lib.load().mv_conv1x1_upsample_add_f32, x, x.data_ptr(), wd.data_ptr(), bsd.data_ptr(), None, None, top.data_ptr(),
                y.data_ptr(), n, c, h, w, c, th, tw, 0, 0)
    assert _lib.last_kernel().startswith("k_conv1x1_up<"), _lib.last_kernel()

    def small(lo, hi):  # even cuts: rows lo .. hi - 1 read top rows lo / 2 .. hi / 2 - 1
        return F.conv1x1_upsample_add(x[:, :, lo:hi].contiguous(), wd, bsd, top=top[:, :, lo // 2:hi // 2].contiguous())

    def oracle(lo, hi):
        return FR.oracle_lateral(x[:, :, lo:hi].cpu().numpy(), wt, bias, None, None, top[:, :, lo // 2:hi // 2].cpu().numpy(), 0, None,
                                 slice_len=0)

    conv_rows_case(n, c, c, h, w, y, small, oracle, 0, 2048, ("input element 2^31", "output element 2^31"), even=True)


def test_conv_norm_act_pointwise_batch_at_the_grid_limit():
    """n = 65535, the most images the pointwise kernel's grid takes (65536 is refused: tests/test_fpn_host.py), at 3 x 3 pixels."""
    n, c, h, w = 65535, 8, 3, 3
    x = L.fill(torch.empty((n, c, h, w), device="cuda"), 430)
    res = L.fill(torch.empty((n, c, h, w), device="cuda"), 431)
    wt = philox_f32(432, (c, c, 1, 1)) - 0.5
    alpha, beta = _cna_terms(c, 433)
    wd, ad, bd = dev(wt), dev(alpha), dev(beta)
    y = nans((n, c, h, w))
    p = _lib.ptr
    _lib.launch(_lib.load().mv_conv_norm_act_f32, x, 2, x.data_ptr(), wd.data_ptr(), None, p(ad), p(bd), res.data_ptr(), y.data_ptr(),
                n, c, h, w, c, 1, 2, 1)
    assert _lib.last_kernel().startswith("k_conv1x1<"), _lib.last_kernel()
    for a, b in ((0, 64), (n - 64, n)):
        slices, sl = F.conv1x1_k_slices(n, c, h, w, c)
        want = ref.conv2d_affine_act(x[a:b].cpu().numpy(), wt, None, alpha, beta, res[a:b].cpu().numpy(), 1, 0, 1, 2, "relu",
                                     slice_len=sl if slices > 1 else 0)
        np.testing.assert_array_equal(y[a:b].cpu().numpy(), want)
    assert F.conv1x1_k_slices(n, c, h, w, c)[0] == 1
    for a in range(0, n, 8192):
        b = min(a + 8192, n)
        assert F.conv1x1_k_slices(b - a, c, h, w, c)[0] == 1
        assert equal_on_device(y[a:b], F.conv_norm_act(x[a:b], wd, None, ad, bd, residual=res[a:b], affine="fma", activation="relu"))


# ---- warp, resize, resized_crop, the classification preset: planes * h * w past 2^31 ------------------------------------------------------
# These go through the Python API, which allocates its own output: there is no sentinel, and an element that was not written
# shows only as a difference from the band's own launch.
def independent_planes_case(x, y, small, reference, compare, need):
    """x (planes, ...) -> y (planes, ...): output plane i depends on input plane i alone.  reference(x planes on the host) is
    compared with compare(got, want); small(x planes on the device) is the op's own launch on a band."""
    planes, xe, ye = x.shape[0], x[0].numel(), y[0].numel()
    picks = L.pick_rows(1, planes, xe, x.element_size(), planes, ye, y.element_size())
    what = L.assert_crossings_straddled(picks, L.cut_same, 1, planes, xe, x.element_size(), planes, ye, y.element_size(), need)
    for a, b in picks[0]:
        compare(y[a:b], reference(x[a:b].cpu()), f"planes [{a}, {b}); {what}")
    band = 2 ** 30 // max(xe * x.element_size(), ye * y.element_size())
    for a in range(0, planes, band):
        b = min(a + band, planes)
        a = max(b - band, 0)  # the last band is as long as the others (it overlaps its neighbour): no launch on a handful of planes
        assert torch.equal(y[a:b], small(x[a:b])), f"planes [{a}, {b}) differ from the band's own launch"


def _exact(got, want, what):
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=what)


@pytest.mark.parametrize("dtype,mode", [(torch.uint8, "bilinear"), (torch.float32, "nearest"), (torch.float32, "bilinear")], ids=str)
def test_warp_planes_past_2_31_elements(dtype, mode):
    from tests.test_gpu_warp import assert_matches_reference, ref_affine
    h, w = 135, 240
    planes = 2 ** 31 // (h * w) + 3
    x = L.fill(torch.empty((planes, 1, h, w), dtype=dtype, device="cuda"), 500, 0, 256 if dtype == torch.uint8 else 1)
    args = (17.0, [5, -3], 1.1, [4.0, 2.0])
    y = F.affine(x, *args, interpolation=mode, fill=[0.25 if dtype == torch.float32 else 7])
    assert _lib.last_kernel().startswith("k_warp<" + ("u8" if dtype == torch.uint8 else "f32")), _lib.last_kernel()
    fill = [0.25 if dtype == torch.float32 else 7]
    independent_planes_case(x, y, lambda xs: F.affine(xs, *args, interpolation=mode, fill=fill),
                            lambda xs: ref_affine(xs, *args, mode=mode, fill=fill), assert_matches_reference,
                            ("input element 2^31", "output element 2^31"))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("h,w,size,need", [(135, 240, [68], "input element 2^31"), (30, 40, [60], "output element 2^31")], ids=["down", "up"])
def test_resize_planes_past_2_31_elements(h, w, size, need, dtype):
    from cpu_vision_amd import functional_v1 as F1
    oh, ow = ref.resized_output_size(h, w, size)
    planes = 2 ** 31 // max(h * w, oh * ow) + 3
    x = L.fill(torch.empty((planes, h, w), dtype=dtype, device="cuda"), 510, 0, 256 if dtype == torch.uint8 else 255)
    y = F1.resize(x, size)
    assert y.shape == (planes, oh, ow) and _lib.last_kernel().startswith("k_resize"), (y.shape, _lib.last_kernel())
    independent_planes_case(x, y, lambda xs: F1.resize(xs, size), lambda xs: ref.resize(xs.numpy(), size), _exact, (need,))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_resized_crop_planes_past_2_31_elements(dtype):
    from tests import _crop_ref as CR
    from tests.test_gpu_warp import assert_matches_reference
    h, w = 135, 240
    planes = 2 ** 31 // (h * w) + 3
    x = L.fill(torch.empty((planes, 1, h, w), dtype=dtype, device="cuda"), 520, 0, 256 if dtype == torch.uint8 else 1)
    args = (10, 20, 100, 180, [64, 96])
    y = F.resized_crop(x, *args)
    assert _lib.last_kernel().startswith("k_resize"), _lib.last_kernel()
    independent_planes_case(x, y, lambda xs: F.resized_crop(xs, *args), lambda xs: CR.resized_crop_image(xs, *args),
                            assert_matches_reference, ("input element 2^31",))


def test_preset_classification_batch_past_2_31_elements():
    from cpu_vision_amd.presets import ImageClassification
    h, w = 135, 240
    n = 2 ** 31 // (3 * h * w) + 3
    x = L.fill(torch.empty((n, 3, h, w), dtype=torch.uint8, device="cuda"), 530, 0, 256)
    pre = ImageClassification(crop_size=56, resize_size=64)
    y = pre(x)
    assert y.shape == (n, 3, 56, 56) and y.dtype == torch.float32
    independent_planes_case(x, y, pre, lambda xs: ref.image_classification_preset(xs.numpy(), 56, 64, MEAN, STD), _exact,
                            ("input element 2^31",))


# ---- rpn_topk / rpn_decode: the second image of every level more than 2^31 elements after the first ---------------------------------------
def test_rpn_image_stride_past_2_31_elements():
    """The entries take the distance between the images of a map, so the maps themselves stay small: every level's logits and
    deltas are views into ONE buffer of a little more than 2^31 floats, image 0 at its start and image 1 past element 2^31.  The
    values and the restatement are those of tests/test_gpu_rpn.py::test_decode_equals_the_restatement."""
    from tests import _rpn_ref as P
    from tests.test_gpu_rpn import CLIP, SIZES, STRIDES, _decode_inputs, _restatement
    ob, dl = _decode_inputs(8200)
    stride = 2 ** 31 + 4099  # elements from image 0 to image 1 of every map
    room = sum(m[0].numel() for m in ob + dl)
    buf = torch.empty(stride + room, device="cuda")
    views, off = [], 0
    for m in ob + dl:
        _, c, h, w = m.shape
        v = torch.as_strided(buf, (2, c, h, w), (stride, h * w, w, 1), off)
        v.copy_(m.cuda())
        assert v.stride(0) == stride and v[1].data_ptr() - buf.data_ptr() >= 2 ** 33  # image 1: past element 2^31, byte 2^33
        views.append(v)
        off += c * h * w
    dob, ddl = views[:len(ob)], views[len(ob):]
    m = _restatement()
    want = m.from_head_outputs(P.ImageList(torch.zeros(2, 3, 64, 96), SIZES), ob, dl, detailed=True)
    idx = F.rpn_topk(dob, 4096)
    assert _lib.last_kernel() == "k_rpn_topk<levels3,k4096>", _lib.last_kernel()
    assert torch.equal(idx.cpu(), want["idx"].to(torch.int32))
    assert torch.equal(idx, F.rpn_topk([o.cuda() for o in ob], 4096)), "differs from the launch on dense maps"
    got = F.rpn_decode(dob, ddl, idx, m.anchor_generator.cell_anchors, STRIDES, SIZES, (1.0, 1.0, 1.0, 1.0), CLIP, 1e-3, 0.0)
    assert _lib.last_kernel() == "k_rpn_decode<levels3>"
    P.same(got[0], want["boxes"], "boxes")
    P.same(got[1], want["scores"], "scores")
    assert torch.equal(got[2].cpu(), want["levels"]) and torch.equal(got[3].cpu(), want["valid"])
    dense = F.rpn_decode([o.cuda() for o in ob], [d.cuda() for d in dl], idx, m.anchor_generator.cell_anchors, STRIDES, SIZES,
                         (1.0, 1.0, 1.0, 1.0), CLIP, 1e-3, 0.0)
    for a, b in zip(got, dense):  # NaN boxes and scores are part of the inputs: compare the bits
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ---- conv2d, implicit GEMM (mv_conv2d_bias_act_f32 / mv_conv2d_affine_act_f32) ----------------------------------------------------------------
def test_conv2d_implicit_gemm_one_image_just_below_2_30_elements():
    """The implicit kernel addresses an image with 32-bit byte offsets and refuses one of 2^30 elements (tests/test_conv2d_abi_host.py).
    357 channels of 1000000 x 3 pixels are 2741824 elements short of it: the offsets of the last channels lie in [2^31, 2^32).  The
    shape keeps the output plane (999998 x 1) and K (3213) inside the kernel's ranges and a row of all channels at 4 KB for the oracle."""
    cin, cout, h, w = 357, 8, 1000000, 3
    oh = h - 2
    assert 2 ** 30 - 2 ** 22 < cin * h * w < 2 ** 30 and oh < 2 ** 20
    lib = _lib.load()
    assert lib.mv_conv2d_needs_workspace(1, cin, cout, h, w, 3, 3, 1, 1, 0, 0, 1, 1, 1) == 0
    x = L.fill(torch.empty((1, cin, h, w), device="cuda"), 600)
    wt = (philox_f32(601, (cout, cin, 3, 3)) - 0.5) * 0.05
    bias = philox_f32(602, (cout,)) + 0.5
    wd, bd = dev(wt), dev(bias)
    y = nans((1, cout, oh, 1))
    _lib.launch(lib.mv_conv2d_bias_act_f32, x, x.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), 1, cin, h, w, cout, 3, 3, 1, 1, 0, 0,
                1, 1, 1, 1, None, 0)
    assert "implicit" in _lib.last_kernel(), _lib.last_kernel()
    rows = {0, 1, oh - 2, oh - 1}
    xc = L.crossings(x.numel(), 4)
    assert list(xc) == ["byte 2^31"] and not L.crossings(y.numel(), 4)
    for e in xc.values():
        for r in L.rows_near(e, w, h, reach=0):
            rows.update(o for o in range(r - 2, r + 1) if 0 <= o < oh)  # output row o reads input rows o .. o + 2
    in_ranges = []
    for a, b in L.strips(rows):
        in_ranges += L.plane_ranges(range(cin), h, w, a, b + 2)
    for name, e in xc.items():
        L.assert_straddles(in_ranges, e, "input " + name)
    what = f"input {L.describe(in_ranges, 4)}"
    for a, b in L.strips(rows):
        want = ref.conv2d_affine_act(x[:, :, a:b + 2].cpu().numpy(), wt, bias, None, None, None, 1, 0, 1, 0, "relu")
        np.testing.assert_array_equal(y[:, :, a:b].cpu().numpy(), want, err_msg=f"rows [{a}, {b}); {what}")
    band = 250000
    for a in range(0, oh, band):
        b = min(a + band, oh)
        assert cin * (b + 2 - a) * w * 4 < L.B31
        yb = F.conv2d_bias_act(x[:, :, a:b + 2].contiguous(), wd, bd, activation="relu")
        assert "implicit" in _lib.last_kernel()
        assert equal_on_device(y[:, :, a:b], yb), f"rows [{a}, {b}) differ from the band's own launch"


def test_conv2d_implicit_gemm_batch_past_2_31_elements():
    n, cin, cout, h, w = 2 ** 31 // (3 * 110 * 110) + 3, 3, 8, 110, 110
    assert n <= 65535 and n * cin * h * w > 2 ** 31
    x = L.fill(torch.empty((n, cin, h, w), device="cuda"), 610)
    wt = (philox_f32(611, (cout, cin, 5, 5)) - 0.5) * 0.2
    bias = philox_f32(612, (cout,)) - 0.5
    alpha, beta = _cna_terms(cout, 613)
    wd, bsd, ad, bd = dev(wt), dev(bias), dev(alpha), dev(beta)
    run = lambda xs: F.conv2d_affine_act(xs, wd, bsd, ad, bd, None, stride=2, padding=2, affine="fma", activation="relu")  # noqa: E731
    lib = _lib.load()
    assert lib.mv_conv2d_needs_workspace(n, cin, cout, h, w, 5, 5, 2, 2, 2, 2, 1, 1, 1) == 0
    y = nans((n, cout, 55, 55))
    _lib.launch(lib.mv_conv2d_affine_act_f32, x, x.data_ptr(), wd.data_ptr(), bsd.data_ptr(), ad.data_ptr(), bd.data_ptr(), None, y.data_ptr(),
                n, cin, h, w, cout, 5, 5, 2, 2, 2, 2, 1, 1, 1, 2, 1, None, 0)
    assert "implicit" in _lib.last_kernel(), _lib.last_kernel()
    assert _no_nan(y)
    independent_planes_case(x, y, run, lambda xs: ref.conv2d_affine_act(xs.numpy(), wt, bias, alpha, beta, None, 2, 2, 1, 2, "relu"), _exact,
                            ("input element 2^31", "output byte 2^32"))


# ---- the fused InvertedResidual block ---------------------------------------------------------------------------------------------------
def test_inverted_residual_batch_past_2_31_elements():
    """24 -> 144 -> 24 on 56 x 56 maps with `+ x` (k_invres_wide, the fewest channels among the fused shapes of MobileNetV2 whose
    input and output are equally large).  From 64 images up the plan is one chain per output (mv_inverted_residual_k_slices), for the
    whole batch and for every band alike; the oracle composes the three convolutions in that order on the compared images."""
    from cpu_vision_amd.mobilenet import InvertedResidual
    from tests._util import oracle_conv_block, randomize_norms
    cin, hw = 24, 56
    n = 2 ** 31 // (cin * hw * hw) + 3
    assert F.inverted_residual_k_slices(n, cin, 6 * cin, cin, hw, hw, 1) == (1, 6 * cin)
    torch.manual_seed(7)
    cpu_block = InvertedResidual(cin, cin, 1, 6).eval()
    randomize_norms(cpu_block, 8)
    block = InvertedResidual(cin, cin, 1, 6).eval()
    block.load_state_dict(cpu_block.state_dict())
    block = block.cuda()
    x = L.fill(torch.empty((n, cin, hw, hw), device="cuda"), 700)

    def run(xs):
        assert F.inverted_residual_k_slices(xs.shape[0], cin, 6 * cin, cin, hw, hw, 1)[0] == 1
        with torch.no_grad():
            return block(xs)

    def oracle(xs):
        blocks = list(cpu_block.conv)
        a = xs = xs.numpy()
        for blk in blocks[:-2]:
            a = oracle_conv_block(ref, a, blk[0], blk[1], "relu6", slice_len=0)
        return oracle_conv_block(ref, a, blocks[-2], blocks[-1], None, xs, slice_len=0)

    y = run(x)
    assert _lib.last_kernel().startswith("k_invres_wide<56,s1,"), _lib.last_kernel()
    independent_planes_case(x, y, run, oracle, _exact, ("input element 2^31", "output element 2^31"))


# ---- deform_conv2d: the fused kernel, and the columns passes through a capped workspace -------------------------------------------------------
def per_image_case(inputs, y, small, reference, need):
    """Several per-image inputs (n, ...) -> y (n, ...), image i of y from image i of every input.  small(a, b) / reference(a, b): the op on
    images [a, b) on the device / the oracle on the host.  The images compared with the reference lie around every boundary that
    any input or the output crosses."""
    n, ye = y.shape[0], y[0].numel()
    images, crossed = set(), []
    for k, t in enumerate(inputs):
        te = t[0].numel()
        picks = L.pick_rows(1, n, te, 4, n, ye, 4, reach=0)  # the image that holds the boundary, the first and the last
        L.assert_crossings_straddled(picks, L.cut_same, 1, n, te, 4, n, ye, 4)
        crossed += [f"input {k} {name}" for name in L.crossings(t.numel(), 4)]
        images.update(i for a, b in picks[0] for i in range(a, b))
    crossed += [f"output {name}" for name in L.crossings(y.numel(), 4)]
    assert all(k in crossed for k in need), (need, crossed)
    for a, b in L.strips(images):
        np.testing.assert_array_equal(y[a:b].cpu().numpy(), reference(a, b), err_msg=f"images [{a}, {b}); crossed {crossed}")
    band = 2 ** 30 // (4 * max([ye] + [t[0].numel() for t in inputs]))
    for a in range(0, n, band):
        b = min(a + band, n)
        a = max(b - band, 0)
        assert torch.equal(y[a:b], small(a, b)), f"images [{a}, {b}) differ from the band's own launch"


def test_deform_conv2d_fused_batch_past_2_31_elements():
    """64 -> 64 channels on 28 x 28 maps, 3 x 3, with a mask: the fewest channels at which input, output, offsets (18 planes per image)
    and mask (9) fit the memory cap together.  No sentinel: ops.deform_conv2d allocates the output."""
    c, hw = 64, 28
    n = 2 ** 31 // (c * hw * hw) + 3
    assert _lib.load().mv_deform_conv2d_needs_workspace(n, c, c, hw, hw, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1) == 0
    x = L.fill(torch.empty((n, c, hw, hw), device="cuda"), 800)
    off = L.fill(torch.empty((n, 18, hw, hw), device="cuda"), 801, -3.0, 3.0)
    mask = L.fill(torch.empty((n, 9, hw, hw), device="cuda"), 802, 0.0, 1.0)
    wt = (philox_f32(803, (c, c, 3, 3)) - 0.5) * 0.1
    bias = philox_f32(804, (c,)) - 0.5
    wd, bd = dev(wt), dev(bias)
    run = lambda a, b: ops.deform_conv2d(x[a:b], off[a:b], wd, bd, padding=1, mask=mask[a:b])  # noqa: E731
    y = run(0, n)
    assert _lib.last_kernel().startswith("k_deform_fused<"), _lib.last_kernel()
    per_image_case([x, off, mask], y, run,
                   lambda a, b: ref.deform_conv2d(x[a:b].cpu().numpy(), off[a:b].cpu().numpy(), wt, bias, (1, 1), (1, 1), (1, 1), mask[a:b].cpu().numpy()),
                   ("input 0 element 2^31", "input 1 byte 2^31", "output element 2^31"))


def test_deform_conv2d_columns_passes_input_past_2_31_elements(monkeypatch):
    """A geometry without a fused kernel (stride 9 on 200 x 200 maps): the columns form, its workspace capped at 64 MiB so that the
    batch runs in passes of 440 images.  Only the input passes 2^31 elements (the output is 23 x 23 per channel)."""
    cin, cout, hw = 8, 8, 200
    n = 2 ** 31 // (cin * hw * hw) + 3
    lib = _lib.load()
    assert lib.mv_deform_conv2d_needs_workspace(n, cin, cout, hw, hw, 3, 3, 9, 9, 1, 1, 1, 1, 1, 1) == 1
    per_image = int(lib.mv_deform_conv2d_workspace_bytes(1, cin, hw, hw, 3, 3, 9, 9, 1, 1, 1, 1))
    monkeypatch.setattr(ops, "MAX_WORKSPACE_BYTES", 64 << 20)
    assert 8 < n * per_image // (64 << 20)  # more than 8 passes
    ohw = (hw + 2 - 3) // 9 + 1
    x = L.fill(torch.empty((n, cin, hw, hw), device="cuda"), 810)
    off = L.fill(torch.empty((n, 18, ohw, ohw), device="cuda"), 811, -3.0, 3.0)
    wt = (philox_f32(812, (cout, cin, 3, 3)) - 0.5) * 0.3
    wd = dev(wt)
    run = lambda a, b: ops.deform_conv2d(x[a:b], off[a:b], wd, None, stride=9, padding=1)  # noqa: E731
    asked, real_workspace = [], _lib.workspace
    monkeypatch.setattr(_lib, "workspace", lambda nbytes, device: asked.append(nbytes) or real_workspace(nbytes, device))
    y = run(0, n)
    # the workspace the wrapper passed holds `images` whole images, and the library runs the batch in passes of that many
    images = asked[-1] // per_image
    assert asked[-1] == _lib.columns_workspace_bytes(n, per_image, 64 << 20) <= 64 << 20 and asked[-1] % per_image == 0
    assert 0 < images < n and -(-n // images) == 16, (asked, images)
    assert "k_deform_im2col" in _lib.last_kernel() or "k_conv1x1" in _lib.last_kernel(), _lib.last_kernel()
    per_image_case([x, off], y, run,
                   lambda a, b: ref.deform_conv2d(x[a:b].cpu().numpy(), off[a:b].cpu().numpy(), wt, None, (9, 9), (1, 1), (1, 1), None),
                   ("input 0 element 2^31",))


def test_masks_to_boxes_tallest_mask_one_launch_takes():
    """One workgroup per 32-row chunk and fewer than 2^32 threads in a grid: 32 (2^24 - 1) rows are the most one mask may have (one
    row more is refused: tests/test_boxes_host.py).  One uint8 mask of that height, one pixel wide, 512 MiB; the box is known from
    where the set pixels were put, the host sees nothing of the mask."""
    h = 32 * (2 ** 24 - 1)
    masks = torch.zeros((1, h, 1), dtype=torch.uint8, device="cuda")
    masks[0, 12345, 0] = 7
    masks[0, h - 1, 0] = 1  # the last row of the last chunk
    boxes = ops.masks_to_boxes(masks)
    assert "k_mtb_reduce<u8" in _lib.last_kernel(), _lib.last_kernel()
    assert np.float32(h - 1) != np.float32(h - 33)  # float32 tells the last two chunks apart at this height
    assert boxes.cpu().tolist() == [[0.0, 12345.0, 0.0, float(np.float32(h - 1))]]
    masks[0, h - 1, 0] = 0
    masks[0, h - 33, 0] = 1  # the last row of the chunk before
    assert ops.masks_to_boxes(masks).cpu().tolist() == [[0.0, 12345.0, 0.0, float(np.float32(h - 33))]]
    with pytest.raises(_lib.Mi355VisionError, match="launch grid"):
        ops.masks_to_boxes(torch.zeros((1, h + 1, 1), dtype=torch.uint8, device="cuda"))
