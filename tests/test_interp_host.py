"""F.interpolate / F.detection_batch and the detection transform's resize without a device: the oracle (tests/_interp_ref.py) against
torch's CPU interpolate -- bit for bit where torch takes its vectorised channels-first loop, within a derived bound where it takes
another -- the size rule against the shapes torch's interpolate returns, the argument errors, the refusals of the two entry points
with host pointers (they come before any launch) and the transform's behaviour on CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cpu_vision_amd as mv
from cpu_vision_amd import _lib
from cpu_vision_amd import functional as F
from cpu_vision_amd import transform as T
from tests import _interp_ref as R


def _image(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 4 - 2


def _torch_interp(x, oh, ow):
    return torch.nn.functional.interpolate(x, size=[oh, ow], mode="bilinear", align_corners=False)


# ---- the oracle and torch's CPU kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [4, 2])
@pytest.mark.parametrize("h,w,oh,ow", [(60, 90, 100, 150), (300, 200, 150, 100)])
def test_oracle_equals_torch_cpu_bit_for_bit(c, h, w, oh, ow):
    x = _image(100 + c, (1, c, h, w))
    assert torch.equal(R.bits(R.interpolate(x.numpy(), oh, ow)), R.bits(_torch_interp(x, oh, ow)))


@pytest.mark.skipif((os.cpu_count() or 1) < 2, reason="torch picks its channels-last kernel for 3 channels on one thread")
def test_oracle_equals_torch_cpu_three_channels_two_threads():
    x = _image(103, (1, 3, 120, 160))
    before = torch.get_num_threads()
    torch.set_num_threads(2)
    try:
        want = _torch_interp(x, 200, 267)
    finally:
        torch.set_num_threads(before)
    assert torch.equal(R.bits(R.interpolate(x.numpy(), 200, 267)), R.bits(want))


def _bound(h, w, x):
    """6 roundings of values no greater than max|x| (the weights are convex), each 2^-24 relative; and a `src` computed without the fma
    is off by at most 1 ulp(src) <= 2^-23 max(h, w), which shifts `lam` by as much and the value by that times |b - a| <= 2 max|x|, per
    axis: 2 axes x 2 x 2^-23 max(h, w) = 8 max(h, w) 2^-24."""
    return (6 + 8 * max(h, w)) * 2.0 ** -24 * float(x.abs().max())


@pytest.mark.parametrize("c,h,w,oh,ow,threads", [(2, 5, 7, 9, 13, None), (2, 37, 53, 24, 34, None), (3, 120, 160, 200, 267, 1)],
                         ids=["5x7-small-loop", "37x53-small-loop", "c3-one-thread-channels-last"])
def test_torch_cpu_other_loops_within_the_bound(c, h, w, oh, ow, threads):
    x = _image(110 + h, (1, c, h, w))
    before = torch.get_num_threads()
    if threads:
        torch.set_num_threads(threads)
    try:
        want = _torch_interp(x, oh, ow)
    finally:
        torch.set_num_threads(before)
    got = torch.from_numpy(R.interpolate(x.numpy(), oh, ow))
    worst = float((got.double() - want.double()).abs().max())
    print(f"{h}x{w}->{oh}x{ow} c={c}: max |torch - oracle| = {worst:.3e} = {worst / float(x.abs().max()):.3e} max|x|, bound {_bound(h, w, x):.3e}")
    assert worst <= _bound(h, w, x)


def test_oracle_fma_is_one_rounding():
    """a * b = 2^-14 - 2^-60 lies just below half an ulp of c = 1024 + 2^-13: the fma is c.  The float64 sum drops the 2^-60, lands ON
    the float32 tie and would then round to even, up."""
    a, b, c = np.float32(2.0 ** -7 + 2.0 ** -30), np.float32(2.0 ** -7 - 2.0 ** -30), np.float32(1024 + 2.0 ** -13)
    assert np.float64(a) * np.float64(b) == 2.0 ** -14 - 2.0 ** -60
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(1024 + 2.0 ** -12)  # rounded twice
    assert R.fma32(np.array([a, -a]), np.array([b, b]), np.array([c, -c], np.float32)).tolist() == [float(c), -float(c)]


# ---- the size rule -----------------------------------------------------------------------------------------------------------------------
SWEEP = ([(s, s) for s in (33, 64, 100, 201, 289, 305, 322, 480, 800, 1000)]
         + [(3 * k, 4 * k) for k in (11, 40, 107, 160, 250)] + [(4 * k, 3 * k) for k in (11, 125, 160)]
         + [(480, 640), (427, 640), (640, 480), (500, 375), (40, 56), (50, 37), (1, 7), (1200, 300)])


@pytest.mark.parametrize("min_size,max_size", [(800, 1333), (64, 96)])
def test_size_rule_equals_the_shape_torch_returns(min_size, max_size):
    for h, w in SWEEP:
        if max(h, w) * min(min_size / min(h, w), max_size / max(h, w)) > 1400:
            continue
        scale = min(float(min_size) / float(min(h, w)), float(max_size) / float(max(h, w)))
        want = tuple(torch.nn.functional.interpolate(torch.zeros(1, 1, h, w), scale_factor=scale, mode="bilinear", recompute_scale_factor=True,
                                                     align_corners=False).shape[-2:])
        assert T.resized_size(h, w, min_size, max_size) == want == R.resized_size(h, w, min_size, max_size), (h, w)
        assert tuple(F.interpolate_output_size((h, w), scale_factor=scale)) == want


def test_size_rule_is_the_eager_branch():
    """289, 305 and 322 squares at 800 / 1333 become 799, not 800, in Python floats too (s * (800 / s) < 800); 201 x 201 is 800 with the
    scale in Python floats and 799 with the scripted branch's float32 scale, and 20 x 31 at 64 / 96 differs likewise."""
    for s in (289, 305, 322):
        assert T.resized_size(s, s, 800, 1333) == (799, 799)
    assert T.resized_size(201, 201, 800, 1333) == (800, 800) and R.scripted_resized_size(201, 201, 800, 1333) == (799, 799)
    assert T.resized_size(20, 31, 64, 96) == (61, 96) and R.scripted_resized_size(20, 31, 64, 96) == (61, 95)
    assert T.resized_size(480, 640, 800, 1333) == (800, 1066) and T.resized_size(300, 1200, 800, 1333) == (333, 1333)


def test_size_rule_fixed_size():
    assert T.resized_size(480, 640, 800, 1333, fixed_size=(320, 200)) == (200, 320) == R.resized_size(480, 640, 800, 1333, (320, 200))
    t = mv.GeneralizedRCNNTransform(800, 1333, [0.0] * 3, [1.0] * 3, fixed_size=(320, 200))
    assert t.fixed_size == (320, 200) and t._skip_resize is False
    assert F.interpolate_output_size((5, 7), size=[9, 13]) == [9, 13] and F.interpolate_output_size((5, 7), size=4) == [4, 4]
    assert F.interpolate_output_size((5, 7), scale_factor=(2.0, 1.5)) == [10, 10]


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------
def test_interpolate_argument_errors():
    x = torch.zeros(1, 3, 8, 8)
    for kw, name in ((dict(size=[4, 4], mode="nearest"), "mode"), (dict(size=[4, 4], mode="bicubic"), "mode"),
                     (dict(size=[4, 4], align_corners=True), "align_corners"), (dict(size=[4, 4], antialias=True), "antialias"),
                     (dict(scale_factor=2.0), "scale_factor"), (dict(scale_factor=2.0, recompute_scale_factor=False), "scale_factor")):
        with pytest.raises(NotImplementedError, match=name):
            F.interpolate(x, **kw)
    with pytest.raises(NotImplementedError, match="dtype"):
        F.interpolate(x.double(), size=[4, 4])
    with pytest.raises(NotImplementedError, match="dimensions"):
        F.interpolate(x[0], size=[4, 4])
    with pytest.raises(ValueError, match="only one of size or scale_factor"):
        F.interpolate(x, size=[4, 4], scale_factor=2.0, recompute_scale_factor=True)
    with pytest.raises(ValueError, match="either size or scale_factor"):
        F.interpolate(x)
    with pytest.raises(ValueError, match="greater than 0"):
        F.interpolate(x, scale_factor=0.01, recompute_scale_factor=True)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.interpolate(x, size=[4, 4])
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.interpolate(x, scale_factor=1.5, recompute_scale_factor=True)


def test_detection_batch_argument_errors():
    img = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="empty list"):
        F.detection_batch([], [], [0.0] * 3, [1.0] * 3)
    with pytest.raises(ValueError, match="1 images and 2 sizes"):
        F.detection_batch([img], [(8, 8), (8, 8)], [0.0] * 3, [1.0] * 3)
    with pytest.raises(ValueError, match="list of 3d tensors"):
        F.detection_batch([img[None]], [(8, 8)], [0.0] * 3, [1.0] * 3)
    with pytest.raises(TypeError, match="float32"):
        F.detection_batch([img.double()], [(8, 8)], [0.0] * 3, [1.0] * 3)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.detection_batch([img], [(8, 8)], [0.0] * 3, [1.0] * 3)


# ---- the entry points refuse before any launch ------------------------------------------------------------------------------------
def _ints(v):
    return (C.c_int * len(v))(*v)


def test_interpolate_abi_refusals_without_a_device():
    lib = _lib.load()
    x = np.zeros((2, 4, 4), np.float32)
    y = np.zeros((2, 8, 8), np.float32)
    xp, yp = x.ctypes.data, y.ctypes.data

    def call(**o):
        a = {**dict(x=xp, y=yp, planes=2, h=4, w=4, oh=8, ow=8), **o}
        return lib.mv_interpolate_bilinear_f32(a["x"], a["y"], a["planes"], a["h"], a["w"], a["oh"], a["ow"], None)
    for over, text in ((dict(x=None), "null pointer"), (dict(y=None), "null pointer"), (dict(h=0), "bad shape"), (dict(w=-1), "bad shape"),
                       (dict(oh=0), "bad shape"), (dict(ow=0), "bad shape"), (dict(planes=-1), "bad shape"), (dict(y=xp), "must not overlap"),
                       (dict(y=xp + 64), "must not overlap")):
        assert call(**over) == -1 and text in lib.mv_last_error().decode(), (over, lib.mv_last_error())
    assert call(planes=0, x=None, y=None) == 0
    assert call(planes=2 ** 40, oh=2 ** 20, ow=2 ** 20, y=xp + 2 ** 50) < 0  # exceeds the address space or the grid
    assert not y.any()


def test_detection_batch_abi_refusals_without_a_device():
    lib = _lib.load()
    imgs = [np.zeros((3, 4, 6), np.float32), np.zeros((3, 5, 5), np.float32)]
    y = np.zeros((2, 3, 8, 12), np.float32)
    mean, std = _lib.taps([0.5] * 3), _lib.taps([0.25] * 3)

    def call(**o):
        a = {**dict(xs=[i.ctypes.data for i in imgs], hs=[4, 5], ws=[6, 5], ohs=[8, 8], ows=[12, 8], n=2, c=3, mean=mean, std=std, y=y.ctypes.data,
                    hp=8, wp=12), **o}
        xs = None if a["xs"] is None else (C.c_void_p * len(a["xs"]))(*a["xs"])
        tables = [None if a[k] is None else _ints(a[k]) for k in ("hs", "ws", "ohs", "ows")]
        return lib.mv_detection_batch_f32(xs, *tables, a["n"], a["c"], a["mean"], a["std"], a["y"], a["hp"], a["wp"], None)
    cases = ((dict(xs=None), -1, "null pointer"), (dict(hs=None), -1, "null pointer"), (dict(ows=None), -1, "null pointer"), (dict(mean=None), -1, "null pointer"),
             (dict(std=None), -1, "null pointer"), (dict(y=None), -1, "null pointer"), (dict(xs=[imgs[0].ctypes.data, None]), -1, "null pointer (image 1)"),
             (dict(n=-1), -1, "bad shape"), (dict(c=0), -1, "bad shape"), (dict(hp=0), -1, "bad shape"), (dict(wp=-3), -1, "bad shape"),
             (dict(c=17), -2, "up to 16 channels"), (dict(hs=[4, 0]), -1, "bad size"), (dict(ows=[12, 0]), -1, "bad size"),
             (dict(ohs=[9, 8]), -1, "does not fit the batch"), (dict(ows=[12, 13]), -1, "does not fit the batch"),
             (dict(std=_lib.taps([0.25, 0.0, 0.25])), -1, "std evaluated to zero"), (dict(y=imgs[1].ctypes.data), -1, "must not overlap"))
    for over, rc, text in cases:
        assert call(**over) == rc and text in lib.mv_last_error().decode(), (over, lib.mv_last_error())
    assert call(n=0, xs=None, y=None) == 0
    assert not y.any()


# ---- the transform on CPU tensors ----------------------------------------------------------------------------------------------------------
def test_transform_resize_on_the_host():
    t = mv.GeneralizedRCNNTransform(64, 96, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    with pytest.raises(NotImplementedError, match="non-antialiased bilinear interpolate runs on the device only"):
        t.resize(torch.zeros(3, 8, 8))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        t([torch.zeros(3, 8, 8)])
    with pytest.raises(ValueError, match="list of 3d tensors"):
        t([torch.zeros(3, 8, 8), torch.zeros(1, 3, 8, 8)])
    with pytest.raises(TypeError, match="floating type"):
        t([torch.zeros(3, 8, 8, dtype=torch.uint8)])
    with pytest.raises(TypeError, match="float32"):
        t([torch.zeros(3, 8, 8, dtype=torch.float64)])
    skip = mv.GeneralizedRCNNTransform(64, 96, [0.0] * 3, [1.0] * 3, _skip_resize=True)
    image = torch.zeros(3, 8, 8)
    assert skip.resize(image) is image
    assert "resized_size" in T.__all__


# ---- the helpers of the large-offset test ------------------------------------------------------------------------------------------------
def test_torch_fma_and_the_separable_form_equal_the_oracle():
    """tests/test_gpu_interp_large.py compares the whole 2^31-element output with fma32_torch(wy0, T[y0], wy1 * T[y1]), T the rows
    interpolated along x only: the same bits as the oracle, here at 7 x 9 -> 40 x 33."""
    g = np.random.Generator(np.random.Philox(77))
    a, b, c = (g.standard_normal(4096).astype(np.float32) for _ in range(3))
    a[:2], b[:2], c[:2] = np.float32(2.0 ** -7 + 2.0 ** -30), np.float32(2.0 ** -7 - 2.0 ** -30), [np.float32(1024 + 2.0 ** -13), np.float32(3)]
    got = R.fma32_torch(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c))
    assert torch.equal(R.bits(got), R.bits(R.fma32(a, b, c))) and got[0] == float(np.float32(1024 + 2.0 ** -13))
    x = (g.random((2, 7, 9), dtype=np.float32) * 4 - 2)
    want = torch.from_numpy(R.interpolate(x, 40, 33))
    t = torch.from_numpy(R.interpolate(x, 7, 33))
    y0, y1, wy0, wy1 = (torch.from_numpy(v) for v in R.axis_taps(7, 40))
    top, bot = t[:, y0], t[:, y1]
    sep = R.fma32_torch(wy0[:, None].expand_as(top), top, wy1[:, None] * bot)
    assert torch.equal(R.bits(sep), R.bits(want))
    rows = np.array([0, 5, 39])
    assert np.array_equal(R.interpolate(x, 40, 33, rows=rows), want.numpy()[:, rows])
