"""F.affine / F.rotate / F.perspective and RandomAffine / RandomRotation / RandomPerspective host logic (no GPU): the C ABI's
argument checks, the registered kernels, the reference's argument errors, the host math (inverse matrix, rotate's expand
size, perspective coefficients), the rounding of the grid the kernel computes against the reference's CPU bmm, and the
transforms' seeded parameter draws.  Every check here runs before any device use."""
import ctypes
import math

import numpy as np
import pytest
import torch

from cpu_vision_amd import _lib, _pil, functional as F, transforms, tv_tensors
from cpu_vision_amd._registry import _get_kernel


IH, IW = 5, 7
FAKE_X, FAKE_Y = 0x10000, 0x20000


def _call(name, **over):
    """One mv_warp_* call whose arguments are valid except for `over`: it must be rejected before any launch (the pointers
    are fake)."""
    args = dict(x=FAKE_X, y=FAKE_Y, planes=6, channels=3, ih=IH, iw=IW, oh=IH + 2, ow=IW - 1, coeffs=_lib.taps([0.0] * 8),
                kind=0, order=1, mode=0, fill=None)
    args.update(over)
    lib = _lib.load()
    rc = getattr(lib, name)(args["x"], args["y"], args["planes"], args["channels"], args["ih"], args["iw"], args["oh"],
                            args["ow"], args["coeffs"], args["kind"], args["order"], args["mode"], args["fill"], None)
    return rc, lib.mv_last_error().decode()


@pytest.mark.parametrize("name", ["mv_warp_f32", "mv_warp_u8"])
@pytest.mark.parametrize("over,rc_want,msg", [
    (dict(ih=0), -1, "bad shape"),
    (dict(iw=-3), -1, "bad shape"),
    (dict(oh=0), -1, "bad shape"),
    (dict(ow=-1), -1, "bad shape"),
    (dict(planes=0), -1, "bad shape"),
    (dict(planes=-2), -1, "bad shape"),
    (dict(planes=7), -1, "multiple of channels"),
    (dict(channels=0), -1, "multiple of channels"),
    (dict(kind=2), -1, "unknown kind"),
    (dict(kind=-1), -1, "unknown kind"),
    (dict(order=2), -1, "unknown grid order"),
    (dict(mode=2), -1, "unknown mode"),
    (dict(mode=-1), -1, "unknown mode"),
    (dict(x=None), -1, "null pointer"),
    (dict(y=None), -1, "null pointer"),
    (dict(coeffs=None), -1, "null pointer"),
    (dict(y=FAKE_X), -1, "alias"),
    (dict(ih=65536, iw=65536), -2, "exceed 2^31"),
    (dict(oh=65536, ow=65536), -2, "exceed 2^31"),
    (dict(planes=17, channels=17, fill=_lib.taps([0.0] * 17)), -2, "up to 16 channels"),
])
def test_abi_rejects_bad_arguments_before_any_launch(name, over, rc_want, msg):
    rc, err = _call(name, **over)
    assert rc == rc_want and msg in err, (rc, err)


def test_abi_binding_declares_the_warp_entry_points():
    for name in ("mv_warp_f32", "mv_warp_u8"):
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == 14
    assert _lib.load().mv_abi_version() == 1


@pytest.mark.parametrize("fn", [F.affine, F.rotate, F.perspective], ids=lambda f: f.__name__)
def test_kernels_are_registered_for_every_input_type(fn):
    for t in (torch.Tensor, tv_tensors.Image, tv_tensors.Video, tv_tensors.Mask, tv_tensors.BoundingBoxes):
        assert _get_kernel(fn, t) is not None
    args = {F.affine: dict(angle=10.0, translate=[0, 0], scale=1.0, shear=[0.0, 0.0]), F.rotate: dict(angle=10.0),
            F.perspective: dict(startpoints=None, endpoints=None, coefficients=[1, 0, 0, 0, 1, 0, 0, 0])}[fn]
    with pytest.raises(NotImplementedError, match="BoundingBoxes"):
        fn(tv_tensors.BoundingBoxes(torch.zeros(2, 4)), **args)
    if _pil.PIL is not None:
        pic = _pil.PIL.Image.new("RGB", (IW, IH))
        with pytest.raises(NotImplementedError, match="PIL images are resampled by Pillow"):
            fn(pic, **args)


def test_reference_argument_errors_come_before_device_use():
    img = torch.zeros(3, IH, IW)
    with pytest.raises(TypeError, match="angle should be int or float"):
        F.affine(img, "10", [0, 0], 1.0, [0.0, 0.0])
    with pytest.raises(TypeError, match="translate should be a sequence"):
        F.affine(img, 10.0, 0, 1.0, [0.0, 0.0])
    with pytest.raises(ValueError, match="translate should be a sequence of length 2"):
        F.affine(img, 10.0, [0, 0, 0], 1.0, [0.0, 0.0])
    with pytest.raises(ValueError, match="scale should be positive"):
        F.affine(img, 10.0, [0, 0], 0.0, [0.0, 0.0])
    with pytest.raises(TypeError, match="Shear should be either"):
        F.affine(img, 10.0, [0, 0], 1.0, "x")
    with pytest.raises(ValueError, match="Shear should be a sequence containing two values"):
        F.affine(img, 10.0, [0, 0], 1.0, [1.0, 2.0, 3.0])
    with pytest.raises(TypeError, match="center should be a sequence"):
        F.affine(img, 10.0, [0, 0], 1.0, [0.0, 0.0], center=3)
    for fn, args in ((F.affine, (10.0, [0, 0], 1.0, [0.0, 0.0])), (F.rotate, (10.0,)),
                     (F.perspective, (None, None))):
        kw = dict(coefficients=[1, 0, 0, 0, 1, 0, 0, 0]) if fn is F.perspective else {}
        with pytest.raises(ValueError, match="Interpolation mode 'bicubic' is unsupported with Tensor input"):
            fn(img, *args, interpolation=transforms.InterpolationMode.BICUBIC, **kw)
        with pytest.raises(ValueError, match="Interpolation mode 'bicubic' is unsupported"):
            fn(img, *args, interpolation=3, **kw)  # Pillow's BICUBIC constant
        with pytest.raises(ValueError, match="InterpolationMode"):
            fn(img, *args, interpolation=1.5, **kw)
        with pytest.raises(ValueError, match="cannot broadcast to match the number of channels of the image: 2 != 3"):
            fn(img, *args, fill=[1.0, 2.0], **kw)
        with pytest.raises(ValueError, match="fill should be either int, float, tuple or list"):
            fn(img, *args, fill="white", **kw)
        with pytest.raises(NotImplementedError, match="float64"):
            fn(img.double(), *args, **kw)
    with pytest.raises(ValueError, match="shouldn't be defined concurrently"):
        F.perspective(img, [[0, 0]] * 4, [[0, 0]] * 4, coefficients=[0.0] * 8)
    with pytest.raises(ValueError, match="coefficients should have 8 float values"):
        F.perspective(img, None, None, coefficients=[0.0] * 7)
    with pytest.raises(ValueError, match="Either the startpoints/endpoints or the coefficients"):
        F.perspective(img, None, [[0, 0]] * 4)
    with pytest.raises(ValueError, match="exactly four corners, got 3 startpoints and 4 endpoints"):
        F.perspective(img, [[0, 0]] * 3, [[0, 0]] * 4)


@pytest.mark.parametrize("fill", [None, 0, 127, [10, 20, 30], (1.5,)])
@pytest.mark.parametrize("interpolation", ["bilinear", "nearest", transforms.InterpolationMode.NEAREST, 2])
def test_cpu_tensors_raise_like_every_other_kernel(fill, interpolation):
    """Valid arguments on host tensors: the library's no-CPU-fallback error, not a silent torch computation."""
    for img in (torch.zeros(3, IH, IW), torch.zeros(2, 3, IH, IW, dtype=torch.uint8)):
        for call in (lambda: F.affine(img, 10.0, [1, 2], 1.1, [3.0, 4.0], interpolation=interpolation, fill=fill),
                     lambda: F.rotate(img, 33.0, interpolation=interpolation, expand=True, fill=fill),
                     lambda: F.perspective(img, [[0, 0], [6, 0], [6, 4], [0, 4]], [[1, 0], [6, 1], [5, 4], [0, 3]],
                                           interpolation=interpolation, fill=fill)):
            with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
                call()


def test_empty_images_return_without_a_device():
    img = torch.zeros(0, 3, IH, IW)
    assert F.affine(img, 10.0, [0, 0], 1.0, [0.0, 0.0]).shape == img.shape
    assert F.perspective(img, None, None, coefficients=[1, 0, 0, 0, 1, 0, 0, 0]).shape == img.shape
    w, h = F._compute_affine_output_size(F._get_inverse_affine_matrix([0.0, 0.0], -90.0, [0.0, 0.0], 1.0, [0.0, 0.0]), IW, IH)
    assert F.rotate(img, 90.0, expand=True).shape == (0, 3, h, w) == (0, 3, IW, IH)


def _ref_inverse_matrix(center, angle, translate, scale, shear):
    """The reference's docstring form of the inverse: M = T * C * RotateScaleShear * C^-1 (float64 matrices), inverted."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    T = torch.tensor([[1, 0, tx], [0, 1, ty], [0, 0, 1]], dtype=torch.float64)
    C = torch.tensor([[1, 0, cx], [0, 1, cy], [0, 0, 1]], dtype=torch.float64)
    R = torch.tensor([[math.cos(rot), -math.sin(rot), 0], [math.sin(rot), math.cos(rot), 0], [0, 0, 1]], dtype=torch.float64)
    Sx = torch.tensor([[1, -math.tan(sx), 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float64)
    Sy = torch.tensor([[1, 0, 0], [-math.tan(sy), 1, 0], [0, 0, 1]], dtype=torch.float64)
    S = torch.diag(torch.tensor([scale, scale, 1.0], dtype=torch.float64))
    M = T @ C @ R @ S @ Sy @ Sx @ torch.linalg.inv(C)
    return torch.linalg.inv(M)[:2].reshape(6)


@pytest.mark.parametrize("center,angle,translate,scale,shear", [
    ([0.0, 0.0], 30.0, [0.0, 0.0], 1.0, [0.0, 0.0]),
    ([3.5, -2.0], -73.2, [5.0, -1.0], 0.7, [12.0, 0.0]),
    ([-10.0, 4.0], 190.0, [0.0, 2.0], 1.6, [-8.0, 20.0]),
])
def test_inverse_affine_matrix_against_composed_matrices(center, angle, translate, scale, shear):
    got = torch.tensor(F._get_inverse_affine_matrix(center, angle, translate, scale, shear), dtype=torch.float64)
    want = _ref_inverse_matrix(center, angle, translate, scale, shear)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_rotate_expand_size():
    """The rotated frame's bounding box (corners at +-w/2, +-h/2 about the centre), ceil / floor after shifting by the
    half sizes: 90 and 180 degrees swap / keep the sides exactly (cos 90 is 6e-17, not 0: the 1e-4 truncation absorbs it)."""
    for w, h, angle, want in ((1920, 1080, 90.0, (1080, 1920)), (1920, 1080, 180.0, (1920, 1080)), (100, 100, 45.0, (142, 142)),
                              (7, 5, 0.0, (7, 5)), (64, 32, 30.0, (72, 60)), (64, 32, -30.0, (72, 60)), (1, 9, 90.0, (9, 1))):
        matrix = F._get_inverse_affine_matrix([0.0, 0.0], -angle, [0.0, 0.0], 1.0, [0.0, 0.0])
        assert F._compute_affine_output_size(matrix, w, h) == want, (w, h, angle)


def test_perspective_coefficients_map_the_corners():
    start = [[0, 0], [99, 0], [99, 59], [0, 59]]
    end = [[7, 3], [90, 9], [95, 55], [2, 50]]
    c = F._get_perspective_coeffs(start, end)
    assert len(c) == 8 and all(isinstance(v, float) for v in c)
    assert torch.tensor(c, dtype=torch.float32).tolist() == c  # rounded to float32, as the reference returns them
    for (xs, ys), (xe, ye) in zip(start, end):  # output (end) pixel -> input (start) pixel
        den = c[6] * xe + c[7] * ye + 1
        assert abs((c[0] * xe + c[1] * ye + c[2]) / den - xs) < 1e-3
        assert abs((c[3] * xe + c[4] * ye + c[5]) / den - ys) < 1e-3
    assert F._perspective_coefficients(None, None, [1, 2, 3, 4, 5, 6, 7, 8]) == [1, 2, 3, 4, 5, 6, 7, 8]


# ---- the grid the kernel computes, emulated exactly in float32, against the reference's CPU bmm
def _fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c) of float32 arrays (float64 product is exact; TwoSum fixes the float64 rounding
    of the sum where it lands exactly on a float32 tie)."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    rd = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > rd, np.float32(np.inf), np.float32(-np.inf))).astype(np.float32)
    tie = (s == (rd + other.astype(np.float64)) / 2) & (e != 0) & (s != rd)
    return np.where(tie, np.where(e > 0, np.maximum(r, other), np.minimum(r, other)), r).astype(np.float32)


def _kernel_lin(x, y, a, b, c, order):
    """k_warp's g = fma(y, b, x * a) + c (order 1) or (x * a + y * b) + c (order 0), float32."""
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    if order:
        return (_fma32(y, b, x * a) + c).astype(np.float32)
    return ((x * a + y * b) + c).astype(np.float32)


def _base(oh, ow, kind):
    j = np.arange(ow, dtype=np.float32)[None, :].repeat(oh, 0)
    i = np.arange(oh, dtype=np.float32)[:, None].repeat(ow, 1)
    if kind == "affine":
        return j - np.float32(0.5 * (ow - 1)), i - np.float32(0.5 * (oh - 1))
    return j + np.float32(0.5), i + np.float32(0.5)


SIZES = [(11, 6), (17, 4), (6, 11), (4, 17), (1, 66), (1, 67), (33, 2), (2, 34), (23, 37), (224, 224), (480, 640), (1, 1), (9, 1)]


def _matrices(seed, n=6):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        r = (torch.rand(5, generator=g, dtype=torch.float64) * 2 - 1).tolist()
        out.append(F._get_inverse_affine_matrix([r[0] * 10, r[1] * 10], r[2] * 180, [r[3] * 5, r[4] * 5], 0.5 + abs(r[0]),
                                                [r[1] * 30, r[2] * 20]))
    return out


@pytest.mark.parametrize("oh,ow", SIZES, ids=lambda v: str(v))
def test_affine_grid_formula_equals_cpu_bmm(oh, ow):
    """The kernel's grid form, picked by the 400 rule and this host's probed bmm rounding, against the reference's
    `_affine_grid` bmm on this host, both axes."""
    order = F._grid_order(oh, ow)
    assert order == (0 if oh * ow * 3 * 2 < 400 or not F._blocked_bmm_fuses() else 1)
    x, y = _base(oh, ow, "affine")
    for ih, iw in ((oh, ow), (oh + 5, ow * 2 + 1)):  # rotate's expand: normalised by the input size
        for matrix in _matrices(oh * 1000 + ow):
            theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
            rt = theta.transpose(1, 2).div_(torch.tensor([0.5 * iw, 0.5 * ih], dtype=torch.float32))
            base = torch.empty(1, oh, ow, 3)
            base[..., 0].copy_(torch.linspace((1.0 - ow) * 0.5, (ow - 1.0) * 0.5, steps=ow))
            base[..., 1].copy_(torch.linspace((1.0 - oh) * 0.5, (oh - 1.0) * 0.5, steps=oh).unsqueeze_(-1))
            base[..., 2].fill_(1)
            want = base.view(1, oh * ow, 3).bmm(rt).view(oh, ow, 2).numpy()
            k = F._affine_coeffs(matrix, iw, ih)
            assert k[:6] == rt[0].t().reshape(6).tolist()
            np.testing.assert_array_equal(_kernel_lin(x, y, k[0], k[1], k[2], order), want[..., 0])
            np.testing.assert_array_equal(_kernel_lin(x, y, k[3], k[4], k[5], order), want[..., 1])


@pytest.mark.parametrize("oh,ow", SIZES, ids=lambda v: str(v))
def test_perspective_grid_formula_equals_cpu_bmm(oh, ow):
    order = F._grid_order(oh, ow)
    x, y = _base(oh, ow, "perspective")
    g = torch.Generator().manual_seed(oh * 31 + ow)
    for _ in range(6):
        start = [[0, 0], [ow - 1, 0], [ow - 1, oh - 1], [0, oh - 1]]
        end = [[int(px + torch.randint(-3, 4, (1,), generator=g)), int(py + torch.randint(-3, 4, (1,), generator=g))]
               for px, py in start]
        coeffs = (torch.rand(8, generator=g) * 2 - 1).tolist() if min(oh, ow) < 4 else F._get_perspective_coeffs(start, end)
        coeffs[6:] = [v * 1e-3 for v in coeffs[6:]] if min(oh, ow) < 4 else coeffs[6:]
        theta1 = torch.tensor([[[coeffs[0], coeffs[1], coeffs[2]], [coeffs[3], coeffs[4], coeffs[5]]]], dtype=torch.float32)
        theta2 = torch.tensor([[[coeffs[6], coeffs[7], 1.0], [coeffs[6], coeffs[7], 1.0]]], dtype=torch.float32)
        base = torch.empty(1, oh, ow, 3)
        base[..., 0].copy_(torch.linspace(0.5, ow + 0.5 - 1.0, steps=ow))
        base[..., 1].copy_(torch.linspace(0.5, oh + 0.5 - 1.0, steps=oh).unsqueeze_(-1))
        base[..., 2].fill_(1)
        rt1 = theta1.transpose(1, 2).div_(torch.tensor([0.5 * ow, 0.5 * oh], dtype=torch.float32))
        g1 = base.view(1, oh * ow, 3).bmm(rt1)
        g2 = base.view(1, oh * ow, 3).bmm(theta2.transpose(1, 2))
        want = g1.div_(g2).sub_(1.0).view(oh, ow, 2).numpy()
        k = F._perspective_grid_coeffs(coeffs, ow, oh)
        den = _kernel_lin(x, y, k[6], k[7], 1.0, order)
        with np.errstate(divide="ignore", invalid="ignore"):
            gx = (_kernel_lin(x, y, k[0], k[1], k[2], order) / den - np.float32(1)).astype(np.float32)
            gy = (_kernel_lin(x, y, k[3], k[4], k[5], order) / den - np.float32(1)).astype(np.float32)
        np.testing.assert_array_equal(gx, want[..., 0])
        np.testing.assert_array_equal(gy, want[..., 1])


def test_base_grid_vectors_are_the_closed_forms():
    """The reference's linspace base vectors have step exactly 1: j - (n - 1) / 2 (affine) and j + 0.5 (perspective)."""
    for n in list(range(1, 700)) + [1023, 1024, 1080, 1920, 2160, 3840, 4096, 8191, 16384]:
        j = torch.arange(n, dtype=torch.float32)
        assert torch.equal(torch.linspace((1.0 - n) * 0.5, (n - 1.0) * 0.5, steps=n), j - 0.5 * (n - 1)), n
        assert torch.equal(torch.linspace(0.5, n + 0.5 - 1.0, steps=n, dtype=torch.float32), j + 0.5), n


# ---- the transforms
def test_transform_arguments():
    tr = transforms.RandomRotation(30)
    assert tr.degrees == [-30.0, 30.0] and tr.interpolation is transforms.InterpolationMode.NEAREST and tr.fill == 0
    assert transforms._get_fill(tr._fill, tv_tensors.Image) == 0
    with pytest.raises(ValueError, match="If degrees is a single number, it must be positive"):
        transforms.RandomRotation(-1)
    with pytest.raises(ValueError, match="degrees should be a sequence of length 2"):
        transforms.RandomRotation([1, 2, 3])
    with pytest.raises(ValueError, match="center should be a sequence of length 2"):
        transforms.RandomRotation(3, center=[1])
    tr = transforms.RandomAffine((-5, 15), shear=7)
    assert tr.degrees == [-5.0, 15.0] and tr.shear == [-7.0, 7.0] and tr.interpolation is transforms.InterpolationMode.NEAREST
    with pytest.raises(ValueError, match="translation values should be between 0 and 1"):
        transforms.RandomAffine(0, translate=(0.5, 1.5))
    with pytest.raises(ValueError, match="scale values should be positive"):
        transforms.RandomAffine(0, scale=(0.0, 1.0))
    with pytest.raises(ValueError, match="shear should be a sequence of length 2 or 4"):
        transforms.RandomAffine(0, shear=(1, 2, 3))
    with pytest.raises(TypeError, match="inappropriate fill arg"):
        transforms.RandomAffine(0, fill="white")
    tr = transforms.RandomPerspective()
    assert tr.distortion_scale == 0.5 and tr.p == 0.5 and tr.interpolation is transforms.InterpolationMode.BILINEAR
    assert isinstance(tr, transforms._RandomApplyTransform)
    with pytest.raises(ValueError, match="distortion_scale value should be between 0 and 1"):
        transforms.RandomPerspective(1.5)


def test_seeded_get_params_follow_the_reference_draws():
    h, w = 40, 60
    sample = [torch.zeros(3, h, w)]
    tr = transforms.RandomAffine((-20, 30), translate=(0.1, 0.25), scale=(0.8, 1.2), shear=(-5, 10, 2, 6))
    torch.manual_seed(3)
    got = tr._get_params(sample)
    torch.manual_seed(3)
    angle = torch.empty(1).uniform_(-20.0, 30.0).item()
    tx = int(round(torch.empty(1).uniform_(-0.1 * w, 0.1 * w).item()))
    ty = int(round(torch.empty(1).uniform_(-0.25 * h, 0.25 * h).item()))
    scale = torch.empty(1).uniform_(0.8, 1.2).item()
    sx = torch.empty(1).uniform_(-5.0, 10.0).item()
    sy = torch.empty(1).uniform_(2.0, 6.0).item()
    assert got == dict(angle=angle, translate=(tx, ty), scale=scale, shear=(sx, sy))
    torch.manual_seed(3)
    got = transforms.RandomAffine(10)._get_params(sample)
    assert got == dict(angle=_draw_after_seed(3, -10.0, 10.0), translate=(0, 0), scale=1.0, shear=(0.0, 0.0))

    torch.manual_seed(4)
    got = transforms.RandomRotation((10, 80))._get_params(sample)
    assert got == dict(angle=_draw_after_seed(4, 10.0, 80.0))

    torch.manual_seed(5)
    got = transforms.RandomPerspective(0.4)._get_params(sample)
    torch.manual_seed(5)
    bh, bw = int(0.4 * (h // 2)) + 1, int(0.4 * (w // 2)) + 1
    tl = [int(torch.randint(0, bw, size=(1,))), int(torch.randint(0, bh, size=(1,)))]
    tr_ = [int(torch.randint(w - bw, w, size=(1,))), int(torch.randint(0, bh, size=(1,)))]
    br = [int(torch.randint(w - bw, w, size=(1,))), int(torch.randint(h - bh, h, size=(1,)))]
    bl = [int(torch.randint(0, bw, size=(1,))), int(torch.randint(h - bh, h, size=(1,)))]
    start = [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]]
    assert got == dict(coefficients=F._get_perspective_coeffs(start, [tl, tr_, br, bl]))


def _draw_after_seed(seed, lo, hi):
    torch.manual_seed(seed)
    return torch.empty(1).uniform_(lo, hi).item()


def test_transforms_route_to_the_functionals():
    """_transform calls F.affine / F.rotate / F.perspective with the transform's fill and interpolation (here the host
    tensor reaches the library and raises its no-CPU error; a fill of the wrong length raises the reference's error)."""
    img = torch.zeros(3, IH, IW)
    for tr, params in ((transforms.RandomAffine(10), dict(angle=3.0, translate=(0, 0), scale=1.0, shear=(0.0, 0.0))),
                       (transforms.RandomRotation(10, expand=True), dict(angle=3.0)),
                       (transforms.RandomPerspective(), dict(coefficients=[1.0, 0, 0, 0, 1.0, 0, 0, 0]))):
        with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
            tr._transform(img, params)
        tr._fill = transforms._setup_fill_arg([1, 2])
        with pytest.raises(ValueError, match="cannot broadcast"):
            tr._transform(img, params)
