"""F.affine / F.rotate / F.perspective and RandomAffine / RandomRotation / RandomPerspective on the MI355X (`-m gpu`) against
the reference's own computation on the host CPU: torchvision 0.20's v2 affine_image / rotate_image / perspective_image
(transforms/v2/functional/_geometry.py: _affine_grid / _perspective_grid via bmm + _apply_grid_transform) restated below with
the same torch ops.  The host math (inverse matrix, expand size, perspective coefficients) is the library's restatement of the
reference's, checked without a GPU in tests/test_warp_host.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, functional as F, transforms, tv_tensors  # noqa: E402


def _affine_grid(theta, w, h, ow, oh):   # v2 _affine_grid, CPU
    base_grid = torch.empty(1, oh, ow, 3, dtype=theta.dtype)
    base_grid[..., 0].copy_(torch.linspace((1.0 - ow) * 0.5, (ow - 1.0) * 0.5, steps=ow))
    base_grid[..., 1].copy_(torch.linspace((1.0 - oh) * 0.5, (oh - 1.0) * 0.5, steps=oh).unsqueeze_(-1))
    base_grid[..., 2].fill_(1)
    rescaled_theta = theta.transpose(1, 2).div_(torch.tensor([0.5 * w, 0.5 * h], dtype=theta.dtype))
    return base_grid.view(1, oh * ow, 3).bmm(rescaled_theta).view(1, oh, ow, 2)


def _perspective_grid(coeffs, ow, oh, dtype):   # v2 _perspective_grid, CPU
    theta1 = torch.tensor([[[coeffs[0], coeffs[1], coeffs[2]], [coeffs[3], coeffs[4], coeffs[5]]]], dtype=dtype)
    theta2 = torch.tensor([[[coeffs[6], coeffs[7], 1.0], [coeffs[6], coeffs[7], 1.0]]], dtype=dtype)
    d = 0.5
    base_grid = torch.empty(1, oh, ow, 3, dtype=dtype)
    base_grid[..., 0].copy_(torch.linspace(d, ow + d - 1.0, steps=ow, dtype=dtype))
    base_grid[..., 1].copy_(torch.linspace(d, oh + d - 1.0, steps=oh, dtype=dtype).unsqueeze_(-1))
    base_grid[..., 2].fill_(1)
    rescaled_theta1 = theta1.transpose(1, 2).div_(torch.tensor([0.5 * ow, 0.5 * oh], dtype=dtype))
    shape = (1, oh * ow, 3)
    output_grid1 = base_grid.view(shape).bmm(rescaled_theta1)
    output_grid2 = base_grid.view(shape).bmm(theta2.transpose(1, 2))
    return output_grid1.div_(output_grid2).sub_(1.0).view(1, oh, ow, 2)


def _apply_grid_transform(img, grid, mode, fill):   # v2 _apply_grid_transform, CPU
    input_shape = img.shape
    oh, ow = grid.shape[1], grid.shape[2]
    c, ih, iw = input_shape[-3:]
    output_shape = input_shape[:-3] + (c, oh, ow)
    img = img.reshape(-1, c, ih, iw)
    n = img.shape[0]
    fp = img.dtype == grid.dtype
    fi = img if fp else img.to(grid.dtype)
    if n > 1:
        grid = grid.expand(n, -1, -1, -1)
    if fill is not None:
        fi = torch.cat((fi, torch.ones((n, 1, ih, iw), dtype=fi.dtype)), dim=1)
    fi = torch.nn.functional.grid_sample(fi, grid, mode=mode, padding_mode="zeros", align_corners=False)
    if fill is not None:
        fi, mask = torch.tensor_split(fi, indices=(-1,), dim=-3)
        mask = mask.expand_as(fi)
        fill_list = fill if isinstance(fill, (tuple, list)) else [float(fill)]
        fill_img = torch.tensor(fill_list, dtype=fi.dtype).view(1, -1, 1, 1)
        if mode == "nearest":
            fi = torch.where(mask < 0.5, fill_img.expand_as(fi), fi)
        else:
            fi = fi.sub_(fill_img).mul_(mask).add_(fill_img)
    img = fi.round_().to(img.dtype) if not fp else fi
    return img.reshape(output_shape)


def ref_affine(img, angle, translate, scale, shear, mode="nearest", fill=None, center=None):   # v2 affine_image
    angle, translate, shear, center = F._affine_parse_args(angle, translate, scale, shear, center)
    height, width = img.shape[-2:]
    center_f = [0.0, 0.0] if center is None else [(c - s * 0.5) for c, s in zip(center, [width, height])]
    matrix = F._get_inverse_affine_matrix(center_f, angle, [float(t) for t in translate], scale, shear)
    dtype = img.dtype if torch.is_floating_point(img) else torch.float32
    theta = torch.tensor(matrix, dtype=dtype).reshape(1, 2, 3)
    return _apply_grid_transform(img, _affine_grid(theta, w=width, h=height, ow=width, oh=height), mode, fill)


def ref_rotate(img, angle, mode="nearest", expand=False, center=None, fill=None):   # v2 rotate_image
    shape = img.shape
    c, height, width = shape[-3:]
    center_f = [0.0, 0.0] if center is None else [(cc - s * 0.5) for cc, s in zip(center, [width, height])]
    matrix = F._get_inverse_affine_matrix(center_f, -angle, [0.0, 0.0], 1.0, [0.0, 0.0])
    img = img.reshape(-1, c, height, width)
    ow, oh = F._compute_affine_output_size(matrix, width, height) if expand else (width, height)
    dtype = img.dtype if torch.is_floating_point(img) else torch.float32
    theta = torch.tensor(matrix, dtype=dtype).reshape(1, 2, 3)
    out = _apply_grid_transform(img, _affine_grid(theta, w=width, h=height, ow=ow, oh=oh), mode, fill)
    return out.reshape(shape[:-3] + (c, oh, ow))


def ref_perspective(img, coeffs, mode="bilinear", fill=None):   # v2 perspective_image
    oh, ow = img.shape[-2:]
    dtype = img.dtype if torch.is_floating_point(img) else torch.float32
    return _apply_grid_transform(img, _perspective_grid(coeffs, ow=ow, oh=oh, dtype=dtype), mode, fill)


EXACT = torch.backends.cpu.get_cpu_capability() in ("AVX2", "AVX512")


def assert_matches_reference(got, want, what=""):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if EXACT:
        if not torch.equal(got, want):
            diff = (got.double() - want.double()).abs()
            raise AssertionError(f"{what}: {int((diff > 0).sum())} of {diff.numel()} elements differ (max {float(diff.max())})")
    elif want.dtype == torch.uint8:
        assert (got.int() - want.int()).abs().max() <= 1, what
    else:
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6, msg=what)


def _image(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    if dtype == torch.bool:
        return torch.rand(shape, generator=g) > 0.5
    return torch.rand(shape, generator=g, dtype=torch.float32)


def _fill_for(fill, c):
    return fill[:c] if isinstance(fill, list) and c < len(fill) else fill


def _coeffs_from_corners(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    start = [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]]
    end = [[int(x + torch.randint(-w // 5, w // 5 + 1, (1,), generator=g)), int(y + torch.randint(-h // 5, h // 5 + 1, (1,), generator=g))]
           for x, y in start]
    return start, end


# (name, F call, reference call) over an image tensor
def _ops(h, w):
    start, end = _coeffs_from_corners(h, w, seed=h * 7 + w)
    coeffs = F._get_perspective_coeffs(start, end)
    return [
        ("rot30", lambda x, **k: F.rotate(x, 30.0, **k), lambda x, mode, fill: ref_rotate(x, 30.0, mode=mode, fill=fill)),
        ("rot90", lambda x, **k: F.rotate(x, 90, **k), lambda x, mode, fill: ref_rotate(x, 90, mode=mode, fill=fill)),
        ("rot-137.3_expand", lambda x, **k: F.rotate(x, -137.3, expand=True, **k),
         lambda x, mode, fill: ref_rotate(x, -137.3, mode=mode, expand=True, fill=fill)),
        ("affine_shear", lambda x, **k: F.affine(x, 12.5, [3, -2], 0.85, [10.0, -4.0], **k),
         lambda x, mode, fill: ref_affine(x, 12.5, [3, -2], 0.85, [10.0, -4.0], mode=mode, fill=fill)),
        ("affine_center", lambda x, **k: F.affine(x, -40.0, (1.5, 0), 1.3, 5, center=[2, h - 3], **k),
         lambda x, mode, fill: ref_affine(x, -40.0, (1.5, 0), 1.3, 5, mode=mode, fill=fill, center=[2, h - 3])),
    ] + ([] if min(h, w) < 4 else [  # fewer than four distinct corners make no perspective
        ("perspective", lambda x, **k: F.perspective(x, start, end, **k),
         lambda x, mode, fill: ref_perspective(x, coeffs, mode=mode, fill=fill))])


SHAPES = [(3, 37, 53), (1, 224, 224), (2, 3, 97, 130), (2, 2, 3, 31, 64), (3, 11, 6), (1, 17, 4), (3, 9, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fill", [None, 0, 127, [10, 20, 30]], ids=["nofill", "fill0", "fill127", "fill_list"])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.bool], ids=["f32", "u8", "bool"])
def test_parity_matrix(dtype, mode, fill, shape):
    h, w = shape[-2:]
    img = _image(shape, dtype, seed=h * 131 + w)
    fill = _fill_for(fill, shape[-3])
    if dtype == torch.bool and fill not in (None, 0):
        fill = 1
    img_d = img.cuda()
    for name, ours, ref in _ops(h, w):
        got = ours(img_d, interpolation=mode, fill=fill)
        assert _lib.last_kernel().startswith("k_warp<" + ("u8" if dtype == torch.uint8 else "f32")), _lib.last_kernel()
        assert_matches_reference(got, ref(img, mode, fill), f"{name} {dtype} {mode} fill={fill} {shape}")
    assert torch.equal(img_d.cpu(), img)  # the input is untouched


@pytest.mark.parametrize("angle", [0, 90, 180, 270, -90, 1e-3, 44.99, 45, 359.5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
def test_rotate_angles_and_expand(angle, dtype):
    img = _image((3, 45, 62), dtype, seed=3)
    x = img.cuda()
    for expand in (False, True):
        for mode in ("bilinear", "nearest"):
            got = F.rotate(x, angle, interpolation=mode, expand=expand, fill=[1, 2, 3])
            want = ref_rotate(img, angle, mode=mode, expand=expand, fill=[1, 2, 3])
            assert_matches_reference(got, want, f"{angle} expand={expand} {mode}")


@pytest.mark.parametrize("offset", [37, 64])
@pytest.mark.parametrize("w", [1, 2, 61, 63, 64, 257])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_canary_ragged_widths(w, dtype, offset):
    """The output placed inside a larger sentinel-filled buffer (at an odd element offset, or an aligned one that lets widths
    w % 4 == 0 take the vector stores), both layouts: nothing outside it changes and the result equals the reference."""
    h, planes = 9, 6
    img = _image((2, 3, h, w), dtype, seed=w)
    x = img.cuda()
    lib = _lib.load()
    fn = lib.mv_warp_u8 if dtype == torch.uint8 else lib.mv_warp_f32
    for angle in (0.0, 33.0):  # row and block layouts
        matrix = F._get_inverse_affine_matrix([0.0, 0.0], -angle, [0.0, 0.0], 1.0, [0.0, 0.0])
        for mode in ("bilinear", "nearest"):
            n = planes * h * w
            sentinel = 0xA5 if dtype == torch.uint8 else -7.25
            buf = torch.full((n + 2 * offset,), sentinel, dtype=dtype, device="cuda")
            y = buf[offset: offset + n]
            _lib.check(fn(x.data_ptr(), y.data_ptr(), planes, 3, h, w, h, w, _lib.taps(F._affine_coeffs(matrix, w, h)), 0,
                          F._grid_order(h, w), 0 if mode == "bilinear" else 1, _lib.taps([3.0, 4.0, 5.0]), _lib.stream_ptr(x)))
            torch.cuda.synchronize()
            host = buf.cpu()
            assert (host[:offset] == sentinel).all() and (host[offset + n:] == sentinel).all()
            assert_matches_reference(y.reshape(img.shape), ref_rotate(img, angle, mode=mode, fill=[3.0, 4.0, 5.0]),
                                     f"w={w} angle={angle} {mode}")
    assert torch.equal(x.cpu(), img)


def test_masks_videos_and_non_contiguous_input():
    h, w = 40, 52
    mask = tv_tensors.Mask((_image((h, w), torch.uint8, 2) % 5).cuda())
    got = F.rotate(mask, 33.0, fill=255)
    assert type(got) is tv_tensors.Mask and got.shape == (h, w)
    want = ref_rotate(mask.as_subclass(torch.Tensor).cpu().unsqueeze(0), 33.0, mode="nearest", fill=255).squeeze(0)
    assert_matches_reference(got.as_subclass(torch.Tensor), want, "mask rotate")
    got = F.affine(mask, 10.0, [2, 3], 1.1, [4.0, 0.0], interpolation="bilinear")  # masks are always nearest
    want = ref_affine(mask.as_subclass(torch.Tensor).cpu().unsqueeze(0), 10.0, [2, 3], 1.1, [4.0, 0.0]).squeeze(0)
    assert_matches_reference(got.as_subclass(torch.Tensor), want, "mask affine")
    start, end = _coeffs_from_corners(h, w, 5)
    got = F.perspective(mask, start, end)
    want = ref_perspective(mask.as_subclass(torch.Tensor).cpu().unsqueeze(0), F._get_perspective_coeffs(start, end),
                           mode="nearest").squeeze(0)
    assert_matches_reference(got.as_subclass(torch.Tensor), want, "mask perspective")

    video = tv_tensors.Video(_image((2, 3, h, w), torch.float32, 4).cuda())
    got = F.rotate(video, -20.0, interpolation="bilinear", expand=True, fill=0)
    assert type(got) is tv_tensors.Video
    assert_matches_reference(got.as_subclass(torch.Tensor),
                             ref_rotate(video.as_subclass(torch.Tensor).cpu(), -20.0, mode="bilinear", expand=True, fill=0))

    base = _image((3, w, h), torch.float32, 6)
    nc = base.cuda().transpose(-1, -2)  # (3, h, w), not contiguous
    assert not nc.is_contiguous()
    got = F.affine(nc, 25.0, [0, 0], 1.0, [0.0, 0.0], interpolation="bilinear", fill=[1.0, 2.0, 3.0])
    assert_matches_reference(got, ref_affine(base.transpose(-1, -2).contiguous(), 25.0, [0, 0], 1.0, [0.0, 0.0],
                                             mode="bilinear", fill=[1.0, 2.0, 3.0]), "non-contiguous")


def test_random_transforms_on_a_sample_match_the_reference():
    """Seeded RandomAffine / RandomRotation / RandomPerspective on {Image u8, Mask u8, Video f32}: the params the transform
    draws under a seed, applied by the reference restated, equal the transform's outputs; masks use nearest."""
    h, w = 64, 96
    img = tv_tensors.Image(_image((3, h, w), torch.uint8, 1).cuda())
    mask = tv_tensors.Mask((_image((h, w), torch.uint8, 2) % 5).cuda())
    video = tv_tensors.Video(_image((2, 3, h, w), torch.float32, 3).cuda())
    cases = [
        (transforms.RandomAffine(30, translate=(0.1, 0.2), scale=(0.7, 1.3), shear=(-10, 10, -5, 5),
                                 interpolation=transforms.InterpolationMode.BILINEAR, fill=7),
         lambda x, p, mode, fill: ref_affine(x, p["angle"], list(p["translate"]), p["scale"], list(p["shear"]), mode=mode,
                                             fill=fill)),
        (transforms.RandomAffine(15, fill={tv_tensors.Image: [10, 20, 30], tv_tensors.Mask: 255, "others": None}, center=[5, 9]),
         lambda x, p, mode, fill: ref_affine(x, p["angle"], list(p["translate"]), p["scale"], list(p["shear"]), mode=mode,
                                             fill=fill, center=[5, 9])),
        (transforms.RandomRotation((-60, 60), interpolation=transforms.InterpolationMode.BILINEAR, expand=True),
         lambda x, p, mode, fill: ref_rotate(x, p["angle"], mode=mode, expand=True, fill=fill)),
        (transforms.RandomPerspective(0.6, p=1.0),
         lambda x, p, mode, fill: ref_perspective(x, p["coefficients"], mode=mode, fill=fill)),
    ]
    for tr, ref in cases:
        torch.manual_seed(21)
        out = tr({"image": img, "mask": mask, "video": video})
        torch.manual_seed(21)
        if isinstance(tr, transforms.RandomPerspective):
            torch.rand(1)  # _RandomApplyTransform's draw
        params = tr._get_params([img, mask, video])
        mode = tr.interpolation.value
        f_img = transforms._get_fill(tr._fill, tv_tensors.Image)
        f_mask = transforms._get_fill(tr._fill, tv_tensors.Mask)
        f_vid = transforms._get_fill(tr._fill, tv_tensors.Video)
        assert type(out["image"]) is tv_tensors.Image and type(out["mask"]) is tv_tensors.Mask
        assert type(out["video"]) is tv_tensors.Video
        what = type(tr).__name__
        assert_matches_reference(out["image"].as_subclass(torch.Tensor),
                                 ref(img.as_subclass(torch.Tensor).cpu(), params, mode, f_img), f"{what} image")
        m_ref = ref(mask.as_subclass(torch.Tensor).cpu().unsqueeze(0), params, "nearest", f_mask).squeeze(0)
        assert_matches_reference(out["mask"].as_subclass(torch.Tensor), m_ref, f"{what} mask")
        assert_matches_reference(out["video"].as_subclass(torch.Tensor),
                                 ref(video.as_subclass(torch.Tensor).cpu(), params, mode, f_vid), f"{what} video")


def test_float_output_is_forward_only_and_runs_on_the_current_stream():
    img = _image((2, 3, 97, 130), torch.float32, 12).cuda()
    want = F.rotate(img, 30.0, interpolation="bilinear", fill=0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = F.rotate(img, 30.0, interpolation="bilinear", fill=0)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    x = img.clone().requires_grad_(True)
    y = F.affine(x, 5.0, [0, 0], 1.0, [0.0, 0.0])
    with pytest.raises(RuntimeError, match="forward-only"):
        y.sum().backward()
