"""F.elastic / ElasticTransform on the MI355X (`-m gpu`) against the reference's own computation on the host CPU:
torchvision 0.20's v2 elastic_image (transforms/v2/functional/_geometry.py: _create_identity_grid + _apply_grid_transform)
restated below with the same torch ops.  On an AVX2 / AVX-512 host the results are bit-identical (the kernel follows ATen's
vectorised grid_sampler, whose multiply-adds are fused there)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, _pil, functional as F, transforms, tv_tensors  # noqa: E402


def ref_elastic_image(img, displacement, mode="bilinear", fill=None):   # v2 elastic_image, CPU
    H, W = img.shape[-2:]
    dt = img.dtype if img.is_floating_point() else torch.float32
    if displacement.shape != (1, H, W, 2):
        raise ValueError(f"Argument displacement shape should be {(1, H, W, 2)}, but given {displacement.shape}")
    g = torch.empty(1, H, W, 2, dtype=dt)
    g[..., 0].copy_(torch.linspace((-W + 1) / W, (W - 1) / W, W, dtype=dt))
    g[..., 1].copy_(torch.linspace((-H + 1) / H, (H - 1) / H, H, dtype=dt).unsqueeze_(-1))
    g = g.add_(displacement.to(dt))
    C = img.shape[-3]; x = img.reshape(-1, C, H, W); n = x.shape[0]  # noqa: E702
    fp = img.dtype == dt; fi = x if fp else x.to(dt)  # noqa: E702
    if fill is not None:                                 # dummy mask channel for the fill colour
        fi = torch.cat((fi, torch.ones(n, 1, H, W, dtype=dt)), 1)
    fi = torch.nn.functional.grid_sample(fi, g.expand(n, -1, -1, -1), mode=mode,
                                         padding_mode="zeros", align_corners=False)
    if fill is not None:
        fi, m = torch.tensor_split(fi, indices=(-1,), dim=-3); m = m.expand_as(fi)  # noqa: E702
        fl = fill if isinstance(fill, (tuple, list)) else [float(fill)]
        f_img = torch.tensor(fl, dtype=dt).view(1, -1, 1, 1)
        fi = (torch.where(m < 0.5, f_img.expand_as(fi), fi) if mode == "nearest"
              else fi.sub_(f_img).mul_(m).add_(f_img))
    return (fi.round_().to(img.dtype) if not fp else fi).reshape(img.shape)


EXACT = torch.backends.cpu.get_cpu_capability() in ("AVX2", "AVX512")


def assert_matches_reference(got, want, what=""):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, what
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
    return torch.rand(shape, generator=g, dtype=torch.float32)


def _fields(h, w, seed):
    """(name, field on the device): small random, ElasticTransform's own, alpha = 1000 (many samples leave the frame), zero."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    probe = torch.zeros(1, h, w)
    return [
        ("random", ((torch.rand(1, h, w, 2, generator=g) - 0.5) * 0.1).cuda()),
        ("alpha50", transforms.ElasticTransform(alpha=50.0, sigma=5.0).get_params(probe)["displacement"]),
        ("alpha1000", transforms.ElasticTransform(alpha=1000.0, sigma=5.0).get_params(probe)["displacement"]),
        ("zero", torch.zeros(1, h, w, 2, device="cuda")),
    ]


def _fill_for(fill, c):
    return fill[:c] if isinstance(fill, list) and c < len(fill) else fill


SHAPES = [(3, 37, 53), (1, 224, 224), (2, 3, 97, 130), (2, 4, 3, 64, 80)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fill", [None, 0, 127, [10, 20, 30]], ids=["nofill", "fill0", "fill127", "fill_list"])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
def test_parity_matrix(dtype, mode, fill, shape):
    h, w = shape[-2:]
    img = _image(shape, dtype, seed=h * 131 + w)
    fill = _fill_for(fill, shape[-3])  # one value per channel: [10] for the 1-channel shape
    img_d = img.cuda()
    for name, disp in _fields(h, w, seed=w):
        got = F.elastic(img_d, disp, interpolation=mode, fill=fill)
        assert _lib.last_kernel().startswith("k_elastic<" + ("f32" if dtype == torch.float32 else "u8") + "," + mode), _lib.last_kernel()
        want = ref_elastic_image(img, disp.cpu(), mode=mode, fill=fill)
        assert_matches_reference(got, want, f"{name} {dtype} {mode} fill={fill} {shape}")
    assert torch.equal(img_d.cpu(), img)  # the input is untouched


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
def test_permuted_and_contiguous_fields_agree(dtype):
    img = _image((2, 3, 97, 130), dtype, seed=3).cuda()
    torch.manual_seed(11)
    disp = transforms.ElasticTransform(alpha=80.0, sigma=4.0).get_params(img)["displacement"]
    assert not disp.is_contiguous() and disp.stride(3) == 97 * 130  # _get_params' dx plane / dy plane permute
    for mode in ("bilinear", "nearest"):
        a = F.elastic(img, disp, interpolation=mode, fill=[1, 2, 3])
        b = F.elastic(img, disp.contiguous(), interpolation=mode, fill=[1, 2, 3])
        assert torch.equal(a, b)
        assert_matches_reference(a, ref_elastic_image(img.cpu(), disp.cpu(), mode=mode, fill=[1, 2, 3]), mode)


def test_plane_offsets_past_2_31_elements():
    """A uint8 batch of more than 2^31 elements: the first and the last plane against the reference (planes are independent,
    so the reference runs on just those two)."""
    h, w = 1080, 1920
    planes = (2 ** 31) // (h * w) + 2
    assert planes * h * w > 2 ** 31
    x = torch.empty((planes, 1, h, w), dtype=torch.uint8, device="cuda")
    x[0].random_(0, 256)
    x[-1].random_(0, 256)
    torch.manual_seed(5)
    disp = transforms.ElasticTransform(alpha=50.0, sigma=5.0).get_params(x[0])["displacement"]
    y = F.elastic(x, disp, fill=7)
    torch.cuda.synchronize()
    ends = torch.stack([x[0].cpu(), x[-1].cpu()])
    want = ref_elastic_image(ends, disp.cpu(), fill=7)
    assert_matches_reference(y[0], want[0], "first plane")
    assert_matches_reference(y[-1], want[1], "last plane")
    del x, y
    torch.cuda.empty_cache()


@pytest.mark.parametrize("offset", [37, 64])
@pytest.mark.parametrize("w", [61, 62, 63, 64, 257])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_canary_ragged_widths(w, dtype, mode, offset):
    """The output placed inside a larger sentinel-filled buffer (at an odd element offset, or an aligned one that lets widths
    w % 4 == 0 take the vector stores): nothing outside it changes, the input is unchanged, and the result equals the
    reference."""
    h, planes = 9, 6
    img = _image((2, 3, h, w), dtype, seed=w)
    x = img.cuda()
    torch.manual_seed(w)
    disp = transforms.ElasticTransform(alpha=200.0, sigma=2.0).get_params(x)["displacement"]
    n = planes * h * w
    sentinel = 0xA5 if dtype == torch.uint8 else -7.25
    buf = torch.full((n + 2 * offset,), sentinel, dtype=dtype, device="cuda")
    y = buf[offset: offset + n]
    d = disp.contiguous()
    bx, by = F._identity_grid_vectors(h, w, x.device)
    lib = _lib.load()
    fn = lib.mv_elastic_u8 if dtype == torch.uint8 else lib.mv_elastic_f32
    fill = _lib.taps([3.0, 4.0, 5.0])
    _lib.check(fn(x.data_ptr(), y.data_ptr(), planes, 3, h, w, bx.data_ptr(), by.data_ptr(), d.data_ptr(), d.stride(1), d.stride(2),
                  d.stride(3), 0 if mode == "bilinear" else 1, fill, _lib.stream_ptr(x)))
    torch.cuda.synchronize()
    host = buf.cpu()
    assert (host[:offset] == sentinel).all() and (host[offset + n:] == sentinel).all()
    assert torch.equal(x.cpu(), img)
    assert_matches_reference(y.reshape(img.shape), ref_elastic_image(img, disp.cpu(), mode=mode, fill=[3.0, 4.0, 5.0]),
                             f"w={w}")


def test_transform_on_a_sample_matches_the_reference():
    """ElasticTransform(fill=...) on {Image u8, Mask u8, Video f32} under a fixed seed equals the reference applied with the
    field get_params draws under the same seed; masks use nearest; the second pure tensor passes through."""
    h, w = 64, 96
    img = tv_tensors.Image(_image((3, h, w), torch.uint8, 1).cuda())
    mask = tv_tensors.Mask((_image((h, w), torch.uint8, 2) % 5).cuda())
    video = tv_tensors.Video(_image((2, 3, h, w), torch.float32, 3).cuda())
    plain = _image((3, h, w), torch.float32, 4).cuda()
    plain_copy = plain.clone()
    for fill in (0, 127, {tv_tensors.Image: [10, 20, 30], tv_tensors.Mask: 255, "others": None}):
        tr = transforms.ElasticTransform(alpha=60.0, sigma=4.0, fill=fill)
        torch.manual_seed(21)
        out = tr({"image": img, "mask": mask, "video": video, "plain": plain})
        torch.manual_seed(21)
        disp = tr.get_params(img, mask, video)["displacement"].cpu()
        f_img = transforms._get_fill(tr._fill, tv_tensors.Image)
        f_mask = transforms._get_fill(tr._fill, tv_tensors.Mask)
        f_vid = transforms._get_fill(tr._fill, tv_tensors.Video)
        assert type(out["image"]) is tv_tensors.Image and type(out["mask"]) is tv_tensors.Mask
        assert type(out["video"]) is tv_tensors.Video and out["plain"] is plain and torch.equal(plain, plain_copy)
        plain_img = img.as_subclass(torch.Tensor).cpu()
        assert_matches_reference(out["image"].as_subclass(torch.Tensor), ref_elastic_image(plain_img, disp, fill=f_img),
                                 f"image {fill}")
        m_ref = ref_elastic_image(mask.as_subclass(torch.Tensor).cpu().unsqueeze(0), disp, mode="nearest", fill=f_mask).squeeze(0)
        assert_matches_reference(out["mask"].as_subclass(torch.Tensor), m_ref, f"mask {fill}")
        v_ref = ref_elastic_image(video.as_subclass(torch.Tensor).cpu(), disp, fill=f_vid)
        assert_matches_reference(out["video"].as_subclass(torch.Tensor), v_ref, f"video {fill}")


def test_pil_round_trip_matches_the_reference():
    if _pil.PIL is None:
        pytest.skip("PIL is not installed")
    arr = _image((40, 56, 3), torch.uint8, 9).numpy()
    pic = _pil.PIL.Image.fromarray(arr, mode="RGB")
    tr = transforms.ElasticTransform(alpha=40.0, sigma=3.0, fill=[1, 2, 3])
    torch.manual_seed(8)
    got = tr(pic)
    torch.manual_seed(8)
    disp = tr.get_params(pic)["displacement"].cpu()
    want = _pil.to_pil_image(ref_elastic_image(_pil.pil_to_tensor(pic), disp, fill=[1.0, 2.0, 3.0]), mode="RGB")
    assert got.mode == "RGB" and got.size == pic.size
    if EXACT:
        assert np.array_equal(np.asarray(got), np.asarray(want))
    else:
        assert np.abs(np.asarray(got).astype(int) - np.asarray(want).astype(int)).max() <= 1


def test_runs_on_the_current_stream():
    img = _image((2, 3, 97, 130), torch.float32, 12).cuda()
    torch.manual_seed(4)
    disp = transforms.ElasticTransform().get_params(img)["displacement"]
    want = F.elastic(img, disp, fill=0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = F.elastic(img, disp, fill=0)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert_matches_reference(got, ref_elastic_image(img.cpu(), disp.cpu(), fill=0))


def test_bool_mask_and_forward_only():
    h, w = 33, 47
    torch.manual_seed(2)
    m = tv_tensors.Mask((torch.rand(1, h, w) > 0.5).cuda())
    disp = transforms.ElasticTransform(alpha=70.0, sigma=3.0).get_params(m)["displacement"]
    got = F.elastic(m, disp, fill=0)
    assert type(got) is tv_tensors.Mask and got.dtype == torch.bool
    assert torch.equal(got.cpu().as_subclass(torch.Tensor),
                       ref_elastic_image(m.cpu().as_subclass(torch.Tensor), disp.cpu(), mode="nearest", fill=0))
    x = torch.rand(3, h, w, device="cuda", requires_grad=True)
    y = F.elastic(x, disp)
    with pytest.raises(RuntimeError, match="forward-only"):
        y.sum().backward()
