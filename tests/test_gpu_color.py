"""F.adjust_brightness / adjust_contrast / adjust_saturation / adjust_hue / rgb_to_grayscale and ColorJitter / Grayscale /
RandomGrayscale on the MI355X (`-m gpu`) against the reference's own computation on the host CPU: torchvision 0.20's v2
_color.py restated with the same torch ops in tests/_color_ref.py.  Brightness, saturation, hue and grayscale are the
reference's bits.  Contrast is the library's exact form (the fused blend against the mean -- uint8 from the exact integer sum,
float32 correctly rounded), checked bit for bit against the host emulation, and the reference's blend against that mean is
checked to take only the fused or the plain rounding (tests/_color_ref.check_contrast_reference)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, functional as F, transforms, tv_tensors  # noqa: E402
from tests._color_ref import (REF_OPS, check_contrast_reference, emu_chain, emu_grayscale, emu_mean,  # noqa: E402
                              ref_chain, ref_contrast_mean, ref_rgb_to_grayscale)

SIZES = [(1, 1), (1, 257), (7, 9), (224, 224), (375, 500), (1080, 1920)]
FACTORS = [0.0, 0.5, 1.0, 1.7, 50.0]
HUES = [-0.5, -0.27, 0.0, 0.1, 0.5]
FUNCS = {"brightness": F.adjust_brightness, "contrast": F.adjust_contrast, "saturation": F.adjust_saturation,
         "hue": F.adjust_hue}


def _image(shape, dtype, seed, special=None):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    else:
        x = torch.rand(shape, generator=g)
    if special == "grey":  # r = g = b
        x = x[..., :1, :, :].expand(shape).contiguous()
    elif special == "primaries":
        hi = 255 if dtype == torch.uint8 else 1.0
        x = torch.zeros(shape, dtype=dtype)
        idx = torch.arange(shape[-1]) % 3
        for c in range(shape[-3]):
            x[..., c, :, :] = (idx == c).to(dtype) * hi
    elif special == "zeros":
        x = torch.zeros(shape, dtype=dtype)
    elif special == "full":
        x = torch.full(shape, 255 if dtype == torch.uint8 else 1.0, dtype=dtype)
    elif special == "outside":  # float inputs outside [0, 1]
        x = x * 3.0 - 1.0
    return x


def _check(name, x, f, got):
    got = got.cpu()
    if name == "contrast":
        check_contrast_reference(x, f, got)
        if x.dtype == torch.uint8 and x.shape[-1] * x.shape[-2] <= 256 * 256:  # ATen's float sum is exact there
            assert torch.equal(torch.from_numpy(emu_mean(x.numpy().astype(np.float32), True)), ref_contrast_mean(x))
    else:
        want = REF_OPS[name](x, f)
        assert torch.equal(got, want), f"{name} {f}: {(got != want).sum().item()} elements differ"
        assert torch.equal(got, emu_chain(x, [(name, f)]))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("name", ["brightness", "contrast", "saturation", "hue"])
def test_each_op_matches_the_reference(name, dtype, c, size):
    x = _image((2, c) + size, dtype, seed=size[0] * 7 + size[1] + c)
    xd = x.cuda()
    for f in (HUES if name == "hue" else FACTORS):
        _check(name, x, f, FUNCS[name](xd, f))


@pytest.mark.parametrize("dtype,special", [(d, s) for d in (torch.float32, torch.uint8)
                                           for s in ("grey", "primaries", "zeros", "full", "outside")
                                           if not (s == "outside" and d == torch.uint8)])  # uint8 has no values outside
@pytest.mark.parametrize("name", ["brightness", "contrast", "saturation", "hue"])
def test_special_pixels(name, dtype, special):
    x = _image((3, 3, 33, 47), dtype, seed=5, special=special)
    xd = x.cuda()
    for f in (HUES if name == "hue" else FACTORS):
        _check(name, x, f, FUNCS[name](xd, f))


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
def test_batches_videos_views_and_empty_images(dtype):
    x = _image((2, 4, 3, 19, 37), dtype, seed=11)  # a 5-D video batch: contrast's mean is per frame
    for name in FUNCS:
        f = 0.1 if name == "hue" else 0.6
        got = FUNCS[name](tv_tensors.Video(x.cuda()), f)
        assert type(got) is tv_tensors.Video
        _check(name, x, f, got.as_subclass(torch.Tensor))
    big = _image((2, 3, 40, 60), dtype, seed=12)
    crop = big[:, :, 3:30, 5:50]  # a cropped view
    cl = big.contiguous(memory_format=torch.channels_last)
    for name in FUNCS:
        f = -0.2 if name == "hue" else 1.3
        _check(name, crop.contiguous(), f, FUNCS[name](big.cuda()[:, :, 3:30, 5:50], f))
        _check(name, big, f, FUNCS[name](cl.cuda(), f))
    empty = torch.empty((0, 3, 8, 8), dtype=dtype, device="cuda")
    for name in FUNCS:
        out = FUNCS[name](empty, 0.1 if name == "hue" else 0.5)
        assert out.shape == empty.shape
    assert F.adjust_hue(empty, 0.1) is empty
    one = _image((3, 1, 8, 8), dtype, seed=13).cuda()
    assert F.adjust_saturation(one, 0.3) is one and F.adjust_hue(one, 0.3) is one


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("c", [1, 3])
def test_grayscale_matches_the_reference(c, dtype):
    x = _image((2, c, 75, 101), dtype, seed=21)
    for n in (1, 3):
        got = F.rgb_to_grayscale(x.cuda(), num_output_channels=n).cpu()
        want = ref_rgb_to_grayscale(x, n)
        assert got.shape == want.shape and torch.equal(got, want)
        if c == 3:
            assert torch.equal(got, emu_grayscale(x, n))
        got = transforms.Grayscale(num_output_channels=n)(tv_tensors.Image(x.cuda()))
        assert type(got) is tv_tensors.Image and torch.equal(got.as_subclass(torch.Tensor).cpu(), want)
    got = transforms.RandomGrayscale(p=1.0)(x.cuda()).cpu()
    assert torch.equal(got, ref_rgb_to_grayscale(x, c))


def _jitter_cases():
    return [(0.4, 0.4, 0.4, 0.1), (0.0, 0.5, 0.0, 0.0), ((0.5, 0.5), None, (1.5, 1.5), (-0.2, -0.2)),
            (None, (0.2, 0.9), None, 0.5)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("args", _jitter_cases(), ids=["standard", "contrast_only", "fixed", "contrast_hue"])
def test_color_jitter_matches_the_reference_over_seeds(args, dtype):
    t = transforms.ColorJitter(*args)
    x = _image((2, 3, 57, 91), dtype, seed=31)
    xd = x.cuda()
    positions = set()
    for seed in range(24):
        torch.manual_seed(seed)
        params = t._get_params([xd])
        torch.manual_seed(seed)
        got = t(xd).cpu()
        ops = [(n, params[n + "_factor"]) for n in (("brightness", "contrast", "saturation", "hue")[int(i)]
                                                    for i in params["fn_idx"]) if params[n + "_factor"] is not None]
        if params["contrast_factor"] is not None:
            positions.add(int((params["fn_idx"] == 1).nonzero()))
        assert torch.equal(got, emu_chain(x, ops)), (seed, ops)
        if dtype == torch.uint8 or not any(n == "contrast" for n, _ in ops):
            assert torch.equal(got, ref_chain(x, ops)), (seed, ops)
        loop = xd
        for n, f in ops:  # the four single GPU calls
            loop = FUNCS[n](loop, f)
        assert torch.equal(got, loop.cpu()), (seed, ops)
    if t.contrast is not None:  # contrast took every position in the order
        assert positions == {0, 1, 2, 3}


def test_color_jitter_types_and_passthrough():
    t = transforms.ColorJitter(0.4, 0.4, 0.4, 0.1)
    img = tv_tensors.Image(_image((3, 20, 30), torch.uint8, seed=41).cuda())
    vid = tv_tensors.Video(_image((2, 3, 20, 30), torch.float32, seed=42).cuda())
    mask = tv_tensors.Mask(torch.ones(20, 30, dtype=torch.uint8, device="cuda"))
    out = t({"image": img, "video": vid, "mask": mask})
    assert type(out["image"]) is tv_tensors.Image and type(out["video"]) is tv_tensors.Video
    assert out["mask"] is mask


def test_float_contrast_is_repeatable():
    x = _image((4, 3, 541, 769), torch.float32, seed=51).cuda()
    first = F.adjust_contrast(x, 0.7)
    for _ in range(5):
        assert torch.equal(F.adjust_contrast(x, 0.7), first)


def test_uint8_above_2_pow_31_elements():
    n = (1 << 31) // (3 * 1080 * 1920) + 1  # 346 frames, 2.15e9 elements
    x = torch.empty((n, 3, 1080, 1920), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    x.random_(0, 256, generator=g)
    y = F.adjust_saturation(x, 0.7)
    z = F.adjust_contrast(x, 1.4)
    for k in (0, n // 2, n - 1):
        xf = x[k:k + 1].cpu()
        assert torch.equal(y[k:k + 1].cpu(), REF_OPS["saturation"](xf, 0.7)), k
        assert torch.equal(z[k:k + 1].cpu(), emu_chain(xf, [("contrast", 1.4)])), k
    del x, y, z
    torch.cuda.empty_cache()


def test_color_jitter_in_a_captured_graph():
    x = _image((4, 3, 64, 96), torch.uint8, seed=61).cuda()
    ops = [("hue", 0.1), ("contrast", 1.3), ("brightness", 0.8), ("saturation", 1.2)]
    eager = F.color_jitter_image(x, ops)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.color_jitter_image(x, ops)  # warm-up (library load, probes) outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = F.color_jitter_image(x, ops)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_float_output_is_forward_only():
    x = _image((1, 3, 8, 8), torch.float32, seed=71).cuda().requires_grad_(True)
    y = F.adjust_brightness(x, 0.5)
    with pytest.raises(RuntimeError, match="forward-only"):
        y.sum().backward()
    assert _lib.last_kernel().startswith("k_color<f32,c3")
