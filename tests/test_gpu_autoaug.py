"""F.invert / posterize / solarize / autocontrast / equalize, the Random* colour transforms and AutoAugment / RandAugment /
TrivialAugmentWide on the MI355X (`-m gpu`) against the reference's own computation on the host CPU: torchvision 0.20's v2
_color.py and _auto_augment.py restated with the same torch ops in tests/_autoaug_ref.py.  Every op is the reference's bits;
float equalize outside [0, 1] is the library's documented saturation."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import functional as F, transforms, tv_tensors  # noqa: E402
from tests._autoaug_ref import (REF_OPS, ref_apply, ref_autoaugment_draws, ref_randaugment_draws,  # noqa: E402
                                ref_trivialaugment_draws)
from tests._color_ref import REF_OPS as COLOR_REF  # noqa: E402

SIZES = [(1, 1), (1, 257), (7, 9), (224, 224), (375, 500), (1080, 1920)]
CHANNELS = {"invert": [1, 3, 4], "posterize": [1, 3, 4], "solarize": [1, 3, 4], "autocontrast": [1, 3], "equalize": [1, 3, 4]}


def _params(name, dtype, x):
    if name == "posterize":
        return [dict(bits=b) for b in (0, 1, 4, 7, 8)]
    if name == "solarize":
        v = x.flatten()[x.numel() // 2].item()  # a threshold equal to a pixel value (not above the bound)
        v = v if v <= (255 if dtype == torch.uint8 else 1.0) else 0.75
        if dtype == torch.uint8:
            return [dict(threshold=t) for t in (0, 1, 100.3, 127.5, 128, 255, 254.9999999, -1, v, float(v))]
        return [dict(threshold=t) for t in (0.0, 0.3, 0.5, 1.0, 1, 0.49999999999, v, -0.5)]
    return [{}]


def _image(shape, dtype, seed, special=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) if dtype == torch.uint8 else torch.rand(shape, generator=g)
    hi = 255 if dtype == torch.uint8 else 1.0
    if special == "constant":
        x = torch.full(shape, 77 if dtype == torch.uint8 else 0.3, dtype=dtype)
    elif special == "two":
        x = torch.where(x > hi / 2, torch.tensor(hi, dtype=dtype), torch.tensor(hi / 4, dtype=dtype)).to(dtype)
    elif special == "zeros":
        x = torch.zeros(shape, dtype=dtype)
    elif special == "full":
        x = torch.full(shape, hi, dtype=dtype)
    elif special == "step0":  # fewer than 255 pixels below the plane's maximum: equalize's step == 0
        x = torch.full(shape, hi, dtype=dtype)
        x.view(-1, shape[-2] * shape[-1])[:, :200] = torch.tensor(hi / 5, dtype=dtype)
    elif special == "outside":
        x = x * 3.0 - 1.0
    elif special == "nan":
        x = x.clone()
        x.view(-1)[x.numel() // 3] = float("nan")
    return x


def _same(got, want):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.is_floating_point():
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(got[~nan], want[~nan])
    else:
        assert torch.equal(got, want)


def _run(name, x, kw):
    return getattr(F, name)(x.cuda(), **kw)


@pytest.mark.parametrize("name", list(CHANNELS))
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("hw", SIZES)
def test_op_matches_reference(name, dtype, hw):
    for c in CHANNELS[name]:
        x = _image((c,) + hw, dtype, seed=hw[0] * 7 + c)
        for kw in _params(name, dtype, x):
            _same(_run(name, x, kw), REF_OPS[name](x, **kw))


SPECIALS = [(dtype, s) for dtype in (torch.uint8, torch.float32) for s in ("constant", "two", "zeros", "full", "step0")]
SPECIALS += [(torch.float32, "outside"), (torch.float32, "nan")]


@pytest.mark.parametrize("name", list(CHANNELS))
@pytest.mark.parametrize("dtype,special", SPECIALS)
def test_special_planes(name, dtype, special):
    if special == "nan" and name == "equalize":
        special = "outside"  # NaN is saturated like the values outside [0, 1]
    for hw in [(7, 9), (64, 80), (375, 500)]:
        x = _image((2, 3) + hw, dtype, seed=1, special=special)
        for kw in _params(name, dtype, x):
            _same(_run(name, x, kw), REF_OPS[name](x, **kw))


@pytest.mark.parametrize("name", list(CHANNELS))
def test_batches_videos_views_and_empty(name):
    for dtype in (torch.uint8, torch.float32):
        x = _image((2, 4, 3, 33, 47), dtype, seed=5)
        kw = _params(name, dtype, x)[-1]
        want = REF_OPS[name](x, **kw)
        got = getattr(F, name)(tv_tensors.Video(x.cuda()), **kw)
        assert isinstance(got, tv_tensors.Video)
        _same(got.as_subclass(torch.Tensor), want)
        img = getattr(F, name)(tv_tensors.Image(x[0, 0].cuda()), **kw)
        assert isinstance(img, tv_tensors.Image)
        _same(img.as_subclass(torch.Tensor), REF_OPS[name](x[0, 0], **kw))
        view = x.cuda().transpose(-1, -2)[..., 3:, :]  # not contiguous
        _same(getattr(F, name)(view, **kw), REF_OPS[name](x.transpose(-1, -2)[..., 3:, :].contiguous(), **kw))
        empty = torch.zeros((0, 3, 5, 5), dtype=dtype, device="cuda")
        out = getattr(F, name)(empty, **kw)
        assert out.shape == empty.shape and out.dtype == dtype


def test_uint8_above_2_pow_31_elements():
    n = (1 << 31) // (3 * 1080 * 1920) + 1
    x = torch.empty((n, 3, 1080, 1920), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    x.random_(0, 256, generator=g)
    y = F.equalize(x)
    for k in (0, n // 2, n - 1):
        assert torch.equal(y[k:k + 1].cpu(), REF_OPS["equalize"](x[k:k + 1].cpu())), k
    del y
    z = F.solarize(x, 100)
    for k in (0, n - 1):
        assert torch.equal(z[k:k + 1].cpu(), REF_OPS["solarize"](x[k:k + 1].cpu(), 100)), k
    assert torch.equal(z[-1, -1, -1, -16:].cpu(), REF_OPS["solarize"](x[-1, -1, -1, -16:].cpu(), 100))
    del x, z
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["equalize", "autocontrast"])
def test_in_a_captured_graph(name):
    x = _image((4, 3, 120, 160), torch.uint8, seed=3).cuda()
    fn = getattr(F, name)
    eager = fn(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(x)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(_image((4, 3, 120, 160), torch.uint8, seed=4).cuda())
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), REF_OPS[name](x.cpu()))


@pytest.mark.parametrize("name", list(CHANNELS))
def test_float_outputs_raise_on_backward(name):
    x = torch.rand(3, 8, 8, device="cuda", requires_grad=True)
    y = getattr(F, name)(x, **_params(name, torch.float32, x.detach())[0])
    with pytest.raises(Exception):
        y.sum().backward()


@pytest.mark.parametrize("cls,kw,name,fkw", [
    (transforms.RandomInvert, {}, "invert", {}),
    (transforms.RandomPosterize, {"bits": 3}, "posterize", {"bits": 3}),
    (transforms.RandomSolarize, {"threshold": 100.5}, "solarize", {"threshold": 100.5}),
    (transforms.RandomAutocontrast, {}, "autocontrast", {}),
    (transforms.RandomEqualize, {}, "equalize", {}),
])
def test_random_transforms(cls, kw, name, fkw):
    x = _image((3, 40, 50), torch.uint8, seed=9)
    t = cls(p=0.5, **kw)
    for seed in range(8):
        torch.manual_seed(seed)
        applied = bool(torch.rand(1) < 0.5)
        torch.manual_seed(seed)
        got = t(tv_tensors.Image(x.cuda()))
        assert isinstance(got, tv_tensors.Image)
        _same(got.as_subclass(torch.Tensor), REF_OPS[name](x, **fkw) if applied else x)


def _policy_case(t, ref_draws, dtype, seeds):
    """Draws, op-by-op pixels and -- where every drawn op has a CPU transcription -- the reference's bits."""
    x = _image((3, 48, 64), dtype, seed=11)
    xd = tv_tensors.Image(x.cuda())
    transcribed = 0
    for seed in seeds:
        calls = []
        orig = t._apply_image_or_video_transform

        def record(image, transform_id, magnitude, interpolation, fill):
            calls.append((transform_id, magnitude))
            return orig(image, transform_id, magnitude, interpolation, fill)

        t._apply_image_or_video_transform = record
        torch.manual_seed(seed)
        got = t(xd)
        del t._apply_image_or_video_transform
        torch.manual_seed(seed)
        assert calls == ref_draws(), seed
        assert isinstance(got, tv_tensors.Image)
        step = xd  # the library's own op-by-op calls
        for op, m in calls:
            step = t._apply_image_or_video_transform(step, op, m, t.interpolation, t._fill)
        _same(got.as_subclass(torch.Tensor), step.as_subclass(torch.Tensor).cpu())
        ref = x
        for op, m in calls:
            if op == "Brightness":
                ref = COLOR_REF["brightness"](ref, 1.0 + m)
            elif op == "Color":
                ref = COLOR_REF["saturation"](ref, 1.0 + m)
            else:
                ref = ref_apply(ref, op, m)
            if ref is None:
                break
        if ref is not None:
            transcribed += 1
            _same(got.as_subclass(torch.Tensor), ref)
    assert transcribed > 0


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("policy", list(transforms.AutoAugmentPolicy))
def test_autoaugment(policy, dtype):
    t = transforms.AutoAugment(policy)
    _policy_case(t, lambda: ref_autoaugment_draws(t._policies, 48, 64), dtype, range(40))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_randaugment(dtype):
    t = transforms.RandAugment()
    _policy_case(t, lambda: ref_randaugment_draws(2, 9, 31, 48, 64), dtype, range(60))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_trivialaugmentwide(dtype):
    t = transforms.TrivialAugmentWide()
    _policy_case(t, lambda: ref_trivialaugment_draws(31, 48, 64), dtype, range(60))


@pytest.mark.parametrize("cls", [transforms.AutoAugment, transforms.RandAugment, transforms.TrivialAugmentWide])
def test_policies_reject_masks_and_boxes(cls):
    image = tv_tensors.Image(torch.zeros(3, 8, 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError, match="not supported"):
        cls()(image, tv_tensors.Mask(torch.zeros(8, 8, dtype=torch.uint8, device="cuda")))
    boxes = tv_tensors.BoundingBoxes(torch.zeros(1, 4))
    with pytest.raises(TypeError, match="not supported"):
        cls()(image, boxes)
