"""pad / crop / flip / resized_crop / erase and their transforms on the GPU against the reference restated on the CPU
(tests/_crop_ref.py).  Pad, crop, flip and erase move bytes: torch.equal on any host.  resized_crop follows
assert_matches_reference's rule (exact where the host's interpolate is the AVX2 / AVX512 kernel)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, functional as F, transforms, tv_tensors  # noqa: E402
from oracle import ref as oracle  # noqa: E402
from tests import _crop_ref as R  # noqa: E402
from tests.test_gpu_warp import assert_matches_reference  # noqa: E402

MODES = ["constant", "edge", "reflect", "symmetric"]
DTYPES = [torch.uint8, torch.float32, torch.bool, torch.float16, torch.int64]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _image(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.bool:
        return torch.rand(shape, generator=g) > 0.5
    if dtype.is_floating_point:
        return torch.rand(shape, generator=g, dtype=torch.float32).to(dtype)
    return torch.randint(0, 256 if dtype == torch.uint8 else 1000, shape, generator=g).to(dtype)


def _equal(got, want, what=""):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert torch.equal(got, want), what


# ---- pad --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("mode", MODES)
def test_pad_modes_dtypes_shapes(mode, dtype):
    if dtype == torch.int64 and mode in ("edge", "reflect"):
        with pytest.raises(NotImplementedError):
            F.pad(_image((1, 9, 9), dtype, 0).cuda(), 2, padding_mode=mode)
        return
    for k, shape in enumerate([(3, 37, 53), (2, 3, 20, 33), (2, 2, 3, 18, 17), (1, 7, 130)]):
        x = _image(shape, dtype, seed=k)
        for padding in (3, [2, 5], [1, 2, 3, 4], [-2, 3, -1, 4], [4, -3, 0, -2], [0, 0, 0, 0]):
            _equal(F.pad(x.cuda(), padding, padding_mode=mode), R.pad_image(x, padding, padding_mode=mode), (shape, padding))
    x = _image((3, 21, 1921), dtype, seed=9)
    _equal(F.pad(x.cuda(), 4, padding_mode=mode), R.pad_image(x, 4, padding_mode=mode), "odd width")
    sliced = _image((3, 30, 70), dtype, seed=10)
    _equal(F.pad(sliced.cuda()[:, 1:, 3:], [5, 2], padding_mode=mode), R.pad_image(sliced[:, 1:, 3:], [5, 2], padding_mode=mode),
           "unaligned base")


def test_pad_fills_and_masks():
    x = _image((2, 3, 19, 35), torch.uint8, seed=1)
    for fill in (7, 3.7, [9], [1, 2, 3], [1.9, 250.2, 3.0]):
        _equal(F.pad(x.cuda(), [3, 1, -2, 4], fill=fill), R.pad_image(x, [3, 1, -2, 4], fill=fill), fill)
    xf = _image((3, 19, 35), torch.float32, seed=2)
    for fill in (0.25, [0.1, 0.2, 0.3], None):
        _equal(F.pad(xf.cuda(), 6, fill=fill), R.pad_image(xf, 6, fill=fill), fill)
    m2 = _image((23, 41), torch.int64, seed=3)  # a 2-D mask
    for mode in ("constant", "symmetric"):
        got = F.pad(tv_tensors.Mask(m2.cuda()), [2, 3], padding_mode=mode)
        assert isinstance(got, tv_tensors.Mask)
        _equal(got.as_subclass(torch.Tensor), R.pad_mask(m2, [2, 3], padding_mode=mode), mode)
    mb = _image((2, 23, 41), torch.bool, seed=4)
    _equal(F.pad(tv_tensors.Mask(mb.cuda()), 3, fill=1).as_subclass(torch.Tensor), R.pad_mask(mb, 3, fill=1))
    assert isinstance(F.pad(tv_tensors.Image(x.cuda()), 1), tv_tensors.Image)
    empty = torch.zeros((0, 3, 5, 5), dtype=torch.uint8, device="cuda")
    assert F.pad(empty, 2).shape == (0, 3, 9, 9)
    got = transforms.Pad([1, 2], fill=5, padding_mode="constant")(x.cuda())
    _equal(got, R.pad_image(x, [1, 2], fill=5))


# ---- flips --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16, torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("w", [1, 15, 16, 17, 1000, 1921])
def test_flips(w, dtype):
    x = _image((2, 3, 7, w), dtype, seed=w)
    h, v = F.horizontal_flip(x.cuda()), F.vertical_flip(x.cuda())
    _equal(h, x.flip(-1)), _equal(v, x.flip(-2))
    assert h.data_ptr() != x.data_ptr()
    _equal(F.hflip(x.cuda()[..., 1:, :]), x[..., 1:, :].flip(-1))
    _equal(F.vflip(tv_tensors.Mask(x[0, 0].cuda())).as_subclass(torch.Tensor), x[0, 0].flip(-2))


# ---- crop ---------------------------------------------------------------------------------------------------------------------------
def test_crop_view_and_outside():
    x = _image((2, 3, 40, 60), torch.uint8, seed=5)
    xd = x.cuda()
    view = F.crop(xd, 3, 5, 20, 30)
    assert view.data_ptr() == xd.data_ptr() + 3 * 60 + 5 and view.stride() == xd.stride()
    _equal(view, x[..., 3:23, 5:35])
    for box in ((-4, 5, 20, 30), (3, -7, 20, 30), (30, 5, 20, 30), (3, 40, 20, 30), (-5, -5, 50, 70), (-30, 0, 10, 10),
                (0, 70, 10, 10), (45, 65, 8, 8)):
        _equal(F.crop(xd, *box), R.crop_image(x, *box), box)
    xf = _image((3, 33, 47), torch.float32, seed=6)
    _equal(F.crop(xf.cuda(), -2, 10, 40, 50), R.crop_image(xf, -2, 10, 40, 50))


def test_random_crop_with_padding_is_one_launch():
    x = _image((8, 3, 32, 32), torch.uint8, seed=7)
    xd = x.cuda()
    for mode in MODES:
        t = transforms.RandomCrop(32, padding=4, padding_mode=mode, fill=3)
        for seed in range(6):
            torch.manual_seed(seed)
            got = t(xd)
            assert _lib.last_kernel().startswith("k_gather<b1")
            torch.manual_seed(seed)
            p = R.random_crop_params(32, 32, (32, 32), padding=4)
            want = R.pad_image(x, p["padding"], fill=3, padding_mode=mode)
            want = want[..., p["top"]:p["top"] + 32, p["left"]:p["left"] + 32]
            _equal(got, want, (mode, seed))
    t = transforms.RandomCrop((40, 20), pad_if_needed=True)
    torch.manual_seed(1)
    got = t(xd)
    torch.manual_seed(1)
    p = R.random_crop_params(32, 32, (40, 20), pad_if_needed=True)
    want = R.pad_image(x, p["padding"], fill=0)[..., p["top"]:p["top"] + 40, p["left"]:p["left"] + 20]
    _equal(got, want)


# ---- resized_crop -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=str)
@pytest.mark.parametrize("hw, box, size", [
    ((375, 500), (20, 30, 300, 400), (224, 224)),      # scale 1-7: the fused kernel
    ((375, 500), (-10, -20, 300, 400), (224, 200)),    # reaches outside on the top / left
    ((375, 500), (200, 300, 250, 300), (128, 160)),    # reaches outside on the bottom / right
    ((100, 120), (10, 10, 40, 50), (224, 224)),        # upsampling
    ((1080, 1920), (8, 100, 1000, 1800), (64, 96)),    # scale above 7: two kernels
    ((1080, 1920), (-40, 1000, 1100, 1000), (64, 96)),
    ((300, 300), (50, 60, 100, 224), (200, 224)),      # identity along the width
])
def test_resized_crop_against_interpolate_and_the_oracle(hw, box, size, dtype):
    x = _image((2, 3) + hw, dtype, seed=11)
    got = F.resized_crop(x.cuda(), *box, list(size))
    cropped = R.crop_image(x, *box)
    assert_matches_reference(got, R.resize_image(cropped, size), "interpolate")
    want = torch.from_numpy(oracle.resize(cropped.numpy(), list(size)))
    assert torch.equal(got.cpu(), want), "oracle"
    two_kernels = max(box[2] / size[0], box[3] / size[1]) > 7
    assert ("k_resize_h" == _lib.last_kernel()) if two_kernels else ("k_resize_fused" in _lib.last_kernel()), _lib.last_kernel()


def test_resized_crop_whole_image_and_same_size():
    for dtype in (torch.uint8, torch.float32):
        x = _image((2, 3, 375, 500), dtype, seed=12).cuda()
        assert torch.equal(F.resized_crop(x, 0, 0, 375, 500, [224, 224]), F.resize(x, [224, 224]))
        assert torch.equal(F.resized_crop(x, 0, 0, 375, 500, [64]), F.resize(x, [64]))
        same = F.resized_crop(x, 5, 6, 100, 120, [100, 120])
        assert same.data_ptr() == x[..., 5:, 6:].data_ptr() and torch.equal(same, x[..., 5:105, 6:126])


def test_resized_crop_flip_normalize_equals_the_composed_calls():
    for dtype in (torch.uint8, torch.float32):
        x = _image((4, 3, 375, 500), dtype, seed=13).cuda()
        for box, flip in (((20, 30, 300, 400), True), ((20, 30, 300, 400), False), ((-9, 250, 200, 300), True)):
            got = F.resized_crop_flip_normalize(x, *box, [224, 224], flip, MEAN, STD)
            y = F.resized_crop(x, *box, [224, 224])
            if flip:
                y = F.horizontal_flip(y)
            want = F.normalize(F.to_dtype(y, torch.float32, scale=True), MEAN, STD)
            assert torch.equal(got, want), (dtype, box, flip)


def test_training_pipeline_in_compose():
    x = _image((3, 375, 500), torch.uint8, seed=14)
    pipe = transforms.Compose([transforms.RandomResizedCrop(224), transforms.RandomHorizontalFlip(),
                               transforms.ToDtype(torch.float32, scale=True), transforms.Normalize(MEAN, STD),
                               transforms.RandomErasing(p=0.7, value="random")])
    flipped = erased = 0
    for seed in range(24):
        torch.manual_seed(seed)
        got = pipe(x.cuda())
        torch.manual_seed(seed)
        p, _ = R.random_resized_crop_params(375, 500)
        want = R.resized_crop_image(x, p["top"], p["left"], p["height"], p["width"], (224, 224))
        if torch.rand(1) < 0.5:
            want = want.flip(-1)
            flipped += 1
        want = R.to_float_normalize(want, MEAN, STD)
        if torch.rand(1) < 0.7:
            e, _ = R.random_erasing_params(3, 224, 224, value=None)
            if e["v"] is not None:
                want = R.erase_image(want, e["i"], e["j"], e["h"], e["w"], e["v"])
                erased += 1
        assert_matches_reference(got, want, f"seed {seed}")
    assert 0 < flipped < 24 and 0 < erased < 24


# ---- erase --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float16], ids=str)
def test_erase(dtype):
    x = _image((2, 3, 45, 67), dtype, seed=15)
    g = torch.Generator().manual_seed(1)
    for (i, j, h, w) in ((5, 9, 20, 33), (0, 0, 45, 67), (44, 66, 1, 1), (10, 3, 0, 5), (7, 30, 16, 16)):
        for v in (torch.tensor([0.5, 100.7, 3.2])[:, None, None], torch.rand((3, h, w), generator=g) * 200,
                  torch.tensor([[[7.9]]])):
            xd = x.cuda()
            keep = xd.clone()
            out = F.erase(xd, i, j, h, w, v)
            _equal(out, R.erase_image(x, i, j, h, w, v), (i, j, h, w, tuple(v.shape)))
            assert torch.equal(xd, keep) and out.data_ptr() != xd.data_ptr()
            inplace = F.erase(xd, i, j, h, w, v.cuda(), inplace=True)
            assert inplace.data_ptr() == xd.data_ptr()
            _equal(xd, R.erase_image(x, i, j, h, w, v))
    img = tv_tensors.Image(x.cuda())
    assert isinstance(F.erase(img, 1, 1, 2, 2, torch.zeros(3, 1, 1)), tv_tensors.Image)


def test_random_erasing_transform():
    x = _image((4, 3, 64, 80), torch.float32, seed=16)
    for value in (0.0, (0.1, 0.2, 0.3), "random"):
        t = transforms.RandomErasing(p=1.0, value=value)
        for seed in range(4):
            torch.manual_seed(seed)
            got = t(x.cuda())
            torch.manual_seed(seed)
            torch.rand(1)
            ref_value = None if value == "random" else ([value] if isinstance(value, float) else list(value))
            e, ok = R.random_erasing_params(3, 64, 80, value=ref_value)
            want = R.erase_image(x, e["i"], e["j"], e["h"], e["w"], e["v"]) if ok else x
            _equal(got, want, (value, seed))


# ---- graphs, large batches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pad", "hflip", "crop", "erase", "erase_inplace", "resized_crop", "resized_crop_two_kernels",
                                  "resized_crop_flip_normalize"])
def test_in_a_captured_graph(name):
    shape = (2, 3, 1080, 1920) if name == "resized_crop_two_kernels" else (4, 3, 120, 160)
    x = _image(shape, torch.uint8, seed=3).cuda()
    v = torch.tensor([1, 2, 3], dtype=torch.uint8, device="cuda")[:, None, None]
    fn = {"pad": lambda t: F.pad(t, [3, 5], fill=[1, 2, 3]), "hflip": F.horizontal_flip,
          "crop": lambda t: F.crop(t, -3, 10, 100, 200), "erase": lambda t: F.erase(t, 10, 20, 30, 40, v),
          "erase_inplace": lambda t: F.erase(t.clone(), 10, 20, 30, 40, v, inplace=True),
          "resized_crop": lambda t: F.resized_crop(t, 5, -6, 100, 140, [64, 64]),
          "resized_crop_two_kernels": lambda t: F.resized_crop(t, 5, 6, 1000, 1800, [64, 64]),
          "resized_crop_flip_normalize": lambda t: F.resized_crop_flip_normalize(t, 5, 6, 100, 140, [64, 64], True, MEAN, STD)}[name]
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
    x.copy_(_image(shape, torch.uint8, seed=4).cuda())
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fn(x))


def test_gather_above_2_pow_31_elements():
    h, w = 1080, 1920
    planes = (2 ** 31) // (h * w) + 2
    assert planes * h * w > 2 ** 31
    x = torch.empty((planes, 1, h, w), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    x[0].random_(0, 256, generator=g)
    x[-1].random_(0, 256, generator=g)
    y = F.horizontal_flip(x)
    for k in (0, planes - 1):
        assert torch.equal(y[k].cpu(), x[k].cpu().flip(-1)), k
    del y
    y = F.pad(x, [3, 2, 1, 4], padding_mode="reflect")
    for k in (0, planes - 1):
        assert torch.equal(y[k].cpu(), R.pad_image(x[k].cpu(), [3, 2, 1, 4], padding_mode="reflect")), k
