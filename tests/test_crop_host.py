"""pad / crop / flip / resized_crop / erase without a GPU: the kernel's index map against torch's padding routines, the
parameter draws of RandomCrop / RandomResizedCrop / RandomErasing against the restated reference (tests/_crop_ref.py) with the
RNG state afterwards, the reference's argument errors, and the ABI's own argument checks."""
import pytest
import torch

from cpu_vision_amd import _lib, functional as F, transforms, tv_tensors
from tests import _crop_ref as R

SEEDS = range(200)


# ---- the per-axis index map -----------------------------------------------------------------------------------------------------
def _torch_axis(n, before, after, mode):
    """The source index of every output position of one padded axis, by torch itself: pad an arange (fill = -1)."""
    x = torch.arange(n, dtype=torch.float32).reshape(1, 1, 1, n)
    if mode == "symmetric":
        out = R.pad_symmetric(x, [before, after, 0, 0])
    elif mode == "constant":
        out = torch.nn.functional.pad(x, [before, after], mode="constant", value=-1.0)
    else:
        out = torch.nn.functional.pad(x, [before, after, 0, 0], mode={"edge": "replicate", "reflect": "reflect"}[mode])
    return [int(v) for v in out.reshape(-1)]


@pytest.mark.parametrize("mode", ["constant", "edge", "reflect", "symmetric"])
def test_axis_index_map_equals_torch_padding(mode):
    checked = 0
    for n in range(1, 10):
        for before in range(-3, 5):
            for after in range(-3, 5):
                kept = n + min(before, 0) + min(after, 0)
                if kept <= 0 or n + before + after <= 0:
                    continue
                limit = {"reflect": n - 1, "symmetric": kept}.get(mode, 99)
                if max(before, after) > limit:
                    continue
                want = _torch_axis(n, before, after, mode)
                assert F.axis_index_map(n, before, after, mode) == want, (n, before, after)
                assert F.axis_index_map(n, before, after, mode, flip=True) == want[::-1], (n, before, after)
                checked += 1
    assert checked > 150


def test_axis_index_map_rejects_what_one_reflection_cannot_reach():
    with pytest.raises(ValueError, match="less than the corresponding input dimension"):
        F.axis_index_map(4, 4, 0, "reflect")
    with pytest.raises(ValueError, match="exceeds"):
        F.axis_index_map(4, 0, 5, "symmetric")
    with pytest.raises(ValueError, match="padding_mode"):
        F.axis_index_map(4, 1, 1, "wrap")
    assert F.axis_index_map(4, 4, 4, "symmetric") == [3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0]


# ---- parameter draws ------------------------------------------------------------------------------------------------------------
def _same_params(got, want):
    assert set(got) == set(want)
    for k in want:
        if isinstance(want[k], torch.Tensor):
            assert torch.equal(got[k], want[k]), k
        else:
            assert got[k] == want[k] and type(got[k]) is type(want[k]), (k, got[k], want[k])


@pytest.mark.parametrize("kwargs, hw", [
    (dict(size=(32, 32), padding=4), (32, 32)),
    (dict(size=(200, 180)), (224, 256)),
    (dict(size=(64, 300), pad_if_needed=True), (50, 280)),
    (dict(size=(40, 40), padding=[1, 2, 3, 4], pad_if_needed=True, padding_mode="reflect"), (30, 60)),
])
def test_random_crop_draws(kwargs, hw):
    t = transforms.RandomCrop(**kwargs)
    img = torch.zeros((3,) + hw, dtype=torch.uint8)
    ref_kwargs = {k: v for k, v in kwargs.items() if k in ("size", "padding", "pad_if_needed")}
    for seed in SEEDS:
        torch.manual_seed(seed)
        got = t._get_params([img])
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        want = R.random_crop_params(*hw, **ref_kwargs)
        _same_params(got, want)
        assert torch.equal(state, torch.get_rng_state())


@pytest.mark.parametrize("kwargs, hw, fits", [
    (dict(), (375, 500), True),
    (dict(ratio=(3.0, 4.0)), (500, 100), False),
])
def test_random_resized_crop_draws_reach_both_branches(kwargs, hw, fits):
    t = transforms.RandomResizedCrop(224, **kwargs)
    img = torch.zeros((3,) + hw, dtype=torch.uint8)
    successes = 0
    for seed in SEEDS:
        torch.manual_seed(seed)
        got = t._get_params([img])
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        want, ok = R.random_resized_crop_params(*hw, **kwargs)
        successes += ok
        _same_params(got, want)
        assert torch.equal(state, torch.get_rng_state())
    assert successes == (len(SEEDS) if fits else 0)


@pytest.mark.parametrize("value", [0.5, (0.1, 0.2, 0.3), "random"])
@pytest.mark.parametrize("kwargs, hw, fits", [
    (dict(), (224, 224), True),
    (dict(scale=(0.9, 1.0), ratio=(0.1, 0.12)), (32, 32), False),
])
def test_random_erasing_draws_reach_both_branches(value, kwargs, hw, fits):
    t = transforms.RandomErasing(p=1.0, value=value, **kwargs)
    ref_value = None if value == "random" else ([float(value)] if isinstance(value, float) else [float(v) for v in value])
    img = torch.zeros((3,) + hw, dtype=torch.float32)
    successes = 0
    for seed in SEEDS:
        torch.manual_seed(seed)
        got = t._get_params([img])
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        want, ok = R.random_erasing_params(3, *hw, value=ref_value, **kwargs)
        successes += ok
        _same_params(got, want)
        assert torch.equal(state, torch.get_rng_state())
    assert successes == (len(SEEDS) if fits else 0)


def test_random_flips_draw_one_rand_and_pass_through_above_p():
    img = torch.zeros((3, 4, 4), dtype=torch.uint8)  # a host tensor: only the branch that does not transform may run
    for cls in (transforms.RandomHorizontalFlip, transforms.RandomVerticalFlip):
        passed = 0
        for seed in range(40):
            torch.manual_seed(seed)
            flips = bool(torch.rand(1) < 0.5)
            state = torch.get_rng_state()
            torch.manual_seed(seed)
            if flips:
                with pytest.raises(_lib.Mi355VisionError):  # reached the kernel: no CPU fallback
                    cls(p=0.5)(img)
            else:
                assert cls(p=0.5)(img) is img
                passed += 1
            assert torch.equal(state, torch.get_rng_state())
        assert 0 < passed < 40


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_reference_argument_errors():
    img = torch.zeros((3, 8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="Padding must be an int or a 1, 2, or 4 element tuple, not a 3 element tuple"):
        F.pad(img, [1, 2, 3])
    with pytest.raises(ValueError, match="Padding must be an int or a 1, 2, or 4 element tuple, not a 3 element tuple"):
        transforms.Pad([1, 2, 3])
    with pytest.raises(TypeError, match="padding"):
        F.pad(img, "1")
    with pytest.raises(ValueError, match="padding_mode"):
        F.pad(img, 1, padding_mode="wrap")
    with pytest.raises(ValueError, match="Padding mode should be either constant, edge, reflect or symmetric"):
        transforms.Pad(1, padding_mode="wrap")
    with pytest.raises(ValueError, match="Padding mode 'reflect' is not supported if fill is not scalar"):
        F.pad(img, 1, fill=[1, 2, 3], padding_mode="reflect")
    with pytest.raises(NotImplementedError):
        F.pad(torch.zeros((3, 8, 8), dtype=torch.int64), 1, padding_mode="reflect")
    with pytest.raises(NotImplementedError, match="per-channel fill"):
        F.pad(torch.zeros((5, 8, 8), dtype=torch.uint8), 1, fill=[1, 2, 3, 4, 5])
    with pytest.raises(ValueError, match="less than the corresponding input dimension"):
        F.pad(img, 8, padding_mode="reflect")
    with pytest.raises(ValueError, match="Required crop size \\(40, 40\\) is larger than input image size \\(8, 8\\)"):
        transforms.RandomCrop(40)(img)
    with pytest.raises(ValueError, match="Required crop size \\(40, 40\\) is larger than padded input image size \\(10, 10\\)"):
        transforms.RandomCrop(40, padding=1)(img)
    with pytest.raises(ValueError, match="Please provide only two dimensions"):
        transforms.RandomResizedCrop((1, 2, 3))
    with pytest.raises(TypeError, match="Scale should be a sequence"):
        transforms.RandomResizedCrop(8, scale=0.5)
    with pytest.raises(TypeError, match="Ratio should be a sequence"):
        transforms.RandomErasing(ratio=0.5)
    with pytest.raises(ValueError, match="Scale should be between 0 and 1"):
        transforms.RandomErasing(scale=(0.1, 1.5))
    with pytest.raises(ValueError, match="If value is str, it should be 'random'"):
        transforms.RandomErasing(value="noise")
    with pytest.raises(TypeError, match="Argument value should be either a number or str or a sequence"):
        transforms.RandomErasing(value=None)
    with pytest.raises(ValueError, match="it should have either a single value or 3"):
        transforms.RandomErasing(p=1.0, value=(1.0, 2.0))(img)
    with pytest.raises(ValueError, match="`p` should be a floating point value"):
        transforms.RandomHorizontalFlip(p=1.5)
    with pytest.raises(NotImplementedError):
        F.resized_crop(img, 0, 0, 4, 4, [8, 8], interpolation="nearest")
    for fn, args in ((F.horizontal_flip, ()), (F.vertical_flip, ()), (F.pad, (1,)), (F.crop, (0, 0, 2, 2)),
                     (F.resized_crop, (0, 0, 2, 2, [4, 4])), (F.erase, (0, 0, 1, 1, torch.zeros(1, 1, 1)))):
        with pytest.raises(NotImplementedError, match="BoundingBoxes"):
            fn(tv_tensors.BoundingBoxes(torch.zeros(1, 4)), *args)


def test_no_cpu_fallback_and_the_view_of_an_inside_crop():
    img = torch.arange(3 * 6 * 8, dtype=torch.uint8).reshape(3, 6, 8)
    view = F.crop(img, 1, 2, 3, 4)  # inside the image: the reference's view, no kernel, so it works on the host too
    assert view.data_ptr() == img[..., 1:4, 2:6].data_ptr() and torch.equal(view, img[..., 1:4, 2:6])
    for call in (lambda: F.crop(img, -1, 0, 3, 4), lambda: F.hflip(img), lambda: F.vflip(img), lambda: F.pad(img, 1),
                 lambda: F.erase(img, 0, 0, 2, 2, torch.zeros(3, 1, 1)), lambda: F.resized_crop(img, 0, 0, 4, 4, [8, 8]),
                 lambda: F.resized_crop_flip_normalize(img, 0, 0, 4, 4, [8, 8], True, [0.5] * 3, [0.5] * 3)):
        with pytest.raises(_lib.Mi355VisionError):
            call()


# ---- the ABI's own checks (before any launch) -----------------------------------------------------------------------------------------
def test_abi_rejects_bad_crop_arguments_without_a_device():
    lib = _lib.load()
    # x, y, planes, channels, elem_bytes, ih, iw, oh, ow, top, left, mode, flip_h, flip_v, fill, stream
    rc = lib.mv_pad_crop_flip(16, 32, 3, 1, 3, 8, 8, 10, 10, -1, -1, 0, 0, 0, None, None)
    assert rc == -1 and b"elem_bytes" in lib.mv_last_error()
    rc = lib.mv_pad_crop_flip(16, 32, 3, 1, 1, 8, 8, 10, 10, -1, -1, 7, 0, 0, None, None)
    assert rc == -1 and b"unknown padding mode" in lib.mv_last_error()
    rc = lib.mv_pad_crop_flip(16, 32, 3, 1, 1, 8, 8, 24, 8, -8, 0, 2, 0, 0, None, None)
    assert rc == -1 and b"reflect padding" in lib.mv_last_error() and b"smaller" in lib.mv_last_error()
    rc = lib.mv_pad_crop_flip(16, 32, 3, 1, 1, 8, 8, 8, 26, 0, -9, 3, 0, 0, None, None)
    assert rc == -1 and b"symmetric padding" in lib.mv_last_error()
    rc = lib.mv_pad_crop_flip(16, 32, 3, 5, 1, 8, 8, 10, 10, -1, -1, 0, 0, 0, None, None)
    assert rc == -1 and b"1 to 4 channels" in lib.mv_last_error()
    rc = lib.mv_pad_crop_flip(16, 32, 4, 3, 1, 8, 8, 10, 10, -1, -1, 0, 0, 0, None, None)
    assert rc == -1 and b"multiple of channels" in lib.mv_last_error()
    rc = lib.mv_pad_crop_flip(16, 16, 3, 1, 1, 8, 8, 10, 10, -1, -1, 0, 0, 0, None, None)
    assert rc == -1 and b"alias" in lib.mv_last_error()
    assert lib.mv_pad_crop_flip(None, None, 0, 1, 1, 8, 8, 10, 10, -1, -1, 0, 0, 0, None, None) == 0  # empty work
    # x, y, planes, channels, elem_bytes, h, w, i, j, eh, ew, v, per_pixel, stream
    rc = lib.mv_erase(16, 32, 3, 3, 1, 8, 8, 4, 4, 5, 2, 48, 0, None)
    assert rc == -1 and b"inside" in lib.mv_last_error()
    rc = lib.mv_erase(16, 32, 3, 3, 16, 8, 8, 0, 0, 2, 2, 48, 0, None)
    assert rc == -1 and b"elem_bytes" in lib.mv_last_error()
    rc = lib.mv_erase(16, 32, 3, 2, 1, 8, 8, 0, 0, 2, 2, 48, 0, None)
    assert rc == -1 and b"multiple of channels" in lib.mv_last_error()
    # x, y, planes, h, w, top, left, wh, ww, oh, ow, flip_h, flip_v, ws, ws_bytes, stream
    rc = lib.mv_resized_crop_u8(16, 32, 3, 8, 8, 0, 0, 0, 4, 8, 8, 0, 0, None, 0, None)
    assert rc == -1 and b"bad resize shape" in lib.mv_last_error()
    rc = lib.mv_resized_crop_f32(16, 16, 3, 8, 8, 0, 0, 4, 4, 8, 8, 0, 0, None, 0, None)
    assert rc == -1 and b"alias" in lib.mv_last_error()
    m = _lib.taps([0.5] * 3)
    z = _lib.taps([0.5, 0.0, 0.5])
    rc = lib.mv_resized_crop_preset_u8(16, 32, 1, 3, 8, 8, 0, 0, 4, 4, 8, 8, 1, 0, 1, m, z, None, 0, None)
    assert rc == -1 and b"std evaluated to zero" in lib.mv_last_error()
    rc = lib.mv_resized_crop_preset_f32(16, 32, 1, 5, 8, 8, 0, 0, 4, 4, 8, 8, 1, 0, 0, m, m, None, 0, None)
    assert rc == -1 and b"1..4 channels" in lib.mv_last_error()
