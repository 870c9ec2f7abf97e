"""F.elastic / ElasticTransform host logic (no GPU): the C ABI's argument checks, the registered kernels, the reference's
argument errors, and the transform's fill / interpolation arguments.  Every check here runs before any device use."""
import ctypes

import pytest
import torch

from cpu_vision_amd import _lib, _pil, functional as F, transforms, tv_tensors
from cpu_vision_amd._registry import _get_kernel


H, W = 5, 7
FAKE_X, FAKE_Y, FAKE_BX, FAKE_BY, FAKE_D = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


def _call(name, **over):
    """One mv_elastic_* call whose arguments are valid except for `over`: it must be rejected before any launch (the
    pointers are fake)."""
    args = dict(x=FAKE_X, y=FAKE_Y, planes=6, channels=3, h=H, w=W, bx=FAKE_BX, by=FAKE_BY, d=FAKE_D, sh=2 * W, sw=2, sc=1,
                mode=0, fill=None)
    args.update(over)
    lib = _lib.load()
    rc = getattr(lib, name)(args["x"], args["y"], args["planes"], args["channels"], args["h"], args["w"], args["bx"], args["by"],
                            args["d"], args["sh"], args["sw"], args["sc"], args["mode"], args["fill"], None)
    return rc, lib.mv_last_error().decode()


@pytest.mark.parametrize("name", ["mv_elastic_f32", "mv_elastic_u8"])
@pytest.mark.parametrize("over,rc_want,msg", [
    (dict(h=0), -1, "bad shape"),
    (dict(w=-3), -1, "bad shape"),
    (dict(planes=0), -1, "bad shape"),
    (dict(planes=-2), -1, "bad shape"),
    (dict(planes=7), -1, "multiple of channels"),
    (dict(channels=0), -1, "multiple of channels"),
    (dict(mode=2), -1, "unknown mode"),
    (dict(mode=-1), -1, "unknown mode"),
    (dict(x=None), -1, "null pointer"),
    (dict(y=None), -1, "null pointer"),
    (dict(bx=None), -1, "null pointer"),
    (dict(by=None), -1, "null pointer"),
    (dict(d=None), -1, "null pointer"),
    (dict(y=FAKE_X), -1, "alias"),
    (dict(h=65536, w=65536, sh=2 * 65536), -2, "exceed 2^31"),
    (dict(planes=17, channels=17, fill=_lib.taps([0.0] * 17)), -2, "up to 16 channels"),
])
def test_abi_rejects_bad_arguments_before_any_launch(name, over, rc_want, msg):
    rc, err = _call(name, **over)
    assert rc == rc_want and msg in err, (rc, err)


def test_abi_binding_declares_the_elastic_entry_points():
    for name in ("mv_elastic_f32", "mv_elastic_u8"):
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == 15
    assert _lib.load().mv_abi_version() == 1


def test_elastic_kernels_are_registered_for_every_input_type():
    for t in (torch.Tensor, tv_tensors.Image, tv_tensors.Video, tv_tensors.Mask):
        assert _get_kernel(F.elastic, t) is not None
    if _pil.PIL is not None:
        assert _get_kernel(F.elastic, _pil.PIL.Image.Image) is F._elastic_image_pil
    assert F.elastic_transform is F.elastic
    boxes = tv_tensors.BoundingBoxes(torch.zeros(2, 4))
    with pytest.raises(NotImplementedError, match="BoundingBoxes"):
        F.elastic(boxes, torch.zeros(1, H, W, 2))


def test_reference_argument_errors_come_before_device_use():
    img = torch.zeros(3, H, W)
    with pytest.raises(TypeError, match="displacement should be a Tensor"):
        F.elastic(img, [[0.0, 0.0]])
    with pytest.raises(ValueError, match=r"displacement shape should be \(1, 5, 7, 2\)"):
        F.elastic(img, torch.zeros(1, W, H, 2))
    with pytest.raises(ValueError, match="displacement shape"):
        F.elastic(img, torch.zeros(H, W, 2))
    with pytest.raises(RuntimeError, match="must match"):
        F.elastic(img, torch.zeros(1, H, W, 2), fill=[1.0, 2.0])
    with pytest.raises(RuntimeError, match="must match"):
        F.elastic(img, torch.zeros(1, H, W, 2), fill=[1.0, 2.0, 3.0, 4.0])
    with pytest.raises(NotImplementedError, match="bicubic"):
        F.elastic(img, torch.zeros(1, H, W, 2), interpolation=transforms.InterpolationMode.BICUBIC)
    with pytest.raises(NotImplementedError, match="bicubic"):
        F.elastic(img, torch.zeros(1, H, W, 2), interpolation=3)  # Pillow's BICUBIC constant
    with pytest.raises(ValueError, match="InterpolationMode"):
        F.elastic(img, torch.zeros(1, H, W, 2), interpolation=1.5)
    with pytest.raises(NotImplementedError, match="float64"):
        F.elastic(img.double(), torch.zeros(1, H, W, 2))
    with pytest.raises(NotImplementedError, match="float16"):
        F.elastic(tv_tensors.Video(torch.zeros(2, 3, H, W, dtype=torch.float16)), torch.zeros(1, H, W, 2))


@pytest.mark.parametrize("fill", [None, 0, 127, [10, 20, 30], (1.5,)])
@pytest.mark.parametrize("interpolation", ["bilinear", "nearest", transforms.InterpolationMode.NEAREST, 2])
def test_cpu_tensors_raise_like_every_other_kernel(fill, interpolation):
    """Valid arguments on host tensors: the library's no-CPU-fallback error, not a silent torch computation."""
    for img in (torch.zeros(3, H, W), torch.zeros(2, 3, H, W, dtype=torch.uint8)):
        with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
            F.elastic(img, torch.zeros(1, H, W, 2), interpolation=interpolation, fill=fill)


def test_empty_image_returns_without_a_device():
    img = torch.zeros(0, 3, H, W)
    assert F.elastic(img, torch.zeros(1, H, W, 2)).shape == img.shape


def test_elastic_transform_fill_and_interpolation_arguments():
    tr = transforms.ElasticTransform()
    assert tr.interpolation is transforms.InterpolationMode.BILINEAR and tr.fill == 0
    assert transforms._get_fill(tr._fill, tv_tensors.Image) == 0 and transforms._get_fill(tr._fill, tv_tensors.Mask) == 0
    assert transforms.ElasticTransform(interpolation="nearest").interpolation is transforms.InterpolationMode.NEAREST
    assert transforms.ElasticTransform(interpolation=0).interpolation is transforms.InterpolationMode.NEAREST
    assert transforms.ElasticTransform(interpolation=2).interpolation is transforms.InterpolationMode.BILINEAR
    with pytest.raises(ValueError, match="InterpolationMode"):
        transforms.ElasticTransform(interpolation="cubic-ish")
    with pytest.raises(ValueError, match="not supported"):
        transforms.ElasticTransform(interpolation=9)
    with pytest.raises(TypeError, match="inappropriate fill arg"):
        transforms.ElasticTransform(fill="white")
    with pytest.raises(TypeError, match="inappropriate fill arg"):
        transforms.ElasticTransform(fill={tv_tensors.Image: object()})
    tr = transforms.ElasticTransform(fill=(1, 2, 3))
    assert transforms._get_fill(tr._fill, tv_tensors.Video) == [1.0, 2.0, 3.0]
    tr = transforms.ElasticTransform(fill={tv_tensors.Image: 7, "others": None})
    assert transforms._get_fill(tr._fill, tv_tensors.Image) == 7
    assert transforms._get_fill(tr._fill, tv_tensors.Mask) is None
    assert transforms._get_fill(transforms.ElasticTransform(fill=None)._fill, torch.Tensor) is None


def test_transform_without_displacement_names_the_resampler():
    with pytest.raises(NotImplementedError, match="grid_sample"):
        transforms.ElasticTransform()._transform(torch.zeros(3, H, W), {})


def test_transform_routes_to_f_elastic():
    """With a displacement in the params, _transform calls F.elastic with the transform's fill and interpolation (here the
    host tensor reaches the library and raises its no-CPU error)."""
    tr = transforms.ElasticTransform(fill=[1, 2, 3], interpolation="nearest")
    with pytest.raises(_lib.Mi355VisionError):
        tr._transform(torch.zeros(3, H, W), {"displacement": torch.zeros(1, H, W, 2)})
    with pytest.raises(RuntimeError, match="must match"):  # the fill reached F.elastic: 3 values for 1 channel
        tr._transform(tv_tensors.Mask(torch.zeros(1, H, W, dtype=torch.uint8)), {"displacement": torch.zeros(1, H, W, 2)})
