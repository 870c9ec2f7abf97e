"""F.interpolate, F.detection_batch and the detection transform's resize on the device (`-m gpu`), bit for bit against the oracle of
tests/_interp_ref.py (the formula of include/mi355vision.h in numpy float32): the edge shapes of the interpolation, the fused front
end against the reference composition normalize -> interpolate -> zero-padded batch and against the library's own three launches,
GeneralizedRCNNTransform.forward / postprocess with real ratios, and FasterRCNN / RetinaNet end to end on raw images of two sizes.

NaNs are compared by position (a NaN's sign and payload are the processor's: the default NaN of 0 * inf differs between the host's
and the device's); everything else, -0.0 included, as bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd import transform as T  # noqa: E402
from tests import _fpn_ref as PF  # noqa: E402
from tests import _interp_ref as R  # noqa: E402
from tests import _roi_heads_ref as H  # noqa: E402
from tests._util import philox_f32  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
QNAN = 0x7FC00000


def same_bits(got, want, what=""):
    got = got.detach().cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    want = want.detach().cpu() if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g = torch.where(torch.isnan(got), torch.full_like(R.bits(got), QNAN), R.bits(got))
    w = torch.where(torch.isnan(want), torch.full_like(R.bits(want), QNAN), R.bits(want))
    if not torch.equal(g, w):
        bad = (g != w).reshape(-1)
        first = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at flat index {first}: got "
                             f"{got.reshape(-1)[first].item()!r}, want {want.reshape(-1)[first].item()!r}")


def signed(seed, shape):
    return philox_f32(seed, shape) * 4 - 2


# ---- F.interpolate ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 3, 5), (1, 1, 1, 1), (5, 7, 9, 13), (23, 31, 7, 5), (6, 6, 6, 6), (9, 11, 4, 1), (9, 11, 5, 2), (9, 11, 6, 3), (12, 300, 30, 777),
          (7, 5, 13, 8)]


@pytest.mark.parametrize("h,w,oh,ow", SHAPES, ids=[f"{h}x{w}-{oh}x{ow}" for h, w, oh, ow in SHAPES])
def test_interpolate_equals_the_oracle(h, w, oh, ow):
    x = signed(9000 + h * w + oh, (2, 3, h, w))
    got = F.interpolate(torch.from_numpy(x).cuda(), size=[oh, ow])
    assert _lib.last_kernel() == f"k_interp_batch<plain,{'vec16' if ow % 4 == 0 else 'scalar'}>", _lib.last_kernel()
    same_bits(got, R.interpolate(x, oh, ow), f"{h}x{w} -> {oh}x{ow}")
    if (h, w) == (oh, ow):
        same_bits(got, x, "the same size is the input")


def test_interpolate_wide_row_needs_the_fma_in_src():
    x = signed(9020, (1, 1, 1, 2049))
    got = F.interpolate(torch.from_numpy(x).cuda(), size=[1, 4099])
    same_bits(got, R.interpolate(x, 1, 4099), "2049 -> 4099")
    # what the test is for: without the fma, src = s * (d + 0.5) - 0.5 with two roundings, some weights differ
    s = np.float32(2049) / np.float32(4099)
    d = np.arange(4099, dtype=np.float32)
    plain = np.maximum(s * (d + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    fused = np.maximum(R.fma32(np.full(4099, s, np.float32), d + np.float32(0.5), np.float32(-0.5)), np.float32(0))
    assert (plain != fused).any()


def test_interpolate_scale_factor_with_recompute():
    x = signed(9021, (1, 2, 40, 56))
    scale = min(64 / 40, 96 / 56)
    got = F.interpolate(torch.from_numpy(x).cuda(), scale_factor=scale, recompute_scale_factor=True)
    assert tuple(got.shape) == (1, 2, 64, 89)
    same_bits(got, R.interpolate(x, 64, 89))


def test_interpolate_input_view_offset_by_one_element():
    flat = torch.from_numpy(signed(9022, (1 + 3 * 13 * 17,))).cuda()
    view = flat[1:].view(1, 3, 13, 17)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    for oh, ow in ((20, 32), (7, 9)):
        same_bits(F.interpolate(view, size=[oh, ow]), R.interpolate(view.cpu().numpy(), oh, ow), f"offset view -> {oh}x{ow}")


@pytest.mark.parametrize("planes", [1, 3, 4, 5])
def test_interpolate_plane_counts(planes):
    x = signed(9030 + planes, (planes, 1, 10, 14))
    same_bits(F.interpolate(torch.from_numpy(x).cuda(), size=[17, 24]), R.interpolate(x, 17, 24))
    x = x.reshape(1, planes, 10, 14)
    same_bits(F.interpolate(torch.from_numpy(x).cuda(), size=[5, 1028]), R.interpolate(x, 5, 1028))  # 16-byte stores, five column blocks, one lane in the last


def test_interpolate_nan_and_inf_follow_the_formula():
    x = signed(9040, (1, 2, 6, 9))
    x[0, 0, 2, 3] = np.nan
    x[0, 1, 4, 8] = np.inf
    x[0, 1, 0, 0] = -0.0
    for oh, ow in ((11, 17), (6, 9), (3, 4)):
        want = R.interpolate(x, oh, ow)
        got = F.interpolate(torch.from_numpy(x).cuda(), size=[oh, ow])
        same_bits(got, want, f"NaN / inf -> {oh}x{ow}")
        # at the same size every weight next to the inf is 0: all of its outputs are 0 * inf = NaN
        assert np.isnan(want).any() and np.isinf(want).any() == ((oh, ow) != (6, 9))
    assert np.isnan(R.interpolate(x, 6, 9)[0, 1, 4, 7])  # the tap to the left of the inf: 1 * a + 0 * inf


def test_interpolate_empty_and_forward_only():
    x = torch.zeros((0, 3, 5, 5), device="cuda")
    assert tuple(F.interpolate(x, size=[7, 7]).shape) == (0, 3, 7, 7)
    y = F.interpolate(torch.ones((1, 1, 4, 4), device="cuda", requires_grad=True), size=[8, 8])
    with pytest.raises(RuntimeError, match="forward-only"):
        y.sum().backward()


# ---- F.detection_batch --------------------------------------------------------------------------------------------------------------------
SIZES3 = [(40, 56), (50, 37), (33, 33)]  # at 64 / 96: (64, 89), (86, 64), (64, 64) -- the second sets Hp, the first Wp


def _images(seed, c, sizes):
    return [torch.from_numpy(philox_f32(seed + i, (c, h, w))) for i, (h, w) in enumerate(sizes)]


def _composition(images, sizes, mean, std, div):
    """The library's own three steps on the device: F.normalize -> F.interpolate -> batch_images."""
    t = mv.GeneralizedRCNNTransform(64, 96, mean, std, size_divisible=div, _skip_resize=True)
    resized = [F.interpolate(F.normalize(im, mean, std)[None], size=list(s))[0] for im, s in zip(images, sizes)]
    return t.batch_images(resized, div)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("div", [32, 1, 3])
def test_detection_batch_equals_the_reference_composition(c, div):
    images = _images(9100 + 10 * c, c, SIZES3)
    sizes = [R.resized_size(h, w, 64, 96) for h, w in SIZES3]
    assert sizes == [(64, 89), (86, 64), (64, 64)]
    mean, std = MEAN[:c], STD[:c]
    want = R.detection_batch(images, sizes, mean, std, div)
    dev = [im.cuda() for im in images]
    got = F.detection_batch(dev, sizes, mean, std, div)
    hp, wp = R.padded_side(86, div), R.padded_side(89, div)
    assert tuple(got.shape) == (3, c, hp, wp) == tuple(want.shape)
    assert _lib.last_kernel() == f"k_interp_batch<norm,{'vec16' if wp % 4 == 0 else 'scalar'}>", _lib.last_kernel()
    same_bits(got, want, f"c={c} div={div}")
    # the padding is +0.0, as bits
    pad = R.bits(got)
    for i, (oh, ow) in enumerate(sizes):
        assert not pad[i, :, oh:, :].any() and not pad[i, :, :, ow:].any()
    # and the library's own composition gives the same bits
    same_bits(_composition(dev, sizes, mean, std, div), got, "normalize -> interpolate -> batch_images")


def test_detection_batch_without_a_resize_is_normalize_and_pad():
    sizes = [(33, 47), (40, 21)]
    images = _images(9150, 3, sizes)
    want = R.detection_batch(images, sizes, MEAN[:3], STD[:3], 32)
    got = F.detection_batch([im.cuda() for im in images], sizes, MEAN[:3], STD[:3], 32)
    assert tuple(got.shape) == (2, 3, 64, 64)
    same_bits(got, want)
    for i, (im, (h, w)) in enumerate(zip(images, sizes)):  # src == d exactly: the values are the normalised pixels
        same_bits(got[i, :, :h, :w], R.normalize(im, MEAN[:3], STD[:3]), f"image {i}")


def test_detection_batch_downscale_and_upscale_in_one_batch():
    """A lane of a downscaled image reads more than five source columns (the general path), one of an upscaled image at most five."""
    shapes = [(120, 200), (20, 31), (150, 90)]
    sizes = [R.resized_size(h, w, 64, 96) for h, w in shapes]
    assert sizes == [(57, 96), (61, 96), (96, 57)]
    images = _images(9155, 3, shapes)
    want = R.detection_batch(images, sizes, MEAN[:3], STD[:3], 32)
    same_bits(F.detection_batch([im.cuda() for im in images], sizes, MEAN[:3], STD[:3], 32), want)


def test_detection_batch_more_images_than_one_launch_holds():
    sizes = [(5 + i % 3, 4 + i % 5) for i in range(70)]
    images = _images(9160, 2, sizes)
    out = [(7 + i % 4, 9 - i % 2) for i in range(70)]
    want = R.detection_batch(images, out, MEAN[:2], STD[:2], 4)
    same_bits(F.detection_batch([im.cuda() for im in images], out, MEAN[:2], STD[:2], 4), want)


def test_detection_batch_non_contiguous_image():
    base = torch.from_numpy(philox_f32(9170, (3, 30, 64))).cuda()
    view = base[:, :, 5:42]
    assert not view.is_contiguous()
    want = R.detection_batch([view.cpu().contiguous()], [(50, 61)], MEAN[:3], STD[:3], 32)
    same_bits(F.detection_batch([view], [(50, 61)], MEAN[:3], STD[:3], 32), want)


# ---- GeneralizedRCNNTransform -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [None, (72, 40)], ids=["min-max", "fixed_size"])
def test_transform_forward_and_postprocess(fixed):
    t = mv.GeneralizedRCNNTransform(64, 96, MEAN[:3], STD[:3], fixed_size=fixed)
    images = _images(9200, 3, SIZES3)
    sizes = [R.resized_size(h, w, 64, 96, fixed) for h, w in SIZES3]
    il, targets = t([im.cuda() for im in images])
    assert targets is None and isinstance(il, mv.ImageList)
    assert [tuple(s) for s in il.image_sizes] == sizes == [T.resized_size(h, w, 64, 96, fixed) for h, w in SIZES3]
    assert sizes == ([(40, 72)] * 3 if fixed else [(64, 89), (86, 64), (64, 64)])
    same_bits(il.tensors, R.detection_batch(images, sizes, MEAN[:3], STD[:3], 32), "ImageList.tensors")
    assert il.tensors.shape[-2] % 32 == 0 and il.tensors.shape[-1] % 32 == 0
    # resize on its own is the same interpolation
    one = t.resize(F.normalize(images[0].cuda(), MEAN[:3], STD[:3]))
    same_bits(one, il.tensors[0, :, :sizes[0][0], :sizes[0][1]], "resize")
    # postprocess with real ratios
    g = torch.Generator().manual_seed(9201)
    boxes = [torch.rand((5, 4), generator=g) * 60, torch.rand((0, 4), generator=g), torch.rand((3, 4), generator=g) * 60]
    got = t.postprocess([{"boxes": b.cuda()} for b in boxes], il.image_sizes, SIZES3)
    for b, r, s, o in zip(boxes, got, sizes, SIZES3):
        assert s != o
        same_bits(r["boxes"], H.resize_boxes(b, s, o), "postprocess")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
RAW = [(40, 56), (50, 37)]


def _randomize(module, seed, std):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * std)


def _end_to_end(build, prepare):
    """build(**transform keywords) -> the model.  One model on the raw images; the same parameters in a model built with
    _skip_resize=True and the identity normalisation on the oracle's normalised and resized images, its boxes rescaled with the
    replica's resize_boxes: an exact match."""
    for h, w in RAW:
        assert R.resized_size(h, w, 64, 96) == R.scripted_resized_size(h, w, 64, 96)  # the two size rules agree on these
    sizes = [R.resized_size(h, w, 64, 96) for h, w in RAW]
    assert all(s != o for s, o in zip(sizes, RAW))
    model = build()
    prepare(model)
    plain = build(_skip_resize=True, image_mean=[0.0, 0.0, 0.0], image_std=[1.0, 1.0, 1.0])
    plain.load_state_dict(model.state_dict(), strict=True)
    images = _images(9300, 3, RAW)
    mean, std = model.transform.image_mean, model.transform.image_std
    resized = [torch.from_numpy(R.interpolate(R.normalize(im, mean, std).numpy(), oh, ow)) for im, (oh, ow) in zip(images, sizes)]
    with torch.no_grad():
        got = model.cuda()([im.cuda() for im in images])
        want = plain.cuda()([im.cuda() for im in resized])
    assert sum(len(d["boxes"]) for d in got) > 0, "no detection: the comparison would be empty"
    for d, wd, s, o in zip(got, want, sizes, RAW):
        same_bits(d["boxes"], H.resize_boxes(wd["boxes"].cpu(), s, o), "boxes")
        same_bits(d["scores"], wd["scores"], "scores")
        assert torch.equal(d["labels"].cpu(), wd["labels"].cpu())


def test_faster_rcnn_on_raw_images():
    def build(**kw):
        torch.manual_seed(9310)
        return mv.FasterRCNN(mv.resnet_fpn_backbone(backbone_name="resnet18"), num_classes=5, min_size=64, max_size=96, rpn_pre_nms_top_n_test=200,
                             rpn_post_nms_top_n_test=50, box_detections_per_img=20, **kw)

    def prepare(model):
        replica_bb = PF.resnet_fpn_backbone(backbone_name="resnet18").eval()
        PF.randomize(replica_bb, 9311)
        model.backbone.load_state_dict(replica_bb.state_dict(), strict=True)
        _randomize(model.rpn.head, 9312, 0.03)
        _randomize(model.roi_heads.box_head, 9313, 0.02)
        _randomize(model.roi_heads.box_predictor, 9314, 0.04)
    _end_to_end(build, prepare)


def test_retinanet_on_raw_images():
    def build(**kw):
        torch.manual_seed(9320)
        backbone = mv.resnet_fpn_backbone(backbone_name="resnet18", returned_layers=[2, 3, 4], extra_blocks=mv.LastLevelP6P7(256, 256))
        return mv.RetinaNet(backbone, 5, min_size=64, max_size=96, topk_candidates=100, **kw)

    def prepare(model):
        replica_bb = PF.resnet_fpn_backbone(backbone_name="resnet18", returned_layers=[2, 3, 4], extra_blocks=PF.LastLevelP6P7(256, 256)).eval()
        PF.randomize(replica_bb, 9321)
        model.backbone.load_state_dict(replica_bb.state_dict(), strict=True)
        _randomize(model.head, 9322, 0.02)
        with torch.no_grad():
            model.head.classification_head.cls_logits.bias.fill_(-2.2)
    _end_to_end(build, prepare)
