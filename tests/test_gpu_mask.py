"""The mask branch of Mask R-CNN on the GPU (`-m gpu`): F.paste_masks_in_image and F.mask_probs (csrc/mask.hip),
F.conv_transpose2d_bias_act (the pixel-shuffle instance of csrc/convnorm.hip's pointwise kernel), MaskRCNNHeads, MaskRCNNPredictor,
RoIHeads' mask branch and MaskRCNN.forward.  Everything is compared bit for bit (NaN in equal places, == elsewhere) with the
restatement and the oracle compositions of tests/_mask_ref.py on the CPU."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cpu_vision_amd as mv  # noqa: E402
from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from tests import _fpn_ref as PF  # noqa: E402
from tests import _interp_ref as IR  # noqa: E402
from tests import _mask_ref as M  # noqa: E402
from tests import _roi_heads_ref as H  # noqa: E402
from tests import _rpn_ref as P  # noqa: E402
from tests._util import philox_f32  # noqa: E402

NAN, INF = float("nan"), float("inf")


def _same_bits(got, want, what=""):
    """float32 results as bits: NaN equals itself, -0.0 differs from +0.0 (the zeros of the paste are +0.0)."""
    want = torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(IR.bits(got), IR.bits(want)):
        bad = (IR.bits(got) != IR.bits(want)).reshape(-1)
        first = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at flat index {first}: got "
                             f"{got.reshape(-1)[first].item()!r}, want {want.reshape(-1)[first].item()!r}")


# ---- F.paste_masks_in_image ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def paste_case(h, w, m, padding):
    """(masks, boxes, want) on the CPU: every roi of tests/_mask_ref.paste_boxes, the zero-plane ones included."""
    finite, zero_plane = M.paste_boxes(h, w)
    boxes = np.concatenate([finite[:5], zero_plane[:1], finite[5:], zero_plane[1:]])
    masks = M.paste_masks(9700 + m, len(boxes), m)
    return masks, torch.from_numpy(boxes), M.paste(masks.numpy(), boxes, h, w, padding)


@pytest.mark.parametrize("m,padding", [(28, 1), (14, 1), (1, 1), (28, 0), (14, 0), (1, 0)])
@pytest.mark.parametrize("h,w", M.PASTE_IMAGES)
def test_paste_equals_the_restatement(h, w, m, padding):
    masks, boxes, want = paste_case(h, w, m, padding)
    got = F.paste_masks_in_image(masks.cuda(), boxes.cuda(), (h, w), padding)
    assert _lib.last_kernel() == f"k_paste_masks<{'vec16' if w % 4 == 0 else 'scalar'}>", _lib.last_kernel()
    _same_bits(got, want, f"paste {h}x{w} m={m} padding={padding}")
    flat = want.reshape(len(want), -1)
    assert (flat != 0).any(1).sum() >= 7 and not flat[5].any() and not flat[-2:].any(), "the zero-plane rois, and only rois like them, are empty"
    if m > 1:
        assert set(np.unique(masks.numpy())) >= {0.0, 1.0}
    if w > 256 and m > 1:
        assert (flat[-3].reshape(h, w)[:, [10, 300, 590]] != 0).any(0).all(), "the wide roi spans three column blocks"


def test_paste_of_no_roi_and_of_one():
    got = F.paste_masks_in_image(torch.zeros((0, 1, 28, 28), device="cuda"), torch.zeros((0, 4), device="cuda"), (37, 53))
    assert tuple(got.shape) == (0, 1, 37, 53) and got.dtype == torch.float32 and got.is_cuda
    masks, boxes, want = paste_case(37, 53, 28, 1)
    one = F.paste_masks_in_image(masks[:1].cuda(), boxes[:1].cuda(), (37, 53))
    _same_bits(one, want[:1], "one roi")
    # views: masks and boxes that are not contiguous
    wide = torch.zeros((len(masks), 2, 28, 28)).cuda()
    wide[:, 1] = masks[:, 0].cuda()
    six = torch.zeros((len(boxes), 6)).cuda()
    six[:, 1:5] = boxes.cuda()
    _same_bits(F.paste_masks_in_image(wide[:, 1:], six[:, 1:5], (37, 53)), want, "non-contiguous views")
    with pytest.raises(RuntimeError, match="forward-only"):
        F.paste_masks_in_image(masks.cuda().requires_grad_(), boxes.cuda(), (37, 53)).sum().backward()


def test_paste_equals_the_reference_composition_on_the_device():
    """The library's own unfused composition -- F.interpolate of each zero-padded mask, a zeros image and a slice copy -- gives the
    same bits: the fused kernel is that composition, not another resize."""
    h, w, m, padding = 40, 56, 28, 1
    masks, boxes, want = paste_case(h, w, m, padding)
    ints, ok = M.expanded_boxes(boxes.numpy(), m, padding)
    dev = masks.cuda()
    for i in (0, 1, 4, 6):
        assert ok[i]
        bx0, by0, bx1, by1 = ints[i].tolist()
        bw, bh = max(bx1 - bx0 + 1, 1), max(by1 - by0 + 1, 1)
        resized = F.interpolate(torch.nn.functional.pad(dev[i:i + 1], (padding,) * 4), size=[bh, bw])[0, 0]
        image = torch.zeros((h, w), device="cuda")
        x0, x1, y0, y1 = max(bx0, 0), min(bx1 + 1, w), max(by0, 0), min(by1 + 1, h)
        image[y0:y1, x0:x1] = resized[y0 - by0:y1 - by0, x0 - bx0:x1 - bx0]
        _same_bits(image, want[i, 0], f"roi {i}")


# ---- F.mask_probs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 5])
@pytest.mark.parametrize("r", [1, 7])
def test_mask_probs_equals_the_restatement(r, c):
    g = torch.Generator().manual_seed(9710 + 10 * r + c)
    logits = torch.randn((r, c, 28, 28), generator=g) * 5
    special = torch.tensor([0.0, -0.0, 88.0, -88.0, INF, -INF, NAN, 17.0, -104.0, 89.0, -89.0])
    logits[:, :, 0, :len(special)] = special
    logits[:, :, 13, 5:5 + len(special)] = special
    labels = torch.tensor([0, c - 1, c, 1 % c, -1, c - 1, 0][:r]) if r > 1 else torch.tensor([c - 1])
    want = M.mask_probs(logits, labels)
    got = F.mask_probs(logits.cuda(), labels.cuda())
    assert _lib.last_kernel() == "k_mask_probs" and tuple(got.shape) == (r, 1, 28, 28)
    _same_bits(got, want, f"mask_probs r={r} c={c}")
    if r > 1:
        assert not want[2].any() and not want[4].any() and want[1].any(), "a label out of range gives a zero plane"
    assert bool(torch.isnan(want).any()) and bool((want == 1).any()) and bool((want == 0).any())
    # a non-contiguous mask_logits: a channel slice of a wider tensor, odd plane size
    wide = torch.randn((r, c + 3, 5, 7), generator=g) * 3
    view = wide.cuda()[:, 2:2 + c]
    assert not view.is_contiguous() or r == 1
    _same_bits(F.mask_probs(view, labels.cuda()), M.mask_probs(wide[:, 2:2 + c].contiguous(), labels), "non-contiguous logits")
    assert tuple(F.mask_probs(torch.zeros((0, c, 4, 4), device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda")).shape) == (0, 1, 4, 4)


# ---- F.conv_transpose2d_bias_act ------------------------------------------------------------------------------------------------------------
# (n, cin, h, w, cout); the last two run K in slices inside the workgroup: F.conv1x1_k_slices(1, 256, 14, 14, 4 * 16) names 2 slices of 128
# channels, F.conv1x1_k_slices(1, 512, 7, 7, 4 * 8) 4 slices of 128
CT_SHAPES = [(3, 40, 7, 7, 5), (2, 32, 14, 14, 24), (5, 256, 14, 14, 16), (1, 3, 5, 9, 1), (1, 256, 14, 14, 16), (1, 512, 7, 7, 8)]


@functools.lru_cache(maxsize=None)
def ct_case(n, cin, h, w, cout):
    x = philox_f32(9720 + cin + h, (n, cin, h, w)) * 2 - 1
    wt = (philox_f32(9721 + cin + cout, (cin, cout, 2, 2)) * 2 - 1) * np.float32(2.0 / np.sqrt(cin))
    b = philox_f32(9722 + cout, (cout,)) * 2 - 1
    want = {(bias, act): M.oracle_conv_transpose(x, wt, b if bias else None, act) for bias in (True, False) for act in ("relu", None)}
    return x, wt, b, want


def test_the_sliced_shapes_are_sliced():
    assert F.conv1x1_k_slices(1, 256, 14, 14, 64) == (2, 128) and F.conv1x1_k_slices(1, 512, 7, 7, 32) == (4, 128)
    assert F.conv1x1_k_slices(5, 256, 14, 14, 64)[0] > 1 and F.conv1x1_k_slices(3, 40, 7, 7, 20)[0] == 1


@pytest.mark.parametrize("n,cin,h,w,cout", CT_SHAPES)
def test_conv_transpose_equals_the_pixel_shuffled_oracle(n, cin, h, w, cout):
    x, wt, b, want = ct_case(n, cin, h, w, cout)
    xd, wd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(wt).cuda(), torch.from_numpy(b).cuda()
    slices = F.conv1x1_k_slices(n, cin, h, w, 4 * cout)[0]
    for (bias, act), ref in want.items():
        got = F.conv_transpose2d_bias_act(xd, wd, bd if bias else None, act)
        kernel = _lib.last_kernel()
        assert kernel.startswith("k_conv1x1_ct<") and kernel.endswith(f"ks{slices},{'vec16' if w % 2 == 0 else 'scalar'}>"), kernel
        assert tuple(got.shape) == (n, cout, 2 * h, 2 * w)
        _same_bits(got, ref, f"conv_transpose {(n, cin, h, w, cout)} bias={bias} act={act}")
    assert (want[(True, "relu")] == 0).any() and (want[(True, "relu")] > 0).any() and (want[(True, None)] < 0).any()
    # an input view offset by one element (4-byte aligned only), and the cached relayout a module passes
    flat = torch.zeros(x.size + 1, device="cuda")
    flat[1:] = xd.reshape(-1)
    view = flat[1:].view(n, cin, h, w)
    assert view.data_ptr() % 16 == 4
    relaid = F.conv_transpose2x2_relayout(wd, bd, xd.device)
    _same_bits(F.conv_transpose2d_bias_act(view, wd, bd, "relu", relaid=relaid), want[(True, "relu")], "offset input view")


def test_conv_transpose_equals_torch_within_rounding():
    n, cin, h, w, cout = 2, 32, 14, 14, 24
    x, wt, b, want = ct_case(n, cin, h, w, cout)
    ref = torch.relu(torch.nn.functional.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), stride=2))
    got = F.conv_transpose2d_bias_act(torch.from_numpy(x).cuda(), torch.from_numpy(wt).cuda(), torch.from_numpy(b).cuda(), "relu").cpu()
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


# ---- the modules --------------------------------------------------------------------------------------------------------------------------
def _randomize(module, seed, std):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * std)


def _counting(call, launches, names=("linear_bias_relu", "roi_detections", "conv_norm_act", "conv2d_bias_relu", "conv_transpose2d_bias_act",
                                     "mask_probs", "paste_masks_in_image", "interpolate", "rpn_topk", "rpn_decode")):
    """call(), recording the library calls made through the functional layer (tests/test_gpu_roi_heads.py::_counting)."""
    originals = {n: getattr(F, n) for n in names}

    def wrap(n):
        def wrapped(*a, **k):
            launches.append(n)
            return originals[n](*a, **k)
        return wrapped
    try:
        for n in originals:
            setattr(F, n, wrap(n))
        return call()
    finally:
        for n, f in originals.items():
            setattr(F, n, f)


def test_mask_heads_and_predictor_equal_their_oracle_compositions():
    heads, pred = mv.MaskRCNNHeads(24, (32, 16), 1), mv.MaskRCNNPredictor(16, 12, 5)
    _randomize(heads, 9730, 0.08), _randomize(pred, 9731, 0.15)
    x = philox_f32(9732, (7, 24, 14, 14)) * 2 - 1
    want_hidden = M.oracle_heads(heads, x)
    want_up, want_logits = M.oracle_predictor(pred, want_hidden)
    heads, pred = heads.cuda(), pred.cuda()
    launches = []
    hidden = _counting(lambda: heads(torch.from_numpy(x).cuda()), launches)
    logits = _counting(lambda: pred(hidden), launches)
    assert launches == ["conv2d_bias_relu"] * 2 + ["conv_transpose2d_bias_act", "conv_norm_act"]
    _same_bits(hidden, want_hidden, "MaskRCNNHeads")
    _same_bits(logits, want_logits, "MaskRCNNPredictor")
    assert tuple(logits.shape) == (7, 5, 28, 28) and (want_hidden > 0).mean() > 0.1 and (want_up > 0).mean() > 0.1
    # the relayout follows the parameters
    with torch.no_grad():
        pred.conv5_mask.weight.mul_(0.5)
    _, want_half = M.oracle_predictor(pred.cpu(), want_hidden)
    _same_bits(pred.cuda()(hidden), want_half, "after a weight update")


# ---- RoIHeads' mask branch and MaskRCNN.forward, stage by stage -----------------------------------------------------------------------------
MODEL_KW = dict(num_classes=5, rpn_pre_nms_top_n_test=200, rpn_post_nms_top_n_test=50, box_score_thresh=0.05, box_detections_per_img=20,
                _skip_resize=True)
MASK_LAYERS = (64, 64, 64, 256)


def whole_setup():
    """(library model, replica model in the restatement's numerics, images), on the CPU with equal parameters: the backbone, rpn and
    box branch of tests/test_gpu_roi_heads.py::whole_setup (seed 0: every image returns detections), and a mask branch whose head
    is narrower in the middle (64 channels: the CPU oracle of four 256 -> 256 convs on 40 rois takes 5 s) in front of the default
    256 -> 256 predictor."""
    torch.manual_seed(8900)
    replica = M.MaskRCNN(PF.resnet_fpn_backbone(backbone_name="resnet18"), numerics=H.RESTATEMENT, mask_head=M.MaskRCNNHeads(256, MASK_LAYERS, 1),
                         **MODEL_KW).eval()
    PF.randomize(replica.backbone, 8901)
    _randomize(replica.rpn.head, 8902, 0.03)
    _randomize(replica.roi_heads.box_head, 8903, 0.02)
    _randomize(replica.roi_heads.box_predictor, 8904, 0.04)
    _randomize(replica.roi_heads.mask_head, 9740, 0.03)
    _randomize(replica.roi_heads.mask_predictor, 9741, 0.05)
    model = mv.MaskRCNN(mv.resnet_fpn_backbone(backbone_name="resnet18"), mask_head=mv.MaskRCNNHeads(256, MASK_LAYERS, 1), **MODEL_KW)
    model.load_state_dict(replica.state_dict(), strict=True)
    images = [torch.from_numpy(philox_f32(8905, (3, 128, 160))), torch.from_numpy(philox_f32(8906, (3, 120, 150)))]
    return model, replica, images


@torch.no_grad()
def test_mask_rcnn_stage_by_stage():
    """Each stage's reference takes the library's own output of the stage before, so that a last-bit difference upstream cannot
    cascade: detections -> pooled mask features -> mask head -> predictor -> probabilities -> pasted masks."""
    model, replica, images = whole_setup()
    model = model.cuda()
    dev_images = [im.cuda() for im in images]
    sizes = [(128, 160), (120, 150)]
    il, _ = model.transform(dev_images)
    feats = model.backbone(il.tensors)
    proposals, _ = model.rpn(il, feats)
    heads = model.roi_heads
    # RoIHeads.forward: the box branch, then the mask branch, in that order and nothing else
    launches = []
    result, losses = _counting(lambda: heads(feats, proposals, il.image_sizes), launches)
    assert losses == {}
    assert launches == ["linear_bias_relu"] * 3 + ["roi_detections"] + ["conv2d_bias_relu"] * 4 + ["conv_transpose2d_bias_act", "conv_norm_act",
                                                                                                    "mask_probs"], launches
    boxes, labels = [r["boxes"] for r in result], [r["labels"] for r in result]
    counts = [len(b) for b in boxes]
    for i in range(2):
        assert list(result[i]) == ["boxes", "labels", "scores", "masks"]
        assert 0 < counts[i] <= 20, "every image returns detections"
        assert tuple(result[i]["masks"].shape) == (counts[i], 1, 28, 28)
    # pooled mask features
    cpu_feats, cpu_boxes = {k: v.cpu() for k, v in feats.items()}, [b.cpu() for b in boxes]
    pooled = heads.mask_roi_pool(feats, boxes, il.image_sizes)
    assert tuple(pooled.shape) == (sum(counts), 256, 14, 14)
    P.same(pooled, replica.roi_heads.mask_roi_pool(cpu_feats, cpu_boxes, il.image_sizes), "pooled mask features")
    # mask head, predictor
    hidden = heads.mask_head(pooled)
    _same_bits(hidden, M.oracle_heads(replica.roi_heads.mask_head, pooled.cpu().numpy()), "mask head")
    logits = heads.mask_predictor(hidden)
    _same_bits(logits, M.oracle_predictor(replica.roi_heads.mask_predictor, hidden.cpu().numpy())[1], "mask predictor")
    assert tuple(logits.shape) == (sum(counts), 5, 28, 28)
    # probabilities: the restatement on the library's logits and labels
    probs = F.mask_probs(logits, torch.cat(labels))
    want_probs = M.mask_probs(logits.cpu(), torch.cat(labels).cpu())
    _same_bits(probs, want_probs, "mask probabilities")
    for got, want in zip(result, want_probs.split(counts)):
        _same_bits(got["masks"], want, "result masks")
    assert 0.0 < float(want_probs.min()) and float(want_probs.max()) < 1.0 and float(want_probs.std()) > 1e-3
    # pasted masks: transform.postprocess, ONE paste launch per image; first at the images' own sizes, then rescaled
    for originals in (sizes, [(256, 200), (77, 150)]):
        launches = []
        copies = [{k: v.clone() for k, v in r.items()} for r in result]
        out = _counting(lambda: model.transform.postprocess(copies, il.image_sizes, originals), launches)
        assert launches == ["paste_masks_in_image"] * 2
        want_boxes = replica.transform.postprocess([{"boxes": b.clone()} for b in cpu_boxes], il.image_sizes, originals)
        for i, (got, (oh, ow)) in enumerate(zip(out, originals)):
            assert list(got) == ["boxes", "labels", "scores", "masks"]
            P.same(got["boxes"], want_boxes[i]["boxes"], f"rescaled boxes of image {i}")
            want = M.paste(result[i]["masks"].cpu().numpy(), got["boxes"].cpu().numpy(), oh, ow)
            assert tuple(got["masks"].shape) == (counts[i], 1, oh, ow)
            _same_bits(got["masks"], want, f"pasted masks of image {i} at {oh}x{ow}")
            assert (want.reshape(counts[i], -1) != 0).any(1).all() and (want == 0).any(), "every pasted mask holds values other than 0"
    # the whole model: the same detections and masks
    whole = model(dev_images)
    for i, got in enumerate(whole):
        assert list(got) == ["boxes", "labels", "scores", "masks"] and got["masks"].is_cuda and got["masks"].dtype == torch.float32
        P.same(got["labels"], result[i]["labels"]), P.same(got["scores"], result[i]["scores"])
        want = M.paste(result[i]["masks"].cpu().numpy(), got["boxes"].cpu().numpy(), *sizes[i])
        _same_bits(got["masks"], want, f"MaskRCNN.forward masks of image {i}")


@torch.no_grad()
def test_mask_branch_without_detections_launches_nothing():
    model, _, images = whole_setup()
    model = model.cuda()
    model.roi_heads.score_thresh = 2.0  # no score passes
    launches = []
    out = _counting(lambda: model([im.cuda() for im in images]), launches)
    assert "roi_detections" in launches and "mask_probs" not in launches and "conv_transpose2d_bias_act" not in launches
    for got, (h, w) in zip(out, [(128, 160), (120, 150)]):
        assert list(got) == ["boxes", "labels", "scores", "masks"]
        assert tuple(got["boxes"].shape) == (0, 4) and tuple(got["masks"].shape) == (0, 1, h, w) and got["masks"].dtype == torch.float32
