"""MixUp / CutMix and the random containers on the GPU against the reference restated on the CPU (tests/_mix_ref.py).
The arithmetic is fully specified (two rounded products, one rounded sum; CutMix moves bytes), so every comparison is
torch.equal: there are no tolerances."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, functional as F, transforms, tv_tensors  # noqa: E402
from tests import _mix_ref as R  # noqa: E402

FLOATS = [torch.float32, torch.float16, torch.float64]
MOVED = [torch.uint8, torch.float32, torch.float16, torch.int64, torch.bool]
# (B, 3, H, W): B in {1, 2, 7, 256}, widths off the 16-byte vector (1, 17, 1921) and on it (224)
SHAPES = [(1, 3, 5, 17), (2, 3, 4, 1), (7, 3, 9, 17), (7, 3, 2, 1921), (2, 3, 224, 224), (256, 3, 6, 17), (7, 1, 1, 1)]
DRAWN_LAM = 0.6180339887498949


def _batch(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.bool:
        return torch.rand(shape, generator=g) > 0.5
    if dtype.is_floating_point:
        return (torch.rand(shape, generator=g, dtype=torch.float32) * 4 - 2).to(dtype)
    return torch.randint(0, 256 if dtype == torch.uint8 else 1 << 40, shape, generator=g).to(dtype)


def _equal(got, want, what=""):
    assert got.is_cuda
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert torch.equal(got, want), what


# ---- MixUp ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", FLOATS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mixup_image_bit_for_bit(shape, dtype):
    x = _batch(shape, dtype, seed=sum(shape))
    for lam in (0.0, 1.0, DRAWN_LAM, 0.0123):
        _equal(F.mixup_image(x.cuda(), lam), R.mixup_image(x, lam), (shape, lam))


def test_mixup_image_takes_both_kernels():
    x = _batch((7, 3, 9, 17), torch.float32, seed=1).cuda()
    F.mixup_image(x, 0.3)
    assert _lib.last_kernel().startswith("k_mixup_roll<f32"), _lib.last_kernel()
    F.mixup_image(x[:, :1, :1, :10], 0.3)  # rows of three 16-byte groups
    assert _lib.last_kernel() == "k_mixup_flat<f32>", _lib.last_kernel()


def test_mixup_batch_of_one_mixes_the_sample_with_itself():
    x = _batch((1, 3, 33, 65), torch.float32, seed=3)
    got = F.mixup_image(x.cuda(), DRAWN_LAM)
    _equal(got, R.mixup_image(x, DRAWN_LAM))
    _equal(got, x * torch.tensor(1.0 - DRAWN_LAM).float() + x * torch.tensor(DRAWN_LAM).float())


def test_mixup_video_noncontiguous_and_empty():
    v = _batch((3, 2, 3, 10, 13), torch.float32, seed=4)  # (B, T, C, H, W)
    _equal(F.mixup_image(v.cuda(), DRAWN_LAM), R.mixup_image(v, DRAWN_LAM), "5-D")
    big = _batch((7, 3, 12, 40), torch.float16, seed=5)
    for view in (lambda t: t[:, :, 1:, 3:], lambda t: t[::2], lambda t: t.permute(0, 1, 3, 2), lambda t: t[1:]):
        _equal(F.mixup_image(view(big.cuda()), DRAWN_LAM), R.mixup_image(view(big), DRAWN_LAM), "view")
    assert F.mixup_image(torch.zeros((0, 3, 4, 4), device="cuda"), 0.5).shape == (0, 3, 4, 4)
    assert F.mixup_image(torch.zeros((4, 3, 0, 4), device="cuda"), 0.5).shape == (4, 3, 0, 4)


def test_mixup_special_values():
    x = _batch((5, 3, 8, 20), torch.float32, seed=6)
    x.view(-1)[::7] = float("inf")
    x.view(-1)[3::11] = 1e-42  # subnormal
    x.view(-1)[5::13] = -0.0
    got, want = F.mixup_image(x.cuda(), DRAWN_LAM).cpu(), R.mixup_image(x, DRAWN_LAM)
    assert torch.equal(got.isnan(), want.isnan())
    assert torch.equal(got.nan_to_num(nan=7.0).view(torch.int32), want.nan_to_num(nan=7.0).view(torch.int32))


def test_mixup_rejects_integer_images():
    x = _batch((4, 3, 8, 8), torch.uint8, seed=7).cuda()
    with pytest.raises(TypeError, match="convert first"):
        F.mixup_image(x, 0.5)
    with pytest.raises(TypeError, match="convert first"):
        transforms.MixUp(num_classes=3)(x, torch.arange(4).cuda() % 3)


# ---- CutMix -----------------------------------------------------------------------------------------------------------------------------
def _boxes(h, w):
    """Interior, clipped at each edge, empty (zero width, zero height) and the whole image."""
    cx, cy = w // 2, h // 2
    boxes = {(max(cx - w // 4, 0), max(cy - h // 4, 0), min(cx + max(w // 4, 1), w), min(cy + max(h // 4, 1), h)), (0, 0, cx + 1, cy + 1),
             (cx, cy, w, h), (0, cy, w, h), (cx, 0, cx, h), (0, cy, w, cy), (0, 0, 0, 0), (w, h, w, h), (0, 0, w, h)}
    return sorted(boxes)


@pytest.mark.parametrize("dtype", MOVED, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_cutmix_image_moves_the_box(shape, dtype):
    x = _batch(shape, dtype, seed=sum(shape) + 1)
    xd = x.cuda()
    for box in _boxes(shape[-2], shape[-1]):
        _equal(F.cutmix_image(xd, box), R.cutmix_image(x, box), (shape, box))


def test_cutmix_odd_offsets_video_and_views():
    x = _batch((5, 3, 37, 53), torch.uint8, seed=8)
    for box in ((1, 1, 2, 2), (15, 0, 17, 37), (16, 5, 33, 6), (31, 36, 53, 37), (7, 3, 50, 30)):
        _equal(F.cutmix_image(x.cuda(), box), R.cutmix_image(x, box), box)
    v = _batch((3, 2, 3, 10, 13), torch.float64, seed=9)
    _equal(F.cutmix_image(v.cuda(), (2, 3, 9, 8)), R.cutmix_image(v, (2, 3, 9, 8)), "5-D")
    sliced = _batch((6, 3, 12, 40), torch.int64, seed=10)
    _equal(F.cutmix_image(sliced.cuda()[1:, :, 1:, 3:], (4, 2, 20, 9)), R.cutmix_image(sliced[1:, :, 1:, 3:], (4, 2, 20, 9)), "view")
    assert F.cutmix_image(torch.zeros((0, 3, 4, 4), dtype=torch.uint8, device="cuda"), (0, 0, 2, 2)).shape == (0, 3, 4, 4)


# ---- labels -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_classes", [2, 10, 1000])
def test_index_labels(num_classes):
    g = torch.Generator().manual_seed(num_classes)
    for batch in (1, 2, 7, 256):
        labels = torch.randint(0, num_classes, (batch,), generator=g)
        if batch >= 7:
            labels[2] = labels[1]  # repeated neighbours: fl(fl(1 - lam) + fl(lam))
            labels[0] = labels[-1]  # and across the wrap
        for lam in (0.0, 1.0, DRAWN_LAM, 0.9371873140335083):
            _equal(F.mixup_labels(labels.cuda(), lam, num_classes=num_classes), R.mixup_label(labels, lam, num_classes),
                   (batch, lam))


def test_index_labels_out_of_range_match_no_class():
    """The documented choice: no read-back, a label outside [0, K) matches no class; its share of the rows it is in is zeros."""
    labels = torch.tensor([1, 9, -3, 2, 1 << 40, 0])
    out = F.mixup_labels(labels.cuda(), 0.25, num_classes=4)
    wp, ws = torch.tensor(0.75), torch.tensor(0.25)
    want = torch.zeros(6, 4)
    for b, (prev, cur) in enumerate(zip(labels.roll(1).tolist(), labels.tolist())):
        for c in range(4):
            want[b, c] = (wp if prev == c else 0.0) + (ws if cur == c else 0.0)
    _equal(out, want)


@pytest.mark.parametrize("dtype", FLOATS + [torch.int64], ids=str)
def test_probability_labels(dtype):
    for batch, k in ((7, 2), (5, 10), (256, 1000), (1, 3)):
        labels = _batch((batch, k), dtype, seed=batch + k) if dtype.is_floating_point else _batch((batch, k), dtype, batch) % 5
        _equal(F.mixup_labels(labels.cuda(), DRAWN_LAM), R.mixup_label(labels, DRAWN_LAM), (batch, k))


# ---- the transforms, end to end under seeds ---------------------------------------------------------------------------------------------
K = 10


def _sample(seed, dtype=torch.float32, shape=(8, 3, 32, 48)):
    return _batch(shape, dtype, seed), torch.randint(0, K, (shape[0],), generator=torch.Generator().manual_seed(seed))


class _Recorded(torch.nn.Module):
    """A transform that notes its name when it runs: which branch a container took."""

    def __init__(self, inner, log):
        super().__init__()
        self.inner, self.log = inner, log

    def forward(self, *inputs):
        self.log.append(type(self.inner).__name__)
        return self.inner(*inputs)


@pytest.mark.parametrize("as_dict", [False, True], ids=["pair", "dict"])
def test_random_choice_of_mixup_and_cutmix_matches_the_reference_pipeline(as_dict):
    log = []
    ours = transforms.RandomChoice([_Recorded(transforms.MixUp(num_classes=K), log), _Recorded(transforms.CutMix(num_classes=K), log)])
    ref = [R.MixUp(num_classes=K), R.CutMix(num_classes=K)]
    for seed in range(24):
        images, labels = _sample(seed)
        torch.manual_seed(seed)
        if as_dict:  # one argument: the default labels getter finds "labels" in the dict
            got = ours({"image": images.cuda(), "labels": labels.cuda(), "id": seed})
            assert got["id"] == seed
            got_images, got_labels = got["image"], got["labels"]
        else:
            got_images, got_labels = ours(images.cuda(), labels.cuda())
        assert _lib.last_kernel() == "k_mixup_labels<vec>"  # the labels come last in both branches
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        want_images, want_labels = R.random_choice(ref, None, images, labels)
        assert torch.equal(state, torch.get_rng_state()), seed
        _equal(got_images, want_images, seed), _equal(got_labels, want_labels, seed)
    assert len(log) == 24 and set(log) == {"MixUp", "CutMix"}, log  # both branches were taken over the seeds
    assert got_labels.shape == (8, K) and got_labels.dtype == torch.float32


@pytest.mark.parametrize("cls", ["MixUp", "CutMix"])
def test_dict_samples_tv_tensors_and_alpha(cls):
    for seed, alpha in enumerate((1.0, 0.05, 0.05, 3.0, 0.05)):  # alpha = 0.05: empty and edge-clipped boxes
        images, labels = _sample(seed + 40)
        ours, ref = getattr(transforms, cls)(alpha=alpha, num_classes=K), getattr(R, cls)(alpha=alpha, num_classes=K)
        torch.manual_seed(seed)
        got = ours({"image": tv_tensors.Image(images.cuda()), "Label": labels.cuda(), "name": "n", "extra": images.cuda()})
        torch.manual_seed(seed)
        want_images, want_labels = ref(images, labels)
        assert type(got["image"]) is tv_tensors.Image and got["name"] == "n"
        assert type(got["Label"]) is torch.Tensor
        _equal(got["image"].as_subclass(torch.Tensor), want_images, (alpha, seed)), _equal(got["Label"], want_labels, (alpha, seed))
        _equal(got["extra"], images, "a pure tensor next to an Image passes through")
    video = _batch((4, 2, 3, 8, 12), torch.float32, seed=50)
    labels = torch.arange(4) % K
    torch.manual_seed(3)
    got_video, got_labels = getattr(transforms, cls)(num_classes=K)(tv_tensors.Video(video.cuda()), labels.cuda())
    torch.manual_seed(3)
    want_video, want_labels = getattr(R, cls)(num_classes=K)(video, labels)
    assert type(got_video) is tv_tensors.Video
    _equal(got_video.as_subclass(torch.Tensor), want_video), _equal(got_labels, want_labels)


def test_cutmix_on_uint8_and_probability_labels_through_a_getter():
    images = _batch((6, 3, 20, 30), torch.uint8, seed=60)
    probs = torch.rand((6, K), generator=torch.Generator().manual_seed(61))
    t = transforms.CutMix(labels_getter=lambda sample: sample[1]["soft"])
    torch.manual_seed(11)
    got_images, got_target = t(images.cuda(), {"soft": probs.cuda(), "id": 5})
    torch.manual_seed(11)
    want_images, want_labels = R.CutMix()(images, probs)
    _equal(got_images, want_images), _equal(got_target["soft"], want_labels)
    assert got_target["id"] == 5


def test_random_apply_and_order_thread_the_pair():
    images, labels = _sample(70)
    mix, cut = transforms.MixUp(num_classes=K), transforms.CutMix(num_classes=K)
    torch.manual_seed(5)
    got = transforms.RandomApply([mix], p=1.0)(images.cuda(), labels.cuda())
    torch.manual_seed(5)
    want = R.random_apply([R.MixUp(num_classes=K)], 1.0, images, labels)
    _equal(got[0], want[0]), _equal(got[1], want[1])
    same = transforms.RandomApply([mix], p=0.0)(images.cuda(), labels.cuda())
    _equal(same[0], images), _equal(same[1], labels)
    # RandomOrder: the second transform sees (B, K) probability labels
    for seed in range(4):
        torch.manual_seed(seed)
        got = transforms.RandomOrder([mix, cut])(images.cuda(), labels.cuda())
        torch.manual_seed(seed)
        want = R.random_order([R.MixUp(num_classes=K), R.CutMix(num_classes=K)], images, labels)
        _equal(got[0], want[0], seed), _equal(got[1], want[1], seed)


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def test_results_are_forward_only():
    x = _batch((4, 3, 8, 8), torch.float32, seed=80).cuda().requires_grad_()
    for out in (F.mixup_image(x, 0.3), F.cutmix_image(x, (1, 1, 5, 5)), F.mixup_labels(x[:, 0, 0, :], 0.3)):
        assert out.requires_grad
        with pytest.raises(RuntimeError, match="forward-only"):
            out.sum().backward()
    with torch.no_grad():
        assert not F.mixup_image(x, 0.3).requires_grad


def test_runs_on_the_current_stream_and_the_inputs_device():
    images, labels = _sample(90, shape=(16, 3, 64, 64))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xd, ld = images.cuda(non_blocking=False), labels.cuda()
        a = F.mixup_image(xd, DRAWN_LAM)
        b = F.cutmix_image(xd, (3, 5, 40, 50))
        c = F.mixup_labels(ld, DRAWN_LAM, num_classes=K)
        # work queued behind the kernels on the same stream sees their results
        a2, b2, c2 = a.clone(), b.clone(), c.clone()
    stream.synchronize()
    for t in (a, b, c):
        assert t.device == xd.device
    _equal(a2, R.mixup_image(images, DRAWN_LAM)), _equal(b2, R.cutmix_image(images, (3, 5, 40, 50)))
    _equal(c2, R.mixup_label(labels, DRAWN_LAM, K))
