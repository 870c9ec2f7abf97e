"""MixUp / CutMix / RandomApply / RandomChoice / RandomOrder without a GPU: constructor and input checks with the reference's
messages, the labels getter, the host RNG draws against the restated reference (tests/_mix_ref.py) with the RNG state afterwards,
the rounding sequence the kernel implements against the reference's own arithmetic, and the ABI's argument checks."""
import pytest
import torch

from cpu_vision_amd import _lib, _pil, functional as F, transforms, tv_tensors
from tests import _mix_ref as R

SEEDS = range(100)


# ---- constructors ---------------------------------------------------------------------------------------------------------------------
def test_containers_check_their_arguments():
    with pytest.raises(TypeError, match="should be a sequence of callables or a `nn.ModuleList`"):
        transforms.RandomApply(lambda x: x)
    with pytest.raises(ValueError, match=r"`p` should be a floating point value in the interval \[0.0, 1.0\]"):
        transforms.RandomApply([lambda x: x], p=1.5)
    transforms.RandomApply(torch.nn.ModuleList([transforms.MixUp(num_classes=3)]))
    with pytest.raises(TypeError, match="should be a sequence of callables"):
        transforms.RandomChoice(lambda x: x)
    with pytest.raises(ValueError, match="Length of p doesn't match the number of transforms: 1 != 2"):
        transforms.RandomChoice([lambda x: x, lambda x: x], p=[1.0])
    with pytest.raises(TypeError, match="should be a sequence of callables"):
        transforms.RandomOrder(lambda x: x)


def test_random_choice_normalises_p():
    t = transforms.RandomChoice([lambda x: x] * 3, p=[1, 2, 5])
    assert t.p == [1 / 8, 2 / 8, 5 / 8]
    assert transforms.RandomChoice([lambda x: x] * 4).p == [0.25] * 4


def test_mixup_cutmix_constructor():
    for cls in (transforms.MixUp, transforms.CutMix):
        t = cls(alpha=2, num_classes=10)
        assert t.alpha == 2.0 and isinstance(t.alpha, float) and t.num_classes == 10
        with pytest.raises(ValueError, match="labels_getter should either be 'default', a callable, or None"):
            cls(labels_getter="labels")
        with pytest.raises(TypeError):
            cls(0.5)  # keyword-only, as in the reference


# ---- the labels getter ---------------------------------------------------------------------------------------------------------------
def test_labels_getter_on_tuple_dict_and_callable():
    default = transforms._parse_labels_getter("default")
    labels, image = torch.arange(4), torch.zeros(4, 3, 2, 2)
    assert default((image, labels)) is labels
    assert default([image, labels]) is labels
    assert default((image, {"boxes": 1, "Labels": labels})) is labels
    assert default({"image": image, "LABEL": labels}) is labels
    with pytest.raises(ValueError, match="Could not infer where the labels are"):
        default({"image": image, "target": labels})
    with pytest.raises(ValueError, match="must be a dictionary or a two-tuple"):
        default((image, "labels"))
    getter = lambda sample: sample["t"]["y"]  # noqa: E731
    assert transforms._parse_labels_getter(getter) is getter
    assert transforms._parse_labels_getter(None)((image, labels)) is None


@pytest.mark.parametrize("cls", ["MixUp", "CutMix"])
def test_input_checks_come_before_any_device_work(cls):
    make = getattr(transforms, cls)
    image = torch.zeros(4, 3, 8, 8)
    with pytest.raises(ValueError, match=r"The labels must be a tensor, but got <class 'NoneType'> instead."):
        make(num_classes=3, labels_getter=None)(image, torch.arange(4))
    with pytest.raises(ValueError, match="The labels must be a tensor, but got <class 'int'> instead."):
        make(num_classes=3, labels_getter=lambda s: 3)(image, torch.arange(4))
    with pytest.raises(ValueError, match="labels should be index based"):
        make(num_classes=3)(image, torch.zeros(4, 3, 1))
    with pytest.raises(ValueError, match="must match num_classes: 5 != 3"):
        make(num_classes=3)(image, torch.zeros(4, 5))
    with pytest.raises(ValueError, match=r"num_classes must be passed if the labels are index-based \(1D\)"):
        make()(image, torch.arange(4))
    with pytest.raises(ValueError, match="Expected a batched input with 4 dims, but got 3 dimensions instead."):
        make(num_classes=3)(image[0], torch.arange(4))
    with pytest.raises(ValueError, match="Expected a batched input with 5 dims, but got 4 dimensions instead."):
        make(num_classes=3)(tv_tensors.Video(image), torch.arange(4))
    with pytest.raises(ValueError, match="does not match the batch size of the labels: 4 != 5."):
        make(num_classes=3)(image, torch.arange(5))
    for bad in (tv_tensors.Mask(torch.zeros(4, 8, 8)), tv_tensors.BoundingBoxes(torch.zeros(4, 4))):
        with pytest.raises(ValueError, match=rf"{cls}\(\) does not support PIL images, bounding boxes and masks."):
            make(num_classes=3)(image, torch.arange(4), bad)
    if _pil.PIL is not None:
        with pytest.raises(ValueError, match=rf"{cls}\(\) does not support PIL images, bounding boxes and masks."):
            make(num_classes=3)(_pil.PIL.Image.new("RGB", (8, 8)), torch.arange(4))


def test_no_cpu_fallback():
    image, labels = torch.rand(4, 3, 8, 8), torch.arange(4) % 3
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.mixup_image(image, 0.3)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.cutmix_image(image, (1, 2, 5, 6))
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.mixup_labels(labels, 0.3, num_classes=3)
    with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
        F.mixup_labels(torch.rand(4, 3), 0.3)
    for cls in (transforms.MixUp, transforms.CutMix):
        with pytest.raises(_lib.Mi355VisionError, match="no CPU"):
            cls(num_classes=3)(image, labels)


def test_functional_argument_checks():
    with pytest.raises(TypeError, match="convert first"):
        F.mixup_image(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), 0.5)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        F.mixup_image(torch.zeros(4, 3, 8, 8, dtype=torch.bfloat16), 0.5)
    with pytest.raises(NotImplementedError, match="complex64"):
        F.cutmix_image(torch.zeros(4, 3, 8, 8, dtype=torch.complex64), (0, 0, 1, 1))
    for box in ((-1, 0, 4, 4), (0, 0, 9, 4), (5, 0, 4, 4), (0, 6, 4, 5)):
        with pytest.raises(ValueError, match="must lie inside"):
            F.cutmix_image(torch.zeros(4, 3, 8, 8), box)
    with pytest.raises(ValueError, match="num_classes must be passed"):
        F.mixup_labels(torch.arange(4), 0.5)
    with pytest.raises(RuntimeError, match="one_hot is only applicable to index tensor"):
        F.mixup_labels(torch.arange(4, dtype=torch.int32), 0.5, num_classes=4)
    with pytest.raises(ValueError, match="labels should be index based"):
        F.mixup_labels(torch.zeros(2, 2, 2), 0.5)


# ---- draws ----------------------------------------------------------------------------------------------------------------------------
def _tagger(tag, log):
    def fn(*inputs):
        log.append(tag)
        return tuple(f"{tag}({i})" for i in inputs) if len(inputs) > 1 else f"{tag}({inputs[0]})"

    return fn


def _run_both(ours, ref):
    """Run the transform and the reference under every seed: same picks, same outputs, same RNG state afterwards."""
    for seed in SEEDS:
        for inputs in (("x",), ("x", "y")):
            log, ref_log = [], []
            torch.manual_seed(seed)
            got = ours(log)(*inputs)
            state = torch.get_rng_state()
            torch.manual_seed(seed)
            want = ref(ref_log, *inputs)
            assert got == want and log == ref_log, (seed, inputs)
            assert torch.equal(state, torch.get_rng_state()), seed


def test_random_choice_picks_what_the_reference_picks():
    for p in (None, [0.1, 0.6, 0.3], [3, 1, 1]):
        make = lambda log: [_tagger(t, log) for t in "abc"]  # noqa: E731
        _run_both(lambda log: transforms.RandomChoice(make(log), p=p), lambda log, *i: R.random_choice(make(log), p, *i))


def test_random_order_runs_in_the_reference_order():
    make = lambda log: [_tagger(t, log) for t in "abcd"]  # noqa: E731
    _run_both(lambda log: transforms.RandomOrder(make(log)), lambda log, *i: R.random_order(make(log), *i))


def test_random_apply_applies_when_the_reference_does():
    for p in (0.0, 0.3, 0.5, 1.0):
        make = lambda log: [_tagger(t, log) for t in "ab"]  # noqa: E731
        _run_both(lambda log: transforms.RandomApply(make(log), p=p), lambda log, *i: R.random_apply(make(log), p, *i))


def _draw(transform, image, seed):
    torch.manual_seed(seed)
    params = transform._get_params([image])
    return params, torch.get_rng_state()


def test_mixup_draws_the_reference_lam():
    image = torch.zeros(2, 3, 4, 4)
    for alpha in (1.0, 0.2, 4.0):
        t = transforms.MixUp(alpha=alpha, num_classes=2)
        for seed in SEEDS:
            got, state = _draw(t, image, seed)
            torch.manual_seed(seed)
            assert got == R.mixup_params(R.beta(alpha))
            assert torch.equal(state, torch.get_rng_state())


def test_cutmix_draws_the_reference_box():
    """Over the seeds: interior boxes, boxes clipped at each edge, and (alpha = 0.05, lam next to 1) empty ones."""
    H, W = 32, 48
    image = torch.zeros(2, 3, H, W)
    kinds = {"interior": 0, "clipped": 0, "empty": 0}
    for alpha in (1.0, 0.05):
        t = transforms.CutMix(alpha=alpha, num_classes=2)
        for seed in SEEDS:
            got, state = _draw(t, image, seed)
            torch.manual_seed(seed)
            want = R.cutmix_params(R.beta(alpha), H, W)
            assert got == want, (alpha, seed)
            assert torch.equal(state, torch.get_rng_state())
            x1, y1, x2, y2 = got["box"]
            assert 0 <= x1 <= x2 <= W and 0 <= y1 <= y2 <= H
            if (x2 - x1) * (y2 - y1) == 0:
                kinds["empty"] += 1
                assert got["lam"] == 1.0
            elif x1 == 0 or y1 == 0 or x2 == W or y2 == H:
                kinds["clipped"] += 1
            else:
                kinds["interior"] += 1
    assert all(kinds.values()), kinds
    # the seeds the GPU tests use by name
    got, _ = _draw(transforms.CutMix(alpha=0.05, num_classes=2), image, 1)
    assert (got["box"][2] - got["box"][0]) * (got["box"][3] - got["box"][1]) == 0
    got, _ = _draw(transforms.CutMix(alpha=1.0, num_classes=2), image, 1)
    x1, y1, x2, y2 = got["box"]
    assert (x2 - x1) * (y2 - y1) > 0 and (x1 == 0 or y1 == 0 or x2 == W or y2 == H)


# ---- the rounding sequence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.float64], ids=str)
def test_kernel_rounding_sequence_is_the_reference_arithmetic(dtype):
    """csrc/batchmix.hip computes fl(fl(prev * wp) + fl(self * ws)) with wp = 1 - lam, ws = lam narrowed to the compute type
    (float32 for float16 storage, each result rounded to float16).  Spelled out with separately rounded torch ops it equals the
    reference's roll / mul_ / add_ bit for bit, and a contracted fma form does not.

    This is a check of the specification on the host, not of the kernel: it calls no code of the package and cannot catch a
    kernel regression (tests/test_gpu_mix.py does that).  It is what entitles the GPU tests to torch.equal."""
    g = torch.Generator().manual_seed(5)
    x = (torch.rand((9, 3, 31, 33), generator=g, dtype=torch.float32) * 2 - 1).to(dtype)
    compute = torch.float64 if dtype == torch.float64 else torch.float32
    for lam in (0.0, 1.0, 0.3, 0.9371873140335083, 1e-3):
        wp, ws = torch.tensor(1.0 - lam, dtype=compute), torch.tensor(lam, dtype=compute)
        prev, self_ = x.roll(1, 0).to(compute), x.to(compute)
        a, b = (prev * wp).to(dtype), (self_ * ws).to(dtype)
        spelled = (a.to(compute) + b.to(compute)).to(dtype)
        want = R.mixup_image(x, lam)
        assert torch.equal(spelled, want), lam
    if dtype == torch.float32:
        wp, ws = torch.tensor(0.7, dtype=torch.float32), torch.tensor(0.3, dtype=torch.float32)
        fma = torch.addcmul((x.roll(1, 0) * wp).double(), x.double(), ws.double()).float()  # fma(self, ws, fl(prev * wp))
        assert (fma != R.mixup_image(x, 0.3)).float().mean() > 0.05


def test_label_arithmetic_keeps_the_three_roundings():
    """A one_hot row whose neighbour has the same label holds fl(fl(1 - lam) + fl(lam)) in its hot column, the other rows
    fl(1 - lam) and fl(lam): what mv_mixup_labels_i64 computes from the two indices alone.  Like the test above this checks
    the specification on the host and calls no code of the package; the kernel is held to it in tests/test_gpu_mix.py."""
    labels = torch.tensor([2, 2, 0, 1, 1, 1, 0])
    for seed in range(50):
        lam = float(torch.rand((), generator=torch.Generator().manual_seed(seed), dtype=torch.float64))
        want = R.mixup_label(labels, lam, 3)
        f = torch.tensor([1.0 - lam, lam], dtype=torch.float64).float()
        assert want[1, 2] == f[0] + f[1]
        assert want[2, 2] == f[0] and want[2, 0] == f[1] and want[2, 1] == 0


# ---- the ABI's own checks ---------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments_without_a_device():
    lib = _lib.load()
    rc = lib.mv_mixup_f32(16, 16, 2, 8, 0.5, None)
    assert rc == -1 and b"alias" in lib.mv_last_error()
    rc = lib.mv_mixup_f16(16, 32, -1, 8, 0.5, None)
    assert rc == -1 and b"bad shape" in lib.mv_last_error()
    rc = lib.mv_mixup_f64(None, 32, 2, 8, 0.5, None)
    assert rc == -1 and b"null" in lib.mv_last_error()
    rc = lib.mv_mixup_f32(16, 32, 2, 8, float("nan"), None)
    assert rc == -1 and b"NaN" in lib.mv_last_error()
    assert lib.mv_mixup_f32(None, None, 0, 8, 0.5, None) == 0  # empty work
    assert lib.mv_mixup_f32(None, None, 4, 0, 0.5, None) == 0
    rc = lib.mv_cutmix(16, 32, 2, 3, 3, 8, 8, 0, 0, 4, 4, None)
    assert rc == -1 and b"elem_bytes" in lib.mv_last_error()
    for box in ((2, 2, 9, 4), (-1, 0, 4, 4), (3, 0, 2, 4), (0, 5, 4, 4), (0, 0, 4, 9)):
        rc = lib.mv_cutmix(16, 32, 2, 3, 1, 8, 8, *box, None)
        assert rc == -1 and b"must lie inside" in lib.mv_last_error(), box
    rc = lib.mv_cutmix(16, 16, 2, 3, 1, 8, 8, 0, 0, 4, 4, None)
    assert rc == -1 and b"alias" in lib.mv_last_error()
    assert lib.mv_cutmix(None, None, 0, 3, 1, 8, 8, 0, 0, 4, 4, None) == 0
    rc = lib.mv_mixup_labels_i64(16, 32, 2, 0, 0.5, None)
    assert rc == -1 and b"num_classes" in lib.mv_last_error()
    rc = lib.mv_mixup_labels_i64(None, 32, 2, 4, 0.5, None)
    assert rc == -1 and b"null" in lib.mv_last_error()
    assert lib.mv_mixup_labels_i64(None, None, 0, 4, 0.5, None) == 0
