"""F.l2_normalize_scale and F.ssd_scores with an image stride past 2^31 elements ("Large offsets"; `-m gpu`): N = 2 images
2^31 + 64 elements apart in one allocation of about 8 GiB.  Image 1's result equals, bit for bit, the same image run alone, so the image
offsets of both kernels are 64-bit.  The test holds less than 10 GiB of device memory (asserted)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import functional as F  # noqa: E402
from tests import _ssd_ref as R  # noqa: E402

CAP = 10 * 2 ** 30
STRIDE = 2 ** 31 + 64


@pytest.fixture(autouse=True)
def device_memory_cap():
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak <= CAP, f"the test held {peak / 2 ** 30:.1f} GiB of device memory"


def test_image_stride_past_2_to_31_elements():
    g = torch.Generator().manual_seed(9970)
    c, h, w = 37, 5, 7
    x = torch.randn((2, c, h, w), generator=g) * 2
    wt = torch.randn(c, generator=g) + 20
    classes, a = 6, 4
    m = torch.randn((2, a * classes, h, w), generator=g) * 3
    nx, nm = c * h * w, a * classes * h * w
    try:
        big = torch.empty(STRIDE + nx + nm, dtype=torch.float32, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.fail("8 GiB of device memory are not available")
    for i in range(2):
        big[i * STRIDE:i * STRIDE + nx] = x[i].flatten().cuda()
        big[i * STRIDE + nx:i * STRIDE + nx + nm] = m[i].flatten().cuda()
    xv = torch.as_strided(big, (2, c, h, w), (STRIDE, h * w, w, 1))
    mview = torch.as_strided(big, (2, a * classes, h, w), (STRIDE, h * w, w, 1), nx)
    got = F.l2_normalize_scale(xv, wt.cuda())
    alone = F.l2_normalize_scale(x[1:].cuda(), wt.cuda())
    assert torch.equal(got[1:], alone)
    R.same(got, R.l2_normalize_scale(x, wt), "l2_normalize_scale")
    sc = F.ssd_scores([mview], classes)
    assert torch.equal(sc[1:], F.ssd_scores([m[1:].cuda()], classes))
    R.same(sc, R.scores([m], classes), "ssd_scores")
    # in place across the stride: image 1 is written where it lies
    assert F.l2_normalize_scale(xv, wt.cuda(), out=xv) is xv
    assert torch.equal(big[STRIDE:STRIDE + nx].view(1, c, h, w), alone)
    del big, xv, mview
    torch.cuda.empty_cache()
