"""The MobileNetV3 kernels past element offset 2^31 ("Large offsets"; `-m gpu`), one run each, with the helpers of
tests/_large.py: the 5x5 depthwise conv and se_scale on tensors of just over 2^31 elements, the oracle on the planes at the boundary;
global_avg_pool with an image stride of 2^31 + 64 elements; the gated projection on a batch whose third image starts at element 2^31.
Every test holds less than 24 GiB of device memory (asserted)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import functional as F  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _large as L  # noqa: E402
from tests import _mobilenetv3_ref as R  # noqa: E402

CAP = 24 * 2 ** 30


@pytest.fixture(autouse=True)
def device_memory_cap():
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak <= CAP, f"the test held {peak / 2 ** 30:.1f} GiB of device memory"


def _big(shape):
    try:
        return torch.empty(shape, dtype=torch.float32, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.fail(f"{np.prod(shape) * 4 / 2 ** 30:.1f} GiB of device memory are not available")


C, H, W = 4, 256, 256
N = L.E31 // (C * H * W) + 1  # 8193 images: 4 planes past element 2^31


def _boundary_planes():
    e = L.crossings(N * C * H * W, 4)["element 2^31"]
    p = e // (H * W)  # the plane that holds element 2^31; p - 1 holds element 2^31 - 1
    return [0, p - 1, p, N * C - 1]


def test_depthwise5x5_past_2_to_31_elements():
    x = L.fill(_big((N, C, H, W)), 9971)
    wt = torch.randn((C, 1, 5, 5), generator=torch.Generator().manual_seed(9972)) * 0.3
    beta = torch.randn(C, generator=torch.Generator().manual_seed(9973))
    y = F.conv_norm_act(x, wt.cuda(), beta.cuda(), stride=2, groups=C, activation="relu")
    assert tuple(y.shape) == (N, C, H // 2, W // 2)
    planes = _boundary_planes()
    L.assert_straddles([(p * H * W, (p + 1) * H * W) for p in planes], L.E31, "input element 2^31")
    for p in planes:
        i, c = divmod(p, C)
        want = ref.conv2d_affine_act(x[i, c][None, None].cpu().numpy(), wt[c:c + 1].numpy(), beta[c:c + 1].numpy(), None, None, None, 2, 2, 1, 0, "relu")
        R.same(y[i, c], want[0, 0], f"depthwise 5x5, plane {p}")
    del x, y
    torch.cuda.empty_cache()


def test_se_scale_past_2_to_31_elements():
    x = L.fill(_big((N, C, H, W)), 9974)
    g = torch.rand((N, C), generator=torch.Generator().manual_seed(9975))
    y = F.se_scale(x, g.cuda())
    planes = _boundary_planes()
    L.assert_straddles([(p * H * W, (p + 1) * H * W) for p in planes], L.E31, "element 2^31")
    for p in planes:
        i, c = divmod(p, C)
        R.same(y[i, c], (g[i, c] * x[i, c].cpu()).numpy(), f"se_scale, plane {p}")
    del x, y
    torch.cuda.empty_cache()


def test_global_avg_pool_image_stride_past_2_to_31_elements():
    stride = 2 ** 31 + 64
    c, h, w = 5, 7, 9
    x = torch.randn((2, c, h, w), generator=torch.Generator().manual_seed(9976))
    big = _big((stride + c * h * w,))
    for i in range(2):
        big[i * stride:i * stride + c * h * w] = x[i].flatten().cuda()
    xv = torch.as_strided(big, (2, c, h, w), (stride, h * w, w, 1))
    got = F.global_avg_pool(xv)
    assert torch.equal(got[1:], F.global_avg_pool(x[1:].cuda()))
    R.same(got, R.global_avg_pool(x.numpy()), "global_avg_pool across the stride")
    del big, xv
    torch.cuda.empty_cache()


def test_scaled_projection_image_offset_past_2_to_31_elements():
    n, cin, cout, h, w = 3, 32, 3, 4096, 8192  # an image is 2^30 elements: image 2 starts at element 2^31
    x = L.fill(_big((n, cin, h, w)), 9977)
    gen = torch.Generator().manual_seed(9978)
    g, wt, beta = torch.rand((n, cin), generator=gen), torch.randn((cout, cin, 1, 1), generator=gen) * 0.2, torch.randn(cout, generator=gen)
    assert F.conv1x1_k_slices(n, cin, h, w, cout)[0] == 1
    y = F.conv_norm_act(x, wt.cuda(), beta.cuda(), activation="relu", input_scale=g.cuda())
    for i, rows in ((0, slice(0, 2)), (1, slice(h - 2, h)), (2, slice(0, 2)), (2, slice(h - 2, h))):  # both sides of element 2^31 and the ends
        xs = x[i:i + 1, :, rows].cpu().numpy()
        want = ref.conv2d_affine_act(R.se_scale(xs, g[i:i + 1].numpy()), wt.numpy(), beta.numpy(), None, None, None, 1, 0, 1, 0, "relu")
        R.same(y[i:i + 1, :, rows], want, f"scaled projection, image {i}, rows {rows}")
    del x, y
    torch.cuda.empty_cache()
