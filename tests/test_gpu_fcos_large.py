"""F.group_norm_act on ONE allocation whose element offsets pass 2^31 and whose byte offsets pass 2^33 ("Large offsets";
`-m gpu`): x (1, 66, 1, 2^25) in 66 groups, so that group 63 ends at element 2^31 and group 64 starts there, into an output pre-filled
with NaN.  The slabs on both sides of the boundary, the first and the last equal, bit for bit, the same slabs run alone (a group's
result depends on its own values only); every element of the output was written, and every slab is normalised.  The test holds less
than 24 GiB of device memory (asserted)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402

CAP = 24 * 2 ** 30
GROUPS, M = 66, 2 ** 25


@pytest.fixture(autouse=True)
def device_memory_cap():
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak <= CAP, f"the test held {peak / 2 ** 30:.1f} GiB of device memory"


def test_group_norm_past_2_31_elements():
    assert 64 * M == 2 ** 31 and GROUPS * M * 4 > 2 ** 33
    g = torch.Generator(device="cuda").manual_seed(9950)
    try:
        x = torch.randn((1, GROUPS, 1, M), generator=g, device="cuda")
        y = torch.full((1, GROUPS, 1, M), float("nan"), device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.fail("17 GiB of device memory are not available")
    x.mul_(torch.arange(1, GROUPS + 1, device="cuda").view(1, -1, 1, 1) * 0.125).add_(torch.arange(GROUPS, device="cuda").view(1, -1, 1, 1) - 30.0)
    gamma = torch.randn(GROUPS, generator=g, device="cuda") + 1
    beta = torch.randn(GROUPS, generator=g, device="cuda")
    lib = _lib.load()
    nbytes = int(lib.mv_group_norm_workspace_bytes(1, GROUPS, 1, M, GROUPS))
    assert nbytes == GROUPS * (M // F.group_norm_chunk()) * 16
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.launch(lib.mv_group_norm_act_f32, x, x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1, GROUPS, 1, M, GROUPS, GROUPS * M,
                GROUPS * M, 1e-5, 0, ws.data_ptr(), nbytes)
    assert _lib.last_kernel() == "k_gn_apply<vec,relu0>"
    for grp in (0, 62, 63, 64, 65):  # 63 ends at element 2^31, 64 starts there
        alone = F.group_norm_act(x[:, grp:grp + 1].clone(), 1, gamma[grp:grp + 1], beta[grp:grp + 1])
        assert torch.equal(y[:, grp:grp + 1], alone), f"group {grp} differs from the same slab run alone"
    assert not bool(torch.isnan(y).any()), "an element of the output was not written"
    # every slab is normalised: mean beta, standard deviation |gamma|
    flat = y.view(GROUPS, M)
    mean = torch.stack([flat[i].double().mean() for i in range(GROUPS)])  # slab by slab: a float64 copy of one slab at a time
    std = torch.stack([flat[i].double().std() for i in range(GROUPS)])
    assert float((mean - beta.double()).abs().max()) < 1e-3 and float((std - gamma.double().abs()).abs().max()) < 1e-3
    # in place, relu: the same bits as max(y, 0)
    want = torch.relu(y[:, 60:])
    del y
    F.group_norm_act(x, GROUPS, gamma, beta, relu=True, out=x)
    assert torch.equal(x[:, 60:], want)
