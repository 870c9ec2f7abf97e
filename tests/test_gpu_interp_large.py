"""mv_interpolate_bilinear_f32 with an output past 2^31 elements and 2^33 bytes ("Large offsets"; `-m gpu`): a tiny input,
2 planes of 16 x 16, to 32768 x 32769 in ONE launch into an output pre-filled with NaN.

  * The oracle (tests/_interp_ref.py), bit for bit, on the first rows, the last rows and the rows on both sides of every boundary
    the output crosses (tests/_large.py states the flat offsets and asserts they straddle).
  * The WHOLE output, band by band on the device, against the formula's own separable form: out = fma(wy0, T[y0], wy1 * T[y1]) with
    T the horizontal interpolation of the 16 source rows -- a launch of its own to 16 x 32769 whose every offset stays below 2^23
    bytes and which is itself compared with the oracle in full -- and the fma of tests/_interp_ref.fma32_torch.  This is what finds
    a store that wrapped to a place the sampled rows do not see.
The test holds less than 24 GiB of device memory (asserted) and the host touches a few MB."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from tests import _interp_ref as R  # noqa: E402
from tests import _large as L  # noqa: E402
from tests._util import philox_f32  # noqa: E402

CAP = 24 * 2 ** 30
PLANES, H, W, OH, OW = 2, 16, 16, 32768, 32769
BAND = 256


@pytest.fixture(autouse=True)
def device_memory_cap():
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak <= CAP, f"the test held {peak / 2 ** 30:.1f} GiB of device memory"


def test_interpolate_output_past_2_31_elements_and_2_33_bytes():
    numel = PLANES * OH * OW
    assert numel > 2 ** 31 and numel * 4 > 2 ** 33
    x = philox_f32(9500, (PLANES, H, W)) * 4 - 2
    xd = torch.from_numpy(x).cuda()
    y = torch.full((PLANES, OH, OW), float("nan"), device="cuda")
    _lib.launch(_lib.load().mv_interpolate_bilinear_f32, xd, xd.data_ptr(), y.data_ptr(), PLANES, H, W, OH, OW)
    assert _lib.last_kernel() == "k_interp_batch<plain,scalar>", _lib.last_kernel()  # 32769 % 4 != 0

    # the rows around every boundary, the first and the last, against the oracle
    crossed = L.crossings(numel, 4)
    assert set(crossed) == {"element 2^31", "byte 2^31", "byte 2^32"} and crossed["element 2^31"] * 4 == 2 ** 33
    rows = {0: {0, 1}, PLANES - 1: {OH - 2, OH - 1}}
    for e in crossed.values():
        for q in (e - 1, e):
            p, r = divmod(q // OW, OH)
            rows.setdefault(p, set()).update(v for v in (r - 1, r, r + 1) if 0 <= v < OH)
    ranges = [rg for p, rs in rows.items() for a, b in L.strips(rs) for rg in L.plane_ranges([p], OH, OW, a, b)]
    for name, e in crossed.items():
        L.assert_straddles(ranges, e, "output " + name)
    what = f"output {L.describe(ranges, 4)}; crossed {sorted(crossed)}"
    for p, rs in rows.items():
        idx = np.array(sorted(rs))
        want = R.interpolate(x[p], OH, OW, rows=idx)
        np.testing.assert_array_equal(y[p, torch.from_numpy(idx).cuda()].cpu().numpy(), want, err_msg=f"plane {p} rows {idx.tolist()}; {what}")

    # the whole output against the separable form, band by band
    t = F.interpolate(xd[None], size=[H, OW])[0]  # (planes, 16, OW): the source rows interpolated along x (src == d along y)
    np.testing.assert_array_equal(t.cpu().numpy(), R.interpolate(x, H, OW))
    y0, y1, wy0, wy1 = (torch.from_numpy(a).cuda() for a in R.axis_taps(H, OH))
    for a in range(0, OH, BAND):
        b = min(a + BAND, OH)
        top, bot = t[:, y0[a:b]], t[:, y1[a:b]]
        want = R.fma32_torch(wy0[a:b, None].expand_as(top), top, wy1[a:b, None] * bot)
        got = y[:, a:b]
        assert not bool(torch.isnan(got).any()) and torch.equal(got, want), f"rows [{a}, {b}) differ from the separable form"
