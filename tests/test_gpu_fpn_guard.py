"""Guard-band runs of mv_conv1x1_upsample_add_f32 at the C ABI (`-m gpu`), with the helpers of tests/_guard.py and the case runner
of tests/test_gpu_layer_guard_bands.py (its assertions: the oracle's bits; nothing outside y written and y written whole; every
input bit-unchanged, NaN guards included -- a read of `top` past its last element would put a NaN into the result).  x, w, top
and y sit at element offsets 0 - 3 of their buffers: the 16-byte and the element-wise store both run where h * w % 4 == 0, the
element-wise one alone on the ragged shape; refused calls write nothing."""
import pytest

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _fpn_ref as P  # noqa: E402
from tests._util import philox_f32  # noqa: E402
from tests.test_gpu_guard_bands import _stream  # noqa: E402
from tests.test_gpu_layer_guard_bands import INVALID, _refused, _run, _t  # noqa: E402

NAMES = ["x", "w", "top", "y"]
# every tensor at offset 0 (16-byte aligned), each one alone at 1, 2, 3, and all of them at different odd offsets
OFFSETS = [dict.fromkeys(NAMES, 0)] + [{**dict.fromkeys(NAMES, 0), n: o} for n in NAMES for o in (1, 2, 3)] + [{"x": 3, "w": 1, "top": 2, "y": 1},
                                                                                                             {"x": 0, "w": 0, "top": 3, "y": 3}]
# (n, cin, h, w, cout, top_h, top_w): the ragged shape (h * w = 35: element-wise stores, two channel tiles, the last with one
# channel), one with h * w % 4 == 0 (16-byte stores where y allows), and K slices inside the workgroup
CASES = [(2, 5, 5, 7, 33, 3, 4), (2, 8, 4, 9, 33, 2, 5), (1, 192, 5, 7, 33, 3, 4)]


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("affine", [0, 1, 2])
def test_conv1x1_upsample_add(case, affine):
    lib = _lib.load()
    n, cin, h, w, cout, top_h, top_w = case
    x = philox_f32(12000 + cin + h, (n, cin, h, w)) * 2 - 1
    wt = (philox_f32(12001 + cout, (cout, cin, 1, 1)) - 0.5) * 0.5
    a, b, bias = philox_f32(12002, (cout,)) + 0.5, philox_f32(12003, (cout,)) - 0.5, philox_f32(12004, (cout,)) - 0.5
    top = philox_f32(12005, (n, cout, top_h, top_w)) * 2 - 1
    use = affine != 0
    want = _t(P.oracle_lateral(x, wt, bias, a if use else None, b if use else None, top, affine, "relu"))
    kernels = set()
    for offs in OFFSETS:
        def call(p, y, ws, nb):
            return lib.mv_conv1x1_upsample_add_f32(p["x"], p["w"], p["bias"], p["a"], p["b"], p["top"], y, n, cin, h, w, cout, top_h, top_w,
                                                   affine, 1, _stream())
        what = f"conv1x1_upsample_add {case} affine={affine} offsets={offs}"
        kernels.add(_run(what, call, {"x": _t(x), "w": _t(wt), "bias": _t(bias), "a": _t(a) if use else None, "b": _t(b) if use else None,
                                      "top": _t(top)}, {**offs, "bias": 2, "a": 1, "b": 3}, (n, cout, h, w), want))
    assert len(kernels) == 1 and kernels.pop().startswith("k_conv1x1_up<1,2,ks2>" if cin == 192 else "k_conv1x1_up<1,"), kernels


def test_refusals_write_nothing():
    lib = _lib.load()
    n, cin, h, w, cout, top_h, top_w = 2, 5, 5, 7, 33, 3, 4
    x, wt = philox_f32(12100, (n, cin, h, w)), philox_f32(12101, (cout, cin))
    a, top = philox_f32(12102, (cout,)), philox_f32(12103, (n, cout, top_h, top_w))
    inputs = {"x": _t(x), "w": _t(wt), "a": _t(a), "top": _t(top)}
    offs = {"x": 0, "w": 0, "a": 0, "top": 0, "y": 0}
    shape = (n, cin, h, w, cout)
    entry = lib.mv_conv1x1_upsample_add_f32
    refusals = [
        ("affine without alpha", lambda p, y: entry(p["x"], p["w"], None, None, p["a"], p["top"], y, *shape, top_h, top_w, 2, 1, _stream()), "affine without alpha / beta"),
        ("no top", lambda p, y: entry(p["x"], p["w"], None, None, None, None, y, *shape, top_h, top_w, 0, 1, _stream()), "null pointer"),
        ("top_h = 0", lambda p, y: entry(p["x"], p["w"], None, None, None, p["top"], y, *shape, 0, top_w, 0, 1, _stream()), "bad top size"),
        ("top is y", lambda p, y: entry(p["x"], p["w"], None, None, None, y, y, *shape, top_h, top_w, 0, 1, _stream()), "must not overlap"),
        ("top overlaps y's end", lambda p, y: entry(p["x"], p["w"], None, None, None, y + 4 * (n * cout * h * w - 1), y, *shape, top_h, top_w, 0, 1,
                                                    _stream()), "must not overlap"),
        ("bad activation code", lambda p, y: entry(p["x"], p["w"], None, None, None, p["top"], y, *shape, top_h, top_w, 0, 9, _stream()), "bad affine"),
    ]
    for what, call, message in refusals:
        _refused(what, lambda p, y, wsp, nb, call=call: call(p, y), inputs, offs, (n, cout, h, w), INVALID, message=message)
