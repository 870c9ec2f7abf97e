"""Guard-band runs of mv_conv2d_affine_act_f32 and mv_maxpool2d_pad_f32 at the C ABI (`-m gpu`), with the helpers of tests/_guard.py
and the case runner of tests/test_gpu_layer_guard_bands.py (its four assertions: the oracle's bits; nothing outside y written and y
written whole; every input bit-unchanged, NaN guards included; a workspace of exactly the queried bytes keeps its guards and gives
the same bits on 0xFF and on 0x00 garbage).  y, residual, x and weight sit at element offsets 0 - 3 of their buffers, so the 16-byte
and the element-wise forms of the residual load, the store and the weight load all run; refused calls write nothing."""
import pytest

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from tests import _resnet_ref as R  # noqa: E402
from tests._util import philox_f32  # noqa: E402
from tests.test_gpu_guard_bands import _stream  # noqa: E402
from tests.test_gpu_layer_guard_bands import INVALID, _refused, _run, _t  # noqa: E402

NAMES = ["x", "w", "res", "y"]
# every tensor at offset 0 (16-byte aligned), each one alone at 1, 2, 3, and all of them at different odd offsets
OFFSETS = [dict.fromkeys(NAMES, 0)] + [{**dict.fromkeys(NAMES, 0), n: o} for n in NAMES for o in (1, 2, 3)] + [{"x": 3, "w": 1, "res": 2, "y": 1},
                                                                                                             {"x": 0, "w": 0, "res": 3, "y": 3}]
# (n, cin, h, w, cout, k, stride, pad, dilation, groups): oh * ow % 4 == 0 (16-byte stores where y allows) and != 0
CASES = [(2, 5, 8, 8, 70, 3, 1, 1, 1, 1), (2, 4, 9, 7, 33, 3, 1, 1, 1, 1), (1, 3, 17, 16, 64, 7, 2, 3, 1, 1), (2, 6, 9, 8, 10, 3, 1, 2, 2, 2)]


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("affine", [1, 2])
def test_conv2d_affine_act(case, affine):
    lib = _lib.load()
    n, cin, h, w, cout, k, stride, pad, dil, groups = case
    geometry = (k, k, stride, stride, pad, pad, dil, dil)
    assert lib.mv_conv2d_needs_workspace(n, cin, cout, h, w, *geometry, groups) == 2  # optional: both forms run below
    span = dil * (k - 1) + 1
    oh, ow = (h + 2 * pad - span) // stride + 1, (w + 2 * pad - span) // stride + 1
    x = philox_f32(11000 + cin + h, (n, cin, h, w)) * 2 - 1
    wt = (philox_f32(11001 + cout, (cout, cin // groups, k, k)) - 0.5) * 0.5
    a, b = philox_f32(11002, (cout,)) + 0.5, philox_f32(11003, (cout,)) - 0.5
    res = philox_f32(11004, (n, cout, oh, ow)) - 0.5
    want = _t(R.oracle_conv(x, wt, None, a, b, res, stride, pad, dil, groups, affine, "relu"))
    ws_one = int(lib.mv_deform_conv2d_workspace_bytes(1, cin, h, w, *geometry))
    assert ws_one == 4 * cin * k * k * oh * ow
    kernels = set()
    for offs in OFFSETS:
        for ws_bytes in (0, ws_one):
            def call(p, y, ws, nb):
                return lib.mv_conv2d_affine_act_f32(p["x"], p["w"], None, p["a"], p["b"], p["res"], y, n, cin, h, w, cout, *geometry, groups,
                                                    affine, 1, ws, nb, _stream())
            what = f"conv2d_affine_act {case} affine={affine} offsets={offs} workspace={ws_bytes}"
            kernel = _run(what, call, {"x": _t(x), "w": _t(wt), "a": _t(a), "b": _t(b), "res": _t(res)}, {**offs, "a": 1, "b": 3},
                          (n, cout, oh, ow), want, ws_bytes=ws_bytes)
            assert kernel.startswith("k_conv1x1<" if ws_bytes else "k_conv_igemm_full<"), (what, kernel)
            kernels.add(kernel.split("<")[0])
    assert kernels == {"k_conv1x1", "k_conv_igemm_full"}


def test_conv2d_affine_act_refusals_write_nothing():
    lib = _lib.load()
    n, cin, h, w, cout = 2, 5, 8, 8, 70
    x, wt = philox_f32(11100, (n, cin, h, w)), philox_f32(11101, (cout, cin, 3, 3))
    a = philox_f32(11102, (cout,))
    inputs = {"x": _t(x), "w": _t(wt), "a": _t(a)}
    offs = {"x": 0, "w": 0, "a": 0, "y": 0}
    ws = int(lib.mv_deform_conv2d_workspace_bytes(1, cin, h, w, 3, 3, 1, 1, 1, 1, 1, 1))
    tail = (n, cin, h, w, cout, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    _refused("affine without alpha", lambda p, y, wsp, nb: lib.mv_conv2d_affine_act_f32(p["x"], p["w"], None, None, p["a"], None, y, *tail, 2, 1,
                                                                                         wsp, nb, _stream()),
             inputs, offs, (n, cout, h, w), INVALID, ws_bytes=ws, message="affine without alpha / beta")
    _refused("residual is y", lambda p, y, wsp, nb: lib.mv_conv2d_affine_act_f32(p["x"], p["w"], None, p["a"], p["a"], y, y, *tail, 2, 1, wsp, nb,
                                                                                  _stream()),
             inputs, offs, (n, cout, h, w), INVALID, ws_bytes=ws, message="must not overlap")
    _refused("residual overlaps y", lambda p, y, wsp, nb: lib.mv_conv2d_affine_act_f32(p["x"], p["w"], None, p["a"], p["a"], y + 64, y, *tail, 2, 1,
                                                                                        wsp, nb, _stream()),
             inputs, offs, (n, cout, h, w), INVALID, ws_bytes=ws, message="must not overlap")
    _refused("bad affine code", lambda p, y, wsp, nb: lib.mv_conv2d_affine_act_f32(p["x"], p["w"], None, p["a"], p["a"], None, y, *tail, 3, 1, wsp,
                                                                                    nb, _stream()),
             inputs, offs, (n, cout, h, w), INVALID, ws_bytes=ws, message="bad affine")
    small = (n, cin, 2, 2, cout, 3, 3, 1, 1, 0, 0, 1, 1, 1)
    _refused("no output", lambda p, y, wsp, nb: lib.mv_conv2d_affine_act_f32(p["x"], p["w"], None, p["a"], p["a"], None, y, *small, 2, 1, wsp, nb,
                                                                              _stream()),
             inputs, offs, (n, cout, h, w), INVALID, ws_bytes=ws, message="output size too small")


POOLS = [((6, 7, 7), 3, 2, 1), ((3, 17, 33), 3, 2, 1), ((4, 8, 12), 3, 1, 1), ((2, 17, 33), 5, 2, 2), ((5, 1, 9), 3, 2, 1)]


@pytest.mark.parametrize("shape,k,stride,pad", POOLS, ids=str)
def test_maxpool2d_pad(shape, k, stride, pad):
    lib = _lib.load()
    planes, h, w = shape
    x = philox_f32(11200 + w, shape) * 4 - 3  # mostly negative: a zero read from a padded position would win
    want = _t(R.padded_max_pool(x, k, stride, pad))
    for off in range(4):
        for offs in ({"x": off, "y": 3 - off}, {"x": 0, "y": off}):
            kernel = _run(f"maxpool2d_pad {shape} k={k} s={stride} p={pad} offsets={offs}",
                          lambda p, y, ws, nb: lib.mv_maxpool2d_pad_f32(p["x"], y, planes, h, w, k, stride, pad, _stream()), {"x": _t(x)}, offs,
                          tuple(want.shape), want)
            assert kernel == "k_maxpool2d_pad"


def test_maxpool2d_pad_refusals_write_nothing():
    lib = _lib.load()
    x = philox_f32(11300, (3, 6, 6))
    for what, args, message in (("pad > k / 2", (3, 6, 6, 3, 2, 2), "pad should be at most half"), ("negative pad", (3, 6, 6, 3, 2, -1), "pad should"),
                                ("no output", (3, 1, 6, 4, 1, 1), "Output size is too small"), ("stride 0", (3, 6, 6, 3, 0, 1), "bad pooling shape")):
        _refused(what, lambda p, y, ws, nb, args=args: lib.mv_maxpool2d_pad_f32(p["x"], y, *args, _stream()), {"x": _t(x)}, {"x": 0, "y": 0},
                 (3, 6, 6), INVALID, message=message)
