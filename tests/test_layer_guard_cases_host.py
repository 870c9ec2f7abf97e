"""tests/_layer_guard_cases.py against the library's host-only plan queries (no GPU): every case takes the plan its row claims --
single chain or K slices, slice length, workspace bytes -- so that a change to a plan cannot quietly empty a sweep of
tests/test_gpu_layer_guard_bands.py, and the table is checked before any GPU time is spent."""
import ctypes as C

import pytest

from cpu_vision_amd import _lib
from tests import _layer_guard_cases as T


def _conv3x3_plan(lib, n, cin, cout, h, w):
    sc = C.c_int(0)
    slices = lib.mv_conv3x3_k_slices(n, cin, h, w, cout, C.byref(sc))
    return slices, sc.value, int(lib.mv_conv3x3_workspace_bytes(n, cin, h, w, cout))


@pytest.mark.parametrize("case", T.CONV3X3, ids=lambda c: "-".join(map(str, c["shape"])) + "".join(f",{k[8:]}={v}" for k, v in c["env"].items()))
def test_conv3x3_plans(case, monkeypatch):
    n, cin, cout, h, w = case["shape"]
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    with _lib.tuning_library() if case["env"] else _NoSwitch() as lib:
        slices, sc, ws = _conv3x3_plan(lib, n, cin, cout, h, w)
    assert (slices, sc) == (case["slices"], case["slice_channels"]), case
    assert ws == (4 * slices * n * cout * h * w if slices > 1 else 0), case
    assert ("reduce" in case["kernel"]) == (slices > 1), case
    if "k_conv3x3_c3" == case["kernel"]:
        assert cin == 3 and cout <= 64 and w % 4 == 0
    if case["kernel"] == "k_conv3x3":
        assert w > 510  # whole rows do not fit k_conv3x3_gen's tile


class _NoSwitch:
    def __enter__(self):
        return _lib.load()

    def __exit__(self, *exc):
        return False


def test_conv3x3_table_reaches_every_form():
    envs = [c["env"] for c in T.CONV3X3]
    for shape in ("0", "1", "2"):
        assert any(e.get("MV_CONV_SHAPE") == shape for e in envs)
    for knob in ("MV_CONV_SPEC42", "MV_CONV_DENSE"):
        assert {e[knob] for e in envs if knob in e} == {"0", "1"}
    assert {e["MV_CONV_GROUP"] for e in envs if "MV_CONV_GROUP" in e} == {"3", "64"}
    assert {c["shape"][4] for c in T.CONV3X3} >= {3, 5, 12, 13, 14, 33}
    assert {c["shape"][1] for c in T.CONV3X3} >= {4, 5, 13, 130}
    assert {c["shape"][2] for c in T.CONV3X3} >= {8, 33, 40, 130}
    assert any(c["slices"] > 1 and c["shape"][1] >= 256 and c["shape"][3:] == (7, 7) for c in T.CONV3X3)
    for n, cout, h, w in T.CONV3X3_U8NORM:
        assert cout <= 64 and w % 4 == 0
    assert T.CONV3X3_U8NORM_REFUSED_WIDTH[3] % 4 != 0


@pytest.mark.parametrize("case", T.LINEAR, ids=lambda c: "-".join(map(str, c["shape"])))
def test_linear_plans(case):
    lib = _lib.load()
    n, k, m = case["shape"]
    sl = C.c_int(0)
    slices = lib.mv_linear_k_slices(n, k, m, C.byref(sl))
    assert (slices, sl.value, int(lib.mv_linear_workspace_bytes(n, k, m))) == (case["slices"], case["slice_len"], case["workspace"]), case
    assert case["workspace"] == (4 * slices * n * m if slices > 1 else 0)
    assert ("reduce" in case["kernel"]) == (slices > 1)


def test_linear_table_reaches_every_form():
    sliced = [c for c in T.LINEAR if c["slices"] > 1]
    single = [c for c in T.LINEAR if c["slices"] == 1]
    for group in (sliced, single):
        for small in (True, False):  # n <= 4: k_linear_gemv when k % 4 == 0
            ks = {c["shape"][1] % 4 == 0 for c in group if (c["shape"][0] <= 4) == small}
            assert True in ks, (small, group)
    assert any(c["shape"][1] % 4 for c in sliced) and any(c["shape"][1] % 4 for c in single)
    assert any(c["shape"][2] % 4 == 0 for c in sliced)  # vec_y decided by the workspace pointer
    assert any(c["shape"][0] <= 4 and c["shape"][2] > 128 and c["shape"][2] % 128 for c in T.LINEAR)
    assert any(c["shape"][0] == 4 and c["shape"][1] % 4 == 0 and c["shape"][2] > 128 and c["shape"][2] % 128 for c in single)  # unsliced k_linear_gemv, n = 4


@pytest.mark.parametrize("case", T.POINTWISE, ids=lambda c: "-".join(map(str, c["shape"])))
def test_pointwise_plans(case):
    lib = _lib.load()
    n, cin, cout, h, w = case["shape"]
    sl = C.c_int(0)
    slices = lib.mv_conv1x1_k_slices(n, cin, h, w, cout, C.byref(sl))
    assert (slices, sl.value) == (case["slices"], case["slice_len"]), case
    if slices > 1:
        assert sl.value % 32 == 0 and (slices - 1) * sl.value < cin <= slices * sl.value


def test_conv_norm_act_table_reaches_every_flag():
    assert any(c["slices"] > 1 for c in T.POINTWISE) and any(c["slices"] == 1 for c in T.POINTWISE)
    hw4 = {(c["shape"][3] * c["shape"][4]) % 4 == 0 for c in T.POINTWISE}
    k4 = {c["shape"][1] % 4 == 0 for c in T.POINTWISE}
    assert hw4 == {True, False} and k4 == {True, False}
    for (n, c, h, w, stride), kernel, _ in T.DEPTHWISE:
        small = w in (7, 14, 28) and h <= 28  # launch_dwpc3x3: whole planes through LDS, on a 16-byte x
        assert kernel.startswith("k_dwpc3x3_small") == small, (n, c, h, w, stride)
        if small:
            assert kernel == f"k_dwpc3x3_small<{w},s{stride}>"
    # `aligned` of k_dwpc3x3 decided by x alone: W % (4 * stride) == 0 and planes * strips * groups_x % 64 == 0 (one strip here)
    alone = [(n, c, h, w, s) for (n, c, h, w, s), kernel, _ in T.DEPTHWISE if kernel == "k_dwpc3x3" and w % (4 * s) == 0]
    assert {s for *_, s in alone} == {1, 2}
    for n, c, h, w, s in alone:
        ow = (w - 1) // s + 1
        assert (n * c * ((ow + 3) // 4)) % 64 == 0 and (h - 1) // s + 1 <= 4
    for n, cin, cout, h, w, stride in T.STEM:
        assert cin <= 4 and stride in (1, 2)


def _geometry(case):
    k, stride, pad, dil = case["k"], case["stride"], case["pad"], case["dil"]
    n, cin, cout, h, w = case["shape"]
    oh = (h + 2 * pad[0] - (dil[0] * (k[0] - 1) + 1)) // stride[0] + 1
    ow = (w + 2 * pad[1] - (dil[1] * (k[1] - 1) + 1)) // stride[1] + 1
    return (k[0], k[1], stride[0], stride[1], pad[0], pad[1], dil[0], dil[1]), oh, ow


@pytest.mark.parametrize("case", T.CONV2D, ids=lambda c: "-".join(map(str, c["shape"])))
def test_conv2d_plans(case):
    """Every row is a small launch: 2 = the implicit kernel without a workspace, the columns form with one of exactly
    mv_deform_conv2d_workspace_bytes; hw4 / k4 state the shape halves of vec_y / vec_w."""
    lib = _lib.load()
    n, cin, cout, h, w = case["shape"]
    geometry, oh, ow = _geometry(case)
    assert lib.mv_conv2d_needs_workspace(n, cin, cout, h, w, *geometry, case["groups"]) == 2, case
    for images in (1, n):
        assert int(lib.mv_deform_conv2d_workspace_bytes(images, cin, h, w, *geometry)) == 4 * images * cin * geometry[0] * geometry[1] * oh * ow
    assert case["hw4"] == (oh * ow % 4 == 0) and case["k4"] == (cin // case["groups"] * geometry[0] * geometry[1] % 4 == 0), case


def test_conv2d_table_reaches_every_flag():
    assert {(c["hw4"], c["k4"]) for c in T.CONV2D} == {(a, b) for a in (True, False) for b in (True, False)}
    assert any(c["groups"] > 1 for c in T.CONV2D) and any(c["shape"][0] > 1 for c in T.CONV2D)


@pytest.mark.parametrize("case", T.DEFORM, ids=lambda c: "-".join(map(str, c["shape"])))
def test_deform_plans(case):
    lib = _lib.load()
    n, cin, cout, h, w = case["shape"]
    geometry, oh, ow = _geometry(case)
    assert lib.mv_deform_conv2d_needs_workspace(n, cin, cout, h, w, *geometry, case["groups"], case["og"]) == case["needs"], case
    assert int(lib.mv_deform_conv2d_workspace_bytes(n, cin, h, w, *geometry)) == 4 * n * cin * geometry[0] * geometry[1] * oh * ow
    assert case["ow4"] == (ow % 4 == 0), case
    # the columns form's gather: k_deform_im2col_lds while its window of 8 channels fits 64 KiB (deform.hip), else k_deform_im2col
    win_h = 7 * geometry[2] + (geometry[0] - 1) * geometry[6] + 14
    win_w = 31 * geometry[3] + (geometry[1] - 1) * geometry[7] + 14
    assert (4 * 8 * win_h * (win_w | 1) > 64 * 1024) == ("k_deform_im2col" in case["why"]), case


def test_deform_table_reaches_every_form():
    fused = [c for c in T.DEFORM if c["needs"] == 2]
    assert {c["ow4"] for c in fused} == {True, False}
    assert {c["mask"] for c in T.DEFORM} == {True, False} and {c["og"] for c in T.DEFORM} >= {1, 2}
    assert any(c["far"] for c in T.DEFORM) and any(c["needs"] == 1 for c in T.DEFORM)
    assert any(c["shape"][0] > 1 for c in T.DEFORM)  # one image's workspace = several passes
    assert any("k_deform_im2col" in c["why"] for c in T.DEFORM)


@pytest.mark.parametrize("case", T.INVRES, ids=lambda c: "-".join(map(str, c["block"])))
def test_inverted_residual_plans(case):
    lib = _lib.load()
    cin, hidden, cout, side, stride = case["block"]
    ow = (side - 1) // stride + 1
    for n, (slices, slice_len, workspace) in case["plans"].items():
        sl = C.c_int(0)
        got = lib.mv_inverted_residual_k_slices(n, cin, hidden, cout, side, side, stride, C.byref(sl))
        assert (got, sl.value, int(lib.mv_inverted_residual_workspace_bytes(n, cin, hidden, cout, side, side, stride))) == (slices, slice_len, workspace), (case, n)
        assert workspace == (4 * slices * n * cout * ow * ow if slices > 1 else 0)


def test_inverted_residual_table_reaches_every_form():
    blocks = {c["block"] for c in T.INVRES}
    assert blocks >= {(160, 960, 160, 7, 1), (64, 384, 64, 14, 1), (96, 576, 160, 14, 2), (32, 192, 32, 28, 1), (32, 192, 64, 28, 2)}
    assert (24, 72, 20, 56, 1) in blocks and (32, 32, 16, 112, 1) in blocks
    seven = next(c for c in T.INVRES if c["block"][3] == 7)
    assert set(seven["plans"]) >= {1, 2, 3}  # two images per region: whole regions, and one left with a single image
    for kind in ("k_invres<", "k_invres_wide<"):
        plans = [p for c in T.INVRES if c["kernel"].startswith(kind) for p in c["plans"].values()]
        assert any(s == 1 for s, _, _ in plans) and any(s > 1 for s, _, _ in plans), kind
    totals = [n * c["block"][2] * ((c["block"][3] - 1) // c["block"][4] + 1) ** 2 for c in T.INVRES for n, p in c["plans"].items() if p[0] > 1]
    assert min(totals) == 160 * 49  # k_invres_reduce's smallest total: one image of the 7 x 7 stage


def test_inverted_residual_refusal_case_plan():
    lib = _lib.load()
    case = T.INVRES_REFUSAL
    n, cin, hidden, cout, h, w, stride = case["shape"]
    sl = C.c_int(0)
    slices = lib.mv_inverted_residual_k_slices(n, cin, hidden, cout, h, w, stride, C.byref(sl))
    ws = int(lib.mv_inverted_residual_workspace_bytes(n, cin, hidden, cout, h, w, stride))
    assert (slices, sl.value, ws) == (case["slices"], case["slice_len"], case["workspace"])
    assert ws == 4 * slices * n * cout * ((h - 1) // stride + 1) * ((w - 1) // stride + 1)
