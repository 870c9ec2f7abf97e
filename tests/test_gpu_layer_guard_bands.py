"""Guard-band sweeps of the CNN layer kernels at the C ABI (`-m gpu`), in the style of tests/test_gpu_filter_guard_bands.py:
mv_conv3x3_bias_relu_f32 / _ws_f32 / _u8norm_f32 (k_conv3x3_gen in its three wave tiles, dense and first small-launch forms,
loader waves on and off, stacked images, K slices + k_conv3x3_reduce; k_conv3x3; k_conv3x3_c3), mv_linear_bias_relu_f32 / _ws_f32
(k_linear, k_linear_gemv, k_linear_reduce), the pools, mv_conv_norm_act_f32 (k_conv3x3_smallcin, k_dwpc3x3, k_dwpc3x3_small,
k_conv1x1 with and without K slices), mv_conv2d_bias_act_f32 (k_conv_igemm's implicit form; with the optional small-launch
workspace k_deform_im2col's plain im2col + k_conv1x1), mv_deform_conv2d_f32 (k_deform_fused; with a workspace of one image or of
the batch k_deform_im2col_lds / k_deform_im2col + k_conv1x1; mask, offset groups, offsets far outside the image) and
mv_inverted_residual_f32 (k_invres at 7 / 14 / 28 pixels, k_invres_wide at 56 and 112, with and without the workspace and
k_invres_reduce; its alignment refusals).  The value tests of this family
(test_gpu_cnn.py, test_gpu_mobilenet.py, test_gpu_deform.py) go through the Python layer, which hands every kernel fresh 256-byte aligned tensors:
the launchers' pointer tests (vec_w / vec_x / vec_y, vec_rows, `aligned`, `vec`) then always answer "aligned".  Here every tensor
lies inside a sentinel-filled buffer (tests/_guard.py), one tensor at a time at an odd element offset and once all of them, at
the shapes of tests/_layer_guard_cases.py (whose plans tests/test_layer_guard_cases_host.py checks without a GPU).  Every case
asserts that

  1. the result equals the reference its value test uses (oracle/ref.py), bit for bit (G.assert_same);
  2. nothing outside y changed (y starts filled with the sentinel, so equality also proves it was written whole);
  3. every input buffer -- x, weights, bias, alpha, beta, residual; NaN guards for floats, 0 / 255 around pixels from [40, 200] for
     the uint8 image -- is bit-unchanged, guards included: a value read from past a tensor's end shows in the output even
     through a zero weight;
  4. a workspace is allocated with exactly the bytes the query returns, keeps its guards, and runs on 0xFF and on 0x00 garbage
     give the same bits.

Combinations an entry point refuses by contract are called as well: the documented status, and nothing written.  Each test
collects mv_last_kernel() and asserts which kernels ran at aligned and at odd offsets, or were rerouted where that is the
contract (k_conv3x3_c3 needs a 16-byte y, k_dwpc3x3_small a 16-byte x, k_linear_gemv 16-byte x and w; the fused block refuses
an under-aligned x, y, w_expand, w_project or workspace, so its value cases move w_dw and the six norm vectors only).  The
columns forms end in k_conv1x1, which is what mv_last_kernel() then names: which gather kernel fed it follows from the geometry
(tests/test_layer_guard_cases_host.py restates deform.hip's LDS-window bound for every row)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _guard as G, _layer_guard_cases as T  # noqa: E402
from tests._util import philox_f32, philox_u8  # noqa: E402
from tests.test_gpu_filter_guard_bands import _Seen  # noqa: E402
from tests.test_gpu_guard_bands import _in_guard, _stream  # noqa: E402

DEV = "cuda"
A = G.ALIGNED
F32, U8 = torch.float32, torch.uint8
INVALID, UNSUPPORTED = -1, -2  # MV_ERR_INVALID_ARGUMENT, MV_ERR_UNSUPPORTED
ACT_CODES = {None: 0, "relu": 1, "relu6": 2, "hardswish": 3}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _offset_sets(names, odd=(1, 3, 5, 7, 9, 11, 13)):
    """{name: element offset} dicts: every tensor 16-byte aligned, each of `names` at an odd element alone, all of them odd."""
    sets = [{n: A for n in names}]
    for i, n in enumerate(names):
        sets.append({m: (odd[i % len(odd)] if m == n else A) for m in names})
    sets.append({n: odd[i % len(odd)] for i, n in enumerate(names)})
    return sets


def _all_aligned(offs):
    return all(o == A for o in offs.values())


def _run(what, call, inputs, offs, y_shape, want, ws_bytes=0, ws_offset=0):
    """One case.  inputs: {name: host tensor or None}; offs: {name: element offset} for the inputs and "y".
    call(ptrs: {name: device pointer or None}, y_ptr, ws_ptr, ws_bytes) -> status.  The four assertions of the module docstring;
    with a workspace (ws_offset bytes past a 256-byte boundary) the call runs twice, on 0xFF and on 0x00 garbage.
    -> the last launched kernel's label."""
    bufs = {n: G.guarded(v, v.dtype, DEV, offs.get(n, A), sentinel=_in_guard(v.dtype)) for n, v in inputs.items() if v is not None}
    before = {n: b.cpu() for n, (b, _) in bufs.items()}
    ptrs = {n: (bufs[n][1].data_ptr() if n in bufs else None) for n in inputs}
    ybuf, yv = G.guarded(y_shape, F32, DEV, offs["y"])
    results = []
    for garbage in ((0xFF, 0x00) if ws_bytes else (None,)):
        tag = what if garbage is None else f"{what} workspace={garbage:#04x}"
        if results:
            yv.fill_(G.sentinel_for(F32))
        wbuf, ws = G.guarded_workspace(ws_bytes, DEV, garbage, offset_bytes=ws_offset)
        _lib.check(call(ptrs, yv.data_ptr(), None if ws is None else ws.data_ptr(), ws_bytes))
        torch.cuda.synchronize()
        kernel = _lib.last_kernel()
        tag = f"{tag} [{kernel}]"
        G.assert_guards_intact(ybuf, yv, what=tag + ": output")
        G.assert_same(yv, want, tag)
        for n, (b, _) in bufs.items():
            G.assert_unchanged(b, before[n], f"{tag}: input {n}")
        if wbuf is not None:
            G.assert_guards_intact(wbuf, ws, what=tag + ": workspace")
        results.append(yv.cpu())
    if len(results) == 2:
        G.assert_unchanged(results[1], results[0], what + ": the result depends on the workspace's content")
    return kernel


def _refused(what, call, inputs, offs, y_shape, status, ws_bytes=0, ws_offset=0, ws_null=False, message=None):
    """The entry point refuses the call: the documented status (and message), no byte of y or of the workspace written."""
    bufs = {n: G.guarded(v, v.dtype, DEV, offs.get(n, A), sentinel=_in_guard(v.dtype)) for n, v in inputs.items() if v is not None}
    ptrs = {n: (bufs[n][1].data_ptr() if n in bufs else None) for n in inputs}
    ybuf, yv = G.guarded(y_shape, F32, DEV, offs["y"])
    ybefore = ybuf.cpu()
    wbuf, ws = G.guarded_workspace(ws_bytes, DEV, 0xFF, offset_bytes=ws_offset)
    wbefore = None if wbuf is None else wbuf.cpu()
    rc = call(ptrs, yv.data_ptr(), None if (ws is None or ws_null) else ws.data_ptr(), ws_bytes)
    torch.cuda.synchronize()
    error = _lib.load().mv_last_error().decode()
    assert rc == status, (what, rc, error)
    if message is not None:
        assert message in error, (what, error)
    G.assert_unchanged(ybuf, ybefore, what + ": output of a refused call")
    if wbuf is not None:
        G.assert_unchanged(wbuf, wbefore, what + ": workspace of a refused call")


# ---- mv_conv3x3_bias_relu_f32 / _ws_f32 -------------------------------------------------------------------------------------------
def _conv3x3_data(shape):
    n, cin, cout, h, w = shape
    x = philox_f32(9000 + cin + h, (n, cin, h, w)) - 0.5
    wt = (philox_f32(9001 + cout, (cout, cin, 3, 3)) - 0.5) * 0.4
    b = philox_f32(9002 + w, (cout,)) - 0.5
    return x, wt, b


def _conv3x3_expected(case, offs):
    """The kernel the offsets decide: k_conv3x3_c3 needs a 16-byte y (conv3x3_c3_supported), else k_conv3x3_gen serves cin = 3."""
    if case["kernel"] == "k_conv3x3_c3" and offs["y"] != A:
        return "k_conv3x3_gen"
    return case["kernel"]


def _conv3x3_sweep(cases, seen):
    lib = _lib.load()
    for case in cases:
        n, cin, cout, h, w = case["shape"]
        x, wt, b = _conv3x3_data(case["shape"])
        sc = C.c_int(0)
        slices = lib.mv_conv3x3_k_slices(n, cin, h, w, cout, C.byref(sc))
        ws_bytes = int(lib.mv_conv3x3_workspace_bytes(n, cin, h, w, cout))
        assert (slices, sc.value) == (case["slices"], case["slice_channels"]), case
        sl = sc.value if slices > 1 else 0
        wants = {(True, 1): _t(ref.conv3x3_bias_relu(x, wt, b, relu=True, slice_channels=sl)),
                 (False, 0): _t(ref.conv3x3_bias_relu(x, wt, None, relu=False, slice_channels=sl))}
        sets = _offset_sets(["x", "w", "b", "y"])
        for i, offs in enumerate(sets):
            for bias, relu in ([(True, 1), (False, 0)] if i in (0, len(sets) - 1) else [(True, 1)]):
                def call(p, y, ws, nb, relu=relu):
                    if ws_bytes:
                        return lib.mv_conv3x3_bias_relu_ws_f32(p["x"], p["w"], p["b"], y, n, cin, h, w, cout, relu, ws, nb, _stream())
                    return lib.mv_conv3x3_bias_relu_f32(p["x"], p["w"], p["b"], y, n, cin, h, w, cout, relu, _stream())
                what = f"conv3x3 {case['shape']} {case['env']} bias={bias} relu={relu} offsets={offs}"
                kernel = _run(what, call, {"x": _t(x), "w": _t(wt), "b": _t(b) if bias else None}, offs, (n, cout, h, w), wants[(bias, relu)],
                              ws_bytes=ws_bytes)
                expected = _conv3x3_expected(case, offs)
                if expected == "k_conv3x3":
                    assert kernel.startswith("k_conv3x3<"), (what, kernel)  # k_conv3x3<ks0>, <ks5>, <ks14[,fullw]>: not _gen, not _c3
                else:
                    assert expected in kernel, (what, kernel)
                seen.note(kernel, _all_aligned(offs))
        if ws_bytes:  # the workspace entry: four bytes short, and no workspace at all
            inputs = {"x": _t(x), "w": _t(wt), "b": _t(b)}
            al = sets[0]
            _refused(f"conv3x3 {case['shape']} workspace of need - 4 bytes",
                     lambda p, y, ws, nb: lib.mv_conv3x3_bias_relu_ws_f32(p["x"], p["w"], p["b"], y, n, cin, h, w, cout, 1, ws, nb - 4, _stream()),
                     inputs, al, (n, cout, h, w), INVALID, ws_bytes=ws_bytes, message="workspace")
            _refused(f"conv3x3 {case['shape']} null workspace",
                     lambda p, y, ws, nb: lib.mv_conv3x3_bias_relu_ws_f32(p["x"], p["w"], p["b"], y, n, cin, h, w, cout, 1, ws, nb, _stream()),
                     inputs, al, (n, cout, h, w), INVALID, ws_bytes=ws_bytes, ws_null=True, message="workspace")


def test_conv3x3():
    seen = _Seen()
    _conv3x3_sweep([c for c in T.CONV3X3 if not c["env"]], seen)
    seen.report("mv_conv3x3_bias_relu_f32 / _ws_f32")
    seen.require("k_conv3x3_gen")
    seen.require("k_conv3x3_reduce<ks2>")
    seen.require("k_conv3x3_reduce<ks4>")
    seen.require("k_conv3x3_c3", aligned=(True,))
    assert any(k == "k_conv3x3_c3" for k in seen.labels[False])  # x, w or b odd: still the first-layer kernel
    for al in (True, False):
        assert any(k.startswith("k_conv3x3<") for k in seen.labels[al]), seen.labels


_ENVS = sorted({tuple(sorted(c["env"].items())) for c in T.CONV3X3 if c["env"]})


@pytest.mark.parametrize("env", _ENVS, ids=lambda e: ",".join(f"{k[8:]}={v}" for k, v in e))
def test_conv3x3_forced_forms(env, monkeypatch, tuning_library):
    """k_conv3x3_gen's wave tiles (MV_CONV_SHAPE 0 / 1 / 2 = 4x2 / 2x1 / 1x1), loader waves (MV_CONV_SPEC42), the dense loop
    (MV_CONV_DENSE) and image stacking with a group that does not divide the batch (MV_CONV_GROUP), in the tuning build."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    seen = _Seen()
    _conv3x3_sweep([c for c in T.CONV3X3 if tuple(sorted(c["env"].items())) == env], seen)
    seen.report(f"mv_conv3x3_bias_relu_f32 {dict(env)}")
    seen.require("k_conv3x3_gen")


# ---- mv_conv3x3_bias_relu_u8norm_f32 ------------------------------------------------------------------------------------------------
def test_conv3x3_u8norm():
    lib = _lib.load()
    fn = lib.mv_conv3x3_bias_relu_u8norm_f32
    mm, ss = [0.4, 0.5, 0.3], [0.2, 0.25, 0.3]
    mean, std = _lib.taps(mm), _lib.taps(ss)
    seen = _Seen()

    def data(n, cout, h, w):
        x = (philox_u8(9100 + w, (n, 3, h, w)) % 161 + 40).astype(np.uint8)  # [40, 200] between 0 / 255 guards
        wt = (philox_f32(9101 + cout, (cout, 3, 3, 3)) - 0.5) * 0.4
        b = philox_f32(9102 + h, (cout,)) - 0.5
        return x, wt, b

    for n, cout, h, w in T.CONV3X3_U8NORM:
        x, wt, b = data(n, cout, h, w)
        want = _t(ref.conv3x3_bias_relu(ref.to_float_normalize(x, mm, ss), wt, b))
        call = lambda p, y, ws, nb: fn(p["x"], mean, std, p["w"], p["b"], y, n, h, w, cout, 1, _stream())  # noqa: E731
        inputs = {"x": _t(x), "w": _t(wt), "b": _t(b)}
        for offs in ({"x": A, "w": A, "b": A, "y": A}, {"x": 1, "w": A, "b": A, "y": A}, {"x": 3, "w": A, "b": A, "y": A},
                     {"x": 4, "w": A, "b": A, "y": A}, {"x": A, "w": 1, "b": A, "y": A}, {"x": A, "w": A, "b": 3, "y": A},
                     {"x": 37, "w": 5, "b": 7, "y": A}):
            what = f"conv3x3_u8norm {(n, cout, h, w)} offsets={offs}"
            kernel = _run(what, call, inputs, offs, (n, cout, h, w), want)
            assert kernel == "k_conv3x3_c3", (what, kernel)
            seen.note(kernel, _all_aligned(offs))
        _refused(f"conv3x3_u8norm {(n, cout, h, w)} y odd", call, inputs, {"x": A, "w": A, "b": A, "y": 3}, (n, cout, h, w), UNSUPPORTED,
                 message="16-byte aligned output")
    n, cout, h, w = T.CONV3X3_U8NORM_REFUSED_WIDTH
    x, wt, b = data(n, cout, h, w)
    _refused(f"conv3x3_u8norm {(n, cout, h, w)} W % 4 != 0", lambda p, y, ws, nb: fn(p["x"], mean, std, p["w"], p["b"], y, n, h, w, cout, 1, _stream()),
             {"x": _t(x), "w": _t(wt), "b": _t(b)}, {"y": A}, (n, cout, h, w), UNSUPPORTED, message="W % 4 == 0")
    seen.report("mv_conv3x3_bias_relu_u8norm_f32")
    seen.require("k_conv3x3_c3")


# ---- mv_linear_bias_relu_f32 / _ws_f32 ----------------------------------------------------------------------------------------------
def test_linear():
    lib = _lib.load()
    seen = _Seen()
    refused = 0
    for case in T.LINEAR:
        n, k, m = case["shape"]
        x = philox_f32(9200 + k, (n, k)) - 0.5
        wt = (philox_f32(9201 + m, (m, k)) - 0.5) * 0.2
        b = philox_f32(9202 + n, (m,)) - 0.5
        sl = C.c_int(0)
        slices = lib.mv_linear_k_slices(n, k, m, C.byref(sl))
        ws_bytes = int(lib.mv_linear_workspace_bytes(n, k, m))
        assert (slices, sl.value, ws_bytes) == (case["slices"], case["slice_len"], case["workspace"]), case
        slen = sl.value if slices > 1 else 0
        wants = {(True, 1): _t(ref.linear_bias_relu(x, wt, b, relu=True, slice_len=slen)),
                 (False, 0): _t(ref.linear_bias_relu(x, wt, None, relu=False, slice_len=slen))}
        inputs = {"x": _t(x), "w": _t(wt), "b": _t(b)}
        sets = [(o, 0) for o in _offset_sets(["x", "w", "b", "y"])]
        if ws_bytes:  # a workspace that is 4-byte but not 16-byte aligned is accepted: vec_y falls back
            sets += [(sets[0][0], 4), (sets[-1][0], 12)]
        for i, (offs, ws_off) in enumerate(sets):
            for bias, relu in ([(True, 1), (False, 0)] if i in (0, len(sets) - 1) else [(True, 1)]):
                def call(p, y, ws, nb, relu=relu, bias=bias):
                    return lib.mv_linear_bias_relu_ws_f32(p["x"], p["w"], p["b"] if bias else None, y, n, k, m, relu, ws, nb, _stream())
                what = f"linear {case['shape']} bias={bias} relu={relu} offsets={offs} workspace_offset={ws_off}"
                kernel = _run(what, call, inputs, offs, (n, m), wants[(bias, relu)], ws_bytes=ws_bytes, ws_offset=ws_off)
                gemv = case["kernel"] == "k_linear_gemv" and offs["x"] == A and offs["w"] == A
                assert kernel == ("k_linear_gemv" if gemv else "k_linear" if not ws_bytes else "k_linear_reduce"), (what, kernel)
                seen.note(kernel, _all_aligned(offs) and ws_off == 0)
        if not ws_bytes:  # the plain entry point is the same launch
            kernel = _run(f"linear {case['shape']} plain entry", lambda p, y, ws, nb: lib.mv_linear_bias_relu_f32(p["x"], p["w"], p["b"], y, n, k, m, 1, _stream()),
                          inputs, sets[-1][0], (n, m), wants[(True, 1)])
            assert kernel == "k_linear", kernel
        else:
            call = lambda p, y, ws, nb: lib.mv_linear_bias_relu_ws_f32(p["x"], p["w"], p["b"], y, n, k, m, 1, ws, nb, _stream())  # noqa: E731
            _refused(f"linear {case['shape']} workspace at 2 mod 4", call, inputs, sets[0][0], (n, m), INVALID, ws_bytes=ws_bytes, ws_offset=2,
                     message="4-byte aligned")
            _refused(f"linear {case['shape']} null workspace", call, inputs, sets[0][0], (n, m), INVALID, ws_bytes=ws_bytes, ws_null=True,
                     message="workspace")
            refused += 2
    seen.report("mv_linear_bias_relu_ws_f32")
    assert refused
    seen.require("k_linear_reduce")
    seen.require("k_linear_gemv", aligned=(True,))
    assert "k_linear_gemv" in seen.labels[False]  # b or y odd: x and w alone decide (asserted case by case above)
    for al in (True, False):
        assert "k_linear" in seen.labels[al], seen.labels


# ---- the pools ------------------------------------------------------------------------------------------------------------------------
def _xy_sets():
    return [{"x": A, "y": A}, {"x": 1, "y": A}, {"x": A, "y": 3}, {"x": 1, "y": 3}]


def test_maxpool2x2():
    lib = _lib.load()
    seen = _Seen()
    for planes, h, w in T.MAXPOOL2X2:
        x = philox_f32(9300 + w, (planes, h, w)) - 0.5
        if h >= 2 and w >= 2:
            x[0, 0, 1] = np.nan
        want = _t(ref.maxpool2x2(x))
        for offs in _xy_sets():
            what = f"maxpool2x2 {(planes, h, w)} offsets={offs}"
            call = lambda p, y, ws, nb: lib.mv_maxpool2x2_f32(p["x"], y, planes, h, w, _stream())  # noqa: E731
            if want.numel() == 0:  # h or w below 2: nothing to write, nothing launched (y: one element that must stay)
                _refused(what, call, {"x": _t(x)}, offs, (1,), 0)
                continue
            kernel = _run(what, call, {"x": _t(x)}, offs, want.shape, want)
            assert kernel == "k_maxpool2x2", (what, kernel)
            seen.note(kernel, _all_aligned(offs))
    seen.report("mv_maxpool2x2_f32")
    seen.require("k_maxpool2x2")


def test_maxpool2d():
    lib = _lib.load()
    seen = _Seen()
    for planes, h, w, k, s in T.MAXPOOL2D:
        x = philox_f32(9400 + w, (planes, h, w)) - 0.5
        x[0, 0, 0] = np.nan
        want = _t(ref.maxpool2d(x, k, s))
        for offs in _xy_sets():
            what = f"maxpool2d {(planes, h, w, k, s)} offsets={offs}"
            kernel = _run(what, lambda p, y, ws, nb: lib.mv_maxpool2d_f32(p["x"], y, planes, h, w, k, s, _stream()), {"x": _t(x)}, offs,
                          want.shape, want)
            assert kernel == "k_maxpool2d", (what, kernel)
            seen.note(kernel, _all_aligned(offs))
    seen.report("mv_maxpool2d_f32")
    seen.require("k_maxpool2d")


def test_adaptive_avgpool():
    lib = _lib.load()
    seen = _Seen()
    for (planes, h, w, oh, ow), expected in T.AVGPOOL:
        x = philox_f32(9500 + h * w + planes, (planes, h, w)) * 2 - 1
        want = _t(ref.adaptive_avgpool(x, oh, ow))
        for offs in _xy_sets():
            what = f"adaptive_avgpool {(planes, h, w, oh, ow)} offsets={offs}"
            kernel = _run(what, lambda p, y, ws, nb: lib.mv_adaptive_avgpool_f32(p["x"], y, planes, h, w, oh, ow, _stream()), {"x": _t(x)}, offs,
                          want.shape, want)
            assert kernel == expected, (what, kernel)
            seen.note(kernel, _all_aligned(offs))
    seen.report("mv_adaptive_avgpool_f32")
    seen.require("k_global_avgpool_small")
    seen.require("k_adaptive_avgpool")


# ---- mv_conv_norm_act_f32 -------------------------------------------------------------------------------------------------------------
DENSE3X3, DW3X3, PW1X1 = 0, 1, 2
# (bias, affine, act, residual): the activations none, ReLU, ReLU6 and Hardswish, both folded-norm forms
EPILOGUES = [(False, 2, "relu6", False), (True, 1, None, True), (False, 0, "relu", False), (True, 2, "hardswish", True)]


@functools.lru_cache(maxsize=None)
def _cna_data(kind, shape_x, w_seed, cout, stride, epilogue, seed, slice_len):
    """Inputs and reference of one conv_norm_act case, computed once and shared by every offset set (never modified)."""
    n, cin, h, w = shape_x
    bias, affine, act, residual = epilogue
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    w_shape = {DENSE3X3: (cout, cin, 3, 3), DW3X3: (cout, 1, 3, 3), PW1X1: (cout, cin, 1, 1)}[kind]
    wt = (philox_f32(w_seed, w_shape) - 0.5) * 0.4
    x = philox_f32(seed, shape_x) - 0.5
    b = (philox_f32(seed + 1, (cout,)) - 0.5) if bias else None
    alpha = (philox_f32(seed + 2, (cout,)) + 0.5) if affine else None
    beta = (philox_f32(seed + 3, (cout,)) - 0.5) if affine else None
    res = (philox_f32(seed + 4, (n, cout, oh, ow)) - 0.5) if residual else None
    pad, groups = (0, 1) if kind == PW1X1 else (1, cin if kind == DW3X3 else 1)
    want = _t(ref.conv2d_affine_act(x, wt, b, alpha, beta, res, stride, pad, groups, affine, act, slice_len=slice_len))
    opt = lambda a: None if a is None else _t(a)  # noqa: E731
    return {"x": _t(x), "w": _t(wt), "bias": opt(b), "alpha": opt(alpha), "beta": opt(beta), "residual": opt(res)}, want


def _cna_case(seen, kind, shape_x, w_seed, cout, stride, epilogue, offs, seed, slice_len=0, expected=None):
    lib = _lib.load()
    n, cin, h, w = shape_x
    _, affine, act, _ = epilogue
    inputs, want = _cna_data(kind, shape_x, w_seed, cout, stride, epilogue, seed, slice_len)
    what = f"conv_norm_act kind={kind} x={shape_x} cout={cout} stride={stride} epilogue={epilogue} offsets={offs}"
    kernel = _run(what, lambda p, y, ws, nb: lib.mv_conv_norm_act_f32(kind, p["x"], p["w"], p["bias"], p["alpha"], p["beta"], p["residual"], y, n, cin,
                                                                     h, w, cout, stride, affine, ACT_CODES[act], _stream()),
                  inputs, offs, tuple(want.shape), want)
    if expected is not None:
        assert kernel == (expected(offs) if callable(expected) else expected), (what, kernel)
    seen.note(kernel, _all_aligned(offs))
    return kernel


CNA_NAMES = ["x", "w", "bias", "alpha", "beta", "residual", "y"]


def test_conv_norm_act_stem():
    seen = _Seen()
    for i, (n, cin, cout, h, w, stride) in enumerate(T.STEM):
        for j, offs in enumerate(_offset_sets(CNA_NAMES)):
            _cna_case(seen, DENSE3X3, (n, cin, h, w), 9600 + cout, cout, stride, EPILOGUES[(i + j) % 4 | 1], offs, 9610 + h, expected="k_conv3x3_smallcin")
            if j in (0, len(CNA_NAMES) + 1):
                _cna_case(seen, DENSE3X3, (n, cin, h, w), 9600 + cout, cout, stride, EPILOGUES[(i + j) % 4 & 2], offs, 9610 + h, expected="k_conv3x3_smallcin")
    seen.report("mv_conv_norm_act_f32 dense 3x3")
    seen.require("k_conv3x3_smallcin")


def test_conv_norm_act_depthwise():
    seen = _Seen()
    for i, ((n, c, h, w, stride), kernel_aligned, _) in enumerate(T.DEPTHWISE):
        # k_dwpc3x3_small streams whole planes with 16-byte loads: launch_dwpc3x3 takes it on a 16-byte x only
        expected = lambda offs, k=kernel_aligned: k if offs["x"] == A else "k_dwpc3x3"  # noqa: E731
        for j, offs in enumerate(_offset_sets(CNA_NAMES)):
            _cna_case(seen, DW3X3, (n, c, h, w), 9700 + c, c, stride, EPILOGUES[(i + j) % 4 | 1], offs, 9710 + h + w, expected=expected)
            if j in (0, len(CNA_NAMES) + 1):
                _cna_case(seen, DW3X3, (n, c, h, w), 9700 + c, c, stride, EPILOGUES[(i + j) % 4 & 2], offs, 9710 + h + w, expected=expected)
    seen.report("mv_conv_norm_act_f32 depthwise")
    seen.require("k_dwpc3x3")
    for size in ("<7,s1>", "<7,s2>", "<14,s2>", "<28,s1>"):
        seen.require("k_dwpc3x3_small" + size, aligned=(True,))
        assert "k_dwpc3x3_small" + size in seen.labels[False]  # w, y, residual or a norm vector odd: still the LDS kernel
    for k in seen.labels[False]:
        assert k == "k_dwpc3x3" or k.startswith("k_dwpc3x3_small"), k


def test_conv_norm_act_pointwise():
    lib = _lib.load()
    seen = _Seen()
    for i, case in enumerate(T.POINTWISE):
        n, cin, cout, h, w = case["shape"]
        sl = C.c_int(0)
        slices = lib.mv_conv1x1_k_slices(n, cin, h, w, cout, C.byref(sl))
        assert (slices, sl.value) == (case["slices"], case["slice_len"]), case
        head = "k_conv1x1<1," if slices > 1 else "k_conv1x1<"
        for j, offs in enumerate(_offset_sets(CNA_NAMES)):
            for ep in ([EPILOGUES[(i + j) % 4 | 1], EPILOGUES[(i + j) % 4 & 2]] if j in (0, len(CNA_NAMES) + 1) else [EPILOGUES[(i + j) % 4 | 1]]):
                kernel = _cna_case(seen, PW1X1, (n, cin, h, w), 9800 + cout, cout, 1, ep, offs, 9810 + cin, slice_len=sl.value if slices > 1 else 0)
                assert kernel.startswith(head) and (f",ks{slices}>" in kernel) == (slices > 1), (case, offs, kernel)
    seen.report("mv_conv_norm_act_f32 pointwise")
    seen.require("k_conv1x1<")
    seen.require("k_conv1x1<1,", ",ks2>")
    seen.require("k_conv1x1<1,", ",ks4>")


# ---- mv_conv2d_bias_act_f32 -----------------------------------------------------------------------------------------------------------
def _out_hw(h, w, k, stride, pad, dil):
    return ((h + 2 * pad[0] - (dil[0] * (k[0] - 1) + 1)) // stride[0] + 1, (w + 2 * pad[1] - (dil[1] * (k[1] - 1) + 1)) // stride[1] + 1)


def _ws_plans(lib, n, cin, h, w, k, stride, pad, dil):
    """(workspace bytes, offset of the workspace in bytes past a 256-byte boundary): none; one image's columns; the whole batch's;
    and the batch's at 4-byte but not 16-byte alignment (the GEMM's vec_x must fall back)."""
    size = lambda images: int(lib.mv_deform_conv2d_workspace_bytes(images, cin, h, w, k[0], k[1], stride[0], stride[1], pad[0], pad[1], dil[0], dil[1]))  # noqa: E731
    return [(0, 0), (size(1), 0), (size(n), 0), (size(n), 4)]


def test_conv2d():
    """k_conv_igemm's implicit form without a workspace; with the optional small-launch workspace, sized exactly for one image
    and for the batch, plain im2col (k_deform_im2col) + k_conv1x1.  Reference: what test_gpu_cnn.py's value test asserts, the
    oracle's deform_conv2d with zero offsets, then the activation -- bit for bit."""
    lib = _lib.load()
    seen = {False: _Seen(), True: _Seen()}  # without / with a workspace
    for case in T.CONV2D:
        n, cin, cout, h, w = case["shape"]
        k, stride, pad, dil, groups = case["k"], case["stride"], case["pad"], case["dil"], case["groups"]
        geometry = (k[0], k[1], stride[0], stride[1], pad[0], pad[1], dil[0], dil[1])
        assert lib.mv_conv2d_needs_workspace(n, cin, cout, h, w, *geometry, groups) == 2, case
        oh, ow = _out_hw(h, w, k, stride, pad, dil)
        x = philox_f32(10000 + cin + h, (n, cin, h, w)) * 2 - 1
        wt = (philox_f32(10001 + cout, (cout, cin // groups, k[0], k[1])) - 0.5) * 0.5
        b = philox_f32(10002 + w, (cout,)) - 0.5
        zero_off = np.zeros((n, 2 * k[0] * k[1], oh, ow), np.float32)
        wants = {(True, 1): _t(np.maximum(ref.deform_conv2d(x, zero_off, wt, b, stride, pad, dil, None), 0)),
                 (False, 0): _t(ref.deform_conv2d(x, zero_off, wt, None, stride, pad, dil, None))}
        plans = _ws_plans(lib, n, cin, h, w, k, stride, pad, dil)
        sets = _offset_sets(["x", "w", "b", "y"])
        for i, offs in enumerate(sets):
            for ws_bytes, ws_off in (plans if i in (0, len(sets) - 1) else (plans[0], plans[2])):
                for bias, act in ([(True, 1), (False, 0)] if i == len(sets) - 1 else [(True, 1)]):
                    def call(p, y, ws, nb, act=act):
                        return lib.mv_conv2d_bias_act_f32(p["x"], p["w"], p["b"], y, n, cin, h, w, cout, *geometry, groups, act, ws, nb, _stream())
                    what = f"conv2d {case['shape']} k={k} s={stride} p={pad} d={dil} g={groups} bias={bias} act={act} offsets={offs} workspace={ws_bytes}+{ws_off}"
                    kernel = _run(what, call, {"x": _t(x), "w": _t(wt), "b": _t(b) if bias else None}, offs, (n, cout, oh, ow), wants[(bias, act)],
                                  ws_bytes=ws_bytes, ws_offset=ws_off)
                    if ws_bytes:
                        assert kernel.startswith("k_conv1x1<"), (what, kernel)
                    else:
                        assert kernel.startswith("k_conv_igemm<") and "implicit" in kernel, (what, kernel)
                    seen[bool(ws_bytes)].note(kernel, _all_aligned(offs) and ws_off == 0)
    seen[False].report("mv_conv2d_bias_act_f32 without a workspace")
    seen[True].report("mv_conv2d_bias_act_f32 with the small-launch workspace")
    seen[False].require("k_conv_igemm<")
    seen[True].require("k_conv1x1<")


# ---- mv_deform_conv2d_f32 -------------------------------------------------------------------------------------------------------------
def test_deform_conv2d():
    """k_deform_fused without a workspace; the columns form (k_deform_im2col_lds or k_deform_im2col, then k_conv1x1) with a
    workspace sized exactly for one image (one pass per image) and for the batch.  tests/test_gpu_deform.py asserts bit equality
    with ref.deform_conv2d for both forms (np.testing.assert_array_equal), so does this."""
    from tests.test_gpu_deform import _case as deform_data
    lib = _lib.load()
    seen = {False: _Seen(), True: _Seen()}
    names = ["x", "w", "offset", "mask", "b", "y"]
    for case in T.DEFORM:
        n, cin, cout, h, w = case["shape"]
        k, stride, pad, dil, groups, og = case["k"], case["stride"], case["pad"], case["dil"], case["groups"], case["og"]
        geometry = (k[0], k[1], stride[0], stride[1], pad[0], pad[1], dil[0], dil[1])
        needs = lib.mv_deform_conv2d_needs_workspace(n, cin, cout, h, w, *geometry, groups, og)
        assert needs == case["needs"], (case, needs)
        oh, ow = _out_hw(h, w, k, stride, pad, dil)
        x, off, wt, b, mask = deform_data(10100 + cin * 7 + h, n, cin, cout, h, w, k[0], k[1], stride, pad, dil, groups, og, case["mask"], case["bias"],
                                          scale=case["scale"])
        if case["far"]:  # samples far outside the image, and outside the staged window: the per-sample global path, exactly 0
            off[0, 0, oh // 2, ow // 2], off[0, 1, oh // 2, ow // 2] = 1000.0, -1000.0
            off[n - 1, 2 * k[0] * k[1] * og - 1, oh - 1, ow - 1] = -40.0
        want = _t(ref.deform_conv2d(x, off, wt, b, stride, pad, dil, mask))
        opt = lambda a: None if a is None else _t(a)  # noqa: E731
        inputs = {"x": _t(x), "w": _t(wt), "offset": _t(off), "mask": opt(mask), "b": opt(b)}
        plans = _ws_plans(lib, n, cin, h, w, k, stride, pad, dil)

        def call(p, y, ws, nb):
            return lib.mv_deform_conv2d_f32(p["x"], p["w"], p["offset"], p["mask"], p["b"], y, n, cin, h, w, cout, *geometry, groups, og,
                                            int(case["mask"]), ws, nb, _stream())
        sets = _offset_sets(names)
        for i, offs in enumerate(sets):
            for ws_bytes, ws_off in (plans if i in (0, len(sets) - 1) else (plans[0], plans[2])):
                what = f"deform_conv2d {case['shape']} k={k} s={stride} p={pad} d={dil} g={groups} og={og} offsets={offs} workspace={ws_bytes}+{ws_off}"
                if needs == 1 and not ws_bytes:  # 49 taps have no fused kernel: the documented refusal, nothing written
                    _refused(what, call, inputs, offs, (n, cout, oh, ow), INVALID, message="workspace")
                    continue
                kernel = _run(what, call, inputs, offs, (n, cout, oh, ow), want, ws_bytes=ws_bytes, ws_offset=ws_off)
                assert kernel.startswith("k_conv1x1<" if ws_bytes else "k_deform_fused<"), (what, kernel)
                seen[bool(ws_bytes)].note(kernel, _all_aligned(offs) and ws_off == 0)
    seen[False].report("mv_deform_conv2d_f32 without a workspace")
    seen[True].report("mv_deform_conv2d_f32 with a workspace")
    seen[False].require("k_deform_fused<")
    seen[True].require("k_conv1x1<")


# ---- mv_inverted_residual_f32: values -------------------------------------------------------------------------------------------------
INVRES_NAMES = ["x", "w_expand", "a1", "b1", "w_dw", "a2", "b2", "w_project", "a3", "b3"]


def _invres_call(lib, residual, n, cin, hidden, cout, side, stride):
    return lambda p, y, ws, nb: lib.mv_inverted_residual_f32(p["x"], p["w_expand"], p["a1"], p["b1"], p["w_dw"], p["a2"], p["b2"], p["w_project"],
                                                             p["a3"], p["b3"], residual, y, n, cin, hidden, cout, side, side, stride, 1, ws, nb, _stream())


@pytest.mark.parametrize("case", T.INVRES, ids=lambda c: "-".join(map(str, c["block"])))
def test_inverted_residual(case):
    """The fused block at the C ABI: x, y, w_expand, w_project and the workspace 16-byte aligned as the contract requires, w_dw
    and the six norm vectors aligned, w_dw alone odd, and all seven odd -- the same bits, equal to
    tests/_util.oracle_inverted_residual (FrozenBatchNorm2d's folded norms, MV_AFFINE_MUL_ADD), with the workspace sized exactly."""
    from cpu_vision_amd.mobilenet import FrozenBatchNorm2d, InvertedResidual
    from tests._util import oracle_inverted_residual, randomize_norms
    lib = _lib.load()
    cin, hidden, cout, side, stride = case["block"]
    assert hidden % cin == 0
    torch.manual_seed(cin * 7 + cout)
    layer = InvertedResidual(cin, cout, stride, hidden // cin, norm_layer=FrozenBatchNorm2d).eval()
    randomize_norms(layer, cin + cout + side)
    blocks = list(layer.conv)
    params = {n: None for n in INVRES_NAMES}
    if hidden != cin:
        params["w_expand"] = blocks[0][0].weight.detach().reshape(hidden, cin).clone()
        params["a1"], params["b1"] = (t.clone() for t in blocks[0][1].folded())
    params["w_dw"] = blocks[-3][0].weight.detach().reshape(hidden, 3, 3).clone()
    params["a2"], params["b2"] = (t.clone() for t in blocks[-3][1].folded())
    params["w_project"] = blocks[-2].weight.detach().reshape(cout, hidden).clone()
    params["a3"], params["b3"] = (t.clone() for t in blocks[-1].folded())
    small = ["a1", "b1", "w_dw", "a2", "b2", "a3", "b3"]  # 4-byte alignment is enough for these
    seen = _Seen()
    for n, (slices, slice_len, ws_bytes) in case["plans"].items():
        sl = C.c_int(0)
        assert lib.mv_inverted_residual_k_slices(n, cin, hidden, cout, side, side, stride, C.byref(sl)) == slices and sl.value == slice_len, (case, n)
        assert int(lib.mv_inverted_residual_workspace_bytes(n, cin, hidden, cout, side, side, stride)) == ws_bytes, (case, n)
        x = philox_f32(10200 + n + side, (n, cin, side, side)) * 2 - 1
        want = _t(oracle_inverted_residual(ref, layer, x))
        inputs = dict(params, x=_t(x))
        call = _invres_call(lib, int(layer.use_res_connect), n, cin, hidden, cout, side, stride)
        for offs in ({"y": A}, {"y": A, "w_dw": 1}, dict({"y": A}, **{name: 2 * i + 1 for i, name in enumerate(small)})):
            what = f"inverted_residual {case['block']} batch {n} ({slices} slices) offsets={offs}"
            kernel = _run(what, call, inputs, offs, tuple(want.shape), want, ws_bytes=ws_bytes)
            assert kernel.startswith(case["kernel"]) and kernel.endswith("+k_invres_reduce") == (slices > 1), (what, kernel)
            assert ("(no expansion)" in kernel) == (hidden == cin), (what, kernel)
            seen.note(kernel, len(offs) == 1)
    seen.report(f"mv_inverted_residual_f32 {case['block']}")
    seen.require(case["kernel"])


# ---- mv_inverted_residual_f32: the alignment refusals --------------------------------------------------------------------------------
def test_inverted_residual_refuses_under_aligned_pointers():
    """x, y, w_expand, w_project and the workspace of the fused block must be 16-byte aligned (launch_invres): each of them at an
    odd offset returns MV_ERR_INVALID_ARGUMENT with the documented message, and neither y nor the workspace is written."""
    lib = _lib.load()
    n, cin, hidden, cout, h, w, stride = T.INVRES_REFUSAL["shape"]
    ws_bytes = int(lib.mv_inverted_residual_workspace_bytes(n, cin, hidden, cout, h, w, stride))
    assert ws_bytes == T.INVRES_REFUSAL["workspace"]
    vec = lambda seed, c, lo: _t(philox_f32(seed, (c,)) + lo)  # noqa: E731
    inputs = {"x": _t(philox_f32(9900, (n, cin, h, w)) - 0.5), "w_expand": _t((philox_f32(9901, (hidden, cin)) - 0.5) * 0.3),
              "a1": vec(9902, hidden, 0.5), "b1": vec(9903, hidden, -0.5), "w_dw": _t((philox_f32(9904, (hidden, 3, 3)) - 0.5) * 0.6),
              "a2": vec(9905, hidden, 0.5), "b2": vec(9906, hidden, -0.5), "w_project": _t((philox_f32(9907, (cout, hidden)) - 0.5) * 0.3),
              "a3": vec(9908, cout, 0.5), "b3": vec(9909, cout, -0.5)}
    call = lambda p, y, ws, nb: lib.mv_inverted_residual_f32(p["x"], p["w_expand"], p["a1"], p["b1"], p["w_dw"], p["a2"], p["b2"], p["w_project"],  # noqa: E731
                                                            p["a3"], p["b3"], 1, y, n, cin, hidden, cout, h, w, stride, 2, ws, nb, _stream())
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    for name in ("x", "y", "w_expand", "w_project"):
        offs = {"y": A, name: 1}
        _refused(f"inverted_residual {name} at an odd offset", call, inputs, offs, (n, cout, oh, ow), INVALID, ws_bytes=ws_bytes,
                 message=T.INVRES_MESSAGE)
    for ws_off in (4, 8):
        _refused(f"inverted_residual workspace at {ws_off} mod 16", call, inputs, {"y": A}, (n, cout, oh, ow), INVALID, ws_bytes=ws_bytes,
                 ws_offset=ws_off, message=T.INVRES_MESSAGE)
