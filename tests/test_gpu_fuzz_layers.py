"""Seeded random-shape sweeps of the CNN layer kernels against their references (`-m gpu`): the cases of tests/_fuzz_cases.py --
the depthwise 5x5 conv, the gated pointwise conv, the squeeze-excitation kernels, conv2d_affine_act in both forms, max_pool2d, the two
transposed convs, group_norm_act, l2_normalize_scale, the FPN lateral, interpolate, interpolate_argmax and the gated upsample.

Every comparison is the one the family's own test file makes: bit for bit, NaN in equal places.  Each call's kernel name is
recorded; test_<family>_reaches_every_kernel asserts that the sweep ran every instance the family's own tests name (it runs the
chunks that have not run in this process on the GPU alone).  tests/test_fuzz_cases_host.py shows, without a GPU, that the cases
reach the regimes they are meant to and that the references are right at these shapes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from tests import _fuzz_cases as FC  # noqa: E402
from tests._fuzz_gpu import chunked, dev, kernels_of, same_bits, sweep  # noqa: E402
from tests._mobilenetv3_ref import same  # noqa: E402


def _epilogue_args(d):
    return dev(d["bias"]), dev(d["alpha"]), dev(d["beta"])


# ---- 1. depthwise 5x5 ------------------------------------------------------------------------------------------------------------------
def run_dw5x5(case, d, want):
    g = case.g
    got = F.conv_norm_act(dev(d["x"]), dev(d["w"]), *_epilogue_args(d), dev(d["res"]), stride=g["stride"], groups=g["c"], affine=g["affine"],
                          activation=g["act"], dilation=g["dilation"])
    name = _lib.last_kernel()
    rows = FC.dw5x5_plan(g["n"], g["c"], g["h"], g["w"], g["stride"], g["dilation"])[0]
    assert name == (f"k_dwpc5x5<s1,d2,rows{rows}>" if g["dilation"] == 2 else f"k_dwpc5x5<s{g['stride']},rows{rows}>"), (case.id, name)
    if want is not None:
        same(got, want, case.id)
    return [name]


@chunked("dw5x5")
def test_dw5x5(chunk):
    sweep("dw5x5", chunk, run_dw5x5)


def test_dw5x5_reaches_every_kernel():
    rows = FC.constant("kDw5Rows")
    want = {f"k_dwpc5x5<{inst}rows{r}>" for inst in ("s1,", "s2,", "s1,d2,") for r in (rows, rows // 2)}
    assert kernels_of("dw5x5", run_dw5x5) == want


# ---- 2. pointwise conv with input_scale -----------------------------------------------------------------------------------------------
def run_pw_scaled(case, d, want):
    g = case.g
    xd, wd, gd, rd = dev(d["x"]), dev(d["w"]), dev(d["gate"]), dev(d["res"])
    got = F.conv_norm_act(xd, wd, *_epilogue_args(d), rd, affine=g["affine"], activation=g["act"], input_scale=gd)
    gated = _lib.last_kernel()
    unfused = F.conv_norm_act(F.se_scale(xd, gd), wd, *_epilogue_args(d), rd, affine=g["affine"], activation=g["act"])
    plain = _lib.last_kernel()
    assert gated.startswith("k_conv1x1_sc<") and plain.startswith("k_conv1x1<"), (case.id, gated, plain)
    sliced = F.conv1x1_k_slices(g["n"], g["cin"], g["h"], g["w"], g["cout"])[0] > 1
    assert ("ks" in gated) == ("ks" in plain) == sliced, (case.id, gated, plain)
    assert torch.equal(got, unfused), case.id + ": the fused and the unfused form differ"
    if want is not None:
        same(got, want, case.id)
    return [gated, plain]


@chunked("pw_scaled")
def test_pw_scaled(chunk):
    sweep("pw_scaled", chunk, run_pw_scaled)


def test_pw_scaled_reaches_every_kernel():
    names = kernels_of("pw_scaled", run_pw_scaled)
    for prefix in ("k_conv1x1_sc<", "k_conv1x1<"):
        mine = {n for n in names if n.startswith(prefix)}
        assert any("ks" in n for n in mine) and any("ks" not in n for n in mine), (prefix, names)


# ---- 3. squeeze-excitation kernels ------------------------------------------------------------------------------------------------------
def run_se(case, d, want):
    g = case.g
    xd = dev(d["x"])
    names = []
    pool = F.global_avg_pool(xd)
    names.append(_lib.last_kernel())
    scale = F.se_scale(xd, dev(d["gate"]))
    names.append(_lib.last_kernel())
    assert names[-1] == ("k_se_scale<vec16>" if g["h"] * g["w"] % 4 == 0 else "k_se_scale<scalar>"), (case.id, names[-1])
    linear = F.linear_act(dev(d["xl"]), dev(d["wl"]), dev(d["bl"]), g["act"])
    names.append(_lib.last_kernel())
    gate = F.squeeze_excitation_gate(xd, dev(d["w1"]), dev(d["b1"]), dev(d["w2"]), dev(d["b2"]), g["gate_act"], g["scale_act"])
    names.append(_lib.last_kernel())
    if want is not None:
        for got, key in ((pool, "pool"), (scale, "scale"), (linear, "linear"), (gate, "gate")):
            same(got, want[key], f"{case.id}: {key}")
    return names


@chunked("se")
def test_se(chunk):
    sweep("se", chunk, run_se)


def test_se_reaches_every_kernel():
    assert kernels_of("se", run_se) == {"k_se_pool", "k_linear_act", "k_se_scale<vec16>", "k_se_scale<scalar>"}


# ---- 4. conv2d_affine_act --------------------------------------------------------------------------------------------------------------
def needs_workspace(g):
    return int(_lib.load().mv_conv2d_needs_workspace(g["n"], g["cin"], g["cout"], g["h"], g["w"], g["kh"], g["kw"], g["stride"], g["stride"],
                                                     g["padding"], g["padding"], g["dilation"], g["dilation"], g["groups"]))


def run_conv2d(case, d, want, monkeypatch):
    g = case.g
    monkeypatch.setattr(F, "CONV2D_SMALL_LAUNCH_WORKSPACE", g["columns"])
    got = F.conv2d_affine_act(dev(d["x"]), dev(d["w"]), *_epilogue_args(d), dev(d["res"]), stride=g["stride"], padding=g["padding"],
                              dilation=g["dilation"], groups=g["groups"], affine=g["affine"], activation=g["act"])
    name = _lib.last_kernel()
    need = needs_workspace(g)
    if need == 2:  # the optional workspace: the switch decides the form
        assert name.startswith("k_conv1x1" if g["columns"] else "k_conv_igemm"), (case.id, name)
    if want is not None:
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{case.id} [{name}]")
    return [name]


@chunked("conv2d")
def test_conv2d(chunk, monkeypatch):
    sweep("conv2d", chunk, lambda case, d, want: run_conv2d(case, d, want, monkeypatch))


def test_conv2d_reaches_every_kernel(monkeypatch):
    names = kernels_of("conv2d", lambda case, d, want: run_conv2d(case, d, want, monkeypatch))
    for prefix in ("k_conv_igemm_full<", "k_conv_igemm<", "k_conv1x1"):
        assert any(n.startswith(prefix) for n in names), (prefix, names)


# ---- 5. max_pool2d -----------------------------------------------------------------------------------------------------------------------
def run_maxpool(case, d, want):
    g = case.g
    got = F.max_pool2d(dev(d["x"]), g["k"], g["stride"], g["padding"], ceil_mode=g["ceil_mode"])
    name = _lib.last_kernel()
    if g["ceil_mode"]:
        assert name == "k_maxpool2d_pad<ceil>", (case.id, name)
    elif g["padding"]:
        assert name == "k_maxpool2d_pad", (case.id, name)
    if want is not None:
        same(got, want, case.id)
    return [name]


@chunked("maxpool")
def test_maxpool(chunk):
    sweep("maxpool", chunk, run_maxpool)


def test_maxpool_reaches_every_kernel():
    assert kernels_of("maxpool", run_maxpool) >= {"k_maxpool2d", "k_maxpool2d_pad", "k_maxpool2d_pad<ceil>"}


# ---- 6. conv_transpose2d_bias_act -------------------------------------------------------------------------------------------------------
def run_convt(case, d, want):
    g = case.g
    got = F.conv_transpose2d_bias_act(dev(d["x"]), dev(d["w"]), dev(d["bias"]), g["act"], padding=0 if g["k"] == 2 else 1)
    name = _lib.last_kernel()
    assert tuple(got.shape) == (g["n"], g["cout"], 2 * g["h"], 2 * g["w"]), case.id
    if g["k"] == 2:
        slices = F.conv1x1_k_slices(g["n"], g["cin"], g["h"], g["w"], 4 * g["cout"])[0]
        assert name.startswith("k_conv1x1_ct<") and name.endswith(f"ks{slices},{'vec16' if g['w'] % 2 == 0 else 'scalar'}>"), (case.id, name)
    else:
        assert name.startswith("k_conv_igemm_tr<"), (case.id, name)
    if want is not None:
        same_bits(got, want, case.id)
    return [name]


@chunked("convt")
def test_convt(chunk):
    sweep("convt", chunk, run_convt)


def test_convt_reaches_every_kernel():
    names = kernels_of("convt", run_convt)
    pixel_shuffle = {n for n in names if n.startswith("k_conv1x1_ct<")}
    assert any(n.startswith("k_conv_igemm_tr<") for n in names), names
    assert any("ks1," in n for n in pixel_shuffle) and any("ks1," not in n for n in pixel_shuffle), names
    assert any(n.endswith("vec16>") for n in pixel_shuffle) and any(n.endswith("scalar>") for n in pixel_shuffle), names


# ---- 7. group_norm_act -------------------------------------------------------------------------------------------------------------------
def run_groupnorm(case, d, want):
    g = case.g
    got = F.group_norm_act(dev(d["x"]), g["groups"], dev(d["weight"]), dev(d["bias"]), g["eps"], relu=g["relu"])
    name = _lib.last_kernel()
    assert name.startswith("k_gn_apply<") and name.endswith(f"relu{int(g['relu'])}>"), (case.id, name)
    if want is not None:
        same_bits(got, want, case.id)
    return [name]


@chunked("groupnorm")
def test_groupnorm(chunk):
    sweep("groupnorm", chunk, run_groupnorm)


def test_groupnorm_reaches_every_kernel():
    names = kernels_of("groupnorm", run_groupnorm)
    forms = {(n.split("<")[1].split(",")[0], n[-6:-1]) for n in names}
    assert forms == {(form, relu) for form in ("vec", "scalar") for relu in ("relu0", "relu1")}, names


# ---- 8. l2_normalize_scale ---------------------------------------------------------------------------------------------------------------
def run_l2norm(case, d, want):
    got = F.l2_normalize_scale(dev(d["x"]), dev(d["weight"]), case.g["eps"])
    name = _lib.last_kernel()
    if want is not None:
        same(got, want, case.id)
    return [name]


@chunked("l2norm")
def test_l2norm(chunk):
    sweep("l2norm", chunk, run_l2norm)


def test_l2norm_reaches_every_kernel():
    assert kernels_of("l2norm", run_l2norm) == {"k_l2_normalize_scale"}


# ---- 9. conv1x1_upsample_add -------------------------------------------------------------------------------------------------------------
def run_lateral(case, d, want):
    g = case.g
    got = F.conv1x1_upsample_add(dev(d["x"]), dev(d["w"]), *_epilogue_args(d), dev(d["top"]), affine=g["affine"], activation=g["act"])
    name = _lib.last_kernel()
    assert name.startswith("k_conv1x1_up<"), (case.id, name)
    if want is not None:
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{case.id} [{name}]")
    return [name]


@chunked("lateral")
def test_lateral(chunk):
    sweep("lateral", chunk, run_lateral)


def test_lateral_reaches_every_kernel():
    names = kernels_of("lateral", run_lateral)
    # one K chunk, and cout <= 32 / <= 64 / more: the three widths of a wave tile (tests/test_gpu_fpn.py::INSTANCES)
    assert names >= {"k_conv1x1_up<1,1>", "k_conv1x1_up<1,2>", "k_conv1x1_up<1,4>"}, names


# ---- 10. interpolate, interpolate_argmax, conv1x1_gated_upsample -----------------------------------------------------------------------
def run_interp(case, d, want):
    g = case.g
    got = F.interpolate(dev(d["x"]), size=(g["oh"], g["ow"]))
    name = _lib.last_kernel()
    assert name == f"k_interp_batch<plain,{'vec16' if g['ow'] % 4 == 0 else 'scalar'}>", (case.id, name)
    if want is not None:
        same(got, want, case.id)
    return [name]


@chunked("interp")
def test_interp(chunk):
    sweep("interp", chunk, run_interp)


def test_interp_reaches_every_kernel():
    assert kernels_of("interp", run_interp) == {"k_interp_batch<plain,vec16>", "k_interp_batch<plain,scalar>"}


def run_argmax(case, d, want):
    g = case.g
    xd = dev(d["x"])
    names = []
    for dtype, kind in ((torch.int64, "i64"), (torch.uint8, "u8")):
        got = F.interpolate_argmax(xd, size=(g["oh"], g["ow"]), dtype=dtype)
        names.append(_lib.last_kernel())
        assert names[-1] == f"k_interp_argmax<{kind},{'vec' if g['ow'] % 4 == 0 else 'scalar'}>", (case.id, names[-1])
        assert got.dtype == dtype and tuple(got.shape) == (g["n"], g["oh"], g["ow"]), case.id
        if want is not None:
            assert np.array_equal(got.cpu().numpy().astype(np.int64), want), f"{case.id} {kind}"
    return names


@chunked("argmax")
def test_argmax(chunk):
    sweep("argmax", chunk, run_argmax)


def test_argmax_reaches_every_kernel():
    assert kernels_of("argmax", run_argmax) == {f"k_interp_argmax<{kind},{form}>" for kind in ("i64", "u8") for form in ("vec", "scalar")}


def run_gated_up(case, d, want):
    g = case.g
    xd, gd, wd, bd, rd = (dev(d[k]) for k in ("x", "gate", "w", "bias", "res"))
    size = (g["oh"], g["ow"])
    got = F.conv1x1_gated_upsample(xd, gd, wd, bd, rd, size=size)
    name = _lib.last_kernel()
    assert name.startswith("k_conv1x1_gu<"), (case.id, name)
    assert ("ks" in name) == (F.conv1x1_k_slices(g["n"], g["cin"], g["oh"], g["ow"], g["cout"])[0] > 1), (case.id, name)
    unfused = F.conv_norm_act(F.interpolate(F.se_scale(xd, gd), size=size), wd, bd, residual=rd)
    same(got, unfused, case.id + " vs the unfused composition")
    if want is not None:
        same(got, want, case.id)
    return [name]


@chunked("gated_up")
def test_gated_up(chunk):
    sweep("gated_up", chunk, run_gated_up)


def test_gated_up_reaches_every_kernel():
    names = kernels_of("gated_up", run_gated_up)
    assert all(n.startswith("k_conv1x1_gu<") for n in names) and any("ks" in n for n in names) and any("ks" not in n for n in names), names
