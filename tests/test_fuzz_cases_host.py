"""The random-shape sweeps of tests/test_gpu_fuzz_layers.py and tests/test_gpu_fuzz_ops.py cannot pass vacuously (runs without a GPU).
For every family of tests/_fuzz_cases.py:

  reproducible   generating a chunk twice gives the same cases; the ids are unique;
  valid          every case has outputs of at least one element a side, stays a few MB at the most, and passes the entry point's own
                 host path: the public function runs on CPU tensors with the launch replaced by nothing, so every check in front of
                 the launch sees the case (a refused case would otherwise hide behind a pytest.raises nobody wrote);
  coverage       conditions on the geometry and on the library's host queries alone: the drawn cases reach every regime the
                 family's kernel has (the residues of w mod 4, a one-row last block, both sides of the short-launch rule, the K-slice
                 plans, both sides of group_norm_chunk(), several column blocks, every box kind, every nms block size, ...).  These
                 are conditions, not measurements: the seeds and boundary lists of _fuzz_cases.py are chosen so that they hold;
  float64        every case's reference against the same operation composed from torch's CPU ops in float64, within a derived bound.

The bound.  With u = 2^-24 and gamma(k) = k u / (1 - k u), a float32 chain of T multiply-adds followed by E rounded epilogue
operations differs from the exact value by at most gamma(T + E) A, A the float64 sum of the absolute values of every term that enters
the output (the products |w x|, then |bias|, times |alpha| plus |beta|, plus |residual|: Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1); the float64 yardstick adds less than one more u A, and one more covers the input of the
activation, so

      |reference - float64| <= gamma(T + E + 2) A L,

L the activation's Lipschitz constant (1 for none / ReLU / ReLU6, 1.5 for Hardswish, whose own three roundings count in E and whose
output is at most |v| <= A).  sigmoid and hardsigmoid (the squeeze-excitation gates) have outputs that A does not bound, so their
own roundings are taken relative to the output: gamma(T + E + 2) (A L + |y|).  A reference that sums in float64 and rounds once
(the pool, the dense layer, GroupNorm's statistics, the L2 norm) lies far inside the same bound.  The others follow the same rule:

  group_norm   y = ((x - mean) rstd) w + b with float32 mean and rstd: 6 roundings on terms of size (|x| + |mean|) rstd |w| and |b|;
  l2_normalize y = w (x / norm): 3 roundings of y itself;
  bilinear     3 fused multiply-adds and 2 products on the four taps: gamma(6 + 2) A; the float32 source coordinate s (d + 0.5) - 0.5
               carries 2 roundings of size u n_in and 1 - lambda one more, which moves the value by at most gamma(3) (n_in + 1) times
               the largest difference D of two neighbouring pixels along that axis (the interpolant is piecewise linear with slope
               <= D, and continuous where the taps change);
  gated upsample   the pointwise chain over the resized gated map u: gamma(cin + E + 2 + slices) A, plus sum |w| (the bound of u);
  squeeze-excitation gate   the two dense layers in turn, each passing the bound e of its input on as L |w| e;
  RoI ops      a bin is the mean of S bilinear samples: gamma(4 S + 12) max|x|, and the float32 sample coordinate (6 operations on
               coordinates up to c) moves a sample by at most 4 max|x| gamma(8) (c + 2); the max pools are exact.  The float64 side
               is not the restatement run in float64 but a composition of its own: per roi and axis a matrix of summed bilinear
               weights, applied with torch.einsum, and explicit integer windows under torch's max and mean.

Outputs that are labels or indices (argmax, nms, the pools' windows, roi_pool's argmax, the position-sensitive ops' channel mappings,
the keypoints' positions) must be equal wherever the float64 margin exceeds the bound of the two candidates; the share excluded by that margin is at most 1 % per family, asserted.  paste and
keypoints keep their stated bounds, tests/_mask_ref.paste_bound and tests/_keypoint_ref.bicubic_bound, against the replicas, as
tests/test_mask_host.py and tests/test_keypoint_host.py apply them."""
import functools

import numpy as np
import pytest
import torch
from torch.nn import functional as TF

from cpu_vision_amd import _lib, ops
from cpu_vision_amd import functional as F
from tests import _fuzz_cases as FC

U = 2.0 ** -24
FAMILIES = list(FC.SWEEPS)
MAX_BYTES = 8 << 20


def gamma(k):
    return k * U / (1 - k * U)


@functools.lru_cache(maxsize=None)
def all_cases(family):
    return tuple(FC.cases(family))


def g64(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).double()


def close(ref, f64, bound, what):
    """|ref - f64| <= bound elementwise (arrays or tensors)."""
    ref, f64, bound = (np.asarray(v, np.float64) for v in (ref, f64, bound))
    assert ref.shape == f64.shape, (what, ref.shape, f64.shape)
    err = np.abs(ref - f64)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outputs outside the bound, the worst {float(np.nanmax(err / np.maximum(bound, 1e-300))):.3g} x it"


# ---- reproducible, unique ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_cases_are_reproducible_and_ids_unique(family):
    first, chunks, count = FC.SWEEPS[family]
    assert 2 <= chunks <= 4 and 10 <= count <= 25
    again = FC.cases(family)
    assert list(all_cases(family)) == again and len(again) == chunks * count
    ids = [c.id for c in again]
    assert len(set(ids)) == len(ids)
    for c in again[:3]:
        assert c.id.startswith(f"{family}[sweep {c.sweep} #{c.index}] ") and all(f"{k}={v}" in c.id for k, v in c.geom)
        a, b = FC.inputs(c), FC.inputs(c)
        assert all(np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


def test_the_constants_come_from_the_sources():
    assert FC.constant("kWave") == 64 and FC.constant("kColsPerBlock", "segment.hip") == 4 * FC.constant("kWave")
    assert FC.constant("kGnChunk") == F.group_norm_chunk()
    assert FC.around(4, 8) == [3, 4, 5, 7, 8, 9] and FC.factor(257) == (1, 257) and FC.factor(256) == (16, 16)


# ---- valid -------------------------------------------------------------------------------------------------------------------------------
def cpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def dry_call(case, d, monkeypatch):
    """The public entry point of a case on CPU tensors: everything in front of the launch runs, the launch does not."""
    g = case.g
    ep = lambda: (cpu(d["bias"]), cpu(d["alpha"]), cpu(d["beta"]))  # noqa: E731
    fam = case.family
    if fam == "dw5x5":
        return F.conv_norm_act(cpu(d["x"]), cpu(d["w"]), *ep(), cpu(d["res"]), stride=g["stride"], groups=g["c"], affine=g["affine"],
                               activation=g["act"], dilation=g["dilation"])
    if fam == "pw_scaled":
        return F.conv_norm_act(cpu(d["x"]), cpu(d["w"]), *ep(), cpu(d["res"]), affine=g["affine"], activation=g["act"], input_scale=cpu(d["gate"]))
    if fam == "se":
        F.global_avg_pool(cpu(d["x"])), F.se_scale(cpu(d["x"]), cpu(d["gate"])), F.linear_act(cpu(d["xl"]), cpu(d["wl"]), cpu(d["bl"]), g["act"])
        return F.squeeze_excitation_gate(cpu(d["x"]), cpu(d["w1"]), cpu(d["b1"]), cpu(d["w2"]), cpu(d["b2"]), g["gate_act"], g["scale_act"])
    if fam == "conv2d":
        monkeypatch.setattr(F, "CONV2D_SMALL_LAUNCH_WORKSPACE", g["columns"])
        return F.conv2d_affine_act(cpu(d["x"]), cpu(d["w"]), *ep(), cpu(d["res"]), stride=g["stride"], padding=g["padding"], dilation=g["dilation"],
                                   groups=g["groups"], affine=g["affine"], activation=g["act"])
    if fam == "maxpool":
        return F.max_pool2d(cpu(d["x"]), g["k"], g["stride"], g["padding"], ceil_mode=g["ceil_mode"])
    if fam == "convt":
        return F.conv_transpose2d_bias_act(cpu(d["x"]), cpu(d["w"]), cpu(d["bias"]), g["act"], padding=0 if g["k"] == 2 else 1)
    if fam == "groupnorm":
        return F.group_norm_act(cpu(d["x"]), g["groups"], cpu(d["weight"]), cpu(d["bias"]), g["eps"], relu=g["relu"])
    if fam == "l2norm":
        return F.l2_normalize_scale(cpu(d["x"]), cpu(d["weight"]), g["eps"])
    if fam == "lateral":
        return F.conv1x1_upsample_add(cpu(d["x"]), cpu(d["w"]), *ep(), cpu(d["top"]), affine=g["affine"], activation=g["act"])
    if fam == "interp":
        return F.interpolate(cpu(d["x"]), size=(g["oh"], g["ow"]))
    if fam == "argmax":
        return [F.interpolate_argmax(cpu(d["x"]), size=(g["oh"], g["ow"]), dtype=t) for t in (torch.int64, torch.uint8)][0]
    if fam == "gated_up":
        return F.conv1x1_gated_upsample(cpu(d["x"]), cpu(d["gate"]), cpu(d["w"]), cpu(d["bias"]), cpu(d["res"]), size=(g["oh"], g["ow"]))
    if fam == "roi":
        tail = {"roi_align": (g.get("ratio"), g.get("aligned")), "ps_roi_align": (g.get("ratio"),)}.get(g["op"], ())
        return getattr(ops, g["op"])(cpu(d["x"]), cpu(d["rois"]), (g["ph"], g["pw"]), g["scale"], *tail)
    if fam == "nms":
        if "idxs" in d:
            return ops.batched_nms(cpu(d["boxes"]), cpu(d["scores"]), cpu(d["idxs"]), g["thr"])
        return ops.nms(cpu(d["boxes"]), cpu(d["scores"]), g["thr"])  # (its length is the one read-back: a count nothing wrote)
    if fam == "paste":
        return F.paste_masks_in_image(cpu(d["masks"]), cpu(d["boxes"]), (g["h"], g["w"]), g["padding"])
    assert fam == "keypoints", fam
    return F.heatmaps_to_keypoints(cpu(d["maps"]), cpu(d["rois"]))[0]


def _stub_the_launch(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda t, what="input": None)
    monkeypatch.setattr(_lib, "launch", lambda fn, on, *args: None)


def expected_shape(case):
    g = case.g
    fam = case.family
    if fam == "dw5x5":
        return (g["n"], g["c"], (g["h"] - 1) // g["stride"] + 1, (g["w"] - 1) // g["stride"] + 1)
    if fam in ("pw_scaled", "lateral"):
        return (g["n"], g["cout"], g["h"], g["w"])
    if fam == "se":
        return (g["n"], g["c"])
    if fam == "conv2d":
        return (g["n"], g["cout"]) + tuple(FC.conv_out(g[a], g[k], g["stride"], g["padding"], g["dilation"]) for a, k in (("h", "kh"), ("w", "kw")))
    if fam == "maxpool":
        x = torch.zeros(1, 1, g["h"], g["w"])
        return (g["n"], g["c"]) + tuple(TF.max_pool2d(x, g["k"], g["stride"], g["padding"], ceil_mode=g["ceil_mode"]).shape[-2:])
    if fam == "convt":
        return (g["n"], g["cout"], 2 * g["h"], 2 * g["w"])
    if fam in ("groupnorm", "l2norm"):
        return (g["n"], g["c"], g["h"], g["w"])
    if fam == "interp":
        return (g["n"], g["c"], g["oh"], g["ow"])
    if fam == "argmax":
        return (g["n"], g["oh"], g["ow"])
    if fam == "gated_up":
        return (g["n"], g["cout"], g["oh"], g["ow"])
    if fam == "roi":
        return (g["rois"], g["c"] // (g["ph"] * g["pw"]) if g["op"].startswith("ps_") else g["c"], g["ph"], g["pw"])
    if fam == "paste":
        return (g["rois"], 1, g["h"], g["w"])
    if fam == "keypoints":
        return (g["rois"], g["k"], 3)
    return None  # nms: a list of indices


@pytest.mark.parametrize("family", FAMILIES)
def test_cases_are_valid(family, monkeypatch):
    _stub_the_launch(monkeypatch)
    sizes = []
    for case in all_cases(family):
        d = FC.inputs(case)
        sizes.append(FC.nbytes(d))
        shape = expected_shape(case)
        out = dry_call(case, d, monkeypatch)  # raises where the host path refuses the case
        if shape is not None:
            assert tuple(out.shape) == shape, (case.id, tuple(out.shape), shape)
            assert all(s >= 1 for s in shape[1:]) and (shape[0] >= 1 or family == "roi"), case.id
    assert max(sizes) <= MAX_BYTES and np.median(sizes) <= 1 << 20, (family, max(sizes), np.median(sizes))


def test_cases_stay_inside_the_stated_limits():
    """The limits that the entry points' comments state and no Python check enforces."""
    for c in all_cases("argmax"):
        assert c.g["classes"] <= 256  # uint8 labels
    for c in all_cases("nms"):
        assert c.g["boxes"] <= FC.constant("kNmsMaxBoxes")
    for c in all_cases("keypoints"):
        assert c.g["mh"] * c.g["mw"] <= FC.constant("kKpMaxPlane")
        assert float(np.abs(FC.inputs(c)["rois"]).max()) < FC.constant("kKpMaxRoiSide", "keypoint.hip") / 2
    for c in all_cases("maxpool"):
        assert FC.pool_is_valid(*(c.g[k] for k in ("h", "w", "k", "stride", "padding", "ceil_mode")))
    for c in all_cases("groupnorm"):
        assert c.g["c"] % c.g["groups"] == 0 and 1 <= c.g["c"] // c.g["groups"] <= 16
    for c in all_cases("conv2d"):
        assert c.g["cin"] % c.g["groups"] == 0 and c.g["cout"] % c.g["groups"] == 0


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
def values(family, *keys):
    return {tuple(c.g[k] for k in keys) if len(keys) > 1 else c.g[keys[0]] for c in all_cases(family)}


def epilogue_classes(family, keys=("bias", "affine", "res", "act")):
    return {tuple(c.g[k] for k in keys) for c in all_cases(family)}


def test_coverage_dw5x5():
    cs = all_cases("dw5x5")
    rows, short = FC.constant("kDw5Rows"), FC.constant("kDw5ShortLaunch")
    assert values("dw5x5", "stride", "dilation") == set(FC.DW_MODES)
    assert epilogue_classes("dw5x5") == set(FC.EPILOGUES)
    for mode in FC.DW_MODES:
        mine = [c.g for c in cs if (c.g["stride"], c.g["dilation"]) == mode]
        assert {g["w"] % 4 for g in mine} == {0, 1, 2, 3} and {((g["w"] - 1) // mode[0] + 1) % 4 for g in mine} == {0, 1, 2, 3}, mode
        plans = [FC.dw5x5_plan(g["n"], g["c"], g["h"], g["w"], *mode) for g in mine]
        assert {p[0] for p in plans} == {rows, rows // 2}, mode  # both sides of the short-launch rule
        assert min(p[1] for p in plans if p[0] == rows) == short, mode  # and the launch exactly at it
        # a last row block of one row, under the strip the launcher takes
        assert any(((g["h"] - 1) // mode[0] + 1) % (p[0] * mode[1]) == 1 and (g["h"] - 1) // mode[0] + 1 > 1 for g, p in zip(mine, plans)), mode
        assert {g["act"] for g in mine} == set(FC.ACTS) and {g["affine"] for g in mine} == {None, "mul_add", "fma"}
    assert any(FC.dw5x5_plan(c.g["n"], c.g["c"], c.g["h"], c.g["w"], 1, 1)[1] in range(short - 1024, short) for c in cs if c.g["dilation"] == 1)
    assert min(c.g["h"] for c in cs) == 1 and min(c.g["w"] for c in cs) == 1 and {1, 2} <= {c.g["c"] for c in cs}
    for chunk in FC.chunks("dw5x5"):  # every chunk has a launch at the threshold
        assert any(FC.dw5x5_plan(c.g["n"], c.g["c"], c.g["h"], c.g["w"], c.g["stride"], c.g["dilation"]) == (rows, short) for c in FC.cases("dw5x5", chunk)), chunk


def _pointwise_plans(family, out=("h", "w"), cout=1):
    return [F.conv1x1_k_slices(c.g["n"], c.g["cin"], c.g[out[0]], c.g[out[1]], cout * c.g["cout"]) for c in all_cases(family)]


def test_coverage_pw_scaled():
    cs = all_cases("pw_scaled")
    plans = _pointwise_plans("pw_scaled")
    assert {p[0] for p in plans} >= {1, 2} and any(s > 1 and c.g["cin"] % sl for c, (s, sl) in zip(cs, plans))  # a ragged last slice
    step = FC.conv1x1_slice_steps()[1][0]  # the first channel count a small launch runs in slices
    assert {step - 1, step} <= {c.g["cin"] for c in cs}
    chunk = FC.constant("kPK", "convnorm.hip")
    assert {c.g["cin"] % chunk == 0 for c in cs} == {True, False} and any(c.g["cin"] < chunk for c in cs)
    assert epilogue_classes("pw_scaled") == set(FC.EPILOGUES)
    assert {(1, 1), (28, 28)} <= values("pw_scaled", "h", "w") | {(c.g["h"], c.g["h"]) for c in cs if c.g["h"] == c.g["w"]}
    assert {1, 200} <= {c.g["cin"] for c in cs} and {1, 200} <= {c.g["cout"] for c in cs}
    assert all((FC.inputs(c)["gate"] == 0).any() for c in cs[:8])


def test_coverage_se():
    cs = all_cases("se")
    wave = FC.constant("kWave")
    lengths = {c.g["h"] * c.g["w"] for c in cs}
    for edge in (wave, 4 * wave):
        assert {edge - 1, edge, edge + 1} <= lengths, (edge, sorted(lengths))
    assert {1, 33 * 33} <= lengths and max(c.g["n"] * c.g["c"] for c in cs) <= 300
    assert {c.g["act"] for c in cs} == set(FC.LIN_ACTS) and {c.g["lin_bias"] for c in cs} == {True, False}
    ks, ms = {c.g["k"] for c in cs}, {c.g["m"] for c in cs}
    assert any(k < wave for k in ks) and any(k % wave == 0 for k in ks) and any(k > 16 * wave for k in ks) and max(ks) <= 1100
    assert min(ms) >= 1 and max(ms) <= 130 and any(m > wave for m in ms)
    assert {(c.g["h"] * c.g["w"]) % 4 == 0 for c in cs} == {True, False}  # both forms of se_scale
    assert values("se", "gate_act", "scale_act") == {(a, b) for a in ("relu", "hardswish") for b in ("sigmoid", "hardsigmoid")}


def test_coverage_conv2d():
    cs = all_cases("conv2d")
    assert {c.g["kh"] for c in cs} == {c.g["kw"] for c in cs} == set(range(1, 8))
    assert {c.g["stride"] for c in cs} == {1, 2} and {c.g["padding"] for c in cs} == {0, 1, 2, 3} and {c.g["dilation"] for c in cs} == {1, 2, 3}
    kinds = {("1" if c.g["groups"] == 1 else "2" if c.g["groups"] == 2 and c.g["cin"] != 2 else "cin") for c in cs}
    assert kinds == {"1", "2", "cin"}
    per_group = [c.g["cin"] // c.g["groups"] for c in cs]
    slices = {-(-k // FC.SLICE_CHANNELS) for k in per_group}
    assert slices >= {1, 2, 3} and any(k > FC.SLICE_CHANNELS and k % FC.SLICE_CHANNELS for k in per_group)
    assert epilogue_classes("conv2d") == set(FC.EPILOGUES)
    lib = _lib.load()
    need = {}
    for c in cs:
        g = c.g
        n = int(lib.mv_conv2d_needs_workspace(g["n"], g["cin"], g["cout"], g["h"], g["w"], g["kh"], g["kw"], g["stride"], g["stride"], g["padding"],
                                              g["padding"], g["dilation"], g["dilation"], g["groups"]))
        need.setdefault(n, set()).add(g["columns"])
    assert need.get(2) == {True, False}, need  # launches whose form the switch decides, with the switch both ways


def test_coverage_maxpool():
    cs = all_cases("maxpool")
    assert values("maxpool", "k", "ceil_mode") == {(k, m) for k in (2, 3) for m in (False, True)}
    assert {c.g["stride"] for c in cs} == {1, 2, 3} and {c.g["padding"] for c in cs} == {0, 1}
    assert {c.g["ceil_mode"] for c in cs if c.g["h"] == 1 and c.g["w"] == 1} == {False, True}  # a 1 x 1 map in both modes
    # ceil mode with a clipped last window, and with the last window dropped because it would start in the padding
    clipped = dropped = False
    for c in cs:
        g = c.g
        if g["ceil_mode"]:
            o = -((g["h"] + 2 * g["padding"] - g["k"]) // -g["stride"]) + 1
            floor = (g["h"] + 2 * g["padding"] - g["k"]) // g["stride"] + 1
            kept = o - 1 if (o - 1) * g["stride"] >= g["h"] + g["padding"] else o
            clipped |= kept > floor
            dropped |= kept < o
    assert clipped and dropped


def test_coverage_convt():
    cs = all_cases("convt")
    assert values("convt", "k", "act") == {(k, a) for k in (2, 4) for a in FC.CT_ACTS}
    assert values("convt", "k", "bias") == {(k, b) for k in (2, 4) for b in (False, True)}
    two = [c for c in cs if c.g["k"] == 2]
    plans = [F.conv1x1_k_slices(c.g["n"], c.g["cin"], c.g["h"], c.g["w"], 4 * c.g["cout"])[0] for c in two]
    assert 1 in plans and max(plans) > 1
    assert {c.g["w"] % 2 for c in two} == {0, 1}  # the 16-byte and the scalar store of the pixel shuffle
    assert min(c.g["h"] * c.g["w"] for c in cs) == 1 and max(c.g["cin"] for c in cs) >= 256 and {1, 40} <= {c.g["cout"] for c in cs}


def test_coverage_groupnorm():
    cs = all_cases("groupnorm")
    wave, group, chunk = FC.constant("kWave"), FC.constant("kGnThreads", "groupnorm.hip"), F.group_norm_chunk()
    slabs = {(c.g["c"] // c.g["groups"]) * c.g["h"] * c.g["w"] for c in cs}
    assert any(m < wave for m in slabs)
    for edge in (group, chunk):
        assert {edge - 1, edge, edge + 1} <= slabs, (edge, sorted(slabs))
    assert any(m > 2 * chunk for m in slabs) and any(chunk < m < 2 * chunk for m in slabs)
    assert {m % 4 == 0 for m in slabs} == {True, False}
    assert values("groupnorm", "weight", "gn_bias", "relu") == {(a, b, r) for a in (False, True) for b in (False, True) for r in (False, True)}
    per = {c.g["c"] // c.g["groups"] for c in cs}
    assert {1, 16} <= per and any(c.g["groups"] == 1 for c in cs) and any(c.g["groups"] == c.g["c"] > 1 for c in cs)


def test_coverage_l2norm():
    cs = all_cases("l2norm")
    pixels, groups = FC.constant("kL2Pixels"), FC.constant("kL2Groups")
    cset, pset = {c.g["c"] for c in cs}, {c.g["h"] * c.g["w"] for c in cs}
    assert any(c < groups for c in cset) and any(c % groups == 0 for c in cset) and any(c > groups and c % groups for c in cset) and max(cset) <= 600
    assert {1, 600} <= cset and any(p < pixels for p in pset) and any(p > pixels and p % pixels for p in pset) and 1 in pset
    zero = [c for c in cs if c.g["zero_pixel"]]
    assert zero and len(zero) < len(cs)
    for c in zero[:3]:
        assert (np.abs(FC.inputs(c)["x"]).sum(1) == 0).any()


def test_coverage_lateral():
    cs = all_cases("lateral")
    rel = set()
    for c in cs:
        g = c.g
        for a, t in ((g["h"], g["th"]), (g["w"], g["tw"])):
            rel.add("equal" if t == a else "one" if t == 1 else "larger" if t > a else "half" if 2 * t == a else "ceil-half" if t == (a + 1) // 2 else "smaller")
    assert rel == {"equal", "one", "larger", "half", "ceil-half", "smaller"}
    # sizes at which torch's nearest index repeats unevenly: the output is no multiple of the top map
    assert any(g["h"] % g["th"] and g["th"] < g["h"] for g in (c.g for c in cs)) and any(g["w"] % g["tw"] and g["tw"] < g["w"] for g in (c.g for c in cs))
    assert epilogue_classes("lateral", ("bias", "affine", "act")) == {(b, a, t) for b, a, _, t in FC.EPILOGUES}
    chunk = FC.constant("kPK", "convnorm.hip")
    assert any(c.g["cin"] <= chunk for c in cs) and any(c.g["cin"] > chunk for c in cs)
    assert any(c.g["cout"] <= 32 for c in cs) and any(32 < c.g["cout"] <= 64 for c in cs) and any(c.g["cout"] > 64 for c in cs)


def _resize_coverage(family, source):
    cs = all_cases(family)
    cols = FC.constant("kColsPerBlock", source)
    kinds = set()
    for c in cs:
        g = c.g
        for a, b in ((g["h"], g["oh"]), (g["w"], g["ow"])):
            kinds.add("identity" if a == b else "enlarge" if b > a else "shrink")
    assert kinds == {"identity", "enlarge", "shrink"}
    blocks = {-(-c.g["ow"] // cols) for c in cs}
    assert {1, 2, 3} <= blocks, blocks  # one column block, two, and more
    assert {c.g["ow"] % 4 == 0 for c in cs} == {True, False}
    assert any(c.g["h"] == 1 or c.g["w"] == 1 for c in cs) and any(c.g["oh"] == 1 or c.g["ow"] == 1 for c in cs)
    assert any(c.g["ow"] in (cols, 2 * cols) for c in cs) and any(c.g["ow"] in (cols + 1, 2 * cols + 1) for c in cs)
    return cs


def test_coverage_interp_and_argmax():
    _resize_coverage("interp", "interp.hip")
    cs = _resize_coverage("argmax", "segment.hip")
    assert {1, 2, 40} <= {c.g["classes"] for c in cs}
    dup = [c for c in cs if c.g["dup"] >= 0]
    assert len(dup) >= 8
    wins = 0
    for c in dup[:8]:
        x = FC.inputs(c)["x"]
        want = FC.reference(c, dict(x=x))
        assert np.array_equal(x[:, -1], x[:, c.g["dup"]]) and not (want == c.g["classes"] - 1).any()  # of two equal planes the first wins
        wins += bool((want == c.g["dup"]).any())
    assert wins >= 4  # and the tie is met: the earlier plane is the maximum somewhere


def test_coverage_gated_up():
    cs = all_cases("gated_up")
    plans = _pointwise_plans("gated_up", ("oh", "ow"))
    assert {p[0] for p in plans} >= {1, 2} and any(s > 1 and c.g["cin"] % sl for c, (s, sl) in zip(cs, plans))
    assert values("gated_up", "bias", "res") == {(a, b) for a in (False, True) for b in (False, True)}
    kinds = {("identity" if (c.g["h"], c.g["w"]) == (c.g["oh"], c.g["ow"]) else "enlarge" if c.g["oh"] > c.g["h"] else "shrink") for c in cs}
    assert kinds == {"identity", "enlarge", "shrink"}
    assert any(c.g["h"] * c.g["w"] == 1 for c in cs) and any(c.g["oh"] * c.g["ow"] == 1 for c in cs)  # a 1 x 1 source, a 1 x 1 output


def test_coverage_roi():
    cs = all_cases("roi")
    assert {c.g["op"] for c in cs} == set(FC.ROI_OPS)
    for op in FC.ROI_OPS:
        mine = [c.g for c in cs if c.g["op"] == op]
        assert {g["scale"] for g in mine} == set(FC.ROI_SCALES), op
        if "ratio" in mine[0]:
            assert {g["ratio"] for g in mine} == {0, 1, 2, 3}, op
        assert any(g["ph"] != g["pw"] for g in mine) and {1, 7} <= {g["ph"] for g in mine} | {g["pw"] for g in mine}, op
    assert {(c.g["aligned"], c.g["ratio"] > 0) for c in cs if c.g["op"] == "roi_align"} == {(a, f) for a in (False, True) for f in (False, True)}
    assert {c.g["op"] for c in cs if c.g["rois"] == 0} == set(FC.ROI_OPS)  # the empty list through every operator
    assert any(c.g["h"] == 1 for c in cs) and any(c.g["w"] == 1 for c in cs) and any(c.g["h"] == 40 for c in cs)
    # every box kind, checked on the boxes themselves
    c = next(c for c in cs if c.g["rois"] and c.g["n"] > 1 and c.g["h"] > 4 and c.g["w"] > 4)
    rois = FC.inputs(c)["rois"].astype(np.float64)
    b = rois[:, 1:] * c.g["scale"]
    W, H = c.g["w"], c.g["h"]
    kinds = set()
    for x1, y1, x2, y2 in b:
        kinds.add("inverted" if x2 < x1 and y2 < y1 else "zero_width" if x2 == x1 else "zero_height" if y2 == y1 else
                  "outside" if x2 < 0 or y2 < 0 or x1 > W or y1 > H else "larger" if x1 < 0 and y1 < 0 and x2 > W and y2 > H else
                  "left" if abs(x1) < 1e-5 else "top" if abs(y1) < 1e-5 else "right" if abs(x2 - W) < 1e-4 else "bottom" if abs(y2 - H) < 1e-4 else "inside")
    assert kinds == set(FC.ROI_KINDS), kinds
    assert {0, c.g["n"] - 1} <= set(rois[:, 0].astype(int))  # the first and the last image


def test_coverage_nms():
    cs = all_cases("nms")
    counts = {c.g["boxes"] for c in cs}
    assert {0, 1, 2} <= counts and max(counts) == 1500
    for block in FC.nms_block_sizes():
        assert {block - 1, block, block + 1} <= counts, (block, sorted(counts))
    assert values("nms", "kind", "thr") == {(k, t) for k in FC.NMS_KINDS for t in FC.NMS_THRESHOLDS}
    batched = [c for c in cs if c.g["classes"]]
    assert len(batched) >= 10 and {c.g["kind"] for c in batched} == set(FC.NMS_KINDS)


def test_coverage_paste_and_keypoints():
    cols = FC.constant("kPasteColsPerBlock", "mask.hip")
    cs = all_cases("paste")
    assert any(c.g["w"] > cols for c in cs) and {c.g["w"] % 4 == 0 for c in cs} == {True, False} and {c.g["padding"] for c in cs} == {0, 1}
    assert min(c.g["h"] for c in cs) <= 2 and min(c.g["w"] for c in cs) <= 2 and {1, 28} <= {c.g["m"] for c in cs}
    for fam, key in (("paste", "boxes"), ("keypoints", "rois")):
        c = next(c for c in all_cases(fam) if c.g["h"] > 8 and c.g["w"] > 8)
        b, (H, W) = FC.inputs(c)[key].astype(np.float64), (c.g["h"], c.g["w"])
        assert len(b) == len(FC.BOX_KINDS)
        assert (b[1, 0] < 0 < b[1, 2]) and (b[2, 1] < 0 < b[2, 3]) and (b[3, 0] < W < b[3, 2]) and (b[4, 1] < H < b[4, 3])  # partly outside
        assert b[5, 2] < 0 or b[5, 0] > W or b[5, 3] < 0 or b[5, 1] > H  # wholly outside
        assert b[6, 2] - b[6, 0] < 1  # one pixel wide
        assert b[7, 0] < 0 and b[7, 1] < 0 and b[7, 2] > W and b[7, 3] > H  # larger than the image
    ks = all_cases("keypoints")
    assert {1, 17} <= {c.g["k"] for c in ks} and min(c.g["mh"] for c in ks) == min(c.g["mw"] for c in ks) == 2
    assert any(c.g["mh"] >= c.g["h"] for c in ks) and any(8 * c.g["mh"] <= c.g["h"] + 7 and c.g["h"] > 16 for c in ks)  # maps as large as the image, and an eighth


# ---- the references against float64 ------------------------------------------------------------------------------------------------------
ACT_ROUNDINGS = {None: 0, "relu": 0, "relu6": 0, "hardswish": 4, "hardsigmoid": 3, "sigmoid": 3}
LIPSCHITZ = {None: 1.0, "relu": 1.0, "relu6": 1.0, "hardswish": 1.5, "hardsigmoid": 1.0, "sigmoid": 1.0}


def act64(v, act):
    if act == "relu":
        return v.clamp(min=0)
    if act == "relu6":
        return v.clamp(0, 6)
    if act == "hardswish":
        return v * (v + 3).clamp(0, 6) / 6
    if act == "hardsigmoid":
        return (v + 3).clamp(0, 6) / 6
    if act == "sigmoid":
        return torch.sigmoid(v)
    assert act is None, act
    return v


def epilogue64(v, a, d, act, terms):
    """(value, bound) of the conv epilogue in float64: v the float64 conv, a its sum of absolute terms, `terms` its chain length."""
    col = lambda t: g64(t).reshape(1, -1, 1, 1)  # noqa: E731
    e = 0
    if d.get("bias") is not None:
        v, a, e = v + col(d["bias"]), a + col(d["bias"]).abs(), e + 1
    if d.get("alpha") is not None:
        v, a, e = v * col(d["alpha"]) + col(d["beta"]), a * col(d["alpha"]).abs() + col(d["beta"]).abs(), e + 2
    if d.get("res") is not None:
        v, a, e = v + g64(d["res"]), a + g64(d["res"]).abs(), e + 1
    return act64(v, act), gamma(terms + e + ACT_ROUNDINGS[act] + 2) * a * LIPSCHITZ[act]


def conv64(x, w, **kw):
    return TF.conv2d(g64(x), g64(w), **kw), TF.conv2d(g64(x).abs(), g64(w).abs(), **kw)


def f64_dw5x5(case, d, ref):
    g = case.g
    v, a = conv64(d["x"], d["w"], stride=g["stride"], padding=2 * g["dilation"], dilation=g["dilation"], groups=g["c"])
    return [("", ref) + epilogue64(v, a, d, g["act"], 25)]


def f64_pw_scaled(case, d, ref):
    g = case.g
    xs = g64(d["x"]) * g64(d["gate"])[:, :, None, None]  # exact: 24 + 24 bits
    v, a = conv64(xs.numpy(), d["w"])
    slices = F.conv1x1_k_slices(g["n"], g["cin"], g["h"], g["w"], g["cout"])[0]
    return [("", ref) + epilogue64(v, a, d, g["act"], g["cin"] + 1 + slices)]


def linear64(x, ex, w, b, act):
    """(value, bound) of act(x w^T + b) in float64 on an input known to within ex."""
    w64 = g64(w)
    v, a = TF.linear(x, w64), TF.linear(x.abs(), w64.abs())
    e = 0
    if b is not None:
        v, a, e = v + g64(b), a + g64(b).abs(), 1
    y = act64(v, act)
    a = a * LIPSCHITZ[act] + (y.abs() if act in ("sigmoid", "hardsigmoid") else 0)  # the gates' outputs are not bounded by A
    return y, gamma(x.shape[1] + e + ACT_ROUNDINGS[act] + 2) * a + LIPSCHITZ[act] * TF.linear(ex, w64.abs())


def f64_se(case, d, ref):
    g = case.g
    x = g64(d["x"])
    pool, pool_a = x.mean((2, 3)), x.abs().mean((2, 3))
    pool_bound = gamma(g["h"] * g["w"] + 2) * pool_a
    scale = x * g64(d["gate"])[:, :, None, None]
    lin, lin_bound = linear64(g64(d["xl"]), torch.zeros(g["rows"], g["k"], dtype=torch.float64), d["wl"], d["bl"], g["act"])
    h1, e1 = linear64(pool, pool_bound, d["w1"], d["b1"], g["gate_act"])
    gate, gate_bound = linear64(h1, e1, d["w2"], d["b2"], g["scale_act"])
    return [("pool", ref["pool"], pool, pool_bound), ("scale", ref["scale"], scale, gamma(2) * scale.abs()), ("linear", ref["linear"], lin, lin_bound),
            ("gate", ref["gate"], gate, gate_bound)]


def f64_conv2d(case, d, ref):
    g = case.g
    v, a = conv64(d["x"], d["w"], stride=g["stride"], padding=g["padding"], dilation=g["dilation"], groups=g["groups"])
    return [("", ref) + epilogue64(v, a, d, g["act"], g["cin"] // g["groups"] * g["kh"] * g["kw"])]


def f64_maxpool(case, d, ref):
    g = case.g
    want = TF.max_pool2d(g64(d["x"]), g["k"], g["stride"], g["padding"], ceil_mode=g["ceil_mode"])
    return [("", ref, want, 0.0)]  # a maximum is exact


def f64_convt(case, d, ref):
    g = case.g
    kw = dict(stride=2, padding=0 if g["k"] == 2 else 1)
    v = TF.conv_transpose2d(g64(d["x"]), g64(d["w"]), **kw)
    a = TF.conv_transpose2d(g64(d["x"]).abs(), g64(d["w"]).abs(), **kw)
    return [("", ref) + epilogue64(v, a, d, g["act"], g["cin"] * (g["k"] * g["k"] // 4) + 4)]


def f64_groupnorm(case, d, ref):
    g = case.g
    x = g64(d["x"])
    eps = float(np.float32(g["eps"]))  # the kernel's eps is the float32 one
    slabs = x.reshape(g["n"], g["groups"], -1)
    mean = slabs.mean(2, keepdim=True)
    rstd = 1 / (slabs.var(2, unbiased=False, keepdim=True) + eps).sqrt()
    if x.numel() // g["groups"] > 1:
        y = TF.group_norm(x, g["groups"], g64(d["weight"]), g64(d["bias"]), eps)
    else:  # one value in all: torch refuses it ("more than 1 value per channel"); the same composition by hand
        y = ((slabs - mean) * rstd).reshape(x.shape)
        y = y if d["weight"] is None else y * g64(d["weight"]).reshape(1, -1, 1, 1)
        y = y if d["bias"] is None else y + g64(d["bias"]).reshape(1, -1, 1, 1)
    a = ((slabs.abs() + mean.abs()) * rstd).reshape(x.shape)
    if d["weight"] is not None:
        a = a * g64(d["weight"]).abs().reshape(1, -1, 1, 1)
    if d["bias"] is not None:
        a = a + g64(d["bias"]).abs().reshape(1, -1, 1, 1)
    return [("", ref, y.clamp(min=0) if g["relu"] else y, gamma(6 + 2) * a)]


def f64_l2norm(case, d, ref):
    x = g64(d["x"])
    y = g64(d["weight"]).reshape(1, -1, 1, 1) * x / x.pow(2).sum(1, keepdim=True).sqrt().clamp(min=case.g["eps"])
    return [("", ref, y, gamma(3 + 2) * y.abs())]


def f64_lateral(case, d, ref):
    from tests import _fpn_ref as PF
    g = case.g
    v, a = conv64(d["x"], d["w"])
    slices = F.conv1x1_k_slices(g["n"], g["cin"], g["h"], g["w"], g["cout"])[0]
    res = PF.nearest(d["top"], (g["h"], g["w"]))  # a gather: exact
    return [("", ref) + epilogue64(v, a, dict(d, res=res), g["act"], g["cin"] + slices)]


def interp64(x, oh, ow):
    """(value, bound) of the bilinear resize of a float64 tensor (N, C, h, w) whose values are float32 numbers."""
    h, w = x.shape[-2:]
    v = TF.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False)
    a = TF.interpolate(x.abs(), size=(oh, ow), mode="bilinear", align_corners=False)
    dy = (x[..., 1:, :] - x[..., :-1, :]).abs().amax((-2, -1), keepdim=True) if h > 1 else torch.zeros_like(x[..., :1, :1])
    dx = (x[..., :, 1:] - x[..., :, :-1]).abs().amax((-2, -1), keepdim=True) if w > 1 else torch.zeros_like(x[..., :1, :1])
    return v, gamma(6 + 2) * a + gamma(3) * ((h + 1) * dy + (w + 1) * dx)


def f64_interp(case, d, ref):
    return [("", ref) + interp64(g64(d["x"]), case.g["oh"], case.g["ow"])]


def f64_gated_up(case, d, ref):
    g = case.g
    xs = g64(d["x"]) * g64(d["gate"])[:, :, None, None]
    u, eu = interp64(xs, g["oh"], g["ow"])
    eu = eu + gamma(1) * TF.interpolate(xs.abs(), size=(g["oh"], g["ow"]), mode="bilinear", align_corners=False)  # the gate product's rounding
    w = g64(d["w"])
    v, a = TF.conv2d(u, w), TF.conv2d(u.abs(), w.abs())
    slices = F.conv1x1_k_slices(g["n"], g["cin"], g["oh"], g["ow"], g["cout"])[0]
    y, bound = epilogue64(v, a, d, None, g["cin"] + slices)
    return [("", ref, y, bound + TF.conv2d(eu, w.abs()))]


VALUE_FAMILIES = {"dw5x5": f64_dw5x5, "pw_scaled": f64_pw_scaled, "se": f64_se, "conv2d": f64_conv2d, "maxpool": f64_maxpool, "convt": f64_convt,
                  "groupnorm": f64_groupnorm, "l2norm": f64_l2norm, "lateral": f64_lateral, "interp": f64_interp, "gated_up": f64_gated_up}


@pytest.mark.parametrize("family", list(VALUE_FAMILIES))
def test_reference_against_float64(family):
    for case in all_cases(family):
        d = FC.inputs(case)
        ref = FC.reference(case, d)
        for name, r, want, bound in VALUE_FAMILIES[family](case, d, ref):
            r = r.numpy() if isinstance(r, torch.Tensor) else r
            assert r.dtype == np.float32, case.id
            close(r, want.numpy(), bound.numpy() if isinstance(bound, torch.Tensor) else np.full(r.shape, bound), f"{case.id} {name}")


def test_argmax_reference_against_float64():
    """The labels equal the float64 ones wherever the best class leads the runner-up by more than both their bounds; a plane and its
    copy are one candidate (of the two the rule takes the first, in float32 as in float64)."""
    from tests import _segmentation_ref as GR
    total = excluded = 0
    for case in all_cases("argmax"):
        g = case.g
        d = FC.inputs(case)
        ref = FC.reference(case, d)
        v, bound = interp64(g64(d["x"]), g["oh"], g["ow"])
        v, bound = v.numpy(), bound.numpy()
        assert np.array_equal(GR.argmax_rule(v.astype(np.float32)), np.argmax(v.astype(np.float32), axis=1)), case.id
        if g["dup"] >= 0:
            # the last plane is a copy of an earlier one: by argmax_rule it never wins (a later class wins only when it is greater), so
            # the candidates are the other planes (torch's float64 loops round the two planes apart in the last bit)
            assert not (ref == g["classes"] - 1).any(), case.id
            v = v[:, :-1]
        want = np.argmax(v, axis=1)  # the first maximum: argmax_rule on finite data
        rest = v.copy()
        np.put_along_axis(rest, want[:, None], -np.inf, axis=1)
        margin = v.max(axis=1) - rest.max(axis=1)
        decided = margin > 2 * bound.max(axis=1)
        assert np.array_equal(ref[decided], want[decided]), f"{case.id}: {int((ref != want)[decided].sum())} decided labels differ"
        total += decided.size
        excluded += int((~decided).sum())
    assert excluded <= 0.01 * total, (excluded, total)


# ---- the RoI operators: the float32 restatements against an independent float64 composition -----------------------------------------
# Not the restatements run in float64 (an error in them would show on both sides): the averaging ops as two matrices of summed
# bilinear weights per roi, one per axis, around the plane (torch.einsum); the pools from explicit integer windows with torch's max
# and mean.
def _axis_weights(start, size, bins, grid, extent):
    """(bins, extent) float64: for every bin the sum over its `grid` samples of the two bilinear weights along one axis -- sample
    (p, i) at start + p size / bins + (i + 0.5) size / (bins grid), no weight outside [-1, extent], clamped into [0, extent - 1]."""
    if grid <= 0:
        return torch.zeros(bins, extent, dtype=torch.float64)
    p, i = torch.arange(bins, dtype=torch.float64)[:, None], torch.arange(grid, dtype=torch.float64)[None, :]
    pos = start + p * (size / bins) + (i + 0.5) * (size / bins) / grid
    valid = ((pos >= -1) & (pos <= extent)).double()
    pos = pos.clamp(min=0)
    low = pos.floor().clamp(max=extent - 1)
    pos = torch.where(low >= extent - 1, low, pos)
    high = (low + 1).clamp(max=extent - 1)
    upper = pos - low
    w = torch.zeros(bins, grid, extent, dtype=torch.float64)
    w.scatter_add_(2, low.long()[..., None], ((1 - upper) * valid)[..., None])
    w.scatter_add_(2, high.long()[..., None], (upper * valid)[..., None])
    return w.sum(1)


def roi_align64(x, rois, out, scale, ratio, aligned, position_sensitive):
    """roi_align (aligned or not) and ps_roi_align of a float64 tensor x (N, C, H, W) -> numpy (K, C or C / bins, PH, PW)."""
    n, c, h, w = x.shape
    ph_n, pw_n = out
    result = []
    for roi in rois:
        offset = 0.5 if aligned else 0.0
        x1, y1, x2, y2 = (float(v) * scale - offset for v in roi[1:])
        roi_w, roi_h = x2 - x1, y2 - y1
        if not aligned:
            roi_w, roi_h = max(roi_w, 1.0), max(roi_h, 1.0)
        grid_h = ratio if ratio > 0 else int(np.ceil(roi_h / ph_n))
        grid_w = ratio if ratio > 0 else int(np.ceil(roi_w / pw_n))
        count = float(grid_h * grid_w) if position_sensitive else float(max(grid_h * grid_w, 1))
        ay, ax = _axis_weights(y1, roi_h, ph_n, grid_h, h), _axis_weights(x1, roi_w, pw_n, grid_w, w)
        with np.errstate(invalid="ignore", divide="ignore"):
            full = torch.einsum("ph,chw,qw->cpq", ay, x[int(roi[0])], ax).numpy() / np.float64(count)  # 0 / 0: NaN, as the reference
        if position_sensitive:  # output channel co of bin (p, q) reads input channel (co PH + p) PW + q
            full = np.stack([np.stack([full[:, p, q].reshape(-1, ph_n, pw_n)[:, p, q] for q in range(pw_n)], -1) for p in range(ph_n)], -2)
        result.append(full)
    return np.stack(result)


def _round_half_away(v):
    return int(np.copysign(np.floor(abs(v) + 0.5), v))


def roi_pool64(x, rois, out, scale, position_sensitive):
    """roi_pool -> (max, argmax, the maximum is unique) and ps_roi_pool -> (mean, None, None) of a float64 tensor, window by window."""
    n, c, h, w = x.shape
    ph_n, pw_n = out
    c_out = c // (ph_n * pw_n) if position_sensitive else c
    y = np.zeros((len(rois), c_out, ph_n, pw_n))
    arg, unique = np.full(y.shape, -1, np.int64), np.ones(y.shape, bool)
    for k, roi in enumerate(rois):
        plane = x[int(roi[0])]
        x1, y1, x2, y2 = (_round_half_away(float(v) * scale) for v in roi[1:])
        extra = 0 if position_sensitive else 1
        roi_w, roi_h = max(x2 - x1 + extra, 1), max(y2 - y1 + extra, 1)
        for p in range(ph_n):
            for q in range(pw_n):
                if position_sensitive:
                    rows = int(np.floor(p * roi_h / ph_n + y1)), int(np.ceil((p + 1) * roi_h / ph_n + y1))
                    cols = int(np.floor(q * roi_w / pw_n + x1)), int(np.ceil((q + 1) * roi_w / pw_n + x1))
                else:
                    rows = int(np.floor(p * roi_h / ph_n)) + y1, int(np.ceil((p + 1) * roi_h / ph_n)) + y1
                    cols = int(np.floor(q * roi_w / pw_n)) + x1, int(np.ceil((q + 1) * roi_w / pw_n)) + x1
                (r0, r1), (c0, c1) = (np.clip(rows, 0, h), np.clip(cols, 0, w))
                if r1 <= r0 or c1 <= c0:
                    continue  # an empty bin: 0 and -1
                if position_sensitive:
                    channels = torch.arange(c_out) * (ph_n * pw_n) + p * pw_n + q
                    y[k, :, p, q] = plane[channels, r0:r1, c0:c1].mean((1, 2)).numpy()
                    continue
                flat = plane[:, r0:r1, c0:c1].reshape(c, -1)
                best, pos = flat.max(1)  # torch: the first of several maxima
                y[k, :, p, q] = best.numpy()
                arg[k, :, p, q] = ((r0 + pos // (c1 - c0)) * w + c0 + pos % (c1 - c0)).numpy()
                unique[k, :, p, q] = ((flat == best[:, None]).sum(1) == 1).numpy()
    return (y, None, None) if position_sensitive else (y, arg, unique)


def roi64(case, x, rois):
    g = case.g
    out = (g["ph"], g["pw"])
    if g["op"] in ("roi_align", "ps_roi_align"):
        ps = g["op"] == "ps_roi_align"
        return roi_align64(x, rois, out, g["scale"], g["ratio"], True if ps else g["aligned"], ps), None, None
    return roi_pool64(x, rois, out, g["scale"], g["op"] == "ps_roi_pool")


def test_roi_reference_against_float64():
    """Values within the bound, NaN in equal places; an output may miss only where the float64 result itself jumps under a relative
    change of 2^-21 of the box (a sample on the border of the map, a bin edge on a pixel, roi_h / ph an integer), and at most 1 % do.
    roi_pool's argmax equals the float64 one wherever the value does and the maximum is unique; the channel mappings are equal."""
    total = excluded = 0
    for case in all_cases("roi"):
        g = case.g
        d = FC.inputs(case)
        if not g["rois"]:
            continue
        got = FC.reference(case, d)
        ref, second = got if isinstance(got, tuple) else (got, None)
        x64, rois = g64(d["x"]), d["rois"].astype(np.float64)
        moved = []
        for f in (1.0, 1 + 2.0 ** -21, 1 - 2.0 ** -21):
            r = rois.copy()
            r[:, 1:] *= f
            moved.append(roi64(case, x64, r))
        want, want_arg, unique = moved[0]
        assert ref.dtype == np.float32 and ref.shape == want.shape, (case.id, ref.shape, want.shape)
        xmax, cmax = float(np.abs(d["x"]).max()), float(np.abs(rois[:, 1:]).max()) * g["scale"]
        if g["op"] == "roi_pool":
            bound = 0.0
        elif g["op"] == "ps_roi_pool":
            bound = gamma(g["h"] * g["w"] + 4) * xmax
        else:
            samples = g["ratio"] ** 2 if g["ratio"] > 0 else (int(np.ceil(cmax + 2)) + 1) ** 2
            bound = (gamma(4 * samples + 12) + 4 * gamma(8) * (cmax + 2)) * xmax
        with np.errstate(invalid="ignore"):
            ok = (np.abs(ref.astype(np.float64) - want) <= bound) | (np.isnan(ref) & np.isnan(want))
            jumps = np.zeros(ok.shape, bool)
            for m, _, _ in moved[1:]:
                jumps |= ~((np.abs(m - want) <= bound + 8 * xmax * 2.0 ** -21 * (cmax + 2)) | (np.isnan(m) & np.isnan(want)))
        assert not (~ok & ~jumps).any(), f"{case.id}: {int((~ok & ~jumps).sum())} of {ok.size} outputs outside the bound away from any jump"
        if g["op"] == "roi_pool":
            decided = ok & unique
            assert second.dtype == np.int32 and np.array_equal(second[decided], want_arg[decided]), f"{case.id}: argmax"
            assert decided.mean() > 0.99, case.id
        elif second is not None:
            c_out = g["c"] // (g["ph"] * g["pw"])
            mapping = np.arange(c_out * g["ph"] * g["pw"]).reshape(1, c_out, g["ph"], g["pw"])
            assert np.array_equal(second, np.broadcast_to(mapping, second.shape)), f"{case.id}: channel mapping"
        total += ok.size
        excluded += int((~ok).sum())
    assert total > 10000 and excluded <= 0.01 * total, (excluded, total)


# ---- nms: the kept indices from the float64 IoU matrix --------------------------------------------------------------------------------
def nms64(boxes, scores, thr):
    from tests import _detect_ref as DR
    iou = DR.iou_matrix64(boxes)[0]
    suppressed = np.zeros(len(boxes), bool)
    keep = []
    with np.errstate(invalid="ignore"):
        for i in np.argsort(-scores, kind="stable"):
            if not suppressed[i]:
                keep.append(i)
                suppressed |= iou[i] > thr  # a NaN (0 / 0) suppresses nothing, as in the float32 loop
    return np.asarray(keep, np.int64)


def test_nms_reference_against_float64():
    from tests import _detect_ref as DR
    for case in all_cases("nms"):
        d = FC.inputs(case)
        boxes, scores, thr = d["boxes"], d["scores"], case.g["thr"]
        assert DR.tie_margin_ok(boxes, thr), case.id  # no decision rests on float32 against float64 rounding: nothing is excluded
        ref = FC.reference(case, d)
        if "idxs" in d:
            idxs = d["idxs"]
            kept = np.concatenate([np.flatnonzero(idxs == c)[nms64(boxes[idxs == c], scores[idxs == c], thr)] for c in range(case.g["classes"])])
            want = kept[np.lexsort((kept, -scores[kept]))]
        else:
            want = nms64(boxes, scores, thr)
        assert ref.tolist() == want.tolist(), case.id
    some = [c for c in all_cases("nms") if c.g["boxes"] > 100 and c.g["kind"] == "clustered" and c.g["thr"] == 0.5]
    assert some and all(0 < len(FC.reference(c, FC.inputs(c))) < c.g["boxes"] for c in some)  # boxes are suppressed, and not all


# ---- paste and keypoints: the stated bounds against the replicas ----------------------------------------------------------------------
def test_paste_reference_against_the_replica():
    from tests import _mask_ref as M
    empty = pasted = 0
    for case in all_cases("paste"):
        g = case.g
        d = FC.inputs(case)
        ref = FC.reference(case, d)
        ints, ok = M.expanded_boxes(d["boxes"], g["m"], g["padding"])
        assert ok.all(), case.id
        bound = M.paste_bound(g["m"], g["padding"], float(d["masks"].max()))
        for i, (bx0, by0, bx1, by1) in enumerate(ints.tolist()):
            x0, x1, y0, y1 = max(bx0, 0), min(bx1 + 1, g["w"]), max(by0, 0), min(by1 + 1, g["h"])
            if x0 >= x1 or y0 >= y1:  # wholly outside: the reference raises or wraps around, the library writes zeros
                assert not ref[i].any(), (case.id, i)
                empty += 1
                continue
            want = M.paste_masks_in_image(torch.from_numpy(d["masks"][i:i + 1]), torch.from_numpy(d["boxes"][i:i + 1]), (g["h"], g["w"]), g["padding"]).numpy()
            inside = np.zeros((g["h"], g["w"]), bool)
            inside[y0:y1, x0:x1] = True
            assert not ref[i, 0][~inside].any() and not want[0, 0][~inside].any(), (case.id, i)
            worst = float(np.abs(ref[i].astype(np.float64) - want[0]).max())
            assert worst <= bound, (case.id, i, worst, bound)
            pasted += 1
    assert empty >= len(all_cases("paste")) and pasted >= 6 * len(all_cases("paste"))


def test_keypoints_reference_against_the_replica():
    from tests import _keypoint_ref as KR
    total = excluded = 0
    for case in all_cases("keypoints"):
        g = case.g
        d = FC.inputs(case)
        maps, rois = torch.from_numpy(d["maps"]), torch.from_numpy(d["rois"])
        got_xy, got_scores, roi_maps = KR.keypoints(d["maps"], d["rois"], with_maps=True)
        want_xy, want_scores = KR.heatmaps_to_keypoints(maps, rois)
        bound = KR.bicubic_bound(g["mh"], g["mw"], float(np.abs(d["maps"]).max()))
        for i in range(g["rois"]):
            ok, _, _, rw, rh = KR.roi_geometry(d["rois"][i])
            assert ok, (case.id, i)
            theirs = TF.interpolate(maps[i][:, None], size=(rh, rw), mode="bicubic", align_corners=False)[:, 0].numpy()
            assert float(np.abs(roi_maps[i].astype(np.float64) - theirs).max()) <= bound, (case.id, i)
            flat = np.sort(theirs.reshape(g["k"], -1), axis=1)
            for j in range(g["k"]):
                total += 1
                if rw * rh == 1 or float(flat[j, -1]) - float(flat[j, -2]) > 2 * bound:
                    np.testing.assert_array_equal(got_xy[i, j], want_xy[i, j].numpy(), err_msg=f"{case.id} roi {i} keypoint {j}")
                else:
                    excluded += 1
        assert float(np.abs(got_scores - want_scores.numpy()).max()) <= bound, case.id
    assert excluded <= 0.01 * total, (excluded, total)
