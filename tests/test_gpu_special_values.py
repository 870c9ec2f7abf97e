"""NaN, Inf, subnormal and huge inputs through the arithmetic kernels (`-m gpu`).  Almost every other GPU test draws its data from
[-1, 1), [0, 1) or [0, 255]; the kernels that carry the workloads pad K chunks, channel tiles, ragged edges and stacked images, and
where such padding is cancelled by a zero operand instead of a select, 0 x Inf = NaN reaches outputs that never saw the value.
Every case of tests/_special_value_cases.py (whose oracle results tests/test_special_values_host.py proves non-vacuous without a
GPU) runs three checks and asserts the kernel it was written for (mv_last_kernel):

  placement  +Inf, -Inf and NaN at the sites of tests/_special_values.poison_sites -- a +Inf and a -Inf inside one receptive
             field, so that Inf - Inf occurs -- and one non-finite entry in bias, alpha, beta and residual where the shape leaves
             room: the result has the oracle's values (assert_same_values: NaN positions, then ==);
  locality   without the oracle: for each site alone, NaN in one parametrisation and +Inf in the other, the outputs outside the
             site's footprint (geometry only) are bit-identical to the clean run's, and inside it at least one differs;
  range      inputs scaled until the outputs are subnormal, and until some chains overflow: both bit for bit the oracle (MFMA
             operands follow MODE.denorm; a flushed subnormal or a sum that overflows elsewhere than in the stated order shows).

Weights stay finite: a zero-padded tap times an Inf weight has no agreed meaning.  Families: the 3 x 3 conv, linear, the
conv_norm_act kernels, the average pools, the fused InvertedResidual block, the generic conv (implicit and columns form, and with
the full epilogue), the two transposed convs, the deformable conv, and the filters (blur, separable blur, Gaussian + Sobel,
sharpness, the depthwise primitive; float32, float64, float16, bfloat16; the frame-list entries), the sampling ops (affine,
rotate, perspective -- one with a pole inside the output --, elastic; bilinear and nearest; the antialiased resize in both
forms) and the float32 colour ops (the chain, autocontrast, normalize).  What these cases found and what was fixed: DESIGN.md
section 4.2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, functional as F, ops  # noqa: E402
from tests import _special_values as S  # noqa: E402
from tests._special_value_cases import COLOR_CASES, FILTER_CASES, LAYER_CASES, SAMPLING_CASES  # noqa: E402

CASES = list(LAYER_CASES) + list(FILTER_CASES) + list(SAMPLING_CASES) + list(COLOR_CASES)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def image(c, d):
    """x in the case's storage type (bfloat16 values travel as float32 arrays: the conversion is exact)."""
    x = dev(d["x"])
    return x.to(torch.bfloat16) if c.dtype == "bfloat16" else x


def host(t):
    if isinstance(t, (tuple, list)):
        return tuple(host(v) for v in t)
    t = t.detach().cpu()
    return (t.float() if t.dtype == torch.bfloat16 else t).numpy()


# ---- one launch per family ----------------------------------------------------------------------------------------------------------------
def _conv3x3(c, d):
    return F.conv2d_bias_relu(dev(d["x"]), dev(d["w"]), dev(d["b"]), relu=c.call["relu"])


def _conv3x3_u8norm(c, d):
    from tests._special_value_cases import U8_MEAN, U8_STD
    return F.normalized_conv2d_bias_relu(dev(d["x"]), U8_MEAN, U8_STD, dev(d["w"]), dev(d["b"]), relu=False)


def _linear(c, d):
    return F.linear_bias_relu(dev(d["x"]), dev(d["w"]), dev(d["b"]), relu=c.call["relu"])


def _conv_norm_act(c, d):
    return F.conv_norm_act(dev(d["x"]), dev(d["w"]), dev(d["bias"]), dev(d["alpha"]), dev(d["beta"]), dev(d["residual"]), **c.call)


def _avgpool(c, d):
    return F.adaptive_avg_pool2d(dev(d["x"]), c.call["out"])


def _conv2d(c, d):
    return F.conv2d_bias_act(dev(d["x"]), dev(d["w"]), dev(d["b"]), **c.call)


def _conv2d_affine(c, d):
    return F.conv2d_affine_act(dev(d["x"]), dev(d["w"]), dev(d["bias"]), dev(d["alpha"]), dev(d["beta"]), dev(d["residual"]), **c.call)


def _transpose(c, d):
    return F.conv_transpose2d_bias_act(dev(d["x"]), dev(d["w"]), dev(d["b"]), c.call["activation"], padding=c.call["padding"])


def _deform(c, d):
    kw = {k: v for k, v in c.call.items() if k != "columns"}
    return ops.deform_conv2d(dev(d["x"]), dev(d["offset"]), dev(d["w"]), dev(d["b"]), mask=dev(d["mask"]), **kw)


def _invres(c, d):
    from tests._special_value_cases import INVRES_NAMES
    return F.inverted_residual(dev(d["x"]), *[dev(d[n]) for n in INVRES_NAMES], residual=c.call["residual"], stride=c.call["stride"],
                               affine=c.call["affine"])


def _frames(x):
    """Separately allocated frames, as a DataLoader hands them to a transform."""
    return [x[i].clone() for i in range(x.shape[0])]


def _blur(c, d):
    x = image(c, d)
    if c.call["frames"]:
        return torch.stack(F.gaussian_blur_frames(_frames(x), c.call["kernel_size"]))
    fn = F.separable_gaussian_blur if c.family == "sepblur" else F.gaussian_blur_image
    return fn(x, c.call["kernel_size"])


def _depthwise_conv2d(c, d):
    return F.depthwise_conv2d(image(c, d), torch.from_numpy(np.array(d["w"])), c.call["border"])


def _gaussian_sobel(c, d):
    return F.gaussian_sobel(image(c, d), c.call["kernel_size"])


def _sharpness(c, d):
    x = image(c, d)
    if c.call["frames"]:
        return torch.stack(F.adjust_sharpness_frames(_frames(x), c.call["factor"]))
    return F.adjust_sharpness_image(x, c.call["factor"])


def _warp(c, d):
    x = dev(d["x"])
    op = c.call["op"]
    if op == "elastic":
        return F.elastic(x, dev(c.call["field"]), interpolation=c.call["mode"])
    return getattr(F, op)(x, interpolation=c.call["mode"], **c.call["args"])


def _resize(c, d):
    from cpu_vision_amd import functional_v1 as F1
    return F1.resize(dev(d["x"]), c.call["size"])


def _color(c, d):
    return F.color_jitter_image(dev(d["x"]), c.call["ops"])


def _autocontrast(c, d):
    return F.autocontrast_image(dev(d["x"]))


def _normalize(c, d):
    return F.normalize(dev(d["x"]), c.call["mean"], c.call["std"])


LAUNCH = {"conv3x3": _conv3x3, "conv3x3_u8norm": _conv3x3_u8norm, "linear": _linear, "stem": _conv_norm_act, "depthwise": _conv_norm_act,
          "pointwise": _conv_norm_act, "avgpool": _avgpool, "conv2d": _conv2d, "conv2d_affine": _conv2d_affine, "transpose2x2": _transpose, "transpose4x4": _transpose, "deform": _deform, "invres": _invres,
          "blur": _blur, "sepblur": _blur, "blur_v": _blur, "depthwise_conv2d": _depthwise_conv2d, "gaussian_sobel": _gaussian_sobel,
          "sharpness": _sharpness, "sharpness_v": _sharpness, "warp": _warp, "elastic": _warp, "resize": _resize, "color": _color,
          "autocontrast": _autocontrast, "normalize": _normalize}


def _assert_kernel(case, what):
    kernel = _lib.last_kernel()
    expected = case.kernel
    if callable(expected):
        assert expected(kernel), (what, kernel)
    elif expected == "k_conv3x3":
        assert kernel.startswith("k_conv3x3<"), (what, kernel)  # k_conv3x3<ks0>, <ks5>, <ks14[,fullw]>: not _gen, not _c3
    elif isinstance(expected, tuple):
        assert kernel.startswith(expected[0]) and all(part in kernel for part in expected[1:]), (what, kernel, expected)
    elif expected.startswith(("k_dwpc3x3", "k_global", "k_adaptive", "k_sharp", "k_dw3x3", "k_to_float")):
        assert kernel == expected, (what, kernel, expected)
    else:
        assert expected in kernel, (what, kernel, expected)


def _run(case, d, what):
    got = host(LAUNCH[case.family](case, d))
    _assert_kernel(case, f"{case.id} {what}")
    if case.family == "invres":
        assert _lib.last_kernel().endswith("+k_invres_reduce") == (case.call["slices"] > 1), (case.id, _lib.last_kernel())
    return got


@pytest.fixture
def library(request, monkeypatch):
    """The library a case runs on: the tuning build with the case's MV_* knobs set where it has any (as tests/test_gpu_cnn.py
    does), else the product library; and the case's module switches of `functional`."""
    def enter(case):
        for k, v in case.switches.items():
            monkeypatch.setattr(F, k, v)
        if case.family == "deform":  # the columns form (a workspace) where the row can take either; the fused kernel otherwise
            monkeypatch.setattr(ops, "FUSED_WHENEVER_POSSIBLE", not case.call["columns"])
        if case.env:
            for k, v in case.env.items():
                monkeypatch.setenv(k, v)
            request.getfixturevalue("tuning_library")
    return enter


def _flat(y):
    return np.concatenate([v.ravel() for v in y]) if isinstance(y, tuple) else y


def _pairs(got, want):
    got, want = (got if isinstance(got, tuple) else (got,)), (want if isinstance(want, tuple) else (want,))
    assert len(got) == len(want)
    return list(zip(got, want))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_placement(case, library):
    library(case)
    d = case.placement_inputs()
    want = case.oracle(d)
    got = _run(case, d, "placement")
    S.placement_conditions(_flat(want), case.id, inf=case.inf_reaches_output)
    for i, (g, w) in enumerate(_pairs(got, want)):
        S.assert_same_values(g, w, f"{case.id} placement, output {i}; sites {case.placement_sites}")


@pytest.mark.parametrize("value", [S.NAN, S.PINF], ids=["nan", "inf"])
@pytest.mark.parametrize("case", [c for c in CASES if c.poison], ids=repr)
def test_locality(case, value, library):
    library(case)
    clean = _run(case, case.clean, "clean")
    for name, site in case.sites.items():
        mask = S.footprint(site, case.geometry)
        dirty = _run(case, case.with_site(site, value), f"{name} = {value}")
        for i, (cl, di) in enumerate(_pairs(clean, dirty)):
            S.assert_local(cl, di, mask, f"{case.id}: {value} at {name} {site}, output {i}")


@pytest.mark.parametrize("case,run", [(c, r) for c in CASES for r in ("subnormal", "overflow") if r == "subnormal" or c.overflow],
                         ids=lambda v: repr(v) if not isinstance(v, str) else v)
def test_range(case, run, library):
    library(case)
    d = case.range_inputs(run)
    want = case.oracle(d)
    got = _run(case, d, run)
    if run == "subnormal":
        S.subnormal_conditions(_flat(want), case.id, inputs=None if case.subnormal_outputs else d["x"])
    else:
        S.overflow_conditions(_flat(want), case.id)
    for i, (g, w) in enumerate(_pairs(got, want)):
        S.assert_same_values(g, w, f"{case.id} {run} (x * 2^{case.exponents(run)[0]}, products * 2^{case.exponents(run)[1]}), output {i}")
