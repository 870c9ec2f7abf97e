"""tests/test_gpu_special_values.py cannot pass vacuously (runs without a GPU): for every case of tests/_special_value_cases.py the
ORACLE ALONE, on the inputs the GPU test will use, gives

  placement   at least one NaN, at least one +Inf or -Inf, and at least half of the outputs finite;
  subnormal   at least a quarter of the non-zero outputs subnormal;
  overflow    at least one Inf and at least half of the outputs finite.

These are conditions on the inputs (sites and scales are chosen to meet them), not tolerances.  Where torch has a CPU op of the
same semantics (conv2d, linear, adaptive_avg_pool2d, ...) the oracle's NaN, +Inf and -Inf positions equal torch's on the same
inputs; and the helper's footprint(), which is geometry alone, is checked against the oracle: one NaN at a site turns exactly
the footprint into NaN (every weight of these cases is non-zero, and NaN passes every activation)."""
import numpy as np
import pytest

from tests import _special_values as S
from tests._special_value_cases import COLOR_CASES, FILTER_CASES, LAYER_CASES, SAMPLING_CASES

CASES = list(LAYER_CASES) + list(FILTER_CASES) + list(SAMPLING_CASES) + list(COLOR_CASES)


def _first(y):
    return y[0] if isinstance(y, tuple) else y


def _outputs(y):
    """The outputs of an op as one array for the conditions (Gaussian + Sobel has two: gx need not overflow where gy does)."""
    return (np.concatenate([v.ravel() for v in y]),) if isinstance(y, tuple) else (y,)


def test_ids_are_unique_and_every_family_is_there():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    assert {c.family for c in CASES} >= {"conv3x3", "conv3x3_u8norm", "linear", "stem", "depthwise", "pointwise", "avgpool", "conv2d", "conv2d_affine", "transpose2x2", "transpose4x4", "deform", "invres"}


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_placement_case_is_not_vacuous(case):
    d = case.placement_inputs()
    want = case.oracle(d)
    for y in _outputs(want):
        S.placement_conditions(y, case.id, inf=case.inf_reaches_output)
    if case.poison and "pair_a" in case.sites:
        sites = case.placement_sites
        assert list(sites)[:2] == ["pair_a", "pair_b"], (case.id, sites)
        assert d[case.poison][tuple(sites["pair_a"])] == np.inf and d[case.poison][tuple(sites["pair_b"])] == -np.inf  # Inf - Inf in one field
    if case.torch_ref is not None:
        theirs = case.torch_ref(d)
        ours = _first(want)
        assert theirs.shape == ours.shape
        for name, f in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
            assert np.array_equal(f(ours), f(theirs)), f"{case.id}: the oracle's {name} positions differ from torch's at {int((f(ours) != f(theirs)).sum())} outputs"


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_range_cases_are_not_vacuous(case):
    d = case.range_inputs("subnormal")
    for y in _outputs(case.oracle(d)):
        S.subnormal_conditions(y, case.id, inputs=None if case.subnormal_outputs else d["x"])
        assert np.array_equal(np.isfinite(y), np.isfinite(_outputs(case.want_clean)[0])), case.id  # (the pole column of a perspective is NaN)
    if case.overflow:
        for y in _outputs(case.oracle(case.range_inputs("overflow"))):
            S.overflow_conditions(y, case.id)


@pytest.mark.parametrize("case", [c for c in CASES if c.poison], ids=repr)
def test_footprint_is_where_the_oracle_spreads_a_nan(case):
    """footprint() against the oracle: one NaN at a site -> NaN exactly on the footprint.  This is a check of the helper (and of
    the sites: each lies inside the tensor and reaches at least one output), made where a GPU is not needed."""
    clean = _first(case.want_clean)
    base = np.isnan(clean)  # all False, but for the perspective whose denominator is 0 along a column: NaN coordinates, NaN samples
    assert np.isfinite(clean[~base]).all() and base.mean() < 0.1
    assert sum(bool(S.footprint(site, case.geometry).any()) for site in case.sites.values()) >= 3, case.sites
    for name, site in case.sites.items():
        mask = S.footprint(site, case.geometry)
        assert mask.shape == clean.shape, (case.id, name)
        got = _first(case.oracle(case.with_site(site, S.NAN)))
        assert np.array_equal(np.isnan(got), mask | base), (case.id, name, site)
        S.assert_local(clean, got, mask, f"{case.id} {name}")


def test_cases_take_the_plans_their_rows_state():
    """(Needs the built library, like tests/test_layer_guard_cases_host.py: the plan queries are host-only entry points of
    libmi355vision.so and run without a GPU.)  Rows that run at another batch than tests/_layer_guard_cases.py states (one output pixel per image: batch 4) keep the
    plan the row is there for: the pointwise rows their K slices, the generic conv rows the optional workspace."""
    from cpu_vision_amd import _lib, functional as F
    lib = _lib.load()
    for c in CASES:
        if c.family == "pointwise":
            n, cin, h, w = c.geometry["in_shape"]
            slices, sl = F.conv1x1_k_slices(n, cin, h, w, c.geometry["cout"])
            assert (sl if slices > 1 else 0) == c.plan["slice"], c.id
            assert (f",ks{slices}>" in "".join(c.kernel)) == (slices > 1), c.id
        if c.family == "conv2d":
            n, cin, h, w = c.geometry["in_shape"]
            g = c.geometry
            assert lib.mv_conv2d_needs_workspace(n, cin, g["cout"], h, w, *g["k"], *g["stride"], *g["pad"], *g["dil"], g["groups"]) == 2, c.id


# ---- the helper itself ----------------------------------------------------------------------------------------------------------------
def test_assert_same_values_semantics():
    a = np.array([1.0, np.nan, np.inf, -np.inf, 0.0], np.float32)
    S.assert_same_values(a, a.copy())
    S.assert_same_values(np.array([-0.0], np.float32), np.array([0.0], np.float32))  # the sign of a zero is not asserted
    for bad in ([1.0, 0.0, np.inf, -np.inf, 0.0], [1.0, np.nan, -np.inf, -np.inf, 0.0], [np.nextafter(np.float32(1), np.float32(2)), np.nan, np.inf, -np.inf, 0.0],
                [np.nan, np.nan, np.inf, -np.inf, 0.0]):
        with pytest.raises(AssertionError):
            S.assert_same_values(np.array(bad, np.float32), a)
    with pytest.raises(AssertionError):
        S.assert_same_values(a.astype(np.float64), a)


def test_assert_local_semantics():
    clean = np.zeros((2, 3), np.float32)
    mask = np.zeros((2, 3), bool)
    mask[0, 1] = True
    dirty = clean.copy()
    dirty[0, 1] = np.nan
    S.assert_local(clean, dirty, mask)
    with pytest.raises(AssertionError, match="outside"):
        leak = dirty.copy()
        leak[1, 2] = -0.0  # a flipped sign bit outside the footprint is a leak: bit-identical means bits
        S.assert_local(clean, leak, mask)
    with pytest.raises(AssertionError, match="inside"):
        S.assert_local(clean, clean.copy(), mask)


def test_footprint_restates_small_geometries_by_hand():
    g = dict(op="conv", in_shape=(1, 4, 5, 5), cout=6, k=(3, 3), stride=(2, 2), pad=(1, 1), dil=(1, 1), groups=2)
    m = S.footprint((0, 3, 4, 0), g)  # channel 3 = group 1 -> outputs 3..5; row 4 -> output row 2 only; column 0 -> output column 0
    want = np.zeros((1, 6, 3, 3), bool)
    want[0, 3:, 2, 0] = True
    assert np.array_equal(m, want)
    f = dict(op="filter", in_shape=(2, 6, 7), k=(5, 5), border="reflect")
    m = S.footprint((1, 1, 0), f)  # row 1 is read by rows 0..3 directly and by row 0 again through the mirror (-1 -> 1)
    assert m[1, :4, :3].all() and not m[0].any() and not m[1, 4:].any() and not m[1, :, 3:].any()
    assert not S.footprint((1, 1, 0), dict(f, border="zero"))[1, 4:, :].any()
    v = S.footprint((0, 0, 0), dict(f, border="valid"))
    assert v.shape == (2, 2, 3) and v.sum() == 1 and v[0, 0, 0]
    p = S.footprint((0, 6, 6), dict(op="avgpool", in_shape=(1, 14, 14), out=(7, 7)))
    assert p.sum() == 1 and p[0, 3, 3]
    t = S.footprint((0, 0, 1, 1), dict(op="transpose", in_shape=(1, 2, 3, 3), cout=2, k=4, stride=2, pad=1))
    assert t.shape == (1, 2, 6, 6) and t[0, 0, 1:5, 1:5].all() and t.sum() == 2 * 16
