"""The random-shape sweeps of tests/test_gpu_fuzz_detect.py cannot pass vacuously (runs without a GPU).  For every family of
tests/_fuzz_detect_cases.py:

  reproducible   generating a chunk twice gives the same cases, the ids are unique and carry the geometry and the seed;
  valid          every case passes its entry point's own host path: the public function runs on CPU tensors with the launch replaced
                 by nothing (a level that is only ever materialised on the device is an uninitialised tensor of its shape);
  coverage       conditions on the geometry and on the REFERENCE's keys alone (nothing a kernel produced): every level count
                 1 .. kMaxRpnLevels in every chunk, the sizes around the kernels' steps, every way out of select_keys (select_exit, a
                 restatement of its control flow) for stage 2 and for k_ssd_topk, stage 1's early exit, empty chunk and later passes,
                 both sides of the stage-2 read trip, the rpn's tie counts, tile counts and scan steps, the threshold kinds, the
                 residues of R mod kRoiWaves and of the classes mod kWave;
  independent    the references against a statement of their own.  The selection is exact once the float32 scores are given: numpy's
                 lexsort on (flat index, -score) over the passing scores, the flat index from explicit arithmetic on the memory
                 offset (not permute_level), the level's start added here; for the rpn on the kernel's 32-bit key (NaN greatest,
                 -0 == +0).  The scores and the boxes against torch's float64 within a derived bound; the float64 ORDER against the
                 float32 one wherever the float64 gap exceeds the bounds of both neighbours.

The bounds, with u = 2^-24 and gamma(k) = k u / (1 - k u) (Higham, section 3.1), m = 2^-126 the smallest normal float32:
  sigmoid      1 / (1 + E(-x)): the correctly rounded exp, the sum and the quotient, one rounding each, all on positive terms:
               gamma(3) s; with the float64 side's own roundings gamma(4) s + m (m: E overflows for x < -88.7, the score is 0).
  fcos score   sqrt(s1 s2): the two sigmoids (gamma(3) each) and the product's rounding are halved by the square root, which adds its
               own: gamma(5) s, taken as gamma(6) s + 2^-62 (a product below m loses its relative precision; its root is below 2^-63).
  softmax      e_j = E(x_j - max): the difference's rounding moves the exponent by u |x_j - max| <= u D, D the row's spread, so e_j
               carries (D + 1) u, the float64 sum the same, the quotient one more: gamma(2 D + 4) p + m for mv_ssd_scores_f32; the
               float32 chain of mv_roi_detections_f32 adds gamma(C - 1) for its C - 1 additions.
  decode       BoxCoder.decode_single has at most 7 roundings on the way to a corner and the exponent carries u |dw| <= u clip < 5 u:
               gamma(14) A with A = |x1| + |x2| + |dx| (|x1| + |x2|) + exp(dw) (|x1| + |x2|), the sum of the absolute terms; the clamp to the
               image is 1-Lipschitz.  BoxLinearCoder.decode: 4 roundings, gamma(6) A with A = |x1| + |x2| + r (|x1| + |x2|).  The
               default boxes of SSD add 5 roundings on terms of size (|cx| + |w| / 2) W: their error passes through decode_single
               with the gain 1 + |dx| + exp(dw), taken into A.
A label, a level or a validity flag must be equal wherever the value it rests on is further from its threshold than the bound; the
share excluded by that margin is at most 1 % per family, asserted with the measured share in the message.
"""
import functools

import numpy as np
import pytest
import torch

from cpu_vision_amd import _detection, _lib
from cpu_vision_amd import functional as F
from tests import _fcos_ref as FR
from tests import _fuzz_detect_cases as DC
from tests import _retinanet_ref as RR
from tests import _rpn_ref as P
from tests import _ssd_ref as SR

U = 2.0 ** -24
TINY = 2.0 ** -126
FAMILIES = list(DC.SWEEPS)
F32 = np.float32


def gamma(k):
    return k * U / (1 - k * U)


@functools.lru_cache(maxsize=None)
def all_cases(family):
    return tuple(DC.cases(family))


@functools.lru_cache(maxsize=None)
def data(family):
    """((case, inputs, reference), ...) of a family, computed once."""
    out = []
    for case in all_cases(family):
        d = DC.inputs(case)
        out.append((case, d, DC.reference(case, d)))
    return tuple(out)


# ---- reproducible, unique ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_cases_are_reproducible_and_ids_unique(family):
    first, chunks, count = DC.SWEEPS[family]
    assert first == 2700 + 100 * FAMILIES.index(family) and 2 <= chunks <= 4 and 10 <= count <= 25
    again = DC.cases(family)
    assert list(all_cases(family)) == again and len(again) == chunks * count
    ids = [c.id for c in again]
    assert len(set(ids)) == len(ids)
    for c in again[:3]:
        assert c.id.startswith(f"{family}[sweep {c.sweep} #{c.index}] ") and all(f"{k}={v}" in c.id for k, v in c.geom) and "seed=" in c.id
        rebuilt = DC.Case(c.family, c.sweep, c.index, c.geom)  # a case built by hand from what its id states
        a, b = DC.inputs(c), DC.inputs(rebuilt)
        for k in a:
            va, vb = a[k], b[k]
            for x, y in zip(va if isinstance(va, list) else [va], vb if isinstance(vb, list) else [vb]):
                if isinstance(x, np.ndarray):
                    assert np.array_equal(x, y, equal_nan=True), (c.id, k)


def test_the_constants_come_from_the_sources():
    c = DC.consts()
    assert c["chunk"] == F.retinanet_topk_chunk()
    assert (c["max_levels"], c["max_k"], c["roi_max_classes"]) == (_detection.MAX_RPN_LEVELS, _detection.MAX_RPN_TOPK, _detection.MAX_ROI_CLASSES)
    assert c["rpn_trip"] % c["rpn_step"] == 0 and c["rank_trip"] <= c["max_k"] and c["roi_waves"] * c["wave"] == c["scores_block"]
    assert DC.index_cut(6, 10, 5000) == 256 and DC.index_cut(6, 250, 5000) == 512 and DC.index_cut(5, 0, 1 << 20) == 1 << 16


# ---- valid: the host path of every case ------------------------------------------------------------------------------------------------
def cpu(m, layout="dense"):
    if isinstance(m, DC.Sparse):
        return torch.empty(m.shape)  # never read: the launch is replaced by nothing
    return DC.place(torch.from_numpy(np.ascontiguousarray(m)), layout)


def dry_call(case, d):
    """The public entry point of a case on CPU tensors: everything in front of the launch runs, the launch does not -> (output, shape)."""
    g, fam = case.g, case.family
    lay = g.get("layout", "dense")
    levels = g.get("levels", ())
    if fam in ("rpn_topk", "ret_topk", "fcos_topk"):
        kc = g.get("classes", 1)
        total = sum(min(g["k"], a * h * w * kc) for a, h, w in levels)
        maps = [cpu(m, lay) for m in d["maps"]]
        if fam == "rpn_topk":
            return F.rpn_topk(maps, g["k"]), (g["n"], total)
        if fam == "ret_topk":
            return F.retinanet_topk(maps, kc, g["k"], d["thresh"]), (g["n"], total)
        return F.fcos_topk(maps, [cpu(m, lay) for m in d["ctrs"]], kc, g["k"], d["thresh"]), (g["n"], total)
    if fam in ("rpn_decode", "ret_decode", "fcos_decode"):
        lg, dl, idx = [cpu(m, lay) for m in d["logits"]], [cpu(m, lay) for m in d["deltas"]], torch.from_numpy(d["idx"])
        cells = [torch.from_numpy(c) for c in d["cells"]]
        shape = tuple(d["idx"].shape)
        if fam == "rpn_decode":
            return F.rpn_decode(lg, dl, idx, cells, g["strides"], d["sizes"], g["weights"], DC.CLIP, g["min_size"], g["score_thresh"])[1], shape
        if fam == "ret_decode":
            return F.retinanet_decode(lg, dl, idx, cells, g["strides"], d["sizes"], g["classes"], g["weights"], g["clip"])[1], shape
        return F.fcos_decode(lg, [cpu(m, lay) for m in d["ctrs"]], dl, idx, cells, g["strides"], d["sizes"], g["classes"])[1], shape
    if fam == "ssd_scores":
        return F.ssd_scores([cpu(m, lay) for m in d["maps"]], g["classes"]), (g["n"], g["classes"], int(DC.level_starts(levels)[-1]))
    if fam == "ssd_topk":
        s = torch.empty((g["n"], g["classes"], g["v"])) if isinstance(d["scores"], DC.Sparse) else torch.from_numpy(d["scores"])
        return F.ssd_topk(s, g["k"], d["thresh"]), (g["n"], (g["classes"] - 1) * g["k"])
    if fam == "ssd_decode":
        out = F.ssd_decode(torch.from_numpy(d["scores"]), [cpu(m, lay) for m in d["deltas"]], torch.from_numpy(d["idx"]),
                           [torch.from_numpy(p) for p in d["pairs"]], g["steps"], g["batch"], d["sizes"], g["weights"], g["clip_pairs"])
        return out[1], tuple(d["idx"].shape)
    if fam == "roi_det":
        lg, dl = roi_inputs(d, g["sliced"], lambda t: t)
        return F.roi_detections(lg, dl, torch.from_numpy(d["rois"]), d["sizes"], g["weights"], DC.CLIP, g["score_thresh"], g["min_size"])[1], (g["r"], g["classes"] - 1)
    assert fam == "box_decode", fam
    return F.box_decode(torch.from_numpy(d["boxes"]), torch.from_numpy(d["codes"]), g["weights"], g["clip"]), (g["m"], 4 * g["c"])


def roi_inputs(d, sliced, to):
    """class_logits and box_regression: two tensors, or the column slices of one wider tensor."""
    lg, dl = to(torch.from_numpy(d["logits"])), to(torch.from_numpy(d["deltas"]))
    if not sliced:
        return lg, dl
    both = torch.cat([lg, dl], 1)
    return both[:, :lg.shape[1]], both[:, lg.shape[1]:]


@pytest.mark.parametrize("family", FAMILIES)
def test_cases_pass_the_host_path(family, monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda t, what="input": None)
    monkeypatch.setattr(_lib, "launch", lambda fn, on, *args: None)
    for case, d, ref in data(family):
        out, shape = dry_call(case, d)  # raises where the host path refuses the case
        assert tuple(out.shape) == shape, (case.id, tuple(out.shape), shape)
        first = ref[1] if isinstance(ref, tuple) else ref
        assert tuple(first.shape) == shape, (case.id, first.shape, shape)
        maps = d.get("maps") or d.get("deltas")
        if case.g.get("layout", "dense") != "dense" and not isinstance(maps[0], DC.Sparse):
            m = cpu(maps[0], case.g["layout"])
            assert m.shape[0] == 1 or m.stride(0) > m[0].numel(), case.id  # the image stride is larger than the map
            assert (_detection._dense_images(m).data_ptr() != m.data_ptr()) == (case.g["layout"] == "strided"), case.id  # only that one is copied


# ---- coverage: the geometry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", DC.PYRAMID_FAMILIES)
def test_coverage_pyramids(family):
    cs = all_cases(family)
    top = DC.consts()["max_levels"]
    assert {len(c.g["levels"]) for c in cs} == set(range(1, top + 1))
    for chunk in DC.chunks(family):
        assert any(len(c.g["levels"]) == top for c in DC.cases(family, chunk)), chunk
    shapes = [lv for c in cs for lv in c.g["levels"]]
    assert any(h == w == 1 for _, h, w in shapes) and np.mean([h != w for _, h, w in shapes if h * w > 1]) > 0.5
    several = [[a * h * w for a, h, w in c.g["levels"]] for c in cs if len(c.g["levels"]) > 2]
    assert np.mean([s != sorted(s) and s != sorted(s, reverse=True) for s in several]) > 0.5  # in no order of size
    assert {c.g["n"] for c in cs} == {1, 2, 3}
    layouts = [c.g["layout"] for c in cs]
    assert 0.25 <= layouts.count("slice") / len(cs) <= 0.4 and 1 <= layouts.count("strided") <= len(cs) // 8
    anchors = {a for a, _, _ in shapes}
    assert anchors == {1} if family.startswith("fcos") else ({1, 2, 3} <= anchors and max(anchors) <= 12)
    if "classes" in cs[0].g and family != "rpn_decode":
        classes = {c.g["classes"] for c in cs}
        assert min(classes) == (2 if family.startswith("ssd") else 1) and max(classes) <= 91 and len(classes) >= 5


def _edges_met(values, edges, what):
    missing = [e for e in edges if e not in values]
    assert not missing, (what, missing, sorted(values))


@pytest.mark.parametrize("family", ["rpn_topk", "ret_topk", "fcos_topk", "ssd_topk"])
def test_coverage_topk_sizes(family):
    c = DC.consts()
    cs = all_cases(family)
    _edges_met({x.g["k"] for x in cs}, DC._k_edges(), "k")
    if family == "ssd_topk":
        counts = [x.g["v"] for x in cs]
        steps = DC.around(c["ssd_step"], c["ssd_trip"], 2 * c["ssd_trip"])
    else:
        counts = [np.prod(x.g["levels"][x.g["main"]]) * x.g.get("classes", 1) for x in cs]
        steps = DC.around(c["rpn_step"], c["rpn_trip"], 2 * c["rpn_trip"]) if family == "rpn_topk" else DC.around(c["chunk"], 2 * c["chunk"], 3 * c["chunk"])
    _edges_met(set(counts), steps + [1, 2], "elements")
    rel = {int(np.sign(x.g["k"] - n)) for x, n in zip(cs, counts)}
    assert rel == {-1, 0, 1}
    assert {x.g["k"] - n for x, n in zip(cs, counts)} >= {-1, 0, 1}  # k one below, at and one above the level
    assert [x.g["kind"] for x in cs[:6]] == list(DC.KINDS)


def test_coverage_ssd_scores_roi_det_box_decode():
    c = DC.consts()
    totals = {int(DC.level_starts(x.g["levels"])[-1]) for x in all_cases("ssd_scores")}
    _edges_met(totals, DC.around(c["scores_block"], 2 * c["scores_block"], 3 * c["scores_block"]), "anchors")
    assert {2, 91} <= {x.g["classes"] for x in all_cases("ssd_scores")}
    rs = all_cases("roi_det")
    assert {x.g["r"] % c["roi_waves"] for x in rs} == set(range(c["roi_waves"])) and set(range(10)) <= {x.g["r"] for x in rs}
    _edges_met({x.g["r"] for x in rs}, DC.around(c["roi_waves"], 2 * c["roi_waves"], c["wave"]), "rois")
    _edges_met({x.g["classes"] for x in rs}, [2] + DC.around(c["wave"], 2 * c["wave"], 3 * c["wave"]), "classes")
    assert {0, 1, c["wave"] - 1} <= {x.g["classes"] % c["wave"] for x in rs}
    assert sum(x.g["classes"] == c["roi_max_classes"] for x in rs) == 1 and {x.g["n"] for x in rs} == {1, 2, 3} and {x.g["sliced"] for x in rs} == {False, True}
    seen = set()
    for case, d, ref in data("roi_det"):
        n = case.g["n"]
        for v in d["rois"][:, 0]:
            seen |= {name for name, b in zip(("nan", "-1", "-0.5", "n-0.5", "n"), DC.bad_image_indices(n)) if v == F32(b) or (np.isnan(v) and np.isnan(b))}
    assert seen == {"nan", "-1", "-0.5", "n-0.5", "n"}
    valid = np.concatenate([ref[3].reshape(-1) for _, _, ref in data("roi_det")])
    assert 0.05 < valid.mean() < 0.95  # the flags are mixed
    bs = all_cases("box_decode")
    _edges_met({x.g["m"] for x in bs}, [0, 1, 600] + DC.around(c["scores_block"], 2 * c["scores_block"]), "boxes")
    assert {x.g["c"] for x in bs} == set(range(1, 8))
    for fam in ("rpn_decode", "ret_decode", "fcos_decode", "ssd_decode"):
        for case, d, ref in data(fam):
            total = int(DC.level_starts(case.g["levels"])[-1]) * case.g["classes"]
            assert d["idx"][0, -6:].tolist() == [-1, total, 2 ** 31 - 1, -2 ** 31, 0, total - 1], case.id
            if fam == "rpn_decode":  # its flag also rests on the box and the score; the level tells whether the index was taken
                assert ((ref[2][:, -6:] >= 0) == np.array([False, False, False, False, True, True])).all(), case.id
            else:
                assert ref[3][:, -6:].tolist() == [[False, False, False, False, True, True]] * case.g["n"], case.id
    ssd = all_cases("ssd_decode")
    assert {(x.g["steps"] is None, x.g["clip_pairs"]) for x in ssd} == {(a, b) for a in (False, True) for b in (False, True)}
    assert len({x.g["weights"] for x in ssd}) == 2
    valid = np.concatenate([ref[3].reshape(-1) for _, _, ref in data("rpn_decode")])
    assert 0.1 < valid.mean() < 0.9  # the rpn's flags are mixed


# ---- coverage: the ways through select_keys and k_rpn_topk -------------------------------------------------------------------------------
def onestage_views(case, d):
    """[(stage, exit, take, pool size)] of every workgroup of a ret_topk / fcos_topk case that has a key to look at, and the count of
    stage-1 workgroups without one -- from the reference's float32 scores."""
    g = case.g
    kc, k, thr = g["classes"], g["k"], F32(d["thresh"])
    starts = DC.level_starts(g["levels"])
    views, empty = [], 0
    for l, (a, h, w) in enumerate(g["levels"]):
        count, hw = a * kc * h * w, h * w
        chunks = -(-count // DC.consts()["chunk"])
        if l == g["main"] and d["sparse"] is not None:
            per_image = [(d["sparse"]["flat"], d["sparse"]["scores"])]  # the same in every image
        else:
            s = DC.level_flat_scores(case.family, d, g, l)
            per_image = [(int(starts[l]) * kc + np.arange(count), s[i]) for i in range(g["n"])]
        for f, s in per_image:
            with np.errstate(invalid="ignore"):
                ok = s > thr
            keys = DC.score_keys(s[ok], f[ok], np.ones(int(ok.sum()), bool))
            exits, pool = DC.stage1_views(keys, DC.mem_of_flat(f[ok], hw, a, kc, int(starts[l])), k)
            views += [(1,) + e + (0,) for e in exits]
            empty += chunks - len(exits)
            views.append((2,) + DC.select_exit(pool, k) + (len(pool),))
    return views, empty


@pytest.mark.parametrize("family", ["ret_topk", "fcos_topk"])
def test_coverage_select_keys_of_the_two_stages(family):
    stage1, stage2, pools, empty = set(), set(), [], 0
    wanted = {}
    for case, d, ref in data(family):
        views, e = onestage_views(case, d)
        empty += e
        stage1 |= {v[1] for v in views if v[0] == 1}
        stage2 |= {v[1] for v in views if v[0] == 2}
        pools += [v[3] for v in views if v[0] == 2]
        if case.g["kind"] == "sparse":
            wanted[case.g["exit"]] = {v[1] for v in views if v[0] == 2}
    assert stage2 == set(DC.EXITS), stage2  # early, and every pass 0 .. 7
    assert all(want in got for want, got in wanted.items()) and set(wanted) == set(DC.EXITS), wanted  # each by the case built for it
    assert "early" in stage1 and empty > 0 and len(stage1 - {"early"}) >= 2, (stage1, empty)
    trip = DC.consts()["rank_trip"]
    assert 0 in pools and any(0 < p < trip for p in pools) and any(p > trip for p in pools) and any(p > 2 * trip for p in pools)


def test_coverage_select_keys_of_ssd_topk():
    exits, wanted = set(), {}
    for case, d, ref in data("ssd_topk"):
        g = case.g
        thr = F32(d["thresh"])
        if d["sparse"] is not None:
            f, s = d["sparse"]["flat"], d["sparse"]["scores"]
            mine = {DC.select_exit(DC.score_keys(s, f, s > thr), g["k"])[0]}
            wanted[g["exit"]] = mine
        else:
            with np.errstate(invalid="ignore"):
                mine = {DC.select_exit(DC.score_keys(row, np.arange(g["v"]), row > thr), g["k"])[0] for img in d["scores"] for row in img[1:]}
        exits |= mine
    assert exits == set(DC.EXITS), exits
    assert all(want in got for want, got in wanted.items()) and set(wanted) == set(DC.EXITS), wanted


@pytest.mark.parametrize("family", DC.THRESHOLD_FAMILIES)
def main_scores(case, d):
    """The reference's float32 scores of image 0 in the view the threshold is taken from (the main level; SSD: the row of class 1),
    in the order the kernel's workgroups scan them (memory order; SSD: the row) -- None for a level that only exists on the device."""
    g = case.g
    if case.family == "ssd_topk":
        return None if isinstance(d["scores"], DC.Sparse) else d["scores"][0, 1]
    if isinstance(d["maps"][g["main"]], DC.Sparse):
        return None
    return onestage_scores_in_memory_order(case.family, d, g["main"])[0]


@pytest.mark.parametrize("family", DC.THRESHOLD_FAMILIES)
def test_coverage_thresholds(family):
    kinds, passing_minus_k = {}, set()
    for case, d, ref in data(family):
        g = case.g
        if family == "ssd_topk":
            first = ref.reshape(g["n"], g["classes"] - 1, g["k"])[0, 0]
            room = min(g["k"], g["v"])
        else:
            a, h, w = g["levels"][g["main"]]
            room = min(g["k"], a * h * w * g["classes"])
            at = sum(min(g["k"], x * y * z * g["classes"]) for x, y, z in g["levels"][:g["main"]])
            first = ref[0, at:at + room]
        taken = int((first >= 0).sum())
        kinds.setdefault(g["thr"], set()).add("none" if taken == 0 else "all" if taken == room else "some")
        if g["thr"] == "between" and g["kind"] == "normal":  # counted on the reference's scores, not read from the case's label
            with np.errstate(invalid="ignore"):
                passing = int((main_scores(case, d) > F32(d["thresh"])).sum())
            assert passing - g["k"] == g["rel"] and passing >= 1, (case.id, passing)
            passing_minus_k.add(passing - g["k"])
        assert (d["thresh"] < 0) == (g["thr"] == "negative" or (g["thr"] == "below" and d["thresh"] < 0)), case.id
    assert set(kinds) == set(DC.THRESHOLDS)
    assert kinds["above"] == {"none"} and "all" in kinds["negative"] and "all" in kinds["below"] and "some" in kinds["between"] and "some" in kinds["exact"]
    assert passing_minus_k == {-1, 0, 1}  # the passing candidates one below, at and one above k: either side of select_keys' early exit


@pytest.mark.parametrize("family", DC.THRESHOLD_FAMILIES)
def test_coverage_cut_in_ties(family):
    """On the reference's scores: the k-th and the (k + 1)-th passing candidate are equal, with 1, some and all of the tied run taken,
    and the run lies across a boundary of the scan (two stage-1 chunks; for k_ssd_topk a 1024-score step and a 4096-score trip)."""
    c = DC.consts()
    sizes = {"chunk": c["chunk"]} if family != "ssd_topk" else {"step": c["ssd_step"], "trip": c["ssd_trip"]}
    taken, crossing, cut = set(), set(), 0
    for case, d, ref in data(family):
        g = case.g
        if g["kind"] != "cut_in_ties":
            continue
        s = main_scores(case, d)
        with np.errstate(invalid="ignore"):
            ok = s > F32(d["thresh"])
        order = np.sort(s[ok])[::-1]
        if len(order) <= g["k"] or order[g["k"] - 1] != order[g["k"]]:
            continue
        cut += 1
        ties = np.flatnonzero(ok & (s == order[g["k"]]))
        need = g["k"] - int((s[ok] > order[g["k"]]).sum())
        assert 1 <= need < len(ties) and ties[-1] - ties[0] == len(ties) - 1, case.id  # one run, cut inside
        taken.add("one" if need == 1 else "some")
        crossing |= {name for name, size in sizes.items() if ties[0] // size != ties[-1] // size}
    assert cut >= 6 and taken == {"one", "some"} and crossing == set(sizes), (family, cut, taken, crossing)


def test_coverage_rpn_topk():
    c = DC.consts()
    need, takes, crossing = set(), set(), set()
    for case, d, ref in data("rpn_topk"):
        g = case.g
        for m in d["maps"]:
            flat = DC.rpn_flat(m)
            take = min(g["k"], flat.shape[1])
            takes.add(take)
            for row in flat:
                keys = DC.rpn_key(row)
                t = np.sort(keys)[::-1][take - 1]
                need_eq, ties = take - int((keys > t).sum()), np.flatnonzero(keys == t)
                assert 1 <= need_eq <= len(ties)  # the k-th key itself is one of them: need_eq == 0 cannot occur
                need.add("one" if need_eq == 1 else "all" if need_eq == len(ties) else "inside")
                if 1 < len(ties) < 16 and need_eq < len(ties) and ties[-1] - ties[0] == len(ties) - 1:  # the cut falls inside a run
                    over = [ties[0] // size != ties[-1] // size for size in (c["rpn_step"], c["rpn_trip"])]
                    crossing |= {"trip"} if over[1] else {"step"} if over[0] else set()  # a step inside a trip, or the end of a trip
    assert need == {"one", "all", "inside"}
    assert {c["rpn_step"] - 1, c["rpn_step"], c["rpn_step"] + 1} <= takes  # one ranking tile, and two
    assert crossing == {"step", "trip"}, crossing


# ---- independent: the selection ----------------------------------------------------------------------------------------------------------
def lexsort_select(scores, flat, thresh, k, strict=True):
    """The selection stated with numpy: the passing scores by (-score, flat index), the first k."""
    with np.errstate(invalid="ignore"):
        ok = scores > thresh if strict else scores >= thresh
    order = np.lexsort((flat[ok], -scores[ok].astype(np.float64)))
    return flat[ok][order][:k]


def onestage_scores_in_memory_order(family, d, l):
    m = torch.from_numpy(d["maps"][l])
    n = m.shape[0]
    if family.startswith("fcos"):
        return FR.score(m.reshape(n, m.shape[1], -1), torch.from_numpy(d["ctrs"][l]).reshape(n, 1, -1)).reshape(n, -1).numpy()
    return P.sigmoid_cr(m.reshape(n, -1)).numpy()


def independent_select(case, d):
    g = case.g
    kc, k = g["classes"], g["k"]
    starts = DC.level_starts(g["levels"])
    out = []
    for l, (a, h, w) in enumerate(g["levels"]):
        count = a * kc * h * w
        seg = min(k, count)
        rows = np.full((g["n"], seg), -1, np.int32)
        if isinstance(d["maps"][l], DC.Sparse):
            sel = lexsort_select(d["sparse"]["scores"], d["sparse"]["flat"], F32(d["thresh"]), k)
            rows[:, :len(sel)] = sel
        else:
            s = onestage_scores_in_memory_order(case.family, d, l)
            e = np.arange(count)
            flat = ((starts[l] + (e % (h * w)) * a + (e // (h * w)) // kc) * kc + (e // (h * w)) % kc).astype(np.int64)
            for i in range(g["n"]):
                sel = lexsort_select(s[i], flat, F32(d["thresh"]), k)
                rows[i, :len(sel)] = sel
        out.append(rows)
    return np.concatenate(out, 1)


@pytest.mark.parametrize("family", ["ret_topk", "fcos_topk"])
def test_selection_against_lexsort(family):
    for case, d, ref in data(family):
        assert ref.dtype == np.int32 and np.array_equal(ref, independent_select(case, d)), case.id
        if d["sparse"] is not None and not isinstance(d["maps"][case.g["main"]], DC.Sparse):
            # the closed form of a sparse case equals the restatement on the materialised maps
            maps = [torch.from_numpy(m) for m in d["maps"]]
            full = FR.select(maps, [torch.from_numpy(c) for c in d["ctrs"]], case.g["classes"], case.g["k"], d["thresh"]) if family == "fcos_topk" \
                else RR.select(maps, case.g["classes"], case.g["k"], d["thresh"])
            assert np.array_equal(ref, full.numpy()), case.id


def test_ssd_selection_against_lexsort():
    for case, d, ref in data("ssd_topk"):
        g = case.g
        want = np.full((g["n"], g["classes"] - 1, g["k"]), -1, np.int32)
        for i in range(g["n"]):
            for c in range(1, g["classes"]):
                if d["sparse"] is not None:
                    sel = lexsort_select(d["sparse"]["scores"], d["sparse"]["flat"], F32(d["thresh"]), g["k"])
                else:
                    sel = lexsort_select(d["scores"][i, c], np.arange(g["v"]), F32(d["thresh"]), g["k"])
                want[i, c - 1, :len(sel)] = sel * g["classes"] + c
        assert np.array_equal(ref, want.reshape(g["n"], -1)), case.id
        if d["sparse"] is not None and not isinstance(d["scores"], DC.Sparse):
            assert np.array_equal(ref, SR.select(torch.from_numpy(d["scores"]), g["k"], d["thresh"]).numpy()), case.id


def test_rpn_selection_against_lexsort():
    for case, d, ref in data("rpn_topk"):
        g = case.g
        out, start = [], 0
        for (a, h, w), m in zip(g["levels"], d["maps"]):
            e = np.arange(a * h * w)
            flat = (e % (h * w)) * a + e // (h * w)  # memory offset -> (y, x, a)
            rows = []
            for i in range(g["n"]):
                keys = DC.rpn_key(m[i].reshape(-1)).astype(np.int64)  # NaN greatest, -0 == +0
                rows.append(flat[np.lexsort((flat, -keys))][:g["k"]] + start)
            out.append(np.stack(rows))
            start += a * h * w
        assert np.array_equal(ref, np.concatenate(out, 1)), case.id


# ---- independent: the scores and the order against float64 ----------------------------------------------------------------------------
def close(ref, f64, bound, what):
    ref, f64, bound = (np.asarray(v, np.float64) for v in (ref, f64, bound))
    assert ref.shape == f64.shape, (what, ref.shape, f64.shape)
    finite = np.isfinite(f64)
    assert np.array_equal(np.isfinite(ref), finite), f"{what}: finite in other places"
    assert np.array_equal(np.isnan(ref), np.isnan(f64)), f"{what}: NaN in other places"
    err = np.abs(ref[finite] - f64[finite])
    bad = ~(err <= bound[finite] if bound.shape == ref.shape else err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outputs outside the bound"


def score64(family, d, l):
    m = torch.from_numpy(d["maps"][l]).double()
    n = m.shape[0]
    if family.startswith("fcos"):
        c = torch.from_numpy(d["ctrs"][l]).double().reshape(n, 1, -1)
        s = torch.sqrt(torch.sigmoid(m.reshape(n, m.shape[1], -1)) * torch.sigmoid(c)).reshape(n, -1).numpy()
        return s, gamma(6) * s + 2.0 ** -62
    s = torch.sigmoid(m.reshape(n, -1)).numpy()
    return s, gamma(4) * s + TINY


@pytest.mark.parametrize("family", ["ret_topk", "fcos_topk"])
def test_scores_and_order_against_float64(family):
    """The float32 scores within the bound of the float64 ones; the float64 selection equal to the float32 one at every position
    whose float64 score stands clear of both neighbours (or equals one exactly: a copied input) and of the threshold."""
    total = excluded = 0
    for case, d, ref in data(family):
        g = case.g
        kc, k, thr = g["classes"], g["k"], float(F32(d["thresh"]))
        starts = DC.level_starts(g["levels"])
        at = 0
        for l, (a, h, w) in enumerate(g["levels"]):
            count = a * kc * h * w
            seg = min(k, count)
            if not isinstance(d["maps"][l], DC.Sparse):
                s64, bound = score64(family, d, l)
                close(onestage_scores_in_memory_order(family, d, l), s64, bound, f"{case.id} level {l}")
                e = np.arange(count)
                flat = ((starts[l] + (e % (h * w)) * a + (e // (h * w)) // kc) * kc + (e // (h * w)) % kc).astype(np.int64)
                for i in range(g["n"]) if g["thr"] != "exact" else ():
                    s, b = s64[i], bound[i]
                    got = ref[i, at:at + seg]
                    taken = int((got >= 0).sum())
                    with np.errstate(invalid="ignore"):
                        maybe = s > thr - b  # every score that can pass in float32
                    order = np.lexsort((flat[maybe], -s[maybe]))[:seg + 1]
                    so, bo, fo = s[maybe][order], b[maybe][order], flat[maybe][order]
                    sure = so - thr > bo  # ... and those that must: a prefix of the order
                    m = min(seg, len(so) if sure.all() else int(np.argmin(sure)))
                    assert m <= taken <= min(seg, len(so)), f"{case.id} image {i} level {l}: the count of passing scores"
                    gap = so[:-1] - so[1:]
                    clear = (gap == 0) | (gap > bo[:-1] + bo[1:])  # equal inputs, or clear of both bounds
                    decided = (np.concatenate([[True], clear]) & np.concatenate([clear, [True]]))[:m]
                    assert np.array_equal(got[:m][decided], fo[:m][decided]), f"{case.id} image {i} level {l}"
                    total += taken
                    excluded += taken - int(decided.sum())
            at += seg
    share = excluded / total
    assert share <= 0.01, f"{family}: {excluded} of {total} positions ({share:.3%}) excluded by the margin"
    print(f"{family}: {excluded} of {total} positions ({share:.3%}) excluded by the margin")


def finite_spread(logits):
    """max - min over the finite logits of every row (the last axis): a -inf logit has the exponential 0 whatever the rounding."""
    with np.errstate(all="ignore"):
        fin = np.isfinite(logits)
        return np.where(fin.any(-1), np.where(fin, logits, -np.inf).max(-1) - np.where(fin, logits, np.inf).min(-1), 0.0)


def test_ssd_scores_against_float64():
    for case, d, ref in data("ssd_scores"):
        g = case.g
        logits = torch.cat([SR.permute_level(torch.from_numpy(m), g["classes"]) for m in d["maps"]], 1).double()  # (N, V, K)
        with np.errstate(all="ignore"):
            p = torch.softmax(logits, -1).permute(0, 2, 1).numpy()
        bound = gamma(2 * np.ceil(finite_spread(logits.numpy()))[:, None, :] + 4) * p + TINY
        assert ref.dtype == F32, case.id
        close(ref, p, bound, case.id)  # a row with a NaN or a +inf logit is NaN on both sides; a -inf logit scores 0


# ---- independent: the decodes against float64 ------------------------------------------------------------------------------------------
def decode64(boxes, codes, weights, clip):
    """BoxCoder.decode_single in float64 -> (boxes, bound); boxes (M, 4), codes (M, 4 C)."""
    b, c = torch.from_numpy(np.ascontiguousarray(boxes)).double(), torch.from_numpy(np.ascontiguousarray(codes)).double()
    clip32 = float(F32(clip))
    with np.errstate(all="ignore"):
        out = P.BoxCoder(weights, clip32, numerics=P.REPLICA).decode_single(c, b).numpy()
        span = (b[:, 0].abs() + b[:, 2].abs()).numpy()[:, None], (b[:, 1].abs() + b[:, 3].abs()).numpy()[:, None]
        dx, dy = np.abs(c[:, 0::4].numpy()) / weights[0], np.abs(c[:, 1::4].numpy()) / weights[1]
        ew = np.exp(np.minimum(c[:, 2::4].numpy() / weights[2], clip32))
        eh = np.exp(np.minimum(c[:, 3::4].numpy() / weights[3], clip32))
        ax, ay = span[0] * (1 + dx + ew), span[1] * (1 + dy + eh)
        bound = gamma(14) * np.stack([ax, ay, ax, ay], 2).reshape(out.shape)
    return out, bound


def clip64(boxes, size, bound=None):
    """clip_boxes_to_image in float64 (a NaN stays).  With `bound`: also the bound of the clipped value -- 0 where the float64 corner
    lies beyond the border by more than its bound (the float32 one is clamped to the same exact number)."""
    out = boxes.copy()
    bound = np.zeros_like(boxes) if bound is None else np.broadcast_to(bound, boxes.shape).copy()
    with np.errstate(invalid="ignore"):
        for sl, hi in ((np.s_[..., 0::2], size[1]), (np.s_[..., 1::2], size[0])):
            v, b = boxes[sl], bound[sl]
            bound[sl] = np.where((v < -b) | (v > hi + b) | np.isinf(v), 0.0, b)
            out[sl] = np.where(np.isnan(v), np.nan, np.clip(v, 0, hi))
    return out, bound


def test_box_decode_against_float64():
    for case, d, ref in data("box_decode"):
        want, bound = decode64(d["boxes"], d["codes"], case.g["weights"], case.g["clip"])
        close(ref, want, bound, case.id)


def gather_level(maps, per):
    """Per-level NCHW maps -> (N, total anchors, per) in the (y, x, a) layout, by explicit index arithmetic."""
    out = []
    for m in maps:
        n, c, h, w = m.shape
        a = c // per
        out.append(m.reshape(n, a, per, h * w).transpose(0, 3, 1, 2).reshape(n, h * w * a, per))
    return np.concatenate(out, 1)


@pytest.mark.parametrize("family", ["rpn_decode", "ret_decode", "fcos_decode"])
def test_pyramid_decode_against_float64(family):
    total = excluded = 0
    for case, d, ref in data(family):
        g = case.g
        kc = g["classes"]
        boxes, scores, third, valid = ref
        anchors = DC.grid_anchors(g["levels"], d["cells"], g["strides"]).astype(np.float64)  # exact: small integers and halves
        deltas, logits = gather_level(d["deltas"], 4), gather_level(d["logits"], kc)
        count = anchors.shape[0]
        starts = DC.level_starts(g["levels"])
        for i in range(g["n"]):
            f = d["idx"][i].astype(np.int64)
            ok = (f >= 0) & (f < count * kc)
            assert np.array_equal(valid[i] | (family == "rpn_decode"), ok | (family == "rpn_decode")) and not (valid[i] & ~ok).any(), case.id
            v, c = f[ok] // kc, f[ok] % kc
            if family == "fcos_decode":
                r = np.maximum(deltas[i][v].astype(np.float64), 0)
                with np.errstate(invalid="ignore"):
                    r = np.where(np.isnan(deltas[i][v]), np.nan, r)
                a4 = anchors[v]
                cx, cy, w, h = (a4[:, 0] + a4[:, 2]) / 2, (a4[:, 1] + a4[:, 3]) / 2, a4[:, 2] - a4[:, 0], a4[:, 3] - a4[:, 1]
                with np.errstate(all="ignore"):
                    want = np.stack([cx - r[:, 0] * w, cy - r[:, 1] * h, cx + r[:, 2] * w, cy + r[:, 3] * h], 1)
                    span = np.stack([np.abs(a4[:, 0]) + np.abs(a4[:, 2]), np.abs(a4[:, 1]) + np.abs(a4[:, 3])] * 2, 1)
                    bound = gamma(6) * span * (1 + np.abs(r))
                ctr = gather_level(d["ctrs"], 1)[i][v, 0].astype(np.float64)
                x = logits[i][v, c].astype(np.float64)
                with np.errstate(all="ignore"):
                    s64 = np.sqrt(1 / (1 + np.exp(-x)) / (1 + np.exp(-ctr)))
                sb = gamma(6) * s64 + 2.0 ** -62
            else:
                want, bound = decode64(anchors[v], deltas[i][v], g["weights"], g.get("clip", DC.CLIP))
                with np.errstate(all="ignore"):
                    s64 = 1 / (1 + np.exp(-logits[i][v, c].astype(np.float64)))
                sb = gamma(4) * s64 + TINY
            want, bound = clip64(want, d["sizes"][i], bound)
            close(boxes[i][ok], want, bound, f"{case.id} image {i} boxes")
            close(scores[i][ok], s64, sb, f"{case.id} image {i} scores")
            assert not boxes[i][~ok].any() and not scores[i][~ok].any(), case.id
            if family == "rpn_decode":
                level = np.searchsorted(starts[1:], v, side="right")
                assert np.array_equal(third[i][ok], level) and (third[i][~ok] == -1).all(), case.id
                with np.errstate(invalid="ignore"):
                    ws, hs = want[:, 2] - want[:, 0], want[:, 3] - want[:, 1]
                    flag = (ws >= g["min_size"]) & (hs >= g["min_size"]) & (s64 >= g["score_thresh"])
                    mw, mh = bound[:, 0] + bound[:, 2], bound[:, 1] + bound[:, 3]  # 0: both corners clamped, the side is exact
                    decided = ((np.abs(ws - g["min_size"]) > mw) | (mw == 0)) & ((np.abs(hs - g["min_size"]) > mh) | (mh == 0)) & (np.abs(s64 - g["score_thresh"]) > sb)
                    decided |= np.isnan(ws) | np.isnan(hs) | np.isnan(s64)  # a NaN fails in float32 as in float64
                    decided |= ((s64 == 0) | (s64 == 1)) & ((np.abs(ws - g["min_size"]) > mw) | (mw == 0)) & ((np.abs(hs - g["min_size"]) > mh) | (mh == 0))  # exact in both
                assert np.array_equal(valid[i][ok][decided], flag[decided]), case.id
                total += len(decided)
                excluded += int((~decided).sum())
            else:
                assert np.array_equal(third[i][ok], c) and not third[i][~ok].any(), case.id
    if family == "rpn_decode":
        share = excluded / total
        assert share <= 0.01, f"rpn_decode: {excluded} of {total} flags ({share:.3%}) excluded by the margin"
        print(f"rpn_decode: {excluded} of {total} flags ({share:.3%}) excluded by the margin")


def default_boxes64(levels, pairs, steps, clip, batch):
    """DefaultBoxGenerator in float64 on the float32 pairs: (V, 4) in the (y, x, a) layout."""
    bh, bw = batch
    out = []
    for l, (a, h, w) in enumerate(levels):
        x_f, y_f = (float(F32(bw / steps[l])), float(F32(bh / steps[l]))) if steps is not None else (float(w), float(h))
        p = pairs[l].astype(np.float64)
        p = np.clip(p, 0, 1) if clip else p
        cy, cx = np.meshgrid((np.arange(h) + 0.5) / y_f, (np.arange(w) + 0.5) / x_f, indexing="ij")
        cx, cy = cx.reshape(-1, 1), cy.reshape(-1, 1)
        out.append(np.stack([(cx - p[:, 0] / 2) * bw, (cy - p[:, 1] / 2) * bh, (cx + p[:, 0] / 2) * bw, (cy + p[:, 1] / 2) * bh], 2).reshape(-1, 4))
    return np.concatenate(out)


def test_ssd_decode_against_float64():
    for case, d, ref in data("ssd_decode"):
        g = case.g
        kc = g["classes"]
        boxes, scores, labels, valid = ref
        dboxes = default_boxes64(g["levels"], d["pairs"], g["steps"], g["clip_pairs"], g["batch"])
        deltas = gather_level(d["deltas"], 4)
        count = dboxes.shape[0]
        for i in range(g["n"]):
            f = d["idx"][i].astype(np.int64)
            ok = (f >= 0) & (f < count * kc)
            assert np.array_equal(valid[i], ok), case.id
            v, c = f[ok] // kc, f[ok] % kc
            want, bound = decode64(dboxes[v], deltas[i][v], g["weights"], DC.CLIP)
            # the default box itself: 5 roundings on (|cx| + |w| / 2) W, through decode_single's gain (already in `bound` / gamma(14))
            bound = bound * (1 + 5 / 14)
            close(boxes[i][ok], *clip64(want, d["sizes"][i], bound), f"{case.id} image {i} boxes")
            assert np.array_equal(scores[i][ok], d["scores"][i, c, v], equal_nan=True) and np.array_equal(labels[i][ok], c), case.id
            assert (c >= 0).all() and not boxes[i][~ok].any() and not scores[i][~ok].any() and not labels[i][~ok].any(), case.id


def test_roi_det_against_float64():
    total = excluded = 0
    for case, d, ref in data("roi_det"):
        g = case.g
        r, c = g["r"], g["classes"]
        boxes, scores, labels, valid = ref
        assert boxes.shape == (r, c - 1, 4) and scores.shape == labels.shape == valid.shape == (r, c - 1), case.id  # the background column is gone
        if not r:
            continue
        logits = torch.from_numpy(d["logits"]).double()
        with np.errstate(all="ignore"):
            p = torch.softmax(logits, -1).numpy()[:, 1:]
        spread = finite_spread(logits.numpy())
        want, bound = decode64(d["rois"][:, 1:], d["deltas"], g["weights"], DC.CLIP)
        want, bound = want.reshape(r, c, 4)[:, 1:], bound.reshape(r, c, 4)[:, 1:]
        for i in range(r):
            img = DC.roi_image(float(d["rois"][i, 0]), g["n"])
            if img is None:
                assert not boxes[i].any() and not scores[i].any() and not labels[i].any() and not valid[i].any(), (case.id, i)
                continue
            assert labels[i].tolist() == list(range(1, c)), (case.id, i)
            w, wb = clip64(want[i], d["sizes"][img], bound[i])
            close(boxes[i], w, wb, f"{case.id} roi {i} boxes")
            if np.isfinite(p[i]).all():
                sb = gamma(2 * np.ceil(spread[i]) + 4 + c - 1) * p[i] + TINY
                close(scores[i], p[i], sb, f"{case.id} roi {i} scores")
                with np.errstate(invalid="ignore"):
                    ws, hs = w[:, 2] - w[:, 0], w[:, 3] - w[:, 1]
                    flag = (p[i] > g["score_thresh"]) & (ws >= g["min_size"]) & (hs >= g["min_size"])
                    mw, mh = wb[:, 0] + wb[:, 2], wb[:, 1] + wb[:, 3]
                    decided = ((np.abs(ws - g["min_size"]) > mw) | (mw == 0)) & ((np.abs(hs - g["min_size"]) > mh) | (mh == 0)) & (np.abs(p[i] - g["score_thresh"]) > sb)
                    decided |= np.isnan(ws) | np.isnan(hs)
                assert np.array_equal(valid[i][decided], flag[decided]), (case.id, i)
                total += len(decided)
                excluded += int((~decided).sum())
    share = excluded / total
    assert share <= 0.01, f"roi_det: {excluded} of {total} flags ({share:.3%}) excluded by the margin"
    print(f"roi_det: {excluded} of {total} flags ({share:.3%}) excluded by the margin")
