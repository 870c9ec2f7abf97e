"""Seeded random-shape sweeps of the top-k, score and decode kernels of RPN / RetinaNet / FCOS / SSD / RoIHeads against their
references (`-m gpu`): the cases of tests/_fuzz_detect_cases.py -- F.rpn_topk, F.rpn_decode, F.retinanet_topk, F.fcos_topk,
F.retinanet_decode, F.fcos_decode, F.ssd_scores, F.ssd_topk, F.ssd_decode, F.roi_detections and F.box_decode.

Every comparison is the one the family's own test file makes: indices, labels, levels and flags equal, float32 outputs bit for bit with
NaN in equal places (-0 equals +0, as tests/_rpn_ref.same).  The kernel names are recorded and checked as in
tests/test_gpu_fuzz_layers.py; each family's sweep must have launched its kernel with every level count 1 .. kMaxRpnLevels (the RoI
kernel: with class counts on every side of the wave).  tests/test_fuzz_detect_host.py holds what keeps the sweeps from passing
vacuously."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from tests import _fuzz_detect_cases as DC  # noqa: E402
from tests import _fuzz_gpu  # noqa: E402
from tests import _rpn_ref as P  # noqa: E402


def dev(m, layout="dense"):
    """A map on the device as the entry sees it; a Sparse one is filled and scattered there."""
    if isinstance(m, DC.Sparse):
        return m.tensor("cuda")
    return DC.place(torch.from_numpy(np.ascontiguousarray(m)), layout, lambda t: t.cuda())


def sweep(family, chunk, run):
    return _fuzz_gpu.sweep(family, chunk, run, cases=DC)


def kernels_of(family, run):
    return _fuzz_gpu.kernels_of(family, run, cases=DC)


def chunked(family):
    return _fuzz_gpu.chunked(family, cases=DC)


def level_counts(names, pattern):
    found = [re.fullmatch(pattern, n) for n in names]
    assert all(found), names
    return {int(m.group(1)) for m in found}


ALL_LEVELS = set(range(1, DC.consts()["max_levels"] + 1))


def same_indices(got, want, case):
    assert got.dtype == torch.int32 and tuple(got.shape) == tuple(want.shape), (case.id, tuple(got.shape), want.shape)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), f"{case.id}: {int((got != want).sum())} of {want.size} indices differ, the first at {np.argwhere(got != want)[0].tolist()}"


def same_candidates(got, want, case, third="labels"):
    boxes, scores, ints, valid = got
    assert ints.dtype == torch.int64 and valid.dtype == torch.bool, case.id
    for name, g, w in zip(("boxes", "scores", third, "valid"), got, want):
        P.same(g, torch.from_numpy(np.ascontiguousarray(w)), f"{case.id} {name}")


# ---- the top-k families -----------------------------------------------------------------------------------------------------------------
def run_rpn_topk(case, d, want):
    g = case.g
    got = F.rpn_topk([dev(m, g["layout"]) for m in d["maps"]], g["k"])
    name = _lib.last_kernel()
    assert name == f"k_rpn_topk<levels{len(g['levels'])},k{g['k']}>", (case.id, name)
    if want is not None:
        same_indices(got, want, case)
    return [name]


@chunked("rpn_topk")
def test_rpn_topk(chunk):
    sweep("rpn_topk", chunk, run_rpn_topk)


def test_rpn_topk_reaches_every_kernel():
    assert level_counts(kernels_of("rpn_topk", run_rpn_topk), r"k_rpn_topk<levels(\d+),k\d+>") == ALL_LEVELS


def run_onestage_topk(case, d, want):
    g = case.g
    maps = [dev(m, g["layout"]) for m in d["maps"]]
    if case.family == "fcos_topk":
        got = F.fcos_topk(maps, [dev(m, g["layout"]) for m in d["ctrs"]], g["classes"], g["k"], d["thresh"])
    else:
        got = F.retinanet_topk(maps, g["classes"], g["k"], d["thresh"])
    name = _lib.last_kernel()
    assert name == f"k_retinanet_rank<{'fcos,' if case.family == 'fcos_topk' else ''}levels{len(g['levels'])},k{g['k']}>", (case.id, name)
    if want is not None:
        same_indices(got, want, case)
    return [name]


@chunked("ret_topk")
def test_ret_topk(chunk):
    sweep("ret_topk", chunk, run_onestage_topk)


def test_ret_topk_reaches_every_kernel():
    assert level_counts(kernels_of("ret_topk", run_onestage_topk), r"k_retinanet_rank<levels(\d+),k\d+>") == ALL_LEVELS


@chunked("fcos_topk")
def test_fcos_topk(chunk):
    sweep("fcos_topk", chunk, run_onestage_topk)


def test_fcos_topk_reaches_every_kernel():
    assert level_counts(kernels_of("fcos_topk", run_onestage_topk), r"k_retinanet_rank<fcos,levels(\d+),k\d+>") == ALL_LEVELS


def run_ssd_topk(case, d, want):
    g = case.g
    s = d["scores"]
    scores = s.tensor("cuda").reshape(g["n"], g["classes"], g["v"]) if isinstance(s, DC.Sparse) else torch.from_numpy(s).cuda()
    got = F.ssd_topk(scores, g["k"], d["thresh"])
    name = _lib.last_kernel()
    assert name == f"k_ssd_topk<classes{g['classes']},k{g['k']}>", (case.id, name)
    if want is not None:
        same_indices(got, want, case)
    return [name]


@chunked("ssd_topk")
def test_ssd_topk(chunk):
    sweep("ssd_topk", chunk, run_ssd_topk)


def test_ssd_topk_reaches_every_kernel():
    classes = level_counts(kernels_of("ssd_topk", run_ssd_topk), r"k_ssd_topk<classes(\d+),k\d+>")
    assert {2, 3, 91} <= classes


# ---- the scores ---------------------------------------------------------------------------------------------------------------------------
def run_ssd_scores(case, d, want):
    g = case.g
    got = F.ssd_scores([dev(m, g["layout"]) for m in d["maps"]], g["classes"])
    name = _lib.last_kernel()
    assert name == f"k_ssd_scores<levels{len(g['levels'])},classes{g['classes']}>", (case.id, name)
    if want is not None:
        P.same(got, torch.from_numpy(want), case.id)
    return [name]


@chunked("ssd_scores")
def test_ssd_scores(chunk):
    sweep("ssd_scores", chunk, run_ssd_scores)


def test_ssd_scores_reaches_every_kernel():
    assert level_counts(kernels_of("ssd_scores", run_ssd_scores), r"k_ssd_scores<levels(\d+),classes\d+>") == ALL_LEVELS


# ---- the decodes --------------------------------------------------------------------------------------------------------------------------
def run_pyramid_decode(case, d, want):
    g, fam = case.g, case.family
    lay = g["layout"]
    lg, dl = [dev(m, lay) for m in d["logits"]], [dev(m, lay) for m in d["deltas"]]
    idx, cells = torch.from_numpy(d["idx"]).cuda(), [torch.from_numpy(c) for c in d["cells"]]
    if fam == "rpn_decode":
        got = F.rpn_decode(lg, dl, idx, cells, g["strides"], d["sizes"], g["weights"], DC.CLIP, g["min_size"], g["score_thresh"])
        kernel = "k_rpn_decode"
    elif fam == "ret_decode":
        got = F.retinanet_decode(lg, dl, idx, cells, g["strides"], d["sizes"], g["classes"], g["weights"], g["clip"])
        kernel = "k_retinanet_decode"
    else:
        got = F.fcos_decode(lg, [dev(m, lay) for m in d["ctrs"]], dl, idx, cells, g["strides"], d["sizes"], g["classes"])
        kernel = "k_fcos_decode"
    name = _lib.last_kernel()
    assert name == f"{kernel}<levels{len(g['levels'])}>", (case.id, name)
    if want is not None:
        same_candidates(got, want, case, "levels" if fam == "rpn_decode" else "labels")
    return [name]


@chunked("rpn_decode")
def test_rpn_decode(chunk):
    sweep("rpn_decode", chunk, run_pyramid_decode)


def test_rpn_decode_reaches_every_kernel():
    assert level_counts(kernels_of("rpn_decode", run_pyramid_decode), r"k_rpn_decode<levels(\d+)>") == ALL_LEVELS


@chunked("ret_decode")
def test_ret_decode(chunk):
    sweep("ret_decode", chunk, run_pyramid_decode)


def test_ret_decode_reaches_every_kernel():
    assert level_counts(kernels_of("ret_decode", run_pyramid_decode), r"k_retinanet_decode<levels(\d+)>") == ALL_LEVELS


@chunked("fcos_decode")
def test_fcos_decode(chunk):
    sweep("fcos_decode", chunk, run_pyramid_decode)


def test_fcos_decode_reaches_every_kernel():
    assert level_counts(kernels_of("fcos_decode", run_pyramid_decode), r"k_fcos_decode<levels(\d+)>") == ALL_LEVELS


def run_ssd_decode(case, d, want):
    g = case.g
    got = F.ssd_decode(torch.from_numpy(d["scores"]).cuda(), [dev(m, g["layout"]) for m in d["deltas"]], torch.from_numpy(d["idx"]).cuda(),
                       [torch.from_numpy(p) for p in d["pairs"]], g["steps"], g["batch"], d["sizes"], g["weights"], g["clip_pairs"])
    name = _lib.last_kernel()
    assert name == f"k_ssd_decode<levels{len(g['levels'])}>", (case.id, name)
    if want is not None:
        same_candidates(got, want, case)
    return [name]


@chunked("ssd_decode")
def test_ssd_decode(chunk):
    sweep("ssd_decode", chunk, run_ssd_decode)


def test_ssd_decode_reaches_every_kernel():
    assert level_counts(kernels_of("ssd_decode", run_ssd_decode), r"k_ssd_decode<levels(\d+)>") == ALL_LEVELS


# ---- roi_detections, box_decode ----------------------------------------------------------------------------------------------------------
def run_roi_det(case, d, want):
    g = case.g
    lg, dl = torch.from_numpy(d["logits"]).cuda(), torch.from_numpy(d["deltas"]).cuda()
    if g["sliced"]:  # column slices of one wider tensor, passed by their row strides
        both = torch.cat([lg, dl], 1)
        lg, dl = both[:, :g["classes"]], both[:, g["classes"]:]
    got = F.roi_detections(lg, dl, torch.from_numpy(d["rois"]).cuda(), d["sizes"], g["weights"], DC.CLIP, g["score_thresh"], g["min_size"])
    if want is not None:
        same_candidates(got, want, case)
    if not g["r"]:
        return []
    name = _lib.last_kernel()
    assert name == f"k_roi_detections<classes{g['classes']}>", (case.id, name)
    return [name]


@chunked("roi_det")
def test_roi_det(chunk):
    sweep("roi_det", chunk, run_roi_det)


def test_roi_det_reaches_every_kernel():
    c = DC.consts()
    classes = level_counts(kernels_of("roi_det", run_roi_det), r"k_roi_detections<classes(\d+)>")
    assert {2, c["roi_max_classes"]} <= classes and {0, 1, c["wave"] - 1} <= {k % c["wave"] for k in classes}
    assert {-(-k // c["wave"]) for k in classes} >= {1, 2, 3, 4}  # one to four strides of the lanes over the classes


def run_box_decode(case, d, want):
    g = case.g
    got = F.box_decode(torch.from_numpy(d["boxes"]).cuda(), torch.from_numpy(d["codes"]).cuda(), g["weights"], g["clip"])
    assert tuple(got.shape) == (g["m"], 4 * g["c"]) and got.dtype == torch.float32, case.id
    if want is not None:
        P.same(got, torch.from_numpy(want), case.id)
    if not g["m"]:
        return []
    assert _lib.last_kernel() == "k_box_decode", (case.id, _lib.last_kernel())
    return ["k_box_decode"]


@chunked("box_decode")
def test_box_decode(chunk):
    sweep("box_decode", chunk, run_box_decode)


def test_box_decode_reaches_every_kernel():
    assert kernels_of("box_decode", run_box_decode) == {"k_box_decode"}
