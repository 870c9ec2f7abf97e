"""Seeded random-shape sweeps of the RoI and detection kernels against their references (`-m gpu`): the cases of
tests/_fuzz_cases.py -- roi_align, roi_pool, ps_roi_pool, ps_roi_align, nms and batched_nms, paste_masks_in_image and
heatmaps_to_keypoints.

Every comparison is the one the family's own test file makes: the float32 restatement bit for bit (NaN in equal places), the kept
indices of nms equal.  The kernel names are recorded and checked as in tests/test_gpu_fuzz_layers.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, ops  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from tests import _fuzz_cases as FC  # noqa: E402
from tests._fuzz_gpu import chunked, dev, kernels_of, same_bits, sweep  # noqa: E402


# ---- 11. the RoI operators ---------------------------------------------------------------------------------------------------------------
def run_roi(case, d, want):
    g = case.g
    x, rois, out = dev(d["x"]), dev(d["rois"]), (g["ph"], g["pw"])
    if g["op"] == "roi_align":
        got = ops.roi_align(x, rois, out, g["scale"], g["ratio"], g["aligned"])
        name = f"k_roi_align<{'aligned' if g['aligned'] else 'legacy'},{'fixed' if g['ratio'] > 0 else 'adaptive'}>"
    elif g["op"] == "ps_roi_align":
        got = ops.ps_roi_align(x, rois, out, g["scale"], g["ratio"])
        name = f"k_ps_roi_align<{'fixed' if g['ratio'] > 0 else 'adaptive'}>"
    else:
        got = getattr(ops, g["op"])(x, rois, out, g["scale"])
        name = "k_" + g["op"]
    c_out = g["c"] // (g["ph"] * g["pw"]) if g["op"].startswith("ps_") else g["c"]
    assert tuple(got.shape) == (g["rois"], c_out) + out and got.dtype == torch.float32, case.id
    if g["rois"]:
        assert _lib.last_kernel() == name, (case.id, _lib.last_kernel())
    if want is not None:
        want = want[0] if isinstance(want, tuple) else want
        assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), \
            f"{case.id}: {int((~np.isclose(got.cpu().numpy(), want, rtol=0, atol=0, equal_nan=True)).sum())} of {want.size} elements differ"
    return [name] if g["rois"] else []


@chunked("roi")
def test_roi(chunk):
    sweep("roi", chunk, run_roi)


def test_roi_reaches_every_kernel():
    want = {f"k_roi_align<{a},{r}>" for a in ("aligned", "legacy") for r in ("fixed", "adaptive")}
    want |= {"k_roi_pool", "k_ps_roi_pool", "k_ps_roi_align<fixed>", "k_ps_roi_align<adaptive>"}
    assert kernels_of("roi", run_roi) == want


# ---- 12. nms, batched_nms ----------------------------------------------------------------------------------------------------------------
def run_nms(case, d, want):
    g = case.g
    b, s = dev(d["boxes"]), dev(d["scores"])
    keep = ops.batched_nms(b, s, dev(d["idxs"]), g["thr"]) if "idxs" in d else ops.nms(b, s, g["thr"])
    assert keep.dtype == torch.int64 and keep.ndim == 1 and keep.is_cuda, case.id
    if want is not None:
        assert keep.cpu().tolist() == want.tolist(), f"{case.id} (boxes of make_boxes seed {d['box_seed']}): {len(keep)} kept, reference {len(want)}"
    if not g["boxes"]:
        return []
    tiles = -(-g["boxes"] // FC.nms_block_sizes()[0])
    assert _lib.last_kernel() == f"k_nms_rank+k_nms_mask<64x64>+k_nms_reduce<tiles{tiles}>", (case.id, _lib.last_kernel())
    return [_lib.last_kernel()]


@chunked("nms")
def test_nms(chunk):
    sweep("nms", chunk, run_nms)


def test_nms_reaches_every_kernel():
    tiles = {int(n.split("tiles")[1].rstrip(">")) for n in kernels_of("nms", run_nms)}
    wave, _, staged = FC.nms_block_sizes()
    assert {1, 2, 3} <= tiles and max(tiles) > staged // wave, tiles  # one mask tile, several, and more boxes than one rank step stages


# ---- 13. paste_masks_in_image, heatmaps_to_keypoints -----------------------------------------------------------------------------------
def run_paste(case, d, want):
    g = case.g
    got = F.paste_masks_in_image(dev(d["masks"]), dev(d["boxes"]), (g["h"], g["w"]), g["padding"])
    name = _lib.last_kernel()
    assert name == f"k_paste_masks<{'vec16' if g['w'] % 4 == 0 else 'scalar'}>", (case.id, name)
    if want is not None:
        same_bits(got, want, case.id)
    return [name]


@chunked("paste")
def test_paste(chunk):
    sweep("paste", chunk, run_paste)


def test_paste_reaches_every_kernel():
    assert kernels_of("paste", run_paste) == {"k_paste_masks<vec16>", "k_paste_masks<scalar>"}


def run_keypoints(case, d, want):
    xy, scores = F.heatmaps_to_keypoints(dev(d["maps"]), dev(d["rois"]))
    name = _lib.last_kernel()
    if want is not None:
        same_bits(xy, want[0], case.id + ": xy")
        same_bits(scores, want[1], case.id + ": scores")
    return [name]


@chunked("keypoints")
def test_keypoints(chunk):
    sweep("keypoints", chunk, run_keypoints)


def test_keypoints_reaches_every_kernel():
    assert kernels_of("keypoints", run_keypoints) == {"k_heatmaps_to_keypoints"}
