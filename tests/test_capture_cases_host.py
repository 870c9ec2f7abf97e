"""The capture cases of tests/_capture_cases.py without a GPU: every case runs its public wrapper on CPU tensors with the library
replaced by a recording proxy (_capture_cases.Recorder), as _lib.tuning_library swaps it -- a call of a stream-taking entry point is
recorded and reports success without running; the host queries (workspace sizes, K slices) go to the real library.

  * the names CALLED over all cases, together with the not-capturable table and the one entry point no wrapper calls, are exactly
    the stream-taking entry points of include/mi355vision.h, which declares 111 of them (restated from the header, not written down);
  * no case is one the host path refuses, every case records at least one launch, and its tensors total at most MAX_BYTES;
  * the two data seeds of a case differ in EVERY array -- weights, biases, norm terms, boxes and gates included -- and their CPU
    references differ: where the inputs select the outputs (RoI boxes, pasted boxes, keypoint rois) the second seed changes the
    selection, and no case is vacuous."""
import numpy as np
import pytest
import torch

from cpu_vision_amd import _filters, _lib
from tests import _capture_cases as CC
from tests import _fuzz_cases as FC

STREAM = CC.stream_entry_points()


@pytest.fixture
def recorder(monkeypatch):
    rec = CC.Recorder(_lib.load())
    monkeypatch.setattr(_lib, "_lib", rec)
    monkeypatch.setattr(_lib, "require_device", lambda t, what="input": None)
    monkeypatch.setattr(_lib, "stream_ptr", lambda t: 0)
    # the lists of frames go through one mv_*_v launch when they lie on one device: here the CPU stands for it
    monkeypatch.setattr(_filters, "_same_frames", lambda frames: all(f.dtype == frames[0].dtype and f.shape == frames[0].shape for f in frames))
    return rec


def test_the_header_declares_the_entry_points_the_binding_declares():
    assert STREAM <= set(_lib.SYMBOLS) and len(STREAM) == 111
    assert not any(n in STREAM for n in ("mv_abi_version", "mv_fold_batchnorm", "mv_conv1x1_k_slices", "mv_nms_workspace_bytes"))
    assert {"mv_nms_f32", "mv_conv_norm_act_f32", "mv_pad_crop_flip", "mv_erase", "mv_gaussian_blur_u8_ws"} <= STREAM


def test_every_family_has_a_case_per_form():
    table = CC.cases()
    assert len(table) == len({c.id for c in table.values()})
    for family in CC.CALLS:
        mine = [c for c in table.values() if c.family == family]
        forms = {CC.FORMS[family](c.g) for c in FC.cases(family) if CC._usable(c, FC.inputs(c))}
        assert len(mine) == len(forms) >= 1, family
        assert {CC.FORMS[family](c.g) for c in mine} == forms, family
    roi = {c.g["op"] for c in table.values() if c.family == "roi"}
    assert roi == {"roi_align", "roi_pool", "ps_roi_pool", "ps_roi_align"}
    assert {c.g["k"] for c in table.values() if c.family == "convt"} == {2, 4}
    assert {(c.g["stride"], c.g["dilation"]) for c in table.values() if c.family == "dw5x5"} == {(1, 1), (2, 1), (1, 2)}


@pytest.mark.parametrize("name", list(CC.cases()))
def test_case_passes_its_host_path_and_launches(name, recorder):
    case = CC.cases()[name]
    d = CC.inputs(case)
    assert sum(a.nbytes for _, a in CC.arrays(d)) <= CC.MAX_BYTES
    out = CC.call(case, CC.tensors(d))
    outs = out if isinstance(out, tuple) else (out,)
    assert all(isinstance(o, torch.Tensor) and o.numel() for o in outs), name
    assert recorder.names and set(recorder.names) <= CC.captured_entry_points(), (name, recorder.names)


def test_census_of_the_stream_taking_entry_points(recorder):
    """The names the cases call, together with the not-capturable table, are exactly the stream-taking entry points of the header;
    the two tables are disjoint."""
    for case in CC.cases().values():
        CC.call(case, CC.tensors(CC.inputs(case)))
    called = set(recorder.names)
    assert not called & set(CC.NOT_CAPTURABLE) and not called & set(CC.NO_WRAPPER) and not set(CC.NOT_CAPTURABLE) & set(CC.NO_WRAPPER)
    assert called | set(CC.NOT_CAPTURABLE) | set(CC.NO_WRAPPER) == STREAM
    for name, reason in CC.NOT_CAPTURABLE.items():
        assert reason.startswith(("the wrapper returns a data-dependent shape", "the wrapper returns a host value",
                                  "the wrapper draws its parameters from the host RNG")) and "ops.py" in reason, name


def test_the_proxy_records_calls_not_lookups(recorder):
    recorder.mv_nms_f32, recorder.mv_erase  # fetched, as _filter_f32_u8's callers fetch both storage types' entries
    assert recorder.names == []
    assert recorder.mv_erase(1, 2, 3) == 0 and recorder.names == ["mv_erase"]


def test_no_wrapper_calls_the_entry_point_listed_as_such():
    import re
    from pathlib import Path
    sources = "".join(p.read_text() for p in Path(_lib.__file__).parent.glob("*.py") if p.name != "_lib.py")
    for name in CC.NO_WRAPPER:
        assert not re.search(rf"\blib\.{name}\b|getattr\([^)]*{name}", sources), name


def test_host_tables_are_uploaded_once_per_contents():
    """_lib.table_on: what keeps the decode wrappers and the float64 filter capturable when their tables come from the host."""
    a = torch.tensor([[1.5, 2.0], [3.0, 4.25]], dtype=torch.float64)
    first = _lib.table_on(a, torch.device("cpu"))
    assert first.dtype == torch.float32 and first.is_contiguous() and torch.equal(first, a.float())
    assert _lib.table_on(a.clone(), torch.device("cpu")) is first  # the same contents: no second upload
    assert _lib.table_on([a.clone()][0].t().contiguous().t(), torch.device("cpu")) is first  # whatever the strides
    other = _lib.table_on(a + 1, torch.device("cpu"))
    assert other is not first and torch.equal(other, (a + 1).float()) and torch.equal(first, a.float())
    assert _lib.table_on(a, torch.device("cpu"), torch.float64) is not first
    assert _lib.table_on(a.reshape(4), torch.device("cpu")).shape == (4,)
    assert _lib.table_on(a, torch.device("meta")).device.type == "meta"
    on_device = _lib.table_on(a.to("meta"), torch.device("meta"))  # a table that lies on a device is used, not read
    assert on_device.device.type == "meta" and on_device.dtype == torch.float32
    assert _lib.table_on(torch.zeros((0, 2)), torch.device("cpu")).shape == (0, 2)


def test_the_not_capturable_wrappers_do_read_back():
    """The reasons of the not-capturable table, checked against the sources they cite."""
    import inspect
    from cpu_vision_amd import ops
    assert "keep[:int(count.item())]" in inspect.getsource(ops._nms_impl)
    assert "int(flag.item())" in inspect.getsource(ops.masks_to_boxes)


@pytest.mark.parametrize("name", list(CC.cases()))
def test_the_second_seed_changes_every_input_and_the_reference(name):
    case = CC.cases()[name]
    d1, d2 = CC.inputs(case), CC.inputs(case, second=True)
    assert d1.keys() == d2.keys() and all(v is None or isinstance(v, (np.ndarray, list)) for v in d1.values()), name
    a1, a2 = CC.arrays(d1), CC.arrays(d2)
    assert a1 and [k for k, _ in a1] == [k for k, _ in a2]
    for (k, u), (_, v) in zip(a1, a2):
        assert u.shape == v.shape and u.dtype == v.dtype and not np.array_equal(u, v), (name, k)
    if isinstance(case, CC.Hand):  # no CPU reference here: the GPU test asserts that the two eager results differ
        return
    assert CC.references_differ(case), f"{name}: the two seeds give one reference"
