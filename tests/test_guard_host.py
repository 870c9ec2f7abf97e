"""tests/_guard.py catches what it is for, shown on CPU tensors with plain torch "kernels": a store one element in front of the
output, one behind it, an output element left unwritten and a read one element past the input each fail the corresponding
assertion; a correct kernel passes all of them.  No defect is ever planted on a GPU."""
import pytest
import torch

from tests import _guard as G

DTYPES = [torch.uint8, torch.int16, torch.int32, torch.int64, torch.float16, torch.float32, torch.float64]
NAN = float("nan")


def _values(n, dtype):
    g = torch.Generator().manual_seed(n)
    if dtype.is_floating_point:
        return torch.rand(n, generator=g).to(dtype)
    return torch.randint(40, 120, (n,), generator=g).to(dtype)


def _op(x):
    return x + x  # the "operation"; its reference is the same expression on the values themselves


def _run(kernel, dtype, n=37, x_off=3, y_off=5):
    """kernel(xbuf, x, ybuf, y): reads x, writes y (both views of their guarded buffers); then the four checks of a case."""
    values = _values(n, dtype)
    in_guard = NAN if dtype.is_floating_point else torch.tensor([0, 255]).to(dtype)
    xbuf, x = G.guarded(values, dtype, "cpu", x_off, sentinel=in_guard)
    ybuf, y = G.guarded((n,), dtype, "cpu", y_off)
    before = xbuf.clone()
    kernel(xbuf, x, ybuf, y)
    G.assert_same(y, _op(values), "result")
    G.assert_guards_intact(ybuf, y, what="output")
    G.assert_unchanged(xbuf, before, "input")


def _correct(xbuf, x, ybuf, y):
    y.copy_(_op(x))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_correct_kernel_passes(dtype):
    for x_off, y_off in ((G.ALIGNED, G.ALIGNED), (1, G.ALIGNED), (G.ALIGNED, 3), (37, 1)):
        _run(_correct, dtype, x_off=x_off, y_off=y_off)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_store_in_front_of_the_view_is_caught(dtype):
    def kernel(xbuf, x, ybuf, y):
        _correct(xbuf, x, ybuf, y)
        ybuf[G.GUARD_ELEMS + 5 - 1] = 1
    with pytest.raises(AssertionError, match=r"output: 1 guard element\(s\) changed, the first at index -1 "):
        _run(kernel, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_store_behind_the_view_is_caught(dtype):
    def kernel(xbuf, x, ybuf, y):
        _correct(xbuf, x, ybuf, y)
        ybuf[G.GUARD_ELEMS + 5 + y.numel()] = 1
    with pytest.raises(AssertionError, match=r"output: 1 guard element\(s\) changed, the first at index 37 "):
        _run(kernel, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_an_unwritten_last_element_is_caught(dtype):
    def kernel(xbuf, x, ybuf, y):
        y[:-1].copy_(_op(x[:-1]))
    with pytest.raises(AssertionError, match="result: 1 of 37 elements differ, first at flat index 36"):
        _run(kernel, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_read_past_the_input_is_caught(dtype):
    """A reduction that takes one element too many: the input's guards hold NaN (floats) or 0 / 255 around values drawn from
    [40, 120), so the range (max - min) it computes is not the reference's, whichever of the two the stray element is."""
    def stray(xbuf, x, ybuf, y):
        start = G.GUARD_ELEMS + x_off
        seen = xbuf[start:start + x.numel() + 1]
        y.fill_(seen.max() - seen.min())

    def good(xbuf, x, ybuf, y):
        y.fill_(x.max() - x.min())

    for x_off in (3, 4):  # the element behind the view: the pattern's 0, then its 255
        values = _values(37, dtype)
        in_guard = NAN if dtype.is_floating_point else torch.tensor([0, 255]).to(dtype)
        want = (values.max() - values.min()).expand(4).clone()
        for kernel, fails in ((good, False), (stray, True)):
            xbuf, x = G.guarded(values, dtype, "cpu", x_off, sentinel=in_guard)
            ybuf, y = G.guarded((4,), dtype, "cpu", 1)
            kernel(xbuf, x, ybuf, y)
            G.assert_guards_intact(ybuf, y, what="output")
            if fails:
                with pytest.raises(AssertionError, match="result: "):
                    G.assert_same(y, want, "result")
            else:
                G.assert_same(y, want, "result")


def test_a_store_into_the_input_is_caught():
    def kernel(xbuf, x, ybuf, y):
        _correct(xbuf, x, ybuf, y)
        xbuf[0] = 1
    with pytest.raises(AssertionError, match="input: the buffer changed, first at flat index 0"):
        _run(kernel, torch.float32)


def test_nan_results_compare_as_the_gpu_tests_do():
    want = torch.tensor([1.0, NAN, 3.0])
    G.assert_same(torch.tensor([1.0, NAN, 3.0]), want)
    with pytest.raises(AssertionError, match="NaN positions differ, first at flat index 2"):
        G.assert_same(torch.tensor([1.0, NAN, NAN]), want)
    with pytest.raises(AssertionError):
        G.assert_same(torch.tensor([1.0, NAN, 3.0], dtype=torch.float64), want)


def test_sentinels_and_patterns():
    for dtype in DTYPES:
        s = G.sentinel_for(dtype)
        buf, view = G.guarded((2, 3), dtype, "cpu", 1)
        assert buf.numel() == 2 * G.GUARD_ELEMS + 1 + 6 and view.shape == (2, 3)
        assert bool((buf == s).all()) and s != 0
        if not dtype.is_floating_point:
            assert s != -1 and s != torch.iinfo(dtype).max
    assert G.sentinel_for(torch.uint8) == 0xA5 and G.sentinel_for(torch.float32) == -7.25
    buf, view = G.guarded(torch.full((5,), 100, dtype=torch.uint8), torch.uint8, "cpu", 1, guard_elems=4,
                          sentinel=torch.tensor([0, 255]))
    assert buf.tolist() == [0, 255, 0, 255, 0, 100, 100, 100, 100, 100, 0, 255, 0, 255]
    G.assert_guards_intact(buf, view, torch.tensor([0, 255]), "pattern")
    buf[11] = 0
    with pytest.raises(AssertionError, match="the first at index 6 "):
        G.assert_guards_intact(buf, view, torch.tensor([0, 255]), "pattern")


def test_guarded_workspace():
    assert G.guarded_workspace(0, "cpu") == (None, None)
    buf, ws = G.guarded_workspace(48, "cpu", fill=0xFF)
    assert ws.numel() == 48 and ws.dtype == torch.uint8 and bool((ws == 0xFF).all())
    ws.zero_()
    G.assert_guards_intact(buf, ws, what="workspace")
    buf[G.GUARD_ELEMS + 48] = 0
    with pytest.raises(AssertionError, match="workspace: 1 guard element"):
        G.assert_guards_intact(buf, ws, what="workspace")


def test_guarded_workspace_at_a_byte_offset():
    """offset_bytes moves the workspace off its 256-byte boundary: still exactly nbytes bytes of `fill`, and the bytes between
    the boundary and the workspace are guard bytes like the rest."""
    buf, ws = G.guarded_workspace(40, "cpu", fill=0x00, offset_bytes=4)
    assert ws.numel() == 40 and bool((ws == 0).all())
    assert ws.storage_offset() - buf.storage_offset() == G.GUARD_ELEMS + 4 and buf.numel() == 2 * G.GUARD_ELEMS + 4 + 40
    G.assert_guards_intact(buf, ws, what="workspace")
    buf[G.GUARD_ELEMS + 3] = 0
    with pytest.raises(AssertionError, match=r"workspace: 1 guard element\(s\) changed, the first at index -1 "):
        G.assert_guards_intact(buf, ws, what="workspace")
    with pytest.raises(AssertionError):
        G.guarded_workspace(8, "cpu", offset_bytes=256)
