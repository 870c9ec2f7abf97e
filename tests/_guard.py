"""Guard bands for tests that call a kernel through the C ABI: a tensor is placed at a chosen element offset inside a larger
flat buffer whose remaining elements hold a sentinel, so that a store before the tensor, a store past its end, an element the
kernel never wrote and (with guards whose values would change the result) a stray read all become visible to the test.

A helper module, not a conftest and without fixtures; it works on any device (tests/test_guard_host.py runs it on the CPU).

  buf, view = guarded(values_or_shape, dtype, device, offset_elems)   the buffer and the contiguous tensor inside it
  assert_guards_intact(buf, view, sentinel, what)                     nothing outside the view changed
  assert_unchanged(buf, before, what)                                  an input buffer still holds the bits of `before`
  assert_same(got, want, what)                                         the NaN-aware equality of test_gpu_autoaug._same
  guarded_workspace(nbytes, device, fill, offset_bytes=0)              exactly nbytes bytes, offset_bytes past a 256-byte
                                                                       boundary, guarded

A sentinel is a scalar or a 1-D pattern that is repeated over the guard (index 0 of the pattern at element 0 of the buffer).
Output views are pre-filled with the sentinel too: equality with the reference then proves that every element was written.
"""
import torch

GUARD_ELEMS = 1024
ALIGNED = 64  # an element offset that keeps every element type 16-byte aligned

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
# 1-byte types 0xA5 and floats -7.25, as tests/test_gpu_warp.py::test_canary_ragged_widths; wider integers a fixed bit
# pattern that is neither 0 nor all ones
_INT_SENTINELS = {torch.uint8: 0xA5, torch.int8: 0xA5 - 256, torch.int16: 0x5AA5, torch.int32: 0x5AA5C33C,
                  torch.int64: 0x5AA5C33C0FF0A55A}
FLOAT_SENTINEL = -7.25


def sentinel_for(dtype):
    if dtype.is_floating_point:
        return FLOAT_SENTINEL
    if dtype == torch.bool:
        return True
    return _INT_SENTINELS[dtype]


def _fill(n, dtype, sentinel):
    """n elements of the sentinel (a scalar, or a 1-D pattern repeated from index 0) on the CPU."""
    if isinstance(sentinel, torch.Tensor) and sentinel.ndim == 1:
        reps = (n + sentinel.numel() - 1) // sentinel.numel()
        return sentinel.to(dtype).repeat(reps)[:n].clone()
    return torch.full((n,), sentinel, dtype=dtype)


def _bits(t):
    """The tensor's elements as integers of the same width: NaN sentinels compare equal to themselves."""
    t = t.contiguous()
    return t if t.dtype == torch.bool else t.view(_BITS[t.element_size()])


def guarded(values_or_shape, dtype, device, offset_elems, guard_elems=GUARD_ELEMS, sentinel=None):
    """-> (buf, view): `buf` is a flat tensor of guard_elems + offset_elems + n + guard_elems elements filled with the sentinel,
    `view` the contiguous tensor at element offset guard_elems + offset_elems in it -- a copy of `values_or_shape` when that
    is a tensor (an input), otherwise a tensor of that shape still holding the sentinel (an output)."""
    if sentinel is None:
        sentinel = sentinel_for(dtype)
    values = values_or_shape if isinstance(values_or_shape, torch.Tensor) else None
    shape = tuple(values.shape) if values is not None else tuple(values_or_shape)
    n = 1
    for s in shape:
        n *= int(s)
    start = guard_elems + offset_elems
    host = _fill(start + n + guard_elems, dtype, sentinel)
    if values is not None:
        assert values.dtype == dtype, (values.dtype, dtype)
        host[start:start + n] = values.detach().cpu().reshape(-1)
    buf = host.to(device)
    view = buf[start:start + n].view(shape)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + start * buf.element_size()
    return buf, view


def _span(buf, view):
    start = view.storage_offset() - buf.storage_offset()
    assert view.is_contiguous() and 0 <= start and start + view.numel() <= buf.numel(), "the view does not lie in the buffer"
    return start, view.numel()


def assert_guards_intact(buf, view, sentinel=None, what=""):
    """One host copy of `buf`; every element before and after `view` still holds the sentinel.  A failure names the first
    changed element by its index relative to the view (negative: in front of it; >= view.numel(): behind it)."""
    if sentinel is None:
        sentinel = sentinel_for(buf.dtype)
    start, n = _span(buf, view)
    host = _bits(buf.detach().cpu())
    want = _bits(_fill(buf.numel(), buf.dtype, sentinel))
    changed = host != want
    changed[start:start + n] = False
    if bool(changed.any()):
        first = int(changed.nonzero()[0])
        where = "before" if first < start else "after"
        raise AssertionError(f"{what}: {int(changed.sum())} guard element(s) changed, the first at index {first - start} relative to "
                             f"the view of {n} elements ({where} it): {buf.detach().cpu()[first].item()!r}")


def assert_unchanged(buf, before, what=""):
    """`buf` (an input with its guards, or anything else a kernel must not write) still holds the bits of the host copy `before`."""
    now, was = _bits(buf.detach().cpu()), _bits(before)
    if not torch.equal(now, was):
        first = int((now != was).nonzero()[0])
        raise AssertionError(f"{what}: the buffer changed, first at flat index {first}")


def assert_same(got, want, what=""):
    """tests/test_gpu_autoaug.py `_same` with a message: dtype and shape, the NaN positions, and equality everywhere else."""
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.is_floating_point():
        nan = torch.isnan(want)
        if not torch.equal(torch.isnan(got), nan):
            first = int((torch.isnan(got) != nan).reshape(-1).nonzero()[0])
            raise AssertionError(f"{what}: NaN positions differ, first at flat index {first} of {got.numel()}")
        got, want = got[~nan], want[~nan]
    if not torch.equal(got, want):
        bad = (got != want).reshape(-1)
        first = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at flat index {first}: got "
                             f"{got.reshape(-1)[first].item()!r}, want {want.reshape(-1)[first].item()!r}")


def guarded_workspace(nbytes, device, fill=0xFF, guard_bytes=GUARD_ELEMS, offset_bytes=0):
    """-> (buf, ws): a workspace of exactly `nbytes` bytes holding `fill`, `offset_bytes` (< 256; 0: 256-byte aligned) past a
    256-byte aligned position of a byte buffer whose guards hold the 1-byte sentinel; (None, None) when nbytes == 0."""
    if not nbytes:
        return None, None
    assert guard_bytes % 256 == 0 and 0 <= offset_bytes < 256
    buf, ws = guarded((int(nbytes),), torch.uint8, device, offset_bytes, guard_elems=guard_bytes)
    assert buf.device.type == "cpu" or ws.data_ptr() % 256 == offset_bytes
    ws.fill_(fill)
    return buf, ws
