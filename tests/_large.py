"""Helpers of tests/test_gpu_large_offsets.py: where a contiguous tensor crosses element offset 2^31 and byte offsets 2^31 and
2^32, which rows to cut around those places, and the bookkeeping that proves the compared slices lie on both sides of each.

Nothing here touches the GPU except `fill`, which fills a big tensor on the device it lives on."""
from __future__ import annotations

from typing import Dict, Iterable, List, Sequence, Tuple

import torch

E31 = 2 ** 31  # element offset
B31 = 2 ** 31  # byte offsets
B32 = 2 ** 32


def crossings(numel: int, itemsize: int) -> Dict[str, int]:
    """The boundaries a contiguous tensor of `numel` elements of `itemsize` bytes crosses, as {name: e}: e is the flat index of the
    first element at or past the boundary, so elements e - 1 and e lie on its two sides.  A boundary at the very end is not
    crossed."""
    out = {}
    for name, e in (("element 2^31", E31), ("byte 2^31", B31 // itemsize), ("byte 2^32", B32 // itemsize)):
        if 0 < e < numel:
            out[name] = e
    return out


def fill(t: torch.Tensor, seed: int, lo=-1.0, hi=1.0) -> torch.Tensor:
    """Seeded values on the device, in pieces of 2^28 elements: floating tensors uniform in [lo, hi), integer ones in [lo, hi)."""
    g = torch.Generator(device=t.device).manual_seed(seed)
    flat = t.view(-1)
    for a in range(0, flat.numel(), 1 << 28):
        piece = flat[a:a + (1 << 28)]
        if t.dtype.is_floating_point:
            piece.uniform_(lo, hi, generator=g)
        else:
            piece.random_(int(lo), int(hi), generator=g)
    return t


def rows_near(e: int, width: int, rows_per_plane: int, reach: int = 1) -> List[int]:
    """Rows (inside their plane of rows_per_plane rows of `width` elements) within `reach` rows of the rows that hold flat
    elements e - 1 and e, clipped to the plane."""
    out = set()
    for q in (e - 1, e):
        r = (q // width) % rows_per_plane
        out.update(range(max(r - reach, 0), min(r + reach + 1, rows_per_plane)))
    return sorted(out)


def strips(rows: Iterable[int]) -> List[Tuple[int, int]]:
    """Sorted row numbers -> maximal runs [a, b)."""
    runs: List[List[int]] = []
    for r in sorted(set(rows)):
        if runs and runs[-1][1] == r:
            runs[-1][1] = r + 1
        else:
            runs.append([r, r + 1])
    return [(a, b) for a, b in runs]


def plane_ranges(planes: Sequence[int], rows_per_plane: int, width: int, a: int, b: int) -> List[Tuple[int, int]]:
    """Flat element ranges [lo, hi) of rows [a, b) of each of `planes` in a contiguous (P, rows_per_plane, width) tensor."""
    return [((p * rows_per_plane + a) * width, (p * rows_per_plane + b) * width) for p in planes]


def assert_straddles(ranges: Sequence[Tuple[int, int]], e: int, what: str) -> None:
    """The flat ranges that were compared hold element e - 1 and element e: both sides of the boundary `what`."""
    below = any(lo <= e - 1 < hi for lo, hi in ranges)
    above = any(lo <= e < hi for lo, hi in ranges)
    assert below and above, f"{what}: compared ranges do not straddle flat element {e} (below {below}, above {above})"


def describe(ranges: Sequence[Tuple[int, int]], itemsize: int) -> str:
    """The compared flat ranges as text: element and byte offsets of the lowest and highest."""
    lo, hi = min(r[0] for r in ranges), max(r[1] for r in ranges)
    return f"{len(ranges)} ranges, elements [{lo}, {hi}), bytes [{lo * itemsize}, {hi * itemsize})"


# ---- ops whose output rows depend on a few input rows of the same plane ---------------------------------------------------------------
# A cut maps output rows [a, b) of a plane with `rin` input rows to (lo, hi, drop, first): run the op on input rows [lo, hi), throw
# away its first `drop` output rows (their windows reach outside the cut), keep the next b - a; `first` is the first input row the
# kept outputs read (hi - 1 is the last).
def cut_same(a: int, b: int, rin: int):
    return a, b, 0, a


def cut_pool2(a: int, b: int, rin: int):  # kernel 2, stride 2
    return 2 * a, 2 * b, 0, 2 * a


def cut_pool3s2(a: int, b: int, rin: int):  # kernel 3, stride 2, no padding: output o reads rows 2o .. 2o + 2
    return 2 * a, 2 * b + 1, 0, 2 * a


def cut_pool3s2p1(a: int, b: int, rin: int):  # kernel 3, stride 2, padding 1: output o reads rows 2o - 1 .. 2o + 1 inside the plane
    lo = max(2 * a - 2, 0)  # an even row, so that the cut's windows fall where the plane's do
    return lo, min(2 * b, rin), (1 if a > 0 else 0), max(2 * a - 1, 0)


def cut_conv3(a: int, b: int, rin: int):  # 3 x 3, stride 1, padding 1
    lo = max(a - 1, 0)
    return lo, min(b + 1, rin), a - lo, lo


def pick_rows(planes: int, rin: int, win: int, in_item: int, rout: int, wout: int, out_item: int,
              scale: int = 1, reach: int = 1) -> Dict[int, List[Tuple[int, int]]]:
    """Which output rows of which planes to compare with the reference, as {plane: [(a, b), ...]}: the first two rows of the first
    plane, the last two of the last, and the rows within `reach` rows of every boundary the output (planes, rout, wout) crosses and
    of the outputs that read the input rows at every boundary the input (planes, rin, win) crosses (input row r feeds output row
    r // scale and its neighbours)."""
    picks: Dict[int, set] = {}

    def add(p, rows):
        picks.setdefault(p, set()).update(r for r in rows if 0 <= r < rout)

    add(0, range(0, reach + 1))
    add(planes - 1, range(rout - 1 - reach, rout))
    for e in crossings(planes * rout * wout, out_item).values():
        for q in (e - 1, e):
            p, r = divmod(q // wout, rout)
            add(p, range(r - reach, r + reach + 1))
    for e in crossings(planes * rin * win, in_item).values():
        for q in (e - 1, e):
            p, r = divmod(q // win, rin)
            o = min(r // scale, rout - 1)
            add(p, range(o - reach, o + reach + 1))
    return {p: strips(rows) for p, rows in sorted(picks.items())}


def compared_ranges(picks, cut, rin: int, win: int, rout: int, wout: int):
    """(output ranges, input ranges): the flat element ranges of the picked output rows and of the input rows they read."""
    out_ranges, in_ranges = [], []
    for p, runs in picks.items():
        for a, b in runs:
            _, hi, _, first = cut(a, b, rin)
            out_ranges += plane_ranges([p], rout, wout, a, b)
            in_ranges += plane_ranges([p], rin, win, first, hi)
    return out_ranges, in_ranges


def assert_crossings_straddled(picks, cut, planes: int, rin: int, win: int, in_item: int, rout: int, wout: int, out_item: int,
                               need=()) -> str:
    """Every boundary the input and the output cross lies inside what `picks` compares; `need` names boundaries the case exists
    for ("input element 2^31", "output byte 2^32", ...), which must be among them.  Returns a description for failure messages."""
    out_ranges, in_ranges = compared_ranges(picks, cut, rin, win, rout, wout)
    crossed = []
    for side, ranges, numel, item in (("input", in_ranges, planes * rin * win, in_item), ("output", out_ranges, planes * rout * wout, out_item)):
        for name, e in crossings(numel, item).items():
            assert_straddles(ranges, e, f"{side} {name}")
            crossed.append(f"{side} {name}")
    for name in need:
        assert name in crossed, f"the case does not cross {name}: {crossed}"
    return f"output {describe(out_ranges, out_item)}; input {describe(in_ranges, in_item)}; crossed: {crossed}"
