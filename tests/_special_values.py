"""Helpers of tests/test_special_values_host.py and tests/test_gpu_special_values.py: where to put a NaN or an Inf inside a
tensor (poison_sites), which outputs may see it (footprint), and the comparison that treats NaN as a value (assert_same_values).

The kernels under test pad K chunks, channel tiles, ragged right edges and stacked images, and some of them stage cells of the
neighbouring channel, row or image and cancel the surplus with a zero operand.  That is exact for finite data; 0 x Inf and
0 x NaN are NaN.  The sites below are the cells such a kernel over-reads: the two sides of every boundary its tiling crosses.
footprint() is geometry alone -- kernel size, stride, padding, dilation, groups, border mode -- so the locality test needs no
oracle: an output outside the footprint of the one poisoned cell keeps its bits.

Plain numpy: no fixtures, no device code."""
import numpy as np

NAN, PINF, NINF = np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)
TINY32 = np.finfo(np.float32).tiny  # 2^-126, the smallest normal float32


# ---- sites -------------------------------------------------------------------------------------------------------------------------
def poison_sites(shape, plan=None):
    """{name: index tuple} of the cells of a tensor of `shape` that tiled kernels over-read, in priority order (a dict keeps it).

    shape (n, c, h, w), (planes, h, w) or (h, w): an image tensor; (n, k): a matrix of rows.  plan (all keys optional):
      slice=<int>      channels (or k) per K slice where the library states more than one (the *_k_slices queries): the cell on
                       each side of the first and of the last slice boundary
      radius=(ry, rx)  tap radius of a filter with a reflecting border: a cell closer to the top-left corner than the radius,
                       which the reflection reads twice
      image=<int>      the image i whose last row / last channel is paired with image i + 1's first (default 0)
    Names: pair_a / pair_b (neighbours in one row -- of a matrix, the last two elements of the last row -- so that one receptive
    field holds both), first, last, ragged_last / ragged_left (the
    last column of a row and the one left of it), row_last_i / row_first_next (last row of image i, first row of image i + 1),
    chan_last_i / chan_first_next (channel c - 1 of image i, channel 0 of image i + 1), slice_lo / slice_hi (+ _end for the last
    boundary), mirrored."""
    plan = dict(plan or {})
    shape = tuple(int(d) for d in shape)
    sites = {}
    if len(shape) == 2 and plan.get("matrix"):
        n, k = shape
        sites["pair_a"] = (n - 1, k - 1)  # the last element
        if k >= 2:
            sites["pair_b"] = (n - 1, k - 2)
        sites["first"] = (0, 0)
        if k % 4:
            sites["ragged_left"] = (n // 2, k - k % 4)  # the first k of the ragged 4-k stage
        sl = plan.get("slice")
        if sl and sl < k:
            bounds = sorted({sl, ((k - 1) // sl) * sl})
            for tag, b in zip(("", "_end"), bounds):
                sites["slice_lo" + tag] = (n // 2, b - 1)
                sites["slice_hi" + tag] = (n // 2, b)
        return sites
    lead, (h, w) = shape[:-2], shape[-2:]
    if len(lead) == 2:
        n, c = lead
    else:
        n, c = (lead[0] if lead else 1), None
    at = lambda i, ch, y, x: ((i, ch, y, x) if c is not None else ((i, y, x) if lead else (y, x)))  # noqa: E731
    cy, cx = h // 2, w // 2
    last_c = (c - 1) if c is not None else 0
    if w >= 2:
        sites["pair_a"] = at(0, 0, cy, max(cx, 1))
        sites["pair_b"] = at(0, 0, cy, max(cx, 1) - 1)
    elif c is not None and c >= 2:  # one column: the pair lies in two channels of one pixel (one field of a dense conv)
        sites["pair_a"] = at(0, 0, cy, 0)
        sites["pair_b"] = at(0, 1, cy, 0)
    sites["last"] = at(n - 1, last_c, h - 1, w - 1)
    sites["first"] = at(0, 0, 0, 0)
    sites["ragged_last"] = at(n - 1, 0, cy, w - 1)
    if w >= 2:
        sites["ragged_left"] = at(n - 1, 0, cy, w - 2)
    i = int(plan.get("image", 0))
    if n >= i + 2:
        sites["row_last_i"] = at(i, last_c, h - 1, cx)
        sites["row_first_next"] = at(i + 1, 0, 0, cx)
        if c is not None:
            sites["chan_last_i"] = at(i, c - 1, cy, cx)
            sites["chan_first_next"] = at(i + 1, 0, cy, cx)
    elif c is not None and c >= 2:
        sites["chan_last_i"] = at(0, c - 1, cy, cx)
    sl = plan.get("slice")
    if c is not None and sl and sl < c:
        bounds = sorted({sl, ((c - 1) // sl) * sl})
        for tag, b in zip(("", "_end"), bounds):
            sites["slice_lo" + tag] = at(n - 1, b - 1, cy, cx)
            sites["slice_hi" + tag] = at(n - 1, b, cy, cx)
    if plan.get("radius"):
        ry, rx = plan["radius"]
        sites["mirrored"] = at(0, 0, min(max(ry - 1, 0), h - 1), min(max(rx - 1, 0), w - 1))
    return sites


# ---- footprints --------------------------------------------------------------------------------------------------------------------
def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * (n - 1) - i if i >= n else i


def _axis_reach(pos, size, out, k, stride, pad, dil, border):
    """Boolean (out,): the outputs o of one axis with a tap t for which the source index of (o, t) is `pos`."""
    reach = np.zeros(out, bool)
    for o in range(out):
        for t in range(k):
            s = o * stride - pad + t * dil
            if border == "reflect":
                s = _reflect(s, size)
            if s == pos:
                reach[o] = True
    return reach


def conv_out_hw(h, w, k, stride, pad, dil):
    return ((h + 2 * pad[0] - (dil[0] * (k[0] - 1) + 1)) // stride[0] + 1, (w + 2 * pad[1] - (dil[1] * (k[1] - 1) + 1)) // stride[1] + 1)


def footprint(site, geometry):
    """Boolean mask, shaped like the output, of the outputs whose receptive field contains the input cell `site`.

    geometry["op"]:
      "conv"      in_shape (n, cin, h, w), cout, k, stride, pad, dil (pairs), groups; zero padding.  Output (n, cout, oh, ow): the
                  channels of the site's group, the rows and columns with a tap on the site.
      "filter"    in_shape (..., h, w), k (ky, kx), border "reflect" | "zero" | "valid".  One plane in, the same plane out; with
                  "reflect" a cell near the border is read through its mirror image as well.
      "linear"    in_shape (n, k), m.  Output (n, m): the site's row.
                  then=(ky2, kx2): a second filter applied to the first one's result (Gaussian, then Sobel).
      "sharpness" in_shape (..., h, w): the 3 x 3 neighbours of the site that are interior pixels, and the site itself.
      "avgpool"   in_shape (..., h, w), out (oh, ow): torch's adaptive bins [floor(i * h / oh), ceil((i + 1) * h / oh)).
      "transpose" in_shape (n, cin, h, w), cout, k, stride (ints), pad: ConvTranspose2d, output (n, cout, (h-1)*s - 2p + k, ...);
                  input cell y reaches outputs y * s - p + t, t < k.
      "pointwise" in_shape any: the output cell of the same index (elementwise ops).
      "channel"   out_shape (n, cout, oh, ow), site (channel,): a per-channel epilogue term (bias, alpha, beta)."""
    op = geometry["op"]
    site = tuple(int(v) for v in site)
    if op == "linear":
        n, _ = geometry["in_shape"]
        mask = np.zeros((n, geometry["m"]), bool)
        mask[site[0], :] = True
        return mask
    if op == "pointwise":
        mask = np.zeros(geometry["in_shape"], bool)
        mask[site] = True
        return mask
    if op == "channel":
        mask = np.zeros(geometry["out_shape"], bool)
        if len(mask.shape) == 2:
            mask[:, site[0]] = True
        else:
            mask[:, site[0], ...] = True
        return mask
    if op == "conv":
        n, cin, h, w = geometry["in_shape"]
        cout, k, stride, pad, dil, groups = geometry["cout"], geometry["k"], geometry["stride"], geometry["pad"], geometry["dil"], geometry["groups"]
        oh, ow = conv_out_hw(h, w, k, stride, pad, dil)
        img, c, y, x = site
        ry = _axis_reach(y, h, oh, k[0], stride[0], pad[0], dil[0], "zero")
        rx = _axis_reach(x, w, ow, k[1], stride[1], pad[1], dil[1], "zero")
        g = c // (cin // groups)
        mask = np.zeros((n, cout, oh, ow), bool)
        mg = cout // groups
        mask[img, g * mg:(g + 1) * mg] = np.outer(ry, rx)
        return mask
    if op in ("pixel", "image", "plane"):
        # colour ops on (n, c, h, w): a cell reaches its pixel in every channel (grey value, hue), its whole image (the contrast
        # mean) or its (image, channel) plane (autocontrast's minimum and maximum)
        mask = np.zeros(geometry["in_shape"], bool)
        if op == "pixel":
            mask[site[0], :, site[2], site[3]] = True
        elif op == "image":
            mask[site[0]] = True
        else:
            mask[site[0], site[1]] = True
        return mask
    if op == "sample":
        # grid sampling of (n, c, h, w): `ix`, `iy` (oh, ow) float32 source pixel coordinates of every output, mode "bilinear"
        # (the four cells around the sample that lie in the image, with weight 0 too) or "nearest" (the cell at the coordinates
        # rounded half to even).  A NaN or infinite coordinate reads no cell.
        n, c, h, w = geometry["in_shape"]
        ix, iy = np.asarray(geometry["ix"], np.float32), np.asarray(geometry["iy"], np.float32)
        img, ch, y, x = site
        with np.errstate(invalid="ignore"):
            if geometry["mode"] == "nearest":
                hit = (np.rint(ix) == x) & (np.rint(iy) == y)
            else:
                x0, y0 = np.floor(ix), np.floor(iy)
                hit = ((x0 == x) | (x0 + 1 == x)) & ((y0 == y) | (y0 + 1 == y))
        mask = np.zeros((n, c) + ix.shape, bool)
        mask[img, ch] = hit
        return mask
    if op == "resize":
        # antialiased bilinear resize of (..., h, w) to out (oh, ow): per axis the source range of an output,
        # [int(centre - support + 0.5), int(centre + support + 0.5)) clipped to the axis, centre = scale (o + 0.5), in float32
        shape = tuple(geometry["in_shape"])
        h, w = shape[-2:]
        oh, ow = geometry["out"]

        def reach(pos, size, out):
            f = np.float32
            scale = f(size) / f(out)
            support = scale if scale >= 1 else f(1)
            r = np.zeros(out, bool)
            for o in range(out):
                centre = f(float(scale) * (o + 0.5))
                lo = max(int(f(centre - support) + f(0.5)), 0)
                hi = min(int(f(centre + support) + f(0.5)), size)
                r[o] = lo <= pos < hi
            return r
        mask = np.zeros(shape[:-2] + (oh, ow), bool)
        mask[site[:-2]] = np.outer(reach(site[-2], h, oh), reach(site[-1], w, ow))
        return mask
    if op == "deform":
        # deformable conv: the cells a tap samples depend on the offsets.  in_shape, cout, k, stride, pad, dil, groups, og and
        # `offset` (n, 2 og kh kw, oh, ow) float32.  A sample at (yy, xx) inside (-1, h) x (-1, w) reads the four cells around it
        # that lie in the image -- with weight 0 as well, when it falls on a row or column exactly.  float32 as the op states it.
        n, cin, h, w = geometry["in_shape"]
        cout, k, stride, pad, dil, groups, og = (geometry[key] for key in ("cout", "k", "stride", "pad", "dil", "groups", "og"))
        off = np.asarray(geometry["offset"], np.float32)
        oh, ow = off.shape[-2:]
        img, c, y, x = site
        g_off = c // (cin // og)
        hit = np.zeros((oh, ow), bool)
        base_y = (np.arange(oh) * stride[0] - pad[0]).astype(np.float32)[:, None]
        base_x = (np.arange(ow) * stride[1] - pad[1]).astype(np.float32)[None, :]
        for i in range(k[0]):
            for j in range(k[1]):
                t = (g_off * k[0] * k[1] + i * k[1] + j) * 2
                yy = (base_y + np.float32(i * dil[0])) + off[img, t]
                xx = (base_x + np.float32(j * dil[1])) + off[img, t + 1]
                inside = ~((yy <= -1) | (yy >= h) | (xx <= -1) | (xx >= w))
                y0, x0 = np.floor(yy), np.floor(xx)
                hit |= inside & ((y0 == y) | (y0 + 1 == y)) & ((x0 == x) | (x0 + 1 == x))
        mask = np.zeros((n, cout, oh, ow), bool)
        gw, mg = c // (cin // groups), cout // groups
        mask[img, gw * mg:(gw + 1) * mg] = hit
        return mask
    if op == "transpose":
        n, cin, h, w = geometry["in_shape"]
        cout, k, s, p = geometry["cout"], geometry["k"], geometry["stride"], geometry["pad"]
        oh, ow = (h - 1) * s - 2 * p + k, (w - 1) * s - 2 * p + k
        img, c, y, x = site
        ry, rx = np.zeros(oh, bool), np.zeros(ow, bool)
        for t in range(k):
            if 0 <= y * s - p + t < oh:
                ry[y * s - p + t] = True
            if 0 <= x * s - p + t < ow:
                rx[x * s - p + t] = True
        mask = np.zeros((n, cout, oh, ow), bool)
        mask[img] = np.outer(ry, rx)
        return mask
    shape = tuple(geometry["in_shape"])
    h, w = shape[-2:]
    lead, (y, x) = site[:-2], site[-2:]
    if op == "filter":
        ky, kx = geometry["k"]
        border = geometry["border"]
        if border == "valid":
            oh, ow, py, px = h - ky + 1, w - kx + 1, 0, 0
        else:
            oh, ow, py, px = h, w, ky // 2, kx // 2
        ry = _axis_reach(y, h, oh, ky, 1, py, 1, border)
        rx = _axis_reach(x, w, ow, kx, 1, px, 1, border)
        if geometry.get("then"):  # a second filter of the first one's result, same border: every cell the first reaches, again
            ky2, kx2 = geometry["then"]
            ry = np.any([_axis_reach(p, oh, oh, ky2, 1, ky2 // 2, 1, border) for p in np.flatnonzero(ry)], axis=0)
            rx = np.any([_axis_reach(p, ow, ow, kx2, 1, kx2 // 2, 1, border) for p in np.flatnonzero(rx)], axis=0)
    elif op == "sharpness":
        # adjust_sharpness: interior pixels blend x with a 3 x 3 smoothing of x; the one-pixel border is x itself
        oh, ow = h, w
        ry = np.array([abs(i - y) <= 1 and 0 < i < h - 1 for i in range(h)])
        rx = np.array([abs(j - x) <= 1 and 0 < j < w - 1 for j in range(w)])
        mask = np.zeros(shape, bool)
        mask[lead] = np.outer(ry, rx)
        mask[site] = True
        return mask
    elif op == "avgpool":
        oh, ow = geometry["out"]
        ry = np.array([(i * h) // oh <= y < -((-(i + 1) * h) // oh) for i in range(oh)])
        rx = np.array([(j * w) // ow <= x < -((-(j + 1) * w) // ow) for j in range(ow)])
    else:
        raise ValueError(op)
    mask = np.zeros(shape[:-2] + (oh, ow), bool)
    mask[lead] = np.outer(ry, rx)
    return mask


def choose_sites(candidates, budget=0.5):
    """candidates: [(key, footprint mask)] in priority order.  -> the keys whose footprints together stay within `budget` of the
    outputs: small shapes cannot hold every site and still leave half of the result finite.  The first candidate is taken
    regardless, and so is the second if it adds no output to the union (pair_b in pair_a's row of a matrix, or plane of a global
    pool); any later one that adds no output is left out -- it would only mix further values into fields that are taken."""
    chosen, union = [], None
    for key, fp in candidates:
        new = fp if union is None else (union | fp)
        grows = union is None or new.sum() > union.sum()
        if union is None or (grows and new.mean() <= budget) or (len(chosen) == 1 and not grows):
            chosen.append(key)
            union = new
    return chosen


VALUES = (PINF, NINF, PINF, NAN, NINF)


def poisoned(a, sites, values=VALUES):
    """A copy of `a` with the sites set to +Inf, -Inf, +Inf, NaN, -Inf in turn: the first two are pair_a and pair_b, which get opposite
    infinities, so that Inf - Inf occurs inside one receptive field; the third is an Inf alone in its field."""
    out = np.array(a, copy=True)
    for i, site in enumerate(sites.values()):
        out[tuple(site)] = values[i % len(values)]
    return out


# ---- comparison ----------------------------------------------------------------------------------------------------------------------
def assert_same_values(got, want, what=""):
    """got == want as values: the NaN positions agree first; everywhere else `==`, so the sign of an Inf counts and a value one
    ulp off fails.  The sign of a zero is deliberately NOT asserted (-0 == +0, as np.testing.assert_array_equal has it): the
    layer kernels add the bias as a last MFMA tap through a 0 / 1 selector, which adds +0 where there is no bias, and
    (-0) + (+0) is +0.  The payload and sign of a NaN are not asserted either: IEEE 754 leaves them to the implementation."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} vs {want.dtype}"
    gn, wn = np.isnan(got), np.isnan(want)
    if (gn != wn).any():
        i = tuple(int(v) for v in np.argwhere(gn != wn)[0])
        raise AssertionError(f"{what}: NaN where the reference has none or the reverse at {int((gn != wn).sum())} of {got.size} positions; "
                             f"first at {i}: got {got[i]!r}, want {want[i]!r}")
    bad = ~wn & (got != want)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} values differ; first at {i}: got {got[i]!r}, want {want[i]!r}")


def same_bits(a, b):
    """Elementwise: the same value bit for bit (NaN equal to NaN of the same payload)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.view(u) == b.view(u)


def assert_local(clean, dirty, mask, what=""):
    """The locality property: outside `mask` the two results are bit-identical, inside it at least one element differs.  An
    empty mask (a cell that a strided or dilated window never reads) means that nothing changes at all."""
    clean, dirty = np.asarray(clean), np.asarray(dirty)
    assert clean.shape == dirty.shape == mask.shape, f"{what}: shapes {clean.shape}, {dirty.shape}, footprint {mask.shape}"
    same = same_bits(clean, dirty)
    leaked = ~same & ~mask
    if leaked.any():
        i = tuple(int(v) for v in np.argwhere(leaked)[0])
        raise AssertionError(f"{what}: {int(leaked.sum())} outputs outside the site's receptive field changed; first at {i}: "
                             f"{clean[i]!r} -> {dirty[i]!r}")
    assert not mask.any() or not same[mask].all(), f"{what}: no output inside the site's receptive field changed"


# ---- conditions on a reference result (tests/test_special_values_host.py) -------------------------------------------------------------
def is_subnormal(a):
    a = np.asarray(a)
    return (a != 0) & np.isfinite(a) & (np.abs(a) < np.finfo(a.dtype).tiny)


def placement_conditions(want, what="", inf=True):
    """inf=False: an op that clamps before its output (ReLU6 inside a block without a residual) turns every Inf finite."""
    want = np.asarray(want)
    assert np.isnan(want).any(), f"{what}: the reference result holds no NaN"
    assert not inf or np.isinf(want).any(), f"{what}: the reference result holds no Inf"
    assert np.isfinite(want).mean() >= 0.5, f"{what}: only {np.isfinite(want).mean():.2f} of the reference result is finite"


def subnormal_conditions(want, what="", inputs=None):
    """inputs: for an op whose outputs are normal whatever the inputs are, the condition is on `inputs` instead."""
    want = np.asarray(want if inputs is None else inputs)
    nz = want != 0
    assert nz.any(), f"{what}: the reference result is all zero"
    frac = is_subnormal(want).sum() / nz.sum()
    assert frac >= 0.25, f"{what}: only {frac:.2f} of the non-zero reference outputs are subnormal"


def overflow_conditions(want, what=""):
    want = np.asarray(want)
    assert np.isinf(want).any(), f"{what}: no chain of the reference overflows"
    assert np.isfinite(want).mean() >= 0.5, f"{what}: only {np.isfinite(want).mean():.2f} of the reference result is finite"
