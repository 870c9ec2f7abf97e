"""Guard-band sweeps of the pointwise image kernels at the C ABI (`-m gpu`): csrc/color.hip, autoaug.hip, crop.hip,
batchmix.hip and the source window of resize.hip, called the way tests/test_gpu_warp.py::test_canary_ragged_widths calls
mv_warp_*.  The Python API always hands these kernels a fresh, 256-byte aligned torch.empty; here input, output and workspace
each lie inside a sentinel-filled buffer (tests/_guard.py) at 16-byte aligned and at odd element offsets, at the sizes where the
kernels' chunking (256 lanes x V = 16 / elem_bytes elements x kItems groups, rows sharing a workgroup, the flat / walk
threshold) changes.  Every case asserts that

  1. the result equals the reference of that op (tests/_color_ref.py, _autoaug_ref.py, _crop_ref.py, _mix_ref.py), compared
     as tests/test_gpu_autoaug.py `_same` does: no tolerance;
  2. nothing outside the output changed (it is pre-filled with the sentinel, so equality also proves it was written whole);
  3. the input buffer -- whose guards hold NaN, or 0 / 255 around pixels drawn from [40, 200], or a value absent from the
     image, so that a stray read would change the result -- is unchanged, guards included;
  4. the workspace's guards are intact, and a second run on 0x00 instead of 0xFF garbage gives the same bits.

mv_pad_crop_flip / mv_erase run with planes = 6, channels = 3 (the entry points require planes % channels == 0; plane p takes
channel p % 3, which wraps once)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd._color import _blend_form  # noqa: E402
from oracle import ref as oracle  # noqa: E402
from tests import _crop_ref as CR, _guard as G, _mix_ref as MR  # noqa: E402
from tests._autoaug_ref import REF_OPS as AA_REF  # noqa: E402
from tests._color_ref import (REF_OPS as COLOR_REF, check_contrast_reference, emu_chain, emu_grayscale,  # noqa: E402
                              ref_chain, ref_rgb_to_grayscale)
from tests.test_gpu_warp import assert_matches_reference  # noqa: E402

DEV = "cuda"
A = G.ALIGNED
NAN = float("nan")
U8, F32 = torch.uint8, torch.float32
LAM = 0.6180339887498949


class _OnDevice:
    device = torch.device(DEV)


def _stream():
    return _lib.stream_ptr(_OnDevice)  # the current stream of the device the guarded buffers live on


def _alignments(elem_bytes):
    """(x_offset, y_offset) in elements: both 16-byte aligned, then either or both at an odd element."""
    cases = [(A, A)]
    for odd in ((1, 37) if elem_bytes == 1 else (1, 3)):
        cases += [(odd, A), (A, odd), (odd, odd)]
    return cases


def _aligned(xo, yo):
    return xo == A and yo == A


def _in_guard(dtype):
    """What surrounds an input: NaN for floats, alternating 0 / 255 for uint8, the dtype's sentinel for wider integers (the
    images below never contain it)."""
    if dtype.is_floating_point:
        return NAN
    return torch.tensor([0, 255]) if dtype == U8 else G.sentinel_for(dtype)


def _pixels(shape, dtype, seed):
    """uint8 in [40, 200], float32 in [40 / 255, 200 / 255]: a stray 0, 255 or NaN moves min, max, histogram and mean."""
    g = torch.Generator().manual_seed(seed)
    if dtype == U8:
        return torch.randint(40, 201, shape, generator=g, dtype=U8)
    return torch.rand(shape, generator=g) * (160.0 / 255.0) + 40.0 / 255.0


def _elements(shape, dtype, seed):
    """What the byte movers and MixUp carry: any value but the one in the input's guards."""
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        return (torch.rand(shape, generator=g) * 4 - 2).to(dtype)
    hi = {1: 256, 2: 1000, 4: 1 << 30, 8: 1 << 40}[dtype.itemsize]
    x = torch.randint(0, hi, shape, generator=g).to(dtype)
    if dtype == U8:
        x[x == G.sentinel_for(U8)] = 0x3C
    return x


def _factor(hw):
    """(h, w) with h > 1 where hw allows it."""
    for h in (8, 3, 2):
        if hw % h == 0 and hw > h:
            return h, hw // h
    return 1, hw


def _run(what, call, x, x_off, y_shape, y_dtype, y_off, want, ws_bytes=0, x_guard=None):
    """One case: call(x_ptr, y_ptr, ws_ptr, ws_bytes) -> status on guarded buffers, then the four assertions.  With a workspace
    the call runs twice, on 0xFF and on 0x00 garbage.  -> (the launched kernel's name, the result on the host)."""
    x_guard = _in_guard(x.dtype) if x_guard is None else x_guard
    xbuf, xv = G.guarded(x, x.dtype, DEV, x_off, sentinel=x_guard)
    before = xbuf.cpu()
    ybuf, yv = G.guarded(y_shape, y_dtype, DEV, y_off)
    results = []
    for garbage in ((0xFF, 0x00) if ws_bytes else (None,)):
        tag = what if garbage is None else f"{what} workspace={garbage:#04x}"
        if results:
            yv.fill_(G.sentinel_for(y_dtype))
        wbuf, ws = G.guarded_workspace(ws_bytes, DEV, garbage)
        _lib.check(call(xv.data_ptr(), yv.data_ptr(), None if ws is None else ws.data_ptr(), ws_bytes))
        torch.cuda.synchronize()
        kernel = _lib.last_kernel()
        tag = f"{tag} [{kernel}]"
        G.assert_guards_intact(ybuf, yv, what=tag + ": output")
        G.assert_same(yv, want, tag)
        G.assert_unchanged(xbuf, before, tag + ": input")
        if wbuf is not None:
            G.assert_guards_intact(wbuf, ws, what=tag + ": workspace")
        results.append(yv.cpu())
    if len(results) == 2:
        G.assert_unchanged(results[1], results[0], what + ": the result depends on the workspace's content")
    return kernel, results[0]


# ---- mv_pointwise_* ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_pointwise(dtype):
    lib = _lib.load()
    fn = lib.mv_pointwise_u8 if dtype == U8 else lib.mv_pointwise_f32
    v = 16 // dtype.itemsize
    seen = set()
    for n in (1, v - 1, v, v + 1, 256 * v - 1, 256 * v, 256 * v + 1, 2 * 256 * v + v + 3):
        g = torch.Generator().manual_seed(n)
        x = torch.randint(0, 256, (n,), generator=g, dtype=U8) if dtype == U8 else torch.rand((n,), generator=g)
        thr = x[n // 2].item()  # a threshold equal to a pixel value
        ops = [("invert", 0, 0.0, {})] + [("posterize", 1, float(b), dict(bits=b)) for b in (0, 3, 8)]
        ops += [("solarize", 2, float(thr), dict(threshold=thr))]
        for name, code, param, kw in ops:
            want = AA_REF[name](x, **kw)
            for xo, yo in _alignments(dtype.itemsize):
                what = f"pointwise {name} {kw} n={n} x_offset={xo} y_offset={yo}"
                kernel, _ = _run(what, lambda xp, yp, ws, nb: fn(xp, yp, n, code, param, _stream()), x, xo, (n,), dtype, yo,
                                 want)
                assert ("vec16" if _aligned(xo, yo) else "px") in kernel and f"op{code}" in kernel, (what, kernel)
                seen.add(kernel.split(",")[-1])
    assert seen == {"vec16>", "px>"}, seen


# ---- mv_color_chain_*, mv_rgb_to_grayscale_* ----------------------------------------------------------------------------------------
COLOR_CODES = {"brightness": 0, "contrast": 1, "saturation": 2, "hue": 3}
COLOR_CHAINS = [[("brightness", 1.7)], [("contrast", 1.3)], [("saturation", 0.6)], [("hue", -0.27)],
                [("contrast", 0.5), ("brightness", 1.2), ("saturation", 1.5), ("hue", 0.1)],
                [("hue", 0.1), ("brightness", 1.2), ("saturation", 1.5), ("contrast", 0.5)]]


def _color_sizes(v):
    return (1, v - 1, v, v + 1, 256 * v, 256 * v + v, 8 * 256 * v - v, 8 * 256 * v, 8 * 256 * v + 1)


@pytest.mark.parametrize("channels", [1, 3], ids=["c1", "c3"])
@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_color_chain(dtype, channels):
    lib = _lib.load()
    fn = lib.mv_color_chain_u8 if dtype == U8 else lib.mv_color_chain_f32
    v = 16 // dtype.itemsize
    form = _blend_form()
    images = 2
    seen = set()
    for hw in _color_sizes(v):
        h, w = _factor(hw)
        x = _pixels((images, channels, h, w), dtype, seed=hw + channels)
        for ops in COLOR_CHAINS:
            want = emu_chain(x, ops, form)
            contrast = any(name == "contrast" for name, _ in ops)
            if len(ops) == 1 and not contrast:  # the library's formula is the reference's bits
                assert torch.equal(want, COLOR_REF[ops[0][0]](x, ops[0][1])), (ops, hw)
            elif dtype == U8:  # the exact integer mean is ATen's at these sizes
                assert torch.equal(want, ref_chain(x, ops)), (ops, hw)
            codes = (C.c_int * len(ops))(*[COLOR_CODES[name] for name, _ in ops])
            factors = (C.c_double * len(ops))(*[f for _, f in ops])
            ws_bytes = int(lib.mv_color_workspace_bytes(images, h, w, int(dtype == U8))) if contrast else 0
            for xo, yo in _alignments(dtype.itemsize):
                what = f"color_chain {ops} c={channels} ({h}, {w}) x_offset={xo} y_offset={yo}"
                kernel, got = _run(what, lambda xp, yp, ws, nb: fn(xp, yp, images, channels, h, w, codes, factors, len(ops), form,
                                                                   ws, nb, _stream()), x, xo, x.shape, dtype, yo, want,
                                   ws_bytes=ws_bytes)
                vec = _aligned(xo, yo) and hw % v == 0
                assert ("vec16" if vec else "px") in kernel and (",mean" in kernel) == contrast, (what, kernel)
                seen.add("vec16" if vec else "px")
                if contrast and len(ops) == 1 and _aligned(xo, yo) and form == 1:
                    check_contrast_reference(x, ops[0][1], got)
    assert seen == {"vec16", "px"}, seen


@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_rgb_to_grayscale(dtype):
    lib = _lib.load()
    fn = lib.mv_rgb_to_grayscale_u8 if dtype == U8 else lib.mv_rgb_to_grayscale_f32
    v = 16 // dtype.itemsize
    form = _blend_form()
    images = 2
    seen = set()
    for hw in _color_sizes(v):
        h, w = _factor(hw)
        x = _pixels((images, 3, h, w), dtype, seed=hw)
        for out_c in (1, 3):
            want = emu_grayscale(x, out_c, form)
            if form == 1:
                assert torch.equal(want, ref_rgb_to_grayscale(x, out_c))
            for xo, yo in _alignments(dtype.itemsize):
                what = f"rgb_to_grayscale out_channels={out_c} ({h}, {w}) x_offset={xo} y_offset={yo}"
                kernel, _ = _run(what, lambda xp, yp, ws, nb: fn(xp, yp, images, h, w, out_c, form, _stream()), x, xo,
                                 (images, out_c, h, w), dtype, yo, want)
                vec = _aligned(xo, yo) and hw % v == 0
                assert ("vec16" if vec else "px") in kernel, (what, kernel)
                seen.add("vec16" if vec else "px")
    assert seen == {"vec16", "px"}, seen


# ---- mv_autocontrast_*, mv_equalize_* ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
@pytest.mark.parametrize("name", ["autocontrast", "equalize"])
def test_plane_ops(name, dtype):
    lib = _lib.load()
    u8 = dtype == U8
    fn = getattr(lib, f"mv_{name}_{'u8' if u8 else 'f32'}")
    ws_fn = getattr(lib, f"mv_{name}_workspace_bytes")
    v = 16 // dtype.itemsize
    m, r = 4 * 256 * v, 8 * 256 * v  # the map chunk (kMapItems) and the reduce chunk (kItems)
    planes = 3
    hi = 255 if u8 else 1.0
    seen = set()
    for hw in (1, v - 1, v, v + 1, m - v, m, m + 1, r, r + v, 2 * r + 5):
        h, w = _factor(hw)
        x = _pixels((planes, h, w), dtype, seed=hw)
        x[1] = 77 if u8 else 0.3  # a flat plane
        if name == "equalize":  # fewer than 255 pixels below the plane's maximum: step == 0
            x[2] = hi
            x[2].view(-1)[:200] = torch.tensor(hi / 5, dtype=dtype)
        inputs = [("", x)]
        if not u8:  # one NaN in the last element of a plane: the scalar tail
            xn = x.clone()
            xn[0].view(-1)[-1] = NAN
            inputs.append((" NaN at the end of plane 0", xn))
        ws_bytes = int(ws_fn(planes, h, w, int(u8)))
        assert ws_bytes > 0
        for label, xi in inputs:
            want = AA_REF[name](xi)
            for xo, yo in _alignments(dtype.itemsize):
                what = f"{name}{label} ({h}, {w}) x_offset={xo} y_offset={yo}"
                kernel, _ = _run(what, lambda xp, yp, ws, nb: fn(xp, yp, planes, h, w, ws, nb, _stream()), xi, xo, xi.shape,
                                 dtype, yo, want, ws_bytes=ws_bytes)
                vec = _aligned(xo, yo) and hw % v == 0
                assert kernel.startswith(f"k_{name}<") and ("vec16" if vec else "px") in kernel, (what, kernel)
                seen.add("vec16" if vec else "px")
    assert seen == {"vec16", "px"}, seen


# ---- mv_pad_crop_flip, mv_erase -------------------------------------------------------------------------------------------------------
MOVER_DTYPES = {1: torch.uint8, 2: torch.int16, 4: torch.float32, 8: torch.float64}  # reflect / edge pad through float32 in
PAD_MODES = {"constant": 0, "edge": 1, "reflect": 2, "symmetric": 3}                 # the reference: exact for these


def _gather_ref(x, oh, ow, top, left, mode, flip_h, flip_v, fill):
    """Output (oy, ox) = source (map(oy), map(ox)) with p = (flip ? out - 1 - o : o) + offset: pad what the window lacks,
    take the window, then mirror the output."""
    ih, iw = x.shape[-2:]
    pl, pr, pt, pb = max(-left, 0), max(left + ow - iw, 0), max(-top, 0), max(top + oh - ih, 0)
    out = CR.pad_image(x, [pl, pt, pr, pb], fill=fill, padding_mode=mode)
    out = out[..., top + pt:top + pt + oh, left + pl:left + pl + ow]
    dims = [d for d, f in ((-1, flip_h), (-2, flip_v)) if f]
    return (out.flip(dims) if dims else out).contiguous()


def _paddings(out, mode, wanted):
    """(before, after, in) along one axis of `out` output elements: the first of `wanted` the mode allows."""
    for before, after in wanted + [(0, 0)]:
        n = out - before - after
        if n < 1 or (mode == "reflect" and max(before, after) >= n) or (mode == "symmetric" and max(before, after) > n):
            continue
        return before, after, n
    raise AssertionError((out, mode))


def _gather_cases(ih, ow, dtype):
    """(label, x shape (2, 3, ., .), oh, ow, top, left, mode, flip_h, flip_v, fill)"""
    cases = [("copy", (ih, ow), ih, ow, 0, 0, "constant", 0, 0, None),
             ("crop", (ih + 2, ow + 5), ih, ow, 1, 2, "constant", 0, 0, None),
             ("hflip", (ih, ow), ih, ow, 0, 0, "constant", 1, 0, None),
             ("vflip", (ih, ow), ih, ow, 0, 0, "constant", 0, 1, None),
             ("hflip + vflip", (ih, ow), ih, ow, 0, 0, "constant", 1, 1, None)]
    for mode in PAD_MODES:  # unequal paddings of 1 .. 3 per side where the side allows them
        pl, pr, iw = _paddings(ow, mode, [(1, 3), (1, 2), (0, 1)])
        pt, pb = next((t, b) for t, b in [(2, 1), (1, 0), (0, 0)]
                      if not (mode == "reflect" and max(t, b) >= ih) and not (mode == "symmetric" and max(t, b) > ih))
        cases.append((f"pad {mode} l{pl} r{pr} t{pt} b{pb}", (ih, iw), ih + pt + pb, ow, -pt, -pl, mode, 0, 0,
                      7 if mode == "constant" else None))
    fill = [1.5, -2.25, 3.0] if dtype.is_floating_point else [1, 2, 3]
    cases.append(("pad + crop + hflip, per-channel fill", (ih, ow + 1), ih, ow, 1, -2, "constant", 1, 0, fill))
    return cases


@pytest.mark.parametrize("elem_bytes", [1, 2, 4, 8])
def test_pad_crop_flip(elem_bytes):
    lib = _lib.load()
    dtype = MOVER_DTYPES[elem_bytes]
    v = 16 // elem_bytes
    planes, channels = 6, 3
    for ih in (1, 3):
        for ow in (1, v - 1, v, v + 1, 2 * v - 1, 4 * v, 4 * v + 1, 256 * v + 3):
            for label, in_hw, oh, _, top, left, mode, fh, fv, fill in _gather_cases(ih, ow, dtype):
                x = _elements((2, 3) + in_hw, dtype, seed=ih * 1000 + ow)
                want = _gather_ref(x, oh, ow, top, left, mode, fh, fv, fill)
                fill_host = None
                if fill is not None:  # a HOST array of `channels` elements in the image's dtype
                    fill_host = torch.tensor(fill if isinstance(fill, list) else [fill] * channels, dtype=dtype)
                fill_ptr = None if fill_host is None else fill_host.data_ptr()
                for xo, yo in _alignments(elem_bytes):
                    what = f"pad_crop_flip b{elem_bytes} {label} {in_hw} -> ({oh}, {ow}) top={top} left={left} x_offset={xo} y_offset={yo}"
                    kernel, _ = _run(what, lambda xp, yp, ws, nb: lib.mv_pad_crop_flip(
                        xp, yp, planes, channels, elem_bytes, in_hw[0], in_hw[1], oh, ow, top, left, PAD_MODES[mode], fh, fv, fill_ptr,
                        _stream()), x, xo, want.shape, dtype, yo, want)
                    assert kernel.startswith(f"k_gather<b{elem_bytes},"), (what, kernel)


@pytest.mark.parametrize("elem_bytes", [1, 2, 4, 8])
def test_erase(elem_bytes):
    lib = _lib.load()
    dtype = MOVER_DTYPES[elem_bytes]
    v = 16 // elem_bytes
    planes, channels = 6, 3
    for h in (1, 3):
        i, eh = (0, 1) if h == 1 else (1, 2)
        for w in (1, v - 1, v, v + 1, 2 * v - 1, 4 * v, 4 * v + 1, 256 * v + 3):
            x = _elements((2, 3, h, w), dtype, seed=h * 1000 + w + 1)
            boxes = {(0, min(2, w)), (w - 1, 1)}  # at column 0, at the last column
            if w >= v + 1:
                boxes.add((v - 1, 2))  # straddling a group boundary
            for j, ew in sorted(boxes):
                for per_pixel in (0, 1):
                    value = _elements((3, eh, ew) if per_pixel else (3, 1, 1), dtype, seed=j + ew + per_pixel)
                    vd = value.to(DEV)
                    want = CR.erase_image(x, i, j, eh, ew, value)
                    for xo, yo in _alignments(elem_bytes):
                        what = (f"erase b{elem_bytes} ({h}, {w}) box=({i}, {j}, {eh}, {ew}) v_is_per_pixel={per_pixel} x_offset={xo} "
                                f"y_offset={yo}")
                        kernel, _ = _run(what, lambda xp, yp, ws, nb: lib.mv_erase(
                            xp, yp, planes, channels, elem_bytes, h, w, i, j, eh, ew, vd.data_ptr(), per_pixel, _stream()),
                            x, xo, x.shape, dtype, yo, want)
                        assert kernel.startswith(f"k_gather<b{elem_bytes},") and "box" in kernel, (what, kernel)
                    # in place: only the box changes -- the rest of the image and both guards keep their bits
                    for xo in sorted({xo for xo, _ in _alignments(elem_bytes)}):
                        what = f"erase in place b{elem_bytes} ({h}, {w}) box=({i}, {j}, {eh}, {ew}) v_is_per_pixel={per_pixel} offset={xo}"
                        buf, view = G.guarded(x, dtype, DEV, xo, sentinel=_in_guard(dtype))
                        expect = buf.cpu()
                        start = view.storage_offset()
                        expect[start:start + x.numel()] = want.reshape(-1)
                        _lib.check(lib.mv_erase(view.data_ptr(), view.data_ptr(), planes, channels, elem_bytes, h, w, i, j, eh, ew,
                                                vd.data_ptr(), per_pixel, _stream()))
                        torch.cuda.synchronize()
                        assert _lib.last_kernel() == f"k_erase_box<b{elem_bytes}>", what
                        G.assert_guards_intact(buf, view, _in_guard(dtype), what)
                        G.assert_unchanged(buf, expect, what)


# ---- mv_mixup_*, mv_cutmix, mv_mixup_labels_i64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.float64], ids=["f32", "f16", "f64"])
def test_mixup(dtype):
    lib = _lib.load()
    name = {torch.float32: "f32", torch.float16: "f16", torch.float64: "f64"}[dtype]
    fn = getattr(lib, f"mv_mixup_{name}")
    v = 16 // dtype.itemsize
    seen = set()
    for elems in (1, v - 1, v, v + 1, 63 * v, 63 * v + 1, 256 * v + 1):  # 63 groups: the last flat size; 64: the first walk
        for batch in (1, 2, 5, 17, 20, 33):
            x = _elements((batch, elems), dtype, seed=batch * 10000 + elems)
            for lam in (0.0, 1.0, LAM):
                want = MR.mixup_image(x, lam)
                for xo, yo in _alignments(dtype.itemsize):
                    what = f"mixup {name} batch={batch} sample_elems={elems} lam={lam} x_offset={xo} y_offset={yo}"
                    kernel, _ = _run(what, lambda xp, yp, ws, nb: fn(xp, yp, batch, elems, lam, _stream()), x, xo, x.shape,
                                     dtype, yo, want)
                    walk = batch > 1 and (elems + v - 1) // v >= 64
                    assert kernel.startswith(f"k_mixup_roll<{name}," if walk else f"k_mixup_flat<{name}>"), (what, kernel)
                    seen.add(kernel.split("<")[0])
    assert seen == {"k_mixup_flat", "k_mixup_roll"}, seen


CUTMIX_DTYPES = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@pytest.mark.parametrize("elem_bytes", [1, 2, 4, 8])
def test_cutmix(elem_bytes):
    lib = _lib.load()
    dtype = CUTMIX_DTYPES[elem_bytes]
    v = 16 // elem_bytes
    for pps in (1, 3):
        for h in (3, 5):
            for batch in (1, 3):
                for w in sorted({1, v - 1, v + 1, 2 * v + 3}):  # w < V: groups span rows and wrap into the next plane
                    x = _elements((batch, pps, h, w), dtype, seed=pps * 1000 + h * 100 + batch * 10 + w)
                    inner = (1, 1, w - 1, h - 1) if w >= 3 else (0, 1, w, h - 1)  # both edges inside a group
                    boxes = [(0, 0, 0, 0), (0, 0, w, h), (w - 1, h - 1, w, h), inner, (0, h - 1, w, h)]
                    for box in boxes:
                        want = MR.cutmix_image(x, box)
                        for xo, yo in _alignments(elem_bytes):
                            what = f"cutmix b{elem_bytes} {tuple(x.shape)} box(x1, y1, x2, y2)={box} x_offset={xo} y_offset={yo}"
                            kernel, _ = _run(what, lambda xp, yp, ws, nb: lib.mv_cutmix(xp, yp, batch, pps, elem_bytes, h, w, *box,
                                                                                        _stream()), x, xo, x.shape, dtype,
                                             yo, want)
                            assert kernel == f"k_cutmix<b{elem_bytes}>", (what, kernel)


def test_mixup_labels():
    lib = _lib.load()
    seen = set()
    for batch, classes in ((1, 1), (1, 2), (3, 3), (7, 10), (3, 1000), (7, 1000)):
        g = torch.Generator().manual_seed(batch * classes)
        plain = torch.randint(0, classes, (batch,), generator=g)
        outside = plain.clone()  # labels outside [0, classes) match no column: rows without an own share, nothing scattered
        outside[0] = -1
        outside[-1] = classes
        for label, labels in (("", plain), (" with -1 and num_classes", outside)):
            one_hot = (labels[:, None] == torch.arange(classes)[None, :]).float()
            if not label:
                assert torch.equal(one_hot, torch.nn.functional.one_hot(labels, classes).float())
            for lam in (0.0, 1.0, LAM):
                want = MR.mixup_label(one_hot, lam)
                for xo, yo in ((A, A), (A, 1), (1, A), (1, 1)):
                    what = f"mixup_labels{label} batch={batch} classes={classes} lam={lam} x_offset={xo} y_offset={yo}"
                    # label 0 is a class: a stray read of the guard would put a share into column 0
                    kernel, _ = _run(what, lambda xp, yp, ws, nb: lib.mv_mixup_labels_i64(xp, yp, batch, classes, lam,
                                                                                         _stream()),
                                     labels, xo, (batch, classes), torch.float32, yo, want, x_guard=0)
                    assert kernel == ("k_mixup_labels<vec>" if yo == A else "k_mixup_labels<scalar>"), (what, kernel)
                    seen.add(kernel)
    assert seen == {"k_mixup_labels<vec>", "k_mixup_labels<scalar>"}, seen


# ---- mv_resized_crop_*: the source window of resize.hip -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_resized_crop(dtype):
    lib = _lib.load()
    fn = lib.mv_resized_crop_u8 if dtype == U8 else lib.mv_resized_crop_f32
    planes, h, w = 3, 19, 23
    x = _pixels((planes, h, w), dtype, seed=19)
    seen = set()
    # (top, left, height, width): the whole image, interior, reaching outside on the top-left and on the bottom-right
    for box in ((0, 0, h, w), (3, 4, 11, 13), (-3, -4, 15, 17), (8, 10, 15, 17)):
        cropped = CR.crop_image(x, *box)
        for oh, ow in ((1, 1), (7, 9), (16, 17), (5, 64)):
            plain = torch.from_numpy(oracle.resize(cropped.numpy(), [oh, ow]))
            ws_bytes = int(lib.mv_resize_workspace_bytes(planes, box[2], box[3], oh, ow, 0, 0, oh, ow))
            for flip in (0, 1):
                want = plain.flip((-1, -2)).contiguous() if flip else plain
                for xo, yo in _alignments(dtype.itemsize):
                    what = f"resized_crop box={box} -> ({oh}, {ow}) flips={flip} x_offset={xo} y_offset={yo}"
                    kernel, got = _run(what, lambda xp, yp, ws, nb: fn(xp, yp, planes, h, w, *box, oh, ow, flip, flip, ws, nb,
                                                                       _stream()), x, xo, want.shape, dtype, yo, want,
                                       ws_bytes=ws_bytes)
                    assert (kernel == "k_resize_h") == (ws_bytes > 0), (what, kernel, ws_bytes)
                    seen.add(kernel.split("<")[0])
                    if _aligned(xo, yo):  # as test_resized_crop_against_interpolate_and_the_oracle: interpolate, then the oracle
                        interp = CR.resize_image(cropped, (oh, ow))
                        assert_matches_reference(got, interp.flip((-1, -2)).contiguous() if flip else interp, what)
    assert seen == {"k_resize_h", "k_resize_fused"}, seen
