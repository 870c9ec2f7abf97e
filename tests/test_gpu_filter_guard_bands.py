"""Guard-band sweeps of the filter kernels at the C ABI (`-m gpu`): blur, depthwise, separable, Sobel and sharpness -- k_dwtile,
k_dw3x3, k_dw3x3_u8, k_dwk_u8, k_sepfast, k_sepstream, k_separable, k_u8_tie_fixup, k_dwf64 and k_sharp_f64 -- in the style of
tests/test_gpu_guard_bands.py.  The value tests of this family (test_gpu_parity.py, test_gpu_fuzz.py, test_gpu_frames.py) hand
every kernel a fresh, 256-byte aligned torch.empty; here every input, output, frame, workspace and device tap array lies inside a
sentinel-filled buffer (tests/_guard.py) at 16-byte aligned and at odd element offsets, at the widths and heights where the
kernels change their lane layout (16 pixels per lane with a 4-byte halo, 4-pixel vector stores chosen by a pointer test made once
per launch, lane groups walking (plane, strip) units on narrow images, tiles narrowing to 128 / 64 / 32 pixels, the frame-pointer
table of the *_v entry points, the tie list of mv_gaussian_blur_u8_ws).  Every case asserts that

  1. the result equals the oracle of that entry point (oracle/ref.py), bit for bit (G.assert_same: no tolerance);
  2. nothing outside any output changed (outputs are pre-filled with the sentinel, so equality also proves they were written
     whole); Sobel's two outputs and every frame of a *_v call have a guarded buffer each, so a frame's guards also prove that no
     other frame's launch wrote into it;
  3. every input buffer -- whose guards hold NaN for floats, so that a guard value that reaches an output shows even through a
     zero-padded tap (0 * NaN = NaN), or alternating 0 / 255 around pixels drawn from [40, 200] for uint8 -- is unchanged, guards
     included.  A value that is loaded and then discarded (a lane that loads a clamped address and never uses it) cannot be seen
     this way, and nothing here tries to;
  4. the workspace of mv_gaussian_blur_u8_ws, sized with exactly mv_gaussian_blur_u8_workspace_bytes, keeps its guards, and runs
     on 0xFF and on 0x00 garbage give the same bits; tap arrays passed as device pointers are guarded and unchanged too.

Combinations an entry point refuses by contract are called as well and must return the documented status.  Each test collects
mv_last_kernel() over its sweep and asserts which kernel families ran at aligned and at odd offsets: a sweep that silently stopped
reaching a kernel fails.  k_sepfast is the one family that cannot run at an odd offset (sepfast_supported requires 16-byte
pointers); for it the tests assert that an odd offset takes the fallback."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib, functional as F  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests.test_gpu_guard_bands import _aligned, _alignments, _in_guard, _pixels, _stream  # noqa: E402

DEV = "cuda"
A = G.ALIGNED
NAN = float("nan")
U8, F32, F16, BF16, F64 = torch.uint8, torch.float32, torch.float16, torch.bfloat16, torch.float64
VALID, REFLECT, ZERO = ref.BORDER_VALID, ref.BORDER_REFLECT, ref.BORDER_ZERO
BORDERS = {"valid": VALID, "reflect": REFLECT, "zero": ZERO}
INVALID, UNSUPPORTED = -1, -2  # MV_ERR_INVALID_ARGUMENT, MV_ERR_UNSUPPORTED
HEIGHTS = (1, 2, 3, 7, 8, 9, 17, 33)
PLANES = 3


def _offsets(elem_bytes, full):
    """(x_offset, y_offset) pairs.  full (the alignment decides the instantiation): _alignments, plus for 2-byte types an
    offset that is 4-byte but not 8-byte aligned (for 8-byte types every odd offset is 8-byte but not 16-byte aligned).
    Otherwise aligned, x odd, y odd and both odd."""
    cases = _alignments(elem_bytes)
    if not full:
        return cases[:4]
    if elem_bytes == 2:
        cases = cases + [(2, A), (A, 2), (2, 2)]
    return cases


def _heights(i, allowed=HEIGHTS, n=2):
    """n heights of `allowed`, rotating with the case index so that a sweep over widths meets all of them."""
    return sorted({allowed[(i + j * 3) % len(allowed)] for j in range(n)})


def _k1d(k, sigma, dtype=F32):
    return F._get_gaussian_kernel1d(k, sigma, dtype).numpy()


def _taps(a):
    return _lib.taps_from_tensor(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


class _Seen:
    """Kernel labels of one sweep, by whether every pointer of the case was 16-byte aligned."""

    def __init__(self):
        self.labels = {True: set(), False: set()}
        self.cases = 0

    def note(self, kernel, aligned):
        self.labels[bool(aligned)].add(kernel)
        self.cases += 1

    def require(self, *parts, aligned=(True, False)):
        """A label containing every one of `parts` ran at each of the `aligned` kinds of offset."""
        for al in aligned:
            assert any(all(p in k for p in parts) for k in self.labels[al]), (
                f"no kernel matching {parts} ran at {'aligned' if al else 'odd'} offsets", sorted(self.labels[al]))

    def never(self, part, aligned):
        assert not any(part in k for k in self.labels[aligned]), (part, aligned, sorted(self.labels[aligned]))

    def report(self, name):
        print(f"{name}: {self.cases} cases; aligned: {sorted(self.labels[True])}; odd: {sorted(self.labels[False])}")


def _run(what, call, xs, x_offs, y_specs, wants, ws_bytes=0, fixed=()):
    """One case: call(x views, y views, ws_ptr, ws_bytes) -> status on guarded buffers, then the four assertions.
    xs: host inputs, each placed at its offset of x_offs; y_specs: (shape, dtype, offset) per output; wants: the expected
    outputs; fixed: (buf, host copy, name) of further device buffers (tap arrays) that must stay as they are.  With a workspace
    the call runs twice, on 0xFF and on 0x00 garbage.  -> the last launched kernel's label."""
    xb = [G.guarded(x, x.dtype, DEV, o, sentinel=_in_guard(x.dtype)) for x, o in zip(xs, x_offs)]
    before = [buf.cpu() for buf, _ in xb]
    yb = [G.guarded(shape, dtype, DEV, o) for shape, dtype, o in y_specs]
    results = []
    for garbage in ((0xFF, 0x00) if ws_bytes else (None,)):
        tag = what if garbage is None else f"{what} workspace={garbage:#04x}"
        if results:
            for _, yv in yb:
                yv.fill_(G.sentinel_for(yv.dtype))
        wbuf, ws = G.guarded_workspace(ws_bytes, DEV, garbage)
        _lib.check(call([v for _, v in xb], [v for _, v in yb], None if ws is None else ws.data_ptr(), ws_bytes))
        torch.cuda.synchronize()
        kernel = _lib.last_kernel()
        tag = f"{tag} [{kernel}]"
        for i, ((ybuf, yv), want) in enumerate(zip(yb, wants)):
            G.assert_guards_intact(ybuf, yv, what=f"{tag}: output {i}")
            G.assert_same(yv, want, f"{tag}: output {i}")
        for i, ((xbuf, _), was) in enumerate(zip(xb, before)):
            G.assert_unchanged(xbuf, was, f"{tag}: input {i}")
        for buf, was, name in fixed:
            G.assert_unchanged(buf, was, f"{tag}: {name}")
        if wbuf is not None:
            G.assert_guards_intact(wbuf, ws, what=tag + ": workspace")
        results.append([yv.cpu() for _, yv in yb])
    if len(results) == 2:
        for r1, r0 in zip(results[1], results[0]):
            G.assert_unchanged(r1, r0, what + ": the result depends on the workspace's content")
    return kernel


def _refused(what, fn, x, y_shape, args, status):
    """An entry point refuses the combination by contract: the documented status, and nothing written."""
    xbuf, xv = G.guarded(x, x.dtype, DEV, A, sentinel=_in_guard(x.dtype))
    ybuf, yv = G.guarded(y_shape, x.dtype, DEV, A)
    ybefore = ybuf.cpu()
    rc = fn(xv.data_ptr(), yv.data_ptr(), *args)
    torch.cuda.synchronize()
    assert rc == status, (what, rc, _lib.load().mv_last_error())
    G.assert_unchanged(ybuf, ybefore, what + ": output of a refused call")


def _refused_call(what, call, xs, x_offs, y_specs, status, ws_bytes=0, ws_offset=0):
    """As _refused for any argument list: call(x views, y views, ws_ptr, ws_bytes) -> status with every input, output and (if
    any) a workspace of ws_bytes bytes, ws_offset bytes past a 256-byte boundary, in guarded buffers; the documented status, and
    no output or workspace byte written."""
    xb = [G.guarded(x, x.dtype, DEV, o, sentinel=_in_guard(x.dtype)) for x, o in zip(xs, x_offs)]
    yb = [G.guarded(shape, dtype, DEV, o) for shape, dtype, o in y_specs]
    ybefore = [buf.cpu() for buf, _ in yb]
    wbuf = ws = wbefore = None
    if ws_bytes:
        wbuf, ws = G.guarded((ws_bytes,), U8, DEV, ws_offset)
        assert ws.data_ptr() % 256 == ws_offset % 256
        wbefore = wbuf.cpu()
    rc = call([v for _, v in xb], [v for _, v in yb], None if ws is None else ws.data_ptr(), ws_bytes)
    torch.cuda.synchronize()
    assert rc == status, (what, rc, _lib.load().mv_last_error())
    for i, ((ybuf, _), was) in enumerate(zip(yb, ybefore)):
        G.assert_unchanged(ybuf, was, f"{what}: output {i} of a refused call")
    if wbuf is not None:
        G.assert_unchanged(wbuf, wbefore, what + ": workspace of a refused call")


def _device_taps(w, dtype, offset):
    """A tap array on the device inside NaN guards -> (buf, view, host copy of buf)."""
    buf, view = G.guarded(_t(w, dtype), dtype, DEV, offset, sentinel=NAN)
    return buf, view, buf.cpu()


# ---- what alignment decides (csrc/dwtile.hip launch_dwtile) ---------------------------------------------------------------------
def _dwtile_head(dtype):
    return "k_dwtile<" + {U8: "u8", F32: "f32"}.get(dtype, "f16/bf16") + ","


def _expect_2d(kernel, what, dtype, w, x_ptr_ok, y_ptr_ok):
    """A 2-D entry point ran one of its families; which one, size by size, is the launchers' business and is asserted per sweep
    (_Seen.require).  Per case only what the pointers decide: k_dwtile stores 4 pixels per access exactly when W % 4 == 0 and
    both pointers have the alignment of 4 pixels (16 bytes for float32, 4 for uint8, 8 for the half types)."""
    if kernel.startswith("k_dwtile<"):
        assert kernel.startswith(_dwtile_head(dtype)), (what, kernel)
        assert (",vec16," in kernel) == (w % 4 == 0 and x_ptr_ok and y_ptr_ok), (what, kernel)
    elif dtype == U8:
        assert kernel in ("k_dw3x3", "k_dw3x3_u8") or (kernel.startswith("k_dwk_u8<") and kernel.endswith(",2d>")), (what, kernel)
    else:
        assert dtype == F32 and kernel == "k_dw3x3", (what, kernel)


def _ptr_ok(offset, dtype):
    return (offset * dtype.itemsize) % {1: 4, 2: 8, 4: 16}[dtype.itemsize] == 0


# ---- mv_depthwise_conv2d_f32 / _u8 ---------------------------------------------------------------------------------------------
def _depthwise_taps(ky, kx, kind, seed):
    """float32 (ky, kx) taps.  'signed': any sign; 'avg': non-negative, sum < 1 (the uint8 16-pixel kernels); 'one negative':
    a heavy centre and one tap of -0.01, so that uint8 results stay inside [0, 255] on pixels from [40, 200] with any border."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand((ky, kx), generator=g)
    if kind == "signed":
        return (w - 0.5).numpy()
    w = w + 0.05
    if kind == "one negative":
        w[ky // 2, kx // 2] += 1.0 + 0.05 * ky * kx
    w = (w / w.sum() * 0.999).to(torch.float32)
    if kind == "one negative":
        w[0, 0] = -0.01
    return w.numpy()


DW_SIZES = [(3, 3), (5, 5), (3, 5), (7, 7), (1, 5), (9, 1), (11, 11), (13, 13)]  # (ky, kx); 13 x 13 through device taps
DW_WIDTHS = {(3, 3): (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 20, 33, 36, 64, 65, 127, 128, 129, 255, 256, 257, 260, 1025),
             (5, 5): (3, 4, 5, 8, 16, 19, 20, 32, 33, 64, 65, 128, 129, 256, 257, 260, 1040)}
DW_WIDTHS_OTHER = (7, 8, 20, 64, 129, 260)


def _depthwise_sweep(dtype, border_name, kinds):
    lib = _lib.load()
    u8 = dtype == U8
    fn = lib.mv_depthwise_conv2d_u8 if u8 else lib.mv_depthwise_conv2d_f32
    border = BORDERS[border_name]
    seen = _Seen()
    refused = 0
    for kind in kinds:
        for ky, kx in DW_SIZES:
            if kind == "one negative" and (ky, kx) not in ((3, 3), (5, 5), (1, 5)):
                continue
            on_device = int(ky * kx > _lib.MAX_HOST_TAPS_2D)
            w2 = _depthwise_taps(ky, kx, kind, seed=ky * 31 + kx)
            widths = DW_WIDTHS.get((ky, kx), DW_WIDTHS_OTHER)
            for i, w in enumerate(widths[::2] if kind == "one negative" else widths):
                for h in _heights(i + ky):
                    x = _pixels((PLANES, h, w), dtype, seed=1000 * h + w)
                    args = lambda wp: (wp, on_device, PLANES, h, w, ky, kx, border)  # noqa: E731
                    what = f"depthwise {dtype} {border_name} {kind} {ky}x{kx} ({h}, {w})"
                    too_big = (border == REFLECT and (ky // 2 >= h or kx // 2 >= w)) or (border == VALID and (ky > h or kx > w))
                    host = _taps(w2)  # kept alive over the calls below
                    if too_big:  # refused by contract
                        tb, tv, _ = _device_taps(w2, F32, A)
                        _refused(what, fn, x, (PLANES, h, w), args(tv.data_ptr() if on_device else host) + (_stream(),), INVALID)
                        refused += 1
                        continue
                    xf = x.numpy().astype(np.float32)
                    got = ref.depthwise_conv2d(xf, w2, border)
                    want = _t(np.rint(got).astype(np.uint8)) if u8 else _t(got)
                    # the uint8 16-pixel kernels take any alignment: there the pointer decides nothing
                    x16 = u8 and kind == "avg" and not on_device and border != VALID and w >= 16 and max(ky, kx) <= 7
                    for xo, yo in _offsets(dtype.itemsize, w % 4 == 0 and not x16):
                        tag = f"{what} x_offset={xo} y_offset={yo}"
                        fixed = ()
                        if on_device:
                            tb, tv, twas = _device_taps(w2, F32, 1 if xo != A else A)
                            wp, fixed = tv.data_ptr(), ((tb, twas, "device taps"),)
                        else:
                            wp = C.cast(host, C.c_void_p)
                        kernel = _run(tag, lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), *args(wp), _stream()),
                                      [x], [xo], [(want.shape, dtype, yo)], [want], fixed=fixed)
                        _expect_2d(kernel, tag, dtype, w, _ptr_ok(xo, dtype), _ptr_ok(yo, dtype))
                        seen.note(kernel, _aligned(xo, yo))
    seen.report(f"mv_depthwise_conv2d {dtype} {border_name}")
    assert refused or border == ZERO
    return seen


@pytest.mark.parametrize("border", ["reflect", "zero", "valid"])
def test_depthwise_f32(border):
    seen = _depthwise_sweep(F32, border, ["signed"])
    seen.require("k_dwtile<f32", "tw256>")
    seen.require("k_dwtile<f32", "tw128>")
    seen.require("k_dwtile<f32", "tw64>")
    seen.require("k_dwtile<f32", "tw32>")
    seen.require("k_dwtile<f32,0x0,")
    seen.require("k_dwtile<f32", "scalar")
    seen.require("k_dwtile<f32", "vec16", aligned=(True,))
    seen.never("vec16", False)
    if border != "valid":
        seen.require("k_dw3x3")


@pytest.mark.parametrize("border", ["reflect", "zero", "valid"])
def test_depthwise_u8(border):
    seen = _depthwise_sweep(U8, border, ["avg", "one negative"])
    seen.require("k_dwtile<u8", "tw256>")
    seen.require("k_dwtile<u8,0x0,")
    if border != "valid":
        seen.require("k_dw3x3_u8")
        seen.require("k_dwk_u8<5x5,2d>")
        seen.require("k_dwk_u8<3x5,2d>")
        seen.require("k_dwk_u8<7x7,2d>")
        assert "k_dw3x3" in seen.labels[True] and "k_dw3x3" in seen.labels[False], seen.labels


# ---- mv_gaussian_blur_f32 / _u8 / _f16 / _bf16 -----------------------------------------------------------------------------------
BLUR_SIZES = [(3, 3), (5, 5), (7, 3), (9, 9), (11, 3), (1, 1)]  # (kx, ky)
U8X16_WIDTHS = (15, 16, 17, 19, 20, 21, 31, 32, 33, 35, 36, 48, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260, 511, 512, 513, 1023,
                1024, 1025, 1040)
TINY_WIDTHS = (1, 2, 3, 4, 5, 7, 8)
BLUR_WIDTHS_F = {(3, 3): TINY_WIDTHS + (16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260, 513, 1024, 1025),
                 (5, 5): (3, 4, 5, 8, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257, 260, 1024, 1025)}
BLUR_WIDTHS_OTHER = (8, 16, 19, 20, 33, 36, 64, 129, 260, 1025, 1040)


def _blur_want(x, tx, ty):
    """ref.gaussian_blur; for the half types .float() -> ref.gaussian_blur -> .to(dtype)."""
    if x.dtype in (F16, BF16):
        return _t(ref.gaussian_blur(x.float().numpy(), tx, ty)).to(x.dtype)
    return _t(ref.gaussian_blur(x.numpy(), tx, ty))


def _image(shape, dtype, seed):
    if dtype in (U8, F32):
        return _pixels(shape, dtype, seed)
    return _pixels(shape, F32, seed).to(dtype)


@pytest.mark.parametrize("dtype", [F32, U8, F16, BF16], ids=["f32", "u8", "f16", "bf16"])
def test_gaussian_blur(dtype):
    lib = _lib.load()
    name = {F32: "f32", U8: "u8", F16: "f16", BF16: "bf16"}[dtype]
    fn = getattr(lib, f"mv_gaussian_blur_{name}")
    u8 = dtype == U8
    seen = _Seen()
    refused = 0
    for kx, ky in BLUR_SIZES:
        tx, ty = _k1d(kx, 0.5 + kx / 5.0), _k1d(ky, 0.4 + ky / 4.0)
        if u8 and (kx, ky) in ((3, 3), (5, 5)):
            widths = TINY_WIDTHS + U8X16_WIDTHS
        elif dtype in (F16, BF16):  # the tile kernel at one tile width: W % 4 and the column tiles are what matter
            widths = {(3, 3): TINY_WIDTHS + (255, 256, 257, 260, 1024, 1025), (5, 5): (3, 4, 8, 256, 257, 260)}.get((kx, ky), (8, 20, 260, 1025))
        else:
            widths = BLUR_WIDTHS_F.get((kx, ky), BLUR_WIDTHS_OTHER)
        for i, w in enumerate(widths):
            for h in _heights(i + kx):
                x = _image((PLANES, h, w), dtype, seed=1000 * h + w + kx)
                what = f"gaussian_blur {name} {kx}x{ky} ({h}, {w})"
                args = (PLANES, h, w, _taps(tx), kx, _taps(ty), ky)
                if kx // 2 >= w or ky // 2 >= h:
                    _refused(what, fn, x, x.shape, args + (_stream(),), INVALID)
                    refused += 1
                    continue
                want = _blur_want(x, tx, ty)
                # the uint8 16-pixel kernels take any alignment: there the pointer decides nothing
                full = w % 4 == 0 and not (u8 and w >= 16 and max(kx, ky) <= 7)
                for xo, yo in _offsets(dtype.itemsize, full):
                    tag = f"{what} x_offset={xo} y_offset={yo}"
                    kernel = _run(tag, lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), *args, _stream()), [x], [xo],
                                  [(x.shape, dtype, yo)], [want])
                    _expect_2d(kernel, tag, dtype, w, _ptr_ok(xo, dtype), _ptr_ok(yo, dtype))
                    seen.note(kernel, _aligned(xo, yo))
    seen.report(f"mv_gaussian_blur_{name}")
    assert refused
    if u8:
        seen.require("k_dw3x3_u8")
        seen.require("k_dwk_u8<5x5,2d>")
        seen.require("k_dwk_u8<3x7,2d>")
        seen.require("k_dwtile<u8,9x9,")
        assert "k_dw3x3" in seen.labels[True] and "k_dw3x3" in seen.labels[False], seen.labels
    else:
        head = _dwtile_head(dtype)
        seen.require(head, "tw256>")
        seen.require(head, "scalar")
        seen.require(head, "vec16", aligned=(True,))
        if dtype == F32:
            seen.require("k_dw3x3")
            seen.require(head, "tw128>")
            seen.require(head, "tw32>")
        else:  # 4-byte but not 8-byte aligned: the scalar instantiation
            seen.never("vec16", False)


# ---- mv_gaussian_blur_u8_ws -----------------------------------------------------------------------------------------------------
def test_gaussian_blur_u8_ws():
    lib = _lib.load()
    fn = lib.mv_gaussian_blur_u8_ws
    seen = _Seen()
    with_ws = without_ws = refused_misaligned = 0
    widths = (8, 12, 16, 17, 20, 33, 36, 64, 260, 512, 513, 1024, 1025, 1040)
    # the last row: k_sepstream<u8,ties> in 64-row strips (stream_launch: 128 rows only from 4096 waves up, which no test-sized
    # batch reaches) -- two strips with one row in the second, three with the last partly filled, and the tie list across them
    sweeps = ((5, (3, 8, 33), widths), (9, (7, 9, 17), widths), (23, (12, 17, 33), widths), (23, (65, 129), (12, 33, 260, 513)))
    refused = 0
    for k, heights, ws_widths in sweeps:
        tx, ty = _k1d(k, 1.0 + k / 6.0), _k1d(k, 0.8 + k / 5.0)
        for i, w in enumerate(ws_widths):
            for h in _heights(i, heights):
                x = _pixels((PLANES, h, w), U8, seed=1000 * h + w + k)
                args = (PLANES, h, w, _taps(tx), k, _taps(ty), k)
                call = lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), *args, ws, nb, _stream())  # noqa: E731
                ws_bytes = int(lib.mv_gaussian_blur_u8_workspace_bytes(PLANES, h, w, k, k))
                what = f"gaussian_blur_u8_ws {k}x{k} ({h}, {w}) workspace_bytes={ws_bytes}"
                if k // 2 >= w:  # reflect padding not smaller than the image: refused, with a workspace offered all the same
                    assert ws_bytes == 0, what
                    _refused_call(what, call, [x], [A], [(x.shape, U8, A)], INVALID, ws_bytes=4096)
                    refused += 1
                    continue
                want = _t(ref.gaussian_blur(x.numpy(), tx, ty))
                with_ws += ws_bytes > 0
                without_ws += ws_bytes == 0
                if ws_bytes and refused_misaligned < 4:  # a workspace that is 8-byte but not 16-byte aligned is refused
                    _refused_call(what + " workspace at 8 mod 16", call, [x], [A], [(x.shape, U8, A)], INVALID, ws_bytes=ws_bytes,
                                  ws_offset=8)
                    refused_misaligned += 1
                for xo, yo in _offsets(1, False):
                    tag = f"{what} x_offset={xo} y_offset={yo}"
                    kernel = _run(tag, call, [x], [xo], [(x.shape, U8, yo)], [want], ws_bytes=ws_bytes)
                    assert kernel.endswith("+k_u8_tie_fixup") == (ws_bytes > 0), (tag, kernel)
                    seen.note(kernel, _aligned(xo, yo))
    seen.report("mv_gaussian_blur_u8_ws")
    assert with_ws and without_ws and refused and refused_misaligned
    seen.require("k_dwk_u8<separable,ties>+k_u8_tie_fixup")
    seen.require("k_sepstream<u8,ties>+k_u8_tie_fixup")
    seen.require("k_dwk_u8<5x5,2d>")  # workspace_bytes == 0: the call is mv_gaussian_blur_u8


# ---- mv_separable_blur_f32 --------------------------------------------------------------------------------------------------------
def _expect_separable_f32(kernel, what, kx, ky, h, w, all_aligned):
    """mv_separable_blur_f32 (csrc/abi.hip): k_sepfast for sides <= 7 on 16-byte pointers and rows, k_sepstream for a side above
    7 on W >= 8, else the LDS kernel."""
    if kx <= 7 and ky <= 7 and all_aligned and w % 4 == 0 and w >= 8 and h >= 8:
        assert kernel == f"k_sepfast<{max(kx, ky, 3)},blur>", (what, kernel)
    elif (kx > 7 or ky > 7) and w >= 8:
        assert kernel == "k_sepstream", (what, kernel)
    else:
        assert kernel == "k_separable", (what, kernel)


SEP_F32 = [  # (kx, ky), widths, heights
    ((3, 3), (2, 4, 5, 7, 8, 12, 16, 17, 64, 255, 256, 257, 260, 1024, 1040), HEIGHTS),
    ((5, 5), (3, 4, 7, 8, 9, 64, 65, 256, 260, 1024, 1025), (3, 7, 8, 9, 17, 33)),
    ((7, 7), (4, 7, 8, 12, 63, 64, 256, 257, 1040), (4, 7, 8, 9, 17, 33)),
    ((7, 3), (4, 8, 9, 64, 260), (2, 7, 8, 17)),
    ((9, 9), (5, 7, 8, 9, 12, 33, 64, 255, 256, 257, 260, 1025), (5, 7, 8, 9, 17, 33)),
    ((23, 23), (12, 15, 16, 33, 64, 256, 257, 1025), (12, 17, 33)),
    ((63, 1), (32, 33, 64, 255, 256, 1025), (1, 2, 9)),
    # k_sepstream in more than one strip: stream_launch takes 64-row strips below 4096 waves (128 from there up, which no
    # test-sized batch reaches), so 65 is one row into a second strip and 129 one row into a third
    ((9, 9), (8, 9, 33, 260), (65, 129)),
    ((23, 23), (12, 64, 257), (65, 129)),
    ((63, 1), (33, 256), (65,)),
]


def test_separable_blur_f32():
    lib = _lib.load()
    fn = lib.mv_separable_blur_f32
    seen = _Seen()
    refused = 0
    for (kx, ky), widths, heights in SEP_F32:
        tx, ty = _k1d(kx, 1.1), _k1d(ky, 2.0)
        for i, w in enumerate(widths):
            for h in _heights(i, heights):
                x = _pixels((PLANES, h, w), F32, seed=1000 * h + w + kx)
                args = (PLANES, h, w, _taps(tx), kx, _taps(ty), ky)
                if kx // 2 >= w or ky // 2 >= h:
                    _refused(f"separable_blur_f32 {kx}x{ky} ({h}, {w})", fn, x, x.shape, args + (_stream(),), INVALID)
                    refused += 1
                    continue
                want = _t(ref.separable_blur(x.numpy(), tx, ty))
                for xo, yo in _offsets(4, w % 4 == 0 and kx <= 7):
                    tag = f"separable_blur_f32 {kx}x{ky} ({h}, {w}) x_offset={xo} y_offset={yo}"
                    kernel = _run(tag, lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), *args, _stream()), [x], [xo],
                                  [(x.shape, F32, yo)], [want])
                    _expect_separable_f32(kernel, tag, kx, ky, h, w, _aligned(xo, yo))
                    seen.note(kernel, _aligned(xo, yo))
    seen.report("mv_separable_blur_f32")
    assert refused
    for k in (3, 5, 7):
        seen.require(f"k_sepfast<{k},blur>", aligned=(True,))
    seen.never("k_sepfast", False)  # sepfast_supported: 16-byte pointers only
    seen.require("k_sepstream")
    seen.require("k_separable")


# ---- mv_separable_blur_u8 ---------------------------------------------------------------------------------------------------------
# Strip heights met here: k_dwk_u8's separable form starts from 48..128-row strips, which dwk_plan halves down to 6..8 rows for
# launches this small, so 7, 8, 9 and 17 sit on its strip boundaries (49 and 65 only add strips); k_sepstream: 64 rows.
SEP_U8 = [  # (kx, ky), widths, heights
    ((5, 5), (15,) + U8X16_WIDTHS[1:], (3, 7, 8, 9, 17, 33, 65)),
    ((7, 3), (15, 16, 17, 20, 33, 36, 64, 260, 513, 1025), (2, 9, 49)),
    ((9, 9), (7, 8, 12, 15, 16, 17, 19, 20, 21, 33, 35, 36, 48, 64, 65, 129, 257, 260, 512, 513, 1024, 1025, 1040), (5, 8, 9, 17, 49)),
    ((9, 7), (8, 15, 16, 19, 20, 36, 64, 260, 1025), (4, 9, 49)),
    ((23, 23), (12, 15, 16, 33, 64, 255, 256, 257, 260, 1025), (12, 17, 33)),
    ((63, 5), (32, 33, 64, 255, 256, 257, 1025), (3, 9, 17)),
    # k_sepstream in more than one 64-row strip (see SEP_F32): 9 x 9 reaches it below W = 16 only
    ((9, 9), (8, 12, 15), (65, 129)),
    ((23, 23), (12, 16, 33, 257, 1025), (65, 129)),
    ((63, 5), (33, 256), (65,)),
]


def test_separable_blur_u8():
    lib = _lib.load()
    fn = lib.mv_separable_blur_u8
    seen = _Seen()
    refused = 0
    for (kx, ky), widths, heights in SEP_U8:
        tx, ty = _k1d(kx, 1.0 + kx / 6.0), _k1d(ky, 1.0 + ky / 6.0)
        x16 = kx <= 9 and ky <= 9  # sep_u8x16_sides: {3, 5, 7}^2 and 9 x 9, 9 x 7, 7 x 9
        for i, w in enumerate(widths):
            for h in _heights(i, heights):
                x = _pixels((PLANES, h, w), U8, seed=1000 * h + w + kx)
                args = (PLANES, h, w, _taps(tx), kx, _taps(ty), ky)
                what = f"separable_blur_u8 {kx}x{ky} ({h}, {w})"
                if (x16 and w < 16 and max(kx, ky) <= 7) or w < 8:  # below W = 16 with sides <= 7; below W = 8 with larger ones
                    _refused(what, fn, x, x.shape, args + (_stream(),), UNSUPPORTED)
                    refused += 1
                    continue
                want = _t(ref.separable_blur_u8(x.numpy(), tx, ty))
                for xo, yo in _offsets(1, False):
                    tag = f"{what} x_offset={xo} y_offset={yo}"
                    kernel = _run(tag, lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), *args, _stream()), [x], [xo],
                                  [(x.shape, U8, yo)], [want])
                    if x16 and w >= 16:
                        assert kernel == f"k_dwk_u8<{max(ky, 3)}x{max(kx, 3)},separable>", (tag, kernel)
                    else:
                        assert kernel == "k_sepstream", (tag, kernel)
                    seen.note(kernel, _aligned(xo, yo))
    seen.report("mv_separable_blur_u8")
    assert refused
    for size in ("5x5", "3x7", "9x9", "7x9"):
        seen.require(f"k_dwk_u8<{size},separable>")
    seen.require("k_sepstream")


# ---- mv_sobel_f32, mv_gaussian_sobel_f32 ----------------------------------------------------------------------------------------
def _pair_offsets(w):
    """(x, gx, gy) offsets: all aligned, then each pointer odd alone, then all odd."""
    if w % 4:
        return [(A, A, A), (1, A, 3), (A, 3, 1), (1, 3, 3)]
    return [(A, A, A), (1, A, A), (A, 3, A), (A, A, 1), (1, 3, 1)]


@pytest.mark.parametrize("border", ["reflect", "zero", "valid"])
def test_sobel(border):
    lib = _lib.load()
    fn = lib.mv_sobel_f32
    b = BORDERS[border]
    seen = _Seen()
    refused = 0
    for i, w in enumerate(TINY_WIDTHS + (16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260, 512, 513)):
        for h in _heights(i):
            x = _pixels((PLANES, h, w), F32, seed=1000 * h + w)
            what = f"sobel {border} ({h}, {w})"
            if (b == REFLECT and (h < 2 or w < 2)) or (b == VALID and (h < 3 or w < 3)):
                xbuf, xv = G.guarded(x, F32, DEV, A, sentinel=NAN)
                ybuf, yv = G.guarded((2, PLANES, h, w), F32, DEV, A)
                ybefore = ybuf.cpu()
                rc = fn(xv.data_ptr(), yv[0].data_ptr(), yv[1].data_ptr(), PLANES, h, w, b, _stream())
                torch.cuda.synchronize()
                assert rc == INVALID, (what, rc)
                G.assert_unchanged(ybuf, ybefore, what + ": outputs of a refused call")
                refused += 1
                continue
            gx, gy = (_t(a) for a in ref.sobel(x.numpy(), b))
            for xo, go, ho in _pair_offsets(w):
                tag = f"{what} x_offset={xo} gx_offset={go} gy_offset={ho}"
                kernel = _run(tag, lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), yv[1].data_ptr(), PLANES, h, w, b,
                                                            _stream()), [x], [xo], [(gx.shape, F32, go), (gy.shape, F32, ho)], [gx, gy])
                if b == VALID:  # two launches of the tile kernel; the label is the second one's (x -> gy)
                    assert kernel.startswith("k_dwtile<f32,3x3,"), (tag, kernel)
                    assert (",vec16," in kernel) == (w % 4 == 0 and xo == A and ho == A), (tag, kernel)
                else:
                    assert kernel == "k_dw3x3", (tag, kernel)
                seen.note(kernel, xo == go == ho == A)
    seen.report(f"mv_sobel_f32 {border}")
    assert refused or b == ZERO
    seen.require("k_dwtile<f32,3x3," if b == VALID else "k_dw3x3")


def test_gaussian_sobel():
    lib = _lib.load()
    fn = lib.mv_gaussian_sobel_f32
    seen = _Seen()
    refused = 0
    for k, heights in ((3, (2, 7, 8, 9, 17, 49)), (5, (3, 7, 8, 9, 33, 49)), (9, (5, 8, 9, 17))):
        tx, ty = _k1d(k, 1.1), _k1d(k, 2.0)
        for i, w in enumerate((2, 4, 5, 7, 8, 9, 12, 16, 17, 64, 255, 256, 257, 260, 1024)):
            for h in _heights(i, heights):
                x = _pixels((PLANES, h, w), F32, seed=1000 * h + w + k)
                args = (PLANES, h, w, _taps(tx), k, _taps(ty), k)
                what = f"gaussian_sobel {k}x{k} ({h}, {w})"
                if k // 2 >= w or k // 2 >= h:
                    xbuf, xv = G.guarded(x, F32, DEV, A, sentinel=NAN)
                    ybuf, yv = G.guarded((2, PLANES, h, w), F32, DEV, A)
                    ybefore = ybuf.cpu()
                    rc = fn(xv.data_ptr(), yv[0].data_ptr(), yv[1].data_ptr(), *args, _stream())
                    torch.cuda.synchronize()
                    assert rc == INVALID, (what, rc)
                    G.assert_unchanged(ybuf, ybefore, what + ": outputs of a refused call")
                    refused += 1
                    continue
                gx, gy = (_t(a) for a in ref.gaussian_sobel(x.numpy(), tx, ty))
                for xo, go, ho in _pair_offsets(w):
                    tag = f"{what} x_offset={xo} gx_offset={go} gy_offset={ho}"
                    kernel = _run(tag, lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), yv[1].data_ptr(), *args,
                                                                _stream()), [x], [xo], [(gx.shape, F32, go), (gy.shape, F32, ho)],
                                  [gx, gy])
                    al = xo == go == ho == A
                    fast = k <= 7 and al and w % 4 == 0 and w >= 8 and h >= 8
                    assert kernel == (f"k_sepfast<{k},sobel>" if fast else "k_separable"), (tag, kernel)
                    seen.note(kernel, al)
    seen.report("mv_gaussian_sobel_f32")
    assert refused
    seen.require("k_sepfast<3,sobel>", aligned=(True,))
    seen.require("k_sepfast<5,sobel>", aligned=(True,))
    seen.never("k_sepfast", False)
    seen.require("k_separable")


# ---- mv_sharpness_f32 / _u8 --------------------------------------------------------------------------------------------------------
FACTORS = (0.0, 0.4, 1.0, 2.3)
SHARP_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 19, 20, 21, 33, 36, 64, 65, 128, 129, 256, 257, 260, 513, 1025)


@pytest.mark.parametrize("v1", [0, 1], ids=["v2", "v1"])
@pytest.mark.parametrize("dtype", [F32, U8], ids=["f32", "u8"])
def test_sharpness(dtype, v1):
    lib = _lib.load()
    u8 = dtype == U8
    seen = _Seen()
    copies = 0
    for i, w in enumerate(SHARP_WIDTHS):
        for h in _heights(i):
            x = _pixels((PLANES, h, w), dtype, seed=1000 * h + w)
            for f in FACTORS:
                want = _t(ref.adjust_sharpness(x.numpy(), f, v1=bool(v1)))
                if h <= 2 or w <= 2:
                    assert torch.equal(want, x)  # a device copy of the input
                if u8:
                    call = lambda xv, yv, ws, nb: lib.mv_sharpness_u8(xv[0].data_ptr(), yv[0].data_ptr(), PLANES, h, w, f, v1,  # noqa: E731
                                                                     _stream())
                else:
                    call = lambda xv, yv, ws, nb: lib.mv_sharpness_f32(xv[0].data_ptr(), yv[0].data_ptr(), PLANES, h, w, f, v1,  # noqa: E731
                                                                      1.0, 0, _stream())
                offsets = _offsets(dtype.itemsize, w % 4 == 0 and f == 0.4)
                if f != 0.4:
                    offsets = [offsets[0], offsets[1 + FACTORS.index(f) % 3]]
                for xo, yo in offsets:
                    tag = f"sharpness {dtype} v1={v1} factor={f} ({h}, {w}) x_offset={xo} y_offset={yo}"
                    kernel = _run(tag, call, [x], [xo], [(x.shape, dtype, yo)], [want])
                    if h <= 2 or w <= 2:  # a device copy (no kernel, so no label of its own): values and guards are the check
                        copies += 1
                        continue
                    assert kernel == ("k_dw3x3_u8" if u8 and w >= 16 else "k_dw3x3"), (tag, kernel)
                    seen.note(kernel, _aligned(xo, yo))
    seen.report(f"mv_sharpness {dtype} v1={v1}")
    assert copies
    assert "k_dw3x3" in seen.labels[True] and "k_dw3x3" in seen.labels[False], seen.labels
    if u8:
        seen.require("k_dw3x3_u8")


# ---- mv_gaussian_blur_f64, mv_depthwise_conv2d_f64, mv_sharpness_f64 ---------------------------------------------------------------
def _pixels64(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=F64) * (160.0 / 255.0) + 40.0 / 255.0


F64_WIDTHS = (1, 2, 3, 5, 8, 63, 64, 65, 129)
F64_HEIGHTS = (1, 2, 3, 9, 16, 17, 33)


def test_gaussian_blur_f64():
    lib = _lib.load()
    fn = lib.mv_gaussian_blur_f64
    seen = _Seen()
    refused = 0
    for kx, ky in ((3, 3), (5, 5), (7, 3), (9, 9), (1, 1)):
        tx, ty = _k1d(kx, 0.5 + kx / 5.0, F64), _k1d(ky, 0.4 + ky / 4.0, F64)
        ax, ay = _lib.taps64_from_tensor(_t(tx)), _lib.taps64_from_tensor(_t(ty))
        for i, w in enumerate(F64_WIDTHS):
            for h in _heights(i + kx, F64_HEIGHTS):
                x = _pixels64((PLANES, h, w), seed=1000 * h + w)
                args = (PLANES, h, w, ax, kx, ay, ky)
                what = f"gaussian_blur_f64 {kx}x{ky} ({h}, {w})"
                if kx // 2 >= w or ky // 2 >= h:
                    _refused(what, fn, x, x.shape, args + (_stream(),), INVALID)
                    refused += 1
                    continue
                want = _t(ref.gaussian_blur_f64(x.numpy(), tx, ty))
                for xo, yo in _offsets(8, False):  # an odd offset is 8-byte but not 16-byte aligned
                    tag = f"{what} x_offset={xo} y_offset={yo}"
                    kernel = _run(tag, lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), *args, _stream()), [x], [xo],
                                  [(x.shape, F64, yo)], [want])
                    assert kernel == f"k_dwf64<{ky}x{kx}>", (tag, kernel)
                    seen.note(kernel, _aligned(xo, yo))
    seen.report("mv_gaussian_blur_f64")
    assert refused
    seen.require("k_dwf64<")


@pytest.mark.parametrize("border", ["reflect", "zero", "valid"])
def test_depthwise_f64(border):
    lib = _lib.load()
    fn = lib.mv_depthwise_conv2d_f64
    b = BORDERS[border]
    seen = _Seen()
    refused = 0
    for ky, kx in ((3, 3), (5, 3), (7, 7)):
        g = torch.Generator().manual_seed(ky * 31 + kx)
        w2 = (torch.rand((ky, kx), generator=g, dtype=F64) - 0.5).numpy()
        for i, w in enumerate(F64_WIDTHS):
            for h in _heights(i + ky, F64_HEIGHTS):
                x = _pixels64((PLANES, h, w), seed=1000 * h + w + 1)
                what = f"depthwise_f64 {border} {ky}x{kx} ({h}, {w})"
                if (b == REFLECT and (ky // 2 >= h or kx // 2 >= w)) or (b == VALID and (ky > h or kx > w)):
                    tb, tv, _ = _device_taps(w2, F64, A)
                    _refused(what, fn, x, x.shape, (tv.data_ptr(), PLANES, h, w, ky, kx, b, _stream()), INVALID)
                    refused += 1
                    continue
                want = _t(ref.depthwise_conv2d_f64(x.numpy(), w2, b))
                for xo, yo in _offsets(8, False):
                    tag = f"{what} x_offset={xo} y_offset={yo}"
                    tb, tv, twas = _device_taps(w2, F64, yo)
                    kernel = _run(tag, lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), tv.data_ptr(), PLANES, h, w, ky, kx,
                                                                b, _stream()), [x], [xo], [(want.shape, F64, yo)], [want],
                                  fixed=((tb, twas, "device taps"),))
                    assert kernel == f"k_dwf64<{ky}x{kx}>", (tag, kernel)
                    seen.note(kernel, _aligned(xo, yo))
    seen.report(f"mv_depthwise_conv2d_f64 {border}")
    assert refused or b == ZERO
    seen.require("k_dwf64<")


def test_sharpness_f64():
    lib = _lib.load()
    fn = lib.mv_sharpness_f64
    seen = _Seen()
    copies = 0
    for i, w in enumerate((1, 2, 3, 4, 5, 8, 63, 64, 65, 257)):
        for h in _heights(i, F64_HEIGHTS):
            x = _pixels64((PLANES, h, w), seed=1000 * h + w + 2)
            for v1 in (0, 1):
                for f in FACTORS:
                    want = _t(ref.adjust_sharpness_f64(x.numpy(), f, v1=bool(v1)))
                    offsets = _offsets(8, False)
                    for xo, yo in (offsets if f == 0.4 else [offsets[0], offsets[3]]):
                        tag = f"sharpness_f64 v1={v1} factor={f} ({h}, {w}) x_offset={xo} y_offset={yo}"
                        kernel = _run(tag, lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), PLANES, h, w, f, v1, _stream()),
                                      [x], [xo], [(x.shape, F64, yo)], [want])
                        if h <= 2 or w <= 2:
                            assert torch.equal(want, x), tag  # a device copy: values and guards are the check
                            copies += 1
                            continue
                        assert kernel == "k_sharp_f64", (tag, kernel)
                        seen.note(kernel, _aligned(xo, yo))
    seen.report("mv_sharpness_f64")
    assert copies
    seen.require("k_sharp_f64")


# ---- the six *_v entry points ------------------------------------------------------------------------------------------------------
def _frames_case(what, fn, args, frames, offsets, wants, dtype):
    """One *_v call: every frame and every output in a guarded buffer of its own, at its own offset."""
    n = len(frames)

    def call(xv, yv, ws, nb):
        return fn(_lib.pointer_table(xv), _lib.pointer_table(yv), n, *args, _stream())

    return _run(what, call, frames, offsets, [(f.shape, dtype, o) for f, o in zip(frames, offsets)], wants)


def _frame_offsets(n, odd_frame):
    """All frames 16-byte aligned (the table path), or one frame at an odd offset (one launch per frame)."""
    odd = 1
    return [odd if i == odd_frame else A for i in range(n)]


V_ENTRIES = {  # name -> (dtype, reference(x, tx, ty) or None for sharpness)
    "gaussian_blur_f32_v": (F32, ref.gaussian_blur), "gaussian_blur_u8_v": (U8, ref.gaussian_blur),
    "separable_blur_f32_v": (F32, ref.separable_blur), "separable_blur_u8_v": (U8, ref.separable_blur_u8),
    "sharpness_f32_v": (F32, None), "sharpness_u8_v": (U8, None),
}


@pytest.mark.parametrize("entry", list(V_ENTRIES))
def test_frame_lists(entry):
    lib = _lib.load()
    fn = getattr(lib, "mv_" + entry)
    dtype, reference = V_ENTRIES[entry]
    seen = _Seen()
    refused = 0
    if reference is None:
        variants = [(f, v1) for v1 in (0, 1) for f in (0.4, 2.3)]
    else:
        variants = [(3, 3), (5, 5), (9, 9)] if "gaussian" in entry else [(5, 5), (7, 3), (9, 9), (23, 23)]
    # (frames, planes per frame, h, w); the last: 113 tiny frames cross kMaxFrames = 112 (two launches on the table path)
    shapes = [(3, 1, 9, 16), (5, 3, 17, 64), (3, 3, 9, 260), (5, 1, 33, 20), (3, 2, 2, 24), (113, 1, 3, 16)]
    for n, ppf, h, w in shapes:
        batch = _pixels((n, ppf, h, w), dtype, seed=h + w)  # one reference call per variant: the planes are independent
        frames = list(batch)
        for variant in variants:
            if reference is None:
                f, v1 = variant
                wants = list(_t(ref.adjust_sharpness(batch.numpy(), f, v1=bool(v1))))
                args = (ppf, h, w, f, v1) + ((1.0, 0) if dtype == F32 else ())
            else:
                kx, ky = variant
                tx, ty = _k1d(kx, 0.5 + kx / 5.0), _k1d(ky, 0.4 + ky / 4.0)
                if kx // 2 >= w or ky // 2 >= h:  # refused on the table path and on the per-frame path alike
                    args = (ppf, h, w, _taps(tx), kx, _taps(ty), ky)
                    for odd_frame in (None, n - 1):
                        offs = _frame_offsets(n, odd_frame)
                        _refused_call(f"{entry} {variant} {n} frames of ({ppf}, {h}, {w}), odd frame: {odd_frame}",
                                      lambda xv, yv, ws, nb: fn(_lib.pointer_table(xv), _lib.pointer_table(yv), n, *args, _stream()),
                                      frames, offs, [(f.shape, dtype, o) for f, o in zip(frames, offs)], INVALID)
                    refused += 1
                    continue
                wants = list(_t(reference(batch.numpy(), tx, ty)))
                args = (ppf, h, w, _taps(tx), kx, _taps(ty), ky)
            for odd_frame in (None, n - 1):  # the last launch, whose label is read, is the odd frame's
                what = f"{entry} {variant} {n} frames of ({ppf}, {h}, {w}), odd frame: {odd_frame}"
                kernel = _frames_case(what, fn, args, frames, _frame_offsets(n, odd_frame), wants, dtype)
                if reference is None and (h <= 2 or w <= 2):  # device copies, one per frame
                    continue
                seen.note(kernel, odd_frame is None)
    seen.report("mv_" + entry)
    assert refused or reference is None
    family = {"gaussian_blur_f32_v": ["k_dwtile<f32", "k_dw3x3"], "gaussian_blur_u8_v": ["k_dw3x3_u8", "k_dwk_u8<5x5,2d>", "k_dwtile<u8"],
              "separable_blur_f32_v": ["k_sepstream", "k_separable"], "separable_blur_u8_v": ["k_dwk_u8<5x5,separable>", "k_sepstream"],
              "sharpness_f32_v": ["k_dw3x3"], "sharpness_u8_v": ["k_dw3x3_u8"]}[entry]
    for part in family:
        seen.require(part)
    if entry == "separable_blur_f32_v":
        seen.require("k_sepfast<5,blur>", aligned=(True,))
        seen.never("k_sepfast", False)


# ---- planes 1 and 5 on narrow images: the (plane, strip) units of k_dw3x3, k_dw3x3_u8 and k_dwk_u8 ----------------------------------
@pytest.mark.parametrize("dtype", [F32, U8], ids=["f32", "u8"])
def test_plane_counts(dtype):
    """Images narrower than a wave's 64 lanes put 64 / lpr (plane, strip) units into one wave, across plane boundaries; the
    sweeps above run 3 planes.  One plane has fewer units than a wave has lane groups (the idle groups are clamped to the last
    unit and must store nothing), five give another tail and another plane stride.  Heights 9 and 33: two and five 8-row strips
    (k_dw3x3, k_dwk_u8 after dwk_plan's halving), one and two 32-row strips (k_dw3x3_u8)."""
    lib = _lib.load()
    u8 = dtype == U8
    name = "u8" if u8 else "f32"
    seen = _Seen()
    t3, t5 = _k1d(3, 0.8), _k1d(5, 1.1)
    w9 = _depthwise_taps(3, 3, "avg", seed=9)
    host9 = _taps(w9)
    for planes in (1, 5):
        for w in ((5, 8, 16, 17, 20, 33, 48, 64) if u8 else (5, 8, 16, 33, 64, 128)):
            for h in (9, 33):
                x = _pixels((planes, h, w), dtype, seed=1000 * h + w + planes)
                xn = x.numpy()
                dw = ref.depthwise_conv2d(xn.astype(np.float32), w9, ZERO)
                cases = [
                    ("gaussian_blur 3x3", getattr(lib, f"mv_gaussian_blur_{name}"), (planes, h, w, _taps(t3), 3, _taps(t3), 3),
                     _t(ref.gaussian_blur(xn, t3, t3))),
                    ("depthwise 3x3 zero", getattr(lib, f"mv_depthwise_conv2d_{name}"),
                     (C.cast(host9, C.c_void_p), 0, planes, h, w, 3, 3, ZERO), _t(np.rint(dw).astype(np.uint8)) if u8 else _t(dw)),
                    ("sharpness v2 0.4", getattr(lib, f"mv_sharpness_{name}"), (planes, h, w, 0.4, 0) + (() if u8 else (1.0, 0)),
                     _t(ref.adjust_sharpness(xn, 0.4))),
                ]
                if u8:
                    cases.append(("gaussian_blur 5x5", lib.mv_gaussian_blur_u8, (planes, h, w, _taps(t5), 5, _taps(t5), 5),
                                  _t(ref.gaussian_blur(xn, t5, t5))))
                if u8 and w >= 16:
                    cases.append(("separable_blur 5x5", lib.mv_separable_blur_u8, (planes, h, w, _taps(t5), 5, _taps(t5), 5),
                                  _t(ref.separable_blur_u8(xn, t5, t5))))
                for label, fn, args, want in cases:
                    for xo, yo in ((A, A), (1, 37 if u8 else 3)):
                        tag = f"{label} {name} planes={planes} ({h}, {w}) x_offset={xo} y_offset={yo}"
                        kernel = _run(tag, lambda xv, yv, ws, nb: fn(xv[0].data_ptr(), yv[0].data_ptr(), *args, _stream()), [x], [xo],
                                      [(x.shape, dtype, yo)], [want])
                        seen.note(kernel, _aligned(xo, yo))
    seen.report(f"planes 1 and 5, {name}")
    assert "k_dw3x3" in seen.labels[True] and "k_dw3x3" in seen.labels[False], seen.labels
    if u8:
        seen.require("k_dw3x3_u8")
        seen.require("k_dwk_u8<5x5,2d>")
        seen.require("k_dwk_u8<5x5,separable>")
