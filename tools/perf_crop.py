#!/usr/bin/env python3
"""pad / flip / erase / RandomCrop / resized_crop on one MI355X: time per call (HIP events, median of 7 rounds of `--iters`
back-to-back calls after a warm-up, the two sides of a comparison alternating round by round), algorithmic bytes (window read
+ output written), TB/s and the fraction of the 8 TB/s HBM peak, and the same ops composed with torch on the same GPU.

  python tools/perf_crop.py [--iters 5] [--parent-lib PATH]

Cases: 32 x 3 x 1080p, 256 x 3 x 224^2 and 4096 x 3 x 32^2 (the CIFAR recipe), uint8 and float32: pad(4, reflect), hflip,
out-of-place erase, RandomCrop(padding=4) as one launch, resized_crop -> 224 against F.resize(image[window].contiguous()) (what
the package offered before the source window) and resized_crop_flip_normalize against its four composed calls.
--parent-lib: a libmi355vision.so built from the parent commit; the existing F.resize / preset entry points are then timed
on both libraries in alternating rounds, with the parent measured twice to show its own run-to-run spread."""
import argparse
import ctypes
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from cpu_vision_amd import _lib, functional as F  # noqa: E402

PEAK_TBS = 8.0
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def alternate(fns, iters, rounds=7):
    """Median ms per call of each fn, the fns taking turns round by round."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / iters)
    return [sorted(t)[len(t) // 2] for t in ts]


def compare(what, ours, ref, nbytes, iters, ref_name="torch composition"):
    ours()
    kernel = _lib.last_kernel()
    ms, ms_ref = alternate([ours, ref], iters)
    tbs = nbytes / (ms * 1e-3) / 1e12
    print(f"{what:52s} {ms:8.4f} ms  {nbytes / 1e9:6.3f} GB  {tbs:5.2f} TB/s  {tbs / PEAK_TBS * 100:5.1f} % of 8 TB/s  {kernel}")
    print(f"  {ref_name:50s} {ms_ref:8.4f} ms  -> {ms_ref / ms:.2f}x", flush=True)


def image(shape, dtype):
    g = torch.Generator(device="cuda").manual_seed(0)
    if dtype == torch.uint8:
        return torch.empty(shape, dtype=dtype, device="cuda").random_(0, 256, generator=g)
    return torch.rand(shape, dtype=dtype, device="cuda", generator=g)


def parent_cases(path, iters):
    parent = ctypes.CDLL(path)
    for name in ("mv_resize_workspace_bytes", "mv_resize_bilinear_aa_u8", "mv_resize_bilinear_aa_f32", "mv_preset_classification_u8",
                 "mv_preset_classification_f32"):
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    ours = _lib.load()
    m, s = _lib.taps(MEAN), _lib.taps(STD)
    print("existing resize / preset entry points: this commit against the parent library (ms per call; parent twice = its spread)")
    for shape, dtype, oh, ow, ct, cl, ch, cw in [((64, 3, 375, 500), torch.uint8, 256, 341, 16, 58, 224, 224),
                                                 ((64, 3, 375, 500), torch.float32, 256, 341, 16, 58, 224, 224),
                                                 ((24, 3, 1080, 1920), torch.uint8, 256, 455, 16, 115, 224, 224),
                                                 ((8, 3, 2160, 3840), torch.uint8, 256, 455, 16, 115, 224, 224),
                                                 ((256, 3, 224, 224), torch.uint8, 112, 112, 0, 0, 112, 112)]:
        x = image(shape, dtype)
        n, c, h, w = shape
        u8 = dtype == torch.uint8
        nbytes = int(ours.mv_resize_workspace_bytes(n * c, h, w, oh, ow, ct, cl, ch, cw))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
        sp = _lib.stream_ptr(x)
        for preset in (False, True):
            y = torch.empty((n, c, ch, cw), dtype=torch.float32 if preset else dtype, device="cuda")

            def call(lib):
                if preset:
                    fn = lib.mv_preset_classification_u8 if u8 else lib.mv_preset_classification_f32
                    return lambda: _lib.check(fn(x.data_ptr(), y.data_ptr(), n, c, h, w, oh, ow, ct, cl, ch, cw, m, s, ws.data_ptr(),
                                                 nbytes, sp))
                fn = lib.mv_resize_bilinear_aa_u8 if u8 else lib.mv_resize_bilinear_aa_f32
                return lambda: _lib.check(fn(x.data_ptr(), y.data_ptr(), n * c, h, w, oh, ow, ct, cl, ch, cw, ws.data_ptr(), nbytes, sp))

            t_new, t_par, t_par2 = alternate([call(ours), call(parent), call(parent)], iters)
            print(f"  {str(shape):22s} {str(dtype):14s} {'preset' if preset else 'resize':6s}  this {t_new:8.4f}  parent {t_par:8.4f} / "
                  f"{t_par2:8.4f}  this/parent {t_new / min(t_par, t_par2):.3f}  parent spread {abs(t_par - t_par2) / min(t_par, t_par2):.3f}",
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    it = args.iters
    for shape in [(32, 3, 1080, 1920), (256, 3, 224, 224), (4096, 3, 32, 32)]:
        n, c, h, w = shape
        for dtype in (torch.uint8, torch.float32):
            x = image(shape, dtype)
            es = x.element_size()
            tag = f"{n}x{c}x{h}x{w} {str(dtype)[6:]}"
            full = x.numel() * es
            padded = n * c * (h + 8) * (w + 8) * es
            compare(f"pad(4, reflect) {tag}", lambda: F.pad(x, 4, padding_mode="reflect"),
                    lambda: torch.nn.functional.pad(x.float() if dtype == torch.uint8 else x, [4] * 4, mode="reflect").to(dtype),
                    full + padded, it)
            compare(f"hflip {tag}", lambda: F.horizontal_flip(x), lambda: x.flip(-1), 2 * full, it)
            v = torch.zeros((c, 1, 1), dtype=dtype, device="cuda")
            bh, bw = h // 3, w // 3

            def torch_erase():
                y = x.clone()
                y[..., 5:5 + bh, 7:7 + bw] = v
                return y

            compare(f"erase {tag}", lambda: F.erase(x, 5, 7, bh, bw, v), torch_erase, 2 * full - n * c * bh * bw * es, it)
            compare(f"RandomCrop(padding=4) {tag}", lambda: F.pad_crop(x, 4, 3, 5, h, w),
                    lambda: torch.nn.functional.pad(x, [4] * 4)[..., 3:3 + h, 5:5 + w].contiguous(), 2 * full, it)
            if h >= 224:
                wh, ww = (h * 3) // 4, (w * 3) // 4
                top, left = h // 8, w // 8
                out = n * c * 224 * 224
                compare(f"resized_crop -> 224 {tag}", lambda: F.resized_crop(x, top, left, wh, ww, [224, 224]),
                        lambda: F.resize(x[..., top:top + wh, left:left + ww].contiguous(), [224, 224]),
                        n * c * wh * ww * es + out * es, it, ref_name="F.resize(image[window].contiguous())")

                def composed():
                    y = F.horizontal_flip(F.resized_crop(x, top, left, wh, ww, [224, 224]))
                    return F.normalize(F.to_dtype(y, torch.float32, scale=True), MEAN, STD)

                compare(f"resized_crop_flip_normalize {tag}",
                        lambda: F.resized_crop_flip_normalize(x, top, left, wh, ww, [224, 224], True, MEAN, STD), composed,
                        n * c * wh * ww * es + out * 4, it, ref_name="the four composed calls")
            del x
    if args.parent_lib:
        parent_cases(args.parent_lib, it)


if __name__ == "__main__":
    main()
