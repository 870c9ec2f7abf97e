#!/usr/bin/env python3
"""MixUp / CutMix / label mixing on one MI355X: time per call (HIP events, median of 7 rounds of `--iters` back-to-back calls
after a warm-up, the sides of a comparison alternating round by round), algorithmic bytes (batch read once + output written
once), TB/s and the fraction of the 8 TB/s HBM peak, next to the reference composition run with torch on the same GPU.

  python tools/perf_mix.py [--iters 5] [--kernels] [--segments]
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR1 -- python tools/perf_mix.py --pmc-run
  rocprofv3 --pmc WRITE_SIZE --output-format csv -d DIR2 -- python tools/perf_mix.py --pmc-run
  python tools/perf_mix.py --pmc-read DIR1 DIR2

Cases: MixUp and CutMix on 256 x 3 x 224^2, 4096 x 3 x 32^2 and 32 x 3 x 1080p float32 (CutMix also uint8), index labels at
256 x 1000.  --kernels also times MixUp's two kernels (the walk k_mixup_roll and the two-load k_mixup_flat) through the
-DMV_TUNING library (MV_MIX_KERNEL=roll|flat); --segments the walk at several segment lengths (MV_MIX_SEG_LEN).
--pmc-run launches each MixUp kernel a few times per shape and nothing else, for a counter pass of its own (no tracing flags with
--pmc; FETCH_SIZE and WRITE_SIZE do not fit one pass, so each gets its own); --pmc-read merges the passes and prints both
counters per shape and kernel relative to the input bytes."""
import argparse
import collections
import csv
import glob
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from cpu_vision_amd import _lib, functional as F  # noqa: E402

PEAK_TBS = 8.0
SHAPES = [(256, 3, 224, 224), (4096, 3, 32, 32), (32, 3, 1080, 1920)]
LAM = 0.6180339887498949


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


def row(what, ms, nbytes, note=""):
    tbs = nbytes / (ms * 1e-3) / 1e12
    print(f"{what:52s} {ms:8.4f} ms  {nbytes / 1e9:6.3f} GB  {tbs:5.2f} TB/s  {tbs / PEAK_TBS * 100:5.1f} % of 8 TB/s  {note}", flush=True)


def compare(what, ours, ref, nbytes, iters):
    ours()
    kernel = _lib.last_kernel()
    ms, ms_ref = alternate([ours, ref], iters)
    row(what, ms, nbytes, kernel)
    print(f"  {'torch composition':50s} {ms_ref:8.4f} ms  -> {ms_ref / ms:.2f}x", flush=True)


def image(shape, dtype):
    g = torch.Generator(device="cuda").manual_seed(0)
    if dtype == torch.uint8:
        return torch.empty(shape, dtype=dtype, device="cuda").random_(0, 256, generator=g)
    return torch.rand(shape, dtype=dtype, device="cuda", generator=g)


def torch_mixup(x):
    return x.roll(1, 0).mul_(1.0 - LAM).add_(x.mul(LAM))


def torch_cutmix(x, box):
    x1, y1, x2, y2 = box
    rolled = x.roll(1, 0)
    out = x.clone()
    out[..., y1:y2, x1:x2] = rolled[..., y1:y2, x1:x2]
    return out


def torch_labels(labels, k):
    y = torch.nn.functional.one_hot(labels, num_classes=k).float()
    return y.roll(1, 0).mul_(1.0 - LAM).add_(y.mul(LAM))


def forced(env, value, fn, iters):
    """ms per call of fn through the tuning library with one knob set."""
    with _lib.tuning_library():
        os.environ[env] = value
        try:
            fn()
            kernel = _lib.last_kernel()
            ms = alternate([fn], iters)[0]
        finally:
            del os.environ[env]
    return ms, kernel


PMC_KERNELS = ("roll", "flat")
PMC_LAUNCHES = 3


def pmc_run():
    """SHAPES in order, each with PMC_LAUNCHES launches of every PMC_KERNELS entry: pmc_read() finds a dispatch's case by its
    place in this order."""
    with _lib.tuning_library():
        for shape in SHAPES:
            x = image(shape, torch.float32)
            for kernel in PMC_KERNELS:
                os.environ["MV_MIX_KERNEL"] = kernel
                for _ in range(PMC_LAUNCHES):
                    F.mixup_image(x, LAM)
                torch.cuda.synchronize()
            del os.environ["MV_MIX_KERNEL"], x
            torch.cuda.empty_cache()


def pmc_read(directories):
    """The k_mixup dispatches of each pass in dispatch order, which is pmc_run()'s order: the n-th one belongs to shape
    n // (kernels x launches) and kernel (n // launches) % kernels.  The launch constants of csrc/batchmix.hip are not repeated
    here; a pass whose dispatch count or kernel names do not fit that order is reported and not tabulated."""
    per = len(PMC_KERNELS) * PMC_LAUNCHES
    sums = collections.defaultdict(lambda: collections.defaultdict(list))
    grids = {}
    for directory in directories:
        by_counter = collections.defaultdict(dict)
        for f in glob.glob(directory + "/**/*counter_collection.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                if "k_mixup" in r["Kernel_Name"]:
                    by_counter[r["Counter_Name"]][int(r["Dispatch_Id"])] = r
        for counter, rows in by_counter.items():
            if len(rows) != per * len(SHAPES):
                print(f"{directory}: {len(rows)} k_mixup dispatches with {counter}, expected {per * len(SHAPES)}: not tabulated")
                continue
            for n, dispatch in enumerate(sorted(rows)):
                r = rows[dispatch]
                key = (SHAPES[n // per], PMC_KERNELS[(n // PMC_LAUNCHES) % len(PMC_KERNELS)])
                if "k_mixup_" + key[1] not in r["Kernel_Name"]:
                    print(f"{directory}: dispatch {dispatch} is {r['Kernel_Name']}, expected k_mixup_{key[1]}: not tabulated")
                    continue
                sums[key][counter].append(float(r["Counter_Value"]))
                grids[key] = int(r["Grid_Size"])
    print("FETCH_SIZE / WRITE_SIZE in KiB as the counters report them, mean over the dispatches")
    for shape in SHAPES:
        for kernel in PMC_KERNELS:
            key = (shape, kernel)
            if key not in sums:
                continue
            kib = shape[0] * shape[1] * shape[2] * shape[3] * 4 / 1024
            cells = []
            for counter in ("FETCH_SIZE", "WRITE_SIZE"):
                v = sums[key].get(counter)
                cells.append(f"{counter} {sum(v) / len(v):12.0f} = {sum(v) / len(v) / kib:5.3f} x input (n={len(v)})" if v else f"{counter} absent")
            print(f"  {str(shape):22s} {kernel:5s} grid {grids[key]:9d}  " + "   ".join(cells))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--segments", action="store_true")
    ap.add_argument("--pmc-run", action="store_true")
    ap.add_argument("--pmc-read", nargs="+", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.pmc_read:
        return pmc_read(args.pmc_read)
    if args.pmc_run:
        return pmc_run()
    it = args.iters
    for shape in SHAPES:
        n, c, h, w = shape
        box = (w // 4, h // 4, w // 4 + w // 2, h // 4 + h // 2)  # lam = 0.75: a quarter of the area
        for dtype in (torch.float32, torch.uint8):
            x = image(shape, dtype)
            tag = f"{n}x{c}x{h}x{w} {str(dtype)[6:]}"
            full = x.numel() * x.element_size()
            if dtype == torch.float32:
                compare(f"MixUp {tag}", lambda: F.mixup_image(x, LAM), lambda: torch_mixup(x), 2 * full, it)
                if args.kernels:
                    for kernel in ("roll", "flat"):
                        ms, name = forced("MV_MIX_KERNEL", kernel, lambda: F.mixup_image(x, LAM), it)
                        row(f"  kernel {kernel}", ms, 2 * full, name)
                if args.segments:
                    for seg in (1, 2, 4, 8, 16, 32, 64, 4096):
                        if seg <= n or seg == 4096:
                            ms, name = forced("MV_MIX_SEG_LEN", str(seg), lambda: F.mixup_image(x, LAM), it)
                            row(f"  segment length {min(seg, n)}", ms, 2 * full, name)
            compare(f"CutMix {tag}", lambda: F.cutmix_image(x, box), lambda: torch_cutmix(x, box), 2 * full, it)
            del x
            torch.cuda.empty_cache()
    labels = torch.randint(0, 1000, (256,), device="cuda")
    compare("labels 256 x 1000 int64 -> float32", lambda: F.mixup_labels(labels, LAM, num_classes=1000),
            lambda: torch_labels(labels, 1000), 256 * 8 + 256 * 1000 * 4, it)
    probs = torch.rand((256, 1000), device="cuda")
    compare("labels 256 x 1000 float32 probabilities", lambda: F.mixup_labels(probs, LAM), lambda: torch_mixup(probs),
            2 * 256 * 1000 * 4, it)


if __name__ == "__main__":
    main()
