"""The cases of the random-shape sweeps of the layer and RoI kernels (tests/test_fuzz_cases_host.py, tests/test_gpu_fuzz_layers.py,
tests/test_gpu_fuzz_ops.py): one seeded generator per family, the inputs of a case and its CPU reference.  numpy and CPU torch only;
nothing here touches a device.

A family is swept in SWEEPS[family] = (first seed, chunks, cases per chunk); chunk k draws from np.random.Generator(np.random.
Philox(first seed + k)).  A size comes either from a small random range or from a short list of boundary values built from the
kernels' own constants -- one below, at and one above a tile, chunk or slice size -- which are read from the sources (constant())
or asked of the library's host queries (F.conv1x1_k_slices, F.group_norm_chunk); no such number is written down here.  A case's id
names the family, the sweep seed, the index and the whole geometry, the seed of its data included: inputs(case) of a Case built by
hand from an id is the failing input.

Families (the reference of each in parentheses):
  dw5x5      depthwise 5x5 through F.conv_norm_act, stride 1 / 2 and dilation 2 (oracle.ref.conv2d_affine_act, _lraspp_ref.dw_dilated)
  pw_scaled  pointwise conv with input_scale= (the oracle on _mobilenetv3_ref.se_scale(x, gate), in the stated K-slice order)
  se         F.global_avg_pool, F.linear_act, F.se_scale, F.squeeze_excitation_gate (_mobilenetv3_ref)
  conv2d     F.conv2d_affine_act, both forms of CONV2D_SMALL_LAUNCH_WORKSPACE (_resnet_ref.oracle_conv)
  maxpool    F.max_pool2d, floor and ceil mode (torch's CPU max_pool2d)
  convt      F.conv_transpose2d_bias_act, kernel 2 and kernel 4 (_mask_ref.oracle_conv_transpose, _keypoint_ref.oracle_conv_transpose4)
  groupnorm  F.group_norm_act (_fcos_ref.group_norm)
  l2norm     F.l2_normalize_scale (_ssd_ref.l2_normalize_scale)
  lateral    F.conv1x1_upsample_add (_fpn_ref.oracle_lateral)
  interp     F.interpolate (_interp_ref.interpolate)
  argmax     F.interpolate_argmax, int64 and uint8 labels (_segmentation_ref.interpolate_argmax)
  gated_up   F.conv1x1_gated_upsample (_lraspp_ref.gated_upsample)
  roi        ops.roi_align, roi_pool, ps_roi_pool, ps_roi_align (_detect_ref.roi_align_ref, _roipool_ref)
  nms        ops.nms, ops.batched_nms (_detect_ref.nms_ref)
  paste      F.paste_masks_in_image (_mask_ref.paste)
  keypoints  F.heatmaps_to_keypoints (_keypoint_ref.keypoints)

The top-k, score and decode kernels of RPN / RetinaNet / FCOS / SSD / RoIHeads have sweeps of their own, on the tie-stable references
of their test files: tests/_fuzz_detect_cases.py.  Out of scope: the box-IoU family, and the pointwise image ops -- colour, crop, mix,
autoaugment -- whose guard-band suites already run the ragged widths.
"""
import functools
import itertools
import re
from dataclasses import dataclass

import numpy as np
import torch

from tests._boxes_ref import CSRC
from tests._segmentation_ref import SLICE_CHANNELS  # the channel slices of the convs over many input channels
from tests._util import philox_f32

F32 = np.float32
AFFINE = {None: 0, "mul_add": 1, "fma": 2}
ACTS = (None, "relu", "relu6", "hardswish")  # the exact activations of the conv epilogue
# bias x affine x residual x activation: 48 classes, dealt round-robin over a family's cases
EPILOGUES = tuple(itertools.product((False, True), (None, "mul_add", "fma"), (False, True), ACTS))

# family: (first sweep seed, chunks, cases per chunk)
SWEEPS = {
    "dw5x5": (1100, 4, 24), "pw_scaled": (1200, 4, 24), "se": (1300, 3, 16), "conv2d": (1400, 4, 24), "maxpool": (1500, 2, 25),
    "convt": (1600, 3, 16), "groupnorm": (1700, 3, 16), "l2norm": (1800, 2, 16), "lateral": (1900, 4, 24), "interp": (2000, 3, 16),
    "argmax": (2100, 3, 16), "gated_up": (2200, 3, 16), "roi": (2300, 4, 12), "nms": (2400, 4, 15), "paste": (2500, 2, 12),
    "keypoints": (2600, 2, 10),
}


# ---- the kernels' constants ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _constants(source):
    """{name: value} of every `constexpr int a = <expr>[, b = <expr>];` of a kernel source whose expression is integers, + - * / ( ),
    << and names defined earlier (in the same file or in mv_common.h)."""
    known = dict(_constants("mv_common.h")) if source != "mv_common.h" else {}
    for decl in re.findall(r"constexpr int ([^;]+);", (CSRC / source).read_text()):
        for part in decl.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*([\w\s+\-*/()<]+?)\s*", part)
            if not m:
                continue
            try:
                known[m.group(1)] = int(eval(m.group(2).replace("/", "//"), {"__builtins__": {}}, dict(known)))  # noqa: S307
            except Exception:  # an expression over something that is no integer constant
                continue
    return known


def constant(name, source="mv_common.h"):
    """The value of a `constexpr int` of a kernel source (tests/_boxes_ref.kernel_constant, with the expressions over other constants)."""
    found = _constants(source)
    assert name in found, f"{name} not found in {source}"
    return found[name]


@functools.lru_cache(maxsize=None)
def pointwise_cout_steps():
    """The output channel counts up to which the pointwise kernel's workgroup has one and two 32-channel wave tiles, from the plan in
    convnorm.hip (`p.mw = cout <= A ? 1 : (cout <= B ? 2 : 4)`)."""
    found = re.search(r"p\.mw = cout <= (\d+) \? 1 : \(cout <= (\d+) \? 2 : 4\)", (CSRC / "convnorm.hip").read_text())
    assert found, "the pointwise plan's channel-tile rule was not found in convnorm.hip"
    return int(found.group(1)), int(found.group(2))


def around(*values, lo=1, hi=None):
    """One below, at and one above every value, inside [lo, hi], ascending and without repeats."""
    out = sorted({v + d for v in values for d in (-1, 0, 1)})
    return [v for v in out if v >= lo and (hi is None or v <= hi)]


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    family: str
    sweep: int   # the seed of the chunk's generator
    index: int   # position in the chunk
    geom: tuple  # ((name, value), ...): the geometry, the call's keyword arguments and the seed of the data

    @property
    def g(self):
        return dict(self.geom)

    @property
    def id(self):
        return f"{self.family}[sweep {self.sweep} #{self.index}] " + " ".join(f"{k}={v}" for k, v in self.geom)

    def __repr__(self):
        return self.id


def rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def _mix(g, lo, hi, edges, turn=None):
    """An integer in [lo, hi]: half of the time from the boundary values, else uniform.  turn: an even turn takes the boundary values
    in order instead (value turn / 2 of the list), so that a family of twice as many cases as values meets each of them."""
    edges = [e for e in edges if lo <= e <= hi]
    if turn is not None and turn % 2 == 0:
        return int(edges[turn // 2 % len(edges)])
    if edges and g.random() < 0.5:
        return int(edges[int(g.integers(0, len(edges)))])
    return int(g.integers(lo, hi + 1))


def _pick(g, seq):
    return seq[int(g.integers(0, len(seq)))]


def factor(length):
    """(h, w) with h * w == length, h the largest divisor not above the square root."""
    for d in range(int(length ** 0.5), 0, -1):
        if length % d == 0:
            return d, length // d


def _epilogue(gi):
    bias, affine, res, act = EPILOGUES[gi % len(EPILOGUES)]
    return [("bias", bias), ("affine", affine), ("res", res), ("act", act)]


def _make(family, chunk, build):
    """The cases of one chunk: build(g, i, gi) -> a list of (name, value) pairs, gi the index in the whole family."""
    first, chunks, count = SWEEPS[family]
    assert 0 <= chunk < chunks
    g = rng(first + chunk)
    out = []
    for i in range(count):
        geom = build(g, i, chunk * count + i)
        out.append(Case(family, first + chunk, i, tuple(geom) + (("seed", 100000 * (first + chunk) + 100 * i),)))
    return out


def chunks(family):
    return range(SWEEPS[family][1])


def cases(family, chunk=None):
    if chunk is None:
        return [c for k in chunks(family) for c in cases(family, k)]
    return GENERATORS[family](chunk)


# ---- 1. depthwise 5x5 ------------------------------------------------------------------------------------------------------------------
DW_MODES = ((1, 1), (2, 1), (1, 2))  # (stride, dilation)


def dw5x5_plan(n, c, h, w, stride, dilation):
    """(rows of a strip, threads) of launch_dwpc5x5, restated from dw5x5.hip with its two constants."""
    rows, short = constant("kDw5Rows"), constant("kDw5ShortLaunch")
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    strips = lambda r: dilation * -(-oh // (dilation * r))  # noqa: E731
    if n * c * strips(rows) * -(-ow // 4) < short:
        rows //= 2
    return rows, n * c * strips(rows) * -(-ow // 4)


def _dw5x5(chunk):
    rows, short = constant("kDw5Rows"), constant("kDw5ShortLaunch")

    def build(g, i, gi):
        stride, dil = DW_MODES[gi % 3]
        last = SWEEPS["dw5x5"][2] - 1
        if i == last or (chunk == 3 and i == last - 1):
            # the chunk's last case is a launch exactly at the short-launch threshold: two strips of the full length, 32 quads a row,
            # and as many planes as make `short` threads.  Chunk 3 has, in front of it, the same launch with one plane fewer: the
            # largest that still takes the half strip
            stride, dil = DW_MODES[chunk % 3]
            n, ow, oh = 2, 128 // stride, (2 * rows if stride == 1 else 3)
            strips = dil * -(-oh // (dil * rows))
            c = short // (n * strips * (ow // 4)) - (0 if i == last else 1)
            h, w = (oh, ow) if stride == 1 else (2 * oh - 1, 2 * ow - 1)
        else:
            n, c = int(g.integers(1, 4)), _mix(g, 1, 70, [1, 2, 70] + around(constant("kWave"), hi=70))
            blocks = [rows // 2 * dil, rows * dil]  # output rows of a row block under the short and the full strip
            oh = _mix(g, 1, 40 // stride, [1] + [k * b + 1 for b in blocks for k in (1, 2)] + around(*blocks))
            ow = int(g.integers(0, 10)) * 4 + (gi // 3) % 4  # every residue of ow mod 4
            ow = min(max(ow, 1), 40 // stride)
            h = oh if stride == 1 else 2 * oh - int(g.integers(0, 2))
            w = ow if stride == 1 else 2 * ow - int(g.integers(0, 2))
            h, w = max(h, 1), max(w, 1)
        return [("n", n), ("c", c), ("h", h), ("w", w), ("stride", stride), ("dilation", dil)] + _epilogue(gi // 3 + 16 * (gi % 3))
    return _make("dw5x5", chunk, build)


def _epilogue_inputs(seed, cout, out_shape, g):
    bias = philox_f32(seed + 2, (cout,)) - F32(0.5) if g["bias"] else None
    alpha = philox_f32(seed + 3, (cout,)) + F32(0.5) if g["affine"] else None
    beta = philox_f32(seed + 4, (cout,)) - F32(0.5) if g["affine"] else None
    res = philox_f32(seed + 5, out_shape) * 2 - 1 if g["res"] else None
    return dict(bias=bias, alpha=alpha, beta=beta, res=res)


def _dw5x5_inputs(case):
    g = case.g
    n, c, h, w, s = g["n"], g["c"], g["h"], g["w"], g["stride"]
    d = dict(x=philox_f32(g["seed"], (n, c, h, w)) * 4 - 2, w=(philox_f32(g["seed"] + 1, (c, 1, 5, 5)) - F32(0.5)) * F32(0.8))
    d.update(_epilogue_inputs(g["seed"], c, (n, c, (h - 1) // s + 1, (w - 1) // s + 1), g))
    return d


def _dw5x5_reference(case, d):
    from oracle import ref
    from tests import _lraspp_ref as LR
    g = case.g
    code = AFFINE[g["affine"]]
    if g["dilation"] == 2:
        return LR.dw_dilated(d["x"], d["w"], d["bias"], d["alpha"], d["beta"], d["res"], code, g["act"])
    return ref.conv2d_affine_act(d["x"], d["w"], d["bias"], d["alpha"], d["beta"], d["res"], g["stride"], 2, g["c"], code, g["act"])


# ---- 2. pointwise conv with input_scale -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv1x1_slice_steps(n=1, h=3, w=3, cout=8, upto=400):
    """The input channel counts at which F.conv1x1_k_slices changes its slice count for a small launch: [(cin, slices), ...]."""
    from cpu_vision_amd import functional as F
    steps, last = [], None
    for cin in range(1, upto + 1):
        s = F.conv1x1_k_slices(n, cin, h, w, cout)[0]
        if s != last:
            steps.append((cin, s))
            last = s
    return steps


def _cin_edges(hi):
    chunk = constant("kPK", "convnorm.hip")
    return around(chunk, 2 * chunk, *[cin for cin, _ in conv1x1_slice_steps()[1:]], hi=hi) + [1, hi]


def _pw_scaled(chunk):
    def build(g, i, gi):
        n = int(g.integers(1, 4))
        cin, cout = _mix(g, 1, 200, _cin_edges(200)), _mix(g, 1, 200, around(*pointwise_cout_steps(), 2 * pointwise_cout_steps()[1], hi=200) + [1, 200])
        h, w = _mix(g, 1, 28, [1, 7, 28]), _mix(g, 1, 28, [1, 7, 28])
        return [("n", n), ("cin", cin), ("cout", cout), ("h", h), ("w", w)] + _epilogue(gi)
    return _make("pw_scaled", chunk, build)


def _gate(seed, n, c):
    """A squeeze-excitation gate in [0, 1) with exact zeros (every fifth entry, and the first)."""
    gate = philox_f32(seed, (n, c))
    gate.reshape(-1)[::5] = 0
    return gate


def _pw_scaled_inputs(case):
    g = case.g
    n, cin, cout, h, w = g["n"], g["cin"], g["cout"], g["h"], g["w"]
    d = dict(x=philox_f32(g["seed"], (n, cin, h, w)) * 4 - 2, w=(philox_f32(g["seed"] + 1, (cout, cin, 1, 1)) - F32(0.5)) * F32(0.8),
             gate=_gate(g["seed"] + 6, n, cin))
    d.update(_epilogue_inputs(g["seed"], cout, (n, cout, h, w), g))
    return d


def _pw_scaled_reference(case, d):
    from cpu_vision_amd import functional as F
    from oracle import ref
    from tests import _mobilenetv3_ref as MR
    g = case.g
    slices, sl = F.conv1x1_k_slices(g["n"], g["cin"], g["h"], g["w"], g["cout"])
    return ref.conv2d_affine_act(MR.se_scale(d["x"], d["gate"]), d["w"], d["bias"], d["alpha"], d["beta"], d["res"], 1, 0, 1,
                                 AFFINE[g["affine"]], g["act"], slice_len=sl if slices > 1 else 0)


# ---- 3. squeeze-excitation kernels ------------------------------------------------------------------------------------------------------
LIN_ACTS = (None, "relu", "hardswish", "hardsigmoid", "sigmoid")


def _se(chunk):
    wave = constant("kWave")

    def build(g, i, gi):
        n = int(g.integers(1, 4))
        c = _mix(g, 1, 100, [1, 2, 99, 100])
        length = _mix(g, 1, 33 * 33, [1, 2, 3, 33 * 33] + around(wave, 4 * wave, 8 * wave), turn=gi)
        h, w = factor(length)
        k, m = _mix(g, 1, 1100, [1, 1100] + around(wave, 2 * wave, 16 * wave), turn=gi + 1), _mix(g, 1, 130, [1, 130] + around(wave, 2 * wave))
        return [("n", n), ("c", c), ("h", h), ("w", w), ("rows", int(g.integers(1, 6))), ("k", k), ("m", m),
                ("act", LIN_ACTS[gi % 5]), ("lin_bias", bool(gi // 5 % 2)), ("squeeze", _mix(g, 1, 32, [1, 8, 32])),
                ("gate_act", ("relu", "hardswish")[gi % 2]), ("scale_act", ("sigmoid", "hardsigmoid")[gi // 2 % 2])]
    return _make("se", chunk, build)


def _se_inputs(case):
    g = case.g
    n, c, h, w, k, m, sq, s = g["n"], g["c"], g["h"], g["w"], g["k"], g["m"], g["squeeze"], g["seed"]
    return dict(x=philox_f32(s, (n, c, h, w)) * 4 - F32(1.5), gate=_gate(s + 1, n, c),
                xl=philox_f32(s + 2, (g["rows"], k)) * 2 - 1, wl=(philox_f32(s + 3, (m, k)) - F32(0.5)) * F32(0.6),
                bl=philox_f32(s + 4, (m,)) - F32(0.5) if g["lin_bias"] else None,
                w1=(philox_f32(s + 5, (sq, c)) - F32(0.5)) * F32(0.8), b1=philox_f32(s + 6, (sq,)) - F32(0.5),
                w2=(philox_f32(s + 7, (c, sq)) - F32(0.5)) * F32(2), b2=philox_f32(s + 8, (c,)) - F32(0.5))


def _se_reference(case, d):
    from tests import _mobilenetv3_ref as MR
    g = case.g
    return dict(pool=MR.global_avg_pool(d["x"]), scale=MR.se_scale(d["x"], d["gate"]),
                linear=MR.linear_act(d["xl"], d["wl"], d["bl"], g["act"]),
                gate=MR.squeeze_excitation_gate(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], g["gate_act"], g["scale_act"]))


# ---- 4. conv2d_affine_act --------------------------------------------------------------------------------------------------------------


def conv_out(size, k, stride, padding, dilation):
    return (size + 2 * padding - (dilation * (k - 1) + 1)) // stride + 1


def _conv2d(chunk):
    kchunk = constant("kIgK", "conv_igemm.hip")

    def build(g, i, gi):
        while True:
            kh, kw = int(g.integers(1, 8)), int(g.integers(1, 8))
            stride, padding, dilation = int(g.integers(1, 3)), int(g.integers(0, 4)), int(g.integers(1, 4))
            kind = gi % 3  # groups 1, 2, cin
            if kind == 0:
                cin = _mix(g, 1, 300, around(kchunk, SLICE_CHANNELS, 2 * SLICE_CHANNELS, hi=300) + [1, 300])
                groups, cout = 1, _mix(g, 1, 40, [1, 40] + around(kchunk, hi=40))
            elif kind == 1:
                cin, groups = 2 * _mix(g, 1, 150, around(kchunk, SLICE_CHANNELS, hi=150) + [1, 150]), 2
                cout = 2 * int(g.integers(1, 21))
            else:
                cin = _mix(g, 1, 300, around(2 * SLICE_CHANNELS, hi=300) + [1, 2, 300])
                groups, cout = cin, cin * int(g.integers(1, 3))
            n, h, w = int(g.integers(1, 3)), int(g.integers(1, 15)), int(g.integers(1, 15))
            oh, ow = conv_out(h, kh, stride, padding, dilation), conv_out(w, kw, stride, padding, dilation)
            if oh < 1 or ow < 1:
                continue
            # the reference runs the zero-stuffed kernel: keep its multiply-adds below 3e7 (a fraction of a second)
            taps = (dilation * (kh - 1) + 1) * (dilation * (kw - 1) + 1)
            if n * cout * oh * ow * (cin // groups) * taps > 3e7:
                continue
            break
        return [("n", n), ("cin", cin), ("h", h), ("w", w), ("cout", cout), ("kh", kh), ("kw", kw), ("stride", stride), ("padding", padding),
                ("dilation", dilation), ("groups", groups), ("columns", bool(gi // 3 % 2))] + _epilogue(gi // 6 + 8 * (gi % 6))
    return _make("conv2d", chunk, build)


def _conv2d_inputs(case):
    g = case.g
    n, cin, cout, s = g["n"], g["cin"], g["cout"], g["seed"]
    oh, ow = (conv_out(g[a], g[k], g["stride"], g["padding"], g["dilation"]) for a, k in (("h", "kh"), ("w", "kw")))
    d = dict(x=philox_f32(s, (n, cin, g["h"], g["w"])) * 2 - 1, w=(philox_f32(s + 1, (cout, cin // g["groups"], g["kh"], g["kw"])) - F32(0.5)) * F32(0.5))
    d.update(_epilogue_inputs(s, cout, (n, cout, oh, ow), g))
    return d


def _conv2d_reference(case, d):
    from tests import _resnet_ref as RR
    g = case.g
    return RR.oracle_conv(d["x"], d["w"], d["bias"], d["alpha"], d["beta"], d["res"], g["stride"], g["padding"], g["dilation"], g["groups"],
                          AFFINE[g["affine"]], g["act"])


# ---- 5. max_pool2d -----------------------------------------------------------------------------------------------------------------------
def pool_is_valid(h, w, k, stride, padding, ceil_mode):
    """What F.max_pool2d accepts (cpu_vision_amd/_layers.py)."""
    if padding > k // 2 or h + 2 * padding < k or w + 2 * padding < k:
        return False
    return ceil_mode or padding > 0 or (k <= h and k <= w)


def _maxpool(chunk):
    def build(g, i, gi):
        while True:
            k, stride, padding, ceil_mode = int(g.integers(2, 4)), int(g.integers(1, 4)), int(g.integers(0, 2)), bool(gi % 2)
            h, w = _mix(g, 1, 40, [1, 2, 3, 4, 39, 40]), _mix(g, 1, 40, [1, 2, 3, 4, 5, 39, 40])
            if i == 0:
                h, w, padding = 1, 1, 1  # every chunk begins with a 1 x 1 map (it needs the padding), floor mode in one, ceil in the other
            if pool_is_valid(h, w, k, stride, padding, ceil_mode):
                break
        return [("n", int(g.integers(1, 3))), ("c", int(g.integers(1, 6))), ("h", h), ("w", w), ("k", k), ("stride", stride), ("padding", padding),
                ("ceil_mode", ceil_mode)]
    return _make("maxpool", chunk, build)


def _maxpool_inputs(case):
    g = case.g
    x = philox_f32(g["seed"], (g["n"], g["c"], g["h"], g["w"])) * 4 - 2
    flat = x.reshape(-1)
    flat[::7] = -np.abs(flat[::7]) - F32(1)  # windows whose maximum is negative: a padding of 0 would win
    return dict(x=x)


def _maxpool_reference(case, d):
    g = case.g
    return torch.nn.functional.max_pool2d(torch.from_numpy(d["x"]), g["k"], g["stride"], g["padding"], ceil_mode=g["ceil_mode"]).numpy()


# ---- 6. conv_transpose2d_bias_act -------------------------------------------------------------------------------------------------------
CT_ACTS = (None, "relu", "relu6")


def _convt(chunk):
    def build(g, i, gi):
        while True:
            k = (2, 4)[gi % 2]
            cin, cout = _mix(g, 1, 300, _cin_edges(300)), _mix(g, 1, 40, [1, 40] + around(pointwise_cout_steps()[0] // 4))
            n, h, w = int(g.integers(1, 4)), _mix(g, 1, 15, [1, 2, 15]), _mix(g, 1, 15, [1, 2, 15])
            if n * cin * cout * 16 * (h + 1) * (w + 1) <= 3e7:
                break
        return [("n", n), ("cin", cin), ("h", h), ("w", w), ("cout", cout), ("k", k), ("bias", bool(gi // 2 % 2)), ("act", CT_ACTS[gi // 4 % 3])]
    return _make("convt", chunk, build)


def _convt_inputs(case):
    g = case.g
    cin, cout, k, s = g["cin"], g["cout"], g["k"], g["seed"]
    return dict(x=philox_f32(s, (g["n"], cin, g["h"], g["w"])) * 2 - 1,
                w=(philox_f32(s + 1, (cin, cout, k, k)) * 2 - 1) * F32(2.0 / np.sqrt(cin)),
                bias=philox_f32(s + 2, (cout,)) * 2 - 1 if g["bias"] else None)


def _convt_reference(case, d):
    from tests import _keypoint_ref as KR
    from tests import _mask_ref as M
    oracle = M.oracle_conv_transpose if case.g["k"] == 2 else KR.oracle_conv_transpose4
    return oracle(d["x"], d["w"], d["bias"], case.g["act"])


# ---- 7. group_norm_act -------------------------------------------------------------------------------------------------------------------
def _groupnorm(chunk):
    from cpu_vision_amd import functional as F
    wave, group, slab_chunk = constant("kWave"), constant("kGnThreads", "groupnorm.hip"), F.group_norm_chunk()
    edges = around(wave, group, slab_chunk, 2 * slab_chunk) + [1, 2, 3, wave // 2, 2 * slab_chunk + 4]

    def build(g, i, gi):
        m = _mix(g, 1, 2 * slab_chunk + 8, edges, turn=gi)  # the slab of one (image, group)
        per_group = _pick(g, [d for d in range(1, 17) if m % d == 0])
        h, w = factor(m // per_group)
        groups = int(g.integers(1, 9)) if m <= 1024 else int(g.integers(1, 3))
        return [("n", int(g.integers(1, 3))), ("c", per_group * groups), ("h", h), ("w", w), ("groups", groups), ("weight", bool(gi % 2)),
                ("gn_bias", bool(gi // 2 % 2)), ("relu", bool(gi // 4 % 2)), ("eps", (1e-5, 1e-3)[gi // 8 % 2])]
    return _make("groupnorm", chunk, build)


def _groupnorm_inputs(case):
    g = case.g
    c, s = g["c"], g["seed"]
    return dict(x=philox_f32(s, (g["n"], c, g["h"], g["w"])) * 6 - F32(2.4),
                weight=philox_f32(s + 1, (c,)) * 2 - F32(0.5) if g["weight"] else None, bias=philox_f32(s + 2, (c,)) * 2 - 1 if g["gn_bias"] else None)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _groupnorm_reference(case, d):
    from tests import _fcos_ref as FR
    g = case.g
    return FR.group_norm(_t(d["x"]), g["groups"], _t(d["weight"]), _t(d["bias"]), g["eps"], g["relu"]).numpy()


# ---- 8. l2_normalize_scale ---------------------------------------------------------------------------------------------------------------
def _l2norm(chunk):
    pixels, groups = constant("kL2Pixels"), constant("kL2Groups")

    def build(g, i, gi):
        c = _mix(g, 1, 600, around(groups, 2 * groups, 32 * groups) + [1, 599, 600], turn=gi)
        h, w = int(g.integers(1, 41)), int(g.integers(1, 41))
        if gi % 2:
            h, w = factor(_mix(g, 1, 1600, around(pixels, 2 * pixels) + [1, 1600], turn=gi + 1))
        n = int(g.integers(1, 3))
        while n * c * h * w > 500000:  # 2 MB
            h = (h + 1) // 2
        return [("n", n), ("c", c), ("h", h), ("w", w), ("zero_pixel", bool(gi % 3 == 0)), ("eps", 1e-12)]
    return _make("l2norm", chunk, build)


def _l2norm_inputs(case):
    g = case.g
    x = philox_f32(g["seed"], (g["n"], g["c"], g["h"], g["w"])) * 6 - 3
    if g["zero_pixel"]:
        x[g["n"] - 1, :, g["h"] // 2, g["w"] - 1] = 0
    return dict(x=x, weight=philox_f32(g["seed"] + 1, (g["c"],)) * 2 + 19)


def _l2norm_reference(case, d):
    from tests import _ssd_ref as SR
    return SR.l2_normalize_scale(_t(d["x"]), _t(d["weight"]), case.g["eps"]).numpy()


# ---- 9. conv1x1_upsample_add -------------------------------------------------------------------------------------------------------------
def _lateral(chunk):
    kchunk = constant("kPK", "convnorm.hip")

    def build(g, i, gi):
        n, cin, cout = int(g.integers(1, 3)), _mix(g, 1, 70, around(kchunk, 2 * kchunk, hi=70) + [1]), _mix(g, 1, 70, around(*pointwise_cout_steps(), hi=70) + [1])
        h, w = _mix(g, 1, 25, [1, 2, 25]), _mix(g, 1, 25, [1, 2, 25])
        # a top map of any size: smaller (FPN's direction; the odd sizes repeat the nearest index unevenly), equal, larger
        th, tw = _mix(g, 1, 2 * h + 1, [1, h // 2, (h + 1) // 2, h, h + 1, 2 * h + 1]), _mix(g, 1, 2 * w + 1, [1, w // 2, (w + 1) // 2, w, w + 3])
        ep = [p for p in _epilogue(gi) if p[0] != "res"]
        return [("n", n), ("cin", cin), ("cout", cout), ("h", h), ("w", w), ("th", th), ("tw", tw)] + ep
    return _make("lateral", chunk, build)


def _lateral_inputs(case):
    g = case.g
    n, cin, cout, s = g["n"], g["cin"], g["cout"], g["seed"]
    d = dict(x=philox_f32(s, (n, cin, g["h"], g["w"])) * 2 - 1, w=(philox_f32(s + 1, (cout, cin, 1, 1)) - F32(0.5)) * F32(0.5),
             top=philox_f32(s + 6, (n, cout, g["th"], g["tw"])) * 2 - 1)
    d.update(_epilogue_inputs(s, cout, None, dict(g, res=False)))
    return d


def _lateral_reference(case, d):
    from tests import _fpn_ref as PF
    g = case.g
    return PF.oracle_lateral(d["x"], d["w"], d["bias"], d["alpha"], d["beta"], d["top"], AFFINE[g["affine"]], g["act"])


# ---- 10. interpolate, interpolate_argmax, conv1x1_gated_upsample -----------------------------------------------------------------------
def _sizes(g, gi, wide_every, source):
    """(h, w, oh, ow) in 1..48, some identities, and every `wide_every`-th case of the family an output row of about one, two or
    three column blocks, the widths taken in turn."""
    cols = constant("kColsPerBlock", source)
    h, w = _mix(g, 1, 48, [1, 2, 47, 48]), _mix(g, 1, 48, [1, 2, 47, 48])
    oh, ow = _mix(g, 1, 48, [1, 2, h, 2 * h, 48]), _mix(g, 1, 48, [1, 2, w, 2 * w, 48])
    if gi % wide_every == wide_every - 1:
        wide = [cols, 2 * cols + 1, 2 * cols, cols + 1, 2 * cols + 8, cols + 4, cols - 1, 2 * cols - 1]
        oh, ow = min(oh, 6), wide[gi // wide_every % len(wide)]
    return h, w, oh, ow


def _interp(chunk):
    def build(g, i, gi):
        h, w, oh, ow = _sizes(g, gi, 6, "interp.hip")
        return [("n", int(g.integers(1, 3))), ("c", int(g.integers(1, 6))), ("h", h), ("w", w), ("oh", oh), ("ow", ow)]
    return _make("interp", chunk, build)


def _interp_inputs(case):
    g = case.g
    return dict(x=philox_f32(g["seed"], (g["n"], g["c"], g["h"], g["w"])) * 4 - 2)


def _interp_reference(case, d):
    from tests import _interp_ref as IR
    return IR.interpolate(d["x"], case.g["oh"], case.g["ow"])


def _argmax(chunk):
    def build(g, i, gi):
        h, w, oh, ow = _sizes(g, gi, 6, "segment.hip")
        classes = _mix(g, 1, 40, [1, 2, 3, 21, 40])
        dup = int(g.integers(0, classes - 1)) if classes > 2 and gi % 2 else -1  # plane `classes - 1` a copy of plane `dup`
        return [("n", int(g.integers(1, 3))), ("classes", classes), ("h", h), ("w", w), ("oh", oh), ("ow", ow), ("dup", dup)]
    return _make("argmax", chunk, build)


def _argmax_inputs(case):
    g = case.g
    x = rng(g["seed"]).standard_normal((g["n"], g["classes"], g["h"], g["w"]), dtype=F32)
    if g["dup"] >= 0:
        x[:, g["classes"] - 1] = x[:, g["dup"]]
    return dict(x=x)


def _argmax_reference(case, d):
    from tests import _segmentation_ref as GR
    return GR.interpolate_argmax(d["x"], case.g["oh"], case.g["ow"])


def _gated_up(chunk):
    def build(g, i, gi):
        while True:
            h, w, oh, ow = (_mix(g, 1, 24, [1, 2, 24]) for _ in range(4))
            if gi % 5 == 4:
                oh, ow = h, w  # the identity
            if i == 0:
                h, w = 1, 1  # every chunk begins with a 1 x 1 source: all four taps clamp at both borders
            n, cin, cout = int(g.integers(1, 3)), _mix(g, 1, 200, _cin_edges(200)), _mix(g, 1, 40, [1, 21, 40] + around(pointwise_cout_steps()[0], hi=40))
            if n * cin * cout * oh * ow <= 2e7:
                break
        return [("n", n), ("cin", cin), ("h", h), ("w", w), ("oh", oh), ("ow", ow), ("cout", cout), ("bias", bool(gi % 2)), ("res", bool(gi // 2 % 2))]
    return _make("gated_up", chunk, build)


def _gated_up_inputs(case):
    g = case.g
    n, cin, cout, s = g["n"], g["cin"], g["cout"], g["seed"]
    return dict(x=philox_f32(s, (n, cin, g["h"], g["w"])) * 4 - 2, gate=_gate(s + 1, n, cin), w=(philox_f32(s + 2, (cout, cin, 1, 1)) - F32(0.5)) * F32(0.6),
                bias=philox_f32(s + 3, (cout,)) - F32(0.5) if g["bias"] else None,
                res=philox_f32(s + 4, (n, cout, g["oh"], g["ow"])) * 2 - 1 if g["res"] else None)


def _gated_up_reference(case, d):
    from tests import _lraspp_ref as LR
    return LR.gated_upsample(d["x"], d["gate"], d["w"], d["bias"], d["res"], case.g["oh"], case.g["ow"])


# ---- 11. the RoI operators ---------------------------------------------------------------------------------------------------------------
ROI_OPS = ("roi_align", "roi_pool", "ps_roi_pool", "ps_roi_align")
ROI_KINDS = ("inside", "left", "top", "right", "bottom", "outside", "zero_width", "zero_height", "inverted", "larger")
ROI_SCALES = (1.0, 0.5, 0.25, 0.3)


def roi_box(kind, g, h, w):
    """One box (x1, y1, x2, y2) of a kind in MAP coordinates of an (h, w) map, corners on a grid of 1 / 8 without the halves: the
    pools round a corner to the nearest integer, and at a half a non-dyadic spatial_scale would let float32 and float64 differ."""
    W, H = float(w), float(h)
    q = lambda v: (round(float(v) * 8) + (round(float(v) * 8) % 8 == 4)) / 8  # noqa: E731
    x1, y1 = q(g.random() * W * 0.6), q(g.random() * H * 0.6)
    x2, y2 = q(x1 + 0.25 + g.random() * (W - x1)), q(y1 + 0.25 + g.random() * (H - y1))
    x2, y2 = min(x2, W), min(y2, H)
    if kind == "left":
        x1 = 0.0
    elif kind == "top":
        y1 = 0.0
    elif kind == "right":
        x2 = W
    elif kind == "bottom":
        y2 = H
    elif kind == "outside":
        dx, dy = _pick(g, [(-W - 20, 0), (W + 20, 0), (0, -H - 20), (0, H + 20), (W + 9, H + 9)])
        x1, x2, y1, y2 = x1 + dx, x2 + dx, y1 + dy, y2 + dy
    elif kind == "zero_width":
        x2 = x1
    elif kind == "zero_height":
        y2 = y1
    elif kind == "inverted":
        x1, x2, y1, y2 = x2, x1, y2, y1
    elif kind == "larger":
        x1, y1, x2, y2 = -q(3 + g.random() * 5), -q(2 + g.random() * 5), W + q(3 + g.random() * 5), H + q(2 + g.random() * 5)
    else:
        assert kind == "inside", kind
    return x1, y1, x2, y2


def _roi(chunk):
    def build(g, i, gi):
        op = ROI_OPS[gi % 4]
        ph, pw = (_mix(g, 1, 7, [1, 7]), _mix(g, 1, 7, [1, 7]))
        h, w = _mix(g, 1, 40, [1, 2, 40]), _mix(g, 1, 40, [1, 2, 40])
        n, c = int(g.integers(1, 4)), int(g.integers(1, 5))
        if op.startswith("ps_"):
            c *= ph * pw
        j = gi // 4  # the case's turn among those of its operator: scale, ratio and aligned in every combination class
        geom = [("op", op), ("n", n), ("c", c), ("h", h), ("w", w), ("ph", ph), ("pw", pw), ("scale", ROI_SCALES[j % 4]),
                ("rois", 0 if j == 5 else 2 * len(ROI_KINDS))]  # turn 5 of every operator: the empty list
        if op in ("roi_align", "ps_roi_align"):
            geom.append(("ratio", (j // 4 + j) % 4))
        if op == "roi_align":
            geom.append(("aligned", bool(j // 2 % 2)))
        return geom
    return _make("roi", chunk, build)


def _roi_inputs(case):
    g = case.g
    r = rng(g["seed"] + 1)
    rows = []
    for j in range(g["rois"]):
        kind = ROI_KINDS[j % len(ROI_KINDS)]
        x1, y1, x2, y2 = roi_box(kind, r, g["h"], g["w"])
        batch = (0, g["n"] - 1)[j % 2] if j < 4 else int(r.integers(0, g["n"]))  # the first and the last image
        rows.append([batch] + [v / g["scale"] for v in (x1, y1, x2, y2)])
    return dict(x=philox_f32(g["seed"], (g["n"], g["c"], g["h"], g["w"])) * 4 - 2, rois=np.asarray(rows, F32).reshape(-1, 5))


def _roi_reference(case, d, dtype=F32):
    from tests import _detect_ref as DR
    from tests import _roipool_ref as RP
    g = case.g
    out = (g["ph"], g["pw"])
    if g["op"] == "roi_align":
        return DR.roi_align_ref(d["x"], d["rois"], out, g["scale"], g["ratio"], g["aligned"], dtype)
    if g["op"] == "roi_pool":
        return RP.roi_pool_ref(d["x"], d["rois"], out, g["scale"], dtype)
    if g["op"] == "ps_roi_pool":
        return RP.ps_roi_pool_ref(d["x"], d["rois"], out, g["scale"], dtype)
    return RP.ps_roi_align_ref(d["x"], d["rois"], out, g["scale"], g["ratio"], dtype)


# ---- 12. nms, batched_nms ----------------------------------------------------------------------------------------------------------------
NMS_KINDS = ("clustered", "identical", "disjoint", "ties", "degenerate")
NMS_THRESHOLDS = (0.0, 0.3, 0.5, 0.7, 1.0)


def nms_block_sizes():
    """The block sizes of detect.hip's three nms kernels: a mask tile, a rank workgroup, the keys a rank step stages."""
    return constant("kWave"), constant("kRankBlock", "detect.hip"), constant("kRankTile", "detect.hip")


def _nms(chunk):
    edges = [0, 1, 2] + around(*nms_block_sizes(), *[2 * b for b in nms_block_sizes()[:2]]) + [1500]

    def build(g, i, gi):
        n = _mix(g, 0, 1500, edges) if i % 3 else edges[(gi // 3) % len(edges)]
        return [("boxes", n), ("kind", NMS_KINDS[gi % 5]), ("thr", NMS_THRESHOLDS[gi // 5 % 5]), ("classes", 3 if gi % 4 == 1 else 0)]
    return _make("nms", chunk, build)


def _nms_inputs(case):
    """boxes and scores clear of the threshold by tests/_detect_ref.boxes_with_margin; a batched case (classes > 0) on a grid of
    1 / 4, where moving the boxes apart by class is exact in float32 (tests/test_gpu_detect.py)."""
    from tests import _detect_ref as DR
    g = case.g
    n, thr = g["boxes"], g["thr"]
    if not g["classes"]:
        boxes, scores, used = DR.boxes_with_margin(g["kind"], n, (thr,), seed=g["seed"])
        return dict(boxes=boxes, scores=scores, box_seed=used)
    for s in range(g["seed"], g["seed"] + 20):
        boxes, scores = DR.make_boxes(g["kind"], n, s)
        boxes = (np.round(boxes * 4) / 4).astype(F32)
        if DR.tie_margin_ok(boxes, thr):
            return dict(boxes=boxes, scores=scores, box_seed=s, idxs=rng(s).integers(0, g["classes"], n))
    raise AssertionError(f"{case.id}: no seed gives boxes clear of the threshold")


def _nms_reference(case, d):
    from tests import _detect_ref as DR
    boxes, scores, thr = d["boxes"], d["scores"], case.g["thr"]
    if "idxs" not in d:
        return DR.nms_ref(boxes, scores, thr)
    idxs = d["idxs"]
    kept = [np.flatnonzero(idxs == c)[DR.nms_ref(boxes[idxs == c], scores[idxs == c], thr)] for c in range(case.g["classes"])]
    kept = np.concatenate(kept).astype(np.int64) if kept else np.zeros(0, np.int64)
    return kept[np.lexsort((kept, -scores[kept]))]


# ---- 13. paste_masks_in_image, heatmaps_to_keypoints -----------------------------------------------------------------------------------
BOX_KINDS = ("inside", "left", "top", "right", "bottom", "outside", "one_pixel", "larger")


def image_box(kind, g, h, w):
    """One box of a kind in the pixel coordinates of an (h, w) image."""
    W, H = float(w), float(h)
    x1, y1 = g.random() * W * 0.6, g.random() * H * 0.6
    x2, y2 = x1 + 1.5 + g.random() * (W - x1), y1 + 1.5 + g.random() * (H - y1)
    if kind == "left":
        x1 = -2.5 - g.random() * 5
    elif kind == "top":
        y1 = -2.5 - g.random() * 5
    elif kind == "right":
        x2 = W + 2.5 + g.random() * 5
    elif kind == "bottom":
        y2 = H + 2.5 + g.random() * 5
    elif kind == "outside":
        dx, dy = _pick(g, [(-2 * W - 40, 0), (2 * W + 40, 0), (0, -2 * H - 40), (0, 2 * H + 40)])
        x1, x2, y1, y2 = x1 + dx, x2 + dx, y1 + dy, y2 + dy
    elif kind == "one_pixel":
        x2, y2 = (x1 + 0.2, y2) if g.random() < 0.5 else (x1 + 0.2, y1 + 0.2)
    elif kind == "larger":
        x1, y1, x2, y2 = -3.0 - g.random() * 9, -3.0 - g.random() * 9, W + 3 + g.random() * 9, H + 3 + g.random() * 9
    else:
        assert kind == "inside", kind
    return x1, y1, x2, y2


def _image_boxes(seed, h, w, count):
    g = rng(seed)
    return np.asarray([image_box(BOX_KINDS[j % len(BOX_KINDS)], g, h, w) for j in range(count)], F32).reshape(-1, 4)


def _paste(chunk):
    cols, rows = constant("kPasteColsPerBlock", "mask.hip"), constant("kPasteRowsPerBlock", "mask.hip")

    def build(g, i, gi):
        h, w = _mix(g, 1, 70, [1, 2, 70] + around(rows, 2 * rows)), _mix(g, 1, 90, [1, 2, 3, 4, 88, 89, 90])
        if i == 0:
            w = cols + 1 + 4 * chunk  # one image a chunk with more than one column block
        return [("h", h), ("w", w), ("m", _pick(g, [1, 2, 7, 14, 28])), ("padding", gi % 2), ("rois", len(BOX_KINDS))]
    return _make("paste", chunk, build)


def _paste_inputs(case):
    from tests import _mask_ref as M
    g = case.g
    return dict(masks=M.paste_masks(g["seed"], g["rois"], g["m"]).numpy(), boxes=_image_boxes(g["seed"] + 1, g["h"], g["w"], g["rois"]))


def _paste_reference(case, d):
    from tests import _mask_ref as M
    g = case.g
    return M.paste(d["masks"], d["boxes"], g["h"], g["w"], g["padding"])


def _keypoints(chunk):
    def build(g, i, gi):
        # the heatmap is the image shrunk by 1, 2, 4 or 8 a side: the rois (one pixel wide .. larger than the image) then resize it by
        # factors from far below 1 to about 10, where the resized maximum still stands clear of its neighbours
        h, w, shrink = _mix(g, 1, 70, [1, 2, 70]), _mix(g, 1, 90, [1, 2, 90]), (1, 2, 4, 8)[gi % 4]
        return [("h", h), ("w", w), ("k", _pick(g, [1, 2, 3, 17])), ("mh", max(2, -(-h // shrink))), ("mw", max(2, -(-w // shrink))),
                ("rois", len(BOX_KINDS))]
    return _make("keypoints", chunk, build)


def _keypoints_inputs(case):
    """Heatmaps with a heavy tail, exp(6 u) / 20 of uniform u: wherever a resize samples the plane, its largest value leads the next
    by a margin far above the bicubic bound (which grows with max|x|), so the position of the maximum is decided."""
    g = case.g
    maps = (np.exp(6 * philox_f32(g["seed"], (g["rois"], g["k"], g["mh"], g["mw"])).astype(np.float64)) / 20).astype(F32)
    return dict(maps=maps, rois=_image_boxes(g["seed"] + 1, g["h"], g["w"], g["rois"]))


def _keypoints_reference(case, d):
    from tests import _keypoint_ref as KR
    return KR.keypoints(d["maps"], d["rois"])


GENERATORS = {"dw5x5": _dw5x5, "pw_scaled": _pw_scaled, "se": _se, "conv2d": _conv2d, "maxpool": _maxpool, "convt": _convt,
              "groupnorm": _groupnorm, "l2norm": _l2norm, "lateral": _lateral, "interp": _interp, "argmax": _argmax, "gated_up": _gated_up,
              "roi": _roi, "nms": _nms, "paste": _paste, "keypoints": _keypoints}
INPUTS = {"dw5x5": _dw5x5_inputs, "pw_scaled": _pw_scaled_inputs, "se": _se_inputs, "conv2d": _conv2d_inputs, "maxpool": _maxpool_inputs,
          "convt": _convt_inputs, "groupnorm": _groupnorm_inputs, "l2norm": _l2norm_inputs, "lateral": _lateral_inputs, "interp": _interp_inputs,
          "argmax": _argmax_inputs, "gated_up": _gated_up_inputs, "roi": _roi_inputs, "nms": _nms_inputs, "paste": _paste_inputs,
          "keypoints": _keypoints_inputs}
REFERENCES = {"dw5x5": _dw5x5_reference, "pw_scaled": _pw_scaled_reference, "se": _se_reference, "conv2d": _conv2d_reference,
              "maxpool": _maxpool_reference, "convt": _convt_reference, "groupnorm": _groupnorm_reference, "l2norm": _l2norm_reference,
              "lateral": _lateral_reference, "interp": _interp_reference, "argmax": _argmax_reference, "gated_up": _gated_up_reference,
              "roi": _roi_reference, "nms": _nms_reference, "paste": _paste_reference, "keypoints": _keypoints_reference}
assert set(GENERATORS) == set(INPUTS) == set(REFERENCES) == set(SWEEPS)


def inputs(case):
    """{name: numpy array or None} of a case, from its seed alone."""
    return INPUTS[case.family](case)


def reference(case, d):
    """The CPU reference of a case on inputs(case)."""
    return REFERENCES[case.family](case, d)


def nbytes(d):
    return sum(v.nbytes for v in d.values() if isinstance(v, np.ndarray))
