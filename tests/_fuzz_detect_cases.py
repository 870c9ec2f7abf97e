"""The cases of the random-shape sweeps of the top-k, score and decode kernels of RPN / RetinaNet / FCOS / SSD / RoIHeads
(tests/test_fuzz_detect_host.py, tests/test_gpu_fuzz_detect.py): one seeded generator per family, the inputs of a case and its CPU
reference.  numpy and CPU torch only; nothing here touches a device.  Case, rng, _mix, around, constant and factor are those of
tests/_fuzz_cases.py, and the rules are the same: SWEEPS[family] = (first seed, chunks, cases per chunk), chunk k draws from
Philox(first seed + k), every boundary value is read from the kernels' sources, and a case's id carries its whole geometry and the
seed of its data.

Families (entry -> reference, bit for bit; indices, labels and valid equal):
  rpn_topk     F.rpn_topk -> _rpn_ref.topk_stable per level on the keys' order (NaN greatest, -0 == +0), the level's start added
  rpn_decode   F.rpn_decode on the reference's own indices plus hand indices -> BoxCoder.decode_single, clip, sigmoid_cr, the filters
  ret_topk     F.retinanet_topk -> _retinanet_ref.select          fcos_topk    F.fcos_topk -> _fcos_ref.select
  ret_decode   F.retinanet_decode -> _retinanet_ref.decode        fcos_decode  F.fcos_decode -> _fcos_ref.decode
  ssd_scores   F.ssd_scores -> _ssd_ref.scores
  ssd_topk     F.ssd_topk on a score matrix of the case's own (no softmax in front) -> _ssd_ref.select
  ssd_decode   F.ssd_decode -> _ssd_ref.decode on _ssd_ref.default_boxes
  roi_det      F.roi_detections -> _roi_heads_ref.RoIHeads.dense, roi by roi (an image index outside the batch: zeros)
  box_decode   F.box_decode -> _rpn_ref.BoxCoder.decode_single under the restatement numerics

A pyramid has 1 .. kMaxRpnLevels levels (case gi has 1 + gi % kMaxRpnLevels: every count in every chunk), one `main` level whose
element count is drawn around the sizes the kernels step in and small ones (1 x 1 upwards) around it, in no order of size.  The
scored maps of a top-k family take one of six value kinds in turn (KINDS); a `sparse` case holds one failing value everywhere but at
a few dozen chosen places, its reference is closed form (no sort of the map), and the largest of them -- a level past 2^24
candidates, where select_keys' pass 4 first tells two keys apart -- is only ever materialised on the device (Sparse).  Two more
value kinds serve the families without a selection: `centred` (N(0, 2^2), the decodes' logits: scores on both sides of the rpn's
thresholds) and `wide` (N(0, 40^2), ssd_scores: exponentials that underflow to 0 and to denormals).  _deal gives a case its
threshold kind and, for "between", how many candidates pass relative to k.

select_exit restates the control flow of mv_topk.h's select_keys on the 64-bit keys of one workgroup's view; the sparse cases take
their k from it so that the sweep leaves select_keys early and after every pass 0 .. 7 (tests/test_fuzz_detect_host.py asserts it).
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from tests._fuzz_cases import Case, _mix, _pick, around, constant, factor, rng

F32 = np.float32
CLIP = math.log(1000.0 / 16)
KINDS = ("normal", "lattice", "all_equal", "cut_in_ties", "special", "sparse")
THRESHOLDS = ("negative", "below", "between", "exact", "above")
LAYOUTS = ("dense", "slice", "strided")
EXITS = ("early", 0, 1, 2, 3, 4, 5, 6, 7)  # how select_keys returns: at most k keys, or after pass p
LARGE = 1 << 20  # a sparse level above this many elements is never materialised on the CPU

# family: (first sweep seed, chunks, cases per chunk)
SWEEPS = {
    "rpn_topk": (2700, 4, 16), "rpn_decode": (2800, 2, 16), "ret_topk": (2900, 4, 18), "fcos_topk": (3000, 4, 18), "ret_decode": (3100, 2, 16),
    "fcos_decode": (3200, 2, 16), "ssd_scores": (3300, 2, 16), "ssd_topk": (3400, 4, 18), "ssd_decode": (3500, 2, 16), "roi_det": (3600, 3, 16),
    "box_decode": (3700, 2, 16),
}
PYRAMID_FAMILIES = ("rpn_topk", "rpn_decode", "ret_topk", "fcos_topk", "ret_decode", "fcos_decode", "ssd_scores", "ssd_decode")
THRESHOLD_FAMILIES = ("ret_topk", "fcos_topk", "ssd_topk")


@functools.lru_cache(maxsize=None)
def consts():
    """The kernels' sizes, each from its source."""
    c = dict(chunk=constant("kRetChunk"), max_k=constant("kRpnMaxK"), max_levels=constant("kMaxRpnLevels"), wave=constant("kWave"),
             roi_max_classes=constant("kRoiMaxClasses"), roi_waves=constant("kRoiWaves", "roi_heads.hip"),
             rpn_step=constant("kTopkThreads", "rpn.hip"), rpn_trip=constant("kTopkThreads", "rpn.hip") * constant("kTopkLoads", "rpn.hip"),
             rank_trip=constant("kRetThreads", "retinanet.hip") * constant("kRankLoads", "retinanet.hip"),
             ssd_step=constant("kSsdTopkThreads", "ssd.hip"), ssd_trip=constant("kSsdTopkThreads", "ssd.hip") * constant("kSsdTopkLoads", "ssd.hip"),
             scores_block=constant("kWave") * 4)  # k_ssd_scores and the decode kernels: 256 lanes a workgroup
    return c


def _make(family, chunk, build):
    """tests/_fuzz_cases._make over this module's SWEEPS."""
    first, chunks, count = SWEEPS[family]
    assert 0 <= chunk < chunks
    g = rng(first + chunk)
    out = []
    for i in range(count):
        seed = 100000 * (first + chunk) + 100 * i
        geom = build(g, i, chunk * count + i, seed)
        out.append(Case(family, first + chunk, i, tuple(geom) + (("seed", seed),)))
    return out


def chunks(family):
    return range(SWEEPS[family][1])


def cases(family, chunk=None):
    if chunk is None:
        return [c for k in chunks(family) for c in cases(family, k)]
    return GENERATORS[family](chunk)


# ---- keys and select_keys ---------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def score_keys(scores, flat, passing):
    """The 64-bit keys of retinanet.hip / ssd.hip: score bits << 32 | ~f for a passing candidate, else 0."""
    key = (bits(scores).astype(np.uint64) << np.uint64(32)) | (~np.asarray(flat, dtype=np.uint32)).astype(np.uint64)
    return np.where(passing, key, np.uint64(0))


def rpn_key(logits):
    """rpn.hip logit_key: the monotonic 32-bit image of a logit, -0 as +0, every NaN the one greatest key."""
    u = bits(logits)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    key = np.where(u == np.uint32(0x80000000), np.uint32(0x80000000), key)
    return np.where(np.isnan(logits), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def select_exit(keys, k):
    """mv_topk.h select_keys restated on the non-zero keys of one workgroup's view -> (exit, take): exit "early" when at most k keys
    pass, else the pass 0 .. 7 at which the bin of the k-th greatest key is taken whole."""
    keys = np.asarray(keys, dtype=np.uint64)
    keys = keys[keys != 0]
    if len(keys) <= k:
        return "early", len(keys)
    prefix, rem = 0, k
    for p in range(8):
        shift = 56 - 8 * p
        live = keys if p == 0 else keys[(keys >> np.uint64(shift + 8)) == np.uint64(prefix)]
        hist = np.bincount(((live >> np.uint64(shift)) & np.uint64(255)).astype(np.int64), minlength=256)
        above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])
        digit = int(np.flatnonzero((above < rem) & (above + hist >= rem))[0])
        prefix, rem, mine = (prefix << 8) | digit, rem - int(above[digit]), int(hist[digit])
        if mine == rem:
            return p, k
    raise AssertionError("the keys are not pairwise distinct")


def stage1_views(keys, mem, k):
    """The views of RetinaNet's two stages for one (image, level): keys and memory offsets of its passing candidates -> ([(exit, take)
    of every stage-1 chunk with a passing key], the pool stage 2 reads)."""
    chunk = np.asarray(mem) // consts()["chunk"]
    exits, pool = [], []
    for c in np.unique(chunk):
        mine = np.sort(keys[chunk == c])[::-1]
        exits.append(select_exit(mine, k))
        pool.append(mine[:k])
    return exits, (np.concatenate(pool) if pool else np.zeros(0, np.uint64))


# ---- pyramids -----------------------------------------------------------------------------------------------------------------------------
def _split(total, g, a_hi=12, k_range=(1, 91)):
    """(A, K, h, w) with A K h w == total, A in 1 .. a_hi, K in k_range, h != w where the count allows."""
    opts = [(a, k) for a in range(1, a_hi + 1) for k in range(k_range[0], k_range[1] + 1) if total % (a * k) == 0]
    assert opts, total
    a, k = _pick(g, opts)
    h, w = factor(total // (a * k))
    return (a, k, w, h) if g.random() < 0.5 else (a, k, h, w)


def _pyramid(g, gi, main, a_hi=4):
    """[(A, h, w), ...] and the position of the main level: 1 + gi % kMaxRpnLevels levels, the others small (1 x 1 upwards)."""
    count = 1 + gi % consts()["max_levels"]
    at = int(g.integers(0, count))
    levels = []
    for l in range(count):
        if l == at:
            levels.append(main)
        elif l == (at + 1) % count:
            levels.append((int(g.integers(1, a_hi + 1)), 1, 1))  # a 1 x 1 map in every pyramid of two levels or more
        else:
            levels.append((int(g.integers(1, a_hi + 1)), int(g.integers(1, 5)), int(g.integers(1, 6))))
    return tuple(levels), at


def _layout(gi):
    return "strided" if gi % 16 == 6 else "slice" if gi % 3 == 1 else "dense"


def place(m, layout, to=lambda t: t):
    """A (n, c, h, w) tensor as the entry sees it: itself, a channel slice of a wider tensor (the image stride is larger than the map;
    the rest is NaN) or every other column of a wider one (not dense: the entry copies it)."""
    m = to(m)
    if layout == "slice":
        wide = torch.cat([m, torch.full((m.shape[0], 2) + tuple(m.shape[2:]), float("nan"), dtype=m.dtype, device=m.device)], 1)
        return wide[:, :m.shape[1]]
    if layout == "strided":
        wide = torch.full(tuple(m.shape[:3]) + (2 * m.shape[3],), float("nan"), dtype=m.dtype, device=m.device)
        wide[..., ::2] = m
        return wide[..., ::2]
    assert layout == "dense", layout
    return m


@dataclass(frozen=True)
class Sparse:
    """A (n, c, h, w) map that is `fill` everywhere but at the memory offsets e of the images img, where it is val."""
    shape: tuple
    fill: float
    img: np.ndarray
    e: np.ndarray
    val: np.ndarray

    def numpy(self):
        n = self.shape[0]
        out = np.full((n, int(np.prod(self.shape[1:]))), self.fill, F32)
        out[self.img, self.e] = self.val
        return out.reshape(self.shape)

    def tensor(self, device="cpu"):
        n = self.shape[0]
        out = torch.full((n, int(np.prod(self.shape[1:]))), self.fill, dtype=torch.float32, device=device)
        out[torch.from_numpy(self.img).to(device), torch.from_numpy(self.e).to(device)] = torch.from_numpy(self.val).to(device)
        return out.reshape(self.shape)


def tensor_of(m, device="cpu"):
    return m.tensor(device) if isinstance(m, Sparse) else torch.from_numpy(np.ascontiguousarray(m)).to(device)


def flat_of_mem(e, hw, a_count, k_count, start):
    """Memory offset e (channel a K + c, position pos) of a level's map -> the flat index (start + pos A + a) K + c."""
    e = np.asarray(e, np.int64)
    ch, pos = e // hw, e % hw
    return ((start + pos * a_count + ch // k_count) * k_count + ch % k_count).astype(np.int64)


def mem_of_flat(f, hw, a_count, k_count, start):
    f = np.asarray(f, np.int64) - start * k_count
    v, c = f // k_count, f % k_count
    return ((v % a_count) * k_count + c) * hw + v // a_count


def level_starts(levels):
    return np.concatenate([[0], np.cumsum([a * h * w for a, h, w in levels])]).astype(np.int64)


# ---- the values of a scored map ---------------------------------------------------------------------------------------------------------
def _tied_run(n, count, k, boundary, gi):
    """cut_in_ties in the order the kernel scans (`count` elements): everything below -6.5, a run of -6.0 across `boundary` (or the
    middle), and k - j values above it in [-5.5, 0), j = 1, half the run, the whole run by image and case -> (values (n, count), the runs)."""
    r = rng(7000 + gi)
    x = -(r.random((n, count), dtype=F32) * F32(11.5) + F32(6.5))  # spread thin: neighbours in the order stay clear of float32's rounding
    b = boundary * max(1, min((count - 1) // boundary, 1 + gi % 2)) if count > boundary + 1 else count // 2
    runs = []
    for i in range(n):
        length = min(count, 3 + (gi + i) % 9)
        lo = max(0, min(b - 1 - (gi + i) % max(1, length - 1), count - length))
        take = (1, max(1, length // 2), length)[(gi // 2 + i) % 3]  # ties taken when the cut is at k
        above = min(max(k - take, 0), count - length)
        others = np.setdiff1d(np.arange(count), np.arange(lo, lo + length))
        x[i, r.choice(others, above, replace=False)] = -r.random(above, dtype=F32) * F32(5.5)
        x[i, lo:lo + length] = F32(-6)
        runs.append((lo, length))
    return x, runs


def _values(kind, seed, n, count, k, boundary, gi):
    """(n, count) float32 logits of a value kind, in the order the kernel scans."""
    r = rng(seed)
    if kind == "normal":  # a detector's logits: mostly far below 0, so that the greatest scores lie where the sigmoid is steep and
        return (r.standard_normal((n, count)) * 1.5 - 4).astype(F32)  # neighbours in the order differ by far more than a rounding
    if kind == "centred":
        return (r.standard_normal((n, count)) * 2).astype(F32)
    if kind == "lattice":
        return (r.integers(-64, 65, (n, count)) / 8).astype(F32)
    if kind == "all_equal":
        return np.full((n, count), (r.integers(-16, 17) / 8), F32)
    if kind == "cut_in_ties":
        return _tied_run(n, count, k, boundary, gi)[0]
    assert kind == "special", kind
    x = (r.standard_normal((n, count)) * 1.5 - 4).astype(F32)
    u = r.random((n, count))
    for lo, hi, v in ((0, .05, np.nan), (.05, .08, np.inf), (.08, .11, -np.inf), (.11, .15, 0.0), (.15, .19, -0.0)):
        x[(u >= lo) & (u < hi)] = v
    x[(u >= .19) & (u < .2)] = np.array([0xFFC00001], np.uint32).view(F32)[0]  # a NaN with the sign bit and a payload
    return x


def _sparse_picks(seed, n, lo, hi, want, boundary_of):
    """The chosen places of a sparse case in FLAT indices lo <= f < hi and their logits, the same in every image but for a shift of the
    values: for an exit in the index passes 4 .. 7 all logits are equal and the places sit on both sides of a multiple of 2^24, 2^16,
    2^8 (boundary_of(p)); else ~300 N(0, 1.5^2) logits, some of them 1e-5 apart (scores that share their top three bytes)."""
    r = rng(seed)
    if want in (4, 5, 6, 7):
        if want == 7:
            block = 256
            base = -(-lo // block) * block
            base = base if base + 40 <= hi else lo
            f = base + np.sort(r.choice(min(block, hi - base), min(24, hi - base), replace=False))
            below = len(f) // 2
        else:
            cut = boundary_of(want)
            span = min(cut - lo, hi - cut, 1 << 8 * (7 - want))
            assert span >= 2, (want, lo, hi, cut)
            f = np.concatenate([cut - 1 - np.sort(r.choice(span, min(12, span), replace=False))[::-1],
                                cut + np.sort(r.choice(span, min(12, span), replace=False))])
            below = int((f < cut).sum())
        return f.astype(np.int64), np.full(len(f), 0.75, F32), below
    m = min(300, hi - lo)
    f = lo + np.sort(r.choice(hi - lo, m, replace=False))
    v = (r.standard_normal(m) * 1.5).astype(F32)
    v[1:16:2] = v[0:15:2][:len(v[1:16:2])] + F32(1e-5)
    return f.astype(np.int64), v, None


def index_cut(want, lo, hi):
    """The smallest multiple of the block of index pass `want` (2^24, 2^16, 2^8) with room on both sides inside [lo, hi) that is no
    multiple of the next larger block (for want == 4 there is none larger below 2^31)."""
    block = 1 << 8 * (7 - want)
    cut = (lo // block + 1) * block
    if cut - lo < 16:
        cut += block
    if want > 4 and cut % (block << 8) == 0:
        cut += block
    assert lo < cut < hi, (want, lo, hi)
    return cut


# ---- 1. the one-stage top-k families: ret_topk, fcos_topk -----------------------------------------------------------------------------
def _k_by_level(k, count, kind, gi):
    """Every fourth case of the dense kinds: k one below, at and one above the level's element count, in turn."""
    if gi % 4 == 2 and kind not in ("sparse", "cut_in_ties") and count + 1 <= consts()["max_k"]:
        return max(1, count + (gi // 12) % 3 - 1)
    return k


def _k_edges(count=None):
    c = consts()
    edges = [1, 2] + around(c["wave"], 4 * c["wave"], c["rpn_step"], c["max_k"], hi=c["max_k"])
    return edges if count is None else edges + [v for v in (count - 1, count, count + 1) if 1 <= v <= c["max_k"]]


def _deal(kind, gi):
    """(threshold kind, rel) of case gi, j its turn among the cases of its value kind.  `normal` takes "between" in every second turn
    with rel = -1, 0, 1 in turn: the passing candidates of the main level of image 0 are then k + rel, on continuous scores.  A sparse
    case needs a threshold its fill fails; in a cut_in_ties case everything passes, so that the cut at k falls into the tied run."""
    j = gi // len(KINDS)
    if kind == "sparse":
        return ("between", "exact")[j % 2], 0
    if kind == "cut_in_ties":
        return ("negative", "below")[j % 2], 0
    if kind == "normal":
        return ("between", j // 2 % 3 - 1) if j % 2 else (THRESHOLDS[j // 2 % len(THRESHOLDS)], 0)
    return THRESHOLDS[(j + KINDS.index(kind)) % len(THRESHOLDS)], j % 3 - 1


def _onestage_topk(family):
    fcos = family == "fcos_topk"

    def generator(chunk):
        c = consts()
        per = SWEEPS[family][2]
        counts = [1, 2, 5, 37, 600] + around(c["chunk"], 2 * c["chunk"], 3 * c["chunk"])

        def build(g, i, gi, seed):
            kind = KINDS[gi % len(KINDS)]
            want = EXITS[(gi // len(KINDS)) % len(EXITS)] if kind == "sparse" else None
            count = _mix(g, 1, 3 * c["chunk"] + 1, counts, turn=gi)
            if kind == "normal":
                count = max(count, 5)
            if kind == "sparse" and want != "early":
                # stage 2 looks inside a bin only when several stage-1 chunks hand it more than k keys between them
                count = max(count, 2 * c["chunk"] + 600, 3 << 16 if want == 5 else 0)
            if want == 4:
                count = (1 << 24) + (5 << 10)  # the one level past 2^24 candidates
            thr, rel = _deal(kind, gi)
            if kind == "cut_in_ties":
                count = max(count, c["max_k"] + 16, c["chunk"] + 64 if gi // len(KINDS) % 2 == 0 else 0)  # room below any k; every second one: a run across two chunks
            if gi in (24, 48):
                count = 3 * c["chunk"] - gi  # three chunks that hand stage 2 up to kRpnMaxK keys each: several trips of its read loop
            a, k_cls, h, w = _split(count, g, a_hi=1 if fcos else 12)
            if want in (6, 7):
                # the chosen places are neighbours in the flat order: with two classes they alternate between two channel planes,
                # each longer than a chunk, so that two stage-1 workgroups see them
                a, k_cls, (h, w) = 1, 2, factor(c["chunk"] + 9 + gi % 5)
            levels, at = _pyramid(g, gi, (a, h, w), a_hi=1 if fcos else 4)
            if want == 4:
                levels, at = ((a, h, w),), 0  # alone: 64 MB of logits
            n = 1 if want == 4 else int(g.integers(1, 4))
            k = _k_by_level(_mix(g, 1, c["max_k"], _k_edges(count), turn=gi + 1), count, kind, gi)
            if kind == "normal" and thr == "between":
                k = max(2, min(k, count - 2))  # 1 <= k + rel < the level
            if gi in (24, 48):
                k, thr = c["max_k"] - gi % 7, ("below", "negative")[gi // 24 % 2]
            geom = [("n", n), ("levels", levels), ("main", at), ("classes", k_cls), ("k", k), ("kind", kind), ("thr", thr), ("layout", _layout(gi)),
                    ("rel", rel)]  # rel: the passing candidates of the main level of image 0 are k + rel (thr "between")
            if kind == "sparse":
                geom[4] = ("k", _sparse_k(family, dict(geom), seed, want))
                geom.append(("exit", want))
            return geom
        assert per >= 2 * len(KINDS)
        return _make(family, chunk, build)
    return generator


def _sparse_level(g, seed):
    """The chosen places of a sparse one-stage case: (flat indices, logits, how many lie below the cut or None, the level's geometry)."""
    a, h, w = g["levels"][g["main"]]
    kc, start = g["classes"], int(level_starts(g["levels"])[g["main"]])
    lo, hi = start * kc, (start + a * h * w) * kc
    f, v, below = _sparse_picks(seed + 1, g["n"], lo, hi, g.get("exit"), lambda p: index_cut(p, lo, hi))
    return f, v, below, (a, h, w, kc, start)


def _sparse_scores(family, v):
    """The float32 scores of the chosen logits (FCOS: with the centerness 0.5 everywhere)."""
    from tests import _fcos_ref as FR
    from tests._rpn_ref import sigmoid_cr
    t = torch.from_numpy(np.ascontiguousarray(v))
    s = FR.score(t, torch.full_like(t, 0.5)) if family.startswith("fcos") else sigmoid_cr(t)
    return s.numpy()


def _sparse_k(family, g, seed, want):
    """The k of a sparse case: the one at which stage 2 leaves select_keys as `want`, found with select_exit on the reference's keys."""
    g = dict(g, exit=want)
    f, v, below, (a, h, w, kc, start) = _sparse_level(g, seed)
    if below is not None:
        return below
    s = _sparse_scores(family, v)
    keys, mem = score_keys(s, f, np.ones(len(f), bool)), mem_of_flat(f, h * w, a, kc, start)
    if want == "early":
        return len(keys) + 3
    for k in range(1, len(keys)):
        if select_exit(stage1_views(keys, mem, k)[1], k)[0] == want:
            return k
    raise AssertionError(f"{family} seed {seed}: no k leaves stage 2's select_keys after pass {want}")


def _threshold(kind, scores, k, rel):
    """The float32 threshold of a kind for the scores (1-D, any order) of the main level of image 0."""
    s = np.sort(scores[~np.isnan(scores)])[::-1]
    if len(s) == 0:  # nothing but NaN
        return F32(-0.25) if kind in ("negative", "below") else F32(1)
    if kind == "negative":
        return F32(-0.25)
    if kind == "below":
        return F32(s[-1] / 2) if s[-1] > 0 else np.nextafter(F32(0), F32(-1))
    if kind == "above":
        return F32((np.float64(s[0]) + 1) / 2) if np.isfinite(s[0]) and s[0] < 1 else F32(1)
    j = min(max(k + rel, 1), len(s)) - 1  # s[j] is the last passing one
    if kind == "exact" or j + 1 >= len(s) or s[j + 1] == s[j]:
        return s[min(j + 1, len(s) - 1)]
    mid = F32((np.float64(s[j]) + np.float64(s[j + 1])) / 2)
    return mid if s[j + 1] <= mid < s[j] else s[j + 1]


def _sparse_threshold(kind, fill, scores):
    """A sparse case's threshold: exactly the fill's score, or between it and the smallest chosen one -- the fill fails either way."""
    assert fill < scores.min()
    return float(fill) if kind == "exact" else float(F32((np.float64(fill) + np.float64(scores.min())) / 2))


def _onestage_inputs(case):
    from tests import _fcos_ref as FR
    from tests._rpn_ref import sigmoid_cr
    g = case.g
    fcos = case.family.startswith("fcos")
    n, kc, seed = g["n"], g["classes"], g["seed"]
    maps, ctrs, sparse = [], [], None
    for l, (a, h, w) in enumerate(g["levels"]):
        count = a * kc * h * w
        ctrs.append((rng(seed + 50 + l).standard_normal((n, 1, h, w)) * 2).astype(F32) if fcos else None)
        if l != g["main"]:
            kind = g["kind"] if g["kind"] in ("normal", "lattice", "all_equal", "special") else "lattice"
            maps.append(_values(kind, seed + 10 + l, n, count, g["k"], consts()["chunk"], l).reshape(n, a * kc, h, w))
        elif g["kind"] == "sparse":
            f, v, _, _ = _sparse_level(g, seed)
            e = mem_of_flat(f, h * w, a, kc, int(level_starts(g["levels"])[l]))
            img = np.repeat(np.arange(n), len(f))
            m = Sparse((n, a * kc, h, w), -30.0, img, np.tile(e, n), np.tile(v, n))
            sparse = dict(flat=f, logits=v, scores=_sparse_scores(case.family, v))
            if fcos:
                ctrs[l] = Sparse((n, 1, h, w), 0.5, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, F32))
            maps.append(m if count > LARGE else m.numpy())
            if fcos and count <= LARGE:
                ctrs[l] = ctrs[l].numpy()
        else:
            x = _values(g["kind"], seed, n, count, g["k"], consts()["chunk"], case.index + case.sweep)
            if fcos and g["kind"] in ("all_equal", "cut_in_ties"):
                ctrs[l] = np.full((n, 1, h, w), 0.25, F32)  # FCOS's ties are whole (cls, ctr) pairs
            elif fcos and g["kind"] == "special":
                ctrs[l] = _values("special", seed + 70, n, h * w, 1, 1, l).reshape(n, 1, h, w)
            elif fcos and g["kind"] == "lattice":
                # continuous pairs; ties by copying whole positions (all class logits and the centerness) and, within a position, the
                # logits of the even classes to the odd ones
                xs, cs = (rng(seed).standard_normal((n, kc, h * w)) * 2).astype(F32), ctrs[l].reshape(n, h * w)
                src, dst = rng(seed + 2).integers(0, h * w, h * w // 4), rng(seed + 3).integers(0, h * w, h * w // 4)
                xs[:, :, dst], cs[:, dst] = xs[:, :, src], cs[:, src]
                xs[:, 1::2] = xs[:, 0:2 * (kc // 2):2]
                x = xs.reshape(n, count)
            maps.append(x.reshape(n, a * kc, h, w))
    d = dict(maps=maps, ctrs=ctrs if fcos else None, sparse=sparse)
    # the threshold: from the float32 scores of the main level of image 0
    if sparse is not None:
        d["thresh"] = _sparse_threshold(g["thr"], _sparse_scores(case.family, np.array([-30.0], F32))[0], sparse["scores"])
    else:
        m0 = torch.from_numpy(maps[g["main"]][:1])
        s = FR.level_scores(m0, torch.from_numpy(ctrs[g["main"]][:1]), kc) if fcos else sigmoid_cr(m0)
        d["thresh"] = float(_threshold(g["thr"], s.numpy().reshape(-1), g["k"], g["rel"]))
    return d


def level_flat_scores(family, d, g, l):
    """The float32 scores of level l in FLAT order (n, HWA K) -- the restatement's own arithmetic."""
    from tests import _fcos_ref as FR
    from tests import _retinanet_ref as RR
    m = torch.from_numpy(d["maps"][l])
    if family.startswith("fcos"):
        return FR.level_scores(m, torch.from_numpy(d["ctrs"][l]), g["classes"]).numpy()
    return RR.sigmoid_cr(RR.permute_level(m, g["classes"]).flatten(1)).numpy()


def sparse_select(case, d):
    """The closed form of a sparse case's selection: from the chosen places and their scores alone."""
    g = case.g
    thresh = F32(d["thresh"])
    f, s = d["sparse"]["flat"], d["sparse"]["scores"]
    keep = s > thresh
    order = np.lexsort((f[keep], -s[keep].astype(np.float64)))
    return f[keep][order][:g["k"]]


def _onestage_reference(case, d):
    from tests import _fcos_ref as FR
    from tests import _retinanet_ref as RR
    g = case.g
    fcos = case.family.startswith("fcos")
    kc, k = g["classes"], g["k"]
    if d["sparse"] is None:
        maps = [torch.from_numpy(m) for m in d["maps"]]
        if fcos:
            return FR.select(maps, [torch.from_numpy(c) for c in d["ctrs"]], kc, k, d["thresh"]).numpy()
        return RR.select(maps, kc, k, d["thresh"]).numpy()
    # sparse: the other levels by the restatement, the main level in closed form
    out, start = [], 0
    for l, (a, h, w) in enumerate(g["levels"]):
        seg = min(k, a * h * w * kc)
        if l == g["main"]:
            sel = sparse_select(case, d)
            row = np.full(seg, -1, np.int32)
            row[:len(sel)] = sel
            out.append(np.broadcast_to(row, (g["n"], seg)))
        else:
            m = [torch.from_numpy(d["maps"][l])]
            one = FR.select(m, [torch.from_numpy(d["ctrs"][l])], kc, k, d["thresh"]) if fcos else RR.select(m, kc, k, d["thresh"])
            one = one.numpy()
            out.append(np.where(one >= 0, one + start * kc, -1).astype(np.int32))
        start += a * h * w
    return np.ascontiguousarray(np.concatenate(out, 1))


# ---- 2. rpn_topk ------------------------------------------------------------------------------------------------------------------------
def _rpn_topk(chunk):
    c = consts()
    counts = [1, 2, 7, 70] + around(c["rpn_step"], c["rpn_trip"], 2 * c["rpn_trip"])

    def build(g, i, gi, seed):
        kind = KINDS[gi % len(KINDS)]
        count = _mix(g, 1, 2 * c["rpn_trip"] + 1000, counts, turn=gi)
        if kind == "cut_in_ties" and gi % 4 < 2:
            count = 2 * c["rpn_trip"] + 1000 - gi  # room for a run across the 4096-element trip and a take of a tile +- 1
        a, _, h, w = _split(count, g, k_range=(1, 1))
        levels, at = _pyramid(g, gi, (a, h, w))
        k = _k_by_level(_mix(g, 1, c["max_k"], _k_edges(count), turn=gi + 1), count, kind, gi)
        if kind == "cut_in_ties":
            k = min(count - 1, (c["rpn_step"] - 1, c["rpn_step"] + 1, c["rpn_step"], 300)[gi // 12 % 4]) or 1
        return [("n", int(g.integers(1, 4))), ("levels", levels), ("main", at), ("k", k), ("kind", kind), ("layout", _layout(gi))]
    return _make("rpn_topk", chunk, build)


def _rpn_boundary(case):
    c = consts()
    return c["rpn_trip"] if (case.index + case.sweep) % 2 else c["rpn_step"]


def _flat_to_map(flat, a, h, w):
    """(n, H W A) in the reference's flat order -> the head's (n, A, H, W) map."""
    return np.ascontiguousarray(flat.reshape(flat.shape[0], h, w, a).transpose(0, 3, 1, 2))


def _rpn_topk_inputs(case):
    g = case.g
    n, seed = g["n"], g["seed"]
    maps, sparse = [], None
    for l, (a, h, w) in enumerate(g["levels"]):
        count = a * h * w
        if l != g["main"]:
            kind = g["kind"] if g["kind"] in ("normal", "lattice", "all_equal", "special") else "lattice"
            flat = _values(kind, seed + 10 + l, n, count, g["k"], 1, l)
        elif g["kind"] == "sparse":
            f, v, _ = _sparse_picks(seed + 1, n, 0, count, None, None)
            flat = np.full((n, count), -30.0, F32)
            flat[:, f] = v
            sparse = dict(flat=f, logits=v)
        else:
            flat = _values(g["kind"], seed, n, count, g["k"], _rpn_boundary(case), case.index + case.sweep)
        maps.append(_flat_to_map(flat, a, h, w))
    return dict(maps=maps, sparse=sparse)


def rpn_flat(m):
    return np.ascontiguousarray(m.transpose(0, 2, 3, 1).reshape(m.shape[0], -1))


def _rpn_topk_reference(case, d):
    from tests import _rpn_ref as P
    g = case.g
    out, start = [], 0
    for l, m in enumerate(d["maps"]):
        flat = rpn_flat(m)
        take = min(g["k"], flat.shape[1])
        if l == g["main"] and d["sparse"] is not None:
            # closed form: the chosen logits above the fill in stable descending order, then the fill's places in ascending order
            f, v = d["sparse"]["flat"], d["sparse"]["logits"]
            up = v > F32(-30)
            head = f[up][np.lexsort((f[up], -v[up].astype(np.float64)))]
            rest = np.setdiff1d(np.arange(min(flat.shape[1], take + len(f))), f[up])
            one = np.concatenate([head, rest])[:take]
            out.append(np.broadcast_to(one + start, (g["n"], take)))
        else:
            out.append(P.topk_stable(torch.from_numpy(flat), take).numpy() + start)
        start += flat.shape[1]
    return np.ascontiguousarray(np.concatenate(out, 1).astype(np.int32))


# ---- 3. ssd_scores, ssd_topk -----------------------------------------------------------------------------------------------------------
def _ssd_scores(chunk):
    c = consts()
    totals = [1, 2, 9] + around(c["scores_block"], 2 * c["scores_block"], 3 * c["scores_block"])

    def build(g, i, gi, seed):
        count = 1 + gi % c["max_levels"]
        total = max(_mix(g, 1, 3 * c["scores_block"] + 40, totals, turn=gi), count)
        # `count` levels whose anchors sum to `total`: small ones first, the main level takes the rest
        small = ([(int(g.integers(1, 4)), 1, 1)] + [tuple(int(v) for v in g.integers(1, 4, 3)) for _ in range(count - 2)])[:count - 1]
        if sum(a * h * w for a, h, w in small) >= total:
            small = [(1, 1, 1)] * len(small)
        total = max(total, len(small) + 1)
        rest = total - sum(a * h * w for a, h, w in small)
        a, _, h, w = _split(rest, g, k_range=(1, 1))
        at = int(g.integers(0, count))
        levels = small[:at] + [(a, h, w)] + small[at:]
        return [("n", int(g.integers(1, 4))), ("levels", tuple(levels)), ("main", at), ("classes", _mix(g, 2, 91, [2, 3, 21, 90, 91])),
                ("kind", ("normal", "lattice", "all_equal", "special", "wide")[gi % 5]), ("layout", _layout(gi))]
    return _make("ssd_scores", chunk, build)


def _ssd_scores_inputs(case):
    g = case.g
    maps = []
    for l, (a, h, w) in enumerate(g["levels"]):
        count = a * g["classes"] * h * w
        if g["kind"] == "wide":  # logits far apart: exponentials that underflow to 0 and to denormals
            x = (rng(g["seed"] + l).standard_normal((g["n"], count)) * 40).astype(F32)
        else:
            x = _values(g["kind"], g["seed"] + l, g["n"], count, 1, 1, l)
        maps.append(x.reshape(g["n"], a * g["classes"], h, w))
    return dict(maps=maps)


def _ssd_scores_reference(case, d):
    from tests import _ssd_ref as SR
    return SR.scores([torch.from_numpy(m) for m in d["maps"]], case.g["classes"]).numpy()


def _ssd_topk(chunk):
    c = consts()
    rows = [1, 2, 30, 500] + around(c["ssd_step"], c["ssd_trip"], 2 * c["ssd_trip"])

    def build(g, i, gi, seed):
        kind = KINDS[gi % len(KINDS)]
        want = EXITS[(gi // len(KINDS)) % len(EXITS)] if kind == "sparse" else None
        v = _mix(g, 1, 2 * c["ssd_trip"] + 1, rows, turn=gi)
        classes = _mix(g, 2, 91, [2, 3, 91]) if v < 3000 else int(g.integers(2, 6))
        n = int(g.integers(1, 4))
        thr, rel = _deal(kind, gi)
        if kind == "normal":
            v = max(v, 5)
        if kind == "cut_in_ties":
            v = max(v, c["max_k"] + 16, c["ssd_trip"] + 64 if gi // len(KINDS) % 2 == 0 else 0)  # room below any k; every second one past a trip
        if kind == "sparse":
            v = max(v, 600, 3 << 8 * (7 - want) if want in (5, 6) else 0)
        if want == 4:
            v, classes, n = (1 << 24) + (3 << 10), 2, 1  # the one row past 2^24 anchors: 134 MB of scores
        if want == 5:
            classes, n = 2, 1
        k = _k_by_level(_mix(g, 1, c["max_k"], _k_edges(v), turn=gi + 1), v, kind, gi)
        if kind == "normal" and thr == "between":
            k = max(2, min(k, v - 2))
        geom = [("n", n), ("classes", classes), ("v", v), ("k", k), ("kind", kind), ("thr", thr), ("rel", rel)]
        if kind == "sparse":
            geom[3] = ("k", _ssd_sparse_k(dict(geom), seed, want))
            geom.append(("exit", want))
        return geom
    return _make("ssd_topk", chunk, build)


def _unit(x):
    """Logits -> scores in [0, 1] that keep the logits' ties (a float32 function of the logit alone); a NaN stays."""
    with np.errstate(all="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x.astype(np.float64)).astype(F32))).astype(F32)


def _ssd_sparse(g, seed):
    f, v, below = _sparse_picks(seed + 1, g["n"], 0, g["v"], g.get("exit"), lambda p: index_cut(p, 0, g["v"]))
    return f, _unit(v), below


def _ssd_sparse_k(g, seed, want):
    g = dict(g, exit=want)
    f, s, below = _ssd_sparse(g, seed)
    if below is not None:
        return below
    keys = np.sort(score_keys(s, f, np.ones(len(f), bool)))[::-1]
    if want == "early":
        return len(keys) + 3
    for k in range(1, len(keys)):
        if select_exit(keys, k)[0] == want:
            return k
    raise AssertionError(f"ssd_topk seed {seed}: no k leaves select_keys after pass {want}")


def _ssd_topk_inputs(case):
    """A score matrix (n, K, V) of the case's own, in [0, 1] as a softmax's (the keys order as the scores only there), NaN included;
    row 0, the background, is never read for a candidate and holds the greatest scores."""
    g = case.g
    n, kc, v, seed = g["n"], g["classes"], g["v"], g["seed"]
    if g["kind"] == "sparse":
        f, s, _ = _ssd_sparse(g, seed)
        rows = np.arange(n * kc)
        rows = rows[rows % kc != 0]  # every class row but the background holds the same places
        m = Sparse((n, kc, v, 1), 0.0, np.repeat(rows // kc, len(f)), np.tile(f, len(rows)) + np.repeat(rows % kc, len(f)) * v, np.tile(s, len(rows)))
        d = dict(scores=m if n * kc * v > LARGE else m.numpy().reshape(n, kc, v), sparse=dict(flat=f, scores=s))
        d["thresh"] = _sparse_threshold(g["thr"], F32(0), s)
        return d
    x = _values(g["kind"], seed, n * kc, v, g["k"], consts()["ssd_trip"] if case.index % 2 else consts()["ssd_step"], case.index + case.sweep)
    s = _unit(x).reshape(n, kc, v)
    s[:, 0] = 1.0
    return dict(scores=s, sparse=None, thresh=float(_threshold(g["thr"], s[0, 1], g["k"], g["rel"])))


def _ssd_topk_reference(case, d):
    from tests import _ssd_ref as SR
    g = case.g
    if d["sparse"] is None:
        return SR.select(torch.from_numpy(d["scores"]), g["k"], d["thresh"]).numpy()
    f, s = d["sparse"]["flat"], d["sparse"]["scores"]
    keep = s > F32(d["thresh"])
    sel = f[keep][np.lexsort((f[keep], -s[keep].astype(np.float64)))][:g["k"]]
    out = np.full((g["n"], (g["classes"] - 1), g["k"]), -1, np.int32)
    for c in range(1, g["classes"]):
        out[:, c - 1, :len(sel)] = sel * g["classes"] + c
    return out.reshape(g["n"], -1)


# ---- 4. the decode families -------------------------------------------------------------------------------------------------------------
def _hand_tail(total_flat):
    """The indices no selection writes: the padding, the first past the pyramid, the ends of int32, the first and the last valid."""
    return [-1, total_flat, 2 ** 31 - 1, -2 ** 31, 0, total_flat - 1]


def _decode_geom(g, gi, a_hi, classes):
    c = consts()
    counts = [1, 2, 11] + around(c["scores_block"])
    count = _mix(g, 1, 2 * c["scores_block"], counts, turn=gi)
    a, _, h, w = _split(count, g, a_hi=a_hi, k_range=(1, 1))
    levels, at = _pyramid(g, gi, (a, h, w), a_hi=min(a_hi, 4))
    strides = tuple((int(g.integers(1, 40)), int(g.integers(1, 40))) for _ in levels)
    return [("n", int(g.integers(1, 4))), ("levels", levels), ("main", at), ("classes", classes), ("k", _mix(g, 1, 300, [1, 2, 255, 256, 257])),
            ("strides", strides), ("layout", _layout(gi))]


def _ret_decode(chunk):
    def build(g, i, gi, seed):
        geom = _decode_geom(g, gi, 12, _mix(g, 1, 91, [1, 2, 91]))
        return geom + [("weights", ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0), (2.0, 3.0, 0.5, 1.5))[gi % 3]), ("clip", (CLIP, 2.0)[gi // 3 % 2])]
    return _make("ret_decode", chunk, build)


def _fcos_decode(chunk):
    return _make("fcos_decode", chunk, lambda g, i, gi, seed: _decode_geom(g, gi, 1, _mix(g, 1, 91, [1, 2, 91])))


def _rpn_decode(chunk):
    def build(g, i, gi, seed):
        geom = _decode_geom(g, gi, 12, 1)
        return geom + [("weights", ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0))[gi % 2]), ("min_size", (1e-3, 4.0, 0.0)[gi % 3]),
                       ("score_thresh", (0.0, 0.5, 0.3)[gi // 3 % 3])]
    return _make("rpn_decode", chunk, build)


def _deltas(seed, n, a, h, w, weights):
    """N(0, 1) codes (times the weights, so that dx .. dh are N(0, 1) after the division) with values above, at and one float above the
    clip, NaN and +-Inf sprinkled in."""
    r = rng(seed)
    d = r.standard_normal((n, a, 4, h * w)).astype(F32)
    u = r.random(d.shape)
    clip32 = F32(CLIP)
    for lo, hi, v in ((0, .02, np.nan), (.02, .03, np.inf), (.03, .04, -np.inf), (.04, .06, 9.0), (.06, .08, clip32),
                      (.08, .10, np.nextafter(clip32, F32(9)))):
        d[(u >= lo) & (u < hi)] = v
    d *= np.asarray(weights, F32).reshape(1, 1, 4, 1)
    return d.reshape(n, 4 * a, h, w)


def _cell_anchors(seed, levels):
    r = rng(seed)
    out = []
    for a, _, _ in levels:
        half = (r.integers(1, 120, (a, 2)) / 2).astype(F32)
        out.append(np.concatenate([-half, half], 1) + (r.integers(-4, 5, (a, 1)) / 2).astype(F32))
    return out


def grid_anchors(levels, cells, strides):
    """AnchorGenerator.grid_anchors in numpy: the int32 shifts (x sw, y sh) plus the float32 base anchors, in the (y, x, a) layout."""
    out = []
    for (a, h, w), base, (sh, sw) in zip(levels, cells, strides):
        sy, sx = np.meshgrid(np.arange(h, dtype=np.int32) * np.int32(sh), np.arange(w, dtype=np.int32) * np.int32(sw), indexing="ij")
        shifts = np.stack([sx, sy, sx, sy], -1).reshape(-1, 1, 4).astype(F32)
        out.append((shifts + base[None]).astype(F32).reshape(-1, 4))
    return np.concatenate(out)


def _image_sizes(seed, n, levels, strides):
    """Images smaller than the anchors reach, so that every border clips; half sizes included."""
    r = rng(seed)
    reach_h = max(h * s[0] for (_, h, _), s in zip(levels, strides))
    reach_w = max(w * s[1] for (_, _, w), s in zip(levels, strides))
    return [(float(max(1, int(reach_h * (0.3 + 0.5 * r.random())))) + 0.5 * (i % 2), float(max(1, int(reach_w * (0.3 + 0.5 * r.random()))))) for i in range(n)]


def _pyramid_decode_inputs(case):
    g = case.g
    fam = case.family
    n, kc, seed = g["n"], g["classes"], g["seed"]
    weights = g.get("weights", (1.0, 1.0, 1.0, 1.0))
    logits = [_values("special" if l % 2 else "centred", seed + l, n, a * kc * h * w, 1, 1, l).reshape(n, a * kc, h, w) for l, (a, h, w) in enumerate(g["levels"])]
    deltas = [_deltas(seed + 20 + l, n, a, h, w, weights) for l, (a, h, w) in enumerate(g["levels"])]
    d = dict(logits=logits, deltas=deltas, cells=_cell_anchors(seed + 40, g["levels"]), sizes=_image_sizes(seed + 41, n, g["levels"], g["strides"]))
    if fam == "fcos_decode":
        d["ctrs"] = [(rng(seed + 60 + l).standard_normal((n, 1, h, w)) * 2).astype(F32) for l, (_, h, w) in enumerate(g["levels"])]
        d["cells"] = [c[:1] for c in d["cells"]]
        for m in deltas:  # the head's ReLU has run over most of a regression map; the kernel's max(r, 0) covers the rest
            m[(m < 0) & (rng(seed + 61).random(m.shape) < 0.8)] = 0
    total = int(level_starts(g["levels"])[-1]) * kc
    # idx: the reference's own selection, then the hand tail
    if fam == "ret_decode":
        from tests import _retinanet_ref as RR
        sel = RR.select([torch.from_numpy(m) for m in logits], kc, g["k"], 0.3).numpy()
    elif fam == "fcos_decode":
        from tests import _fcos_ref as FR
        sel = FR.select([torch.from_numpy(m) for m in logits], [torch.from_numpy(m) for m in d["ctrs"]], kc, g["k"], 0.3).numpy()
    else:
        sel = _rpn_topk_reference(case, dict(maps=logits, sparse=None))
    tail = np.asarray(_hand_tail(total), np.int64).astype(np.int32)
    d["idx"] = np.ascontiguousarray(np.concatenate([sel, np.broadcast_to(tail, (n, len(tail)))], 1).astype(np.int32))
    return d


def _pyramid_decode_reference(case, d):
    from tests import _fcos_ref as FR
    from tests import _retinanet_ref as RR
    g = case.g
    t = lambda maps: [torch.from_numpy(m) for m in maps]  # noqa: E731
    anchors = torch.from_numpy(grid_anchors(g["levels"], d["cells"], g["strides"]))
    idx = torch.from_numpy(d["idx"])
    with np.errstate(all="ignore"):
        if case.family == "fcos_decode":
            out = FR.decode(t(d["logits"]), t(d["ctrs"]), t(d["deltas"]), idx, [anchors] * g["n"], d["sizes"], g["classes"])
        elif case.family == "ret_decode":
            out = RR.decode(t(d["logits"]), t(d["deltas"]), idx, [anchors] * g["n"], d["sizes"], g["classes"], g["weights"], g["clip"])
        else:
            boxes, scores, _, ok = RR.decode(t(d["logits"]), t(d["deltas"]), idx, [anchors] * g["n"], d["sizes"], 1, g["weights"], CLIP)
            starts = torch.from_numpy(level_starts(g["levels"])[:-1])
            levels = torch.where(ok, (idx.long()[..., None] >= starts).sum(-1) - 1, torch.full_like(idx.long(), -1))
            ws, hs = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
            valid = ok & (ws >= g["min_size"]) & (hs >= g["min_size"]) & (scores >= g["score_thresh"])
            out = (boxes, scores, levels, valid)
    return tuple(o.numpy() for o in out)


def _ssd_decode(chunk):
    def build(g, i, gi, seed):
        geom = _decode_geom(g, gi, 6, _mix(g, 2, 91, [2, 3, 91]))
        geom = [p for p in geom if p[0] != "strides"]
        levels = dict(geom)["levels"]
        steps = None if gi % 2 else tuple(float(int(g.integers(1, 40))) + 0.5 * (l % 2) for l in range(len(levels)))
        return geom + [("steps", steps), ("clip_pairs", bool(gi // 2 % 2)), ("weights", ((10.0, 10.0, 5.0, 5.0), (1.0, 2.0, 3.0, 0.5))[gi // 4 % 2]),
                       ("batch", (int(g.integers(8, 400)), int(g.integers(8, 400))))]
    return _make("ssd_decode", chunk, build)


class _Gen:
    """What _ssd_ref.default_boxes reads of a DefaultBoxGenerator."""

    def __init__(self, pairs, steps, clip):
        self._wh_pairs, self.steps, self.clip = pairs, steps, clip


def _ssd_decode_inputs(case):
    g = case.g
    n, kc, seed = g["n"], g["classes"], g["seed"]
    r = rng(seed)
    total = int(level_starts(g["levels"])[-1])
    scores = r.random((n, kc, total), dtype=F32)
    scores[r.random(scores.shape) < 0.03] = np.nan
    deltas = [_deltas(seed + 20 + l, n, a, h, w, g["weights"]) for l, (a, h, w) in enumerate(g["levels"])]
    pairs = [(r.random((a, 2), dtype=F32) * F32(1.4)).astype(F32) for a, _, _ in g["levels"]]  # some above 1: the clamp matters
    bh, bw = g["batch"]
    sizes = [(float(max(1, int(bh * (0.4 + 0.5 * r.random())))), float(max(1, int(bw * (0.4 + 0.5 * r.random()))))) for _ in range(n)]
    from tests import _ssd_ref as SR
    sel = SR.select(torch.from_numpy(np.nan_to_num(scores, nan=0.0)), min(g["k"], 7), 0.6).numpy()
    tail = np.asarray(_hand_tail(total * kc), np.int64).astype(np.int32)
    idx = np.ascontiguousarray(np.concatenate([sel, np.broadcast_to(tail, (n, len(tail)))], 1).astype(np.int32))
    return dict(scores=scores, deltas=deltas, pairs=pairs, sizes=sizes, idx=idx)


def _ssd_decode_reference(case, d):
    from tests import _ssd_ref as SR
    g = case.g
    gen = _Gen([torch.from_numpy(p) for p in d["pairs"]], g["steps"], g["clip_pairs"])
    dboxes = SR.default_boxes(gen, [(h, w) for _, h, w in g["levels"]], g["batch"])
    out = SR.decode(torch.from_numpy(d["scores"]), [torch.from_numpy(m) for m in d["deltas"]], torch.from_numpy(d["idx"]), dboxes, d["sizes"], g["weights"])
    return tuple(o.numpy() for o in out)


# ---- 5. roi_det, box_decode -------------------------------------------------------------------------------------------------------------
def _roi_det(chunk):
    c = consts()
    rois = list(range(0, 10)) + around(c["roi_waves"], 2 * c["roi_waves"], c["wave"])
    classes = [2] + around(c["wave"], 2 * c["wave"], 3 * c["wave"], lo=2)

    def build(g, i, gi, seed):
        r, k = _mix(g, 0, 70, rois, turn=gi), _mix(g, 2, 200, classes, turn=gi + 1)
        if gi == 1:
            r, k = 3, c["roi_max_classes"]  # the one case at the limit
        return [("r", r), ("classes", k), ("n", 1 + gi % 3), ("sliced", bool(gi // 2 % 2)), ("weights", ((10.0, 10.0, 5.0, 5.0), (1.0, 1.0, 1.0, 1.0))[gi % 2]),
                ("score_thresh", (0.05, 1e-3, -1.0, 0.5)[gi % 4]), ("min_size", (1e-2, 0.0, 3.0)[gi % 3])]
    return _make("roi_det", chunk, build)


def bad_image_indices(n):
    return [float("nan"), -1.0, -0.5, n - 0.5, float(n)]


def _roi_det_inputs(case):
    g = case.g
    r, c, n, seed = g["r"], g["classes"], g["n"], g["seed"]
    q = rng(seed)
    logits = (q.standard_normal((r, c)) * 3).astype(F32)
    for i in range(r):
        kind = (i + c) % 8
        if kind == 1:
            logits[i] = 0.75
        elif kind == 2:
            logits[i] = (q.standard_normal(c) * 3 - 25).astype(F32)
            logits[i, (i * 5 + 1) % c] = 80.0
        elif kind == 3:
            logits[i] = np.array([0.0, -0.0], F32)[q.integers(0, 2, c)]
        elif kind == 4:
            logits[i, (i * 3) % c] = np.nan
        elif kind == 5:
            logits[i, (i * 3 + 1) % c] = np.inf
        elif kind == 6:
            logits[i] = -np.inf
    deltas = _deltas(seed + 1, 1, r * c, 1, 1, g["weights"]).reshape(r, 4 * c) if r else np.zeros((0, 4 * c), F32)
    sizes = [(40.0 + 7 * i, 60.0 - 5 * i + 0.5) for i in range(n)]
    p = q.random((r, 2)) * np.array([70.0, 50.0]) - 8
    boxes = np.concatenate([p, p + 1 + q.random((r, 2)) * 40], 1).astype(F32)
    image = (np.arange(r) % n).astype(F32)
    bad = bad_image_indices(n)
    for j, i in enumerate(range(2, r, 4)):
        image[i] = bad[j % len(bad)]
    return dict(logits=logits, deltas=deltas, rois=np.concatenate([image[:, None], boxes], 1).astype(F32).reshape(r, 5), sizes=sizes)


def roi_image(index, n):
    """The image of a roi as k_roi_detections reads its float index: truncated inside (-1, n), else none."""
    if not (index > -1.0 and index < n):
        return None
    i = int(index)
    return i if i < n else None


def _roi_det_reference(case, d):
    from tests import _roi_heads_ref as H
    g = case.g
    r, c = g["r"], g["classes"]
    heads = H.RoIHeads(None, None, None, 0.5, 0.5, 512, 0.25, g["weights"], g["score_thresh"], 0.5, 100, numerics=H.RESTATEMENT)
    boxes, scores = np.zeros((r, c - 1, 4), F32), np.zeros((r, c - 1), F32)
    labels, valid = np.zeros((r, c - 1), np.int64), np.zeros((r, c - 1), bool)
    images = [roi_image(float(v), g["n"]) for v in d["rois"][:, 0]]
    logits, deltas, rois = torch.from_numpy(d["logits"]), torch.from_numpy(d["deltas"]), torch.from_numpy(d["rois"])
    for img in range(g["n"]):
        rows = [i for i, v in enumerate(images) if v == img]
        if not rows:
            continue
        with np.errstate(all="ignore"):
            out = heads.dense(logits[rows], deltas[rows], [rois[rows, 1:]], [d["sizes"][img]], g["min_size"])
        boxes[rows], scores[rows], labels[rows], valid[rows] = (o.numpy() for o in out)
    return boxes, scores, labels, valid


def _box_decode(chunk):
    c = consts()

    def build(g, i, gi, seed):
        return [("m", _mix(g, 0, 600, [0, 1, 2, 600] + around(c["scores_block"], 2 * c["scores_block"]), turn=gi)), ("c", 1 + gi % 7),
                ("weights", ((10.0, 10.0, 5.0, 5.0), (1.0, 1.0, 1.0, 1.0), (2.0, 3.0, 0.5, 1.5))[gi % 3]), ("clip", (CLIP, 2.0)[gi // 3 % 2])]
    return _make("box_decode", chunk, build)


def _box_decode_inputs(case):
    g = case.g
    m, c = g["m"], g["c"]
    q = rng(g["seed"])
    p = q.random((m, 2)) * 100 - 10
    boxes = np.concatenate([p, p + q.random((m, 2)) * 60 - 2], 1).astype(F32)  # a few inverted boxes
    codes = _deltas(g["seed"] + 1, 1, m * c, 1, 1, g["weights"]).reshape(m, 4 * c) if m else np.zeros((0, 4 * c), F32)
    return dict(boxes=boxes.reshape(m, 4), codes=codes)


def _box_decode_reference(case, d):
    from tests import _rpn_ref as P
    g = case.g
    with np.errstate(all="ignore"):
        return P.BoxCoder(g["weights"], g["clip"], numerics=P.RESTATEMENT).decode_single(torch.from_numpy(d["codes"]), torch.from_numpy(d["boxes"])).numpy()


GENERATORS = {"rpn_topk": _rpn_topk, "rpn_decode": _rpn_decode, "ret_topk": _onestage_topk("ret_topk"), "fcos_topk": _onestage_topk("fcos_topk"),
              "ret_decode": _ret_decode, "fcos_decode": _fcos_decode, "ssd_scores": _ssd_scores, "ssd_topk": _ssd_topk, "ssd_decode": _ssd_decode,
              "roi_det": _roi_det, "box_decode": _box_decode}
INPUTS = {"rpn_topk": _rpn_topk_inputs, "rpn_decode": _pyramid_decode_inputs, "ret_topk": _onestage_inputs, "fcos_topk": _onestage_inputs,
          "ret_decode": _pyramid_decode_inputs, "fcos_decode": _pyramid_decode_inputs, "ssd_scores": _ssd_scores_inputs, "ssd_topk": _ssd_topk_inputs,
          "ssd_decode": _ssd_decode_inputs, "roi_det": _roi_det_inputs, "box_decode": _box_decode_inputs}
REFERENCES = {"rpn_topk": _rpn_topk_reference, "rpn_decode": _pyramid_decode_reference, "ret_topk": _onestage_reference,
              "fcos_topk": _onestage_reference, "ret_decode": _pyramid_decode_reference, "fcos_decode": _pyramid_decode_reference,
              "ssd_scores": _ssd_scores_reference, "ssd_topk": _ssd_topk_reference, "ssd_decode": _ssd_decode_reference,
              "roi_det": _roi_det_reference, "box_decode": _box_decode_reference}
assert set(GENERATORS) == set(INPUTS) == set(REFERENCES) == set(SWEEPS)


def inputs(case):
    """{name: value} of a case, from its geometry and its seed alone."""
    return INPUTS[case.family](case)


def reference(case, d):
    """The CPU reference of a case on inputs(case)."""
    return REFERENCES[case.family](case, d)
