"""The cases tests/test_special_values_host.py and tests/test_gpu_special_values.py share: for every arithmetic entry point the
shapes (the rows of tests/_layer_guard_cases.py with their MV_* knobs and expected kernel), seeded finite inputs, the input that
receives NaN / Inf, its sites (tests/_special_values.poison_sites), the geometry of its footprint, the oracle call and -- where
one exists -- torch's CPU op.  The host file proves on the oracle alone that no case is vacuous; the GPU file runs the kernels.

A case is data plus two small callables (`oracle(inputs) -> numpy`, `torch_ref(inputs) -> numpy | None`); the GPU call lives in
the GPU test.  No fixtures, no device code.

Scales of the range runs.  Every input has a role: "x" and "w" are the two factors of the products, "out" terms (bias, beta,
residual) are added to sums of products, None is left alone (alpha).  With S = sx * sw a run scales x by sx, w by sw and the
"out" terms by S -- powers of two, so the finite result is the clean one times S wherever nothing under- or overflows.
  subnormal run: sx = 2^-100 (1 where x is uint8), S = 2^floor(log2(2^-127 / max |y|)): the largest output lies in the top
                 subnormal binade, the rest below it;
  overflow run:  sx = 2^100, S = the smallest power of two, from 2^(floor(log2(FLT_MAX / max |y|)) - 8) upwards, at which the
                 oracle's result holds an Inf: the few largest chains overflow, at the end or on the way in the oracle's
                 stated order, the rest stay finite.  The "out" terms are scaled by S / 8 in this run, so that a bias that
                 dominates its output (a 1 x 1 depthwise map) does not reach FLT_MAX before any sum of products does.
y is the oracle's result on the clean inputs.  An op without a "w" (pooling, the filters with fixed taps) scales x by S.  The
host test checks the conditions the issue sets on every case."""
import functools

import numpy as np

from oracle import ref
from tests import _layer_guard_cases as T, _special_values as S
from tests._util import philox_f32, philox_u8

FLT_MAX = float(np.finfo(np.float32).max)
OVERFLOW_OUT_SHIFT = 3  # the overflow run scales the "out" terms by S / 8: the sums of products overflow before a bias does


class Case:
    def __init__(self, family, name, make, oracle, geometry, roles, kernel, env=None, plan=None, poison="x", torch_ref=None, call=None,
                 extras=(), switches=None, note="", x_exp=None, inf_reaches_output=True, dtype="float32", overflow=True,
                 subnormal_outputs=True):
        self.family, self.name, self.id = family, name, f"{family}-{name}"
        self._make, self.oracle, self.geometry, self.roles, self.kernel = make, oracle, geometry, roles, kernel
        self.env, self.plan, self.poison, self.torch_ref, self.call = dict(env or {}), dict(plan or {}), poison, torch_ref, call or {}
        self.extras, self.switches, self.note = tuple(extras), dict(switches or {}), note
        self.inf_reaches_output = inf_reaches_output  # False: ReLU6 between x and y, no residual -- an Inf in x ends as 0 or 6
        self.dtype = dtype  # storage type of x and y; "bfloat16" data is held as float32 arrays of bfloat16 values (numpy has no such type)
        self.overflow = overflow  # False: finite inputs cannot overflow the op (a convex combination, a clamp): no overflow run
        # False: the op maps subnormal inputs to normal outputs (autocontrast rescales to [0, 1], normalize subtracts a mean): the
        # subnormal run scales x by 2^-128 and the condition is on the inputs
        self.subnormal_outputs = subnormal_outputs
        self.x_exp = x_exp  # {run: exponent of x} where +-100 does not fit the op (a block with ReLU6 inside)

    @functools.cached_property
    def clean(self):
        """{name: numpy array or None}: seeded finite inputs, never modified (copies are made before poisoning)."""
        d = self._make()
        for v in d.values():
            if v is not None:
                v.setflags(write=False)
        return d

    def quantize(self, a):
        """`a` rounded to the case's storage type (a no-op but for bfloat16, whose values live in float32 arrays)."""
        if self.dtype != "bfloat16" or a is None:
            return a
        import torch
        return torch.from_numpy(np.array(a, np.float32)).to(torch.bfloat16).float().numpy()

    @functools.cached_property
    def sites(self):
        return S.poison_sites(self.clean[self.poison].shape, self.plan) if self.poison else {}

    @functools.cached_property
    def out_shape(self):
        return self._first(self.want_clean).shape

    def extra_footprint(self, name, site):
        """A per-channel term (one index) reaches its whole output channel, a residual cell the output cell of the same index, a
        cell of a deformable conv's mask every channel of its output pixel (at most)."""
        if name == "mask":
            m = np.zeros(self.out_shape, bool)
            m[site[0], :, site[2], site[3]] = True
            return m
        if len(site) == 1:
            return S.footprint(site, dict(op="channel", out_shape=self.out_shape))
        return S.footprint(site, dict(op="pointwise", in_shape=self.out_shape))

    @functools.cached_property
    def placement_plan(self):
        """(sites of x, extras) of the placement run: the pair first, then the epilogue terms, then the other sites, as long as
        the union of the footprints leaves half of the outputs untouched (S.choose_sites)."""
        names, cells = [], set()
        for n, site in self.sites.items():  # two names of one cell (`first` of a one-column map is pair_a): the first name
            if tuple(site) not in cells:
                names.append(n)
                cells.add(tuple(site))
        head = [n for n in names if n.startswith("pair_")]
        cands = [(("x", n), S.footprint(self.sites[n], self.geometry)) for n in head]
        cands += [(("extra", i), self.extra_footprint(name, site)) for i, (name, site, _) in enumerate(self.extras)]
        cands += [(("x", n), S.footprint(self.sites[n], self.geometry)) for n in names if n not in head]
        chosen = S.choose_sites(cands)
        return ({n: self.sites[n] for k, n in chosen if k == "x"}, [self.extras[i] for k, i in chosen if k == "extra"])

    @property
    def placement_sites(self):
        return self.placement_plan[0]

    def placement_inputs(self):
        """x with +Inf, -Inf, NaN in turn at the chosen sites (the first two are pair_a and pair_b: Inf - Inf occurs), and the
        chosen epilogue terms of `extras` with one non-finite entry each."""
        d = dict(self.clean)
        sites, extras = self.placement_plan
        if self.poison:
            d[self.poison] = S.poisoned(self.clean[self.poison], sites)
        for name, site, value in extras:
            a = np.array(d[name], copy=True)
            a[tuple(site)] = value
            d[name] = a
        return d

    def with_site(self, site, value):
        d = dict(self.clean)
        a = np.array(d[self.poison], copy=True)
        a[tuple(site)] = value
        d[self.poison] = a
        return d

    @functools.cached_property
    def want_clean(self):
        return self.oracle(self.clean)

    def _first(self, y):
        return y[0] if isinstance(y, tuple) else y

    def _roles(self, run):
        return self.roles[run] if "subnormal" in self.roles else self.roles

    def _scaled(self, ex, es, out_shift=0, run="subnormal"):
        """The clean inputs with x * 2^ex, w * 2^(es - ex) and the "out" terms * 2^(es - out_shift) (x * 2^es where there is no w)."""
        roles = self._roles(run)
        has_w = "w" in roles.values()
        d = {}
        for name, a in self.clean.items():
            role = roles.get(name)
            if a is None or role is None or a.dtype.kind != "f":
                d[name] = a
                continue
            e = {"x": ex if has_w else es, "w": es - ex, "out": es - out_shift}[role]
            with np.errstate(over="ignore"):
                b = self.quantize(np.ldexp(a.astype(np.float64), e).astype(a.dtype))
            if not np.isfinite(b).all():
                return None  # an input itself overflows at this scale
            d[name] = b
        return d

    @functools.lru_cache(maxsize=None)
    def exponents(self, run):
        """(ex, es) of the "subnormal" or "overflow" run: the rule of the module docstring."""
        y = np.abs(self._first(self.want_clean).astype(np.float64))
        top = y[np.isfinite(y)].max()
        x_is_float = self.clean[[k for k, r in self._roles(run).items() if r == "x"][0]].dtype.kind == "f"
        if run == "subnormal" and not self.subnormal_outputs:
            return 0, -128
        if run == "subnormal":
            ex = self.x_exp[run] if self.x_exp else (-100 if x_is_float else 0)
            tiny = {"float16": 2.0 ** -14, "float64": 2.0 ** -1022}.get(self.dtype, 2.0 ** -126)  # the smallest normal value
            return ex, int(np.floor(np.log2(tiny / 2 / top)))
        ex = self.x_exp[run] if self.x_exp else (100 if x_is_float else 0)
        es = int(np.floor(np.log2({"float16": 65504.0, "float64": float(np.finfo(np.float64).max)}.get(self.dtype, FLT_MAX)) - np.log2(top))) - 8
        for es in range(es, es + 16):
            d = self._scaled(ex, es, OVERFLOW_OUT_SHIFT, run)
            if d is not None and any(np.isinf(o).any() for o in self._outputs(self.oracle(d))):
                return ex, es
        raise AssertionError(f"{self.id}: no power-of-two scale near FLT_MAX / max |y| makes a chain of the oracle overflow")

    def _outputs(self, y):
        return y if isinstance(y, tuple) else (y,)

    def range_inputs(self, run):
        return self._scaled(*self.exponents(run), out_shift=OVERFLOW_OUT_SHIFT if run == "overflow" else 0, run=run)

    def __repr__(self):
        return self.id


def _two_images_if_one_pixel(n, oh, ow):
    """A table row with one output pixel per image runs at batch 4 here: every cell of an image lies in that pixel's field, so a
    poisoned cell takes the whole image; the Inf - Inf pair and the lone Inf take one image each and leave half."""
    return max(n, 4) if oh * ow == 1 else n


def _shape_id(shape, env=None):
    return "x".join(map(str, shape)) + "".join(f",{k[3:].lower()}={v}" for k, v in (env or {}).items())


# ---- 3 x 3 conv: F.conv2d_bias_relu (every row of CONV3X3) and F.normalized_conv2d_bias_relu ---------------------------------------
def _torch_conv(x, w, b, stride=1, padding=1, dilation=1, groups=1, relu=False):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.array(a))  # noqa: E731
    y = torch.nn.functional.conv2d(t(x), t(w), t(b), stride, padding, dilation, groups)
    return (torch.relu(y) if relu else y).numpy()


def _conv3x3_cases():
    out = []
    for i, row in enumerate(T.CONV3X3):
        n, cin, cout, h, w = row["shape"]
        sl = row["slice_channels"] if row["slices"] > 1 else 0
        # (bias, relu): the K-sliced rows and the three kernels besides k_conv3x3_gen run all four combinations, the other rows
        # take them in turn
        combos = [(True, True), (False, False), (True, False), (False, True)]
        variants = combos if (row["slices"] > 1 or row["kernel"] != "k_conv3x3_gen") else [combos[i % 4]]
        for bias, relu in variants:
            def make(row=row, bias=bias):
                n, cin, cout, h, w = row["shape"]
                return {"x": philox_f32(9000 + cin + h, (n, cin, h, w)) - 0.5, "w": (philox_f32(9001 + cout, (cout, cin, 3, 3)) - 0.5) * 0.4,
                        "b": (philox_f32(9002 + w, (cout,)) - 0.5) if bias else None}
            geometry = dict(op="conv", in_shape=(n, cin, h, w), cout=cout, k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), groups=1)
            extras = [("b", (cout - 1,), S.PINF)] if bias else []
            out.append(Case("conv3x3", _shape_id(row["shape"], row["env"]) + f",bias={int(bias)},relu={int(relu)}", make,
                            lambda d, relu=relu, sl=sl: ref.conv3x3_bias_relu(d["x"], d["w"], d["b"], relu=relu, slice_channels=sl),
                            geometry, {"x": "x", "w": "w", "b": "out"}, row["kernel"], env=row["env"], plan={"slice": sl},
                            torch_ref=lambda d, relu=relu: _torch_conv(d["x"], d["w"], d["b"], relu=relu), call=dict(relu=relu), extras=extras,
                            note=row["why"]))
    return out


U8_MEAN, U8_STD = [0.4, 0.5, 0.3], [0.2, 0.25, 0.3]


def _conv3x3_u8norm_cases():
    """uint8 pixels cannot hold a NaN: the bias alone is poisoned (its footprint is a whole output channel), and the range runs
    scale the weights and the bias only."""
    out = []
    for n, cout, h, w in T.CONV3X3_U8NORM:
        def make(n=n, cout=cout, h=h, w=w):
            return {"x": philox_u8(9100 + w, (n, 3, h, w)), "w": (philox_f32(9101 + cout, (cout, 3, 3, 3)) - 0.5) * 0.4,
                    "b": philox_f32(9102 + h, (cout,)) - 0.5}
        extras = [("b", (0,), S.NAN), ("b", (cout - 1,), S.PINF), ("b", (cout // 2,), S.NINF)]
        out.append(Case("conv3x3_u8norm", _shape_id((n, cout, h, w)), make,
                        lambda d: ref.conv3x3_bias_relu(ref.to_float_normalize(d["x"], U8_MEAN, U8_STD), d["w"], d["b"], relu=False),
                        dict(op="channel", out_shape=(n, cout, h, w)), {"x": "x", "w": "w", "b": "out"}, "k_conv3x3_c3", poison=None,
                        torch_ref=lambda d: _torch_conv(ref.to_float_normalize(d["x"], U8_MEAN, U8_STD), d["w"], d["b"]), extras=extras))
    return out


# ---- linear: F.linear_bias_relu (every row of LINEAR) ---------------------------------------------------------------------------------
def _linear_cases():
    out = []
    for i, row in enumerate(T.LINEAR):
        n, k, m = row["shape"]
        sl = row["slice_len"] if row["slices"] > 1 else 0
        bias, relu = i % 2 == 0, i % 3 != 1

        def make(row=row, bias=bias):
            n, k, m = row["shape"]
            return {"x": philox_f32(9200 + k, (n, k)) - 0.5, "w": (philox_f32(9201 + m, (m, k)) - 0.5) * 0.2,
                    "b": (philox_f32(9202 + n, (m,)) - 0.5) if bias else None}

        def torch_ref(d, relu=relu):
            import torch
            y = torch.nn.functional.linear(torch.from_numpy(np.array(d["x"])), torch.from_numpy(np.array(d["w"])), None if d["b"] is None else torch.from_numpy(np.array(d["b"])))
            return (torch.relu(y) if relu else y).numpy()
        out.append(Case("linear", _shape_id(row["shape"]) + f",bias={int(bias)},relu={int(relu)}", make,
                        lambda d, relu=relu, sl=sl: ref.linear_bias_relu(d["x"], d["w"], d["b"], relu=relu, slice_len=sl),
                        dict(op="linear", in_shape=(n, k), m=m), {"x": "x", "w": "w", "b": "out"}, row["kernel"],
                        plan={"matrix": True, "slice": sl}, torch_ref=torch_ref, call=dict(relu=relu),
                        extras=[("b", (m - 1,), S.NINF)] if bias else [], note=row["why"]))
    return out


# ---- MobileNet kernels: F.conv_norm_act over STEM, DEPTHWISE and POINTWISE; F.adaptive_avg_pool2d -----------------------------------
# (bias, affine, act, residual).  ReLU6 is left out: it clamps an overflowed sum to 6, so a row that carries it cannot meet the
# overflow run's "one Inf" condition.  The depthwise rows take the two epilogues without ReLU: the footprint of a cell is at most
# nine outputs of one channel, and where ReLU turns all of them to 0 with and without a +Inf (a negative tap, outputs that were 0
# already) the locality check's "at least one output inside differs" cannot hold although nothing is wrong.
CNA_EPILOGUES = [(True, 1, None, True), (False, 0, "relu", False), (True, 2, "hardswish", True), (False, 2, "relu", False)]
AFFINE_NAMES = {0: None, 1: "mul_add", 2: "fma"}


def _cna_case(family, name, shape_x, w_shape, cout, stride, groups, epilogue, seed, kernel, slice_len=0, note=""):
    n, cin, h, w = shape_x
    bias, affine, act, residual = epilogue
    kh = w_shape[2]
    pad = (kh - 1) // 2
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1

    def make():
        return {"x": philox_f32(seed, shape_x) - 0.5, "w": (philox_f32(seed + 7, w_shape) - 0.5) * 0.4,
                "bias": (philox_f32(seed + 1, (cout,)) - 0.5) if bias else None,
                "alpha": (philox_f32(seed + 2, (cout,)) + 0.5) if affine else None,
                "beta": (philox_f32(seed + 3, (cout,)) - 0.5) if affine else None,
                "residual": (philox_f32(seed + 4, (n, cout, oh, ow)) - 0.5) if residual else None}

    def oracle(d):
        return ref.conv2d_affine_act(d["x"], d["w"], d["bias"], d["alpha"], d["beta"], d["residual"], stride, pad, groups, affine, act, slice_len=slice_len)

    def torch_ref(d):
        """conv2d, then the epilogue in torch ops (mul + add for both folded-norm forms: the NaN and Inf positions of a fused
        multiply-add and of mul then add are the same unless the product alone overflows, which these inputs do not do)."""
        import torch
        t = lambda a: None if a is None else torch.from_numpy(np.array(a))  # noqa: E731
        y = torch.nn.functional.conv2d(t(d["x"]), t(d["w"]), t(d["bias"]), stride, pad, 1, groups)
        if affine:
            y = y * t(d["alpha"]).view(1, -1, 1, 1) + t(d["beta"]).view(1, -1, 1, 1)
        if residual:
            y = t(d["residual"]) + y
        if act == "relu":
            y = torch.relu(y)
        elif act == "hardswish":
            y = y * torch.clamp(y + 3, 0, 6) / 6  # the source's expression; F.hardswish's CPU kernel is the same one
        return y.numpy()
    extras = []
    if bias:
        extras.append(("bias", (0,), S.PINF))
    if affine:
        extras += [("alpha", (cout - 1,), S.PINF), ("beta", (cout // 2,), S.NAN)]
    if residual:
        extras.append(("residual", (n - 1, cout - 1 if cout < 3 else 1, oh - 1, ow - 1), S.NINF))
    geometry = dict(op="conv", in_shape=shape_x, cout=cout, k=(kh, kh), stride=(stride, stride), pad=(pad, pad), dil=(1, 1), groups=groups)
    return Case(family, name + f",{'b' if bias else ''}a{affine}{act or 'none'}{'+r' if residual else ''}", make, oracle, geometry,
                {"x": "x", "w": "w", "bias": "out", "beta": "out", "residual": "out", "alpha": None}, kernel, plan={"slice": slice_len},
                torch_ref=torch_ref, call=dict(stride=stride, groups=groups, affine=AFFINE_NAMES[affine], activation=act), extras=extras, note=note)


def _conv_norm_act_cases():
    out = []
    for i, (n, cin, cout, h, w, stride) in enumerate(T.STEM):
        n = _two_images_if_one_pixel(n, (h - 1) // stride + 1, (w - 1) // stride + 1)
        out.append(_cna_case("stem", _shape_id((n, cin, cout, h, w, stride)), (n, cin, h, w), (cout, cin, 3, 3), cout, stride, 1, CNA_EPILOGUES[i % 4],
                             9610 + h, "k_conv3x3_smallcin"))
    for i, ((n, c, h, w, stride), kernel, why) in enumerate(T.DEPTHWISE):
        n = _two_images_if_one_pixel(n, (h - 1) // stride + 1, (w - 1) // stride + 1)
        out.append(_cna_case("depthwise", _shape_id((n, c, h, w, stride)), (n, c, h, w), (c, 1, 3, 3), c, stride, c, CNA_EPILOGUES[(i + 1) % 2 * 2],
                             9710 + h + w, kernel, note=why))
    for i, row in enumerate(T.POINTWISE):
        n, cin, cout, h, w = row["shape"]
        n = _two_images_if_one_pixel(n, h, w)
        sl = row["slice_len"] if row["slices"] > 1 else 0
        kernel = ("k_conv1x1<1,", f",ks{row['slices']}>") if row["slices"] > 1 else ("k_conv1x1<",)
        out.append(_cna_case("pointwise", _shape_id((n,) + row["shape"][1:]), (n, cin, h, w), (cout, cin, 1, 1), cout, 1, 1, CNA_EPILOGUES[(i + 2) % 4],
                             9810 + cin, kernel, slice_len=sl, note=row["why"]))
    return out


def _avgpool_cases():
    out = []
    for (planes, h, w, oh, ow), kernel in T.AVGPOOL:
        if planes == 300 or h * w == 1:
            continue  # the same kernel and window as the 5-plane rows; a 1 x 1 plane is a copy, which cannot overflow
        if oh * ow == 1:
            planes = max(planes, 4)  # one output per plane: the pair and the lone Inf take a plane each and leave half
        def make(planes=planes, h=h, w=w):
            return {"x": philox_f32(9500 + h * w + planes, (planes, h, w)) * 2 - 1}

        def torch_ref(d, oh=oh, ow=ow):
            import torch
            return torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(np.array(d["x"])), (oh, ow)).numpy()
        out.append(Case("avgpool", _shape_id((planes, h, w, oh, ow)), make, lambda d, oh=oh, ow=ow: ref.adaptive_avgpool(d["x"], oh, ow),
                        dict(op="avgpool", in_shape=(planes, h, w), out=(oh, ow)), {"x": "x"}, kernel, torch_ref=torch_ref, call=dict(out=(oh, ow))))
    return out


# ---- generic conv: F.conv2d_bias_act over CONV2D, implicit and columns forms; F.conv2d_affine_act ------------------------------------
def _conv2d_cases():
    out = []
    for i, row in enumerate(T.CONV2D):
        n, cin, cout, h, w = row["shape"]
        k, stride, pad, dil, groups = row["k"], row["stride"], row["pad"], row["dil"], row["groups"]
        n = _two_images_if_one_pixel(n, *S.conv_out_hw(h, w, k, stride, pad, dil))
        for columns in (False, True):
            bias, act = (i + columns) % 2 == 0, ("relu" if i % 2 else None)

            def make(row=row, bias=bias, n=n):
                _, cin, cout, h, w = row["shape"]
                k, groups = row["k"], row["groups"]
                return {"x": philox_f32(10000 + cin + h, (n, cin, h, w)) * 2 - 1, "w": (philox_f32(10001 + cout, (cout, cin // groups, k[0], k[1])) - 0.5) * 0.5,
                        "b": (philox_f32(10002 + w, (cout,)) - 0.5) if bias else None}
            geometry = dict(op="conv", in_shape=(n, cin, h, w), cout=cout, k=k, stride=stride, pad=pad, dil=dil, groups=groups)
            kw = dict(stride=stride, padding=pad, dilation=dil, groups=groups)
            out.append(Case("conv2d", _shape_id((n,) + row["shape"][1:]) + f",k{k[0]}x{k[1]},g{groups}," + ("columns" if columns else "implicit"), make,
                            lambda d, kw=kw, act=act: ref.conv2d_bias_act(d["x"], d["w"], d["b"], act=act, **kw), geometry,
                            {"x": "x", "w": "w", "b": "out"}, ("k_conv1x1<",) if columns else ("k_conv_igemm<", "implicit"),
                            torch_ref=lambda d, kw=kw, act=act: _torch_conv(d["x"], d["w"], d["b"], relu=act == "relu", **kw),
                            call=dict(activation=act, **kw), extras=[("b", (cout - 1,), S.NAN)] if bias else [],
                            switches={"CONV2D_SMALL_LAUNCH_WORKSPACE": columns, "CONV2D_COLUMNS_WORKSPACE": False}, note=row["why"]))
    return out


def _conv2d_affine_cases():
    """F.conv2d_affine_act: tests/test_gpu_resnet.py places NaN and Inf; here the locality check and the two range runs, on
    ResNet's three geometries at small sizes (7 x 7 stride 2 stem, 3 x 3, 1 x 1 stride 2 downsample)."""
    out = []
    for (shape, cout, k, stride, pad, ep) in [((2, 3, 13, 14), 9, 7, 2, 3, (False, 2, "relu", False)), ((1, 5, 9, 7), 33, 3, 1, 1, (True, 1, None, True)),
                                              ((2, 8, 7, 9), 12, 1, 2, 0, (False, 1, "relu", True))]:
        n, cin, h, w = shape
        bias, affine, act, residual = ep
        oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1

        def make(shape=shape, cout=cout, k=k, ep=ep, oh=oh, ow=ow):
            n, cin, h, w = shape
            bias, affine, act, residual = ep
            seed = 10300 + k
            return {"x": philox_f32(seed, shape) - 0.5, "w": (philox_f32(seed + 7, (cout, cin, k, k)) - 0.5) * 0.4,
                    "bias": (philox_f32(seed + 1, (cout,)) - 0.5) if bias else None, "alpha": philox_f32(seed + 2, (cout,)) + 0.5,
                    "beta": philox_f32(seed + 3, (cout,)) - 0.5, "residual": (philox_f32(seed + 4, (n, cout, oh, ow)) - 0.5) if residual else None}
        geometry = dict(op="conv", in_shape=shape, cout=cout, k=(k, k), stride=(stride, stride), pad=(pad, pad), dil=(1, 1), groups=1)
        out.append(Case("conv2d_affine", _shape_id(shape) + f",k{k},s{stride}", make,
                        lambda d, stride=stride, pad=pad, affine=affine, act=act: ref.conv2d_affine_act(d["x"], d["w"], d["bias"], d["alpha"], d["beta"],
                                                                                                        d["residual"], stride, pad, 1, affine, act),
                        geometry, {"x": "x", "w": "w", "bias": "out", "beta": "out", "residual": "out", "alpha": None}, ("k_conv_igemm_full<", "implicit"),
                        call=dict(stride=stride, padding=pad, affine=AFFINE_NAMES[affine], activation=act),
                        switches={"CONV2D_SMALL_LAUNCH_WORKSPACE": False, "CONV2D_COLUMNS_WORKSPACE": False}))
    return out


# ---- the two transposed convs: F.conv_transpose2d_bias_act, kernel 2 stride 2 and kernel 4 stride 2 padding 1 -------------------------
def _transpose_cases():
    from tests import _keypoint_ref as KR, _mask_ref as MR
    out = []
    # (k, n, cin, h, w, cout): the shapes of tests/test_gpu_mask.py and tests/test_gpu_keypoint.py that are a few workgroups, one of
    # them K-sliced (F.conv1x1_k_slices(1, 256, 6, 5, 4 * 5) is asserted by the host test), odd widths (the scalar store) and even
    for (k, n, cin, h, w, cout, bias, act) in [(2, 3, 40, 7, 7, 5, True, "relu"), (2, 2, 3, 5, 8, 1, False, None), (2, 1, 512, 7, 7, 8, True, None),
                                               (4, 2, 8, 5, 7, 3, True, None), (4, 4, 4, 1, 1, 1, False, "relu"), (4, 1, 13, 6, 8, 17, True, "relu")]:
        pad = 0 if k == 2 else 1

        def make(k=k, n=n, cin=cin, h=h, w=w, cout=cout, bias=bias):
            return {"x": philox_f32(9720 + cin + h, (n, cin, h, w)) * 2 - 1,
                    "w": (philox_f32(9721 + cin + cout, (cin, cout, k, k)) * 2 - 1) * np.float32(2.0 / np.sqrt(cin)),
                    "b": (philox_f32(9722 + cout, (cout,)) * 2 - 1) if bias else None}

        def torch_ref(d, pad=pad, act=act):
            import torch
            t = lambda a: None if a is None else torch.from_numpy(np.array(a))  # noqa: E731
            y = torch.nn.functional.conv_transpose2d(t(d["x"]), t(d["w"]), t(d["b"]), stride=2, padding=pad)
            return (torch.relu(y) if act == "relu" else y).numpy()
        oracle = ((lambda d, act=act: MR.oracle_conv_transpose(d["x"], d["w"], d["b"], act)) if k == 2 else
                  (lambda d, act=act: KR.oracle_conv_transpose4(d["x"], d["w"], d["b"], act)))
        out.append(Case(f"transpose{k}x{k}", _shape_id((n, cin, h, w, cout)) + f",bias={int(bias)},{act or 'none'}", make, oracle,
                        dict(op="transpose", in_shape=(n, cin, h, w), cout=cout, k=k, stride=2, pad=pad), {"x": "x", "w": "w", "b": "out"},
                        ("k_conv1x1_ct<",) if k == 2 else ("k_conv_igemm_tr<",), torch_ref=torch_ref, call=dict(activation=act, padding=pad),
                        extras=[("b", (cout - 1,), S.NAN)] if bias else []))
    return out


# ---- deformable conv: ops.deform_conv2d over DEFORM; NaN / Inf in x and in the mask, finite offsets --------------------------------------
def _deform_cases():
    out = []
    for row in T.DEFORM:
        n, cin, cout, h, w = row["shape"]
        k, stride, pad, dil, groups, og = row["k"], row["stride"], row["pad"], row["dil"], row["groups"], row["og"]
        oh, ow = S.conv_out_hw(h, w, k, stride, pad, dil)
        n = _two_images_if_one_pixel(n, oh, ow)
        for columns in ((True,) if row["needs"] == 1 else (False, True)):
            def make(row=row, n=n, oh=oh, ow=ow):
                _, cin, cout, h, w = row["shape"]
                k, groups, og = row["k"], row["groups"], row["og"]
                rng = np.random.Generator(np.random.Philox(10100 + cin * 7 + h))
                x = rng.random((n, cin, h, w), dtype=np.float32) * 2 - 1
                off = (rng.standard_normal((n, og * 2 * k[0] * k[1], oh, ow)) * row["scale"]).astype(np.float32)
                mask = rng.random((n, og * k[0] * k[1], oh, ow), dtype=np.float32) if row["mask"] else None
                wt = ((rng.random((cout, cin // groups, k[0], k[1]), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
                b = (rng.random(cout, dtype=np.float32) - 0.5) if row["bias"] else None
                if row["far"]:  # samples far outside the image and outside the staged window: exactly 0
                    off[0, 0, oh // 2, ow // 2], off[0, 1, oh // 2, ow // 2] = 1000.0, -1000.0
                    off[n - 1, 2 * k[0] * k[1] * og - 1, oh - 1, ow - 1] = -40.0
                return {"x": x, "offset": off, "w": wt, "b": b, "mask": mask}
            kw = dict(stride=stride, padding=pad, dilation=dil)
            case = Case("deform", _shape_id((n,) + row["shape"][1:]) + f",k{k[0]}x{k[1]},og{og}," + ("columns" if columns else "fused"), make,
                        lambda d, kw=kw: ref.deform_conv2d(d["x"], d["offset"], d["w"], d["b"], mask=d["mask"], **kw),
                        None, {"x": "x", "w": "w", "b": "out"}, ("k_conv1x1<",) if columns else ("k_deform_fused<",), call=dict(columns=columns, **kw),
                        extras=([("mask", (n - 1, 0, oh - 1, ow - 1), S.NAN), ("mask", (0, og * k[0] * k[1] - 1, 0, 0), S.PINF)] if row["mask"] else [])
                        + ([("b", (cout - 1,), S.NINF)] if row["bias"] else []), note=row["why"])
            case.geometry = dict(op="deform", in_shape=(n, cin, h, w), cout=cout, k=k, stride=stride, pad=pad, dil=dil, groups=groups, og=og,
                                 offset=case.clean["offset"])
            out.append(case)
    return out


# ---- the fused InvertedResidual block: F.inverted_residual over INVRES ---------------------------------------------------------------------
INVRES_NAMES = ["w_expand", "a1", "b1", "w_dw", "a2", "b2", "w_project", "a3", "b3"]


@functools.lru_cache(maxsize=None)
def invres_layer(block):
    """The block of tests/test_gpu_layer_guard_bands.py::test_inverted_residual: seeded weights, randomised frozen norms."""
    import torch
    from cpu_vision_amd.mobilenet import FrozenBatchNorm2d, InvertedResidual
    from tests._util import randomize_norms
    cin, hidden, cout, side, stride = block
    torch.manual_seed(cin * 7 + cout)
    layer = InvertedResidual(cin, cout, stride, hidden // cin, norm_layer=FrozenBatchNorm2d).eval()
    randomize_norms(layer, cin + cout + side)
    return layer


def invres_params(layer, cin, hidden, cout):
    """{name: numpy array or None} of the nine parameter tensors F.inverted_residual takes."""
    blocks = list(layer.conv)
    p = {n: None for n in INVRES_NAMES}
    if hidden != cin:
        p["w_expand"] = blocks[0][0].weight.detach().reshape(hidden, cin).numpy().copy()
        p["a1"], p["b1"] = (t.numpy().copy() for t in blocks[0][1].folded())
    p["w_dw"] = blocks[-3][0].weight.detach().reshape(hidden, 1, 3, 3).numpy().copy()
    p["a2"], p["b2"] = (t.numpy().copy() for t in blocks[-3][1].folded())
    p["w_project"] = blocks[-2].weight.detach().reshape(cout, hidden, 1, 1).numpy().copy()
    p["a3"], p["b3"] = (t.numpy().copy() for t in blocks[-1].folded())
    return p


def invres_oracle(block, d):
    """tests/_util.oracle_inverted_residual on a copy of the block that carries d's norm terms (the range runs scale b1, b2, b3
    and w_project; every other parameter is the block's own)."""
    import copy
    import torch
    from tests._util import oracle_inverted_residual
    cin, hidden, cout, side, stride = block
    layer = copy.deepcopy(invres_layer(block))
    blocks = list(layer.conv)
    norms = ([blocks[0][1]] if hidden != cin else []) + [blocks[-3][1], blocks[-1]]
    names = ([("a1", "b1")] if hidden != cin else []) + [("a2", "b2"), ("a3", "b3")]
    for norm, (a, b) in zip(norms, names):
        # FrozenBatchNorm2d folds to alpha = weight * rsqrt(var + eps), beta = bias - mean * alpha: mean 0, var 1 - eps, weight =
        # alpha, bias = beta restate given (alpha, beta) exactly when rsqrt(1) == 1
        a0, b0 = norm.folded()
        if np.array_equal(a0.numpy(), d[a]) and np.array_equal(b0.numpy(), d[b]):
            continue
        with torch.no_grad():
            norm.running_mean.zero_()
            norm.running_var.fill_(1.0 - norm.eps)
            norm.weight.copy_(torch.from_numpy(np.array(d[a])))
            norm.bias.copy_(torch.from_numpy(np.array(d[b])))
        a1, b1 = norm.folded()
        assert np.array_equal(a1.numpy(), d[a]) and np.array_equal(b1.numpy(), d[b]), "the folded norm does not restate (alpha, beta)"
    with torch.no_grad():
        blocks[-2].weight.copy_(torch.from_numpy(np.array(d["w_project"])))
    return oracle_inverted_residual(ref, layer, np.ascontiguousarray(d["x"]))


def _invres_cases():
    """Batch 1 and the row's next batch (two images per region at 7 pixels).  x alone is poisoned: it is the expansion's input,
    and the residual.  ReLU6 sits between the three convolutions, so the range runs cannot scale x by 2^+-100 and keep the block's
    arithmetic: the subnormal run scales x, b1, b2 and b3 alike (every intermediate is subnormal, ReLU6 passes them), the overflow
    run scales the projection -- w_project and b3 -- which is where a sum can overflow behind a ReLU6."""
    out = []
    for row in T.INVRES:
        cin, hidden, cout, side, stride = row["block"]
        batches = sorted(b for b in row["plans"] if b <= 3)[:2]
        for n in batches:
            def make(row=row, n=n):
                cin, hidden, cout, side, stride = row["block"]
                d = invres_params(invres_layer(row["block"]), cin, hidden, cout)
                d["x"] = philox_f32(10200 + n + side, (n, cin, side, side)) * 2 - 1
                return d
            residual = stride == 1 and cin == cout
            roles = {"subnormal": {"x": "x", "b1": "out", "b2": "out", "b3": "out"}, "overflow": {"x": "x", "w_project": "w", "b3": "out"}}
            out.append(Case("invres", "-".join(map(str, row["block"])) + f",n{n}", make, lambda d, block=row["block"]: invres_oracle(block, d),
                            dict(op="conv", in_shape=(n, cin, side, side), cout=cout, k=(3, 3), stride=(stride, stride), pad=(1, 1), dil=(1, 1), groups=1),
                            roles, (row["kernel"],), call=dict(residual=residual, stride=stride, affine="mul_add", slices=row["plans"][n][0]),
                            x_exp={"subnormal": 0, "overflow": 0}, note=row["why"], inf_reaches_output=residual))
    return out


# ---- the filters: blur, separable blur, Gaussian + Sobel, sharpness, the depthwise primitive, the frame-list entries -------------------
NP_DTYPE = {"float32": np.float32, "float64": np.float64, "float16": np.float16, "bfloat16": np.float32}


def _narrow(y32, dtype):
    """The float32 oracle's result rounded once to the storage type: what a half-precision image must equal
    (tests/test_gpu_parity.py::test_half_precision_storage_is_the_fp32_path_rounded_once)."""
    if isinstance(y32, tuple):
        return tuple(_narrow(v, dtype) for v in y32)
    if dtype == "bfloat16":
        import torch
        return torch.from_numpy(np.ascontiguousarray(y32)).to(torch.bfloat16).float().numpy()
    return y32.astype(NP_DTYPE[dtype])


def _k1d(k, sigma=None, dtype="float32"):
    import torch
    from cpu_vision_amd import functional as F
    sigma = k * 0.15 + 0.35 if sigma is None else sigma  # gaussian_blur's default, in its own expression
    return F._get_gaussian_kernel1d(k, sigma, torch.float64 if dtype == "float64" else torch.float32).numpy()


def _uses_separable(kx, ky, shape, dtype):
    import torch
    from cpu_vision_amd._filters import _use_separable
    return bool(_use_separable(kx, ky, torch.empty(shape, dtype=getattr(torch, dtype))))


def _is_2d_kernel(dtype):
    head = "k_dwtile<" + ("f32" if dtype == "float32" else "f16/bf16") + ","
    return lambda k: k.startswith(head) or (dtype == "float32" and k == "k_dw3x3")


def _is_separable_kernel(kx, ky, h, w):
    """tests/test_gpu_filter_guard_bands.py::_expect_separable_f32 with aligned pointers."""
    if kx <= 7 and ky <= 7 and w % 4 == 0 and w >= 8 and h >= 8:
        return lambda k: k == f"k_sepfast<{max(kx, ky, 3)},blur>"
    if (kx > 7 or ky > 7) and w >= 8:
        return lambda k: k == "k_sepstream"
    return lambda k: k == "k_separable"


def _image(seed, shape, dtype):
    x = philox_f32(seed, shape).astype(NP_DTYPE[dtype])
    if dtype == "bfloat16":
        import torch
        x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    return x


FILTER_H = 13  # a 23-tap column needs 11 < h rows to reflect


def _blur_case(op, side, w, dtype, frames=False):
    """F.gaussian_blur_image / F.separable_gaussian_blur / F.gaussian_blur_frames at one side, width and storage type.  A Gaussian
    is a convex combination: finite inputs cannot overflow it, so there is no overflow run."""
    shape = (4, 1, FILTER_H, w) if frames else (4, FILTER_H, w)  # four planes: a 23 x 23 window covers most of one
    separable = op == "separable" or _uses_separable(side, side, shape, dtype)
    if dtype == "float64":
        separable = False
    tx = _k1d(side, dtype=dtype)

    def oracle(d):
        if dtype == "float64":
            return ref.gaussian_blur_f64(d["x"], tx, tx)
        fn = ref.separable_blur if separable else ref.gaussian_blur
        return _narrow(fn(d["x"].astype(np.float32), tx, tx), dtype)
    if dtype == "float64":
        kernel = lambda k: k.startswith("k_dwf64<")  # noqa: E731
    elif separable:
        kernel = _is_separable_kernel(side, side, FILTER_H, w)
    else:
        kernel = _is_2d_kernel(dtype)
    name = {"blur": "blur", "separable": "sepblur"}[op] + ("_v" if frames else "")
    return Case(name, f"{side}x{side},w{w},{dtype}", lambda: {"x": _image(11000 + side + w, shape, dtype)}, oracle,
                dict(op="filter", in_shape=shape, k=(side, side), border="reflect"), {"x": "x"}, kernel, plan={"radius": (side // 2, side // 2)},
                call=dict(kernel_size=[side, side], frames=frames), dtype=dtype, overflow=False)


def _filter_cases():
    out = []
    for side in (3, 5, 9, 11, 23):
        for w in (5, 17, 257, 260):
            if side // 2 < w:  # ATen's reflection_pad2d refuses the others
                out.append(_blur_case("blur", side, w, "float32"))
    out += [_blur_case("blur", s_, w, "float64") for s_, w in ((3, 17), (9, 260), (23, 257))]
    out += [_blur_case("blur", s_, w, "float16") for s_, w in ((5, 17), (11, 257), (23, 260), (3, 5))]
    out += [_blur_case("blur", s_, w, "bfloat16") for s_, w in ((3, 260), (9, 17), (23, 257), (5, 5))]
    out += [_blur_case("separable", s_, w, "float32") for s_, w in ((3, 5), (5, 260), (9, 17), (11, 257), (23, 260))]
    out += [_blur_case("separable", 9, 260, "float16"), _blur_case("separable", 5, 17, "bfloat16")]
    out += [_blur_case("blur", 5, 260, "float32", frames=True), _blur_case("blur", 9, 17, "float32", frames=True)]
    # the primitive: signed taps (a sum can overflow), the three borders
    for border, code in (("reflect", ref.BORDER_REFLECT), ("zero", ref.BORDER_ZERO), ("valid", ref.BORDER_VALID)):
        for (ky, kx), w, dtype in (((3, 3), 17, "float32"), ((5, 3), 260, "float32"), ((9, 9), 257, "float32"), ((11, 11), 17, "float32"),
                                   ((3, 5), 17, "float64"), ((23, 23), 260, "float32")):
            shape = (2, 25 if ky == 23 else FILTER_H, w)

            def make(ky=ky, kx=kx, w=w, dtype=dtype, shape=shape):
                return {"x": _image(11500 + w + ky, shape, dtype) - NP_DTYPE[dtype](0.5),
                        "w": ((philox_f32(11501 + ky * kx, (ky, kx)) - 0.5) * 0.5).astype(NP_DTYPE[dtype])}
            fn = ref.depthwise_conv2d_f64 if dtype == "float64" else ref.depthwise_conv2d
            out.append(Case("depthwise_conv2d", f"{ky}x{kx},w{w},{border},{dtype}", make, lambda d, fn=fn, code=code: fn(d["x"], d["w"], code),
                            dict(op="filter", in_shape=shape, k=(ky, kx), border=border), {"x": "x", "w": "w"},
                            (lambda k: k.startswith("k_dwf64<")) if dtype == "float64" else _is_2d_kernel(dtype),
                            plan={"radius": (ky // 2, kx // 2)}, call=dict(border=border), dtype=dtype))
    # Gaussian, then Sobel of the blurred image: two outputs, signed taps
    for side, w in ((3, 17), (5, 260), (11, 257), (3, 5)):
        shape = (2, FILTER_H, w)
        tx = _k1d(side)
        out.append(Case("gaussian_sobel", f"{side}x{side},w{w}", lambda side=side, w=w, shape=shape: {"x": _image(11700 + side + w, shape, "float32")},
                        lambda d, tx=tx: ref.gaussian_sobel(d["x"], tx, tx),
                        dict(op="filter", in_shape=shape, k=(side, side), border="reflect", then=(3, 3)), {"x": "x"},
                        lambda k: k == "k_separable" or (k.startswith("k_sepfast<") and k.endswith(",sobel>")),
                        plan={"radius": (side // 2, side // 2)}, call=dict(kernel_size=[side, side])))
    # sharpness: clamps to [0, 1], so an Inf ends as 0 or 1 and nothing overflows
    for w, dtype, frames in ((5, "float32", False), (17, "float32", False), (260, "float32", False), (257, "float64", False), (17, "float16", False),
                             (260, "bfloat16", False), (17, "float32", True)):
        shape = (3, 3, 9, w) if frames else (2, 3, 9, w)

        def oracle(d, dtype=dtype):
            if dtype == "float64":
                return ref.adjust_sharpness_f64(d["x"], 1.7)
            return _narrow(ref.adjust_sharpness(d["x"].astype(np.float32), 1.7), dtype)
        out.append(Case("sharpness" + ("_v" if frames else ""), f"w{w},{dtype}", lambda w=w, dtype=dtype, shape=shape: {"x": _image(11800 + w, shape, dtype)},
                        oracle, dict(op="sharpness", in_shape=shape), {"x": "x"}, "k_sharp_f64" if dtype == "float64" else "k_dw3x3", call=dict(factor=1.7, frames=frames),
                        dtype=dtype, overflow=False, inf_reaches_output=False))
    return out


FILTER_CASES = _filter_cases()

# ---- sampling: F.affine / rotate / perspective, F.elastic (bilinear and nearest, float32), F1.resize in both forms ---------------------
def _unnormalize(g, size):
    """grid_sample's source pixel coordinate of a normalised one, align_corners=False, in float32."""
    return ((np.asarray(g, np.float32) + np.float32(1)) * np.float32(size) - np.float32(1)) / np.float32(2)


def _sampling_cases():
    """The expected values are the reference's own composition (the grid builders, torch's CPU grid_sample, the fill blend):
    tests/test_gpu_warp.py and tests/test_gpu_elastic.py restate it, exact on AVX2 hosts.  Bilinear interpolation is a convex
    combination: no overflow run.  `perspective_pole`: the denominator c6 x + c7 y + 1 is 0 along a column inside the output, so
    source coordinates are +-Inf or NaN there (torch: a bilinear sample is NaN, a nearest one reads nothing and gives 0)."""
    import torch
    from cpu_vision_amd import functional as F
    from tests import test_gpu_elastic as TE, test_gpu_warp as TW
    out = []
    n, c, h, w = 2, 3, 11, 14
    shape = (n, c, h, w)
    start, end = [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], [[1, 2], [w - 3, 1], [w - 2, h - 2], [2, h - 1]]
    coeffs = F._get_perspective_coeffs(start, end)
    pole = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0 / (w - 1.5), 0.0]  # 1 - x / (w - 1.5) = 0 at the centre of column w - 2
    field = ((torch.rand(1, h, w, 2, generator=torch.Generator().manual_seed(77)) - 0.5) * 0.6)
    t = lambda a: torch.from_numpy(np.array(a))  # noqa: E731

    def affine_grid(matrix, ow, oh):
        theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
        return TW._affine_grid(theta, w=w, h=h, ow=ow, oh=oh)[0].numpy()

    ops = {
        "affine": (dict(angle=12.5, translate=[3, -2], scale=0.85, shear=[10.0, -4.0]),
                   lambda x, mode: TW.ref_affine(x, 12.5, [3, -2], 0.85, [10.0, -4.0], mode=mode),
                   lambda: affine_grid(F._get_inverse_affine_matrix([0.0, 0.0], 12.5, [3.0, -2.0], 0.85, [10.0, -4.0]), w, h)),
        "rotate": (dict(angle=30.0), lambda x, mode: TW.ref_rotate(x, 30.0, mode=mode),
                   lambda: affine_grid(F._get_inverse_affine_matrix([0.0, 0.0], -30.0, [0.0, 0.0], 1.0, [0.0, 0.0]), w, h)),
        "perspective": (dict(startpoints=start, endpoints=end), lambda x, mode: TW.ref_perspective(x, coeffs, mode=mode),
                        lambda: TW._perspective_grid(coeffs, ow=w, oh=h, dtype=torch.float32)[0].numpy()),
        "perspective_pole": (dict(startpoints=None, endpoints=None, coefficients=pole), lambda x, mode: TW.ref_perspective(x, pole, mode=mode),
                             lambda: TW._perspective_grid(pole, ow=w, oh=h, dtype=torch.float32)[0].numpy()),
        "elastic": (dict(), lambda x, mode: TE.ref_elastic_image(x, field, mode=mode),
                    lambda: (torch.stack(torch.meshgrid(torch.linspace((-h + 1) / h, (h - 1) / h, h), torch.linspace((-w + 1) / w, (w - 1) / w, w),
                                                        indexing="ij")[::-1], -1) + field[0]).numpy()),
    }
    for name, (args, reference, grid) in ops.items():
        for mode in ("bilinear", "nearest"):
            g = grid()
            geometry = dict(op="sample", in_shape=shape, ix=_unnormalize(g[..., 0], w), iy=_unnormalize(g[..., 1], h), mode=mode)
            oracle = lambda d, reference=reference, mode=mode: reference(t(d["x"]), mode).numpy()  # noqa: E731
            out.append(Case("elastic" if name == "elastic" else "warp", f"{name},{mode}", lambda: {"x": philox_f32(12000, shape)}, oracle, geometry,
                            {"x": "x"}, ("k_elastic<f32," + mode,) if name == "elastic" else ("k_warp<f32",), torch_ref=oracle,
                            call=dict(op=name.split("_")[0], args=args, mode=mode, field=field.numpy()), overflow=False))
    # F1.resize, antialiased bilinear: one fused kernel up to scale 7, the width pass to a workspace + height pass beyond (or forced)
    for rshape, size, two, kernel in (((2, 3, 20, 30), 8, False, "k_resize_fused"), ((2, 3, 60, 72), 8, False, "k_resize_h"),
                                      ((2, 3, 20, 30), 8, True, "k_resize_h"), ((2, 3, 9, 13), 12, False, "k_resize_fused")):
        oh, ow = ref.resized_output_size(rshape[-2], rshape[-1], [size])

        def torch_ref(d, oh=oh, ow=ow):
            return torch.nn.functional.interpolate(t(d["x"]), size=(oh, ow), mode="bilinear", align_corners=False, antialias=True).numpy()
        out.append(Case("resize", _shape_id(rshape) + f",to{size}" + (",two_kernels" if two else ""), lambda rshape=rshape: {"x": philox_f32(12100 + rshape[-1], rshape)},
                        lambda d, size=size: ref.resize(d["x"], [size]), dict(op="resize", in_shape=rshape, out=(oh, ow)), {"x": "x"}, (kernel,),
                        env={"MV_RESIZE_TWO_KERNELS": "1"} if two else None, torch_ref=torch_ref, call=dict(size=[size]), overflow=False))
    return out


# ---- colour: the float32 chain (brightness, contrast, saturation, hue), autocontrast, normalize; values outside [0, 1] ---------------------
def _color_cases():
    """Expected values: the reference's own torch expressions (tests/_color_ref.py, tests/_autoaug_ref.py).  The chain ops and
    autocontrast clamp to [0, 1]: an Inf ends at a bound (or as NaN through Inf - Inf, Inf / Inf) and nothing overflows;
    normalize does not clamp.  F.to_float_normalize takes uint8 pixels and host-side means: it has no cell that could hold a NaN;
    its kernel, k_to_float_normalize, is the one F.normalize runs here on float32 pixels."""
    import torch
    from tests import _autoaug_ref as AR, _color_ref as CR
    out = []
    shape = (4, 3, 6, 9)  # four images: the contrast mean spreads a cell over its whole image
    t = lambda a: torch.from_numpy(np.array(a))  # noqa: E731
    make = lambda: {"x": philox_f32(12200, shape) * 2 - np.float32(0.5)}  # noqa: E731  [-0.5, 1.5): values outside [0, 1]
    chains = {"brightness": ([("brightness", 0.6)], "pointwise"),  # 0.6 x 1.5 < 1: no clean output sits at the bound an Inf ends at
               "saturation": ([("saturation", 0.6)], "pixel"), "hue": ([("hue", 0.2)], "pixel"),
              "contrast": ([("contrast", 1.4)], "image"),
              "jitter": ([("contrast", 0.7), ("brightness", 0.8), ("saturation", 1.5), ("hue", -0.1)], "image")}
    def chain(d, ops):
        """tests/_color_ref.ref_chain with the library's rule for a pixel without a hue (include/mi355vision.h): a NaN or infinite
        channel going into adjust_hue gives three NaNs.  (torch picks the sector from int(NaN) -- INT_MIN on x86, 0 elsewhere --
        and so leaves an Inf in one host-dependent channel.)"""
        x = t(d["x"])
        for name, f in ops:
            y = CR.REF_OPS[name](x, f)
            if name == "hue":
                y = torch.where(torch.isfinite(x).all(dim=-3, keepdim=True), y, torch.full_like(y, float("nan")))
            x = y
        return x.numpy()
    for name, (ops, reach) in chains.items():
        out.append(Case("color", name, make, lambda d, ops=ops: chain(d, ops), dict(op=reach, in_shape=shape), {"x": "x"},
                        ("k_color<f32,c3",), call=dict(ops=ops), overflow=False, inf_reaches_output=False))
    out.append(Case("autocontrast", "f32", make, lambda d: AR.ref_autocontrast(t(d["x"])).numpy(), dict(op="plane", in_shape=shape), {"x": "x"},
                    ("k_autocontrast<f32",), overflow=False, inf_reaches_output=False,
                    subnormal_outputs=False))
    mean, std = [0.4, 0.5, 0.3], [0.2, 0.25, 0.3]
    out.append(Case("normalize", "f32", make, lambda d: ref.to_float_normalize(d["x"], mean, std), dict(op="pointwise", in_shape=shape), {"x": "x"},
                    "k_to_float_normalize", torch_ref=lambda d: ((t(d["x"]) - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)).numpy(),
                    call=dict(mean=mean, std=std), subnormal_outputs=False))
    return out


SAMPLING_CASES = _sampling_cases()
COLOR_CASES = _color_cases()

LAYER_CASES = (_conv3x3_cases() + _conv3x3_u8norm_cases() + _linear_cases() + _conv_norm_act_cases() + _avgpool_cases() + _conv2d_cases()
               + _conv2d_affine_cases() + _transpose_cases() + _deform_cases() + _invres_cases())
