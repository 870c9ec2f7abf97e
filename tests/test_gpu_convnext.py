"""ConvNeXt on the GPU (`-m gpu`): the depthwise 7x7 kernel, LayerNorm over the channels, the pointwise conv with the norm in its loads
and GELU in its epilogue, the block and the networks.  Every comparison is bit for bit -- NaN in equal places, == elsewhere -- against
oracle/ref.py (the convs) and the restatements of tests/_convnext_ref.py (LayerNorm's float64 sums, the erf GELU); the block at real K
and the network's logits are also held to the project's accuracy condition against a float64 evaluation.  (tests/test_convnext_host.py
shows that no GELU argument of these cases lies near a rounding tie of erf.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpu_vision_amd import _lib  # noqa: E402
from cpu_vision_amd import functional as F  # noqa: E402
from cpu_vision_amd import convnext as CN  # noqa: E402
from cpu_vision_amd.convnext import CNBlock, CNBlockConfig, ConvNeXt, convnext_tiny  # noqa: E402
from oracle import ref  # noqa: E402
from tests import _convnext_ref as R  # noqa: E402

NAN, INF = float("nan"), float("inf")


def _rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def _randn(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _offset_by_4_bytes(a):
    """The array on the device, starting 4 bytes past a 16-byte boundary."""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------------------------- depthwise 7x7
def _dw(x, w, bias=None, xd=None):
    got = F.dwconv7x7(_cuda(x) if xd is None else xd, _cuda(w), _cuda(bias))
    want = ref.conv2d_affine_act(x, w, bias, None, None, None, 1, 3, x.shape[1], 0, None)
    return got, want


SIZES = [(1, 1), (3, 3), (6, 6), (7, 7), (8, 8), (14, 14), (33, 31), (6, 64), (3, 260)]


def test_depthwise7x7_sizes_channels_batches():
    """Maps smaller than the window, one thread group per row and several, rows of whole quads; with and without bias."""
    rng = _rng(100)
    for h, w in SIZES:
        for c in (1, 3, 65):
            for n in (1, 2):
                x, wt, b = _randn(rng, (n, c, h, w)), _randn(rng, (c, 1, 7, 7), 0.3), _randn(rng, c)
                for bias in (None, b):
                    got, want = _dw(x, wt, bias)
                    rows, _ = R.dw7x7_plan(n, c, h, w)
                    assert _lib.last_kernel() == f"k_dwpc7x7<rows{rows}>", _lib.last_kernel()
                    R.same(got, want, f"dw7x7 {(n, c, h, w)} bias={bias is not None}")
    assert tuple(F.dwconv7x7(torch.empty((0, 4, 6, 6), device="cuda"), _cuda(_randn(rng, (4, 1, 7, 7)))).shape) == (0, 4, 6, 6)


def test_depthwise7x7_heights_around_the_strip_lengths():
    """A thread's strip is 8 output rows, 4 in launches of fewer than 16384 threads: heights 3, 4, 5 and 7, 8, 9 under both."""
    rng = _rng(110)
    for h in (3, 4, 5, 7, 8, 9):
        for (n, c, w), rows in (((1, 3, 9), 4), ((4, 65, 260), 8)):
            x, wt, b = _randn(rng, (n, c, h, w)), _randn(rng, (c, 1, 7, 7), 0.3), _randn(rng, c)
            got, want = _dw(x, wt, b)
            assert _lib.last_kernel() == f"k_dwpc7x7<rows{rows}>", (_lib.last_kernel(), n, c, h, w)
            R.same(got, want, f"dw7x7 {(n, c, h, w)}")


def test_depthwise7x7_x_at_a_4_byte_offset_gives_the_same_bits():
    rng = _rng(120)
    for shape in ((2, 3, 28, 28), (1, 5, 8, 64), (1, 2, 14, 14), (1, 2, 7, 7)):
        x, wt = _randn(rng, shape), _randn(rng, (shape[1], 1, 7, 7), 0.3)
        aligned, want = _dw(x, wt)
        shifted, _ = _dw(x, wt, xd=_offset_by_4_bytes(x))
        R.same(aligned, want, f"aligned {shape}")
        assert torch.equal(aligned, shifted)


@pytest.mark.parametrize("value", [NAN, INF])
def test_depthwise7x7_special_weights_reach_the_border_pixels(value):
    """A padding tap enters the chain as fmaf(w, +0, acc): a NaN or infinite weight at tap (0, 0) makes the outputs whose tap lies in
    the padding NaN (inf * 0) -- the top rows and left columns -- and no output of its channel finite; a special input value reaches
    its 49 windows only."""
    rng = _rng(130)
    n, c, h, w = 1, 3, 9, 10
    x, wt = _randn(rng, (n, c, h, w)), _randn(rng, (c, 1, 7, 7), 0.3) + 0.01
    wt[1, 0, 0, 0] = value
    got, want = _dw(x, wt, _randn(rng, c))
    R.same(got, want, "special weight")
    g = got.cpu().numpy()
    assert np.isnan(g[0, 1, :3]).all() and np.isnan(g[0, 1, :, :3]).all() and not np.isfinite(g[0, 1]).any()
    assert np.isfinite(g[0, 0]).all() and np.isfinite(g[0, 2]).all()
    x2, w2 = _randn(rng, (1, 2, 13, 14)), _randn(rng, (2, 1, 7, 7), 0.3) + 0.01
    x2[0, 1, 6, 9] = value
    got, want = _dw(x2, w2)
    R.same(got, want, "special value")
    mask = np.zeros((1, 2, 13, 14), bool)
    mask[0, 1, 3:10, 6:13] = True
    np.testing.assert_array_equal(~np.isfinite(got.cpu().numpy()), mask)


# ------------------------------------------------------------------------------------------------------------- LayerNorm
LN_PLANES = {1: (1, 1), 15: (3, 5), 16: (4, 4), 17: (1, 17), 49: (7, 7), 50: (5, 10), 300: (15, 20)}  # a workgroup covers 16 pixels


@pytest.mark.parametrize("c", [1, 2, 63, 64, 65, 96, 257])
def test_layer_norm2d_and_its_stats_against_the_restatement(c):
    rng = _rng(200 + c)
    for hw, (h, w) in LN_PLANES.items():
        for n in (1, 2):
            x = _randn(rng, (n, c, h, w)) + np.float32(0.5)
            x[n - 1, :, h - 1, w - 1] = 1.25  # a pixel with all channels equal
            g, b = _randn(rng, c) + np.float32(1.5), _randn(rng, c)
            mean, rstd = F.layer_norm2d_stats(_cuda(x), 1e-6)
            assert _lib.last_kernel() == "k_layer_norm2d<stats>" and tuple(mean.shape) == tuple(rstd.shape) == (n, h, w)
            want_mean, want_rstd = R.layer_norm2d_stats(x, 1e-6)
            R.same(mean, want_mean, f"mean {(n, c, h, w)}")
            R.same(rstd, want_rstd, f"rstd {(n, c, h, w)}")
            assert mean[n - 1, h - 1, w - 1].item() == 1.25 and rstd[n - 1, h - 1, w - 1].item() == np.float32(1 / np.sqrt(np.float64(np.float32(1e-6))))
            for wt, bs in ((g, b), (None, None), (g, None), (None, b)):
                got = F.layer_norm2d(_cuda(x), _cuda(wt), _cuda(bs), 1e-6)
                assert _lib.last_kernel() == "k_layer_norm2d<apply>"
                R.same(got, R.layer_norm2d_apply(x, want_mean, want_rstd, wt, bs), f"layer_norm2d {(n, c, h, w)} w={wt is not None} b={bs is not None}")
    assert tuple(F.layer_norm2d(torch.empty((0, c, 4, 4), device="cuda")).shape) == (0, c, 4, 4)


def test_layer_norm2d_eps_0_offsets_and_independence_of_the_place():
    rng = _rng(250)
    x = _randn(rng, (2, 5, 3, 3))
    x[1, :, 2, 1] = -3.0  # a constant pixel at eps = 0: rstd = +inf, the result 0 * inf = NaN
    mean, rstd = F.layer_norm2d_stats(_cuda(x), 0.0)
    wm, wr = R.layer_norm2d_stats(x, 0.0)
    R.same(mean, wm, "mean, eps 0")
    R.same(rstd, wr, "rstd, eps 0")
    assert rstd[1, 2, 1].item() == INF
    got = F.layer_norm2d(_cuda(x), eps=0.0)
    R.same(got, R.layer_norm2d(x, eps=0.0), "eps 0")
    assert bool(torch.isnan(got[1, :, 2, 1]).all()) and int(torch.isnan(got).sum()) == 5
    for shape in ((2, 7, 4, 4), (1, 96, 7, 7), (1, 3, 1, 1)):
        x = _randn(rng, shape)
        g, b = _randn(rng, shape[1]), _randn(rng, shape[1])
        a, s = F.layer_norm2d(_cuda(x), _cuda(g), _cuda(b)), F.layer_norm2d(_offset_by_4_bytes(x), _cuda(g), _cuda(b))
        assert torch.equal(a, s)
        R.same(a, R.layer_norm2d(x, g, b), f"offset {shape}")
        sa, ss = F.layer_norm2d_stats(_cuda(x)), F.layer_norm2d_stats(_offset_by_4_bytes(x))
        assert torch.equal(sa[0], ss[0]) and torch.equal(sa[1], ss[1])
    # one pixel's result at two places, in maps of different sizes and batches
    px = _randn(rng, 96)
    x1, x2 = _randn(rng, (1, 96, 1, 1)), _randn(rng, (3, 96, 5, 7))
    x1[0, :, 0, 0], x2[2, :, 4, 3] = px, px
    a, b = F.layer_norm2d(_cuda(x1)), F.layer_norm2d(_cuda(x2))
    assert torch.equal(a[0, :, 0, 0], b[2, :, 4, 3])
    # NaN / Inf stay in their pixel
    x = _randn(rng, (1, 4, 2, 3))
    x[0, 1, 0, 0], x[0, 2, 1, 2] = NAN, INF
    got = F.layer_norm2d(_cuda(x))
    R.same(got, R.layer_norm2d(x), "special values")
    bad = ~torch.isfinite(got.cpu())
    assert bool(bad[0, :, 0, 0].all()) and bool(bad[0, :, 1, 2].all()) and int(bad.sum()) == 8


# ------------------------------------------------------------------------------------------------------------- conv1x1_gelu
def _pw_check(i, shape, large):
    n, cin, cout, h, w = shape
    x, wt, b, lw, lb = R.pw_case(i, shape)
    xd, wd, bd, lwd, lbd = (_cuda(a) for a in (x, wt, b, lw, lb))
    hw = h * w
    what = f"conv1x1_gelu {shape}"
    # without the norm: the plain pointwise conv + bias + GELU
    plain = F.conv1x1_gelu(xd, wd, bd)
    assert _lib.last_kernel() == R.ln_kernel_name(n, cin, hw, cout, False), (_lib.last_kernel(), shape)
    # with the norm in the loads, against the materialised composition
    mean, rstd = F.layer_norm2d_stats(xd, 1e-6)
    fused = F.conv1x1_gelu(xd, wd, bd, norm=(mean, rstd, lwd, lbd))
    assert _lib.last_kernel() == R.ln_kernel_name(n, cin, hw, cout, True), (_lib.last_kernel(), shape)
    unfused = F.conv1x1_gelu(F.layer_norm2d(xd, lwd, lbd, 1e-6), wd, bd)
    R.same(fused, unfused, what + " fused == unfused")
    # against the reference (a large case: on a sample of its pixels; its plan is one chain per output)
    if large:
        assert R.pw_plan(n, cin, hw, cout)[2] == 1
        idx = R.sample_pixels(hw, i)
        xs, pick = x.reshape(n, cin, 1, hw)[:, :, :, idx], (lambda t: t.reshape(n, cout, 1, hw)[:, :, :, torch.from_numpy(idx).cuda()])
        sl = 0
    else:
        xs, pick, sl = x, (lambda t: t), None
    R.same(pick(plain), R.conv1x1_gelu(xs, wt, b, slice_len=sl), what + " plain")
    stats = R.layer_norm2d_stats(xs, 1e-6)
    R.same(pick(fused), R.conv1x1_gelu(xs, wt, b, norm=stats + (lw, lb), slice_len=sl), what + " norm")
    return xd, wd, bd, mean, rstd, lwd, lbd, xs, stats, pick, sl


@pytest.mark.parametrize("i", range(len(R.PW_SMALL)))
def test_conv1x1_gelu_small_shapes(i):
    """cin around the 32-row chunk, cout around 32 / 64 / 128, H W around the pixels of a workgroup, the K-slice instances, batch 2:
    fused == unfused bit for bit, both against the reference; also gelu=False, no bias, and LayerNorm terms left out."""
    shape = R.PW_SMALL[i]
    x, wt, b, lw, lb = R.pw_case(i, shape)
    xd, wd, bd, mean, rstd, lwd, lbd, xs, stats, pick, sl = _pw_check(i, shape, False)
    R.same(F.conv1x1_gelu(xd, wd, bd, gelu=False), R.conv1x1_gelu(x, wt, b, gelu_on=False), f"{shape} gelu=False")
    R.same(F.conv1x1_gelu(xd, wd.view(shape[2], shape[1], 1, 1), None, norm=(mean, rstd, None, lbd), gelu=False),
           R.conv1x1_gelu(x, wt, None, norm=stats + (None, lb), gelu_on=False), f"{shape} no bias, no ln weight, gelu=False")
    R.same(F.conv1x1_gelu(xd, wd, bd, norm=(mean, rstd, lwd, None), gelu=False),
           R.conv1x1_gelu(x, wt, b, norm=stats + (lw, None), gelu_on=False), f"{shape} no ln bias, gelu=False")


@pytest.mark.parametrize("i", range(len(R.PW_LARGE)))
def test_conv1x1_gelu_instances_with_several_pixel_tiles_per_wave(i):
    _pw_check(len(R.PW_SMALL) + i, R.PW_LARGE[i], True)


def test_conv1x1_gelu_special_values_and_empty_batches():
    """K = 1 and w = 1: the pre-activation values are x itself.  GELU(NaN) = NaN, GELU(+inf) = +inf, GELU(-inf) = NaN (-inf * 0): the
    formula's values.  NaN statistics reach their pixel only, in equal places with and without the fusion."""
    v = R.SPECIAL_GELU_VALUES
    got = F.conv1x1_gelu(_cuda(v.reshape(1, 1, 1, -1)), torch.ones((1, 1), device="cuda")).cpu().numpy().reshape(-1)
    R.same(got, R.gelu(v), "special values")
    assert np.isnan(got[0]) and got[1] == INF and np.isnan(got[2]) and got[8] == 30 and got[9] == 0
    rng = _rng(340)
    x, wt = _randn(rng, (2, 40, 3, 5)), _randn(rng, (24, 40), 0.3)
    x[0, 3, 1, 1], x[1, 7, 2, 4] = NAN, INF
    xd, wd = _cuda(x), _cuda(wt)
    mean, rstd = F.layer_norm2d_stats(xd)
    fused = F.conv1x1_gelu(xd, wd, norm=(mean, rstd, None, None))
    R.same(fused, F.conv1x1_gelu(F.layer_norm2d(xd), wd), "NaN in equal places")
    bad = torch.isnan(fused.cpu())
    assert bool(bad[0, :, 1, 1].all()) and bool(bad[1, :, 2, 4].all()) and int(bad.sum()) == 48
    assert tuple(F.conv1x1_gelu(torch.empty((0, 40, 3, 5), device="cuda"), wd).shape) == (0, 24, 3, 5)
    assert tuple(F.conv1x1_gelu(torch.empty((2, 40, 0, 5), device="cuda"), wd).shape) == (2, 24, 0, 5)


# ------------------------------------------------------------------------------------------------------------- CNBlock
def _device_block(cpu, dim):
    dev = CNBlock(dim, 1e-6, 0.0)
    dev.load_state_dict(cpu.state_dict(), strict=True)
    return dev.cuda().eval()


@pytest.mark.parametrize("dim,h,w", R.BLOCK_CASES)
def test_cnblock_stage_by_stage(dim, h, w, monkeypatch):
    """Each launch of the block against the stage-by-stage reference; the block's result equals the composition of public F calls, with
    the norm in the loads (four launches) and materialised (five)."""
    _, cpu = R.block_pair(dim, 40 + dim, CNBlock)
    dev = _device_block(cpu, dim)
    x = R.block_input(dim, h, w, 50 + dim)
    want = R.block_stages(cpu, x)
    conv, norm, fc1, fc2 = dev.block[0], dev.block[2], dev.block[3], dev.block[5]
    with torch.no_grad():
        xd = _cuda(x)
        hd = F.dwconv7x7(xd, conv.weight, conv.bias)
        mean, rstd = F.layer_norm2d_stats(hd, norm.eps)
        gd = F.conv1x1_gelu(hd, fc1.weight, fc1.bias, norm=(mean, rstd, norm.weight, norm.bias))
        out = F.conv_norm_act(gd, fc2.weight.view(dim, 4 * dim, 1, 1), fc2.bias, alpha=dev.layer_scale.reshape(dim),
                              beta=torch.zeros(dim, device="cuda"), residual=xd, affine="mul_add")
        R.same(hd, want[0], f"block {dim}: depthwise")
        R.same(mean, want[1][0], f"block {dim}: mean")
        R.same(rstd, want[1][1], f"block {dim}: rstd")
        R.same(gd, want[2], f"block {dim}: Linear + GELU")
        R.same(out, want[3], f"block {dim}: output")
        for fused in (True, False):
            monkeypatch.setattr(CN, "_use_fused", lambda d, px, f=fused: f)
            got = dev(xd)
            assert _lib.last_kernel().startswith("k_conv1x1<"), _lib.last_kernel()
            assert torch.equal(got, out), f"block {dim}: forward, fused={fused}"
    assert float(np.abs(want[3] - x).max()) > 0.05  # the branch is not scaled away
    with pytest.raises(RuntimeError, match="inference only"):
        dev.train()(xd)


def test_cnblock_accuracy_at_real_k():
    """One CNBlock at dim 768 on a 2 x 2 map, perturbed weights, layer_scale 1: the second Linear sums 3072 products per output.  The
    project's condition against the float64 replica: library error <= 2 x the float32 replica's error + 2^-22 max|f64|.  Measured, in
    units of 2^-24 max|f64|: see DESIGN.md 3.36."""
    dim = 768
    rep, cpu = R.block_pair(dim, 61, CNBlock, layer_scale=1.0, weight_factor=4.0)
    dev = _device_block(cpu, dim)
    x = torch.from_numpy(R.block_input(dim, 2, 2, 62))
    with torch.no_grad():
        got = dev(x.cuda()).cpu()
        t32 = rep(x.clone())
        f64 = rep.double()(x.double())
    scale = float(f64.abs().max())
    e_lib, e_t = float((got.double() - f64).abs().max()), float((t32.double() - f64).abs().max())
    branch = float((f64 - x.double()).abs().max())
    print(f"CNBlock dim 768 on 2 x 2: library {e_lib / scale * 2 ** 24:.2f}, torch float32 replica {e_t / scale * 2 ** 24:.2f} "
          f"(x 2^-24 max|f64| = {scale:.3g}); the branch's largest value {branch:.3g}; plan {F.conv1x1_k_slices(2, 4 * dim, 2, 2, dim)}")
    assert branch > 0.25 * scale  # the branch weighs as much as the input
    assert e_lib <= 2 * e_t + 2.0 ** -22 * scale


# ------------------------------------------------------------------------------------------------------------- networks
def _run_with_stages(dev, x):
    outs = []
    hooks = [m.register_forward_hook(lambda _m, _i, o: outs.append(o)) for m in dev.features]
    with torch.no_grad():
        logits = dev(_cuda(x))
    for hk in hooks:
        hk.remove()
    return outs, logits


def test_network_stage_by_stage_and_accuracy():
    """block_setting [(8, 16, 1), (16, 24, 2), (24, None, 1)], 7 classes, batch 2, 64 x 64: every features[i] and the logits bit for
    bit against the stage-by-stage reference; the logits against float64 within the project's condition (figures: DESIGN.md 3.36)."""
    builder = lambda **kw: ConvNeXt([CNBlockConfig(*r) for r in R.NET_ROWS], **kw)  # noqa: E731
    rep, cpu = R.net_pair(R.NET_ROWS, 31, builder)
    dev = builder(num_classes=7)
    dev.load_state_dict(rep.state_dict(), strict=True)  # a state dict of the replica, as it is
    dev = dev.cuda()
    x = R.block_input(3, 64, 64, 800)
    feats, want = R.forward_stages(cpu, x)
    outs, logits = _run_with_stages(dev, x)
    assert len(outs) == len(feats) == 6
    for i, (g, wnt) in enumerate(zip(outs, feats)):
        R.same(g, wnt, f"features[{i}]")
    R.same(logits, want, "logits")
    with torch.no_grad():
        t32 = rep(torch.from_numpy(x))
        f64 = rep.double()(torch.from_numpy(x).double())
    scale = float(f64.abs().max())
    e_lib, e_t = float((logits.cpu().double() - f64).abs().max()), float((t32.double() - f64).abs().max())
    print(f"ConvNeXt {R.NET_ROWS} logits: library {e_lib / scale * 2 ** 24:.2f}, torch float32 replica {e_t / scale * 2 ** 24:.2f} "
          f"(x 2^-24 max|f64| = {scale:.3g})")
    assert e_lib <= 2 * e_t + 2.0 ** -22 * scale


def test_convnext_tiny_logits():
    rep, cpu = R.net_pair("convnext_tiny", 33, convnext_tiny)
    dev = convnext_tiny(num_classes=7)
    dev.load_state_dict(rep.state_dict(), strict=True)
    dev = dev.cuda()
    x = R.block_input(3, 32, 32, 801)[:1]
    feats, want = R.forward_stages(cpu, x)
    outs, logits = _run_with_stages(dev, x)
    R.same(outs[-1], feats[-1], "convnext_tiny features")
    R.same(logits, want, "convnext_tiny logits")
    assert tuple(logits.shape) == (1, 7) and float(np.abs(want).max()) > 0
    with pytest.raises(RuntimeError, match="forward-only"):
        dev(_cuda(x).requires_grad_()).sum().backward()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_the_existing_surface_keeps_its_refusals():
    rng = _rng(900)
    x = _cuda(_randn(rng, (2, 5, 9, 7)))
    with pytest.raises(NotImplementedError, match="depthwise 3x3 and 5x5"):
        F.conv_norm_act(x, _cuda(_randn(rng, (5, 1, 7, 7))), groups=5)
    w1 = _cuda(_randn(rng, (4, 5, 1, 1)))
    with pytest.raises(ValueError, match="unknown activation 'gelu'"):
        F.conv_norm_act(x, w1, activation="gelu")
    with pytest.raises(ValueError, match="unknown activation"):
        F.dwconv_pointwise(x, _cuda(_randn(rng, (5, 1, 3, 3))), weight=w1, activation="gelu")
    with pytest.raises(ValueError, match="unknown activation"):
        F.conv1x1_upsample_add(x, w1, top=_cuda(_randn(rng, (2, 4, 5, 4))), activation="gelu")
    lib = _lib.load()
    y = torch.empty((2, 4, 9, 7), device="cuda")
    for act in (5, 7):  # Hardsigmoid's code and the pointwise family's internal GELU code
        rc = lib.mv_conv_norm_act_f32(2, x.data_ptr(), w1.data_ptr(), None, None, None, None, y.data_ptr(), 2, 5, 9, 7, 4, 1, 0, act, _lib.stream_ptr(x))
        assert rc == -1 and f"activation ({act})" in lib.mv_last_error().decode()
    rc = lib.mv_dwconv_norm_act_f32(x.data_ptr(), w1.data_ptr(), None, None, None, None, y.data_ptr(), 2, 5, 9, 7, 7, 1, 0, 0, _lib.stream_ptr(x))
    assert rc == -2 and "kernel 3 or 5" in lib.mv_last_error().decode()
    # without a norm and GELU the existing instances run, under the names they had
    F.conv_norm_act(_cuda(_randn(rng, (1, 72, 28, 28))), _cuda(_randn(rng, (40, 72, 1, 1))))
    assert _lib.last_kernel() == "k_conv1x1<1,2>", _lib.last_kernel()
